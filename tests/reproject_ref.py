"""The normative definition of the reprojection of a previous view's frame into a new camera view
(rt_reproject), restated in NumPy fp32. Only add, subtract, multiply, IEEE divide, floor and
comparisons, in the order written; no fused multiply-add; dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z.
Every operation has exactly one fp32 result, so the device output equals this in every bit.
A helper module of the reproject tests, not a test file."""
import numpy as np

from denoise_ref import to_u8_ref

F = np.float32
REASONS = ("object_range", "not_reusable", "position_nan", "behind", "outside", "tap_outside", "tap_object",
           "tap_nonfinite", "tap_normal", "tap_plane", "low_weight")


def dot(a, b):
    return ((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]).astype(F) + a[..., 2] * b[..., 2]).astype(F)


def view_constants(view):
    """a = p - c, w = cross(du, dv) (each product rounded, then the subtraction), aw = dot(a, w),
    iu = 1 / dot(du, du), iv = 1 / dot(dv, dv) - all fp32."""
    c, p, du, dv = (np.asarray(view[k], dtype=F) for k in ("center", "pixel00", "du", "dv"))
    a = (p - c).astype(F)
    w = np.array([F(du[1] * dv[2]) - F(du[2] * dv[1]),
                  F(du[2] * dv[0]) - F(du[0] * dv[2]),
                  F(du[0] * dv[1]) - F(du[1] * dv[0])], dtype=F)
    with np.errstate(all="ignore"):
        return {"c": c, "a": a, "du": du, "dv": dv, "w": w, "aw": dot(a, w), "iu": F(F(1) / dot(du, du)),
                "iv": F(F(1) / dot(dv, dv)), "width": int(view["width"]), "height": int(view["height"])}


def reusable_from_scene(scene):
    """reusable[o] = 1 iff object o's resolved material is lambert or light (material ids followed)."""
    by_id = {m["id"]: m["material"] for m in scene.get("materials", [])}
    out = []
    for ob in scene["objects"]:
        m = ob.get("material")
        while isinstance(m, str):
            m = by_id.get(m)
        out.append(1 if isinstance(m, dict) and m.get("type") in ("lambert", "light") else 0)
    return np.array(out, np.uint8)


def reproject_ref(prev_radiance, prev_view, prev_guides, normal, position, distance, object, reusable, region=None,
                  prev_region=None, radiance=None, px_samples=None, samples=None, normal_min=0.9, sigma_plane=0.01,
                  min_weight=0.25, history_samples=32.0, reasons=None):
    """Returns {"history": (H, W, 3), "weight": (H, W), "radiance": (H, W, 3) or None, "rgb": u8 or
    None} as full-frame arrays of the new frame; outside `region` history and weight are zero and
    radiance / rgb are the fresh frame and its u8. `reasons` (a dict) receives, per name in
    REASONS, how many region pixels (or taps) were rejected for it."""
    V = view_constants(prev_view)
    Wp, Hp = V["width"], V["height"]
    Hh, Ww = object.shape
    x0, y0, w, h = region or (0, 0, Ww, Hh)
    qx0, qy0, qw, qh = prev_region or (0, 0, Wp, Hp)
    sl = (slice(y0, y0 + h), slice(x0, x0 + w))
    n = np.asarray(normal, F)[sl]; P = np.asarray(position, F)[sl]; D = np.asarray(distance, F)[sl]
    o = np.asarray(object, np.int32)[sl]
    reusable = np.asarray(reusable, np.uint8)
    pn = np.asarray(prev_guides["normal"], F); pP = np.asarray(prev_guides["position"], F)
    po = np.asarray(prev_guides["object"], np.int32); pc = np.asarray(prev_radiance, F).reshape(Hp, Wp, 3)
    nm, sp, mw, Nh = F(normal_min), F(sigma_plane), F(min_weight), F(history_samples)
    count = {k: 0 for k in REASONS}
    with np.errstate(all="ignore"):
        in_range = (o >= 0) & (o < len(reusable))
        reus = in_range & (reusable[np.where(in_range, o, 0)] != 0)
        pfin = np.isfinite(P).all(-1)
        valid = reus & pfin
        d = (P - V["c"]).astype(F)
        s = (V["aw"] / dot(d, V["w"])).astype(F)
        front = np.isfinite(s) & (s > 0)
        q = ((d * s[..., None]).astype(F) - V["a"]).astype(F)
        fi = (dot(q, V["du"]) * V["iu"]).astype(F)
        fj = (dot(q, V["dv"]) * V["iv"]).astype(F)
        inside = (np.isfinite(fi) & np.isfinite(fj) & (fi > F(-1)) & (fi < F(Wp)) & (fj > F(-1)) & (fj < F(Hp)))
        count["object_range"] = int((~in_range).sum()); count["not_reusable"] = int((in_range & ~reus).sum())
        count["position_nan"] = int((reus & ~pfin).sum()); count["behind"] = int((valid & ~front).sum())
        count["outside"] = int((valid & front & ~inside).sum())
        valid = valid & front & inside
        fi = np.where(valid, fi, F(0)).astype(F); fj = np.where(valid, fj, F(0)).astype(F)
        fi0, fj0 = np.floor(fi), np.floor(fj)
        i0, j0 = fi0.astype(np.int64), fj0.astype(np.int64)
        ax, ay = (fi - fi0).astype(F), (fj - fj0).astype(F)
        plane = (sp * D).astype(F)
        ws = np.zeros((h, w), F); acc = np.zeros((h, w, 3), F)
        for dy in (0, 1):                                  # tap order: dy outer, dx inner
            for dx in (0, 1):
                ti, tj = i0 + dx, j0 + dy
                tin = ((ti >= 0) & (ti < Wp) & (tj >= 0) & (tj < Hp) & (ti >= qx0) & (ti < qx0 + qw) & (tj >= qy0)
                       & (tj < qy0 + qh))
                tic, tjc = np.clip(ti, 0, Wp - 1), np.clip(tj, 0, Hp - 1)
                nq, Pq, oq, cq = pn[tjc, tic], pP[tjc, tic], po[tjc, tic], pc[tjc, tic]
                b = ((ax if dx else (F(1) - ax).astype(F)) * (ay if dy else (F(1) - ay).astype(F))).astype(F)
                same = oq == o
                cfin = np.isfinite(cq).all(-1)
                nok = dot(n, nq) >= nm
                pok = np.abs(dot(n, (Pq - P).astype(F))) <= plane
                ok = valid & tin & same & cfin & nok & pok
                t = valid & tin
                count["tap_outside"] += int((valid & ~tin).sum()); count["tap_object"] += int((t & ~same).sum())
                count["tap_nonfinite"] += int((t & same & ~cfin).sum())
                count["tap_normal"] += int((t & same & cfin & ~nok).sum())
                count["tap_plane"] += int((t & same & cfin & nok & ~pok).sum())
                ws = (ws + np.where(ok, b, F(0))).astype(F)
                acc = (acc + np.where(ok[..., None], (b[..., None] * cq).astype(F), F(0))).astype(F)  # multiply, then add
        weight = np.where(ws >= mw, ws, F(0)).astype(F)
        count["low_weight"] = int(((ws > 0) & (weight == 0)).sum())
        has = weight > 0
        history = np.where(has[..., None], (acc / ws[..., None]).astype(F), F(0)).astype(F)
    if reasons is not None:
        reasons.update(count)
    res = {"history": np.zeros((Hh, Ww, 3), F), "weight": np.zeros((Hh, Ww), F), "radiance": None, "rgb": None}
    res["history"][sl] = history; res["weight"][sl] = weight
    if radiance is not None:
        full = np.asarray(radiance, F).reshape(Hh, Ww, 3)
        c = full[sl]
        m = (np.asarray(px_samples, np.int32).reshape(Hh, Ww)[sl].astype(F) if px_samples is not None
             else np.full((h, w), F(samples if samples is not None else 0), F))
        with np.errstate(all="ignore"):
            blend = (((history * Nh).astype(F) + (c * m[..., None]).astype(F)).astype(F) / (Nh + m).astype(F)[..., None])
        use = has & np.isfinite(c).all(-1) & (m > 0)
        out = np.where(use[..., None], blend, np.where(has[..., None], history, c)).astype(F)
        res["radiance"] = full.copy(); res["radiance"][sl] = out
        res["rgb"] = to_u8_ref(res["radiance"])
    return res


# ---- shared fixtures of the reproject tests ---------------------------------------------------
MOVE = (0.5, 0.2, -0.2)


def moved_scene(scene, move=MOVE):
    """The scene seen from a camera whose `from` is moved by `move` (everything else unchanged)."""
    cam = dict(scene["camera"])
    cam["from"] = [float(a) + float(b) for a, b in zip(cam["from"], move)]
    return {**scene, "camera": cam}


def oracle_view(oracle, scene, render_opts):
    ci = oracle.camera_info(scene, render_opts)
    return {**{k: np.asarray(ci[k], dtype=F) for k in ("center", "pixel00", "du", "dv")}, "width": ci["width"],
            "height": ci["height"]}


def oracle_quality(oracle, scene, width, move=MOVE, spp_prev=256, spp_fresh=4, spp_truth=1024, threads=8, **opts):
    """View A = the scene's camera at spp_prev, view B = `from` moved by `move`, fresh at
    spp_fresh, truth B at spp_truth (depth 8, aTolerance 0); the restatement on oracle frames and
    oracle guides. Returns {"share": pixels with weight > 0, "ratio": display-domain MSE of the
    blend / of the fresh frame, "mse_fresh"}."""
    from denoise_ref import display_mse, oracle_guides
    ro = {"width": width, "depth": 8, "aTolerance": 0}
    sb = moved_scene(scene, move)
    prev = oracle.render(scene, {**ro, "samples": spp_prev}, threads=threads)["radiance"]
    fresh = oracle.render(sb, {**ro, "samples": spp_fresh}, threads=threads)
    truth = oracle.render(sb, {**ro, "samples": spp_truth}, threads=threads)["radiance"]
    pn, pP, pd, po, _ = oracle_guides(oracle, scene, {**ro, "samples": 4})
    n, P, d, o, _ = oracle_guides(oracle, sb, {**ro, "samples": 4})
    res = reproject_ref(prev, oracle_view(oracle, scene, ro), {"normal": pn, "position": pP, "distance": pd, "object": po},
                        n, P, d, o, reusable_from_scene(scene), radiance=fresh["radiance"],
                        px_samples=fresh["px_samples"], **opts)
    before = display_mse(fresh["radiance"], truth)
    return {"share": float((res["weight"] > 0).mean()), "ratio": display_mse(res["radiance"], truth) / before,
            "mse_fresh": before, "frame": f"{truth.shape[1]}x{truth.shape[0]}"}
