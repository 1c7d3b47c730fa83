"""The normative definition of the accumulation across views with a per-pixel history length and
variance (rt_temporal_accumulate, rt_camera_progressive_accumulate), restated in NumPy fp32. Only
add, subtract, multiply, IEEE divide, floor, min and comparisons, in the order written; no fused
multiply-add; dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z. Every operation has exactly one fp32
result, so the device output equals this in every bit. The projection and the tap conditions are
tests/reproject_ref.py's, with one more: a tap counts only where the history's length is finite and
> 0. A helper module of the temporal tests, not a test file."""
import numpy as np

from denoise_ref import to_u8_ref
from denoise_var_ref import denoise_var_ref
from reproject_ref import F, dot, view_constants


def sanitise(v):
    """The variance filter's rule: anything that is not (v >= 0 and finite) becomes 0."""
    v = np.asarray(v, F)
    with np.errstate(all="ignore"):
        return np.where((v >= 0) & np.isfinite(v), v, F(0)).astype(F)


def temporal_ref(history, normal, position, distance, object, radiance, variance, reusable, px_samples=None,
                 samples=None, region=None, normal_min=0.9, sigma_plane=0.01, min_weight=0.25, max_history=256.0,
                 filter_levels=0, sigma_variance=2.0):
    """history: None (empty) or {"view", "region" (x, y, w, h), "guides": {"normal", "position",
    "distance", "object"}, "radiance" (Hp, Wp, 3), "variance" (Hp, Wp), "length" (Hp, Wp)}, full
    frames of the history's own image. Returns {"radiance", "rgb", "variance", "length", "weight":
    full-frame arrays of the new frame, zero outside `region`; "history": the committed history},
    where radiance / rgb / variance are filtered when filter_levels > 0 and the committed history
    never is."""
    Hh, Ww = np.asarray(object).shape
    x0, y0, w, h = region or (0, 0, Ww, Hh)
    sl = (slice(y0, y0 + h), slice(x0, x0 + w))
    n = np.asarray(normal, F)[sl]; P = np.asarray(position, F)[sl]; D = np.asarray(distance, F)[sl]
    o = np.asarray(object, np.int32)[sl]
    c = np.asarray(radiance, F).reshape(Hh, Ww, 3)[sl]
    v = sanitise(np.asarray(variance, F).reshape(Hh, Ww)[sl])
    m = (np.asarray(px_samples, np.int32).reshape(Hh, Ww)[sl].astype(F) if px_samples is not None
         else np.full((h, w), F(samples if samples is not None else 0), F))
    reusable = np.asarray(reusable, np.uint8)
    nm, sp, mw, mh = F(normal_min), F(sigma_plane), F(min_weight), F(max_history)
    ws = np.zeros((h, w), F); acc = np.zeros((h, w, 3), F); av = np.zeros((h, w), F); al = np.zeros((h, w), F)
    if history is not None:
        V = view_constants(history["view"])
        Wp, Hp = V["width"], V["height"]
        qx0, qy0, qw, qh = history["region"] or (0, 0, Wp, Hp)
        pn = np.asarray(history["guides"]["normal"], F); pP = np.asarray(history["guides"]["position"], F)
        po = np.asarray(history["guides"]["object"], np.int32)
        pc = np.asarray(history["radiance"], F).reshape(Hp, Wp, 3)
        pV = sanitise(np.asarray(history["variance"], F).reshape(Hp, Wp))
        pL = np.asarray(history["length"], F).reshape(Hp, Wp)
        with np.errstate(all="ignore"):
            # 1. projection and validity: reproject_ref's, plus the tap's length
            in_range = (o >= 0) & (o < len(reusable))
            valid = in_range & (reusable[np.where(in_range, o, 0)] != 0) & np.isfinite(P).all(-1)
            d = (P - V["c"]).astype(F)
            s = (V["aw"] / dot(d, V["w"])).astype(F)
            q = ((d * s[..., None]).astype(F) - V["a"]).astype(F)
            fi = (dot(q, V["du"]) * V["iu"]).astype(F)
            fj = (dot(q, V["dv"]) * V["iv"]).astype(F)
            valid = (valid & np.isfinite(s) & (s > 0) & np.isfinite(fi) & np.isfinite(fj) & (fi > F(-1)) & (fi < F(Wp))
                     & (fj > F(-1)) & (fj < F(Hp)))
            fi = np.where(valid, fi, F(0)).astype(F); fj = np.where(valid, fj, F(0)).astype(F)
            fi0, fj0 = np.floor(fi), np.floor(fj)
            i0, j0 = fi0.astype(np.int64), fj0.astype(np.int64)
            ax, ay = (fi - fi0).astype(F), (fj - fj0).astype(F)
            plane = (sp * D).astype(F)
            # 2. the gather over the taps that count (dy outer, dx inner; multiply, then add)
            for dy in (0, 1):
                for dx in (0, 1):
                    ti, tj = i0 + dx, j0 + dy
                    tin = ((ti >= 0) & (ti < Wp) & (tj >= 0) & (tj < Hp) & (ti >= qx0) & (ti < qx0 + qw) & (tj >= qy0)
                           & (tj < qy0 + qh))
                    tic, tjc = np.clip(ti, 0, Wp - 1), np.clip(tj, 0, Hp - 1)
                    nq, Pq, oq, cq, Vq, Lq = pn[tjc, tic], pP[tjc, tic], po[tjc, tic], pc[tjc, tic], pV[tjc, tic], pL[tjc, tic]
                    b = ((ax if dx else (F(1) - ax).astype(F)) * (ay if dy else (F(1) - ay).astype(F))).astype(F)
                    ok = (valid & tin & (oq == o) & np.isfinite(cq).all(-1) & (dot(n, nq) >= nm)
                          & (np.abs(dot(n, (Pq - P).astype(F))) <= plane) & np.isfinite(Lq) & (Lq > 0))
                    ws = (ws + np.where(ok, b, F(0))).astype(F)
                    acc = (acc + np.where(ok[..., None], (b[..., None] * cq).astype(F), F(0))).astype(F)
                    av = (av + np.where(ok, (b * Vq).astype(F), F(0))).astype(F)
                    al = (al + np.where(ok, (b * Lq).astype(F), F(0))).astype(F)
    with np.errstate(all="ignore"):
        weight = np.where(ws >= mw, ws, F(0)).astype(F)
        has = weight > 0
        hc = (acc / ws[..., None]).astype(F); Vh = (av / ws).astype(F); Lh = (al / ws).astype(F)
        N = np.minimum(Lh, mh).astype(F)
        # 3. the blend
        cfin = np.isfinite(c).all(-1)
        use = has & cfin & (m > 0)
        den = (N + m).astype(F)
        blend = (((hc * N[..., None]).astype(F) + (c * m[..., None]).astype(F)).astype(F) / den[..., None]).astype(F)
        g = (N / den).astype(F); a = (m / den).astype(F)
        Vb = (((g * g).astype(F) * Vh).astype(F) + ((a * a).astype(F) * v).astype(F)).astype(F)
        out = np.where(use[..., None], blend, np.where(has[..., None], hc, c)).astype(F)
        Vout = np.where(use, Vb, np.where(has, Vh, v)).astype(F)
        Lout = np.where(use, den, np.where(has, N, np.where(cfin, m, F(0)))).astype(F)
    rad_f = np.zeros((Hh, Ww, 3), F)
    var_f, len_f, wgt_f = (np.zeros((Hh, Ww), F) for _ in range(3))
    rad_f[sl] = out; var_f[sl] = Vout; len_f[sl] = Lout; wgt_f[sl] = weight
    committed = {"view": None, "region": (x0, y0, w, h),
                 "guides": {"normal": np.asarray(normal, F), "position": np.asarray(position, F),
                            "distance": np.asarray(distance, F), "object": np.asarray(object, np.int32)},
                 "radiance": rad_f.copy(), "variance": var_f.copy(), "length": len_f.copy()}
    res = {"radiance": rad_f, "variance": var_f, "length": len_f, "weight": wgt_f, "history": committed}
    if filter_levels > 0:
        # 4. the optional filter of what is returned; the history keeps the unfiltered frame
        fr, fv = denoise_var_ref(rad_f, var_f, np.asarray(normal, F), np.asarray(position, F), np.asarray(distance, F),
                                 np.asarray(object, np.int32), region=(x0, y0, w, h), levels=filter_levels,
                                 sigma_variance=sigma_variance, sigma_plane=sigma_plane)
        res["radiance"], res["variance"] = fr, fv
    res["rgb"] = np.zeros((Hh, Ww, 3), np.uint8)
    res["rgb"][sl] = to_u8_ref(res["radiance"][sl])
    return res


def accumulate_ref(history, view, guides, radiance, variance, reusable, **kw):
    """One view of a chain: temporal_ref, with the committed history carrying `view` (the new
    view, as Camera.view()). Returns (result, history for the next view)."""
    res = temporal_ref(history, **guides, radiance=radiance, variance=variance, reusable=reusable, **kw)
    res["history"]["view"] = view
    return res, res["history"]


# ---- the quality trial on oracle frames (tools/temporal_quality.py, tests/test_temporal_abi.py) ----
STEP = (0.125, 0.05, -0.05)


def oracle_trial(oracle, scene, width, views=5, spp=4, spp_truth=1024, step=STEP, threads=8, filter_levels=4):
    """Views k = 0 .. views-1 of `scene` with `from` moved by k * step, `spp` samples per view,
    seed 1000 + k (depth 8, aTolerance 0), frames and variances from oracle_window, guides from
    the oracle; truth = the last view at spp_truth. Returns display-domain MSE ratios to the last
    view's fresh frame: {"chained", "accumulated", "fresh_filtered", "chained_filtered",
    "accumulated_filtered", "mse_fresh", "frame", "length_ok"}."""
    from denoise_ref import display_mse, oracle_guides
    from denoise_var_ref import oracle_window
    from reproject_ref import moved_scene, oracle_view, reproject_ref, reusable_from_scene
    reusable = reusable_from_scene(scene)
    hist, chain, prev = None, None, None
    length_ok = True
    for k in range(views):
        sk = moved_scene(scene, tuple(k * s for s in step))
        ro = {"width": width, "depth": 8, "aTolerance": 0, "seed": 1000 + k}
        fresh, var = oracle_window(oracle, sk, ro, spp)
        n, P, d, o, _ = oracle_guides(oracle, sk, {**ro, "samples": 4})
        g = {"normal": n, "position": P, "distance": d, "object": o}
        view = oracle_view(oracle, sk, ro)
        res, hist = accumulate_ref(hist, view, g, fresh, var, reusable, samples=spp)
        length_ok &= bool((res["length"][res["weight"] == 0] == F(spp)).all()
                          and (res["length"] <= F(256.0 + spp)).all())
        if prev is None:
            chain = fresh
        else:
            chain = reproject_ref(chain, prev[0], prev[1], n, P, d, o, reusable, radiance=fresh, samples=spp)["radiance"]
        prev = (view, g)
    truth = oracle.render(sk, {**ro, "samples": spp_truth}, threads=threads)["radiance"]
    ga = (g["normal"], g["position"], g["distance"], g["object"])
    before = display_mse(fresh, truth)
    ratio = lambda a: display_mse(a, truth) / before                           # noqa: E731
    return {"chained": ratio(chain), "accumulated": ratio(res["radiance"]),
            "fresh_filtered": ratio(denoise_var_ref(fresh, var, *ga, levels=filter_levels)[0]),
            "chained_filtered": ratio(denoise_var_ref(chain, var, *ga, levels=filter_levels)[0]),
            "accumulated_filtered": ratio(denoise_var_ref(res["radiance"], res["variance"], *ga, levels=filter_levels)[0]),
            "mse_fresh": before, "frame": f"{truth.shape[1]}x{truth.shape[0]}", "length_ok": length_ok}
