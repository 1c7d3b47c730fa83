"""The normative definition of the reprojection of a previous view's frame through specular chains
(rt_reproject_specular), restated in NumPy fp32 in the style of reproject_ref.py: only add,
subtract, multiply, IEEE divide, floor and comparisons, in the order written; no fused
multiply-add; reproject_ref's dot. Every operation has exactly one fp32 result, so the device
output equals this in every bit.

A pixel whose chain word has k = ch & 0xff == 0 is reproject_ref's pixel on the first-hit guides.
A pixel with k >= 1 that ends on a surface (e = (ch >> 8) & 0xff == 1) projects
X = cn + (P1 - cn) * (Ds / D1) - the point at the summed path length along the primary ray - into
the previous view and tests its taps on the previous view's chain guides.
A helper module of the specular-reproject tests, not a test file."""
import copy
import json
from pathlib import Path

import numpy as np

from denoise_ref import to_u8_ref
from reproject_ref import F, MOVE, REASONS as RP_REASONS, dot, moved_scene, oracle_view, view_constants

REASONS = RP_REASONS + ("chain_end", "not_through", "tap_chain", "tap_first_object", "tap_point")
THROUGH_METAL, THROUGH_GLASS, THROUGH_MIXED, THROUGH_LAYERED = 1, 2, 4, 8
GOLDEN = Path(__file__).resolve().parent / "golden"


def pix2_of(V):
    """dot(du, du) / dot(a, a) of view_constants' V: the squared footprint of a previous pixel per
    squared unit of distance."""
    with np.errstate(all="ignore"):
        return F(dot(V["du"], V["du"]) / dot(V["a"], V["a"]))


def through_from_scene(scene, mask=15, max_fuzz=0.0):
    """through[o] = 1 iff object o's resolved top-level material (ids followed) is a metal of fuzz
    <= max_fuzz (mask bit 1), glass (2), mixed (4) or layered (8)."""
    by_id = {m["id"]: m["material"] for m in scene.get("materials", [])}
    out = []
    for ob in scene["objects"]:
        m = ob.get("material")
        while isinstance(m, str):
            m = by_id.get(m)
        kind = m.get("type") if isinstance(m, dict) else None
        ok = False
        if kind == "metal":
            fuzz = float(m.get("fuzz", 0.0))
            fuzz = max(0.0, fuzz) if fuzz < 1 else 1.0            # Metal's constructor
            ok = bool(mask & THROUGH_METAL) and not fuzz > float(F(max_fuzz))
        elif kind == "glass":
            ok = bool(mask & THROUGH_GLASS)
        elif kind == "mixed":
            ok = bool(mask & THROUGH_MIXED)
        elif kind == "layered":
            ok = bool(mask & THROUGH_LAYERED)
        out.append(1 if ok else 0)
    return np.array(out, np.uint8)


def chain_point(cn, P1, D1, Ds):
    """X = cn + (P1 - cn) * (Ds / D1): subtract, multiply, add, each rounded once."""
    with np.errstate(all="ignore"):
        r = (Ds / D1).astype(F)
        return (cn + ((P1 - cn).astype(F) * r[..., None]).astype(F)).astype(F)


def specular_reproject_ref(prev_radiance, prev_view, prev_first, prev_chain, view, first, chain, reusable, through,
                           region=None, prev_region=None, radiance=None, px_samples=None, samples=None, normal_min=0.9,
                           sigma_plane=0.01, min_weight=0.25, history_samples=32.0, point_pixels=4.0, reasons=None,
                           points=None):
    """first / prev_first: {"normal", "position", "distance", "object"} - the first-hit guides of
    the new and the previous view; chain / prev_chain: the same four plus "chain", the guides
    through the specular chain of one rt_guide_options. view: the new view (its centre is used).
    Returns reproject_ref's dict plus "kind": uint8 (H, W), 0 no history, 1 first hit, 2 chain.
    `reasons` (a dict) receives the rejection counts per name in REASONS; `points` (a dict) the
    projected point of every region pixel under "X"."""
    V = view_constants(prev_view)
    Wp, Hp = V["width"], V["height"]
    cn = np.asarray(view["center"], F)
    Hh, Ww = np.asarray(first["object"]).shape
    x0, y0, w, h = region or (0, 0, Ww, Hh)
    qx0, qy0, qw, qh = prev_region or (0, 0, Wp, Hp)
    sl = (slice(y0, y0 + h), slice(x0, x0 + w))
    n1 = np.asarray(first["normal"], F)[sl]; P1 = np.asarray(first["position"], F)[sl]
    D1 = np.asarray(first["distance"], F)[sl]; o1 = np.asarray(first["object"], np.int32)[sl]
    ns = np.asarray(chain["normal"], F)[sl]; Ps = np.asarray(chain["position"], F)[sl]
    Ds = np.asarray(chain["distance"], F)[sl]; os_ = np.asarray(chain["object"], np.int32)[sl]
    ch = np.asarray(chain["chain"], np.int32)[sl]
    reusable = np.asarray(reusable, np.uint8); through = np.asarray(through, np.uint8)
    n_obj = len(reusable)
    assert len(through) == n_obj
    pn1 = np.asarray(prev_first["normal"], F); pP1 = np.asarray(prev_first["position"], F)
    po1 = np.asarray(prev_first["object"], np.int32)
    pns = np.asarray(prev_chain["normal"], F); pPs = np.asarray(prev_chain["position"], F)
    pos_ = np.asarray(prev_chain["object"], np.int32); pch = np.asarray(prev_chain["chain"], np.int32)
    pc = np.asarray(prev_radiance, F).reshape(Hp, Wp, 3)
    nm, sp, mw, Nh = F(normal_min), F(sigma_plane), F(min_weight), F(history_samples)
    pp = F(point_pixels)
    pp2 = F(F(pp * pp) * pix2_of(V))
    count = {k: 0 for k in REASONS}
    with np.errstate(all="ignore"):
        spec = (ch & 0xff) >= 1
        ends = ((ch >> 8) & 0xff) == 1
        # the guides a pixel is tested on: the chain's where k >= 1, the first hit's elsewhere
        n = np.where(spec[..., None], ns, n1).astype(F); P = np.where(spec[..., None], Ps, P1).astype(F)
        D = np.where(spec, Ds, D1).astype(F); o = np.where(spec, os_, o1)
        in_range = (o >= 0) & (o < n_obj)
        reus = in_range & (reusable[np.where(in_range, o, 0)] != 0)
        in1 = (o1 >= 0) & (o1 < n_obj)
        thr = in1 & (through[np.where(in1, o1, 0)] != 0)
        pfin = np.isfinite(P).all(-1) & (~spec | (np.isfinite(P1).all(-1) & np.isfinite(Ds) & np.isfinite(D1) & (D1 > 0)))
        end_ok = ~spec | ends
        thr_ok = ~spec | thr
        count["chain_end"] = int((~end_ok).sum())
        count["object_range"] = int((end_ok & ~in_range).sum())
        count["not_reusable"] = int((end_ok & in_range & ~reus).sum())
        count["not_through"] = int((end_ok & reus & ~thr_ok).sum())
        count["position_nan"] = int((end_ok & reus & thr_ok & ~pfin).sum())
        valid = end_ok & reus & thr_ok & pfin
        X = np.where(spec[..., None], chain_point(cn, P1, D1, Ds), P1).astype(F)
        d = (X - V["c"]).astype(F)
        s = (V["aw"] / dot(d, V["w"])).astype(F)
        front = np.isfinite(s) & (s > 0)
        q = ((d * s[..., None]).astype(F) - V["a"]).astype(F)
        fi = (dot(q, V["du"]) * V["iu"]).astype(F)
        fj = (dot(q, V["dv"]) * V["iv"]).astype(F)
        inside = (np.isfinite(fi) & np.isfinite(fj) & (fi > F(-1)) & (fi < F(Wp)) & (fj > F(-1)) & (fj < F(Hp)))
        count["behind"] = int((valid & ~front).sum())
        count["outside"] = int((valid & front & ~inside).sum())
        valid = valid & front & inside
        fi = np.where(valid, fi, F(0)).astype(F); fj = np.where(valid, fj, F(0)).astype(F)
        fi0, fj0 = np.floor(fi), np.floor(fj)
        i0, j0 = fi0.astype(np.int64), fj0.astype(np.int64)
        ax, ay = (fi - fi0).astype(F), (fj - fj0).astype(F)
        plane = (sp * D).astype(F)
        point = ((pp2 * D).astype(F) * D).astype(F)
        ws = np.zeros((h, w), F); acc = np.zeros((h, w, 3), F)
        for dy in (0, 1):                                  # tap order: dy outer, dx inner
            for dx in (0, 1):
                ti, tj = i0 + dx, j0 + dy
                tin = ((ti >= 0) & (ti < Wp) & (tj >= 0) & (tj < Hp) & (ti >= qx0) & (ti < qx0 + qw) & (tj >= qy0)
                       & (tj < qy0 + qh))
                tic, tjc = np.clip(ti, 0, Wp - 1), np.clip(tj, 0, Hp - 1)
                sp3 = spec[..., None]
                nq = np.where(sp3, pns[tjc, tic], pn1[tjc, tic]).astype(F)
                Pq = np.where(sp3, pPs[tjc, tic], pP1[tjc, tic]).astype(F)
                oq1, oqs, chq, cq = po1[tjc, tic], pos_[tjc, tic], pch[tjc, tic], pc[tjc, tic]
                b = ((ax if dx else (F(1) - ax).astype(F)) * (ay if dy else (F(1) - ay).astype(F))).astype(F)
                same_ch = ~spec | (chq == ch)
                same_1 = ~spec | (oq1 == o1)
                same = np.where(spec, oqs == os_, oq1 == o1)
                cfin = np.isfinite(cq).all(-1)
                nok = dot(n, nq) >= nm
                e = (Pq - P).astype(F)
                pok = np.abs(dot(n, e)) <= plane
                ptok = ~spec | (dot(e, e) <= point)
                t = valid & tin
                ok = t & same_ch & same_1 & same & cfin & nok & pok & ptok
                count["tap_outside"] += int((valid & ~tin).sum())
                count["tap_chain"] += int((t & ~same_ch).sum()); t = t & same_ch
                count["tap_first_object"] += int((t & ~same_1).sum()); t = t & same_1
                count["tap_object"] += int((t & ~same).sum()); t = t & same
                count["tap_nonfinite"] += int((t & ~cfin).sum()); t = t & cfin
                count["tap_normal"] += int((t & ~nok).sum()); t = t & nok
                count["tap_plane"] += int((t & ~pok).sum()); t = t & pok
                count["tap_point"] += int((t & ~ptok).sum())
                ws = (ws + np.where(ok, b, F(0))).astype(F)
                acc = (acc + np.where(ok[..., None], (b[..., None] * cq).astype(F), F(0))).astype(F)  # multiply, then add
        weight = np.where(ws >= mw, ws, F(0)).astype(F)
        count["low_weight"] = int(((ws > 0) & (weight == 0)).sum())
        has = weight > 0
        history = np.where(has[..., None], (acc / ws[..., None]).astype(F), F(0)).astype(F)
    if reasons is not None:
        reasons.update(count)
    if points is not None:
        points["X"] = X
    res = {"history": np.zeros((Hh, Ww, 3), F), "weight": np.zeros((Hh, Ww), F), "radiance": None, "rgb": None,
           "kind": np.zeros((Hh, Ww), np.uint8)}
    res["history"][sl] = history; res["weight"][sl] = weight
    res["kind"][sl] = np.where(has, np.where(spec, 2, 1), 0).astype(np.uint8)
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


# ---- shared fixtures of the specular-reproject tests ------------------------------------------------
def golden_scene(name):
    return json.loads((GOLDEN / f"scene_{name}.json").read_text())["scene"]


def mirror_room():
    """Cornell's JSON with its back wall (the third quad) a fuzz-0 metal."""
    sd = copy.deepcopy(golden_scene("cornell"))
    sd["materials"].append({"id": "mirror", "material": {"type": "metal", "color": [0.9, 0.9, 0.9], "fuzz": 0}})
    sd["objects"][2]["material"] = "mirror"
    return sd


def cornell_without_spheres():
    """Cornell's JSON without its spheres: no specular material anywhere."""
    sd = copy.deepcopy(golden_scene("cornell"))
    sd["objects"] = [o for o in sd["objects"] if o["type"] != "sphere"]
    return sd


def analytic_scene():
    """A fuzz-0 metal quad in the plane z = -1 facing a camera at (0, 0, 4), a Lambert wall in the
    plane z = 6 behind the camera, a gradient sky: the mirror shows the wall, whose image lies in
    the plane z = -8."""
    return {"camera": {"from": [0, 0, 4], "at": [0, 0, 0], "up": [0, 1, 0], "vfov": 40, "aperture": 0, "focus": 1,
                       "background": {"type": "gradient", "top": [1, 1, 1], "bottom": [0.5, 0.7, 1.0]}},
            "render": {"aspect": 1},
            "materials": [{"id": "mirror", "material": {"type": "metal", "color": [0.9, 0.9, 0.9], "fuzz": 0}},
                          {"id": "wall", "material": {"type": "lambert", "color": [0.6, 0.4, 0.3]}}],
            "objects": [{"type": "quad", "pos": [-1, -1, -1], "u": [2, 0, 0], "v": [0, 2, 0], "material": "mirror"},
                        {"type": "quad", "pos": [-8, -8, 6], "u": [16, 0, 0], "v": [0, 16, 0], "material": "wall"}]}


def oracle_pair(oracle, scene, render_opts, move=MOVE, max_bounces=8, max_fuzz=0.0):
    """Both views' guides from the oracle: {"prev_view", "view", "prev_first", "prev_chain", "first",
    "chain", "moved"} for the scene's camera and the camera moved by `move`."""
    from denoise_ref import oracle_guides
    from guide_walk_ref import guide_walk_ref
    ro = {**render_opts, "samples": 4}
    keys = ("normal", "position", "distance", "object", "chain")
    sb = moved_scene(scene, move)
    out = {"moved": sb, "prev_view": oracle_view(oracle, scene, ro), "view": oracle_view(oracle, sb, ro)}
    for tag, sd in (("prev_", scene), ("", sb)):
        out[tag + "first"] = dict(zip(keys, oracle_guides(oracle, sd, ro)[:4]))
        out[tag + "chain"] = dict(zip(keys, guide_walk_ref(oracle, sd, ro, max_bounces, max_fuzz)))
    return out


def oracle_quality(oracle, scene, width, move=MOVE, spp_prev=256, spp_fresh=4, spp_truth=1024, threads=8, aspect=None,
                   max_fuzz=0.0, through=15, variants=(), **opts):
    """reproject_ref.oracle_quality's experiment with the chains: view A at spp_prev, view B moved
    by `move` at spp_fresh, truth B at spp_truth (depth 8, aTolerance 0). Returns the share of
    k >= 1 pixels, of those with a history, and display-domain MSE ratios blend / fresh: over the
    frame for reproject_ref ("first_hit") and this restatement ("chains"), and over the k >= 1
    pixels only ("k1_chains"). `variants`: further option dicts ({"point_pixels": ..} /
    {"through": ..}) measured on the same frames, returned under "variants"."""
    from reproject_ref import reproject_ref, reusable_from_scene
    ro = {"width": width, "depth": 8, "aTolerance": 0}
    if aspect is not None:
        ro["aspect"] = aspect
    g = oracle_pair(oracle, scene, ro, move, max_fuzz=max_fuzz)
    prev = oracle.render(scene, {**ro, "samples": spp_prev}, threads=threads)["radiance"]
    fresh = oracle.render(g["moved"], {**ro, "samples": spp_fresh}, threads=threads)
    truth = oracle.render(g["moved"], {**ro, "samples": spp_truth}, threads=threads)["radiance"]
    reus = reusable_from_scene(scene)
    k1 = (g["chain"]["chain"] & 0xff) >= 1

    def mse(a, b, mask=None):
        with np.errstate(all="ignore"):
            da = np.sqrt(np.clip(a.astype(np.float64), 0, 1)); db = np.sqrt(np.clip(b.astype(np.float64), 0, 1))
        e = ((da - db) ** 2).mean(-1)
        return float(e.mean() if mask is None else e[mask].mean())

    before = mse(fresh["radiance"], truth)
    base = reproject_ref(prev, g["prev_view"], g["prev_first"], **g["first"], reusable=reus,
                         radiance=fresh["radiance"], px_samples=fresh["px_samples"])

    def run(through=through, **o):
        reasons = {}
        r = specular_reproject_ref(prev, g["prev_view"], g["prev_first"], g["prev_chain"], g["view"], g["first"],
                                   g["chain"], reus, through_from_scene(scene, through, max_fuzz),
                                   radiance=fresh["radiance"], px_samples=fresh["px_samples"], reasons=reasons,
                                   **{**opts, **o})
        row = {"chains": mse(r["radiance"], truth) / before, "k1_with_history": float((r["kind"][k1] == 2).mean()) if k1.any() else 0.0,
               "tap_point": reasons["tap_point"]}
        if k1.any():
            row["k1_chains"] = mse(r["radiance"], truth, k1) / mse(fresh["radiance"], truth, k1)
        return row

    out = {"frame": f"{truth.shape[1]}x{truth.shape[0]}", "k1": float(k1.mean()), "mse_fresh": before,
           "first_hit": mse(base["radiance"], truth) / before, **run()}
    out["variants"] = [{**v, **run(**v)} for v in variants]
    return out


# ---- a synthetic pair of views -----------------------------------------------------------------------
NEW_SHAPE, REGION = (29, 37), (3, 5, 29, 19)       # (H, W); x, y, w, h
PREV_SHAPE, PREV_REGION = (23, 41), (2, 3, 33, 17)
N_B = np.array([0.6, 0.0, 0.8], F)                  # plane B's unit normal
MIRROR_X, WALL_Z = 1.0, 2.0
SYN_REUSABLE = np.array([1, 1, 0, 0, 1], np.uint8)  # planes A and B, a glossy object, the mirror, the wall
SYN_THROUGH = np.array([0, 0, 0, 1, 0], np.uint8)
SURFACE, LEFT = 1 << 8, 2 << 8                      # end codes of a chain word


def _pinhole(shape, center, spacing):
    H, W = shape
    c = np.asarray(center, F)
    view = {"center": c, "pixel00": (c + np.array([-(W - 1) / 2 * spacing, (H - 1) / 2 * spacing, -1.0])).astype(F),
            "du": np.array([spacing, 0, 0], F), "dv": np.array([0, -spacing, 0], F), "width": W, "height": H}
    i = np.arange(W, dtype=F)[None, :, None]; j = np.arange(H, dtype=F)[:, None, None]
    d = ((view["pixel00"] + view["du"] * i + view["dv"] * j) - c).astype(F)
    return view, d


def _length(q):
    return np.sqrt(((q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1]).astype(F) + q[..., 2] * q[..., 2]).astype(F))


def _two_planes_and_a_mirror(view, d, miss_rows):
    """First hits of the rays c + t d on plane A (z = -5, normal +z) where that hit has x >= -0.5,
    else on plane B (N_B . X = -4.5, object 1); `miss_rows` are misses. Plane A is object 0 where
    x < MIRROR_X and beyond it a fuzz-0 mirror, object 3, that shows the wall z = WALL_Z (object 4,
    normal -z) behind the cameras. Returns (first-hit guides, guides through the chain)."""
    c = view["center"]
    tA = ((F(-5) - c[2]) / d[..., 2]).astype(F)
    PA = (c + d * tA[..., None]).astype(F)
    tB = ((F(-4.5) - (N_B * c).sum()) / (d * N_B).sum(-1)).astype(F)
    PB = (c + d * tB[..., None]).astype(F)
    useA = PA[..., 0] >= F(-0.5)
    P = np.where(useA[..., None], PA, PB).astype(F)
    n = np.where(useA[..., None], np.array([0, 0, 1], F), N_B).astype(F)
    obj = np.where(useA, np.where(PA[..., 0] >= F(MIRROR_X), 3, 0), 1).astype(np.int32)
    obj[miss_rows] = -1; P[miss_rows] = 0; n[miss_rows] = 0
    D = np.where(obj >= 0, _length((P - c).astype(F)), F(0)).astype(F)
    first = {"normal": n, "position": P, "distance": D, "object": obj}
    mir = obj == 3
    dr = (d * np.array([1, 1, -1], F)).astype(F)
    s = ((F(WALL_Z) - P[..., 2]) / dr[..., 2]).astype(F)
    Pw = (P + dr * s[..., None]).astype(F)
    chain = {"normal": np.where(mir[..., None], np.array([0, 0, -1], F), n).astype(F),
             "position": np.where(mir[..., None], Pw, P).astype(F),
             "distance": np.where(mir, (D + _length((Pw - P).astype(F))).astype(F), D).astype(F),
             "object": np.where(mir, 4, obj).astype(np.int32),
             "chain": np.where(mir, 1 | SURFACE, np.where(obj >= 0, SURFACE, 0)).astype(np.int32)}
    return first, chain


def synthetic_pair(faults=True, new_shape=NEW_SHAPE, prev_shape=PREV_SHAPE, new_spacing=0.064, prev_spacing=0.05):
    """Two analytic planes, a mirror and the wall it shows, seen from two pinhole cameras, plus
    misses and (faults=True, for the default shapes) injected faults that make every rejection
    reason occur. The new view is wider than the previous one and moved, so projections land
    inside, on the border and outside the previous image. Returns a dict of read-only arrays."""
    rng = np.random.default_rng(17)
    Hn, Hp = new_shape[0], prev_shape[0]
    pview, pd = _pinhole(prev_shape, (0, 0, 0), prev_spacing)
    view, d = _pinhole(new_shape, (0.35, 0.1, 0.3), new_spacing)
    p1, ps = _two_planes_and_a_mirror(pview, pd, slice(0, Hp * 4 // 23))
    g1, gs = _two_planes_and_a_mirror(view, d, slice(Hn * 21 // 29, Hn))
    prad = (rng.random((*prev_shape, 3), dtype=F) * F(4)).astype(F)
    fresh = (rng.random((*new_shape, 3), dtype=F) * F(4)).astype(F)
    pxs = rng.integers(0, 9, new_shape).astype(np.int32)
    if faults:
        assert new_shape == NEW_SHAPE and prev_shape == PREV_SHAPE
        # the previous view: radiance, then first-hit planes (k == 0 taps), then chain planes (k >= 1 taps)
        prad[8, 20, 0] = np.nan; prad[9, 26, 1] = np.inf; prad[12, 28, 2] = 1e30; prad[7, 30] = np.nan
        p1["normal"][10, 12] = -p1["normal"][10, 12]                          # a flipped normal
        p1["position"][14, 14] += p1["normal"][14, 14]                          # a tap off the plane
        p1["object"][16, 10] = 7; p1["object"][11, 16] = 2                      # another object
        p1["object"][16, 30] = 0; p1["object"][6, 27] = 7                       # a chain from another first object
        ps["normal"][10, 27] = -ps["normal"][10, 27]
        ps["position"][14, 29, 2] += F(0.5)                                     # off the wall's plane
        ps["position"][9, 30, 0] += F(3)                                        # on the plane, another point
        ps["position"][11, 32, 1] -= F(2)
        ps["object"][15, 27] = 1                                                # a chain that ends elsewhere
        ps["chain"][12, 31] = 2 | SURFACE; ps["chain"][8, 25] = 1 | LEFT        # another chain
        # the new view, k == 0 pixels
        g1["position"][8, 10, 1] = np.nan                                       # a NaN position
        g1["object"][9, 12] = 7                                                 # an out-of-range object
        g1["object"][10, 14:18] = 2                                             # a non-reusable object
        g1["position"][12, 16] = (0.3, 0.2, 2.0); g1["position"][13, 17] = (-0.2, 0.1, 0.5)   # behind the previous camera
        # the new view, k >= 1 pixels
        gs["chain"][7, 22] = 1 | LEFT; gs["chain"][7, 23] = 1 | (3 << 8)        # chains that end on no surface
        gs["chain"][14, 22] = 2 | SURFACE                                       # a chain no previous pixel walked
        g1["object"][8, 23] = 0; g1["object"][8, 24] = 7; g1["object"][8, 25] = -1   # a first object chains do not start on
        gs["object"][9, 24] = 7; gs["object"][10, 25] = 2
        g1["distance"][11, 26] = 0; g1["distance"][11, 27] = np.inf
        gs["position"][12, 27, 0] = np.inf; gs["distance"][13, 28] = np.nan; g1["position"][13, 29, 2] = np.nan
        gs["distance"][15, 24] = F(-3)                                          # the virtual point behind the previous camera
        fresh[15, 15, 1] = np.nan; fresh[16, 22, 0] = np.inf
    out = {"view": view, "prev_view": pview, "first": g1, "chain": gs, "prev_first": p1, "prev_chain": ps,
           "prev_radiance": prad, "fresh": fresh, "px_samples": pxs, "reusable": SYN_REUSABLE, "through": SYN_THROUGH}
    for v in (prad, fresh, pxs, *g1.values(), *gs.values(), *p1.values(), *ps.values()):
        v.setflags(write=False)
    return out


def synthetic_call(s, **kw):
    """The restatement on a synthetic pair."""
    return specular_reproject_ref(s["prev_radiance"], s["prev_view"], s["prev_first"], s["prev_chain"], s["view"],
                                  s["first"], s["chain"], s["reusable"], s["through"], **kw)
