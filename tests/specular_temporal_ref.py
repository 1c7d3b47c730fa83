"""The normative definition of the accumulation across views through specular chains
(rt_temporal_accumulate_specular, rt_camera_progressive_accumulate_specular), restated in NumPy fp32
from temporal_ref.py and specular_reproject_ref.py: only add, subtract, multiply, IEEE divide,
floor, min and comparisons, in the order written; no fused multiply-add; reproject_ref's dot. Every
operation has exactly one fp32 result, so the device output equals this in every bit.

A pixel whose chain word has k = ch & 0xff == 0 is temporal_ref's pixel on the first-hit guides. A
pixel with k >= 1 whose chain ends on a surface projects X = cn + (P1 - cn) * (Ds / D1) into the
history's view and tests its taps on the chain planes the history keeps of that view - if it keeps
any, walked with the same guide options; a tap counts where specular_reproject_ref's chain test
holds with temporal_ref's colour and length conditions in place of the finite flag. Sums, the
min_weight cut and the blend are temporal_ref's.
A helper module of the specular-temporal tests, not a test file."""
import numpy as np

from denoise_ref import to_u8_ref
from denoise_var_ref import denoise_var_ref
from reproject_ref import F, dot, view_constants
from specular_reproject_ref import REASONS as RS_REASONS, chain_point, pix2_of
from temporal_ref import STEP, sanitise

REASONS = RS_REASONS + ("tap_length", "no_chain_history")
GUIDE_KEYS = ("normal", "position", "distance", "object")


def same_guide_options(a, b):
    """{max_bounces, max_fuzz} equal in every bit (max_fuzz as fp32)."""
    return (a is not None and b is not None and int(a[0]) == int(b[0])
            and np.asarray(a[1], F).view(np.uint32) == np.asarray(b[1], F).view(np.uint32))


def specular_temporal_ref(history, view, first, chain, radiance, variance, reusable, through, guide_options=(8, 0.0),
                          px_samples=None, samples=None, region=None, normal_min=0.9, sigma_plane=0.01, min_weight=0.25,
                          max_history=256.0, filter_levels=0, sigma_variance=2.0, point_pixels=4.0, reasons=None):
    """history: None (empty) or temporal_ref's history dict ("guides": the first-hit planes), with,
    when it was committed by this function, "chain": {"normal", "position", "distance", "object",
    "chain"} and "guide_options": (max_bounces, max_fuzz) of the view it holds. view: the new view
    (its centre is used; it is committed). first / chain: the new view's first-hit guides and its
    guides through the chain with the chain word, walked with `guide_options`. Returns
    temporal_ref's dict plus "kind": uint8 (H, W), 0 no history, 1 first hit, 2 chain; "history" is
    the committed history. `reasons` (a dict) receives the rejection counts per name in REASONS."""
    Hh, Ww = np.asarray(first["object"]).shape
    x0, y0, w, h = region or (0, 0, Ww, Hh)
    sl = (slice(y0, y0 + h), slice(x0, x0 + w))
    cn = np.asarray(view["center"], F)
    n1 = np.asarray(first["normal"], F)[sl]; P1 = np.asarray(first["position"], F)[sl]
    D1 = np.asarray(first["distance"], F)[sl]; o1 = np.asarray(first["object"], np.int32)[sl]
    ns = np.asarray(chain["normal"], F)[sl]; Ps = np.asarray(chain["position"], F)[sl]
    Ds = np.asarray(chain["distance"], F)[sl]; os_ = np.asarray(chain["object"], np.int32)[sl]
    ch = np.asarray(chain["chain"], np.int32)[sl]
    c = np.asarray(radiance, F).reshape(Hh, Ww, 3)[sl]
    v = sanitise(np.asarray(variance, F).reshape(Hh, Ww)[sl])
    m = (np.asarray(px_samples, np.int32).reshape(Hh, Ww)[sl].astype(F) if px_samples is not None
         else np.full((h, w), F(samples if samples is not None else 0), F))
    reusable = np.asarray(reusable, np.uint8); through = np.asarray(through, np.uint8)
    n_obj = len(reusable)
    assert len(through) == n_obj
    nm, sp, mw, mh = F(normal_min), F(sigma_plane), F(min_weight), F(max_history)
    pp = F(point_pixels)
    count = {k: 0 for k in REASONS}
    spec = (ch & 0xff) >= 1
    ws = np.zeros((h, w), F); acc = np.zeros((h, w, 3), F); av = np.zeros((h, w), F); al = np.zeros((h, w), F)
    if history is not None:
        V = view_constants(history["view"])
        Wp, Hp = V["width"], V["height"]
        qx0, qy0, qw, qh = history["region"] or (0, 0, Wp, Hp)
        pn1 = np.asarray(history["guides"]["normal"], F); pP1 = np.asarray(history["guides"]["position"], F)
        po1 = np.asarray(history["guides"]["object"], np.int32)
        held = history.get("chain") is not None and same_guide_options(history.get("guide_options"), guide_options)
        if held:
            pns = np.asarray(history["chain"]["normal"], F); pPs = np.asarray(history["chain"]["position"], F)
            pos_ = np.asarray(history["chain"]["object"], np.int32); pch = np.asarray(history["chain"]["chain"], np.int32)
        else:                                               # (never read: every k >= 1 pixel is invalid)
            pns, pPs, pos_, pch = pn1, pP1, po1, np.zeros((Hp, Wp), np.int32)
        pc = np.asarray(history["radiance"], F).reshape(Hp, Wp, 3)
        pV = sanitise(np.asarray(history["variance"], F).reshape(Hp, Wp))
        pL = np.asarray(history["length"], F).reshape(Hp, Wp)
        pp2 = F(F(pp * pp) * pix2_of(V))
        with np.errstate(all="ignore"):
            ends = ((ch >> 8) & 0xff) == 1
            # the guides a pixel is tested on: the chain's where k >= 1, the first hit's elsewhere
            n = np.where(spec[..., None], ns, n1).astype(F); P = np.where(spec[..., None], Ps, P1).astype(F)
            D = np.where(spec, Ds, D1).astype(F); o = np.where(spec, os_, o1)
            in_range = (o >= 0) & (o < n_obj)
            reus = in_range & (reusable[np.where(in_range, o, 0)] != 0)
            in1 = (o1 >= 0) & (o1 < n_obj)
            thr = in1 & (through[np.where(in1, o1, 0)] != 0)
            pfin = np.isfinite(P).all(-1) & (~spec | (np.isfinite(P1).all(-1) & np.isfinite(Ds) & np.isfinite(D1) & (D1 > 0)))
            held_ok = ~spec | held
            end_ok = ~spec | ends
            thr_ok = ~spec | thr
            count["no_chain_history"] = int((~held_ok).sum())
            t = held_ok
            count["chain_end"] = int((t & ~end_ok).sum()); t = t & end_ok
            count["object_range"] = int((t & ~in_range).sum())
            count["not_reusable"] = int((t & in_range & ~reus).sum()); t = t & reus
            count["not_through"] = int((t & ~thr_ok).sum()); t = t & thr_ok
            count["position_nan"] = int((t & ~pfin).sum())
            valid = t & pfin
            # 1. projection and validity: X in place of P where k >= 1
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
            # 2. the gather over the taps that count (dy outer, dx inner; multiply, then add)
            for dy in (0, 1):
                for dx in (0, 1):
                    ti, tj = i0 + dx, j0 + dy
                    tin = ((ti >= 0) & (ti < Wp) & (tj >= 0) & (tj < Hp) & (ti >= qx0) & (ti < qx0 + qw) & (tj >= qy0)
                           & (tj < qy0 + qh))
                    tic, tjc = np.clip(ti, 0, Wp - 1), np.clip(tj, 0, Hp - 1)
                    sp3 = spec[..., None]
                    nq = np.where(sp3, pns[tjc, tic], pn1[tjc, tic]).astype(F)
                    Pq = np.where(sp3, pPs[tjc, tic], pP1[tjc, tic]).astype(F)
                    oq1, oqs, chq = po1[tjc, tic], pos_[tjc, tic], pch[tjc, tic]
                    cq, Vq, Lq = pc[tjc, tic], pV[tjc, tic], pL[tjc, tic]
                    b = ((ax if dx else (F(1) - ax).astype(F)) * (ay if dy else (F(1) - ay).astype(F))).astype(F)
                    same_ch = ~spec | (chq == ch)
                    same_1 = ~spec | (oq1 == o1)
                    same = np.where(spec, oqs == os_, oq1 == o1)
                    cfin = np.isfinite(cq).all(-1)
                    nok = dot(n, nq) >= nm
                    e = (Pq - P).astype(F)
                    pok = np.abs(dot(n, e)) <= plane
                    ptok = ~spec | (dot(e, e) <= point)
                    lok = np.isfinite(Lq) & (Lq > 0)
                    t = valid & tin
                    ok = t & same_ch & same_1 & same & cfin & nok & pok & ptok & lok
                    count["tap_outside"] += int((valid & ~tin).sum())
                    count["tap_chain"] += int((t & ~same_ch).sum()); t = t & same_ch
                    count["tap_first_object"] += int((t & ~same_1).sum()); t = t & same_1
                    count["tap_object"] += int((t & ~same).sum()); t = t & same
                    count["tap_nonfinite"] += int((t & ~cfin).sum()); t = t & cfin
                    count["tap_normal"] += int((t & ~nok).sum()); t = t & nok
                    count["tap_plane"] += int((t & ~pok).sum()); t = t & pok
                    count["tap_point"] += int((t & ~ptok).sum()); t = t & ptok
                    count["tap_length"] += int((t & ~lok).sum())
                    ws = (ws + np.where(ok, b, F(0))).astype(F)
                    acc = (acc + np.where(ok[..., None], (b[..., None] * cq).astype(F), F(0))).astype(F)
                    av = (av + np.where(ok, (b * Vq).astype(F), F(0))).astype(F)
                    al = (al + np.where(ok, (b * Lq).astype(F), F(0))).astype(F)
    with np.errstate(all="ignore"):
        weight = np.where(ws >= mw, ws, F(0)).astype(F)
        count["low_weight"] = int(((ws > 0) & (weight == 0)).sum())
        has = weight > 0
        hc = (acc / ws[..., None]).astype(F); Vh = (av / ws).astype(F); Lh = (al / ws).astype(F)
        N = np.minimum(Lh, mh).astype(F)
        # 3. the blend: temporal_ref's
        cfin = np.isfinite(c).all(-1)
        use = has & cfin & (m > 0)
        den = (N + m).astype(F)
        blend = (((hc * N[..., None]).astype(F) + (c * m[..., None]).astype(F)).astype(F) / den[..., None]).astype(F)
        g = (N / den).astype(F); a = (m / den).astype(F)
        Vb = (((g * g).astype(F) * Vh).astype(F) + ((a * a).astype(F) * v).astype(F)).astype(F)
        out = np.where(use[..., None], blend, np.where(has[..., None], hc, c)).astype(F)
        Vout = np.where(use, Vb, np.where(has, Vh, v)).astype(F)
        Lout = np.where(use, den, np.where(has, N, np.where(cfin, m, F(0)))).astype(F)
    if reasons is not None:
        reasons.update(count)
    rad_f = np.zeros((Hh, Ww, 3), F)
    var_f, len_f, wgt_f = (np.zeros((Hh, Ww), F) for _ in range(3))
    kind_f = np.zeros((Hh, Ww), np.uint8)
    rad_f[sl] = out; var_f[sl] = Vout; len_f[sl] = Lout; wgt_f[sl] = weight
    kind_f[sl] = np.where(has, np.where(spec, 2, 1), 0).astype(np.uint8)
    dtypes = {"object": np.int32, "chain": np.int32}
    committed = {"view": view, "region": (x0, y0, w, h),
                 "guides": {k: np.asarray(first[k], dtypes.get(k, F)) for k in GUIDE_KEYS},
                 "chain": {k: np.asarray(chain[k], dtypes.get(k, F)) for k in GUIDE_KEYS + ("chain",)},
                 "guide_options": (int(guide_options[0]), float(F(guide_options[1]))),
                 "radiance": rad_f.copy(), "variance": var_f.copy(), "length": len_f.copy()}
    res = {"radiance": rad_f, "variance": var_f, "length": len_f, "weight": wgt_f, "kind": kind_f, "history": committed}
    if filter_levels > 0:
        # 4. the optional filter of what is returned, on the CHAIN guides of the new view: what a
        # mirror shows is edge-stopped by the surface it shows; the history keeps the unfiltered frame
        cg = committed["chain"]
        fr, fv = denoise_var_ref(rad_f, var_f, cg["normal"], cg["position"], cg["distance"], cg["object"],
                                 region=(x0, y0, w, h), levels=filter_levels, sigma_variance=sigma_variance,
                                 sigma_plane=sigma_plane)
        res["radiance"], res["variance"] = fr, fv
    res["rgb"] = np.zeros((Hh, Ww, 3), np.uint8)
    res["rgb"][sl] = to_u8_ref(res["radiance"][sl])
    return res


def plain_history(history):
    """A history as a plain commit leaves it: no chain planes."""
    return {k: v for k, v in history.items() if k not in ("chain", "guide_options")}


# ---- the quality trial on oracle frames (tools/specular_temporal_quality.py, the ABI test) --------------
def oracle_views(oracle, scene, width, views=5, spp=4, step=STEP, max_bounces=8, max_fuzz=0.0, aspect=None):
    """Views k = 0 .. views-1 of `scene` with `from` moved by k * step, `spp` samples per view, seed
    1000 + k (depth 8, aTolerance 0): per view {"scene", "ro", "view", "first", "chain", "radiance",
    "variance"} - frames and variances from oracle_window, guides from the oracle and guide_walk_ref."""
    from denoise_ref import oracle_guides
    from denoise_var_ref import oracle_window
    from guide_walk_ref import guide_walk_ref
    from reproject_ref import moved_scene, oracle_view
    out = []
    for k in range(views):
        sk = moved_scene(scene, tuple(k * s for s in step))
        ro = {"width": width, "depth": 8, "aTolerance": 0, "seed": 1000 + k}
        if aspect is not None:
            ro["aspect"] = aspect
        fresh, var = oracle_window(oracle, sk, ro, spp)
        gro = {**ro, "samples": 4}
        out.append({"scene": sk, "ro": ro, "view": oracle_view(oracle, sk, ro),
                    "first": dict(zip(GUIDE_KEYS, oracle_guides(oracle, sk, gro)[:4])),
                    "chain": dict(zip(GUIDE_KEYS + ("chain",), guide_walk_ref(oracle, sk, gro, max_bounces, max_fuzz))),
                    "radiance": fresh, "variance": var})
    return out


def oracle_trial(oracle, scene, width, views=5, spp=4, spp_truth=1024, step=STEP, threads=8, filter_levels=4,
                 max_bounces=8, max_fuzz=0.0, through=15, aspect=None, **opts):
    """temporal_ref.oracle_trial's experiment with the chains: the same frames accumulated by
    temporal_ref ("plain") and by this restatement ("chains"); truth = the last view at spp_truth of
    another seed. Returns display-domain MSE ratios to the last view's fresh frame over the frame and
    over its k >= 1 pixels ("k1_*"), unfiltered and (filter_levels) filtered, and the shares."""
    from reproject_ref import reusable_from_scene
    from specular_reproject_ref import through_from_scene
    from temporal_ref import accumulate_ref
    vs = oracle_views(oracle, scene, width, views, spp, step, max_bounces, max_fuzz, aspect)
    reus = reusable_from_scene(scene); thr = through_from_scene(scene, through, max_fuzz)
    hp = hs = None
    for u in vs:
        rp, hp = accumulate_ref(hp, u["view"], u["first"], u["radiance"], u["variance"], reus, samples=spp)
        rs = specular_temporal_ref(hs, u["view"], u["first"], u["chain"], u["radiance"], u["variance"], reus, thr,
                                   (max_bounces, max_fuzz), samples=spp, **opts)
        hs = rs["history"]
    last = vs[-1]
    truth = oracle.render(last["scene"], {**last["ro"], "seed": 77, "samples": spp_truth}, threads=threads)["radiance"]
    k1 = (last["chain"]["chain"] & 0xff) >= 1

    def mse(a, mask=None):
        with np.errstate(all="ignore"):
            da = np.sqrt(np.clip(a.astype(np.float64), 0, 1)); db = np.sqrt(np.clip(truth.astype(np.float64), 0, 1))
        e = ((da - db) ** 2).mean(-1)
        return float(e.mean() if mask is None else e[mask].mean())

    fresh = last["radiance"]
    before, before1 = mse(fresh), (mse(fresh, k1) if k1.any() else float("nan"))
    out = {"frame": f"{truth.shape[1]}x{truth.shape[0]}", "k1": float(k1.mean()), "mse_fresh": before,
           "k1_with_history": float((rs["kind"][k1] == 2).mean()) if k1.any() else 0.0,
           "plain": mse(rp["radiance"]) / before, "chains": mse(rs["radiance"]) / before}
    if k1.any():
        out["k1_plain"] = mse(rp["radiance"], k1) / before1
        out["k1_chains"] = mse(rs["radiance"], k1) / before1
        out["k1_length"] = float(rs["length"][k1].mean())
    if filter_levels > 0:
        f1, c1 = last["first"], last["chain"]
        fp = denoise_var_ref(rp["radiance"], rp["variance"], *(f1[k] for k in GUIDE_KEYS), levels=filter_levels)[0]
        fs = denoise_var_ref(rs["radiance"], rs["variance"], *(c1[k] for k in GUIDE_KEYS), levels=filter_levels)[0]
        out["plain_filtered"] = mse(fp) / before; out["chains_filtered"] = mse(fs) / before
        if k1.any():
            out["k1_plain_filtered"] = mse(fp, k1) / before1; out["k1_chains_filtered"] = mse(fs, k1) / before1
    return out


# ---- a synthetic sequence --------------------------------------------------------------------------------
def synthetic_history(s, guide_options=(8, 0.0), chain=True, seed=23):
    """The previous view of synthetic_pair(faults=True) as a history: its radiance with the injected
    faults, a variance plane and a length plane that contains zeros, NaNs and infinities."""
    rng = np.random.default_rng(seed)
    Hp, Wp = s["prev_first"]["object"].shape
    L = rng.integers(1, 40, (Hp, Wp)).astype(F)
    L[10, 20] = 0; L[11, 22] = np.nan; L[13, 24] = np.inf; L[9, 28] = 0; L[12, 29] = np.nan; L[13, 30] = np.inf
    L[8:15:3, 26:33:2] = 0                                  # taps of k >= 1 pixels
    Vp = (rng.random((Hp, Wp), dtype=F) * F(0.5)).astype(F)
    Vp[9, 15] = -1; Vp[10, 16] = np.nan; Vp[12, 27] = np.inf
    hist = {"view": s["prev_view"], "region": None, "guides": dict(s["prev_first"]), "radiance": s["prev_radiance"],
            "variance": Vp, "length": L}
    if chain:
        hist["chain"] = dict(s["prev_chain"]); hist["guide_options"] = guide_options
    return hist


def synthetic_variance(s, seed=29):
    rng = np.random.default_rng(seed)
    v = (rng.random(s["fresh"].shape[:2], dtype=F) * F(0.5)).astype(F)
    v[6, 9] = -2; v[7, 11] = np.nan; v[9, 13] = np.inf
    return v
