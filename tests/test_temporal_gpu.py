"""Accumulation across views on the GPU. Every comparison with the NumPy restatement
(tests/temporal_ref.py, the normative definition) is exact: == on bits, NaN equal to NaN -
radiance, variance, length, weight and u8."""
import functools
import json
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
from denoise_ref import bits_equal, display_mse  # noqa: E402
from reproject_ref import moved_scene  # noqa: E402
from temporal_ref import STEP, accumulate_ref, temporal_ref  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
GOLDEN = Path(__file__).resolve().parent / "golden"
SENT = np.float32(-123.25)
NON_DEFAULT = dict(normal_min=0.5, sigma_plane=0.05, min_weight=0.6, max_history=6.0, sigma_variance=1.5)
OUTPUTS = ("radiance", "variance", "length", "weight")


@functools.lru_cache(maxsize=None)
def _scene(rt, key):
    return rt.generate_scene_data(json.loads(key))


def scene(rt, cfg):
    return _scene(rt, json.dumps(cfg, sort_keys=True))


def _box(region, H, W):
    x, y, w, h = region or (0, 0, W, H)
    box = (slice(y, y + h), slice(x, x + w))
    mask = np.ones((H, W), bool)
    mask[box] = False
    return box, mask


def sentinels(H, W):
    return {"rgb": np.full((H, W, 3), 0xA5, np.uint8), "radiance": np.full((H, W, 3), SENT, F),
            "variance": np.full((H, W), SENT, F), "length": np.full((H, W), SENT, F), "weight": np.full((H, W), SENT, F)}


def assert_outputs(got, want, region, what):
    """The five outputs against `want` inside the region, their sentinels outside it."""
    H, W = want["weight"].shape
    box, mask = _box(region, H, W)
    bad = {k: int((~bits_equal(got[k][box], want[k][box])).sum()) for k in OUTPUTS}
    bad["rgb"] = int((got["rgb"][box] != want["rgb"][box]).sum())
    share = float((want["weight"][box] > 0).mean())
    print(f"{what}: values differing from the restatement {bad} ({share:.3f} of the region has a history)")
    assert not any(bad.values()), what
    assert (got["rgb"][mask] == 0xA5).all() and all((got[k][mask] == SENT).all() for k in OUTPUTS), what


# ---- 1. explicit buffers, synthetic ------------------------------------------------------------------
N_B = np.array([0.6, 0.0, 0.8], F)                  # plane B's unit normal


def _pinhole(shape, center, spacing):
    H, W = shape
    c = np.asarray(center, F)
    view = {"center": c, "pixel00": (c + np.array([-(W - 1) / 2 * spacing, (H - 1) / 2 * spacing, -1.0])).astype(F),
            "du": np.array([spacing, 0, 0], F), "dv": np.array([0, -spacing, 0], F), "width": W, "height": H}
    i = np.arange(W, dtype=F)[None, :, None]; j = np.arange(H, dtype=F)[:, None, None]
    d = ((view["pixel00"] + view["du"] * i + view["dv"] * j) - c).astype(F)
    return view, d


def _two_planes(view, d, miss_rows):
    """First hits of the rays c + t d on plane A (z = -5, object 0, normal +z) where that hit has
    x >= -0.5, else on plane B (N_B . X = -4.5, object 1); `miss_rows` are misses."""
    c = view["center"]
    tA = ((F(-5) - c[2]) / d[..., 2]).astype(F)
    PA = (c + d * tA[..., None]).astype(F)
    tB = ((F(-4.5) - (N_B * c).sum()) / (d * N_B).sum(-1)).astype(F)
    PB = (c + d * tB[..., None]).astype(F)
    useA = PA[..., 0] >= F(-0.5)
    P = np.where(useA[..., None], PA, PB).astype(F)
    n = np.where(useA[..., None], np.array([0, 0, 1], F), N_B).astype(F)
    obj = np.where(useA, 0, 1).astype(np.int32)
    obj[miss_rows] = -1; P[miss_rows] = 0; n[miss_rows] = 0
    q = (P - c).astype(F)
    D = np.where(obj >= 0, np.sqrt(((q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1]).astype(F)
                                    + q[..., 2] * q[..., 2]).astype(F)), F(0)).astype(F)
    return {"normal": n, "position": P, "distance": D, "object": obj}


def _planes(rng, shape, pshape):
    """What the accumulation adds to a pair of views: the history's length and variance planes and
    the fresh variance, with the values that must not count sprinkled in."""
    plen = rng.integers(1, 40, pshape).astype(F)
    plen[rng.random(pshape) < 0.08] = 0                                         # never held a sample
    plen.flat[rng.choice(plen.size, 6, replace=False)] = [np.inf, np.nan, 1000.0, np.inf, np.nan, 1000.0]
    pvar = (rng.random(pshape, dtype=F) * F(0.5)).astype(F)
    pvar.flat[rng.choice(pvar.size, 6, replace=False)] = [-1.0, np.nan, np.inf, -0.25, np.nan, np.inf]
    var = (rng.random(shape, dtype=F) * F(0.5)).astype(F)
    var.flat[rng.choice(var.size, 6, replace=False)] = [-1.0, np.nan, np.inf, -0.25, np.nan, np.inf]
    return plen, pvar, var


@functools.lru_cache(maxsize=None)
def synthetic(pair):
    """Two analytic planes seen from two pinhole cameras, plus misses and injected faults. "small":
    the new view 29x37 with region (3, 5, 29, 19) is wider than the previous one (23x41, region
    (2, 3, 33, 17)) and moved, so projections land inside, on the border and outside the previous
    image, and two points lie behind it. "wide": 9 rows x 130 columns, the whole frame - three
    workgroup columns, the last one partial."""
    rng = np.random.default_rng(17)
    if pair == "small":
        shape, region, pshape, pregion = (29, 37), (3, 5, 29, 19), (23, 41), (2, 3, 33, 17)
        pview, pd = _pinhole(pshape, (0, 0, 0), 0.05)
        view, d = _pinhole(shape, (0.35, 0.1, 0.3), 0.064)
        pg = _two_planes(pview, pd, slice(0, 4))
        g = _two_planes(view, d, slice(21, 29))
    else:
        shape, region, pshape, pregion = (9, 130), None, (9, 130), None
        pview, pd = _pinhole(pshape, (0, 0, 0), 0.02)
        view, d = _pinhole(shape, (0.11, 0.02, 0.05), 0.02)
        pg = _two_planes(pview, pd, slice(0, 1))
        g = _two_planes(view, d, slice(8, 9))
    prad = (rng.random((*pshape, 3), dtype=F) * F(4)).astype(F)
    fresh = (rng.random((*shape, 3), dtype=F) * F(4)).astype(F)
    pxs = rng.integers(0, 9, shape).astype(np.int32)
    if pair == "small":
        prad[8, 20, 0] = np.nan; prad[9, 24, 1] = np.inf; prad[12, 28, 2] = 1e30   # non-finite / huge radiance
        pg["normal"][10, 22] = -pg["normal"][10, 22]                                # a flipped normal
        pg["position"][14, 26] += pg["normal"][14, 26]                              # a tap off the plane
        pg["object"][16, 30] = 7; pg["object"][11, 18] = 2
        g["position"][8, 10, 1] = np.nan                                            # a NaN position
        g["object"][9, 12] = 7                                                      # an out-of-range object
        g["object"][10, 14:18] = 2                                                  # a non-reusable object
        g["position"][12, 20] = (0.3, 0.2, 2.0); g["position"][13, 21] = (-0.2, 0.1, 0.5)   # behind the previous camera
        fresh[15, 15, 1] = np.nan; fresh[16, 22, 0] = np.inf
    else:
        prad[4, 70, 1] = np.nan; fresh[3, 129, 2] = np.nan; fresh[5, 64, 0] = np.inf
    plen, pvar, var = _planes(rng, shape, pshape)
    for a in (prad, fresh, pxs, plen, pvar, var, *g.values(), *pg.values()):
        a.setflags(write=False)
    hist = {"view": pview, "region": pregion, "guides": pg, "radiance": prad, "variance": pvar, "length": plen}
    return region, g, hist, fresh, pxs, var, np.array([1, 1, 0], np.uint8)


@pytest.mark.parametrize("opts,counts,levels", [({}, True, 0), (NON_DEFAULT, False, 0), ({}, False, 2),
                                                (NON_DEFAULT, True, 2)],
                         ids=["default-pxs", "non-default-scalar", "default-scalar-filter2", "non-default-pxs-filter2"])
@pytest.mark.parametrize("pair", ["small", "wide"])
def test_explicit_buffers_on_synthetic_pairs_of_views(rt, gpu, pair, opts, counts, levels):
    region, g, hist, fresh, pxs, var, reusable = synthetic(pair)
    kw = dict(reusable=reusable, region=region, radiance=fresh, variance=var, filter_levels=levels, **opts)
    kw.update(px_samples=pxs) if counts else kw.update(samples=3)
    want = temporal_ref(hist, **g, **kw)
    H, W = pxs.shape
    box, _ = _box(region, H, W)
    has = want["weight"][box] > 0
    assert 0.2 <= has.mean() < 1                     # some pixels gather a history, some are disoccluded
    if not opts:
        assert (want["length"][box] > 256).any()     # the 1000-sample taps met max_history
    out = sentinels(H, W)
    res = rt.temporal_accumulate(hist["radiance"], hist["variance"], hist["length"], hist["view"], hist["guides"], **g,
                                 prev_region=hist["region"], rgb=out["rgb"], out=out["radiance"],
                                 variance_out=out["variance"], length_out=out["length"], weight_out=out["weight"], **kw)
    assert res is out["radiance"]
    assert_outputs(out, want, region, f"synthetic {pair} {opts or 'defaults'} filter {levels}")
    if levels:                                       # the filter changed the frame, not the length or the weight
        plain = temporal_ref(hist, **g, **{**kw, "filter_levels": 0})
        assert (~bits_equal(plain["radiance"][box], want["radiance"][box])).any()
        assert bits_equal(plain["length"], want["length"]).all() and bits_equal(plain["weight"], want["weight"]).all()


BANDS = (slice(0, 64), slice(64, 128), slice(128, 130))   # the workgroup columns of a 130-pixel row


@functools.lru_cache(maxsize=None)
def wide_pair():
    """The two planes on a 9 x 130 new view - three workgroup columns of 64 pixels, the last one
    partial, and three row groups of 4 - against a history of another shape, 11 x 120. The new
    view's last row and the history's first are misses."""
    rng = np.random.default_rng(23)
    shape, pshape = (9, 130), (11, 120)
    pview, pd = _pinhole(pshape, (0, 0, 0), 0.02)
    view, d = _pinhole(shape, (-0.11, 0.02, 0.05), 0.018)
    pg = _two_planes(pview, pd, slice(0, 1))
    g = _two_planes(view, d, slice(8, 9))
    prad = (rng.random((*pshape, 3), dtype=F) * F(4)).astype(F)
    fresh = (rng.random((*shape, 3), dtype=F) * F(4)).astype(F)
    prad[4, 70, 1] = np.nan; fresh[3, 129, 2] = np.nan; fresh[5, 64, 0] = np.inf
    plen, pvar, var = _planes(rng, shape, pshape)
    for a in (prad, fresh, plen, pvar, var, *g.values(), *pg.values()):
        a.setflags(write=False)
    hist = {"view": pview, "region": None, "guides": pg, "radiance": prad, "variance": pvar, "length": plen}
    return g, hist, fresh, var, np.array([1, 1, 0], np.uint8)


def test_a_9x130_frame_spans_three_workgroup_columns(rt, gpu):
    g, hist, fresh, var, reusable = wide_pair()
    kw = dict(reusable=reusable, radiance=fresh, variance=var, samples=3)
    want = temporal_ref(hist, **g, **kw)
    has = want["weight"] > 0
    assert all(has[:, b].any() and not has[:, b].all() for b in BANDS)
    out = sentinels(9, 130)
    rt.temporal_accumulate(hist["radiance"], hist["variance"], hist["length"], hist["view"], hist["guides"], **g,
                           rgb=out["rgb"], out=out["radiance"], variance_out=out["variance"], length_out=out["length"],
                           weight_out=out["weight"], **kw)
    assert_outputs(out, want, None, "synthetic 9x130")


@pytest.mark.parametrize("levels", [0, 2], ids=["unfiltered", "filter2"])
def test_each_output_alone_is_the_all_outputs_call_on_the_small_pair(rt, gpu, levels):
    """The raw entry with one output pointer at a time (the outputs gate the filter and which
    unpack passes run): every single output equals, bit for bit, the same output of the call that
    asks for all five."""
    import pass_error_cases as pc
    region, g, hist, fresh, pxs, var, reusable = synthetic("small")
    H, W = pxs.shape
    env = pc.Env(rt)
    base = dict(width=W, height=H, region=region, **g, radiance=fresh, px_samples=pxs, samples=0, variance=var,
                prev_view=hist["view"], prev_region=hist["region"], **{"prev_" + k: v for k, v in hist["guides"].items()},
                prev_radiance=hist["radiance"], prev_variance=hist["variance"], prev_length=hist["length"],
                reusable=reusable, n_objects=len(reusable), options={"filter_levels": levels})
    new = lambda: {k + "_out": v for k, v in sentinels(H, W).items()}   # noqa: E731
    full = new()
    assert env.call("rt_temporal_accumulate", {**base, **full})[0] == 0
    box, _ = _box(region, H, W)
    assert all((a[box] != new()[k][box]).any() for k, a in full.items())
    for k in full:
        one = new()
        assert env.call("rt_temporal_accumulate", {**base, k: one[k]})[0] == 0, k
        assert bits_equal(one[k], full[k]).all(), (k, levels)


# ---- 2. the session entry ------------------------------------------------------------------------------
SESSION_CASES = {
    "cornell40": ({"type": "cornell"}, {"width": 40, "samples": 60, "depth": 8}, "brute"),
    "spheres200-fast": ({"type": "spheres", "options": {"count": 200, "seed": 42}},
                        {"width": 48, "aspect": 1, "samples": 60, "depth": 8, "traversal": "fast"}, "fast"),
    "spheres200-reference": ({"type": "spheres", "options": {"count": 200, "seed": 42}},
                             {"width": 48, "aspect": 1, "samples": 60, "depth": 8, "traversal": "reference"}, "reference"),
    "default40": ({"type": "default"}, {"width": 40, "samples": 60, "depth": 8}, None),
}
MOVE = (0.25, 0.1, -0.1)


def view_camera(rt, sd, ro, k, move=MOVE):
    """View k of a path: `from` moved by k * move, seed 1000 + k."""
    return rt.create_camera_from_scene_data(moved_scene(sd, tuple(k * m for m in move)), {**ro, "seed": 1000 + k})


def _step(cam, pr, n):
    H, W = cam.image_height, cam.image_width
    rgb = np.zeros((H, W, 3), np.uint8)
    rad = np.zeros((H, W, 3), np.float32)
    pxs = np.zeros((H, W), np.int32)
    st = pr.step(n, rgb, radiance=rad, px_samples=pxs)
    return rgb, rad, pxs, st


def accumulate(pr, history, H, W, **kw):
    out = sentinels(H, W)
    res = pr.accumulated(history, out["rgb"], out["radiance"], variance_out=out["variance"], length_out=out["length"],
                         weight_out=out["weight"], **kw)
    assert res is out["radiance"]
    return out


def assert_history(history, ref_hist, views, what):
    i = history.info
    H, W = i["height"], i["width"]
    box, mask = _box(ref_hist["region"], H, W)
    got = history.read()
    assert i["views"] == history.views == views and i["region"] == tuple(ref_hist["region"]) and i["bytes"] > 0, what
    for k in ("radiance", "variance", "length"):
        assert bits_equal(got[k][box], ref_hist[k][box]).all(), f"{what}: history {k}"
        assert (got[k][mask] == 0).all(), what
    for k in ("center", "pixel00", "du", "dv"):
        assert i["view"][k].tobytes() == ref_hist["view"][k].tobytes(), what


@pytest.mark.parametrize("whole", [True, False], ids=["frame", "region"])
@pytest.mark.parametrize("case", list(SESSION_CASES))
def test_session_entry_follows_the_restatement_along_three_views(rt, gpu, case, whole):
    from raytracer_amd import _lib
    cfg, ro, trav = SESSION_CASES[case]
    sd = scene(rt, cfg)
    ref_hist, counts, prev = None, set(), None
    with rt.History() as history:
        for k in range(3):
            cam = view_camera(rt, sd, ro, k)
            if trav is not None:
                assert cam.info["traversal"] == _lib.TRAVERSAL[trav]
            H, W = cam.image_height, cam.image_width
            region = None if whole else (5, 3, W - 11, H - 8)
            box, _ = _box(region, H, W)
            with cam.progressive(region) as pr:
                _step(cam, pr, 10)
                _, rad, pxs, _ = _step(cam, pr, 10)
                counts |= {int(v) for v in np.unique(pxs[box])}
                var = pr.variance()
                if prev is not None:
                    prev.close()                     # the history needs neither the previous camera nor its session
                kw = dict(reusable=cam.reusable_objects(), px_samples=pxs, region=region)
                if k == 2:                           # the filtered frame first, uncommitted
                    want, _ = accumulate_ref(ref_hist, cam.view(), cam.render_guides(), rad, var, filter_levels=2, **kw)
                    got = accumulate(pr, history, H, W, commit=False, filter_levels=2)
                    assert_outputs(got, want, region, f"{case} view {k} filter 2")
                    assert history.views == 2
                want, ref_hist = accumulate_ref(ref_hist, cam.view(), cam.render_guides(), rad, var, **kw)
                got = accumulate(pr, history, H, W)
                assert_outputs(got, want, region, f"{case} view {k}")
                if k:
                    assert (want["weight"][box] > 0).any() and (want["length"][box] > pxs[box]).any()
                else:
                    assert (want["weight"] == 0).all() and bits_equal(want["radiance"][box], rad[box]).all()
                assert_history(history, ref_hist, k + 1, f"{case} view {k}")
            prev = cam
        t = history.times()
        assert t["guide_ms"] > 0 and t["gather_ms"] > 0 and t["filter_ms"] == 0
        assert t["total_ms"] >= t["guide_ms"] + t["gather_ms"]
    print(f"{case} {'frame' if whole else 'region'}: px_samples seen {sorted(counts)}")
    if case == "cornell40":
        assert len(counts) >= 2                      # pixels have retired at different counts


# ---- 3. commit semantics ---------------------------------------------------------------------------------
def test_commit_semantics_leave_history_and_session_alone(rt, gpu):
    sd = scene(rt, {"type": "cornell"})
    ro = {"width": 40, "samples": 60, "depth": 8}
    cam0, cam, plain = view_camera(rt, sd, ro, 0), view_camera(rt, sd, ro, 1), view_camera(rt, sd, ro, 1)
    with rt.History() as history, cam.progressive() as pr, plain.progressive() as pq:
        with cam0.progressive() as p0:
            _step(cam0, p0, 10)
            accumulate(p0, history, 40, 40)
        _step(cam, pr, 10); _step(plain, pq, 10)
        _step(cam, pr, 10); _step(plain, pq, 10)
        blob = pr.save()
        before, info = history.read(), history.info
        a = accumulate(pr, history, 40, 40, commit=False)
        b = accumulate(pr, history, 40, 40, commit=False)
        assert all(bits_equal(a[k], b[k]).all() for k in a) and (a["weight"] > 0).any()
        after = history.read()
        assert all(bits_equal(before[k], after[k]).all() for k in before)
        i2 = history.info
        assert i2["views"] == 1 and all(np.array_equal(i2[k], info[k]) for k in info if k not in ("view", "bytes"))
        assert pr.save() == blob
        c = accumulate(pr, history, 40, 40)          # the committed call returns the same frame
        assert all(bits_equal(a[k], c[k]).all() for k in a) and history.views == 2
        got = history.read()
        assert bits_equal(got["radiance"], c["radiance"]).all() and bits_equal(got["length"], c["length"]).all()
        assert pr.save() == blob and pr.samples_done == 20 and pr.steps == 2
        # the session's next step is that of a session that never accumulated
        rgb_p, rad_p, pxs_p, st_p = _step(cam, pr, 10)
        rgb_q, rad_q, pxs_q, st_q = _step(plain, pq, 10)
        assert (rgb_p == rgb_q).all() and bits_equal(rad_p, rad_q).all() and (pxs_p == pxs_q).all()
        assert (st_p.pixels, st_p.samples, st_p.bounces) == (st_q.pixels, st_q.samples, st_q.bounces)
        assert pr.save() == pq.save()


def test_uncommitted_preview_of_another_scene_leaves_no_trace(rt, gpu):
    """An empty history previewed (commit=False) from one scene, then fed another: nothing of the
    first - its reusable table, its image size - is left in the views that follow."""
    other = rt.create_camera_from_scene_data(scene(rt, {"type": "default"}), {"width": 56, "samples": 8, "seed": 7})
    sd = scene(rt, {"type": "cornell"})
    ro = {"width": 40, "samples": 8, "depth": 8, "aTolerance": 0}
    with rt.History() as history:
        with other.progressive() as po:
            po.step(4)
            po.accumulated(history, commit=False)
        assert history.views == 0 and history.info["device"] == -1
        ref_hist = None
        for k in range(2):
            cam = view_camera(rt, sd, ro, k)
            with cam.progressive() as pr:
                _, rad, pxs, _ = _step(cam, pr, 4)
                want, ref_hist = accumulate_ref(ref_hist, cam.view(), cam.render_guides(), rad, pr.variance(),
                                                cam.reusable_objects(), px_samples=pxs)
                assert_outputs(accumulate(pr, history, 40, 40), want, None, f"cornell after a foreign preview, view {k}")
        assert (want["weight"] > 0).mean() > 0.5


# ---- 4. errors on an open session --------------------------------------------------------------------------
def test_session_errors(rt, gpu):
    from raytracer_amd import _lib
    sd = scene(rt, {"type": "cornell"})
    ro = {"width": 40, "samples": 60, "depth": 8}
    with rt.History() as history:
        for mode in ("bounces", "samples"):
            cam = rt.create_camera_from_scene_data(sd, {**ro, "mode": mode})
            with cam.progressive() as pr:
                pr.step(4)
                with pytest.raises(rt.RtError, match="not radiance") as e:
                    pr.accumulated(history)
                assert e.value.code == _lib.RT_ERR_INVALID
        cam = rt.create_camera_from_scene_data(sd, ro)
        other = rt.create_camera_from_scene_data(scene(rt, {"type": "default"}), {"width": 40, "samples": 60})
        with cam.progressive() as pr:
            pr.step(1)
            with pytest.raises(rt.RtError, match="samples_done < 2") as e:
                pr.accumulated(history)
            assert e.value.code == _lib.RT_ERR_INVALID and history.views == 0
            pr.step(3)
            for kw, word in (({"sigma_plane": -1.0}, "sigma_plane"), ({"max_history": float("nan")}, "max_history"),
                             ({"filter_levels": 9}, "filter_levels")):
                with pytest.raises(rt.RtError, match=word) as e:
                    pr.accumulated(history, **kw)
                assert e.value.code == _lib.RT_ERR_INVALID
            assert history.views == 0
            assert np.isfinite(pr.accumulated(history)).all() and history.views == 1
            with other.progressive() as po:
                po.step(4)
                with pytest.raises(rt.RtError, match="temporal: the history holds a different scene") as e:
                    po.accumulated(history)
                assert e.value.code == _lib.RT_ERR_INVALID
            assert history.views == 1
            assert np.isfinite(pr.accumulated(history)).all() and history.views == 2   # the session still works
            pr.step(4)


# ---- 5. end to end --------------------------------------------------------------------------------------------
def test_end_to_end_cornell_96_beats_the_fresh_filtered_frame(rt, gpu):
    """Cornell 96x96, depth 8, aTolerance 0, every frame from the GPU: 5 views moved by
    k (0.125, 0.05, -0.05), 4 samples per view, seed 1000 + k, filter_levels 4, truth = the last
    view at spp 1024. The restatement on oracle frames of this size gives accumulation + filter /
    fresh 0.1078 (tools/temporal_quality.py); asserted <= 0.1186, the same 10 % headroom as the
    host test, and below the GPU's own fresh + variance-guided filter."""
    sd = json.loads((GOLDEN / "scene_cornell.json").read_text())["scene"]
    ro = {"width": 96, "depth": 8, "aTolerance": 0, "samples": 4}
    with rt.History() as history:
        for k in range(5):
            cam = view_camera(rt, sd, ro, k, STEP)
            with cam.progressive() as pr:
                _, fresh, _, _ = _step(cam, pr, 4)
                out = pr.accumulated(history, filter_levels=4)
                if k == 4:
                    fresh_filtered = pr.denoised(variance=True)
        assert history.views == 5
    truth_cam = rt.create_camera_from_scene_data(moved_scene(sd, tuple(4 * s for s in STEP)),
                                                 {**ro, "samples": 1024, "seed": 1004})
    truth = np.zeros((96, 96, 3), np.float32)
    truth_cam.render(np.zeros((96, 96, 3), np.uint8), radiance=truth)
    before = display_mse(fresh, truth)
    ratio, ratio_fresh = display_mse(out, truth) / before, display_mse(fresh_filtered, truth) / before
    print(f"cornell 96x96 on the GPU, 5 views of 4 spp: fresh MSE {before:.6e}, accumulation + filter / fresh {ratio:.4f}, "
          f"fresh + variance-guided filter / fresh {ratio_fresh:.4f}")
    assert ratio <= 0.1186
    assert ratio < ratio_fresh


# ---- 6. repeatability ---------------------------------------------------------------------------------------------
def test_two_histories_are_identical_and_survive_release_device(rt, gpu):
    sd = scene(rt, {"type": "cornell"})
    ro = {"width": 40, "samples": 8, "depth": 8, "aTolerance": 0}

    def run(history, release):
        outs = []
        for k in range(3):
            cam = view_camera(rt, sd, ro, k)
            with cam.progressive() as pr:
                pr.step(4)
                outs.append(accumulate(pr, history, 40, 40, filter_levels=2 if k == 2 else 0))
            if release:
                cam.release_device()                 # frees the camera's buffers, not the history's
            cam.close()
        return outs, history.read()

    with rt.History() as ha, rt.History() as hb:
        (oa, ra), (ob, rb) = run(ha, False), run(hb, True)
        for a, b in zip(oa, ob):
            assert all(bits_equal(a[k], b[k]).all() for k in a)
        assert all(bits_equal(ra[k], rb[k]).all() for k in ra)
        assert (oa[2]["weight"] > 0).any() and ha.info["bytes"] == hb.info["bytes"] > 0
        t = ha.times()
        assert t["filter_ms"] > 0 and t["total_ms"] >= t["guide_ms"] + t["gather_ms"] + t["filter_ms"]
    # close() freed the buffers: the handle is gone, and a new history starts empty
    with pytest.raises(ValueError):
        ha.read()
    with rt.History() as hc:
        assert hc.views == 0 and hc.info["bytes"] == 0
