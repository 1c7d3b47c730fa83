"""Reprojection of a previous view's frame on the GPU. Every comparison with the NumPy restatement
(tests/reproject_ref.py, the normative definition) is exact: == on bits, NaN equal to NaN -
history, weight, blend and u8."""
import functools
import json
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
from denoise_ref import bits_equal, display_mse  # noqa: E402
from reproject_ref import MOVE, REASONS, moved_scene, reproject_ref  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
GOLDEN = Path(__file__).resolve().parent / "golden"
SENT = np.float32(-123.25)
NON_DEFAULT = dict(normal_min=0.5, sigma_plane=0.05, min_weight=0.6, history_samples=8.0)


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


def render(cam):
    H, W = cam.image_height, cam.image_width
    rgb = np.zeros((H, W, 3), np.uint8)
    rad = np.zeros((H, W, 3), np.float32)
    cam.render(rgb, radiance=rad)
    return rad


def assert_is_restatement(call, want, fresh, region, what):
    """call(rgb=, out=, history_out=, weight_out=) -> blend; all four outputs against `want`
    inside the region, their sentinels outside it."""
    H, W = want["weight"].shape
    rgb = np.full((H, W, 3), 0xA5, np.uint8)
    out = np.full((H, W, 3), SENT, np.float32)
    hist = np.full((H, W, 3), SENT, np.float32)
    wgt = np.full((H, W), SENT, np.float32)
    res = call(rgb=rgb, out=out, history_out=hist, weight_out=wgt)
    assert res is out
    box, mask = _box(region, H, W)
    n_h = int((~bits_equal(hist[box], want["history"][box])).any(-1).sum())
    n_w = int((~bits_equal(wgt[box], want["weight"][box])).sum())
    n_b = int((~bits_equal(out[box], want["radiance"][box])).any(-1).sum())
    n_u = int((rgb[box] != want["rgb"][box]).any(-1).sum())
    share = float((want["weight"][box] > 0).mean())
    changed = int((~bits_equal(out[box], fresh[box])).any(-1).sum())
    print(f"{what}: pixels differing from the restatement: history {n_h}, weight {n_w}, blend {n_b}, u8 {n_u} "
          f"({share:.3f} of the region has a history, {changed} pixels changed by the blend)")
    assert n_h == 0 and n_w == 0 and n_b == 0 and n_u == 0, what
    assert (rgb[mask] == 0xA5).all() and (out[mask] == SENT).all() and (hist[mask] == SENT).all(), what
    assert (wgt[mask] == SENT).all(), what
    return out, hist, wgt


# ---- 1. explicit buffers, synthetic ------------------------------------------------------------------
NEW_SHAPE, REGION = (29, 37), (3, 5, 29, 19)       # (H, W); x, y, w, h
PREV_SHAPE, PREV_REGION = (23, 41), (2, 3, 33, 17)
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


@functools.lru_cache(maxsize=None)
def synthetic():
    """Two analytic planes seen from two pinhole cameras, plus misses and injected faults. The new
    view is wider than the previous one and moved, so projections land inside, on the border
    (-1 < f < 0, W - 1 < f < W) and outside the previous image; two points lie behind it."""
    rng = np.random.default_rng(17)
    pview, pd = _pinhole(PREV_SHAPE, (0, 0, 0), 0.05)
    view, d = _pinhole(NEW_SHAPE, (0.35, 0.1, 0.3), 0.064)
    pg = _two_planes(pview, pd, slice(0, 4))
    g = _two_planes(view, d, slice(21, 29))
    prad = (rng.random((*PREV_SHAPE, 3), dtype=F) * F(4)).astype(F)
    prad[8, 20, 0] = np.nan; prad[9, 24, 1] = np.inf; prad[12, 28, 2] = 1e30   # non-finite / huge radiance
    pg["normal"][10, 22] = -pg["normal"][10, 22]                                # a flipped normal
    pg["position"][14, 26] += pg["normal"][14, 26]                              # a tap off the plane
    pg["object"][16, 30] = 7; pg["object"][11, 18] = 2
    g["position"][8, 10, 1] = np.nan                                            # a NaN position
    g["object"][9, 12] = 7                                                      # an out-of-range object
    g["object"][10, 14:18] = 2                                                  # a non-reusable object
    g["position"][12, 20] = (0.3, 0.2, 2.0); g["position"][13, 21] = (-0.2, 0.1, 0.5)   # behind the previous camera
    fresh = (rng.random((*NEW_SHAPE, 3), dtype=F) * F(4)).astype(F)
    fresh[15, 15, 1] = np.nan; fresh[16, 22, 0] = np.inf
    pxs = rng.integers(0, 9, NEW_SHAPE).astype(np.int32)
    for a in (prad, fresh, pxs, *g.values(), *pg.values()):
        a.setflags(write=False)
    return view, g, pview, pg, prad, fresh, pxs, np.array([1, 1, 0], np.uint8)


@pytest.mark.parametrize("opts,counts", [({}, True), (NON_DEFAULT, False)], ids=["default", "non-default"])
def test_explicit_buffers_on_a_synthetic_pair_of_views(rt, gpu, opts, counts):
    view, g, pview, pg, prad, fresh, pxs, reusable = synthetic()
    kw = dict(reusable=reusable, region=REGION, prev_region=PREV_REGION, radiance=fresh, **opts)
    kw.update(px_samples=pxs) if counts else kw.update(samples=3)
    reasons = {}
    want = reproject_ref(prad, pview, pg, **g, reasons=reasons, **kw)
    box, _ = _box(REGION, *NEW_SHAPE)
    print(f"synthetic {opts or 'defaults'}: rejections {reasons}")
    if not opts:
        assert all(reasons[k] > 0 for k in REASONS), reasons
        assert (want["weight"][box] > 0).mean() >= 0.3
    assert (want["history"][box] > 1e29).any()       # the 1e30 tap is finite: it is gathered
    out, hist, wgt = assert_is_restatement(lambda **o: rt.reproject(prad, pview, pg, **g, **kw, **o), want, fresh, REGION,
                                           f"synthetic {opts or 'defaults'}")
    # history only: no fresh frame, the history is returned
    kw2 = {k: v for k, v in kw.items() if k not in ("radiance", "px_samples", "samples")}
    h2 = rt.reproject(prad, pview, pg, **g, **kw2)
    assert bits_equal(h2[box], hist[box]).all() and (h2[_box(REGION, *NEW_SHAPE)[1]] == 0).all()


def test_each_output_alone_is_the_all_outputs_call_on_the_synthetic_pair(rt, gpu):
    """The raw entry with one output pointer at a time (the outputs gate which unpack passes run):
    every single output equals, bit for bit, the same output of the call that asks for all four."""
    import pass_error_cases as pc
    view, g, pview, pg, prad, fresh, pxs, reusable = synthetic()
    H, W = NEW_SHAPE
    env = pc.Env(rt)
    base = dict(width=W, height=H, region=REGION, **g, prev_view=pview, prev_region=PREV_REGION, prev_radiance=prad,
                **{"prev_" + k: v for k, v in pg.items()}, reusable=reusable, n_objects=len(reusable), radiance=fresh,
                px_samples=pxs, samples=0)
    new = lambda: {"history_out": np.full((H, W, 3), SENT, F), "weight_out": np.full((H, W), SENT, F),   # noqa: E731
                   "radiance_out": np.full((H, W, 3), SENT, F), "rgb_out": np.full((H, W, 3), 0xA5, np.uint8)}
    full = new()
    assert env.call("rt_reproject", {**base, **full})[0] == 0
    box, _ = _box(REGION, H, W)
    assert all((a[box] != new()[k][box]).any() for k, a in full.items())
    for k in full:
        one = new()
        assert env.call("rt_reproject", {**base, k: one[k]})[0] == 0, k
        assert bits_equal(one[k], full[k]).all(), k
    # history only (no fresh frame): the history and the weight, alone and together
    hist_only = {k: v for k, v in base.items() if k not in ("radiance", "px_samples")}
    for keys in (("history_out",), ("weight_out",), ("history_out", "weight_out")):
        one = new()
        assert env.call("rt_reproject", {**hist_only, **{k: one[k] for k in keys}})[0] == 0, keys
        assert all(bits_equal(one[k], full[k]).all() for k in keys), keys


BANDS = (slice(0, 64), slice(64, 128), slice(128, 130))   # the workgroup columns of a 130-pixel row


@functools.lru_cache(maxsize=None)
def wide_pair():
    """The two planes on a 9 x 130 new view - three workgroup columns of 64 pixels, the last one
    partial, and three row groups of 4 - against a previous view of another shape, 11 x 120. The
    new view's last row and the previous view's first are misses."""
    rng = np.random.default_rng(23)
    pview, pd = _pinhole((11, 120), (0, 0, 0), 0.02)
    view, d = _pinhole((9, 130), (-0.11, 0.02, 0.05), 0.018)
    pg = _two_planes(pview, pd, slice(0, 1))
    g = _two_planes(view, d, slice(8, 9))
    prad = (rng.random((11, 120, 3), dtype=F) * F(4)).astype(F)
    fresh = (rng.random((9, 130, 3), dtype=F) * F(4)).astype(F)
    prad[4, 70, 1] = np.nan; fresh[3, 129, 2] = np.nan; fresh[5, 64, 0] = np.inf
    for a in (prad, fresh, *g.values(), *pg.values()):
        a.setflags(write=False)
    return g, pview, pg, prad, fresh, np.array([1, 1, 0], np.uint8)


def test_a_9x130_frame_spans_three_workgroup_columns(rt, gpu):
    g, pview, pg, prad, fresh, reusable = wide_pair()
    kw = dict(reusable=reusable, radiance=fresh, samples=3)
    want = reproject_ref(prad, pview, pg, **g, **kw)
    has = want["weight"] > 0
    assert all(has[:, b].any() and not has[:, b].all() for b in BANDS)
    assert_is_restatement(lambda **o: rt.reproject(prad, pview, pg, **g, **kw, **o), want, fresh, None, "synthetic 9x130")


# ---- 2. the camera entry ---------------------------------------------------------------------------
CAMERA_CASES = {
    "cornell40": ({"type": "cornell"}, {"width": 40, "samples": 8, "depth": 8, "aTolerance": 0}, "brute"),
    "spheres200-fast": ({"type": "spheres", "options": {"count": 200, "seed": 42}},
                        {"width": 48, "aspect": 1, "samples": 8, "depth": 8, "aTolerance": 0, "traversal": "fast"}, "fast"),
    "spheres200-reference": ({"type": "spheres", "options": {"count": 200, "seed": 42}},
                             {"width": 48, "aspect": 1, "samples": 8, "depth": 8, "aTolerance": 0,
                              "traversal": "reference"}, "reference"),
    "default40": ({"type": "default"}, {"width": 40, "samples": 8, "depth": 8, "aTolerance": 0}, None),
}


@pytest.mark.parametrize("case", list(CAMERA_CASES))
def test_camera_entry_is_the_restatement_of_both_cameras_guides(rt, gpu, case):
    from raytracer_amd import _lib
    cfg, ro, trav = CAMERA_CASES[case]
    sd = scene(rt, cfg)
    prev_cam = rt.create_camera_from_scene_data(sd, ro)
    cam = rt.create_camera_from_scene_data(moved_scene(sd), ro)
    if trav is not None:
        assert cam.info["traversal"] == _lib.TRAVERSAL[trav]
    prad, fresh = render(prev_cam), render(cam)
    H, W = cam.image_height, cam.image_width
    g, pg, pview, reusable = cam.render_guides(), prev_cam.render_guides(), prev_cam.view(), cam.reusable_objects()
    sub, psub = (5, 3, W - 9, H - 8), (2, 1, W - 4, H - 5)
    for region, prev_region, opts in ((None, None, {}), (sub, psub, NON_DEFAULT)):
        kw = dict(region=region, prev_region=prev_region, radiance=fresh, samples=8, **opts)
        want = reproject_ref(prad, pview, pg, **g, reusable=reusable, **kw)
        assert (want["weight"] > 0).any()
        assert_is_restatement(lambda **o: cam.reproject(prev_cam, prad, **kw, **o), want, fresh, region,
                              f"{case} region {region}")
    t = cam.reproject_times()
    assert t["guide_ms"] > 0 and t["reproject_ms"] > 0 and t["total_ms"] >= t["guide_ms"] + t["reproject_ms"]
    # the explicit-buffer call on the same inputs gives the same frame
    a = cam.reproject(prev_cam, prad, radiance=fresh, samples=8)
    b = rt.reproject(prad, pview, pg, **g, reusable=reusable, radiance=fresh, samples=8)
    assert bits_equal(a, b).all() and (a != fresh).any()


# ---- 3. the session ----------------------------------------------------------------------------------
SESSION_RO = {"width": 40, "samples": 60, "depth": 8}   # the reference's adaptive defaults


def _step(cam, pr, n):
    H, W = cam.image_height, cam.image_width
    rgb = np.zeros((H, W, 3), np.uint8)
    rad = np.zeros((H, W, 3), np.float32)
    pxs = np.zeros((H, W), np.int32)
    st = pr.step(n, rgb, radiance=rad, px_samples=pxs)
    return rgb, rad, pxs, st


@pytest.mark.parametrize("region", [None, (5, 3, 29, 31)], ids=["frame", "region"])
def test_session_blend_uses_each_pixels_own_samples_and_leaves_the_session_alone(rt, gpu, region):
    sd = scene(rt, {"type": "cornell"})
    prev_cam = rt.create_camera_from_scene_data(sd, {**SESSION_RO, "samples": 8, "aTolerance": 0})
    prad = render(prev_cam)
    msd = moved_scene(sd)
    cam = rt.create_camera_from_scene_data(msd, SESSION_RO)
    plain = rt.create_camera_from_scene_data(msd, SESSION_RO)   # a session that never reprojects
    box, mask = _box(region, 40, 40)
    with cam.progressive(region) as pr, plain.progressive(region) as pq:
        _step(cam, pr, 10); _step(plain, pq, 10)
        _, rad, pxs, _ = _step(cam, pr, 10); _step(plain, pq, 10)
        counts = sorted(int(k) for k in np.unique(pxs[box]))
        print(f"cornell 40x40 adaptive session {region} after 10 + 10 samples: px_samples {counts}")
        assert len(counts) >= 2                                  # pixels have retired at different counts
        blob = pr.save()
        u8 = np.full((40, 40, 3), 0xA5, np.uint8)
        out = np.full((40, 40, 3), SENT, np.float32)
        wgt = np.full((40, 40), SENT, np.float32)
        assert pr.reprojected(prev_cam, prad, u8, out, wgt) is out
        want = reproject_ref(prad, prev_cam.view(), prev_cam.render_guides(), **cam.render_guides(),
                             reusable=cam.reusable_objects(), region=region, radiance=rad, px_samples=pxs)
        assert bits_equal(out[box], want["radiance"][box]).all() and (u8[box] == want["rgb"][box]).all()
        assert bits_equal(wgt[box], want["weight"][box]).all() and (wgt[box] > 0).mean() >= 0.5
        assert (out[mask] == SENT).all() and (u8[mask] == 0xA5).all() and (wgt[mask] == SENT).all()
        assert (out[box] != rad[box]).any()
        # a uniform count gives another frame: the blend really read px_samples
        uni = reproject_ref(prad, prev_cam.view(), prev_cam.render_guides(), **cam.render_guides(),
                            reusable=cam.reusable_objects(), region=region, radiance=rad, samples=20)
        assert (uni["radiance"][box] != want["radiance"][box]).any()
        # the session is as it was, and its next step is that of a session that never reprojected
        assert pr.save() == blob and pr.samples_done == 20 and pr.steps == 2
        rgb_p, rad_p, pxs_p, st_p = _step(cam, pr, 10)
        rgb_q, rad_q, pxs_q, st_q = _step(plain, pq, 10)
        assert (rgb_p == rgb_q).all() and bits_equal(rad_p, rad_q).all() and (pxs_p == pxs_q).all()
        assert (st_p.pixels, st_p.samples, st_p.bounces) == (st_q.pixels, st_q.samples, st_q.bounces)
        assert pr.save() == pq.save()


def test_session_errors(rt, gpu):
    from raytracer_amd import _lib
    sd = scene(rt, {"type": "cornell"})
    prev_cam = rt.create_camera_from_scene_data(sd, SESSION_RO)
    prad = np.zeros((40, 40, 3), np.float32)
    for mode in ("bounces", "samples"):
        cam = rt.create_camera_from_scene_data(sd, {**SESSION_RO, "mode": mode})
        with cam.progressive() as pr:
            pr.step(4)
            with pytest.raises(rt.RtError, match="not radiance") as e:
                pr.reprojected(prev_cam, prad)
            assert e.value.code == _lib.RT_ERR_INVALID
    cam = rt.create_camera_from_scene_data(sd, SESSION_RO)
    other = rt.create_camera_from_scene_data(scene(rt, {"type": "default"}), {"width": 40, "samples": 4})
    with cam.progressive() as pr:
        pr.step(4)
        for call, word in ((lambda: pr.reprojected(prev_cam, prad, sigma_plane=-1.0), "sigma_plane"),
                           (lambda: pr.reprojected(prev_cam, prad, history_samples=float("nan")), "history_samples"),
                           (lambda: pr.reprojected(prev_cam, prad, prev_region=(40, 0, 4, 4)), "empty after clamping"),
                           (lambda: pr.reprojected(other, np.zeros((other.image_height, 40, 3), np.float32)),
                            "reproject: the cameras hold different scenes")):
            with pytest.raises(rt.RtError, match=word) as e:
                call()
            assert e.value.code == _lib.RT_ERR_INVALID
        assert np.isfinite(pr.reprojected(prev_cam, prad)).all()   # the session still works
    with pytest.raises(rt.RtError, match="no progressive session is open"):
        rt.ProgressiveRender(cam).reprojected(prev_cam, prad)


# ---- 4. end to end -------------------------------------------------------------------------------------
def test_end_to_end_cornell_96_beats_the_fresh_frame(rt, gpu):
    """Cornell 96x96, depth 8, aTolerance 0, every frame from the GPU: view A = the scene's camera
    at spp 256, view B = `from` moved by (0.5, 0.2, -0.2), fresh at spp 4, truth B at spp 1024.
    The restatement on oracle frames of this size gives blend / fresh 0.1841 with 83.5 % of the
    pixels holding a history (tools/reproject_quality.py); asserted <= 0.2025, the same 10 %
    headroom as the host test."""
    sd = json.loads((GOLDEN / "scene_cornell.json").read_text())["scene"]
    ro = {"width": 96, "depth": 8, "aTolerance": 0}
    prev_cam = rt.create_camera_from_scene_data(sd, {**ro, "samples": 256})
    msd = moved_scene(sd, MOVE)
    cam = rt.create_camera_from_scene_data(msd, {**ro, "samples": 4})
    prad, fresh = render(prev_cam), render(cam)
    truth = render(rt.create_camera_from_scene_data(msd, {**ro, "samples": 1024}))
    wgt = np.zeros((96, 96), np.float32)
    out = cam.reproject(prev_cam, prad, radiance=fresh, samples=4, weight_out=wgt)
    before = display_mse(fresh, truth)
    ratio = display_mse(out, truth) / before
    share = float((wgt > 0).mean())
    print(f"cornell 96x96 on the GPU, move {MOVE}: share {share:.4f}, fresh MSE {before:.6e}, blend / fresh {ratio:.4f}")
    assert share >= 0.6
    assert ratio <= 0.2025


# ---- 5. repeatability -------------------------------------------------------------------------------------
def test_two_calls_are_identical_and_release_device_frees_the_buffers(rt, gpu):
    sd = scene(rt, {"type": "cornell"})
    ro = {"width": 40, "samples": 8, "depth": 8, "aTolerance": 0}
    prev_cam = rt.create_camera_from_scene_data(sd, ro)
    cam = rt.create_camera_from_scene_data(moved_scene(sd), ro)
    prad, fresh = render(prev_cam), render(cam)

    def call(c=cam, p=prev_cam):
        rgb = np.zeros((40, 40, 3), np.uint8)
        hist = np.zeros((40, 40, 3), np.float32)
        wgt = np.zeros((40, 40), np.float32)
        out = c.reproject(p, prad, radiance=fresh, samples=8, rgb=rgb, history_out=hist, weight_out=wgt)
        return out, rgb, hist, wgt

    first = call()
    assert (first[3] > 0).any() and (first[0] != fresh).any()
    for again in (call(),):
        assert all(bits_equal(a, b).all() for a, b in zip(first, again))
    cam.release_device(); prev_cam.release_device()
    assert all(bits_equal(a, b).all() for a, b in zip(first, call()))
    # one camera as both views: the same view gathers its own frame
    same = prev_cam.reproject(prev_cam, prad)
    g = prev_cam.render_guides()
    want = reproject_ref(prad, prev_cam.view(), g, **g, reusable=prev_cam.reusable_objects())
    assert bits_equal(same, want["history"]).all() and (same > 0).any()
