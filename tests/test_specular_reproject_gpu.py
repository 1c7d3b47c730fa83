"""Reprojection through specular chains on the GPU. Every comparison with the NumPy restatement
(tests/specular_reproject_ref.py, the normative definition) is exact: == on bits, NaN equal to NaN -
history, weight, blend, u8 and kind."""
import functools
import json
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
from denoise_ref import bits_equal, display_mse  # noqa: E402
from reproject_ref import MOVE, moved_scene, reproject_ref  # noqa: E402
from specular_reproject_ref import (PREV_REGION, REASONS, REGION, analytic_scene,  # noqa: E402
                                    cornell_without_spheres, golden_scene, mirror_room, oracle_pair,
                                    specular_reproject_ref, synthetic_call, synthetic_pair, through_from_scene)

pytestmark = pytest.mark.gpu

F = np.float32
SENT = np.float32(-123.25)
NON_DEFAULT = dict(normal_min=0.5, sigma_plane=0.05, min_weight=0.6, history_samples=8.0, point_pixels=1.5)


@functools.lru_cache(maxsize=None)
def _scene(rt, key):
    return rt.generate_scene_data(json.loads(key))


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
    """call(rgb=, out=, history_out=, weight_out=, kind=) -> blend; all five outputs against `want`
    inside the region, their sentinels outside it."""
    H, W = want["weight"].shape
    rgb = np.full((H, W, 3), 0xA5, np.uint8)
    out = np.full((H, W, 3), SENT, np.float32)
    hist = np.full((H, W, 3), SENT, np.float32)
    wgt = np.full((H, W), SENT, np.float32)
    kind = np.full((H, W), 0x5A, np.uint8)
    res = call(rgb=rgb, out=out, history_out=hist, weight_out=wgt, kind=kind)
    assert res is out
    box, mask = _box(region, H, W)
    n_h = int((~bits_equal(hist[box], want["history"][box])).any(-1).sum())
    n_w = int((~bits_equal(wgt[box], want["weight"][box])).sum())
    n_b = int((~bits_equal(out[box], want["radiance"][box])).any(-1).sum())
    n_u = int((rgb[box] != want["rgb"][box]).any(-1).sum())
    n_k = int((kind[box] != want["kind"][box]).sum())
    counts = np.bincount(want["kind"][box].ravel(), minlength=3).tolist()
    changed = int((~bits_equal(out[box], fresh[box])).any(-1).sum())
    print(f"{what}: pixels differing from the restatement: history {n_h}, weight {n_w}, blend {n_b}, u8 {n_u}, kind {n_k} "
          f"(kind 0 / 1 / 2 on {counts} pixels, {changed} changed by the blend)")
    assert n_h == 0 and n_w == 0 and n_b == 0 and n_u == 0 and n_k == 0, what
    assert (rgb[mask] == 0xA5).all() and (out[mask] == SENT).all() and (hist[mask] == SENT).all(), what
    assert (wgt[mask] == SENT).all() and (kind[mask] == 0x5A).all(), what
    return out, hist, wgt, kind


def explicit(rt, s, **kw):
    return rt.reproject_specular(s["prev_radiance"], s["prev_view"], s["prev_first"], s["prev_chain"], s["view"],
                                 s["first"], s["chain"], s["reusable"], s["through"], **kw)


# ---- 1. explicit buffers, synthetic ------------------------------------------------------------------
@pytest.mark.parametrize("opts,counts", [({}, True), (NON_DEFAULT, False)], ids=["default", "non-default"])
def test_explicit_buffers_on_the_synthetic_pair(rt, gpu, opts, counts):
    s = synthetic_pair()
    kw = dict(region=REGION, prev_region=PREV_REGION, radiance=s["fresh"], **opts)
    kw.update(px_samples=s["px_samples"]) if counts else kw.update(samples=3)
    reasons = {}
    want = synthetic_call(s, reasons=reasons, **kw)
    print(f"synthetic {opts or 'defaults'}: rejections {reasons}")
    box, mask = _box(REGION, *want["weight"].shape)
    if not opts:
        assert all(reasons[k] > 0 for k in REASONS), reasons
        assert (want["kind"][box] == 2).mean() >= 0.1 and (want["kind"][box] == 1).mean() >= 0.25
    assert (want["history"][box] > 1e29).any()       # the 1e30 tap is finite: it is gathered
    out, hist, wgt, kind = assert_is_restatement(lambda **o: explicit(rt, s, **kw, **o), want, s["fresh"], REGION,
                                                 f"synthetic {opts or 'defaults'}")
    # history only: no fresh frame, the history is returned
    kw2 = {k: v for k, v in kw.items() if k not in ("radiance", "px_samples", "samples")}
    k2 = np.zeros(kind.shape, np.uint8)
    h2 = explicit(rt, s, kind=k2, **kw2)
    assert bits_equal(h2[box], hist[box]).all() and (h2[mask] == 0).all() and (k2[box] == kind[box]).all()


def test_each_output_alone_is_the_all_outputs_call_on_the_synthetic_pair(rt, gpu):
    s = synthetic_pair()
    H, W = s["first"]["object"].shape
    kw = dict(region=REGION, prev_region=PREV_REGION, radiance=s["fresh"], px_samples=s["px_samples"])
    new = lambda: {"history_out": np.full((H, W, 3), SENT, F), "weight_out": np.full((H, W), SENT, F),   # noqa: E731
                   "out": np.full((H, W, 3), SENT, F), "rgb": np.full((H, W, 3), 0xA5, np.uint8),
                   "kind": np.full((H, W), 0x5A, np.uint8)}
    full = new()
    explicit(rt, s, **kw, **full)
    box, _ = _box(REGION, H, W)
    assert all((a[box] != new()[k][box]).any() for k, a in full.items())
    for k in full:
        one = new()
        explicit(rt, s, **kw, **{k: one[k]})
        assert bits_equal(one[k], full[k]).all(), k
    hist_only = {k: v for k, v in kw.items() if k not in ("radiance", "px_samples")}
    for keys in (("history_out",), ("weight_out",), ("kind",), ("history_out", "weight_out", "kind")):
        one = new()
        explicit(rt, s, **hist_only, **{k: one[k] for k in keys})
        assert all(bits_equal(one[k], full[k]).all() for k in keys), keys


def test_a_9x130_frame_spans_three_workgroup_columns(rt, gpu):
    s = synthetic_pair(False, (9, 130), (11, 120), 0.012, 0.05 * 41 / 120)
    kw = dict(radiance=s["fresh"], samples=3)
    want = synthetic_call(s, **kw)
    assert (want["kind"][:, 128:] == 2).any() and (want["kind"][:, :64] == 1).any() and (want["kind"][:, 64:128] > 0).any()
    assert_is_restatement(lambda **o: explicit(rt, s, **kw, **o), want, s["fresh"], None, "synthetic 9x130")


# ---- 2. the camera entry ---------------------------------------------------------------------------
SPHERES = {"type": "spheres", "options": {"count": 200, "seed": 42}}
CAMERA_CASES = {
    "analytic32": (analytic_scene, {"width": 32}, None, "specular"),
    "mirror-room40": (mirror_room, {"width": 40}, "brute", "specular"),
    "default40": (lambda: golden_scene("default"), {"width": 40}, None, {"max_bounces": 6, "max_fuzz": 0.5}),
    "spheres200-fast": (SPHERES, {"width": 48, "aspect": 1, "traversal": "fast"}, "fast", "specular"),
    "spheres200-reference": (SPHERES, {"width": 48, "aspect": 1, "traversal": "reference"}, "reference", "specular"),
}


@pytest.mark.parametrize("case", list(CAMERA_CASES))
def test_camera_entry_is_the_restatement_on_the_oracles_guides(rt, gpu, oracle, case):
    from raytracer_amd import _lib
    cfg, ro, trav, guides = CAMERA_CASES[case]
    sd = _scene(rt, json.dumps(cfg, sort_keys=True)) if isinstance(cfg, dict) else cfg()
    ro = {**ro, "samples": 8, "depth": 8, "aTolerance": 0}
    go = {"max_bounces": 8, "max_fuzz": 0.0, **(guides if isinstance(guides, dict) else {})}
    prev_cam = rt.create_camera_from_scene_data(sd, ro)
    cam = rt.create_camera_from_scene_data(moved_scene(sd), ro)
    if trav is not None:
        assert cam.info["traversal"] == _lib.TRAVERSAL[trav]
    prad, fresh = render(prev_cam), render(cam)
    H, W = cam.image_height, cam.image_width
    if case == "default40":
        assert (H, W) == (23, 40)
    g = oracle_pair(oracle, sd, {k: v for k, v in ro.items() if k in ("width", "aspect")}, MOVE, **go)
    reusable = cam.reusable_objects()
    sub, psub = (5, 3, W - 9, H - 8), (2, 1, W - 4, H - 5)
    for region, prev_region, opts in ((None, None, {}), (sub, psub, {**NON_DEFAULT, "through": 1})):
        kw = dict(region=region, prev_region=prev_region, radiance=fresh, samples=8)
        ref_kw = {k: v for k, v in opts.items() if k != "through"}
        through = through_from_scene(sd, opts.get("through", 15), go["max_fuzz"])
        assert through.tolist() == cam.through_objects(opts.get("through", 15), go["max_fuzz"]).tolist()
        want = specular_reproject_ref(prad, g["prev_view"], g["prev_first"], g["prev_chain"], g["view"], g["first"],
                                      g["chain"], reusable, through, **kw, **ref_kw)
        if region is None:
            # (the spheres' curved mirrors and glass: 84 pixels walk a chain, none finds its point)
            assert (want["kind"] == 2).any() or (case.startswith("spheres200") and (g["chain"]["chain"] & 0xff).any())
            assert (want["kind"] == 1).any() or case == "analytic32"
        assert_is_restatement(lambda **o: cam.reproject(prev_cam, prad, guides=guides, **kw, **opts, **o), want, fresh,
                              region, f"{case} region {region}")
    t = cam.reproject_times()
    assert t["guide_ms"] > 0 and t["reproject_ms"] > 0 and t["total_ms"] >= t["guide_ms"] + t["reproject_ms"]
    # the explicit-buffer call on the device's own guides gives the same frame
    gk = dict(through_specular=True, max_bounces=go["max_bounces"], max_fuzz=go["max_fuzz"])
    a = cam.reproject(prev_cam, prad, radiance=fresh, samples=8, guides=guides)
    b = rt.reproject_specular(prad, prev_cam.view(), prev_cam.render_guides(), prev_cam.render_guides(**gk), cam.view(),
                              cam.render_guides(), cam.render_guides(**gk), reusable,
                              cam.through_objects(15, go["max_fuzz"]), radiance=fresh, samples=8)
    assert bits_equal(a, b).all() and (a != fresh).any()


def test_without_specular_materials_the_call_is_todays(rt, gpu):
    sd = cornell_without_spheres()
    ro = {"width": 40, "samples": 8, "depth": 8, "aTolerance": 0}
    prev_cam = rt.create_camera_from_scene_data(sd, ro)
    cam = rt.create_camera_from_scene_data(moved_scene(sd), ro)
    prad, fresh = render(prev_cam), render(cam)
    assert not cam.through_objects().any()
    for region, prev_region, opts in ((None, None, {}), ((5, 3, 31, 32), (2, 1, 36, 35), dict(normal_min=0.5, min_weight=0.6))):
        outs = []
        for extra in ({}, {"guides": "specular"}):
            rgb = np.full((40, 40, 3), 0xA5, np.uint8)
            hist = np.full((40, 40, 3), SENT, F); wgt = np.full((40, 40), SENT, F)
            kind = np.zeros((40, 40), np.uint8)
            if extra:
                extra = {**extra, "kind": kind}
            out = cam.reproject(prev_cam, prad, region, prev_region, radiance=fresh, samples=8, rgb=rgb, history_out=hist,
                                weight_out=wgt, **opts, **extra)
            outs.append((out, rgb, hist, wgt))
        assert all(bits_equal(a, b).all() for a, b in zip(*outs))
        assert ((kind == 1) == (outs[0][3] > 0)).all() and (kind == 1).mean() > 0.3 and (kind < 2).all()


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
    sd = mirror_room()
    prev_cam = rt.create_camera_from_scene_data(sd, {**SESSION_RO, "samples": 8, "aTolerance": 0})
    prad = render(prev_cam)
    msd = moved_scene(sd)
    cam = rt.create_camera_from_scene_data(msd, SESSION_RO)
    plain = rt.create_camera_from_scene_data(msd, SESSION_RO)   # a session that never reprojects
    box, mask = _box(region, 40, 40)
    gk = dict(through_specular=True)
    with cam.progressive(region) as pr, plain.progressive(region) as pq:
        _step(cam, pr, 10); _step(plain, pq, 10)
        _, rad, pxs, _ = _step(cam, pr, 10); _step(plain, pq, 10)
        counts = sorted(int(k) for k in np.unique(pxs[box]))
        print(f"mirror room 40x40 adaptive session {region} after 10 + 10 samples: px_samples {counts}")
        assert counts == [10, 20]                                # pixels that retired after the first step, and the rest
        blob = pr.save()
        u8 = np.full((40, 40, 3), 0xA5, np.uint8)
        out = np.full((40, 40, 3), SENT, np.float32)
        wgt = np.full((40, 40), SENT, np.float32)
        kind = np.full((40, 40), 0x5A, np.uint8)
        assert pr.reprojected(prev_cam, prad, u8, out, wgt, guides="specular", kind=kind) is out
        args = (prad, prev_cam.view(), prev_cam.render_guides(), prev_cam.render_guides(**gk), cam.view(),
                cam.render_guides(), cam.render_guides(**gk), cam.reusable_objects(), cam.through_objects())
        want = specular_reproject_ref(*args, region=region, radiance=rad, px_samples=pxs)
        assert bits_equal(out[box], want["radiance"][box]).all() and (u8[box] == want["rgb"][box]).all()
        assert bits_equal(wgt[box], want["weight"][box]).all() and (kind[box] == want["kind"][box]).all()
        assert (kind[box] == 2).any() and (kind[box] == 1).mean() >= 0.3
        assert (out[mask] == SENT).all() and (u8[mask] == 0xA5).all() and (wgt[mask] == SENT).all()
        assert (kind[mask] == 0x5A).all()
        # a uniform count gives another frame: the blend really read px_samples
        uni = specular_reproject_ref(*args, region=region, radiance=rad, samples=20)
        assert (uni["radiance"][box] != want["radiance"][box]).any()
        # a second call (the session's kept guides and chain plane) and other options
        again = pr.reprojected(prev_cam, prad, guides="specular")
        assert bits_equal(again[box], out[box]).all()
        w2 = specular_reproject_ref(*args[:3], prev_cam.render_guides(through_specular=True, max_bounces=2), *args[4:6],
                                    cam.render_guides(through_specular=True, max_bounces=2), *args[7:], region=region,
                                    radiance=rad, px_samples=pxs, point_pixels=2.0)
        o2 = pr.reprojected(prev_cam, prad, guides={"max_bounces": 2}, point_pixels=2.0)
        assert bits_equal(o2[box], w2["radiance"][box]).all()
        # a following call without guides= is today's
        plain_out = pr.reprojected(prev_cam, prad)
        p_want = reproject_ref(prad, prev_cam.view(), prev_cam.render_guides(), **cam.render_guides(),
                               reusable=cam.reusable_objects(), region=region, radiance=rad, px_samples=pxs)
        assert bits_equal(plain_out[box], p_want["radiance"][box]).all()
        assert (plain_out[box] != out[box]).any()
        # the session is as it was, and its next step is that of a session that never reprojected
        assert pr.save() == blob and pr.samples_done == 20 and pr.steps == 2
        rgb_p, rad_p, pxs_p, st_p = _step(cam, pr, 10)
        rgb_q, rad_q, pxs_q, st_q = _step(plain, pq, 10)
        assert (rgb_p == rgb_q).all() and bits_equal(rad_p, rad_q).all() and (pxs_p == pxs_q).all()
        assert (st_p.pixels, st_p.samples, st_p.bounces) == (st_q.pixels, st_q.samples, st_q.bounces)
        assert pr.save() == pq.save()


def test_session_errors(rt, gpu):
    from raytracer_amd import _lib
    sd = mirror_room()
    prev_cam = rt.create_camera_from_scene_data(sd, SESSION_RO)
    prad = np.zeros((40, 40, 3), np.float32)
    for mode in ("bounces", "samples"):
        cam = rt.create_camera_from_scene_data(sd, {**SESSION_RO, "mode": mode})
        with cam.progressive() as pr:
            pr.step(4)
            with pytest.raises(rt.RtError, match="not radiance") as e:
                pr.reprojected(prev_cam, prad, guides="specular")
            assert e.value.code == _lib.RT_ERR_INVALID
    cam = rt.create_camera_from_scene_data(sd, SESSION_RO)
    other = rt.create_camera_from_scene_data(golden_scene("default"), {"width": 40, "samples": 4})
    sp = dict(guides="specular")
    with cam.progressive() as pr:
        pr.step(4)
        for call, word in ((lambda: pr.reprojected(prev_cam, prad, sigma_plane=-1.0, **sp), "sigma_plane"),
                           (lambda: pr.reprojected(prev_cam, prad, point_pixels=float("nan"), **sp), "point_pixels"),
                           (lambda: pr.reprojected(prev_cam, prad, through=16, **sp), "through"),
                           (lambda: pr.reprojected(prev_cam, prad, guides="first_hit"), "RT_GUIDES_SPECULAR"),
                           (lambda: pr.reprojected(prev_cam, prad, guides={"max_bounces": 65}), "max_bounces"),
                           (lambda: pr.reprojected(prev_cam, prad, prev_region=(40, 0, 4, 4), **sp), "empty after clamping"),
                           (lambda: pr.reprojected(other, np.zeros((other.image_height, 40, 3), np.float32), **sp),
                            "reproject: the cameras hold different scenes")):
            with pytest.raises(rt.RtError, match=word) as e:
                call()
            assert e.value.code == _lib.RT_ERR_INVALID
        assert np.isfinite(pr.reprojected(prev_cam, prad, **sp)).all()   # the session still works
    with pytest.raises(rt.RtError, match="no progressive session is open"):
        rt.ProgressiveRender(cam).reprojected(prev_cam, prad, **sp)


# ---- 4. end to end -------------------------------------------------------------------------------------
def test_end_to_end_mirror_room_64_beats_the_first_hit_reprojection(rt, gpu):
    """The mirror room 64x64, depth 8, aTolerance 0, every frame from the GPU: view A at spp 256,
    view B = `from` moved by (0.5, 0.2, -0.2), fresh at spp 4, truth B at spp 1024. The restatement on
    oracle frames of this size gives blend / fresh 0.4540 without and 0.3855 with the chains
    (tools/specular_reproject_quality.py); asserted below the first-hit ratio of the same frames and
    <= 0.424, the CPU value plus 10 %."""
    sd = mirror_room()
    ro = {"width": 64, "depth": 8, "aTolerance": 0}
    prev_cam = rt.create_camera_from_scene_data(sd, {**ro, "samples": 256})
    msd = moved_scene(sd, MOVE)
    cam = rt.create_camera_from_scene_data(msd, {**ro, "samples": 4})
    prad, fresh = render(prev_cam), render(cam)
    truth = render(rt.create_camera_from_scene_data(msd, {**ro, "samples": 1024}))
    kind = np.zeros((64, 64), np.uint8)
    first = cam.reproject(prev_cam, prad, radiance=fresh, samples=4)
    out = cam.reproject(prev_cam, prad, radiance=fresh, samples=4, guides="specular", kind=kind)
    before = display_mse(fresh, truth)
    r1, r2 = display_mse(first, truth) / before, display_mse(out, truth) / before
    print(f"mirror room 64x64 on the GPU, move {MOVE}: kind 2 on {(kind == 2).mean():.4f} of the frame, fresh MSE "
          f"{before:.6e}, blend / fresh {r1:.4f} first hit, {r2:.4f} with chains")
    assert (kind == 2).mean() >= 0.05
    assert r2 < r1
    assert r2 <= 0.424


# ---- 5. repeatability -------------------------------------------------------------------------------------
def test_two_calls_are_identical_and_release_device_frees_the_buffers(rt, gpu):
    sd = mirror_room()
    ro = {"width": 40, "samples": 8, "depth": 8, "aTolerance": 0}
    prev_cam = rt.create_camera_from_scene_data(sd, ro)
    cam = rt.create_camera_from_scene_data(moved_scene(sd), ro)
    prad, fresh = render(prev_cam), render(cam)

    def call(c=cam, p=prev_cam):
        rgb = np.zeros((40, 40, 3), np.uint8)
        hist = np.zeros((40, 40, 3), np.float32)
        wgt = np.zeros((40, 40), np.float32)
        kind = np.zeros((40, 40), np.uint8)
        out = c.reproject(p, prad, radiance=fresh, samples=8, rgb=rgb, history_out=hist, weight_out=wgt,
                          guides="specular", kind=kind)
        return out, rgb, hist, wgt, kind

    first = call()
    assert (first[4] == 2).any() and (first[4] == 1).any() and (first[0] != fresh).any()
    assert all(bits_equal(a, b).all() for a, b in zip(first, call()))
    cam.release_device(); prev_cam.release_device()
    assert all(bits_equal(a, b).all() for a, b in zip(first, call()))
    # another mask rebuilds the through table: no chain starts on the mirror (object 2) any more
    k0 = np.zeros((40, 40), np.uint8)
    cam.reproject(prev_cam, prad, guides="specular", through=2, kind=k0)
    on_mirror = cam.render_guides()["object"] == 2
    assert ((k0 == 1) == (first[4] == 1)).all() and (first[4][on_mirror] == 2).any() and (k0[on_mirror] == 0).all()
    assert all(bits_equal(a, b).all() for a, b in zip(first, call()))
    # one camera as both views: the same view gathers its own frame, in the mirror too
    ks = np.zeros((40, 40), np.uint8)
    same = prev_cam.reproject(prev_cam, prad, guides="specular", kind=ks)
    gk = dict(through_specular=True)
    want = specular_reproject_ref(prad, prev_cam.view(), prev_cam.render_guides(), prev_cam.render_guides(**gk),
                                  prev_cam.view(), prev_cam.render_guides(), prev_cam.render_guides(**gk),
                                  prev_cam.reusable_objects(), prev_cam.through_objects())
    assert bits_equal(same, want["history"]).all() and (ks == want["kind"]).all() and (ks == 2).mean() > 0.05
