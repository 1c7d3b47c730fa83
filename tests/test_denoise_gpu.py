"""Guide buffers and the a-trous filter on the GPU. Every comparison is exact (== on bits, NaN
equal to NaN): the guides against the CPU oracle's world_hit, the filter against its NumPy
restatement (tests/denoise_ref.py, the normative definition)."""
import ctypes as C
import functools
import json
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
from denoise_ref import (bits_equal, denoise_ref, display_mse, distance_ref, leak_frame, oracle_guides,  # noqa: E402
                         to_u8_ref)

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"
REGION = (5, 3, 29, 31)
CORNELL = {"type": "cornell"}
SPHERES200 = {"type": "spheres", "options": {"count": 200, "seed": 3}}
SPHERES200_RO = {"width": 48, "aspect": 1}
GUIDE_SCENES = {
    "cornell_brute": (CORNELL, {"width": 40}),
    "spheres200_lds_tree": (SPHERES200, SPHERES200_RO),
    "default_aperture_planes": ({"type": "default"}, {"width": 40}),
    # (seeded: an unseeded scene is random, and a failure must be reproducible)
    "spheres6000_global_tree": ({"type": "spheres", "options": {"count": 6000, "seed": 3}}, {"width": 32}),
}


@functools.lru_cache(maxsize=None)
def _scene(rt, key):
    return rt.generate_scene_data(json.loads(key))


def scene(rt, cfg):
    return _scene(rt, json.dumps(cfg, sort_keys=True))


_ORACLE_GUIDES = {}


def guides_of_oracle(rt, oracle, cfg, ro):
    """(normal, position, distance, object, hit) of the oracle, computed once, read-only."""
    key = (json.dumps(cfg, sort_keys=True), json.dumps(ro, sort_keys=True))
    if key not in _ORACLE_GUIDES:
        g = oracle_guides(oracle, scene(rt, cfg), ro)
        for a in g:
            a.setflags(write=False)
        _ORACLE_GUIDES[key] = g
    return _ORACLE_GUIDES[key]


def assert_guides_are_oracle(g, ref, what, box=None):
    n, P, dist, obj, hit = ref
    ys, xs = box or (slice(None), slice(None))
    bad = {"hit": int(((g["object"][ys, xs] >= 0) != hit[ys, xs]).sum()),
           "normal": int((g["normal"][ys, xs] != n[ys, xs]).any(-1).sum()),
           "position": int((g["position"][ys, xs] != P[ys, xs]).any(-1).sum()),
           "distance": int((g["distance"][ys, xs] != dist[ys, xs]).sum()),
           "object": int((g["object"][ys, xs] != obj[ys, xs]).sum())}
    print(f"{what}: {int(hit[ys, xs].sum())} hits of {hit[ys, xs].size} pixels; pixels differing from the oracle: {bad}")
    assert not any(bad.values()), (what, bad)
    miss = ~hit[ys, xs]
    assert (g["normal"][ys, xs][miss] == 0).all() and (g["position"][ys, xs][miss] == 0).all()
    assert (g["distance"][ys, xs][miss] == 0).all() and (g["object"][ys, xs][miss] == -1).all()


# ---- 1. guides ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GUIDE_SCENES))
def test_guides_equal_the_oracle(rt, gpu, oracle, name):
    cfg, ro = GUIDE_SCENES[name]
    cam = rt.create_camera_from_scene_data(scene(rt, cfg), ro)
    ref = guides_of_oracle(rt, oracle, cfg, ro)
    g = cam.render_guides()
    assert g["normal"].dtype == np.float32 and g["object"].dtype == np.int32
    assert g["object"].shape == (cam.image_height, cam.image_width)
    assert_guides_are_oracle(g, ref, name)
    assert len(np.unique(g["object"])) > 2  # (several objects in view: the comparison is not vacuous)


def test_cornell_guide_rays_are_get_ray_of_one_sample(rt, oracle):
    """The ray the guide pass defines is Camera.getRay of a `samples: 1` camera."""
    sd, ro = scene(rt, CORNELL), {"width": 40, "samples": 1}
    ci = oracle.camera_info(sd, ro)
    f = np.float32
    p00, du, dv, cen = (np.asarray(ci[k], dtype=f) for k in ("pixel00", "du", "dv", "center"))
    for i, j in [(0, 0), (39, 39), (17, 5), (3, 28)]:
        d = ((p00 + du * f(i)).astype(f) + (dv * f(j)).astype(f)).astype(f) - cen
        o_ref, d_ref = oracle.get_ray(sd, ro, i, j, 0)
        assert (np.asarray(o_ref, f) == cen).all() and (np.asarray(d_ref, f) == d).all()


def test_guides_do_not_depend_on_traversal_or_precision(rt, gpu, oracle):
    ref = guides_of_oracle(rt, oracle, SPHERES200, SPHERES200_RO)
    sd = scene(rt, SPHERES200)
    for trav in ("reference", "fast", "brute"):
        cam = rt.create_camera_from_scene_data(sd, {**SPHERES200_RO, "traversal": trav})
        assert_guides_are_oracle(cam.render_guides(), ref, f"traversal {trav}")
    cam = rt.create_camera_from_scene_data(sd, SPHERES200_RO)
    cam.set_precision("fp32")
    assert_guides_are_oracle(cam.render_guides(), ref, "precision fp32")


def test_guides_of_a_region_leave_the_rest_untouched(rt, gpu, oracle):
    from raytracer_amd import _lib
    cam = rt.create_camera_from_scene_data(scene(rt, SPHERES200), SPHERES200_RO)
    ref = guides_of_oracle(rt, oracle, SPHERES200, SPHERES200_RO)
    H, W = cam.image_height, cam.image_width
    g = {"normal": np.full((H, W, 3), -123.25, np.float32), "position": np.full((H, W, 3), -123.25, np.float32),
         "distance": np.full((H, W), -123.25, np.float32), "object": np.full((H, W), -7, np.int32)}
    reg = _lib.RtRegion(*REGION)
    _lib.check(cam._lib.rt_camera_render_guides(cam._h, C.byref(reg), g["normal"].ctypes.data, g["position"].ctypes.data,
                                                g["distance"].ctypes.data, g["object"].ctypes.data))
    x, y, w, h = REGION
    box = (slice(y, y + h), slice(x, x + w))
    assert_guides_are_oracle(g, ref, "region", box)
    mask = np.ones((H, W), bool)
    mask[box] = False
    assert (g["normal"][mask] == np.float32(-123.25)).all() and (g["position"][mask] == np.float32(-123.25)).all()
    assert (g["distance"][mask] == np.float32(-123.25)).all() and (g["object"][mask] == -7).all()
    # the Python method: zeros / -1 outside the region
    gp = cam.render_guides(REGION)
    assert (gp["object"][mask] == -1).all() and (gp["normal"][box] == g["normal"][box]).all()
    # any output may be omitted
    obj = np.full((H, W), -7, np.int32)
    _lib.check(cam._lib.rt_camera_render_guides(cam._h, None, None, None, None, obj.ctypes.data))
    assert (obj == ref[3]).all()


# ---- 2. the filter against its restatement -----------------------------------------------------
def assert_filter_is_restatement(rt, c, n, P, dist, obj, what, region=None, **opts):
    H, W = obj.shape
    rgb = np.full((H, W, 3), 0xA5, np.uint8)
    out = rt.denoise(c, n, P, dist, obj, region=region, rgb=rgb, **opts)
    want = denoise_ref(c, n, P, dist, obj, region=region, **opts)
    n_bad = int((~bits_equal(out, want)).any(-1).sum())
    x, y, w, h = region or (0, 0, W, H)
    box = (slice(y, y + h), slice(x, x + w))
    n_u8 = int((rgb[box] != to_u8_ref(want[box])).any(-1).sum())
    changed = int((~bits_equal(out, c)).any(-1).sum())
    print(f"{what} {opts}: pixels differing from the restatement: radiance {n_bad}, u8 {n_u8} "
          f"({changed} pixels changed by the filter)")
    assert n_bad == 0 and n_u8 == 0, what
    mask = np.ones((H, W), bool)
    mask[box] = False
    assert (rgb[mask] == 0xA5).all() and bits_equal(out[mask], c[mask]).all(), what
    return out


@pytest.fixture(scope="module")
def cornell40(rt, gpu):
    """The GPU's Cornell 40x40 spp 8 frame and guides (read-only)."""
    cam = rt.create_camera_from_scene_data(scene(rt, CORNELL), {"width": 40, "samples": 8, "depth": 8, "aTolerance": 0})
    rgb = np.zeros((40, 40, 3), np.uint8)
    rad = np.zeros((40, 40, 3), np.float32)
    cam.render(rgb, radiance=rad)
    g = cam.render_guides()
    for a in (rad, *g.values()):
        a.setflags(write=False)
    return cam, rad, g


@pytest.mark.parametrize("levels", [1, 2, 3, 4, 6])
def test_filter_of_a_cornell_frame(rt, cornell40, levels):
    """Steps 1 and 2 are LDS-staged, 4 and up read global memory; step 8 and above reaches
    outside a 40-pixel frame, so whole rows and columns of taps are skipped."""
    _, rad, g = cornell40
    out = assert_filter_is_restatement(rt, rad, g["normal"], g["position"], g["distance"], g["object"], "cornell40",
                                       levels=levels)
    assert (out != rad).any()


def test_filter_of_a_region(rt, cornell40):
    _, rad, g = cornell40
    assert_filter_is_restatement(rt, rad, g["normal"], g["position"], g["distance"], g["object"], "cornell40 region",
                                 region=REGION)


def synthetic_frame(H=23, W=37):
    f = np.float32
    rng = np.random.default_rng(11)
    s = f(1) / np.sqrt(f(3))
    dirs = np.array([[a, b, c] for a in (-s, s) for b in (-s, s) for c in (-s, s)], dtype=f)  # 8 unit directions
    n = dirs[rng.integers(0, 8, (H, W))]
    x = np.arange(W, dtype=f)[None, :]
    y = np.arange(H, dtype=f)[:, None]
    P = np.stack(np.broadcast_arrays(x * f(0.1), y * f(0.1), f(5) + x * f(0.03) + y * f(0.02)), -1).astype(f)  # a tilted plane
    obj = rng.integers(0, 5, (H, W)).astype(np.int32)
    miss = rng.random((H, W)) < 0.1
    obj[miss] = -1
    n[miss] = 0
    P[miss] = 0
    dist = distance_ref(P, np.zeros(3, f), obj)
    c = (rng.random((H, W, 3), dtype=f) * f(20)).astype(f)
    c[5, 7, 0] = np.nan
    c[12, 30, 1] = np.inf
    c[20, 3, 2] = 1e30
    return c, n, P, dist, obj


def test_filter_of_a_synthetic_frame_with_non_finite_pixels(rt, gpu):
    c, n, P, dist, obj = synthetic_frame()
    assert 20 < int((obj < 0).sum()) < 200
    for levels in (1, 4):
        out = assert_filter_is_restatement(rt, c, n, P, dist, obj, "synthetic", levels=levels, sigma_color=0.1,
                                           sigma_plane=0.05)
    # the non-finite pixels stay in their own pixel, as they came
    bad = ~np.isfinite(out).all(-1)
    assert int(bad.sum()) == 2 and bad[5, 7] and bad[12, 30] and out[20, 3, 2] == np.float32(1e30)


def test_filter_of_a_synthetic_frame_wider_than_a_row_group(rt, gpu):
    """70x21: the global kernel (step 4) covers 64 pixels of 4 rows per workgroup, so 70 crosses
    its row group and the 16-pixel tiles with a ragged edge, 21 its 4 rows and a tile."""
    c, n, P, dist, obj = synthetic_frame(21, 70)
    assert_filter_is_restatement(rt, c, n, P, dist, obj, "synthetic 70x21", levels=3, sigma_color=0.1, sigma_plane=0.05)


def test_filter_returns_the_leak_frame_unchanged(rt, gpu):
    c, n, P, dist, obj = leak_frame()
    out = assert_filter_is_restatement(rt, c, n, P, dist, obj, "leak frame", levels=4)
    assert bits_equal(out, c).all()


# ---- 3. the camera entry -------------------------------------------------------------------------
def test_camera_denoise_is_denoise_with_its_guides(rt, cornell40):
    cam, rad, g = cornell40
    want = rt.denoise(rad, **g)
    rgb = np.zeros((40, 40, 3), np.uint8)
    out = cam.denoise(rad, rgb=rgb)
    assert out is not rad and bits_equal(out, want).all() and (out != rad).any()
    assert (rgb == to_u8_ref(want)).all()
    # the output aliased onto the input
    buf = rad.copy()
    assert cam.denoise(buf, out=buf) is buf and bits_equal(buf, want).all()
    buf = rad.copy()
    rt.denoise(buf, **g, out=buf)
    assert bits_equal(buf, want).all()
    # a region, and non-default parameters
    o = dict(levels=2, sigma_color=0.2, sigma_plane=0.02)
    assert bits_equal(cam.denoise(rad, REGION, **o), rt.denoise(rad, **g, region=REGION, **o)).all()
    # release_device frees the filter's buffers; the next call re-creates them
    cam.release_device()
    assert bits_equal(cam.denoise(rad), want).all()


# ---- 4. progressive ------------------------------------------------------------------------------
PROG_RO = {"width": 40, "samples": 24, "depth": 8, "aTolerance": 0}


def _step(cam, pr, n):
    H, W = cam.image_height, cam.image_width
    rgb = np.zeros((H, W, 3), np.uint8)
    rad = np.zeros((H, W, 3), np.float32)
    st = pr.step(n, rgb, radiance=rad)
    return rgb, rad, st


def test_progressive_denoised_is_denoise_of_the_step_and_leaves_the_session_alone(rt, gpu):
    sd = scene(rt, CORNELL)
    cam = rt.create_camera_from_scene_data(sd, PROG_RO)
    plain = rt.create_camera_from_scene_data(sd, PROG_RO)  # a session that never calls denoised()
    helper = rt.create_camera_from_scene_data(sd, PROG_RO)
    blob = None
    with cam.progressive() as pr, plain.progressive() as pq:
        for k in range(3):
            rgb, rad, st = _step(cam, pr, 8)
            rgb_q, rad_q, st_q = _step(plain, pq, 8)
            assert (rgb == rgb_q).all() and bits_equal(rad, rad_q).all(), k
            assert (st.pixels, st.samples, st.bounces) == (st_q.pixels, st_q.samples, st_q.bounces), k
            u8 = np.zeros((40, 40, 3), np.uint8)
            out = pr.denoised(u8)
            want = helper.denoise(rad)
            assert bits_equal(out, want).all() and (u8 == to_u8_ref(want)).all(), k
            assert (out != rad).any()
            assert pr.samples_done == 8 * (k + 1) and pr.steps == k + 1
            if k == 0:
                blob = pr.save()
                o = dict(levels=2, sigma_color=0.25)  # the kept guides serve other parameters too
                assert bits_equal(pr.denoised(**o), helper.denoise(rad, **o)).all()
        assert pr.done and pq.done
    # after resume(blob): the restored session's frame at 8 samples, filtered
    other = rt.create_camera_from_scene_data(sd, PROG_RO)
    with other.resume(blob) as pr:
        rgb8, rad8, _ = _step(helper, helper.progressive(), 8)
        assert bits_equal(pr.denoised(), helper.denoise(rad8)).all()
        rgb, rad, _ = _step(other, pr, 8)
        assert pr.samples_done == 16


def test_progressive_denoised_of_a_region_session(rt, gpu):
    cam = rt.create_camera_from_scene_data(scene(rt, CORNELL), PROG_RO)
    x, y, w, h = REGION
    box = (slice(y, y + h), slice(x, x + w))
    with cam.progressive(REGION) as pr:
        _, rad, _ = _step(cam, pr, 8)
        u8 = np.full((40, 40, 3), 0xA5, np.uint8)
        out = np.full((40, 40, 3), -123.25, np.float32)
        assert pr.denoised(u8, out) is out
        want = cam.denoise(rad, REGION)
        assert bits_equal(out[box], want[box]).all() and (u8[box] == to_u8_ref(want[box])).all()
        mask = np.ones((40, 40), bool)
        mask[box] = False
        assert (out[mask] == np.float32(-123.25)).all() and (u8[mask] == 0xA5).all()


def test_progressive_denoised_refuses_frames_that_are_not_radiance(rt, gpu):
    from raytracer_amd import _lib
    for mode in ("bounces", "samples"):
        cam = rt.create_camera_from_scene_data(scene(rt, CORNELL), {**PROG_RO, "mode": mode})
        with cam.progressive() as pr:
            pr.step(8)
            with pytest.raises(rt.RtError, match="not radiance") as e:
                pr.denoised()
            assert e.value.code == _lib.RT_ERR_INVALID


# ---- 5. end to end -------------------------------------------------------------------------------
def test_end_to_end_cornell_128_equals_the_restatement_of_the_oracle_frame(rt, gpu, oracle):
    """cam.denoise of the GPU's spp 4 frame = denoise_ref of the oracle's frame with the
    oracle's guides, bit for bit; so the ratio is the CPU test's (0.2158). The converged frame
    of the metric is rendered on the GPU."""
    sd = json.loads((GOLDEN / "scene_cornell.json").read_text())["scene"]
    ro = {"width": 128, "samples": 4, "depth": 8, "aTolerance": 0}
    cam = rt.create_camera_from_scene_data(sd, ro)
    rgb = np.zeros((128, 128, 3), np.uint8)
    rad = np.zeros((128, 128, 3), np.float32)
    cam.render(rgb, radiance=rad)
    out = cam.denoise(rad)
    noisy = oracle.render(sd, ro, threads=8)["radiance"]
    n, P, dist, obj, _ = oracle_guides(oracle, sd, ro)
    want = denoise_ref(noisy, n, P, dist, obj)
    n_bad = int((~bits_equal(out, want)).any(-1).sum())
    conv = np.zeros((128, 128, 3), np.float32)
    rt.create_camera_from_scene_data(sd, {**ro, "samples": 1024}).render(rgb, radiance=conv)
    before, after = display_mse(rad, conv), display_mse(out, conv)
    print(f"cornell 128x128 spp4: {n_bad} pixels differ from the restatement of the oracle frame; "
          f"MSE {before:.6e} -> {after:.6e}, ratio {after / before:.4f}")
    assert n_bad == 0
    assert after / before <= 0.25
