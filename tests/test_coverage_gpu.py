"""Sub-pixel coverage and the filters' edge hold on the GPU. Every comparison is exact: the device's
coverage words against the restatement (tests/coverage_ref.py, the normative definition) in every
bit, and the held filter outputs - colour, u8 and variance - against hold_ref applied to the
filters' own restatements (tests/denoise_ref.py, tests/denoise_var_ref.py), == on bits."""
import functools
import json
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
from coverage_ref import agree_of, coverage_ref, hold_ref, hold_var_ref, mixed_of, objects_of  # noqa: E402
from denoise_ref import bits_equal, denoise_ref, to_u8_ref  # noqa: E402
from denoise_var_ref import denoise_var_ref  # noqa: E402

pytestmark = pytest.mark.gpu

CORNELL = {"type": "cornell"}
SPHERES200 = {"type": "spheres", "options": {"count": 200, "seed": 3}}
SPHERES200_RO = {"width": 64, "aspect": 1}
REGION = (13, 7, 24, 16)     # an odd offset; both edges cut 8x8 tiles of the region's own numbering
# name -> (scene, render options, camera-only options, precision, region)
CASES = {
    "cornell_brute": (CORNELL, {"width": 40}, {"traversal": "brute"}, "ref", None),
    "spheres200_reference": (SPHERES200, SPHERES200_RO, {"traversal": "reference"}, "ref", None),
    "spheres200_fast": (SPHERES200, SPHERES200_RO, {"traversal": "fast"}, "ref", None),
    "spheres200_brute": (SPHERES200, SPHERES200_RO, {"traversal": "brute"}, "ref", None),
    "default_aperture_planes": ({"type": "default"}, {"width": 64}, {}, "ref", None),
    "spheres200_region": (SPHERES200, SPHERES200_RO, {}, "ref", REGION),
    "spheres200_fp32": (SPHERES200, SPHERES200_RO, {}, "fp32", None),
}


@functools.lru_cache(maxsize=None)
def _scene(rt, key):
    return rt.generate_scene_data(json.loads(key))


def scene(rt, cfg):
    return _scene(rt, json.dumps(cfg, sort_keys=True))


_WORDS = {}


def words_of_oracle(rt, oracle, cfg, ro, k):
    """The restatement's full-frame coverage words, computed once per scene, size and k, read-only."""
    key = (json.dumps(cfg, sort_keys=True), json.dumps(ro, sort_keys=True), k)
    if key not in _WORDS:
        _WORDS[key] = coverage_ref(oracle, scene(rt, cfg), ro, k)
        _WORDS[key].setflags(write=False)
    return _WORDS[key]


def _box(region, H, W):
    x, y, w, h = region or (0, 0, W, H)
    box = (slice(y, y + h), slice(x, x + w))
    outside = np.ones((H, W), bool)
    outside[box] = False
    return box, outside


# ---- 1. the coverage words ---------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("name", list(CASES))
def test_coverage_words_equal_the_restatement(rt, gpu, oracle, name, k):
    cfg, ro, cam_ro, precision, region = CASES[name]
    cam = rt.create_camera_from_scene_data(scene(rt, cfg), {**ro, **cam_ro})
    if precision != "ref":
        cam.set_precision(precision)
    want = words_of_oracle(rt, oracle, cfg, ro, k)
    H, W = want.shape
    box, outside = _box(region, H, W)
    got = cam.render_coverage(region, k=k)
    assert got["agree"].dtype == np.uint16 and got["objects"].dtype == np.uint8 and got["mixed"].dtype == bool
    assert got["agree"].shape == got["objects"].shape == got["mixed"].shape == (H, W)
    bad = {"agree": int((got["agree"][box] != agree_of(want)[box]).sum()),
           "objects": int((got["objects"][box] != objects_of(want)[box]).sum()),
           "mixed": int((got["mixed"][box] != mixed_of(want, k)[box]).sum())}
    share = float(got["mixed"][box].mean())
    print(f"{name} K={k}: pixels differing from the restatement {bad}; mixed share {share:.3f}, "
          f"up to {int(got['objects'].max())} objects in a pixel")
    assert not any(bad.values()), (name, k, bad)
    assert 0 < got["mixed"][box].sum() < got["mixed"][box].size     # the comparison is not vacuous
    assert not got["agree"][outside].any() and not got["objects"][outside].any() and not got["mixed"][outside].any()
    assert cam.coverage_time() > 0.0


def test_raw_coverage_words_write_only_the_region(rt, gpu, oracle):
    from raytracer_amd import _lib
    import ctypes as C
    cam = rt.create_camera_from_scene_data(scene(rt, SPHERES200), SPHERES200_RO)
    want = words_of_oracle(rt, oracle, SPHERES200, SPHERES200_RO, 4)
    box, outside = _box(REGION, 64, 64)
    words = np.full((64, 64), 0xA5A5A5A5, np.uint32)
    reg = _lib.RtRegion(*REGION)
    _lib.check(cam._lib.rt_camera_render_coverage(cam._h, C.byref(reg), 4, words.ctypes.data))
    assert (words[box] == want[box]).all() and (words[outside] == 0xA5A5A5A5).all()


# ---- 2. the hold in the filters ------------------------------------------------------------------
CORNELL_RO = {"width": 40, "samples": 24, "depth": 8, "aTolerance": 0}


def _step(cam, pr, n):
    H, W = cam.image_height, cam.image_width
    rgb = np.zeros((H, W, 3), np.uint8)
    rad = np.zeros((H, W, 3), np.float32)
    pr.step(n, rgb, radiance=rad)
    return rgb, rad


@pytest.fixture(scope="module")
def cornell40(rt, gpu, oracle):
    """The GPU's Cornell 40x40 frame after step(4) of a session, its variance map, its guides, the
    restatement's K = 2 and K = 4 masks and both filters' restatement outputs (read-only)."""
    cam = rt.create_camera_from_scene_data(scene(rt, CORNELL), CORNELL_RO)
    with cam.progressive() as pr:
        _, rad = _step(cam, pr, 4)
        var = pr.variance()
    g = cam.render_guides()
    masks = {k: mixed_of(words_of_oracle(rt, oracle, CORNELL, {"width": 40}, k), k) for k in (2, 4)}
    plain = denoise_ref(rad, g["normal"], g["position"], g["distance"], g["object"])
    guided, guided_var = denoise_var_ref(rad, var, g["normal"], g["position"], g["distance"], g["object"])
    for a in (rad, var, *g.values(), *masks.values(), plain, guided, guided_var):
        a.setflags(write=False)
    assert 0 < masks[2].sum() < masks[4].sum() < 800
    return cam, rad, var, g, masks, plain, guided, guided_var


def assert_held(out, want, rad, mask, what):
    n_bad = int((~bits_equal(out, want)).any(-1).sum())
    n_kept = int(bits_equal(out[mask], rad[mask]).all(-1).sum())
    print(f"{what}: {n_bad} pixels differ from hold_ref of the restatement; {n_kept} of {int(mask.sum())} held pixels "
          f"are their input")
    assert n_bad == 0 and n_kept == int(mask.sum()), what
    assert (out[~mask] != rad[~mask]).any(), what


@pytest.mark.parametrize("k", [2, 4])
def test_camera_denoise_with_the_hold_is_hold_ref_of_the_restatement(rt, cornell40, k):
    cam, rad, var, g, masks, plain, guided, guided_var = cornell40
    m = masks[k]
    rgb = np.zeros((40, 40, 3), np.uint8)
    want = hold_ref(plain, rad, m)
    assert_held(cam.denoise(rad, rgb=rgb, hold_edges=k), want, rad, m, f"plain K={k}")
    assert (rgb == to_u8_ref(want)).all()
    vout = np.full((40, 40), -123.25, np.float32)
    want = hold_ref(guided, rad, m)
    out = cam.denoise(rad, rgb=rgb, variance=var, variance_out=vout, hold_edges=k)
    assert_held(out, want, rad, m, f"variance-guided K={k}")
    assert (rgb == to_u8_ref(want)).all()
    assert bits_equal(vout, hold_var_ref(guided_var, var, m)).all() and bits_equal(vout[m], var[m]).all()
    # the outputs aliased onto the inputs
    buf, vbuf = rad.copy(), var.copy()
    assert cam.denoise(buf, out=buf, variance=vbuf, variance_out=vbuf, hold_edges=k) is buf
    assert bits_equal(buf, want).all() and bits_equal(vbuf, vout).all()


def test_a_held_pixel_keeps_a_non_finite_colour_and_a_sanitised_variance(rt, cornell40):
    cam, rad, var, g, masks, *_ = cornell40
    m = masks[2]
    ys, xs = np.nonzero(m)
    c, v = rad.copy(), var.copy()
    c[ys[0], xs[0], 1] = np.nan
    c[ys[1], xs[1], 2] = np.inf
    v[ys[0], xs[0]], v[ys[2], xs[2]], v[ys[3], xs[3]] = 7.5, -1.5, np.nan
    want, want_v = denoise_var_ref(c, v, g["normal"], g["position"], g["distance"], g["object"])
    vout = np.zeros((40, 40), np.float32)
    out = cam.denoise(c, variance=v, variance_out=vout, hold_edges=2)
    assert bits_equal(out, hold_ref(want, c, m)).all() and bits_equal(vout, hold_var_ref(want_v, v, m)).all()
    assert np.isnan(out[ys[0], xs[0], 1]) and np.isinf(out[ys[1], xs[1], 2])
    assert vout[ys[0], xs[0]] == 7.5 and vout[ys[2], xs[2]] == 0 and vout[ys[3], xs[3]] == 0


def test_denoise_with_an_explicit_mask_and_a_region(rt, cornell40):
    cam, rad, var, g, masks, *_ = cornell40
    region = (5, 3, 29, 31)
    box, outside = _box(region, 40, 40)
    rng = np.random.default_rng(3)
    mask = rng.random((40, 40)) < 0.3                    # any mask, not only a coverage mask
    inside = mask & ~outside
    want = hold_ref(denoise_ref(rad, g["normal"], g["position"], g["distance"], g["object"], region=region), rad, inside)
    rgb = np.full((40, 40, 3), 0xA5, np.uint8)
    out = rt.denoise(rad, **g, region=region, rgb=rgb, hold=mask)
    assert bits_equal(out, want).all() and (rgb[box] == to_u8_ref(want[box])).all() and (rgb[outside] == 0xA5).all()
    want, want_v = denoise_var_ref(rad, var, g["normal"], g["position"], g["distance"], g["object"], region=region)
    vout = np.full((40, 40), -123.25, np.float32)
    out = rt.denoise(rad, **g, region=region, variance=var, variance_out=vout, hold=mask.astype(np.uint8) * 200)
    assert bits_equal(out, hold_ref(want, rad, inside)).all()
    assert bits_equal(vout[box], hold_var_ref(want_v, var, inside)[box]).all()
    assert (vout[outside] == np.float32(-123.25)).all()
    # the camera call over the same region: its own mask
    inside = masks[2] & ~outside
    want = hold_ref(denoise_ref(rad, g["normal"], g["position"], g["distance"], g["object"], region=region), rad, inside)
    assert bits_equal(cam.denoise(rad, region, hold_edges=2), want).all()


def test_hold_edges_0_is_the_call_without_it(rt, cornell40):
    cam, rad, var, g, masks, plain, guided, guided_var = cornell40
    assert bits_equal(cam.denoise(rad, hold_edges=0), plain).all()
    vout = np.zeros((40, 40), np.float32)
    assert bits_equal(cam.denoise(rad, variance=var, variance_out=vout, hold_edges=0), guided).all()
    assert bits_equal(vout, guided_var).all()
    nothing = np.zeros((40, 40), np.uint8)
    assert bits_equal(rt.denoise(rad, **g, hold=nothing), plain).all()


def test_the_mask_is_first_hit_whatever_the_guides_are(rt, cornell40):
    cam, rad, var, g, masks, *_ = cornell40
    spec = cam.denoise(rad, guides="specular")
    assert bits_equal(cam.denoise(rad, guides="specular", hold_edges=2), hold_ref(spec, rad, masks[2])).all()


# ---- 3. the session ------------------------------------------------------------------------------
def test_progressive_denoised_with_the_hold_and_the_session_left_alone(rt, gpu, cornell40):
    _, _, _, g, masks, *_ = cornell40
    sd = scene(rt, CORNELL)
    cam = rt.create_camera_from_scene_data(sd, CORNELL_RO)
    twin = rt.create_camera_from_scene_data(sd, CORNELL_RO)   # a session that never calls denoised()
    gd = (g["normal"], g["position"], g["distance"], g["object"])
    with cam.progressive() as pr, twin.progressive() as pq:
        for step in range(3):
            rgb, rad = _step(cam, pr, 4)
            rgb_q, rad_q = _step(twin, pq, 4)
            assert (rgb == rgb_q).all() and bits_equal(rad, rad_q).all(), step
            var = pr.variance()
            k = (2, 4, 2)[step]          # the kept mask is replaced when k changes, and comes back
            m = masks[k]
            u8 = np.zeros((40, 40, 3), np.uint8)
            vout = np.full((40, 40), -123.25, np.float32)
            out = pr.denoised(u8, variance=True, variance_out=vout, hold_edges=k)
            want, want_v = denoise_var_ref(rad, var, *gd)
            assert_held(out, hold_ref(want, rad, m), rad, m, f"session step {step} K={k}")
            assert (u8 == to_u8_ref(hold_ref(want, rad, m))).all()
            assert bits_equal(vout, hold_var_ref(want_v, var, m)).all()
            # the kept mask serves the plain form and a second call
            want = hold_ref(denoise_ref(rad, *gd), rad, m)
            assert bits_equal(pr.denoised(hold_edges=k), want).all() and bits_equal(pr.denoised(hold_edges=k), want).all()
            assert bits_equal(pr.denoised(), denoise_ref(rad, *gd)).all()       # and no hold is no hold
            assert pr.samples_done == 4 * (step + 1) and pr.steps == step + 1
        assert cam.coverage_time() > 0.0


def test_progressive_denoised_with_the_hold_of_a_region_session(rt, gpu, cornell40):
    _, _, _, g, masks, *_ = cornell40
    region = (5, 3, 29, 31)
    box, outside = _box(region, 40, 40)
    cam = rt.create_camera_from_scene_data(scene(rt, CORNELL), CORNELL_RO)
    with cam.progressive(region) as pr:
        _, rad = _step(cam, pr, 4)
        u8 = np.full((40, 40, 3), 0xA5, np.uint8)
        out = np.full((40, 40, 3), -123.25, np.float32)
        assert pr.denoised(u8, out, hold_edges=2) is out
        want = hold_ref(denoise_ref(rad, g["normal"], g["position"], g["distance"], g["object"], region=region), rad,
                        masks[2] & ~outside)
        assert bits_equal(out[box], want[box]).all() and (u8[box] == to_u8_ref(want[box])).all()
        assert (out[outside] == np.float32(-123.25)).all() and (u8[outside] == 0xA5).all()


def test_session_hold_errors(rt, gpu):
    from raytracer_amd import _lib
    cam = rt.create_camera_from_scene_data(scene(rt, CORNELL), CORNELL_RO)
    with cam.progressive() as pr:
        pr.step(1)
        for call, word in ((lambda: pr.denoised(hold_edges=3), "hold_k must be 0, 2 or 4"),
                           (lambda: pr.denoised(variance=True, hold_edges=8), "hold_k must be 0, 2 or 4"),
                           (lambda: pr.denoised(variance=True, hold_edges=2), "samples_done < 2")):
            with pytest.raises(rt.RtError, match=word) as e:
                call()
            assert e.value.code == _lib.RT_ERR_INVALID
        pr.step(1)
        assert (pr.denoised(variance=True, hold_edges=2) != 0).any()
