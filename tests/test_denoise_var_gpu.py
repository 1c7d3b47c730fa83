"""Variance map and variance-guided filter on the GPU. Every comparison is exact (== on bits, NaN
equal to NaN): the variance map against the restatement's evaluation of the session's own
checkpoint blob, the filter - colour and variance - against its NumPy restatement
(tests/denoise_var_ref.py, the normative definition)."""
import functools
import json
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
from denoise_ref import (bits_equal, denoise_ref, display_mse, distance_ref, oracle_guides,  # noqa: E402
                         to_u8_ref)
from denoise_var_ref import denoise_var_ref, samples_from_blob, variance_from_blob  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"
REGION = (5, 3, 29, 31)
CORNELL = {"type": "cornell"}
CORNELL_RO = {"width": 40, "samples": 24, "depth": 8, "aTolerance": 0}
SPHERES200 = {"type": "spheres", "options": {"count": 200, "seed": 3}}
SPHERES200_RO = {"width": 48, "aspect": 1, "samples": 50, "depth": 8}   # the reference's adaptive defaults (0.05, 10)


@functools.lru_cache(maxsize=None)
def _scene(rt, key):
    return rt.generate_scene_data(json.loads(key))


def scene(rt, cfg):
    return _scene(rt, json.dumps(cfg, sort_keys=True))


def _step(cam, pr, n):
    H, W = cam.image_height, cam.image_width
    rgb = np.zeros((H, W, 3), np.uint8)
    rad = np.zeros((H, W, 3), np.float32)
    st = pr.step(n, rgb, radiance=rad)
    return rgb, rad, st


def _box(region, H, W):
    x, y, w, h = region or (0, 0, W, H)
    box = (slice(y, y + h), slice(x, x + w))
    mask = np.ones((H, W), bool)
    mask[box] = False
    return box, mask


# ---- 1. the variance map -----------------------------------------------------------------------
def assert_variance_is_blob_variance(pr, what):
    got = pr.variance()
    want = variance_from_blob(pr.save())
    n_bad = int((~bits_equal(got, want)).sum())
    print(f"{what}: {n_bad} of {got.size} variances differ from the restatement of the blob; "
          f"{int((got > 0).sum())} positive, max {got.max():.3e}")
    assert got.dtype == np.float32 and got.shape == want.shape
    assert n_bad == 0 and (got > 0).any() and np.isfinite(got).all() and (got >= 0).all(), what
    return got


def test_variance_of_a_cornell_session(rt, gpu):
    cam = rt.create_camera_from_scene_data(scene(rt, CORNELL), CORNELL_RO)
    with cam.progressive() as pr:
        pr.step(4)
        assert_variance_is_blob_variance(pr, "cornell 40x40 after step(4)")
        out = np.full((40, 40), -123.25, np.float32)
        assert pr.variance(out) is out and bits_equal(out, variance_from_blob(pr.save())).all()


def test_variance_of_an_adaptive_session_uses_each_pixels_own_n(rt, gpu):
    cam = rt.create_camera_from_scene_data(scene(rt, SPHERES200), SPHERES200_RO)
    with cam.progressive() as pr:
        pr.step(20)
        blob = pr.save()
        n = samples_from_blob(blob)
        counts = {int(k): int((n == k).sum()) for k in np.unique(n)}
        print(f"spheres-200 48x48 adaptive after step(20): pixels by sample count {counts}")
        assert len(counts) >= 2 and set(counts) <= {10, 20}   # pixels have retired at different n
        var = assert_variance_is_blob_variance(pr, "spheres-200 adaptive")
        pr.step(5)   # a retired pixel keeps the variance it retired with
        later = pr.variance()
        assert bits_equal(later[n == 10], var[n == 10]).all() and (later[n == 20] != var[n == 20]).any()


def test_variance_of_a_region_session_writes_only_the_region(rt, gpu):
    cam = rt.create_camera_from_scene_data(scene(rt, CORNELL), CORNELL_RO)
    box, mask = _box(REGION, 40, 40)
    with cam.progressive(REGION) as pr:
        pr.step(4)
        var = assert_variance_is_blob_variance(pr, "cornell region session")
        assert (var[mask] == 0).all() and (var[box] > 0).any()
        out = np.full((40, 40), -123.25, np.float32)
        pr.variance(out)
        assert (out[mask] == np.float32(-123.25)).all() and bits_equal(out[box], var[box]).all()


def test_variance_needs_two_samples_and_a_radiance_frame(rt, gpu):
    from raytracer_amd import _lib
    cam = rt.create_camera_from_scene_data(scene(rt, CORNELL), CORNELL_RO)
    with cam.progressive() as pr:
        for done in (0, 1):
            assert pr.samples_done == done
            for call in (pr.variance, lambda: pr.denoised(variance=True)):
                with pytest.raises(rt.RtError, match="samples_done < 2") as e:
                    call()
                assert e.value.code == _lib.RT_ERR_INVALID
            pr.step(1)
        assert pr.samples_done == 2 and (pr.variance() > 0).any()
    for mode in ("bounces", "samples"):
        cam = rt.create_camera_from_scene_data(scene(rt, CORNELL), {**CORNELL_RO, "mode": mode})
        with cam.progressive() as pr:
            pr.step(8)
            for call in (pr.variance, lambda: pr.denoised(variance=True)):
                with pytest.raises(rt.RtError, match="not radiance") as e:
                    call()
                assert e.value.code == _lib.RT_ERR_INVALID


# ---- 2. the filter against its restatement -----------------------------------------------------
def assert_filter_is_restatement(rt, c, var, n, P, dist, obj, what, region=None, **opts):
    H, W = obj.shape
    rgb = np.full((H, W, 3), 0xA5, np.uint8)
    vout = np.full((H, W), -123.25, np.float32)
    out = rt.denoise(c, n, P, dist, obj, region=region, rgb=rgb, variance=var, variance_out=vout, **opts)
    want, want_v = denoise_var_ref(c, var, n, P, dist, obj, region=region, **opts)
    box, mask = _box(region, H, W)
    n_bad = int((~bits_equal(out, want)).any(-1).sum())
    n_var = int((~bits_equal(vout[box], want_v[box])).sum())
    n_u8 = int((rgb[box] != to_u8_ref(want[box])).any(-1).sum())
    changed = int((~bits_equal(out, c)).any(-1).sum())
    print(f"{what} {opts}: pixels differing from the restatement: radiance {n_bad}, variance {n_var}, u8 {n_u8} "
          f"({changed} pixels changed by the filter)")
    assert n_bad == 0 and n_var == 0 and n_u8 == 0, what
    assert (rgb[mask] == 0xA5).all() and bits_equal(out[mask], c[mask]).all(), what
    assert (vout[mask] == np.float32(-123.25)).all(), what
    return out, vout


@pytest.fixture(scope="module")
def cornell40(rt, gpu):
    """The GPU's Cornell 40x40 frame after step(8) of a session, its variance map and its guides
    (read-only)."""
    cam = rt.create_camera_from_scene_data(scene(rt, CORNELL), CORNELL_RO)
    with cam.progressive() as pr:
        _, rad, _ = _step(cam, pr, 8)
        var = pr.variance()
    g = cam.render_guides()
    for a in (rad, var, *g.values()):
        a.setflags(write=False)
    return cam, rad, var, g


@pytest.mark.parametrize("levels", [1, 2, 3, 4, 6])
def test_filter_of_a_cornell_frame(rt, cornell40, levels):
    """Steps 1 and 2 are LDS-staged, 4 and up read global memory; step 8 and above reaches
    outside a 40-pixel frame, so whole rows and columns of taps are skipped."""
    _, rad, var, g = cornell40
    out, vout = assert_filter_is_restatement(rt, rad, var, g["normal"], g["position"], g["distance"], g["object"],
                                             "cornell40", levels=levels)
    assert (out != rad).any() and (vout < var).any()


def test_filter_of_a_region(rt, cornell40):
    """29x31 at (5, 3): tile edges inside it, partial tiles, narrower than a 64-pixel row."""
    _, rad, var, g = cornell40
    assert_filter_is_restatement(rt, rad, var, g["normal"], g["position"], g["distance"], g["object"],
                                 "cornell40 region", region=REGION)


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
    var = (rng.random((H, W), dtype=f) * f(30)).astype(f)
    var[2, 2] = np.nan
    var[3, 9] = -1.5
    var[4, 16] = np.inf
    var[6:9, 20:24] = 0
    var[5, 7] = 7.5   # the NaN pixel's own variance is kept
    return c, var, n, P, dist, obj


def test_filter_of_a_synthetic_frame_with_non_finite_pixels(rt, gpu):
    c, var, n, P, dist, obj = synthetic_frame()
    assert 20 < int((obj < 0).sum()) < 200
    for levels in (1, 4):
        out, vout = assert_filter_is_restatement(rt, c, var, n, P, dist, obj, "synthetic", levels=levels,
                                                 sigma_variance=0.7, sigma_plane=0.05)
    # the non-finite pixels stay in their own pixel, as they came, with their variance
    bad = ~np.isfinite(out).all(-1)
    assert int(bad.sum()) == 2 and bad[5, 7] and bad[12, 30] and out[20, 3, 2] == np.float32(1e30)
    assert vout[5, 7] == np.float32(7.5) and vout[12, 30] == var[12, 30]
    assert np.isfinite(vout).all() and (vout >= 0).all()


def test_each_output_alone_is_the_all_outputs_call_on_the_synthetic_frame(rt, gpu):
    """The raw entry with one output pointer at a time over a region off the tile grid: every
    single output equals, bit for bit, the same output of the call that asks for all three."""
    import pass_error_cases as pc
    c, var, n, P, dist, obj = synthetic_frame()
    H, W = obj.shape
    region = (3, 5, 29, 15)
    env = pc.Env(rt)
    base = dict(width=W, height=H, region=region, options={"levels": 3, "sigma_variance": 0.7, "sigma_plane": 0.05},
                radiance=c, variance=var, normal=n, position=P, distance=np.ascontiguousarray(dist), object=obj)
    new = lambda: {"radiance_out": np.full((H, W, 3), -123.25, np.float32),   # noqa: E731
                   "variance_out": np.full((H, W), -123.25, np.float32), "rgb_out": np.full((H, W, 3), 0xA5, np.uint8)}
    full = new()
    assert env.call("rt_denoise_variance", {**base, **full})[0] == 0
    box, _ = _box(region, H, W)
    assert all((a[box] != new()[k][box]).any() for k, a in full.items())
    for k in full:
        one = new()
        assert env.call("rt_denoise_variance", {**base, k: one[k]})[0] == 0, k
        assert bits_equal(one[k], full[k]).all(), k


def test_filter_of_a_synthetic_frame_wider_than_a_row_group(rt, gpu):
    """70x21: the global kernel (step 4) covers 64 pixels of 4 rows per workgroup, so 70 crosses
    its row group and the 16-pixel tiles with a ragged edge, 21 its 4 rows and a tile. The
    variance map is compared with the colour."""
    c, var, n, P, dist, obj = synthetic_frame(21, 70)
    assert_filter_is_restatement(rt, c, var, n, P, dist, obj, "synthetic 70x21", levels=3, sigma_variance=0.7,
                                 sigma_plane=0.05)


# ---- 3. the entries ------------------------------------------------------------------------------
def test_denoise_with_guides_is_camera_denoise_and_the_plain_filter_is_untouched(rt, cornell40):
    cam, rad, var, g = cornell40
    plain = cam.denoise(rad)
    v_want = np.zeros((40, 40), np.float32)
    want = rt.denoise(rad, **g, variance=var, variance_out=v_want)
    rgb = np.zeros((40, 40, 3), np.uint8)
    v_got = np.zeros((40, 40), np.float32)
    out = cam.denoise(rad, rgb=rgb, variance=var, variance_out=v_got)
    assert out is not rad and bits_equal(out, want).all() and bits_equal(v_got, v_want).all()
    assert (out != rad).any() and (out != plain).any() and (rgb == to_u8_ref(want)).all()
    # the existing filter's output is the same before and after a variance-guided call
    assert bits_equal(cam.denoise(rad), plain).all() and bits_equal(rt.denoise(rad, **g), plain).all()
    # outputs aliased onto the inputs
    buf, vbuf = rad.copy(), var.copy()
    assert cam.denoise(buf, out=buf, variance=vbuf, variance_out=vbuf) is buf
    assert bits_equal(buf, want).all() and bits_equal(vbuf, v_want).all()
    # a region, and non-default parameters
    o = dict(levels=2, sigma_variance=1.25, sigma_plane=0.02)
    assert bits_equal(cam.denoise(rad, REGION, variance=var, **o),
                      rt.denoise(rad, **g, region=REGION, variance=var, **o)).all()
    # release_device frees the filter's buffers; the next call re-creates them
    cam.release_device()
    assert bits_equal(cam.denoise(rad, variance=var), want).all()
    t = cam.denoise_times()
    assert t["levels"] == 4 and all(ms > 0 for ms in t["level_ms"]) and t["total_ms"] > 0


def test_progressive_denoised_of_a_region_session(rt, gpu):
    cam = rt.create_camera_from_scene_data(scene(rt, CORNELL), CORNELL_RO)
    box, mask = _box(REGION, 40, 40)
    with cam.progressive(REGION) as pr:
        _, rad, _ = _step(cam, pr, 8)
        var = pr.variance()
        u8 = np.full((40, 40, 3), 0xA5, np.uint8)
        out = np.full((40, 40, 3), -123.25, np.float32)
        vout = np.full((40, 40), -123.25, np.float32)
        assert pr.denoised(u8, out, variance=True, variance_out=vout) is out
        v_want = np.zeros((40, 40), np.float32)
        want = cam.denoise(rad, REGION, variance=var, variance_out=v_want)
        assert bits_equal(out[box], want[box]).all() and (u8[box] == to_u8_ref(want[box])).all()
        assert bits_equal(vout[box], v_want[box]).all()
        assert (out[mask] == np.float32(-123.25)).all() and (u8[mask] == 0xA5).all()
        assert (vout[mask] == np.float32(-123.25)).all()


# ---- 4. end to end -------------------------------------------------------------------------------
def test_end_to_end_cornell_128_equals_the_restatement_of_the_oracle_frame(rt, gpu, oracle):
    """pr.denoised(variance=True) of a Cornell 128x128 session at 4 samples = denoise_var_ref of
    the oracle's spp 4 frame with the variance of the session's blob and the oracle's guides, bit
    for bit; a second call is identical, and the session's next step is that of a session that
    never filtered. On this frame - the product's own sample window 0..3 - the display-domain MSE
    against the GPU's spp 1024 frame, after / before: existing filter 0.2158,
    variance-guided 0.1543 (nothing is random; asserted strictly below the existing filter's
    and <= 0.170, about 10 % above the measurement for a different libm sqrt in the metric)."""
    sd = json.loads((GOLDEN / "scene_cornell.json").read_text())["scene"]
    ro = {"width": 128, "samples": 8, "depth": 8, "aTolerance": 0}
    cam = rt.create_camera_from_scene_data(sd, ro)
    plain = rt.create_camera_from_scene_data(sd, ro)   # a session that never filters
    with cam.progressive() as pr, plain.progressive() as pq:
        _, rad, _ = _step(cam, pr, 4)
        _step(plain, pq, 4)
        blob = pr.save()
        u8 = np.zeros((128, 128, 3), np.uint8)
        vout = np.zeros((128, 128), np.float32)
        out = pr.denoised(u8, variance=True, variance_out=vout)
        ro4 = {**ro, "samples": 4}
        noisy = oracle.render(sd, ro4, threads=8)["radiance"]
        n, P, dist, obj, _ = oracle_guides(oracle, sd, ro4)
        want, want_v = denoise_var_ref(noisy, variance_from_blob(blob), n, P, dist, obj)
        n_bad = int((~bits_equal(out, want)).any(-1).sum())
        n_var = int((~bits_equal(vout, want_v)).sum())
        n_u8 = int((u8 != to_u8_ref(want)).any(-1).sum())
        # a second call: identical, and the state is as it was
        u8b = np.zeros((128, 128, 3), np.uint8)
        again = pr.denoised(u8b, variance=True)
        assert bits_equal(again, out).all() and (u8b == u8).all() and pr.save() == blob
        assert pr.samples_done == 4 and pr.steps == 1
        rgb_p, rad_p, st_p = _step(cam, pr, 4)
        rgb_q, rad_q, st_q = _step(plain, pq, 4)
        same_step = bool((rgb_p == rgb_q).all() and bits_equal(rad_p, rad_q).all()
                         and (st_p.pixels, st_p.samples, st_p.bounces) == (st_q.pixels, st_q.samples, st_q.bounces))
    conv = np.zeros((128, 128, 3), np.float32)
    rgb = np.zeros((128, 128, 3), np.uint8)
    rt.create_camera_from_scene_data(sd, {**ro, "samples": 1024}).render(rgb, radiance=conv)
    before = display_mse(rad, conv)
    r_old = display_mse(denoise_ref(noisy, n, P, dist, obj), conv) / before
    r_new = display_mse(out, conv) / before
    print(f"cornell 128x128 session at 4 samples: pixels differing from the restatement of the oracle frame: radiance "
          f"{n_bad}, variance {n_var}, u8 {n_u8}; MSE {before:.6e}; after / before: existing filter {r_old:.4f}, "
          f"variance-guided {r_new:.4f}")
    assert n_bad == 0 and n_var == 0 and n_u8 == 0
    assert same_step
    assert bits_equal(rad, noisy).all()
    assert r_new < r_old
    assert r_new <= 0.170

