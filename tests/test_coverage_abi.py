"""Sub-pixel coverage and the filters' edge hold, host side: the ABI surface, the argument errors
that need no device, the restatement's own properties, and the quality contract - what the hold is
worth on oracle frames against converged oracle frames, through the restatements alone
(tests/coverage_ref.py is the normative definition; tools/coverage_quality.py prints the whole table).

Measured with the restatement (fp32-formed sub-rays; display-domain MSE, filtered / raw, the
variance-guided filter with the hold, K = 2), beside the bounds asserted below:
    rain 128 px spp 8:        0.9013 (without the hold 1.2380), bound < 1.0
    spheres-500 96x96 spp 32: 1.0174 (without the hold 1.2168), bound <= 1.05
    Cornell 128x128 spp 4:    0.1918 (without the hold 0.1481), bound <= 0.22
The figures first measured with fp64-offset sub-rays (0.90, 1.017, 0.192) are these to the digit
given, and so are the mixed shares, so the bounds stand as first stated. The spheres-500 bound holds
with 3.2 % to spare, not 5 %: it was kept, not widened - the oracle is deterministic.
"""
import ctypes as C
import functools
import json
import re
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
from coverage_ref import (F, agree_of, coverage_ref, hold_ref, hold_var_ref, mixed_of, objects_of,  # noqa: E402
                          sub_offsets)
from denoise_ref import display_mse, oracle_guides  # noqa: E402
from denoise_var_ref import denoise_var_ref, oracle_window  # noqa: E402

GOLDEN = Path(__file__).resolve().parent / "golden"

DECLARED = {
    "rt_camera_render_coverage": "(rt_camera* cam, const rt_region* region, int32_t k, uint32_t* coverage)",
    "rt_camera_coverage_time": "(rt_camera* cam, float* coverage_ms)",
    "rt_denoise_hold": "(int32_t width, int32_t height, const rt_region* region, const rt_denoise_options* options, "
                       "const float* radiance, const float* normal, const float* position, const float* distance, "
                       "const int32_t* object, const uint8_t* hold, float* radiance_out, uint8_t* rgb_out)",
    "rt_denoise_variance_hold": "(int32_t width, int32_t height, const rt_region* region, const rt_denoise_var_options* "
                                "options, const float* radiance, const float* variance, const float* normal, const "
                                "float* position, const float* distance, const int32_t* object, const uint8_t* hold, "
                                "float* radiance_out, float* variance_out, uint8_t* rgb_out)",
    "rt_camera_denoise_hold": "(rt_camera* cam, const rt_region* region, const rt_denoise_options* options, int32_t "
                              "hold_k, const float* radiance, float* radiance_out, uint8_t* rgb_out)",
    "rt_camera_denoise_variance_hold": "(rt_camera* cam, const rt_region* region, const rt_denoise_var_options* options, "
                                       "int32_t hold_k, const float* radiance, const float* variance, float* "
                                       "radiance_out, float* variance_out, uint8_t* rgb_out)",
    "rt_camera_progressive_denoise_hold": "(rt_camera* cam, const rt_denoise_options* options, int32_t hold_k, uint8_t* "
                                          "rgb, float* radiance)",
    "rt_camera_progressive_denoise_variance_hold": "(rt_camera* cam, const rt_denoise_var_options* options, int32_t "
                                                   "hold_k, uint8_t* rgb, float* radiance, float* variance_out)",
}


def test_coverage_symbols_are_declared_exported_and_bound(rt):
    from raytracer_amd import _lib
    lib = _lib.load()
    text = re.sub(r"\s+", " ", _lib.HEADER.read_text())
    for name, args in DECLARED.items():
        assert f"int {name}{args};" in text, f"{name} is not declared as proposed"
        assert hasattr(lib, name), f"{name} is not exported"
        res, argtypes = _lib._SIGS[name]
        assert res is C.c_int and len(argtypes) == args.count(",") + 1
    assert lib.rt_version() == 3                       # functions were added, nothing changed
    assert hasattr(rt.Camera, "render_coverage") and hasattr(rt.Camera, "coverage_time")


# ---- argument errors that need no device -------------------------------------------------------
def _camera(rt, **ro):
    sd = rt.generate_scene_data({"type": "cornell"})
    return rt.create_camera_from_scene_data(sd, {"width": 16, "samples": 4, "depth": 4, **ro})


def _frame16():
    rad = np.zeros((16, 16, 3), np.float32)
    g = {"normal": rad, "position": rad, "distance": rad[..., 0], "object": np.zeros((16, 16), np.int32)}
    return rad, np.zeros((16, 16), np.float32), g


def _invalid(rt, call, word):
    from raytracer_amd import _lib
    with pytest.raises(rt.RtError, match=word) as e:
        call()
    assert e.value.code == _lib.RT_ERR_INVALID


@pytest.mark.parametrize("k", [0, 1, 3, 5, 8, -2])
def test_coverage_of_another_k_is_invalid(rt, k):
    _invalid(rt, lambda: _camera(rt).render_coverage(k=k), "k must be 2 or 4")


def test_coverage_without_an_output_or_in_an_empty_region_is_invalid(rt):
    from raytracer_amd import _lib
    cam = _camera(rt)
    _invalid(rt, lambda: _lib.check(cam._lib.rt_camera_render_coverage(cam._h, None, 2, None)), "coverage is required")
    for region in [(16, 0, 4, 4), (0, 0, 0, 5), (-8, -8, 8, 8)]:
        _invalid(rt, lambda: cam.render_coverage(region), "empty after clamping")
    _invalid(rt, cam.coverage_time, "no coverage pass yet")
    _invalid(rt, lambda: _lib.check(cam._lib.rt_camera_coverage_time(cam._h, None)), "null argument")


@pytest.mark.parametrize("k", [1, 3, 8, -2])
def test_a_hold_of_another_k_is_invalid(rt, k):
    cam = _camera(rt)
    rad, var, _ = _frame16()
    _invalid(rt, lambda: cam.denoise(rad, hold_edges=k), "hold_k must be 0, 2 or 4")
    _invalid(rt, lambda: cam.denoise(rad, variance=var, hold_edges=k), "hold_k must be 0, 2 or 4")


def test_the_base_entrys_errors_come_first_in_a_hold_call(rt):
    cam = _camera(rt)
    rad, var, g = _frame16()
    mask = np.zeros((16, 16), np.uint8)
    _invalid(rt, lambda: cam.denoise(rad, hold_edges=3, levels=9), "levels")
    _invalid(rt, lambda: cam.denoise(rad, (16, 0, 4, 4), hold_edges=2), "empty after clamping")
    _invalid(rt, lambda: rt.denoise(rad, **g, hold=mask, levels=9), "rt_denoise_hold: levels")
    _invalid(rt, lambda: rt.denoise(rad, **g, hold=mask, variance=var, sigma_variance=-1.0),
             "rt_denoise_variance_hold: sigma_variance")
    with pytest.raises(ValueError, match="hold must hold 16x16 values"):
        rt.denoise(rad, **g, hold=np.zeros((4, 4), np.uint8))


def test_an_explicit_hold_call_needs_its_mask(rt):
    from raytracer_amd import _lib
    lib = _lib.load()
    rad, var, g = _frame16()
    p = [a.ctypes.data for a in (g["normal"], g["position"], g["distance"], g["object"])]
    _invalid(rt, lambda: _lib.check(lib.rt_denoise_hold(16, 16, None, None, rad.ctypes.data, *p, None, rad.ctypes.data,
                                                        None)), "rt_denoise_hold: hold is required")
    _invalid(rt, lambda: _lib.check(lib.rt_denoise_variance_hold(16, 16, None, None, rad.ctypes.data, var.ctypes.data, *p,
                                                                 None, rad.ctypes.data, None, None)),
             "rt_denoise_variance_hold: hold is required")


def test_session_hold_calls_without_a_session_are_invalid(rt):
    from raytracer_amd.camera import ProgressiveRender
    pr = ProgressiveRender(_camera(rt))  # a handle with no session behind it
    for call in (lambda: pr.denoised(hold_edges=2), lambda: pr.denoised(variance=True, hold_edges=4)):
        _invalid(rt, call, "no progressive session is open")


# ---- the restatement's own properties ----------------------------------------------------------
def test_sub_offsets_are_the_cell_centres():
    assert [(b, float(x), float(y)) for b, x, y in sub_offsets(2)] == [(0, -0.25, -0.25), (1, 0.25, -0.25),
                                                                         (2, -0.25, 0.25), (3, 0.25, 0.25)]
    o4 = sub_offsets(4)
    assert [b for b, _, _ in o4] == list(range(16))
    assert sorted({float(x) for _, x, _ in o4}) == [-0.375, -0.125, 0.125, 0.375]
    assert all(float(x) == (b % 4 + 0.5) / 4 - 0.5 and float(y) == (b // 4 + 0.5) / 4 - 0.5 for b, x, y in o4)


def test_hold_is_a_select_of_the_inputs():
    rng = np.random.default_rng(5)
    noisy = rng.random((6, 7, 3), dtype=F)
    noisy[2, 3, 1] = np.nan                              # a held pixel keeps even this
    filtered = rng.random((6, 7, 3), dtype=F)
    var = rng.random((6, 7), dtype=F)
    var[2, 3], var[0, 0], var[5, 6] = np.nan, -1.0, np.inf
    fvar = rng.random((6, 7), dtype=F)
    mask = np.zeros((6, 7), bool)
    mask[2, 3] = mask[0, 0] = mask[5, 6] = mask[4, 1] = True
    out, vout = hold_ref(filtered, noisy, mask), hold_var_ref(fvar, var, mask)
    assert out.dtype == F and vout.dtype == F
    assert (out[~mask] == filtered[~mask]).all() and (vout[~mask] == fvar[~mask]).all()
    assert np.array_equal(out[mask], noisy[mask], equal_nan=True)
    assert vout[2, 3] == 0 and vout[0, 0] == 0 and vout[5, 6] == 0 and vout[4, 1] == var[4, 1]


@pytest.mark.parametrize("k", [2, 4])
def test_coverage_words_of_a_small_cornell(oracle, k):
    """The word's two fields agree with each other, a region writes only itself, and the K = 2 rays
    are not a subset of the K = 4 ones - but a pixel whose 16 rays agree is whole."""
    sd = json.loads((GOLDEN / "scene_cornell.json").read_text())["scene"]
    ro = {"width": 24, "samples": 4}
    w = coverage_ref(oracle, sd, ro, k)
    mixed, objects = mixed_of(w, k), objects_of(w)
    assert w.dtype == np.uint32 and w.shape == (24, 24) and (w >> np.uint32(24) == 0).all()
    assert (agree_of(w) >> np.uint16(k * k) == 0).all() if k == 2 else True
    assert (objects >= 1).all() and (objects <= k * k + 1).all()
    assert ((objects >= 2) == mixed).all()               # every ray shows the centre's object <=> one object
    assert 0 < mixed.sum() < mixed.size // 2
    region = (5, 3, 11, 9)
    wr = coverage_ref(oracle, sd, ro, k, region)
    box = (slice(3, 12), slice(5, 16))
    assert (wr[box] == w[box]).all() and wr.sum() == wr[box].sum()
    assert not mixed_of(wr, k, region)[0, 0] and mixed_of(wr, k)[0, 0]   # a zero word outside the region is no pixel


# ---- the quality contract ----------------------------------------------------------------------
# scene -> (render options, converged spp, the mixed share of K = 2 and K = 4 as first measured with
# fp64-offset sub-rays)
SCENES = {"rain_seed42": ({"width": 128}, 512, (0.025, 0.035)),
          "spheres500_seed42": ({"width": 96, "aspect": 1}, 512, (0.174, 0.242)),
          "cornell": ({"width": 128}, 1024, (0.042, 0.060)),
          "default": ({"width": 128}, 512, (0.029, 0.042))}
# (scene, spp) -> the bound on the variance-guided filter's ratio with the hold, K = 2
QUALITY = {("rain_seed42", 8): ("<", 1.0), ("spheres500_seed42", 32): ("<=", 1.05), ("cornell", 4): ("<=", 0.22)}


@functools.lru_cache(maxsize=None)
def _scene(name):
    return json.loads((GOLDEN / f"scene_{name}.json").read_text())["scene"]


def _ro(name):
    return {**SCENES[name][0], "depth": 8, "aTolerance": 0}


@pytest.fixture(scope="module")
def masks(oracle):
    """scene -> {k: the mixed mask} of the four golden scenes at the table's sizes (read-only)."""
    out = {}
    for name in SCENES:
        out[name] = {k: mixed_of(coverage_ref(oracle, _scene(name), {**_ro(name), "samples": 4}, k), k) for k in (2, 4)}
        for m in out[name].values():
            m.setflags(write=False)
    return out


@pytest.mark.parametrize("name", list(SCENES))
def test_the_mixed_share_is_the_measured_one(masks, name):
    """Within +-20 % (relative) of the share first measured: a broken ray formation - a wrong
    offset, a swapped axis, rays through the pixel corner - moves it by far more."""
    for k, want in zip((2, 4), SCENES[name][2]):
        got = float(masks[name][k].mean())
        print(f"{name} K={k}: mixed share {got:.4f} (first measured {want:.3f})")
        assert 0.8 * want <= got <= 1.2 * want, (name, k, got)
    assert (masks[name][4] | ~masks[name][2]).mean() > 0.99   # K = 4 sees nearly all K = 2 sees


@pytest.fixture(scope="module")
def converged(oracle):
    """(scene) -> the converged oracle frame and the oracle's guides, rendered once per module."""
    @functools.lru_cache(maxsize=None)
    def get(name):
        conv = oracle.render(_scene(name), {**_ro(name), "samples": SCENES[name][1]}, threads=16)["radiance"]
        return conv, oracle_guides(oracle, _scene(name), {**_ro(name), "samples": 4})
    return get


@pytest.mark.parametrize("name,spp", list(QUALITY))
def test_the_hold_keeps_the_variance_guided_filter_safe(oracle, masks, converged, name, spp):
    conv, (n, P, dist, obj, _) = converged(name)
    noisy, var = oracle_window(oracle, _scene(name), _ro(name), spp)
    before = display_mse(noisy, conv)
    guided = denoise_var_ref(noisy, var, n, P, dist, obj)[0]
    today = display_mse(guided, conv) / before
    held = display_mse(hold_ref(guided, noisy, masks[name][2]), conv) / before
    op, bound = QUALITY[(name, spp)]
    print(f"{name} spp {spp}: variance-guided / raw {today:.4f}, with the K=2 hold {held:.4f} (bound {op} {bound})")
    assert held < bound if op == "<" else held <= bound, (name, spp, held)
    if name != "cornell":
        assert held < today            # the scenes the filter used to damage: the hold repairs them
    else:
        assert held > today            # the price indoors: the still-noisy edge pixels
