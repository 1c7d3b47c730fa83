"""Reprojection through specular chains, host side: the ABI surface, the through table, the
argument errors that need no device, the restatement's own properties (tests/
specular_reproject_ref.py is the normative definition) and what the chains are worth on oracle
frames."""
import ctypes as C
import inspect
import re
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
from denoise_ref import bits_equal  # noqa: E402
from reproject_ref import MOVE, REASONS as RP_REASONS, reproject_ref, reusable_from_scene  # noqa: E402
from specular_reproject_ref import (PREV_REGION, REASONS, REGION, analytic_scene,  # noqa: E402
                                    cornell_without_spheres, golden_scene, mirror_room, oracle_pair, oracle_quality,
                                    specular_reproject_ref, synthetic_call, synthetic_pair, through_from_scene)

F = np.float32
OPTS = "const rt_specular_reproject_options* options"
DECLARED = {
    "rt_specular_reproject_options_default": ("void", "(rt_specular_reproject_options* options)"),
    "rt_camera_through_objects": ("int", "(const rt_camera* cam, int32_t mask, float max_fuzz, uint8_t* out, int32_t capacity)"),
    "rt_reproject_specular": (
        "int", "(int32_t width, int32_t height, const rt_region* region, const float* normal, const float* position, "
        "const float* distance, const int32_t* object, const float* chain_normal, const float* chain_position, "
        "const float* chain_distance, const int32_t* chain_object, const int32_t* chain, const rt_view* view, "
        "const rt_view* prev_view, const rt_region* prev_region, const float* prev_radiance, const float* prev_normal, "
        "const float* prev_position, const float* prev_distance, const int32_t* prev_object, "
        "const float* prev_chain_normal, const float* prev_chain_position, const float* prev_chain_distance, "
        "const int32_t* prev_chain_object, const int32_t* prev_chain, const uint8_t* reusable, const uint8_t* through, "
        f"int32_t n_objects, {OPTS}, const float* radiance, const int32_t* px_samples, int32_t samples, "
        "float* history_out, float* weight_out, float* radiance_out, uint8_t* rgb_out, uint8_t* kind_out)"),
    "rt_camera_reproject_specular": (
        "int", "(rt_camera* cam, const rt_region* region, rt_camera* prev_cam, const rt_region* prev_region, "
        f"const rt_guide_options* guide_options, {OPTS}, const float* prev_radiance, const float* radiance, "
        "const int32_t* px_samples, int32_t samples, float* history_out, float* weight_out, float* radiance_out, "
        "uint8_t* rgb_out, uint8_t* kind_out)"),
    "rt_camera_progressive_reproject_specular": (
        "int", "(rt_camera* cam, rt_camera* prev_cam, const rt_region* prev_region, const rt_guide_options* guide_options, "
        f"{OPTS}, const float* prev_radiance, uint8_t* rgb, float* radiance, float* weight_out, uint8_t* kind_out)"),
}


def test_symbols_are_declared_exported_and_bound(rt):
    from raytracer_amd import _lib
    lib = _lib.load()
    text = re.sub(r"\s+", " ", _lib.HEADER.read_text())
    assert ("typedef struct { rt_reproject_options base; float point_pixels; int32_t through; } "
            "rt_specular_reproject_options;") in text
    for name, (res, args) in DECLARED.items():
        assert f"{res} {name}{args};" in text, f"{name} is not declared as proposed"
        assert hasattr(lib, name), f"{name} is not exported"
        restype, argtypes = _lib._SIGS[name]
        assert restype is (C.c_int if res == "int" else None) and len(argtypes) == args.count(",") + 1
    assert C.sizeof(_lib.RtSpecularReprojectOptions) == 24 and C.sizeof(_lib.RtReprojectOptions) == 16
    assert lib.rt_version() == 3                       # functions were added, nothing changed
    assert callable(rt.reproject_specular) and hasattr(rt.Camera, "through_objects")
    for fn in (rt.Camera.reproject, rt.ProgressiveRender.reprojected):
        p = inspect.signature(fn).parameters
        assert [p[k].default for k in ("guides", "point_pixels", "through", "kind")] == [None, 4.0, 15, None]
    p = inspect.signature(rt.Camera.through_objects).parameters
    assert (p["mask"].default, p["max_fuzz"].default) == (15, 0.0)
    # the new units are built as their §13 counterparts are: nothing contracted, on the host either
    from raytracer_amd import _build
    units = {u[0]: u[1:] for u in _build._UNITS}
    assert units["reproject_spec.hip"] == units["reproject.hip"]
    assert units["reproject_spec_api.cpp"] == units["api_reproject.cpp"] == (["-ffp-contract=off", "-x", "hip"], True)


def test_options_default(rt):
    from raytracer_amd import _lib
    o = _lib.RtSpecularReprojectOptions()
    _lib.load().rt_specular_reproject_options_default(C.byref(o))
    b = o.base
    assert (b.normal_min, b.sigma_plane, b.min_weight, b.history_samples) == (F(0.9), F(0.01), 0.25, 32.0)
    assert (o.point_pixels, o.through) == (4.0, 15)
    _lib.load().rt_specular_reproject_options_default(None)


# ---- the restatement against reproject_ref -------------------------------------------------------------
def _frames(g, seed=5):
    rng = np.random.default_rng(seed)
    Hp, Wp = g["prev_first"]["object"].shape
    H, W = g["first"]["object"].shape
    prad = (rng.random((Hp, Wp, 3), dtype=F) * F(2)).astype(F)
    fresh = (rng.random((H, W, 3), dtype=F) * F(2)).astype(F)
    return prad, fresh, rng.integers(0, 9, (H, W)).astype(np.int32)


def _both(sd, g, **kw):
    prad, fresh, pxs = _frames(g)
    reus = reusable_from_scene(sd)
    a = reproject_ref(prad, g["prev_view"], g["prev_first"], **g["first"], reusable=reus, radiance=fresh, px_samples=pxs,
                      **kw)
    b = specular_reproject_ref(prad, g["prev_view"], g["prev_first"], g["prev_chain"], g["view"], g["first"], g["chain"],
                               reus, through_from_scene(sd), radiance=fresh, px_samples=pxs, **kw)
    return a, b


def test_without_specular_materials_the_restatement_is_reproject_ref(oracle):
    sd = cornell_without_spheres()
    assert through_from_scene(sd).sum() == 0
    g = oracle_pair(oracle, sd, {"width": 32})
    assert ((g["chain"]["chain"] & 0xff) == 0).all()
    for kw in ({}, {"region": (3, 2, 20, 25), "prev_region": (1, 1, 28, 30), "normal_min": 0.5, "min_weight": 0.6}):
        a, b = _both(sd, g, **kw)
        for k in ("history", "weight", "radiance"):
            assert bits_equal(a[k], b[k]).all(), k
        assert (a["rgb"] == b["rgb"]).all()
        assert set(np.unique(b["kind"])) == {0, 1} and ((b["kind"] == 1) == (a["weight"] > 0)).all()


@pytest.mark.parametrize("name", ["mirror_room", "default"])
def test_pixels_without_a_chain_are_reproject_refs(oracle, name):
    sd = mirror_room() if name == "mirror_room" else golden_scene("default")
    g = oracle_pair(oracle, sd, {"width": 40})
    k0 = (g["chain"]["chain"] & 0xff) == 0
    assert 0.5 < k0.mean() < 1
    a, b = _both(sd, g)
    for k in ("history", "weight", "radiance"):
        assert bits_equal(a[k][k0], b[k][k0]).all(), k
    assert ((b["kind"][k0] == 1) == (a["weight"][k0] > 0)).all() and (b["kind"][k0] < 2).all()
    assert set(np.unique(b["kind"][~k0])) <= {0, 2} and (b["kind"] == 2).any()
    assert (a["weight"][~k0] == 0).all()                  # the first hit's reprojection stops at the specular surface


def test_analytic_planar_mirror(oracle):
    """A planar mirror (z = -1) facing a Lambert wall (z = 6): the chain's virtual point is the wall
    point's mirror image in the plane z = -8, no tap fails the point check at the default 4
    footprints, and at least 0.75 of the mirror's pixels find a history (measured: 0.818, the rest
    sees the wall's image outside the previous frame's mirror)."""
    sd = analytic_scene()
    g = oracle_pair(oracle, sd, {"width": 32})
    assert g["chain"]["chain"].shape == (32, 32)
    k1 = (g["chain"]["chain"] & 0xff) >= 1
    assert 0.25 < k1.mean() < 0.45
    prad, fresh, pxs = _frames(g)
    reasons, points = {}, {}
    r = specular_reproject_ref(prad, g["prev_view"], g["prev_first"], g["prev_chain"], g["view"], g["first"], g["chain"],
                               reusable_from_scene(sd), through_from_scene(sd), radiance=fresh, px_samples=pxs,
                               reasons=reasons, points=points)
    share = float((r["kind"][k1] == 2).mean())
    print(f"analytic 32x32: k >= 1 on {k1.mean():.4f} of the frame, {share:.4f} of those have a history; {reasons}")
    assert reasons["tap_point"] == 0
    assert share >= 0.75
    assert (r["kind"][~k1] == 0).all()                    # the sky and nothing else: no first-hit history
    y, x = 16, 16
    assert k1[y, x] and g["chain"]["object"][y, x] == 1 and g["first"]["object"][y, x] == 0
    wall = g["chain"]["position"][y, x].astype(np.float64)
    image = np.array([wall[0], wall[1], -1.0 - (wall[2] - -1.0)])
    assert wall[2] == 6.0 and np.allclose(points["X"][y, x], image, rtol=1e-5, atol=0)


def test_synthetic_pair_meets_every_rejection_reason():
    assert REASONS[:len(RP_REASONS)] == RP_REASONS
    assert REASONS[len(RP_REASONS):] == ("chain_end", "not_through", "tap_chain", "tap_first_object", "tap_point")
    s = synthetic_pair()
    reasons = {}
    r = synthetic_call(s, region=REGION, prev_region=PREV_REGION, radiance=s["fresh"], px_samples=s["px_samples"],
                       reasons=reasons)
    print(f"synthetic pair: rejections {reasons}")
    assert set(reasons) == set(REASONS) and all(reasons[k] > 0 for k in REASONS), reasons
    x, y, w, h = REGION
    box = r["kind"][y:y + h, x:x + w]
    assert (box == 1).mean() >= 0.25 and (box == 2).mean() >= 0.1
    assert (r["history"] > 1e29).any()                   # the 1e30 tap is finite: it is gathered
    outside = np.ones(r["kind"].shape, bool); outside[y:y + h, x:x + w] = False
    assert (r["kind"][outside] == 0).all() and (r["weight"][outside] == 0).all()
    # the point check alone: a wide one admits the taps it rejected, and only adds history
    wide = {}
    r8 = synthetic_call(s, region=REGION, prev_region=PREV_REGION, point_pixels=64.0, reasons=wide)
    assert wide["tap_point"] < reasons["tap_point"] and (r8["weight"] >= r["weight"]).all()


# ---- the through table ---------------------------------------------------------------------------------
def every_material_scene():
    lam = {"type": "lambert", "color": [0.5, 0.5, 0.5]}
    metal = lambda fuzz: {"type": "metal", "color": [0.8, 0.8, 0.8], "fuzz": fuzz}   # noqa: E731
    mats = [lam, {"type": "light", "emit": [4, 4, 4]}, metal(0), metal(0.2), metal(0.4), metal(7), {"type": "glass", "ior": 1.5},
            {"type": "mixed", "weight": 0.3, "diff": lam, "spec": metal(0)},
            {"type": "layered", "outer": {"type": "glass", "ior": 1.5}, "inner": lam}]
    sd = golden_scene("default")
    objects = [{"type": "sphere", "pos": [i - 4.0, 0.5, -2], "r": 0.4, "material": m} for i, m in enumerate(mats)]
    objects.append({"type": "sphere", "pos": [0, 2, -2], "r": 0.4, "material": "silver"})      # an id beside inline ones
    objects.append({"type": "sphere", "pos": [1, 2, -2], "r": 0.4, "material": "gold"})        # fuzz 0.5
    return {**sd, "objects": objects}


@pytest.mark.parametrize("max_fuzz", [0.0, 0.3])
def test_through_table(rt, max_fuzz):
    from raytracer_amd import _lib
    sd = every_material_scene()
    cam = rt.create_camera_from_scene_data(sd, {"width": 16, "samples": 4})
    #          lam light m0 m.2 m.4 m7 glass mixed layered silver gold
    classes = [0, 0, 1, 1, 1, 1, 2, 4, 8, 1, 1]
    fuzz = [None, None, 0, 0.2, 0.4, 1.0, None, None, None, 0, 0.5]
    for mask in (0, 1, 2, 4, 8, 15):
        want = [int(bool(c & mask) and (c != 1 or f <= max_fuzz)) for c, f in zip(classes, fuzz)]
        got = cam.through_objects(mask, max_fuzz)
        assert got.dtype == np.uint8 and got.tolist() == want == through_from_scene(sd, mask, max_fuzz).tolist(), mask
    assert cam.through_objects().tolist() == cam.through_objects(15, 0.0).tolist()
    assert not (cam.through_objects(15, 1.0) & cam.reusable_objects()).any()
    out = np.zeros(16, np.uint8)
    lib = _lib.load()
    assert lib.rt_camera_through_objects(cam._h, 15, 0.0, out.ctypes.data, 10) == _lib.RT_ERR_INVALID
    assert b"capacity" in lib.rt_last_error()
    for mask, fz in ((-1, 0.0), (16, 0.0), (15, -0.5), (15, float("nan")), (15, float("inf"))):
        assert lib.rt_camera_through_objects(cam._h, mask, fz, out.ctypes.data, 16) == _lib.RT_ERR_INVALID, (mask, fz)
    assert lib.rt_camera_through_objects(cam._h, 15, 0.0, None, 16) == _lib.RT_ERR_INVALID
    assert (out == 0).all()


# ---- errors that need no device ------------------------------------------------------------------------
def _camera(rt, sd=None, **ro):
    return rt.create_camera_from_scene_data(sd or golden_scene("cornell"), {"width": 16, "samples": 4, "depth": 4, **ro})


def _zero_call(rt, cam, **kw):
    H, W = cam.image_height, cam.image_width
    z = np.zeros((H, W, 3), np.float32)
    g = {"normal": z, "position": z, "distance": z[..., 0], "object": np.zeros((H, W), np.int32)}
    gc = {**g, "chain": np.zeros((H, W), np.int32)}
    return rt.reproject_specular(z, cam.view(), g, gc, cam.view(), g, gc, cam.reusable_objects(), cam.through_objects(),
                                 **kw)


BAD_OPTIONS = ([({k: v}, k) for k in ("normal_min", "sigma_plane", "min_weight", "history_samples", "point_pixels")
                for v in (-0.5, float("nan"), float("inf"))])


@pytest.mark.parametrize("opts,word", BAD_OPTIONS)
def test_bad_options_are_invalid_without_a_device(rt, opts, word):
    from raytracer_amd import _lib
    cam = _camera(rt)
    rad = np.zeros((16, 16, 3), np.float32)
    for call in (lambda: _zero_call(rt, cam, **opts), lambda: cam.reproject(cam, rad, guides="specular", **opts)):
        with pytest.raises(rt.RtError, match=word) as e:
            call()
        assert e.value.code == _lib.RT_ERR_INVALID


def test_masks_guide_options_and_the_first_hit_mode_are_refused_without_a_device(rt):
    from raytracer_amd import _lib
    lib = _lib.load()
    cam = _camera(rt)
    rad = np.zeros((16, 16, 3), np.float32)
    p = rad.ctypes.data
    for through in (-1, 16, 255):
        with pytest.raises(rt.RtError, match="through") as e:
            cam.reproject(cam, rad, guides="specular", through=through)
        assert e.value.code == _lib.RT_ERR_INVALID
    for guides, word in (("first_hit", "RT_GUIDES_SPECULAR"), ({"max_bounces": 0}, "max_bounces"),
                         ({"max_bounces": 65}, "max_bounces"), ({"max_fuzz": -1.0}, "max_fuzz"),
                         ({"max_fuzz": float("nan")}, "max_fuzz")):
        with pytest.raises(rt.RtError, match=word) as e:
            cam.reproject(cam, rad, guides=guides)
        assert e.value.code == _lib.RT_ERR_INVALID
    go = _lib.RtGuideOptions(7, 8, 0.0)                  # an unknown mode
    assert lib.rt_camera_reproject_specular(cam._h, None, cam._h, None, C.byref(go), None, p, None, None, 0, None, None,
                                            None, None, None) == _lib.RT_ERR_INVALID and b"mode" in lib.rt_last_error()
    # the keywords of the chains need guides=; without it the call is today's
    for kw in ({"kind": np.zeros((16, 16), np.uint8)}, {"point_pixels": 2.0}, {"through": 1}):
        with pytest.raises(ValueError, match="guides="):
            cam.reproject(cam, rad, **kw)
    with pytest.raises(ValueError):
        cam.reproject(cam, rad, guides="specular", kind=np.zeros((16, 16), np.float32))   # not uint8


def test_regions_samples_pointers_scenes_and_sessions_are_refused_without_a_device(rt):
    from raytracer_amd import _lib
    from raytracer_amd.camera import ProgressiveRender
    lib = _lib.load()
    cam = _camera(rt)
    rad = np.zeros((16, 16, 3), np.float32)
    for region in [(16, 0, 4, 4), (0, 0, 0, 5), (-8, -8, 8, 8)]:
        for call in (lambda: _zero_call(rt, cam, region=region), lambda: _zero_call(rt, cam, prev_region=region),
                     lambda: cam.reproject(cam, rad, region, guides="specular"),
                     lambda: cam.reproject(cam, rad, prev_region=region, guides="specular")):
            with pytest.raises(rt.RtError, match="empty after clamping") as e:
                call()
            assert e.value.code == _lib.RT_ERR_INVALID
    for call in (lambda: _zero_call(rt, cam, radiance=rad, samples=-1),
                 lambda: cam.reproject(cam, rad, radiance=rad, samples=-1, guides="specular")):
        with pytest.raises(rt.RtError, match="samples") as e:
            call()
        assert e.value.code == _lib.RT_ERR_INVALID
    # the raw explicit entry: every required pointer
    view = _lib.RtView()
    lib.rt_camera_get_view(cam._h, C.byref(view))
    p, ip = rad.ctypes.data, np.zeros((16, 16), np.int32)
    g = [p, p, p, ip.ctypes.data]
    gc = [*g, ip.ctypes.data]
    reus, thr = cam.reusable_objects(), cam.through_objects()
    good = [16, 16, None, *g, *gc, C.byref(view), C.byref(view), None, p, *g, *gc, reus.ctypes.data, thr.ctypes.data,
            int(reus.size), None, None, None, 0, None, None, None, None, None]
    assert len(good) == len(_lib._SIGS["rt_reproject_specular"][1])
    for k in [*range(3, 14), *range(15, 27)]:
        args = list(good)
        args[k] = None
        assert lib.rt_reproject_specular(*args) == _lib.RT_ERR_INVALID, k
        assert any(w in lib.rt_last_error() for w in (b"required", b"reusable")), k
    args = list(good)
    args[34] = p                                         # radiance_out without radiance
    assert lib.rt_reproject_specular(*args) == _lib.RT_ERR_INVALID and b"fresh radiance" in lib.rt_last_error()
    assert lib.rt_camera_reproject_specular(cam._h, None, cam._h, None, None, None, None, None, None, 0, None, None, None,
                                            None, None) == _lib.RT_ERR_INVALID
    assert b"prev_radiance is required" in lib.rt_last_error()
    assert lib.rt_camera_reproject_specular(cam._h, None, None, None, None, None, p, None, None, 0, None, None, None, None,
                                            None) == _lib.RT_ERR_INVALID
    # cameras of different scenes
    other = _camera(rt, golden_scene("default"))
    with pytest.raises(rt.RtError, match="reproject: the cameras hold different scenes") as e:
        cam.reproject(other, np.zeros((other.image_height, 16, 3), np.float32), guides="specular")
    assert e.value.code == _lib.RT_ERR_INVALID
    # a session call without a session; a closed handle
    pr = ProgressiveRender(cam)
    with pytest.raises(rt.RtError, match="no progressive session is open") as e:
        pr.reprojected(cam, rad, guides="specular")
    assert e.value.code == _lib.RT_ERR_INVALID
    pr.close()
    with pytest.raises(ValueError):
        pr.reprojected(cam, rad, guides="specular")
    with pytest.raises(rt.RtError, match="no reproject call yet"):
        cam.reproject_times()


# ---- what the chains are worth ---------------------------------------------------------------------------
def test_quality_on_the_oracle_mirror_room(oracle):
    """Cornell with a mirror for a back wall, 64x64, depth 8, aTolerance 0: view A at spp 256, view
    B moved by (0.5, 0.2, -0.2) at spp 4, truth B at spp 1024; default parameters, guides from the
    oracle (tools/specular_reproject_quality.py). Measured: 32.3 % of the pixels have k >= 1, 33.8 %
    of those find a history; display-domain MSE of the blend / of the fresh frame 0.4540 with
    reproject_ref, 0.3855 with the chains (asserted below the former, and <= 0.424: the measurement
    plus 10 %)."""
    q = oracle_quality(oracle, mirror_room(), 64, MOVE)
    print(f"mirror room {q['frame']} move {MOVE}: {q}")
    assert 0.25 < q["k1"] < 0.4 and q["k1_with_history"] >= 0.25
    assert q["chains"] < q["first_hit"]
    assert q["chains"] <= 0.424


def test_quality_on_the_oracle_default_scene(oracle):
    """The default scene 128x72, the same move and sample counts: 15.3 % of the pixels have k >= 1,
    25.4 % of those find a history; blend / fresh 0.8177 with reproject_ref, 0.5756 with the chains
    (asserted below the former, and <= 0.633: the measurement plus 10 %)."""
    q = oracle_quality(oracle, golden_scene("default"), 128, MOVE)
    print(f"default {q['frame']} move {MOVE}: {q}")
    assert 0.1 < q["k1"] < 0.25 and q["k1_with_history"] >= 0.2
    assert q["chains"] < q["first_hit"]
    assert q["chains"] <= 0.633
