"""Reprojection of a previous view's frame, host side: the ABI surface, the host-only entries
(view, reusable table), the argument errors that need no device, the restatement's own properties
and what the history is worth on oracle frames (tests/reproject_ref.py is the normative
definition)."""
import ctypes as C
import json
import re
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
from reproject_ref import (F, MOVE, oracle_quality, reproject_ref, reusable_from_scene,  # noqa: E402
                           view_constants)

GOLDEN = Path(__file__).resolve().parent / "golden"

DECLARED = {
    "rt_camera_get_view": "(const rt_camera* cam, rt_view* view)",
    "rt_camera_reusable_objects": "(const rt_camera* cam, uint8_t* out, int32_t capacity)",
    "rt_reproject": "(int32_t width, int32_t height, const rt_region* region, const float* normal, const float* "
                    "position, const float* distance, const int32_t* object, const rt_view* prev_view, const rt_region* "
                    "prev_region, const float* prev_radiance, const float* prev_normal, const float* prev_position, "
                    "const float* prev_distance, const int32_t* prev_object, const uint8_t* reusable, int32_t "
                    "n_objects, const rt_reproject_options* options, const float* radiance, const int32_t* "
                    "px_samples, int32_t samples, float* history_out, float* weight_out, float* radiance_out, "
                    "uint8_t* rgb_out)",
    "rt_camera_reproject": "(rt_camera* cam, const rt_region* region, rt_camera* prev_cam, const rt_region* "
                           "prev_region, const rt_reproject_options* options, const float* prev_radiance, const float* "
                           "radiance, const int32_t* px_samples, int32_t samples, float* history_out, float* "
                           "weight_out, float* radiance_out, uint8_t* rgb_out)",
    "rt_camera_progressive_reproject": "(rt_camera* cam, rt_camera* prev_cam, const rt_region* prev_region, const "
                                       "rt_reproject_options* options, const float* prev_radiance, uint8_t* rgb, "
                                       "float* radiance, float* weight_out)",
    "rt_camera_reproject_times": "(rt_camera* cam, float* guide_ms, float* reproject_ms, float* total_ms)",
}


def scene_of(name):
    return json.loads((GOLDEN / f"scene_{name}.json").read_text())["scene"]


def test_reproject_symbols_are_declared_exported_and_bound(rt):
    from raytracer_amd import _lib
    lib = _lib.load()
    text = re.sub(r"\s+", " ", _lib.HEADER.read_text())
    assert "typedef struct { float center[3], pixel00[3], du[3], dv[3]; int32_t width, height; } rt_view;" in text
    assert ("typedef struct { float normal_min, sigma_plane, min_weight, history_samples; } rt_reproject_options;"
            in text)
    for name, args in DECLARED.items():
        assert f"int {name}{args};" in text, f"{name} is not declared as proposed"
        assert hasattr(lib, name), f"{name} is not exported"
        res, argtypes = _lib._SIGS[name]
        assert res is C.c_int and len(argtypes) == args.count(",") + 1
    assert C.sizeof(_lib.RtView) == 56 and C.sizeof(_lib.RtReprojectOptions) == 16
    assert lib.rt_version() == 3
    assert callable(rt.reproject) and all(hasattr(rt.Camera, m) for m in ("view", "reusable_objects", "reproject",
                                                                           "reproject_times"))
    assert hasattr(rt.ProgressiveRender, "reprojected")


# ---- the host-only entries ------------------------------------------------------------------------
CUSTOM_CAMERA = {"from": [1.25, 0.5, 3.0], "at": [0.1, -0.2, 0.3], "up": [0.1, 1.0, 0.05], "vfov": 55}


@pytest.mark.parametrize("name,camera", [("cornell", {}), ("default", {}), ("cornell", CUSTOM_CAMERA)])
def test_view_is_the_oracles_camera_rounded_to_fp32(rt, oracle, name, camera):
    sd = scene_of(name)
    sd = {**sd, "camera": {**sd["camera"], **camera}}
    if name == "default":
        assert sd["camera"]["aperture"] == 0.05      # a defocus camera still reports its pinhole frame
    ro = {"width": 40, "samples": 4}
    view = rt.create_camera_from_scene_data(sd, ro).view()
    ci = oracle.camera_info(sd, ro)
    assert (view["width"], view["height"]) == (ci["width"], ci["height"]) and view["width"] == 40
    for k in ("center", "pixel00", "du", "dv"):
        want = np.asarray(ci[k], dtype=np.float32)
        assert view[k].dtype == np.float32 and view[k].tobytes() == want.tobytes(), k


def test_reusable_table(rt):
    from raytracer_amd import _lib
    cam = rt.create_camera_from_scene_data(scene_of("cornell"), {"width": 16, "samples": 4})
    assert cam.reusable_objects().tolist() == [1, 1, 1, 1, 1, 1, 1, 0]
    sd = scene_of("default")
    by_id = {m["id"]: m["material"]["type"] for m in sd["materials"]}
    want = [1 if by_id[o["material"]] in ("lambert", "light") else 0 for o in sd["objects"]]
    cam = rt.create_camera_from_scene_data(sd, {"width": 16, "samples": 4})
    got = cam.reusable_objects()
    assert got.dtype == np.uint8 and got.tolist() == want == reusable_from_scene(sd).tolist()
    assert 0 < sum(want) < len(want) and {by_id[o["material"]] for o in sd["objects"]} >= {"metal", "glass", "layered"}
    # inline materials beside ids
    lam = {"type": "lambert", "color": [0.5, 0.5, 0.5]}
    sd2 = {**sd, "objects": [{**sd["objects"][0], "material": lam},
                             {**sd["objects"][1], "material": {"type": "mixed", "weight": 0.5, "diff": lam,
                                                               "spec": {"type": "metal", "color": [0.5, 0.5, 0.5]}}},
                             {**sd["objects"][2], "material": "blue"}, {**sd["objects"][3], "material": "gold"}]}
    cam2 = rt.create_camera_from_scene_data(sd2, {"width": 16, "samples": 4})
    assert cam2.reusable_objects().tolist() == [1, 0, 1, 0] == reusable_from_scene(sd2).tolist()
    out = np.zeros(4, np.uint8)
    assert _lib.load().rt_camera_reusable_objects(cam._h, out.ctypes.data, 4) == _lib.RT_ERR_INVALID


# ---- the restatement's own properties -------------------------------------------------------------
S = 2.0 ** -5


def quad_view(W, H, shift=0.0):
    """A camera at the origin looking down -z whose pixels are 2^-5 apart on the plane z = -1,
    pixel (0, 0) moved by `shift` pixels along both axes: every value is exact in fp32."""
    return {"center": [0, 0, 0], "pixel00": [(-(W - 1) / 2 + shift) * S, ((H - 1) / 2 - shift) * S, -1.0],
            "du": [S, 0, 0], "dv": [0, -S, 0], "width": W, "height": H}


def quad_guides(view):
    """First hits of the view's pinhole rays on the fronto-parallel plane z = -4, object 0."""
    W, H = view["width"], view["height"]
    p, du, dv = (np.asarray(view[k], F) for k in ("pixel00", "du", "dv"))
    i = np.arange(W, dtype=F)[None, :, None]; j = np.arange(H, dtype=F)[:, None, None]
    P = (F(4) * (p + du * i + dv * j)).astype(F)
    n = np.zeros((H, W, 3), F); n[..., 2] = 1
    D = np.sqrt((P * P).sum(-1)).astype(F)
    return {"normal": n, "position": P, "distance": D, "object": np.zeros((H, W), np.int32)}


def test_restatement_same_view_returns_the_constant_with_weight_one():
    W, H = 32, 24
    view = quad_view(W, H)
    g = quad_guides(view)
    vc = view_constants(view)
    assert vc["w"].tolist() == [0, 0, -S * S] and vc["aw"] == F(S * S) and vc["iu"] == F(1 / (S * S)) == vc["iv"]
    colour = np.array([0.375, 1.7, 0.01], F)
    prev = np.broadcast_to(colour, (H, W, 3)).copy()
    r = reproject_ref(prev, view, g, **g, reusable=[1])
    inner = (slice(1, H - 1), slice(1, W - 1))
    assert r["radiance"] is None and r["rgb"] is None
    assert np.allclose(r["weight"][inner], 1, rtol=1e-6, atol=0) and (r["weight"] > 0).all()
    assert np.allclose(r["history"][inner], colour, rtol=1e-6, atol=0)
    # the blend: Nh = 32 history samples against m fresh ones
    fresh = np.full((H, W, 3), 2.0, F)
    pxs = np.full((H, W), 4, np.int32); pxs[3, 4] = 0
    fresh[5, 6] = np.nan
    r = reproject_ref(prev, view, g, **g, reusable=[1], radiance=fresh, px_samples=pxs)
    want = ((colour * F(32) + F(2) * F(4)) / F(36)).astype(F)
    assert np.allclose(r["radiance"][10, 10], want, rtol=1e-6, atol=0)
    assert np.allclose(r["radiance"][3, 4], colour, rtol=1e-6) and np.allclose(r["radiance"][5, 6], colour, rtol=1e-6)
    r0 = reproject_ref(prev, view, g, **g, reusable=[0], radiance=fresh, px_samples=pxs)
    assert (r0["weight"] == 0).all() and (r0["history"] == 0).all()
    assert (r0["radiance"][10, 10] == 2).all() and np.isnan(r0["radiance"][5, 6]).all()   # no history: the fresh frame


def test_restatement_rejections_remove_exactly_the_affected_taps():
    """The previous view is the new one moved by half a pixel, so every new pixel (i, j) gathers
    the previous pixels (i - 1 .. i, j - 1 .. j) with b = 1/4 each, exactly."""
    W, H = 32, 24
    new, prev_view = quad_view(W, H), quad_view(W, H, shift=0.5)
    g, pg = quad_guides(new), quad_guides(prev_view)
    colour = np.array([0.375, 1.7, 0.01], F)
    prev = np.broadcast_to(colour, (H, W, 3)).copy()
    pg["object"][10, 10] = 1                       # an object-id mismatch
    pg["normal"][10, 20] = (0, 0, -1)              # a flipped normal
    prev[15, 10, 1] = np.inf                       # a non-finite tap
    pg["position"][15, 20, 2] += 1                 # a tap off the pixel's plane
    g["position"][18, 5] = -g["position"][18, 5]   # a point behind the previous camera
    reasons = {}
    r = reproject_ref(prev, prev_view, pg, **g, reusable=[1, 1], reasons=reasons)
    bad = np.zeros((H, W), int)
    for (y, x) in ((10, 10), (10, 20), (15, 10), (15, 20)):
        bad[y:y + 2, x:x + 2] += 1                 # the four new pixels that gather previous pixel (x, y)
    want = (1 - 0.25 * bad).astype(F)
    want[0, :] = 0.5; want[:, 0] = 0.5; want[0, 0] = 0.25   # first row / column: taps outside the previous image
    want[18, 5] = 0
    assert (r["weight"] == want).all()
    has = r["weight"] > 0
    assert np.allclose(r["history"][has], colour, rtol=1e-6, atol=0) and (r["history"][~has] == 0).all()
    assert reasons["behind"] == 1 and reasons["tap_object"] == 4 and reasons["tap_normal"] == 4
    assert reasons["tap_nonfinite"] == 4 and reasons["tap_plane"] == 4 and reasons["tap_outside"] == 2 * (W + H) - 1
    # min_weight: a pixel that keeps less than it has no history
    r = reproject_ref(prev, prev_view, pg, **g, reusable=[1, 1], min_weight=0.8)
    assert (r["weight"][bad > 0] == 0).all()
    assert r["weight"][5, 5] == 1 and r["weight"][0, 5] == 0
    # prev_region: taps outside it do not count
    r = reproject_ref(prev, prev_view, pg, **g, reusable=[1, 1], prev_region=(8, 0, W - 8, H))
    assert (r["weight"][2:9, :8] == 0).all() and (r["weight"][2:9, 8] == 0.5).all() and r["weight"][5, 9] == 1


# ---- errors that need no device -------------------------------------------------------------------
def _camera(rt, name="cornell", **ro):
    return rt.create_camera_from_scene_data(scene_of(name), {"width": 16, "samples": 4, "depth": 4, **ro})


def _frames16(cam):
    H, W = cam.image_height, cam.image_width
    rad = np.zeros((H, W, 3), np.float32)
    g = {"normal": rad, "position": rad, "distance": rad[..., 0], "object": np.zeros((H, W), np.int32)}
    return rad, g


BAD_OPTIONS = [({k: v}, k) for k in ("normal_min", "sigma_plane", "min_weight", "history_samples")
               for v in (-0.5, float("nan"), float("inf"))]


@pytest.mark.parametrize("opts,word", BAD_OPTIONS)
def test_bad_options_are_invalid_without_a_device(rt, opts, word):
    from raytracer_amd import _lib
    cam = _camera(rt)
    rad, g = _frames16(cam)
    for call in (lambda: rt.reproject(rad, cam.view(), g, **g, reusable=cam.reusable_objects(), **opts),
                 lambda: cam.reproject(cam, rad, **opts)):
        with pytest.raises(rt.RtError, match=word) as e:
            call()
        assert e.value.code == _lib.RT_ERR_INVALID


def test_empty_regions_negative_samples_and_missing_pointers_are_invalid_without_a_device(rt):
    from raytracer_amd import _lib
    lib = _lib.load()
    cam = _camera(rt)
    rad, g = _frames16(cam)
    reus = cam.reusable_objects()
    for region in [(16, 0, 4, 4), (0, 0, 0, 5), (-8, -8, 8, 8)]:
        for call in (lambda: rt.reproject(rad, cam.view(), g, **g, reusable=reus, region=region),
                     lambda: rt.reproject(rad, cam.view(), g, **g, reusable=reus, prev_region=region),
                     lambda: cam.reproject(cam, rad, region),
                     lambda: cam.reproject(cam, rad, prev_region=region)):
            with pytest.raises(rt.RtError, match="empty after clamping") as e:
                call()
            assert e.value.code == _lib.RT_ERR_INVALID
    for call in (lambda: rt.reproject(rad, cam.view(), g, **g, reusable=reus, radiance=rad, samples=-1),
                 lambda: cam.reproject(cam, rad, radiance=rad, samples=-1)):
        with pytest.raises(rt.RtError, match="samples") as e:
            call()
        assert e.value.code == _lib.RT_ERR_INVALID
    # the raw entries: a missing required pointer, and blend outputs without a fresh frame
    view = _lib.RtView()
    lib.rt_camera_get_view(cam._h, C.byref(view))
    p = rad.ctypes.data
    gp = [g["normal"].ctypes.data, g["position"].ctypes.data, g["distance"].ctypes.data, g["object"].ctypes.data]
    good = [16, 16, None, *gp, C.byref(view), None, p, *gp, reus.ctypes.data, int(reus.size), None, None, None, 0,
            None, None, None, None]
    for k in (3, 4, 5, 6, 7, 9, 10, 11, 12, 13, 14):
        args = list(good)
        args[k] = None
        assert lib.rt_reproject(*args) == _lib.RT_ERR_INVALID, k
        assert b"required" in lib.rt_last_error() or b"reusable" in lib.rt_last_error()
    out = np.zeros((16, 16, 3), np.float32)
    args = list(good)
    args[22] = out.ctypes.data                       # radiance_out without radiance
    assert lib.rt_reproject(*args) == _lib.RT_ERR_INVALID and b"fresh radiance" in lib.rt_last_error()
    assert lib.rt_camera_reproject(cam._h, None, cam._h, None, None, None, None, None, 0, None, None, None,
                                   None) == _lib.RT_ERR_INVALID and b"prev_radiance is required" in lib.rt_last_error()
    assert lib.rt_camera_reproject(cam._h, None, cam._h, None, None, p, None, None, 0, None, None, out.ctypes.data,
                                   None) == _lib.RT_ERR_INVALID and b"fresh radiance" in lib.rt_last_error()
    assert lib.rt_camera_reproject(cam._h, None, None, None, None, p, None, None, 0, None, None, None,
                                   None) == _lib.RT_ERR_INVALID
    assert lib.rt_camera_get_view(cam._h, None) == _lib.RT_ERR_INVALID
    assert lib.rt_camera_reproject_times(cam._h, None, None, None) == _lib.RT_ERR_INVALID
    assert (out == 0).all()
    with pytest.raises(ValueError):
        cam.reproject(cam, rad, out=out)             # out without radiance


def test_cameras_of_different_scenes_are_refused_on_the_host(rt):
    from raytracer_amd import _lib
    from raytracer_amd.camera import ProgressiveRender
    cam, other = _camera(rt), _camera(rt, "default")
    rad, _ = _frames16(other)
    with pytest.raises(rt.RtError, match="reproject: the cameras hold different scenes") as e:
        cam.reproject(other, rad)
    assert e.value.code == _lib.RT_ERR_INVALID
    # one object's material changed: the same shapes, another scene
    sd = scene_of("cornell")
    sd2 = {**sd, "objects": [*sd["objects"][:-1], {**sd["objects"][-1], "material": "sphere-white"}]}
    changed = rt.create_camera_from_scene_data(sd2, {"width": 16, "samples": 4, "depth": 4})
    with pytest.raises(rt.RtError, match="different scenes"):
        cam.reproject(changed, np.zeros((16, 16, 3), np.float32))
    # a session call without a session; a closed handle
    pr = ProgressiveRender(cam)
    with pytest.raises(rt.RtError, match="no progressive session is open") as e:
        pr.reprojected(cam, np.zeros((16, 16, 3), np.float32))
    assert e.value.code == _lib.RT_ERR_INVALID
    pr.close()
    with pytest.raises(ValueError):
        pr.reprojected(cam, np.zeros((16, 16, 3), np.float32))
    with pytest.raises(rt.RtError, match="no reproject call yet"):
        cam.reproject_times()


# ---- what the history is worth ----------------------------------------------------------------------
def test_reprojected_history_quality_on_oracle_cornell(oracle):
    """Cornell 64x64, depth 8, aTolerance 0: view A = the scene's camera at spp 256, view B =
    `from` moved by (0.5, 0.2, -0.2), fresh at spp 4, truth B at spp 1024; default parameters,
    guides from the oracle. Measured (nothing is random): 82.8 % of the pixels have a history,
    display-domain MSE of the blend / of the fresh frame 0.2164 (asserted <= 0.238, about 10 %
    above the measurement for a different libm sqrt in the metric)."""
    q = oracle_quality(oracle, scene_of("cornell"), 64, MOVE)
    print(f"cornell {q['frame']} move {MOVE}: share {q['share']:.4f}, fresh MSE {q['mse_fresh']:.6e}, "
          f"blend / fresh {q['ratio']:.4f}")
    assert q["share"] >= 0.6
    assert q["ratio"] <= 0.238


def test_reprojected_history_quality_on_oracle_default_scene(oracle):
    """The default scene (sky, glass, metal, layered paint) 128x72, the same move and sample
    counts: 26.8 % of the pixels have a history (the ground plane and the blue sphere), blend /
    fresh 0.8177 (asserted <= 0.899: the measurement plus 10 %, below 1 - it never gets worse)."""
    q = oracle_quality(oracle, scene_of("default"), 128, MOVE)
    print(f"default {q['frame']} move {MOVE}: share {q['share']:.4f}, fresh MSE {q['mse_fresh']:.6e}, "
          f"blend / fresh {q['ratio']:.4f}")
    assert 0.1 < q["share"] < 0.6
    assert q["ratio"] <= 0.899 < 1
