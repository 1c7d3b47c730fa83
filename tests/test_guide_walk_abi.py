"""Guides through the specular chain, host side: the ABI surface, the restatement
(tests/guide_walk_ref.py, the normative definition) pinned to the oracle's materials and to
oracle_guides, an analytic two-segment case, and the argument errors decided without a device.
Every comparison is exact (== on bits)."""
import ctypes as C
import inspect
import re
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
from denoise_ref import oracle_guides  # noqa: E402
from guide_walk_ref import END_SURFACE, F, continue_dir, guide_walk_ref, unit  # noqa: E402

DECLARED = {
    "rt_guide_options_default": ("void", "(rt_guide_options* options)"),
    "rt_camera_render_guides_ex": ("int", "(rt_camera* cam, const rt_region* region, const rt_guide_options* options, "
                                          "float* normal, float* position, float* distance, int32_t* object, "
                                          "int32_t* chain)"),
    "rt_camera_set_denoise_guides": ("int", "(rt_camera* cam, const rt_guide_options* options)"),
    "rt_camera_get_denoise_guides": ("int", "(rt_camera* cam, rt_guide_options* options)"),
}
CORNELL_EMPTY = {"type": "cornell", "options": {"variant": "empty"}}
CAMERA = {"vfov": 40, "aperture": 0, "focus": 1, "from": [0, 0, 0], "at": [0, 0, -1], "up": [0, 1, 0],
          "background": {"type": "gradient", "top": [1, 1, 1], "bottom": [0.5, 0.7, 1]}}


def test_symbols_are_declared_exported_and_bound(rt):
    from raytracer_amd import _lib
    lib = _lib.load()
    text = re.sub(r"\s+", " ", _lib.HEADER.read_text())
    assert "typedef struct { int32_t mode; int32_t max_bounces; float max_fuzz; } rt_guide_options;" in text
    assert "enum { RT_GUIDES_FIRST_HIT = 0, RT_GUIDES_SPECULAR = 1 };" in text
    for name, (res, args) in DECLARED.items():
        assert f"{res} {name}{args};" in text, f"{name} is not declared as proposed"
        assert hasattr(lib, name), f"{name} is not exported"
        restype, argtypes = _lib._SIGS[name]
        assert restype is (C.c_int if res == "int" else None) and len(argtypes) == args.count(",") + 1
    assert C.sizeof(_lib.RtGuideOptions) == 12
    assert lib.rt_version() == 3                       # functions were added, nothing changed
    assert C.sizeof(_lib.RtDenoiseOptions) == 12 and C.sizeof(_lib.RtDenoiseVarOptions) == 12
    for limit in ("Schlick", "fuzzy metals above max_fuzz", "defocused", "still stop at specular surfaces"):
        assert limit in text, limit
    sig = inspect.signature(rt.Camera.render_guides)
    assert [sig.parameters[k].default for k in ("through_specular", "max_bounces", "max_fuzz")] == [False, 8, 0.0]
    assert inspect.signature(rt.Camera.denoise).parameters["guides"].default == "first_hit"
    assert inspect.signature(rt.ProgressiveRender.denoised).parameters["guides"].default == "first_hit"
    assert inspect.signature(rt.denoise).parameters["chain"].default is None


def test_options_default(rt):
    from raytracer_amd import _lib
    lib = _lib.load()
    o = _lib.RtGuideOptions(9, 9, 9.0)
    lib.rt_guide_options_default(C.byref(o))
    assert (o.mode, o.max_bounces, o.max_fuzz) == (_lib.GUIDES_FIRST_HIT, 8, 0.0)
    assert (_lib.GUIDES_FIRST_HIT, _lib.GUIDES_SPECULAR) == (0, 1)
    lib.rt_guide_options_default(None)                  # harmless


# ---- the restatement's directions against the oracle's materials -------------------------------------
def _incidences():
    """(din, normal) pairs: several normals, incidence from normal to grazing, unnormalised."""
    rng = np.random.default_rng(11)
    out = []
    for n in ([0, 1, 0], [0, 0, -1], [0.6, 0.0, 0.8], [-0.48, 0.64, 0.6]):
        n = unit(np.asarray([n], F))[0]
        t = unit(np.cross(n, [0.3, -0.7, 0.2]).astype(F)[None])[0]
        for deg in (0.0, 12.0, 40.0, 41.5, 42.5, 60.0, 75.0, 89.0):
            a = np.deg2rad(deg)
            d = (-np.cos(a) * n + np.sin(a) * t) * rng.uniform(0.5, 3.0)
            out.append((d.astype(F), n))
    return out


def _probe_dirs(oracle, mat, din, n, front, trials):
    pr = oracle.material_probe(mat, din.tolist(), n.tolist(), front=front, seed=5, n=trials)
    return pr[:, 0] > 0, pr[:, 2] > 0, pr[:, 6:9].astype(F)


def _ref_dir(mat, din, n, front, max_fuzz=0.0):
    cont, d = continue_dir({}, mat, din[None], n[None], np.array([front]), max_fuzz)
    return bool(cont[0]), d[0]


def test_metal_direction_equals_every_probe_direction(oracle):
    mat = {"type": "metal", "color": [0.8, 0.8, 0.8], "fuzz": 0}
    seen = 0
    for din, n in _incidences():
        for front in (True, False):
            valid, _, dirs = _probe_dirs(oracle, mat, din, n, front, 4)
            cont, d = _ref_dir(mat, din, n, front)
            assert cont == bool(valid.all()) == bool(valid.any())
            if cont:
                assert (dirs == d).all(), (din, n, front)
                seen += 1
    assert seen >= 32
    # a mirror direction that points into the surface (a ray leaving it: no pixel's hit, the guide
    # normal faces the ray): the probe does not scatter, the walk is terminal
    for din, n in _incidences()[:8]:
        valid, _, _ = _probe_dirs(oracle, mat, -din, n, True, 2)
        assert not valid.any() and _ref_dir(mat, -din, n, True)[0] is False
    # above max_fuzz a metal is terminal; at or below it continues along the mirror direction
    fuzzy = {"type": "metal", "color": [1, 1, 1], "fuzz": 0.2}
    din, n = _incidences()[2]
    assert _ref_dir(fuzzy, din, n, True, 0.0)[0] is False
    cont, d = _ref_dir(fuzzy, din, n, True, 0.25)
    assert cont and (d == _ref_dir(mat, din, n, True)[1]).all()
    assert _ref_dir({"type": "metal", "color": [1, 1, 1], "fuzz": 7}, din, n, True, 0.99)[0] is False   # clamped to 1
    assert _ref_dir({"type": "lambert", "color": [1, 1, 1]}, din, n, True)[0] is False
    assert _ref_dir({"type": "light", "emit": [1, 1, 1]}, din, n, True)[0] is False


GLASSY = {
    "glass": {"type": "glass", "ior": 1.5},
    "glass_dense": {"type": "glass", "ior": 2.4},
    "layered_metal": {"type": "layered", "outer": {"type": "glass", "ior": 1.5},
                      "inner": {"type": "metal", "color": [1, 1, 1], "fuzz": 0}},
    "layered_glass": {"type": "layered", "outer": {"type": "glass", "ior": 1.5}, "inner": {"type": "glass", "ior": 1.3}},
}


@pytest.mark.parametrize("name", sorted(GLASSY))
def test_glass_and_layered_directions_equal_the_unreflected_probe_trials(oracle, name):
    mat = GLASSY[name]
    refracted = total = 0
    for din, n in _incidences():
        for front in (True, False):
            valid, refl, dirs = _probe_dirs(oracle, mat, din, n, front, 24)
            cont, d = _ref_dir(mat, din, n, front)
            if refl.all():
                # no trial refracts. For plain glass that is total internal reflection (a Schlick
                # reflectance of 1 also gives it: then the restatement refracts, and is not compared)
                if name.startswith("glass") and not front and (dirs == d).all():
                    total += 1
                continue
            keep = valid & ~refl
            if not keep.any():      # (a layered inner metal may absorb: the probe is invalid, the walk terminal)
                assert not cont or name != "layered_metal"
                continue
            assert cont and (dirs[keep] == d).all(), (name, din, n, front)
            refracted += 1
    assert refracted >= 24
    if name.startswith("glass"):
        assert total >= 4           # back faces beyond the critical angle


def test_total_internal_reflection_is_the_reflected_probe_direction(oracle):
    mat = GLASSY["glass"]
    n = np.asarray([0, 1, 0], F)
    for deg in (45.0, 60.0, 80.0):          # the critical angle of ior 1.5 is 41.8 degrees
        a = np.deg2rad(deg)
        din = np.asarray([np.sin(a), -np.cos(a), 0], F)
        valid, refl, dirs = _probe_dirs(oracle, mat, din, n, False, 8)
        assert valid.all() and refl.all()
        cont, d = _ref_dir(mat, din, n, False)
        assert cont and (dirs == d).all()
        # and the same through a layered material's coat
        lay = GLASSY["layered_metal"]
        valid, refl, dirs = _probe_dirs(oracle, lay, din, n, False, 8)
        assert valid.all() and refl.all()
        assert (dirs == _ref_dir(lay, din, n, False)[1]).all()


def test_mixed_takes_the_likelier_child():
    mirror, paint = {"type": "metal", "color": [1, 1, 1], "fuzz": 0}, {"type": "lambert", "color": [1, 1, 1]}
    din, n = _incidences()[3]
    for w, first in ((0.3, False), (0.5, True), (0.7, True)):
        assert _ref_dir({"type": "mixed", "diff": mirror, "spec": paint, "weight": w}, din, n, True)[0] is first
        assert _ref_dir({"type": "mixed", "diff": paint, "spec": mirror, "weight": w}, din, n, True)[0] is not first


# ---- the walk -----------------------------------------------------------------------------------------
def test_walk_without_specular_materials_is_oracle_guides(rt, oracle):
    """The Cornell box without its two spheres holds no specular material: the walk is the first-hit
    guides in every bit. (The default variant holds a glass sphere: there the pixels off the glass
    are the first-hit guides, and the glass continues.)"""
    ro = {"width": 24}
    sd = rt.generate_scene_data(CORNELL_EMPTY)
    n, P, dist, obj, hit = oracle_guides(oracle, sd, ro)
    wn, wP, wdist, wobj, chain = guide_walk_ref(oracle, sd, ro)
    assert hit.sum() > 400 and (~hit).sum() > 50             # hits and misses both occur
    assert (wn.view(np.uint32) == n.view(np.uint32)).all() and (wP.view(np.uint32) == P.view(np.uint32)).all()
    assert (wdist.view(np.uint32) == dist.view(np.uint32)).all() and (wobj == obj).all()
    assert (chain == np.where(hit, END_SURFACE << 8, 0)).all()
    sd = rt.generate_scene_data({"type": "cornell"})
    glass = next(i for i, o in enumerate(sd["objects"]) if o["material"] == "sphere-glass")
    n, P, dist, obj, hit = oracle_guides(oracle, sd, ro)
    wn, wP, wdist, wobj, chain = guide_walk_ref(oracle, sd, ro)
    off = obj != glass
    assert (~off).sum() > 10 and ((chain[~off] & 0xff) >= 1).all()
    assert (wn[off] == n[off]).all() and (wP[off] == P[off]).all() and (wobj[off] == obj[off]).all()
    assert (wdist[off].view(np.uint32) == dist[off].view(np.uint32)).all()
    assert (chain[off] == np.where(hit[off], END_SURFACE << 8, 0)).all()


def mirror_scene():
    """A fuzz-0 metal quad facing the camera at z = -2 and a Lambert quad behind the camera at z = 3."""
    return {"camera": CAMERA,
            "materials": [{"id": "mirror", "material": {"type": "metal", "color": [0.9, 0.9, 0.9], "fuzz": 0}},
                          {"id": "wall", "material": {"type": "lambert", "color": [0.5, 0.5, 0.5]}}],
            "objects": [{"type": "quad", "pos": [-5, -5, -2], "u": [10, 0, 0], "v": [0, 10, 0], "material": "mirror"},
                        {"type": "quad", "pos": [-20, -20, 3], "u": [40, 0, 0], "v": [0, 40, 0], "material": "wall"}]}


def test_analytic_mirror_and_wall(oracle):
    sd, ro = mirror_scene(), {"width": 16, "aspect": 1}
    fn, fP, fdist, fobj, hit = oracle_guides(oracle, sd, ro)
    assert hit.all() and (fobj == 0).all()                          # the first hit is the mirror everywhere
    n, P, dist, obj, chain = guide_walk_ref(oracle, sd, ro)
    assert (obj == 1).all() and (chain == (1 | END_SURFACE << 8)).all()
    assert (P[..., 2] == 3).all() and (n == np.asarray([0, 0, -1], F)).all()
    # the mirror at z = -2 maps (x, y) to 3.5 (x, y) on the wall at z = 3
    assert np.allclose(P[..., :2], 3.5 * fP[..., :2], rtol=1e-5, atol=1e-6)
    q = (P - fP).astype(F)
    seg = np.sqrt(((q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1]).astype(F) + q[..., 2] * q[..., 2]).astype(F))
    assert (dist.view(np.uint32) == (fdist + seg).astype(F).view(np.uint32)).all()
    assert np.allclose(dist, 3.5 * fdist, rtol=1e-5)
    # one continuation allowed, none left: the wall is reached either way; a mirror pair would stop at 3
    assert (guide_walk_ref(oracle, sd, ro, max_bounces=1)[4] == chain).all()


def test_mirror_room_gains_over_first_hit_guides(oracle):
    """Cornell's JSON with its back wall a fuzz-0 metal (tools/guide_quality.py's mirror room),
    64x64, depth 8, the oracle's spp 8 frame through denoise_ref with both guide sets, against its
    512-sample frame of another seed. Display-domain MSE, specular-guided / first-hit-guided:
    measured 0.7881 (0.011734 / 0.014890; the raw frame 0.017550), a gain of 0.2119; asserted with
    half of it as margin."""
    import copy
    import json
    from denoise_ref import denoise_ref, display_mse
    sd = copy.deepcopy(json.loads((Path(__file__).resolve().parent / "golden/scene_cornell.json").read_text())["scene"])
    sd["materials"].append({"id": "mirror", "material": {"type": "metal", "color": [0.9, 0.9, 0.9], "fuzz": 0}})
    sd["objects"][2]["material"] = "mirror"
    ro = {"width": 64, "depth": 8, "aTolerance": 0}
    conv = oracle.render(sd, {**ro, "samples": 512, "seed": 977}, threads=8)["radiance"]
    noisy = oracle.render(sd, {**ro, "samples": 8}, threads=8)["radiance"]
    first = display_mse(denoise_ref(noisy, *oracle_guides(oracle, sd, ro)[:4]), conv)
    spec = display_mse(denoise_ref(noisy, *guide_walk_ref(oracle, sd, ro)[:4]), conv)
    print(f"mirror room 64x64 spp 8: first-hit {first:.6f}, specular {spec:.6f}, ratio {spec / first:.4f}, "
          f"raw {display_mse(noisy, conv):.6f}")
    assert spec / first <= 1.0 - 0.2119 / 2


# ---- errors and state that need no device -----------------------------------------------------------------
BAD = [((2, 8, 0.0), "mode"), ((-1, 8, 0.0), "mode"), ((1, 0, 0.0), "max_bounces"), ((1, 65, 0.0), "max_bounces"),
       ((0, -3, 0.0), "max_bounces"), ((1, 8, -0.5), "max_fuzz"), ((1, 8, float("nan")), "max_fuzz"),
       ((0, 8, float("inf")), "max_fuzz")]


@pytest.mark.parametrize("fields,word", BAD)
def test_bad_options_are_invalid_without_a_device(rt, fields, word):
    from raytracer_amd import _lib
    lib = _lib.load()
    cam = rt.create_camera_from_scene_data(mirror_scene(), {"width": 16, "aspect": 1})
    o = _lib.RtGuideOptions(*fields)
    obj = np.full((16, 16), -7, np.int32)
    assert lib.rt_camera_render_guides_ex(cam._h, None, C.byref(o), None, None, None, obj.ctypes.data,
                                          None) == _lib.RT_ERR_INVALID
    assert b"rt_camera_render_guides_ex" in lib.rt_last_error() and word.encode() in lib.rt_last_error()
    assert (obj == -7).all()
    assert lib.rt_camera_set_denoise_guides(cam._h, C.byref(o)) == _lib.RT_ERR_INVALID
    assert b"rt_camera_set_denoise_guides" in lib.rt_last_error() and word.encode() in lib.rt_last_error()
    got = _lib.RtGuideOptions(9, 9, 9.0)
    assert lib.rt_camera_get_denoise_guides(cam._h, C.byref(got)) == _lib.RT_OK
    assert (got.mode, got.max_bounces, got.max_fuzz) == (0, 8, 0.0)   # a refused set changes nothing


def test_python_arguments_are_checked_without_a_device(rt):
    from raytracer_amd import _lib
    cam = rt.create_camera_from_scene_data(mirror_scene(), {"width": 16, "aspect": 1})
    rad = np.zeros((16, 16, 3), np.float32)
    for kw in ({"max_bounces": 0}, {"max_bounces": 65}, {"max_fuzz": -1.0}, {"max_fuzz": float("inf")}):
        with pytest.raises(rt.RtError) as e:
            cam.render_guides(through_specular=True, **kw)
        assert e.value.code == _lib.RT_ERR_INVALID
        with pytest.raises(rt.RtError) as e:
            cam.denoise(rad, guides=kw)
        assert e.value.code == _lib.RT_ERR_INVALID
    for bad in ("mirror", None, {"bounces": 3}, 1):
        with pytest.raises(ValueError):
            cam.denoise(rad, guides=bad)
    with pytest.raises(rt.RtError, match="region is empty"):
        cam.render_guides((40, 40, 4, 4), through_specular=True)


def test_setter_getter_round_trip(rt):
    from raytracer_amd import _lib
    lib = _lib.load()
    cam = rt.create_camera_from_scene_data(mirror_scene(), {"width": 16, "aspect": 1})

    def get():
        g = _lib.RtGuideOptions(9, 9, 9.0)
        assert lib.rt_camera_get_denoise_guides(cam._h, C.byref(g)) == _lib.RT_OK
        return g.mode, g.max_bounces, g.max_fuzz

    assert get() == (0, 8, 0.0)                         # never set: first hit
    assert lib.rt_camera_set_denoise_guides(cam._h, C.byref(_lib.RtGuideOptions(1, 5, 0.25))) == _lib.RT_OK
    assert get() == (1, 5, 0.25)
    assert lib.rt_camera_set_denoise_guides(cam._h, C.byref(_lib.RtGuideOptions(1, 64, 0.0))) == _lib.RT_OK
    assert get() == (1, 64, 0.0)
    assert lib.rt_camera_set_denoise_guides(cam._h, None) == _lib.RT_OK
    assert get() == (0, 8, 0.0)                         # NULL: the default
    assert lib.rt_camera_get_denoise_guides(cam._h, None) == _lib.RT_ERR_INVALID
    assert lib.rt_camera_set_denoise_guides(None, None) == _lib.RT_ERR_INVALID
    assert lib.rt_camera_get_denoise_guides(None, C.byref(_lib.RtGuideOptions())) == _lib.RT_ERR_INVALID
