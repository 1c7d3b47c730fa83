"""Guides through the specular chain on the GPU. Every comparison is exact (== on bits, NaN equal
to NaN): the guides and the chain word against the restatement (tests/guide_walk_ref.py, the
normative definition, which walks through the CPU oracle's world_hit), the filter against
tests/denoise_ref.py / tests/denoise_var_ref.py applied to the restated guides.

A metal hit whose mirror direction points into the surface cannot be constructed at a pixel: the
guide normal faces the ray, so f . n = -(unit(d) . n) >= 0, and it is 0 only for a ray exactly
tangent to the surface, which a pixel grid does not produce on purpose. The branch is pinned on the
host (test_guide_walk_abi.py, a direction leaving the surface)."""
import ctypes as C
import functools
import json
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
from denoise_ref import bits_equal, denoise_ref, oracle_guides, to_u8_ref  # noqa: E402
from denoise_var_ref import denoise_var_ref  # noqa: E402
from guide_walk_ref import (END_BOUNCES, END_LEFT, END_MISS, END_SURFACE, F, dielectric_dir, guide_walk_ref,  # noqa: E402
                            primary_rays)
from reproject_ref import moved_scene, reproject_ref  # noqa: E402

pytestmark = pytest.mark.gpu

REGION = (5, 3, 29, 31)
CORNELL = {"type": "cornell"}
DEFAULT = {"type": "default"}
SPHERES200 = {"type": "spheres", "options": {"count": 200, "seed": 3}}
SPHERES200_RO = {"width": 48, "aspect": 1}
SPHERES6000 = {"type": "spheres", "options": {"count": 6000, "seed": 3}}
KEYS = ("normal", "position", "distance", "object", "chain")


@functools.lru_cache(maxsize=None)
def _scene(rt, key):
    return rt.generate_scene_data(json.loads(key))


def scene(rt, cfg):
    return _scene(rt, json.dumps(cfg, sort_keys=True))


_REF = {}


def walk_of_ref(oracle, sd, ro, max_bounces=8, max_fuzz=0.0):
    """The restated (normal, position, distance, object, chain), computed once, read-only."""
    key = (json.dumps(sd, sort_keys=True), json.dumps(ro, sort_keys=True), max_bounces, max_fuzz)
    if key not in _REF:
        g = guide_walk_ref(oracle, sd, ro, max_bounces, max_fuzz)
        for a in g:
            a.setflags(write=False)
        _REF[key] = g
    return _REF[key]


def codes(chain):
    return chain & 0xff, chain >> 8


def assert_walk_is_ref(g, ref, what, box=None):
    ys, xs = box or (slice(None), slice(None))
    bad = {k: int((~bits_equal(g[k][ys, xs], r[ys, xs])).reshape(r[ys, xs].shape[:2] + (-1,)).any(-1).sum())
           for k, r in zip(KEYS, ref)}
    k, end = codes(ref[4][ys, xs])
    hist = {int(e): int((end == e).sum()) for e in np.unique(end)}
    print(f"{what}: end codes {hist}, continuations up to {int(k.max())}; pixels differing from the restatement: {bad}")
    assert not any(bad.values()), (what, bad)


def assert_occurs(ref, what, ends=(), k_min=2):
    k, end = codes(ref[4])
    for e in ends:
        assert (end == e).any(), f"{what}: end code {e} does not occur"
    assert (k >= k_min).any(), f"{what}: no pixel continues {k_min} times"


# ---- 1. guides and chain against the restatement: the generated scenes -----------------------------
def test_default_scene(rt, gpu, oracle):
    """Mirror, glass (a hollow ball around a Lambert core), layered paint, plane, sphere light; the
    camera's aperture is ignored."""
    sd, ro = scene(rt, DEFAULT), {"width": 40}
    assert sd["camera"]["aperture"] > 0
    cam = rt.create_camera_from_scene_data(sd, ro)
    ref = walk_of_ref(oracle, sd, ro)
    g = cam.render_guides(through_specular=True)
    assert g["chain"].dtype == np.int32 and g["chain"].shape == (cam.image_height, cam.image_width)
    assert_walk_is_ref(g, ref, "default")
    assert_occurs(ref, "default", ends=(END_MISS, END_SURFACE, END_LEFT))
    first = cam.render_guides()
    assert "chain" not in first
    moved = (g["object"] != first["object"]) | (g["position"] != first["position"]).any(-1)
    assert ((g["chain"] & 0xff) >= 1)[moved].all() and moved.sum() > 20
    ref25 = walk_of_ref(oracle, sd, ro, 8, 0.25)          # (gold's fuzz is 0.5: still terminal)
    assert_walk_is_ref(cam.render_guides(through_specular=True, max_fuzz=0.25), ref25, "default max_fuzz 0.25")


def test_spheres200_does_not_depend_on_traversal_or_precision(rt, gpu, oracle):
    sd = scene(rt, SPHERES200)
    ref = walk_of_ref(oracle, sd, SPHERES200_RO)
    assert_occurs(ref, "spheres200", ends=(END_MISS, END_SURFACE, END_LEFT))
    for trav in ("reference", "fast", "brute"):
        cam = rt.create_camera_from_scene_data(sd, {**SPHERES200_RO, "traversal": trav})
        assert_walk_is_ref(cam.render_guides(through_specular=True), ref, f"traversal {trav}")
    cam = rt.create_camera_from_scene_data(sd, SPHERES200_RO)
    cam.set_precision("fp32")
    assert_walk_is_ref(cam.render_guides(through_specular=True), ref, "precision fp32")
    # fuzzy metals followed: another walk, one more bounce budget
    ref25 = walk_of_ref(oracle, sd, SPHERES200_RO, 12, 0.25)
    assert (ref25[4] != ref[4]).any()
    assert_walk_is_ref(cam.render_guides(through_specular=True, max_bounces=12, max_fuzz=0.25), ref25, "max_fuzz 0.25")


def test_spheres6000_tree_in_global_memory(rt, gpu, oracle):
    sd, ro = scene(rt, SPHERES6000), {"width": 32}
    cam = rt.create_camera_from_scene_data(sd, ro)
    ref = walk_of_ref(oracle, sd, ro)
    assert_walk_is_ref(cam.render_guides(through_specular=True), ref, "spheres6000")
    assert_occurs(ref, "spheres6000", ends=(END_SURFACE,), k_min=1)


# ---- 2. custom scenes of at most 8 objects -----------------------------------------------------------
SKY = {"type": "gradient", "top": [1, 1, 1], "bottom": [0.5, 0.7, 1]}
RO = {"width": 24, "aspect": 1}


def camera(frm=(0, 0, 0), at=(0, 0, -1), vfov=50):
    return {"vfov": vfov, "aperture": 0, "focus": 1, "from": list(frm), "at": list(at), "up": [0, 1, 0], "background": SKY}


def mat(kind, **kw):
    return {"type": kind, **kw}


MIRROR = mat("metal", color=[0.9, 0.9, 0.9], fuzz=0)
PAINT = mat("lambert", color=[0.5, 0.4, 0.3])
GLASS = mat("glass", ior=1.5)


def sphere(pos, r, m):
    return {"type": "sphere", "pos": list(pos), "r": r, "material": m}


def quad(pos, u, v, m):
    return {"type": "quad", "pos": list(pos), "u": list(u), "v": list(v), "material": m}


def custom(objects, **cam):
    assert len(objects) <= 8
    return {"camera": camera(**cam), "materials": [], "objects": objects}


def facing_mirrors():
    return custom([quad((-4, -4, -3), (8, 0, 0), (0, 8, 0), MIRROR), quad((-4, -4, 3), (8, 0, 0), (0, 8, 0), MIRROR),
                   sphere((0.7, 0.2, -1.5), 0.4, PAINT)])


def sky_balls():
    return custom([sphere((-0.7, 0, -3), 0.6, GLASS), sphere((0.7, 0, -3), 0.6, mat("metal", color=[0.9, 0.5, 0.5], fuzz=0))])


def inside_glass():
    return custom([sphere((0, 0, 0), 5, GLASS), quad((-30, -8, -30), (60, 0, 0), (0, 0, 60), PAINT)],
                  frm=(0, 0, 4), at=(1, -0.2, 4.4), vfov=70)


def hollow_shell():
    return custom([sphere((0, 0, -3), 1.0, GLASS), sphere((0, 0, -3), -0.9, GLASS),
                   quad((-10, -10, -6), (20, 0, 0), (0, 20, 0), PAINT)])


def fuzzy_metals():
    return custom([sphere((-0.8, 0, -3), 0.7, MIRROR), sphere((0.8, 0, -3), 0.7, mat("metal", color=[0.8, 0.8, 0.8], fuzz=0.2)),
                   quad((-10, -0.7, -10), (20, 0, 0), (0, 0, 20), PAINT)])


def mixed_balls():
    balls = []
    for row, (diff, spec) in enumerate(((MIRROR, PAINT), (PAINT, MIRROR))):
        for col, w in enumerate((0.3, 0.5, 0.7)):
            balls.append(sphere((col - 1.0, 0.55 - 1.1 * row, -3), 0.45, mat("mixed", diff=diff, spec=spec, weight=w)))
    return custom(balls + [quad((-10, -10, -6), (20, 0, 0), (0, 20, 0), PAINT)])


def layered_balls():
    coat = mat("glass", ior=1.5)
    return custom([sphere((-0.8, 0, -3), 0.7, mat("layered", outer=coat, inner=PAINT)),
                   sphere((0.8, 0, -3), 0.7, mat("layered", outer=coat, inner=MIRROR)),
                   quad((-10, -0.7, -10), (20, 0, 0), (0, 0, 20), PAINT)])


def run_custom(rt, oracle, sd, what, ends, k_min=2, **opts):
    cam = rt.create_camera_from_scene_data(sd, RO)
    ref = walk_of_ref(oracle, sd, RO, opts.get("max_bounces", 8), opts.get("max_fuzz", 0.0))
    assert_walk_is_ref(cam.render_guides(through_specular=True, **opts), ref, f"{what} {opts}")
    assert_occurs(ref, what, ends, k_min)
    return ref


@pytest.mark.parametrize("max_bounces", [1, 3, 8])
def test_facing_mirrors_reach_max_bounces(rt, gpu, oracle, max_bounces):
    ref = run_custom(rt, oracle, facing_mirrors(), "facing mirrors", (END_SURFACE, END_BOUNCES), k_min=max_bounces,
                     max_bounces=max_bounces)
    k, end = codes(ref[4])
    assert (k[end == END_BOUNCES] == max_bounces).all() and (k <= max_bounces).all()


def test_glass_and_mirror_before_the_sky(rt, gpu, oracle):
    ref = run_custom(rt, oracle, sky_balls(), "sky balls", (END_MISS, END_LEFT))
    k, end = codes(ref[4])
    assert (end != END_SURFACE).all()                        # nothing terminal in the scene
    assert (ref[3][end == END_LEFT] >= 0).all() and (ref[3][end == END_MISS] == -1).all()


def test_camera_inside_glass_total_internal_reflection(rt, gpu, oracle):
    sd = inside_glass()
    ref = run_custom(rt, oracle, sd, "inside glass", (END_SURFACE,))
    # segment 0 leaves through a back face; where ratio * sinT > 1 the continuation is the reflection
    n, _, _, obj, hit = oracle_guides(oracle, sd, RO)
    _, d, W, H = primary_rays(oracle, sd, RO)
    assert hit.all() and (obj == 0).all()
    reflected = dielectric_dir(1.5, np.zeros(W * H, bool), d, n.reshape(-1, 3))[1]
    assert 20 < reflected.sum() < W * H - 20                # both continuations occur


def test_hollow_glass_shell(rt, gpu, oracle):
    ref = run_custom(rt, oracle, hollow_shell(), "hollow shell", (END_SURFACE,), k_min=4)   # four interfaces


@pytest.mark.parametrize("max_fuzz", [0.0, 0.25])
def test_metals_of_fuzz_0_and_02(rt, gpu, oracle, max_fuzz):
    sd = fuzzy_metals()
    ref = run_custom(rt, oracle, sd, "fuzzy metals", (END_SURFACE, END_LEFT), k_min=1, max_fuzz=max_fuzz)
    first = oracle_guides(oracle, sd, RO)[3]
    k, _ = codes(ref[4])
    assert (k[first == 0] >= 1).all() and ((k[first == 1] >= 1).all() if max_fuzz else (k[first == 1] == 0).all())
    assert (first == 1).sum() > 20


def test_mixed_materials_take_the_likelier_child(rt, gpu, oracle):
    sd = mixed_balls()
    ref = run_custom(rt, oracle, sd, "mixed", (END_SURFACE,), k_min=1)
    first = oracle_guides(oracle, sd, RO)[3]
    k, _ = codes(ref[4])
    for o, mirror in enumerate((False, True, True, True, False, False)):   # diff = mirror at w >= 0.5; spec = mirror below
        assert (first == o).sum() >= 4, o
        assert ((k[first == o] >= 1) == mirror).all(), o


def test_layered_over_lambert_and_over_a_mirror(rt, gpu, oracle):
    sd = layered_balls()
    ref = run_custom(rt, oracle, sd, "layered", (END_SURFACE, END_LEFT), k_min=1)
    first = oracle_guides(oracle, sd, RO)[3]
    k, _ = codes(ref[4])
    assert (k[first == 0] == 0).all() and (first == 0).sum() > 20      # a refracting coat over paint: terminal
    assert (k[first == 1] >= 1).all() and (first == 1).sum() > 20      # over a mirror: continues


# ---- 3. regions and omitted outputs -------------------------------------------------------------------
def test_region_leaves_the_rest_untouched_and_outputs_may_be_omitted(rt, gpu, oracle):
    from raytracer_amd import _lib
    sd = scene(rt, SPHERES200)
    cam = rt.create_camera_from_scene_data(sd, SPHERES200_RO)
    ref = walk_of_ref(oracle, sd, SPHERES200_RO)
    H, W = cam.image_height, cam.image_width
    x, y, w, h = REGION
    box = (slice(y, y + h), slice(x, x + w))
    mask = np.ones((H, W), bool)
    mask[box] = False
    opts = _lib.RtGuideOptions(_lib.GUIDES_SPECULAR, 8, 0.0)
    reg = _lib.RtRegion(*REGION)

    def call(region, keep):
        g = {"normal": np.full((H, W, 3), -123.25, np.float32), "position": np.full((H, W, 3), -123.25, np.float32),
             "distance": np.full((H, W), -123.25, np.float32), "object": np.full((H, W), -7, np.int32),
             "chain": np.full((H, W), -7, np.int32)}
        ptr = [g[k].ctypes.data if k in keep else None for k in KEYS]
        _lib.check(cam._lib.rt_camera_render_guides_ex(cam._h, region, C.byref(opts), *ptr))
        return g

    g = call(C.byref(reg), KEYS)
    assert_walk_is_ref(g, ref, "region", box)
    for k in KEYS:
        assert (g[k][mask] == (-7 if g[k].dtype == np.int32 else np.float32(-123.25))).all(), k
    gp = cam.render_guides(REGION, through_specular=True)    # the Python method: zeros / -1 outside the region
    assert (gp["object"][mask] == -1).all() and (gp["chain"][mask] == 0).all() and (gp["normal"][mask] == 0).all()
    assert all(bits_equal(gp[k][box], g[k][box]).all() for k in KEYS)
    for omit in KEYS:                                        # each output omitted
        keep = [k for k in KEYS if k != omit]
        g = call(None, keep)
        assert_walk_is_ref({**g, omit: ref[KEYS.index(omit)]}, ref, f"without {omit}")
        assert (g[omit] == (-7 if g[omit].dtype == np.int32 else np.float32(-123.25))).all()


# ---- 4. mode 0 through _ex ------------------------------------------------------------------------------
def test_first_hit_mode_is_render_guides(rt, gpu):
    from raytracer_amd import _lib
    for cfg, ro in ((DEFAULT, {"width": 40}), (CORNELL, {"width": 40})):
        cam = rt.create_camera_from_scene_data(scene(rt, cfg), ro)
        H, W = cam.image_height, cam.image_width
        want = cam.render_guides()
        g = {"normal": np.zeros((H, W, 3), np.float32), "position": np.zeros((H, W, 3), np.float32),
             "distance": np.zeros((H, W), np.float32), "object": np.zeros((H, W), np.int32),
             "chain": np.full((H, W), -7, np.int32)}
        for opts in (None, C.byref(_lib.RtGuideOptions(_lib.GUIDES_FIRST_HIT, 3, 0.5))):
            _lib.check(cam._lib.rt_camera_render_guides_ex(cam._h, None, opts, *[g[k].ctypes.data for k in KEYS]))
            assert all(bits_equal(g[k], want[k]).all() for k in KEYS[:4])
            assert (g["chain"] == np.where(want["object"] >= 0, END_SURFACE << 8, 0)).all()


def test_a_scene_without_specular_materials_gives_the_first_hit_guides(rt, gpu):
    """The Cornell box without its spheres (the default variant holds a glass ball: there the
    pixels off the ball are equal, and the ball's pixels continue)."""
    cam = rt.create_camera_from_scene_data(scene(rt, {"type": "cornell", "options": {"variant": "empty"}}), {"width": 40})
    first, spec = cam.render_guides(), cam.render_guides(through_specular=True)
    assert all(bits_equal(first[k], spec[k]).all() for k in KEYS[:4])
    assert (spec["chain"] == np.where(first["object"] >= 0, END_SURFACE << 8, 0)).all() and (first["object"] >= 0).any()
    sd = scene(rt, CORNELL)
    glass = next(i for i, o in enumerate(sd["objects"]) if o["material"] == "sphere-glass")
    cam = rt.create_camera_from_scene_data(sd, {"width": 40})
    first, spec = cam.render_guides(), cam.render_guides(through_specular=True)
    off = first["object"] != glass
    assert (~off).sum() > 20 and ((spec["chain"][~off] & 0xff) >= 1).all()
    assert all(bits_equal(first[k][off], spec[k][off]).all() for k in KEYS[:4])
    assert (spec["chain"][off] == np.where(first["object"][off] >= 0, END_SURFACE << 8, 0)).all()


# ---- 5. the filter ----------------------------------------------------------------------------------------
PROG_RO = {"width": 40, "samples": 16, "depth": 8, "aTolerance": 0}


def _step(cam, pr, n):
    H, W = cam.image_height, cam.image_width
    rgb = np.zeros((H, W, 3), np.uint8)
    rad = np.zeros((H, W, 3), np.float32)
    st = pr.step(n, rgb, radiance=rad)
    return rgb, rad, st


@pytest.fixture(scope="module")
def default40(rt, gpu):
    """The default scene at width 40 after step(4): camera, frame, variance map (read-only)."""
    cam = rt.create_camera_from_scene_data(scene(rt, DEFAULT), PROG_RO)
    with cam.progressive() as pr:
        _, rad, _ = _step(cam, pr, 4)
        var = pr.variance()
    for a in (rad, var):
        a.setflags(write=False)
    return cam, rad, var


def test_camera_denoise_with_specular_guides(rt, oracle, default40):
    cam, rad, var = default40
    before = cam.denoise(rad)                                # before any setter call
    g = cam.render_guides(through_specular=True)
    n, P, dist, obj, _ = walk_of_ref(oracle, scene(rt, DEFAULT), {"width": 40})
    rgb = np.zeros(rad.shape, np.uint8)
    out = cam.denoise(rad, guides="specular", rgb=rgb)
    want = denoise_ref(rad, n, P, dist, obj)
    assert bits_equal(out, rt.denoise(rad, **g)).all() and bits_equal(out, want).all()
    assert (rgb == to_u8_ref(want)).all() and (out != before).any()
    t = cam.denoise_times()
    assert t["guide_ms"] > 0 and t["levels"] == 4
    # the variance form
    v_out = np.zeros(var.shape, np.float32)
    out_v = cam.denoise(rad, guides="specular", variance=var, variance_out=v_out)
    want_v, want_vv = denoise_var_ref(rad, var, n, P, dist, obj)
    assert bits_equal(out_v, want_v).all() and bits_equal(v_out, want_vv).all()
    assert bits_equal(out_v, rt.denoise(rad, **g, variance=var)).all()
    # other options, a region
    o = {"max_bounces": 2, "max_fuzz": 0.5}
    g2 = cam.render_guides(REGION, through_specular=True, **o)
    assert (g2["chain"] != g["chain"]).any()
    assert bits_equal(cam.denoise(rad, REGION, guides=o), rt.denoise(rad, **g2, region=REGION)).all()
    # without the keyword: as before any setter call; "first_hit" restores the default
    assert bits_equal(cam.denoise(rad), before).all()
    cam.denoise(rad, guides="specular")
    assert bits_equal(cam.denoise(rad, guides="first_hit"), before).all()
    assert bits_equal(before, rt.denoise(rad, **cam.render_guides())).all()


# ---- 6. the session -----------------------------------------------------------------------------------------
def test_session_keeps_both_guide_pairs(rt, gpu, oracle):
    sd = scene(rt, DEFAULT)
    msd = moved_scene(sd)
    cam = rt.create_camera_from_scene_data(msd, PROG_RO)
    plain = rt.create_camera_from_scene_data(msd, PROG_RO)   # a session that never denoises
    prev_cam = rt.create_camera_from_scene_data(sd, PROG_RO)
    H, W = cam.image_height, cam.image_width
    prad = np.zeros((prev_cam.image_height, prev_cam.image_width, 3), np.float32)
    prev_cam.render(np.zeros(prad.shape, np.uint8), radiance=prad)
    ro = {"width": 40}
    with cam.progressive() as pr, plain.progressive() as pq:
        _, rad, _ = _step(cam, pr, 4)
        _step(plain, pq, 4)
        pxs = np.full((H, W), 4, np.int32)
        want = {"first_hit": denoise_ref(rad, *oracle_guides(oracle, msd, ro)[:4])}
        for name, (mb, mf) in {"specular": (8, 0.0), "one": (1, 0.0), "fuzzy": (8, 0.5)}.items():
            want[name] = denoise_ref(rad, *walk_of_ref(oracle, msd, ro, mb, mf)[:4])
        assert len({w.tobytes() for w in want.values()}) == 4          # four different results
        kw = {"first_hit": "first_hit", "specular": "specular", "one": {"max_bounces": 1},
              "fuzzy": {"max_fuzz": 0.5}}
        u8 = np.zeros((H, W, 3), np.uint8)
        assert bits_equal(pr.denoised(u8, guides="specular"), want["specular"]).all()
        assert (u8 == to_u8_ref(want["specular"])).all() and cam.denoise_times()["guide_ms"] > 0
        pr.denoised(guides="specular")
        assert cam.denoise_times()["guide_ms"] == 0                     # the kept pair served
        for name in ("first_hit", "specular", "one", "specular", "fuzzy", "first_hit", "one", "fuzzy", "specular"):
            assert bits_equal(pr.denoised(guides=kw[name]), want[name]).all(), name
        assert bits_equal(pr.denoised(), want["first_hit"]).all()
        # reprojection after a specular denoise reads the first-hit guides
        pr.denoised(guides="specular")
        got = pr.reprojected(prev_cam, prad)
        ref = reproject_ref(prad, prev_cam.view(), prev_cam.render_guides(), **cam.render_guides(),
                            reusable=cam.reusable_objects(), radiance=rad, px_samples=pxs)
        assert bits_equal(got, ref["radiance"]).all() and (ref["weight"] > 0).any()
        # later steps are those of a session that never denoised
        rgb_p, rad_p, st_p = _step(cam, pr, 4)
        rgb_q, rad_q, st_q = _step(plain, pq, 4)
        assert (rgb_p == rgb_q).all() and bits_equal(rad_p, rad_q).all()
        assert (st_p.pixels, st_p.samples, st_p.bounces) == (st_q.pixels, st_q.samples, st_q.bounces)
        assert pr.save() == pq.save()
