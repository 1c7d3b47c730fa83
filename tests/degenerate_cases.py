"""Degenerate and non-finite scenes, cameras and render options.

One base scene - a lambert plane, a glass sphere and a tilted quad light under a sky - and
three families of cases on it: scene cases add objects (zero, infinite, NaN, huge and tiny
geometry, coincident primitives, odd materials), camera cases change the camera, option
cases change the RenderOptions. test_degenerate_abi.py (CPU) pins what the host makes of
every case and what the oracle renders; test_degenerate_gpu.py holds the GPU to the oracle.

SCENE_CASES[name] = (objects added, materials added, effective traversal). The effective
traversal is what cam.info["traversal"] must report when auto / fast / brute is asked for:
"reference" - the host's gate (scene_tree.cpp prims_inside_boxes) sends the scene to the
reference walk, "asked" - the scene keeps the traversal asked for (auto: brute force, the
scenes have at most 7 primitives).
"""
import copy

import fp32_cases as fc

NAN = float("nan")
INF = float("inf")

WIDTH, HEIGHT = 48, 32
N = WIDTH * HEIGHT
SEEDS = fc.SEEDS
P = [0.45, 0.4, 0.7]       # where the added primitive stands: right of the glass sphere, in view
P2 = [0.1, 0.25, 1.3]
CAM_FROM = [0, 1.3, 3.4]

# scene cases whose fp32 render is not held to D_gpu <= 2 D_orc + 0.005 N: the fp32 oracle
# itself leaves the ref oracle there (test_degenerate_abi.py measures and pins by how much)
FP32_OUTSIDE = ("r0_light", "huge", "light_nonemissive")


def base_scene():
    return {
        "camera": {"vfov": 45, "from": list(CAM_FROM), "at": [0, 0.45, 0], "up": [0, 1, 0], "aperture": 0.0,
                   "focus": 0, "background": copy.deepcopy(fc.SKY)},
        "render": {"aspect": 1.5},
        "materials": [{"id": "floor", "material": {"type": "lambert", "color": [0.6, 0.6, 0.55]}},
                      {"id": "lamp", "material": {"type": "light", "emit": [9, 8, 7]}},
                      {"id": "red", "material": {"type": "lambert", "color": [0.7, 0.25, 0.2]}},
                      {"id": "glass", "material": {"type": "glass", "ior": 1.5}},
                      {"id": "mirror", "material": {"type": "metal", "color": [0.9, 0.85, 0.8], "fuzz": 0}}],
        "objects": [
            {"type": "plane", "pos": [0, 0, 0], "u": [1, 0, 0], "v": [0, 0, -1], "material": "floor"},
            {"type": "sphere", "pos": [-0.7, 0.5, 0.1], "r": 0.5, "material": "glass"},
            {"type": "quad", "pos": [-1, 2.6, -1], "u": [2, 0, 0], "v": [0, -0.4, 1.5], "material": "lamp",
             "light": True},
        ],
    }


def render_options(**kw):
    return {"width": WIDTH, "samples": 2, "depth": 10, "aTolerance": 0, "seed": 5, **kw}


def _sphere(pos=P, r=0.35, material="red", **kw):
    return {"type": "sphere", "pos": list(pos), "r": r, "material": material, **kw}


def _quad(u, v, pos=P, material="red", **kw):
    return {"type": "quad", "pos": list(pos), "u": list(u), "v": list(v), "material": material, **kw}


def _nested8():
    """n0 .. n7 alternate mixed (spec: the lamp, so the path code keeps an emission stack) and
    layered by id; n8 = mixed(red, mirror) ends the chain."""
    mats = []
    for k in range(8):
        nxt = f"n{k + 1}"
        m = ({"type": "mixed", "diff": nxt, "spec": "lamp", "weight": 0.8} if k % 2 == 0 else
             {"type": "layered", "outer": "glass", "inner": nxt})
        mats.append({"id": f"n{k}", "material": m})
    mats.append({"id": "n8", "material": {"type": "mixed", "diff": "red", "spec": "mirror", "weight": 0.5}})
    return mats


_TILTED = ([0.6, 0, -0.3], [0, 0.55, 0.2])

SCENE_CASES = {
    "r0": ([_sphere(r=0)], [], "reference"),
    "r0_light": ([_sphere(r=0, material="lamp", light=True)], [], "reference"),
    "quad_u_par_v": ([_quad([1, 0, 0], [2, 0, 0])], [], "reference"),
    "quad_u0": ([_quad([0, 0, 0], [0, 0.6, 0])], [], "reference"),
    "quad_light_area0": ([_quad([1, 0, 0], [2, 0, 0], material="lamp", light=True)], [], "reference"),
    "nan_pos": ([_sphere(pos=[NAN, P[1], P[2]])], [], "reference"),
    "inf_r": ([_sphere(r=INF)], [], "reference"),
    "inf_pos": ([_sphere(pos=[INF, P[1], P[2]])], [], "asked"),
    # the floor's 2e-4 slab is below the resolution of a ray origin at 1e30; the tiny spheres'
    # boxes have no extent in fp32 (scene_tree.cpp boxes_keep_their_extent)
    "huge": ([_sphere(pos=[1e30, 0, 0], r=1e30), _sphere(pos=[0, 0, -1e39], r=1e38)], [], "reference"),
    "tiny": ([_sphere(r=1e-30), _sphere(pos=P2, r=1e-42)], [], "reference"),
    "coincident": ([_sphere(), _sphere(material="mirror"), _quad(*_TILTED, pos=P2),
                    _quad(*_TILTED, pos=P2, material="mirror")], [], "asked"),
    "ior0": ([_sphere(material="g")], [{"id": "g", "material": {"type": "glass", "ior": 0}}], "asked"),
    "ior_neg": ([_sphere(material="g")], [{"id": "g", "material": {"type": "glass", "ior": -1.5}}], "asked"),
    "ior_nan": ([_sphere(material="g")], [{"id": "g", "material": {"type": "glass", "ior": NAN}}], "asked"),
    "ior1": ([_sphere(material="g")], [{"id": "g", "material": {"type": "glass", "ior": 1}}], "asked"),
    "weight_nan": ([_sphere(material="w")],
                   [{"id": "w", "material": {"type": "mixed", "diff": "red", "spec": "mirror", "weight": NAN}}],
                   "asked"),
    "emit_neg_inf": ([_sphere(material="e", light=True)],
                     [{"id": "e", "material": {"type": "light", "emit": [-1, INF, 0]}}], "asked"),
    "albedo_nan": ([_sphere(material="a")], [{"id": "a", "material": {"type": "lambert", "color": [NAN, 2, -1]}}],
                   "asked"),
    "light_nonemissive": ([_sphere(light=True)], [], "asked"),
    # a plane has no pdf in the reference ('pdf' in object is false), so it is no light
    "plane_light": ([{"type": "plane", "pos": [0, 5, 0], "u": [1, 0, 0], "v": [0, 0, 1], "material": "lamp",
                      "light": True}], [], "asked"),
    "cam_inside": ([_sphere(pos=CAM_FROM, r=0.5, material="glass")], [], "asked"),
    "cam_on_surface": ([_sphere(pos=[0, 1.3, 3.9], r=0.5)], [], "asked"),
    "nested8": ([_sphere(material="n0")], _nested8(), "asked"),
}

CAMERA_CASES = {
    "vfov_missing": {"vfov": None},          # the key is removed: a NaN frame
    "from_eq_at": {"at": list(CAM_FROM)},
    "vfov0": {"vfov": 0},
    "vfov180": {"vfov": 180},
    "vfov_neg": {"vfov": -45},
    "aperture_neg": {"aperture": -0.2},
    "aperture_nan": {"aperture": NAN},
    "aperture_inf": {"aperture": INF},
    "focus_neg": {"focus": -2, "aperture": 0.1},
    "from_nan": {"from": [NAN, 1.3, 3.4]},
    "from_far": {"from": [0, 1e20, 0]},
    "bg_nan": {"background": {"type": "gradient", "top": [NAN, 0.7, 1.0], "bottom": [1, 1, 1]}},
    "bg_inf": {"background": {"type": "gradient", "top": [0.5, INF, 1.0], "bottom": [1, 1, 1]}},
    "bg_neg": {"background": {"type": "gradient", "top": [0.5, 0.7, -1], "bottom": [1, -1, 1]}},
}

# camera cases the same gate sends to the reference walk: a centre 1e20 above the floor's slab, a NaN centre
CAMERA_REFERENCE = ("from_nan", "from_far")

_ADAPT = {"samples": 20}
OPTION_CASES = {
    "samples0": {"samples": 0},
    "samples2_5": {"samples": 2.5},
    "samples_neg": {"samples": -3},
    "samples_nan": {"samples": NAN},
    "depth0": {"depth": 0},
    "depth_neg": {"depth": -1},
    "depth0_5": {"depth": 0.5},
    "rdepth0": {"rouletteDepth": 0},
    "rdepth_neg": {"rouletteDepth": -1},
    "rdepth_nan": {"rouletteDepth": NAN},
    "abatch0": {**_ADAPT, "aTolerance": 0.05, "aBatch": 0},
    "abatch_nan": {**_ADAPT, "aTolerance": 0.05, "aBatch": NAN},
    "abatch_neg": {**_ADAPT, "aTolerance": 0.05, "aBatch": -2},
    "atol_nan": {**_ADAPT, "aTolerance": NAN},
    "atol_inf": {**_ADAPT, "aTolerance": INF},
    "atol_neg": {**_ADAPT, "aTolerance": -1},
    "tall_1x1000": {"width": 1, "aspect": 1e-3},
    "width0": {"width": 0},
    "seed_2p32_5": {"seed": 2 ** 32 + 5},
    "seed_neg": {"seed": -1},
    "seed1_5": {"seed": 1.5},
}

# what build_scene makes of the seed cases (non-finite -> 0, else truncated, modulo 2^32)
SEED_WORDS = {"seed_2p32_5": 5, "seed_neg": 2 ** 32 - 1, "seed1_5": 1}


def effective_traversal(name):
    """"reference": the case reports the reference walk whatever is asked for; "asked" otherwise."""
    if name in SCENE_CASES:
        return SCENE_CASES[name][2]
    return "reference" if name in CAMERA_REFERENCE else "asked"


# scene cases whose paths keep an emission stack, which the pool kernel does not have: the nested
# mixtures emit, a NaN mixture weight makes the mixture's emission NaN, a NaN albedo makes the
# throughput NaN and with it the zero emission of every later hit (scene.cpp)
EMISSION_STACK = ("nested8", "weight_nan", "albedo_nan")


def scene_names():
    return list(SCENE_CASES)


def camera_names():
    return list(CAMERA_CASES)


def option_names():
    return list(OPTION_CASES)


def all_names():
    return scene_names() + camera_names() + option_names()


def case(name, **ro):
    """(SceneData, RenderOptions) of a case of any family; `ro` overrides render options."""
    sd = base_scene()
    opts = render_options()
    if name in SCENE_CASES:
        objs, mats, _ = SCENE_CASES[name]
        sd["objects"] += copy.deepcopy(objs)
        sd["materials"] += copy.deepcopy(mats)
    elif name in CAMERA_CASES:
        for k, v in CAMERA_CASES[name].items():
            if v is None:
                del sd["camera"][k]
            else:
                sd["camera"][k] = copy.deepcopy(v)
    elif name != "base":
        opts.update(OPTION_CASES[name])
    opts.update(ro)
    return sd, opts


def sample_case(name, seed):
    """A scene case as the fp32 per-sample measure renders it: one sample per pixel."""
    return case(name, samples=1, seed=seed)


def added_pos(name):
    """`pos` of the first object a scene case adds."""
    return list(SCENE_CASES[name][0][0]["pos"])


_ORACLE = {}


def oracle_render(oracle, name, precision="ref", **ro):
    """The oracle's frame of a case, rendered once per session and left unchanged."""
    key = (name, precision, tuple(sorted(ro.items())))
    if key not in _ORACLE:
        sd, opts = case(name, **ro)
        _ORACLE[key] = oracle.render(sd, opts, precision=precision, threads=4)
    return _ORACLE[key]


def d_orc(oracle, name, seed):
    """(disagreeing samples of the fp32 oracle with the ref oracle, new non-finite samples)."""
    ref = oracle_render(oracle, name, samples=1, seed=seed)
    f32 = oracle_render(oracle, name, "fp32", samples=1, seed=seed)
    return fc.disagreeing(f32["radiance"], f32["px_bounces"], ref), fc.new_nonfinite(f32["radiance"], ref["radiance"])
