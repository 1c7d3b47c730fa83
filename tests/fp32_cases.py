"""Scenes and the per-sample measure of the fp32 precision tests.

Every case renders one sample per pixel with adaptive sampling off, so a pixel
is one path with the oracle's draws and `px_bounces` is that path's bounce
count. A sample *agrees* with the ref oracle (fp64 scalars) when its bounce
count is equal and every channel is within 1e-4 + 1e-4|c_ref| (NaN matching
NaN). A sample that does not agree took another branch: an fp32 rounding moved
a comparison. How often that may happen is set by the oracle's own fp32 mode:

    D_gpu <= 2 * D_orc + 0.005 * N

test_fp32_oracle.py (CPU) bounds D_orc per case, test_fp32_gpu.py applies the
condition to the GPU's fp32 render.
"""
import copy
import functools

import numpy as np

WIDTH = 64
SEEDS = (1, 77)
SKY = {"type": "gradient", "top": [0.5, 0.7, 1.0], "bottom": [1, 1, 1]}
BLACK = {"type": "gradient", "top": [0, 0, 0], "bottom": [0, 0, 0]}

MATERIALS = {
    "lambert": {"type": "lambert", "color": [0.7, 0.4, 0.3]},
    "mirror": {"type": "metal", "color": [0.9, 0.85, 0.8], "fuzz": 0},
    "fuzzy": {"type": "metal", "color": [0.9, 0.85, 0.8], "fuzz": 0.3},
    "glass": {"type": "glass", "ior": 1.5},
    "mixed": {"type": "mixed", "diff": {"type": "lambert", "color": [0.7, 0.4, 0.3]},
              "spec": {"type": "metal", "color": [0.9, 0.9, 0.9], "fuzz": 0.05}, "weight": 0.6},
    "layered": {"type": "layered", "outer": {"type": "glass", "ior": 1.5},
                "inner": {"type": "lambert", "color": [0.3, 0.5, 0.8]}},
}
LIGHTS = ("sky", "quad", "sphere")


def ropts(seed, depth=12, **kw):
    return {"width": WIDTH, "samples": 1, "depth": depth, "aTolerance": 0, "seed": seed, **kw}


def matrix_scene(material, light, aperture=0.0):
    """A lambert plane as floor, one sphere and one free-standing quad of the material
    under test. The quad leans towards the camera, so the camera sees its front and
    bounces off the floor behind it reach its back."""
    objs = [
        {"type": "plane", "pos": [0, 0, 0], "u": [1, 0, 0], "v": [0, 0, -1], "material": "floor"},
        {"type": "sphere", "pos": [-0.7, 0.5, 0.1], "r": 0.5, "material": "test"},
        {"type": "quad", "pos": [0.15, 0.05, -0.2], "u": [1.0, 0, -0.45], "v": [0, 0.95, 0.3], "material": "test"},
    ]
    if light == "quad":
        # tilted: not an axis-aligned quad, so its light PDF takes the general planar test
        objs.append({"type": "quad", "pos": [-1, 2.6, -1], "u": [2, 0, 0], "v": [0, -0.4, 1.5], "material": "lamp",
                     "light": True})
    elif light == "sphere":
        objs.append({"type": "sphere", "pos": [0.4, 2.3, 0.8], "r": 0.4, "material": "lamp", "light": True})
    return {
        "camera": {"vfov": 45, "from": [0, 1.3, 3.4], "at": [0, 0.45, 0], "up": [0, 1, 0], "aperture": aperture,
                   "focus": 0, "background": SKY if light == "sky" else BLACK},
        "render": {"aspect": 1.5},
        "materials": [{"id": "floor", "material": {"type": "lambert", "color": [0.6, 0.6, 0.55]}},
                      {"id": "lamp", "material": {"type": "light", "emit": [9, 8, 7]}},
                      {"id": "test", "material": MATERIALS[material]}],
        "objects": objs,
    }


def mixed_scene():
    """test_gpu_parity._mixed_scene(): an emissive mixture component, a mixed
    metal/glass material and a layered glass/metal material."""
    from test_gpu_parity import _mixed_scene
    return _mixed_scene()


def backface_scene():
    """A lambert plane and a lambert quad whose normals point away from the camera:
    every first hit on either is a back face, so the diffuse bounce reads the
    back-face half of the planar ONB table."""
    return {
        "camera": {"vfov": 50, "from": [0, 1.5, 3], "at": [0, 0.4, 0], "up": [0, 1, 0], "aperture": 0.0, "focus": 0,
                   "background": SKY},
        "render": {"aspect": 1.5},
        "materials": [{"id": "a", "material": {"type": "lambert", "color": [0.7, 0.7, 0.6]}},
                      {"id": "b", "material": {"type": "lambert", "color": [0.3, 0.6, 0.4]}}],
        "objects": [
            {"type": "plane", "pos": [0, 0, 0], "u": [0, 0, -1], "v": [1, 0, 0], "material": "a"},   # normal -y
            {"type": "quad", "pos": [-0.9, 0, -0.5], "u": [0, 1.4, 0.3], "v": [1.8, 0, 0.4], "material": "b"},
            {"type": "sphere", "pos": [0.2, 0.3, 0.9], "r": 0.3, "material": "b"},
        ],
    }


def glass_floor_scene():
    """A glass plane seen at a shallow angle over a lambert plane, and a glass sphere on it:
    1 - cos of the camera rays on the glass is 0.8 - 0.95, where Schlick's fifth power decides
    a reflection on a large share of the frame."""
    return {
        "camera": {"vfov": 45, "from": [0, 0.6, 3.4], "at": [0, 0.25, 0], "up": [0, 1, 0], "aperture": 0.0,
                   "focus": 0, "background": SKY},
        "render": {"aspect": 1.5},
        "materials": [{"id": "glass", "material": MATERIALS["glass"]},
                      {"id": "bed", "material": {"type": "lambert", "color": [0.6, 0.5, 0.3]}}],
        "objects": [
            {"type": "plane", "pos": [0, 0, 0], "u": [1, 0, 0], "v": [0, 0, -1], "material": "glass"},
            {"type": "plane", "pos": [0, -0.5, 0], "u": [1, 0, 0], "v": [0, 0, -1], "material": "bed"},
            {"type": "sphere", "pos": [0.3, 0.5, 0], "r": 0.5, "material": "glass"},
        ],
    }


def ground_scene(r):
    """A ground sphere of radius r under a glass sphere and a fuzzy-metal sphere."""
    return {
        "camera": {"vfov": 40, "from": [0, 1.0, 4], "at": [0, 0.4, 0], "up": [0, 1, 0], "aperture": 0.0, "focus": 0,
                   "background": SKY},
        "render": {"aspect": 1.5},
        "materials": [{"id": "ground", "material": {"type": "lambert", "color": [0.5, 0.6, 0.4]}},
                      {"id": "glass", "material": MATERIALS["glass"]},
                      {"id": "fuzzy", "material": MATERIALS["fuzzy"]}],
        "objects": [
            {"type": "sphere", "pos": [0, -r, 0], "r": r, "material": "ground"},
            {"type": "sphere", "pos": [-0.6, 0.5, 0], "r": 0.5, "material": "glass"},
            {"type": "sphere", "pos": [0.6, 0.5, -0.2], "r": 0.5, "material": "fuzzy"},
        ],
    }


STOCK = {
    "cornell": ({"type": "cornell"}, 16, {}),
    "default": ({"type": "default"}, 12, {}),
    "rain": ({"type": "rain", "options": {"seed": 42}}, 16, {}),
    "spheres500": ({"type": "spheres", "options": {"count": 500, "seed": 42}}, 8, {"aspect": 1}),
}

# D_orc <= ORACLE_BOUND * N, checked on the CPU (test_fp32_oracle.py)
ORACLE_BOUND = {"rain": 0.005, "spheres500": 0.05}
ORACLE_BOUND_DEFAULT = 0.001


def case_names():
    names = [f"{m}-{l}" for m in MATERIALS for l in LIGHTS]
    names += ["mixed-scene", "backface", "defocus", "glass-floor", "ground10", "ground100", "ground1000"]
    return names + list(STOCK)


@functools.lru_cache(maxsize=None)
def _case(name):
    if name in STOCK:
        import raytracer_amd as rt
        cfg, depth, extra = STOCK[name]
        return rt.generate_scene_data(cfg), depth, extra
    if name == "mixed-scene":
        return mixed_scene(), 12, {}
    if name == "backface":
        return backface_scene(), 12, {}
    if name == "defocus":
        return matrix_scene("glass", "quad", aperture=0.2), 12, {}
    if name == "glass-floor":
        return glass_floor_scene(), 12, {}
    if name.startswith("ground"):
        return ground_scene(float(name[6:])), 12, {}
    m, l = name.split("-")
    return matrix_scene(m, l), 12, {}


def case(name, seed):
    """(SceneData, RenderOptions) of a case."""
    sd, depth, extra = _case(name)
    return copy.deepcopy(sd), ropts(seed, depth, **extra)


def agree(rad, bounces, ref_rad, ref_bounces):
    """Per-sample agreement mask (H, W) of a frame with the ref oracle's."""
    a = np.asarray(rad, np.float64)
    b = np.asarray(ref_rad, np.float64)
    with np.errstate(invalid="ignore"):
        close = (np.abs(a - b) <= 1e-4 + 1e-4 * np.abs(b)) | (a == b) | (np.isnan(a) & np.isnan(b))
    return close.all(axis=-1) & (np.asarray(bounces) == np.asarray(ref_bounces))


def disagreeing(rad, bounces, ref):
    return int((~agree(rad, bounces, ref["radiance"], ref["px_bounces"])).sum())


def new_nonfinite(rad, ref_rad):
    """Samples with a non-finite channel where the ref oracle's sample is finite."""
    return int((~np.isfinite(rad).all(axis=-1) & np.isfinite(ref_rad).all(axis=-1)).sum())


_ORACLE = {}


def oracle_pair(oracle, name, seed):
    """The ref and the fp32 oracle's frames of a case, rendered once per session."""
    key = (name, seed)
    if key not in _ORACLE:
        sd, ro = case(name, seed)
        _ORACLE[key] = (oracle.render(sd, ro, threads=8), oracle.render(sd, ro, precision="fp32", threads=8))
    return _ORACLE[key]


# ---------------------------------------------------------------------------
# The hit probe: rays, the residual of a hit point on its primitive, agreement
# ---------------------------------------------------------------------------
FAMILIES = ("base", "surface", "inside", "edges")


def probe_scene(name):
    import raytracer_amd as rt
    from test_gpu_parity import _tiny_scene
    if name == "spheres200":
        return rt.generate_scene_data({"type": "spheres", "options": {"count": 200, "seed": 3}})
    if name in ("cornell", "default"):
        return rt.generate_scene_data({"type": name})
    if name.startswith("tiny"):
        return _tiny_scene(int(name[4:]))
    return ground_scene(1000.0)


PROBE_SCENES = ("cornell", "default", "spheres200", "tiny1", "tiny5", "ground1000")


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def probe_rays(oracle, sd, seed=7):
    """{family: (origins, directions)} as float32. base: 4000 rays, an eighth axis-parallel,
    the rest random (test_world_hit_matches_oracle's); then 500 each: origins on a surface
    (ref hit points of the base rays) leaving at random and at grazing (< 1 degree) angles;
    origins inside spheres and inside the box the scene spans; rays aimed within +-1e-5 of
    quad edges and corners and of sphere silhouettes."""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    n = 4000
    o = rng.uniform(-1.5, 1.5, (n, 3)).astype(f32) + f32([0, 0.5, 0])
    d = rng.normal(size=(n, 3)).astype(f32)
    d[: n // 8, rng.integers(0, 3)] = 0
    fam = {"base": (o, d)}
    m = 500
    # on a surface
    ref = oracle.world_hit(sd, o, d)
    hit = np.flatnonzero(ref[:, 0] > 0)
    pick = hit[np.arange(m) % hit.size]
    p, nr = ref[pick, 2:5], ref[pick, 5:8]
    v = rng.normal(size=(m, 3))
    tang = _unit(v - (v * nr).sum(-1, keepdims=True) * nr)
    th = np.radians(rng.uniform(0, 1, (m, 1)))
    ds = np.where(np.arange(m)[:, None] % 2 == 0, rng.normal(size=(m, 3)), np.cos(th) * tang + np.sin(th) * nr)
    fam["surface"] = (p.astype(f32), ds.astype(f32))
    # inside spheres / inside the box
    spheres = [ob for ob in sd["objects"] if ob["type"] == "sphere"]
    quads = [ob for ob in sd["objects"] if ob["type"] == "quad"]
    oi = np.zeros((m, 3))
    for k in range(m):
        if quads and k % 2:
            oi[k] = rng.uniform(-0.99, 0.99, 3)  # Cornell's box / between default's quads
        else:
            s = spheres[rng.integers(len(spheres))]
            oi[k] = np.asarray(s["pos"], float) + _unit(rng.normal(size=3)) * rng.uniform(0, 0.9) * s["r"]
    fam["inside"] = (oi.astype(f32), rng.normal(size=(m, 3)).astype(f32))
    # edges, corners, silhouettes
    oe = o[:m].astype(np.float64)
    te = np.zeros((m, 3))
    for k in range(m):
        eps = rng.uniform(-1e-5, 1e-5)
        if quads and k % 2:
            q = quads[rng.integers(len(quads))]
            q0, u, w = (np.asarray(q[a], float) for a in ("pos", "u", "v"))
            side = rng.integers(0, 6)
            if side >= 4:  # a corner
                a, b = rng.integers(0, 2, 2)
                te[k] = q0 + a * u + b * w + eps * (_unit(u) + _unit(w))
            else:
                s = rng.uniform(0, 1)
                along, across = (u, w) if side < 2 else (w, u)
                te[k] = q0 + s * along + (side % 2) * across + eps * _unit(across)
        else:
            sp = spheres[rng.integers(len(spheres))]
            c, r = np.asarray(sp["pos"], float), abs(float(sp["r"]))
            L = c - oe[k]
            dist = np.linalg.norm(L)
            if dist <= r + 1e-3:  # origin inside: move it out along -L
                oe[k] = c - _unit(L if dist > 0 else np.array([0, 0, 1.0])) * (2 * r + 1)
                L = c - oe[k]
                dist = np.linalg.norm(L)
            e = rng.normal(size=3)
            e = _unit(e - (e @ L) / dist ** 2 * L)
            rho = (r + eps) * dist / np.sqrt(dist ** 2 - (r + eps) ** 2)  # the ray passes the centre at r + eps
            te[k] = c + rho * e
    fam["edges"] = (oe.astype(f32), (te - oe).astype(f32))
    return fam


def hit_residual(sd, o, d, rows, obj):
    """|distance of o + t d to the reported primitive| / (|o| + |t||d| + |c| + r) (|q| for
    planar primitives), in fp64, for the rows that report a hit (NaN elsewhere)."""
    o = np.asarray(o, np.float64)
    d = np.asarray(d, np.float64)
    out = np.full(len(rows), np.nan)
    for k in np.flatnonzero(rows[:, 0] > 0):
        ob = sd["objects"][int(obj[k])]
        p = o[k] + rows[k, 1] * d[k]
        c = np.asarray(ob["pos"], np.float64)
        scale = np.linalg.norm(o[k]) + abs(rows[k, 1]) * np.linalg.norm(d[k]) + np.linalg.norm(c)
        if ob["type"] == "sphere":
            out[k] = abs(np.linalg.norm(p - c) - abs(ob["r"])) / (scale + abs(ob["r"]))  # default: a shell, r < 0
        else:
            nn = np.cross(np.asarray(ob["u"], np.float64), np.asarray(ob["v"], np.float64))
            out[k] = abs((p - c) @ nn) / np.linalg.norm(nn) / scale
    return out


def hits_agree(rows, obj, ref):
    """Per ray: same hit flag, and on a hit the same object and |t - t_ref| <= 1e-4 (1 + |t_ref|)."""
    same = rows[:, 0] == ref[:, 0]
    h = ref[:, 0] > 0
    ok = (obj == ref[:, 9]) & (np.abs(rows[:, 1] - ref[:, 1]) <= 1e-4 * (1 + np.abs(ref[:, 1])))
    return same & (~h | ok)


_PROBE = {}


def probe_reference(oracle, name):
    """(SceneData, rays, ref oracle rows, fp32 oracle rows) per family, computed once per session."""
    if name not in _PROBE:
        sd = probe_scene(name)
        rays = probe_rays(oracle, sd)
        _PROBE[name] = (sd, rays, {f: oracle.world_hit(sd, *rays[f]) for f in FAMILIES},
                        {f: oracle.world_hit(sd, *rays[f], precision="fp32") for f in FAMILIES})
    return _PROBE[name]


def backface_share(oracle, sd, ro):
    """Share of the frame whose first hit, by the ref oracle, is a back face."""
    info = oracle.camera_info(sd, ro)
    n = info["width"] * info["height"]
    o = np.zeros((n, 3))
    d = np.zeros((n, 3))
    for j in range(info["height"]):
        for i in range(info["width"]):
            o[j * info["width"] + i], d[j * info["width"] + i] = oracle.get_ray(sd, ro, i, j, 0)
    h = oracle.world_hit(sd, o, d)
    return float(((h[:, 0] > 0) & (h[:, 8] == 0)).sum()) / n
