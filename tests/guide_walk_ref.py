"""The normative definition of the guides through the specular chain (rt_camera_render_guides_ex,
RT_GUIDES_SPECULAR; include/rt_amd.h restates it in words, csrc/guide_walk.hip computes it on the
device). Built as oracle_guides in tests/denoise_ref.py is: one pyoracle.world_hit call per segment
over the rays still walking, the materials looked up from the SceneData JSON by the returned
object index, and the direction arithmetic in NumPy float64 with an fp32 store per Vec3 operation
(the reference's gl-matrix Float32Array vectors and JS-number scalars). No random number is drawn:
every draw of Material.scatter is replaced by a policy (continue_dir). A helper module of the
guide-walk tests, not a test file."""
import numpy as np

F = np.float32
D = np.float64
END_MISS, END_SURFACE, END_LEFT, END_BOUNCES = 0, 1, 2, 3


# ---- Vec3 operations: computed in double, each component rounded to fp32 on store ---------------
def scale(a, t):
    return (a.astype(D) * np.asarray(t, D)[..., None]).astype(F)


def dot(a, b):
    a, b = a.astype(D), b.astype(D)
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def unit(a):
    """gl-matrix vec3.normalize: len = x^2 + y^2 + z^2; if (len > 0) len = 1 / sqrt(len)."""
    l = dot(a, a)
    with np.errstate(all="ignore"):
        l = np.where(l > 0, 1.0 / np.sqrt(l), l)
    return scale(a, l)


def neg(a):
    """Vec3.negate: -0 is normalised to +0."""
    r = (-a).astype(F)
    r[r == 0] = 0
    return r


def reflect(v, n):
    """Vec3.reflect: v - n * (2 * (v . n))."""
    return (v - scale(n, 2.0 * dot(v, n))).astype(F)


def dielectric_dir(ior, front, din, n):
    """Dielectric.scatter's direction without its draw: refract whenever ratio * sinT <= 1, reflect
    otherwise (Schlick's reflectance is ignored). Returns (direction, reflected)."""
    with np.errstate(all="ignore"):
        ratio = np.where(front, 1.0 / D(ior), D(ior))
        ud = unit(din)
        cos_t = np.minimum(dot(neg(ud), n), 1.0)
        sin_t = np.sqrt(1.0 - cos_t * cos_t)
        reflected = ratio * sin_t > 1.0
        perp = scale((ud + scale(n, cos_t)).astype(F), ratio)
        par = scale(n, -np.sqrt(np.abs(1.0 - dot(perp, perp))))
        refracted = (perp + par).astype(F)
    return np.where(reflected[..., None], reflect(ud, n), refracted).astype(F), reflected


# ---- materials ------------------------------------------------------------------------------------
def material_of(scene, ref):
    """createMaterial's lookup: an id of SceneData.materials, or an inline material."""
    if isinstance(ref, str):
        return next(m["material"] for m in scene.get("materials", []) if m["id"] == ref)
    return ref


def continue_dir(scene, mat, din, n, front, max_fuzz=0.0):
    """Material.scatter's structure with a policy in place of each draw, for rays `din` (fp32
    (N, 3)) hitting `mat` with normals `n` facing them on the faces `front`: (continues (N,) bool,
    direction fp32 (N, 3), meaningful where it continues).
      lambert, light, none: terminal.
      metal: f = reflect(unit(d), n); terminal when fuzz > max_fuzz or f . n <= 0, else f.
      glass: dielectric_dir; always continues.
      mixed: the child `diff` when its weight >= 0.5, else `spec`.
      layered: the outer dielectric by the glass rule; a reflection continues, a refraction is the
      incoming direction of the inner material at the same hit."""
    mat = material_of(scene, mat)
    kind = mat.get("type") if mat else None
    none = np.zeros(len(din), bool)
    if kind == "metal":
        fuzz = float(mat.get("fuzz", 0.0))
        fuzz = max(0.0, fuzz) if fuzz < 1 else 1.0            # Metal's constructor
        f = reflect(unit(din), n)
        if fuzz > float(F(max_fuzz)):
            return none, f
        return ~(dot(f, n) <= 0.0), f
    if kind == "glass":
        return ~none, dielectric_dir(mat["ior"], front, din, n)[0]
    if kind == "mixed":
        w = float(mat["weight"])
        w = w if w != w else max(0.0, min(1.0, w))             # MixedMaterial's constructor (Math.max / min keep a NaN)
        return continue_dir(scene, mat["diff"] if w >= 0.5 else mat["spec"], din, n, front, max_fuzz)
    if kind == "layered":
        d2, reflected = dielectric_dir(material_of(scene, mat["outer"])["ior"], front, din, n)
        cont, inner = continue_dir(scene, mat["inner"], d2, n, front, max_fuzz)
        return reflected | cont, np.where(reflected[..., None], d2, inner).astype(F)
    return none, np.zeros_like(din)


# ---- the walk ---------------------------------------------------------------------------------------
def primary_rays(oracle, scene, render_opts):
    """Segment 0, the first-hit guides' ray of every pixel: (origin, direction, width, height)."""
    ci = oracle.camera_info(scene, render_opts)
    W, H = ci["width"], ci["height"]
    p00, du, dv, cen = (np.asarray(ci[k], dtype=F) for k in ("pixel00", "du", "dv", "center"))
    i = np.arange(W, dtype=F)[None, :, None]
    j = np.arange(H, dtype=F)[:, None, None]
    pc = ((p00 + du * i).astype(F) + (dv * j).astype(F)).astype(F)
    d = (pc - cen).astype(F).reshape(-1, 3)
    return np.broadcast_to(cen, d.shape).copy(), d, W, H


def walk(oracle, scene, o, d, max_bounces=8, max_fuzz=0.0):
    """The walk of the rays (o, d), fp32 (N, 3): (normal, position, distance, object, chain)."""
    assert 1 <= max_bounces <= 64 and max_fuzz >= 0 and np.isfinite(max_fuzz)
    o, d = o.astype(F).copy(), d.astype(F).copy()
    N = len(o)
    nrm, pos = np.zeros((N, 3), F), np.zeros((N, 3), F)
    dist, obj = np.zeros(N, F), np.full(N, -1, np.int32)
    last = [nrm.copy(), pos.copy(), dist.copy(), obj.copy()]   # the specular surface the chain left through
    acc = np.zeros(N, F)
    k, end = np.zeros(N, np.int32), np.full(N, -1, np.int32)
    act = np.arange(N)
    while act.size:
        wh = oracle.world_hit(scene, o[act], d[act])
        hit = wh[:, 0] > 0
        m = act[~hit]
        end[m] = np.where(k[m] == 0, END_MISS, END_LEFT)
        nrm[m], pos[m], dist[m], obj[m] = (a[m] for a in last)
        a, w = act[hit], wh[hit]
        p, n, front, ob = w[:, 2:5].astype(F), w[:, 5:8].astype(F), w[:, 8] > 0, w[:, 9].astype(np.int32)
        q = (p - o[a]).astype(F)
        acc[a] = acc[a] + np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]).astype(F) + q[:, 2] * q[:, 2]).astype(F))
        nrm[a], pos[a], dist[a], obj[a] = n, p, acc[a], ob
        cont, nd = np.zeros(len(a), bool), np.zeros((len(a), 3), F)
        for x in np.unique(ob):
            s = ob == x
            cont[s], nd[s] = continue_dir(scene, scene["objects"][x].get("material"), d[a][s], n[s], front[s], max_fuzz)
        end[a[~cont]] = END_SURFACE
        capped = cont & (k[a] == max_bounces)
        end[a[capped]] = END_BOUNCES
        go = cont & ~capped
        act = a[go]
        for dst, src in zip(last, (nrm, pos, dist, obj)):
            dst[act] = src[act]
        o[act], d[act] = p[go], nd[go]
        k[act] += 1
    return nrm, pos, dist, obj, (k | end << 8).astype(np.int32)


def guide_walk_ref(oracle, scene, render_opts, max_bounces=8, max_fuzz=0.0):
    """The guides through the specular chain as full-frame arrays (normal, position, distance,
    object, chain), chain = continuations | end code << 8."""
    o, d, W, H = primary_rays(oracle, scene, render_opts)
    n, P, dist, obj, chain = walk(oracle, scene, o, d, max_bounces, max_fuzz)
    return n.reshape(H, W, 3), P.reshape(H, W, 3), dist.reshape(H, W), obj.reshape(H, W), chain.reshape(H, W)
