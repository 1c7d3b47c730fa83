"""Shared pieces of the primary-ray candidate table tests (test_primary_table.py,
test_primary_gpu.py): the custom scene, the record decoding and the per-pixel ray set."""
import numpy as np

_BG = {"type": "gradient", "top": [1, 1, 1], "bottom": [0.5, 0.7, 1.0]}


def _lam(r, g, b):
    return {"type": "lambert", "color": [r, g, b]}


def custom_scene(pool=False):
    """<= 16 primitives, a 120 degree field of view from the origin down -z, built to break a
    conservative table. At width 24 a pixel spans 2 tan(60) / 24 = 0.1443 of the distance.
    `pool`: the 8 of them that a render on the pool kernel can hold."""
    px5 = 5 * 2 * np.tan(np.radians(60)) / 24  # one pixel at distance 5
    objects = [
        # smaller than a pixel (r = 0.1 against 0.72), centred on a corner shared by four pixels
        {"type": "sphere", "pos": [px5, px5, -5], "r": 0.1, "material": _lam(0.9, 0.1, 0.1)},
        # contains the camera (and the whole scene): hit from inside, by the far root
        {"type": "sphere", "pos": [0.5, 0.25, 0.5], "r": 40, "material": _lam(0.5, 0.5, 0.5)},
        # axis quad in the plane x = 0.05 seen edge-on: the centre columns' footprints hold rays
        # parallel to it, rays that hit it and rays that pass on either side
        {"type": "quad", "pos": [0.05, -1, -4], "u": [0, 2, 0], "v": [0, 0, -2], "material": _lam(0.1, 0.8, 0.1)},
        # the same for a plane y = const (rows instead of columns), the other winding
        {"type": "quad", "pos": [-1, -0.02, -3], "u": [0, 0, -1.5], "v": [2, 0, 0], "material": _lam(0.1, 0.1, 0.8)},
        # behind the camera: a sphere and an axis quad
        {"type": "sphere", "pos": [0, 0, 5], "r": 1, "material": _lam(0.7, 0.7, 0.1)},
        {"type": "quad", "pos": [-2, -2, 3], "u": [4, 0, 0], "v": [0, 4, 0], "material": _lam(0.7, 0.1, 0.7)},
        # the bound-0 class: a tilted quad and a plane
        {"type": "quad", "pos": [-3, -2, -6], "u": [2, 0.5, 0], "v": [0, 2, -1], "material": _lam(0.2, 0.6, 0.6)},
        {"type": "plane", "pos": [0, -3, 0], "u": [1, 0, 0], "v": [0, 0, -1], "material": _lam(0.6, 0.6, 0.6)},
        # a wall facing the camera, a sphere in front of it, glass, metal and a light
        {"type": "quad", "pos": [-4, -3, -8], "u": [8, 0, 0], "v": [0, 6, 0], "material": _lam(0.73, 0.73, 0.73)},
        {"type": "sphere", "pos": [1.5, -1, -6], "r": 1.2, "material": {"type": "glass", "ior": 1.5}},
        {"type": "sphere", "pos": [-2, 1.5, -5], "r": 0.8, "material": {"type": "metal", "color": [0.8, 0.8, 0.8],
                                                                       "fuzz": 0.1}},
        {"type": "quad", "pos": [-1, 2.9, -5], "u": [2, 0, 0], "v": [0, 0, -2], "light": True,
         "material": {"type": "light", "emit": [12, 12, 12]}},
    ]
    if pool:
        # the pool kernel's per-wave path pools leave LDS for the candidate columns of 8 primitives
        # (Cornell's count): every class above once, the light included
        objects = [objects[k] for k in (0, 1, 2, 4, 6, 7, 8, 11)]
    return {"camera": {"vfov": 120, "from": [0, 0, 0], "at": [0, 0, -1], "up": [0, 1, 0], "aperture": 0,
                       "background": _BG},
            "render": {"aspect": 1.0, "roulette": True, "rouletteDepth": 3},
            "objects": objects}


def on_plane_scene():
    """The camera origin lies on the planes of two axis quads (x = 0 and y = 0)."""
    objects = [
        {"type": "quad", "pos": [0, -1, -2], "u": [0, 2, 0], "v": [0, 0, -2], "material": _lam(0.8, 0.2, 0.2)},
        {"type": "quad", "pos": [-1, 0, -2], "u": [2, 0, 0], "v": [0, 0, -2], "material": _lam(0.2, 0.8, 0.2)},
        {"type": "quad", "pos": [-3, -3, -6], "u": [6, 0, 0], "v": [0, 6, 0], "material": _lam(0.7, 0.7, 0.7)},
        {"type": "sphere", "pos": [0.6, 0.5, -3], "r": 0.4, "material": _lam(0.3, 0.3, 0.9)},
    ]
    return {"camera": {"vfov": 60, "from": [0, 0, 0], "at": [0, 0, -1], "up": [0, 1, 0], "aperture": 0,
                       "background": _BG},
            "render": {"aspect": 1.0}, "objects": objects}


def decode(table):
    """uint64 records -> (mask, nearest slot, nearest bound, others' bound), bounds as float64."""
    t = np.asarray(table, np.uint64)
    mask = (t & np.uint64(0xffff)).astype(np.uint32)
    near = ((t >> np.uint64(16)) & np.uint64(15)).astype(np.int32)
    bn = ((t >> np.uint64(32)) & np.uint64(0xffff)).astype(np.uint16).view(np.float16).astype(np.float64)
    bo = ((t >> np.uint64(48)) & np.uint64(0xffff)).astype(np.uint16).view(np.float16).astype(np.float64)
    return mask, near, bn, bo


FOOTPRINT = [(a, b) for a in (-0.5, 0.0, 0.5) for b in (-0.5, 0.0, 0.5) if (a, b) != (0.0, 0.0)]  # corners, edge midpoints


def pixel_rays(oracle, sd, ro, i, j, info, n_samples=32):
    """Pixel (i, j)'s primary rays: samples 0..n-1 as Camera.getRay draws them, and the footprint's
    four corners and four edge midpoints. -> (origins, directions) float64 arrays."""
    o, d = [], []
    for n in range(n_samples):
        ro_, rd_ = oracle.get_ray(sd, ro, i, j, n)
        o.append(ro_)
        d.append(rd_)
    p00, du, dv, cen = (np.asarray(info[k], np.float64) for k in ("pixel00", "du", "dv", "center"))
    pc = p00 + du * i + dv * j
    for a, b in FOOTPRINT:
        o.append(cen)
        d.append(pc + a * du + b * dv - cen)
    return np.asarray(o, np.float64), np.asarray(d, np.float64)
