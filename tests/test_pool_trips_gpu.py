"""The pool kernel's trips (pt_pool.hpp pool_trips): a front stage (path start, diffuse
shading, or none for a specular continuation) followed by the common back stage that traces the
path's next ray. Every case renders on the pool kernel, on the chunked kernel of the same build
and on the oracle, with and without the primary-ray table, and compares u8, fp32 radiance bit
patterns and RenderStats exactly. The shapes are the smallest at which the control flow differs:
depth cut-offs and roulette right after a diffuse front, specular paths riding in diffuse trips
and drained alone, scenes without specular paths, without a light and with two, pools far below
one wave, partial tiles, tile-group shares, adaptive rounds and fp32."""
import copy

import numpy as np
import pytest

NOADAPT = {"aTolerance": 0}
_BG = {"type": "gradient", "top": [1, 1, 1], "bottom": [0.5, 0.7, 1.0]}


def _lam(r, g, b):
    return {"type": "lambert", "color": [r, g, b]}


_LIGHT2 = {"type": "quad", "pos": [-2.5, -0.5, -1], "u": [0, 0, -1], "v": [0, 1, 0], "light": True,
           "material": {"type": "light", "emit": [6, 5, 4]}}


def _custom(lights=1):
    """A fuzzy metal sphere, a glass sphere, a Lambertian sphere, three walls and `lights` light
    quads: at most 8 primitives, the pool kernel's LDS limit."""
    objects = [
        {"type": "quad", "pos": [-3, -1.5, -5], "u": [6, 0, 0], "v": [0, 4, 0], "material": _lam(0.73, 0.73, 0.73)},
        {"type": "quad", "pos": [-3, -1.5, 1], "u": [6, 0, 0], "v": [0, 0, -6], "material": _lam(0.6, 0.6, 0.2)},
        {"type": "quad", "pos": [3, -1.5, -5], "u": [0, 0, 6], "v": [0, 4, 0], "material": _lam(0.2, 0.6, 0.2)},
        {"type": "sphere", "pos": [-1.2, -0.7, -2.5], "r": 0.8,
         "material": {"type": "metal", "color": [0.8, 0.8, 0.8], "fuzz": 0.3}},
        {"type": "sphere", "pos": [0.9, -0.8, -1.8], "r": 0.7, "material": {"type": "glass", "ior": 1.5}},
        {"type": "sphere", "pos": [0.1, -1.1, -3.4], "r": 0.4, "material": _lam(0.8, 0.2, 0.2)},
    ]
    if lights >= 1:
        objects.append({"type": "quad", "pos": [-1, 2.4, -3.5], "u": [2, 0, 0], "v": [0, 0, 1.5], "light": True,
                        "material": {"type": "light", "emit": [12, 12, 12]}})
    if lights >= 2:
        objects.append(copy.deepcopy(_LIGHT2))
    assert len(objects) <= 8
    return {"camera": {"vfov": 70, "from": [0, 0, 1.5], "at": [0, -0.3, -2], "up": [0, 1, 0], "aperture": 0,
                       "background": _BG},
            "render": {"aspect": 1.0, "roulette": True, "rouletteDepth": 3},
            "objects": objects}


def _scene(rt, name):
    if name == "cornell":
        return rt.generate_scene_data({"type": "cornell"})
    if name == "cornell-rr1":  # roulette from the first bounce on
        sd = rt.generate_scene_data({"type": "cornell"})
        sd["render"] = {**sd.get("render", {}), "roulette": True, "rouletteDepth": 1}
        return sd
    if name == "cornell-empty":
        return rt.generate_scene_data({"type": "cornell", "options": {"variant": "empty"}})
    return _custom({"custom": 1, "custom-nolight": 0, "custom-2lights": 2}[name])


class Out:
    def __init__(self, cam, st, rgb, rad):
        self.cam, self.st, self.rgb, self.rad = cam, st, rgb, rad


def _render(rt, sd, ro, region=None):
    cam = rt.create_camera_from_scene_data(sd, ro)
    H, W = cam.image_height, cam.image_width
    rgb = np.zeros((H, W, 3), np.uint8)
    rad = np.zeros((H, W, 3), np.float32)
    st = cam.render_region(rgb, region or (0, 0, W, H), radiance=rad)
    return Out(cam, st, rgb, rad)


def _same(a, b, what):
    n_rgb = int((a.rgb != b.rgb).any(axis=-1).sum())
    n_rad = int((a.rad.view(np.uint32) != b.rad.view(np.uint32)).any(axis=-1).sum())
    print(f"{what}: pixels differing rgb {n_rgb}, radiance {n_rad} of {a.rgb[..., 0].size}")
    assert n_rgb == 0 and n_rad == 0, what
    assert a.st.pixels == b.st.pixels and a.st.samples == b.st.samples and a.st.bounces == b.st.bounces, what


def _same_as_oracle(a, orc, what):
    n_rgb = int((a.rgb != orc["rgb"]).any(axis=-1).sum())
    n_rad = int((a.rad.view(np.uint32) != orc["radiance"].view(np.uint32)).any(axis=-1).sum())
    print(f"{what} vs oracle: pixels differing rgb {n_rgb}, radiance {n_rad}")
    assert n_rgb == 0 and n_rad == 0, what
    assert a.st.pixels == orc["stats"]["pixels"], what
    for k in ("total", "min", "max"):
        assert a.st.samples[k] == orc["stats"]["samples"][k] and a.st.bounces[k] == orc["stats"]["bounces"][k], (what, k)


def _pool_and_chunked(rt, monkeypatch, sd, ro, table, region=None):
    """The render on the pool kernel (primary-ray table on / off) and on the chunked kernel."""
    monkeypatch.setenv("RT_AMD_PRIMARY_TABLE", table)
    pool = _render(rt, sd, ro, region)
    assert pool.cam.last_kernel() == "pool" and pool.cam.primary_info()["used"] == (table == "1")
    monkeypatch.setenv("RT_AMD_POOL_KERNEL", "0")
    chunked = _render(rt, sd, ro, region)
    monkeypatch.delenv("RT_AMD_POOL_KERNEL")
    monkeypatch.delenv("RT_AMD_PRIMARY_TABLE")
    assert chunked.cam.last_kernel() != "pool"
    return pool, chunked


# name: (scene, render options, region)
CASES = {
    # the depth cut-off inside a fused trip
    "cornell-16-depth1": ("cornell", {"width": 16, "samples": 4, "depth": 1, **NOADAPT}, None),
    "cornell-16-depth2": ("cornell", {"width": 16, "samples": 4, "depth": 2, **NOADAPT}, None),
    "cornell-16-depth3": ("cornell", {"width": 16, "samples": 4, "depth": 3, **NOADAPT}, None),
    # roulette right after the first diffuse bounce
    "cornell-16-roulette1": ("cornell-rr1", {"width": 16, "samples": 8, "depth": 8, **NOADAPT}, None),
    # specular paths riding in D trips, pure ac trips at the drain
    "cornell-40-spp8": ("cornell", {"width": 40, "samples": 8, "depth": 8, **NOADAPT}, None),
    "custom-24-spp16": ("custom", {"width": 24, "samples": 16, "depth": 8, **NOADAPT}, None),
    # no specular paths: ac stays empty
    "empty-24-spp8": ("cornell-empty", {"width": 24, "samples": 8, "depth": 8, **NOADAPT}, None),
    # no light: dl is never used, the light-PDF loop is empty; two lights
    "nolight-24-spp16": ("custom-nolight", {"width": 24, "samples": 16, "depth": 8, **NOADAPT}, None),
    "2lights-24-spp16": ("custom-2lights", {"width": 24, "samples": 16, "depth": 8, **NOADAPT}, None),
    # nearly empty pools: stacks far below 64, a 1-sample item in every slot
    "cornell-8-spp1": ("cornell", {"width": 8, "samples": 1, "depth": 8, **NOADAPT}, None),
    "cornell-8-spp3": ("cornell", {"width": 8, "samples": 3, "depth": 8, **NOADAPT}, None),
    # a region not aligned to the 8x8 tiles
    "region": ("cornell", {"width": 40, "samples": 8, "depth": 8, **NOADAPT}, (3, 5, 17, 11)),
    # adaptive rounds on the pool kernel (the reference's adaptive defaults), error flags in the records
    "adaptive-defaults": ("cornell", {"width": 32}, None),
}

_oracle_cache = {}


def _oracle(oracle, rt, case):
    """The oracle's render of a case, computed once for both table settings."""
    if case not in _oracle_cache:
        scene, ro, region = CASES[case]
        _oracle_cache[case] = oracle.render(_scene(rt, scene), ro, region=region)
    return _oracle_cache[case]


@pytest.mark.gpu
@pytest.mark.parametrize("table", ["1", "0"])
@pytest.mark.parametrize("case", list(CASES))
def test_pool_equals_chunked_equals_oracle(rt, oracle, gpu, monkeypatch, case, table):
    scene, ro, region = CASES[case]
    sd = _scene(rt, scene)
    pool, chunked = _pool_and_chunked(rt, monkeypatch, sd, ro, table, region)
    _same(pool, chunked, f"{case} table {table}: pool == chunked")
    _same_as_oracle(pool, _oracle(oracle, rt, case), f"{case} table {table}")
    if case == "adaptive-defaults":
        assert pool.cam.adaptive_info()[0] >= 1  # adaptive rounds ran


@pytest.mark.gpu
@pytest.mark.parametrize("table", ["1", "0"])
def test_tile_group_shares_sum_to_the_oracle(rt, oracle, gpu, monkeypatch, table):
    import torch
    sd = _scene(rt, "cornell")
    ro = {"width": 40, "samples": 8, "depth": 8, **NOADAPT}
    shares = {}
    for kernel in ("pool", "chunked"):
        monkeypatch.setenv("RT_AMD_PRIMARY_TABLE", table)
        monkeypatch.setenv("RT_AMD_POOL_KERNEL", "1" if kernel == "pool" else "0")
        cam = rt.create_camera_from_scene_data(sd, ro)
        H, W = cam.image_height, cam.image_width
        parts = []
        for g in range(3):
            rgb = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
            rad = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
            st, _ = cam.render_device(rgb_ptr=rgb.data_ptr(), radiance_ptr=rad.data_ptr(), tile_group=g,
                                      tile_groups=3, synchronize=True)
            assert (cam.last_kernel() == "pool") == (kernel == "pool")
            parts.append((rgb.cpu().numpy(), rad.cpu().numpy(), (st.pixels, st.samples, st.bounces)))
        shares[kernel] = parts
    monkeypatch.delenv("RT_AMD_POOL_KERNEL")
    monkeypatch.delenv("RT_AMD_PRIMARY_TABLE")
    for g in range(3):
        p, c = shares["pool"][g], shares["chunked"][g]
        assert np.array_equal(p[0], c[0]) and np.array_equal(p[1].view(np.uint32), c[1].view(np.uint32)), g
        assert p[2] == c[2], g
    orc = _oracle(oracle, rt, "cornell-40-spp8")
    rgb = sum(p[0].astype(np.int32) for p in shares["pool"])  # the shares are disjoint
    rad = sum(p[1] for p in shares["pool"])
    assert np.array_equal(rgb, orc["rgb"])
    assert np.array_equal(rad.view(np.uint32), orc["radiance"].view(np.uint32))
    assert sum(p[2][0] for p in shares["pool"]) == orc["stats"]["pixels"]
    assert sum(p[2][1]["total"] for p in shares["pool"]) == orc["stats"]["samples"]["total"]
    assert sum(p[2][2]["total"] for p in shares["pool"]) == orc["stats"]["bounces"]["total"]


@pytest.mark.gpu
@pytest.mark.parametrize("table", ["1", "0"])
def test_fp32_pool_equals_chunked(rt, gpu, monkeypatch, table):
    sd = _scene(rt, "cornell")
    ro = {"width": 40, "samples": 8, "depth": 8, "precision": "fp32", **NOADAPT}
    pool, chunked = _pool_and_chunked(rt, monkeypatch, sd, ro, table)
    _same(pool, chunked, f"fp32 table {table}: pool == chunked")
