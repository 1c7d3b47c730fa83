"""GPU parity: the HIP path tracer against the CPU oracle (same seeds).

Contract: in ref precision the GPU restates the reference's
arithmetic (fp64 scalars, fp32 vector stores, no FMA) and the oracle's
transcendental choices, so images must agree bit-for-bit: every pixel's u8
value and fp32 radiance, and the RenderStats. fp32 precision is checked
against the same ref oracle with SURVEY.md §8c's tolerance (>= 99 % of pixels
within 1e-3 + 1e-3|c|, image-mean relative difference <= 1e-3 at spp >= 64).
"""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NOADAPT = {"aTolerance": 0}


def _cfgs():
    return {
        "cornell": ({"type": "cornell"}, {"width": 48, "samples": 16, "depth": 16, **NOADAPT}),
        "spheres": ({"type": "spheres", "options": {"count": 500, "seed": 42}},
                    {"width": 48, "aspect": 1, "samples": 8, "depth": 8, **NOADAPT}),
        "rain": ({"type": "rain", "options": {"seed": 42}}, {"width": 64, "samples": 8, "depth": 16, **NOADAPT}),
        "default": ({"type": "default"}, {"width": 48, "samples": 8, "depth": 12, **NOADAPT}),
    }


def _mixed_scene():
    """custom SceneData with mixed (emissive component) + layered materials."""
    return {
        "camera": {"vfov": 50, "from": [0, 1, 3], "at": [0, 0.3, 0], "up": [0, 1, 0], "aperture": 0.0, "focus": 0,
                   "background": {"type": "gradient", "top": [0.6, 0.7, 1.0], "bottom": [1, 1, 1]}},
        "render": {"aspect": 1.5},
        "materials": [
            {"id": "glow", "material": {"type": "light", "emit": [4, 3, 2]}},
            {"id": "red", "material": {"type": "lambert", "color": [0.8, 0.2, 0.2]}},
            {"id": "mix", "material": {"type": "mixed", "diff": "red", "spec": "glow", "weight": 0.7}},
            {"id": "mixm", "material": {"type": "mixed", "diff": {"type": "metal", "color": [0.9, 0.9, 0.9],
                                                                   "fuzz": 0.2},
                                        "spec": {"type": "glass", "ior": 1.4}, "weight": 0.5}},
            {"id": "coat", "material": {"type": "layered", "outer": {"type": "glass", "ior": 1.5},
                                        "inner": {"type": "metal", "color": [0.8, 0.6, 0.3], "fuzz": 0.1}}},
        ],
        "objects": [
            {"type": "plane", "pos": [0, 0, 0], "u": [1, 0, 0], "v": [0, 0, -1], "material": "red"},
            {"type": "sphere", "pos": [-0.8, 0.5, 0], "r": 0.5, "material": "mix"},
            {"type": "sphere", "pos": [0.4, 0.4, 0.3], "r": 0.4, "material": "mixm"},
            {"type": "sphere", "pos": [1.0, 0.35, -0.6], "r": 0.35, "material": "coat"},
            {"type": "quad", "pos": [-1, 2, -1], "u": [2, 0, 0], "v": [0, 0, 1], "material": "glow", "light": True},
        ],
    }


def _render_gpu(rt, scene_data, ropts, precision="ref", region=None):
    cam = rt.create_camera_from_scene_data(scene_data, {**ropts, "precision": precision})
    W, H = cam.image_width, cam.image_height
    rgb = np.zeros((H, W, 3), np.uint8)
    rad = np.zeros((H, W, 3), np.float32)
    st = cam.render_region(rgb, region or (0, 0, W, H), radiance=rad)
    return cam, rgb, rad, st


def _diff(a_rad, a_rgb, b_rad, b_rgb):
    """(pixels whose u8 differs, pixels whose fp32 radiance differs, max |d|)."""
    n_rgb = int((a_rgb != b_rgb).any(axis=-1).sum())
    same = (a_rad == b_rad) | (np.isnan(a_rad) & np.isnan(b_rad))
    n_rad = int((~same).any(axis=-1).sum())
    d = np.abs(a_rad.astype(np.float64) - b_rad)
    return n_rgb, n_rad, float(np.nanmax(d)) if d.size else 0.0


def assert_identical(a_rad, a_rgb, b_rad, b_rgb, what=""):
    n_rgb, n_rad, maxd = _diff(a_rad, a_rgb, b_rad, b_rgb)
    print(f"{what}: pixels differing rgb {n_rgb}, radiance {n_rad} (max |d| {maxd:.3g}) of {a_rgb[..., 0].size}")
    assert n_rgb == 0 and n_rad == 0, (what, n_rgb, n_rad, maxd)


def assert_stats_identical(st, orc_stats):
    assert st.pixels == orc_stats["pixels"]
    for k in ("total", "min", "max"):
        assert st.samples[k] == orc_stats["samples"][k], ("samples", k)
        assert st.bounces[k] == orc_stats["bounces"][k], ("bounces", k)


@pytest.mark.parametrize("name", ["cornell", "spheres", "rain", "default"])
def test_ref_precision_matches_oracle(rt, oracle, gpu, name):
    cfg, ro = _cfgs()[name]
    sd = rt.generate_scene_data(cfg)
    cam, rgb, rad, st = _render_gpu(rt, sd, ro)
    orc = oracle.render(sd, ro)
    assert_identical(rad, rgb, orc["radiance"], orc["rgb"], name)
    assert_stats_identical(st, orc["stats"])


def test_custom_mixed_layered_emissive_matches_oracle(rt, oracle, gpu):
    sd = _mixed_scene()
    ro = {"width": 48, "samples": 8, "depth": 10, **NOADAPT}
    cam, rgb, rad, st = _render_gpu(rt, sd, ro)
    assert cam.info["n_lights"] == 1
    orc = oracle.render(sd, ro)
    assert_identical(rad, rgb, orc["radiance"], orc["rgb"], "mixed")
    assert_stats_identical(st, orc["stats"])


def test_adaptive_sampling_matches_oracle(rt, oracle, gpu):
    """Default RenderOptions: adaptive sampling on (aTolerance 0.05, aBatch 10)."""
    sd = rt.generate_scene_data({"type": "cornell"})
    ro = {"width": 40, "samples": 60, "depth": 8}
    cam, rgb, rad, st = _render_gpu(rt, sd, ro)
    orc = oracle.render(sd, ro)
    assert_identical(rad, rgb, orc["radiance"], orc["rgb"], "adaptive")
    assert st.samples["min"] < 60  # some pixels converged early
    assert_stats_identical(st, orc["stats"])


@pytest.mark.parametrize("mode", ["bounces", "samples"])
def test_render_modes(rt, oracle, gpu, mode):
    sd = rt.generate_scene_data({"type": "cornell"})
    ro = {"width": 32, "samples": 20, "depth": 8, "mode": mode}
    cam, rgb, rad, st = _render_gpu(rt, sd, ro)
    orc = oracle.render(sd, ro)
    assert_identical(rad, rgb, orc["radiance"], orc["rgb"], mode)
    assert_stats_identical(st, orc["stats"])
    if mode == "bounces":
        assert np.all(rad[..., :2] == 0)
    else:
        assert np.all(rad[..., 1:] == 0)


def test_region_writes_only_region(rt, gpu):
    sd = rt.generate_scene_data({"type": "cornell"})
    ro = {"width": 40, "samples": 4, "depth": 6, **NOADAPT}
    cam = rt.create_camera_from_scene_data(sd, ro)
    full = np.zeros((40, 40, 3), np.uint8)
    cam.render(full)
    part = np.full((40, 40, 3), 7, np.uint8)
    st = cam.render_region(part, {"x": 5, "y": 9, "width": 13, "height": 50})
    assert st.pixels == 13 * 31
    assert np.array_equal(part[9:40, 5:18], full[9:40, 5:18])
    mask = np.ones((40, 40), bool)
    mask[9:40, 5:18] = False
    assert np.all(part[mask] == 7)


def test_tile_groups_partition_the_image(rt, gpu):
    """Multi-GPU interleave: the union of tile groups equals the single render."""
    import ctypes
    import torch
    sd = rt.generate_scene_data({"type": "rain", "options": {"seed": 42}})
    ro = {"width": 72, "samples": 4, "depth": 8, **NOADAPT}
    cam = rt.create_camera_from_scene_data(sd, ro)
    W, H = cam.image_width, cam.image_height
    full = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    cam.render_device(rgb_ptr=full.data_ptr(), synchronize=True)
    acc = torch.zeros_like(full)
    total = 0
    for g in range(3):
        part = torch.zeros_like(full)
        st, _ = cam.render_device(rgb_ptr=part.data_ptr(), tile_group=g, tile_groups=3, synchronize=True)
        total += st.pixels
        acc += part
    torch.cuda.synchronize()
    assert total == W * H
    assert torch.equal(acc, full)
    # the kernel's tile walk is exactly raytracer_amd.distributed.owner_mask
    from raytracer_amd.distributed import owner_mask
    for g in range(3):
        pxs = torch.full((H, W), -1, dtype=torch.int32, device="cuda")
        part = torch.zeros_like(full)
        cam.render_device(rgb_ptr=part.data_ptr(), px_samples_ptr=pxs.data_ptr(), tile_group=g, tile_groups=3,
                          synchronize=True)
        written = (pxs >= 0).cpu().numpy()
        assert np.array_equal(written, owner_mask(W, H, (0, 0, W, H), g, 3))


def test_fp32_precision_within_tolerance(rt, oracle, gpu):
    """fp32 mode against the ref oracle on the headline scene, SURVEY.md §8c's
    contract: >= 99 % of pixels within |d| <= 1e-3 + 1e-3|c| (every channel),
    image-mean |d|/mean <= 1e-3 at spp >= 64, u8 within 1 LSB on >= 99 %."""
    sd = rt.generate_scene_data({"type": "cornell"})
    ro = {"width": 48, "samples": 64, "depth": 16, **NOADAPT}
    _, rgb, rad, _ = _render_gpu(rt, sd, ro, precision="fp32")
    orc = oracle.render(sd, ro)
    d = np.abs(rad.astype(np.float64) - orc["radiance"])
    tol = 1e-3 + 1e-3 * np.abs(orc["radiance"])
    within = (d <= tol).all(axis=-1)
    frac = float(within.mean())
    mean_rel = float(abs(rad.astype(np.float64).mean() - orc["radiance"].mean()) / orc["radiance"].mean())
    lsb = float((np.abs(rgb.astype(int) - orc["rgb"]) <= 1).all(axis=-1).mean())
    print(f"fp32 cornell: {int((~within).sum())} of {within.size} pixels outside tol ({frac:.4f} within), "
          f"image-mean rel diff {mean_rel:.2e}, u8 within 1 LSB {lsb:.4f}, max |d| {d.max():.3g}")
    assert frac >= 0.99
    assert mean_rel <= 1e-3
    assert lsb >= 0.99


def test_fp32_precision_statistical_on_rejection_sampling_scene(rt, oracle, gpu):
    """spheres-500 (fuzzy metal, glass): fp32 arithmetic moves the rejection-sampling,
    Schlick and roulette comparisons, so a path can take another branch and the
    pixel decorrelates like a re-seeded one - the per-pixel contract above does not
    apply (20 % of pixels leave it at spp 64). What must hold: the image mean within
    1e-3 relative, and the per-pixel difference to the ref oracle no larger than the
    ref renderer's own seed-to-seed difference (95th and 99th percentiles)."""
    sd = rt.generate_scene_data({"type": "spheres", "options": {"count": 500, "seed": 42}})
    ro = {"width": 48, "aspect": 1, "samples": 64, "depth": 8, **NOADAPT}
    _, rgb, rad, _ = _render_gpu(rt, sd, ro, precision="fp32")
    orc = oracle.render(sd, ro)
    orc2 = oracle.render(sd, {**ro, "seed": 12345})
    d = np.abs(rad.astype(np.float64) - orc["radiance"]).max(axis=-1)
    noise = np.abs(orc2["radiance"].astype(np.float64) - orc["radiance"]).max(axis=-1)
    mean_rel = float(abs(rad.astype(np.float64).mean() - orc["radiance"].mean()) / orc["radiance"].mean())
    q = {p: (float(np.percentile(d, p)), float(np.percentile(noise, p))) for p in (95, 99)}
    print(f"fp32 spheres: image-mean rel diff {mean_rel:.2e}, |d| p95/p99 {q[95][0]:.3g}/{q[99][0]:.3g} vs "
          f"seed-to-seed {q[95][1]:.3g}/{q[99][1]:.3g}")
    assert mean_rel <= 1e-3
    for p, (a, b) in q.items():
        assert a <= b, (p, a, b)


def test_work_counters_match_oracle(rt, oracle, gpu):
    import torch
    sd = rt.generate_scene_data({"type": "cornell"})
    ro = {"width": 32, "samples": 8, "depth": 16, **NOADAPT}
    # reference-order traversal: the same node / primitive tests as the reference
    cam = rt.create_camera_from_scene_data(sd, {**ro, "traversal": "reference"})
    buf = torch.zeros((32, 32, 3), dtype=torch.uint8, device="cuda")
    st, cnt = cam.render_device(rgb_ptr=buf.data_ptr(), synchronize=True, count_work=True)
    orc = oracle.render(sd, ro, counters=True)["counters"]
    for k in ["samples", "rays", "node", "sphere", "quad", "material", "light_quad", "bounces", "diffuse"]:
        assert abs(cnt[k] - orc[k]) <= 0.01 * orc[k] + 2, (k, cnt[k], orc[k])


def test_work_counters_adaptive_count_the_references_samples(rt, oracle, gpu):
    """with adaptive sampling on, an instrumented launch runs the sequential kernel
    (adaptive rounds would render - and count - samples past each pixel's convergence), so the
    counters are the work of exactly the reference's samples."""
    import torch
    sd = rt.generate_scene_data({"type": "cornell"})
    ro = {"width": 32, "samples": 60, "depth": 16, "aTolerance": 0.05, "aBatch": 10}
    cam = rt.create_camera_from_scene_data(sd, {**ro, "traversal": "reference"})
    buf = torch.zeros((32, 32, 3), dtype=torch.uint8, device="cuda")
    st, cnt = cam.render_device(rgb_ptr=buf.data_ptr(), synchronize=True, count_work=True)
    assert cam.last_kernel() == "sequential"
    orc = oracle.render(sd, ro, counters=True)
    assert st.samples["total"] == orc["stats"]["samples"]["total"] < 32 * 32 * 60  # some pixels converged
    assert cnt["samples"] == orc["counters"]["samples"]
    for k in ["rays", "node", "sphere", "quad", "material", "light_quad", "bounces", "diffuse"]:
        assert abs(cnt[k] - orc["counters"][k]) <= 0.01 * orc["counters"][k] + 2, (k, cnt[k], orc["counters"][k])


def test_world_hit_matches_oracle(rt, oracle, gpu):
    rng = np.random.default_rng(7)
    for cfg in [{"type": "spheres", "options": {"count": 200, "seed": 3}}, {"type": "cornell"}, {"type": "default"}]:
        sd = rt.generate_scene_data(cfg)
        cam = rt.create_camera_from_scene_data(sd, {"width": 8})
        n = 4000
        o = rng.uniform(-1.5, 1.5, (n, 3)).astype(np.float32) + np.float32([0, 0.5, 0])
        d = rng.normal(size=(n, 3)).astype(np.float32)
        d[: n // 8, rng.integers(0, 3)] = 0  # axis-parallel rays: 1/0 in the slab tests
        c = oracle.world_hit(sd, o, d)
        po = cam.export()["prim_object"]
        for trav in ["reference", "fast", "brute"]:
            g = cam.debug_world_hit(o, d, traversal=trav)
            assert np.array_equal(g[:, 0], c[:, 0]), trav
            h = g[:, 0] > 0
            assert np.array_equal(g[h, 1], c[h, 1]), trav
            assert np.array_equal(g[h, 2:9], c[h, 2:9]), trav
            # prim slot -> SceneData object index
            assert np.array_equal(po[g[h, 9].astype(int)], c[h, 9].astype(int)), trav


@pytest.mark.parametrize("name", ["cornell", "spheres", "rain", "default"])
def test_fast_traversal_equals_reference_traversal(rt, gpu, name, monkeypatch):
    """Larger images than the oracle can render quickly: the fast (with and
    without deferred exact tests) and the brute-force closest hit must reproduce
    the reference-order traversal bit-for-bit."""
    cfg, ro = _cfgs()[name]
    sd = rt.generate_scene_data(cfg)
    ro = {**ro, "width": 192, "samples": 16}
    outs = []
    for trav, defer in [("reference", "0"), ("fast", "0"), ("brute", "0"), ("fast", "1")]:
        monkeypatch.setenv("RT_AMD_DEFER", defer)
        cam, rgb, rad, st = _render_gpu(rt, sd, {**ro, "traversal": trav})
        outs.append((rgb, rad, st))
    for k in (1, 2, 3):
        assert np.array_equal(outs[0][0], outs[k][0])
        assert np.array_equal(outs[0][1], outs[k][1], equal_nan=True)
        assert outs[0][2].bounces == outs[k][2].bounces


def test_missing_background_raises_like_reference(rt, gpu):
    sd = rt.generate_scene_data({"type": "cornell"})
    del sd["camera"]["background"]
    cam = rt.create_camera_from_scene_data(sd, {"width": 16, "samples": 2, "depth": 4, **NOADAPT})
    with pytest.raises(rt.RtError, match="reading 'top'"):
        cam.render(np.zeros((16, 16, 3), np.uint8))
    # a scene whose rays all hit never reads the background (the reference is lazy too)
    sd2 = rt.generate_scene_data({"type": "cornell"})
    sd2["camera"]["background"] = None
    sd2["camera"]["vfov"] = 10
    cam2 = rt.create_camera_from_scene_data(sd2, {"width": 8, "samples": 1, "depth": 1, **NOADAPT})
    cam2.render(np.zeros((8, 8, 3), np.uint8))


def _slit_box(gap):
    """A closed box [-1, 1]^3 around the camera with an emissive ceiling and a slit of width
    `gap` along one edge of the wall behind the camera, no background: a path misses (and
    the reference throws "reading 'top'") only when it leaves through the slit."""
    return {
        "camera": {"vfov": 60, "from": [0, 0, 0.5], "at": [0, 0, -1], "up": [0, 1, 0], "aperture": 0.0, "focus": 0},
        "render": {"aspect": 1},
        "materials": [
            {"id": "white", "material": {"type": "lambert", "color": [0.73, 0.73, 0.73]}},
            {"id": "red", "material": {"type": "lambert", "color": [0.65, 0.05, 0.05]}},
            {"id": "lamp", "material": {"type": "light", "emit": [1, 1, 1]}},
        ],
        "objects": [
            {"type": "quad", "pos": [-1, -1, -1], "u": [2, 0, 0], "v": [0, 2, 0], "material": "white"},
            {"type": "quad", "pos": [-1, -1, 1], "u": [2 - gap, 0, 0], "v": [0, 2, 0], "material": "white"},
            {"type": "quad", "pos": [-1, -1, -1], "u": [0, 0, 2], "v": [0, 2, 0], "material": "red"},
            {"type": "quad", "pos": [1, -1, -1], "u": [0, 0, 2], "v": [0, 2, 0], "material": "white"},
            {"type": "quad", "pos": [-1, -1, -1], "u": [2, 0, 0], "v": [0, 0, 2], "material": "white"},
            {"type": "quad", "pos": [-1, 1, -1], "u": [2, 0, 0], "v": [0, 0, 2], "material": "lamp", "light": True},
        ],
    }


@pytest.mark.parametrize("path", ["pool", "chunked", "fast"])
def test_adaptive_rounds_ignore_misses_past_convergence(rt, oracle, gpu, path, monkeypatch):
    """adaptive rounds render samples past a pixel's convergence, which the
    reference's loop never renders (src/camera.ts:400-425). A miss among THOSE samples must
    not raise. Premise, checked with the oracle: pixel (0, 0) of the slit box (seed 1,
    aTolerance 0.3) converges after 60 samples without a miss, while its samples 0..199 do
    miss (first at index 71) - and the rounds of a one-pixel region, [0, 10), [10, 40),
    [40, 130), render sample 71 inside the round in which the pixel converges."""
    sd = _slit_box(0.05)
    ro = {"width": 16, "samples": 200, "depth": 16, "aTolerance": 0.3, "aBatch": 10, "seed": 1}
    if path == "fast":
        ro["traversal"] = "fast"
    if path == "chunked":
        monkeypatch.setenv("RT_AMD_POOL_KERNEL", "0")
    region = (0, 0, 1, 1)
    orc = oracle.render(sd, ro, region=region)
    assert int(orc["px_samples"][0, 0]) == 60
    with pytest.raises(Exception, match="reading 'top'"):
        oracle.render(sd, {**ro, "aTolerance": 0}, region=region)
    oracle.render(sd, {**ro, "aTolerance": 0, "samples": 71}, region=region)  # samples 0..70 hit
    with pytest.raises(Exception, match="reading 'top'"):
        oracle.render(sd, {**ro, "aTolerance": 0, "samples": 72}, region=region)
    cam, rgb, rad, st = _render_gpu(rt, sd, ro, region=region)
    assert cam.last_kernel() == ("chunked" if path != "pool" else "pool")
    rounds, rendered = cam.adaptive_info()
    # round 1 retires none of the region's one pixel, so the round-length rule takes the rest:
    # [0, 10), [10, 200) - the round in which the pixel converges rendered sample 71 (a miss)
    assert rounds == 2 and rendered == 200
    # without the rule (RT_AMD_ADAPT_JUMP=0: rounds grow x3) [0, 10), [10, 40), [40, 130): the
    # third round renders sample 71 past the convergence at 60
    monkeypatch.setenv("RT_AMD_ADAPT_JUMP", "0")
    cam3, rgb3, rad3, st3 = _render_gpu(rt, sd, ro, region=region)
    assert cam3.adaptive_info() == (3, 130)  # 10 + 30 + 90 samples of the one pixel
    assert_identical(rad3[:1, :1], rgb3[:1, :1], orc["radiance"][:1, :1], orc["rgb"][:1, :1], f"slit box {path} x3")
    assert_stats_identical(st3, orc["stats"])
    monkeypatch.delenv("RT_AMD_ADAPT_JUMP")
    assert_identical(rad[:1, :1], rgb[:1, :1], orc["radiance"][:1, :1], orc["rgb"][:1, :1], f"slit box {path}")
    assert_stats_identical(st, orc["stats"])
    # fixed spp renders sample 71 for real: the reference's error
    cam2 = rt.create_camera_from_scene_data(sd, {**ro, "aTolerance": 0})
    with pytest.raises(rt.RtError, match="reading 'top'"):
        cam2.render_region(np.zeros((16, 16, 3), np.uint8), region)


def test_generate_image_buffer_png(rt, gpu):
    from raytracer_amd.png import decode_png_rgb
    png, st = rt.generate_image_buffer({"type": "cornell", "render": {"width": 24, "samples": 4, "depth": 4}},
                                       return_stats=True)
    w, h, px = decode_png_rgb(png)
    assert (w, h) == (24, 24) and len(px) == 24 * 24 * 3
    png2 = rt.generate_image_buffer({"type": "cornell", "render": {"width": 24, "samples": 4, "depth": 4}},
                                    {"parallel": True, "threads": 5})
    assert png2 == png  # the band split never changes pixels (RNG keyed by pixel/sample)


def _hit_equal(rt, oracle, sd, o, d, travs=("reference", "fast", "brute")):
    """world_hit under every strategy vs the oracle: hit flag, t, p, n, front, object."""
    cam = rt.create_camera_from_scene_data(sd, {"width": 8})
    c = oracle.world_hit(sd, o, d)
    po = cam.export()["prim_object"]
    for trav in travs:
        g = cam.debug_world_hit(o, d, traversal=trav)
        assert np.array_equal(g[:, 0], c[:, 0]), trav
        h = g[:, 0] > 0
        assert np.array_equal(g[h, 1], c[h, 1]), trav
        assert np.array_equal(g[h, 2:9], c[h, 2:9]), trav
        assert np.array_equal(po[g[h, 9].astype(int)], c[h, 9].astype(int)), trav
    return c


@pytest.mark.parametrize("spheres", [
    [((0, 0, -1), 0.5), ((-1, 0, -1), 0.5), ((1, 0, -1), 0.5), ((0, -100.5, -1), 100)],  # bvh.test.ts:15-20
    [((i - 5, 0, -5), 0.3) for i in range(10)],  # bvh.test.ts:23-28 (leaf)
    [((0, 0, -3), 0.5), ((0, 0, -1), 0.5)],  # hittableList.test.ts:49-50, far sphere added first
], ids=["bvh4", "bvh_leaf", "list2"])
def test_reference_bvh_and_list_scenes(rt, oracle, gpu, spheres):
    """The reference's BVH / HittableList test worlds through the product's
    world_hit (every traversal) vs the oracle, on the tests' rays plus a fan."""
    sd = {"camera": {"vfov": 90, "from": [0, 0, 0], "at": [0, 0, -1], "up": [0, 1, 0],
                     "background": {"type": "gradient", "top": [1, 1, 1], "bottom": [0.5, 0.7, 1]}},
          "objects": [{"type": "sphere", "pos": list(c), "r": r,
                       "material": {"type": "lambert", "color": [0.8, 0.8, 0.8]}} for c, r in spheres]}
    rng = np.random.default_rng(3)
    d = np.concatenate([np.float32([[0, 0, -1], [0, 1, 0], [0.408248, -0.408248, -0.816497]]),
                        rng.normal(size=(509, 3)).astype(np.float32)])
    o = np.zeros_like(d)
    o[1] = (0, 5, 0)
    c = _hit_equal(rt, oracle, sd, o, d)
    assert c[0, 0] > 0 and c[1, 0] == 0


def test_axis_quad_edges_and_corners(rt, oracle, gpu):
    """Cornell walls are axis-aligned quads (aquad_t): rays aimed exactly at
    edges, corners and just outside them must decide alpha/beta like the
    reference's general formula."""
    sd = rt.generate_scene_data({"type": "cornell"})
    rng = np.random.default_rng(11)
    targets = []
    for obj in sd["objects"]:
        if obj["type"] != "quad":
            continue
        q, u, v = (np.array(obj[k], np.float64) for k in ("pos", "u", "v"))
        for a in (0.0, 1.0, 0.5, 1e-7, 1 - 1e-7, -1e-7, 1 + 1e-7):
            for b in (0.0, 1.0, 0.25, -1e-7, 1 + 1e-7):
                targets.append(q + a * u + b * v)
    targets = np.array(targets)
    n = len(targets)
    o = rng.uniform(50, 500, (n, 3))
    d = (targets - o).astype(np.float32)
    c = _hit_equal(rt, oracle, sd, o.astype(np.float32), d)
    assert (c[:, 0] > 0).mean() > 0.5


def _pair_scene():
    """16 primitives for the brute-force pre-filter's records (scene_blob.cpp prefilter_records):
    axis-aligned quads of all six axis codes (u / v swapped gives the second code of an axis),
    three of one code (a pair and a single), two of another on the same plane, five spheres (two
    pairs and a single, one of them a light), a tilted quad and a plane (single records that
    read the RtPrim)."""
    m = {"type": "lambert", "color": [0.7, 0.6, 0.5]}
    quads = [
        ((-1.5, -1, -1), (0, 2, 0), (0, 0, 2)), ((1.5, -1, 1), (0, 2, 0), (0, 0, -2)),       # x, one code
        ((0.2, -0.5, -0.5), (0, 0, 1), (0, 1, 0)),                                            # x, swapped
        ((-1.5, -1, -1), (3, 0, 0), (0, 0, 2)), ((-1.5, 1.2, 1), (3, 0, 0), (0, 0, -2)),      # y
        ((-0.3, 0.99, -0.3), (0.6, 0, 0), (0, 0, 0.6)),                                       # y, same code: 3rd
        ((-1.5, -1, -1.2), (3, 0, 0), (0, 2.2, 0)), ((-1.5, -1, -1.2), (0, 2.2, 0), (3, 0, 0)),  # z, both codes
        ((-1.0, -0.2, 0.4), (0.5, 0, 0), (0, 0.5, 0)),                                        # z, 2nd of a code
    ]
    objs = [{"type": "quad", "pos": list(q), "u": list(u), "v": list(v), "material": m} for q, u, v in quads]
    objs[5]["light"] = True
    objs[5]["material"] = {"type": "light", "emit": [8, 8, 8]}
    for k, (c, r) in enumerate([((-0.6, -0.6, -0.3), 0.35), ((0.6, -0.7, 0.2), 0.3), ((0.0, 0.3, -0.6), 0.25),
                                ((0.9, 0.5, 0.5), 0.2), ((-0.9, 0.6, 0.6), 0.15)]):
        mat = {"type": "glass", "ior": 1.5} if k == 1 else m
        objs.append({"type": "sphere", "pos": list(c), "r": r, "material": mat})
    objs.append({"type": "quad", "pos": [0.3, -0.8, -0.9], "u": [0.4, 0.3, 0.1], "v": [-0.1, 0.2, 0.5],
                 "material": m})
    objs.append({"type": "plane", "pos": [0, -1.05, 0], "u": [1, 0, 0], "v": [0, 0, -1], "material": m})
    return {"camera": {"vfov": 60, "from": [0, 0, 3.5], "at": [0, 0, 0], "up": [0, 1, 0],
                       "background": {"type": "gradient", "top": [0.5, 0.7, 1.0], "bottom": [1, 1, 1]}},
            "objects": objs}


def test_prefilter_pair_records_match_oracle(rt, oracle, gpu):
    """The brute-force pass evaluates spheres and same-code axis quads two at a time (packed
    fp32). Hits from inside and outside the box, rays leaving the walls and spheres (self-hit
    rejection), near-parallel rays and window edges, then a rendered image, against the oracle."""
    sd = _pair_scene()
    assert len(sd["objects"]) == 16
    rng = np.random.default_rng(21)
    n = 6000
    o = rng.uniform(-1.4, 1.4, (n, 3))
    o[: n // 4] = rng.uniform(-60, 60, (n // 4, 3))
    d = rng.normal(size=(n, 3))
    # rays starting on the walls x = -1.5 / y = -1 / z = -1.2 and on a sphere, leaving them
    k = n // 8
    o[k:2 * k, 0] = -1.5
    d[k:2 * k, 0] = np.abs(d[k:2 * k, 0])
    o[2 * k:3 * k, 1] = -1.0
    o[3 * k:4 * k, 2] = -1.2
    u = rng.normal(size=(k, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    o[4 * k:5 * k] = np.float64([-0.6, -0.6, -0.3]) + 0.35 * u
    # near-parallel to the y planes, and aimed at quad edges
    d[5 * k:6 * k, 1] = d[5 * k:6 * k, 1] * 1e-4
    o = o.astype(np.float32)
    d = d.astype(np.float32)
    c = _hit_equal(rt, oracle, sd, o, d)
    assert (c[:, 0] > 0).mean() > 0.5
    ro = {"width": 48, "samples": 8, "depth": 10, **NOADAPT}
    orc = oracle.render(sd, ro)
    for prec_trav in ("brute", "auto"):
        _, rgb, rad, st = _render_gpu(rt, sd, {**ro, "traversal": prec_trav})
        assert_identical(rad, rgb, orc["radiance"], orc["rgb"], f"pair scene {prec_trav}")
        assert_stats_identical(st, orc["stats"])


@pytest.mark.parametrize("cfg", [{"type": "cornell"}, {"type": "spheres", "options": {"count": 500, "seed": 42}},
                                 {"type": "spheres", "options": {"count": 6000, "seed": 9}}],
                         ids=["cornell", "spheres500", "spheres6000"])
def test_near_parallel_rays_match_oracle(rt, oracle, gpu, cfg):
    """make_fray leaves an axis with 0 < |d_a| < 1e-3 max|d| out of the slab test's
    absolute slack (pt_walk.hpp make_fray): rays whose components are +-1e-4, 1e-6 and 1e-9
    times max|d| on one or two axes, from origins at |o| = 10 .. 1e4 aimed at the scene, through
    the fast walk (and brute force) against the reference-order traversal and the oracle."""
    sd = rt.generate_scene_data(cfg)
    rng = np.random.default_rng(17)
    n = 3000
    centre = np.float64([278, 278, 278]) if cfg["type"] == "cornell" else np.float64([0, 1, 0])
    rad = 10.0 ** rng.uniform(1, 4, n)
    dirn = rng.normal(size=(n, 3))
    dirn /= np.linalg.norm(dirn, axis=1, keepdims=True)
    o = centre + rad[:, None] * dirn
    d = centre + rng.normal(scale=2.0, size=(n, 3)) - o
    scale = np.float64([1e-4, 1e-6, 1e-9])[rng.integers(0, 3, n)] * np.abs(d).max(axis=1)
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    ax = rng.integers(0, 3, n)
    d[np.arange(n), ax] = sign * scale
    two = rng.random(n) < 0.3  # a second near-parallel axis
    ax2 = (ax + 1 + rng.integers(0, 2, n)) % 3
    d[np.arange(n)[two], ax2[two]] = -sign[two] * scale[two]
    travs = ("reference", "fast", "brute") if cfg["type"] == "cornell" else ("reference", "fast")
    _hit_equal(rt, oracle, sd, o.astype(np.float32), d.astype(np.float32), travs=travs)


def test_sah_tree_on_surface_and_grazing_rays(rt, oracle, gpu):
    """spheres-500 (SAH fast tree): secondary-ray-like origins on sphere surfaces,
    tangent directions, and far/axis-parallel rays."""
    sd = rt.generate_scene_data({"type": "spheres", "options": {"count": 500, "seed": 42}})
    rng = np.random.default_rng(5)
    sph = [ob for ob in sd["objects"] if ob["type"] == "sphere"]
    n = 6000
    idx = rng.integers(0, len(sph), n)
    c = np.array([sph[k]["pos"] for k in idx], np.float64)
    r = np.array([sph[k]["r"] for k in idx], np.float64)
    nrm = rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    o = (c + np.abs(r)[:, None] * nrm).astype(np.float32)   # on the surface
    d = rng.normal(size=(n, 3))
    d[: n // 3] -= (d[: n // 3] * nrm[: n // 3]).sum(1, keepdims=True) * nrm[: n // 3]  # tangent
    d[n // 3: n // 2, rng.integers(0, 3)] = 0.0
    far = rng.uniform(-50, 50, (n // 4, 3)).astype(np.float32)
    o[-(n // 4):] = far
    _hit_equal(rt, oracle, sd, o, d.astype(np.float32), travs=("reference", "fast"))


@pytest.mark.parametrize("name", ["cornell", "spheres", "rain"])
def test_chunked_kernel_equals_sequential(rt, gpu, name, monkeypatch):
    """The chunked kernel (lane work pool + in-order accumulate) reproduces the
    sequential kernel's image and stats bit for bit."""
    cfg, ro = _cfgs()[name]
    sd = rt.generate_scene_data(cfg)
    ro = {**ro, "width": 160, "samples": 37}  # odd spp: every guided phase, partial tiles
    outs = []
    for flag in ("1", "0"):
        monkeypatch.setenv("RT_AMD_CHUNKED", flag)
        cam, rgb, rad, st = _render_gpu(rt, sd, ro)
        outs.append((rgb, rad, st))
    assert np.array_equal(outs[0][0], outs[1][0])
    assert np.array_equal(outs[0][1], outs[1][1], equal_nan=True)
    assert outs[0][2].samples == outs[1][2].samples and outs[0][2].bounces == outs[1][2].bounces


def _pool_cases():
    sd_c = {"type": "cornell"}
    return [
        ("cornell ref", sd_c, {"width": 164, "samples": 37, "depth": 16}, "ref"),  # partial tiles, every phase
        ("cornell fp32", sd_c, {"width": 96, "samples": 64, "depth": 16}, "fp32"),
        ("cornell d100 spp1", sd_c, {"width": 72, "samples": 1, "depth": 100}, "ref"),
        ("tiny1", 1, {"width": 40, "samples": 9, "depth": 6}, "ref"),
        ("tiny5", 5, {"width": 56, "samples": 9, "depth": 6}, "ref"),
    ]


@pytest.mark.parametrize("case", range(5))
def test_pool_kernel_equals_chunked_kernel(rt, gpu, case, monkeypatch):
    """The stage-compacted pool kernel (per-wave path pools, A/D queues) writes
    the chunked kernel's per-sample records, so images and stats are identical;
    also a region render and a tile-group share."""
    what, cfg, ro, prec = _pool_cases()[case]
    sd = _tiny_scene(cfg) if isinstance(cfg, int) else rt.generate_scene_data(cfg)
    ro = {**ro, **NOADAPT, "traversal": "brute"}
    monkeypatch.setenv("RT_AMD_CHUNKED", "1")
    outs = []
    for flag in ("1", "0"):
        monkeypatch.setenv("RT_AMD_POOL_KERNEL", flag)
        cam, rgb, rad, st = _render_gpu(rt, sd, ro, precision=prec)
        assert cam.last_kernel() == ("pool" if flag == "1" else "chunked"), what
        W, H = cam.image_width, cam.image_height
        reg = (5, 3, W - 9, H - 6)
        _, rgb_r, rad_r, st_r = _render_gpu(rt, sd, ro, precision=prec, region=reg)
        outs.append((rgb, rad, st, rgb_r, rad_r, st_r))
    a, b = outs
    assert_identical(a[1], a[0], b[1], b[0], f"pool vs chunked: {what}")
    assert_identical(a[4], a[3], b[4], b[3], f"pool vs chunked region: {what}")
    for sa, sb in ((a[2], b[2]), (a[5], b[5])):
        assert sa.pixels == sb.pixels and sa.samples == sb.samples and sa.bounces == sb.bounces


@pytest.mark.parametrize("ro,kernel", [
    ({"width": 24, "samples": 3, "depth": 250}, "pool"),        # deepest path a slot's phase byte holds
    ({"width": 24, "samples": 3, "depth": 251}, "chunked"),     # past it: host falls back
    ({"width": 4, "samples": 65535, "depth": 4}, "pool"),       # largest sample index a slot holds
    ({"width": 4, "samples": 65536, "depth": 4}, "chunked"),
])
def test_pool_host_gates_fall_back_bit_exact(rt, oracle, gpu, ro, kernel):
    """The pool kernel packs the bounce phase into 8 bits and the sample index
    into 16 (pt_pool.hpp pool_meta / pool_hs); launch_plan.cpp gates it on
    depth <= 250 and spp <= 65535. On each side of both gates the default path
    picks the expected kernel and matches the oracle bit for bit."""
    sd = rt.generate_scene_data({"type": "cornell"})
    ro = {**ro, "aspect": 1, **NOADAPT}
    cam, rgb, rad, st = _render_gpu(rt, sd, ro)
    assert cam.last_kernel() == kernel
    orc = oracle.render(sd, ro, threads=8)
    assert_identical(rad, rgb, orc["radiance"], orc["rgb"], f"gate {ro} -> {kernel}")
    assert_stats_identical(st, orc["stats"])


def _cornell_plus_spheres(n_extra):
    """Cornell with n_extra small Lambertian spheres on the floor (8 + n_extra primitives)."""
    import copy
    import raytracer_amd as rt
    sd = copy.deepcopy(rt.generate_scene_data({"type": "cornell"}))
    for k in range(n_extra):
        sd["objects"].append({"type": "sphere", "pos": [-0.8 + 0.2 * k, -0.9, 0.3 - 0.1 * (k % 3)], "r": 0.08,
                              "material": "sphere-white"})
    return sd


@pytest.mark.parametrize("n_extra,kernel", [(1, "pool"), (8, "chunked")])
def test_pool_lds_budget_gate_falls_back_bit_exact(rt, oracle, gpu, n_extra, kernel):
    """The pool kernel's LDS: fp16 candidate columns (primitives x 1024 x 2 B) + the level-2
    scene + 16 waves x 152 path slots. Cornell + 1 sphere (9 primitives) still fits; Cornell +
    8 (16 primitives: 32 KB of columns) does not, and launch_plan.cpp's gate must hand the launch
    to the chunked kernel - the same image either way."""
    sd = _cornell_plus_spheres(n_extra)
    ro = {"width": 48, "aspect": 1, "samples": 8, "depth": 10, **NOADAPT}
    cam, rgb, rad, st = _render_gpu(rt, sd, ro)
    assert cam.info["traversal"] == 2  # AUTO -> brute force (<= 16 primitives)
    assert cam.last_kernel() == kernel
    orc = oracle.render(sd, ro)
    assert_identical(rad, rgb, orc["radiance"], orc["rgb"], f"LDS gate +{n_extra} -> {kernel}")
    assert_stats_identical(st, orc["stats"])


def _tiny_scene(n):
    objs = [{"type": "sphere", "pos": [0.9 * k - 0.9, 0.3 * (k % 2), -0.2 * k], "r": 0.45, "material": "m"}
            for k in range(n)]
    return {"camera": {"vfov": 40, "from": [0, 0.5, 4], "at": [0, 0, 0], "up": [0, 1, 0],
                       "background": {"type": "gradient", "top": [0.5, 0.7, 1.0], "bottom": [1, 1, 1]}},
            "materials": [{"id": "m", "material": {"type": "metal", "color": [0.8, 0.8, 0.8], "fuzz": 0.1}}],
            "objects": objs}


@pytest.mark.parametrize("n", [1, 3, 5])
def test_tiny_scenes_every_strategy(rt, oracle, gpu, n):
    """One-leaf trees (the fast walk starts on a leaf) and two-leaf trees: every
    closest-hit strategy against the oracle, on hits and on images."""
    sd = _tiny_scene(n)
    rng = np.random.default_rng(n)
    m = 3000
    o = rng.uniform(-3, 3, (m, 3)).astype(np.float32)
    d = rng.normal(size=(m, 3)).astype(np.float32)
    c = _hit_equal(rt, oracle, sd, o, d)
    assert (c[:, 0] > 0).any()
    ro = {"width": 40, "samples": 4, "depth": 6, **NOADAPT}
    orc = oracle.render(sd, ro)
    for trav in ("fast", "brute", "reference"):
        _, rgb, rad, st = _render_gpu(rt, sd, {**ro, "traversal": trav})
        assert_identical(rad, rgb, orc["radiance"], orc["rgb"], f"tiny {n} {trav}")
        assert_stats_identical(st, orc["stats"])


def test_large_scene_global_traversal(rt, oracle, gpu, monkeypatch):
    """A scene too large for the LDS-resident copy (deeper SAH tree walked from
    global memory, chunked kernel): fast == reference traversal bit for bit,
    and hits against the oracle."""
    sd = rt.generate_scene_data({"type": "spheres", "options": {"count": 6000, "seed": 9}})
    ro = {"width": 96, "aspect": 1, "samples": 8, "depth": 12, **NOADAPT}
    outs = []
    # (the chunked kernels read the fp64 leaf records, tsph2; the sequential kernel of the
    # reference-order pass does not), with and without deferred exact tests and the LDS top
    # cache, and with SAH leaves of 1 (this size's default), 2 and 4
    for trav, defer, top, leaf in (("reference", "0", "1", "1"), ("fast", "0", "1", "1"), ("fast", "1", "1", "1"),
                                   ("fast", "0", "0", "1"), ("fast", "1", "0", "1"), ("fast", "0", "1", "2"),
                                   ("fast", "0", "1", "4")):
        monkeypatch.setenv("RT_AMD_DEFER", defer)
        monkeypatch.setenv("RT_AMD_TOP_CACHE", top)
        monkeypatch.setenv("RT_AMD_SAH_MAXLEAF", leaf)
        cam, rgb, rad, st = _render_gpu(rt, sd, {**ro, "traversal": trav})
        outs.append((rgb, rad, st))
    for k in range(1, len(outs)):
        assert np.array_equal(outs[0][0], outs[k][0])
        assert np.array_equal(outs[0][1], outs[k][1], equal_nan=True)
        assert outs[0][2].bounces == outs[k][2].bounces
    rng = np.random.default_rng(3)
    n = 4000
    o = (rng.uniform(-20, 20, (n, 3)) + np.float64([0, 2, 0])).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d[:, 1] = -np.abs(d[:, 1])  # mostly toward the sphere field
    _hit_equal(rt, oracle, sd, o, d, travs=("reference", "fast"))


# BASELINE.json configs at their full sizes: the GPU renders the whole frame;
# the oracle (8 threads) re-renders a few full rows of it, which must agree
# bit-for-bit (same contract as above). Config 5 (spheres-100k, spp 1024) runs
# at spp 16 here: its per-sample work is the same, only the loop is shorter.
FULL = {
    "cornell": ({"type": "cornell"}, {"width": 800, "samples": 256, "depth": 16}, [0, 233, 400, 611, 799]),
    "spheres": ({"type": "spheres", "options": {"count": 500, "seed": 42}},
                {"width": 800, "aspect": 1, "samples": 64, "depth": 8}, [57, 400, 743]),
    "rain": ({"type": "rain", "options": {"seed": 42}}, {"width": 1920, "samples": 512, "depth": 16}, [540]),
    "spheres100k": ({"type": "spheres", "options": {"count": 100000, "seed": 42}},
                    {"width": 4096, "aspect": 1, "samples": 16, "depth": 100}, [2048]),
}


@pytest.mark.parametrize("name", list(FULL))
def test_full_size_config_rows_match_oracle(rt, oracle, gpu, name):
    cfg, ro, rows = FULL[name]
    ro = {**ro, **NOADAPT}
    sd = rt.generate_scene_data(cfg)
    cam, rgb, rad, st = _render_gpu(rt, sd, ro)
    W, H = cam.image_width, cam.image_height
    assert st.pixels == W * H
    assert st.samples["total"] == W * H * ro["samples"]
    assert st.samples["min"] == st.samples["max"] == ro["samples"]
    for y in rows:
        orc = oracle.render(sd, ro, region=(0, y, W, 1), threads=8)
        assert_identical(rad[y:y + 1], rgb[y:y + 1], orc["radiance"][y:y + 1], orc["rgb"][y:y + 1],
                         f"{name} {W}x{H} row {y}")


def test_full_size_headline_partition_and_determinism(rt, gpu):
    """Cornell 800x800 spp 256: repeated renders are identical, and the 8-way
    tile interleave (the 8-GPU split) reassembles the single-launch frame."""
    import torch
    sd = rt.generate_scene_data({"type": "cornell"})
    cam = rt.create_camera_from_scene_data(sd, {"width": 800, "samples": 256, "depth": 16, **NOADAPT})
    W, H = cam.image_width, cam.image_height
    full = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    rad = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    cam.render_device(rgb_ptr=full.data_ptr(), radiance_ptr=rad.data_ptr(), synchronize=True)
    again = torch.zeros_like(full)
    rad2 = torch.zeros_like(rad)
    cam.render_device(rgb_ptr=again.data_ptr(), radiance_ptr=rad2.data_ptr(), synchronize=True)
    assert torch.equal(full, again) and torch.equal(rad, rad2)
    acc = torch.zeros_like(full)
    acc_rad = torch.zeros_like(rad)
    total = 0
    for g in range(8):
        part = torch.zeros_like(full)
        prad = torch.zeros_like(rad)
        st, _ = cam.render_device(rgb_ptr=part.data_ptr(), radiance_ptr=prad.data_ptr(), tile_group=g,
                                  tile_groups=8, synchronize=True)
        total += st.pixels
        acc += part
        acc_rad += prad
    assert total == W * H
    assert torch.equal(acc, full) and torch.equal(acc_rad, rad)


def _random_scene(seed):
    """A randomized custom SceneData: 1-40 objects (brute force up to 16, the 4-wide tree above),
    every material kind (nested mixed/layered, emissive), axis-aligned and tilted quads, planes,
    quad and sphere lights, sometimes a negative-radius sphere (reference-order traversal) and
    a lens aperture."""
    r = np.random.default_rng(seed)

    def col():
        return [round(float(x), 3) for x in r.uniform(0.05, 0.95, 3)]

    def base_mat():
        k = r.integers(0, 4)
        if k == 0:
            return {"type": "lambert", "color": col()}
        if k == 1:
            return {"type": "metal", "color": col(), "fuzz": round(float(r.uniform(0, 0.6)), 3)}
        if k == 2:
            return {"type": "glass", "ior": round(float(r.uniform(1.2, 2.0)), 3)}
        return {"type": "light", "emit": [round(float(x), 2) for x in r.uniform(0.5, 6, 3)]}

    mats = [{"id": f"m{i}", "material": base_mat()} for i in range(5)]
    mats.append({"id": "mx", "material": {"type": "mixed", "diff": "m0", "spec": base_mat(),
                                          "weight": round(float(r.uniform(0.1, 0.9)), 3)}})
    mats.append({"id": "ly", "material": {"type": "layered", "outer": {"type": "glass", "ior": 1.5},
                                          "inner": base_mat()}})
    ids = [m["id"] for m in mats]
    objs = []
    n = int(r.integers(1, 41))
    for _ in range(n):
        k = r.integers(0, 10)
        pos = [round(float(x), 3) for x in r.uniform(-2, 2, 3)]
        mat = ids[int(r.integers(0, len(ids)))]
        if k < 6:
            rad = round(float(r.uniform(0.1, 0.7)), 3)
            if r.random() < 0.05:
                rad = -rad
            objs.append({"type": "sphere", "pos": pos, "r": rad, "material": mat})
        elif k < 9:
            if r.random() < 0.5:  # axis-aligned
                a = int(r.integers(0, 3))
                u = [0.0, 0.0, 0.0]
                v = [0.0, 0.0, 0.0]
                u[(a + 1) % 3] = round(float(r.uniform(0.3, 2)), 3)
                v[(a + 2) % 3] = round(float(r.uniform(0.3, 2)), 3)
            else:
                u = [round(float(x), 3) for x in r.uniform(-1.5, 1.5, 3)]
                v = [round(float(x), 3) for x in r.uniform(-1.5, 1.5, 3)]
            objs.append({"type": "quad", "pos": pos, "u": u, "v": v, "material": mat})
        else:
            objs.append({"type": "plane", "pos": [0, -2.5, 0], "u": [1, 0, 0], "v": [0, 0, -1], "material": mat})
        if r.random() < 0.15 and objs[-1]["type"] != "plane":
            objs[-1]["light"] = True
    ap = 0.05 if r.random() < 0.3 else 0.0
    return {"camera": {"vfov": 45, "from": [0.3, 1.0, 6.0], "at": [0, 0, 0], "up": [0, 1, 0], "aperture": ap,
                       "focus": 6.0 if ap else 0,
                       "background": {"type": "gradient", "top": [0.5, 0.7, 1.0], "bottom": [1, 1, 1]}},
            "materials": mats, "objects": objs}


@pytest.mark.parametrize("seed", range(12))
def test_random_scenes_match_oracle(rt, oracle, gpu, seed, monkeypatch):
    sd = _random_scene(seed)
    ro = {"width": 32, "samples": 4, "depth": 8, **NOADAPT}
    orc = oracle.render(sd, ro)
    for trav, defer in (("auto", "0"), ("fast", "0"), ("fast", "1"), ("brute", "0"), ("reference", "0")):
        monkeypatch.setenv("RT_AMD_DEFER", defer)
        cam, rgb, rad, st = _render_gpu(rt, sd, {**ro, "traversal": trav})
        assert_identical(rad, rgb, orc["radiance"], orc["rgb"],
                         f"random {seed} {trav} defer {defer} ({len(sd['objects'])} objects)")
        assert_stats_identical(st, orc["stats"])


def test_edge_cases_match_oracle(rt, oracle, gpu):
    """No objects (the reference's BVHNode dereferences a null box: the same error),
    a single-pixel-wide image, samples = 1 (no jitter)."""
    empty = {"camera": {"vfov": 40, "from": [0, 0, 3], "at": [0, 0, 0], "up": [0, 1, 0],
                        "background": {"type": "gradient", "top": [0.2, 0.4, 1.0], "bottom": [1, 0.9, 0.8]}},
             "materials": [], "objects": []}
    with pytest.raises(rt.RtError, match="reading 'maximum'"):
        rt.create_camera_from_scene_data(empty, {"width": 16})
    for sd, ro in [(rt.generate_scene_data({"type": "cornell"}), {"width": 1, "aspect": 0.25, "samples": 8, "depth": 8}),
                   (rt.generate_scene_data({"type": "cornell"}), {"width": 24, "samples": 1, "depth": 8})]:
        ro = {**ro, **NOADAPT}
        orc = oracle.render(sd, ro)
        cam, rgb, rad, st = _render_gpu(rt, sd, ro)
        assert rgb.shape == orc["rgb"].shape
        assert_identical(rad, rgb, orc["radiance"], orc["rgb"], f"edge {ro}")
        assert_stats_identical(st, orc["stats"])


def test_config1_spheres10_full_frame_matches_oracle(rt, oracle, gpu):
    """BASELINE config 1 at its stated workload: spheres (count 10, seed 42),
    200x200, spp 4, depth 4 (src/benchmark.ts:25-97, scenes-spheres.ts:32) -
    the whole frame against the oracle, bit for bit."""
    sd = rt.generate_scene_data({"type": "spheres", "options": {"seed": 42}})
    assert len(sd["objects"]) == 10  # count 10 (scenes-spheres.ts:32)
    ro = {"width": 200, "aspect": 1, "samples": 4, "depth": 4, **NOADAPT}
    cam, rgb, rad, st = _render_gpu(rt, sd, ro)
    assert (cam.image_width, cam.image_height) == (200, 200)
    orc = oracle.render(sd, ro, threads=8)
    assert_identical(rad, rgb, orc["radiance"], orc["rgb"], "config 1")
    assert_stats_identical(st, orc["stats"])


def test_config5_spheres100k_spp1024_full_frame(rt, oracle, gpu):
    """BASELINE config 5 at its stated workload: spheres-100k (seed 42), 4096x4096,
    spp 1024, depth 100. The GPU renders the whole frame through the multi-pass
    sample-record path (~34 passes of <= 8 GB); the oracle re-renders two 8-pixel
    row segments (sky/field boundary and the sphere field) at spp 1024, depth 100."""
    sd = rt.generate_scene_data({"type": "spheres", "options": {"count": 100000, "seed": 42}})
    ro = {"width": 4096, "aspect": 1, "samples": 1024, "depth": 100, **NOADAPT}
    cam, rgb, rad, st = _render_gpu(rt, sd, ro)
    W, H = cam.image_width, cam.image_height
    assert st.pixels == W * H and st.samples["total"] == W * H * 1024
    assert st.samples["min"] == st.samples["max"] == 1024
    passes = cam.pass_count()
    print(f"config 5: {passes} passes, bounces avg {st.bounces['avg']:.3f} max {st.bounces['max']}")
    assert passes > 1
    for (x, y) in [(2044, 1900), (1000, 3000)]:
        orc = oracle.render(sd, ro, region=(x, y, 8, 1), threads=16)
        assert_identical(rad[y:y + 1, x:x + 8], rgb[y:y + 1, x:x + 8], orc["radiance"][y:y + 1, x:x + 8],
                         orc["rgb"][y:y + 1, x:x + 8], f"config 5 row {y} x {x}..{x + 7}")


def test_multipass_chunked_equals_single_pass(rt, gpu, monkeypatch):
    """A small record budget forces several chunked passes (dev_ctx.cpp launch_fixed);
    the image, stats and per-pass kernel timing must be the single-pass ones."""
    sd = rt.generate_scene_data({"type": "cornell"})
    ro = {"width": 96, "samples": 37, "depth": 16, **NOADAPT}
    monkeypatch.setenv("RT_AMD_CHUNKED", "1")
    cam1, rgb1, rad1, st1 = _render_gpu(rt, sd, ro)
    assert cam1.pass_count() == 1
    # 1 MB / (64 px x 37 x 12 B) = 36 tiles per pass: 4 passes of the 144 tiles; with 16-byte
    # records (RT_AMD_REC12=0: the bounce word in the record) 27 tiles per pass: 6 passes
    monkeypatch.setenv("RT_AMD_SBUF_MB", "1")
    for rec12, passes in (("1", 4), ("0", 6)):
        monkeypatch.setenv("RT_AMD_REC12", rec12)
        cam2, rgb2, rad2, st2 = _render_gpu(rt, sd, ro)
        assert cam2.pass_count() == passes
        path_ms, acc_ms = cam2.kernel_times()
        assert path_ms > 0 and acc_ms > 0
        assert np.array_equal(rgb1, rgb2) and np.array_equal(rad1, rad2, equal_nan=True)
        assert st1.samples == st2.samples and st1.bounces == st2.bounces


@pytest.mark.gpu
@pytest.mark.parametrize("scene,kernel_env", [("cornell", {}), ("spheres", {}), ("cornell", {"RT_AMD_CHUNKED": "1"})])
def test_twelve_byte_records_equal_sixteen_byte_records(rt, gpu, monkeypatch, scene, kernel_env):
    """SampleBuf::rec12: {r, g, b} records with the bounce statistics reduced per lane in the
    path kernel give the 16-byte records' image and RenderStats (bounce total / min / max
    included) on the pool and the chunked kernel, over a region that cuts tiles."""
    opts = {"cornell": {"type": "cornell"}, "spheres": {"type": "spheres", "options": {"count": 200, "seed": 3}}}[scene]
    sd = rt.generate_scene_data(opts)
    ro = {"width": 72, "samples": 21, "depth": 12, **NOADAPT}
    for k, v in kernel_env.items():
        monkeypatch.setenv(k, v)
    out = []
    for rec12 in ("1", "0"):
        monkeypatch.setenv("RT_AMD_REC12", rec12)
        cam = rt.create_camera_from_scene_data(sd, ro)
        W, H = cam.image_width, cam.image_height
        rgb = np.zeros((H, W, 3), np.uint8)
        rad = np.zeros((H, W, 3), np.float32)
        st = cam.render_region(rgb, (3, 5, W - 7, H - 9), radiance=rad)
        out.append((rgb, rad, st))
    (a_rgb, a_rad, a_st), (b_rgb, b_rad, b_st) = out
    assert_identical(a_rad, a_rgb, b_rad, b_rgb, f"rec12 vs rec16 {scene} {kernel_env}")
    assert a_st.pixels == b_st.pixels and a_st.samples == b_st.samples and a_st.bounces == b_st.bounces


def test_release_device_then_render_again(rt, gpu):
    """rt_camera_release_device frees every device buffer and nulls it; the next
    render must re-create all of them (no use of a freed frame buffer)."""
    sd = rt.generate_scene_data({"type": "cornell"})
    ro = {"width": 40, "samples": 8, "depth": 8, **NOADAPT}
    cam, rgb, rad, st = _render_gpu(rt, sd, ro)
    for _ in range(2):
        cam.release_device()
        rgb2 = np.zeros_like(rgb)
        rad2 = np.zeros_like(rad)
        st2 = cam.render(rgb2, radiance=rad2)
        assert np.array_equal(rgb, rgb2) and np.array_equal(rad, rad2) and st.bounces == st2.bounces


PACKED_CASES = {
    # chunked kernel, one pass
    "rain": ({"type": "rain", "options": {"seed": 42}}, {"width": 72, "samples": 4, "depth": 8, **NOADAPT}, {},
             "chunked"),
    # the pool kernel's packed-index path
    "cornell_pool": ({"type": "cornell"}, {"width": 72, "samples": 8, "depth": 8, **NOADAPT}, {}, "pool"),
    # adaptive sampling: the rounds' packed index (launch slot) and the sequential kernel's
    "adaptive": ({"type": "cornell"}, {"width": 72, "samples": 30, "depth": 8}, {}, "pool"),
    "adaptive_seq": ({"type": "cornell"}, {"width": 72, "samples": 30, "depth": 8}, {"RT_AMD_ADAPT_ROUNDS": "0"},
                     "sequential"),
    # a record budget that forces several passes (the pass's tile offset in the packed index)
    "multipass": ({"type": "rain", "options": {"seed": 42}}, {"width": 72, "samples": 64, "depth": 8, **NOADAPT},
                  {"RT_AMD_SBUF_MB": "1"}, "chunked"),
}


@pytest.mark.parametrize("case", sorted(PACKED_CASES))
@pytest.mark.parametrize("region", [None, (3, 5, 50, 41)])
def test_packed_slabs_unpack_to_the_frame(rt, gpu, region, case, monkeypatch):
    """The multi-GPU gather's device side: each tile group's tile-packed render
    (rt_launch.packed_tiles), stacked as the RCCL gather stacks them, unpacked by
    rt_tiles_unpack, equals the single full-frame render (u8 and fp32) - for every
    kernel's packed-index path (chunked, pool, sequential / adaptive, multi-pass)."""
    import torch
    from raytracer_amd import distributed as rtd
    cfg, ro, env, kernel = PACKED_CASES[case]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sd = rt.generate_scene_data(cfg)
    cam = rt.create_camera_from_scene_data(sd, ro)
    W, H = cam.image_width, cam.image_height
    reg = rtd.clamp_region(region or (0, 0, W, H), W, H)
    full = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    frad = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    cam.render_device(rgb_ptr=full.data_ptr(), radiance_ptr=frad.data_ptr(), region=reg, synchronize=True)
    assert cam.last_kernel() == kernel
    if case == "multipass":
        assert cam.pass_count() > 1
    for world in (1, 3, 8):
        n_px = rtd.slab_tiles(reg, world) * 64
        slabs = torch.zeros((world, n_px, 3), dtype=torch.uint8, device="cuda")
        rslabs = torch.zeros((world, n_px, 3), dtype=torch.float32, device="cuda")
        for g in range(world):
            cam.render_device(rgb_ptr=slabs[g].data_ptr(), radiance_ptr=rslabs[g].data_ptr(), region=reg,
                              tile_group=g, tile_groups=world, packed=True, synchronize=True)
        out = torch.zeros_like(full)
        rout = torch.zeros_like(frad)
        rtd.unpack_tiles(slabs, reg, W, H, out)
        rtd.unpack_tiles(rslabs, reg, W, H, rout)
        torch.cuda.synchronize()
        assert torch.equal(out, full) and torch.equal(rout, frad), world


def test_generate_image_buffer_png_pixels_equal_render(rt, gpu):
    """generateImageBuffer's PNG (rendered and encoded on the device,
    rt_camera_render_png) carries exactly the rendered u8 frame, is byte-identical
    to the host run of the same encoder, and its merged stats equal a render's."""
    from raytracer_amd.png import debug_png_host, decode_png_rgb
    cfg = {"type": "cornell", "render": {"width": 48, "samples": 4, "depth": 4, "aTolerance": 0}}
    png, st = rt.generate_image_buffer(cfg, {"parallel": True, "threads": 7}, return_stats=True)
    cam = rt.generate_scene(cfg)
    rgb = np.zeros((48, 48, 3), np.uint8)
    st1 = cam.render(rgb)
    w, h, px = decode_png_rgb(png)
    assert (w, h) == (48, 48) and px == rgb.tobytes()
    assert png == debug_png_host(rgb.tobytes(), 48, 48)
    assert (st.pixels, st.samples, st.bounces) == (st1.pixels, st1.samples, st1.bounces)


def test_device_png_encoder_matches_host_run(rt, gpu):
    """rt_encode_png_device on frames already in HBM: the bytes equal the host run
    of the same algorithm (rt_debug_png_host) and decode to the frame - a rendered
    frame, noise (stored blocks), a flat frame (runs) and a 4096-wide gradient
    whose rows span several segments."""
    import torch
    from raytracer_amd.png import debug_png_host, decode_png_rgb, encode_png_device
    g = torch.Generator().manual_seed(3)
    yy, xx = torch.meshgrid(torch.arange(40), torch.arange(4096), indexing="ij")
    grad = torch.stack([xx % 256, (yy * 6) % 256, (xx // 16 + yy) % 256], -1).to(torch.uint8)
    sd = rt.generate_scene_data({"type": "cornell"})
    cam = rt.create_camera_from_scene_data(sd, {"width": 64, "samples": 8, "depth": 6, "aTolerance": 0})
    frame = torch.zeros((64, 64, 3), dtype=torch.uint8, device="cuda")
    cam.render_device(rgb_ptr=frame.data_ptr(), synchronize=True)
    frames = {"render": frame.cpu(), "noise": torch.randint(0, 256, (33, 129, 3), generator=g, dtype=torch.uint8),
              "flat": torch.full((20, 700, 3), 200, dtype=torch.uint8), "wide_gradient": grad}
    for name, f in frames.items():
        h, w, _ = f.shape
        d = f.cuda().contiguous()
        png = encode_png_device(d.data_ptr(), w, h)
        host = f.numpy().tobytes()
        assert png == debug_png_host(host, w, h), name
        assert decode_png_rgb(png) == (w, h, host), name


def test_bench_two_ranks_one_gpu_assemble_the_frame(gpu):
    """bench.py's multi-GPU path end to end on one device: 2 ranks (launched by
    bench.py --gpus 2 itself) render their tile-packed shares, gather them over a
    CPU backend and rank 0 unpacks them; the frame equals one single-launch render."""
    import json
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parents[1]
    env = {k: v for k, v in __import__("os").environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, str(root / "bench.py"), "--gpus", "2", "--backend", "gloo", "--steps", "2",
                        "--warmup", "1", "--full", "--no-cpu", "--no-count", "--check", "--width", "200",
                        "--spp", "16"],
                       capture_output=True, text=True, timeout=240, env=env, cwd=str(root))
    assert r.returncode == 0, r.stderr[-4000:]
    line = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    print({k: line[k] for k in ("value", "n_gpus", "ms_per_step", "frame_check")})
    assert line["n_gpus"] == 2 and line["frame_check"] is True


def test_bench_plain_run_dumps_the_timed_frame(gpu, rt, tmp_path):
    """A plain bench.py run (no --full) times exactly --steps steps once, prints the headline
    keys without the --full legs, and --dump-outputs writes the last timed frame: float32,
    equal to an in-process render of the same scene, options and seed."""
    import json
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parents[1]
    env = {k: v for k, v in __import__("os").environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, str(root / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--width", "72", "--spp", "8", "--depth", "8", "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=120, env=env, cwd=str(root))
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = lines[0]
    assert line["steps"] == 3 and line["warmup"] == 1 and line["repeats"]["n"] == 1
    assert line["ms_per_step"] > 0 and line["repeats"]["ms_per_step"] == [line["ms_per_step"]]
    assert line["unit"] == "Msamples/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    # value = samples per step / ms_per_step; ms_per_step is printed to 1 us, a step takes > 25 us
    assert line["value"] == pytest.approx(72 * 72 * 8 / line["ms_per_step"] / 1e3, rel=2e-2)
    assert not {"parity", "roofline", "cpu_baseline"} & set(line)
    out = np.load(tmp_path / "frame.npy")
    assert out.dtype == np.float32 and out.shape == (72, 72, 3)
    cam = rt.create_camera_from_scene_data(rt.generate_scene_data({"type": "cornell"}),
                                           {"width": 72, "samples": 8, "depth": 8, "aTolerance": 0, "seed": 0x5EED})
    rgb = np.zeros((72, 72, 3), np.uint8)
    cam.render(rgb)
    assert np.array_equal(out, rgb)


@pytest.mark.parametrize("groups,scene", [(3, "cornell"), (2, "spheres")])
def test_rccl_gather_of_tile_groups_assembles_the_frame(gpu, groups, scene):
    """The RCCL leg on a one-GPU box (RCCL refuses two ranks on one device): a world-1
    "nccl" process group in a child process gathers each tile group's packed u8 slab
    (with its stats tile) through dist.gather, rt_tiles_unpack assembles the frame, and
    frame and merged stats equal a single launch (tests/rccl_one_rank.py)."""
    import json
    import os
    import socket
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parents[1]
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    r = subprocess.run([sys.executable, str(root / "tests" / "rccl_one_rank.py"), str(groups), scene],
                       capture_output=True, text=True, timeout=180, env=env, cwd=str(root))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    out = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    print(out)
    assert out["backend"] == "nccl" and out["frame_equal"] and out["stats_equal"] and out["slabs_equal_gathered"]
    assert out["all_reduce"] == [1.5, 2.5]


# ---------------------------------------------------------------------------
# Adaptive sampling in rounds (dev_ctx.cpp launch_adaptive_rounds, pt_adapt_kernel):
# the chunked / pool kernels render each round's samples speculatively, the adapt
# pass settles them in sample order with the reference's convergence check after
# every sample (src/camera.ts:348-368,400-425). Same pixels, same stats as the
# sequential kernel and the oracle.
# ---------------------------------------------------------------------------
ADAPT_CASES = {
    # (scene, render options, env, kernel that renders the rounds)
    "cornell_pool": ({"type": "cornell"}, {"width": 48, "samples": 90, "depth": 8}, {}, "pool"),
    "cornell_batch1": ({"type": "cornell"}, {"width": 40, "samples": 37, "depth": 8, "aBatch": 1}, {}, "pool"),
    "cornell_batch2_5": ({"type": "cornell"}, {"width": 40, "samples": 41, "depth": 8, "aBatch": 2.5,
                                               "aTolerance": 0.2}, {}, "pool"),
    "cornell_multipass": ({"type": "cornell"}, {"width": 64, "samples": 70, "depth": 8},
                          {"RT_AMD_SBUF_MB": "1"}, "pool"),
    "cornell_chunked": ({"type": "cornell"}, {"width": 40, "samples": 60, "depth": 8},
                        {"RT_AMD_POOL_KERNEL": "0"}, "chunked"),
    "spheres_bvh": ({"type": "spheres", "options": {"count": 500, "seed": 42}},
                    {"width": 48, "aspect": 1, "samples": 50, "depth": 8, "aTolerance": 0.1}, {}, "chunked"),
    "default_scene": ({"type": "default"}, {"width": 40, "samples": 30, "depth": 10, "aTolerance": 0.1}, {},
                      "chunked"),
}


@pytest.mark.parametrize("case", sorted(ADAPT_CASES))
def test_adaptive_rounds_match_oracle_and_sequential(rt, oracle, gpu, case, monkeypatch):
    cfg, ro, env, kernel = ADAPT_CASES[case]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sd = rt.generate_scene_data(cfg)
    cam, rgb, rad, st = _render_gpu(rt, sd, ro)
    assert cam.last_kernel() == kernel
    if case == "cornell_multipass":
        assert cam.pass_count() > 4  # several rounds, several passes each
    orc = oracle.render(sd, ro)
    assert_identical(rad, rgb, orc["radiance"], orc["rgb"], f"adaptive rounds {case}")
    assert_stats_identical(st, orc["stats"])
    assert st.samples["min"] < ro["samples"]  # some pixels converged early
    monkeypatch.setenv("RT_AMD_ADAPT_ROUNDS", "0")
    cam2, rgb2, rad2, st2 = _render_gpu(rt, sd, ro)
    assert cam2.last_kernel() == "sequential"
    assert_identical(rad, rgb, rad2, rgb2, f"adaptive rounds == sequential {case}")
    assert st.samples == st2.samples and st.bounces == st2.bounces


@pytest.mark.parametrize("mode", ["bounces", "samples"])
def test_adaptive_rounds_render_modes_and_tile_groups(rt, oracle, gpu, mode):
    """The visualisation modes and a 3-way tile split (a rank's share) through the
    adaptive rounds: the three shares reassemble the oracle's frame, and their
    merged stats are the whole frame's."""
    import torch
    from raytracer_amd import distributed as rtd
    sd = rt.generate_scene_data({"type": "cornell"})
    ro = {"width": 40, "samples": 50, "depth": 8, "mode": mode}
    orc = oracle.render(sd, ro)
    cam = rt.create_camera_from_scene_data(sd, ro)
    W, H = cam.image_width, cam.image_height
    rgb = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    rad = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    words = torch.zeros((3, 8), dtype=torch.int64, device="cuda")
    for g in range(3):
        cam.render_device(rgb_ptr=rgb.data_ptr(), radiance_ptr=rad.data_ptr(), tile_group=g, tile_groups=3,
                          synchronize=True)
        assert cam.last_kernel() == "pool"
        cam.stats_words(words[g].data_ptr())
    torch.cuda.synchronize()
    assert_identical(rad.cpu().numpy(), rgb.cpu().numpy(), orc["radiance"], orc["rgb"], f"adaptive {mode} 3 groups")
    st = rtd.stats_from_words(rtd.merge_stats_words(words).tolist())
    assert_stats_identical(st, orc["stats"])


def test_adaptive_full_size_headline_rows_match_oracle(rt, oracle, gpu):
    """Cornell 800x800 spp 256 depth 16 with the reference's adaptive defaults
    (aTolerance 0.05, aBatch 10; src/camera.ts:77-78): the whole frame through
    the rounds, oracle rows bit for bit, and the frame equals the sequential
    kernel's."""
    sd = rt.generate_scene_data({"type": "cornell"})
    ro = {"width": 800, "samples": 256, "depth": 16}
    cam, rgb, rad, st = _render_gpu(rt, sd, ro)
    assert cam.last_kernel() == "pool"
    # round 1 (10 samples) retires 17 % of the pixels, and few carried pixels are likely to
    # converge within a grown round: the round-length rule takes the rest (2 rounds)
    assert cam.adaptive_info()[0] == 2
    W, H = cam.image_width, cam.image_height
    assert st.pixels == W * H and st.samples["min"] < 256 and st.samples["max"] == 256
    for y in (0, 311, 400, 799):
        orc = oracle.render(sd, ro, region=(0, y, W, 1), threads=8)
        assert_identical(rad[y:y + 1], rgb[y:y + 1], orc["radiance"][y:y + 1], orc["rgb"][y:y + 1],
                         f"adaptive cornell 800 row {y}")
    import os
    os.environ["RT_AMD_ADAPT_ROUNDS"] = "0"
    try:
        cam2, rgb2, rad2, st2 = _render_gpu(rt, sd, ro)
    finally:
        del os.environ["RT_AMD_ADAPT_ROUNDS"]
    assert_identical(rad, rgb, rad2, rgb2, "adaptive 800 rounds == sequential")
    assert st.samples == st2.samples and st.bounces == st2.bounces
    # the likely-to-converge arm off (RT_AMD_ADAPT_LIKELY=0): round 1's 17 % keeps the rounds
    # growing x3 - [0, 10), [10, 40), [40, 256) - and the image is the same
    os.environ["RT_AMD_ADAPT_LIKELY"] = "0"
    try:
        cam3, rgb3, rad3, st3 = _render_gpu(rt, sd, ro)
    finally:
        del os.environ["RT_AMD_ADAPT_LIKELY"]
    assert cam3.adaptive_info()[0] == 3
    assert_identical(rad, rgb, rad3, rgb3, "adaptive 800 likely rule off")
    assert st.samples == st3.samples and st.bounces == st3.bounces


# ---------------------------------------------------------------------------
# The camera configurations of the reference's camera.test.ts (defocus, focus
# distance, orientations incl. a view direction parallel to `up`, roulette off /
# early, zero and >1 albedo) through the product path, bit-exact vs the oracle.
# ---------------------------------------------------------------------------
def _cam_scene(albedo=0.5, **cam):
    c = {"vfov": 90, "from": [0, 0, 0], "at": [0, 0, -1], "up": [0, 1, 0],
         "background": {"type": "gradient", "top": [1, 1, 1], "bottom": [0.5, 0.7, 1.0]}}
    c.update(cam)
    return {"camera": c, "materials": [{"id": "m", "material": {"type": "lambert", "color": [albedo] * 3}}],
            "objects": [{"type": "sphere", "pos": [0, 0, -1], "r": 0.5, "material": "m"}]}


CAMERA_CASES = {  # name: (scene kwargs, render options) - camera.test.ts line ranges
    "aperture0": ({"aperture": 0}, {}),                                        # 202-222
    "aperture2_focus1": ({"aperture": 2.0, "focus": 1.0}, {"samples": 10}),    # 224-248
    "auto_focus": ({"from": [0, 0, 3], "at": [0, 0, 0], "aperture": 1.0}, {}),  # 176-187
    "aperture_tiny": ({"aperture": 0.001, "focus": 1.0}, {}),                  # 278-289
    "aperture_large": ({"aperture": 10.0, "focus": 1.0}, {}),                  # 290-300
    "orient_diag": ({"from": [1, 1, 1], "at": [0, 0, 0], "aperture": 1.0}, {}),  # 417-439
    "orient_up_parallel": ({"from": [0, 5, 0], "at": [0, 0, 0], "aperture": 1.0}, {}),
    "roulette_off": ({}, {"roulette": False, "samples": 16}),                  # 592-624
    "roulette_depth2": ({}, {"roulette": True, "rouletteDepth": 2, "samples": 16}),  # 628-654
    "zero_albedo": ({"albedo": 0.0}, {"rouletteDepth": 1}),                    # 658-677
    "high_albedo": ({"albedo": 2.0}, {"rouletteDepth": 1}),                    # 679-698
}


@pytest.mark.parametrize("case", sorted(CAMERA_CASES))
def test_reference_camera_configurations_match_oracle(rt, oracle, gpu, case):
    kw, extra = CAMERA_CASES[case]
    sd = _cam_scene(**kw)
    ro = {"width": 24, "aspect": 1.0, "samples": 4, "depth": 10, **NOADAPT, **extra}
    cam, rgb, rad, st = _render_gpu(rt, sd, ro)
    orc = oracle.render(sd, ro)
    assert_identical(rad, rgb, orc["radiance"], orc["rgb"], f"camera {case} ({cam.last_kernel()})")
    assert_stats_identical(st, orc["stats"])


def _raytracer_test_scene():
    """createTestSceneData of the reference's raytracer.test.ts:7-37."""
    return {"camera": {"vfov": 40, "from": [0, 0, 2], "at": [0, 0, -1], "up": [0, 1, 0],
                       "background": {"type": "gradient", "top": [1, 1, 1], "bottom": [0.5, 0.7, 1.0]}},
            "materials": [{"id": "test-material", "material": {"type": "lambert", "color": [0.7, 0.3, 0.3]}}],
            "objects": [{"type": "sphere", "pos": [0, 0, -1], "r": 0.5, "material": "test-material"}]}


RAYTRACER_CASES = [  # (scene config, generateImageBuffer options, expected size) - raytracer.test.ts
    ({"type": "custom", "render": {"width": 10, "aspect": 1.0, "samples": 1}}, {}, (10, 10)),        # 38-58
    ({"type": "spheres", "render": {"width": 8, "aspect": 2.0, "samples": 1},
      "options": {"count": 5, "seed": 12345}}, {}, (8, 4)),                                          # 60-82
    ({"type": "custom", "render": {"width": 16, "aspect": 1.0, "samples": 1}}, {}, (16, 16)),        # 84-108
    ({"type": "custom", "render": {"width": 20, "aspect": 2.0, "samples": 1}}, {}, (20, 10)),
    ({"type": "custom", "render": {"width": 30, "aspect": 1.5, "samples": 1}}, {}, (30, 20)),
    ({"type": "spheres", "render": {"width": 6, "aspect": 1.0, "samples": 1},
      "options": {"count": 3, "seed": 42}}, {}, (6, 6)),                                             # 110-145
    ({"type": "spheres", "render": {"width": 12, "aspect": 1.0, "samples": 2},
      "options": {"count": 3, "seed": 54321}}, {"parallel": True, "threads": 2}, (12, 12)),          # 147-173
    ({"type": "spheres", "render": {"width": 12, "aspect": 1.0, "samples": 20, "aTolerance": 0.1},
      "options": {"count": 3, "seed": 54321}}, {}, (12, 12)),                                        # 175-
]


@pytest.mark.parametrize("k", range(len(RAYTRACER_CASES)))
def test_reference_raytracer_cases_png_matches_oracle(rt, oracle, gpu, k):
    """generateImageBuffer on the reference's raytracer.test.ts configurations: a PNG of
    the stated size whose pixels are the oracle's render of the same scene, bit for bit."""
    from raytracer_amd.png import decode_png_rgb
    cfg, opts, (W, H) = RAYTRACER_CASES[k]
    cfg = dict(cfg)
    if cfg["type"] == "custom":
        cfg["data"] = _raytracer_test_scene()
        sd = cfg["data"]
    else:
        sd = rt.generate_scene_data({"type": cfg["type"], "options": cfg["options"]})
    png = rt.generate_image_buffer(cfg, opts)
    assert png[:8] == b"\x89PNG\r\n\x1a\n"
    w, h, px = decode_png_rgb(png)
    assert (w, h) == (W, H)
    orc = oracle.render(sd, cfg["render"])
    assert px == np.ascontiguousarray(orc["rgb"]).tobytes()
