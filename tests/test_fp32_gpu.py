"""fp32 precision mode on the GPU, pinned per sample.

Part A: every case of fp32_cases.py, one sample per pixel, against the ref
oracle with the fp32 oracle's own disagreement as the yardstick:
D_gpu <= 2 * D_orc + 0.005 * N. Part B: fp32 against itself - the three path
kernels and adaptive sampling write identical frames; the traversals are equal where that
holds and under the same measure where it does not. Part C: the fp32 hit probe
(rt_debug_world_hit_fp32) against the oracle's fp32 and fp64 closest hits.
"""
import numpy as np
import pytest

import fp32_cases as fc
from test_gpu_parity import _cfgs, _mixed_scene

pytestmark = pytest.mark.gpu


def _render_device(rt, sd, ro, precision="fp32"):
    """Device render into torch buffers -> (camera, dict of host arrays, RenderStats)."""
    import torch
    cam = rt.create_camera_from_scene_data(sd, {**ro, "precision": precision})
    W, H = cam.image_width, cam.image_height
    rgb = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    rad = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    pxs = torch.full((H, W), -1, dtype=torch.int32, device="cuda")
    pxb = torch.full((H, W), -1, dtype=torch.int32, device="cuda")
    st, _ = cam.render_device(rgb_ptr=rgb.data_ptr(), radiance_ptr=rad.data_ptr(), px_samples_ptr=pxs.data_ptr(),
                              px_bounces_ptr=pxb.data_ptr(), precision=precision, synchronize=True)
    out = {"rgb": rgb.cpu().numpy(), "radiance": rad.cpu().numpy(), "px_samples": pxs.cpu().numpy(),
           "px_bounces": pxb.cpu().numpy()}
    return cam, out, st


def _assert_stats_are_the_frames(st, out, per_sample_bounces):
    """RenderStats = sums, minima and maxima of the returned px_samples / px_bounces.
    bounces min/max are per sample, so they are checked where a pixel is one sample."""
    pxs, pxb = out["px_samples"], out["px_bounces"]
    assert st.pixels == pxs.size
    assert (st.samples["total"], st.samples["min"], st.samples["max"]) == (pxs.sum(), pxs.min(), pxs.max())
    assert st.bounces["total"] == float(pxb.sum())
    if per_sample_bounces:
        assert st.bounces["min"] == float(pxb.min()) and st.bounces["max"] == float(pxb.max())


def _same(a, b, what):
    (ca, oa, sa), (cb, ob, sb) = a, b
    for k in ("rgb", "px_samples", "px_bounces"):
        assert np.array_equal(oa[k], ob[k]), (what, k, int((oa[k] != ob[k]).sum()))
    assert np.array_equal(oa["radiance"], ob["radiance"], equal_nan=True), (what, "radiance")
    assert sa == sb, (what, sa, sb)


# ---------------------------------------------------------------------------
# Part A: per sample against the oracle
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", fc.case_names())
def test_fp32_samples_agree_with_the_ref_oracle(rt, oracle, gpu, name):
    for seed in fc.SEEDS:
        sd, ro = fc.case(name, seed)
        ref, f32 = fc.oracle_pair(oracle, name, seed)
        cam, out, st = _render_device(rt, sd, ro)
        n = ref["px_bounces"].size
        d_orc = fc.disagreeing(f32["radiance"], f32["px_bounces"], ref)
        d_gpu = fc.disagreeing(out["radiance"], out["px_bounces"], ref)
        d_both = fc.disagreeing(out["radiance"], out["px_bounces"], f32)
        print(f"fp32 per sample: {name} seed {seed}: D_orc {d_orc} D_gpu {d_gpu} N {n} "
              f"(GPU vs fp32 oracle {d_both}; kernel {cam.last_kernel()})")
        assert out["radiance"].shape == ref["radiance"].shape and np.all(out["px_samples"] == 1)
        assert d_gpu <= 2 * d_orc + 0.005 * n, (name, seed, d_gpu, d_orc, n)
        assert fc.new_nonfinite(out["radiance"], ref["radiance"]) == 0
        _assert_stats_are_the_frames(st, out, per_sample_bounces=True)


# ---------------------------------------------------------------------------
# Part B: fp32 against itself
# ---------------------------------------------------------------------------
KERNEL_ENV = {"sequential": {"RT_AMD_CHUNKED": "0"},
              "chunked": {"RT_AMD_CHUNKED": "1", "RT_AMD_POOL_KERNEL": "0"},
              "pool": {"RT_AMD_CHUNKED": "1", "RT_AMD_POOL_KERNEL": "1"}}


def _kernel_scene(rt, name):
    """(SceneData, RenderOptions, whether the pool kernel's gates admit it)."""
    if name == "spheres500":
        cfg, ro = _cfgs()["spheres"]
        return rt.generate_scene_data(cfg), ro, False     # 500 primitives: no brute force
    if name == "rain":
        cfg, ro = _cfgs()["rain"]
        return rt.generate_scene_data(cfg), ro, False
    if name == "mixed-scene":
        return _mixed_scene(), {"depth": 10}, False          # an emissive mixture: emission stack
    return fc.matrix_scene("mixed", "quad"), {"depth": 12}, True


def _with_kernel(rt, monkeypatch, kernel, sd, ro, expect):
    for k, v in KERNEL_ENV[kernel].items():
        monkeypatch.setenv(k, v)
    r = _render_device(rt, sd, ro)
    assert r[0].last_kernel() == expect, (kernel, r[0].last_kernel())
    return r


@pytest.mark.parametrize("name", ["spheres500", "rain", "mixed-scene", "matrix-plane"])
def test_fp32_kernels_write_identical_frames(rt, gpu, name, monkeypatch):
    """Sequential, chunked and pool kernel in fp32: identical u8, radiance, per-pixel
    counts and stats, at a width with partial tiles and an odd sample count."""
    sd, ro, pool = _kernel_scene(rt, name)
    ro = {**ro, "width": 72, "samples": 9, "aTolerance": 0}
    if pool or name == "mixed-scene":
        ro["traversal"] = "brute"
    seq = _with_kernel(rt, monkeypatch, "sequential", sd, ro, "sequential")
    _assert_stats_are_the_frames(seq[2], seq[1], per_sample_bounces=False)
    _same(seq, _with_kernel(rt, monkeypatch, "chunked", sd, ro, "chunked"), f"{name}: chunked vs sequential")
    # where a gate keeps the pool kernel out, asking for it must leave the chunked kernel's frame
    _same(seq, _with_kernel(rt, monkeypatch, "pool", sd, ro, "pool" if pool else "chunked"),
          f"{name}: pool vs sequential")


@pytest.mark.parametrize("name", ["cornell", "spheres", "rain", "default"])
def test_fp32_traversals(rt, oracle, gpu, name, monkeypatch):
    """The traversal values in fp32. README's "all returning the same hits" is a promise of
    reference precision: in fp32 the fast walk's frames leave the reference walk's in the last
    bit of a few pixels (spheres-500: 71 of 9216 pixels, rain: 51 of 5184, no bounce count
    differs; Cornell and default: none), although the three walks
    return bitwise equal hits for the same ray (test_fp32_hit_probe_traversals_agree): a
    product is contracted differently where the path code is inlined into the fast kernels.
    So what holds is asserted as equality - brute force equals the reference walk, the fast
    walk is the same with and without deferred exact tests - and the fast walk is held to the
    per-sample measure: against the reference walk (same bounce counts, channels within
    1e-4 + 1e-4|c| on all but 0.5 % of pixels) and, one sample per pixel, every traversal
    against the ref oracle under D_gpu <= 2 D_orc + 0.005 N."""
    cfg, ro = _cfgs()[name]
    sd = rt.generate_scene_data(cfg)
    ro = {**ro, "width": 96, "samples": 8}
    runs = [("reference", "0"), ("fast", "0"), ("fast", "1"), ("brute", "0")]
    outs = {}
    for trav, defer in runs:
        monkeypatch.setenv("RT_AMD_DEFER", defer)
        outs[trav, defer] = _render_device(rt, sd, {**ro, "traversal": trav})
    base = outs["reference", "0"]
    for key, r in outs.items():
        a, b = r[1]["radiance"], base[1]["radiance"]
        n = int((~((a == b) | (np.isnan(a) & np.isnan(b)))).any(axis=-1).sum())
        print(f"fp32 traversals: {name} {key}: {n} pixels differ from the reference traversal")
    _same(base, outs["brute", "0"], f"{name}: brute vs reference")
    _same(outs["fast", "0"], outs["fast", "1"], f"{name}: fast, deferred vs immediate exact tests")
    fast = outs["fast", "0"][1]
    assert np.array_equal(fast["px_bounces"], base[1]["px_bounces"]) and outs["fast", "0"][2].bounces == base[2].bounces
    away = int((~fc.agree(fast["radiance"], fast["px_bounces"], base[1]["radiance"], base[1]["px_bounces"])).sum())
    assert away <= 0.005 * fast["px_bounces"].size, (name, away)
    # one sample per pixel: every traversal against the ref oracle
    ro1 = {**ro, "samples": 1, "seed": fc.SEEDS[0]}
    ref = oracle.render(sd, ro1, threads=8)
    f32 = oracle.render(sd, ro1, precision="fp32", threads=8)
    n = ref["px_bounces"].size
    d_orc = fc.disagreeing(f32["radiance"], f32["px_bounces"], ref)
    for trav, defer in runs:
        monkeypatch.setenv("RT_AMD_DEFER", defer)
        _, out, _ = _render_device(rt, sd, {**ro1, "traversal": trav})
        d_gpu = fc.disagreeing(out["radiance"], out["px_bounces"], ref)
        print(f"fp32 traversals per sample: {name} {trav} defer {defer}: D_orc {d_orc} D_gpu {d_gpu} N {n}")
        assert d_gpu <= 2 * d_orc + 0.005 * n, (name, trav, defer, d_gpu, d_orc, n)


def test_fp32_adaptive_is_the_same_through_every_kernel(rt, oracle, gpu, monkeypatch):
    """Default adaptive options in fp32: the three kernels agree bit for bit, some
    pixels converge early, and a pixel whose samples all agree with the ref oracle's
    stops at the ref oracle's sample count. Whether a pixel's samples agree is decided
    from a fixed 60-sample pair of frames: the summed bounce counts equal and the mean
    within the per-sample tolerance (the renders return sums over a pixel's samples,
    not each sample)."""
    sd = rt.generate_scene_data({"type": "cornell"})
    ro = {"width": 40, "samples": 60, "depth": 8, "traversal": "brute"}
    seq = _with_kernel(rt, monkeypatch, "sequential", sd, ro, "sequential")
    _same(seq, _with_kernel(rt, monkeypatch, "chunked", sd, ro, "chunked"), "adaptive: chunked vs sequential")
    _same(seq, _with_kernel(rt, monkeypatch, "pool", sd, ro, "pool"), "adaptive: pool vs sequential")
    st, out = seq[2], seq[1]
    assert st.samples["min"] < 60
    _assert_stats_are_the_frames(st, out, per_sample_bounces=False)
    fixed = {**ro, "aTolerance": 0}
    ref_fixed = oracle.render(sd, fixed, threads=8)
    _, gpu_fixed, _ = _render_device(rt, sd, fixed)
    same_paths = fc.agree(gpu_fixed["radiance"], gpu_fixed["px_bounces"], ref_fixed["radiance"],
                          ref_fixed["px_bounces"])
    ref = oracle.render(sd, ro, threads=8)
    differ = out["px_samples"] != ref["px_samples"]
    print(f"fp32 adaptive: {int(same_paths.sum())} of {same_paths.size} pixels with all 60 samples agreeing, "
          f"px_samples differs on {int(differ.sum())} pixels, {int((differ & same_paths).sum())} of them agreeing")
    assert same_paths.mean() > 0.5
    assert not (differ & same_paths).any()


# ---------------------------------------------------------------------------
# Part C: the fp32 hit probe
# ---------------------------------------------------------------------------
_PROBE_GPU = {}


def _probe_gpu(rt, oracle, name):
    """(camera, {family: fp32 probe rows through the camera's traversal}), once per scene."""
    if name not in _PROBE_GPU:
        sd, rays, _, _ = fc.probe_reference(oracle, name)
        cam = rt.create_camera_from_scene_data(sd, {"width": 8})
        _PROBE_GPU[name] = (cam, {f: cam.debug_world_hit(*rays[f], precision="fp32") for f in fc.FAMILIES})
    return _PROBE_GPU[name]


@pytest.mark.parametrize("name", fc.PROBE_SCENES)
def test_fp32_hit_probe(rt, oracle, gpu, name):
    """rt_debug_world_hit_fp32 on random, axis-parallel, on-surface, grazing, inside and
    edge rays: hard invariants of every reported hit (t, slot, side), the hit point on the
    reported primitive as closely as the fp32 oracle's, agreement with the fp64 oracle as
    often as the fp32 oracle's (per ray family)."""
    sd, rays, ref, f32 = fc.probe_reference(oracle, name)
    cam, rows = _probe_gpu(rt, oracle, name)
    po = cam.export()["prim_object"]
    res_gpu, res_orc = [], []
    for fam in fc.FAMILIES:
        o, d = rays[fam]
        g = rows[fam]
        h = g[:, 0] > 0
        slot = g[:, 9].astype(int)
        # hard invariants
        assert np.all((g[:, 0] == 0) | (g[:, 0] == 1))
        assert np.all(g[~h, 9] == -1)
        assert np.all(np.isfinite(g[h, 1]) & (g[h, 1] > np.float32(0.001))), (name, fam)
        assert np.all((slot[h] >= 0) & (slot[h] < len(po))), (name, fam)
        obj = np.where(h, po[np.clip(slot, 0, len(po) - 1)], -1)
        o64, d64 = o.astype(np.float64), d.astype(np.float64)
        for k in np.flatnonzero(h):
            ob = sd["objects"][int(obj[k])]
            if ob["type"] == "sphere":
                n_out = (o64[k] + g[k, 1] * d64[k] - np.asarray(ob["pos"], float)) / ob["r"]
            else:
                n_out = np.cross(np.asarray(ob["u"], float), np.asarray(ob["v"], float))
                n_out /= np.linalg.norm(n_out)
            dn = d64[k] @ n_out
            if abs(dn) > 1e-5 * np.linalg.norm(d64[k]):
                assert bool(g[k, 8]) == (dn <= 0), (name, fam, k, dn)
        # the hit point on the reported primitive
        res_gpu.append(fc.hit_residual(sd, o, d, g, obj))
        res_orc.append(fc.hit_residual(sd, o, d, f32[fam], f32[fam][:, 9]))
        # agreement with the fp64 oracle
        n = len(g)
        d_gpu = int((~fc.hits_agree(g, obj, ref[fam])).sum())
        d_orc = int((~fc.hits_agree(f32[fam], f32[fam][:, 9], ref[fam])).sum())
        print(f"fp32 probe: {name} {fam}: D_orc {d_orc} D_gpu {d_gpu} N {n} ({int(h.sum())} hits)")
        assert d_gpu <= 2 * d_orc + 0.005 * n, (name, fam, d_gpu, d_orc, n)
    q_gpu = float(np.nanpercentile(np.concatenate(res_gpu), 99.9))
    q_orc = float(np.nanpercentile(np.concatenate(res_orc), 99.9))
    print(f"fp32 probe: {name}: residual p99.9 GPU {q_gpu:.3g}, fp32 oracle {q_orc:.3g}")
    assert q_gpu <= 4 * q_orc, (name, q_gpu, q_orc)


@pytest.mark.parametrize("name", fc.PROBE_SCENES)
def test_fp32_hit_probe_traversals_agree(rt, oracle, gpu, name):
    """The three traversals return bitwise equal fp32 hit records."""
    _, rays, _, _ = fc.probe_reference(oracle, name)
    cam, rows = _probe_gpu(rt, oracle, name)
    for fam in fc.FAMILIES:
        for trav in ("reference", "fast", "brute"):
            gt = cam.debug_world_hit(*rays[fam], traversal=trav, precision="fp32")
            differ = int((gt.view(np.uint64) != rows[fam].view(np.uint64)).any(axis=1).sum())
            print(f"fp32 probe: {name} {fam}: traversal {trav} differs from the camera's on {differ} rays")
            assert differ == 0, (name, fam, trav, differ)


@pytest.mark.parametrize("name", fc.PROBE_SCENES)
def test_fp32_hit_probe_normals_have_unit_length(rt, oracle, gpu, name):
    """Every reported normal has | |n|^2 - 1 | <= 1e-5.

    The reference's sphere normal is (p - c) / r with p = o + t d. Evaluated in fp32 it is
    off unit length by up to 5e-4 on spheres-200 and 1.6e-5 on default (the fp32 oracle's
    figures, printed beside the GPU's; the fp64 oracle stays within 5e-6), so the fp32 build
    normalises it (pt_shade.hpp sphere_normal): measured 3e-7 at most on every ray here."""
    _, _, _, f32 = fc.probe_reference(oracle, name)
    _, rows = _probe_gpu(rt, oracle, name)
    worst = {}
    for fam in fc.FAMILIES:
        g, c = rows[fam], f32[fam]
        dev = np.abs((g[g[:, 0] > 0, 5:8] ** 2).sum(-1) - 1)
        dev_orc = np.abs((c[c[:, 0] > 0, 5:8] ** 2).sum(-1) - 1)
        worst[fam] = float(dev.max())
        print(f"fp32 probe: {name} {fam}: max | |n|^2 - 1 | GPU {dev.max():.3g} ({int((dev > 1e-5).sum())} above "
              f"1e-5), fp32 oracle {dev_orc.max():.3g} ({int((dev_orc > 1e-5).sum())} above)")
    assert max(worst.values()) <= 1e-5, (name, worst)
