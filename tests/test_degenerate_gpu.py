"""Degenerate and non-finite scenes on the GPU (degenerate_cases.py).

Ref precision: every scene, camera and option case against the oracle bit for bit (NaN equal
to NaN) - frames, per-pixel counts and stats through every traversal and path kernel, the
closest hit of hostile rays, the guide buffers. fp32: the three kernels agree with each
other on every case, and every scene case but the three named in degenerate_cases.py stays
under the per-sample measure D_gpu <= 2 D_orc + 0.005 N. Progressive steps of 1 equal the
one-shot frame on a frame with infinities and on a fractional sample count.
"""
import numpy as np
import pytest

import degenerate_cases as dc
import fp32_cases as fc
from denoise_ref import bits_equal, oracle_guides
from guide_walk_ref import guide_walk_ref
from test_fp32_gpu import KERNEL_ENV, _assert_stats_are_the_frames, _render_device, _same
from test_gpu_parity import assert_identical, assert_stats_identical

pytestmark = pytest.mark.gpu

TRAVERSALS = (("auto", "0"), ("fast", "0"), ("fast", "1"), ("brute", "0"), ("reference", "0"))
GUIDE_KEYS = ("normal", "position", "distance", "object", "chain")


def _assert_is_oracle(out, st, orc, what):
    assert out["radiance"].shape == orc["radiance"].shape, what
    assert_identical(out["radiance"], out["rgb"], orc["radiance"], orc["rgb"], what)
    assert np.array_equal(out["px_samples"], orc["px_samples"]), (what, "px_samples")
    assert np.array_equal(out["px_bounces"], orc["px_bounces"]), (what, "px_bounces")
    assert_stats_identical(st, orc["stats"])


# ---------------------------------------------------------------------------
# Ref precision, bit for bit
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", dc.all_names())
def test_ref_matches_oracle_through_every_traversal(rt, oracle, gpu, name, monkeypatch):
    sd, ro = dc.case(name)
    orc = dc.oracle_render(oracle, name)
    for trav, defer in TRAVERSALS:
        monkeypatch.setenv("RT_AMD_DEFER", defer)
        cam, out, st = _render_device(rt, sd, {**ro, "traversal": trav}, precision="ref")
        _assert_is_oracle(out, st, orc, f"{name} {trav} defer {defer} ({cam.last_kernel()})")
        if name == "width0":   # zero pixels, zero stats, nothing launched
            assert (st.pixels, st.samples["total"], st.bounces["total"]) == (0, 0, 0)
            assert cam.last_kernel() == "none" and cam.pass_count() == 0


def _pool_admits(name):
    """The pool kernel's gates (launch_plan.cpp): brute force in effect, no emission stack."""
    return dc.effective_traversal(name) == "asked" and name not in dc.EMISSION_STACK


@pytest.mark.parametrize("name", dc.scene_names())
def test_ref_matches_oracle_through_every_kernel(rt, oracle, gpu, name, monkeypatch):
    sd, ro = dc.case(name)
    orc = dc.oracle_render(oracle, name)
    for kernel, env in KERNEL_ENV.items():
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        cam, out, st = _render_device(rt, sd, {**ro, "traversal": "brute"}, precision="ref")
        expect = kernel if kernel != "pool" or _pool_admits(name) else "chunked"
        assert cam.last_kernel() == expect, (name, kernel, cam.last_kernel())
        _assert_is_oracle(out, st, orc, f"{name} kernel {kernel}")


# ---------------------------------------------------------------------------
# The hit probe
# ---------------------------------------------------------------------------
def probe_rays(name):
    """2000 random rays (an eighth with one zero direction component), 500 aimed within
    +-1e-5 of the added primitive's pos, 16 with direction (0,0,0), 16 with a NaN component
    in origin or direction."""
    rng = np.random.default_rng(31)
    f32 = np.float32
    n = 2000
    o = rng.uniform(-1.5, 1.5, (n, 3)).astype(f32) + f32([0, 0.5, 0])
    d = rng.normal(size=(n, 3)).astype(f32)
    d[: n // 8, rng.integers(0, 3)] = 0
    pos = np.asarray(dc.added_pos(name), np.float64)
    oa = (rng.uniform(-2, 2, (500, 3)) + [0, 1, 2]).astype(f32)
    with np.errstate(invalid="ignore", over="ignore"):
        da = ((pos + rng.uniform(-1e-5, 1e-5, (500, 3))) - oa).astype(f32)
    oz = rng.uniform(-1, 1, (16, 3)).astype(f32)
    dz = np.zeros((16, 3), f32)
    on = rng.uniform(-1, 1, (16, 3)).astype(f32)
    dn = rng.normal(size=(16, 3)).astype(f32)
    on[:8, rng.integers(0, 3, 8)[0]] = np.nan
    dn[8:, rng.integers(0, 3, 8)[0]] = np.nan
    return np.concatenate([o, oa, oz, on]), np.concatenate([d, da, dz, dn])


@pytest.mark.parametrize("name", dc.scene_names())
def test_hit_probe(rt, oracle, gpu, name):
    sd, _ = dc.case(name)
    o, d = probe_rays(name)
    c = oracle.world_hit(sd, o, d)
    cam = rt.create_camera_from_scene_data(sd, {"width": 8})
    po = cam.export()["prim_object"]
    h = c[:, 0] > 0
    print(f"degenerate probe: {name}: {int(h.sum())} of {len(c)} rays hit, "
          f"{int((c[h, 9] >= 3).sum())} the added primitives")
    for trav in ("reference", "fast", "brute"):
        g = cam.debug_world_hit(o, d, traversal=trav)
        assert np.array_equal(g[:, 0], c[:, 0]), (name, trav, int((g[:, 0] != c[:, 0]).sum()))
        assert bits_equal(g[h, 1:9], c[h, 1:9]).all(), (name, trav)
        assert np.array_equal(po[g[h, 9].astype(int)], c[h, 9].astype(int)), (name, trav)
    # fp32: the hard invariants of every record, and the three traversals bitwise equal
    rows = {trav: cam.debug_world_hit(o, d, traversal=trav, precision="fp32") for trav in ("reference", "fast", "brute")}
    g = rows["reference"]
    hf = g[:, 0] > 0
    slot = g[:, 9].astype(int)
    assert np.all((g[:, 0] == 0) | (g[:, 0] == 1))
    assert np.all(g[~hf, 9] == -1)
    assert np.all(np.isfinite(g[hf, 1]) & (g[hf, 1] > np.float32(0.001))), name
    assert np.all((slot[hf] >= 0) & (slot[hf] < len(po))), name
    for trav in ("fast", "brute"):
        differ = int((rows[trav].view(np.uint64) != g.view(np.uint64)).any(axis=1).sum())
        assert differ == 0, (name, trav, differ)


# ---------------------------------------------------------------------------
# Guides
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", dc.scene_names() + dc.camera_names())
def test_guides(rt, oracle, gpu, name):
    sd, ro = dc.case(name)
    cam = rt.create_camera_from_scene_data(sd, ro)
    n, P, dist, obj, _ = oracle_guides(oracle, sd, ro)
    g = cam.render_guides()
    for k, ref in zip(GUIDE_KEYS, (n, P, dist, obj)):
        assert g[k].shape == ref.shape and bits_equal(g[k], ref).all(), (name, "first hit", k)
    walk = guide_walk_ref(oracle, sd, ro)
    gs = cam.render_guides(through_specular=True)
    for k, ref in zip(GUIDE_KEYS, walk):
        bad = int((~bits_equal(gs[k], ref)).reshape(ref.shape[:2] + (-1,)).any(-1).sum())
        assert bad == 0, (name, "through specular", k, bad)


# ---------------------------------------------------------------------------
# fp32
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", dc.all_names())
def test_fp32_kernels_write_identical_frames(rt, gpu, name, monkeypatch):
    """Sequential, chunked and pool kernel in fp32: identical frames, counts and stats.

    Before miss_color spelled |d|^2 out in one order (pt_shade.hpp), the sequential kernel's
    sky pixels left the other two kernels' in the last bit: 13 of 1536 on the base scene, max
    |d| 1.2e-7, none with a black background."""
    sd, ro = dc.case(name)
    runs = {}
    for kernel, env in KERNEL_ENV.items():
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        runs[kernel] = _render_device(rt, sd, ro)
    seq = runs["sequential"]
    if seq[1]["px_samples"].size:
        _assert_stats_are_the_frames(seq[2], seq[1], per_sample_bounces=False)
    else:
        assert (seq[2].pixels, seq[2].samples["total"], seq[2].bounces["total"]) == (0, 0, 0)
    _same(seq, runs["chunked"], f"{name}: chunked vs sequential")
    _same(seq, runs["pool"], f"{name}: pool vs sequential")


@pytest.mark.parametrize("name", [n for n in dc.scene_names() if n not in dc.FP32_OUTSIDE])
def test_fp32_samples_agree_with_the_ref_oracle(rt, oracle, gpu, name):
    for seed in dc.SEEDS:
        sd, ro = dc.sample_case(name, seed)
        ref = dc.oracle_render(oracle, name, samples=1, seed=seed)
        d_orc, _ = dc.d_orc(oracle, name, seed)
        cam, out, st = _render_device(rt, sd, ro)
        d_gpu = fc.disagreeing(out["radiance"], out["px_bounces"], ref)
        print(f"degenerate fp32 per sample: {name} seed {seed}: D_orc {d_orc} D_gpu {d_gpu} N {dc.N} "
              f"(kernel {cam.last_kernel()})")
        assert np.all(out["px_samples"] == 1)
        assert d_gpu <= 2 * d_orc + 0.005 * dc.N, (name, seed, d_gpu, d_orc)
        assert fc.new_nonfinite(out["radiance"], ref["radiance"]) == 0
        _assert_stats_are_the_frames(st, out, per_sample_bounces=True)


@pytest.mark.parametrize("name", dc.FP32_OUTSIDE)
def test_fp32_cases_outside_the_measure_still_render(rt, oracle, gpu, name):
    """The three cases the fp32 oracle itself leaves the ref oracle on: the figure is printed,
    the frame's counts must still add up."""
    for seed in dc.SEEDS:
        sd, ro = dc.sample_case(name, seed)
        ref = dc.oracle_render(oracle, name, samples=1, seed=seed)
        cam, out, st = _render_device(rt, sd, ro)
        print(f"degenerate fp32 per sample (outside the measure): {name} seed {seed}: "
              f"D_orc {dc.d_orc(oracle, name, seed)[0]} D_gpu {fc.disagreeing(out['radiance'], out['px_bounces'], ref)}")
        _assert_stats_are_the_frames(st, out, per_sample_bounces=True)


# ---------------------------------------------------------------------------
# Progressive
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["emit_neg_inf", "samples2_5"])
def test_progressive_steps_of_one_equal_the_one_shot_frame(rt, gpu, name):
    sd, ro = dc.case(name)
    cam = rt.create_camera_from_scene_data(sd, ro)
    H, W = cam.image_height, cam.image_width
    rgb1, rad1 = np.zeros((H, W, 3), np.uint8), np.zeros((H, W, 3), np.float32)
    st1 = cam.render(rgb1, radiance=rad1)
    rgb, rad = np.zeros_like(rgb1), np.zeros_like(rad1)
    pxs, pxb = np.zeros((H, W), np.int32), np.zeros((H, W), np.int32)
    with cam.progressive() as pr:
        steps = 0
        while not pr.done:
            st = pr.step(1, rgb, radiance=rad, px_samples=pxs, px_bounces=pxb)
            steps += 1
            assert steps <= cam.info["samples_loop"]
            if pr.samples_done >= 2:
                var, blob_var = pr.variance(), rt.progressive_blob_variance(pr.save())
                assert bits_equal(var, blob_var).all(), (name, pr.samples_done)
        assert steps == cam.info["samples_loop"] == pr.samples_done
    assert np.array_equal(rgb, rgb1) and bits_equal(rad, rad1).all(), name
    assert (st.pixels, st.samples, st.bounces) == (st1.pixels, st1.samples, st1.bounces)
    assert pxs.sum() == st1.samples["total"] and pxb.sum() == st1.bounces["total"]
