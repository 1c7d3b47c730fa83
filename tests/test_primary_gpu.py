"""The primary-ray candidate table on the device: the builder kernel against the host loop, and
renders with the table (pt_pool_primary_kernel) against renders without it and the oracle."""
import re
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import primary_ref as pr

NOADAPT = {"aTolerance": 0}


def _cornell(rt):
    return rt.generate_scene_data({"type": "cornell"})


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell", "custom"])
def test_device_table_equals_host_table(rt, gpu, name):
    sd, ro, shape = {"cornell": (_cornell(rt), {"width": 40, "samples": 32}, (40, 40)),
                     "custom": (pr.custom_scene(), {"width": 33, "aspect": 2.0, "samples": 32}, (17, 33))}[name]
    cam = rt.create_camera_from_scene_data(sd, {**ro, **NOADAPT})
    host, dev = cam.primary_table(), cam.primary_table(device=True)
    assert host.shape == shape and dev.shape == shape
    n = int((host != dev).sum())
    print(f"{name}: {n} of {host.size} records differ; builder kernel {cam.primary_info()['build_ms']:.4f} ms")
    assert n == 0
    assert (host & np.uint64(0xffff)).any()


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


def _same(a, b, what, stats=True):
    n_rgb = int((a.rgb != b.rgb).any(axis=-1).sum())
    n_rad = int((a.rad.view(np.uint32) != b.rad.view(np.uint32)).any(axis=-1).sum())
    print(f"{what}: pixels differing rgb {n_rgb}, radiance {n_rad} of {a.rgb[..., 0].size}")
    assert n_rgb == 0 and n_rad == 0, what
    assert not stats or a.st.pixels == b.st.pixels and a.st.samples == b.st.samples and a.st.bounces == b.st.bounces, what


def _same_as_oracle(a, orc, what):
    n_rgb = int((a.rgb != orc["rgb"]).any(axis=-1).sum())
    n_rad = int((a.rad.view(np.uint32) != orc["radiance"].view(np.uint32)).any(axis=-1).sum())
    print(f"{what} vs oracle: pixels differing rgb {n_rgb}, radiance {n_rad}")
    assert n_rgb == 0 and n_rad == 0, what
    assert a.st.pixels == orc["stats"]["pixels"], what
    for k in ("total", "min", "max"):
        assert a.st.samples[k] == orc["stats"]["samples"][k] and a.st.bounces[k] == orc["stats"]["bounces"][k], (what, k)


def _on_off(rt, monkeypatch, sd, ro, region=None, kernel="pool"):
    monkeypatch.setenv("RT_AMD_PRIMARY_TABLE", "1")
    on = _render(rt, sd, ro, region)
    assert on.cam.last_kernel() == kernel and on.cam.primary_info()["used"] == (kernel == "pool")
    monkeypatch.setenv("RT_AMD_PRIMARY_TABLE", "0")
    off = _render(rt, sd, ro, region)
    info = off.cam.primary_info()
    assert off.cam.last_kernel() == kernel and not info["used"] and not info["built"]
    monkeypatch.delenv("RT_AMD_PRIMARY_TABLE")
    return on, off


CASES = {
    "cornell-40-spp8": ("cornell", {"width": 40, "samples": 8, "depth": 8, **NOADAPT}, None),
    "cornell-8-spp1": ("cornell", {"width": 8, "samples": 1, "depth": 8, **NOADAPT}, None),   # no jitter branch
    "cornell-8-spp3": ("cornell", {"width": 8, "samples": 3, "depth": 8, **NOADAPT}, None),   # 1-sample items
    "custom-24-spp16": ("custom", {"width": 24, "samples": 16, "depth": 8, **NOADAPT}, None),
    "region": ("cornell", {"width": 40, "samples": 8, "depth": 8, **NOADAPT}, (3, 5, 17, 11)),
    "adaptive-defaults": ("cornell", {"width": 32}, None),  # the reference's adaptive defaults
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_table_on_equals_table_off_equals_oracle(rt, oracle, gpu, monkeypatch, case):
    scene, ro, region = CASES[case]
    sd = _cornell(rt) if scene == "cornell" else pr.custom_scene(pool=True)
    on, off = _on_off(rt, monkeypatch, sd, ro, region)
    _same(on, off, case)
    _same_as_oracle(on, oracle.render(sd, ro, region=region), case)
    if case == "adaptive-defaults":
        assert on.cam.adaptive_info()[0] >= 1  # adaptive rounds on the pool kernel


@pytest.mark.gpu
def test_default_builds_the_table_from_the_threshold(rt, gpu):
    """Without the switch a render uses the table from min_samples samples per pixel on."""
    sd = _cornell(rt)
    n = rt.create_camera_from_scene_data(sd, {"width": 8, **NOADAPT}).primary_info()["min_samples"]
    at = _render(rt, sd, {"width": 16, "samples": n, "depth": 4, **NOADAPT})
    assert at.cam.last_kernel() == "pool" and at.cam.primary_info()["used"] and at.cam.primary_info()["built"]
    if n > 1:
        below = _render(rt, sd, {"width": 16, "samples": n - 1, "depth": 4, **NOADAPT})
        assert below.cam.last_kernel() == "pool" and not below.cam.primary_info()["used"]


@pytest.mark.gpu
def test_tile_group_shares(rt, oracle, gpu, monkeypatch):
    import torch
    sd = _cornell(rt)
    ro = {"width": 40, "samples": 8, "depth": 8, **NOADAPT}
    frames = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("RT_AMD_PRIMARY_TABLE", flag)
        cam = rt.create_camera_from_scene_data(sd, ro)
        H, W = cam.image_height, cam.image_width
        parts, stats = [], []
        for g in range(3):
            rgb = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
            rad = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
            st, _ = cam.render_device(rgb_ptr=rgb.data_ptr(), radiance_ptr=rad.data_ptr(), tile_group=g,
                                      tile_groups=3, synchronize=True)
            assert cam.last_kernel() == "pool" and cam.primary_info()["used"] == (flag == "1")
            parts.append((rgb.cpu().numpy(), rad.cpu().numpy()))
            stats.append((st.pixels, st.samples, st.bounces))
        frames[flag] = (parts, stats)
    monkeypatch.delenv("RT_AMD_PRIMARY_TABLE")
    for g in range(3):
        assert np.array_equal(frames["1"][0][g][0], frames["0"][0][g][0]), g
        assert np.array_equal(frames["1"][0][g][1].view(np.uint32), frames["0"][0][g][1].view(np.uint32)), g
        assert frames["1"][1][g] == frames["0"][1][g], g
    orc = oracle.render(sd, ro)
    rgb = sum(p[0].astype(np.int32) for p in frames["1"][0])  # the shares are disjoint
    rad = sum(p[1] for p in frames["1"][0])
    assert np.array_equal(rgb, orc["rgb"]) and np.array_equal(rad, orc["radiance"])
    assert sum(s[0] for s in frames["1"][1]) == orc["stats"]["pixels"]


@pytest.mark.gpu
def test_fp32_pool_with_table_equals_chunked_kernel(rt, gpu, monkeypatch):
    sd = _cornell(rt)
    ro = {"width": 40, "samples": 8, "depth": 8, "precision": "fp32", **NOADAPT}
    on, off = _on_off(rt, monkeypatch, sd, ro)
    _same(on, off, "fp32 table on / off")
    monkeypatch.setenv("RT_AMD_POOL_KERNEL", "0")
    chunked = _render(rt, sd, ro)
    assert chunked.cam.last_kernel() == "chunked" and not chunked.cam.primary_info()["used"]
    _same(on, chunked, "fp32 pool with table == chunked")


@pytest.mark.gpu
def test_two_step_session_equals_one_shot(rt, gpu, monkeypatch):
    sd = _cornell(rt)
    ro = {"width": 24, "samples": 12, "depth": 8, **NOADAPT}
    monkeypatch.setenv("RT_AMD_PRIMARY_TABLE", "1")
    shot = _render(rt, sd, ro)
    cam = rt.create_camera_from_scene_data(sd, ro)
    H, W = cam.image_height, cam.image_width
    rgb, rad = np.zeros((H, W, 3), np.uint8), np.zeros((H, W, 3), np.float32)
    with cam.progressive() as session:
        for n in (5, 7):
            st = session.step(n, rgb, radiance=rad)
            assert cam.last_kernel() == "pool" and cam.primary_info()["used"]
        assert session.done
    _same(Out(cam, st, rgb, rad), shot, "two steps == one shot")
    monkeypatch.setenv("RT_AMD_PRIMARY_TABLE", "0")
    _same(_render(rt, sd, ro), shot, "table off == one shot")


@pytest.mark.gpu
def test_defocus_camera_renders_as_before(rt, oracle, gpu, monkeypatch):
    sd = _cornell(rt)
    sd["camera"] = {**sd["camera"], "aperture": 0.2, "focus": 4.0}
    ro = {"width": 24, "samples": 16, "depth": 8, **NOADAPT}
    monkeypatch.setenv("RT_AMD_PRIMARY_TABLE", "1")
    out = _render(rt, sd, ro)
    info = out.cam.primary_info()
    assert out.cam.last_kernel() == "pool" and not info["available"] and not info["used"] and not info["built"]
    assert out.cam.primary_table(device=True) is None
    _same_as_oracle(out, oracle.render(sd, ro), "defocus")


def test_primary_kernel_trip_loop_adds_one_wait(rt, tmp_path):
    """test_abi's disassembly count on the new entry: pt_pool_primary_kernel's LDS-resident
    instances have at most one `s_waitcnt vmcnt(0)` more than pt_pool_kernel's of the same
    precision (the wait for the table record, the trip loop's only vector-memory load), and
    stay within the pool kernels' register budget."""
    from raytracer_amd import _lib
    objdump = Path("/opt/rocm/lib/llvm/bin/llvm-objdump")
    if not objdump.exists():
        objdump = Path(shutil.which("llvm-objdump") or "/nonexistent")
    if not objdump.exists():
        pytest.skip("llvm-objdump not found")
    sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tools"))
    import kernel_resources
    counts = {}
    for i, code in enumerate(kernel_resources.code_objects(_lib.LIB_PATH)):
        f = tmp_path / f"co{i}.o"
        f.write_bytes(code)
        text = subprocess.run([str(objdump), "-d", "--no-show-raw-insn", str(f)], check=True,
                              capture_output=True, text=True).stdout
        name = None
        for line in text.splitlines():
            m = re.match(r"^[0-9a-f]+ <_ZN2rt\d+(pt_pool_kernel|pt_pool_primary_kernel)I([df])Li2ELi2E[^>]*>:", line)
            if m:
                name = (m.group(1), m.group(2))
                counts[name] = 0
            elif re.match(r"^[0-9a-f]+ <", line):
                name = None
            elif name and "s_waitcnt vmcnt(0)" in line:
                counts[name] += 1
    print(counts)
    assert len(counts) == 4, counts
    for prec in "df":
        assert counts[("pt_pool_primary_kernel", prec)] <= counts[("pt_pool_kernel", prec)] + 1, counts
    res = kernel_resources.resources(_lib.LIB_PATH, r"pt_pool_primary_kernel")
    assert len(res) == 4
    for k in res:
        assert k["vgpr"] <= 128 and k["scratch"] == 0 and not k["vgpr_spill"], k
