"""The launch plan and the guided hand-out schedule (launch_plan.cpp plan_launch /
guided_schedule) on the host, no GPU. Every parity test is bit-exact under any schedule, so a
slip in these decisions would change only speed: tests/golden/launch_plans.json pins them, as
recorded from the build before the planner became a unit of its own (a dry run of its launch()),
for an MI355X: 256 compute units, 160 KB of workgroup LDS (profiles/r05/launch_log/)."""
import json
import time
from pathlib import Path

import pytest

GOLDEN = Path(__file__).parent / "golden" / "launch_plans.json"
CUS, LDS_MAX = 256, 163840
ITEM_CAP = (1 << 31) - (1 << 22)  # launch_plan.hpp kItemCap
NOADAPT = {"aTolerance": 0}
ADAPT = {"aTolerance": 0.05, "aBatch": 10}

CORNELL = {"type": "cornell"}
SPHERES500 = {"type": "spheres", "options": {"count": 500, "seed": 42}}
RAIN = {"type": "rain", "options": {"seed": 42}}
SPHERES100K = {"type": "spheres", "options": {"count": 100000, "seed": 42}}
CORNELL_RO = {"width": 800, "samples": 256, "depth": 16}


def _brute17():
    """17 spheres, brute force forced: past kBruteMaxPrims (the in-order loop, no records)."""
    objs = [{"type": "sphere", "pos": [(k % 6) - 2.5, (k // 6) - 1.0, -4.0], "r": 0.4,
             "material": {"type": "lambert", "color": [0.6, 0.6, 0.7]}} for k in range(17)]
    return {"camera": {"vfov": 60, "from": [0, 0, 3], "at": [0, 0, -4], "up": [0, 1, 0],
                       "background": {"type": "gradient", "top": [0.5, 0.7, 1.0], "bottom": [1, 1, 1]}},
            "objects": objs}


def _case(scene, ro, *, size=None, groups=(0, 1), region=None, precision=-1, count=0, env=None, table=False):
    return {"scene": scene, "ro": ro, "size": size, "groups": groups, "region": region, "precision": precision,
            "count": count, "env": env or {}, "table": table}


def _cases():
    c = {}
    for prec, tag in ((-1, "ref"), (1, "fp32")):
        for g, n in ((0, 1), (0, 2), (0, 4), (0, 8)):
            c[f"cornell_{tag}_{g}of{n}"] = _case(CORNELL, {**CORNELL_RO, **NOADAPT}, size=(800, 800), groups=(g, n),
                                                 precision=prec)
    for g, n in ((0, 1), (0, 2), (0, 4), (0, 8)):
        c[f"cornell_adaptive_{g}of{n}"] = _case(CORNELL, {**CORNELL_RO, **ADAPT}, size=(800, 800), groups=(g, n))
    c["cornell_adaptive_count1"] = _case(CORNELL, {**CORNELL_RO, **ADAPT}, count=1)
    c["cornell_spp16"] = _case(CORNELL, {**CORNELL_RO, "samples": 16, **NOADAPT})
    c["cornell_spp16_table"] = _case(CORNELL, {**CORNELL_RO, "samples": 16, **NOADAPT}, table=True)
    sph = {"width": 800, "samples": 64, "depth": 8, "aspect": 1, **NOADAPT}
    c["spheres500_0of1"] = _case(SPHERES500, sph, size=(800, 800))
    c["spheres500_0of8"] = _case(SPHERES500, sph, groups=(0, 8))
    rain = {"width": 1920, "samples": 512, "depth": 16, **NOADAPT}
    c["rain_0of1"] = _case(RAIN, rain, size=(1920, 1080))
    c["rain_0of2"] = _case(RAIN, rain, groups=(0, 2))
    c["spheres100k"] = _case(SPHERES100K, {"width": 2048, "samples": 16, "depth": 8, "aspect": 1, **NOADAPT},
                             size=(2048, 2048))
    c["cornell_reference"] = _case(CORNELL, {**CORNELL_RO, **NOADAPT, "traversal": "reference"})
    c["brute17"] = _case(_brute17(), {"width": 256, "samples": 32, "depth": 8, "traversal": "brute", **NOADAPT})
    # the pool kernel's slot fields: depth <= 250, spp <= 65535
    for depth in (250, 251):
        c[f"cornell_depth{depth}"] = _case(CORNELL, {**CORNELL_RO, **NOADAPT, "depth": depth})
    for spp in (65535, 65536):
        c[f"cornell_spp{spp}"] = _case(CORNELL, {"width": 64, "samples": spp, "depth": 16, **NOADAPT})
    for k, v in (("RT_AMD_POOL_KERNEL", "0"), ("RT_AMD_CHUNKED", "0"), ("RT_AMD_GUIDED", "0"), ("RT_AMD_CHUNK", "64"),
                 ("RT_AMD_SBUF_MB", "64"), ("RT_AMD_LDS_SCENE", "0"), ("RT_AMD_PRIMARY_TABLE", "0"),
                 ("RT_AMD_PRIMARY_TABLE", "1")):
        c[f"cornell_{k}={v}"] = _case(CORNELL, {**CORNELL_RO, **NOADAPT}, env={k: v})
    c["spheres500_RT_AMD_LDS_SCENE=0"] = _case(SPHERES500, sph, env={"RT_AMD_LDS_SCENE": "0"})
    c["cornell_spp16_RT_AMD_PRIMARY_TABLE=1"] = _case(CORNELL, {**CORNELL_RO, "samples": 16, **NOADAPT},
                                                      env={"RT_AMD_PRIMARY_TABLE": "1"})
    c["cornell_empty_region"] = _case(CORNELL, {**CORNELL_RO, **NOADAPT}, region=(10, 10, 0, 0))
    c["cornell_region_outside"] = _case(CORNELL, {**CORNELL_RO, **NOADAPT}, region=(800, 0, 64, 64))
    return c


CASES = _cases()
_SWITCHES = ["RT_AMD_POOL_KERNEL", "RT_AMD_CHUNKED", "RT_AMD_GUIDED", "RT_AMD_CHUNK", "RT_AMD_SBUF_MB",
             "RT_AMD_LDS_SCENE", "RT_AMD_PRIMARY_TABLE", "RT_AMD_POOL", "RT_AMD_REFILL", "RT_AMD_READY",
             "RT_AMD_ADAPT_FIRST", "RT_AMD_ADAPT_ROUNDS", "RT_AMD_REC12", "RT_AMD_DEFER", "RT_AMD_LDS_MATS",
             "RT_AMD_TOP_CACHE", "RT_AMD_NODE_PAD"]
_cameras = {}


def _camera(rt, case):
    """One camera per (scene, options): the 100k-sphere build takes a few seconds."""
    key = json.dumps([case["scene"], case["ro"]], sort_keys=True)
    if key not in _cameras:
        sd = case["scene"] if "objects" in case["scene"] else rt.generate_scene_data(case["scene"])
        t0 = time.perf_counter()
        _cameras[key] = rt.create_camera_from_scene_data(sd, case["ro"])
        print(f"camera built in {time.perf_counter() - t0:.1f} s")
    return _cameras[key]


def plan_of(rt, case, setenv, delenv):
    """The case's plan; setenv / delenv as monkeypatch's (the switches are read per call)."""
    from raytracer_amd import _lib
    for k in _SWITCHES:
        delenv(k, raising=False)
    for k, v in case["env"].items():
        setenv(k, v)
    cam = _camera(rt, case)
    if case["size"]:
        assert (cam.image_width, cam.image_height) == tuple(case["size"])
    region = case["region"] or (0, 0, cam.image_width, cam.image_height)
    return _lib.launch_plan(cam._h, region, case["groups"][0], case["groups"][1], CUS, LDS_MAX, case["precision"],
                            case["count"], case["table"])


def _check_schedule(p):
    """Whatever the fixture says: the phases cover [0, samples) without gap or overlap, chunks
    are powers of two, and a pass numbers fewer than kItemCap items."""
    if p["kernel"] in ("none", "sequential"):
        assert p["n_phases"] == 0
        return
    assert 1 <= p["n_phases"] <= 8
    covered = 0
    for s0, chunk, nch in zip(p["s0"], p["chunk"], p["nch"]):
        assert s0 == covered and nch >= 1
        assert chunk >= 1 and chunk & (chunk - 1) == 0
        covered += chunk * nch
    assert covered == p["samples"]
    assert 1 <= p["pass_units"] <= max(p["tiles"], 1)
    assert p["pass_units"] * 64 * sum(p["nch"]) < ITEM_CAP
    assert p["passes"] == -(-p["tiles"] // p["pass_units"])
    assert p["sb_pool"] % 64 == 0 and 1 <= p["grid"] <= CUS
    if p["kernel"] == "pool":
        assert max(p["chunk"]) <= 128  # kPoolMaxChunk


@pytest.mark.parametrize("name", list(CASES))
def test_launch_plan_matches_the_recorded_plan(rt, monkeypatch, name):
    want = json.loads(GOLDEN.read_text())[name]
    got = plan_of(rt, CASES[name], monkeypatch.setenv, monkeypatch.delenv)
    print(name, got)
    _check_schedule(got)
    for k in sorted(set(got) | set(want)):
        assert got.get(k) == want.get(k), k


def test_hand_out_rules_of_the_design_table(rt, monkeypatch):
    """DESIGN.md §4 'Hand-out rules', pool kernel row: 8 tile-chunks per atomic from 512 samples
    per resident lane, a first chunk of the power-of-two floor of spl / 64, at most 4 - Cornell
    800^2 spp 256: 4 for the whole frame, 2 for a 1/4 share, 1 for a 1/8 share."""
    def plan(n):
        return plan_of(rt, CASES[f"cornell_ref_0of{n}"], monkeypatch.setenv, monkeypatch.delenv)
    whole = plan(1)
    assert whole["kernel"] == "pool" and whole["sb_pool"] == 8 * 64 and whole["chunk"][0] == 4
    assert whole["tiles"] == 100 * 100 and whole["grid"] == CUS and whole["primary_ok"] == 1
    assert plan(4)["chunk"][0] == 2
    assert plan(8)["chunk"][0] == 1


def test_launch_plan_gates(rt, monkeypatch):
    """The decisions stated next to their code: instrumented adaptive launches keep the
    sequential kernel; the primary-ray table is built from 32 samples per pixel and used at any
    count once it exists; the pool kernel's slot fields hold depth <= 250 and spp <= 65535."""
    def plan(name):
        return plan_of(rt, CASES[name], monkeypatch.setenv, monkeypatch.delenv)
    assert plan("cornell_adaptive_count1")["kernel"] == "sequential"
    assert plan("cornell_adaptive_0of1")["kernel"] == "pool"
    assert plan("cornell_spp16")["primary_ok"] == 0 and plan("cornell_spp16_table")["primary_ok"] == 1
    assert plan("cornell_spp16_RT_AMD_PRIMARY_TABLE=1")["primary_ok"] == 1
    assert plan("cornell_RT_AMD_PRIMARY_TABLE=0")["primary_ok"] == 0
    assert plan("cornell_depth250")["kernel"] == "pool" and plan("cornell_depth251")["kernel"] == "chunked"
    assert plan("cornell_spp65535")["kernel"] == "pool" and plan("cornell_spp65536")["kernel"] == "chunked"
    assert plan("cornell_RT_AMD_POOL_KERNEL=0")["kernel"] == "chunked"
    assert plan("cornell_RT_AMD_CHUNKED=0")["kernel"] == "sequential"
    assert plan("cornell_reference")["lds_level"] == 0 and plan("cornell_reference")["kernel"] == "chunked"
    assert plan("cornell_RT_AMD_SBUF_MB=64")["passes"] > 1
    assert plan("spheres500_0of1")["lds_level"] >= 1 and plan("spheres500_RT_AMD_LDS_SCENE=0")["lds_level"] == 0
    assert plan("spheres100k")["lds_level"] == 0 and plan("spheres100k")["n_top"] > 0
    for name in ("cornell_empty_region", "cornell_region_outside"):
        p = plan(name)
        assert p["kernel"] == "none" and p["tiles"] == 0 and p["passes"] == 0


def test_launch_plan_bad_arguments(rt):
    import ctypes
    from raytracer_amd import _lib
    lib = _lib.load()
    cam = _camera(rt, CASES["cornell_spp16"])
    reg, p = _lib.RtRegion(0, 0, 8, 8), _lib.RtLaunchPlan()
    ok = (cam._h, ctypes.byref(reg), 0, 1, CUS, LDS_MAX, -1, 0, ctypes.byref(p))
    assert lib.rt_debug_launch_plan(*ok) == _lib.RT_OK
    for k, bad in ((0, None), (1, None), (8, None), (2, 1), (2, -1), (3, 0), (4, 0), (5, 0), (6, 2), (7, 3), (7, -1)):
        args = list(ok)
        args[k] = bad
        assert lib.rt_debug_launch_plan(*args) == _lib.RT_ERR_INVALID, (k, bad)


_GPU_CASES = {
    "cornell_spp32": (CORNELL, {"width": 64, "samples": 32, "depth": 8, **NOADAPT}, {}),
    "cornell_spp8_sbuf1": (CORNELL, {"width": 64, "samples": 8, "depth": 8, **NOADAPT}, {"RT_AMD_SBUF_MB": "1"}),
    "spheres50": ({"type": "spheres", "options": {"count": 50, "seed": 42}},
                  {"width": 64, "samples": 8, "depth": 8, "aspect": 1, **NOADAPT}, {}),
    "cornell_adaptive": (CORNELL, {"width": 32, "samples": 64, "depth": 8}, {}),  # aTolerance / aBatch defaults
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(_GPU_CASES))
def test_debug_plan_matches_the_launch(rt, gpu, monkeypatch, name):
    """rt_debug_launch_plan against what a render of the same region actually launched: the
    kernel class (rt_camera_last_kernel), the pass count (rt_camera_pass_count; an adaptive
    render's rounds each take the first round's single pass) and whether the pool kernel read
    the primary-ray table (rt_camera_primary_info). MI355X: 256 CUs, 160 KB of LDS."""
    import numpy as np
    from raytracer_amd import _lib
    scene, ro, env = _GPU_CASES[name]
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cam = rt.create_camera_from_scene_data(rt.generate_scene_data(scene), ro)
    try:
        w, h = cam.image_width, cam.image_height
        plan = _lib.launch_plan(cam._h, (0, 0, w, h), 0, 1, CUS, LDS_MAX)  # (a fresh camera: no table yet)
        rgb = np.zeros((h, w, 3), np.uint8)
        cam.render(rgb)
        print(name, plan, cam.last_kernel(), cam.pass_count(), cam.primary_info(), cam.adaptive_info())
        _check_schedule(plan)
        assert plan["kernel"] == cam.last_kernel()
        if name == "cornell_adaptive":
            assert cam.info["adaptive"] and plan["samples"] == 10
            rounds = cam.adaptive_info()[0]
            assert rounds >= 1 and plan["passes"] == 1 and cam.pass_count() == rounds
        else:
            assert plan["passes"] == cam.pass_count()
        assert bool(plan["primary_ok"]) == cam.primary_info()["used"]
    finally:
        cam.close()
