"""Degenerate and non-finite scenes on the host (CPU; DESIGN.md §2, degenerate_cases.py).

What the library makes of every case without a device - the camera, the effective
traversal (the gate scene_tree.cpp prims_inside_boxes in both directions), the scene blob
and the launch plan - what the oracle renders of it in both precisions, and the inputs that
used to end the process: materials that reach themselves, material chains and JSON nested
deeper than the stack, seeds whose conversion to an integer was undefined.
"""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import degenerate_cases as dc

HERE = Path(__file__).resolve().parent
TRAV = {"fast": 0, "reference": 1, "brute": 2}


# ---------------------------------------------------------------------------
# The camera, the gate, the blob and the plan
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", dc.all_names())
def test_camera_and_effective_traversal(rt, name):
    """Every case creates a camera. A scene the gate must send to the reference walk reports
    traversal 1 whatever is asked for; every other case keeps what was asked for (auto: brute
    force, at most 7 primitives) - the fast paths are not lost silently."""
    sd, ro = dc.case(name)
    forced = dc.effective_traversal(name) == "reference"
    for asked, kept in (("auto", TRAV["brute"]), ("fast", TRAV["fast"]), ("brute", TRAV["brute"]),
                        ("reference", TRAV["reference"])):
        cam = rt.create_camera_from_scene_data(sd, {**ro, "traversal": asked})
        assert cam.info["traversal"] == (TRAV["reference"] if forced else kept), (name, asked)
        assert cam.info["n_objects"] == len(sd["objects"])
        cam.close()


def test_image_sizes_and_loop_counts(rt):
    """What the options cases turn into: image sizes (0x0 and 1x1000 included) and the integer
    loop bounds the kernels run to."""
    def info(name):
        return rt.create_camera_from_scene_data(*dc.case(name)).info
    assert (info("width0")["width"], info("width0")["height"]) == (0, 0)
    assert (info("tall_1x1000")["width"], info("tall_1x1000")["height"]) == (1, 1000)
    assert [info(n)["samples_loop"] for n in ("samples0", "samples2_5", "samples_neg", "samples_nan")] == [0, 3, 0, 0]
    assert [info(n)["depth"] for n in ("depth0", "depth_neg", "depth0_5")] == [0, 0, 1]
    assert [info(n)["roulette_depth"] for n in ("rdepth0", "rdepth_neg")] == [0, 0]
    assert info("rdepth_nan")["roulette_depth"] == 2 ** 31 - 1      # bounces >= NaN never holds
    assert [info(n)["adaptive"] for n in ("abatch0", "abatch_nan", "abatch_neg")] == [1, 1, 1]
    assert [info(n)["adaptive"] for n in ("atol_nan", "atol_inf", "atol_neg")] == [0, 1, 0]
    with pytest.raises(rt.RtError, match="Maximum call stack size exceeded"):
        rt.create_camera_from_scene_data(*dc.case("base", depth=float("nan")))


@pytest.mark.parametrize("name", dc.all_names())
def test_scene_blob_and_launch_plan(rt, name):
    from raytracer_amd import _lib
    sd, ro = dc.case(name)
    cam = rt.create_camera_from_scene_data(sd, ro)
    blob, info = _lib.scene_blob(cam._h)
    assert len(blob) == info["bytes"] > 0
    W, H = cam.image_width, cam.image_height
    for prec in (0, 1):
        plan = _lib.launch_plan(cam._h, (0, 0, W, H), precision=prec)
        assert plan["traversal"] == cam.info["traversal"]
        if W * H:
            assert plan["kernel"] in ("sequential", "chunked", "pool") and plan["grid"] > 0 and plan["passes"] >= 1
        else:  # no pixels: nothing to launch, and no empty grid
            assert (plan["kernel"], plan["grid"], plan["tiles"], plan["passes"]) == ("none", 0, 0, 0)
        if cam.info["traversal"] == TRAV["reference"]:
            assert plan["pool"] == 0 and plan["primary_ok"] == 0    # the pool reads the brute-force layouts
    cam.close()


# ---------------------------------------------------------------------------
# The oracle
# ---------------------------------------------------------------------------
# fp32 oracle against the ref oracle, one sample per pixel, seeds 1 and 77, N = 1536:
# (disagreeing samples, new non-finite samples) as measured. r0_light: the light PDF of a
# point sphere is 0/0 in either precision and the roulette decides on it; huge: 1e30^2
# overflows fp32 and the sphere disappears; light_nonemissive: sampling a lambert sphere as
# a light divides by differences that fp32 rounds to zero.
D_ORC_OUTSIDE = {"r0_light": ((155, 0), (184, 0)), "huge": ((452, 0), (458, 0)),
                 "light_nonemissive": ((61, 29), (54, 22))}


@pytest.mark.parametrize("name", dc.all_names())
def test_oracle_renders_every_case(oracle, name):
    ref = dc.oracle_render(oracle, name)
    f32 = dc.oracle_render(oracle, name, "fp32")
    sd, ro = dc.case(name)
    dm = oracle.dims(sd, ro)
    for o in (ref, f32):
        assert o["radiance"].shape == (dm["height"], dm["width"], 3)
        assert o["stats"]["pixels"] == dm["height"] * dm["width"]
        assert o["stats"]["samples"]["total"] == o["px_samples"].sum()
        assert o["stats"]["bounces"]["total"] == o["px_bounces"].sum()
    if name == "width0":
        assert ref["stats"]["samples"]["total"] == 0 and ref["stats"]["bounces"]["total"] == 0


def test_the_cases_outside_the_fp32_measure_are_the_named_three():
    assert set(D_ORC_OUTSIDE) == set(dc.FP32_OUTSIDE) and len(dc.FP32_OUTSIDE) == 3


@pytest.mark.parametrize("name", dc.scene_names())
def test_fp32_oracle_agrees_with_the_ref_oracle(oracle, name):
    """D_orc is 0 at both seeds for every scene case but the three named ones; those stay at
    or under what was measured."""
    for k, seed in enumerate(dc.SEEDS):
        d, nonfinite = dc.d_orc(oracle, name, seed)
        print(f"degenerate fp32 oracle: {name} seed {seed}: D_orc {d} of {dc.N}, new non-finite {nonfinite}")
        if name in dc.FP32_OUTSIDE:
            assert d <= D_ORC_OUTSIDE[name][k][0] and nonfinite <= D_ORC_OUTSIDE[name][k][1], (name, seed, d)
        else:
            assert d == 0 and nonfinite == 0, (name, seed, d, nonfinite)


# ---------------------------------------------------------------------------
# Inputs that used to end the process (each in a child)
# ---------------------------------------------------------------------------
def _child(kind):
    r = subprocess.run([sys.executable, str(HERE / "degenerate_child.py"), kind], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, (kind, r.returncode, r.stderr[-2000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("kind", ["cycle1", "cycle2", "chain"])
def test_cyclic_and_endless_materials_raise(kind):
    """mixed(a, a) named a; layered a -> mixed b -> a; an acyclic chain of 100 000 ids: the
    reference's RangeError from the library (RtError) and from the oracle in both precisions."""
    res = _child(kind)
    assert res["lib"].startswith("RtError: Maximum call stack size exceeded (material "), res
    for k in ("oracle", "oracle_fp32"):
        assert "Maximum call stack size exceeded" in res[k], res


def test_deep_json_raises_a_parse_error():
    """Arrays and objects nested 100 000 deep, in the scene and in the render options of
    rt_camera_create and in rt_generate_scene_data's options: a parse error naming the
    limit. 200 levels parse."""
    res = _child("deep_json")
    for what in ("arrays", "objects"):
        for entry in ("scene", "options", "generate"):
            msg = res[f"{what} {entry}"]
            assert msg and "JSON parse error at offset" in msg and "nesting deeper than 1000" in msg, (what, entry, msg)
        assert res[f"{what} scene 200"] is None and res[f"{what} generate 200"] is None, res
    assert "nesting deeper than 1000" in res["unclosed"]


def test_json_nesting_limit_is_exactly_1000(rt):
    from raytracer_amd.camera import Camera
    from raytracer_amd import _lib
    sd, ro = dc.case("base")
    text = _lib.to_json(sd).decode()
    for depth, ok in ((999, True), (1000, False)):   # the document's own object is one level
        doc = ('{"junk":' + "[" * depth + "]" * depth + "," + text[1:]).encode()
        if ok:
            Camera(doc, _lib.to_json(ro)).close()
        else:
            with pytest.raises(rt.RtError, match="nesting deeper than 1000"):
                Camera(doc, _lib.to_json(ro))


# ---------------------------------------------------------------------------
# Seeds
# ---------------------------------------------------------------------------
SEEDS = [(1e30, 0), (float("nan"), 0), (float("inf"), 0), (float("-inf"), 0), (2.0 ** 63, 0), (-2.0 ** 63, 0),
         (2 ** 32 + 5, 5), (-1, 2 ** 32 - 1), (1.5, 1), (-1.9, 2 ** 32 - 1), (-0.5, 0), (2 ** 32 - 0.5, 2 ** 32 - 1),
         (-2.0 ** 32, 0), (2.0 ** 31, 2 ** 31), (-2.0 ** 31 - 1, 2 ** 31 - 1), (2.0 ** 53 + 2, 2), (0x5EED, 0x5EED)]


@pytest.mark.parametrize("seed,word", SEEDS)
def test_seed_mapping(rt, oracle, seed, word):
    """RenderOptions.seed -> the RNG's seed word: non-finite -> 0, otherwise truncated towards
    zero, modulo 2^32. The oracle maps the same way: its frame with `seed` is its frame with
    the word."""
    sd, ro = dc.case("base", seed=seed)
    assert rt.create_camera_from_scene_data(sd, ro).info["seed"] == word
    a = oracle.render(sd, {**ro, "width": 16})
    b = oracle.render(sd, {**ro, "width": 16, "seed": word})
    assert np.array_equal(a["radiance"], b["radiance"], equal_nan=True)
    assert np.array_equal(a["px_bounces"], b["px_bounces"])


def test_seed_cases_of_the_table(rt):
    for name, word in dc.SEED_WORDS.items():
        assert rt.create_camera_from_scene_data(*dc.case(name)).info["seed"] == word, name
