"""The scene blob (scene_blob.cpp build_scene_blob) on the host, no GPU: its bytes, length and
section offsets against tests/golden/blob_scenes.json, recorded from the build before the blob
builder became a unit of its own, plus the structural facts the layout promises."""
import hashlib
import json
from pathlib import Path

import pytest

from test_gpu_parity import _pair_scene

# (not scene_*.json: test_golden.py takes every such file for a generated scene)
GOLDEN = Path(__file__).parent / "golden" / "blob_scenes.json"
RO = {"width": 64, "samples": 4, "depth": 8, "aTolerance": 0}

CASES = {
    "cornell": lambda rt: rt.generate_scene_data({"type": "cornell"}),
    "spheres10": lambda rt: rt.generate_scene_data({"type": "spheres", "options": {"count": 10, "seed": 42}}),
    "spheres500": lambda rt: rt.generate_scene_data({"type": "spheres", "options": {"count": 500, "seed": 42}}),
    "rain50": lambda rt: rt.generate_scene_data({"type": "rain", "options": {"count": 50, "seed": 42}}),
    "default": lambda rt: rt.generate_scene_data({"type": "default"}),  # plane, layered, glass, sphere light, aperture
    "pairs16": lambda rt: _pair_scene(),  # spheres, axis quads of every code, an odd one out, a tilted quad, a plane
    "spheres5000": lambda rt: rt.generate_scene_data({"type": "spheres", "options": {"count": 5000, "seed": 42}}),  # tsph2, LDS level 0
}


def blob_record(rt, name):
    """What the fixture stores of a case: sha256, length and every info field."""
    from raytracer_amd import _lib
    cam = rt.create_camera_from_scene_data(CASES[name](rt), RO)
    try:
        data, info = _lib.scene_blob(cam._h)
    finally:
        cam.close()
    return {"sha256": hashlib.sha256(data).hexdigest(), "length": len(data), "info": info}


@pytest.mark.parametrize("name", list(CASES))
def test_scene_blob_matches_the_recorded_bytes(rt, name):
    want = json.loads(GOLDEN.read_text())[name]
    got = blob_record(rt, name)
    info = got["info"]
    print(name, got)
    assert got["length"] == want["length"] == info["bytes"]
    assert info == want["info"]
    assert got["sha256"] == want["sha256"]
    # the layout's promises (scene_blob.hpp): 16-byte sections, the two LDS prefixes end where
    # the materials / the reference nodes begin
    offs = {k: v for k, v in info.items() if k.startswith("off_")}
    assert len(offs) == 10
    for k, v in offs.items():
        assert v % 16 == 0 or (k == "off_tsph2" and v == -1), k
    assert info["bytes"] % 16 == 0
    assert info["lds_words"] * 16 == info["off_mats"]
    assert info["lds_words2"] * 16 == info["off_nodes"]
    if name == "cornell":
        assert info["n_pre"] == 5  # 8 primitives in 5 pre-filter records
    if name == "spheres5000":
        assert info["off_tsph2"] > info["off_pre"]  # leaf records of a tree walked from global memory


def test_scene_blob_size_query_and_capacity(rt):
    import ctypes
    from raytracer_amd import _lib
    lib = _lib.load()
    cam = rt.create_camera_from_scene_data(CASES["cornell"](rt), RO)
    try:
        info = _lib.RtSceneBlobInfo()
        assert lib.rt_debug_scene_blob(cam._h, None, 0, ctypes.byref(info)) == _lib.RT_OK and info.bytes > 0
        small = ctypes.create_string_buffer(16)
        assert lib.rt_debug_scene_blob(cam._h, small, 16, ctypes.byref(info)) == _lib.RT_ERR_INVALID
        assert lib.rt_debug_scene_blob(cam._h, None, 0, None) == _lib.RT_ERR_INVALID
        assert lib.rt_debug_scene_blob(None, None, 0, ctypes.byref(info)) == _lib.RT_ERR_INVALID
    finally:
        cam.close()
