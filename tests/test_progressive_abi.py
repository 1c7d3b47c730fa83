"""Progressive rendering, host side: the ABI surface, the argument errors that need no
device, and the checkpoint blob's header parser (rt_progressive_blob_info)."""
import ctypes as C
import re
import struct
from pathlib import Path

import pytest

GOLDEN = Path(__file__).resolve().parent / "golden" / "progressive_spheres500_s20.bin"

SYMBOLS = ["rt_camera_progressive_begin", "rt_camera_progressive_step", "rt_camera_progressive_info",
           "rt_camera_progressive_save", "rt_camera_progressive_restore", "rt_progressive_blob_info",
           "rt_camera_progressive_end"]


def test_progressive_symbols_are_declared_exported_and_bound(rt):
    from raytracer_amd import _lib
    lib = _lib.load()
    text = re.sub(r"\s+", " ", _lib.HEADER.read_text())
    declared = {
        "rt_camera_progressive_begin": "(rt_camera* cam, const rt_region* region)",
        "rt_camera_progressive_step": "(rt_camera* cam, int32_t n_samples, uint8_t* rgb, float* radiance, "
                                      "int32_t* px_samples, int32_t* px_bounces, rt_render_stats* stats)",
        "rt_camera_progressive_info": "(rt_camera* cam, rt_progressive_info* info)",
        "rt_camera_progressive_save": "(rt_camera* cam, uint8_t** blob, size_t* len)",
        "rt_camera_progressive_restore": "(rt_camera* cam, const uint8_t* blob, size_t len)",
        "rt_progressive_blob_info": "(const uint8_t* blob, size_t len, rt_progressive_info* info)",
        "rt_camera_progressive_end": "(rt_camera* cam)",
    }
    assert sorted(declared) == sorted(SYMBOLS)
    for name, args in declared.items():
        assert f"int {name}{args};" in text, f"{name} is not declared as proposed"
        assert hasattr(lib, name), f"{name} is not exported"
        res, argtypes = _lib._SIGS[name]
        assert res is C.c_int and len(argtypes) == args.count(",") + 1
    # rt_progressive_info as the header lays it out: region, 8 x 32 bit, i64, u64, char[24]
    assert C.sizeof(_lib.RtProgressiveInfo) == 16 + 8 * 4 + 8 + 8 + 24
    assert lib.rt_version() == 3


def _camera(rt):
    sd = rt.generate_scene_data({"type": "cornell"})
    return rt.create_camera_from_scene_data(sd, {"width": 16, "samples": 4, "depth": 4})


def test_calls_without_a_session_are_invalid(rt):
    from raytracer_amd import _lib
    from raytracer_amd.camera import ProgressiveRender
    cam = _camera(rt)
    pr = ProgressiveRender(cam)  # a handle with no session behind it
    for call in (lambda: pr.step(1), lambda: pr.samples_done, pr.save):
        with pytest.raises(rt.RtError, match="no progressive session is open") as e:
            call()
        assert e.value.code == _lib.RT_ERR_INVALID
    pr.close()  # ending no session is not an error
    with pytest.raises(ValueError):
        pr.step(1)


def test_begin_rejects_a_region_empty_after_clamping(rt):
    from raytracer_amd import _lib
    cam = _camera(rt)
    for region in [(16, 0, 4, 4), (0, 0, 0, 5), (-8, -8, 8, 8)]:
        with pytest.raises(rt.RtError, match="empty after clamping") as e:
            cam.progressive(region)
        assert e.value.code == _lib.RT_ERR_INVALID


def test_blob_info_rejects_bad_blobs_with_distinct_messages(rt):
    from raytracer_amd import _lib
    msgs = {}
    for what, blob in [("empty", b""), ("garbage", b"not a checkpoint"), ("magic", b"RTPROGXX" + bytes(200))]:
        with pytest.raises(rt.RtError) as e:
            rt.progressive_blob_info(blob)
        assert e.value.code == _lib.RT_ERR_INVALID
        msgs[what] = str(e.value)
    assert "empty" in msgs["empty"] and "truncated" in msgs["garbage"] and "magic" in msgs["magic"]
    assert len(set(msgs.values())) == 3
    cam = _camera(rt)
    with pytest.raises(rt.RtError, match="bad magic") as e:  # validated before any device is touched
        cam.resume(b"RTPROGXX" + bytes(200))
    assert e.value.code == _lib.RT_ERR_INVALID


def test_golden_blob_parses_on_the_host(rt):
    """The checkpoint of the spheres-500 session (48x48, samples 50, aTolerance 0.1) saved
    on an MI355X at samples_done 20: 2304 pixel slots x 48 bytes of state."""
    blob = GOLDEN.read_bytes()
    info = rt.progressive_blob_info(blob)
    assert info["region"] == (0, 0, 48, 48) and (info["width"], info["height"]) == (48, 48)
    assert info["samples_done"] == 20 and info["samples"] == 50 and info["steps"] == 2
    assert info["active_pixels"] == 975 and not info["done"]
    assert info["precision"] == "ref" and info["state_bytes"] == 2304 * 48
    assert len(blob) == 144 + info["state_bytes"]
    # the state is the source of truth: unfinished pixels (bit 31 of n clear) are the active ones
    n = [struct.unpack_from("<I", blob, 144 + 48 * k + 12)[0] for k in range(2304)]
    assert sum(1 for v in n if not v >> 31) == 975 and all(v & 0x7fffffff == 20 for v in n if not v >> 31)
    assert sorted({v & 0x7fffffff for v in n}) == [10, 20]
    # corrupt and truncated blobs are told apart
    flipped = bytearray(blob)
    flipped[144 + 1000] ^= 0x40
    with pytest.raises(rt.RtError, match="corrupt payload"):
        rt.progressive_blob_info(bytes(flipped))
    with pytest.raises(rt.RtError, match="truncated"):
        rt.progressive_blob_info(blob[:-1])
    hdr = bytearray(blob)
    hdr[60] ^= 1  # a header field
    with pytest.raises(rt.RtError, match="corrupt header"):
        rt.progressive_blob_info(bytes(hdr))
