"""The device PNG encoder on the GPU (rt_encode_png_device: png_filter_kernel, png_deflate_kernel,
png_gather_kernel). Every frame of the case table (tests/png_cases.py) and of test_abi.py's
_png_frames: the bytes equal the host run of the same algorithm (rt_debug_png_host) - which
tests/test_png_abi.py pins block by block against restatements and witnesses - and the PNG
decodes to the frame. Every comparison is exact."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import png_cases  # noqa: E402
from test_abi import _png_frames  # noqa: E402

pytestmark = pytest.mark.gpu


def _frames():
    out = {f"{name}/{label}": f for name in png_cases.CASES for label, f in png_cases.frames(name).items()}
    out.update({f"existing/{name}": np.ascontiguousarray(f) for name, f in _png_frames()})
    return out


FRAMES = _frames()


@pytest.fixture(scope="module")
def host(rt):
    """The host run's bytes of every frame, once."""
    from raytracer_amd.png import debug_png_host
    return {k: debug_png_host(f.tobytes(), f.shape[1], f.shape[0]) for k, f in FRAMES.items()}


@pytest.fixture(scope="module")
def device(gpu):
    """Every frame in device memory, once."""
    import torch
    return {k: torch.from_numpy(np.array(f)).cuda().contiguous() for k, f in FRAMES.items()}


def test_device_bytes_equal_the_host_run_on_two_streams(rt, gpu, host, device):
    """Once on the default stream, once on a side stream; the file decodes to the frame."""
    import torch
    from raytracer_amd.png import decode_png_rgb, encode_png_device
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for k, f in FRAMES.items():
        h, w, _ = f.shape
        png = encode_png_device(device[k].data_ptr(), w, h)
        assert png == host[k], k
        assert encode_png_device(device[k].data_ptr(), w, h, stream=side.cuda_stream) == host[k], k
        assert decode_png_rgb(png) == (w, h, f.tobytes()), k


def test_frame_at_an_odd_byte_offset(rt, gpu, host):
    """The frame need not be aligned: it starts 1 (then 3) bytes into a larger buffer whose other
    bytes are 0xA5, and none of those shows in the file."""
    import torch
    from raytracer_amd.png import encode_png_device
    for k, f in FRAMES.items():
        h, w, _ = f.shape
        flat = torch.from_numpy(np.array(f)).reshape(-1)
        for off in (1, 3):
            buf = torch.full((flat.numel() + 64,), 0xA5, dtype=torch.uint8, device="cuda")
            buf[off:off + flat.numel()] = flat.cuda()
            torch.cuda.synchronize()
            assert encode_png_device(buf.data_ptr() + off, w, h) == host[k], (k, off)


def test_back_to_back_on_one_stream(rt, gpu, host, device):
    """Different frames one after the other on one stream - each case after each of its two
    neighbours in the table: a row-filter array or a segment buffer left over from the frame
    before would show in the bytes."""
    import torch
    from raytracer_amd.png import encode_png_device
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    keys = list(FRAMES)
    for k in keys + keys[::-1]:
        h, w, _ = FRAMES[k].shape
        assert encode_png_device(device[k].data_ptr(), w, h, stream=side.cuda_stream) == host[k], k


def test_render_png_of_a_frame_taller_than_256_rows(rt, gpu):
    """cam.render_png and generate_image_buffer on an 8 x 300 Cornell frame (two workgroups of
    png_filter_kernel): the file is the host encoding of the frame a plain render gives."""
    from raytracer_amd.png import debug_png_host, decode_png_rgb
    ro = {"width": 8, "aspect": 8 / 299.5, "samples": 2, "depth": 2, "aTolerance": 0}
    cfg = {"type": "cornell", "render": ro}
    cam = rt.generate_scene(cfg)
    assert (cam.image_width, cam.image_height) == (8, 300)
    rgb = np.zeros((300, 8, 3), np.uint8)
    cam.render(rgb)
    assert len(np.unique(rgb.reshape(-1, 3), axis=0)) > 16       # a picture, not a flat frame
    want = debug_png_host(rgb.tobytes(), 8, 300)
    png, _ = cam.render_png(1)
    assert png == want
    assert decode_png_rgb(png) == (8, 300, rgb.tobytes())
    assert rt.generate_image_buffer(cfg) == want
    assert rt.generate_image_buffer(cfg, {"parallel": True, "threads": 3}) == want
