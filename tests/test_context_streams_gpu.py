"""Streams and threads on a camera's device context (include/rt_amd.h, rt_launch: Ordering).

Calls on one camera take effect in the order they were issued, whatever stream each was queued on;
calls on different cameras are independent. Every result here is compared bit for bit with the same
call made alone, synchronously, on the default stream of a fresh camera. The tests pass whether or
not the queued work actually overlaps: they pin the contract, not a race.
"""
import contextlib
import ctypes
import sys
import threading
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import context_cases as cc  # noqa: E402

pytestmark = pytest.mark.gpu

H, W, F = cc.H, cc.W, cc.F
HIP_STREAM_NON_BLOCKING = 1
JOIN_SECONDS = 120


def hip_runtime():
    """The HIP runtime this process has already loaded (the library and torch share it)."""
    paths = [ln.split()[-1] for ln in Path("/proc/self/maps").read_text().splitlines() if "libamdhip64" in ln]
    assert paths, "no HIP runtime is loaded"
    lib = ctypes.CDLL(paths[0])
    for fn in (lib.hipStreamGetFlags, lib.hipStreamCreateWithFlags, lib.hipStreamSynchronize, lib.hipStreamDestroy):
        fn.restype = ctypes.c_int
    return lib


def side_stream():
    """A torch side stream, checked to be non-blocking: the null stream does not wait for it."""
    import torch
    s = torch.cuda.Stream()
    flags = ctypes.c_uint(0xFFFF)
    assert hip_runtime().hipStreamGetFlags(ctypes.c_void_p(s.cuda_stream), ctypes.byref(flags)) == 0
    assert s.cuda_stream != 0 and flags.value & HIP_STREAM_NON_BLOCKING
    return s


class Launch:
    """One rt_camera_render_device into outputs allocated and zeroed on `stream` (None: the default
    stream, synchronous), with the stats words queued right behind it."""

    def __init__(self, cam, stream=None, region=cc.FULL, shape=None, **kw):
        import torch
        h, w = (cam.image_height, cam.image_width)
        shape = shape or (h, w)
        with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
            self.rgb = torch.zeros((*shape, 3), dtype=torch.uint8, device="cuda")
            self.rad = torch.zeros((*shape, 3), dtype=torch.float32, device="cuda")
            self.words = torch.zeros(8, dtype=torch.int64, device="cuda")
        handle = stream.cuda_stream if stream is not None else None
        self.stats, _ = cam.render_device(rgb_ptr=self.rgb.data_ptr(), radiance_ptr=self.rad.data_ptr(), region=region,
                                          stream=handle, synchronize=stream is None, **kw)
        cam.stats_words(self.words.data_ptr(), stream=handle)
        if stream is None:
            torch.cuda.synchronize()

    def result(self):
        """(after a sync of the launch's stream)"""
        return {"rgb": self.rgb.cpu().numpy(), "rad": self.rad.cpu().numpy(), "words": self.words.cpu().numpy()}


def assert_same(got, want, what):
    assert cc.differing(got, want) == [], what


PATHS = {
    # name: (camera, environment, launch options, kernel, passes at least)
    "pool": ("cornell9", {}, {}, "pool", 1),
    "chunked_multipass": ("cornell37", {"RT_AMD_POOL_KERNEL": "0", "RT_AMD_SBUF_MB": "1"}, {}, "chunked", 2),
    "sequential": ("cornell9", {"RT_AMD_CHUNKED": "0"}, {"precision": "fp32"}, "sequential", 1),
    "adaptive": ("adaptive", {}, {}, "pool", 1),
    "spheres_region": ("spheres", {}, {"region": cc.REGION}, "chunked", 1),
}


@pytest.mark.parametrize("path", sorted(PATHS))
def test_side_stream_launch_is_the_default_stream_render(rt, gpu, monkeypatch, path):
    cam_name, env, kw, kernel, passes = PATHS[path]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    solo = Launch(cc.camera(rt, cam_name), **kw)
    assert solo.stats.pixels > 0 and solo.rgb.any()
    s = side_stream()
    cam = cc.camera(rt, cam_name)
    for turn in range(2):  # the second launch reuses the context on the same stream
        side = Launch(cam, s, **kw)
        s.synchronize()
        assert_same(side.result(), solo.result(), f"{path}, launch {turn}")
        assert cam.last_kernel() == kernel and cam.pass_count() >= passes
    assert int(solo.words.cpu()[0]) == solo.stats.pixels


def test_side_stream_packed_tiles_and_unpack(rt, gpu):
    import torch
    from raytracer_amd.distributed import slab_pixels, unpack_tiles
    solo = Launch(cc.camera(rt, "cornell9"), region=cc.REGION)
    s = side_stream()
    cam = cc.camera(rt, "cornell9")
    n = slab_pixels(cc.REGION, 3)
    with torch.cuda.stream(s):
        slabs = torch.zeros((3, n, 3), dtype=torch.uint8, device="cuda")
        rslabs = torch.zeros((3, n, 3), dtype=torch.float32, device="cuda")
        frame = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
        rframe = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
        words = torch.zeros((3, 8), dtype=torch.int64, device="cuda")
    for g in range(3):
        cam.render_device(rgb_ptr=slabs[g].data_ptr(), radiance_ptr=rslabs[g].data_ptr(), region=cc.REGION, tile_group=g,
                          tile_groups=3, packed=True, stream=s.cuda_stream, synchronize=False)
        cam.stats_words(words[g].data_ptr(), stream=s.cuda_stream)
    unpack_tiles(slabs, cc.REGION, W, H, frame, stream=s.cuda_stream)
    unpack_tiles(rslabs, cc.REGION, W, H, rframe, stream=s.cuda_stream)
    s.synchronize()
    want = solo.result()
    assert_same({"rgb": frame.cpu().numpy(), "rad": rframe.cpu().numpy()}, {k: want[k] for k in ("rgb", "rad")}, "unpacked")
    w = words.cpu().numpy()
    assert w[:, 0].sum() == want["words"][0] and w[:, 1].sum() == want["words"][1] and w[:, 4].sum() == want["words"][4]


REGION_B = (20, 30, 40, 33)


def test_back_to_back_launches_on_one_stream(rt, gpu):
    solo_a = Launch(cc.camera(rt, "cornell9"), region=cc.REGION)
    solo_b = Launch(cc.camera(rt, "cornell9"), region=REGION_B, precision="fp32")
    s = side_stream()
    cam = cc.camera(rt, "cornell9")
    a = Launch(cam, s, region=cc.REGION)
    b = Launch(cam, s, region=REGION_B, precision="fp32")  # (no host sync in between)
    s.synchronize()
    assert_same(a.result(), solo_a.result(), "first launch")
    assert_same(b.result(), solo_b.result(), "second launch")
    assert not np.array_equal(solo_a.result()["words"], solo_b.result()["words"])


def test_primary_table_built_on_one_stream_read_on_another(rt, gpu):
    solo = Launch(cc.camera(rt, "cornell37"))
    sa, sb = side_stream(), side_stream()
    cam = cc.camera(rt, "cornell37")
    a = Launch(cam, sa)  # builds the table on sa
    b = Launch(cam, sb)  # no host sync: sb waits for the builder and for the first launch
    sb.synchronize()
    sa.synchronize()
    info = cam.primary_info()
    assert info["built"] and info["used"] and info["build_ms"] > 0
    assert_same(a.result(), solo.result(), "the launch that built the table")
    assert_same(b.result(), solo.result(), "the launch on the other stream")


def test_primary_table_outlives_the_stream_that_built_it(rt, gpu):
    """The context keeps the builder's events, not the caller's stream: after the stream is destroyed
    the table is still read, timed and used."""
    import torch
    hip = hip_runtime()
    solo = Launch(cc.camera(rt, "cornell37"))
    cam = cc.camera(rt, "cornell37")
    raw = ctypes.c_void_p()
    assert hip.hipStreamCreateWithFlags(ctypes.byref(raw), HIP_STREAM_NON_BLOCKING) == 0
    rgb = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    cam.render_device(rgb_ptr=rgb.data_ptr(), stream=raw.value, synchronize=False)
    assert hip.hipStreamSynchronize(raw) == 0
    assert hip.hipStreamDestroy(raw) == 0
    records = cam.primary_table(device=True)
    info = cam.primary_info()
    assert info["built"] and info["used"] and info["build_ms"] > 0
    assert np.array_equal(records, cam.primary_table())
    assert np.array_equal(rgb.cpu().numpy(), solo.result()["rgb"])
    assert_same(Launch(cam).result(), solo.result(), "a default-stream launch afterwards")
    s = side_stream()
    again = Launch(cam, s)
    s.synchronize()
    assert_same(again.result(), solo.result(), "a side-stream launch afterwards")


BIG = {"width": 128, "aspect": 1, "samples": 256, "depth": 8, **cc.NOADAPT}


def _region_call(cam):
    rgb, rad = np.zeros((128, 128, 3), np.uint8), np.zeros((128, 128, 3), F)
    st = cam.render_region(rgb, cc.REGION, radiance=rad)
    return {"rgb": rgb, "rad": rad, "stats": cc.stats_tuple(st), "kernel": cam.last_kernel()}


def _guides_call(cam):
    return cam.render_guides(cc.REGION, through_specular=True)


def _session_call(cam):
    rgb, rad = np.zeros((128, 128, 3), np.uint8), np.zeros((128, 128, 3), F)
    pxs = np.zeros((128, 128), np.int32)
    with cam.progressive(cc.SESSION) as pr:
        st = pr.step(4, rgb, rad, pxs)
        blob = pr.save()
    return {"rgb": rgb, "rad": rad, "pxs": pxs, "stats": cc.stats_tuple(st), "blob": blob}


def test_null_stream_calls_after_an_asynchronous_side_stream_launch(rt, gpu):
    """The launch and the calls behind it share the context's stats words, hand-out counter and
    record buffer: the null-stream entries wait, on the device, for the side stream's launch."""
    def big():
        return cc.camera(rt, "cornell37", **BIG)

    solo = Launch(big())
    want = [f(big()) for f in (_region_call, _guides_call, _session_call)]
    s = side_stream()
    cam = big()
    first = Launch(cam, s)  # asynchronous, not waited for
    got = [f(cam) for f in (_region_call, _guides_call, _session_call)]
    s.synchronize()
    for g, w, what in zip(got, want, ("render_region", "render_guides", "progressive step")):
        assert_same(g, w, what)
    assert_same(first.result(), solo.result(), "the asynchronous launch itself")
    # and the other way round: the side stream's next launch follows the null-stream calls
    second = Launch(cam, s)
    s.synchronize()
    assert_same(second.result(), solo.result(), "a launch after the null-stream calls")


def test_two_cameras_on_two_streams_alternate(rt, gpu):
    names = ("cornell9", "spheres")
    solo = [Launch(cc.camera(rt, n)).result() for n in names]
    streams = [side_stream(), side_stream()]
    cams = [cc.camera(rt, n) for n in names]
    launches = [[], []]
    for _ in range(3):
        for k in (0, 1):
            launches[k].append(Launch(cams[k], streams[k]))
    for s in streams:
        s.synchronize()
    for k in (0, 1):
        for n, launch in enumerate(launches[k]):
            assert_same(launch.result(), solo[k], f"{names[k]}, launch {n}")


def run_threads(targets):
    """Runs the callables on one thread each (at most 4), joins each with a timeout and fails if one
    is still alive or raised; returns their results."""
    assert len(targets) <= 4
    out, errs = [None] * len(targets), []

    def body(k):
        try:
            out[k] = targets[k]()
        except BaseException as e:  # noqa: BLE001 (reported below)
            errs.append((k, repr(e)))

    threads = [threading.Thread(target=body, args=(k,), daemon=True) for k in range(len(targets))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(JOIN_SECONDS)
    assert not [t.name for t in threads if t.is_alive()], "a thread did not finish"
    assert errs == []
    return out


def test_worker_threads_render_bands_of_one_buffer(rt, gpu):
    """The reference's worker model: every worker has its own camera and renders its band of rows
    into the one shared buffer; the merged stats are the single render's."""
    single = cc.camera(rt, "spheres")
    want_rgb, want_rad = cc.frames()
    want = single.render(want_rgb, radiance=want_rad)
    rgb, rad = cc.frames()
    rows = -(-H // 4)
    cams = [cc.camera(rt, "spheres") for _ in range(4)]
    stats = run_threads([lambda k=k: cams[k].render_region(rgb, (0, k * rows, W, rows), radiance=rad) for k in range(4)])
    assert np.array_equal(rgb, want_rgb) and cc.same(rad, want_rad)
    assert cc.stats_tuple(rt.RenderStats.merge(stats)) == cc.stats_tuple(want)
    assert sum(st.pixels for st in stats) == W * H


def test_two_threads_share_one_camera(rt, gpu):
    regions = (cc.REGION, REGION_B)
    want = []
    for r in regions:
        rgb, rad = cc.frames()
        st = cc.camera(rt, "cornell9").render_region(rgb, r, radiance=rad)
        want.append({"rgb": rgb, "rad": rad, "stats": cc.stats_tuple(st)})
    cam = cc.camera(rt, "cornell9")

    def worker(r):
        outs = []
        for _ in range(3):
            rgb, rad = cc.frames()
            st = cam.render_region(rgb, r, radiance=rad)
            outs.append({"rgb": rgb, "rad": rad, "stats": cc.stats_tuple(st)})
        return outs

    for k, outs in enumerate(run_threads([lambda r=r: worker(r) for r in regions])):
        for n, got in enumerate(outs):
            assert_same(got, want[k], f"thread {k}, render {n}")


def test_two_threads_reproject_each_other(rt, gpu):
    prad = cc.seeded(61, H, W, 3)

    def pair():
        return cc.camera(rt, "mirror"), cc.moved_camera(rt, "mirror")

    def call(new, prev):
        wgt = np.zeros((H, W), F)
        hist = new.reproject(prev, prad, region=cc.REGION, weight_out=wgt, guides="specular", through=5)
        return {"history": hist, "weight": wgt}

    a, b = pair()
    want = [call(a, b), call(b, a)]
    a, b = pair()
    got = run_threads([lambda: [call(a, b) for _ in range(3)], lambda: [call(b, a) for _ in range(3)]])
    for k in (0, 1):
        for n, g in enumerate(got[k]):
            assert_same(g, want[k], f"thread {k}, call {n}")
