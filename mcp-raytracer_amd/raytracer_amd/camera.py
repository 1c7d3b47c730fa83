"""Camera: the reference's Camera surface over the HIP path tracer.

Mirrors src/camera.ts (RenderOptions 42-52, RenderRegion 54-59,
renderRegion 388-431, render 439-446) and RenderStats
(src/render-utils/renderStats.ts:6-64). A Camera is created by
create_camera_from_scene_data (scenes.py), exactly like the reference.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field
from typing import Iterable, Optional, Sequence

from . import _lib
from .passes import (_as_frame, _denoise_out, _f32_frame, _f32_outs, _gather_options, _guide_options, _hold_entry,
                     _host_ptr,
                     _region, _region_ptr, _reproject_frames, _reproject_options, _session_frame, _session_result,
                     _temporal_options, _var_call, _var_out, _view_dict)
from .passes import _c_view  # noqa: F401  (callers that imported it from this module still find it)

RENDER_MODES = ("default", "bounces", "samples")


def _mm(total=0.0, mn=math.inf, mx=0.0, avg=0.0):
    return {"total": total, "min": mn, "max": mx, "avg": avg}


@dataclass
class RenderStats:
    """RenderStats (src/render-utils/renderStats.ts:6-64)."""

    pixels: float = 0
    samples: dict = field(default_factory=_mm)
    bounces: dict = field(default_factory=_mm)

    @classmethod
    def _from_c(cls, s: _lib.RtRenderStats) -> "RenderStats":
        return cls(pixels=s.pixels,
                   samples=_mm(s.samples_total, s.samples_min, s.samples_max, s.samples_avg),
                   bounces=_mm(s.bounces_total, s.bounces_min, s.bounces_max, s.bounces_avg))

    @staticmethod
    def merge(stats: Iterable["RenderStats"]) -> "RenderStats":
        """RenderStats.merge (renderStats.ts:42-64)."""
        m = RenderStats()
        for st in stats:
            m.pixels += st.pixels
            m.samples["total"] += st.samples["total"]
            m.samples["min"] = min(m.samples["min"], st.samples["min"])
            m.samples["max"] = max(m.samples["max"], st.samples["max"])
            m.bounces["total"] += st.bounces["total"]
            m.bounces["min"] = min(m.bounces["min"], st.bounces["min"])
            m.bounces["max"] = max(m.bounces["max"], st.bounces["max"])
        if m.pixels > 0:
            m.samples["avg"] = m.samples["total"] / m.pixels
        if m.samples["total"] > 0:
            m.bounces["avg"] = m.bounces["total"] / m.samples["total"]
        return m


class History:
    """A view history (rt_history_*): per pixel the accumulated radiance, the effective number of
    samples behind it and the variance of the accumulated mean's illuminance, kept on the device
    and carried from view to view by ProgressiveRender.accumulated. It owns its buffers: the
    cameras it was fed from may be closed, and Camera.release_device does not free it. Use as a
    context manager, or close() it."""

    def __init__(self):
        self._lib = _lib.load()
        h = C.c_void_p()
        _lib.check(self._lib.rt_history_create(C.byref(h)))
        self._h = h

    def _handle(self):
        if not getattr(self, "_h", None):
            raise ValueError("the history is closed")
        return self._h

    @property
    def info(self) -> dict:
        """rt_history_get_info: {"width", "height", "region", "views", "device", "scene_hash",
        "bytes", "view"} of the last committed view (views 0, device -1: empty)."""
        i = _lib.RtHistoryInfo()
        _lib.check(self._lib.rt_history_get_info(self._handle(), C.byref(i)))
        return {"width": int(i.width), "height": int(i.height),
                "region": (int(i.region.x), int(i.region.y), int(i.region.width), int(i.region.height)),
                "views": int(i.views), "device": int(i.device), "scene_hash": int(i.scene_hash), "bytes": int(i.bytes),
                "view": _view_dict(i.view)}

    @property
    def views(self) -> int:
        return self.info["views"]

    @property
    def chain_guides(self) -> Optional[dict]:
        """rt_history_chain_guides: None, or {"max_bounces", "max_fuzz"} of the chain planes the last
        committed view holds (a commit of ProgressiveRender.accumulated(guides=...))."""
        go, held = _lib.RtGuideOptions(), C.c_int32(0)
        _lib.check(self._lib.rt_history_chain_guides(self._handle(), C.byref(go), C.byref(held)))
        return {"max_bounces": int(go.max_bounces), "max_fuzz": float(go.max_fuzz)} if held.value else None

    def read(self) -> dict:
        """rt_history_read: {"radiance": float32 (H, W, 3), "variance", "length": float32 (H, W)} in
        the history's own full-frame layout, zero outside its region."""
        import numpy as np
        i = self.info
        H, W = i["height"], i["width"]
        out = {"radiance": np.zeros((H, W, 3), np.float32), "variance": np.zeros((H, W), np.float32),
               "length": np.zeros((H, W), np.float32)}
        _lib.check(self._lib.rt_history_read(self._handle(), out["radiance"].ctypes.data, out["variance"].ctypes.data,
                                             out["length"].ctypes.data))
        return out

    def times(self) -> dict:
        """Device time of the last ProgressiveRender.accumulated call, from HIP events
        (rt_history_times): guide + variance passes, the gather kernel, the filter, the whole span."""
        g, k, f, t = C.c_float(), C.c_float(), C.c_float(), C.c_float()
        _lib.check(self._lib.rt_history_times(self._handle(), C.byref(g), C.byref(k), C.byref(f), C.byref(t)))
        return {"guide_ms": float(g.value), "gather_ms": float(k.value), "filter_ms": float(f.value),
                "total_ms": float(t.value)}

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.rt_history_destroy(self._h)
            self._h = None

    def __enter__(self) -> "History":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Camera:
    """The reference Camera (src/camera.ts:61-472), rendering on MI355X."""

    channels = 3

    def __init__(self, scene_json: bytes, render_options_json: Optional[bytes]):
        lib = _lib.load()
        h = C.c_void_p()
        _lib.check(lib.rt_camera_create(scene_json, render_options_json, C.byref(h)))
        self._h = h
        self._lib = lib
        info = _lib.RtCameraInfo()
        _lib.check(lib.rt_camera_get_info(self._h, C.byref(info)))
        self._info = info

    # -- properties named as in the reference -------------------------------
    @property
    def image_width(self) -> int:
        return self._info.width

    @property
    def image_height(self) -> int:
        return self._info.height

    imageWidth = image_width
    imageHeight = image_height

    @property
    def info(self) -> dict:
        i = self._info
        return {f: getattr(i, f) for f, _ in _lib.RtCameraInfo._fields_}

    @property
    def precision(self) -> str:
        return "fp32" if self._info.precision == 1 else "ref"

    def set_precision(self, precision: str) -> None:
        _lib.check(self._lib.rt_camera_set_precision(self._h, _lib.PRECISION[precision]))
        self._info.precision = _lib.PRECISION[precision]

    @property
    def byte_length(self) -> int:
        return self.image_width * self.image_height * self.channels

    # -- rendering -----------------------------------------------------------
    def render_region(self, buffer, region, radiance=None) -> RenderStats:
        """Camera.renderRegion(buffer, region): writes the region's pixels of
        the full-frame RGB buffer (W*H*3 bytes) and returns RenderStats.
        `radiance` (optional float32 W*H*3) receives the final pixel colours."""
        ptr, _keep = _host_ptr(buffer, self.byte_length, "buffer")
        rptr, _keep2 = _host_ptr(radiance, self.byte_length * 4, "radiance")
        st = _lib.RtRenderStats()
        reg = _region(region)
        _lib.check(self._lib.rt_camera_render_region(self._h, C.byref(reg), ptr, rptr, C.byref(st)))
        return RenderStats._from_c(st)

    def render(self, buffer, radiance=None) -> RenderStats:
        """Camera.render(pixelData) (src/camera.ts:439-446)."""
        return self.render_region(buffer, (0, 0, self.image_width, self.image_height), radiance)

    renderRegion = render_region

    def render_png(self, bands: int = 1):
        """generateImageBuffer's core on the device (rt_camera_render_png): the frame
        rendered in one launch (`bands`, the reference's worker count, changes neither
        the image nor the merged stats), PNG encoded on the GPU -> (png bytes, RenderStats)."""
        out, n = C.c_void_p(), C.c_size_t()
        st = _lib.RtRenderStats()
        _lib.check(self._lib.rt_camera_render_png(self._h, int(bands), C.byref(st), C.byref(out), C.byref(n)))
        try:
            return C.string_at(out, n.value), RenderStats._from_c(st)
        finally:
            self._lib.rt_free(out)

    def render_region_multi(self, buffer, region, devices, radiance=None) -> RenderStats:
        """Camera.renderRegion over several GPUs from this one process (rt_camera_render_multi):
        the region's 8x8 tiles dealt round-robin over `devices` (HIP ordinals; one may repeat
        to rehearse the split on fewer GPUs), gathered on devices[0] over RCCL, stats merged as
        RenderStats.merge. Same buffers and result as render_region, bit for bit."""
        ptr, _keep = _host_ptr(buffer, self.byte_length, "buffer")
        rptr, _keep2 = _host_ptr(radiance, self.byte_length * 4, "radiance")
        devs = (C.c_int32 * len(devices))(*[int(d) for d in devices])
        st = _lib.RtRenderStats()
        reg = _region(region)
        _lib.check(self._lib.rt_camera_render_multi(self._h, devs, len(devices), C.byref(reg), ptr, rptr, C.byref(st)))
        return RenderStats._from_c(st)

    def render_multi(self, buffer, devices, radiance=None) -> RenderStats:
        """Camera.render over several GPUs (render_region_multi of the whole image)."""
        return self.render_region_multi(buffer, (0, 0, self.image_width, self.image_height), devices, radiance)

    renderRegionMulti = render_region_multi

    def render_png_multi(self, devices):
        """generateImageBuffer over several GPUs (rt_camera_render_png_multi): the frame gathered on
        devices[0], PNG encoded there -> (png bytes, merged RenderStats)."""
        devs = (C.c_int32 * len(devices))(*[int(d) for d in devices])
        out, n = C.c_void_p(), C.c_size_t()
        st = _lib.RtRenderStats()
        _lib.check(self._lib.rt_camera_render_png_multi(self._h, devs, len(devices), C.byref(st), C.byref(out),
                                                        C.byref(n)))
        try:
            return C.string_at(out, n.value), RenderStats._from_c(st)
        finally:
            self._lib.rt_free(out)

    def multi_info(self) -> dict:
        """The last multi-GPU render (rt_camera_multi_info): devices, transport, per-device
        path / accumulate ms and the root's gather ms (waits for their events)."""
        i = _lib.RtMultiInfo()
        _lib.check(self._lib.rt_camera_multi_info(self._h, C.byref(i)))
        n = i.n_devices
        return {"n_devices": n, "transport": _lib.GATHER.get(i.transport, "none") if n else "none",
                "devices": list(i.devices)[:n], "path_ms": list(i.path_ms)[:n], "accum_ms": list(i.accum_ms)[:n],
                "gather_ms": float(i.gather_ms), "slab_tiles": i.plan.slab_tiles, "tiles": i.plan.tiles}

    def render_device(self, *, rgb_ptr=None, radiance_ptr=None, region=None, tile_group=0, tile_groups=1,
                      precision: Optional[str] = None, stream=None, synchronize=False, count_work=False,
                      px_samples_ptr=None, px_bounces_ptr=None, traversal: Optional[str] = None,
                      packed: bool = False):
        """Device-resident render into caller-owned device buffers (full-frame
        layout, or with `packed` the tile-packed slab layout of rt_launch).
        Returns (RenderStats|None, work_counters|None)."""
        if region is None:
            region = (0, 0, self.image_width, self.image_height)
        L = _lib.RtLaunch()
        L.region = _region(region)
        L.tile_group, L.tile_groups = int(tile_group), int(tile_groups)
        L.precision = -1 if precision is None else _lib.PRECISION[precision]
        L.traversal = -1 if traversal is None else _lib.TRAVERSAL[traversal]
        # count_work: False/True (work counters) or "profile" (section timing, diagnostic)
        L.count_work = 2 if count_work == "profile" else (1 if count_work else 0)
        L.rgb = rgb_ptr
        L.radiance = radiance_ptr
        L.px_samples = px_samples_ptr
        L.px_bounces = px_bounces_ptr
        L.stream = stream
        L.synchronize = 1 if synchronize else 0
        L.packed_tiles = 1 if packed else 0
        st = _lib.RtRenderStats()
        cnt = (C.c_uint64 * _lib.COUNTER_WORDS)()
        _lib.check(self._lib.rt_camera_render_device(self._h, C.byref(L), C.byref(st), cnt))
        if not synchronize:
            return None, None
        if count_work == "profile":
            base = len(_lib.CT_NAMES)
            counters = {k: int(cnt[base + i]) for i, k in enumerate(_lib.PR_NAMES)}
            nl = _lib.PR_NAMES.index("loop")
            lb = base + len(_lib.PR_NAMES)
            for i, k in enumerate(_lib.PR_NAMES[:nl]):
                counters[f"lanes_{k}"] = int(cnt[lb + i])
                counters[f"execs_{k}"] = int(cnt[lb + nl + i])
        else:
            counters = dict(zip(_lib.CT_NAMES, [int(v) for v in cnt])) if count_work else None
        return RenderStats._from_c(st), counters

    def kernel_times(self):
        """(path_ms, accum_ms) of the last render call, from HIP events on its stream."""
        a, b = C.c_float(), C.c_float()
        _lib.check(self._lib.rt_camera_kernel_times(self._h, C.byref(a), C.byref(b)))
        return float(a.value), float(b.value)

    def stats_words(self, dst_ptr: int, stream=None) -> None:
        """Queue a copy of the last render's 8 RenderStats words (u64) to the
        device address `dst_ptr` on `stream` (rt_camera_stats_words)."""
        _lib.check(self._lib.rt_camera_stats_words(self._h, C.c_void_p(dst_ptr), C.c_void_p(stream)))

    def adaptive_info(self):
        """(rounds, samples rendered) of the last render's adaptive rounds
        (rt_camera_adaptive_info); (0, 0) when it was not adaptive or ran sequentially."""
        r, n = C.c_int32(), C.c_uint64()
        _lib.check(self._lib.rt_camera_adaptive_info(self._h, C.byref(r), C.byref(n)))
        return int(r.value), int(n.value)

    def pass_count(self) -> int:
        """Chunked-kernel passes of the last render (rt_camera_pass_count)."""
        n = C.c_int32()
        _lib.check(self._lib.rt_camera_pass_count(self._h, C.byref(n)))
        return int(n.value)

    KERNELS = ("none", "sequential", "chunked", "pool")

    def last_kernel(self) -> str:
        """Path kernel of the last render (rt_camera_last_kernel): 'sequential',
        'chunked' or 'pool' ('none' before any)."""
        n = C.c_int32()
        _lib.check(self._lib.rt_camera_last_kernel(self._h, C.byref(n)))
        return self.KERNELS[int(n.value)]

    # -- the primary-ray candidate table --------------------------------------------
    def primary_table(self, device: bool = False):
        """The pool kernel's primary-ray candidate table (rt_camera_primary_table): a uint64
        (height, width) array, one record per pixel - candidate mask (bits 0-15), nearest
        candidate's slot (16-19) and fp16 bound (32-47), the other candidates' shared fp16
        bound (48-63). Evaluated on the host; `device=True` returns the records the current
        device built. None when the camera has no table (defocus, more than 16 primitives, or
        a traversal other than brute force)."""
        import numpy as np
        w, h = self.info["width"], self.info["height"]
        out = np.zeros((h, w), np.uint64)
        fn = self._lib.rt_camera_primary_table_device if device else self._lib.rt_camera_primary_table
        code = fn(self._h, out.ctypes.data, int(out.size))
        if code == _lib.RT_PRIMARY_TABLE_NONE:
            return None
        _lib.check(code)
        return out

    def primary_info(self) -> dict:
        """rt_camera_primary_info: {"available": the camera qualifies for the table, "used": the
        last render's pool kernel read it, "built": the device holds it, "min_samples": samples
        per pixel from which a render builds it, "build_ms": the builder kernel's device time}."""
        i = _lib.RtPrimaryInfo()
        _lib.check(self._lib.rt_camera_primary_info(self._h, C.byref(i)))
        return {"available": bool(i.available), "used": bool(i.used), "built": bool(i.built),
                "min_samples": int(i.min_samples), "build_ms": float(i.build_ms)}

    # -- progressive rendering -------------------------------------------------
    def progressive(self, region=None) -> "ProgressiveRender":
        """Open a progressive session over `region` (default: the whole image) at zero
        samples (rt_camera_progressive_begin). A camera holds one session: opening
        another drops the first."""
        _lib.check(self._lib.rt_camera_progressive_begin(self._h, _region_ptr(region)))
        return ProgressiveRender(self)

    def resume(self, blob: bytes) -> "ProgressiveRender":
        """Open a session from ProgressiveRender.save()'s blob (rt_camera_progressive_restore).
        Raises RtError naming the first mismatch when the blob is truncated or corrupt or was
        saved by a camera with another scene, options, image size, precision or library build."""
        blob = bytes(blob)
        _lib.check(self._lib.rt_camera_progressive_restore(self._h, blob, len(blob)))
        return ProgressiveRender(self)

    # -- guides and the denoised preview ------------------------------------------
    def render_guides(self, region=None, *, through_specular=False, max_bounces=8, max_fuzz=0.0) -> dict:
        """First-hit guide buffers (rt_camera_render_guides): one deterministic pinhole primary
        ray per pixel of `region` (default: the whole image). Returns full-frame arrays
        {"normal": float32 (H, W, 3), "position": float32 (H, W, 3), "distance": float32 (H, W),
        "object": int32 (H, W): index in SceneData.objects, -1 on a miss}; pixels outside the
        region hold zeros (object -1).

        `through_specular=True` (rt_camera_render_guides_ex, RT_GUIDES_SPECULAR) follows mirrors
        (metals of fuzz <= max_fuzz) and glass for up to `max_bounces` continuations to the first
        surface that is not specular: the same four arrays, the distance summed along the chain,
        and "chain": int32 (H, W) = continuations | end code << 8 (0 miss, 1 terminal surface,
        2 the chain left the scene, 3 max_bounces reached), zero outside the region. Equals
        tests/guide_walk_ref.py in every bit."""
        import numpy as np
        H, W = self.image_height, self.image_width
        g = {"normal": np.zeros((H, W, 3), np.float32), "position": np.zeros((H, W, 3), np.float32),
             "distance": np.zeros((H, W), np.float32), "object": np.full((H, W), -1, np.int32)}
        rptr = _region_ptr(region)
        if through_specular:
            g["chain"] = np.zeros((H, W), np.int32)
            opts = _lib.RtGuideOptions(_lib.GUIDES_SPECULAR, int(max_bounces), float(max_fuzz))
            _lib.check(self._lib.rt_camera_render_guides_ex(self._h, rptr, C.byref(opts), g["normal"].ctypes.data,
                                                            g["position"].ctypes.data, g["distance"].ctypes.data,
                                                            g["object"].ctypes.data, g["chain"].ctypes.data))
        else:
            _lib.check(self._lib.rt_camera_render_guides(self._h, rptr, g["normal"].ctypes.data,
                                                         g["position"].ctypes.data, g["distance"].ctypes.data,
                                                         g["object"].ctypes.data))
        return g

    def render_coverage(self, region=None, k: int = 2) -> dict:
        """Sub-pixel coverage (rt_camera_render_coverage): k x k deterministic pinhole primary rays
        per pixel of `region` (default: the whole image), k 2 or 4, compared with the pixel's own
        centre ray - the one render_guides traces. Returns full-frame arrays {"agree": uint16
        (H, W), bit b*k + a set when sub-ray (a, b) shows the centre ray's object (a miss equals a
        miss), "objects": uint8 (H, W), the number of distinct objects among the sub-rays and the
        centre, "mixed": bool (H, W), a bit of the low k*k is clear}; pixels outside the region
        hold zeros (not mixed). Pinhole rays whatever the camera's aperture, reference precision
        whatever its precision. Equals tests/coverage_ref.py in every bit."""
        import numpy as np
        H, W = self.image_height, self.image_width
        words = np.zeros((H, W), np.uint32)
        _lib.check(self._lib.rt_camera_render_coverage(self._h, _region_ptr(region), int(k), words.ctypes.data))
        full = np.uint32((1 << (int(k) * int(k))) - 1)
        inside = np.zeros((H, W), bool)
        if region is None:
            inside[:] = True
        else:
            r = _region(region)
            inside[max(r.y, 0):max(r.y + r.height, 0), max(r.x, 0):max(r.x + r.width, 0)] = True
        return {"agree": (words & np.uint32(0xffff)).astype(np.uint16), "objects": ((words >> 16) & 0xff).astype(np.uint8),
                "mixed": inside & ((words & full) != full)}

    def coverage_time(self) -> float:
        """Device time in ms of the camera's last coverage pass - render_coverage, or the first
        hold_edges call of a frame or session (rt_camera_coverage_time), from HIP events."""
        ms = C.c_float()
        _lib.check(self._lib.rt_camera_coverage_time(self._h, C.byref(ms)))
        return float(ms.value)

    def _set_denoise_guides(self, guides) -> None:
        opts = _guide_options(guides)
        _lib.check(self._lib.rt_camera_set_denoise_guides(self._h, C.byref(opts)))

    def denoise(self, radiance, region=None, *, levels=4, sigma_color=None, sigma_plane=0.01, rgb=None, out=None,
                variance=None, sigma_variance=2.0, variance_out=None, guides="first_hit", hold_edges=0):
        """rt_camera_denoise: the a-trous filter of a frame of this camera (float32 (H, W, 3), as
        render_region's `radiance`), its guides computed on the device. Returns the filtered
        radiance (H, W, 3) - a new array, or `out` (which may be `radiance` itself); `rgb`
        (optional u8 W*H*3) receives the region's u8. Equals denoise(radiance,
        **render_guides(region), region=region, ...). `variance` (float32 (H, W)), `sigma_variance`
        and `variance_out` select the variance-guided filter (rt_camera_denoise_variance) as in
        denoise(). `guides` selects the guides the call computes (rt_camera_set_denoise_guides):
        "first_hit", "specular" - those of render_guides(through_specular=True) - or a dict of
        max_bounces / max_fuzz for the latter. `hold_edges` (0, 2 or 4; rt_camera_denoise_hold,
        rt_camera_denoise_variance_hold) copies the pixels render_coverage(region, k=hold_edges)
        calls mixed through unfiltered - colour, u8 and variance_out are their inputs - while they
        still serve as taps: the switch that makes the filter safe on sky-lit scenes with sub-pixel
        geometry, at the price of still-noisy edge pixels indoors. The mask is always first-hit and
        pinhole, whatever `guides` is. 0 is the call without it, byte for byte."""
        H, W = self.image_height, self.image_width
        self._set_denoise_guides(guides)
        rad = _f32_frame(radiance, (H, W, 3), "radiance")
        res = _denoise_out(rad, out)
        uptr, _k = _host_ptr(rgb, self.byte_length, "rgb")
        rptr = _region_ptr(region)
        guided, opts = _var_call(variance, sigma_color, sigma_variance, variance_out, levels, sigma_plane)
        if guided:
            var = _f32_frame(variance, (H, W), "variance")
            fn, *hold = _hold_entry(self._lib, "rt_camera_denoise_variance", hold_edges)
            _lib.check(fn(self._h, rptr, C.byref(opts), *hold, rad.ctypes.data, var.ctypes.data, res.ctypes.data,
                          _var_out(variance_out, (H, W)), uptr))
        else:
            fn, *hold = _hold_entry(self._lib, "rt_camera_denoise", hold_edges)
            _lib.check(fn(self._h, rptr, C.byref(opts), *hold, rad.ctypes.data, res.ctypes.data, uptr))
        return _as_frame(res, H, W)

    def denoise_times(self) -> dict:
        """Device time of the last denoise / ProgressiveRender.denoised call, from HIP events
        (rt_camera_denoise_times): guide pass ms (0 when a session reused its guides), ms of each
        level, and the whole span guide pass .. filtered frame."""
        n, g, t = C.c_int32(), C.c_float(), C.c_float()
        lv = (C.c_float * _lib.DENOISE_MAX_LEVELS)()
        _lib.check(self._lib.rt_camera_denoise_times(self._h, C.byref(n), C.byref(g), lv, C.byref(t)))
        return {"levels": int(n.value), "guide_ms": float(g.value), "level_ms": [float(v) for v in lv][:n.value],
                "total_ms": float(t.value)}

    # -- reprojection of a previous view's frame -------------------------------------
    def view(self) -> dict:
        """The camera's view (rt_camera_get_view): {"center", "pixel00", "du", "dv": float32 (3,),
        "width", "height"} - the fp32 vectors the guide pass builds its rays from."""
        v = _lib.RtView()
        _lib.check(self._lib.rt_camera_get_view(self._h, C.byref(v)))
        return _view_dict(v)

    def reusable_objects(self):
        """rt_camera_reusable_objects: uint8 per SceneData.objects entry, 1 where the object's
        resolved material is lambert or light - the surfaces whose radiance another view may reuse."""
        import numpy as np
        out = np.zeros(max(self._info.n_objects, 1), np.uint8)
        _lib.check(self._lib.rt_camera_reusable_objects(self._h, out.ctypes.data, int(out.size)))
        return out[:self._info.n_objects]

    def through_objects(self, mask: int = 15, max_fuzz: float = 0.0):
        """rt_camera_through_objects: uint8 per SceneData.objects entry, 1 where the object's resolved
        material class is in `mask` (1 a metal of fuzz <= max_fuzz, 2 glass, 4 mixed, 8 layered) -
        the surfaces a reprojection through specular chains may start a chain on."""
        import numpy as np
        out = np.zeros(max(self._info.n_objects, 1), np.uint8)
        _lib.check(self._lib.rt_camera_through_objects(self._h, int(mask), float(max_fuzz), out.ctypes.data,
                                                       int(out.size)))
        return out[:self._info.n_objects]

    def reproject(self, prev_cam: "Camera", prev_radiance, region=None, prev_region=None, radiance=None,
                  px_samples=None, samples=None, rgb=None, out=None, history_out=None, weight_out=None, *,
                  normal_min=0.9, sigma_plane=0.01, min_weight=0.25, history_samples=32.0, guides=None,
                  point_pixels=4.0, through=15, kind=None):
        """rt_camera_reproject: `prev_radiance` (float32 (Hp, Wp, 3), a frame of `prev_cam`, a camera
        of the same scene) reprojected into this camera's view; both views' guides are computed on
        the device. With a fresh `radiance` of this camera and its sample counts (`px_samples`
        int32 (H, W), or one scalar `samples`) returns the blend (H, W, 3) - a new array, or `out` -
        and `rgb` receives its u8; without, returns the history. `history_out` / `weight_out` are
        optional float32 arrays; only the region is written. Equals reproject(prev_radiance,
        prev_cam.view(), prev_cam.render_guides(), reusable=self.reusable_objects(),
        **self.render_guides(), ...). The result can be fed to denoise() and chained as the next
        call's prev_radiance.

        `guides="specular"` (or a dict of max_bounces / max_fuzz) runs rt_camera_reproject_specular
        instead: pixels that show a lambert or light surface through mirrors or glass find their
        history at the chain's virtual point, within `point_pixels` footprints, where the chain
        starts on an object of `through_objects(through, max_fuzz)`; `kind` (optional uint8 (H, W))
        receives 0 no history, 1 first hit, 2 chain. Equals reproject_specular() on both cameras'
        guides. Without `guides=` the three keywords must be left alone."""
        H, W = self.image_height, self.image_width
        prad = _f32_frame(prev_radiance, (prev_cam.image_height, prev_cam.image_width, 3), "prev_radiance")
        args, res, _keep = _reproject_frames(H, W, radiance, px_samples, samples, rgb, out, history_out, weight_out)
        rptr, pptr = _region_ptr(region), _region_ptr(prev_region)
        go, opts, *kptr = _gather_options(guides, _reproject_options(normal_min, sigma_plane, min_weight, history_samples),
                                          _lib.RtSpecularReprojectOptions, point_pixels, through, kind, (H, W))
        if go is None:
            _lib.check(self._lib.rt_camera_reproject(self._h, rptr, prev_cam._h, pptr, C.byref(opts), prad.ctypes.data,
                                                     *args))
        else:
            _lib.check(self._lib.rt_camera_reproject_specular(self._h, rptr, prev_cam._h, pptr, C.byref(go),
                                                              C.byref(opts), prad.ctypes.data, *args, *kptr))
        return res

    def reproject_times(self) -> dict:
        """Device time of the last reproject / ProgressiveRender.reprojected call, from HIP events
        (rt_camera_reproject_times): the guide passes, the gather kernel and the whole span."""
        g, r, t = C.c_float(), C.c_float(), C.c_float()
        _lib.check(self._lib.rt_camera_reproject_times(self._h, C.byref(g), C.byref(r), C.byref(t)))
        return {"guide_ms": float(g.value), "reproject_ms": float(r.value), "total_ms": float(t.value)}

    def release_device(self) -> None:
        """Free the device copies; the next render re-creates them (rt_camera_release_device)."""
        _lib.check(self._lib.rt_camera_release_device(self._h))

    # -- introspection (tests) -----------------------------------------------
    def export(self):
        """Host copies of the flattened scene as numpy structured arrays."""
        import numpy as np
        i = self._info
        nodes = np.zeros(i.n_nodes, dtype=NODE_DTYPE)
        prims = np.zeros(i.n_objects, dtype=PRIM_DTYPE)
        mats = np.zeros(i.n_materials, dtype=MAT_DTYPE)
        lights = np.zeros(i.n_lights, dtype=LIGHT_DTYPE)
        prim_object = np.zeros(i.n_objects, dtype=np.int32)
        _lib.check(self._lib.rt_camera_export(self._h, nodes.ctypes.data, prims.ctypes.data, mats.ctypes.data,
                                              lights.ctypes.data if i.n_lights else None,
                                              prim_object.ctypes.data))
        return {"nodes": nodes, "prims": prims, "materials": mats, "lights": lights, "prim_object": prim_object}

    def debug_world_hit(self, origins, directions, traversal: Optional[str] = None, precision: str = "ref"):
        """Closest hit of rays through the device BVH, in ref precision or through the fp32
        build (rt_debug_world_hit_fp32): rows of {hit, t, p.xyz, n.xyz, front, prim slot}."""
        import numpy as np
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(directions, dtype=np.float32).reshape(-1, 3)
        out = np.zeros((o.shape[0], 10), dtype=np.float64)
        tr = -1 if traversal is None else _lib.TRAVERSAL[traversal]
        fn = self._lib.rt_debug_world_hit_fp32 if _lib.PRECISION[precision] == 1 else self._lib.rt_debug_world_hit
        _lib.check(fn(self._h, tr, o.shape[0], o.ctypes.data, d.ctypes.data, out.ctypes.data))
        return out

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.rt_camera_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ProgressiveRender:
    """A progressive session of a Camera (rt_camera_progressive_*): the region rendered a few
    samples at a time, every step returning the whole region's frame - finished pixels final,
    the others previewed from the samples they have. The frame at samples_done == s is the
    one-shot frame of the same camera with `samples: s`, bit for bit, however the steps were
    cut. Use as a context manager, or close() it."""

    def __init__(self, camera: Camera):
        self._cam = camera

    def _info(self) -> _lib.RtProgressiveInfo:
        if self._cam is None:
            raise ValueError("the progressive session is closed")
        info = _lib.RtProgressiveInfo()
        _lib.check(self._cam._lib.rt_camera_progressive_info(self._cam._h, C.byref(info)))
        return info

    def step(self, n: int, buffer=None, radiance=None, px_samples=None, px_bounces=None) -> RenderStats:
        """Render the next `n` samples (clamped to the camera's `samples`) of every pixel still
        sampling. `buffer` (u8 W*H*3), `radiance` (float32 W*H*3), `px_samples` / `px_bounces`
        (int32 W*H) are optional caller-owned full-frame buffers; only the region is written.
        Returns the RenderStats of the region's frame so far."""
        if self._cam is None:
            raise ValueError("the progressive session is closed")
        cam = self._cam
        px = cam.image_width * cam.image_height
        ptr, _k0 = _host_ptr(buffer, cam.byte_length, "buffer")
        rptr, _k1 = _host_ptr(radiance, cam.byte_length * 4, "radiance")
        sptr, _k2 = _host_ptr(px_samples, px * 4, "px_samples")
        bptr, _k3 = _host_ptr(px_bounces, px * 4, "px_bounces")
        st = _lib.RtRenderStats()
        _lib.check(cam._lib.rt_camera_progressive_step(cam._h, int(n), ptr, rptr, sptr, bptr, C.byref(st)))
        return RenderStats._from_c(st)

    def focus(self, n: int, buffer=None, radiance=None, px_samples=None, px_bounces=None, selected=None, *,
              score=None, permille=250, min_score=0.0, max_pixels=0) -> RenderStats:
        """A focused step (rt_camera_progressive_focus): `n` further samples for the noisiest of the
        pixels still sampling only. `score` ranks them: None - the session's own variance (needs
        samples_done >= 2); a float32 array, (H, W) or region-shaped - e.g. a `variance_out` of
        denoised(variance=True); or an rt.History - its variance plane (its last committed region
        and image size must be the session's). Scores that are not (>= 0 and finite) count as 0;
        the pixels with score > `min_score` are eligible, and those at or above the K-th largest
        eligible score are selected, ties included: K = ceil(active_pixels * permille / 1000),
        capped by `max_pixels` when > 0. They render sample indices from samples + the session's
        focus cursor on, so samples_done does not move and a pixel never selected stays
        bit-identical to the one-shot frame with `samples: samples_done`; a selected pixel holds
        more samples (px_samples says how many) and finishes at the camera's `samples` like any
        other. Nothing eligible: nothing is rendered or changed. `selected` (u8 W*H) receives 1 at
        every selected pixel of the region; the other buffers are step()'s. After a focused step
        that rendered, save() is refused. Returns the RenderStats of the region's frame so far;
        `focus_info` describes the selection."""
        if self._cam is None:
            raise ValueError("the progressive session is closed")
        import numpy as np
        cam = self._cam
        px = cam.image_width * cam.image_height
        opts = _lib.RtFocusOptions(_lib.FOCUS_SCORE_VARIANCE, int(permille), float(min_score), int(max_pixels))
        mptr = hptr = None
        if isinstance(score, History):
            opts.source = _lib.FOCUS_SCORE_HISTORY
            hptr = score._handle()
        elif score is not None:
            opts.source = _lib.FOCUS_SCORE_MAP
            _x, _y, rw, rh = self._info().as_dict()["region"]
            smap = np.asarray(score, dtype=np.float32)
            if smap.shape == (cam.image_height, cam.image_width):
                smap = smap[_y:_y + rh, _x:_x + rw]
            elif smap.shape != (rh, rw):
                raise ValueError(f"score must be a ({cam.image_height}, {cam.image_width}) or ({rh}, {rw}) array, "
                                 f"not {smap.shape}")
            smap = np.ascontiguousarray(smap)
            mptr = smap.ctypes.data
        ptr, _k0 = _host_ptr(buffer, cam.byte_length, "buffer")
        rptr, _k1 = _host_ptr(radiance, cam.byte_length * 4, "radiance")
        sptr, _k2 = _host_ptr(px_samples, px * 4, "px_samples")
        bptr, _k3 = _host_ptr(px_bounces, px * 4, "px_bounces")
        selptr, _k4 = _host_ptr(selected, px, "selected")
        st, info = _lib.RtRenderStats(), _lib.RtFocusInfo()
        _lib.check(cam._lib.rt_camera_progressive_focus(cam._h, int(n), C.byref(opts), mptr, hptr, ptr, rptr, sptr, bptr,
                                                        selptr, C.byref(st), C.byref(info)))
        self._focus_info = info.as_dict()
        return RenderStats._from_c(st)

    @property
    def focus_info(self) -> Optional[dict]:
        """The last focus() call's selection (rt_focus_info): active, eligible, selected,
        threshold, focus_done, first_sample and select_ms (device time of the selection); None
        before the first call."""
        return getattr(self, "_focus_info", None)

    def variance(self, out=None):
        """The per-pixel variance of the pixel mean's illuminance from the session's running sums
        (rt_camera_progressive_variance): a float32 (H, W) array - `out` when given, else a new
        one, zero outside the region. Every pixel uses its own sample count. Needs
        samples_done >= 2 and a camera in the default mode."""
        if self._cam is None:
            raise ValueError("the progressive session is closed")
        import numpy as np
        cam = self._cam
        shape = (cam.image_height, cam.image_width)
        if out is None:
            out = np.zeros(shape, np.float32)
        ptr = _var_out(out, shape)
        _lib.check(cam._lib.rt_camera_progressive_variance(cam._h, ptr))
        return out if out.shape == shape else out.reshape(shape)

    def denoised(self, buffer=None, radiance=None, *, levels=4, sigma_color=None, sigma_plane=0.01, variance=False,
                 sigma_variance=2.0, variance_out=None, guides="first_hit", hold_edges=0):
        """The session's frame as it stands after the last step, through the a-trous filter
        (rt_camera_progressive_denoise): the frame never leaves the device, the region's guides
        are computed on first use and kept, and the session itself is not touched. `buffer` (u8
        W*H*3) and `radiance` (float32 W*H*3) are optional caller-owned full-frame buffers; only
        the region is written. Returns the filtered radiance as a (H, W, 3) array (`radiance`
        when given; else a new one, zero outside the region). `variance=True` runs the
        variance-guided filter on the variance of the session's own state
        (rt_camera_progressive_denoise_variance; needs samples_done >= 2) with `sigma_variance`
        in place of sigma_color; `variance_out` (optional float32 (H, W)) receives the region's
        filtered variance. `guides` as in Camera.denoise: the session keeps its specular guides
        beside the first-hit ones (which reprojected / accumulate / focus always use) and
        recomputes them when max_bounces or max_fuzz change. `hold_edges` (0, 2 or 4) as in
        Camera.denoise (rt_camera_progressive_denoise_hold, ..._variance_hold): the session computes
        the mask of its region once per value and keeps it; held pixels come back as the session's
        frame (and its state's variance) has them. accumulated(filter_levels=) has no hold."""
        if self._cam is None:
            raise ValueError("the progressive session is closed")
        cam = self._cam
        cam._set_denoise_guides(guides)
        ptr, rptr, radiance, _keep = _session_frame(cam, buffer, radiance, "buffer")
        guided, opts = _var_call(variance, sigma_color, sigma_variance, variance_out, levels, sigma_plane)
        if guided:
            vptr = _var_out(variance_out, (cam.image_height, cam.image_width))
            fn, *hold = _hold_entry(cam._lib, "rt_camera_progressive_denoise_variance", hold_edges)
            _lib.check(fn(cam._h, C.byref(opts), *hold, ptr, rptr, vptr))
        else:
            fn, *hold = _hold_entry(cam._lib, "rt_camera_progressive_denoise", hold_edges)
            _lib.check(fn(cam._h, C.byref(opts), *hold, ptr, rptr))
        return _session_result(cam, radiance)

    def reprojected(self, prev_cam: Camera, prev_radiance, rgb=None, radiance=None, weight_out=None, *,
                    prev_region=None, normal_min=0.9, sigma_plane=0.01, min_weight=0.25, history_samples=32.0,
                    guides=None, point_pixels=4.0, through=15, kind=None):
        """The session's frame as it stands after the last step, blended with `prev_radiance`
        (float32 (Hp, Wp, 3), a frame of `prev_cam`, a camera of the same scene) reprojected into
        this view, every pixel weighted by its own sample count (rt_camera_progressive_reproject):
        only the previous radiance is uploaded, and the session itself is not touched. `rgb` (u8
        W*H*3), `radiance` (float32 W*H*3) and `weight_out` (float32 (H, W)) are optional
        caller-owned full-frame buffers; only the region is written. Returns the blend as a
        (H, W, 3) array (`radiance` when given; else a new one, zero outside the region).
        `guides`, `point_pixels`, `through` and `kind` as in Camera.reproject
        (rt_camera_progressive_reproject_specular): the session keeps the chain guides and their
        chain plane beside its first-hit ones; its state and checkpoint bytes are not touched."""
        if self._cam is None:
            raise ValueError("the progressive session is closed")
        cam = self._cam
        H, W = cam.image_height, cam.image_width
        prad = _f32_frame(prev_radiance, (prev_cam.image_height, prev_cam.image_width, 3), "prev_radiance")
        ptr, rptr, radiance, _keep = _session_frame(cam, rgb, radiance)
        wptr, = _f32_outs(H, W, weight_out=weight_out)
        pptr = _region_ptr(prev_region)
        go, opts, *kptr = _gather_options(guides, _reproject_options(normal_min, sigma_plane, min_weight, history_samples),
                                          _lib.RtSpecularReprojectOptions, point_pixels, through, kind, (H, W))
        if go is None:
            _lib.check(cam._lib.rt_camera_progressive_reproject(cam._h, prev_cam._h, pptr, C.byref(opts),
                                                                prad.ctypes.data, ptr, rptr, wptr))
        else:
            _lib.check(cam._lib.rt_camera_progressive_reproject_specular(
                cam._h, prev_cam._h, pptr, C.byref(go), C.byref(opts), prad.ctypes.data, ptr, rptr, wptr, *kptr))
        return _session_result(cam, radiance)

    def accumulated(self, history: History, rgb=None, radiance=None, *, commit=True, variance_out=None,
                    length_out=None, weight_out=None, filter_levels=0, sigma_variance=2.0, normal_min=0.9,
                    sigma_plane=0.01, min_weight=0.25, max_history=256.0, guides=None, point_pixels=4.0, through=15,
                    kind=None):
        """The session's frame as it stands after the last step, accumulated onto `history`
        (rt_camera_progressive_accumulate): every pixel's history - gathered from the history's
        view as reprojected() does - is blended by its own length N = min(length, max_history)
        against the pixel's own sample count, and a variance is carried along. Nothing is uploaded:
        the frame, the counts, the state's variance and the guides are the session's device
        buffers. `commit=True` makes the result the history (its first call commits the frame
        itself); the session is never touched. `filter_levels > 0` returns the frame through the
        variance-guided filter driven by the accumulated variance (the history keeps the
        unfiltered frame). `rgb` (u8 W*H*3), `radiance` (float32 W*H*3), `variance_out`,
        `length_out`, `weight_out` (float32 (H, W)) are optional caller-owned full-frame buffers;
        only the region is written. Returns the radiance as a (H, W, 3) array. Needs
        samples_done >= 2, and every view rendered with its own `seed`: views that share a seed
        have correlated noise and the carried variance is then wrong.
        `guides` ("specular", or a dict of max_bounces / max_fuzz) carries the history through
        mirrors and glass (rt_camera_progressive_accumulate_specular): a pixel behind a specular
        chain finds its history at the chain's virtual point, on the chain planes the history keeps
        of its view (History.chain_guides) - if a call with the same `guides` committed them; the
        filter then uses the chain guides. `point_pixels`, `through` and `kind` (uint8 (H, W): 0 no
        history, 1 first hit, 2 chain) as in reprojected(), with `guides` only. Plain and specular
        calls mix freely on one history; the session's state and checkpoint bytes are not touched."""
        if self._cam is None:
            raise ValueError("the progressive session is closed")
        cam = self._cam
        H, W = cam.image_height, cam.image_width
        ptr, rptr, radiance, _keep = _session_frame(cam, rgb, radiance)
        outs = _f32_outs(H, W, variance_out=variance_out, length_out=length_out, weight_out=weight_out)
        go, opts, *kptr = _gather_options(
            guides, _temporal_options(normal_min, sigma_plane, min_weight, max_history, filter_levels, sigma_variance),
            _lib.RtSpecularTemporalOptions, point_pixels, through, kind, (H, W))
        if go is None:
            _lib.check(cam._lib.rt_camera_progressive_accumulate(
                cam._h, history._handle(), C.byref(opts), 1 if commit else 0, ptr, rptr, *outs))
        else:
            _lib.check(cam._lib.rt_camera_progressive_accumulate_specular(
                cam._h, history._handle(), C.byref(go), C.byref(opts), 1 if commit else 0, ptr, rptr, *outs, *kptr))
        return _session_result(cam, radiance)

    @property
    def info(self) -> dict:
        return self._info().as_dict()

    @property
    def samples_done(self) -> int:
        return self._info().samples_done

    @property
    def samples(self) -> int:
        return self._info().samples

    @property
    def active_pixels(self) -> int:
        return self._info().active_pixels

    @property
    def steps(self) -> int:
        return self._info().steps

    @property
    def done(self) -> bool:
        return bool(self._info().done)

    def save(self) -> bytes:
        """The session's checkpoint blob (rt_camera_progressive_save); Camera.resume continues it."""
        if self._cam is None:
            raise ValueError("the progressive session is closed")
        out, n = C.c_void_p(), C.c_size_t()
        _lib.check(self._cam._lib.rt_camera_progressive_save(self._cam._h, C.byref(out), C.byref(n)))
        try:
            return C.string_at(out, n.value)
        finally:
            self._cam._lib.rt_free(out)

    def close(self) -> None:
        cam, self._cam = self._cam, None
        if cam is not None and getattr(cam, "_h", None):
            _lib.check(cam._lib.rt_camera_progressive_end(cam._h))

    def __enter__(self) -> "ProgressiveRender":
        return self

    def __exit__(self, *exc) -> None:
        self.close()


def _dtypes():
    import numpy as np
    node = np.dtype([("bmin", "<f4", 3), ("a", "<i4"), ("bmax", "<f4", 3), ("b", "<i4")])
    prim = np.dtype([("type", "<i4"), ("mat", "<i4"), ("s0", "<f8"), ("g0", "<f4", 4), ("g1", "<f4", 4),
                     ("g2", "<f4", 4), ("g3", "<f4", 4), ("g4", "<f4", 4)])
    mat = np.dtype([("type", "<i4"), ("c0", "<i4"), ("c1", "<i4"), ("pad0", "<i4"), ("color", "<f4", 4),
                    ("emitted", "<f4", 4), ("p0", "<f8"), ("pad1", "<f8")])
    light = np.dtype([("prim", "<i4"), ("type", "<i4"), ("area", "<f8")])
    assert node.itemsize == 32 and prim.itemsize == 96 and mat.itemsize == 64 and light.itemsize == 16
    return node, prim, mat, light


try:
    NODE_DTYPE, PRIM_DTYPE, MAT_DTYPE, LIGHT_DTYPE = _dtypes()
except ImportError:  # pragma: no cover
    NODE_DTYPE = PRIM_DTYPE = MAT_DTYPE = LIGHT_DTYPE = None


def rng_stream(seed: int, pixel: int, sample: int, n: int) -> Sequence[int]:
    """The path RNG stream (seeded Math.random replacement), host evaluation."""
    out = (C.c_uint32 * n)()
    _lib.check(_lib.load().rt_debug_rng(seed, pixel, sample, n, out))
    return list(out)
