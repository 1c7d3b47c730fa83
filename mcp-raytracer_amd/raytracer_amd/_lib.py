"""ctypes binding of librt_amd.so (include/rt_amd.h).

The library is loaded from this package's lib/ directory only; if it is
missing or does not export the ABI, import fails loudly - there is no CPU
fallback anywhere in the product path.
"""
from __future__ import annotations

import ctypes as C
import json
import os
from pathlib import Path

from ._build import LIB_PATH, id_path, source_hash

# Public header, parsed by tests to check that every declared symbol is exported.
HEADER = Path(__file__).resolve().parents[2] / "include" / "rt_amd.h"

RT_OK, RT_ERR_INVALID, RT_ERR_DEVICE, RT_ERR_RENDER = 0, 1, 2, 3
PRECISION = {"ref": 0, "fp32": 1}
TRAVERSAL = {"fast": 0, "reference": 1, "brute": 2, "auto": 3}

CT_NAMES = ["node", "sphere", "quad", "plane", "material", "light_quad", "light_sphere",
            "bounces", "diffuse", "samples", "rays", "exact", "exact_wave", "cand0", "cand2", "exact2"]
PR_NAMES = ["newpath", "rr", "hit", "miss", "hitrec", "scatter", "sample", "pdf", "acc", "tile", "node", "leaf",
            "wnode", "wleaf", "loop", "trips"]
COUNTER_WORDS = 64
STATS_WORDS = 8  # RT_STATS_WORDS: pixels, samples, smin, smax, bounces, bmin, bmax, error


class RtRegion(C.Structure):
    _fields_ = [("x", C.c_int32), ("y", C.c_int32), ("width", C.c_int32), ("height", C.c_int32)]


class RtRenderStats(C.Structure):
    _fields_ = [("pixels", C.c_double),
                ("samples_total", C.c_double), ("samples_min", C.c_double),
                ("samples_max", C.c_double), ("samples_avg", C.c_double),
                ("bounces_total", C.c_double), ("bounces_min", C.c_double),
                ("bounces_max", C.c_double), ("bounces_avg", C.c_double)]


class RtCameraInfo(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("channels", C.c_int32),
                ("n_objects", C.c_int32), ("n_nodes", C.c_int32), ("n_lights", C.c_int32),
                ("n_materials", C.c_int32), ("bvh_depth", C.c_int32),
                ("samples_loop", C.c_int32), ("depth", C.c_int32), ("roulette", C.c_int32),
                ("roulette_depth", C.c_int32), ("mode", C.c_int32), ("adaptive", C.c_int32),
                ("precision", C.c_int32), ("traversal", C.c_int32), ("seed", C.c_uint32),
                ("samples", C.c_double), ("aperture", C.c_double),
                ("a_tolerance", C.c_double), ("a_batch", C.c_double)]


class RtLaunch(C.Structure):
    _fields_ = [("region", RtRegion), ("tile_group", C.c_int32), ("tile_groups", C.c_int32),
                ("precision", C.c_int32), ("traversal", C.c_int32), ("count_work", C.c_int32),
                ("rgb", C.c_void_p), ("radiance", C.c_void_p),
                ("px_samples", C.c_void_p), ("px_bounces", C.c_void_p),
                ("stream", C.c_void_p), ("synchronize", C.c_int32), ("packed_tiles", C.c_int32)]


MAX_DEVICES = 16  # RT_MAX_DEVICES
GATHER = {0: "rccl", 1: "peer"}  # RT_GATHER_*


class RtMultiPlan(C.Structure):
    _fields_ = [("region", RtRegion), ("n_devices", C.c_int32), ("slab_tiles", C.c_int32), ("tiles", C.c_int64),
                ("slab_bytes_rgb", C.c_int64), ("slab_bytes_radiance", C.c_int64), ("stats_offset", C.c_int64),
                ("group_tiles", C.c_int32 * MAX_DEVICES)]


class RtMultiInfo(C.Structure):
    _fields_ = [("n_devices", C.c_int32), ("transport", C.c_int32), ("devices", C.c_int32 * MAX_DEVICES),
                ("path_ms", C.c_float * MAX_DEVICES), ("accum_ms", C.c_float * MAX_DEVICES),
                ("gather_ms", C.c_float), ("plan", RtMultiPlan)]


class RtProgressiveInfo(C.Structure):
    _fields_ = [("region", RtRegion), ("width", C.c_int32), ("height", C.c_int32),
                ("samples_done", C.c_int32), ("samples", C.c_int32), ("steps", C.c_int32), ("done", C.c_int32),
                ("precision", C.c_int32), ("seed", C.c_uint32), ("active_pixels", C.c_int64),
                ("state_bytes", C.c_uint64), ("build_id", C.c_char * 24)]

    def as_dict(self) -> dict:
        r = self.region
        return {"region": (r.x, r.y, r.width, r.height), "width": self.width, "height": self.height,
                "samples_done": self.samples_done, "samples": self.samples, "steps": self.steps,
                "done": bool(self.done), "precision": "fp32" if self.precision == 1 else "ref", "seed": self.seed,
                "active_pixels": self.active_pixels, "state_bytes": self.state_bytes,
                "build_id": self.build_id.decode()}


class RtDenoiseOptions(C.Structure):
    _fields_ = [("levels", C.c_int32), ("sigma_color", C.c_float), ("sigma_plane", C.c_float)]


class RtDenoiseVarOptions(C.Structure):
    _fields_ = [("levels", C.c_int32), ("sigma_variance", C.c_float), ("sigma_plane", C.c_float)]


DENOISE_MAX_LEVELS = 8


GUIDES_FIRST_HIT, GUIDES_SPECULAR = 0, 1  # RT_GUIDES_*


class RtGuideOptions(C.Structure):
    _fields_ = [("mode", C.c_int32), ("max_bounces", C.c_int32), ("max_fuzz", C.c_float)]


class RtView(C.Structure):
    _fields_ = [("center", C.c_float * 3), ("pixel00", C.c_float * 3), ("du", C.c_float * 3), ("dv", C.c_float * 3),
                ("width", C.c_int32), ("height", C.c_int32)]


class RtReprojectOptions(C.Structure):
    _fields_ = [("normal_min", C.c_float), ("sigma_plane", C.c_float), ("min_weight", C.c_float),
                ("history_samples", C.c_float)]


class RtSpecularReprojectOptions(C.Structure):
    _fields_ = [("base", RtReprojectOptions), ("point_pixels", C.c_float), ("through", C.c_int32)]


class RtTemporalOptions(C.Structure):
    _fields_ = [("normal_min", C.c_float), ("sigma_plane", C.c_float), ("min_weight", C.c_float),
                ("max_history", C.c_float), ("filter_levels", C.c_int32), ("sigma_variance", C.c_float)]


class RtSpecularTemporalOptions(C.Structure):
    _fields_ = [("base", RtTemporalOptions), ("point_pixels", C.c_float), ("through", C.c_int32)]


class RtHistoryInfo(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("region", RtRegion), ("views", C.c_int32),
                ("device", C.c_int32), ("scene_hash", C.c_uint64), ("bytes", C.c_uint64), ("view", RtView)]


FOCUS_SCORE_VARIANCE, FOCUS_SCORE_MAP, FOCUS_SCORE_HISTORY = 0, 1, 2


class RtFocusOptions(C.Structure):
    _fields_ = [("source", C.c_int32), ("permille", C.c_int32), ("min_score", C.c_float), ("max_pixels", C.c_int32)]


class RtFocusInfo(C.Structure):
    _fields_ = [("active", C.c_int64), ("eligible", C.c_int64), ("selected", C.c_int64), ("threshold", C.c_float),
                ("focus_done", C.c_int32), ("first_sample", C.c_int32), ("select_ms", C.c_float)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class RtPrimaryInfo(C.Structure):
    _fields_ = [("available", C.c_int32), ("used", C.c_int32), ("built", C.c_int32), ("min_samples", C.c_int32),
                ("build_ms", C.c_float)]


RT_PRIMARY_TABLE_NONE = 4  # rt_camera_primary_table: the camera has no primary-ray table


class RtSceneBlobInfo(C.Structure):
    _fields_ = [("bytes", C.c_int64)] + [(n, C.c_int32) for n in (
        "off_tprims", "off_tsph", "off_prims", "off_xrec", "off_mats", "off_lights", "off_onbs", "off_nodes",
        "off_pre", "off_tsph2", "lds_words", "lds_words2", "n_pre", "n_onb")]


PLAN_MAX_PHASES = 8  # RT_PLAN_MAX_PHASES
KERNEL = {0: "none", 1: "sequential", 2: "chunked", 3: "pool"}  # RT_KERNEL_*


class RtLaunchPlan(C.Structure):
    _fields_ = [("table_exists", C.c_int32), ("region", RtRegion),
                ("kernel", C.c_int32), ("traversal", C.c_int32), ("tiles", C.c_int32),
                ("lds_level", C.c_int32), ("n_top", C.c_int32), ("lds_bytes", C.c_int64), ("stack_bytes", C.c_int64),
                ("defer", C.c_int32), ("pool", C.c_int32), ("primary_ok", C.c_int32), ("rec12", C.c_int32),
                ("grid", C.c_int32), ("sb_pool", C.c_int32), ("n_phases", C.c_int32),
                ("s0", C.c_int32 * PLAN_MAX_PHASES), ("chunk", C.c_int32 * PLAN_MAX_PHASES),
                ("nch", C.c_int32 * PLAN_MAX_PHASES), ("refill_min", C.c_int32), ("min_ready", C.c_int32),
                ("samples", C.c_int32), ("passes", C.c_int32), ("pass_units", C.c_int64)]


class RtError(RuntimeError):
    """An error returned through the C ABI (the reference would throw an Error)."""

    def __init__(self, code: int, message: str):
        super().__init__(message)
        self.code = code


_SIGS = {
    "rt_version": (C.c_int, []),
    "rt_last_error": (C.c_char_p, []),
    "rt_free": (None, [C.c_void_p]),
    "rt_generate_scene_data": (C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(C.c_void_p)]),
    "rt_camera_create": (C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(C.c_void_p)]),
    "rt_camera_destroy": (None, [C.c_void_p]),
    "rt_camera_get_info": (C.c_int, [C.c_void_p, C.POINTER(RtCameraInfo)]),
    "rt_camera_set_precision": (C.c_int, [C.c_void_p, C.c_int32]),
    "rt_camera_render_region": (C.c_int, [C.c_void_p, C.POINTER(RtRegion), C.c_void_p, C.c_void_p,
                                          C.POINTER(RtRenderStats)]),
    "rt_camera_render": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(RtRenderStats)]),
    "rt_camera_render_device": (C.c_int, [C.c_void_p, C.POINTER(RtLaunch), C.POINTER(RtRenderStats),
                                          C.POINTER(C.c_uint64)]),
    "rt_camera_export": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p]),
    "rt_debug_world_hit": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_debug_world_hit_fp32": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_debug_pass_plan": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64,
                                     C.POINTER(C.c_int64)]),
    "rt_debug_scene_blob": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(RtSceneBlobInfo)]),
    "rt_debug_launch_plan": (C.c_int, [C.c_void_p, C.POINTER(RtRegion), C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                       C.c_int32, C.c_int32, C.POINTER(RtLaunchPlan)]),
    "rt_debug_rng": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32, C.c_void_p]),
    "rt_debug_math": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p]),
    "rt_debug_fp64": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p]),
    "rt_device_count": (C.c_int, [C.POINTER(C.c_int32)]),
    "rt_camera_kernel_times": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "rt_camera_adaptive_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_uint64)]),
    "rt_camera_stats_words": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_camera_pass_count": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "rt_camera_last_kernel": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "rt_camera_primary_table": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    "rt_camera_primary_table_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    "rt_camera_primary_info": (C.c_int, [C.c_void_p, C.POINTER(RtPrimaryInfo)]),
    "rt_camera_release_device": (C.c_int, [C.c_void_p]),
    "rt_build_id": (C.c_char_p, []),
    "rt_tiles_unpack": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(RtRegion), C.c_int32, C.c_int32,
                                  C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "rt_encode_png": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p),
                                C.POINTER(C.c_size_t)]),
    "rt_encode_ppm": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "rt_encode_png_device": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_void_p),
                                       C.POINTER(C.c_size_t)]),
    "rt_debug_png_host": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_void_p),
                                    C.POINTER(C.c_size_t)]),
    "rt_camera_render_png": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(RtRenderStats), C.POINTER(C.c_void_p),
                                       C.POINTER(C.c_size_t)]),
    "rt_multi_plan_region": (C.c_int, [C.POINTER(RtRegion), C.c_int32, C.c_int32, C.c_int32,
                                       C.POINTER(RtMultiPlan)]),
    "rt_camera_render_multi": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int32, C.POINTER(RtRegion),
                                         C.c_void_p, C.c_void_p, C.POINTER(RtRenderStats)]),
    "rt_camera_render_png_multi": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int32, C.POINTER(RtRenderStats),
                                             C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "rt_camera_multi_info": (C.c_int, [C.c_void_p, C.POINTER(RtMultiInfo)]),
    "rt_camera_progressive_begin": (C.c_int, [C.c_void_p, C.POINTER(RtRegion)]),
    "rt_camera_progressive_step": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.POINTER(RtRenderStats)]),
    "rt_camera_progressive_info": (C.c_int, [C.c_void_p, C.POINTER(RtProgressiveInfo)]),
    "rt_camera_progressive_save": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "rt_camera_progressive_restore": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t]),
    "rt_progressive_blob_info": (C.c_int, [C.c_char_p, C.c_size_t, C.POINTER(RtProgressiveInfo)]),
    "rt_camera_progressive_end": (C.c_int, [C.c_void_p]),
    "rt_camera_render_guides": (C.c_int, [C.c_void_p, C.POINTER(RtRegion), C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p]),
    "rt_guide_options_default": (None, [C.POINTER(RtGuideOptions)]),
    "rt_camera_render_guides_ex": (C.c_int, [C.c_void_p, C.POINTER(RtRegion), C.POINTER(RtGuideOptions), C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_camera_set_denoise_guides": (C.c_int, [C.c_void_p, C.POINTER(RtGuideOptions)]),
    "rt_camera_get_denoise_guides": (C.c_int, [C.c_void_p, C.POINTER(RtGuideOptions)]),
    "rt_denoise": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(RtRegion), C.POINTER(RtDenoiseOptions), C.c_void_p,
                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_camera_denoise": (C.c_int, [C.c_void_p, C.POINTER(RtRegion), C.POINTER(RtDenoiseOptions), C.c_void_p,
                                    C.c_void_p, C.c_void_p]),
    "rt_camera_progressive_denoise": (C.c_int, [C.c_void_p, C.POINTER(RtDenoiseOptions), C.c_void_p, C.c_void_p]),
    "rt_camera_denoise_times": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_float),
                                          C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "rt_progressive_blob_variance": (C.c_int, [C.c_char_p, C.c_size_t, C.c_void_p]),
    "rt_camera_progressive_variance": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rt_denoise_variance": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(RtRegion), C.POINTER(RtDenoiseVarOptions),
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_camera_denoise_variance": (C.c_int, [C.c_void_p, C.POINTER(RtRegion), C.POINTER(RtDenoiseVarOptions),
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_camera_progressive_denoise_variance": (C.c_int, [C.c_void_p, C.POINTER(RtDenoiseVarOptions), C.c_void_p,
                                                         C.c_void_p, C.c_void_p]),
    "rt_camera_render_coverage": (C.c_int, [C.c_void_p, C.POINTER(RtRegion), C.c_int32, C.c_void_p]),
    "rt_camera_coverage_time": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "rt_denoise_hold": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(RtRegion), C.POINTER(RtDenoiseOptions), C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_denoise_variance_hold": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(RtRegion), C.POINTER(RtDenoiseVarOptions),
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_camera_denoise_hold": (C.c_int, [C.c_void_p, C.POINTER(RtRegion), C.POINTER(RtDenoiseOptions), C.c_int32,
                                         C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_camera_denoise_variance_hold": (C.c_int, [C.c_void_p, C.POINTER(RtRegion), C.POINTER(RtDenoiseVarOptions),
                                                  C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_void_p]),
    "rt_camera_progressive_denoise_hold": (C.c_int, [C.c_void_p, C.POINTER(RtDenoiseOptions), C.c_int32, C.c_void_p,
                                                     C.c_void_p]),
    "rt_camera_progressive_denoise_variance_hold": (C.c_int, [C.c_void_p, C.POINTER(RtDenoiseVarOptions), C.c_int32,
                                                              C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_camera_get_view": (C.c_int, [C.c_void_p, C.POINTER(RtView)]),
    "rt_camera_reusable_objects": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    "rt_reproject": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(RtRegion), C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_void_p, C.POINTER(RtView), C.POINTER(RtRegion), C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(RtReprojectOptions),
                               C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_camera_reproject": (C.c_int, [C.c_void_p, C.POINTER(RtRegion), C.c_void_p, C.POINTER(RtRegion),
                                      C.POINTER(RtReprojectOptions), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_camera_progressive_reproject": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(RtRegion),
                                                  C.POINTER(RtReprojectOptions), C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_void_p]),
    "rt_camera_reproject_times": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                            C.POINTER(C.c_float)]),
    "rt_specular_reproject_options_default": (None, [C.POINTER(RtSpecularReprojectOptions)]),
    "rt_camera_through_objects": (C.c_int, [C.c_void_p, C.c_int32, C.c_float, C.c_void_p, C.c_int32]),
    "rt_reproject_specular": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(RtRegion), *[C.c_void_p] * 9, C.POINTER(RtView),
                                        C.POINTER(RtView), C.POINTER(RtRegion), *[C.c_void_p] * 10, C.c_void_p,
                                        C.c_void_p, C.c_int32, C.POINTER(RtSpecularReprojectOptions), C.c_void_p,
                                        C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
    "rt_camera_reproject_specular": (C.c_int, [C.c_void_p, C.POINTER(RtRegion), C.c_void_p, C.POINTER(RtRegion),
                                               C.POINTER(RtGuideOptions), C.POINTER(RtSpecularReprojectOptions),
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_camera_progressive_reproject_specular": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(RtRegion),
                                                           C.POINTER(RtGuideOptions),
                                                           C.POINTER(RtSpecularReprojectOptions), C.c_void_p, C.c_void_p,
                                                           C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_history_create": (C.c_int, [C.POINTER(C.c_void_p)]),
    "rt_history_destroy": (None, [C.c_void_p]),
    "rt_history_get_info": (C.c_int, [C.c_void_p, C.POINTER(RtHistoryInfo)]),
    "rt_history_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_camera_progressive_accumulate": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(RtTemporalOptions), C.c_int32,
                                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_temporal_accumulate": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(RtRegion), C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(RtView),
                                         C.POINTER(RtRegion), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                         C.POINTER(RtTemporalOptions), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p]),
    "rt_history_times": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                   C.POINTER(C.c_float)]),
    "rt_specular_temporal_options_default": (None, [C.POINTER(RtSpecularTemporalOptions)]),
    "rt_history_chain_guides": (C.c_int, [C.c_void_p, C.POINTER(RtGuideOptions), C.POINTER(C.c_int32)]),
    "rt_camera_progressive_accumulate_specular": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(RtGuideOptions),
                                                            C.POINTER(RtSpecularTemporalOptions), C.c_int32,
                                                            *[C.c_void_p] * 6]),
    "rt_temporal_accumulate_specular": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(RtRegion), *[C.c_void_p] * 9,
                                                  C.POINTER(RtView), C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                                  C.POINTER(RtView), C.POINTER(RtRegion), *[C.c_void_p] * 9,
                                                  *[C.c_void_p] * 3, C.c_void_p, C.c_void_p, C.c_int32,
                                                  C.POINTER(RtSpecularTemporalOptions), *[C.c_void_p] * 6]),
    "rt_focus_options_default": (None, [C.POINTER(RtFocusOptions)]),
    "rt_camera_progressive_focus": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(RtFocusOptions), C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.POINTER(RtRenderStats), C.POINTER(RtFocusInfo)]),
}

_lib = None


def load() -> C.CDLL:
    """Load librt_amd.so (built in-tree by __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    path = LIB_PATH
    variant = os.environ.get("RT_AMD_VARIANT")  # experiments: lib/librt_amd_<variant>.so (same package dir)
    if variant:
        if not variant.isidentifier():
            raise ImportError(f"bad RT_AMD_VARIANT {variant!r}")
        path = LIB_PATH.with_name(f"librt_amd_{variant}.so")
    if not path.exists():
        raise ImportError(f"{path.name} not found at {path}; run __graft_entry__.build() "
                          "(hipcc --offload-arch=gfx950) first - there is no CPU fallback")
    # PyTorch-ROCm ships its own libamdhip64.so.7 (same soname as /opt/rocm's).
    # Whichever loads first serves the whole process, and torch cannot run on a
    # newer runtime, so let torch's copy load first when torch is installed; the
    # library then shares torch's HIP runtime (device memory, streams).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(os.fspath(path))
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    # the binary must have been built from these sources (no stale .so under test)
    built = lib.rt_build_id().decode()
    want = source_hash() if not variant else (id_path(path).read_text().strip() if id_path(path).exists() else "")
    if built != want:
        raise ImportError(f"{path.name} was built from sources {built}, the tree has {want}: "
                          "rebuild with __graft_entry__.build()")
    _lib = lib
    return lib


def build_id() -> str:
    """Source hash librt_amd.so was built from (rt_build_id)."""
    return load().rt_build_id().decode()


def check(code: int) -> None:
    if code != RT_OK:
        msg = load().rt_last_error()
        raise RtError(code, msg.decode("utf-8", "replace") if msg else f"rt error {code}")


def to_json(obj) -> bytes:
    """Serialise like JSON.stringify, keeping Infinity/NaN (accepted by the C parser)."""
    return json.dumps(obj, allow_nan=True, separators=(",", ":")).encode()


def multi_plan(region, width: int, height: int, n_devices: int) -> dict:
    """rt_multi_plan_region: the split of a region over n devices (host only)."""
    p = RtMultiPlan()
    reg = RtRegion(*[int(v) for v in region])
    check(load().rt_multi_plan_region(C.byref(reg), int(width), int(height), int(n_devices), C.byref(p)))
    return {"region": (p.region.x, p.region.y, p.region.width, p.region.height), "n_devices": p.n_devices,
            "slab_tiles": p.slab_tiles, "tiles": p.tiles, "slab_bytes_rgb": p.slab_bytes_rgb,
            "slab_bytes_radiance": p.slab_bytes_radiance, "stats_offset": p.stats_offset,
            "group_tiles": list(p.group_tiles)[:p.n_devices]}


def scene_blob(cam_handle) -> tuple[bytes, dict]:
    """rt_debug_scene_blob: the scene blob a device context would upload for the camera, and its
    section offsets and counts (host only)."""
    info = RtSceneBlobInfo()
    check(load().rt_debug_scene_blob(cam_handle, None, 0, C.byref(info)))
    buf = C.create_string_buffer(max(int(info.bytes), 1))
    check(load().rt_debug_scene_blob(cam_handle, buf, int(info.bytes), C.byref(info)))
    return buf.raw[:info.bytes], {n: int(getattr(info, n)) for n, _ in RtSceneBlobInfo._fields_}


def launch_plan(cam_handle, region, tile_group: int = 0, tile_groups: int = 1, cus: int = 256, lds_max: int = 163840,
                precision: int = -1, count: int = 0, table_exists: bool = False) -> dict:
    """rt_debug_launch_plan: what a render of `region` would launch on a device of `cus` compute
    units and `lds_max` bytes of LDS (host only); the schedule arrays cut to n_phases."""
    p = RtLaunchPlan()
    p.table_exists = 1 if table_exists else 0
    reg = RtRegion(*[int(v) for v in region])
    check(load().rt_debug_launch_plan(cam_handle, C.byref(reg), int(tile_group), int(tile_groups), int(cus),
                                      int(lds_max), int(precision), int(count), C.byref(p)))
    d = {}
    for n, _ in RtLaunchPlan._fields_[2:]:
        v = getattr(p, n)
        d[n] = [int(x) for x in v][:p.n_phases] if n in ("s0", "chunk", "nch") else int(v)
    d["kernel"] = KERNEL[p.kernel]
    d["region"] = [p.region.x, p.region.y, p.region.width, p.region.height]
    return d


def progressive_blob_info(blob: bytes) -> dict:
    """rt_progressive_blob_info: a checkpoint blob's header, parsed and validated (length,
    magic, version, checksums) on the host - region, samples_done, samples, steps, done,
    active_pixels, precision, seed, state_bytes, build_id. Raises RtError on a bad blob."""
    info = RtProgressiveInfo()
    blob = bytes(blob)
    check(load().rt_progressive_blob_info(blob, len(blob), C.byref(info)))
    return info.as_dict()


def progressive_blob_variance(blob: bytes):
    """rt_progressive_blob_variance: the per-pixel variance of the pixel mean's illuminance held
    by a checkpoint blob, on the host (no device) - a float32 (height, width) array, zero outside
    the blob's region. Equals ProgressiveRender.variance() of the session that saved it. Raises
    RtError on a bad blob."""
    import numpy as np
    blob = bytes(blob)
    info = progressive_blob_info(blob)
    var = np.zeros((info["height"], info["width"]), np.float32)
    check(load().rt_progressive_blob_variance(blob, len(blob), var.ctypes.data))
    return var


def device_count() -> int:
    n = C.c_int32(0)
    check(load().rt_device_count(C.byref(n)))
    return int(n.value)
