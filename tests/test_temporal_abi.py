"""Accumulation across views, host side: the ABI surface, the history object without a device, the
argument errors that need no device, the restatement's own properties and what the accumulation
is worth on oracle frames (tests/temporal_ref.py is the normative definition)."""
import ctypes as C
import functools
import json
import re
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
from temporal_ref import F, oracle_trial, temporal_ref  # noqa: E402

GOLDEN = Path(__file__).resolve().parent / "golden"

DECLARED = {
    "rt_history_create": ("int", "(rt_history** out)"),
    "rt_history_destroy": ("void", "(rt_history* h)"),
    "rt_history_get_info": ("int", "(const rt_history* h, rt_history_info* info)"),
    "rt_history_read": ("int", "(rt_history* h, float* radiance, float* variance, float* length)"),
    "rt_camera_progressive_accumulate": ("int", "(rt_camera* cam, rt_history* h, const rt_temporal_options* options, "
                                                "int32_t commit, uint8_t* rgb, float* radiance, float* variance_out, "
                                                "float* length_out, float* weight_out)"),
    "rt_temporal_accumulate": ("int", "(int32_t width, int32_t height, const rt_region* region, const float* normal, "
                                      "const float* position, const float* distance, const int32_t* object, const float* "
                                      "radiance, const int32_t* px_samples, int32_t samples, const float* variance, const "
                                      "rt_view* prev_view, const rt_region* prev_region, const float* prev_normal, const "
                                      "float* prev_position, const float* prev_distance, const int32_t* prev_object, "
                                      "const float* prev_radiance, const float* prev_variance, const float* prev_length, "
                                      "const uint8_t* reusable, int32_t n_objects, const rt_temporal_options* options, "
                                      "float* radiance_out, float* variance_out, float* length_out, float* weight_out, "
                                      "uint8_t* rgb_out)"),
    "rt_history_times": ("int", "(rt_history* h, float* guide_ms, float* gather_ms, float* filter_ms, float* total_ms)"),
}


def scene_of(name):
    return json.loads((GOLDEN / f"scene_{name}.json").read_text())["scene"]


def test_temporal_symbols_are_declared_exported_and_bound(rt):
    from raytracer_amd import _lib
    lib = _lib.load()
    text = re.sub(r"\s+", " ", _lib.HEADER.read_text())
    assert "typedef struct rt_history rt_history;" in text
    assert ("typedef struct { float normal_min, sigma_plane, min_weight, max_history; int32_t filter_levels; float "
            "sigma_variance; } rt_temporal_options;" in text)
    assert ("typedef struct { int32_t width, height; rt_region region; int32_t views, device; uint64_t scene_hash, bytes; "
            "rt_view view; } rt_history_info;" in text)
    for name, (res, args) in DECLARED.items():
        assert f"{res} {name}{args};" in text, f"{name} is not declared as proposed"
        assert hasattr(lib, name), f"{name} is not exported"
        restype, argtypes = _lib._SIGS[name]
        assert restype is (C.c_int if res == "int" else None) and len(argtypes) == args.count(",") + 1
    assert C.sizeof(_lib.RtTemporalOptions) == 24 and C.sizeof(_lib.RtHistoryInfo) == 104
    assert lib.rt_version() == 3                       # functions were added, nothing changed
    assert callable(rt.temporal_accumulate) and hasattr(rt.ProgressiveRender, "accumulated")
    assert all(hasattr(rt.History, m) for m in ("info", "views", "read", "times", "close", "__enter__", "__exit__"))
    assert "seed" in rt.ProgressiveRender.accumulated.__doc__ and "VARY THE SEED" in _lib.HEADER.read_text()


def test_history_object_needs_no_device(rt):
    from raytracer_amd import _lib
    lib = _lib.load()
    with rt.History() as h:
        i = h.info
        assert h.views == 0 and i["views"] == 0 and i["device"] == -1 and i["bytes"] == 0
        assert (i["width"], i["height"], i["region"], i["scene_hash"]) == (0, 0, (0, 0, 0, 0), 0)
        with pytest.raises(rt.RtError, match="the history is empty") as e:
            h.read()
        assert e.value.code == _lib.RT_ERR_INVALID
        with pytest.raises(rt.RtError, match="no accumulate call yet"):
            h.times()
        assert lib.rt_history_get_info(h._h, None) == _lib.RT_ERR_INVALID
        assert lib.rt_history_times(h._h, None, None, None, None) == _lib.RT_ERR_INVALID
    with pytest.raises(ValueError):
        h.info
    h.close()                                          # closing twice is harmless
    assert lib.rt_history_create(None) == _lib.RT_ERR_INVALID
    assert lib.rt_history_get_info(None, C.byref(_lib.RtHistoryInfo())) == _lib.RT_ERR_INVALID
    assert lib.rt_history_read(None, None, None, None) == _lib.RT_ERR_INVALID
    lib.rt_history_destroy(None)


# ---- errors that need no device -------------------------------------------------------------------
def _frames16():
    rad = np.zeros((16, 16, 3), np.float32)
    g = {"normal": rad, "position": rad, "distance": rad[..., 0].copy(), "object": np.zeros((16, 16), np.int32)}
    view = {"center": [0, 0, 0], "pixel00": [-0.5, 0.5, -1], "du": [1 / 16, 0, 0], "dv": [0, -1 / 16, 0], "width": 16,
            "height": 16}
    return rad, g, view


def _explicit(rt, **kw):
    rad, g, view = _frames16()
    return rt.temporal_accumulate(rad, g["distance"], g["distance"], view, g, **g, reusable=np.ones(1, np.uint8),
                                  radiance=rad, variance=g["distance"], **{"samples": 4, **kw})


BAD_OPTIONS = [({k: v}, k) for k in ("normal_min", "sigma_plane", "min_weight", "max_history", "sigma_variance")
               for v in (-0.5, float("nan"), float("inf"))] + [({"filter_levels": 9}, "filter_levels"),
                                                              ({"filter_levels": -1}, "filter_levels")]


@pytest.mark.parametrize("opts,word", BAD_OPTIONS)
def test_bad_options_are_invalid_without_a_device(rt, opts, word):
    from raytracer_amd import _lib
    cam = rt.create_camera_from_scene_data(scene_of("cornell"), {"width": 16, "samples": 4, "depth": 4})
    with rt.History() as h:
        for call in (lambda: _explicit(rt, **opts), lambda: rt.ProgressiveRender(cam).accumulated(h, **opts)):
            with pytest.raises(rt.RtError, match=word) as e:
                call()
            assert e.value.code == _lib.RT_ERR_INVALID
        assert h.views == 0


def test_empty_regions_negative_samples_missing_pointers_and_no_session_without_a_device(rt):
    from raytracer_amd import _lib
    lib = _lib.load()
    for region in [(16, 0, 4, 4), (0, 0, 0, 5), (-8, -8, 8, 8)]:
        for key in ("region", "prev_region"):
            with pytest.raises(rt.RtError, match="empty after clamping") as e:
                _explicit(rt, **{key: region})
            assert e.value.code == _lib.RT_ERR_INVALID
    with pytest.raises(rt.RtError, match="samples") as e:
        _explicit(rt, samples=-1)
    assert e.value.code == _lib.RT_ERR_INVALID
    # the raw entry: every required pointer
    rad, g, _ = _frames16()
    view = _lib.RtView()
    view.width = view.height = 16
    p, d = rad.ctypes.data, g["distance"].ctypes.data
    gp = [p, p, d, g["object"].ctypes.data]
    reus = np.ones(1, np.uint8)
    good = [16, 16, None, *gp, p, None, 4, d, C.byref(view), None, *gp, p, d, d, reus.ctypes.data, 1, None, None, None,
            None, None, None]
    assert len(good) == len(_lib._SIGS["rt_temporal_accumulate"][1])
    for k in (3, 4, 5, 6, 7, 10, 11, 13, 14, 15, 16, 17, 18, 19, 20):
        args = list(good)
        args[k] = None
        assert lib.rt_temporal_accumulate(*args) == _lib.RT_ERR_INVALID, k
        assert b"required" in lib.rt_last_error() or b"reusable" in lib.rt_last_error(), k
    view.width = 0
    assert lib.rt_temporal_accumulate(*good) == _lib.RT_ERR_INVALID and b"previous view" in lib.rt_last_error()
    # the session entry: no session, no history, no camera
    cam = rt.create_camera_from_scene_data(scene_of("cornell"), {"width": 16, "samples": 4, "depth": 4})
    with rt.History() as h:
        with pytest.raises(rt.RtError, match="no progressive session is open") as e:
            rt.ProgressiveRender(cam).accumulated(h)
        assert e.value.code == _lib.RT_ERR_INVALID
        assert lib.rt_camera_progressive_accumulate(cam._h, None, None, 1, None, None, None, None,
                                                    None) == _lib.RT_ERR_INVALID
        assert lib.rt_camera_progressive_accumulate(None, h._h, None, 1, None, None, None, None,
                                                    None) == _lib.RT_ERR_INVALID
        pr = rt.ProgressiveRender(cam)
        pr.close()
        with pytest.raises(ValueError):
            pr.accumulated(h)
        assert h.views == 0


# ---- the restatement's own properties -------------------------------------------------------------
S = 2.0 ** -5


def quad_view(W, H, shift=0.0):
    """A camera at the origin looking down -z whose pixels are 2^-5 apart on the plane z = -1,
    pixel (0, 0) moved by `shift` pixels along both axes: every value is exact in fp32."""
    return {"center": [0, 0, 0], "pixel00": [(-(W - 1) / 2 + shift) * S, ((H - 1) / 2 - shift) * S, -1.0],
            "du": [S, 0, 0], "dv": [0, -S, 0], "width": W, "height": H}


def quad_guides(view):
    """First hits of the view's pinhole rays on the fronto-parallel plane z = -4, object 0."""
    W, H = view["width"], view["height"]
    p, du, dv = (np.asarray(view[k], F) for k in ("pixel00", "du", "dv"))
    i = np.arange(W, dtype=F)[None, :, None]; j = np.arange(H, dtype=F)[:, None, None]
    P = (F(4) * (p + du * i + dv * j)).astype(F)
    n = np.zeros((H, W, 3), F); n[..., 2] = 1
    D = np.sqrt((P * P).sum(-1)).astype(F)
    return {"normal": n, "position": P, "distance": D, "object": np.zeros((H, W), np.int32)}


def test_restatement_accumulates_lengths_and_variances_on_a_static_view():
    W, H = 32, 24
    view = quad_view(W, H)
    g = quad_guides(view)
    inner = (slice(1, H - 1), slice(1, W - 1))
    c0 = np.full((H, W, 3), 1.0, F); v0 = np.full((H, W), 0.5, F)
    # an empty history: the fresh frame, its variance and its counts are committed as they are
    r = temporal_ref(None, **g, radiance=c0, variance=v0, reusable=[1], samples=4)
    assert (r["weight"] == 0).all() and (r["radiance"] == c0).all() and (r["variance"] == v0).all()
    assert (r["length"] == 4).all()
    hist = {**r["history"], "view": view}
    # 4 + 12 samples: out = (1 * 4 + 3 * 12) / 16, V = (1/4)^2 * 0.5 + (3/4)^2 * 0.25, L = 16 - all exact
    c1 = np.full((H, W, 3), 3.0, F); v1 = np.full((H, W), 0.25, F)
    pxs = np.full((H, W), 12, np.int32); pxs[3, 4] = 0
    c1[5, 6] = np.nan
    v1[7, 8] = -1.0; v1[7, 9] = np.nan; v1[7, 10] = np.inf       # sanitised to 0
    r = temporal_ref(hist, **g, radiance=c1, variance=v1, reusable=[1], px_samples=pxs)
    assert (r["weight"][inner] == 1).all()
    assert (r["radiance"][10, 10] == F(2.5)).all() and r["length"][10, 10] == 16
    assert r["variance"][10, 10] == F(0.5 / 16 + 0.25 * 9 / 16)
    assert r["variance"][7, 8] == r["variance"][7, 9] == r["variance"][7, 10] == F(0.5 / 16)
    # no fresh sample / a non-finite fresh colour: the history as it is, its length unchanged
    for y, x in ((3, 4), (5, 6)):
        assert (r["radiance"][y, x] == 1).all() and r["variance"][y, x] == F(0.5) and r["length"][y, x] == 4
    # max_history bounds the weight of the past
    r = temporal_ref(hist, **g, radiance=c1, variance=v1, reusable=[1], samples=2, max_history=2.0)
    assert (r["radiance"][10, 10] == 2).all() and r["length"][10, 10] == 4
    # a history pixel that never held a sample is not history; nor is a NaN or inf length
    hist2 = {**hist, "length": hist["length"].copy()}
    hist2["length"][10, 10] = 0; hist2["length"][12, 12] = np.nan; hist2["length"][14, 14] = np.inf
    r = temporal_ref(hist2, **g, radiance=c1, variance=v1, reusable=[1], samples=12)
    for y, x in ((10, 10), (12, 12), (14, 14)):
        assert r["weight"][y, x] == 0 and (r["radiance"][y, x] == 3).all() and r["length"][y, x] == 12
        assert r["variance"][y, x] == F(0.25)
    # not reusable: nothing is history, and a non-finite fresh pixel holds no sample
    r = temporal_ref(hist, **g, radiance=c1, variance=v1, reusable=[0], samples=12)
    assert (r["weight"] == 0).all() and r["length"][5, 6] == 0 and np.isnan(r["radiance"][5, 6]).all()
    assert r["length"][10, 10] == 12
    # the filter changes what is returned, never the committed history, the length or the weight
    rf = temporal_ref(hist, **g, radiance=c1, variance=v1, reusable=[1], px_samples=pxs, filter_levels=2)
    ru = temporal_ref(hist, **g, radiance=c1, variance=v1, reusable=[1], px_samples=pxs)
    assert (rf["radiance"] != ru["radiance"]).any()
    for k in ("radiance", "variance", "length"):
        assert (rf["history"][k] == ru["history"][k])[~np.isnan(ru["history"][k])].all()
    assert (rf["length"] == ru["length"]).all() and (rf["weight"] == ru["weight"]).all()


def test_restatement_half_pixel_shift_gathers_length_and_variance_bilinearly():
    """The history's view is the new one moved by half a pixel: every new pixel gathers the
    history pixels (i - 1 .. i, j - 1 .. j) with b = 1/4 each, exactly."""
    W, H = 32, 24
    new, prev_view = quad_view(W, H), quad_view(W, H, shift=0.5)
    g, pg = quad_guides(new), quad_guides(prev_view)
    L = np.full((H, W), 8.0, F); L[10, 10] = 0.0; L[15, 20] = 24.0
    Vp = np.full((H, W), 0.5, F); Vp[15, 20] = 2.5
    hist = {"view": prev_view, "region": None, "guides": pg, "radiance": np.full((H, W, 3), 1.0, F), "variance": Vp,
            "length": L}
    zero = np.zeros((H, W), F)
    r = temporal_ref(hist, **g, radiance=np.zeros((H, W, 3), F), variance=zero, reusable=[1], samples=0)
    assert r["weight"][5, 5] == 1 and r["length"][5, 5] == 8 and r["variance"][5, 5] == F(0.5)
    assert (r["weight"][10:12, 10:12] == 0.75).all() and (r["length"][10:12, 10:12] == 8).all()   # the L = 0 tap is out
    assert (r["length"][15:17, 20:22] == 12).all() and (r["variance"][15:17, 20:22] == 1).all()  # (3 * 8 + 24) / 4
    assert r["weight"][0, 0] == 0.25 and r["weight"][0, 5] == 0.5


# ---- what the accumulation is worth -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _trial(oracle):
    return oracle_trial(oracle, scene_of("cornell"), 64, views=5, spp=4)


def test_accumulation_quality_on_oracle_cornell(oracle):
    """Cornell 64x64, depth 8, aTolerance 0: 5 views moved by k (0.125, 0.05, -0.05), 4 samples per
    view, seed 1000 + k, truth = the last view at spp 1024; frames, variances and guides from the
    oracle (tools/temporal_quality.py's first row). Display-domain MSE relative to the last
    view's fresh frame, measured (nothing is random): chained reproject 0.3587, accumulation
    0.3376, fresh + variance-guided filter 0.2142, chained reproject + filter 0.2185,
    accumulation + filter with the accumulated variance 0.1762 (asserted <= 0.1938: the
    measurement plus 10 % for a different libm sqrt in the metric)."""
    q = _trial(oracle)
    print("cornell 64x64, 5 views of 4 spp: " + ", ".join(f"{k} {v:.4f}" for k, v in q.items() if isinstance(v, float)))
    assert q["accumulated"] < 1
    assert q["accumulated_filtered"] < q["fresh_filtered"]
    assert q["accumulated_filtered"] < q["chained_filtered"]
    assert q["accumulated_filtered"] <= 0.1938
    assert q["length_ok"]                              # Lout == m where weight == 0; Lout <= max_history + m
