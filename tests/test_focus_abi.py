"""Focused progressive steps, host side: the ABI surface, the restatement (tests/focus_ref.py, the
normative definition of the selection) against a brute-force loop, and the argument errors that
are decided without a device. The errors that need an open session (mode, samples_done < 2, a
mismatching history, the sample index overflow) are in tests/test_focus_gpu.py."""
import ctypes as C
import json
import re
import struct
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
from focus_ref import sanitise, select  # noqa: E402

GOLDEN = Path(__file__).resolve().parent / "golden"

DECLARED = {
    "rt_focus_options_default": ("void", "(rt_focus_options* options)"),
    "rt_camera_progressive_focus": ("int", "(rt_camera* cam, int32_t n_samples, const rt_focus_options* options, "
                                           "const float* score, rt_history* h, uint8_t* rgb, float* radiance, "
                                           "int32_t* px_samples, int32_t* px_bounces, uint8_t* selected_out, "
                                           "rt_render_stats* stats, rt_focus_info* info)"),
}


def scene_of(name):
    return json.loads((GOLDEN / f"scene_{name}.json").read_text())["scene"]


def test_focus_symbols_are_declared_exported_and_bound(rt):
    from raytracer_amd import _lib
    lib = _lib.load()
    text = re.sub(r"\s+", " ", _lib.HEADER.read_text())
    assert "typedef struct { int32_t source, permille; float min_score; int32_t max_pixels; } rt_focus_options;" in text
    for name, (res, args) in DECLARED.items():
        assert f"{res} {name}{args};" in text, f"{name} is not declared as proposed"
        assert hasattr(lib, name), f"{name} is not exported"
        restype, argtypes = _lib._SIGS[name]
        assert restype is (C.c_int if res == "int" else None) and len(argtypes) == args.count(",") + 1
    assert C.sizeof(_lib.RtFocusOptions) == 16 and C.sizeof(_lib.RtFocusInfo) == 40
    assert lib.rt_version() == 3                       # functions were added, nothing changed
    # rt_progressive_info keeps its layout
    assert C.sizeof(_lib.RtProgressiveInfo) == 88
    assert ("int32_t samples_done; /* samples every unfinished pixel holds */ int32_t samples;" in text
            and "uint64_t state_bytes; /* per-pixel state: the payload of a checkpoint blob */ char build_id[24];" in text)
    assert hasattr(rt.ProgressiveRender, "focus") and isinstance(rt.ProgressiveRender.focus_info, property)
    assert "a focused session cannot be saved" in text


def test_options_default(rt):
    from raytracer_amd import _lib
    lib = _lib.load()
    o = _lib.RtFocusOptions(9, 9, 9.0, 9)
    lib.rt_focus_options_default(C.byref(o))
    assert (o.source, o.permille, o.min_score, o.max_pixels) == (_lib.FOCUS_SCORE_VARIANCE, 250, 0.0, 0)
    assert (_lib.FOCUS_SCORE_VARIANCE, _lib.FOCUS_SCORE_MAP, _lib.FOCUS_SCORE_HISTORY) == (0, 1, 2)
    lib.rt_focus_options_default(None)                  # harmless
    import inspect
    sig = inspect.signature(rt.ProgressiveRender.focus)
    assert [sig.parameters[k].default for k in ("score", "permille", "min_score", "max_pixels")] == [None, 250, 0.0, 0]


# ---- the restatement against a brute-force loop ---------------------------------------------------
def brute(score, active, permille, min_score, max_pixels):
    """The definition, one pixel at a time, on Python floats and struct-packed bit patterns."""
    def pattern(v):
        return struct.unpack("<I", struct.pack("<f", v))[0]
    min_score = float(np.float32(min_score))           # the option is a float
    flat, act = np.asarray(score, np.float32).ravel(), np.asarray(active, bool).ravel()
    vals = []
    for v in flat:
        v = float(v)
        vals.append(v if (v >= 0 and v != float("inf") and v == v) else 0.0)
    elig = [i for i in range(len(vals)) if act[i] and vals[i] > min_score]
    k = (int(act.sum()) * permille + 999) // 1000
    if max_pixels > 0:
        k = min(k, max_pixels)
    if not elig:
        return set(), 0, 0
    ranked = sorted((pattern(vals[i]) for i in elig), reverse=True)
    t = ranked[min(k, len(ranked)) - 1]
    return {i for i in elig if pattern(vals[i]) >= t}, t, len(elig)


def _maps(rng, n):
    e = rng.random(n, dtype=np.float32)
    special = e.copy()
    special[:12] = [np.nan, np.inf, -np.inf, -1.0, -0.0, 0.0, 1e-45, 3e-39, 1e-38, -1e-45, 3.0e38, 1.0]
    lo = (np.uint32(0x3f800000) + rng.integers(0, 1 << 16, n, dtype=np.uint32)).view(np.float32)
    hi = (rng.integers(1, 0x7f7f, n, dtype=np.uint32) << np.uint32(16)).view(np.float32)
    return {"random": e, "equal": np.full(n, 0.25, np.float32), "zero": np.zeros(n, np.float32), "special": special,
            "low16": lo, "high16": hi, "few": np.where(np.arange(n) % 7 == 0, e, 0).astype(np.float32)}


@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (9, 13)])
def test_restatement_equals_the_brute_force_loop(shape):
    rng = np.random.default_rng(7)
    n = shape[0] * shape[1]
    for name, m in _maps(rng, max(n, 12)).items():
        m = m[:n].reshape(shape)
        for active in (np.ones(shape, bool), rng.random(shape) < 0.6):
            for permille, min_score, max_pixels in [(250, 0.0, 0), (1, 0.0, 0), (1000, 0.0, 0), (500, 0.0, 1),
                                                    (250, 0.5, 0), (999, 1e-38, 3)]:
                r = select(m, active, permille, min_score, max_pixels)
                want, t, ne = brute(m, active, permille, min_score, max_pixels)
                got = set(np.flatnonzero(r["mask"].ravel()).tolist())
                what = (name, shape, permille, min_score, max_pixels)
                assert got == want, what
                assert r["eligible"] == ne and r["selected"] == len(want) and r["active"] == int(active.sum()), what
                assert int(np.float32(r["threshold"]).view(np.uint32)) == t, what
                assert r["selected"] >= min(r["k"], ne), what        # ties only ever add
                if name == "equal" and min_score < 0.25:
                    assert r["selected"] == r["active"], what         # ties select everyone, whatever K is
                if name == "zero":
                    assert r["selected"] == 0 and r["threshold"] == 0, what


def test_restatement_properties():
    s = sanitise(np.array([np.nan, np.inf, -np.inf, -2.0, 1e-45, 0.5], np.float32))
    assert s.tolist() == [0, 0, 0, 0, float(np.float32(1e-45)), 0.5]
    m = np.array([[4.0, 3.0, 3.0, 1.0, 0.0, 9.0]], np.float32)
    on = np.array([[1, 1, 1, 1, 1, 0]], bool)
    r = select(m, on, permille=400)                     # K = 2 of 5 active: T = 3, the tie is taken
    assert r["k"] == 2 and r["threshold"] == 3 and r["mask"].tolist() == [[True, True, True, False, False, False]]
    assert (r["active"], r["eligible"], r["selected"]) == (5, 4, 3)
    r = select(m, on, permille=1000)                    # the zero score is never chosen
    assert r["selected"] == 4 and r["threshold"] == 1
    r = select(m, on, permille=1000, max_pixels=1)
    assert r["mask"].tolist() == [[True, False, False, False, False, False]]
    r = select(m, on, min_score=3.0)                    # strictly above
    assert r["eligible"] == 1 and r["mask"].tolist() == [[True, False, False, False, False, False]]
    r = select(m, np.zeros((1, 6), bool))
    assert (r["active"], r["selected"], r["k"]) == (0, 0, 0)
    # the selected set does not depend on the order of the pixels
    rng = np.random.default_rng(3)
    v = rng.random(200, dtype=np.float32).round(1)
    p = rng.permutation(200)
    a, b = select(v, np.ones(200, bool), 100), select(v[p], np.ones(200, bool), 100)
    assert (a["mask"][p] == b["mask"]).all() and a["threshold"] == b["threshold"]


# ---- errors that need no device -------------------------------------------------------------------
BAD = [({"n": 0}, "n_samples"), ({"n": -3}, "n_samples"), ({"n": 65536}, "n_samples"),
       ({"permille": 0}, "permille"), ({"permille": 1001}, "permille"), ({"permille": -5}, "permille"),
       ({"min_score": -0.5}, "min_score"), ({"min_score": float("nan")}, "min_score"),
       ({"min_score": float("inf")}, "min_score"), ({"max_pixels": -1}, "max_pixels")]


@pytest.mark.parametrize("kw,word", BAD)
def test_bad_arguments_are_invalid_without_a_device(rt, kw, word):
    from raytracer_amd import _lib
    cam = rt.create_camera_from_scene_data(scene_of("cornell"), {"width": 16, "samples": 4, "depth": 4})
    kw = dict(kw)
    n = kw.pop("n", 4)
    with pytest.raises(rt.RtError, match=word) as e:
        rt.ProgressiveRender(cam).focus(n, **kw)
    assert e.value.code == _lib.RT_ERR_INVALID
    assert "rt_camera_progressive_focus" in str(e.value)


def test_missing_sources_no_session_and_no_camera_without_a_device(rt):
    from raytracer_amd import _lib
    lib = _lib.load()
    cam = rt.create_camera_from_scene_data(scene_of("cornell"), {"width": 16, "samples": 4, "depth": 4})
    st, info = _lib.RtRenderStats(), _lib.RtFocusInfo()

    def raw(opts, score=None, h=None, c=cam._h):
        return lib.rt_camera_progressive_focus(c, 4, C.byref(opts) if opts is not None else None, score, h, None, None,
                                               None, None, None, C.byref(st), C.byref(info))

    assert raw(_lib.RtFocusOptions(_lib.FOCUS_SCORE_MAP, 250, 0.0, 0)) == _lib.RT_ERR_INVALID
    assert b"the score map is required" in lib.rt_last_error()
    assert raw(_lib.RtFocusOptions(_lib.FOCUS_SCORE_HISTORY, 250, 0.0, 0)) == _lib.RT_ERR_INVALID
    assert b"the history is required" in lib.rt_last_error()
    assert raw(_lib.RtFocusOptions(7, 250, 0.0, 0)) == _lib.RT_ERR_INVALID
    assert b"source must be one of RT_FOCUS_SCORE_" in lib.rt_last_error()
    # valid arguments, NULL options (the defaults) included: no session
    for opts in (None, _lib.RtFocusOptions(_lib.FOCUS_SCORE_VARIANCE, 250, 0.0, 0)):
        assert raw(opts) == _lib.RT_ERR_INVALID
        assert b"rt_camera_progressive_focus: no progressive session is open" in lib.rt_last_error()
    with rt.History() as h:
        assert raw(_lib.RtFocusOptions(_lib.FOCUS_SCORE_HISTORY, 250, 0.0, 0), h=h._h) == _lib.RT_ERR_INVALID
        assert b"no progressive session is open" in lib.rt_last_error()
        with pytest.raises(rt.RtError, match="no progressive session is open"):
            rt.ProgressiveRender(cam).focus(4, score=h)
    with pytest.raises(rt.RtError, match="no progressive session is open") as e:
        rt.ProgressiveRender(cam).focus(4, score=np.ones((16, 16), np.float32))
    assert e.value.code == _lib.RT_ERR_INVALID
    assert raw(None, c=None) == _lib.RT_ERR_INVALID
    pr = rt.ProgressiveRender(cam)
    assert pr.focus_info is None
    pr.close()
    with pytest.raises(ValueError):
        pr.focus(4)
