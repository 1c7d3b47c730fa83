"""Call-order independence of a camera's device context.

A device context keeps buffers, caches, counters and events between calls; every other GPU test makes
its calls on a fresh camera, so it pins a context's first use only. Here every probe of
tests/context_cases.py runs after every history on one long-lived camera, and each of its outputs
must equal, bit for bit, the output of the same probe on a fresh camera of the same scene and options
(computed once per probe). The fresh ref-precision render probes are also compared with the oracle,
so the expectation is not the code under test alone; the fp32 probe, which the oracle's fp32 build
does not reproduce bit for bit, is compared with the sequential fp32 kernel instead. No tolerance
appears anywhere.

One output may follow the history by design: primary_info()["used"]. A pool-kernel launch reads the
primary-ray table whenever the context holds it, so a 9-spp probe (which never builds the table)
reads it after a history that built it - with unchanged pixels, which is the point of that history.
"""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import context_cases as cc  # noqa: E402

pytestmark = pytest.mark.gpu

_fresh = {}


def fresh(rt, probe):
    if probe not in _fresh:
        cam_name, fn, _ = cc.PROBES[probe]
        out = fn(rt, cc.camera(rt, cam_name))
        for v in out.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _fresh[probe] = out
    return _fresh[probe]


def _box(a):
    x, y, w, h = cc.REGION
    return a[y:y + h, x:x + w]


def _outside_is_zero(a):
    m = np.ones(a.shape[:2], bool)
    _box(m)[...] = False
    return not a[m].any()


@pytest.mark.parametrize("probe", [p for p, c in cc.PROBES.items() if c[2] == "ref"])
def test_fresh_render_probe_is_the_oracle(rt, oracle, gpu, probe):
    cam_name, _, _ = cc.PROBES[probe]
    got = fresh(rt, probe)
    orc = oracle.render(cc.scene_of(rt, cam_name), cc.CAMERAS[cam_name][1], region=cc.REGION)
    assert np.array_equal(_box(got["rgb"]), _box(orc["rgb"]))
    assert cc.same(np.ascontiguousarray(_box(got["rad"])), np.ascontiguousarray(_box(orc["radiance"])))
    assert _outside_is_zero(got["rgb"]) and _outside_is_zero(got["rad"])
    s = orc["stats"]
    assert got["stats"] == (s["pixels"], s["samples"]["total"], s["samples"]["min"], s["samples"]["max"],
                            s["bounces"]["total"], s["bounces"]["min"], s["bounces"]["max"])
    assert got["q.last_kernel"] == cc.PROBE_KERNEL[probe] and got["q.path_ms_positive"] and got["q.pass_count"] >= 1
    if probe == "adaptive":
        rounds, rendered = got["adaptive_info"]
        assert rounds >= 1 and rendered >= s["samples"]["total"] and s["samples"]["min"] < 60


def test_fresh_fp32_probe_is_the_sequential_kernel(rt, gpu, monkeypatch):
    got = fresh(rt, "device_fp32")
    monkeypatch.setenv("RT_AMD_CHUNKED", "0")
    seq = cc.probe_device_fp32(rt, cc.camera(rt, "cornell9"))
    monkeypatch.delenv("RT_AMD_CHUNKED")
    assert got["q.last_kernel"] == "pool" and seq["q.last_kernel"] == "sequential"
    assert cc.differing({k: got[k] for k in ("rgb", "rad", "stats")}, {k: seq[k] for k in ("rgb", "rad", "stats")}) == []
    assert _box(got["rgb"]).any() and _outside_is_zero(got["rgb"]) and _outside_is_zero(got["rad"])


def test_fresh_packed_probe_is_the_oracles_tiles(rt, oracle, gpu):
    """Tile group 1 of 3 of REGION's 4 x 3 tiles: the launch's k-th tile is region tile 1 + 3k, lane
    l = 8 * row + col; lanes outside the region and the slab's other entries stay as they were."""
    got = fresh(rt, "packed")
    orc = oracle.render(cc.scene_of(rt, "cornell9"), cc.CAMERAS["cornell9"][1], region=cc.REGION)
    x0, y0, w, h = cc.REGION
    tiles_x = (w + 7) // 8
    want = {"rgb": np.zeros((cc.PACKED_TILES * 64, 3), np.uint8), "rad": np.zeros((cc.PACKED_TILES * 64, 3), cc.F),
            "pxs": np.full(cc.PACKED_TILES * 64, -1, np.int32), "pxb": np.full(cc.PACKED_TILES * 64, -1, np.int32)}
    src = {"rgb": orc["rgb"], "rad": orc["radiance"], "pxs": orc["px_samples"], "pxb": orc["px_bounces"]}
    pixels = 0
    for k, t in enumerate(range(1, cc.PACKED_TILES, 3)):
        for lane in range(64):
            i, j = (t % tiles_x) * 8 + lane % 8, (t // tiles_x) * 8 + lane // 8
            if i < w and j < h:
                pixels += 1
                for name in want:
                    want[name][k * 64 + lane] = src[name][y0 + j, x0 + i]
    assert cc.differing({k: got[k] for k in want}, want) == []
    assert got["stats"][0] == pixels and got["q.last_kernel"] == "pool"


def test_session_guide_cache_is_keyed_by_max_fuzz(rt, gpu):
    """The session probe filters with max_fuzz 0.3, then with 0 and the same max_bounces. Its second
    result must be that of a session that never walked the fuzz-0.3 guides - and differ from the first."""
    want = fresh(rt, "session")
    cam = cc.camera(rt, "mirror")
    with cam.progressive(cc.SESSION) as pr:
        pr.step(4)
        pr.step(5)
        rgb = np.zeros((cc.H, cc.W, 3), np.uint8)
        alone = pr.denoised(rgb, guides=cc.SPEC_GUIDES_0)
    assert cc.same(alone, want["dn_spec0"]) and np.array_equal(rgb, want["dn_spec0.rgb"])
    assert not cc.same(want["dn_spec0"], want["dn_spec"])


@pytest.mark.parametrize("history", sorted(cc.HISTORIES))
@pytest.mark.parametrize("probe", sorted(cc.PROBES))
def test_probe_after_history_is_the_fresh_probe(rt, gpu, monkeypatch, probe, history):
    cam_name, fn, _ = cc.PROBES[probe]
    want = fresh(rt, probe)
    cam = cc.camera(rt, cam_name)
    cc.HISTORIES[history](rt, cam, monkeypatch)
    for what in (f"after the history '{history}'", "and once more on the same camera"):
        table = cam.primary_info()
        got = fn(rt, cam)
        expect = dict(want)
        for k in [k for k in want if k.endswith("q.used")]:
            kernel = got.get(k.replace("q.used", "q.last_kernel"))
            expect[k] = want[k] or (table["built"] and table["available"] and kernel == "pool")
        assert cc.differing(got, expect) == [], what
