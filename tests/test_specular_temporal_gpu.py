"""Accumulation across views through specular chains on the GPU. Every comparison with the NumPy
restatement (tests/specular_temporal_ref.py, the normative definition) is exact: == on bits, NaN
equal to NaN - radiance, variance, length, weight, u8 and kind."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
from denoise_ref import bits_equal, oracle_guides  # noqa: E402
from guide_walk_ref import guide_walk_ref  # noqa: E402
from reproject_ref import moved_scene  # noqa: E402
from specular_reproject_ref import (PREV_REGION, REGION, cornell_without_spheres, golden_scene,  # noqa: E402
                                    mirror_room, synthetic_pair, through_from_scene)
from specular_temporal_ref import (GUIDE_KEYS, plain_history, specular_temporal_ref, synthetic_history,  # noqa: E402
                                   synthetic_variance)
from temporal_ref import accumulate_ref  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
SENT = np.float32(-123.25)
NON_DEFAULT = dict(normal_min=0.5, sigma_plane=0.05, min_weight=0.6, max_history=6.0, sigma_variance=1.5,
                   point_pixels=1.5)
OUTPUTS = ("radiance", "variance", "length", "weight")
MOVE = (0.25, 0.1, -0.1)


def _box(region, H, W):
    x, y, w, h = region or (0, 0, W, H)
    box = (slice(y, y + h), slice(x, x + w))
    mask = np.ones((H, W), bool)
    mask[box] = False
    return box, mask


def sentinels(H, W):
    return {"rgb": np.full((H, W, 3), 0xA5, np.uint8), "radiance": np.full((H, W, 3), SENT, F),
            "variance": np.full((H, W), SENT, F), "length": np.full((H, W), SENT, F), "weight": np.full((H, W), SENT, F),
            "kind": np.full((H, W), 0x5A, np.uint8)}


def assert_outputs(got, want, region, what):
    """The six outputs against `want` inside the region, their sentinels outside it."""
    H, W = want["weight"].shape
    box, mask = _box(region, H, W)
    bad = {k: int((~bits_equal(got[k][box], want[k][box])).sum()) for k in OUTPUTS}
    bad["rgb"] = int((got["rgb"][box] != want["rgb"][box]).sum())
    bad["kind"] = int((got["kind"][box] != want["kind"][box]).sum())
    counts = np.bincount(want["kind"][box].ravel(), minlength=3).tolist()
    print(f"{what}: values differing from the restatement {bad} (kind 0 / 1 / 2 on {counts} pixels)")
    assert not any(bad.values()), what
    assert (got["rgb"][mask] == 0xA5).all() and (got["kind"][mask] == 0x5A).all(), what
    assert all((got[k][mask] == SENT).all() for k in OUTPUTS), what


# ---- 1. explicit buffers, synthetic ------------------------------------------------------------------
def explicit(rt, hist, s, out, **kw):
    return rt.temporal_accumulate_specular(
        hist["radiance"], hist["variance"], hist["length"], hist["view"], hist["guides"], hist.get("chain"), s["view"],
        s["first"], s["chain"], s["reusable"], s["through"], radiance=s["fresh"], rgb=out["rgb"], out=out["radiance"],
        variance_out=out["variance"], length_out=out["length"], weight_out=out["weight"], kind=out["kind"], **kw)


def ref_call(hist, s, variance, **kw):
    return specular_temporal_ref(hist, s["view"], s["first"], s["chain"], s["fresh"], variance, s["reusable"], s["through"],
                                 **kw)


@pytest.mark.parametrize("opts,counts,levels,chain", [({}, True, 0, True), (NON_DEFAULT, False, 0, True),
                                                      ({}, False, 2, True), (NON_DEFAULT, True, 2, True),
                                                      ({}, True, 0, False)],
                         ids=["default-pxs", "non-default-scalar", "default-scalar-filter2", "non-default-pxs-filter2",
                              "no-chain-planes"])
def test_explicit_buffers_on_the_synthetic_sequence(rt, gpu, opts, counts, levels, chain):
    s = synthetic_pair()
    var = synthetic_variance(s)
    hist = {**synthetic_history(s, chain=chain), "region": PREV_REGION}
    kw = dict(region=REGION, filter_levels=levels, **opts)
    kw.update(px_samples=s["px_samples"]) if counts else kw.update(samples=3)
    reasons = {}
    want = ref_call(hist, s, var, reasons=reasons, **kw)
    H, W = s["px_samples"].shape
    box, _ = _box(REGION, H, W)
    if chain and not opts:
        assert all(v > 0 for k, v in reasons.items() if k != "no_chain_history"), reasons
        assert (want["kind"][box] == 2).mean() >= 0.05 and (want["kind"][box] == 1).mean() >= 0.2
    if not chain:
        assert reasons["no_chain_history"] > 0 and (want["kind"] < 2).all()
    out = sentinels(H, W)
    res = explicit(rt, hist, s, out, prev_region=PREV_REGION, variance=var, **kw)
    assert res is out["radiance"]
    assert_outputs(out, want, REGION, f"synthetic {opts or 'defaults'} filter {levels} chain planes {chain}")
    if levels:                                       # the filter changed the frame, not the length, weight or kind
        plain = ref_call(hist, s, var, **{**kw, "filter_levels": 0})
        assert (~bits_equal(plain["radiance"][box], want["radiance"][box])).any()
        assert bits_equal(plain["length"], want["length"]).all() and (plain["kind"] == want["kind"]).all()


def _raw_explicit(rt, hist, s, var, region, prev_region, levels, outs):
    """The raw entry with the output pointers of `outs` only."""
    from raytracer_amd import _lib
    from raytracer_amd.passes import _c_view, _region
    f32 = lambda a: np.ascontiguousarray(a, F)                                   # noqa: E731
    i32 = lambda a: np.ascontiguousarray(a, np.int32)                            # noqa: E731
    planes = lambda g, ch: ([f32(g["normal"]), f32(g["position"]), f32(g["distance"]), i32(g["object"])]   # noqa: E731
                            + ([i32(g["chain"])] if ch else []))
    keep = [*planes(s["first"], False), *planes(s["chain"], True), f32(s["fresh"]), i32(s["px_samples"]), f32(var),
            *planes(hist["guides"], False), *planes(hist["chain"], True), f32(hist["radiance"]), f32(hist["variance"]),
            f32(hist["length"]), np.ascontiguousarray(s["reusable"], np.uint8), np.ascontiguousarray(s["through"], np.uint8)]
    p = [a.ctypes.data for a in keep]
    v, pv, reg, preg = _c_view(s["view"]), _c_view(hist["view"]), _region(region), _region(prev_region)
    opts = _lib.RtSpecularTemporalOptions()
    opts.base.filter_levels = levels
    H, W = s["px_samples"].shape
    o = {k: (outs[k].ctypes.data if k in outs else None) for k in ("radiance", "variance", "length", "weight", "rgb", "kind")}
    return _lib.load().rt_temporal_accumulate_specular(
        W, H, C.byref(reg), *p[0:9], C.byref(v), p[9], p[10], 0, p[11], C.byref(pv), C.byref(preg), *p[12:21], p[21], p[22],
        p[23], p[24], p[25], len(s["reusable"]), C.byref(opts), o["radiance"], o["variance"], o["length"], o["weight"],
        o["rgb"], o["kind"])


@pytest.mark.parametrize("levels", [0, 2], ids=["unfiltered", "filter2"])
def test_each_output_alone_is_the_all_outputs_call(rt, gpu, levels):
    s = synthetic_pair()
    var = synthetic_variance(s)
    hist = synthetic_history(s)
    H, W = s["px_samples"].shape
    full = sentinels(H, W)
    assert _raw_explicit(rt, hist, s, var, REGION, PREV_REGION, levels, full) == 0
    box, _ = _box(REGION, H, W)
    assert all((a[box] != sentinels(H, W)[k][box]).any() for k, a in full.items())
    want = ref_call({**hist, "region": PREV_REGION}, s, var, region=REGION, px_samples=s["px_samples"], filter_levels=levels)
    assert_outputs(full, want, REGION, f"raw entry, filter {levels}")
    for k in full:
        one = sentinels(H, W)
        assert _raw_explicit(rt, hist, s, var, REGION, PREV_REGION, levels, {k: one[k]}) == 0, k
        assert bits_equal(one[k], full[k]).all() if k in OUTPUTS else (one[k] == full[k]).all(), (k, levels)


def test_a_9x130_frame_spans_three_workgroup_columns_and_three_row_groups(rt, gpu):
    s = synthetic_pair(False, (9, 130), (11, 120), 0.012, 0.05 * 41 / 120)
    rng = np.random.default_rng(31)
    var = (rng.random((9, 130), dtype=F) * F(0.5)).astype(F)
    hist = {"view": s["prev_view"], "region": None, "guides": s["prev_first"], "chain": s["prev_chain"],
            "guide_options": (8, 0.0), "radiance": s["prev_radiance"],
            "variance": (rng.random((11, 120), dtype=F) * F(0.5)).astype(F),
            "length": rng.integers(0, 40, (11, 120)).astype(F)}
    for levels in (0, 2):
        want = ref_call(hist, s, var, samples=3, filter_levels=levels)
        k = want["kind"]
        assert (k[:, 128:] == 2).any() and (k[:, :64] == 1).any() and (k[:, 64:128] > 0).any()
        # three row groups: rows 0-3, 4-7 and the partial third (row 8, misses: the fresh frame as it is)
        assert (k[:4] > 0).any() and (k[4:6] > 0).any() and (k[8] == 0).all()
        out = sentinels(9, 130)
        explicit(rt, hist, s, out, variance=var, samples=3, filter_levels=levels)
        assert_outputs(out, want, None, f"synthetic 9x130 filter {levels}")


# ---- 2. the session entry ------------------------------------------------------------------------------
def view_camera(rt, sd, ro, k, move=MOVE, seed=None):
    """View k of a path: `from` moved by k * move, seed 1 + k."""
    return rt.create_camera_from_scene_data(moved_scene(sd, tuple(k * m for m in move)),
                                            {**ro, "seed": (1 + k) if seed is None else seed})


def oracle_planes(oracle, sd, ro, k, go, move=MOVE):
    """View k's first-hit guides from the oracle and its chain guides from guide_walk_ref."""
    sk = moved_scene(sd, tuple(k * m for m in move))
    gro = {kk: v for kk, v in ro.items() if kk in ("width", "aspect")}
    gro["samples"] = 4
    first = dict(zip(GUIDE_KEYS, oracle_guides(oracle, sk, gro)[:4]))
    chain = dict(zip(GUIDE_KEYS + ("chain",), guide_walk_ref(oracle, sk, gro, *go)))
    return first, chain


def _step(cam, pr, n):
    H, W = cam.image_height, cam.image_width
    rgb = np.zeros((H, W, 3), np.uint8)
    rad = np.zeros((H, W, 3), np.float32)
    pxs = np.zeros((H, W), np.int32)
    st = pr.step(n, rgb, radiance=rad, px_samples=pxs)
    return rgb, rad, pxs, st


def accumulate(pr, history, H, W, plain=False, **kw):
    out = sentinels(H, W)
    if plain:
        out.pop("kind")
    else:
        kw.setdefault("guides", "specular")
        kw["kind"] = out["kind"]
    res = pr.accumulated(history, out["rgb"], out["radiance"], variance_out=out["variance"], length_out=out["length"],
                         weight_out=out["weight"], **kw)
    assert res is out["radiance"]
    return out


def assert_history(history, ref_hist, views, what):
    i = history.info
    H, W = i["height"], i["width"]
    box, mask = _box(ref_hist["region"], H, W)
    got = history.read()
    assert i["views"] == history.views == views and i["region"] == tuple(ref_hist["region"]) and i["bytes"] > 0, what
    for k in ("radiance", "variance", "length"):
        assert bits_equal(got[k][box], ref_hist[k][box]).all(), f"{what}: history {k}"
        assert (got[k][mask] == 0).all(), what
    for k in ("center", "pixel00", "du", "dv"):
        assert i["view"][k].tobytes() == np.asarray(ref_hist["view"][k], F).tobytes(), what
    go = ref_hist.get("guide_options")
    assert history.chain_guides == (None if go is None else {"max_bounces": go[0], "max_fuzz": go[1]}), what


SESSION_CASES = {
    "mirror-room40": (mirror_room, {"width": 40, "samples": 60, "depth": 8}, "specular", (8, 0.0), None),
    "default40x23": (lambda: golden_scene("default"), {"width": 40, "samples": 60, "depth": 8},
                     {"max_bounces": 6, "max_fuzz": 0.5}, (6, 0.5), None),
    "mirror-room40-regions": (mirror_room, {"width": 40, "samples": 60, "depth": 8}, "specular", (8, 0.0),
                              [(2, 1, 36, 37), (5, 3, 29, 31), (0, 4, 33, 30)]),
}


@pytest.mark.parametrize("case", list(SESSION_CASES))
def test_session_entry_follows_the_restatement_along_three_views(rt, gpu, oracle, case):
    make, ro, guides, go, regions = SESSION_CASES[case]
    sd = make()
    reus = None
    ref_hist, prev = None, None
    with rt.History() as history:
        for k in range(3):
            cam = view_camera(rt, sd, ro, k)
            H, W = cam.image_height, cam.image_width
            if case == "default40x23":
                assert (H, W) == (23, 40)
            region = regions[k] if regions else None
            box, _ = _box(region, H, W)
            first, chain = oracle_planes(oracle, sd, ro, k, go)
            reus = cam.reusable_objects()
            thr = through_from_scene(sd, 15, go[1])
            assert thr.tolist() == cam.through_objects(15, go[1]).tolist()
            with cam.progressive(region) as pr:
                _step(cam, pr, 10)
                _, rad, pxs, _ = _step(cam, pr, 10)
                var = pr.variance()
                if prev is not None:
                    prev.close()                     # the history needs neither the previous camera nor its session
                kw = dict(guide_options=go, px_samples=pxs, region=region)
                if k == 2:                           # the filtered frame first, uncommitted
                    want = specular_temporal_ref(ref_hist, cam.view(), first, chain, rad, var, reus, thr, filter_levels=2, **kw)
                    got = accumulate(pr, history, H, W, guides=guides, commit=False, filter_levels=2)
                    assert_outputs(got, want, region, f"{case} view {k} filter 2")
                    assert history.views == 2
                want = specular_temporal_ref(ref_hist, cam.view(), first, chain, rad, var, reus, thr, **kw)
                ref_hist = want["history"]
                got = accumulate(pr, history, H, W, guides=guides)
                assert_outputs(got, want, region, f"{case} view {k}")
                if k:
                    on = want["kind"][box] == 2
                    assert on.any() and (want["kind"][box] == 1).any()
                    assert (want["length"][box][on] > pxs[box][on]).all()
                else:
                    assert (want["weight"] == 0).all() and bits_equal(want["radiance"][box], rad[box]).all()
                assert_history(history, ref_hist, k + 1, f"{case} view {k}")
            prev = cam
        t = history.times()
        assert t["guide_ms"] > 0 and t["gather_ms"] > 0 and t["filter_ms"] == 0
        assert t["total_ms"] >= t["guide_ms"] + t["gather_ms"]


# ---- 3. commit semantics, mixing, the session ---------------------------------------------------------------
SESSION_RO = {"width": 40, "samples": 60, "depth": 8}   # the reference's adaptive defaults


def test_commit_false_mixing_and_the_untouched_session(rt, gpu):
    sd = mirror_room()
    cam0, cam = view_camera(rt, sd, SESSION_RO, 0), view_camera(rt, sd, SESSION_RO, 1)
    plain = view_camera(rt, sd, SESSION_RO, 1)                   # a session that never accumulates
    k1 = cam.render_guides(through_specular=True)["chain"] & 0xff >= 1
    assert 0.1 < k1.mean() < 0.6
    with rt.History() as history, rt.History() as h2, cam.progressive() as pr, plain.progressive() as pq:
        assert history.chain_guides is None
        with cam0.progressive() as p0:
            _step(cam0, p0, 10)
            accumulate(p0, history, 40, 40)
        assert history.chain_guides == {"max_bounces": 8, "max_fuzz": 0.0}
        bytes_spec = history.info["bytes"]
        _step(cam, pr, 10); _step(plain, pq, 10)
        _, rad, pxs, _ = _step(cam, pr, 10); _step(plain, pq, 10)
        assert sorted(int(v) for v in np.unique(pxs)) == [10, 20]    # an adaptive session: two sample counts
        blob = pr.save()
        before, info = history.read(), history.info
        # commit=False, twice: identical outputs, the history as it was
        a = accumulate(pr, history, 40, 40, commit=False)
        b = accumulate(pr, history, 40, 40, commit=False)
        assert all(bits_equal(a[k], b[k]).all() for k in a) and (a["kind"] == 2).any() and (a["kind"] == 1).any()
        assert set(np.unique(a["kind"][k1])) <= {0, 2} and set(np.unique(a["kind"][~k1])) <= {0, 1}
        after, i2 = history.read(), history.info
        assert all(bits_equal(before[k], after[k]).all() for k in before)
        assert i2["views"] == 1 and all(np.array_equal(i2[k], info[k]) for k in info if k not in ("view", "bytes"))
        assert history.chain_guides == {"max_bounces": 8, "max_fuzz": 0.0}
        assert pr.save() == blob
        # other guide options: the history's chain planes do not serve; k == 0 pixels are what they were
        o = accumulate(pr, history, 40, 40, guides={"max_bounces": 6}, commit=False)
        assert (o["kind"][k1] == 0).all() and (o["length"][k1] == pxs[k1]).all()
        assert all(bits_equal(o[k][~k1], a[k][~k1]).all() for k in a)
        # a plain call on the same history is temporal_ref's, and its commit holds no chain planes
        hist_ref = {"view": cam0.view(), "region": (0, 0, 40, 40), "guides": cam0.render_guides(), **before}
        want, _ = accumulate_ref(hist_ref, cam.view(), cam.render_guides(), rad, pr.variance(), cam.reusable_objects(),
                                 px_samples=pxs)
        p = accumulate(pr, history, 40, 40, plain=True)
        assert all(bits_equal(p[k], want[k]).all() for k in OUTPUTS) and (p["rgb"] == want["rgb"]).all()
        assert (p["weight"][k1] == 0).all() and history.views == 2 and history.chain_guides is None
        # plain, then specular: no chain planes to use; the call commits its own
        o = accumulate(pr, history, 40, 40)
        assert (o["kind"][k1] == 0).all() and (o["kind"][~k1] == 1).any() and history.views == 3
        assert history.chain_guides == {"max_bounces": 8, "max_fuzz": 0.0}
        # specular with other guide options after that commit, then a matching one
        o = accumulate(pr, history, 40, 40, guides={"max_fuzz": 0.25})
        assert (o["kind"][k1] == 0).all() and history.chain_guides == {"max_bounces": 8, "max_fuzz": 0.25}
        o = accumulate(pr, history, 40, 40, guides={"max_fuzz": 0.25}, commit=False)
        assert (o["kind"][k1] == 2).any()
        # the session is as it was; a plain call on a second history is temporal_ref's
        assert pr.save() == blob and pr.samples_done == 20 and pr.steps == 2
        p2 = accumulate(pr, h2, 40, 40, plain=True)
        w2, _ = accumulate_ref(None, cam.view(), cam.render_guides(), rad, pr.variance(), cam.reusable_objects(),
                               px_samples=pxs)
        assert all(bits_equal(p2[k], w2[k]).all() for k in OUTPUTS)
        assert h2.info["bytes"] < bytes_spec and h2.chain_guides is None   # no chain planes were ever allocated
        rgb_p, rad_p, pxs_p, st_p = _step(cam, pr, 10)
        rgb_q, rad_q, pxs_q, st_q = _step(plain, pq, 10)
        assert (rgb_p == rgb_q).all() and bits_equal(rad_p, rad_q).all() and (pxs_p == pxs_q).all()
        assert (st_p.pixels, st_p.samples, st_p.bounces) == (st_q.pixels, st_q.samples, st_q.bounces)
        assert pr.save() == pq.save()


def test_one_history_fed_by_plain_and_specular_calls_follows_both_restatements(rt, gpu, oracle):
    """The session body the two accumulate entries share: one history over four views of the 16x16
    mirror room - a plain commit, a specular commit, a specular commit=False, a plain commit - with
    every output requested. Each call's outputs and the history's planes are the restatements' in
    every bit; the chain planes are held after the specular commit only."""
    sd, ro, go = mirror_room(), {"width": 16, "samples": 60, "depth": 8}, (8, 0.0)
    ref_hist, views, sizes, held = None, 0, [], []
    with rt.History() as history:
        for k, (plain, commit) in enumerate([(True, True), (False, True), (False, False), (True, True)]):
            cam = view_camera(rt, sd, ro, k)
            H, W = cam.image_height, cam.image_width
            assert (H, W) == (16, 16)
            first, chain = oracle_planes(oracle, sd, ro, k, go)
            reus, thr = cam.reusable_objects(), cam.through_objects(15, go[1])
            with cam.progressive() as pr:
                _step(cam, pr, 10)
                _, rad, pxs, _ = _step(cam, pr, 10)
                var = pr.variance()
                if plain:
                    want, committed = accumulate_ref(ref_hist and plain_history(ref_hist), cam.view(), first, rad, var, reus,
                                                     px_samples=pxs)
                else:
                    want = specular_temporal_ref(ref_hist, cam.view(), first, chain, rad, var, reus, thr, guide_options=go,
                                                 px_samples=pxs)
                    committed = want["history"]
                got = accumulate(pr, history, H, W, plain=plain, commit=commit)
            what = f"view {k} ({'plain' if plain else 'specular'}, commit {commit})"
            if plain:
                bad = {o: int((~bits_equal(got[o], want[o])).sum()) for o in OUTPUTS}
                bad["rgb"] = int((got["rgb"] != want["rgb"]).sum())
                print(f"{what}: values differing from the restatement {bad}")
                assert not any(bad.values()), what
            else:
                assert_outputs(got, want, None, what)
            if k == 2:                               # the specular commit's chain planes served
                assert (want["kind"] == 2).any() and (want["kind"] == 1).any()
            if commit:
                ref_hist, views = committed, views + 1
            # (chain_guides: None, the options, unchanged by commit=False, None again)
            assert_history(history, ref_hist, views, what)
            t = history.times()
            assert len(t) == 4 and all(np.isfinite(v) and v >= 0 for v in t.values()), (what, t)
            sizes.append(history.info["bytes"])
            held.append(history.chain_guides)
            cam.close()
    assert views == 3 and held == [None, {"max_bounces": 8, "max_fuzz": 0.0}, {"max_bounces": 8, "max_fuzz": 0.0}, None]
    assert sizes[0] < sizes[1] == sizes[2] == sizes[3], sizes     # the chain planes: the first specular commit alone


def test_without_specular_materials_the_call_and_the_history_are_the_plain_ones(rt, gpu):
    sd = cornell_without_spheres()
    ro = {"width": 40, "samples": 8, "depth": 8, "aTolerance": 0}
    with rt.History() as ha, rt.History() as hb:
        for k in range(3):
            cam = view_camera(rt, sd, ro, k)
            assert not cam.through_objects().any()
            with cam.progressive() as pr:
                pr.step(4)
                levels = 2 if k == 2 else 0
                a = accumulate(pr, ha, 40, 40, plain=True, filter_levels=levels)
                b = accumulate(pr, hb, 40, 40, filter_levels=levels)
                assert all(bits_equal(a[key], b[key]).all() for key in a)
                assert ((b["kind"] == 1) == (a["weight"] > 0)).all() and (b["kind"] < 2).all()
                ra, rb = ha.read(), hb.read()
                assert all(bits_equal(ra[key], rb[key]).all() for key in ra)
        assert (a["weight"] > 0).mean() > 0.5


def test_the_history_survives_its_cameras_and_release_device(rt, gpu):
    sd = mirror_room()
    ro = {"width": 40, "samples": 8, "depth": 8, "aTolerance": 0}

    def run(history, release):
        outs = []
        for k in range(3):
            cam = view_camera(rt, sd, ro, k)
            with cam.progressive() as pr:
                pr.step(4)
                outs.append(accumulate(pr, history, 40, 40, filter_levels=2 if k == 2 else 0))
            if release:
                cam.release_device()                 # frees the camera's buffers, not the history's
            cam.close()
        return outs, history.read()

    with rt.History() as ha, rt.History() as hb:
        (oa, ra), (ob, rb) = run(ha, False), run(hb, True)
        for a, b in zip(oa, ob):
            assert all(bits_equal(a[k], b[k]).all() for k in a)
        assert all(bits_equal(ra[k], rb[k]).all() for k in ra)
        assert (oa[2]["kind"] == 2).any() and ha.info["bytes"] == hb.info["bytes"] > 0
        t = ha.times()
        assert t["filter_ms"] > 0 and t["total_ms"] >= t["guide_ms"] + t["gather_ms"] + t["filter_ms"]
    with pytest.raises(ValueError):
        ha.chain_guides


# ---- 4. errors on an open session --------------------------------------------------------------------------
def test_session_errors(rt, gpu):
    from raytracer_amd import _lib
    sd = mirror_room()
    sp = dict(guides="specular")
    with rt.History() as history:
        for mode in ("bounces", "samples"):
            cam = rt.create_camera_from_scene_data(sd, {**SESSION_RO, "mode": mode})
            with cam.progressive() as pr:
                pr.step(4)
                with pytest.raises(rt.RtError, match="not radiance") as e:
                    pr.accumulated(history, **sp)
                assert e.value.code == _lib.RT_ERR_INVALID
        cam = rt.create_camera_from_scene_data(sd, SESSION_RO)
        other = rt.create_camera_from_scene_data(golden_scene("default"), {"width": 40, "samples": 60})
        with pytest.raises(rt.RtError, match="no progressive session is open"):
            rt.ProgressiveRender(cam).accumulated(history, **sp)
        with cam.progressive() as pr:
            pr.step(1)
            with pytest.raises(rt.RtError, match="samples_done < 2") as e:
                pr.accumulated(history, **sp)
            assert e.value.code == _lib.RT_ERR_INVALID and history.views == 0
            pr.step(3)
            for kw, word in (({"sigma_plane": -1.0, **sp}, "sigma_plane"), ({"point_pixels": float("nan"), **sp}, "point_pixels"),
                             ({"through": 16, **sp}, "through"), ({"filter_levels": 9, **sp}, "filter_levels"),
                             ({"guides": "first_hit"}, "RT_GUIDES_SPECULAR"), ({"guides": {"max_bounces": 65}}, "max_bounces")):
                with pytest.raises(rt.RtError, match=word) as e:
                    pr.accumulated(history, **kw)
                assert e.value.code == _lib.RT_ERR_INVALID
            assert history.views == 0 and history.chain_guides is None
            assert np.isfinite(pr.accumulated(history, **sp)).all() and history.views == 1
            with other.progressive() as po:
                po.step(4)
                with pytest.raises(rt.RtError, match="temporal: the history holds a different scene") as e:
                    po.accumulated(history, **sp)
                assert e.value.code == _lib.RT_ERR_INVALID
            assert history.views == 1
            assert np.isfinite(pr.accumulated(history, **sp)).all() and history.views == 2   # the session still works
            pr.step(4)


def test_a_history_committed_on_another_device_is_refused(rt, gpu):
    """The history records the device of its first commit; a session on another device is refused on
    the host. Needs two visible devices to commit on one and call from the other; with one device
    the history's recorded id is checked alone."""
    from raytracer_amd import _lib
    sd = mirror_room()
    ro = {"width": 40, "samples": 8, "depth": 8, "aTolerance": 0}
    hip = C.CDLL("libamdhip64.so.7")
    last = gpu - 1
    print(f"{gpu} visible device(s): the history is committed on device {last}")
    with rt.History() as history:
        try:
            assert hip.hipSetDevice(last) == 0
            cam = view_camera(rt, sd, ro, 0)
            with cam.progressive() as pr:
                pr.step(4)
                pr.accumulated(history, guides="specular")
            assert history.info["device"] == last and history.views == 1
        finally:
            assert hip.hipSetDevice(0) == 0
        if last != 0:
            cam = view_camera(rt, sd, ro, 1)
            with cam.progressive() as pr:
                pr.step(4)
                with pytest.raises(rt.RtError, match="the history was committed on another device") as e:
                    pr.accumulated(history, guides="specular")
                assert e.value.code == _lib.RT_ERR_INVALID and history.views == 1
