"""Focused progressive steps on the GPU (rt_camera_progressive_focus). The selection is compared
exactly with its NumPy restatement (tests/focus_ref.py); the frames exactly with the CPU oracle,
with one-shot renders and with plain sessions - but for the one radiance check of case 3, whose
bound is derived beside it."""
import functools
import json
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
from denoise_ref import bits_equal  # noqa: E402
from denoise_var_ref import blob_pixels, variance_from_blob  # noqa: E402
from focus_ref import select  # noqa: E402
from temporal_ref import accumulate_ref  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
CORNELL = {"type": "cornell"}
SPHERES50 = {"type": "spheres", "options": {"count": 50, "seed": 42}}
SPHERES200 = {"type": "spheres", "options": {"count": 200, "seed": 3}}
FIXED = {"depth": 4, "aTolerance": 0}
SENT = 0xA5


@functools.lru_cache(maxsize=None)
def _scene(rt, key):
    return rt.generate_scene_data(json.loads(key))


def scene(rt, cfg):
    return _scene(rt, json.dumps(cfg, sort_keys=True))


def camera(rt, cfg, ro):
    return rt.create_camera_from_scene_data(scene(rt, cfg), ro)


class Out:
    """Caller-owned full-frame buffers of a step or a focused step."""

    def __init__(self, cam):
        H, W = cam.image_height, cam.image_width
        self.rgb = np.zeros((H, W, 3), np.uint8)
        self.rad = np.zeros((H, W, 3), F)
        self.pxs = np.zeros((H, W), np.int32)
        self.pxb = np.zeros((H, W), np.int32)
        self.sel = np.full((H, W), SENT, np.uint8)
        self.stats = None

    def step(self, pr, n):
        self.stats = pr.step(n, self.rgb, radiance=self.rad, px_samples=self.pxs, px_bounces=self.pxb)
        return self

    def focus(self, pr, n, **kw):
        self.sel[...] = SENT
        self.stats = pr.focus(n, self.rgb, self.rad, self.pxs, self.pxb, self.sel, **kw)
        return self

    def mask(self):
        assert set(np.unique(self.sel).tolist()) <= {0, 1, SENT}
        return self.sel == 1

    def copy(self):
        import copy
        return copy.deepcopy(self)


def same_frames(a, b, where=None):
    w = np.ones(a.pxs.shape, bool) if where is None else where
    return bool((a.rgb[w] == b.rgb[w]).all() and bits_equal(a.rad[w], b.rad[w]).all() and (a.pxs[w] == b.pxs[w]).all()
                and (a.pxb[w] == b.pxb[w]).all())


def same_stats(a, b):
    return (a.pixels, a.samples, a.bounces) == (b.pixels, b.samples, b.bounces)


def box_of(region, H, W):
    x, y, w, h = region or (0, 0, W, H)
    return (slice(y, y + h), slice(x, x + w))


# ---- 1. the selection, exact against focus_ref ------------------------------------------------------
SEL_CASES = {
    "70x50": ({"width": 70, "aspect": 70 / 49.5}, None, (50, 70)),          # partial 8x8 tiles, > 1 workgroup
    "9x130": ({"width": 9, "aspect": 9 / 129.5}, None, (130, 9)),
    "sub-of-64x48": ({"width": 64, "aspect": 64 / 47.5}, (3, 5, 41, 23), (48, 64)),
    "5x3": ({"width": 16, "aspect": 1}, (2, 1, 5, 3), (16, 16)),           # fewer than 64 active pixels
}


def score_maps(shape, rng):
    """name -> (region-shaped map, focus keywords)."""
    n = shape[0] * shape[1]
    rnd = (rng.random(shape, dtype=F) + F(0.01)).astype(F)
    special = rnd.copy().ravel()
    bad = [np.nan, np.inf, -np.inf, -1.0, -0.0, 1e-45, 3e-39, 1.1e-38, -1e-45, -np.nan]
    special[rng.permutation(n)[:len(bad)]] = np.array(bad, F)
    low16 = (np.uint32(0x3f800000) + rng.integers(0, 1 << 16, shape, dtype=np.uint32)).view(F)
    high16 = (rng.integers(1, 0x7f7f, shape, dtype=np.uint32) << np.uint32(16)).view(F)
    holes = np.where(rng.random(shape) < 0.3, F(0), rnd).astype(F)
    return {
        "random": (rnd, {}),
        "equal": (np.full(shape, 0.25, F), {"permille": 1}),               # ties select everyone whatever K is
        "zero": (np.zeros(shape, F), {}),
        "special": (special.reshape(shape), {"permille": 900}),
        "low16": (low16, {"permille": 100}),
        "high16": (high16, {"permille": 500}),
        "k=1": (rnd, {"max_pixels": 1}),
        "permille=1000": (holes, {"permille": 1000}),
        "min_score": (rnd, {"permille": 1000, "min_score": float(np.sort(rnd.ravel())[(2 * n) // 3])}),
    }


def assert_selection(pr, out, score_region, active_region, region, kw, what):
    """out.sel and pr.focus_info against the restatement of (score, active) over the region."""
    H, W = out.sel.shape
    box = box_of(region, H, W)
    want = select(score_region, active_region, **kw)
    got, info = out.mask(), pr.focus_info
    outside = np.ones((H, W), bool)
    outside[box] = False
    n_bad = int((got[box] != want["mask"]).sum())
    print(f"{what}: K {want['k']}, active {info['active']}, eligible {info['eligible']}, selected {info['selected']} "
          f"(restatement {want['selected']}), T {info['threshold']!r}, {n_bad} mask pixels differ, "
          f"selection {info['select_ms']:.3f} ms")
    assert n_bad == 0 and (out.sel[outside] == SENT).all() and not (out.sel[box] == SENT).any(), what
    assert (info["active"], info["eligible"], info["selected"]) == (want["active"], want["eligible"], want["selected"]), what
    assert F(info["threshold"]).view(np.uint32) == F(want["threshold"]).view(np.uint32), what
    return want


@pytest.mark.parametrize("case", list(SEL_CASES))
def test_selection_equals_the_restatement(rt, gpu, case):
    ro, region, (H, W) = SEL_CASES[case]
    cam = camera(rt, CORNELL, {**ro, **FIXED, "samples": 64})
    assert (cam.image_height, cam.image_width) == (H, W)
    x, y, w, h = region or (0, 0, W, H)
    rng = np.random.default_rng(11)
    on = np.ones((h, w), bool)
    with cam.progressive(region) as pr:
        out = Out(cam).step(pr, 2)
        done = 0
        for name, (m, kw) in score_maps((h, w), rng).items():
            before, steps = out.copy(), pr.steps
            assert pr.active_pixels == w * h                             # 64 samples, no tolerance: nobody retires
            score = m
            if name == "random":                                         # a full-frame map is cut to the region
                score = np.full((H, W), 7.0, F)
                score[y:y + h, x:x + w] = m
            out.focus(pr, 1, score=score, **kw)
            want = assert_selection(pr, out, m, on, region, kw, f"{case} {name}")
            info = pr.focus_info
            assert info["first_sample"] == 64 + done
            if name == "zero":                                           # nothing eligible: RT_OK, nothing changes
                assert want["selected"] == 0 and info["threshold"] == 0 and pr.steps == steps
                assert same_frames(out, before) and same_stats(out.stats, before.stats)
            else:
                assert want["selected"] >= 1 and pr.steps == steps + 1
                done += 1
                sel = np.zeros((H, W), bool)
                sel[y:y + h, x:x + w] = want["mask"]
                assert (out.pxs[sel] == before.pxs[sel] + 1).all() and same_frames(out, before, ~sel)
            if name == "equal":
                assert want["k"] < w * h or w * h == 1
                assert want["selected"] == w * h
            if name == "k=1":
                assert want["selected"] == 1
            assert info["focus_done"] == done and pr.samples_done == 2


def test_selection_on_an_adaptive_session_uses_the_active_list(rt, gpu):
    """spheres-50, aTolerance 0.05, after step(20): the pixels that converged at n = 10 are
    finished and must never be selected, whatever their variance."""
    cam = camera(rt, SPHERES50, {"width": 48, "aspect": 1, "samples": 50, "depth": 4, "aTolerance": 0.05})
    with cam.progressive() as pr:
        Out(cam).step(pr, 20)
        blob = pr.save()
        width, height, _, j, i, st = blob_pixels(blob)
        active = np.zeros((height, width), bool)
        active[j, i] = (st["n"] >> np.uint32(31)) == 0
        n_on, n_off = int(active.sum()), int((~active).sum())
        print(f"spheres-50 48x48 after step(20): {n_on} pixels still sampling, {n_off} finished")
        assert n_on > 0 and n_off > 0 and pr.active_pixels == n_on
        var = pr.variance()
        assert bits_equal(var, variance_from_blob(blob)).all() and (var[~active] > 0).any()
        out = Out(cam).focus(pr, 5, permille=300)
        want = assert_selection(pr, out, var, active, None, {"permille": 300}, "spheres-50 adaptive, session variance")
        assert want["selected"] >= 1 and not (out.mask() & ~active).any()


# ---- 2. unselected pixels are untouched and still the one-shot frame ---------------------------------
@pytest.mark.parametrize("case", ["cornell-ref", "spheres200-ref", "cornell-fp32"])
def test_unselected_pixels_are_the_one_shot_frame(rt, oracle, gpu, case):
    cfg = SPHERES200 if case.startswith("spheres") else CORNELL
    ro = {"width": 48 if cfg is SPHERES200 else 40, "aspect": 1, "samples": 32, **FIXED}
    if case.endswith("fp32"):
        ro["precision"] = "fp32"
    cam = camera(rt, cfg, ro)
    with cam.progressive() as pr:
        out = Out(cam).step(pr, 4)
        out.focus(pr, 8, permille=250)
        assert cam.last_kernel() == ("chunked" if cfg is SPHERES200 else "pool")
        sel = out.mask()
        assert pr.samples_done == 4 and pr.focus_info["focus_done"] == 8 and pr.focus_info["first_sample"] == 32
        assert (out.pxs[sel] == 12).all() and (out.pxs[~sel] == 4).all()
        out.step(pr, 4)
        assert pr.samples_done == 8 and (out.pxs[sel] == 16).all()
    if case.endswith("fp32"):                                            # the session's own one-shot camera
        shot = camera(rt, cfg, {**ro, "samples": 8})
        ref = Out(shot)
        shot.render(ref.rgb, radiance=ref.rad)
        bad = int(((out.rgb != ref.rgb).any(-1) | (~bits_equal(out.rad, ref.rad)).any(-1))[~sel].sum())
        bad_px = 0
    else:
        orc = oracle.render(scene(rt, cfg), {**ro, "samples": 8}, threads=8)
        bad = int(((out.rgb != orc["rgb"]).any(-1) | (~bits_equal(out.rad, orc["radiance"])).any(-1))[~sel].sum())
        bad_px = int(((out.pxs != orc["px_samples"]) | (out.pxb != orc["px_bounces"]))[~sel].sum())
    print(f"{case}: {int(sel.sum())} of {sel.size} pixels selected; unselected pixels differing from samples: 8: "
          f"frame {bad}, counts {bad_px}")
    assert int((~sel).sum()) * 2 >= sel.size and sel.any()
    assert bad == 0 and bad_px == 0


# ---- 3. selected pixels hold the right samples --------------------------------------------------------
def test_selected_pixels_hold_the_window_past_the_cameras_samples(rt, gpu):
    base = {"width": 40, **FIXED}
    rng = np.random.default_rng(5)
    m = rng.random((40, 40), dtype=F) + F(0.01)
    cam_a, cam_b = camera(rt, CORNELL, {**base, "samples": 16}), camera(rt, CORNELL, {**base, "samples": 22})
    with cam_a.progressive() as pa:
        a4 = Out(cam_a).step(pa, 4).copy()
        a = Out(cam_a).focus(pa, 6, score=m)
        sel = a.mask()
        assert pa.focus_info["first_sample"] == 16 and pa.focus_info["focus_done"] == 6
    with cam_b.progressive() as pb:
        b16 = Out(cam_b).step(pb, 16).copy()
        b22 = Out(cam_b).step(pb, 6).copy()
        assert pb.samples_done == 22
    assert 0 < sel.sum() < sel.size
    # exact: the counts - any other sample index than 0..3 and 16..21 would change the bounce sum
    assert (a.pxs[sel] == 10).all() and (a.pxs[~sel] == 4).all()
    assert (a.pxb[sel] == a4.pxb[sel] + b22.pxb[sel] - b16.pxb[sel]).all()
    assert same_frames(a, a4, ~sel)
    # The radiance. A pixel's colour sum is a sequence of fp32 additions of non-negative samples c_i
    # in sample order, and its radiance the sum divided by n, rounded to fp32 once more. With u =
    # 2^-24 and T(S) the real sum over a sample set S, a stored mean of m samples times m is T(S)
    # within (m - 1 + 2) u T(S): m - 1 additions whose partial sums never exceed T(S), one rounding
    # of the quotient, and one more u for a quotient formed in another precision before it is
    # stored. So
    #     10 r_A     = T(A)     within 11 u T(A),   A = {0..3, 16..21}
    #      4 r_A(4)  = T(0..3)  within  5 u T(0..3)
    #     22 r_B(22) = T(0..21) within 23 u T(0..21)
    #     16 r_B(16) = T(0..15) within 17 u T(0..15)
    # and T(A) = T(0..3) + T(0..21) - T(0..15) exactly. Every set is a subset of {0..21} and the
    # samples are non-negative, so every T is at most T(0..21), itself at most 22 r_B(22) / (1 - 23 u):
    #     |10 r_A - (4 r_A(4) + 22 r_B(22) - 16 r_B(16))| <= (11 + 5 + 23 + 17) u T(0..21) = 56 u T(0..21).
    # 57 in place of 56 covers the second-order terms (below 56 u * 2^-18) and the fp64 evaluation
    # of the estimate; 2^-149 * 52 / 10 covers a mean that underflowed (each of the four stored
    # means then carries up to 2^-149, weighted 10 + 4 + 22 + 16).
    r_a, r_a4, r_b16, r_b22 = (v.rad.astype(np.float64) for v in (a, a4, b16, b22))
    assert np.isfinite(r_b22).all() and (r_b22 >= 0).all()
    est = (4.0 * r_a4 + 22.0 * r_b22 - 16.0 * r_b16) / 10.0
    bound = 57.0 * 2.0 ** -24 * (22.0 * r_b22) / 10.0 + 2.0 ** -149 * 5.2
    err = np.abs(r_a - est)
    worst = float((err[sel] / np.maximum(bound[sel], 1e-300)).max())
    print(f"selected pixels: {int(sel.sum())}; worst |r_A - estimate| / bound = {worst:.4f}")
    assert (err[sel] <= bound[sel]).all()


# ---- 4. independence of how steps are cut and of neighbours -------------------------------------------
def test_cut_and_neighbour_independence(rt, gpu):
    ro = {"width": 40, "samples": 32, **FIXED}
    rng = np.random.default_rng(9)
    m = rng.random((40, 40), dtype=F) + F(0.01)
    m2 = m.copy()
    m2[:, 20:] = rng.random((40, 20), dtype=F) * F(0.5)                 # another ranking on the right half
    runs = {}
    for name, cuts, score in (("8", [8], m), ("3+5", [3, 5], m), ("other", [8], m2)):
        cam = camera(rt, CORNELL, ro)
        with cam.progressive() as pr:
            out = Out(cam).step(pr, 4)
            masks = [out.focus(pr, n, score=score).mask().copy() for n in cuts]
            assert pr.focus_info["focus_done"] == 8 and pr.samples_done == 4
            runs[name] = (out.copy(), masks)
    (a, ma), (b, mb), (c, mc) = runs["8"], runs["3+5"], runs["other"]
    assert (ma[0] == mb[0]).all() and (mb[0] == mb[1]).all()
    assert same_frames(a, b) and same_stats(a.stats, b.stats)
    both = ma[0] & mc[0]
    print(f"selected under m {int(ma[0].sum())}, under m2 {int(mc[0].sum())}, under both {int(both.sum())}")
    assert both.any() and (ma[0] != mc[0]).any()
    assert same_frames(a, c, both) and same_frames(a, c, ~ma[0] & ~mc[0])


# ---- 5. mixing and finishing ----------------------------------------------------------------------------
def test_mixing_finishing_and_save(rt, gpu):
    ro = {"width": 40, "samples": 12, **FIXED}
    rng = np.random.default_rng(2)
    m = rng.random((40, 40), dtype=F) + F(0.01)
    cam = camera(rt, CORNELL, ro)
    with cam.progressive() as pr:
        out = Out(cam).step(pr, 4)
        blob = pr.save()                                                   # no focused step yet: saved
        m1 = out.focus(pr, 6, score=m).mask().copy()
        with pytest.raises(rt.RtError, match="progressive: a focused session cannot be saved") as e:
            pr.save()
        assert e.value.code == 1
        m2 = out.focus(pr, 6, score=m).mask().copy()                       # 4 + 6 + 6 > 12: stops at samples
        assert (m1 == m2).all() and (out.pxs[m1] == 12).all() and (out.pxs[~m1] == 4).all()
        assert pr.active_pixels == int((~m1).sum())
        m3 = out.focus(pr, 2, score=m).mask().copy()                       # the finished pixels are never visited again
        assert m3.any() and not (m3 & m1).any() and pr.focus_info["active"] == int((~m1).sum())
        assert (out.pxs[m1] == 12).all() and (out.pxs[m3] == 6).all()
        out.step(pr, 100)
        assert pr.samples_done == 12 and pr.done and pr.active_pixels == 0 and (out.pxs == 12).all()
        assert out.stats.samples["total"] == 12 * 1600
        out.focus(pr, 3, score=m)                                          # a finished session: nothing to select
        assert pr.focus_info["selected"] == 0 and pr.focus_info["active"] == 0 and not out.mask().any()
    # a session that took no focused step saves and restores as before
    cam2, cam3 = camera(rt, CORNELL, ro), camera(rt, CORNELL, ro)
    with cam2.resume(blob) as pr2, cam3.progressive() as pr3:
        assert pr2.samples_done == 4
        assert same_frames(Out(cam2).step(pr2, 4), Out(cam3).step(pr3, 8))


def test_adaptive_camera_retires_focused_pixels(rt, gpu):
    cam = camera(rt, SPHERES50, {"width": 48, "aspect": 1, "samples": 200, "depth": 4, "aTolerance": 0.05})
    with cam.progressive() as pr:
        out = Out(cam).step(pr, 20)
        active = [pr.active_pixels]
        for _ in range(3):
            out.focus(pr, 20, permille=1000)
            active.append(pr.active_pixels)
        print(f"spheres-50 adaptive: active pixels across focused steps {active}; px_samples up to {out.pxs.max()}")
        assert all(b <= a for a, b in zip(active, active[1:])) and active[-1] < active[0]
        assert out.pxs.max() == 80 and pr.samples_done == 20


def test_session_queries_after_a_focused_step(rt, gpu):
    """variance(), denoised(variance=True) and accumulated() use every pixel's own count: after a
    focused step they still equal their restatements fed the session's own outputs."""
    region = (5, 3, 29, 31)
    cam = camera(rt, CORNELL, {"width": 40, "samples": 32, "depth": 4, "aTolerance": 0, "seed": 1000})
    box = box_of(region, 40, 40)
    with rt.History() as history, cam.progressive(region) as pr:
        out = Out(cam).step(pr, 4)
        before = variance_from_blob(pr.save())
        out.focus(pr, 8, permille=250)
        sel = out.mask()
        var = pr.variance()
        assert bits_equal(var[~sel], before[~sel]).all() and (var[sel] != before[sel]).any()
        assert np.isfinite(var).all() and (var >= 0).all() and (out.pxs[sel] == 12).all()
        v_want = np.zeros((40, 40), F)
        want = cam.denoise(out.rad, region, variance=var, variance_out=v_want)
        v_got = np.zeros((40, 40), F)
        got = pr.denoised(variance=True, variance_out=v_got)
        assert bits_equal(got[box], want[box]).all() and bits_equal(v_got[box], v_want[box]).all()
        ref, _ = accumulate_ref(None, cam.view(), cam.render_guides(), out.rad, var, cam.reusable_objects(),
                                px_samples=out.pxs, region=region)
        lens = np.zeros((40, 40), F)
        acc = pr.accumulated(history, length_out=lens)
        assert bits_equal(acc[box], ref["radiance"][box]).all() and bits_equal(lens[box], ref["length"][box]).all()
        assert set(np.unique(lens[box]).tolist()) == {4.0, 12.0}
        got_h = history.read()
        assert bits_equal(got_h["variance"][box], ref["history"]["variance"][box]).all()


# ---- 6. a history as the score ---------------------------------------------------------------------------
def test_history_as_the_score(rt, gpu):
    region = (5, 3, 29, 31)
    ro = {"width": 40, "samples": 32, "depth": 4, "aTolerance": 0, "seed": 1000}
    cam, twin, other = camera(rt, CORNELL, ro), camera(rt, CORNELL, ro), camera(rt, CORNELL, ro)
    with rt.History() as history, cam.progressive(region) as pr, twin.progressive(region) as pt:
        Out(cam).step(pr, 4)
        Out(twin).step(pt, 4)
        pr.accumulated(history)
        a = Out(cam).focus(pr, 4, score=history, permille=200)
        plane = history.read()["variance"]
        b = Out(twin).focus(pt, 4, score=plane, permille=200)
        ia, ib = pr.focus_info, pt.focus_info
        print(f"history as the score: selected {ia['selected']}, from its read-back plane {ib['selected']}")
        assert a.mask().any() and (a.mask() == b.mask()).all() and same_frames(a, b)
        assert all(ia[k] == ib[k] for k in ("active", "eligible", "selected", "threshold", "focus_done", "first_sample"))
        assert_selection(pr, a, plane[box_of(region, 40, 40)], np.ones((31, 29), bool), region, {"permille": 200},
                         "history plane")
        # a history whose last committed region is not the session's
        with other.progressive() as po:
            po.step(4)
            with pytest.raises(rt.RtError, match="region and image size are not the session's") as e:
                po.focus(4, score=history)
            assert e.value.code == 1


# ---- 7. record passes ---------------------------------------------------------------------------------------
def test_focused_step_split_into_record_passes(rt, gpu, monkeypatch):
    ro = {"width": 96, "samples": 64, **FIXED}
    ones = np.ones((96, 96), F)
    outs = []
    for mb in ("1", None):
        cam = camera(rt, CORNELL, ro)
        with cam.progressive() as pr:
            out = Out(cam).step(pr, 4)
            if mb:
                monkeypatch.setenv("RT_AMD_SBUF_MB", mb)
            out.focus(pr, 20, score=ones, permille=1000)                  # 9216 pixels x 20 records of 16 bytes
            if mb:
                monkeypatch.delenv("RT_AMD_SBUF_MB")
            print(f"RT_AMD_SBUF_MB={mb}: {cam.pass_count()} record passes, {pr.focus_info['selected']} pixels")
            assert pr.focus_info["selected"] == 96 * 96 and (cam.pass_count() > 1) == bool(mb)
            outs.append(out.copy())
    assert same_frames(*outs) and same_stats(outs[0].stats, outs[1].stats) and (outs[0].pxs == 24).all()


# ---- 8. value: a condition, not a tolerance --------------------------------------------------------------------
def test_focused_samples_lower_the_summed_variance(rt, gpu):
    ro = {"width": 96, "samples": 64, **FIXED}
    cam_f, cam_u = camera(rt, CORNELL, ro), camera(rt, CORNELL, ro)
    with cam_f.progressive() as pf, cam_u.progressive() as pu:
        pf.step(8)
        for _ in range(4):
            st_f = pf.focus(8, permille=240)
        st_u = pu.step(16)
        v_f, v_u = float(pf.variance().astype(np.float64).sum()), float(pu.variance().astype(np.float64).sum())
    print(f"Cornell 96x96: focused {st_f.samples['total']:.0f} samples, summed variance {v_f:.6g}; "
          f"uniform {st_u.samples['total']:.0f} samples, summed variance {v_u:.6g}")
    assert st_f.samples["total"] <= st_u.samples["total"]
    assert v_f < v_u


# ---- the argument errors that need an open session (the others: tests/test_focus_abi.py) -------------------------
def test_session_errors(rt, gpu):
    ones = np.ones((40, 40), F)
    for mode in ("bounces", "samples"):
        cam = camera(rt, CORNELL, {"width": 40, "samples": 16, "depth": 4, "mode": mode})
        with cam.progressive() as pr:
            pr.step(4)
            with pytest.raises(rt.RtError, match="mode bounces / samples") as e:
                pr.focus(4, score=ones)
            assert e.value.code == 1
    cam = camera(rt, CORNELL, {"width": 40, "samples": 16, **FIXED})
    with cam.progressive() as pr, rt.History() as empty:
        pr.step(1)
        with pytest.raises(rt.RtError, match=r"samples_done < 2") as e:
            pr.focus(4)
        assert e.value.code == 1
        out = Out(cam).focus(pr, 4, score=ones, permille=1000)           # a map needs no variance
        assert out.mask().all() and (out.pxs == 5).all()
        with pytest.raises(rt.RtError, match="the history is empty") as e:
            pr.focus(4, score=empty)
        assert e.value.code == 1
        with pytest.raises(ValueError):
            pr.focus(4, score=np.ones((7, 7), F))
    # (samples + focus_done + n_samples > INT32_MAX is refused too, but a camera's sample loop is
    # capped at 10^9: the cursor would have to pass 1.1 * 10^9 first - some 17,000 focused steps of
    # 65535 samples - so no test reaches it)
