"""Progressive rendering on the GPU (rt_camera_progressive_*): every comparison is exact -
u8, fp32 radiance (NaN equal to NaN), px_samples, px_bounces and RenderStats total / min /
max / pixels - against the CPU oracle at `samples: s` and against one-shot GPU renders."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CORNELL_FIXED = {"width": 40, "samples": 24, "depth": 8, "aTolerance": 0}
SPHERES_CFG = {"type": "spheres", "options": {"count": 500, "seed": 42}}
SPHERES_RO = {"width": 48, "aspect": 1, "samples": 50, "depth": 8, "aTolerance": 0.1}
SPHERES_STEPS = [7, 13, 13, 17]
CORNELL_ADAPT = {"width": 40, "samples": 60, "depth": 8}
DEFAULT_RO = {"width": 40, "samples": 30, "depth": 10, "aTolerance": 0.1}
SENTINEL = {"rgb": 0xA5, "rad": -123.25, "pxs": -7, "pxb": -9}


# ---- helpers ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scene(rt, cfg_key):
    import json
    return rt.generate_scene_data(json.loads(cfg_key))


def scene(rt, cfg):
    import json
    return _scene(rt, json.dumps(cfg, sort_keys=True))


_ORACLE = {}


def oracle_at(rt, oracle, cfg, ro, s, region=None):
    """The oracle's render of the camera with `samples: s` (computed once, never modified)."""
    import json
    key = (json.dumps(cfg, sort_keys=True), json.dumps(ro, sort_keys=True), s, region)
    if key not in _ORACLE:
        o = oracle.render(scene(rt, cfg), {**ro, "samples": s}, region=region, threads=8)
        for a in ("radiance", "rgb", "px_samples", "px_bounces"):
            o[a].setflags(write=False)
        _ORACLE[key] = o
    return _ORACLE[key]


class Frame:
    """Caller-owned full-frame buffers, pre-filled with sentinels."""

    def __init__(self, cam):
        H, W = cam.image_height, cam.image_width
        self.rgb = np.full((H, W, 3), SENTINEL["rgb"], np.uint8)
        self.rad = np.full((H, W, 3), SENTINEL["rad"], np.float32)
        self.pxs = np.full((H, W), SENTINEL["pxs"], np.int32)
        self.pxb = np.full((H, W), SENTINEL["pxb"], np.int32)
        self.stats = None

    def step(self, pr, n):
        self.stats = pr.step(n, self.rgb, radiance=self.rad, px_samples=self.pxs, px_bounces=self.pxb)
        return self

    def copy(self):
        import copy
        return copy.deepcopy(self)


def _box(region, H, W):
    x, y, w, h = region or (0, 0, W, H)
    return slice(y, y + h), slice(x, x + w)


def _rad_equal(a, b):
    return (a == b) | (np.isnan(a) & np.isnan(b))


def assert_stats(st, ref, what):
    """RenderStats (ours) against an oracle stats dict or another RenderStats."""
    if not isinstance(ref, dict):
        ref = {"pixels": ref.pixels, "samples": ref.samples, "bounces": ref.bounces}
    print(f"{what}: stats pixels {st.pixels} samples {st.samples} bounces {st.bounces}")
    assert st.pixels == ref["pixels"], what
    for k in ("total", "min", "max"):
        assert st.samples[k] == ref["samples"][k], (what, "samples", k)
        assert st.bounces[k] == ref["bounces"][k], (what, "bounces", k)


def assert_frame_is_oracle(f, orc, region, what):
    H, W = f.pxs.shape
    ys, xs = _box(region, H, W)
    n_rgb = int((f.rgb[ys, xs] != orc["rgb"][ys, xs]).any(axis=-1).sum())
    n_rad = int((~_rad_equal(f.rad[ys, xs], orc["radiance"][ys, xs])).any(axis=-1).sum())
    n_pxs = int((f.pxs[ys, xs] != orc["px_samples"][ys, xs]).sum())
    n_pxb = int((f.pxb[ys, xs] != orc["px_bounces"][ys, xs]).sum())
    print(f"{what}: pixels differing from the oracle: rgb {n_rgb}, radiance {n_rad}, px_samples {n_pxs}, "
          f"px_bounces {n_pxb}")
    assert (n_rgb, n_rad, n_pxs, n_pxb) == (0, 0, 0, 0), what
    assert_stats(f.stats, orc["stats"], what)


def assert_outside_untouched(f, region):
    H, W = f.pxs.shape
    ys, xs = _box(region, H, W)
    mask = np.ones((H, W), bool)
    mask[ys, xs] = False
    assert (f.rgb[mask] == SENTINEL["rgb"]).all() and (f.rad[mask] == np.float32(SENTINEL["rad"])).all()
    assert (f.pxs[mask] == SENTINEL["pxs"]).all() and (f.pxb[mask] == SENTINEL["pxb"]).all()


def assert_frames_equal(a, b, what, px=True):
    assert (a.rgb == b.rgb).all() and _rad_equal(a.rad, b.rad).all(), what
    if px:
        assert (a.pxs == b.pxs).all() and (a.pxb == b.pxb).all(), what
    assert_stats(a.stats, b.stats, what)


def one_shot(rt, sd, ro, region=None):
    cam = rt.create_camera_from_scene_data(sd, ro)
    f = Frame(cam)
    f.stats = cam.render_region(f.rgb, region or (0, 0, cam.image_width, cam.image_height), radiance=f.rad)
    return cam, f


def run_steps(rt, oracle, cfg, ro, steps, region=None, check_oracle=True, kernel=None, active=None):
    """A session cut into `steps`; every frame with s >= 2 against the oracle at samples: s."""
    sd = scene(rt, cfg)
    cam = rt.create_camera_from_scene_data(sd, ro)
    f, frames, s = Frame(cam), [], 0
    with cam.progressive(region) as pr:
        assert pr.samples == ro["samples"] and pr.samples_done == 0 and pr.steps == 0 and not pr.done
        for k, n in enumerate(steps):
            f.step(pr, n)
            s += n
            assert pr.samples_done == s and pr.steps == k + 1
            if kernel:
                assert cam.last_kernel() == kernel
            assert_outside_untouched(f, region)
            if check_oracle and s >= 2:
                orc = oracle_at(rt, oracle, cfg, ro, s, region)
                assert_frame_is_oracle(f, orc, region, f"{cfg['type']} s={s}")
                if active is not None:
                    ys, xs = _box(region, *f.pxs.shape)
                    want = 0 if s == ro["samples"] else int((orc["px_samples"][ys, xs] == s).sum())
                    print(f"  active pixels after s={s}: {pr.active_pixels} (oracle pixels with px_samples == s: {want})")
                    assert pr.active_pixels == want == active[k]
            frames.append(f.copy())
        assert pr.done and pr.active_pixels == 0
    return cam, frames


# ---- 1, 2: fixed spp on the pool kernel --------------------------------------------------------
@pytest.mark.parametrize("precision", ["ref", "fp32"])
def test_fixed_spp_region_steps(rt, oracle, gpu, precision):
    region = (3, 5, 21, 18)  # cuts 8x8 tiles on every side
    ro = {**CORNELL_FIXED, "precision": precision}
    # (the oracle comparison is for ref precision; fp32 is pinned to its own one-shot render)
    cam, frames = run_steps(rt, oracle, {"type": "cornell"}, ro if precision == "fp32" else CORNELL_FIXED,
                            [2, 5, 1, 16], region, check_oracle=precision == "ref", kernel="pool")
    assert cam.precision == precision
    _, shot = one_shot(rt, scene(rt, {"type": "cornell"}), ro, region)
    assert_frames_equal(frames[-1], shot, f"final frame == one-shot ({precision})", px=False)


def test_step_size_independence_and_clamp(rt, oracle, gpu):
    finals = []
    for steps in ([24], [1] * 24, [7, 17]):
        _, frames = run_steps(rt, oracle, {"type": "cornell"}, CORNELL_FIXED, steps, check_oracle=False)
        finals.append(frames[-1])
    assert_frames_equal(finals[0], finals[1], "[24] == [1]*24")
    assert_frames_equal(finals[0], finals[2], "[24] == [7, 17]")
    assert_frame_is_oracle(finals[0], oracle_at(rt, oracle, {"type": "cornell"}, CORNELL_FIXED, 24), None, "s=24")
    cam = rt.create_camera_from_scene_data(scene(rt, {"type": "cornell"}), CORNELL_FIXED)
    with cam.progressive() as pr:
        f = Frame(cam).step(pr, 1000)
        assert pr.samples_done == 24 and pr.done and pr.steps == 1
        assert_frames_equal(f, finals[0], "a step of 1000 clamps to 24")
        g = Frame(cam).step(pr, 5)  # a finished session renders nothing
        assert pr.samples_done == 24 and pr.active_pixels == 0 and pr.steps == 1
        assert_frames_equal(g, finals[0], "a further step returns the same frame")
        with pytest.raises(rt.RtError, match="n_samples must be positive") as e:
            pr.step(0)
        assert e.value.code == 1  # RT_ERR_INVALID


# ---- 3, 4: adaptive cameras ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def spheres_session(rt, oracle, gpu):
    """The uninterrupted spheres-500 session: its frames at s = 7, 20, 33, 50 and the
    checkpoint saved at s = 20 (shared by the adaptive and the checkpoint tests)."""
    sd = scene(rt, SPHERES_CFG)
    cam = rt.create_camera_from_scene_data(sd, SPHERES_RO)
    f, frames, active, blob = Frame(cam), [], [], None
    with cam.progressive() as pr:
        for n in SPHERES_STEPS:
            frames.append(f.step(pr, n).copy())
            active.append(pr.active_pixels)
            kernel = cam.last_kernel()
            if pr.samples_done == 20:
                blob = pr.save()
        info = pr.info
    return {"frames": frames, "active": active, "blob": blob, "kernel": kernel, "info": info}


def test_adaptive_bvh_steps_match_oracle(rt, oracle, gpu, spheres_session):
    assert spheres_session["kernel"] == "chunked"
    s = 0
    for k, n in enumerate(SPHERES_STEPS):
        s += n
        orc = oracle_at(rt, oracle, SPHERES_CFG, SPHERES_RO, s)
        assert_frame_is_oracle(spheres_session["frames"][k], orc, None, f"spheres-500 s={s}")
        want = 0 if s == 50 else int((orc["px_samples"] == s).sum())
        print(f"  active after s={s}: {spheres_session['active'][k]}, oracle px_samples == s: {want}")
        assert spheres_session["active"][k] == want == [2304, 975, 881, 0][k]
    # pixels retire at several steps, and 841 run to the cap
    full = oracle_at(rt, oracle, SPHERES_CFG, SPHERES_RO, 50)["px_samples"]
    assert int((full == 50).sum()) == 841 and spheres_session["info"]["done"]


def test_adaptive_pool_and_default_scene(rt, oracle, gpu):
    # Cornell: 175 of 1600 pixels retire at n = 10, 1425 run to the cap
    run_steps(rt, oracle, {"type": "cornell"}, CORNELL_ADAPT, [20, 13, 27], kernel="pool", active=[1425, 1425, 0])
    full = oracle_at(rt, oracle, {"type": "cornell"}, CORNELL_ADAPT, 60)["px_samples"]
    assert int((full == 10).sum()) == 175 and int((full == 60).sum()) == 1425
    # default scene: 543 of 920 still sampling at s = 20, 513 reach the cap
    run_steps(rt, oracle, {"type": "default"}, DEFAULT_RO, [7, 13, 10], active=[920, 543, 0])
    full = oracle_at(rt, oracle, {"type": "default"}, DEFAULT_RO, 30)["px_samples"]
    assert int((full == 30).sum()) == 513


# ---- 5: visualisation modes ------------------------------------------------------------------------
def test_mode_bounces_every_step(rt, oracle, gpu):
    run_steps(rt, oracle, {"type": "cornell"}, {"width": 40, "samples": 50, "depth": 8, "mode": "bounces"},
              [9, 21, 20], kernel="pool")


def test_mode_samples_preview_and_final(rt, oracle, gpu):
    cfg, ro = {"type": "cornell"}, {"width": 40, "samples": 50, "depth": 8, "mode": "samples"}
    cam, frames = run_steps(rt, oracle, cfg, ro, [9, 21, 20], check_oracle=False)
    assert_frame_is_oracle(frames[-1], oracle_at(rt, oracle, cfg, ro, 50), None, "mode samples, final")
    for f, s in zip(frames[:-1], (9, 30)):
        # finalColor divides by the camera's own `samples` (src/camera.ts:333): a JS double, stored as fp32
        red = np.minimum(f.pxs.astype(np.float64) / 50.0, 1.0).astype(np.float32)
        assert (f.rad[..., 0] == red).all() and (f.rad[..., 1:] == 0).all()
        assert f.pxs.max() == s and (f.pxs == oracle_at(rt, oracle, cfg, ro, s)["px_samples"]).all()


# ---- 6: several record passes inside a step ----------------------------------------------------------
def test_steps_split_into_record_passes(rt, oracle, gpu, monkeypatch):
    sd = scene(rt, {"type": "cornell"})
    ro = {"width": 96, "samples": 37, "depth": 16, "aTolerance": 0}
    monkeypatch.setenv("RT_AMD_SBUF_MB", "1")
    cam = rt.create_camera_from_scene_data(sd, ro)
    f = Frame(cam)
    with cam.progressive() as pr:
        for n in (20, 17):
            f.step(pr, n)
            print(f"  step of {n}: {cam.pass_count()} record passes")
            assert cam.pass_count() > 1
    monkeypatch.delenv("RT_AMD_SBUF_MB")
    cam2, shot = one_shot(rt, sd, ro)
    assert cam2.pass_count() == 1
    assert_frames_equal(f, shot, "multi-pass steps == one-shot", px=False)


# ---- 7: fp32 (case 1 is parametrised above) ------------------------------------------------------------
def test_fp32_adaptive_bvh_final_equals_one_shot(rt, oracle, gpu):
    ro = {**SPHERES_RO, "precision": "fp32"}
    cam, frames = run_steps(rt, oracle, SPHERES_CFG, ro, SPHERES_STEPS, check_oracle=False, kernel="chunked")
    _, shot = one_shot(rt, scene(rt, SPHERES_CFG), ro)
    assert_frames_equal(frames[-1], shot, "fp32 spheres-500 final == one-shot", px=False)
    assert shot.stats.samples["min"] < 50  # adaptive: some pixels converged early


# ---- 8: checkpoint ----------------------------------------------------------------------------------------
def test_checkpoint_resume_reproduces_the_session(rt, oracle, gpu, spheres_session):
    blob = spheres_session["blob"]
    info = rt.progressive_blob_info(blob)
    assert info["samples_done"] == 20 and info["region"] == (0, 0, 48, 48) and info["active_pixels"] == 975
    assert info["samples"] == 50 and info["steps"] == 2 and info["build_id"] == rt.build_id()
    assert len(blob) == 144 + info["state_bytes"] and info["state_bytes"] == 2304 * 48
    # (the session and its camera are gone: the fixture closed one and dropped the other)
    sd = scene(rt, SPHERES_CFG)
    cam = rt.create_camera_from_scene_data(sd, SPHERES_RO)
    f = Frame(cam)
    with cam.resume(blob) as pr:
        assert pr.samples_done == 20 and pr.active_pixels == 975 and pr.steps == 2
        for k, n in ((2, 13), (3, 17)):
            f.step(pr, n)
            assert_frames_equal(f, spheres_session["frames"][k], f"resumed frame at s={pr.samples_done}")
        assert pr.done and pr.steps == 4

    def refused(ro, b, word):
        c = rt.create_camera_from_scene_data(sd, ro)
        with pytest.raises(rt.RtError, match=word) as e:
            c.resume(b)
        assert e.value.code == 1  # RT_ERR_INVALID
        print(f"  refused: {e.value}")

    refused({**SPHERES_RO, "seed": 7}, blob, "seed")
    refused({**SPHERES_RO, "width": 40}, blob, "dimensions")
    refused({**SPHERES_RO, "precision": "fp32"}, blob, "precision")
    refused({**SPHERES_RO, "depth": 9}, blob, "fingerprint")
    flipped = bytearray(blob)
    flipped[144 + 48 * 1000 + 5] ^= 0x10
    refused(SPHERES_RO, bytes(flipped), "corrupt payload")
    refused(SPHERES_RO, blob[:-1], "truncated")


# ---- 9: isolation from one-shot renders ---------------------------------------------------------------------
def test_one_shot_renders_between_steps_do_not_disturb(rt, oracle, gpu):
    cfg, ro = {"type": "cornell"}, CORNELL_ADAPT
    sd = scene(rt, cfg)
    cam = rt.create_camera_from_scene_data(sd, ro)
    f = Frame(cam)
    with cam.progressive() as pr:
        f.step(pr, 20)
        assert_frame_is_oracle(f, oracle_at(rt, oracle, cfg, ro, 20), None, "before the one-shot, s=20")
        shot = Frame(cam)
        shot.stats = cam.render_region(shot.rgb, (0, 0, 40, 40), radiance=shot.rad)  # adaptive rounds
        orc = oracle_at(rt, oracle, cfg, ro, 60)
        assert (shot.rgb == orc["rgb"]).all() and _rad_equal(shot.rad, orc["radiance"]).all()
        assert_stats(shot.stats, orc["stats"], "one-shot between two steps")
        for n, s in ((13, 33), (27, 60)):
            f.step(pr, n)
            assert_frame_is_oracle(f, oracle_at(rt, oracle, cfg, ro, s), None, f"after the one-shot, s={s}")
    pr = cam.progressive()
    pr.step(5)
    cam.release_device()  # ends the session
    with pytest.raises(rt.RtError, match="no progressive session is open"):
        pr.step(5)
    # and the camera still renders
    with cam.progressive() as pr2:
        g = Frame(cam).step(pr2, 60)
    assert_frames_equal(g, f, "a new session after release_device")
