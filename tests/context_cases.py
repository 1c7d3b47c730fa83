"""Probes and histories of tests/test_context_reuse_gpu.py and tests/test_context_streams_gpu.py.

A *probe* is a call, or a short script of calls, with fixed arguments on one camera; it returns every
output it can capture as a flat dict. A *history* is a deterministic list of calls made on that
camera before the probe. The contract the tests pin: a probe's outputs do not depend on the history -
they are the outputs of the same probe on a fresh camera of the same scene and options, bit for bit.

Frame size and samples per pixel belong to the camera, so a history can differ from its probe only
in region, session step lengths, launch options and environment switches. Every probe camera
therefore has a 72x72 frame (81 tiles: at 37 spp a 1 MiB record budget cuts it into several passes),
the probes render the 29x22 region REGION (partial tiles on both edges, three tile rows; the mirror
scene's passes the 41x26 MREGION, which holds its specular objects) and the sessions run over the
24x24 SESSION; "bigger" is the full frame, "smaller" the 8x8 SMALL at one
session sample.
"""
import copy
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
from reproject_ref import moved_scene  # noqa: E402
from specular_reproject_ref import golden_scene, mirror_room  # noqa: E402
from test_gpu_parity import _mixed_scene  # noqa: E402

F = np.float32
W = H = 72
FULL = (0, 0, W, H)
REGION = (3, 5, 29, 22)
SESSION = (28, 42, 24, 24)
MREGION = (18, 39, 41, 26)  # the mirror scene's probes: both spheres and their images in the mirror
SMALL = (40, 48, 8, 8)
NOADAPT = {"aTolerance": 0}
MOVE = (0.25, 0.1, -0.1)
SPEC_GUIDES = {"max_bounces": 6, "max_fuzz": 0.3}    # follows the fuzz-0.2 metal
SPEC_GUIDES_0 = {"max_bounces": 6, "max_fuzz": 0.0}  # stops on it: the same key but for max_fuzz


def mirror_scene():
    """The specular tests' mirror room (a fuzz-0 mirror wall, a glass sphere) with its Lambert sphere
    turned into a fuzz-0.2 metal: a chain starts or ends on it depending on max_fuzz, and on the glass
    sphere depending on the through mask, so both cache keys change pixels."""
    sd = mirror_room()
    for m in sd["materials"]:
        if m["id"] == "sphere-white":
            m["material"] = {"type": "metal", "color": [0.8, 0.8, 0.8], "fuzz": 0.2}
    return sd


def _ro(**kw):
    return {"width": W, "aspect": 1, "depth": 6, **kw}


# name -> (scene builder(rt), render options)
CAMERAS = {
    "cornell37": (lambda rt: rt.generate_scene_data({"type": "cornell"}), _ro(samples=37, **NOADAPT)),
    "cornell9": (lambda rt: rt.generate_scene_data({"type": "cornell"}), _ro(samples=9, **NOADAPT)),
    "adaptive": (lambda rt: rt.generate_scene_data({"type": "cornell"}), _ro(samples=60)),
    "spheres": (lambda rt: rt.generate_scene_data({"type": "spheres", "options": {"count": 50, "seed": 42}}),
                _ro(samples=9, **NOADAPT)),
    "mixed": (lambda rt: _mixed_scene(), _ro(samples=9, **NOADAPT)),
    "mirror": (lambda rt: mirror_scene(), _ro(samples=37)),
}
_scenes = {}


def scene_of(rt, name):
    if name not in _scenes:
        _scenes[name] = CAMERAS[name][0](rt)
    return copy.deepcopy(_scenes[name])


def camera(rt, name, **ro):
    return rt.create_camera_from_scene_data(scene_of(rt, name), {**CAMERAS[name][1], **ro})


def moved_camera(rt, name):
    """The second camera of the reprojection probes: the same scene from a moved `from`."""
    return rt.create_camera_from_scene_data(moved_scene(scene_of(rt, name), MOVE), {**CAMERAS[name][1], "seed": 1001})


def seeded(seed, *shape, scale=4.0):
    return (np.random.default_rng(seed).random(shape, dtype=F) * F(scale)).astype(F)


def stats_tuple(st):
    return (st.pixels, st.samples["total"], st.samples["min"], st.samples["max"], st.bounces["total"],
            st.bounces["min"], st.bounces["max"])


def same(a, b):
    """Bit for bit: arrays by dtype, shape and value (NaN equal to NaN), bytes, scalars and tuples by ==."""
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        if not (isinstance(a, np.ndarray) and isinstance(b, np.ndarray)) or a.dtype != b.dtype or a.shape != b.shape:
            return False
        if a.dtype.kind == "f":
            return bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)) or
                        ((a == b) | (np.isnan(a) & np.isnan(b))).all())
        return bool(np.array_equal(a, b))
    return type(a) is type(b) and a == b


def differing(got, want):
    """The keys of two probe results that differ (missing keys included)."""
    return sorted(k for k in set(got) | set(want) if k not in got or k not in want or not same(got[k], want[k]))


def queries(cam, ran=True):
    """What every probe captures after its last call."""
    path_ms, _ = cam.kernel_times()
    out = {"q.last_kernel": cam.last_kernel(), "q.pass_count": cam.pass_count(), "q.used": cam.primary_info()["used"]}
    if ran:
        out["q.path_ms_positive"] = path_ms > 0
    return out


def frames():
    return np.zeros((H, W, 3), np.uint8), np.zeros((H, W, 3), F)


# ---- probes: fn(rt, cam) -> dict -------------------------------------------------------------------
def probe_region(rt, cam):
    rgb, rad = frames()
    st = cam.render_region(rgb, REGION, radiance=rad)
    return {"rgb": rgb, "rad": rad, "stats": stats_tuple(st), **queries(cam)}


def probe_adaptive(rt, cam):
    out = probe_region(rt, cam)
    out["adaptive_info"] = cam.adaptive_info()
    return out


def probe_device_fp32(rt, cam):
    import torch
    rgb = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    rad = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    st, _ = cam.render_device(rgb_ptr=rgb.data_ptr(), radiance_ptr=rad.data_ptr(), region=REGION, precision="fp32",
                              synchronize=True)
    return {"rgb": rgb.cpu().numpy(), "rad": rad.cpu().numpy(), "stats": stats_tuple(st), **queries(cam)}


PACKED_TILES = 12  # REGION's 4 x 3 tiles; group 1 of 3 writes 4 of them


def probe_packed(rt, cam):
    import torch
    n = PACKED_TILES * 64
    rgb = torch.zeros((n, 3), dtype=torch.uint8, device="cuda")
    rad = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    pxs = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    pxb = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    st, _ = cam.render_device(rgb_ptr=rgb.data_ptr(), radiance_ptr=rad.data_ptr(), px_samples_ptr=pxs.data_ptr(),
                              px_bounces_ptr=pxb.data_ptr(), region=REGION, tile_group=1, tile_groups=3, packed=True,
                              synchronize=True)
    return {"rgb": rgb.cpu().numpy(), "rad": rad.cpu().numpy(), "pxs": pxs.cpu().numpy(), "pxb": pxb.cpu().numpy(),
            "stats": stats_tuple(st), **queries(cam)}


def probe_guides(rt, cam):
    out = {}
    for tag, kw in (("first", {}), ("chain", {"through_specular": True, "max_bounces": 8, "max_fuzz": 0.0})):
        for k, v in cam.render_guides(MREGION, **kw).items():
            out[f"{tag}.{k}"] = v
    return out


def probe_denoise(rt, cam):
    rad, var = seeded(11, H, W, 3), seeded(12, H, W, scale=0.5)
    rgb, rgb_v = np.zeros((H, W, 3), np.uint8), np.zeros((H, W, 3), np.uint8)
    vout = np.zeros((H, W), F)
    out = {"plain": cam.denoise(rad, REGION, levels=4, rgb=rgb), "plain.rgb": rgb}
    out["guided"] = cam.denoise(rad, REGION, levels=3, variance=var, variance_out=vout, rgb=rgb_v)
    out["guided.rgb"], out["guided.var"] = rgb_v, vout
    return out


def _reproject_outs():
    return {"rgb": np.zeros((H, W, 3), np.uint8), "history_out": np.zeros((H, W, 3), F), "weight_out": np.zeros((H, W), F)}


def probe_reproject(rt, cam):
    prev = moved_camera(rt, "mirror")
    prad, fresh = seeded(21, H, W, 3), seeded(22, H, W, 3)
    out = {}
    for tag, kw in (("plain", {}), ("spec", {"guides": "specular", "through": 5, "kind": np.zeros((H, W), np.uint8)})):
        o = _reproject_outs()
        out[f"{tag}.blend"] = cam.reproject(prev, prad, region=MREGION, radiance=fresh, samples=4, **o, **kw)
        for k, v in {**o, **({"kind": kw["kind"]} if "kind" in kw else {})}.items():
            out[f"{tag}.{k}"] = v
    return out


def probe_session(rt, cam):
    prev = moved_camera(rt, "mirror")
    prad = seeded(31, H, W, 3)
    out = {}

    def step(tag, call):
        rgb, rad = frames()
        pxs, pxb = np.zeros((H, W), np.int32), np.zeros((H, W), np.int32)
        st = call(rgb, rad, pxs, pxb)
        out.update({f"{tag}.rgb": rgb, f"{tag}.rad": rad, f"{tag}.pxs": pxs, f"{tag}.pxb": pxb,
                    f"{tag}.stats": stats_tuple(st)})

    with cam.progressive(SESSION) as pr, rt.History() as hist:
        step("step4", lambda *b: pr.step(4, *b))
        step("step5", lambda *b: pr.step(5, *b))
        out.update({f"step5.{k}": v for k, v in queries(cam).items()})
        for tag, kw in (("dn_first", {}), ("dn_spec", {"guides": SPEC_GUIDES}), ("dn_spec0", {"guides": SPEC_GUIDES_0}),
                        ("dn_var", {"variance": True, "variance_out": np.zeros((H, W), F)})):
            rgb = np.zeros((H, W, 3), np.uint8)
            out[tag] = pr.denoised(rgb, **kw)
            out[f"{tag}.rgb"] = rgb
            if "variance_out" in kw:
                out[f"{tag}.var"] = kw["variance_out"]
        out["variance"] = pr.variance()
        out["blob"] = pr.save()
        for tag, kw in (("rp", {}), ("rp_spec", {"guides": "specular", "through": 5, "kind": np.zeros((H, W), np.uint8)})):
            rgb, wgt = np.zeros((H, W, 3), np.uint8), np.zeros((H, W), F)
            out[tag] = pr.reprojected(prev, prad, rgb=rgb, weight_out=wgt, **kw)
            out[f"{tag}.rgb"], out[f"{tag}.weight"] = rgb, wgt
            if "kind" in kw:
                out[f"{tag}.kind"] = kw["kind"]
        acc = {k: np.zeros((H, W), F) for k in ("variance_out", "length_out", "weight_out")}
        rgb = np.zeros((H, W, 3), np.uint8)
        out["acc"] = pr.accumulated(hist, rgb, **acc)
        out.update({"acc.rgb": rgb, **{f"acc.{k}": v for k, v in acc.items()}})
        sel = np.zeros((H, W), np.uint8)
        step("focus3", lambda *b: pr.focus(3, *b, sel))
        out["focus3.selected"] = sel
        out["focus3.info"] = tuple(sorted((k, v) for k, v in pr.focus_info.items() if k != "select_ms"))
        out["info"] = tuple(sorted((k, v) for k, v in pr.info.items()))
    out.update(queries(cam))
    return out


# name -> (camera, probe, oracle check: compare render outputs with oracle.render over REGION)
PROBES = {
    "region_ref": ("cornell37", probe_region, "ref"),
    "device_fp32": ("cornell9", probe_device_fp32, "fp32"),
    "adaptive": ("adaptive", probe_adaptive, "ref"),
    "spheres": ("spheres", probe_region, "ref"),
    "mixed": ("mixed", probe_region, "ref"),
    "packed": ("cornell9", probe_packed, None),
    "guides": ("mirror", probe_guides, None),
    "denoise": ("cornell9", probe_denoise, None),
    "reproject": ("mirror", probe_reproject, None),
    "session": ("mirror", probe_session, None),
}
# the kernel each render probe runs on a fresh camera (the histories must not change it)
PROBE_KERNEL = {"region_ref": "pool", "device_fp32": "pool", "adaptive": "pool", "spheres": "chunked",
                "mixed": "chunked", "packed": "pool"}


# ---- histories: fn(rt, cam, env) ----------------------------------------------------------------------
# env is pytest's monkeypatch; every history leaves the environment as it found it.
def _render(cam, region):
    rgb, rad = frames()
    cam.render_region(rgb, region, radiance=rad)
    return rad


def _device(cam, region, **kw):
    import torch
    px = max(W * H, PACKED_TILES * 64 * 8)
    rgb = torch.zeros((px, 3), dtype=torch.uint8, device="cuda")
    pxs = torch.zeros((px,), dtype=torch.int32, device="cuda")
    return cam.render_device(rgb_ptr=rgb.data_ptr(), px_samples_ptr=pxs.data_ptr(), region=region, synchronize=True, **kw)


def _passes(rt, cam, region, levels, steps, prev=None):
    """One call of every pass family over `region`; a session over it, closed."""
    prev = prev or cam
    rad = _render(cam, region)
    cam.render_guides(region)
    cam.render_guides(region, through_specular=True, max_bounces=3, max_fuzz=0.7)
    cam.denoise(rad, region, levels=levels)
    cam.denoise(rad, region, levels=levels, variance=seeded(5, H, W), variance_out=np.zeros((H, W), F))
    cam.reproject(prev, rad, region=region, radiance=rad, samples=2)
    cam.reproject(prev, rad, region=region, guides="specular", through=15)
    with cam.progressive(region) as pr, rt.History() as hist:
        for n in steps:
            pr.step(n)
        if pr.samples_done >= 2:
            pr.denoised(levels=levels)
            pr.denoised(levels=levels, guides={"max_bounces": 2, "max_fuzz": 0.9})
            pr.denoised(levels=levels, variance=True)
            pr.variance()
            pr.reprojected(prev, rad, guides="specular", through=15)
            pr.accumulated(hist, filter_levels=1)
            pr.focus(2)


def history_none(rt, cam, env):
    pass


def history_bigger(rt, cam, env):
    env.setenv("RT_AMD_SBUF_MB", "1")
    _passes(rt, cam, FULL, 5, (cam.info["samples_loop"],))
    _device(cam, FULL, precision="fp32")
    env.delenv("RT_AMD_SBUF_MB")


def history_smaller(rt, cam, env):
    _passes(rt, cam, SMALL, 1, (1,))
    _device(cam, SMALL)


def history_kernels(rt, cam, env):
    for switches in ({}, {"RT_AMD_POOL_KERNEL": "0"}, {"RT_AMD_CHUNKED": "0"}, {"RT_AMD_ADAPT_ROUNDS": "0"}):
        for k, v in switches.items():
            env.setenv(k, v)
        _render(cam, FULL)
        for k in switches:
            env.delenv(k)
    _device(cam, REGION, precision="fp32")
    for trav in ("reference", "fast", "brute"):
        _device(cam, FULL, traversal=trav)
    _device(cam, REGION, count_work=True)
    _device(cam, FULL, packed=True, tile_group=2, tile_groups=3)
    # a camera below the table's sample threshold never builds it by rendering: the device query
    # builds it the way a launch does, so a later low-spp probe runs with the table
    cam.primary_table(device=True)
    _render(cam, SMALL)


def history_options(rt, cam, env):
    rad = seeded(41, H, W, 3)
    cam.render_guides(FULL, through_specular=True, max_bounces=2, max_fuzz=0.0)
    cam.render_guides(REGION, through_specular=True, max_bounces=8, max_fuzz=0.9)
    cam.reproject(cam, rad, region=REGION, guides={"max_bounces": 8, "max_fuzz": 0.9}, through=5)
    for levels in (1, 8):
        cam.denoise(rad, FULL, levels=levels)
    with cam.progressive((0, 0, 33, 17)) as pr:
        pr.step(3)
        pr.denoised(guides={"max_bounces": 6, "max_fuzz": 0.0})
        pr.denoised(guides={"max_bounces": 6, "max_fuzz": 0.9})
        blob = pr.save()
    with cam.resume(blob) as pr:
        pr.step(2)
        pr.reprojected(cam, rad, guides={"max_bounces": 6, "max_fuzz": 0.9}, through=5)
    # last, the probes' own guide options: the through table they find differs from theirs (mask 5)
    # in the mask alone
    for through in (15, 5, 15):
        cam.reproject(cam, rad, region=MREGION, guides="specular", through=through)
    pr = cam.progressive((16, 0, 40, 50))  # still open when the probe starts
    pr.step(2)
    pr.denoised(guides={"max_bounces": 6, "max_fuzz": 0.9})


def history_refusals(rt, cam, env):
    import pytest
    rad = seeded(51, H, W, 3)
    _render(cam, SMALL)
    with pytest.raises(rt.RtError, match="empty"):
        cam.progressive((W + 5, 0, 4, 4))
    with pytest.raises(rt.RtError, match="empty"):
        cam.denoise(rad, (0, H + 1, 4, 4))
    with pytest.raises(rt.RtError, match="levels must be"):
        cam.denoise(rad, REGION, levels=9)
    with pytest.raises(rt.RtError, match="no progressive session is open"):
        rt.ProgressiveRender(cam).step(1)
    other = rt.create_camera_from_scene_data(golden_scene("default"), {"width": W, "aspect": 1, "samples": 4})
    with pytest.raises(rt.RtError, match="different scenes"):
        cam.reproject(other, rad, region=REGION)
    first = cam.progressive(SMALL)
    with cam.progressive(FULL) as pr:  # (drops the first session)
        pr.step(2)
        with pytest.raises(rt.RtError, match="different scenes"):
            pr.reprojected(other, rad)
        pr.focus(2)
        with pytest.raises(rt.RtError, match="focused session cannot be saved"):
            pr.save()
    with pytest.raises(rt.RtError, match="no progressive session is open"):
        first.step(1)
    with pytest.raises(rt.RtError):
        cam.resume(b"not a checkpoint")


def history_release(rt, cam, env):
    history_smaller(rt, cam, env)
    pr = cam.progressive(FULL)
    pr.step(2)
    cam.primary_table(device=True)
    cam.release_device()  # with the session open
    _render(cam, SMALL)
    history_options(rt, cam, env)
    cam.release_device()


HISTORIES = {"none": history_none, "bigger": history_bigger, "smaller": history_smaller, "kernels": history_kernels,
             "options": history_options, "refusals": history_refusals, "release": history_release}
