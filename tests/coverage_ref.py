"""The normative definition of the sub-pixel coverage word (rt_camera_render_coverage) and of the
filters' edge hold, restated in NumPy. The rays are fp32 vector arithmetic with one result per
operation, traced by the oracle's world_hit, so the device words equal these in every bit; the hold
is a select. A helper module of the coverage tests, not a test file."""
import numpy as np

F = np.float32


def sub_offsets(k):
    """[(bit, ox, oy)] of the k x k sub-rays: bit = b k + a, ox = (a + 0.5) / k - 0.5, oy likewise
    from b - +-0.25, or +-0.125 and +-0.375: exact in fp32."""
    assert k in (2, 4)
    return [(b * k + a, F((a + 0.5) / k - 0.5), F((b + 0.5) / k - 0.5)) for b in range(k) for a in range(k)]


def _objects(oracle, scene, cen, through):
    """The first-hit object of the pinhole rays from `cen` through the points `through` (H, W, 3):
    int32 (H, W), -1 on a miss."""
    d = (through - cen).astype(F)
    o = np.broadcast_to(cen, d.shape)
    wh = oracle.world_hit(scene, o.reshape(-1, 3), d.reshape(-1, 3)).reshape(d.shape[:2] + (10,))
    return np.where(wh[..., 0] > 0, wh[..., 9], -1).astype(np.int32)


def coverage_ref(oracle, scene, render_opts, k=2, region=None):
    """The coverage words, uint32 (H, W), zero outside `region` (x, y, w, h). The centre ray is the
    guide pass's (denoise_ref.oracle_guides): pixel00 + du i, then + dv j, then - centre; sub-ray
    (a, b) goes through that pixel centre + du ox, then + dv oy, then - centre, every vector
    operation rounded to fp32. Bit b k + a: the sub-ray's object equals the centre's (a miss is -1);
    bits 16..23: the number of distinct objects among the sub-rays and the centre."""
    ci = oracle.camera_info(scene, render_opts)
    W, H = ci["width"], ci["height"]
    p00, du, dv, cen = (np.asarray(ci[n], dtype=F) for n in ("pixel00", "du", "dv", "center"))
    i = np.arange(W, dtype=F)[None, :, None]
    j = np.arange(H, dtype=F)[:, None, None]
    pc = ((p00 + du * i).astype(F) + (dv * j).astype(F)).astype(F)
    centre = _objects(oracle, scene, cen, pc)
    seen = [centre]
    agree = np.zeros((H, W), np.uint32)
    for bit, ox, oy in sub_offsets(k):
        ps = ((pc + (du * ox).astype(F)).astype(F) + (dv * oy).astype(F)).astype(F)
        obj = _objects(oracle, scene, cen, ps)
        agree |= (obj == centre).astype(np.uint32) << np.uint32(bit)
        seen.append(obj)
    s = np.sort(np.stack(seen), axis=0)
    distinct = (1 + (s[1:] != s[:-1]).sum(0)).astype(np.uint32)
    words = agree | (np.minimum(distinct, 255).astype(np.uint32) << np.uint32(16))
    if region is not None:
        x0, y0, w, h = region
        out = np.zeros_like(words)
        out[y0:y0 + h, x0:x0 + w] = words[y0:y0 + h, x0:x0 + w]
        words = out
    return words


def agree_of(words):
    return (words & np.uint32(0xffff)).astype(np.uint16)


def objects_of(words):
    return ((words >> np.uint32(16)) & np.uint32(0xff)).astype(np.uint8)


def mixed_of(words, k, region=None):
    """bool (H, W): one of the low k^2 bits is clear; False outside `region`."""
    full = np.uint32((1 << (k * k)) - 1)
    m = (words & full) != full
    if region is not None:
        x0, y0, w, h = region
        inside = np.zeros_like(m)
        inside[y0:y0 + h, x0:x0 + w] = True
        m &= inside
    return m


def hold_ref(filtered, noisy, mask):
    """The filter's colour with the hold: a held pixel's colour is its input, as it stands."""
    return np.where(mask[..., None], noisy.astype(F), filtered.astype(F)).astype(F)


def hold_var_ref(filtered_var, var, mask):
    """The variance-guided filter's variance with the hold: a held pixel's variance is its input,
    sanitised as the filter reads it (not (v >= 0 and finite) -> 0)."""
    v = var.astype(F)
    with np.errstate(all="ignore"):
        v = np.where((v >= 0) & np.isfinite(v), v, F(0)).astype(F)
    return np.where(mask, v, filtered_var.astype(F)).astype(F)
