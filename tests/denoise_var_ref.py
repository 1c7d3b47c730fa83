"""The normative definition of the variance-guided a-trous filter (rt_denoise_variance) and of
the progressive session's variance map (rt_camera_progressive_variance,
rt_progressive_blob_variance), restated in NumPy. The filter is tests/denoise_ref.py's with the
colour edge-stop replaced by a luminance difference relative to the centre pixel's pre-blurred
variance, and a variance channel carried along; every operation has exactly one fp32 result
(add, multiply, IEEE divide, max, repeated squaring; no exp, no fused multiply-add, a fixed
summation order), so the device output - colour and variance - equals this in every bit. The
variance map is fp64 arithmetic in the reference's expression order, rounded to fp32 once.
A helper module of the denoise_var tests, not a test file."""
import struct

import numpy as np

from denoise_ref import F, H5

H3 = np.array([1/4, 1/2, 1/4], dtype=F)            # the variance pre-blur, exact in fp32
LUM = (F(0.299), F(0.587), F(0.114))               # Color.illuminance
EPS = F(1e-10)


def luminance(c):
    return (LUM[0]*c[..., 0] + LUM[1]*c[..., 1]).astype(F) + LUM[2]*c[..., 2]


def _taps(H, W, oy, ox):
    """Slices (centres ys, xs; taps yq, xq) of the pixels whose tap at offset (oy, ox) lies in
    the H x W region, or None when there are none."""
    ys = slice(max(0, -oy), min(H, H - oy)); xs = slice(max(0, -ox), min(W, W - ox))
    if ys.stop <= ys.start or xs.stop <= xs.start: return None
    return ys, xs, slice(ys.start + oy, ys.stop + oy), slice(xs.start + ox, xs.stop + ox)


def preblur_ref(v):
    """3x3 blur of the variance at UNIT spacing, weights (1/4, 1/2, 1/4)^2, over the in-region
    taps, normalised by the sum of the weights used (dy outer, dx inner; multiply, then add)."""
    H, W = v.shape
    sv = np.zeros((H, W), F); sw = np.zeros((H, W), F)
    for dy in range(-1, 2):
        for dx in range(-1, 2):
            ys, xs, yq, xq = _taps(H, W, dy, dx)
            hk = F(H3[dy + 1] * H3[dx + 1])
            with np.errstate(all="ignore"):
                sv[ys, xs] += hk * v[yq, xq]
            sw[ys, xs] += hk
    with np.errstate(all="ignore"):
        return (sv / sw).astype(F)


def denoise_var_ref(c, var, n, P, dist, obj, region=None, levels=4, sigma_variance=2.0, sigma_plane=0.01):
    """Returns (colour (H, W, 3), variance (H, W)): the inputs with the region filtered."""
    Hh, Ww, _ = c.shape
    x0, y0, w, h = region or (0, 0, Ww, Hh)
    sl = (slice(y0, y0 + h), slice(x0, x0 + w))
    cur = c[sl].astype(F).copy(); n = n[sl]; P = P[sl]; dist = dist[sl]; miss = obj[sl] < 0
    v = var[sl].astype(F)
    v = np.where((v >= 0) & np.isfinite(v), v, F(0)).astype(F)   # sanitised once, at pack time
    H, W = h, w
    s2 = F(float(F(sigma_variance)) * float(F(sigma_variance)))   # host, double -> fp32
    with np.errstate(all="ignore"):
        r_p = F(1) / (F(sigma_plane) * dist)              # per pixel, once
    for lv in range(levels):
        s = 1 << lv
        with np.errstate(all="ignore"):
            k = F(1) / ((s2 * preblur_ref(v)).astype(F) + EPS)   # the centre pixel's falloff k_p
        lum = luminance(cur)
        sum_c = np.zeros_like(cur); sum_w = np.zeros((H, W), dtype=F); sum_v = np.zeros((H, W), dtype=F)
        fin = np.isfinite(cur).all(-1)
        for dy in range(-2, 3):                            # tap order: dy outer, dx inner
            for dx in range(-2, 3):
                t = _taps(H, W, dy * s, dx * s)
                if t is None: continue                     # taps outside the REGION are skipped
                ys, xs, yq, xq = t
                hk = F(H5[dy + 2] * H5[dx + 2])
                a, b = n[ys, xs], n[yq, xq]
                dn = (a[..., 0]*b[..., 0] + a[..., 1]*b[..., 1]).astype(F) + a[..., 2]*b[..., 2]
                dn = np.maximum(dn, F(0))
                for _ in range(5): dn = dn * dn            # max(0, n.n')^32
                dP = P[yq, xq] - P[ys, xs]
                e = (a[..., 0]*dP[..., 0] + a[..., 1]*dP[..., 1]).astype(F) + a[..., 2]*dP[..., 2]
                cq = cur[yq, xq]
                with np.errstate(all="ignore"):
                    x = e * r_p[ys, xs]                    # plane distance relative to sigma_plane * distance(p)
                    d = lum[yq, xq] - lum[ys, xs]
                    cw = F(1) + (d * d) * k[ys, xs]
                    wt = (hk * dn) / ((F(1) + x * x) * cw) # one IEEE division per tap
                    wm = hk / cw                           # both pixels are misses: luminance weight only
                mp, mq = miss[ys, xs], miss[yq, xq]
                wt = np.where(mp | mq, np.where(mp & mq, wm, F(0)), wt).astype(F)  # hit <-> miss never mix
                ok = np.isfinite(cq).all(-1) & fin[ys, xs]                         # non-finite taps are skipped
                wt = np.where(ok, wt, F(0)).astype(F)
                cq0 = np.where(ok[..., None], cq, F(0)).astype(F)
                vq0 = np.where(ok, v[yq, xq], F(0)).astype(F)
                with np.errstate(all="ignore"):
                    sum_c[ys, xs] += wt[..., None] * cq0   # multiply, then add: no fma
                    sum_w[ys, xs] += wt
                    sum_v[ys, xs] += (wt * wt) * vq0
        with np.errstate(all="ignore"):
            nxt = sum_c / sum_w[..., None]
            nxv = sum_v / (sum_w * sum_w)
        cur = np.where(fin[..., None], nxt, cur).astype(F) # a non-finite centre keeps its colour
        v = np.abs(np.where(fin, nxv, v)).astype(F)        # ... and its variance (|.|: a NaN's sign is not defined)
    out = c.astype(F).copy(); out[sl] = cur
    vout = var.astype(F).copy(); vout[sl] = v
    return out, vout


# ---- the variance map -------------------------------------------------------------------------
BLOB_HEADER = struct.Struct("<8sII24s7iIdiiiiqQQQQQ")    # the checkpoint blob's 144-byte header
PROG_PIX = np.dtype([("c", "<f4", 3), ("n", "<u4"), ("sumIll", "<f8"), ("sumIll2", "<f8"), ("b", "<i4", 4)])
assert BLOB_HEADER.size == 144 and PROG_PIX.itemsize == 48


def blob_state(blob):
    """(width, height, region, per-slot records) of a checkpoint blob: the documented payload,
    48 bytes per slot (slot = region tile * 64 + lane, 8x8 tiles row-major over the region, lane
    = 8 * row + column) - colour sum, n (bit 31: finished), sumIll, sumIll2, bounce words."""
    f = BLOB_HEADER.unpack_from(blob)
    width, height, rx, ry, rw, rh = f[4:10]
    payload = f[-3]
    st = np.frombuffer(blob, dtype=PROG_PIX, count=payload // 48, offset=BLOB_HEADER.size)
    return width, height, (rx, ry, rw, rh), st


def variance_from_state(sum_ill, sum_ill2, n):
    """Variance of the pixel mean's illuminance (src/camera.ts:356-357, then / n) in fp64, then
    fp32: m2 = sumIll2 - (sumIll sumIll) / n; v = (m2 / (n - 1)) / n; NaN, negatives, n < 2 -> 0."""
    nd = n.astype(np.float64)
    with np.errstate(all="ignore"):
        m2 = sum_ill2 - (sum_ill * sum_ill) / nd
        v = (m2 / (nd - 1.0)) / nd
    v = np.where((n >= 2) & (v > 0), v, 0.0)               # (NaN > 0 is false)
    with np.errstate(all="ignore"):
        return v.astype(F)


def blob_pixels(blob):
    """(width, height, region, j, i, records): the blob's records of the slots inside the region
    and their pixel coordinates."""
    width, height, (rx, ry, rw, rh), st = blob_state(blob)
    tiles_x = (rw + 7) // 8
    slot = np.arange(st.size)
    tile, lane = slot // 64, slot % 64
    i = rx + (tile % tiles_x) * 8 + (lane & 7)
    j = ry + (tile // tiles_x) * 8 + lane // 8
    inside = (i < rx + rw) & (j < ry + rh)
    return width, height, (rx, ry, rw, rh), j[inside], i[inside], st[inside]


def variance_from_blob(blob):
    """The variance map of a checkpoint blob: float32 (height, width), zero outside the region."""
    width, height, _, j, i, st = blob_pixels(blob)
    out = np.zeros((height, width), F)
    out[j, i] = variance_from_state(st["sumIll"], st["sumIll2"], st["n"] & np.uint32(0x7fffffff))
    return out


def samples_from_blob(blob):
    """Per-pixel sample counts n of a checkpoint blob: int64 (height, width), zero outside the region."""
    width, height, _, j, i, st = blob_pixels(blob)
    out = np.zeros((height, width), np.int64)
    out[j, i] = st["n"] & np.uint32(0x7fffffff)
    return out


# ---- shared fixtures of the denoise_var tests -------------------------------------------------
def oracle_window(oracle, scene, render_opts, spp):
    """A noisy frame of `spp` samples per pixel and the variance of its mean illuminance, from
    the oracle alone. The oracle renders whole frames, so single samples are recovered from
    frames of successive `samples`: sample k-1 = k frame(k) - (k-1) frame(k-1) (fp64), k =
    3 .. spp + 2. NOTE: this window is samples 2 .. spp+1 of every pixel, not the product's
    0 .. spp-1 (frame(1) - 0 would give sample 0, but the window stays clear of the first
    frames so that every difference is formed the same way), and the recovered samples carry
    the frames' fp32 rounding; the GPU end-to-end test uses the product's own window.
    Returns (frame float32 (H, W, 3), variance float32 (H, W))."""
    frames = {k: oracle.render(scene, {**render_opts, "samples": k}, threads=16)["radiance"].astype(np.float64)
              for k in range(2, spp + 3)}
    samples = [k * frames[k] - (k - 1) * frames[k - 1] for k in range(3, spp + 3)]
    ill = [0.299 * s[..., 0] + 0.587 * s[..., 1] + 0.114 * s[..., 2] for s in samples]
    frame = (sum(samples) / spp).astype(F)
    s1 = sum(ill); s2 = sum(x * x for x in ill)
    n = np.full(s1.shape, spp, np.uint32)
    return frame, variance_from_state(s1, s2, n)
