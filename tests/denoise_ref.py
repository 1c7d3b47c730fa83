"""The normative definition of the guided edge-avoiding a-trous filter (rt_denoise) and of the
guide pass's distance, restated in NumPy fp32. Every operation has exactly one fp32 result
(add, multiply, IEEE divide and square root, max, repeated squaring; no exp, no fused
multiply-add, a fixed summation order), so the device output equals this in every bit.
A helper module of the denoise tests, not a test file."""
import numpy as np

F = np.float32
H5 = np.array([1/16, 1/4, 3/8, 1/4, 1/16], dtype=F)   # B3 spline, exact in fp32


def distance_ref(P, center, obj):
    d = (P - center.astype(F)).astype(F)
    s = (d[..., 0]*d[..., 0] + d[..., 1]*d[..., 1]).astype(F) + d[..., 2]*d[..., 2]
    return np.where(obj >= 0, np.sqrt(s.astype(F)), F(0)).astype(F)


def denoise_ref(c, n, P, dist, obj, region=None, levels=4, sigma_color=0.5, sigma_plane=0.01):
    Hh, Ww, _ = c.shape
    x0, y0, w, h = region or (0, 0, Ww, Hh)
    sl = (slice(y0, y0 + h), slice(x0, x0 + w))
    cur = c[sl].astype(F).copy(); n = n[sl]; P = P[sl]; dist = dist[sl]; miss = obj[sl] < 0
    H, W = h, w
    with np.errstate(all="ignore"):
        r_p = F(1) / (F(sigma_plane) * dist)              # per pixel, once
    for lv in range(levels):
        s = 1 << lv
        k_c = F((4.0 ** lv) / (float(F(sigma_color)) * float(F(sigma_color))))  # host, double -> fp32
        sum_c = np.zeros_like(cur); sum_w = np.zeros((H, W), dtype=F)
        fin = np.isfinite(cur).all(-1)
        for dy in range(-2, 3):                            # tap order: dy outer, dx inner
            for dx in range(-2, 3):
                oy, ox = dy * s, dx * s
                ys = slice(max(0, -oy), min(H, H - oy)); xs = slice(max(0, -ox), min(W, W - ox))
                if ys.stop <= ys.start or xs.stop <= xs.start: continue   # taps outside the REGION are skipped
                yq = slice(ys.start + oy, ys.stop + oy); xq = slice(xs.start + ox, xs.stop + ox)
                hk = F(H5[dy + 2] * H5[dx + 2])
                a, b = n[ys, xs], n[yq, xq]
                dn = (a[..., 0]*b[..., 0] + a[..., 1]*b[..., 1]).astype(F) + a[..., 2]*b[..., 2]
                dn = np.maximum(dn, F(0))
                for _ in range(5): dn = dn * dn            # max(0, n.n')^32
                dP = P[yq, xq] - P[ys, xs]
                e = (a[..., 0]*dP[..., 0] + a[..., 1]*dP[..., 1]).astype(F) + a[..., 2]*dP[..., 2]
                cq, cp = cur[yq, xq], cur[ys, xs]
                with np.errstate(all="ignore"):
                    x = e * r_p[ys, xs]                    # plane distance relative to sigma_plane * distance(p)
                    dc = cq - cp
                    y = (dc[..., 0]*dc[..., 0] + dc[..., 1]*dc[..., 1]).astype(F) + dc[..., 2]*dc[..., 2]
                    wt = (hk * dn) / ((F(1) + x * x) * (F(1) + y * k_c))   # one IEEE division per tap
                    wm = hk / (F(1) + y * k_c)             # both pixels are misses: colour weight only
                mp, mq = miss[ys, xs], miss[yq, xq]
                wt = np.where(mp | mq, np.where(mp & mq, wm, F(0)), wt).astype(F)  # hit <-> miss never mix
                ok = np.isfinite(cq).all(-1) & fin[ys, xs]                         # non-finite taps are skipped
                wt = np.where(ok, wt, F(0)).astype(F)
                cq0 = np.where(ok[..., None], cq, F(0)).astype(F)
                sum_c[ys, xs] += wt[..., None] * cq0       # multiply, then add: no fma
                sum_w[ys, xs] += wt
        with np.errstate(all="ignore"):
            nxt = sum_c / sum_w[..., None]
        cur = np.where(fin[..., None], nxt, cur).astype(F) # a non-finite centre is copied through
    out = c.astype(F).copy(); out[sl] = cur
    return out


def to_u8_ref(c):
    """The frame's u8 of a colour (writeColorToBuffer): floor(255.999 sqrt((double)c)) clamped
    to 0..255, non-positive or NaN -> 0."""
    with np.errstate(all="ignore"):
        v = np.floor(255.999 * np.sqrt(c.astype(np.float64)))
    v = np.where(v > 0.0, np.minimum(v, 255.0), 0.0)   # (NaN > 0 is false)
    return v.astype(np.uint8)


# ---- shared fixtures of the denoise tests -----------------------------------------------------
def oracle_guides(oracle, scene, render_opts):
    """The guide buffers as the oracle gives them: the pinhole ray of every pixel built in fp32
    from camera_info (p00 + du i, then + dv j, then - center) through world_hit. Returns
    (normal, position, distance, object, hit) as full-frame arrays."""
    ci = oracle.camera_info(scene, render_opts)
    W, H = ci["width"], ci["height"]
    p00, du, dv, cen = (np.asarray(ci[k], dtype=F) for k in ("pixel00", "du", "dv", "center"))
    i = np.arange(W, dtype=F)[None, :, None]
    j = np.arange(H, dtype=F)[:, None, None]
    pc = ((p00 + du * i).astype(F) + (dv * j).astype(F)).astype(F)
    d = (pc - cen).astype(F)
    o = np.broadcast_to(cen, d.shape)
    wh = oracle.world_hit(scene, o.reshape(-1, 3), d.reshape(-1, 3)).reshape(H, W, 10)
    hit = wh[..., 0] > 0
    P = np.where(hit[..., None], wh[..., 2:5], 0.0).astype(F)
    n = np.where(hit[..., None], wh[..., 5:8], 0.0).astype(F)
    obj = np.where(hit, wh[..., 9], -1).astype(np.int32)
    return n, P, distance_ref(P, cen, obj), obj, hit


def leak_frame():
    """37x23: the left 18 columns normal (1,0,0) colour (1,0,0), the rest normal (0,1,0) colour
    (0,1,0), the top 4 rows misses of colour (0,0,1), one NaN pixel, every position (0,0,5) and
    distance 5. The filter must return it unchanged: normals at right angles weigh 0, the 0 / 1
    colours make every sum exact, hits and misses never mix and the NaN stays in its pixel."""
    H, W = 23, 37
    c = np.zeros((H, W, 3), F); n = np.zeros((H, W, 3), F)
    c[:, :18, 0] = 1; n[:, :18, 0] = 1
    c[:, 18:, 1] = 1; n[:, 18:, 1] = 1
    obj = np.zeros((H, W), np.int32); obj[:, 18:] = 1
    c[:4] = (0, 0, 1); obj[:4] = -1
    c[11, 20] = np.nan
    P = np.zeros((H, W, 3), F); P[..., 2] = 5
    return c, n, P, np.full((H, W), 5, F), obj


def display_mse(a, b):
    """Mean squared error in the display domain sqrt(clip(c, 0, 1))."""
    with np.errstate(all="ignore"):
        da = np.sqrt(np.clip(a.astype(np.float64), 0, 1)); db = np.sqrt(np.clip(b.astype(np.float64), 0, 1))
    return float(np.mean((da - db) ** 2))


def bits_equal(a, b):
    """Elementwise: the same fp32 value (== on bits up to the sign of zero), NaN equal to NaN."""
    return (a == b) | (np.isnan(a) & np.isnan(b))
