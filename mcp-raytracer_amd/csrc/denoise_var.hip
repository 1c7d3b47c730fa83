// Variance map and variance-guided a-trous filter (denoise_var.hpp). Compiled like denoise.hip:
// -ffp-contract=off and no fast-math, denormal-flushing or approximate-reciprocal flag, so every
// fp32 operation of the filter and every fp64 operation of the variance has exactly one result;
// the tap order and the multiply-then-add accumulation are part of the definition -
// tests/denoise_var_ref.py.
#include "denoise_var.hpp"

#include <algorithm>

namespace rt {

constexpr int kDvBlock = 256;
constexpr uint32_t kDvFlag = 0x80000000u;  // colour.w's sign bit: the colour is not finite

__device__ __forceinline__ bool dv_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ bool dv_flag(const float4& c) { return (__float_as_uint(c.w) & kDvFlag) != 0u; }
__device__ __forceinline__ float dv_var(const float4& c) { return __uint_as_float(__float_as_uint(c.w) & ~kDvFlag); }
__device__ __forceinline__ float dv_pack_w(float v, bool finite) {
    return __uint_as_float((__float_as_uint(v) & ~kDvFlag) | (finite ? 0u : kDvFlag));
}
// Color.illuminance of a colour, in the definition's order
__device__ __forceinline__ float dv_lum(const float4& c) { return (0.299f * c.x + 0.587f * c.y) + 0.114f * c.z; }

// ---- variance pass ----------------------------------------------------------------------------
__global__ __launch_bounds__(kDvBlock) void prog_variance_kernel(const ProgPix* __restrict__ state, int slots,
                                                                  RtRegion reg, int tiles_x,
                                                                  float* __restrict__ variance) {
    const int slot = blockIdx.x * kDvBlock + (int)threadIdx.x;
    if (slot >= slots) return;
    int i, j;
    item_pixel(reg, tiles_x, slot / kWave, slot & (kWave - 1), i, j);
    if (i >= reg.x + reg.width || j >= reg.y + reg.height) return;
    const uint32_t n = __float_as_uint(state[slot].c.w) & ~kProgFinished;
    const double2 ill = state[slot].ill;
    variance[(size_t)(j - reg.y) * (size_t)reg.width + (size_t)(i - reg.x)] = prog_variance(ill.x, ill.y, n);
}

// ---- pack / unpack ----------------------------------------------------------------------------
__global__ __launch_bounds__(kDvBlock) void denoise_var_pack_kernel(const float* rad, int pitch_px, int x0, int y0, int w,
                                                                     int h, const float4* gn, float sigma_plane,
                                                                     const float* variance, float4* colour, float4* fn) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= w * h) return;
    const int y = k / w, x = k - y * w;
    const float* s = rad + 3 * ((size_t)(y0 + y) * (size_t)pitch_px + (size_t)(x0 + x));
    const float r = s[0], g = s[1], b = s[2];
    const float v = variance[k];
    const float vs = v >= 0.0f && dv_finite(v) ? v : 0.0f;  // sanitised once: NaN, negatives and inf -> 0
    colour[k] = make_float4(r, g, b, dv_pack_w(vs, dv_finite(r) && dv_finite(g) && dv_finite(b)));
    const float4 a = gn[k];
    fn[k] = make_float4(a.x, a.y, a.z, 1.0f / (sigma_plane * a.w));
}

__global__ __launch_bounds__(kDvBlock) void denoise_var_unpack_kernel(const float4* colour, int n, float* variance) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    variance[k] = dv_var(colour[k]);
}

// ---- filter -----------------------------------------------------------------------------------
// The B3 spline's taps and the pre-blur's (1/4, 1/2, 1/4): exact in fp32, and so are their products.
__device__ __forceinline__ float dv_h5(int k) { return k == 2 ? 0.375f : (k == 1 || k == 3) ? 0.25f : 0.0625f; }
__device__ __forceinline__ float dv_h3(int k) { return k == 1 ? 0.5f : 0.25f; }

struct DvSum {
    float r, g, b, w, v;
};

// One tap of pixel p (luminance lp, guides np / pp, finite flag finp, miss flag missp, falloff
// k_p) at pixel q, in the definition's operation order.
__device__ __forceinline__ void dv_tap(float lp, const float4& np, const float4& pp, bool finp, bool missp,
                                       const float4& cq, const float4& nq, const float4& pq, float hk, float k_p,
                                       DvSum& s) {
    float dn = (np.x * nq.x + np.y * nq.y) + np.z * nq.z;
    dn = dn < 0.0f ? 0.0f : dn;  // max(dn, 0), a NaN kept
    dn = dn * dn;
    dn = dn * dn;
    dn = dn * dn;
    dn = dn * dn;
    dn = dn * dn;  // ^32
    const float dpx = pq.x - pp.x, dpy = pq.y - pp.y, dpz = pq.z - pp.z;
    const float e = (np.x * dpx + np.y * dpy) + np.z * dpz;
    const float x = e * np.w;
    const float d = dv_lum(cq) - lp;
    const float cw = 1.0f + (d * d) * k_p;
    const bool missq = __float_as_int(pq.w) < 0;
    // two misses: the luminance weight only; a hit and a miss never mix. One IEEE division.
    const bool both = missp && missq;
    const float num = both ? hk : hk * dn;
    const float den = both ? cw : (1.0f + x * x) * cw;
    const float wq = num / den;
    const bool ok = finp && !dv_flag(cq);  // non-finite taps are skipped
    const float wt = ok && missp == missq ? wq : 0.0f;
    s.r = s.r + wt * (ok ? cq.x : 0.0f);
    s.g = s.g + wt * (ok ? cq.y : 0.0f);
    s.b = s.b + wt * (ok ? cq.z : 0.0f);
    s.w = s.w + wt;
    s.v = s.v + (wt * wt) * (ok ? dv_var(cq) : 0.0f);
}

// k_p = 1 / (s2 * gv + 1e-10f) from the pre-blur's sums
__device__ __forceinline__ float dv_falloff(float sv, float sw, float s2) { return 1.0f / (s2 * (sv / sw) + 1e-10f); }

__device__ __forceinline__ float4 dv_finish(const float4& cp, bool finp, const DvSum& s) {
    float4 o = cp;
    float v = dv_var(cp);
    if (finp) {  // (a non-finite centre keeps its colour and its variance)
        o.x = s.r / s.w;
        o.y = s.g / s.w;
        o.z = s.b / s.w;
        v = s.v / (s.w * s.w);
    }
    o.w = dv_pack_w(v, dv_finite(o.x) && dv_finite(o.y) && dv_finite(o.z));
    return o;
}

// Steps 1 and 2: as denoise_lds_kernel, a 16x16 tile and its 2 * STEP halo in LDS as three float4
// planes (19 and 27 KB); the variance rides in the colour plane's w, and the halo (>= 2) covers
// the pre-blur's +-1. Cells outside the region are never read.
constexpr int kDvTile = 16;
template <int STEP>
__global__ __launch_bounds__(kDvBlock) void denoise_var_lds_kernel(const float4* __restrict__ src,
                                                                    float4* __restrict__ dst,
                                                                    const float4* __restrict__ fn,
                                                                    const float4* __restrict__ gp, int w, int h,
                                                                    float s2) {
    constexpr int R = 2 * STEP, LW = kDvTile + 2 * R;
    __shared__ float4 sc[LW * LW];
    __shared__ float4 sn[LW * LW];
    __shared__ float4 sp[LW * LW];
    const int bx0 = blockIdx.x * kDvTile, by0 = blockIdx.y * kDvTile;
    for (int k = threadIdx.x; k < LW * LW; k += kDvBlock) {
        const int ly = k / LW, lx = k - ly * LW;
        const int gx = bx0 - R + lx, gy = by0 - R + ly;
        if (gx >= 0 && gx < w && gy >= 0 && gy < h) {
            const size_t q = (size_t)gy * (size_t)w + (size_t)gx;
            sc[k] = src[q];
            sn[k] = fn[q];
            sp[k] = gp[q];
        }
    }
    __syncthreads();
    const int tx = threadIdx.x & (kDvTile - 1), ty = threadIdx.x / kDvTile;
    const int px = bx0 + tx, py = by0 + ty;
    if (px >= w || py >= h) return;
    const int lc = (ty + R) * LW + tx + R;
    const float4 cp = sc[lc], np = sn[lc], pp = sp[lc];
    const bool finp = !dv_flag(cp), missp = __float_as_int(pp.w) < 0;
    float sv = 0.0f, sw = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = px + dx, qy = py + dy;
            if (qx < 0 || qx >= w || qy < 0 || qy >= h) continue;
            const float hk = dv_h3(dy + 1) * dv_h3(dx + 1);
            sv = sv + hk * dv_var(sc[lc + dy * LW + dx]);
            sw = sw + hk;
        }
    }
    const float k_p = dv_falloff(sv, sw, s2);
    const float lp = dv_lum(cp);
    DvSum s{0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = px + dx * STEP, qy = py + dy * STEP;
            if (qx < 0 || qx >= w || qy < 0 || qy >= h) continue;  // taps outside the region are skipped
            const int lq = lc + dy * STEP * LW + dx * STEP;
            dv_tap(lp, np, pp, finp, missp, sc[lq], sn[lq], sp[lq], dv_h5(dy + 2) * dv_h5(dx + 2), k_p, s);
        }
    }
    dst[(size_t)py * (size_t)w + (size_t)px] = dv_finish(cp, finp, s);
}

// Larger steps: global reads (L2 / MALL) in workgroups of 4 rows of 64 pixels, as
// denoise_global_kernel; the pre-blur's nine variances are the w lanes of the centre's
// neighbours, which share its cache lines.
constexpr int kDvRow = 64;
__global__ __launch_bounds__(kDvBlock) void denoise_var_global_kernel(const float4* __restrict__ src,
                                                                       float4* __restrict__ dst,
                                                                       const float4* __restrict__ fn,
                                                                       const float4* __restrict__ gp, int w, int h,
                                                                       int step, float s2) {
    const int px = blockIdx.x * kDvRow + (int)(threadIdx.x & (kDvRow - 1));
    const int py = blockIdx.y * (kDvBlock / kDvRow) + (int)(threadIdx.x / kDvRow);
    if (px >= w || py >= h) return;
    const size_t pc = (size_t)py * (size_t)w + (size_t)px;
    const float4 cp = src[pc], np = fn[pc], pp = gp[pc];
    const bool finp = !dv_flag(cp), missp = __float_as_int(pp.w) < 0;
    float sv = 0.0f, sw = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
        const int qy = py + dy;
        if (qy < 0 || qy >= h) continue;
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = px + dx;
            if (qx < 0 || qx >= w) continue;
            const float hk = dv_h3(dy + 1) * dv_h3(dx + 1);
            sv = sv + hk * dv_var(src[(size_t)qy * (size_t)w + (size_t)qx]);
            sw = sw + hk;
        }
    }
    const float k_p = dv_falloff(sv, sw, s2);
    const float lp = dv_lum(cp);
    DvSum s{0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = py + dy * step;
        if (qy < 0 || qy >= h) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = px + dx * step;
            if (qx < 0 || qx >= w) continue;
            const size_t q = (size_t)qy * (size_t)w + (size_t)qx;
            dv_tap(lp, np, pp, finp, missp, src[q], fn[q], gp[q], dv_h5(dy + 2) * dv_h5(dx + 2), k_p, s);
        }
    }
    dst[pc] = dv_finish(cp, finp, s);
}

// ---- launches ---------------------------------------------------------------------------------
static dim3 dv_grid1(long n) { return dim3((unsigned)std::max(1l, (n + kDvBlock - 1) / kDvBlock)); }

hipError_t launch_prog_variance(const ProgPix* state, int slots, const RtRegion& reg, int tiles_x, float* variance,
                                hipStream_t stream) {
    if (slots <= 0) return hipSuccess;
    const RtRegion r{reg.x, reg.y, reg.width, reg.height, 0, 1};
    hipLaunchKernelGGL(prog_variance_kernel, dv_grid1(slots), dim3(kDvBlock), 0, stream, state, slots, r, tiles_x,
                       variance);
    return hipGetLastError();
}

hipError_t launch_denoise_var_pack(const float* rad, int pitch_px, int x0, int y0, int w, int h, const float4* gn,
                                   float sigma_plane, const float* variance, float4* colour, float4* fn,
                                   hipStream_t stream) {
    if (w <= 0 || h <= 0) return hipSuccess;
    hipLaunchKernelGGL(denoise_var_pack_kernel, dv_grid1((long)w * h), dim3(kDvBlock), 0, stream, rad, pitch_px, x0, y0, w,
                       h, gn, sigma_plane, variance, colour, fn);
    return hipGetLastError();
}

hipError_t launch_denoise_var_level(const float4* src, float4* dst, const float4* fn, const float4* gp, int w, int h,
                                    int step, float s2, hipStream_t stream) {
    if (w <= 0 || h <= 0) return hipSuccess;
    const dim3 tiles((unsigned)((w + kDvTile - 1) / kDvTile), (unsigned)((h + kDvTile - 1) / kDvTile));
    if (step == 1)
        hipLaunchKernelGGL(denoise_var_lds_kernel<1>, tiles, dim3(kDvBlock), 0, stream, src, dst, fn, gp, w, h, s2);
    else if (step == 2)
        hipLaunchKernelGGL(denoise_var_lds_kernel<2>, tiles, dim3(kDvBlock), 0, stream, src, dst, fn, gp, w, h, s2);
    else
        hipLaunchKernelGGL(denoise_var_global_kernel,
                           dim3((unsigned)((w + kDvRow - 1) / kDvRow),
                                (unsigned)((h + kDvBlock / kDvRow - 1) / (kDvBlock / kDvRow))),
                           dim3(kDvBlock), 0, stream, src, dst, fn, gp, w, h, step, s2);
    return hipGetLastError();
}

hipError_t launch_denoise_var_unpack(const float4* colour, int n, float* variance, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(denoise_var_unpack_kernel, dv_grid1(n), dim3(kDvBlock), 0, stream, colour, n, variance);
    return hipGetLastError();
}

}  // namespace rt
