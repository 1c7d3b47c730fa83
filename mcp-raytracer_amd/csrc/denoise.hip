// Guide pass and a-trous filter (denoise.hpp). Compiled with -ffp-contract=off and without any
// fast-math, denormal-flushing or approximate-reciprocal flag: every fp32 operation of the
// filter (add, multiply, IEEE divide, max, repeated squaring) and of the guide distance
// (correctly rounded sqrtf) has exactly one result, and the tap order and the
// multiply-then-add accumulation are part of it - tests/denoise_ref.py is the definition, and
// tests/denoise_var_ref.py that of the variance-guided form.
#include "denoise.hpp"

#include <algorithm>

#include "pt_pixel.hpp"  // item_pixel
#include "pt_shade.hpp"  // pixel_center, closest_hit_any

namespace rt {

// ---- guide pass -------------------------------------------------------------------------------
// One thread per pixel, a wave per 8x8 tile of the region (item_pixel numbering), so a wave's
// rays stay coherent. Stack and residency as world_hit_kernel: the traversal stack (or the
// brute force's candidate bounds) in LDS, the scene read from global memory.
template <int TRAV>
__global__ __launch_bounds__(kBlock) void guide_kernel(DevScene S, RtRegion reg, int tiles_x, int n_tiles,
                                                       const int32_t* prim_object, DenoiseGuides g) {
    extern __shared__ int lds_stack[];
    const int tile = blockIdx.x * (kBlock / kWave) + (int)(threadIdx.x / kWave);
    if (tile >= n_tiles) return;
    int i, j;
    item_pixel(reg, tiles_x, tile, (int)(threadIdx.x & (kWave - 1)), i, j);
    if (i >= reg.x + reg.width || j >= reg.y + reg.height) return;
    const RtCamera& C = S.cam;
    // Camera.getRay of a `samples: 1`, `aperture: 0` camera (src/camera.ts:176-210)
    const V3 o = ld3(C.center);
    const V3 d = sub(pixel_center<double>(C, i, j), o);
    const RayK<double> r = make_ray<double>(o, d);
    double t = 0;
    int* stk = lds_stack + threadIdx.x;
    const int h = closest_hit_any<double, false, TRAV>(S, C.n_prims, r, t, stk, nullptr);
    float4 gn = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 gp = make_float4(0.f, 0.f, 0.f, __int_as_float(-1));
    if (h >= 0) {
        const RtPrim pr = S.prims[h];
        const V3 p = ray_at<double>(o, d, t);
        V3 nrm;
        if (pr.type == PRIM_SPHERE) {
            nrm = divs<double>(sub(p, ld3(pr.g0)), sphere_radius<double>(pr));
            if (!(dot<double>(d, nrm) <= 0.0)) nrm = neg(nrm);
        } else {
            const V3 pn = ld3(pr.g3);
            nrm = dot<double>(d, pn) <= 0.0 ? pn : neg(pn);
        }
        const V3 q = sub(p, o);
        const float dist = ::sqrtf((q.x * q.x + q.y * q.y) + q.z * q.z);
        gn = make_float4(nrm.x, nrm.y, nrm.z, dist);
        gp = make_float4(p.x, p.y, p.z, __int_as_float(prim_object[h]));
    }
    const size_t k = (size_t)(j - reg.y) * (size_t)reg.width + (size_t)(i - reg.x);
    g.gn[k] = gn;
    g.gp[k] = gp;
}

constexpr int kDnBlock = 256;

__global__ __launch_bounds__(kDnBlock) void guides_unpack_kernel(DenoiseGuides g, int n, float* normal, float* position,
                                                                  float* distance, int32_t* object) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const float4 a = g.gn[k], b = g.gp[k];
    if (normal) {
        normal[3 * (size_t)k] = a.x;
        normal[3 * (size_t)k + 1] = a.y;
        normal[3 * (size_t)k + 2] = a.z;
    }
    if (position) {
        position[3 * (size_t)k] = b.x;
        position[3 * (size_t)k + 1] = b.y;
        position[3 * (size_t)k + 2] = b.z;
    }
    if (distance) distance[k] = a.w;
    if (object) object[k] = __float_as_int(b.w);
}

__global__ __launch_bounds__(kDnBlock) void guides_pack_kernel(DenoiseGuides g, int n, const float* normal,
                                                                const float* position, const float* distance,
                                                                const int32_t* object) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    g.gn[k] = make_float4(normal[3 * (size_t)k], normal[3 * (size_t)k + 1], normal[3 * (size_t)k + 2], distance[k]);
    g.gp[k] = make_float4(position[3 * (size_t)k], position[3 * (size_t)k + 1], position[3 * (size_t)k + 2],
                          __int_as_float(object[k]));
}

// ---- filter -----------------------------------------------------------------------------------
// One filter, two forms chosen at compile time (VAR: the variance-guided one). They differ in
// the colour weight, in the variance lane (pre-blur, accumulation, divide) and in what colour.w
// holds - the helpers below and the `if constexpr (VAR)` lines; everything else is written once.
__device__ __forceinline__ bool finite_f(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// colour.w. Plain: the finite flag, 1.0f / 0.0f. VAR: the variance, its sign bit set when the
// colour is not finite.
constexpr uint32_t kDnFlag = 0x80000000u;
template <bool VAR>
__device__ __forceinline__ bool dn_is_finite(const float4& c) {
    if constexpr (VAR) return (__float_as_uint(c.w) & kDnFlag) == 0u;
    else return c.w != 0.0f;
}
__device__ __forceinline__ float dn_var(const float4& c) { return __uint_as_float(__float_as_uint(c.w) & ~kDnFlag); }
template <bool VAR>
__device__ __forceinline__ float dn_pack_w(float v, bool finite) {
    if constexpr (VAR) return __uint_as_float((__float_as_uint(v) & ~kDnFlag) | (finite ? 0u : kDnFlag));
    else return finite ? 1.0f : 0.0f;
}
// Color.illuminance of a colour, in the definition's order
__device__ __forceinline__ float dn_lum(const float4& c) { return (0.299f * c.x + 0.587f * c.y) + 0.114f * c.z; }

template <bool VAR>
__global__ __launch_bounds__(kDnBlock) void denoise_pack_kernel(const float* rad, int pitch_px, int x0, int y0, int w,
                                                                 int h, const float4* gn, float sigma_plane,
                                                                 float4* colour, float4* fn, const float* variance) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= w * h) return;
    const int y = k / w, x = k - y * w;
    const float* s = rad + 3 * ((size_t)(y0 + y) * (size_t)pitch_px + (size_t)(x0 + x));
    const float r = s[0], g = s[1], b = s[2];
    float vs = 0.0f;
    if constexpr (VAR) {
        const float v = variance[k];
        vs = v >= 0.0f && finite_f(v) ? v : 0.0f;  // sanitised once: NaN, negatives and inf -> 0
    }
    colour[k] = make_float4(r, g, b, dn_pack_w<VAR>(vs, finite_f(r) && finite_f(g) && finite_f(b)));
    const float4 a = gn[k];
    fn[k] = make_float4(a.x, a.y, a.z, 1.0f / (sigma_plane * a.w));
}

// hd.mask (or null): a held pixel's outputs are the filter's INPUTS, read again where the pack pass
// read them - the colour as it stands, the variance sanitised as there. Each thread reads its own
// pixel's inputs before it writes, so the outputs may be the input arrays themselves.
__global__ __launch_bounds__(kDnBlock) void denoise_unpack_kernel(const float4* colour, int n, float* rad, uint8_t* rgb,
                                                                   float* variance, DenoiseHold hd) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    float4 c = colour[k];
    if (hd.mask && hd.mask[k]) {
        const int y = k / hd.w, x = k - y * hd.w;
        const float* s = hd.rad + 3 * ((size_t)(hd.y0 + y) * (size_t)hd.pitch_px + (size_t)(hd.x0 + x));
        float vs = 0.0f;
        if (hd.variance) {
            const float v = hd.variance[k];
            vs = v >= 0.0f && finite_f(v) ? v : 0.0f;
        }
        c = make_float4(s[0], s[1], s[2], vs);
    }
    if (variance) variance[k] = dn_var(c);
    if (rad) {
        rad[3 * (size_t)k] = c.x;
        rad[3 * (size_t)k + 1] = c.y;
        rad[3 * (size_t)k + 2] = c.z;
    }
    if (rgb) {
        rgb[3 * (size_t)k] = to_u8(c.x);
        rgb[3 * (size_t)k + 1] = to_u8(c.y);
        rgb[3 * (size_t)k + 2] = to_u8(c.z);
    }
}

// The B3 spline's taps and the pre-blur's (1/4, 1/2, 1/4): exact in fp32, and so are their products.
__device__ __forceinline__ float h5(int k) {
    return k == 2 ? 0.375f : (k == 1 || k == 3) ? 0.25f : 0.0625f;
}
__device__ __forceinline__ float h3(int k) { return k == 1 ? 0.5f : 0.25f; }

// A pixel's weighted sums. The plain form has no variance lane at all: a dead one is removed
// but still renumbers the kernel's registers.
template <bool VAR>
struct DnSum {
    float r, g, b, w;
};
template <>
struct DnSum<true> {
    float r, g, b, w, v;
};

// The centre pixel's part of the colour weight. Plain: nothing, the launch's k_c = 4^level /
// sigma_color^2 is the falloff. VAR: its luminance, and k_p = 1 / (s2 * gv + 1e-10f), gv the
// 3x3 (1/4, 1/2, 1/4) blur of the variance around it; var_at(dx, dy) reads a neighbour's
// variance, and neighbours outside the region are skipped.
struct DnCentre {
    float lum, k;
};
template <class VarAt>
__device__ __forceinline__ DnCentre dn_centre(const float4& cp, int px, int py, int w, int h, float s2, VarAt var_at) {
    float sv = 0.0f, sw = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = px + dx, qy = py + dy;
            if (qx < 0 || qx >= w || qy < 0 || qy >= h) continue;
            const float hk = h3(dy + 1) * h3(dx + 1);
            sv = sv + hk * var_at(dx, dy);
            sw = sw + hk;
        }
    }
    return DnCentre{dn_lum(cp), 1.0f / (s2 * (sv / sw) + 1e-10f)};
}

// One tap of pixel p (colour cp, centre part ce, guides np / pp, finite flag finp, miss flag
// missp) at pixel q, in the definition's operation order.
template <bool VAR>
__device__ __forceinline__ void dn_tap(const float4& cp, const DnCentre& ce, const float4& np, const float4& pp, bool finp,
                                       bool missp, const float4& cq, const float4& nq, const float4& pq, float hk,
                                       DnSum<VAR>& s) {
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
    float cw;
    if constexpr (VAR) {  // the luminance difference against the centre's own variance
        const float d = dn_lum(cq) - ce.lum;
        cw = 1.0f + (d * d) * ce.k;
    } else {  // the RGB distance
        const float dcx = cq.x - cp.x, dcy = cq.y - cp.y, dcz = cq.z - cp.z;
        const float y = (dcx * dcx + dcy * dcy) + dcz * dcz;
        cw = 1.0f + y * ce.k;
    }
    const bool missq = __float_as_int(pq.w) < 0;
    // two misses: the colour weight only; a hit and a miss never mix. One IEEE division.
    const bool both = missp && missq;
    const float num = both ? hk : hk * dn;
    const float den = both ? cw : (1.0f + x * x) * cw;
    const float wq = num / den;
    const bool ok = finp && dn_is_finite<VAR>(cq);  // non-finite taps are skipped
    const float wt = ok && missp == missq ? wq : 0.0f;
    s.r = s.r + wt * (ok ? cq.x : 0.0f);
    s.g = s.g + wt * (ok ? cq.y : 0.0f);
    s.b = s.b + wt * (ok ? cq.z : 0.0f);
    s.w = s.w + wt;
    if constexpr (VAR) s.v = s.v + (wt * wt) * (ok ? dn_var(cq) : 0.0f);
}

template <bool VAR>
__device__ __forceinline__ float4 dn_finish(const float4& cp, bool finp, const DnSum<VAR>& s) {
    float4 o = cp;
    float v = dn_var(cp);
    if (finp) {  // (a non-finite centre is copied through, and keeps its variance)
        o.x = s.r / s.w;
        o.y = s.g / s.w;
        o.z = s.b / s.w;
        if constexpr (VAR) v = s.v / (s.w * s.w);
    }
    o.w = dn_pack_w<VAR>(v, finite_f(o.x) && finite_f(o.y) && finite_f(o.z));
    return o;
}

// Steps 1 and 2: a 16x16 tile and its 2 * STEP halo staged in LDS as three float4 planes
// (20x20 at step 1, 24x24 at step 2: 19 and 27 KB), so each input is fetched once per tile
// instead of up to 25 times. Cells outside the region are never read (their taps are skipped).
// The halo (>= 2) covers the pre-blur's +-1.
constexpr int kDnTile = 16;
template <bool VAR, int STEP>
__global__ __launch_bounds__(kDnBlock) void denoise_lds_kernel(const float4* __restrict__ src, float4* __restrict__ dst,
                                                                const float4* __restrict__ fn,
                                                                const float4* __restrict__ gp, int w, int h, float ks) {
    constexpr int R = 2 * STEP, LW = kDnTile + 2 * R;
    __shared__ float4 sc[LW * LW];
    __shared__ float4 sn[LW * LW];
    __shared__ float4 sp[LW * LW];
    const int bx0 = blockIdx.x * kDnTile, by0 = blockIdx.y * kDnTile;
    for (int k = threadIdx.x; k < LW * LW; k += kDnBlock) {
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
    const int tx = threadIdx.x & (kDnTile - 1), ty = threadIdx.x / kDnTile;
    const int px = bx0 + tx, py = by0 + ty;
    if (px >= w || py >= h) return;
    const int lc = (ty + R) * LW + tx + R;
    const float4 cp = sc[lc], np = sn[lc], pp = sp[lc];
    const bool finp = dn_is_finite<VAR>(cp), missp = __float_as_int(pp.w) < 0;
    DnCentre ce{0.0f, ks};
    if constexpr (VAR) ce = dn_centre(cp, px, py, w, h, ks, [&](int dx, int dy) { return dn_var(sc[lc + dy * LW + dx]); });
    DnSum<VAR> s{};
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = px + dx * STEP, qy = py + dy * STEP;
            if (qx < 0 || qx >= w || qy < 0 || qy >= h) continue;  // taps outside the region are skipped
            const int lq = lc + dy * STEP * LW + dx * STEP;
            dn_tap<VAR>(cp, ce, np, pp, finp, missp, sc[lq], sn[lq], sp[lq], h5(dy + 2) * h5(dx + 2), s);
        }
    }
    dst[(size_t)py * (size_t)w + (size_t)px] = dn_finish<VAR>(cp, finp, s);
}

// Larger steps: the taps are 4+ pixels apart, so a tile's halo would dwarf it; they read
// global memory (L2 / MALL). A workgroup is 4 rows of 64 pixels: a wave reads 64 consecutive
// pixels of a row per tap. The pre-blur's nine variances are the w lanes of the centre's
// neighbours, which share its cache lines.
constexpr int kDnRow = 64;
template <bool VAR>
__global__ __launch_bounds__(kDnBlock) void denoise_global_kernel(const float4* __restrict__ src, float4* __restrict__ dst,
                                                                   const float4* __restrict__ fn,
                                                                   const float4* __restrict__ gp, int w, int h, int step,
                                                                   float ks) {
    const int px = blockIdx.x * kDnRow + (int)(threadIdx.x & (kDnRow - 1));
    const int py = blockIdx.y * (kDnBlock / kDnRow) + (int)(threadIdx.x / kDnRow);
    if (px >= w || py >= h) return;
    const size_t pc = (size_t)py * (size_t)w + (size_t)px;
    const float4 cp = src[pc], np = fn[pc], pp = gp[pc];
    const bool finp = dn_is_finite<VAR>(cp), missp = __float_as_int(pp.w) < 0;
    DnCentre ce{0.0f, ks};
    if constexpr (VAR)
        ce = dn_centre(cp, px, py, w, h, ks, [&](int dx, int dy) {
            return dn_var(src[(size_t)(py + dy) * (size_t)w + (size_t)(px + dx)]);
        });
    DnSum<VAR> s{};
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = py + dy * step;
        if (qy < 0 || qy >= h) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = px + dx * step;
            if (qx < 0 || qx >= w) continue;
            const size_t q = (size_t)qy * (size_t)w + (size_t)qx;
            dn_tap<VAR>(cp, ce, np, pp, finp, missp, src[q], fn[q], gp[q], h5(dy + 2) * h5(dx + 2), s);
        }
    }
    dst[pc] = dn_finish<VAR>(cp, finp, s);
}

// ---- launches ---------------------------------------------------------------------------------
static dim3 grid1(long n) { return dim3((unsigned)std::max(1l, (n + kDnBlock - 1) / kDnBlock)); }

hipError_t launch_guides(const DevScene& S, int trav, const RtRegion& reg, const int32_t* prim_object,
                         const DenoiseGuides& g, int lds_max, hipStream_t stream) {
    const int tiles_x = std::max((reg.width + kTile - 1) / kTile, 1);
    const long tiles = (long)tiles_x * ((reg.height + kTile - 1) / kTile);
    if (tiles <= 0) return hipSuccess;
    if (tiles > 0x7fffffffl / kWave) return hipErrorInvalidValue;
    const RtRegion r{reg.x, reg.y, reg.width, reg.height, 0, 1};
    const size_t lds = stack_lds_bytes(S.cam.stack_depth, trav, S.cam.n_prims);
    if (lds > (size_t)lds_max) return hipErrorInvalidValue;
    const int waves = kBlock / kWave;
    const dim3 grid((unsigned)((tiles + waves - 1) / waves));
    if (trav == TRAV_BRUTE)
        hipLaunchKernelGGL(guide_kernel<TRAV_BRUTE>, grid, dim3(kBlock), lds, stream, S, r, tiles_x, (int)tiles,
                           prim_object, g);
    else if (trav == TRAV_FAST)
        hipLaunchKernelGGL(guide_kernel<TRAV_FAST>, grid, dim3(kBlock), lds, stream, S, r, tiles_x, (int)tiles,
                           prim_object, g);
    else
        hipLaunchKernelGGL(guide_kernel<TRAV_REFERENCE>, grid, dim3(kBlock), lds, stream, S, r, tiles_x, (int)tiles,
                           prim_object, g);
    return hipGetLastError();
}

hipError_t launch_guides_unpack(const DenoiseGuides& g, int n, float* normal, float* position, float* distance,
                                int32_t* object, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(guides_unpack_kernel, grid1(n), dim3(kDnBlock), 0, stream, g, n, normal, position, distance,
                       object);
    return hipGetLastError();
}

hipError_t launch_guides_pack(const DenoiseGuides& g, int n, const float* normal, const float* position,
                              const float* distance, const int32_t* object, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(guides_pack_kernel, grid1(n), dim3(kDnBlock), 0, stream, g, n, normal, position, distance, object);
    return hipGetLastError();
}

hipError_t launch_denoise_pack(const float* rad, int pitch_px, int x0, int y0, int w, int h, const float4* gn,
                               float sigma_plane, const float* variance, float4* colour, float4* fn,
                               hipStream_t stream) {
    if (w <= 0 || h <= 0) return hipSuccess;
    const auto kernel = variance ? denoise_pack_kernel<true> : denoise_pack_kernel<false>;
    hipLaunchKernelGGL(kernel, grid1((long)w * h), dim3(kDnBlock), 0, stream, rad, pitch_px, x0, y0, w, h, gn,
                       sigma_plane, colour, fn, variance);
    return hipGetLastError();
}

template <bool VAR>
static void launch_level(const float4* src, float4* dst, const float4* fn, const float4* gp, int w, int h, int step,
                         float ks, hipStream_t stream) {
    const dim3 tiles((unsigned)((w + kDnTile - 1) / kDnTile), (unsigned)((h + kDnTile - 1) / kDnTile));
    if (step == 1)
        hipLaunchKernelGGL((denoise_lds_kernel<VAR, 1>), tiles, dim3(kDnBlock), 0, stream, src, dst, fn, gp, w, h, ks);
    else if (step == 2)
        hipLaunchKernelGGL((denoise_lds_kernel<VAR, 2>), tiles, dim3(kDnBlock), 0, stream, src, dst, fn, gp, w, h, ks);
    else
        hipLaunchKernelGGL(denoise_global_kernel<VAR>,
                           dim3((unsigned)((w + kDnRow - 1) / kDnRow),
                                (unsigned)((h + kDnBlock / kDnRow - 1) / (kDnBlock / kDnRow))),
                           dim3(kDnBlock), 0, stream, src, dst, fn, gp, w, h, step, ks);
}

hipError_t launch_denoise_level(bool var, const float4* src, float4* dst, const float4* fn, const float4* gp, int w,
                                int h, int step, float ks, hipStream_t stream) {
    if (w <= 0 || h <= 0) return hipSuccess;
    if (var)
        launch_level<true>(src, dst, fn, gp, w, h, step, ks, stream);
    else
        launch_level<false>(src, dst, fn, gp, w, h, step, ks, stream);
    return hipGetLastError();
}

hipError_t launch_denoise_unpack(const float4* colour, int n, float* rad, uint8_t* rgb, float* variance,
                                 hipStream_t stream, const DenoiseHold& hold) {
    if (n <= 0) return hipSuccess;
    if (hold.mask && (hold.w <= 0 || !hold.rad)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(denoise_unpack_kernel, grid1(n), dim3(kDnBlock), 0, stream, colour, n, rad, rgb, variance, hold);
    return hipGetLastError();
}

}  // namespace rt
