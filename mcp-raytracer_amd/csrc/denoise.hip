// Guide pass and a-trous filter (denoise.hpp). Compiled with -ffp-contract=off and without any
// fast-math, denormal-flushing or approximate-reciprocal flag: every fp32 operation of the
// filter (add, multiply, IEEE divide, max, repeated squaring) and of the guide distance
// (correctly rounded sqrtf) has exactly one result, and the tap order and the
// multiply-then-add accumulation are part of it - tests/denoise_ref.py is the definition.
#include "denoise.hpp"

#include <algorithm>

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
__device__ __forceinline__ bool finite_f(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

__global__ __launch_bounds__(kDnBlock) void denoise_pack_kernel(const float* rad, int pitch_px, int x0, int y0, int w,
                                                                 int h, const float4* gn, float sigma_plane,
                                                                 float4* colour, float4* fn) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= w * h) return;
    const int y = k / w, x = k - y * w;
    const float* s = rad + 3 * ((size_t)(y0 + y) * (size_t)pitch_px + (size_t)(x0 + x));
    const float r = s[0], g = s[1], b = s[2];
    colour[k] = make_float4(r, g, b, finite_f(r) && finite_f(g) && finite_f(b) ? 1.0f : 0.0f);
    const float4 a = gn[k];
    fn[k] = make_float4(a.x, a.y, a.z, 1.0f / (sigma_plane * a.w));
}

__global__ __launch_bounds__(kDnBlock) void denoise_unpack_kernel(const float4* colour, int n, float* rad, uint8_t* rgb) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const float4 c = colour[k];
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

// The B3 spline's taps (exact in fp32, and so are their products).
__device__ __forceinline__ float h5(int k) {
    return k == 2 ? 0.375f : (k == 1 || k == 3) ? 0.25f : 0.0625f;
}

struct DnSum {
    float r, g, b, w;
};

// One tap of pixel p (colour cp, guides np / pp, finite flag finp, miss flag missp) at pixel q,
// in the definition's operation order.
__device__ __forceinline__ void dn_tap(const float4& cp, const float4& np, const float4& pp, bool finp, bool missp,
                                       const float4& cq, const float4& nq, const float4& pq, float hk, float k_c,
                                       DnSum& s) {
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
    const float dcx = cq.x - cp.x, dcy = cq.y - cp.y, dcz = cq.z - cp.z;
    const float y = (dcx * dcx + dcy * dcy) + dcz * dcz;
    const float cw = 1.0f + y * k_c;
    const bool missq = __float_as_int(pq.w) < 0;
    // two misses: the colour weight only; a hit and a miss never mix. One IEEE division.
    const bool both = missp && missq;
    const float num = both ? hk : hk * dn;
    const float den = both ? cw : (1.0f + x * x) * cw;
    const float wq = num / den;
    const bool ok = finp && cq.w != 0.0f;  // non-finite taps are skipped
    const float wt = ok && missp == missq ? wq : 0.0f;
    s.r = s.r + wt * (ok ? cq.x : 0.0f);
    s.g = s.g + wt * (ok ? cq.y : 0.0f);
    s.b = s.b + wt * (ok ? cq.z : 0.0f);
    s.w = s.w + wt;
}

__device__ __forceinline__ float4 dn_finish(const float4& cp, bool finp, const DnSum& s) {
    float4 o = cp;
    if (finp) {  // (a non-finite centre is copied through)
        o.x = s.r / s.w;
        o.y = s.g / s.w;
        o.z = s.b / s.w;
    }
    o.w = finite_f(o.x) && finite_f(o.y) && finite_f(o.z) ? 1.0f : 0.0f;
    return o;
}

// Steps 1 and 2: a 16x16 tile and its 2 * STEP halo staged in LDS as three float4 planes
// (20x20 at step 1, 24x24 at step 2: 19 and 27 KB), so each input is fetched once per tile
// instead of up to 25 times. Cells outside the region are never read (their taps are skipped).
constexpr int kDnTile = 16;
template <int STEP>
__global__ __launch_bounds__(kDnBlock) void denoise_lds_kernel(const float4* __restrict__ src, float4* __restrict__ dst,
                                                                const float4* __restrict__ fn,
                                                                const float4* __restrict__ gp, int w, int h, float k_c) {
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
    const bool finp = cp.w != 0.0f, missp = __float_as_int(pp.w) < 0;
    DnSum s{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = px + dx * STEP, qy = py + dy * STEP;
            if (qx < 0 || qx >= w || qy < 0 || qy >= h) continue;  // taps outside the region are skipped
            const int lq = lc + dy * STEP * LW + dx * STEP;
            dn_tap(cp, np, pp, finp, missp, sc[lq], sn[lq], sp[lq], h5(dy + 2) * h5(dx + 2), k_c, s);
        }
    }
    dst[(size_t)py * (size_t)w + (size_t)px] = dn_finish(cp, finp, s);
}

// Larger steps: the taps are 4+ pixels apart, so a tile's halo would dwarf it; they read
// global memory (L2 / MALL). A workgroup is 4 rows of 64 pixels: a wave reads 64 consecutive
// pixels of a row per tap.
constexpr int kDnRow = 64;
__global__ __launch_bounds__(kDnBlock) void denoise_global_kernel(const float4* __restrict__ src, float4* __restrict__ dst,
                                                                   const float4* __restrict__ fn,
                                                                   const float4* __restrict__ gp, int w, int h, int step,
                                                                   float k_c) {
    const int px = blockIdx.x * kDnRow + (int)(threadIdx.x & (kDnRow - 1));
    const int py = blockIdx.y * (kDnBlock / kDnRow) + (int)(threadIdx.x / kDnRow);
    if (px >= w || py >= h) return;
    const size_t pc = (size_t)py * (size_t)w + (size_t)px;
    const float4 cp = src[pc], np = fn[pc], pp = gp[pc];
    const bool finp = cp.w != 0.0f, missp = __float_as_int(pp.w) < 0;
    DnSum s{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = py + dy * step;
        if (qy < 0 || qy >= h) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = px + dx * step;
            if (qx < 0 || qx >= w) continue;
            const size_t q = (size_t)qy * (size_t)w + (size_t)qx;
            dn_tap(cp, np, pp, finp, missp, src[q], fn[q], gp[q], h5(dy + 2) * h5(dx + 2), k_c, s);
        }
    }
    dst[pc] = dn_finish(cp, finp, s);
}

// ---- launches ---------------------------------------------------------------------------------
static dim3 grid1(int n) { return dim3((unsigned)std::max(1, (n + kDnBlock - 1) / kDnBlock)); }

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
                               float sigma_plane, float4* colour, float4* fn, hipStream_t stream) {
    if (w <= 0 || h <= 0) return hipSuccess;
    hipLaunchKernelGGL(denoise_pack_kernel, grid1(w * h), dim3(kDnBlock), 0, stream, rad, pitch_px, x0, y0, w, h, gn,
                       sigma_plane, colour, fn);
    return hipGetLastError();
}

hipError_t launch_denoise_level(const float4* src, float4* dst, const float4* fn, const float4* gp, int w, int h,
                                int step, float k_c, hipStream_t stream) {
    if (w <= 0 || h <= 0) return hipSuccess;
    const dim3 tiles((unsigned)((w + kDnTile - 1) / kDnTile), (unsigned)((h + kDnTile - 1) / kDnTile));
    if (step == 1)
        hipLaunchKernelGGL(denoise_lds_kernel<1>, tiles, dim3(kDnBlock), 0, stream, src, dst, fn, gp, w, h, k_c);
    else if (step == 2)
        hipLaunchKernelGGL(denoise_lds_kernel<2>, tiles, dim3(kDnBlock), 0, stream, src, dst, fn, gp, w, h, k_c);
    else
        hipLaunchKernelGGL(denoise_global_kernel,
                           dim3((unsigned)((w + kDnRow - 1) / kDnRow),
                                (unsigned)((h + kDnBlock / kDnRow - 1) / (kDnBlock / kDnRow))),
                           dim3(kDnBlock), 0, stream, src, dst, fn, gp, w, h, step, k_c);
    return hipGetLastError();
}

hipError_t launch_denoise_unpack(const float4* colour, int n, float* rad, uint8_t* rgb, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(denoise_unpack_kernel, grid1(n), dim3(kDnBlock), 0, stream, colour, n, rad, rgb);
    return hipGetLastError();
}

}  // namespace rt
