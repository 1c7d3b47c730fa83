// The sub-pixel coverage pass (coverage.hpp). Compiled with denoise.hip's flags (-ffp-contract=off,
// no fast-math): the sub-ray directions are fp32 vector arithmetic with one result per operation -
// tests/coverage_ref.py is the definition.
#include "coverage.hpp"

#include <algorithm>

#include "pt_pixel.hpp"  // item_pixel
#include "pt_shade.hpp"  // pixel_center, closest_hit_any

namespace rt {

// guide_kernel's shape (denoise.hip): one thread per pixel, a wave per 8x8 tile of the region
// (item_pixel numbering), the traversal stack (or the brute force's candidate bounds) in LDS, the
// scene read from global memory. The K^2 sub-rays run in one rolled loop, so every lane of a wave
// walks the same sub-offset at the same time and the wave's rays stay as coherent as the guide
// pass's; the objects seen so far stay in registers (ob[], written through a select chain: the loop
// counter never indexes it).
template <int TRAV, int K>
__global__ __launch_bounds__(kBlock) void coverage_kernel(DevScene S, RtRegion reg, int tiles_x, int n_tiles,
                                                          const int32_t* prim_object, uint32_t* coverage,
                                                          uint8_t* hold) {
    extern __shared__ int lds_stack[];
    constexpr int N = K * K;
    const int tile = blockIdx.x * (kBlock / kWave) + (int)(threadIdx.x / kWave);
    if (tile >= n_tiles) return;
    int i, j;
    item_pixel(reg, tiles_x, tile, (int)(threadIdx.x & (kWave - 1)), i, j);
    if (i >= reg.x + reg.width || j >= reg.y + reg.height) return;
    const RtCamera& C = S.cam;
    const V3 o = ld3(C.center), du = ld3(C.du), dv = ld3(C.dv);
    const V3 pc = pixel_center<double>(C, i, j);
    int* stk = lds_stack + threadIdx.x;
    auto object_of = [&](V3 through) {
        const RayK<double> r = make_ray<double>(o, sub(through, o));
        double t = 0;
        const int h = closest_hit_any<double, false, TRAV>(S, C.n_prims, r, t, stk, nullptr);
        return h >= 0 ? prim_object[h] : -1;
    };
    const int oc = object_of(pc);  // launch_guides' ray
    int ob[N];
#pragma unroll
    for (int q = 0; q < N; ++q) ob[q] = 0;
    uint32_t agree = 0u, distinct = 1u;
#pragma unroll 1
    for (int s = 0; s < N; ++s) {
        const float ox = ((float)(s % K) + 0.5f) * (1.0f / K) - 0.5f;  // exact: K is a power of two
        const float oy = ((float)(s / K) + 0.5f) * (1.0f / K) - 0.5f;
        const int ow = object_of(add(add(pc, scale<float>(du, ox)), scale<float>(dv, oy)));
        bool seen = ow == oc;
        agree |= (seen ? 1u : 0u) << s;
#pragma unroll
        for (int q = 0; q < N; ++q) {
            seen = seen || (q < s && ob[q] == ow);
            ob[q] = q == s ? ow : ob[q];
        }
        distinct += seen ? 0u : 1u;
    }
    const size_t k = (size_t)(j - reg.y) * (size_t)reg.width + (size_t)(i - reg.x);
    if (coverage) coverage[k] = agree | (distinct > 255u ? 255u : distinct) << 16;
    if (hold) hold[k] = agree != (1u << N) - 1u ? 1 : 0;
}

template <int TRAV>
static void launch_k(int k, dim3 grid, size_t lds, hipStream_t stream, const DevScene& S, const RtRegion& r, int tiles_x,
                     int tiles, const int32_t* prim_object, uint32_t* coverage, uint8_t* hold) {
    if (k == 2)
        hipLaunchKernelGGL((coverage_kernel<TRAV, 2>), grid, dim3(kBlock), lds, stream, S, r, tiles_x, tiles, prim_object,
                           coverage, hold);
    else
        hipLaunchKernelGGL((coverage_kernel<TRAV, 4>), grid, dim3(kBlock), lds, stream, S, r, tiles_x, tiles, prim_object,
                           coverage, hold);
}

hipError_t launch_coverage(const DevScene& S, int trav, const RtRegion& reg, const int32_t* prim_object, int k,
                           uint32_t* coverage, uint8_t* hold, int lds_max, hipStream_t stream) {
    if (k != 2 && k != 4) return hipErrorInvalidValue;
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
        launch_k<TRAV_BRUTE>(k, grid, lds, stream, S, r, tiles_x, (int)tiles, prim_object, coverage, hold);
    else if (trav == TRAV_FAST)
        launch_k<TRAV_FAST>(k, grid, lds, stream, S, r, tiles_x, (int)tiles, prim_object, coverage, hold);
    else
        launch_k<TRAV_REFERENCE>(k, grid, lds, stream, S, r, tiles_x, (int)tiles, prim_object, coverage, hold);
    return hipGetLastError();
}

}  // namespace rt
