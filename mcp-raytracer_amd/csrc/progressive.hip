// Progressive rendering passes (progressive.hpp). Compiled with -ffp-contract=off: the fp32
// colour sum and the fp64 illuminance arithmetic round as the reference's PixelStats.add and
// pixelConverged do (src/render-utils/renderStats.ts:76-88, src/camera.ts:348-368).
#include "progressive.hpp"

#include <algorithm>

#include "pt_pixel.hpp"

namespace rt {

constexpr int kProgBlock = 256;
constexpr int kSettleUnroll = 4;

// One record pass of a step: every pixel of the pass adds the step's samples to its running
// PixelStats in sample order and checks convergence after each one, as pt_adapt_kernel does
// for a round - except after the step's last sample, whose check is made when the pixel's next
// step begins (it is a function of the state alone). So after a step every pixel has either
// finished (converged inside the step, or reached the camera's samples) or holds exactly
// samples_done samples, which is what a camera with `samples: samples_done` would hold; the
// samples the step rendered past a convergence are dropped. Only the state is written: the
// frame, RenderStats and the next active list come from pt_resolve_kernel.
__global__ __launch_bounds__(kProgBlock) void pt_settle_kernel(DevScene S0, RtRegion reg, RenderOut out, int tiles_x,
                                                                SampleBuf sb, ProgPass pp) {
    const RtCamera& C = S0.cam;
    const int lane = threadIdx.x & (kWave - 1);
    const double rtx = 1.0 / (double)tiles_x;
    const int endX = min(reg.x + reg.width, C.width), endY = min(reg.y + reg.height, C.height);
    // fmod(n, aBatch) == 0 is n % aBatch == 0 for an integral aBatch (pt_adapt_kernel)
    const double abd = C.a_batch;
    const bool ib = abd >= 1.0 && abd < 2147483648.0 && abd == ::floor(abd);
    const int batch = ib ? (int)abd : 1;
    unsigned long long st_err = 0;  // error flags of the samples kept (SampleBuf::err_in_rec)
    for (int a = blockIdx.x * blockDim.x + threadIdx.x; a < sb.slots; a += gridDim.x * blockDim.x) {
        int i = 0, j = 0;
        if (!slot_pixel(sb, reg, tiles_x, rtx, endX, endY, a, i, j)) continue;
        const int ls = sb.act[a];  // (a step always renders through the active list: unfinished pixels only)
        const ProgPix q = pp.state[ls];
        V3 color = v3(q.c.x, q.c.y, q.c.z);
        int n = __float_as_int(q.c.w);
        double sIll = q.ill.x, sIll2 = q.ill.y;
        unsigned long long bsum = (unsigned long long)(uint32_t)q.b.x | ((unsigned long long)(uint32_t)q.b.w << 32);
        int bmin = n > 0 ? q.b.y : 0x7fffffff, bmax = n > 0 ? q.b.z : 0;
        // the check after the previous step's last sample
        bool done = n > 0 && pixel_converged(C, n, sIll, sIll2);
        int until = ib ? batch - n % batch : 0;  // samples to add until n is the next multiple
        const float4* rec = sb.rec + (size_t)a * sb.stride_slot;
        const size_t stride = (size_t)sb.stride_s;
        // kSettleUnroll record loads in flight (sample-major records: coalesced across the wave)
        for (int k = 0; k < pp.len && !done; k += kSettleUnroll) {
            float4 r[kSettleUnroll];
#pragma unroll
            for (int m = 0; m < kSettleUnroll; ++m)
                r[m] = k + m < pp.len ? rec[(size_t)(k + m) * stride] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int m = 0; m < kSettleUnroll; ++m) {
                if (k + m < pp.len && !done) {
                    // PixelStats.add (renderStats.ts:76-88), then the while condition
                    const V3 c = v3(r[m].x, r[m].y, r[m].z);
                    color = add(color, c);
                    ++n;
                    const uint32_t bw = __float_as_uint(r[m].w);
                    const int b = (int)(bw & kRecBounceMask);
                    st_err |= (unsigned long long)(bw >> kRecErrShift);
                    bsum += (unsigned long long)b;
                    bmin = min(bmin, b);
                    bmax = max(bmax, b);
                    const double il = illuminance(c);
                    sIll += il;
                    sIll2 += il * il;
                    const bool last = k + m == pp.len - 1;
                    if (ib) {
                        const bool check = --until == 0;
                        if (check) until = batch;
                        done = n >= C.n_samples || (!last && check && pixel_converged_at_batch(C, n, sIll, sIll2));
                    } else {
                        done = n >= C.n_samples || (!last && pixel_converged(C, n, sIll, sIll2));
                    }
                }
            }
        }
        ProgPix w;
        w.c = make_float4(color.x, color.y, color.z, __uint_as_float((uint32_t)n | (done ? kProgFinished : 0u)));
        w.ill = make_double2(sIll, sIll2);
        w.b = make_int4((int)(uint32_t)bsum, bmin, bmax, (int)(uint32_t)(bsum >> 32));
        pp.state[ls] = w;
    }
    const unsigned long long err = wave_or(st_err);
    if (lane == 0 && err) atomicOr(&out.stats[ST_ERROR * kStatStride], err);
}

// State -> outputs. Every pixel of the region gets finalColor / writeColorToBuffer of its
// PixelStats (finish_pixel: a finished pixel exactly as a one-shot render writes it, an
// unfinished one its preview) and is counted by RenderStats.addPixel with the samples and
// bounces it has so far; the unfinished ones are compacted into the next step's active list
// (__ballot + mbcnt, one atomic per block and iteration; the order is irrelevant: a pixel's
// result depends on its own samples only). Runs after a step's settle passes, and on its own
// when a session begins or is restored from a checkpoint.
__global__ __launch_bounds__(kProgBlock) void pt_resolve_kernel(DevScene S0, RtRegion reg, RenderOut out, int tiles_x,
                                                                 ProgResolve pr) {
    const RtCamera& C = S0.cam;
    const int lane = threadIdx.x & (kWave - 1);
    const int w = threadIdx.x / kWave;
    const double rtx = 1.0 / (double)tiles_x;
    const int endX = min(reg.x + reg.width, C.width), endY = min(reg.y + reg.height, C.height);
    PixStats st;
    __shared__ unsigned int wcnt[kProgBlock / kWave];
    __shared__ unsigned int wbase;
    const int stride = gridDim.x * blockDim.x;
    const int n_iter = (pr.slots + stride - 1) / stride;  // block-uniform trip count (the append syncs)
    for (int it = 0; it < n_iter; ++it) {
        const int ls = it * stride + blockIdx.x * blockDim.x + threadIdx.x;
        bool carry = false;
        if (ls < pr.slots) {
            int i, j;
            item_pixel(reg, tiles_x, rtx, ls >> 6, ls & 63, i, j);
            if (i < endX && j < endY) {
                const ProgPix q = pr.state[ls];
                const uint32_t nw = __float_as_uint(q.c.w);
                const int n = (int)(nw & ~kProgFinished);
                const unsigned long long bsum =
                    (unsigned long long)(uint32_t)q.b.x | ((unsigned long long)(uint32_t)q.b.w << 32);
                finish_pixel(C, out, (uint32_t)j * (uint32_t)C.width + (uint32_t)i, v3(q.c.x, q.c.y, q.c.z), n, bsum,
                             q.b.y, q.b.z, st);
                carry = !(nw & kProgFinished);
            }
        }
        const unsigned long long m = __ballot(carry);
        if (lane == 0) wcnt[w] = (unsigned int)__popcll(m);
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned int tot = 0;
            for (int q = 0; q < kProgBlock / kWave; ++q) {
                const unsigned int c = wcnt[q];
                wcnt[q] = tot;
                tot += c;
            }
            wbase = tot ? atomicAdd(pr.count, tot) : 0u;
        }
        __syncthreads();
        if (carry) {
            const int r = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            pr.act[wbase + wcnt[w] + (unsigned int)r] = ls;
        }
        __syncthreads();
    }
    // RenderStats.merge: waves -> LDS -> one lane per block
    __shared__ unsigned long long red[kProgBlock / kWave][7];
    const unsigned long long v[7] = {wave_sum(st.pixels), wave_sum(st.samples), wave_min(st.smin), wave_max(st.smax),
                                     wave_sum(st.b),      wave_min(st.bmin),    wave_max(st.bmax)};
    if (lane == 0)
        for (int q = 0; q < 7; ++q) red[w][q] = v[q];
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t[7];
        for (int q = 0; q < 7; ++q) t[q] = red[0][q];
        for (int u = 1; u < kProgBlock / kWave; ++u) {
            t[0] += red[u][0];
            t[1] += red[u][1];
            t[2] = min(t[2], red[u][2]);
            t[3] = max(t[3], red[u][3]);
            t[4] += red[u][4];
            t[5] = min(t[5], red[u][5]);
            t[6] = max(t[6], red[u][6]);
        }
        stats_atomics(out, t[0], t[1], t[2], t[3], t[4], t[5], t[6], 0ull);
    }
}

// State -> the variance map (prog_variance of every pixel of the region).
__global__ __launch_bounds__(kProgBlock) void prog_variance_kernel(const ProgPix* __restrict__ state, int slots,
                                                                    RtRegion reg, int tiles_x,
                                                                    float* __restrict__ variance) {
    const int slot = blockIdx.x * kProgBlock + (int)threadIdx.x;
    if (slot >= slots) return;
    int i, j;
    item_pixel(reg, tiles_x, slot / kWave, slot & (kWave - 1), i, j);
    if (i >= reg.x + reg.width || j >= reg.y + reg.height) return;
    const uint32_t n = __float_as_uint(state[slot].c.w) & ~kProgFinished;
    const double2 ill = state[slot].ill;
    variance[(size_t)(j - reg.y) * (size_t)reg.width + (size_t)(i - reg.x)] = prog_variance(ill.x, ill.y, n);
}

hipError_t launch_prog_variance(const ProgPix* state, int slots, const RtRegion& reg, int tiles_x, float* variance,
                                hipStream_t stream) {
    if (slots <= 0) return hipSuccess;
    const RtRegion r{reg.x, reg.y, reg.width, reg.height, 0, 1};
    hipLaunchKernelGGL(prog_variance_kernel, dim3((unsigned)((slots + kProgBlock - 1) / kProgBlock)), dim3(kProgBlock), 0,
                       stream, state, slots, r, tiles_x, variance);
    return hipGetLastError();
}

hipError_t launch_settle(const DevScene& S, const RtRegion& reg, const RenderOut& out, int tiles_x,
                         const SampleBuf& sb, const ProgPass& pp, hipStream_t stream) {
    const int grid = std::max(1, std::min((sb.slots + kProgBlock - 1) / kProgBlock, 1024));
    hipLaunchKernelGGL(pt_settle_kernel, dim3(grid), dim3(kProgBlock), 0, stream, S, reg, out, tiles_x, sb, pp);
    return hipGetLastError();
}

hipError_t launch_resolve(const DevScene& S, const RtRegion& reg, const RenderOut& out, int tiles_x,
                          const ProgResolve& pr, hipStream_t stream) {
    const int grid = std::max(1, std::min((pr.slots + kProgBlock - 1) / kProgBlock, 1024));
    hipLaunchKernelGGL(pt_resolve_kernel, dim3(grid), dim3(kProgBlock), 0, stream, S, reg, out, tiles_x, pr);
    return hipGetLastError();
}

}  // namespace rt
