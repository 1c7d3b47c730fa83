// The path-tracing hot path as one persistent HIP kernel for gfx950.
//
// Restates, per lane, Camera.renderRegion's pixel loop (src/camera.ts:388-431)
// with getRay (176-210), the rayColor recursion turned into a bounce loop
// (221-319), BVH traversal (src/geometry/bvh.ts:128-146, aabb.ts:30-55,
// hittableList.ts:71-87), sphere/quad/plane intersection (src/entities/*),
// material scatter (src/materials/*), the mixture-PDF light sampling
// (src/geometry/pdf.ts) and the spp accumulate (src/render-utils/renderStats.ts:76-88).
//
// Work decomposition (MI355X): a wave owns an 8x8 pixel tile, one pixel per
// lane; waves pull tiles from a global atomic counter (persistent grid, load
// balanced across the 256 CUs / 8 XCDs). Each lane renders its pixel's samples
// in order - the reference accumulates samples sequentially in fp32, so the
// per-pixel order is part of the result - but lanes are NOT synchronised per
// sample: a lane whose path terminates immediately starts its next sample in
// the same loop trip (path regeneration), so the wave runs for
// max_lane(sum of path lengths), not sum_samples(max_lane(path length)).
// The BVH traversal stack lives in LDS, lane-interleaved ([depth][lane]) so
// every push/pop is a conflict-free ds_write/ds_read_b32.
//
// Numerics: `Real` = double restates the reference exactly (fp64 scalars,
// fp32 vector stores; built with -ffp-contract=off); Real = float is the fp32
// fast mode. See rt_math.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include "pt_pixel.hpp"
#include "pt_shade.hpp"

namespace rt {

// The scene as the kernel sees it after scene_prologue: LDS-resident arrays at their
// LDS addresses (the prologue's copy of the blob prefix), the rest global.
template <int LDSS>
__device__ __forceinline__ DevScene scene_view(const DevScene& S0, int* lds_stack) {
    DevScene S = S0;
    // near / far rows (t4_step) where the tree is in LDS: spheres-500 +5.3 %, rain +2.8 %; in the
    // LDSS 0 kernels the three row offsets per ray pushed the chunk kernel from 48 to 88 bytes of
    // scratch spills and spheres-100k lost 2.3 % (profiles/r04/nearfar/). A constant per level, so
    // the unused form folds away.
    S.nearfar = LDSS > 0 ? 1 : 0;
    if (LDSS > 0) {
        S.tsph2 = nullptr;  // (fp64 leaf records: trees walked from global memory only)
    }
    if (LDSS == 0) S.top_lds = reinterpret_cast<const char*>(lds_stack) + S0.lds_stack_bytes;
    if (LDSS > 0) {
        S.n_top = 0;  // the whole tree is in LDS (a constant: the walk's reads stay ds_read)
        const char* b = reinterpret_cast<const char*>(lds_stack) + S0.lds_stack_bytes;
        S.t4nodes = reinterpret_cast<const RtT4Node*>(b);
        S.t4_stride = S0.lds_node_pad > 0 ? (int)sizeof(RtT4Node) + 16 : (int)sizeof(RtT4Node);
        b += (size_t)S0.lds_node_pad * 16;  // every section after the nodes moves by the pad rows
        S.tprims = reinterpret_cast<const int32_t*>(b + S0.off_tprims);
        S.tsph = reinterpret_cast<const float4*>(b + S0.off_tsph);
        S.prims = reinterpret_cast<const RtPrim*>(b + S0.off_prims);
        S.xrec = reinterpret_cast<const RtExact*>(b + S0.off_xrec);
        if (LDSS == 2) {
            S.mats = reinterpret_cast<const RtMat*>(b + S0.off_mats);
            S.lights = reinterpret_cast<const RtLight*>(b + S0.off_lights);
            S.onbs = reinterpret_cast<const RtOnb*>(b + S0.off_onbs);
        }
    }
    return S;
}

// Workgroup prologue shared by the render kernels: LDS-resident scene data
// (one cooperative copy per workgroup) and this thread's stack columns.
// LDSS 0: all scene reads from global memory; 1: the traversal data and the
// primitive records in LDS; 2: also the material and light tables. (Wave-uniform
// reads - the brute-force primitive loop, the light list - stay on scalar loads
// from the global copy.)
template <int LDSS>
__device__ __forceinline__ DevScene scene_prologue(const DevScene& S0, int* lds_stack) {
    if (LDSS == 0 && S0.n_top > 0) {  // the tree's top: n_top nodes of 8 rows, a pad row each
        uint4* dst = reinterpret_cast<uint4*>(reinterpret_cast<char*>(lds_stack) + S0.lds_stack_bytes);
        for (int w = threadIdx.x; w < S0.n_top * 8; w += blockDim.x) dst[w + (w >> 3)] = S0.blob[w];
        __syncthreads();
    }
    if (LDSS > 0) {
        uint4* dst = reinterpret_cast<uint4*>(reinterpret_cast<char*>(lds_stack) + S0.lds_stack_bytes);
        // the 4-wide nodes (8 rows each) take a pad row each (t4_node); the rest moves by those rows
        const int node_rows = S0.lds_node_pad * 8;
        for (int w = threadIdx.x; w < S0.lds_words; w += blockDim.x)
            dst[w < node_rows ? w + (w >> 3) : w + S0.lds_node_pad] = S0.blob[w];
        __syncthreads();
    }
    return scene_view<LDSS>(S0, lds_stack);
}

// ---------------------------------------------------------------------------
// Sequential-pixel kernel (adaptive sampling, and the reference-order
// traversal): a wave owns an 8x8 tile, lane = pixel, samples in order with
// per-pixel convergence checks (pixelConverged, src/camera.ts:348-368).
// Kernel arguments: S0 must stay the first parameter (cam_opaque reads it at kernarg offset 0).
// INSTR: 0 = product build, 1 = work counters, 2 = section timing.
// ---------------------------------------------------------------------------
template <class Real, bool EMIT, int INSTR, int TRAV, int LDSS>
__global__ __launch_bounds__(kBlock) void pt_render_kernel(DevScene S0, RtRegion reg, RenderOut out,
                                                                         int tiles_x, int my_tiles) {
    constexpr bool COUNT = INSTR == 1;
    constexpr bool PROF = INSTR == 2;
    extern __shared__ int lds_stack[];
    const RtCamera& C = S0.cam;
    const DevScene S = scene_prologue<LDSS>(S0, lds_stack);
    const int lane = threadIdx.x & (kWave - 1);
    StackT<LDSS>* stk = reinterpret_cast<StackT<LDSS>*>(lds_stack) + threadIdx.x;

    const int endX = min(reg.x + reg.width, C.width);
    const int endY = min(reg.y + reg.height, C.height);

    uint32_t cnt[CT_WORDS];
    if (COUNT) {
#pragma unroll
        for (int k = 0; k < CT_WORDS; ++k) cnt[k] = 0;
    }
    PixStats st;
    unsigned long long st_err = 0;
    __shared__ unsigned long long prof_lds[PROF ? kProfWaves * kProfSlot : 1];
    Prof pf;
    prof_init<PROF>(pf, prof_lds, lane);

    while (true) {
        unsigned int tile = 0;
        if (lane == 0) tile = atomicAdd(out.tile_counter, 1u);
        tile = __shfl(tile, 0, 64);
        if ((int)tile >= my_tiles) break;
        const int gt = reg.tile_group + (int)tile * reg.tile_groups;
        const int i = reg.x + (gt % tiles_x) * kTile + (lane & (kTile - 1));
        const int j = reg.y + (gt / tiles_x) * kTile + (lane / kTile);
        bool active = i < endX && j < endY && C.n_samples > 0;
        const bool valid_px = i < endX && j < endY;
        const uint32_t pix = (uint32_t)j * (uint32_t)C.width + (uint32_t)i;

        // PixelStats (src/render-utils/renderStats.ts:66-88)
        V3 color = v3(0, 0, 0);
        int n = 0;
        unsigned long long bsum = 0;
        int bmin = 0x7fffffff, bmax = 0;
        double sIll = 0.0, sIll2 = 0.0;

        bool new_path = true;
        Path<EMIT> P;
        psec<PROF>(pf, PR_TILE);
        while (active) {
            const RtCamera& C = cam_opaque();
            prof_trip<PROF>(pf);
            if (new_path) {
                path_begin<Real, EMIT>(C, P, pixel_center<Real>(C, i, j), pix, (uint32_t)n);
                new_path = false;
                psec<PROF>(pf, PR_NEWPATH);
            }
            V3 c;
            if (path_trip<Real, EMIT, COUNT, PROF, TRAV>(S, C, P, stk, cnt, st_err, pf, c)) {
                // PixelStats.add (renderStats.ts:76-88)
                color = add(color, c);
                ++n;
                bsum += (unsigned long long)P.bounces;
                bmin = min(bmin, P.bounces);
                bmax = max(bmax, P.bounces);
                if (C.adaptive) {
                    const double il = illuminance(c);
                    sIll += il;
                    sIll2 += il * il;
                }
                if (COUNT) {
                    cnt[CT_SAMPLES]++;
                    cnt[CT_BOUNCES] += (uint32_t)P.bounces;
                }
                if (n >= C.n_samples || pixel_converged(C, n, sIll, sIll2)) active = false;
                else new_path = true;
                psec<PROF>(pf, PR_ACC);
            }
        }
        if (valid_px) finish_pixel(C, out, out.packed ? tile * kWave + (uint32_t)lane : pix, color, n, bsum, bmin, bmax, st);
    }
    publish_stats(out, st, st_err, lane);
    publish_counters<COUNT, PROF>(out, cnt, pf, lane);
}

// ---------------------------------------------------------------------------
// Chunked kernel (fixed spp, no adaptive sampling): the work items are
// (pixel, chunk of kChunk consecutive samples). Every lane pulls its own items
// from its wave's pool, which refills 64 items (one tile-chunk) at a time from
// a global counter - so no lane idles while its wave finishes a tile, and the
// tail of the launch is one chunk long. Each finished sample's radiance (and
// bounce count) goes to the sample buffer; pt_accum_kernel then adds every
// pixel's samples in sample order in fp32, which is exactly PixelStats.add's
// sequence, so the image is bit-identical to the sequential kernel's.
// ---------------------------------------------------------------------------
// The guided schedule's phase rows, copied to LDS at kernel start: an item's
// phase is per lane, and indexing the kernel-argument arrays by it costs a
// select chain per field (and SGPRs the path code then spills).
struct PhaseRow {
    int32_t s0, chunk, nch, base;
    double rnch;
    int32_t pad[2];
};
__device__ __forceinline__ void phase_table_init(const SampleBuf& sb, PhaseRow* tab) {
    const int t = threadIdx.x;
    if (t < kMaxPhases) {
        PhaseRow r;
        r.s0 = sb.s0[t];
        r.chunk = sb.chunk[t];
        r.nch = sb.nch[t];
        r.base = t < sb.n_phases ? sb.item_base[t] : 0x7fffffff;
        r.rnch = sb.rnch[t];
        r.pad[0] = r.pad[1] = 0;
        tab[t] = r;
    }
    __syncthreads();
}
// Item u of the launch -> (tile among this pass's tiles, lane-pixel l, sample range [s, s_end)).
__device__ __forceinline__ void item_decode(const SampleBuf& sb, const PhaseRow* tab, int u, int& tl, int& l, int& s,
                                            int& s_end) {
    int ph = 0;
    for (int q = 1; q < sb.n_phases; ++q) ph += u >= tab[q].base ? 1 : 0;
    const PhaseRow r = tab[ph];
    const int v = u - r.base;  // item within the phase: (tile, chunk) groups of 64
    const int q = v >> 6;
    l = v & 63;
    tl = udiv(q, r.nch, r.rnch);
    const int ch = q - tl * r.nch;
    s = r.s0 + ch * r.chunk;
    s_end = s + r.chunk;
}

// Item hand-out: every wave's first pool is static (wave w takes items
// [w * pool, (w + 1) * pool)), the global counter deals the rest from
// grid_waves * pool on - so the launch does not open with every wave's atomic
// on one word (4096 returning atomics serialise for ~50 us).
__device__ __forceinline__ void first_pool(const SampleBuf& sb, int& pool_next, int& pool_end, bool& exhausted) {
    const int gw = (int)(blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave);
    pool_next = gw * sb.pool;
    pool_end = min(pool_next + sb.pool, sb.n_items);
    exhausted = pool_next >= sb.n_items;
}
// A wave's next item range [pool_next, pool_end) from the global counter (wave-uniform;
// exhausted when none is left). (A second counter dealing the launch's last items in
// smaller takes measured within noise of this, profiles/r03/tail/.)
__device__ __forceinline__ void take_pool(const RenderOut& out, const SampleBuf& sb, int lane, int& pool_next,
                                          int& pool_end, bool& exhausted) {
    int base = 0;
    if (lane == 0) base = (int)atomicAdd(out.tile_counter, (unsigned)sb.pool);
    base = __builtin_amdgcn_readfirstlane(__shfl(base, 0, 64)) + (int)(gridDim.x * (blockDim.x / kWave)) * sb.pool;
    if (base >= sb.n_items) {
        exhausted = true;
        return;
    }
    pool_next = base;
    pool_end = min(base + sb.pool, sb.n_items);
}

// The chunked kernel's parameters as one block (the kernarg segment has this struct's layout).
// Its trip loop reads them through an opaque kernarg pointer at each use
// (scalar loads from the constant cache) instead of keeping them live across the loop, where
// the compiler ran out of SGPRs (106), spilled ~75 of them to VGPR lanes (v_writelane /
// v_readlane, VALU issue) and spilled VGPRs to scratch: SGPR spills 72-75 -> 34-40 in the
// fast-traversal builds; spheres-100k 2048^2 spp16 39.97 -> 38.55 ms, rain 11.65 -> 11.56 ms,
// spheres-500 unchanged (profiles/r03/exp5_ckopq/). The same change in the pool kernel (SGPR
// spills 97 -> 48) was within noise on Cornell ref and 1 % slower in fp32
// (profiles/r03/exp4_kopq/), so the pool kernel keeps its parameters in registers.
struct KernArgs {
    DevScene S0;
    RtRegion reg;
    RenderOut out;
    int tiles_x;
    SampleBuf sb;
};
__device__ __forceinline__ const KernArgs& kern_args() {
    KArgPtr p = (KArgPtr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return *(const KernArgs*)p;
}

template <class Real, bool EMIT, int INSTR, int TRAV, int LDSS>
__global__ __launch_bounds__(kBlockChunk) void pt_chunk_kernel(DevScene S0, RtRegion reg, RenderOut out,
                                                                        int tiles_x, SampleBuf sb) {
    constexpr bool COUNT = INSTR == 1;
    constexpr bool PROF = INSTR == 2;
    extern __shared__ int lds_stack[];
    const RtCamera& C0 = S0.cam;
    __shared__ PhaseRow ptab[kMaxPhases];
    phase_table_init(sb, ptab);
    const DevScene S = scene_prologue<LDSS>(S0, lds_stack);
    const int lane = threadIdx.x & (kWave - 1);
    StackT<LDSS>* stk = reinterpret_cast<StackT<LDSS>*>(lds_stack) + threadIdx.x;
    const int endX = min(reg.x + reg.width, C0.width);
    const int endY = min(reg.y + reg.height, C0.height);
    const int n_items = sb.n_items;

    uint32_t cnt[CT_WORDS];
    if (COUNT) {
#pragma unroll
        for (int k = 0; k < CT_WORDS; ++k) cnt[k] = 0;
    }
    unsigned long long st_err = 0;
    __shared__ unsigned long long prof_lds[PROF ? kProfWaves * kProfSlot : 1];
    Prof pf;
    prof_init<PROF>(pf, prof_lds, lane);

    int pool_next, pool_end;  // wave-uniform
    bool exhausted;           // wave-uniform
    first_pool(sb, pool_next, pool_end, exhausted);
    int slot = -1;                    // this lane's pixel slot (-1: idle)
    int s = 0, s_end = 0, i = 0, j = 0;
    uint32_t pix = 0;
    V3 pc = v3(0, 0, 0);  // the current item's pixel centre
    bool new_path = false;
    Path<EMIT> P;
    const double rtx = 1.0 / (double)tiles_x;
    // resumable fast traversal (product builds): per-lane walk state across iterations
    // (round 5 also parked diffuse hits until 32 / 48 lanes waited, then shaded them together:
    // 8-16 % slower - parked lanes are not walking; profiles/r05/defer_diffuse/)
    constexpr bool RS = trav_fast(TRAV) && INSTR != 1;  // (INSTR 2: timed sections)
    FastWalk<Real> W;
    bool walking = false;
    LaneBounces lb;  // SampleBuf::rec12

#define PK_SB (kern_args().sb)
#define PK_REG (kern_args().reg)
#define PK_OUT (kern_args().out)
#define PK_S (scene_view<LDSS>(kern_args().S0, lds_stack))
    while (true) {
        // hand out items to idle lanes (wave-uniform control flow); waits until
        // refill_min lanes are idle so the hand-out cost is shared
        const unsigned long long need = __ballot(slot < 0);
        const int n_need = __popcll(need);
        if (n_need != 0 && !exhausted && (n_need >= PK_SB.refill_min || __ballot(slot >= 0) == 0ull)) {
            if (pool_next >= pool_end) take_pool(PK_OUT, PK_SB, lane, pool_next, pool_end, exhausted);
            if (!exhausted) {
                const int take = min(n_need, pool_end - pool_next);
                const int rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(need >> 32),
                                                           __builtin_amdgcn_mbcnt_lo((uint32_t)need, 0u));
                if (slot < 0 && rank < take) {
                    int tl, l, s1, e1;
                    item_decode(PK_SB, ptab, pool_next + rank, tl, l, s1, e1);
                    if (slot_pixel(PK_SB, PK_REG, tiles_x, rtx, endX, endY, tl * 64 + l, i, j)) {
                        slot = tl * 64 + l;
                        s = s1;
                        s_end = e1;
                        pix = (uint32_t)j * (uint32_t)C0.width + (uint32_t)i;
                        pc = pixel_center<Real>(cam_opaque(), i, j);
                        new_path = true;
                    }
                }
                pool_next += take;
            }
        }
        psec<PROF>(pf, PR_TILE);  // the item hand-out (wave-uniform)
        if (__ballot(slot >= 0) == 0ull) {
            if (exhausted) break;
            continue;
        }
        if constexpr (RS) {
            // the sample's radiance and bounce count to its record; next sample or idle
            auto finish_sample = [&](V3 c) {
                rec_put<false>(PK_SB, (size_t)s * PK_SB.stride_s + (size_t)slot * PK_SB.stride_slot, c,
                               P.bounces | rec_err_bits(PK_SB.err_in_rec, st_err), lb, PK_OUT.stats);
                ++s;
                if (s < s_end) new_path = true;
                else slot = -1;
            };
            const RtCamera& C = cam_opaque();
            prof_trip<PROF>(pf);
            // lanes between rays: start a path if needed, then the level's depth
            // cut-off / roulette, and the walk of its ray
            if (slot >= 0 && !walking) {
                if (new_path) {
                    path_begin<Real, EMIT>(C, P, pc, pix, (uint32_t)(PK_SB.s_base + s));
                    new_path = false;
                    psec<PROF>(pf, PR_NEWPATH);
                }
                V3 c;
                if (path_pre<Real, EMIT, PROF>(C, P, pf, c)) {
                    finish_sample(c);
                } else {
                    fast_walk_begin<Real, COUNT>(PK_S, P.o, P.d, W, cnt);
                    walking = true;
                }
            }
            psec<PROF>(pf, PR_RR);
            const bool was_walking = walking;
            fast_walk_rounds<Real, COUNT, TRAV == TRAV_FAST_DEFER, PROF, kStackStride, LDSS == 0>(
                PK_S, P.o, P.d, W, walking, stk, PK_SB.min_ready, exhausted, cnt, &pf);
            psec<PROF>(pf, PR_HIT);
            // walks that ended: the rest of the level (miss / emission / scatter / light sampling)
            if (was_walking && !walking) {
                fast_walk_resolve<Real, COUNT>(PK_S, P.o, P.d, W, cnt);
                V3 c;
                if (path_post<Real, EMIT, COUNT, PROF>(PK_S, C, P, W.best, W.best_t, cnt, st_err, pf, c))
                    finish_sample(c);
            }
            psec<PROF>(pf, PR_ACC);
        } else if (slot >= 0) {
            const RtCamera& C = cam_opaque();
            prof_trip<PROF>(pf);
            if (new_path) {
                path_begin<Real, EMIT>(C, P, pc, pix, (uint32_t)(PK_SB.s_base + s));
                new_path = false;
                psec<PROF>(pf, PR_NEWPATH);
            }
            V3 c;
            if (path_trip<Real, EMIT, COUNT, PROF, TRAV>(PK_S, C, P, stk, cnt, st_err, pf, c)) {
                rec_put<false>(PK_SB, (size_t)s * PK_SB.stride_s + (size_t)slot * PK_SB.stride_slot, c,
                               P.bounces | rec_err_bits(PK_SB.err_in_rec, st_err), lb, PK_OUT.stats);
                if (COUNT) {
                    cnt[CT_SAMPLES]++;
                    cnt[CT_BOUNCES] += (uint32_t)P.bounces;
                }
                ++s;
                if (s < s_end) new_path = true;
                else slot = -1;
                psec<PROF>(pf, PR_ACC);
            }
        }
    }
    PixStats st;
    lb.to(st);
    publish_stats(out, st, st_err, lane);
    publish_counters<COUNT, PROF>(out, cnt, pf, lane);
#undef PK_SB
#undef PK_REG
#undef PK_OUT
#undef PK_S
}

}  // namespace rt
