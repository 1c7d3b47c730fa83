// ---------------------------------------------------------------------------
// Stage-compacted pool kernel (fixed spp, no emission stack): the chunked
// kernel's work items and per-sample records, but lanes are not tied to paths.
// Each wave keeps kPoolK path slots in LDS and four stacks of slot indices:
// `an` (samples whose path is to start), `d` / `dl` (diffuse hits waiting for the
// cosine-PDF / light-PDF generate) and `ac` (paths continuing after a specular
// scatter). A trip pops up to 64 slots and runs one FRONT stage, chosen for the
// whole wave, then the BACK stage that every path shares:
//   front N: pops `an` - the item hand-out and the path start (getRay);
//   front Dc / Dl: pops `d` / `dl` - the mixture-PDF light sampling, its value and
//     the throughput update (src/camera.ts:263-315) of one sampling branch; the
//     bounce's new ray stays in registers. Free lanes are filled from `ac`; they idle
//     through the front;
//   no front: pops `ac` alone - only from a full wave or when no other stack has work
//     (the drain at a launch's end), so specular paths never park slots;
//   back: depth cut-off / roulette, closest hit (after N with the primary-ray table:
//     the table's candidates), miss or hit record + material scatter. The path's sample
//     is recorded, or it continues specularly (`ac`), or its diffuse hit is queued by the
//     mixture's branch: the back draws the mixture uniform ahead (on a copy of the path's
//     RNG state; D draws the same value again), so a D front runs one of the two sampling
//     branches instead of both at half the lanes.
// One slot-store block and one group of ballot/mbcnt queue appends end a trip: a diffuse
// bounce passes through the slot once (hit -> D), not twice (2.6 trips per 64 samples
// where a trace stage and a diffuse stage of their own took 4.1). The diffuse shading
// still runs on full waves rather than on the lanes whose path happens to need it in a
// given trip (the north star's persistent-wavefront work queues). Each path's arithmetic
// and draw order are path_trip's, so every sample record - and the image - is
// bit-identical.
// ---------------------------------------------------------------------------
#pragma once

#include <hip/hip_runtime.h>

#include "pt_kernels.hpp"

namespace rt {

// Per wave: slot state as [group][slot] float4, then the A queue (a ring) and the D queue
// (u8 slot indices; two stacks in one array each. D: cosine-branch paths from
// the bottom, light-branch paths from the top - together at most kPoolK entries).
// 56 bytes per slot (more slots per wave fill more trips: 64 / 80 / 96 slots ran Cornell in
// 21.7 / 17.7 / 16.1 ms, profiles/r02/poolsize/; 119 / 134 / 152 slots followed):
//   g0 {rng lo, rng hi, meta, hs}   meta = (phase + 2) | log2(item chunk) << 8 | lambert material << 11
//                                   (D only), phase: bounces so far (>= 0), PH_NEW or PH_ITEM;
//                                   hs = h | planar << 14 | front << 15 (D only) | s << 16
//   g1 {o (hit point p when queued for D), slot}
//   g2 {d (the face normal when queued for D), T.x}
//   g3 {T.y, T.z}                    (the 8-byte group)
// The item's end is the next multiple of its (power-of-two) chunk, the pixel comes from the
// slot (item_pixel), and the D stage reads the Lambertian albedo (the scatter's attenuation)
// from the material table. Host gates: spp <= 65535, depth <= 250, materials < 2^21,
// primitives < 2^14, power-of-two chunks.
__device__ __forceinline__ float pool_meta(int phase, int clog2, int mat) {
    return __uint_as_float((uint32_t)((phase + 2) & 0xff) | ((uint32_t)clog2 << 8) | ((uint32_t)mat << 11));
}
__device__ __forceinline__ int meta_phase(float m) { return (int)(__float_as_uint(m) & 0xffu) - 2; }
__device__ __forceinline__ int meta_clog2(float m) { return (int)((__float_as_uint(m) >> 8) & 7u); }
__device__ __forceinline__ int meta_mat(float m) { return (int)(__float_as_uint(m) >> 11); }
__device__ __forceinline__ float pool_hs(int hf16, int s) { return __uint_as_float(((uint32_t)hf16 & 0xffffu) | ((uint32_t)s << 16)); }
__device__ __forceinline__ int hs_s(float v) { return (int)(__float_as_uint(v) >> 16); }
__device__ __forceinline__ int hs_hf(float v) { return (int)(__float_as_uint(v) & 0xffffu); }
__device__ __forceinline__ int item_end(int s, int clog2) { return ((s >> clog2) + 1) << clog2; }
enum : int { PH_NEW = -1, PH_ITEM = -2 };  // next sample's path to start / no work item

// Stacks in one array: the bottom one fills [0, cnt), the top one [kPoolK - cnt, kPoolK).
__device__ __forceinline__ void stack_push(uint8_t* q, bool top, int& cnt, bool want, int k) {
    const unsigned long long m = __ballot(want);
    if (want) {
        const int r = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        q[top ? kPoolK - 1 - (cnt + r) : cnt + r] = (uint8_t)k;
    }
    cnt += __popcll(m);
}

// The primary-ray candidate table's pointer (pt_pool_primary_kernel's last argument, after
// pt_pool_kernel's), read through the opaque kernarg pointer where a new-path trip needs it
// (one scalar load) instead of a register pair live across the trip loop.
struct KernArgsPrimary {
    KernArgs args;
    const uint2* ptab;  // by row-major pixel (primary.hpp)
};
__device__ __forceinline__ const uint2* primary_table_opaque() {
    KArgPtr p = (KArgPtr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return *(const uint2* const*)(p + offsetof(KernArgsPrimary, ptab));
}

// The pool kernel's body, shared by its two entries. PRIM: the trips that start new paths
// take each primary ray's candidates from the primary-ray table (primary.hpp) instead
// of running the fp32 pre-filter pass: an N trip pops only the `an` stack (no `ac` lanes
// ride in it), so a trip is wave-uniformly all primary rays or none, and the branch costs
// no divergence.
template <class Real, int TRAV, int LDSS, bool PRIM>
// (The arguments by value, as the entries take them: by reference the compiler kept them in the
// kernarg segment and the LDS-resident ref kernel went from 53 to 76 spilled SGPRs.)
__device__ __forceinline__ void pool_trips(DevScene S0, RtRegion reg, RenderOut out, int tiles_x, SampleBuf sb) {
    extern __shared__ int lds_stack[];
    const RtCamera& C0 = S0.cam;
    __shared__ PhaseRow ptab[kMaxPhases];
    phase_table_init(sb, ptab);
    const DevScene S = scene_prologue<LDSS>(S0, lds_stack);
    const int lane = threadIdx.x & (kWave - 1);
    StackT<LDSS>* stk = reinterpret_cast<StackT<LDSS>*>(lds_stack) + threadIdx.x;
    char* wpool = reinterpret_cast<char*>(lds_stack) + S0.lds_pool_off + (size_t)(threadIdx.x / kWave) * kPoolWaveBytes;
    float4* G = reinterpret_cast<float4*>(wpool);  // group q of slot k: G[q * kPoolK + k]
    float2* G3 = reinterpret_cast<float2*>(wpool + (size_t)kPoolK * kPoolGroups * 16);  // the 8-byte group
    uint8_t* qa = reinterpret_cast<uint8_t*>(wpool + (size_t)kPoolK * (kPoolGroups * 16 + 8));
    uint8_t* qd = qa + kPoolK;
    const int endX = min(reg.x + reg.width, C0.width);
    const int endY = min(reg.y + reg.height, C0.height);
    const int n_items = sb.n_items;
    const double rtx = 1.0 / (double)tiles_x;
    uint32_t* cnt = nullptr;  // product build: no work counters
    unsigned long long st_err = 0;
    constexpr bool PP = RT_POOL_PROF;
    __shared__ unsigned long long prof_lds[PP ? kProfWaves * kProfSlot : 1];
    Prof pf;
    prof_init<PP>(pf, prof_lds, lane);

    for (int k = lane; k < kPoolK; k += kWave) {
        qa[k] = (uint8_t)k;
        G[k] = make_float4(0.f, 0.f, pool_meta(PH_ITEM, 0, 0), 0.f);
    }
    // wave-uniform queue state. qd: the cosine-branch stack from the bottom (d_cnt), the
    // light-branch stack from the top (dl_cnt). qa: paths to start from the bottom (an_cnt),
    // paths continuing after a specular scatter from the top (ac_cnt).
    int d_cnt = 0, dl_cnt = 0;
    int an_cnt = kPoolK, ac_cnt = 0;
    int pool_next, pool_end;  // wave-uniform item hand-out
    bool exhausted;
    first_pool(sb, pool_next, pool_end, exhausted);

    // the sample's radiance and bounce count to its record; the slot's next phase
    // `err`: the sample's error flags (its miss without a background): in the record in
    // adaptive rounds (SampleBuf::err_in_rec), else in the launch's stats
    LaneBounces lb;  // SampleBuf::rec12
    auto record = [&](V3 c, int bounces, int slot, int& s, int s_end, unsigned long long err = 0ull) -> int {
        if (!sb.err_in_rec) st_err |= err;
        rec_put<true>(sb, (size_t)s * sb.stride_s + (size_t)slot * sb.stride_slot, c,
                           bounces | (sb.err_in_rec ? (int)((uint32_t)err << kRecErrShift) : 0), lb, out.stats);
        ++s;
        return s < s_end ? PH_NEW : PH_ITEM;
    };

    enum : int { FR_N, FR_D, FR_NONE };  // a trip's front stage
    while (an_cnt + ac_cnt + d_cnt + dl_cnt > 0) {
        // other lanes' slot and queue writes of the previous trip (one wave: LDS is in order)
        __asm__ volatile("" ::: "memory");
        prof_trip<PP>(pf);
        psec<PP>(pf, PR_ACC);  // the previous trip's records, slot stores and queue appends
        // ---- the front's choice: a stack that fills the wave (D, ac, N in that order), else the
        // longer D stack, else N; ac alone only as a full wave or when nothing else has work ----
        const bool dtop = dl_cnt > d_cnt;  // the longer D stack
        const int dn = dtop ? dl_cnt : d_cnt;
        const int fr = dn >= kWave       ? FR_D
                       : ac_cnt >= kWave ? FR_NONE
                       : an_cnt >= kWave ? FR_N
                       : dn > 0          ? FR_D
                       : an_cnt > 0      ? FR_N
                                         : FR_NONE;
        int k = -1;
        int nd = 0;  // FR_D: the lanes that shade a diffuse bounce (the rest ride from ac)
        if (fr == FR_D) {
            nd = min(kWave, dn);
            const int na = min(kWave - nd, ac_cnt);
            if (lane < nd) k = (int)qd[dtop ? kPoolK - dl_cnt + lane : d_cnt - nd + lane];
            else if (lane < nd + na) k = (int)qa[kPoolK - ac_cnt + lane - nd];
            if (dtop) dl_cnt -= nd;
            else d_cnt -= nd;
            ac_cnt -= na;
        } else if (fr == FR_N) {
            const int n = min(kWave, an_cnt);
            if (lane < n) k = (int)qa[an_cnt - n + lane];
            an_cnt -= n;
        } else {
            const int n = min(kWave, ac_cnt);
            if (lane < n) k = (int)qa[kPoolK - ac_cnt + lane];
            ac_cnt -= n;
        }
        float4 g0 = make_float4(0.f, 0.f, pool_meta(PH_ITEM, 0, 0), 0.f), g1 = g0, g2 = g0;
        float2 g3 = make_float2(0.f, 0.f);
        if (k >= 0) {
            g0 = G[k];
            g1 = G[kPoolK + k];
            g2 = G[2 * kPoolK + k];
            g3 = G3[k];
        }
        int phase = meta_phase(g0.z), clog2 = meta_clog2(g0.z), slot = __float_as_int(g1.w);
        int s = hs_s(g0.w);
        const RtCamera& C = cam_opaque();
        Path<false> P;
        bool keep = k >= 0;
        bool path = false;  // the lane holds a path in this trip
        bool term = false;  // ... which ends in it: `c` is the sample's radiance
        V3 c = v3(0, 0, 0);
        uint2 prec = make_uint2(0u, 0u);  // PRIM: the pixel's record of the primary-ray table
        if (fr == FR_N) {
            // ---- N: work items for slots without one (the chunked kernel's guided hand-out),
            // then the path starts ----
            const unsigned long long need = __ballot(k >= 0 && phase == PH_ITEM);
            if (need != 0ull && !exhausted) {
                if (pool_next >= pool_end) take_pool(out, sb, lane, pool_next, pool_end, exhausted);
                if (!exhausted) {
                    const int take = min(__popcll(need), pool_end - pool_next);
                    const int rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(need >> 32),
                                                               __builtin_amdgcn_mbcnt_lo((uint32_t)need, 0u));
                    if (k >= 0 && phase == PH_ITEM && rank < take) {
                        int tl, l, s1, e1, i, j;
                        item_decode(sb, ptab, pool_next + rank, tl, l, s1, e1);
                        if (slot_pixel(sb, reg, tiles_x, rtx, endX, endY, tl * 64 + l, i, j)) {
                            slot = tl * 64 + l;
                            s = s1;
                            clog2 = __builtin_ctz((uint32_t)(e1 - s1));  // power-of-two, aligned chunks
                            phase = PH_NEW;
                        }
                    }
                    pool_next += take;
                }
            }
            keep = k >= 0 && (phase != PH_ITEM || !exhausted);  // drained slots leave the pool
            if (k >= 0 && phase == PH_NEW) {
                path = true;
                int i, j;  // the slot's pixel (the hand-out's slot_pixel)
                slot_pixel(sb, reg, tiles_x, rtx, endX, endY, slot, i, j);
                const uint32_t pix = (uint32_t)j * (uint32_t)C.width + (uint32_t)i;
                if (PRIM) prec = primary_table_opaque()[pix];  // in flight during the path start
                path_begin<Real, false>(C, P, pixel_center<Real>(C, i, j), pix, (uint32_t)(sb.s_base + s));
                // Wait for the record here, inside the block that issued its load (slot_pixel's
                // note): pending on the paths around this block, its registers would make later
                // writes of them wait with vmcnt(0), for the sample records stored before them too.
                // This is the trip loop's one vector-memory load; on gfx9 the wait also covers the
                // previous trip's record stores, which the path start has given time to drain.
                if (PRIM) __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0) (gfx9 encoding)
            }
            psec<PP>(pf, PR_NEWPATH);  // item hand-out and path starts
        } else {
            if (k >= 0) {
                path = true;
                P.rng = (uint64_t)__float_as_uint(g0.x) | ((uint64_t)__float_as_uint(g0.y) << 32);
                P.o = V3{g1.x, g1.y, g1.z};
                P.d = V3{g2.x, g2.y, g2.z};
                P.T = V3{g2.w, g3.x, g3.y};
                P.bounces = phase;
                P.em_n = 0;
            }
            if (fr == FR_D) {
                // ---- Dc / Dl: diffuse shading of the queued hits (o = the hit point, d = the face
                // normal); the new ray stays in registers for the back ----
                if (lane < nd) {
                    const int hf = hs_hf(g0.w);
                    const int h = hf & 0x3fff;
                    const bool planar = (hf >> 14) & 1, front = (hf >> 15) & 1;
                    const V3 att = ld3(S.mats[meta_mat(g0.z)].color);  // the Lambertian scatter's attenuation
                    const bool dterm =
                        dtop ? shade_diffuse<Real, false, false, PP, 2>(S, C, P, h, planar, front, P.o, P.d, att, cnt, pf)
                             : shade_diffuse<Real, false, false, PP, 1>(S, C, P, h, planar, front, P.o, P.d, att, cnt, pf);
                    if (dterm) {
                        // mixture value cut-off: the level's emission (as computed at the hit: T is unchanged)
                        term = true;
                        c = mulv(ld3(S.mats[S.prims[h].mat].emitted), P.T);
                    }
                }
            } else {
                psec<PP>(pf, PR_NEWPATH);  // a pure ac trip: the slot loads
            }
        }
        // ---- the back: depth cut-off / roulette, closest hit, miss or hit record + scatter ----
        bool to_d = false, d_light = false;
        int hf = 0, dmat = 0;
        unsigned long long err = 0ull;  // this sample's error flags (its miss)
        if (path && !term) {
            term = path_pre<Real, false, PP>(C, P, pf, c);
            if (!term) {
                const RayK<Real> ray = make_ray<Real>(P.o, P.d);
                Real t;
                int h;
                V3 att;
                if (PRIM && fr == FR_N) {  // every lane traces a primary ray
                    psec<PP>(pf, PR_TILE);  // (no pre-filter section)
                    h = closest_hit_primary<Real, false>(S, ray, t, prec, cnt);
                } else if (PP && TRAV == TRAV_BRUTE && C.n_prims <= kBruteMaxPrims)  // section timer
                    h = closest_hit_brute_nf<Real, false>(S, C.n_prims, ray, t, lot_column(stk), cnt,
                                                          [&]() { psec<PP>(pf, PR_TILE); });
                else
                    h = closest_hit_any<Real, false, TRAV>(S, C.n_prims, ray, t, stk, cnt);
                psec<PP>(pf, PR_HIT);
                if (h < 0) {
                    term = true;
                    c = miss_color<Real, false, PP>(C, P, err, pf);
                } else {
                    V3 p, nrm, emitted, sdir;
                    bool front, planar;
                    const int kind = shade_hit<Real, false, false, PP>(S, P, h, t, cnt, pf, p, nrm, front, planar,
                                                                          emitted, att, sdir, &dmat);
                    if (kind == SC_NONE) {
                        term = true;
                        c = emitted;
                    } else {
                        ++P.bounces;
                        P.o = p;
                        if (kind == SC_SPEC) {
                            P.T = mulv(P.T, att);
                            P.d = sdir;
                        } else {
                            to_d = true;
                            P.d = nrm;  // queued for D: g2 carries the face normal
                            hf = h | (planar ? (1 << 14) : 0) | (front ? (1 << 15) : 0);
                            {  // shade_diffuse's first draw and branch, ahead
                                uint64_t r = P.rng;
                                const Real u0 = uniform<Real>(r);
                                const Real rnd = S.mix_total == 1.0 ? u0 : u0 * (Real)S.mix_total;
                                d_light = !(rnd < (Real)0.5 || C.n_lights == 0);
                            }
                        }
                    }
                }
            }
        }
        // ---- the trip's end: the record, the slot and its queue ----
        if (path) {
            phase = term ? record(c, P.bounces, slot, s, item_end(s, clog2), err) : P.bounces;
            g0 = make_float4(__uint_as_float((uint32_t)P.rng), __uint_as_float((uint32_t)(P.rng >> 32)),
                             pool_meta(phase, clog2, to_d ? dmat : 0), pool_hs(to_d ? hf : 0, s));
            g1 = make_float4(P.o.x, P.o.y, P.o.z, __int_as_float(slot));
            g2 = make_float4(P.d.x, P.d.y, P.d.z, P.T.x);
            g3 = make_float2(P.T.y, P.T.z);
        } else if (keep) {  // a slot still waiting for a work item
            g0 = make_float4(0.f, 0.f, pool_meta(PH_ITEM, 0, 0), 0.f);
        }
        if (keep) {
            G[k] = g0;
            G[kPoolK + k] = g1;
            G[2 * kPoolK + k] = g2;
            G3[k] = g3;
        }
        stack_push(qa, false, an_cnt, keep && !to_d && phase < 0, k);
        stack_push(qa, true, ac_cnt, keep && !to_d && phase >= 0, k);
        stack_push(qd, false, d_cnt, to_d && !d_light, k);
        stack_push(qd, true, dl_cnt, to_d && d_light, k);
    }
    PixStats st;
    lb.to(st);
    publish_stats(out, st, st_err, lane);
    publish_counters<false, PP>(out, cnt, pf, lane);
}

template <class Real, int TRAV, int LDSS>
__global__ __launch_bounds__(kBlockPool) void pt_pool_kernel(DevScene S0, RtRegion reg, RenderOut out, int tiles_x,
                                                               SampleBuf sb) {
    pool_trips<Real, TRAV, LDSS, false>(S0, reg, out, tiles_x, sb);
}
// The pool kernel with the primary-ray candidate table `ptab`: brute-force launches of a
// pinhole camera with at most kBruteMaxPrims primitives (launch_plan.cpp). The trip loop reads
// `ptab` through primary_table_opaque.
template <class Real, int TRAV, int LDSS>
__global__ __launch_bounds__(kBlockPool) void pt_pool_primary_kernel(DevScene S0, RtRegion reg, RenderOut out,
                                                                       int tiles_x, SampleBuf sb, const uint2* ptab) {
    (void)ptab;
    pool_trips<Real, TRAV, LDSS, true>(S0, reg, out, tiles_x, sb);
}

}  // namespace rt
