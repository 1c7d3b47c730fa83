// The launch ABI between the host units and the kernels: the scene view, the output and
// sample-buffer structs, the stats / counter word indices and the launch-geometry constants.
// Declarations only: no device code (the kernels' layers are pt_num.hpp ... pt_pool.hpp).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "rt_math.hpp"
#include "scene_types.hpp"

namespace rt {

// The scene lives in one device buffer ("blob", scene_blob.cpp build_scene_blob):
// [t4nodes][tprims][tsph][prims][xrec] | [mats][lights][onbs] | [nodes][pre][tsph2], 16-byte
// aligned sections. When the first group fits beside the stack, every workgroup copies it into
// LDS (LDS-resident launch, level 1): traversal and primitive reads are LDS reads; level 2 also
// copies the second group.
struct DevScene {
    const RtT4Node* __restrict__ t4nodes; // fast traversal: 4-wide nodes (blob start; LDS when resident)
    const RtPrim* __restrict__ prims;   // global, or LDS in an LDS-resident launch
    const RtPrim* __restrict__ gprims;  // always the global copy (scalar-load reads)
    const RtPre* __restrict__ gpre;     // brute-force pre-filter records (global, scalar-load reads)
    int32_t n_pre;                      // ... and their count (pairs count once)
    const RtExact* __restrict__ xrec;   // brute-force exact-test records (LDS when resident), slot order
    int32_t off_xrec;                   // byte offset of xrec in the blob
    const int32_t* __restrict__ tprims; // fast-traversal leaves -> primitive slots (LDS when resident)
    const float4* __restrict__ tsph;    // per tprims entry: sphere {centre, fp32 radius} or NaNs (LDS when resident)
    const RtMat* __restrict__ mats;
    const RtLight* __restrict__ lights;
    const RtLight* __restrict__ glights; // always the global copy (scalar-load reads)
    const RtNode* __restrict__ nodes;   // the reference's boxes (reference traversal)
    const RtOnb* __restrict__ onbs;     // [slot][precision][face] for slots < n_onb (LDS at level 2)
    int32_t n_onb;                      // planar primitives' ONB table covers slots [0, n_onb)
    int32_t off_onbs;                   // byte offset of onbs in the blob
    const uint4* __restrict__ blob;     // the whole scene (section order above)
    int32_t lds_words;                  // 16-byte words of the blob prefix copied to LDS (LDSS 1: [t4nodes][tprims][tsph][prims][xrec],
                                        // LDSS 2: also [mats][lights][onbs])
    int32_t off_prims;                  // byte offset of prims in the blob
    int32_t off_mats;                   // byte offset of mats in the blob
    int32_t off_lights;                 // byte offset of lights in the blob
    int32_t off_tprims;                 // byte offset of tprims in the blob
    int32_t off_tsph;                   // byte offset of tsph in the blob
    int32_t lds_stack_bytes;            // LDS bytes of the traversal stack (scene follows)
    int32_t lds_pool_off;               // pool kernel: byte offset of the per-wave path pools (after the scene)
    int32_t lds_node_pad;               // LDS copy: one 16-byte pad row after each 4-wide node (t4 nodes, or 0)
    int32_t t4_stride;                  // bytes between 4-wide nodes where the walk reads them (128 or 144)
    int32_t n_top;                      // launches walking the tree from global memory: nodes [0, n_top)
                                        // (breadth-first: the tree's top) have a padded copy in LDS
    const char* top_lds;                // ... after the traversal stack (scene_view; LDSS 0 only)
    const RtLeafSph* __restrict__ tsph2; // trees walked from global memory: leaf-order sphere records with
                                         // the fp64 radius and the slot (one load per exact test), or null
    int32_t nearfar;                    // 4-wide node step picks near / far rows by the ray's signs (t4_step);
                                        // scene_view sets a constant per LDS level (see there)
    int32_t t4root;                     // fast traversal root reference (node index or leaf code)
    RtNode root_box;                    // fast traversal root box (padded)
    RtCamera cam;
    double mix_total;  // MixturePDF.totalWeight for [0.5, 0.5/nL x nL]
    double light_w;    // 0.5 / nL
};

// Stats words (u64): pixels, samples total, samples min, samples max,
// bounces total, bounces min, bounces max, error flags.
enum { ST_PIXELS = 0, ST_SAMPLES, ST_SMIN, ST_SMAX, ST_BOUNCES, ST_BMIN, ST_BMAX, ST_ERROR, ST_WORDS };
// Each stats word on a 128-byte line of its own (stats[k * kStatStride]): the atomics of
// thousands of waves on one line serialise (~90 per us per line).
constexpr int kStatStride = 16;
// Instrumentation words (u64): the algorithmic-work counts of SURVEY.md §8d.
enum {
    CT_NODE = 0, CT_SPHERE, CT_QUAD, CT_PLANE, CT_MATERIAL, CT_LIGHT_QUAD, CT_LIGHT_SPHERE,
    CT_BOUNCES, CT_DIFFUSE, CT_SAMPLES, CT_RAYS,
    CT_EXACT,       // primitives whose exact fp64 test ran (per lane)
    CT_EXACT_WAVE,  // exact-test blocks a wave executed (any lane), counted once per wave
    CT_CAND0,       // brute force: rays with no pre-filter candidate
    CT_CAND2,       // brute force: rays with two or more pre-filter candidates
    CT_EXACT2,      // brute force: rays that needed two or more exact tests
    CT_WORDS
};
enum : unsigned long long { ERR_NO_BACKGROUND = 1ull, ERR_EMIT_STACK = 2ull };
constexpr int kRecErrShift = 30;  // error flags in a sample record's bounce word (SampleBuf::err_in_rec)
constexpr uint32_t kRecBounceMask = (1u << kRecErrShift) - 1u;
// Diagnostic build (INSTR == 2): wave-cycles spent in each section of the path
// loop (s_memtime, summed over waves), stored after the CT_WORDS counters.
enum {
    PR_NEWPATH = 0, PR_RR, PR_HIT, PR_MISS, PR_HITREC, PR_SCATTER, PR_SAMPLE, PR_PDF, PR_ACC, PR_TILE,
    PR_NODE, PR_LEAF,  // lane counts only (no cycles): node-step and leaf-test iterations of the walk
    PR_WNODE, PR_WLEAF,  // resumable walk: cycles of its node-step loops / leaf phases (part of PR_HIT's walk)
    PR_LOOP, PR_TRIPS, PR_WORDS
};
// INSTR == 2 also records, per section k < PR_LOOP, the lanes active when a wave
// ended it (summed, at CT_WORDS + PR_WORDS + k) and how many times a wave did
// (at CT_WORDS + PR_WORDS + PR_LOOP + k): active lanes per execution of a section.
constexpr int kCounterWords = 64;  // CT_WORDS + PR_WORDS + 2 * PR_LOOP, rounded up
static_assert(CT_WORDS + PR_WORDS + 2 * PR_LOOP <= kCounterWords, "counter words");

struct RenderOut {
    uint8_t* rgb;        // W*H*3 (full frame layout), may be null
    float* radiance;     // W*H*3, may be null
    int32_t* px_samples; // W*H, may be null
    int32_t* px_bounces; // W*H, may be null
    unsigned long long* stats;     // ST_WORDS words, kStatStride apart
    unsigned long long* counters;  // kCounterWords (instrumented builds only)
    unsigned int* tile_counter;
    // 0: outputs in full-frame layout (index j*W + i); 1: tile-packed slab, the
    // pixel of lane l of this launch's k-th tile at k*64 + l (multi-GPU gather)
    int32_t packed;
};

// Closest-hit strategies; all return the reference's hit bit-for-bit (pt_isect.hpp closest_hit,
// pt_walk.hpp closest_hit_fast, pt_brute.hpp closest_hit_brute*). AUTO is resolved on the host.
enum Traversal : int32_t { TRAV_FAST = 0, TRAV_REFERENCE = 1, TRAV_BRUTE = 2, TRAV_AUTO = 3,
                           TRAV_FAST_DEFER = 4 };  // kernel-internal: FAST with deferred exact sphere tests
constexpr bool trav_fast(int t) { return t == TRAV_FAST || t == TRAV_FAST_DEFER; }
constexpr int kBruteMaxPrims = 16;  // AUTO picks BRUTE up to this many primitives (nearest-first form: <= 32)

constexpr int kWave = 64;
// Persistent workgroups, one per CU, sharing one LDS scene copy:
//   sequential kernel 768 threads (12 waves = 3 per SIMD, <= 168 VGPRs),
//   chunked kernel 1024 threads (16 waves = 4 per SIMD, <= 128 VGPRs).
constexpr int kBlock = 768;
constexpr int kBlockChunk = 1024;
constexpr int kStackStride = 1024;  // LDS traversal-stack column stride (>= any block size)
// Stack entries of the fast walk: 16-bit in launches whose tree is LDS-resident (its
// node references and leaf codes ~(first << 3 | count) fit an int16: at most ~1,000 nodes and
// primitives fit the LDS copy), so the stack takes half the LDS and the material / light tables
// fit beside it (LDS residency level 2); 32-bit where the tree is walked from global memory.
// Entries hold a node reference only (a popped subtree is culled one level later by its
// children's slab tests).
template <int LDSS>
using StackT = typename std::conditional<(LDSS > 0), int16_t, int32_t>::type;
constexpr int kTile = 8;          // 8x8 pixels per wave-tile
constexpr int kEmitStack = 128;   // emission terms kept for the right fold (EMIT builds)
// The section timer's per-wave LDS slot (pt_prof.hpp): [0] last stamp, [1] start stamp, then
// cycles, active lanes and executions per section.
constexpr int kProfSlot = 2 + 3 * PR_WORDS;
constexpr int kProfWaves = 16;  // >= waves per workgroup of either kernel

// Guided schedule: phase p covers samples [s0[p], s0[p] + nch[p] * chunk[p]) in
// chunks of chunk[p]; items are numbered phase by phase (item_base[p]), and
// chunks halve from phase to phase, so the launch ends on 1-sample items.
constexpr int kMaxPhases = 8;
struct SampleBuf {
    float4* rec;    // record of (sample s, pixel slot) at s * stride_s + slot * stride_slot: {r, g, b, bounces (int bits)}
    int64_t stride_s, stride_slot;  // sample-major ([sample][slot]) or slot-major ([slot][sample])
    int32_t slots;  // pixel slots in this pass = pass_tiles * 64
    int32_t tile0;  // first of this pass's tiles (index among this launch's tiles)
    int32_t pool;   // items a wave takes from the global counter at a time (multiple of 64)
    int32_t n_phases;
    int32_t n_items;
    int32_t refill_min;  // idle lanes that trigger a hand-out (all-idle always does)
    int32_t min_ready;   // resumable fast traversal: lanes done walking before the wave shades
    // Adaptive-sampling rounds (pt_adapt_kernel): the pass's record slot a renders the launch
    // slot act[a] (tile * 64 + lane over the launch's tiles; tile0 is 0), samples s_base + s.
    // act == nullptr: slot a is pass tile tile0 + a / 64, lane a % 64, samples from 0.
    const int32_t* act;
    int32_t s_base;
    // Adaptive rounds: a sample's error flags (ERR_*) travel in bits 30-31 of its record's
    // bounce word instead of the launch's stats, so pt_adapt_kernel counts only the flags of
    // the samples it keeps - a round renders samples past a pixel's convergence, which the
    // reference never renders (src/camera.ts:400-425). Bounce counts stay below 2^30
    // (loop_threshold caps depth at 1e9).
    int32_t err_in_rec;
    // 12-byte records {r, g, b} (float triples at (float*)rec + 3 * index), the bounce statistics
    // reduced by the path kernel itself (LaneBounces): fixed spp in colour mode without the
    // per-pixel bounce output, where the accumulate pass needs only each pixel's colour sum in
    // sample order - RenderStats' bounce total / min / max are order-free integer reductions
    // (src/render-utils/renderStats.ts:21-35). A quarter less record traffic.
    int32_t rec12;
    int32_t s0[kMaxPhases], chunk[kMaxPhases], nch[kMaxPhases], item_base[kMaxPhases];
    double rnch[kMaxPhases];  // 1.0 / nch
};

// Adaptive sampling in rounds (pt_adapt_kernel): a pixel's running PixelStats
// between rounds (src/render-utils/renderStats.ts:66-88), by launch slot.
struct AdaptPix {
    float4 c;     // colour sum (fp32, sample order), n (int bits)
    double2 ill;  // sumIll, sumIll2
    int4 b;       // bounce sum (low 32 bits), min, max, bounce sum (high 32 bits)
};
struct AdaptRound {
    AdaptPix* state;        // launch slots (tile * 64 + lane)
    int32_t* next_act;      // the pixels still sampling after this round
    unsigned int* next_count;  // [0]: pixels carried; [1]: those likely to converge by `horizon`
    int32_t len;            // samples of this round
    int32_t horizon;        // sample count the round-length rule asks about (dev_ctx.cpp)
};

#ifndef RT_POOL_K
#define RT_POOL_K 152  // 56-byte slots + 2 queue bytes per wave, beside fp16 candidate columns
#endif
#ifndef RT_POOL_PROF
#define RT_POOL_PROF 0  // diagnostic variant: section timing (INSTR == 2 launches) in the pool kernel
#endif
constexpr int kPoolK = RT_POOL_K;          // path slots per wave
constexpr int kBlockPool = 1024;           // persistent workgroup size
constexpr int kPoolGroups = 3;             // 16-byte groups per slot, plus one 8-byte group
static_assert(kPoolK >= kWave && kPoolK <= 256, "pool slots: one full wave, u8 queue entries");
// Per wave (pt_pool.hpp has the slot layout): kPoolK slots of kPoolGroups float4 groups and one
// 8-byte group, then the two u8 queues of kPoolK entries each; rounded up to 16 bytes.
constexpr size_t kPoolWaveBytes = ((size_t)kPoolK * (kPoolGroups * 16 + 8) + 2 * kPoolK + 15) / 16 * 16;
constexpr int kPoolClog2Bits = 3;  // log2(item chunk) field of the slot meta word
constexpr int kPoolMaxChunk = 1 << ((1 << kPoolClog2Bits) - 1);  // 128 samples
constexpr size_t pool_lds_bytes() { return (size_t)(kBlockPool / kWave) * kPoolWaveBytes; }

}  // namespace rt
