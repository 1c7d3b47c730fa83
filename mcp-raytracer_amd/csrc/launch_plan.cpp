// Launch planning (launch_plan.hpp). Compiled like the ABI units (it reads pt_types.hpp's
// constants and SampleBuf) but calls nothing of the HIP runtime.
#include "launch_plan.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>

#include "dev_ctx.hpp"
#include "host_util.hpp"

namespace rt {

static_assert(kBlobBruteMaxPrims == kBruteMaxPrims, "scene_blob.hpp restates kBruteMaxPrims");

long pass_units(long units_left, long unit_slots, long chunks_per_slot, size_t rec_bytes_per_unit, size_t budget) {
    const long by_budget = (long)(budget / std::max<size_t>(rec_bytes_per_unit, 1));
    const long by_items = (kItemCap - 1) / (std::max<long>(unit_slots, 1) * std::max<long>(chunks_per_slot, 1));
    return std::max<long>(1, std::min(units_left, std::min(by_budget, by_items)));
}

long chunks_per_slot(const SampleBuf& sb) {
    long n = 0;
    for (int p = 0; p < sb.n_phases; ++p) n += sb.nch[p];
    return n;
}

size_t sbuf_budget() {
    const char* e = std::getenv("RT_AMD_SBUF_MB");
    const long mb = e ? std::atol(e) : 8192;
    return (size_t)std::max<long>(mb, 1) << 20;
}

long record_pass_slots(long n_act, const SampleBuf& sb, int len) {
    const size_t rec_per_slot = (size_t)len * sizeof(float4);
    return kWave * pass_units((n_act + kWave - 1) / kWave, kWave, chunks_per_slot(sb), rec_per_slot * kWave, sbuf_budget());
}

// first round: one convergence batch, then rounds x3 (tools/adapt_sweep.py, 800^2 / 1080p,
// profiles/r03/adapt_sweep.log: first 10 / 20 / 40 samples x growth 2 / 3 - one batch
// wastes least on scenes whose sky converges at the first check (rain 2.59 vs 3.36 ms at
// 20, spheres-500 5.87 vs 6.00 ms); Cornell, whose pixels converge at 10 or run to 256,
// prefers few long rounds: 15.94 ms with growth 3 vs 16.35 with 2, 15.56 at first 40)
int adaptive_first_len(const RtCamera& C) {
    const double ab = C.a_batch;
    const int batch = (ab >= 1.0 && ab < 65536.0) ? (int)ab : std::max(1, std::min(C.n_samples, 16));
    return batch * std::max(1, (env_int("RT_AMD_ADAPT_FIRST", batch) + batch - 1) / batch);
}

size_t fixed_rec_bytes_per_tile(const RtCamera& C, bool rec12) {
    return (size_t)kWave * (size_t)C.n_samples * (rec12 ? 12 : sizeof(float4));
}

int number_pass_items(SampleBuf& sb, bool pool, int cus) {
    // items come in (tile, chunk) groups of 64 (item_decode): a pass of an adaptive round
    // whose slot count is not a multiple of 64 still numbers whole groups (the slots past
    // sb.slots are skipped by slot_pixel)
    const long group_slots = ((long)sb.slots + kWave - 1) / kWave * kWave;
    long items = 0;
    for (int p = 0; p < sb.n_phases; ++p) {
        sb.item_base[p] = (int32_t)items;
        items += group_slots * sb.nch[p];
    }
    if (items >= kItemCap) throw std::runtime_error("chunked pass too large");  // pass_units keeps it below
    sb.n_items = (int32_t)items;
    const int block = pool ? kBlockPool : kBlockChunk;
    return (int)std::max<long>(1, std::min<long>(items / block + 1, (long)cus));
}

long region_pixels(const RtRegion& reg, long mine) {
    const int tiles_x = std::max((reg.width + kTile - 1) / kTile, 1);
    long n = 0;
    for (long k = 0; k < mine; ++k) {
        const long t = reg.tile_group + k * reg.tile_groups;
        const int tx = (int)(t % tiles_x), ty = (int)(t / tiles_x);
        n += (long)std::min(kTile, reg.width - tx * kTile) * std::min(kTile, reg.height - ty * kTile);
    }
    return n;
}

LaunchPlan plan_launch(const CamHost& host, const SceneBlob& blob, int cus, int lds_max, const rt_region& region,
                       int tile_group, int tile_groups, int prec, int trav, int count, int prog_len, bool have_ptab,
                       bool px_bounces) {
    const SceneBuild& build = host.build;
    const RtCamera& C = build.cam;
    const int32_t lds_words = blob.lds_words, lds_words2 = blob.lds_words2;
    if (tile_groups < 1 || tile_group < 0 || tile_group >= tile_groups)
        throw std::invalid_argument("tile_group must satisfy 0 <= tile_group < tile_groups");
    LaunchPlan plan;
    RtRegion& reg = plan.reg;
    reg = RtRegion{region.x, region.y, region.width, region.height, tile_group, tile_groups};
    const int tiles_x = (reg.width + kTile - 1) / kTile;
    const int tiles_y = (reg.height + kTile - 1) / kTile;
    const long total = (long)tiles_x * tiles_y;
    const long mine = total > tile_group ? (total - tile_group + tile_groups - 1) / tile_groups : 0;
    LaunchGeom& g = plan.g;
    g.tiles_x = std::max(tiles_x, 1);
    g.my_tiles = (int)mine;
    const long want = (mine + (kBlock / kWave) - 1) / (kBlock / kWave);
    g.grid = (int)std::max<long>(1, std::min<long>(want, (long)cus));  // one persistent workgroup per CU
    KernelVariant& v = plan.v;
    v = KernelVariant{C.emissive_scatter != 0, count, host.effective_traversal(trav)};
    const size_t stack0 = stack_lds_bytes(C.stack_depth, v.trav, C.n_prims);        // tree in global memory
    const size_t stack1 = stack_lds_bytes(C.stack_depth, v.trav, C.n_prims, true);  // LDS-resident tree
    // LDS-resident scene: the BVH walk's data and the primitive records
    // (level 1), plus the material and light tables when they fit too
    // (level 2). The brute-force loop reads its wave-uniform primitive
    // records through scalar loads either way; LDS serves the per-lane
    // reads (hit record, materials, light sampling).
    const size_t lds_cap = (size_t)std::min(lds_max, kLdsSceneMaxBytes);
    // the LDS copy pads every 4-wide node to 144 bytes (pt_walk.hpp t4_node: LDS bank windows)
    const int32_t node_pad =
        v.trav == TRAV_FAST && env_flag("RT_AMD_NODE_PAD", true) ? (int32_t)build.t4nodes.size() : 0;
    g.lds_level = 0;
    if (lds_scene_enabled() && v.trav != TRAV_REFERENCE) {
        if (stack1 + (size_t)(lds_words2 + node_pad) * 16 <= lds_cap && env_flag("RT_AMD_LDS_MATS", true))
            g.lds_level = 2;
        else if (v.trav == TRAV_FAST && stack1 + (size_t)(lds_words + node_pad) * 16 <= lds_cap)
            g.lds_level = 1;
    }
    // (16-bit stack entries hold node references < 2^15 and leaf codes ~(first << 3 | count) with
    // first < 2^12: always so for a tree that fits the LDS copy; checked)
    if (g.lds_level > 0 && v.trav == TRAV_FAST &&
        (build.t4nodes.size() >= (1u << 15) || build.tprims.size() >= (1u << 12)))
        g.lds_level = 0;
    const size_t stack = g.lds_level > 0 ? stack1 : stack0;
    g.lds_bytes = stack + (g.lds_level == 0 ? 0 : (size_t)((g.lds_level == 2 ? lds_words2 : lds_words) + node_pad) * 16);
    // a tree walked from global memory: its top (breadth-first prefix) in the LDS left beside the stack
    int32_t n_top = 0;
    // (round 5 also walked 8-bit quantised 64-byte nodes here, twice the nodes in the cache:
    // 2 % slower, the decode costing more than the halved loads; profiles/r05/qnodes/)
    const size_t node_lds = sizeof(RtT4Node) + 16;
    if (g.lds_level == 0 && v.trav == TRAV_FAST && lds_scene_enabled() && env_flag("RT_AMD_TOP_CACHE", true)) {
        const size_t room = lds_cap > stack ? lds_cap - stack : 0;
        n_top = (int32_t)std::min<size_t>(build.t4nodes.size(), room / node_lds);
        g.lds_bytes = stack + (size_t)n_top * node_lds;
    }
    // Deferred exact sphere tests pay where the walk is VALU-bound and leaves hold
    // several candidates: LDS-resident trees of >= 100 primitives (spheres-500
    // +4.7 %); tiny trees have ~1 candidate per ray (rain-50 -1.3 %) and trees
    // walked from global memory are bound by node fetches (spheres-100k -2.3 %;
    // profiles/r02/defer/). RT_AMD_DEFER=0/1 overrides.
    v.defer = v.trav == TRAV_FAST &&
              env_flag("RT_AMD_DEFER", g.lds_level >= 1 && C.n_prims >= 100);
    if (g.lds_bytes + static_lds_bytes(count, false) > (size_t)lds_max)
        throw std::runtime_error("traversal stack exceeds the workgroup LDS (BVH too deep)");
    if (env_flag("RT_AMD_LAUNCH_LOG", false))
        std::fprintf(stderr,
                     "[rt launch] prims %d stack_depth %d trav %d lds_level %d lds %zu B (stack %zu, scene L1 %d / "
                     "L2 %d B) lds_max %d tiles %ld\n",
                     C.n_prims, C.stack_depth, v.trav, g.lds_level, g.lds_bytes, stack, lds_words * 16,
                     lds_words2 * 16, lds_max, mine);
    plan.stack = stack;
    plan.node_pad = g.lds_level > 0 ? node_pad : 0;
    plan.n_top = n_top;
    if (mine == 0) return plan;
    // Fixed spp: the chunked / pool kernels (per-sample records, in-order accumulate)
    // at every size. Round 1 kept the sequential kernel for images of >= 4 tiles per
    // resident wave; with the hand-out rules above the chunked kernel is faster there
    // too (rain-50 1080p spp512: 50.7 -> 44.1 ms, profiles/r02/sched/), records and all.
    const bool chunked = env_flag("RT_AMD_CHUNKED", true);
    // Adaptive sampling runs in rounds on the chunked / pool kernels (pt_adapt_kernel
    // settles each round in sample order); RT_AMD_ADAPT_ROUNDS=0 keeps the sequential kernel.
    // Instrumented launches (count == 1) keep the sequential kernel: a round renders samples
    // past a pixel's convergence, and the work counters would count them.
    const bool rounds = C.adaptive && count != 1 && env_flag("RT_AMD_ADAPT_ROUNDS", true);
    plan.rounds = rounds;
    // sequential-pixel kernel (pixelConverged needs each pixel's samples in one place)
    // aTolerance NaN is not adaptive sampling (NaN > 0 fails, camera.ts:165), but pixelConverged's
    // own guard (NaN <= 0, camera.ts:350) fails as well and the illuminance sums stay 0: the variance
    // is 0 and every pixel "converges" at the first multiple of aBatch. Only the sequential kernel
    // asks pixelConverged after every sample.
    const bool nan_tolerance = std::isnan(C.a_tolerance) && C.samples > 1.0;
    plan.sequential = prog_len <= 0 && (C.n_samples <= 0 || !chunked || (C.adaptive && !rounds) || nan_tolerance);
    if (plan.sequential) return plan;

    // Stage-compacted pool kernel (pt_pool_kernel): possible for product brute-force
    // launches without an emission stack whose per-wave path pools fit in LDS beside
    // the scene; the default in both precisions since its diffuse and trace queues are
    // split by branch (Cornell 800^2 spp256 ref 16.82 ms vs chunked ~18.9 ms; fp32
    // 14.12 vs 14.23 ms, profiles/r02/asplit/). RT_AMD_POOL_KERNEL=0/1 overrides.
    plan.lds_pool_off = (int32_t)((g.lds_bytes + 15) / 16 * 16);
    const bool pool_ok = !v.emit && (count == 0 || (RT_POOL_PROF && count == 2 && prec == PREC_REF)) && v.trav == TRAV_BRUTE && C.width < 65536 && C.height < 65536 &&
             C.n_samples <= 65535 && C.depth <= 250 && build.mats.size() < (1u << 21) &&  // 56-byte slot fields
             build.prims.size() < (1u << 14) &&
             (size_t)plan.lds_pool_off + pool_lds_bytes() + static_lds_bytes(count, true) <= (size_t)lds_max &&
             env_flag("RT_AMD_POOL_KERNEL", true);
    // The primary-ray candidate table (primary.hpp) for the pool kernel's new-path trips:
    // built once the camera renders enough samples per pixel to repay the builder kernel
    // (kPrimaryMinSamples), used whenever it exists. RT_AMD_PRIMARY_TABLE=0 keeps every launch
    // on the pre-filter pass, =1 uses the table at any sample count (A/B and the tests).
    const int primary_env = env_int0("RT_AMD_PRIMARY_TABLE", -1);
    const bool primary_ok = pool_ok && host.primary_table_ok(trav) &&
                            (primary_env > 0 || (primary_env < 0 && kPrimaryDefault &&
                                                 (have_ptab || C.n_samples >= kPrimaryMinSamples)));
    plan.pool_ok = pool_ok;
    plan.primary_ok = primary_ok;
    // fixed spp: 12-byte records where no pixel's bounce count is an output (SampleBuf::rec12)
    plan.rec12 = prog_len <= 0 && !rounds && C.mode != MODE_BOUNCES && !px_bounces && env_flag("RT_AMD_REC12", true);
    return plan;
}

// guided schedule of `nsamp` samples over `slots` pixel slots: half of the remaining
// samples per phase, chunks halving. First-phase chunk from the samples per resident
// lane: an item is the critical path of its pixel, so small per-launch workloads (a
// rank's share of the image, small images) or a few very expensive pixels (rays
// grazing a field of spheres) need short items, while large ones amortise the
// hand-out over long items (tools/tail_probe.py sweep).
bool guided_schedule(const LaunchPlan& plan, double slots, int nsamp, bool rounds, int cus, SampleBuf& sb) {
    const KernelVariant& v = plan.v;
    const LaunchGeom& g = plan.g;
    bool pool = plan.pool_ok;
    // spl: samples per resident lane of this launch.
    const double spl = slots * (double)nsamp / ((double)cus * kBlockChunk);
    // Brute-force scenes in the chunked kernel: two tile-chunks per atomic from 512 spl
    // and first items of spl / 8 (round 1, profiles/r01/sweep_b/).
    // The pool kernel (96 path slots per wave, any slot takes any item) wants wider takes
    // and shorter first items: 4 tile-chunks per atomic from 256 samples per resident
    // lane, 2 from 128, and first items of at most 8 samples (Cornell 800^2 spp256:
    // N=1 16.84 -> 16.63 ms, a rank's 1/2 share 9.18 -> 8.43 ms; tools/sched_sweep.py,
    // profiles/r02/sched/).
    // LDS-resident BVH scenes in the chunked kernel (resumable walks): 4 tile-chunks per
    // atomic from 256 samples per resident lane (2 below) and a first chunk of the
    // power-of-two floor of sqrt(spl) / 3 (spheres-500 800^2 spp64: N=1 6.62 -> 6.26 ms,
    // rank shares N=2 3.54 -> 3.27, N=4 2.04 -> 1.78, N=8 1.21 -> 1.03 ms; rain-50 1080p
    // spp512 rank shares N=2 31.5 -> 22.2 ms, N=8 7.8 -> 5.8 ms; profiles/r02/sched/).
    // Trees walked from global memory (a sample costs ~150 us of a lane at config 5) cap
    // the first chunk at 4 (config 5, 4096^2 spp1024: 9617 -> 8980 ms per frame; 2 since round 4).
    const bool bvh = v.trav == TRAV_FAST;
    // (pool kernel, re-tuned at 152 slots per wave: 8 tile-chunks per atomic from 512 spl,
    // 4 from 48, 2 from 24, first items of at most 4 samples - Cornell N=1 14.61 -> 14.43 ms,
    // 1/2 share 7.57 -> 7.40, 1/8 share 2.57 -> 2.10 ms; profiles/r02/sched/)
    // (trees walked from global memory, round 4: 8 tile-chunks per atomic from 1024 spl,
    // chunks of at most 2 samples and shading from 40 walks done, not 48 - config 5's 1/8
    // share 1070.8 -> 1045.0 ms, spheres-100k 4096^2 spp16 N=1 134.9 -> 131.4 ms;
    // profiles/r04/cfg5/)
    const bool gtree = bvh && g.lds_level == 0;
    const int pool_auto = pool ? (spl >= 512.0 ? 8 : spl >= 48.0 ? 4 : spl >= 24.0 ? 2 : 1)
                         : bvh ? (gtree && spl >= 1024.0 ? 8 : spl >= 256.0 ? 4 : 2)
                               : (v.trav == TRAV_BRUTE && spl >= 512.0 ? 2 : 1);
    sb.pool = kWave * env_int("RT_AMD_POOL", pool_auto);
    const int c_max = pool ? 4 : gtree ? 2 : 32;
    // (pool kernel, fixed spp, re-checked at the round-3 build: first items of spl / 64, so 4
    // samples for the whole frame and a 1/2 share, 2 for a 1/4 share, 1 for a 1/8 share -
    // Cornell 1/8 share 2.248 -> 2.051 ms, 1/4 3.998 -> 3.931 ms, N=1 and 1/2 unchanged;
    // profiles/r03/sched/. Adaptive rounds keep spl / 8.)
    const double c_target = bvh ? std::sqrt(spl) / 3.0 : (pool && !rounds) ? spl / 64.0 : spl / 8.0;
    int c_auto = 1;
    while (c_auto * 2 <= c_max && c_auto * 2 <= c_target) c_auto *= 2;  // pow2 floor, in [1, c_max]
    // power-of-two chunks: items are aligned to their chunk (the pool kernel derives an
    // item's end from its sample index)
    auto pow2floor = [](int x) { int p = 1; while (p * 2 <= x) p *= 2; return p; };
    int s0 = 0, c = pow2floor(std::min(env_int("RT_AMD_CHUNK", c_auto), std::max(1, nsamp / 2))), np = 0;
    if (!env_flag("RT_AMD_GUIDED", true)) {  // uniform chunks (A/B)
        c = pow2floor(std::max(1, std::min(env_int("RT_AMD_CHUNK", c_auto), nsamp)));
        const int full = nsamp / c;
        sb.s0[np] = 0; sb.chunk[np] = c; sb.nch[np] = full; ++np;
        s0 = full * c;
    }
    while (s0 < nsamp) {
        const int rem = nsamp - s0;
        if (c <= 1 || np == kMaxPhases - 1) {  // final phase: 1-sample items
            sb.s0[np] = s0; sb.chunk[np] = 1; sb.nch[np] = rem;
            ++np;
            break;
        }
        const int span = (rem / 2) / c * c;
        if (span == 0) { c /= 2; continue; }
        sb.s0[np] = s0; sb.chunk[np] = c; sb.nch[np] = span / c;
        ++np;
        s0 += span;
        c /= 2;
    }
    sb.n_phases = np;
    // the pool kernel keeps log2(item chunk) in a 3-bit slot field (pool_meta): chunks
    // of more than kPoolMaxChunk samples (RT_AMD_CHUNK overrides) take the chunked kernel
    for (int p = 0; p < np; ++p)
        if (sb.chunk[p] > kPoolMaxChunk) pool = false;
    int covered = 0;
    for (int p = 0; p < np; ++p) {
        if (sb.s0[p] != covered) throw std::runtime_error("guided schedule: gap");
        covered += sb.chunk[p] * sb.nch[p];
    }
    if (covered != nsamp) throw std::runtime_error("guided schedule: coverage");
    for (int p = 0; p < np; ++p) sb.rnch[p] = 1.0 / (double)sb.nch[p];
    sb.refill_min = std::min(env_int("RT_AMD_REFILL", 4), kWave);
    sb.min_ready = std::min(env_int("RT_AMD_READY", gtree ? 40 : 48), kWave);
    return pool;
}

}  // namespace rt
