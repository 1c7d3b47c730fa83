// What one render launches, decided on the host before anything is queued: the kernel variant,
// LDS residency, the pool and primary-table gates (plan_launch), the guided hand-out schedule
// of a pass loop (guided_schedule) and the pass sizing. No HIP runtime call in this unit:
// dev_ctx.cpp executes a plan, rt_debug_launch_plan reports one.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/rt_amd.h"
#include "launch.hpp"
#include "scene_blob.hpp"

namespace rt {

struct CamHost;  // dev_ctx.hpp

// Samples per pixel from which a launch builds the primary-ray candidate table (an existing
// table is used at any count): the measured break-even of a fresh camera's first render,
// rounded up to a power of two. Cornell 800x800 on MI355X: the builder kernel takes 0.060 ms
// and the first render 0.08 ms more than without the table (allocation and events included);
// the table saves 0.032 ms of a 16-sample frame and 1.30 ms of a 256-sample one, so the first
// render breaks even at ~25 samples per pixel.
constexpr int kPrimaryMinSamples = 32;
constexpr bool kPrimaryDefault = true;  // RT_AMD_PRIMARY_TABLE unset

// Pass sizing of the chunked / pool kernels. A pass hands out its items through one int32
// counter (take_pool), which may overshoot the item count by 2 x grid waves x pool before the
// last wave sees it exhausted: items must stay below kItemCap. A pass of `units` groups of
// `unit_slots` pixel slots numbers ceil64(units * unit_slots) x chunks_per_slot items
// (chunks_per_slot = the schedule's sum of nch: one item per (slot, chunk)). So each pass is
// the smallest of: the units left, the record budget, and the counter headroom - a larger
// record budget gives fewer, bounded passes instead of an error.
constexpr long kItemCap = (1l << 31) - (1l << 22);
long pass_units(long units_left, long unit_slots, long chunks_per_slot, size_t rec_bytes_per_unit, size_t budget);
long chunks_per_slot(const SampleBuf& sb);
size_t sbuf_budget();  // RT_AMD_SBUF_MB
// Slots per pass of a round or step over n_act active slots with `len` 16-byte records each:
// whole 64-slot groups (items are numbered per group of 64 slots).
long record_pass_slots(long n_act, const SampleBuf& sb, int len);
// The first round of an adaptive launch: whole convergence batches (RT_AMD_ADAPT_FIRST).
int adaptive_first_len(const RtCamera& C);
// Record bytes of one 64-slot tile of a fixed-spp launch.
size_t fixed_rec_bytes_per_tile(const RtCamera& C, bool rec12);
// Numbers the items of a pass over sb.slots slots phase by phase (sb.item_base, sb.n_items) and
// returns the path kernel's grid for it.
int number_pass_items(SampleBuf& sb, bool pool, int cus);

// Pixels inside the region among the `mine` tiles this launch owns (tile t of the region is
// owned iff t % tile_groups == tile_group, as the kernels' item_pixel maps them).
long region_pixels(const RtRegion& reg, long mine);

struct LaunchPlan {
    RtRegion reg;
    LaunchGeom g;           // g.my_tiles == 0: nothing to render
    size_t stack = 0;       // traversal stack bytes
    int32_t node_pad = 0;   // LDS-resident trees: the padded nodes (0 otherwise)
    int32_t n_top = 0;      // trees walked from global memory: nodes of the cached top
    int32_t lds_pool_off = 0;
    KernelVariant v;        // (ptab: set per pass by the executing side)
    bool sequential = false;  // the sequential-pixel kernel, one pass
    bool rounds = false;      // adaptive sampling in rounds
    bool pool_ok = false, primary_ok = false;
    bool rec12 = false;       // fixed spp: 12-byte records
};

// Throws std::invalid_argument for a bad tile group, std::runtime_error where the traversal
// stack does not fit. `region`: clamped to the image. have_ptab: the context has built the
// primary-ray table; px_bounces: the launch writes per-pixel bounce counts.
LaunchPlan plan_launch(const CamHost& host, const SceneBlob& blob, int cus, int lds_max, const rt_region& region,
                       int tile_group, int tile_groups, int prec, int trav, int count, int prog_len, bool have_ptab,
                       bool px_bounces);

// Guided schedule of `nsamp` samples over `slots` pixel slots into sb's schedule fields.
// Returns whether the passes run the pool kernel (plan.pool_ok, unless a chunk exceeds
// kPoolMaxChunk).
bool guided_schedule(const LaunchPlan& plan, double slots, int nsamp, bool rounds, int cus, SampleBuf& sb);

}  // namespace rt
