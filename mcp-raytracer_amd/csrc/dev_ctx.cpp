// Device contexts of a camera (dev_ctx.hpp): upload, buffers, and the executing half of a
// launch - the passes of a LaunchPlan on a stream.
#include "dev_ctx.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <stdexcept>

#include "coverage.hpp"
#include "pass_host.hpp"
#include "prog_blob.hpp"

namespace rt {

static_assert(kProgPixBytes == sizeof(ProgPix) && kProgTile == kTile && kProgWave == kWave,
              "prog_blob.hpp restates the session record's size and the tile shape");

DevCtx::~DevCtx() {
    release();
    DeviceScope scope;
    (void)hipSetDevice(device);
    d_slab.reset();
    d_rslab.reset();
    d_gather.reset();
    d_rgather.reset();
    if (h_words) (void)hipHostFree(h_words);
    for (hipEvent_t e : {ev_rendered, ev_gather0, ev_gather1})
        if (e) (void)hipEventDestroy(e);
    if (stream) (void)hipStreamDestroy(stream);
}

void DevCtx::ensure_multi(size_t slab_bytes, size_t rslab_bytes, bool root, int n) {
    if (!stream) hip_check(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking), "hipStreamCreate");
    for (hipEvent_t* e : {&ev_rendered, &ev_gather0, &ev_gather1})
        if (!*e) hip_check(hipEventCreate(e), "hipEventCreate");
    d_slab.ensure(slab_bytes, "hipMalloc(slab)");
    if (rslab_bytes) d_rslab.ensure(rslab_bytes / sizeof(float), "hipMalloc(radiance slab)");
    if (!root) return;
    d_gather.ensure(slab_bytes * n, "hipMalloc(gathered slabs)");
    if (rslab_bytes) d_rgather.ensure(rslab_bytes / sizeof(float) * n, "hipMalloc(gathered radiance)");
    if (h_words_cap < n) {
        if (h_words) (void)hipHostFree(h_words);
        h_words = nullptr;
        h_words_cap = 0;
        hip_check(hipHostMalloc((void**)&h_words, (size_t)n * ST_WORDS * sizeof(unsigned long long), 0),
                  "hipHostMalloc");
        h_words_cap = n;
    }
}

void DevCtx::release() {
    if (!live) return;
    DeviceScope scope;
    (void)hipSetDevice(device);
    // every buffer is reset: a later ensure_device / ensure_frame / launch (possibly on
    // another device) must reallocate all of them
    d_blob.reset();
    d_stats.reset();
    d_counters.reset();
    d_tile.reset();
    d_rgb.reset();
    d_rad.reset();
    d_sbuf.reset();
    d_ptab.reset();
    for (hipEvent_t& e : ptab_ev)
        if (e) (void)hipEventDestroy(e), e = nullptr;
    ptab_used = false;
    d_astate.reset();
    d_act[0].reset();
    d_act[1].reset();
    prog_free();
    dn.free();
    d_prim_object.reset();
    for (hipEvent_t& e : dn_ev)
        if (e) (void)hipEventDestroy(e), e = nullptr;
    dn_ev.clear();
    dn_levels = 0;
    d_cov.reset();
    d_hold.reset();
    for (hipEvent_t& e : cov_ev)
        if (e) (void)hipEventDestroy(e), e = nullptr;
    cov_timed = false;
    rp_prev.free();
    d_reusable.reset();
    for (hipEvent_t& e : rp_ev)
        if (e) (void)hipEventDestroy(e), e = nullptr;
    rp_ev.clear();
    rp_timed = false;
    rs.free();
    rs_prev.free();
    d_through.reset();
    through_mask = -1;
    d_acount.reset();
    if (h_acount) (void)hipHostFree(h_acount);
    h_acount = nullptr;
    for (hipEvent_t& e : ev)
        if (e) (void)hipEventDestroy(e), e = nullptr;
    ev.clear();
    n_passes = 0;
    if (order_ev) (void)hipEventDestroy(order_ev);
    order_ev = nullptr;
    order_pending = false;
    live = false;
}

void DevCtx::ensure_device() {
    int dev = 0;
    hip_check(hipGetDevice(&dev), "hipGetDevice");
    if (dev != device) throw std::logic_error("device context used on another device");
    if (live) return;
    blob = build_scene_blob(build);
    d_blob.ensure((blob.size + sizeof(uint4) - 1) / sizeof(uint4), "hipMalloc");
    if (blob.size) hip_check(hipMemcpy(d_blob, blob.bytes.data(), blob.size, hipMemcpyHostToDevice), "hipMemcpy");
    blob.bytes = std::vector<char>();
    d_stats.ensure(ST_WORDS * kStatStride, "hipMalloc");
    d_counters.ensure(kCounterWords, "hipMalloc");
    d_tile.ensure(16, "hipMalloc");
    live = true;
    cus = device_cus(dev);
    int smem = 0;
    if (hipDeviceGetAttribute(&smem, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) == hipSuccess && smem > 0)
        lds_max = smem;
}

void DevCtx::ensure_frame() {
    if (d_rgb) return;
    const size_t px = (size_t)build.cam.width * build.cam.height;
    d_rgb.ensure(px * 3, "hipMalloc");
    d_rad.ensure(px * 3, "hipMalloc");
}

hipEvent_t DevCtx::pass_event(int p, int k) {
    while ((int)ev.size() < 3 * (p + 1)) {
        hipEvent_t e = nullptr;
        hip_check(hipEventCreate(&e), "hipEventCreate");
        ev.push_back(e);
    }
    return ev[3 * p + k];
}

void DevCtx::times(float* path_ms, float* accum_ms) {
    *path_ms = 0.0f;
    *accum_ms = 0.0f;
    for (int p = 0; p < n_passes; ++p) {
        float a = 0.0f, b = 0.0f;
        hip_check(hipEventSynchronize(ev[3 * p + 1]), "hipEventSynchronize");
        hip_check(hipEventElapsedTime(&a, ev[3 * p], ev[3 * p + 1]), "hipEventElapsedTime");
        *path_ms += a;
        if (ev_accum) {
            hip_check(hipEventSynchronize(ev[3 * p + 2]), "hipEventSynchronize");
            hip_check(hipEventElapsedTime(&b, ev[3 * p + 1], ev[3 * p + 2]), "hipEventElapsedTime");
            *accum_ms += b;
        }
    }
}

DevScene DevCtx::dev_scene() const {
    DevScene S;
    const char* b = reinterpret_cast<const char*>(d_blob.p);
    S.t4nodes = reinterpret_cast<const RtT4Node*>(b);
    S.prims = reinterpret_cast<const RtPrim*>(b + blob.off_prims);
    S.gprims = S.prims;
    S.gpre = reinterpret_cast<const RtPre*>(b + blob.off_pre);
    S.n_pre = blob.n_pre;
    S.xrec = reinterpret_cast<const RtExact*>(b + blob.off_xrec);
    S.off_xrec = blob.off_xrec;
    S.tprims = reinterpret_cast<const int32_t*>(b + blob.off_tprims);
    S.off_tprims = blob.off_tprims;
    S.tsph = reinterpret_cast<const float4*>(b + blob.off_tsph);
    S.off_tsph = blob.off_tsph;
    S.mats = reinterpret_cast<const RtMat*>(b + blob.off_mats);
    S.lights = reinterpret_cast<const RtLight*>(b + blob.off_lights);
    S.glights = S.lights;
    S.nodes = reinterpret_cast<const RtNode*>(b + blob.off_nodes);
    S.onbs = reinterpret_cast<const RtOnb*>(b + blob.off_onbs);
    S.n_onb = blob.n_onb;
    S.off_onbs = blob.off_onbs;
    S.blob = d_blob;
    S.tsph2 = nullptr;  // (set per launch: trees walked from global memory)
    S.lds_words = blob.lds_words;
    S.off_prims = blob.off_prims;
    S.off_mats = blob.off_mats;
    S.off_lights = blob.off_lights;
    S.lds_stack_bytes = 0;
    S.lds_pool_off = 0;
    S.lds_node_pad = 0;  // set per launch when the scene is LDS-resident
    S.t4_stride = (int32_t)sizeof(RtT4Node);
    S.n_top = 0;         // set per launch when the tree is walked from global memory
    S.top_lds = nullptr;
    S.nearfar = 0;       // (scene_view sets it per LDS level)
    S.t4root = build.t4root;
    S.root_box = build.t4root_box;
    S.cam = build.cam;
    S.mix_total = host.mix_total;
    S.light_w = host.light_w;
    return S;
}

const uint2* DevCtx::ensure_primary_table(hipStream_t stream) {
    if (!d_ptab) {
        const RtCamera& C = build.cam;
        const size_t n = (size_t)C.width * (size_t)C.height;
        d_ptab.ensure(n, "hipMalloc(primary table)");
        for (hipEvent_t& e : ptab_ev)
            if (!e) hip_check(hipEventCreate(&e), "hipEventCreate");
        hip_check(hipEventRecord(ptab_ev[0], stream), "hipEventRecord");
        hip_check(launch_primary_table(C, reinterpret_cast<const RtPrim*>(reinterpret_cast<const char*>(d_blob.p) + blob.off_prims),
                                       C.n_prims, d_ptab, stream),
                  "primary_table_kernel launch");
        hip_check(hipEventRecord(ptab_ev[1], stream), "hipEventRecord");
    } else {
        hip_check(hipStreamWaitEvent(stream, ptab_ev[1], 0), "hipStreamWaitEvent");
    }
    return reinterpret_cast<const uint2*>(d_ptab.p);
}

void DevCtx::order_after(hipStream_t stream) {
    if (order_pending && order_key != reinterpret_cast<uintptr_t>(stream))
        hip_check(hipStreamWaitEvent(stream, order_ev, 0), "hipStreamWaitEvent");
}

void DevCtx::order_mark(hipStream_t stream, bool check) {
    hipError_t e = hipSuccess;
    if (!order_ev) e = hipEventCreateWithFlags(&order_ev, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(order_ev, stream);
    if (e == hipSuccess) {
        order_key = reinterpret_cast<uintptr_t>(stream);
        order_pending = true;
    }
    if (check) hip_check(e, "hipEventRecord(order)");
}

float DevCtx::primary_table_ms() {
    float ms = 0.0f;
    if (d_ptab && ptab_ev[1]) {
        hip_check(hipEventSynchronize(ptab_ev[1]), "hipEventSynchronize");
        hip_check(hipEventElapsedTime(&ms, ptab_ev[0], ptab_ev[1]), "hipEventElapsedTime");
    }
    return ms;
}

struct DevCtx::LaunchRun {
    const LaunchPlan& plan;
    KernelVariant v;  // plan.v with the pass loop's pool decision and table
    DevScene S;
    RenderOut out;
    int prec;
    hipStream_t stream;
    SampleBuf sb{};
    int pass = 0;
};

void DevCtx::launch(const rt_region& region, int tile_group, int tile_groups, int prec, int trav, int count,
                    uint8_t* rgb, float* rad, int32_t* pxs, int32_t* pxb, int packed, hipStream_t stream,
                    const ProgStep* step) {
    const RtCamera& C = build.cam;
    const int prog_len = step ? step->len : 0;
    const LaunchPlan plan = plan_launch(host, blob, cus, lds_max, clamp_region(region, C.width, C.height), tile_group,
                                        tile_groups, prec, trav, count, prog_len, d_ptab.p != nullptr, pxb != nullptr);
    const LaunchGeom& g = plan.g;
    RenderOut out{rgb, rad, pxs, pxb, d_stats, d_counters, d_tile, packed ? 1 : 0};
    hip_check(launch_init_stats(d_stats, count ? d_counters.p : nullptr, d_tile, stream), "init_stats");
    n_passes = 0;
    last_kernel = RT_KERNEL_NONE;
    ptab_used = false;
    adapt_rounds = 0;
    adapt_rendered = 0;
    if (g.my_tiles == 0) return;
    LaunchRun r{plan, plan.v, dev_scene(), out, prec, stream};
    DevScene& S = r.S;
    S.lds_stack_bytes = (int32_t)plan.stack;
    S.lds_words = g.lds_level == 2 ? blob.lds_words2 : blob.lds_words;
    S.lds_node_pad = plan.node_pad;
    S.n_top = plan.n_top;
    // trees walked from global memory: leaf records that carry the exact test's fp64 radius
    // (the LDSS-0 chunked kernels read them, pt_walk.hpp leaf_test L2)
    S.tsph2 = blob.off_tsph2 >= 0 ? reinterpret_cast<const RtLeafSph*>(reinterpret_cast<const char*>(d_blob.p) + blob.off_tsph2)
                                  : nullptr;
    if (g.lds_level == 0 && r.v.trav == TRAV_FAST && !S.tsph2 && C.n_prims > 0)
        throw std::runtime_error("fast traversal without leaf records");
    if (plan.sequential) {
        hip_check(hipEventRecord(pass_event(0, 0), stream), "hipEventRecord");
        hipError_t e = prec == PREC_FP32 ? launch_render_fp32(r.v, S, plan.reg, out, g, nullptr, stream)
                                         : launch_render_ref(r.v, S, plan.reg, out, g, nullptr, stream);
        hip_check(e, "pt_render_kernel launch");
        hip_check(hipEventRecord(pass_event(0, 1), stream), "hipEventRecord");
        n_passes = 1;
        ev_accum = false;
        last_kernel = RT_KERNEL_SEQUENTIAL;
        return;
    }
    S.lds_pool_off = plan.lds_pool_off;
    if (prog_len > 0) launch_progressive(r, *step);
    else if (plan.rounds) launch_adaptive_rounds(r);
    else launch_fixed(r);
    n_passes = r.pass;
    ev_accum = true;
    last_kernel = r.v.pool ? RT_KERNEL_POOL : RT_KERNEL_CHUNKED;
}

// one pass of the path kernel over sb.slots slots (items numbered phase by phase)
void DevCtx::run_pass(LaunchRun& r, bool first) {
    const hipStream_t stream = r.stream;
    LaunchGeom gp = r.plan.g;
    gp.grid = number_pass_items(r.sb, r.v.pool, cus);
    if (!first) hip_check(hipMemsetAsync(d_tile, 0, 2 * sizeof(unsigned int), stream), "hipMemsetAsync");
    if (r.v.pool) gp.lds_bytes = (size_t)r.S.lds_pool_off + pool_lds_bytes();
    r.v.ptab = nullptr;
    if (r.v.pool && r.plan.primary_ok) {  // pt_pool_primary_kernel
        r.v.ptab = ensure_primary_table(stream);
        ptab_used = true;
    }
    // per-pass events: path kernel [0, 1), accumulate [1, 2)
    hip_check(hipEventRecord(pass_event(r.pass, 0), stream), "hipEventRecord");
    hipError_t e = r.prec == PREC_FP32 ? launch_render_fp32(r.v, r.S, r.plan.reg, r.out, gp, &r.sb, stream)
                                       : launch_render_ref(r.v, r.S, r.plan.reg, r.out, gp, &r.sb, stream);
    hip_check(e, "pt_chunk_kernel launch");
    hip_check(hipEventRecord(pass_event(r.pass, 1), stream), "hipEventRecord");
}

// fixed spp: passes over at most sbuf_budget bytes of per-sample records
void DevCtx::launch_fixed(LaunchRun& r) {
    const RtCamera& C = build.cam;
    SampleBuf& sb = r.sb;
    int& pass = r.pass;
    const long mine = r.plan.g.my_tiles;
    sb.rec12 = r.plan.rec12;
    const size_t rec_per_tile = fixed_rec_bytes_per_tile(C, r.plan.rec12);
    r.v.pool = guided_schedule(r.plan, (double)mine * kWave, C.n_samples, r.plan.rounds, cus, sb);
    const long pass_tiles = pass_units(mine, kWave, chunks_per_slot(sb), rec_per_tile, sbuf_budget());
    sb.rec = sample_records((size_t)pass_tiles * rec_per_tile);
    for (long t0 = 0; t0 < mine; t0 += pass_tiles, ++pass) {
        const long nt = std::min(pass_tiles, mine - t0);
        sb.tile0 = (int32_t)t0;
        sb.slots = (int32_t)(nt * kWave);
        // record layout: sample-major (default) or slot-major (RT_AMD_REC_SLOT_MAJOR=1, A/B)
        if (env_flag("RT_AMD_REC_SLOT_MAJOR", false)) {
            sb.stride_s = 1;
            sb.stride_slot = C.n_samples;
        } else {
            sb.stride_s = sb.slots;
            sb.stride_slot = 1;
        }
        run_pass(r, t0 == 0);
        hip_check(launch_accum(r.S, r.plan.reg, r.out, r.plan.g.tiles_x, sb, r.stream), "pt_accum_kernel launch");
        hip_check(hipEventRecord(pass_event(pass, 2), r.stream), "hipEventRecord");
    }
}

// Adaptive sampling in rounds (src/camera.ts:400-425). Round r renders samples
// [s_base, s_base + len) of every pixel still sampling - speculatively, since a pixel
// may converge inside the round - on the chunked / pool kernels; pt_adapt_kernel then
// adds them to each pixel's running PixelStats in sample order with the reference's
// convergence check after every sample, finishes converged / complete pixels and
// compacts the rest into the next round's active list. Rounds double in length from
// two convergence batches (aBatch) so a pixel renders at most one round past its
// convergence; the pixel count of each round comes back to the host (one small copy).
void DevCtx::launch_adaptive_rounds(LaunchRun& r) {
    const RtCamera& C = build.cam;
    const RtRegion& reg = r.plan.reg;
    const hipStream_t stream = r.stream;
    SampleBuf& sb = r.sb;
    int& pass = r.pass;
    const long mine = r.plan.g.my_tiles;
    const long slots_all = mine * kWave;
    ensure_adapt((size_t)slots_all);
    int len = adaptive_first_len(C);
    const int grow = env_int("RT_AMD_ADAPT_GROW", 3);
    // after a round that retired fewer than RT_AMD_ADAPT_JUMP per mille of its pixels, the rest
    // are taken to run long and the next round renders every remaining sample: Cornell (pixels
    // converge at the first check or run to spp) 15.17 -> 14.86 ms with 3 rounds; spheres-500 and
    // rain unchanged at 100; 200 cost rain 47 % (profiles/r03/exp2/)
    const int jump = env_int0("RT_AMD_ADAPT_JUMP", 100);
    // ... or after a round whose carried pixels are mostly not expected to converge within the
    // next (grown) round: fewer than RT_AMD_ADAPT_LIKELY per mille of them have a confidence
    // interval that would close by then at their current mean and variance (pt_adapt_kernel).
    // Cornell's pixels converge at the first checks or never: 474 of 530,755 carried after round
    // 1 are likely, so it runs in 2 rounds instead of 3 (14.79 -> 14.45 ms); rain's 20 % and
    // spheres-500's 11 % keep their rounds; the default scene 13.09 -> 12.96 ms path kernel
    // (profiles/r05/adaptive_likely/). 0 turns the rule off.
    const int likely_pm = env_int0("RT_AMD_ADAPT_LIKELY", 100);
    const bool trace = env_flag("RT_AMD_ADAPT_LOG", false);
    adapt_rounds = 0;
    adapt_rendered = 0;
    long n_act = slots_all;
    const int32_t* act = nullptr;  // round 0: every slot of the launch (invalid pixels skipped)
    int cur = 0;
    AdaptRound ar{};
    ar.state = d_astate;
    ar.next_count = d_acount;
    sb.stride_slot = 1;
    bool take_rest = false;
    for (int s_base = 0; n_act > 0 && s_base < C.n_samples; s_base += len, len = take_rest ? C.n_samples : len * grow) {
        len = std::min(len, C.n_samples - s_base);
        ++adapt_rounds;
        // round 0 numbers every slot of the launch's tiles; only the pixels inside the region render
        adapt_rendered += (unsigned long long)(act ? n_act : region_pixels(reg, mine)) * (unsigned long long)len;
        if (trace) std::fprintf(stderr, "[rt adaptive] round %d: samples [%d, %d) of %ld pixels\n", adapt_rounds,
                                s_base, s_base + len, n_act);
        ar.len = len;
        ar.horizon = (int32_t)std::min<long>(C.n_samples, (long)s_base + len + (long)len * grow);
        ar.next_act = d_act[1 - cur];
        sb.s_base = s_base;
        sb.err_in_rec = 1;
        r.v.pool = guided_schedule(r.plan, (double)n_act, len, r.plan.rounds, cus, sb);
        const size_t rec_per_slot = (size_t)len * sizeof(float4);
        const long pass_slots = record_pass_slots(n_act, sb, len);
        sb.rec = sample_records((size_t)pass_slots * rec_per_slot);
        hip_check(hipMemsetAsync(d_acount, 0, 2 * sizeof(unsigned int), stream), "hipMemsetAsync");
        for (long a0 = 0; a0 < n_act; a0 += pass_slots, ++pass) {
            sb.slots = (int32_t)std::min<long>(pass_slots, n_act - a0);
            sb.stride_s = sb.slots;
            sb.act = act ? act + a0 : nullptr;
            sb.tile0 = act ? 0 : (int32_t)(a0 / kWave);
            run_pass(r, pass == 0);
            hip_check(launch_adapt(r.S, reg, r.out, r.plan.g.tiles_x, sb, ar, stream), "pt_adapt_kernel launch");
            hip_check(hipEventRecord(pass_event(pass, 2), stream), "hipEventRecord");
        }
        hip_check(hipMemcpyAsync(h_acount, d_acount, 2 * sizeof(unsigned int), hipMemcpyDeviceToHost, stream),
                  "hipMemcpyAsync");
        hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");
        const long n_prev = n_act;
        n_act = (long)h_acount[0];
        const long n_likely = (long)h_acount[1];
        if (trace)
            std::fprintf(stderr, "[rt adaptive]   %ld carried, %ld likely to converge by sample %d\n", n_act, n_likely,
                         ar.horizon);
        act = d_act[1 - cur];
        cur = 1 - cur;
        take_rest = jump > 0 && n_act > 0 &&
                    ((double)(n_prev - n_act) < (double)jump * 1e-3 * (double)n_prev ||
                     (likely_pm > 0 && (double)n_likely < (double)likely_pm * 1e-3 * (double)n_act));
    }
}

void DevCtx::prog_free() {
    if (prog.h_count) (void)hipHostFree(prog.h_count);
    if (prog.h_fwords) (void)hipHostFree(prog.h_fwords);
    for (hipEvent_t e : prog.fev)
        if (e) (void)hipEventDestroy(e);
    prog = ProgSession{};
}

void DevCtx::prog_alloc(const rt_region& region, int32_t precision) {
    const RtCamera& C = build.cam;
    const rt_region clamped = clamp_region(region, C.width, C.height);
    if (region_empty(clamped)) throw std::invalid_argument("progressive: the region is empty after clamping to the image");
    prog_free();
    ProgSession& P = prog;
    P.region = clamped;
    P.precision = precision;
    P.slots = (long)((P.region.width + kTile - 1) / kTile) * ((P.region.height + kTile - 1) / kTile) * kWave;
    if (P.slots >= kItemCap) throw std::invalid_argument("progressive: the region has too many pixels");
    const size_t px = (size_t)C.width * C.height;
    try {
        P.d_state.ensure((size_t)P.slots, "hipMalloc(progressive state)");
        P.d_act.ensure((size_t)P.slots, "hipMalloc(active list)");
        P.d_count.ensure(2, "hipMalloc");
        hip_check(hipHostMalloc((void**)&P.h_count, 2 * sizeof(unsigned int), 0), "hipHostMalloc");
        P.d_rgb.ensure(px * 3, "hipMalloc(progressive frame)");
        P.d_rad.ensure(px * 3, "hipMalloc(progressive frame)");
        P.d_pxs.ensure(px, "hipMalloc(progressive frame)");
        P.d_pxb.ensure(px, "hipMalloc(progressive frame)");
        hip_check(hipMemset(P.d_state, 0, (size_t)P.slots * sizeof(ProgPix)), "hipMemset");
    } catch (...) {
        prog_free();
        throw;
    }
    P.open = true;
}

void DevCtx::prog_resolve(hipStream_t stream) {
    ProgSession& P = prog;
    hip_check(hipMemsetAsync(P.d_count, 0, 2 * sizeof(unsigned int), stream), "hipMemsetAsync");
    const ProgResolve pr{P.d_state, (int32_t)P.slots, P.d_act, P.d_count};
    const int tiles_x = std::max((P.region.width + kTile - 1) / kTile, 1);
    hip_check(launch_resolve(dev_scene(), prog_reg(), prog_out(), tiles_x, pr, stream), "pt_resolve_kernel launch");
}

void DevCtx::prog_read(hipStream_t stream) {
    ProgSession& P = prog;
    unsigned long long wl[ST_WORDS * kStatStride];
    hip_check(hipMemcpyAsync(wl, d_stats, sizeof wl, hipMemcpyDeviceToHost, stream), "hipMemcpyAsync");
    hip_check(hipMemcpyAsync(P.h_count, P.d_count, 2 * sizeof(unsigned int), hipMemcpyDeviceToHost, stream),
              "hipMemcpyAsync");
    hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");
    for (int k = 0; k < ST_WORDS; ++k) P.words[k] = wl[k * kStatStride];
    P.err |= P.words[ST_ERROR];
    P.words[ST_ERROR] = P.err;
    P.n_act = (long)P.h_count[0];
}

void DevCtx::prog_start(hipStream_t stream) {
    hip_check(launch_init_stats(d_stats, nullptr, d_tile, stream), "init_stats");
    prog_resolve(stream);
    prog_read(stream);
}

void DevCtx::prog_focus_alloc() {
    ProgSession& P = prog;
    const size_t px = (size_t)build.cam.width * build.cam.height;
    P.d_focus.ensure((size_t)P.slots, "hipMalloc(focus list)");
    P.d_fkey.ensure((size_t)P.slots, "hipMalloc(focus keys)");
    P.d_fwords.ensure(kFocusWords, "hipMalloc(focus words)");
    P.d_fmap.ensure((size_t)P.region.width * P.region.height, "hipMalloc(focus score)");
    P.d_fmask.ensure(px, "hipMalloc(focus mask)");
    if (!P.h_fwords) hip_check(hipHostMalloc((void**)&P.h_fwords, 4 * sizeof(uint32_t), 0), "hipHostMalloc");
    for (hipEvent_t& e : P.fev)
        if (!e) hip_check(hipEventCreate(&e), "hipEventCreate");
}

// One step of the session, from launch(): samples [s_base, s_base + len) of the step's pixels (a
// plain step: the active pixels from samples_done) on the chunked / pool kernel like an
// adaptive round (16-byte records, error flags in the records), in record passes under the
// record budget, each settled into the state (pt_settle_kernel); then one resolve pass over the
// whole region.
void DevCtx::launch_progressive(LaunchRun& r, const ProgStep& step) {
    ProgSession& P = prog;
    const hipStream_t stream = r.stream;
    SampleBuf& sb = r.sb;
    int& pass = r.pass;
    const long n_act = step.n;
    const int len = step.len;
    sb.s_base = step.s_base;
    sb.err_in_rec = 1;
    sb.rec12 = 0;
    sb.stride_slot = 1;
    sb.tile0 = 0;
    r.v.pool = guided_schedule(r.plan, (double)n_act, len, r.plan.rounds, cus, sb);
    const size_t rec_per_slot = (size_t)len * sizeof(float4);
    const long pass_slots = record_pass_slots(n_act, sb, len);
    sb.rec = sample_records((size_t)pass_slots * rec_per_slot);
    const ProgPass pp{P.d_state, len};
    for (long a0 = 0; a0 < n_act; a0 += pass_slots, ++pass) {
        sb.slots = (int32_t)std::min<long>(pass_slots, n_act - a0);
        sb.stride_s = sb.slots;
        sb.act = step.list + a0;
        run_pass(r, pass == 0);
        hip_check(launch_settle(r.S, r.plan.reg, r.out, r.plan.g.tiles_x, sb, pp, stream), "pt_settle_kernel launch");
        if (a0 + pass_slots >= n_act) prog_resolve(stream);  // (timed with the last pass's settle)
        hip_check(hipEventRecord(pass_event(pass, 2), stream), "hipEventRecord");
    }
}

hipEvent_t* DevCtx::dn_events(int levels) {
    while ((int)dn_ev.size() < kDenoiseMaxLevels + 5) {
        hipEvent_t e = nullptr;
        hip_check(hipEventCreate(&e), "hipEventCreate");
        dn_ev.push_back(e);
    }
    dn_levels = levels;
    return dn_ev.data();
}

int DevCtx::first_hit_traversal(int trav) {
    const RtCamera& C = build.cam;
    if (!d_prim_object) {
        std::vector<int32_t> po(std::max<size_t>(C.n_prims, 1), -1);
        std::copy(build.prim_object.begin(), build.prim_object.begin() + std::min(build.prim_object.size(), po.size()),
                  po.begin());
        d_prim_object.ensure(po.size(), "hipMalloc(prim_object)");
        hip_check(hipMemcpy(d_prim_object, po.data(), po.size() * sizeof(int32_t), hipMemcpyHostToDevice), "hipMemcpy");
    }
    const int tr = effective_traversal(trav);
    if (stack_lds_bytes(C.stack_depth, tr, C.n_prims) > (size_t)lds_max)
        throw std::runtime_error("traversal stack exceeds the workgroup LDS (BVH too deep)");
    return tr;
}

void DevCtx::launch_coverage_pass(const rt_region& r, int trav, int k, uint32_t* coverage, uint8_t* hold,
                                  hipStream_t stream) {
    const int tr = first_hit_traversal(trav);
    for (hipEvent_t& e : cov_ev)
        if (!e) hip_check(hipEventCreate(&e), "hipEventCreate");
    hip_check(hipEventRecord(cov_ev[0], stream), "hipEventRecord");
    hip_check(launch_coverage(dev_scene(), tr, RtRegion{r.x, r.y, r.width, r.height, 0, 1}, d_prim_object, k, coverage,
                              hold, lds_max, stream),
              "coverage_kernel launch");
    hip_check(hipEventRecord(cov_ev[1], stream), "hipEventRecord");
    cov_timed = true;
}

void DevCtx::launch_guide_pass(const rt_region& r, int trav, const DenoiseGuides& g, hipStream_t stream,
                               const rt_guide_options* go, int32_t* chain) {
    const int tr = first_hit_traversal(trav);
    const RtRegion reg{r.x, r.y, r.width, r.height, 0, 1};
    if (go && go->mode == RT_GUIDES_SPECULAR) {
        hip_check(launch_guide_walk(dev_scene(), tr, reg, d_prim_object, g, chain, go->max_bounces, go->max_fuzz, lds_max,
                                    stream),
                  "guide_walk_kernel launch");
        return;
    }
    hip_check(launch_guides(dev_scene(), tr, reg, d_prim_object, g, lds_max, stream), "guide_kernel launch");
    hip_check(launch_guides_chain(g, r.width * r.height, chain, stream), "guides_chain_kernel");
}

hipEvent_t* DevCtx::rp_events() {
    while (rp_ev.size() < 5) {
        hipEvent_t e = nullptr;
        hip_check(hipEventCreate(&e), "hipEventCreate");
        rp_ev.push_back(e);
    }
    return rp_ev.data();
}

const uint8_t* DevCtx::ensure_reusable() {
    if (!d_reusable) upload_table(d_reusable, host.reusable_objects(), "hipMalloc(reusable objects)");
    return d_reusable;
}

void DevCtx::ensure_adapt(size_t slots) {
    if (!h_acount) hip_check(hipHostMalloc((void**)&h_acount, 2 * sizeof(unsigned int), 0), "hipHostMalloc");
    d_acount.ensure(2, "hipMalloc");
    if (slots > d_astate.cap) {  // (all three freed before the first grows)
        d_astate.reset();
        d_act[0].reset();
        d_act[1].reset();
    }
    d_astate.ensure(slots, "hipMalloc(adaptive state)");
    d_act[0].ensure(slots, "hipMalloc(active list)");
    d_act[1].ensure(slots, "hipMalloc(active list)");
}

void DevCtx::read_stats(rt_render_stats* st, uint64_t* counters, hipStream_t stream) {
    unsigned long long wl[ST_WORDS * kStatStride], w[ST_WORDS];
    hip_check(hipMemcpyAsync(wl, d_stats, sizeof wl, hipMemcpyDeviceToHost, stream), "hipMemcpyAsync");
    unsigned long long c[kCounterWords];
    if (counters)
        hip_check(hipMemcpyAsync(c, d_counters, sizeof c, hipMemcpyDeviceToHost, stream), "hipMemcpyAsync");
    hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");
    for (int k = 0; k < ST_WORDS; ++k) w[k] = wl[k * kStatStride];
    if (counters)
        for (int k = 0; k < kCounterWords; ++k) counters[k] = c[k];
    stats_from_words(w, st);
}

void DevCtx::stats_from_words(const unsigned long long* w, rt_render_stats* st) {
    if (w[ST_ERROR] & ERR_NO_BACKGROUND)
        throw std::runtime_error("Cannot read properties of undefined (reading 'top')");
    if (w[ST_ERROR] & ERR_EMIT_STACK)
        throw std::runtime_error("emission stack overflow: depth exceeds the emissive-scatter limit (128)");
    if (!st) return;
    st->pixels = (double)w[ST_PIXELS];
    st->samples_total = (double)w[ST_SAMPLES];
    st->samples_min = w[ST_SMIN] == ~0ull ? INFINITY : (double)w[ST_SMIN];
    st->samples_max = (double)w[ST_SMAX];
    st->samples_avg = st->pixels > 0 ? st->samples_total / st->pixels : 0.0;
    st->bounces_total = (double)w[ST_BOUNCES];
    st->bounces_min = w[ST_BMIN] == ~0ull ? INFINITY : (double)w[ST_BMIN];
    st->bounces_max = (double)w[ST_BMAX];
    st->bounces_avg = st->samples_total > 0 ? st->bounces_total / st->samples_total : 0.0;
}

}  // namespace rt

void rt_history::release() {
    if (alloc_device >= 0) {
        rt::DeviceScope scope;
        (void)hipSetDevice(alloc_device);
        for (hipEvent_t& e : ev) {
            if (e) (void)hipEventDestroy(e);
            e = nullptr;
        }
        side[0] = Side{};
        side[1] = Side{};
        d_reusable.reset();
        d_through.reset();
    }
    through_mask = -1;
    views = 0, device = -1, alloc_device = -1, front = 0, n_objects = 0;
    width = height = 0;
    region = rt_region{};
    scene_hash = 0;
    timed = filtered = false;
}
