// A camera and its device contexts: the host build (scene.cpp), and per device the uploaded
// scene blob, the frame, record, stats and session buffers and the launch that executes a
// LaunchPlan (launch_plan.hpp). rt_api.cpp is the C ABI over these; multi_gpu.cpp the
// single-process multi-GPU render.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/rt_amd.h"
#include "denoise.hpp"
#include "focus.hpp"
#include "host_util.hpp"
#include "launch.hpp"
#include "launch_plan.hpp"
#include "primary.hpp"
#include "progressive.hpp"
#include "reproject.hpp"
#include "scene.hpp"
#include "scene_blob.hpp"
#include "temporal.hpp"

namespace rt {

// Region-packed device buffers of one filter call (denoise.hpp), grown on demand: the colour
// ping-pong pair, the per-call guide plane, a guide pair, and the staging arrays the host
// copies go through (radiance / normal / position float[3], distance, object, u8).
struct DnBufs {
    DevBuf<float4> c0, c1, fn, gn, gp;
    DevBuf<float> stage;  // 10 floats per pixel
    DevBuf<int32_t> obj;
    DevBuf<uint8_t> u8;
    size_t cap = 0;     // pixels
    DevBuf<float> var;  // region-packed variance of the variance-guided calls
    float* rad() const { return stage; }
    float* nrm() const { return stage + 3 * cap; }
    float* pos() const { return stage + 6 * cap; }
    float* dist() const { return stage + 9 * cap; }
    // (the caller has made the buffers' device current)
    void free() { *this = DnBufs{}; }
    void ensure(size_t n) {
        if (n <= cap) return;
        free();
        try {
            for (DevBuf<float4>* p : {&c0, &c1, &fn, &gn, &gp}) p->ensure(n, "hipMalloc(denoise)");
            stage.ensure(n * 10, "hipMalloc(denoise)");
            obj.ensure(n, "hipMalloc(denoise)");
            u8.ensure(n * 3, "hipMalloc(denoise)");
        } catch (...) {
            free();
            throw;
        }
        cap = n;
    }
};

// The host half of a camera: the reference's Camera after createCameraFromSceneData
// (src/scenes/scenes.ts:60-104) - the flattened scene, options and mixture weights.
struct CamHost {
    SceneBuild build;
    int32_t precision = PREC_REF;
    int32_t traversal = TRAV_AUTO;
    double mix_total = 0.5, light_w = 0.0;
    // the guides the camera's filter calls compute (rt_camera_set_denoise_guides)
    rt_guide_options dn_guide{RT_GUIDES_FIRST_HIT, 8, 0.0f};

    // The strategy a launch actually uses: BRUTE/FAST are exact only where every
    // primitive lies inside its reference box (scene_tree.cpp prims_inside_boxes).
    int effective_traversal(int trav) const {
        if (!build.fast_ok) return TRAV_REFERENCE;
        if (trav == TRAV_AUTO) return build.cam.n_prims <= kBruteMaxPrims ? TRAV_BRUTE : TRAV_FAST;
        return trav;
    }
    // reusable[o] = 1 iff SceneData.objects[o]'s material (already resolved to a table index by
    // the build) is lambert or light: what a reprojection may carry over to another view.
    std::vector<uint8_t> reusable_objects() const {
        std::vector<uint8_t> t((size_t)std::max(build.cam.n_prims, 0), 0);
        for (size_t s = 0; s < build.prims.size() && s < build.prim_object.size(); ++s) {
            const int32_t o = build.prim_object[s], m = build.prims[s].mat;
            if (o < 0 || (size_t)o >= t.size() || m < 0 || (size_t)m >= build.mats.size()) continue;
            t[o] = build.mats[m].type == MAT_LAMBERT || build.mats[m].type == MAT_LIGHT;
        }
        return t;
    }
    // The primary-ray candidate table (primary.hpp) serves brute-force launches of a pinhole
    // camera (path_begin moves the origin only when aperture > 0) over at most 16 primitives.
    bool primary_table_ok(int trav) const {
        return effective_traversal(trav) == TRAV_BRUTE && !(build.cam.aperture > 0.0) &&
               build.cam.n_prims <= kPrimaryMaxPrims && (size_t)build.cam.n_prims == build.prims.size();
    }
};

// One step of a progressive session: `len` samples from index s_base of the n slots in `list`.
// A plain step: the session's active list from samples_done; a focused step: the focus list
// from samples + focus_done.
struct ProgStep {
    const int32_t* list;
    long n;
    int32_t s_base, len;
};

// One device's copy of a camera: the scene blob in that device's HBM, its frame, record and
// stats buffers, events and (multi-GPU) its stream and tile-packed slabs. A camera keeps one
// per device it rendered on (rt_camera_render_multi: one per listed device entry), so moving
// between devices never re-uploads.
struct DevCtx {
    const CamHost& host;
    const SceneBuild& build;
    const int device;    // HIP device ordinal the buffers live on
    const int instance;  // >0: a further context on the same device (a device listed twice)
    bool live = false;   // scene uploaded, buffers allocated
    DevCtx(const CamHost& h, int dev, int inst) : host(h), build(h.build), device(dev), instance(inst) {}
    DevCtx(const DevCtx&) = delete;
    DevCtx& operator=(const DevCtx&) = delete;
    ~DevCtx();

    DevBuf<uint4> d_blob;  // the scene blob (scene_blob.hpp)
    SceneBlob blob;        // its offsets and counts (bytes dropped after the upload)
    int lds_max = 64 * 1024;  // dynamic LDS bytes a workgroup may use on this device
    // HIP events of the last launch, 3 per pass: path kernel start, path kernel
    // end, accumulate end (the sequential kernel: one pass, no accumulate)
    std::vector<hipEvent_t> ev;
    int n_passes = 0;
    bool ev_accum = false;
    int last_kernel = RT_KERNEL_NONE;
    // the primary-ray candidate table (primary.hpp): W x H records beside the scene blob, built
    // on first use (the camera and the primitives never change after rt_camera_create)
    DevBuf<uint64_t> d_ptab;
    hipEvent_t ptab_ev[2] = {nullptr, nullptr};  // around the builder kernel
    bool ptab_used = false;                      // the last launch ran pt_pool_primary_kernel
    DevBuf<unsigned long long> d_stats, d_counters;
    DevBuf<unsigned int> d_tile;
    DevBuf<uint8_t> d_rgb;
    DevBuf<float> d_rad;
    int cus = 256;

    // multi-GPU (rt_camera_render_multi): this context's stream, its tile-packed slabs, and on
    // the root context the gathered slabs of every device plus the stats words' host copy
    hipStream_t stream = nullptr;
    hipEvent_t ev_rendered = nullptr, ev_gather0 = nullptr, ev_gather1 = nullptr;
    DevBuf<uint8_t> d_slab, d_gather;
    DevBuf<float> d_rslab, d_rgather;
    unsigned long long* h_words = nullptr;
    int h_words_cap = 0;
    // multi-GPU buffers (grown on demand; the caller has made `device` current)
    void ensure_multi(size_t slab_bytes, size_t rslab_bytes, bool root, int n);

    // Frees what ensure_device and the launches allocated; makes `device` current meanwhile.
    void release();
    // Uploads the scene on first use; the caller has made `device` current.
    void ensure_device();
    void ensure_frame();

    // Events of pass p (created on demand on the camera's device).
    hipEvent_t pass_event(int p, int k);

    // The strategy a launch actually uses: BRUTE/FAST are exact only where every
    // primitive lies inside its reference box (scene_tree.cpp prims_inside_boxes).
    int effective_traversal(int trav) const { return host.effective_traversal(trav); }

    // Device time of the last launch from its events: path kernel(s) and accumulate passes,
    // summed per pass (never one span across both). Waits for those events.
    void times(float* path_ms, float* accum_ms);

    DevScene dev_scene() const;

    // The primary-ray candidate table, built on `stream` at first use; every later launch makes
    // its stream wait for the builder's end event (nothing to wait for on the builder's own stream
    // or once it has run). No stream handle is kept: the caller may destroy its stream.
    const uint2* ensure_primary_table(hipStream_t stream);
    // Device time of the builder kernel (0 before it ran). Waits for it.
    float primary_table_ms();

    // Launch one render: plan (launch_plan.hpp), then execute; returns after queueing.
    void launch(const rt_region& region, int tile_group, int tile_groups, int prec, int trav, int count,
                uint8_t* rgb, float* rad, int32_t* pxs, int32_t* pxb, int packed, hipStream_t stream,
                const ProgStep* step = nullptr);  // one step of the progressive session (launch_progressive)

    // What the passes of one launch share (dev_ctx.cpp).
    struct LaunchRun;
    void run_pass(LaunchRun& r, bool first);
    void launch_fixed(LaunchRun& r);
    void launch_adaptive_rounds(LaunchRun& r);
    void launch_progressive(LaunchRun& r, const ProgStep& step);

    // ---- Progressive session (rt_camera_progressive_*) ----------------------------------------
    // State that outlives a call: every region pixel's running PixelStats under its slot (region
    // tile * 64 + lane), the list of the slots still sampling, and the session's own frame. None
    // of it is shared with one-shot renders (whose adaptive rounds use d_astate / d_act, and
    // whose frame is d_rgb / d_rad); the record buffer, the stats words and the hand-out
    // counter are per launch and shared.
    struct ProgSession {
        bool open = false;
        rt_region region{};  // clamped to the image
        int32_t precision = PREC_REF;
        long slots = 0;      // region tiles * 64
        int32_t done = 0;    // samples every unfinished pixel holds
        int32_t steps = 0;
        long n_act = 0;      // pixels still sampling
        unsigned long long err = 0;             // error flags of the samples kept so far
        unsigned long long words[ST_WORDS]{};   // RenderStats words of the current frame
        DevBuf<ProgPix> d_state;
        DevBuf<int32_t> d_act;
        DevBuf<unsigned int> d_count;
        unsigned int* h_count = nullptr;
        DevBuf<uint8_t> d_rgb;
        DevBuf<float> d_rad;
        DevBuf<int32_t> d_pxs, d_pxb;
        DevBuf<float4> d_gn;  // the region's guides (denoise.hpp), computed by the first
        DevBuf<float4> d_gp;  // rt_camera_progressive_denoise of the session
        // the region's guides through the specular chain (guide_walk.hip), of the options sg_key:
        // a pair of their own - reprojection, accumulation and focus read d_gn / d_gp
        DevBuf<float4> d_sgn, d_sgp;
        // the region's edge-hold mask (coverage.hpp) for hold_k sub-rays a side (0: none yet),
        // computed by the first rt_camera_progressive_denoise*_hold call that asks for that k
        DevBuf<uint8_t> d_hold;
        int32_t hold_k = 0;
        rt_guide_options sg_key{};
        bool sg_valid = false;
        // the chain plane of that walk, kept once a reprojection through the chains asked for it
        DevBuf<int32_t> d_sch;
        bool sch_valid = false;
        // Focused steps (focus.hpp), allocated by the first one: the selected slots, the score
        // keys of the active entries, the selection's words (counts, T, digit states and
        // histograms) and their host copy, an uploaded score map, the full-frame selected mask,
        // and the events around the selection.
        int32_t focus_done = 0;  // samples the focused steps have used past the camera's `samples`
        bool focused = false;    // a focused step has rendered: pixels differ in their sample sets
        DevBuf<int32_t> d_focus;
        DevBuf<uint32_t> d_fkey, d_fwords;
        uint32_t* h_fwords = nullptr;
        DevBuf<float> d_fmap;
        DevBuf<uint8_t> d_fmask;
        hipEvent_t fev[2] = {nullptr, nullptr};
    } prog;

    // (the caller has made `device` current, or this runs from release(), which has)
    void prog_free();
    // Opens a session over `region` (clamped; empty: invalid) with every pixel at zero samples.
    void prog_alloc(const rt_region& region, int32_t precision);

    RtRegion prog_reg() const { return RtRegion{prog.region.x, prog.region.y, prog.region.width, prog.region.height, 0, 1}; }
    RenderOut prog_out() const { return RenderOut{prog.d_rgb, prog.d_rad, prog.d_pxs, prog.d_pxb, d_stats, d_counters, d_tile, 0}; }

    // State -> the session's frame, RenderStats (added to d_stats: the caller has reset the
    // words, launch() or launch_init_stats) and the active list; queued.
    void prog_resolve(hipStream_t stream);
    // Waits for the resolve pass: the frame's stats words (error flags: every kept sample's so
    // far) and the number of pixels still sampling.
    void prog_read(hipStream_t stream);
    // A new or restored session's first resolve (no path kernel): frame, stats, active list.
    void prog_start(hipStream_t stream);
    // The focus buffers of the open session (first focused step).
    void prog_focus_alloc();

    // ---- Guides and the a-trous filter (denoise.hpp) -------------------------------------------
    DnBufs dn;                       // one call's buffers (kept between calls)
    DevBuf<int32_t> d_prim_object;   // prim slot -> SceneData.objects index
    // HIP events of the last filter call: [0, 1) the guide pass, then dn_filter's levels + 3
    std::vector<hipEvent_t> dn_ev;
    int dn_levels = 0;        // levels of the last call (0: none yet)
    bool dn_guides = false;   // the last call ran the guide pass (a session computes it once)
    hipEvent_t* dn_events(int levels);

    // The guide pass over `r` (clamped) into g, through the strategy `trav` resolves to; queued.
    // go (null: first hit) selects the walk through the specular chain; chain (region-packed, or
    // null) receives either pass's chain word.
    void launch_guide_pass(const rt_region& r, int trav, const DenoiseGuides& g, hipStream_t stream,
                           const rt_guide_options* go = nullptr, int32_t* chain = nullptr);

    // What the first-hit passes share: d_prim_object uploaded once, and the strategy `trav` resolves
    // to, whose traversal stack must fit the workgroup's LDS.
    int first_hit_traversal(int trav);

    // ---- Sub-pixel coverage (coverage.hpp) -------------------------------------------------------
    DevBuf<uint32_t> d_cov;   // one call's coverage words (region-packed, kept between calls)
    DevBuf<uint8_t> d_hold;   // a camera filter call's hold mask (a session keeps its own)
    // HIP events around the last coverage pass of this context
    hipEvent_t cov_ev[2] = {nullptr, nullptr};
    bool cov_timed = false;
    // The coverage pass over `r` (clamped) for k x k sub-rays into coverage / hold (region-packed,
    // either may be null), through the strategy `trav` resolves to, between cov_ev; queued.
    void launch_coverage_pass(const rt_region& r, int trav, int k, uint32_t* coverage, uint8_t* hold, hipStream_t stream);

    // ---- Reprojection (reproject.hpp) -----------------------------------------------------------
    // As the NEW view's context: the reusable table and the events of the last call. As the
    // PREVIOUS view's context: that view's guides (gn / gp), its uploaded radiance (rad()) and
    // packed colour (c0) - buffers of their own, so a camera may be both views of one call.
    DnBufs rp_prev;
    DevBuf<uint8_t> d_reusable;      // object index -> 1: lambert or light
    // HIP events of the last reproject call: start, after the guide passes, before and after
    // the gather kernel, after the unpack passes
    std::vector<hipEvent_t> rp_ev;
    bool rp_timed = false;           // a call has recorded them
    hipEvent_t* rp_events();
    // The reusable table on the device (uploaded once: the scene never changes).
    const uint8_t* ensure_reusable();

    // ---- Reprojection through specular chains (reproject_spec.hpp) ------------------------------
    // One view's guides through the chain and its chain plane, region-packed, beside the first-hit
    // pair in dn / rp_prev: rs as the NEW view's context (with the call's kind plane), rs_prev as
    // the PREVIOUS view's - a camera may be both views of one call.
    struct RsBufs {
        DevBuf<float4> sgn, sgp;
        DevBuf<int32_t> chain;
        DevBuf<uint8_t> kind;
        void ensure(size_t n) {
            sgn.ensure(n, "hipMalloc(chain guides)");
            sgp.ensure(n, "hipMalloc(chain guides)");
            chain.ensure(n, "hipMalloc(chain guides)");
            kind.ensure(n, "hipMalloc(chain guides)");
        }
        void free() { *this = RsBufs{}; }
    } rs, rs_prev;
    // object index -> 1: a chain may start on it, for the mask and max_fuzz it was built from
    DevBuf<uint8_t> d_through;
    int32_t through_mask = -1;
    float through_fuzz = 0.0f;

    int adapt_rounds = 0;                  // rounds of the last adaptive render
    unsigned long long adapt_rendered = 0;  // samples its rounds rendered (>= the samples kept)
    // Adaptive rounds: per-slot running PixelStats, two active lists, the list counter.
    DevBuf<AdaptPix> d_astate;
    DevBuf<int32_t> d_act[2];
    DevBuf<unsigned int> d_acount;
    unsigned int* h_acount = nullptr;
    void ensure_adapt(size_t slots);

    // Per-sample record buffer of the chunked kernel (grown on demand, kept).
    DevBuf<float4> d_sbuf;
    float4* sample_records(size_t bytes) {
        d_sbuf.ensure((bytes + sizeof(float4) - 1) / sizeof(float4), "hipMalloc(sample buffer)");
        return d_sbuf;
    }

    void read_stats(rt_render_stats* st, uint64_t* counters, hipStream_t stream);

    // ---- Ordering between calls (rt_amd.h, rt_launch) -------------------------------------------
    // Calls on one context take effect in the order they were issued, whatever stream each queues
    // on: they share the stats words, the hand-out counter, the record buffer and every cache
    // above. An entry that returns with work still queued (an asynchronous rt_camera_render_device,
    // rt_camera_stats_words) records order_ev after it; the next call that queues on another stream
    // makes its stream wait for the event first. order_key is that stream's handle as a number: it
    // is compared and never handed to the runtime, so the caller may destroy the stream. A call on
    // the same stream adds no wait and no host sync.
    hipEvent_t order_ev = nullptr;  // hipEventDisableTiming
    uintptr_t order_key = 0;
    bool order_pending = false;
    // `stream` is about to queue work of this context (the context's device is current).
    void order_after(hipStream_t stream);
    // The call that queued on `stream` returns without a host sync. check: throw on a HIP error.
    void order_mark(hipStream_t stream, bool check = true);

    // RenderStats from the 8 stats words; the reference's thrown Errors for the error flags.
    static void stats_from_words(const unsigned long long* w, rt_render_stats* st);
};

}  // namespace rt

struct rt_camera : rt::CamHost {
    std::mutex mu;
    std::vector<std::unique_ptr<rt::DevCtx>> ctxs;
    rt::DevCtx* last = nullptr;  // the context of the most recent render (queries read it)
    // the most recent rt_camera_render_multi: its device contexts, transport and plan
    std::vector<rt::DevCtx*> multi;
    int multi_transport = -1;
    rt_multi_plan multi_plan{};

    rt::DevCtx& ctx(int dev, int inst = 0) {
        for (auto& c : ctxs)
            if (c->device == dev && c->instance == inst) return *c;
        ctxs.emplace_back(new rt::DevCtx(*this, dev, inst));
        return *ctxs.back();
    }
    // the context of the calling thread's current HIP device, for a call that queues on `stream`
    // (every entry but rt_camera_render_device: the null stream): ordered after the context's
    // previous call (DevCtx::order_after)
    rt::DevCtx& current(hipStream_t stream = nullptr) {
        int dev = 0;
        rt::hip_check(hipGetDevice(&dev), "hipGetDevice");
        rt::DevCtx& c = ctx(dev, 0);
        c.order_after(stream);
        return c;
    }
    rt::DevCtx* prog = nullptr;  // the context that holds the open progressive session
    void release() {
        multi.clear();
        last = nullptr;
        prog = nullptr;  // (the session's buffers go with its context)
        ctxs.clear();
    }
    // the open session's context; a step, info or save without one is an argument error
    rt::DevCtx& session(const char* what) {
        if (!prog || !prog->prog.open) throw std::invalid_argument(std::string(what) + ": no progressive session is open");
        if (prog->order_pending) {  // (the session entries queue on the null stream)
            rt::DeviceScope scope;
            rt::hip_check(hipSetDevice(prog->device), "hipSetDevice");
            prog->order_after(nullptr);
        }
        return *prog;
    }
    void end_session() {
        if (!prog) return;
        rt::DeviceScope scope;
        (void)hipSetDevice(prog->device);
        prog->prog_free();
        prog = nullptr;
    }
};

// A view history (rt_history_*, temporal.hpp): device buffers of its own on the device of its first
// commit, so the cameras and sessions it was fed from may go. Two sets of planes: the kernel reads
// set `front` and writes the other, and a commit swaps them.
struct rt_history {
    std::mutex mu;
    struct Side {
        rt::DevBuf<float4> col, gn, gp;  // {r, g, b, length}; the guides of the view it holds
        rt::DevBuf<float> var;
        void ensure(size_t n) {
            for (rt::DevBuf<float4>* p : {&col, &gn, &gp}) p->ensure(n, "hipMalloc(history)");
            var.ensure(n, "hipMalloc(history)");
        }
        // the chain planes of that view (temporal_spec.hpp), allocated by the first specular commit:
        // its guides through the chain and its chain words, held when has_chain, walked with chain_go
        rt::DevBuf<float4> sgn, sgp;
        rt::DevBuf<int32_t> chain;
        bool has_chain = false;
        rt_guide_options chain_go{};
        void ensure_chain(size_t n) {
            sgn.ensure(n, "hipMalloc(history)");
            sgp.ensure(n, "hipMalloc(history)");
            chain.ensure(n, "hipMalloc(history)");
        }
        size_t bytes() const {
            return (col.cap + gn.cap + gp.cap + sgn.cap + sgp.cap) * sizeof(float4) + var.cap * sizeof(float) +
                   chain.cap * sizeof(int32_t);
        }
    } side[2];
    int front = 0;
    rt::DevBuf<uint8_t> d_reusable;
    // object index -> 1: a chain may start on it, for the mask and max_fuzz it was built from
    // (the specular calls; rebuilt when either changes)
    rt::DevBuf<uint8_t> d_through;
    int32_t through_mask = -1;
    float through_fuzz = 0.0f;
    int32_t n_objects = 0;
    int32_t views = 0, device = -1;
    int32_t width = 0, height = 0;
    rt_region region{};
    rt_view view{};
    rt::RpView rp_view{};
    uint64_t scene_hash = 0;
    // HIP events of the last session call: start, after the guide and variance passes, after the
    // gather, after the filter, after the unpack passes and the commit's guide copy
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    int alloc_device = -1;  // where the buffers and events live: `device` once a view is committed
    bool timed = false, filtered = false;
    // Frees everything on the devices that hold it; the history is empty afterwards.
    void release();
    ~rt_history() { release(); }
};

namespace rt {

// ---- multi_gpu.cpp ------------------------------------------------------------------------------
// The multi-GPU split of a region: its 8x8 tiles dealt round-robin over n
// devices (tile t -> entry t % n), each device's tiles packed into an equal-size slab padded
// to the largest share, plus one spare tile whose first 64 bytes carry the device's stats
// words (the gather brings them along; rt_tiles_unpack never reads that tile).
rt_multi_plan make_multi_plan(const rt_region& region, int width, int height, int n);

// Single-process multi-GPU render (rt_camera_render_multi); returns the root context with the
// frame in d_rgb / d_rad: `outputs` queues the caller's copies on its stream before the one
// host sync, after which *merged holds the merged stats words.
DevCtx& render_multi(rt_camera* cam, const int32_t* devices, int n, const rt_region& region, bool want_rgb,
                     bool want_rad, unsigned long long* merged, const std::function<void(DevCtx&)>& outputs);

}  // namespace rt
