// C ABI of the accumulation across views (temporal.hpp): the history object, the plain session and
// stand-alone accumulate calls and their timings - and the run, the session body and the stand-alone
// body those share with the calls through specular chains (temporal_spec_api.cpp), which pass a
// chain argument.
#include <algorithm>
#include <cstring>
#include <vector>

#include "pass_host.hpp"
#include "prog_blob.hpp"
#include "temporal_spec.hpp"

using namespace rt;

TpOpts rt::tp_resolve(const rt_temporal_options* o, const std::string& who) {
    const rt_temporal_options z = o ? *o : rt_temporal_options{0.0f, 0.0f, 0.0f, 0.0f, 0, 0.0f};
    TpOpts r{gather_resolve(z.normal_min, z.sigma_plane, z.min_weight, who), 0.0f, z.filter_levels, 0.0f};
    r.max_history = resolve_field(z.max_history, 256.0f, who, "max_history");
    r.sigma_variance = resolve_field(z.sigma_variance, 2.0f, who, "sigma_variance");
    if (r.levels < 0 || r.levels > kDenoiseMaxLevels)
        throw std::invalid_argument(who + ": filter_levels must be 0.." + std::to_string(kDenoiseMaxLevels) +
                                    " (0: no filter)");
    return r;
}

// The hash a history keeps of its scene: the arrays the reprojection's same-scene check compares.
uint64_t rt::tp_scene_hash(const SceneBuild& b) {
    uint64_t f = fnv1a(b.nodes.data(), b.nodes.size() * sizeof(RtNode));
    f = fnv1a(b.prims.data(), b.prims.size() * sizeof(RtPrim), f);
    f = fnv1a(b.mats.data(), b.mats.size() * sizeof(RtMat), f);
    f = fnv1a(b.lights.data(), b.lights.size() * sizeof(RtLight), f);
    return fnv1a(b.prim_object.data(), b.prim_object.size() * sizeof(int32_t), f);
}

void rt::tp_run(DnBufs& b, const TpNew& nw, const rt_region& r, const TpHistory& hist, const RpView& view, const rt_region& pr,
                const uint8_t* d_reusable, int n_objects, const TpOpts& o, float4* out_col, float* out_var, bool want_rad,
                bool want_u8, bool want_var, bool want_len, hipStream_t stream, hipEvent_t* ev, const TpChain* ch) {
    const int n = r.width * r.height;
    const TpOut out{out_col, out_var, b.dist()};
    auto args = [&](auto a) {  // the head TpArgs and TsArgs share
        a = gather_args<decltype(a)>(view, r, pr, n_objects, o, nw);
        a.max_history = o.max_history;
        a.vpitch = r.width, a.vx0 = 0, a.vy0 = 0;
        return a;
    };
    if (ch) {
        TsArgs a = args(TsArgs{});
        a.chain_history = ch->chain_history ? 1 : 0;
        a.pp2 = pr.width > 0 ? rs_pp2(view, ch->point_pixels) : 0.0f;
        for (int k = 0; k < 3; ++k) a.cn[k] = ch->cn[k];
        TsHistory sh{{hist.gn, hist.gp, nullptr, nullptr, nullptr}, hist.col, hist.var};
        if (ch->chain_history) sh.g = ch->hg;
        hip_check(launch_temporal_spec(a, ch->ng, sh, d_reusable, ch->d_through, nw.fresh, nw.pxs, nw.var, out, ch->d_kind,
                                       stream),
                  "temporal_spec_kernel");
    } else {
        hip_check(launch_temporal(args(TpArgs{}), nw.gn, nw.gp, hist, d_reusable, nw.fresh, nw.pxs, nw.var, out, stream),
                  "temporal_kernel");
    }
    if (ev) hip_check(hipEventRecord(ev[2], stream), "hipEventRecord");
    const bool filter = o.levels > 0 && (want_rad || want_u8 || want_var);
    if (filter || want_var) {
        // (the kernel has read the fresh variance, which may be b.var itself)
        b.var.ensure((size_t)n, "hipMalloc(denoise variance)");
        hip_check(hipMemcpyAsync(b.var, out_var, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, stream), "hipMemcpyAsync");
    }
    if (filter) {
        hip_check(launch_denoise_unpack(out_col, n, b.rad(), nullptr, nullptr, stream), "denoise_unpack_kernel");
        dn_filter(b, ch ? ch->ng.sgn : nw.gn, ch ? ch->ng.sgp : nw.gp, b.rad(), r.width, 0, 0, r.width, r.height,
                  DnOpts{true, o.levels, o.sigma_variance, o.sigma_plane}, want_rad, want_u8, want_var, stream, nullptr);
    }
    if (ev) hip_check(hipEventRecord(ev[3], stream), "hipEventRecord");
    if (!filter && (want_rad || want_u8))
        hip_check(launch_denoise_unpack(out_col, n, want_rad ? b.rad() : nullptr, want_u8 ? b.u8.p : nullptr, nullptr, stream),
                  "denoise_unpack_kernel");
    if (want_len) hip_check(launch_denoise_unpack(out_col, n, nullptr, nullptr, b.nrm(), stream), "denoise_unpack_kernel");
}

// A call's outputs into the caller's arrays, then its one host sync.
static void tp_outputs(const DnBufs& b, const RegionIo& io, float* radiance, uint8_t* rgb, float* variance, float* length,
                       float* weight) {
    io.down(radiance, b.rad(), 3 * sizeof(float));
    io.down(rgb, b.u8, 3);
    io.down(variance, b.var, sizeof(float));
    io.down(length, b.nrm(), sizeof(float));
    io.down(weight, b.dist(), sizeof(float));
    hip_check(hipStreamSynchronize(io.stream), "hipStreamSynchronize");
}

static bool same_bits(float a, float b) { return std::memcmp(&a, &b, sizeof(float)) == 0; }

void rt::tp_session(rt_camera* cam, rt_history* h, const std::string& who, const TpOpts& o, int32_t commit, uint8_t* rgb,
                    float* radiance, float* variance_out, float* length_out, float* weight_out, const TpSessionChain* sc) {
    DevCtx& c = session_with(cam, who, 2);
    const uint64_t hash = tp_scene_hash(cam->build);
    if (h->views > 0 && hash != h->scene_hash) throw std::invalid_argument("temporal: the history holds a different scene");
    if (h->views > 0 && h->device != c.device)
        throw std::invalid_argument(who + ": the history was committed on another device");
    const RtCamera& C = cam->build.cam;
    DevCtx::ProgSession& P = c.prog;
    const hipStream_t stream = nullptr;
    const RegionIo io{C.width, P.region, stream};
    const rt_region& r = io.r;
    const size_t n = (size_t)io.n();
    if (h->views == 0 && h->alloc_device != c.device) {
        h->release();  // (buffers of an uncommitted call elsewhere)
        h->alloc_device = c.device;
    }
    for (hipEvent_t& e : h->ev)
        if (!e) hip_check(hipEventCreate(&e), "hipEventCreate");
    rt_history::Side& back = h->side[h->front ^ 1];
    const rt_history::Side& front = h->side[h->front];
    back.ensure(n);
    if (sc && commit) back.ensure_chain(n);
    if (!h->d_reusable || h->views == 0) {  // (an uncommitted call may have been another scene's)
        std::vector<uint8_t> t = cam->reusable_objects();
        h->n_objects = (int32_t)t.size();
        upload_table(h->d_reusable, std::move(t), "hipMalloc(reusable objects)");
    }
    if (sc && (!h->d_through || h->views == 0 || h->through_mask != sc->through ||
               !same_bits(h->through_fuzz, sc->go.max_fuzz))) {
        upload_table(h->d_through, through_objects(*cam, sc->through, sc->go.max_fuzz), "hipMalloc(through objects)");
        h->through_mask = sc->through;
        h->through_fuzz = sc->go.max_fuzz;
    }
    DnBufs& b = c.dn;
    b.ensure(n);
    if (sc) c.rs.kind.ensure(n, "hipMalloc(chain guides)");
    hip_check(hipEventRecord(h->ev[0], stream), "hipEventRecord");
    session_guides(cam, c, stream);
    if (sc) session_specular_guides(cam, c, sc->go, stream, true);
    prog_variance_pass(c, stream);
    hip_check(hipEventRecord(h->ev[1], stream), "hipEventRecord");
    const bool has = h->views > 0;
    const TpHistory hist = has ? TpHistory{front.gn, front.gp, front.col, front.var} : TpHistory{};
    const rt_region pr = has ? h->region : rt_region{0, 0, 0, 0};
    const TpNew nw{{P.d_gn, P.d_gp, P.d_rad, P.d_pxs, C.width, r.x, r.y, 0.0f}, b.var};
    TpChain ch{};
    if (sc) {
        // the history's chain planes serve only when they were walked with these very options
        const bool chain_history = has && front.has_chain && front.chain_go.max_bounces == sc->go.max_bounces &&
                                   same_bits(front.chain_go.max_fuzz, sc->go.max_fuzz);
        ch = TpChain{{P.d_gn, P.d_gp, P.d_sgn, P.d_sgp, P.d_sch}, {front.gn, front.gp, front.sgn, front.sgp, front.chain},
                     chain_history, C.center, h->d_through, sc->point_pixels, c.rs.kind};
    }
    tp_run(b, nw, r, hist, h->rp_view, pr, h->d_reusable, h->n_objects, o, back.col, back.var, radiance != nullptr,
           rgb != nullptr, variance_out != nullptr, length_out != nullptr, stream, h->ev, sc ? &ch : nullptr);
    if (commit) {
        // the session may be gone before the next view: the history keeps the guides itself, and
        // after a plain commit no chain planes (a specular one may have left those of an older view)
        auto keep = [&](void* dst, const void* src, size_t elem) {
            hip_check(hipMemcpyAsync(dst, src, n * elem, hipMemcpyDeviceToDevice, stream), "hipMemcpyAsync");
        };
        keep(back.gn, P.d_gn, sizeof(float4));
        keep(back.gp, P.d_gp, sizeof(float4));
        if (sc) {
            keep(back.sgn, P.d_sgn, sizeof(float4));
            keep(back.sgp, P.d_sgp, sizeof(float4));
            keep(back.chain, P.d_sch, sizeof(int32_t));
            back.chain_go = sc->go;
        }
        back.has_chain = sc != nullptr;
    }
    hip_check(hipEventRecord(h->ev[4], stream), "hipEventRecord");
    h->timed = true;
    h->filtered = o.levels > 0 && (radiance || rgb || variance_out);
    if (sc) io.down(sc->kind_out, c.rs.kind, 1);
    tp_outputs(b, io, radiance, rgb, variance_out, length_out, weight_out);
    if (commit) {
        h->front ^= 1;
        h->views += 1;
        h->device = c.device;
        h->width = C.width, h->height = C.height;
        h->region = r;
        h->scene_hash = hash;
        (void)rt_camera_get_view(cam, &h->view);
        h->rp_view = rp_camera_view(cam);
    }
}

void rt::tp_explicit(const std::string& who, const TpCall& a, const TpOpts& o, float point_pixels) {
    const bool spec = point_pixels >= 0.0f;
    const hipStream_t stream = nullptr;
    const RegionIo io{a.width, dn_region(a.region, a.width, a.height, who), stream};
    const rt_view& pv = *a.prev_view;
    const RegionIo pio{pv.width, dn_region(a.prev_region, pv.width, pv.height, who), stream};
    const RpView view = rp_view_constants(pv.center, pv.pixel00, pv.du, pv.dv, pv.width, pv.height);
    const size_t n = (size_t)io.n(), np = (size_t)pio.n();
    // (ns / ps: the chain guides' pairs, their obj planes the chain words, ns.u8 the kind plane)
    DnBufs nb, pb, ns, ps;
    rt_history::Side out;
    DevBuf<float> d_var;
    DevBuf<uint8_t> d_reusable, d_through;
    out.ensure(n);
    d_var.ensure(n, "hipMalloc(denoise variance)");
    upload_reusable(d_reusable, a.reusable, a.n_objects, stream);
    if (spec) upload_reusable(d_through, a.through, a.n_objects, stream);
    TpChain ch{};
    upload_views(nb, ns, io, a.g, pb, ps, pio, a.pg, &ch.ng, &ch.hg);
    pb.var.ensure(np, "hipMalloc(history)");  // (after pb's own allocation, which resets it)
    // (the guides are packed: the staging arrays now carry the frames, the length and the counts)
    pio.up(pb.rad(), a.prev_radiance, 3 * sizeof(float));
    pio.up(pb.dist(), a.prev_length, sizeof(float));
    pio.up(pb.var, a.prev_variance, sizeof(float));
    hip_check(launch_temporal_pack(pb.rad(), pb.dist(), (int)np, pb.c0, stream), "temporal_pack_kernel");
    io.up(nb.pos(), a.radiance, 3 * sizeof(float));
    io.up(d_var, a.variance, sizeof(float));
    if (a.px_samples) io.up(nb.obj, a.px_samples, sizeof(int32_t));
    const TpNew nw{{nb.gn, nb.gp, nb.pos(), a.px_samples ? nb.obj.p : nullptr, io.r.width, 0, 0, (float)a.samples}, d_var};
    if (spec) {
        ch.chain_history = a.pg.chain != nullptr;
        ch.cn = a.view->center, ch.d_through = d_through, ch.point_pixels = point_pixels, ch.d_kind = ns.u8;
    }
    tp_run(nb, nw, io.r, TpHistory{pb.gn, pb.gp, pb.c0, pb.var}, view, pio.r, d_reusable, a.n_objects, o, out.col, out.var,
           a.radiance_out != nullptr, a.rgb_out != nullptr, a.variance_out != nullptr, a.length_out != nullptr, stream,
           nullptr, spec ? &ch : nullptr);
    if (spec) io.down(a.kind_out, ns.u8, 1);
    tp_outputs(nb, io, a.radiance_out, a.rgb_out, a.variance_out, a.length_out, a.weight_out);
}

extern "C" {

int rt_history_create(rt_history** out) {
    if (!out) return set_error(RT_ERR_INVALID, "null argument");
    try {
        *out = new rt_history();
        return RT_OK;
    } catch (const std::exception& e) {
        return set_error(RT_ERR_RENDER, e.what());
    }
}

void rt_history_destroy(rt_history* h) { delete h; }

int rt_history_get_info(const rt_history* h, rt_history_info* info) {
    if (!h || !info) return set_error(RT_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lock(const_cast<rt_history*>(h)->mu);
    *info = rt_history_info{};
    info->width = h->width;
    info->height = h->height;
    info->region = h->region;
    info->views = h->views;
    info->device = h->device;
    info->scene_hash = h->scene_hash;
    info->bytes = h->side[0].bytes() + h->side[1].bytes() + h->d_reusable.cap;
    info->view = h->view;
    return RT_OK;
}

int rt_history_read(rt_history* h, float* radiance, float* variance, float* length) {
    return history_call(h, [&] {
        if (h->views <= 0) throw std::invalid_argument("rt_history_read: the history is empty");
        DeviceScope scope;
        hip_check(hipSetDevice(h->device), "hipSetDevice");
        const rt_history::Side& s = h->side[h->front];
        const RegionIo io{h->width, h->region, nullptr};
        DnBufs b;  // staging of this call alone
        b.ensure((size_t)io.n());
        hip_check(launch_denoise_unpack(s.col, io.n(), radiance ? b.rad() : nullptr, nullptr, length ? b.dist() : nullptr,
                                        io.stream),
                  "denoise_unpack_kernel");
        io.down(radiance, b.rad(), 3 * sizeof(float));
        io.down(length, b.dist(), sizeof(float));
        io.down(variance, s.var, sizeof(float));
        hip_check(hipStreamSynchronize(io.stream), "hipStreamSynchronize");
    });
}

int rt_camera_progressive_accumulate(rt_camera* cam, rt_history* h, const rt_temporal_options* options, int32_t commit,
                                     uint8_t* rgb, float* radiance, float* variance_out, float* length_out,
                                     float* weight_out) {
    if (!h) return set_error(RT_ERR_INVALID, "null history");
    std::lock_guard<std::mutex> hlock(h->mu);
    return camera_call(cam, [&] {
        const std::string who = "rt_camera_progressive_accumulate";
        const TpOpts o = tp_resolve(options, who);
        tp_session(cam, h, who, o, commit, rgb, radiance, variance_out, length_out, weight_out);
    });
}

int rt_temporal_accumulate(int32_t width, int32_t height, const rt_region* region, const float* normal,
                           const float* position, const float* distance, const int32_t* object, const float* radiance,
                           const int32_t* px_samples, int32_t samples, const float* variance, const rt_view* prev_view,
                           const rt_region* prev_region, const float* prev_normal, const float* prev_position,
                           const float* prev_distance, const int32_t* prev_object, const float* prev_radiance,
                           const float* prev_variance, const float* prev_length, const uint8_t* reusable,
                           int32_t n_objects, const rt_temporal_options* options, float* radiance_out,
                           float* variance_out, float* length_out, float* weight_out, uint8_t* rgb_out) {
    return api_guard([&] {
        const std::string who = "rt_temporal_accumulate";
        if (width <= 0 || height <= 0) throw std::invalid_argument(who + ": width and height must be positive");
        if (!normal || !position || !distance || !object || !radiance || !variance)
            throw std::invalid_argument(who + ": normal, position, distance, object, radiance and variance are required");
        if (!prev_view || !prev_normal || !prev_position || !prev_distance || !prev_object || !prev_radiance ||
            !prev_variance || !prev_length)
            throw std::invalid_argument(who + ": prev_view, prev_normal, prev_position, prev_distance, prev_object, "
                                              "prev_radiance, prev_variance and prev_length are required");
        if (prev_view->width <= 0 || prev_view->height <= 0)
            throw std::invalid_argument(who + ": the previous view's width and height must be positive");
        if (n_objects < 0 || (n_objects > 0 && !reusable))
            throw std::invalid_argument(who + ": reusable must hold n_objects >= 0 entries");
        if (samples < 0) throw std::invalid_argument(who + ": samples must not be negative");
        const TpOpts o = tp_resolve(options, who);
        tp_explicit(who,
                    TpCall{width, height, samples, n_objects, region, prev_region, nullptr, prev_view,
                           {normal, position, distance, object}, {prev_normal, prev_position, prev_distance, prev_object},
                           radiance, variance, prev_radiance, prev_variance, prev_length, px_samples, reusable, nullptr,
                           radiance_out, variance_out, length_out, weight_out, rgb_out, nullptr},
                    o);
    });
}

int rt_history_times(rt_history* h, float* guide_ms, float* gather_ms, float* filter_ms, float* total_ms) {
    if (!guide_ms || !gather_ms || !filter_ms || !total_ms) return set_error(RT_ERR_INVALID, "null argument");
    return history_call(h, [&] {
        if (!h->timed) throw std::invalid_argument("rt_history_times: no accumulate call yet");
        DeviceScope scope;
        hip_check(hipSetDevice(h->alloc_device), "hipSetDevice");
        hipEvent_t* ev = h->ev;  // guide + variance [0, 1), gather [1, 2), filter [2, 3), outputs + commit [3, 4)
        hip_check(hipEventSynchronize(ev[4]), "hipEventSynchronize");
        hip_check(hipEventElapsedTime(guide_ms, ev[0], ev[1]), "hipEventElapsedTime");
        hip_check(hipEventElapsedTime(gather_ms, ev[1], ev[2]), "hipEventElapsedTime");
        *filter_ms = 0.0f;
        if (h->filtered) hip_check(hipEventElapsedTime(filter_ms, ev[2], ev[3]), "hipEventElapsedTime");
        hip_check(hipEventElapsedTime(total_ms, ev[0], ev[4]), "hipEventElapsedTime");
    });
}

}  // extern "C"
