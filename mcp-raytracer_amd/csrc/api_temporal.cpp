// C ABI of the accumulation across views (temporal.hpp): the history object, the session and
// stand-alone accumulate calls and their timings.
#include <algorithm>
#include <vector>

#include "pass_host.hpp"
#include "prog_blob.hpp"

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

// The device side of a call: the gather and blend into `out` (weight -> b.dist()), then the
// caller's outputs - the optional variance-guided filter of out / Vout, else out itself - into
// b.rad() / b.u8 / b.var, and the length into b.nrm(). pr.width == 0: an empty history. ev (or
// null): events 2 and 3, recorded after the gather and after the filter. Queued.
static void tp_run(DnBufs& b, const TpNew& nw, const rt_region& r, const TpHistory& hist, const RpView& view,
                   const rt_region& pr, const uint8_t* d_reusable, int n_objects, const TpOpts& o, float4* out_col,
                   float* out_var, bool want_rad, bool want_u8, bool want_var, bool want_len, hipStream_t stream,
                   hipEvent_t* ev) {
    const int n = r.width * r.height;
    TpArgs a = gather_args<TpArgs>(view, r, pr, n_objects, o, nw);
    a.max_history = o.max_history;
    a.vpitch = r.width, a.vx0 = 0, a.vy0 = 0;
    hip_check(launch_temporal(a, nw.gn, nw.gp, hist, d_reusable, nw.fresh, nw.pxs, nw.var, TpOut{out_col, out_var, b.dist()},
                              stream),
              "temporal_kernel");
    tp_finish(b, nw.gn, nw.gp, r, o, out_col, out_var, want_rad, want_u8, want_var, want_len, stream, ev);
}

void rt::tp_finish(DnBufs& b, const float4* fgn, const float4* fgp, const rt_region& r, const TpOpts& o, float4* out_col,
                   float* out_var, bool want_rad, bool want_u8, bool want_var, bool want_len, hipStream_t stream,
                   hipEvent_t* ev) {
    const int n = r.width * r.height;
    if (ev) hip_check(hipEventRecord(ev[2], stream), "hipEventRecord");
    const bool filter = o.levels > 0 && (want_rad || want_u8 || want_var);
    if (filter || want_var) {
        // (the kernel has read the fresh variance, which may be b.var itself)
        b.var.ensure((size_t)n, "hipMalloc(denoise variance)");
        hip_check(hipMemcpyAsync(b.var, out_var, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, stream), "hipMemcpyAsync");
    }
    if (filter) {
        hip_check(launch_denoise_unpack(out_col, n, b.rad(), nullptr, nullptr, stream), "denoise_unpack_kernel");
        dn_filter(b, fgn, fgp, b.rad(), r.width, 0, 0, r.width, r.height,
                  DnOpts{true, o.levels, o.sigma_variance, o.sigma_plane}, want_rad, want_u8, want_var, stream, nullptr);
    }
    if (ev) hip_check(hipEventRecord(ev[3], stream), "hipEventRecord");
    if (!filter && (want_rad || want_u8))
        hip_check(launch_denoise_unpack(out_col, n, want_rad ? b.rad() : nullptr, want_u8 ? b.u8.p : nullptr, nullptr, stream),
                  "denoise_unpack_kernel");
    if (want_len) hip_check(launch_denoise_unpack(out_col, n, nullptr, nullptr, b.nrm(), stream), "denoise_unpack_kernel");
}

void rt::tp_outputs(const DnBufs& b, const RegionIo& io, float* radiance, uint8_t* rgb, float* variance, float* length,
                    float* weight) {
    io.down(radiance, b.rad(), 3 * sizeof(float));
    io.down(rgb, b.u8, 3);
    io.down(variance, b.var, sizeof(float));
    io.down(length, b.nrm(), sizeof(float));
    io.down(weight, b.dist(), sizeof(float));
    hip_check(hipStreamSynchronize(io.stream), "hipStreamSynchronize");
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
        if (!h->d_reusable || h->views == 0) {  // (an uncommitted call may have been another scene's)
            std::vector<uint8_t> t = cam->reusable_objects();
            h->n_objects = (int32_t)t.size();
            upload_table(h->d_reusable, std::move(t), "hipMalloc(reusable objects)");
        }
        DnBufs& b = c.dn;
        b.ensure(n);
        hip_check(hipEventRecord(h->ev[0], stream), "hipEventRecord");
        session_guides(cam, c, stream);
        prog_variance_pass(c, stream);
        hip_check(hipEventRecord(h->ev[1], stream), "hipEventRecord");
        const bool has = h->views > 0;
        const TpHistory hist = has ? TpHistory{front.gn, front.gp, front.col, front.var} : TpHistory{};
        const rt_region pr = has ? h->region : rt_region{0, 0, 0, 0};
        const TpNew nw{{P.d_gn, P.d_gp, P.d_rad, P.d_pxs, C.width, r.x, r.y, 0.0f}, b.var};
        tp_run(b, nw, r, hist, h->rp_view, pr, h->d_reusable, h->n_objects, o, back.col, back.var, radiance != nullptr,
               rgb != nullptr, variance_out != nullptr, length_out != nullptr, stream, h->ev);
        if (commit) {
            // the session may be gone before the next view: the history keeps the guides itself
            hip_check(hipMemcpyAsync(back.gn, P.d_gn, n * sizeof(float4), hipMemcpyDeviceToDevice, stream), "hipMemcpyAsync");
            hip_check(hipMemcpyAsync(back.gp, P.d_gp, n * sizeof(float4), hipMemcpyDeviceToDevice, stream), "hipMemcpyAsync");
            back.has_chain = false;  // (a specular commit may have left chain planes of an older view)
        }
        hip_check(hipEventRecord(h->ev[4], stream), "hipEventRecord");
        h->timed = true;
        h->filtered = o.levels > 0 && (radiance || rgb || variance_out);
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
        const hipStream_t stream = nullptr;
        const RegionIo io{width, dn_region(region, width, height, who), stream};
        const RegionIo pio{prev_view->width, dn_region(prev_region, prev_view->width, prev_view->height, who), stream};
        const RpView view = rp_view_constants(prev_view->center, prev_view->pixel00, prev_view->du, prev_view->dv,
                                              prev_view->width, prev_view->height);
        const size_t n = (size_t)io.n(), np = (size_t)pio.n();
        DnBufs nb, pb;
        rt_history::Side out;
        DevBuf<float> d_var;
        DevBuf<uint8_t> d_reusable;
        nb.ensure(n);
        pb.ensure(np);
        pb.var.ensure(np, "hipMalloc(history)");
        out.ensure(n);
        d_var.ensure(n, "hipMalloc(denoise variance)");
        upload_reusable(d_reusable, reusable, n_objects, stream);
        upload_guides(nb, io, normal, position, distance, object);
        upload_guides(pb, pio, prev_normal, prev_position, prev_distance, prev_object);
        // (the guides are packed: the staging arrays now carry the frames, the length and the counts)
        pio.up(pb.rad(), prev_radiance, 3 * sizeof(float));
        pio.up(pb.dist(), prev_length, sizeof(float));
        pio.up(pb.var, prev_variance, sizeof(float));
        hip_check(launch_temporal_pack(pb.rad(), pb.dist(), (int)np, pb.c0, stream), "temporal_pack_kernel");
        io.up(nb.pos(), radiance, 3 * sizeof(float));
        io.up(d_var, variance, sizeof(float));
        if (px_samples) io.up(nb.obj, px_samples, sizeof(int32_t));
        const TpNew nw{{nb.gn, nb.gp, nb.pos(), px_samples ? nb.obj.p : nullptr, io.r.width, 0, 0, (float)samples}, d_var};
        tp_run(nb, nw, io.r, TpHistory{pb.gn, pb.gp, pb.c0, pb.var}, view, pio.r, d_reusable, n_objects, o, out.col, out.var,
               radiance_out != nullptr, rgb_out != nullptr, variance_out != nullptr, length_out != nullptr, stream, nullptr);
        tp_outputs(nb, io, radiance_out, rgb_out, variance_out, length_out, weight_out);
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
