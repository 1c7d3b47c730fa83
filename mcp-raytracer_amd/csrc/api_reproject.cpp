// C ABI of the reprojection of a previous view's frame (reproject.hpp): the view and
// reusable-table queries, the stand-alone, camera and session calls and their timings.
#include <cstring>
#include <functional>
#include <vector>

#include "pass_host.hpp"

using namespace rt;

// The device side of a call once both views' guides and the previous radiance (pb.rad(),
// region-packed) are there: the previous colour packed as the plain filter packs it, the gather,
// then history -> nb.nrm(), weight -> nb.dist(), the blend -> nb.rad() / nb.u8 and, through chains,
// the kind -> ch->d_kind. ev (or null): events 2..4, recorded before and after the gather and after
// the unpack passes. Queued.
void rt::rp_run(DnBufs& nb, DnBufs& pb, const RpView& view, const rt_region& r, const rt_region& pr,
                const uint8_t* d_reusable, int n_objects, const RpOpts& o, const RpNew& nw, bool want_hist, bool want_rad,
                bool want_u8, hipStream_t stream, hipEvent_t* ev, const RpChain* ch) {
    auto mark = [&](int k) {
        if (ev) hip_check(hipEventRecord(ev[k], stream), "hipEventRecord");
    };
    hip_check(launch_denoise_pack(pb.rad(), pr.width, 0, 0, pr.width, pr.height, pb.gn, 1.0f, nullptr, pb.c0, pb.fn, stream),
              "denoise_pack_kernel");
    mark(2);
    if (ch) {
        RsArgs a = gather_args<RsArgs>(view, r, pr, n_objects, o, nw);
        a.nh = o.nh;
        a.pp2 = rs_pp2(view, ch->point_pixels);
        for (int k = 0; k < 3; ++k) a.cn[k] = ch->cn[k];
        hip_check(launch_reproject_spec(a, ch->ng, ch->pg, pb.c0, d_reusable, ch->d_through, nw.fresh, nw.pxs, nb.c0, nb.c1,
                                        stream),
                  "reproject_spec_kernel");
    } else {
        RpArgs a = gather_args<RpArgs>(view, r, pr, n_objects, o, nw);
        a.nh = o.nh;
        hip_check(launch_reproject(a, nw.gn, nw.gp, pb.gn, pb.gp, pb.c0, d_reusable, nw.fresh, nw.pxs, nb.c0,
                                   nw.fresh ? nb.c1.p : nullptr, stream),
                  "reproject_kernel");
    }
    mark(3);
    const int n = r.width * r.height;
    if (want_hist) hip_check(launch_denoise_unpack(nb.c0, n, nb.nrm(), nullptr, nb.dist(), stream), "denoise_unpack_kernel");
    if (nw.fresh && (want_rad || want_u8))
        hip_check(launch_denoise_unpack(nb.c1, n, want_rad ? nb.rad() : nullptr, want_u8 ? nb.u8.p : nullptr, nullptr, stream),
                  "denoise_unpack_kernel");
    if (ch && ch->want_kind) hip_check(launch_reproject_spec_kind(nb.c1, n, ch->d_kind, stream), "reproject_spec_kind_kernel");
    mark(4);
}

// A call's outputs into the caller's arrays, then its one host sync.
void rt::rp_outputs(const DnBufs& nb, const RegionIo& io, float* history, float* weight, float* radiance, uint8_t* rgb,
                    uint8_t* kind, const uint8_t* d_kind) {
    io.down(history, nb.nrm(), 3 * sizeof(float));
    io.down(weight, nb.dist(), sizeof(float));
    io.down(radiance, nb.rad(), 3 * sizeof(float));
    io.down(rgb, nb.u8, 3);
    io.down(kind, d_kind, 1);
    hip_check(hipStreamSynchronize(io.stream), "hipStreamSynchronize");
}

// The previous view's side of a camera call, on the current device: its context with the
// radiance uploaded into rp_prev.rad() and the guide pass queued into rp_prev.gn / gp; with `go`,
// also the guide pass through the chain into its rs_prev.
DevCtx& rt::rp_prev_side(rt_camera* prev_cam, const rt_region& pr, const float* prev_radiance, hipStream_t stream,
                         hipEvent_t* ev, const std::function<void()>& new_guides, const rt_guide_options* go) {
    DevCtx& p = prev_cam->current();
    p.ensure_device();
    DnBufs& pb = p.rp_prev;
    const size_t n = (size_t)pr.width * pr.height;
    pb.ensure(n);
    if (go) p.rs_prev.ensure(n);
    RegionIo{prev_cam->build.cam.width, pr, stream}.up(pb.rad(), prev_radiance, 3 * sizeof(float));
    hip_check(hipEventRecord(ev[0], stream), "hipEventRecord");
    new_guides();
    p.launch_guide_pass(pr, prev_cam->traversal, DenoiseGuides{pb.gn, pb.gp}, stream);
    if (go) p.launch_guide_pass(pr, prev_cam->traversal, DenoiseGuides{p.rs_prev.sgn, p.rs_prev.sgp}, stream, go, p.rs_prev.chain);
    hip_check(hipEventRecord(ev[1], stream), "hipEventRecord");
    return p;
}

extern "C" {

int rt_camera_get_view(const rt_camera* cam, rt_view* view) {
    if (!cam || !view) return set_error(RT_ERR_INVALID, "null argument");
    const RtCamera& C = cam->build.cam;
    for (int k = 0; k < 3; ++k) {
        view->center[k] = C.center[k];
        view->pixel00[k] = C.pixel00[k];
        view->du[k] = C.du[k];
        view->dv[k] = C.dv[k];
    }
    view->width = C.width;
    view->height = C.height;
    return RT_OK;
}

int rt_camera_reusable_objects(const rt_camera* cam, uint8_t* out, int32_t capacity) {
    if (!cam || !out) return set_error(RT_ERR_INVALID, "null argument");
    const std::vector<uint8_t> t = cam->reusable_objects();
    if ((int64_t)capacity < (int64_t)t.size())
        return set_error(RT_ERR_INVALID, "rt_camera_reusable_objects: capacity below the number of objects");
    if (!t.empty()) std::memcpy(out, t.data(), t.size());
    return RT_OK;
}

int rt_reproject(int32_t width, int32_t height, const rt_region* region, const float* normal, const float* position,
                 const float* distance, const int32_t* object, const rt_view* prev_view, const rt_region* prev_region,
                 const float* prev_radiance, const float* prev_normal, const float* prev_position,
                 const float* prev_distance, const int32_t* prev_object, const uint8_t* reusable, int32_t n_objects,
                 const rt_reproject_options* options, const float* radiance, const int32_t* px_samples, int32_t samples,
                 float* history_out, float* weight_out, float* radiance_out, uint8_t* rgb_out) {
    return api_guard([&] {
        const std::string who = "rt_reproject";
        if (width <= 0 || height <= 0) throw std::invalid_argument(who + ": width and height must be positive");
        if (!normal || !position || !distance || !object)
            throw std::invalid_argument(who + ": normal, position, distance and object are required");
        if (!prev_view || !prev_normal || !prev_position || !prev_distance || !prev_object)
            throw std::invalid_argument(who + ": prev_view, prev_normal, prev_position, prev_distance and prev_object are required");
        if (prev_view->width <= 0 || prev_view->height <= 0)
            throw std::invalid_argument(who + ": the previous view's width and height must be positive");
        if (n_objects < 0 || (n_objects > 0 && !reusable))
            throw std::invalid_argument(who + ": reusable must hold n_objects >= 0 entries");
        rp_check(who, prev_radiance, radiance, samples, radiance_out, rgb_out);
        const RpOpts o = rp_resolve(options, who);
        const hipStream_t stream = nullptr;
        const RegionIo io{width, dn_region(region, width, height, who), stream};
        const RegionIo pio{prev_view->width, dn_region(prev_region, prev_view->width, prev_view->height, who), stream};
        const RpView view = rp_view_constants(prev_view->center, prev_view->pixel00, prev_view->du, prev_view->dv,
                                              prev_view->width, prev_view->height);
        DnBufs nb, pb;
        DevBuf<uint8_t> d_reusable;
        nb.ensure((size_t)io.n());
        pb.ensure((size_t)pio.n());
        upload_reusable(d_reusable, reusable, n_objects, stream);
        upload_guides(nb, io, normal, position, distance, object);
        upload_guides(pb, pio, prev_normal, prev_position, prev_distance, prev_object);
        pio.up(pb.rad(), prev_radiance, 3 * sizeof(float));
        // (the guides are packed: the staging arrays now carry the fresh frame and the counts)
        if (radiance) io.up(nb.rad(), radiance, 3 * sizeof(float));
        if (radiance && px_samples) io.up(nb.obj, px_samples, sizeof(int32_t));
        const RpNew nw{nb.gn, nb.gp, radiance ? nb.rad() : nullptr, radiance && px_samples ? nb.obj.p : nullptr,
                       io.r.width, 0, 0, (float)samples};
        rp_run(nb, pb, view, io.r, pio.r, d_reusable, n_objects, o, nw, history_out || weight_out, radiance_out != nullptr,
               rgb_out != nullptr, stream, nullptr);
        rp_outputs(nb, io, history_out, weight_out, radiance_out, rgb_out);
    });
}

int rt_camera_reproject(rt_camera* cam, const rt_region* region, rt_camera* prev_cam, const rt_region* prev_region,
                        const rt_reproject_options* options, const float* prev_radiance, const float* radiance,
                        const int32_t* px_samples, int32_t samples, float* history_out, float* weight_out,
                        float* radiance_out, uint8_t* rgb_out) {
    return two_camera_call(cam, prev_cam, [&] {
        const std::string who = "rt_camera_reproject";
        const RtCamera &C = cam->build.cam, &PC = prev_cam->build.cam;
        rp_check(who, prev_radiance, radiance, samples, radiance_out, rgb_out);
        const RpOpts o = rp_resolve(options, who);
        const hipStream_t stream = nullptr;
        const RegionIo io{C.width, dn_region(region, C.width, C.height, who), stream};
        const rt_region pr = dn_region(prev_region, PC.width, PC.height, who);
        rp_same_scene(cam, prev_cam);
        DevCtx& c = cam->current();
        c.ensure_device();
        DnBufs& nb = c.dn;
        nb.ensure((size_t)io.n());
        hipEvent_t* ev = c.rp_events();
        const uint8_t* d_reusable = c.ensure_reusable();
        if (radiance) io.up(nb.rad(), radiance, 3 * sizeof(float));
        if (radiance && px_samples) io.up(nb.obj, px_samples, sizeof(int32_t));
        DnBufs& pb = rp_prev_side(prev_cam, pr, prev_radiance, stream, ev, [&] {
            c.launch_guide_pass(io.r, cam->traversal, DenoiseGuides{nb.gn, nb.gp}, stream);
        }).rp_prev;
        const RpNew nw{nb.gn, nb.gp, radiance ? nb.rad() : nullptr, radiance && px_samples ? nb.obj.p : nullptr,
                       io.r.width, 0, 0, (float)samples};
        rp_run(nb, pb, rp_camera_view(prev_cam), io.r, pr, d_reusable, C.n_prims, o, nw, history_out || weight_out,
               radiance_out != nullptr, rgb_out != nullptr, stream, ev);
        c.rp_timed = true;
        rp_outputs(nb, io, history_out, weight_out, radiance_out, rgb_out);
    });
}

int rt_camera_progressive_reproject(rt_camera* cam, rt_camera* prev_cam, const rt_region* prev_region,
                                    const rt_reproject_options* options, const float* prev_radiance, uint8_t* rgb,
                                    float* radiance, float* weight_out) {
    return two_camera_call(cam, prev_cam, [&] {
        const std::string who = "rt_camera_progressive_reproject";
        (void)cam->session(who.c_str());
        session_radiance(cam, who);
        rp_check(who, prev_radiance, nullptr, 0, nullptr, nullptr);
        const RpOpts o = rp_resolve(options, who);
        const RtCamera &C = cam->build.cam, &PC = prev_cam->build.cam;
        const rt_region pr = dn_region(prev_region, PC.width, PC.height, who);
        rp_same_scene(cam, prev_cam);
        DevCtx& c = session_with(cam, who, 0);
        DevCtx::ProgSession& P = c.prog;
        const hipStream_t stream = nullptr;
        const RegionIo io{C.width, P.region, stream};
        DnBufs& nb = c.dn;
        nb.ensure((size_t)io.n());
        hipEvent_t* ev = c.rp_events();
        const uint8_t* d_reusable = c.ensure_reusable();
        DnBufs& pb = rp_prev_side(prev_cam, pr, prev_radiance, stream, ev, [&] { session_guides(cam, c, stream); }).rp_prev;
        const RpNew nw{P.d_gn, P.d_gp, P.d_rad, P.d_pxs, C.width, io.r.x, io.r.y, 0.0f};
        rp_run(nb, pb, rp_camera_view(prev_cam), io.r, pr, d_reusable, C.n_prims, o, nw, weight_out != nullptr,
               radiance != nullptr, rgb != nullptr, stream, ev);
        c.rp_timed = true;
        rp_outputs(nb, io, nullptr, weight_out, radiance, rgb);
    });
}

int rt_camera_reproject_times(rt_camera* cam, float* guide_ms, float* reproject_ms, float* total_ms) {
    if (!guide_ms || !reproject_ms || !total_ms) return set_error(RT_ERR_INVALID, "null argument");
    return camera_call(cam, [&] {
        DevCtx* c = nullptr;
        for (auto& x : cam->ctxs)
            if (x->rp_timed) c = x.get();
        if (!c) throw std::invalid_argument("rt_camera_reproject_times: no reproject call yet");
        DeviceScope scope;
        hip_check(hipSetDevice(c->device), "hipSetDevice");
        hipEvent_t* ev = c->rp_ev.data();  // guide passes [0, 1), pack [1, 2), gather [2, 3), unpack [3, 4)
        hip_check(hipEventSynchronize(ev[4]), "hipEventSynchronize");
        hip_check(hipEventElapsedTime(guide_ms, ev[0], ev[1]), "hipEventElapsedTime");
        hip_check(hipEventElapsedTime(reproject_ms, ev[2], ev[3]), "hipEventElapsedTime");
        hip_check(hipEventElapsedTime(total_ms, ev[0], ev[4]), "hipEventElapsedTime");
    });
}

}  // extern "C"
