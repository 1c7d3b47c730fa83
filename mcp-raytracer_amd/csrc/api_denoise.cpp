// C ABI of the guides and the a-trous filter (denoise.hpp), plain and variance-guided: the guide
// render (first hit, or through the specular chain) and the guides a camera's filter calls compute,
// the three shapes of a filter call, the session's variance and the filter's timings.
#include "pass_host.hpp"

using namespace rt;

// rt_denoise_options / rt_denoise_var_options (NULL: all zero), then resolved by dn_resolve: a
// zero field = the default.
static DnOpts dn_options(const rt_denoise_options* o) {
    return o ? DnOpts{false, o->levels, o->sigma_color, o->sigma_plane} : DnOpts{false, 0, 0.0f, 0.0f};
}
static DnOpts dn_options(const rt_denoise_var_options* o) {
    return o ? DnOpts{true, o->levels, o->sigma_variance, o->sigma_plane} : DnOpts{true, 0, 0.0f, 0.0f};
}
static DnOpts dn_resolve(DnOpts o, const std::string& who) {
    if (o.levels < 0 || o.levels > kDenoiseMaxLevels)
        throw std::invalid_argument(who + ": levels must be 1.." + std::to_string(kDenoiseMaxLevels) + " (0: the default)");
    if (!o.levels) o.levels = 4;
    o.sigma = resolve_field(o.sigma, o.var ? 2.0f : 0.5f, who, o.var ? "sigma_variance" : "sigma_color");
    o.sigma_plane = resolve_field(o.sigma_plane, 0.01f, who, "sigma_plane");
    return o;
}

// The filter's outputs into the caller's arrays, then the call's one host sync.
static void dn_outputs(const DnBufs& b, const RegionIo& io, bool var, float* radiance, float* variance, uint8_t* rgb) {
    io.down(radiance, b.rad(), 3 * sizeof(float));
    if (var) io.down(variance, b.var, sizeof(float));
    io.down(rgb, b.u8, 3);
    hip_check(hipStreamSynchronize(io.stream), "hipStreamSynchronize");
}

// The three shapes of a filter call, plain or variance-guided (o.var: `variance` in, or the
// session's own, and `variance_out`); `o` as dn_options gives it, resolved where the entry point
// always has. Every argument error comes before anything touches a device. The edge hold
// (coverage.hpp) is the frame call's `hold` mask (null: none) and the other two's hold_k (0: none),
// whose mask the coverage pass computes on the device.

// The stand-alone frame call: explicit guides, buffers of its own.
static int dn_frame_call(const std::string& who, DnOpts o, int32_t width, int32_t height, const rt_region* region,
                         const float* radiance, const float* variance, const float* normal, const float* position,
                         const float* distance, const int32_t* object, float* radiance_out, float* variance_out,
                         uint8_t* rgb_out, const uint8_t* hold = nullptr) {
    return api_guard([&] {
        if (width <= 0 || height <= 0) throw std::invalid_argument(who + ": width and height must be positive");
        if (!radiance || (o.var && !variance) || !normal || !position || !distance || !object)
            throw std::invalid_argument(who + ": radiance, " + (o.var ? "variance, " : "") +
                                        "normal, position, distance and object are required");
        o = dn_resolve(o, who);
        const RegionIo io{width, dn_region(region, width, height, who), nullptr};
        DnBufs b;
        b.ensure((size_t)io.n());
        io.up(b.rad(), radiance, 3 * sizeof(float));
        if (o.var) {
            b.var.ensure((size_t)io.n(), "hipMalloc(denoise variance)");
            io.up(b.var, variance, sizeof(float));
        }
        upload_guides(b, io, normal, position, distance, object);
        DevBuf<uint8_t> d_hold;
        if (hold) {
            d_hold.ensure((size_t)io.n(), "hipMalloc(denoise hold)");
            io.up(d_hold, hold, 1);
        }
        dn_filter(b, b.gn, b.gp, b.rad(), io.r.width, 0, 0, io.r.width, io.r.height, o, radiance_out != nullptr,
                  rgb_out != nullptr, variance_out != nullptr, io.stream, nullptr, d_hold);
        dn_outputs(b, io, o.var, radiance_out, variance_out, rgb_out);
    });
}

// The camera call: the guide pass of the camera's scene over the region, the camera's buffers.
static int dn_camera_call(rt_camera* cam, const std::string& who, DnOpts o, const rt_region* region,
                          const float* radiance, const float* variance, float* radiance_out, float* variance_out,
                          uint8_t* rgb_out, int32_t hold_k = 0) {
    return camera_call(cam, [&] {
        const RtCamera& C = cam->build.cam;
        if (!radiance || (o.var && !variance))
            throw std::invalid_argument(who + (o.var ? ": radiance and variance are required" : ": radiance is required"));
        o = dn_resolve(o, who);
        hold_check(hold_k, who);
        const RegionIo io{C.width, dn_region(region, C.width, C.height, who), nullptr};
        DevCtx& c = cam->current();
        c.ensure_device();
        DnBufs& b = c.dn;
        b.ensure((size_t)io.n());
        hipEvent_t* ev = c.dn_events(o.levels);
        io.up(b.rad(), radiance, 3 * sizeof(float));
        if (o.var) {
            b.var.ensure((size_t)io.n(), "hipMalloc(denoise variance)");
            io.up(b.var, variance, sizeof(float));
        }
        // (the coverage pass has events of its own and runs before the filter's span)
        if (hold_k) {
            c.d_hold.ensure((size_t)io.n(), "hipMalloc(denoise hold)");
            c.launch_coverage_pass(io.r, cam->traversal, hold_k, nullptr, c.d_hold, io.stream);
        }
        hip_check(hipEventRecord(ev[0], io.stream), "hipEventRecord");
        c.launch_guide_pass(io.r, cam->traversal, DenoiseGuides{b.gn, b.gp}, io.stream, &cam->dn_guide);
        c.dn_guides = true;
        dn_filter(b, b.gn, b.gp, b.rad(), io.r.width, 0, 0, io.r.width, io.r.height, o, radiance_out != nullptr,
                  rgb_out != nullptr, variance_out != nullptr, io.stream, ev + 1, hold_k ? c.d_hold.p : nullptr);
        dn_outputs(b, io, o.var, radiance_out, variance_out, rgb_out);
    });
}

// The session's hold mask for hold_k (0: none asked for): computed once per k (queued), freed with
// the session.
static void session_hold(rt_camera* cam, DevCtx& c, int32_t hold_k, hipStream_t stream) {
    DevCtx::ProgSession& P = c.prog;
    if (!hold_k || P.hold_k == hold_k) return;
    P.hold_k = 0;
    P.d_hold.ensure((size_t)P.region.width * P.region.height, "hipMalloc(session hold)");
    c.launch_coverage_pass(P.region, cam->traversal, hold_k, nullptr, P.d_hold, stream);
    P.hold_k = hold_k;
}

// The session call: the session's device frame (and, variance-guided, its state) as they stand
// after the last step - nothing is uploaded - and the session's guides.
static int dn_session_call(rt_camera* cam, const std::string& who, DnOpts o, uint8_t* rgb, float* radiance,
                           float* variance_out, int32_t hold_k = 0) {
    return camera_call(cam, [&] {
        (void)cam->session(who.c_str());
        // (the plain call names a wrong mode before its options, the variance-guided one its
        // options before the mode and the sample count)
        if (!o.var) session_radiance(cam, who);
        o = dn_resolve(o, who);
        hold_check(hold_k, who);
        DevCtx& c = session_with(cam, who, o.var ? 2 : 0);
        const RtCamera& C = cam->build.cam;
        DevCtx::ProgSession& P = c.prog;
        const RegionIo io{C.width, P.region, nullptr};
        DnBufs& b = c.dn;
        b.ensure((size_t)io.n());
        hipEvent_t* ev = c.dn_events(o.levels);
        session_hold(cam, c, hold_k, io.stream);
        hip_check(hipEventRecord(ev[0], io.stream), "hipEventRecord");
        // the span [0, 1): the guide pass of a first call (through the specular chain: of the first
        // call with these options) and, variance-guided, the variance pass
        const bool spec = cam->dn_guide.mode == RT_GUIDES_SPECULAR;
        c.dn_guides = o.var || (spec ? !session_specular_cached(c, cam->dn_guide) : !P.d_gn);
        if (spec)
            session_specular_guides(cam, c, cam->dn_guide, io.stream);
        else
            session_guides(cam, c, io.stream);
        const float4 *gn = spec ? P.d_sgn : P.d_gn, *gp = spec ? P.d_sgp : P.d_gp;
        if (o.var) prog_variance_pass(c, io.stream);
        dn_filter(b, gn, gp, P.d_rad, C.width, io.r.x, io.r.y, io.r.width, io.r.height, o, radiance != nullptr,
                  rgb != nullptr, variance_out != nullptr, io.stream, ev + 1, hold_k ? P.d_hold.p : nullptr);
        dn_outputs(b, io, o.var, radiance, variance_out, rgb);
    });
}

// The guide render: the pass `go` selects (null: first hit) over the region, unpacked into the
// caller's arrays. The chain words go through the colour plane c0, which a guide render leaves free.
static void guides_call(rt_camera* cam, const char* who, const rt_region* region, const rt_guide_options* go,
                        float* normal, float* position, float* distance, int32_t* object, int32_t* chain) {
    const RtCamera& C = cam->build.cam;
    const RegionIo io{C.width, dn_region(region, C.width, C.height, who), nullptr};
    DevCtx& c = cam->current();
    c.ensure_device();
    DnBufs& b = c.dn;
    b.ensure((size_t)io.n());
    const DenoiseGuides g{b.gn, b.gp};
    int32_t* d_chain = chain ? reinterpret_cast<int32_t*>(b.c0.p) : nullptr;
    c.launch_guide_pass(io.r, cam->traversal, g, io.stream, go, d_chain);
    hip_check(launch_guides_unpack(g, io.n(), b.nrm(), b.pos(), b.dist(), b.obj, io.stream), "guides_unpack_kernel");
    io.down(normal, b.nrm(), 3 * sizeof(float));
    io.down(position, b.pos(), 3 * sizeof(float));
    io.down(distance, b.dist(), sizeof(float));
    io.down(object, b.obj, sizeof(int32_t));
    io.down(chain, d_chain, sizeof(int32_t));
    hip_check(hipStreamSynchronize(io.stream), "hipStreamSynchronize");
}

extern "C" {

int rt_camera_render_guides(rt_camera* cam, const rt_region* region, float* normal, float* position, float* distance,
                            int32_t* object) {
    return camera_call(cam, [&] {
        guides_call(cam, "rt_camera_render_guides", region, nullptr, normal, position, distance, object, nullptr);
    });
}

void rt_guide_options_default(rt_guide_options* options) {
    if (options) *options = rt_guide_options{RT_GUIDES_FIRST_HIT, 8, 0.0f};
}

int rt_camera_render_guides_ex(rt_camera* cam, const rt_region* region, const rt_guide_options* options, float* normal,
                               float* position, float* distance, int32_t* object, int32_t* chain) {
    return camera_call(cam, [&] {
        const char* who = "rt_camera_render_guides_ex";
        const rt_guide_options go = guide_options(options, who);
        guides_call(cam, who, region, &go, normal, position, distance, object, chain);
    });
}

int rt_camera_set_denoise_guides(rt_camera* cam, const rt_guide_options* options) {
    return camera_call(cam, [&] { cam->dn_guide = guide_options(options, "rt_camera_set_denoise_guides"); });
}

int rt_camera_get_denoise_guides(rt_camera* cam, rt_guide_options* options) {
    if (!options) return set_error(RT_ERR_INVALID, "null argument");
    return camera_call(cam, [&] { *options = cam->dn_guide; });
}

int rt_denoise(int32_t width, int32_t height, const rt_region* region, const rt_denoise_options* options,
               const float* radiance, const float* normal, const float* position, const float* distance,
               const int32_t* object, float* radiance_out, uint8_t* rgb_out) {
    return dn_frame_call("rt_denoise", dn_options(options), width, height, region, radiance, nullptr, normal, position,
                         distance, object, radiance_out, nullptr, rgb_out);
}

int rt_denoise_variance(int32_t width, int32_t height, const rt_region* region, const rt_denoise_var_options* options,
                        const float* radiance, const float* variance, const float* normal, const float* position,
                        const float* distance, const int32_t* object, float* radiance_out, float* variance_out,
                        uint8_t* rgb_out) {
    return dn_frame_call("rt_denoise_variance", dn_options(options), width, height, region, radiance, variance, normal,
                         position, distance, object, radiance_out, variance_out, rgb_out);
}

int rt_camera_denoise(rt_camera* cam, const rt_region* region, const rt_denoise_options* options, const float* radiance,
                      float* radiance_out, uint8_t* rgb_out) {
    return dn_camera_call(cam, "rt_camera_denoise", dn_options(options), region, radiance, nullptr, radiance_out, nullptr,
                          rgb_out);
}

int rt_camera_denoise_variance(rt_camera* cam, const rt_region* region, const rt_denoise_var_options* options,
                               const float* radiance, const float* variance, float* radiance_out, float* variance_out,
                               uint8_t* rgb_out) {
    return dn_camera_call(cam, "rt_camera_denoise_variance", dn_options(options), region, radiance, variance,
                          radiance_out, variance_out, rgb_out);
}

int rt_camera_progressive_denoise(rt_camera* cam, const rt_denoise_options* options, uint8_t* rgb, float* radiance) {
    return dn_session_call(cam, "rt_camera_progressive_denoise", dn_options(options), rgb, radiance, nullptr);
}

int rt_camera_progressive_denoise_variance(rt_camera* cam, const rt_denoise_var_options* options, uint8_t* rgb,
                                           float* radiance, float* variance_out) {
    return dn_session_call(cam, "rt_camera_progressive_denoise_variance", dn_options(options), rgb, radiance,
                           variance_out);
}

int rt_camera_progressive_variance(rt_camera* cam, float* variance) {
    return camera_call(cam, [&] {
        if (!variance) throw std::invalid_argument("rt_camera_progressive_variance: variance is required");
        DevCtx& c = session_with(cam, "rt_camera_progressive_variance", 2);
        const RegionIo io{cam->build.cam.width, c.prog.region, nullptr};
        prog_variance_pass(c, io.stream);
        io.down(variance, c.dn.var, sizeof(float));
        hip_check(hipStreamSynchronize(io.stream), "hipStreamSynchronize");
    });
}

int rt_camera_render_coverage(rt_camera* cam, const rt_region* region, int32_t k, uint32_t* coverage) {
    return camera_call(cam, [&] {
        const std::string who = "rt_camera_render_coverage";
        if (k != 2 && k != 4) throw std::invalid_argument(who + ": k must be 2 or 4");
        if (!coverage) throw std::invalid_argument(who + ": coverage is required");
        const RtCamera& C = cam->build.cam;
        const RegionIo io{C.width, dn_region(region, C.width, C.height, who), nullptr};
        DevCtx& c = cam->current();
        c.ensure_device();
        c.d_cov.ensure((size_t)io.n(), "hipMalloc(coverage)");
        c.launch_coverage_pass(io.r, cam->traversal, k, c.d_cov, nullptr, io.stream);
        io.down(coverage, c.d_cov, sizeof(uint32_t));
        hip_check(hipStreamSynchronize(io.stream), "hipStreamSynchronize");
    });
}

int rt_denoise_hold(int32_t width, int32_t height, const rt_region* region, const rt_denoise_options* options,
                    const float* radiance, const float* normal, const float* position, const float* distance,
                    const int32_t* object, const uint8_t* hold, float* radiance_out, uint8_t* rgb_out) {
    if (!hold) return set_error(RT_ERR_INVALID, "rt_denoise_hold: hold is required");
    return dn_frame_call("rt_denoise_hold", dn_options(options), width, height, region, radiance, nullptr, normal,
                         position, distance, object, radiance_out, nullptr, rgb_out, hold);
}

int rt_denoise_variance_hold(int32_t width, int32_t height, const rt_region* region,
                             const rt_denoise_var_options* options, const float* radiance, const float* variance,
                             const float* normal, const float* position, const float* distance, const int32_t* object,
                             const uint8_t* hold, float* radiance_out, float* variance_out, uint8_t* rgb_out) {
    if (!hold) return set_error(RT_ERR_INVALID, "rt_denoise_variance_hold: hold is required");
    return dn_frame_call("rt_denoise_variance_hold", dn_options(options), width, height, region, radiance, variance,
                         normal, position, distance, object, radiance_out, variance_out, rgb_out, hold);
}

int rt_camera_denoise_hold(rt_camera* cam, const rt_region* region, const rt_denoise_options* options, int32_t hold_k,
                           const float* radiance, float* radiance_out, uint8_t* rgb_out) {
    return dn_camera_call(cam, "rt_camera_denoise_hold", dn_options(options), region, radiance, nullptr, radiance_out,
                          nullptr, rgb_out, hold_k);
}

int rt_camera_denoise_variance_hold(rt_camera* cam, const rt_region* region, const rt_denoise_var_options* options,
                                    int32_t hold_k, const float* radiance, const float* variance, float* radiance_out,
                                    float* variance_out, uint8_t* rgb_out) {
    return dn_camera_call(cam, "rt_camera_denoise_variance_hold", dn_options(options), region, radiance, variance,
                          radiance_out, variance_out, rgb_out, hold_k);
}

int rt_camera_progressive_denoise_hold(rt_camera* cam, const rt_denoise_options* options, int32_t hold_k, uint8_t* rgb,
                                       float* radiance) {
    return dn_session_call(cam, "rt_camera_progressive_denoise_hold", dn_options(options), rgb, radiance, nullptr,
                           hold_k);
}

int rt_camera_progressive_denoise_variance_hold(rt_camera* cam, const rt_denoise_var_options* options, int32_t hold_k,
                                                uint8_t* rgb, float* radiance, float* variance_out) {
    return dn_session_call(cam, "rt_camera_progressive_denoise_variance_hold", dn_options(options), rgb, radiance,
                           variance_out, hold_k);
}

int rt_camera_coverage_time(rt_camera* cam, float* coverage_ms) {
    if (!coverage_ms) return set_error(RT_ERR_INVALID, "null argument");
    return camera_call(cam, [&] {
        DevCtx* c = nullptr;
        for (auto& x : cam->ctxs)
            if (x->cov_timed) c = x.get();
        if (!c) throw std::invalid_argument("rt_camera_coverage_time: no coverage pass yet");
        DeviceScope scope;
        hip_check(hipSetDevice(c->device), "hipSetDevice");
        hip_check(hipEventSynchronize(c->cov_ev[1]), "hipEventSynchronize");
        hip_check(hipEventElapsedTime(coverage_ms, c->cov_ev[0], c->cov_ev[1]), "hipEventElapsedTime");
    });
}

int rt_camera_denoise_times(rt_camera* cam, int32_t* levels, float* guide_ms, float* level_ms, float* total_ms) {
    if (!levels || !guide_ms || !level_ms || !total_ms) return set_error(RT_ERR_INVALID, "null argument");
    return camera_call(cam, [&] {
        DevCtx* c = nullptr;
        for (auto& x : cam->ctxs)
            if (x->dn_levels > 0) c = x.get();
        if (!c) throw std::invalid_argument("rt_camera_denoise_times: no filter call yet");
        DeviceScope scope;
        hip_check(hipSetDevice(c->device), "hipSetDevice");
        const int L = c->dn_levels;
        hipEvent_t* ev = c->dn_ev.data();  // guide [0, 1), pack [1, 2), level l [2 + l, 3 + l), unpack
        hip_check(hipEventSynchronize(ev[L + 3]), "hipEventSynchronize");
        *levels = L;
        *guide_ms = 0.0f;
        if (c->dn_guides) hip_check(hipEventElapsedTime(guide_ms, ev[0], ev[1]), "hipEventElapsedTime");
        for (int l = 0; l < kDenoiseMaxLevels; ++l) {
            level_ms[l] = 0.0f;
            if (l < L) hip_check(hipEventElapsedTime(&level_ms[l], ev[2 + l], ev[3 + l]), "hipEventElapsedTime");
        }
        hip_check(hipEventElapsedTime(total_ms, ev[0], ev[L + 3]), "hipEventElapsedTime");
    });
}

}  // extern "C"
