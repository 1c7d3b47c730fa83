// The frame passes' shared host side (pass_host.hpp).
#include "pass_host.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace rt {

float resolve_field(float v, float dflt, const std::string& who, const char* name) {
    if (!(v >= 0.0f) || !std::isfinite(v))
        throw std::invalid_argument(who + ": " + name + " must be positive and finite (0: the default)");
    return v == 0.0f ? dflt : v;
}

GatherOpts gather_resolve(float normal_min, float sigma_plane, float min_weight, const std::string& who) {
    GatherOpts o;
    o.normal_min = resolve_field(normal_min, 0.9f, who, "normal_min");
    o.sigma_plane = resolve_field(sigma_plane, 0.01f, who, "sigma_plane");
    o.min_weight = resolve_field(min_weight, 0.25f, who, "min_weight");
    return o;
}

RpOpts rp_resolve(const rt_reproject_options* o, const std::string& who) {
    const rt_reproject_options z = o ? *o : rt_reproject_options{0.0f, 0.0f, 0.0f, 0.0f};
    RpOpts r{gather_resolve(z.normal_min, z.sigma_plane, z.min_weight, who), 0.0f};
    r.nh = resolve_field(z.history_samples, 32.0f, who, "history_samples");
    return r;
}

void rp_check(const std::string& who, const float* prev_radiance, const float* radiance, int32_t samples,
              const float* radiance_out, const uint8_t* rgb_out) {
    if (!prev_radiance) throw std::invalid_argument(who + ": prev_radiance is required");
    if ((radiance_out || rgb_out) && !radiance)
        throw std::invalid_argument(who + ": radiance_out and rgb_out need a fresh radiance to blend");
    if (samples < 0) throw std::invalid_argument(who + ": samples must not be negative");
}

template <class T>
static bool same_bytes(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}
void rp_same_scene(const rt_camera* a, const rt_camera* b) {
    const SceneBuild &x = a->build, &y = b->build;
    if (a != b && !(same_bytes(x.nodes, y.nodes) && same_bytes(x.prims, y.prims) && same_bytes(x.mats, y.mats) &&
                    same_bytes(x.lights, y.lights) && same_bytes(x.prim_object, y.prim_object)))
        throw std::invalid_argument("reproject: the cameras hold different scenes");
}

constexpr long kDenoiseMaxPixels = 1l << 28;
rt_region dn_region(const rt_region* region, int32_t width, int32_t height, const std::string& who) {
    const rt_region r = clamp_region(region ? *region : rt_region{0, 0, width, height}, width, height);
    if (region_empty(r)) throw std::invalid_argument(who + ": the region is empty after clamping to the image");
    if ((long)r.width * r.height > kDenoiseMaxPixels) throw std::invalid_argument(who + ": the region has too many pixels");
    return r;
}

void RegionIo::up(void* dev, const void* host, size_t elem) const {
    const size_t off = ((size_t)r.y * width + r.x) * elem;
    hip_check(hipMemcpy2DAsync(dev, (size_t)r.width * elem, (const char*)host + off, (size_t)width * elem,
                               (size_t)r.width * elem, r.height, hipMemcpyHostToDevice, stream),
              "hipMemcpy2DAsync");
}
void RegionIo::down(void* host, const void* dev, size_t elem) const {
    if (!host) return;
    const size_t off = ((size_t)r.y * width + r.x) * elem;
    hip_check(hipMemcpy2DAsync((char*)host + off, (size_t)width * elem, dev, (size_t)r.width * elem,
                               (size_t)r.width * elem, r.height, hipMemcpyDeviceToHost, stream),
              "hipMemcpy2DAsync");
}

void upload_guides(DnBufs& b, const RegionIo& io, const float* normal, const float* position, const float* distance,
                   const int32_t* object) {
    io.up(b.nrm(), normal, 3 * sizeof(float));
    io.up(b.pos(), position, 3 * sizeof(float));
    io.up(b.dist(), distance, sizeof(float));
    io.up(b.obj, object, sizeof(int32_t));
    hip_check(launch_guides_pack(DenoiseGuides{b.gn, b.gp}, io.n(), b.nrm(), b.pos(), b.dist(), b.obj, io.stream),
              "guides_pack_kernel");
}

void upload_views(DnBufs& nb, DnBufs& ns, const RegionIo& io, const HostGuides& g, DnBufs& pb, DnBufs& ps,
                  const RegionIo& pio, const HostGuides& pg, RsGuides* ng, RsGuides* pgd) {
    struct V {
        DnBufs &b, &s;
        const RegionIo& io;
        const HostGuides& g;
    } views[] = {{nb, ns, io, g}, {pb, ps, pio, pg}};
    for (V& v : views) {
        v.b.ensure((size_t)v.io.n());
        if (v.g.chain_normal) v.s.ensure((size_t)v.io.n());
    }
    for (V& v : views) {
        upload_guides(v.b, v.io, v.g.normal, v.g.position, v.g.distance, v.g.object);
        if (v.g.chain_normal)
            upload_guides(v.s, v.io, v.g.chain_normal, v.g.chain_position, v.g.chain_distance, v.g.chain_object);
    }
    // (the chain guides are packed: their object planes now carry the chain words)
    for (V& v : views)
        if (v.g.chain_normal) v.io.up(v.s.obj, v.g.chain, sizeof(int32_t));
    *ng = g.chain_normal ? RsGuides{nb.gn, nb.gp, ns.gn, ns.gp, ns.obj} : RsGuides{nb.gn, nb.gp, nullptr, nullptr, nullptr};
    *pgd = pg.chain_normal ? RsGuides{pb.gn, pb.gp, ps.gn, ps.gp, ps.obj} : RsGuides{pb.gn, pb.gp, nullptr, nullptr, nullptr};
}

void upload_reusable(DevBuf<uint8_t>& d, const uint8_t* reusable, int32_t n_objects, hipStream_t stream) {
    d.ensure((size_t)std::max(n_objects, 1), "hipMalloc(reusable objects)");
    if (n_objects > 0)
        hip_check(hipMemcpyAsync(d, reusable, (size_t)n_objects, hipMemcpyHostToDevice, stream), "hipMemcpyAsync");
}

void upload_table(DevBuf<uint8_t>& d, std::vector<uint8_t> t, const char* what) {
    t.resize(std::max<size_t>(t.size(), 1), 0);
    d.ensure(t.size(), what);
    hip_check(hipMemcpy(d, t.data(), t.size(), hipMemcpyHostToDevice), "hipMemcpy");
}

SpecOpts spec_resolve(float point_pixels, int32_t through, const std::string& who) {
    SpecOpts r{resolve_field(point_pixels, 4.0f, who, "point_pixels"), 0};
    if (through < 0 || through > 15) throw std::invalid_argument(who + ": through must be a mask in 0..15 (0: the default, 15)");
    r.through = through ? through : 15;
    return r;
}

void session_radiance(rt_camera* cam, const std::string& who) {
    if (cam->build.cam.mode != MODE_DEFAULT)
        throw std::invalid_argument(who + ": the frames of mode bounces / samples are not radiance");
}

DevCtx& session_host(rt_camera* cam, const std::string& who, int min_samples) {
    DevCtx& c = cam->session(who.c_str());
    session_radiance(cam, who);
    if (c.prog.done < min_samples)
        throw std::invalid_argument(who + ": a variance needs at least 2 samples per pixel, the session has " +
                                    std::to_string(c.prog.done) + " (samples_done < 2)");
    return c;
}

void session_on_device(const DevCtx& c, const std::string& who) {
    int dev = 0;
    hip_check(hipGetDevice(&dev), "hipGetDevice");
    if (dev != c.device) throw std::invalid_argument(who + ": the session lives on another device");
}

DevCtx& session_with(rt_camera* cam, const std::string& who, int min_samples) {
    DevCtx& c = session_host(cam, who, min_samples);
    session_on_device(c, who);
    return c;
}

void session_guides(rt_camera* cam, DevCtx& c, hipStream_t stream) {
    DevCtx::ProgSession& P = c.prog;
    if (P.d_gn) return;
    const size_t n = (size_t)P.region.width * P.region.height;
    try {
        P.d_gn.ensure(n, "hipMalloc(session guides)");
        P.d_gp.ensure(n, "hipMalloc(session guides)");
        c.launch_guide_pass(P.region, cam->traversal, DenoiseGuides{P.d_gn, P.d_gp}, stream);
    } catch (...) {
        P.d_gn.reset();
        P.d_gp.reset();
        throw;
    }
}

rt_guide_options guide_options(const rt_guide_options* o, const std::string& who) {
    rt_guide_options g;
    rt_guide_options_default(&g);
    if (o) g = *o;
    if (g.mode != RT_GUIDES_FIRST_HIT && g.mode != RT_GUIDES_SPECULAR)
        throw std::invalid_argument(who + ": mode must be RT_GUIDES_FIRST_HIT or RT_GUIDES_SPECULAR");
    if (g.max_bounces < 1 || g.max_bounces > 64) throw std::invalid_argument(who + ": max_bounces must be 1..64");
    if (!(g.max_fuzz >= 0.0f) || !std::isfinite(g.max_fuzz))
        throw std::invalid_argument(who + ": max_fuzz must not be negative and be finite");
    return g;
}

bool session_specular_cached(const DevCtx& c, const rt_guide_options& go, bool want_chain) {
    const DevCtx::ProgSession& P = c.prog;
    return P.sg_valid && P.sg_key.max_bounces == go.max_bounces && P.sg_key.max_fuzz == go.max_fuzz &&
           (!want_chain || P.sch_valid);
}

void session_specular_guides(rt_camera* cam, DevCtx& c, const rt_guide_options& go, hipStream_t stream, bool want_chain) {
    DevCtx::ProgSession& P = c.prog;
    if (session_specular_cached(c, go, want_chain)) return;
    const size_t n = (size_t)P.region.width * P.region.height;
    P.sg_valid = P.sch_valid = false;
    P.d_sgn.ensure(n, "hipMalloc(session guides)");
    P.d_sgp.ensure(n, "hipMalloc(session guides)");
    if (want_chain) P.d_sch.ensure(n, "hipMalloc(session guides)");
    c.launch_guide_pass(P.region, cam->traversal, DenoiseGuides{P.d_sgn, P.d_sgp}, stream, &go,
                        want_chain ? P.d_sch.p : nullptr);
    P.sg_key = go;
    P.sg_valid = true;
    P.sch_valid = want_chain;
}

void prog_variance_pass(DevCtx& c, hipStream_t stream) {
    DevCtx::ProgSession& P = c.prog;
    c.dn.var.ensure((size_t)P.region.width * P.region.height, "hipMalloc(denoise variance)");
    const int tiles_x = std::max((P.region.width + kTile - 1) / kTile, 1);
    hip_check(launch_prog_variance(P.d_state, (int)P.slots, c.prog_reg(), tiles_x, c.dn.var, stream),
              "prog_variance_kernel");
}

void prog_copy_out(const DevCtx& c, void* host, const void* dev, size_t elem, hipStream_t stream) {
    if (!host) return;
    const rt_region& r = c.prog.region;
    const size_t pitch = (size_t)c.build.cam.width * elem;
    const size_t off = ((size_t)r.y * c.build.cam.width + r.x) * elem;
    hip_check(hipMemcpy2DAsync((char*)host + off, pitch, (const char*)dev + off, pitch, (size_t)r.width * elem, r.height,
                               hipMemcpyDeviceToHost, stream),
              "hipMemcpy2DAsync");
}

void hold_check(int32_t hold_k, const std::string& who) {
    if (hold_k != 0 && hold_k != 2 && hold_k != 4) throw std::invalid_argument(who + ": hold_k must be 0, 2 or 4");
}

void dn_filter(DnBufs& b, const float4* gn, const float4* gp, const float* rad, int pitch_px, int x0, int y0, int w,
               int h, const DnOpts& o, bool want_rad, bool want_u8, bool want_var, hipStream_t stream, hipEvent_t* ev,
               const uint8_t* hold) {
    int e = 0;
    auto mark = [&] {
        if (ev) hip_check(hipEventRecord(ev[e++], stream), "hipEventRecord");
    };
    mark();
    hip_check(launch_denoise_pack(rad, pitch_px, x0, y0, w, h, gn, o.sigma_plane, o.var ? b.var.p : nullptr, b.c0, b.fn,
                                  stream),
              "denoise_pack_kernel");
    mark();
    // the level's scalar, in double on the host, rounded to fp32 once: sigma_variance^2, or
    // 4^level / sigma_color^2
    const double s2 = (double)o.sigma * (double)o.sigma;
    float4 *src = b.c0, *dst = b.c1;
    for (int lv = 0; lv < o.levels; ++lv) {
        const float ks = (float)(o.var ? s2 : std::ldexp(1.0, 2 * lv) / s2);
        hip_check(launch_denoise_level(o.var, src, dst, b.fn, gp, w, h, 1 << lv, ks, stream), "denoise kernel");
        mark();
        std::swap(src, dst);
    }
    hip_check(launch_denoise_unpack(src, w * h, want_rad ? b.rad() : nullptr, want_u8 ? b.u8.p : nullptr,
                                    o.var && want_var ? b.var.p : nullptr, stream,
                                    DenoiseHold{hold, rad, pitch_px, x0, y0, w, o.var ? b.var.p : nullptr}),
              "denoise_unpack_kernel");
    mark();
}

}  // namespace rt
