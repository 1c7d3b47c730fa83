// C ABI of the reprojection through specular chains (reproject_spec.hpp): the through-table
// query and the stand-alone, camera and session calls. Their timings are rt_camera_reproject_times'.
#include <cmath>
#include <cstring>
#include <vector>

#include "pass_host.hpp"
#include "reproject_spec.hpp"

using namespace rt;

// rt_specular_reproject_options resolved: a zero field = the default.
struct RsOpts : SpecOpts {
    RpOpts base;
};
static RsOpts rs_resolve(const rt_specular_reproject_options* o, const std::string& who) {
    rt_specular_reproject_options z{};
    if (o) z = *o;
    const RpOpts base = rp_resolve(&z.base, who);  // (its errors first)
    return RsOpts{spec_resolve(z.point_pixels, z.through, who), base};
}

// The guide options of a call: NULL = the specular walk's defaults; first-hit guides have no chains.
rt_guide_options rt::rs_guide_options(const rt_guide_options* go, const std::string& who) {
    const rt_guide_options dflt{RT_GUIDES_SPECULAR, 8, 0.0f};
    const rt_guide_options g = guide_options(go ? go : &dflt, who);
    if (g.mode != RT_GUIDES_SPECULAR) throw std::invalid_argument(who + ": guide_options must have mode RT_GUIDES_SPECULAR");
    return g;
}

// through[o] = 1 iff SceneData.objects[o]'s material (resolved to a table index by the build) is
// in `mask`: 1 a metal of fuzz <= max_fuzz (the walk's own comparison), 2 glass, 4 mixed, 8 layered.
std::vector<uint8_t> rt::through_objects(const CamHost& h, int32_t mask, float max_fuzz) {
    const SceneBuild& b = h.build;
    std::vector<uint8_t> t((size_t)std::max(b.cam.n_prims, 0), 0);
    for (size_t s = 0; s < b.prims.size() && s < b.prim_object.size(); ++s) {
        const int32_t o = b.prim_object[s], m = b.prims[s].mat;
        if (o < 0 || (size_t)o >= t.size() || m < 0 || (size_t)m >= b.mats.size()) continue;
        const auto& mat = b.mats[m];
        bool ok = false;
        switch (mat.type) {
            case MAT_METAL: ok = (mask & 1) && !(mat.p0 > (double)max_fuzz); break;
            case MAT_GLASS: ok = (mask & 2) != 0; break;
            case MAT_MIXED: ok = (mask & 4) != 0; break;
            case MAT_LAYERED: ok = (mask & 8) != 0; break;
            default: break;
        }
        t[o] = ok;
    }
    return t;
}
static void through_check(const std::string& who, int32_t mask, float max_fuzz) {
    if (mask < 0 || mask > 15) throw std::invalid_argument(who + ": mask must be in 0..15");
    if (!(max_fuzz >= 0.0f) || !std::isfinite(max_fuzz))
        throw std::invalid_argument(who + ": max_fuzz must not be negative and be finite");
}
// The table on the device, rebuilt when the mask or max_fuzz change.
static const uint8_t* ensure_through(DevCtx& c, int32_t mask, float max_fuzz) {
    if (!c.d_through || c.through_mask != mask || c.through_fuzz != max_fuzz) {
        upload_table(c.d_through, through_objects(c.host, mask, max_fuzz), "hipMalloc(through objects)");
        c.through_mask = mask;
        c.through_fuzz = max_fuzz;
    }
    return c.d_through;
}

// (pp * pp) * (du.du / a.a): each product, sum and the division rounded once (this unit is
// compiled without contraction).
float rt::rs_pp2(const RpView& v, float pp) {
    auto dot = [](const float* a, const float* b) {
        const float x = a[0] * b[0], y = a[1] * b[1], z = a[2] * b[2];
        const float xy = x + y;
        return xy + z;
    };
    const float pix2 = dot(v.du, v.du) / dot(v.a, v.a);
    const float p2 = pp * pp;
    return p2 * pix2;
}

// The previous view's guide planes after rp_prev_side walked them.
static RsGuides prev_guides(const DevCtx& p) {
    return RsGuides{p.rp_prev.gn, p.rp_prev.gp, p.rs_prev.sgn, p.rs_prev.sgp, p.rs_prev.chain};
}

extern "C" {

void rt_specular_reproject_options_default(rt_specular_reproject_options* options) {
    if (options) *options = rt_specular_reproject_options{{0.9f, 0.01f, 0.25f, 32.0f}, 4.0f, 15};
}

int rt_camera_through_objects(const rt_camera* cam, int32_t mask, float max_fuzz, uint8_t* out, int32_t capacity) {
    if (!cam || !out) return set_error(RT_ERR_INVALID, "null argument");
    return api_guard([&] {
        through_check("rt_camera_through_objects", mask, max_fuzz);
        const std::vector<uint8_t> t = through_objects(*cam, mask, max_fuzz);
        if ((int64_t)capacity < (int64_t)t.size())
            throw std::invalid_argument("rt_camera_through_objects: capacity below the number of objects");
        if (!t.empty()) std::memcpy(out, t.data(), t.size());
    });
}

int rt_reproject_specular(int32_t width, int32_t height, const rt_region* region, const float* normal,
                          const float* position, const float* distance, const int32_t* object,
                          const float* chain_normal, const float* chain_position, const float* chain_distance,
                          const int32_t* chain_object, const int32_t* chain, const rt_view* view,
                          const rt_view* prev_view, const rt_region* prev_region, const float* prev_radiance,
                          const float* prev_normal, const float* prev_position, const float* prev_distance,
                          const int32_t* prev_object, const float* prev_chain_normal, const float* prev_chain_position,
                          const float* prev_chain_distance, const int32_t* prev_chain_object, const int32_t* prev_chain,
                          const uint8_t* reusable, const uint8_t* through, int32_t n_objects,
                          const rt_specular_reproject_options* options, const float* radiance, const int32_t* px_samples,
                          int32_t samples, float* history_out, float* weight_out, float* radiance_out, uint8_t* rgb_out,
                          uint8_t* kind_out) {
    return api_guard([&] {
        const std::string who = "rt_reproject_specular";
        if (width <= 0 || height <= 0) throw std::invalid_argument(who + ": width and height must be positive");
        if (!normal || !position || !distance || !object)
            throw std::invalid_argument(who + ": normal, position, distance and object are required");
        if (!chain_normal || !chain_position || !chain_distance || !chain_object || !chain)
            throw std::invalid_argument(who + ": chain_normal, chain_position, chain_distance, chain_object and chain are required");
        if (!view) throw std::invalid_argument(who + ": view is required");
        if (!prev_view || !prev_normal || !prev_position || !prev_distance || !prev_object)
            throw std::invalid_argument(who + ": prev_view, prev_normal, prev_position, prev_distance and prev_object are required");
        if (!prev_chain_normal || !prev_chain_position || !prev_chain_distance || !prev_chain_object || !prev_chain)
            throw std::invalid_argument(who + ": prev_chain_normal, prev_chain_position, prev_chain_distance, "
                                              "prev_chain_object and prev_chain are required");
        if (prev_view->width <= 0 || prev_view->height <= 0)
            throw std::invalid_argument(who + ": the previous view's width and height must be positive");
        if (n_objects < 0 || (n_objects > 0 && (!reusable || !through)))
            throw std::invalid_argument(who + ": reusable and through must hold n_objects >= 0 entries");
        rp_check(who, prev_radiance, radiance, samples, radiance_out, rgb_out);
        const RsOpts o = rs_resolve(options, who);
        const hipStream_t stream = nullptr;
        const RegionIo io{width, dn_region(region, width, height, who), stream};
        const RegionIo pio{prev_view->width, dn_region(prev_region, prev_view->width, prev_view->height, who), stream};
        const RpView pv = rp_view_constants(prev_view->center, prev_view->pixel00, prev_view->du, prev_view->dv,
                                            prev_view->width, prev_view->height);
        // (ns / ps: the chain guides' pairs, their obj planes the chain words, ns.u8 the kind plane)
        DnBufs nb, pb, ns, ps;
        DevBuf<uint8_t> d_reusable, d_through;
        upload_reusable(d_reusable, reusable, n_objects, stream);
        upload_reusable(d_through, through, n_objects, stream);
        RsGuides ng, pg;
        upload_views(nb, ns, io, {normal, position, distance, object, chain_normal, chain_position, chain_distance, chain_object, chain},
                     pb, ps, pio, {prev_normal, prev_position, prev_distance, prev_object, prev_chain_normal, prev_chain_position,
                                   prev_chain_distance, prev_chain_object, prev_chain}, &ng, &pg);
        // (the guides are packed: the staging arrays now carry the frames and the counts)
        pio.up(pb.rad(), prev_radiance, 3 * sizeof(float));
        if (radiance) io.up(nb.rad(), radiance, 3 * sizeof(float));
        if (radiance && px_samples) io.up(nb.obj, px_samples, sizeof(int32_t));
        const RpNew nw{nb.gn, nb.gp, radiance ? nb.rad() : nullptr, radiance && px_samples ? nb.obj.p : nullptr,
                       io.r.width, 0, 0, (float)samples};
        const RpChain ch{ng, pg, view->center, d_through, o.point_pixels, ns.u8, kind_out != nullptr};
        rp_run(nb, pb, pv, io.r, pio.r, d_reusable, n_objects, o.base, nw, history_out || weight_out,
               radiance_out != nullptr, rgb_out != nullptr, stream, nullptr, &ch);
        rp_outputs(nb, io, history_out, weight_out, radiance_out, rgb_out, kind_out, ns.u8);
    });
}

int rt_camera_reproject_specular(rt_camera* cam, const rt_region* region, rt_camera* prev_cam,
                                 const rt_region* prev_region, const rt_guide_options* guide_options_,
                                 const rt_specular_reproject_options* options, const float* prev_radiance,
                                 const float* radiance, const int32_t* px_samples, int32_t samples, float* history_out,
                                 float* weight_out, float* radiance_out, uint8_t* rgb_out, uint8_t* kind_out) {
    return two_camera_call(cam, prev_cam, [&] {
        const std::string who = "rt_camera_reproject_specular";
        const RtCamera &C = cam->build.cam, &PC = prev_cam->build.cam;
        rp_check(who, prev_radiance, radiance, samples, radiance_out, rgb_out);
        const RsOpts o = rs_resolve(options, who);
        const rt_guide_options go = rs_guide_options(guide_options_, who);
        const hipStream_t stream = nullptr;
        const RegionIo io{C.width, dn_region(region, C.width, C.height, who), stream};
        const rt_region pr = dn_region(prev_region, PC.width, PC.height, who);
        rp_same_scene(cam, prev_cam);
        DevCtx& c = cam->current();
        c.ensure_device();
        DnBufs& nb = c.dn;
        nb.ensure((size_t)io.n());
        c.rs.ensure((size_t)io.n());
        hipEvent_t* ev = c.rp_events();
        const uint8_t* d_reusable = c.ensure_reusable();
        const uint8_t* d_through = ensure_through(c, o.through, go.max_fuzz);
        if (radiance) io.up(nb.rad(), radiance, 3 * sizeof(float));
        if (radiance && px_samples) io.up(nb.obj, px_samples, sizeof(int32_t));
        DevCtx& p = rp_prev_side(prev_cam, pr, prev_radiance, stream, ev, [&] {
            c.launch_guide_pass(io.r, cam->traversal, DenoiseGuides{nb.gn, nb.gp}, stream);
            c.launch_guide_pass(io.r, cam->traversal, DenoiseGuides{c.rs.sgn, c.rs.sgp}, stream, &go, c.rs.chain);
        }, &go);
        const RpNew nw{nb.gn, nb.gp, radiance ? nb.rad() : nullptr, radiance && px_samples ? nb.obj.p : nullptr,
                       io.r.width, 0, 0, (float)samples};
        const RpChain ch{{nb.gn, nb.gp, c.rs.sgn, c.rs.sgp, c.rs.chain}, prev_guides(p), C.center, d_through,
                         o.point_pixels, c.rs.kind, kind_out != nullptr};
        rp_run(nb, p.rp_prev, rp_camera_view(prev_cam), io.r, pr, d_reusable, C.n_prims, o.base, nw,
               history_out || weight_out, radiance_out != nullptr, rgb_out != nullptr, stream, ev, &ch);
        c.rp_timed = true;
        rp_outputs(nb, io, history_out, weight_out, radiance_out, rgb_out, kind_out, c.rs.kind);
    });
}

int rt_camera_progressive_reproject_specular(rt_camera* cam, rt_camera* prev_cam, const rt_region* prev_region,
                                             const rt_guide_options* guide_options_,
                                             const rt_specular_reproject_options* options, const float* prev_radiance,
                                             uint8_t* rgb, float* radiance, float* weight_out, uint8_t* kind_out) {
    return two_camera_call(cam, prev_cam, [&] {
        const std::string who = "rt_camera_progressive_reproject_specular";
        (void)cam->session(who.c_str());
        session_radiance(cam, who);
        rp_check(who, prev_radiance, nullptr, 0, nullptr, nullptr);
        const RsOpts o = rs_resolve(options, who);
        const rt_guide_options go = rs_guide_options(guide_options_, who);
        const RtCamera &C = cam->build.cam, &PC = prev_cam->build.cam;
        const rt_region pr = dn_region(prev_region, PC.width, PC.height, who);
        rp_same_scene(cam, prev_cam);
        DevCtx& c = session_with(cam, who, 0);
        DevCtx::ProgSession& P = c.prog;
        const hipStream_t stream = nullptr;
        const RegionIo io{C.width, P.region, stream};
        DnBufs& nb = c.dn;
        nb.ensure((size_t)io.n());
        c.rs.kind.ensure((size_t)io.n(), "hipMalloc(chain guides)");
        hipEvent_t* ev = c.rp_events();
        const uint8_t* d_reusable = c.ensure_reusable();
        const uint8_t* d_through = ensure_through(c, o.through, go.max_fuzz);
        DevCtx& p = rp_prev_side(prev_cam, pr, prev_radiance, stream, ev, [&] {
            session_guides(cam, c, stream);
            session_specular_guides(cam, c, go, stream, true);
        }, &go);
        const RpNew nw{P.d_gn, P.d_gp, P.d_rad, P.d_pxs, C.width, io.r.x, io.r.y, 0.0f};
        const RpChain ch{{P.d_gn, P.d_gp, P.d_sgn, P.d_sgp, P.d_sch}, prev_guides(p), C.center, d_through, o.point_pixels,
                         c.rs.kind, kind_out != nullptr};
        rp_run(nb, p.rp_prev, rp_camera_view(prev_cam), io.r, pr, d_reusable, C.n_prims, o.base, nw, weight_out != nullptr,
               radiance != nullptr, rgb != nullptr, stream, ev, &ch);
        c.rp_timed = true;
        rp_outputs(nb, io, nullptr, weight_out, radiance, rgb, kind_out, c.rs.kind);
    });
}

}  // extern "C"
