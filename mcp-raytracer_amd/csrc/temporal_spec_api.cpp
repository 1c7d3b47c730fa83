// C ABI of the accumulation across views through specular chains (temporal_spec.hpp): the options,
// the history's chain-guide query and the session and stand-alone accumulate calls. The history
// object, its read-back and its timings are api_temporal.cpp's.
#include <algorithm>
#include <cstring>
#include <vector>

#include "pass_host.hpp"
#include "temporal_spec.hpp"

using namespace rt;

// rt_specular_temporal_options resolved: a zero field = the default.
struct TsOpts : SpecOpts {
    TpOpts base;
};
static TsOpts ts_resolve(const rt_specular_temporal_options* o, const std::string& who) {
    rt_specular_temporal_options z{};
    if (o) z = *o;
    const TpOpts base = tp_resolve(&z.base, who);  // (its errors first)
    return TsOpts{spec_resolve(z.point_pixels, z.through, who), base};
}

static bool same_bits(float a, float b) { return std::memcmp(&a, &b, sizeof(float)) == 0; }

// The device side of a call: the gather and blend into out_col / out_var (weight -> b.dist(), kind
// -> d_kind), then tp_finish with the new view's CHAIN guides as the filter's. pr.width == 0: an
// empty history. Queued.
static void ts_run(DnBufs& b, const RsGuides& ng, const TpNew& nw, const float* cn, const rt_region& r,
                   const TsHistory& hist, bool chain_history, const RpView& view, const rt_region& pr,
                   const uint8_t* d_reusable, const uint8_t* d_through, int n_objects, const TsOpts& o, float4* out_col,
                   float* out_var, uint8_t* d_kind, bool want_rad, bool want_u8, bool want_var, bool want_len,
                   hipStream_t stream, hipEvent_t* ev) {
    TsArgs a = gather_args<TsArgs>(view, r, pr, n_objects, o.base, nw);
    a.max_history = o.base.max_history;
    a.vpitch = r.width, a.vx0 = 0, a.vy0 = 0;
    a.chain_history = chain_history ? 1 : 0;
    a.pp2 = pr.width > 0 ? rs_pp2(view, o.point_pixels) : 0.0f;
    for (int k = 0; k < 3; ++k) a.cn[k] = cn[k];
    hip_check(launch_temporal_spec(a, ng, hist, d_reusable, d_through, nw.fresh, nw.pxs, nw.var,
                                   TpOut{out_col, out_var, b.dist()}, d_kind, stream),
              "temporal_spec_kernel");
    tp_finish(b, ng.sgn, ng.sgp, r, o.base, out_col, out_var, want_rad, want_u8, want_var, want_len, stream, ev);
}

extern "C" {

void rt_specular_temporal_options_default(rt_specular_temporal_options* options) {
    if (options) *options = rt_specular_temporal_options{{0.9f, 0.01f, 0.25f, 256.0f, 0, 2.0f}, 4.0f, 15};
}

int rt_history_chain_guides(const rt_history* h, rt_guide_options* out, int32_t* held) {
    if (!h || !out || !held) return set_error(RT_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lock(const_cast<rt_history*>(h)->mu);
    const rt_history::Side& s = h->side[h->front];
    *held = h->views > 0 && s.has_chain ? 1 : 0;
    *out = *held ? s.chain_go : rt_guide_options{RT_GUIDES_SPECULAR, 0, 0.0f};
    return RT_OK;
}

int rt_camera_progressive_accumulate_specular(rt_camera* cam, rt_history* h, const rt_guide_options* guide_options_,
                                              const rt_specular_temporal_options* options, int32_t commit, uint8_t* rgb,
                                              float* radiance, float* variance_out, float* length_out, float* weight_out,
                                              uint8_t* kind_out) {
    if (!h) return set_error(RT_ERR_INVALID, "null history");
    std::lock_guard<std::mutex> hlock(h->mu);
    return camera_call(cam, [&] {
        const std::string who = "rt_camera_progressive_accumulate_specular";
        const TsOpts o = ts_resolve(options, who);
        const rt_guide_options go = rs_guide_options(guide_options_, who);
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
        if (commit) back.ensure_chain(n);
        if (!h->d_reusable || h->views == 0) {  // (an uncommitted call may have been another scene's)
            std::vector<uint8_t> t = cam->reusable_objects();
            h->n_objects = (int32_t)t.size();
            upload_table(h->d_reusable, std::move(t), "hipMalloc(reusable objects)");
        }
        if (!h->d_through || h->views == 0 || h->through_mask != o.through || !same_bits(h->through_fuzz, go.max_fuzz)) {
            upload_table(h->d_through, through_objects(*cam, o.through, go.max_fuzz), "hipMalloc(through objects)");
            h->through_mask = o.through;
            h->through_fuzz = go.max_fuzz;
        }
        DnBufs& b = c.dn;
        b.ensure(n);
        c.rs.kind.ensure(n, "hipMalloc(chain guides)");
        hip_check(hipEventRecord(h->ev[0], stream), "hipEventRecord");
        session_guides(cam, c, stream);
        session_specular_guides(cam, c, go, stream, true);
        prog_variance_pass(c, stream);
        hip_check(hipEventRecord(h->ev[1], stream), "hipEventRecord");
        const bool has = h->views > 0;
        // the history's chain planes serve only when they were walked with these very options
        const bool chain_history = has && front.has_chain && front.chain_go.max_bounces == go.max_bounces &&
                                   same_bits(front.chain_go.max_fuzz, go.max_fuzz);
        TsHistory hist{};
        if (has) hist = TsHistory{{front.gn, front.gp, nullptr, nullptr, nullptr}, front.col, front.var};
        if (chain_history) hist.g = RsGuides{front.gn, front.gp, front.sgn, front.sgp, front.chain};
        const rt_region pr = has ? h->region : rt_region{0, 0, 0, 0};
        const TpNew nw{{P.d_gn, P.d_gp, P.d_rad, P.d_pxs, C.width, r.x, r.y, 0.0f}, b.var};
        const RsGuides ng{P.d_gn, P.d_gp, P.d_sgn, P.d_sgp, P.d_sch};
        ts_run(b, ng, nw, C.center, r, hist, chain_history, h->rp_view, pr, h->d_reusable, h->d_through, h->n_objects, o,
               back.col, back.var, c.rs.kind, radiance != nullptr, rgb != nullptr, variance_out != nullptr,
               length_out != nullptr, stream, h->ev);
        if (commit) {
            // the session may be gone before the next view: the history keeps the guides itself
            float4* const dst[] = {back.gn, back.gp, back.sgn, back.sgp};
            const float4* const src[] = {P.d_gn, P.d_gp, P.d_sgn, P.d_sgp};
            for (int k = 0; k < 4; ++k)
                hip_check(hipMemcpyAsync(dst[k], src[k], n * sizeof(float4), hipMemcpyDeviceToDevice, stream), "hipMemcpyAsync");
            hip_check(hipMemcpyAsync(back.chain, P.d_sch, n * sizeof(int32_t), hipMemcpyDeviceToDevice, stream), "hipMemcpyAsync");
            back.has_chain = true;
            back.chain_go = go;
        }
        hip_check(hipEventRecord(h->ev[4], stream), "hipEventRecord");
        h->timed = true;
        h->filtered = o.base.levels > 0 && (radiance || rgb || variance_out);
        io.down(kind_out, c.rs.kind, 1);
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

int rt_temporal_accumulate_specular(
    int32_t width, int32_t height, const rt_region* region, const float* normal, const float* position,
    const float* distance, const int32_t* object, const float* chain_normal, const float* chain_position,
    const float* chain_distance, const int32_t* chain_object, const int32_t* chain, const rt_view* view,
    const float* radiance, const int32_t* px_samples, int32_t samples, const float* variance, const rt_view* prev_view,
    const rt_region* prev_region, const float* prev_normal, const float* prev_position, const float* prev_distance,
    const int32_t* prev_object, const float* prev_chain_normal, const float* prev_chain_position,
    const float* prev_chain_distance, const int32_t* prev_chain_object, const int32_t* prev_chain,
    const float* prev_radiance, const float* prev_variance, const float* prev_length, const uint8_t* reusable,
    const uint8_t* through, int32_t n_objects, const rt_specular_temporal_options* options, float* radiance_out,
    float* variance_out, float* length_out, float* weight_out, uint8_t* rgb_out, uint8_t* kind_out) {
    return api_guard([&] {
        const std::string who = "rt_temporal_accumulate_specular";
        if (width <= 0 || height <= 0) throw std::invalid_argument(who + ": width and height must be positive");
        if (!normal || !position || !distance || !object || !radiance || !variance)
            throw std::invalid_argument(who + ": normal, position, distance, object, radiance and variance are required");
        if (!chain_normal || !chain_position || !chain_distance || !chain_object || !chain)
            throw std::invalid_argument(who + ": chain_normal, chain_position, chain_distance, chain_object and chain are required");
        if (!view) throw std::invalid_argument(who + ": view is required");
        if (!prev_view || !prev_normal || !prev_position || !prev_distance || !prev_object || !prev_radiance ||
            !prev_variance || !prev_length)
            throw std::invalid_argument(who + ": prev_view, prev_normal, prev_position, prev_distance, prev_object, "
                                              "prev_radiance, prev_variance and prev_length are required");
        const int pc = (prev_chain_normal != nullptr) + (prev_chain_position != nullptr) + (prev_chain_distance != nullptr) +
                       (prev_chain_object != nullptr) + (prev_chain != nullptr);
        if (pc != 0 && pc != 5)
            throw std::invalid_argument(who + ": prev_chain_normal, prev_chain_position, prev_chain_distance, "
                                              "prev_chain_object and prev_chain must be all given or all NULL "
                                              "(NULL: the history holds no chain planes)");
        if (prev_view->width <= 0 || prev_view->height <= 0)
            throw std::invalid_argument(who + ": the previous view's width and height must be positive");
        if (n_objects < 0 || (n_objects > 0 && (!reusable || !through)))
            throw std::invalid_argument(who + ": reusable and through must hold n_objects >= 0 entries");
        if (samples < 0) throw std::invalid_argument(who + ": samples must not be negative");
        const TsOpts o = ts_resolve(options, who);
        const bool chain_history = pc == 5;
        const hipStream_t stream = nullptr;
        const RegionIo io{width, dn_region(region, width, height, who), stream};
        const RegionIo pio{prev_view->width, dn_region(prev_region, prev_view->width, prev_view->height, who), stream};
        const RpView pv = rp_view_constants(prev_view->center, prev_view->pixel00, prev_view->du, prev_view->dv,
                                            prev_view->width, prev_view->height);
        const size_t n = (size_t)io.n(), np = (size_t)pio.n();
        // (ns / ps: the chain guides' pairs, their obj planes the chain words, ns.u8 the kind plane)
        DnBufs nb, pb, ns, ps;
        rt_history::Side out;
        DevBuf<float> d_var;
        DevBuf<uint8_t> d_reusable, d_through;
        nb.ensure(n);
        ns.ensure(n);
        pb.ensure(np);
        if (chain_history) ps.ensure(np);
        pb.var.ensure(np, "hipMalloc(history)");
        out.ensure(n);
        d_var.ensure(n, "hipMalloc(denoise variance)");
        upload_reusable(d_reusable, reusable, n_objects, stream);
        upload_reusable(d_through, through, n_objects, stream);
        upload_guides(nb, io, normal, position, distance, object);
        upload_guides(ns, io, chain_normal, chain_position, chain_distance, chain_object);
        upload_guides(pb, pio, prev_normal, prev_position, prev_distance, prev_object);
        if (chain_history) upload_guides(ps, pio, prev_chain_normal, prev_chain_position, prev_chain_distance, prev_chain_object);
        // (the guides are packed: the staging arrays now carry the chain words, the frames, the length and the counts)
        io.up(ns.obj, chain, sizeof(int32_t));
        if (chain_history) pio.up(ps.obj, prev_chain, sizeof(int32_t));
        pio.up(pb.rad(), prev_radiance, 3 * sizeof(float));
        pio.up(pb.dist(), prev_length, sizeof(float));
        pio.up(pb.var, prev_variance, sizeof(float));
        hip_check(launch_temporal_pack(pb.rad(), pb.dist(), (int)np, pb.c0, stream), "temporal_pack_kernel");
        io.up(nb.pos(), radiance, 3 * sizeof(float));
        io.up(d_var, variance, sizeof(float));
        if (px_samples) io.up(nb.obj, px_samples, sizeof(int32_t));
        const TpNew nw{{nb.gn, nb.gp, nb.pos(), px_samples ? nb.obj.p : nullptr, io.r.width, 0, 0, (float)samples}, d_var};
        const RsGuides ng{nb.gn, nb.gp, ns.gn, ns.gp, ns.obj};
        TsHistory hist{{pb.gn, pb.gp, nullptr, nullptr, nullptr}, pb.c0, pb.var};
        if (chain_history) hist.g = RsGuides{pb.gn, pb.gp, ps.gn, ps.gp, ps.obj};
        ts_run(nb, ng, nw, view->center, io.r, hist, chain_history, pv, pio.r, d_reusable, d_through, n_objects, o, out.col,
               out.var, ns.u8, radiance_out != nullptr, rgb_out != nullptr, variance_out != nullptr, length_out != nullptr,
               stream, nullptr);
        io.down(kind_out, ns.u8, 1);
        tp_outputs(nb, io, radiance_out, rgb_out, variance_out, length_out, weight_out);
    });
}

}  // extern "C"
