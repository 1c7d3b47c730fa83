// What the frame passes' ABI units (api_denoise / api_reproject / api_temporal / api_focus.cpp and
// the two *_spec_api.cpp) share on the host: option fields, the region check and its copies, the
// guide and reusable-table uploads, the open session's checks and passes, the filter's launch
// sequence, the common head of the gather kernels' arguments, and the reprojection's and the
// accumulation's run, session and stand-alone bodies, each with an optional chain argument.
#pragma once

#include <functional>
#include <string>
#include <vector>

#include "api_call.hpp"
#include "reproject_spec.hpp"

namespace rt {

// An option field where zero means `dflt`: anything else must not be negative and be finite.
float resolve_field(float v, float dflt, const std::string& who, const char* name);

// The fields of rt_denoise_options / rt_denoise_var_options as the caller gave them; var: the
// variance-guided filter, whose sigma is sigma_variance (the plain one's: sigma_color).
struct DnOpts {
    bool var;
    int32_t levels;
    float sigma, sigma_plane;
};

// The three thresholds rt_reproject_options and rt_temporal_options share, resolved.
struct GatherOpts {
    float normal_min, sigma_plane, min_weight;
};
GatherOpts gather_resolve(float normal_min, float sigma_plane, float min_weight, const std::string& who);

// rt_reproject_options resolved: a zero field = the default.
struct RpOpts : GatherOpts {
    float nh;
};
RpOpts rp_resolve(const rt_reproject_options* o, const std::string& who);
// The argument errors every reproject entry shares (host only).
void rp_check(const std::string& who, const float* prev_radiance, const float* radiance, int32_t samples,
              const float* radiance_out, const uint8_t* rgb_out);
// "reproject: the cameras hold different scenes" unless both builds are equal in every byte.
void rp_same_scene(const rt_camera* a, const rt_camera* b);

// `region` (NULL: the whole image) clamped to a width x height image; empty: an argument error.
rt_region dn_region(const rt_region* region, int32_t width, int32_t height, const std::string& who);

// Queued copies between a host array in full-frame layout (`elem` bytes per pixel, image width
// `width`) and a region-packed device array: the rows of region `r` only. down: a null host
// array is an output the caller did not ask for.
struct RegionIo {
    int32_t width;
    rt_region r;
    hipStream_t stream;
    int n() const { return r.width * r.height; }
    void up(void* dev, const void* host, size_t elem) const;
    void down(void* host, const void* dev, size_t elem) const;
};

// The four guide arrays of io's region through b's staging arrays (nrm / pos / dist / obj), then
// packed into b.gn / b.gp. Queued: the staging arrays may be reused by whatever is queued after.
void upload_guides(DnBufs& b, const RegionIo& io, const float* normal, const float* position, const float* distance,
                   const int32_t* object);

// A view's guide planes in a caller's arrays: the first-hit four and, through specular chains, the
// chain four and the chain words (chain_normal null: none).
struct HostGuides {
    const float *normal, *position, *distance;
    const int32_t* object;
    const float *chain_normal, *chain_position, *chain_distance;
    const int32_t *chain_object, *chain;
};
// Both views' planes of a stand-alone call: upload_guides of g through nb and of pg through pb and,
// where a view has chain planes, of those through ns / ps, whose obj planes then take the chain
// words (after their pack pass has read the chain objects). Allocates the four. Returns through
// *ng / *pgd the device planes, the chain three null for a view without them. Queued.
void upload_views(DnBufs& nb, DnBufs& ns, const RegionIo& io, const HostGuides& g, DnBufs& pb, DnBufs& ps,
                  const RegionIo& pio, const HostGuides& pg, RsGuides* ng, RsGuides* pgd);

// The caller's reusable table (n_objects >= 0 entries) into d, at least one byte. Queued.
void upload_reusable(DevBuf<uint8_t>& d, const uint8_t* reusable, int32_t n_objects, hipStream_t stream);
// A per-object table the host built (reusable or through objects) into d, at least one byte: an
// empty table is one zero. `what` names the allocation. Done on return.
void upload_table(DevBuf<uint8_t>& d, std::vector<uint8_t> t, const char* what);

// The open session's frames must be radiance.
void session_radiance(rt_camera* cam, const std::string& who);
// The open session, whose state holds radiance and at least min_samples samples per pixel (2: a
// variance); no device call.
DevCtx& session_host(rt_camera* cam, const std::string& who, int min_samples);
// The session must live on the current device.
void session_on_device(const DevCtx& c, const std::string& who);
// Both: argument errors first, then the device check.
DevCtx& session_with(rt_camera* cam, const std::string& who, int min_samples);
// The session's guides: computed once (queued), freed with the session.
void session_guides(rt_camera* cam, DevCtx& c, hipStream_t stream);
// rt_guide_options as the caller gave them (NULL: rt_guide_options_default), checked: an unknown
// mode, max_bounces outside 1..64 and a negative or non-finite max_fuzz are argument errors.
rt_guide_options guide_options(const rt_guide_options* o, const std::string& who);
// The session's guides through the specular chain for the options `go`: true when they are the
// kept ones, else recomputed (queued). Freed with the session.
// want_chain: the walk's chain plane is kept beside them (P.d_sch); kept guides without it are
// walked again.
bool session_specular_cached(const DevCtx& c, const rt_guide_options& go, bool want_chain = false);
void session_specular_guides(rt_camera* cam, DevCtx& c, const rt_guide_options& go, hipStream_t stream,
                             bool want_chain = false);
// The session's state -> c.dn.var (region-packed); queued.
void prog_variance_pass(DevCtx& c, hipStream_t stream);
// Queues the copy of the session region's rows of a full-frame device array (`elem` bytes per
// pixel) into the caller's host array of the same layout.
void prog_copy_out(const DevCtx& c, void* host, const void* dev, size_t elem, hipStream_t stream);

// The filter over a w x h region whose guides are gn / gp: colour and fn from `rad` (row pitch
// `pitch_px` pixels, region at (x0, y0)) and, variance-guided, from the region-packed b.var; one
// launch per level over the ping-pong pair, then the result into b.rad() / b.u8 and, when
// want_var, the filtered variance into b.var (region-packed). `o` is resolved. ev (or null):
// levels + 3 events, recorded before the pack pass, after it, after every level and after the
// unpack pass. hold (region-packed, or null): the pixels the unpack pass copies through from `rad`
// and b.var (DenoiseHold). Queued.
void dn_filter(DnBufs& b, const float4* gn, const float4* gp, const float* rad, int pitch_px, int x0, int y0, int w,
               int h, const DnOpts& o, bool want_rad, bool want_u8, bool want_var, hipStream_t stream, hipEvent_t* ev,
               const uint8_t* hold = nullptr);
// hold_k of a camera or session filter call: 0 (no hold), 2 or 4, else an argument error.
void hold_check(int32_t hold_k, const std::string& who);

inline RpView rp_camera_view(const rt_camera* cam) {
    const RtCamera& C = cam->build.cam;
    return rp_view_constants(C.center, C.pixel00, C.du, C.dv, C.width, C.height);
}

// The new view's side of a gather: its guides, and the fresh frame and sample counts to blend
// (null: history only) in one layout - row pitch `pitch` pixels, the region at (fx0, fy0) - with
// the scalar sample count m. The accumulation adds the region-packed fresh variance.
struct RpNew {
    const float4 *gn, *gp;
    const float* fresh;
    const int32_t* pxs;
    int pitch, fx0, fy0;
    float m;
};
struct TpNew : RpNew {
    const float* var;
};

// The head RpArgs and TpArgs have in common; the rest is zero.
template <class Args>
Args gather_args(const RpView& view, const rt_region& r, const rt_region& pr, int n_objects, const GatherOpts& o,
                 const RpNew& nw) {
    Args a{};
    a.view = view;
    a.w = r.width, a.h = r.height;
    a.px0 = pr.x, a.py0 = pr.y, a.pw = pr.width, a.ph = pr.height;
    a.n_objects = n_objects;
    a.normal_min = o.normal_min, a.sigma_plane = o.sigma_plane, a.min_weight = o.min_weight;
    a.pitch = nw.pitch, a.fx0 = nw.fx0, a.fy0 = nw.fy0;
    a.m = nw.m;
    return a;
}

// ---- what the reprojection's two ABI units share (api_reproject.cpp) -------------------------------
// What a call through specular chains adds to the plain one: both views' guide planes, the new
// view's centre, the through table, point_pixels resolved and the kind plane.
struct RpChain {
    RsGuides ng, pg;
    const float* cn;
    const uint8_t* d_through;
    float point_pixels;
    uint8_t* d_kind;
    bool want_kind;
};
// The device side of a call once both views' guides and the previous radiance (pb.rad(),
// region-packed) are there: the pack pass, the gather (ch: through chains), the unpack passes. ev
// (or null): events 2..4. Queued.
void rp_run(DnBufs& nb, DnBufs& pb, const RpView& view, const rt_region& r, const rt_region& pr, const uint8_t* d_reusable,
            int n_objects, const RpOpts& o, const RpNew& nw, bool want_hist, bool want_rad, bool want_u8, hipStream_t stream,
            hipEvent_t* ev, const RpChain* ch = nullptr);
// A call's outputs into the caller's arrays, then its one host sync.
void rp_outputs(const DnBufs& nb, const RegionIo& io, float* history, float* weight, float* radiance, uint8_t* rgb,
                uint8_t* kind = nullptr, const uint8_t* d_kind = nullptr);
// The previous view's side of a camera call: its context on the current device, the radiance
// uploaded into its rp_prev (event 0), new_guides(), its guide pass - with `go` also the one
// through the chain into its rs_prev - (event 1). Queued.
DevCtx& rp_prev_side(rt_camera* prev_cam, const rt_region& pr, const float* prev_radiance, hipStream_t stream,
                     hipEvent_t* ev, const std::function<void()>& new_guides, const rt_guide_options* go = nullptr);

// ---- what the accumulation's two ABI units share (api_temporal.cpp) --------------------------------
// rt_temporal_options resolved: a zero field = the default; levels 0 = no filter.
struct TpOpts : GatherOpts {
    float max_history;
    int32_t levels;
    float sigma_variance;
};
TpOpts tp_resolve(const rt_temporal_options* o, const std::string& who);
// The hash a history keeps of its scene: the arrays the reprojection's same-scene check compares.
uint64_t tp_scene_hash(const SceneBuild& b);
// What a call through specular chains adds to the plain one: the new view's guide planes, the
// history's (hg, read only when chain_history: it holds chain planes walked with the call's guide
// options), the new view's centre, the through table, point_pixels resolved and the kind plane.
struct TpChain {
    RsGuides ng, hg;
    bool chain_history;
    const float* cn;
    const uint8_t* d_through;
    float point_pixels;
    uint8_t* d_kind;
};
// The device side of a call: the gather and blend into out_col / out_var (weight -> b.dist(); ch:
// through chains, kind -> ch->d_kind), then the caller's outputs - the optional variance-guided
// filter of out / Vout on the new view's first-hit guides (ch: its chain guides), else out itself -
// into b.rad() / b.u8 / b.var, and the length into b.nrm(). pr.width == 0: an empty history. ev (or
// null): events 2 and 3, recorded after the gather and after the filter. Queued.
void tp_run(DnBufs& b, const TpNew& nw, const rt_region& r, const TpHistory& hist, const RpView& view, const rt_region& pr,
            const uint8_t* d_reusable, int n_objects, const TpOpts& o, float4* out_col, float* out_var, bool want_rad,
            bool want_u8, bool want_var, bool want_len, hipStream_t stream, hipEvent_t* ev, const TpChain* ch = nullptr);
// What the session call through chains adds: the guide options, the through mask and point_pixels
// resolved, and the caller's kind plane.
struct TpSessionChain {
    rt_guide_options go;
    int32_t through;
    float point_pixels;
    uint8_t* kind_out;
};
// rt_camera_progressive_accumulate[_specular] from session_with() on: the caller holds the history's
// and the camera's locks and has resolved the options.
void tp_session(rt_camera* cam, rt_history* h, const std::string& who, const TpOpts& o, int32_t commit, uint8_t* rgb,
                float* radiance, float* variance_out, float* length_out, float* weight_out,
                const TpSessionChain* sc = nullptr);
// The arguments rt_temporal_accumulate[_specular] share, as the caller gave them and the entry
// checked them; view (the new one), through and kind_out: through chains only, else null.
struct TpCall {
    int32_t width, height, samples, n_objects;
    const rt_region *region, *prev_region;
    const rt_view *view, *prev_view;
    HostGuides g, pg;
    const float *radiance, *variance, *prev_radiance, *prev_variance, *prev_length;
    const int32_t* px_samples;
    const uint8_t *reusable, *through;
    float *radiance_out, *variance_out, *length_out, *weight_out;
    uint8_t *rgb_out, *kind_out;
};
// A stand-alone call after its argument checks: the regions, the uploads, the run and the outputs.
// point_pixels < 0: the plain call.
void tp_explicit(const std::string& who, const TpCall& a, const TpOpts& o, float point_pixels = -1.0f);

// ---- what the two specular ABI units share (reproject_spec_api.cpp) --------------------------------
// The two fields rt_specular_reproject_options and rt_specular_temporal_options add to their base,
// resolved: a zero field = the default.
struct SpecOpts {
    float point_pixels;
    int32_t through;
};
SpecOpts spec_resolve(float point_pixels, int32_t through, const std::string& who);
// The guide options of a call: NULL = the specular walk's defaults; first-hit guides have no chains.
rt_guide_options rs_guide_options(const rt_guide_options* go, const std::string& who);
// through[o] for the mask and max_fuzz, as rt_camera_through_objects returns it.
std::vector<uint8_t> through_objects(const CamHost& h, int32_t mask, float max_fuzz);
// (pp * pp) * (du.du / a.a) of a view: each product, sum and the division rounded once.
float rs_pp2(const RpView& v, float pp);

}  // namespace rt
