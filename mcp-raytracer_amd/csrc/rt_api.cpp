// C ABI of the path-tracing core (include/rt_amd.h).
//
// rt_camera = the reference's Camera object after createCameraFromSceneData:
// the host build (scene.cpp) plus lazily allocated device copies. Rendering
// follows Camera.renderRegion's contract: the caller owns the output buffer,
// only the region is written, RenderStats are returned. This unit is the ABI layer only:
// argument checks, error mapping and the call sequences over dev_ctx.hpp's contexts.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/rt_amd.h"
#include "dev_ctx.hpp"
#include "json.hpp"
#include "prog_blob.hpp"

using namespace rt;

// png.hip: the frame's PNG, encoded on the device queue `stream` (waited for).
std::vector<uint8_t> rt_png_encode_device(const uint8_t* d_rgb, int32_t w, int32_t h, hipStream_t stream);

static_assert(ST_WORDS == RT_STATS_WORDS, "rt_camera_stats_words layout");
static_assert(kMaxPhases == RT_PLAN_MAX_PHASES, "rt_launch_plan schedule arrays");

#ifndef RT_BUILD_ID
#define RT_BUILD_ID "unhashed"
#endif

namespace {

thread_local std::string g_error;

int set_error(int code, const std::string& msg) {
    g_error = msg;
    return code;
}

}  // namespace

// error hook for the other translation units of the library (image.cpp)
int rt_set_error_message(int code, const char* msg) { return set_error(code, msg ? msg : ""); }

// The fields of rt_denoise_options / rt_denoise_var_options (NULL: all zero) as the caller gave
// them, then resolved by dn_resolve: a zero field = the default. var: the variance-guided
// filter, whose sigma is sigma_variance (the plain one's: sigma_color).
struct DnOpts {
    bool var;
    int32_t levels;
    float sigma, sigma_plane;
};
static DnOpts dn_options(const rt_denoise_options* o) {
    return o ? DnOpts{false, o->levels, o->sigma_color, o->sigma_plane} : DnOpts{false, 0, 0.0f, 0.0f};
}
static DnOpts dn_options(const rt_denoise_var_options* o) {
    return o ? DnOpts{true, o->levels, o->sigma_variance, o->sigma_plane} : DnOpts{true, 0, 0.0f, 0.0f};
}
static DnOpts dn_resolve(DnOpts o, const std::string& who) {
    if (o.levels < 0 || o.levels > kDenoiseMaxLevels)
        throw std::invalid_argument(who + ": levels must be 1.." + std::to_string(kDenoiseMaxLevels) + " (0: the default)");
    if (!(o.sigma >= 0.0f) || !std::isfinite(o.sigma))
        throw std::invalid_argument(who + (o.var ? ": sigma_variance" : ": sigma_color") +
                                    " must be positive and finite (0: the default)");
    if (!(o.sigma_plane >= 0.0f) || !std::isfinite(o.sigma_plane))
        throw std::invalid_argument(who + ": sigma_plane must be positive and finite (0: the default)");
    if (!o.levels) o.levels = 4;
    if (o.sigma == 0.0f) o.sigma = o.var ? 2.0f : 0.5f;
    if (o.sigma_plane == 0.0f) o.sigma_plane = 0.01f;
    return o;
}

// `region` (NULL: the whole image) clamped to a width x height image; empty: an argument error.
constexpr long kDenoiseMaxPixels = 1l << 28;
static rt_region dn_region(const rt_region* region, int32_t width, int32_t height, const std::string& who) {
    const rt_region r = clamp_region(region ? *region : rt_region{0, 0, width, height}, width, height);
    if (region_empty(r)) throw std::invalid_argument(who + ": the region is empty after clamping to the image");
    if ((long)r.width * r.height > kDenoiseMaxPixels) throw std::invalid_argument(who + ": the region has too many pixels");
    return r;
}

// Queued copies between a host array in full-frame layout (`elem` bytes per pixel, image
// width `width`) and a region-packed device array: the region's rows only.
static void dn_upload(void* dev, const void* host, size_t elem, int32_t width, const rt_region& r, hipStream_t stream) {
    const size_t off = ((size_t)r.y * width + r.x) * elem;
    hip_check(hipMemcpy2DAsync(dev, (size_t)r.width * elem, (const char*)host + off, (size_t)width * elem,
                               (size_t)r.width * elem, r.height, hipMemcpyHostToDevice, stream),
              "hipMemcpy2DAsync");
}
static void dn_download(void* host, const void* dev, size_t elem, int32_t width, const rt_region& r, hipStream_t stream) {
    if (!host) return;
    const size_t off = ((size_t)r.y * width + r.x) * elem;
    hip_check(hipMemcpy2DAsync((char*)host + off, (size_t)width * elem, dev, (size_t)r.width * elem,
                               (size_t)r.width * elem, r.height, hipMemcpyDeviceToHost, stream),
              "hipMemcpy2DAsync");
}

// The filter over a w x h region whose guides are gn / gp: colour and fn from `rad` (row pitch
// `pitch_px` pixels, region at (x0, y0)) and, variance-guided, from the region-packed b.var; one
// launch per level over the ping-pong pair, then the result into b.rad() / b.u8 and, when
// want_var, the filtered variance into b.var (region-packed). ev (or null): levels + 3 events,
// recorded before the pack pass, after it, after every level and after the unpack pass. Queued.
static void dn_filter(DnBufs& b, const float4* gn, const float4* gp, const float* rad, int pitch_px, int x0, int y0,
                      int w, int h, const DnOpts& o, bool want_rad, bool want_u8, bool want_var, hipStream_t stream,
                      hipEvent_t* ev) {
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
                                    o.var && want_var ? b.var.p : nullptr, stream),
              "denoise_unpack_kernel");
    mark();
}

// Queues the copy of a region's rows of the context's full frame into the caller's host
// buffers (full-frame layout: only the region is written, as Camera.renderRegion does).
static void copy_region_to_host(DevCtx& c, const rt_region& region, uint8_t* rgb, float* radiance, hipStream_t stream) {
    const RtCamera& C = c.build.cam;
    const rt_region r = clamp_region(region, C.width, C.height);
    if (region_empty(r)) return;
    const size_t pitch = (size_t)C.width * 3;
    const size_t off = ((size_t)r.y * C.width + r.x) * 3;
    const size_t w = (size_t)r.width * 3;
    if (rgb)
        hip_check(hipMemcpy2DAsync(rgb + off, pitch, c.d_rgb + off, pitch, w, r.height, hipMemcpyDeviceToHost, stream),
                  "hipMemcpy2DAsync");
    if (radiance)
        hip_check(hipMemcpy2DAsync(radiance + off, pitch * sizeof(float), c.d_rad + off, pitch * sizeof(float),
                                   w * sizeof(float), r.height, hipMemcpyDeviceToHost, stream),
                  "hipMemcpy2DAsync");
}

// The frame's PNG: encoded on the device from the context's u8 frame (png.hip), malloc'ed.
static void png_out(DevCtx& c, hipStream_t stream, uint8_t** out, size_t* out_len) {
    const RtCamera& C = c.build.cam;
    const std::vector<uint8_t> png = rt_png_encode_device(c.d_rgb, C.width, C.height, stream);
    uint8_t* b = (uint8_t*)std::malloc(png.size());
    if (!b) throw std::runtime_error("out of memory");
    std::memcpy(b, png.data(), png.size());
    *out = b;
    *out_len = png.size();
}

// The open session's header (payload fields left to the caller).
static ProgBlobHeader prog_header(const rt_camera* cam, const DevCtx& c) {
    const DevCtx::ProgSession& P = c.prog;
    const RtCamera& C = cam->build.cam;
    ProgBlobHeader h{};
    std::memcpy(h.magic, kProgMagic, sizeof kProgMagic);
    h.version = kProgBlobVersion;
    h.header_bytes = sizeof(ProgBlobHeader);
    std::strncpy(h.build_id, RT_BUILD_ID, sizeof h.build_id - 1);
    h.width = C.width;
    h.height = C.height;
    h.rx = P.region.x;
    h.ry = P.region.y;
    h.rw = P.region.width;
    h.rh = P.region.height;
    h.precision = P.precision;
    h.seed = C.seed;
    h.samples = C.samples;
    h.samples_loop = C.n_samples;
    h.samples_done = P.done;
    h.steps = P.steps;
    h.active_pixels = P.n_act;
    h.err_flags = P.err;
    h.fingerprint = prog_fingerprint(cam->build);
    h.payload_bytes = (uint64_t)P.slots * sizeof(ProgPix);
    return h;
}

// Queues the copy of the session region's rows of a full-frame device array (`elem` bytes per
// pixel) into the caller's host array of the same layout.
static void prog_copy_out(const DevCtx& c, void* host, const void* dev, size_t elem, hipStream_t stream) {
    if (!host) return;
    const rt_region& r = c.prog.region;
    const size_t pitch = (size_t)c.build.cam.width * elem;
    const size_t off = ((size_t)r.y * c.build.cam.width + r.x) * elem;
    hip_check(hipMemcpy2DAsync((char*)host + off, pitch, (const char*)dev + off, pitch, (size_t)r.width * elem, r.height,
                               hipMemcpyDeviceToHost, stream),
              "hipMemcpy2DAsync");
}

// Runs f under the camera's lock with the single-device entries' error mapping.
template <class F>
static int camera_call(rt_camera* cam, F&& f) {
    if (!cam) return set_error(RT_ERR_INVALID, "null camera");
    std::lock_guard<std::mutex> lock(cam->mu);
    try {
        f();
        return RT_OK;
    } catch (const HipError& e) {
        return set_error(RT_ERR_DEVICE, e.what());
    } catch (const std::invalid_argument& e) {
        return set_error(RT_ERR_INVALID, e.what());
    } catch (const std::exception& e) {
        return set_error(RT_ERR_RENDER, e.what());
    }
}

// Runs f under both cameras' locks (one lock when they are the same camera), with the
// single-device entries' error mapping.
template <class F>
static int two_camera_call(rt_camera* cam, rt_camera* prev_cam, F&& f) {
    if (!cam || !prev_cam) return set_error(RT_ERR_INVALID, "null camera");
    std::unique_lock<std::mutex> la(cam->mu, std::defer_lock), lb(prev_cam->mu, std::defer_lock);
    if (cam == prev_cam)
        la.lock();
    else
        std::lock(la, lb);
    try {
        f();
        return RT_OK;
    } catch (const HipError& e) {
        return set_error(RT_ERR_DEVICE, e.what());
    } catch (const std::invalid_argument& e) {
        return set_error(RT_ERR_INVALID, e.what());
    } catch (const std::exception& e) {
        return set_error(RT_ERR_RENDER, e.what());
    }
}

// Runs f under the history's lock with the single-device entries' error mapping.
template <class F>
static int history_call(rt_history* h, F&& f) {
    if (!h) return set_error(RT_ERR_INVALID, "null history");
    std::lock_guard<std::mutex> lock(h->mu);
    try {
        f();
        return RT_OK;
    } catch (const HipError& e) {
        return set_error(RT_ERR_DEVICE, e.what());
    } catch (const std::invalid_argument& e) {
        return set_error(RT_ERR_INVALID, e.what());
    } catch (const std::exception& e) {
        return set_error(RT_ERR_RENDER, e.what());
    }
}

template <class T>
static bool same_bytes(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}
extern "C" {

int rt_version(void) { return RT_AMD_VERSION; }

const char* rt_last_error(void) { return g_error.c_str(); }

void rt_free(void* p) { std::free(p); }

int rt_generate_scene_data(const char* type, const char* options_json, char** out_json) {
    try {
        if (!type || !out_json) return set_error(RT_ERR_INVALID, "type and out_json are required");
        rtj::Value opts;
        const rtj::Value* optp = nullptr;
        if (options_json && options_json[0]) {
            opts = rtj::parse(options_json, std::strlen(options_json));
            if (!opts.is_null()) optp = &opts;
        }
        const std::string s = rtj::dump(generate_scene_data(type, optp));
        char* buf = (char*)std::malloc(s.size() + 1);
        if (!buf) return set_error(RT_ERR_INVALID, "out of memory");
        std::memcpy(buf, s.c_str(), s.size() + 1);
        *out_json = buf;
        return RT_OK;
    } catch (const std::exception& e) {
        return set_error(RT_ERR_INVALID, e.what());
    }
}

int rt_camera_create(const char* scene_json, const char* render_options_json, rt_camera** out) {
    try {
        if (!scene_json || !out) return set_error(RT_ERR_INVALID, "scene_json and out are required");
        const rtj::Value scene = rtj::parse(scene_json, std::strlen(scene_json));
        rtj::Value ro;
        const rtj::Value* rop = nullptr;
        if (render_options_json && render_options_json[0]) {
            ro = rtj::parse(render_options_json, std::strlen(render_options_json));
            if (!ro.is_null()) rop = &ro;
        }
        auto* cam = new rt_camera();
        try {
            cam->build = build_scene(scene, rop);
            int32_t prec = PREC_REF;
            auto pick = [&](const rtj::Value* v) {
                if (v && v->is_string()) {
                    if (v->str == "fp32") prec = PREC_FP32;
                    else if (v->str == "ref") prec = PREC_REF;
                    else throw std::runtime_error("precision must be 'ref' or 'fp32'");
                }
            };
            if (const rtj::Value* r = scene.get("render")) pick(r->get("precision"));
            if (rop) pick(rop->get("precision"));
            cam->precision = prec;
            int32_t trav = TRAV_AUTO;
            auto pick_t = [&](const rtj::Value* v) {
                if (v && v->is_string()) {
                    if (v->str == "reference") trav = TRAV_REFERENCE;
                    else if (v->str == "fast") trav = TRAV_FAST;
                    else if (v->str == "brute") trav = TRAV_BRUTE;
                    else if (v->str == "auto") trav = TRAV_AUTO;
                    else throw std::runtime_error("traversal must be 'auto', 'fast', 'brute' or 'reference'");
                }
            };
            if (const rtj::Value* r = scene.get("render")) pick_t(r->get("traversal"));
            if (rop) pick_t(rop->get("traversal"));
            cam->traversal = trav;
            if (env_flag("RT_AMD_LAUNCH_LOG", false)) {
                const SceneBuild& b = cam->build;
                std::fprintf(stderr,
                             "[rt scene] prims %zu t4nodes %zu (%zu B) tnodes %zu tprims %zu B tsph %zu B prims %zu B "
                             "mats %zu B lights %zu B nodes %zu stack_depth %d\n",
                             b.prims.size(), b.t4nodes.size(), b.t4nodes.size() * sizeof(b.t4nodes[0]), b.tnodes.size(),
                             b.tprims.size() * 4, b.tsph.size() * 16, b.prims.size() * sizeof(RtPrim),
                             b.mats.size() * sizeof(RtMat), b.lights.size() * sizeof(RtLight), b.nodes.size(),
                             b.cam.stack_depth);
            }
            // MixturePDF([cosine, ...lights], [0.5, ...0.5/nL]).totalWeight (pdf.ts:48-52)
            const int nl = cam->build.cam.n_lights;
            cam->light_w = nl > 0 ? 0.5 / (double)nl : 0.0;
            double total = 0.0;
            total += 0.5;
            for (int k = 0; k < nl; ++k) total += cam->light_w;
            cam->mix_total = total;
        } catch (...) {
            delete cam;
            throw;
        }
        *out = cam;
        return RT_OK;
    } catch (const std::exception& e) {
        return set_error(RT_ERR_INVALID, e.what());
    }
}

void rt_camera_destroy(rt_camera* cam) { delete cam; }

int rt_camera_get_info(const rt_camera* cam, rt_camera_info* info) {
    if (!cam || !info) return set_error(RT_ERR_INVALID, "null argument");
    const RtCamera& C = cam->build.cam;
    info->width = C.width;
    info->height = C.height;
    info->channels = 3;
    info->n_objects = C.n_prims;
    info->n_nodes = C.n_nodes;
    info->n_lights = C.n_lights;
    info->n_materials = C.n_mats;
    info->bvh_depth = cam->build.bvh_depth;
    info->samples_loop = C.n_samples;
    info->depth = C.depth;
    info->roulette = C.roulette;
    info->roulette_depth = C.roulette_depth;
    info->mode = C.mode;
    info->adaptive = C.adaptive;
    info->precision = cam->precision;
    // effective traversal: fast/brute only where provably exact (scene.cpp prims_inside_boxes)
    info->traversal = cam->effective_traversal(cam->traversal);
    info->seed = C.seed;
    info->samples = C.samples;
    info->aperture = C.aperture;
    info->a_tolerance = C.a_tolerance;
    info->a_batch = C.a_batch;
    return RT_OK;
}

int rt_camera_set_precision(rt_camera* cam, int32_t precision) {
    if (!cam) return set_error(RT_ERR_INVALID, "null camera");
    if (precision != PREC_REF && precision != PREC_FP32) return set_error(RT_ERR_INVALID, "bad precision");
    cam->precision = precision;
    return RT_OK;
}

int rt_camera_render_region(rt_camera* cam, const rt_region* region, uint8_t* rgb, float* radiance,
                            rt_render_stats* stats) {
    if (!cam || !region) return set_error(RT_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lock(cam->mu);
    try {
        DevCtx& c = cam->current();
        c.ensure_device();
        c.ensure_frame();
        const hipStream_t stream = nullptr;
        cam->last = &c;
        cam->multi.clear();
        c.launch(*region, 0, 1, cam->precision, cam->traversal, 0, rgb ? c.d_rgb : nullptr,
                 radiance ? c.d_rad : nullptr, nullptr, nullptr, 0, stream);
        c.read_stats(stats, nullptr, stream);
        copy_region_to_host(c, *region, rgb, radiance, stream);
        hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");
        return RT_OK;
    } catch (const HipError& e) {
        return set_error(RT_ERR_DEVICE, e.what());
    } catch (const std::invalid_argument& e) {
        return set_error(RT_ERR_INVALID, e.what());
    } catch (const std::exception& e) {
        return set_error(RT_ERR_RENDER, e.what());
    }
}

int rt_camera_render(rt_camera* cam, uint8_t* rgb, float* radiance, rt_render_stats* stats) {
    if (!cam) return set_error(RT_ERR_INVALID, "null camera");
    rt_region r{0, 0, cam->build.cam.width, cam->build.cam.height};
    return rt_camera_render_region(cam, &r, rgb, radiance, stats);
}

int rt_camera_render_png(rt_camera* cam, int32_t bands, rt_render_stats* stats, uint8_t** out, size_t* out_len) {
    if (!cam || !out || !out_len) return set_error(RT_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lock(cam->mu);
    try {
        DevCtx& c = cam->current();
        c.ensure_device();
        c.ensure_frame();
        const RtCamera& C = cam->build.cam;
        const hipStream_t stream = nullptr;
        // The reference renders divideIntoRegions' ceil(H / count)-row bands on `count` workers
        // (src/raytracer.ts:60-90, 185-205) and merges their RenderStats (renderStats.ts:42-64).
        // Neither the image nor the merged stats depend on the split (the path RNG is keyed by
        // pixel and sample; merge sums totals and takes minima / maxima), so the device renders
        // the whole frame in one launch whatever `bands` says - one launch and one stats read
        // instead of `bands` small ones, each waiting for the GPU.
        (void)bands;
        const rt_region r{0, 0, C.width, C.height};
        cam->last = &c;
        cam->multi.clear();
        c.launch(r, 0, 1, cam->precision, cam->traversal, 0, c.d_rgb, nullptr, nullptr, nullptr, 0, stream);
        rt_render_stats m;
        c.read_stats(&m, nullptr, stream);
        if (stats) *stats = m;
        png_out(c, stream, out, out_len);
        return RT_OK;
    } catch (const HipError& e) {
        return set_error(RT_ERR_DEVICE, e.what());
    } catch (const std::invalid_argument& e) {
        return set_error(RT_ERR_INVALID, e.what());
    } catch (const std::exception& e) {
        return set_error(RT_ERR_RENDER, e.what());
    }
}

int rt_camera_render_device(rt_camera* cam, const rt_launch* L, rt_render_stats* stats, uint64_t* work_counters) {
    if (!cam || !L) return set_error(RT_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lock(cam->mu);
    try {
        DevCtx& c = cam->current();
        c.ensure_device();
        const hipStream_t stream = (hipStream_t)L->stream;
        const int prec = L->precision < 0 ? cam->precision : L->precision;
        const int trav = L->traversal < 0 ? cam->traversal : L->traversal;
        if (L->count_work < 0 || L->count_work > 2) throw std::invalid_argument("count_work must be 0, 1 or 2");
        cam->last = &c;
        cam->multi.clear();
        c.launch(L->region, L->tile_group, L->tile_groups, prec, trav, L->count_work, L->rgb, L->radiance,
                 L->px_samples, L->px_bounces, L->packed_tiles, stream);
        if (L->synchronize) c.read_stats(stats, L->count_work ? work_counters : nullptr, stream);
        return RT_OK;
    } catch (const HipError& e) {
        return set_error(RT_ERR_DEVICE, e.what());
    } catch (const std::invalid_argument& e) {
        return set_error(RT_ERR_INVALID, e.what());
    } catch (const std::exception& e) {
        return set_error(RT_ERR_RENDER, e.what());
    }
}

int rt_camera_export(const rt_camera* cam, void* nodes, void* prims, void* materials, void* lights,
                     int32_t* prim_object) {
    if (!cam) return set_error(RT_ERR_INVALID, "null camera");
    const SceneBuild& b = cam->build;
    if (nodes) std::memcpy(nodes, b.nodes.data(), b.nodes.size() * sizeof(RtNode));
    if (prims) std::memcpy(prims, b.prims.data(), b.prims.size() * sizeof(RtPrim));
    if (materials) std::memcpy(materials, b.mats.data(), b.mats.size() * sizeof(RtMat));
    if (lights) std::memcpy(lights, b.lights.data(), b.lights.size() * sizeof(RtLight));
    if (prim_object) std::memcpy(prim_object, b.prim_object.data(), b.prim_object.size() * sizeof(int32_t));
    return RT_OK;
}

int rt_debug_world_hit(rt_camera* cam, int32_t traversal, int32_t n, const float* orig, const float* dir,
                       double* out) {
    if (!cam || n < 0 || (n > 0 && (!orig || !dir || !out))) return set_error(RT_ERR_INVALID, "bad arguments");
    std::lock_guard<std::mutex> lock(cam->mu);
    float* d_o = nullptr;
    float* d_d = nullptr;
    double* d_out = nullptr;
    try {
        DevCtx& c = cam->current();
        c.ensure_device();
        if (n == 0) return RT_OK;
        hip_check(hipMalloc(&d_o, (size_t)n * 3 * sizeof(float)), "hipMalloc");
        hip_check(hipMalloc(&d_d, (size_t)n * 3 * sizeof(float)), "hipMalloc");
        hip_check(hipMalloc(&d_out, (size_t)n * 10 * sizeof(double)), "hipMalloc");
        hip_check(hipMemcpy(d_o, orig, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy");
        hip_check(hipMemcpy(d_d, dir, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy");
        const int trav = c.effective_traversal(traversal < 0 ? cam->traversal : traversal);
        hip_check(launch_world_hit_ref(c.dev_scene(), trav, n, d_o, d_d, d_out, nullptr),
                  "world_hit_kernel");
        hip_check(hipMemcpy(out, d_out, (size_t)n * 10 * sizeof(double), hipMemcpyDeviceToHost), "hipMemcpy");
        (void)hipFree(d_o);
        (void)hipFree(d_d);
        (void)hipFree(d_out);
        return RT_OK;
    } catch (const std::exception& e) {
        if (d_o) (void)hipFree(d_o);
        if (d_d) (void)hipFree(d_d);
        if (d_out) (void)hipFree(d_out);
        return set_error(RT_ERR_DEVICE, e.what());
    }
}

int rt_debug_math(int32_t n, const uint32_t* u, double* out) {
    if (n < 0 || (n > 0 && (!u || !out))) return set_error(RT_ERR_INVALID, "bad arguments");
    uint32_t* d_u = nullptr;
    double* d_out = nullptr;
    try {
        if (n == 0) return RT_OK;
        hip_check(hipMalloc(&d_u, (size_t)n * sizeof(uint32_t)), "hipMalloc");
        hip_check(hipMalloc(&d_out, (size_t)n * 3 * sizeof(double)), "hipMalloc");
        hip_check(hipMemcpy(d_u, u, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice), "hipMemcpy");
        hip_check(launch_math_probe(n, d_u, d_out, nullptr), "math_probe_kernel");
        hip_check(hipMemcpy(out, d_out, (size_t)n * 3 * sizeof(double), hipMemcpyDeviceToHost), "hipMemcpy");
        (void)hipFree(d_u);
        (void)hipFree(d_out);
        return RT_OK;
    } catch (const std::exception& e) {
        if (d_u) (void)hipFree(d_u);
        if (d_out) (void)hipFree(d_out);
        return set_error(RT_ERR_DEVICE, e.what());
    }
}

int rt_debug_fp64(int32_t n, const double* x, double* out) {
    if (n < 0 || (n > 0 && (!x || !out))) return set_error(RT_ERR_INVALID, "bad arguments");
    double* d_x = nullptr;
    double* d_out = nullptr;
    try {
        if (n == 0) return RT_OK;
        hip_check(hipMalloc(&d_x, (size_t)n * sizeof(double)), "hipMalloc");
        hip_check(hipMalloc(&d_out, (size_t)n * 4 * sizeof(double)), "hipMalloc");
        hip_check(hipMemcpy(d_x, x, (size_t)n * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy");
        hip_check(launch_fp64_probe(n, d_x, d_out, nullptr), "fp64_probe_kernel");
        hip_check(hipMemcpy(out, d_out, (size_t)n * 4 * sizeof(double), hipMemcpyDeviceToHost), "hipMemcpy");
        (void)hipFree(d_x);
        (void)hipFree(d_out);
        return RT_OK;
    } catch (const std::exception& e) {
        if (d_x) (void)hipFree(d_x);
        if (d_out) (void)hipFree(d_out);
        return set_error(RT_ERR_DEVICE, e.what());
    }
}

int rt_debug_pass_plan(int64_t units, int64_t unit_slots, int64_t chunks_per_slot, int64_t rec_bytes_per_unit,
                       int64_t budget_bytes, int64_t* pass_units_out) {
    if (units < 0 || unit_slots < 1 || chunks_per_slot < 1 || rec_bytes_per_unit < 1 || budget_bytes < 1 ||
        !pass_units_out)
        return set_error(RT_ERR_INVALID, "bad arguments");
    *pass_units_out = pass_units((long)units, (long)unit_slots, (long)chunks_per_slot, (size_t)rec_bytes_per_unit,
                                 (size_t)budget_bytes);
    return RT_OK;
}

int rt_debug_scene_blob(const rt_camera* cam, uint8_t* out, int64_t capacity, rt_scene_blob_info* info) {
    if (!cam || !info) return set_error(RT_ERR_INVALID, "bad arguments");
    try {
        const SceneBlob b = build_scene_blob(cam->build);
        *info = rt_scene_blob_info{(int64_t)b.size, b.off_tprims, b.off_tsph, b.off_prims, b.off_xrec, b.off_mats,
                                   b.off_lights, b.off_onbs, b.off_nodes, b.off_pre, b.off_tsph2, b.lds_words,
                                   b.lds_words2, b.n_pre, b.n_onb};
        if (out) {
            if (capacity < info->bytes) return set_error(RT_ERR_INVALID, "rt_debug_scene_blob: capacity below the blob's size");
            std::memcpy(out, b.bytes.data(), b.size);
        }
        return RT_OK;
    } catch (const std::exception& e) {
        return set_error(RT_ERR_RENDER, e.what());
    }
}

int rt_debug_launch_plan(const rt_camera* cam, const rt_region* region, int32_t tile_group, int32_t tile_groups,
                         int32_t cus, int32_t lds_max, int32_t precision, int32_t count, rt_launch_plan* out) {
    if (!cam || !region || !out || cus < 1 || lds_max < 1 || precision > PREC_FP32 || count < 0 || count > 2)
        return set_error(RT_ERR_INVALID, "bad arguments");
    try {
        const RtCamera& C = cam->build.cam;
        const bool table = out->table_exists != 0;
        *out = rt_launch_plan{};
        out->table_exists = table;
        SceneBlob blob = build_scene_blob(cam->build);
        const LaunchPlan plan = plan_launch(*cam, blob, cus, lds_max, clamp_region(*region, C.width, C.height), tile_group,
                                            tile_groups, precision < 0 ? cam->precision : precision, cam->traversal, count,
                                            0, table, false);
        const long mine = plan.g.my_tiles;
        out->region = rt_region{plan.reg.x, plan.reg.y, plan.reg.width, plan.reg.height};
        out->traversal = plan.v.trav;
        out->tiles = (int32_t)mine;
        out->lds_level = plan.g.lds_level;
        out->n_top = plan.n_top;
        out->lds_bytes = (int64_t)plan.g.lds_bytes;
        out->stack_bytes = (int64_t)plan.stack;
        out->defer = plan.v.defer;
        out->kernel = RT_KERNEL_NONE;
        if (mine == 0) return RT_OK;
        if (plan.sequential) {
            out->kernel = RT_KERNEL_SEQUENTIAL;
            out->grid = plan.g.grid;
            out->passes = 1;
            return RT_OK;
        }
        // the first pass loop of DevCtx::launch_adaptive_rounds / launch_fixed
        SampleBuf sb{};
        const int nsamp = plan.rounds ? std::min(adaptive_first_len(C), C.n_samples) : C.n_samples;
        const bool pool = guided_schedule(plan, (double)mine * kWave, nsamp, plan.rounds, cus, sb);
        const long units = plan.rounds ? record_pass_slots(mine * kWave, sb, nsamp) / kWave
                                       : pass_units(mine, kWave, chunks_per_slot(sb),
                                                    fixed_rec_bytes_per_tile(C, plan.rec12), sbuf_budget());
        sb.slots = (int32_t)(std::min(units, mine) * kWave);
        out->grid = number_pass_items(sb, pool, cus);
        out->kernel = pool ? RT_KERNEL_POOL : RT_KERNEL_CHUNKED;
        out->pool = pool;
        out->primary_ok = plan.primary_ok;
        out->rec12 = plan.rec12;
        out->sb_pool = sb.pool;
        out->n_phases = sb.n_phases;
        for (int p = 0; p < sb.n_phases; ++p) {
            out->s0[p] = sb.s0[p];
            out->chunk[p] = sb.chunk[p];
            out->nch[p] = sb.nch[p];
        }
        out->refill_min = sb.refill_min;
        out->min_ready = sb.min_ready;
        out->samples = nsamp;
        out->pass_units = units;
        out->passes = (int32_t)((mine + units - 1) / units);
        return RT_OK;
    } catch (const std::invalid_argument& e) {
        return set_error(RT_ERR_INVALID, e.what());
    } catch (const std::exception& e) {
        return set_error(RT_ERR_RENDER, e.what());
    }
}

int rt_debug_rng(uint32_t seed, uint32_t pixel, uint32_t sample, int32_t n, uint32_t* out) {
    if (n < 0 || (n > 0 && !out)) return set_error(RT_ERR_INVALID, "bad arguments");
    uint64_t s = splitmix64((((uint64_t)pixel << 32) | sample) ^ splitmix64(seed));
    for (int32_t k = 0; k < n; ++k) {
        const uint64_t old = s;
        s = old * 6364136223846793005ull + 1442695040888963407ull;
        const uint32_t xs = (uint32_t)(((old >> 18u) ^ old) >> 27u);
        const uint32_t rot = (uint32_t)(old >> 59u);
        out[k] = (xs >> rot) | (xs << ((32u - rot) & 31u));
    }
    return RT_OK;
}

int rt_camera_kernel_times(rt_camera* cam, float* path_ms, float* accum_ms) {
    if (!cam || !path_ms || !accum_ms) return set_error(RT_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lock(cam->mu);
    try {
        *path_ms = 0.0f;
        *accum_ms = 0.0f;
        if (cam->last) cam->last->times(path_ms, accum_ms);
        return RT_OK;
    } catch (const std::exception& e) {
        return set_error(RT_ERR_DEVICE, e.what());
    }
}

int rt_camera_stats_words(rt_camera* cam, uint64_t* dst, void* stream) {
    if (!cam || !dst) return set_error(RT_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lock(cam->mu);
    try {
        DevCtx* c = cam->last;
        if (!c || !c->live || !c->d_stats) throw std::invalid_argument("rt_camera_stats_words: no render yet");
        // the ST_WORDS words sit kStatStride apart (one 128-B line each); dst gets them packed
        hip_check(hipMemcpy2DAsync(dst, sizeof(uint64_t), c->d_stats, kStatStride * sizeof(unsigned long long),
                                   sizeof(uint64_t), ST_WORDS, hipMemcpyDeviceToDevice, (hipStream_t)stream),
                  "hipMemcpy2DAsync(stats)");
        return RT_OK;
    } catch (const std::invalid_argument& e) {
        return set_error(RT_ERR_INVALID, e.what());
    } catch (const std::exception& e) {
        return set_error(RT_ERR_DEVICE, e.what());
    }
}

int rt_camera_adaptive_info(rt_camera* cam, int32_t* rounds, uint64_t* samples_rendered) {
    if (!cam || !rounds || !samples_rendered) return set_error(RT_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lock(cam->mu);
    *rounds = cam->last ? cam->last->adapt_rounds : 0;
    *samples_rendered = cam->last ? cam->last->adapt_rendered : 0;
    return RT_OK;
}

int rt_camera_pass_count(rt_camera* cam, int32_t* passes) {
    if (!cam || !passes) return set_error(RT_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lock(cam->mu);
    *passes = cam->last ? cam->last->n_passes : 0;
    return RT_OK;
}

int rt_camera_last_kernel(rt_camera* cam, int32_t* kernel) {
    if (!cam || !kernel) return set_error(RT_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lock(cam->mu);
    *kernel = cam->last ? cam->last->last_kernel : RT_KERNEL_NONE;
    return RT_OK;
}

int rt_camera_primary_table(const rt_camera* cam, uint64_t* out, int32_t capacity) {
    if (!cam || !out) return set_error(RT_ERR_INVALID, "null argument");
    const RtCamera& C = cam->build.cam;
    if (!cam->primary_table_ok(cam->traversal))
        return set_error(RT_PRIMARY_TABLE_NONE,
                         "no primary-ray table: it needs a pinhole camera (aperture 0) and brute-force traversal "
                         "of at most 16 primitives");
    if ((int64_t)capacity < (int64_t)C.width * C.height)
        return set_error(RT_ERR_INVALID, "rt_camera_primary_table: capacity below width * height records");
    primary_table_host(C, cam->build.prims.data(), C.n_prims, out);
    return RT_OK;
}

int rt_camera_primary_info(rt_camera* cam, rt_primary_info* info) {
    if (!cam || !info) return set_error(RT_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lock(cam->mu);
    try {
        DevCtx* c = cam->last;
        info->available = cam->primary_table_ok(cam->traversal) ? 1 : 0;
        info->used = c && c->ptab_used ? 1 : 0;
        info->built = c && c->d_ptab ? 1 : 0;
        info->min_samples = kPrimaryMinSamples;
        info->build_ms = 0.0f;
        if (c && c->d_ptab) {
            DeviceScope scope;
            hip_check(hipSetDevice(c->device), "hipSetDevice");
            info->build_ms = c->primary_table_ms();
        }
        return RT_OK;
    } catch (const std::exception& e) {
        return set_error(RT_ERR_DEVICE, e.what());
    }
}

int rt_camera_primary_table_device(rt_camera* cam, uint64_t* out, int32_t capacity) {
    if (!cam || !out) return set_error(RT_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lock(cam->mu);
    try {
        const RtCamera& C = cam->build.cam;
        if (!cam->primary_table_ok(cam->traversal))
            return set_error(RT_PRIMARY_TABLE_NONE, "no primary-ray table for this camera");
        if ((int64_t)capacity < (int64_t)C.width * C.height)
            throw std::invalid_argument("rt_camera_primary_table_device: capacity below width * height records");
        DevCtx& c = cam->current();
        c.ensure_device();
        c.ensure_primary_table(nullptr);
        hip_check(hipStreamSynchronize(c.ptab_stream), "hipStreamSynchronize");
        hip_check(hipMemcpy(out, c.d_ptab, (size_t)C.width * C.height * sizeof(uint64_t), hipMemcpyDeviceToHost),
                  "hipMemcpy(primary table)");
        return RT_OK;
    } catch (const HipError& e) {
        return set_error(RT_ERR_DEVICE, e.what());
    } catch (const std::invalid_argument& e) {
        return set_error(RT_ERR_INVALID, e.what());
    } catch (const std::exception& e) {
        return set_error(RT_ERR_RENDER, e.what());
    }
}

int rt_multi_plan_region(const rt_region* region, int32_t width, int32_t height, int32_t n_devices,
                         rt_multi_plan* plan) {
    if (!region || !plan || width < 0 || height < 0 || n_devices < 1 || n_devices > RT_MAX_DEVICES)
        return set_error(RT_ERR_INVALID, "rt_multi_plan_region: bad arguments");
    *plan = make_multi_plan(*region, width, height, n_devices);
    return RT_OK;
}

// Errors of the multi-GPU entries: the reference's render errors, HIP / RCCL errors, bad arguments.
static int multi_call(rt_camera* cam, const std::function<void()>& f) {
    if (!cam) return set_error(RT_ERR_INVALID, "null camera");
    std::lock_guard<std::mutex> lock(cam->mu);
    try {
        f();
        return RT_OK;
    } catch (const HipError& e) {
        return set_error(RT_ERR_DEVICE, e.what());
    } catch (const std::invalid_argument& e) {
        return set_error(RT_ERR_INVALID, e.what());
    } catch (const std::exception& e) {
        return set_error(RT_ERR_RENDER, e.what());
    }
}

int rt_camera_render_multi(rt_camera* cam, const int32_t* devices, int32_t n_devices, const rt_region* region,
                           uint8_t* rgb, float* radiance, rt_render_stats* stats) {
    if (!region) return set_error(RT_ERR_INVALID, "null region");
    return multi_call(cam, [&] {
        unsigned long long m[ST_WORDS];
        render_multi(cam, devices, n_devices, *region, rgb != nullptr, radiance != nullptr, m,
                     [&](DevCtx& root) { copy_region_to_host(root, *region, rgb, radiance, root.stream); });
        DevCtx::stats_from_words(m, stats);
    });
}

int rt_camera_render_png_multi(rt_camera* cam, const int32_t* devices, int32_t n_devices, rt_render_stats* stats,
                               uint8_t** out, size_t* out_len) {
    if (!out || !out_len) return set_error(RT_ERR_INVALID, "null argument");
    return multi_call(cam, [&] {
        const rt_region r{0, 0, cam->build.cam.width, cam->build.cam.height};
        unsigned long long m[ST_WORDS];
        DevCtx& root = render_multi(cam, devices, n_devices, r, true, false, m, nullptr);
        DevCtx::stats_from_words(m, stats);
        png_out(root, root.stream, out, out_len);
    });
}

int rt_camera_multi_info(rt_camera* cam, rt_multi_info* info) {
    if (!info) return set_error(RT_ERR_INVALID, "null argument");
    return multi_call(cam, [&] {
        *info = rt_multi_info{};
        if (cam->multi.empty()) return;
        info->n_devices = (int32_t)cam->multi.size();
        info->transport = cam->multi_transport;
        info->plan = cam->multi_plan;
        for (size_t g = 0; g < cam->multi.size(); ++g) {
            DevCtx& c = *cam->multi[g];
            info->devices[g] = c.device;
            c.times(&info->path_ms[g], &info->accum_ms[g]);
        }
        DevCtx& root = *cam->multi[0];
        hip_check(hipEventSynchronize(root.ev_gather1), "hipEventSynchronize");
        hip_check(hipEventElapsedTime(&info->gather_ms, root.ev_gather0, root.ev_gather1), "hipEventElapsedTime");
    });
}

int rt_camera_progressive_begin(rt_camera* cam, const rt_region* region) {
    return camera_call(cam, [&] {
        const RtCamera& C = cam->build.cam;
        const rt_region r = region ? *region : rt_region{0, 0, C.width, C.height};
        // (checked before the device is touched; prog_alloc clamps the same way)
        if (region_empty(clamp_region(r, C.width, C.height)))
            throw std::invalid_argument("rt_camera_progressive_begin: the region is empty after clamping to the image");
        DevCtx& c = cam->current();
        c.ensure_device();
        if (cam->prog && cam->prog != &c) cam->end_session();
        c.prog_alloc(r, cam->precision);  // (throws before dropping an open session on a bad region)
        cam->prog = &c;
        try {
            c.prog_start(nullptr);
        } catch (...) {
            cam->end_session();
            throw;
        }
    });
}

int rt_camera_progressive_step(rt_camera* cam, int32_t n_samples, uint8_t* rgb, float* radiance, int32_t* px_samples,
                               int32_t* px_bounces, rt_render_stats* stats) {
    return camera_call(cam, [&] {
        DevCtx& c = cam->session("rt_camera_progressive_step");
        if (n_samples <= 0) throw std::invalid_argument("rt_camera_progressive_step: n_samples must be positive");
        int dev = 0;
        hip_check(hipGetDevice(&dev), "hipGetDevice");
        if (dev != c.device) throw std::invalid_argument("rt_camera_progressive_step: the session lives on another device");
        DevCtx::ProgSession& P = c.prog;
        const RtCamera& C = cam->build.cam;
        const hipStream_t stream = nullptr;
        const int len = std::min<long>(n_samples, (long)C.n_samples - P.done);
        if (len > 0 && P.n_act > 0) {  // (a finished session renders nothing)
            cam->last = &c;
            cam->multi.clear();
            const ProgStep step{P.d_act, P.n_act, P.done, len};
            c.launch(P.region, 0, 1, P.precision, cam->traversal, 0, P.d_rgb, P.d_rad, P.d_pxs, P.d_pxb, 0, stream, &step);
            c.prog_read(stream);
            P.done += len;
            ++P.steps;
        }
        DevCtx::stats_from_words(P.words, stats);  // throws the render errors of the samples kept
        prog_copy_out(c, rgb, P.d_rgb, 3, stream);
        prog_copy_out(c, radiance, P.d_rad, 3 * sizeof(float), stream);
        prog_copy_out(c, px_samples, P.d_pxs, sizeof(int32_t), stream);
        prog_copy_out(c, px_bounces, P.d_pxb, sizeof(int32_t), stream);
        hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");
    });
}

int rt_camera_progressive_info(rt_camera* cam, rt_progressive_info* info) {
    if (!info) return set_error(RT_ERR_INVALID, "null argument");
    return camera_call(cam, [&] {
        DevCtx& c = cam->session("rt_camera_progressive_info");
        prog_info_from_header(prog_header(cam, c), info);
    });
}

int rt_camera_progressive_save(rt_camera* cam, uint8_t** blob, size_t* len) {
    if (!blob || !len) return set_error(RT_ERR_INVALID, "null argument");
    return camera_call(cam, [&] {
        DevCtx& c = cam->session("rt_camera_progressive_save");
        // (format version 1 has no field for the focused steps' sample cursor)
        if (c.prog.focused) throw std::invalid_argument("progressive: a focused session cannot be saved");
        ProgBlobHeader h = prog_header(cam, c);
        const size_t total = sizeof h + (size_t)h.payload_bytes;
        uint8_t* b = (uint8_t*)std::malloc(total);
        if (!b) throw std::runtime_error("out of memory");
        DeviceScope scope;
        hipError_t e = hipSetDevice(c.device);
        if (e == hipSuccess) e = hipMemcpy(b + sizeof h, c.prog.d_state, (size_t)h.payload_bytes, hipMemcpyDeviceToHost);
        if (e != hipSuccess) {
            std::free(b);
            hip_check(e, "hipMemcpy(progressive state)");
        }
        h.payload_checksum = fnv1a(b + sizeof h, (size_t)h.payload_bytes);
        h.header_checksum = fnv1a(&h, offsetof(ProgBlobHeader, header_checksum));
        std::memcpy(b, &h, sizeof h);
        *blob = b;
        *len = total;
    });
}

int rt_camera_progressive_restore(rt_camera* cam, const uint8_t* blob, size_t len) {
    return camera_call(cam, [&] {
        const ProgBlobHeader h = prog_parse_blob(blob, len);
        const RtCamera& C = cam->build.cam;
        auto refuse = [](const std::string& what) {
            throw std::invalid_argument("rt_camera_progressive_restore: the blob's " + what);
        };
        char bid[sizeof h.build_id] = {};
        std::strncpy(bid, RT_BUILD_ID, sizeof bid - 1);
        if (std::memcmp(bid, h.build_id, sizeof bid) != 0)
            refuse("build id " + std::string(h.build_id, strnlen(h.build_id, sizeof h.build_id)) +
                   " differs from this library's " + RT_BUILD_ID);
        if (h.width != C.width || h.height != C.height)
            refuse("image dimensions " + std::to_string(h.width) + "x" + std::to_string(h.height) +
                   " differ from the camera's " + std::to_string(C.width) + "x" + std::to_string(C.height));
        if (h.precision != cam->precision)
            refuse(std::string("precision ") + (h.precision == PREC_FP32 ? "fp32" : "ref") + " differs from the camera's " +
                   (cam->precision == PREC_FP32 ? "fp32" : "ref"));
        if (h.seed != C.seed)
            refuse("seed " + std::to_string(h.seed) + " differs from the camera's " + std::to_string(C.seed));
        if (std::memcmp(&h.samples, &C.samples, sizeof(double)) != 0 || h.samples_loop != C.n_samples)
            refuse("samples " + std::to_string(h.samples) + " differ from the camera's " + std::to_string(C.samples));
        if (h.fingerprint != prog_fingerprint(cam->build)) refuse("scene / render options fingerprint differs from the camera's");
        if (h.samples_done < 0 || h.samples_done > h.samples_loop || h.rx < 0 || h.ry < 0 || h.rx + h.rw > C.width ||
            h.ry + h.rh > C.height)
            refuse("header is inconsistent (region or sample count out of range)");
        DevCtx& c = cam->current();
        c.ensure_device();
        if (cam->prog && cam->prog != &c) cam->end_session();
        c.prog_alloc(rt_region{h.rx, h.ry, h.rw, h.rh}, h.precision);
        cam->prog = &c;
        try {
            DevCtx::ProgSession& P = c.prog;
            hip_check(hipMemcpy(P.d_state, blob + sizeof h, (size_t)h.payload_bytes, hipMemcpyHostToDevice),
                      "hipMemcpy(progressive state)");
            P.done = h.samples_done;
            P.steps = h.steps;
            P.err = h.err_flags;
            c.prog_start(nullptr);
            if (P.n_act != h.active_pixels) refuse("state does not match its header (active pixel count)");
        } catch (...) {
            cam->end_session();
            throw;
        }
    });
}

int rt_progressive_blob_info(const uint8_t* blob, size_t len, rt_progressive_info* info) {
    if (!info) return set_error(RT_ERR_INVALID, "null argument");
    try {
        prog_info_from_header(prog_parse_blob(blob, len), info);
        return RT_OK;
    } catch (const std::exception& e) {
        return set_error(RT_ERR_INVALID, e.what());
    }
}

int rt_progressive_blob_variance(const uint8_t* blob, size_t len, float* variance) {
    if (!variance) return set_error(RT_ERR_INVALID, "null argument");
    try {
        const ProgBlobHeader h = prog_parse_blob(blob, len);
        if (h.width <= 0 || h.height <= 0 || h.rx < 0 || h.ry < 0 || (long)h.rx + h.rw > h.width ||
            (long)h.ry + h.rh > h.height)
            throw std::invalid_argument("progressive blob: corrupt header (the region does not fit the image)");
        // the payload by slot = region tile * 64 + lane (the kernels' item_pixel numbering)
        const int tiles_x = (h.rw + kTile - 1) / kTile;
        const long slots = (long)(h.payload_bytes / sizeof(ProgPix));
        for (long slot = 0; slot < slots; ++slot) {
            const int tile = (int)(slot / kWave), lane = (int)(slot % kWave);
            const int ty = tile / tiles_x;
            const int i = h.rx + (tile - ty * tiles_x) * kTile + (lane & (kTile - 1));
            const int j = h.ry + ty * kTile + lane / kTile;
            if (i >= h.rx + h.rw || j >= h.ry + h.rh) continue;
            ProgPix p;
            std::memcpy(&p, blob + sizeof h + (size_t)slot * sizeof p, sizeof p);
            variance[(size_t)j * h.width + i] = prog_variance(p.ill.x, p.ill.y, prog_pix_samples(p));
        }
        return RT_OK;
    } catch (const std::exception& e) {
        return set_error(RT_ERR_INVALID, e.what());
    }
}

int rt_camera_progressive_end(rt_camera* cam) {
    return camera_call(cam, [&] { cam->end_session(); });
}

// ---- Guides and the a-trous filter ------------------------------------------------------------
int rt_camera_render_guides(rt_camera* cam, const rt_region* region, float* normal, float* position, float* distance,
                            int32_t* object) {
    return camera_call(cam, [&] {
        const RtCamera& C = cam->build.cam;
        const rt_region r = dn_region(region, C.width, C.height, "rt_camera_render_guides");
        DevCtx& c = cam->current();
        c.ensure_device();
        const hipStream_t stream = nullptr;
        const int n = r.width * r.height;
        DnBufs& b = c.dn;
        b.ensure((size_t)n);
        const DenoiseGuides g{b.gn, b.gp};
        c.launch_guide_pass(r, cam->traversal, g, stream);
        hip_check(launch_guides_unpack(g, n, b.nrm(), b.pos(), b.dist(), b.obj, stream), "guides_unpack_kernel");
        dn_download(normal, b.nrm(), 3 * sizeof(float), C.width, r, stream);
        dn_download(position, b.pos(), 3 * sizeof(float), C.width, r, stream);
        dn_download(distance, b.dist(), sizeof(float), C.width, r, stream);
        dn_download(object, b.obj, sizeof(int32_t), C.width, r, stream);
        hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");
    });
}

// The three shapes of a filter call, plain or variance-guided (o.var: `variance` in, or the
// session's own, and `variance_out`); `o` as dn_options gives it, resolved where the entry point
// always has. Every argument error comes before anything touches a device.

// The stand-alone frame call: explicit guides, buffers of its own.
static int dn_frame_call(const std::string& who, DnOpts o, int32_t width, int32_t height, const rt_region* region,
                         const float* radiance, const float* variance, const float* normal, const float* position,
                         const float* distance, const int32_t* object, float* radiance_out, float* variance_out,
                         uint8_t* rgb_out) {
    DnBufs b;
    int rc = RT_OK;
    try {
        if (width <= 0 || height <= 0) throw std::invalid_argument(who + ": width and height must be positive");
        if (!radiance || (o.var && !variance) || !normal || !position || !distance || !object)
            throw std::invalid_argument(who + ": radiance, " + (o.var ? "variance, " : "") +
                                        "normal, position, distance and object are required");
        o = dn_resolve(o, who);
        const rt_region r = dn_region(region, width, height, who);
        const hipStream_t stream = nullptr;
        const int n = r.width * r.height;
        b.ensure((size_t)n);
        dn_upload(b.rad(), radiance, 3 * sizeof(float), width, r, stream);
        if (o.var) {
            b.var.ensure((size_t)n, "hipMalloc(denoise variance)");
            dn_upload(b.var, variance, sizeof(float), width, r, stream);
        }
        dn_upload(b.nrm(), normal, 3 * sizeof(float), width, r, stream);
        dn_upload(b.pos(), position, 3 * sizeof(float), width, r, stream);
        dn_upload(b.dist(), distance, sizeof(float), width, r, stream);
        dn_upload(b.obj, object, sizeof(int32_t), width, r, stream);
        const DenoiseGuides g{b.gn, b.gp};
        hip_check(launch_guides_pack(g, n, b.nrm(), b.pos(), b.dist(), b.obj, stream), "guides_pack_kernel");
        dn_filter(b, b.gn, b.gp, b.rad(), r.width, 0, 0, r.width, r.height, o, radiance_out != nullptr,
                  rgb_out != nullptr, variance_out != nullptr, stream, nullptr);
        dn_download(radiance_out, b.rad(), 3 * sizeof(float), width, r, stream);
        if (o.var) dn_download(variance_out, b.var, sizeof(float), width, r, stream);
        dn_download(rgb_out, b.u8, 3, width, r, stream);
        hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");
    } catch (const HipError& e) {
        rc = set_error(RT_ERR_DEVICE, e.what());
    } catch (const std::invalid_argument& e) {
        rc = set_error(RT_ERR_INVALID, e.what());
    } catch (const std::exception& e) {
        rc = set_error(RT_ERR_RENDER, e.what());
    }
    b.free();
    return rc;
}

// The camera call: the guide pass of the camera's scene over the region, the camera's buffers.
static int dn_camera_call(rt_camera* cam, const std::string& who, DnOpts o, const rt_region* region,
                          const float* radiance, const float* variance, float* radiance_out, float* variance_out,
                          uint8_t* rgb_out) {
    return camera_call(cam, [&] {
        const RtCamera& C = cam->build.cam;
        if (!radiance || (o.var && !variance))
            throw std::invalid_argument(who + (o.var ? ": radiance and variance are required" : ": radiance is required"));
        o = dn_resolve(o, who);
        const rt_region r = dn_region(region, C.width, C.height, who);
        DevCtx& c = cam->current();
        c.ensure_device();
        const hipStream_t stream = nullptr;
        DnBufs& b = c.dn;
        b.ensure((size_t)r.width * r.height);
        hipEvent_t* ev = c.dn_events(o.levels);
        dn_upload(b.rad(), radiance, 3 * sizeof(float), C.width, r, stream);
        if (o.var) {
            b.var.ensure((size_t)r.width * r.height, "hipMalloc(denoise variance)");
            dn_upload(b.var, variance, sizeof(float), C.width, r, stream);
        }
        hip_check(hipEventRecord(ev[0], stream), "hipEventRecord");
        c.launch_guide_pass(r, cam->traversal, DenoiseGuides{b.gn, b.gp}, stream);
        c.dn_guides = true;
        dn_filter(b, b.gn, b.gp, b.rad(), r.width, 0, 0, r.width, r.height, o, radiance_out != nullptr,
                  rgb_out != nullptr, variance_out != nullptr, stream, ev + 1);
        dn_download(radiance_out, b.rad(), 3 * sizeof(float), C.width, r, stream);
        if (o.var) dn_download(variance_out, b.var, sizeof(float), C.width, r, stream);
        dn_download(rgb_out, b.u8, 3, C.width, r, stream);
        hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");
    });
}

// The open session's frames must be radiance.
static void session_radiance(rt_camera* cam, const std::string& who) {
    if (cam->build.cam.mode != MODE_DEFAULT)
        throw std::invalid_argument(who + ": the frames of mode bounces / samples are not radiance");
}

// The open session, on the current device, whose state holds radiance and at least min_samples
// samples per pixel (2: a variance). Argument errors first, then the device check.
static DevCtx& session_with(rt_camera* cam, const std::string& who, int min_samples) {
    DevCtx& c = cam->session(who.c_str());
    session_radiance(cam, who);
    if (c.prog.done < min_samples)
        throw std::invalid_argument(who + ": a variance needs at least 2 samples per pixel, the session has " +
                                    std::to_string(c.prog.done) + " (samples_done < 2)");
    int dev = 0;
    hip_check(hipGetDevice(&dev), "hipGetDevice");
    if (dev != c.device) throw std::invalid_argument(who + ": the session lives on another device");
    return c;
}

// The session's guides: computed once (queued), freed with the session.
static void session_guides(rt_camera* cam, DevCtx& c, hipStream_t stream) {
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

// The session's state -> b.var (region-packed); queued.
static void prog_variance_pass(DevCtx& c, hipStream_t stream) {
    DevCtx::ProgSession& P = c.prog;
    c.dn.var.ensure((size_t)P.region.width * P.region.height, "hipMalloc(denoise variance)");
    const int tiles_x = std::max((P.region.width + kTile - 1) / kTile, 1);
    hip_check(launch_prog_variance(P.d_state, (int)P.slots, c.prog_reg(), tiles_x, c.dn.var, stream),
              "prog_variance_kernel");
}

// The session call: the session's device frame (and, variance-guided, its state) as they stand
// after the last step - nothing is uploaded - and the session's guides.
static int dn_session_call(rt_camera* cam, const std::string& who, DnOpts o, uint8_t* rgb, float* radiance,
                           float* variance_out) {
    return camera_call(cam, [&] {
        (void)cam->session(who.c_str());
        // (the plain call names a wrong mode before its options, the variance-guided one its
        // options before the mode and the sample count)
        if (!o.var) session_radiance(cam, who);
        o = dn_resolve(o, who);
        DevCtx& c = session_with(cam, who, o.var ? 2 : 0);
        const RtCamera& C = cam->build.cam;
        DevCtx::ProgSession& P = c.prog;
        const rt_region r = P.region;
        const hipStream_t stream = nullptr;
        DnBufs& b = c.dn;
        b.ensure((size_t)r.width * r.height);
        hipEvent_t* ev = c.dn_events(o.levels);
        hip_check(hipEventRecord(ev[0], stream), "hipEventRecord");
        // the span [0, 1): the guide pass of a first call and, variance-guided, the variance pass
        c.dn_guides = o.var || !P.d_gn;
        session_guides(cam, c, stream);
        if (o.var) prog_variance_pass(c, stream);
        dn_filter(b, P.d_gn, P.d_gp, P.d_rad, C.width, r.x, r.y, r.width, r.height, o, radiance != nullptr, rgb != nullptr,
                  variance_out != nullptr, stream, ev + 1);
        dn_download(radiance, b.rad(), 3 * sizeof(float), C.width, r, stream);
        if (o.var) dn_download(variance_out, b.var, sizeof(float), C.width, r, stream);
        dn_download(rgb, b.u8, 3, C.width, r, stream);
        hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");
    });
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
        const hipStream_t stream = nullptr;
        prog_variance_pass(c, stream);
        dn_download(variance, c.dn.var, sizeof(float), cam->build.cam.width, c.prog.region, stream);
        hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");
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

// ---- Reprojection of a previous view's frame (reproject.hpp) -----------------------------------
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

// rt_reproject_options resolved: a zero field = the default.
struct RpOpts {
    float normal_min, sigma_plane, min_weight, nh;
};
static RpOpts rp_resolve(const rt_reproject_options* o, const std::string& who) {
    RpOpts r = o ? RpOpts{o->normal_min, o->sigma_plane, o->min_weight, o->history_samples} : RpOpts{0.0f, 0.0f, 0.0f, 0.0f};
    const std::pair<const char*, float> fields[] = {{"normal_min", r.normal_min},
                                                    {"sigma_plane", r.sigma_plane},
                                                    {"min_weight", r.min_weight},
                                                    {"history_samples", r.nh}};
    for (const auto& f : fields)
        if (!(f.second >= 0.0f) || !std::isfinite(f.second))
            throw std::invalid_argument(who + ": " + f.first + " must be positive and finite (0: the default)");
    if (r.normal_min == 0.0f) r.normal_min = 0.9f;
    if (r.sigma_plane == 0.0f) r.sigma_plane = 0.01f;
    if (r.min_weight == 0.0f) r.min_weight = 0.25f;
    if (r.nh == 0.0f) r.nh = 32.0f;
    return r;
}

// The argument errors every reproject entry shares (host only).
static void rp_check(const std::string& who, const float* prev_radiance, const float* radiance, int32_t samples,
                     const float* radiance_out, const uint8_t* rgb_out) {
    if (!prev_radiance) throw std::invalid_argument(who + ": prev_radiance is required");
    if ((radiance_out || rgb_out) && !radiance)
        throw std::invalid_argument(who + ": radiance_out and rgb_out need a fresh radiance to blend");
    if (samples < 0) throw std::invalid_argument(who + ": samples must not be negative");
}

static void rp_same_scene(const rt_camera* a, const rt_camera* b) {
    const SceneBuild &x = a->build, &y = b->build;
    if (a != b && !(same_bytes(x.nodes, y.nodes) && same_bytes(x.prims, y.prims) && same_bytes(x.mats, y.mats) &&
                    same_bytes(x.lights, y.lights) && same_bytes(x.prim_object, y.prim_object)))
        throw std::invalid_argument("reproject: the cameras hold different scenes");
}

// The new view's side of a call: its guides, and the fresh frame and sample counts to blend
// (null: history only) in one layout - row pitch `pitch` pixels, the region at (fx0, fy0).
struct RpNew {
    const float4 *gn, *gp;
    const float* fresh;
    const int32_t* pxs;
    int pitch, fx0, fy0;
    float m;
};

// The device side of a call once both views' guides and the previous radiance (pb.rad(),
// region-packed) are there: the previous colour packed as the plain filter packs it, the gather,
// then history -> nb.nrm(), weight -> nb.dist(), the blend -> nb.rad() / nb.u8. ev (or null):
// events 2..4, recorded before and after the gather and after the unpack passes. Queued.
static void rp_run(DnBufs& nb, DnBufs& pb, const RpView& view, const rt_region& r, const rt_region& pr,
                   const uint8_t* d_reusable, int n_objects, const RpOpts& o, const RpNew& nw, bool want_hist,
                   bool want_rad, bool want_u8, hipStream_t stream, hipEvent_t* ev) {
    auto mark = [&](int k) {
        if (ev) hip_check(hipEventRecord(ev[k], stream), "hipEventRecord");
    };
    hip_check(launch_denoise_pack(pb.rad(), pr.width, 0, 0, pr.width, pr.height, pb.gn, 1.0f, nullptr, pb.c0, pb.fn, stream),
              "denoise_pack_kernel");
    mark(2);
    RpArgs a{};
    a.view = view;
    a.w = r.width, a.h = r.height;
    a.px0 = pr.x, a.py0 = pr.y, a.pw = pr.width, a.ph = pr.height;
    a.n_objects = n_objects;
    a.normal_min = o.normal_min, a.sigma_plane = o.sigma_plane, a.min_weight = o.min_weight, a.nh = o.nh;
    a.pitch = nw.pitch, a.fx0 = nw.fx0, a.fy0 = nw.fy0;
    a.m = nw.m;
    hip_check(launch_reproject(a, nw.gn, nw.gp, pb.gn, pb.gp, pb.c0, d_reusable, nw.fresh, nw.pxs, nb.c0,
                               nw.fresh ? nb.c1.p : nullptr, stream),
              "reproject_kernel");
    mark(3);
    const int n = r.width * r.height;
    if (want_hist) hip_check(launch_denoise_unpack(nb.c0, n, nb.nrm(), nullptr, nb.dist(), stream), "denoise_unpack_kernel");
    if (nw.fresh && (want_rad || want_u8))
        hip_check(launch_denoise_unpack(nb.c1, n, want_rad ? nb.rad() : nullptr, want_u8 ? nb.u8.p : nullptr, nullptr, stream),
                  "denoise_unpack_kernel");
    mark(4);
}

int rt_reproject(int32_t width, int32_t height, const rt_region* region, const float* normal, const float* position,
                 const float* distance, const int32_t* object, const rt_view* prev_view, const rt_region* prev_region,
                 const float* prev_radiance, const float* prev_normal, const float* prev_position,
                 const float* prev_distance, const int32_t* prev_object, const uint8_t* reusable, int32_t n_objects,
                 const rt_reproject_options* options, const float* radiance, const int32_t* px_samples, int32_t samples,
                 float* history_out, float* weight_out, float* radiance_out, uint8_t* rgb_out) {
    const std::string who = "rt_reproject";
    DnBufs nb, pb;
    DevBuf<uint8_t> d_reusable;
    int rc = RT_OK;
    try {
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
        const rt_region r = dn_region(region, width, height, who);
        const rt_region pr = dn_region(prev_region, prev_view->width, prev_view->height, who);
        const RpView view = rp_view_constants(prev_view->center, prev_view->pixel00, prev_view->du, prev_view->dv,
                                              prev_view->width, prev_view->height);
        const hipStream_t stream = nullptr;
        const int n = r.width * r.height, np = pr.width * pr.height;
        nb.ensure((size_t)n);
        pb.ensure((size_t)np);
        d_reusable.ensure((size_t)std::max(n_objects, 1), "hipMalloc(reusable objects)");
        if (n_objects > 0)
            hip_check(hipMemcpyAsync(d_reusable, reusable, (size_t)n_objects, hipMemcpyHostToDevice, stream), "hipMemcpyAsync");
        dn_upload(nb.nrm(), normal, 3 * sizeof(float), width, r, stream);
        dn_upload(nb.pos(), position, 3 * sizeof(float), width, r, stream);
        dn_upload(nb.dist(), distance, sizeof(float), width, r, stream);
        dn_upload(nb.obj, object, sizeof(int32_t), width, r, stream);
        hip_check(launch_guides_pack(DenoiseGuides{nb.gn, nb.gp}, n, nb.nrm(), nb.pos(), nb.dist(), nb.obj, stream),
                  "guides_pack_kernel");
        dn_upload(pb.nrm(), prev_normal, 3 * sizeof(float), prev_view->width, pr, stream);
        dn_upload(pb.pos(), prev_position, 3 * sizeof(float), prev_view->width, pr, stream);
        dn_upload(pb.dist(), prev_distance, sizeof(float), prev_view->width, pr, stream);
        dn_upload(pb.obj, prev_object, sizeof(int32_t), prev_view->width, pr, stream);
        hip_check(launch_guides_pack(DenoiseGuides{pb.gn, pb.gp}, np, pb.nrm(), pb.pos(), pb.dist(), pb.obj, stream),
                  "guides_pack_kernel");
        dn_upload(pb.rad(), prev_radiance, 3 * sizeof(float), prev_view->width, pr, stream);
        // (the guides are packed: the staging arrays now carry the fresh frame and the counts)
        if (radiance) dn_upload(nb.rad(), radiance, 3 * sizeof(float), width, r, stream);
        if (radiance && px_samples) dn_upload(nb.obj, px_samples, sizeof(int32_t), width, r, stream);
        const RpNew nw{nb.gn, nb.gp, radiance ? nb.rad() : nullptr, radiance && px_samples ? nb.obj.p : nullptr,
                       r.width, 0, 0, (float)samples};
        rp_run(nb, pb, view, r, pr, d_reusable, n_objects, o, nw, history_out || weight_out, radiance_out != nullptr,
               rgb_out != nullptr, stream, nullptr);
        dn_download(history_out, nb.nrm(), 3 * sizeof(float), width, r, stream);
        dn_download(weight_out, nb.dist(), sizeof(float), width, r, stream);
        dn_download(radiance_out, nb.rad(), 3 * sizeof(float), width, r, stream);
        dn_download(rgb_out, nb.u8, 3, width, r, stream);
        hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");
    } catch (const HipError& e) {
        rc = set_error(RT_ERR_DEVICE, e.what());
    } catch (const std::invalid_argument& e) {
        rc = set_error(RT_ERR_INVALID, e.what());
    } catch (const std::exception& e) {
        rc = set_error(RT_ERR_RENDER, e.what());
    }
    nb.free();
    pb.free();
    d_reusable.reset();
    return rc;
}

// The previous view's side of a camera call, on the current device: its context with the
// radiance uploaded into rp_prev.rad() and the guide pass queued into rp_prev.gn / gp.
static DnBufs& rp_prev_side(rt_camera* prev_cam, const rt_region& pr, const float* prev_radiance, hipStream_t stream,
                            hipEvent_t* ev, const std::function<void()>& new_guides) {
    DevCtx& p = prev_cam->current();
    p.ensure_device();
    DnBufs& pb = p.rp_prev;
    pb.ensure((size_t)pr.width * pr.height);
    dn_upload(pb.rad(), prev_radiance, 3 * sizeof(float), prev_cam->build.cam.width, pr, stream);
    hip_check(hipEventRecord(ev[0], stream), "hipEventRecord");
    new_guides();
    p.launch_guide_pass(pr, prev_cam->traversal, DenoiseGuides{pb.gn, pb.gp}, stream);
    hip_check(hipEventRecord(ev[1], stream), "hipEventRecord");
    return pb;
}

static RpView rp_camera_view(const rt_camera* cam) {
    const RtCamera& C = cam->build.cam;
    return rp_view_constants(C.center, C.pixel00, C.du, C.dv, C.width, C.height);
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
        const rt_region r = dn_region(region, C.width, C.height, who);
        const rt_region pr = dn_region(prev_region, PC.width, PC.height, who);
        rp_same_scene(cam, prev_cam);
        DevCtx& c = cam->current();
        c.ensure_device();
        const hipStream_t stream = nullptr;
        DnBufs& nb = c.dn;
        nb.ensure((size_t)r.width * r.height);
        hipEvent_t* ev = c.rp_events();
        const uint8_t* d_reusable = c.ensure_reusable();
        if (radiance) dn_upload(nb.rad(), radiance, 3 * sizeof(float), C.width, r, stream);
        if (radiance && px_samples) dn_upload(nb.obj, px_samples, sizeof(int32_t), C.width, r, stream);
        DnBufs& pb = rp_prev_side(prev_cam, pr, prev_radiance, stream, ev, [&] {
            c.launch_guide_pass(r, cam->traversal, DenoiseGuides{nb.gn, nb.gp}, stream);
        });
        const RpNew nw{nb.gn, nb.gp, radiance ? nb.rad() : nullptr, radiance && px_samples ? nb.obj.p : nullptr,
                       r.width, 0, 0, (float)samples};
        rp_run(nb, pb, rp_camera_view(prev_cam), r, pr, d_reusable, C.n_prims, o, nw, history_out || weight_out,
               radiance_out != nullptr, rgb_out != nullptr, stream, ev);
        c.rp_timed = true;
        dn_download(history_out, nb.nrm(), 3 * sizeof(float), C.width, r, stream);
        dn_download(weight_out, nb.dist(), sizeof(float), C.width, r, stream);
        dn_download(radiance_out, nb.rad(), 3 * sizeof(float), C.width, r, stream);
        dn_download(rgb_out, nb.u8, 3, C.width, r, stream);
        hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");
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
        const rt_region r = P.region;
        const hipStream_t stream = nullptr;
        DnBufs& nb = c.dn;
        nb.ensure((size_t)r.width * r.height);
        hipEvent_t* ev = c.rp_events();
        const uint8_t* d_reusable = c.ensure_reusable();
        DnBufs& pb = rp_prev_side(prev_cam, pr, prev_radiance, stream, ev, [&] { session_guides(cam, c, stream); });
        const RpNew nw{P.d_gn, P.d_gp, P.d_rad, P.d_pxs, C.width, r.x, r.y, 0.0f};
        rp_run(nb, pb, rp_camera_view(prev_cam), r, pr, d_reusable, C.n_prims, o, nw, weight_out != nullptr,
               radiance != nullptr, rgb != nullptr, stream, ev);
        c.rp_timed = true;
        dn_download(weight_out, nb.dist(), sizeof(float), C.width, r, stream);
        dn_download(radiance, nb.rad(), 3 * sizeof(float), C.width, r, stream);
        dn_download(rgb, nb.u8, 3, C.width, r, stream);
        hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");
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

// ---- Accumulation across views (temporal.hpp) ---------------------------------------------------
// rt_temporal_options resolved: a zero field = the default; levels 0 = no filter.
struct TpOpts {
    float normal_min, sigma_plane, min_weight, max_history;
    int32_t levels;
    float sigma_variance;
};
static TpOpts tp_resolve(const rt_temporal_options* o, const std::string& who) {
    TpOpts r = o ? TpOpts{o->normal_min, o->sigma_plane, o->min_weight, o->max_history, o->filter_levels, o->sigma_variance}
                 : TpOpts{0.0f, 0.0f, 0.0f, 0.0f, 0, 0.0f};
    const std::pair<const char*, float> fields[] = {{"normal_min", r.normal_min},
                                                    {"sigma_plane", r.sigma_plane},
                                                    {"min_weight", r.min_weight},
                                                    {"max_history", r.max_history},
                                                    {"sigma_variance", r.sigma_variance}};
    for (const auto& f : fields)
        if (!(f.second >= 0.0f) || !std::isfinite(f.second))
            throw std::invalid_argument(who + ": " + f.first + " must be positive and finite (0: the default)");
    if (r.levels < 0 || r.levels > kDenoiseMaxLevels)
        throw std::invalid_argument(who + ": filter_levels must be 0.." + std::to_string(kDenoiseMaxLevels) +
                                    " (0: no filter)");
    if (r.normal_min == 0.0f) r.normal_min = 0.9f;
    if (r.sigma_plane == 0.0f) r.sigma_plane = 0.01f;
    if (r.min_weight == 0.0f) r.min_weight = 0.25f;
    if (r.max_history == 0.0f) r.max_history = 256.0f;
    if (r.sigma_variance == 0.0f) r.sigma_variance = 2.0f;
    return r;
}

// The hash a history keeps of its scene: the arrays rp_same_scene compares.
static uint64_t tp_scene_hash(const SceneBuild& b) {
    uint64_t f = fnv1a(b.nodes.data(), b.nodes.size() * sizeof(RtNode));
    f = fnv1a(b.prims.data(), b.prims.size() * sizeof(RtPrim), f);
    f = fnv1a(b.mats.data(), b.mats.size() * sizeof(RtMat), f);
    f = fnv1a(b.lights.data(), b.lights.size() * sizeof(RtLight), f);
    return fnv1a(b.prim_object.data(), b.prim_object.size() * sizeof(int32_t), f);
}

// The new view's side of a call: its guides, the fresh frame and sample counts in one layout (row
// pitch `pitch` pixels, the region at (fx0, fy0)) and the region-packed fresh variance.
struct TpNew {
    const float4 *gn, *gp;
    const float* fresh;
    const int32_t* pxs;
    int pitch, fx0, fy0;
    const float* var;
    float m;
};

// The device side of a call: the gather and blend into `out` (weight -> b.dist()), then the
// caller's outputs - the optional variance-guided filter of out / Vout, else out itself - into
// b.rad() / b.u8 / b.var, and the length into b.nrm(). pr.width == 0: an empty history. ev (or
// null): events 2 and 3, recorded after the gather and after the filter. Queued.
static void tp_run(DnBufs& b, const TpNew& nw, const rt_region& r, const TpHistory& hist, const RpView& view,
                   const rt_region& pr, const uint8_t* d_reusable, int n_objects, const TpOpts& o, float4* out_col,
                   float* out_var, bool want_rad, bool want_u8, bool want_var, bool want_len, hipStream_t stream,
                   hipEvent_t* ev) {
    const int n = r.width * r.height;
    TpArgs a{};
    a.view = view;
    a.w = r.width, a.h = r.height;
    a.px0 = pr.x, a.py0 = pr.y, a.pw = pr.width, a.ph = pr.height;
    a.n_objects = n_objects;
    a.normal_min = o.normal_min, a.sigma_plane = o.sigma_plane, a.min_weight = o.min_weight, a.max_history = o.max_history;
    a.pitch = nw.pitch, a.fx0 = nw.fx0, a.fy0 = nw.fy0;
    a.vpitch = r.width, a.vx0 = 0, a.vy0 = 0;
    a.m = nw.m;
    hip_check(launch_temporal(a, nw.gn, nw.gp, hist, d_reusable, nw.fresh, nw.pxs, nw.var, TpOut{out_col, out_var, b.dist()},
                              stream),
              "temporal_kernel");
    if (ev) hip_check(hipEventRecord(ev[2], stream), "hipEventRecord");
    const bool filter = o.levels > 0 && (want_rad || want_u8 || want_var);
    if (filter || want_var) {
        // (the kernel has read the fresh variance, which may be b.var itself)
        b.var.ensure((size_t)n, "hipMalloc(denoise variance)");
        hip_check(hipMemcpyAsync(b.var, out_var, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, stream), "hipMemcpyAsync");
    }
    if (filter) {
        hip_check(launch_denoise_unpack(out_col, n, b.rad(), nullptr, nullptr, stream), "denoise_unpack_kernel");
        dn_filter(b, nw.gn, nw.gp, b.rad(), r.width, 0, 0, r.width, r.height,
                  DnOpts{true, o.levels, o.sigma_variance, o.sigma_plane}, want_rad, want_u8, want_var, stream, nullptr);
    }
    if (ev) hip_check(hipEventRecord(ev[3], stream), "hipEventRecord");
    if (!filter && (want_rad || want_u8))
        hip_check(launch_denoise_unpack(out_col, n, want_rad ? b.rad() : nullptr, want_u8 ? b.u8.p : nullptr, nullptr, stream),
                  "denoise_unpack_kernel");
    if (want_len) hip_check(launch_denoise_unpack(out_col, n, nullptr, nullptr, b.nrm(), stream), "denoise_unpack_kernel");
}

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
        const hipStream_t stream = nullptr;
        const rt_history::Side& s = h->side[h->front];
        const rt_region& r = h->region;
        const int n = r.width * r.height;
        DnBufs b;  // staging of this call alone
        b.ensure((size_t)n);
        hip_check(launch_denoise_unpack(s.col, n, radiance ? b.rad() : nullptr, nullptr, length ? b.dist() : nullptr, stream),
                  "denoise_unpack_kernel");
        dn_download(radiance, b.rad(), 3 * sizeof(float), h->width, r, stream);
        dn_download(length, b.dist(), sizeof(float), h->width, r, stream);
        dn_download(variance, s.var, sizeof(float), h->width, r, stream);
        hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");
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
        const rt_region r = P.region;
        const size_t n = (size_t)r.width * r.height;
        const hipStream_t stream = nullptr;
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
            t.resize(std::max<size_t>(t.size(), 1), 0);
            h->d_reusable.ensure(t.size(), "hipMalloc(reusable objects)");
            hip_check(hipMemcpy(h->d_reusable, t.data(), t.size(), hipMemcpyHostToDevice), "hipMemcpy");
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
        const TpNew nw{P.d_gn, P.d_gp, P.d_rad, P.d_pxs, C.width, r.x, r.y, b.var, 0.0f};
        tp_run(b, nw, r, hist, h->rp_view, pr, h->d_reusable, h->n_objects, o, back.col, back.var, radiance != nullptr,
               rgb != nullptr, variance_out != nullptr, length_out != nullptr, stream, h->ev);
        if (commit) {
            // the session may be gone before the next view: the history keeps the guides itself
            hip_check(hipMemcpyAsync(back.gn, P.d_gn, n * sizeof(float4), hipMemcpyDeviceToDevice, stream), "hipMemcpyAsync");
            hip_check(hipMemcpyAsync(back.gp, P.d_gp, n * sizeof(float4), hipMemcpyDeviceToDevice, stream), "hipMemcpyAsync");
        }
        hip_check(hipEventRecord(h->ev[4], stream), "hipEventRecord");
        h->timed = true;
        h->filtered = o.levels > 0 && (radiance || rgb || variance_out);
        dn_download(radiance, b.rad(), 3 * sizeof(float), C.width, r, stream);
        dn_download(rgb, b.u8, 3, C.width, r, stream);
        dn_download(variance_out, b.var, sizeof(float), C.width, r, stream);
        dn_download(length_out, b.nrm(), sizeof(float), C.width, r, stream);
        dn_download(weight_out, b.dist(), sizeof(float), C.width, r, stream);
        hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");
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
    const std::string who = "rt_temporal_accumulate";
    DnBufs nb, pb;
    rt_history::Side out;
    DevBuf<float> d_var;
    DevBuf<uint8_t> d_reusable;
    int rc = RT_OK;
    try {
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
        const rt_region r = dn_region(region, width, height, who);
        const rt_region pr = dn_region(prev_region, prev_view->width, prev_view->height, who);
        const RpView view = rp_view_constants(prev_view->center, prev_view->pixel00, prev_view->du, prev_view->dv,
                                              prev_view->width, prev_view->height);
        const hipStream_t stream = nullptr;
        const int n = r.width * r.height, np = pr.width * pr.height;
        nb.ensure((size_t)n);
        pb.ensure((size_t)np);
        pb.var.ensure((size_t)np, "hipMalloc(history)");
        out.ensure((size_t)n);
        d_var.ensure((size_t)n, "hipMalloc(denoise variance)");
        d_reusable.ensure((size_t)std::max(n_objects, 1), "hipMalloc(reusable objects)");
        if (n_objects > 0)
            hip_check(hipMemcpyAsync(d_reusable, reusable, (size_t)n_objects, hipMemcpyHostToDevice, stream), "hipMemcpyAsync");
        dn_upload(nb.nrm(), normal, 3 * sizeof(float), width, r, stream);
        dn_upload(nb.pos(), position, 3 * sizeof(float), width, r, stream);
        dn_upload(nb.dist(), distance, sizeof(float), width, r, stream);
        dn_upload(nb.obj, object, sizeof(int32_t), width, r, stream);
        hip_check(launch_guides_pack(DenoiseGuides{nb.gn, nb.gp}, n, nb.nrm(), nb.pos(), nb.dist(), nb.obj, stream),
                  "guides_pack_kernel");
        dn_upload(pb.nrm(), prev_normal, 3 * sizeof(float), prev_view->width, pr, stream);
        dn_upload(pb.pos(), prev_position, 3 * sizeof(float), prev_view->width, pr, stream);
        dn_upload(pb.dist(), prev_distance, sizeof(float), prev_view->width, pr, stream);
        dn_upload(pb.obj, prev_object, sizeof(int32_t), prev_view->width, pr, stream);
        hip_check(launch_guides_pack(DenoiseGuides{pb.gn, pb.gp}, np, pb.nrm(), pb.pos(), pb.dist(), pb.obj, stream),
                  "guides_pack_kernel");
        // (the guides are packed: the staging arrays now carry the frames, the length and the counts)
        dn_upload(pb.rad(), prev_radiance, 3 * sizeof(float), prev_view->width, pr, stream);
        dn_upload(pb.dist(), prev_length, sizeof(float), prev_view->width, pr, stream);
        dn_upload(pb.var, prev_variance, sizeof(float), prev_view->width, pr, stream);
        hip_check(launch_temporal_pack(pb.rad(), pb.dist(), np, pb.c0, stream), "temporal_pack_kernel");
        dn_upload(nb.pos(), radiance, 3 * sizeof(float), width, r, stream);
        dn_upload(d_var, variance, sizeof(float), width, r, stream);
        if (px_samples) dn_upload(nb.obj, px_samples, sizeof(int32_t), width, r, stream);
        const TpNew nw{nb.gn, nb.gp, nb.pos(), px_samples ? nb.obj.p : nullptr, r.width, 0, 0, d_var, (float)samples};
        tp_run(nb, nw, r, TpHistory{pb.gn, pb.gp, pb.c0, pb.var}, view, pr, d_reusable, n_objects, o, out.col, out.var,
               radiance_out != nullptr, rgb_out != nullptr, variance_out != nullptr, length_out != nullptr, stream, nullptr);
        dn_download(radiance_out, nb.rad(), 3 * sizeof(float), width, r, stream);
        dn_download(rgb_out, nb.u8, 3, width, r, stream);
        dn_download(variance_out, nb.var, sizeof(float), width, r, stream);
        dn_download(length_out, nb.nrm(), sizeof(float), width, r, stream);
        dn_download(weight_out, nb.dist(), sizeof(float), width, r, stream);
        hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");
    } catch (const HipError& e) {
        rc = set_error(RT_ERR_DEVICE, e.what());
    } catch (const std::invalid_argument& e) {
        rc = set_error(RT_ERR_INVALID, e.what());
    } catch (const std::exception& e) {
        rc = set_error(RT_ERR_RENDER, e.what());
    }
    nb.free();
    pb.free();
    out = rt_history::Side{};
    d_var.reset();
    d_reusable.reset();
    return rc;
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

// ---- Focused steps (focus.hpp) ------------------------------------------------------------------
void rt_focus_options_default(rt_focus_options* options) {
    if (options) *options = rt_focus_options{RT_FOCUS_SCORE_VARIANCE, 250, 0.0f, 0};
}

int rt_camera_progressive_focus(rt_camera* cam, int32_t n_samples, const rt_focus_options* options, const float* score,
                                rt_history* h, uint8_t* rgb, float* radiance, int32_t* px_samples, int32_t* px_bounces,
                                uint8_t* selected_out, rt_render_stats* stats, rt_focus_info* info) {
    const std::string who = "rt_camera_progressive_focus";
    rt_focus_options o;
    rt_focus_options_default(&o);
    if (options) o = *options;
    std::unique_lock<std::mutex> hlock;
    if (h && o.source == RT_FOCUS_SCORE_HISTORY) hlock = std::unique_lock<std::mutex>(h->mu);
    return camera_call(cam, [&] {
        // argument errors first, all of them before any device call
        if (n_samples <= 0 || n_samples > 65535)
            throw std::invalid_argument(who + ": n_samples must be in 1..65535 (the pool kernel's 16-bit sample field)");
        if (o.permille < 1 || o.permille > 1000) throw std::invalid_argument(who + ": permille must be in 1..1000");
        if (!(o.min_score >= 0.0f) || !std::isfinite(o.min_score))
            throw std::invalid_argument(who + ": min_score must be finite and not negative");
        if (o.max_pixels < 0) throw std::invalid_argument(who + ": max_pixels must not be negative");
        if (o.source != RT_FOCUS_SCORE_VARIANCE && o.source != RT_FOCUS_SCORE_MAP && o.source != RT_FOCUS_SCORE_HISTORY)
            throw std::invalid_argument(who + ": source must be one of RT_FOCUS_SCORE_*");
        if (o.source == RT_FOCUS_SCORE_MAP && !score) throw std::invalid_argument(who + ": the score map is required");
        if (o.source == RT_FOCUS_SCORE_HISTORY && !h) throw std::invalid_argument(who + ": the history is required");
        DevCtx& c = cam->session(who.c_str());
        session_radiance(cam, who);
        DevCtx::ProgSession& P = c.prog;
        const RtCamera& C = cam->build.cam;
        if (o.source == RT_FOCUS_SCORE_VARIANCE && P.done < 2)
            throw std::invalid_argument(who + ": a variance needs at least 2 samples per pixel, the session has " +
                                        std::to_string(P.done) + " (samples_done < 2)");
        if (o.source == RT_FOCUS_SCORE_HISTORY) {
            const rt_region& r = h->region;
            if (h->views <= 0) throw std::invalid_argument(who + ": the history is empty");
            if (h->device != c.device) throw std::invalid_argument(who + ": the history was committed on another device");
            if (h->width != C.width || h->height != C.height || r.x != P.region.x || r.y != P.region.y ||
                r.width != P.region.width || r.height != P.region.height)
                throw std::invalid_argument(who + ": the history's last committed region and image size are not the session's");
        }
        if ((long long)C.n_samples + P.focus_done + n_samples > (long long)INT32_MAX)
            throw std::invalid_argument(who + ": the sample index would exceed INT32_MAX");
        int dev = 0;
        hip_check(hipGetDevice(&dev), "hipGetDevice");
        if (dev != c.device) throw std::invalid_argument(who + ": the session lives on another device");
        const hipStream_t stream = nullptr;
        const int len = n_samples;
        rt_focus_info fi{};
        fi.active = P.n_act;
        fi.first_sample = C.n_samples + P.focus_done;
        if (P.n_act > 0) {  // (a finished session has nothing to select)
            c.prog_focus_alloc();
            long long k = ((long long)P.n_act * o.permille + 999) / 1000;
            if (o.max_pixels > 0) k = std::min<long long>(k, o.max_pixels);
            FocusArgs a{};
            a.act = P.d_act;
            a.n_act = (int32_t)P.n_act;
            a.k = (uint32_t)k;
            std::memcpy(&a.min_bits, &o.min_score, sizeof a.min_bits);
            if (o.min_score == 0.0f) a.min_bits = 0u;  // (-0)
            a.state = P.d_state;
            a.plane = nullptr;
            if (o.source == RT_FOCUS_SCORE_MAP) {
                hip_check(hipMemcpyAsync(P.d_fmap, score, (size_t)P.region.width * P.region.height * sizeof(float),
                                         hipMemcpyHostToDevice, stream),
                          "hipMemcpyAsync");
                a.plane = P.d_fmap;
            } else if (o.source == RT_FOCUS_SCORE_HISTORY) {
                a.plane = h->side[h->front].var;
            }
            a.tiles_x = std::max((P.region.width + kTile - 1) / kTile, 1);
            a.w = P.region.width, a.h = P.region.height;
            a.x0 = P.region.x, a.y0 = P.region.y, a.pitch = C.width;
            a.key = P.d_fkey;
            a.words = P.d_fwords;
            a.list = P.d_focus;
            a.mask = selected_out ? P.d_fmask.p : nullptr;
            if (selected_out)
                hip_check(hipMemsetAsync(P.d_fmask, 0, (size_t)C.width * C.height, stream), "hipMemsetAsync");
            hip_check(hipEventRecord(P.fev[0], stream), "hipEventRecord");
            hip_check(launch_focus_select(a, stream), "focus kernels launch");
            hip_check(hipEventRecord(P.fev[1], stream), "hipEventRecord");
            // the one host sync of the selection: the launch plan needs the count (as prog_read)
            hip_check(hipMemcpyAsync(P.h_fwords, P.d_fwords, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, stream),
                      "hipMemcpyAsync");
            hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");
            hip_check(hipEventElapsedTime(&fi.select_ms, P.fev[0], P.fev[1]), "hipEventElapsedTime");
            fi.selected = P.h_fwords[kFocusSelected];
            fi.eligible = P.h_fwords[kFocusEligible];
            std::memcpy(&fi.threshold, &P.h_fwords[kFocusThreshold], sizeof fi.threshold);
            if (fi.selected > 0) {
                cam->last = &c;
                cam->multi.clear();
                const ProgStep step{P.d_focus, (long)fi.selected, fi.first_sample, len};
                c.launch(P.region, 0, 1, P.precision, cam->traversal, 0, P.d_rgb, P.d_rad, P.d_pxs, P.d_pxb, 0, stream,
                         &step);
                c.prog_read(stream);
                P.focus_done += len;
                P.focused = true;
                ++P.steps;
            }
        } else if (selected_out) {
            c.prog_focus_alloc();
            hip_check(hipMemsetAsync(P.d_fmask, 0, (size_t)C.width * C.height, stream), "hipMemsetAsync");
        }
        fi.focus_done = P.focus_done;
        if (info) *info = fi;
        DevCtx::stats_from_words(P.words, stats);  // throws the render errors of the samples kept
        prog_copy_out(c, rgb, P.d_rgb, 3, stream);
        prog_copy_out(c, radiance, P.d_rad, 3 * sizeof(float), stream);
        prog_copy_out(c, px_samples, P.d_pxs, sizeof(int32_t), stream);
        prog_copy_out(c, px_bounces, P.d_pxb, sizeof(int32_t), stream);
        prog_copy_out(c, selected_out, P.d_fmask, 1, stream);
        hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");
    });
}

int rt_camera_release_device(rt_camera* cam) {
    if (!cam) return set_error(RT_ERR_INVALID, "null camera");
    std::lock_guard<std::mutex> lock(cam->mu);
    cam->release();
    return RT_OK;
}

const char* rt_build_id(void) { return RT_BUILD_ID; }

int rt_tiles_unpack(const void* slabs, int32_t tile_groups, int32_t slab_tiles, const rt_region* region,
                    int32_t width, int32_t height, int32_t channels, int32_t elem_bytes, void* frame, void* stream) {
    if (!region || tile_groups < 1 || slab_tiles < 0 || width < 0 || height < 0 || channels < 1 ||
        (elem_bytes != 1 && elem_bytes != 4) || (slab_tiles > 0 && (!slabs || !frame)))
        return set_error(RT_ERR_INVALID, "rt_tiles_unpack: bad arguments");
    try {
        // the region clamped to the image, as the render launch clamps it
        const rt_region r = clamp_region(*region, width, height);
        const RtRegion reg{r.x, r.y, r.width, r.height, 0, 1};
        const long tiles = (long)((reg.width + kTile - 1) / kTile) * ((reg.height + kTile - 1) / kTile);
        if ((long)slab_tiles * tile_groups < tiles)
            throw std::invalid_argument("rt_tiles_unpack: slabs hold fewer tiles than the region");
        hip_check(launch_tiles_unpack(slabs, tile_groups, slab_tiles, reg, width, channels, elem_bytes, frame,
                                      (hipStream_t)stream),
                  "tiles_unpack_kernel");
        return RT_OK;
    } catch (const std::invalid_argument& e) {
        return set_error(RT_ERR_INVALID, e.what());
    } catch (const std::exception& e) {
        return set_error(RT_ERR_DEVICE, e.what());
    }
}

int rt_device_count(int32_t* count) {
    if (!count) return set_error(RT_ERR_INVALID, "null argument");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    *count = n;
    return RT_OK;
}

}  // extern "C"
