// C ABI of the path-tracing core (include/rt_amd.h).
//
// rt_camera = the reference's Camera object after createCameraFromSceneData:
// the host build (scene.cpp) plus lazily allocated device copies. Rendering
// follows Camera.renderRegion's contract: the caller owns the output buffer,
// only the region is written, RenderStats are returned. This unit is the ABI layer of the
// scene, camera, render, debug, multi-GPU and session entries: argument checks and the call
// sequences over dev_ctx.hpp's contexts, under api_call.hpp's error mapping. The frame passes
// have units of their own (api_denoise / api_reproject / api_temporal / api_focus.cpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "json.hpp"
#include "pass_host.hpp"
#include "prog_blob.hpp"

using namespace rt;

// png.hip: the frame's PNG, encoded on the device queue `stream` (waited for).
std::vector<uint8_t> rt_png_encode_device(const uint8_t* d_rgb, int32_t w, int32_t h, hipStream_t stream);

static_assert(ST_WORDS == RT_STATS_WORDS, "rt_camera_stats_words layout");
static_assert(kMaxPhases == RT_PLAN_MAX_PHASES, "rt_launch_plan schedule arrays");

#ifndef RT_BUILD_ID
#define RT_BUILD_ID "unhashed"
#endif

static thread_local std::string g_error;

int rt::set_error(int code, const std::string& msg) {
    g_error = msg;
    return code;
}

// error hook for the other translation units of the library (image.cpp)
int rt_set_error_message(int code, const char* msg) { return set_error(code, msg ? msg : ""); }

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
                             "[rt scene] prims %zu t4nodes %zu (%zu B) tprims %zu B tsph %zu B prims %zu B "
                             "mats %zu B lights %zu B nodes %zu stack_depth %d\n",
                             b.prims.size(), b.t4nodes.size(), b.t4nodes.size() * sizeof(b.t4nodes[0]),
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
    // effective traversal: fast/brute only where provably exact (scene_tree.cpp prims_inside_boxes)
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
    return camera_call(cam, [&] {
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
    });
}

int rt_camera_render(rt_camera* cam, uint8_t* rgb, float* radiance, rt_render_stats* stats) {
    if (!cam) return set_error(RT_ERR_INVALID, "null camera");
    rt_region r{0, 0, cam->build.cam.width, cam->build.cam.height};
    return rt_camera_render_region(cam, &r, rgb, radiance, stats);
}

int rt_camera_render_png(rt_camera* cam, int32_t bands, rt_render_stats* stats, uint8_t** out, size_t* out_len) {
    if (!cam || !out || !out_len) return set_error(RT_ERR_INVALID, "null argument");
    return camera_call(cam, [&] {
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
    });
}

int rt_camera_render_device(rt_camera* cam, const rt_launch* L, rt_render_stats* stats, uint64_t* work_counters) {
    if (!cam || !L) return set_error(RT_ERR_INVALID, "null argument");
    return camera_call(cam, [&] {
        const hipStream_t stream = (hipStream_t)L->stream;
        DevCtx& c = cam->current(stream);
        c.ensure_device();
        const int prec = L->precision < 0 ? cam->precision : L->precision;
        const int trav = L->traversal < 0 ? cam->traversal : L->traversal;
        if (L->count_work < 0 || L->count_work > 2) throw std::invalid_argument("count_work must be 0, 1 or 2");
        cam->last = &c;
        cam->multi.clear();
        try {
            c.launch(L->region, L->tile_group, L->tile_groups, prec, trav, L->count_work, L->rgb, L->radiance,
                     L->px_samples, L->px_bounces, L->packed_tiles, stream);
        } catch (...) {  // (what it queued before it threw is ordered like a launch)
            c.order_mark(stream, false);
            throw;
        }
        if (L->synchronize) c.read_stats(stats, L->count_work ? work_counters : nullptr, stream);
        else c.order_mark(stream);
    });
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

namespace {
int debug_world_hit(rt_camera* cam, int prec, int32_t traversal, int32_t n, const float* orig, const float* dir,
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
        hip_check((prec == PREC_FP32 ? launch_world_hit_fp32 : launch_world_hit_ref)(c.dev_scene(), trav, n, d_o, d_d,
                                                                                     d_out, nullptr),
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
}  // namespace

int rt_debug_world_hit(rt_camera* cam, int32_t traversal, int32_t n, const float* orig, const float* dir,
                       double* out) {
    return debug_world_hit(cam, PREC_REF, traversal, n, orig, dir, out);
}

int rt_debug_world_hit_fp32(rt_camera* cam, int32_t traversal, int32_t n, const float* orig, const float* dir,
                            double* out) {
    return debug_world_hit(cam, PREC_FP32, traversal, n, orig, dir, out);
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
        c->order_after((hipStream_t)stream);
        // the ST_WORDS words sit kStatStride apart (one 128-B line each); dst gets them packed
        hip_check(hipMemcpy2DAsync(dst, sizeof(uint64_t), c->d_stats, kStatStride * sizeof(unsigned long long),
                                   sizeof(uint64_t), ST_WORDS, hipMemcpyDeviceToDevice, (hipStream_t)stream),
                  "hipMemcpy2DAsync(stats)");
        c->order_mark((hipStream_t)stream);
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
    // (no table: a result of its own, not an error the mapping knows; traversal never changes)
    if (!cam->primary_table_ok(cam->traversal))
        return set_error(RT_PRIMARY_TABLE_NONE, "no primary-ray table for this camera");
    return camera_call(cam, [&] {
        const RtCamera& C = cam->build.cam;
        if ((int64_t)capacity < (int64_t)C.width * C.height)
            throw std::invalid_argument("rt_camera_primary_table_device: capacity below width * height records");
        DevCtx& c = cam->current();
        c.ensure_device();
        c.ensure_primary_table(nullptr);
        hip_check(hipEventSynchronize(c.ptab_ev[1]), "hipEventSynchronize");
        hip_check(hipMemcpy(out, c.d_ptab, (size_t)C.width * C.height * sizeof(uint64_t), hipMemcpyDeviceToHost),
                  "hipMemcpy(primary table)");
    });
}

int rt_multi_plan_region(const rt_region* region, int32_t width, int32_t height, int32_t n_devices,
                         rt_multi_plan* plan) {
    if (!region || !plan || width < 0 || height < 0 || n_devices < 1 || n_devices > RT_MAX_DEVICES)
        return set_error(RT_ERR_INVALID, "rt_multi_plan_region: bad arguments");
    *plan = make_multi_plan(*region, width, height, n_devices);
    return RT_OK;
}

int rt_camera_render_multi(rt_camera* cam, const int32_t* devices, int32_t n_devices, const rt_region* region,
                           uint8_t* rgb, float* radiance, rt_render_stats* stats) {
    if (!region) return set_error(RT_ERR_INVALID, "null region");
    return camera_call(cam, [&] {
        unsigned long long m[ST_WORDS];
        render_multi(cam, devices, n_devices, *region, rgb != nullptr, radiance != nullptr, m,
                     [&](DevCtx& root) { copy_region_to_host(root, *region, rgb, radiance, root.stream); });
        DevCtx::stats_from_words(m, stats);
    });
}

int rt_camera_render_png_multi(rt_camera* cam, const int32_t* devices, int32_t n_devices, rt_render_stats* stats,
                               uint8_t** out, size_t* out_len) {
    if (!out || !out_len) return set_error(RT_ERR_INVALID, "null argument");
    return camera_call(cam, [&] {
        const rt_region r{0, 0, cam->build.cam.width, cam->build.cam.height};
        unsigned long long m[ST_WORDS];
        DevCtx& root = render_multi(cam, devices, n_devices, r, true, false, m, nullptr);
        DevCtx::stats_from_words(m, stats);
        png_out(root, root.stream, out, out_len);
    });
}

int rt_camera_multi_info(rt_camera* cam, rt_multi_info* info) {
    if (!info) return set_error(RT_ERR_INVALID, "null argument");
    return camera_call(cam, [&] {
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
        session_on_device(c, "rt_camera_progressive_step");
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
