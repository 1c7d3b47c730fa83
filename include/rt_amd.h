/*
 * rt_amd.h - C ABI of the MI355X path-tracing core (librt_amd.so).
 *
 * This is the drop-in boundary for df07/mcp-raytracer's hot path. The
 * reference has no FFI: its boundary is the TypeScript object model, and the
 * call site this library replaces is
 *
 *     createCameraFromSceneData(sceneData, renderOptions)   src/scenes/scenes.ts:60-104
 *     camera.renderRegion(buffer, region) -> RenderStats     src/camera.ts:388-431
 *     camera.render(buffer)                                  src/camera.ts:439-446
 *
 * called from generateImageBuffer (src/raytracer.ts:56-59) and from each render
 * worker (src/render-utils/renderWorker.ts:17-26). Scenes cross the boundary in
 * the reference's own wire format, SceneData JSON (src/scenes/sceneData.ts:8-110);
 * render options are the RenderOptions object (src/camera.ts:42-52) as JSON, plus
 * two extensions: "seed" (u32 path-RNG seed; the reference's Math.random is
 * unseeded) and "precision" ("ref" = JS-double scalars, the default; "fp32").
 *
 * Conventions: plain pointers and sizes, no torch types. Every function returns
 * 0 on success and a nonzero status on failure; rt_last_error() then holds the
 * message (thread-local), mirroring the reference's thrown Error messages.
 * Host-side functions (scene generation, camera build, info, export) run without
 * a GPU; render functions need a visible gfx950 device.
 */
#ifndef RT_AMD_H
#define RT_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_AMD_VERSION 3

enum {
    RT_OK = 0,
    RT_ERR_INVALID = 1,   /* bad arguments / scene (reference throws an Error) */
    RT_ERR_DEVICE = 2,    /* HIP error */
    RT_ERR_RENDER = 3,    /* error raised during rendering (e.g. miss without background) */
    RT_PRIMARY_TABLE_NONE = 4  /* rt_camera_primary_table: the camera has no primary-ray table */
};

enum { RT_PRECISION_REF = 0, RT_PRECISION_FP32 = 1 };
/* Closest-hit strategy. All return the reference's closest hit bit-for-bit:
 * REFERENCE visits nodes in BVHNode.hit's order with AABB.hit's per-axis test
 * (src/geometry/bvh.ts:128-146); FAST culls with a strict slab test on padded
 * boxes, near child first, and breaks t ties by leaf order; BRUTE tests every
 * primitive in leaf order (small scenes). AUTO (default) = BRUTE up to 16
 * primitives, else FAST. FAST/BRUTE fall back to REFERENCE for scenes where a
 * primitive can be hit outside its reference box (rt_camera_info.traversal
 * reports the strategy in effect). */
enum { RT_TRAVERSAL_FAST = 0, RT_TRAVERSAL_REFERENCE = 1, RT_TRAVERSAL_BRUTE = 2, RT_TRAVERSAL_AUTO = 3 };

typedef struct rt_camera rt_camera;

/* RenderRegion (src/camera.ts:54-59) */
typedef struct {
    int32_t x, y, width, height;
} rt_region;

/* RenderStats (src/render-utils/renderStats.ts:6-19). min fields are +inf when
 * no pixel / sample was rendered, exactly as the reference's Infinity seed. */
typedef struct {
    double pixels;
    double samples_total, samples_min, samples_max, samples_avg;
    double bounces_total, bounces_min, bounces_max, bounces_avg;
} rt_render_stats;

/* Camera geometry and options after createCameraFromSceneData. */
typedef struct {
    int32_t width, height, channels;
    int32_t n_objects, n_nodes, n_lights, n_materials, bvh_depth;
    int32_t samples_loop, depth, roulette, roulette_depth, mode, adaptive, precision, traversal;
    uint32_t seed;
    double samples, aperture, a_tolerance, a_batch;
} rt_camera_info;

/* Device-resident launch (benchmarks, multi-GPU). Output pointers are DEVICE
 * pointers in full-frame layout (width*height*3, row-major, RGB) and only the
 * region's tiles are written. Tiles are 8x8 pixel blocks enumerated row-major
 * over the region; this launch renders tile t iff t % tile_groups == tile_group
 * (tile_groups = 1: the whole region). `stream` is a hipStream_t (NULL = default).
 *
 * Ordering. Calls on one camera take effect in the order they were issued, whatever stream
 * each was queued on. Every entry but rt_camera_render_device and rt_camera_stats_words queues
 * on the null stream and returns with its work done. A camera's device context shares its stats
 * words, hand-out counter, record buffer and caches between all of its calls, so a call that
 * queues on a stream other than the one the context's previous call left work on (an
 * asynchronous launch, a stats-words copy) first makes its stream wait, on the device, for
 * that work: a non-blocking side stream followed by a null-stream entry needs no host sync from
 * the caller. A sequence of calls on one stream adds no wait and no host sync. Calls on
 * different cameras are independent. The caller's output buffers are the caller's to order: an
 * asynchronous launch's outputs are ready once `stream` has run. The camera keeps no stream
 * handle: a stream may be destroyed once the work queued on it has run. */
typedef struct {
    rt_region region;
    int32_t tile_group, tile_groups;
    int32_t precision;       /* -1: the camera's precision */
    int32_t traversal;       /* -1: the camera's; else an RT_TRAVERSAL_* value */
    int32_t count_work;      /* 1: instrumented build, fills work_counters; 2: section-timing diagnostic */
    uint8_t* rgb;            /* device, may be NULL */
    float* radiance;         /* device, may be NULL */
    int32_t* px_samples;     /* device W*H, may be NULL */
    int32_t* px_bounces;     /* device W*H, may be NULL */
    void* stream;
    int32_t synchronize;     /* 1: wait and fill stats / work_counters; 0: asynchronous (an adaptive-
                              * sampling render still waits on `stream` once per round: the next
                              * round's launch is sized by the pixels left) */
    int32_t packed_tiles;    /* 0: outputs in full-frame layout; 1: tile-packed slab - the pixel
                              * of lane l (= 8*row + col inside the tile) of this launch's k-th
                              * tile at index k*64 + l (rgb/radiance 3 values per index, the
                              * px_* arrays 1); unpack with rt_tiles_unpack (multi-GPU gather) */
} rt_launch;

/* Work counters of an instrumented launch (SURVEY.md §8d algorithmic bytes). */
enum {
    RT_CT_NODE = 0, RT_CT_SPHERE, RT_CT_QUAD, RT_CT_PLANE, RT_CT_MATERIAL, RT_CT_LIGHT_QUAD,
    RT_CT_LIGHT_SPHERE, RT_CT_BOUNCES, RT_CT_DIFFUSE, RT_CT_SAMPLES, RT_CT_RAYS,
    RT_CT_EXACT,       /* primitives whose exact fp64 test ran (fast/brute strategies) */
    RT_CT_EXACT_WAVE,  /* wave-level executions of those exact tests */
    RT_CT_WORDS
};
/* count_work == 2 (diagnostic): wave-cycles (s_memtime) per path-loop section,
 * summed over waves, at work_counters[RT_CT_WORDS + RT_PR_*]; for sections
 * k < RT_PR_LOOP also the active lanes summed over the wave executions of the
 * section at [RT_CT_WORDS + RT_PR_WORDS + k] and the number of those executions
 * at [RT_CT_WORDS + RT_PR_WORDS + RT_PR_LOOP + k]. */
enum {
    RT_PR_NEWPATH = 0, RT_PR_RR, RT_PR_HIT, RT_PR_MISS, RT_PR_HITREC, RT_PR_SCATTER, RT_PR_SAMPLE, RT_PR_PDF,
    RT_PR_ACC, RT_PR_TILE,
    RT_PR_NODE, RT_PR_LEAF,  /* lane counts only (no cycles): the resumable walk's node steps and leaf tests */
    RT_PR_LOOP, RT_PR_TRIPS, RT_PR_WORDS
};
/* work_counters arrays passed to rt_camera_render_device hold this many entries. */
#define RT_COUNTER_WORDS 64

int rt_version(void);
const char* rt_last_error(void);
void rt_free(void* p);

/* generateSceneData({type, options}) (src/scenes/scenes.ts:42-50). type is
 * "default" | "spheres" | "rain" | "cornell"; options_json the *SceneOptions
 * object or NULL. *out_json is malloc'ed; release with rt_free. */
int rt_generate_scene_data(const char* type, const char* options_json, char** out_json);

/* createCameraFromSceneData (src/scenes/scenes.ts:60-104). Host only. */
int rt_camera_create(const char* scene_json, const char* render_options_json, rt_camera** out);
void rt_camera_destroy(rt_camera* cam);
int rt_camera_get_info(const rt_camera* cam, rt_camera_info* info);
int rt_camera_set_precision(rt_camera* cam, int32_t precision);

/* Camera.renderRegion (src/camera.ts:388-431). rgb: caller-owned HOST buffer of
 * width*height*3 bytes (Uint8ClampedArray layout), only the region is written.
 * radiance: optional host float buffer of width*height*3 (final pixel colour).
 * stats: optional. */
int rt_camera_render_region(rt_camera* cam, const rt_region* region, uint8_t* rgb, float* radiance,
                            rt_render_stats* stats);
/* Camera.render (src/camera.ts:439-446): the whole image. */
int rt_camera_render(rt_camera* cam, uint8_t* rgb, float* radiance, rt_render_stats* stats);

/* Device-resident render (see rt_launch). stats / work_counters (RT_COUNTER_WORDS
 * u64) are filled only when launch->synchronize is 1. */
int rt_camera_render_device(rt_camera* cam, const rt_launch* launch, rt_render_stats* stats,
                            uint64_t* work_counters);

/* Host copies of the flattened scene, for tests: sizes in bytes are
 * n_nodes*32, n_objects*96, n_materials*64, n_lights*16; prim_object gets
 * n_objects int32 (leaf slot -> SceneData.objects index). Any pointer may be NULL. */
int rt_camera_export(const rt_camera* cam, void* nodes, void* prims, void* materials, void* lights,
                     int32_t* prim_object);

/* Closest hit of n rays through the device BVH (ref precision; traversal -1 =
 * the camera's). orig/dir: host float[3*n]; out: host double[10*n] =
 * {hit, t, p.xyz, n.xyz, front, prim_slot}. */
int rt_debug_world_hit(rt_camera* cam, int32_t traversal, int32_t n, const float* orig, const float* dir,
                       double* out);

/* rt_debug_world_hit through the fp32 build (precision "fp32": the fp32 intersectors, radius
 * and plane constants, and the hit record as the fp32 path kernels form it), whatever the
 * camera's precision. Same arguments and layout; t, p and n are fp32 values widened to double. */
int rt_debug_world_hit_fp32(rt_camera* cam, int32_t traversal, int32_t n, const float* orig, const float* dir,
                            double* out);

/* The device's Math.cos(phi), Math.sin(phi) (phi = 2 PI xi, the cosine-PDF angle)
 * and Math.pow(xi, 5) (Schlick) for xi = u[k] / 2^32: out = host double[3*n]. */
int rt_debug_math(int32_t n, const uint32_t* u, double* out);

/* The device's restricted-domain double square root and reciprocal beside the general
 * ones, for x = host double[n]: out = host double[4*n] = {sqrt_rn(x), sqrt(x), rcp_rn(x),
 * 1 / x} (pins rt_math.hpp sqrt_rn / rcp_rn bit for bit on their domains). */
int rt_debug_fp64(int32_t n, const double* x, double* out);

/* Pass sizing of a fixed-spp / adaptive launch (host only, no device): the units (64-slot
 * tile groups) one pass of the path kernel takes out of `units`, given each unit's slots,
 * the guided schedule's chunks per slot (items per slot), each unit's record bytes and the
 * record budget. A pass never numbers 2^31 - 2^22 or more items (the hand-out counter's
 * headroom): a budget past that gives more passes, not an error. */
int rt_debug_pass_plan(int64_t units, int64_t unit_slots, int64_t chunks_per_slot, int64_t rec_bytes_per_unit,
                       int64_t budget_bytes, int64_t* pass_units);

/* The scene blob a device context uploads (host only, no device): the bytes of every section in
 * upload order, and in `info` the byte offset of each section (all multiples of 16; off_tsph2 is
 * -1 without leaf-order sphere records), the 16-byte word counts of the two LDS-resident
 * prefixes, the pre-filter record and planar-basis counts and the total size. `out` may be NULL
 * (size query); otherwise `capacity` must hold info->bytes. */
typedef struct {
    int64_t bytes;
    int32_t off_tprims, off_tsph, off_prims, off_xrec, off_mats, off_lights, off_onbs, off_nodes, off_pre, off_tsph2;
    int32_t lds_words, lds_words2, n_pre, n_onb;
} rt_scene_blob_info;
int rt_debug_scene_blob(const rt_camera* cam, uint8_t* out, int64_t capacity, rt_scene_blob_info* info);

/* What a render of `region` (tile group `tile_group` of `tile_groups`) would launch on a device
 * of `cus` compute units and `lds_max` bytes of workgroup LDS (host only, no device): the path kernel (RT_KERNEL_*; NONE: the region is empty), the LDS
 * residency level and bytes, the traversal stack's bytes, the cached tree top, the defer / pool /
 * primary-table / 12-byte-record switches, the first pass's grid, the guided schedule and the
 * pass sizing (units of 64 slots per pass, pass count). Adaptive launches report their first
 * round. precision < 0: the camera's; count: rt_launch.count_work. `table_exists` is the one
 * field read: set it to 1 to plan as a context that has already built the table, else to 0. */
#define RT_PLAN_MAX_PHASES 8
typedef struct {
    int32_t table_exists; /* in */
    rt_region region; /* clamped to the image */
    int32_t kernel, traversal, tiles;
    int32_t lds_level, n_top;
    int64_t lds_bytes, stack_bytes;
    int32_t defer, pool, primary_ok, rec12;
    int32_t grid;
    int32_t sb_pool, n_phases, s0[RT_PLAN_MAX_PHASES], chunk[RT_PLAN_MAX_PHASES], nch[RT_PLAN_MAX_PHASES];
    int32_t refill_min, min_ready;
    int32_t samples; /* samples per slot the schedule covers (an adaptive launch: its first round) */
    int32_t passes;
    int64_t pass_units;
} rt_launch_plan;
int rt_debug_launch_plan(const rt_camera* cam, const rt_region* region, int32_t tile_group, int32_t tile_groups,
                         int32_t cus, int32_t lds_max, int32_t precision, int32_t count, rt_launch_plan* out);

/* The path RNG stream (seeded Math.random replacement), host evaluation. */
int rt_debug_rng(uint32_t seed, uint32_t pixel, uint32_t sample, int32_t n, uint32_t* out);

/* Number of visible HIP devices (0 without a GPU). */
int rt_device_count(int32_t* count);

/* Device time of the most recent rt_camera_render_device / render_region call,
 * from HIP events recorded on its stream: `path_ms` = the path-tracing
 * kernel(s), `accum_ms` = the chunked mode's in-order accumulate pass (0 for the
 * sequential kernel). Waits for that call's events. */
int rt_camera_kernel_times(rt_camera* cam, float* path_ms, float* accum_ms);

/* RenderStats words of the most recent render, queued on `stream` as a
 * device-to-device copy into `dst` (DEVICE, 8 u64): pixels, samples total,
 * samples min (~0 = none), samples max, bounces total, bounces min (~0 = none),
 * bounces max, error flags. Multi-GPU ranks ship these beside their slab so rank
 * 0 can merge them as RenderStats.merge does (src/render-utils/renderStats.ts:
 * 42-64, called from src/raytracer.ts:86-89) without a host round trip.
 * Ordered like a launch (rt_launch, Ordering): on the render's own stream the copy simply
 * follows it; on another stream it first waits for the render, and a later call on the camera
 * that queues elsewhere waits for the copy before it resets the words. */
#define RT_STATS_WORDS 8
int rt_camera_stats_words(rt_camera* cam, uint64_t* dst, void* stream);

/* Adaptive sampling of the most recent render: the rounds it ran on the chunked /
 * pool kernels (0: not adaptive, or the sequential kernel) and the samples those
 * rounds rendered - at least RenderStats.samples.total; the excess is the
 * speculation past each pixel's convergence (src/camera.ts:400-425 loop). */
int rt_camera_adaptive_info(rt_camera* cam, int32_t* rounds, uint64_t* samples_rendered);

/* Number of chunked-kernel passes of the most recent render (0 before any; the
 * sequential kernel counts as one). Passes split the per-sample record buffer. */
int rt_camera_pass_count(rt_camera* cam, int32_t* passes);

/* Path kernel of the most recent render: RT_KERNEL_NONE before any,
 * RT_KERNEL_SEQUENTIAL (wave per 8x8 tile, adaptive sampling), RT_KERNEL_CHUNKED
 * (lane work pool + in-order accumulate) or RT_KERNEL_POOL (stage-compacted
 * path pools + in-order accumulate). Diagnostics and tests; no reference
 * counterpart (the reference has one CPU loop, src/camera.ts:388-431).
 * (Values 4 and 5 named the round-3 walker-pool and wavefront kernels, removed
 * in round 4; they are not reused.) */
enum { RT_KERNEL_NONE = 0, RT_KERNEL_SEQUENTIAL = 1, RT_KERNEL_CHUNKED = 2, RT_KERNEL_POOL = 3 };
int rt_camera_last_kernel(rt_camera* cam, int32_t* kernel);

/* The primary-ray candidate table of the pool kernel. With a pinhole camera (aperture 0)
 * every primary ray of a pixel starts at the camera centre and points into the pixel's
 * footprint, so which of the scene's <= 16 brute-force primitives such a ray can hit, and
 * how far away at least, is computed once per pixel - conservatively for the whole footprint,
 * in double interval arithmetic - instead of by the fp32 pre-filter pass of every sample. The
 * pool kernel's new-path trips read the pixel's record and run only the exact tests, which
 * take the closest hit over any superset of the true candidates: results do not change.
 *
 * rt_camera_primary_table evaluates the table on the host (no device): width * height
 * records into `out` (`capacity` records), row-major by pixel. A record is
 *   bits  0-15  candidate mask by primitive slot (rt_camera_export's prims order)
 *   bits 16-19  slot of the candidate with the smallest bound
 *   bits 32-47  that candidate's bound on t, fp16
 *   bits 48-63  one fp16 bound shared by all other candidates (the minimum of theirs)
 * with bounds >= 0, rounded toward zero; 0 means "always tested". Returns
 * RT_PRIMARY_TABLE_NONE when the camera does not qualify: a defocus camera (aperture > 0),
 * more than 16 primitives, or a traversal other than brute force.
 * rt_camera_primary_table_device returns the records the current device built (building
 * them if need be): equal to the host's bit for bit.
 * rt_camera_primary_info: `available` - the camera qualifies; `used` - the most recent render
 * ran the pool kernel with the table; `built` - its device holds the table; `min_samples` -
 * samples per pixel from which a render builds it (an existing table is used at any count);
 * `build_ms` - device time of the builder kernel (waits for it; 0 when not built).
 * RT_AMD_PRIMARY_TABLE=0 in the environment keeps every launch on the pre-filter pass; =1 uses
 * the table at any sample count. */
typedef struct {
    int32_t available, used, built, min_samples;
    float build_ms;
} rt_primary_info;
int rt_camera_primary_table(const rt_camera* cam, uint64_t* out, int32_t capacity);
int rt_camera_primary_table_device(rt_camera* cam, uint64_t* out, int32_t capacity);
int rt_camera_primary_info(rt_camera* cam, rt_primary_info* info);

/* Frees the camera's device resources on every device it rendered on (scene copies, frame,
 * record and slab buffers, streams, events). A camera otherwise keeps one scene copy per device
 * (the calling thread's current device for the single-device entries, each listed device for
 * rt_camera_render_multi), so moving between devices never re-uploads; the next render
 * re-creates what it needs. */
int rt_camera_release_device(rt_camera* cam);

/* Hash of the HIP/C++ sources and compiler flags this library was built from
 * (static string, never freed). */
const char* rt_build_id(void);

/* Reassembles a region's frame from tile-packed slabs (multi-GPU gather): slabs
 * holds `tile_groups` slabs of `slab_tiles` tiles each, slab r = the packed
 * output of tile_group r (rt_launch.packed_tiles); tile k of slab r is the
 * region's tile r + k*tile_groups. Writes the region's pixels of `frame`
 * (full-frame layout, width*height pixels, `channels` values of `elem_bytes`
 * bytes each: 1 = u8 RGB, 4 = f32 radiance). DEVICE pointers; queued on
 * `stream` (a hipStream_t, NULL = default). */
int rt_tiles_unpack(const void* slabs, int32_t tile_groups, int32_t slab_tiles, const rt_region* region,
                    int32_t width, int32_t height, int32_t channels, int32_t elem_bytes, void* frame, void* stream);

/* Image file encoders for the framebuffer (the reference hands its buffer to
 * sharp, src/raytracer.ts:101-110): 8-bit RGB PNG (zlib level 0-9) or binary
 * PPM (P6). rgb: host width*height*3 bytes. *out is malloc'ed (rt_free). */
int rt_encode_png(const uint8_t* rgb, int32_t width, int32_t height, int32_t level, uint8_t** out, size_t* out_len);
int rt_encode_ppm(const uint8_t* rgb, int32_t width, int32_t height, uint8_t** out, size_t* out_len);

/* PNG of a DEVICE-resident u8 RGB frame (width*height*3), encoded on the GPU:
 * per-row PNG filter (libpng's min-sum choice), the filtered stream cut into
 * 4 KiB segments, each one deflate block with its own dynamic Huffman code
 * (run matches at distance 1 / 3) ended by a sync flush, plus its Adler-32 and
 * CRC-32; the host only combines those words and writes the chunk headers.
 * Queued on `stream` (hipStream_t, NULL = default) and waited for; *out is
 * malloc'ed (rt_free). Replaces sharp(...).png().toBuffer() (src/raytracer.ts:
 * 101-110) without the frame crossing PCIe uncompressed. */
int rt_encode_png_device(const uint8_t* d_rgb, int32_t width, int32_t height, void* stream, uint8_t** out,
                         size_t* out_len);

/* The same encoder run on the host, byte-identical to rt_encode_png_device
 * (tests: the CPU pin of the device encoder's bytes). rgb: HOST pointer. */
int rt_debug_png_host(const uint8_t* rgb, int32_t width, int32_t height, uint8_t** out, size_t* out_len);

/* generateImageBuffer's core (src/raytracer.ts:39-113): renders the whole frame
 * on the device, writes its RenderStats into *stats (may be NULL) and returns the
 * PNG encoded on the device (rt_encode_png_device). `bands` is the reference's worker
 * count (divideIntoRegions, src/raytracer.ts:185-205): neither the image nor the
 * merged stats (RenderStats.merge) depend on it, so the frame is one launch.
 * *out is malloc'ed (rt_free). */
int rt_camera_render_png(rt_camera* cam, int32_t bands, rt_render_stats* stats, uint8_t** out, size_t* out_len);

/* ---- Single-process multi-GPU (SURVEY.md §8b "rt_render_multi", §8e) ----------------------
 * The reference's parallel path is one process driving N workers over bands of one buffer
 * (src/raytracer.ts:60-90 generateImageBuffer with parallel workers, 185-205
 * divideIntoRegions; src/render-utils/renderWorker.ts:17-35 each worker's renderRegion,
 * merged with RenderStats.merge, src/render-utils/renderStats.ts:42-64). Here one call drives
 * N GPUs: the region's 8x8 tiles are dealt round-robin (tile t -> devices[t % n]); every
 * listed device renders its tiles into a tile-packed slab on its own stream (one host thread
 * per device, the camera's scene uploaded once per device and kept); the slabs - each with the
 * device's RenderStats words in a spare tile - are gathered on devices[0] over RCCL (one
 * ncclSend / ncclRecv group on single-process communicators, ncclCommInitAll, i.e. xGMI
 * between MI355X GPUs), unpacked into the full frame by rt_tiles_unpack and the stats merged
 * as RenderStats.merge does. The path RNG is keyed by (pixel, sample): the image and the
 * merged stats equal a single-device render bit for bit, for any n. A device may be listed
 * more than once (the split rehearsed on fewer GPUs); the gather then uses device-to-device
 * copies (RT_GATHER_PEER), since RCCL needs distinct devices. The environment variable
 * RT_AMD_GATHER=rccl|peer forces the transport. */
#define RT_MAX_DEVICES 16
enum { RT_GATHER_RCCL = 0, RT_GATHER_PEER = 1 };

/* The split of a region over n devices (host only). */
typedef struct {
    rt_region region;          /* the region clamped to the image */
    int32_t n_devices;
    int32_t slab_tiles;        /* tiles per slab: the largest share, ceil(tiles / n) */
    int64_t tiles;             /* 8x8 tiles of the region, row-major */
    int64_t slab_bytes_rgb;    /* u8 slab: (slab_tiles + 1) * 64 * 3 (the spare tile carries the stats words) */
    int64_t slab_bytes_radiance; /* f32 slab: slab_tiles * 64 * 3 * 4 */
    int64_t stats_offset;      /* byte offset of the 8 stats words in a u8 slab */
    int32_t group_tiles[RT_MAX_DEVICES]; /* tiles device entry g renders */
} rt_multi_plan;
int rt_multi_plan_region(const rt_region* region, int32_t width, int32_t height, int32_t n_devices,
                         rt_multi_plan* plan);

/* Camera.renderRegion over n_devices GPUs (see above). rgb / radiance: caller-owned HOST
 * buffers in full-frame layout as rt_camera_render_region (only the region is written; either
 * may be NULL); stats: the merged RenderStats (may be NULL). */
int rt_camera_render_multi(rt_camera* cam, const int32_t* devices, int32_t n_devices, const rt_region* region,
                           uint8_t* rgb, float* radiance, rt_render_stats* stats);

/* generateImageBuffer over n_devices GPUs: the whole frame as rt_camera_render_multi, then its
 * PNG encoded on devices[0] (rt_encode_png_device). *out is malloc'ed (rt_free). */
int rt_camera_render_png_multi(rt_camera* cam, const int32_t* devices, int32_t n_devices, rt_render_stats* stats,
                               uint8_t** out, size_t* out_len);

/* The most recent rt_camera_render_multi / _png_multi of this camera (n_devices = 0 when a
 * single-device render came after it): devices, transport, plan, each device's path-kernel and
 * accumulate time (HIP events on its stream) and gather_ms = devices[0]'s time from the end of
 * its own render to the assembled frame (waiting for the slowest device, the gather, the unpack
 * and the stats words' copy). Waits for those events. */
typedef struct {
    int32_t n_devices;
    int32_t transport;         /* RT_GATHER_* */
    int32_t devices[RT_MAX_DEVICES];
    float path_ms[RT_MAX_DEVICES];
    float accum_ms[RT_MAX_DEVICES];
    float gather_ms;
    rt_multi_plan plan;
} rt_multi_info;
int rt_camera_multi_info(rt_camera* cam, rt_multi_info* info);

/* ---- Progressive rendering: resumable sample steps with a live preview ---------------------
 * A session on a camera renders its region a few samples at a time. The path RNG is keyed by
 * (pixel, sample) and PixelStats accumulates in sample order (src/render-utils/renderStats.ts:
 * 76-88), so the frame a session reaches does not depend on how the steps were cut. A session
 * is single-device (the calling thread's current device, as rt_camera_render_region) and owns
 * its state and frame buffers: one-shot renders on the same camera between two steps neither
 * disturb it nor are disturbed. No reference counterpart: the reference renders a frame in one
 * call (src/camera.ts:388-431).
 *
 * A step renders the next min(n_samples, samples - samples_done) samples of every pixel still
 * sampling and adds them to the pixel's running PixelStats in sample order, with the
 * reference's convergence check (pixelConverged, src/camera.ts:348-368,406) after every sample;
 * samples rendered past a pixel's convergence are dropped. A pixel is finished when it has
 * converged or holds the camera's `samples`, and is never visited again; this holds for adaptive
 * and fixed-spp cameras alike. The check after a step's last sample is made when the next step
 * begins, so `active_pixels` counts the pixels that hold samples_done samples and have not
 * reached the camera's `samples`.
 *
 * After every step the outputs describe ALL pixels of the region: finished pixels exactly as a
 * one-shot render writes them, unfinished ones finalColor / writeColorToBuffer of their running
 * PixelStats (the preview); stats is RenderStats.addPixel over all of them, each with the
 * samples and bounces it has so far.
 *
 * Contract. With s = samples_done after a step, u8, radiance, px_samples, px_bounces and stats
 * are bit-identical to rt_camera_render_region of a camera that differs only in `samples: s`,
 * for mode default and bounces and s >= 2. (s = 1: a camera with samples > 1 jitters its first
 * sample and a `samples: 1` camera does not, src/camera.ts:184. mode samples divides by the
 * camera's own `samples`, src/camera.ts:333: its preview is min(n / samples, 1) of the session's
 * camera.) When samples_done == samples the outputs equal the one-shot render of the same
 * camera in every mode and both precisions.
 *
 * n_samples <= 0, a step / info / save without an open session and a region that is empty
 * after clamping return RT_ERR_INVALID. A step on a finished session renders nothing and
 * returns the final frame and stats again. Render errors (no background, emission stack)
 * surface as in one-shot renders, from the samples that were kept only.
 * rt_camera_release_device and rt_camera_destroy end the session. */
typedef struct {
    rt_region region;         /* the session's region, clamped to the image */
    int32_t width, height;    /* the camera's image */
    int32_t samples_done;     /* samples every unfinished pixel holds */
    int32_t samples;          /* the camera's sample loop count (rt_camera_info.samples_loop) */
    int32_t steps;            /* steps that rendered something */
    int32_t done;             /* 1: no pixel is still sampling */
    int32_t precision;        /* RT_PRECISION_* the session renders in */
    uint32_t seed;
    int64_t active_pixels;    /* pixels still sampling */
    uint64_t state_bytes;     /* per-pixel state: the payload of a checkpoint blob */
    char build_id[24];        /* rt_build_id of the library that holds / wrote the state */
} rt_progressive_info;

/* Opens a session over `region` (NULL: the whole image) at zero samples; an open one is dropped. */
int rt_camera_progressive_begin(rt_camera* cam, const rt_region* region);
/* One step (above). rgb / radiance: HOST buffers in full-frame layout as rt_camera_render_region,
 * px_samples / px_bounces: HOST width*height int32; only the region is written; any may be NULL. */
int rt_camera_progressive_step(rt_camera* cam, int32_t n_samples, uint8_t* rgb, float* radiance, int32_t* px_samples,
                               int32_t* px_bounces, rt_render_stats* stats);
int rt_camera_progressive_info(rt_camera* cam, rt_progressive_info* info);
/* Checkpoint of the open session: a fixed header (magic, format version, rt_build_id, image size,
 * region, precision, seed, samples, samples_done, steps, active pixels, a fingerprint of the
 * flattened scene and the resolved camera options, payload length, checksums) and the per-pixel
 * state (48 bytes per pixel slot: colour sum, n, finished flag, illuminance sums, bounce sum /
 * min / max). The frame, the stats and the active list are rebuilt from the state, so the blob
 * holds no frame. *blob is malloc'ed (rt_free). */
int rt_camera_progressive_save(rt_camera* cam, uint8_t** blob, size_t* len);
/* Opens a session from a blob (an open one is dropped on success). Refused with RT_ERR_INVALID
 * and a message naming the first mismatch when the blob is truncated or corrupt, or when build
 * id, image size, precision, seed, samples or the scene fingerprint differ from the camera's.
 * The steps that follow give the frames the uninterrupted session would have given, bit for bit
 * - in another camera object or another process. */
int rt_camera_progressive_restore(rt_camera* cam, const uint8_t* blob, size_t len);
/* Parses and validates a blob's header and checksums (host only, no device). */
int rt_progressive_blob_info(const uint8_t* blob, size_t len, rt_progressive_info* info);
int rt_camera_progressive_end(rt_camera* cam);

/* ---- Guide buffers and the guided edge-avoiding a-trous filter -------------------------------
 * No reference counterpart (the reference never filters a frame). Opt-in: no other call changes.
 *
 * Guides. One deterministic primary ray per pixel of the region: origin = the camera's centre,
 * direction = pixel00 + du i + dv j - centre in fp32 - Camera.getRay of a `samples: 1`,
 * `aperture: 0` camera (src/camera.ts:176-210): no jitter, no defocus sample (a camera with an
 * aperture still gets this pinhole ray), no RNG. Always ref precision, the camera's own
 * traversal, interval (0.001, inf). normal (float[3]: facing the ray), position (float[3]: the
 * hit point), distance (float: sqrtf((dx dx + dy dy) + dz dz) of position - centre in fp32) and
 * object (int32: index in SceneData.objects) equal the reference's world.hit of that ray bit
 * for bit; a miss gives normal = position = 0, distance = 0, object = -1. glass and mirrors
 * report their own surface, not what is seen through them.
 *
 * Filter. `levels` passes of a 5x5 B3-spline a-trous kernel at steps 1, 2, 4, ..., each tap
 * weighted by max(0, n.n')^32, by the tap's distance from the centre pixel's tangent plane
 * relative to sigma_plane * distance, and by the colour difference relative to sigma_color
 * (halved per level); hit and miss pixels never mix, taps outside the region and non-finite
 * taps are skipped, a non-finite pixel is copied through. Built from fp32 add, multiply, IEEE
 * divide and square root in a fixed order: the result equals the NumPy restatement
 * tests/denoise_ref.py (the normative definition) in every bit. rgb_out is the frame's own
 * u8 of the filtered colour: floor(255.999 sqrt(c)) clamped to 0..255, non-positive / NaN -> 0.
 *
 * All buffers are HOST buffers in full-frame layout (normal / position / radiance width*height*3
 * floats, distance / object width*height, rgb width*height*3 bytes); only the region (NULL: the
 * whole image) is read and written; outputs may be NULL, and radiance_out may be radiance.
 * Negative or non-finite parameters, levels > 8 and a region that is empty after clamping return
 * RT_ERR_INVALID. rt_camera_release_device frees every device buffer of these calls. */
typedef struct { int32_t levels; float sigma_color, sigma_plane; } rt_denoise_options;   /* NULL or a zero field = default (4, 0.5, 0.01) */
int rt_camera_render_guides(rt_camera* cam, const rt_region* region, float* normal, float* position, float* distance,
                            int32_t* object);
/* explicit guides, no camera (the calling thread's current device) */
int rt_denoise(int32_t width, int32_t height, const rt_region* region, const rt_denoise_options* options,
               const float* radiance, const float* normal, const float* position, const float* distance,
               const int32_t* object, float* radiance_out, uint8_t* rgb_out);
/* guides computed on the device (they never reach the host) */
int rt_camera_denoise(rt_camera* cam, const rt_region* region, const rt_denoise_options* options, const float* radiance,
                      float* radiance_out, uint8_t* rgb_out);
/* The open progressive session's device frame as it stands after the last step, filtered over
 * the session's region: nothing is uploaded. The region's guides are computed on first use and
 * kept until the session ends. The session's state, frame and stats are not touched, so its
 * later steps are those of a session that never called this. RT_ERR_INVALID without an open
 * session and for a camera in mode bounces / samples (those frames are not radiance). */
int rt_camera_progressive_denoise(rt_camera* cam, const rt_denoise_options* options, uint8_t* rgb, float* radiance);
/* Device time of the camera's last rt_camera_denoise / rt_camera_progressive_denoise from HIP
 * events: the guide pass (0 when a session reused its guides), each level (level_ms: 8 floats)
 * and the whole span guide pass .. filtered frame (host copies excluded). Waits for the events. */
int rt_camera_denoise_times(rt_camera* cam, int32_t* levels, float* guide_ms, float* level_ms, float* total_ms);

/* ---- Variance map and the variance-guided filter ---------------------------------------------
 * Opt-in like the block above: no other call changes.
 *
 * Variance map. Per pixel of a progressive session's region, the variance of the pixel mean's
 * illuminance (0.299 r + 0.587 g + 0.114 b, Color.illuminance) from the pixel's own running sums
 * in fp64, in the reference's expression order (src/camera.ts:356-357), for n >= 2:
 *     m2 = sumIll2 - (sumIll * sumIll) / n;   v = (m2 / (n - 1)) / n;   (float)(v > 0 ? v : 0)
 * (NaN and negatives -> 0, n < 2 -> 0). Every pixel uses its own n: an adaptive pixel that
 * retired early keeps the variance it retired with. `variance` is a HOST buffer in full-frame
 * layout (width*height floats); only the region is written. rt_progressive_blob_variance
 * evaluates the same formula on a checkpoint blob's payload on the host (no device; the blob is
 * validated as rt_progressive_blob_info does; `variance` holds the blob's width*height floats).
 * rt_camera_progressive_variance returns RT_ERR_INVALID without an open session, for a camera in
 * mode bounces / samples and while samples_done < 2.
 *
 * Filter. The a-trous filter above with the colour edge-stop replaced and a variance channel
 * carried along: `levels` passes at steps 1, 2, 4, ...; in each, the centre pixel's variance is
 * pre-blurred (3x3, weights (1/4, 1/2, 1/4)^2 at unit spacing over the in-region pixels,
 * normalised) to gv, k = 1 / (sigma_variance^2 gv + 1e-10), and a tap weighs
 *     w = h max(0, n.n')^32 / ((1 + x^2) (1 + d^2 k)),   d = illuminance(tap) - illuminance(centre)
 * with the plane term x, the hit / miss rule and the skipped taps of the filter above; then
 * c' = sum(w c) / sum(w) and variance' = sum(w^2 variance) / sum(w)^2. The input variance is
 * sanitised once (not (v >= 0 and finite) -> 0); a non-finite pixel keeps its colour and its
 * variance. The result - colour and variance - equals the NumPy restatement
 * tests/denoise_var_ref.py (the normative definition) in every bit. Buffers and errors as above
 * (HOST buffers, full-frame layout, only the region read and written, outputs may be NULL);
 * variance_out may be variance. rt_camera_progressive_denoise_variance filters the open session's
 * device frame with the variance of its state and its kept guides, touches neither state nor
 * frame, and also returns RT_ERR_INVALID while samples_done < 2. rt_camera_denoise_times reports
 * these calls too; for the session call its guide_ms span includes the variance pass. */
typedef struct { int32_t levels; float sigma_variance, sigma_plane; } rt_denoise_var_options;   /* NULL or a zero field = default (4, 2.0, 0.01) */
int rt_progressive_blob_variance(const uint8_t* blob, size_t len, float* variance);
int rt_camera_progressive_variance(rt_camera* cam, float* variance);
int rt_denoise_variance(int32_t width, int32_t height, const rt_region* region, const rt_denoise_var_options* options,
                        const float* radiance, const float* variance, const float* normal, const float* position,
                        const float* distance, const int32_t* object, float* radiance_out, float* variance_out,
                        uint8_t* rgb_out);
int rt_camera_denoise_variance(rt_camera* cam, const rt_region* region, const rt_denoise_var_options* options,
                               const float* radiance, const float* variance, float* radiance_out, float* variance_out,
                               uint8_t* rgb_out);
int rt_camera_progressive_denoise_variance(rt_camera* cam, const rt_denoise_var_options* options, uint8_t* rgb,
                                           float* radiance, float* variance_out);

/* ---- Guides through mirrors and glass ----------------------------------------------------------
 * Opt-in like the blocks above: no other call changes. The first-hit guides report a mirror's or
 * a glass ball's own surface; these follow the pixel's specular chain to the first surface that
 * is not specular, so the filter sees the edges of what is reflected or seen through.
 * tests/guide_walk_ref.py is the normative definition; in words:
 *
 * A deterministic walk per pixel, no RNG, always ref precision, through the camera's traversal.
 * State: a ray, an fp32 dist = 0, k = 0. Segment 0 is the first-hit guides' pinhole ray. Loop:
 * take the ray's closest hit on (0.001, inf). A miss ends the walk: with k == 0 the pixel is a
 * miss (zeros, object -1, end code 0), else the guide is the specular surface the chain left
 * through last (end code 2). On a hit, position, the normal facing the ray and the face are the
 * first-hit guides'; dist += sqrtf((qx qx + qy qy) + qz qz) of q = position - origin in fp32, in
 * segment order; cur = (normal, position, dist, object). The hit's material is then resolved as
 * Material.scatter resolves it, with a policy in place of every random draw:
 *   lambert, light, no material  terminal
 *   metal     f = reflect(unit(d), n); terminal when fuzz > max_fuzz or f.n <= 0; else continue
 *             along f (the fuzz term is dropped)
 *   glass     the dielectric's arithmetic without its draw: refract whenever ratio sinT <= 1,
 *             else reflect (Schlick's reflectance is ignored); always continues
 *   mixed     the child `diff` when its weight >= 0.5, else `spec`
 *   layered   the outer dielectric by the glass rule; a reflection continues; a refraction
 *             becomes the incoming direction of the inner material at the same hit
 * A terminal material ends the walk with cur (end code 1); k == max_bounces ends it with cur
 * (end code 3); otherwise the walk continues from the position along the new direction, k += 1.
 * Outputs: the four guide arrays of rt_camera_render_guides, and chain (int32) = k | end << 8.
 * A scene without specular materials gives the first-hit guides in every bit, chain = 1 << 8 on
 * every hit.
 *
 * rt_camera_render_guides_ex: any output may be NULL; options NULL = rt_guide_options_default
 * (first hit, 8, 0). Mode RT_GUIDES_FIRST_HIT is rt_camera_render_guides, chain = hit ? 1 << 8 : 0.
 * rt_camera_set_denoise_guides selects the guides the four camera filter calls compute
 * (rt_camera_denoise, rt_camera_denoise_variance, rt_camera_progressive_denoise,
 * rt_camera_progressive_denoise_variance); NULL, or never calling it, means first hit. A session
 * keeps its specular guides beside its first-hit ones, recomputed when the options change;
 * reprojection, accumulation and focus always use first-hit guides. rt_camera_denoise_times'
 * guide_ms covers whichever pass ran. RT_ERR_INVALID, decided before any device call: an unknown
 * mode, max_bounces outside 1..64, a negative or non-finite max_fuzz.
 * Limits: one deterministic branch per interface (no Schlick split), fuzzy metals above max_fuzz
 * are terminal, a defocused camera's blur is not in the guides, and rt_reproject and
 * rt_camera_progressive_accumulate still stop at specular surfaces (rt_reproject_specular and
 * rt_camera_progressive_accumulate_specular with their sibling calls, below, follow the chains on
 * request). Not in the N-API addon or the multi-GPU render. */
enum { RT_GUIDES_FIRST_HIT = 0, RT_GUIDES_SPECULAR = 1 };
typedef struct { int32_t mode; int32_t max_bounces; float max_fuzz; } rt_guide_options;
void rt_guide_options_default(rt_guide_options* options);
int rt_camera_render_guides_ex(rt_camera* cam, const rt_region* region, const rt_guide_options* options, float* normal,
                               float* position, float* distance, int32_t* object, int32_t* chain);
int rt_camera_set_denoise_guides(rt_camera* cam, const rt_guide_options* options);
int rt_camera_get_denoise_guides(rt_camera* cam, rt_guide_options* options);

/* ---- Reprojection of a previous view's frame into a new camera view --------------------------
 * No reference counterpart (the reference renders every frame from scratch). Opt-in like the two
 * blocks above: no other call changes.
 *
 * A service re-renders one scene from a moved camera. On Lambertian and emissive surfaces the
 * radiance leaving a point does not depend on the viewer, so the previous view's converged
 * frame is a history for the new view's first frames. Per pixel of the new region, with guides
 * n, P, D (distance), o (object): no history when o < 0, o >= n_objects, reusable[o] == 0 or P
 * is not finite. Otherwise P is projected into the previous view V = {center c, pixel00 p, du,
 * dv, width, height} (the vectors the guide pass builds its rays from), in fp32:
 *     a = p - c, w = cross(du, dv), aw = a.w, iu = 1 / du.du, iv = 1 / dv.dv      (per view)
 *     d = P - c, s = aw / d.w, q = d s - a, fi = (q.du) iu, fj = (q.dv) iv
 * no history unless s is finite and > 0, and fi, fj are finite with -1 < fi < width,
 * -1 < fj < height. The four bilinear taps at (floor(fi) + dx, floor(fj) + dy), dy outer, weigh
 * b = (dx ? ax : 1 - ax) (dy ? ay : 1 - ay); a tap counts iff it lies inside the previous image
 * and prev_region, shows the same object, has finite radiance, n.n' >= normal_min and
 * |n.(P' - P)| <= sigma_plane D. ws = sum b, acc = sum b c' over the taps that count;
 * weight = ws if ws >= min_weight else 0; history = acc / ws where weight > 0, else 0.
 * With a fresh `radiance` c and m = the pixel's own sample count (px_samples, or the scalar
 * `samples` when px_samples is NULL) as a float, Nh = history_samples:
 *     weight > 0, c finite, m > 0:  out = (history Nh + c m) / (Nh + m)
 *     weight > 0 otherwise:         out = history
 *     weight == 0:                  out = c
 * and rgb_out is the frame's own u8 of out. Built from fp32 add, subtract, multiply, IEEE divide
 * and floor in a fixed order, no fused multiply-add, dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z:
 * the result equals the NumPy restatement tests/reproject_ref.py (the normative definition) in
 * every bit.
 *
 * Limits. The guides are pinhole first hits: view-dependent surfaces (metal, glass, mixed,
 * layered: reusable = 0) and misses get no history (what a mirror or glass shows can get one
 * through rt_reproject_specular, below), and a defocus camera's blur is not in them.
 * The lighting must not have changed between the views. The history is weighted by the constant
 * history_samples, whatever the previous frame's own sample counts.
 *
 * Buffers as the denoise block: HOST buffers in full-frame layout of their own image (the new
 * frame's width x height, the previous view's width x height), only `region` / `prev_region`
 * (NULL: the whole image) read and written, outputs may be NULL (radiance_out / rgb_out need
 * `radiance`). history_out: width*height*3 floats, weight_out: width*height floats.
 * RT_ERR_INVALID for negative or non-finite options, negative `samples`, a region that is empty
 * after clamping and a missing required pointer - before any device call.
 * rt_camera_release_device frees every device buffer of the camera calls. */
typedef struct { float center[3], pixel00[3], du[3], dv[3]; int32_t width, height; } rt_view;
typedef struct { float normal_min, sigma_plane, min_weight, history_samples; } rt_reproject_options;   /* NULL or a zero field = default (0.9, 0.01, 0.25, 32) */
/* The camera's view: the RtCamera vectors in fp32 (host only). */
int rt_camera_get_view(const rt_camera* cam, rt_view* view);
/* reusable[o] = 1 iff SceneData.objects[o]'s resolved material (ids followed) is lambert or
 * light; out holds rt_camera_info.n_objects bytes (capacity below that: RT_ERR_INVALID). Host only. */
int rt_camera_reusable_objects(const rt_camera* cam, uint8_t* out, int32_t capacity);
/* explicit buffers, no camera (the calling thread's current device) */
int rt_reproject(int32_t width, int32_t height, const rt_region* region, const float* normal, const float* position,
                 const float* distance, const int32_t* object, const rt_view* prev_view, const rt_region* prev_region,
                 const float* prev_radiance, const float* prev_normal, const float* prev_position,
                 const float* prev_distance, const int32_t* prev_object, const uint8_t* reusable, int32_t n_objects,
                 const rt_reproject_options* options, const float* radiance, const int32_t* px_samples, int32_t samples,
                 float* history_out, float* weight_out, float* radiance_out, uint8_t* rgb_out);
/* Both cameras' guides are computed on the calling thread's device and never reach the host;
 * the view and the reusable table are prev_cam's and cam's own. The two cameras must hold the
 * same scene (flattened nodes, primitives, materials, lights and the object map), else
 * RT_ERR_INVALID "reproject: the cameras hold different scenes", decided on the host. */
int rt_camera_reproject(rt_camera* cam, const rt_region* region, rt_camera* prev_cam, const rt_region* prev_region,
                        const rt_reproject_options* options, const float* prev_radiance, const float* radiance,
                        const int32_t* px_samples, int32_t samples, float* history_out, float* weight_out,
                        float* radiance_out, uint8_t* rgb_out);
/* The open progressive session's device frame blended with the history over the session's
 * region, each pixel with its own px_samples: nothing is uploaded but the previous radiance.
 * The session's state, frame and stats are not touched (as rt_camera_progressive_denoise).
 * RT_ERR_INVALID without an open session and in mode bounces / samples. */
int rt_camera_progressive_reproject(rt_camera* cam, rt_camera* prev_cam, const rt_region* prev_region,
                                    const rt_reproject_options* options, const float* prev_radiance, uint8_t* rgb,
                                    float* radiance, float* weight_out);
/* Device time of the camera's last rt_camera_reproject / rt_camera_progressive_reproject from
 * HIP events: the guide passes (both views'; a session reuses its own), the gather kernel, and
 * the whole span guide passes .. unpacked outputs (host copies excluded). Waits for the events. */
int rt_camera_reproject_times(rt_camera* cam, float* guide_ms, float* reproject_ms, float* total_ms);

/* ---- Reprojection through mirrors and glass (specular chains) ----------------------------------
 * Opt-in like the blocks above: no other call changes. The radiance a pixel receives along a
 * chain of perfect mirrors that ends on a Lambertian or emissive surface does not depend on the
 * viewer, and through a planar mirror the previous view sees that surface point at the same
 * virtual location: the point at the chain's summed path length along the primary ray.
 * tests/specular_reproject_ref.py is the normative definition; in words, with the rules of the
 * reprojection block (fp32, no fused multiply-add, its dot, projection, taps and blend):
 *
 * Per pixel of the new region: the first-hit guides n1, P1, D1, o1; the guides through the chain
 * n, P, Ds, o and the chain word ch of ONE rt_guide_options (mode RT_GUIDES_SPECULAR), k = ch & 0xff,
 * e = (ch >> 8) & 0xff; the new view's centre cn; the previous view V with the constants above and
 * pix2 = du.du / a.a; the previous view's first-hit planes, chain planes and chain words, walked
 * with the same options; two byte tables per object, reusable (above) and through.
 *   k == 0  the reprojection block verbatim on n1, P1, D1, o1 against the previous first-hit
 *           planes; kind = 1 where weight > 0.
 *   k >= 1  no history unless e == 1, 0 <= o < n_objects and reusable[o], 0 <= o1 < n_objects and
 *           through[o1], P and P1 finite, Ds finite, D1 finite and > 0. Then r = Ds / D1,
 *           X = cn + (P1 - cn) r (subtract, multiply, add), and X is projected in place of P with
 *           the same validity tests, taps and weights. A tap counts iff it lies inside the previous
 *           image and prev_region, its chain word equals ch, its first-hit object equals o1, its
 *           chain object equals o, its radiance is finite, n.n' >= normal_min,
 *           |n.(P' - P)| <= sigma_plane Ds and q.q <= (pp2 Ds) Ds with q = P' - P,
 *           pp2 = (point_pixels point_pixels) pix2 - n', P' the tap's chain guides. ws, acc,
 *           min_weight, history and the blend as above; kind = 2 where weight > 0.
 * The point check asks that the previous pixel showed the same surface point, not only the same
 * plane, within point_pixels footprints of a previous pixel at the chain's length.
 * through[o] = 1 iff object o's resolved top-level material class is in a mask: 1 a metal of fuzz
 * <= max_fuzz, 2 glass, 4 mixed, 8 layered (default 15: everything the walk follows). Only the
 * chain's first object is checked; longer chains are tied down by the equal chain word, the equal
 * first and last objects and the point check.
 *
 * Limits. A curved mirror's image does not lie at the summed length, so it gets little or no
 * history; grazing reflections are under-covered by the isotropic point check; through glass the
 * Schlick split varies with the angle, so the history is an approximation; chains that leave the
 * scene (end code 2) or reach max_bounces get no history; the lighting must be unchanged.
 *
 * Buffers and errors as the reprojection block; kind_out: width*height uint8 (0 none, 1 first hit,
 * 2 chain). Also RT_ERR_INVALID before any device call: guide options rt_camera_render_guides_ex
 * would refuse, mode RT_GUIDES_FIRST_HIT, a negative or non-finite point_pixels, a through mask
 * outside 0..15. rt_camera_release_device frees every device buffer of the camera calls, and
 * rt_camera_reproject_times covers them (guide_ms: all four guide passes; a session reuses its own). */
typedef struct { rt_reproject_options base; float point_pixels; int32_t through; } rt_specular_reproject_options;   /* NULL or a zero field = default (base's, 4, 15) */
/* {{0.9, 0.01, 0.25, 32}, 4, 15}. Host only. */
void rt_specular_reproject_options_default(rt_specular_reproject_options* options);
/* through[o] for the mask and max_fuzz (from the build's material table, ids followed); out holds
 * rt_camera_info.n_objects bytes (capacity below that: RT_ERR_INVALID). Host only. */
int rt_camera_through_objects(const rt_camera* cam, int32_t mask, float max_fuzz, uint8_t* out, int32_t capacity);
/* explicit buffers, no camera (the calling thread's current device); view: the new view */
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
                          uint8_t* kind_out);
/* Both cameras' two guide passes run on the calling thread's device and never reach the host;
 * guide_options NULL = {RT_GUIDES_SPECULAR, 8, 0}; the through table is cam's for options->through
 * and guide_options->max_fuzz. The cameras must hold the same scene, as rt_camera_reproject. */
int rt_camera_reproject_specular(rt_camera* cam, const rt_region* region, rt_camera* prev_cam,
                                 const rt_region* prev_region, const rt_guide_options* guide_options,
                                 const rt_specular_reproject_options* options, const float* prev_radiance,
                                 const float* radiance, const int32_t* px_samples, int32_t samples, float* history_out,
                                 float* weight_out, float* radiance_out, uint8_t* rgb_out, uint8_t* kind_out);
/* rt_camera_progressive_reproject through the chains: the session's kept first-hit and chain
 * guides serve (the chain plane is kept beside the latter); its state, frame, stats and
 * checkpoint bytes are not touched. */
int rt_camera_progressive_reproject_specular(rt_camera* cam, rt_camera* prev_cam, const rt_region* prev_region,
                                             const rt_guide_options* guide_options,
                                             const rt_specular_reproject_options* options, const float* prev_radiance,
                                             uint8_t* rgb, float* radiance, float* weight_out, uint8_t* kind_out);

/* ---- Accumulation across views: per-pixel history length and variance -------------------------
 * A view history follows a camera along a path. Per pixel it keeps the accumulated radiance c',
 * the effective number of samples behind it (the history length L') and the variance V' of the
 * accumulated mean's illuminance - the meaning of rt_camera_progressive_variance, so the
 * variance-guided filter consumes it unchanged. One call takes a new view's fresh frame c, its
 * per-pixel sample counts m (as a float) and variance v, and a history (view, region, guides, c',
 * L', V'); v and V' are sanitised as the variance filter does (not (>= 0 and finite) -> 0).
 *   1. Projection, validity and the four taps exactly as the reprojection block above, with one
 *      more tap condition: L' is finite and > 0 (a pixel that never held a sample is not history).
 *   2. ws = sum b, acc = sum b c', av = sum b V', al = sum b L' over the taps that count (multiply,
 *      then add); weight = ws if ws >= min_weight else 0; where weight > 0: h = acc / ws,
 *      Vh = av / ws, Lh = al / ws, N = min(Lh, max_history).
 *   3. weight > 0, c finite, m > 0:  den = N + m; out = (h N + c m) / den; g = N / den; a = m / den;
 *                                    Vout = (g g) Vh + (a a) v; Lout = den
 *      weight > 0 otherwise:         out = h, Vout = Vh, Lout = N
 *      weight == 0:                  out = c, Vout = v, Lout = m if c is finite else 0
 *   4. filter_levels > 0: the returned radiance, rgb and variance_out are the variance-guided
 *      filter (rt_denoise_variance: levels = filter_levels, sigma_variance, sigma_plane) of out and
 *      Vout over the region with the new view's guides. length_out / weight_out are never
 *      filtered, and the history keeps the unfiltered out, Vout and Lout.
 *   5. Commit: out, Vout, Lout and the new view, guides and region become the history.
 * An empty history has weight 0 everywhere: the first call commits the fresh frame itself. Built
 * from fp32 add, subtract, multiply, IEEE divide, floor and min in a fixed order, no fused
 * multiply-add: the result equals the NumPy restatement tests/temporal_ref.py (the normative
 * definition) in every bit.
 *
 * THE CALLER MUST VARY THE SEED PER VIEW. The path RNG is keyed by (pixel, sample, seed): views
 * that share a seed have correlated noise, and a static camera with the same seed re-renders the
 * very same samples - nothing is gained and the carried variance is wrong.
 *
 * Limits as the reprojection block (lambert and light surfaces only, unchanged lighting; what a
 * mirror or glass shows gets a history through rt_camera_progressive_accumulate_specular, below).
 * max_history (default 256) bounds the weight of the past; it is a design choice, not tuned.
 *
 * RT_ERR_INVALID, decided before any device call: negative or non-finite options or
 * filter_levels outside 0..8; no open session, mode bounces / samples, samples_done < 2; a
 * missing pointer of the explicit entry; a region that is empty after clamping; "temporal: the
 * history holds a different scene" (the flattened nodes, primitives, materials, lights and object
 * map are hashed at the first commit); a history committed on another device. A history of
 * another image size is allowed. */
typedef struct rt_history rt_history;
typedef struct { float normal_min, sigma_plane, min_weight, max_history; int32_t filter_levels; float sigma_variance; } rt_temporal_options;   /* NULL or a zero field = default (0.9, 0.01, 0.25, 256, no filter, 2.0) */
typedef struct { int32_t width, height; rt_region region; int32_t views, device; uint64_t scene_hash, bytes; rt_view view; } rt_history_info;
/* Host only: an empty history (views = 0, device -1). The history owns its device buffers - two
 * sets of colour + length, variance and guides, and the reusable table - on the device of its
 * first commit; the cameras and sessions it was fed from may be destroyed, and
 * rt_camera_release_device does not free it. rt_history_destroy does. */
int rt_history_create(rt_history** out);
void rt_history_destroy(rt_history* h);
/* Image size, region and view of the last committed view, the number of committed views, the
 * device, the scene's hash and the device bytes held. Host only. */
int rt_history_get_info(const rt_history* h, rt_history_info* info);
/* The history's radiance (width*height*3 floats), variance and length (width*height floats) to
 * HOST buffers in the history's own full-frame layout; only its region is written; any may be
 * NULL. RT_ERR_INVALID while the history is empty. */
int rt_history_read(rt_history* h, float* radiance, float* variance, float* length);
/* The open progressive session's device frame, px_samples, state variance and kept guides
 * accumulated onto the history over the session's region: only the caller's outputs (HOST,
 * full-frame layout of the camera's image, only the region written, any may be NULL) cross the
 * bus. commit = 0 leaves the history as it was; the session (state, frame, stats, the bytes of
 * rt_camera_progressive_save) is never touched. */
int rt_camera_progressive_accumulate(rt_camera* cam, rt_history* h, const rt_temporal_options* options, int32_t commit,
                                     uint8_t* rgb, float* radiance, float* variance_out, float* length_out,
                                     float* weight_out);
/* Explicit HOST buffers, no camera and no history object (the calling thread's current device),
 * as rt_reproject: the new view's guides, fresh radiance, px_samples (or the scalar `samples` when
 * NULL) and variance; the previous view, its region, guides, radiance, variance and length. Every
 * input pointer but region, prev_region, px_samples and options is required. */
int rt_temporal_accumulate(int32_t width, int32_t height, const rt_region* region, const float* normal,
                           const float* position, const float* distance, const int32_t* object, const float* radiance,
                           const int32_t* px_samples, int32_t samples, const float* variance, const rt_view* prev_view,
                           const rt_region* prev_region, const float* prev_normal, const float* prev_position,
                           const float* prev_distance, const int32_t* prev_object, const float* prev_radiance,
                           const float* prev_variance, const float* prev_length, const uint8_t* reusable,
                           int32_t n_objects, const rt_temporal_options* options, float* radiance_out,
                           float* variance_out, float* length_out, float* weight_out, uint8_t* rgb_out);
/* Device time of the history's last rt_camera_progressive_accumulate from HIP events: the guide
 * and variance passes (a session computes its guides once), the gather kernel, the filter (0
 * without one), and the whole span up to the unpacked outputs and the commit's guide copy (host
 * copies excluded). Waits for the events. */
int rt_history_times(rt_history* h, float* guide_ms, float* gather_ms, float* filter_ms, float* total_ms);

/* ---- Accumulation across views through mirrors and glass (specular chains) ----------------------
 * Opt-in like the blocks above: no other call changes, and a history that never sees a call of this
 * block holds the device bytes it held before. The view history above stops at every specular
 * surface (reusable[o] == 0: weight 0, the length restarts at the fresh count on every view). This
 * block carries it through the chains of the specular-reprojection block: the history keeps, beside
 * the first-hit planes of the view it was committed from, that view's chain planes, chain words and
 * the {max_bounces, max_fuzz} they were walked with. tests/specular_temporal_ref.py is the normative
 * definition; in words, with the rules of the two blocks it combines (fp32, no fused multiply-add,
 * their dot, projection, tap order and multiply-then-add sums):
 *
 * Per pixel of the new region: the first-hit guides n1, P1, D1, o1; the guides through the chain
 * n, P, Ds, o and the chain word ch of ONE rt_guide_options, k = ch & 0xff, e = (ch >> 8) & 0xff;
 * the new view's centre cn; the fresh colour c, its sample count m and variance v, sanitised as the
 * accumulation block does. The history holds c', L', V' and the planes above for its view.
 *   k == 0  the accumulation block's steps 1-3 verbatim on n1, P1, D1, o1 against the history's
 *           first-hit planes; kind = 1 where weight > 0.
 *   k >= 1  no history unless the history holds chain planes walked with bit-equal guide options
 *           and the specular-reprojection block's conditions hold: e == 1, 0 <= o < n_objects and
 *           reusable[o], 0 <= o1 < n_objects and through[o1], P, P1 and Ds finite, D1 finite and
 *           > 0. Then r = Ds / D1, X = cn + (P1 - cn) r, and X is projected in place of P. A tap
 *           counts iff it passes that block's chain tap test (equal chain word, first-hit object
 *           == o1, chain object == o, n.n' >= normal_min, |n.(P' - P)| <= sigma_plane Ds,
 *           q.q <= (pp2 Ds) Ds) with the accumulation block's colour and length conditions (c'
 *           finite, L' finite and > 0) in place of the finite flag. ws, acc, av, al, the min_weight
 *           cut, h, Vh, Lh, N = min(Lh, max_history) and the three blend cases are the accumulation
 *           block's steps 2-3 unchanged; kind = 2 where weight > 0.
 *   filter_levels > 0: step 4 with the CHAIN guides of the new view as the filter's guides (what
 *           rt_camera_set_denoise_guides selects for the filters), so what a mirror shows is
 *           edge-stopped by the surface it shows. length_out, weight_out and kind_out are never
 *           filtered; the history keeps the unfiltered values.
 *   Commit: as step 5, plus the new view's chain planes, chain words and guide options.
 * Plain and specular calls mix freely on one history. rt_camera_progressive_accumulate is bit for
 * bit what it was and commits a view without chain planes. A specular call uses the history's chain
 * planes only if the last committed view holds them AND they were walked with bit-equal
 * max_bounces and max_fuzz; otherwise every k >= 1 pixel has weight 0 and the call commits its own.
 *
 * THE CALLER MUST VARY THE SEED PER VIEW, as above. Limits as the specular-reprojection block: a
 * curved mirror's image does not lie at the summed length, so it gets little or no history; glass
 * is approximate (the Schlick split varies with the angle); grazing reflections are under-covered
 * by the isotropic point check; chains that leave the scene or reach max_bounces get none; the
 * lighting must be unchanged. Not in the N-API addon and not in the multi-GPU render.
 *
 * RT_ERR_INVALID, decided before any device call: everything the two blocks refuse - negative or
 * non-finite temporal options, filter_levels outside 0..8, guide options
 * rt_camera_render_guides_ex would refuse, mode RT_GUIDES_FIRST_HIT, a negative or non-finite
 * point_pixels, a through mask outside 0..15, no open session, mode bounces / samples,
 * samples_done < 2, a history of another scene or device, a missing pointer or an empty region of
 * the explicit entry - and some but not all of its prev_chain* arguments NULL. */
typedef struct { rt_temporal_options base; float point_pixels; int32_t through; } rt_specular_temporal_options;   /* NULL or a zero field = default (base's, 4, 15) */
/* {{0.9, 0.01, 0.25, 256, 0, 2.0}, 4, 15}. Host only. */
void rt_specular_temporal_options_default(rt_specular_temporal_options* options);
/* held = 1 iff the last committed view holds chain planes; out then receives the options they were
 * walked with (mode RT_GUIDES_SPECULAR), else {RT_GUIDES_SPECULAR, 0, 0}. Host only. */
int rt_history_chain_guides(const rt_history* h, rt_guide_options* out, int32_t* held);
/* rt_camera_progressive_accumulate through the chains: the session's kept first-hit guides and its
 * kept chain guides with their chain plane serve (those rt_camera_progressive_reproject_specular
 * and the filters keep, walked again when the options change); guide_options NULL =
 * {RT_GUIDES_SPECULAR, 8, 0}; the through table is the camera's for options->through and
 * guide_options->max_fuzz, kept by the history and rebuilt when either changes. kind_out: HOST
 * width*height uint8 (0 none, 1 first hit, 2 chain), only the region written. The session's state,
 * frame, stats and the bytes of rt_camera_progressive_save are never touched. rt_history_times
 * covers the call; its guide_ms includes the chain walk. */
int rt_camera_progressive_accumulate_specular(rt_camera* cam, rt_history* h, const rt_guide_options* guide_options,
                                              const rt_specular_temporal_options* options, int32_t commit, uint8_t* rgb,
                                              float* radiance, float* variance_out, float* length_out, float* weight_out,
                                              uint8_t* kind_out);
/* Explicit HOST buffers, no camera and no history object (the calling thread's current device), as
 * rt_temporal_accumulate, plus the new `view`, both views' chain guides and chain words (walked
 * with one rt_guide_options), `through` and kind_out. prev_chain_normal .. prev_chain all NULL: the
 * history holds no chain planes; some but not all of them NULL: RT_ERR_INVALID. */
int rt_temporal_accumulate_specular(int32_t width, int32_t height, const rt_region* region, const float* normal,
                                    const float* position, const float* distance, const int32_t* object,
                                    const float* chain_normal, const float* chain_position, const float* chain_distance,
                                    const int32_t* chain_object, const int32_t* chain, const rt_view* view,
                                    const float* radiance, const int32_t* px_samples, int32_t samples,
                                    const float* variance, const rt_view* prev_view, const rt_region* prev_region,
                                    const float* prev_normal, const float* prev_position, const float* prev_distance,
                                    const int32_t* prev_object, const float* prev_chain_normal,
                                    const float* prev_chain_position, const float* prev_chain_distance,
                                    const int32_t* prev_chain_object, const int32_t* prev_chain,
                                    const float* prev_radiance, const float* prev_variance, const float* prev_length,
                                    const uint8_t* reusable, const uint8_t* through, int32_t n_objects,
                                    const rt_specular_temporal_options* options, float* radiance_out,
                                    float* variance_out, float* length_out, float* weight_out, uint8_t* rgb_out,
                                    uint8_t* kind_out);

/* ---- Focused steps: the next samples go to the noisiest pixels ---------------------------------
 * No reference counterpart (the reference gives every pixel the same loop). Opt-in: a session
 * that never takes a focused step is what it was. tests/focus_ref.py is the normative NumPy
 * definition of the selection; the device result equals it exactly.
 *
 * A focused step of n_samples on the open session:
 *   1. Score, one fp32 per pixel of the region, from options->source:
 *        RT_FOCUS_SCORE_VARIANCE  the session's own variance, the value
 *                                 rt_camera_progressive_variance returns (needs samples_done >= 2);
 *        RT_FOCUS_SCORE_MAP       `score`: a HOST map, REGION-PACKED (pixel (i, j) of the region
 *                                 at (j - region.y) * region.width + (i - region.x)) - a
 *                                 variance_out of the variance-guided filter cut to the region,
 *                                 or anything else;
 *        RT_FOCUS_SCORE_HISTORY   `h`'s variance plane; only when the history's last committed
 *                                 region and image size are the session's and it lives on the
 *                                 session's device.
 *      Sanitised as the variance filter does: not (>= 0 and finite) becomes 0.
 *   2. Eligible: the pixels still sampling (the session's active list) with score > min_score.
 *      min_score defaults to 0, so a zero score is never chosen.
 *   3. Budget: K = (active_pixels * permille + 999) / 1000 in integers, permille in 1..1000
 *      (default 250); capped by max_pixels when that is > 0.
 *   4. Threshold: T = the K-th largest eligible score, compared as the uint32 bit pattern (which
 *      orders non-negative finite floats).
 *   5. Selected: the eligible pixels with score >= T; all of them when at most K are eligible.
 *      Ties at T are ALL taken, so more than K pixels may be selected, and the selected set is a
 *      function of the scores alone (the order of the active list is not deterministic).
 *   6. Nothing eligible: the step renders nothing, changes nothing and returns RT_OK with
 *      selected = 0.
 *   7. The selected pixels render the sample indices [samples + focus_done, samples + focus_done
 *      + n_samples), `samples` being the camera's loop count; focus_done, a cursor of the
 *      session, then advances by n_samples. samples_done does not move: the plain windows
 *      [0, samples) are never consumed by a focused step.
 *   8. The records are settled as a plain step's: in sample order, the convergence check after
 *      every sample, a pixel finished at `samples` samples and what was rendered past that
 *      dropped. One resolve pass follows; the outputs are those of rt_camera_progressive_step.
 *
 * Consequences.
 *   - A pixel that was never selected holds samples_done samples and is still bit-identical to
 *     the one-shot render with `samples: samples_done`: the session's contract holds per pixel.
 *   - A selected pixel holds more samples than that; px_samples says how many.
 *     rt_camera_progressive_variance, _denoise_variance and _accumulate use each pixel's own count.
 *   - active_pixels no longer means "holds samples_done samples" once a focused step has run.
 *   - Plain and focused steps mix freely. A selected pixel stops at `samples` samples like any
 *     other and is never visited again.
 *   - The frame depends on the selected sets only: cutting a focused step in two (the same set
 *     selected both times) or selecting other pixels beside a pixel does not change it.
 *   - A session that has taken a focused step that rendered refuses rt_camera_progressive_save
 *     with RT_ERR_INVALID ("progressive: a focused session cannot be saved"): blob format
 *     version 1 has no field for focus_done.
 *
 * RT_ERR_INVALID, decided before any device call: n_samples outside 1..65535 (the pool kernel
 * keeps a step's relative sample index in 16 bits); permille outside 1..1000; a negative or
 * non-finite min_score; a negative max_pixels; an unknown source; RT_FOCUS_SCORE_MAP with a NULL
 * score, RT_FOCUS_SCORE_HISTORY with a NULL, empty or mismatching history; no open session; mode
 * bounces / samples; RT_FOCUS_SCORE_VARIANCE while samples_done < 2; samples + focus_done +
 * n_samples above INT32_MAX. */
#define RT_FOCUS_SCORE_VARIANCE 0
#define RT_FOCUS_SCORE_MAP 1
#define RT_FOCUS_SCORE_HISTORY 2
typedef struct { int32_t source, permille; float min_score; int32_t max_pixels; } rt_focus_options;   /* NULL = rt_focus_options_default; every field is taken as it is */
typedef struct {
    int64_t active;           /* pixels still sampling before the step */
    int64_t eligible;         /* of them: score > min_score */
    int64_t selected;         /* of them: score >= threshold (0: the step rendered nothing) */
    float threshold;          /* T (0 when nothing was eligible) */
    int32_t focus_done;       /* the session's cursor after the step */
    int32_t first_sample;     /* the first sample index of the step's window */
    float select_ms;          /* device time of the selection (score, select, compact) from HIP events */
} rt_focus_info;
/* {RT_FOCUS_SCORE_VARIANCE, 250, 0, 0}. Host only. */
void rt_focus_options_default(rt_focus_options* options);
/* One focused step (above). rgb / radiance / px_samples / px_bounces / stats as
 * rt_camera_progressive_step; selected_out: HOST width*height uint8, 1 at every pixel the step
 * selected and 0 at the other pixels of the region (only the region is written); score and h as
 * options->source says (the others are ignored); any output and info may be NULL. */
int rt_camera_progressive_focus(rt_camera* cam, int32_t n_samples, const rt_focus_options* options, const float* score,
                                rt_history* h, uint8_t* rgb, float* radiance, int32_t* px_samples, int32_t* px_bounces,
                                uint8_t* selected_out, rt_render_stats* stats, rt_focus_info* info);

/* ---- Sub-pixel coverage and the filters' edge hold ------------------------------------------------
 * Opt-in and additive like the blocks above: no other call changes, RT_AMD_VERSION stays.
 *
 * A pixel whose footprint shows more than one surface is an anti-aliased mix, but its guides name
 * the one surface its centre ray hits; the filters average it with that surface's neighbours and
 * destroy the mix. On a low-noise frame of a scene with sub-pixel geometry that costs more than the
 * filter removes. The edge hold copies exactly those pixels through unfiltered.
 *
 * Coverage (tests/coverage_ref.py is the definition): for every pixel of the region k x k
 * deterministic pinhole primary rays, k in {2, 4}. Sub-ray (a, b), a, b in 0..k-1, has the offsets
 * ox = (a + 0.5) / k - 0.5 and oy = (b + 0.5) / k - 0.5 (exact in fp32); origin = the camera's
 * centre, direction = ((pixel00 + du i + dv j, as rt_camera_render_guides forms it) + du ox) + dv oy
 * - centre, each vector operation in fp32; no RNG and no defocus sample whatever the camera's
 * aperture; reference precision whatever the camera's; interval (0.001, inf); the camera's
 * traversal. The coverage word of a pixel:
 *   bit b k + a   the sub-ray shows the object rt_camera_render_guides reports for the pixel (the
 *                 index in SceneData.objects; a miss is -1, and a miss equals a miss)
 *   bits 16..23   the number of distinct objects among the sub-rays and the centre ray
 * A pixel is MIXED when one of the low k^2 bits is clear.
 * rt_camera_render_coverage: `coverage` is HOST width*height uint32, full-frame layout, only the
 * region (NULL: the whole image) written; computed on the camera's device context.
 *
 * The hold forms of the six filter entries take one more argument and are otherwise their base
 * entries: a held pixel takes part in every level as ever, also as a tap of its neighbours, and the
 * last pass writes its INPUT instead - radiance_out and the u8 from the input radiance as it stands,
 * variance_out the input variance sanitised as the filter reads it (not (v >= 0 and finite) -> 0).
 * rt_denoise_hold / rt_denoise_variance_hold: `hold` is HOST width*height uint8, full-frame layout,
 * non-zero = held, only the region read. The camera and session forms take hold_k: 0 = no hold
 * (the base entry, byte for byte), 2 or 4 = the mixed pixels of that coverage, computed on the
 * device; a session computes the mask once per hold_k and keeps it as it keeps its guides. The mask
 * always comes from first-hit pinhole sub-rays, whatever rt_camera_set_denoise_guides selected.
 * rt_camera_coverage_time: device time of the camera's last coverage pass (either entry kind) from
 * HIP events; the pass runs before the span rt_camera_denoise_times reports and is not part of it.
 * RT_ERR_INVALID, decided before any device call: k not 2 or 4, hold_k not 0, 2 or 4, a NULL
 * coverage or hold, and whatever the base entry refuses; rt_camera_coverage_time before any pass.
 * Limits: the mask is pinhole, so a defocus camera's blur is not in it; held pixels stay as noisy
 * as they were; behind mirrors and glass the mask describes the specular surface, not what it
 * shows. rt_camera_progressive_accumulate's filter, the N-API addon and multi-GPU renders have no
 * hold form. */
int rt_camera_render_coverage(rt_camera* cam, const rt_region* region, int32_t k, uint32_t* coverage);
int rt_camera_coverage_time(rt_camera* cam, float* coverage_ms);
int rt_denoise_hold(int32_t width, int32_t height, const rt_region* region, const rt_denoise_options* options,
                    const float* radiance, const float* normal, const float* position, const float* distance,
                    const int32_t* object, const uint8_t* hold, float* radiance_out, uint8_t* rgb_out);
int rt_denoise_variance_hold(int32_t width, int32_t height, const rt_region* region,
                             const rt_denoise_var_options* options, const float* radiance, const float* variance,
                             const float* normal, const float* position, const float* distance, const int32_t* object,
                             const uint8_t* hold, float* radiance_out, float* variance_out, uint8_t* rgb_out);
int rt_camera_denoise_hold(rt_camera* cam, const rt_region* region, const rt_denoise_options* options, int32_t hold_k,
                           const float* radiance, float* radiance_out, uint8_t* rgb_out);
int rt_camera_denoise_variance_hold(rt_camera* cam, const rt_region* region, const rt_denoise_var_options* options,
                                    int32_t hold_k, const float* radiance, const float* variance, float* radiance_out,
                                    float* variance_out, uint8_t* rgb_out);
int rt_camera_progressive_denoise_hold(rt_camera* cam, const rt_denoise_options* options, int32_t hold_k, uint8_t* rgb,
                                       float* radiance);
int rt_camera_progressive_denoise_variance_hold(rt_camera* cam, const rt_denoise_var_options* options, int32_t hold_k,
                                                uint8_t* rgb, float* radiance, float* variance_out);

#ifdef __cplusplus
}
#endif

#endif /* RT_AMD_H */
