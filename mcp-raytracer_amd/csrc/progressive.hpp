// Progressive rendering (rt_camera_progressive_*): the per-pixel state that outlives a call
// and the passes over it, its variance map among them (progressive.hip). The path kernels render a step's sample
// window [samples_done, samples_done + len) of the session's active pixels as they render an
// adaptive round (SampleBuf::s_base / act, 16-byte records, err_in_rec).
#pragma once

#include "launch.hpp"

namespace rt {

// A pixel's running PixelStats (src/render-utils/renderStats.ts:66-88), as AdaptPix, by the
// session's slot (region tile * 64 + lane): the single source of truth of a session - frame,
// RenderStats and the active list are rebuilt from it (pt_resolve_kernel), and it is the
// payload of a checkpoint blob. All zero = no sample yet.
struct ProgPix {
    float4 c;     // colour sum (fp32, sample order); w: n in bits 0-30, finished in bit 31
    double2 ill;  // sumIll, sumIll2
    int4 b;       // bounce sum (low 32 bits), min, max, bounce sum (high 32 bits)
};
static_assert(sizeof(ProgPix) == 48, "ProgPix is the checkpoint blob's record");
constexpr uint32_t kProgFinished = 0x80000000u;
inline uint32_t prog_pix_samples(const ProgPix& p) {
    uint32_t w;
    __builtin_memcpy(&w, &p.c.w, sizeof w);
    return w & ~kProgFinished;
}

// Variance of the mean of a pixel's sample illuminances from its running sums, in fp64 in the
// reference's expression order (pixelConverged, src/camera.ts:357, then / n), rounded to fp32
// once; n < 2, NaN and negatives give 0. Host (rt_progressive_blob_variance) and device
// (rt_camera_progressive_variance) evaluate this same function, neither with contraction.
__host__ __device__ inline float prog_variance(double sum_ill, double sum_ill2, uint32_t n) {
    if (n < 2u) return 0.0f;
    const double dn = (double)n;
    const double m2 = sum_ill2 - (sum_ill * sum_ill) / dn;
    const double v = (m2 / (dn - 1.0)) / dn;
    return (float)(v > 0.0 ? v : 0.0);
}

struct ProgPass {
    ProgPix* state;  // session slots
    int32_t len;     // samples of this step
};
struct ProgResolve {
    const ProgPix* state;
    int32_t slots;        // session slots (region tiles * 64)
    int32_t* act;         // out: the slots still sampling
    unsigned int* count;  // out: their number (zeroed by the caller)
};

// Adds a record pass's samples to its pixels' state in sample order, with the reference's
// convergence check after every sample (as pt_adapt_kernel); error flags of the kept
// samples go to out.stats.
hipError_t launch_settle(const DevScene& S, const RtRegion& reg, const RenderOut& out, int tiles_x,
                         const SampleBuf& sb, const ProgPass& pp, hipStream_t stream);
// State -> frame (finalColor / u8 / px_samples / px_bounces of every pixel of the region,
// finished or not), RenderStats (added to out.stats) and the active list.
hipError_t launch_resolve(const DevScene& S, const RtRegion& reg, const RenderOut& out, int tiles_x,
                          const ProgResolve& pr, hipStream_t stream);
// State -> region-packed variance map (one float per pixel of the region: pixel (i, j) is
// element (j - reg.y) * reg.width + (i - reg.x)), one thread per session slot; slots outside
// the region write nothing.
hipError_t launch_prog_variance(const ProgPix* state, int slots, const RtRegion& reg, int tiles_x, float* variance,
                                hipStream_t stream);

}  // namespace rt
