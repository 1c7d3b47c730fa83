// The per-pixel variance map of a progressive session and the variance-guided a-trous filter
// (rt_camera_progressive_variance, rt_progressive_blob_variance, rt_denoise_variance,
// rt_camera_denoise_variance, rt_camera_progressive_denoise_variance): denoise_var.hip.
// The filter is denoise.hpp's with the colour edge-stop replaced by a luminance difference
// relative to the centre pixel's own (3x3 pre-blurred) variance, and the variance filtered
// along with the colour. Arrays are REGION-PACKED as in denoise.hpp; a pixel is still three
// float4:
//   colour {r, g, b, variance}   - ping-pong; the variance is >= 0 as a value, and its SIGN BIT
//                                  is the pixel's "colour is not finite" flag
//   fn, gp                       - as denoise.hpp
// No reference counterpart beyond the variance formula (src/camera.ts:356-357).
#pragma once

#include "denoise.hpp"
#include "progressive.hpp"

namespace rt {

// Variance of the mean of a pixel's sample illuminances from its running sums, in fp64 in the
// reference's expression order (pixelConverged, src/camera.ts:357, then / n), rounded to fp32
// once; n < 2, NaN and negatives give 0. Host and device evaluate this same function.
__host__ __device__ inline float prog_variance(double sum_ill, double sum_ill2, uint32_t n) {
    if (n < 2u) return 0.0f;
    const double dn = (double)n;
    const double m2 = sum_ill2 - (sum_ill * sum_ill) / dn;
    const double v = (m2 / (dn - 1.0)) / dn;
    return (float)(v > 0.0 ? v : 0.0);
}
inline uint32_t prog_pix_samples(const ProgPix& p) {
    uint32_t w;
    __builtin_memcpy(&w, &p.c.w, sizeof w);
    return w & ~kProgFinished;
}

// State -> region-packed variance (one float per pixel of the region), one thread per session
// slot (slot = region tile * 64 + lane, item_pixel numbering); slots outside the region write
// nothing.
hipError_t launch_prog_variance(const ProgPix* state, int slots, const RtRegion& reg, int tiles_x, float* variance,
                                hipStream_t stream);

// The filter's per-call inputs: colour {r, g, b, variance | flag} from `rad` (as
// launch_denoise_pack) and the region-packed `variance` (not (v >= 0 and finite) -> 0), and fn.
hipError_t launch_denoise_var_pack(const float* rad, int pitch_px, int x0, int y0, int w, int h, const float4* gn,
                                   float sigma_plane, const float* variance, float4* colour, float4* fn,
                                   hipStream_t stream);
// One level: step = 1 << level taps of the 5x5 B3 kernel; s2 = sigma_variance^2 (host, double ->
// fp32). Steps 1 and 2 stage a 16x16 tile plus halo in LDS; larger steps read global memory.
// The 3x3 variance pre-blur of the centre pixel runs inside the level kernel.
hipError_t launch_denoise_var_level(const float4* src, float4* dst, const float4* fn, const float4* gp, int w, int h,
                                    int step, float s2, hipStream_t stream);
// colour.w -> the region-packed filtered variance (the flag bit cleared).
hipError_t launch_denoise_var_unpack(const float4* colour, int n, float* variance, hipStream_t stream);

}  // namespace rt
