// First-hit guide buffers and the guided edge-avoiding a-trous filter (rt_camera_render_guides,
// rt_denoise, rt_camera_denoise, rt_camera_progressive_denoise): denoise.hip. All device arrays
// here are REGION-PACKED: pixel (i, j) of a w x h region at (x0, y0) is element
// (j - y0) * w + (i - x0). The filter reads three float4 per pixel:
//   colour {r, g, b, finite flag (1.0f / 0.0f)}   - ping-pong, one pair per call
//   fn     {n.xyz, 1 / (sigma_plane * distance)}  - per call (the parameters may change)
//   gp     {P.xyz, object index bits}             - the guides as the guide pass writes them
// and the guide pass also keeps gn {n.xyz, distance}, from which fn is made.
// No reference counterpart: the reference renders a frame and never filters it.
#pragma once

#include "launch.hpp"

namespace rt {

constexpr int kDenoiseMaxLevels = 8;

struct DenoiseGuides {
    float4* gn;  // {n.xyz, distance}
    float4* gp;  // {P.xyz, object bits}
};

// One deterministic pinhole primary ray per pixel of the region (origin = the camera's centre,
// direction = pixel00 + du i + dv j - centre in the path kernel's fp32 vector arithmetic: no
// jitter, no defocus sample, no RNG), ref precision (Real = double) whatever the camera's,
// through the resolved traversal `trav`, interval (0.001, inf). A miss writes zeros and object
// -1. prim_object: the device copy of the camera's prim slot -> SceneData.objects index map.
// lds_max: the dynamic LDS a workgroup may use (hipErrorInvalidValue when the stack exceeds it).
hipError_t launch_guides(const DevScene& S, int trav, const RtRegion& reg, const int32_t* prim_object,
                         const DenoiseGuides& g, int lds_max, hipStream_t stream);

// gn / gp -> the caller-facing arrays (region-packed: normal, position float[3], distance float,
// object int32; any may be null), and back (explicit guides, rt_denoise).
hipError_t launch_guides_unpack(const DenoiseGuides& g, int n, float* normal, float* position, float* distance,
                                int32_t* object, hipStream_t stream);
hipError_t launch_guides_pack(const DenoiseGuides& g, int n, const float* normal, const float* position,
                              const float* distance, const int32_t* object, hipStream_t stream);

// The filter's per-call inputs: colour {r, g, b, finite} from `rad` (float[3] per pixel, row
// pitch `pitch_px` pixels, the region's first pixel at rad + 3 * (y0 * pitch_px + x0)), and
// fn = {n.xyz, 1 / (sigma_plane * distance)} from gn.
hipError_t launch_denoise_pack(const float* rad, int pitch_px, int x0, int y0, int w, int h, const float4* gn,
                               float sigma_plane, float4* colour, float4* fn, hipStream_t stream);
// One level: step = 1 << level taps of the 5x5 B3 kernel, k_c = 4^level / sigma_color^2 (host).
// Steps 1 and 2 stage a 16x16 tile plus halo in LDS; larger steps read global memory.
hipError_t launch_denoise_level(const float4* src, float4* dst, const float4* fn, const float4* gp, int w, int h,
                                int step, float k_c, hipStream_t stream);
// colour -> region-packed float[3] radiance and / or its u8 (the frame's own to_u8).
hipError_t launch_denoise_unpack(const float4* colour, int n, float* rad, uint8_t* rgb, hipStream_t stream);

}  // namespace rt
