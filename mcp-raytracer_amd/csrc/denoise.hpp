// First-hit guide buffers and the guided edge-avoiding a-trous filter (rt_camera_render_guides,
// rt_denoise, rt_camera_denoise, rt_camera_progressive_denoise and their *_variance forms):
// denoise.hip. All device arrays here are REGION-PACKED: pixel (i, j) of a w x h region at
// (x0, y0) is element (j - y0) * w + (i - x0). The filter reads three float4 per pixel:
//   colour {r, g, b, w}                           - ping-pong, one pair per call
//   fn     {n.xyz, 1 / (sigma_plane * distance)}  - per call (the parameters may change)
//   gp     {P.xyz, object index bits}             - the guides as the guide pass writes them
// and the guide pass also keeps gn {n.xyz, distance}, from which fn is made.
// The filter has two forms, one implementation with a compile-time switch. The plain form
// stops at colour edges by the RGB distance over a launch-wide sigma_color, and colour.w is the
// pixel's finite flag (1.0f / 0.0f). The variance-guided form stops by the luminance difference
// relative to the centre pixel's own (3x3 pre-blurred) variance and filters the variance along
// with the colour: colour.w is the variance, >= 0 as a value, and its SIGN BIT is the pixel's
// "colour is not finite" flag.
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

// The guides at the first non-specular surface along the pixel's specular chain (guide_walk.hip;
// tests/guide_walk_ref.py is the definition, include/rt_amd.h restates it): segment 0 is
// launch_guides' ray, and a fuzz <= max_fuzz metal, glass, or what a mixed / layered material
// resolves to continues the walk by one deterministic direction, up to max_bounces times. Same
// outputs and layout, the distance summed over the segments; chain (region-packed int32, or
// null) receives segments continued | end code << 8 (0 miss, 1 terminal surface, 2 the chain
// left the scene: the last specular surface is the guide, 3 max_bounces reached).
hipError_t launch_guide_walk(const DevScene& S, int trav, const RtRegion& reg, const int32_t* prim_object,
                             const DenoiseGuides& g, int32_t* chain, int max_bounces, float max_fuzz, int lds_max,
                             hipStream_t stream);
// The chain word of first-hit guides: hit ? 1 << 8 : 0, from gp's object bits.
hipError_t launch_guides_chain(const DenoiseGuides& g, int n, int32_t* chain, hipStream_t stream);

// gn / gp -> the caller-facing arrays (region-packed: normal, position float[3], distance float,
// object int32; any may be null), and back (explicit guides, rt_denoise).
hipError_t launch_guides_unpack(const DenoiseGuides& g, int n, float* normal, float* position, float* distance,
                                int32_t* object, hipStream_t stream);
hipError_t launch_guides_pack(const DenoiseGuides& g, int n, const float* normal, const float* position,
                              const float* distance, const int32_t* object, hipStream_t stream);

// The filter's per-call inputs: colour from `rad` (float[3] per pixel, row pitch `pitch_px`
// pixels, the region's first pixel at rad + 3 * (y0 * pitch_px + x0)), and
// fn = {n.xyz, 1 / (sigma_plane * distance)} from gn. `variance` (region-packed; not (v >= 0 and
// finite) -> 0) selects the variance-guided form's colour.w, null the plain one's.
hipError_t launch_denoise_pack(const float* rad, int pitch_px, int x0, int y0, int w, int h, const float4* gn,
                               float sigma_plane, const float* variance, float4* colour, float4* fn,
                               hipStream_t stream);
// One level: step = 1 << level taps of the 5x5 B3 kernel. ks (host, double -> fp32): the plain
// form's k_c = 4^level / sigma_color^2, or with `var` the variance-guided form's
// s2 = sigma_variance^2, whose 3x3 variance pre-blur of the centre pixel runs inside the kernel.
// Steps 1 and 2 stage a 16x16 tile plus halo in LDS; larger steps read global memory.
hipError_t launch_denoise_level(bool var, const float4* src, float4* dst, const float4* fn, const float4* gp, int w,
                                int h, int step, float ks, hipStream_t stream);
// The edge hold (coverage.hpp): pixels the filter's unpack pass copies through. mask: region-packed,
// non-zero = held (null: none). A held pixel took part in every level as ever, taps included; its
// outputs are the filter's inputs as launch_denoise_pack read them: `rad` / pitch_px / x0 / y0 and
// the region's width w, and `variance` (region-packed, sanitised as there; null: the plain form).
struct DenoiseHold {
    const uint8_t* mask = nullptr;
    const float* rad = nullptr;
    int pitch_px = 0, x0 = 0, y0 = 0, w = 0;
    const float* variance = nullptr;
};

// colour -> region-packed float[3] radiance and / or its u8 (the frame's own to_u8) and / or,
// after the variance-guided form, the filtered variance (the flag bit cleared). hold: above; its
// inputs may be the very arrays `rad` and `variance` name.
hipError_t launch_denoise_unpack(const float4* colour, int n, float* rad, uint8_t* rgb, float* variance,
                                 hipStream_t stream, const DenoiseHold& hold = DenoiseHold{});

}  // namespace rt
