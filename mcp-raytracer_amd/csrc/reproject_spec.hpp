// Reprojection of a previous view's frame through specular chains (rt_reproject_specular,
// rt_camera_reproject_specular, rt_camera_progressive_reproject_specular): reproject_spec.hip.
// A pixel whose chain word has k = ch & 0xff == 0 is reproject.hpp's pixel on the first-hit
// guides. A pixel with k >= 1 whose chain ends on a surface (end code 1) looks for its history at
// X = cn + (P1 - cn) * (Ds / D1), the point at the chain's summed path length along the primary ray
// - where a planar mirror's image of the surface lies, whoever looks - and tests the previous
// view's taps on that view's chain guides. tests/specular_reproject_ref.py is the normative
// definition; the device result equals it in every bit.
// All device arrays are REGION-PACKED as in denoise.hpp. Per view the kernel reads the first-hit
// pair gn / gp, the pair through the chain sgn / sgp (both walked with one rt_guide_options) and
// the chain word; of the previous view also the colour {r, g, b, finite flag} as the plain filter's
// pack pass writes it. The projection, the tap walk and the tap tests are gather.hpp's, shared with
// reproject.hip and the two accumulation units.
// No reference counterpart: the reference renders every frame from scratch.
#pragma once

#include "reproject.hpp"

namespace rt {

struct RsArgs {
    RpView view;                     // the previous view
    float cn[3];                     // the new view's centre
    float pp2;                       // (point_pixels * point_pixels) * (du.du / a.a) of the previous view, host fp32
    int32_t w, h;                    // the new region
    int32_t px0, py0, pw, ph;        // prev_region (clamped to the previous image)
    int32_t n_objects;
    float normal_min, sigma_plane, min_weight, nh;
    int32_t pitch, fx0, fy0;         // the fresh frame's layout, as RpArgs
    float m;
};

// One view's guide planes.
struct RsGuides {
    const float4 *gn, *gp;    // first hit
    const float4 *sgn, *sgp;  // through the chain
    const int32_t* chain;
};

// One thread per pixel of the new region. through: object index -> 1 where a chain may start.
// hist = {history.rgb, weight}; outc = {blend.rgb (zero without `fresh`), kind as a float: 0 no
// history, 1 first hit, 2 chain}. fresh / px_samples may be null.
hipError_t launch_reproject_spec(const RsArgs& a, const RsGuides& nw, const RsGuides& pv, const float4* pcol,
                                 const uint8_t* reusable, const uint8_t* through, const float* fresh,
                                 const int32_t* px_samples, float4* hist, float4* outc, hipStream_t stream);
// outc.w -> kind (uint8, region-packed).
hipError_t launch_reproject_spec_kind(const float4* outc, int n, uint8_t* kind, hipStream_t stream);

}  // namespace rt
