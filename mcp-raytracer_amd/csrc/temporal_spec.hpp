// Accumulation across views through specular chains (rt_temporal_accumulate_specular,
// rt_camera_progressive_accumulate_specular): temporal_spec.hip. A pixel whose chain word has
// k = ch & 0xff == 0 is temporal.hpp's pixel on the first-hit guides. A pixel with k >= 1 whose
// chain ends on a surface looks for its history at reproject_spec.hpp's point X and tests the
// history's taps on the chain planes the history keeps of its view; a tap counts where
// reproject_spec.hpp's chain test holds with temporal.hpp's colour and length conditions in place
// of the finite flag. The sums, the min_weight cut and the blend by the gathered length and
// variance are temporal.hpp's; one copy of each of these pieces is in gather.hpp.
// tests/specular_temporal_ref.py is the normative definition; the device result equals it in
// every bit.
// All device arrays are REGION-PACKED as in denoise.hpp. The kernel writes temporal.hpp's TpOut
// and the kind plane (uint8: 0 no history, 1 first hit, 2 chain) directly - no staging plane.
// No reference counterpart: the reference renders every frame from scratch.
#pragma once

#include "reproject_spec.hpp"
#include "temporal.hpp"

namespace rt {

struct TsArgs {
    RpView view;                     // the history's view (unused while pw == 0)
    float cn[3];                     // the new view's centre
    float pp2;                       // reproject_spec.hpp's pp2 for the history's view, host fp32
    int32_t w, h;                    // the new region
    int32_t px0, py0, pw, ph;        // the history's region; pw == 0: an empty history
    int32_t n_objects;
    int32_t chain_history;           // the history holds chain planes (of the same guide options)
    float normal_min, sigma_plane, min_weight, max_history;
    int32_t pitch, fx0, fy0;         // the fresh frame's and the counts' layout, as TpArgs
    int32_t vpitch, vx0, vy0;        // the fresh variance's
    float m;                         // the scalar sample count (px_samples == null)
};

// The history's side of a launch: its first-hit pair, its chain planes (null unless
// chain_history), colour {r, g, b, length} and variance. All null while the history is empty.
struct TsHistory {
    RsGuides g;
    const float4* col;
    const float* var;
};

// One thread per pixel of the new region. nw: the new view's first-hit pair, chain pair and chain
// words; through: object index -> 1 where a chain may start; px_samples may be null (the scalar
// count a.m); kind: uint8, region-packed. Null or negative parameters: hipErrorInvalidValue.
hipError_t launch_temporal_spec(const TsArgs& a, const RsGuides& nw, const TsHistory& hist, const uint8_t* reusable,
                                const uint8_t* through, const float* fresh, const int32_t* px_samples,
                                const float* variance, const TpOut& out, uint8_t* kind, hipStream_t stream);

}  // namespace rt
