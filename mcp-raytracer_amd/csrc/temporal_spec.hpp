// Accumulation across views through specular chains (rt_temporal_accumulate_specular,
// rt_camera_progressive_accumulate_specular): temporal_spec.hip. A pixel whose chain word has
// k = ch & 0xff == 0 is temporal.hpp's pixel on the first-hit guides. A pixel with k >= 1 whose
// chain ends on a surface looks for its history at reproject_spec.hpp's point X and tests the
// history's taps on the chain planes the history keeps of its view; a tap counts where
// reproject_spec.hpp's chain test holds with temporal.hpp's colour and length conditions in place
// of the finite flag. The sums, the min_weight cut and the blend by the gathered length and
// variance are temporal.hpp's. tests/specular_temporal_ref.py is the normative definition; the
// device result equals it in every bit.
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

#ifdef __HIPCC__
// The variance filter's rule: not (v >= 0 and finite) -> 0.
__device__ __forceinline__ float ts_variance(float v) { return v >= 0.0f && rs_finite(v) ? v : 0.0f; }

// The tap test of a k >= 1 pixel: rs_chain_tap_counts with the accumulation's colour and length
// conditions - cq = {r, g, b, length}, all finite, the length > 0 - in place of the finite flag.
// (every comparison is false for a NaN)
__device__ __forceinline__ bool ts_chain_tap_counts(const RsChainPixel& p, float normal_min, const float4& pfirst,
                                                    const float4& nq, const float4& Pq, const float4& cq, int32_t chq) {
    const float ex = Pq.x - p.P.x, ey = Pq.y - p.P.y, ez = Pq.z - p.P.z;
    const float dn = rs_dot(p.n.x, p.n.y, p.n.z, nq.x, nq.y, nq.z);
    const float e = rs_dot(p.n.x, p.n.y, p.n.z, ex, ey, ez);
    const float qq = rs_dot(ex, ey, ez, ex, ey, ez);
    return chq == p.ch && __float_as_int(pfirst.w) == p.o1 && __float_as_int(Pq.w) == __float_as_int(p.P.w) &&
           rs_finite(cq.x) && rs_finite(cq.y) && rs_finite(cq.z) && dn >= normal_min && fabsf(e) <= p.plane &&
           qq <= p.point && rs_finite(cq.w) && cq.w > 0.0f;
}
#endif

// One thread per pixel of the new region. nw: the new view's first-hit pair, chain pair and chain
// words; through: object index -> 1 where a chain may start; px_samples may be null (the scalar
// count a.m); kind: uint8, region-packed. Null or negative parameters: hipErrorInvalidValue.
hipError_t launch_temporal_spec(const TsArgs& a, const RsGuides& nw, const TsHistory& hist, const uint8_t* reusable,
                                const uint8_t* through, const float* fresh, const int32_t* px_samples,
                                const float* variance, const TpOut& out, uint8_t* kind, hipStream_t stream);

}  // namespace rt
