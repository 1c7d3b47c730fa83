// Sub-pixel coverage (rt_camera_render_coverage and the filters' edge hold): coverage.hip. For every
// pixel of a region K x K deterministic pinhole primary rays, K in {2, 4}, beside the pixel's own
// centre ray (launch_guides' ray, denoise.hpp). Sub-ray (a, b), a, b in 0..K-1, goes through the
// pixel centre + du ox + dv oy with ox = (a + 0.5) / K - 0.5 and oy = (b + 0.5) / K - 0.5 (exact in
// fp32), its direction formed as path_begin forms a jittered ray (pt_shade.hpp): centre, plus
// du ox, plus dv oy, minus the camera's centre, each vector operation rounded to fp32. Origin = the
// camera's centre, no RNG, no defocus sample, ref precision (Real = double) whatever the camera's,
// interval (0.001, inf), through the resolved traversal.
// The coverage word of a pixel (region-packed uint32, as denoise.hpp's arrays):
//   bit b K + a   sub-ray (a, b) shows the object of the centre ray (prim_object; a miss is -1, and
//                 a miss equals a miss)
//   bits 16..23   the number of distinct objects among the sub-rays and the centre (a miss is one)
// A pixel is MIXED when one of the low K^2 bits is clear. tests/coverage_ref.py is the definition.
// No reference counterpart: the reference renders a frame and never classifies its pixels.
#pragma once

#include "launch.hpp"

namespace rt {

// coverage (or null): the words; hold (or null): 1 for a mixed pixel, else 0 - the mask
// launch_denoise_unpack takes. Both region-packed. k outside {2, 4}: hipErrorInvalidValue, as when the
// traversal stack exceeds lds_max.
hipError_t launch_coverage(const DevScene& S, int trav, const RtRegion& reg, const int32_t* prim_object, int k,
                           uint32_t* coverage, uint8_t* hold, int lds_max, hipStream_t stream);

}  // namespace rt
