// Accumulation across views with a per-pixel history length and variance (rt_temporal_accumulate,
// rt_camera_progressive_accumulate): temporal.hip. The new view's first-hit points are projected
// into the history's view exactly as reproject.hpp does; the taps that show the same surface AND
// hold a history (length finite and > 0) give the history's colour, variance and length, which
// are blended with the fresh frame by the pixel's own counts: N = min(length, max_history)
// against m fresh samples. tests/temporal_ref.py is the normative definition; the device result
// equals it in every bit.
// All device arrays are REGION-PACKED as in denoise.hpp. A history plane pair is
//   colour {r, g, b, length}   and   variance (float)
// beside the guides gn / gp of the view it was committed from. The kernel writes the same pair
// for the new view, so a commit is a swap of the two sets.
// No reference counterpart: the reference renders every frame from scratch.
#pragma once

#include "reproject.hpp"

namespace rt {

struct TpArgs {
    RpView view;                     // the history's view (unused while pw == 0)
    int32_t w, h;                    // the new region
    int32_t px0, py0, pw, ph;        // the history's region; pw == 0: an empty history
    int32_t n_objects;
    float normal_min, sigma_plane, min_weight, max_history;
    // the fresh frame (float[3] per pixel) and the per-pixel sample counts share one layout: row
    // pitch `pitch` pixels, the region's first pixel at (fx0, fy0); the fresh variance has its own
    int32_t pitch, fx0, fy0;
    int32_t vpitch, vx0, vy0;
    float m;                         // the scalar sample count (px_samples == null)
};

// The history's side of a launch (null while the history is empty) and what the launch writes.
struct TpHistory {
    const float4 *gn, *gp, *col;
    const float* var;
};
struct TpOut {
    float4* col;   // {out.rgb, Lout}
    float* var;    // Vout
    float* weight;
};

// One thread per pixel of the new region. px_samples may be null (the scalar count A.m).
hipError_t launch_temporal(const TpArgs& a, const float4* gn, const float4* gp, const TpHistory& hist,
                           const uint8_t* reusable, const float* fresh, const int32_t* px_samples, const float* variance,
                           const TpOut& out, hipStream_t stream);

// {r, g, b} (float[3], region-packed) and a length plane -> the history's colour plane: the
// explicit entry's upload of a previous view.
hipError_t launch_temporal_pack(const float* rad, const float* length, int n, float4* col, hipStream_t stream);

}  // namespace rt
