// Reprojection of a previous view's frame into a new camera view (rt_reproject,
// rt_camera_reproject, rt_camera_progressive_reproject): reproject.hip. The new view's first-hit
// points are projected into the previous view, whose radiance is gathered bilinearly from the
// taps that show the same surface (object, normal and plane checks), and optionally blended with
// a fresh frame as if the history held history_samples samples. tests/reproject_ref.py is the
// normative definition; the device result equals it in every bit.
// All device arrays are REGION-PACKED as in denoise.hpp. The kernel reads the new view's guides
// gn / gp, and per tap three float4 of the previous view: its gn, its gp and its colour
// {r, g, b, finite flag} as the plain filter's pack pass writes it.
// No reference counterpart: the reference renders every frame from scratch.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace rt {

// The previous view and its per-view constants, all fp32, computed on the host in the
// definition's operation order (rp_view_constants).
struct RpView {
    float c[3];   // centre
    float a[3];   // pixel00 - centre
    float du[3], dv[3];
    float w[3];   // cross(du, dv)
    float aw;     // dot(a, w)
    float iu, iv; // 1 / dot(du, du), 1 / dot(dv, dv)
    int32_t width, height;
};

// dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z; each product and sum rounded once.
inline RpView rp_view_constants(const float* center, const float* pixel00, const float* du, const float* dv,
                                int32_t width, int32_t height) {
    RpView v{};
    for (int k = 0; k < 3; ++k) {
        v.c[k] = center[k];
        v.a[k] = pixel00[k] - center[k];
        v.du[k] = du[k];
        v.dv[k] = dv[k];
    }
    auto sub_prod = [](float p, float q, float r, float s) {
        const float x = p * q, y = r * s;
        return x - y;
    };
    v.w[0] = sub_prod(du[1], dv[2], du[2], dv[1]);
    v.w[1] = sub_prod(du[2], dv[0], du[0], dv[2]);
    v.w[2] = sub_prod(du[0], dv[1], du[1], dv[0]);
    auto dot = [](const float* a, const float* b) {
        const float x = a[0] * b[0], y = a[1] * b[1], z = a[2] * b[2];
        const float xy = x + y;
        return xy + z;
    };
    v.aw = dot(v.a, v.w);
    v.iu = 1.0f / dot(du, du);
    v.iv = 1.0f / dot(dv, dv);
    v.width = width;
    v.height = height;
    return v;
}

struct RpArgs {
    RpView view;
    int32_t w, h;                    // the new region
    int32_t px0, py0, pw, ph;        // prev_region (clamped to the previous image)
    int32_t n_objects;
    float normal_min, sigma_plane, min_weight, nh;
    // the fresh frame (float[3] per pixel) and the per-pixel sample counts share one layout: row
    // pitch `pitch` pixels, the region's first pixel at (fx0, fy0)
    int32_t pitch, fx0, fy0;
    float m;                         // the scalar sample count (px_samples == null)
};

// One thread per pixel of the new region. hist = {history.rgb, weight}; outc (with `fresh`) =
// {blend.rgb, 0}. fresh / px_samples / outc may be null.
hipError_t launch_reproject(const RpArgs& a, const float4* gn, const float4* gp, const float4* pgn, const float4* pgp,
                            const float4* pcol, const uint8_t* reusable, const float* fresh, const int32_t* px_samples,
                            float4* hist, float4* outc, hipStream_t stream);

}  // namespace rt
