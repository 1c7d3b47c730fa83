// The gather the four view-history kernels share (reproject.hip, temporal.hip, reproject_spec.hip,
// temporal_spec.hip): project the new view's surface point into an older view, walk the four
// bilinear taps, test each tap's surface, blend. Device code only. Every unit that includes it is
// compiled with -ffp-contract=off and no fast-math flag, so each fp32 expression below has exactly
// one result; their form and order are pinned in every bit by tests/reproject_ref.py,
// tests/temporal_ref.py, tests/specular_reproject_ref.py and tests/specular_temporal_ref.py.
// `Args` is any of RpArgs / TpArgs / RsArgs / TsArgs: the functions read the fields those share.
#pragma once

#include "reproject_spec.hpp"

#ifdef __HIPCC__
namespace rt {

constexpr int kGaBlock = 256;
constexpr int kGaRow = 64;  // a workgroup is 4 rows of 64 pixels, as denoise_global_kernel

inline dim3 ga_grid(int w, int h) {
    return dim3((unsigned)((w + kGaRow - 1) / kGaRow), (unsigned)((h + kGaBlock / kGaRow - 1) / (kGaBlock / kGaRow)));
}

__device__ __forceinline__ bool ga_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ float ga_dot(float ax, float ay, float az, float bx, float by, float bz) {
    return (ax * bx + ay * by) + az * bz;
}
// The variance filter's rule: not (v >= 0 and finite) -> 0.
__device__ __forceinline__ float ga_variance(float v) { return v >= 0.0f && ga_finite(v) ? v : 0.0f; }

// The thread's pixel of the w x h region and its region-packed index; false outside the region.
struct GaPixel {
    int px, py;
    size_t k;
};
__device__ __forceinline__ bool ga_pixel(int w, int h, GaPixel& p) {
    p.px = blockIdx.x * kGaRow + (int)(threadIdx.x & (kGaRow - 1));
    p.py = blockIdx.y * (kGaBlock / kGaRow) + (int)(threadIdx.x / kGaRow);
    if (p.px >= w || p.py >= h) return false;
    p.k = (size_t)p.py * (size_t)w + (size_t)p.px;
    return true;
}

// A guide point {x, y, z, object bits} is finite and its object is marked in `table` (the reusable
// or the through table), which is read only for an object index inside it.
__device__ __forceinline__ bool ga_marked_point(const float4& P, int n_objects, const uint8_t* __restrict__ table) {
    const int o = __float_as_int(P.w);
    bool ok = o >= 0 && o < n_objects && ga_finite(P.x) && ga_finite(P.y) && ga_finite(P.z);
    if (ok) ok = table[o] != 0;
    return ok;
}

// The point (x, y, z) projected into the older view A.view, then its 2 x 2 bilinear taps, dy outer
// and dx inner: tap(q, b) is called for each tap inside the older image and inside the history's
// region (A.px0, A.py0, A.pw, A.ph), with its region-packed index q and its bilinear weight b.
// Nothing is called when the projection is not finite, behind the view or outside the image.
template <class Args, class Tap>
__device__ __forceinline__ void ga_taps(const Args& A, float x, float y, float z, Tap tap) {
    const RpView& V = A.view;
    const float dx_ = x - V.c[0], dy_ = y - V.c[1], dz_ = z - V.c[2];
    const float s = V.aw / ga_dot(dx_, dy_, dz_, V.w[0], V.w[1], V.w[2]);
    const float qx = dx_ * s - V.a[0], qy = dy_ * s - V.a[1], qz = dz_ * s - V.a[2];
    const float fi = ga_dot(qx, qy, qz, V.du[0], V.du[1], V.du[2]) * V.iu;
    const float fj = ga_dot(qx, qy, qz, V.dv[0], V.dv[1], V.dv[2]) * V.iv;
    // (every comparison is false for a NaN)
    const bool valid = ga_finite(s) && s > 0.0f && ga_finite(fi) && ga_finite(fj) && fi > -1.0f &&
                       fi < (float)V.width && fj > -1.0f && fj < (float)V.height;
    if (!valid) return;
    const float fi0 = floorf(fi), fj0 = floorf(fj);
    const int i0 = (int)fi0, j0 = (int)fj0;
    const float ax = fi - fi0, ay = fj - fj0;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
            const int ti = i0 + dx, tj = j0 + dy;
            if (ti < 0 || ti >= V.width || tj < 0 || tj >= V.height) continue;
            const int ri = ti - A.px0, rj = tj - A.py0;
            if (ri < 0 || ri >= A.pw || rj < 0 || rj >= A.ph) continue;
            tap((size_t)rj * (size_t)A.pw + (size_t)ri, (dx ? ax : 1.0f - ax) * (dy ? ay : 1.0f - ay));
        }
    }
}

// The first-hit tap test: the tap's guides {nq, Pq} show the pixel's surface {n, P} - equal object
// bits, the normals within normal_min, the tap's point within `plane` of the pixel's plane.
__device__ __forceinline__ bool ga_same_surface(const float4& n, const float4& P, float plane, float normal_min,
                                                const float4& nq, const float4& Pq) {
    const float dn = ga_dot(n.x, n.y, n.z, nq.x, nq.y, nq.z);
    const float e = ga_dot(n.x, n.y, n.z, Pq.x - P.x, Pq.y - P.y, Pq.z - P.z);
    return __float_as_int(Pq.w) == __float_as_int(P.w) && dn >= normal_min && fabsf(e) <= plane;
}

// What a tap's colour must be to count. The reprojection: the pack pass's finite flag in cq.w. The
// accumulation: cq = {r, g, b, length} holds a history - all finite and the length > 0 (a pixel
// that never held a sample is not history).
__device__ __forceinline__ bool ga_flagged(const float4& cq) { return cq.w != 0.0f; }
__device__ __forceinline__ bool ga_holds_history(const float4& cq) {
    return ga_finite(cq.x) && ga_finite(cq.y) && ga_finite(cq.z) && ga_finite(cq.w) && cq.w > 0.0f;
}

// A pixel of the chain kernels. spec (k = ch & 0xff >= 1): it tests taps on the chain's guides,
// else on the first hit's: {n, P with the object bits} are the ones it uses. o1 / ch: its first
// object and chain word. X: where it looks for its history - the first hit, or for a chain the
// point at the summed path length along the primary ray. The bounds of the tap tests:
// plane = sigma_plane Ds, point = (pp2 Ds) Ds.
struct GaChainPixel {
    float4 n, P;
    int32_t o1, ch;
    bool spec, valid;
    float X[3];
    float plane, point;
};

// The chain pixel at k of the new view's guides N. It is valid where `has_history`, P is finite
// and its object reusable; a chain pixel also needs `chain_ok`, a chain that ends on a surface
// (end code 1), finite path lengths and a first hit on an object chains may start on.
template <class Args>
__device__ __forceinline__ GaChainPixel ga_chain_pixel(const Args& A, const RsGuides& N, size_t k, bool has_history,
                                                       bool chain_ok, const uint8_t* __restrict__ reusable,
                                                       const uint8_t* __restrict__ through) {
    GaChainPixel p;
    p.ch = N.chain[k];
    p.spec = (p.ch & 0xff) >= 1;  // per lane: the chain's guides, or the first hit's
    const float4 n1 = N.gn[k], P1 = N.gp[k];
    p.n = p.spec ? N.sgn[k] : n1;
    p.P = p.spec ? N.sgp[k] : P1;
    p.o1 = __float_as_int(P1.w);
    p.valid = has_history && ga_marked_point(p.P, A.n_objects, reusable);
    p.X[0] = P1.x, p.X[1] = P1.y, p.X[2] = P1.z;
    if (p.spec) {
        p.valid = p.valid && chain_ok && ((p.ch >> 8) & 0xff) == 1 && ga_finite(p.n.w) && ga_finite(n1.w) &&
                  n1.w > 0.0f && ga_marked_point(P1, A.n_objects, through);
        // the point at the summed path length along the primary ray
        const float r = p.n.w / n1.w;
        p.X[0] = A.cn[0] + (P1.x - A.cn[0]) * r;
        p.X[1] = A.cn[1] + (P1.y - A.cn[1]) * r;
        p.X[2] = A.cn[2] + (P1.z - A.cn[2]) * r;
    }
    p.plane = A.sigma_plane * p.n.w;
    p.point = (A.pp2 * p.n.w) * p.n.w;
    return p;
}

// The tap test of a chain pixel: the previous pixel walked the same chain (equal chain word, first
// and last object) and its chain guides {nq, Pq} show the same surface point - ga_same_surface on
// the chain guides, and the point check |Pq - P|^2 <= point. pfirst: the previous first-hit gp.
// (every comparison is false for a NaN)
__device__ __forceinline__ bool ga_chain_same_surface(const GaChainPixel& p, float normal_min, const float4& pfirst,
                                                      const float4& nq, const float4& Pq, int32_t chq) {
    const float ex = Pq.x - p.P.x, ey = Pq.y - p.P.y, ez = Pq.z - p.P.z;
    const float dn = ga_dot(p.n.x, p.n.y, p.n.z, nq.x, nq.y, nq.z);
    const float e = ga_dot(p.n.x, p.n.y, p.n.z, ex, ey, ez);
    const float qq = ga_dot(ex, ey, ez, ex, ey, ez);
    // `&`, not `&&`: the chain word and the first object are two 4-byte loads that are waited for
    // together; with `&&` the compiler gives each a load, a wait and a branch of its own, one
    // memory round trip more per chain tap
    const bool same_start = (chq == p.ch) & (__float_as_int(pfirst.w) == p.o1);
    return same_start && __float_as_int(Pq.w) == __float_as_int(p.P.w) && dn >= normal_min && fabsf(e) <= p.plane &&
           qq <= p.point;
}

// The reprojection's result from its four sums: {history.rgb, weight}, zero below min_weight.
__device__ __forceinline__ float4 ga_history(float ws, float ar, float ag, float ab, float min_weight) {
    const float weight = ws >= min_weight ? ws : 0.0f;
    float4 hv = make_float4(0.0f, 0.0f, 0.0f, weight);
    if (weight > 0.0f) {
        hv.x = ar / ws;
        hv.y = ag / ws;
        hv.z = ab / ws;
    }
    return hv;
}

// The reprojection blend into ov.rgb (ov.w is the caller's): the fresh colour of pixel (px, py),
// blended where hv holds a history as if that held A.nh samples against the pixel's m fresh ones;
// the history alone where the fresh colour is not finite or m is 0. `fresh` is not null.
template <class Args>
__device__ __forceinline__ void ga_reproject_blend(const Args& A, const GaPixel& p, const float4& hv,
                                                   const float* __restrict__ fresh,
                                                   const int32_t* __restrict__ px_samples, float4& ov) {
    const size_t f = (size_t)(A.fy0 + p.py) * (size_t)A.pitch + (size_t)(A.fx0 + p.px);
    const float cr = fresh[3 * f], cg = fresh[3 * f + 1], cb = fresh[3 * f + 2];
    ov.x = cr;
    ov.y = cg;
    ov.z = cb;
    if (hv.w > 0.0f) {
        const float m = px_samples ? (float)px_samples[f] : A.m;
        if (ga_finite(cr) && ga_finite(cg) && ga_finite(cb) && m > 0.0f) {
            const float den = A.nh + m;
            ov.x = (hv.x * A.nh + cr * m) / den;
            ov.y = (hv.y * A.nh + cg * m) / den;
            ov.z = (hv.z * A.nh + cb * m) / den;
        } else {
            ov.x = hv.x;
            ov.y = hv.y;
            ov.z = hv.z;
        }
    }
}

// The accumulation blend from its six sums: oc = {out.rgb, Lout}, ov = Vout; returns the weight
// (zero below A.min_weight). The gathered length is clamped to A.max_history and blended with the
// m fresh samples of pixel (px, py) by the counts, the variances by the squared shares.
template <class Args>
__device__ __forceinline__ float ga_accumulate_blend(const Args& A, const GaPixel& p, float ws, float ar, float ag,
                                                     float ab, float av, float al, const float* __restrict__ fresh,
                                                     const int32_t* __restrict__ px_samples,
                                                     const float* __restrict__ variance, float4& oc, float& ov) {
    const float weight = ws >= A.min_weight ? ws : 0.0f;
    const size_t f = (size_t)(A.fy0 + p.py) * (size_t)A.pitch + (size_t)(A.fx0 + p.px);
    const float cr = fresh[3 * f], cg = fresh[3 * f + 1], cb = fresh[3 * f + 2];
    const float m = px_samples ? (float)px_samples[f] : A.m;
    const float v = ga_variance(variance[(size_t)(A.vy0 + p.py) * (size_t)A.vpitch + (size_t)(A.vx0 + p.px)]);
    const bool cfin = ga_finite(cr) && ga_finite(cg) && ga_finite(cb);
    oc = make_float4(cr, cg, cb, cfin ? m : 0.0f);
    ov = v;
    if (weight > 0.0f) {
        const float hr = ar / ws, hg = ag / ws, hb = ab / ws, vh = av / ws, lh = al / ws;
        const float N = fminf(lh, A.max_history);
        if (cfin && m > 0.0f) {
            const float den = N + m;
            oc.x = (hr * N + cr * m) / den;
            oc.y = (hg * N + cg * m) / den;
            oc.z = (hb * N + cb * m) / den;
            oc.w = den;
            const float g = N / den, a = m / den;
            ov = (g * g) * vh + (a * a) * v;
        } else {
            oc = make_float4(hr, hg, hb, N);
            ov = vh;
        }
    }
    return weight;
}

}  // namespace rt
#endif
