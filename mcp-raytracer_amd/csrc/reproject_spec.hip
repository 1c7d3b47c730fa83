// The reprojection gather through specular chains (reproject_spec.hpp). Compiled as reproject.hip:
// -ffp-contract=off and no fast-math, denormal-flushing or approximate-reciprocal flag, so every
// fp32 operation (add, subtract, multiply, IEEE divide, floor) has exactly one result, and the tap
// order and the multiply-then-add accumulation are part of it - tests/specular_reproject_ref.py is
// the definition.
#include "reproject_spec.hpp"

namespace rt {

constexpr int kRsBlock = 256;
constexpr int kRsRow = 64;  // a workgroup is 4 rows of 64 pixels, as reproject_kernel

__global__ __launch_bounds__(kRsBlock) void reproject_spec_kernel(RsArgs A, RsGuides N, RsGuides Q,
                                                                  const float4* __restrict__ pcol,
                                                                  const uint8_t* __restrict__ reusable,
                                                                  const uint8_t* __restrict__ through,
                                                                  const float* __restrict__ fresh,
                                                                  const int32_t* __restrict__ px_samples,
                                                                  float4* __restrict__ hist, float4* __restrict__ outc) {
    const int px = blockIdx.x * kRsRow + (int)(threadIdx.x & (kRsRow - 1));
    const int py = blockIdx.y * (kRsBlock / kRsRow) + (int)(threadIdx.x / kRsRow);
    if (px >= A.w || py >= A.h) return;
    const size_t k = (size_t)py * (size_t)A.w + (size_t)px;
    const int32_t ch = N.chain[k];
    const bool spec = (ch & 0xff) >= 1;  // per lane: the chain's guides, or the first hit's
    const float4 n1 = N.gn[k], P1 = N.gp[k];
    const float4 n = spec ? N.sgn[k] : n1, P = spec ? N.sgp[k] : P1;
    const RpView& V = A.view;
    const int o = __float_as_int(P.w), o1 = __float_as_int(P1.w);
    float ws = 0.0f, ar = 0.0f, ag = 0.0f, ab = 0.0f;
    bool valid = o >= 0 && o < A.n_objects && rs_finite(P.x) && rs_finite(P.y) && rs_finite(P.z);
    if (valid) valid = reusable[o] != 0;
    float X[3] = {P1.x, P1.y, P1.z};
    if (spec) {
        valid = valid && ((ch >> 8) & 0xff) == 1 && o1 >= 0 && o1 < A.n_objects && rs_finite(P1.x) && rs_finite(P1.y) &&
                rs_finite(P1.z) && rs_finite(n.w) && rs_finite(n1.w) && n1.w > 0.0f;
        if (valid) valid = through[o1] != 0;
        // the point at the summed path length along the primary ray
        const float r = n.w / n1.w;
        X[0] = A.cn[0] + (P1.x - A.cn[0]) * r;
        X[1] = A.cn[1] + (P1.y - A.cn[1]) * r;
        X[2] = A.cn[2] + (P1.z - A.cn[2]) * r;
    }
    if (valid) {
        const float dx_ = X[0] - V.c[0], dy_ = X[1] - V.c[1], dz_ = X[2] - V.c[2];
        const float s = V.aw / rs_dot(dx_, dy_, dz_, V.w[0], V.w[1], V.w[2]);
        const float qx = dx_ * s - V.a[0], qy = dy_ * s - V.a[1], qz = dz_ * s - V.a[2];
        const float fi = rs_dot(qx, qy, qz, V.du[0], V.du[1], V.du[2]) * V.iu;
        const float fj = rs_dot(qx, qy, qz, V.dv[0], V.dv[1], V.dv[2]) * V.iv;
        // (every comparison is false for a NaN)
        valid = rs_finite(s) && s > 0.0f && rs_finite(fi) && rs_finite(fj) && fi > -1.0f && fi < (float)V.width &&
                fj > -1.0f && fj < (float)V.height;
        if (valid) {
            const float fi0 = floorf(fi), fj0 = floorf(fj);
            const int i0 = (int)fi0, j0 = (int)fj0;
            const float ax = fi - fi0, ay = fj - fj0;
            const float plane = A.sigma_plane * n.w;
            const RsChainPixel cp{n, P, o1, ch, plane, (A.pp2 * n.w) * n.w};
#pragma unroll
            for (int dy = 0; dy < 2; ++dy) {
#pragma unroll
                for (int dx = 0; dx < 2; ++dx) {
                    const int ti = i0 + dx, tj = j0 + dy;
                    if (ti < 0 || ti >= V.width || tj < 0 || tj >= V.height) continue;
                    const int ri = ti - A.px0, rj = tj - A.py0;
                    if (ri < 0 || ri >= A.pw || rj < 0 || rj >= A.ph) continue;
                    const size_t q = (size_t)rj * (size_t)A.pw + (size_t)ri;
                    const float b = (dx ? ax : 1.0f - ax) * (dy ? ay : 1.0f - ay);
                    const float4 cq = pcol[q];
                    bool ok;
                    if (spec) {
                        // four 16-byte loads and one 4-byte load, issued together before the tests
                        const float4 pf = Q.gp[q], nq = Q.sgn[q], Pq = Q.sgp[q];
                        const int32_t chq = Q.chain[q];
                        ok = rs_chain_tap_counts(cp, A.normal_min, pf, nq, Pq, cq, chq);
                    } else {
                        const float4 nq = Q.gn[q], Pq = Q.gp[q];
                        const float dn = rs_dot(n.x, n.y, n.z, nq.x, nq.y, nq.z);
                        const float e = rs_dot(n.x, n.y, n.z, Pq.x - P.x, Pq.y - P.y, Pq.z - P.z);
                        ok = __float_as_int(Pq.w) == o && cq.w != 0.0f && dn >= A.normal_min && fabsf(e) <= plane;
                    }
                    ws = ws + (ok ? b : 0.0f);
                    ar = ar + (ok ? b * cq.x : 0.0f);
                    ag = ag + (ok ? b * cq.y : 0.0f);
                    ab = ab + (ok ? b * cq.z : 0.0f);
                }
            }
        }
    }
    const float weight = ws >= A.min_weight ? ws : 0.0f;
    float4 hv = make_float4(0.0f, 0.0f, 0.0f, weight);
    if (weight > 0.0f) {
        hv.x = ar / ws;
        hv.y = ag / ws;
        hv.z = ab / ws;
    }
    hist[k] = hv;
    float4 ov = make_float4(0.0f, 0.0f, 0.0f, weight > 0.0f ? (spec ? 2.0f : 1.0f) : 0.0f);
    if (fresh) {
        const size_t f = (size_t)(A.fy0 + py) * (size_t)A.pitch + (size_t)(A.fx0 + px);
        const float cr = fresh[3 * f], cg = fresh[3 * f + 1], cb = fresh[3 * f + 2];
        ov.x = cr;
        ov.y = cg;
        ov.z = cb;
        if (weight > 0.0f) {
            const float m = px_samples ? (float)px_samples[f] : A.m;
            if (rs_finite(cr) && rs_finite(cg) && rs_finite(cb) && m > 0.0f) {
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
    outc[k] = ov;
}

__global__ __launch_bounds__(kRsBlock) void reproject_spec_kind_kernel(const float4* __restrict__ outc, int n,
                                                                       uint8_t* __restrict__ kind) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) kind[k] = (uint8_t)(int)outc[k].w;
}

hipError_t launch_reproject_spec(const RsArgs& a, const RsGuides& nw, const RsGuides& pv, const float4* pcol,
                                 const uint8_t* reusable, const uint8_t* through, const float* fresh,
                                 const int32_t* px_samples, float4* hist, float4* outc, hipStream_t stream) {
    if (a.w <= 0 || a.h <= 0) return hipSuccess;
    if (a.pw <= 0 || a.ph <= 0 || !hist || !outc || !reusable || !through || !pcol) return hipErrorInvalidValue;
    for (const RsGuides* g : {&nw, &pv})
        if (!g->gn || !g->gp || !g->sgn || !g->sgp || !g->chain) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((a.w + kRsRow - 1) / kRsRow),
                    (unsigned)((a.h + kRsBlock / kRsRow - 1) / (kRsBlock / kRsRow)));
    hipLaunchKernelGGL(reproject_spec_kernel, grid, dim3(kRsBlock), 0, stream, a, nw, pv, pcol, reusable, through, fresh,
                       px_samples, hist, outc);
    return hipGetLastError();
}

hipError_t launch_reproject_spec_kind(const float4* outc, int n, uint8_t* kind, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    if (!outc || !kind) return hipErrorInvalidValue;
    hipLaunchKernelGGL(reproject_spec_kind_kernel, dim3((unsigned)((n + kRsBlock - 1) / kRsBlock)), dim3(kRsBlock), 0,
                       stream, outc, n, kind);
    return hipGetLastError();
}

}  // namespace rt
