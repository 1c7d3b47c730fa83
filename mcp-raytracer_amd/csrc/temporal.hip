// The accumulation gather and blend (temporal.hpp). Compiled with -ffp-contract=off and without
// any fast-math, denormal-flushing or approximate-reciprocal flag: every fp32 operation (add,
// subtract, multiply, IEEE divide, floor, min) has exactly one result, and the tap order and the
// multiply-then-add accumulation are part of it - tests/temporal_ref.py is the definition. The
// projection arithmetic is reproject_kernel's, copied so that unit stays as it is.
#include "temporal.hpp"

namespace rt {

constexpr int kTpBlock = 256;
constexpr int kTpRow = 64;  // a workgroup is 4 rows of 64 pixels, as reproject_kernel

__device__ __forceinline__ bool tp_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ float tp_dot(float ax, float ay, float az, float bx, float by, float bz) {
    return (ax * bx + ay * by) + az * bz;
}
// the variance filter's rule: not (v >= 0 and finite) -> 0
__device__ __forceinline__ float tp_variance(float v) { return v >= 0.0f && tp_finite(v) ? v : 0.0f; }

__global__ __launch_bounds__(kTpBlock) void temporal_kernel(TpArgs A, const float4* __restrict__ gn,
                                                            const float4* __restrict__ gp,
                                                            const float4* __restrict__ pgn,
                                                            const float4* __restrict__ pgp,
                                                            const float4* __restrict__ pcol,
                                                            const float* __restrict__ pvar,
                                                            const uint8_t* __restrict__ reusable,
                                                            const float* __restrict__ fresh,
                                                            const int32_t* __restrict__ px_samples,
                                                            const float* __restrict__ variance,
                                                            float4* __restrict__ ocol, float* __restrict__ ovar,
                                                            float* __restrict__ oweight) {
    const int px = blockIdx.x * kTpRow + (int)(threadIdx.x & (kTpRow - 1));
    const int py = blockIdx.y * (kTpBlock / kTpRow) + (int)(threadIdx.x / kTpRow);
    if (px >= A.w || py >= A.h) return;
    const size_t k = (size_t)py * (size_t)A.w + (size_t)px;
    const float4 n = gn[k], P = gp[k];
    const RpView& V = A.view;
    const int o = __float_as_int(P.w);
    float ws = 0.0f, ar = 0.0f, ag = 0.0f, ab = 0.0f, av = 0.0f, al = 0.0f;
    bool valid = A.pw > 0 && o >= 0 && o < A.n_objects && tp_finite(P.x) && tp_finite(P.y) && tp_finite(P.z);
    if (valid) valid = reusable[o] != 0;
    if (valid) {
        const float dx_ = P.x - V.c[0], dy_ = P.y - V.c[1], dz_ = P.z - V.c[2];
        const float s = V.aw / tp_dot(dx_, dy_, dz_, V.w[0], V.w[1], V.w[2]);
        const float qx = dx_ * s - V.a[0], qy = dy_ * s - V.a[1], qz = dz_ * s - V.a[2];
        const float fi = tp_dot(qx, qy, qz, V.du[0], V.du[1], V.du[2]) * V.iu;
        const float fj = tp_dot(qx, qy, qz, V.dv[0], V.dv[1], V.dv[2]) * V.iv;
        // (every comparison is false for a NaN)
        valid = tp_finite(s) && s > 0.0f && tp_finite(fi) && tp_finite(fj) && fi > -1.0f && fi < (float)V.width &&
                fj > -1.0f && fj < (float)V.height;
        if (valid) {
            const float fi0 = floorf(fi), fj0 = floorf(fj);
            const int i0 = (int)fi0, j0 = (int)fj0;
            const float ax = fi - fi0, ay = fj - fj0;
            const float plane = A.sigma_plane * n.w;
#pragma unroll
            for (int dy = 0; dy < 2; ++dy) {
#pragma unroll
                for (int dx = 0; dx < 2; ++dx) {
                    const int ti = i0 + dx, tj = j0 + dy;
                    if (ti < 0 || ti >= V.width || tj < 0 || tj >= V.height) continue;
                    const int ri = ti - A.px0, rj = tj - A.py0;
                    if (ri < 0 || ri >= A.pw || rj < 0 || rj >= A.ph) continue;
                    const size_t q = (size_t)rj * (size_t)A.pw + (size_t)ri;
                    const float4 nq = pgn[q], Pq = pgp[q], cq = pcol[q];
                    const float vq = tp_variance(pvar[q]);
                    const float b = (dx ? ax : 1.0f - ax) * (dy ? ay : 1.0f - ay);
                    const float dn = tp_dot(n.x, n.y, n.z, nq.x, nq.y, nq.z);
                    const float e = tp_dot(n.x, n.y, n.z, Pq.x - P.x, Pq.y - P.y, Pq.z - P.z);
                    // cq.w is the tap's history length: a pixel that never held a sample is not history
                    const bool ok = __float_as_int(Pq.w) == o && tp_finite(cq.x) && tp_finite(cq.y) && tp_finite(cq.z) &&
                                    dn >= A.normal_min && fabsf(e) <= plane && tp_finite(cq.w) && cq.w > 0.0f;
                    ws = ws + (ok ? b : 0.0f);
                    ar = ar + (ok ? b * cq.x : 0.0f);
                    ag = ag + (ok ? b * cq.y : 0.0f);
                    ab = ab + (ok ? b * cq.z : 0.0f);
                    av = av + (ok ? b * vq : 0.0f);
                    al = al + (ok ? b * cq.w : 0.0f);
                }
            }
        }
    }
    const float weight = ws >= A.min_weight ? ws : 0.0f;
    const size_t f = (size_t)(A.fy0 + py) * (size_t)A.pitch + (size_t)(A.fx0 + px);
    const float cr = fresh[3 * f], cg = fresh[3 * f + 1], cb = fresh[3 * f + 2];
    const float m = px_samples ? (float)px_samples[f] : A.m;
    const float v = tp_variance(variance[(size_t)(A.vy0 + py) * (size_t)A.vpitch + (size_t)(A.vx0 + px)]);
    const bool cfin = tp_finite(cr) && tp_finite(cg) && tp_finite(cb);
    float4 oc = make_float4(cr, cg, cb, cfin ? m : 0.0f);
    float ov = v;
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
    ocol[k] = oc;
    ovar[k] = ov;
    oweight[k] = weight;
}

__global__ __launch_bounds__(kTpBlock) void temporal_pack_kernel(const float* __restrict__ rad,
                                                                 const float* __restrict__ length, int n,
                                                                 float4* __restrict__ col) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    col[k] = make_float4(rad[3 * (size_t)k], rad[3 * (size_t)k + 1], rad[3 * (size_t)k + 2], length[k]);
}

hipError_t launch_temporal(const TpArgs& a, const float4* gn, const float4* gp, const TpHistory& hist,
                           const uint8_t* reusable, const float* fresh, const int32_t* px_samples, const float* variance,
                           const TpOut& out, hipStream_t stream) {
    if (a.w <= 0 || a.h <= 0) return hipSuccess;
    if (!gn || !gp || !fresh || !variance || !out.col || !out.var || !out.weight || a.pw < 0 || a.ph < 0)
        return hipErrorInvalidValue;
    if (a.pw > 0 && (a.ph <= 0 || !hist.gn || !hist.gp || !hist.col || !hist.var || !reusable)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((a.w + kTpRow - 1) / kTpRow),
                    (unsigned)((a.h + kTpBlock / kTpRow - 1) / (kTpBlock / kTpRow)));
    hipLaunchKernelGGL(temporal_kernel, grid, dim3(kTpBlock), 0, stream, a, gn, gp, hist.gn, hist.gp, hist.col, hist.var,
                       reusable, fresh, px_samples, variance, out.col, out.var, out.weight);
    return hipGetLastError();
}

hipError_t launch_temporal_pack(const float* rad, const float* length, int n, float4* col, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(temporal_pack_kernel, dim3((unsigned)((n + kTpBlock - 1) / kTpBlock)), dim3(kTpBlock), 0, stream,
                       rad, length, n, col);
    return hipGetLastError();
}

}  // namespace rt
