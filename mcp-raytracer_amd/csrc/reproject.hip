// The reprojection gather (reproject.hpp). Compiled with -ffp-contract=off and without any
// fast-math, denormal-flushing or approximate-reciprocal flag: every fp32 operation (add,
// subtract, multiply, IEEE divide, floor) has exactly one result, and the tap order and the
// multiply-then-add accumulation are part of it - tests/reproject_ref.py is the definition.
#include "reproject.hpp"

namespace rt {

constexpr int kRpBlock = 256;
constexpr int kRpRow = 64;  // a workgroup is 4 rows of 64 pixels, as denoise_global_kernel

__device__ __forceinline__ bool rp_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ float rp_dot(float ax, float ay, float az, float bx, float by, float bz) {
    return (ax * bx + ay * by) + az * bz;
}

__global__ __launch_bounds__(kRpBlock) void reproject_kernel(RpArgs A, const float4* __restrict__ gn,
                                                             const float4* __restrict__ gp,
                                                             const float4* __restrict__ pgn,
                                                             const float4* __restrict__ pgp,
                                                             const float4* __restrict__ pcol,
                                                             const uint8_t* __restrict__ reusable,
                                                             const float* __restrict__ fresh,
                                                             const int32_t* __restrict__ px_samples,
                                                             float4* __restrict__ hist, float4* __restrict__ outc) {
    const int px = blockIdx.x * kRpRow + (int)(threadIdx.x & (kRpRow - 1));
    const int py = blockIdx.y * (kRpBlock / kRpRow) + (int)(threadIdx.x / kRpRow);
    if (px >= A.w || py >= A.h) return;
    const size_t k = (size_t)py * (size_t)A.w + (size_t)px;
    const float4 n = gn[k], P = gp[k];
    const RpView& V = A.view;
    const int o = __float_as_int(P.w);
    float ws = 0.0f, ar = 0.0f, ag = 0.0f, ab = 0.0f;
    bool valid = o >= 0 && o < A.n_objects && rp_finite(P.x) && rp_finite(P.y) && rp_finite(P.z);
    if (valid) valid = reusable[o] != 0;
    if (valid) {
        const float dx_ = P.x - V.c[0], dy_ = P.y - V.c[1], dz_ = P.z - V.c[2];
        const float s = V.aw / rp_dot(dx_, dy_, dz_, V.w[0], V.w[1], V.w[2]);
        const float qx = dx_ * s - V.a[0], qy = dy_ * s - V.a[1], qz = dz_ * s - V.a[2];
        const float fi = rp_dot(qx, qy, qz, V.du[0], V.du[1], V.du[2]) * V.iu;
        const float fj = rp_dot(qx, qy, qz, V.dv[0], V.dv[1], V.dv[2]) * V.iv;
        // (every comparison is false for a NaN)
        valid = rp_finite(s) && s > 0.0f && rp_finite(fi) && rp_finite(fj) && fi > -1.0f && fi < (float)V.width &&
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
                    const float b = (dx ? ax : 1.0f - ax) * (dy ? ay : 1.0f - ay);
                    const float dn = rp_dot(n.x, n.y, n.z, nq.x, nq.y, nq.z);
                    const float e = rp_dot(n.x, n.y, n.z, Pq.x - P.x, Pq.y - P.y, Pq.z - P.z);
                    const bool ok = __float_as_int(Pq.w) == o && cq.w != 0.0f && dn >= A.normal_min && fabsf(e) <= plane;
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
    if (!fresh) return;
    const size_t f = (size_t)(A.fy0 + py) * (size_t)A.pitch + (size_t)(A.fx0 + px);
    const float cr = fresh[3 * f], cg = fresh[3 * f + 1], cb = fresh[3 * f + 2];
    float4 ov = make_float4(cr, cg, cb, 0.0f);
    if (weight > 0.0f) {
        const float m = px_samples ? (float)px_samples[f] : A.m;
        if (rp_finite(cr) && rp_finite(cg) && rp_finite(cb) && m > 0.0f) {
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
    outc[k] = ov;
}

hipError_t launch_reproject(const RpArgs& a, const float4* gn, const float4* gp, const float4* pgn, const float4* pgp,
                            const float4* pcol, const uint8_t* reusable, const float* fresh, const int32_t* px_samples,
                            float4* hist, float4* outc, hipStream_t stream) {
    if (a.w <= 0 || a.h <= 0) return hipSuccess;
    if (a.pw <= 0 || a.ph <= 0 || !hist || (fresh && !outc)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((a.w + kRpRow - 1) / kRpRow),
                    (unsigned)((a.h + kRpBlock / kRpRow - 1) / (kRpBlock / kRpRow)));
    hipLaunchKernelGGL(reproject_kernel, grid, dim3(kRpBlock), 0, stream, a, gn, gp, pgn, pgp, pcol, reusable, fresh,
                       px_samples, hist, outc);
    return hipGetLastError();
}

}  // namespace rt
