// The accumulation gather and blend through specular chains (temporal_spec.hpp). Compiled as
// temporal.hip: -ffp-contract=off and no fast-math, denormal-flushing or approximate-reciprocal
// flag, so every fp32 operation (add, subtract, multiply, IEEE divide, floor, min) has exactly one
// result, and the tap order and the multiply-then-add accumulation are part of it -
// tests/specular_temporal_ref.py is the definition. The projection arithmetic is
// reproject_kernel's, copied as in the sibling units.
#include "temporal_spec.hpp"

namespace rt {

constexpr int kTsBlock = 256;
constexpr int kTsRow = 64;  // a workgroup is 4 rows of 64 pixels, as temporal_kernel

__global__ __launch_bounds__(kTsBlock) void temporal_spec_kernel(TsArgs A, RsGuides N, TsHistory Q,
                                                                 const uint8_t* __restrict__ reusable,
                                                                 const uint8_t* __restrict__ through,
                                                                 const float* __restrict__ fresh,
                                                                 const int32_t* __restrict__ px_samples,
                                                                 const float* __restrict__ variance,
                                                                 float4* __restrict__ ocol, float* __restrict__ ovar,
                                                                 float* __restrict__ oweight,
                                                                 uint8_t* __restrict__ okind) {
    const int px = blockIdx.x * kTsRow + (int)(threadIdx.x & (kTsRow - 1));
    const int py = blockIdx.y * (kTsBlock / kTsRow) + (int)(threadIdx.x / kTsRow);
    if (px >= A.w || py >= A.h) return;
    const size_t k = (size_t)py * (size_t)A.w + (size_t)px;
    const int32_t ch = N.chain[k];
    const bool spec = (ch & 0xff) >= 1;  // per lane: the chain's guides, or the first hit's
    const float4 n1 = N.gn[k], P1 = N.gp[k];
    const float4 n = spec ? N.sgn[k] : n1, P = spec ? N.sgp[k] : P1;
    const RpView& V = A.view;
    const int o = __float_as_int(P.w), o1 = __float_as_int(P1.w);
    float ws = 0.0f, ar = 0.0f, ag = 0.0f, ab = 0.0f, av = 0.0f, al = 0.0f;
    bool valid = A.pw > 0 && o >= 0 && o < A.n_objects && rs_finite(P.x) && rs_finite(P.y) && rs_finite(P.z);
    if (valid) valid = reusable[o] != 0;
    float X[3] = {P1.x, P1.y, P1.z};
    if (spec) {
        valid = valid && A.chain_history != 0 && ((ch >> 8) & 0xff) == 1 && o1 >= 0 && o1 < A.n_objects &&
                rs_finite(P1.x) && rs_finite(P1.y) && rs_finite(P1.z) && rs_finite(n.w) && rs_finite(n1.w) && n1.w > 0.0f;
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
                    const float4 cq = Q.col[q];
                    const float vraw = Q.var[q];
                    bool ok;
                    if (spec) {
                        // with cq and vraw: four 16-byte loads and two 4-byte loads, issued together
                        // before the tests
                        const float4 pf = Q.g.gp[q], nq = Q.g.sgn[q], Pq = Q.g.sgp[q];
                        const int32_t chq = Q.g.chain[q];
                        ok = ts_chain_tap_counts(cp, A.normal_min, pf, nq, Pq, cq, chq);
                    } else {
                        const float4 nq = Q.g.gn[q], Pq = Q.g.gp[q];
                        const float dn = rs_dot(n.x, n.y, n.z, nq.x, nq.y, nq.z);
                        const float e = rs_dot(n.x, n.y, n.z, Pq.x - P.x, Pq.y - P.y, Pq.z - P.z);
                        // cq.w is the tap's history length: a pixel that never held a sample is not history
                        ok = __float_as_int(Pq.w) == o && rs_finite(cq.x) && rs_finite(cq.y) && rs_finite(cq.z) &&
                             dn >= A.normal_min && fabsf(e) <= plane && rs_finite(cq.w) && cq.w > 0.0f;
                    }
                    const float vq = ts_variance(vraw);
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
    const float v = ts_variance(variance[(size_t)(A.vy0 + py) * (size_t)A.vpitch + (size_t)(A.vx0 + px)]);
    const bool cfin = rs_finite(cr) && rs_finite(cg) && rs_finite(cb);
    float4 oc = make_float4(cr, cg, cb, cfin ? m : 0.0f);
    float ov = v;
    if (weight > 0.0f) {
        const float hr = ar / ws, hg = ag / ws, hb = ab / ws, vh = av / ws, lh = al / ws;
        const float L = fminf(lh, A.max_history);
        if (cfin && m > 0.0f) {
            const float den = L + m;
            oc.x = (hr * L + cr * m) / den;
            oc.y = (hg * L + cg * m) / den;
            oc.z = (hb * L + cb * m) / den;
            oc.w = den;
            const float g = L / den, a = m / den;
            ov = (g * g) * vh + (a * a) * v;
        } else {
            oc = make_float4(hr, hg, hb, L);
            ov = vh;
        }
    }
    ocol[k] = oc;
    ovar[k] = ov;
    oweight[k] = weight;
    okind[k] = weight > 0.0f ? (spec ? (uint8_t)2 : (uint8_t)1) : (uint8_t)0;
}

hipError_t launch_temporal_spec(const TsArgs& a, const RsGuides& nw, const TsHistory& hist, const uint8_t* reusable,
                                const uint8_t* through, const float* fresh, const int32_t* px_samples,
                                const float* variance, const TpOut& out, uint8_t* kind, hipStream_t stream) {
    if (a.w < 0 || a.h < 0 || a.pw < 0 || a.ph < 0 || a.n_objects < 0 || a.pitch < 0 || a.fx0 < 0 || a.fy0 < 0 ||
        a.vpitch < 0 || a.vx0 < 0 || a.vy0 < 0)
        return hipErrorInvalidValue;
    if (a.w == 0 || a.h == 0) return hipSuccess;
    if (!nw.gn || !nw.gp || !nw.sgn || !nw.sgp || !nw.chain || !fresh || !variance || !out.col || !out.var ||
        !out.weight || !kind)
        return hipErrorInvalidValue;
    if (a.pw > 0) {
        if (a.ph <= 0 || !hist.g.gn || !hist.g.gp || !hist.col || !hist.var || !reusable || !through)
            return hipErrorInvalidValue;
        if (a.chain_history && (!hist.g.sgn || !hist.g.sgp || !hist.g.chain)) return hipErrorInvalidValue;
    }
    const dim3 grid((unsigned)((a.w + kTsRow - 1) / kTsRow),
                    (unsigned)((a.h + kTsBlock / kTsRow - 1) / (kTsBlock / kTsRow)));
    hipLaunchKernelGGL(temporal_spec_kernel, grid, dim3(kTsBlock), 0, stream, a, nw, hist, reusable, through, fresh,
                       px_samples, variance, out.col, out.var, out.weight, kind);
    return hipGetLastError();
}

}  // namespace rt
