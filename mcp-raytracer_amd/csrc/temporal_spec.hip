// The accumulation gather and blend through specular chains (temporal_spec.hpp). Compiled as
// temporal.hip: -ffp-contract=off and no fast-math, denormal-flushing or approximate-reciprocal
// flag, so every fp32 operation (add, subtract, multiply, IEEE divide, floor, min) has exactly one
// result, and the tap order and the multiply-then-add accumulation are part of it -
// tests/specular_temporal_ref.py is the definition. The chain pixel, the projection, the tap walk,
// the tap tests and the blend are gather.hpp's.
#include "temporal_spec.hpp"

#include "gather.hpp"

namespace rt {

__global__ __launch_bounds__(kGaBlock) void temporal_spec_kernel(TsArgs A, RsGuides N, TsHistory Q,
                                                                 const uint8_t* __restrict__ reusable,
                                                                 const uint8_t* __restrict__ through,
                                                                 const float* __restrict__ fresh,
                                                                 const int32_t* __restrict__ px_samples,
                                                                 const float* __restrict__ variance,
                                                                 float4* __restrict__ ocol, float* __restrict__ ovar,
                                                                 float* __restrict__ oweight,
                                                                 uint8_t* __restrict__ okind) {
    GaPixel p;
    if (!ga_pixel(A.w, A.h, p)) return;
    // (an empty history, pw == 0, has no planes and no tables; one without chain planes serves
    // the first-hit pixels only)
    const GaChainPixel cp = ga_chain_pixel(A, N, p.k, A.pw > 0, A.chain_history != 0, reusable, through);
    float ws = 0.0f, ar = 0.0f, ag = 0.0f, ab = 0.0f, av = 0.0f, al = 0.0f;
    if (cp.valid) {
        ga_taps(A, cp.X[0], cp.X[1], cp.X[2], [&](size_t q, float b) {
            const float4 cq = Q.col[q];
            const float vraw = Q.var[q];
            bool ok;
            if (cp.spec) {
                // with cq and vraw: four 16-byte loads and two 4-byte loads, issued together
                // before the tests
                const float4 pf = Q.g.gp[q], nq = Q.g.sgn[q], Pq = Q.g.sgp[q];
                const int32_t chq = Q.g.chain[q];
                ok = ga_chain_same_surface(cp, A.normal_min, pf, nq, Pq, chq) && ga_holds_history(cq);
            } else {
                const float4 nq = Q.g.gn[q], Pq = Q.g.gp[q];
                ok = ga_same_surface(cp.n, cp.P, cp.plane, A.normal_min, nq, Pq) && ga_holds_history(cq);
            }
            const float vq = ga_variance(vraw);
            ws = ws + (ok ? b : 0.0f);
            ar = ar + (ok ? b * cq.x : 0.0f);
            ag = ag + (ok ? b * cq.y : 0.0f);
            ab = ab + (ok ? b * cq.z : 0.0f);
            av = av + (ok ? b * vq : 0.0f);
            al = al + (ok ? b * cq.w : 0.0f);
        });
    }
    float4 oc;
    float ov;
    const float weight = ga_accumulate_blend(A, p, ws, ar, ag, ab, av, al, fresh, px_samples, variance, oc, ov);
    ocol[p.k] = oc;
    ovar[p.k] = ov;
    oweight[p.k] = weight;
    okind[p.k] = weight > 0.0f ? (cp.spec ? (uint8_t)2 : (uint8_t)1) : (uint8_t)0;
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
    hipLaunchKernelGGL(temporal_spec_kernel, ga_grid(a.w, a.h), dim3(kGaBlock), 0, stream, a, nw, hist, reusable,
                       through, fresh, px_samples, variance, out.col, out.var, out.weight, kind);
    return hipGetLastError();
}

}  // namespace rt
