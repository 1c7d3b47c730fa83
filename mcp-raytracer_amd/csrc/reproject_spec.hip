// The reprojection gather through specular chains (reproject_spec.hpp). Compiled as reproject.hip:
// -ffp-contract=off and no fast-math, denormal-flushing or approximate-reciprocal flag, so every
// fp32 operation (add, subtract, multiply, IEEE divide, floor) has exactly one result, and the tap
// order and the multiply-then-add accumulation are part of it - tests/specular_reproject_ref.py is
// the definition. The chain pixel, the projection, the tap walk, the tap tests and the blend are
// gather.hpp's.
#include "gather.hpp"

namespace rt {

__global__ __launch_bounds__(kGaBlock) void reproject_spec_kernel(RsArgs A, RsGuides N, RsGuides Q,
                                                                  const float4* __restrict__ pcol,
                                                                  const uint8_t* __restrict__ reusable,
                                                                  const uint8_t* __restrict__ through,
                                                                  const float* __restrict__ fresh,
                                                                  const int32_t* __restrict__ px_samples,
                                                                  float4* __restrict__ hist, float4* __restrict__ outc) {
    GaPixel p;
    if (!ga_pixel(A.w, A.h, p)) return;
    const GaChainPixel cp = ga_chain_pixel(A, N, p.k, true, true, reusable, through);
    float ws = 0.0f, ar = 0.0f, ag = 0.0f, ab = 0.0f;
    if (cp.valid) {
        ga_taps(A, cp.X[0], cp.X[1], cp.X[2], [&](size_t q, float b) {
            const float4 cq = pcol[q];
            bool ok;
            if (cp.spec) {
                // four 16-byte loads and one 4-byte load, issued together before the tests
                const float4 pf = Q.gp[q], nq = Q.sgn[q], Pq = Q.sgp[q];
                const int32_t chq = Q.chain[q];
                ok = ga_chain_same_surface(cp, A.normal_min, pf, nq, Pq, chq) && ga_flagged(cq);
            } else {
                const float4 nq = Q.gn[q], Pq = Q.gp[q];
                ok = ga_same_surface(cp.n, cp.P, cp.plane, A.normal_min, nq, Pq) && ga_flagged(cq);
            }
            ws = ws + (ok ? b : 0.0f);
            ar = ar + (ok ? b * cq.x : 0.0f);
            ag = ag + (ok ? b * cq.y : 0.0f);
            ab = ab + (ok ? b * cq.z : 0.0f);
        });
    }
    const float4 hv = ga_history(ws, ar, ag, ab, A.min_weight);
    hist[p.k] = hv;
    // always written: the kind travels in .w
    float4 ov = make_float4(0.0f, 0.0f, 0.0f, hv.w > 0.0f ? (cp.spec ? 2.0f : 1.0f) : 0.0f);
    if (fresh) ga_reproject_blend(A, p, hv, fresh, px_samples, ov);
    outc[p.k] = ov;
}

__global__ __launch_bounds__(kGaBlock) void reproject_spec_kind_kernel(const float4* __restrict__ outc, int n,
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
    hipLaunchKernelGGL(reproject_spec_kernel, ga_grid(a.w, a.h), dim3(kGaBlock), 0, stream, a, nw, pv, pcol, reusable,
                       through, fresh, px_samples, hist, outc);
    return hipGetLastError();
}

hipError_t launch_reproject_spec_kind(const float4* outc, int n, uint8_t* kind, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    if (!outc || !kind) return hipErrorInvalidValue;
    hipLaunchKernelGGL(reproject_spec_kind_kernel, dim3((unsigned)((n + kGaBlock - 1) / kGaBlock)), dim3(kGaBlock), 0,
                       stream, outc, n, kind);
    return hipGetLastError();
}

}  // namespace rt
