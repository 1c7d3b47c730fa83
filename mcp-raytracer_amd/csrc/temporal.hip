// The accumulation gather and blend (temporal.hpp). Compiled with -ffp-contract=off and without
// any fast-math, denormal-flushing or approximate-reciprocal flag: every fp32 operation (add,
// subtract, multiply, IEEE divide, floor, min) has exactly one result, and the tap order and the
// multiply-then-add accumulation are part of it - tests/temporal_ref.py is the definition. The
// projection, the tap walk, the tap test and the blend are gather.hpp's.
#include "temporal.hpp"

#include "gather.hpp"

namespace rt {

__global__ __launch_bounds__(kGaBlock) void temporal_kernel(TpArgs A, const float4* __restrict__ gn,
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
    GaPixel p;
    if (!ga_pixel(A.w, A.h, p)) return;
    const float4 n = gn[p.k], P = gp[p.k];
    float ws = 0.0f, ar = 0.0f, ag = 0.0f, ab = 0.0f, av = 0.0f, al = 0.0f;
    // (an empty history, pw == 0, has no planes and no reusable table)
    if (A.pw > 0 && ga_marked_point(P, A.n_objects, reusable)) {
        const float plane = A.sigma_plane * n.w;
        ga_taps(A, P.x, P.y, P.z, [&](size_t q, float b) {
            const float4 nq = pgn[q], Pq = pgp[q], cq = pcol[q];
            const float vq = ga_variance(pvar[q]);
            const bool ok = ga_same_surface(n, P, plane, A.normal_min, nq, Pq) && ga_holds_history(cq);
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
}

__global__ __launch_bounds__(kGaBlock) void temporal_pack_kernel(const float* __restrict__ rad,
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
    hipLaunchKernelGGL(temporal_kernel, ga_grid(a.w, a.h), dim3(kGaBlock), 0, stream, a, gn, gp, hist.gn, hist.gp,
                       hist.col, hist.var, reusable, fresh, px_samples, variance, out.col, out.var, out.weight);
    return hipGetLastError();
}

hipError_t launch_temporal_pack(const float* rad, const float* length, int n, float4* col, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(temporal_pack_kernel, dim3((unsigned)((n + kGaBlock - 1) / kGaBlock)), dim3(kGaBlock), 0, stream,
                       rad, length, n, col);
    return hipGetLastError();
}

}  // namespace rt
