// The reprojection gather (reproject.hpp). Compiled with -ffp-contract=off and without any
// fast-math, denormal-flushing or approximate-reciprocal flag: every fp32 operation (add,
// subtract, multiply, IEEE divide, floor) has exactly one result, and the tap order and the
// multiply-then-add accumulation are part of it - tests/reproject_ref.py is the definition.
// The projection, the tap walk, the tap test and the blend are gather.hpp's.
#include "gather.hpp"

namespace rt {

__global__ __launch_bounds__(kGaBlock) void reproject_kernel(RpArgs A, const float4* __restrict__ gn,
                                                             const float4* __restrict__ gp,
                                                             const float4* __restrict__ pgn,
                                                             const float4* __restrict__ pgp,
                                                             const float4* __restrict__ pcol,
                                                             const uint8_t* __restrict__ reusable,
                                                             const float* __restrict__ fresh,
                                                             const int32_t* __restrict__ px_samples,
                                                             float4* __restrict__ hist, float4* __restrict__ outc) {
    GaPixel p;
    if (!ga_pixel(A.w, A.h, p)) return;
    const float4 n = gn[p.k], P = gp[p.k];
    float ws = 0.0f, ar = 0.0f, ag = 0.0f, ab = 0.0f;
    if (ga_marked_point(P, A.n_objects, reusable)) {
        const float plane = A.sigma_plane * n.w;
        ga_taps(A, P.x, P.y, P.z, [&](size_t q, float b) {
            const float4 nq = pgn[q], Pq = pgp[q], cq = pcol[q];
            const bool ok = ga_same_surface(n, P, plane, A.normal_min, nq, Pq) && ga_flagged(cq);
            ws = ws + (ok ? b : 0.0f);
            ar = ar + (ok ? b * cq.x : 0.0f);
            ag = ag + (ok ? b * cq.y : 0.0f);
            ab = ab + (ok ? b * cq.z : 0.0f);
        });
    }
    const float4 hv = ga_history(ws, ar, ag, ab, A.min_weight);
    hist[p.k] = hv;
    if (!fresh) return;  // (outc may be null)
    float4 ov = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    ga_reproject_blend(A, p, hv, fresh, px_samples, ov);
    outc[p.k] = ov;
}

hipError_t launch_reproject(const RpArgs& a, const float4* gn, const float4* gp, const float4* pgn, const float4* pgp,
                            const float4* pcol, const uint8_t* reusable, const float* fresh, const int32_t* px_samples,
                            float4* hist, float4* outc, hipStream_t stream) {
    if (a.w <= 0 || a.h <= 0) return hipSuccess;
    if (a.pw <= 0 || a.ph <= 0 || !hist || (fresh && !outc)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(reproject_kernel, ga_grid(a.w, a.h), dim3(kGaBlock), 0, stream, a, gn, gp, pgn, pgp, pcol,
                       reusable, fresh, px_samples, hist, outc);
    return hipGetLastError();
}

}  // namespace rt
