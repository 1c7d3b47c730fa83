// Closest-hit probe of the fp32 build (rt_debug_world_hit_fp32; parity tests). Compiled with
// pt_fp32.hip's flags, so the intersectors and the hit record here are the fp32 path kernels'
// own code (Real = float: sphere_radius<float>, plane_d<float>, the fp32 leaf and exact-test
// records). A unit of its own: pt_ref.hip and pt_fp32.hip do not change.
#include <algorithm>

#include "launch.hpp"
#include "pt_shade.hpp"  // closest_hit_any, sphere_normal

namespace rt {

// out per ray: {hit, t, p.xyz, n.xyz, front, prim} - world_hit_kernel's layout (pt_ref.hip);
// p, the normal and the side as shade_hit (pt_shade.hpp) forms them.
template <class Real, int TRAV>
__global__ __launch_bounds__(kBlock) void world_hit_kernel(DevScene S, int n, const float* orig, const float* dir,
                                                           double* out) {
    extern __shared__ int lds_stack[];
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const V3 o = v3(orig[3 * k], orig[3 * k + 1], orig[3 * k + 2]);
    const V3 d = v3(dir[3 * k], dir[3 * k + 1], dir[3 * k + 2]);
    const RayK<Real> r = make_ray<Real>(o, d);
    Real t = 0;
    int* stk = lds_stack + threadIdx.x;
    const int h = closest_hit_any<Real, false, TRAV>(S, S.cam.n_prims, r, t, stk, nullptr);
    double* w = out + 10 * (size_t)k;
    w[0] = h >= 0;
    w[1] = h >= 0 ? (double)t : 0.0;
    for (int a = 2; a < 10; ++a) w[a] = 0.0;
    w[9] = h;
    if (h >= 0) {
        const RtPrim pr = S.prims[h];
        const V3 p = ray_at<Real>(o, d, t);
        V3 nrm;
        bool front;
        if (pr.type == PRIM_SPHERE) {
            nrm = sphere_normal<Real>(pr, p);
            front = dot<Real>(d, nrm) <= (Real)0;
            if (!front) nrm = neg(nrm);
        } else {
            const V3 pn = ld3(pr.g3);
            front = dot<Real>(d, pn) <= (Real)0;
            nrm = front ? pn : neg(pn);
        }
        w[2] = p.x; w[3] = p.y; w[4] = p.z;
        w[5] = nrm.x; w[6] = nrm.y; w[7] = nrm.z;
        w[8] = front;
    }
}

hipError_t launch_world_hit_fp32(const DevScene& S, int trav, int n, const float* orig, const float* dir,
                                 double* out, hipStream_t stream) {
    const int grid = (n + kBlock - 1) / kBlock;
    const size_t lds = std::max(stack_lds_bytes(S.cam.stack_depth, TRAV_FAST, S.cam.n_prims),
                                stack_lds_bytes(S.cam.stack_depth, TRAV_BRUTE, S.cam.n_prims));  // largest footprint
    if (trav == TRAV_BRUTE)
        hipLaunchKernelGGL((world_hit_kernel<float, TRAV_BRUTE>), dim3(grid), dim3(kBlock), lds, stream, S, n, orig,
                           dir, out);
    else if (trav == TRAV_FAST)
        hipLaunchKernelGGL((world_hit_kernel<float, TRAV_FAST>), dim3(grid), dim3(kBlock), lds, stream, S, n, orig,
                           dir, out);
    else
        hipLaunchKernelGGL((world_hit_kernel<float, TRAV_REFERENCE>), dim3(grid), dim3(kBlock), lds, stream, S, n,
                           orig, dir, out);
    return hipGetLastError();
}

}  // namespace rt
