// Guides through the specular chain (denoise.hpp launch_guide_walk). Compiled as denoise.hip is:
// -ffp-contract=off and no fast-math flag, so every operation of the walk has exactly one result -
// tests/guide_walk_ref.py is the definition. The walk draws no random number: each material has a
// policy in place of scatter's draws (pt_shade.hpp), and the arithmetic of a direction is
// scatter's own in ref precision (fp64 scalars, fp32 vector stores).
#include <algorithm>

#include "denoise.hpp"
#include "pt_pixel.hpp"  // item_pixel
#include "pt_shade.hpp"  // pixel_center, closest_hit_any

namespace rt {

// dielectric_dir (pt_shade.hpp) without its draw: refract whenever refraction is possible, reflect
// otherwise - Schlick's reflectance is ignored. Written again here, not shared: the path units'
// code generation must not move (pt_shade.hpp stays as it is).
__device__ __forceinline__ V3 walk_dielectric_dir(double ior, bool front, V3 din, V3 n, bool& reflected) {
    const double ratio = front ? (1.0 / ior) : ior;
    const V3 ud = unit<double>(din);
    const double cosT = js_min<double>(dot<double>(neg(ud), n), 1.0);
    const double sinT = m_sqrt(1.0 - cosT * cosT);
    reflected = ratio * sinT > 1.0;
    if (reflected) return reflect<double>(ud, n);
    // Vec3.refract (src/geometry/vec3.ts:193-209)
    const V3 perp = scale<double>(add(ud, scale<double>(n, cosT)), ratio);
    const V3 par = scale<double>(n, -m_sqrt(m_abs(1.0 - len2<double>(perp))));
    return add(perp, par);
}

// scatter's structure (pt_shade.hpp) over the material table with a policy in place of each draw:
// true when the walk continues from this hit, along `dir`. Lambert, lights and the default
// material are terminal; so is a metal whose fuzz exceeds max_fuzz or whose mirror direction
// points into the surface (its fuzz term is dropped otherwise); glass follows
// walk_dielectric_dir; a mixed material is its likelier child (c0 on a tie); a layered one its
// coat by the glass rule, and under a refracting coat its inner material with the refracted
// direction as the incoming one.
__device__ __forceinline__ bool walk_continue(const DevScene& S, int mi, V3 din, V3 n, bool front, double max_fuzz,
                                              V3& dir) {
    while (true) {
        const RtMat m = S.mats[mi];
        switch (m.type) {
            case MAT_METAL: {
                const V3 f = reflect<double>(unit<double>(din), n);
                if (m.p0 > max_fuzz || dot<double>(f, n) <= 0.0) return false;
                dir = f;
                return true;
            }
            case MAT_GLASS:
            case MAT_LAYERED: {
                const bool coat = m.type == MAT_LAYERED;
                bool r;
                const V3 d2 = walk_dielectric_dir(coat ? S.mats[m.c0].p0 : m.p0, front, din, n, r);
                if (!coat || r) {
                    dir = d2;
                    return true;
                }
                din = d2;  // the refracted ray becomes rIn for the inner material
                mi = m.c1;
                continue;
            }
            case MAT_MIXED:
                mi = m.p0 >= 0.5 ? m.c0 : m.c1;
                continue;
            default:
                return false;
        }
    }
}

enum WalkEnd { WALK_MISS = 0, WALK_SURFACE = 1, WALK_LEFT = 2, WALK_BOUNCES = 3 };

// Launch shape, stack and residency as guide_kernel (denoise.hip): one thread per pixel, a wave
// per 8x8 tile, the per-lane LDS stack reused by every segment, the scene read from global
// memory. One closest_hit_any call site in a loop that is never unrolled; a lane leaves the loop
// when its walk ends, the wave when all its lanes have.
template <int TRAV>
__global__ __launch_bounds__(kBlock) void guide_walk_kernel(DevScene S, RtRegion reg, int tiles_x, int n_tiles,
                                                            const int32_t* prim_object, DenoiseGuides g,
                                                            int32_t* chain, int max_bounces, double max_fuzz) {
    extern __shared__ int lds_stack[];
    const int tile = blockIdx.x * (kBlock / kWave) + (int)(threadIdx.x / kWave);
    if (tile >= n_tiles) return;
    int i, j;
    item_pixel(reg, tiles_x, tile, (int)(threadIdx.x & (kWave - 1)), i, j);
    if (i >= reg.x + reg.width || j >= reg.y + reg.height) return;
    const RtCamera& C = S.cam;
    int* stk = lds_stack + threadIdx.x;
    // segment 0: guide_kernel's ray
    V3 o = ld3(C.center);
    V3 d = sub(pixel_center<double>(C, i, j), o);
    float dist = 0.0f;
    int k = 0, end = -1;
    float4 gn = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 gp = make_float4(0.f, 0.f, 0.f, __int_as_float(-1));
    float4 ln = gn, lp = gp;  // the specular surface the chain last left through
#pragma clang loop unroll(disable)
    while (end < 0) {
        const RayK<double> r = make_ray<double>(o, d);
        double t = 0;
        const int h = closest_hit_any<double, false, TRAV>(S, C.n_prims, r, t, stk, nullptr);
        if (h < 0) {
            gn = ln;
            gp = lp;
            end = k == 0 ? WALK_MISS : WALK_LEFT;
            break;
        }
        const RtPrim pr = S.prims[h];
        const V3 p = ray_at<double>(o, d, t);
        V3 nrm;
        bool front;
        if (pr.type == PRIM_SPHERE) {
            nrm = divs<double>(sub(p, ld3(pr.g0)), sphere_radius<double>(pr));
            front = dot<double>(d, nrm) <= 0.0;
            if (!front) nrm = neg(nrm);
        } else {
            const V3 pn = ld3(pr.g3);
            front = dot<double>(d, pn) <= 0.0;
            nrm = front ? pn : neg(pn);
        }
        const V3 q = sub(p, o);
        dist = dist + ::sqrtf((q.x * q.x + q.y * q.y) + q.z * q.z);
        gn = make_float4(nrm.x, nrm.y, nrm.z, dist);
        gp = make_float4(p.x, p.y, p.z, __int_as_float(prim_object[h]));
        V3 nd;
        if (!walk_continue(S, pr.mat, d, nrm, front, max_fuzz, nd)) {
            end = WALK_SURFACE;
        } else if (k == max_bounces) {
            end = WALK_BOUNCES;
        } else {
            ln = gn;
            lp = gp;
            o = p;
            d = nd;
            ++k;
        }
    }
    const size_t px = (size_t)(j - reg.y) * (size_t)reg.width + (size_t)(i - reg.x);
    g.gn[px] = gn;
    g.gp[px] = gp;
    if (chain) chain[px] = k | end << 8;
}

__global__ __launch_bounds__(256) void guides_chain_kernel(DenoiseGuides g, int n, int32_t* chain) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    chain[k] = __float_as_int(g.gp[k].w) >= 0 ? WALK_SURFACE << 8 : 0;
}

hipError_t launch_guide_walk(const DevScene& S, int trav, const RtRegion& reg, const int32_t* prim_object,
                             const DenoiseGuides& g, int32_t* chain, int max_bounces, float max_fuzz, int lds_max,
                             hipStream_t stream) {
    const int tiles_x = std::max((reg.width + kTile - 1) / kTile, 1);
    const long tiles = (long)tiles_x * ((reg.height + kTile - 1) / kTile);
    if (tiles <= 0) return hipSuccess;
    if (tiles > 0x7fffffffl / kWave) return hipErrorInvalidValue;
    const RtRegion r{reg.x, reg.y, reg.width, reg.height, 0, 1};
    const size_t lds = stack_lds_bytes(S.cam.stack_depth, trav, S.cam.n_prims);
    if (lds > (size_t)lds_max) return hipErrorInvalidValue;
    const int waves = kBlock / kWave;
    const dim3 grid((unsigned)((tiles + waves - 1) / waves));
    const double mf = (double)max_fuzz;
    if (trav == TRAV_BRUTE)
        hipLaunchKernelGGL(guide_walk_kernel<TRAV_BRUTE>, grid, dim3(kBlock), lds, stream, S, r, tiles_x, (int)tiles,
                           prim_object, g, chain, max_bounces, mf);
    else if (trav == TRAV_FAST)
        hipLaunchKernelGGL(guide_walk_kernel<TRAV_FAST>, grid, dim3(kBlock), lds, stream, S, r, tiles_x, (int)tiles,
                           prim_object, g, chain, max_bounces, mf);
    else
        hipLaunchKernelGGL(guide_walk_kernel<TRAV_REFERENCE>, grid, dim3(kBlock), lds, stream, S, r, tiles_x, (int)tiles,
                           prim_object, g, chain, max_bounces, mf);
    return hipGetLastError();
}

hipError_t launch_guides_chain(const DenoiseGuides& g, int n, int32_t* chain, hipStream_t stream) {
    if (n <= 0 || !chain) return hipSuccess;
    hipLaunchKernelGGL(guides_chain_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, g, n, chain);
    return hipGetLastError();
}

}  // namespace rt
