// Exact ray / primitive intersection tests and the reference-order BVH traversal.
#pragma once

#include <hip/hip_runtime.h>

#include "pt_num.hpp"

namespace rt {

// Per-ray constants reused by every node and primitive test.
template <class Real> struct RayK {
    V3 o, d;
    Real inv[3];  // 1/d[a] (AABB.hit computes it per node; same value)
    Real a;       // d.lengthSquared() (Sphere.hit computes it per sphere; same value)
};

template <class Real>
__device__ __forceinline__ RayK<Real> make_ray(V3 o, V3 d) {
    RayK<Real> r;
    r.o = o;
    r.d = d;
    r.inv[0] = (Real)1 / (Real)d.x;
    r.inv[1] = (Real)1 / (Real)d.y;
    r.inv[2] = (Real)1 / (Real)d.z;
    r.a = len2<Real>(d);
    return r;
}

// The ray as the exact (Real) tests inside a traversal loop see it: o and d
// pass through an empty asm so their conversions to Real (and |d|^2) are
// redone per test instead of being hoisted out of the loop as long-lived fp64
// values - which the register allocator then spills to scratch every trip.
// Values are unchanged; the tests run on a small fraction of loop iterations.
template <class Real>
__device__ __forceinline__ RayK<Real> ray_at_use(const RayK<Real>& r) {
    RayK<Real> q = r;
    asm volatile("" : "+v"(q.o.x), "+v"(q.o.y), "+v"(q.o.z), "+v"(q.d.x), "+v"(q.d.y), "+v"(q.d.z));
    q.a = len2<Real>(q.d);
    return q;
}

// AABB.hit (src/geometry/aabb.ts:30-55): each axis is clipped against the
// ORIGINAL interval (the reference does not carry tMin/tMax across axes);
// comparisons keep the reference's NaN behaviour.
template <class Real>
__device__ __forceinline__ bool box_hit(const RtNode& n, const RayK<Real>& r, Real tmin, Real tmax) {
    const float o[3] = {r.o.x, r.o.y, r.o.z};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const Real invD = r.inv[a];
        Real t0 = ((Real)n.bmin[a] - (Real)o[a]) * invD;
        Real t1 = ((Real)n.bmax[a] - (Real)o[a]) * invD;
        if (invD < (Real)0) { Real tmp = t0; t0 = t1; t1 = tmp; }
        const Real lo = t0 > tmin ? t0 : tmin;
        const Real hi = t1 < tmax ? t1 : tmax;
        if (hi <= lo) return false;
    }
    return true;
}

template <class Real> __device__ __forceinline__ Real sphere_radius(const RtPrim& p);
template <> __device__ __forceinline__ double sphere_radius<double>(const RtPrim& p) { return p.s0; }
template <> __device__ __forceinline__ float sphere_radius<float>(const RtPrim& p) { return p.g0[3]; }
// 1 / radius (Vec3.divide's reciprocal, vec3.ts:126-130), computed on the host with the same
// IEEE division: sphere records carry it in g1 (double bits in g1[0..1], fp32 in g1[2]).
template <class Real> __device__ __forceinline__ Real sphere_inv_radius(const RtPrim& p);
template <> __device__ __forceinline__ double sphere_inv_radius<double>(const RtPrim& p) {
    return __hiloint2double(__float_as_int(p.g1[1]), __float_as_int(p.g1[0]));
}
template <> __device__ __forceinline__ float sphere_inv_radius<float>(const RtPrim& p) { return p.g1[2]; }
template <class Real> __device__ __forceinline__ Real plane_d(const RtPrim& p);
template <> __device__ __forceinline__ double plane_d<double>(const RtPrim& p) { return p.s0; }
template <> __device__ __forceinline__ float plane_d<float>(const RtPrim& p) { return p.g0[3]; }

// Sphere.hit root selection (src/entities/sphere.ts:45-65); returns t only.
template <class Real>
__device__ __forceinline__ bool sphere_t_cr(V3 c, Real rad, const RayK<Real>& r, Real tmin, Real tmax, Real& t) {
    const V3 oc = sub(r.o, c);
    const Real halfB = dot<Real>(oc, r.d);
    const Real cc = len2<Real>(oc) - rad * rad;
    const Real disc = halfB * halfB - r.a * cc;
    if (disc < (Real)0) return false;
    const Real sq = m_sqrt(disc);
    Real root = (-halfB - sq) / r.a;
    if (!(tmin < root && root < tmax)) {
        root = (-halfB + sq) / r.a;
        if (!(tmin < root && root < tmax)) return false;
    }
    t = root;
    return true;
}
template <class Real>
__device__ __forceinline__ bool sphere_t(const RtPrim& p, const RayK<Real>& r, Real tmin, Real tmax, Real& t) {
    return sphere_t_cr<Real>(ld3(p.g0), sphere_radius<Real>(p), r, tmin, tmax, t);
}

// Plane.intersect (src/entities/plane.ts:55-77) + Quad bounds (quad.ts:50-76).
template <class Real, bool QUAD>
__device__ __forceinline__ bool planar_t(const RtPrim& p, const RayK<Real>& r, Real tmin, Real tmax, Real& t) {
    const V3 n = ld3(p.g3);
    const Real denom = dot<Real>(n, r.d);
    if (m_abs(denom) < (Real)1e-8) return false;
    const Real tt = (plane_d<Real>(p) - dot<Real>(n, r.o)) / denom;
    if (!(tmin < tt && tt < tmax)) return false;
    if (QUAD) {
        const V3 ip = ray_at<Real>(r.o, r.d, tt);
        const V3 ph = sub(ip, ld3(p.g0));
        const V3 w = ld3(p.g4);
        const Real alpha = dot<Real>(w, cross<Real>(ph, ld3(p.g2)));
        const Real beta = dot<Real>(w, cross<Real>(ld3(p.g1), ph));
        if (alpha < (Real)0 || alpha > (Real)1 || beta < (Real)0 || beta > (Real)1) return false;
    }
    t = tt;
    return true;
}

constexpr float kTminLo = 0.001f * (1.0f - 1e-5f);  // below the reference's tMin with margin (fp32 tests)
// fp32 pre-filter error model: every estimate below is an fp32 evaluation of the
// reference's fp64 formula, off by at most a few tens of ulps of the operand
// magnitudes (products of fp32 values are exact in fp64). kRel (~170 ulps)
// bounds that with a wide margin; the margins scale with |o|, |d|, |Q|, r so
// they hold for any scene scale. Hardware rcp/sqrt (<= 1 ulp) are inside kRel.
constexpr float kRel = 1e-5f;

// The fp32 conservative filters (slab tests, sphere / planar / axis-quad pre-filters, the
// FRay constants, the culling bound) may contract a*b+c into one FMA even in the ref TU,
// which is compiled with -ffp-contract=off because the reference's JS arithmetic never
// fuses. That flag must keep holding for the fp64 path and for the fp32 vector stores of
// the exact tests, so contraction is opened per function body (RT_FP32_FUSED, a block-
// scoped pragma: it marks only the operations written inside that block, and inlining
// keeps the marks per operation). A filter's result reaches the output only through the
// exact fp64 test it lets through, so the filter may round differently as long as it stays
// conservative. Every margin below is of the form c * u * (sum of the magnitudes of the
// terms): a fused a*b+c rounds once where the unfused form rounds twice, so each margin
// still bounds it. The one changed form is the slab test, which no longer subtracts first
// (see slab_t4 / FRay::eps). Before: SQ_INSTS_VALU_FMA_F32 was 0.0 % of VALU
// on Cornell ref, 1.0 % on spheres-500 and 0.5 % on spheres-100k.
#define RT_FP32_FUSED _Pragma("clang fp contract(fast)")

// Axis-aligned quad (scene.cpp encode_axis_quad): Plane.intersect + Quad's
// alpha/beta test with the terms that are exact zeros dropped. Every kept
// operation is the reference's own (a product of two fp32 values is exact in
// double, x - (+-0) = x, sums with +-0 are exact), so t and the accept/reject
// decision are bit-identical to planar_t - provided no 0*inf/NaN term would
// have turned the reference's result into NaN, which the finiteness guard
// reproduces (a non-finite off-axis ray component makes the reference miss).
// One specialisation per axis code (constant indices: no selects, no branches).
template <class Real, int CODE>
__device__ __forceinline__ bool aquad_t_c(const RtPrim& p, V3 o3, V3 d3, Real tmin, Real tmax, Real& t) {
    constexpr int a = (CODE - 1) % 3, vflag = (CODE - 1) / 3;
    constexpr int ia = vflag ? (a + 1) % 3 : (a + 2) % 3, ib = vflag ? (a + 2) % 3 : (a + 1) % 3;
    const float o[3] = {o3.x, o3.y, o3.z}, d[3] = {d3.x, d3.y, d3.z};
    if (!(::isfinite(o[ia]) && ::isfinite(d[ia]) && ::isfinite(o[ib]) && ::isfinite(d[ib]))) return false;
    const Real na = (Real)p.g3[a];
    const Real denom = na * (Real)d[a];
    if (m_abs(denom) < (Real)1e-8) return false;
    const Real tt = (plane_d<Real>(p) - na * (Real)o[a]) / denom;
    if (!(tmin < tt && tt < tmax)) return false;
    // Ray.at(t) in-plane components, hit point minus Q (fp32 stores)
    const float ph1 = (o[ia] + (float)((Real)d[ia] * tt)) - p.g0[ia];
    const float ph2 = (o[ib] + (float)((Real)d[ib] * tt)) - p.g0[ib];
    const Real sw = (Real)p.g3[3];
    const Real alpha = sw * (Real)(ph1 * p.g2[3]);
    const Real beta = sw * (Real)(ph2 * p.g1[3]);
    if (alpha < (Real)0 || alpha > (Real)1 || beta < (Real)0 || beta > (Real)1) return false;
    t = tt;
    return true;
}

// fp32 pre-filter of aquad_t_c: false only when the exact test surely rejects or
// gives no t <= thi.
// `lo` (all pre-filters): a lower bound of the exact t the test can return.
// Fields: na = n[a], D, q1 = Q[ia], q2 = Q[ib], sw = +-w[a], sv = v[iv], su = u[iu] (RtPre order).
template <int CODE>
__device__ __forceinline__ bool aquad_maybe_v(float na, float D, float q1, float q2, float sw, float sv, float su,
                                              const float* o, const float* d, float dn, float thi, float& lo) {
    RT_FP32_FUSED
    constexpr int a = (CODE - 1) % 3, vflag = (CODE - 1) / 3;
    constexpr int ia = vflag ? (a + 1) % 3 : (a + 2) % 3, ib = vflag ? (a + 2) % 3 : (a + 1) % 3;
    const float denom = na * d[a];
    lo = kTminLo;
    if (!(::fabsf(denom) > 1e-3f * dn)) return true;  // near-parallel: decide exactly
    const float no = na * o[a];
    const float idn = __builtin_amdgcn_rcpf(denom);
    const float t = (D - no) * idn;
    const float et = kRel * ((::fabsf(D) + ::fabsf(no)) * ::fabsf(idn) + 2.0f * ::fabsf(t)) + 1e-30f;
    if (t + et < kTminLo || t - et > thi) return false;
    lo = t - et;
    const float ph1 = o[ia] + t * d[ia] - q1;
    const float ph2 = o[ib] + t * d[ib] - q2;
    const float alpha = sw * (ph1 * sv);
    const float beta = sw * (ph2 * su);
    // in-plane hit-point error, times |w_a v| (alpha) / |w_a u| (beta)
    const float dp1 = et * ::fabsf(d[ia]) + kRel * (::fabsf(o[ia]) + ::fabsf(t * d[ia]) + ::fabsf(q1));
    const float dp2 = et * ::fabsf(d[ib]) + kRel * (::fabsf(o[ib]) + ::fabsf(t * d[ib]) + ::fabsf(q2));
    const float ea = ::fabsf(sw * sv) * dp1 + 1e-4f;
    const float eb = ::fabsf(sw * su) * dp2 + 1e-4f;
    return !(alpha < -ea || alpha > 1.0f + ea || beta < -eb || beta > 1.0f + eb);
}
template <int CODE>
__device__ __forceinline__ bool aquad_maybe_c(const RtPrim& p, const float* o, const float* d, float dn, float thi,
                                              float& lo) {
    constexpr int a = (CODE - 1) % 3, vflag = (CODE - 1) / 3;
    constexpr int ia = vflag ? (a + 1) % 3 : (a + 2) % 3, ib = vflag ? (a + 2) % 3 : (a + 1) % 3;
    return aquad_maybe_v<CODE>(p.g3[a], p.g0[3], p.g0[ia], p.g0[ib], p.g3[3], p.g2[3], p.g1[3], o, d, dn, thi, lo);
}

template <class Real>
__device__ __forceinline__ bool aquad_t(const RtPrim& p, int code, V3 o, V3 d, Real tmin, Real tmax, Real& t) {
    switch (code) {
        case 1: return aquad_t_c<Real, 1>(p, o, d, tmin, tmax, t);
        case 2: return aquad_t_c<Real, 2>(p, o, d, tmin, tmax, t);
        case 3: return aquad_t_c<Real, 3>(p, o, d, tmin, tmax, t);
        case 4: return aquad_t_c<Real, 4>(p, o, d, tmin, tmax, t);
        case 5: return aquad_t_c<Real, 5>(p, o, d, tmin, tmax, t);
        default: return aquad_t_c<Real, 6>(p, o, d, tmin, tmax, t);
    }
}
__device__ __forceinline__ bool aquad_maybe(const RtPrim& p, int code, const float* o, const float* d, float dn,
                                            float thi, float& lo) {
    switch (code) {
        case 1: return aquad_maybe_c<1>(p, o, d, dn, thi, lo);
        case 2: return aquad_maybe_c<2>(p, o, d, dn, thi, lo);
        case 3: return aquad_maybe_c<3>(p, o, d, dn, thi, lo);
        case 4: return aquad_maybe_c<4>(p, o, d, dn, thi, lo);
        case 5: return aquad_maybe_c<5>(p, o, d, dn, thi, lo);
        default: return aquad_maybe_c<6>(p, o, d, dn, thi, lo);
    }
}

// aquad_t_c with the axis code as a runtime value (one code path for lanes
// testing different walls): the same operations on the same operands.
__device__ __forceinline__ float sel3(float x, float y, float z, int i) { return i == 0 ? x : (i == 1 ? y : z); }
constexpr uint32_t aquad_axes(int field) {  // 2-bit fields per code 1..6: a, ia, ib
    uint32_t m = 0;
    for (int c = 1; c <= 6; ++c) {
        const int a = (c - 1) % 3, vflag = (c - 1) / 3;
        const int ia = vflag ? (a + 1) % 3 : (a + 2) % 3, ib = vflag ? (a + 2) % 3 : (a + 1) % 3;
        m |= (uint32_t)(field == 0 ? a : field == 1 ? ia : ib) << (2 * c);
    }
    return m;
}
template <class Real>
__device__ __forceinline__ bool aquad_t_rt(const RtPrim& p, int code, V3 o3, V3 d3, Real tmin, Real tmax, Real& t) {
    const int a = (int)((aquad_axes(0) >> (2 * code)) & 3u);
    const int ia = (int)((aquad_axes(1) >> (2 * code)) & 3u);
    const int ib = (int)((aquad_axes(2) >> (2 * code)) & 3u);
    const float oa = sel3(o3.x, o3.y, o3.z, a), da = sel3(d3.x, d3.y, d3.z, a);
    const float o1 = sel3(o3.x, o3.y, o3.z, ia), d1 = sel3(d3.x, d3.y, d3.z, ia);
    const float o2 = sel3(o3.x, o3.y, o3.z, ib), d2 = sel3(d3.x, d3.y, d3.z, ib);
    if (!(::isfinite(o1) && ::isfinite(d1) && ::isfinite(o2) && ::isfinite(d2))) return false;
    const Real na = (Real)sel3(p.g3[0], p.g3[1], p.g3[2], a);
    const Real denom = na * (Real)da;
    if (m_abs(denom) < (Real)1e-8) return false;
    const Real tt = (plane_d<Real>(p) - na * (Real)oa) / denom;
    if (!(tmin < tt && tt < tmax)) return false;
    const float ph1 = (o1 + (float)((Real)d1 * tt)) - sel3(p.g0[0], p.g0[1], p.g0[2], ia);
    const float ph2 = (o2 + (float)((Real)d2 * tt)) - sel3(p.g0[0], p.g0[1], p.g0[2], ib);
    const Real sw = (Real)p.g3[3];
    const Real alpha = sw * (Real)(ph1 * p.g2[3]);
    const Real beta = sw * (Real)(ph2 * p.g1[3]);
    if (alpha < (Real)0 || alpha > (Real)1 || beta < (Real)0 || beta > (Real)1) return false;
    t = tt;
    return true;
}
__device__ __forceinline__ int aquad_code(const RtPrim& p) { return __float_as_int(p.g4[3]); }

template <class Real, bool COUNT>
__device__ __forceinline__ bool prim_t(const RtPrim& p, const RayK<Real>& r, Real tmin, Real tmax, Real& t,
                                       uint32_t* cnt) {
    if (p.type == PRIM_SPHERE) {
        if (COUNT) cnt[CT_SPHERE]++;
        return sphere_t<Real>(p, r, tmin, tmax, t);
    }
    if (p.type == PRIM_QUAD) {
        if (COUNT) cnt[CT_QUAD]++;
        return planar_t<Real, true>(p, r, tmin, tmax, t);
    }
    if (COUNT) cnt[CT_PLANE]++;
    return planar_t<Real, false>(p, r, tmin, tmax, t);
}

// BVHNode.hit restated as an explicit DFS with the same visiting order: the
// box is tested when a node is entered with the closest-so-far interval, left
// subtree before right, leaf primitives in leaf order with a narrowing max.
// `stk` points at this lane's column of the LDS stack (stride kStackStride ints).
template <class Real, bool COUNT, class SK>
__device__ __forceinline__ int closest_hit(const DevScene& S, const RayK<Real>& r, Real& t_hit, SK* stk,
                                           uint32_t* cnt) {
    const Real tmin = K<Real>::TMIN;
    Real tmax = (Real)__builtin_inf();
    int hit = -1;
    int sp = 0;
    int node = 0;
    while (true) {
        const RtNode nd = S.nodes[node];
        if (COUNT) cnt[CT_NODE]++;
        bool descend = false;
        if (box_hit<Real>(nd, r, tmin, tmax)) {
            if (nd.b < 0) {
                const int end = nd.a - nd.b;
                for (int k = nd.a; k < end; ++k) {
                    Real t;
                    if (prim_t<Real, COUNT>(S.prims[k], r, tmin, tmax, t, cnt)) {
                        tmax = t;
                        hit = k;
                    }
                }
            } else {
                stk[sp * kStackStride] = (SK)nd.b;
                ++sp;
                node = nd.a;
                descend = true;
            }
        }
        if (!descend) {
            if (sp == 0) break;
            --sp;
            node = stk[sp * kStackStride];
        }
    }
    t_hit = tmax;
    return hit;
}

}  // namespace rt
