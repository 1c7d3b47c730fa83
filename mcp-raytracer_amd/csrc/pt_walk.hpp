// The fast traversal: fp32 conservative filters in front of the exact tests, 4-wide node steps.
#pragma once

#include <hip/hip_runtime.h>

#include "pt_isect.hpp"
#include "pt_prof.hpp"

namespace rt {

// ---------------------------------------------------------------------------
// Fast traversal with the SAME result.
//
// The reference tests primitive k with the closest-so-far interval and keeps
// it iff its first root t_k in (0.001, inf) satisfies t_k < tmax (strict), in
// DFS leaf order. So its answer is the lexicographic minimum of (t_k, leaf
// slot) over all primitives - independent of visiting order - provided no box
// containing a valid hit is culled. This traversal therefore
//   * culls with a strict fp32 slab test (the reference's per-axis test culls
//     far less) on boxes padded outward by ~1e-6 relative, accepting ties,
//   * visits the nearer child first and culls stacked nodes against the best t,
//   * rejects a primitive from an fp32 estimate only when it is clearly not a
//     candidate, and otherwise computes t_k with the reference's exact
//     arithmetic (Real) and compares (t, slot) lexicographically.
// The parity tests check it bit-for-bit against both the oracle and the
// reference-order traversal above.
// ---------------------------------------------------------------------------
struct FRay {
    float o[3];
    float d[3];
    float inv[3];  // 1/d with zero components replaced by +-1e-30 (no 0*inf NaNs)
    float noi[3];  // -(o * inv): the slab planes' t = fma(b, inv, noi)
    float eps;     // absolute t slack of the fused slab test (>= 2u max|o * inv|, see slab_t)
    float pthr;    // |d[a]| at or below which an axis quad counts as near-parallel (inf: every one)
    int nrow[3];   // byte offset in a 4-wide node of axis a's near-plane row (bmin[a], or bmax[a] when inv[a] < 0)
    float a;       // |d|^2
    float ia;      // ~1/|d|^2
    float on;      // |o| (rounded up)
    float dn;      // |d| (rounded up)
};

__device__ __forceinline__ FRay make_fray(V3 o, V3 d) {
    RT_FP32_FUSED
    FRay f;
    f.o[0] = o.x; f.o[1] = o.y; f.o[2] = o.z;
    f.d[0] = d.x; f.d[1] = d.y; f.d[2] = d.z;
    float m = 0.0f, mall = 0.0f;
    const float dmax = ::fmaxf(::fmaxf(::fabsf(d.x), ::fabsf(d.y)), ::fabsf(d.z));
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float c = f.d[a];
        const float cc = ::fabsf(c) < 1e-30f ? ::copysignf(1e-30f, c) : c;
        f.inv[a] = __builtin_amdgcn_rcpf(cc);  // <= 1 ulp: a common factor of an axis' two planes
        f.noi[a] = -(f.o[a] * f.inv[a]);
        const float an = ::fabsf(f.noi[a]);
        mall = ::fmaxf(mall, an);
        // near-parallel axes (|d_a| < 1e-3 max|d|) stay out of eps (an exact zero
        // component, inv = 1e30, made eps ~1e24 and every box accepted). Their planes need no
        // absolute slack: the fused error is u|o_a inv_a| + relative terms, and for a face b
        // either |o_a| <= 4 (1 + |b|), where the box's outward padding of 1e-6 (1 + |b|)
        // (scene_tree.cpp make_fast_nodes) is >= 2u|o_a| in coordinates, so the padded face's computed
        // t stays outside the unpadded face's exact t; or |o_a| > 4 (1 + |b|), where
        // |t_a| = |b - o_a| |inv_a| >= 0.75 |o_a inv_a| and the error is relative, <= 2.7u |t_a|,
        // inside slab_accept's relative 2e-6 (~33u) with the rcp and fma roundings (~3u).
        m = ::fabsf(c) >= 1e-3f * dmax ? ::fmaxf(m, an) : m;
        f.nrow[a] = 16 * a + (f.inv[a] < 0.0f ? 48 : 0);
    }
    // 1e-6 * max|o * inv| ~ 16 u: covers the rounding of o * inv at both ends of the interval
    f.eps = m * 1e-6f;
    f.a = d.x * d.x + d.y * d.y + d.z * d.z;
    f.ia = __builtin_amdgcn_rcpf(f.a);
    f.dn = __builtin_amdgcn_sqrtf(f.a) * (1.0f + kRel);
    f.pthr = 1e-3f * f.dn;
    if (!(mall < 1e37f)) {  // o * inv overflowed (|o| > ~1e7 with an axis-parallel d): cull nothing
#pragma unroll
        for (int a = 0; a < 3; ++a) f.inv[a] = f.noi[a] = 0.0f;
        f.eps = __builtin_inff();
        f.pthr = __builtin_inff();  // and every axis quad is decided exactly
    }
    f.on = __builtin_amdgcn_sqrtf(o.x * o.x + o.y * o.y + o.z * o.z) * (1.0f + kRel);
    return f;
}

// The slab test's entry / exit parameter of the plane x_a = b: t = fma(b, inv, -o*inv), one
// FMA instead of (b - o) * inv. The unfused form's error is relative to |t|; the fused one's
// is absolute, |err| <= u (|o * inv| + |t|): the rounding of o * inv (FRay::noi) and the
// final one, u = 2^-24. The acceptance test tn <= tf * 1.000002 + eps covers it: the u|t|
// part is inside the relative 2e-6 (tn and tf are both positive whenever the box can hold a
// hit, t > 0.001), the u|o * inv| part of either end inside eps = 1e-6 max_a |o_a inv_a|
// (~16 u). On top of that every box is padded by 1e-6 (1 + |b|) (scene_tree.cpp make_fast_nodes),
// the margin the unfused test already relied on for the exact hit point.
// A ray whose o * inv overflows gets inv = noi = 0, eps = inf: t = 0 on every plane (NaN
// on an infinite bound, which fminf / fmaxf ignore), tf = min(thi, 0) >= 0, and the test
// accepts every box - still the reference's hit, at brute-force cost (|o| > ~1e7 only).
__device__ __forceinline__ float slab_t(float b, const FRay& f, int a) { return __builtin_fmaf(b, f.inv[a], f.noi[a]); }
// Two-float vectors for packed fp32 (v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32: one instruction
// for both elements, the same IEEE operation on each); operand pairs in aligned register pairs,
// broadcast scalars by op_sel.
typedef float pf2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ pf2 pf2_of(float x) { return pf2{x, x}; }
__device__ __forceinline__ pf2 pf2_fma(pf2 a, pf2 b, pf2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ pf2 pf2_abs(pf2 a) { return __builtin_elementwise_abs(a); }
__device__ __forceinline__ bool slab_accept(float tn, float tf, const FRay& f) {
    return tn <= __builtin_fmaf(tf, 1.000002f, f.eps);
}

template <class R>
__device__ __forceinline__ bool slab(const RtNode& n, const R& f, float thi, float& tnear) {
    if (n.bmin[0] != n.bmin[0]) return false;  // box the reference can never enter
    float tn = kTminLo, tf = thi;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float t0 = slab_t(n.bmin[a], f, a);
        const float t1 = slab_t(n.bmax[a], f, a);
        tn = ::fmaxf(tn, ::fminf(t0, t1));
        tf = ::fminf(tf, ::fmaxf(t0, t1));
    }
    tnear = tn;
    return slab_accept(tn, tf, f);
}

// 4-wide node `ref` where the walk reads it: the blob (global, 128-byte nodes) or the LDS copy,
// where each node is followed by a 16-byte pad row (scene_prologue). A ds_read_b128 serves 16
// lanes per LDS cycle, 16 bytes each, from bank (address / 4) mod 64: with 128-byte nodes, row r
// of node i sits at bank 32 i + 4 r (mod 64), only two bank windows for the 16 lanes reading that
// row of their (different) nodes - up to 8-way conflicts (spheres-500: 40 % of the LDS-array
// cycles were bank conflicts, SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE). At 144 bytes the
// window is 36 i + 4 r: 16 distinct windows for i mod 16.
// A launch that walks the tree from global memory (LDSS 0: spheres-100k's 2.8 MB of nodes) keeps
// the tree's top - the first n_top nodes in breadth-first order, the part every walk starts with -
// in LDS beside the stack (t4_step reads a node from there or from global memory: two loads in two
// branches, so each stays a ds_read / global_load - one generic pointer made them flat loads,
// 3.5 % slower on spheres-100k).
// (a 24-bit multiply, full rate: node indices stay below 2^24, scene_tree.cpp make_t4nodes)
__device__ __forceinline__ const RtT4Node* t4_node(const DevScene& S, int ref) {
    return reinterpret_cast<const RtT4Node*>(reinterpret_cast<const char*>(S.t4nodes) +
                                             (size_t)__umul24((unsigned)ref, (unsigned)S.t4_stride));
}
struct T4Rows {
    float4 nr[3], fr[3];  // per axis: the four children's near-plane / far-plane coordinates
    int4 rf;
};
// A node's rows through a pointer of address space AS (1 global, 3 LDS, 0 generic: whatever the
// compiler infers): typed loads of distinct address spaces in the two branches of t4_step cannot
// be merged into one flat load. The ray's direction signs pick which row of each axis is the near
// plane (FRay::nrow): the slab test then needs no min / max per plane pair (below).
template <int AS>
__device__ __forceinline__ void t4_rows(const void* nd0, const FRay& f, bool nf, T4Rows& R) {
    typedef float v4 __attribute__((ext_vector_type(4)));
    typedef const __attribute__((address_space(AS))) v4* P4;
    typedef const __attribute__((address_space(AS))) char* PC;
    const PC b = (PC)__builtin_assume_aligned(nd0, 16);
    auto f4 = [](v4 v) { return make_float4(v.x, v.y, v.z, v.w); };
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int nrow = nf ? f.nrow[a] : 16 * a;
        R.nr[a] = f4(*(P4)(b + nrow));
        R.fr[a] = f4(*(P4)(b + (32 * a + 48 - nrow)));  // the other row of axis a
    }
    const v4 r = *(P4)(b + 96);
    R.rf = make_int4(__float_as_int(r.x), __float_as_int(r.y), __float_as_int(r.z), __float_as_int(r.w));
}

// One step of the 4-wide walk (RtT4Node) at node `nd`: the slab tests of its four children,
// the nearest hit child is returned as the next reference and the other hit children are
// pushed farthest first (so the nearer pop first); with no hit child the next reference is
// popped (kTravDone when the stack is empty). Branch-free:
//  * each child's key is its entry distance's bits (a positive float orders as its bits), or
//    ~0 for a miss / empty slot; (key, reference) pairs go through a 5-exchange network
//    (one compare, min / max of the keys, two selects of the references per exchange).
//    (Round 4 also tried keys carrying the child index in their low two bits, sorted alone
//    with min / max and the references re-read from the node afterwards: 4 dependent loads
//    per step - spheres-100k, whose tree is walked from global memory, lost 14 %.)
//  * with n hit children the pairs s1..s3 are written in the order s3, s2, s1 at stack
//    positions sp + max(n - 1 - j, 0), so s_{n-1} .. s1 land at sp .. sp + n - 2 and the
//    writes of missed children land at sp, overwritten or above the new top. No write
//    goes past sp + 2: at a node of level L (root 1) the stack holds at most 3 (L - 1)
//    entries (3 per ancestor), so writes stay below 3 t4depth <= stack_depth - 2 entries
//    (scene.cpp: stack_depth = max(..., 3 t4depth + 1) + 1).
// The pair sort and stack pushes of a 4-wide node step (below): keys k (entry-distance bits, ~0
// for a miss), child references r, n hit children.
template <int STRIDE, class SK>
__device__ __forceinline__ int t4_push(uint32_t (&k)[4], int (&r)[4], int n, SK* stk, int& sp) {
    auto cx = [&](int i, int j) {
        const bool sw = k[j] < k[i];
        const uint32_t lo = min(k[i], k[j]), hi = max(k[i], k[j]);
        const int ri = r[i], rj = r[j];
        k[i] = lo;
        k[j] = hi;
        r[i] = sw ? rj : ri;
        r[j] = sw ? ri : rj;
    };
    cx(0, 1); cx(2, 3); cx(0, 2); cx(1, 3); cx(1, 2);
    const int popped = stk[max(sp - 1, 0) * STRIDE];
#pragma unroll
    for (int j = 3; j >= 1; --j) stk[max(sp + n - 1 - j, sp) * STRIDE] = (SK)r[j];
    const int next = n > 0 ? r[0] : (sp > 0 ? popped : kT4Empty);  // (kT4Empty = kTravDone)
    sp = n > 0 ? sp + n - 1 : max(sp - 1, 0);
    return next;
}

template <int STRIDE, class SK>
__device__ __forceinline__ int t4_step(const DevScene& S, int ref, const FRay& f, float thi, SK* stk, int& sp) {
    T4Rows R;
    const bool nf = S.nearfar;
    if (ref < S.n_top) t4_rows<3>(S.top_lds + (size_t)ref * (sizeof(RtT4Node) + 16), f, nf, R);
    else if (S.n_top > 0) t4_rows<1>(t4_node(S, ref), f, nf, R);  // (LDSS 0: the rest is in global memory)
    else t4_rows<0>(t4_node(S, ref), f, nf, R);
    const float bn[3][4] = {{R.nr[0].x, R.nr[0].y, R.nr[0].z, R.nr[0].w}, {R.nr[1].x, R.nr[1].y, R.nr[1].z, R.nr[1].w},
                            {R.nr[2].x, R.nr[2].y, R.nr[2].z, R.nr[2].w}};
    const float bf[3][4] = {{R.fr[0].x, R.fr[0].y, R.fr[0].z, R.fr[0].w}, {R.fr[1].x, R.fr[1].y, R.fr[1].z, R.fr[1].w},
                            {R.fr[2].x, R.fr[2].y, R.fr[2].z, R.fr[2].w}};
    const int cr[4] = {R.rf.x, R.rf.y, R.rf.z, R.rf.w};
    uint32_t k[4];
    int r[4];
    int n = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        // near / far plane t per axis: the same two values min / max would pick (fma is monotone
        // in b for a fixed inv, so the sign of inv orders the planes; a NaN plane - an infinite
        // bound times inv = 0 - is ignored by fmaxf / fminf either way). (Round 6: the 24 plane
        // FMAs as 12 packed v_pk_fma_f32 ran 1.2-2.4 % slower on the BVH configs, profiles/r06/pairs/.)
        float tn = kTminLo, tf = thi;
        if (nf) {
            tn = ::fmaxf(::fmaxf(::fmaxf(slab_t(bn[0][c], f, 0), slab_t(bn[1][c], f, 1)), slab_t(bn[2][c], f, 2)), tn);
            tf = ::fminf(::fminf(::fminf(slab_t(bf[0][c], f, 0), slab_t(bf[1][c], f, 1)), slab_t(bf[2][c], f, 2)), tf);
        } else {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float t0 = slab_t(bn[a][c], f, a);
                const float t1 = slab_t(bf[a][c], f, a);
                tn = ::fmaxf(tn, ::fminf(t0, t1));
                tf = ::fminf(tf, ::fmaxf(t0, t1));
            }
        }
        const bool hit = (cr[c] != kT4Empty) & slab_accept(tn, tf, f);
        k[c] = hit ? __float_as_uint(tn) : ~0u;
        r[c] = cr[c];
        n += hit ? 1 : 0;
    }
    return t4_push<STRIDE>(k, r, n, stk, sp);
}

// fp32 pre-filters: false only when the exact test surely gives no t <= thi.
// The sphere roots' absolute error bound, kRel (|oc| |d| + |b| + sq) / a (+ a denormal floor),
// with |oc| |d| bounded without a square root (round 4: one v_sqrt fewer per test): a |oc|^2 =
// b^2 - disc + a r^2, and the exact disc >= -2 tol once the computed one passed -tol (its
// rounding is far below tol), so |oc| |d| <= |b| + |d| r + sqrt(2 tol) <= |b| + dn r + 1.5 sq
// (sq >= sqrt(tol)); the bound used, kRel (2 |b| + dn r + 3 sq) / a, is never smaller.
__device__ __forceinline__ float sphere_et(float b, float r, float sq, const FRay& f) {
    RT_FP32_FUSED
    return kRel * (2.0f * ::fabsf(b) + f.dn * r + 3.0f * sq) * f.ia + 1e-30f;
}
__device__ __forceinline__ bool sphere_maybe(float4 g, const FRay& f, float thi, float& lo) {
    RT_FP32_FUSED
    const float ox = f.o[0] - g.x, oy = f.o[1] - g.y, oz = f.o[2] - g.z;  // = the reference's oc
    const float b = ox * f.d[0] + oy * f.d[1] + oz * f.d[2];
    const float r = g.w;
    const float oo = ox * ox + oy * oy + oz * oz;
    const float disc = b * b - f.a * (oo - r * r);
    // every term of disc is bounded by a*(|oc|^2 + r^2) (b^2 <= a|oc|^2); the
    // bound holds through the cancellation of |oc|^2 - r^2 for rays leaving the surface
    const float tol = 4.0f * kRel * f.a * (oo + r * r) + 1e-30f;
    if (disc < -tol) return false;
    const float sq = __builtin_amdgcn_sqrtf(::fmaxf(disc, 0.0f) + tol) * (1.0f + kRel);
    const float et = sphere_et(b, r, sq, f);
    if ((-b + sq) * f.ia * (1.0f + kRel) + et < kTminLo) return false;
    const float r1 = (-b - sq) * f.ia;
    lo = r1 - ::fabsf(r1) * kRel - et;  // <= the first root; the second is larger
    if (lo > thi) return false;
    return true;
}

// sphere_maybe plus, when the sphere is SURELY hit at some t > 0.001 (the exact
// discriminant is positive and the larger root exceeds tMin under the same error
// model), an upper bound `hi` of the t the exact test will return (+inf otherwise).
// A surely-hit candidate's `hi` may cull the walk before its exact test runs.
__device__ __forceinline__ bool sphere_maybe_hi(float4 g, const FRay& f, float thi, float& lo, float& hi) {
    RT_FP32_FUSED
    const float ox = f.o[0] - g.x, oy = f.o[1] - g.y, oz = f.o[2] - g.z;
    const float b = ox * f.d[0] + oy * f.d[1] + oz * f.d[2];
    const float r = g.w;
    const float oo = ox * ox + oy * oy + oz * oz;
    const float disc = b * b - f.a * (oo - r * r);
    const float tol = 4.0f * kRel * f.a * (oo + r * r) + 1e-30f;
    if (disc < -tol) return false;
    const float sq = __builtin_amdgcn_sqrtf(::fmaxf(disc, 0.0f) + tol) * (1.0f + kRel);
    const float et = sphere_et(b, r, sq, f);
    const float hi2 = (-b + sq) * f.ia * (1.0f + kRel) + et;  // >= every root
    if (hi2 < kTminLo) return false;
    const float r1 = (-b - sq) * f.ia;
    lo = r1 - ::fabsf(r1) * kRel - et;  // <= the first root; the second is larger
    if (lo > thi) return false;
    hi = __builtin_inff();
    const float dm = disc - tol;  // <= the exact discriminant
    if (dm > 0.0f) {
        const float sql = __builtin_amdgcn_sqrtf(dm) * (1.0f - kRel);  // <= its square root
        const float r2 = (-b + sql) * f.ia;
        const float r2lo = r2 - ::fabsf(r2) * kRel - et;                // <= the larger root
        if (r2lo > 0.001f * (1.0f + 1e-5f)) hi = hi2 * (1.0f + 4e-6f) + 1e-30f;
    }
    return true;
}

template <bool QUAD>
__device__ __forceinline__ bool planar_maybe(const RtPrim& p, const FRay& f, float thi, float& lo) {
    RT_FP32_FUSED
    const float nx = p.g3[0], ny = p.g3[1], nz = p.g3[2];
    const float denom = nx * f.d[0] + ny * f.d[1] + nz * f.d[2];
    lo = kTminLo;
    if (!(::fabsf(denom) > 1e-3f * f.dn)) return true;  // near-parallel: decide exactly
    const float no = nx * f.o[0] + ny * f.o[1] + nz * f.o[2];
    const float D = p.g0[3];
    const float idn = __builtin_amdgcn_rcpf(denom);
    const float t = (D - no) * idn;
    // |n| = 1: num error <= kRel(|D| + |o|), denominator error <= kRel|d| (< 1% of |denom|)
    const float et = (kRel * (::fabsf(D) + f.on) + 2.0f * kRel * f.dn * ::fabsf(t)) * ::fabsf(idn) +
                     kRel * ::fabsf(t) + 1e-30f;
    if (t + et < kTminLo || t - et > thi) return false;
    lo = t - et;
    if (!QUAD) return true;
    const float px = f.o[0] + t * f.d[0] - p.g0[0];
    const float py = f.o[1] + t * f.d[1] - p.g0[1];
    const float pz = f.o[2] + t * f.d[2] - p.g0[2];
    const float ux = p.g1[0], uy = p.g1[1], uz = p.g1[2];
    const float vx = p.g2[0], vy = p.g2[1], vz = p.g2[2];
    const float wx = p.g4[0], wy = p.g4[1], wz = p.g4[2];
    // alpha = w . (ph x v), beta = w . (u x ph)
    const float alpha = wx * (py * vz - pz * vy) + wy * (pz * vx - px * vz) + wz * (px * vy - py * vx);
    const float beta = wx * (uy * pz - uz * py) + wy * (uz * px - ux * pz) + wz * (ux * py - uy * px);
    // hit-point error (t error, Ray.at's and ph's roundings) times |w||v| / |w||u| (scene.cpp)
    const float dp = et * f.dn + kRel * (f.on + ::fabsf(t) * f.dn + ::fabsf(p.g0[0]) + ::fabsf(p.g0[1]) +
                                         ::fabsf(p.g0[2]) + ::fabsf(px) + ::fabsf(py) + ::fabsf(pz));
    const float ea = p.g2[3] * dp + 1e-4f, eb = p.g1[3] * dp + 1e-4f;
    if (alpha < -ea || alpha > 1.0f + ea || beta < -eb || beta > 1.0f + eb) return false;
    return true;
}

// Exact candidate t (reference arithmetic) of primitive p on (0.001, inf).
__device__ __forceinline__ void count_exact(uint32_t* cnt) {
    cnt[CT_EXACT]++;
    const unsigned long long m = __ballot(1);
    if ((int)(threadIdx.x & 63) == __builtin_ctzll(m)) cnt[CT_EXACT_WAVE]++;
}

template <class Real, bool COUNT>
__device__ __forceinline__ bool prim_candidate(const RtPrim& p, const RayK<Real>& r, const FRay& f, float thi,
                                               Real& t, uint32_t* cnt) {
    const Real inf = (Real)__builtin_inf();
    float lo;
    if (p.type == PRIM_SPHERE) {
        if (COUNT) cnt[CT_SPHERE]++;
        if (!sphere_maybe(make_float4(p.g0[0], p.g0[1], p.g0[2], p.g0[3]), f, thi, lo)) return false;
        if (COUNT) count_exact(cnt);
        return sphere_t<Real>(p, r, K<Real>::TMIN, inf, t);
    }
    if (p.type == PRIM_QUAD) {
        if (COUNT) cnt[CT_QUAD]++;
        const int code = aquad_code(p);
        if (code != 0) {
            if (!aquad_maybe(p, code, f.o, f.d, f.dn, thi, lo)) return false;
            if (COUNT) count_exact(cnt);
            return aquad_t<Real>(p, code, r.o, r.d, K<Real>::TMIN, inf, t);
        }
        if (!planar_maybe<true>(p, f, thi, lo)) return false;
        if (COUNT) count_exact(cnt);
        return planar_t<Real, true>(p, r, K<Real>::TMIN, inf, t);
    }
    if (COUNT) cnt[CT_PLANE]++;
    if (!planar_maybe<false>(p, f, thi, lo)) return false;
    return planar_t<Real, false>(p, r, K<Real>::TMIN, inf, t);
}

template <class Real>
__device__ __forceinline__ float upper_f(Real t) {
    RT_FP32_FUSED
    // fp32 value >= t (rounded up with margin) used to cull against the best hit.
    const float x = (float)t;
    return x + ::fabsf(x) * 4e-6f + 1e-30f;
}

// `stk`: this lane's column of the LDS node stack.
// Walks the 4-wide tree (RtT4Node) from S.t4root after one slab test of the root box: a node
// step (t4_step) reads one 128-byte node and tests its four children's boxes; the nearest hit
// child is taken, the other hit children are pushed farthest first. Stack entries hold a node
// reference only: a popped subtree is culled one level later by its children's slab tests
// against the best hit so far. The result is the (t, slot) minimum over the leaves reached.
//
// Lanes of a wave reach leaves at different steps. Node steps and leaf tests run as two
// separate loops: a lane that reaches a leaf
// parks it and keeps walking nodes until every lane still walking holds a
// parked leaf, then the wave tests leaves together - otherwise nearly every
// node step would also pay for some lane's (four times longer) leaf test.
// Node steps taken while a leaf is parked cull with a possibly stale bound;
// that only costs extra node tests (the answer is the (t, slot) minimum).
constexpr int kTravDone = (int)0x80000000;  // no node / leaf (leaf refs are ~v, v < 2^31 - 1)

// Deferred exact sphere tests (DEFER, TRAV_FAST_DEFER kernels): a leaf's sphere that passes the
// fp32 pre-filter becomes this lane's PENDING candidate instead of being tested
// exactly on the spot - lanes reach leaves at different steps, so an in-loop
// fp64 test ran with a handful of active lanes (spheres-100k: 14 wave-level
// exact blocks per ray-trip for 1.0 tests per ray). A surely-hit candidate's
// upper bound culls the walk meanwhile; a second candidate resolves the first;
// the walk's end resolves the last, batched over the lanes finishing together.
// Exact t and the (t, slot) minimum are unchanged.
template <class Real, bool COUNT>
__device__ __forceinline__ void resolve_pending(const DevScene& S, const RayK<Real>& r, float& thi, Real& best_t,
                                                int& best, int& pk, uint32_t* cnt) {
    // (pk < 0: nothing pending)
    if (pk >= 0) {
        if (COUNT) count_exact(cnt);
        Real t;
        if (sphere_t<Real>(S.prims[pk], ray_at_use<Real>(r), K<Real>::TMIN, (Real)__builtin_inf(), t) &&
            (t < best_t || (t == best_t && pk < best))) {
            best_t = t;
            best = pk;
            thi = ::fminf(thi, upper_f<Real>(t));
        }
        pk = -1;
    }
}

// A leaf's primitives in leaf order: the fp32 pre-filter from the compact leaf-order record, then
// the exact test (or, with DEFER, the pending-candidate rule). L2 (trees walked from global memory):
// one 32-byte record per primitive (S.tsph2) that also carries the fp64 radius and the
// slot, so a sphere's exact test needs no dependent tprims -> RtPrim loads (two L2 round trips).
// (Round 5 also tried loading a leaf's four records before its first test, and loading a
// parked leaf's record when it is parked: spheres-100k 37.1 -> 44.8 and 30.0 -> 36.0 ms,
// profiles/r05/coop_v2_prefetch/, leaf_pre/ - dropped.)
template <class Real, bool COUNT, bool DEFER, bool L2 = false>
__device__ __forceinline__ void leaf_test(const DevScene& S, int ref, const RayK<Real>& r, const FRay& f, float& thi,
                                          Real& best_t, int& best, int& pk, float& plo, uint32_t* cnt) {
    const int v = ~ref;
    const int first = v >> 3;
    const int end = first + (v & 7);
    for (int m = first; m < end; ++m) {
        if constexpr (L2 && !DEFER) {
            const RtLeafSph q = S.tsph2[m];
            Real t;
            bool cand;
            if (q.r32 == q.r32) {  // sphere
                if (COUNT) cnt[CT_SPHERE]++;
                float lo;
                if (!sphere_maybe(make_float4(q.c[0], q.c[1], q.c[2], q.r32), f, thi, lo)) continue;
                if (COUNT) count_exact(cnt);
                cand = sphere_t_cr<Real>(v3(q.c[0], q.c[1], q.c[2]), sizeof(Real) == 8 ? (Real)q.r64 : (Real)q.r32,
                                         ray_at_use<Real>(r), K<Real>::TMIN, (Real)__builtin_inf(), t);
            } else {
                cand = prim_candidate<Real, COUNT>(S.prims[q.slot], ray_at_use<Real>(r), f, thi, t, cnt);
            }
            if (cand && (t < best_t || (t == best_t && q.slot < best))) {
                best_t = t;
                best = q.slot;
                thi = ::fminf(thi, upper_f<Real>(t));
            }
            continue;
        }
        const float4 g = S.tsph[m];
        Real t;
        int k;  // reference leaf slot (the tie-break key)
        bool cand;
        if (g.w == g.w) {  // sphere: pre-filter from the compact leaf-order record
            if (COUNT) cnt[CT_SPHERE]++;
            float lo;
            if constexpr (DEFER) {
            float hi;
            if (!sphere_maybe_hi(g, f, thi, lo, hi)) continue;
            k = S.tprims[m];
            // a second candidate: one surely hit before the pending one's lower bound
            // replaces it untested (t_new <= hi < plo <= t_pending); otherwise the
            // pending one is settled first
            if (pk >= 0 && !(hi < plo)) resolve_pending<Real, COUNT>(S, r, thi, best_t, best, pk, cnt);
            if (lo <= thi) {
                pk = k;
                plo = lo;
                thi = ::fminf(thi, hi);
            }
            continue;
            } else {
            if (!sphere_maybe(g, f, thi, lo)) continue;
            if (COUNT) count_exact(cnt);
            k = S.tprims[m];
            cand = sphere_t<Real>(S.prims[k], ray_at_use<Real>(r), K<Real>::TMIN, (Real)__builtin_inf(), t);
            }
        } else {
            k = S.tprims[m];
            cand = prim_candidate<Real, COUNT>(S.prims[k], ray_at_use<Real>(r), f, thi, t, cnt);
        }
        if (cand && (t < best_t || (t == best_t && k < best))) {
            best_t = t;
            best = k;
            thi = ::fminf(thi, upper_f<Real>(t));
        }
    }
}

template <class Real, bool COUNT, bool DEFER, class SK>
__device__ __forceinline__ int closest_hit_fast(const DevScene& S, const RayK<Real>& r, Real& t_hit, SK* stk,
                                                uint32_t* cnt) {
    const FRay f = make_fray(r.o, r.d);
    Real best_t = (Real)__builtin_inf();
    int best = -1;
    int pk = -1;  // pending (deferred) exact sphere test
    float plo = 0.0f;  // its lower bound
    float thi = __builtin_inff();
    float tn0;
    if (COUNT) cnt[CT_NODE]++;
    if (!slab(S.root_box, f, thi, tn0)) {
        t_hit = best_t;
        return -1;
    }
    int sp = 0;
    // next stacked entry (kTravDone when the stack is empty)
    auto pop = [&]() -> int {
        if (sp > 0) {
            --sp;
            return stk[sp * kStackStride];
        }
        return kTravDone;
    };
    // one 4-wide node step: the nearest hit child is next, the other hit
    // children are pushed farthest first (so the nearer pop first)
    auto node_step = [&](int ref) -> int {
        if (COUNT) cnt[CT_NODE] += 4;
        return t4_step<kStackStride>(S, ref, f, thi, stk, sp);
    };
    int ref = S.t4root;
    int leaf = kTravDone;  // parked leaf
    while (ref != kTravDone || leaf != kTravDone) {
        while (ref >= 0) {
            ref = node_step(ref);
            if (ref < 0 && ref != kTravDone && leaf == kTravDone) {
                leaf = ref;
                ref = pop();
            }
            if (__ballot(leaf == kTravDone) == 0ull) break;  // every walking lane holds a leaf
        }
        if (leaf == kTravDone && ref != kTravDone) {  // the walk stopped on a leaf (or started on one)
            leaf = ref;
            ref = pop();
        }
        while (leaf != kTravDone) {
            leaf_test<Real, COUNT, DEFER>(S, leaf, r, f, thi, best_t, best, pk, plo, cnt);
            leaf = kTravDone;
            if (ref < 0 && ref != kTravDone) {  // the walk also stopped on a leaf
                leaf = ref;
                ref = pop();
            }
        }
    }
    resolve_pending<Real, COUNT>(S, r, thi, best_t, best, pk, cnt);  // the whole wave at once
    t_hit = best_t;
    return best;
}

// ---------------------------------------------------------------------------
// Resumable fast traversal (chunked kernel). closest_hit_fast keeps
// the whole wave in its loop until the lane with the longest walk is done - a
// ray grazing a field of spheres can need ten times the mean node visits, and
// every other lane idles meanwhile. Here a lane's walk state persists across
// the wave's loop iterations: the wave walks until `min_ready` of its lanes are
// done, they shade and start their next rays, and the long walks continue next
// to them. Same walk (culling, parked leaves, (t, slot) minimum) as
// closest_hit_fast, so the same hit.
// ---------------------------------------------------------------------------
template <class Real>
struct FastWalk {
    int ref, leaf, sp, best;
    int pk;     // pending (deferred) exact sphere test, resolved by fast_walk_resolve
    float plo;  // its lower bound
    float thi;
    Real best_t;
};

template <class Real, bool COUNT>
__device__ __forceinline__ void fast_walk_begin(const DevScene& S, V3 o, V3 d, FastWalk<Real>& W, uint32_t* cnt) {
    const FRay f = make_fray(o, d);
    W.best_t = (Real)__builtin_inf();
    W.best = -1;
    W.thi = __builtin_inff();
    W.sp = 0;
    W.pk = -1;
    W.leaf = kTravDone;
    float tn0;
    if (COUNT) cnt[CT_NODE]++;
    W.ref = slab(S.root_box, f, W.thi, tn0) ? S.t4root : kTravDone;
}

// Called by the whole wave with uniform control flow; lanes with `walking`
// advance their walks. Returns when no lane walks, or (unless `drain`) after at
// least one round once `min_ready` lanes of the wave are not walking.
template <class Real, bool COUNT, bool DEFER, bool PROF = false, int STRIDE = kStackStride, bool L2 = false,
          class SK = int>
__device__ __forceinline__ void fast_walk_rounds(const DevScene& S, V3 o, V3 d, FastWalk<Real>& W, bool& walking,
                                                 SK* stk, int min_ready, bool drain, uint32_t* cnt, Prof* pf = nullptr) {
    const FRay f = make_fray(o, d);
    const RayK<Real> r = make_ray<Real>(o, d);
    int rounds = 0;
    while (true) {
        const unsigned long long wm = __ballot(walking);
        if (wm == 0ull) break;
        if (rounds > 0 && !drain && kWave - __popcll(wm) >= min_ready) break;
        ++rounds;
        if (walking) {
            int sp = W.sp;
            float thi = W.thi;
            auto pop = [&]() -> int {
                if (sp > 0) {
                    --sp;
                    return stk[sp * STRIDE];
                }
                return kTravDone;
            };
            auto node_step = [&](int ref) -> int {
                if (COUNT) cnt[CT_NODE] += 4;
                return t4_step<STRIDE>(S, ref, f, thi, stk, sp);
            };
            // one round of closest_hit_fast's parked-leaf walk
            int ref = W.ref, leaf = W.leaf;
            while (ref >= 0) {
                if (PROF) pcount<PROF>(*pf, PR_NODE);
                ref = node_step(ref);
                if (ref < 0 && ref != kTravDone && leaf == kTravDone) {
                    leaf = ref;
                    ref = pop();
                }
                if (__ballot(leaf == kTravDone) == 0ull) break;  // every walking lane holds a leaf
            }
            if (PROF) psec<PROF>(*pf, PR_WNODE);
            if (leaf == kTravDone && ref != kTravDone) {
                leaf = ref;
                ref = pop();
            }
            while (leaf != kTravDone) {
                if (PROF) pcount<PROF>(*pf, PR_LEAF);
                leaf_test<Real, COUNT, DEFER, L2>(S, leaf, r, f, thi, W.best_t, W.best, W.pk, W.plo, cnt);
                leaf = kTravDone;
                if (ref < 0 && ref != kTravDone) {
                    leaf = ref;
                    ref = pop();
                }
            }
            if (PROF) psec<PROF>(*pf, PR_WLEAF);
            W.ref = ref;
            W.leaf = leaf;
            W.sp = sp;
            W.thi = thi;
            if (ref == kTravDone && leaf == kTravDone) walking = false;
        }
    }
}

// The exact test of a finished walk's pending candidate (called by the lanes whose
// walks ended, together, before they shade).
template <class Real, bool COUNT>
__device__ __forceinline__ void fast_walk_resolve(const DevScene& S, V3 o, V3 d, FastWalk<Real>& W, uint32_t* cnt) {
    const RayK<Real> r = make_ray<Real>(o, d);
    resolve_pending<Real, COUNT>(S, r, W.thi, W.best_t, W.best, W.pk, cnt);
}

}  // namespace rt
