// Brute-force closest hit for small scenes (pre-filter pass + nearest-first exact tests), and
// closest_hit_any, the dispatch over the three traversals.
#pragma once

#include <hip/hip_runtime.h>

#include "pt_walk.hpp"

namespace rt {

// Small scenes: test every primitive in leaf order. The answer is the same
// lexicographic minimum of (t, leaf slot) the fast traversal returns (valid
// under the same condition, SceneBuild::fast_ok). The loop bound and the
// primitive index are wave-uniform, so primitive records come through scalar
// loads and no lane waits on a BVH stack.
template <class Real, bool COUNT>
__device__ __forceinline__ int closest_hit_brute(const DevScene& S, int n_prims, const RayK<Real>& r, Real& t_hit,
                                                 uint32_t* cnt) {
    const FRay f = make_fray(r.o, r.d);
    Real best_t = (Real)__builtin_inf();
    int best = -1;
    float thi = __builtin_inff();
    for (int k = 0; k < n_prims; ++k) {
        Real t;
        const RtPrim p = ld_uniform(S.gprims, k);
        if (prim_candidate<Real, COUNT>(p, r, f, thi, t, cnt) && t < best_t) {
            best_t = t;
            best = k;
            thi = upper_f<Real>(t);
        }
    }
    t_hit = best_t;
    return best;
}

// Nearest-first brute force (up to kBruteMaxPrims primitives). The loop above runs primitive
// k's exact test whenever ANY lane of the wave needs it - lanes hit different
// walls, so a wave executes nearly every primitive's exact test per ray while
// each lane needs about one. Here pass 1 (wave-uniform, scalar primitive
// loads) only runs the fp32 pre-filters and keeps, per lane, the candidate set
// and each candidate's lower bound on t (in this lane's LDS column `lot`).
// Pass 2 exact-tests each lane's candidates nearest-first through one
// type-generic code path per primitive type, and stops once the nearest
// remaining lower bound lies beyond the best hit. Same (t, slot) minimum.
template <bool COUNT>
__device__ __forceinline__ bool prim_maybe(const RtPrim& p, const FRay& f, float& lo, uint32_t* cnt) {
    const float thi = __builtin_inff();
    if (p.type == PRIM_SPHERE) {
        if (COUNT) cnt[CT_SPHERE]++;
        return sphere_maybe(make_float4(p.g0[0], p.g0[1], p.g0[2], p.g0[3]), f, thi, lo);
    }
    if (p.type == PRIM_QUAD) {
        if (COUNT) cnt[CT_QUAD]++;
        const int code = aquad_code(p);
        if (code != 0) return aquad_maybe(p, code, f.o, f.d, f.dn, thi, lo);
        return planar_maybe<true>(p, f, thi, lo);
    }
    if (COUNT) cnt[CT_PLANE]++;
    return planar_maybe<false>(p, f, thi, lo);
}

// The reference's exact t of primitive p on (0.001, inf); per-lane p.
template <class Real>
__device__ __forceinline__ bool prim_exact(const RtPrim& p, const RayK<Real>& r, Real& t) {
    const Real inf = (Real)__builtin_inf();
    if (p.type == PRIM_SPHERE) return sphere_t<Real>(p, r, K<Real>::TMIN, inf, t);
    if (p.type == PRIM_QUAD) {
        const int code = aquad_code(p);
        if (code != 0) return aquad_t_rt<Real>(p, code, r.o, r.d, K<Real>::TMIN, inf, t);
        return planar_t<Real, true>(p, r, K<Real>::TMIN, inf, t);
    }
    return planar_t<Real, false>(p, r, K<Real>::TMIN, inf, t);
}

// The record's two 16-byte loads, issued together and waited for once: the empty asm takes the
// loaded words as its operands, so the loads cannot sink to their first uses (the compiler did
// that: kind, then s0, then the fields - dependent round trips again).
__device__ __forceinline__ RtExact xrec_load(const RtExact* px) {
    typedef uint32_t u4 __attribute__((ext_vector_type(4)));
    const u4* src = reinterpret_cast<const u4*>(px);
    u4 w0 = src[0], w1 = src[1];
    __asm__ volatile("" : "+v"(w0), "+v"(w1));
    struct W {
        u4 a, b;
    } w{w0, w1};
    return __builtin_bit_cast(RtExact, w);
}
// The nearest-first pass's exact test, from the primitive's RtExact record: prim_exact's
// operations on the same operands (the record holds the RtPrim fields aquad_t_c / sphere_t
// read), with the sphere's root and the axis-aligned quad's plane t through ONE division -
// lanes of a wave test different primitive types, and each type's block costs the whole wave;
// the prologues stay per type, the division (the longest piece of either) is shared: sphere_t's
// (-h - sqrt(disc)) / a and aquad_t_rt's (D - n.o) / (n.d). PRE_OTHER records take prim_exact
// on the RtPrim `p` (read only there).
template <class Real>
__device__ __forceinline__ bool prim_exact_rec(const RtExact& x, const RtPrim& p, const RayK<Real>& r, Real& t) {
    const Real inf = (Real)__builtin_inf();
    const int code = x.kind & 7;
    const bool sph = code == PRE_SPHERE;
    if (code == PRE_OTHER) return prim_exact<Real>(p, r, t);
    const Real s0 = (Real)x.s0;  // the JS double, or the fp32 mode's (float) s0 = RtPrim g0[3]
    Real num, den, halfB = (Real)0, sq = (Real)0;
    float o1 = 0.f, d1 = 0.f, o2 = 0.f, d2 = 0.f;
    if (sph) {
        const V3 c = V3{x.f[0], x.f[1], x.f[2]};
        const V3 oc = sub(r.o, c);
        halfB = dot<Real>(oc, r.d);
        const Real cc = len2<Real>(oc) - s0 * s0;
        const Real disc = halfB * halfB - r.a * cc;
        if (disc < (Real)0) return false;
        sq = m_sqrt(disc);
        num = -halfB - sq;
        den = r.a;
    } else {
        const int a = (int)((aquad_axes(0) >> (2 * code)) & 3u);
        const int ia = (int)((aquad_axes(1) >> (2 * code)) & 3u);
        const int ib = (int)((aquad_axes(2) >> (2 * code)) & 3u);
        const V3 o3 = r.o, d3 = r.d;
        const float oa = sel3(o3.x, o3.y, o3.z, a), da = sel3(d3.x, d3.y, d3.z, a);
        o1 = sel3(o3.x, o3.y, o3.z, ia);
        d1 = sel3(d3.x, d3.y, d3.z, ia);
        o2 = sel3(o3.x, o3.y, o3.z, ib);
        d2 = sel3(d3.x, d3.y, d3.z, ib);
        if (!(::isfinite(o1) && ::isfinite(d1) && ::isfinite(o2) && ::isfinite(d2))) return false;
        const Real na = (x.kind & kExactNegNa) ? (Real)-1 : (Real)1;  // n[a], exactly +-1
        den = na * (Real)da;
        if (m_abs(den) < (Real)1e-8) return false;
        num = s0 - na * (Real)oa;
    }
    Real q = num / den;
    if (sph) {
        if (!(K<Real>::TMIN < q && q < inf)) {
            q = (-halfB + sq) / r.a;
            if (!(K<Real>::TMIN < q && q < inf)) return false;
        }
    } else {
        if (!(K<Real>::TMIN < q && q < inf)) return false;
        const float ph1 = (o1 + (float)((Real)d1 * q)) - x.f[0];
        const float ph2 = (o2 + (float)((Real)d2 * q)) - x.f[1];
        const Real sw = (Real)x.f[2];
        const Real alpha = sw * (Real)(ph1 * x.f[3]);
        const Real beta = sw * (Real)(ph2 * x.f[4]);
        if (alpha < (Real)0 || alpha > (Real)1 || beta < (Real)0 || beta > (Real)1) return false;
    }
    t = q;
    return true;
}

// The brute-force pass's axis-quad pre-filter over an RtPre record {x_a, sv, su, -Q[ia] sv - 1/2,
// -Q[ib] su - 1/2, kRel qm} (qm = max(|Q[ia]|, |Q[ib]|)). The plane's t comes from the ray's slab
// constants, t = fma(x_a, inv[a], noi[a]), instead of a reciprocal of n.d per quad, and alpha - 1/2,
// beta - 1/2 are two FMAs each on host-folded products (round 4: 45 -> ~16 VALU per quad).
// Error of t, first order (u = 2^-24): inv = (1/d)(1 + e1), |e1| <= 2u (v_rcp_f32, 1 ulp);
// noi = -o inv (1 + e2) and x_a = x*(1 + e3), |e2|, |e3| <= u (x* = D / n_a, the exact test's
// plane); the fma rounds once more (e4). With t* = (x* - o) / d the exact test's t,
//   t - t* = t* e1 + inv (x* e3 - o e2) + t e4,  |t - t*| <= 2u |t*| + u (|x* inv| + |noi|) + u |t|
//                                                          <= 2u |noi| + 4u |t|   (|x* inv| <= |t| + |noi|)
// (the exact test's own double rounding is ~1e-16 relative). et = kEt (|t| + |noi|), kEt = 1e-6
// ~ 17u, covers each term 4x over. Round 2/3 used kRel = 1e-5 here: a ray leaving a wall at
// x_a = 555 has |noi| = 555 / |d_a|, so the wall it starts on stayed a candidate (lower bound
// < 0: tested FIRST) unless |d_a| > 5.5 - never - so it was tested first, and then the wall the
// ray does hit; at kEt the wall it leaves is rejected whenever |d_a| > ~0.56 (the exact test
// could only return a self-hit t = (x* - o) / d ~ 3e-5 / |d_a| > 0.001 below |d_a| ~ 0.03).
// The in-plane coordinate o + t d - Q is off by at most et |d| + a few u (|o| + |t d| + |Q|),
// which dp = (|t| + |noi|) c1 + c0 + kRel qm bounds (c1 = (kEt + kRel) dn, c0 = kRel on +
// 1e-30 dn: QuadPreRay; |o| <= on, |d| <= dn, |Q| <= qm), times |sv| (|su|) in alpha (beta).
// The window test alpha in [-ea, 1 + ea], ea = |sv| dp + 1e-4 (the absolute part covers alpha's
// own rounding near [0, 1], and the host's folding of the 1/2), is |alpha - 1/2| - |sv| dp <=
// 1/2 + 1e-4, one FMA with source modifiers, compared against kWin (1e-6 more for that FMA's own
// rounding); a NaN passes. Near-parallel rays (|d[a]| <= 1e-3 |d|, or a ray whose slab constants
// overflowed: pthr = inf) are decided by the exact test.
constexpr float kEt = 1e-6f;
constexpr float kWin = 0.5f + 1e-4f + 1e-6f;
struct QuadPreRay {
    float c1, c0;
};
__device__ __forceinline__ QuadPreRay quad_pre_ray(const FRay& f) {
    RT_FP32_FUSED
    return QuadPreRay{(kEt + kRel) * f.dn, kRel * f.on + 1e-30f * f.dn};
}
template <int CODE>
__device__ __forceinline__ bool aquad_maybe_pre(const float* v, const FRay& f, const QuadPreRay& qr, float& lo) {
    RT_FP32_FUSED
    constexpr int a = (CODE - 1) % 3, vflag = (CODE - 1) / 3;
    constexpr int ia = vflag ? (a + 1) % 3 : (a + 2) % 3, ib = vflag ? (a + 2) % 3 : (a + 1) % 3;
    const float xa = v[0], sv = v[1], su = v[2], nq1 = v[3], nq2 = v[4], qk = v[5];
    lo = kTminLo;
    if (!(::fabsf(f.d[a]) > f.pthr)) return true;
    const float t = __builtin_fmaf(xa, f.inv[a], f.noi[a]);
    const float tn = ::fabsf(t) + ::fabsf(f.noi[a]);
    const float et = __builtin_fmaf(kEt, tn, 1e-30f);
    if (t + et < kTminLo) return false;
    lo = t - et;
    const float alpha = __builtin_fmaf(__builtin_fmaf(t, f.d[ia], f.o[ia]), sv, nq1);  // alpha - 1/2
    const float beta = __builtin_fmaf(__builtin_fmaf(t, f.d[ib], f.o[ib]), su, nq2);   // beta - 1/2
    const float dp = __builtin_fmaf(tn, qr.c1, qr.c0 + qk);
    const float wa = __builtin_fmaf(-::fabsf(sv), dp, ::fabsf(alpha));
    const float wb = __builtin_fmaf(-::fabsf(su), dp, ::fabsf(beta));
    return !(wa > kWin) && !(wb > kWin);
}

// Pre-filters of a PAIR of primitives in packed fp32 (RtPre PRE_SPHERE2 / PRE_QUAD2): the same
// operations as sphere_maybe / aquad_maybe_pre, element by element, on two-float vectors that
// the compiler issues as v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32 (one instruction for both
// primitives; the record's element pairs sit in aligned SGPR pairs, the ray's operands are
// broadcast with op_sel). Branch-free: both results are computed and masked. The margins are
// the single tests' (a filter may round differently as long as it stays conservative; the
// pair's window margin uses the larger qk of the two).

__device__ __forceinline__ void sphere_maybe2(const float* v, const FRay& f, bool& m0, bool& m1, float& lo0,
                                              float& lo1) {
    RT_FP32_FUSED
    const pf2 cx = {v[0], v[1]}, cy = {v[2], v[3]}, cz = {v[4], v[5]}, r = {v[6], v[7]}, rr = {v[8], v[9]};
    const pf2 ox = pf2_of(f.o[0]) - cx, oy = pf2_of(f.o[1]) - cy, oz = pf2_of(f.o[2]) - cz;
    const pf2 b = pf2_fma(oz, pf2_of(f.d[2]), pf2_fma(oy, pf2_of(f.d[1]), ox * pf2_of(f.d[0])));
    const pf2 oo = pf2_fma(oz, oz, pf2_fma(oy, oy, ox * ox));
    const pf2 disc = pf2_fma(b, b, -(pf2_of(f.a) * (oo - rr)));
    const pf2 tol = pf2_fma(pf2_of(4.0f * kRel * f.a), oo + rr, pf2_of(1e-30f));
    const pf2 dt = __builtin_elementwise_max(disc, pf2_of(0.0f)) + tol;
    const pf2 sq = pf2{__builtin_amdgcn_sqrtf(dt.x), __builtin_amdgcn_sqrtf(dt.y)} * pf2_of(1.0f + kRel);
    // sphere_et: kRel (2 |b| + dn r + 3 sq) ia + 1e-30
    const pf2 e0 = pf2_fma(pf2_of(3.0f), sq, pf2_fma(pf2_of(f.dn), r, pf2_of(2.0f) * pf2_abs(b)));
    const pf2 et = pf2_fma(e0, pf2_of(kRel * f.ia), pf2_of(1e-30f));
    const pf2 far = pf2_fma((sq - b) * pf2_of(f.ia), pf2_of(1.0f + kRel), et);
    const pf2 r1 = (-b - sq) * pf2_of(f.ia);
    const pf2 lo = pf2_fma(-pf2_abs(r1), pf2_of(kRel), r1) - et;
    m0 = !(disc.x < -tol.x) && !(far.x < kTminLo);
    m1 = !(disc.y < -tol.y) && !(far.y < kTminLo);
    lo0 = lo.x;
    lo1 = lo.y;
}

template <int CODE>
__device__ __forceinline__ void aquad_maybe_pre2(const float* v, const FRay& f, const QuadPreRay& qr, bool& m0,
                                                 bool& m1, float& lo0, float& lo1) {
    RT_FP32_FUSED
    constexpr int a = (CODE - 1) % 3, vflag = (CODE - 1) / 3;
    constexpr int ia = vflag ? (a + 1) % 3 : (a + 2) % 3, ib = vflag ? (a + 2) % 3 : (a + 1) % 3;
    const pf2 xa = {v[0], v[1]}, sv = {v[2], v[3]}, su = {v[4], v[5]}, nq1 = {v[6], v[7]}, nq2 = {v[8], v[9]};
    const pf2 nsv = {v[10], v[11]}, nsu = {v[12], v[13]};
    const float qk = v[14];
    const pf2 t = pf2_fma(xa, pf2_of(f.inv[a]), pf2_of(f.noi[a]));
    const float an = ::fabsf(f.noi[a]);
    const pf2 tn = {::fabsf(t.x) + an, ::fabsf(t.y) + an};  // source modifiers, no masks
    const pf2 et = pf2_fma(pf2_of(kEt), tn, pf2_of(1e-30f));
    const pf2 te = t + et;
    const pf2 lo = t - et;
    const pf2 alpha = pf2_fma(pf2_fma(t, pf2_of(f.d[ia]), pf2_of(f.o[ia])), sv, nq1);  // alpha - 1/2
    const pf2 beta = pf2_fma(pf2_fma(t, pf2_of(f.d[ib]), pf2_of(f.o[ib])), su, nq2);   // beta - 1/2
    const pf2 dp = pf2_fma(tn, pf2_of(qr.c1), pf2_of(qr.c0 + qk));
    const pf2 wa = pf2_fma(nsv, dp, pf2_abs(alpha));
    const pf2 wb = pf2_fma(nsu, dp, pf2_abs(beta));
    const bool par = !(::fabsf(f.d[a]) > f.pthr);  // near-parallel: the exact test decides
    m0 = par || (!(te.x < kTminLo) && !(wa.x > kWin) && !(wb.x > kWin));
    m1 = par || (!(te.y < kTminLo) && !(wa.y > kWin) && !(wb.y > kWin));
    lo0 = par ? kTminLo : lo.x;
    lo1 = par ? kTminLo : lo.y;
}

// The brute-force pass's per-lane candidate bounds live in fp16 LDS columns (half the
// LDS of fp32: room for more pool slots). A stored bound must stay a lower bound: clamped
// at 0 (every hit has t > 0.001) and converted toward zero (v_cvt_pkrtz: round down for
// non-negative values; above 65504 it saturates to 65504, still below). A NaN bound stores
// 0, the smallest bound: such a candidate is tested before any other and never ends the
// nearest-first loop (0 <= every best t), so it is always tested.
__device__ __forceinline__ float lot_clamp(float lo) { return lo > 0.0f ? lo : 0.0f; }
__device__ __forceinline__ uint16_t lot_store(float lo) {
    const auto h = __builtin_amdgcn_cvt_pkrtz(lot_clamp(lo), 0.0f);
    return __builtin_bit_cast(uint16_t, h[0]);
}
__device__ __forceinline__ float lot_load(uint16_t b) { return (float)__builtin_bit_cast(_Float16, b); }
// This lane's fp16 column base (stk = the block's LDS base + threadIdx.x, as int*).
template <class SK>
__device__ __forceinline__ uint16_t* lot_column(SK* stk) {
    return reinterpret_cast<uint16_t*>(stk - threadIdx.x) + threadIdx.x;
}

struct NoHook {
    __device__ void operator()() const {}
};
// The brute-force pass's second half: exact tests of the candidates in `mask`, nearest lower
// bound first, until the next bound exceeds the best hit. `next(mask, kb, lb)` picks the
// remaining candidate with the smallest bound (never NaN). The result is the lexicographic
// minimum of (t, slot) over the candidates' exact hits, whatever the order of the tests: any
// superset of the true candidates with valid lower bounds returns the same hit.
template <class Real, bool COUNT, class Next>
__device__ __forceinline__ int brute_nearest_first(const DevScene& S, const RayK<Real>& r, uint32_t mask, Real& t_hit,
                                                   uint32_t* cnt, Next next) {
    Real best_t = (Real)__builtin_inf();
    int best = -1;
    float thi = __builtin_inff();
    int n_exact = 0;
    if (COUNT) {
        cnt[CT_CAND0] += mask == 0u ? 1u : 0u;
        cnt[CT_CAND2] += __popc(mask) >= 2 ? 1u : 0u;
    }
    while (mask != 0u) {
        int kb;
        float lb;
        next(mask, kb, lb);
        if (lb > thi) break;  // every remaining candidate's t exceeds the best hit
        mask &= ~(1u << kb);
        if (COUNT) {
            count_exact(cnt);
            if (++n_exact == 2) cnt[CT_EXACT2]++;
        }
        Real t;
        // ref precision: the ray as is, not ray_at_use - its fp64 conversions may then be
        // scheduled while the record loads are in flight (13.14 -> 13.11 ms,
        // profiles/r06/pairs/r06_rayhoist/). The fp32 build keeps ray_at_use: there |d|^2 may be
        // contracted (fma) differently where make_ray is inlined, and the pool and chunked kernels
        // must return the same hits (test_pool_kernel_equals_chunked_kernel caught 613 pixels).
        const bool hit = sizeof(Real) == 8
                             ? prim_exact_rec<Real>(xrec_load(S.xrec + kb), S.prims[kb], r, t)
                             : prim_exact_rec<Real>(xrec_load(S.xrec + kb), S.prims[kb], ray_at_use<Real>(r), t);
        if (hit && (t < best_t || (t == best_t && kb < best))) {
            best_t = t;
            best = kb;
            thi = upper_f<Real>(t);
        }
    }
    t_hit = best_t;
    return best;
}

// The closest hit of a primary ray of a pinhole camera from its pixel's record of the
// primary-ray candidate table (primary.hpp): the candidate mask, the nearest candidate's slot
// and fp16 bound, and one fp16 bound shared by the others. No fp32 pre-filter pass.
template <class Real, bool COUNT>
__device__ __forceinline__ int closest_hit_primary(const DevScene& S, const RayK<Real>& r, Real& t_hit, uint2 rec,
                                                   uint32_t* cnt) {
    const int near = (int)((rec.x >> 16) & 15u);
    const float bn = lot_load((uint16_t)rec.y), bo = lot_load((uint16_t)(rec.y >> 16));
    return brute_nearest_first<Real, COUNT>(S, r, rec.x & 0xffffu, t_hit, cnt, [&](uint32_t m, int& kb, float& lb) {
        const bool n = ((m >> near) & 1u) != 0u;  // bn <= bo: the nearest candidate first
        kb = n ? near : __builtin_ctz(m);
        lb = n ? bn : bo;
    });
}

// `after_prefilter`: called once the pre-filter pass is done (diagnostic section timer).
template <class Real, bool COUNT, class Hook = NoHook>
__device__ __forceinline__ int closest_hit_brute_nf(const DevScene& S, int n_prims, const RayK<Real>& r, Real& t_hit,
                                                    uint16_t* lot, uint32_t* cnt, Hook after_prefilter = Hook()) {
    (void)n_prims;  // the records (S.n_pre) cover the primitives; the mask holds their slots
    const FRay f = make_fray(r.o, r.d);
    const QuadPreRay qr = quad_pre_ray(f);
    uint32_t mask = 0u;
    for (int g = 0; g < S.n_pre; ++g) {
        // one scalar load (wave-uniform). (Round 4 tried issuing the next record's load an
        // iteration ahead: the two records' SGPRs pushed the pool kernel into SGPR spills,
        // Cornell path kernel 13.93 -> 14.65 ms; profiles/r04/ahead/.)
        const RtPre q = ld_uniform(S.gpre, g);
        const int kind = q.head & 0xff, k0 = (q.head >> 8) & 0xff, k1 = q.head >> 16;
        const float* v = q.f;
        if (kind >= PRE_SPHERE2) {  // a pair
            bool m0, m1;
            float lo0, lo1;
            if (kind == PRE_SPHERE2) {
                if (COUNT) cnt[CT_SPHERE] += 2;
                sphere_maybe2(v, f, m0, m1, lo0, lo1);
            } else {
                if (COUNT) cnt[CT_QUAD] += 2;
                switch (kind - PRE_QUAD2) {
                    case 1: aquad_maybe_pre2<1>(v, f, qr, m0, m1, lo0, lo1); break;
                    case 2: aquad_maybe_pre2<2>(v, f, qr, m0, m1, lo0, lo1); break;
                    case 3: aquad_maybe_pre2<3>(v, f, qr, m0, m1, lo0, lo1); break;
                    case 4: aquad_maybe_pre2<4>(v, f, qr, m0, m1, lo0, lo1); break;
                    case 5: aquad_maybe_pre2<5>(v, f, qr, m0, m1, lo0, lo1); break;
                    default: aquad_maybe_pre2<6>(v, f, qr, m0, m1, lo0, lo1); break;
                }
            }
            // both bounds in one conversion. (The halves are taken as integer bits: with h[1]
            // stored directly this compiler stored the LOW half for both.)
            const uint32_t hw = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(lot_clamp(lo0), lot_clamp(lo1)));
            if (m0) {
                lot[k0 * kStackStride] = (uint16_t)hw;
                mask |= 1u << k0;
            }
            if (m1) {
                lot[k1 * kStackStride] = (uint16_t)(hw >> 16);
                mask |= 1u << k1;
            }
            continue;
        }
        float lo;
        bool maybe;
        if (kind == PRE_SPHERE) {
            if (COUNT) cnt[CT_SPHERE]++;
            maybe = sphere_maybe(make_float4(v[0], v[1], v[2], v[3]), f, __builtin_inff(), lo);
        } else if (kind != PRE_OTHER) {
            if (COUNT) cnt[CT_QUAD]++;
            switch (kind) {
                case 1: maybe = aquad_maybe_pre<1>(v, f, qr, lo); break;
                case 2: maybe = aquad_maybe_pre<2>(v, f, qr, lo); break;
                case 3: maybe = aquad_maybe_pre<3>(v, f, qr, lo); break;
                case 4: maybe = aquad_maybe_pre<4>(v, f, qr, lo); break;
                case 5: maybe = aquad_maybe_pre<5>(v, f, qr, lo); break;
                default: maybe = aquad_maybe_pre<6>(v, f, qr, lo); break;
            }
        } else {
            maybe = prim_maybe<COUNT>(ld_uniform(S.gprims, k0), f, lo, cnt);
        }
        if (maybe) {
            lot[k0 * kStackStride] = lot_store(lo);
            mask |= 1u << k0;
        }
    }
    after_prefilter();
    return brute_nearest_first<Real, COUNT>(S, r, mask, t_hit, cnt, [&](uint32_t rest, int& kb, float& lb) {
        // nearest remaining candidate (stored bounds are never NaN: lot_store)
        kb = __builtin_ctz(rest);
        lb = lot_load(lot[kb * kStackStride]);
        for (uint32_t m = rest & (rest - 1u); m != 0u; m &= m - 1u) {
            const int k = __builtin_ctz(m);
            const float l = lot_load(lot[k * kStackStride]);
            if (l < lb) {
                lb = l;
                kb = k;
            }
        }
    });
}

template <class Real, bool COUNT, int TRAV, class SK>
__device__ __forceinline__ int closest_hit_any(const DevScene& S, int n_prims, const RayK<Real>& r, Real& t, SK* stk,
                                               uint32_t* cnt) {
    if (TRAV == TRAV_BRUTE) {
        if (n_prims <= kBruteMaxPrims)
            return closest_hit_brute_nf<Real, COUNT>(S, n_prims, r, t, lot_column(stk), cnt);
        return closest_hit_brute<Real, COUNT>(S, n_prims, r, t, cnt);
    }
    if (trav_fast(TRAV)) return closest_hit_fast<Real, COUNT, TRAV == TRAV_FAST_DEFER>(S, r, t, stk, cnt);
    return closest_hit<Real, COUNT>(S, r, t, stk, cnt);
}

}  // namespace rt
