// Materials, light sampling and the path state machine (path_begin ... path_trip).
#pragma once

#include <hip/hip_runtime.h>

#include "pt_brute.hpp"

namespace rt {

// ONBasis (src/geometry/onbasis.ts:18-51)
struct Onb {
    V3 u, v, w;
};
template <class Real>
__device__ __forceinline__ Onb make_onb(V3 n) {
    Onb b;
    b.w = unit<Real>(n);
    const V3 a = m_abs((Real)b.w.x) > (Real)0.9 ? v3(0, 1, 0) : v3(1, 0, 0);
    b.v = unit<Real>(cross<Real>(b.w, a));
    b.u = cross<Real>(b.w, b.v);
    return b;
}
template <class Real>
__device__ __forceinline__ V3 onb_local(const Onb& b, V3 a) {
    return add(add(scale<Real>(b.u, (Real)a.x), scale<Real>(b.v, (Real)a.y)), scale<Real>(b.w, (Real)a.z));
}

// Vec3.randomInUnitSphere (src/geometry/vec3.ts:285-292): 3 draws per try.
template <class Real>
__device__ __forceinline__ V3 random_in_unit_sphere(uint64_t& rng) {
    while (true) {
        const Real x = (Real)-1 + (Real)2 * uniform<Real>(rng);
        const Real y = (Real)-1 + (Real)2 * uniform<Real>(rng);
        const Real z = (Real)-1 + (Real)2 * uniform<Real>(rng);
        const V3 p = mk<Real>(x, y, z);
        if (len2<Real>(p) < (Real)1) return p;
    }
}

// Dielectric.scatter direction (src/materials/dielectric.ts:44-98). Draws one
// random only when refraction is possible (short-circuit ||).
template <class Real>
__device__ __forceinline__ V3 dielectric_dir(Real ior, bool front, V3 din, V3 n, uint64_t& rng, bool& reflected) {
    const Real ratio = front ? ((Real)1 / ior) : ior;
    const V3 ud = unit<Real>(din);
    const Real cosT = js_min<Real>(dot<Real>(neg(ud), n), (Real)1);
    const Real sinT = m_sqrt((Real)1 - cosT * cosT);
    const bool cannot = ratio * sinT > (Real)1;
    bool refl = cannot;
    if (!refl) {
        Real r0 = ((Real)1 - ratio) / ((Real)1 + ratio);
        r0 = r0 * r0;
        const Real reflectance = r0 + ((Real)1 - r0) * pow5((Real)1 - cosT);
        refl = reflectance > uniform<Real>(rng);
    }
    reflected = refl;
    if (refl) return reflect<Real>(ud, n);
    // Vec3.refract (src/geometry/vec3.ts:193-209)
    const V3 perp = scale<Real>(add(ud, scale<Real>(n, cosT)), ratio);
    const V3 par = scale<Real>(n, -m_sqrt(m_abs((Real)1 - len2<Real>(perp))));
    return add(perp, par);
}

enum ScatterKind { SC_NONE = 0, SC_SPEC = 1, SC_PDF = 2 };

// Material.scatter over the flat material table; Mixed and Layered follow
// their children iteratively (mixedMaterial.ts:38-44, layeredMaterial.ts:36-53).
template <class Real>
__device__ __forceinline__ int scatter(const DevScene& S, int mi, V3 din, V3 n, bool front, uint64_t& rng, V3& att,
                                       V3& dir, int* pdf_mat = nullptr) {
    while (true) {
        const RtMat m = S.mats[mi];
        switch (m.type) {
            case MAT_LAMBERT:
                att = ld3(m.color);
                if (pdf_mat) *pdf_mat = mi;  // att is this material's albedo
                return SC_PDF;
            case MAT_METAL: {
                const V3 refl = reflect<Real>(unit<Real>(din), n);
                const Real fuzz = (Real)m.p0;
                V3 f = refl;
                if (fuzz > (Real)0) f = add(refl, scale<Real>(random_in_unit_sphere<Real>(rng), fuzz));
                if (dot<Real>(f, n) <= (Real)0) return SC_NONE;
                att = ld3(m.color);
                dir = f;
                return SC_SPEC;
            }
            case MAT_GLASS: {
                bool r;
                dir = dielectric_dir<Real>((Real)m.p0, front, din, n, rng, r);
                att = v3(1, 1, 1);
                return SC_SPEC;
            }
            case MAT_MIXED:
                mi = uniform<Real>(rng) < (Real)m.p0 ? m.c0 : m.c1;
                continue;
            case MAT_LAYERED: {
                bool r;
                const V3 d2 = dielectric_dir<Real>((Real)S.mats[m.c0].p0, front, din, n, rng, r);
                if (r) {
                    att = v3(1, 1, 1);
                    dir = d2;
                    return SC_SPEC;
                }
                din = d2;  // the refracted ray becomes rIn for the inner material
                mi = m.c1;
                continue;
            }
            default:  // MAT_LIGHT and DefaultMaterial: no scatter
                return SC_NONE;
        }
    }
}

// Quad.pdfValue / Sphere.pdfValue (quad.ts:123-140, sphere.ts:106-131):
// re-intersect the light on (0.001, inf), not occlusion-aware.
template <class Real, bool COUNT, bool UNIFORM = false>
__device__ __forceinline__ Real light_pdf_value(const DevScene& S, const RtLight& L, V3 origin, V3 dir,
                                                uint32_t* cnt) {
    const RtPrim p = UNIFORM ? ld_uniform(S.gprims, L.prim) : S.prims[L.prim];
    const RayK<Real> r = make_ray<Real>(origin, dir);
    Real t;
    if (L.type == PRIM_QUAD) {
        if (COUNT) cnt[CT_LIGHT_QUAD]++;
        const int code = aquad_code(p);
        const bool hit = code != 0 ? aquad_t<Real>(p, code, origin, dir, K<Real>::TMIN, (Real)__builtin_inf(), t)
                                   : planar_t<Real, true>(p, r, K<Real>::TMIN, (Real)__builtin_inf(), t);
        if (!hit) return (Real)0;
        const V3 hp = ray_at<Real>(origin, dir, t);
        const V3 n = ld3(p.g3);
        const bool front = dot<Real>(dir, n) <= (Real)0;
        const V3 hn = front ? n : neg(n);
        const Real d2 = len2<Real>(sub(hp, origin));
        const Real cosine = m_abs(dot<Real>(dir, hn));
        return d2 / ((Real)L.area * cosine);
    }
    if (COUNT) cnt[CT_LIGHT_SPHERE]++;
    if (!sphere_t<Real>(p, r, K<Real>::TMIN, (Real)__builtin_inf(), t)) return (Real)0;
    const Real rad = sphere_radius<Real>(p);
    const Real d2 = len2<Real>(sub(ld3(p.g0), origin));
    if (d2 <= rad * rad) return (Real)1 / ((Real)4 * K<Real>::PI);
    const Real cosT = m_sqrt((Real)1 - rad * rad / d2);
    const Real solid = (Real)2 * K<Real>::PI * ((Real)1 - cosT);
    return (Real)1 / solid;
}

// Quad.pdfRandomVec / Sphere.pdfRandomVec (quad.ts:148-158, sphere.ts:140-147)
template <class Real>
__device__ __forceinline__ V3 light_generate(const DevScene& S, const RtLight& L, V3 origin, uint64_t& rng) {
    const RtPrim p = S.prims[L.prim];
    if (L.type == PRIM_QUAD) {
        const Real alpha = uniform<Real>(rng);
        const Real beta = uniform<Real>(rng);
        const V3 rp = add(add(ld3(p.g0), scale<Real>(ld3(p.g1), alpha)), scale<Real>(ld3(p.g2), beta));
        return unit<Real>(sub(rp, origin));
    }
    const V3 oc = sub(ld3(p.g0), origin);
    const Real d2 = len2<Real>(oc);
    const Onb b = make_onb<Real>(oc);
    // Vec3.randomToSphere (src/geometry/vec3.ts:345-351)
    const Real rad = sphere_radius<Real>(p);
    const Real r1 = uniform<Real>(rng);
    const Real r2 = uniform<Real>(rng);
    const Real z = (Real)1 + r2 * (m_sqrt((Real)1 - rad * rad / d2) - (Real)1);
    const Real phi = (Real)2 * K<Real>::PI * r1;
    const Real s = m_sqrt((Real)1 - z * z);
    Real sn, cs;
    m_sincos(phi, sn, cs);
    return onb_local<Real>(b, mk<Real>(cs * s, sn * s, z));
}

// CosinePDF.value (src/geometry/pdf.ts:43-46)
// x / PI, correctly rounded: q = RN(x * RN(1/PI)) corrected once by the exact
// residual x - q*PI (fma) - Markstein's theorem for a correctly rounded reciprocal
// gives RN(x / PI) (also checked on 4e8 doubles in (0, 1], tools/probes/div_pi.c);
// 3 fp64 operations instead of the division sequence.
__device__ __forceinline__ double div_pi(double x) {
    constexpr double kPi = 3.141592653589793, kInvPi = 1.0 / 3.141592653589793;
    const double q = x * kInvPi;
    const double r = __builtin_fma(-q, kPi, x);
    return __builtin_fma(r, kInvPi, q);
}
__device__ __forceinline__ float div_pi(float x) { return x / K<float>::PI; }

template <class Real>
__device__ __forceinline__ Real cosine_value(const Onb& b, V3 dir) {
    const Real c = dot<Real>(unit<Real>(dir), b.w);
    return c <= (Real)0 ? (Real)0 : div_pi(c);
}

// One path (one rayColor recursion) in flight on a lane.
template <bool EMIT>
struct Path {
    uint64_t rng;
    V3 o, d, T;
    int bounces;
    int em_n;
    V3 em[EMIT ? kEmitStack : 1];
};

// Camera.getRay (src/camera.ts:176-210) for sample `sample` of pixel (i, j).
// pixel00Loc + i*pixelDeltaU + j*pixelDeltaV (src/camera.ts:181), fixed per pixel.
// The scalings by the integers i, j (< 2^16) are fp32 multiplies: an fp32 times an
// integer below 2^24 is exact in double, so the double product rounded to fp32 is
// the fp32 product (rt_math.hpp identities) - the ref build's result, bit for bit.
template <class Real>
__device__ __forceinline__ V3 pixel_center(const RtCamera& C, int i, int j) {
    return add(add(ld3(C.pixel00), scale<float>(ld3(C.du), (float)i)), scale<float>(ld3(C.dv), (float)j));
}

template <class Real, bool EMIT>
__device__ __forceinline__ void path_begin(const RtCamera& C, Path<EMIT>& P, V3 pc, uint32_t pix, uint32_t sample) {
    P.rng = rng_init(C.seed_mix, pix, sample);
    const V3 du = ld3(C.du), dv = ld3(C.dv), cen = ld3(C.center);
    V3 ps = pc;
    if (C.samples > 1.0) {
        const Real px = (Real)-0.5 + uniform<Real>(P.rng);
        const Real py = (Real)-0.5 + uniform<Real>(P.rng);
        ps = add(add(pc, scale<Real>(du, px)), scale<Real>(dv, py));
    }
    P.o = cen;
    P.d = sub(ps, cen);
    if (C.aperture > 0.0) {
        V3 rd;
        while (true) {  // Vec3.randomInUnitDisk (vec3.ts:357-364)
            const Real a = (Real)2 * uniform<Real>(P.rng) - (Real)1;
            const Real b = (Real)2 * uniform<Real>(P.rng) - (Real)1;
            rd = mk<Real>(a, b, (Real)0);
            if (len2<Real>(rd) < (Real)1) break;
        }
        const V3 off = add(scale<Real>(ld3(C.ddu), (Real)rd.x), scale<Real>(ld3(C.ddv), (Real)rd.y));
        P.o = add(cen, off);
        P.d = sub(ps, P.o);
    }
    P.T = v3(1, 1, 1);
    P.bounces = 0;
    P.em_n = 0;
}

// One level of rayColor (src/camera.ts:221-319). Returns true when the path
// ends; `c` is then the sample's radiance (the recursion's emitted + ... right
// fold included).
// The emission right fold of a terminated path (EMIT builds).
template <bool EMIT>
__device__ __forceinline__ void fold_emission(const Path<EMIT>& P, V3& c) {
    if (EMIT) {
        for (int k = min(P.em_n, kEmitStack) - 1; k >= 0; --k) c = add(P.em[k], c);
    }
}

// First half of a rayColor level: the depth cut-off and Russian roulette
// (src/camera.ts:221-235). Returns true when the path ends here (`c` is then
// the sample's radiance), false when its ray must be traced next.
template <class Real, bool EMIT, bool PROF>
__device__ __forceinline__ bool path_pre(const RtCamera& C, Path<EMIT>& P, Prof& pf, V3& c) {
    bool term = false;
    c = v3(0, 0, 0);
    if (P.bounces >= C.depth) {
        term = true;
    } else if (C.roulette && P.bounces >= C.roulette_depth) {
        const Real mc = js_max<Real>(js_max<Real>((Real)P.T.x, (Real)P.T.y), (Real)P.T.z);
        const Real p = js_min<Real>(mc, (Real)0.95);
        if (uniform<Real>(P.rng) > p) term = true;
        else P.T = divs<Real>(P.T, p);
    }
    if (term) fold_emission<EMIT>(P, c);
    psec<PROF>(pf, PR_RR);
    return term;
}

// The stages of the second half of a rayColor level (src/camera.ts:236-319),
// shared by path_post and the stage-compacted pool kernel.

// Miss: the background gradient times the throughput (camera.ts:236-244).
template <class Real, bool EMIT, bool PROF>
__device__ __forceinline__ V3 miss_color(const RtCamera& C, const Path<EMIT>& P, unsigned long long& st_err,
                                         Prof& pf) {
    if (!C.has_background) st_err |= ERR_NO_BACKGROUND;
    V3 ud;
    if constexpr (sizeof(Real) == 4) {
        // The fp32 build contracts |d|^2 = x x + y y + z z, and which product it left unfused
        // depended on the kernel: the sequential kernel rounded x x first, the chunked and pool
        // kernels y y, and their sky pixels differed in the last bit (about 1 % of them). One
        // order, spelled out - the chunked and pool kernels' - so all three write the same bits.
        float l = __builtin_fmaf(P.d.z, P.d.z, __builtin_fmaf(P.d.x, P.d.x, P.d.y * P.d.y));
        if (l > 0.0f) l = rsqrt_rn<float>(l);
        ud = V3{P.d.x * l, P.d.y * l, P.d.z * l};
    } else {
        ud = unit<Real>(P.d);
    }
    const Real a = (Real)0.5 * ((Real)ud.y + (Real)1);
    const V3 c = mulv(add(scale<Real>(ld3(C.bg_top), (Real)1 - a), scale<Real>(ld3(C.bg_bottom), a)), P.T);
    psec<PROF>(pf, PR_MISS);
    return c;
}

// A sphere's hit normal: Vec3.divide(radius) of p - center (sphere.ts:72). The fp32 build then
// normalises the quotient: with p = o + t d and t rounded to fp32 it is off unit length by up
// to 5e-4 on a small sphere a few units away, and reflect, refract and the
// cosine PDF take a unit normal. The ref build keeps the reference's quotient bit for bit.
// v_rsq_f32 (<= 1 ulp; |n|^2 is within 1e-3 of 1, far from its denormal range) leaves |n|^2
// within 4e-7 of 1; the IEEE 1 / sqrt cost fp32 Cornell 1.0 % and spheres-500 0.6 %.
template <class Real>
__device__ __forceinline__ V3 sphere_normal(const RtPrim& pr, V3 p) {
    const V3 n = scale<Real>(sub(p, ld3(pr.g0)), sphere_inv_radius<Real>(pr));
    if constexpr (sizeof(Real) == 4) return scale<Real>(n, __builtin_amdgcn_rsqf(len2<Real>(n)));
    else return n;
}

// Hit record (sphere.ts:67-84, quad.ts:72-83, plane.ts:246-259) and the
// material's emission and scatter (camera.ts:246-262). Returns the scatter kind;
// `planar` = the primitive has a fixed normal (quad / plane: ONB table lookup).
template <class Real, bool EMIT, bool COUNT, bool PROF>
__device__ __forceinline__ int shade_hit(const DevScene& S, Path<EMIT>& P, int h, Real t, uint32_t* cnt, Prof& pf,
                                         V3& p, V3& nrm, bool& front, bool& planar, V3& emitted, V3& att, V3& sdir,
                                         int* pdf_mat = nullptr) {
    if (COUNT) cnt[CT_MATERIAL]++;
    const RtPrim pr = S.prims[h];
    p = ray_at<Real>(P.o, P.d, t);
    planar = pr.type != PRIM_SPHERE;
    if (!planar) {
        nrm = sphere_normal<Real>(pr, p);
        front = dot<Real>(P.d, nrm) <= (Real)0;
        if (!front) nrm = neg(nrm);
    } else {
        const V3 pn = ld3(pr.g3);
        front = dot<Real>(P.d, pn) <= (Real)0;
        nrm = front ? pn : neg(pn);
    }
    const RtMat hm = S.mats[pr.mat];
    emitted = mulv(ld3(hm.emitted), P.T);
    psec<PROF>(pf, PR_HITREC);
    const int kind = scatter<Real>(S, pr.mat, P.d, nrm, front, P.rng, att, sdir, pdf_mat);
    psec<PROF>(pf, PR_SCATTER);
    return kind;
}

// A diffuse (PDF) scatter: MixturePDF([CosinePDF(n), light PDFs...], [0.5,
// 0.5/nL...]) generate + value and the throughput update (camera.ts:263-315).
// Returns true when the path ends here (mixture value <= 0.0001: the caller's
// sample radiance is the level's emission); else P continues from p.
// BR: 0 = the mixture's branch decided here; 1 / 2 = the caller knows it is the
// cosine / light branch (pool kernel: the draw was classified ahead) - the light
// branch then needs only the ONB's w (CosinePDF.value), not u and v.
template <class Real, bool EMIT, bool COUNT, bool PROF, int BR = 0>
__device__ __forceinline__ bool shade_diffuse(const DevScene& S, const RtCamera& C, Path<EMIT>& P, int h, bool planar,
                                              bool front, V3 p, V3 nrm, V3 att, uint32_t* cnt, Prof& pf) {
    if (COUNT) cnt[CT_DIFFUSE]++;
    Onb b;
    if (planar && h < S.n_onb) {
        const RtOnb& ob = S.onbs[(h * 2 + (sizeof(Real) == 4 ? 1 : 0)) * 2 + (front ? 0 : 1)];
        if (BR != 2) {
            b.u = ld3(ob.u);
            b.v = ld3(ob.v);
        }
        b.w = ld3(ob.w);
    } else if (BR == 2) {
        b.w = unit<Real>(nrm);  // make_onb's w
    } else {
        b = make_onb<Real>(nrm);
    }
    const Real total = (Real)S.mix_total;
    const bool total1 = S.mix_total == 1.0;  // x * 1 and x / 1 are exact: skip them (uniform branch)
    const Real lw = (Real)S.light_w;
    const Real u0 = uniform<Real>(P.rng);
    const Real rnd = total1 ? u0 : u0 * total;
    Real partial = (Real)0.5;
    V3 gdir;
    if (BR == 1 || (BR == 0 && (rnd < partial || C.n_lights == 0))) {
        const Real r1 = uniform<Real>(P.rng);
        const Real r2 = uniform<Real>(P.rng);
        const Real phi = (Real)2 * K<Real>::PI * r1;
        const Real sr2 = m_sqrt(r2);
        Real sn, cs;
        m_sincos(phi, sn, cs);
        gdir = onb_local<Real>(b, mk<Real>(cs * sr2, sn * sr2, m_sqrt((Real)1 - r2)));
    } else {
        int pick = C.n_lights - 1;
        for (int l = 0; l < C.n_lights; ++l) {
            partial += lw;
            if (rnd < partial) { pick = l; break; }
        }
        gdir = light_generate<Real>(S, S.lights[pick], p, P.rng);  // pick: per lane
    }
    psec<PROF>(pf, PR_SAMPLE);
    const Real cv = cosine_value<Real>(b, gdir);
    Real sum = (Real)0.5 * cv;
    for (int l = 0; l < C.n_lights; ++l)
        sum += lw * light_pdf_value<Real, COUNT, true>(S, ld_uniform(S.glights, l), p, gdir, cnt);
    const Real pv = total1 ? sum : sum / total;
    bool term = false;
    if (pv <= (Real)0.0001) {
        term = true;
    } else {
        const V3 brdf = scale<Real>(att, cv);
        P.T = divs<Real>(mulv(P.T, brdf), pv);
        P.o = p;
        P.d = gdir;
    }
    psec<PROF>(pf, PR_PDF);
    return term;
}

// Second half: given the closest hit (h, t) of the path's ray, the miss /
// emission / scatter / light sampling of the same level (src/camera.ts:236-319).
// Returns true when the path ends (`c` = the sample's radiance).
template <class Real, bool EMIT, bool COUNT, bool PROF>
__device__ __forceinline__ bool path_post(const DevScene& S, const RtCamera& C, Path<EMIT>& P, int h, Real t,
                                          uint32_t* cnt, unsigned long long& st_err, Prof& pf, V3& c) {
    bool term = false;
    c = v3(0, 0, 0);
    if (h < 0) {
        term = true;
        c = miss_color<Real, EMIT, PROF>(C, P, st_err, pf);
    } else {
        V3 p, nrm, emitted, att, sdir;
        bool front, planar;
        const int kind = shade_hit<Real, EMIT, COUNT, PROF>(S, P, h, t, cnt, pf, p, nrm, front, planar, emitted, att,
                                                            sdir);
        if (kind == SC_NONE) {
            term = true;
            c = emitted;
        } else {
            ++P.bounces;
            if (kind == SC_SPEC) {
                P.T = mulv(P.T, att);
                P.o = p;
                P.d = sdir;
            } else if (shade_diffuse<Real, EMIT, COUNT, PROF>(S, C, P, h, planar, front, p, nrm, att, cnt, pf)) {
                term = true;
                c = emitted;
            }
            if (EMIT && !term) {
                if (P.em_n < kEmitStack) P.em[P.em_n] = emitted;
                else st_err |= ERR_EMIT_STACK;
                ++P.em_n;
            }
        }
    }
    // emitted.add(rayColor(...)) at every level: a right fold.
    if (term) fold_emission<EMIT>(P, c);
    return term;
}

// One level of rayColor (src/camera.ts:221-319): path_pre, the closest hit,
// path_post. Returns true when the path ends; `c` is then the sample's radiance
// (the recursion's emitted + ... right fold included).
template <class Real, bool EMIT, bool COUNT, bool PROF, int TRAV, class SK>
__device__ __forceinline__ bool path_trip(const DevScene& S, const RtCamera& C, Path<EMIT>& P, SK* stk, uint32_t* cnt,
                                          unsigned long long& st_err, Prof& pf, V3& c) {
    if (path_pre<Real, EMIT, PROF>(C, P, pf, c)) return true;
    const RayK<Real> ray = make_ray<Real>(P.o, P.d);
    Real t;
    if (COUNT) cnt[CT_RAYS]++;
    const int h = closest_hit_any<Real, COUNT, TRAV>(S, C.n_prims, ray, t, stk, cnt);
    psec<PROF>(pf, PR_HIT);
    return path_post<Real, EMIT, COUNT, PROF>(S, C, P, h, t, cnt, st_err, pf, c);
}

}  // namespace rt
