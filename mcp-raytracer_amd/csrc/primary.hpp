// Per-pixel primary-ray candidate table of the brute-force pool kernel.
//
// With a pinhole camera (aperture == 0) every primary ray of pixel (i, j) starts at
// C.center, and its direction is pc + px du + py dv - center with px, py in [-0.5, 0.5]
// (path_begin). The nearest-first brute-force pass (closest_hit_brute_nf) first runs an fp32
// pre-filter over all <= 16 primitives to find, per ray, the candidates and a lower bound of
// each one's t; for the primary rays of one pixel that answer is nearly the same for every
// sample. primary_record() computes it ONCE per pixel, conservatively for the pixel's whole
// footprint, in double interval arithmetic; the pool kernel's primary-ray trips read the
// record and go straight to the exact tests (pt_brute.hpp closest_hit_primary). The exact
// pass takes the lexicographic minimum of (t, slot) over the candidates it tests, so any
// superset of the true candidates with valid lower bounds returns the same hit.
//
// Record (8 bytes, one load, always valid):
//   bits  0-15  candidate mask by primitive slot
//   bits 16-19  slot of the candidate with the smallest bound ("nearest")
//   bits 32-47  fp16 bound of the nearest candidate
//   bits 48-63  fp16 bound shared by every other candidate: the minimum of theirs (a lowered
//               bound is still a bound)
// fp16 bounds are clamped at 0 and converted toward zero, as lot_store does. Bound 0 means
// "always exact-tested". The table is indexed by the row-major pixel j * width + i, the index
// the path start already forms for its RNG key.
//
// One table serves both precisions: every margin below is a kRel-sized (1e-5, ~170 fp32 ulps)
// multiple of the operand magnitudes, like the pre-filters', so it also covers the fp32
// build's exact tests, whose t carries a few fp32 roundings.
#pragma once

#include <cstdint>

#include "rt_math.hpp"
#include "scene_types.hpp"

namespace rt {

constexpr int kPrimaryMaxPrims = 16;          // = kBruteMaxPrims: one mask bit per primitive
constexpr double kPrimRel = 1e-5;             // pt_isect.hpp kRel
constexpr double kPrimTmin = 0.001 * (1.0 - 1e-5);  // pt_isect.hpp kTminLo

// Closed interval [lo, hi] of doubles. Outward rounding is not applied per operation: the
// double roundings (2^-53 relative) are ~2^-29 of the kRel margins every decision carries.
struct PIv {
    double lo, hi;
};
RT_HD double pmin(double a, double b) { return a < b ? a : b; }
RT_HD double pmax(double a, double b) { return a > b ? a : b; }
RT_HD double pabs(double a) { return a < 0.0 ? -a : a; }
RT_HD double piv_mag(PIv a) { return pmax(pabs(a.lo), pabs(a.hi)); }
RT_HD PIv piv_scale(PIv a, double s) { return s >= 0.0 ? PIv{a.lo * s, a.hi * s} : PIv{a.hi * s, a.lo * s}; }
RT_HD PIv piv_add(PIv a, PIv b) { return PIv{a.lo + b.lo, a.hi + b.hi}; }
RT_HD PIv piv_mul(PIv a, PIv b) {
    const double p0 = a.lo * b.lo, p1 = a.lo * b.hi, p2 = a.hi * b.lo, p3 = a.hi * b.hi;
    return PIv{pmin(pmin(p0, p1), pmin(p2, p3)), pmax(pmax(p0, p1), pmax(p2, p3))};
}
RT_HD PIv piv_sq(PIv a) {
    const double l = a.lo * a.lo, h = a.hi * a.hi;
    return PIv{(a.lo <= 0.0 && a.hi >= 0.0) ? 0.0 : pmin(l, h), pmax(l, h)};
}

// A non-negative bound as fp16 bits, rounded toward zero (integer arithmetic: the same bits
// on the host and on the device). NaN and negative values give 0, values from 65504 saturate.
RT_HD uint32_t primary_half(double lo) {
    if (!(lo > 0.0)) return 0u;
    float f = lo >= 65504.0 ? 65504.0f : (float)lo;
    uint32_t b = __builtin_bit_cast(uint32_t, f);
    if ((double)f > lo) --b;  // the conversion rounded up: one fp32 step down
    const int e = (int)(b >> 23);
    const uint32_t m = b & 0x7fffffu;
    if (e >= 113) return (uint32_t)(e - 112) << 10 | m >> 13;  // normal half (f < 65536)
    if (e < 103) return 0u;                                    // below the smallest subnormal
    return (m | 0x800000u) >> (126 - e);                       // subnormal half
}

// The candidate test of one primitive over the footprint: false when no ray of the footprint
// can be exact-tested to a hit with t > 0.001; else `lo` is a lower bound of any such t.
// o: the origin; d[a]: the direction box. Every rejection is a `<` comparison that a NaN
// fails, so a non-finite input leaves the primitive a candidate (with bound 0: primary_half).
RT_HD bool primary_candidate(const RtPrim& p, const double* o, const PIv* d, double dn, double& lo) {
    lo = 0.0;
    if (p.type == PRIM_SPHERE) {
        const double r = p.s0;
        if (!((float)r == p.g0[3])) return true;  // the fp32 mode's radius is another number: bound 0
        const double oc[3] = {o[0] - (double)p.g0[0], o[1] - (double)p.g0[1], o[2] - (double)p.g0[2]};
        // Sphere.hit: halfB = oc.d, cc = |oc|^2 - r^2, disc = halfB^2 - a cc, roots (-halfB -+ sqrt(disc)) / a
        const PIv b = piv_add(piv_add(piv_scale(d[0], oc[0]), piv_scale(d[1], oc[1])), piv_scale(d[2], oc[2]));
        const PIv a = piv_add(piv_add(piv_sq(d[0]), piv_sq(d[1])), piv_sq(d[2]));
        const double oo = oc[0] * oc[0] + oc[1] * oc[1] + oc[2] * oc[2], rr = r * r;
        const double cc = oo - rr;
        const double b2 = piv_sq(b).hi;
        // the exact tests' rounding of disc: a few ulps of halfB^2 + a (|oc|^2 + r^2) (sphere_maybe's tol)
        const double tol = 4.0 * kPrimRel * (b2 + a.hi * (oo + rr)) + 1e-300;
        // disc = halfB^2 - a (|oc|^2 - r^2) = a r^2 - |oc x d|^2 (Lagrange). Bounded in the second
        // form: the cross product's components are linear in d, so their intervals are exact,
        // whereas halfB^2 and a |oc|^2 nearly cancel and their separate bounds over the box would
        // widen a sphere's silhouette by several pixels.
        const PIv cx = piv_add(piv_scale(d[2], oc[1]), piv_scale(d[1], -oc[2]));
        const PIv cy = piv_add(piv_scale(d[0], oc[2]), piv_scale(d[2], -oc[0]));
        const PIv cz = piv_add(piv_scale(d[1], oc[0]), piv_scale(d[0], -oc[1]));
        const double disc_hi = a.hi * rr - (piv_sq(cx).lo + piv_sq(cy).lo + piv_sq(cz).lo);
        if (disc_hi < -tol) return false;
        const double sq = sqrt(pmax(disc_hi, 0.0) + tol) * (1.0 + kPrimRel);  // >= any sqrt(disc) computed
        // rounding of a root: kRel (2 |halfB| + |d| r + 3 sq) / a (sphere_et)
        const double et = kPrimRel * (2.0 * piv_mag(b) + dn * pabs(r) + 3.0 * sq) / a.lo + 1e-300;
        const double far_n = sq - b.lo;  // the far root's numerator, upper bound
        const double far_hi = (far_n >= 0.0 ? far_n / a.lo : far_n / a.hi) * (1.0 + kPrimRel) + et;
        if (far_hi < kPrimTmin) return false;  // behind the camera over the whole footprint
        // origin inside or on the sphere (within the rounding of cc): the far root, bound 0
        if (!(cc > 4.0 * kPrimRel * (oo + rr))) return true;
        // outside: the near root (-halfB - sq) / a = cc / (-halfB + sq), smallest at the largest denominator
        const double den = far_n;
        if (!(den > 0.0)) return true;
        const double t1 = cc / den;
        lo = t1 - kPrimRel * t1 - et;
        return true;
    }
    const int32_t code = __builtin_bit_cast(int32_t, p.g4[3]);
    if (p.type != PRIM_QUAD || code < 1 || code > 6) return true;  // general quads, planes: bound 0
    if (!((float)p.s0 == p.g0[3])) return true;
    // aquad_t_c: tt = (D - n_a o_a) / (n_a d_a), in-plane hit point o + tt d - Q against
    // alpha = sw (ph1 v) in [0, 1], beta = sw (ph2 u) in [0, 1]
    const int ax = (code - 1) % 3, vflag = (code - 1) / 3;
    const int ia = vflag ? (ax + 1) % 3 : (ax + 2) % 3, ib = vflag ? (ax + 2) % 3 : (ax + 1) % 3;
    const double na = (double)p.g3[ax];
    const double no = na * o[ax];
    const double num = p.s0 - no;
    const PIv den = piv_scale(d[ax], na);
    PIv t;
    double idn;
    // `open`: the direction box contains a ray parallel to the plane. The rays that reach the
    // plane in front of the camera then have tt in [t.lo, +inf), t.lo from the box's end on
    // that side; t holds that single value and the in-plane test below is one-sided.
    const bool open = !(den.lo > 0.0 || den.hi < 0.0);
    if (open) {
        const double dd = num > 0.0 ? den.hi : den.lo;
        if (!(num != 0.0) || !(pabs(dd) > 0.0)) return true;  // the origin on the plane: bound 0
        idn = 1.0 / pabs(dd);
        t = PIv{num / dd, num / dd};
    } else {
        const double t0 = num / den.lo, t1 = num / den.hi;
        t = PIv{pmin(t0, t1), pmax(t0, t1)};
        idn = 1.0 / pmin(pabs(den.lo), pabs(den.hi));
    }
    // rounding of tt (aquad_maybe_v's et): kRel ((|D| + |n_a o_a|) / |n_a d_a| + 2 |tt|)
    const double et = kPrimRel * ((pabs(p.s0) + pabs(no)) * idn + 2.0 * piv_mag(t)) + 1e-300;
    if (!open && t.hi + et < kPrimTmin) return false;  // the plane is behind the camera
    const int axes[2] = {ia, ib};
    const double edge[2] = {(double)p.g2[3], (double)p.g1[3]};  // v along ia (alpha), u along ib (beta)
    for (int q = 0; q < 2; ++q) {
        const int c = axes[q];
        const PIv td = piv_mul(t, d[c]);
        PIv ph = {o[c] + td.lo - (double)p.g0[c], o[c] + td.hi - (double)p.g0[c]};
        // in-plane hit-point error times |sw v| (|sw u|), plus alpha's own rounding near [0, 1]
        const double dp = et * piv_mag(d[c]) + kPrimRel * (pabs(o[c]) + piv_mag(td) + pabs((double)p.g0[c]));
        if (open) {
            // beyond t.lo the coordinate moves one way, faster than its error bound grows (dp is
            // at most linear in tt): the value at t.lo bounds it on that side
            if (d[c].lo * t.lo > 2.0 * dp) ph.hi = __builtin_inf();
            else if (d[c].hi * t.lo < -2.0 * dp) ph.lo = -__builtin_inf();
            else continue;
        }
        const double s = (double)p.g3[3] * edge[q];
        const PIv w = piv_scale(ph, s);  // alpha (beta) over the footprint
        const double ew = pabs(s) * dp + 1e-4;
        if (w.hi < -ew || w.lo > 1.0 + ew) return false;
    }
    lo = t.lo - et;
    return true;
}

// Pixel (i, j)'s record. `prims` in slot order, n_prims <= kPrimaryMaxPrims.
RT_HD uint64_t primary_record(const RtCamera& C, const RtPrim* prims, int n_prims, int i, int j) {
    // pixel_center's fp32 operations (pt_shade.hpp); the box below is widened for their
    // rounding anyway, so the value need not be the kernel's in every bit
    double o[3];
    PIv d[3];
    double dn2 = 0.0;
    for (int a = 0; a < 3; ++a) {
        const float pcf = (C.pixel00[a] + C.du[a] * (float)i) + C.dv[a] * (float)j;
        const double pc = (double)pcf, cen = (double)C.center[a];
        const double h = 0.5 * pabs((double)C.du[a]) + 0.5 * pabs((double)C.dv[a]);
        // fp32 roundings between pc and the ray's direction (u = 2^-24 relative each): the two
        // scaled offsets (<= u h together), the two sums (<= u (|pc| + h) and u (|pc| + 2 h)),
        // the subtraction of the centre (<= u (|pc| + 2 h + |center|)): below 3 u (|pc| + |center| + 2 h).
        // 8 u of that sum, more than twice over, also covers pc's own last bits between builds.
        const double e = 8.0 * 0x1p-24 * (pabs(pc) + pabs(cen) + 2.0 * h);
        o[a] = cen;
        d[a] = PIv{pc - cen - h - e, pc - cen + h + e};
        const double m = piv_mag(d[a]);
        dn2 += m * m;
    }
    const double dn = sqrt(dn2);  // >= |d| of every ray of the footprint
    uint32_t mask = 0u, near = 0u, hn = 0u, ho = 0u;
    bool have_near = false, have_other = false;
    for (int k = 0; k < n_prims && k < kPrimaryMaxPrims; ++k) {
        double lo;
        if (!primary_candidate(prims[k], o, d, dn, lo)) continue;
        const uint32_t h = primary_half(lo);
        mask |= 1u << k;
        if (!have_near) {
            have_near = true;
            near = (uint32_t)k;
            hn = h;
        } else {
            uint32_t other = h;
            if (h < hn) {  // non-negative fp16 values order as their bits; ties keep the lower slot
                other = hn;
                near = (uint32_t)k;
                hn = h;
            }
            ho = have_other ? (other < ho ? other : ho) : other;
            have_other = true;
        }
    }
    const uint32_t w0 = mask | near << 16, w1 = hn | ho << 16;
    return (uint64_t)w0 | (uint64_t)w1 << 32;
}

// The host loop over primary_record (rt_camera_primary_table and the CPU tests): W x H records.
void primary_table_host(const RtCamera& C, const RtPrim* prims, int n_prims, uint64_t* out);
#if defined(__HIPCC__)
// The same records from the device: `prims` and `out` (width * height records) in device memory.
hipError_t launch_primary_table(const RtCamera& C, const RtPrim* prims, int n_prims, uint64_t* out,
                                hipStream_t stream);
#endif

}  // namespace rt
