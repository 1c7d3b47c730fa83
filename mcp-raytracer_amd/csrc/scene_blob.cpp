// The scene blob's host build (scene_blob.hpp): the records derived from the primitives and the
// section order. Plain C++ compiled without contraction, like scene.cpp: the stored bases equal
// the ones the kernel would build.
#include "scene_blob.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <stdexcept>

namespace rt {

namespace {

// ONBasis of a hit normal (src/geometry/onbasis.ts:18-51), host side: the same
// rt_math.hpp operations as the kernel's make_onb, so the stored basis equals
// the one the kernel would build (ref: fp64 scalars, -ffp-contract=off).
template <class Real>
RtOnb host_onb(V3 n) {
    const V3 w = unit<Real>(n);
    const V3 a = std::fabs((Real)w.x) > (Real)0.9 ? v3(0, 1, 0) : v3(1, 0, 0);
    const V3 v = unit<Real>(cross<Real>(w, a));
    const V3 u = cross<Real>(w, v);
    return RtOnb{{u.x, u.y, u.z, 0.f}, {v.x, v.y, v.z, 0.f}, {w.x, w.y, w.z, 0.f}};
}

// Per planar primitive slot: [precision ref, fp32][face front, back] bases of
// its hit normals (front: the plane normal; back: Vec3.negate of it). Covers
// slots [0, last planar slot]; empty when the scene has no quad or plane.
std::vector<RtOnb> planar_onbs(const std::vector<RtPrim>& prims, int32_t* n_onb) {
    int32_t n = 0;
    for (size_t k = 0; k < prims.size(); ++k)
        if (prims[k].type != PRIM_SPHERE) n = (int32_t)k + 1;
    std::vector<RtOnb> t((size_t)n * 4, RtOnb{});
    for (int32_t k = 0; k < n; ++k) {
        if (prims[k].type == PRIM_SPHERE) continue;
        const V3 pn = v3(prims[k].g3[0], prims[k].g3[1], prims[k].g3[2]);
        t[k * 4 + 0] = host_onb<double>(pn);
        t[k * 4 + 1] = host_onb<double>(neg(pn));
        t[k * 4 + 2] = host_onb<float>(pn);
        t[k * 4 + 3] = host_onb<float>(neg(pn));
    }
    *n_onb = n;
    return t;
}

// The RtExact records (scene_types.hpp) of a brute-force scene's primitives (empty above
// kBruteMaxPrims: only closest_hit_brute_nf reads them)
std::vector<RtExact> exact_records(const std::vector<RtPrim>& prims) {
    std::vector<RtExact> out;
    if (prims.size() > (size_t)kBlobBruteMaxPrims) return out;
    for (const RtPrim& p : prims) {
        RtExact x{};
        int32_t code = 0;
        std::memcpy(&code, &p.g4[3], sizeof code);
        x.s0 = p.s0;
        x.kind = PRE_OTHER;
        // the fp32 mode's radius / D is (float)s0; a primitive whose g0[3] is not (NaN
        // fields, say) keeps the RtPrim path
        const bool s0f_ok = (float)p.s0 == p.g0[3];
        if (p.type == PRIM_SPHERE && s0f_ok) {
            x.kind = PRE_SPHERE;
            for (int i = 0; i < 3; ++i) x.f[i] = p.g0[i];
        } else if (p.type == PRIM_QUAD && code >= 1 && code <= 6 && s0f_ok) {
            const int a = (code - 1) % 3, vflag = (code - 1) / 3;
            const int ia = vflag ? (a + 1) % 3 : (a + 2) % 3, ib = vflag ? (a + 2) % 3 : (a + 1) % 3;
            if (p.g3[a] == 1.0f || p.g3[a] == -1.0f) {  // always so (a one-component unit normal)
                x.kind = code | (p.g3[a] < 0.0f ? kExactNegNa : 0);
                x.f[0] = p.g0[ia];
                x.f[1] = p.g0[ib];
                x.f[2] = p.g3[3];
                x.f[3] = p.g2[3];
                x.f[4] = p.g1[3];
            }
        }
        out.push_back(x);
    }
    return out;
}

// The RtPre records (scene_types.hpp) of the brute-force pre-filter pass, from the RtPrim fields:
// spheres in pairs, axis-aligned quads in pairs of one axis code, the rest (an odd one out,
// planar quads, planes) one per record. The pass sets each primitive's candidate bit and
// bound by its slot, so the records' order is free; pairs come first. Sets *n_rec.
std::vector<RtPre> prefilter_records(const std::vector<RtPrim>& prims, int32_t* n_rec) {
    struct One {
        int kind;  // PRE_SPHERE, axis code 1..6, PRE_OTHER
        float f[6];
    };
    std::vector<RtPre> out;
    *n_rec = 0;
    if (prims.size() > (size_t)kBlobBruteMaxPrims) {  // closest_hit_brute_nf runs up to kBruteMaxPrims
        out.resize(1);
        return out;
    }
    std::vector<One> one(prims.size());
    for (size_t k = 0; k < prims.size(); ++k) {
        const RtPrim& p = prims[k];
        One q{};
        int32_t code = 0;
        std::memcpy(&code, &p.g4[3], sizeof code);
        if (p.type == PRIM_SPHERE) {
            q.kind = PRE_SPHERE;
            for (int i = 0; i < 4; ++i) q.f[i] = p.g0[i];
        } else if (p.type == PRIM_QUAD && code >= 1 && code <= 6) {
            const int a = (code - 1) % 3, vflag = (code - 1) / 3;
            const int ia = vflag ? (a + 1) % 3 : (a + 2) % 3, ib = vflag ? (a + 2) % 3 : (a + 1) % 3;
            q.kind = code;
            const double asv = (double)p.g3[3] * (double)p.g2[3];  // w_a * v (alpha's factor)
            const double asu = (double)p.g3[3] * (double)p.g1[3];  // w_a * u (beta's factor)
            q.f[0] = (float)(p.s0 / (double)p.g3[a]);          // the plane x_a = D / n_a
            q.f[1] = (float)asv;
            q.f[2] = (float)asu;
            q.f[3] = (float)(-(double)p.g0[ia] * asv - 0.5);  // alpha - 1/2 at the quad's corner
            q.f[4] = (float)(-(double)p.g0[ib] * asu - 0.5);
            constexpr double kRelPre = 1e-5;  // pt_isect.hpp kRel
            q.f[5] = (float)(kRelPre * std::max(std::fabs((double)p.g0[ia]), std::fabs((double)p.g0[ib])) * (1.0 + 1e-6));
        } else {
            q.kind = PRE_OTHER;
        }
        one[k] = q;
    }
    std::vector<bool> used(prims.size(), false);
    auto head = [](int kind, size_t k0, size_t k1) { return (int32_t)(kind | (int)k0 << 8 | (int)k1 << 16); };
    for (size_t k0 = 0; k0 < prims.size(); ++k0) {  // pairs of one kind (sphere / axis code)
        const int kind = one[k0].kind;
        if (used[k0] || kind == PRE_OTHER) continue;
        size_t k1 = k0 + 1;
        while (k1 < prims.size() && (used[k1] || one[k1].kind != kind)) ++k1;
        if (k1 == prims.size()) continue;
        used[k0] = used[k1] = true;
        const One &a = one[k0], &b = one[k1];
        RtPre r{};
        if (kind == PRE_SPHERE) {
            for (int i = 0; i < 4; ++i) {
                r.f[2 * i] = a.f[i];
                r.f[2 * i + 1] = b.f[i];
            }
            r.f[8] = a.f[3] * a.f[3];
            r.f[9] = b.f[3] * b.f[3];
            r.head = head(PRE_SPHERE2, k0, k1);
        } else {
            for (int i = 0; i < 5; ++i) {
                r.f[2 * i] = a.f[i];
                r.f[2 * i + 1] = b.f[i];
            }
            r.f[10] = -std::fabs(a.f[1]);
            r.f[11] = -std::fabs(b.f[1]);
            r.f[12] = -std::fabs(a.f[2]);
            r.f[13] = -std::fabs(b.f[2]);
            r.f[14] = std::max(a.f[5], b.f[5]);
            r.head = head(PRE_QUAD2 + kind, k0, k1);
        }
        out.push_back(r);
    }
    for (size_t k = 0; k < prims.size(); ++k) {  // the rest, one per record
        if (used[k]) continue;
        RtPre r{};
        for (int i = 0; i < 6; ++i) r.f[i] = one[k].f[i];
        r.head = head(one[k].kind, k, 0);
        out.push_back(r);
    }
    *n_rec = (int32_t)out.size();
    if (out.empty()) out.resize(1);  // 16-byte multiple, never empty
    return out;
}

template <class T>
void append(std::vector<char>& blob, const std::vector<T>& v, int32_t* off) {
    if ((v.size() * sizeof(T)) % 16) throw std::runtime_error("blob sections must be 16-byte multiples");
    if (off) *off = (int32_t)blob.size();
    const char* p = reinterpret_cast<const char*>(v.data());
    blob.insert(blob.end(), p, p + v.size() * sizeof(T));
}

}  // namespace

SceneBlob build_scene_blob(const SceneBuild& build) {
    SceneBlob b;
    std::vector<char>& blob = b.bytes;
    append(blob, build.t4nodes, nullptr);  // the fast traversal's 4-wide tree heads the blob
    append(blob, build.tprims, &b.off_tprims);
    append(blob, build.tsph, &b.off_tsph);
    append(blob, build.prims, &b.off_prims);
    append(blob, exact_records(build.prims), &b.off_xrec);
    b.lds_words = (int32_t)(blob.size() / 16);
    append(blob, build.mats, &b.off_mats);
    append(blob, build.lights, &b.off_lights);
    const std::vector<RtOnb> onbs = planar_onbs(build.prims, &b.n_onb);
    append(blob, onbs, &b.off_onbs);
    b.lds_words2 = (int32_t)(blob.size() / 16);
    append(blob, build.nodes, &b.off_nodes);
    append(blob, prefilter_records(build.prims, &b.n_pre), &b.off_pre);
    b.off_tsph2 = -1;
    if (!build.tsph2.empty()) append(blob, build.tsph2, &b.off_tsph2);
    b.size = blob.size();
    return b;
}

}  // namespace rt
