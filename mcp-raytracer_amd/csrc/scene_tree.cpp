// The fast-traversal tree's host build (scene_tree.hpp). Plain C++ compiled without
// contraction, like scene.cpp: the padded boxes and the SAH costs round as written.
#include "scene_tree.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <limits>
#include <stdexcept>

namespace rt {

namespace {

// Boxes for the fast traversal (pt_walk.hpp closest_hit_fast). The
// reference's AABB.hit never accepts a box that is inverted or flat on an
// axis (its per-axis interval is empty), and always accepts one with a NaN
// bound; a strict slab test would treat those differently, so they are
// encoded as "always reject" (NaN in bmin[0]) and "always accept" (infinite
// box). Every other box is padded outward by ~1e-6 relative, so the fp32
// slab test can never cull a box the exact primitive tests would hit.
std::vector<RtNode> make_fast_nodes(const std::vector<RtNode>& nodes) {
    std::vector<RtNode> out(nodes);
    for (RtNode& n : out) {
        bool nan = false, empty = false;
        for (int a = 0; a < 3; ++a) {
            if (std::isnan(n.bmin[a]) || std::isnan(n.bmax[a])) nan = true;
            else if (!(n.bmin[a] < n.bmax[a])) empty = true;
        }
        if (nan) {
            for (int a = 0; a < 3; ++a) { n.bmin[a] = -INFINITY; n.bmax[a] = INFINITY; }
        } else if (empty) {
            n.bmin[0] = NAN;
        } else {
            for (int a = 0; a < 3; ++a) {
                const double lo = n.bmin[a], hi = n.bmax[a];
                if (std::isfinite(lo)) n.bmin[a] = std::nextafter((float)(lo - 1e-6 * (1.0 + std::fabs(lo))), -INFINITY);
                if (std::isfinite(hi)) n.bmax[a] = std::nextafter((float)(hi + 1e-6 * (1.0 + std::fabs(hi))), INFINITY);
            }
        }
    }
    return out;
}

// The padded binary tree (DFS, node 0 = root) collapsed to 4-wide nodes: each
// 4-node takes a binary node's two children and keeps replacing its largest
// interior child by that child's two children until it holds four. Boxes are
// the binary tree's (padded) boxes, so every primitive stays inside each box on
// its path; boxes the reference can never enter (NaN-marked) become empty slots.
int32_t t4_leaf_ref(const RtNode& n) {
    const int32_t count = -n.b;
    if (count < 1 || count > 7 || n.a >= (1 << 27)) throw std::runtime_error("BVH leaf does not fit the TNode code");
    return ~((n.a << 3) | count);
}
double t4_area(const RtNode& n) {
    double e[3];
    for (int a = 0; a < 3; ++a) {
        e[a] = (double)n.bmax[a] - (double)n.bmin[a];
        if (!(e[a] >= 0) || !std::isfinite(e[a])) e[a] = 1e30;
    }
    return e[0] * e[1] + e[1] * e[2] + e[2] * e[0];
}
int32_t t4_build(const std::vector<RtNode>& f, int32_t i, int depth, std::vector<RtT4Node>& out, int& max_depth) {
    max_depth = std::max(max_depth, depth);
    std::vector<int32_t> ch = {f[(size_t)i].a, f[(size_t)i].b};
    while (ch.size() < 4) {
        int best = -1;
        double best_a = -1.0;
        for (size_t k = 0; k < ch.size(); ++k) {
            const RtNode& c = f[(size_t)ch[k]];
            if (c.b >= 0 && !std::isnan(c.bmin[0]) && t4_area(c) > best_a) { best_a = t4_area(c); best = (int)k; }
        }
        if (best < 0) break;
        const RtNode c = f[(size_t)ch[(size_t)best]];
        ch[(size_t)best] = c.a;
        ch.insert(ch.begin() + best + 1, c.b);
    }
    const int32_t idx = (int32_t)out.size();
    out.push_back(RtT4Node{});
    for (int k = 0; k < 4; ++k) {
        RtT4Node& t = out[(size_t)idx];
        for (int a = 0; a < 3; ++a) { t.bmin[a][k] = NAN; t.bmax[a][k] = NAN; }
        t.ref[k] = kT4Empty;
        t.pad[k] = 0;
    }
    for (size_t k = 0; k < ch.size(); ++k) {
        const RtNode& c = f[(size_t)ch[k]];
        if (std::isnan(c.bmin[0])) continue;  // the reference never enters it: no hit below
        const int32_t r = c.b >= 0 ? t4_build(f, ch[k], depth + 1, out, max_depth) : t4_leaf_ref(c);
        RtT4Node& t = out[(size_t)idx];
        for (int a = 0; a < 3; ++a) { t.bmin[a][k] = c.bmin[a]; t.bmax[a][k] = c.bmax[a]; }
        t.ref[k] = r;
    }
    return idx;
}
// The 4-wide nodes re-numbered breadth-first (root 0, then its children, ...): any prefix of
// the array is the top of the tree - the nodes every ray's walk starts with - which a launch
// walking the tree from global memory copies into LDS (pt_walk.hpp t4_node). The walk's
// result does not depend on node numbering (the (t, slot) minimum).
std::vector<RtT4Node> t4_breadth_first(const std::vector<RtT4Node>& in) {
    std::vector<int32_t> order, idx(in.size(), -1);
    order.reserve(in.size());
    order.push_back(0);
    idx[0] = 0;
    for (size_t h = 0; h < order.size(); ++h)
        for (int k = 0; k < 4; ++k) {
            const int32_t r = in[(size_t)order[h]].ref[k];
            if (r >= 0) {  // interior child (leaf codes and empty slots are negative)
                idx[(size_t)r] = (int32_t)order.size();
                order.push_back(r);
            }
        }
    if (order.size() != in.size()) throw std::runtime_error("4-wide tree: unreachable nodes");
    std::vector<RtT4Node> out(in.size());
    for (size_t i = 0; i < order.size(); ++i) {
        RtT4Node n = in[(size_t)order[i]];
        for (int k = 0; k < 4; ++k)
            if (n.ref[k] >= 0) n.ref[k] = idx[(size_t)n.ref[k]];
        out[i] = n;
    }
    return out;
}

std::vector<RtT4Node> make_t4nodes(const std::vector<RtNode>& f, int32_t& root_ref, int& depth) {
    std::vector<RtT4Node> out;
    depth = 0;
    if (f.empty()) { root_ref = ~0; return out; }
    if (f[0].b < 0) { root_ref = t4_leaf_ref(f[0]); return out; }
    root_ref = t4_build(f, 0, 1, out, depth);  // the root is node 0 (pre-order)
    if (out.size() >= (1u << 24)) throw std::runtime_error("4-wide tree: more than 2^24 nodes");  // (t4_node: 24-bit multiply)
    return t4_breadth_first(out);
}

// Fast-traversal tree built for speed, not for the reference's visiting order:
// the fast traversal returns the (t, slot) minimum over all primitives, so any
// tree whose boxes enclose their primitives gives the reference's hit. Binned
// SAH (16 bins on the longest centroid axis, leaves of <= 4), falling back to
// median splits where the depth would outgrow the LDS traversal stack. Leaves
// index `order` (-> SceneBuild::tprims), i.e. reference leaf slots.
struct SahBuilder {
    const std::vector<Box>& pbox;  // per slot
    std::vector<int32_t> order;
    std::vector<RtNode> nodes;     // DFS, RtNode conventions (leaf: a = first, b = -count)
    int cap;                       // maximum depth (root = 1)
    // SAH constants: cost of a traversal step relative to one primitive test, the largest leaf
    // the cost rule may keep, and the size below which a node is always a leaf (defaults 1, 4, 2;
    // RT_AMD_SAH_CT / RT_AMD_SAH_MAXLEAF / RT_AMD_SAH_FORCELEAF override, for A/B)
    // One primitive per leaf where the walk tests a leaf's primitives exactly as it reaches them
    // (no deferred exact tests, pt_walk.hpp leaf_test): trees too large for the LDS-resident copy
    // (> 1,024 primitives: every leaf costs an L2 round trip for its records and its pre-filter loop
    // runs at the lanes that hold it; spheres-100k 2048^2 spp16 with the fp64 leaf records: leaves
    // <= 4: 33.6 ms, <= 2: 32.1, 1: 30.1) and small ones (< 100 primitives; rain-50 1080p spp128:
    // 11.09 -> 10.91 ms). LDS-resident trees of 100 .. 1,024 primitives run the deferred exact tests
    // (launch_plan.cpp v.defer), whose leaf loop is cheap per primitive: they keep <= 4 / 2 (spheres-500:
    // leaves of 1 5.72 -> 5.76 ms, of <= 2 7.27 ms) (profiles/r05/sah/).
    bool one_leaf = pbox.size() > 1024 || pbox.size() < 100;
    double trav_cost = env_double("RT_AMD_SAH_CT", 1.0);
    int max_leaf = std::min(7, std::max(1, (int)env_double("RT_AMD_SAH_MAXLEAF", one_leaf ? 1 : 4)));
    int force_leaf = std::min(max_leaf, std::max(1, (int)env_double("RT_AMD_SAH_FORCELEAF", one_leaf ? 1 : 2)));
    static double env_double(const char* name, double dflt) {
        const char* e = std::getenv(name);
        return (e && e[0]) ? std::atof(e) : dflt;
    }

    SahBuilder(const std::vector<Box>& b, int cap_) : pbox(b), cap(cap_) {
        order.resize(b.size());
        for (size_t i = 0; i < b.size(); ++i) order[i] = (int32_t)i;
    }
    static double area(const Box& b) {
        const double dx = (double)b.mx.x - b.mn.x, dy = (double)b.mx.y - b.mn.y, dz = (double)b.mx.z - b.mn.z;
        return 2.0 * (dx * dy + dy * dz + dz * dx);
    }
    static Box merge(const Box& a, const Box& b) {
        return Box{v3(std::min(a.mn.x, b.mn.x), std::min(a.mn.y, b.mn.y), std::min(a.mn.z, b.mn.z)),
                   v3(std::max(a.mx.x, b.mx.x), std::max(a.mx.y, b.mx.y), std::max(a.mx.z, b.mx.z))};
    }
    static float cen(const Box& b, int a) { return 0.5f * (comp(b.mn, a) + comp(b.mx, a)); }

    int build(int begin, int end, int depth) {
        const int idx = (int)nodes.size();
        nodes.push_back(RtNode{});
        Box bb = pbox[(size_t)order[(size_t)begin]];
        Box cb{v3(INFINITY, INFINITY, INFINITY), v3(-INFINITY, -INFINITY, -INFINITY)};
        for (int i = begin; i < end; ++i) {
            const Box& b = pbox[(size_t)order[(size_t)i]];
            bb = merge(bb, b);
            const V3 c = v3(cen(b, 0), cen(b, 1), cen(b, 2));
            cb = merge(cb, Box{c, c});
        }
        auto set_box = [&](RtNode& n) {
            n.bmin[0] = bb.mn.x; n.bmin[1] = bb.mn.y; n.bmin[2] = bb.mn.z;
            n.bmax[0] = bb.mx.x; n.bmax[1] = bb.mx.y; n.bmax[2] = bb.mx.z;
        };
        const int count = end - begin;
        auto make_leaf = [&]() {
            RtNode& n = nodes[(size_t)idx];
            set_box(n);
            n.a = begin;
            n.b = -count;
            return idx;
        };
        if (count <= force_leaf) return make_leaf();
        int axis = 0;
        float ext[3] = {cb.mx.x - cb.mn.x, cb.mx.y - cb.mn.y, cb.mx.z - cb.mn.z};
        if (ext[1] > ext[axis]) axis = 1;
        if (ext[2] > ext[axis]) axis = 2;
        int mid = -1;
        const int need = (int)std::ceil(std::log2(std::max(1.0, count / (double)max_leaf)));
        if (ext[axis] > 0.0f && depth + need + 2 < cap) {
            constexpr int kBins = 16;
            Box binb[kBins];
            int binn[kBins] = {0};
            const float lo = comp(cb.mn, axis), scale = kBins / ext[axis];
            auto bin_of = [&](const Box& b) {
                int k = (int)((cen(b, axis) - lo) * scale);
                return std::min(std::max(k, 0), kBins - 1);
            };
            for (int i = begin; i < end; ++i) {
                const Box& b = pbox[(size_t)order[(size_t)i]];
                const int k = bin_of(b);
                binb[k] = binn[k] ? merge(binb[k], b) : b;
                ++binn[k];
            }
            double best = INFINITY;
            int best_k = -1;
            for (int k = 1; k < kBins; ++k) {  // split between bin k-1 and k
                Box lb{}, rb{};
                int ln = 0, rn = 0;
                for (int q = 0; q < k; ++q) if (binn[q]) { lb = ln ? merge(lb, binb[q]) : binb[q]; ln += binn[q]; }
                for (int q = k; q < kBins; ++q) if (binn[q]) { rb = rn ? merge(rb, binb[q]) : binb[q]; rn += binn[q]; }
                if (!ln || !rn) continue;
                const double c = area(lb) * ln + area(rb) * rn;
                if (c < best) { best = c; best_k = k; }
            }
            const double leaf_cost = (double)count;
            const double split_cost = trav_cost + best / std::max(area(bb), 1e-30);
            if (count <= max_leaf && !(split_cost < leaf_cost)) return make_leaf();
            if (best_k > 0) {
                auto it = std::partition(order.begin() + begin, order.begin() + end,
                                         [&](int32_t s) { return bin_of(pbox[(size_t)s]) < best_k; });
                mid = (int)(it - order.begin());
                if (mid == begin || mid == end) mid = -1;
            }
        }
        if (mid < 0) {  // median split by centroid (balanced; also for coincident centroids)
            if (count <= max_leaf) return make_leaf();
            mid = begin + count / 2;
            std::nth_element(order.begin() + begin, order.begin() + mid, order.begin() + end, [&](int32_t x, int32_t y) {
                const float cx = cen(pbox[(size_t)x], axis), cy = cen(pbox[(size_t)y], axis);
                return cx < cy || (cx == cy && x < y);
            });
        }
        const int l = build(begin, mid, depth + 1);
        const int r = build(mid, end, depth + 1);
        RtNode& n = nodes[(size_t)idx];
        set_box(n);
        n.a = l;
        n.b = r;
        return idx;
    }
};

}  // namespace

// The fast traversal is exact only if no primitive can be hit outside the box
// the reference gives it: a negative-radius sphere (inverted box, e.g. the
// default scene's hollow glass), a NaN bound, or a plane whose normal passes
// the 0.9999 axis test without being exactly axis-aligned (thin slab box around
// a tilted plane, src/entities/plane.ts:280-307). Such scenes use the
// reference-order traversal.
bool prims_inside_boxes(const std::vector<RtPrim>& prims) {
    for (const RtPrim& p : prims) {
        for (int k = 0; k < 4; ++k) {
            if (std::isnan(p.g0[k])) return false;
            // a sphere's g1 holds its reciprocal radius (double bits), its g2..g4 are unused
            if (p.type != PRIM_SPHERE &&
                (std::isnan(p.g1[k]) || std::isnan(p.g2[k]) || std::isnan(p.g3[k]) || std::isnan(p.g4[k])))
                return false;
        }
        if (std::isnan(p.s0)) return false;
        if (p.type == PRIM_SPHERE) {
            if (!(p.s0 > 0) || !std::isfinite(p.s0)) return false;
        } else if (p.type == PRIM_PLANE) {
            const double n[3] = {p.g3[0], p.g3[1], p.g3[2]};
            for (int a = 0; a < 3; ++a) {
                if (std::fabs(n[a]) > 0.9999) {
                    const bool exact = std::fabs(n[a]) == 1.0 && n[(a + 1) % 3] == 0.0 && n[(a + 2) % 3] == 0.0;
                    if (!exact) return false;
                    break;
                }
            }
        }
    }
    return true;
}

// AABB.hit subtracts the ray origin from both faces of an axis in doubles (aabb.ts:36-60) and
// rejects the box when `tmax <= tmin`. From an origin of magnitude M two faces closer than
// ulp(M) = M 2^-52 round to the same difference: the reference then never enters a box the ray
// crosses (a camera at y = 1e20 above the floor plane's 2e-4 slab; a sphere whose radius is lost
// in its centre's fp32 store) while brute force and the fast walk, which do not depend on that
// box, still hit the primitive. Ray origins are the camera centre and hit points, which lie in
// the primitives' boxes (or anywhere on an infinite plane: not covered). So every finite extent
// must be positive and at least 2^10 ulp(M), M the largest finite coordinate of any box or of
// the centre; a centre that is not finite fails too. Such scenes use the reference-order traversal.
bool boxes_keep_their_extent(const std::vector<Box>& boxes, V3 center) {
    double big = 0.0, thin = INFINITY;
    for (float c : {center.x, center.y, center.z}) {
        if (!std::isfinite(c)) return false;
        big = std::max(big, std::fabs((double)c));
    }
    for (const Box& b : boxes) {
        for (int a = 0; a < 3; ++a) {
            const double lo = comp(b.mn, a), hi = comp(b.mx, a);
            if (std::isfinite(lo)) big = std::max(big, std::fabs(lo));
            if (std::isfinite(hi)) big = std::max(big, std::fabs(hi));
            if (std::isfinite(lo) && std::isfinite(hi)) thin = std::min(thin, hi - lo);
        }
    }
    return thin > 0.0 && thin >= std::ldexp(big, -42);  // (also false for a NaN extent)
}

void build_fast_tree(SceneBuild& out, const std::vector<Box>& slot_box) {
    // SAH over the reference's per-object boxes (finite boxes only, i.e. no planes), else the
    // reference tree itself
    bool finite = true;
    for (const Box& x : slot_box) {
        for (float v : {x.mn.x, x.mn.y, x.mn.z, x.mx.x, x.mx.y, x.mx.z})
            if (!std::isfinite(v)) finite = false;
        if (!(x.mn.x <= x.mx.x && x.mn.y <= x.mx.y && x.mn.z <= x.mx.z)) finite = false;
    }
    const char* env = std::getenv("RT_AMD_SAH");
    const bool sah = finite && slot_box.size() > 16 && !(env && env[0] == '0');
    if (sah) {
        SahBuilder sb(slot_box, std::max(out.bvh_depth + 2, 12));
        sb.build(0, (int)slot_box.size(), 1);
        out.tprims = sb.order;
        const std::vector<RtNode> padded = make_fast_nodes(sb.nodes);
        out.t4nodes = make_t4nodes(padded, out.t4root, out.t4depth);
        out.t4root_box = padded[0];
    } else {
        out.tprims.resize(out.prims.size());
        for (size_t k = 0; k < out.tprims.size(); ++k) out.tprims[k] = (int32_t)k;
        const std::vector<RtNode> fnodes = make_fast_nodes(out.nodes);
        out.t4nodes = make_t4nodes(fnodes, out.t4root, out.t4depth);
        out.t4root_box = fnodes[0];
    }
    out.tprims.resize((out.tprims.size() + 3) / 4 * 4, 0);  // 16-byte blob sections
    // leaf-order sphere records for the fp32 pre-filter: contiguous per leaf and
    // a quarter of a primitive record, so large scenes stay cache-resident
    out.tsph.assign(out.tprims.size() * 4, std::numeric_limits<float>::quiet_NaN());
    out.tsph2.assign(out.tprims.size(), RtLeafSph{});
    for (size_t m = 0; m < out.tprims.size(); ++m) {
        const RtPrim& p = out.prims[(size_t)out.tprims[m]];
        RtLeafSph& q = out.tsph2[m];
        q.slot = out.tprims[m];
        for (int c = 0; c < 3; ++c) q.c[c] = std::numeric_limits<float>::quiet_NaN();
        q.r32 = std::numeric_limits<float>::quiet_NaN();
        if (p.type == PRIM_SPHERE) {
            for (int c = 0; c < 4; ++c) out.tsph[m * 4 + c] = p.g0[c];
            for (int c = 0; c < 3; ++c) q.c[c] = p.g0[c];
            q.r32 = p.g0[3];
            q.r64 = p.s0;  // the JS double radius (sphere_radius<double>)
        }
    }
}

}  // namespace rt
