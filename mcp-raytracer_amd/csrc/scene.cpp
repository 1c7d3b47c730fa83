// Host side of the drop-in: SceneData -> flat device arrays (createCameraFromSceneData).
// The scene generators are scene_gen.cpp, the fast-traversal tree is scene_tree.cpp.
//
// Each function cites the reference code it restates. Vector quantities are
// fp32 (gl-matrix Float32Array), scalars are doubles, exactly as the reference.
#include "scene.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "scene_js.hpp"
#include "scene_tree.hpp"

namespace rt {

// V8 Math.hypot (used by gl-matrix vec3.length)
double v8_hypot3(double x, double y, double z) {
    double vals[3] = {x, y, z};
    double absv[3] = {0, 0, 0};
    bool nan = false;
    double mx = 0;
    for (int i = 0; i < 3; ++i) {
        if (std::isnan(vals[i])) { nan = true; continue; }
        absv[i] = std::fabs(vals[i]);
        if (absv[i] > mx) mx = absv[i];
    }
    if (mx == INFINITY) return INFINITY;
    if (nan) return NAN;
    if (mx == 0) return 0;
    double sum = 0, comp = 0;
    for (int i = 0; i < 3; ++i) {
        double n = absv[i] / mx;
        double summand = n * n - comp;
        double prelim = sum + summand;
        comp = (prelim - sum) - summand;
        sum = prelim;
    }
    return std::sqrt(sum) * mx;
}

static double vlength(V3 a) { return v8_hypot3(a.x, a.y, a.z); }

// createCameraFromSceneData (src/scenes/scenes.ts:60-104)
namespace {

// AABB.surroundingBox (src/geometry/aabb.ts:68-82)
Box surrounding(const Box& a, const Box& b) {
    return Box{mk<double>(js_min<double>(a.mn.x, b.mn.x), js_min<double>(a.mn.y, b.mn.y), js_min<double>(a.mn.z, b.mn.z)),
               mk<double>(js_max<double>(a.mx.x, b.mx.x), js_max<double>(a.mx.y, b.mx.y), js_max<double>(a.mx.z, b.mx.z))};
}

Box empty_box() { return Box{mk<double>(INFINITY, INFINITY, INFINITY), mk<double>(-INFINITY, -INFINITY, -INFINITY)}; }

struct Builder {
    const Value& scene;
    std::unordered_map<std::string, const Value*> matmap;
    SceneBuild out;
    std::vector<Box> boxes;  // per object

    explicit Builder(const Value& s) : scene(s) {}

    int add_mat(RtMat m) {
        out.mats.push_back(m);
        return (int)out.mats.size() - 1;
    }

    const Value* resolve(const Value* ref) {
        if (ref && ref->is_string()) {
            auto it = matmap.find(ref->str);
            return it == matmap.end() ? nullptr : it->second;
        }
        if (!ref || ref->is_null()) return nullptr;
        if (ref->is_bool() && !ref->b) return nullptr;
        if (ref->is_number() && (ref->num == 0 || std::isnan(ref->num))) return nullptr;
        return ref;
    }

    // createMaterial (src/scenes/scenes.ts:144-180). Returns a material index.
    // The reference recurses on the JS stack and a material that reaches itself
    // ends as a RangeError; here the materials being resolved are kept on `resolving`
    // and re-entry, or more than kMaxMaterialDepth of them, fails with that message.
    static constexpr size_t kMaxMaterialDepth = 1000;
    std::vector<const Value*> resolving;
    struct Resolving {
        std::vector<const Value*>& s;
        Resolving(std::vector<const Value*>& st, const Value* md) : s(st) { s.push_back(md); }
        ~Resolving() { s.pop_back(); }
    };

    int create_material(const Value* ref) {
        const Value* md = resolve(ref);
        if (!md) fail("Material not found: " + js_string(ref));
        if (resolving.size() >= kMaxMaterialDepth || std::find(resolving.begin(), resolving.end(), md) != resolving.end())
            fail("Maximum call stack size exceeded (material " + js_string(ref) + ")");
        Resolving guard(resolving, md);
        const Value* tv = md->get("type");
        const std::string type = tv && tv->is_string() ? tv->str : js_string(tv);
        RtMat m{};
        m.c0 = m.c1 = -1;
        if (type == "lambert") {
            m.type = MAT_LAMBERT;
            V3 c = vec_from(md->get("color"), "materialData.color");
            m.color[0] = c.x; m.color[1] = c.y; m.color[2] = c.z;
        } else if (type == "metal") {
            m.type = MAT_METAL;
            V3 c = vec_from(md->get("color"), "materialData.color");
            m.color[0] = c.x; m.color[1] = c.y; m.color[2] = c.z;
            // Metal ctor: fuzz default 0.0; fuzz < 1 ? Math.max(0, fuzz) : 1 (src/materials/metal.ts:20)
            const Value* fv = md->get("fuzz");
            double fuzz = fv ? to_number(fv, 0.0) : 0.0;
            m.p0 = fuzz < 1 ? js_max<double>(0, fuzz) : 1;
        } else if (type == "glass") {
            m.type = MAT_GLASS;
            m.p0 = to_number(md->get("ior"), NAN);
        } else if (type == "light") {
            m.type = MAT_LIGHT;
            V3 c = vec_from(md->get("emit"), "materialData.emit");
            m.color[0] = c.x; m.color[1] = c.y; m.color[2] = c.z;
        } else if (type == "mixed") {
            m.type = MAT_MIXED;
            m.c0 = create_material(md->get("diff"));
            m.c1 = create_material(md->get("spec"));
            // weight = Math.max(0.0, Math.min(1.0, weight)) (src/materials/mixedMaterial.ts:29)
            m.p0 = js_max<double>(0.0, js_min<double>(1.0, to_number(md->get("weight"), NAN)));
        } else if (type == "layered") {
            m.type = MAT_LAYERED;
            // createDielectric (src/scenes/scenes.ts:182-199) runs before the inner material.
            const Value* oref = md->get("outer");
            const Value* od = resolve(oref);
            if (!od) fail("Material not found: " + js_string(oref));
            const Value* otv = od->get("type");
            if (!(otv && otv->is_string() && otv->str == "glass"))
                fail("Material is not a dielectric: " + js_string(oref));
            RtMat g{};
            g.type = MAT_GLASS;
            g.c0 = g.c1 = -1;
            g.p0 = to_number(od->get("ior"), NAN);
            m.c0 = add_mat(g);
            m.c1 = create_material(md->get("inner"));
        } else {
            fail("Unknown material type: " + type);
        }
        return add_mat(m);
    }

    // Material.emitted(rec) is a constant per material: DefaultMaterial -> BLACK,
    // DiffuseLight -> emit, Mixed -> E1*w + E2*(1-w), Layered -> inner's.
    // Both walk a material's children, which create_material nests at most
    // kMaxMaterialDepth deep; `level` holds them to that bound on their own.
    static void check_level(size_t level) {
        if (level > kMaxMaterialDepth) fail("Maximum call stack size exceeded (material nesting)");
    }
    V3 emitted_of(int mi, size_t level = 1) {
        check_level(level);
        const RtMat& m = out.mats[mi];
        switch (m.type) {
            case MAT_LIGHT: return v3(m.color[0], m.color[1], m.color[2]);
            case MAT_MIXED: {
                V3 e1 = scale<double>(emitted_of(m.c0, level + 1), m.p0);
                V3 e2 = scale<double>(emitted_of(m.c1, level + 1), 1.0 - m.p0);
                return add(e1, e2);
            }
            case MAT_LAYERED: return emitted_of(m.c1, level + 1);
            default: return v3(0, 0, 0);
        }
    }
    bool can_scatter(int mi, size_t level = 1) {
        check_level(level);
        const RtMat& m = out.mats[mi];
        if (m.type == MAT_LIGHT) return false;
        if (m.type == MAT_MIXED) return can_scatter(m.c0, level + 1) || can_scatter(m.c1, level + 1);
        return true;
    }

    // Plane ctor (src/entities/plane.ts:180-200) + boxes (plane.ts:276-308,
    // quad.ts:400-422); Sphere ctor (sphere.ts:20-31).
    // Axis-aligned quad (u, v each along one axis): the kernel evaluates the
    // reference's Plane.intersect / alpha / beta with the zero terms dropped,
    // which rounds identically (pt_isect.hpp aquad_t). Encoding:
    //   g4[3] = int code 1 + a + 3*vflag (a = normal axis; vflag: v along (a+2)%3),
    //   g3[3] = +-w[a] (sign folded from the cross product), g2[3] = v's nonzero
    //   component, g1[3] = u's nonzero component. code 0 = general quad.
    static void encode_axis_quad(RtPrim& p, V3 u, V3 v, V3 cp, V3 w) {
        const float uu[3] = {u.x, u.y, u.z}, vv[3] = {v.x, v.y, v.z}, cc[3] = {cp.x, cp.y, cp.z},
                    ww[3] = {w.x, w.y, w.z};
        auto only = [](const float* x) {
            int k = -1;
            for (int i = 0; i < 3; ++i) {
                if (!std::isfinite(x[i])) return -2;
                if (x[i] != 0.0f) k = (k == -1) ? i : -2;
            }
            return k;
        };
        const int iu = only(uu), iv = only(vv), a = only(cc), iw = only(ww);
        if (iu < 0 || iv < 0 || a < 0 || iw != a || iu == iv || iu == a || iv == a) return;
        const int b = (a + 1) % 3, c = (a + 2) % 3;
        const bool vflag = iv == c;  // then u is along b
        if (!(vflag ? iu == b : (iv == b && iu == c))) return;
        int32_t code = 1 + a + 3 * (vflag ? 1 : 0);
        std::memcpy(&p.g4[3], &code, sizeof code);
        p.g3[3] = vflag ? ww[a] : -ww[a];
        p.g2[3] = vv[iv];
        p.g1[3] = uu[iu];
    }

    RtPrim make_prim(const Value& od, int mat, Box& box, std::string& type_out) {
        RtPrim p{};
        p.mat = mat;
        const Value* tv = od.get("type");
        const std::string type = tv && tv->is_string() ? tv->str : js_string(tv);
        type_out = type;
        if (type == "sphere") {
            p.type = PRIM_SPHERE;
            V3 c = vec_from(od.get("pos"), "objectData.pos");
            double r = to_number(od.get("r"), NAN);
            p.s0 = r;
            p.g0[0] = c.x; p.g0[1] = c.y; p.g0[2] = c.z; p.g0[3] = (float)r;
            {  // reciprocal radius for the hit normal (kernel sphere_inv_radius)
                const double ir = 1.0 / r;
                std::memcpy(&p.g1[0], &ir, sizeof ir);
                const float irf = 1.0f / (float)r;
                p.g1[2] = irf;
            }
            V3 rv = mk<double>(r, r, r);
            box = Box{sub(c, rv), add(c, rv)};
            return p;
        }
        if (type == "plane" || type == "quad") {
            p.type = type == "plane" ? PRIM_PLANE : PRIM_QUAD;
            V3 q = vec_from(od.get("pos"), "objectData.pos");
            V3 u = vec_from(od.get("u"), "objectData.u");
            V3 v = vec_from(od.get("v"), "objectData.v");
            V3 cp = cross<double>(u, v);
            V3 n = unit<double>(cp);
            double d = dot<double>(n, q);
            double cl2 = len2<double>(cp);
            V3 w = divs<double>(cp, cl2);
            p.s0 = d;
            p.g0[0] = q.x; p.g0[1] = q.y; p.g0[2] = q.z; p.g0[3] = (float)d;
            p.g1[0] = u.x; p.g1[1] = u.y; p.g1[2] = u.z;
            p.g2[0] = v.x; p.g2[1] = v.y; p.g2[2] = v.z;
            p.g3[0] = n.x; p.g3[1] = n.y; p.g3[2] = n.z;
            p.g4[0] = w.x; p.g4[1] = w.y; p.g4[2] = w.z;
            // general quads: |w||u|, |w||v| (rounded up) scale the kernel's alpha/beta
            // error margins (pt_walk.hpp planar_maybe); axis quads re-use the slots
            {
                const double wn = std::sqrt(len2<double>(w));
                p.g1[3] = (float)(wn * std::sqrt(len2<double>(u)) * (1.0 + 1e-5));
                p.g2[3] = (float)(wn * std::sqrt(len2<double>(v)) * (1.0 + 1e-5));
            }
            if (p.type == PRIM_QUAD) encode_axis_quad(p, u, v, cp, w);
            if (p.type == PRIM_PLANE) {
                const double eps = 1e-4;
                if (std::fabs((double)n.x) > 0.9999) {
                    double px = d / (double)n.x;
                    box = Box{mk<double>(px - eps, -INFINITY, -INFINITY), mk<double>(px + eps, INFINITY, INFINITY)};
                } else if (std::fabs((double)n.y) > 0.9999) {
                    double py = d / (double)n.y;
                    box = Box{mk<double>(-INFINITY, py - eps, -INFINITY), mk<double>(INFINITY, py + eps, INFINITY)};
                } else if (std::fabs((double)n.z) > 0.9999) {
                    double pz = d / (double)n.z;
                    box = Box{mk<double>(-INFINITY, -INFINITY, pz - eps), mk<double>(INFINITY, INFINITY, pz + eps)};
                } else {
                    box = Box{mk<double>(-INFINITY, -INFINITY, -INFINITY), mk<double>(INFINITY, INFINITY, INFINITY)};
                }
            } else {
                V3 v1 = q, v2 = add(q, u), v3_ = add(q, v), v4 = add(add(q, u), v);
                auto mn4 = [](double a, double b, double c, double e) {
                    return js_min<double>(js_min<double>(js_min<double>(a, b), c), e);
                };
                auto mx4 = [](double a, double b, double c, double e) {
                    return js_max<double>(js_max<double>(js_max<double>(a, b), c), e);
                };
                const double eps = 1e-4;
                double mnx = mn4(v1.x, v2.x, v3_.x, v4.x), mny = mn4(v1.y, v2.y, v3_.y, v4.y),
                       mnz = mn4(v1.z, v2.z, v3_.z, v4.z);
                double mxx = mx4(v1.x, v2.x, v3_.x, v4.x), mxy = mx4(v1.y, v2.y, v3_.y, v4.y),
                       mxz = mx4(v1.z, v2.z, v3_.z, v4.z);
                box = Box{mk<double>(mnx - eps, mny - eps, mnz - eps), mk<double>(mxx + eps, mxy + eps, mxz + eps)};
            }
            return p;
        }
        fail("Unknown object type: " + type);
    }

    // BVHNode ctor (src/geometry/bvh.ts:34-102). `list` is this node's
    // objectsList. Array.prototype.sort with the comparator
    // (a,b) => boxA.min[axis] < boxB.min[axis] ? -1 : 1 is V8's TimSort, which
    // only ever calls the comparator as (later element, earlier element); with
    // this comparator that makes ties keep input order, i.e. a stable sort.
    int build(std::vector<int> list, int depth, Box& node_box) {
        out.bvh_depth = std::max(out.bvh_depth, depth);
        Box nb = boxes[list[0]];
        for (size_t k = 1; k < list.size(); ++k) nb = surrounding(nb, boxes[list[k]]);
        const double xe = (double)nb.mx.x - (double)nb.mn.x;
        const double ye = (double)nb.mx.y - (double)nb.mn.y;
        const double ze = (double)nb.mx.z - (double)nb.mn.z;
        int axis = 0;
        if (ye > xe && ye > ze) axis = 1;
        else if (ze > xe && ze > ye) axis = 2;
        const size_t span = list.size();

        const int self = (int)out.nodes.size();
        out.nodes.push_back(RtNode{});
        auto less = [&](int a, int b) { return comp(boxes[a].mn, axis) < comp(boxes[b].mn, axis); };

        Box box;
        if (span <= 4) {
            std::vector<int> leaf;
            if (span == 1) {
                leaf = {list[0]};
                box = surrounding(boxes[list[0]], empty_box());
            } else if (span == 2) {
                if (less(list[0], list[1])) leaf = {list[0], list[1]};
                else leaf = {list[1], list[0]};
                box = surrounding(boxes[leaf[0]], boxes[leaf[1]]);
            } else {
                leaf = list;
                // HittableList.boundingBox (src/geometry/hittableList.ts:29-52)
                Box lb = boxes[leaf[0]];
                for (size_t k = 1; k < leaf.size(); ++k) lb = surrounding(lb, boxes[leaf[k]]);
                box = surrounding(lb, empty_box());
            }
            RtNode& n = out.nodes[self];
            n.a = (int32_t)out.prims.size();
            n.b = -(int32_t)leaf.size();
            for (int o : leaf) {
                out.prims.push_back(tmp_prims[o]);
                out.prim_object.push_back(o);
            }
        } else {
            std::stable_sort(list.begin(), list.end(), less);
            const size_t mid = span / 2;
            std::vector<int> l(list.begin(), list.begin() + mid), r(list.begin() + mid, list.end());
            Box lbx, rbx;
            int li = build(std::move(l), depth + 1, lbx);
            int ri = build(std::move(r), depth + 1, rbx);
            out.nodes[self].a = li;
            out.nodes[self].b = ri;
            box = surrounding(lbx, rbx);
        }
        RtNode& n = out.nodes[self];
        n.bmin[0] = box.mn.x; n.bmin[1] = box.mn.y; n.bmin[2] = box.mn.z;
        n.bmax[0] = box.mx.x; n.bmax[1] = box.mx.y; n.bmax[2] = box.mx.z;
        node_box = box;
        return self;
    }

    std::vector<RtPrim> tmp_prims;
};

// Spread-merge lookup: provided render options win over the scene's (scenes.ts:97-100).
const Value* render_opt(const Value* scene_render, const Value* provided, const char* key) {
    if (provided && provided->is_object()) {
        if (const Value* v = provided->get(key)) return v;
    }
    if (scene_render && scene_render->is_object()) {
        if (const Value* v = scene_render->get(key)) return v;
    }
    return nullptr;
}

int32_t loop_threshold(double x) {
    // Smallest integer n with (n >= x) for integer counters starting at 0.
    if (std::isnan(x)) return INT32_MAX;
    if (x <= 0) return 0;
    if (x > 1e9) return 1000000000;
    return (int32_t)std::ceil(x);
}

// RenderOptions.seed -> the RNG's 32-bit seed word: a non-finite number is 0, any other is
// truncated towards zero and taken modulo 2^32 (so -1 is 0xFFFFFFFF and 2^32 + 5 is 5).
uint32_t seed_word(double seed) {
    if (!std::isfinite(seed)) return 0;
    double m = std::fmod(std::trunc(seed), 4294967296.0);  // exact, inside (-2^32, 2^32)
    if (m < 0) m += 4294967296.0;
    return (uint32_t)m;
}

}  // namespace

SceneBuild build_scene(const Value& scene_data, const Value* render_options) {
    if (!scene_data.is_object()) fail("sceneData must be an object");
    Builder b(scene_data);

    // materials lookup: sceneData.materials?.forEach(({id, material}) => ...)
    if (const Value* mats = scene_data.get("materials")) {
        if (mats->is_array()) {
            for (const Value& e : mats->arr) {
                const Value* id = e.get("id");
                const Value* m = e.get("material");
                b.matmap[js_string(id)] = m;
            }
        }
    }
    const Value* objs = scene_data.get("objects");
    if (!objs || !objs->is_array()) fail("Cannot read properties of undefined (reading 'map')");
    const size_t nobj = objs->arr.size();
    if (nobj == 0) fail("Cannot read properties of null (reading 'maximum')");  // BVHNode over an empty list

    b.boxes.resize(nobj);
    b.tmp_prims.resize(nobj);
    std::vector<std::string> types(nobj);
    for (size_t i = 0; i < nobj; ++i) {
        const Value& od = objs->arr[i];
        int mat = b.create_material(od.get("material"));
        b.tmp_prims[i] = b.make_prim(od, mat, b.boxes[i], types[i]);
    }
    // emitted constants + emissive-scatter flag
    int emissive_scatter = 0;
    for (size_t mi = 0; mi < b.out.mats.size(); ++mi) {
        V3 e = b.emitted_of((int)mi);
        RtMat& m = b.out.mats[mi];
        m.emitted[0] = e.x; m.emitted[1] = e.y; m.emitted[2] = e.z;
        bool nz = !(e.x == 0.0f && e.y == 0.0f && e.z == 0.0f);
        if (nz && b.can_scatter((int)mi)) emissive_scatter = 1;
    }

    // world = BVHNode.fromList(objects)
    std::vector<int> all(nobj);
    for (size_t i = 0; i < nobj; ++i) all[i] = (int)i;
    Box root_box;
    b.build(all, 1, root_box);

    // lights: objData.light && 'pdf' in object  (Sphere and Quad are PDFHittable)
    std::vector<int> slot_of(nobj);
    for (size_t s = 0; s < b.out.prim_object.size(); ++s) slot_of[b.out.prim_object[s]] = (int)s;
    for (size_t i = 0; i < nobj; ++i) {
        const Value& od = objs->arr[i];
        if (!truthy(od.get("light"))) continue;
        if (types[i] != "sphere" && types[i] != "quad") continue;
        RtLight l{};
        l.prim = slot_of[i];
        l.type = types[i] == "sphere" ? PRIM_SPHERE : PRIM_QUAD;
        if (l.type == PRIM_QUAD) {
            const RtPrim& p = b.tmp_prims[i];
            V3 u = v3(p.g1[0], p.g1[1], p.g1[2]), v = v3(p.g2[0], p.g2[1], p.g2[2]);
            l.area = vlength(cross<double>(u, v));  // Quad.area = u.cross(v).length()
        }
        b.out.lights.push_back(l);
    }

    // A throughput that is not finite makes the zero emission of every later hit NaN (0 * NaN,
    // 0 * inf: emitted.multiplyVec(throughput), camera.ts:261), so such paths need the emission
    // stack as well. The scene can produce one through a scattering material with a non-finite
    // colour (the attenuation) or a light whose geometry is not finite (its direction and PDF
    // value are NaN, and NaN <= 0.0001 does not end the path).
    for (const RtMat& m : b.out.mats)
        if ((m.type == MAT_LAMBERT || m.type == MAT_METAL) &&
            !(std::isfinite(m.color[0]) && std::isfinite(m.color[1]) && std::isfinite(m.color[2])))
            emissive_scatter = 1;
    for (const RtLight& l : b.out.lights) {
        const RtPrim& p = b.out.prims[(size_t)l.prim];
        bool finite = std::isfinite(p.s0);
        for (int k = 0; k < 3; ++k)
            finite = finite && std::isfinite(p.g0[k]) &&
                     (p.type == PRIM_SPHERE || (std::isfinite(p.g1[k]) && std::isfinite(p.g2[k])));
        if (!finite) emissive_scatter = 1;
    }

    // Camera (src/camera.ts:107-166) with createCameraFromSceneData's option mapping
    const Value* camd = scene_data.get("camera");
    if (!camd || !camd->is_object()) fail("Cannot read properties of undefined (reading 'vfov')");
    RtCamera& cam = b.out.cam;

    const Value* vfv = camd->get("vfov");
    const double vfov = vfv ? to_number(vfv, NAN) : NAN;  // undefined overrides the default
    if (!truthy(camd->get("from"))) fail("Cannot read properties of undefined (reading 'subtract')");
    if (!truthy(camd->get("at"))) fail("Cannot read properties of undefined (reading 'glVec')");
    if (!truthy(camd->get("up"))) fail("Cannot read properties of undefined (reading 'cross')");
    const V3 from = vec_from(camd->get("from"), "camera.from");
    const V3 at = vec_from(camd->get("at"), "camera.at");
    const V3 up = vec_from(camd->get("up"), "camera.up");
    const Value* apv = camd->get("aperture");
    const double aperture = apv ? to_number(apv, NAN) : NAN;
    const Value* fov = camd->get("focus");
    const double focus = fov ? to_number(fov, NAN) : NAN;
    const Value* bgv = camd->get("background");
    const bool has_bg = truthy(bgv);
    V3 bg_top{0, 0, 0}, bg_bottom{0, 0, 0};
    if (has_bg) {
        bg_top = vec_from(bgv->get("top"), "camera.background.top");
        bg_bottom = vec_from(bgv->get("bottom"), "camera.background.bottom");
    }

    // render options: {...defaultRenderData, ...sceneData.render, ...renderOptions}
    const Value* srender = scene_data.get("render");
    auto ropt = [&](const char* key) { return render_opt(srender, render_options, key); };
    const double width = ropt("width") ? to_number(ropt("width"), NAN) : 400;
    const double aspect = ropt("aspect") ? to_number(ropt("aspect"), NAN) : 16.0 / 9.0;
    const double samples = ropt("samples") ? to_number(ropt("samples"), NAN) : 100;
    const double depth = ropt("depth") ? to_number(ropt("depth"), NAN) : 100;
    const double aTol = ropt("aTolerance") ? to_number(ropt("aTolerance"), NAN) : 0.05;
    const double aBatch = ropt("aBatch") ? to_number(ropt("aBatch"), NAN) : 10;
    const bool roulette = ropt("roulette") ? truthy(ropt("roulette")) : true;
    const double rdepth = ropt("rouletteDepth") ? to_number(ropt("rouletteDepth"), NAN) : 3;
    std::string mode = "default";
    if (const Value* mv = ropt("mode")) mode = js_string(mv);
    const Value* sv = ropt("seed");
    const double seed = sv ? to_number(sv, 0) : (double)0x5EED;

    const double imageHeight = std::ceil(width / aspect);
    if (!(width >= 0) || width != std::floor(width) || width > 1e6 || !(imageHeight >= 0) || imageHeight > 1e6)
        fail("Invalid typed array length: image " + num_str(width) + "x" + num_str(imageHeight));
    if (std::isnan(depth)) fail("Maximum call stack size exceeded (depth is NaN)");

    const double focusDistance = (focus != 0 && !std::isnan(focus)) ? focus : vlength(sub(from, at));
    const double theta = vfov * (kPI / 180);
    const double h = std::tan(theta / 2);
    const double viewportHeight = 2 * h * focusDistance;
    const double aspectRatio = width / imageHeight;
    const double viewportWidth = viewportHeight * aspectRatio;
    const V3 w = unit<double>(sub(from, at));
    const V3 u = unit<double>(cross<double>(up, w));
    const V3 v = cross<double>(w, u);
    const V3 viewportU = scale<double>(u, viewportWidth);
    const V3 viewportV = scale<double>(v, -viewportHeight);
    const V3 pdu = divs<double>(viewportU, width);
    const V3 pdv = divs<double>(viewportV, imageHeight);
    const V3 halfU = divs<double>(viewportU, 2.0);
    const V3 halfV = divs<double>(viewportV, 2.0);
    const V3 upperLeft = sub(sub(sub(from, scale<double>(w, focusDistance)), halfU), halfV);
    const V3 p00 = add(upperLeft, scale<double>(add(pdu, pdv), 0.5));
    const V3 ddu = scale<double>(u, aperture / 2);
    const V3 ddv = scale<double>(v, aperture / 2);

    auto put = [](float* d, V3 s) { d[0] = s.x; d[1] = s.y; d[2] = s.z; d[3] = 0; };
    put(cam.pixel00, p00);
    put(cam.du, pdu);
    put(cam.dv, pdv);
    put(cam.center, from);
    put(cam.ddu, ddu);
    put(cam.ddv, ddv);
    put(cam.bg_top, bg_top);
    put(cam.bg_bottom, bg_bottom);
    cam.aperture = aperture;
    cam.samples = samples;
    cam.a_tolerance = aTol;
    cam.a_batch = aBatch;
    cam.depth_raw = depth;
    cam.width = (int32_t)width;
    cam.height = (int32_t)imageHeight;
    cam.n_samples = loop_threshold(samples);
    if (cam.n_samples == INT32_MAX) cam.n_samples = 0;  // NaN samples: the while loop never runs
    cam.depth = loop_threshold(depth);
    cam.roulette = roulette ? 1 : 0;
    cam.roulette_depth = loop_threshold(rdepth);
    cam.mode = mode == "bounces" ? MODE_BOUNCES : (mode == "samples" ? MODE_SAMPLES : MODE_DEFAULT);
    cam.adaptive = (aTol > 0 && samples > 1) ? 1 : 0;
    cam.n_lights = (int32_t)b.out.lights.size();
    cam.has_background = has_bg ? 1 : 0;
    cam.emissive_scatter = emissive_scatter;
    cam.n_nodes = (int32_t)b.out.nodes.size();
    cam.n_prims = (int32_t)b.out.prims.size();
    cam.n_mats = (int32_t)b.out.mats.size();
    cam.seed = seed_word(seed);
    cam.seed_mix = splitmix64(cam.seed);
    // fast-traversal tree over the reference's per-object boxes, in slot order (scene_tree.cpp)
    {
        std::vector<Box> slot_box(b.out.prims.size());
        for (size_t k = 0; k < slot_box.size(); ++k) slot_box[k] = b.boxes[(size_t)b.out.prim_object[k]];
        build_fast_tree(b.out, slot_box);
    }
    // stack entries: reference DFS (depth + 1), 4-wide tree (up to 3 pushes per level + 1).
    // The 4-wide node step (pt_walk.hpp t4_step) writes up to sp + 2 whatever it pushes: at
    // a node of level L the stack holds at most 3 (L - 1) entries, so its writes stay below
    // 3 t4depth entries - inside this bound.
    cam.stack_depth = std::max(b.out.bvh_depth, 3 * b.out.t4depth + 1) + 1;
    b.out.fast_ok = prims_inside_boxes(b.out.prims) && boxes_keep_their_extent(b.boxes, from);
    return std::move(b.out);
}

}  // namespace rt
