// The scene generators (src/scenes/scenes-*.ts) that produce the benchmark inputs: SceneData
// as JSON values, from mulberry32 with JS number semantics. No render path calls them.
#include "scene.hpp"

#include <algorithm>
#include <array>
#include <cmath>
#include <random>
#include <string>
#include <unordered_map>
#include <vector>

#include "scene_js.hpp"

namespace rt {

namespace {

// mulberry32 (src/scenes/scenes-utils.ts:8-23) with JS number semantics: the
// seed is a double that grows without wrapping; bit ops see ToInt32/ToUint32.
int32_t js_to_int32(double d) {
    if (!std::isfinite(d)) return 0;
    double t = std::trunc(d);
    double m = std::fmod(t, 4294967296.0);
    if (m < 0) m += 4294967296.0;
    return (int32_t)(uint32_t)m;
}
int32_t js_imul(int32_t a, int32_t b) { return (int32_t)((uint32_t)a * (uint32_t)b); }

}  // namespace

double SeededRandom::next() {
    seed += 1831565813.0;  // 0x6D2B79F5
    int32_t t = js_to_int32(seed);
    t = js_imul(t ^ (int32_t)((uint32_t)t >> 15), t | 1);
    double s = (double)t + (double)js_imul(t ^ (int32_t)((uint32_t)t >> 7), t | 61);
    t ^= js_to_int32(s);
    uint32_t r = (uint32_t)(t ^ (int32_t)((uint32_t)t >> 14));
    return (double)r / 4294967296.0;
}

namespace {

double opt_num(const Value* opts, const char* key, double dflt) {
    const Value* v = opts ? opts->get(key) : nullptr;
    return v ? to_number(v, dflt) : dflt;
}

std::vector<double> opt_vec3(const Value* opts, const char* key, std::vector<double> dflt) {
    const Value* v = opts ? opts->get(key) : nullptr;
    if (!v || !v->is_array()) return dflt;
    std::vector<double> out(3, NAN);
    for (size_t i = 0; i < 3 && i < v->arr.size(); ++i) out[i] = to_number(&v->arr[i], NAN);
    return out;
}

double default_seed() {
    // Math.floor(Math.random() * 2147483647): an unseeded scene, as in the reference.
    std::random_device rd;
    return std::floor(((double)rd() / 4294967296.0) * 2147483647.0);
}

Value material_entry(const std::string& id, Value material) {
    Value m = Value::object();
    m.set("id", Value::string(id));
    m.set("material", std::move(material));
    return m;
}

Value lambert(double r, double g, double b) {
    Value m = Value::object();
    m.set("type", Value::string("lambert"));
    m.set("color", rtj::vec3(r, g, b));
    return m;
}

Value camera_data(double vfov, double aperture, double focus, std::vector<double> from,
                  std::vector<double> at, std::vector<double> top, std::vector<double> bottom) {
    Value cam = Value::object();
    cam.set("vfov", Value::number(vfov));
    cam.set("aperture", Value::number(aperture));
    cam.set("focus", Value::number(focus));
    cam.set("from", rtj::vec3(from[0], from[1], from[2]));
    cam.set("at", rtj::vec3(at[0], at[1], at[2]));
    cam.set("up", rtj::vec3(0, 1, 0));
    Value bg = Value::object();
    bg.set("type", Value::string("gradient"));
    bg.set("top", rtj::vec3(top[0], top[1], top[2]));
    bg.set("bottom", rtj::vec3(bottom[0], bottom[1], bottom[2]));
    cam.set("background", std::move(bg));
    return cam;
}

Value metadata(const std::string& name, const std::string& desc) {
    Value md = Value::object();
    md.set("name", Value::string(name));
    md.set("description", Value::string(desc));
    md.set("version", Value::string("2.0"));
    return md;
}

// generateSpheresSceneData (src/scenes/scenes-spheres.ts:27-119). The overlap
// test (checkOverlap, 124-137) is the same predicate evaluated against a uniform
// grid of cell size 2r instead of the whole list, so large counts finish.
Value gen_spheres(const Value* opts) {
    const double count = opt_num(opts, "count", 10);
    const std::vector<double> centerPoint = opt_vec3(opts, "centerPoint", {0, 0, -2});
    const double distRadius = opt_num(opts, "radius", 1.25);
    const double minSphereRadius = opt_num(opts, "minSphereRadius", 0.1);
    const double maxSphereRadius = opt_num(opts, "maxSphereRadius", 0.2);
    const Value* seedv = opts ? opts->get("seed") : nullptr;
    const double seed = seedv ? to_number(seedv, 0) : default_seed();

    SeededRandom random(seed);
    const double scaleFactor = js_max<double>(minSphereRadius, 1 - std::log10(count + 1) / 4);
    const double adjustedMaxRadius = maxSphereRadius * scaleFactor;

    Value materials = Value::array();
    Value objects = Value::array();

    struct Placed { double c[3]; double r; };
    std::vector<Placed> placed;

    // Uniform grid over the placement ball for the overlap query.
    const double cell = std::max(2.0 * std::fabs(adjustedMaxRadius), 1e-9);
    const double lo[3] = {centerPoint[0] - distRadius - cell, centerPoint[1] - distRadius - cell,
                          centerPoint[2] - distRadius - cell};
    const double span = 2 * distRadius + 2 * cell;
    const bool use_grid = std::isfinite(span / cell) && span / cell < 1024 && count > 64;
    const int gdim = use_grid ? (int)std::ceil(span / cell) + 1 : 0;
    std::unordered_map<int64_t, std::vector<int>> grid;
    auto cell_of = [&](const double* c, int a) { return (int)std::floor((c[a] - lo[a]) / cell); };
    auto key_of = [&](int ix, int iy, int iz) { return ((int64_t)ix * gdim + iy) * gdim + iz; };

    auto overlaps = [&](const double* c, double radius) {
        auto test = [&](const Placed& s) {
            const double dx = c[0] - s.c[0], dy = c[1] - s.c[1], dz = c[2] - s.c[2];
            const double distance = std::sqrt(dx * dx + dy * dy + dz * dz);
            return distance < (radius + s.r);
        };
        if (!use_grid) {
            for (const Placed& s : placed) if (test(s)) return true;
            return false;
        }
        const int ix = cell_of(c, 0), iy = cell_of(c, 1), iz = cell_of(c, 2);
        for (int dx = -1; dx <= 1; ++dx)
            for (int dy = -1; dy <= 1; ++dy)
                for (int dz = -1; dz <= 1; ++dz) {
                    auto it = grid.find(key_of(ix + dx, iy + dy, iz + dz));
                    if (it == grid.end()) continue;
                    for (int k : it->second) if (test(placed[k])) return true;
                }
        return false;
    };

    double attempts = 0;
    const double maxAttempts = count * 100;
    double spheresCreated = 0;
    while (spheresCreated < count && attempts < maxAttempts) {
        attempts++;
        const double radius = adjustedMaxRadius;
        // randomPointInSphere (141-157): SeededRandom.randomInUnitSphere stores fp32.
        V3 p;
        while (true) {
            double x = -1 + 2 * random.next();
            double y = -1 + 2 * random.next();
            double z = -1 + 2 * random.next();
            p = mk<double>(x, y, z);
            if (len2<double>(p) < 1) break;
        }
        const double distanceFactor = std::pow(random.next(), 1.0 / 3.0) * distRadius;
        double c[3] = {centerPoint[0] + (double)p.x * distanceFactor,
                       centerPoint[1] + (double)p.y * distanceFactor,
                       centerPoint[2] + (double)p.z * distanceFactor};
        if (overlaps(c, radius)) continue;

        const std::string materialId = "sphere-" + num_str(spheresCreated);
        // generateRandomMaterialData (162-182)
        Value mat = Value::object();
        const double materialType = random.next();
        if (materialType < 0.6) {
            double r = random.next(), g = random.next(), b = random.next();
            mat = lambert(r, g, b);
        } else if (materialType < 0.9) {
            const double fuzz = random.next() * 0.5;
            double r = random.next(), g = random.next(), b = random.next();
            mat.set("type", Value::string("metal"));
            mat.set("color", rtj::vec3(r, g, b));
            mat.set("fuzz", Value::number(fuzz));
        } else {
            const double ior = 1.3 + random.next() * 1.2;
            mat.set("type", Value::string("glass"));
            mat.set("ior", Value::number(ior));
        }
        materials.push(material_entry(materialId, std::move(mat)));

        Value obj = Value::object();
        obj.set("type", Value::string("sphere"));
        obj.set("pos", rtj::vec3(c[0], c[1], c[2]));
        obj.set("r", Value::number(radius));
        obj.set("material", Value::string(materialId));
        objects.push(std::move(obj));

        placed.push_back(Placed{{c[0], c[1], c[2]}, radius});
        if (use_grid)
            grid[key_of(cell_of(c, 0), cell_of(c, 1), cell_of(c, 2))].push_back((int)placed.size() - 1);
        spheresCreated++;
    }

    Value scene = Value::object();
    scene.set("camera", camera_data(40, 0.0, 1.0, {0, 0, 2}, centerPoint, {0.5, 0.7, 1.0}, {1.0, 1.0, 1.0}));
    scene.set("materials", std::move(materials));
    scene.set("objects", std::move(objects));
    scene.set("metadata", metadata("Random Spheres", "Scene with " + num_str(spheresCreated) +
                                                         " randomly placed spheres (seed: " + num_str(seed) + ")"));
    return scene;
}

// generateRainSceneData (src/scenes/scenes-rain.ts:19-145)
Value gen_rain(const Value* opts) {
    const double count = opt_num(opts, "count", 50);
    const double sphereRadius = opt_num(opts, "sphereRadius", 0.05);
    const double width = opt_num(opts, "width", 4);
    const double height = opt_num(opts, "height", 3);
    const double depth = opt_num(opts, "depth", 2);
    const std::vector<double> centerPoint = opt_vec3(opts, "centerPoint", {0, 0, -2});
    const double metalFuzz = opt_num(opts, "metalFuzz", 0.1);
    const bool groundSphere = opts && opts->get("groundSphere") ? truthy(opts->get("groundSphere")) : true;
    const double groundY = opt_num(opts, "groundY", -100.5);
    const double groundRadius = opt_num(opts, "groundRadius", 100);
    const Value* seedv = opts ? opts->get("seed") : nullptr;
    const double seed = seedv ? to_number(seedv, 0) : default_seed();

    SeededRandom random(seed);
    Value materials = Value::array();
    Value objects = Value::array();
    if (groundSphere) materials.push(material_entry("ground", lambert(0.1, 0.1, 0.1)));
    if (groundSphere) {
        Value g = Value::object();
        g.set("type", Value::string("sphere"));
        g.set("pos", rtj::vec3(0, groundY, 0));
        g.set("r", Value::number(groundRadius));
        g.set("material", Value::string("ground"));
        objects.push(std::move(g));
    }
    const double spd = std::ceil(std::pow(count, 1.0 / 3.0));
    const double xSpacing = width / spd, ySpacing = height / spd, zSpacing = depth / spd;
    const double totalW = spd * xSpacing, totalH = spd * ySpacing, totalD = spd * zSpacing;
    const double startX = centerPoint[0] - totalW / 2 + xSpacing / 2;
    const double startY = centerPoint[1] - totalH / 2 + ySpacing / 2;
    const double startZ = centerPoint[2] - totalD / 2 + zSpacing / 2;

    std::vector<std::array<double, 3>> positions;
    const long n = spd > 0 && std::isfinite(spd) ? (long)spd : 0;
    for (long x = 0; x < n; x++)
        for (long y = 0; y < n; y++)
            for (long z = 0; z < n; z++) {
                double px = startX + x * xSpacing + (random.next() - 0.5) * xSpacing * 0.3;
                double py = startY + y * ySpacing + (random.next() - 0.5) * ySpacing * 0.3;
                double pz = startZ + z * zSpacing + (random.next() - 0.5) * zSpacing * 0.3;
                positions.push_back({px, py, pz});
            }
    // shuffleArray: Fisher-Yates (152-158)
    for (long i = (long)positions.size() - 1; i > 0; i--) {
        long j = (long)std::floor(random.next() * (double)(i + 1));
        std::swap(positions[i], positions[j]);
    }
    const long take = std::min<long>((long)positions.size(), count > 0 ? (long)std::ceil(count) : 0);
    for (long i = 0; i < take; i++) {
        const auto& pos = positions[i];
        const double brightness = 0.7 + random.next() * 0.3;
        const double fuzz = metalFuzz * random.next();
        const std::string materialId = "rain-" + std::to_string(i);
        Value mat = Value::object();
        mat.set("type", Value::string("metal"));
        mat.set("color", rtj::vec3(brightness, brightness, brightness));
        mat.set("fuzz", Value::number(fuzz));
        materials.push(material_entry(materialId, std::move(mat)));
        Value obj = Value::object();
        obj.set("type", Value::string("sphere"));
        obj.set("pos", rtj::vec3(pos[0], pos[1], pos[2]));
        obj.set("r", Value::number(sphereRadius));
        obj.set("material", Value::string(materialId));
        objects.push(std::move(obj));
    }
    Value scene = Value::object();
    scene.set("camera", camera_data(40, 0.0, 1.0, {0, 0, 2}, centerPoint, {0.5, 0.7, 1.0}, {1.0, 1.0, 1.0}));
    scene.set("materials", std::move(materials));
    scene.set("objects", std::move(objects));
    scene.set("metadata", metadata("Rain Scene", "Scene with " + std::to_string(take) +
                                                     " metallic rain spheres (seed: " + num_str(seed) + ")"));
    return scene;
}

Value quad_obj(std::vector<double> pos, std::vector<double> u, std::vector<double> v, const char* mat) {
    Value o = Value::object();
    o.set("type", Value::string("quad"));
    o.set("pos", rtj::vec3(pos[0], pos[1], pos[2]));
    o.set("u", rtj::vec3(u[0], u[1], u[2]));
    o.set("v", rtj::vec3(v[0], v[1], v[2]));
    o.set("material", Value::string(mat));
    return o;
}

Value sphere_obj(std::vector<double> pos, double r, const char* mat) {
    Value o = Value::object();
    o.set("type", Value::string("sphere"));
    o.set("pos", rtj::vec3(pos[0], pos[1], pos[2]));
    o.set("r", Value::number(r));
    o.set("material", Value::string(mat));
    return o;
}

// generateCornellSceneData (src/scenes/scenes-cornell.ts:19-134)
Value gen_cornell(const Value* opts) {
    const Value* vv = opts ? opts->get("variant") : nullptr;
    const std::string variant = (vv && vv->is_string()) ? vv->str : "spheres";
    const bool spheres = variant == "spheres";
    const double boxSize = 2.0, halfSize = boxSize / 2;
    Value materials = Value::array();
    materials.push(material_entry("red", lambert(0.65, 0.05, 0.05)));
    materials.push(material_entry("green", lambert(0.12, 0.45, 0.15)));
    materials.push(material_entry("white", lambert(0.73, 0.73, 0.73)));
    {
        Value l = Value::object();
        l.set("type", Value::string("light"));
        l.set("emit", rtj::vec3(15, 15, 15));
        materials.push(material_entry("light", std::move(l)));
    }
    if (spheres) {
        materials.push(material_entry("sphere-white", lambert(0.6, 0.6, 0.6)));
        Value g = Value::object();
        g.set("type", Value::string("glass"));
        g.set("ior", Value::number(1.5));
        materials.push(material_entry("sphere-glass", std::move(g)));
    }
    Value objects = Value::array();
    const double h = halfSize;
    objects.push(quad_obj({-h, -h, -h}, {0, boxSize, 0}, {0, 0, boxSize}, "red"));
    objects.push(quad_obj({h, -h, h}, {0, boxSize, 0}, {0, 0, -boxSize}, "green"));
    objects.push(quad_obj({-h, -h, -h}, {boxSize, 0, 0}, {0, boxSize, 0}, "white"));
    objects.push(quad_obj({-h, -h, -h}, {boxSize, 0, 0}, {0, 0, boxSize}, "white"));
    objects.push(quad_obj({-h, h, h}, {boxSize, 0, 0}, {0, 0, -boxSize}, "white"));
    const double lightSize = boxSize * 0.3;
    {
        Value l = quad_obj({-lightSize / 2, halfSize - 0.01, -lightSize / 2}, {lightSize, 0, 0},
                           {0, 0, lightSize}, "light");
        l.set("light", Value::boolean(true));
        objects.push(std::move(l));
    }
    if (spheres) {
        const double sphereRadius = 0.3;
        objects.push(sphere_obj({-halfSize * 0.4, -halfSize + sphereRadius, -halfSize * 0.3}, sphereRadius,
                                "sphere-white"));
        objects.push(sphere_obj({halfSize * 0.4, -halfSize + sphereRadius, halfSize * 0.3}, sphereRadius,
                                "sphere-glass"));
    }
    Value scene = Value::object();
    scene.set("camera", camera_data(40, 0.0, 1.0, {0, 0, halfSize * 4}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}));
    Value render = Value::object();
    render.set("aspect", Value::number(1.0));
    render.set("roulette", Value::boolean(true));
    render.set("rouletteDepth", Value::number(5));
    scene.set("render", std::move(render));
    scene.set("materials", std::move(materials));
    scene.set("objects", std::move(objects));
    scene.set("metadata",
              metadata("Cornell Box (" + variant + ")",
                       std::string("Cornell box scene with ") + (spheres ? "two spheres inside" : "empty interior")));
    return scene;
}

// generateDefaultSceneData (src/scenes/scenes-default.ts:8-82)
Value gen_default() {
    Value materials = Value::array();
    materials.push(material_entry("ground", lambert(0.4, 0.4, 0.0)));
    materials.push(material_entry("blue", lambert(0.1, 0.1, 0.9)));
    {
        Value g = Value::object();
        g.set("type", Value::string("glass"));
        g.set("ior", Value::number(1.5));
        materials.push(material_entry("glass", std::move(g)));
    }
    auto metal = [](double r, double g, double b, double fuzz) {
        Value m = Value::object();
        m.set("type", Value::string("metal"));
        m.set("color", rtj::vec3(r, g, b));
        m.set("fuzz", Value::number(fuzz));
        return m;
    };
    materials.push(material_entry("silver", metal(0.8, 0.8, 0.8, 0.0)));
    materials.push(material_entry("gold", metal(0.8, 0.6, 0.2, 0.5)));
    {
        Value lay = Value::object();
        lay.set("type", Value::string("layered"));
        Value outer = Value::object();
        outer.set("type", Value::string("glass"));
        outer.set("ior", Value::number(1.5));
        lay.set("outer", std::move(outer));
        lay.set("inner", lambert(0.7, 0.3, 0.3));
        materials.push(material_entry("layered-paint", std::move(lay)));
    }
    {
        Value l = Value::object();
        l.set("type", Value::string("light"));
        l.set("emit", rtj::vec3(15.0, 14.0, 13.0));
        materials.push(material_entry("sun-light", std::move(l)));
    }
    Value objects = Value::array();
    {
        Value p = Value::object();
        p.set("type", Value::string("plane"));
        p.set("pos", rtj::vec3(0, 0, 0));
        p.set("u", rtj::vec3(1, 0, 0));
        p.set("v", rtj::vec3(0, 0, 1));
        p.set("material", Value::string("ground"));
        objects.push(std::move(p));
    }
    objects.push(sphere_obj({0, 0.5, -1}, 0.5, "layered-paint"));
    objects.push(sphere_obj({-1, 0.5, -1}, 0.5, "silver"));
    objects.push(sphere_obj({1, 0.5, -1}, 0.5, "gold"));
    objects.push(sphere_obj({0.5, 0.25, -0.5}, 0.25, "glass"));
    objects.push(sphere_obj({-0.5, 0.25, -0.5}, 0.25, "glass"));
    objects.push(sphere_obj({-0.5, 0.25, -0.5}, -.24, "glass"));
    objects.push(sphere_obj({-0.5, 0.25, -0.5}, 0.20, "blue"));
    {
        Value l = quad_obj({-2, 3, 0}, {1, 0, 0}, {0, -0.707, -0.707}, "sun-light");
        l.set("light", Value::boolean(true));
        objects.push(std::move(l));
    }
    {
        Value s = sphere_obj({30, 30.5, 15}, 10, "sun-light");
        s.set("light", Value::boolean(true));
        objects.push(std::move(s));
    }
    Value scene = Value::object();
    scene.set("camera", camera_data(40, 0.05, 2.8, {0, 0.75, 2}, {0, 0.5, -1}, {1, 1, 1}, {0.5, 0.7, 1.0}));
    scene.set("materials", std::move(materials));
    scene.set("objects", std::move(objects));
    scene.set("metadata", metadata("Default Scene",
                                   "A scene with various spheres demonstrating different materials including "
                                   "layered, mixed, and basic materials"));
    return scene;
}

}  // namespace

Value generate_scene_data(const std::string& type, const Value* options) {
    // generateSceneData (src/scenes/scenes.ts:42-50)
    if (type == "default") return gen_default();
    if (type == "spheres") return gen_spheres(options);
    if (type == "rain") return gen_rain(options);
    if (type == "cornell") return gen_cornell(options);
    fail("Unknown scene type: " + type);
}

}  // namespace rt
