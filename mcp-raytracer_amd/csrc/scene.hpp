// Host build of the flattened, device-resident form of the reference's Camera + world.
//
// The reference builds an object graph per render (createCameraFromSceneData,
// src/scenes/scenes.ts:60-104): Sphere/Plane/Quad objects (src/entities/*),
// Material objects (src/materials/*), a recursive BVHNode tree
// (src/geometry/bvh.ts:34-102) and a Camera (src/camera.ts:107-166). Here the
// same data is laid out as the flat arrays of scene_types.hpp that one HIP kernel reads.
// Host units only: device units include scene_types.hpp.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "json.hpp"
#include "rt_math.hpp"
#include "scene_types.hpp"

namespace rt {

// Host-side build product. Owned by rt_camera; uploaded to the device lazily.
struct SceneBuild {
    std::vector<RtNode> nodes;
    std::vector<RtT4Node> t4nodes; // fast-traversal tree, 4-wide (SAH, or the reference tree; scene_tree.cpp)
    int32_t t4root = 0;          // its root reference (node index or leaf code)
    int t4depth = 0;             // its depth in 4-wide nodes
    RtNode t4root_box{};         // its root box (padded)
    std::vector<int32_t> tprims; // its leaves' primitive slots (padded to a multiple of 4)
    std::vector<float> tsph;     // per tprims entry: sphere {centre, fp32 radius}, NaNs for other types
    std::vector<RtLeafSph> tsph2; // per tprims entry: the same + fp64 radius + slot (trees walked from global memory)
    std::vector<RtPrim> prims;
    std::vector<RtMat> mats;
    std::vector<RtLight> lights;
    RtCamera cam{};
    int bvh_depth = 0;
    // Every primitive lies inside its own reference box (no negative / NaN
    // sphere radius, no slightly tilted plane given a thin axis box), so a
    // conservative culling test returns the reference's hit: fast traversal OK.
    // And every finite box keeps its extent when seen from anywhere in the scene
    // (scene_tree.cpp boxes_keep_their_extent).
    bool fast_ok = true;
    std::vector<int32_t> prim_object;  // prim slot -> index in SceneData.objects
};

// createCameraFromSceneData(sceneData, renderOptions) restated
// (src/scenes/scenes.ts:60-104). Throws std::runtime_error with the reference's
// error message where the reference throws.
SceneBuild build_scene(const rtj::Value& scene_data, const rtj::Value* render_options);

// Scene generators (src/scenes/scenes-*.ts). `type` in {default, spheres, rain,
// cornell}; options as the reference's *SceneOptions object (may be null).
rtj::Value generate_scene_data(const std::string& type, const rtj::Value* options);

// Math.hypot as implemented by V8 (Kahan-summed, max-normalised).
double v8_hypot3(double x, double y, double z);

// mulberry32 SeededRandom.next() with JS double seed arithmetic
// (src/scenes/scenes-utils.ts:8-23).
struct SeededRandom {
    double seed;
    explicit SeededRandom(double s) : seed(s) {}
    double next();
};

}  // namespace rt
