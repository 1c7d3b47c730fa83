// The fast-traversal tree of a scene (pt_walk.hpp closest_hit_fast): padded boxes, binned SAH,
// the collapse to 4-wide nodes and the leaf-order sphere records. Nothing of the reference's
// object model: the input is the reference's box per primitive slot. Host only.
#pragma once

#include <vector>

#include "rt_math.hpp"
#include "scene.hpp"

namespace rt {

struct Box {
    V3 mn, mx;
};

inline float comp(V3 v, int a) { return a == 0 ? v.x : (a == 1 ? v.y : v.z); }

// Builds out's fast-traversal tree from out.nodes / out.prims / out.bvh_depth and the
// primitives' reference boxes in slot order: binned SAH where every box is finite, there are
// more than 16 primitives and RT_AMD_SAH is not 0, else the reference tree itself. Sets tprims
// (padded to a multiple of 4), tsph, tsph2, t4nodes, t4root, t4depth and t4root_box.
void build_fast_tree(SceneBuild& out, const std::vector<Box>& slot_box);

// SceneBuild::fast_ok: every primitive lies inside the box the reference gives it.
bool prims_inside_boxes(const std::vector<RtPrim>& prims);

// SceneBuild::fast_ok, second condition: the reference's slab test can tell the two faces of
// every finite box extent apart from any ray origin inside the scene (camera centre included).
bool boxes_keep_their_extent(const std::vector<Box>& boxes, V3 center);

}  // namespace rt
