// The scene blob: every array of a SceneBuild the kernels read, in one allocation. Built on the
// host (plain C++, no device), uploaded once per device context (dev_ctx.cpp).
//
//   [t4nodes][tprims][tsph][prims][xrec] | [mats][lights][onbs] | [nodes][pre][tsph2]
//
// The first group (lds_words 16-byte words) is the LDS-resident prefix of level 1, the first
// two (lds_words2) of level 2. Every section is a multiple of 16 bytes.
#pragma once

#include <cstdint>
#include <vector>

#include "scene.hpp"

namespace rt {

// = pt_types.hpp kBruteMaxPrims (launch_plan.cpp asserts it): larger scenes carry no exact /
// pre-filter records, only closest_hit_brute_nf reads them
constexpr int kBlobBruteMaxPrims = 16;

struct SceneBlob {
    std::vector<char> bytes;  // (a device context drops them after the upload)
    size_t size = 0;          // their count
    int32_t lds_words = 0;    // [t4nodes][tprims][tsph][prims][xrec] prefix, 16-byte words
    int32_t lds_words2 = 0;   // the same + [mats][lights][onbs]
    int32_t off_prims = 0, off_mats = 0, off_lights = 0, off_nodes = 0, off_tprims = 0, off_tsph = 0, off_onbs = 0;
    int32_t off_tsph2 = -1;  // leaf-order sphere records with the fp64 radius (RtLeafSph), or -1
    int32_t off_pre = 0, n_pre = 0, off_xrec = 0;
    int32_t n_onb = 0;
};

SceneBlob build_scene_blob(const SceneBuild& build);

}  // namespace rt
