// The progressive checkpoint blob (prog_blob.hpp).
#include "prog_blob.hpp"

#include <cstring>
#include <stdexcept>
#include <string>

namespace rt {

uint64_t fnv1a(const void* data, size_t n, uint64_t h) {
    const unsigned char* p = static_cast<const unsigned char*>(data);
    for (size_t k = 0; k < n; ++k) h = (h ^ p[k]) * 1099511628211ull;
    return h;
}

const char kProgMagic[8] = {'R', 'T', 'P', 'R', 'O', 'G', 0x1a, '\n'};

uint64_t prog_fingerprint(const SceneBuild& b) {
    uint64_t f = fnv1a(b.nodes.data(), b.nodes.size() * sizeof(RtNode));
    f = fnv1a(b.prims.data(), b.prims.size() * sizeof(RtPrim), f);
    f = fnv1a(b.mats.data(), b.mats.size() * sizeof(RtMat), f);
    f = fnv1a(b.lights.data(), b.lights.size() * sizeof(RtLight), f);
    const RtCamera& C = b.cam;
    auto add = [&](const auto& v) { f = fnv1a(&v, sizeof v, f); };
    add(C.pixel00); add(C.du); add(C.dv); add(C.center); add(C.ddu); add(C.ddv); add(C.bg_top); add(C.bg_bottom);
    add(C.aperture); add(C.samples); add(C.a_tolerance); add(C.a_batch); add(C.depth_raw);
    add(C.width); add(C.height); add(C.n_samples); add(C.depth); add(C.roulette); add(C.roulette_depth);
    add(C.mode); add(C.adaptive); add(C.n_lights); add(C.has_background); add(C.emissive_scatter);
    add(C.n_nodes); add(C.n_prims); add(C.n_mats); add(C.seed);
    return f;
}

ProgBlobHeader prog_parse_blob(const uint8_t* blob, size_t len) {
    if (!blob || len == 0) throw std::invalid_argument("progressive blob: empty");
    if (len < sizeof(ProgBlobHeader))
        throw std::invalid_argument("progressive blob: truncated, " + std::to_string(len) + " bytes are less than the " +
                                    std::to_string(sizeof(ProgBlobHeader)) + "-byte header");
    ProgBlobHeader h;
    std::memcpy(&h, blob, sizeof h);
    if (std::memcmp(h.magic, kProgMagic, sizeof kProgMagic) != 0)
        throw std::invalid_argument("progressive blob: bad magic (not a progressive checkpoint)");
    if (h.version != kProgBlobVersion || h.header_bytes != sizeof(ProgBlobHeader))
        throw std::invalid_argument("progressive blob: format version " + std::to_string(h.version) + " is not " +
                                    std::to_string(kProgBlobVersion));
    if (fnv1a(&h, offsetof(ProgBlobHeader, header_checksum)) != h.header_checksum)
        throw std::invalid_argument("progressive blob: corrupt header (checksum mismatch)");
    // (in long: rw + 7 overflows an int for a header that claims a region 2^31 - 1 wide)
    const long slots = h.rw > 0 && h.rh > 0
                           ? (((long)h.rw + kProgTile - 1) / kProgTile) * (((long)h.rh + kProgTile - 1) / kProgTile) * kProgWave
                           : 0;
    if (slots <= 0 || h.payload_bytes != (uint64_t)slots * kProgPixBytes)
        throw std::invalid_argument("progressive blob: corrupt header (payload length does not fit the region)");
    if (len < sizeof(ProgBlobHeader) + h.payload_bytes)
        throw std::invalid_argument("progressive blob: truncated, " + std::to_string(len) + " of " +
                                    std::to_string(sizeof(ProgBlobHeader) + h.payload_bytes) + " bytes");
    if (len > sizeof(ProgBlobHeader) + h.payload_bytes)
        throw std::invalid_argument("progressive blob: corrupt (bytes after the payload)");
    if (fnv1a(blob + sizeof(ProgBlobHeader), (size_t)h.payload_bytes) != h.payload_checksum)
        throw std::invalid_argument("progressive blob: corrupt payload (checksum mismatch)");
    return h;
}

void prog_info_from_header(const ProgBlobHeader& h, rt_progressive_info* info) {
    *info = rt_progressive_info{};
    info->region = rt_region{h.rx, h.ry, h.rw, h.rh};
    info->width = h.width;
    info->height = h.height;
    info->samples_done = h.samples_done;
    info->samples = h.samples_loop;
    info->steps = h.steps;
    info->done = h.active_pixels == 0 || h.samples_done >= h.samples_loop;
    info->precision = h.precision;
    info->seed = h.seed;
    info->active_pixels = h.active_pixels;
    info->state_bytes = h.payload_bytes;
    std::memcpy(info->build_id, h.build_id, sizeof info->build_id);
    info->build_id[sizeof info->build_id - 1] = 0;
}

}  // namespace rt
