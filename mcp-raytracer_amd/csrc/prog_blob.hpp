// Progressive sessions: the checkpoint blob's format, its parser and the scene fingerprint.
// [ProgBlobHeader][ProgPix x slots], little-endian as the host writes it. The header's checksum
// covers the header up to that field, the payload's the state bytes (FNV-1a, 64 bit).
// Plain C++ (no device): bytes in, header out.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/rt_amd.h"
#include "scene.hpp"

namespace rt {

// = sizeof(ProgPix) (progressive.hpp), kTile and kWave (pt_types.hpp); dev_ctx.cpp asserts them
constexpr size_t kProgPixBytes = 48;
constexpr int kProgTile = 8, kProgWave = 64;

uint64_t fnv1a(const void* data, size_t n, uint64_t h = 1469598103934665603ull);

extern const char kProgMagic[8];
constexpr uint32_t kProgBlobVersion = 1;
struct ProgBlobHeader {
    char magic[8];
    uint32_t version, header_bytes;
    char build_id[24];
    int32_t width, height;
    int32_t rx, ry, rw, rh;
    int32_t precision;
    uint32_t seed;
    double samples;        // RenderOptions.samples
    int32_t samples_loop;  // its loop count
    int32_t samples_done;
    int32_t steps;
    int32_t reserved;
    int64_t active_pixels;
    uint64_t err_flags;    // ERR_* of the samples kept so far
    uint64_t fingerprint;  // flattened scene + resolved camera options
    uint64_t payload_bytes, payload_checksum;
    uint64_t header_checksum;
};
static_assert(sizeof(ProgBlobHeader) == 144 && offsetof(ProgBlobHeader, header_checksum) == 136, "blob header layout");

// Fingerprint of what a session's samples depend on: the flattened scene (nodes, primitives,
// materials, lights) and every resolved camera / render option, field by field (no padding).
uint64_t prog_fingerprint(const SceneBuild& b);

// Validates a blob (length, magic, version, checksums) and returns its header; the state
// follows at blob + sizeof(ProgBlobHeader). Throws std::invalid_argument.
ProgBlobHeader prog_parse_blob(const uint8_t* blob, size_t len);

void prog_info_from_header(const ProgBlobHeader& h, rt_progressive_info* info);

}  // namespace rt
