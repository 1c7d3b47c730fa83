// Host-side helpers shared by the units of the C ABI: environment switches, the HIP error
// type, device selection, the region clamp and the owner of a device allocation.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <stdexcept>
#include <string>

#include "../../include/rt_amd.h"

namespace rt {

// A/B switches for measurements: RT_AMD_LDS_SCENE=0 (no LDS-resident scene),
// RT_AMD_CHUNKED=0 (sequential-pixel kernel for fixed-spp renders). Read where they are used,
// never cached: a process may change them between renders.
inline bool env_flag(const char* name, bool dflt) {
    const char* e = std::getenv(name);
    if (!e || !e[0]) return dflt;
    return e[0] != '0';
}
inline bool lds_scene_enabled() { return env_flag("RT_AMD_LDS_SCENE", true); }
inline int env_int(const char* name, int dflt) {
    const char* e = std::getenv(name);
    return (e && e[0]) ? std::max(1, std::atoi(e)) : dflt;
}
// the same without the clamp to >= 1 (switches and counts where 0 means off)
inline int env_int0(const char* name, int dflt) {
    const char* e = std::getenv(name);
    return (e && e[0]) ? std::atoi(e) : dflt;
}

struct HipError : std::runtime_error {
    using std::runtime_error::runtime_error;
};

inline void hip_check(hipError_t e, const char* what) {
    if (e != hipSuccess) throw HipError(std::string(what) + ": " + hipGetErrorString(e));
}

inline int device_cus(int dev) {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    return cus;
}

// The current HIP device of the calling thread, restored when the scope ends.
struct DeviceScope {
    int prev = 0;
    DeviceScope() { (void)hipGetDevice(&prev); }
    ~DeviceScope() { (void)hipSetDevice(prev); }
};

// `r` clamped to a width x height image: width or height 0 when nothing of it is inside (each
// caller decides what an empty region means).
inline rt_region clamp_region(const rt_region& r, int width, int height) {
    const long x0 = std::max(r.x, 0), y0 = std::max(r.y, 0);
    const long x1 = std::min<long>((long)r.x + r.width, width), y1 = std::min<long>((long)r.y + r.height, height);
    return rt_region{(int32_t)x0, (int32_t)y0, (int32_t)std::max(x1 - x0, 0l), (int32_t)std::max(y1 - y0, 0l)};
}
inline bool region_empty(const rt_region& r) { return r.width <= 0 || r.height <= 0; }

// Move-only owner of one hipMalloc allocation of `cap` elements. The caller has made the
// buffer's device current whenever it allocates or frees.
template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            reset();
            std::swap(p, o.p);
            std::swap(cap, o.cap);
        }
        return *this;
    }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { reset(); }
    void reset() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    // at least n elements (and 16 bytes): grown on demand, the old allocation freed first
    void ensure(size_t n, const char* what) {
        if (p && n <= cap) return;
        reset();
        hip_check(hipMalloc(&p, std::max<size_t>(n * sizeof(T), 16)), what);
        cap = n;
    }
    operator T*() const { return p; }
};

}  // namespace rt
