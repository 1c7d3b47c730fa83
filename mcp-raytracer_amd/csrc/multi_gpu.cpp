// Single-process multi-GPU render (rt_camera_render_multi): the region's split, the RCCL
// loader and the gather (declared in dev_ctx.hpp).
#include <dlfcn.h>
#include <rccl/rccl.h>  // types and declarations only: librccl is dlopen'ed (Rccl below)

#include <algorithm>
#include <cstdlib>
#include <exception>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "dev_ctx.hpp"

namespace rt {

// RenderStats.merge (src/render-utils/renderStats.ts:42-64) over the stats words of n
// renders (row r at words + r * ST_WORDS): totals summed, minima / maxima over the renders
// (~0 = no sample: skipped by the unsigned minimum), error flags or'ed.
static void merge_stats_words(const unsigned long long* words, int n, unsigned long long* m) {
    m[ST_PIXELS] = m[ST_SAMPLES] = m[ST_BOUNCES] = m[ST_SMAX] = m[ST_BMAX] = m[ST_ERROR] = 0;
    m[ST_SMIN] = m[ST_BMIN] = ~0ull;
    for (int r = 0; r < n; ++r) {
        const unsigned long long* w = words + (size_t)r * ST_WORDS;
        m[ST_PIXELS] += w[ST_PIXELS];
        m[ST_SAMPLES] += w[ST_SAMPLES];
        m[ST_BOUNCES] += w[ST_BOUNCES];
        m[ST_SMIN] = std::min(m[ST_SMIN], w[ST_SMIN]);
        m[ST_BMIN] = std::min(m[ST_BMIN], w[ST_BMIN]);
        m[ST_SMAX] = std::max(m[ST_SMAX], w[ST_SMAX]);
        m[ST_BMAX] = std::max(m[ST_BMAX], w[ST_BMAX]);
        m[ST_ERROR] |= w[ST_ERROR];
    }
}

rt_multi_plan make_multi_plan(const rt_region& region, int width, int height, int n) {
    rt_multi_plan p{};
    p.region = clamp_region(region, width, height);
    p.n_devices = n;
    p.tiles = (int64_t)((p.region.width + kTile - 1) / kTile) * ((p.region.height + kTile - 1) / kTile);
    p.slab_tiles = (int32_t)((p.tiles + n - 1) / n);
    p.slab_bytes_rgb = (int64_t)(p.slab_tiles + 1) * kWave * 3;
    p.slab_bytes_radiance = (int64_t)p.slab_tiles * kWave * 3 * (int64_t)sizeof(float);
    p.stats_offset = (int64_t)p.slab_tiles * kWave * 3;
    for (int g = 0; g < n && g < RT_MAX_DEVICES; ++g)
        p.group_tiles[g] = (int32_t)(p.tiles > g ? (p.tiles - g + n - 1) / n : 0);
    return p;
}

// RCCL, loaded at the first multi-GPU gather (dlopen: a process that already holds PyTorch's
// librccl.so.1 shares it; a Node host loads ROCm's). Single-process communicators over the
// listed devices (ncclCommInitAll), cached per device list for the life of the process.
struct Rccl {
    decltype(&ncclCommInitAll) comm_init_all = nullptr;
    decltype(&ncclGroupStart) group_start = nullptr;
    decltype(&ncclGroupEnd) group_end = nullptr;
    decltype(&ncclSend) send = nullptr;
    decltype(&ncclRecv) recv = nullptr;
    decltype(&ncclGetErrorString) error_string = nullptr;
    std::mutex mu;  // one gather at a time per process (a communicator is not re-entrant)
    std::vector<std::pair<std::vector<int>, std::vector<ncclComm_t>>> comms;

    void check(ncclResult_t r, const char* what) {
        if (r != ncclSuccess) throw HipError(std::string(what) + ": " + (error_string ? error_string(r) : "RCCL error"));
    }
    const std::vector<ncclComm_t>& comms_for(const std::vector<int>& devs) {
        for (auto& c : comms)
            if (c.first == devs) return c.second;
        std::vector<ncclComm_t> cs(devs.size(), nullptr);
        check(comm_init_all(cs.data(), (int)devs.size(), devs.data()), "ncclCommInitAll");
        comms.emplace_back(devs, std::move(cs));
        return comms.back().second;
    }
};

static Rccl& rccl() {
    static std::mutex load_mu;
    static Rccl* lib = nullptr;
    static std::string load_error;
    std::lock_guard<std::mutex> lock(load_mu);
    if (lib) return *lib;
    if (!load_error.empty()) throw HipError(load_error);
    const char* env = std::getenv("RT_AMD_RCCL_LIB");
    void* h = nullptr;
    for (const char* name : {env && env[0] ? env : "librccl.so.1", "librccl.so"})
        if ((h = dlopen(name, RTLD_NOW | RTLD_LOCAL))) break;
    if (!h) {
        load_error = std::string("RCCL not loadable (librccl.so.1): ") + dlerror() +
                     " - set RT_AMD_GATHER=peer for device-to-device copies";
        throw HipError(load_error);
    }
    auto* r = new Rccl();
    auto sym = [&](auto& fn, const char* name) {
        fn = reinterpret_cast<std::remove_reference_t<decltype(fn)>>(dlsym(h, name));
        if (!fn) load_error = std::string("RCCL symbol missing: ") + name;
    };
    sym(r->comm_init_all, "ncclCommInitAll");
    sym(r->group_start, "ncclGroupStart");
    sym(r->group_end, "ncclGroupEnd");
    sym(r->send, "ncclSend");
    sym(r->recv, "ncclRecv");
    sym(r->error_string, "ncclGetErrorString");
    if (!load_error.empty()) {
        delete r;
        throw HipError(load_error);
    }
    lib = r;
    return *lib;
}

// Entry g of `devs` renders tile
// group g of n into its context's tile-packed slab on its own stream (one host thread per entry,
// so renders that wait on the host between rounds - adaptive sampling - still overlap); the
// slabs are gathered on devs[0] (RCCL send / recv in one group over xGMI, or device-to-device
// copies), unpacked into devs[0]'s full frame (rt_tiles_unpack) and the stats words merged as
// RenderStats.merge does (the reference's workers: src/raytracer.ts:60-90, 185-205;
// src/render-utils/renderWorker.ts:17-35).
DevCtx& render_multi(rt_camera* cam, const int32_t* devices, int n, const rt_region& region, bool want_rgb,
                     bool want_rad, unsigned long long* merged, const std::function<void(DevCtx&)>& outputs) {
    int count = 0;
    hip_check(hipGetDeviceCount(&count), "hipGetDeviceCount");
    if (n < 1 || n > RT_MAX_DEVICES || !devices)
        throw std::invalid_argument("rt_camera_render_multi: 1 <= n_devices <= RT_MAX_DEVICES devices are required");
    std::vector<int> devs(devices, devices + n);
    bool distinct = true;
    for (int g = 0; g < n; ++g) {
        if (devs[g] < 0 || devs[g] >= count)
            throw std::invalid_argument("rt_camera_render_multi: device " + std::to_string(devs[g]) + " is not visible (" +
                                        std::to_string(count) + " devices)");
        for (int h = 0; h < g; ++h) distinct = distinct && devs[h] != devs[g];
    }
    // transport: RCCL over xGMI when every entry is its own device, else device-to-device
    // copies (a device listed twice: the split rehearsed on fewer GPUs; RCCL refuses that)
    const char* ge = std::getenv("RT_AMD_GATHER");
    const std::string gs = ge ? ge : "";
    int transport = distinct ? RT_GATHER_RCCL : RT_GATHER_PEER;
    if (gs == "peer") transport = RT_GATHER_PEER;
    else if (gs == "rccl") transport = RT_GATHER_RCCL;
    else if (!gs.empty()) throw std::invalid_argument("RT_AMD_GATHER must be 'rccl' or 'peer'");
    if (transport == RT_GATHER_RCCL && !distinct)
        throw std::invalid_argument("rt_camera_render_multi: RCCL needs distinct devices (RT_AMD_GATHER=peer allows repeats)");

    const RtCamera& C = cam->build.cam;
    const rt_multi_plan plan = make_multi_plan(region, C.width, C.height, n);
    std::vector<DevCtx*> cs(n);
    for (int g = 0; g < n; ++g) {
        int inst = 0;
        for (int h = 0; h < g; ++h) inst += devs[h] == devs[g];
        cs[g] = &cam->ctx(devs[g], inst);
    }
    cam->multi = cs;
    cam->multi_transport = transport;
    cam->multi_plan = plan;
    const size_t slab_b = (size_t)plan.slab_bytes_rgb, rslab_b = want_rad ? (size_t)plan.slab_bytes_radiance : 0;
    DeviceScope scope;

    // renders: one host thread per further entry, entry 0 on the calling thread
    std::vector<std::exception_ptr> errs(n);
    auto work = [&](int g) {
        try {
            DevCtx& c = *cs[g];
            hip_check(hipSetDevice(c.device), "hipSetDevice");
            c.ensure_device();
            c.ensure_multi(slab_b, rslab_b, g == 0, n);
            if (g == 0) c.ensure_frame();
            c.order_after(c.stream);  // (the call ends with a host sync of the root's stream)
            c.launch(plan.region, g, n, cam->precision, cam->traversal, 0, c.d_slab, want_rad ? c.d_rslab.p : nullptr,
                     nullptr, nullptr, 1, c.stream);
            // the stats words into the slab's spare tile (rides in the gather)
            hip_check(hipMemcpy2DAsync(c.d_slab + plan.stats_offset, sizeof(unsigned long long), c.d_stats,
                                       kStatStride * sizeof(unsigned long long), sizeof(unsigned long long), ST_WORDS,
                                       hipMemcpyDeviceToDevice, c.stream),
                      "hipMemcpy2DAsync(stats)");
            hip_check(hipEventRecord(c.ev_rendered, c.stream), "hipEventRecord");
        } catch (...) {
            errs[g] = std::current_exception();
        }
    };
    std::vector<std::thread> th;
    for (int g = 1; g < n; ++g) th.emplace_back(work, g);
    work(0);
    for (auto& t : th) t.join();
    for (auto& e : errs)
        if (e) std::rethrow_exception(e);

    DevCtx& root = *cs[0];
    hip_check(hipSetDevice(root.device), "hipSetDevice");
    hip_check(hipEventRecord(root.ev_gather0, root.stream), "hipEventRecord");
    if (transport == RT_GATHER_RCCL) {
        Rccl& r = rccl();
        std::lock_guard<std::mutex> lock(r.mu);
        const std::vector<ncclComm_t>& comms = r.comms_for(devs);
        // one group: entry g sends its slab(s) to rank 0, rank 0 receives slab g into row g
        // (rank 0's own slab included: a send / recv pair to itself)
        r.check(r.group_start(), "ncclGroupStart");
        for (int g = 0; g < n; ++g) {
            r.check(r.send(cs[g]->d_slab, slab_b, ncclUint8, 0, comms[g], cs[g]->stream), "ncclSend");
            if (want_rad) r.check(r.send(cs[g]->d_rslab, rslab_b / sizeof(float), ncclFloat32, 0, comms[g], cs[g]->stream),
                                  "ncclSend");
        }
        for (int g = 0; g < n; ++g) {
            r.check(r.recv(root.d_gather + (size_t)g * slab_b, slab_b, ncclUint8, g, comms[0], root.stream), "ncclRecv");
            if (want_rad)
                r.check(r.recv(root.d_rgather + (size_t)g * (rslab_b / sizeof(float)), rslab_b / sizeof(float),
                               ncclFloat32, g, comms[0], root.stream),
                        "ncclRecv");
        }
        r.check(r.group_end(), "ncclGroupEnd");
    } else {
        for (int g = 0; g < n; ++g) {
            hip_check(hipStreamWaitEvent(root.stream, cs[g]->ev_rendered, 0), "hipStreamWaitEvent");
            hip_check(hipMemcpyPeerAsync(root.d_gather + (size_t)g * slab_b, root.device, cs[g]->d_slab, cs[g]->device,
                                         slab_b, root.stream),
                      "hipMemcpyPeerAsync");
            if (want_rad)
                hip_check(hipMemcpyPeerAsync(root.d_rgather + (size_t)g * (rslab_b / sizeof(float)), root.device,
                                             cs[g]->d_rslab, cs[g]->device, rslab_b, root.stream),
                          "hipMemcpyPeerAsync");
        }
        // an entry's next render must not overwrite its slab before this copy has read it
        hip_check(hipEventRecord(root.ev_rendered, root.stream), "hipEventRecord");
        for (int g = 1; g < n; ++g) {
            hip_check(hipSetDevice(cs[g]->device), "hipSetDevice");
            hip_check(hipStreamWaitEvent(cs[g]->stream, root.ev_rendered, 0), "hipStreamWaitEvent");
        }
        hip_check(hipSetDevice(root.device), "hipSetDevice");
    }
    const RtRegion reg{plan.region.x, plan.region.y, plan.region.width, plan.region.height, 0, 1};
    if (want_rgb)
        hip_check(launch_tiles_unpack(root.d_gather, n, plan.slab_tiles + 1, reg, C.width, 3, 1, root.d_rgb, root.stream),
                  "tiles_unpack_kernel");
    if (want_rad)
        hip_check(launch_tiles_unpack(root.d_rgather, n, plan.slab_tiles, reg, C.width, 3, 4, root.d_rad, root.stream),
                  "tiles_unpack_kernel");
    hip_check(hipMemcpy2DAsync(root.h_words, ST_WORDS * sizeof(unsigned long long), root.d_gather + plan.stats_offset, slab_b,
                               ST_WORDS * sizeof(unsigned long long), n, hipMemcpyDeviceToHost, root.stream),
              "hipMemcpy2DAsync(stats words)");
    hip_check(hipEventRecord(root.ev_gather1, root.stream), "hipEventRecord");
    if (outputs) outputs(root);  // the caller's copies / encode, queued before the one sync
    hip_check(hipStreamSynchronize(root.stream), "hipStreamSynchronize");
    merge_stats_words(root.h_words, n, merged);
    cam->last = &root;
    return root;
}

}  // namespace rt
