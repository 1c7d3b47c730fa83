// From a launch's KernelVariant to its kernel template instance: included by the two precision
// units (pt_ref.hip, pt_fp32.hip) only, which instantiate the path kernels.
#pragma once

#include "launch.hpp"
#include "pt_pool.hpp"

namespace rt {

// The kernel template instance of a launch (one per scalar precision unit: pt_ref.hip,
// pt_fp32.hip). sb == nullptr: the sequential-pixel kernel; else the chunked kernel, or the
// pool kernel (product brute-force builds; RT_POOL_PROF adds its ref-precision timer build).
template <class Real, bool EMIT, int INSTR, int TRAV, int LDSS>
hipError_t dispatch_kernel(const DevScene& S, const RtRegion& reg, const RenderOut& out, const LaunchGeom& g,
                           const SampleBuf* sb, bool pool, const uint2* ptab, hipStream_t stream) {
    if (sb && pool) {
        if constexpr (!EMIT && TRAV == TRAV_BRUTE && (INSTR == 0 || (RT_POOL_PROF && INSTR == 2 && sizeof(Real) == 8))) {
            if (ptab)  // with the primary-ray candidate table (primary.hpp)
                hipLaunchKernelGGL((pt_pool_primary_kernel<Real, TRAV, LDSS>), dim3(g.grid), dim3(kBlockPool),
                                   g.lds_bytes, stream, S, reg, out, g.tiles_x, *sb, ptab);
            else
                hipLaunchKernelGGL((pt_pool_kernel<Real, TRAV, LDSS>), dim3(g.grid), dim3(kBlockPool), g.lds_bytes,
                                   stream, S, reg, out, g.tiles_x, *sb);
            return hipGetLastError();
        } else {
            return hipErrorInvalidValue;
        }
    }
    if (sb)
        hipLaunchKernelGGL((pt_chunk_kernel<Real, EMIT, INSTR, TRAV, LDSS>), dim3(g.grid), dim3(kBlockChunk),
                           g.lds_bytes, stream, S, reg, out, g.tiles_x, *sb);
    else
        hipLaunchKernelGGL((pt_render_kernel<Real, EMIT, INSTR, TRAV, LDSS>), dim3(g.grid), dim3(kBlock), g.lds_bytes,
                           stream, S, reg, out, g.tiles_x, g.my_tiles);
    return hipGetLastError();
}

template <class Real, bool EMIT, int INSTR, int TRAV>
hipError_t dispatch_level(const DevScene& S, const RtRegion& reg, const RenderOut& out, const LaunchGeom& g,
                          const SampleBuf* sb, bool pool, const uint2* ptab, hipStream_t stream) {
    // LDS residency levels (pt_kernels.hpp scene_prologue); never with the reference traversal
    constexpr int L1 = trav_fast(TRAV) ? 1 : 0, L2 = TRAV == TRAV_REFERENCE ? 0 : 2;
    if (g.lds_level >= 2) return dispatch_kernel<Real, EMIT, INSTR, TRAV, L2>(S, reg, out, g, sb, pool, ptab, stream);
    if (g.lds_level == 1) return dispatch_kernel<Real, EMIT, INSTR, TRAV, L1>(S, reg, out, g, sb, pool, ptab, stream);
    return dispatch_kernel<Real, EMIT, INSTR, TRAV, 0>(S, reg, out, g, sb, pool, ptab, stream);
}

template <class Real, int TRAV>
hipError_t dispatch_variant(const KernelVariant& v, const DevScene& S, const RtRegion& reg, const RenderOut& out,
                            const LaunchGeom& g, const SampleBuf* sb, hipStream_t stream) {
    if (v.count == 2)
        return v.emit ? dispatch_level<Real, true, 2, TRAV>(S, reg, out, g, sb, v.pool, v.ptab, stream)
                      : dispatch_level<Real, false, 2, TRAV>(S, reg, out, g, sb, v.pool, v.ptab, stream);
    if (v.count == 1)
        return v.emit ? dispatch_level<Real, true, 1, TRAV>(S, reg, out, g, sb, v.pool, v.ptab, stream)
                      : dispatch_level<Real, false, 1, TRAV>(S, reg, out, g, sb, v.pool, v.ptab, stream);
    return v.emit ? dispatch_level<Real, true, 0, TRAV>(S, reg, out, g, sb, v.pool, v.ptab, stream)
                  : dispatch_level<Real, false, 0, TRAV>(S, reg, out, g, sb, v.pool, v.ptab, stream);
}

template <class Real>
hipError_t dispatch_render(const KernelVariant& v, const DevScene& S, const RtRegion& reg, const RenderOut& out,
                           const LaunchGeom& g, const SampleBuf* sb, hipStream_t stream) {
    if (v.trav == TRAV_BRUTE) return dispatch_variant<Real, TRAV_BRUTE>(v, S, reg, out, g, sb, stream);
    if (v.trav == TRAV_FAST)
        return v.defer ? dispatch_variant<Real, TRAV_FAST_DEFER>(v, S, reg, out, g, sb, stream)
                       : dispatch_variant<Real, TRAV_FAST>(v, S, reg, out, g, sb, stream);
    return dispatch_variant<Real, TRAV_REFERENCE>(v, S, reg, out, g, sb, stream);
}

}  // namespace rt
