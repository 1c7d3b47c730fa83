// The primary-ray candidate table (primary.hpp): the kernel that fills it for a camera's
// whole image, and the host loop over the same function. Compiled with -ffp-contract=off:
// the host and the device then run the same IEEE double operations and the two tables are
// equal bit for bit.
#include "primary.hpp"

#include <hip/hip_runtime.h>

namespace rt {

constexpr int kPrimaryBlock = 256;

__global__ __launch_bounds__(kPrimaryBlock) void primary_table_kernel(RtCamera C, const RtPrim* __restrict__ prims,
                                                                      int n_prims, uint64_t* __restrict__ out) {
    const long n = (long)C.width * C.height;
    const long p = (long)blockIdx.x * kPrimaryBlock + threadIdx.x;
    if (p >= n) return;
    const int j = (int)(p / C.width), i = (int)(p - (long)j * C.width);
    out[p] = primary_record(C, prims, n_prims, i, j);
}

hipError_t launch_primary_table(const RtCamera& C, const RtPrim* prims, int n_prims, uint64_t* out,
                                hipStream_t stream) {
    const long n = (long)C.width * C.height;
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(primary_table_kernel, dim3((unsigned)((n + kPrimaryBlock - 1) / kPrimaryBlock)),
                       dim3(kPrimaryBlock), 0, stream, C, prims, n_prims, out);
    return hipGetLastError();
}

void primary_table_host(const RtCamera& C, const RtPrim* prims, int n_prims, uint64_t* out) {
    for (int j = 0; j < C.height; ++j)
        for (int i = 0; i < C.width; ++i) out[(size_t)j * C.width + i] = primary_record(C, prims, n_prims, i, j);
}

}  // namespace rt
