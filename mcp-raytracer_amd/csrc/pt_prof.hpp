// The diagnostic section timer of the INSTR == 2 kernel builds.
#pragma once

#include <hip/hip_runtime.h>

#include "pt_types.hpp"

namespace rt {

__device__ __forceinline__ unsigned long long clk() { return __builtin_amdgcn_s_memtime(); }

// Diagnostic section timer (INSTR == 2), wave view: every psec() ends the
// wave's current section - whichever of its lanes execute it - and charges the
// wave-cycles since the previous psec() of ANY lane to it, together with the
// active lanes at that point. The wave's clock and sums live in one LDS slot per
// wave, updated by the first active lane, so time spent in code that only some
// lanes run is attributed once, to that code.
// Slot words: [0] last stamp, [1] start stamp, [2 + k] cycles of section k
// (k = PR_TRIPS: loop trips), [2 + PR_WORDS + k] active lanes, [2 + 2 PR_WORDS + k] executions.
struct Prof {
    unsigned long long* w;  // this wave's LDS slot
};
template <bool PROF>
__device__ __forceinline__ void prof_init(Prof& pf, unsigned long long* lds, int lane) {
    if (PROF) {
        pf.w = lds + (threadIdx.x >> 6) * kProfSlot;
        if (lane == 0) {
            for (int k = 0; k < kProfSlot; ++k) pf.w[k] = 0ull;
            const unsigned long long n = __builtin_amdgcn_s_memtime();
            pf.w[0] = n;
            pf.w[1] = n;
        }
    }
}
template <bool PROF>
__device__ __forceinline__ void psec(Prof& pf, int k) {
    if (PROF) {
        const unsigned long long m = __ballot(1);
        if ((int)(threadIdx.x & 63) == __builtin_ctzll(m)) {
            const unsigned long long n = __builtin_amdgcn_s_memtime();
            pf.w[2 + k] += n - pf.w[0];
            pf.w[0] = n;
            pf.w[2 + PR_WORDS + k] += (unsigned long long)__popcll(m);
            pf.w[2 + 2 * PR_WORDS + k] += 1ull;
        }
    }
}
// Lane count of one execution of section k, without charging cycles (loop bodies too
// short for a timer: node steps, leaf tests).
template <bool PROF>
__device__ __forceinline__ void pcount(Prof& pf, int k) {
    if (PROF) {
        const unsigned long long m = __ballot(1);
        if ((int)(threadIdx.x & 63) == __builtin_ctzll(m)) {
            pf.w[2 + PR_WORDS + k] += (unsigned long long)__popcll(m);
            pf.w[2 + 2 * PR_WORDS + k] += 1ull;
        }
    }
}
template <bool PROF>
__device__ __forceinline__ void prof_trip(Prof& pf) {
    if (PROF) {
        const unsigned long long m = __ballot(1);
        if ((int)(threadIdx.x & 63) == __builtin_ctzll(m)) pf.w[2 + PR_TRIPS] += 1ull;
    }
}

}  // namespace rt
