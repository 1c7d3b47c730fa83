// The selection of a focused step (focus.hpp): score pass, radix select, compaction. Compiled
// with -ffp-contract=off: the session's variance is progressive.hpp's prog_variance, the value
// rt_camera_progressive_variance returns, evaluated without contraction. Everything after the
// score is integer work on bit patterns.
#include "focus.hpp"

#include <algorithm>

namespace rt {

constexpr int kFocusBlock = 256;
static_assert(kFocusBins == kFocusBlock, "one histogram bin per thread of a workgroup");

// Score pass: entry a of the active list -> key[a], its sanitised score's bit pattern when the
// pixel is eligible (score > min_score), else 0. A sanitised score is +0 or a positive finite
// float, whose bit patterns order as the values do: the comparisons are made on them, so
// denormals compare as they are whatever the float mode. Counts the eligible entries (one
// atomic per workgroup).
__global__ __launch_bounds__(kFocusBlock) void focus_score_kernel(FocusArgs A) {
    const int lane = threadIdx.x & (kWave - 1);
    const int w = threadIdx.x / kWave;
    unsigned int mine = 0;
    for (int a = blockIdx.x * kFocusBlock + (int)threadIdx.x; a < A.n_act; a += gridDim.x * kFocusBlock) {
        const int ls = A.act[a];
        uint32_t bits = 0;
        if (A.plane) {
            const int tile = ls >> 6, l = ls & (kWave - 1);
            const int ty = tile / A.tiles_x;
            const int px = (tile - ty * A.tiles_x) * kTile + (l & (kTile - 1)), py = ty * kTile + l / kTile;
            if (px < A.w && py < A.h) bits = __float_as_uint(A.plane[(size_t)py * (size_t)A.w + (size_t)px]);
        } else {
            const ProgPix& q = A.state[ls];
            const uint32_t n = __float_as_uint(q.c.w) & ~kProgFinished;
            const double2 ill = q.ill;
            bits = __float_as_uint(prog_variance(ill.x, ill.y, n));
        }
        // not (>= 0 and finite) -> 0: a negative (sign bit), an infinity or a NaN (exponent all ones)
        if (bits >= 0x7f800000u) bits = 0;
        const bool eligible = bits > A.min_bits;
        A.key[a] = eligible ? bits : 0u;
        mine += eligible ? 1u : 0u;
    }
    __shared__ unsigned int wsum[kFocusBlock / kWave];
    for (int off = kWave / 2; off > 0; off >>= 1) mine += __shfl_down(mine, off);
    if (lane == 0) wsum[w] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned int tot = 0;
        for (int q = 0; q < kFocusBlock / kWave; ++q) tot += wsum[q];
        if (tot) atomicAdd(&A.words[kFocusEligible], tot);
    }
}

// The state before digit pass p - the digits found so far and the rank still to find below them -
// from the state before pass p - 1 and that pass's histogram; every workgroup derives it for
// itself (256 bins: one per thread, a suffix sum in LDS), so the host reads nothing in between.
// Before pass 0: no digit, rank min(K, eligible), so at most K eligible keys make the smallest of
// them the K-th largest. With p == kFocusPasses the prefix is T. Rank 0: nothing is eligible.
// Every thread of the workgroup calls it (it synchronises); scan: kFocusBins words, sh: 2 words.
struct FocusState {
    uint32_t prefix, rank;
};
__device__ __forceinline__ FocusState focus_state(const FocusArgs& A, int p, uint32_t* scan, uint32_t* sh) {
    if (p == 0) return FocusState{0u, min(A.k, A.words[kFocusEligible])};
    const int t = threadIdx.x;
    const uint32_t prefix = A.words[kFocusState + 2 * (p - 1)], rank = A.words[kFocusState + 2 * (p - 1) + 1];
    const uint32_t own = A.words[kFocusHist + (p - 1) * kFocusBins + t];
    // inclusive suffix sum: scan[t] = sum of the bins >= t (Hillis-Steele over 256 threads)
    scan[t] = own;
    __syncthreads();
    for (int off = 1; off < kFocusBins; off <<= 1) {
        const uint32_t add = t + off < kFocusBins ? scan[t + off] : 0u;
        __syncthreads();
        scan[t] += add;
        __syncthreads();
    }
    const uint32_t above = scan[t] - own;  // keys whose digit is larger than t
    if (rank > 0 && above < rank && rank <= above + own) {  // exactly one bin holds the rank-th largest
        sh[0] = prefix | ((uint32_t)t << (32 - kFocusDigitBits * p));
        sh[1] = rank - above;
    }
    if (rank == 0 && t == 0) sh[0] = 0u, sh[1] = 0u;
    __syncthreads();
    return FocusState{sh[0], sh[1]};
}

// Digit pass p: the histogram of digit p over the keys that carry the digits found so far, built
// in LDS per workgroup and merged with one global atomic per non-empty bin.
__global__ __launch_bounds__(kFocusBlock) void focus_digit_kernel(FocusArgs A, int p) {
    __shared__ uint32_t scan[kFocusBins];
    __shared__ uint32_t hist[kFocusBins];
    __shared__ uint32_t sh[2];
    const FocusState s = focus_state(A, p, scan, sh);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        A.words[kFocusState + 2 * p] = s.prefix;
        A.words[kFocusState + 2 * p + 1] = s.rank;
    }
    if (s.rank == 0) return;  // (block-uniform) nothing eligible
    hist[threadIdx.x] = 0u;
    __syncthreads();
    const int shift = 32 - kFocusDigitBits * (p + 1);
    // the bits above digit p: all of them must equal the prefix's (pass 0: there are none)
    const uint32_t high = p == 0 ? 0u : ~0u << (shift + kFocusDigitBits);
    for (int a = blockIdx.x * kFocusBlock + (int)threadIdx.x; a < A.n_act; a += gridDim.x * kFocusBlock) {
        const uint32_t key = A.key[a];
        if (key != 0u && (key & high) == s.prefix) atomicAdd(&hist[(key >> shift) & (kFocusBins - 1)], 1u);
    }
    __syncthreads();
    const uint32_t c = hist[threadIdx.x];
    if (c) atomicAdd(&A.words[kFocusHist + p * kFocusBins + threadIdx.x], c);
}

// Compaction: T from the last digit pass, then every entry with key >= T (and eligible) is
// appended to the focus list as pt_resolve_kernel appends the active list (__ballot + mbcnt,
// one atomic per workgroup and iteration), and marked in the full-frame mask.
__global__ __launch_bounds__(kFocusBlock) void focus_compact_kernel(FocusArgs A) {
    __shared__ uint32_t scan[kFocusBins];
    __shared__ uint32_t sh[2];
    __shared__ unsigned int wcnt[kFocusBlock / kWave];
    __shared__ unsigned int wbase;
    const FocusState s = focus_state(A, kFocusPasses, scan, sh);
    const uint32_t T = s.prefix;
    if (blockIdx.x == 0 && threadIdx.x == 0) A.words[kFocusThreshold] = T;
    if (s.rank == 0) return;  // (block-uniform) nothing eligible: the list stays empty
    const int lane = threadIdx.x & (kWave - 1);
    const int w = threadIdx.x / kWave;
    const int stride = gridDim.x * kFocusBlock;
    const int n_iter = (A.n_act + stride - 1) / stride;  // block-uniform trip count (the append syncs)
    for (int it = 0; it < n_iter; ++it) {
        const int a = it * stride + blockIdx.x * kFocusBlock + (int)threadIdx.x;
        bool take = false;
        int ls = 0;
        if (a < A.n_act) {
            const uint32_t key = A.key[a];
            take = key != 0u && key >= T;
            ls = A.act[a];
        }
        const unsigned long long m = __ballot(take);
        if (lane == 0) wcnt[w] = (unsigned int)__popcll(m);
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned int tot = 0;
            for (int q = 0; q < kFocusBlock / kWave; ++q) {
                const unsigned int c = wcnt[q];
                wcnt[q] = tot;
                tot += c;
            }
            wbase = tot ? atomicAdd(&A.words[kFocusSelected], tot) : 0u;
        }
        __syncthreads();
        if (take) {
            const int r = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            // (at most n_act entries are taken: the list holds the session's slots)
            A.list[wbase + wcnt[w] + (unsigned int)r] = ls;
            if (A.mask) {
                const int tile = ls >> 6, l = ls & (kWave - 1);
                const int ty = tile / A.tiles_x;
                const int px = (tile - ty * A.tiles_x) * kTile + (l & (kTile - 1)), py = ty * kTile + l / kTile;
                if (px < A.w && py < A.h) A.mask[(size_t)(A.y0 + py) * (size_t)A.pitch + (size_t)(A.x0 + px)] = 1;
            }
        }
        __syncthreads();
    }
}

hipError_t launch_focus_select(const FocusArgs& a, hipStream_t stream) {
    if (a.n_act <= 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(a.words, 0, kFocusWords * sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    const int grid = std::max(1, std::min((a.n_act + kFocusBlock - 1) / kFocusBlock, 1024));
    hipLaunchKernelGGL(focus_score_kernel, dim3(grid), dim3(kFocusBlock), 0, stream, a);
    for (int p = 0; p < kFocusPasses; ++p)
        hipLaunchKernelGGL(focus_digit_kernel, dim3(grid), dim3(kFocusBlock), 0, stream, a, p);
    hipLaunchKernelGGL(focus_compact_kernel, dim3(grid), dim3(kFocusBlock), 0, stream, a);
    return hipGetLastError();
}

}  // namespace rt
