// Pixel finishing, RenderStats merging, slot -> pixel maps and sample records: what the
// accumulate / settle / resolve passes share with the path kernels.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

#include "pt_prof.hpp"

namespace rt {

// writeColorToBuffer (src/camera.ts:455-472) into a Uint8ClampedArray.
__device__ __forceinline__ uint8_t to_u8(float c) {
    const double r = ::sqrt((double)c);
    const double v = ::floor(255.999 * r);
    if (!(v > 0.0)) return 0;
    if (v >= 255.0) return 255;
    return (uint8_t)v;
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ unsigned long long wave_min(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { unsigned long long x = __shfl_xor(v, o, 64); v = x < v ? x : v; }
    return v;
}
__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { unsigned long long x = __shfl_xor(v, o, 64); v = x > v ? x : v; }
    return v;
}

// pixelConverged (src/camera.ts:348-368), in JS doubles. pixel_converged_at_batch is its test
// for an n already known to satisfy n % aBatch == 0 (pt_adapt_kernel counts down to those n
// for an integral aBatch instead of an fp64 fmod per sample).
__device__ __forceinline__ bool pixel_converged_at_batch(const RtCamera& c, int n, double sIll, double sIll2);
__device__ __forceinline__ bool pixel_converged(const RtCamera& c, int n, double sIll, double sIll2) {
    if (c.a_tolerance <= 0.0 || c.samples <= 1.0 || n < 2) return false;
    const double rem = ::fmod((double)n, c.a_batch);
    if (rem != 0.0) return false;  // also NaN
    return pixel_converged_at_batch(c, n, sIll, sIll2);
}
__device__ __forceinline__ bool pixel_converged_at_batch(const RtCamera& c, int n, double sIll, double sIll2) {
    if (c.a_tolerance <= 0.0 || c.samples <= 1.0 || n < 2) return false;
    const double mean = sIll / n;
    const double var = (sIll2 - (sIll * sIll) / n) / (n - 1);
    if (var <= 0.0 || var != var) return true;
    const double ci = 1.96 * ::sqrt(var) / ::sqrt((double)n);
    return ci <= c.a_tolerance * mean;
}

// The camera/options block as seen through an opaque kernarg pointer. Reading
// it this way inside the path loop stops the compiler from hoisting ~30 fp64
// conversions of loop-invariant camera fields into VGPRs for the whole kernel
// (the kernarg segment is constant memory: these are cheap scalar loads).
typedef const __attribute__((address_space(4))) char* KArgPtr;
__device__ __forceinline__ const RtCamera& cam_opaque() {
    KArgPtr p = (KArgPtr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return *(const RtCamera*)(p + offsetof(DevScene, cam));  // addrspacecast; inferred back to constant
}

// Per-pixel result: finalColor (src/camera.ts:326-340) + writeColorToBuffer
// (455-472) + RenderStats.addPixel (renderStats.ts:21-35).
struct PixStats {
    unsigned long long pixels = 0, samples = 0, smin = ~0ull, smax = 0, b = 0, bmin = ~0ull, bmax = 0;
};
// `opix`: the pixel's output index (full-frame j*W + i, or its tile-packed slot).
__device__ __forceinline__ void finish_pixel(const RtCamera& C, const RenderOut& out, uint32_t opix, V3 color, int n,
                                             unsigned long long bsum, int bmin, int bmax, PixStats& st) {
    V3 fin;
    if (C.mode == MODE_BOUNCES) {
        const double avg = n > 0 ? (double)bsum / (double)n : 0.0;
        fin = mk<double>(0.0, 0.0, js_min<double>(avg / (double)C.depth_raw, 1.0));
    } else if (C.mode == MODE_SAMPLES) {
        fin = mk<double>(js_min<double>((double)n / C.samples, 1.0), 0.0, 0.0);
    } else {
        fin = divs<double>(color, (double)n);
    }
    const size_t off = (size_t)opix * 3;
    if (out.radiance) {
        out.radiance[off] = fin.x;
        out.radiance[off + 1] = fin.y;
        out.radiance[off + 2] = fin.z;
    }
    if (out.rgb) {
        out.rgb[off] = to_u8(fin.x);
        out.rgb[off + 1] = to_u8(fin.y);
        out.rgb[off + 2] = to_u8(fin.z);
    }
    if (out.px_samples) out.px_samples[opix] = n;
    if (out.px_bounces) out.px_bounces[opix] = (int32_t)bsum;
    st.pixels += 1;
    st.samples += (unsigned long long)n;
    st.smin = min(st.smin, (unsigned long long)n);
    st.smax = max(st.smax, (unsigned long long)n);
    st.b += bsum;
    if (n > 0) st.bmin = min(st.bmin, (unsigned long long)bmin);
    st.bmax = max(st.bmax, (unsigned long long)bmax);
}

// RenderStats.merge (renderStats.ts:42-64): one atomic per word per wave.
__device__ __forceinline__ void stats_atomics(const RenderOut& out, unsigned long long sp, unsigned long long ss,
                                              unsigned long long smn, unsigned long long smx, unsigned long long sb,
                                              unsigned long long bmn, unsigned long long bmx, unsigned long long err) {
    unsigned long long* w = out.stats;
    if (sp > 0) {
        atomicAdd(&w[ST_PIXELS * kStatStride], sp);
        atomicAdd(&w[ST_SAMPLES * kStatStride], ss);
        atomicMin(&w[ST_SMIN * kStatStride], smn);
        atomicMax(&w[ST_SMAX * kStatStride], smx);
    }
    // bounce words also from the path kernels' lanes (12-byte records: LaneBounces, no pixels)
    if (sp > 0 || bmn != ~0ull) {
        atomicAdd(&w[ST_BOUNCES * kStatStride], sb);
        atomicMin(&w[ST_BMIN * kStatStride], bmn);
        atomicMax(&w[ST_BMAX * kStatStride], bmx);
    }
    if (err) atomicOr(&w[ST_ERROR * kStatStride], err);
}
__device__ __forceinline__ unsigned long long wave_or(unsigned long long v) {
#pragma unroll
    for (int k = 32; k > 0; k >>= 1) v |= __shfl_xor(v, k, 64);
    return v;
}
__device__ __forceinline__ void publish_stats(const RenderOut& out, const PixStats& st, unsigned long long st_err,
                                              int lane) {
    const unsigned long long sp = wave_sum(st.pixels), ss = wave_sum(st.samples), sb = wave_sum(st.b);
    const unsigned long long smn = wave_min(st.smin), smx = wave_max(st.smax);
    const unsigned long long bmn = wave_min(st.bmin), bmx = wave_max(st.bmax);
    const unsigned long long err = wave_or(st_err);
    if (lane == 0) stats_atomics(out, sp, ss, smn, smx, sb, bmn, bmx, err);
}

template <bool COUNT, bool PROF>
__device__ __forceinline__ void publish_counters(const RenderOut& out, const uint32_t* cnt, Prof& pf, int lane) {
    if (COUNT) {
#pragma unroll
        for (int k = 0; k < CT_WORDS; ++k) {
            const unsigned long long v = wave_sum((unsigned long long)cnt[k]);
            if (lane == 0 && v) atomicAdd(&out.counters[k], v);
        }
    }
    if (PROF) {
        psec<PROF>(pf, PR_TILE);
        // lane 0 publishes the wave's totals from its LDS slot; PR_LOOP = the wave's lifetime
        if (lane == 0) {
            const unsigned long long life = __builtin_amdgcn_s_memtime() - pf.w[1];
            for (int k = 0; k < PR_WORDS; ++k)
                atomicAdd(&out.counters[CT_WORDS + k], k == PR_LOOP ? life : pf.w[2 + k]);
            for (int k = 0; k < PR_LOOP; ++k) {
                atomicAdd(&out.counters[CT_WORDS + PR_WORDS + k], pf.w[2 + PR_WORDS + k]);
                atomicAdd(&out.counters[CT_WORDS + PR_WORDS + PR_LOOP + k], pf.w[2 + 2 * PR_WORDS + k]);
            }
        }
    }
}

// One 16-byte sample record; NT: a non-temporal store. The pool kernel's records (read once,
// by the accumulate pass) go out non-temporally: Cornell writes 4.27 GB per launch instead of
// 4.78 GB for 2.62 GB of records (1.67x instead of 1.87x) at the same kernel time. The
// chunked kernel keeps plain stores: a lane writes its item's samples in turn, and spheres-500
// wrote 0.97 GB instead of 0.89 GB non-temporally (profiles/r02/recnt/).
// The finished sample's error flags for its record (SampleBuf::err_in_rec): the lane's flags
// since its previous sample (a lane runs one path at a time), which then start over; 0 and
// the flags stay in `st_err` for the launch's stats otherwise.
__device__ __forceinline__ int rec_err_bits(int err_in_rec, unsigned long long& st_err) {
    if (!err_in_rec) return 0;
    const int b = (int)((uint32_t)st_err << kRecErrShift);
    st_err = 0;
    return b;
}

template <bool NT>
__device__ __forceinline__ void rec_store(float4* p, float4 r);
// a 12-byte record (loads / stores of a 3-element vector move 12 bytes; its sizeof is 16, so
// records are addressed in floats)
typedef float RecF3 __attribute__((ext_vector_type(3), aligned(4)));
// A lane's bounce statistics over the samples it recorded (SampleBuf::rec12). The sum is 32-bit
// with a carry: a lane records ~10^4 samples per launch at the 8 GB record budget and depth goes
// up to 1e9, so a 32-bit sum can wrap; on a wrap the old sum goes to the launch's
// bounce total by one atomic (never in practice: 2^32 bounces in one lane's launch). (A 64-bit
// sum instead cost the pool kernel an extra spilled register reloaded in its trip loop: Cornell
// 13.91 -> 14.02 ms, profiles/r05/final/.)
struct LaneBounces {
    uint32_t sum = 0, mn = 0xffffffffu, mx = 0;
    __device__ void add(int b, unsigned long long* stats) {
        const uint32_t ns = sum + (uint32_t)b;
        if (ns < sum) {
            atomicAdd(stats + ST_BOUNCES * kStatStride, (unsigned long long)sum);
            sum = (uint32_t)b;
        } else {
            sum = ns;
        }
        mn = min(mn, (uint32_t)b);
        mx = max(mx, (uint32_t)b);
    }
    // into the launch's RenderStats (publish_stats): the accumulate pass adds none
    __device__ void to(PixStats& st) const {
        st.b = sum;
        st.bmin = mn == 0xffffffffu ? ~0ull : (unsigned long long)mn;
        st.bmax = mx;
    }
};
// The sample's record at index `idx` (s * stride_s + slot * stride_slot): {rgb, w} or, with
// rec12, {rgb} and w's bounce count into the lane's statistics.
template <bool NT>
__device__ __forceinline__ void rec_put(const SampleBuf& sb, size_t idx, V3 c, int w, LaneBounces& lb,
                                        unsigned long long* stats) {
    if (sb.rec12) {
        RecF3* p = reinterpret_cast<RecF3*>(reinterpret_cast<float*>(sb.rec) + 3 * idx);
        if constexpr (NT) __builtin_nontemporal_store(RecF3{c.x, c.y, c.z}, p);
        else *p = RecF3{c.x, c.y, c.z};
        lb.add(w, stats);
    } else {
        rec_store<NT>(sb.rec + idx, make_float4(c.x, c.y, c.z, __int_as_float(w)));
    }
}
template <bool NT>
__device__ __forceinline__ void rec_store(float4* p, float4 r) {
    if constexpr (NT) {
        typedef float f4v __attribute__((ext_vector_type(4)));
        __builtin_nontemporal_store(f4v{r.x, r.y, r.z, r.w}, reinterpret_cast<f4v*>(p));
    } else {
        *p = r;
    }
}

// n / d for 0 <= n < 2^31, d >= 1, through a double reciprocal (rinv = 1.0 / d)
// and one correction step: cheaper than the integer division sequence.
__device__ __forceinline__ int udiv(int n, int d, double rinv) {
    int q = (int)((double)n * rinv);
    const int r = n - q * d;
    q += (r >= d) ? 1 : 0;
    q -= (r < 0) ? 1 : 0;
    return q;
}

__device__ __forceinline__ void item_pixel(const RtRegion& reg, int tiles_x, int mt, int l, int& i, int& j) {
    const int gt = reg.tile_group + mt * reg.tile_groups;
    const int ty = gt / tiles_x;
    i = reg.x + (gt - ty * tiles_x) * kTile + (l & (kTile - 1));
    j = reg.y + ty * kTile + (l / kTile);
}
__device__ __forceinline__ void item_pixel(const RtRegion& reg, int tiles_x, double rtx, int mt, int l, int& i,
                                           int& j) {
    const int gt = reg.tile_group + mt * reg.tile_groups;
    const int ty = udiv(gt, tiles_x, rtx);
    i = reg.x + (gt - ty * tiles_x) * kTile + (l & (kTile - 1));
    j = reg.y + ty * kTile + (l / kTile);
}
// Record slot a of the pass -> its pixel (i, j) (through the adaptive round's
// active list when there is one); false past the pass's slots or outside the region.
template <class SB>
__device__ __forceinline__ bool slot_pixel(const SB& sb, const RtRegion& reg, int tiles_x, double rtx, int endX,
                                           int endY, int a, int& i, int& j) {
    int ls = a;
    if (sb.act) {
        if (a >= sb.slots) return false;
        ls = sb.act[a];
        // Wait for this load here, on every path. Otherwise (fixed-spp launches never take this
        // branch) the wait-count pass kept its destination register pending on the paths around
        // the branch, and every later write of that register - a common temporary - waited with
        // vmcnt(0): for the sample records just stored, too.
        __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0), expcnt / lgkmcnt unchanged (gfx9 encoding)
    }
    item_pixel(reg, tiles_x, rtx, sb.tile0 + (ls >> 6), ls & 63, i, j);
    return i < endX && j < endY;
}

}  // namespace rt
