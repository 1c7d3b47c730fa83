// The path code's numerics: the seeded RNG, Math.* on the scalar type, uniform scene reads.
#pragma once

#include <hip/hip_runtime.h>

#include "pt_types.hpp"

namespace rt {

// ---------------------------------------------------------------------------
// Seeded replacement for Math.random: PCG32 (XSH-RR) stream per (seed, pixel,
// sample), consumed in the reference's draw order.
// ---------------------------------------------------------------------------
// seed_mix = splitmix64(seed), precomputed per camera (RtCamera::seed_mix)
__device__ __forceinline__ uint64_t rng_init(uint64_t seed_mix, uint32_t pixel, uint32_t sample) {
    return splitmix64((((uint64_t)pixel << 32) | sample) ^ seed_mix);
}
__device__ __forceinline__ uint32_t rng_u32(uint64_t& s) {
    const uint64_t old = s;
    s = old * 6364136223846793005ull + 1442695040888963407ull;
    const uint32_t xs = (uint32_t)(((old >> 18u) ^ old) >> 27u);
    const uint32_t rot = (uint32_t)(old >> 59u);
    return (xs >> rot) | (xs << ((32u - rot) & 31u));
}
template <class Real> __device__ __forceinline__ Real uniform(uint64_t& s);
template <> __device__ __forceinline__ double uniform<double>(uint64_t& s) {
    return (double)rng_u32(s) * (1.0 / 4294967296.0);
}
template <> __device__ __forceinline__ float uniform<float>(uint64_t& s) {
    return (float)(rng_u32(s) >> 8) * (1.0f / 16777216.0f);
}

// Math.* on the scalar type.
__device__ __forceinline__ double m_cos(double x) { return ::cos(x); }
__device__ __forceinline__ float m_cos(float x) { return ::cosf(x); }
__device__ __forceinline__ double m_sin(double x) { return ::sin(x); }
__device__ __forceinline__ float m_sin(float x) { return ::sinf(x); }
// Math.cos(x) and Math.sin(x) of one argument: ocml's sincos evaluates the sine and cosine
// polynomials once (separate sin + cos calls each evaluate both and select) and returns
// bit-for-bit sin(x) and cos(x) (tools/probes/sincos_check: all 2^32 cosine-PDF angles, fp64
// and fp32). Cornell 7718 -> 7933 Msamples/s (profiles/r01/sincos/).
template <class Real>
__device__ __forceinline__ void m_sincos(Real x, Real& s, Real& c) {
    if constexpr (sizeof(Real) == 8) ::sincos(x, &s, &c);
    else ::sincosf(x, &s, &c);
}
// Math.pow(x, 5) of Schlick's approximation (src/materials/dielectric.ts:98),
// correctly rounded: x^5 in double-double (exact x^2 and x^4 products via FMA),
// then one rounding. V8's and glibc's pow are within 1 ulp of this value (and
// differ from it for ~0.1 % of arguments); it only feeds `reflectance > xi`.
// The oracle computes the same correctly rounded value independently (binary128).
__device__ __forceinline__ double pow5(double x) {
    const double h2 = x * x, l2 = ::fma(x, x, -h2);
    const double h4 = h2 * h2, l4 = ::fma(h2, h2, -h4) + 2.0 * h2 * l2;
    const double h5 = h4 * x, l5 = ::fma(h4, x, -h5) + l4 * x;
    return h5 + l5;
}
__device__ __forceinline__ float pow5(float x) {
    const float x2 = x * x;
    return x2 * x2 * x;
}
__device__ __forceinline__ double m_abs(double x) { return ::fabs(x); }
__device__ __forceinline__ float m_abs(float x) { return ::fabsf(x); }
// Math.sqrt. (Routing it through rt_math.hpp sqrt_rn behind a range test was no faster anywhere:
// the branch costs what the skipped scaling steps save, profiles/r04/fp64/.)
__device__ __forceinline__ double m_sqrt(double x) { return ::sqrt(x); }
__device__ __forceinline__ float m_sqrt(float x) { return ::sqrtf(x); }

template <class Real> struct K {
    static constexpr Real PI = (Real)3.141592653589793;
    static constexpr Real TMIN = (Real)0.001;
};

__device__ __forceinline__ V3 ld3(const float* p) { return V3{p[0], p[1], p[2]}; }

// Wave-uniform reads of scene records that are never written during a launch:
// through the constant address space, so the compiler emits scalar loads
// (s_load, scalar cache) instead of vector loads with full memory latency.
template <class T>
__device__ __forceinline__ T ld_uniform(const T* base, int k) {
    static_assert(sizeof(T) % 4 == 0, "dword records");
    typedef const __attribute__((address_space(4))) uint32_t* CW;
    const CW src = (CW)(const void*)(base + k);
    T out;
    uint32_t* dst = reinterpret_cast<uint32_t*>(&out);
#pragma unroll
    for (int i = 0; i < (int)(sizeof(T) / 4); ++i) dst[i] = src[i];
    return out;
}

}  // namespace rt
