// switched.hip -- rows of the bootstrap workspace into the modulus-switched stored form and back (switched.h,
// DESIGN.md 6k).
//
// Both sides are contiguous in units: a workspace row is upr = ms_stride / 8 units of 64 bytes (8 words), a
// packed device row upr groups of 12 bytes (8 values of 12 bits), so unit u of the one is group u of the other
// whatever row it lies in, and both launches are flat over the units, one lane per unit.
//
// k_ms_pack.  A lane loads its unit with four 16-byte loads, rounds the eight words to 12 bits (modswitch_2n) and
// stores three dwords; a wave's stores cover 768 bytes without a gap.  The unit that holds word n is read word
// by word, words above n are not read and count as 0: the pad nibble and the group's remaining bytes come out
// zero.  A unit wholly above n (n + 1 a multiple of 8 has none) cannot occur: upr = ceil((n + 1) / 8).
//
// k_ms_unpack.  A lane loads its group's three dwords and stores the eight words v << 52 with four 16-byte
// stores; above n it stores kMsPadWord, what k_oprf_rows leaves there: the blind rotations read words 0 .. n only
// (their prefetches are clamped to the body), so the padding's value is free, and a kernel that writes whole units
// gives it the one content the workspace's other whole-row writer does.
//
// No LDS, no atomics, no scratch; a lane finds its row by one 32-bit division, only to know where word n is.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_math.h"
#include "oprf.h"
#include "switched.h"

namespace fhe {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) u32x4 g_u32x4;
typedef __attribute__((address_space(1))) uint32_t g_u32;
typedef __attribute__((address_space(1))) uint64_t g_u64;

__device__ __forceinline__ uint64_t word_of(u32x4 v, int hi) {
    return hi ? (uint64_t)v.z | ((uint64_t)v.w << 32) : (uint64_t)v.x | ((uint64_t)v.y << 32);
}

__global__ __launch_bounds__(256) void k_ms_pack(const uint64_t* __restrict__ ws, uint32_t* __restrict__ packed,
                                                 uint32_t units, uint32_t upr, uint32_t n) {
    const uint32_t u = blockIdx.x * 256u + threadIdx.x;
    if (u >= units) return;
    const uint32_t row = u / upr, w0 = (u - row * upr) * 8u;  // the unit's first word within its row
    const g_u64* src = (const g_u64*)ws + (size_t)u * 8u;
    uint32_t v[8];
    if (w0 + 8u <= n + 1u) {
        u32x4 x[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = ((const g_u32x4*)src)[k];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = modswitch_2n(word_of(x[j >> 1], j & 1));
    } else {
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) v[j] = w0 + j <= n ? modswitch_2n(src[j]) : 0u;
    }
    g_u32* dst = (g_u32*)packed + (size_t)u * 3u;
    dst[0] = v[0] | v[1] << 12 | v[2] << 24;
    dst[1] = v[2] >> 8 | v[3] << 4 | v[4] << 16 | v[5] << 28;
    dst[2] = v[5] >> 4 | v[6] << 8 | v[7] << 20;
}

__global__ __launch_bounds__(256) void k_ms_unpack(const uint32_t* __restrict__ packed, uint64_t* __restrict__ ws,
                                                   uint32_t units, uint32_t upr, uint32_t n) {
    const uint32_t u = blockIdx.x * 256u + threadIdx.x;
    if (u >= units) return;
    const uint32_t row = u / upr, w0 = (u - row * upr) * 8u;
    const g_u32* src = (const g_u32*)packed + (size_t)u * 3u;
    const uint32_t d0 = src[0], d1 = src[1], d2 = src[2];
    const uint32_t v[8] = {d0 & 4095u,         (d0 >> 12) & 4095u, (d0 >> 24 | d1 << 8) & 4095u, (d1 >> 4) & 4095u,
                           (d1 >> 16) & 4095u, (d1 >> 28 | d2 << 4) & 4095u, (d2 >> 8) & 4095u,  d2 >> 20};
    g_u32x4* dst = (g_u32x4*)((g_u64*)ws + (size_t)u * 8u);
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        // value << 52: the low dword is 0, the high one v << 20
        const uint32_t a = w0 + 2u * k, b = a + 1u;
        u32x4 o;
        o.x = a <= n ? 0u : (uint32_t)kMsPadWord;
        o.y = a <= n ? v[2 * k] << 20 : (uint32_t)(kMsPadWord >> 32);
        o.z = b <= n ? 0u : (uint32_t)kMsPadWord;
        o.w = b <= n ? v[2 * k + 1] << 20 : (uint32_t)(kMsPadWord >> 32);
        dst[k] = o;
    }
}

// at most 2^30 units per launch: the kernels' unit arithmetic is 32-bit
template <class F>
hipError_t over_units(size_t count, uint32_t n, F&& launch) {
    const uint32_t upr = (uint32_t)(ms_stride_words(n) / 8);
    const size_t step = ((size_t)1 << 30) / upr;
    for (size_t at = 0; at < count; at += step) {
        const uint32_t rows = (uint32_t)(count - at < step ? count - at : step);
        launch(at * upr, rows * upr, upr);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace

hipError_t launch_ms_pack(const uint64_t* ws, uint32_t* packed, size_t count, uint32_t n, hipStream_t s) {
    return over_units(count, n, [&](size_t u0, uint32_t units, uint32_t upr) {
        k_ms_pack<<<(units + 255u) / 256u, 256, 0, s>>>(ws + u0 * 8, packed + u0 * 3, units, upr, n);
    });
}

hipError_t launch_ms_unpack(const uint32_t* packed, uint64_t* ws, size_t count, uint32_t n, hipStream_t s) {
    return over_units(count, n, [&](size_t u0, uint32_t units, uint32_t upr) {
        k_ms_unpack<<<(units + 255u) / 256u, 256, 0, s>>>(packed + u0 * 3, ws + u0 * 8, units, upr, n);
    });
}

}  // namespace fhe
