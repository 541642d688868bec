// ms_center.hip -- the centered modulus switch: the public half of the rounding error leaves the
// body before the blind rotation rounds it.
//
// For a keyswitched small LWE row a[0 .. n-1], b = a[n] of 64-bit words, res(x) is the signed distance of x
// from the multiple of 2^52 that modswitch_2n rounds it to, S = sum_i res(a[i]) and b -= S >> 1 (arithmetic
// shift, wrapping).  The mask words stay as they are; ms_center.cpp's ms_center_host is the word-for-word
// definition.
//
// k_ms_center.  One wave per row, four rows per 256-lane workgroup.  In round r lane l takes the mask words
// w = 128 r + 2 l and w + 1 with one 16-byte load: consecutive lanes read consecutive 16 bytes, a wave's load
// covers 1 KB (n = 834: seven rounds, the last half full; n = 2048: sixteen).  An odd n leaves one word, read
// alone.  The loads of eight rounds are issued together before the first is used.  The 64 partial sums meet in six
// exchange steps over the lanes (integer addition is associative and commutative: any order gives the same
// word), then lane 0 writes the body with one ordinary 8-byte store.  No LDS, no barrier, no atomics.  The
// kernel reads words 0 .. n of a row and writes word n: the padding up to the stride is neither read nor
// written, so rows of any stride >= n + 1 work (8-byte alignment is all the loads ask for).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace fhe {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
// a row of stride n + 1 is only 8-byte aligned
typedef __attribute__((address_space(1))) u32x4 g_u32x4_a8 __attribute__((aligned(8)));
typedef __attribute__((address_space(1))) uint64_t g_u64;

constexpr uint64_t kHalf = 1ull << 51;          // half a step of the 2^52 grid (log2(2N) = 12 bits kept)
constexpr uint64_t kResMask = (1ull << 52) - 1;

__device__ __forceinline__ int64_t ms_res(uint64_t x) { return (int64_t)((x + kHalf) & kResMask) - (int64_t)kHalf; }

__global__ __launch_bounds__(256) void k_ms_center(uint64_t* rows, uint32_t count, uint32_t n, size_t stride) {
    const uint32_t lane = threadIdx.x & 63u;
    const size_t row = (size_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (row >= count) return;  // wave-uniform
    g_u64* a = (g_u64*)(rows + row * stride);
    const uint64_t b = lane == 0 ? a[n] : 0ull;
    int64_t acc = 0;
    // eight rounds (1024 words) at a time, their loads issued before the first is used: one trip to memory
    // for n <= 1024, two up to 2048; a lane past the end holds zeros, whose residue is zero
    for (uint32_t base = 0; base < n; base += 1024u) {  // wave-uniform
        u32x4 v[8];
#pragma unroll
        for (uint32_t k = 0; k < 8; ++k) {
            const uint32_t w = base + 128u * k + 2u * lane;
            v[k] = u32x4{0, 0, 0, 0};
            if (w + 1u < n) v[k] = *(const g_u32x4_a8*)(a + w);
        }
#pragma unroll
        for (uint32_t k = 0; k < 8; ++k)
            acc += ms_res((uint64_t)v[k].x | ((uint64_t)v[k].y << 32)) + ms_res((uint64_t)v[k].z | ((uint64_t)v[k].w << 32));
    }
    if ((n & 1u) && lane == ((n - 1u) >> 1 & 63u)) acc += ms_res(a[n - 1u]);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor((long long)acc, m, 64);
    if (lane == 0) a[n] = b - (uint64_t)(acc >> 1);
}

}  // namespace

hipError_t launch_ms_center(uint64_t* rows, size_t count, uint32_t n, size_t stride, hipStream_t s) {
    if (count == 0) return hipSuccess;
    k_ms_center<<<(uint32_t)((count + 3) / 4), 256, 0, s>>>(rows, (uint32_t)count, n, stride);
    return hipGetLastError();
}

}  // namespace fhe
