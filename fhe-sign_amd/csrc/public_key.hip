// public_key.hip -- expansion of a compact ciphertext list (public_key.h) on the GPU.
//
// A list's chunk is one GLWE (C_A, C_B) under the client's big key; coefficient t of it becomes a big LWE by
// sample extraction: mask word u = C_A[t - u] for u <= t, -C_A[t - u + N] for u > t, body C_B[t] -- word
// for word what public_key.cpp:expand_compact_host writes, and the convention of compress.hip's k_pk_unpack.
//
// One 256-lane workgroup fills one slot.  In round s lane l writes mask words u = 512 s + 2 l and u + 1 as
// one dwordx4, so a wave's store covers 1 KB without a gap and the workgroup's four rounds the slot's 16 KB.
// The two words are the reversed pair C_A[(t - u) mod N], C_A[(t - u - 1) mod N], negated where the index
// wrapped (u > t resp. u + 1 > t): two 8-byte loads whose addresses descend with the lane, so a wave reads
// 1 KB of the chunk, contiguous but for the wrap at t.  A chunk's C_A is 16 KB in the staging buffer and
// every workgroup of the chunk reads all of it: after the first one the reads hit L2.  No LDS: each word
// of C_A is read exactly once per slot, so staging it would only add a pass.  The kernel is store-bound
// (16 KB per slot) like k_expand_seeded; slots are 8-byte aligned (2049 words each), which global dwordx4
// stores accept.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "keygen.h"

namespace fhe {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
// a slot is only 8-byte aligned; the slot pointers are loaded from memory, so the compiler cannot prove
// them global and would emit flat stores: say so
typedef __attribute__((address_space(1))) u32x4 g_u32x4_a8 __attribute__((aligned(8)));
typedef __attribute__((address_space(1))) uint8_t g_u8;
typedef __attribute__((address_space(1))) uint64_t g_u64;

constexpr uint32_t kN = 2048;

// ca: the staged chunks' C_A (kN words each); cb[i], dst[i]: body and slot of output i, which is coefficient
// `first + i` counted from the first staged chunk's coefficient 0
__global__ __launch_bounds__(256) void k_compact_extract(const uint64_t* __restrict__ ca, const uint64_t* __restrict__ cb,
                                                         uint64_t* const* __restrict__ dst, uint32_t first) {
    const uint32_t i = blockIdx.x;
    const uint32_t g = first + i, t = g & (kN - 1);
    const uint64_t* __restrict__ A = ca + (size_t)(g / kN) * kN;
    uint64_t* __restrict__ slot = dst[i];
    g_u8* base = (g_u8*)slot + threadIdx.x * 16u;
#pragma unroll
    for (uint32_t s = 0; s < 4; ++s) {
        const uint32_t u = 512u * s + 2u * threadIdx.x;
        uint64_t a0 = A[(t - u) & (kN - 1)], a1 = A[(t - u - 1u) & (kN - 1)];
        if (u > t) a0 = 0 - a0;
        if (u + 1 > t) a1 = 0 - a1;
        u32x4 w;
        w.x = (uint32_t)a0;
        w.y = (uint32_t)(a0 >> 32);
        w.z = (uint32_t)a1;
        w.w = (uint32_t)(a1 >> 32);
        *(g_u32x4_a8*)(base + s * 4096u) = w;
    }
    if (threadIdx.x == 0) ((g_u64*)slot)[kN] = cb[i];
}

}  // namespace

hipError_t launch_compact_extract(const uint64_t* ca, const uint64_t* cb, uint64_t* const* dst, uint32_t first, int count,
                                  hipStream_t s) {
    if (count <= 0) return hipSuccess;
    k_compact_extract<<<count, 256, 0, s>>>(ca, cb, dst, first);
    return hipGetLastError();
}

}  // namespace fhe
