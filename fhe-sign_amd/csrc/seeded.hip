// seeded.hip -- expansion of a seeded (compressed) ciphertext on the GPU.
//
// A seeded object carries a public 32-byte mask seed and one body word per radix block
// (keys.cpp:encrypt_seeded).  Block b's 2048 mask words are u64 words [2048 b, 2048 b + 2048) of the
// ChaCha20 stream keyed by the seed (stream id kStreamSeededMask), i.e. ChaCha blocks 256 b .. 256 b + 255;
// this kernel regenerates them into the block's device slot and appends the body -- word for word what
// keys.cpp:expand_seeded_host writes.
//
// Work unit = one ChaCha block = 64 contiguous bytes of a slot.  One 256-lane workgroup fills one slot
// (256 units), each wave 64 consecutive units = 4 KB.  A lane computes a whole block in registers; if
// it stored its own 64 bytes, every store instruction would touch 64 different cache lines with 16
// bytes each.  Instead the four lanes of a quad exchange quarters (4 x 4 transposition of 16-byte
// parts, three lane exchanges), and in store k lane l writes bytes [1024 k + 16 l, + 16) of the wave's
// 4 KB: every store is a dwordx4 and a wave's store covers 1 KB without a gap.  For that, lane
// (quad q, position p) computes unit 16 p + q of the wave, so that store k holds the units 16 k .. 16 k + 15.
// The kernel is store-bound (16 KB per slot); slots are 8-byte aligned (2049 words each), which global
// dwordx4 stores accept.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "chacha_device.h"
#include "keygen.h"

namespace fhe {

namespace {

// a slot is only 8-byte aligned; the slot pointers are loaded from memory, so the compiler cannot prove
// them global and would emit flat stores: say so
typedef __attribute__((address_space(1))) u32x4 g_u32x4_a8 __attribute__((aligned(8)));
typedef __attribute__((address_space(1))) uint8_t g_u8;
typedef __attribute__((address_space(1))) uint64_t g_u64;

__global__ __launch_bounds__(256) void k_expand_seeded(ChaChaKey k, uint64_t* const* __restrict__ dst,
                                                       const uint64_t* __restrict__ bodies) {
    const uint32_t b = blockIdx.x;
    uint64_t* __restrict__ slot = dst[b];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t p = lane & 3, q = lane >> 2;
    uint32_t o[16];
    chacha_block(k, b * 256u + wave * 64u + p * 16u + q, o);
    u32x4 w[4];
    chacha_quad_exchange(o, p, w);
    g_u8* base = (g_u8*)slot + wave * 4096u + lane * 16u;
#pragma unroll
    for (int s = 0; s < 4; ++s) *(g_u32x4_a8*)(base + s * 1024) = w[s];
    if (threadIdx.x == 0) ((g_u64*)slot)[2048] = bodies[b];
}

}  // namespace

hipError_t launch_expand_seeded(const ChaChaKey& k, uint64_t* const* dst, const uint64_t* bodies, int nblocks,
                                hipStream_t s) {
    if (nblocks <= 0) return hipSuccess;
    k_expand_seeded<<<nblocks, 256, 0, s>>>(k, dst, bodies);
    return hipGetLastError();
}

}  // namespace fhe
