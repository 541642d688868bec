// chacha_device.h -- the ChaCha20 block function (RFC 8439) on the device, shared by the key
// generation stream kernel (keygen.hip), the seeded-ciphertext expansion (seeded.hip), the seeded server
// key's install (seeded_key.hip), the seeded compression key's (seeded_compression.hip) and the rows of the
// oblivious pseudo-random values (oprf.hip); seeded.hip, seeded_key.hip and oprf.hip also share the quad
// exchange for coalesced stores.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "keygen.h"

namespace fhe {

__device__ __forceinline__ uint32_t rotl32(uint32_t v, int c) { return (v << c) | (v >> (32 - c)); }
__device__ __forceinline__ void qr(uint32_t& a, uint32_t& b, uint32_t& c, uint32_t& d) {
    a += b; d ^= a; d = rotl32(d, 16);
    c += d; b ^= c; b = rotl32(b, 12);
    a += b; d ^= a; d = rotl32(d, 8);
    c += d; b ^= c; b = rotl32(b, 7);
}

// o[0..16) = the 32-bit output words of block `counter` (RFC 8439 layout as keys.cpp
// ChaChaStream::refill); u64 word w of the block = o[2 w] | o[2 w + 1] << 32, which in little-endian
// memory is o[] itself
__device__ __forceinline__ void chacha_block(const ChaChaKey& k, uint32_t counter, uint32_t o[16]) {
    const uint32_t s[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u,
                            k.key[0], k.key[1], k.key[2], k.key[3], k.key[4], k.key[5], k.key[6], k.key[7],
                            counter, k.nonce[0], k.nonce[1], k.nonce[2]};
    uint32_t x[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) x[i] = s[i];
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        qr(x[0], x[4], x[8], x[12]);
        qr(x[1], x[5], x[9], x[13]);
        qr(x[2], x[6], x[10], x[14]);
        qr(x[3], x[7], x[11], x[15]);
        qr(x[0], x[5], x[10], x[15]);
        qr(x[1], x[6], x[11], x[12]);
        qr(x[2], x[7], x[8], x[13]);
        qr(x[3], x[4], x[9], x[14]);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) o[i] = x[i] + s[i];
}

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t sel4(uint32_t i, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    const uint32_t lo = (i & 1) ? b : a, hi = (i & 1) ? d : c;
    return (i & 2) ? hi : lo;
}

// Quad exchange for coalesced stores of a wave's 64 consecutive ChaCha blocks (4 KB).  If every lane
// stored the block it computed, a store instruction would touch 64 cache lines with 16 bytes each.
// Instead the four lanes of a quad exchange quarters (a 4 x 4 transposition of 16-byte parts, three lane
// exchanges): with lane (quad q = lane >> 2, position p = lane & 3) holding block 16 p + q of the 64 in
// o[], w[s] becomes bytes [1024 s + 16 lane, + 16) of the 4 KB -- store s of every lane together covers
// 1 KB without a gap, consecutive lanes consecutive 16-byte parts.
__device__ __forceinline__ void chacha_quad_exchange(const uint32_t o[16], uint32_t p, u32x4 w[4]) {
    // y[r] = part p (words 4 p .. 4 p + 3) of the block held by quad position p ^ r
    uint32_t y[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const uint32_t j = p ^ r;  // the part the partner needs from this lane
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t v = sel4(j, o[i], o[4 + i], o[8 + i], o[12 + i]);
            y[r][i] = r ? (uint32_t)__shfl_xor((int)v, r, 4) : v;
        }
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {  // store s: the block of quad position s = y[p ^ s]
        const uint32_t r = p ^ (uint32_t)s;
        w[s].x = sel4(r, y[0][0], y[1][0], y[2][0], y[3][0]);
        w[s].y = sel4(r, y[0][1], y[1][1], y[2][1], y[3][1]);
        w[s].z = sel4(r, y[0][2], y[1][2], y[2][2], y[3][2]);
        w[s].w = sel4(r, y[0][3], y[1][3], y[2][3], y[3][3]);
    }
}

}  // namespace fhe
