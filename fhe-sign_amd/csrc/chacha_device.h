// chacha_device.h -- the ChaCha20 block function (RFC 8439) on the device, shared by the key
// generation stream kernel (keygen.hip) and the seeded-ciphertext expansion (seeded.hip).
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

}  // namespace fhe
