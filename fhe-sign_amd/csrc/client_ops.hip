// client_ops.hip -- encryption and the decryption phase under a client key resident on the device.
//
// The resident buffer holds the big secret key as 2048 packed bits (64 u32 words) and, behind them, the
// encryption stream's parameters of the current call (client_ops_index.h: StreamParams).  Both kernels read it
// through a pointer: no secret is a launch argument.
//
// k_client_encrypt -- word for word keys.cpp:encrypt_big_many.  One 256-lane workgroup per row.  A row is 257
// ChaCha blocks ("units") of ck->enc_rng, and it starts off = (W0 + i) mod 8 words into the first
// (client_ops_index.h).  Lane (quad q, position p) of wave v computes unit t = 64 v + 16 p + q in registers, as
// seeded.hip's k_expand_seeded does; the quad exchange then makes every store a dwordx4 with consecutive lanes on
// consecutive 16 bytes, at byte 64 t - 8 off of the slot -- the whole pattern shifted down by 8 off bytes, which
// 8-byte-aligned slots accept like any other.  Two units are not whole mask words:
//   unit 0 (off > 0): its first `off` words are the previous row's.  Its lane stores the 8 - off others one by one,
//       and the quad's four parts of store 0 are skipped;
//   unit 256: `off` mask words, the noise word, then the next row's.  Wave 0 computes it once more than its 64 units
//       (every lane the same block: no divergence); lane 0 stores the mask words and keeps the noise word.
// Before the exchange a lane holds 8 whole u64 words whose row indices are 8 t - off + w: it adds those whose key
// bit is set (the key is binary: a mask, no multiply) -- key_bits8 gives zero for indices outside [0, 2048), so
// the straddling units need no case of their own.  The 64-bit partial sums meet by six lane exchanges per wave
// (ms_center.hip) and 32 bytes of LDS across the four waves; thread 0 writes body = sum + plaintext + noise.
//
// k_client_phase -- word for word keys.cpp:decrypt_phase_big.  One wave per block, four per workgroup, the rows
// read through the slot-pointer table with 16-byte loads (lane l of round r takes words 128 r + 2 l, + 1), the
// masked sum, six lane exchanges, phase = body - sum as one u64 per block.  No LDS.
//
// Bounds: the vector stores cover row words [8 - off, 2048 - off) for units 1 .. 255, the single stores words
// [0, 8 - off) and [2048 - off, 2048], nothing else: every write lies inside the slot's 2049 words.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "chacha_device.h"
#include "client_ops.h"
#include "client_ops_index.h"

namespace fhe {

namespace {

using namespace client_ops;

// slots are only 8-byte aligned, and their pointers are loaded from memory: say that they are global
typedef __attribute__((address_space(1))) u32x4 g_u32x4_a8 __attribute__((aligned(8)));
typedef __attribute__((address_space(1))) uint8_t g_u8;
typedef __attribute__((address_space(1))) uint64_t g_u64;

__device__ __forceinline__ uint64_t word_of(const uint32_t o[16], int w) { return (uint64_t)o[2 * w] | (uint64_t)o[2 * w + 1] << 32; }

// sum of the unit's words whose key bit is set; bits = key_bits8 at the unit's first row word
__device__ __forceinline__ uint64_t masked_sum(const uint32_t o[16], uint32_t bits) {
    uint64_t acc = 0;
#pragma unroll
    for (int w = 0; w < 8; ++w) acc += word_of(o, w) & (0ull - (uint64_t)((bits >> w) & 1u));
    return acc;
}

__global__ __launch_bounds__(256) void k_client_encrypt(const uint32_t* __restrict__ client, uint64_t* const* __restrict__ dst,
                                                        const uint64_t* __restrict__ pts) {
    __shared__ uint64_t wave_sum[4];
    const uint32_t* __restrict__ kb = client;
    const StreamParams* __restrict__ sp = (const StreamParams*)(client + kKeyWords);
    ChaChaKey k;
#pragma unroll
    for (int i = 0; i < 8; ++i) k.key[i] = sp->key[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) k.nonce[i] = sp->nonce[i];
    const uint32_t b = blockIdx.x;
    const uint64_t g = row_first_word((uint64_t)sp->w0_lo | (uint64_t)sp->w0_hi << 32, b);
    const uint32_t unit0 = row_first_unit(g), off = row_offset(g);
    g_u64* slot = (g_u64*)dst[b];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t p = lane & 3, q = lane >> 2;
    const uint32_t t = wave * 64u + p * 16u + q;
    uint32_t o[16];
    chacha_block(k, unit0 + t, o);
    uint64_t acc = masked_sum(o, key_bits8(kb, unit_row_word(t, off)));
    if (threadIdx.x == 0 && off) {  // unit 0 of a row that starts inside it: words off .. 7 are row words 0 ..
#pragma unroll
        for (int w = 1; w < 8; ++w)
            if ((uint32_t)w >= off) slot[(uint32_t)w - off] = word_of(o, w);
    }
    u32x4 v[4];
    chacha_quad_exchange(o, p, v);
    // byte 4096 wave + 1024 s + 16 lane of the units' bytes is slot byte that - 8 off; off > 0: store 0 of wave 0's
    // first quad is unit 0, written above
    g_u8* base = (g_u8*)slot + wave * 4096u + lane * 16u - 8u * off;
#pragma unroll
    for (int s = 0; s < 4; ++s)
        if (s || off == 0 || threadIdx.x >= 4) *(g_u32x4_a8*)(base + s * 1024) = v[s];
    uint64_t noise = 0;
    if (wave == 0) {  // wave-uniform: unit 256, the row's last `off` mask words and its noise word
        chacha_block(k, unit0 + 256u, o);
        if (lane == 0) {
            acc += masked_sum(o, key_bits8(kb, unit_row_word(256u, off)));
#pragma unroll
            for (int w = 0; w < 7; ++w)
                if ((uint32_t)w < off) slot[kMaskWords - off + (uint32_t)w] = word_of(o, w);
#pragma unroll
            for (int w = 0; w < 8; ++w)
                if ((uint32_t)w == off) noise = word_of(o, w);
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) acc += (uint64_t)__shfl_xor((long long)acc, m, 64);
    if (lane == 0) wave_sum[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0)
        slot[kMaskWords] = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3] + pts[b] + tuniform_word(noise, sp->noise_log2);
}

__global__ __launch_bounds__(256) void k_client_phase(const uint32_t* __restrict__ client, const uint64_t* const* __restrict__ src,
                                                      uint64_t* __restrict__ phases, uint32_t count) {
    const uint32_t lane = threadIdx.x & 63u;
    const size_t row = (size_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (row >= count) return;  // wave-uniform
    const g_u64* a = (const g_u64*)src[row];
    uint64_t acc = 0;
    // eight rounds (1024 words) at a time, their loads issued before the first is used (ms_center.hip)
    for (uint32_t base = 0; base < kMaskWords; base += 1024u) {
        u32x4 v[8];
#pragma unroll
        for (uint32_t r = 0; r < 8; ++r) v[r] = *(const g_u32x4_a8*)(a + base + 128u * r + 2u * lane);
#pragma unroll
        for (uint32_t r = 0; r < 8; ++r) {
            const uint32_t w = base + 128u * r + 2u * lane;  // even: both bits in one key word
            const uint32_t bits = client[w >> 5] >> (w & 31u);
            acc += ((uint64_t)v[r].x | (uint64_t)v[r].y << 32) & (0ull - (uint64_t)(bits & 1u));
            acc += ((uint64_t)v[r].z | (uint64_t)v[r].w << 32) & (0ull - (uint64_t)((bits >> 1) & 1u));
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) acc += (uint64_t)__shfl_xor((long long)acc, m, 64);
    if (lane == 0) phases[row] = a[kMaskWords] - acc;
}

}  // namespace

hipError_t launch_client_encrypt(const uint32_t* client, uint64_t* const* dst, const uint64_t* pts, size_t nblocks,
                                 hipStream_t s) {
    if (nblocks == 0) return hipSuccess;
    k_client_encrypt<<<(uint32_t)nblocks, 256, 0, s>>>(client, dst, pts);
    return hipGetLastError();
}

hipError_t launch_client_phase(const uint32_t* client, const uint64_t* const* src, uint64_t* phases, size_t nblocks,
                               hipStream_t s) {
    if (nblocks == 0) return hipSuccess;
    k_client_phase<<<(uint32_t)((nblocks + 3) / 4), 256, 0, s>>>(client, src, phases, (uint32_t)nblocks);
    return hipGetLastError();
}

}  // namespace fhe
