// rerandomize.hip -- re-randomization of ciphertexts under the compact public key (public_key.h).
//
// k_rerand_zero makes the zero encryptions (Z_A, Z_B) of every chunk; k_rerand_add adds their sample
// extractions to the source blocks and writes fresh slots -- word for word what rerandomize.cpp's
// rerandomize_host computes.  Exact integers only: no FFT, no floating point.
//
// k_rerand_zero.  Grid (segment, polynomial, chunk), 256 lanes; a workgroup owns the 64 outputs j = 64 segment
// + lane of P R (P = A or B) of one chunk, and its four waves a quarter of R's bits each.  The product with the
// binary R is a sum of rotated, sign-flipped copies of P: out[j] = sum_i R_i (i <= j ? P[j - i] : -P[j - i + N]).
// P is staged in LDS as the 2 N-word table ext = [-P | P], which turns both cases into the one read
// ext[j - i + N] (32 KB); R's 32 words, the segment's 64 noise words and the waves' partial sums sit next to it
// (35,584 bytes in all).  In step i lane l reads ext[j_l - i + N]: consecutive lanes read consecutive 8-byte
// words, a wave's ds_read_b64 covers 512 contiguous bytes and meets no bank conflict.  Bit i is the same for
// every lane: R's word is made wave-uniform (readfirstlane) and the bit becomes a mask, so every step is one LDS
// read, one AND and one 64-bit add whatever R is -- no branch, no divergence, and a running time that does not
// depend on the secret R.  The reads of 32 steps are issued together before the first is used (two
// accumulators), so the loop waits for LDS once per 32 steps, not once per step; with 64 workgroups of four
// waves per chunk a wave runs 512 steps.  Wave 0 adds the four partial sums and the noise.  Randomness: R is
// ChaCha blocks 4 c .. 4 c + 3 of the binary stream, the segment's noise 8 consecutive blocks of the noise
// stream; lanes 0 .. 7 of the first wave compute one noise block each and lanes 8 .. 11 one block of R, into
// LDS, so no lane computes 64 bytes to use 8.
//
// k_rerand_add.  k_compact_extract's access pattern (public_key.hip) with one more operand: one 256-lane
// workgroup per block; in round s lane l handles mask words u = 512 s + 2 l and u + 1: one dwordx4 load from the
// source slot (nothing for a trivial block, whose mask is zero), the reversed pair Z_A[(t - u) mod N],
// Z_A[(t - u - 1) mod N] negated where the index wrapped, two 64-bit adds, one dwordx4 store to the fresh slot.
// Lane 0 writes the body.  Read-modify-write bound: 16 KB in, 16 KB out per block; a chunk's Z_A (16 KB) is
// read by all of the chunk's workgroups and stays in L2.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "chacha_device.h"
#include "keygen.h"

namespace fhe {

namespace {

// a slot is only 8-byte aligned; the slot pointers are loaded from memory, so the compiler cannot prove
// them global and would emit flat accesses: say so
typedef __attribute__((address_space(1))) u32x4 g_u32x4_a8 __attribute__((aligned(8)));
typedef __attribute__((address_space(1))) uint8_t g_u8;
typedef __attribute__((address_space(1))) uint64_t g_u64;

constexpr uint32_t kN = 2048;
constexpr uint32_t kSegment = 64;  // outputs per workgroup of k_rerand_zero: one per lane, the waves split the bits

// keys.cpp tuniform_of on a raw stream word
__device__ __forceinline__ uint64_t tuniform_word(uint64_t x, uint32_t b) {
    const uint64_t u = x & ((1ull << (b + 1)) - 1);
    const uint64_t c = (x >> (b + 1)) & 1ull;
    return u + c - (1ull << b);
}

// ab: the public key's A then B (kN words each).  z: per chunk Z_A then Z_B (kN words each); Z_B[j] carries
// its noise for the used j < min(kN, nblocks - kN chunk) only (the others are never read).
__global__ __launch_bounds__(256) void k_rerand_zero(ChaChaKey kbin, ChaChaKey knoise, const uint64_t* __restrict__ ab,
                                                     uint64_t* __restrict__ z, uint32_t nblocks, uint32_t noise_log2) {
    __shared__ uint64_t ext[2 * kN];
    __shared__ uint64_t rw[kN / 64];
    __shared__ uint64_t noise[kSegment];
    __shared__ uint64_t part[4][kSegment];
    const uint32_t seg = blockIdx.x, poly = blockIdx.y, c = blockIdx.z, tid = threadIdx.x;
    const uint32_t q = tid >> 6, lane = tid & 63;
    const uint64_t* __restrict__ P = ab + poly * kN;
    for (uint32_t m = tid; m < kN; m += 256) {
        const uint64_t v = P[m];
        ext[m] = 0 - v;
        ext[kN + m] = v;
    }
    if (tid < 12) {
        const bool is_r = tid >= 8;
        ChaChaKey k;
#pragma unroll
        for (int i = 0; i < 8; ++i) k.key[i] = is_r ? kbin.key[i] : knoise.key[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) k.nonce[i] = is_r ? kbin.nonce[i] : knoise.nonce[i];
        // R: u64 words [32 c, 32 c + 32) = blocks 4 c ..; noise: u64 words 4096 c + 2048 poly + 64 seg + ..
        const uint32_t counter = is_r ? 4u * c + (tid - 8u) : 512u * c + 256u * poly + 8u * seg + tid;
        uint32_t o[16];
        chacha_block(k, counter, o);
        uint64_t* dst = is_r ? rw + 8u * (tid - 8u) : noise + 8u * tid;
#pragma unroll
        for (int w = 0; w < 8; ++w) dst[w] = (uint64_t)o[2 * w] | ((uint64_t)o[2 * w + 1] << 32);
    }
    __syncthreads();
    const uint32_t j = seg * kSegment + lane;
    // wave q takes bits [512 q, 512 q + 512): e[-i'] = the term of bit 512 q + i'
    const uint64_t* __restrict__ e = ext + j + kN - 512u * q;
    uint64_t acc0 = 0, acc1 = 0;
    for (uint32_t w = 0; w < 8; ++w) {
        const uint64_t r = rw[8u * q + w];
        const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)r);
        const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(r >> 32));
        const uint64_t* __restrict__ ew = e - 64 * (int)w;
        uint64_t v[32];
#pragma unroll
        for (int b = 0; b < 32; ++b) v[b] = ew[-b];
#pragma unroll
        for (int b = 0; b < 32; b += 2) {
            acc0 += v[b] & (0ull - (uint64_t)((lo >> b) & 1u));
            acc1 += v[b + 1] & (0ull - (uint64_t)((lo >> (b + 1)) & 1u));
        }
#pragma unroll
        for (int b = 0; b < 32; ++b) v[b] = ew[-32 - b];
#pragma unroll
        for (int b = 0; b < 32; b += 2) {
            acc0 += v[b] & (0ull - (uint64_t)((hi >> b) & 1u));
            acc1 += v[b + 1] & (0ull - (uint64_t)((hi >> (b + 1)) & 1u));
        }
    }
    part[q][lane] = acc0 + acc1;
    __syncthreads();
    if (q == 0) {
        const uint32_t used = min(kN, nblocks - c * kN);
        const uint64_t e0 = (poly == 0 || j < used) ? tuniform_word(noise[lane], noise_log2) : 0ull;
        z[((size_t)c * 2 + poly) * kN + j] = e0 + part[0][lane] + part[1][lane] + part[2][lane] + part[3][lane];
    }
}

// z: k_rerand_zero's output; src[i]: the source slot of block i, or null for a trivial block, whose body is
// tbody[i]; dst[i]: the fresh slot
__global__ __launch_bounds__(256) void k_rerand_add(const uint64_t* __restrict__ z, const uint64_t* const* __restrict__ src,
                                                    const uint64_t* __restrict__ tbody, uint64_t* const* __restrict__ dst) {
    const uint32_t i = blockIdx.x, t = i & (kN - 1);
    const uint64_t* __restrict__ ZA = z + (size_t)(i / kN) * 2 * kN;
    const uint64_t* in = src[i];
    uint64_t* slot = dst[i];
    const g_u8* ibase = (const g_u8*)in + threadIdx.x * 16u;
    g_u8* obase = (g_u8*)slot + threadIdx.x * 16u;
    // the slot is fresh and never the source: all loads first, so that the stores do not fence them
    u32x4 x[4] = {};
    if (in) {
#pragma unroll
        for (uint32_t s = 0; s < 4; ++s) x[s] = *(const g_u32x4_a8*)(ibase + s * 4096u);
    }
    uint64_t a[4][2];
#pragma unroll
    for (uint32_t s = 0; s < 4; ++s) {
        const uint32_t u = 512u * s + 2u * threadIdx.x;
        a[s][0] = ZA[(t - u) & (kN - 1)];
        a[s][1] = ZA[(t - u - 1u) & (kN - 1)];
    }
#pragma unroll
    for (uint32_t s = 0; s < 4; ++s) {
        const uint32_t u = 512u * s + 2u * threadIdx.x;
        uint64_t a0 = a[s][0], a1 = a[s][1];
        if (u > t) a0 = 0 - a0;
        if (u + 1 > t) a1 = 0 - a1;
        a0 += (uint64_t)x[s].x | ((uint64_t)x[s].y << 32);
        a1 += (uint64_t)x[s].z | ((uint64_t)x[s].w << 32);
        u32x4 w;
        w.x = (uint32_t)a0;
        w.y = (uint32_t)(a0 >> 32);
        w.z = (uint32_t)a1;
        w.w = (uint32_t)(a1 >> 32);
        *(g_u32x4_a8*)(obase + s * 4096u) = w;
    }
    if (threadIdx.x == 0) ((g_u64*)slot)[kN] = (in ? ((const g_u64*)in)[kN] : tbody[i]) + ZA[kN + t];
}

}  // namespace

hipError_t launch_rerand_zero(const ChaChaKey& kbin, const ChaChaKey& knoise, const uint64_t* ab, uint64_t* z, uint32_t nblocks,
                              uint32_t noise_log2, hipStream_t s) {
    if (nblocks == 0) return hipSuccess;
    const uint32_t chunks = (nblocks + kN - 1) / kN;
    k_rerand_zero<<<dim3(kN / kSegment, 2, chunks), 256, 0, s>>>(kbin, knoise, ab, z, nblocks, noise_log2);
    return hipGetLastError();
}

hipError_t launch_rerand_add(const uint64_t* z, const uint64_t* const* src, const uint64_t* tbody, uint64_t* const* dst,
                             uint32_t nblocks, hipStream_t s) {
    if (nblocks == 0) return hipSuccess;
    k_rerand_add<<<nblocks, 256, 0, s>>>(z, src, tbody, dst);
    return hipGetLastError();
}

}  // namespace fhe
