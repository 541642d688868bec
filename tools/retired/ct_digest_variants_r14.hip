// RETIRED (r14): k_ct_digest with both ways of loading a row, as measured for profiles/r14/ct_digest_timing_r14.txt.
// csrc/ct_digest.hip keeps the direct variant only: the tile variant was 2 % faster at 128 blocks (every run below
// every run of the other) and within the spread at 4096, so DESIGN.md 5's rule did not adopt it.  This file is a
// record, not built: it needs the launch_ct_digest(..., bool tile, ...) declaration it was measured with.
//
// ct_digest.hip -- SHA-256 digests of big LWE ciphertexts where they live (ct_digest.h): 32 bytes per
// block cross the bus instead of 16 KB.  Word for word what ct_digest.cpp's ct_digest_host computes.
//
// k_ct_digest.  One wave per row, one row per workgroup.  A row digest is a tree of tagged hashes, each 5
// compressions after its tag's midstate: lane j hashes leaf j (row bytes [256 j, 256 j + 256)), so the 64 leaves
// fill the wave exactly; the 64 leaf digests go through 2 KB of LDS; lanes 0 .. 7 hash the 8 nodes (8 leaf
// digests each), lane 0 the root (8 node digests and the body) and stores it.  The serial depth is 15
// compressions whatever the lane count, so the three levels run through ONE copy of the compression (a loop over
// the level, a loop over the level's 5 blocks): in the node and root levels every lane computes (lane & 7's node,
// the root) rather than diverge, and only the owners store.  The compression is 32-bit integer VALU work: 64
// rounds fully unrolled, the message schedule a rolling window of 16 registers, rotates by v_alignbit, the round
// constants literals, the three midstates kernel arguments (scalar registers).  SHA-256's message words are
// big-endian: every loaded dword is byte-swapped (v_perm), a digest is kept as its 8 state words, which are the
// message words of the level above, and swapped once more only when the root is stored.  The next block's words
// are fetched before the current block is compressed.
//
// Two ways to bring a row in (fhe_ctx_set_ct_digest_load; DESIGN.md 6h records both):
//   direct  lane j loads its own 256 contiguous bytes, four dwordx4 per block: a wave's load touches 64 cache
//           lines and relies on L1 / L2 for the other three quarters of each line;
//   tile    the wave loads the row by 16 coalesced dwordx4 (1 KB each) into an LDS tile of 64 leaves at a
//           stride of 65 dwords, so that lane j's reads of its leaf meet no bank conflict (16,640 bytes).
// A trivial block (null source) is the row (0, body): its mask words are zeros, never loaded.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ct_digest.h"

namespace fhe {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
// a slot is only 8-byte aligned; the slot pointers are loaded from memory, so the compiler cannot prove
// them global and would emit flat accesses: say so
typedef __attribute__((address_space(1))) u32x4 g_u32x4_a8 __attribute__((aligned(8)));
typedef __attribute__((address_space(1))) u32x4 g_u32x4;
typedef __attribute__((address_space(1))) uint8_t g_u8;
typedef __attribute__((address_space(1))) uint64_t g_u64;

constexpr uint32_t kN = 2048;
constexpr uint32_t kLeafDwords = 64;    // 256 bytes
constexpr uint32_t kTileStride = 65;    // dwords per leaf in the LDS tile: lane j's dword i sits in bank (j + i) mod 64
constexpr uint32_t kLeafBits = (64 + 256) * 8;      // T || T || 256 bytes
constexpr uint32_t kRowBits = (64 + 256 + 8) * 8;   // T || T || 8 node digests || the body

__device__ constexpr uint32_t kK[64] = {
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5,
    0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174,
    0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
    0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967,
    0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
    0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
    0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3,
    0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};

__device__ __forceinline__ uint32_t rotr(uint32_t x, uint32_t n) { return __builtin_amdgcn_alignbit(x, x, n); }

// one compression: st += F(st, w); w is consumed (the schedule rolls through it)
__device__ __forceinline__ void sha256_compress(uint32_t (&st)[8], uint32_t (&w)[16]) {
    uint32_t v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = st[i];
#pragma unroll
    for (int i = 0; i < 64; ++i) {
        if (i >= 16) {
            const uint32_t w15 = w[(i + 1) & 15], w2 = w[(i + 14) & 15];
            w[i & 15] += (rotr(w15, 7) ^ rotr(w15, 18) ^ (w15 >> 3)) + w[(i + 9) & 15] + (rotr(w2, 17) ^ rotr(w2, 19) ^ (w2 >> 10));
        }
        // the eight working variables rotate by renaming: a is v[-i mod 8]
        const uint32_t a = v[(64 - i) & 7], b = v[(65 - i) & 7], c = v[(66 - i) & 7];
        const uint32_t e = v[(68 - i) & 7], f = v[(69 - i) & 7], g = v[(70 - i) & 7];
        const uint32_t t1 = v[(71 - i) & 7] + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + (g ^ (e & (f ^ g))) + kK[i] + w[i & 15];
        const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) | (c & (a | b)));
        v[(67 - i) & 7] += t1;
        v[(71 - i) & 7] = t1 + t2;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) st[i] += v[i];
}

__device__ __forceinline__ void put_swapped(uint32_t (&m)[16], int at, u32x4 x) {
    m[at] = __builtin_bswap32(x.x);
    m[at + 1] = __builtin_bswap32(x.y);
    m[at + 2] = __builtin_bswap32(x.z);
    m[at + 3] = __builtin_bswap32(x.w);
}

template <bool kTile>
__global__ __launch_bounds__(64) void k_ct_digest(const CtDigestEntry* __restrict__ entries, uint8_t* __restrict__ out,
                                                  CtDigestMidstates mid) {
    __shared__ uint32_t leaf[64 * 8];  // the 64 leaf digests, as state words
    __shared__ uint32_t node[8 * 8];
    __shared__ uint32_t tile[kTile ? 64 * kTileStride : 1];
    const uint32_t lane = threadIdx.x;
    const CtDigestEntry ent = entries[blockIdx.x];
    const g_u8* row = (const g_u8*)ent.src;
    const uint64_t body = row ? ((const g_u64*)ent.src)[kN] : ent.tbody;

    if (kTile) {
        // 16 coalesced loads of 1 KB; 16-byte unit u holds dwords 4 u .. 4 u + 3 of leaf u / 16
        u32x4 x[16] = {};
        if (row) {
#pragma unroll
            for (uint32_t k = 0; k < 16; ++k) x[k] = *(const g_u32x4_a8*)(row + (k * 64u + lane) * 16u);
        }
#pragma unroll
        for (uint32_t k = 0; k < 16; ++k) {
            const uint32_t u = k * 64u + lane;
            uint32_t* t = tile + (u >> 4) * kTileStride + (u & 15u) * 4u;
            t[0] = x[k].x;
            t[1] = x[k].y;
            t[2] = x[k].z;
            t[3] = x[k].w;
        }
        __syncthreads();
    }

    // the 16 message words of block b of the level: blocks 0 .. 3 are data, block 4 the padding (and the body)
    auto fetch = [&](uint32_t level, uint32_t b, uint32_t (&m)[16]) {
        if (b == 4) {
#pragma unroll
            for (int i = 0; i < 15; ++i) m[i] = 0;
            if (level == 2) {
                m[0] = __builtin_bswap32((uint32_t)body);
                m[1] = __builtin_bswap32((uint32_t)(body >> 32));
                m[2] = 0x80000000u;
                m[15] = kRowBits;
            } else {
                m[0] = 0x80000000u;
                m[15] = kLeafBits;
            }
        } else if (level == 0) {
            if (kTile) {
                const uint32_t* t = tile + lane * kTileStride + 16u * b;
#pragma unroll
                for (int i = 0; i < 16; ++i) m[i] = __builtin_bswap32(t[i]);
            } else {
                u32x4 x[4] = {};
                if (row) {
                    const g_u8* p = row + lane * (kLeafDwords * 4u) + b * 64u;
#pragma unroll
                    for (uint32_t q = 0; q < 4; ++q) x[q] = *(const g_u32x4_a8*)(p + q * 16u);
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) put_swapped(m, 4 * q, x[q]);
            }
        } else {
            // node g = lane & 7: leaf digests 8 g + 2 b and + 1; the root: node digests 2 b and + 1
            const uint32_t* s = level == 1 ? leaf + (8u * (lane & 7u) + 2u * b) * 8u : node + 16u * b;
#pragma unroll
            for (int i = 0; i < 16; ++i) m[i] = s[i];
        }
    };

#pragma unroll 1
    for (uint32_t level = 0; level < 3; ++level) {
        uint32_t st[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) st[i] = level == 0 ? mid.leaf[i] : level == 1 ? mid.node[i] : mid.row[i];
        uint32_t next[16];
        fetch(level, 0, next);
#pragma unroll 1
        for (uint32_t b = 0; b < 5; ++b) {
            uint32_t m[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) m[i] = next[i];
            if (b < 4) fetch(level, b + 1, next);
            sha256_compress(st, m);
        }
        if (level == 0) {
#pragma unroll
            for (int i = 0; i < 8; ++i) leaf[lane * 8u + i] = st[i];
        } else if (level == 1) {
            if (lane < 8) {
#pragma unroll
                for (int i = 0; i < 8; ++i) node[lane * 8u + i] = st[i];
            }
        } else if (lane == 0) {
            g_u32x4* o = (g_u32x4*)(out + (size_t)blockIdx.x * 32u);
            u32x4 lo, hi;
            lo.x = __builtin_bswap32(st[0]);
            lo.y = __builtin_bswap32(st[1]);
            lo.z = __builtin_bswap32(st[2]);
            lo.w = __builtin_bswap32(st[3]);
            hi.x = __builtin_bswap32(st[4]);
            hi.y = __builtin_bswap32(st[5]);
            hi.z = __builtin_bswap32(st[6]);
            hi.w = __builtin_bswap32(st[7]);
            o[0] = lo;
            o[1] = hi;
        }
        __syncthreads();
    }
}

}  // namespace

hipError_t launch_ct_digest(const CtDigestEntry* entries, uint8_t* out, uint32_t nblocks, const CtDigestMidstates& mid, bool tile,
                            hipStream_t s) {
    if (nblocks == 0) return hipSuccess;
    if (tile)
        k_ct_digest<true><<<nblocks, 64, 0, s>>>(entries, out, mid);
    else
        k_ct_digest<false><<<nblocks, 64, 0, s>>>(entries, out, mid);
    return hipGetLastError();
}

}  // namespace fhe
