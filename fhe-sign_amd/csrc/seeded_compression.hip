// seeded_compression.hip -- installation of a seeded (compressed) compression key on the GPU.
//
// A seeded compression key carries a public 32-byte seed and the bodies only (compress.h
// fhe_seeded_compression_key).  The packing key's masks are the ChaCha20 stream kStreamSeededPksk under the
// seed, one row per 256 ChaCha blocks (2048 u64 words): row r = j ell + l, coefficient m of mask polynomial
// c < k' = u64 word 2048 r + c N' + m, that is column col = c N' + m < k' N' of the row = word col % 8 of
// ChaCha block 256 r + col / 8.
//   k_expand_pksk_planes  writes, byte for byte, what k_pksk_to_planes (compress.hip) writes from the host-
//                         expanded key: the int8 planes [8][column tiles of 16][KT = 32 ell][64 lanes][16].
//                         The u64 packing key never exists in device memory.
// (The decompression BSK goes through seeded_key.hip's k_expand_bsk_fourier unchanged.)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "chacha_device.h"
#include "compress_kernels.h"
#include "device_math.h"

namespace fhe {

namespace {
typedef int v4i __attribute__((ext_vector_type(4)));
// u64 words between two rows of the LDS tile: 16 columns + 1, so that the 64 rows do not all start on the
// same banks (16 words = 128 bytes is half the 256-byte bank period)
constexpr int PKX_STRIDE = 17;

// One wave per (column tile tt, k-tile kt).  First lane = row: lane i owns k = 64 kt + i (level k >> 11,
// big-key index j = k & 2047, key row r = j ell + level) and produces that row's 16 columns 16 tt .. 16 tt +
// 15 in two halves of 8.  k' N' and (k' + 1) N' are multiples of 8 (N' >= 8), so a half is of one kind: one
// ChaCha block (256 r + 2 tt + h) below k' N', 8 uploaded body words below cols, zeros in the padding of the
// last tile.  The 64 x 16 words cross an 8.5 KB LDS tile; then lane l owns column l & 15 for the 16 rows
// 16 (l >> 4) + jj, k_pksk_to_planes' fragment, and splits them into balanced bytes with its arithmetic.
__global__ __launch_bounds__(64) void k_expand_pksk_planes(ChaChaKey key, const uint64_t* __restrict__ bodies,
                                                           int ell, int Np, int kN, int cols, int tiles,
                                                           int8_t* __restrict__ planes) {
    __shared__ uint64_t tile[64 * PKX_STRIDE];
    const int KT = 32 * ell;
    const int tt = blockIdx.x / KT, kt = blockIdx.x % KT, lane = threadIdx.x;
    {
        const int k = 64 * kt + lane;
        const uint32_t r = (uint32_t)(k & 2047) * (uint32_t)ell + (uint32_t)(k >> 11);
        uint64_t* dst = tile + lane * PKX_STRIDE;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int c0 = 16 * tt + 8 * h;  // wave-uniform
            if (c0 < kN) {
                uint32_t o[16];
                chacha_block(key, r * 256u + (uint32_t)(c0 >> 3), o);
#pragma unroll
                for (int i = 0; i < 8; ++i) dst[8 * h + i] = (uint64_t)o[2 * i] | (uint64_t)o[2 * i + 1] << 32;
            } else if (c0 < cols) {
                const uint64_t* src = bodies + (size_t)r * Np + (c0 - kN);
#pragma unroll
                for (int i = 0; i < 8; ++i) dst[8 * h + i] = src[i];
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i) dst[8 * h + i] = 0ull;
            }
        }
    }
    wave_sync();
    const int c = lane & 15, g = lane >> 4;
    int8_t by[8][16];
#pragma unroll
    for (int jj = 0; jj < 16; ++jj) {
        uint64_t v = tile[(16 * g + jj) * PKX_STRIDE + c];
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            int s = (int)(v & 255u);
            if (s >= 128) s -= 256;
            by[b][jj] = (int8_t)s;
            v = (v - (uint64_t)(int64_t)s) >> 8;
        }
    }
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        v4i o;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            o[q] = (int)((uint32_t)(uint8_t)by[b][4 * q] | (uint32_t)(uint8_t)by[b][4 * q + 1] << 8 |
                         (uint32_t)(uint8_t)by[b][4 * q + 2] << 16 | (uint32_t)(uint8_t)by[b][4 * q + 3] << 24);
        *reinterpret_cast<v4i*>(planes + (size_t)b * tiles * KT * 1024 + (((size_t)tt * KT + kt) * 64 + lane) * 16) = o;
    }
}

}  // namespace

hipError_t launch_expand_pksk_planes(const ChaChaKey& key, const uint64_t* bodies, int ell, int k, int Np,
                                     int8_t* planes, hipStream_t s) {
    // the ranges CompParams::from_c admits: every row's masks fit its 2048-word stride, 256 r + 255 < 2^32
    if (ell < 1 || ell > 32 || k < 1 || Np < 8 || (Np & 7) || k * Np > 2048) return hipErrorInvalidValue;
    const int kN = k * Np, cols = kN + Np, tiles = pk_col_tiles(cols);
    hipLaunchKernelGGL(k_expand_pksk_planes, dim3(tiles * 32 * ell), dim3(64), 0, s, key, bodies, ell, Np, kN, cols,
                       tiles, planes);
    return hipGetLastError();
}

}  // namespace fhe
