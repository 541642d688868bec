// compress.hip -- device path of the compressed computed ciphertexts (compress.h).
//
// Compression, three kernels:
//   k_pk_digits   one workgroup per block: the balanced base-2^beta digits of the 2048 mask words, as the
//                 int8 fragments the contraction reads; the body word kept aside
//   k_pk_mfma     P = D (B x 2048 ell) . PKSK (2048 ell x (k' + 1) N') mod 2^64 on the matrix cores, as
//                 ks_mfma.hip contracts the keyswitch: the key as 8 balanced signed-byte planes, one
//                 v_mfma_i32_16x16x64_i8 per (plane, k-tile), int32 sums exact (|d| <= 64, |byte| <= 128,
//                 2048 ell <= 65536 terms with beta ell <= 32: below 2^27), recombined as sum_b S_b 256^b
//   k_pk_pack     one workgroup per (GLWE, polynomial): G = sum_t X^t T_t with T_t = (0, .., b_t) - P_t and
//                 the negacyclic sign, modswitch12, and the 12-bit stream written as 32-bit words
// Decompression: k_pk_unpack (12-bit stream -> one sample-extracted LWE row per block, every value << 52),
// then the existing blind rotate under the decompression key (context.cpp).
//
// Fragment layouts (k = level * 2048 + j, level-major; KT = 32 ell k-tiles of 64), as ks_mfma.hip:
//   planes  int8 [8 planes][column tiles of 16][KT][64 lanes][16]
//   digits  int8 [block tiles of 16][KT][64 lanes][16]
// lane l of a fragment holds row / column l & 15 and the 16 bytes k = 16 (l >> 4) + jj of the k-tile.
#include "compress_kernels.h"
#include "device_math.h"

namespace fhe {

namespace {
typedef int v4i __attribute__((ext_vector_type(4)));

FHE_DEV size_t pk_frag(size_t tile, int KT, int kt, int lane) { return ((tile * KT + kt) * 64 + lane) * 16; }
}  // namespace

// PKSK u64 [2048][ell][cols] -> balanced byte planes.  One thread per (column tile, k-tile, lane).
__global__ __launch_bounds__(64) void k_pksk_to_planes(const uint64_t* __restrict__ pksk, int ell, int cols, int tiles,
                                                       int8_t* __restrict__ planes) {
    const int KT = 32 * ell;
    const int tt = blockIdx.x / KT, kt = blockIdx.x % KT, lane = threadIdx.x;
    const int col = 16 * tt + (lane & 15);
    int8_t by[8][16];
#pragma unroll
    for (int jj = 0; jj < 16; ++jj) {
        const int k = 64 * kt + 16 * (lane >> 4) + jj;
        const int lvl = k >> 11, j = k & 2047;
        uint64_t v = col < cols ? pksk[((size_t)j * ell + lvl) * cols + col] : 0ull;
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
        *reinterpret_cast<v4i*>(planes + (size_t)b * tiles * KT * 1024 + pk_frag(tt, KT, kt, lane)) = o;
    }
}

// Block i = blockIdx.x, thread q: mask words j = 16 q .. 16 q + 15, every level.  The digits' closed form
// (tests/ks_ref.py digits, generalised): round to the top beta ell bits, add 2^(beta - 1) to every digit
// (`bias`: the carries of that sum are the balancing carries), take the base-2^beta digits, subtract
// 2^(beta - 1) again; the carry out of the top digit falls off.
__global__ __launch_bounds__(128) void k_pk_digits(const uint64_t* const* __restrict__ src, int beta, int ell,
                                                   uint64_t bias, int8_t* __restrict__ digits,
                                                   uint64_t* __restrict__ body) {
    const int i = blockIdx.x, q = threadIdx.x, KT = 32 * ell;
    const uint64_t* ct = src[i];
    const int bl = beta * ell;
    const uint64_t vmask = (1ull << bl) - 1;  // beta ell <= 32
    uint64_t w[16];
#pragma unroll
    for (int jj = 0; jj < 16; ++jj) w[jj] = ((((ct[16 * q + jj] >> (63 - bl)) + 1) >> 1) & vmask) + bias;
    if (q == 0) body[i] = ct[2048];
    const uint32_t dm = (1u << beta) - 1;
    const int half = 1 << (beta - 1);
    for (int l = 0; l < ell; ++l) {
        const int sh = beta * (ell - 1 - l);
        v4i o;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            uint32_t pk = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int d = (int)((uint32_t)(w[4 * c + e] >> sh) & dm) - half;
                pk |= (uint32_t)(uint8_t)(int8_t)d << (8 * e);
            }
            o[c] = (int)pk;
        }
        const int k0 = l * 2048 + 16 * q;
        *reinterpret_cast<v4i*>(digits + pk_frag((size_t)(i >> 4), KT, k0 >> 6, (i & 15) + 16 * ((k0 & 63) >> 4))) = o;
    }
}

// P[ct][col] for the block tiles RW (4 blockIdx.x + wave) + c and the column tile blockIdx.y.  A wave's RW
// digit fragments are reused over the 8 planes, and every plane fragment feeds RW matrix instructions.
template <int RW>
__global__ __launch_bounds__(256) void k_pk_mfma(const int8_t* __restrict__ digits, const int8_t* __restrict__ planes,
                                                 int KT, int tiles, int count, int cols, uint64_t* __restrict__ P,
                                                 int pstride) {
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t rt0 = ((size_t)blockIdx.x * 4 + wv) * RW;  // inside the digit buffer (pk_digits_bytes)
    const int tt = blockIdx.y;
    const size_t plane = (size_t)tiles * KT * 1024;
    const int8_t* A = digits + pk_frag(rt0, KT, 0, lane);
    const int8_t* Bp = planes + pk_frag(tt, KT, 0, lane);
    v4i acc[RW][8];
#pragma unroll
    for (int c = 0; c < RW; ++c)
#pragma unroll
        for (int b = 0; b < 8; ++b) acc[c][b] = v4i{0, 0, 0, 0};
    for (int kt = 0; kt < KT; ++kt) {
        v4i a[RW];
#pragma unroll
        for (int c = 0; c < RW; ++c) a[c] = *reinterpret_cast<const v4i*>(A + ((size_t)c * KT + kt) * 1024);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const v4i bb = *reinterpret_cast<const v4i*>(Bp + (size_t)b * plane + (size_t)kt * 1024);
#pragma unroll
            for (int c = 0; c < RW; ++c) acc[c][b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[c], bb, acc[c][b], 0, 0, 0);
        }
    }
    const int col = 16 * tt + (lane & 15);
    if (col >= cols) return;
#pragma unroll
    for (int c = 0; c < RW; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const size_t ct = (rt0 + c) * 16 + 4 * (lane >> 4) + r;
            if (ct >= (size_t)count) continue;
            uint64_t v = 0;
#pragma unroll
            for (int b = 0; b < 8; ++b) v += (uint64_t)(int64_t)acc[c][b][r] << (8 * b);
            P[ct * pstride + col] = v;
        }
}

// GLWE g = blockIdx.y, polynomial c = blockIdx.x.  Coefficient u of G = sum_t X^t T_t with T_t = -P_t (+ b_t
// at the body's coefficient 0): T_t[u - t] for u >= t, -T_t[u - t + N'] below.  The 12-bit values go through
// LDS so that every thread of the second phase packs 8 of them into three 32-bit words.
__global__ __launch_bounds__(256) void k_pk_pack(const uint64_t* __restrict__ P, int pstride,
                                                 const uint64_t* __restrict__ body, int B, int L, int Np, int k,
                                                 uint8_t* __restrict__ out, int ostride) {
    __shared__ uint16_t vals[2048];
    const int g = blockIdx.y, c = blockIdx.x;
    const int nb = min(L, B - g * L);
    const uint64_t* Pg = P + (size_t)g * L * pstride + (size_t)c * Np;
    for (int u = threadIdx.x; u < Np; u += 256) {
        uint64_t acc = 0;
        for (int t = 0; t < nb; ++t) {
            const uint64_t* Pt = Pg + (size_t)t * pstride;
            const int idx = u - t;
            acc += idx >= 0 ? 0ull - Pt[idx] : Pt[idx + Np];
        }
        uint32_t v;
        if (c == k) {
            if (u < nb) acc += body[(size_t)g * L + u];
            v = u < nb ? modswitch_2n(acc) : 0u;  // the other body coefficients encrypt nothing
        } else {
            v = modswitch_2n(acc);
        }
        vals[u] = (uint16_t)v;
    }
    __syncthreads();
    uint32_t* o = reinterpret_cast<uint32_t*>(out + (size_t)g * ostride + (size_t)c * (Np / 2 * 3));
    for (int q = threadIdx.x; q < Np / 8; q += 256) {
        const uint16_t* v = vals + 8 * q;
        const uint32_t v0 = v[0], v1 = v[1], v2 = v[2], v3 = v[3], v4 = v[4], v5 = v[5], v6 = v[6], v7 = v[7];
        o[3 * q + 0] = v0 | v1 << 12 | (v2 & 0xffu) << 24;
        o[3 * q + 1] = v2 >> 8 | v3 << 4 | v4 << 16 | (v5 & 0xfu) << 28;
        o[3 * q + 2] = v5 >> 4 | v6 << 8 | v7 << 20;
    }
}

namespace {
FHE_DEV uint32_t dev_get12(const uint8_t* p, int i) {
    const int o = 3 * i / 2;
    const uint32_t lo = p[o], hi = p[o + 1];
    return (i & 1) ? lo >> 4 | hi << 4 : lo | (hi & 15u) << 8;
}
}  // namespace

// Block i = blockIdx.x = (g, t): the sample extract at position t of GLWE g, every value << 52 (the blind
// rotation's modulus switch of such a word is the identity).  Mask word (c, u): A_c[t - u] for u <= t,
// -A_c[t - u + N'] mod 4096 above; body: coefficient t of B.
__global__ __launch_bounds__(256) void k_pk_unpack(const uint8_t* __restrict__ packed, int glwe_bytes, int L, int Np,
                                                   int k, uint64_t* __restrict__ rows, int stride) {
    const int i = blockIdx.x, g = i / L, t = i % L, kN = k * Np;
    const uint8_t* base = packed + (size_t)g * glwe_bytes;
    uint64_t* row = rows + (size_t)i * stride;
    for (int idx = threadIdx.x; idx < kN; idx += 256) {
        const int c = idx / Np, u = idx % Np;
        uint32_t v;
        if (u <= t)
            v = dev_get12(base, c * Np + t - u);
        else
            v = (4096u - dev_get12(base, c * Np + t - u + Np)) & 4095u;
        row[idx] = (uint64_t)v << 52;
    }
    if (threadIdx.x == 0) row[kN] = (uint64_t)dev_get12(base, kN + t) << 52;
}

int pk_col_tiles(int cols) { return (cols + 15) / 16; }
size_t pk_planes_bytes(int ell, int cols) { return (size_t)8 * pk_col_tiles(cols) * 32 * ell * 1024; }
constexpr int PK_RW_BIG = 4, PK_RW_BIG_FROM = 2048;
// k_pk_mfma reads the digit fragments of every block tile its grid covers: whole workgroups of the wider RW
size_t pk_digits_bytes(int count, int ell) {
    return (size_t)((count + 64 * PK_RW_BIG - 1) / (64 * PK_RW_BIG)) * 4 * PK_RW_BIG * 32 * ell * 1024;
}
int pk_out_stride(int k, int Np) { return ((k + 1) * (Np / 2 * 3) + 15) / 16 * 16; }

hipError_t launch_pksk_to_planes(const uint64_t* pksk, int ell, int cols, int8_t* planes, hipStream_t s) {
    const int tiles = pk_col_tiles(cols);
    hipLaunchKernelGGL(k_pksk_to_planes, dim3(tiles * 32 * ell), dim3(64), 0, s, pksk, ell, cols, tiles, planes);
    return hipGetLastError();
}

hipError_t launch_pack_keyswitch(const uint64_t* const* src, int count, int beta, int ell, int k, int Np, int L,
                                 const int8_t* planes, int8_t* digits, uint64_t* body, uint64_t* P, uint8_t* out,
                                 hipStream_t s) {
    if (count <= 0) return hipSuccess;
    const int cols = (k + 1) * Np, tiles = pk_col_tiles(cols), KT = 32 * ell;
    uint64_t bias = 0;
    for (int l = 0; l < ell; ++l) bias |= (1ull << (beta - 1)) << (beta * l);
    hipLaunchKernelGGL(k_pk_digits, dim3(count), dim3(128), 0, s, src, beta, ell, bias, digits, body);
    if (count >= PK_RW_BIG_FROM)
        hipLaunchKernelGGL(k_pk_mfma<PK_RW_BIG>, dim3((count + 64 * PK_RW_BIG - 1) / (64 * PK_RW_BIG), tiles), dim3(256),
                           0, s, digits, planes, KT, tiles, count, cols, P, cols);
    else
        hipLaunchKernelGGL(k_pk_mfma<1>, dim3((count + 63) / 64, tiles), dim3(256), 0, s, digits, planes, KT, tiles,
                           count, cols, P, cols);
    hipLaunchKernelGGL(k_pk_pack, dim3(k + 1, (count + L - 1) / L), dim3(256), 0, s, P, cols, body, count, L, Np, k, out,
                       pk_out_stride(k, Np));
    return hipGetLastError();
}

hipError_t launch_pk_unpack(const uint8_t* packed, int count, int glwe_bytes, int L, int Np, int k, uint64_t* rows,
                            int stride, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_pk_unpack, dim3(count), dim3(256), 0, s, packed, glwe_bytes, L, Np, k, rows, stride);
    return hipGetLastError();
}

}  // namespace fhe
