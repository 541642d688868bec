// oprf.hip -- the rows of the oblivious pseudo-random values (oprf.h) written into the bootstrap
// workspace, and the constant their blocks' bodies get after the blind rotation.
//
// k_oprf_rows.  The workspace is contiguous in 64-byte units: a row is upr = ms_stride / 8 units, a ChaCha
// block is one unit.  Row b, unit k < R = ceil(n / 8) is ChaCha block (row0 + b) R + k of the seed's stream;
// the unit that holds word n keeps the stream's words below n, 0 at n and the padding marker above.  When n is
// a multiple of 8 that unit is unit R: it holds no stream word and its lane computes no block.
//
// The launch is flat over the units, as seeded.hip's: a wave takes 64 consecutive units = 4 KB, a lane computes
// one block in registers, the four lanes of a quad exchange quarters (chacha_quad_exchange), and in store s lane
// l writes bytes [1024 s + 16 l, + 16) of the wave's 4 KB -- every store a dwordx4, a wave's store 1 KB without
// a gap.  For that, lane (quad q, position p) computes unit 16 p + q of the wave.  Rows do not line up with
// waves: a lane finds its row by one 32-bit division.  The last wave's units past the end are computed (the
// exchange needs every lane) and not stored.  No LDS, no scratch.
//
// k_oprf_body_add.  One lane per block: word 2048 of the descriptor's destination slot += the descriptor's
// constant, an ordinary 8-byte load and store.  Runs behind the blind rotation that wrote the slot.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "chacha_device.h"
#include "oprf.h"

namespace fhe {

namespace {

// a unit is 64-byte aligned (hipMalloc's alignment, rows of whole units)
typedef __attribute__((address_space(1))) u32x4 g_u32x4;
typedef __attribute__((address_space(1))) uint8_t g_u8;
typedef __attribute__((address_space(1))) uint64_t g_u64;

constexpr uint32_t kPadLo = (uint32_t)kMsPadWord, kPadHi = (uint32_t)(kMsPadWord >> 32);

__global__ __launch_bounds__(256) void k_oprf_rows(ChaChaKey k, uint64_t* __restrict__ ws, uint32_t row0, uint32_t units,
                                                   uint32_t upr, uint32_t R, uint32_t n) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wbase = (blockIdx.x * 4u + (threadIdx.x >> 6)) * 64u;  // the wave's first unit
    if (wbase >= units) return;                                          // wave-uniform
    const uint32_t p = lane & 3u, q = lane >> 2;
    const uint32_t u = wbase + p * 16u + q;
    const uint32_t row = u / upr, unit = u - row * upr;
    uint32_t o[16];
    if (unit < R && u < units) {
        chacha_block(k, (row0 + row) * R + unit, o);
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) o[i] = 0u;
    }
    const uint32_t w0 = unit * 8u;  // the unit's first word
    if (w0 + 8u > n) {              // the unit that holds word n
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) {
            const uint32_t w = w0 + j;
            o[2 * j] = w < n ? o[2 * j] : (w == n ? 0u : kPadLo);
            o[2 * j + 1] = w < n ? o[2 * j + 1] : (w == n ? 0u : kPadHi);
        }
    }
    u32x4 w[4];
    chacha_quad_exchange(o, p, w);
    g_u8* base = (g_u8*)ws + (size_t)wbase * 64u + lane * 16u;
#pragma unroll
    for (uint32_t s = 0; s < 4; ++s)
        if (wbase + 16u * s + q < units) *(g_u32x4*)(base + s * 1024u) = w[s];
}

__global__ __launch_bounds__(256) void k_oprf_body_add(const PbsDesc* __restrict__ desc, uint32_t count) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= count) return;
    g_u64* slot = (g_u64*)desc[i].dst;
    slot[kBigDim] += desc[i].cst;
}

}  // namespace

hipError_t launch_oprf_rows(const ChaChaKey& k, uint64_t* ws, uint32_t row0, uint32_t count, uint32_t n, hipStream_t s) {
    if (count == 0) return hipSuccess;
    const uint32_t upr = (uint32_t)(ms_stride_words(n) / 8), R = oprf_row_blocks(n);
    // at most 2^30 units (64 GB) per launch: the kernel's unit arithmetic is 32-bit
    const uint32_t step = (1u << 30) / upr;
    for (uint32_t at = 0; at < count; at += step) {
        const uint32_t rows = count - at < step ? count - at : step, units = rows * upr;
        k_oprf_rows<<<(units + 255u) / 256u, 256, 0, s>>>(k, ws + (size_t)at * upr * 8, row0 + at, units, upr, R, n);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_oprf_body_add(const PbsDesc* desc, uint32_t count, hipStream_t s) {
    if (count == 0) return hipSuccess;
    k_oprf_body_add<<<(count + 255u) / 256u, 256, 0, s>>>(desc, count);
    return hipGetLastError();
}

}  // namespace fhe
