// oprf.h -- oblivious pseudo-random values: tfhe-rs' generate_oblivious_pseudo_random.
//
// A small-key LWE row whose mask comes from a PUBLIC seed and whose body is 0 has the phase -<a, s>: uniform,
// and unknown to anyone without the key.  One blind rotation through a staircase polynomial, no keyswitch
// before it, turns the row into a clean block of `bits` uniformly random bits.
//   rows         row b: mask word j < n = u64 word j of ChaCha blocks [b R, (b + 1) R) of stream kStreamOprf
//                under the seed, R = ceil(n / 8); word n (the body) = 0; in a layout of `stride` words per row
//                the words above n hold kMsPadWord
//   accumulator  coefficient i < N = (2 floor(i p / 2N) + 1) delta / 2, p = 2^bits: no half-box rotation, no
//                negated head
//   block b      sample extraction of the blind rotation of row b through the accumulator, then
//                (p - 1) delta / 2 added to the body.  With m~ = -sum ms(a_i) s_i mod 2N (ms = the blind
//                rotation's 12-bit rounding) it encrypts floor(m~ p / 2N) + p / 2 for m~ < N and
//                p / 2 - 1 - floor((m~ - N) p / 2N) otherwise: decided by the rounding alone, since every
//                coefficient of one stair holds the same value.  Degree p - 1, noise 1.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "keygen.h"
#include "keys.h"

namespace fhe {

// what a row's padding holds (the Python mirror's MS_PAD_WORD)
constexpr uint64_t kMsPadWord = 0xA5A55A5AC3C33C3Cull;
// rows of one seed: R <= 256 ChaCha blocks each, the block counter stays below 2^31
constexpr size_t kOprfMaxRows = (size_t)1 << 23;

inline uint32_t oprf_row_blocks(uint32_t n) { return (n + 7) / 8; }
// words per row of the bootstrap workspace (fhe_ctx::ensure_ms): n + 1 rounded up to 64 bytes
inline size_t ms_stride_words(uint32_t n) { return ((size_t)n + 1 + 7) / 8 * 8; }

// rows [row0, row0 + count) of the seed into out, `stride` >= n + 1 words per row, padding included
void oprf_rows_host(const uint8_t seed[32], uint32_t n, size_t row0, size_t count, size_t stride, uint64_t* out);
// the accumulator polynomial, kPolySize words; 1 <= bits <= log2(message_modulus) (the caller checks)
void oprf_lut_poly(const Params& p, uint32_t bits, uint64_t* out);
inline uint64_t oprf_body_const(const Params& p, uint32_t bits) { return ((1ull << bits) - 1) * (p.delta() / 2); }
inline uint32_t oprf_max_bits(const Params& p) {
    uint32_t b = 0;
    while ((2u << b) <= p.message_modulus) ++b;
    return b;
}

// oprf.hip.  ws = the bootstrap workspace, ms_stride_words(n) words per row, 64-byte aligned: rows
// [row0, row0 + count) of the stream are written to its rows [0, count), padding included
hipError_t launch_oprf_rows(const ChaChaKey& k, uint64_t* ws, uint32_t row0, uint32_t count, uint32_t n, hipStream_t s);
// desc[i].dst[2048] += desc[i].cst for i < count (desc a device array)
hipError_t launch_oprf_body_add(const PbsDesc* desc, uint32_t count, hipStream_t s);

}  // namespace fhe
