// client_ops_index.h -- where the words of a client-key encryption lie in the encryption stream, stated once for
// the device kernel (client_ops.hip) and for its host restatement (client_ops.cpp:
// fhe_client_encrypt_rows_indexed_host).  Host and device code; no HIP runtime call.
//
// keys.cpp:encrypt_big_many draws, for block i of a batch, the u64 stream words [W0 + 2049 i, W0 + 2049 i + 2049)
// of ck->enc_rng: 2048 mask words, then the word the noise comes from (tuniform_of).  W0 is the stream's position
// in u64 words when the batch starts (the stream is only ever drawn in whole u64 words).  A ChaCha block is 8 u64
// words, so with g = W0 + 2049 i a row starts off = g mod 8 = (W0 + i) mod 8 words into ChaCha block g / 8 and
// touches the 257 blocks ("units") g / 8 + t, t = 0 .. 256 -- always 257: the row's last word is word
// off + 2048 <= 2055 of them.  Word w < 8 of unit t is the row's word 8 t - off + w:
//   below 0         the previous row's (unit 0 when off > 0), not this row's to write
//   0 .. 2047       mask word of that index
//   2048            the noise word (unit 256, w = off)
//   above           the next row's
// Units 1 .. 255 are whole mask words: 64 contiguous bytes at byte 8 (8 t - off) of the 8-byte-aligned slot.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FHE_HD __host__ __device__
#else
#define FHE_HD
#endif

namespace fhe {
namespace client_ops {

constexpr uint32_t kMaskWords = 2048;           // = kBigDim
constexpr uint32_t kRowWords = kMaskWords + 1;  // stream words of one encryption
constexpr uint32_t kUnitWords = 8;              // u64 words of one ChaCha block
constexpr uint32_t kRowUnits = 257;             // ChaCha blocks one row touches, whatever its offset
constexpr uint32_t kKeyWords = kMaskWords / 32; // the packed key bits as u32 words: bit j = word j / 32, bit j % 32

// first stream word of row i of a batch that starts at u64 word w0
FHE_HD inline uint64_t row_first_word(uint64_t w0, uint64_t i) { return w0 + (uint64_t)kRowWords * i; }
// ... its ChaCha block counter (the caller has checked that the batch stays in the 32-bit counter epoch) and the
// row's offset into that block
FHE_HD inline uint32_t row_first_unit(uint64_t g) { return (uint32_t)(g / kUnitWords); }
FHE_HD inline uint32_t row_offset(uint64_t g) { return (uint32_t)(g % kUnitWords); }
// the row word that word 0 of unit t is (negative for unit 0 when off > 0)
FHE_HD inline int32_t unit_row_word(uint32_t t, uint32_t off) { return (int32_t)(kUnitWords * t) - (int32_t)off; }

// bits [p, p + 8) of the packed key as a byte, bit w = key bit p + w; bits outside [0, 2048) are zero, so a unit
// that straddles a row's end or start contributes only its mask words.  -8 < p <= 2048.
FHE_HD inline uint32_t key_bits8(const uint32_t* kb, int32_t p) {
    if (p < 0) return (kb[0] << (uint32_t)(-p)) & 0xFFu;
    const uint32_t w = (uint32_t)p >> 5, sh = (uint32_t)p & 31u;
    const uint64_t lo = w < kKeyWords ? kb[w] : 0u, hi = w + 1 < kKeyWords ? kb[w + 1] : 0u;
    return (uint32_t)((lo | hi << 32) >> sh) & 0xFFu;
}

// keys.cpp:tuniform_of as an unsigned word (added with wrap)
FHE_HD inline uint64_t tuniform_word(uint64_t x, uint32_t b) {
    const uint64_t u = x & ((1ull << (b + 1)) - 1);
    const uint64_t c = (x >> (b + 1)) & 1ull;
    return u + c - (1ull << b);
}

// The stream parameters of one call as the kernel reads them from device memory, behind the key bits: the
// stream's key and nonce, the batch's first word and the noise bound.  16 u32 words.
struct StreamParams {
    uint32_t key[8];
    uint32_t nonce[3];
    uint32_t noise_log2;
    uint32_t w0_lo, w0_hi;
    uint32_t pad[2];
};
constexpr uint32_t kStreamParamWords = sizeof(StreamParams) / 4;  // 16
constexpr uint32_t kClientWords = kKeyWords + kStreamParamWords;  // the resident buffer: key bits, then these

}  // namespace client_ops
}  // namespace fhe
