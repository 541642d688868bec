// switched.h -- modulus-switched stored ciphertexts: tfhe-rs' CompressedModulusSwitchedCiphertext.
//
// A computed block leaves the GPU as the row its next bootstrap would read: keyswitched to the small key, then
// rounded to the blind rotation's 12 bits.  No key beyond the server key is involved.  For a block c (2049 words):
//   r     = keyswitch(c)                      n + 1 words (oracle fho_keyswitch; the kernels of ks_mfma.hip)
//   r     = ms_center(r)                      in FHE_MS_CENTERED only (ms_center.cpp), as every level does
//   v[t]  = (((r[t] >> 51) + 1) >> 1) & 4095  t <= n (device_math.h modswitch_2n, oracle fho_modswitch)
//   store = v[0 .. n] as a 12-bit little-endian bit-contiguous stream from a byte boundary (compress.h put12):
//           row_bytes(n) = ceil(12 (n + 1) / 8) bytes, the pad nibble of an odd n + 1 zero
// Back on the GPU the row's words are v[t] << 52: they have no rounding residue, so the blind rotation's own
// modulus switch returns v[t], and one blind rotation under the server key through the identity table gives
// word for word the bootstrap of c itself.  The rows must NOT be centered again (their residues are zero, and
// k_ms_center runs only behind a keyswitch).  The holder of the client key reads a row with the small key alone:
//   phase = (v[n] - sum_i v[i] s[i]) mod 4096,  value = round(phase / 128) mod 16.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "keys.h"

namespace fhe {

// bytes of one stored row on the wire, and on the device (whole 12-byte groups of 8 values: the workspace's
// rows are whole 64-byte units, oprf.h ms_stride_words)
inline size_t switched_row_bytes(uint32_t n) { return (12 * ((size_t)n + 1) + 7) / 8; }
inline size_t switched_dev_row_bytes(uint32_t n) { return ((size_t)n + 1 + 7) / 8 * 12; }

// The definitions, word for word (no context, no GPU).  rows: `stride` >= n + 1 words per row, words above n
// are not read; out: `out_stride` >= row_bytes(n) bytes per row, bytes above row_bytes(n) are not written.
void switched_pack_host(const uint64_t* rows, size_t count, uint32_t n, size_t stride, uint8_t* out, size_t out_stride);
// the inverse: words 0 .. n = v << 52, the words above n up to `stride` hold kMsPadWord (oprf.h), as a row of
// the bootstrap workspace does
void switched_unpack_host(const uint8_t* packed, size_t count, uint32_t n, size_t in_stride, uint64_t* rows, size_t stride);
// fho_keyswitch of one block under a KSK in the server key's layout [2048][ks_level][n + 1]
void keyswitch_host(const Params& p, const uint64_t* ksk, const uint64_t* ct, uint64_t* out);

// switched.hip.  ws = rows in the bootstrap workspace's layout (ms_stride_words(n) words per row, 64-byte
// aligned), packed = rows of switched_dev_row_bytes(n) bytes, 4-byte aligned.  k_ms_pack reads words 0 .. n of
// every row and writes every byte of the packed rows (zero above the n + 1 values); k_ms_unpack reads the packed
// rows and writes every word of the workspace rows (kMsPadWord above n).
hipError_t launch_ms_pack(const uint64_t* ws, uint32_t* packed, size_t count, uint32_t n, hipStream_t s);
hipError_t launch_ms_unpack(const uint32_t* packed, uint64_t* ws, size_t count, uint32_t n, hipStream_t s);

}  // namespace fhe

// One stored value.  Host object, needs no context.
struct fhe_switched_list {
    fhe::Params params;
    uint32_t form = 0, count = 0;  // FHE_SEEDED_RADIX / FHE_SEEDED_BIGUINT semantics (compress.h compressed_nblocks)
    std::vector<uint8_t> degrees;  // one per block, each < params.msg_carry()
    std::vector<uint8_t> rows;     // nblocks x switched_row_bytes(params.n)
};
