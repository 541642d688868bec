// serial.h -- versioned, checksummed binary format for keys and ciphertexts.
//
// The reference never serializes (keys are regenerated per run; `grep serial` hits only a doc
// comment, src/schnorr.rs:47); tfhe-rs's bincode + tfhe-versionable wire format cannot be pinned
// here (no tfhe-rs fixture, crate absent), so this is this engine's own format, little-endian:
//   header  magic "FHEROCM\0" | u32 version (2; 1 still read) | u32 kind | u64 payload bytes | u64 checksum
//           (FNV-1a over the payload's little-endian u64 words, tail zero-padded)
//   payload params (9 x u32: n, pbs_base_log, ks_base_log, ks_level, lwe/glwe noise log2, msg,
//           carry, grouping -- version 1 has no grouping word: classic) then the kind's fields
//           (serial.cpp / capi_radix.cpp).
//   kind 5 (seeded ciphertext, capi_radix.cpp): params | u32 form (0 radix, 1 BigUintFHE) | u32 count
//           (num_bits, or nlimbs) | 32 seed bytes | nblocks u64 bodies (nblocks = num_bits / 2, or
//           16 nlimbs; LSB block first).  The masks are not stored: block i's are u64 words [2048 i,
//           2048 (i + 1)) of the ChaCha20 stream keyed by the seed, nonce {101, "ROCM", 0} (keys.h).
//   kind 6 (seeded server key, serial.cpp): params | 32 seed bytes | 2048 ks_level u64 KSK bodies |
//           ggsw 2 2048 u64 BSK body polynomials -- 100 + 8 (2048 ks_level + 4096 ggsw) bytes in all.  The
//           masks are not stored: streams 102 (KSK) and 103 (BSK) under the seed, one row per 256 ChaCha
//           blocks (keys.h fhe_seeded_server_key).
//   kinds 7 / 8 / 9 (compress_host.cpp; compressed computed ciphertexts): params | 7 x u32 compression params
//           (k', N', L, pks_base_log, pks_level, pks_noise_log2, storage_log_modulus), then 7: k' N' u64 secret
//           words; 8: the packing KSK u64[2048][pks_level][k' + 1][N'], the decompression BSK u64[k' N'][2][2][2048];
//           9: u32 form | u32 count | u32 B | B degree bytes | per GLWE the 12-bit stream of k' N' + b_g values,
//           each GLWE from a byte boundary -- 108 + B + sum_g ceil(12 (k' N' + b_g) / 8) bytes in all.
//   kind 10 (public key, public_key.cpp): params | 32 seed bytes | 2048 u64 body words -- 16,484 bytes in all.
//   kind 11 (compact ciphertext list, public_key.cpp): params | u32 packed (0 / 1) | u32 nvalues | per value
//           u32 form, u32 count | per chunk 2048 u64 C_A words | ncoef u64 C_B words -- 76 + 8 nvalues +
//           8 (2048 nchunks + ncoef) bytes in all; ncoef and nchunks follow from the value table.
//   kind 12 (seeded compression key, compress_host.cpp): params | 7 x u32 compression params | 32 seed bytes |
//           2048 pks_level N' u64 packing-key bodies | k' N' 2 2048 u64 BSK body polynomials -- 128 +
//           8 (2048 pks_level N' + 4096 k' N') bytes in all.  The masks are not stored: streams 107 (packing
//           KSK) and 108 (decompression BSK) under the seed, one row per 256 ChaCha blocks (compress.h).
//   kind 13 (modulus-switched stored list, switched.cpp): params | u32 form | u32 count | u32 B | B degree bytes
//           (each < mc) | B rows of ceil(12 (n + 1) / 8) bytes, the 12-bit stream of a row's n + 1 values, the pad
//           nibble of an odd n + 1 zero -- 80 + B (1 + ceil(12 (n + 1) / 8)) bytes in all.
//   kind 14 (re-keying key, switched.cpp): the DESTINATION's params | 32 seed bytes | 2048 ks_level u64 body words
//           -- 100 + 8 (2048 ks_level) bytes in all.  The masks are not stored: stream 112 under the seed, one
//           row per 256 ChaCha blocks (keys.h fhe_rekey_key).
// Readers check magic, version, kind, length, checksum, parameter ranges and every count before
// touching memory, and refuse block metadata (degree, noise) outside the radix layer's budget, so a
// corrupted or hostile buffer fails with FHE_ERR_INVALID instead of poisoning the scheduler.
#pragma once
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "keys.h"

namespace fhe::ser {

enum Kind : uint32_t { kClientKey = 1, kServerKey = 2, kRadix = 3, kBigUint = 4, kSeeded = 5, kSeededServerKey = 6,
                       kCompressionPrivateKey = 7, kCompressionKey = 8, kCompressedList = 9,
                       kPublicKey = 10, kCompactList = 11, kSeededCompressionKey = 12, kSwitchedList = 13,
                       kRekeyKey = 14 };
constexpr uint32_t kVersion = 2;  // 2: params carry the blind-rotation grouping (9th word); 1 still read
constexpr size_t kHeaderBytes = 32;

struct Writer {
    std::vector<uint8_t> b;
    void raw(const void* p, size_t n) {
        const uint8_t* q = static_cast<const uint8_t*>(p);
        b.insert(b.end(), q, q + n);
    }
    void u8(uint8_t v) { b.push_back(v); }
    void u32(uint32_t v) { raw(&v, 4); }  // little-endian hosts only (x86-64)
    void u64(uint64_t v) { raw(&v, 8); }
    void words(const uint64_t* p, size_t n) { raw(p, n * 8); }
    void params(const Params& p);
};

struct Reader {
    const uint8_t* p = nullptr;
    size_t n = 0, off = 0;
    bool ok = true;
    uint32_t version = kVersion;  // of the frame (unframe sets it)
    bool take(void* dst, size_t k) {
        if (!ok || n - off < k) return ok = false;
        if (k) memcpy(dst, p + off, k);  // an empty vector's data() may be null
        off += k;
        return true;
    }
    uint8_t u8() { uint8_t v = 0; take(&v, 1); return v; }
    uint32_t u32() { uint32_t v = 0; take(&v, 4); return v; }
    uint64_t u64() { uint64_t v = 0; take(&v, 8); return v; }
    bool words(uint64_t* dst, size_t k) { return k <= (n - off) / 8 && take(dst, k * 8); }
    bool params(Params* out, std::string* why);
    bool done() const { return ok && off == n; }
};

uint64_t fnv1a(const uint8_t* p, size_t n);
// header + payload
std::vector<uint8_t> frame(Kind kind, const std::vector<uint8_t>& payload);
// checks the header; on success `payload` points into buf
bool unframe(const uint8_t* buf, size_t len, Kind kind, Reader* payload, std::string* why);
// size-query convention of the C ABI: buf == NULL -> *len = size, FHE_OK; cap too small ->
// *len = size, FHE_ERR_INVALID; else copy
int emit(const std::vector<uint8_t>& bytes, uint8_t* buf, size_t cap, size_t* len);

}  // namespace fhe::ser
