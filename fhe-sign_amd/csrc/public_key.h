// public_key.h -- public-key encryption: tfhe-rs' CompactPublicKey and CompactCiphertextList.
//
// All polynomials live in Z_2^64[X] / (X^N + 1), N = 2048.  S = the client's big (GLWE) key as a polynomial,
// coefficient order = the big LWE key's.
//   key     A = the first N u64 words of ChaChaStream(bytes_key(seed), kStreamPublicKeyMask), seed PUBLIC;
//           B = A S + E, E_j = tuniform_of(w_j, glwe_noise_log2), w_0 .. w_(N-1) the next N words of the client
//           key's encryption stream
//   list    the values' 2-bit blocks become coefficients in order: one block per coefficient (unpacked), or
//           m_2i + 4 m_(2i+1) (packed; an odd last block stands alone, every value starts on a fresh
//           coefficient).  Coefficients fill chunks of N.  Chunk c draws, from streams keyed by the SECRET
//           32-byte encryption seed:
//             R   bit i = bit (i & 63) of u64 word 32 c + (i >> 6) of stream kStreamCompactBinary
//             E1  N words from u64 word 2 N c of stream kStreamCompactNoise, E2 the words after them (one per
//                 used coefficient), each through tuniform_of at glwe_noise_log2
//           C_A = A R + E1 (N words), C_B[j] = (B R)[j] + E2[j] + delta m_j for the used coefficients j
//   expand  coefficient t of a chunk -> the big LWE with mask word u = C_A[t - u] (u <= t), -C_A[t - u + N]
//           (u > t), body C_B[t]: the sample extraction of compress.hip's k_pk_unpack and of the oracle
// The phase error of a coefficient is E R + E2 - E1 S: |.| <= 2048 2^17 + 2^17 + 2048 2^17 < 2^30 (R, S binary).
//
// Re-randomization (tfhe-rs' re_randomize under the CompactPublicKey): blocks 0 .. n-1 of a value
// get a fresh public-key encryption of ZERO added.  From a 32-byte re-randomization seed, chunk c draws R and
// the noise at the list's positions under stream ids of its own (kStreamRerandBinary / kStreamRerandNoise):
//   Z_A = A R + E1, Z_B[j] = (B R)[j] + E2[j] for the used j (no message term)
//   block i (t = i mod N of chunk i / N): mask word u += Z_A[t - u] (u <= t), -= Z_A[t - u + N] (u > t),
//   body += Z_B[t] -- the sample extraction above, added to the input instead of written.
// The added phase error is again E R + E2 - E1 S, below 2^30 in magnitude.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <thread>
#include <vector>

#include "keys.h"

namespace fhe {
// a chunk's noise words start on a stride of 2 N u64 = 512 ChaCha blocks; 2^24 coefficients are 2^13 chunks
constexpr uint64_t kCompactMaxCoefs = 1ull << 24;
constexpr uint32_t kCompactMaxValues = 1u << 16;
}  // namespace fhe

struct fhe_public_key {
    fhe::Params params;
    uint8_t seed[32] = {};       // PUBLIC: the mask polynomial's
    std::vector<uint64_t> body;  // B, N words
};

struct fhe_compact_list {
    struct Value {
        uint32_t form = 0;   // FHE_SEEDED_RADIX / FHE_SEEDED_BIGUINT
        uint32_t count = 0;  // num_bits, or nlimbs
        size_t nblocks = 0;  // derived: count / 2, or 16 count
        size_t first = 0;    // derived: its first coefficient
        size_t ncoef = 0;    // derived: nblocks (unpacked), (nblocks + 1) / 2 (packed)
    };
    fhe::Params params;
    bool packed = false;
    std::vector<Value> values;
    std::vector<uint64_t> ca;  // nchunks x N
    std::vector<uint64_t> cb;  // ncoef
    size_t ncoef() const { return cb.size(); }
    size_t nchunks() const { return ca.size() / fhe::kPolySize; }
};

// the values pushed so far (CompactCiphertextList::builder): 2-bit blocks, LSB first
struct fhe_compact_builder {
    fhe_public_key pk;
    std::vector<fhe_compact_list::Value> values;
    std::vector<uint8_t> blocks;
};

namespace fhe {
// r += a * s mod (X^N + 1) for the binary polynomial whose coefficient j is bit(j)
template <class Bit>
void negacyclic_binary_mac(uint64_t* r, const uint64_t* a, Bit&& bit) {
    constexpr uint32_t N = kPolySize;
    for (uint32_t j = 0; j < N; ++j) {
        if (!bit(j)) continue;
        for (uint32_t m = j; m < N; ++m) r[m] += a[m - j];
        for (uint32_t m = 0; m < j; ++m) r[m] -= a[m + N - j];
    }
}
// fn(c) for c < chunks on up to 16 host threads: every chunk seeks its own streams, so the split only
// divides the work
template <class F>
void parallel_chunks(size_t chunks, F&& fn) {
    const size_t hw = std::max(1u, std::thread::hardware_concurrency());
    const size_t T = std::min<size_t>(std::min<size_t>(hw, 16), chunks);
    if (T <= 1) {
        for (size_t c = 0; c < chunks; ++c) fn(c);
        return;
    }
    std::vector<std::thread> th;
    for (size_t t = 0; t < T; ++t)
        th.emplace_back([&, t] {
            for (size_t c = t; c < chunks; c += T) fn(c);
        });
    for (auto& x : th) x.join();
}
// A = the first N words of the key's mask stream
void public_key_mask(const uint8_t seed[32], uint64_t* A);
// pk of ck under the PUBLIC mask seed: advances ck->enc_rng by exactly N words, drawn before the threaded pass
void generate_public_key(fhe_client_key* ck, const uint8_t seed[32], fhe_public_key* pk);
// fills first / ncoef / nblocks of every value; false (with the offending field named) on a malformed table
bool compact_layout(std::vector<fhe_compact_list::Value>& values, bool packed, size_t* ncoef, std::string* why);
// the list of `blocks` (sum of the values' nblocks 2-bit messages) under pk and the SECRET encryption seed
void encrypt_compact(const fhe_public_key& pk, const uint8_t enc_seed[32], bool packed,
                     const std::vector<fhe_compact_list::Value>& values, const uint8_t* blocks, fhe_compact_list* out);
// rows[i] = the big LWE of coefficient first + i (i < n): 2049 words each.  The word-for-word definition of
// public_key.hip's k_compact_extract.
void expand_compact_host(const fhe_compact_list& x, size_t first, size_t n, uint64_t* rows);
// the degree of coefficient g's plaintext: 3, or 15 where two blocks share it
uint32_t compact_degree(const fhe_compact_list& x, const fhe_compact_list::Value& v, size_t g);
// rerandomize.cpp: the zero encryptions of n blocks under the re-randomization seed: za = Z_A of every chunk
// (ceil(n / N) x N words), zb = Z_B of the used coefficients (n words).  n <= kCompactMaxCoefs.
void rerandomize_zero_host(const fhe_public_key& pk, const uint8_t seed[32], size_t n, uint64_t* za, uint64_t* zb);
// cts: n rows of 2049 words, re-randomized in place.  The word-for-word definition of rerandomize.hip.
void rerandomize_host(const fhe_public_key& pk, const uint8_t seed[32], uint64_t* cts, size_t n);
}  // namespace fhe
