// compress.h -- compressed computed ciphertexts: tfhe-rs' CompressedCiphertextList.
//
// A list of big-key LWE blocks is packed into GLWEs under a dedicated secret s' by a packing keyswitch,
// every kept coefficient is modulus-switched to 12 bits, and a bootstrap under a decompression key brings
// the blocks back.  For B blocks ct_i = (a_i[2048], b_i), GLWE g = i / L, slot t = i % L:
//   T_i   = (0, .., 0, b_i X^0) - sum_{j < 2048} sum_{l < ell} d[i, j, l] PKSK[j][l]      (k' + 1 polynomials)
//   G_g   = sum_{i in g} X^t T_i                         (negacyclic: coefficient u >= N' - t wraps with a minus)
//   store = modswitch12(every mask coefficient of G_g, body coefficients 0 .. b_g - 1), b_g = min(L, B - g L)
//   modswitch12(x) = (((x >> 51) + 1) >> 1) & 4095       (device_math.h modswitch_2n)
// d[i, j, .] = the balanced base-2^beta digits of a_i[j] rounded to its top beta ell bits, level 0 the most
// significant, in [-2^(beta - 1), 2^(beta - 1) - 1], the top carry dropped.  All of it is exact in Z / 2^64.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "keys.h"

namespace fhe {

// tfhe-rs' COMP_PARAM_MESSAGE_2_CARRY_2_KS_PBS_TUNIFORM_2M64 AS RECALLED (as Params' defaults are)
struct CompParams {
    uint32_t k = 4;    // glwe_dimension k'
    uint32_t N = 256;  // polynomial_size N'
    uint32_t L = 256;  // lwe_per_glwe
    uint32_t beta = 4, ell = 4;  // packing keyswitch base log, levels
    uint32_t pks_noise_log2 = 42;
    uint32_t storage_log_modulus = 12;

    static bool from_c(const fhe_compression_params& c, CompParams* out, const char** why);
    fhe_compression_params to_c() const;
    uint32_t lwe_dim() const { return k * N; }          // the decompression bootstrap's LWE dimension
    uint32_t cols() const { return (k + 1) * N; }       // words of one packing-KSK row
    size_t pksk_words() const { return (size_t)kBigDim * ell * cols(); }
    size_t bsk_words() const { return (size_t)lwe_dim() * 4 * kPolySize; }
    size_t glwes(size_t B) const { return (B + L - 1) / L; }
    size_t bodies(size_t B, size_t g) const { return std::min<size_t>(L, B - g * L); }
    size_t glwe_bytes(size_t nbodies) const { return (12 * ((size_t)lwe_dim() + nbodies) + 7) / 8; }
    // packed bytes of a B-block list: every GLWE but the last is full
    size_t packed_bytes(size_t B) const {
        if (B == 0) return 0;
        const size_t G = glwes(B);
        return (G - 1) * glwe_bytes(L) + glwe_bytes(bodies(B, G - 1));
    }
    // words of the client key's encryption stream fhe_compression_keys_generate consumes
    size_t stream_words() const { return (size_t)lwe_dim() + pksk_words() + bsk_words(); }
    // the seeded form (fhe_seeded_compression_key): body words, and the stream words its generation consumes
    size_t pksk_body_words() const { return (size_t)kBigDim * ell * N; }
    size_t bsk_body_words() const { return (size_t)lwe_dim() * 2 * kPolySize; }
    size_t seeded_stream_words() const { return (size_t)lwe_dim() + pksk_body_words() + bsk_body_words(); }
    bool operator==(const CompParams& o) const {
        return k == o.k && N == o.N && L == o.L && beta == o.beta && ell == o.ell &&
               pks_noise_log2 == o.pks_noise_log2 && storage_log_modulus == o.storage_log_modulus;
    }
};

constexpr uint64_t kCompressedMaxBlocks = 1ull << 24;

// value i of a 12-bit little-endian bit-contiguous stream
inline uint32_t get12(const uint8_t* p, size_t i) {
    const size_t o = 3 * i / 2;
    return (i & 1) ? (uint32_t)(p[o] >> 4) | (uint32_t)p[o + 1] << 4 : (uint32_t)p[o] | (uint32_t)(p[o + 1] & 15) << 8;
}
inline void put12(uint8_t* p, size_t i, uint32_t v) {  // into zeroed bytes
    const size_t o = 3 * i / 2;
    if (i & 1) {
        p[o] |= (uint8_t)(v << 4);
        p[o + 1] = (uint8_t)(v >> 4);
    } else {
        p[o] = (uint8_t)v;
        p[o + 1] |= (uint8_t)((v >> 8) & 15);
    }
}

}  // namespace fhe

struct fhe_compression_private_key {
    fhe::Params params;
    fhe::CompParams cp;
    std::vector<uint64_t> sk;  // k' N' binary, polynomial-major
};

struct fhe_compression_key {
    fhe::Params params;
    fhe::CompParams cp;
    std::vector<uint64_t> pksk;  // [2048][ell][k' + 1][N']
    std::vector<uint64_t> bsk;   // [k' N'][row][poly][2048], standard domain, classic
};

// A seeded (compressed) compression key: tfhe-rs' CompressedCompressionKey + CompressedDecompressionKey
// (DESIGN.md 6e).  Host only.  Of the full key only the bodies are kept; every mask word is regenerated from
// the PUBLIC seed, one row per 256 ChaCha blocks (2048 u64 words; k' N' <= 2048):
//   packing KSK row r = j ell + l (stream kStreamSeededPksk): coefficient m of mask polynomial c < k' = u64 word
//       2048 r + c N' + m; pksk_bodies[r N' ..] = B = sum_c A_c * s'_c + e, then B[0] += S_j << (64 - beta (l + 1))
//   BSK GGSW q < k' N', row rho (stream kStreamSeededCbsk): mask polynomial A = u64 words [2048 (2 q + rho),
//       + 2048); bsk_bodies[(2 q + rho) 2048 ..] = B = A * S + e, then row 1: B[0] += g s'_q; row 0: B[t] -=
//       g s'_q S_t for every t (g = 1 << (64 - pbs_base_log)): the body form of row 0's gadget, as in
//       fhe_seeded_server_key (keys.h) -- the expanded key's words differ from generate_compression_keys' for
//       the same secrets, its phases do not.
// One seed, one object: a seed is never reused for a second key, or for a seeded ciphertext, under the same
// client key.
struct fhe_seeded_compression_key {
    fhe::Params params;
    fhe::CompParams cp;
    uint8_t seed[32] = {};
    std::vector<uint64_t> pksk_bodies;  // [2048][ell][N']
    std::vector<uint64_t> bsk_bodies;   // [k' N'][2][2048]
};

struct fhe_compressed_list {
    fhe::Params params;
    fhe::CompParams cp;
    uint32_t form = 0, count = 0;
    std::vector<uint8_t> degrees;  // one per block
    std::vector<uint8_t> packed;   // the GLWEs' 12-bit streams, each from a byte boundary
};

namespace fhe {
void generate_compression_keys(fhe_client_key* ck, const CompParams& cp, fhe_compression_private_key* priv,
                               fhe_compression_key* key);
// The seeded key of ck under the public `seed`.  Everything is drawn from ck->enc_rng before any threaded pass:
// k' N' secret words (bit 0 of each: the s' generate_compression_keys draws from the same stream state), then
// N' noise words per packing-key row in row order, then 2048 noise words per BSK row in (q, rho) order --
// exactly CompParams::seeded_stream_words() words, whatever the number of host threads.
void generate_seeded_compression_keys(fhe_client_key* ck, const CompParams& cp, const uint8_t seed[32],
                                      fhe_compression_private_key* priv, fhe_seeded_compression_key* out);
// The full key of a seeded one: masks regenerated, bodies in place.  The word-for-word definition of the
// device install (seeded_compression.hip, seeded_key.hip).
void expand_seeded_compression_key_host(const fhe_seeded_compression_key& sck, fhe_compression_key* key);
// The definition of the device path (compress.hip), word for word: packed = CompParams::packed_bytes(B)
// bytes.  Threaded over the blocks of a GLWE; the result does not depend on the thread count (every
// T_i is computed alone, and the sum is taken mod 2^64).
void pack_keyswitch_host(const fhe_compression_key& key, const uint64_t* cts, size_t B, uint8_t* packed);
// blocks of a form / count pair (FHE_SEEDED_RADIX: num_bits / 2, FHE_SEEDED_BIGUINT: 16 nlimbs)
bool compressed_nblocks(uint32_t form, uint32_t count, size_t* nblocks, std::string* why);
// sum v_k 4^k of decoded block values (each < 16), per value (radix) or per 32-bit limb (BigUintFHE: 16 blocks,
// limb i at bits 32 i), the carries of blocks above degree 3 kept inside it -- as fhe_radix_decrypt assembles
void assemble_block_values(const std::vector<uint32_t>& vals, uint32_t form, uint64_t* words, size_t nwords);
// the first main-parameter field in which a and b differ, or null
const char* params_differ(const Params& a, const Params& b, uint32_t* have, uint32_t* want);
}  // namespace fhe
