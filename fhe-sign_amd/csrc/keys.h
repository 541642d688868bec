// keys.h -- client/server key material (host side) and the seeded CSPRNG.
//
// Replaces tfhe::generate_keys / ClientKey / ServerKey (src/schnorr.rs:441-443).  Client-side
// operations (keygen, encrypt, decrypt) run on the host exactly as tfhe-rs runs them on the
// client; the server key is uploaded to the GPU by fhe::Context::set_server_key.
#pragma once
#include <array>
#include <cstdint>
#include <string>
#include <vector>

#include "fhe_rocm.h"

namespace fhe {

// Fixed shape of the device kernels.
constexpr uint32_t kPolySize = 2048;
constexpr uint32_t kBigDim = 2048;      // k * N
constexpr uint32_t kBigCt = kBigDim + 1;

struct Params {
    uint32_t n = 834;
    uint32_t pbs_base_log = 23;
    uint32_t ks_base_log = 3;
    uint32_t ks_level = 5;
    uint32_t lwe_noise_log2 = 45;  // recalled tfhe 0.10 new_t_uniform(45); 44 until r6
    uint32_t glwe_noise_log2 = 17;
    uint32_t message_modulus = 4;
    uint32_t carry_modulus = 4;
    // blind-rotation grouping factor: 1 = one CMUX per key bit (tfhe-rs' classic PBS), 2 = multi-bit
    // (tfhe-rs' MultiBitPBS shape: two key bits per external product, 3 GGSWs per pair of bits)
    uint32_t grouping = 1;

    static bool from_c(const fhe_params& c, Params* out, const char** why);
    fhe_params to_c() const;
    uint64_t delta() const { return (1ull << 63) / ((uint64_t)message_modulus * carry_modulus); }
    uint32_t msg_carry() const { return message_modulus * carry_modulus; }
    // GGSWs in the bootstrapping key: n (classic) or (n / g)(2^g - 1) (multi-bit)
    uint32_t ggsw_count() const { return grouping == 1 ? n : n / grouping * ((1u << grouping) - 1); }
    // the message of GGSW q: s_q (classic); multi-bit group i = q / 3, pattern B = q % 3 + 1 of
    // (s_2i, s_2i+1): f_B = [s_2i = B bit 0][s_2i+1 = B bit 1] (oracle fho_keygen)
    uint64_t ggsw_message(const uint64_t* lwe_sk, uint32_t q) const {
        if (grouping == 1) return lwe_sk[q];
        const uint32_t i = q / 3, B = q % 3 + 1;
        const uint64_t s0 = lwe_sk[2 * i] & 1, s1 = lwe_sk[2 * i + 1] & 1;
        return ((B & 1) ? s0 : 1 - s0) & ((B & 2) ? s1 : 1 - s1);
    }
    // The one rule of the radix layer (FheUint, BigUintFHE, and their seeded, compact, stored and signed forms):
    // it cuts values into 2-bit digits with 2 carry bits above them (engine.h kMsgBits / kMsgMod, 16-entry tables),
    // so it needs message_modulus 4 and carry_modulus 4 exactly -- not another split of 16, and no other product.
    // Keys, block encryption, LUTs, the raw bootstrap, the keyswitch, OPRF blocks and the block-level stored lists
    // take any space Params::from_c admits.  Every radix entry point asks this before it encrypts, records or
    // launches anything (radix_space_refusal is its answer).
    bool radix_space() const { return message_modulus == 4 && carry_modulus == 4; }
};

// the text of a refusal under Params::radix_space: `who` names the entry point or the object
inline std::string radix_space_refusal(const Params& p, const char* who) {
    return std::string(who) + ": the radix layer needs message_modulus 4 and carry_modulus 4; this key has message_modulus " +
           std::to_string(p.message_modulus) + ", carry_modulus " + std::to_string(p.carry_modulus);
}

// (The parameters and keys of the compressed computed ciphertexts -- tfhe-rs' compression parameters AS
// RECALLED, like the defaults above -- are in compress.h: CompParams, fhe_compression_key.)

// The 256-bit ChaCha20 key every key-generation stream is derived from (stream id = nonce word 0).
// Production keys come from 32 bytes of OS entropy (fhe_generate_keys_keyed, generate_keys(seed=None)
// in the Python mirror); `seed_key` expands a 64-bit test seed into {seed, "FHES", 0, ...} -- a
// deterministic, publicly reproducible key meant for tests only.
using KeyWords = std::array<uint32_t, 8>;
KeyWords seed_key(uint64_t seed);
KeyWords bytes_key(const uint8_t* key32);  // little-endian words
// 32 bytes from getrandom(): the default public mask seed of the seeded objects below; false if it fails
bool os_entropy32(uint8_t out[32]);

// ChaCha20 block function (RFC 8439) as a deterministic stream of 64-bit words.
class ChaChaStream {
public:
    ChaChaStream() = default;
    ChaChaStream(uint64_t seed, uint32_t stream) { reset(seed, stream); }
    ChaChaStream(const KeyWords& key, uint32_t stream) { reset(key, stream); }
    void reset(uint64_t seed, uint32_t stream) { reset(seed_key(seed), stream); }
    void reset(const KeyWords& key, uint32_t stream);
    uint64_t next_u64();
    void fill_u64(uint64_t* out, size_t n);  // n next_u64() values (bulk: 8 blocks per step)
    int64_t tuniform(uint32_t log2_bound);
    // absolute position (32-bit words) of the next output within the current nonce epoch, and a
    // jump to such a position (false if it leaves the epoch): lets independent encryptions of a
    // batch run in parallel on copies of the stream with exactly the sequential outputs
    uint64_t word_pos() const { return (uint64_t)counter_ * 16 - (16 - pos_); }
    bool seek(uint64_t word);
    // the key and nonce of the current epoch: with word_pos() all a device restatement of the stream needs
    // (client_ops.hip); secret where the stream's key is
    const std::array<uint32_t, 8>& key_words() const { return key_; }
    const std::array<uint32_t, 3>& nonce_words() const { return nonce_; }
    // full state (key, nonce, counter, buffered block, position) for serialization (serial.cpp)
    static constexpr size_t kStateWords = 8 + 3 + 1 + 16 + 1;
    void save(uint32_t* out) const;
    bool load(const uint32_t* in);  // false if the state is malformed

private:
    void refill();
    std::array<uint32_t, 8> key_{};
    std::array<uint32_t, 3> nonce_{};
    uint32_t counter_ = 0;
    std::array<uint32_t, 16> buf_{};
    uint32_t pos_ = 16;
};

// the TUniform(b) sample ChaChaStream::tuniform draws from one 64-bit stream word x
int64_t tuniform_of(uint64_t x, uint32_t log2_bound);

// Stream ids (shared convention with the oracle so key bytes can be compared).
enum : uint32_t { kStreamSecret = 1, kStreamKsk = 2, kStreamBsk = 3, kStreamEncrypt = 100 };
// Mask stream of a seeded ciphertext (fhe_seeded below).  Keyed by the object's PUBLIC 32-byte seed, not
// by the client's key: it shares nothing with the streams above.
constexpr uint32_t kStreamSeededMask = 101;
// The ChaCha block counter is 32 bits and one radix block takes 256 ChaCha blocks of masks.
constexpr uint64_t kSeededMaxBlocks = 1ull << 24;
// Mask streams of a seeded server key (fhe_seeded_server_key below), keyed by its PUBLIC seed as well.  A
// row (one KSK row, one BSK mask polynomial) starts on a stride of 256 ChaCha blocks = 2048 u64 words, as
// a seeded ciphertext's block does, so row r's words are [2048 r, 2048 r + 2048) whatever n is.
constexpr uint32_t kStreamSeededKsk = 102;
constexpr uint32_t kStreamSeededBsk = 103;
// Public-key encryption (public_key.h), the same nonce and counter layout.  kStreamPublicKeyMask is keyed by
// the key's PUBLIC seed (mask polynomial A = its first 2048 u64 words).  The two others are keyed by a list's
// SECRET encryption seed: chunk c's binary polynomial R is u64 words [32 c, 32 c + 32) of kStreamCompactBinary,
// its noise words start at u64 word 4096 c of kStreamCompactNoise (2048 for E1, then one per used coefficient).
constexpr uint32_t kStreamPublicKeyMask = 104;
constexpr uint32_t kStreamCompactBinary = 105;
constexpr uint32_t kStreamCompactNoise = 106;
// Mask streams of a seeded compression key (compress.h fhe_seeded_compression_key), keyed by its PUBLIC seed,
// with the seeded server key's row stride: packing-KSK row r's k' N' mask words are u64 words [2048 r, ..),
// the decompression BSK's mask polynomial of GGSW q, row rho is u64 words [2048 (2 q + rho), + 2048).
constexpr uint32_t kStreamSeededPksk = 107;
constexpr uint32_t kStreamSeededCbsk = 108;
// Re-randomization under the public key (public_key.h), keyed by a call's re-randomization seed
// with the compact list's positions: chunk c's R is u64 words [32 c, 32 c + 32) of kStreamRerandBinary, its
// noise words start at u64 word 4096 c of kStreamRerandNoise.  Ids of their own: a seed shared by mistake with
// a compact list's encryption seed (105 / 106) does not make related ciphertexts.
constexpr uint32_t kStreamRerandBinary = 109;
constexpr uint32_t kStreamRerandNoise = 110;
// Oblivious pseudo-random values (oprf.h), keyed by a call's PUBLIC seed: row b's n mask words
// are the first n u64 words of ChaCha blocks [b R, (b + 1) R), R = ceil(n / 8) -- a row starts on a block
// boundary, whatever the workspace's stride or the number of rows is.
constexpr uint32_t kStreamOprf = 111;
// Mask stream of a re-keying key (fhe_rekey_key below), keyed by its PUBLIC seed, with the seeded server key's
// row stride: row r's n_dst mask words are u64 words [2048 r, 2048 r + n_dst) -- launch_expand_ksk serves it
// unchanged under this stream's key.
constexpr uint32_t kStreamRekeyKsk = 112;

}  // namespace fhe

struct fhe_client_key {
    fhe::Params params;
    std::vector<uint64_t> lwe_sk;   // n binary
    std::vector<uint64_t> glwe_sk;  // N binary (= big LWE key)
    fhe::ChaChaStream enc_rng;
};

// A seeded (compressed) fresh ciphertext: tfhe-rs' CompressedFheUint.  Host only, no context.
// Block i's 2048 mask words are u64 words [2048 i, 2048 (i + 1)) of ChaChaStream(bytes_key(seed),
// kStreamSeededMask) -- ChaCha block counter 256 i -- so only the seed and one body word per block are
// kept: body_i = <mask_i, glwe_sk> + delta m_i + e_i.
struct fhe_seeded {
    fhe::Params params;
    uint32_t form = 0;   // FHE_SEEDED_RADIX / FHE_SEEDED_BIGUINT
    uint32_t count = 0;  // num_bits (radix) or nlimbs (BigUintFHE: 16 blocks per limb, limb 0 first)
    uint8_t seed[32] = {};
    std::vector<uint64_t> bodies;  // one per block, LSB block first
};

struct fhe_server_key {
    fhe::Params params;
    std::vector<uint64_t> ksk;  // [N][ks_level][n+1]
    std::vector<uint64_t> bsk;  // [n][row][poly][N] standard domain
};

// A seeded (compressed) server key: tfhe-rs' CompressedServerKey.  Host only.  Of the full key only the
// bodies are kept; every mask word is regenerated from the PUBLIC seed:
//   KSK row r = j ks_level + l: mask word t < n = u64 word 2048 r + t of ChaChaStream(bytes_key(seed),
//       kStreamSeededKsk); ksk_bodies[r] = <mask, lwe_sk> + (S_j << (64 - ks_base_log (l + 1))) + e
//   BSK GGSW q, row rho: mask polynomial A = u64 words [2048 (2 q + rho), + 2048) of stream kStreamSeededBsk;
//       bsk_bodies[(2 q + rho) 2048 ..] = B = A * S + e, then row 1: B[0] += g m_q; row 0: B[t] -= g m_q S_t
//       for every t (g = 1 << (64 - pbs_base_log)).  generate_keys puts row 0's gadget into the mask
//       (A[0] += g); a mask that comes from a seed cannot hold it, and the phase B - A * S = e - g m_q S is
//       the same, so every kernel consumes the expanded key unchanged.
// One seed, one object: a seed is never reused for a second key, or for a seeded ciphertext, under the
// same client key.
struct fhe_seeded_server_key {
    fhe::Params params;
    uint8_t seed[32] = {};
    std::vector<uint64_t> ksk_bodies;  // [N * ks_level]
    std::vector<uint64_t> bsk_bodies;  // [ggsw][row][N]
};

// A re-keying key: tfhe-rs' KeySwitchingKey from the big key of a source client key to the small key of a
// destination client key.  Host only and seeded only (the full form would be 2048 ks_level
// (n_dst + 1) words for nothing).  `params` are the DESTINATION's; the source agrees with them in everything but
// lwe_dimension, lwe_noise_log2 and grouping.  Row r = j ks_level + l:
//   mask word t < n_dst = u64 word 2048 r + t of ChaChaStream(bytes_key(seed), kStreamRekeyKsk)
//   bodies[r] = <mask, dst.lwe_sk> + (src.glwe_sk[j] << (64 - ks_base_log (l + 1))) + e
// With it the keyswitch of a block under the source key is a small LWE row under the destination's: a stored
// value (switched.h) the destination's client key reads and the destination's server key bootstraps.
// One seed, one object: a seed is never reused for a second key, or for a seeded ciphertext, under the same
// client key.
struct fhe_rekey_key {
    fhe::Params params;
    uint8_t seed[32] = {};
    std::vector<uint64_t> bodies;  // [N * ks_level]
};

namespace fhe {
// The re-keying key from src to dst under the public `seed`.  Noise: exactly N ks_level words of dst->enc_rng,
// in row order, drawn before the threaded pass: e = tuniform_of(w, dst lwe_noise_log2).  The caller has checked
// that the two parameter sets agree (rekey_params_differ).
void generate_rekey_key(const fhe_client_key* src, fhe_client_key* dst, const uint8_t seed[32], fhe_rekey_key* out);
// the full KSK of a re-keying key, [N][ks_level][n_dst + 1] in the server key's layout: masks regenerated,
// bodies in place.  The word-for-word definition of the device install (fhe_set_rekey_key).
void expand_rekey_key_host(const fhe_rekey_key& key, std::vector<uint64_t>* ksk);
// the first field a re-keying key's two sides must share in which a and b differ, or null
const char* rekey_params_differ(const Params& a, const Params& b, uint32_t* have, uint32_t* want);
void generate_keys(const Params& p, const KeyWords& key, fhe_client_key* ck, fhe_server_key* sk);
// The seeded server key of ck under the public `seed`.  Noise: exactly N ks_level + ggsw 2 N words of
// ck->enc_rng, the KSK rows' first (row order), then the BSK's in (q, rho, m) order, all drawn before the
// threaded pass: e = tuniform_of(w, lwe_noise_log2) (KSK) / tuniform_of(w, glwe_noise_log2) (BSK).
void generate_seeded_server_key(fhe_client_key* ck, const uint8_t seed[32], fhe_seeded_server_key* out);
// The full key of a seeded one: masks regenerated, bodies in place.  The word-for-word definition of the
// device install (seeded_key.hip).
void expand_seeded_server_key_host(const fhe_seeded_server_key& ssk, fhe_server_key* sk);
// false (with a reason) if a key of these parameters has more rows than the 32-bit block counter of a
// mask stream addresses; Params::from_c admits no such set, readers and the install check anyway
bool seeded_key_rows_ok(const Params& p, const char** why);
// the client-key half of generate_keys (secret keys, encryption stream); the device keygen
// (context.cpp: fhe_generate_keys_device) uses it and derives the server key on the GPU
void generate_secret_keys(const Params& p, const KeyWords& key, fhe_client_key* ck);
void encrypt_big(fhe_client_key* ck, uint64_t plaintext, uint64_t* ct);
// n encryptions (plaintexts already scaled), outputs and stream state identical to n encrypt_big
// calls; large batches run on several host threads over seeked copies of the stream
void encrypt_big_many(fhe_client_key* ck, const uint64_t* plaintexts, size_t n, uint64_t* cts);
// The stream state encrypt_big_many(ck, .., n, ..) leaves, without drawing its words: ck->enc_rng stands after the
// n-th encryption, byte for byte (buffered block included) as that call would leave it on this host.  False, and
// nothing changed, if the batch leaves the stream's counter epoch (encrypt_big_many then runs word by word).
bool encrypt_big_skip(fhe_client_key* ck, size_t n);
// Seeded encryption of n scaled plaintexts: bodies[i] as in fhe_seeded, masks from the PUBLIC `seed`
// (32 bytes), noise e_i = tuniform_of(w_i, glwe_noise_log2) with w_i the next u64 of ck->enc_rng -- exactly
// one stream word per block, in block order, whatever the number of host threads.  n <= kSeededMaxBlocks
// (the caller checks).  A seed must never serve two objects under one client key: equal masks make
// body - body' = delta (m - m') + e - e', which leaks the difference of the messages.
void encrypt_seeded(fhe_client_key* ck, const uint8_t seed[32], const uint64_t* plaintexts, size_t n,
                    uint64_t* bodies);
// The full ciphertexts of a seeded object: cts[i] = mask_i (regenerated) then bodies[i]; n x 2049 words.
// The word-for-word definition of the device expansion (seeded.hip).
void expand_seeded_host(const uint8_t seed[32], const uint64_t* bodies, size_t n, uint64_t* cts);
uint64_t decrypt_phase_big(const fhe_client_key* ck, const uint64_t* ct);
uint64_t decode_block(const Params& p, uint64_t phase);  // value incl. carry, mod msg*carry
}  // namespace fhe
