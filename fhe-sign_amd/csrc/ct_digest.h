// ct_digest.h -- SHA-256 digests of ciphertexts and the re-randomization context that derives seeds from them
// (DESIGN.md 6h).  A seed of a re-randomization must not be predictable before the ciphertext is chosen, and
// replicas and ranks must derive the same one: it is a hash of the ciphertexts' own bytes plus domain separators.
//
// Row digest (a row = a big LWE ciphertext, 2049 u64 words, little-endian, 16,392 bytes), a three-level tree
// whose every hash is a tagged hash H_t(m) = SHA-256(T || T || m), T = SHA-256(t), of 5 compressions after the
// tag's midstate:
//   leaf[j]   = H_"fhe-rocm/ct-leaf"(row bytes [256 j, 256 j + 256)),  j < 64 (32 mask words each)
//   node[g]   = H_"fhe-rocm/ct-node"(leaf[8 g] || ... || leaf[8 g + 7]),  g < 8
//   rowdigest = H_"fhe-rocm/ct-row"(node[0] || ... || node[7] || u64le(body))
// Value digest: H_"fhe-rocm/ct-value"(u8 kind || u32le(bits) || u32le(nblocks) || per block u8 tag ||
// u32le(degree) || u32le(noise) || rowdigest).  ct_digest.cpp is the host definition, ct_digest.hip the kernel.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "sha256.h"

namespace fhe {

constexpr const char* kTagCtLeaf = "fhe-rocm/ct-leaf";
constexpr const char* kTagCtNode = "fhe-rocm/ct-node";
constexpr const char* kTagCtRow = "fhe-rocm/ct-row";
constexpr const char* kTagCtValue = "fhe-rocm/ct-value";
constexpr const char* kTagRerandContext = "fhe-rocm/rerandomize-context";
constexpr const char* kTagRerandSeed = "fhe-rocm/rerandomize-seed";
constexpr size_t kCtDigestMaxRows = (size_t)1 << 24;

// the digest of one row of 2049 words
void ct_row_digest_host(const uint64_t* row, uint8_t out[32]);
// rows: n rows of 2049 words; out: 32 bytes per row.  The word-for-word definition of k_ct_digest.
void ct_digest_host(const uint64_t* rows, size_t n, uint8_t* out);
void ct_value_digest_host(uint8_t kind, uint32_t bits, const uint8_t* tags, const uint32_t* degrees, const uint32_t* noises,
                          const uint8_t* rowdigests, size_t nblocks, uint8_t out[32]);

// one block of k_ct_digest's input: the source slot, or null for a trivial block, whose body is tbody
struct CtDigestEntry {
    const uint64_t* src;
    uint64_t tbody;
};
static_assert(sizeof(CtDigestEntry) == 16, "one 16-byte entry per block");

// the chaining values after T || T of the three row-digest tags
struct CtDigestMidstates {
    uint32_t leaf[8], node[8], row[8];
};
const CtDigestMidstates& ct_digest_midstates();

// ct_digest.hip: out[32 i ..] = the row digest of entry i, i < nblocks (out 16-byte aligned); one wave per row
hipError_t launch_ct_digest(const CtDigestEntry* entries, uint8_t* out, uint32_t nblocks, const CtDigestMidstates& mid,
                            hipStream_t s);

}  // namespace fhe

// A running SHA-256 over T_c || T_c || u64le(|domain|) || domain, then items u8 kind || u64le(len) || payload in
// call order; the first seed() finalizes it into `root`
struct fhe_rerand_context {
    fhe::Sha256 h;
    bool finalized = false;
    uint8_t root[32] = {};
};
