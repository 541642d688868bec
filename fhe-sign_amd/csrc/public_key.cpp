// public_key.cpp -- host side of public-key encryption (public_key.h): key generation, encryption under the
// public key alone (no client key, no context), the two wire kinds, the host expansion that defines the
// device kernel, and the client's direct decryption.  The products with the binary R and S are exact adds
// of rotated words: no FFT.
#include "public_key.h"

#include <algorithm>
#include <cstring>
#include <memory>
#include <thread>

#include "biguint.h"
#include "context.h"
#include "fhe_rocm.h"
#include "serial.h"
#include "capi_internal.h"

namespace fhe {

namespace {
constexpr uint32_t N = kPolySize;

}  // namespace

void public_key_mask(const uint8_t seed[32], uint64_t* A) {
    ChaChaStream masks(bytes_key(seed), kStreamPublicKeyMask);
    masks.fill_u64(A, N);
}

void generate_public_key(fhe_client_key* ck, const uint8_t seed[32], fhe_public_key* pk) {
    pk->params = ck->params;
    std::memcpy(pk->seed, seed, 32);
    pk->body.resize(N);
    ck->enc_rng.fill_u64(pk->body.data(), N);  // the N stream words first: the stream advances by exactly N u64
    for (uint64_t& w : pk->body) w = (uint64_t)tuniform_of(w, ck->params.glwe_noise_log2);
    std::vector<uint64_t> A(N);
    public_key_mask(seed, A.data());
    const uint64_t* S = ck->glwe_sk.data();
    negacyclic_binary_mac(pk->body.data(), A.data(), [&](uint32_t j) { return S[j] & 1; });
}

bool compact_layout(std::vector<fhe_compact_list::Value>& values, bool packed, size_t* ncoef, std::string* why) {
    size_t at = 0;
    for (size_t i = 0; i < values.size(); ++i) {
        auto& v = values[i];
        const std::string who = "compact list: value " + std::to_string(i) + "'s ";
        if (v.form == FHE_SEEDED_RADIX) {
            if (v.count < 2 || v.count > FHE_RADIX_MAX_BITS || v.count % 2) {
                *why = who + "num_bits must be even, >= 2 and <= FHE_RADIX_MAX_BITS";
                return false;
            }
            v.nblocks = v.count / 2;
        } else if (v.form == FHE_SEEDED_BIGUINT) {
            if ((uint64_t)v.count * kLimbBlocks > kCompactMaxCoefs) {
                *why = who + "nlimbs makes more than 2^24 coefficients";
                return false;
            }
            v.nblocks = (size_t)v.count * kLimbBlocks;
        } else {
            *why = who + "form is unknown";
            return false;
        }
        v.first = at;
        v.ncoef = packed ? (v.nblocks + 1) / 2 : v.nblocks;
        at += v.ncoef;
        if (at > kCompactMaxCoefs) {
            *why = "compact list: more than 2^24 coefficients";
            return false;
        }
    }
    *ncoef = at;
    return true;
}

uint32_t compact_degree(const fhe_compact_list& x, const fhe_compact_list::Value& v, size_t g) {
    if (!x.packed) return 3;
    return 2 * (g - v.first) + 1 < v.nblocks ? 15 : 3;  // an odd last block stands alone
}

void encrypt_compact(const fhe_public_key& pk, const uint8_t enc_seed[32], bool packed,
                     const std::vector<fhe_compact_list::Value>& values, const uint8_t* blocks, fhe_compact_list* out) {
    out->params = pk.params;
    out->packed = packed;
    out->values = values;
    size_t ncoef = 0;
    for (const auto& v : values) ncoef += v.ncoef;
    // the coefficients' plaintexts
    std::vector<uint8_t> m(ncoef);
    size_t b = 0;
    for (const auto& v : values) {
        for (size_t k = 0; k < v.nblocks; ++k) {
            const uint8_t d = blocks[b + k] & 3;
            if (packed)
                m[v.first + k / 2] |= (uint8_t)(d << (2 * (k & 1)));
            else
                m[v.first + k] = d;
        }
        b += v.nblocks;
    }
    const size_t chunks = (ncoef + N - 1) / N;
    out->ca.assign(chunks * N, 0);
    out->cb.assign(ncoef, 0);
    if (!ncoef) return;
    std::vector<uint64_t> A(N);
    public_key_mask(pk.seed, A.data());
    const KeyWords key = bytes_key(enc_seed);
    const uint32_t nb = pk.params.glwe_noise_log2;
    const uint64_t delta = pk.params.delta();
    parallel_chunks(chunks, [&](size_t c) {
        const size_t used = std::min<size_t>(N, ncoef - c * N);
        uint64_t R[N / 64];
        ChaChaStream rs(key, kStreamCompactBinary);
        rs.seek((uint64_t)c * (N / 64) * 2);
        rs.fill_u64(R, N / 64);
        std::vector<uint64_t> noise(N + used), BR(N, 0);
        ChaChaStream ns(key, kStreamCompactNoise);
        ns.seek((uint64_t)c * 2 * N * 2);
        ns.fill_u64(noise.data(), noise.size());
        auto bit = [&](uint32_t j) { return (R[j >> 6] >> (j & 63)) & 1; };
        uint64_t* CA = out->ca.data() + c * N;
        for (uint32_t j = 0; j < N; ++j) CA[j] = (uint64_t)tuniform_of(noise[j], nb);
        negacyclic_binary_mac(CA, A.data(), bit);
        negacyclic_binary_mac(BR.data(), pk.body.data(), bit);
        uint64_t* CB = out->cb.data() + c * N;
        for (size_t j = 0; j < used; ++j)
            CB[j] = BR[j] + (uint64_t)tuniform_of(noise[N + j], nb) + delta * m[c * N + j];
    });
}

void expand_compact_host(const fhe_compact_list& x, size_t first, size_t n, uint64_t* rows) {
    for (size_t i = 0; i < n; ++i) {
        const size_t g = first + i, t = g % N;
        const uint64_t* CA = x.ca.data() + g / N * N;
        uint64_t* row = rows + i * kBigCt;
        for (size_t u = 0; u <= t; ++u) row[u] = CA[t - u];
        for (size_t u = t + 1; u < N; ++u) row[u] = 0 - CA[t - u + N];
        row[N] = x.cb[g];
    }
}

}  // namespace fhe

using namespace fhe;

namespace {
bool seed_or_entropy(const uint8_t* given, uint8_t out[32]) {
    if (given) {
        std::memcpy(out, given, 32);
        return true;
    }
    return os_entropy32(out);
}
}  // namespace

extern "C" {

int fhe_public_key_generate(fhe_client_key* ck, const uint8_t* mask_seed, fhe_public_key** out) {
    if (!ck || !out) return invalid("null argument to fhe_public_key_generate");
    return guarded_alloc([&] {
        uint8_t seed[32];
        if (!seed_or_entropy(mask_seed, seed)) {
            set_error("getrandom failed: no mask seed");
            return (int)FHE_ERR_UNSUPPORTED;
        }
        auto pk = std::make_unique<fhe_public_key>();
        generate_public_key(ck, seed, pk.get());
        *out = pk.release();
        return (int)FHE_OK;
    });
}

int fhe_public_key_params(const fhe_public_key* pk, fhe_params* params) {
    if (!pk || !params) return FHE_ERR_INVALID;
    *params = pk->params.to_c();
    return FHE_OK;
}

int fhe_public_key_export(const fhe_public_key* pk, uint8_t* seed, uint64_t* body, size_t nwords) {
    if (!pk || (body && nwords < kPolySize)) return invalid("public key export: buffer too small (2048 words)");
    if (seed) std::memcpy(seed, pk->seed, 32);
    if (body) std::memcpy(body, pk->body.data(), kPolySize * 8);
    return FHE_OK;
}

int fhe_public_key_serialize(const fhe_public_key* pk, uint8_t* buf, size_t cap, size_t* len) {
    if (!pk || !len) return FHE_ERR_INVALID;
    return guarded_alloc([&] {
        ser::Writer w;
        w.b.reserve(80 + kPolySize * 8);
        w.params(pk->params);
        w.raw(pk->seed, 32);
        w.words(pk->body.data(), pk->body.size());
        return ser::emit(ser::frame(ser::kPublicKey, w.b), buf, cap, len);
    });
}

int fhe_public_key_deserialize(const uint8_t* buf, size_t len, fhe_public_key** out) {
    if (!out) return FHE_ERR_INVALID;
    return guarded_alloc([&] {
        ser::Reader r;
        std::string why;
        Params p;
        if (!ser::unframe(buf, len, ser::kPublicKey, &r, &why) || !r.params(&p, &why)) return invalid(why);
        // the length first: nothing is allocated unless the payload is exactly a seed and N bodies
        if (r.n - r.off != 32 + (size_t)kPolySize * 8)
            return invalid("public key: payload length differs from a seed and 2048 body words");
        auto pk = std::make_unique<fhe_public_key>();
        pk->params = p;
        r.take(pk->seed, 32);
        pk->body.resize(kPolySize);
        if (!r.words(pk->body.data(), kPolySize) || !r.done()) return invalid("malformed public key");
        *out = pk.release();
        return (int)FHE_OK;
    });
}

void fhe_public_key_destroy(fhe_public_key* pk) { delete pk; }

int fhe_compact_builder_new(const fhe_public_key* pk, fhe_compact_builder** out) {
    if (!pk || !out) return invalid("null argument to fhe_compact_builder_new");
    return guarded_alloc([&] {
        auto b = std::make_unique<fhe_compact_builder>();
        b->pk = *pk;
        *out = b.release();
        return (int)FHE_OK;
    });
}

int fhe_compact_builder_push_radix(fhe_compact_builder* b, const uint64_t* words, uint32_t bits) {
    if (!b || !words) return invalid("null argument to fhe_compact_builder_push_radix");
    // a list holds radix values, 2-bit digits (packed: two to a coefficient): refused where the first would be cut
    if (!b->pk.params.radix_space()) return invalid(radix_space_refusal(b->pk.params, "fhe_compact_builder_push_radix"));
    if (bits < 2 || bits > FHE_RADIX_MAX_BITS || bits % 2)
        return invalid("fhe_compact_builder_push_radix: num_bits must be even, >= 2 and <= FHE_RADIX_MAX_BITS");
    if (b->values.size() >= kCompactMaxValues) return invalid("compact list: more than 2^16 values");
    return guarded_alloc([&] {
        fhe_compact_list::Value v;
        v.form = FHE_SEEDED_RADIX;
        v.count = bits;
        b->values.push_back(v);
        for (uint32_t k = 0; k < bits / 2; ++k) b->blocks.push_back((uint8_t)((words[2 * k / 64] >> (2 * k % 64)) & 3));
        return (int)FHE_OK;
    });
}

int fhe_compact_builder_push_biguint(fhe_compact_builder* b, const uint32_t* limbs, size_t n) {
    if (!b || (n && !limbs)) return invalid("null argument to fhe_compact_builder_push_biguint");
    if (!b->pk.params.radix_space()) return invalid(radix_space_refusal(b->pk.params, "fhe_compact_builder_push_biguint"));
    if (n > kCompactMaxCoefs / kLimbBlocks) return invalid("fhe_compact_builder_push_biguint: nlimbs makes more than 2^24 coefficients");
    if (b->values.size() >= kCompactMaxValues) return invalid("compact list: more than 2^16 values");
    return guarded_alloc([&] {
        fhe_compact_list::Value v;
        v.form = FHE_SEEDED_BIGUINT;
        v.count = (uint32_t)n;
        b->values.push_back(v);
        for (size_t i = 0; i < n; ++i)
            for (uint32_t k = 0; k < kLimbBlocks; ++k) b->blocks.push_back((uint8_t)((limbs[i] >> (2 * k)) & 3));
        return (int)FHE_OK;
    });
}

int fhe_compact_builder_build(const fhe_compact_builder* b, int packed, const uint8_t* encryption_seed,
                              fhe_compact_list** out) {
    if (!b || !out) return invalid("null argument to fhe_compact_builder_build");
    return guarded_alloc([&] {
        std::vector<fhe_compact_list::Value> values = b->values;
        std::string why;
        size_t ncoef = 0;
        if (!compact_layout(values, packed != 0, &ncoef, &why)) return invalid(why);
        uint8_t seed[32];
        if (!seed_or_entropy(encryption_seed, seed)) {
            set_error("getrandom failed: no encryption seed");
            return (int)FHE_ERR_UNSUPPORTED;
        }
        auto x = std::make_unique<fhe_compact_list>();
        encrypt_compact(b->pk, seed, packed != 0, values, b->blocks.data(), x.get());
        // the seed gives away R and with it the messages: it is not kept anywhere
        volatile uint8_t* wipe = seed;
        for (int i = 0; i < 32; ++i) wipe[i] = 0;
        *out = x.release();
        return (int)FHE_OK;
    });
}

void fhe_compact_builder_destroy(fhe_compact_builder* b) { delete b; }

int fhe_compact_list_info(const fhe_compact_list* x, int* packed, uint32_t* nvalues, size_t* ncoef, size_t* nchunks) {
    if (!x) return FHE_ERR_INVALID;
    if (packed) *packed = x->packed ? 1 : 0;
    if (nvalues) *nvalues = (uint32_t)x->values.size();
    if (ncoef) *ncoef = x->ncoef();
    if (nchunks) *nchunks = x->nchunks();
    return FHE_OK;
}

int fhe_compact_list_value_info(const fhe_compact_list* x, uint32_t index, uint32_t* form, uint32_t* count,
                                size_t* nblocks, size_t* first_coef, size_t* ncoef) {
    if (!x) return FHE_ERR_INVALID;
    if (index >= x->values.size())
        return invalid("compact list: value index " + std::to_string(index) + " out of range (the list holds " +
                       std::to_string(x->values.size()) + ")");
    const auto& v = x->values[index];
    if (form) *form = v.form;
    if (count) *count = v.count;
    if (nblocks) *nblocks = v.nblocks;
    if (first_coef) *first_coef = v.first;
    if (ncoef) *ncoef = v.ncoef;
    return FHE_OK;
}

int fhe_compact_list_params(const fhe_compact_list* x, fhe_params* params) {
    if (!x || !params) return FHE_ERR_INVALID;
    *params = x->params.to_c();
    return FHE_OK;
}

int fhe_compact_list_export(const fhe_compact_list* x, uint64_t* ca, size_t ca_words, uint64_t* cb, size_t cb_words) {
    if (!x || (ca && ca_words < x->ca.size()) || (cb && cb_words < x->cb.size()))
        return invalid("compact list export: buffer too small");
    if (ca && !x->ca.empty()) std::memcpy(ca, x->ca.data(), x->ca.size() * 8);
    if (cb && !x->cb.empty()) std::memcpy(cb, x->cb.data(), x->cb.size() * 8);
    return FHE_OK;
}

int fhe_compact_list_serialize(const fhe_compact_list* x, uint8_t* buf, size_t cap, size_t* len) {
    if (!x || !len) return FHE_ERR_INVALID;
    return guarded_alloc([&] {
        ser::Writer w;
        w.b.reserve(96 + 8 * (x->values.size() + x->ca.size() + x->cb.size()));
        w.params(x->params);
        w.u32(x->packed ? 1 : 0);
        w.u32((uint32_t)x->values.size());
        for (const auto& v : x->values) {
            w.u32(v.form);
            w.u32(v.count);
        }
        w.words(x->ca.data(), x->ca.size());
        w.words(x->cb.data(), x->cb.size());
        return ser::emit(ser::frame(ser::kCompactList, w.b), buf, cap, len);
    });
}

int fhe_compact_list_deserialize(const uint8_t* buf, size_t len, fhe_compact_list** out) {
    if (!out) return FHE_ERR_INVALID;
    return guarded_alloc([&] {
        ser::Reader r;
        std::string why;
        Params p;
        if (!ser::unframe(buf, len, ser::kCompactList, &r, &why) || !r.params(&p, &why)) return invalid(why);
        if (!p.radix_space()) return invalid(radix_space_refusal(p, "compact list"));
        const uint32_t packed = r.u32(), nvalues = r.u32();
        if (!r.ok) return invalid("truncated compact list header");
        if (packed > 1) return invalid("compact list: the packed flag is neither 0 nor 1");
        if (nvalues > kCompactMaxValues) return invalid("compact list: more than 2^16 values");
        // every count against the payload before anything of its size is allocated
        if ((r.n - r.off) / 8 < nvalues) return invalid("compact list: value count inconsistent with the payload length");
        std::vector<fhe_compact_list::Value> values(nvalues);
        for (auto& v : values) {
            v.form = r.u32();
            v.count = r.u32();
        }
        size_t ncoef = 0;
        if (!compact_layout(values, packed != 0, &ncoef, &why)) return invalid(why);
        const size_t chunks = (ncoef + kPolySize - 1) / kPolySize;
        if (r.n - r.off != (chunks * kPolySize + ncoef) * 8)
            return invalid("compact list: value table inconsistent with the payload length");
        auto x = std::make_unique<fhe_compact_list>();
        x->params = p;
        x->packed = packed != 0;
        x->values = std::move(values);
        x->ca.resize(chunks * kPolySize);
        x->cb.resize(ncoef);
        if (!r.words(x->ca.data(), x->ca.size()) || !r.words(x->cb.data(), ncoef) || !r.done())
            return invalid("malformed compact list");
        *out = x.release();
        return (int)FHE_OK;
    });
}

void fhe_compact_list_destroy(fhe_compact_list* x) { delete x; }

int fhe_compact_list_expand_host(const fhe_compact_list* x, uint64_t* rows, size_t nwords) {
    if (!x || (!rows && x->ncoef()) || nwords < x->ncoef() * kBigCt)
        return invalid("invalid arguments to fhe_compact_list_expand_host (ncoef x 2049 words)");
    return guarded_alloc([&] {
        expand_compact_host(*x, 0, x->ncoef(), rows);
        return (int)FHE_OK;
    });
}

int fhe_compact_list_decrypt(const fhe_client_key* ck, const fhe_compact_list* x, uint32_t index, uint64_t* words,
                             size_t nwords) {
    if (!ck || !x || !words) return invalid("null argument to fhe_compact_list_decrypt");
    if (index >= x->values.size())
        return invalid("compact list: value index " + std::to_string(index) + " out of range (the list holds " +
                       std::to_string(x->values.size()) + ")");
    uint32_t have = 0, want = 0;
    if (const char* f = params_differ(x->params, ck->params, &have, &want))
        return invalid(std::string("compact list's ") + f + " (" + std::to_string(have) + ") differs from the client key's (" +
                       std::to_string(want) + ")");
    const auto& v = x->values[index];
    if (nwords * 64 < 2 * v.nblocks) return invalid("fhe_compact_list_decrypt: output too small");
    return guarded_alloc([&] {
        std::memset(words, 0, nwords * 8);
        const uint64_t* S = ck->glwe_sk.data();
        std::vector<uint64_t> AS(kPolySize);
        size_t have_chunk = (size_t)-1;
        for (size_t q = 0; q < v.ncoef; ++q) {
            const size_t g = v.first + q, c = g / kPolySize;
            if (c != have_chunk) {  // (C_A S) of the chunk: phase_t = C_B[t] - (C_A S)[t]
                std::fill(AS.begin(), AS.end(), 0ull);
                negacyclic_binary_mac(AS.data(), x->ca.data() + c * kPolySize, [&](uint32_t j) { return S[j] & 1; });
                have_chunk = c;
            }
            const uint64_t m = decode_block(x->params, x->cb[g] - AS[g % kPolySize]);
            const size_t k = x->packed ? 2 * q : q;  // the value's block this coefficient starts at
            const uint64_t bits = x->packed && k + 1 < v.nblocks ? (m & 15) : (m & 3);
            words[2 * k / 64] |= bits << (2 * k % 64);  // 2 or 4 bits at an even position: never across a word
        }
        return (int)FHE_OK;
    });
}

}  // extern "C"
