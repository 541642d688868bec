// compress_host.cpp -- host side of the compressed computed ciphertexts (compress.h): parameters, key
// generation, the packing keyswitch's definition, the wire kinds and the client's direct decryption.
#include "compress.h"

#include <algorithm>
#include <cstring>
#include <memory>
#include <thread>

#include "context.h"
#include "fhe_rocm.h"
#include "serial.h"
#include "capi_internal.h"

namespace fhe {

bool CompParams::from_c(const fhe_compression_params& c, CompParams* out, const char** why) {
    const uint32_t N = c.polynomial_size, k = c.glwe_dimension;
    if (N < 8 || N > 2048 || (N & (N - 1))) {
        *why = "compression polynomial_size must be a power of two in [8, 2048]";
        return false;
    }
    if (k < 1 || k > 8 || k * N > 2048) {
        *why = "compression glwe_dimension must be in [1, 8] with glwe_dimension * polynomial_size <= 2048";
        return false;
    }
    if (c.lwe_per_glwe < 1 || c.lwe_per_glwe > N) {
        *why = "lwe_per_glwe must be in [1, polynomial_size]";
        return false;
    }
    if (c.pks_base_log < 1 || c.pks_base_log > 7) {
        *why = "pks_base_log must be in [1, 7] (digits fit a signed byte)";
        return false;
    }
    if (c.pks_level < 1 || c.pks_base_log * c.pks_level > 32) {
        *why = "pks_level must be >= 1 with pks_base_log * pks_level <= 32";
        return false;
    }
    if (c.pks_noise_log2 > 62) {
        *why = "pks_noise_log2 must be <= 62";
        return false;
    }
    if (c.storage_log_modulus != 12) {
        *why = "storage_log_modulus must be 12 (= log2(2 * 2048): the decompression modulus switch is the identity)";
        return false;
    }
    out->k = k;
    out->N = N;
    out->L = c.lwe_per_glwe;
    out->beta = c.pks_base_log;
    out->ell = c.pks_level;
    out->pks_noise_log2 = c.pks_noise_log2;
    out->storage_log_modulus = 12;
    return true;
}

fhe_compression_params CompParams::to_c() const {
    return fhe_compression_params{k, N, L, beta, ell, pks_noise_log2, storage_log_modulus};
}

bool compressed_nblocks(uint32_t form, uint32_t count, size_t* nblocks, std::string* why) {
    if (form == FHE_SEEDED_RADIX) {
        if (count < 2 || count > FHE_RADIX_MAX_BITS || count % 2) {
            *why = "compressed radix: num_bits must be even, >= 2 and <= FHE_RADIX_MAX_BITS";
            return false;
        }
        *nblocks = count / 2;
        return true;
    }
    if (form == FHE_SEEDED_BIGUINT) {
        if ((uint64_t)count * 16 > kCompressedMaxBlocks) {
            *why = "compressed BigUintFHE: more than 2^24 blocks";
            return false;
        }
        *nblocks = (size_t)count * 16;
        return true;
    }
    *why = "compressed list: unknown form";
    return false;
}

const char* params_differ(const Params& a, const Params& b, uint32_t* have, uint32_t* want) {
    const struct {
        const char* name;
        uint32_t have, want;
    } fields[] = {{"message_modulus", a.message_modulus, b.message_modulus},
                  {"carry_modulus", a.carry_modulus, b.carry_modulus},
                  {"lwe_dimension", a.n, b.n},
                  {"pbs_base_log", a.pbs_base_log, b.pbs_base_log},
                  {"ks_base_log", a.ks_base_log, b.ks_base_log},
                  {"ks_level", a.ks_level, b.ks_level},
                  {"lwe_noise_log2", a.lwe_noise_log2, b.lwe_noise_log2},
                  {"glwe_noise_log2", a.glwe_noise_log2, b.glwe_noise_log2},
                  {"grouping", a.grouping, b.grouping}};
    for (const auto& f : fields)
        if (f.have != f.want) {
            *have = f.have;
            *want = f.want;
            return f.name;
        }
    return nullptr;
}

void assemble_block_values(const std::vector<uint32_t>& vals, uint32_t form, uint64_t* words, size_t nwords) {
    const size_t B = vals.size();
    std::memset(words, 0, nwords * 8);
    const size_t per = form == FHE_SEEDED_RADIX ? B : 16;
    for (size_t base = 0; base < B; base += per ? per : 1) {
        const uint32_t vbits = (uint32_t)(2 * per);
        std::vector<uint64_t> acc(vbits / 64 + 2, 0);
        for (size_t k = 0; k < per; ++k) {
            unsigned __int128 add = (unsigned __int128)vals[base + k] << ((2 * k) % 64);
            for (size_t w = 2 * k / 64; w < acc.size() && add; ++w) {
                const unsigned __int128 s2 = (unsigned __int128)acc[w] + (uint64_t)add;
                acc[w] = (uint64_t)s2;
                add = (add >> 64) + (s2 >> 64);
            }
        }
        for (uint32_t b = 0; b < vbits; ++b)
            if ((acc[b / 64] >> (b % 64)) & 1) {
                const size_t o = 2 * base + b;
                words[o / 64] |= 1ull << (o % 64);
            }
    }
}

namespace {
unsigned pool_size(size_t items) {
    unsigned nth = std::thread::hardware_concurrency();
    if (nth == 0) nth = 4;
    if (nth > 16) nth = 16;
    if (nth > items) nth = items ? (unsigned)items : 1;
    return nth;
}
// fn(i) for i < items, interleaved over at most 16 threads
template <class F>
void parallel_rows(size_t items, F&& fn) {
    const unsigned nth = pool_size(items);
    if (nth <= 1) {
        for (size_t i = 0; i < items; ++i) fn(i);
        return;
    }
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < nth; ++t)
        pool.emplace_back([&, t] {
            for (size_t i = t; i < items; i += nth) fn(i);
        });
    for (auto& th : pool) th.join();
}
// r += a * s mod (X^N + 1), s binary
void negacyclic_binary_mac_n(uint64_t* r, const uint64_t* a, const uint64_t* s, uint32_t N) {
    for (uint32_t j = 0; j < N; ++j) {
        if (!s[j]) continue;
        for (uint32_t m = j; m < N; ++m) r[m] += a[m - j];
        for (uint32_t m = 0; m < j; ++m) r[m] -= a[m + N - j];
    }
}
}  // namespace

void generate_compression_keys(fhe_client_key* ck, const CompParams& cp, fhe_compression_private_key* priv,
                               fhe_compression_key* key) {
    const Params& p = ck->params;
    const uint32_t kN = cp.lwe_dim(), Np = cp.N, cols = cp.cols(), N = kPolySize;
    priv->params = key->params = p;
    priv->cp = key->cp = cp;
    // every stream word first, in the documented order: secret, packing-KSK rows, BSK rows
    priv->sk.resize(kN);
    key->pksk.resize(cp.pksk_words());
    key->bsk.resize(cp.bsk_words());
    ck->enc_rng.fill_u64(priv->sk.data(), kN);
    ck->enc_rng.fill_u64(key->pksk.data(), key->pksk.size());
    ck->enc_rng.fill_u64(key->bsk.data(), key->bsk.size());
    for (auto& v : priv->sk) v &= 1ull;
    const uint64_t *sp = priv->sk.data(), *S = ck->glwe_sk.data();
    parallel_rows((size_t)kBigDim * cp.ell, [&](size_t r) {
        uint64_t* row = key->pksk.data() + r * cols;
        uint64_t* B = row + (size_t)cp.k * Np;
        for (uint32_t m = 0; m < Np; ++m) B[m] = (uint64_t)tuniform_of(B[m], cp.pks_noise_log2);
        for (uint32_t c = 0; c < cp.k; ++c) negacyclic_binary_mac_n(B, row + (size_t)c * Np, sp + (size_t)c * Np, Np);
        const uint32_t j = (uint32_t)(r / cp.ell), l = (uint32_t)(r % cp.ell);
        B[0] += S[j] << (64 - cp.beta * (l + 1));
    });
    parallel_rows((size_t)kN * 2, [&](size_t q) {
        uint64_t* A = key->bsk.data() + (q * 2 + 0) * N;
        uint64_t* B = key->bsk.data() + (q * 2 + 1) * N;
        for (uint32_t m = 0; m < N; ++m) B[m] = (uint64_t)tuniform_of(B[m], p.glwe_noise_log2);
        negacyclic_binary_mac_n(B, A, S, N);
        const uint64_t g = sp[q / 2] << (64 - p.pbs_base_log);
        if (q % 2 == 0) A[0] += g; else B[0] += g;
    });
}

// ------------------------------------------------------------------------- seeded compression key
namespace {
// the seeded server key's row stride (keys.cpp): row r's mask words start at u64 word 2048 r of its stream
constexpr uint64_t kRowWords = 2048;
// fn(row, masks) for row < rows on the pool, `masks` seeked to the row's first word
template <class F>
void seeded_rows(const KeyWords& key, uint32_t stream, size_t rows, F&& fn) {
    parallel_rows(rows, [&](size_t r) {
        ChaChaStream masks(key, stream);
        masks.seek((uint64_t)r * kRowWords * 2);  // in 32-bit stream words
        fn(r, masks);
    });
}
}  // namespace

void generate_seeded_compression_keys(fhe_client_key* ck, const CompParams& cp, const uint8_t seed[32],
                                      fhe_compression_private_key* priv, fhe_seeded_compression_key* out) {
    const Params& p = ck->params;
    const uint32_t kN = cp.lwe_dim(), Np = cp.N, N = kPolySize;
    priv->params = out->params = p;
    priv->cp = out->cp = cp;
    std::memcpy(out->seed, seed, 32);
    // every stream word first, in the documented order: secret, packing-KSK noise, BSK noise
    priv->sk.resize(kN);
    out->pksk_bodies.resize(cp.pksk_body_words());
    out->bsk_bodies.resize(cp.bsk_body_words());
    ck->enc_rng.fill_u64(priv->sk.data(), kN);
    ck->enc_rng.fill_u64(out->pksk_bodies.data(), out->pksk_bodies.size());
    ck->enc_rng.fill_u64(out->bsk_bodies.data(), out->bsk_bodies.size());
    for (auto& v : priv->sk) v &= 1ull;
    const KeyWords key = bytes_key(seed);
    const uint64_t *sp = priv->sk.data(), *S = ck->glwe_sk.data();
    seeded_rows(key, kStreamSeededPksk, (size_t)kBigDim * cp.ell, [&](size_t r, ChaChaStream& masks) {
        std::vector<uint64_t> A(kN);
        masks.fill_u64(A.data(), kN);
        uint64_t* B = out->pksk_bodies.data() + r * Np;
        for (uint32_t m = 0; m < Np; ++m) B[m] = (uint64_t)tuniform_of(B[m], cp.pks_noise_log2);
        for (uint32_t c = 0; c < cp.k; ++c)
            negacyclic_binary_mac_n(B, A.data() + (size_t)c * Np, sp + (size_t)c * Np, Np);
        const uint32_t j = (uint32_t)(r / cp.ell), l = (uint32_t)(r % cp.ell);
        B[0] += S[j] << (64 - cp.beta * (l + 1));
    });
    seeded_rows(key, kStreamSeededCbsk, (size_t)kN * 2, [&](size_t r, ChaChaStream& masks) {
        std::vector<uint64_t> A(N);
        masks.fill_u64(A.data(), N);
        uint64_t* B = out->bsk_bodies.data() + r * N;
        for (uint32_t m = 0; m < N; ++m) B[m] = (uint64_t)tuniform_of(B[m], p.glwe_noise_log2);
        negacyclic_binary_mac_n(B, A.data(), S, N);
        const uint64_t g = sp[r / 2] << (64 - p.pbs_base_log);
        if (r % 2)
            B[0] += g;
        else  // row 0's gadget in body form: a regenerated mask cannot hold it (compress.h)
            for (uint32_t t = 0; t < N; ++t) B[t] -= g * S[t];
    });
}

void expand_seeded_compression_key_host(const fhe_seeded_compression_key& sck, fhe_compression_key* key) {
    const CompParams& cp = sck.cp;
    const uint32_t kN = cp.lwe_dim(), Np = cp.N, cols = cp.cols(), N = kPolySize;
    key->params = sck.params;
    key->cp = cp;
    key->pksk.assign(cp.pksk_words(), 0);
    key->bsk.assign(cp.bsk_words(), 0);
    const KeyWords k = bytes_key(sck.seed);
    seeded_rows(k, kStreamSeededPksk, (size_t)kBigDim * cp.ell, [&](size_t r, ChaChaStream& masks) {
        uint64_t* row = key->pksk.data() + r * cols;
        masks.fill_u64(row, kN);
        std::memcpy(row + kN, sck.pksk_bodies.data() + r * Np, (size_t)Np * 8);
    });
    seeded_rows(k, kStreamSeededCbsk, (size_t)kN * 2, [&](size_t r, ChaChaStream& masks) {
        uint64_t* A = key->bsk.data() + r * 2 * N;
        masks.fill_u64(A, N);
        std::memcpy(A + N, sck.bsk_bodies.data() + r * N, (size_t)N * 8);
    });
}

void pack_keyswitch_host(const fhe_compression_key& key, const uint64_t* cts, size_t B, uint8_t* packed) {
    const CompParams& cp = key.cp;
    const uint32_t Np = cp.N, cols = cp.cols(), kN = cp.lwe_dim(), beta = cp.beta, ell = cp.ell;
    const uint32_t bl = beta * ell;
    const uint64_t vmask = bl == 64 ? ~0ull : (1ull << bl) - 1;
    const int64_t half = 1ll << (beta - 1);
    std::memset(packed, 0, cp.packed_bytes(B));
    std::vector<uint64_t> T((size_t)cp.L * cols), G(cols);
    uint8_t* out = packed;
    for (size_t g = 0; g < cp.glwes(B); ++g) {
        const size_t nb = cp.bodies(B, g);
        parallel_rows(nb, [&](size_t t) {
            const uint64_t* ct = cts + (g * cp.L + t) * kBigCt;
            uint64_t* Ti = T.data() + t * cols;
            std::fill(Ti, Ti + cols, 0ull);
            Ti[(size_t)cp.k * Np] = ct[kBigDim];
            for (uint32_t j = 0; j < kBigDim; ++j) {
                uint64_t v = (((ct[j] >> (63 - bl)) + 1) >> 1) & vmask;  // round to the top beta ell bits
                for (int l = (int)ell - 1; l >= 0; --l) {
                    int64_t d = (int64_t)(v & ((1ull << beta) - 1));
                    v >>= beta;
                    if (d >= half) {
                        d -= 2 * half;
                        v += 1;
                    }
                    if (!d) continue;
                    const uint64_t* row = key.pksk.data() + ((size_t)j * ell + l) * cols;
                    const uint64_t du = (uint64_t)d;
                    for (uint32_t m = 0; m < cols; ++m) Ti[m] -= du * row[m];
                }
            }
        });
        std::fill(G.begin(), G.end(), 0ull);
        for (size_t t = 0; t < nb; ++t)
            for (uint32_t c = 0; c <= cp.k; ++c) {
                const uint64_t* src = T.data() + t * cols + (size_t)c * Np;
                uint64_t* dst = G.data() + (size_t)c * Np;
                for (uint32_t u = (uint32_t)t; u < Np; ++u) dst[u] += src[u - t];
                for (uint32_t u = 0; u < t; ++u) dst[u] -= src[u + Np - t];
            }
        for (size_t i = 0; i < kN + nb; ++i) put12(out, i, (uint32_t)((((G[i] >> 51) + 1) >> 1) & 4095));
        out += cp.glwe_bytes(nb);
    }
}

}  // namespace fhe

using namespace fhe;

namespace {
void write_cp(ser::Writer& w, const CompParams& c) {
    for (uint32_t v : {c.k, c.N, c.L, c.beta, c.ell, c.pks_noise_log2, c.storage_log_modulus}) w.u32(v);
}
bool read_cp(ser::Reader& r, CompParams* out, std::string* why) {
    fhe_compression_params c;
    c.glwe_dimension = r.u32();
    c.polynomial_size = r.u32();
    c.lwe_per_glwe = r.u32();
    c.pks_base_log = r.u32();
    c.pks_level = r.u32();
    c.pks_noise_log2 = r.u32();
    c.storage_log_modulus = r.u32();
    if (!r.ok) {
        *why = "truncated compression parameters";
        return false;
    }
    const char* w = nullptr;
    if (!CompParams::from_c(c, out, &w)) {
        *why = std::string("unsupported compression parameters: ") + w;
        return false;
    }
    return true;
}
bool binary(const std::vector<uint64_t>& v) {
    for (uint64_t x : v)
        if (x > 1) return false;
    return true;
}
}  // namespace

extern "C" {

int fhe_compression_params_default(fhe_compression_params* out) {
    if (!out) return FHE_ERR_INVALID;
    *out = CompParams().to_c();
    return FHE_OK;
}

int fhe_compression_keys_generate(fhe_client_key* ck, const fhe_compression_params* params,
                                  fhe_compression_private_key** priv, fhe_compression_key** key) {
    if (!ck || !priv || !key) return invalid("null argument");
    CompParams cp;
    const char* why = nullptr;
    if (params && !CompParams::from_c(*params, &cp, &why)) {
        set_error(why);
        return FHE_ERR_UNSUPPORTED;
    }
    return guarded_alloc([&] {
        auto a = std::make_unique<fhe_compression_private_key>();
        auto b = std::make_unique<fhe_compression_key>();
        generate_compression_keys(ck, cp, a.get(), b.get());
        *priv = a.release();
        *key = b.release();
        return FHE_OK;
    });
}

int fhe_compression_key_params(const fhe_compression_key* key, fhe_params* main, fhe_compression_params* comp) {
    if (!key) return FHE_ERR_INVALID;
    if (main) *main = key->params.to_c();
    if (comp) *comp = key->cp.to_c();
    return FHE_OK;
}

int fhe_compression_private_key_params(const fhe_compression_private_key* priv, fhe_params* main,
                                       fhe_compression_params* comp) {
    if (!priv) return FHE_ERR_INVALID;
    if (main) *main = priv->params.to_c();
    if (comp) *comp = priv->cp.to_c();
    return FHE_OK;
}

int fhe_compression_key_export(const fhe_compression_key* key, uint64_t* pksk, size_t pksk_len, uint64_t* bsk,
                               size_t bsk_len) {
    if (!key || (pksk && pksk_len < key->pksk.size()) || (bsk && bsk_len < key->bsk.size()))
        return invalid("compression key export: buffer too small");
    if (pksk) std::memcpy(pksk, key->pksk.data(), key->pksk.size() * 8);
    if (bsk) std::memcpy(bsk, key->bsk.data(), key->bsk.size() * 8);
    return FHE_OK;
}

int fhe_compression_private_key_export(const fhe_compression_private_key* priv, uint64_t* sk, size_t len) {
    if (!priv || !sk || len < priv->sk.size()) return invalid("compression private key export: buffer too small");
    std::memcpy(sk, priv->sk.data(), priv->sk.size() * 8);
    return FHE_OK;
}

void fhe_compression_private_key_destroy(fhe_compression_private_key* priv) { delete priv; }
void fhe_compression_key_destroy(fhe_compression_key* key) { delete key; }

int fhe_compression_private_key_serialize(const fhe_compression_private_key* priv, uint8_t* buf, size_t cap,
                                          size_t* len) {
    if (!priv || !len) return FHE_ERR_INVALID;
    return guarded_alloc([&] {
        ser::Writer w;
        w.params(priv->params);
        write_cp(w, priv->cp);
        w.words(priv->sk.data(), priv->sk.size());
        return ser::emit(ser::frame(ser::kCompressionPrivateKey, w.b), buf, cap, len);
    });
}

int fhe_compression_private_key_deserialize(const uint8_t* buf, size_t len, fhe_compression_private_key** out) {
    if (!out) return FHE_ERR_INVALID;
    return guarded_alloc([&] {
        ser::Reader r;
        std::string why;
        Params p;
        CompParams cp;
        if (!ser::unframe(buf, len, ser::kCompressionPrivateKey, &r, &why) || !r.params(&p, &why) ||
            !read_cp(r, &cp, &why))
            return invalid(why);
        if (r.n - r.off != (size_t)cp.lwe_dim() * 8)
            return invalid("compression private key: payload length differs from what its parameters need");
        auto k = std::make_unique<fhe_compression_private_key>();
        k->params = p;
        k->cp = cp;
        k->sk.resize(cp.lwe_dim());
        if (!r.words(k->sk.data(), k->sk.size()) || !r.done() || !binary(k->sk))
            return invalid("malformed compression private key");
        *out = k.release();
        return FHE_OK;
    });
}

int fhe_compression_key_serialize(const fhe_compression_key* key, uint8_t* buf, size_t cap, size_t* len) {
    if (!key || !len) return FHE_ERR_INVALID;
    return guarded_alloc([&] {
        ser::Writer w;
        w.b.reserve(80 + (key->pksk.size() + key->bsk.size()) * 8);
        w.params(key->params);
        write_cp(w, key->cp);
        w.words(key->pksk.data(), key->pksk.size());
        w.words(key->bsk.data(), key->bsk.size());
        return ser::emit(ser::frame(ser::kCompressionKey, w.b), buf, cap, len);
    });
}

int fhe_compression_key_deserialize(const uint8_t* buf, size_t len, fhe_compression_key** out) {
    if (!out) return FHE_ERR_INVALID;
    return guarded_alloc([&] {
        ser::Reader r;
        std::string why;
        Params p;
        CompParams cp;
        if (!ser::unframe(buf, len, ser::kCompressionKey, &r, &why) || !r.params(&p, &why) || !read_cp(r, &cp, &why))
            return invalid(why);
        // the length first: nothing is allocated unless the payload is exactly what the parameters need
        if (r.n - r.off != (cp.pksk_words() + cp.bsk_words()) * 8)
            return invalid("compression key: payload length differs from what its parameters need");
        auto k = std::make_unique<fhe_compression_key>();
        k->params = p;
        k->cp = cp;
        k->pksk.resize(cp.pksk_words());
        k->bsk.resize(cp.bsk_words());
        if (!r.words(k->pksk.data(), k->pksk.size()) || !r.words(k->bsk.data(), k->bsk.size()) || !r.done())
            return invalid("malformed compression key");
        *out = k.release();
        return FHE_OK;
    });
}

// tfhe-rs' CompressedCompressionKey + CompressedDecompressionKey (compress.h fhe_seeded_compression_key).
// Payload of kSeededCompressionKey: params, compression params, 32 seed bytes, the packing-key bodies, the BSK
// body polynomials; no counts -- the parameters fix them.
int fhe_compression_keys_generate_seeded(fhe_client_key* ck, const fhe_compression_params* params,
                                         const uint8_t* mask_seed, fhe_compression_private_key** priv,
                                         fhe_seeded_compression_key** sck) {
    if (!ck || !priv || !sck) return invalid("null argument");
    CompParams cp;
    const char* why = nullptr;
    if (params && !CompParams::from_c(*params, &cp, &why)) {
        set_error(why);
        return FHE_ERR_UNSUPPORTED;
    }
    uint8_t seed[32];
    if (mask_seed) {
        std::memcpy(seed, mask_seed, 32);
    } else if (!os_entropy32(seed)) {
        set_error("getrandom failed: no mask seed");
        return FHE_ERR_UNSUPPORTED;
    }
    return guarded_alloc([&] {
        auto a = std::make_unique<fhe_compression_private_key>();
        auto b = std::make_unique<fhe_seeded_compression_key>();
        generate_seeded_compression_keys(ck, cp, seed, a.get(), b.get());
        *priv = a.release();
        *sck = b.release();
        return FHE_OK;
    });
}

int fhe_seeded_compression_key_params(const fhe_seeded_compression_key* sck, fhe_params* main,
                                      fhe_compression_params* comp) {
    if (!sck) return FHE_ERR_INVALID;
    if (main) *main = sck->params.to_c();
    if (comp) *comp = sck->cp.to_c();
    return FHE_OK;
}

int fhe_seeded_compression_key_serialize(const fhe_seeded_compression_key* sck, uint8_t* buf, size_t cap,
                                         size_t* len) {
    if (!sck || !len) return FHE_ERR_INVALID;
    return guarded_alloc([&] {
        ser::Writer w;
        w.b.reserve(112 + (sck->pksk_bodies.size() + sck->bsk_bodies.size()) * 8);
        w.params(sck->params);
        write_cp(w, sck->cp);
        w.raw(sck->seed, 32);
        w.words(sck->pksk_bodies.data(), sck->pksk_bodies.size());
        w.words(sck->bsk_bodies.data(), sck->bsk_bodies.size());
        return ser::emit(ser::frame(ser::kSeededCompressionKey, w.b), buf, cap, len);
    });
}

int fhe_seeded_compression_key_deserialize(const uint8_t* buf, size_t len, fhe_seeded_compression_key** out) {
    if (!out) return FHE_ERR_INVALID;
    return guarded_alloc([&] {
        ser::Reader r;
        std::string why;
        Params p;
        CompParams cp;
        if (!ser::unframe(buf, len, ser::kSeededCompressionKey, &r, &why) || !r.params(&p, &why) ||
            !read_cp(r, &cp, &why))
            return invalid(why);
        // the length first: nothing is allocated unless the payload is exactly what the parameters need
        if (r.n - r.off != 32 + (cp.pksk_body_words() + cp.bsk_body_words()) * 8)
            return invalid("seeded compression key: payload length differs from what its parameters need");
        auto k = std::make_unique<fhe_seeded_compression_key>();
        k->params = p;
        k->cp = cp;
        k->pksk_bodies.resize(cp.pksk_body_words());
        k->bsk_bodies.resize(cp.bsk_body_words());
        if (!r.take(k->seed, 32) || !r.words(k->pksk_bodies.data(), k->pksk_bodies.size()) ||
            !r.words(k->bsk_bodies.data(), k->bsk_bodies.size()) || !r.done())
            return invalid("malformed seeded compression key");
        *out = k.release();
        return FHE_OK;
    });
}

int fhe_seeded_compression_key_expand_host(const fhe_seeded_compression_key* sck, fhe_compression_key** out) {
    if (!sck || !out) return invalid("null argument");
    if (sck->pksk_bodies.size() != sck->cp.pksk_body_words() || sck->bsk_bodies.size() != sck->cp.bsk_body_words())
        return invalid("seeded compression key: body counts differ from what its parameters need");
    return guarded_alloc([&] {
        auto k = std::make_unique<fhe_compression_key>();
        expand_seeded_compression_key_host(*sck, k.get());
        *out = k.release();
        return FHE_OK;
    });
}

void fhe_seeded_compression_key_destroy(fhe_seeded_compression_key* sck) { delete sck; }

int fhe_compress_host(const fhe_compression_key* key, const uint64_t* cts, size_t nblocks, const uint8_t* degrees,
                      uint32_t form, uint32_t count, fhe_compressed_list** out) {
    if (!key || !out || (nblocks && (!cts || !degrees))) return invalid("null argument to fhe_compress_host");
    std::string why;
    size_t want = 0;
    if (!compressed_nblocks(form, count, &want, &why)) return invalid(why);
    if (want != nblocks) return invalid("fhe_compress_host: nblocks does not match form / count");
    for (size_t i = 0; i < nblocks; ++i)
        if (degrees[i] >= key->params.msg_carry())
            return invalid("fhe_compress_host: block degree >= message_modulus * carry_modulus = " + std::to_string(key->params.msg_carry()));
    return guarded_alloc([&] {
        auto x = std::make_unique<fhe_compressed_list>();
        x->params = key->params;
        x->cp = key->cp;
        x->form = form;
        x->count = count;
        x->degrees.assign(degrees, degrees + nblocks);
        x->packed.resize(key->cp.packed_bytes(nblocks));
        pack_keyswitch_host(*key, cts, nblocks, x->packed.data());
        *out = x.release();
        return FHE_OK;
    });
}

int fhe_compressed_info(const fhe_compressed_list* x, uint32_t* form, uint32_t* count, size_t* nblocks) {
    if (!x) return FHE_ERR_INVALID;
    if (form) *form = x->form;
    if (count) *count = x->count;
    if (nblocks) *nblocks = x->degrees.size();
    return FHE_OK;
}

int fhe_compressed_params(const fhe_compressed_list* x, fhe_params* main, fhe_compression_params* comp) {
    if (!x) return FHE_ERR_INVALID;
    if (main) *main = x->params.to_c();
    if (comp) *comp = x->cp.to_c();
    return FHE_OK;
}

int fhe_compressed_serialize(const fhe_compressed_list* x, uint8_t* buf, size_t cap, size_t* len) {
    if (!x || !len) return FHE_ERR_INVALID;
    return guarded_alloc([&] {
        ser::Writer w;
        w.b.reserve(96 + x->degrees.size() + x->packed.size());
        w.params(x->params);
        write_cp(w, x->cp);
        w.u32(x->form);
        w.u32(x->count);
        w.u32((uint32_t)x->degrees.size());
        w.raw(x->degrees.data(), x->degrees.size());
        w.raw(x->packed.data(), x->packed.size());
        return ser::emit(ser::frame(ser::kCompressedList, w.b), buf, cap, len);
    });
}

int fhe_compressed_deserialize(const uint8_t* buf, size_t len, fhe_compressed_list** out) {
    if (!out) return FHE_ERR_INVALID;
    return guarded_alloc([&] {
        ser::Reader r;
        std::string why;
        Params p;
        CompParams cp;
        if (!ser::unframe(buf, len, ser::kCompressedList, &r, &why) || !r.params(&p, &why) || !read_cp(r, &cp, &why))
            return invalid(why);
        const uint32_t form = r.u32(), count = r.u32(), B = r.u32();
        if (!r.ok) return invalid("truncated compressed list header");
        size_t want = 0;
        if (!compressed_nblocks(form, count, &want, &why)) return invalid(why);
        if (B > kCompressedMaxBlocks) return invalid("compressed list: more than 2^24 blocks");
        if (want != B) return invalid("compressed list: block count does not match form / count");
        // the length first: nothing is allocated for a count the payload does not back
        if (r.n - r.off != (size_t)B + cp.packed_bytes(B))
            return invalid("compressed list: payload length differs from what its parameters and block count need");
        for (size_t i = 0; i < B; ++i)
            if (r.p[r.off + i] >= p.msg_carry())
                return invalid("compressed list: block degree >= message_modulus * carry_modulus = " + std::to_string(p.msg_carry()));
        auto x = std::make_unique<fhe_compressed_list>();
        x->params = p;
        x->cp = cp;
        x->form = form;
        x->count = count;
        x->degrees.resize(B);
        x->packed.resize(cp.packed_bytes(B));
        if (!r.take(x->degrees.data(), B) || !r.take(x->packed.data(), x->packed.size()) || !r.done())
            return invalid("malformed compressed list");
        *out = x.release();
        return FHE_OK;
    });
}

void fhe_compressed_destroy(fhe_compressed_list* x) { delete x; }

int fhe_compressed_decrypt(const fhe_compression_private_key* priv, const fhe_compressed_list* x, uint64_t* words,
                           size_t nwords) {
    if (!priv || !x || !words) return invalid("null argument to fhe_compressed_decrypt");
    if (!(priv->cp == x->cp)) return invalid("compressed list and private key have different compression parameters");
    uint32_t have = 0, want = 0;
    if (const char* f = params_differ(x->params, priv->params, &have, &want))
        return invalid(std::string("compressed list's ") + f + " (" + std::to_string(have) +
                       ") differs from the private key's (" + std::to_string(want) + ")");
    const size_t B = x->degrees.size();
    const uint32_t bits = x->form == FHE_SEEDED_RADIX ? x->count : 32 * x->count;
    if ((uint64_t)nwords * 64 < bits) return invalid("fhe_compressed_decrypt: output too small");
    return guarded_alloc([&] {
        const CompParams& cp = x->cp;
        const uint32_t Np = cp.N, kN = cp.lwe_dim();
        std::vector<uint32_t> vals(B);
        std::vector<uint32_t> A(kN);
        const uint8_t* in = x->packed.data();
        for (size_t g = 0; g < cp.glwes(B); ++g) {
            const size_t nb = cp.bodies(B, g);
            for (uint32_t i = 0; i < kN; ++i) A[i] = get12(in, i);
            for (size_t t = 0; t < nb; ++t) {
                uint32_t ph = get12(in, kN + t);
                for (uint32_t c = 0; c < cp.k; ++c) {
                    const uint32_t* a = A.data() + (size_t)c * Np;
                    const uint64_t* s = priv->sk.data() + (size_t)c * Np;
                    for (uint32_t u = 0; u < Np; ++u) {
                        if (!s[u]) continue;
                        if (u <= t) ph -= a[t - u]; else ph += a[t - u + Np];
                    }
                }
                vals[g * cp.L + t] = (((ph & 4095u) + 64u) >> 7) & 15u;
            }
            in += cp.glwe_bytes(nb);
        }
        assemble_block_values(vals, x->form, words, nwords);
        return FHE_OK;
    });
}

}  // extern "C"
