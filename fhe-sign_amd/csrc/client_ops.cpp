// client_ops.cpp -- host side of the resident client key (client_ops.h): the residency
// (fhe_ctx_set_client_key and what wipes it), the host definitions the kernels are held against (no context, no
// GPU), and the test and measurement entries that run the kernels over scratch rows.  Engine::encrypt_resident
// and Engine::phases_many (engine_ops.cpp) are the device paths; their routing is in capi_radix.cpp.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "client_ops.h"
#include "client_ops_index.h"
#include "engine.h"
#include "capi_internal.h"

namespace fhe {

using namespace client_ops;

void client_pack_key_bits(const fhe_client_key* ck, uint32_t bits[64]) {
    std::memset(bits, 0, kKeyWords * 4);
    for (uint32_t j = 0; j < kMaskWords && j < ck->glwe_sk.size(); ++j) bits[j >> 5] |= (uint32_t)(ck->glwe_sk[j] & 1ull) << (j & 31u);
}

namespace {
inline uint32_t rotl(uint32_t v, int c) { return (v << c) | (v >> (32 - c)); }
inline void qround(uint32_t& a, uint32_t& b, uint32_t& c, uint32_t& d) {
    a += b; d ^= a; d = rotl(d, 16);
    c += d; b ^= c; b = rotl(b, 12);
    a += b; d ^= a; d = rotl(d, 8);
    c += d; b ^= c; b = rotl(b, 7);
}
// u64 words of ChaCha block `counter` (RFC 8439, the layout of keys.cpp ChaChaStream::refill), by its counter alone
void chacha_block_words(const StreamParams& sp, uint32_t counter, uint64_t out[8]) {
    uint32_t s[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u};
    for (int i = 0; i < 8; ++i) s[4 + i] = sp.key[i];
    s[12] = counter;
    for (int i = 0; i < 3; ++i) s[13 + i] = sp.nonce[i];
    uint32_t x[16];
    std::memcpy(x, s, sizeof s);
    for (int r = 0; r < 10; ++r) {
        qround(x[0], x[4], x[8], x[12]);
        qround(x[1], x[5], x[9], x[13]);
        qround(x[2], x[6], x[10], x[14]);
        qround(x[3], x[7], x[11], x[15]);
        qround(x[0], x[5], x[10], x[15]);
        qround(x[1], x[6], x[11], x[12]);
        qround(x[2], x[7], x[8], x[13]);
        qround(x[3], x[4], x[9], x[14]);
    }
    for (int w = 0; w < 8; ++w) out[w] = (uint64_t)(x[2 * w] + s[2 * w]) | (uint64_t)(x[2 * w + 1] + s[2 * w + 1]) << 32;
}

// the stream as it stands, as the kernel's parameters; false if its position is not a whole u64 word
bool stream_params(const ChaChaStream& at, uint32_t noise_log2, StreamParams* sp) {
    const uint64_t w32 = at.word_pos();
    if (w32 % 2) return false;
    std::memset(sp, 0, sizeof *sp);
    for (int i = 0; i < 8; ++i) sp->key[i] = at.key_words()[i];
    for (int i = 0; i < 3; ++i) sp->nonce[i] = at.nonce_words()[i];
    sp->noise_log2 = noise_log2;
    sp->w0_lo = (uint32_t)(w32 / 2);
    sp->w0_hi = (uint32_t)((w32 / 2) >> 32);
    return true;
}

void wipe(volatile uint32_t* p, size_t words) {
    for (size_t i = 0; i < words; ++i) p[i] = 0;
}
}  // namespace

bool client_encrypt_rows_indexed_host(fhe_client_key* ck, const uint64_t* pts, size_t n, uint64_t* cts) {
    StreamParams sp;
    if (!stream_params(ck->enc_rng, ck->params.glwe_noise_log2, &sp)) throw std::runtime_error("encryption stream off a 64-bit word");
    if (!encrypt_big_skip(ck, n)) return false;
    uint32_t kb[kKeyWords];
    client_pack_key_bits(ck, kb);
    const uint64_t w0 = (uint64_t)sp.w0_lo | (uint64_t)sp.w0_hi << 32;
    for (size_t i = 0; i < n; ++i) {
        uint64_t* row = cts + i * kRowWords;
        const uint64_t g = row_first_word(w0, i);
        const uint32_t unit0 = row_first_unit(g), off = row_offset(g);
        uint64_t dot = 0, noise = 0;
        for (uint32_t t = 0; t < kRowUnits; ++t) {
            uint64_t o[8];
            chacha_block_words(sp, unit0 + t, o);
            const int32_t first = unit_row_word(t, off);
            const uint32_t bits = key_bits8(kb, first);
            for (int w = 0; w < 8; ++w) {
                const int32_t j = first + w;
                if (j >= 0 && j < (int32_t)kMaskWords) row[j] = o[w];
                if (j == (int32_t)kMaskWords) noise = o[w];
                dot += o[w] & (0ull - (uint64_t)((bits >> w) & 1u));
            }
        }
        row[kMaskWords] = dot + pts[i] + tuniform_word(noise, sp.noise_log2);
    }
    wipe(sp.key, 8);
    wipe(kb, kKeyWords);
    return true;
}

}  // namespace fhe

using namespace fhe;
using namespace fhe::client_ops;

bool fhe_ctx::client_resident(const fhe_client_key* ck) const {
    if (!has_client || !ck || ck->glwe_sk.size() != kMaskWords) return false;
    uint32_t kb[kKeyWords], diff = 0;
    client_pack_key_bits(ck, kb);
    for (uint32_t i = 0; i < kKeyWords; ++i) diff |= kb[i] ^ h_client[i];
    wipe(kb, kKeyWords);
    return diff == 0;
}

hipError_t fhe_ctx::client_stage_stream(const ChaChaStream& at, uint32_t noise_log2) {
    StreamParams sp;
    engine_check(stream_params(at, noise_log2, &sp), "encryption stream off a 64-bit word");
    std::memcpy(h_client + kKeyWords, &sp, sizeof sp);
    wipe(sp.key, 8);
    return hipMemcpyAsync(d_client + kKeyWords, h_client + kKeyWords, sizeof sp, hipMemcpyHostToDevice, stream);
}

int fhe_ctx::release_client_key() {
    if (!d_client && !h_client) {
        has_client = false;
        return FHE_OK;
    }
    has_client = false;
    hipError_t e = stream ? hipStreamSynchronize(stream) : hipSuccess;
    // zeros over both copies first, whatever the wait said; then the memory goes back
    if (d_client) {
        const hipError_t z = hipMemset(d_client, 0, d_client.capacity() * 4);
        if (e == hipSuccess) e = z;
    }
    if (h_client) wipe(h_client, h_client.capacity());
    (void)d_client.reset();
    (void)h_client.reset();
    if (e != hipSuccess) {
        set_error(std::string("clearing the resident client key: ") + hipGetErrorString(e));
        return FHE_ERR_HIP;
    }
    return FHE_OK;
}

namespace {
int no_key(const char* why) {
    set_error(why);
    return FHE_ERR_NO_KEY;
}
// the checks every entry that uses the resident key shares
int need_resident(fhe_ctx* c, const char* who) {
    if (const int sim = refuse_simulated(c, who)) return sim;
    if (!c) return invalid(std::string("null context to ") + who);
    if (!c->has_key || !c->engine) return no_key("no server key installed (fhe_set_server_key)");
    if (!c->has_client) return no_key("no client key resident (fhe_ctx_set_client_key)");
    return FHE_OK;
}
// scaled plaintexts of block values, as fhe_encrypt_blocks checks and scales them
int scale_values(const fhe_client_key* ck, const uint64_t* values, size_t n, std::vector<uint64_t>* pts) {
    pts->resize(n);
    for (size_t i = 0; i < n; ++i) {
        if (values[i] >= ck->params.msg_carry()) return invalid("block value out of range");
        (*pts)[i] = values[i] * ck->params.delta();
    }
    return FHE_OK;
}
constexpr size_t kMaxHookRows = (size_t)1 << 20;
}  // namespace

extern "C" {

int fhe_ctx_set_client_key(fhe_ctx* c, const fhe_client_key* ck) {
    if (const int rc = dependent_key_preamble(c, ck != nullptr, "fhe_ctx_set_client_key", ck ? &ck->params : nullptr, "client key"))
        return rc;
    if (ck->glwe_sk.size() != kMaskWords) return invalid("client key: the big secret key is not 2048 bits");
    FHE_HIP_CHECK(hipSetDevice(c->device));
    int rc = c->release_client_key();
    if (rc) return rc;
    auto body = [&]() -> int {
        FHE_HIP_CHECK(c->h_client.grow(kClientWords));
        FHE_HIP_CHECK(c->d_client.grow(kClientWords));
        std::memset(c->h_client, 0, kClientWords * 4);
        client_pack_key_bits(ck, c->h_client);
        FHE_HIP_CHECK(hipMemcpyAsync(c->d_client, c->h_client, kClientWords * 4, hipMemcpyHostToDevice, c->stream));
        FHE_HIP_CHECK(hipStreamSynchronize(c->stream));
        return FHE_OK;
    };
    rc = body();
    if (rc) {
        (void)c->release_client_key();
        return rc;
    }
    c->has_client = true;
    return FHE_OK;
}

int fhe_ctx_clear_client_key(fhe_ctx* c) {
    if (const int sim = refuse_simulated(c, "fhe_ctx_clear_client_key")) return sim;
    if (!c) return invalid("null context to fhe_ctx_clear_client_key");
    if (c->d_client || c->h_client) FHE_HIP_CHECK(hipSetDevice(c->device));
    return c->release_client_key();
}

int fhe_ctx_client_ops_info(fhe_ctx* c, int* resident, uint64_t* enc_blocks, uint64_t* phase_blocks) {
    if (const int sim = refuse_simulated(c, "fhe_ctx_client_ops_info")) return sim;
    if (!c || !resident || !enc_blocks || !phase_blocks) return invalid("null argument to fhe_ctx_client_ops_info");
    *resident = c->has_client ? 1 : 0;
    *enc_blocks = c->client_enc_blocks;
    *phase_blocks = c->client_phase_blocks;
    return FHE_OK;
}

int fhe_client_encrypt_rows_indexed_host(fhe_client_key* ck, const uint64_t* values, size_t n, uint64_t* cts) {
    if (!ck || (n && (!values || !cts))) return invalid("null argument to fhe_client_encrypt_rows_indexed_host");
    std::vector<uint64_t> pts;
    if (const int rc = scale_values(ck, values, n, &pts)) return rc;
    try {
        if (!client_encrypt_rows_indexed_host(ck, pts.data(), n, cts))
            return invalid("fhe_client_encrypt_rows_indexed_host: the batch leaves the stream's counter epoch");
    } catch (const std::exception& e) {
        return invalid(e.what());
    }
    return FHE_OK;
}

int fhe_decrypt_phase_host(const fhe_client_key* ck, const uint64_t* cts, size_t n, uint64_t* phases) {
    if (!ck || (n && (!cts || !phases))) return invalid("null argument to fhe_decrypt_phase_host");
    for (size_t i = 0; i < n; ++i) phases[i] = decrypt_phase_big(ck, cts + i * kBigCt);
    return FHE_OK;
}

int fhe_client_encrypt_rows(fhe_ctx* c, fhe_client_key* ck, const uint64_t* values, size_t n, uint64_t* cts) {
    if (const int rc = need_resident(c, "fhe_client_encrypt_rows")) return rc;
    if (!ck || (n && (!values || !cts))) return invalid("null argument to fhe_client_encrypt_rows");
    if (n > kMaxHookRows) return invalid("fhe_client_encrypt_rows: more than 2^20 rows");
    if (!c->client_resident(ck)) return invalid("fhe_client_encrypt_rows: the client key is not the resident one");
    std::vector<uint64_t> pts;
    if (const int rc = scale_values(ck, values, n, &pts)) return rc;
    if (n == 0) return FHE_OK;
    FHE_HIP_CHECK(hipSetDevice(c->device));
    try {
        const ChaChaStream before = ck->enc_rng;
        engine_check(before.word_pos() % 2 == 0, "encryption stream off a 64-bit word");
        if (!encrypt_big_skip(ck, n)) return invalid("fhe_client_encrypt_rows: the batch leaves the stream's counter epoch");
        DeviceBuf<uint64_t> rows, d_pts;
        DeviceBuf<uint64_t*> d_dst;
        FHE_HIP_CHECK(rows.grow(n * kBigCt));
        FHE_HIP_CHECK(d_pts.grow(n));
        FHE_HIP_CHECK(d_dst.grow(n));
        std::vector<uint64_t*> dst(n);
        for (size_t i = 0; i < n; ++i) dst[i] = rows + i * kBigCt;
        FHE_HIP_CHECK(hipMemcpyAsync(d_pts, pts.data(), n * 8, hipMemcpyHostToDevice, c->stream));
        FHE_HIP_CHECK(hipMemcpyAsync(d_dst, dst.data(), n * sizeof(uint64_t*), hipMemcpyHostToDevice, c->stream));
        FHE_HIP_CHECK(c->client_stage_stream(before, ck->params.glwe_noise_log2));
        FHE_HIP_CHECK(launch_client_encrypt(c->d_client, d_dst, d_pts, n, c->stream));
        FHE_HIP_CHECK(hipMemcpyAsync(cts, rows, n * kBigCt * 8, hipMemcpyDeviceToHost, c->stream));
        FHE_HIP_CHECK(hipStreamSynchronize(c->stream));
        return FHE_OK;
    } catch (const EngineError& e) {
        set_error(e.what());
        return e.code;
    } catch (const std::exception& e) {
        return invalid(e.what());
    }
}

int fhe_client_phase_rows(fhe_ctx* c, const uint64_t* cts, size_t n, uint64_t* phases) {
    if (const int rc = need_resident(c, "fhe_client_phase_rows")) return rc;
    if (n && (!cts || !phases)) return invalid("null argument to fhe_client_phase_rows");
    if (n > kMaxHookRows) return invalid("fhe_client_phase_rows: more than 2^20 rows");
    if (n == 0) return FHE_OK;
    FHE_HIP_CHECK(hipSetDevice(c->device));
    DeviceBuf<uint64_t> rows, d_ph;
    DeviceBuf<const uint64_t*> d_src;
    FHE_HIP_CHECK(rows.grow(n * kBigCt));
    FHE_HIP_CHECK(d_ph.grow(n));
    FHE_HIP_CHECK(d_src.grow(n));
    std::vector<const uint64_t*> src(n);
    for (size_t i = 0; i < n; ++i) src[i] = rows + i * kBigCt;
    FHE_HIP_CHECK(hipMemcpyAsync(rows, cts, n * kBigCt * 8, hipMemcpyHostToDevice, c->stream));
    FHE_HIP_CHECK(hipMemcpyAsync(d_src, src.data(), n * sizeof(uint64_t*), hipMemcpyHostToDevice, c->stream));
    FHE_HIP_CHECK(launch_client_phase(c->d_client, d_src, d_ph, n, c->stream));
    FHE_HIP_CHECK(hipMemcpyAsync(phases, d_ph, n * 8, hipMemcpyDeviceToHost, c->stream));
    FHE_HIP_CHECK(hipStreamSynchronize(c->stream));
    return FHE_OK;
}

int fhe_ctx_time_client_ops(fhe_ctx* c, size_t n, uint32_t iters, float* enc_ms, float* phase_ms) {
    if (const int sim = refuse_simulated(c, "fhe_ctx_time_client_ops")) return sim;
    if (!c || !n || !iters || !enc_ms || !phase_ms) return invalid("invalid argument to fhe_ctx_time_client_ops");
    if (n > kMaxHookRows) return invalid("fhe_ctx_time_client_ops: more than 2^20 rows");
    FHE_HIP_CHECK(hipSetDevice(c->device));
    // a key of its own, public and fixed: the kernels' time does not depend on the bits
    DeviceBuf<uint32_t> client;
    DeviceBuf<uint64_t> rows, aux;
    DeviceBuf<uint64_t*> d_dst;
    FHE_HIP_CHECK(client.grow(kClientWords));
    FHE_HIP_CHECK(rows.grow(n * kBigCt));
    FHE_HIP_CHECK(aux.grow(n));
    FHE_HIP_CHECK(d_dst.grow(n));
    std::vector<uint32_t> h(kClientWords, 0);
    for (uint32_t i = 0; i < kKeyWords + 8; ++i) h[i] = 0x9E3779B9u * (i + 1);
    h[kKeyWords + 8] = kStreamEncrypt;
    h[kKeyWords + 11] = 17;  // noise_log2
    h[kKeyWords + 12] = 3;   // W0: rows at every offset
    std::vector<uint64_t*> dst(n);
    for (size_t i = 0; i < n; ++i) dst[i] = rows + i * kBigCt;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    auto body = [&]() -> int {
        FHE_HIP_CHECK(hipMemcpyAsync(client, h.data(), kClientWords * 4, hipMemcpyHostToDevice, c->stream));
        FHE_HIP_CHECK(hipMemcpyAsync(d_dst, dst.data(), n * sizeof(uint64_t*), hipMemcpyHostToDevice, c->stream));
        FHE_HIP_CHECK(hipMemsetAsync(aux, 0, n * 8, c->stream));
        for (hipEvent_t& e : ev) FHE_HIP_CHECK(hipEventCreate(&e));
        // first touch outside the intervals
        FHE_HIP_CHECK(launch_client_encrypt(client, d_dst, aux, n, c->stream));
        FHE_HIP_CHECK(launch_client_phase(client, (const uint64_t* const*)d_dst.get(), aux, n, c->stream));
        FHE_HIP_CHECK(hipMemsetAsync(aux, 0, n * 8, c->stream));
        FHE_HIP_CHECK(hipEventRecord(ev[0], c->stream));
        for (uint32_t r = 0; r < iters; ++r) FHE_HIP_CHECK(launch_client_encrypt(client, d_dst, aux, n, c->stream));
        FHE_HIP_CHECK(hipEventRecord(ev[1], c->stream));
        for (uint32_t r = 0; r < iters; ++r)
            FHE_HIP_CHECK(launch_client_phase(client, (const uint64_t* const*)d_dst.get(), aux, n, c->stream));
        FHE_HIP_CHECK(hipEventRecord(ev[2], c->stream));
        FHE_HIP_CHECK(hipEventSynchronize(ev[2]));
        float a = 0.f, b = 0.f;
        FHE_HIP_CHECK(hipEventElapsedTime(&a, ev[0], ev[1]));
        FHE_HIP_CHECK(hipEventElapsedTime(&b, ev[1], ev[2]));
        *enc_ms = a / (float)iters;
        *phase_ms = b / (float)iters;
        return FHE_OK;
    };
    const int r = body();
    (void)hipStreamSynchronize(c->stream);  // nothing queued reads the buffers when they go
    for (hipEvent_t e : ev)
        if (e) (void)hipEventDestroy(e);
    return r;
}

}  // extern "C"
