// switched.cpp -- host side of the modulus-switched stored ciphertexts (switched.h): the word-for-word
// definitions of the stored rows (no context, no GPU), the list's wire kind and the client's direct decryption,
// and the test and measurement entries that run the two kernels of switched.hip over scratch buffers.
// Engine::switched_compress / switched_decompress (engine_ops.cpp) are the device path; the radix entries are in
// capi_radix.cpp.
#include "switched.h"

#include <algorithm>
#include <cstring>
#include <memory>
#include <thread>

#include "compress.h"
#include "context.h"
#include "fhe_rocm.h"
#include "oprf.h"
#include "serial.h"
#include "capi_internal.h"

namespace fhe {

void ms_center_host(uint64_t* rows, size_t count, uint32_t n, size_t stride);  // ms_center.cpp

void switched_pack_host(const uint64_t* rows, size_t count, uint32_t n, size_t stride, uint8_t* out, size_t out_stride) {
    const size_t bytes = switched_row_bytes(n);
    for (size_t b = 0; b < count; ++b) {
        uint8_t* o = out + b * out_stride;
        std::memset(o, 0, bytes);
        const uint64_t* r = rows + b * stride;
        for (uint32_t t = 0; t <= n; ++t) put12(o, t, (uint32_t)((((r[t] >> 51) + 1) >> 1) & 4095));
    }
}

void switched_unpack_host(const uint8_t* packed, size_t count, uint32_t n, size_t in_stride, uint64_t* rows, size_t stride) {
    for (size_t b = 0; b < count; ++b) {
        const uint8_t* in = packed + b * in_stride;
        uint64_t* r = rows + b * stride;
        // get12 reads bytes 3 t / 2 and the next: the last of them is byte row_bytes(n) - 1 for either parity of n + 1
        for (uint32_t t = 0; t <= n; ++t) r[t] = (uint64_t)get12(in, t) << 52;
        for (size_t j = (size_t)n + 1; j < stride; ++j) r[j] = kMsPadWord;
    }
}

void keyswitch_host(const Params& p, const uint64_t* ksk, const uint64_t* ct, uint64_t* out) {
    const uint32_t n = p.n, L = p.ks_level, bl = p.ks_base_log, bits = bl * L;
    const uint64_t mask = (1ull << bits) - 1;
    const int64_t base = 1ll << bl, halfb = base >> 1;
    std::fill(out, out + n, 0ull);
    out[n] = ct[kBigDim];
    for (uint32_t j = 0; j < kBigDim; ++j) {
        uint64_t v = (((ct[j] >> (63 - bits)) + 1) >> 1) & mask;  // round to the top `bits` bits
        for (int l = (int)L - 1; l >= 0; --l) {
            int64_t d = (int64_t)(v & (uint64_t)(base - 1));
            v >>= bl;
            if (d >= halfb) {
                d -= base;
                v += 1;
            }
            if (!d) continue;
            const uint64_t* row = ksk + ((size_t)j * L + l) * (n + 1);
            const uint64_t du = (uint64_t)d;
            for (uint32_t t = 0; t <= n; ++t) out[t] -= du * row[t];
        }
    }
}

}  // namespace fhe

using namespace fhe;

namespace {
int check_rows(const char* who, uint32_t n, size_t count, size_t stride, size_t byte_stride) {
    if (n < 1 || n > kBigDim) return invalid(std::string(who) + ": n must be 1 .. 2048");
    if (stride < (size_t)n + 1) return invalid(std::string(who) + ": stride must be at least n + 1 words");
    if (byte_stride < switched_row_bytes(n)) return invalid(std::string(who) + ": a packed row is ceil(12 (n + 1) / 8) bytes");
    if (count > kCompressedMaxBlocks) return invalid(std::string(who) + ": more than 2^24 rows");
    return FHE_OK;
}
// the pad nibble of an odd n + 1 is zero in every row
bool pads_zero(const uint8_t* rows, size_t count, uint32_t n) {
    if (((size_t)n + 1) % 2 == 0) return true;
    const size_t bytes = switched_row_bytes(n);
    for (size_t b = 0; b < count; ++b)
        if (rows[b * bytes + bytes - 1] >> 4) return false;
    return true;
}
// the marker a hook's device scratch holds before its kernel runs, and the guard behind it that must survive
constexpr int kScratchByte = 0x5C;
constexpr size_t kGuardBytes = 256;
bool guard_intact(const uint8_t* g) {
    for (size_t i = 0; i < kGuardBytes; ++i)
        if (g[i] != kScratchByte) return false;
    return true;
}
}  // namespace

extern "C" {

int fhe_switched_pack_host(const uint64_t* rows, size_t count, uint32_t n, size_t stride, uint8_t* out, size_t out_stride) {
    if (count && (!rows || !out)) return invalid("null argument to fhe_switched_pack_host");
    if (const int rc = check_rows("fhe_switched_pack_host", n, count, stride, out_stride)) return rc;
    switched_pack_host(rows, count, n, stride, out, out_stride);
    return FHE_OK;
}

int fhe_switched_unpack_host(const uint8_t* packed, size_t count, uint32_t n, size_t in_stride, uint64_t* rows, size_t stride) {
    if (count && (!rows || !packed)) return invalid("null argument to fhe_switched_unpack_host");
    if (const int rc = check_rows("fhe_switched_unpack_host", n, count, stride, in_stride)) return rc;
    switched_unpack_host(packed, count, n, in_stride, rows, stride);
    return FHE_OK;
}

}  // extern "C"

namespace {
// fhe_switched_compress_host under any KSK of the server key's layout: p = the parameters of the rows' key
int compress_host(const Params& p, const std::vector<uint64_t>& ksk, int ms_mode, const uint64_t* cts, size_t nblocks,
                  const uint8_t* degrees, uint32_t form, uint32_t count, fhe_switched_list** out) {
    if (!out || (nblocks && (!cts || !degrees))) return invalid("null argument to fhe_switched_compress_host");
    if (ms_mode != FHE_MS_STANDARD && ms_mode != FHE_MS_CENTERED)
        return invalid("fhe_switched_compress_host: unknown modulus switch mode " + std::to_string(ms_mode));
    std::string why;
    size_t want = 0;
    if (!compressed_nblocks(form, count, &want, &why)) return invalid(why);
    if (want != nblocks) return invalid("fhe_switched_compress_host: nblocks does not match form / count");
    for (size_t i = 0; i < nblocks; ++i)
        if (degrees[i] >= p.msg_carry())
            return invalid("fhe_switched_compress_host: block degree >= message_modulus * carry_modulus = " + std::to_string(p.msg_carry()));
    if (ksk.size() != (size_t)kBigDim * p.ks_level * (p.n + 1))
        return invalid("fhe_switched_compress_host: the KSK does not match its parameters");
    return guarded_alloc([&] {
        auto x = std::make_unique<fhe_switched_list>();
        x->params = p;
        x->form = form;
        x->count = count;
        x->degrees.assign(degrees, degrees + nblocks);
        const size_t bytes = switched_row_bytes(p.n);
        x->rows.resize(nblocks * bytes);
        // every block alone: the result does not depend on the thread count
        unsigned nth = std::min<size_t>(std::min(16u, std::max(1u, std::thread::hardware_concurrency())), std::max<size_t>(nblocks, 1));
        auto work = [&](unsigned t) {
            std::vector<uint64_t> row(p.n + 1);
            for (size_t i = t; i < nblocks; i += nth) {
                keyswitch_host(p, ksk.data(), cts + i * kBigCt, row.data());
                if (ms_mode == FHE_MS_CENTERED) ms_center_host(row.data(), 1, p.n, p.n + 1);
                switched_pack_host(row.data(), 1, p.n, p.n + 1, x->rows.data() + i * bytes, bytes);
            }
        };
        if (nth <= 1) {
            work(0);
        } else {
            std::vector<std::thread> pool;
            for (unsigned t = 0; t < nth; ++t) pool.emplace_back(work, t);
            for (auto& th : pool) th.join();
        }
        *out = x.release();
        return FHE_OK;
    });
}
}  // namespace

extern "C" {

int fhe_switched_compress_host(const fhe_server_key* sk, int ms_mode, const uint64_t* cts, size_t nblocks,
                               const uint8_t* degrees, uint32_t form, uint32_t count, fhe_switched_list** out) {
    if (!sk) return invalid("null argument to fhe_switched_compress_host");
    return compress_host(sk->params, sk->ksk, ms_mode, cts, nblocks, degrees, form, count, out);
}

int fhe_switched_compress_host_rekeyed(const fhe_rekey_key* key, int ms_mode, const uint64_t* cts, size_t nblocks,
                                       const uint8_t* degrees, uint32_t form, uint32_t count, fhe_switched_list** out) {
    if (!key) return invalid("null argument to fhe_switched_compress_host_rekeyed");
    return guarded_alloc([&] {
        std::vector<uint64_t> ksk;
        expand_rekey_key_host(*key, &ksk);
        return compress_host(key->params, ksk, ms_mode, cts, nblocks, degrees, form, count, out);
    });
}

// ------------------------------------------------------------------ the re-keying key (keys.h fhe_rekey_key)
int fhe_rekey_key_generate(const fhe_client_key* src, fhe_client_key* dst, const uint8_t* mask_seed, fhe_rekey_key** out) {
    if (!src || !dst || !out) return invalid("null argument to fhe_rekey_key_generate");
    uint32_t have = 0, want = 0;
    if (const char* f = rekey_params_differ(src->params, dst->params, &have, &want))
        return invalid(std::string("fhe_rekey_key_generate: the source key's ") + f + " (" + std::to_string(have) +
                       ") differs from the destination's (" + std::to_string(want) + ")");
    const char* why = nullptr;
    if (!seeded_key_rows_ok(dst->params, &why)) {
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
        auto k = std::make_unique<fhe_rekey_key>();
        generate_rekey_key(src, dst, seed, k.get());
        *out = k.release();
        return FHE_OK;
    });
}

int fhe_rekey_key_params(const fhe_rekey_key* key, fhe_params* out) {
    if (!key || !out) return FHE_ERR_INVALID;
    *out = key->params.to_c();
    return FHE_OK;
}

int fhe_rekey_key_serialize(const fhe_rekey_key* key, uint8_t* buf, size_t cap, size_t* len) {
    if (!key || !len) return FHE_ERR_INVALID;
    return guarded_alloc([&] {
        ser::Writer w;
        w.b.reserve(80 + key->bodies.size() * 8);
        w.params(key->params);
        w.raw(key->seed, 32);
        w.words(key->bodies.data(), key->bodies.size());
        return ser::emit(ser::frame(ser::kRekeyKey, w.b), buf, cap, len);
    });
}

int fhe_rekey_key_deserialize(const uint8_t* buf, size_t len, fhe_rekey_key** out) {
    if (!out) return FHE_ERR_INVALID;
    return guarded_alloc([&] {
        ser::Reader r;
        std::string why;
        Params p;
        if (!ser::unframe(buf, len, ser::kRekeyKey, &r, &why) || !r.params(&p, &why)) return invalid(why);
        const char* w = nullptr;
        if (!seeded_key_rows_ok(p, &w)) return invalid(w);
        // the length first: nothing is allocated unless the payload is exactly what the parameters need
        const size_t rows = (size_t)kPolySize * p.ks_level;
        if (r.n - r.off != 32 + rows * 8) return invalid("re-keying key: payload length differs from what its parameters need");
        auto k = std::make_unique<fhe_rekey_key>();
        k->params = p;
        k->bodies.resize(rows);
        if (!r.take(k->seed, 32) || !r.words(k->bodies.data(), rows) || !r.done()) return invalid("malformed re-keying key");
        *out = k.release();
        return FHE_OK;
    });
}

int fhe_rekey_key_expand_host(const fhe_rekey_key* key, uint64_t* ksk, size_t len) {
    if (!key || !ksk) return invalid("null argument to fhe_rekey_key_expand_host");
    const size_t need = (size_t)kPolySize * key->params.ks_level * (key->params.n + 1);
    if (len < need || key->bodies.size() != (size_t)kPolySize * key->params.ks_level)
        return invalid("fhe_rekey_key_expand_host: buffer too small");
    return guarded_alloc([&] {
        std::vector<uint64_t> v;
        expand_rekey_key_host(*key, &v);
        std::memcpy(ksk, v.data(), need * 8);
        return FHE_OK;
    });
}

void fhe_rekey_key_destroy(fhe_rekey_key* key) { delete key; }

int fhe_switched_list_info(const fhe_switched_list* x, uint32_t* form, uint32_t* count, size_t* nblocks) {
    if (!x) return FHE_ERR_INVALID;
    if (form) *form = x->form;
    if (count) *count = x->count;
    if (nblocks) *nblocks = x->degrees.size();
    return FHE_OK;
}

int fhe_switched_list_params(const fhe_switched_list* x, fhe_params* main) {
    if (!x || !main) return FHE_ERR_INVALID;
    *main = x->params.to_c();
    return FHE_OK;
}

int fhe_switched_list_serialize(const fhe_switched_list* x, uint8_t* buf, size_t cap, size_t* len) {
    if (!x || !len) return FHE_ERR_INVALID;
    return guarded_alloc([&] {
        ser::Writer w;
        w.b.reserve(64 + x->degrees.size() + x->rows.size());
        w.params(x->params);
        w.u32(x->form);
        w.u32(x->count);
        w.u32((uint32_t)x->degrees.size());
        w.raw(x->degrees.data(), x->degrees.size());
        w.raw(x->rows.data(), x->rows.size());
        return ser::emit(ser::frame(ser::kSwitchedList, w.b), buf, cap, len);
    });
}

int fhe_switched_list_deserialize(const uint8_t* buf, size_t len, fhe_switched_list** out) {
    if (!out) return FHE_ERR_INVALID;
    return guarded_alloc([&] {
        ser::Reader r;
        std::string why;
        Params p;
        if (!ser::unframe(buf, len, ser::kSwitchedList, &r, &why) || !r.params(&p, &why)) return invalid(why);
        const uint32_t form = r.u32(), count = r.u32(), B = r.u32();
        if (!r.ok) return invalid("truncated switched list header");
        size_t want = 0;
        if (!compressed_nblocks(form, count, &want, &why)) return invalid(why);
        if (B > kCompressedMaxBlocks) return invalid("switched list: more than 2^24 blocks");
        if (want != B) return invalid("switched list: block count does not match form / count");
        // the length first: nothing is allocated for a count the payload does not back
        const size_t bytes = switched_row_bytes(p.n);
        if (r.n - r.off != (size_t)B * (1 + bytes))
            return invalid("switched list: payload length differs from what its parameters and block count need");
        for (size_t i = 0; i < B; ++i)
            if (r.p[r.off + i] >= p.msg_carry())
                return invalid("switched list: block degree >= message_modulus * carry_modulus = " + std::to_string(p.msg_carry()));
        if (!pads_zero(r.p + r.off + B, B, p.n)) return invalid("switched list: non-zero pad bits in a row");
        auto x = std::make_unique<fhe_switched_list>();
        x->params = p;
        x->form = form;
        x->count = count;
        x->degrees.resize(B);
        x->rows.resize((size_t)B * bytes);
        if (!r.take(x->degrees.data(), B) || !r.take(x->rows.data(), x->rows.size()) || !r.done())
            return invalid("malformed switched list");
        *out = x.release();
        return FHE_OK;
    });
}

void fhe_switched_list_destroy(fhe_switched_list* x) { delete x; }

int fhe_switched_decrypt(const fhe_client_key* ck, const fhe_switched_list* x, uint64_t* words, size_t nwords) {
    if (!ck || !x || !words) return invalid("null argument to fhe_switched_decrypt");
    uint32_t have = 0, want = 0;
    if (const char* f = params_differ(x->params, ck->params, &have, &want))
        return invalid(std::string("switched list's ") + f + " (" + std::to_string(have) + ") differs from the client key's (" +
                       std::to_string(want) + ")");
    const uint32_t bits = x->form == FHE_SEEDED_RADIX ? x->count : 32 * x->count;
    if ((uint64_t)nwords * 64 < bits) return invalid("fhe_switched_decrypt: output too small");
    return guarded_alloc([&] {
        const uint32_t n = x->params.n;
        const size_t B = x->degrees.size(), bytes = switched_row_bytes(n);
        std::vector<uint32_t> vals(B);
        std::vector<uint64_t> row(n + 1);
        for (size_t i = 0; i < B; ++i) {
            switched_unpack_host(x->rows.data() + i * bytes, 1, n, bytes, row.data(), n + 1);
            uint32_t ph = (uint32_t)(row[n] >> 52);
            for (uint32_t t = 0; t < n; ++t)
                if (ck->lwe_sk[t]) ph -= (uint32_t)(row[t] >> 52);
            vals[i] = (((ph & 4095u) + 64u) >> 7) & 15u;
        }
        assemble_block_values(vals, x->form, words, nwords);
        return FHE_OK;
    });
}

int fhe_switched_pack_rows(fhe_ctx* c, const uint64_t* rows, size_t count, uint32_t n, size_t stride, uint8_t* out,
                           size_t out_stride) {
    if (!c || (count && (!rows || !out))) return invalid("null argument to fhe_switched_pack_rows");
    if (const int rc = check_rows("fhe_switched_pack_rows", n, count, stride, out_stride)) return rc;
    if (count == 0) return FHE_OK;
    FHE_HIP_CHECK(hipSetDevice(c->device));
    // the kernel reads the workspace's layout: the caller's words 0 .. n of every row go there, the padding keeps
    // the scratch marker (a kernel that read it would pack it)
    const size_t ws = ms_stride_words(n), dev_bytes = switched_dev_row_bytes(n);
    DeviceBuf<uint64_t> d_rows;
    DeviceBuf<uint8_t> d_out;
    FHE_HIP_CHECK(d_rows.grow(count * ws));
    FHE_HIP_CHECK(d_out.grow(count * dev_bytes + kGuardBytes));
    FHE_HIP_CHECK(hipMemsetAsync(d_rows, kScratchByte, count * ws * 8, c->stream));
    FHE_HIP_CHECK(hipMemsetAsync(d_out, kScratchByte, count * dev_bytes + kGuardBytes, c->stream));
    FHE_HIP_CHECK(hipMemcpy2DAsync(d_rows, ws * 8, rows, stride * 8, ((size_t)n + 1) * 8, count, hipMemcpyHostToDevice, c->stream));
    FHE_HIP_CHECK(launch_ms_pack(d_rows, reinterpret_cast<uint32_t*>(d_out.get()), count, n, c->stream));
    uint8_t guard[kGuardBytes];
    FHE_HIP_CHECK(hipMemcpy2DAsync(out, out_stride, d_out, dev_bytes, switched_row_bytes(n), count, hipMemcpyDeviceToHost, c->stream));
    FHE_HIP_CHECK(hipMemcpyAsync(guard, d_out.get() + count * dev_bytes, kGuardBytes, hipMemcpyDeviceToHost, c->stream));
    FHE_HIP_CHECK(hipStreamSynchronize(c->stream));
    if (!guard_intact(guard)) return invalid("fhe_switched_pack_rows: the kernel wrote behind its last row");
    return FHE_OK;
}

int fhe_switched_unpack_rows(fhe_ctx* c, const uint8_t* packed, size_t count, uint32_t n, size_t in_stride, uint64_t* rows,
                             size_t stride) {
    if (!c || (count && (!rows || !packed))) return invalid("null argument to fhe_switched_unpack_rows");
    if (const int rc = check_rows("fhe_switched_unpack_rows", n, count, stride, in_stride)) return rc;
    if (count == 0) return FHE_OK;
    FHE_HIP_CHECK(hipSetDevice(c->device));
    // the kernel writes the workspace's layout; the caller's stride gets each row's first min(stride, ws) words,
    // and whatever lies above them the marker (fhe_oprf_rows)
    const size_t ws = ms_stride_words(n), dev_bytes = switched_dev_row_bytes(n);
    DeviceBuf<uint8_t> d_in;
    DeviceBuf<uint64_t> d_rows;
    FHE_HIP_CHECK(d_in.grow(count * dev_bytes));
    FHE_HIP_CHECK(d_rows.grow(count * ws + kGuardBytes / 8));
    FHE_HIP_CHECK(hipMemsetAsync(d_in, kScratchByte, count * dev_bytes, c->stream));
    FHE_HIP_CHECK(hipMemsetAsync(d_rows, kScratchByte, count * ws * 8 + kGuardBytes, c->stream));
    FHE_HIP_CHECK(hipMemcpy2DAsync(d_in, dev_bytes, packed, in_stride, switched_row_bytes(n), count, hipMemcpyHostToDevice, c->stream));
    FHE_HIP_CHECK(launch_ms_unpack(reinterpret_cast<const uint32_t*>(d_in.get()), d_rows, count, n, c->stream));
    if (stride > ws)
        for (size_t b = 0; b < count; ++b) std::fill(rows + b * stride + ws, rows + (b + 1) * stride, kMsPadWord);
    uint8_t guard[kGuardBytes];
    FHE_HIP_CHECK(hipMemcpy2DAsync(rows, stride * 8, d_rows, ws * 8, std::min(stride, ws) * 8, count, hipMemcpyDeviceToHost, c->stream));
    FHE_HIP_CHECK(hipMemcpyAsync(guard, d_rows.get() + count * ws, kGuardBytes, hipMemcpyDeviceToHost, c->stream));
    FHE_HIP_CHECK(hipStreamSynchronize(c->stream));
    if (!guard_intact(guard)) return invalid("fhe_switched_unpack_rows: the kernel wrote behind its last row");
    return FHE_OK;
}

int fhe_ctx_time_switched(fhe_ctx* c, size_t count, uint32_t n, uint32_t reps, float* pack_ms, float* unpack_ms) {
    if (!c || !pack_ms || !unpack_ms || !reps || !count) return invalid("invalid argument to fhe_ctx_time_switched");
    if (const int rc = check_rows("fhe_ctx_time_switched", n, count, (size_t)n + 1, switched_row_bytes(n))) return rc;
    FHE_HIP_CHECK(hipSetDevice(c->device));
    DeviceBuf<uint64_t> d_rows;
    DeviceBuf<uint32_t> d_packed;
    FHE_HIP_CHECK(d_rows.grow(count * ms_stride_words(n)));
    FHE_HIP_CHECK(d_packed.grow(count * switched_dev_row_bytes(n) / 4));
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    auto body = [&]() -> int {
        FHE_HIP_CHECK(hipMemsetAsync(d_rows, 0x5A, count * ms_stride_words(n) * 8, c->stream));
        for (hipEvent_t& e : ev) FHE_HIP_CHECK(hipEventCreate(&e));
        // first touch of both buffers outside the intervals
        FHE_HIP_CHECK(launch_ms_pack(d_rows, d_packed, count, n, c->stream));
        FHE_HIP_CHECK(launch_ms_unpack(d_packed, d_rows, count, n, c->stream));
        FHE_HIP_CHECK(hipEventRecord(ev[0], c->stream));
        for (uint32_t r = 0; r < reps; ++r) FHE_HIP_CHECK(launch_ms_pack(d_rows, d_packed, count, n, c->stream));
        FHE_HIP_CHECK(hipEventRecord(ev[1], c->stream));
        for (uint32_t r = 0; r < reps; ++r) FHE_HIP_CHECK(launch_ms_unpack(d_packed, d_rows, count, n, c->stream));
        FHE_HIP_CHECK(hipEventRecord(ev[2], c->stream));
        FHE_HIP_CHECK(hipEventSynchronize(ev[2]));
        float a = 0.f, b = 0.f;
        FHE_HIP_CHECK(hipEventElapsedTime(&a, ev[0], ev[1]));
        FHE_HIP_CHECK(hipEventElapsedTime(&b, ev[1], ev[2]));
        *pack_ms = a / (float)reps;
        *unpack_ms = b / (float)reps;
        return FHE_OK;
    };
    const int r = body();
    for (hipEvent_t e : ev)
        if (e) (void)hipEventDestroy(e);
    return r;
}

}  // extern "C"
