// oprf.cpp -- host side of the oblivious pseudo-random values (oprf.h): the word-for-word
// definitions of the rows and of the accumulator (no context, no GPU), the accumulator's place in the context's
// LUT registry, and the test and measurement entries that run the row kernel over a scratch buffer or hand
// back raw blocks.  Engine::oprf (engine_ops.cpp) is the device path; the radix entries are in capi_radix.cpp.
#include <algorithm>
#include <cstring>

#include "oprf.h"
#include "radix.h"
#include "capi_internal.h"

namespace fhe {

void oprf_rows_host(const uint8_t seed[32], uint32_t n, size_t row0, size_t count, size_t stride, uint64_t* out) {
    const KeyWords key = bytes_key(seed);
    const uint64_t R = oprf_row_blocks(n);
    ChaChaStream masks(key, kStreamOprf);
    for (size_t b = 0; b < count; ++b) {
        uint64_t* row = out + b * stride;
        masks.seek((uint64_t)(row0 + b) * R * 16);  // 32-bit stream words: the row's first block
        masks.fill_u64(row, n);
        row[n] = 0;
        for (size_t j = (size_t)n + 1; j < stride; ++j) row[j] = kMsPadWord;
    }
}

void oprf_lut_poly(const Params& p, uint32_t bits, uint64_t* out) {
    const uint64_t half = p.delta() / 2;
    for (uint32_t i = 0; i < kPolySize; ++i) out[i] = (2 * (((uint64_t)i << bits) / (2 * kPolySize)) + 1) * half;
}

}  // namespace fhe

using namespace fhe;

// One polynomial per `bits`, keyed apart from the integer tables (msg_carry entries, each below msg_carry) and
// from the half-step tables (msg_carry + 1 entries): three entries, the first no table value.
int fhe_ctx::register_lut_oprf(uint32_t bits, uint32_t* id) {
    std::vector<uint32_t> key{0xFFFFFFFEu, 0x4F505246u /* "OPRF" */, bits};
    auto it = lut_ids.find(key);
    if (it != lut_ids.end()) {
        *id = it->second;
        return FHE_OK;
    }
    std::vector<uint64_t> poly(kPolySize);
    oprf_lut_poly(p, bits, poly.data());
    const uint32_t nid = (uint32_t)lut_ids.size();
    h_luts.insert(h_luts.end(), poly.begin(), poly.end());
    lut_ids.emplace(std::move(key), nid);
    luts_dirty = true;
    *id = nid;
    return FHE_OK;
}

namespace {
int check_rows(const char* who, uint32_t n, size_t count, size_t stride) {
    if (n < 1 || n > kBigDim) return invalid(std::string(who) + ": n must be 1 .. 2048");
    if (stride < (size_t)n + 1) return invalid(std::string(who) + ": stride must be at least n + 1");
    if (count > kOprfMaxRows) return invalid(std::string(who) + ": more than 2^23 rows");
    return FHE_OK;
}
}  // namespace

extern "C" {

int fhe_oprf_rows_host(const uint8_t seed[32], uint32_t n, size_t count, size_t stride, uint64_t* out) {
    if (!seed || (!out && count)) return invalid("null argument to fhe_oprf_rows_host");
    if (const int rc = check_rows("fhe_oprf_rows_host", n, count, stride)) return rc;
    oprf_rows_host(seed, n, 0, count, stride, out);
    return FHE_OK;
}

int fhe_oprf_lut_host(const fhe_params* params, uint32_t bits, uint64_t* out) {
    if (!params || !out) return invalid("null argument to fhe_oprf_lut_host");
    Params p;
    const char* why = nullptr;
    if (!Params::from_c(*params, &p, &why)) {
        set_error(why);
        return FHE_ERR_UNSUPPORTED;
    }
    if (bits < 1 || bits > oprf_max_bits(p))
        return invalid("fhe_oprf_lut_host: bits must be 1 .. log2(message_modulus) = " + std::to_string(oprf_max_bits(p)));
    oprf_lut_poly(p, bits, out);
    return FHE_OK;
}

int fhe_oprf_rows(fhe_ctx* c, const uint8_t seed[32], uint32_t n, size_t count, size_t stride, uint64_t* out) {
    if (!c || !seed || (!out && count)) return invalid("null argument to fhe_oprf_rows");
    if (const int rc = check_rows("fhe_oprf_rows", n, count, stride)) return rc;
    if (count == 0) return FHE_OK;
    FHE_HIP_CHECK(hipSetDevice(c->device));
    // the kernel writes the workspace's layout; the caller's stride gets each row's first min(stride, ws) words,
    // and whatever lies above them the marker
    const size_t ws = ms_stride_words(n);
    DeviceBuf<uint64_t> dev;
    FHE_HIP_CHECK(dev.grow(count * ws));
    const KeyWords key = bytes_key(seed);
    FHE_HIP_CHECK(launch_oprf_rows(chacha_stream_key(key.data(), kStreamOprf), dev, 0, (uint32_t)count, n, c->stream));
    if (stride > ws)
        for (size_t b = 0; b < count; ++b) std::fill(out + b * stride + ws, out + (b + 1) * stride, kMsPadWord);
    FHE_HIP_CHECK(hipMemcpy2DAsync(out, stride * 8, dev, ws * 8, std::min(stride, ws) * 8, count, hipMemcpyDeviceToHost,
                                   c->stream));
    FHE_HIP_CHECK(hipStreamSynchronize(c->stream));
    return FHE_OK;
}

int fhe_ctx_time_oprf_rows(fhe_ctx* c, size_t count, uint32_t n, uint32_t reps, float* ms) {
    if (!c || !ms || !reps || !count) return invalid("invalid argument to fhe_ctx_time_oprf_rows");
    if (const int rc = check_rows("fhe_ctx_time_oprf_rows", n, count, (size_t)n + 1)) return rc;
    FHE_HIP_CHECK(hipSetDevice(c->device));
    DeviceBuf<uint64_t> dev;
    FHE_HIP_CHECK(dev.grow(count * ms_stride_words(n)));
    ChaChaKey k{};
    for (int i = 0; i < 8; ++i) k.key[i] = 0x9E3779B9u * (uint32_t)(i + 1);
    k.nonce[0] = kStreamOprf;
    hipEvent_t ev[2] = {nullptr, nullptr};
    auto body = [&]() -> int {
        FHE_HIP_CHECK(hipEventCreate(&ev[0]));
        FHE_HIP_CHECK(hipEventCreate(&ev[1]));
        FHE_HIP_CHECK(launch_oprf_rows(k, dev, 0, (uint32_t)count, n, c->stream));  // first touch outside the interval
        FHE_HIP_CHECK(hipEventRecord(ev[0], c->stream));
        for (uint32_t r = 0; r < reps; ++r) FHE_HIP_CHECK(launch_oprf_rows(k, dev, 0, (uint32_t)count, n, c->stream));
        FHE_HIP_CHECK(hipEventRecord(ev[1], c->stream));
        FHE_HIP_CHECK(hipEventSynchronize(ev[1]));
        float total = 0.f;
        FHE_HIP_CHECK(hipEventElapsedTime(&total, ev[0], ev[1]));
        *ms = total / (float)reps;
        return FHE_OK;
    };
    const int r = body();
    for (hipEvent_t e : ev)
        if (e) (void)hipEventDestroy(e);
    return r;
}

int fhe_oprf_blocks(fhe_ctx* c, const uint8_t seed[32], size_t count, uint32_t bits, uint64_t* out) {
    if (const int sim = refuse_simulated(c, "fhe_oprf_blocks")) return sim;
    if (!c) return invalid("null context");
    if (!c->has_key || !c->engine) {
        set_error("no server key installed (fhe_set_server_key)");
        return FHE_ERR_NO_KEY;
    }
    if (!seed || (!out && count)) return invalid("null argument to fhe_oprf_blocks");
    FHE_HIP_CHECK(hipSetDevice(c->device));
    try {
        const Blocks blocks = c->engine->oprf(seed, count, bits);
        std::vector<const Block*> ptrs;
        for (const Block& b : blocks) ptrs.push_back(&b);
        if (count) c->engine->download_many(ptrs, out, true);
        return FHE_OK;
    } catch (const EngineError& e) {
        set_error(e.what());
        return e.code;
    } catch (const std::exception& e) {
        set_error(e.what());
        return FHE_ERR_INVALID;
    }
}

}  // extern "C"
