// rerandomize.cpp -- host side of the re-randomization under the compact public key (public_key.h, DESIGN.md
// 6f): the exact-integer definition of rerandomize.hip's two kernels, its C entry points (no context, no GPU),
// and the install of the public key on a context.  Engine::rerandomize (engine_ops.cpp) is the device path.
#include <cstring>
#include <memory>

#include "context.h"
#include "fhe_rocm.h"
#include "keygen.h"
#include "public_key.h"
#include "capi_internal.h"

namespace fhe {

namespace {
constexpr uint32_t N = kPolySize;
}  // namespace

void rerandomize_zero_host(const fhe_public_key& pk, const uint8_t seed[32], size_t n, uint64_t* za, uint64_t* zb) {
    if (!n) return;
    const size_t chunks = (n + N - 1) / N;
    std::vector<uint64_t> A(N);
    public_key_mask(pk.seed, A.data());
    const KeyWords key = bytes_key(seed);
    const uint32_t nb = pk.params.glwe_noise_log2;
    parallel_chunks(chunks, [&](size_t c) {
        const size_t used = std::min<size_t>(N, n - c * N);
        uint64_t R[N / 64];
        ChaChaStream rs(key, kStreamRerandBinary);
        rs.seek((uint64_t)c * (N / 64) * 2);
        rs.fill_u64(R, N / 64);
        std::vector<uint64_t> noise(N + used), BR(N, 0);
        ChaChaStream ns(key, kStreamRerandNoise);
        ns.seek((uint64_t)c * 2 * N * 2);
        ns.fill_u64(noise.data(), noise.size());
        auto bit = [&](uint32_t j) { return (R[j >> 6] >> (j & 63)) & 1; };
        uint64_t* ZA = za + c * N;
        for (uint32_t j = 0; j < N; ++j) ZA[j] = (uint64_t)tuniform_of(noise[j], nb);
        negacyclic_binary_mac(ZA, A.data(), bit);
        negacyclic_binary_mac(BR.data(), pk.body.data(), bit);
        uint64_t* ZB = zb + c * N;
        for (size_t j = 0; j < used; ++j) ZB[j] = BR[j] + (uint64_t)tuniform_of(noise[N + j], nb);
    });
}

void rerandomize_host(const fhe_public_key& pk, const uint8_t seed[32], uint64_t* cts, size_t n) {
    if (!n) return;
    std::vector<uint64_t> za((n + N - 1) / N * N), zb(n);
    rerandomize_zero_host(pk, seed, n, za.data(), zb.data());
    for (size_t i = 0; i < n; ++i) {
        const size_t t = i % N;
        const uint64_t* ZA = za.data() + i / N * N;
        uint64_t* row = cts + i * kBigCt;
        for (size_t u = 0; u <= t; ++u) row[u] += ZA[t - u];
        for (size_t u = t + 1; u < N; ++u) row[u] -= ZA[t - u + N];
        row[N] += zb[i];
    }
}

}  // namespace fhe

using namespace fhe;

int fhe_ctx::ensure_rr(size_t chunks) {
    if (d_rr_z.fits(chunks * 2 * kPolySize)) return FHE_OK;
    FHE_HIP_CHECK(hipStreamSynchronize(stream));  // an earlier call's kernels may still read it
    FHE_HIP_CHECK(d_rr_z.grow(chunks * 2 * kPolySize));
    return FHE_OK;
}

int fhe_ctx::release_public_key() {
    if (stream) FHE_HIP_CHECK(hipStreamSynchronize(stream));
    (void)d_pk_ab.reset();
    (void)d_rr_z.reset();
    has_pk = false;
    return FHE_OK;
}

extern "C" {

int fhe_rerandomize_host(const fhe_public_key* pk, const uint8_t* seed, uint64_t* cts, size_t nblocks) {
    if (!pk || !seed || (!cts && nblocks)) return invalid("null argument to fhe_rerandomize_host");
    if (nblocks > kCompactMaxCoefs) return invalid("fhe_rerandomize_host: more than 2^24 blocks");
    return guarded_alloc([&] {
        rerandomize_host(*pk, seed, cts, nblocks);
        return (int)FHE_OK;
    });
}

int fhe_rerandomize_zero_host(const fhe_public_key* pk, const uint8_t* seed, size_t nblocks, uint64_t* za, size_t za_words,
                              uint64_t* zb, size_t zb_words) {
    if (!pk || !seed || ((!za || !zb) && nblocks)) return invalid("null argument to fhe_rerandomize_zero_host");
    if (nblocks > kCompactMaxCoefs) return invalid("fhe_rerandomize_zero_host: more than 2^24 blocks");
    if (za_words < (nblocks + kPolySize - 1) / kPolySize * kPolySize || zb_words < nblocks)
        return invalid("fhe_rerandomize_zero_host: buffer too small (2048 words per chunk, one per block)");
    return guarded_alloc([&] {
        rerandomize_zero_host(*pk, seed, nblocks, za, zb);
        return (int)FHE_OK;
    });
}

int fhe_set_public_key(fhe_ctx* c, const fhe_public_key* pk) {
    if (const int rc = dependent_key_preamble(c, pk != nullptr, "fhe_set_public_key", pk ? &pk->params : nullptr, "public key"))
        return rc;
    if (pk->body.size() != kPolySize) return invalid("public key: the body is not 2048 words");
    FHE_HIP_CHECK(hipSetDevice(c->device));
    int rc = c->release_public_key();
    if (rc) return rc;
    return guarded_alloc([&] {
        std::vector<uint64_t> ab(2 * kPolySize);
        public_key_mask(pk->seed, ab.data());
        std::memcpy(ab.data() + kPolySize, pk->body.data(), kPolySize * 8);
        auto body = [&]() -> int {
            FHE_HIP_CHECK(c->d_pk_ab.grow(ab.size()));
            FHE_HIP_CHECK(hipMemcpyAsync(c->d_pk_ab, ab.data(), ab.size() * 8, hipMemcpyHostToDevice, c->stream));
            FHE_HIP_CHECK(hipStreamSynchronize(c->stream));
            return FHE_OK;
        };
        const int r = body();
        if (r) {
            (void)c->release_public_key();
            return r;
        }
        c->has_pk = true;
        return (int)FHE_OK;
    });
}

int fhe_ctx_time_rerand_zero(fhe_ctx* c, const uint8_t* seed, size_t nblocks, uint32_t reps, float* ms) {
    if (!c || !seed || !ms || !reps || !nblocks) return invalid("invalid argument to fhe_ctx_time_rerand_zero");
    if (nblocks > kCompactMaxCoefs) return invalid("fhe_ctx_time_rerand_zero: more than 2^24 blocks");
    if (!c->has_pk) {
        set_error("no public key installed (fhe_set_public_key)");
        return FHE_ERR_NO_KEY;
    }
    FHE_HIP_CHECK(hipSetDevice(c->device));
    const int rc = c->ensure_rr((nblocks + kPolySize - 1) / kPolySize);
    if (rc) return rc;
    const KeyWords key = bytes_key(seed);
    const ChaChaKey kb = chacha_stream_key(key.data(), kStreamRerandBinary), kn = chacha_stream_key(key.data(), kStreamRerandNoise);
    hipEvent_t ev[2] = {nullptr, nullptr};
    auto body = [&]() -> int {
        FHE_HIP_CHECK(hipEventCreate(&ev[0]));
        FHE_HIP_CHECK(hipEventCreate(&ev[1]));
        FHE_HIP_CHECK(hipEventRecord(ev[0], c->stream));
        for (uint32_t r = 0; r < reps; ++r)
            FHE_HIP_CHECK(launch_rerand_zero(kb, kn, c->d_pk_ab, c->d_rr_z, (uint32_t)nblocks, c->p.glwe_noise_log2, c->stream));
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

}  // extern "C"
