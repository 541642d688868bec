// ct_digest.cpp -- host side of the ciphertext digests (ct_digest.h): the definition of
// ct_digest.hip's kernel, the value digest, the re-randomization context and their C entry points (no context,
// no GPU), and the kernel's measurement hook.  Engine::digest (engine_ops.cpp) is the device path.
#include <cstring>
#include <memory>
#include <string>

#include "context.h"
#include "ct_digest.h"
#include "fhe_rocm.h"
#include "public_key.h"  // parallel_chunks
#include "capi_internal.h"

namespace fhe {

namespace {
constexpr size_t kRowWords = kBigCt;  // 2049
constexpr size_t kLeafBytes = 256, kLeaves = 64, kGroup = 8;
static_assert(kLeaves * kLeafBytes == kPolySize * 8, "64 leaves of 256 bytes cover the mask");

// the row's words as the bytes that are hashed (little-endian, whatever the host)
void le_bytes(const uint64_t* w, size_t n, uint8_t* out) {
    for (size_t i = 0; i < n; ++i)
        for (int b = 0; b < 8; ++b) out[8 * i + b] = (uint8_t)(w[i] >> (8 * b));
}
}  // namespace

void ct_row_digest_host(const uint64_t* row, uint8_t out[32]) {
    static const Sha256 leaf0 = tagged_start(kTagCtLeaf), node0 = tagged_start(kTagCtNode), row0 = tagged_start(kTagCtRow);
    uint8_t leaves[kLeaves][32];
    uint8_t bytes[kLeafBytes];
    for (size_t j = 0; j < kLeaves; ++j) {
        le_bytes(row + j * (kLeafBytes / 8), kLeafBytes / 8, bytes);
        Sha256 s = leaf0;
        s.update(bytes, kLeafBytes);
        std::memcpy(leaves[j], s.final().data(), 32);
    }
    Sha256 r = row0;
    for (size_t g = 0; g < kLeaves / kGroup; ++g) {
        Sha256 s = node0;
        s.update(leaves[kGroup * g], kGroup * 32);
        r.update(s.final().data(), 32);
    }
    r.u64le(row[kPolySize]);
    std::memcpy(out, r.final().data(), 32);
}

void ct_digest_host(const uint64_t* rows, size_t n, uint8_t* out) {
    parallel_chunks(n, [&](size_t i) { ct_row_digest_host(rows + i * kRowWords, out + 32 * i); });
}

void ct_value_digest_host(uint8_t kind, uint32_t bits, const uint8_t* tags, const uint32_t* degrees, const uint32_t* noises,
                          const uint8_t* rowdigests, size_t nblocks, uint8_t out[32]) {
    Sha256 s = tagged_start(kTagCtValue);
    s.u8(kind);
    s.u32le(bits);
    s.u32le((uint32_t)nblocks);
    for (size_t i = 0; i < nblocks; ++i) {
        s.u8(tags[i]);
        s.u32le(degrees[i]);
        s.u32le(noises[i]);
        s.update(rowdigests + 32 * i, 32);
    }
    std::memcpy(out, s.final().data(), 32);
}

const CtDigestMidstates& ct_digest_midstates() {
    static const CtDigestMidstates m = [] {
        CtDigestMidstates x;
        std::memcpy(x.leaf, tagged_start(kTagCtLeaf).h, 32);
        std::memcpy(x.node, tagged_start(kTagCtNode).h, 32);
        std::memcpy(x.row, tagged_start(kTagCtRow).h, 32);
        return x;
    }();
    return m;
}

}  // namespace fhe

using namespace fhe;

namespace {
int add_item(fhe_rerand_context* rc, uint8_t kind, const uint8_t* p, size_t n, const char* who) {
    if (rc->finalized) return invalid(std::string(who) + ": the context gave out a seed already; a seed depends on everything added");
    rc->h.u8(kind);
    rc->h.u64le((uint64_t)n);
    if (n) rc->h.update(p, n);
    return FHE_OK;
}
}  // namespace

extern "C" {

int fhe_ct_digest_host(const uint64_t* rows, size_t nblocks, uint8_t* out) {
    if ((!rows || !out) && nblocks) return invalid("null argument to fhe_ct_digest_host");
    if (nblocks > kCtDigestMaxRows) return invalid("fhe_ct_digest_host: more than 2^24 rows");
    return guarded_alloc([&] {
        ct_digest_host(rows, nblocks, out);
        return (int)FHE_OK;
    });
}

int fhe_ct_value_digest_host(uint8_t kind, uint32_t bits, const uint8_t* tags, const uint32_t* degrees, const uint32_t* noises,
                             const uint8_t* rowdigests, size_t nblocks, uint8_t out[32]) {
    if (!out || ((!tags || !degrees || !noises || !rowdigests) && nblocks)) return invalid("null argument to fhe_ct_value_digest_host");
    if (nblocks > kCtDigestMaxRows) return invalid("fhe_ct_value_digest_host: more than 2^24 blocks");
    if (kind > FHE_CT_KIND_BIGUINT) return invalid("fhe_ct_value_digest_host: kind is 0 (radix) or 1 (BigUintFHE)");
    for (size_t i = 0; i < nblocks; ++i)
        if (tags[i] > 1) return invalid("fhe_ct_value_digest_host: a block's tag is 0 (trivial) or 1 (ciphertext)");
    ct_value_digest_host(kind, bits, tags, degrees, noises, rowdigests, nblocks, out);
    return FHE_OK;
}

int fhe_rerand_context_new(const uint8_t* domain, size_t domain_len, fhe_rerand_context** rc) {
    if (!rc || (domain_len && !domain)) return invalid("null argument to fhe_rerand_context_new");
    return guarded_alloc([&] {
        auto x = std::make_unique<fhe_rerand_context>();
        x->h = tagged_start(kTagRerandContext);
        x->h.u64le((uint64_t)domain_len);
        if (domain_len) x->h.update(domain, domain_len);
        *rc = x.release();
        return (int)FHE_OK;
    });
}

int fhe_rerand_context_add_bytes(fhe_rerand_context* rc, const uint8_t* data, size_t len) {
    if (!rc || (len && !data)) return invalid("null argument to fhe_rerand_context_add_bytes");
    return add_item(rc, FHE_RERAND_ITEM_BYTES, data, len, "fhe_rerand_context_add_bytes");
}

int fhe_rerand_context_add_digest(fhe_rerand_context* rc, const uint8_t digest[32]) {
    if (!rc || !digest) return invalid("null argument to fhe_rerand_context_add_digest");
    return add_item(rc, FHE_RERAND_ITEM_DIGEST, digest, 32, "fhe_rerand_context_add_digest");
}

int fhe_rerand_context_seed(fhe_rerand_context* rc, uint64_t index, uint8_t out[32]) {
    if (!rc || !out) return invalid("null argument to fhe_rerand_context_seed");
    if (!rc->finalized) {
        std::memcpy(rc->root, rc->h.final().data(), 32);
        rc->finalized = true;
    }
    Sha256 s = tagged_start(kTagRerandSeed);
    s.update(rc->root, 32);
    s.u64le(index);
    std::memcpy(out, s.final().data(), 32);
    return FHE_OK;
}

void fhe_rerand_context_destroy(fhe_rerand_context* rc) { delete rc; }

int fhe_ctx_time_ct_digest(fhe_ctx* c, size_t nblocks, uint32_t reps, float* ms) {
    if (!c || !ms || !reps || !nblocks) return invalid("invalid argument to fhe_ctx_time_ct_digest");
    if (nblocks > kCtDigestMaxRows) return invalid("fhe_ctx_time_ct_digest: more than 2^24 blocks");
    if (!c->stream) return invalid("fhe_ctx_time_ct_digest: the context has no stream");
    FHE_HIP_CHECK(hipSetDevice(c->device));
    // rows at a slot's stride (2049 words: 8-byte aligned, as the pool's), their entries, the digests
    DeviceBuf<uint64_t> d_rows;
    DeviceBuf<CtDigestEntry> d_entries;
    DeviceBuf<uint8_t> d_out;
    hipEvent_t ev[2] = {nullptr, nullptr};
    auto body = [&]() -> int {
        FHE_HIP_CHECK(d_rows.grow(nblocks * kBigCt));
        FHE_HIP_CHECK(d_entries.grow(nblocks));
        FHE_HIP_CHECK(d_out.grow(nblocks * 32));
        std::vector<CtDigestEntry> entries(nblocks);
        for (size_t i = 0; i < nblocks; ++i) entries[i] = {(const uint64_t*)d_rows + i * kBigCt, 0};
        FHE_HIP_CHECK(hipMemsetAsync(d_rows, 0x5A, nblocks * kBigCt * 8, c->stream));
        FHE_HIP_CHECK(hipMemcpyAsync(d_entries, entries.data(), nblocks * sizeof(CtDigestEntry), hipMemcpyHostToDevice, c->stream));
        FHE_HIP_CHECK(hipStreamSynchronize(c->stream));
        FHE_HIP_CHECK(hipEventCreate(&ev[0]));
        FHE_HIP_CHECK(hipEventCreate(&ev[1]));
        FHE_HIP_CHECK(hipEventRecord(ev[0], c->stream));
        for (uint32_t r = 0; r < reps; ++r)
            FHE_HIP_CHECK(launch_ct_digest(d_entries, d_out, (uint32_t)nblocks, ct_digest_midstates(), c->stream));
        FHE_HIP_CHECK(hipEventRecord(ev[1], c->stream));
        FHE_HIP_CHECK(hipEventSynchronize(ev[1]));
        float total = 0.f;
        FHE_HIP_CHECK(hipEventElapsedTime(&total, ev[0], ev[1]));
        *ms = total / (float)reps;
        return FHE_OK;
    };
    const int r = guarded_alloc(body);
    if (c->stream) (void)hipStreamSynchronize(c->stream);  // the buffers go: nothing may still read them
    for (hipEvent_t e : ev)
        if (e) (void)hipEventDestroy(e);
    return r;
}

}  // extern "C"
