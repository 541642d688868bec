// ms_center.cpp -- host side of the centered modulus switch: the exact-integer definition of
// ms_center.hip's kernel, its C entry point (no context, no GPU), the per-context mode, and the test and
// measurement entries that run the kernel over host rows.  fhe_ctx::keyswitch (context.cpp) is the device path.
#include "context.h"
#include "fhe_rocm.h"
#include "capi_internal.h"

namespace fhe {

// signed distance of x from the multiple of 2^52 that modswitch_2n / fho_modswitch rounds it to: [-2^51, 2^51)
static inline int64_t ms_res(uint64_t x) {
    return (int64_t)((x + (1ull << 51)) & ((1ull << 52) - 1)) - (int64_t)(1ull << 51);
}

void ms_center_host(uint64_t* rows, size_t count, uint32_t n, size_t stride) {
    for (size_t r = 0; r < count; ++r) {
        uint64_t* a = rows + r * stride;
        int64_t S = 0;  // |S| <= n 2^51 <= 2^62
        for (uint32_t i = 0; i < n; ++i) S += ms_res(a[i]);
        a[n] -= (uint64_t)(S >> 1);  // arithmetic shift: floor
    }
}

}  // namespace fhe

using namespace fhe;

namespace {
// 1 <= n <= 2048 keeps the sum inside int64; a row holds its n mask words and the body
int check_shape(const char* who, uint32_t n, size_t stride) {
    if (n < 1 || n > FHE_MS_CENTER_MAX_N) return invalid(std::string(who) + ": n must be 1 .. 2048");
    if (stride < (size_t)n + 1) return invalid(std::string(who) + ": stride must be at least n + 1");
    return FHE_OK;
}
}  // namespace

extern "C" {

int fhe_ms_center_host(uint64_t* rows, size_t count, uint32_t n, size_t stride) {
    if (!rows && count) return invalid("null argument to fhe_ms_center_host");
    if (const int rc = check_shape("fhe_ms_center_host", n, stride)) return rc;
    ms_center_host(rows, count, n, stride);
    return FHE_OK;
}

int fhe_ctx_set_modulus_switch(fhe_ctx* c, int mode) {
    if (!c) return invalid("null context");
    if (mode != FHE_MS_STANDARD && mode != FHE_MS_CENTERED)
        return invalid("unknown modulus switch mode " + std::to_string(mode) + " (FHE_MS_STANDARD 0, FHE_MS_CENTERED 1)");
    c->ms_mode = mode;
    return FHE_OK;
}

int fhe_ctx_get_modulus_switch(fhe_ctx* c, int* mode) {
    if (!c || !mode) return invalid("null argument to fhe_ctx_get_modulus_switch");
    *mode = c->ms_mode;
    return FHE_OK;
}

int fhe_ms_center_rows(fhe_ctx* c, uint64_t* rows, size_t count, uint32_t n, size_t stride) {
    if (!c || (!rows && count)) return invalid("null argument to fhe_ms_center_rows");
    if (const int rc = check_shape("fhe_ms_center_rows", n, stride)) return rc;
    if (count > (size_t)0x7fffffff) return invalid("fhe_ms_center_rows: batch too large");
    if (count == 0) return FHE_OK;
    FHE_HIP_CHECK(hipSetDevice(c->device));
    const size_t bytes = count * stride * 8;
    DeviceBuf<uint64_t> dev;
    FHE_HIP_CHECK(dev.grow(count * stride));
    FHE_HIP_CHECK(hipMemcpyAsync(dev, rows, bytes, hipMemcpyHostToDevice, c->stream));
    FHE_HIP_CHECK(launch_ms_center(dev, count, n, stride, c->stream));
    FHE_HIP_CHECK(hipMemcpyAsync(rows, dev, bytes, hipMemcpyDeviceToHost, c->stream));
    FHE_HIP_CHECK(hipStreamSynchronize(c->stream));
    return FHE_OK;
}

int fhe_ctx_time_ms_center(fhe_ctx* c, size_t count, uint32_t n, size_t stride, uint32_t reps, float* ms) {
    if (!c || !ms || !reps || !count) return invalid("invalid argument to fhe_ctx_time_ms_center");
    if (const int rc = check_shape("fhe_ctx_time_ms_center", n, stride)) return rc;
    if (count > (size_t)0x7fffffff) return invalid("fhe_ctx_time_ms_center: batch too large");
    FHE_HIP_CHECK(hipSetDevice(c->device));
    DeviceBuf<uint64_t> dev;
    FHE_HIP_CHECK(dev.grow(count * stride));
    hipEvent_t ev[2] = {nullptr, nullptr};
    auto body = [&]() -> int {
        FHE_HIP_CHECK(hipMemsetAsync(dev, 0x5A, count * stride * 8, c->stream));
        FHE_HIP_CHECK(hipEventCreate(&ev[0]));
        FHE_HIP_CHECK(hipEventCreate(&ev[1]));
        FHE_HIP_CHECK(hipEventRecord(ev[0], c->stream));
        for (uint32_t r = 0; r < reps; ++r) FHE_HIP_CHECK(launch_ms_center(dev, count, n, stride, c->stream));
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
