// ms_center_host_check.c -- stand-alone driver of the host definition of the centered modulus switch
// (fhe_ms_center_host; no GPU call), for a host AddressSanitizer + UndefinedBehaviorSanitizer run with its own main:
//   make -C fhe-sign_amd asan
//   clang -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -shared-libsan -Iinclude \
//         tools/ms_center_host_check.c -Lfhe-sign_amd/lib_asan -lfhe_rocm -Wl,-rpath,$PWD/fhe-sign_amd/lib_asan \
//         -Wl,-rpath,$(dirname $(clang -print-file-name=libclang_rt.asan-x86_64.so)) -o ms_center_host_check
// (clang = the ROCm toolchain's, as for tools/rerandomize_host_check.c).  At n = 1, 2, 63, 64, 65, 834 and 2048,
// 1 to 5 rows, strides n + 1 and n + 1 rounded up to 8, in buffers of exactly count * stride words (a word past
// the end is the sanitizer's), it compares every word with a restatement in 128-bit integers; then the extremes
// of the sum at n = 2048 (S = -2^62 and 2048 (2^51 - 1): a signed overflow would be the sanitizer's), rows on the
// 2^52 grid, an odd negative S, and every refusal.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "fhe_rocm.h"

#define CHECK(x) do { if (!(x)) { printf("FAIL line %d: %s (%s)\n", __LINE__, #x, fhe_last_error()); return 1; } } while (0)

static uint64_t state = 0x9E3779B97F4A7C15ull;
static uint64_t next(void) {  // splitmix64
    uint64_t z = (state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// body' = body - floor(S / 2) in 128-bit integers
static uint64_t expect_body(const uint64_t* a, uint32_t n) {
    __int128 S = 0;
    for (uint32_t i = 0; i < n; ++i) S += (__int128)((a[i] + (1ull << 51)) & ((1ull << 52) - 1)) - ((__int128)1 << 51);
    __int128 h = S >= 0 ? S / 2 : -((-S + 1) / 2);
    return (uint64_t)((__int128)a[n] - h);
}

static int run(uint32_t n, size_t count, size_t stride) {
    const size_t words = count * stride;
    uint64_t* rows = malloc(words * 8);
    uint64_t* in = malloc(words * 8);
    for (size_t i = 0; i < words; ++i) in[i] = rows[i] = next();
    CHECK(fhe_ms_center_host(rows, count, n, stride) == FHE_OK);
    for (size_t r = 0; r < count; ++r)
        for (size_t j = 0; j < stride; ++j)
            CHECK(rows[r * stride + j] == (j == n ? expect_body(in + r * stride, n) : in[r * stride + j]));
    free(rows);
    free(in);
    return 0;
}

int main(void) {
    const uint32_t dims[] = {1, 2, 63, 64, 65, 834, 2048};
    for (size_t d = 0; d < sizeof dims / sizeof *dims; ++d)
        for (size_t count = 1; count <= 5; ++count) {
            if (run(dims[d], count, dims[d] + 1)) return 1;
            if (run(dims[d], count, (dims[d] + 1 + 7) / 8 * 8)) return 1;
        }
    const uint32_t n = 2048;
    uint64_t* row = malloc((n + 1) * 8);
    for (uint32_t i = 0; i < n; ++i) row[i] = 1ull << 51;  // every residue -2^51: S = -2^62
    row[n] = 7;
    CHECK(fhe_ms_center_host(row, 1, n, n + 1) == FHE_OK && row[n] == 7 + (1ull << 61));
    for (uint32_t i = 0; i < n; ++i) row[i] = (1ull << 51) - 1;  // every residue 2^51 - 1
    row[n] = 7;
    CHECK(fhe_ms_center_host(row, 1, n, n + 1) == FHE_OK && row[n] == 7 - 1024 * ((1ull << 51) - 1));
    for (uint32_t i = 0; i < n; ++i) row[i] = (uint64_t)(i % 4096) << 52;  // on the grid: unchanged
    row[n] = 7;
    CHECK(fhe_ms_center_host(row, 1, n, n + 1) == FHE_OK && row[n] == 7);
    row[3] -= 1, row[4] -= 1, row[5] -= 1;  // S = -3: floor(-3 / 2) = -2
    CHECK(fhe_ms_center_host(row, 1, n, n + 1) == FHE_OK && row[n] == 9);
    CHECK(fhe_ms_center_host(row, 1, 0, 8) == FHE_ERR_INVALID);
    CHECK(fhe_ms_center_host(row, 1, 2049, 2056) == FHE_ERR_INVALID);
    CHECK(fhe_ms_center_host(row, 1, n, n) == FHE_ERR_INVALID);
    CHECK(fhe_ms_center_host(NULL, 1, n, n + 1) == FHE_ERR_INVALID);
    CHECK(fhe_ms_center_host(NULL, 0, n, n + 1) == FHE_OK);
    CHECK(row[n] == 9);
    free(row);
    printf("centered modulus switch host code: all checks passed\n");
    return 0;
}
