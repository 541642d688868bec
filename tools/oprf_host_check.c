// oprf_host_check.c -- stand-alone driver of the host definitions of the oblivious pseudo-random values
// (fhe_oprf_rows_host, fhe_oprf_lut_host; no GPU call), for a host AddressSanitizer + UndefinedBehaviorSanitizer
// run with its own main:
//   make -C fhe-sign_amd asan
//   clang -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -shared-libsan -Iinclude \
//         tools/oprf_host_check.c -Lfhe-sign_amd/lib_asan -lfhe_rocm -Wl,-rpath,$PWD/fhe-sign_amd/lib_asan \
//         -Wl,-rpath,$(dirname $(clang -print-file-name=libclang_rt.asan-x86_64.so)) -o oprf_host_check
// (clang = the ROCm toolchain's, as for tools/ms_center_host_check.c).  At n = 1, 2, 15, 16, 255, 256, 833, 834 and
// 2048, 1 to 5 and 65 rows, strides n + 1 and n + 1 rounded up to 8, in buffers of exactly count * stride words (a
// word past the end is the sanitizer's), it compares every word with this file's own RFC 8439 block function;
// then both accumulators against the closed form, and every refusal.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "fhe_rocm.h"

#define CHECK(x) do { if (!(x)) { printf("FAIL line %d: %s (%s)\n", __LINE__, #x, fhe_last_error()); return 1; } } while (0)
#define PAD 0xA5A55A5AC3C33C3Cull

static uint32_t rotl(uint32_t v, int c) { return (v << c) | (v >> (32 - c)); }
#define QR(a, b, c, d) \
    x[a] += x[b], x[d] = rotl(x[d] ^ x[a], 16), x[c] += x[d], x[b] = rotl(x[b] ^ x[c], 12), \
    x[a] += x[b], x[d] = rotl(x[d] ^ x[a], 8), x[c] += x[d], x[b] = rotl(x[b] ^ x[c], 7)

// the 8 u64 words of block `counter` of the stream (key = the seed's little-endian words, nonce {111, "ROCM", 0})
static void block(const uint8_t seed[32], uint32_t counter, uint64_t out[8]) {
    uint32_t s[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u}, x[16];
    for (int i = 0; i < 8; ++i)
        s[4 + i] = (uint32_t)seed[4 * i] | (uint32_t)seed[4 * i + 1] << 8 | (uint32_t)seed[4 * i + 2] << 16 | (uint32_t)seed[4 * i + 3] << 24;
    s[12] = counter, s[13] = 111, s[14] = 0x524f434du, s[15] = 0;
    memcpy(x, s, sizeof x);
    for (int r = 0; r < 10; ++r) {
        QR(0, 4, 8, 12); QR(1, 5, 9, 13); QR(2, 6, 10, 14); QR(3, 7, 11, 15);
        QR(0, 5, 10, 15); QR(1, 6, 11, 12); QR(2, 7, 8, 13); QR(3, 4, 9, 14);
    }
    for (int w = 0; w < 8; ++w) out[w] = (uint64_t)(x[2 * w] + s[2 * w]) | (uint64_t)(x[2 * w + 1] + s[2 * w + 1]) << 32;
}

static int run(const uint8_t seed[32], uint32_t n, size_t count, size_t stride) {
    uint64_t* rows = malloc(count * stride * 8);
    memset(rows, 0x11, count * stride * 8);
    CHECK(fhe_oprf_rows_host(seed, n, count, stride, rows) == FHE_OK);
    const uint32_t R = (n + 7) / 8;
    for (size_t b = 0; b < count; ++b)
        for (size_t j = 0; j < stride; ++j) {
            uint64_t want = PAD, blk[8];
            if (j < n) {
                block(seed, (uint32_t)(b * R + j / 8), blk);
                want = blk[j % 8];
            } else if (j == n) {
                want = 0;
            }
            CHECK(rows[b * stride + j] == want);
        }
    free(rows);
    return 0;
}

int main(void) {
    uint8_t seed[32];
    for (int i = 0; i < 32; ++i) seed[i] = (uint8_t)(7 * i + 3);
    const uint32_t dims[] = {1, 2, 15, 16, 255, 256, 833, 834, 2048};
    const size_t counts[] = {1, 2, 3, 4, 5, 65};
    for (size_t d = 0; d < sizeof dims / sizeof *dims; ++d)
        for (size_t c = 0; c < sizeof counts / sizeof *counts; ++c) {
            if (run(seed, dims[d], counts[c], dims[d] + 1)) return 1;
            if (run(seed, dims[d], counts[c], (dims[d] + 1 + 7) / 8 * 8)) return 1;
        }
    fhe_params p;
    CHECK(fhe_params_default(&p) == FHE_OK);
    const uint64_t half = (1ull << 63) / (p.message_modulus * p.carry_modulus) / 2;
    uint64_t* lut = malloc(2048 * 8);
    for (uint32_t bits = 1; bits <= 2; ++bits) {
        CHECK(fhe_oprf_lut_host(&p, bits, lut) == FHE_OK);
        for (uint32_t i = 0; i < 2048; ++i) CHECK(lut[i] == (2 * (((uint64_t)i << bits) / 4096) + 1) * half);
    }
    CHECK(fhe_oprf_lut_host(&p, 0, lut) == FHE_ERR_INVALID);
    CHECK(fhe_oprf_lut_host(&p, 3, lut) == FHE_ERR_INVALID);
    CHECK(fhe_oprf_lut_host(NULL, 1, lut) == FHE_ERR_INVALID);
    CHECK(fhe_oprf_lut_host(&p, 1, NULL) == FHE_ERR_INVALID);
    CHECK(fhe_oprf_rows_host(seed, 0, 1, 8, lut) == FHE_ERR_INVALID);
    CHECK(fhe_oprf_rows_host(seed, 2049, 1, 2056, lut) == FHE_ERR_INVALID);
    CHECK(fhe_oprf_rows_host(seed, 16, 1, 16, lut) == FHE_ERR_INVALID);
    CHECK(fhe_oprf_rows_host(NULL, 16, 1, 17, lut) == FHE_ERR_INVALID);
    CHECK(fhe_oprf_rows_host(seed, 16, 1, 17, NULL) == FHE_ERR_INVALID);
    CHECK(fhe_oprf_rows_host(seed, 16, 0, 17, NULL) == FHE_OK);
    free(lut);
    printf("oblivious pseudo-random host code: all checks passed\n");
    return 0;
}
