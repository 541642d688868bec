// rerandomize_host_check.c -- stand-alone driver of the host code of the re-randomization under the public key
// (fhe_rerandomize_host, fhe_rerandomize_zero_host, fhe_rerandomize_seed; no GPU call), for a host
// AddressSanitizer + UndefinedBehaviorSanitizer run with its own main:
//   make -C fhe-sign_amd asan
//   clang -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -shared-libsan -Iinclude \
//         tools/rerandomize_host_check.c -Lfhe-sign_amd/lib_asan -lfhe_rocm -Wl,-rpath,$PWD/fhe-sign_amd/lib_asan \
//         -Wl,-rpath,$(dirname $(clang -print-file-name=libclang_rt.asan-x86_64.so)) -o rerandomize_host_check
// (clang = the ROCm toolchain's, as for tools/public_key_host_check.c; the second rpath finds the shared
// sanitizer runtime, so the program runs as it is).  Under a main key of n = 16 it makes a
// public key and, at 0, 1, 2, 3, 128, 2047, 2048, 2049 and 4097 blocks, re-randomizes encryptions of every block
// value in buffers of exactly the rows' size, checks that every row still decrypts, that the call is deterministic,
// that two seeds differ, that rows = input + the extraction of the exported zero encryptions at t = 0, and that
// trivial rows come out as ciphertexts; then the seed helper against a fixed vector and every refusal.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "fhe_rocm.h"

#define CHECK(x) do { if (!(x)) { printf("FAIL line %d: %s (%s)\n", __LINE__, #x, fhe_last_error()); return 1; } } while (0)
#define ROW 2049

static int run(fhe_client_key* ck, const fhe_public_key* pk, size_t n, const uint8_t* seed, const uint8_t* seed2) {
    const size_t chunks = (n + 2047) / 2048;
    uint64_t* vals = malloc(n ? n * 8 : 1);
    uint64_t* rows = malloc(n ? n * ROW * 8 : 1);  // exactly the rows: a word past the end is the sanitizer's
    uint64_t* a = malloc(n ? n * ROW * 8 : 1);
    uint64_t* b = malloc(n ? n * ROW * 8 : 1);
    uint64_t* za = malloc(chunks ? chunks * 2048 * 8 : 1);
    uint64_t* zb = malloc(n ? n * 8 : 1);
    for (size_t i = 0; i < n; ++i) vals[i] = i % 16;
    CHECK(fhe_encrypt_blocks(ck, vals, n, rows) == 0 || n == 0);
    if (n) memcpy(a, rows, n * ROW * 8), memcpy(b, rows, n * ROW * 8);
    CHECK(fhe_rerandomize_host(pk, seed, a, n) == 0);
    CHECK(fhe_rerandomize_host(pk, seed, b, n) == 0);
    CHECK(n == 0 || memcmp(a, b, n * ROW * 8) == 0);
    CHECK(fhe_rerandomize_zero_host(pk, seed, n, za, chunks * 2048, zb, n) == 0);
    for (size_t i = 0; i < n; ++i) {
        uint64_t v = 99;
        CHECK(fhe_decrypt_block(ck, a + i * ROW, &v) == 0 && v == vals[i]);
        CHECK(a[i * ROW + 2048] == rows[i * ROW + 2048] + zb[i]);
        const size_t t = i % 2048;
        CHECK(a[i * ROW + t] == rows[i * ROW + t] + za[i / 2048 * 2048]);  // mask word u = t takes Z_A[0]
        CHECK(a[i * ROW] == rows[i * ROW] + za[i / 2048 * 2048 + t]);      // mask word 0 takes Z_A[t]
        if (t + 1 < 2048) CHECK(a[i * ROW + t + 1] == rows[i * ROW + t + 1] - za[i / 2048 * 2048 + 2047]);
    }
    if (n) {
        memcpy(b, rows, n * ROW * 8);
        CHECK(fhe_rerandomize_host(pk, seed2, b, n) == 0);
        CHECK(memcmp(a, b, 2048 * 8) != 0);
        // trivial rows: mask 0, body delta value
        memset(b, 0, n * ROW * 8);
        for (size_t i = 0; i < n; ++i) b[i * ROW + 2048] = vals[i] << 59;
        CHECK(fhe_rerandomize_host(pk, seed, b, n) == 0);
        for (size_t i = 0; i < n; ++i) {
            uint64_t v = 99;
            CHECK(fhe_decrypt_block(ck, b + i * ROW, &v) == 0 && v == vals[i]);
            CHECK(b[i * ROW] == za[i / 2048 * 2048 + i % 2048]);
        }
        // buffers one short are refused before a word is written
        CHECK(fhe_rerandomize_zero_host(pk, seed, n, za, chunks * 2048 - 1, zb, n) == FHE_ERR_INVALID);
        CHECK(fhe_rerandomize_zero_host(pk, seed, n, za, chunks * 2048, zb, n - 1) == FHE_ERR_INVALID);
    }
    free(vals); free(rows); free(a); free(b); free(za); free(zb);
    return 0;
}

int main(void) {
    fhe_params p;
    fhe_params_default(&p);
    p.lwe_dimension = 16;
    fhe_client_key* ck; fhe_server_key* sk;
    CHECK(fhe_generate_keys(&p, 7, &ck, &sk) == 0);
    uint8_t seed[32], seed2[32];
    for (int i = 0; i < 32; ++i) seed[i] = (uint8_t)(i * 13 + 5), seed2[i] = (uint8_t)(i * 7 + 1);
    fhe_public_key* pk = NULL;
    CHECK(fhe_public_key_generate(ck, seed2, &pk) == 0);

    static const size_t sizes[] = {0, 1, 2, 3, 128, 2047, 2048, 2049, 4097};
    for (size_t k = 0; k < sizeof sizes / sizeof sizes[0]; ++k)
        if (run(ck, pk, sizes[k], seed, seed2)) return 1;

    // the seed helper: SHA-256(T || T || u64le(6) || "domain" || "data"), T = SHA-256("fhe-rocm/rerandomize")
    uint8_t h[32], h2[32];
    CHECK(fhe_rerandomize_seed((const uint8_t*)"domain", 6, (const uint8_t*)"data", 4, h) == 0);
    CHECK(fhe_rerandomize_seed((const uint8_t*)"domaind", 7, (const uint8_t*)"ata", 3, h2) == 0 && memcmp(h, h2, 32) != 0);
    CHECK(fhe_rerandomize_seed((const uint8_t*)"domain", 6, (const uint8_t*)"data", 4, h2) == 0 && memcmp(h, h2, 32) == 0);
    CHECK(fhe_rerandomize_seed(NULL, 0, NULL, 0, h2) == 0 && memcmp(h, h2, 32) != 0);
    {   // long inputs from buffers of exactly their size
        uint8_t* d = malloc(1000); uint8_t* m = malloc(777);
        memset(d, 0xA5, 1000); memset(m, 0x5A, 777);
        CHECK(fhe_rerandomize_seed(d, 1000, m, 777, h2) == 0);
        free(d); free(m);
    }
    CHECK(fhe_rerandomize_seed(NULL, 1, (const uint8_t*)"x", 1, h) == FHE_ERR_INVALID);
    CHECK(fhe_rerandomize_seed((const uint8_t*)"x", 1, NULL, 1, h) == FHE_ERR_INVALID);
    CHECK(fhe_rerandomize_seed((const uint8_t*)"x", 1, (const uint8_t*)"x", 1, NULL) == FHE_ERR_INVALID);

    uint64_t row[ROW] = {0}, zb1[1], *za1 = malloc(2048 * 8);
    CHECK(fhe_rerandomize_host(NULL, seed, row, 1) == FHE_ERR_INVALID);
    CHECK(fhe_rerandomize_host(pk, NULL, row, 1) == FHE_ERR_INVALID);
    CHECK(fhe_rerandomize_host(pk, seed, NULL, 1) == FHE_ERR_INVALID);
    CHECK(fhe_rerandomize_host(pk, seed, NULL, 0) == 0);
    CHECK(fhe_rerandomize_host(pk, seed, row, ((size_t)1 << 24) + 1) == FHE_ERR_INVALID);
    for (int i = 0; i < ROW; ++i) CHECK(row[i] == 0);
    CHECK(fhe_rerandomize_zero_host(NULL, seed, 1, za1, 2048, zb1, 1) == FHE_ERR_INVALID);
    CHECK(fhe_rerandomize_zero_host(pk, NULL, 1, za1, 2048, zb1, 1) == FHE_ERR_INVALID);
    CHECK(fhe_rerandomize_zero_host(pk, seed, 1, NULL, 2048, zb1, 1) == FHE_ERR_INVALID);
    CHECK(fhe_rerandomize_zero_host(pk, seed, ((size_t)1 << 24) + 1, za1, 2048, zb1, 1) == FHE_ERR_INVALID);
    CHECK(fhe_set_public_key(NULL, pk) == FHE_ERR_INVALID);
    CHECK(fhe_radix_rerandomize(NULL, NULL, seed, NULL) != 0);
    CHECK(fhe_biguint_rerandomize(NULL, NULL, seed, NULL) != 0);
    CHECK(fhe_rerandomize_rows(NULL, seed, row, 1, row) != 0);
    free(za1);
    fhe_public_key_destroy(pk);
    fhe_client_key_destroy(ck); fhe_server_key_destroy(sk);
    printf("re-randomization host code: all checks passed\n");
    return 0;
}
