// ct_digest_host_check.c -- stand-alone driver of the host code of the ciphertext digests and the re-randomization
// context (fhe_ct_digest_host, fhe_ct_value_digest_host, fhe_rerand_context_*; no GPU call), for a host
// AddressSanitizer + UndefinedBehaviorSanitizer run with its own main:
//   make -C fhe-sign_amd asan
//   clang -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -shared-libsan -Iinclude \
//         tools/ct_digest_host_check.c -Lfhe-sign_amd/lib_asan -lfhe_rocm -Wl,-rpath,$PWD/fhe-sign_amd/lib_asan \
//         -Wl,-rpath,$(dirname $(clang -print-file-name=libclang_rt.asan-x86_64.so)) -o ct_digest_host_check
// (clang = the ROCm toolchain's, as for tools/rerandomize_host_check.c; the second rpath finds the shared
// sanitizer runtime, so the program runs as it is).  It digests 0, 1, 2, 3, 65 and 300 rows from buffers of exactly
// the rows' size into buffers of exactly 32 bytes per row, checks the two pinned rows, that the call is deterministic,
// that every one-bit flip at the leaf edge, the node edge, the last mask word and the body changes exactly its own
// row's digest; value digests from exact-size arrays; the context with empty, short and long items, a fixed seed
// vector, order, the refusal of an add after a seed; then every null or oversized argument.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "fhe_rocm.h"

#define CHECK(x) do { if (!(x)) { printf("FAIL line %d: %s (%s)\n", __LINE__, #x, fhe_last_error()); return 1; } } while (0)
#define ROW 2049
// hashlib: seed(7) of the context over domain "d" with the items bytes "ab", digest 00 01 .. 1f
#define SEED_VECTOR "cbc9adc5c814a7a1e2e6c22f2a22a1e3357e71d5db64eb4d836717f97ca7103a"

static int hex_is(const uint8_t* d, const char* hex) {
    char buf[65];
    for (int i = 0; i < 32; ++i) sprintf(buf + 2 * i, "%02x", d[i]);
    return strcmp(buf, hex) == 0;
}

static uint64_t next(uint64_t* s) {  // splitmix64
    uint64_t z = (*s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static int run(size_t n) {
    uint64_t s = 0xC7D16E57ull + n;
    uint64_t* rows = malloc(n ? n * ROW * 8 : 1);  // exactly the rows: a word past the end is the sanitizer's
    uint8_t* a = malloc(n ? n * 32 : 1);
    uint8_t* b = malloc(n ? n * 32 : 1);
    for (size_t i = 0; i < n * ROW; ++i) rows[i] = next(&s);
    CHECK(fhe_ct_digest_host(rows, n, a) == 0);
    CHECK(fhe_ct_digest_host(rows, n, b) == 0);
    CHECK(n == 0 || memcmp(a, b, n * 32) == 0);
    for (size_t i = 0; i + 1 < n; ++i) CHECK(memcmp(a + 32 * i, a + 32 * (i + 1), 32) != 0);
    static const size_t flips[] = {0, 31, 32, 255, 256, 2047, 2048};
    for (size_t k = 0; n && k < sizeof flips / sizeof flips[0]; ++k) {
        const size_t r = (k * 7) % n;
        rows[r * ROW + flips[k]] ^= 1ull << (flips[k] % 64);
        CHECK(fhe_ct_digest_host(rows, n, b) == 0);
        for (size_t i = 0; i < n; ++i) CHECK((memcmp(a + 32 * i, b + 32 * i, 32) != 0) == (i == r));
        rows[r * ROW + flips[k]] ^= 1ull << (flips[k] % 64);
    }
    // value digests from arrays of exactly n entries
    uint8_t* tags = malloc(n ? n : 1);
    uint32_t* deg = malloc(n ? n * 4 : 1);
    uint32_t* noi = malloc(n ? n * 4 : 1);
    for (size_t i = 0; i < n; ++i) tags[i] = (uint8_t)(i & 1), deg[i] = (uint32_t)(i % 16), noi[i] = (uint32_t)(i % 25 + 1);
    uint8_t d0[32], d1[32];
    CHECK(fhe_ct_value_digest_host(FHE_CT_KIND_RADIX, (uint32_t)(2 * n), tags, deg, noi, a, n, d0) == 0);
    CHECK(fhe_ct_value_digest_host(FHE_CT_KIND_RADIX, (uint32_t)(2 * n), tags, deg, noi, a, n, d1) == 0 && memcmp(d0, d1, 32) == 0);
    CHECK(fhe_ct_value_digest_host(FHE_CT_KIND_BIGUINT, (uint32_t)(2 * n), tags, deg, noi, a, n, d1) == 0 && memcmp(d0, d1, 32) != 0);
    if (n) {
        deg[n - 1] ^= 1;
        CHECK(fhe_ct_value_digest_host(FHE_CT_KIND_RADIX, (uint32_t)(2 * n), tags, deg, noi, a, n, d1) == 0 && memcmp(d0, d1, 32) != 0);
    }
    free(rows); free(a); free(b); free(tags); free(deg); free(noi);
    return 0;
}

int main(void) {
    static const size_t sizes[] = {0, 1, 2, 3, 65, 300};
    for (size_t k = 0; k < sizeof sizes / sizeof sizes[0]; ++k)
        if (run(sizes[k])) return 1;

    // the pinned rows: all zero; word i = (i + 1) 0x0123456789ABCDEF
    uint64_t* two = calloc(2 * ROW, 8);
    uint8_t d[64], h[32], h2[32];
    for (size_t i = 0; i < ROW; ++i) two[ROW + i] = (uint64_t)(i + 1) * 0x0123456789ABCDEFull;
    CHECK(fhe_ct_digest_host(two, 2, d) == 0);
    CHECK(hex_is(d, "3c4ea852595c986cd5f1502f0b051cc3e145cdc099d76615e86ddf72455bc628"));
    CHECK(hex_is(d + 32, "d485c2a9c9757a3cb8fdae6059fb8e4a3396c53cffd8755fa672ad695f5fb5e0"));

    // the context: items of every length from exact-size buffers, order, finalization
    fhe_rerand_context *rc = NULL, *rc2 = NULL;
    CHECK(fhe_rerand_context_new((const uint8_t*)"domain", 6, &rc) == 0 && rc);
    static const size_t lens[] = {0, 1, 55, 56, 63, 64, 65, 777, 100000};
    for (size_t k = 0; k < sizeof lens / sizeof lens[0]; ++k) {
        uint8_t* m = malloc(lens[k] ? lens[k] : 1);
        memset(m, (int)(0x5A + k), lens[k]);
        CHECK(fhe_rerand_context_add_bytes(rc, lens[k] ? m : NULL, lens[k]) == 0);
        free(m);
    }
    CHECK(fhe_rerand_context_add_digest(rc, d) == 0);
    CHECK(fhe_rerand_context_seed(rc, 0, h) == 0);
    CHECK(fhe_rerand_context_seed(rc, 0, h2) == 0 && memcmp(h, h2, 32) == 0);
    CHECK(fhe_rerand_context_seed(rc, 1, h2) == 0 && memcmp(h, h2, 32) != 0);
    CHECK(fhe_rerand_context_seed(rc, ~0ull, h2) == 0 && memcmp(h, h2, 32) != 0);
    CHECK(fhe_rerand_context_add_bytes(rc, (const uint8_t*)"x", 1) == FHE_ERR_INVALID);
    CHECK(fhe_rerand_context_add_digest(rc, d) == FHE_ERR_INVALID);
    CHECK(fhe_rerand_context_add_radix(NULL, rc, (const fhe_radix*)d) == FHE_ERR_INVALID);    // refused before x is read
    CHECK(fhe_rerand_context_add_biguint(NULL, rc, (const fhe_biguint*)d) == FHE_ERR_INVALID);
    CHECK(fhe_rerand_context_seed(rc, 0, h2) == 0 && memcmp(h, h2, 32) == 0);
    // SHA-256 framing fixed by the header: domain "d", bytes "ab", digest 00 .. 1f -> seed(7)
    CHECK(fhe_rerand_context_new((const uint8_t*)"d", 1, &rc2) == 0);
    for (int i = 0; i < 32; ++i) h2[i] = (uint8_t)i;
    CHECK(fhe_rerand_context_add_bytes(rc2, (const uint8_t*)"ab", 2) == 0);
    CHECK(fhe_rerand_context_add_digest(rc2, h2) == 0);
    CHECK(fhe_rerand_context_seed(rc2, 7, h) == 0);
    CHECK(hex_is(h, SEED_VECTOR));
    fhe_rerand_context_destroy(rc2);
    // order matters
    uint8_t s1[32], s2[32];
    CHECK(fhe_rerand_context_new(NULL, 0, &rc2) == 0);
    CHECK(fhe_rerand_context_add_digest(rc2, d) == 0 && fhe_rerand_context_add_digest(rc2, d + 32) == 0);
    CHECK(fhe_rerand_context_seed(rc2, 0, s1) == 0);
    fhe_rerand_context_destroy(rc2);
    CHECK(fhe_rerand_context_new(NULL, 0, &rc2) == 0);
    CHECK(fhe_rerand_context_add_digest(rc2, d + 32) == 0 && fhe_rerand_context_add_digest(rc2, d) == 0);
    CHECK(fhe_rerand_context_seed(rc2, 0, s2) == 0 && memcmp(s1, s2, 32) != 0);
    fhe_rerand_context_destroy(rc2);

    // refusals
    uint8_t tag1 = 1, tag2 = 2;
    uint32_t one = 1;
    CHECK(fhe_ct_digest_host(NULL, 1, d) == FHE_ERR_INVALID);
    CHECK(fhe_ct_digest_host(two, 1, NULL) == FHE_ERR_INVALID);
    CHECK(fhe_ct_digest_host(NULL, 0, NULL) == 0);
    CHECK(fhe_ct_digest_host(two, ((size_t)1 << 24) + 1, d) == FHE_ERR_INVALID);
    CHECK(fhe_ct_value_digest_host(0, 2, NULL, &one, &one, d, 1, h) == FHE_ERR_INVALID);
    CHECK(fhe_ct_value_digest_host(0, 2, &tag1, NULL, &one, d, 1, h) == FHE_ERR_INVALID);
    CHECK(fhe_ct_value_digest_host(0, 2, &tag1, &one, NULL, d, 1, h) == FHE_ERR_INVALID);
    CHECK(fhe_ct_value_digest_host(0, 2, &tag1, &one, &one, NULL, 1, h) == FHE_ERR_INVALID);
    CHECK(fhe_ct_value_digest_host(0, 2, &tag1, &one, &one, d, 1, NULL) == FHE_ERR_INVALID);
    CHECK(fhe_ct_value_digest_host(0, 2, &tag1, &one, &one, d, ((size_t)1 << 24) + 1, h) == FHE_ERR_INVALID);
    CHECK(fhe_ct_value_digest_host(2, 2, &tag1, &one, &one, d, 1, h) == FHE_ERR_INVALID);
    CHECK(fhe_ct_value_digest_host(0, 2, &tag2, &one, &one, d, 1, h) == FHE_ERR_INVALID);
    CHECK(fhe_ct_value_digest_host(1, 0, NULL, NULL, NULL, NULL, 0, h) == 0);
    CHECK(fhe_rerand_context_new(NULL, 1, &rc2) == FHE_ERR_INVALID);
    CHECK(fhe_rerand_context_new((const uint8_t*)"d", 1, NULL) == FHE_ERR_INVALID);
    CHECK(fhe_rerand_context_add_bytes(NULL, d, 1) == FHE_ERR_INVALID);
    CHECK(fhe_rerand_context_add_digest(NULL, d) == FHE_ERR_INVALID);
    CHECK(fhe_rerand_context_seed(NULL, 0, h) == FHE_ERR_INVALID);
    CHECK(fhe_rerand_context_seed(rc, 0, NULL) == FHE_ERR_INVALID);
    CHECK(fhe_radix_digest(NULL, NULL, h) != 0);
    CHECK(fhe_biguint_digest(NULL, NULL, h) != 0);
    CHECK(fhe_ct_digest_rows(NULL, two, 1, d) != 0);
    float ms;
    CHECK(fhe_ctx_time_ct_digest(NULL, 1, 1, &ms) != 0);
    CHECK(fhe_schnorr_sign_fhe_with_k0_rerand(NULL, NULL, NULL, 0, NULL, NULL, NULL, 0, NULL, 0, NULL) != 0);
    fhe_rerand_context_destroy(rc);
    fhe_rerand_context_destroy(NULL);
    free(two);
    printf("ciphertext digest host code: all checks passed\n");
    return 0;
}
