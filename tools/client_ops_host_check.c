// client_ops_host_check.c -- stand-alone driver of the host code of the resident client key (DESIGN.md 6m:
// fhe_client_encrypt_rows_indexed_host, fhe_decrypt_phase_host, the stream accounting of keys.cpp's
// encrypt_big_skip; no GPU call), for a host AddressSanitizer + UndefinedBehaviorSanitizer run with its own main:
// tools/asan_client_ops_host.sh builds and runs it (the recipe of tools/rerandomize_host_check.c).
// It repeats the addressing sweep of tests/test_client_ops.py: twin client keys (one key deserialized twice,
// seed_encryption(42, 100)) at stream positions W0 = 0, 3 and 2049 + 5 u64 words, batches of 1, 2, 7, 8, 9, 65 and
// 129 blocks; the indexed rows, written into a buffer of exactly their size, must equal fhe_encrypt_blocks' rows,
// the two keys must serialize to the same bytes afterwards and encrypt the same next block; every row must decrypt,
// and fhe_decrypt_phase_host must give the word fhe_decrypt_block decodes.  Then the refusals, and a simulated
// context's refusal of the three residency entry points.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "fhe_rocm.h"

#define CHECK(x) do { if (!(x)) { printf("FAIL line %d: %s (%s)\n", __LINE__, #x, fhe_last_error()); return 1; } } while (0)
#define ROW 2049

static uint8_t* key_bytes;
static size_t key_len;

// a twin at u64 stream word w0: a full block draws 2049 words, a seeded block one
static int twin(size_t w0, fhe_client_key** out) {
    fhe_client_key* ck = NULL;
    CHECK(fhe_client_key_deserialize(key_bytes, key_len, &ck) == 0);
    CHECK(fhe_client_key_seed_encryption(ck, 42, 100) == 0);
    if (w0 >= ROW) {
        uint64_t* row = malloc(ROW * 8);
        CHECK(fhe_encrypt_block(ck, 1, row) == 0);
        free(row);
        w0 -= ROW;
    }
    if (w0) {
        uint8_t seed[32];
        for (int i = 0; i < 32; ++i) seed[i] = (uint8_t)i;
        uint64_t zero = 0;
        fhe_seeded* s = NULL;
        CHECK(fhe_radix_encrypt_seeded(ck, &zero, (uint32_t)(2 * w0), seed, &s) == 0);
        fhe_seeded_destroy(s);
    }
    *out = ck;
    return 0;
}

static int same_keys(const fhe_client_key* a, const fhe_client_key* b) {
    size_t la = 0, lb = 0;
    CHECK(fhe_client_key_serialize(a, NULL, 0, &la) == 0 && fhe_client_key_serialize(b, NULL, 0, &lb) == 0 && la == lb);
    uint8_t* ba = malloc(la);
    uint8_t* bb = malloc(lb);
    CHECK(fhe_client_key_serialize(a, ba, la, &la) == 0 && fhe_client_key_serialize(b, bb, lb, &lb) == 0);
    CHECK(memcmp(ba, bb, la) == 0);
    free(ba); free(bb);
    return 0;
}

static int run(size_t w0, size_t n) {
    fhe_client_key *a = NULL, *b = NULL;
    if (twin(w0, &a) || twin(w0, &b)) return 1;
    uint64_t* vals = malloc(n * 8);
    uint64_t* want = malloc(n * ROW * 8);  // exactly the rows: a word past the end is the sanitizer's
    uint64_t* got = malloc(n * ROW * 8);
    uint64_t* ph = malloc(n * 8);
    for (size_t i = 0; i < n; ++i) vals[i] = (7 * i + 3) % 16;
    CHECK(fhe_encrypt_blocks(a, vals, n, want) == 0);
    CHECK(fhe_client_encrypt_rows_indexed_host(b, vals, n, got) == 0);
    for (size_t i = 0; i < n * ROW; ++i)
        if (want[i] != got[i]) {
            printf("FAIL W0 %zu, %zu blocks: row %zu word %zu\n", w0, n, i / ROW, i % ROW);
            return 1;
        }
    if (same_keys(a, b)) return 1;
    CHECK(fhe_decrypt_phase_host(b, got, n, ph) == 0);
    for (size_t i = 0; i < n; ++i) {
        uint64_t v = 99;
        CHECK(fhe_decrypt_block(a, got + i * ROW, &v) == 0 && v == vals[i]);
        CHECK(((ph[i] + (1ull << 58)) >> 59) % 16 == vals[i]);
    }
    uint64_t five = 5;
    CHECK(fhe_encrypt_blocks(a, &five, 1, want) == 0 && fhe_encrypt_blocks(b, &five, 1, got) == 0);
    CHECK(memcmp(want, got, ROW * 8) == 0);
    free(vals); free(want); free(got); free(ph);
    fhe_client_key_destroy(a); fhe_client_key_destroy(b);
    return 0;
}

int main(void) {
    fhe_params p;
    fhe_params_default(&p);
    p.lwe_dimension = 16;
    fhe_client_key* ck; fhe_server_key* sk;
    CHECK(fhe_generate_keys(&p, 0xC11E, &ck, &sk) == 0);
    CHECK(fhe_client_key_serialize(ck, NULL, 0, &key_len) == 0);
    key_bytes = malloc(key_len);
    CHECK(fhe_client_key_serialize(ck, key_bytes, key_len, &key_len) == 0);

    static const size_t w0s[] = {0, 3, 2049 + 5};
    static const size_t counts[] = {1, 2, 7, 8, 9, 65, 129};
    for (size_t w = 0; w < sizeof w0s / sizeof w0s[0]; ++w)
        for (size_t k = 0; k < sizeof counts / sizeof counts[0]; ++k)
            if (run(w0s[w], counts[k])) return 1;

    uint64_t one = 1, sixteen = 16, ph1[1];
    uint64_t* row = calloc(ROW, 8);
    CHECK(fhe_client_encrypt_rows_indexed_host(NULL, &one, 1, row) == FHE_ERR_INVALID);
    CHECK(fhe_client_encrypt_rows_indexed_host(ck, NULL, 1, row) == FHE_ERR_INVALID);
    CHECK(fhe_client_encrypt_rows_indexed_host(ck, &one, 1, NULL) == FHE_ERR_INVALID);
    CHECK(fhe_client_encrypt_rows_indexed_host(ck, &sixteen, 1, row) == FHE_ERR_INVALID);
    CHECK(fhe_client_encrypt_rows_indexed_host(ck, NULL, 0, NULL) == 0);
    for (int i = 0; i < ROW; ++i) CHECK(row[i] == 0);
    CHECK(fhe_decrypt_phase_host(NULL, row, 1, ph1) == FHE_ERR_INVALID);
    CHECK(fhe_decrypt_phase_host(ck, NULL, 1, ph1) == FHE_ERR_INVALID);
    CHECK(fhe_decrypt_phase_host(ck, row, 1, NULL) == FHE_ERR_INVALID);
    CHECK(fhe_decrypt_phase_host(ck, NULL, 0, NULL) == 0);
    int resident = 7;
    uint64_t e = 7, d = 7;
    float f, g;
    CHECK(fhe_ctx_set_client_key(NULL, ck) == FHE_ERR_INVALID);
    CHECK(fhe_ctx_clear_client_key(NULL) == FHE_ERR_INVALID);
    CHECK(fhe_ctx_client_ops_info(NULL, &resident, &e, &d) == FHE_ERR_INVALID);
    CHECK(fhe_client_encrypt_rows(NULL, ck, &one, 1, row) == FHE_ERR_INVALID);
    CHECK(fhe_client_phase_rows(NULL, row, 1, ph1) == FHE_ERR_INVALID);
    CHECK(fhe_ctx_time_client_ops(NULL, 1, 1, &f, &g) == FHE_ERR_INVALID);
    fhe_ctx* sim = NULL;
    CHECK(fhe_host_sim_ctx_create(&sim) == 0);
    CHECK(fhe_ctx_set_client_key(sim, ck) == FHE_ERR_INVALID && strstr(fhe_last_error(), "simulated context"));
    CHECK(fhe_ctx_clear_client_key(sim) == FHE_ERR_INVALID && strstr(fhe_last_error(), "simulated context"));
    CHECK(fhe_ctx_client_ops_info(sim, &resident, &e, &d) == FHE_ERR_INVALID && resident == 7);
    CHECK(fhe_client_encrypt_rows(sim, ck, &one, 1, row) == FHE_ERR_INVALID);
    CHECK(fhe_client_phase_rows(sim, row, 1, ph1) == FHE_ERR_INVALID);
    fhe_ctx_destroy(sim);
    free(row); free(key_bytes);
    fhe_client_key_destroy(ck); fhe_server_key_destroy(sk);
    printf("client ops host check: all checks passed\n");
    return 0;
}
