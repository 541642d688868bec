// public_key_host_check.c -- stand-alone driver of the host code of public-key encryption (key generation,
// encryption under the public key, the two wire kinds, host expansion, client decryption; no GPU call), for a
// host AddressSanitizer + UndefinedBehaviorSanitizer run with its own main:
//   make -C fhe-sign_amd asan
//   clang -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -shared-libsan -Iinclude \
//         tools/public_key_host_check.c -Lfhe-sign_amd/lib_asan -lfhe_rocm -Wl,-rpath,$PWD/fhe-sign_amd/lib_asan -o public_key_host_check
// (clang = the ROCm toolchain's, as for tools/seeded_host_check.c).  Under a main key of n = 16 it makes a
// public key, builds packed and unpacked lists of radix values of 2 to 4096 bits, BigUintFHE values of 0 to 9
// limbs and lists that end exactly on, one before and one after a chunk boundary, decrypts every value and every
// expanded row, round-trips both kinds, and feeds both readers every truncation and single-byte corruption
// (every byte of the first 512 and the last 64, every 509th between), payloads one word longer and shorter,
// value tables around the edges with the checksum recomputed, and each kind to the other reader.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "fhe_rocm.h"

static uint64_t fnv(const uint8_t* p, size_t n) {
    uint64_t h = 0xcbf29ce484222325ull;
    size_t i = 0;
    for (; i + 8 <= n; i += 8) { uint64_t w; memcpy(&w, p + i, 8); h = (h ^ w) * 0x100000001b3ull; }
    if (i < n) { uint64_t w = 0; memcpy(&w, p + i, n - i); h = (h ^ w) * 0x100000001b3ull; }
    return h;
}
#define CHECK(x) do { if (!(x)) { printf("FAIL line %d: %s (%s)\n", __LINE__, #x, fhe_last_error()); return 1; } } while (0)

typedef int (*reader_fn)(const uint8_t*, size_t, void**);
static int rd_key(const uint8_t* b, size_t n, void** o) { return fhe_public_key_deserialize(b, n, (fhe_public_key**)o); }
static int rd_list(const uint8_t* b, size_t n, void** o) { return fhe_compact_list_deserialize(b, n, (fhe_compact_list**)o); }

static int torture(reader_fn rd, const uint8_t* buf, size_t len) {
    for (size_t n = 0; n < len; n += (n < 512 || len - n < 64) ? 1 : 509) {  // each from a buffer of exactly that size
        uint8_t* t = malloc(n ? n : 1); memcpy(t, buf, n);
        void* x = NULL;
        CHECK(rd(t, n, &x) != 0 && !x);
        free(t);
    }
    uint8_t* t = malloc(len + 8);
    for (size_t i = 0; i < len; i += (i < 512 || len - i < 64) ? 1 : 509) {
        memcpy(t, buf, len); t[i] ^= 0x40;
        void* x = NULL;
        CHECK(rd(t, len, &x) != 0 && !x);
    }
    for (int d = -8; d <= 8; d += 16) {  // one word shorter / longer, length field and checksum right
        memcpy(t, buf, len); if (d > 0) memset(t + len, 0, 8);
        uint64_t plen = len - 32 + d; memcpy(t + 16, &plen, 8);
        uint64_t h = fnv(t + 32, len - 32 + d); memcpy(t + 24, &h, 8);
        void* x = NULL;
        CHECK(rd(t, len + d, &x) != 0 && !x);
    }
    free(t);
    return 0;
}

static uint64_t words[64];
static uint32_t limbs[9];

// a list of the given values (bits > 0: radix; bits < 0: BigUintFHE of -bits - 1 limbs), checked end to end
static int run_list(fhe_client_key* ck, const fhe_public_key* pk, const int* spec, int nspec, int packed, const uint8_t* seed) {
    fhe_compact_builder* b = NULL;
    CHECK(fhe_compact_builder_new(pk, &b) == 0);
    size_t want_coef = 0;
    for (int i = 0; i < nspec; ++i) {
        size_t nb;
        if (spec[i] > 0) { CHECK(fhe_compact_builder_push_radix(b, words, (uint32_t)spec[i]) == 0); nb = spec[i] / 2; }
        else { size_t nl = (size_t)(-spec[i] - 1); CHECK(fhe_compact_builder_push_biguint(b, nl ? limbs : NULL, nl) == 0); nb = 16 * nl; }
        want_coef += packed ? (nb + 1) / 2 : nb;
    }
    fhe_compact_list *x = NULL, *y = NULL;
    CHECK(fhe_compact_builder_build(b, packed, seed, &x) == 0);
    fhe_compact_builder_destroy(b);
    int pk_flag; uint32_t nv; size_t ncoef, nch, len;
    CHECK(fhe_compact_list_info(x, &pk_flag, &nv, &ncoef, &nch) == 0);
    CHECK(pk_flag == packed && nv == (uint32_t)nspec && ncoef == want_coef && nch == (ncoef + 2047) / 2048);
    CHECK(fhe_compact_list_serialize(x, NULL, 0, &len) == 0 && len == 76 + 8 * (size_t)nspec + 8 * (2048 * nch + ncoef));
    uint8_t* buf = malloc(len);
    CHECK(fhe_compact_list_serialize(x, buf, len, &len) == 0);
    CHECK(fhe_compact_list_serialize(x, buf, len - 1, &len) == FHE_ERR_INVALID);
    CHECK(fhe_compact_list_deserialize(buf, len, &y) == 0);
    uint64_t* ra = malloc(ncoef * 2049 * 8 + 8); uint64_t* rb = malloc(ncoef * 2049 * 8 + 8);
    CHECK(fhe_compact_list_expand_host(x, ra, ncoef * 2049) == 0 && fhe_compact_list_expand_host(y, rb, ncoef * 2049) == 0);
    CHECK(memcmp(ra, rb, ncoef * 2049 * 8) == 0);
    if (ncoef) CHECK(fhe_compact_list_expand_host(x, ra, ncoef * 2049 - 1) == FHE_ERR_INVALID);
    uint64_t* ca = malloc(nch * 2048 * 8 + 8); uint64_t* cb = malloc(ncoef * 8 + 8);
    CHECK(fhe_compact_list_export(x, ca, nch * 2048, cb, ncoef) == 0);
    if (ncoef) CHECK(fhe_compact_list_export(x, ca, nch * 2048, cb, ncoef - 1) == FHE_ERR_INVALID);
    for (int i = 0; i < nspec; ++i) {
        uint32_t form, count; size_t nb, first, nc;
        CHECK(fhe_compact_list_value_info(y, (uint32_t)i, &form, &count, &nb, &first, &nc) == 0);
        uint64_t out[64] = {0};
        CHECK(fhe_compact_list_decrypt(ck, y, (uint32_t)i, out, 64) == 0);
        for (size_t k = 0; k < nb; ++k) {
            const uint64_t got = (out[2 * k / 64] >> (2 * k % 64)) & 3;
            const uint64_t want = spec[i] > 0 ? (words[2 * k / 64] >> (2 * k % 64)) & 3 : (limbs[k / 16] >> (2 * (k % 16))) & 3;
            CHECK(got == want);
            // and the expanded row of the coefficient that holds the block
            uint64_t v;
            const size_t g = first + (packed ? k / 2 : k);
            CHECK(fhe_decrypt_block(ck, ra + g * 2049, &v) == 0);
            CHECK(((packed ? v >> (2 * (k & 1)) : v) & 3) == want);
        }
        if (nb) CHECK(fhe_compact_list_decrypt(ck, y, (uint32_t)i, out, (2 * nb + 63) / 64 - 1) == FHE_ERR_INVALID || 2 * nb <= 64);
    }
    CHECK(fhe_compact_list_value_info(y, (uint32_t)nspec, NULL, NULL, NULL, NULL, NULL) == FHE_ERR_INVALID);
    uint64_t out1[64];
    CHECK(fhe_compact_list_decrypt(ck, y, (uint32_t)nspec, out1, 64) == FHE_ERR_INVALID);
    if (len < 40000 && torture(rd_list, buf, len)) return 1;
    free(ra); free(rb); free(ca); free(cb); free(buf);
    fhe_compact_list_destroy(x); fhe_compact_list_destroy(y);
    return 0;
}

int main(void) {
    fhe_params p;
    fhe_params_default(&p);
    p.lwe_dimension = 16;
    fhe_client_key* ck; fhe_server_key* sk;
    CHECK(fhe_generate_keys(&p, 7, &ck, &sk) == 0);
    uint8_t seed[32]; for (int i = 0; i < 32; ++i) seed[i] = (uint8_t)(i * 11 + 3);
    for (int i = 0; i < 64; ++i) words[i] = 0x9E3779B97F4A7C15ull * (i + 1);
    for (int i = 0; i < 9; ++i) limbs[i] = 0xDEADBEEFu + 977u * i;

    fhe_public_key *pk = NULL, *pk2 = NULL, *pk3 = NULL;
    CHECK(fhe_public_key_generate(ck, seed, &pk) == 0);
    CHECK(fhe_public_key_generate(ck, NULL, &pk3) == 0);
    size_t klen;
    CHECK(fhe_public_key_serialize(pk, NULL, 0, &klen) == 0 && klen == 16484);
    uint8_t* kbuf = malloc(klen);
    CHECK(fhe_public_key_serialize(pk, kbuf, klen, &klen) == 0);
    CHECK(fhe_public_key_serialize(pk, kbuf, klen - 1, &klen) == FHE_ERR_INVALID);
    CHECK(fhe_public_key_deserialize(kbuf, klen, &pk2) == 0);
    uint8_t s2[32]; uint64_t* body = malloc(2048 * 8); uint64_t* body2 = malloc(2048 * 8);
    CHECK(fhe_public_key_export(pk, s2, body, 2048) == 0 && memcmp(s2, seed, 32) == 0);
    CHECK(fhe_public_key_export(pk2, NULL, body2, 2048) == 0 && memcmp(body, body2, 2048 * 8) == 0);
    CHECK(fhe_public_key_export(pk, s2, body, 2047) == FHE_ERR_INVALID);
    fhe_params q; CHECK(fhe_public_key_params(pk2, &q) == 0 && q.lwe_dimension == 16);
    if (torture(rd_key, kbuf, klen)) return 1;

    static const int mixed[] = {2, 6, -1, 32, -2, 10, 256, -10};
    static const int wide[] = {4096};
    static const int edge_a[] = {4096, 4094}, edge_b[] = {4096, 4096}, edge_c[] = {4096, 4096, 2};
    for (int packed = 0; packed <= 1; ++packed) {
        if (run_list(ck, pk2, mixed, 8, packed, packed ? NULL : seed)) return 1;
        if (run_list(ck, pk2, wide, 1, packed, seed)) return 1;
        if (run_list(ck, pk2, edge_a, 2, packed, seed)) return 1;
        if (run_list(ck, pk2, edge_b, 2, packed, seed)) return 1;
        if (run_list(ck, pk2, edge_c, 3, packed, NULL)) return 1;
        if (run_list(ck, pk2, mixed, 0, packed, seed)) return 1;  // the empty list
    }

    // value tables around the edges, checksum recomputed: a list of one 4-bit value (packed: 1 coefficient)
    {
        fhe_compact_builder* b = NULL; fhe_compact_list* x = NULL; size_t len;
        CHECK(fhe_compact_builder_new(pk, &b) == 0 && fhe_compact_builder_push_radix(b, words, 4) == 0);
        CHECK(fhe_compact_builder_build(b, 1, seed, &x) == 0);
        CHECK(fhe_compact_list_serialize(x, NULL, 0, &len) == 0);
        uint8_t* buf = malloc(len); CHECK(fhe_compact_list_serialize(x, buf, len, &len) == 0);
        uint32_t flags[] = {0, 1, 2, 0xFFFFFFFFu}, nvs[] = {0, 1, 2, 1u << 16, (1u << 16) + 1, 0xFFFFFFFFu};
        uint32_t forms[] = {0, 1, 2, 0xFFFFFFFFu};
        uint32_t counts[] = {0, 1, 2, 3, 4, 4096, 4098, 1u << 20, (1u << 20) + 1, 0xFFFFFFFFu};
        for (int a = 0; a < 4; ++a) for (int n = 0; n < 6; ++n) for (int f = 0; f < 4; ++f) for (int c = 0; c < 10; ++c) {
            uint8_t* t = malloc(len); memcpy(t, buf, len);
            memcpy(t + 68, &flags[a], 4); memcpy(t + 72, &nvs[n], 4); memcpy(t + 76, &forms[f], 4); memcpy(t + 80, &counts[c], 4);
            uint64_t h = fnv(t + 32, len - 32); memcpy(t + 24, &h, 8);
            fhe_compact_list* y = NULL;
            int rc = fhe_compact_list_deserialize(t, len, &y);
            // exactly one coefficient must come out of one value: radix 2 (either flag) or radix 4 packed
            int ok = flags[a] <= 1 && nvs[n] == 1 && forms[f] == 0 && (counts[c] == 2 || (counts[c] == 4 && flags[a] == 1));
            CHECK((rc == 0) == ok);
            fhe_compact_list_destroy(y); free(t);
        }
        // each kind to the other reader
        void* o = NULL;
        CHECK(rd_key(buf, len, &o) != 0 && !o && rd_list(kbuf, klen, &o) != 0 && !o);
        free(buf); fhe_compact_list_destroy(x);
        CHECK(fhe_compact_builder_push_radix(b, words, 3) == FHE_ERR_INVALID);
        CHECK(fhe_compact_builder_push_radix(b, words, 4098) == FHE_ERR_INVALID);
        CHECK(fhe_compact_builder_push_radix(b, words, 0) == FHE_ERR_INVALID);
        CHECK(fhe_compact_builder_push_biguint(b, limbs, ((size_t)1 << 20) + 1) == FHE_ERR_INVALID);
        CHECK(fhe_compact_builder_push_biguint(b, NULL, 1) == FHE_ERR_INVALID);
        fhe_compact_builder_destroy(b);
    }
    CHECK(fhe_compact_list_expand_radix(NULL, NULL, 0, NULL) != 0);
    CHECK(fhe_compact_list_extract_rows(NULL, NULL, NULL, 0) != 0);
    CHECK(fhe_public_key_generate(NULL, seed, &pk) == FHE_ERR_INVALID);
    free(kbuf); free(body); free(body2);
    fhe_public_key_destroy(pk); fhe_public_key_destroy(pk2); fhe_public_key_destroy(pk3);
    fhe_client_key_destroy(ck); fhe_server_key_destroy(sk);
    printf("public-key host code: all checks passed\n");
    return 0;
}
