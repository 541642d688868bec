// seeded_key_host_check.c -- stand-alone driver of the seeded server key's host code (generation, wire
// format, host expansion; no GPU call), for a host AddressSanitizer + UndefinedBehaviorSanitizer run with
// its own main:
//   make -C fhe-sign_amd asan
//   clang -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -shared-libsan -Iinclude \
//         tools/seeded_key_host_check.c -Lfhe-sign_amd/lib_asan -lfhe_rocm -Wl,-rpath,$PWD/fhe-sign_amd/lib_asan -o seeded_key_host_check
// (clang = the ROCm toolchain's, so that the sanitizer runtime matches the library's; where the loader does
// not find that runtime, add -Wl,-rpath,$(clang -print-runtime-dir)).  At n = 16, classic
// and multi-bit, it generates a seeded key, round-trips it, expands it on the host and checks every KSK
// row's phase against the noise bound; at n = 1 it feeds the reader every truncation and every single-byte
// corruption of a key, and payloads one word longer and shorter with the checksum recomputed.
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

static size_t ggsw(const fhe_params* p) { return p->grouping == 2 ? p->lwe_dimension / 2 * 3 : p->lwe_dimension; }

static int one_set(uint32_t n, uint32_t grouping) {
    fhe_params p;
    fhe_params_default(&p);
    p.lwe_dimension = n;
    p.grouping = grouping;
    fhe_client_key* ck; fhe_server_key* unused;
    CHECK(fhe_generate_keys(&p, 11, &ck, &unused) == 0);
    fhe_server_key_destroy(unused);
    uint8_t seed[32]; for (int i = 0; i < 32; ++i) seed[i] = (uint8_t)(i * 5 + 3);
    fhe_seeded_server_key *s = NULL, *d = NULL, *r = NULL;
    CHECK(fhe_server_key_generate_seeded(ck, seed, &s) == 0);
    CHECK(fhe_server_key_generate_seeded(ck, NULL, &r) == 0);  // OS entropy
    fhe_params q;
    CHECK(fhe_seeded_server_key_params(s, &q) == 0 && q.lwe_dimension == n && q.grouping == grouping);
    const size_t rows = 2048 * 5, ng = ggsw(&p), want = 100 + 8 * (rows + 4096 * ng);
    size_t len = 0;
    CHECK(fhe_seeded_server_key_serialize(s, NULL, 0, &len) == 0 && len == want);
    uint8_t* buf = malloc(len);
    CHECK(fhe_seeded_server_key_serialize(s, buf, len, &len) == 0);
    CHECK(fhe_seeded_server_key_serialize(s, buf, len - 1, &len) == FHE_ERR_INVALID);
    CHECK(memcmp(buf + 68, seed, 32) == 0);
    CHECK(fhe_seeded_server_key_deserialize(buf, len, &d) == 0);
    uint8_t* buf2 = malloc(len);
    CHECK(fhe_seeded_server_key_serialize(d, buf2, len, &len) == 0 && memcmp(buf, buf2, len) == 0);
    // host expansion of both handles: the same words
    fhe_server_key *a = NULL, *b = NULL;
    CHECK(fhe_seeded_server_key_expand_host(s, &a) == 0 && fhe_seeded_server_key_expand_host(d, &b) == 0);
    const size_t kw = rows * (n + 1), bw = ng * 4 * 2048;
    uint64_t *ka = malloc(kw * 8), *ba = malloc(bw * 8), *kb = malloc(kw * 8), *bb = malloc(bw * 8);
    CHECK(fhe_server_key_export(a, ka, kw, ba, bw) == 0 && fhe_server_key_export(b, kb, kw, bb, bw) == 0);
    CHECK(fhe_server_key_export(a, ka, kw - 1, ba, bw) == FHE_ERR_INVALID);
    CHECK(memcmp(ka, kb, kw * 8) == 0 && memcmp(ba, bb, bw * 8) == 0);
    // every KSK row decrypts to its gadget value within the noise bound 2^45
    uint64_t *lwe = malloc(n * 8), *glwe = malloc(2048 * 8);
    CHECK(fhe_client_key_export(ck, lwe, n, glwe, 2048) == 0);
    for (size_t row = 0; row < rows; ++row) {
        const uint64_t* w = ka + row * (n + 1);
        uint64_t dot = 0;
        for (uint32_t t = 0; t < n; ++t) dot += w[t] * lwe[t];
        const size_t j = row / 5, l = row % 5;
        const int64_t e = (int64_t)(w[n] - dot - (glwe[j] << (64 - 3 * (l + 1))));
        CHECK(e >= -((int64_t)1 << 45) && e <= ((int64_t)1 << 45));
        uint64_t wire; memcpy(&wire, buf + 100 + 8 * row, 8);  // bodies start 4-byte aligned
        CHECK(w[n] == wire);
    }
    // the full key of the expansion serializes and reads back as an ordinary server key
    size_t flen = 0;
    CHECK(fhe_server_key_serialize(a, NULL, 0, &flen) == 0);
    uint8_t* fbuf = malloc(flen);
    fhe_server_key* back = NULL;
    CHECK(fhe_server_key_serialize(a, fbuf, flen, &flen) == 0 && fhe_server_key_deserialize(fbuf, flen, &back) == 0);
    // the two kinds refuse each other
    fhe_seeded_server_key* x = NULL; fhe_server_key* y = NULL;
    CHECK(fhe_seeded_server_key_deserialize(fbuf, flen, &x) == FHE_ERR_INVALID && !x && strstr(fhe_last_error(), "kind"));
    CHECK(fhe_server_key_deserialize(buf, len, &y) == FHE_ERR_INVALID && !y && strstr(fhe_last_error(), "kind"));
    free(fbuf); free(lwe); free(glwe); free(ka); free(ba); free(kb); free(bb); free(buf); free(buf2);
    fhe_server_key_destroy(a); fhe_server_key_destroy(b); fhe_server_key_destroy(back);
    fhe_seeded_server_key_destroy(s); fhe_seeded_server_key_destroy(d); fhe_seeded_server_key_destroy(r);
    fhe_client_key_destroy(ck);
    return 0;
}

static int reader(void) {
    fhe_params p;
    fhe_params_default(&p);
    p.lwe_dimension = 1;  // the smallest key: 100 + 8 (10240 + 4096) bytes
    fhe_client_key* ck; fhe_server_key* unused;
    CHECK(fhe_generate_keys(&p, 12, &ck, &unused) == 0);
    fhe_server_key_destroy(unused);
    fhe_seeded_server_key* s = NULL;
    CHECK(fhe_server_key_generate_seeded(ck, NULL, &s) == 0);
    size_t len = 0;
    CHECK(fhe_seeded_server_key_serialize(s, NULL, 0, &len) == 0 && len == 100 + 8 * (10240 + 4096));
    uint8_t* buf = malloc(len);
    CHECK(fhe_seeded_server_key_serialize(s, buf, len, &len) == 0);
    for (size_t n = 0; n < len; ++n) {  // every truncation, each from a buffer of exactly that size
        uint8_t* t = malloc(n ? n : 1); memcpy(t, buf, n);
        fhe_seeded_server_key* x = NULL;
        CHECK(fhe_seeded_server_key_deserialize(t, n, &x) != 0 && !x);
        free(t);
    }
    for (size_t i = 0; i < len; ++i) {  // every single-byte corruption
        buf[i] ^= 0x80; fhe_seeded_server_key* x = NULL;
        CHECK(fhe_seeded_server_key_deserialize(buf, len, &x) != 0 && !x);
        buf[i] ^= 0x80;
    }
    for (int delta = -8; delta <= 8; delta += 16) {  // one word shorter / longer, header consistent
        const size_t m = len + delta;
        uint8_t* t = calloc(m, 1); memcpy(t, buf, m < len ? m : len);
        uint64_t plen = m - 32, h = fnv(t + 32, m - 32);
        memcpy(t + 16, &plen, 8); memcpy(t + 24, &h, 8);
        fhe_seeded_server_key* x = NULL;
        CHECK(fhe_seeded_server_key_deserialize(t, m, &x) == FHE_ERR_INVALID && !x && strstr(fhe_last_error(), "payload length"));
        free(t);
    }
    fhe_seeded_server_key* x = NULL; fhe_server_key* y = NULL; fhe_params q;
    CHECK(fhe_seeded_server_key_deserialize(NULL, 0, &x) != 0 && fhe_seeded_server_key_deserialize(buf, len, NULL) != 0);
    CHECK(fhe_server_key_generate_seeded(NULL, NULL, &x) != 0 && fhe_server_key_generate_seeded(ck, NULL, NULL) != 0);
    CHECK(fhe_seeded_server_key_expand_host(NULL, &y) != 0 && fhe_seeded_server_key_expand_host(s, NULL) != 0);
    CHECK(fhe_seeded_server_key_params(NULL, &q) != 0 && fhe_set_server_key_seeded(NULL, s) == FHE_ERR_INVALID);
    fhe_seeded_server_key_destroy(NULL);
    free(buf);
    fhe_seeded_server_key_destroy(s);
    fhe_client_key_destroy(ck);
    return 0;
}

int main(void) {
    if (one_set(16, 1) || one_set(16, 2) || reader()) return 1;
    printf("seeded server key host code: all checks passed\n");
    return 0;
}
