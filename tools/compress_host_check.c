// compress_host_check.c -- stand-alone driver of the host code of the compressed computed ciphertexts (key
// generation, the packing keyswitch's host definition, the three wire kinds, direct decryption; no GPU
// call), for a host AddressSanitizer + UndefinedBehaviorSanitizer run with its own main:
//   make -C fhe-sign_amd asan
//   clang -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -shared-libsan -Iinclude \
//         tools/compress_host_check.c -Lfhe-sign_amd/lib_asan -lfhe_rocm -Wl,-rpath,$PWD/fhe-sign_amd/lib_asan -o compress_host_check
// (clang = the ROCm toolchain's, as for tools/seeded_key_host_check.c).  At (k', N', L, beta, ell) = (1, 8, 8,
// 4, 4) and (2, 16, 16, 3, 5) under a main key of n = 16 it generates the keys, compresses 1, L and 2 L + 3
// blocks holding all 16 values, decrypts them directly, round-trips the three kinds, and feeds every reader
// every truncation and every single-byte corruption (the 1.5 MB compression key: every byte of its first
// 512 and every 4099th after, each corruption costing a checksum over the whole key), payloads one word
// longer and shorter with the checksum recomputed, and every kind to every other reader.
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
static int rd_priv(const uint8_t* b, size_t n, void** o) { return fhe_compression_private_key_deserialize(b, n, (fhe_compression_private_key**)o); }
static int rd_key(const uint8_t* b, size_t n, void** o) { return fhe_compression_key_deserialize(b, n, (fhe_compression_key**)o); }
static int rd_list(const uint8_t* b, size_t n, void** o) { return fhe_compressed_deserialize(b, n, (fhe_compressed_list**)o); }

// every truncation, corruptions at `step` beyond the first 512 bytes, one word longer / shorter
static int torture(reader_fn rd, uint8_t* buf, size_t len, size_t step) {
    for (size_t n = 0; n < len; n += (n < 512 || len - n < 64) ? 1 : step) {  // each from a buffer of exactly that size
        uint8_t* t = malloc(n ? n : 1); memcpy(t, buf, n);
        void* x = NULL;
        CHECK(rd(t, n, &x) != 0 && !x);
        free(t);
    }
    for (size_t i = 0; i < len; i += (i < 512 || len - i < 64) ? 1 : step) {
        buf[i] ^= 0x80; void* x = NULL;
        CHECK(rd(buf, len, &x) != 0 && !x);
        buf[i] ^= 0x80;
    }
    for (int delta = -8; delta <= 8; delta += 16) {
        const size_t m = len + delta;
        uint8_t* t = calloc(m, 1); memcpy(t, buf, m < len ? m : len);
        uint64_t plen = m - 32, h = fnv(t + 32, m - 32);
        memcpy(t + 16, &plen, 8); memcpy(t + 24, &h, 8);
        void* x = NULL;
        CHECK(rd(t, m, &x) == FHE_ERR_INVALID && !x);
        free(t);
    }
    void* x = NULL;
    CHECK(rd(NULL, 0, &x) != 0 && rd(buf, len, NULL) != 0);
    return 0;
}

static int one_set(const fhe_compression_params* cp) {
    fhe_params p;
    fhe_params_default(&p);
    p.lwe_dimension = 16;
    fhe_client_key* ck; fhe_server_key* unused;
    CHECK(fhe_generate_keys(&p, 11, &ck, &unused) == 0);
    fhe_server_key_destroy(unused);
    fhe_compression_private_key* priv = NULL; fhe_compression_key* key = NULL;
    CHECK(fhe_compression_keys_generate(ck, cp, &priv, &key) == 0);
    fhe_params mp; fhe_compression_params q;
    CHECK(fhe_compression_key_params(key, &mp, &q) == 0 && mp.lwe_dimension == 16 && memcmp(&q, cp, sizeof q) == 0);
    CHECK(fhe_compression_private_key_params(priv, &mp, &q) == 0 && mp.lwe_dimension == 16 && memcmp(&q, cp, sizeof q) == 0);
    const uint32_t kn = cp->glwe_dimension * cp->polynomial_size, L = cp->lwe_per_glwe;
    const size_t pw = (size_t)2048 * cp->pks_level * (cp->glwe_dimension + 1) * cp->polynomial_size, bw = (size_t)kn * 4 * 2048;
    uint64_t *pk = malloc(pw * 8), *bk = malloc(bw * 8), *sk = malloc(kn * 8);
    CHECK(fhe_compression_key_export(key, pk, pw, bk, bw) == 0 && fhe_compression_key_export(key, pk, pw - 1, NULL, 0) != 0);
    CHECK(fhe_compression_private_key_export(priv, sk, kn) == 0 && fhe_compression_private_key_export(priv, sk, kn - 1) != 0);
    for (uint32_t i = 0; i < kn; ++i) CHECK(sk[i] <= 1);

    // the three serialized kinds
    size_t plen = 0, klen = 0;
    CHECK(fhe_compression_private_key_serialize(priv, NULL, 0, &plen) == 0 && plen == 96 + 8 * (size_t)kn);
    CHECK(fhe_compression_key_serialize(key, NULL, 0, &klen) == 0 && klen == 96 + 8 * (pw + bw));
    uint8_t *pbuf = malloc(plen), *kbuf = malloc(klen);
    CHECK(fhe_compression_private_key_serialize(priv, pbuf, plen, &plen) == 0 && fhe_compression_key_serialize(key, kbuf, klen, &klen) == 0);
    CHECK(fhe_compression_key_serialize(key, kbuf, klen - 1, &klen) == FHE_ERR_INVALID);
    fhe_compression_private_key* priv2 = NULL; fhe_compression_key* key2 = NULL;
    CHECK(fhe_compression_private_key_deserialize(pbuf, plen, &priv2) == 0 && fhe_compression_key_deserialize(kbuf, klen, &key2) == 0);

    const size_t counts[3] = {1, L, 2 * (size_t)L + 3};
    uint8_t* lbuf = NULL; size_t llen = 0;
    for (int c = 0; c < 3; ++c) {
        const size_t B = counts[c];
        uint64_t *vals = malloc(B * 8), *cts = malloc(B * 2049 * 8);
        uint8_t* deg = malloc(B);
        for (size_t i = 0; i < B; ++i) { vals[i] = (5 * i + 3) % 16; deg[i] = 15; }
        CHECK(fhe_encrypt_blocks(ck, vals, B, cts) == 0);
        fhe_compressed_list *x = NULL, *y = NULL, *z = NULL;
        CHECK(fhe_compress_host(key, cts, B, deg, FHE_SEEDED_RADIX, (uint32_t)(2 * B), &x) == 0);
        CHECK(fhe_compress_host(key2, cts, B, deg, FHE_SEEDED_RADIX, (uint32_t)(2 * B), &y) == 0);  // the key that travelled
        uint32_t form, count; size_t nb;
        CHECK(fhe_compressed_info(x, &form, &count, &nb) == 0 && form == FHE_SEEDED_RADIX && count == 2 * B && nb == B);
        CHECK(fhe_compressed_params(x, &mp, &q) == 0 && memcmp(&q, cp, sizeof q) == 0);
        size_t want = 108 + B;
        for (size_t g = 0; g * L < B; ++g) want += (12 * (kn + (B - g * L < L ? B - g * L : L)) + 7) / 8;
        size_t len = 0, len2 = 0;
        CHECK(fhe_compressed_serialize(x, NULL, 0, &len) == 0 && len == want);
        uint8_t *buf = malloc(len), *buf2 = malloc(len);
        CHECK(fhe_compressed_serialize(x, buf, len, &len) == 0 && fhe_compressed_serialize(y, buf2, len, &len2) == 0);
        CHECK(len2 == len && memcmp(buf, buf2, len) == 0);
        CHECK(fhe_compressed_deserialize(buf, len, &z) == 0);
        // direct decryption, with both private keys: sum v_i 4^i mod 2^(2 B)
        const size_t nw = (2 * B + 63) / 64;
        uint64_t *w = calloc(nw + 1, 8), *w2 = calloc(nw + 1, 8), *ref = calloc(nw + 2, 8);
        for (size_t i = 0; i < B; ++i) {  // add v << 2 i with carries
            unsigned __int128 add = (unsigned __int128)vals[i] << ((2 * i) % 64);
            for (size_t k = 2 * i / 64; k < nw + 2 && add; ++k) {
                unsigned __int128 s = (unsigned __int128)ref[k] + (uint64_t)add;
                ref[k] = (uint64_t)s; add = (add >> 64) + (s >> 64);
            }
        }
        if ((2 * B) % 64) ref[nw - 1] &= ((uint64_t)1 << ((2 * B) % 64)) - 1;
        CHECK(fhe_compressed_decrypt(priv, z, w, nw) == 0 && fhe_compressed_decrypt(priv2, x, w2, nw) == 0);
        CHECK(memcmp(w, ref, nw * 8) == 0 && memcmp(w2, ref, nw * 8) == 0);
        CHECK(fhe_compressed_decrypt(priv, z, w, nw - 1) == FHE_ERR_INVALID || nw == 1);
        deg[B - 1] = 16;
        fhe_compressed_list* bad = NULL;
        CHECK(fhe_compress_host(key, cts, B, deg, FHE_SEEDED_RADIX, (uint32_t)(2 * B), &bad) == FHE_ERR_INVALID && !bad);
        CHECK(fhe_compress_host(key, cts, B, deg, FHE_SEEDED_RADIX, (uint32_t)(2 * B + 2), &bad) == FHE_ERR_INVALID && !bad);
        if (c == 2) { lbuf = buf; llen = len; } else free(buf);
        free(buf2); free(w); free(w2); free(ref); free(vals); free(cts); free(deg);
        fhe_compressed_destroy(x); fhe_compressed_destroy(y); fhe_compressed_destroy(z);
    }
    // every kind to every other reader
    void* o = NULL;
    CHECK(rd_priv(kbuf, klen, &o) != 0 && !o && strstr(fhe_last_error(), "kind"));
    CHECK(rd_priv(lbuf, llen, &o) != 0 && !o && rd_key(pbuf, plen, &o) != 0 && !o && rd_key(lbuf, llen, &o) != 0 && !o);
    CHECK(rd_list(pbuf, plen, &o) != 0 && !o && rd_list(kbuf, klen, &o) != 0 && !o);
    fhe_client_key* nock = NULL;
    CHECK(fhe_client_key_deserialize(lbuf, llen, &nock) != 0 && !nock);
    if (torture(rd_list, lbuf, llen, 1) || torture(rd_priv, pbuf, plen, 1) || torture(rd_key, kbuf, klen, 4099)) return 1;
    // a degree byte >= 16 with the checksum recomputed
    lbuf[108] = 16;
    uint64_t h = fnv(lbuf + 32, llen - 32); memcpy(lbuf + 24, &h, 8);
    CHECK(rd_list(lbuf, llen, &o) == FHE_ERR_INVALID && !o && strstr(fhe_last_error(), "degree"));
    free(lbuf); free(pbuf); free(kbuf); free(pk); free(bk); free(sk);
    fhe_compression_private_key_destroy(priv); fhe_compression_private_key_destroy(priv2);
    fhe_compression_key_destroy(key); fhe_compression_key_destroy(key2);
    fhe_client_key_destroy(ck);
    return 0;
}

static int ranges(void) {
    fhe_params p;
    fhe_params_default(&p);
    p.lwe_dimension = 1;
    fhe_client_key* ck; fhe_server_key* unused;
    CHECK(fhe_generate_keys(&p, 12, &ck, &unused) == 0);
    fhe_server_key_destroy(unused);
    fhe_compression_params d;
    CHECK(fhe_compression_params_default(&d) == 0 && d.glwe_dimension == 4 && d.polynomial_size == 256 && d.storage_log_modulus == 12);
    const fhe_compression_params bad[] = {{4, 100, 64, 4, 4, 42, 12}, {4, 4, 4, 4, 4, 42, 12}, {0, 256, 256, 4, 4, 42, 12},
                                          {9, 128, 128, 4, 4, 42, 12}, {4, 1024, 256, 4, 4, 42, 12}, {4, 256, 0, 4, 4, 42, 12},
                                          {4, 256, 257, 4, 4, 42, 12}, {4, 256, 256, 8, 4, 42, 12}, {4, 256, 256, 0, 4, 42, 12},
                                          {4, 256, 256, 4, 9, 42, 12}, {4, 256, 256, 4, 0, 42, 12}, {4, 256, 256, 4, 4, 63, 12},
                                          {4, 256, 256, 4, 4, 42, 11}, {4, 256, 256, 4, 4, 42, 13}};
    for (size_t i = 0; i < sizeof bad / sizeof bad[0]; ++i) {
        fhe_compression_private_key* a = NULL; fhe_compression_key* b = NULL;
        CHECK(fhe_compression_keys_generate(ck, &bad[i], &a, &b) == FHE_ERR_UNSUPPORTED && !a && !b);
    }
    fhe_compression_private_key* a = NULL; fhe_compression_key* b = NULL;
    CHECK(fhe_compression_keys_generate(NULL, &d, &a, &b) != 0 && fhe_compression_keys_generate(ck, &d, NULL, &b) != 0);
    CHECK(fhe_set_compression_key(NULL, NULL) == FHE_ERR_INVALID);
    fhe_compression_private_key_destroy(NULL); fhe_compression_key_destroy(NULL); fhe_compressed_destroy(NULL);
    fhe_client_key_destroy(ck);
    return 0;
}

int main(void) {
    const fhe_compression_params a = {1, 8, 8, 4, 4, 42, 12}, b = {2, 16, 16, 3, 5, 42, 12};
    if (one_set(&a) || one_set(&b) || ranges()) return 1;
    printf("compressed computed ciphertexts, host code: all checks passed\n");
    return 0;
}
