// seeded_host_check.c -- stand-alone driver of the seeded form's host code (encryption, wire format,
// host expansion; no GPU call), for a host AddressSanitizer + UndefinedBehaviorSanitizer run with its own
// main:
//   make -C fhe-sign_amd asan
//   clang -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -shared-libsan -Iinclude \
//         tools/seeded_host_check.c -Lfhe-sign_amd/lib_asan -lfhe_rocm -Wl,-rpath,$PWD/fhe-sign_amd/lib_asan -o seeded_host_check
// (clang = the ROCm toolchain's, so that the sanitizer runtime matches the library's).  It round-trips radix
// objects of 1 to 2048 blocks and BigUintFHE objects of 0 to 9 limbs, decrypts every expanded block, and
// feeds the reader every truncation, every single-byte corruption and every form / count pair around the
// edges with the checksum recomputed.
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

int main(void) {
    fhe_params p;
    fhe_params_default(&p);
    p.lwe_dimension = 16;
    fhe_client_key* ck; fhe_server_key* sk;
    CHECK(fhe_generate_keys(&p, 7, &ck, &sk) == 0);
    uint8_t seed[32]; for (int i = 0; i < 32; ++i) seed[i] = (uint8_t)(i * 7 + 1);
    uint64_t words[64]; for (int i = 0; i < 64; ++i) words[i] = 0x9E3779B97F4A7C15ull * (i + 1);
    uint32_t bitsv[] = {2, 4, 10, 32, 256, 4096};
    for (unsigned k = 0; k < 6; ++k) {
        fhe_seeded* s = NULL;
        CHECK(fhe_radix_encrypt_seeded(ck, words, bitsv[k], k & 1 ? seed : NULL, &s) == 0);
        size_t nb = 0, len = 0; uint32_t form, count;
        CHECK(fhe_seeded_info(s, &form, &count, &nb) == 0 && nb == bitsv[k] / 2 && count == bitsv[k] && form == 0);
        CHECK(fhe_seeded_serialize(s, NULL, 0, &len) == 0 && len == 108 + 8 * nb);
        uint8_t* buf = malloc(len);
        CHECK(fhe_seeded_serialize(s, buf, len, &len) == 0);
        CHECK(fhe_seeded_serialize(s, buf, len - 1, &len) == FHE_ERR_INVALID);
        fhe_seeded* d = NULL;
        CHECK(fhe_seeded_deserialize(buf, len, &d) == 0);
        uint64_t* a = malloc(nb * 2049 * 8); uint64_t* b = malloc(nb * 2049 * 8);
        CHECK(fhe_seeded_expand_host(s, a, nb * 2049) == 0 && fhe_seeded_expand_host(d, b, nb * 2049) == 0);
        CHECK(memcmp(a, b, nb * 2049 * 8) == 0);
        CHECK(fhe_seeded_expand_host(s, a, nb * 2049 - 1) == FHE_ERR_INVALID);
        for (size_t i = 0; i < nb; ++i) {
            uint64_t v;
            CHECK(fhe_decrypt_block(ck, a + i * 2049, &v) == 0);
            CHECK(v == ((words[(2 * i) / 64] >> ((2 * i) % 64)) & 3));
        }
        if (len < 400) {
            for (size_t n = 0; n < len; ++n) { fhe_seeded* x = NULL; CHECK(fhe_seeded_deserialize(buf, n, &x) != 0 && !x); }
            for (size_t i = 0; i < len; ++i) {
                buf[i] ^= 0x80; fhe_seeded* x = NULL; CHECK(fhe_seeded_deserialize(buf, len, &x) != 0 && !x); buf[i] ^= 0x80;
            }
            // every form / count pair around the edges, checksum recomputed
            uint32_t forms[] = {0, 1, 2, 0xFFFFFFFFu};
            uint32_t counts[] = {0, 1, 2, 3, (uint32_t)bitsv[k], 4096, 4098, 1u << 20, (1u << 20) + 1, 0xFFFFFFFFu};
            for (int f = 0; f < 4; ++f) for (int c = 0; c < 10; ++c) {
                uint8_t* t = malloc(len); memcpy(t, buf, len);
                memcpy(t + 32 + 36, &forms[f], 4); memcpy(t + 32 + 40, &counts[c], 4);
                uint64_t h = fnv(t + 32, len - 32); memcpy(t + 24, &h, 8);
                fhe_seeded* x = NULL;
                int rc = fhe_seeded_deserialize(t, len, &x);
                size_t want = forms[f] == 0 ? counts[c] / 2 : (size_t)counts[c] * 16;
                int ok = forms[f] <= 1 && want == nb && !(forms[f] == 0 && (counts[c] % 2 || counts[c] < 2 || counts[c] > 4096));
                CHECK((rc == 0) == ok);
                fhe_seeded_destroy(x); free(t);
            }
        }
        free(a); free(b); free(buf);
        fhe_seeded_destroy(s); fhe_seeded_destroy(d);
    }
    for (size_t nl = 0; nl <= 9; nl += 3) {
        uint32_t limbs[9]; for (int i = 0; i < 9; ++i) limbs[i] = 0xDEADBEEFu + 977u * i;
        fhe_seeded* s = NULL;
        CHECK(fhe_biguint_encrypt_seeded(ck, nl ? limbs : NULL, nl, seed, &s) == 0);
        size_t nb, len; CHECK(fhe_seeded_info(s, NULL, NULL, &nb) == 0 && nb == 16 * nl);
        uint64_t* a = malloc(nb * 2049 * 8 + 8);
        CHECK(fhe_seeded_expand_host(s, a, nb * 2049) == 0);
        CHECK(fhe_seeded_serialize(s, NULL, 0, &len) == 0);
        free(a); fhe_seeded_destroy(s);
    }
    fhe_seeded* s = NULL;
    CHECK(fhe_biguint_encrypt_seeded(ck, (uint32_t*)words, ((size_t)1 << 20) + 1, seed, &s) == FHE_ERR_INVALID);
    CHECK(fhe_radix_encrypt_seeded(ck, words, 3, seed, &s) == FHE_ERR_INVALID);
    CHECK(fhe_radix_encrypt_seeded(ck, words, 4098, seed, &s) == FHE_ERR_INVALID);
    CHECK(fhe_seeded_expand_radix(NULL, NULL, NULL) != 0);
    fhe_client_key_destroy(ck); fhe_server_key_destroy(sk);
    printf("seeded host code: all checks passed\n");
    return 0;
}
