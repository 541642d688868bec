// faults_host_check.c -- stand-alone check of what a failed call leaves behind (include/fhe_rocm.h, "Errors after
// validation"), through the C ABI alone: its own main, one simulated context (fhe_host_sim_ctx_create), no GPU call.
// Each program is run once with every fault site enabled and no fault armed (FHE_TUNE_FAULT_SITES = 31,
// FHE_TUNE_FAULT_AFTER = 0), which gives its crossing count C; then once per k -- every k when C <= 48, else the
// first 16, the last 16 and 16 evenly spaced -- with the k-th crossing armed.  A call that returns FHE_ERR_HIP with
// "injected fault" is made again with the same arguments, and the program runs to its end.  Required of every run:
// exactly one injected error (none in the clean run), every decrypted value equal to its expected value (u64
// arithmetic; the host fold fhe_host_biguint_mul for BigUintFHE), and fhe_ctx_pending_info all zero after the
// final flush.  Programs: a 34-bit a * b + c and an 8-bit encrypted division, on demand and in slices of 7 levels;
// the BigUintFHE call site p = a * b (held), t = p + k, decrypt(t) -- a partial flush -- then decrypt(p), at 2 and
// 3 limbs, compat and fast.  Exit status 1 on a wrong value or a missing or extra error.  Plain (one line each):
//   make -C fhe-sign_amd
//   cc -O1 -Iinclude tools/faults_host_check.c -Lfhe-sign_amd/lib -lfhe_rocm
//      -Wl,-rpath,$PWD/fhe-sign_amd/lib -o faults_host_check
// Host AddressSanitizer + UBSan: tools/asan_faults_host.sh (the `make -C fhe-sign_amd asan` library; the program
// links the sanitizer runtime itself, nothing is preloaded).
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "fhe_rocm.h"

static fhe_ctx* ctx;
static int injected;  // injected errors met by the current run
static int bad;       // a wrong value, an unexpected status

// a call that fails with the injected fault is counted and made again, as it was
#define CALL(expr)                                                                        \
    do {                                                                                  \
        int rc_ = (expr);                                                                 \
        if (rc_ == FHE_ERR_HIP && strstr(fhe_last_error(), "injected fault")) {           \
            ++injected;                                                                   \
            rc_ = (expr);                                                                 \
        }                                                                                 \
        if (rc_ != FHE_OK) {                                                              \
            printf("%s: rc=%d (%s)\n", #expr, rc_, fhe_last_error());                     \
            bad = 1;                                                                      \
        }                                                                                 \
    } while (0)

static void want_u64(const char* what, uint64_t got, uint64_t want) {
    if (got != want) {
        printf("%s: %016" PRIx64 " EXPECTED %016" PRIx64 "\n", what, got, want);
        bad = 1;
    }
}

static fhe_radix* enc(uint64_t v, uint32_t bits) {
    const uint64_t w[1] = {v};
    fhe_radix* x = NULL;
    CALL(fhe_radix_encrypt(ctx, NULL, w, bits, &x));
    return x;
}

static uint64_t dec(const fhe_radix* x) {
    uint64_t w[1] = {0};
    if (x) CALL(fhe_radix_decrypt(ctx, NULL, x, w, 1));
    return w[0];
}

static void program_radix(int unused) {
    (void)unused;
    const uint32_t bits = 34;
    const uint64_t m = (1ull << bits) - 1, xv = 0x2B7C9D3A5ull, yv = 0x19E3Bull, zv = 0x3FFFFFFFFull;
    fhe_radix *x = enc(xv, bits), *y = enc(yv, bits), *z = enc(zv, bits), *p = NULL, *s = NULL, *q = NULL, *r = NULL;
    if (x && y && z) {
        CALL(fhe_radix_mul(ctx, x, y, &p));
        if (p) CALL(fhe_radix_add(ctx, p, z, &s));
        want_u64("a * b + c", dec(s), (xv * yv + zv) & m);
        want_u64("a * b", dec(p), (xv * yv) & m);
    }
    fhe_radix *u = enc(0xE7, 8), *v = enc(0x0B, 8);
    if (u && v) CALL(fhe_radix_divrem(ctx, u, v, &q, &r));
    want_u64("q", dec(q), 0xE7 / 0x0B);
    want_u64("r", dec(r), 0xE7 % 0x0B);
    fhe_radix* all[] = {x, y, z, p, s, q, r, u, v};
    for (size_t i = 0; i < sizeof all / sizeof *all; ++i) fhe_radix_destroy(all[i]);
}

// operands and expected limbs of the call site, made before the fault point is armed (the host fold records too)
static int g_limbs, g_mode;
static uint32_t a[3], b[3], k[3], want_p[8], want_t[8];
static size_t np, nt;
static void prepare_call_site(void) {
    const size_t n = (size_t)g_limbs;
    uint64_t st = 0x9E3779B97F4A7C15ull * (uint64_t)(n + 7 * g_mode);
    for (size_t i = 0; i < n; ++i) {
        st = st * 6364136223846793005ull + 1442695040888963407ull;
        a[i] = (uint32_t)(st >> 32) | 0x80000000u;
        st = st * 6364136223846793005ull + 1442695040888963407ull;
        b[i] = (uint32_t)(st >> 32) | 1u;
        st = st * 6364136223846793005ull + 1442695040888963407ull;
        k[i] = (uint32_t)(st >> 32) | 1u;
    }
    np = nt = 0;
    if (fhe_host_biguint_mul(a, n, b, n, NULL, 0, g_mode, want_p, 8, &np) ||
        fhe_host_biguint_mul(a, n, b, n, k, n, g_mode, want_t, 8, &nt)) {
        printf("host fold: %s\n", fhe_last_error());
        bad = 1;
    }
}

static void program_call_site(int unused) {
    (void)unused;
    const size_t n = (size_t)g_limbs;
    uint32_t got[8];
    size_t ng = 0;
    fhe_biguint *A = NULL, *B = NULL, *K = NULL, *P = NULL, *S = NULL;
    CALL(fhe_biguint_encrypt(ctx, NULL, a, n, &A));
    CALL(fhe_biguint_encrypt(ctx, NULL, b, n, &B));
    CALL(fhe_biguint_encrypt(ctx, NULL, k, n, &K));
    if (A && B && K) {
        CALL(fhe_biguint_mul(ctx, A, B, g_mode, &P));
        if (P) CALL(fhe_biguint_add(ctx, K, P, g_mode, &S));
    }
    // the value of a limb vector: compat gives the reference's limbs one for one, fast the true value, whose limb
    // count is the op's own -- compare limb by limb over the longer, missing limbs as zero
    for (int pass = 0; pass < 2 && P && S; ++pass) {
        const fhe_biguint* h = pass == 0 ? S : P;  // decrypt(t) first: the partial flush
        const uint32_t* want = pass == 0 ? want_t : want_p;
        const size_t nw = pass == 0 ? nt : np;
        memset(got, 0, sizeof got);
        ng = 0;
        CALL(fhe_biguint_decrypt(ctx, NULL, h, got, 8, &ng));
        for (size_t i = 0; i < 8; ++i)
            want_u64(pass == 0 ? "t limb" : "p limb", i < ng ? got[i] : 0, i < nw ? want[i] : 0);
    }
    fhe_biguint* all[] = {A, B, K, P, S};
    for (size_t i = 0; i < sizeof all / sizeof *all; ++i) fhe_biguint_destroy(all[i]);
}

// one run with the k-th crossing armed (0: none); returns the crossings counted
static int64_t run(void (*program)(int), int64_t k) {
    int64_t crossings = 0;
    injected = 0;
    fhe_host_set_tuning(FHE_TUNE_FAULT_SITES, 31, NULL);
    fhe_host_set_tuning(FHE_TUNE_FAULT_AFTER, k, NULL);
    program(0);
    // the final flush: every handle of the program is gone, what they left pending is swept as dead
    fhe_radix *x = enc(1, 4), *y = NULL;
    if (x) CALL(fhe_radix_add(ctx, x, x, &y));
    want_u64("final flush", dec(y), 2);
    fhe_radix_destroy(x), fhe_radix_destroy(y);
    fhe_host_set_tuning(FHE_TUNE_FAULT_AFTER, 0, &crossings);
    fhe_host_set_tuning(FHE_TUNE_FAULT_SITES, 0, NULL);
    uint64_t info[3] = {9, 9, 9};
    if (fhe_ctx_pending_info(ctx, info) || info[0] || info[1] || info[2]) {
        printf("pending_info after the final flush: %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", info[0], info[1], info[2]);
        bad = 1;
    }
    return crossings;
}

static int sweep(const char* name, void (*program)(int)) {
    const int bad0 = bad;
    const int64_t count = run(program, 0);
    if (injected != 0 || count < 2) {
        printf("%s: clean run: %d injected errors, %" PRId64 " crossings\n", name, injected, count);
        bad = 1;
        return 0;
    }
    int runs = 0;
    for (int64_t i = 1; i <= (count <= 48 ? count : 48); ++i) {
        int64_t k = i;
        if (count > 48) k = i <= 16 ? i : i <= 32 ? 16 + ((i - 17) * (count - 32)) / 16 + 1 : count - 48 + i;
        run(program, k);
        ++runs;
        if (injected != 1) {
            printf("%s: k = %" PRId64 " of %" PRId64 ": %d injected errors, expected exactly one\n", name, k, count, injected);
            bad = 1;
        }
    }
    printf("%s: %" PRId64 " crossings, %d failed-and-retried runs%s\n", name, count, runs, bad == bad0 ? "" : " -- FAILED");
    return runs;
}

int main(void) {
    if (fhe_host_sim_ctx_create(&ctx)) {
        printf("fhe_host_sim_ctx_create: %s\n", fhe_last_error());
        return 1;
    }
    int64_t depth = 0;
    fhe_host_set_tuning(FHE_TUNE_FLUSH_DEPTH, 0, &depth);
    sweep("radix ops, flush on demand", program_radix);
    fhe_host_set_tuning(FHE_TUNE_FLUSH_DEPTH, 7, NULL);
    sweep("radix ops, slices of 7 levels", program_radix);
    fhe_host_set_tuning(FHE_TUNE_FLUSH_DEPTH, depth, NULL);
    for (g_limbs = 2; g_limbs <= 3; ++g_limbs)
        for (g_mode = 0; g_mode <= 1; ++g_mode) {
            char name[64];
            snprintf(name, sizeof name, "BigUintFHE call site, %d limbs, mode %d", g_limbs, g_mode);
            prepare_call_site();
            sweep(name, program_call_site);
        }
    fhe_ctx_destroy(ctx);
    printf(bad ? "faults host check: FAILED\n" : "faults host check: ok\n");
    return bad ? 1 : 0;
}
