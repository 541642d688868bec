// threads_host_check.c -- stand-alone check of the threading contract (include/fhe_rocm.h, "Threading"): contexts
// are independent across host threads.  Its own main, pthreads, simulated contexts only (fhe_host_sim_ctx_create),
// no GPU call.  Threaded phase, first thing in the process so that every first use races: T threads, each with a
// simulated context and operands of its own (a fixed in-program generator seeded by the thread index), wait on a
// barrier and run one program that reaches the first use of every radix algorithm -- the encrypted shifts first.
// Each thread also causes one refusal of its own and reads fhe_last_error() after a second barrier.  Sequential
// phase: the main thread runs the same T programs on fresh contexts.  Every result is one text line; both sets are
// printed, and the exit status is 1 if a threaded line differs from its sequential line or a value from its
// host-side expected value (u64 arithmetic up to 64 bits, a limb loop for the pseudo-Mersenne remainder, the
// host fold fhe_host_biguint_mul for BigUintFHE).  Plain (each command one line):
//   make -C fhe-sign_amd
//   cc -O1 -pthread -Iinclude tools/threads_host_check.c -Lfhe-sign_amd/lib -lfhe_rocm
//      -Wl,-rpath,$PWD/fhe-sign_amd/lib -o threads_host_check
// Host ThreadSanitizer (tools/tsan_host.sh does this; clang = the ROCm toolchain's):
//   make -C fhe-sign_amd tsan
//   clang -g -O1 -pthread -fsanitize=thread -shared-libsan -Iinclude tools/threads_host_check.c
//         -Lfhe-sign_amd/lib_tsan -lfhe_rocm -Wl,-rpath,$PWD/fhe-sign_amd/lib_tsan
//         -Wl,-rpath,$(dirname $(clang -print-file-name=libclang_rt.tsan-x86_64.so)) -o threads_host_check
#include <inttypes.h>
#include <pthread.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "fhe_rocm.h"

#define T 4
#define BUF (64 * 1024)

typedef struct {
    int idx;
    pthread_barrier_t *start, *refused;  // NULL in the sequential phase
    uint64_t state;                      // splitmix64, seeded by idx
    fhe_ctx* c;
    int bad;  // a required case failed, or a value differs from its expected value
    size_t len;
    char buf[BUF];
} job;

static uint64_t rnd(job* j) {
    uint64_t z = (j->state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static uint64_t mask_of(uint32_t bits) { return bits == 64 ? ~0ull : (1ull << bits) - 1; }

static void emit(job* j, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    const int n = vsnprintf(j->buf + j->len, BUF - j->len, fmt, ap);
    va_end(ap);
    if (n < 0 || (size_t)n >= BUF - j->len)
        j->bad = 1;  // the buffer holds every line of the program with room to spare
    else
        j->len += (size_t)n;
}
static int ok(job* j, const char* name, int rc) {
    if (rc == FHE_OK) return 1;
    emit(j, "%s: rc=%d (%s)\n", name, rc, fhe_last_error());
    j->bad = 1;
    return 0;
}
static fhe_radix* enc(job* j, uint64_t v, uint32_t bits) {
    const uint64_t w[1] = {v};
    fhe_radix* x = NULL;
    ok(j, "encrypt", fhe_radix_encrypt(j->c, NULL, w, bits, &x));
    return x;
}
// decrypts r, writes its line and compares with the expected value; r is destroyed
static void check(job* j, const char* name, uint32_t bits, fhe_radix* r, uint64_t want) {
    uint64_t w[1] = {0};
    if (!r || !ok(j, name, fhe_radix_decrypt(j->c, NULL, r, w, 1))) {
        fhe_radix_destroy(r);
        return;
    }
    emit(j, "%s bits=%u = %016" PRIx64, name, bits, w[0]);
    if (w[0] != want) {
        emit(j, " EXPECTED %016" PRIx64, want);
        j->bad = 1;
    }
    emit(j, "\n");
    fhe_radix_destroy(r);
}

typedef int (*binop_fn)(fhe_ctx*, const fhe_radix*, const fhe_radix*, fhe_radix**);
static void binop(job* j, const char* name, binop_fn fn, uint32_t bits, const fhe_radix* x, const fhe_radix* y, uint64_t want) {
    fhe_radix* r = NULL;
    if (ok(j, name, fn(j->c, x, y, &r))) check(j, name, bits, r, want);
}

// the operands are made apart from the shifts: those of the first pair exist before the start barrier, so that
// the first call behind it is the shift itself
typedef struct {
    uint32_t bits;
    uint64_t xv, sv;
    fhe_radix *x, *amt;
} shift_args;
static shift_args shift_operands(job* j, uint32_t bits) {
    shift_args a = {bits, rnd(j) & mask_of(bits), rnd(j) & mask_of(bits), NULL, NULL};
    a.x = enc(j, a.xv, bits), a.amt = enc(j, a.sv, bits);
    return a;
}
static void shifts(job* j, shift_args a) {
    const uint32_t s = (uint32_t)(a.sv % a.bits);
    binop(j, "shl", fhe_radix_shl, a.bits, a.x, a.amt, (a.xv << s) & mask_of(a.bits));
    binop(j, "shr", fhe_radix_shr, a.bits, a.x, a.amt, a.xv >> s);
    fhe_radix_destroy(a.x), fhe_radix_destroy(a.amt);
}

static void arithmetic(job* j, uint32_t bits) {
    const uint64_t m = mask_of(bits), xv = rnd(j) & m;
    uint64_t yv = rnd(j) & m;
    if (bits > 8) yv >>= bits / 2;  // a quotient of several blocks
    if (yv == 0) yv = 3;
    fhe_radix *x = enc(j, xv, bits), *y = enc(j, yv, bits), *q = NULL, *r = NULL;
    binop(j, "add", fhe_radix_add, bits, x, y, (xv + yv) & m);
    binop(j, "sub", fhe_radix_sub, bits, x, y, (xv - yv) & m);
    binop(j, "mul", fhe_radix_mul, bits, x, y, (xv * yv) & m);
    binop(j, "bitand", fhe_radix_bitand, bits, x, y, xv & yv);
    binop(j, "min", fhe_radix_min, bits, x, y, xv < yv ? xv : yv);
    binop(j, "max", fhe_radix_max, bits, x, y, xv < yv ? yv : xv);
    binop(j, "lt", fhe_radix_lt, bits, x, y, xv < yv);
    binop(j, "div", fhe_radix_div, bits, x, y, xv / yv);
    binop(j, "rem", fhe_radix_rem, bits, x, y, xv % yv);
    if (ok(j, "divrem", fhe_radix_divrem(j->c, x, y, &q, &r))) {
        check(j, "divrem.q", bits, q, xv / yv);
        check(j, "divrem.r", bits, r, xv % yv);
    }
    fhe_radix_destroy(x), fhe_radix_destroy(y);
}

static void scalars(job* j) {
    const uint32_t bits = 34;
    const uint64_t m = mask_of(bits), xv = rnd(j) & m, d = (rnd(j) & 0xffff) | 0x101;
    const uint64_t mw[1] = {rnd(j) & m}, kw[1] = {rnd(j) & m};
    fhe_radix *x = enc(j, xv, bits), *r = NULL;
    if (ok(j, "scalar_div", fhe_radix_scalar_div(j->c, x, d, &r))) check(j, "scalar_div", bits, r, xv / d);
    r = NULL;
    if (ok(j, "scalar_rem", fhe_radix_scalar_rem(j->c, x, d, &r))) check(j, "scalar_rem", bits, r, xv % d);
    r = NULL;
    if (ok(j, "scalar_mul_add_words", fhe_radix_scalar_mul_add_words(j->c, x, mw, 1, kw, 1, &r)))
        check(j, "scalar_mul_add_words", bits, r, (xv * mw[0] + kw[0]) & m);
    r = NULL;
    if (ok(j, "cast", fhe_radix_cast(j->c, x, 16, &r))) check(j, "cast", 16, r, xv & 0xffff);
    r = NULL;
    if (ok(j, "cast", fhe_radix_cast(j->c, x, 50, &r))) check(j, "cast", 50, r, xv);
    fhe_radix_destroy(x);
}

static void mul64(job* j) {
    const uint64_t xv = rnd(j), yv = rnd(j);
    fhe_radix *x = enc(j, xv, 64), *y = enc(j, yv, 64);
    binop(j, "mul", fhe_radix_mul, 64, x, y, xv * yv);
    fhe_radix_destroy(x), fhe_radix_destroy(y);
}

// x mod (2^256 - c) of a 320-bit x, c of one word: x <- (x mod 2^256) + (x >> 256) c until x < 2^256, then one
// conditional subtraction (x >= p exactly where x + c carries out of 256 bits)
static void rem_secp(const uint64_t x[5], uint64_t c, uint64_t out[4]) {
    uint64_t s[5];
    memcpy(s, x, sizeof s);
    while (s[4]) {
        unsigned __int128 t = (unsigned __int128)s[4] * c;
        s[4] = 0;
        for (int i = 0; i < 5; ++i) {
            t += s[i];
            s[i] = (uint64_t)t;
            t >>= 64;
        }
    }
    uint64_t u[4];
    unsigned __int128 t = c;
    for (int i = 0; i < 4; ++i) {
        t += s[i];
        u[i] = (uint64_t)t;
        t >>= 64;
    }
    memcpy(out, t ? u : s, 4 * sizeof(uint64_t));
}
static void rem_pseudo_mersenne(job* j) {
    static const uint64_t kSecpC[1] = {0x1000003D1ull};  // secp256k1: p = 2^256 - 2^32 - 977
    uint64_t xw[5], want[4], got[4] = {0};
    for (int i = 0; i < 5; ++i) xw[i] = rnd(j);
    if (j->idx == 1)
        for (int i = 1; i < 4; ++i) xw[i] = ~0ull;  // the low 256 bits near 2^256: the folds carry into bit 256
    rem_secp(xw, kSecpC[0], want);
    fhe_radix *x = NULL, *r = NULL;
    if (ok(j, "encrypt", fhe_radix_encrypt(j->c, NULL, xw, 320, &x)) &&
        ok(j, "rem_pseudo_mersenne", fhe_radix_rem_pseudo_mersenne(j->c, x, 256, kSecpC, 1, &r)) &&
        ok(j, "rem_pseudo_mersenne", fhe_radix_decrypt(j->c, NULL, r, got, 4))) {
        emit(j, "rem_pseudo_mersenne bits=320 =");
        for (int i = 0; i < 4; ++i) emit(j, " %016" PRIx64, got[i]);
        if (memcmp(got, want, sizeof got)) {
            emit(j, " EXPECTED");
            for (int i = 0; i < 4; ++i) emit(j, " %016" PRIx64, want[i]);
            j->bad = 1;
        }
        emit(j, "\n");
    }
    fhe_radix_destroy(x), fhe_radix_destroy(r);
}

static void limbs_line(job* j, const char* name, size_t l, int mode, const fhe_biguint* v, const uint32_t* want, size_t nwant) {
    uint32_t got[32] = {0};
    size_t n = 0;
    if (!v || !ok(j, name, fhe_biguint_decrypt(j->c, NULL, v, got, 32, &n))) return;
    emit(j, "%s %zux%zu mode=%d n=%zu =", name, l, l, mode, n);
    for (size_t i = 0; i < n; ++i) emit(j, " %08" PRIx32, got[i]);
    if (n != nwant || memcmp(got, want, n * sizeof(uint32_t))) {
        emit(j, " EXPECTED n=%zu", nwant);
        for (size_t i = 0; i < nwant; ++i) emit(j, " %08" PRIx32, want[i]);
        j->bad = 1;
    }
    emit(j, "\n");
}
static void biguint(job* j) {
    static const size_t shapes[2] = {3, 8};
    for (int s = 0; s < 2; ++s)
        for (int mode = FHE_BIGUINT_COMPAT; mode <= FHE_BIGUINT_FAST; ++mode) {
            const size_t l = shapes[s];
            uint32_t a[8], b[8], k[8], want[32];
            size_t nwant = 0;
            for (size_t i = 0; i < l; ++i) a[i] = (uint32_t)rnd(j), b[i] = (uint32_t)rnd(j), k[i] = (uint32_t)rnd(j);
            a[l - 1] |= 1u << 31, b[l - 1] |= 1u << 31;
            fhe_biguint *A = NULL, *B = NULL, *K = NULL, *P = NULL, *S = NULL;
            ok(j, "biguint encrypt", fhe_biguint_encrypt(j->c, NULL, a, l, &A));
            ok(j, "biguint encrypt", fhe_biguint_encrypt(j->c, NULL, b, l, &B));
            ok(j, "biguint encrypt", fhe_biguint_encrypt(j->c, NULL, k, l, &K));
            if (A && B && K) {
                if (ok(j, "biguint_mul", fhe_biguint_mul(j->c, A, B, mode, &P)) &&
                    ok(j, "host_biguint_mul", fhe_host_biguint_mul(a, l, b, l, NULL, 0, mode, want, 32, &nwant)))
                    limbs_line(j, "biguint_mul", l, mode, P, want, nwant);
                if (ok(j, "biguint_mul_add", fhe_biguint_mul_add(j->c, A, B, K, mode, &S)) &&
                    ok(j, "host_biguint_mul", fhe_host_biguint_mul(a, l, b, l, k, l, mode, want, 32, &nwant)))
                    limbs_line(j, "biguint_mul_add", l, mode, S, want, nwant);
            }
            fhe_biguint_destroy(A), fhe_biguint_destroy(B), fhe_biguint_destroy(K), fhe_biguint_destroy(P), fhe_biguint_destroy(S);
        }
}

static void refusal(job* j) {
    const char* want = j->idx % 2 == 0 ? "division by zero" : "operands must have the same bit width";
    fhe_radix *x = enc(j, 0x5a, 8), *a10 = enc(j, 0x5a, 10), *r = NULL;
    const int rc = j->idx % 2 == 0 ? fhe_radix_scalar_div(j->c, x, 0, &r) : fhe_radix_add(j->c, x, a10, &r);
    if (j->refused) pthread_barrier_wait(j->refused);  // every thread's refusal has happened: each reads its own
    const char* msg = fhe_last_error();
    emit(j, "refusal rc=%d (%s)", rc, msg);
    if (rc == FHE_OK || !strstr(msg, want)) {
        emit(j, " EXPECTED (%s)", want);
        j->bad = 1;
    }
    emit(j, "\n");
    fhe_radix_destroy(x), fhe_radix_destroy(a10), fhe_radix_destroy(r);
}

static void* program(void* arg) {
    job* j = (job*)arg;
    j->state = 0x9E3779B97F4A7C15ull * (uint64_t)(j->idx + 1);
    const int made = ok(j, "sim_ctx create", fhe_host_sim_ctx_create(&j->c));
    shift_args first = {0};
    if (made) first = shift_operands(j, 32);
    if (j->start) pthread_barrier_wait(j->start);  // reached by every thread, with or without a context
    if (made) {
        shifts(j, first);
        shifts(j, shift_operands(j, 34));
        arithmetic(j, 8);
        arithmetic(j, 34);
        scalars(j);
        mul64(j);
        rem_pseudo_mersenne(j);
        biguint(j);
        uint64_t label = 0, merged = 0, above = 0, pbs = 0, levels = 0;
        if (ok(j, "noise audit", fhe_ctx_noise_audit(j->c, &label, &merged, &above, 1)) && ok(j, "stats", fhe_ctx_stats(j->c, &pbs, &levels)))
            emit(j, "audit max_label=%" PRIu64 " max_merged=%" PRIu64 " above_label=%" PRIu64 " pbs=%" PRIu64 " levels=%" PRIu64 "\n", label,
                 merged, above, pbs, levels);
    }
    if (made)
        refusal(j);
    else if (j->refused)
        pthread_barrier_wait(j->refused);
    fhe_ctx_destroy(j->c);
    j->c = NULL;
    return NULL;
}

int main(void) {
    static job threaded[T], sequential[T];
    pthread_barrier_t start, refused;
    pthread_t th[T];
    int failed = 0, started = 0;
    pthread_barrier_init(&start, NULL, T);
    pthread_barrier_init(&refused, NULL, T);
    for (int i = 0; i < T; ++i) {
        threaded[i].idx = sequential[i].idx = i;
        threaded[i].start = &start, threaded[i].refused = &refused;
    }
    for (int i = 0; i < T; ++i, ++started)
        if (pthread_create(&th[i], NULL, program, &threaded[i]) != 0) break;
    if (started < T) {  // the others wait on a barrier that never fills: nothing to join
        fprintf(stderr, "pthread_create failed\n");
        _Exit(2);
    }
    for (int i = 0; i < T; ++i) pthread_join(th[i], NULL);
    for (int i = 0; i < T; ++i) program(&sequential[i]);
    for (int i = 0; i < T; ++i) {
        const char *a = threaded[i].buf, *b = sequential[i].buf;
        while (*a || *b) {  // line by line, each under its phase and thread
            const size_t la = strcspn(a, "\n"), lb = strcspn(b, "\n");
            const int same = la == lb && !memcmp(a, b, la);
            printf("threaded   %d: %.*s\nsequential %d: %.*s%s\n", i, (int)la, a, i, (int)lb, b, same ? "" : "   <-- DIFFER");
            if (!same) failed = 1;
            a += la + (a[la] == '\n'), b += lb + (b[lb] == '\n');
        }
        if (threaded[i].bad || sequential[i].bad) failed = 1;
    }
    printf(failed ? "threaded host check: FAILED\n" : "threaded host check: ok\n");
    return failed;
}
