// engine_host_check.c -- stand-alone driver of the engine's host modes (dry, simulated and host-fold runs of the
// radix and BigUintFHE algorithms, the level scheduler; no GPU call), with its own main.  It prints one line per
// case: the dry schedules (bootstraps, levels, an FNV-1a of the level sizes), the recording-order fingerprints
// where a hook returns one, and the simulated results on inputs from a fixed in-program generator.  Two builds of
// the library record the same graphs in the same order iff the outputs are equal line for line (the fingerprint
// covers LUT ids, coefficients, constants and producers of every node in level order).  Plain (each command one
// line):
//   make -C fhe-sign_amd
//   cc -O1 -Iinclude tools/engine_host_check.c -Lfhe-sign_amd/lib -lfhe_rocm
//      -Wl,-rpath,$PWD/fhe-sign_amd/lib -o engine_host_check
// Host AddressSanitizer + UndefinedBehaviorSanitizer:
//   make -C fhe-sign_amd asan
//   clang -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -shared-libsan -Iinclude
//         tools/engine_host_check.c -Lfhe-sign_amd/lib_asan -lfhe_rocm -Wl,-rpath,$PWD/fhe-sign_amd/lib_asan
//         -Wl,-rpath,$(dirname $(clang -print-file-name=libclang_rt.asan-x86_64.so)) -o engine_host_check
// (clang = the ROCm toolchain's, as for tools/oprf_host_check.c).  A refused case prints its status and message,
// which are compared like any other line; the exit status is 1 only if a case that must succeed did not, or an
// ownership case (the "owner" lines, last) that must be refused was accepted.
#include <inttypes.h>
#include <stdio.h>
#include <string.h>
#include "fhe_rocm.h"

#define CAP 8192
static uint32_t g_sizes[CAP];
static int g_failed = 0;

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd(void) {  // splitmix64
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static void limbs(uint32_t* v, size_t n) {
    for (size_t i = 0; i < n; ++i) v[i] = (uint32_t)rnd();
}

static uint64_t fnv_sizes(uint64_t levels) {
    uint64_t x = 1469598103934665603ull;
    for (uint64_t i = 0; i < levels && i < CAP; ++i) x = (x ^ g_sizes[i]) * 1099511628211ull;
    return x;
}
// the status of a case: "ok", or the code and the message (a case that must succeed counts as failed)
static int status(const char* name, int rc, int must) {
    if (rc == FHE_OK) return 1;
    printf("%s rc=%d (%s)\n", name, rc, fhe_last_error());
    if (must) g_failed = 1;
    return 0;
}
static void words_out(const uint64_t* w, size_t n) {
    for (size_t i = 0; i < n; ++i) printf(" %016" PRIx64, w[i]);
}
static void limbs_out(const uint32_t* v, size_t n) {
    for (size_t i = 0; i < n; ++i) printf(" %08" PRIx32, v[i]);
}

static const uint64_t kSecpC[1] = {0x1000003D1ull};  // secp256k1: p = 2^256 - 2^32 - 977
static const size_t kShapes[4][3] = {{8, 8, 0}, {2, 8, 0}, {8, 12, 0}, {8, 1, 8}};

static void radix_stats(void) {
    const uint32_t widths[2] = {32, 256};
    for (int op = 0; op <= 6; ++op)
        for (int w = 0; w < 2; ++w) {
            char name[64];
            snprintf(name, sizeof name, "radix_stats op=%d bits=%u", op, widths[w]);
            uint64_t pbs = 0, levels = 0;
            memset(g_sizes, 0, sizeof g_sizes);
            if (!status(name, fhe_host_radix_stats(op, widths[w], &pbs, &levels, g_sizes, CAP), 1)) continue;
            printf("%s pbs=%" PRIu64 " levels=%" PRIu64 " sizes=%016" PRIx64 "\n", name, pbs, levels, fnv_sizes(levels));
        }
    uint64_t pbs, levels;
    status("radix_stats op=7 bits=32", fhe_host_radix_stats(FHE_HOST_OP_SHL, 32, &pbs, &levels, NULL, 0), 0);
    status("radix_stats op=99 bits=32", fhe_host_radix_stats(99, 32, &pbs, &levels, NULL, 0), 0);
    status("radix_stats op=1 bits=31", fhe_host_radix_stats(FHE_HOST_OP_MUL, 31, &pbs, &levels, NULL, 0), 0);
}

static void sim_radix(void) {
    const uint32_t widths[2] = {32, 64};
    for (int op = 0; op <= 13; ++op)
        for (int w = 0; w < 2; ++w) {
            const uint32_t bits = widths[w];
            const uint64_t mask = bits == 64 ? ~0ull : (1ull << bits) - 1;
            uint64_t a[1] = {rnd() & mask}, b[1] = {rnd() & mask}, out[4] = {0}, out2[4] = {0}, pbs = 0, levels = 0;
            if (op == FHE_HOST_OP_SHR || op == FHE_HOST_OP_SHL) b[0] %= bits;
            if (b[0] == 0) b[0] = 3;
            char name[64];
            snprintf(name, sizeof name, "sim_radix op=%d bits=%u", op, bits);
            if (!status(name, fhe_host_sim_radix(op, bits, a, b, out, out2, &pbs, &levels), 1)) continue;
            printf("%s pbs=%" PRIu64 " levels=%" PRIu64 " out=", name, pbs, levels);
            words_out(out, 2);
            printf(" out2=");
            words_out(out2, 1);
            printf("\n");
        }
    uint64_t a[1] = {5}, b[1] = {3}, out[4], out2[4];
    status("sim_radix op=99 bits=32", fhe_host_sim_radix(99, 32, a, b, out, out2, NULL, NULL), 0);
    status("sim_radix op=0 bits=32 no out2", fhe_host_sim_radix(FHE_HOST_OP_DIVREM, 32, a, b, out, NULL, NULL, NULL), 0);
}

static void biguint_dry(void) {
    const int flags[3] = {0, FHE_HOST_STATS_COLUMNS, FHE_HOST_CALL_SITE | FHE_HOST_DECRYPT_SUM};
    for (int s = 0; s < 4; ++s)
        for (int mode = 0; mode <= 1; ++mode) {
            const size_t la = kShapes[s][0], lb = kShapes[s][1], lk = kShapes[s][2];
            for (int f = 0; f < 3; ++f) {
                char name[96];
                snprintf(name, sizeof name, "biguint_mul_stats %zux%zu+%zu mode=%d flags=%#x", la, lb, lk, mode, flags[f]);
                uint64_t pbs = 0, levels = 0;
                memset(g_sizes, 0, sizeof g_sizes);
                // the column form of a product without an addend is refused by the library: compared, not required
                if (!status(name, fhe_host_biguint_mul_stats(la, lb, lk, mode | flags[f], &pbs, &levels, g_sizes, CAP), f != 1))
                    continue;
                printf("%s pbs=%" PRIu64 " levels=%" PRIu64 " sizes=%016" PRIx64 "\n", name, pbs, levels, fnv_sizes(levels));
            }
            char name[96];
            snprintf(name, sizeof name, "biguint_mul_fingerprint %zux%zu+%zu mode=%d", la, lb, lk, mode);
            uint64_t fp = 0;
            if (status(name, fhe_host_biguint_mul_fingerprint(la, lb, lk, mode, &fp), 1)) printf("%s fp=%016" PRIx64 "\n", name, fp);
        }
    uint64_t fp;
    status("biguint_mul_fingerprint mode=2", fhe_host_biguint_mul_fingerprint(8, 8, 0, 2, &fp), 0);
}

static void biguint_sim(void) {
    uint32_t a[16], b[16], k[16], out[64];
    for (int s = 0; s < 4; ++s)
        for (int mode = 0; mode <= 1; ++mode)
            for (int site = 0; site <= 1; ++site) {
                const size_t la = kShapes[s][0], lb = kShapes[s][1], lk = kShapes[s][2];
                if (site && !lk) continue;
                limbs(a, la), limbs(b, lb), limbs(k, lk);
                const int m = mode | (site ? FHE_HOST_CALL_SITE | FHE_HOST_DECRYPT_SUM : 0);
                char name[96];
                snprintf(name, sizeof name, "sim_biguint_mul %zux%zu+%zu mode=%#x", la, lb, lk, m);
                size_t n = 0;
                uint64_t pbs = 0, levels = 0;
                if (!status(name, fhe_host_sim_biguint_mul(a, la, b, lb, lk ? k : NULL, lk, m, out, 64, &n, &pbs, &levels), 1))
                    continue;
                printf("%s pbs=%" PRIu64 " levels=%" PRIu64 " n=%zu out=", name, pbs, levels, n);
                limbs_out(out, n);
                printf("\n");
                // the same limbs through the host fold
                snprintf(name, sizeof name, "host_biguint_mul %zux%zu+%zu mode=%d", la, lb, lk, mode);
                if (!site && status(name, fhe_host_biguint_mul(a, la, b, lb, lk ? k : NULL, lk, mode, out, 64, &n), 1)) {
                    printf("%s n=%zu out=", name, n);
                    limbs_out(out, n);
                    printf("\n");
                }
            }
    const size_t cshapes[3][3] = {{8, 8, 8}, {8, 1, 8}, {2, 8, 4}};
    for (int s = 0; s < 3; ++s)
        for (int mode = 0; mode <= 1; ++mode) {
            const size_t la = cshapes[s][0], lb = cshapes[s][1], lk = cshapes[s][2];
            limbs(a, la), limbs(b, lb), limbs(k, lk);
            char name[96];
            snprintf(name, sizeof name, "sim_biguint_mul_add_columns %zux%zu+%zu mode=%d", la, lb, lk, mode);
            uint64_t w[16] = {0}, pbs = 0, levels = 0;
            uint32_t bits = 0;
            if (!status(name, fhe_host_sim_biguint_mul_add_columns(a, la, b, lb, k, lk, mode, w, 16, &bits, &pbs, &levels), 1))
                continue;
            printf("%s pbs=%" PRIu64 " levels=%" PRIu64 " bits=%u words=", name, pbs, levels, bits);
            words_out(w, (bits + 63) / 64);
            printf("\n");
        }
    uint64_t w[1];
    uint32_t bits;
    status("sim_biguint_mul_add_columns short buffer",
           fhe_host_sim_biguint_mul_add_columns(a, 8, b, 8, k, 8, 1, w, 1, &bits, NULL, NULL), 0);
}

static void chain_g(void) {
    uint8_t vals[4 * 31];
    uint32_t g[4] = {0};
    uint64_t pbs = 0, levels = 0;
    for (size_t i = 0; i < sizeof vals; ++i) vals[i] = (uint8_t)(rnd() & 3);
    memset(vals + 31, 3, 31);  // every block at its largest: K mod 2^32 in the wrap window
    if (status("sim_chain_g", fhe_host_sim_chain_g(vals, 4, g, &pbs, &levels), 1))
        printf("sim_chain_g pbs=%" PRIu64 " levels=%" PRIu64 " g= %u %u %u %u\n", pbs, levels, g[0], g[1], g[2], g[3]);
    vals[5] = 4;
    status("sim_chain_g value 4", fhe_host_sim_chain_g(vals, 4, g, NULL, NULL), 0);
}

static void rem_pseudo_mersenne(void) {
    const uint32_t widths[3] = {256, 320, 512};
    for (int w = 0; w < 3; ++w) {
        const uint32_t bits = widths[w];
        char name[64];
        snprintf(name, sizeof name, "rem_pseudo_mersenne_stats bits=%u", bits);
        uint64_t pbs = 0, levels = 0, fp = 0;
        uint32_t folds = 0;
        memset(g_sizes, 0, sizeof g_sizes);
        if (status(name, fhe_host_rem_pseudo_mersenne_stats(bits, 256, kSecpC, 1, &pbs, &levels, g_sizes, CAP, &folds, &fp), 1))
            printf("%s pbs=%" PRIu64 " levels=%" PRIu64 " sizes=%016" PRIx64 " folds=%u fp=%016" PRIx64 "\n", name, pbs, levels,
                   fnv_sizes(levels), folds, fp);
        uint64_t x[8], out[4] = {0};
        for (int i = 0; i < 8; ++i) x[i] = w == 0 ? ~0ull : rnd();  // 2^256 - 1 >= the modulus at 256 bits
        snprintf(name, sizeof name, "sim_rem_pseudo_mersenne bits=%u", bits);
        if (status(name, fhe_host_sim_rem_pseudo_mersenne(bits, x, 256, kSecpC, 1, out, 4, &pbs, &levels, &folds), 1)) {
            printf("%s pbs=%" PRIu64 " levels=%" PRIu64 " folds=%u out=", name, pbs, levels, folds);
            words_out(out, 4);
            printf("\n");
        }
    }
    uint64_t pbs, levels, x[8] = {1}, out[4];
    status("rem_pseudo_mersenne_stats k=255", fhe_host_rem_pseudo_mersenne_stats(512, 255, kSecpC, 1, &pbs, &levels, NULL, 0, NULL, NULL), 0);
    status("rem_pseudo_mersenne_stats bits=31", fhe_host_rem_pseudo_mersenne_stats(31, 256, kSecpC, 1, &pbs, &levels, NULL, 0, NULL, NULL), 0);
    status("sim_rem_pseudo_mersenne short out", fhe_host_sim_rem_pseudo_mersenne(512, x, 256, kSecpC, 1, out, 3, NULL, NULL, NULL), 0);
}

static void mul_add_rem(void) {
    const int modes[4] = {FHE_BIGUINT_COMPAT, FHE_BIGUINT_FAST, FHE_SIGN_PUBLIC_OPERANDS,
                          FHE_SIGN_PUBLIC_OPERANDS | FHE_HOST_MUL_THEN_FOLD};
    uint32_t a[8], b[8], k[8];
    limbs(a, 8), limbs(b, 8), limbs(k, 8);
    a[7] >>= 1, k[7] >>= 1;  // public operands below the modulus
    for (int m = 0; m < 4; ++m)
        for (int sim = 0; sim <= 1; ++sim) {
            char name[64];
            snprintf(name, sizeof name, "biguint_mul_add_rem mode=%#x sim=%d", modes[m], sim);
            uint64_t out[4] = {0}, cols[10] = {0}, pbs = 0, levels = 0, fp = 0;
            uint32_t col_bits = 0, folds = 0;
            memset(g_sizes, 0, sizeof g_sizes);
            if (!status(name, fhe_host_biguint_mul_add_rem(sim, a, 8, b, 8, k, 8, modes[m], 256, kSecpC, 1, out, 4, cols, 10, &col_bits,
                                                           &pbs, &levels, g_sizes, CAP, &folds, &fp), 1))
                continue;
            printf("%s pbs=%" PRIu64 " levels=%" PRIu64 " sizes=%016" PRIx64 " folds=%u fp=%016" PRIx64 " col_bits=%u out=", name, pbs,
                   levels, fnv_sizes(levels), folds, fp, col_bits);
            words_out(out, 4);
            printf(" cols=");
            words_out(cols, 10);
            printf("\n");
        }
    status("biguint_mul_add_rem fold of a compat product",
           fhe_host_biguint_mul_add_rem(0, a, 8, b, 8, k, 8, FHE_BIGUINT_COMPAT | FHE_HOST_MUL_THEN_FOLD, 256, kSecpC, 1, NULL, 0, NULL,
                                        0, NULL, NULL, NULL, NULL, 0, NULL, NULL), 0);
}

// 0..3 roots; 4 reads 0, 1; 5 reads 4; 6 reads 2; 7 reads 5, 6; 8 a late root; 9 reads 8
static void schedule(void) {
    const int32_t off[11] = {0, 0, 0, 0, 0, 2, 3, 4, 6, 6, 7}, deps[7] = {0, 1, 4, 2, 5, 6, 8};
    for (int mode = 0; mode <= 1; ++mode) {
        int32_t level_of[10] = {0}, nlevels = 0;
        char name[32];
        snprintf(name, sizeof name, "schedule_levels mode=%d", mode);
        if (!status(name, fhe_schedule_levels(off, deps, 10, mode, level_of, &nlevels), 1)) continue;
        printf("%s levels=%d of=", name, nlevels);
        for (int i = 0; i < 10; ++i) printf(" %d", level_of[i]);
        printf("\n");
    }
    const int32_t bad[2] = {0, 4};  // node 4 reads itself
    int32_t level_of[10], nlevels;
    status("schedule_levels dependency on a later node", fhe_schedule_levels(off, bad, 5, 0, level_of, &nlevels), 0);
}

// The simulated context (fhe_host_sim_ctx_create): the C ABI's own entry points on the CPU.  A short chain whose
// results feed the next op, the aliasing matrix at one width (op(x, x), op(x, clone), op(x, cast round trip)), a
// BigUintFHE product added to itself before and after its decryption, the audit of the noise budget, and what
// such a context refuses.  Last in main: the generator's earlier draws stay what they were.
static uint64_t sim_value(fhe_ctx* c, fhe_radix* x) {
    uint64_t w[2] = {0, 0};
    status("sim_ctx decrypt", fhe_radix_decrypt(c, NULL, x, w, 2), 1);
    return w[0];
}
typedef int (*binop_fn)(fhe_ctx*, const fhe_radix*, const fhe_radix*, fhe_radix**);
static void sim_context(void) {
    static const struct {
        const char* name;
        binop_fn fn;
    } ops[] = {{"add", fhe_radix_add}, {"sub", fhe_radix_sub}, {"mul", fhe_radix_mul},       {"and", fhe_radix_bitand},
               {"min", fhe_radix_min}, {"max", fhe_radix_max}, {"lt", fhe_radix_lt},         {"shr", fhe_radix_shr},
               {"shl", fhe_radix_shl}, {"div", fhe_radix_div}, {"rem", fhe_radix_rem}};
    const int nops = (int)(sizeof ops / sizeof ops[0]);
    fhe_ctx* c = NULL;
    if (!status("sim_ctx create", fhe_host_sim_ctx_create(&c), 1)) return;
    // a chain at 34 bits: each result is the next step's first operand, the second one is the value itself every other step
    {
        uint64_t xw[1] = {rnd() & ((1ull << 34) - 1)}, yw[1] = {rnd() & ((1ull << 34) - 1)};
        fhe_radix *x = NULL, *y = NULL;
        status("sim_ctx encrypt", fhe_radix_encrypt(c, NULL, xw, 34, &x), 1);
        status("sim_ctx encrypt", fhe_radix_encrypt(c, NULL, yw, 34, &y), 1);
        printf("sim_ctx chain bits=34 x=%010" PRIx64 " y=%010" PRIx64 ":", xw[0], yw[0]);
        for (int step = 0; step < 12 && x; ++step) {
            const int op = step % nops == 6 ? 0 : step % nops;  // lt's one bit is not fed on
            fhe_radix* r = NULL;
            const int self = step % 2 && op != 1 && op != 7 && op < 9;  // not where x op x is a constant
            if (!status(ops[op].name, ops[op].fn(c, x, self ? x : y, &r), 1)) break;
            fhe_radix_destroy(x);  // released while its consumer is pending
            x = r;
            if (step % 3 == 2) printf(" %s=%010" PRIx64, ops[op].name, sim_value(c, x));
        }
        printf(" end=%010" PRIx64 "\n", x ? sim_value(c, x) : 0);
        fhe_radix_destroy(x);
        fhe_radix_destroy(y);
    }
    // the aliasing matrix at 8 bits
    const uint64_t vals[5] = {0, 1, 0xff, 0x80, 0xa5};
    for (int v = 0; v < 5; ++v) {
        fhe_radix *x = NULL, *kinds[3] = {NULL, NULL, NULL}, *wide = NULL;
        status("sim_ctx encrypt", fhe_radix_encrypt(c, NULL, &vals[v], 8, &x), 1);
        kinds[0] = x;
        status("sim_ctx clone", fhe_radix_clone(x, &kinds[1]), 1);
        status("sim_ctx cast", fhe_radix_cast(c, x, 14, &wide), 1);
        status("sim_ctx cast", fhe_radix_cast(c, wide, 8, &kinds[2]), 1);
        for (int k = 0; k < 3; ++k) {
            fhe_radix* out[16] = {NULL};
            for (int op = 0; op < nops; ++op) status(ops[op].name, ops[op].fn(c, x, kinds[k], &out[op]), 1);
            status("divrem", fhe_radix_divrem(c, x, kinds[k], &out[nops], &out[nops + 1]), 1);
            printf("sim_ctx alias x=%02" PRIx64 " kind=%d:", vals[v], k);
            for (int op = 0; op < nops + 2; ++op) {
                printf(" %02" PRIx64, out[op] ? sim_value(c, out[op]) : (uint64_t)0xee);
                fhe_radix_destroy(out[op]);
            }
            printf("\n");
        }
        fhe_radix_destroy(wide);
        for (int k = 0; k < 3; ++k) fhe_radix_destroy(kinds[k]);
    }
    // P = a * b, P + P: decrypted before and after the reuse, compat and fast
    for (int mode = 0; mode <= 1; ++mode) {
        uint32_t a[3], b[3], out[16];
        limbs(a, 3), limbs(b, 3);
        a[2] |= 1u << 31, b[2] |= 1u << 31;
        fhe_biguint *A = NULL, *B = NULL, *P = NULL, *S = NULL, *S2 = NULL;
        size_t n = 0;
        status("sim_ctx biguint encrypt", fhe_biguint_encrypt(c, NULL, a, 3, &A), 1);
        status("sim_ctx biguint encrypt", fhe_biguint_encrypt(c, NULL, b, 3, &B), 1);
        status("sim_ctx biguint mul", fhe_biguint_mul(c, A, B, mode, &P), 1);
        status("sim_ctx P + P", fhe_biguint_add(c, P, P, mode, &S), 1);
        printf("sim_ctx P+P mode=%d sum=", mode);
        if (status("sim_ctx biguint decrypt", fhe_biguint_decrypt(c, NULL, S, out, 16, &n), 1)) limbs_out(out, n);
        printf(" P=");
        if (status("sim_ctx biguint decrypt", fhe_biguint_decrypt(c, NULL, P, out, 16, &n), 1)) limbs_out(out, n);
        status("sim_ctx S + S", fhe_biguint_add(c, S, S, mode, &S2), 1);
        fhe_biguint_destroy(S);  // its propagation is pending behind the decryption above
        printf(" 4P=");
        if (status("sim_ctx biguint decrypt", fhe_biguint_decrypt(c, NULL, S2, out, 16, &n), 1)) limbs_out(out, n);
        printf("\n");
        fhe_biguint_destroy(A), fhe_biguint_destroy(B), fhe_biguint_destroy(P), fhe_biguint_destroy(S2);
    }
    uint64_t label = 0, merged = 0, above = 0, pbs = 0, levels = 0;
    status("sim_ctx noise audit", fhe_ctx_noise_audit(c, &label, &merged, &above, 1), 1);
    status("sim_ctx stats", fhe_ctx_stats(c, &pbs, &levels), 1);
    printf("sim_ctx audit max_label=%" PRIu64 " max_merged=%" PRIu64 " above_label=%" PRIu64 " pbs=%" PRIu64 " levels=%" PRIu64 "\n",
           label, merged, above, pbs, levels);
    // refusals: compared line for line, and the context works after them
    {
        const uint64_t w[1] = {0x5a};
        uint64_t cts[4], words[1] = {0};
        uint8_t buf[64], seed[32] = {1};
        size_t len = 0;
        fhe_radix *x = NULL, *a10 = NULL, *r = NULL;
        status("sim_ctx encrypt", fhe_radix_encrypt(c, NULL, w, 8, &x), 1);
        status("sim_ctx encrypt", fhe_radix_encrypt(c, NULL, w, 10, &a10), 1);
        status("sim_ctx refuses export", fhe_radix_export(c, x, cts, 4), 0);
        status("sim_ctx refuses serialize", fhe_radix_serialize(c, x, buf, sizeof buf, &len), 0);
        status("sim_ctx refuses digest", fhe_radix_digest(c, x, buf), 0);
        status("sim_ctx refuses rerandomize", fhe_radix_rerandomize(c, x, seed, &r), 0);
        status("sim_ctx refuses random", fhe_radix_random(c, seed, 8, 8, &r), 0);
        status("sim_ctx refuses broadcast", fhe_ctx_broadcast_radix(c, &x, 0), 0);
        status("sim_ctx refuses set_server_key", fhe_set_server_key(c, NULL), 0);
        status("sim_ctx refuses pbs", fhe_pbs_batch(c, cts, 0, NULL, cts), 0);
        status("sim_ctx width mismatch", fhe_radix_add(c, x, a10, &r), 0);
        status("sim_ctx division by zero", fhe_radix_scalar_div(c, x, 0, &r), 0);
        if (status("sim_ctx after the refusals", fhe_radix_scalar_mul(c, x, 3, &r), 1) &&
            status("sim_ctx after the refusals", fhe_radix_decrypt(c, NULL, r, words, 1), 1))
            printf("sim_ctx after the refusals 3 * 5a = %02" PRIx64 "\n", words[0]);
        fhe_radix_destroy(x), fhe_radix_destroy(a10), fhe_radix_destroy(r);
    }
    fhe_ctx_destroy(c);
}

// Ownership (include/fhe_rocm.h, the radix section): a handle is a value of the context that made it.  Two or three
// simulated contexts live at once; every line here is a refusal that must happen (a library without the check
// prints the value it computed instead, or ends at the last case).  Then the moduli whose 32-bit product wraps to a
// legal message space.  After sim_context and without the generator: every earlier line stays what it was.  The
// pending-foreign case is the last of the program: a library without the check follows a node index of A into B's
// empty list there.
static void must_refuse(const char* name, int rc, uint64_t value) {
    if (rc == FHE_OK) {
        printf("owner %s: ACCEPTED value=%" PRIx64 "\n", name, value);
        g_failed = 1;
    } else {
        printf("owner %s: rc=%d (%s)\n", name, rc, fhe_last_error());
    }
    fflush(stdout);
}
static fhe_radix* sim_enc(fhe_ctx* c, uint64_t v, uint32_t bits) {
    uint64_t w[4] = {v, 0, 0, 0};
    fhe_radix* x = NULL;
    status("owner encrypt", fhe_radix_encrypt(c, NULL, w, bits, &x), 1);
    return x;
}
static void ownership(void) {
    fhe_ctx *A = NULL, *B = NULL, *C3 = NULL;
    if (!status("owner create", fhe_host_sim_ctx_create(&A), 1) || !status("owner create", fhe_host_sim_ctx_create(&B), 1)) return;
    uint64_t w[4] = {0};
    fhe_radix *a1 = sim_enc(A, 0x1234, 16), *a2 = sim_enc(A, 0x0101, 16), *b1 = sim_enc(B, 0xBEEF, 16), *b2 = sim_enc(B, 0x0F0F, 16);
    fhe_radix *r = NULL, *t = NULL, *p = NULL, *q = NULL;
    // the wrong value of a library without the check: B's shadow under A's placeholder address
    must_refuse("a1.decrypt under B", fhe_radix_decrypt(B, NULL, a1, w, 1), w[0]);
    int rc = fhe_radix_add(B, a1, a2, &r);
    if (rc == FHE_OK) fhe_radix_decrypt(B, NULL, r, w, 1);
    must_refuse("a1 + a2 under B", rc, w[0]);
    fhe_radix_destroy(r), r = NULL;
    must_refuse("b1 + a2 under B", fhe_radix_add(B, b1, a2, &r), 0);
    fhe_radix_destroy(r), r = NULL;
    // trivial values have no owner
    const uint64_t tw[1] = {0x0F0F};
    status("owner trivial", fhe_radix_trivial(A, tw, 16, &t), 1);
    if (status("owner b1 + trivial of A", fhe_radix_add(B, b1, t, &r), 1) && status("owner decrypt", fhe_radix_decrypt(B, NULL, r, w, 1), 1))
        printf("owner b1 + trivial of A = %04" PRIx64 "\n", w[0]);
    fhe_radix_destroy(r), r = NULL;
    // both contexts as they were: the right values under the makers
    if (status("owner a1 + a2 under A", fhe_radix_add(A, a1, a2, &r), 1)) printf("owner a1 + a2 under A = %04" PRIx64 "\n", sim_value(A, r));
    fhe_radix_destroy(r), r = NULL;
    if (status("owner b1 + b2 under B", fhe_radix_add(B, b1, b2, &r), 1)) printf("owner b1 + b2 under B = %04" PRIx64 "\n", sim_value(B, r));
    fhe_radix_destroy(r), r = NULL;
    // lifetimes: a context goes while its handles live; they are refused under a live context, destroyed without
    // an error, and a context made afterwards computes
    {
        fhe_ctx* D = NULL;
        status("owner create", fhe_host_sim_ctx_create(&D), 1);
        fhe_radix *d1 = sim_enc(D, 0x4321, 16), *dp = NULL;
        status("owner d1 * d1 pending", fhe_radix_mul(D, d1, d1, &dp), 1);
        fhe_ctx_destroy(D);
        must_refuse("handle of a destroyed context, decrypt under B", fhe_radix_decrypt(B, NULL, d1, w, 1), w[0]);
        must_refuse("pending handle of a destroyed context, b1 + it under B", fhe_radix_add(B, b1, dp, &r), 0);
        fhe_radix_destroy(r), r = NULL;
        fhe_radix_destroy(d1), fhe_radix_destroy(dp);
        status("owner create", fhe_host_sim_ctx_create(&C3), 1);
        fhe_radix* c1 = sim_enc(C3, 0x4321, 16);
        if (status("owner c1 * c1 under C", fhe_radix_mul(C3, c1, c1, &r), 1)) printf("owner c1 * c1 under C = %04" PRIx64 "\n", sim_value(C3, r));
        must_refuse("c1.decrypt under B", fhe_radix_decrypt(B, NULL, c1, w, 1), w[0]);
        fhe_radix_destroy(r), r = NULL;
        fhe_radix_destroy(c1);
        fhe_ctx_destroy(C3);
    }
    // moduli: each refused on its own, the product formed in 64 bits (a zero carry modulus last: a division by it)
    static const uint32_t moduli[8][2] = {{0x40000001u, 4}, {4, 0x40000001u}, {0x80000000u, 2}, {1, 16}, {3, 4}, {128, 1}, {0, 4}, {2, 0}};
    for (int i = 0; i < 8; ++i) {
        fhe_params prm;
        fhe_client_key* ck = NULL;
        fhe_server_key* sk = NULL;
        status("owner params", fhe_params_default(&prm), 1);
        prm.message_modulus = moduli[i][0], prm.carry_modulus = moduli[i][1];
        char name[64];
        snprintf(name, sizeof name, "generate_keys moduli %#x x %#x", moduli[i][0], moduli[i][1]);
        must_refuse(name, fhe_generate_keys(&prm, 7, &ck, &sk), 0);
        fhe_client_key_destroy(ck), fhe_server_key_destroy(sk);
    }
    // B holds forty 256-bit values and nothing pending; A leaves p = (a1 * a2) * a2 + a1 pending; p + b1 under B
    fhe_radix* held[40];
    for (int i = 0; i < 40; ++i) held[i] = sim_enc(B, (uint64_t)i, 256);
    status("owner flush B", fhe_radix_decrypt(B, NULL, held[39], w, 4), 1);
    status("owner a1 * a2", fhe_radix_mul(A, a1, a2, &q), 1);
    status("owner (a1 * a2) * a2", fhe_radix_mul(A, q, a2, &r), 1);
    status("owner (a1 * a2) * a2 + a1", fhe_radix_add(A, r, a1, &p), 1);
    fhe_radix_destroy(q), fhe_radix_destroy(r), r = NULL;
    printf("owner pending foreign value: p + b1 under B follows\n");
    fflush(stdout);
    rc = fhe_radix_add(B, p, b1, &r);
    if (rc == FHE_OK) fhe_radix_decrypt(B, NULL, r, w, 1);
    must_refuse("p + b1 under B, p pending in A", rc, w[0]);
    fhe_radix_destroy(r), r = NULL;
    printf("owner p under A = %04" PRIx64 "\n", sim_value(A, p));
    if (status("owner b1 + b2 under B", fhe_radix_add(B, b1, b2, &r), 1)) printf("owner b1 + b2 under B afterwards = %04" PRIx64 "\n", sim_value(B, r));
    fhe_radix_destroy(r);
    for (int i = 0; i < 40; ++i) fhe_radix_destroy(held[i]);
    fhe_radix_destroy(a1), fhe_radix_destroy(a2), fhe_radix_destroy(b1), fhe_radix_destroy(b2), fhe_radix_destroy(t), fhe_radix_destroy(p);
    fhe_ctx_destroy(A);
    fhe_ctx_destroy(B);
}

int main(void) {
    radix_stats();
    sim_radix();
    biguint_dry();
    biguint_sim();
    chain_g();
    rem_pseudo_mersenne();
    mul_add_rem();
    schedule();
    sim_context();
    ownership();
    printf(g_failed ? "engine host modes: a required case failed\n" : "engine host modes: every required case ran\n");
    return g_failed;
}
