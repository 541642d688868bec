// capi_host.cpp -- the C ABI's host-only hooks (fhe_host_*, fhe_schedule_levels): the radix and BigUintFHE
// algorithms run on a host engine (engine.h: kHostFold on public values, kDry for the schedule, kSim with a
// plaintext shadow), no GPU and no key.  The CPU tests and tools/engine_host_check.c drive them.
#include <algorithm>
#include <memory>
#include <string>

#include "capi_internal.h"

using namespace fhe;

namespace {

// how a hook's operand blocks are made: public values, placeholders, or placeholders with a shadowed value
enum class Kind { kTrivial, kDry, kSim };
Kind kind_of(bool sim) { return sim ? Kind::kSim : Kind::kDry; }

// nblocks blocks holding the words' 2-bit digits (LSB first; w == nullptr: zeros, a dry operand's values are
// never read); odd_trivial: the odd positions public whatever the kind
Radix radix_of_words(Engine& e, Kind kind, const uint64_t* w, uint32_t nblocks, bool odd_trivial = false) {
    Radix r;
    for (uint32_t q = 0; q < nblocks; ++q) {
        const uint32_t v = w ? (uint32_t)(w[q / 32] >> (2 * (q % 32))) & 3u : 0u;
        if (kind == Kind::kTrivial || (odd_trivial && (q & 1)))
            r.blocks.push_back(Block::make_trivial(v));
        else
            r.blocks.push_back(kind == Kind::kSim ? e.sim_block(v, 3) : e.dry_block(3));
    }
    return r;
}

// n FheUint32 limbs (v == nullptr: zeros)
BigUint biguint_of_limbs(Engine& e, Kind kind, const uint32_t* v, size_t n) {
    BigUint r;
    for (size_t i = 0; i < n; ++i) {
        const uint64_t w = v ? v[i] : 0;
        r.digits.push_back(radix_of_words(e, kind, &w, kLimbBlocks));
    }
    return r;
}

BigConst limb_words(const uint32_t* v, size_t n) {
    BigConst w((n + 1) / 2, 0);
    for (size_t i = 0; i < n; ++i) w[i / 2] |= (uint64_t)v[i] << (32 * (i % 2));
    return w;
}

// a * b, or with K: K + a * b -- in one call, or as the reference's call site (mul, then add with the product
// released)
BigUint mul_maybe_add(Engine& e, const BigUint& A, const BigUint& B, const BigUint* K, int mode, bool callsite) {
    if (!K) return biguint_mul(e, A, B, mode);
    return callsite ? biguint_add(e, *K, biguint_mul(e, A, B, mode), mode) : biguint_mul_add(e, A, B, *K, mode);
}

// the digit of a clean result block of a host engine (folded: it must have folded to a public value)
uint32_t clean_digit(const Engine& e, const Block& b, bool folded, const char* what) {
    engine_check(!folded || b.trivial(), what);
    const int64_t h2 = e.sim_half2(b);
    engine_check(h2 % 2 == 0 && h2 >= 0 && h2 < 8, what);
    return (uint32_t)(h2 / 2);
}

// a host engine's clean result -> words
void put_radix_words(const Engine& e, const Radix& r, uint64_t* w, size_t nwords) {
    engine_check(nwords * 64 >= 2 * (size_t)r.nblocks(), "sim: word buffer too small");
    for (size_t i = 0; i < nwords; ++i) w[i] = 0;
    for (uint32_t q = 0; q < r.nblocks(); ++q)
        w[q / 32] |= (uint64_t)clean_digit(e, r.blocks[q], false, "sim radix: an output block off its digit range") << (2 * (q % 32));
}

// ... -> limbs (*n: their number; out optional, up to cap)
void put_limbs(const Engine& e, const BigUint& R, bool folded, uint32_t* out, size_t cap, size_t* n) {
    *n = R.digits.size();
    engine_check(R.digits.size() <= cap || !out, "output buffer too small");
    const char* what = folded ? "host mul: a non-trivial output block" : "sim mul: an output block off its digit range";
    for (size_t i = 0; out && i < R.digits.size(); ++i) {
        uint64_t v = 0;
        for (uint32_t q = 0; q < R.digits[i].nblocks(); ++q) v |= (uint64_t)clean_digit(e, R.digits[i].blocks[q], folded, what) << (2 * q);
        out[i] = (uint32_t)v;
    }
}

// the value of a simulated column form -> words
void put_sim_columns(const Engine& e, const std::vector<Blocks>& cols, uint32_t nb, uint64_t* words, size_t nwords) {
    engine_check(nwords * 64 >= 2 * (size_t)nb, "sim columns: word buffer too small");
    column_value(cols, nb, [&](const Block& x) {
        const int64_t h2 = e.sim_half2(x);
        engine_check(h2 % 2 == 0 && h2 >= 0 && h2 < 32, "sim columns: a block off its message range");
        return h2 / 2;
    }, words, nwords);
}

void put_schedule(const Engine& e, uint64_t* pbs, uint64_t* levels, uint32_t* level_sizes, size_t cap) {
    if (pbs) *pbs = e.pbs_count;
    if (levels) *levels = e.levels;
    for (size_t i = 0; level_sizes && i < e.level_log.size() && i < cap; ++i) level_sizes[i] = e.level_log[i];
}

bool host_width_ok(uint32_t bits) {
    if (bits >= 2 && bits % 2 == 0 && bits <= FHE_RADIX_MAX_BITS) return true;
    set_error("operand width must be even and within 2 .. FHE_RADIX_MAX_BITS");
    return false;
}

// One radix op (FHE_HOST_OP_*) on A, B of nb blocks; b: B's clear words, for the ops that take it public.  The
// results stay referenced through the caller's flush (else they are dead nodes); SCALAR_MAC_COLUMNS leaves its
// column form in *cols.  The ops above DIV_SCALAR exist on a simulating engine only.
std::vector<Radix> host_op(Engine& e, int op, bool sim, const Radix& A, const Radix& B, const uint64_t* b, uint32_t nb,
                           std::vector<Blocks>* cols) {
    engine_check(sim || op <= FHE_HOST_OP_DIV_SCALAR, "unknown host op");
    switch (op) {
    case FHE_HOST_OP_DIVREM: {
        auto qr = radix_divrem(e, A, B);
        return {qr.first, qr.second};
    }
    case FHE_HOST_OP_MUL: return {radix_mul(e, A, B, nb)};
    case FHE_HOST_OP_ADD: return {radix_sum(e, {&A, &B}, nb)};
    case FHE_HOST_OP_SUB: return {radix_sub(e, A, B)};
    case FHE_HOST_OP_SHR: return {radix_shr(e, A, B)};
    case FHE_HOST_OP_LT: return {Radix{{radix_lt(e, A, B)}}};
    case FHE_HOST_OP_DIV_SCALAR: return {radix_scalar_div(e, A, BigConst{0xC0FFEE01u})};
    case FHE_HOST_OP_SHL: return {radix_shl(e, A, B)};
    case FHE_HOST_OP_MUL_FULL: return {radix_mul(e, A, B, 2 * nb)};
    case FHE_HOST_OP_AND: return {radix_bitand(e, A, B)};
    case FHE_HOST_OP_MIN: return {radix_min(e, A, B)};
    case FHE_HOST_OP_DIVREM_CLEAR:
    case FHE_HOST_OP_DIVREM_CLEAR_MIXED: {  // a / b, a % b with b public
        const BigConst d = words_of(b, (2 * nb + 63) / 64);
        return {radix_scalar_div(e, A, d), radix_scalar_rem(e, A, d)};
    }
    case FHE_HOST_OP_SCALAR_MAC_COLUMNS: {  // a * m + m, m = b public: the public signer's column form
        const BigConst m = words_of(b, (2 * nb + 63) / 64);
        *cols = radix_mul_add_columns(e, A, radix_trivial(m, nb), radix_trivial(m, nb), nb);
        return {};
    }
    default: engine_check(false, "unknown host op");
    }
    return {};
}

}  // namespace

extern "C" {

int fhe_schedule_levels(const int32_t* off, const int32_t* deps, size_t n, int mode, int32_t* level_of,
                        int32_t* nlevels) {
    return fhe_schedule_levels_ranks(off, deps, n, mode, 1, level_of, nlevels);
}

int fhe_schedule_levels_ranks(const int32_t* off, const int32_t* deps, size_t n, int mode, int ranks, int32_t* level_of,
                              int32_t* nlevels) {
    if ((n && (!off || !level_of)) || !nlevels || (mode != 0 && mode != 1) || ranks < 1) return FHE_ERR_INVALID;
    return guarded([&] {
        std::vector<std::vector<int32_t>> g(n);
        for (size_t i = 0; i < n; ++i)
            for (int32_t k = off[i]; k < off[i + 1]; ++k) {
                engine_check(deps && deps[k] >= 0 && (size_t)deps[k] < i, "dependency must name an earlier node");
                g[i].push_back(deps[k]);
            }
        // the engine's flush (engine.cpp): a fanned-out level's fill granule is one latency round per rank
        std::vector<std::vector<int32_t>> lv = schedule_levels(g, mode, (size_t)256 * (size_t)ranks);
        for (size_t l = 0; l < lv.size(); ++l)
            for (int32_t i : lv[l]) level_of[i] = (int32_t)l + 1;
        *nlevels = (int32_t)lv.size();
        return FHE_OK;
    });
}

// A simulated context: no device, no stream, the default parameters, has_key set, an Engine::kSim engine.  The
// C ABI's radix layer runs on it through its real code (capi_radix.cpp: widths, casts, clones, word forms, amounts
// of another width, the column-form decryption and its partial flush): fhe_radix_encrypt / fhe_biguint_encrypt make
// shadowed blocks of the plaintext (the client key is ignored and may be NULL), the decryptions make the flush a
// device decryption makes and read the shadow.  What needs device memory or a real key refuses with
// FHE_ERR_INVALID and leaves the context usable.  fhe_ctx_destroy frees it.
// Known limit: the shadow evaluates a bootstrap when it is RECORDED, so a test on this context sees every recorded
// graph and every value, not the launch order -- a schedule that launched a node before its producer would pass.
int fhe_host_sim_ctx_create(fhe_ctx** ctx) {
    if (!ctx) return FHE_ERR_INVALID;
    return guarded([&] {
        auto c = std::make_unique<fhe_ctx>();
        c->simulated = true;
        c->has_key = true;
        c->engine = new Engine(c.get(), Engine::kSim);
        *ctx = c.release();
        return FHE_OK;
    });
}

// Host-only run of the BigUintFHE mul / mul-add on publicly known limbs (no GPU, no key): every block
// is trivial, so the engine folds each lookup on the host (Engine host_only) -- the radix algorithms'
// indexing, LUTs and carry logic checked on the CPU against the reference's limb loop.
int fhe_host_biguint_mul(const uint32_t* a, size_t la, const uint32_t* b, size_t lb, const uint32_t* k, size_t lk,
                         int mode, uint32_t* out, size_t cap, size_t* n) {
    if ((la && !a) || (lb && !b) || (lk && !k) || !n || (mode != kCompat && mode != kFast)) return FHE_ERR_INVALID;
    return guarded([&] {
        fhe_ctx c;  // parameters only: a host-only engine never touches the device
        Engine e(&c, Engine::kHostFold);
        const BigUint A = biguint_of_limbs(e, Kind::kTrivial, a, la), B = biguint_of_limbs(e, Kind::kTrivial, b, lb);
        const BigUint K = biguint_of_limbs(e, Kind::kTrivial, k, lk);
        put_limbs(e, mul_maybe_add(e, A, B, k ? &K : nullptr, mode, false), true, out, cap, n);
        return FHE_OK;
    });
}

// The recording-order fingerprint (Engine::fingerprint) of a dry la x lb BigUintFHE mul (or k + a * b)
int fhe_host_biguint_mul_fingerprint(size_t la, size_t lb, size_t lk, int mode, uint64_t* fp) {
    if (!fp || (mode != kCompat && mode != kFast)) return FHE_ERR_INVALID;
    return guarded([&] {
        fhe_ctx c;
        Engine e(&c, Engine::kDry);
        const BigUint A = biguint_of_limbs(e, Kind::kDry, nullptr, la), B = biguint_of_limbs(e, Kind::kDry, nullptr, lb);
        const BigUint K = biguint_of_limbs(e, Kind::kDry, nullptr, lk);
        const BigUint R = mul_maybe_add(e, A, B, lk ? &K : nullptr, mode, false);
        e.flush();
        *fp = e.fingerprint;
        return FHE_OK;
    });
}

// Test hooks of the radix size rules (engine.h Tuning): process-wide, *previous gets the old value
int fhe_host_set_tuning(int key, int64_t value, int64_t* previous) {
    Tuning& t = tuning();
    int64_t old;
    switch (key) {
    case FHE_TUNE_KARA_MIN: old = t.kara_min; t.kara_min = (uint32_t)std::max<int64_t>(0, value); break;
    case FHE_TUNE_KARA_COMPAT_MIN: old = t.kara_compat_min; t.kara_compat_min = (uint32_t)std::max<int64_t>(0, value); break;
    case FHE_TUNE_KARA_FORCE: old = t.kara_force; t.kara_force = value != 0; break;
    case FHE_TUNE_DIV_R16_LEAD: old = t.div_r16_lead; t.div_r16_lead = (uint32_t)std::max<int64_t>(0, value); break;
    case FHE_TUNE_FLUSH_DEPTH: old = t.flush_depth; t.flush_depth = (uint32_t)std::max<int64_t>(0, value); break;
    case FHE_TUNE_FAULT_SITES: old = t.fault_sites; t.fault_sites = (uint32_t)std::max<int64_t>(0, value) & 63u; break;
    case FHE_TUNE_FAULT_AFTER:  // previous: the crossings of enabled sites since this key was last set
        old = (int64_t)t.fault_crossings;
        t.fault_crossings = 0;
        t.fault_after = (uint64_t)std::max<int64_t>(0, value);
        break;
    case FHE_TUNE_SCALAR_DIV_RESIDUE:
        old = t.scalar_div_residue;
        t.scalar_div_residue = value < 0 ? -1 : value != 0;
        break;
    default: return FHE_ERR_INVALID;
    }
    if (previous) *previous = old;
    return FHE_OK;
}

// Dry run (no GPU): the same op on la x lb "encrypted" limbs (placeholder blocks) recorded and scheduled
// by the engine without launching anything -- its bootstrap count, launch levels and level sizes.
int fhe_host_biguint_mul_stats(size_t la, size_t lb, size_t lk, int mode, uint64_t* pbs, uint64_t* levels,
                               uint32_t* level_sizes, size_t cap) {
    const bool columns = (mode & FHE_HOST_STATS_COLUMNS) != 0;  // the signer's column form instead
    const bool callsite = (mode & FHE_HOST_CALL_SITE) != 0;    // mul, then add (the product released)
    const bool dec = (mode & FHE_HOST_DECRYPT_SUM) != 0;       // ... and the sum's decryption launched
    mode &= ~(FHE_HOST_STATS_COLUMNS | FHE_HOST_CALL_SITE | FHE_HOST_DECRYPT_SUM);
    if (!pbs || !levels || (mode != kCompat && mode != kFast)) return FHE_ERR_INVALID;
    return guarded([&] {
        fhe_ctx c;
        Engine e(&c, Engine::kDry);
        const BigUint A = biguint_of_limbs(e, Kind::kDry, nullptr, la), B = biguint_of_limbs(e, Kind::kDry, nullptr, lb);
        const BigUint K = biguint_of_limbs(e, Kind::kDry, nullptr, lk);
        BigUint R;
        std::vector<Blocks> cols;
        uint32_t nb = 0;
        if (columns)
            cols = biguint_mul_add_columns(e, A, B, K, mode, &nb);
        else
            R = mul_maybe_add(e, A, B, lk ? &K : nullptr, mode, callsite);
        if (dec && R.sum_cols)
            e.flush_for(col_blocks(*R.sum_cols));
        else
            e.flush();
        put_schedule(e, pbs, levels, level_sizes, cap);
        return FHE_OK;
    });
}

// Dry run of one radix op on encrypted operands of the given widths (FHE_HOST_OP_*): its bootstrap
// count and launch levels as the engine schedules them, nothing launched.
int fhe_host_radix_stats(int op, uint32_t bits, uint64_t* pbs, uint64_t* levels, uint32_t* level_sizes, size_t cap) {
    if (!pbs || !levels || bits < 2 || bits % 2 || bits > FHE_RADIX_MAX_BITS) return FHE_ERR_INVALID;
    return guarded([&] {
        fhe_ctx c;
        Engine e(&c, Engine::kDry);
        const Radix A = radix_of_words(e, Kind::kDry, nullptr, bits / 2), B = radix_of_words(e, Kind::kDry, nullptr, bits / 2);
        const std::vector<Radix> keep = host_op(e, op, false, A, B, nullptr, bits / 2, nullptr);
        e.flush();
        put_schedule(e, pbs, levels, level_sizes, cap);
        return FHE_OK;
    });
}

// Simulated run (Engine kSim, no GPU, no key) of x mod (2^k_bits - c) on a `bits`-wide operand: out gets
// the k_bits-wide result (words LSB first, nout >= ceil(k_bits / 64)); *pbs, *levels, *folds optional
int fhe_host_sim_rem_pseudo_mersenne(uint32_t bits, const uint64_t* x, uint32_t k_bits, const uint64_t* c_words, size_t nc,
                                     uint64_t* out, size_t nout, uint64_t* pbs, uint64_t* levels, uint32_t* folds) {
    if (!x || !c_words || !nc || !out) return FHE_ERR_INVALID;
    if (!host_width_ok(bits)) return FHE_ERR_INVALID;
    const BigConst cc = words_of(c_words, nc);
    return guarded([&] {
        fhe_ctx c;
        Engine e(&c, Engine::kSim);
        const Radix A = radix_of_words(e, Kind::kSim, x, bits / 2);
        const Radix R = radix_rem_pseudo_mersenne(e, A, k_bits, cc, folds);
        e.flush();
        engine_check(2 * R.nblocks() == k_bits, "sim: the remainder's width is not k");
        put_radix_words(e, R, out, nout);
        put_schedule(e, pbs, levels, nullptr, 0);
        return FHE_OK;
    });
}

// Dry run (Engine kDry) of the same: bootstraps, launch levels, level sizes (up to cap), folds, and the
// recording-order fingerprint (Engine::fingerprint: equal across processes iff the same graph is recorded
// in the same order)
int fhe_host_rem_pseudo_mersenne_stats(uint32_t bits, uint32_t k_bits, const uint64_t* c_words, size_t nc, uint64_t* pbs,
                                       uint64_t* levels, uint32_t* level_sizes, size_t cap, uint32_t* folds,
                                       uint64_t* fingerprint) {
    if (!c_words || !nc || !pbs || !levels) return FHE_ERR_INVALID;
    if (!host_width_ok(bits)) return FHE_ERR_INVALID;
    const BigConst cc = words_of(c_words, nc);
    return guarded([&] {
        fhe_ctx c;
        Engine e(&c, Engine::kDry);
        const Radix A = radix_of_words(e, Kind::kDry, nullptr, bits / 2);
        const Radix R = radix_rem_pseudo_mersenne(e, A, k_bits, cc, folds);
        e.flush();
        put_schedule(e, pbs, levels, level_sizes, cap);
        if (fingerprint) *fingerprint = e.fingerprint;
        return FHE_OK;
    });
}

// Simulated (sim != 0, kSim) or dry (kDry; encrypted limbs' values are ignored, their counts matter; public
// operands are read in both) run of the reduced signer's FHE block: (k + a * b) mod (2^k_bits - c).
//   mode FHE_COMPAT / FHE_FAST: all three encrypted, biguint_mul_add_columns then the column-form reduction;
//     cols_out (optional, ncols words) gets the column form's value, *col_bits its width -- what the
//     unreduced signer decrypts, so out == cols_out mod n whatever carries the compat product lost.
//   mode FHE_SIGN_PUBLIC_OPERANDS: a and k public, b encrypted, the product reduced as it is formed
//     (radix_scalar_mul_add_rem_pseudo_mersenne: what fhe_schnorr_eval_s_public records).
//   mode FHE_SIGN_PUBLIC_OPERANDS | FHE_HOST_MUL_THEN_FOLD: the same operands through the unreduced public
//     signer's column form (b widened to its exact width) and the column-form reduction: the alternative
//     the residue form is measured against.
int fhe_host_biguint_mul_add_rem(int sim, const uint32_t* a, size_t la, const uint32_t* b, size_t lb, const uint32_t* k,
                                 size_t lk, int mode, uint32_t k_bits, const uint64_t* c_words, size_t nc, uint64_t* out,
                                 size_t nout, uint64_t* cols_out, size_t ncols, uint32_t* col_bits, uint64_t* pbs,
                                 uint64_t* levels, uint32_t* level_sizes, size_t cap, uint32_t* folds,
                                 uint64_t* fingerprint) {
    const bool then_fold = (mode & FHE_HOST_MUL_THEN_FOLD) != 0;
    mode &= ~FHE_HOST_MUL_THEN_FOLD;
    if ((la && !a) || (lb && !b) || (lk && !k) || !c_words || !nc || (sim && !out) ||
        (mode != kCompat && mode != kFast && mode != FHE_SIGN_PUBLIC_OPERANDS) ||
        (then_fold && mode != FHE_SIGN_PUBLIC_OPERANDS))
        return FHE_ERR_INVALID;
    const BigConst cc = words_of(c_words, nc);
    return guarded([&] {
        fhe_ctx c;
        Engine e(&c, sim ? Engine::kSim : Engine::kDry);
        const Kind kind = kind_of(sim != 0);
        auto col_value = [&](const std::vector<Blocks>& cols, uint32_t nb) {
            if (col_bits) *col_bits = 2 * nb;
            if (sim && cols_out) put_sim_columns(e, cols, nb, cols_out, ncols);
        };
        Radix R;
        if (mode == FHE_SIGN_PUBLIC_OPERANDS) {
            const BigUint B = biguint_of_limbs(e, kind, b, lb);
            Radix d;
            for (const Radix& x : B.digits) d.blocks.insert(d.blocks.end(), x.blocks.begin(), x.blocks.end());
            if (then_fold) {
                const uint32_t nb = (uint32_t)(16 * lb + 16 * std::max(la, lk) + 1);
                engine_check(2 * (uint64_t)nb <= FHE_RADIX_MAX_BITS, "operand width out of range");
                const Radix dw = radix_resize(d, nb);
                const std::vector<Blocks> cols =
                    radix_mul_add_columns(e, dw, radix_trivial(limb_words(a, la), nb), radix_trivial(limb_words(k, lk), nb), nb);
                R = radix_rem_pseudo_mersenne_columns(e, cols, nb, k_bits, cc, folds);
                e.flush();
                col_value(cols, nb);
            } else {
                R = radix_scalar_mul_add_rem_pseudo_mersenne(e, d, limb_words(a, la), limb_words(k, lk), k_bits, cc, folds);
                e.flush();
            }
        } else {
            const BigUint A = biguint_of_limbs(e, kind, a, la), B = biguint_of_limbs(e, kind, b, lb);
            const BigUint K = biguint_of_limbs(e, kind, k, lk);
            uint32_t nb = 0;
            const std::vector<Blocks> cols = biguint_mul_add_columns(e, A, B, K, mode, &nb);
            R = radix_rem_pseudo_mersenne_columns(e, cols, nb, k_bits, cc, folds);
            e.flush();
            col_value(cols, nb);
        }
        if (sim) put_radix_words(e, R, out, nout);
        put_schedule(e, pbs, levels, level_sizes, cap);
        if (fingerprint) *fingerprint = e.fingerprint;
        return FHE_OK;
    });
}

// Simulated runs (no GPU, no key; Engine kSim): the operands are "encrypted" blocks whose plaintext
// the engine shadows on the host, so the algorithms take every encrypted path (no trivial folding)
// while each bootstrap is evaluated from its LUT and range-checked -- the end-to-end results of the
// radix algorithms on the CPU.  *pbs / *levels (optional): the op's schedule, as fhe_host_*_stats.
int fhe_host_sim_biguint_mul(const uint32_t* a, size_t la, const uint32_t* b, size_t lb, const uint32_t* k, size_t lk,
                             int mode, uint32_t* out, size_t cap, size_t* n, uint64_t* pbs, uint64_t* levels) {
    const bool callsite = (mode & FHE_HOST_CALL_SITE) != 0;
    const bool dec = (mode & FHE_HOST_DECRYPT_SUM) != 0;
    mode &= ~(FHE_HOST_CALL_SITE | FHE_HOST_DECRYPT_SUM);
    if ((la && !a) || (lb && !b) || (lk && !k) || !n || (mode != kCompat && mode != kFast)) return FHE_ERR_INVALID;
    return guarded([&] {
        fhe_ctx c;
        Engine e(&c, Engine::kSim);
        const BigUint A = biguint_of_limbs(e, Kind::kSim, a, la), B = biguint_of_limbs(e, Kind::kSim, b, lb);
        const BigUint K = biguint_of_limbs(e, Kind::kSim, k, lk);
        const BigUint R = mul_maybe_add(e, A, B, k ? &K : nullptr, mode, callsite);
        if (dec && R.sum_cols) {
            // what fhe_biguint_decrypt launches for a sum: its columns' closure; their value (the
            // columns' plaintext shadows) must be the digits' (whose carry propagation stays pending)
            e.flush_for(col_blocks(*R.sum_cols));
            const uint32_t nb = (uint32_t)R.digits.size() * kLimbBlocks;
            std::vector<uint64_t> w((2 * (size_t)nb + 63) / 64), d(w.size(), 0);
            column_value(*R.sum_cols, nb, [&](const Block& b) { return e.sim_half2(b) / 2; }, w.data(), w.size());
            for (size_t i = 0; i < R.digits.size(); ++i)
                for (uint32_t q = 0; q < kLimbBlocks; ++q) {
                    const uint32_t bit = (uint32_t)(i * 32 + 2 * q);
                    d[bit / 64] |= (uint64_t)(e.sim_half2(R.digits[i].blocks[q]) / 2) << (bit % 64);
                }
            engine_check(w == d, "sim: the sum's column form and its digits differ");
        } else {
            e.flush();
        }
        put_limbs(e, R, false, out, cap, n);
        put_schedule(e, pbs, levels, nullptr, 0);
        return FHE_OK;
    });
}

// biguint_mul_add_columns on simulated limbs: the column form's value (words LSB first, nwords >=
// its bits / 64) -- what fhe_columns_decrypt returns
int fhe_host_sim_biguint_mul_add_columns(const uint32_t* a, size_t la, const uint32_t* b, size_t lb, const uint32_t* k,
                                         size_t lk, int mode, uint64_t* words, size_t nwords, uint32_t* bits,
                                         uint64_t* pbs, uint64_t* levels) {
    if ((la && !a) || (lb && !b) || (lk && !k) || !words || !bits || (mode != kCompat && mode != kFast))
        return FHE_ERR_INVALID;
    return guarded([&] {
        fhe_ctx c;
        Engine e(&c, Engine::kSim);
        const BigUint A = biguint_of_limbs(e, Kind::kSim, a, la), B = biguint_of_limbs(e, Kind::kSim, b, lb);
        const BigUint K = biguint_of_limbs(e, Kind::kSim, k, lk);
        uint32_t nb = 0;
        const std::vector<Blocks> cols = biguint_mul_add_columns(e, A, B, K, mode, &nb);
        e.flush();
        *bits = 2 * nb;
        put_sim_columns(e, cols, nb, words, nwords);
        put_schedule(e, pbs, levels, nullptr, 0);
        return FHE_OK;
    });
}

int fhe_host_sim_chain_g(const uint8_t* vals, size_t nprefix, uint32_t* g, uint64_t* pbs, uint64_t* levels) {
    if ((nprefix && (!vals || !g))) return FHE_ERR_INVALID;
    return guarded([&] {
        fhe_ctx c;
        Engine e(&c, Engine::kSim);
        std::vector<std::vector<Blocks>> P(nprefix, std::vector<Blocks>(kLimbBlocks));
        for (size_t k = 0; k < nprefix; ++k) {
            const uint8_t* v = vals + 31 * k;
            for (int q = 0; q < 31; ++q) engine_check(v[q] <= 3, "sim chain g: a block value above 3");
            P[k][0].push_back(e.sim_block(v[0], 3));
            for (uint32_t m = 1; m < kLimbBlocks; ++m)
                for (int q = 0; q < 2; ++q) P[k][m].push_back(e.sim_block(v[1 + 2 * (m - 1) + q], 3));
        }
        std::vector<const std::vector<Blocks>*> ptrs;
        for (auto& x : P) ptrs.push_back(&x);
        const Blocks out = compat_chain_g(e, ptrs);
        e.flush();
        for (size_t k = 0; k < nprefix; ++k) {
            const int64_t h2 = e.sim_half2(out[k]);
            engine_check(h2 % 2 == 0 && h2 >= 0 && h2 < 32, "sim chain g: g off its range");
            g[k] = (uint32_t)(h2 / 2);
        }
        put_schedule(e, pbs, levels, nullptr, 0);
        return FHE_OK;
    });
}

// One radix op (FHE_HOST_OP_*) on simulated operands a, b of `bits` (words LSB first, ceil(bits / 64)
// each); out gets the result (MUL_FULL: 2 bits wide; LT / the comparison: 0 or 1 in out[0]); out2 the
// remainder of DIVREM.
int fhe_host_sim_radix(int op, uint32_t bits, const uint64_t* a, const uint64_t* b, uint64_t* out, uint64_t* out2,
                       uint64_t* pbs, uint64_t* levels) {
    if (!a || !b || !out || bits < 2 || bits % 2 || bits > FHE_RADIX_MAX_BITS) return FHE_ERR_INVALID;
    const bool two = op == FHE_HOST_OP_DIVREM || op == FHE_HOST_OP_DIVREM_CLEAR || op == FHE_HOST_OP_DIVREM_CLEAR_MIXED;
    if (two && !out2) return FHE_ERR_INVALID;
    return guarded([&] {
        fhe_ctx c;
        Engine e(&c, Engine::kSim);
        const uint32_t nb = bits / 2;
        const Radix A = radix_of_words(e, Kind::kSim, a, nb, op == FHE_HOST_OP_DIVREM_CLEAR_MIXED);
        const Radix B = radix_of_words(e, Kind::kSim, b, nb);
        std::vector<Blocks> cols;
        const std::vector<Radix> keep = host_op(e, op, true, A, B, b, nb, &cols);
        e.flush();
        if (op == FHE_HOST_OP_SCALAR_MAC_COLUMNS) {
            put_sim_columns(e, cols, nb, out, (bits + 63) / 64);
        } else {
            put_radix_words(e, keep[0], out, (keep[0].nblocks() + 31) / 32);
            if (two) put_radix_words(e, keep[1], out2, (keep[1].nblocks() + 31) / 32);
        }
        put_schedule(e, pbs, levels, nullptr, 0);
        return FHE_OK;
    });
}

}  // extern "C"
