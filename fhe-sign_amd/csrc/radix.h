// radix.h -- radix-integer layer over the GPU PBS pipeline.
//
// Replaces tfhe 0.10.0's integer layer under the FheUint{8,32,64} operators the reference calls
// (src/biguint.rs:135-143,221-248; src/perf_test.rs:28-54).  A radix integer of B bits is B/2
// blocks (engine.h), least significant first; every bootstrap of an op goes through Engine::run.
#pragma once
#include "bigconst.h"
#include "engine.h"

namespace fhe {

// ----------------------------------------------------------------------------- radix ops
// All take/return clean blocks (degree <= 3, noise <= 1) unless stated; widths in blocks.
struct Radix {
    Blocks blocks;
    uint32_t nblocks() const { return (uint32_t)blocks.size(); }
};

Radix radix_trivial(uint64_t value_lo, uint64_t value_hi, uint32_t nblocks);
Radix radix_trivial(const BigConst& value, uint32_t nblocks);
Radix radix_resize(const Radix& a, uint32_t nblocks);  // cast: truncate / zero-extend

// Sum of several radix integers (wrapping at `nblocks`; carries propagated).  Used for every add.
Radix radix_sum(Engine& e, const std::vector<const Radix*>& xs, uint32_t nblocks);
// Independent sums advanced through shared levels (one launch pair per level for all of them).
std::vector<Radix> radix_sum_many(Engine& e, const std::vector<std::vector<const Radix*>>& xs,
                                  const std::vector<uint32_t>& nblocks);
// Wrapping window adds w_i + x_i (mod 2^(2 |w_i|)) whose results stay lazy: out_k = v_k + c_(k-1)
// - 4 c_k as an un-bootstrapped combination (range [0, 3], noise 19), so a chain of adds skips the
// final (v + c) mod 4 level.  Inputs: clean x_i; window blocks clean or lazy, where every lazy block
// must belong to a Radix in `refresh` -- those get their cleaning bootstrap in this call's state
// level (updated in place), and the outputs reference the clean copies.  Lazy blocks feed PBS
// inputs only (one lazy term per input); radix_clean turns them back into blocks.
std::vector<Radix> radix_sum_lazy(Engine& e, const std::vector<std::pair<const Radix*, const Radix*>>& xs,
                                  std::vector<Radix*>& refresh);
// Carry propagation of raw column blocks (each column may hold several blocks).
// (compressed: if set, the columns after compression, before the carry propagation -- same value mod
// 4^nblocks, each column <= 7)
Radix radix_propagate_columns(Engine& e, std::vector<Blocks> cols, uint32_t nblocks, uint32_t cap0 = 0,
                              std::vector<Blocks>* compressed = nullptr);
// first-round compression cap for the columns of a * b (4 when both are encrypted and one has <= 16
// live blocks, else 0; radix.cpp)
uint32_t narrow_cap(const Radix& a, const Radix& b);
// The carry out of the top column of each problem (columns already bounded: each a sum <= 6, <= 7 at
// position 0, of <= 3 blocks), and nothing below it: one state level + the carry-chain nodes that
// carry depends on.  A clean bit per problem.
Blocks radix_carry_outs(Engine& e, const std::vector<std::vector<Blocks>>& problems);
// Wrapping product.
Radix radix_mul(Engine& e, const Radix& a, const Radix& b, uint32_t nblocks);
// radix_mul that also hands back the product's block-product columns (before any compression) when
// they sum to the product exactly (no Karatsuba split), else leaves *cols empty: a later add can
// propagate its operand + these columns in one pass (biguint_add), the product's own normalization
// then being dead if nothing else reads it
Radix radix_mul_keep_columns(Engine& e, const Radix& a, const Radix& b, uint32_t nblocks, std::vector<Blocks>* cols);
// Batched independent products (one level schedule for all); addends[i], if given, is summed into
// product i's columns before its carry propagation (a multiply-add costs no extra level).
std::vector<Radix> radix_mul_many(Engine& e, const std::vector<std::pair<const Radix*, const Radix*>>& ops,
                                  uint32_t nblocks, const std::vector<const Radix*>& addends = {});
// The same products summed into columns and compressed only (each column a sum <= 6, <= 7 at
// position 0, of <= 3 blocks; no carry propagation): the columns' value is the product mod 4^nblocks,
// exactly the product when it fits (non-negative entries cannot wrap below it).  With `excess`,
// full products may be Karatsuba-split: product i then has nblocks + 1 columns summing to the product
// + (*excess)[i] 4^nblocks (a public q <= 2; column nblocks holds at most q), else nblocks columns
// and q = 0.  lim_hi > 0: the columns from hi_from on only compressed to sums <= lim_hi of <= 4 blocks
// (for a consumer that reads them through a wider input).
std::vector<std::vector<Blocks>> radix_mul_many_columns(Engine& e,
                                                        const std::vector<std::pair<const Radix*, const Radix*>>& ops,
                                                        uint32_t nblocks, std::vector<int64_t>* excess = nullptr,
                                                        uint32_t hi_from = 0, uint32_t lim_hi = 0);
// a * b + c (wrapping at nblocks), one carry propagation.
Radix radix_mul_add(Engine& e, const Radix& a, const Radix& b, const Radix& c, uint32_t nblocks);
// a * b + c as compressed columns (each <= 3 blocks summing <= 6), value mod 4^nblocks; no carry
// propagation (a decryption's input)
std::vector<Blocks> radix_mul_add_columns(Engine& e, const Radix& a, const Radix& b, const Radix& c, uint32_t nblocks);
Radix radix_scalar_and(Engine& e, const Radix& a, const BigConst& mask);
Radix radix_scalar_shr(Engine& e, const Radix& a, uint32_t bits);
Radix radix_scalar_shl(Engine& e, const Radix& a, uint32_t bits);
Radix radix_scalar_add(Engine& e, const Radix& a, const BigConst& s);
Radix radix_scalar_mul(Engine& e, const Radix& a, const BigConst& s);
// a * m + c for clear m, c (wrapping), one carry propagation
Radix radix_scalar_mul_add(Engine& e, const Radix& a, const BigConst& m, const BigConst& c);
// floor(a / d) and a mod d for a clear divisor d != 0 of any width (Granlund-Montgomery multiply)
Radix radix_scalar_div(Engine& e, const Radix& a, const BigConst& d);
Radix radix_scalar_rem(Engine& e, const Radix& a, const BigConst& d);
// x mod (2^k_bits - c) for a public pseudo-Mersenne modulus (k_bits even, 2 <= k_bits <= FHE_RADIX_MAX_BITS
// - 2, 0 < c < 2^(k_bits - 2); anything else throws), x of any width: folds x <- (x mod 2^k) + (x >> k) c,
// each a clear-scalar multiply-add of the shrinking high part that reads and leaves unpropagated columns,
// their number fixed from a public bound on x (2^width - 1, or what the blocks' degrees give); then, at
// k + 2 bits, the up to four candidates T - j n propagated side by side and one select (radix.cpp has the
// bound and the exactness argument).  k_bits / 2 clean blocks.  The recording depends on (width, k, c,
// degrees) only.  *folds (optional): the number of folds taken.
Radix radix_rem_pseudo_mersenne(Engine& e, const Radix& a, uint32_t k_bits, const BigConst& c, uint32_t* folds = nullptr);
// The same on a column form (radix_mul_add_columns, biguint_mul_add_columns: value = sum_j sum cols[j] 4^j
// mod 4^nblocks).  The fold is linear, so the first one reads the columns as they are: the columns below
// k_bits / 2 join the fold's own columns unpropagated; a wide or unbootstrapped high part (the signer's) is
// normalized on its own, at half the width, before it meets c.  Columns whose degrees could reach
// 4^nblocks are propagated first (the wrap is part of the value).
Radix radix_rem_pseudo_mersenne_columns(Engine& e, const std::vector<Blocks>& cols, uint32_t nblocks, uint32_t k_bits,
                                        const BigConst& c, uint32_t* folds = nullptr);
// Enc(d) (clean blocks) and clear 256-bit-style words e, k -> (k + e d) mod (2^k_bits - c) without ever
// forming e d: sum_i d_i (e 4^i mod n) + k in columns (every entry a clear multiple of a block of d), then
// radix_rem_pseudo_mersenne_columns' few-block fold.  e, k < n.
Radix radix_scalar_mul_add_rem_pseudo_mersenne(Engine& e, const Radix& d, const BigConst& m, const BigConst& k,
                                               uint32_t k_bits, const BigConst& c, uint32_t* folds = nullptr);
inline Radix radix_scalar_and(Engine& e, const Radix& a, uint64_t mask) { return radix_scalar_and(e, a, BigConst{mask}); }
inline Radix radix_scalar_add(Engine& e, const Radix& a, uint64_t s) { return radix_scalar_add(e, a, BigConst{s}); }
inline Radix radix_scalar_mul(Engine& e, const Radix& a, uint64_t s) { return radix_scalar_mul(e, a, BigConst{s}); }
inline Radix radix_scalar_div(Engine& e, const Radix& a, uint64_t d) { return radix_scalar_div(e, a, BigConst{d}); }
inline Radix radix_scalar_rem(Engine& e, const Radix& a, uint64_t d) { return radix_scalar_rem(e, a, BigConst{d}); }
Radix radix_sub(Engine& e, const Radix& a, const Radix& b);
// floor(a / d), a mod d for an encrypted divisor (d = 0: quotient all ones, remainder a)
std::pair<Radix, Radix> radix_divrem(Engine& e, const Radix& a, const Radix& d);
// encrypted boolean (one block, value 0/1)
Block radix_lt(Engine& e, const Radix& a, const Radix& b);
Radix radix_select(Engine& e, const Block& cond, const Radix& if_true, const Radix& if_false);
Radix radix_min(Engine& e, const Radix& a, const Radix& b);
Radix radix_max(Engine& e, const Radix& a, const Radix& b);
Radix radix_shr(Engine& e, const Radix& a, const Radix& amount);
Radix radix_shl(Engine& e, const Radix& a, const Radix& amount);
Radix radix_bitand(Engine& e, const Radix& a, const Radix& b);
// refresh every block through an identity bootstrap (noise reset)
Radix radix_clean(Engine& e, const Radix& a);

// Collective over the context's communicator (comm.cpp): rank `root` replicates radix integers
// (its `groups`) to every rank device-to-device; on the receivers `groups` is replaced by copies
// whose block ciphertexts and metadata (degree, noise, trivial values) equal the root's.
int bcast_radix_groups(fhe_ctx* c, int root, std::vector<Radix>* groups);

}  // namespace fhe
