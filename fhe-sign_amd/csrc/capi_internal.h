// capi_internal.h -- what the files that define C entry points share: the handle types and ownership checks of
// the radix layer (capi_radix.cpp: the device entry points, capi_host.cpp: the host-only hooks), and the two
// exception guards and invalid() that every such file uses.  Private to csrc/.
#pragma once
#include <exception>
#include <new>
#include <string>
#include <vector>

#include "biguint.h"
#include "fhe_rocm.h"

struct fhe_radix {
    fhe::Radix r;
    uint32_t bits = 0;
};

struct fhe_biguint {
    fhe::BigUint v;
};

struct fhe_columns {
    std::vector<fhe::Blocks> cols;
    uint32_t nblocks = 0;
};

namespace fhe {

template <class F>
int guarded(F&& f) {
    try {
        return f();
    } catch (const EngineError& e) {  // carries its status (FHE_ERR_TIMEOUT, FHE_ERR_HIP)
        set_error(e.what());
        return e.code;
    } catch (const std::exception& e) {
        set_error(e.what());
        return FHE_ERR_INVALID;
    }
}

// The entry points outside the radix layer (keys, lists, hooks): an allocation that fails is FHE_ERR_ALLOC there.
// Kept apart from guarded(): a radix entry point answers FHE_ERR_INVALID on bad_alloc, and keeps doing so.
template <class F>
int guarded_alloc(F&& f) {
    try {
        return f();
    } catch (const std::bad_alloc&) {
        set_error("out of memory");
        return FHE_ERR_ALLOC;
    } catch (const std::exception& e) {
        set_error(e.what());
        return FHE_ERR_INVALID;
    }
}

inline int invalid(const std::string& why) {
    set_error(why);
    return FHE_ERR_INVALID;
}

// Ownership at the C boundary (Engine::check_owner): every entry point that takes a context and a handle asks
// this of each handle first, under its operand's name, so that a value made under another context is refused
// before the entry point allocates, records or reads anything.  The engine repeats the check where blocks enter
// it; this one names the operand.  FHE_OK, or FHE_ERR_INVALID with the error text set.
inline int owned(const fhe_ctx* c, const Blocks& blocks, const char* operand) {
    if (!c || !c->engine) return FHE_OK;  // no engine to own anything: the entry point's own checks refuse
    for (const Block& b : blocks)
        if (!c->engine->owns(b)) {
            set_error(std::string("operand ") + operand + " was made under another context");
            return FHE_ERR_INVALID;
        }
    return FHE_OK;
}
inline int owned(const fhe_ctx* c, const std::vector<Blocks>& cols, const char* operand) {
    for (const Blocks& col : cols)
        if (const int rc = owned(c, col, operand)) return rc;
    return FHE_OK;
}
inline int owned(const fhe_ctx* c, const fhe_radix* x, const char* operand) { return owned(c, x->r.blocks, operand); }
inline int owned(const fhe_ctx* c, const fhe_biguint* x, const char* operand) {
    for (const Radix& d : x->v.digits)
        if (const int rc = owned(c, d.blocks, operand)) return rc;
    if (x->v.product_cols)
        if (const int rc = owned(c, *x->v.product_cols, operand)) return rc;
    if (x->v.sum_cols)
        if (const int rc = owned(c, *x->v.sum_cols, operand)) return rc;
    return FHE_OK;
}
inline int owned(const fhe_ctx* c, const fhe_columns* x, const char* operand) { return owned(c, x->cols, operand); }

inline BigConst words_of(const uint64_t* s, size_t nwords) { return BigConst(s, s + nwords); }

// the blocks of a column form, for Engine::flush_for
inline std::vector<const Block*> col_blocks(const std::vector<Blocks>& cols) {
    std::vector<const Block*> v;
    for (const Blocks& col : cols)
        for (const Block& b : col)
            if (!b.trivial()) v.push_back(&b);
    return v;
}

// sum_j sum cols[j] 4^j mod 4^nblocks into words (LSB first), each column entry's value from val():
// trivial blocks as they are, lazy blocks as their linear combination of slot blocks
template <class V>
void column_value(const std::vector<Blocks>& cols, uint32_t nblocks, V&& val, uint64_t* words, size_t nwords) {
    std::vector<uint64_t> acc((2 * (size_t)nblocks + 63) / 64 + 2, 0);
    auto add_at = [&](uint32_t j, int64_t v) {  // acc += v 4^j (every entry's value is >= 0)
        engine_check(v >= 0, "column value below zero");
        unsigned __int128 add = (unsigned __int128)(uint64_t)v << ((2 * j) % 64);
        uint64_t carry = 0;
        for (size_t w = (2 * (size_t)j) / 64; w < acc.size() && (add || carry); ++w) {
            const unsigned __int128 s2 = (unsigned __int128)acc[w] + (uint64_t)add + carry;
            acc[w] = (uint64_t)s2;
            carry = (uint64_t)(s2 >> 64);
            add >>= 64;
        }
    };
    for (uint32_t j = 0; j < nblocks && j < cols.size(); ++j) {
        int64_t v = 0;
        for (const Block& b : cols[j]) {
            if (b.trivial()) {
                v += b.value;
            } else if (b.lazy()) {
                v += b.lin_cst;
                for (const Term& t : *b.lin) v += (int64_t)t.coef * val(t.b);
            } else {
                v += val(b);
            }
        }
        add_at(j, v);
    }
    const uint32_t bits = 2 * nblocks;
    for (size_t w = 0; w < nwords; ++w) {
        uint64_t x = w < acc.size() ? acc[w] : 0;
        if (64 * w >= bits) x = 0;
        else if (64 * (w + 1) > bits) x &= (bits % 64) ? ((1ull << (bits % 64)) - 1) : ~0ull;
        words[w] = x;
    }
}

}  // namespace fhe
