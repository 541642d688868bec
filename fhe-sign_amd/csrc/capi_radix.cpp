// capi_radix.cpp -- C ABI for radix integers (FheUint<N>) and BigUintFHE.
#include <algorithm>
#include <cstring>
#include <unordered_map>
#include <unordered_set>
#include <memory>
#include <string>
#include <stdexcept>

#include <future>

#include "capi_internal.h"
#include "ct_digest.h"
#include "oprf.h"
#include "serial.h"
#include "switched.h"

using namespace fhe;

namespace {

// sim_ok: the entry point runs on a simulated context too (fhe_host_sim_ctx_create: the radix and BigUintFHE
// arithmetic, their encryptions and decryptions); every other one refuses it
// need_rows: the row-level hooks, which take blocks of any message space.  need_engine: every entry point that makes,
// reads or computes on a radix value; on top it asks Params::radix_space() of the installed key, before anything
// is encrypted, recorded or launched (the "LUT table size" check in Engine::run stays as the backstop).
int need_rows(fhe_ctx* c, bool sim_ok = false) {
    if (!c) {
        set_error("null context");
        return FHE_ERR_INVALID;
    }
    if (!c->has_key || !c->engine) {
        set_error("no server key installed (fhe_set_server_key)");
        return FHE_ERR_NO_KEY;
    }
    if (c->simulated) return sim_ok ? FHE_OK : refuse_simulated(c, "this entry point");
    if (hipSetDevice(c->device) != hipSuccess) {
        set_error("hipSetDevice failed");
        return FHE_ERR_HIP;
    }
    return FHE_OK;
}

int need_engine(fhe_ctx* c, bool sim_ok = false) {
    if (const int rc = need_rows(c, sim_ok)) return rc;
    return radix_space_check(c);
}

uint32_t word_bits(const uint64_t* w, uint32_t bit, uint32_t nbits_total) {
    if (bit >= nbits_total) return 0;
    return (uint32_t)(w[bit / 64] >> (bit % 64)) & 3u;
}

fhe_radix* wrap(Radix r, uint32_t bits) {
    auto* x = new fhe_radix();
    x->r = std::move(r);
    x->bits = bits;
    return x;
}

bool valid_bits(uint32_t bits) { return bits >= 2 && bits <= FHE_RADIX_MAX_BITS && bits % 2 == 0; }

// run a binary op on two radix of equal width
constexpr bool kSimOk = true;

// the decoded values of slot blocks (carry bits included): one download, decrypted on the host.  only_needed:
// launch just the pending bootstraps the blocks depend on (Engine::flush_for).  A simulated context makes the same
// flush and reads the plaintext shadow: nothing is launched, the graph is scheduled; ck is not looked at.
std::vector<int64_t> read_blocks(fhe_ctx* c, const fhe_client_key* ck, const std::vector<const Block*>& enc,
                                 bool only_needed) {
    std::vector<int64_t> vals(enc.size());
    if (c->simulated) {
        if (enc.empty()) return vals;
        c->engine->check_owner(enc);  // before the flush, as download_many's
        if (only_needed)
            c->engine->flush_for(enc);
        else
            c->engine->flush();
        for (size_t i = 0; i < enc.size(); ++i) {
            const int64_t h2 = c->engine->sim_half2(*enc[i]);
            engine_check(h2 % 2 == 0 && h2 >= 0 && h2 < 2 * (int64_t)c->p.msg_carry(), "sim: a decrypted block off its message range");
            vals[i] = h2 / 2;
        }
        return vals;
    }
    if (c->client_resident(ck)) {  // the phases on the device, 8 bytes per block back (Engine::phases_many)
        std::vector<uint64_t> phases(enc.size());
        c->engine->phases_many(enc, phases.data(), only_needed);
        for (size_t i = 0; i < enc.size(); ++i) vals[i] = (int64_t)decode_block(ck->params, phases[i]);
        return vals;
    }
    std::vector<uint64_t> cts(enc.size() * kBigCt);
    c->engine->download_many(enc, cts.data(), only_needed);
    for (size_t i = 0; i < enc.size(); ++i)
        vals[i] = (int64_t)decode_block(ck->params, decrypt_phase_big(ck, cts.data() + i * kBigCt));
    return vals;
}

// the device path of a batch of client encryptions: taken when ck is the context's resident key and the batch
// stays in the stream's counter epoch; otherwise false, and the caller's host path runs as ever
bool encrypt_resident(fhe_ctx* c, fhe_client_key* ck, const std::vector<uint64_t>& pts, Blocks* out) {
    return c->client_resident(ck) && c->engine->encrypt_resident(ck, pts.data(), pts.size(), out);
}

// nblocks client-encrypted blocks of the given 2-bit digits; a simulated context makes sim_blocks of them
Blocks encrypt_digits(fhe_ctx* c, fhe_client_key* ck, const std::vector<uint32_t>& digits) {
    Blocks out;
    if (c->simulated) {
        for (uint32_t v : digits) out.push_back(c->engine->sim_block(v, 3));
        return out;
    }
    std::vector<uint64_t> pts(digits.size());
    for (size_t k = 0; k < digits.size(); ++k) pts[k] = (uint64_t)digits[k] * ck->params.delta();
    if (encrypt_resident(c, ck, pts, &out)) return out;
    std::vector<uint64_t> ct(digits.size() * kBigCt);
    encrypt_big_many(ck, pts.data(), pts.size(), ct.data());
    return c->engine->upload_many(ct.data(), digits.size(), 3);
}

template <class F>
int binop(fhe_ctx* c, const fhe_radix* a, const fhe_radix* b, fhe_radix** out, F&& f) {
    int rc = need_engine(c, kSimOk);
    if (rc) return rc;
    if (!a || !b || !out) return FHE_ERR_INVALID;
    if (a->bits != b->bits) {
        set_error("operands must have the same bit width");
        return FHE_ERR_INVALID;
    }
    if ((rc = owned(c, a, "a")) || (rc = owned(c, b, "b"))) return rc;
    return guarded([&] {
        *out = wrap(f(*c->engine, a->r, b->r), a->bits);
        return FHE_OK;
    });
}

template <class F>
int unop(fhe_ctx* c, const fhe_radix* a, fhe_radix** out, F&& f) {
    int rc = need_engine(c, kSimOk);
    if (rc) return rc;
    if (!a || !out) return FHE_ERR_INVALID;
    if ((rc = owned(c, a, "a"))) return rc;
    return guarded([&] {
        *out = wrap(f(*c->engine, a->r), a->bits);
        return FHE_OK;
    });
}

}  // namespace

namespace fhe {
void engine_eager_next_batch(fhe_ctx* c, bool on) {
    if (c && c->engine) c->engine->eager_next_batch(on);
}

void engine_cancel_deferred(fhe_ctx* c) {
    if (c && c->engine) c->engine->cancel_deferred();
}

int biguint_owned(const fhe_ctx* c, const fhe_biguint* x, const char* operand) { return x ? owned(c, x, operand) : FHE_OK; }

// several BigUintFHE encryptions as one batch -- one pass of encrypt_big_many (its host threads over the
// whole batch) and one upload: ciphertexts and encryption-stream state identical to encrypting the
// operands one after the other (the signer's e_fhe and k_fhe)
int biguint_encrypt_batch(fhe_ctx* c, fhe_client_key* ck, const std::vector<const std::vector<uint32_t>*>& limbs,
                          fhe_biguint** outs, bool deferred) {
    int rc = need_engine(c, kSimOk);
    if (rc) return rc;
    if ((!ck && !c->simulated) || !outs) return FHE_ERR_INVALID;
    return guarded([&] {
        size_t total = 0;
        for (auto* l : limbs) total += l->size();
        std::vector<uint32_t> digits;
        digits.reserve(total * kLimbBlocks);
        for (auto* l : limbs)
            for (uint32_t x : *l)
                for (uint32_t k = 0; k < kLimbBlocks; ++k) digits.push_back((x >> (2 * k)) & 3u);
        std::vector<uint64_t> pts;
        if (!c->simulated)
            for (uint32_t v : digits) pts.push_back((uint64_t)v * ck->params.delta());
        Blocks all;
        if (c->simulated) {  // shadowed blocks of the digits, at once: there is no encryption to overlap
            all = encrypt_digits(c, ck, digits);
        } else if (encrypt_resident(c, ck, pts, &all)) {
            // a resident client key: encrypted on the context's stream, nothing to hide behind a helper thread --
            // none is started and no deferred upload is armed
        } else if (deferred) {
            // the encryption runs on a helper thread while the caller records the graph that reads the
            // blocks; the engine uploads them right before its next launch (Engine::upload_deferred)
            // The future is owned by the upload's closure alone, and a std::async future joins its thread when
            // it is released: whether the closure runs, throws or is cancelled (Engine::cancel_deferred, which
            // every exit of the signer goes through), the thread has run to its end -- the client key's stream
            // is where the finished encryption leaves it -- before the closure is gone.
            struct InFlight {  // fhe_ctx_pending_info's helper count: up here, down as the thread's last statement
                std::shared_ptr<std::atomic<uint32_t>> n;
                explicit InFlight(std::shared_ptr<std::atomic<uint32_t>> c) : n(std::move(c)) { ++*n; }
                ~InFlight() { --*n; }
            };
            auto flight = std::make_shared<InFlight>(c->engine->helper_jobs);
            auto job = std::make_shared<std::future<std::vector<uint64_t>>>(std::async(std::launch::async, [ck, pts, flight]() mutable {
                std::shared_ptr<InFlight> done = std::move(flight);  // released when the thread's work is over
                std::vector<uint64_t> ct(pts.size() * kBigCt);
                encrypt_big_many(ck, pts.data(), pts.size(), ct.data());
                return ct;
            }));
            flight.reset();
            all = c->engine->upload_deferred(pts.size(), 3, [job] { return job->get(); });
        } else {
            std::vector<uint64_t> ct(total * kLimbBlocks * kBigCt);
            encrypt_big_many(ck, pts.data(), pts.size(), ct.data());
            all = c->engine->upload_many(ct.data(), total * kLimbBlocks, 3);
        }
        std::vector<std::unique_ptr<fhe_biguint>> made;
        size_t at = 0;
        for (auto* l : limbs) {
            auto b = std::make_unique<fhe_biguint>();
            for (size_t i = 0; i < l->size(); ++i, at += kLimbBlocks) {
                Radix r;
                r.blocks.assign(all.begin() + at, all.begin() + at + kLimbBlocks);
                b->v.digits.push_back(std::move(r));
            }
            made.push_back(std::move(b));
        }
        for (size_t i = 0; i < made.size(); ++i) outs[i] = made[i].release();
        return FHE_OK;
    });
}
}  // namespace fhe

extern "C" {

int fhe_radix_encrypt(fhe_ctx* c, fhe_client_key* ck, const uint64_t* words, uint32_t bits, fhe_radix** out) {
    int rc = need_engine(c, kSimOk);
    if (rc) return rc;
    if ((!ck && !c->simulated) || !words || !out || !valid_bits(bits)) {
        set_error("invalid arguments to fhe_radix_encrypt");
        return FHE_ERR_INVALID;
    }
    return guarded([&] {
        Radix r;
        std::vector<uint32_t> digits(bits / 2);
        for (uint32_t k = 0; k < bits / 2; ++k) digits[k] = word_bits(words, 2 * k, bits);
        r.blocks = encrypt_digits(c, ck, digits);
        *out = wrap(std::move(r), bits);
        return FHE_OK;
    });
}

int fhe_radix_trivial(fhe_ctx* c, const uint64_t* words, uint32_t bits, fhe_radix** out) {
    if (!c || !words || !out || !valid_bits(bits)) return FHE_ERR_INVALID;
    if (const int rc = radix_space_check(c)) return rc;
    Radix r;
    for (uint32_t k = 0; k < bits / 2; ++k) r.blocks.push_back(Block::make_trivial(word_bits(words, 2 * k, bits)));
    *out = wrap(std::move(r), bits);
    return FHE_OK;
}

// the value of a column form (sum_j sum cols[j] 4^j mod 4^nblocks): every slot block (lazy entries:
// their terms) in one download, decrypted on the host.  only_needed: launch just the pending bootstraps
// the blocks depend on (Engine::flush_for)
static void decrypt_columns(fhe_ctx* c, const fhe_client_key* ck, const std::vector<Blocks>& cols, uint32_t nblocks,
                            uint64_t* words, size_t nwords, bool only_needed) {
    std::vector<const Block*> enc;
    std::vector<const uint64_t*> keys;
    std::unordered_set<const uint64_t*> seen;
    auto want = [&](const Block& b) {
        if (!seen.insert(b.ptr()).second) return;
        keys.push_back(b.ptr());
        enc.push_back(&b);
    };
    for (const Blocks& col : cols)
        for (const Block& b : col) {
            if (b.trivial()) continue;
            if (b.lazy())
                for (const Term& t : *b.lin) want(t.b);
            else
                want(b);
        }
    const std::vector<int64_t> got = read_blocks(c, ck, enc, only_needed);
    std::unordered_map<const uint64_t*, int64_t> vals;
    for (size_t i = 0; i < enc.size(); ++i) vals[keys[i]] = got[i];
    column_value(cols, nblocks, [&](const Block& b) { return vals.at(b.ptr()); }, words, nwords);
}

// the decoded values of a radix's blocks (carry bits included): trivial blocks as they are, the
// others downloaded together and decrypted on the host
static std::vector<uint32_t> decrypt_blocks(fhe_ctx* c, const fhe_client_key* ck, const Radix& r) {
    std::vector<uint32_t> vals(r.nblocks());
    std::vector<const Block*> enc;
    for (uint32_t k = 0; k < r.nblocks(); ++k) {
        if (r.blocks[k].trivial())
            vals[k] = r.blocks[k].value;
        else
            enc.push_back(&r.blocks[k]);
    }
    const std::vector<int64_t> got = read_blocks(c, ck, enc, false);
    for (size_t i = 0, k = 0; k < r.nblocks(); ++k)
        if (!r.blocks[k].trivial()) vals[k] = (uint32_t)got[i++];
    return vals;
}

int fhe_radix_decrypt(fhe_ctx* c, const fhe_client_key* ck, const fhe_radix* x, uint64_t* words, size_t nwords) {
    int rc = need_engine(c, kSimOk);
    if (rc) return rc;
    if ((!ck && !c->simulated) || !x || !words || nwords * 64 < x->bits) {
        set_error("invalid arguments to fhe_radix_decrypt");
        return FHE_ERR_INVALID;
    }
    if ((rc = owned(c, x, "x"))) return rc;
    return guarded([&] {
        std::memset(words, 0, nwords * 8);
        // value = sum v_k 4^k mod 2^bits (v_k incl. carry bits)
        unsigned __int128 lo = 0;  // bits < 128 handled by accumulating per block
        const std::vector<uint32_t> vals = decrypt_blocks(c, ck, x->r);
        // big-integer accumulate in 64-bit words
        std::vector<uint64_t> acc((x->bits + 63) / 64 + 2, 0);
        for (uint32_t k = 0; k < vals.size(); ++k) {
            unsigned __int128 add = vals[k];
            uint32_t bit = 2 * k;
            size_t w = bit / 64;
            add <<= (bit % 64);
            while (add && w < acc.size()) {
                unsigned __int128 s = (unsigned __int128)acc[w] + (uint64_t)add;
                acc[w] = (uint64_t)s;
                add = (add >> 64) + (s >> 64);
                ++w;
            }
        }
        (void)lo;
        for (size_t w = 0; w < nwords && w < acc.size(); ++w) words[w] = acc[w];
        // wrap mod 2^bits
        const uint32_t top = x->bits;
        for (size_t w = 0; w < nwords; ++w) {
            const uint32_t lo_bit = (uint32_t)w * 64;
            if (lo_bit >= top)
                words[w] = 0;
            else if (top - lo_bit < 64)
                words[w] &= (1ull << (top - lo_bit)) - 1;
        }
        return FHE_OK;
    });
}

int fhe_radix_num_bits(const fhe_radix* x, uint32_t* bits) {
    if (!x || !bits) return FHE_ERR_INVALID;
    *bits = x->bits;
    return FHE_OK;
}

int fhe_radix_clone(const fhe_radix* x, fhe_radix** out) {
    if (!x || !out) return FHE_ERR_INVALID;
    *out = new fhe_radix(*x);
    return FHE_OK;
}

void fhe_radix_destroy(fhe_radix* x) { delete x; }

int fhe_radix_export(fhe_ctx* c, const fhe_radix* x, uint64_t* cts, size_t nwords) {
    int rc = need_engine(c);
    if (rc) return rc;
    if (!x || !cts || nwords < (size_t)x->r.nblocks() * kBigCt) return FHE_ERR_INVALID;
    if ((rc = owned(c, x, "x"))) return rc;
    return guarded([&] {
        std::vector<const Block*> enc;
        for (uint32_t k = 0; k < x->r.nblocks(); ++k) {
            uint64_t* ct = cts + (size_t)k * kBigCt;
            const Block& b = x->r.blocks[k];
            if (b.trivial()) {
                std::memset(ct, 0, kBigCt * 8);
                ct[kBigDim] = (uint64_t)b.value * c->p.delta();
            } else {
                enc.push_back(&b);
            }
        }
        std::vector<uint64_t> buf(enc.size() * kBigCt);
        c->engine->download_many(enc, buf.data());
        for (size_t i = 0, k = 0; k < x->r.nblocks(); ++k)
            if (!x->r.blocks[k].trivial()) std::memcpy(cts + (size_t)k * kBigCt, buf.data() + kBigCt * i++, kBigCt * 8);
        return FHE_OK;
    });
}

int fhe_radix_add(fhe_ctx* c, const fhe_radix* a, const fhe_radix* b, fhe_radix** out) {
    return binop(c, a, b, out, [](Engine& e, const Radix& x, const Radix& y) { return radix_sum(e, {&x, &y}, x.nblocks()); });
}
int fhe_radix_sub(fhe_ctx* c, const fhe_radix* a, const fhe_radix* b, fhe_radix** out) {
    return binop(c, a, b, out, [](Engine& e, const Radix& x, const Radix& y) { return radix_sub(e, x, y); });
}
int fhe_radix_mul(fhe_ctx* c, const fhe_radix* a, const fhe_radix* b, fhe_radix** out) {
    return binop(c, a, b, out, [](Engine& e, const Radix& x, const Radix& y) { return radix_mul(e, x, y, x.nblocks()); });
}
int fhe_radix_min(fhe_ctx* c, const fhe_radix* a, const fhe_radix* b, fhe_radix** out) {
    return binop(c, a, b, out, [](Engine& e, const Radix& x, const Radix& y) { return radix_min(e, x, y); });
}
int fhe_radix_max(fhe_ctx* c, const fhe_radix* a, const fhe_radix* b, fhe_radix** out) {
    return binop(c, a, b, out, [](Engine& e, const Radix& x, const Radix& y) { return radix_max(e, x, y); });
}
int fhe_radix_bitand(fhe_ctx* c, const fhe_radix* a, const fhe_radix* b, fhe_radix** out) {
    return binop(c, a, b, out, [](Engine& e, const Radix& x, const Radix& y) { return radix_bitand(e, x, y); });
}
int fhe_radix_lt(fhe_ctx* c, const fhe_radix* a, const fhe_radix* b, fhe_radix** out) {
    int rc = binop(c, a, b, out, [](Engine& e, const Radix& x, const Radix& y) {
        Radix r;
        r.blocks = {radix_lt(e, x, y)};
        return r;
    });
    if (rc == FHE_OK) (*out)->bits = 2;
    return rc;
}
int fhe_radix_divrem(fhe_ctx* c, const fhe_radix* a, const fhe_radix* b, fhe_radix** q, fhe_radix** r) {
    int rc = need_engine(c, kSimOk);
    if (rc) return rc;
    if (!a || !b || (!q && !r)) return FHE_ERR_INVALID;
    if (a->bits != b->bits) {
        set_error("operands must have the same bit width");
        return FHE_ERR_INVALID;
    }
    if ((rc = owned(c, a, "a")) || (rc = owned(c, b, "b"))) return rc;
    return guarded([&] {
        auto qr = radix_divrem(*c->engine, a->r, b->r);
        if (q) *q = wrap(std::move(qr.first), a->bits);
        if (r) *r = wrap(std::move(qr.second), a->bits);
        return FHE_OK;
    });
}
int fhe_radix_div(fhe_ctx* c, const fhe_radix* a, const fhe_radix* b, fhe_radix** out) {
    return fhe_radix_divrem(c, a, b, out, nullptr);
}
int fhe_radix_rem(fhe_ctx* c, const fhe_radix* a, const fhe_radix* b, fhe_radix** out) {
    return fhe_radix_divrem(c, a, b, nullptr, out);
}
int fhe_radix_shr(fhe_ctx* c, const fhe_radix* a, const fhe_radix* amount, fhe_radix** out) {
    int rc = need_engine(c, kSimOk);
    if (rc) return rc;
    if (!a || !amount || !out) return FHE_ERR_INVALID;
    if ((rc = owned(c, a, "a")) || (rc = owned(c, amount, "amount"))) return rc;
    return guarded([&] {
        *out = wrap(radix_shr(*c->engine, a->r, amount->r), a->bits);
        return FHE_OK;
    });
}
int fhe_radix_shl(fhe_ctx* c, const fhe_radix* a, const fhe_radix* amount, fhe_radix** out) {
    int rc = need_engine(c, kSimOk);
    if (rc) return rc;
    if (!a || !amount || !out) return FHE_ERR_INVALID;
    if ((rc = owned(c, a, "a")) || (rc = owned(c, amount, "amount"))) return rc;
    return guarded([&] {
        *out = wrap(radix_shl(*c->engine, a->r, amount->r), a->bits);
        return FHE_OK;
    });
}
int fhe_radix_scalar_and(fhe_ctx* c, const fhe_radix* a, uint64_t mask, fhe_radix** out) {
    return unop(c, a, out, [mask](Engine& e, const Radix& x) { return radix_scalar_and(e, x, mask); });
}
int fhe_radix_scalar_shr(fhe_ctx* c, const fhe_radix* a, uint32_t shift, fhe_radix** out) {
    if (!a) return FHE_ERR_INVALID;
    const uint32_t s = shift % a->bits;  // tfhe: shift amount taken modulo the bit width
    return unop(c, a, out, [s](Engine& e, const Radix& x) { return radix_scalar_shr(e, x, s); });
}
int fhe_radix_scalar_shl(fhe_ctx* c, const fhe_radix* a, uint32_t shift, fhe_radix** out) {
    if (!a) return FHE_ERR_INVALID;
    const uint32_t s = shift % a->bits;
    return unop(c, a, out, [s](Engine& e, const Radix& x) { return radix_scalar_shl(e, x, s); });
}
int fhe_radix_scalar_add(fhe_ctx* c, const fhe_radix* a, uint64_t s, fhe_radix** out) {
    return unop(c, a, out, [s](Engine& e, const Radix& x) { return radix_scalar_add(e, x, s); });
}
int fhe_radix_scalar_mul(fhe_ctx* c, const fhe_radix* a, uint64_t s, fhe_radix** out) {
    return unop(c, a, out, [s](Engine& e, const Radix& x) { return radix_scalar_mul(e, x, s); });
}
int fhe_radix_scalar_div(fhe_ctx* c, const fhe_radix* a, uint64_t d, fhe_radix** out) {
    if (d == 0) {
        set_error("division by zero");
        return FHE_ERR_INVALID;
    }
    return unop(c, a, out, [d](Engine& e, const Radix& x) { return radix_scalar_div(e, x, d); });
}
int fhe_radix_scalar_rem(fhe_ctx* c, const fhe_radix* a, uint64_t d, fhe_radix** out) {
    if (d == 0) {
        set_error("division by zero");
        return FHE_ERR_INVALID;
    }
    return unop(c, a, out, [d](Engine& e, const Radix& x) { return radix_scalar_rem(e, x, d); });
}
// ---- wide clear operands (little-endian u64 words)
int fhe_radix_scalar_and_words(fhe_ctx* c, const fhe_radix* a, const uint64_t* s, size_t nwords, fhe_radix** out) {
    if (!s && nwords) return FHE_ERR_INVALID;
    const BigConst v = words_of(s, nwords);
    return unop(c, a, out, [&v](Engine& e, const Radix& x) { return radix_scalar_and(e, x, v); });
}
int fhe_radix_scalar_add_words(fhe_ctx* c, const fhe_radix* a, const uint64_t* s, size_t nwords, fhe_radix** out) {
    if (!s && nwords) return FHE_ERR_INVALID;
    const BigConst v = words_of(s, nwords);
    return unop(c, a, out, [&v](Engine& e, const Radix& x) { return radix_scalar_add(e, x, v); });
}
int fhe_radix_scalar_mul_words(fhe_ctx* c, const fhe_radix* a, const uint64_t* s, size_t nwords, fhe_radix** out) {
    if (!s && nwords) return FHE_ERR_INVALID;
    const BigConst v = words_of(s, nwords);
    return unop(c, a, out, [&v](Engine& e, const Radix& x) { return radix_scalar_mul(e, x, v); });
}
int fhe_radix_scalar_mul_add_words(fhe_ctx* c, const fhe_radix* a, const uint64_t* m, size_t nm, const uint64_t* k,
                                   size_t nk, fhe_radix** out) {
    if ((!m && nm) || (!k && nk)) return FHE_ERR_INVALID;
    const BigConst vm = words_of(m, nm), vk = words_of(k, nk);
    return unop(c, a, out, [&](Engine& e, const Radix& x) { return radix_scalar_mul_add(e, x, vm, vk); });
}
static bool all_zero(const uint64_t* s, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (s[i]) return false;
    return true;
}
int fhe_radix_scalar_div_words(fhe_ctx* c, const fhe_radix* a, const uint64_t* d, size_t nwords, fhe_radix** out) {
    if (!d || all_zero(d, nwords)) {
        set_error("division by zero");
        return FHE_ERR_INVALID;
    }
    const BigConst v = words_of(d, nwords);
    return unop(c, a, out, [&v](Engine& e, const Radix& x) { return radix_scalar_div(e, x, v); });
}
int fhe_radix_scalar_rem_words(fhe_ctx* c, const fhe_radix* a, const uint64_t* d, size_t nwords, fhe_radix** out) {
    if (!d || all_zero(d, nwords)) {
        set_error("division by zero");
        return FHE_ERR_INVALID;
    }
    const BigConst v = words_of(d, nwords);
    return unop(c, a, out, [&v](Engine& e, const Radix& x) { return radix_scalar_rem(e, x, v); });
}
int fhe_radix_cast(fhe_ctx* c, const fhe_radix* a, uint32_t bits, fhe_radix** out) {
    if (!a || !out || !valid_bits(bits)) return FHE_ERR_INVALID;
    // no slot is read; with a context, the result is a value of that context, so the operand must be too
    if (const int rc = owned(c, a, "a")) return rc;
    *out = wrap(radix_resize(a->r, bits / 2), bits);
    return FHE_OK;
}
int fhe_ctx_level_log(fhe_ctx* c, uint32_t* sizes, size_t cap, size_t* n, int reset) {
    if (!c || !n || (cap && !sizes)) return FHE_ERR_INVALID;
    if (!c->engine) {
        *n = 0;
        return FHE_OK;
    }
    const std::vector<uint32_t>& log = c->engine->level_log;
    *n = log.size();
    if (cap && !log.empty()) std::memcpy(sizes, log.data(), std::min(cap, log.size()) * 4);
    if (reset) c->engine->level_log.clear();
    return FHE_OK;
}

int fhe_ctx_stats(fhe_ctx* c, uint64_t* pbs, uint64_t* levels) {
    if (!c) return FHE_ERR_INVALID;
    if (pbs) *pbs = c->engine ? c->engine->pbs_count : 0;
    if (levels) *levels = c->engine ? c->engine->levels : 0;
    return FHE_OK;
}

// The noise budget as the engine enforced it since the last reset (Engine::NoiseAudit): the largest label, the
// largest merged noise, and the number of recorded bootstraps whose merged noise exceeds their label.  Device and
// simulated contexts alike; a context without an engine reports zeros.
int fhe_ctx_noise_audit(fhe_ctx* c, uint64_t* max_label, uint64_t* max_merged, uint64_t* n_above_label, int reset) {
    if (!c) return FHE_ERR_INVALID;
    const Engine::NoiseAudit a = c->engine ? c->engine->audit : Engine::NoiseAudit{};
    if (max_label) *max_label = a.max_label;
    if (max_merged) *max_merged = a.max_merged;
    if (n_above_label) *n_above_label = a.n_above_label;
    if (reset && c->engine) c->engine->audit = Engine::NoiseAudit{};
    return FHE_OK;
}

// ----------------------------------------------------------------- launch trace and its read-only hooks
int fhe_ctx_trace(fhe_ctx* c, int enable) {
    if (!c || !c->engine) {
        set_error("fhe_ctx_trace: a context without an engine (no key installed)");
        return FHE_ERR_INVALID;
    }
    c->engine->trace_enable(enable != 0);
    return FHE_OK;
}

int fhe_ctx_trace_read(fhe_ctx* c, uint64_t* buf, size_t cap, size_t* n, int reset) {
    if (!c || !n || (cap && !buf)) return FHE_ERR_INVALID;
    if (!c->engine) {
        *n = 0;
        return FHE_OK;
    }
    Engine& e = *c->engine;
    if (e.trace_overflowed()) {
        *n = 0;
        if (reset) e.trace_reset();
        set_error("fhe_ctx_trace_read: the launch trace overflowed its " + std::to_string(Engine::kTraceCap) +
                  " words and is incomplete");
        return FHE_ERR_INVALID;
    }
    const std::vector<uint64_t>& t = e.trace_words();
    *n = t.size();
    if (cap && !t.empty()) std::memcpy(buf, t.data(), std::min(cap, t.size()) * 8);
    if (reset) e.trace_reset();
    return FHE_OK;
}

// Test hook, read-only: out[0] = pending bootstraps, out[1] = 1 while a deferred upload is armed, out[2] = helper
// jobs (the deferred encryptions' threads) in flight.  A context without an engine reports zeros.
int fhe_ctx_pending_info(fhe_ctx* c, uint64_t out[3]) {
    if (!c || !out) return FHE_ERR_INVALID;
    out[0] = out[1] = out[2] = 0;
    if (!c->engine) return FHE_OK;
    out[0] = c->engine->pending_nodes();
    out[1] = c->engine->deferred_armed() ? 1 : 0;
    out[2] = c->engine->helper_jobs->load();
    return FHE_OK;
}

// addrs[k] = block k's slot address (a simulated context: its placeholder), 0 for a trivial block, whose value
// goes to values[k] (optional; 0 for the others).  A lazy block (an unevaluated combination) has no address.
static int block_addrs(const fhe_ctx* c, const std::vector<const Block*>& blocks, uint64_t* addrs, uint32_t* values,
                       size_t cap, size_t* n) {
    *n = blocks.size();
    if (cap < blocks.size()) {
        if (cap == 0) return FHE_OK;  // a size query
        set_error("block address buffer too small");
        return FHE_ERR_INVALID;
    }
    if (!addrs) return FHE_ERR_INVALID;
    for (size_t k = 0; k < blocks.size(); ++k) {
        const Block& b = *blocks[k];
        if (b.lazy() || (b.trivial() && b.half_neg)) {
            set_error("block_addrs: block " + std::to_string(k) + " is an unevaluated combination, not a slot");
            return FHE_ERR_INVALID;
        }
        addrs[k] = (uint64_t)reinterpret_cast<uintptr_t>(b.ptr());
        if (values) values[k] = b.trivial() ? b.value : 0;
    }
    (void)c;
    return FHE_OK;
}

int fhe_radix_block_addrs(fhe_ctx* c, const fhe_radix* x, uint64_t* addrs, uint32_t* values, size_t cap, size_t* n) {
    if (!c || !x || !n) return FHE_ERR_INVALID;
    if (const int rc = owned(c, x, "x")) return rc;
    std::vector<const Block*> blocks;
    for (const Block& b : x->r.blocks) blocks.push_back(&b);
    return block_addrs(c, blocks, addrs, values, cap, n);
}

int fhe_biguint_block_addrs(fhe_ctx* c, const fhe_biguint* x, uint64_t* addrs, uint32_t* values, size_t cap, size_t* n) {
    if (!c || !x || !n) return FHE_ERR_INVALID;
    if (const int rc = owned(c, x, "x")) return rc;
    std::vector<const Block*> blocks;
    for (const Radix& d : x->v.digits)
        for (const Block& b : d.blocks) blocks.push_back(&b);
    return block_addrs(c, blocks, addrs, values, cap, n);
}

int fhe_ctx_lut_table(fhe_ctx* c, uint32_t id, int* kind, int32_t entries[16]) {
    if (!c || !kind || !entries) return FHE_ERR_INVALID;
    const uint32_t mods = c->p.msg_carry();
    for (const auto& kv : c->lut_ids) {
        if (kv.second != id) continue;
        const std::vector<uint32_t>& key = kv.first;
        std::memset(entries, 0, 16 * sizeof(int32_t));
        if (key.size() == mods && mods <= 16) {
            *kind = FHE_LUT_INTEGER;
            for (uint32_t i = 0; i < mods; ++i) entries[i] = (int32_t)key[i];
        } else if (key.size() == (size_t)mods + 1 && key[0] == 0xFFFFFFFFu && mods <= 16) {
            *kind = FHE_LUT_HALF_STEP;
            for (uint32_t i = 0; i < mods; ++i) entries[i] = (int32_t)key[1 + i];
        } else if (key.size() == 3 && key[0] == 0xFFFFFFFEu) {
            *kind = FHE_LUT_OPRF;
            entries[0] = (int32_t)key[2];
        } else if (mods > 16 && (key.size() == mods || (key.size() == (size_t)mods + 1 && key[0] == 0xFFFFFFFFu))) {
            // entries[] is the radix layer's 16: the hook reads tables of message spaces up to 16 values
            set_error("fhe_ctx_lut_table: a table of " + std::to_string(mods) + " entries (message_modulus * carry_modulus of the " +
                      "installed key); the hook reports at most 16");
            return FHE_ERR_INVALID;
        } else {
            set_error("fhe_ctx_lut_table: a table of no known kind");
            return FHE_ERR_INVALID;
        }
        return FHE_OK;
    }
    set_error("fhe_ctx_lut_table: no table with id " + std::to_string(id));
    return FHE_ERR_INVALID;
}

int fhe_ctx_export_luts(fhe_ctx* c, uint32_t first, uint32_t count, uint64_t* polys) {
    if (const int sim = refuse_simulated(c, "fhe_ctx_export_luts")) return sim;
    if (!c || (count && !polys)) return FHE_ERR_INVALID;
    if (count == 0) return FHE_OK;
    // the device table as it stands: what sync_luts last sent, not the host copy
    if (!c->d_luts || !c->d_luts.fits(((size_t)first + count) * kPolySize)) {
        set_error("fhe_ctx_export_luts: tables beyond the device table");
        return FHE_ERR_INVALID;
    }
    FHE_HIP_CHECK(hipSetDevice(c->device));
    FHE_HIP_CHECK(hipMemcpyAsync(polys, c->d_luts + (size_t)first * kPolySize, (size_t)count * kPolySize * 8,
                                 hipMemcpyDeviceToHost, c->stream));
    FHE_HIP_CHECK(hipStreamSynchronize(c->stream));
    return FHE_OK;
}

// ----------------------------------------------------------------- operand distribution (comm.cpp)
int fhe_ctx_broadcast_radix(fhe_ctx* c, fhe_radix** x, int root) {
    const bool sends = c && (!c->attached() || c->rank == root);
    if (!c || !x || (sends && !*x)) return FHE_ERR_INVALID;
    if (sends)
        if (const int rc = owned(c, *x, "x")) return rc;
    std::vector<Radix> g;
    if (sends) g.push_back((*x)->r);
    const int rc = bcast_radix_groups(c, root, &g);
    if (rc || (c->attached() && c->rank == root)) return rc;  // the root keeps its handle
    if (g.size() != 1) {
        set_error("broadcast_radix: the root sent a BigUintFHE, not one radix integer");
        return FHE_ERR_INVALID;
    }
    const uint32_t bits = 2 * g[0].nblocks();
    *x = wrap(std::move(g[0]), bits);
    return FHE_OK;
}

int fhe_ctx_broadcast_biguint(fhe_ctx* c, fhe_biguint** x, int root) {
    const bool sends = c && (!c->attached() || c->rank == root);
    if (!c || !x || (sends && !*x)) return FHE_ERR_INVALID;
    if (sends)
        if (const int rc = owned(c, *x, "x")) return rc;
    std::vector<Radix> g;
    if (sends) {
        g = (*x)->v.digits;
        (*x)->v.sum_cols.reset();  // the receivers get digits only: every rank decrypts the same way
    }
    const int rc = bcast_radix_groups(c, root, &g);
    if (rc || (c->attached() && c->rank == root)) return rc;
    for (const Radix& d : g)
        if (d.nblocks() != kLimbBlocks) {
            set_error("broadcast_biguint: the root sent digits that are not FheUint32");
            return FHE_ERR_INVALID;
        }
    auto* b = new fhe_biguint();
    b->v.digits = std::move(g);
    *x = b;
    return FHE_OK;
}

// --------------------------------------------------------------------------- BigUintFHE
int fhe_biguint_encrypt(fhe_ctx* c, fhe_client_key* ck, const uint32_t* limbs, size_t n, fhe_biguint** out) {
    if (n && !limbs) return FHE_ERR_INVALID;
    const std::vector<uint32_t> l(limbs, limbs + n);
    return fhe::biguint_encrypt_batch(c, ck, {&l}, out);
}

int fhe_biguint_from_digits(const fhe_radix* const* digits, size_t n, fhe_biguint** out) {
    if (!out || (n && !digits)) return FHE_ERR_INVALID;
    auto* b = new fhe_biguint();
    for (size_t i = 0; i < n; ++i) {
        if (!digits[i] || digits[i]->bits != 32) {
            delete b;
            set_error("BigUintFHE digits must be FheUint32");
            return FHE_ERR_INVALID;
        }
        b->v.digits.push_back(digits[i]->r);
    }
    *out = b;
    return FHE_OK;
}

int fhe_biguint_decrypt(fhe_ctx* c, const fhe_client_key* ck, const fhe_biguint* x, uint32_t* limbs, size_t cap,
                        size_t* n) {
    int rc = need_engine(c, kSimOk);
    if (rc) return rc;
    if ((!ck && !c->simulated) || !x || !n) return FHE_ERR_INVALID;
    if ((rc = owned(c, x, "x"))) return rc;
    *n = x->v.digits.size();
    if (cap < *n || (*n && !limbs)) {
        set_error("limb buffer too small");
        return FHE_ERR_INVALID;
    }
    return guarded([&] {
        if (x->v.sum_cols) {  // a sum: its column form (the digits' carry propagation may stay pending)
            const uint32_t nb = (uint32_t)*n * kLimbBlocks;
            std::vector<uint64_t> w((2 * (size_t)nb + 63) / 64);
            decrypt_columns(c, ck, *x->v.sum_cols, nb, w.data(), w.size(), true);
            for (size_t i = 0; i < *n; ++i) limbs[i] = (uint32_t)(w[i / 2] >> (32 * (i % 2)));
            return FHE_OK;
        }
        // every limb's blocks in one download: limb = sum v_k 4^k mod 2^32
        Radix all;
        for (size_t i = 0; i < *n; ++i) all.blocks.insert(all.blocks.end(), x->v.digits[i].blocks.begin(), x->v.digits[i].blocks.end());
        const std::vector<uint32_t> vals = decrypt_blocks(c, ck, all);
        for (size_t i = 0, k = 0; i < *n; ++i) {
            uint64_t w = 0;
            for (uint32_t j = 0; j < x->v.digits[i].nblocks(); ++j, ++k) w += (uint64_t)vals[k] << (2 * j);
            limbs[i] = (uint32_t)w;
        }
        return FHE_OK;
    });
}

int fhe_biguint_len(const fhe_biguint* x, size_t* n) {
    if (!x || !n) return FHE_ERR_INVALID;
    *n = x->v.digits.size();
    return FHE_OK;
}

int fhe_biguint_digit(const fhe_biguint* x, size_t i, fhe_radix** out) {
    if (!x || !out || i >= x->v.digits.size()) return FHE_ERR_INVALID;
    *out = wrap(x->v.digits[i], 32);
    return FHE_OK;
}

int fhe_biguint_to_radix(const fhe_biguint* x, uint32_t bits, fhe_radix** out) {
    if (!x || !out || !valid_bits(bits)) return FHE_ERR_INVALID;
    return guarded([&] {
        Radix r;
        for (const Radix& d : x->v.digits) r.blocks.insert(r.blocks.end(), d.blocks.begin(), d.blocks.end());
        *out = wrap(radix_resize(r, bits / 2), bits);
        return FHE_OK;
    });
}

int fhe_biguint_clone(const fhe_biguint* x, fhe_biguint** out) {
    if (!x || !out) return FHE_ERR_INVALID;
    *out = new fhe_biguint(*x);
    return FHE_OK;
}

void fhe_biguint_destroy(fhe_biguint* x) { delete x; }

int fhe_biguint_add(fhe_ctx* c, const fhe_biguint* a, const fhe_biguint* b, int mode, fhe_biguint** out) {
    int rc = need_engine(c, kSimOk);
    if (rc) return rc;
    if (!a || !b || !out) return FHE_ERR_INVALID;
    if ((rc = owned(c, a, "a")) || (rc = owned(c, b, "b"))) return rc;
    return guarded([&] {
        auto r = std::make_unique<fhe_biguint>();
        r->v = biguint_add(*c->engine, a->v, b->v, mode);
        *out = r.release();
        return FHE_OK;
    });
}

int fhe_biguint_mul(fhe_ctx* c, const fhe_biguint* a, const fhe_biguint* b, int mode, fhe_biguint** out) {
    int rc = need_engine(c, kSimOk);
    if (rc) return rc;
    if (!a || !b || !out) return FHE_ERR_INVALID;
    if ((rc = owned(c, a, "a")) || (rc = owned(c, b, "b"))) return rc;
    return guarded([&] {
        auto r = std::make_unique<fhe_biguint>();
        r->v = biguint_mul(*c->engine, a->v, b->v, mode);
        *out = r.release();
        return FHE_OK;
    });
}

// k + a * b in column form for decryption (biguint_mul_add_columns): the FHE work of the mode's
// mul-add without its final carry propagation, which the decryption resolves on the host
int fhe_biguint_mul_add_columns(fhe_ctx* c, const fhe_biguint* a, const fhe_biguint* b, const fhe_biguint* k, int mode,
                                fhe_columns** out) {
    int rc = need_engine(c, kSimOk);
    if (rc) return rc;
    if (!a || !b || !k || !out || (mode != kCompat && mode != kFast)) return FHE_ERR_INVALID;
    if ((rc = owned(c, a, "a")) || (rc = owned(c, b, "b")) || (rc = owned(c, k, "k"))) return rc;
    return guarded([&] {
        auto r = std::make_unique<fhe_columns>();
        r->cols = biguint_mul_add_columns(*c->engine, a->v, b->v, k->v, mode, &r->nblocks);
        *out = r.release();
        return FHE_OK;
    });
}

// m * a + k (m, k public words) in column form, value mod 2^(a's bits): the public-operand signer
int fhe_radix_scalar_mul_add_columns(fhe_ctx* c, const fhe_radix* a, const uint64_t* m, size_t nm, const uint64_t* k,
                                     size_t nk, fhe_columns** out) {
    int rc = need_engine(c, kSimOk);
    if (rc) return rc;
    if (!a || !out || (!m && nm) || (!k && nk)) return FHE_ERR_INVALID;
    if ((rc = owned(c, a, "a"))) return rc;
    const BigConst vm = words_of(m, nm), vk = words_of(k, nk);
    return guarded([&] {
        auto r = std::make_unique<fhe_columns>();
        const uint32_t nb = a->r.nblocks();
        r->cols = radix_mul_add_columns(*c->engine, a->r, radix_trivial(vm, nb), radix_trivial(vk, nb), nb);
        r->nblocks = nb;
        *out = r.release();
        return FHE_OK;
    });
}

int fhe_columns_bits(const fhe_columns* x, uint32_t* bits) {
    if (!x || !bits) return FHE_ERR_INVALID;
    *bits = 2 * x->nblocks;
    return FHE_OK;
}

int fhe_columns_decrypt(fhe_ctx* c, const fhe_client_key* ck, const fhe_columns* x, uint64_t* words, size_t nwords) {
    int rc = need_engine(c, kSimOk);
    if (rc) return rc;
    if ((!ck && !c->simulated) || !x || !words || nwords * 64 < 2 * (size_t)x->nblocks) {
        set_error("invalid arguments to fhe_columns_decrypt");
        return FHE_ERR_INVALID;
    }
    if ((rc = owned(c, x, "x"))) return rc;
    return guarded([&] {
        decrypt_columns(c, ck, x->cols, x->nblocks, words, nwords, false);
        return FHE_OK;
    });
}

void fhe_columns_destroy(fhe_columns* x) { delete x; }

// x mod (2^k_bits - c), c public words: radix_rem_pseudo_mersenne; the result has k_bits bits
int fhe_radix_rem_pseudo_mersenne(fhe_ctx* c, const fhe_radix* a, uint32_t k_bits, const uint64_t* c_words, size_t nc,
                                  fhe_radix** out) {
    int rc = need_engine(c, kSimOk);
    if (rc) return rc;
    if (!a || !out || !c_words || !nc) {
        set_error("invalid arguments to fhe_radix_rem_pseudo_mersenne");
        return FHE_ERR_INVALID;
    }
    if ((rc = owned(c, a, "a"))) return rc;
    const BigConst cc = words_of(c_words, nc);
    return guarded([&] {
        *out = wrap(radix_rem_pseudo_mersenne(*c->engine, a->r, k_bits, cc), k_bits);
        return FHE_OK;
    });
}

// the same on a column form (fhe_biguint_mul_add_columns, fhe_radix_scalar_mul_add_columns): the first
// fold reads the columns unpropagated
int fhe_columns_rem_pseudo_mersenne(fhe_ctx* c, const fhe_columns* x, uint32_t k_bits, const uint64_t* c_words, size_t nc,
                                    fhe_radix** out) {
    int rc = need_engine(c, kSimOk);
    if (rc) return rc;
    if (!x || !out || !c_words || !nc) {
        set_error("invalid arguments to fhe_columns_rem_pseudo_mersenne");
        return FHE_ERR_INVALID;
    }
    if ((rc = owned(c, x, "x"))) return rc;
    const BigConst cc = words_of(c_words, nc);
    return guarded([&] {
        *out = wrap(radix_rem_pseudo_mersenne_columns(*c->engine, x->cols, x->nblocks, k_bits, cc), k_bits);
        return FHE_OK;
    });
}

// (k + m a) mod (2^k_bits - c) for public m, k below the modulus, the product reduced as it is formed
// (radix_scalar_mul_add_rem_pseudo_mersenne)
int fhe_radix_scalar_mul_add_rem_pseudo_mersenne(fhe_ctx* c, const fhe_radix* a, const uint64_t* m, size_t nm,
                                                 const uint64_t* k, size_t nk, uint32_t k_bits, const uint64_t* c_words,
                                                 size_t nc, fhe_radix** out) {
    int rc = need_engine(c, kSimOk);
    if (rc) return rc;
    if (!a || !out || !c_words || !nc || (!m && nm) || (!k && nk)) {
        set_error("invalid arguments to fhe_radix_scalar_mul_add_rem_pseudo_mersenne");
        return FHE_ERR_INVALID;
    }
    if ((rc = owned(c, a, "a"))) return rc;
    const BigConst cc = words_of(c_words, nc), vm = words_of(m, nm), vk = words_of(k, nk);
    return guarded([&] {
        *out = wrap(radix_scalar_mul_add_rem_pseudo_mersenne(*c->engine, a->r, vm, vk, k_bits, cc), k_bits);
        return FHE_OK;
    });
}

int fhe_biguint_mul_add(fhe_ctx* c, const fhe_biguint* a, const fhe_biguint* b, const fhe_biguint* k, int mode,
                        fhe_biguint** out) {
    int rc = need_engine(c, kSimOk);
    if (rc) return rc;
    if (!a || !b || !k || !out) return FHE_ERR_INVALID;
    if ((rc = owned(c, a, "a")) || (rc = owned(c, b, "b")) || (rc = owned(c, k, "k"))) return rc;
    return guarded([&] {
        auto r = std::make_unique<fhe_biguint>();
        r->v = biguint_mul_add(*c->engine, a->v, b->v, k->v, mode);
        *out = r.release();
        return FHE_OK;
    });
}

}  // extern "C"

// ------------------------------------------------------------------------- serialization
// Radix payload: params, u32 bits, u32 blocks, per block u8 tag (0 trivial: u32 value; 1: u32
// degree, u32 noise, 2049 u64 words).  BigUint: params, u32 limbs, then per limb u32 bits + blocks.
namespace {
bool same_params(const Params& a, const Params& b) {
    return a.n == b.n && a.pbs_base_log == b.pbs_base_log && a.ks_base_log == b.ks_base_log &&
           a.ks_level == b.ks_level && a.lwe_noise_log2 == b.lwe_noise_log2 && a.glwe_noise_log2 == b.glwe_noise_log2 &&
           a.message_modulus == b.message_modulus && a.carry_modulus == b.carry_modulus;
}
void put_blocks(ser::Writer& w, fhe_ctx* c, const Radix& r, uint32_t bits) {
    std::vector<uint64_t> ct(kBigCt);
    w.u32(bits);
    w.u32(r.nblocks());
    for (const Block& b : r.blocks) {
        if (b.trivial()) {
            w.u8(0);
            w.u32(b.value);
        } else {
            w.u8(1);
            w.u32(b.degree);
            w.u32(b.noise);
            c->engine->download(b, ct.data());
            w.words(ct.data(), kBigCt);
        }
    }
}
bool get_blocks(ser::Reader& r, fhe_ctx* c, Radix* out, uint32_t* bits, std::string* why) {
    *bits = r.u32();
    const uint32_t nb = r.u32();
    if (!r.ok || !valid_bits(*bits) || nb != *bits / 2) {
        *why = "malformed radix header";
        return false;
    }
    const uint32_t mc = c->p.msg_carry();
    std::vector<uint64_t> ct(kBigCt);
    for (uint32_t k = 0; k < nb; ++k) {
        const uint8_t tag = r.u8();
        if (tag == 0) {
            const uint32_t v = r.u32();
            if (!r.ok || v >= mc) {
                *why = "malformed trivial block";
                return false;
            }
            out->blocks.push_back(Block::make_trivial(v));
        } else if (tag == 1) {
            const uint32_t degree = r.u32(), noise = r.u32();
            if (!r.ok || degree >= mc || noise == 0 || noise > kMaxNoise || !r.words(ct.data(), kBigCt)) {
                *why = "malformed block (metadata outside the radix layer's degree / noise budget)";
                return false;
            }
            Block b = c->engine->upload(ct.data(), degree);
            b.noise = noise;
            out->blocks.push_back(std::move(b));
        } else {
            *why = "malformed block tag";
            return false;
        }
    }
    return true;
}
}  // namespace

extern "C" {

int fhe_radix_serialize(fhe_ctx* c, const fhe_radix* x, uint8_t* buf, size_t cap, size_t* len) {
    int rc = need_engine(c);
    if (rc) return rc;
    if (!x || !len) return FHE_ERR_INVALID;
    if ((rc = owned(c, x, "x"))) return rc;
    return guarded([&] {
        ser::Writer w;
        w.params(c->p);
        put_blocks(w, c, x->r, x->bits);
        return ser::emit(ser::frame(ser::kRadix, w.b), buf, cap, len);
    });
}

int fhe_radix_deserialize(fhe_ctx* c, const uint8_t* buf, size_t len, fhe_radix** out) {
    int rc = need_engine(c);
    if (rc) return rc;
    if (!out) return FHE_ERR_INVALID;
    return guarded([&] {
        ser::Reader r;
        std::string why;
        Params p;
        if (!ser::unframe(buf, len, ser::kRadix, &r, &why) || !r.params(&p, &why)) {
            set_error(why);
            return FHE_ERR_INVALID;
        }
        if (!same_params(p, c->p)) {
            set_error("ciphertext parameters differ from the context's server key");
            return FHE_ERR_INVALID;
        }
        Radix x;
        uint32_t bits = 0;
        if (!get_blocks(r, c, &x, &bits, &why) || !r.done()) {
            set_error(why.empty() ? "trailing bytes" : why);
            return FHE_ERR_INVALID;
        }
        *out = wrap(std::move(x), bits);
        return FHE_OK;
    });
}

int fhe_biguint_serialize(fhe_ctx* c, const fhe_biguint* x, uint8_t* buf, size_t cap, size_t* len) {
    int rc = need_engine(c);
    if (rc) return rc;
    if (!x || !len) return FHE_ERR_INVALID;
    if ((rc = owned(c, x, "x"))) return rc;
    return guarded([&] {
        ser::Writer w;
        w.params(c->p);
        w.u32((uint32_t)x->v.digits.size());
        for (const Radix& d : x->v.digits) put_blocks(w, c, d, 32);
        return ser::emit(ser::frame(ser::kBigUint, w.b), buf, cap, len);
    });
}

int fhe_biguint_deserialize(fhe_ctx* c, const uint8_t* buf, size_t len, fhe_biguint** out) {
    int rc = need_engine(c);
    if (rc) return rc;
    if (!out) return FHE_ERR_INVALID;
    return guarded([&] {
        ser::Reader r;
        std::string why;
        Params p;
        if (!ser::unframe(buf, len, ser::kBigUint, &r, &why) || !r.params(&p, &why)) {
            set_error(why);
            return FHE_ERR_INVALID;
        }
        if (!same_params(p, c->p)) {
            set_error("ciphertext parameters differ from the context's server key");
            return FHE_ERR_INVALID;
        }
        const uint32_t n = r.u32();
        if (!r.ok || (uint64_t)n * 32 > FHE_RADIX_MAX_BITS * 64ull) {
            set_error("malformed limb count");
            return FHE_ERR_INVALID;
        }
        auto v = std::make_unique<fhe_biguint>();
        for (uint32_t i = 0; i < n; ++i) {
            Radix d;
            uint32_t bits = 0;
            if (!get_blocks(r, c, &d, &bits, &why) || bits != 32) {
                set_error(why.empty() ? "limb is not a 32-bit radix" : why);
                return FHE_ERR_INVALID;
            }
            v->v.digits.push_back(std::move(d));
        }
        if (!r.done()) {
            set_error("trailing bytes");
            return FHE_ERR_INVALID;
        }
        *out = v.release();
        return FHE_OK;
    });
}

}  // extern "C"

// ------------------------------------------------------------------------- seeded ciphertexts
// tfhe-rs' CompressedFheUint: a public mask seed and one body per block (keys.h fhe_seeded); the masks
// are regenerated at expansion, on the host (expand_seeded_host) or on the GPU (Engine::expand_seeded).
// Payload of ser::kSeeded: params, u32 form, u32 count, 32 seed bytes, nblocks u64 bodies.
namespace {
// blocks of a form/count pair; false if the pair is malformed or exceeds the ChaCha counter range
bool seeded_nblocks(uint32_t form, uint32_t count, size_t* nblocks, std::string* why) {
    if (form == FHE_SEEDED_RADIX) {
        if (!valid_bits(count)) {
            *why = "seeded radix: num_bits must be even, >= 2 and <= FHE_RADIX_MAX_BITS";
            return false;
        }
        *nblocks = count / 2;
        return true;
    }
    if (form == FHE_SEEDED_BIGUINT) {
        if ((uint64_t)count * kLimbBlocks > kSeededMaxBlocks) {
            *why = "seeded BigUintFHE: more than 2^24 blocks (the mask stream's 32-bit block counter)";
            return false;
        }
        *nblocks = (size_t)count * kLimbBlocks;
        return true;
    }
    *why = "seeded object: unknown form";
    return false;
}
int seeded_encrypt(fhe_client_key* ck, uint32_t form, uint32_t count, const std::vector<uint64_t>& pts,
                   const uint8_t* mask_seed, fhe_seeded** out) {
    return guarded([&] {
        auto x = std::make_unique<fhe_seeded>();
        x->params = ck->params;
        x->form = form;
        x->count = count;
        if (mask_seed) {
            std::memcpy(x->seed, mask_seed, 32);
        } else {
            if (!os_entropy32(x->seed)) {
                set_error("getrandom failed: no mask seed");
                return FHE_ERR_UNSUPPORTED;
            }
        }
        x->bodies.resize(pts.size());
        encrypt_seeded(ck, x->seed, pts.data(), pts.size(), x->bodies.data());
        *out = x.release();
        return FHE_OK;
    });
}
// the checks of every GPU expansion, before anything is allocated or launched
int seeded_expand_check(fhe_ctx* c, const fhe_seeded* x, uint32_t form) {
    int rc = need_engine(c);
    if (rc) return rc;
    if (!x) return invalid("null seeded object");
    if (x->form != form)
        return invalid(form == FHE_SEEDED_RADIX ? "seeded object holds a BigUintFHE, not a radix integer"
                                                : "seeded object holds a radix integer, not a BigUintFHE");
    const Params &a = x->params, &b = c->p;
    const struct {
        const char* name;
        uint32_t have, want;
    } fields[] = {{"message_modulus", a.message_modulus, b.message_modulus},
                  {"carry_modulus", a.carry_modulus, b.carry_modulus},
                  {"lwe_dimension", a.n, b.n},
                  {"pbs_base_log", a.pbs_base_log, b.pbs_base_log},
                  {"ks_base_log", a.ks_base_log, b.ks_base_log},
                  {"ks_level", a.ks_level, b.ks_level},
                  {"lwe_noise_log2", a.lwe_noise_log2, b.lwe_noise_log2},
                  {"glwe_noise_log2", a.glwe_noise_log2, b.glwe_noise_log2}};
    for (const auto& f : fields)
        if (f.have != f.want)
            return invalid(std::string("seeded object's ") + f.name + " (" + std::to_string(f.have) +
                           ") differs from the context's server key (" + std::to_string(f.want) + ")");
    return FHE_OK;
}
}  // namespace

extern "C" {

int fhe_radix_encrypt_seeded(fhe_client_key* ck, const uint64_t* words, uint32_t bits, const uint8_t* mask_seed,
                             fhe_seeded** out) {
    if (!ck || !words || !out || !valid_bits(bits)) return invalid("invalid arguments to fhe_radix_encrypt_seeded");
    if (!ck->params.radix_space()) return invalid(radix_space_refusal(ck->params, "fhe_radix_encrypt_seeded"));
    std::vector<uint64_t> pts(bits / 2);
    for (uint32_t k = 0; k < bits / 2; ++k) pts[k] = (uint64_t)word_bits(words, 2 * k, bits) * ck->params.delta();
    return seeded_encrypt(ck, FHE_SEEDED_RADIX, bits, pts, mask_seed, out);
}

int fhe_biguint_encrypt_seeded(fhe_client_key* ck, const uint32_t* limbs, size_t n, const uint8_t* mask_seed,
                               fhe_seeded** out) {
    if (!ck || !out || (n && !limbs)) return invalid("invalid arguments to fhe_biguint_encrypt_seeded");
    if (!ck->params.radix_space()) return invalid(radix_space_refusal(ck->params, "fhe_biguint_encrypt_seeded"));
    if (n > kSeededMaxBlocks / kLimbBlocks)
        return invalid("seeded BigUintFHE: more than 2^24 blocks (the mask stream's 32-bit block counter)");
    return guarded([&] {
        std::vector<uint64_t> pts(n * kLimbBlocks);
        for (size_t i = 0; i < n; ++i)
            for (uint32_t k = 0; k < kLimbBlocks; ++k)
                pts[i * kLimbBlocks + k] = (uint64_t)((limbs[i] >> (2 * k)) & 3u) * ck->params.delta();
        return seeded_encrypt(ck, FHE_SEEDED_BIGUINT, (uint32_t)n, pts, mask_seed, out);
    });
}

int fhe_seeded_info(const fhe_seeded* x, uint32_t* form, uint32_t* count, size_t* nblocks) {
    if (!x) return FHE_ERR_INVALID;
    if (form) *form = x->form;
    if (count) *count = x->count;
    if (nblocks) *nblocks = x->bodies.size();
    return FHE_OK;
}

int fhe_seeded_serialize(const fhe_seeded* x, uint8_t* buf, size_t cap, size_t* len) {
    if (!x || !len) return FHE_ERR_INVALID;
    return guarded([&] {
        ser::Writer w;
        w.b.reserve(80 + x->bodies.size() * 8);
        w.params(x->params);
        w.u32(x->form);
        w.u32(x->count);
        w.raw(x->seed, 32);
        w.words(x->bodies.data(), x->bodies.size());
        return ser::emit(ser::frame(ser::kSeeded, w.b), buf, cap, len);
    });
}

int fhe_seeded_deserialize(const uint8_t* buf, size_t len, fhe_seeded** out) {
    if (!out) return FHE_ERR_INVALID;
    return guarded([&] {
        ser::Reader r;
        std::string why;
        Params p;
        if (!ser::unframe(buf, len, ser::kSeeded, &r, &why) || !r.params(&p, &why)) return invalid(why);
        if (!p.radix_space()) return invalid(radix_space_refusal(p, "seeded object"));
        const uint32_t form = r.u32(), count = r.u32();
        size_t nblocks = 0;
        if (!r.ok) return invalid("truncated seeded header");
        if (!seeded_nblocks(form, count, &nblocks, &why)) return invalid(why);
        // the length first: nothing is allocated for a count the payload does not back
        if (r.n - r.off != 32 + nblocks * 8) return invalid("seeded object: block count inconsistent with the payload length");
        auto x = std::make_unique<fhe_seeded>();
        x->params = p;
        x->form = form;
        x->count = count;
        r.take(x->seed, 32);
        x->bodies.resize(nblocks);
        if (!r.words(x->bodies.data(), nblocks) || !r.done()) return invalid("malformed seeded object");
        *out = x.release();
        return FHE_OK;
    });
}

int fhe_seeded_expand_host(const fhe_seeded* x, uint64_t* cts, size_t nwords) {
    if (!x || (!cts && !x->bodies.empty()) || nwords < x->bodies.size() * kBigCt)
        return invalid("invalid arguments to fhe_seeded_expand_host (nblocks x 2049 words)");
    return guarded([&] {
        expand_seeded_host(x->seed, x->bodies.data(), x->bodies.size(), cts);
        return FHE_OK;
    });
}

int fhe_seeded_expand_radix(fhe_ctx* c, const fhe_seeded* x, fhe_radix** out) {
    int rc = seeded_expand_check(c, x, FHE_SEEDED_RADIX);
    if (rc) return rc;
    if (!out) return FHE_ERR_INVALID;
    return guarded([&] {
        Radix r;
        r.blocks = c->engine->expand_seeded(x->seed, x->bodies.data(), x->bodies.size());
        *out = wrap(std::move(r), x->count);
        return FHE_OK;
    });
}

int fhe_seeded_expand_biguint(fhe_ctx* c, const fhe_seeded* x, fhe_biguint** out) {
    int rc = seeded_expand_check(c, x, FHE_SEEDED_BIGUINT);
    if (rc) return rc;
    if (!out) return FHE_ERR_INVALID;
    return guarded([&] {
        const Blocks all = c->engine->expand_seeded(x->seed, x->bodies.data(), x->bodies.size());
        auto v = std::make_unique<fhe_biguint>();
        for (size_t at = 0; at < all.size(); at += kLimbBlocks) {
            Radix d;
            d.blocks.assign(all.begin() + at, all.begin() + at + kLimbBlocks);
            v->v.digits.push_back(std::move(d));
        }
        *out = v.release();
        return FHE_OK;
    });
}

void fhe_seeded_destroy(fhe_seeded* x) { delete x; }

}  // extern "C"

// ------------------------------------------------------------------------- compressed computed ciphertexts
// tfhe-rs' CompressedCiphertextList of one value (compress.h): the device ends of it.  The host ends
// (parameters, keys, fhe_compress_host, the wire kind, fhe_compressed_decrypt) are in compress_host.cpp.
namespace {
int compress_blocks(fhe_ctx* c, const std::vector<const Block*>& blocks, uint32_t form, uint32_t count,
                    fhe_compressed_list** out) {
    if (!c->has_comp) {
        set_error("no compression key installed (fhe_set_compression_key)");
        return FHE_ERR_NO_KEY;
    }
    return guarded([&] {
        auto x = std::make_unique<fhe_compressed_list>();
        x->params = c->p;
        x->cp = c->cp;
        x->form = form;
        x->count = count;
        for (const Block* b : blocks) {
            engine_check(b->degree < c->p.msg_carry(), "compress: block degree >= message_modulus * carry_modulus");
            x->degrees.push_back((uint8_t)b->degree);
        }
        x->packed.resize(c->cp.packed_bytes(blocks.size()));
        c->engine->compress(blocks, x->packed.data());
        *out = x.release();
        return FHE_OK;
    });
}
int compressed_expand_check(fhe_ctx* c, const fhe_compressed_list* x, uint32_t form, bool rows = false) {
    int rc = rows ? need_rows(c) : need_engine(c);
    if (rc) return rc;
    if (!x) return invalid("null compressed list");
    if (!c->has_comp) {
        set_error("no compression key installed (fhe_set_compression_key)");
        return FHE_ERR_NO_KEY;
    }
    if (x->form != form)
        return invalid(form == FHE_SEEDED_RADIX ? "compressed list holds a BigUintFHE, not a radix integer"
                                                : "compressed list holds a radix integer, not a BigUintFHE");
    uint32_t have = 0, want = 0;
    if (const char* f = params_differ(x->params, c->p, &have, &want))
        return invalid(std::string("compressed list's ") + f + " (" + std::to_string(have) +
                       ") differs from the context's server key (" + std::to_string(want) + ")");
    if (!(x->cp == c->cp)) return invalid("compressed list's compression parameters differ from the installed compression key's");
    return FHE_OK;
}
}  // namespace

extern "C" {

int fhe_radix_compress(fhe_ctx* c, const fhe_radix* x, fhe_compressed_list** out) {
    int rc = need_engine(c);
    if (rc) return rc;
    if (!x || !out) return invalid("null argument to fhe_radix_compress");
    if ((rc = owned(c, x, "x"))) return rc;
    std::vector<const Block*> blocks;
    for (const Block& b : x->r.blocks) blocks.push_back(&b);
    return compress_blocks(c, blocks, FHE_SEEDED_RADIX, x->bits, out);
}

int fhe_biguint_compress(fhe_ctx* c, const fhe_biguint* x, fhe_compressed_list** out) {
    int rc = need_engine(c);
    if (rc) return rc;
    if (!x || !out) return invalid("null argument to fhe_biguint_compress");
    if ((rc = owned(c, x, "x"))) return rc;
    std::vector<const Block*> blocks;
    for (const Radix& d : x->v.digits) {
        if (d.nblocks() != kLimbBlocks) return invalid("fhe_biguint_compress: a limb is not a 32-bit radix");
        for (const Block& b : d.blocks) blocks.push_back(&b);
    }
    if (blocks.size() > kCompressedMaxBlocks) return invalid("compressed list of more than 2^24 blocks");
    return compress_blocks(c, blocks, FHE_SEEDED_BIGUINT, (uint32_t)x->v.digits.size(), out);
}

int fhe_compressed_expand_radix(fhe_ctx* c, const fhe_compressed_list* x, fhe_radix** out) {
    int rc = compressed_expand_check(c, x, FHE_SEEDED_RADIX);
    if (rc) return rc;
    if (!out) return FHE_ERR_INVALID;
    return guarded([&] {
        Radix r;
        r.blocks = c->engine->decompress(*x);
        *out = wrap(std::move(r), x->count);
        return FHE_OK;
    });
}

int fhe_compressed_expand_biguint(fhe_ctx* c, const fhe_compressed_list* x, fhe_biguint** out) {
    int rc = compressed_expand_check(c, x, FHE_SEEDED_BIGUINT);
    if (rc) return rc;
    if (!out) return FHE_ERR_INVALID;
    return guarded([&] {
        const Blocks all = c->engine->decompress(*x);
        auto v = std::make_unique<fhe_biguint>();
        for (size_t at = 0; at < all.size(); at += kLimbBlocks) {
            Radix d;
            d.blocks.assign(all.begin() + at, all.begin() + at + kLimbBlocks);
            v->v.digits.push_back(std::move(d));
        }
        *out = v.release();
        return FHE_OK;
    });
}

int fhe_compressed_extract_rows(fhe_ctx* c, const fhe_compressed_list* x, uint64_t* rows, size_t nwords) {
    if (!x) return invalid("null compressed list");
    int rc = compressed_expand_check(c, x, x->form, true);
    if (rc) return rc;
    if (!rows || nwords < x->degrees.size() * ((size_t)x->cp.lwe_dim() + 1)) return invalid("fhe_compressed_extract_rows: buffer too small");
    return guarded([&] {
        c->engine->extract_rows(*x, rows);
        return FHE_OK;
    });
}

int fhe_pack_keyswitch_words(fhe_ctx* c, const uint64_t* cts, size_t count, uint64_t* P, size_t p_words,
                             uint64_t* body) {
    int rc = need_rows(c);
    if (rc) return rc;
    if (!c->has_comp) {
        set_error("no compression key installed (fhe_set_compression_key)");
        return FHE_ERR_NO_KEY;
    }
    if (count > kCompressedMaxBlocks) return invalid("compressed list of more than 2^24 blocks");
    if (count && (!cts || !P || !body)) return invalid("null argument to fhe_pack_keyswitch_words");
    if (p_words < count * (size_t)c->cp.cols()) return invalid("fhe_pack_keyswitch_words: buffer too small");
    return guarded([&] {
        c->engine->pack_keyswitch_words(cts, count, P, body);
        return FHE_OK;
    });
}

}  // extern "C"

// ------------------------------------------------------------------------- modulus-switched stored ciphertexts
// tfhe-rs' CompressedModulusSwitchedCiphertext of one value (switched.h): the device ends of it.  The host ends
// (the definitions, the wire kind, fhe_switched_decrypt, the kernel hooks) are in switched.cpp.
namespace {
int switched_blocks(fhe_ctx* c, const std::vector<const Block*>& blocks, uint32_t form, uint32_t count,
                    fhe_switched_list** out, bool rekey = false) {
    if (rekey && !c->has_rekey) {
        set_error("no re-keying key installed (fhe_set_rekey_key)");
        return FHE_ERR_NO_KEY;
    }
    return guarded([&] {
        auto x = std::make_unique<fhe_switched_list>();
        x->params = rekey ? c->rkp : c->p;  // a re-keyed list is the destination key's
        x->form = form;
        x->count = count;
        for (const Block* b : blocks) {
            engine_check(b->degree < x->params.msg_carry(), "compress_switched: block degree >= message_modulus * carry_modulus");
            x->degrees.push_back((uint8_t)b->degree);
        }
        x->rows.resize(blocks.size() * switched_row_bytes(x->params.n));
        c->engine->switched_compress(blocks, x->rows.data(), rekey);
        *out = x.release();
        return FHE_OK;
    });
}
int switched_expand_check(fhe_ctx* c, const fhe_switched_list* x, uint32_t form) {
    int rc = need_engine(c);
    if (rc) return rc;
    if (!x) return invalid("null switched list");
    if (x->form != form)
        return invalid(form == FHE_SEEDED_RADIX ? "switched list holds a BigUintFHE, not a radix integer"
                                                : "switched list holds a radix integer, not a BigUintFHE");
    uint32_t have = 0, want = 0;
    if (const char* f = params_differ(x->params, c->p, &have, &want))
        return invalid(std::string("switched list's ") + f + " (" + std::to_string(have) +
                       ") differs from the context's server key (" + std::to_string(want) + ")");
    return FHE_OK;
}
int radix_switched(fhe_ctx* c, const fhe_radix* x, fhe_switched_list** out, bool rekey) {
    int rc = need_engine(c);
    if (rc) return rc;
    if (!x || !out) return invalid("null argument to fhe_radix_compress_switched");
    if ((rc = owned(c, x, "x"))) return rc;
    std::vector<const Block*> blocks;
    for (const Block& b : x->r.blocks) blocks.push_back(&b);
    return switched_blocks(c, blocks, FHE_SEEDED_RADIX, x->bits, out, rekey);
}
int biguint_switched(fhe_ctx* c, const fhe_biguint* x, fhe_switched_list** out, bool rekey) {
    int rc = need_engine(c);
    if (rc) return rc;
    if (!x || !out) return invalid("null argument to fhe_biguint_compress_switched");
    if ((rc = owned(c, x, "x"))) return rc;
    std::vector<const Block*> blocks;
    for (const Radix& d : x->v.digits) {
        if (d.nblocks() != kLimbBlocks) return invalid("fhe_biguint_compress_switched: a limb is not a 32-bit radix");
        for (const Block& b : d.blocks) blocks.push_back(&b);
    }
    if (blocks.size() > kCompressedMaxBlocks) return invalid("stored list of more than 2^24 blocks");
    return switched_blocks(c, blocks, FHE_SEEDED_BIGUINT, (uint32_t)x->v.digits.size(), out, rekey);
}
}  // namespace

extern "C" {

int fhe_radix_compress_switched(fhe_ctx* c, const fhe_radix* x, fhe_switched_list** out) {
    return radix_switched(c, x, out, false);
}
int fhe_biguint_compress_switched(fhe_ctx* c, const fhe_biguint* x, fhe_switched_list** out) {
    return biguint_switched(c, x, out, false);
}
int fhe_radix_compress_switched_rekeyed(fhe_ctx* c, const fhe_radix* x, fhe_switched_list** out) {
    return radix_switched(c, x, out, true);
}
int fhe_biguint_compress_switched_rekeyed(fhe_ctx* c, const fhe_biguint* x, fhe_switched_list** out) {
    return biguint_switched(c, x, out, true);
}

int fhe_switched_expand_radix(fhe_ctx* c, const fhe_switched_list* x, fhe_radix** out) {
    int rc = switched_expand_check(c, x, FHE_SEEDED_RADIX);
    if (rc) return rc;
    if (!out) return FHE_ERR_INVALID;
    return guarded([&] {
        Radix r;
        r.blocks = c->engine->switched_decompress(*x);
        *out = wrap(std::move(r), x->count);
        return FHE_OK;
    });
}

int fhe_switched_expand_biguint(fhe_ctx* c, const fhe_switched_list* x, fhe_biguint** out) {
    int rc = switched_expand_check(c, x, FHE_SEEDED_BIGUINT);
    if (rc) return rc;
    if (!out) return FHE_ERR_INVALID;
    return guarded([&] {
        const Blocks all = c->engine->switched_decompress(*x);
        auto v = std::make_unique<fhe_biguint>();
        for (size_t at = 0; at < all.size(); at += kLimbBlocks) {
            Radix d;
            d.blocks.assign(all.begin() + at, all.begin() + at + kLimbBlocks);
            v->v.digits.push_back(std::move(d));
        }
        *out = v.release();
        return FHE_OK;
    });
}

}  // extern "C"

// ------------------------------------------------------------------------- compact ciphertext lists
// tfhe-rs' CompactCiphertextList::expand (public_key.h): the device ends of it.  The host ends (key generation,
// encryption under the public key, the wire kinds, fhe_compact_list_expand_host, fhe_compact_list_decrypt) are
// in public_key.cpp.
namespace {
// the checks of every GPU expansion, before anything is allocated or launched
int compact_expand_check(fhe_ctx* c, const fhe_compact_list* x) {
    int rc = need_engine(c);
    if (rc) return rc;
    if (!x) return invalid("null compact list");
    uint32_t have = 0, want = 0;
    if (const char* f = params_differ(x->params, c->p, &have, &want))
        return invalid(std::string("compact list's ") + f + " (" + std::to_string(have) +
                       ") differs from the context's server key (" + std::to_string(want) + ")");
    return FHE_OK;
}
int compact_value_check(fhe_ctx* c, const fhe_compact_list* x, uint32_t index, uint32_t form) {
    int rc = compact_expand_check(c, x);
    if (rc) return rc;
    if (index >= x->values.size())
        return invalid("compact list: value index " + std::to_string(index) + " out of range (the list holds " +
                       std::to_string(x->values.size()) + ")");
    if (x->values[index].form != form)
        return invalid("compact list: value " + std::to_string(index) +
                       (form == FHE_SEEDED_RADIX ? " holds a BigUintFHE, not a radix integer"
                                                 : " holds a radix integer, not a BigUintFHE"));
    return FHE_OK;
}
}  // namespace

extern "C" {

int fhe_compact_list_expand_radix(fhe_ctx* c, const fhe_compact_list* x, uint32_t index, fhe_radix** out) {
    int rc = compact_value_check(c, x, index, FHE_SEEDED_RADIX);
    if (rc) return rc;
    if (!out) return FHE_ERR_INVALID;
    return guarded([&] {
        Radix r;
        r.blocks = c->engine->expand_compact(*x, index);
        *out = wrap(std::move(r), x->values[index].count);
        return FHE_OK;
    });
}

int fhe_compact_list_expand_biguint(fhe_ctx* c, const fhe_compact_list* x, uint32_t index, fhe_biguint** out) {
    int rc = compact_value_check(c, x, index, FHE_SEEDED_BIGUINT);
    if (rc) return rc;
    if (!out) return FHE_ERR_INVALID;
    return guarded([&] {
        const Blocks all = c->engine->expand_compact(*x, index);
        auto v = std::make_unique<fhe_biguint>();
        for (size_t at = 0; at < all.size(); at += kLimbBlocks) {
            Radix d;
            d.blocks.assign(all.begin() + at, all.begin() + at + kLimbBlocks);
            v->v.digits.push_back(std::move(d));
        }
        *out = v.release();
        return FHE_OK;
    });
}

int fhe_compact_list_extract_rows(fhe_ctx* c, const fhe_compact_list* x, uint64_t* rows, size_t nwords) {
    int rc = compact_expand_check(c, x);
    if (rc) return rc;
    if ((!rows && x->ncoef()) || nwords < x->ncoef() * kBigCt)
        return invalid("fhe_compact_list_extract_rows: buffer too small (ncoef x 2049 words)");
    return guarded([&] {
        c->engine->extract_compact_rows(*x, rows);
        return FHE_OK;
    });
}

}  // extern "C"

// ------------------------------------------------------------------------- re-randomization
// tfhe-rs' re_randomize under the CompactPublicKey (public_key.h): the device ends of it.  The host definition
// (fhe_rerandomize_host), the install (fhe_set_public_key) and the seed helper are in rerandomize.cpp and
// schnorr.cpp.
namespace {
// the checks of every re-randomization, before anything is flushed or launched; seed32 = the call's seed
int rerandomize_check(fhe_ctx* c, const uint8_t* seed, uint8_t seed32[32], bool rows = false) {
    int rc = rows ? need_rows(c) : need_engine(c);
    if (rc) return rc;
    if (!c->has_pk) {
        set_error("no public key installed (fhe_set_public_key)");
        return FHE_ERR_NO_KEY;
    }
    if (seed) {
        std::memcpy(seed32, seed, 32);
        return FHE_OK;
    }
    if (c->attached() && c->nranks > 1)
        return invalid("re-randomization under a communicator needs a seed: with seed = NULL every rank would draw its own "
                       "and the ranks' ciphertexts would diverge");
    if (!os_entropy32(seed32)) {
        set_error("getrandom failed: no re-randomization seed");
        return FHE_ERR_UNSUPPORTED;
    }
    return FHE_OK;
}
void wipe32(uint8_t seed32[32]) {
    volatile uint8_t* w = seed32;
    for (int i = 0; i < 32; ++i) w[i] = 0;
}
}  // namespace

extern "C" {

int fhe_radix_rerandomize(fhe_ctx* c, const fhe_radix* x, const uint8_t* seed, fhe_radix** out) {
    if (!x || !out) return invalid("null argument to fhe_radix_rerandomize");
    uint8_t seed32[32];
    int rc = rerandomize_check(c, seed, seed32);
    if (!rc && (rc = owned(c, x, "x"))) wipe32(seed32);
    if (rc) return rc;
    rc = guarded([&] {
        std::vector<const Block*> blocks;
        for (const Block& b : x->r.blocks) blocks.push_back(&b);
        Radix r;
        r.blocks = c->engine->rerandomize(blocks, seed32);
        *out = wrap(std::move(r), x->bits);
        return FHE_OK;
    });
    wipe32(seed32);  // used for this call, kept nowhere
    return rc;
}

int fhe_biguint_rerandomize(fhe_ctx* c, const fhe_biguint* x, const uint8_t* seed, fhe_biguint** out) {
    if (!x || !out) return invalid("null argument to fhe_biguint_rerandomize");
    uint8_t seed32[32];
    int rc = rerandomize_check(c, seed, seed32);
    if (!rc && (rc = owned(c, x, "x"))) wipe32(seed32);
    if (rc) return rc;
    rc = guarded([&] {
        std::vector<const Block*> blocks;
        for (const Radix& d : x->v.digits) {
            engine_check(d.nblocks() == kLimbBlocks, "fhe_biguint_rerandomize: a limb is not a 32-bit radix");
            for (const Block& b : d.blocks) blocks.push_back(&b);
        }
        const Blocks all = c->engine->rerandomize(blocks, seed32);
        auto v = std::make_unique<fhe_biguint>();
        for (size_t at = 0; at < all.size(); at += kLimbBlocks) {
            Radix d;
            d.blocks.assign(all.begin() + at, all.begin() + at + kLimbBlocks);
            v->v.digits.push_back(std::move(d));
        }
        *out = v.release();
        return FHE_OK;
    });
    wipe32(seed32);
    return rc;
}

int fhe_rerandomize_rows(fhe_ctx* c, const uint8_t* seed, const uint64_t* rows, size_t nblocks, uint64_t* out) {
    if (!seed || ((!rows || !out) && nblocks)) return invalid("null argument to fhe_rerandomize_rows");
    if (nblocks > kCompactMaxCoefs) return invalid("fhe_rerandomize_rows: more than 2^24 blocks");
    uint8_t seed32[32];
    int rc = rerandomize_check(c, seed, seed32, true);
    if (rc || !nblocks) return rc;
    return guarded([&] {
        const Blocks in = c->engine->upload_many(rows, nblocks, std::min(kMsgMod, c->p.msg_carry()) - 1);
        std::vector<const Block*> blocks;
        for (const Block& b : in) blocks.push_back(&b);
        const Blocks res = c->engine->rerandomize(blocks, seed32);
        for (size_t i = 0; i < nblocks; ++i) blocks[i] = &res[i];
        c->engine->download_many(blocks, out);
        return FHE_OK;
    });
}

}  // extern "C"

// ------------------------------------------------------------------------- ciphertext digests
// The device ends of ct_digest.h: the value digest of a resident operand, the row digests computed by
// Engine::digest.  The host definitions and the re-randomization context are in ct_digest.cpp.
namespace {
void value_digest(fhe_ctx* c, uint8_t kind, uint32_t bits, const std::vector<const Block*>& blocks, uint8_t out[32]) {
    const size_t n = blocks.size();
    std::vector<uint8_t> rowd(32 * n), tags(n);
    std::vector<uint32_t> degrees(n), noises(n);
    std::vector<Engine::DigestMeta> meta;
    c->engine->digest(blocks, rowd.data(), &meta);
    for (size_t i = 0; i < n; ++i) {
        tags[i] = meta[i].tag;
        degrees[i] = meta[i].degree;
        noises[i] = meta[i].noise;
    }
    ct_value_digest_host(kind, bits, tags.data(), degrees.data(), noises.data(), rowd.data(), n, out);
}
int radix_digest(fhe_ctx* c, const fhe_radix* x, uint8_t out[32]) {
    int rc = need_engine(c);
    if (!rc) rc = owned(c, x, "x");
    if (rc) return rc;
    return guarded([&] {
        std::vector<const Block*> blocks;
        for (const Block& b : x->r.blocks) blocks.push_back(&b);
        value_digest(c, FHE_CT_KIND_RADIX, x->bits, blocks, out);
        return FHE_OK;
    });
}
int biguint_digest(fhe_ctx* c, const fhe_biguint* x, uint8_t out[32]) {
    int rc = need_engine(c);
    if (!rc) rc = owned(c, x, "x");
    if (rc) return rc;
    return guarded([&] {
        std::vector<const Block*> blocks;
        for (const Radix& d : x->v.digits) {
            engine_check(d.nblocks() == kLimbBlocks, "fhe_biguint_digest: a limb is not a 32-bit radix");
            for (const Block& b : d.blocks) blocks.push_back(&b);
        }
        value_digest(c, FHE_CT_KIND_BIGUINT, (uint32_t)(32 * x->v.digits.size()), blocks, out);
        return FHE_OK;
    });
}
}  // namespace

extern "C" {

int fhe_radix_digest(fhe_ctx* c, const fhe_radix* x, uint8_t out[32]) {
    if (!x || !out) return invalid("null argument to fhe_radix_digest");
    return radix_digest(c, x, out);
}

int fhe_biguint_digest(fhe_ctx* c, const fhe_biguint* x, uint8_t out[32]) {
    if (!x || !out) return invalid("null argument to fhe_biguint_digest");
    return biguint_digest(c, x, out);
}

int fhe_rerand_context_add_radix(fhe_ctx* c, fhe_rerand_context* rc, const fhe_radix* x) {
    if (!rc || !x) return invalid("null argument to fhe_rerand_context_add_radix");
    if (rc->finalized) return invalid("fhe_rerand_context_add_radix: the context gave out a seed already; a seed depends on everything added");
    uint8_t d[32];
    const int r = radix_digest(c, x, d);
    return r ? r : fhe_rerand_context_add_digest(rc, d);
}

int fhe_rerand_context_add_biguint(fhe_ctx* c, fhe_rerand_context* rc, const fhe_biguint* x) {
    if (!rc || !x) return invalid("null argument to fhe_rerand_context_add_biguint");
    if (rc->finalized) return invalid("fhe_rerand_context_add_biguint: the context gave out a seed already; a seed depends on everything added");
    uint8_t d[32];
    const int r = biguint_digest(c, x, d);
    return r ? r : fhe_rerand_context_add_digest(rc, d);
}

int fhe_ct_digest_rows(fhe_ctx* c, const uint64_t* rows, size_t nblocks, uint8_t* out) {
    if ((!rows || !out) && nblocks) return invalid("null argument to fhe_ct_digest_rows");
    if (nblocks > kCtDigestMaxRows) return invalid("fhe_ct_digest_rows: more than 2^24 blocks");
    int rc = need_rows(c);
    if (rc || !nblocks) return rc;
    return guarded([&] {
        const Blocks in = c->engine->upload_many(rows, nblocks, std::min(kMsgMod, c->p.msg_carry()) - 1);
        std::vector<const Block*> blocks;
        for (const Block& b : in) blocks.push_back(&b);
        c->engine->digest(blocks, out);
        return FHE_OK;
    });
}

}  // extern "C"

// ------------------------------------------------------------------------- oblivious pseudo-random values
// tfhe-rs' FheUint::generate_oblivious_pseudo_random[_bounded]: the radix ends of oprf.h.  The host definitions,
// the row kernel's test entries and fhe_oprf_blocks are in oprf.cpp, the device path is Engine::oprf.
namespace {
// the checks of every draw, before anything is launched; seed32 = the call's seed
int oprf_check(fhe_ctx* c, const uint8_t* seed, uint8_t seed32[32]) {
    int rc = need_engine(c);
    if (rc) return rc;
    if (seed) {
        std::memcpy(seed32, seed, 32);
        return FHE_OK;
    }
    if (c->attached() && c->nranks > 1)
        return invalid("an oblivious pseudo-random value under a communicator needs a seed: with seed = NULL every rank "
                       "would draw its own and the ranks' ciphertexts would diverge");
    if (!os_entropy32(seed32)) {
        set_error("getrandom failed: no seed for the oblivious pseudo-random value");
        return FHE_ERR_UNSUPPORTED;
    }
    return FHE_OK;
}
// nblocks blocks whose low random_bits bits are random: full blocks on the rows of their index, an odd top bit
// as a 1-bit block on its row, trivial zeros above
Radix radix_random(Engine& e, const uint8_t seed[32], uint32_t nblocks, uint32_t random_bits) {
    Radix r;
    r.blocks = e.oprf(seed, random_bits / kMsgBits, kMsgBits, random_bits % kMsgBits);
    r.blocks.resize(nblocks, Block::make_trivial(0));
    return r;
}
}  // namespace

extern "C" {

int fhe_radix_random(fhe_ctx* c, const uint8_t* seed, uint32_t width_bits, uint32_t random_bits, fhe_radix** out) {
    if (!out) return invalid("null argument to fhe_radix_random");
    if (!valid_bits(width_bits)) return invalid("fhe_radix_random: the width must be even and 2 .. " + std::to_string(FHE_RADIX_MAX_BITS));
    if (random_bits < 1 || random_bits > width_bits) return invalid("fhe_radix_random: random_bits must be 1 .. the width");
    uint8_t seed32[32];
    int rc = oprf_check(c, seed, seed32);
    if (rc) return rc;
    rc = guarded([&] {
        *out = wrap(radix_random(*c->engine, seed32, width_bits / kMsgBits, random_bits), width_bits);
        return FHE_OK;
    });
    wipe32(seed32);
    return rc;
}

int fhe_radix_random_below(fhe_ctx* c, const uint8_t* seed, uint32_t width_bits, const uint64_t* bound, size_t nwords,
                           uint32_t extra_bits, fhe_radix** out) {
    if (!out || (!bound && nwords)) return invalid("null argument to fhe_radix_random_below");
    if (!valid_bits(width_bits))
        return invalid("fhe_radix_random_below: the width must be even and 2 .. " + std::to_string(FHE_RADIX_MAX_BITS));
    BigConst b = words_of(bound, nwords);
    const uint32_t blen = big_bitlen(b);
    if (blen == 0) return invalid("fhe_radix_random_below: the bound must be positive");
    // bit_length(bound - 1)
    BigConst b1 = b;
    for (size_t i = 0; i < b1.size(); ++i)
        if (b1[i]-- != 0) break;
    const uint32_t range_bits = big_bitlen(b1);
    if (range_bits > width_bits) return invalid("fhe_radix_random_below: values below the bound do not fit the width");
    // (r bound) >> m of an m-bit r, computed at m + bit_length(bound) bits: the product does not wrap
    const uint64_t m = (uint64_t)range_bits + extra_bits, wide = (m + blen + 1) / 2 * 2;
    if (wide > FHE_RADIX_MAX_BITS)
        return invalid("fhe_radix_random_below: bit_length(bound - 1) + extra_bits + bit_length(bound) = " + std::to_string(m + blen) +
                       " bits exceed the " + std::to_string(FHE_RADIX_MAX_BITS) + " a radix integer holds");
    uint8_t seed32[32];
    int rc = oprf_check(c, seed, seed32);
    if (rc) return rc;
    rc = guarded([&] {
        Engine& e = *c->engine;
        Radix r = radix_random(e, seed32, (uint32_t)wide / kMsgBits, (uint32_t)m);
        if (m) r = radix_scalar_shr(e, radix_scalar_mul(e, r, b), (uint32_t)m);
        *out = wrap(radix_resize(r, width_bits / kMsgBits), width_bits);
        return FHE_OK;
    });
    wipe32(seed32);
    return rc;
}

int fhe_biguint_random(fhe_ctx* c, const uint8_t* seed, uint32_t bits, fhe_biguint** out) {
    if (!out) return invalid("null argument to fhe_biguint_random");
    if (bits % 32 != 0 || bits / kMsgBits > kOprfMaxRows) return invalid("fhe_biguint_random: bits must be a multiple of 32");
    uint8_t seed32[32];
    int rc = oprf_check(c, seed, seed32);
    if (rc) return rc;
    rc = guarded([&] {
        const Blocks all = c->engine->oprf(seed32, bits / kMsgBits, kMsgBits);
        auto v = std::make_unique<fhe_biguint>();
        for (size_t at = 0; at < all.size(); at += kLimbBlocks) {
            Radix d;
            d.blocks.assign(all.begin() + at, all.begin() + at + kLimbBlocks);
            v->v.digits.push_back(std::move(d));
        }
        *out = v.release();
        return FHE_OK;
    });
    wipe32(seed32);
    return rc;
}

}  // extern "C"
