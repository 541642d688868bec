// engine.cpp -- the engine under the radix layer (engine.h): the block pool, the deferred graph of bootstraps
// (run: host folding, degree and noise bookkeeping, recording), its level scheduler and the flushes that launch
// it (one batched keyswitch + one blind rotate per level), the dry and simulated host modes, lincomb.  The
// eager device operations (uploads, downloads, the seeded / compact / compressed forms) are engine_ops.cpp.
#include "engine.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <queue>
#include <string>

namespace fhe {

Tuning& tuning() {
    static Tuning t;
    return t;
}

void fault_cross(const char* site) {
    Tuning& t = tuning();
    const uint64_t n = ++t.fault_crossings;
    if (t.fault_after && n == t.fault_after) {
        t.fault_after = 0;  // one shot
        throw EngineError(FHE_ERR_HIP, std::string("injected fault at ") + site);
    }
}

const Debug& debug() {
    static const Debug d = [] {
        Debug x;
        const char* v = getenv("FHE_DEBUG");
        const std::string s = v ? std::string(",") + v + "," : std::string();
        auto has = [&](const char* k) { return s.find(std::string(",") + k + ",") != std::string::npos; };
        x.levels = has("levels");
        x.graph = has("graph");
        x.chain = has("chain");
        x.chain_host = has("chain-host");
        x.residue = has("residue");
        x.nodes = has("nodes");
        return x;
    }();
    return d;
}

void engine_check(bool ok, const char* what) {
    if (!ok) throw std::runtime_error(what);
}

void hip_check(hipError_t e, const char* what) {
    if (e != hipSuccess) throw EngineError(FHE_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

void wait_check(fhe_ctx* c, const char* what) {
    const int rc = c->wait_stream(what);
    if (rc != FHE_OK) throw EngineError(rc, last_error());
}

// ============================================================================ block pool
Slot::~Slot() {
    if (pool && p) pool->release(p);
}

BlockPool::~BlockPool() {
    if (dry_ || chunks_.empty()) return;  // a host-only engine never touches the HIP runtime
    (void)hipSetDevice(device_);            // the chunks free themselves
}

std::shared_ptr<Slot> BlockPool::alloc() {
    if (dry_) {
        auto s = std::make_shared<Slot>();
        s->p = reinterpret_cast<uint64_t*>(dry_next_);
        dry_next_ += kBigCt * 8;
        s->pool = shared_from_this();  // the owner (Engine::owns); release() keeps nothing of a placeholder
        return s;
    }
    if (free_.empty()) {
        const size_t per = 1024;  // 16 MiB chunks
        DeviceBuf<uint64_t> chunk;
        const auto t0 = std::chrono::steady_clock::now();
        hip_check(chunk.grow(per * kBigCt), "block pool allocation");
        grow_ns_ += std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count();
        ++grows_;
        uint64_t* const c = chunk;
        chunks_.push_back(std::move(chunk));
        for (size_t i = 0; i < per; ++i) free_.push_back(c + (per - 1 - i) * kBigCt);
        total_ += per;
    }
    auto s = std::make_shared<Slot>();
    s->p = free_.back();
    free_.pop_back();
    s->pool = shared_from_this();
    return s;
}

// ============================================================================ engine
Engine::Engine(fhe_ctx* ctx, int host_mode) : ctx_(ctx), host_mode_(host_mode) {
    pool_ = std::make_shared<BlockPool>(ctx->device, host_mode_ != kDevice);  // host modes allocate no device slots
    if (host_mode_ == kDevice)
        for (auto& ev : desc_ev_) hip_check(hipEventCreateWithFlags(&ev, hipEventDisableTiming), "event");
    trace_ = debug().levels;
    gstats_ = debug().graph;
}

bool Engine::owns(const Block& b) const {
    if (b.lazy()) {
        for (const Term& t : *b.lin)
            if (t.b.slot && t.b.slot->pool.get() != pool_.get()) return false;
        return true;
    }
    return !b.slot || b.slot->pool.get() == pool_.get();
}

void Engine::check_owner(const Block& b, const char* operand) const {
    if (owns(b)) return;
    throw EngineError(FHE_ERR_INVALID, operand ? std::string("operand ") + operand + " was made under another context"
                                               : std::string("a ciphertext block was made under another context"));
}

void Engine::check_owner(const std::vector<const Block*>& blocks, const char* operand) const {
    for (const Block* b : blocks) check_owner(*b, operand);
}

int32_t Engine::depth_of(const Block& b) const {
    check_owner(b);
    int32_t d = 0;
    auto one = [&](const Block& x) {
        // an owned slot's node indexes this engine's list (flush keeps it so); the bound states it
        if (x.slot && x.slot->node >= 0 && (size_t)x.slot->node < pending_.size())
            d = std::max(d, pending_[x.slot->node].depth);
    };
    if (b.lazy())
        for (const Term& t : *b.lin) one(t.b);
    else
        one(b);
    return d;
}

Block Engine::sim_block(uint32_t value, uint32_t degree) {
    engine_check(host_mode_ == kSim && value <= degree, "sim_block outside a simulating engine");
    Block b = dry_block(degree);
    sim_[b.ptr()] = 2 * (int64_t)value;
    return b;
}

int64_t Engine::sim_half2(const Block& b) const {
    if (b.trivial()) return trivial_half2(b);
    check_owner(b);  // another engine's placeholder address would find this engine's shadow under it
    if (b.lazy()) {
        int64_t v = 2 * (int64_t)b.lin_cst;
        for (const Term& t : *b.lin) v += (int64_t)t.coef * sim_half2(t.b);
        return v;
    }
    auto it = sim_.find(b.ptr());
    engine_check(it != sim_.end(), "sim: a block without a plaintext shadow");
    return it->second;
}

Block Engine::dry_block(uint32_t degree) {
    engine_check(host_mode_ == kDry || host_mode_ == kSim, "dry_block outside a dry engine");
    Block b;
    b.slot = pool_->alloc();
    b.degree = degree;
    b.noise = 1;
    if (ltrace_on_) trace_write(kWriteUpload, &b.slot->p, 1);  // a placeholder's "upload"
    return b;
}

// ============================================================================ launch trace (engine.h)
bool Engine::trace_room(size_t words) {
    if (ltrace_overflow_ || ltrace_.size() + words > kTraceCap) {
        ltrace_overflow_ = true;
        return false;
    }
    return true;
}

void Engine::trace_write(uint64_t kind, uint64_t* const* dst, size_t n) {
    if (n == 0 || !trace_room(3 + n)) return;
    ltrace_.push_back(kTraceWrite);
    ltrace_.push_back(kind);
    ltrace_.push_back(n);
    for (size_t i = 0; i < n; ++i) ltrace_.push_back((uint64_t)reinterpret_cast<uintptr_t>(dst[i]));
}

// one node or lincomb record from a descriptor as it is launched; `wide`: the host copy of its TermExt table
void Engine::trace_op(uint64_t tag, const PbsDesc& d, const uint64_t* dst, const TermExt* wide) {
    const bool node = tag == kTraceNode;
    engine_check(wide || d.nterms <= (uint32_t)kMaxTerms, "trace: a wide combination without its term table");
    if (!trace_room((node ? 5 : 4) + 2 * (size_t)d.nterms)) return;
    ltrace_.push_back(tag);
    ltrace_.push_back((uint64_t)reinterpret_cast<uintptr_t>(dst));
    if (node) ltrace_.push_back(d.lut);
    ltrace_.push_back(d.cst);
    ltrace_.push_back(d.nterms);
    for (uint32_t u = 0; u < d.nterms; ++u) {
        ltrace_.push_back((uint64_t)reinterpret_cast<uintptr_t>(wide ? wide[u].src : d.src[u]));
        ltrace_.push_back((uint64_t)(wide ? wide[u].coef : (int64_t)d.coef[u]));
    }
}

Engine::~Engine() {
    if (host_mode_ != kDevice) return;
    (void)hipSetDevice(ctx_->device);
    (void)hipStreamSynchronize(ctx_->stream);
    for (auto ev : desc_ev_)
        if (ev) (void)hipEventDestroy(ev);
}

// The upload / download staging, at least `words` u64: grown to exactly that, behind the stream, when short.
uint64_t* Engine::staging(size_t words) {
    if (!d_up_.fits(words)) {
        hip_check(hipStreamSynchronize(ctx_->stream), "staging sync");
        hip_check(d_up_.grow(words), "staging allocation");
    }
    return d_up_;
}

void Engine::ensure_desc(size_t n) {
    if (n > desc_cap_) {
        const size_t cap = std::max<size_t>(n, 4096);
        desc_cap_ = 0;
        for (int i = 0; i < 2; ++i) {
            if (h_desc_[i]) hip_check(hipEventSynchronize(desc_ev_[i]), "desc event");
            hip_check(h_desc_[i].grow(cap), "pinned descriptors");
        }
        desc_cap_ = cap;
    }
    if (!d_desc_.fits(n)) {
        hip_check(hipStreamSynchronize(ctx_->stream), "sync");
        hip_check(d_desc_.grow(std::max<size_t>(n, 4096)), "device descriptors");
    }
}

// Host staging buffer for n descriptors (double-buffered: wait until its previous copy is done).
PbsDesc* Engine::stage_desc(size_t n, PbsDesc** dev) {
    ensure_desc(n);
    desc_turn_ ^= 1;
    hip_check(hipEventSynchronize(desc_ev_[desc_turn_]), "desc event");
    *dev = d_desc_;
    return h_desc_[desc_turn_];
}

namespace {
// reachable plaintexts of sum coef*x_t + cst (x_t in [0, degree_t]) as a bitmask over [0, 64)
uint64_t reachable(const std::vector<Term>& terms, int64_t cst, bool* ok) {
    *ok = true;
    if (cst < 0 || cst >= 64) {
        *ok = false;
        return 0;
    }
    uint64_t set = 1ull << cst;
    for (const Term& t : terms) {
        // the set shifted by coef * x for every x in [0, degree]; a bit leaving [0, 64) is an input
        // outside the message space
        uint64_t nxt = 0;
        for (uint32_t x = 0; x <= t.b.degree; ++x) {
            const int64_t sh = (int64_t)t.coef * x;
            if (sh >= 0) {
                if (sh >= 64 || (sh > 0 && (set >> (64 - sh)) != 0)) {
                    *ok = false;
                    return 0;
                }
                nxt |= set << sh;
            } else {
                if (-sh >= 64 || (set & ((1ull << -sh) - 1)) != 0) {
                    *ok = false;
                    return 0;
                }
                nxt |= set >> -sh;
            }
        }
        set = nxt;
    }
    return set;
}
// a reachable plaintext at or above the message space of mc values (mc <= 64; at 64 the mask is the whole space)
bool beyond(uint64_t reach, uint32_t mc) { return mc < 64 && (reach >> mc) != 0; }
}  // namespace

Blocks Engine::run(std::vector<PbsItem>& items) {
    struct Clock {  // host time inside run() (FHE_TRACE_LEVELS: printed at the next flush)
        Engine* e;
        std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
        ~Clock() { e->run_ns_ += std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count(); }
    } clock{this};
    fault_point(kFaultRecord, "RECORD");
    // ownership first: a refusal leaves no item processed, no slot allocated and no statistic moved
    for (const PbsItem& it : items)
        for (const Term& t : it.terms) check_owner(t.b);
    ++run_calls_;
    const Params& p = ctx_->p;
    const uint32_t mc = p.msg_carry();
    Blocks out(items.size());
    std::vector<size_t> gpu;
    std::vector<std::vector<Term>> live(items.size());
    std::vector<int64_t> csts(items.size());
    std::vector<uint32_t> labels(items.size(), 0);  // sum coef^2 noise per term (the merged check is at recording)
    for (size_t i = 0; i < items.size(); ++i) {
        PbsItem& it = items[i];
        if (it.raw) {  // caller-guaranteed range (engine.h): no folding, no degree check
            engine_check(it.half_table.size() == mc, "raw LUT table size");
            int64_t cst2 = 2 * (int64_t)it.cst + it.half_cst;  // half steps
            uint32_t noise = 0;
            int64_t lo2 = 0, hi2 = 0;  // worst-case interval of the live terms (half steps, from degrees)
            for (const Term& t : it.terms) {
                if (t.coef == 0) continue;
                if (t.b.trivial())
                    cst2 += (int64_t)t.coef * trivial_half2(t.b);
                else {
                    live[i].push_back(t);
                    noise += (uint32_t)(t.coef * t.coef) * t.b.noise;
                    const int64_t bl = t.b.half_neg ? -1 : 0, bh = 2 * (int64_t)t.b.degree - (t.b.half_neg ? 1 : 0);
                    lo2 += t.coef > 0 ? t.coef * bl : t.coef * bh;
                    hi2 += t.coef > 0 ? t.coef * bh : t.coef * bl;
                }
            }
            labels[i] = noise;
            // the caller guarantees the actual input lies in [-16, 16) (kSim checks every sampled one); the
            // degrees alone must keep it inside one period of the negacyclic domain, [-32, 32) units (the
            // widest raw item of the test suite reaches [-22.5, 21.5)), or a misuse could alias unseen
            engine_check(cst2 + lo2 >= -64 && cst2 + hi2 < 64, "raw PBS item: input interval beyond one negacyclic period");
            if (live[i].empty()) {  // a known input: evaluate on the host (no noise: the label is 0)
                engine_check(cst2 % 2 == 0 && cst2 >= -32 && cst2 < 32, "raw PBS item: known input off the grid");
                const int64_t v = cst2 / 2;
                const int32_t h = v >= 0 ? it.half_table[v] : -it.half_table[v + 16];
                // an integer output, or a sign lookup's +-1/2 (kept as value - 1/2)
                engine_check(h % 2 == 0 ? h >= 0 : (h == 1 || h == -1), "raw PBS item: known output off the grid");
                out[i] = Block::make_trivial((uint32_t)((h + 1) / 2));
                out[i].half_neg = h % 2 != 0;
                continue;
            }
            out[i].degree = it.raw_degree;
            out[i].noise = 1;
            csts[i] = cst2;  // half steps (raw)
            gpu.push_back(i);
            continue;
        }
        engine_check(it.table.size() == mc, "LUT table size");
        int64_t cst = it.cst;
        uint32_t noise = 0;
        for (const Term& t : it.terms) {
            if (t.coef == 0) continue;
            engine_check(!t.b.half_neg, "a sign lookup output in an ordinary item");
            if (t.b.trivial())
                cst += (int64_t)t.coef * t.b.value;
            else {
                live[i].push_back(t);
                noise += (uint32_t)(t.coef * t.coef) * t.b.noise;
            }
        }
        bool ok;
        const uint64_t reach = reachable(live[i], cst, &ok);
        engine_check(ok && !beyond(reach, mc), "PBS input out of the message space (degree overflow)");
        labels[i] = noise;
        uint32_t lo = 0xffffffffu, hi = 0;
        bool identity = live[i].size() == 1 && live[i][0].coef == 1 && cst == 0 && live[i][0].b.noise <= 1 &&
                        !live[i][0].b.lazy();
        for (uint32_t v = 0; v < mc; ++v) {
            if (!(reach >> v & 1)) continue;
            const uint32_t f = it.table[v] % mc;
            lo = std::min(lo, f);
            hi = std::max(hi, f);
            if (f != v) identity = false;
        }
        // an item that folds or aliases on the host launches nothing: its label is checked as it always was
        if (lo == hi || identity) engine_check(noise <= kMaxNoise, "PBS input noise above the budget");
        if (lo == hi) {
            out[i] = Block::make_trivial(lo);
        } else if (identity) {
            out[i] = live[i][0].b;  // LUT is the identity on every reachable input: alias
            out[i].degree = hi;
        } else {
            out[i].degree = hi;
            out[i].noise = 1;
            csts[i] = cst;
            gpu.push_back(i);
        }
    }
    if (gpu.empty()) return out;
    engine_check(host_mode_ != kHostFold, "host-only engine: an item needs a bootstrap (encrypted input)");

    settle();  // nodes a partial flush left behind that were released since (flush_for)
    // register LUTs, allocate destinations, record pending nodes
    const uint64_t delta = p.delta();
    std::vector<TermExt> terms;
    std::vector<uint32_t> term_noise;  // of terms' slots
    const size_t n_before = pending_.size();
    bool all_independent = true;  // no new node reads a pending one
    for (size_t i : gpu) {
        const bool raw = items[i].raw;
        Pending n;
        PbsDesc& d = n.d;
        std::memset(&d, 0, sizeof d);
        n.hold.push_back(nullptr);  // [0]: the output slot, allocated once the item has passed its checks
        // flatten lazy terms into their slot blocks (merging repeats); dcst in half steps for raw items
        int64_t dcst = csts[i];
        const int64_t unit = raw ? 2 : 1;
        terms.clear();
        term_noise.clear();
        const size_t cap = (size_t)kMaxWideTerms;  // > kMaxTerms: staged as a wide combination
        auto put = [&](const Block& b, int32_t coef) {
            for (TermExt& u : terms)
                if (u.src == b.ptr()) {
                    u.coef += coef;
                    return;
                }
            engine_check(terms.size() < cap, "too many terms in one PBS input");
            terms.push_back({b.ptr(), coef});
            term_noise.push_back(b.noise);
            n.hold.push_back(b.slot);
            if (b.slot->node >= 0) {
                // the slot is this engine's (checked above), so its node is an index into this engine's list
                engine_check((size_t)b.slot->node < pending_.size(), "a pending producer outside the recorded graph");
                n.deps.push_back((int32_t)b.slot->node);
            }
        };
        for (const Term& t : live[i]) {
            if (!t.b.lazy()) {
                put(t.b, t.coef);
                continue;
            }
            dcst += unit * (int64_t)t.coef * t.b.lin_cst;
            for (const Term& u : *t.b.lin) put(u.b, t.coef * u.coef);
        }
        // The budget is enforced on what is launched: a slot named twice (x * x's diagonal products, x & x, a
        // value and its clone) enters with its coefficients summed, so its error does too -- variance
        // (sum coef)^2 noise per slot, where the label's sum of coef^2 noise per term assumes independent terms.
        // Cancellation (x - x) makes the merged figure the smaller one.  Fresh client encryptions uploaded twice
        // are distinct slots of equal, tiny noise: not seen here, and not a concern.
        uint64_t merged = 0;
        for (size_t u = 0; u < terms.size(); ++u) merged += (uint64_t)((int64_t)terms[u].coef * terms[u].coef) * term_noise[u];
        audit.max_label = std::max<uint64_t>(audit.max_label, labels[i]);
        audit.max_merged = std::max(audit.max_merged, merged);
        if (merged > labels[i]) ++audit.n_above_label;
        engine_check(merged <= kMaxNoise, raw ? "raw PBS input noise above the budget" : "PBS input noise above the budget");
        uint32_t lut = 0;
        if (raw)
            engine_check(ctx_->register_lut_half(items[i].half_table.data(), &lut) == FHE_OK, "LUT registration");
        else
            engine_check(ctx_->register_lut(items[i].table.data(), &lut) == FHE_OK, "LUT registration");
        out[i].slot = pool_->alloc();
        n.hold[0] = out[i].slot;
        if (host_mode_ == kSim) {  // the plaintext shadow of this bootstrap
            int64_t v2 = raw ? csts[i] : 2 * csts[i];
            for (const Term& t : live[i]) v2 += (int64_t)t.coef * sim_half2(t.b);
            int64_t o2;
            if (raw) {
                engine_check(v2 % 2 == 0 && v2 >= -32 && v2 < 32, "sim: raw PBS input outside [-16, 16)");
                const int64_t v = v2 / 2;
                o2 = v >= 0 ? items[i].half_table[v] : -items[i].half_table[v + 16];
            } else {
                engine_check(v2 % 2 == 0 && v2 >= 0 && v2 < 2 * (int64_t)mc, "sim: PBS input outside the message space");
                o2 = 2 * (int64_t)(items[i].table[v2 / 2] % mc);
            }
            sim_[out[i].ptr()] = o2;
        }
        const uint32_t nt = (uint32_t)terms.size();
        if (nt <= (uint32_t)kMaxTerms) {
            for (uint32_t u = 0; u < nt; ++u) {
                d.src[u] = terms[u].src;
                d.coef[u] = (int32_t)terms[u].coef;
            }
        } else {
            n.ext = terms;  // d.src[0] is set to their staged copy at flush
        }
        d.nterms = nt;
        d.lut = lut;
        d.cst = raw ? (uint64_t)dcst * (delta / 2) : (uint64_t)dcst * delta;
        if (gstats_) {
            std::vector<std::pair<const uint64_t*, int64_t>> tk;
            for (uint32_t u = 0; u < nt; ++u) tk.push_back({terms[u].src, terms[u].coef});
            std::sort(tk.begin(), tk.end());
            std::string key(reinterpret_cast<const char*>(tk.data()), tk.size() * sizeof(tk[0]));
            key.append(reinterpret_cast<const char*>(&dcst), sizeof dcst);
            in_key_.push_back(std::move(key));
            bool okr;
            const uint64_t rr = raw ? 0xFFFFull : reachable(live[i], csts[i], &okr);
            in_deg_.push_back((uint8_t)(raw ? 16 : 63 - __builtin_clzll(rr | 1)));
        }
        d.dst = out[i].slot->p;
        for (int32_t dep : n.deps) n.depth = std::max(n.depth, pending_[dep].depth + 1);
        out[i].slot->node = (int64_t)pending_.size();
        if (!n.deps.empty()) {
            ++pending_dependent_;
            all_independent = false;
        }
        pending_depth_ = std::max(pending_depth_, n.depth);
        pending_.push_back(std::move(n));
    }
    if (pending_.size() >= (size_t)1 << 20) flush();  // bound the deferred graph (host memory)
    // a deep graph (a long dependent chain: the encrypted division's 660 levels) is launched in slices
    // of flush_depth levels, so the GPU runs one slice while the host records the next instead of
    // waiting for the whole graph (the 256-bit division's ~150 ms of host recording); the slice's
    // levels are scheduled on their own (a boundary can cost a fill opportunity, not a level)
    if (tuning().flush_depth && pending_depth_ >= (int32_t)tuning().flush_depth) flush();
    // the first large batch with nothing pending before it (e.g. a wide multiplication's block
    // products) is one throughput level under any schedule: launch it now, so the GPU works while
    // the host builds the rest of the graph (once per explicit flush: later independent batches,
    // e.g. the compressions that follow, stay in the graph to be spread over idle capacity)
    if (eager_ok_ && pending_.size() >= kEagerBatch && pending_dependent_ == 0) {
        flush();
        eager_ok_ = false;
        eager_batch_next_ = false;
    } else if (eager_batch_next_ && n_before > 0 && all_independent && pending_.size() - n_before >= kEagerBatch &&
               !gstats_) {
        // (a batch of independent programs, eager_next_batch) the program's first large batch that reads
        // nothing pending, recorded behind the earlier programs' pending work -- the next signature's
        // block products -- is launched now on its own, so the GPU runs it while the host records the
        // rest; everything else stays deferred and is scheduled together (the programs share their
        // latency levels)
        eager_batch_next_ = false;
        flush_tail(n_before);
    }
    return out;
}

// flush() of the nodes recorded from index k0 on (none of which reads an earlier pending node); the
// nodes before k0 stay pending, with their indices
void Engine::flush_tail(size_t k0) {
    std::vector<Pending> keep(std::make_move_iterator(pending_.begin()), std::make_move_iterator(pending_.begin() + k0));
    pending_.erase(pending_.begin(), pending_.begin() + k0);
    for (size_t i = 0; i < pending_.size(); ++i) {
        engine_check(pending_[i].deps.empty(), "tail flush of a node with pending producers");
        pending_[i].hold[0]->node = (int64_t)i;
    }
    const size_t dependent = pending_dependent_;
    const int32_t depth = pending_depth_;
    const bool eager = eager_ok_;
    pending_dependent_ = 0;
    pending_depth_ = 1;
    try {
        flush();
    } catch (...) {
        // nothing is abandoned: the tail goes back behind the earlier graph, still pending (a node marked written
        // that was never launched would read as computed); the caller's error path releases the tail's outputs,
        // and the next flush sweeps it
        restore_pending(std::move(keep), nullptr);
        eager_ok_ = eager;
        throw;
    }
    pending_ = std::move(keep);
    pending_dependent_ = dependent;
    pending_depth_ = depth;
    eager_ok_ = eager;
}

// After a failed partial flush: `keep` (set aside by the split, in recording order) and what the failed flush left
// in pending_ become one graph again.  need: flush_for's closure marks over the original order (keep and pending_
// interleave by them); null: flush_tail (keep is the head, pending_ the tail).  Every node gets its index back
// in its output slot, and its producers back from the slots it holds -- run() records exactly those: one
// dependency per held input whose producer is pending -- so what flush_for resolved for a launch that did not
// complete is a dependency again.
void Engine::restore_pending(std::vector<Pending>&& keep, const std::vector<uint8_t>* need) {
    std::vector<Pending> all;
    all.reserve(keep.size() + pending_.size());
    size_t n_need = 0;
    if (need)
        for (uint8_t b : *need) n_need += b != 0;
    if (need && n_need == pending_.size() && need->size() - n_need == keep.size()) {
        size_t is = 0, ik = 0;
        for (uint8_t b : *need) all.push_back(std::move(b ? pending_[is++] : keep[ik++]));
    } else if (need) {  // the failed flush dropped nodes of the closure: closure first (it reads nothing outside itself)
        for (auto& n : pending_) all.push_back(std::move(n));
        for (auto& n : keep) all.push_back(std::move(n));
    } else {
        for (auto& n : keep) all.push_back(std::move(n));
        for (auto& n : pending_) all.push_back(std::move(n));
    }
    pending_ = std::move(all);
    for (size_t i = 0; i < pending_.size(); ++i) pending_[i].hold[0]->node = (int64_t)i;
    for (size_t i = 0; i < pending_.size(); ++i) {
        Pending& n = pending_[i];
        n.deps.clear();
        for (size_t h = 1; h < n.hold.size(); ++h) {
            const int64_t prod = n.hold[h]->node;
            if (prod >= 0 && (size_t)prod < i) n.deps.push_back((int32_t)prod);
        }
    }
    recount();
}

// flush() of the pending nodes `blocks` depend on (their ancestor closure); the others stay pending,
// their reads of launched nodes resolved.  Dead nodes are swept first (over the whole graph: a value
// released since the last flush); a closure that is the whole graph is a plain flush.  One rank only:
// under a communicator (or emulated ranks) it is a plain flush -- what it leaves pending could only be
// swept by a collective, and a rank-local read (a broadcast's root, one rank's decryption) that found
// pending work would then run one collective on its own rank.
void Engine::flush_for(const std::vector<const Block*>& blocks) {
    check_owner(blocks);
    if (pending_.empty() || gstats_ || ctx_->fanout_world() > 1 || (ctx_->attached() && ctx_->nranks > 1))
        return flush();
    sweep_dead();
    const size_t N = pending_.size();
    std::vector<uint8_t> need(N, 0);
    std::vector<int32_t> stack;
    auto mark = [&](const Block& b) {
        if (b.slot && b.slot->node >= 0 && (size_t)b.slot->node < N && !need[b.slot->node]) {
            need[b.slot->node] = 1;
            stack.push_back((int32_t)b.slot->node);
        }
    };
    for (const Block* b : blocks) {
        if (b->lazy())
            for (const Term& t : *b->lin) mark(t.b);
        else
            mark(*b);
    }
    size_t n_need = stack.size();
    while (!stack.empty()) {
        const int32_t k = stack.back();
        stack.pop_back();
        for (int32_t d : pending_[k].deps)
            if (!need[d]) {
                need[d] = 1;
                ++n_need;
                stack.push_back(d);
            }
    }
    if (n_need == N) return flush();
    if (n_need == 0) return run_before_launch();
    // split in recording order; the closure reads nothing outside itself
    std::vector<int32_t> idx(N);
    std::vector<Pending> sub, keep;
    sub.reserve(n_need);
    keep.reserve(N - n_need);
    int32_t ns = 0, nk = 0;
    for (size_t k = 0; k < N; ++k) idx[k] = need[k] ? ns++ : nk++;
    for (size_t k = 0; k < N; ++k) {
        Pending& n = pending_[k];
        std::vector<int32_t> deps;
        for (int32_t d : n.deps) {
            if (need[k]) {
                engine_check(need[d], "closure reads a node outside it");
                deps.push_back(idx[d]);
            } else if (!need[d]) {
                deps.push_back(idx[d]);  // a launched producer's output is ready: no dependency
            }
        }
        n.deps = std::move(deps);
        n.hold[0]->node = idx[k];
        (need[k] ? sub : keep).push_back(std::move(n));
    }
    pending_ = std::move(sub);
    try {
        flush();  // a host read, like a full flush: the next program's first large batch may launch
                  // eagerly (eager_ok_), once whatever stays pending has been swept as dead
    } catch (...) {
        // what stayed outside the closure is NOT abandoned (-1 means written: a value the caller still holds
        // would read as computed and return whatever its slots contain): it goes back, in recording order
        restore_pending(std::move(keep), &need);
        throw;
    }
    pending_ = std::move(keep);
    sweep_next_ = true;
    recount();
}

// Level schedule of a dependency graph (deps[i]: earlier nodes node i reads).  Returns the nodes of
// each launch level, in order; the level count is the critical path.  mode 0: backward list
// scheduling (default), 1: forward deadline-driven; levels are filled to multiples of `round`
// (one latency-kernel round: 256 bootstraps per GPU).  See Engine (engine.h).
std::vector<std::vector<int32_t>> schedule_levels(const std::vector<std::vector<int32_t>>& deps, int mode,
                                                  size_t round) {
    const size_t N = deps.size();
    std::vector<std::vector<int32_t>> lv;
    if (N == 0) return lv;
    // ASAP depth, critical path, ALAP deadlines
    std::vector<int32_t> asap(N, 1), alap(N), ndeps(N, 0);
    std::vector<std::vector<int32_t>> users(N);
    int32_t L = 0;
    for (size_t i = 0; i < N; ++i) {
        for (int32_t d : deps[i]) {
            asap[i] = std::max(asap[i], asap[d] + 1);
            users[d].push_back((int32_t)i);
        }
        ndeps[i] = (int32_t)deps[i].size();
        L = std::max(L, asap[i]);
    }
    for (size_t k = N; k-- > 0;) {
        alap[k] = L;
        for (int32_t u : users[k]) alap[k] = std::min(alap[k], alap[u] - 1);
    }
    const size_t kRound = std::max<size_t>(1, round);
    using Key = std::pair<int32_t, int32_t>;
    if (mode == 0) {
        // backward list scheduling from the last level: a level takes every candidate (all users
        // placed later) that cannot go any earlier (asap == t), then fills up to a whole round with
        // the least flexible other candidates; what does not fit lands at its earliest level, where
        // the unabsorbed throughput work forms large batches
        std::vector<int32_t> nusers(N);
        std::priority_queue<Key> cand;  // (asap, node), largest asap first
        for (size_t i = 0; i < N; ++i) {
            nusers[i] = (int32_t)users[i].size();
            if (!nusers[i]) cand.push({asap[i], (int32_t)i});
        }
        for (int32_t t = L; t >= 1; --t) {
            std::vector<int32_t> cur;
            while (!cand.empty() && cand.top().first >= t) {
                cur.push_back(cand.top().second);
                cand.pop();
            }
            const size_t cap = std::max<size_t>(1, (cur.size() + kRound - 1) / kRound) * kRound;
            while (!cand.empty() && cur.size() < cap) {
                cur.push_back(cand.top().second);
                cand.pop();
            }
            for (int32_t i : cur)
                for (int32_t d : deps[i])
                    if (--nusers[d] == 0) cand.push({asap[d], d});
            lv.push_back(std::move(cur));
        }
        engine_check(cand.empty(), "scheduler left nodes unplaced");
        std::reverse(lv.begin(), lv.end());
    } else {
        // forward list scheduling: deadline nodes always, then the most urgent ready ones up to a
        // whole round
        std::priority_queue<Key, std::vector<Key>, std::greater<Key>> ready;  // (deadline, node)
        for (size_t i = 0; i < N; ++i)
            if (!ndeps[i]) ready.push({alap[i], (int32_t)i});
        for (int32_t t = 1; !ready.empty(); ++t) {
            std::vector<int32_t> cur;
            while (!ready.empty() && ready.top().first <= t) {
                cur.push_back(ready.top().second);
                ready.pop();
            }
            const size_t cap = std::max<size_t>(1, (cur.size() + kRound - 1) / kRound) * kRound;
            while (!ready.empty() && cur.size() < cap) {
                cur.push_back(ready.top().second);
                ready.pop();
            }
            for (int32_t i : cur)
                for (int32_t u : users[i])
                    if (--ndeps[u] == 0) ready.push({alap[u], u});
            lv.push_back(std::move(cur));
        }
    }
    return lv;
}

void Engine::run_before_launch() {
    if (!before_launch_) return;
    auto f = std::move(before_launch_);
    before_launch_ = nullptr;
    f();
}

void Engine::recount() {
    pending_dependent_ = 0;
    pending_depth_ = 0;
    for (Pending& n : pending_) {
        n.depth = 1;
        for (int32_t d : n.deps) n.depth = std::max(n.depth, pending_[d].depth + 1);
        if (!n.deps.empty()) ++pending_dependent_;
        pending_depth_ = std::max(pending_depth_, n.depth);
    }
}

void Engine::sweep_dead() {
    // Dead nodes: an output slot referenced by nothing but its own node (no later node reads it, no
    // block of the program holds it -- e.g. a carry-chain state whose every consumer folded to a
    // constant on the host) can never be read, so the node is dropped; newest first, so dropping a
    // node releases its inputs and can make their producers dead in turn.
    // The output counts come from host reference counts, i.e. from how long the caller keeps its
    // handles: under a real communicator the ranks could disagree (one rank still holding an
    // intermediate), and every rank must schedule the same levels (the split, the chunk and the
    // all-gather size all follow from them).  So the ranks agree first: a node is dropped only if it
    // is dead on EVERY rank (one byte-wise min all-reduce).  The result is closed under the cascade --
    // a node kept on some rank keeps its producers' outputs referenced on that rank.
    const size_t N0 = pending_.size();
    std::vector<int32_t> remap(N0, -1);
    std::vector<uint8_t> dead(N0, 0);
    {
        // count the references without releasing any: refs[k] = holders of node k's output slot
        std::vector<long> refs(N0);
        for (size_t k = 0; k < N0; ++k) refs[k] = pending_[k].hold[0].use_count();
        for (size_t k = N0; k-- > 0;) {
            if (refs[k] != 1) continue;
            dead[k] = 1;
            for (size_t h = 1; h < pending_[k].hold.size(); ++h) {
                const int64_t prod = pending_[k].hold[h]->node;
                if (prod >= 0) --refs[prod];
            }
        }
    }
    // Only a real multi-rank communicator needs the agreement (the collective is rank-uniform: every
    // rank takes this branch or none does); at world size 1 it would only drain the stream.
    if (ctx_->attached() && ctx_->nranks > 1) {
        const int rc = ctx_->allreduce_min_u8(dead.data(), N0);
        if (rc != FHE_OK) throw EngineError(rc, std::string("dead-node agreement: ") + last_error());
    }
    for (size_t k = N0; k-- > 0;)
        if (dead[k]) pending_[k].hold.clear();
    size_t live = 0;
    for (size_t k = 0; k < N0; ++k)
        if (!dead[k]) remap[k] = (int32_t)live++;
    if (live < N0) {
        dead_nodes += N0 - live;
        std::vector<Pending> kept;
        kept.reserve(live);
        if (gstats_ && in_key_.size() == N0) {
            size_t o = 0;
            for (size_t k = 0; k < N0; ++k)
                if (!dead[k]) {
                    in_key_[o] = std::move(in_key_[k]);
                    in_deg_[o++] = in_deg_[k];
                }
            in_key_.resize(o);
            in_deg_.resize(o);
        }
        for (size_t k = 0; k < N0; ++k) {
            if (dead[k]) continue;
            Pending& n = pending_[k];
            for (int32_t& d : n.deps) {
                engine_check(remap[d] >= 0, "live node reads a dropped node");
                d = remap[d];
            }
            n.hold[0]->node = remap[k];
            kept.push_back(std::move(n));
        }
        pending_.swap(kept);
    }
    recount();  // the survivors' counters (their producers may have been launched by flush_for)
}

void Engine::flush() {
    run_before_launch();  // a deferred upload lands before anything that could read it is launched
    if (pending_.empty()) return;
    const auto f0 = std::chrono::steady_clock::now();
    if (trace_) {
        size_t grows = 0;
        double grow_ns = 0.0;
        pool_->take_growth(&grows, &grow_ns);
        fprintf(stderr, "[host] %zu run() calls, %.3f ms inside run() since the last flush (pool grown %zu x, %.3f ms)\n",
                run_calls_, run_ns_ * 1e-6, grows, grow_ns * 1e-6);
        run_ns_ = 0.0;
        run_calls_ = 0;
    }
    sweep_next_ = false;
    sweep_dead();
    if (pending_.empty()) return clear_pending();
    const size_t N = pending_.size();
    std::vector<std::vector<int32_t>> deps(N);
    for (size_t k = 0; k < N; ++k) deps[k] = pending_[k].deps;
    if (gstats_) graph_stats(deps);
    // a fanned-out level's round is one latency-kernel round on every rank
    const size_t round = (size_t)kRound * (size_t)std::max(1, ctx_->fanout_world());
    std::vector<std::vector<int32_t>> lv = schedule_levels(deps, 0, round);
    if (host_mode_ == kDry || host_mode_ == kSim) {  // the schedule's statistics, nothing launched
        // level by level, as the device loop below: a level is fingerprinted, traced and counted when it is
        // "launched", so a flush that fails at level i has counted and traced i - 1 levels, and its retry
        // (the whole graph is still pending) counts and traces those again
        auto mix = [&](uint64_t v) { fingerprint = (fingerprint ^ v) * 1099511628211ull; };
        for (auto& l : lv) {
            fault_point(kFaultLevel, "LEVEL");
            mix(l.size());
            for (int32_t k : l) {
                const Pending& pn = pending_[k];
                mix((uint64_t)k);
                mix(pn.d.lut);
                mix(pn.d.nterms);
                mix(pn.d.cst);
                if (pn.ext.empty())
                    for (uint32_t u = 0; u < pn.d.nterms && u < (uint32_t)kMaxTerms; ++u) mix((uint64_t)(int64_t)pn.d.coef[u]);
                else
                    for (const TermExt& t : pn.ext) mix((uint64_t)(int64_t)t.coef);
                for (int32_t dp : pn.deps) mix((uint64_t)(int64_t)dp);
            }
            if (ltrace_on_) {  // nothing is staged here: the pending nodes, in scheduled order
                if (trace_room(4)) ltrace_.insert(ltrace_.end(), {kTraceLevel, levels + 1, (uint64_t)l.size(), 0});
                for (int32_t k : l) {
                    const Pending& pn = pending_[k];
                    trace_op(kTraceNode, pn.d, pn.d.dst, pn.ext.empty() ? nullptr : pn.ext.data());
                }
            }
            pbs_count += l.size();
            levels += 1;
            rank_pbs += l.size();
            if (level_log.size() < kLevelLogCap) level_log.push_back((uint32_t)l.size());
        }
        return clear_pending();
    }
    // one staging copy of every level's descriptors (+ fanned-out levels' destination tables)
    const int W = ctx_->fanout_world();
    struct Shape {
        size_t G;      // bootstraps of the level
        bool split;    // fanned out over the ranks
        size_t chunk;  // bootstraps per rank (G when not split)
        size_t units;  // PbsDesc-sized units staged: the descriptors, then a split level's scatter table
    };
    std::vector<Shape> shape(lv.size());
    size_t ndesc = 0, maxchunk = 0, maxgather = 0;
    for (size_t li = 0; li < lv.size(); ++li) {
        const size_t G = lv[li].size();
        const bool split = W > 1 && G >= ctx_->fanout_min;
        const size_t chunk = split ? (G + W - 1) / W : G;
        shape[li] = {G, split, chunk, G + (split ? (G * sizeof(uint64_t*) + sizeof(PbsDesc) - 1) / sizeof(PbsDesc) : 0)};
        ndesc += shape[li].units;
        maxchunk = std::max(maxchunk, chunk);
        if (split) maxgather = std::max(maxgather, chunk * W);
    }
    // wide combinations' term tables, staged after the level descriptors (PbsDesc-sized units)
    size_t next = 0;
    for (const Pending& n : pending_) next += n.ext.size();
    const size_t ext_at = ndesc;
    ndesc += (next * sizeof(TermExt) + sizeof(PbsDesc) - 1) / sizeof(PbsDesc);
    if (maxgather) engine_check(ctx_->ensure_gather(maxgather) == FHE_OK, "gather workspace");
    fault_point(kFaultWorkspace, "WORKSPACE");
    engine_check(ctx_->ensure_ms(maxchunk) == FHE_OK, "workspace");
    engine_check(ctx_->sync_luts() == FHE_OK, "LUT upload");
    PbsDesc* dev = nullptr;
    fault_point(kFaultStage, "STAGE");
    PbsDesc* h = stage_desc(ndesc, &dev);
    std::vector<size_t> at(lv.size());
    size_t o = 0;
    TermExt* h_ext = reinterpret_cast<TermExt*>(h + ext_at);
    const TermExt* d_ext = reinterpret_cast<const TermExt*>(dev + ext_at);
    size_t eo = 0;
    for (size_t li = 0; li < lv.size(); ++li) {
        const auto [G, split, chunk, units] = shape[li];
        at[li] = o;
        uint64_t** h_scat = reinterpret_cast<uint64_t**>(h + o + G);
        for (size_t g = 0; g < G; ++g) {
            const Pending& pn = pending_[lv[li][g]];
            PbsDesc d = pn.d;
            if (!pn.ext.empty()) {
                std::copy(pn.ext.begin(), pn.ext.end(), h_ext + eo);
                d.src[0] = reinterpret_cast<const uint64_t*>(d_ext + eo);
                eo += pn.ext.size();
            }
            if (split) {
                // fanned-out levels bootstrap into the gather buffer (segment = owning rank), then scatter
                h_scat[g] = d.dst;
                d.dst = ctx_->d_gather + g * kBigCt;
            }
            h[o + g] = d;
        }
        o += units;
    }
    hip_check(hipMemcpyAsync(dev, h, ndesc * sizeof(PbsDesc), hipMemcpyHostToDevice, ctx_->stream), "desc copy");
    hip_check(hipEventRecord(desc_ev_[desc_turn_], ctx_->stream), "desc event");
    // The launch trace of one level, recorded as the level is launched (a flush that fails midway has traced what
    // it launched, and its retry traces those levels again): read back from the staged host buffer, i.e. what the
    // copy above sends -- a node's terms through its staged src[0] into the staged term tables, a split level's
    // destinations from its staged scatter table
    const size_t ext_cap = (ndesc - ext_at) * sizeof(PbsDesc) / sizeof(TermExt);
    auto trace_level = [&](size_t li) {
        const auto [G, split, chunk, units] = shape[li];
        if (trace_room(4)) ltrace_.insert(ltrace_.end(), {kTraceLevel, levels + 1, (uint64_t)G, (uint64_t)split});
        uint64_t* const* scat = reinterpret_cast<uint64_t* const*>(h + at[li] + G);
        for (size_t g = 0; g < G; ++g) {
            const PbsDesc& d = h[at[li] + g];
            const TermExt* wide = nullptr;
            if (d.nterms > (uint32_t)kMaxTerms) {
                const uintptr_t a = reinterpret_cast<uintptr_t>(d.src[0]), a0 = reinterpret_cast<uintptr_t>(d_ext);
                const size_t off = (size_t)(a - a0) / sizeof(TermExt);
                engine_check(a >= a0 && (a - a0) % sizeof(TermExt) == 0 && d.nterms <= (uint32_t)kMaxWideTerms &&
                                 off + d.nterms <= ext_cap,
                             "trace: a staged term table outside the staged copy");
                wide = h_ext + off;
            }
            trace_op(kTraceNode, d, split ? scat[g] : d.dst, wide);
        }
    };
    if (trace_)
        fprintf(stderr, "[flush] %zu nodes (%llu dropped so far), %zu levels, scheduled in %.3f ms\n", N,
                (unsigned long long)dead_nodes, lv.size(),
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - f0).count());
    for (size_t li = 0; li < lv.size(); ++li) {
        fault_point(kFaultLevel, "LEVEL");
        const auto [G, split, chunk, units] = shape[li];
        if (ltrace_on_) trace_level(li);
        PbsDesc* ld = dev + at[li];
        auto pbs = [&](size_t lo, size_t hi) {
            if (hi <= lo) return;
            hip_check(ctx_->keyswitch(nullptr, ld + lo, hi - lo), "keyswitch");
            hip_check(ctx_->blind_rotate(ld + lo, nullptr, nullptr, hi - lo), "blind rotate");
        };
        const auto t0 = std::chrono::steady_clock::now();
        if (!split) {
            pbs(0, G);
        } else {
            // own slice (every slice when ranks are emulated on one GPU)
            for (int r = 0; r < W; ++r)
                if (!ctx_->attached() || r == ctx_->rank) pbs(r * chunk, std::min(G, (r + 1) * chunk));
            if (const int rc = ctx_->allgather(ctx_->d_gather, chunk * kBigCt); rc != FHE_OK)
                throw EngineError(rc, std::string("all-gather: ") + last_error());
            hip_check(launch_scatter_blocks(ctx_->d_gather, reinterpret_cast<uint64_t* const*>(ld + G), (int)G,
                                            ctx_->stream),
                      "scatter");
            fanout_levels += 1;
        }
        ctx_->mark_progress();
        pbs_count += G;
        levels += 1;
        // this rank's bootstraps: its slice of a fanned-out level (rank 0's when ranks are emulated), else all
        const size_t r0 = ctx_->attached() ? (size_t)ctx_->rank : 0;
        rank_pbs += split ? std::min(G, (r0 + 1) * chunk) - std::min(G, r0 * chunk) : G;
        if (level_log.size() < kLevelLogCap) level_log.push_back((uint32_t)G | (split ? kLevelSplit : 0u));
        if (trace_) {
            hip_check(hipStreamSynchronize(ctx_->stream), "trace sync");
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            fprintf(stderr, "[level %llu] %zu PBS %.3f ms\n", (unsigned long long)levels, G, ms);
        }
        if (debug().nodes) {  // FHE_DEBUG=nodes: FNV-1a of every output of this level, in level order
            hip_check(hipStreamSynchronize(ctx_->stream), "nodes sync");
            std::vector<uint64_t> w(kBigCt);
            for (size_t g = 0; g < G; ++g) {
                const PbsDesc& d = h[at[li] + g];
                const uint64_t* dst = split ? reinterpret_cast<uint64_t* const*>(h + at[li] + G)[g] : d.dst;
                hip_check(hipMemcpy(w.data(), dst, kBigCt * 8, hipMemcpyDeviceToHost), "nodes copy");
                uint64_t x = 1469598103934665603ull;
                for (uint64_t v : w) x = (x ^ v) * 1099511628211ull;
                fprintf(stderr, "[node] %llu %zu %u %u %llu %016llx\n", (unsigned long long)levels, g, d.lut, d.nterms,
                        (unsigned long long)d.cst, (unsigned long long)x);
            }
        }
    }
    clear_pending();  // the stream orders any later reuse of the held slots behind these launches
}

void Engine::clear_pending() {
    for (auto& n : pending_) n.hold[0]->node = -1;
    pending_.clear();
    pending_dependent_ = 0;
    pending_depth_ = 0;
    eager_ok_ = true;
}

// FHE_GRAPH_STATS: critical-path width (nodes with zero slack, asap == alap) and two-output candidates
// (bootstraps whose input -- the same blocks, coefficients and constant -- another one also has, with
// input degree <= 7, so that a half-box LUT pair could serve both from one blind rotation)
void Engine::graph_stats(const std::vector<std::vector<int32_t>>& deps) {
    const size_t N = deps.size();
    if (in_key_.size() != N) {  // dropped dead nodes: their keys are gone from the count
        fprintf(stderr, "[graph] %zu nodes (key bookkeeping skipped after dead-node removal)\n", N);
        in_key_.clear();
        in_deg_.clear();
        return;
    }
    std::vector<int32_t> asap(N, 1), alap(N);
    std::vector<std::vector<int32_t>> users(N);
    int32_t L = 0;
    for (size_t i = 0; i < N; ++i) {
        for (int32_t d : deps[i]) {
            asap[i] = std::max(asap[i], asap[d] + 1);
            users[d].push_back((int32_t)i);
        }
        L = std::max(L, asap[i]);
    }
    std::vector<size_t> crit(L + 1, 0);
    for (size_t k = N; k-- > 0;) {
        alap[k] = L;
        for (int32_t u : users[k]) alap[k] = std::min(alap[k], alap[u] - 1);
        if (alap[k] == asap[k]) ++crit[asap[k]];
    }
    size_t ncrit = 0, maxc = 0;
    for (size_t c : crit) {
        ncrit += c;
        maxc = std::max(maxc, c);
    }
    std::map<std::string, std::pair<size_t, size_t>> groups;  // key -> (count, count with degree <= 7)
    for (size_t k = 0; k < N; ++k) {
        auto& g = groups[in_key_[k]];
        ++g.first;
        if (in_deg_[k] <= 7) ++g.second;
    }
    size_t shared = 0, pairs7 = 0;
    for (auto& kv : groups) {
        if (kv.second.first > 1) shared += kv.second.first;
        pairs7 += kv.second.second / 2;
    }
    fprintf(stderr, "[graph] %zu nodes, %d levels, critical %zu (max %zu per level), shared-input nodes %zu, "
                    "degree<=7 pairs %zu (%.1f %% of the nodes saved by two-output blind rotations)\n",
            N, L, ncrit, maxc, shared, pairs7, 100.0 * pairs7 / std::max<size_t>(1, N));
    in_key_.clear();
    in_deg_.clear();
}

// The noise label of a combination that persists (a lazy block, lincomb's output): per slot, the squared SUM of
// its coefficients times its noise -- what Engine::run computes for a descriptor, so a label never understates a
// block that names one slot twice.  The terms are slot blocks.
static uint32_t merged_label(const std::vector<Term>& terms) {
    uint64_t noise = 0;
    for (size_t i = 0; i < terms.size(); ++i) {
        bool first = true;
        int64_t coef = 0;
        for (size_t j = 0; j < terms.size(); ++j)
            if (terms[j].b.ptr() == terms[i].b.ptr()) {
                if (j < i) first = false;
                coef += terms[j].coef;
            }
        if (first) noise += (uint64_t)(coef * coef) * terms[i].b.noise;
    }
    return (uint32_t)std::min<uint64_t>(noise, 0xffffffffu);
}

Block Engine::lincomb(const std::vector<Term>& terms, uint32_t cst) {
    for (const Term& t : terms) {
        engine_check(!t.b.lazy(), "lincomb of a lazy block");
        check_owner(t.b);
    }
    flush();
    int64_t c = cst;
    std::vector<Term> live;
    for (const Term& t : terms) {
        if (t.b.trivial())
            c += (int64_t)t.coef * t.b.value;
        else if (t.coef)
            live.push_back(t);
    }
    const uint32_t noise = merged_label(live);
    bool ok;
    const uint64_t reach = reachable(live, c, &ok);
    engine_check(ok && !beyond(reach, ctx_->p.msg_carry()), "linear combination out of range");
    uint32_t hi = 63 - __builtin_clzll(reach);
    if (live.empty()) return Block::make_trivial((uint32_t)c);
    engine_check(live.size() <= (size_t)kMaxTerms, "linear combination of more terms than a descriptor holds");
    Block b;
    b.degree = hi;
    b.noise = noise;
    b.slot = pool_->alloc();
    PbsDesc* dev = nullptr;
    PbsDesc* h = stage_desc(1, &dev);
    PbsDesc d;
    std::memset(&d, 0, sizeof d);
    for (size_t t = 0; t < live.size(); ++t) {
        d.src[t] = live[t].b.ptr();
        d.coef[t] = live[t].coef;
    }
    d.nterms = (uint32_t)live.size();
    d.cst = (uint64_t)c * ctx_->p.delta();
    d.dst = b.slot->p;
    h[0] = d;
    if (ltrace_on_) trace_op(kTraceLincomb, h[0], h[0].dst, nullptr);
    hip_check(hipMemcpyAsync(dev, h, sizeof(PbsDesc), hipMemcpyHostToDevice, ctx_->stream), "desc copy");
    hip_check(hipEventRecord(desc_ev_[desc_turn_], ctx_->stream), "desc event");
    hip_check(launch_lincomb(dev, 1, ctx_->stream), "lincomb");
    return b;
}

Block block_lazy(const std::vector<Term>& terms, int32_t cst, uint32_t degree) {
    auto lin = std::make_shared<std::vector<Term>>();
    Block b;
    b.degree = degree;
    for (const Term& t : terms) {
        if (t.coef == 0) continue;
        engine_check(!t.b.lazy(), "nested lazy block");
        if (t.b.trivial()) {
            cst += t.coef * (int32_t)t.b.value;
            continue;
        }
        lin->push_back(t);
    }
    b.noise = merged_label(*lin);
    if (lin->empty()) {
        engine_check(cst >= 0 && (uint32_t)cst <= degree, "lazy constant out of its range");
        return Block::make_trivial((uint32_t)cst);
    }
    b.lin = std::move(lin);
    b.lin_cst = cst;
    return b;
}

}  // namespace fhe
