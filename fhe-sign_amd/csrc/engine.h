// engine.h -- blocks, the block pool and the engine that executes bootstraps on them (engine.cpp,
// engine_ops.cpp); the radix integers built from blocks are radix.h.
//
// A block is a 2-bit message + 2-bit carry space in a big-key LWE in a fixed-size device slot.
// Host-side metadata per block:
//   degree   -- largest plaintext the block can hold (public, from the op structure)
//   noise    -- variance in units of one fresh bootstrap output
//   trivial  -- a publicly known value with no device storage (zero-extension, masks, constants)
// Every bootstrap is a PbsItem: LUT( sum coef_t * block_t + cst ).  Items of one dependency level
// run as ONE batched keyswitch (with the linear combination fused in) + ONE blind-rotate launch.
// Items whose LUT is constant over the reachable inputs fold to trivial blocks on the host.
#pragma once
#include <atomic>
#include <cstdint>
#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <unordered_map>
#include <vector>

#include "context.h"
#include "kernels.h"
#include "public_key.h"

struct fhe_switched_list;  // switched.h

namespace fhe {

constexpr uint32_t kMsgBits = 2;
constexpr uint32_t kMsgMod = 4;
// Params::radix_space() (keys.h) is the predicate of these two: a key of any other message space bootstraps raw
// blocks on this engine, and every radix entry point refuses it at the door
static_assert(kMsgMod == 1u << kMsgBits && kMsgMod == 4, "Params::radix_space() states message_modulus 4, carry_modulus 4");
constexpr uint32_t kMaxNoise = 25;  // variance units (sigma <= 5 fresh sigmas, tfhe-rs 2_2 max noise level 5)

// Size rules of the radix algorithms that tests move (fhe_host_set_tuning; process-wide, set before
// an op runs).  The defaults are the product; a test lowers a threshold so that a small CPU or GPU
// case takes the code path the product takes at 256 bits.  No environment variable is read on an op
// path (engine diagnostics: FHE_DEBUG, read once per process, below).
struct Tuning {
    uint32_t kara_min = 24;         // Karatsuba for full products of >= this many live blocks (0: never)
    uint32_t kara_compat_min = 16;  // ... for the compat chain's 16-block limb products (0: never)
    bool kara_force = false;        // split publicly known operands too (the host-folding algebra checks)
    uint32_t div_r16_lead = 32;     // encrypted division: leading dividend blocks taken in radix-16 steps
    int scalar_div_residue = -1;    // public divisors: -1 size rule (dividends >= 64 blocks), 0 never, 1 where valid
    uint32_t flush_depth = 64;      // flush the deferred graph once it is this many levels deep (0: only on demand)
    // Host-side fault point (test hook, off by default; fault_point below): a mask of kFault* sites, the crossing
    // that throws (0: none), and the crossings of enabled sites since fault_after was last set
    uint32_t fault_sites = 0;
    uint64_t fault_after = 0;
    uint64_t fault_crossings = 0;
};
Tuning& tuning();
// The fault sites (FHE_TUNE_FAULT_SITES), all in engine code, one integer test per level or per call.  An enabled
// site counts its crossings; the fault_after-th one throws EngineError(FHE_ERR_HIP, "injected fault at <site>") and
// disarms.  It only throws on the host: no HIP call, synchronisation or launch argument is skipped or altered.
enum : uint32_t {
    kFaultLevel = 1,      // the top of each level's iteration in Engine::flush (device and host modes)
    kFaultStage = 2,      // before the level descriptors are staged (device)
    kFaultWorkspace = 4,  // before the bootstrap workspace is sized (device)
    kFaultDeferred = 8,   // first statement of upload_deferred's closure
    kFaultRecord = 16,    // the entry of Engine::run
    kFaultClient = 32,    // encrypt_resident before it stages anything; phases_many after its flush, before its launch
};
void fault_cross(const char* site);
inline void fault_point(uint32_t site, const char* name) {
    if (tuning().fault_sites & site) fault_cross(name);
}
// Engine diagnostics on stderr, read once per process from FHE_DEBUG (comma-separated): levels (sync and
// time every level), graph (graph statistics), chain (compat chain phases, flushed), chain-host (the
// same, host time only), residue (the residue split's phases), nodes (a hash of every launched
// bootstrap's output, per level: cross-run / cross-rank comparisons)
struct Debug {
    bool levels = false, graph = false, chain = false, chain_host = false, residue = false, nodes = false;
};
const Debug& debug();

class BlockPool;

struct Slot {
    uint64_t* p = nullptr;
    std::shared_ptr<BlockPool> pool;  // the maker's pool: kept alive by the slot, and the slot's owner (Engine::owns)
    int64_t node = -1;  // index of the pending bootstrap that writes this slot (Engine::flush), or -1
    ~Slot();
};

struct Term;

struct Block {
    std::shared_ptr<Slot> slot;  // null => trivial (or lazy)
    uint32_t value = 0;          // trivial value
    uint32_t degree = 0;
    uint32_t noise = 0;
    // lazy: an un-bootstrapped linear combination sum coef * block + lin_cst of slot blocks whose
    // value is known from the op structure to lie in [0, degree] (block_lazy); only ever a PBS
    // input term, flattened into the descriptor by Engine::run
    std::shared_ptr<const std::vector<Term>> lin;
    int32_t lin_cst = 0;
    // trivial only: the block stands for value - 1/2 (a sign lookup's known output, raw items only)
    bool half_neg = false;
    bool trivial() const { return !slot && !lin; }
    bool lazy() const { return (bool)lin; }
    const uint64_t* ptr() const { return slot ? slot->p : nullptr; }
    static Block make_trivial(uint32_t v) {
        Block b;
        b.value = v;
        b.degree = v;
        return b;
    }
};

using Blocks = std::vector<Block>;

class BlockPool : public std::enable_shared_from_this<BlockPool> {
public:
    explicit BlockPool(int device, bool dry = false) : device_(device), dry_(dry) {}
    ~BlockPool();
    std::shared_ptr<Slot> alloc();
    void release(uint64_t* p) {
        if (!dry_) free_.push_back(p);  // placeholder addresses are never handed out twice
    }
    size_t live() const { return total_ - free_.size(); }
    // growth since the last call (the level trace prints it with the host time of run()); per pool:
    // contexts on other threads grow their own
    void take_growth(size_t* grows, double* ns) {
        *grows = grows_, *ns = grow_ns_;
        grows_ = 0, grow_ns_ = 0.0;
    }

private:
    int device_;
    bool dry_;                // Engine kDry: slots are distinct placeholder addresses, never dereferenced
    uintptr_t dry_next_ = 0x10000;
    std::vector<DeviceBuf<uint64_t>> chunks_;
    std::vector<uint64_t*> free_;
    size_t total_ = 0;
    size_t grows_ = 0;
    double grow_ns_ = 0.0;
};

struct Term {
    Block b;
    int32_t coef;
};

// Lazy block of the given semantic range [0, degree] (caller's guarantee; noise = sum coef^2 noise, a slot
// named twice counted with its coefficients summed).
Block block_lazy(const std::vector<Term>& terms, int32_t cst, uint32_t degree);

struct PbsItem {
    std::vector<Term> terms;
    uint32_t cst = 0;             // plaintext constant (units of one message step)
    std::vector<uint32_t> table;  // LUT over [0, msg*carry)
    // Raw items (the compat mul's carry-count chain, csrc/biguint.cpp): the caller guarantees the
    // input's actual value lies in [-16, 16) (message steps; [-16, 0) reaches the negacyclic half of
    // the blind rotation, where the output is -f(v + 16)).  No folding and no degree check; the LUT
    // is `half_table` (16 outputs f(0..15) in units of HALF a message step) and `half_cst` (half steps,
    // signed) is added to `cst`.  Output block: degree `raw_degree`, fresh noise.  Up to
    // kMaxWideTerms input terms (ordinary items: kMaxTerms).
    bool raw = false;
    std::vector<int32_t> half_table;
    int32_t half_cst = 0;
    uint32_t raw_degree = 3;
};

// Executes PBS items on a context as a deferred dependency graph.  run() does the host-side
// bookkeeping at once (trivial folding, degrees, noise, output slots) and records each remaining
// bootstrap as a pending node that depends on the pending producers of its inputs; flush() (called
// before any host read: sync, download, lincomb) schedules all pending nodes into launch levels
// and runs them.  Scheduling: as-late-as-possible deadlines from the critical path, each level
// takes every node at its deadline and fills up to the next whole round of the latency kernel (a
// multiple of 256) with the most urgent ready nodes -- work off the critical path (e.g. the
// products a later window add needs) rides in the idle CUs of latency-bound levels.  The level
// count equals the critical path.
class Engine {
public:
    // Host modes (no device work; the CPU tests and graph statistics):
    //   kHostFold -- every item must fold on the host (trivial inputs): radix algorithms evaluated on
    //                publicly known values (fhe_host_biguint_mul);
    //   kDry      -- items on dry_block() inputs are recorded and scheduled like the real thing, nothing
    //                is launched: levels and bootstrap counts of an op (fhe_host_biguint_mul_stats).
    //   kSim      -- kDry plus a plaintext shadow: sim_block() inputs carry a value the algorithms
    //                cannot see (they take every encrypted path), each bootstrap is evaluated on the
    //                host from its LUT (raw items by their negacyclic half rule) and checked to stay in
    //                its input range -- the radix algorithms' end-to-end results on the CPU
    //                (fhe_host_sim_*), with the degree / noise bookkeeping of the real thing.
    enum HostMode { kDevice = 0, kHostFold = 1, kDry = 2, kSim = 3 };
    explicit Engine(fhe_ctx* ctx, int host_mode = kDevice);
    // kDry / kSim: an "encrypted" block of the given degree (a placeholder slot)
    Block dry_block(uint32_t degree);
    // kSim: an "encrypted" block holding `value`; sim_value: a block's plaintext in half message steps
    Block sim_block(uint32_t value, uint32_t degree);
    int64_t sim_half2(const Block& b) const;
    // diagnostics: the dependency depth (levels) of a pending block's producer, 0 if none is pending
    int32_t depth_of(const Block& b) const;
    // Ownership: a slot block (a lazy block: each of its terms) belongs to the engine whose pool made its slot,
    // and only there do its address, its pending node index and (kSim) its plaintext shadow mean anything.
    // Every block that enters an engine passes check_owner first -- one pointer comparison per slot -- and a
    // foreign one is refused with FHE_ERR_INVALID before anything is recorded, staged, launched or read
    // (`operand`: the entry point's name for it, when the C layer knows it).  Trivial blocks have no owner.
    bool owns(const Block& b) const;
    void check_owner(const Block& b, const char* operand = nullptr) const;
    void check_owner(const std::vector<const Block*>& blocks, const char* operand = nullptr) const;
    ~Engine();
    fhe_ctx* ctx() const { return ctx_; }
    // Records one dependency level of items; returns one output block per item (possibly trivial).
    // Throws on error.
    Blocks run(std::vector<PbsItem>& items);
    // Schedules and launches every pending bootstrap (asynchronously on the context's stream).
    void flush();
    // Schedules and launches only the pending bootstraps the given blocks (lazy ones: their terms)
    // depend on; the rest stay pending with their dependencies on the launched ones resolved (a
    // decryption that reads a value's column form leaves the value's normalization pending -- dead,
    // and dropped before the next recording, once the caller releases the value).
    void flush_for(const std::vector<const Block*>& blocks);
    // Linear combination without bootstrap (caller guarantees degree/noise stay legal).
    Block lincomb(const std::vector<Term>& terms, uint32_t cst);
    // Upload client-encrypted blocks.
    Block upload(const uint64_t* ct, uint32_t degree);
    // n client-encrypted blocks (contiguous big LWEs): one copy + one scatter into their slots
    Blocks upload_many(const uint64_t* cts, size_t n, uint32_t degree);
    // Deferred upload: n fresh slots now (degree, noise 1), their ciphertexts later.  `fill` produces the
    // n contiguous big LWEs (e.g. a host encryption still running on another thread); it is called, and
    // its result uploaded into the slots, right before the next flush launches anything -- so the graph
    // that reads the slots is recorded while the ciphertexts are being made, and the upload still
    // precedes every launch on the stream.  One pending deferred upload at a time.
    // A closure that throws (its fill() included) is gone with the error: the engine is left without an armed
    // upload, and whatever reads the slots belongs to the failed call.
    Blocks upload_deferred(size_t n, uint32_t degree, std::function<std::vector<uint64_t>()> fill);
    // Drops an armed deferred upload without running it, and waits for what it holds: the closure owns its
    // producer (the helper thread's future, whose release joins the thread), so on return nothing of it runs.
    // The slots are never written; the caller's error path owns every value that reads them.
    void cancel_deferred() { before_launch_ = nullptr; }
    bool deferred_armed() const { return (bool)before_launch_; }
    size_t pending_nodes() const { return pending_.size(); }
    // helper jobs in flight (biguint_encrypt_batch's encryption threads): counted up where one is started, down
    // as its last statement; shared with the thread, which may finish after a cancelled closure is gone
    std::shared_ptr<std::atomic<uint32_t>> helper_jobs = std::make_shared<std::atomic<uint32_t>>(0);
    // A seeded ciphertext's blocks (fhe_seeded: public mask seed + one body per block) expanded on the
    // device: n fresh slots (degree 3, noise 1, as upload_many's), only the slot pointers and the bodies
    // (16 B per block) staged through the upload buffer, the masks regenerated by seeded.hip into the
    // slots -- word for word expand_seeded_host's output.  Stream-ordered like an upload: the slots are
    // new, so nothing recorded in the deferred graph reads them; no flush, and a pending upload_deferred
    // stays pending (it stages its own data when it runs).  Device engines only: the host modes (kDry,
    // kSim, kHostFold) refuse, as they have no ciphertexts to expand into.  Issues no collective: it is
    // deterministic and rank-local, so under an attached communicator EVERY rank must expand the same
    // bytes (the fan-out's identical-inputs rule).
    Blocks expand_seeded(const uint8_t seed[32], const uint64_t* bodies, size_t n);
    // Compressed computed ciphertexts (compress.h).  compress: the blocks (slot or trivial; a trivial block goes
    // through as the ciphertext (0, b)) -> the packed 12-bit GLWE streams, CompParams::packed_bytes(n) bytes,
    // byte for byte pack_keyswitch_host's output.  Flushes like a download (a plain flush: rank-local under a
    // communicator, no collective), then digits, matrix-core contraction, rotate / switch / pack, one copy
    // back.  decompress: n fresh slots (noise 1, degrees from the list), stream-ordered like expand_seeded --
    // no flush, no collective: the unpack + sample-extract kernel, then the blind rotate under the
    // decompression key with the identity table.  Device engines with a compression key only.
    void compress(const std::vector<const Block*>& blocks, uint8_t* packed);
    Blocks decompress(const fhe_compressed_list& x);
    // the unpack + sample-extract kernel alone: n x (k' N' + 1) words to the host (tests)
    void extract_rows(const fhe_compressed_list& x, uint64_t* rows);
    // the packing keyswitch alone over n host rows of 2049 words, launched as compress launches it: the
    // contraction's n x (k' + 1) N' words and the n bodies to the host (tests)
    void pack_keyswitch_words(const uint64_t* cts, size_t n, uint64_t* P, uint64_t* body);
    // A compact ciphertext list's value (public_key.h) expanded on the device, as expand_seeded is: fresh
    // slots, the touched chunks' C_A (16 KB each), the bodies and the slot pointers staged through the upload
    // buffer, public_key.hip's sample extraction into the slots -- word for word expand_compact_host's rows.
    // Stream-ordered like an upload: no flush, no collective (under a communicator every rank expands the same
    // bytes).  Unpacked: the extracted blocks are the result (degree 3, noise 1).  Packed: a coefficient holds
    // m_2i + 4 m_(2i+1) at degree 15, noise 1, and goes through run() as two items, x & 3 and x >> 2 -- recorded
    // in the deferred graph, where they share levels with whatever else is pending; a lone last block (degree 3)
    // folds to an alias by run()'s identity rule.  Device engines only.
    Blocks expand_compact(const fhe_compact_list& x, size_t value);
    // the extraction kernel alone over every coefficient of the list: ncoef x 2049 words to the host (tests)
    void extract_compact_rows(const fhe_compact_list& x, uint64_t* rows);
    // Re-randomization under the installed public key (public_key.h, fhe_set_public_key), staged as
    // compact_extract: block i of the result = block i of `blocks` + the sample extraction, at coefficient i, of
    // the zero encryptions the 32-byte seed defines -- word for word rerandomize_host of the blocks' exported
    // rows.  Out of place: fresh slots, the sources untouched.  Pending producers of the blocks are launched
    // first (flush_for; under a communicator that is the plain flush a decryption makes), a lazy block is made
    // real by lincomb, a trivial block enters as the ciphertext (0, delta value).  Only the seed and the slot
    // pointers (24 B per block) are staged; rerandomize.hip makes the zero encryptions and adds them.
    // Stream-ordered, no collective of its own: under a communicator every rank passes the same seed and
    // computes the same words.  Degree and noise label of a block are unchanged (the added error is below
    // 2^30, against 2^49.7 of a bootstrap's output); a trivial block becomes a slot block of degree
    // max(value, 3) with no known-value shortcut left.  Device engines with a public key only.
    Blocks rerandomize(const std::vector<const Block*>& blocks, const uint8_t seed[32]);
    // Row digests of the blocks on the device (ct_digest.h), its inputs made real as rerandomize's: out = 32 bytes per block,
    // word for word ct_digest_host of the blocks' exported rows.  Pending producers of the blocks are launched
    // first (flush_for), a lazy block is made real by lincomb, a trivial block enters as the row (0, delta
    // value).  One 16-byte entry per block is staged, one kernel, one download of 32 n bytes, one wait; the
    // blocks are untouched.  No collective of its own: every rank hashes its own replica.  meta (optional): per
    // block the value digest's fields -- tag 1, degree, noise label of a ciphertext (a lazy block: as made
    // real), tag 0, the value, 0 of a trivial block.  Device engines only.
    struct DigestMeta {
        uint8_t tag;
        uint32_t degree, noise;
    };
    void digest(const std::vector<const Block*>& blocks, uint8_t* out, std::vector<DigestMeta>* meta = nullptr);
    // Oblivious pseudo-random blocks (oprf.h): block b < count = the bootstrap of row b of the PUBLIC 32-byte
    // seed through the `bits`-bit staircase, degree 2^bits - 1, noise 1; with tail_bits != 0 one more block, row
    // `count` at tail_bits (a radix value's odd top bit).  Eager, like decompress: fresh slots, the row
    // kernel into the bootstrap workspace, descriptors without terms, the blind rotation under the main key set
    // (the kernel chosen by count, as for any level), the body constant -- all on the context's stream behind
    // whatever is launched.  No keyswitch, no upload, no flush: pending deferred nodes stay pending, and the
    // workspace they will use is theirs again once this is through (stream order).  Counts above the workspace
    // go in chunks.  No collective: it is deterministic, every rank (and every emulated one) computes every
    // block.  Independent of fhe_ctx_set_modulus_switch: the rows are not centered, their phase is the
    // randomness.  Device engines only.
    Blocks oprf(const uint8_t seed[32], size_t count, uint32_t bits, uint32_t tail_bits = 0);
    // Modulus-switched stored ciphertexts (switched.h).  switched_compress: the blocks -> their stored rows, n x
    // switched_row_bytes(p.n) bytes, byte for byte fhe_switched_compress_host of the blocks' exported rows in
    // the context's modulus-switch mode.  Inputs made real as rerandomize's (pending producers launched: a plain
    // flush, rank-local under a communicator; a lazy block combined; a trivial block enters as (0, delta value));
    // a block whose noise label admits no lookup (> kMaxNoise) is refused.  In chunks of the bootstrap workspace
    // as it stands (oprf's rule): the context's keyswitch through one-term descriptors, k_ms_pack, one download.
    // switched_decompress: n fresh slots (noise 1, degrees from the list), stream-ordered like decompress -- no
    // flush, no collective: upload, k_ms_unpack into the workspace, the blind rotation under the main key set with
    // the identity table; no keyswitch and no k_ms_center, whatever the mode.  Device engines only.
    // rekey: the keyswitch runs under the installed re-keying key (fhe_set_rekey_key) into its own workspace, and
    // the rows are the destination key's: switched_row_bytes(rkp.n) bytes each.
    void switched_compress(const std::vector<const Block*>& blocks, uint8_t* rows, bool rekey = false);
    Blocks switched_decompress(const fhe_switched_list& x);
    // Client-key encryption on the device under the context's resident key (client_ops.h; the caller
    // has checked fhe_ctx::client_resident(ck)): n fresh slots (degree 3, noise 1, as upload_many's) filled by
    // client_ops.hip with, word for word, what encrypt_big_many(ck, pts, n, ..) writes.  ck's stream is moved past
    // the n encryptions first (encrypt_big_skip), then the kFaultClient site is crossed, then the slot pointers and
    // the scaled plaintexts (16 B per block) and the stream's parameters are staged: a call that fails later leaves
    // the stream where the host path's failed upload leaves it.  Stream-ordered like expand_seeded: no flush, a
    // pending upload_deferred stays pending, no collective.  False, with nothing changed, if the batch leaves the
    // stream's counter epoch: the caller takes the host path.
    bool encrypt_resident(fhe_client_key* ck, const uint64_t* pts, size_t n, Blocks* out);
    // The decryption phases body - <mask, key> of slot blocks under the resident key, one u64 per block: the same
    // flush or flush_for as download_many, the kFaultClient site, the slot pointers staged, client_ops.hip's phase
    // kernel, one copy of 8 n bytes, one wait.  Word for word decrypt_phase_big of the blocks' rows.
    void phases_many(const std::vector<const Block*>& blocks, uint64_t* phases, bool only_needed = false);
    void download(const Block& b, uint64_t* ct);
    // the slot blocks' ciphertexts -> host, contiguous (one gather + one copy + one wait instead of a
    // round trip per block: the decryption of a 256-bit result is 128-144 blocks)
    // (only_needed: flush_for(blocks) instead of flush())
    void download_many(const std::vector<const Block*>& blocks, uint64_t* cts, bool only_needed = false);
    // n big LWEs contiguous in device memory -> fresh slots (one scatter); degree/noise set by the caller
    Blocks adopt_device(const uint64_t* d_cts, size_t n);
    // the slot blocks' ciphertexts -> contiguous device buffer (one gather; flushes first)
    void gather_device(const std::vector<const Block*>& blocks, uint64_t* d_out);
    void sync();
    static constexpr size_t kEagerHead = 3072;  // 4 rounds of the throughput kernel (3 x 256 CUs)
    // nothing pending and no eager batch since the last flush (radix_mul_many's early head launch)
    bool eager_head_ok() {
        settle();
        return eager_ok_ && pending_.empty();
    }
    // one-shot, before each program of a batch of independent programs recorded back to back
    // (fhe_schnorr_sign_fhe_with_k0_batch): the program's first large batch of bootstraps that reads
    // nothing pending (its block products) is launched as soon as it is recorded
    void eager_next_batch(bool on) { eager_batch_next_ = on; }
    // statistics
    uint64_t pbs_count = 0, levels = 0, fanout_levels = 0;
    uint64_t dead_nodes = 0;  // recorded bootstraps dropped at flush: nothing could read their outputs
    // bootstraps per launched level, in launch order (fhe_ctx_level_log; the bench's CPU replay);
    // kLevelSplit marks a level fanned out over the ranks (fan-out only, never at world size 1)
    std::vector<uint32_t> level_log;
    static constexpr uint32_t kLevelSplit = 1u << 31;
    uint64_t rank_pbs = 0;  // bootstraps this rank ran itself (fanned-out levels: its slice)
    // The noise budget as enforced, over the recorded bootstraps since the last reset (fhe_ctx_noise_audit).
    // label: sum coef^2 noise over an item's terms, which treats them as independent; merged: per slot of the
    // descriptor the squared sum of its coefficients times its noise -- the variance of what is launched, and the
    // figure run() holds against kMaxNoise.  They differ where an item names one slot twice.
    struct NoiseAudit {
        uint64_t max_label = 0, max_merged = 0;
        uint64_t n_above_label = 0;  // items whose merged noise exceeds their label
    } audit;
    // kDry / kSim: FNV-1a over every scheduled level's nodes in order (LUT, terms' coefficients, constant,
    // producers by recording index) -- no addresses.  Equal across processes iff the program records
    // the same graph in the same order, which the fan-out's split relies on (every rank scatters the
    // gathered slices by its own node order)
    uint64_t fingerprint = 1469598103934665603ull;
    static constexpr size_t kLevelLogCap = 1u << 20;
    // Launch trace (test hook, fhe_ctx_trace / fhe_ctx_trace_read; off by default: one branch per flush and per
    // eager op): what is enqueued on the stream, in that order, as a flat stream of u64 records
    //   kTraceLevel   level number, bootstraps, split flag -- followed by one node record per bootstrap, in launch order
    //   kTraceNode    dst, LUT id, cst, nterms, then nterms x (src, coefficient as int64)
    //   kTraceLincomb dst, cst, nterms, then nterms x (src, coefficient)
    //   kTraceWrite   kind (kWrite*), n, then n destination addresses
    // A device engine reads a node's fields back from the staged host copy of what goes to the device (the level's
    // descriptors, a wide combination's staged TermExt table through the staged src[0], a split level's scatter
    // table); the dry and simulated modes, which stage nothing, record from the pending nodes in scheduled order.
    // At most kTraceCap words are kept; a record that would pass them sets the overflow flag instead.
    enum : uint64_t { kTraceLevel = 1, kTraceNode = 2, kTraceLincomb = 3, kTraceWrite = 4 };
    enum : uint64_t { kWriteUpload = 0, kWriteDeferred = 1, kWriteOpaque = 2 };
    static constexpr size_t kTraceCap = (size_t)1 << 23;  // 64 MiB
    void trace_enable(bool on) { ltrace_on_ = on; }
    bool trace_overflowed() const { return ltrace_overflow_; }
    const std::vector<uint64_t>& trace_words() const { return ltrace_; }
    void trace_reset() {
        ltrace_.clear();
        ltrace_overflow_ = false;
    }

private:
    fhe_ctx* ctx_;
    int host_mode_ = kDevice;
    std::unordered_map<const uint64_t*, int64_t> sim_;  // kSim: slot -> plaintext (half steps)
    std::shared_ptr<BlockPool> pool_;
    DeviceBuf<uint64_t> d_up_;  // upload / download staging, carved by engine_ops.cpp's cursor
    uint64_t* staging(size_t words);
    // n blocks in fresh slots (noise 1), one degree for all or one per block; write_kind: the launch trace's
    // record of the op that fills them (-1: the caller records it itself, when the write is enqueued)
    Blocks fresh_blocks(size_t n, uint32_t degree, int write_kind = (int)kWriteOpaque);
    Blocks fresh_blocks(const std::vector<uint32_t>& degrees, int write_kind = (int)kWriteOpaque);
    // launch trace (above)
    bool ltrace_on_ = false, ltrace_overflow_ = false;
    std::vector<uint64_t> ltrace_;
    bool trace_room(size_t words);
    void trace_write(uint64_t kind, uint64_t* const* dst, size_t n);
    void trace_op(uint64_t tag, const PbsDesc& d, const uint64_t* dst, const TermExt* wide);
    // dst.size() contiguous host ciphertexts into the slots: two copies, one scatter, one stream sync
    void scatter_upload(const uint64_t* cts, const std::vector<uint64_t*>& dst);
    bool trace_ = false;
    // FHE_GRAPH_STATS=1: per flush, the critical-path width and the bootstraps that share their exact
    // input with another one at input degree <= 7 (two-output blind rotation candidates); stderr
    bool gstats_ = false;
    std::vector<uint8_t> in_deg_;              // gstats_: max input value of each pending node
    std::vector<std::string> in_key_;          // gstats_: the node's input (terms + constant)
    static constexpr int kRound = 256;  // level fill granule: one latency round (a ciphertext per CU)
    double run_ns_ = 0.0;  // host time inside run() (trace)
    size_t run_calls_ = 0;
    static constexpr size_t kEagerBatch = 4096;
    bool eager_ok_ = true;
    bool eager_batch_next_ = false;
    std::function<void()> before_launch_;  // upload_deferred's pending upload (run at the next flush)
    void run_before_launch();
    struct Pending {
        PbsDesc d;
        std::vector<std::shared_ptr<Slot>> hold;  // [0] output, then inputs: alive until launched
        std::vector<int32_t> deps;                // pending producers of the inputs
        std::vector<TermExt> ext;                 // terms of a wide combination (d.nterms > kMaxTerms)
        int32_t depth = 1;                        // 1 + the deepest pending producer (diagnostics)
    };
    std::vector<Pending> pending_;
    size_t pending_dependent_ = 0;  // pending nodes with at least one pending producer
    int32_t pending_depth_ = 0;     // the deepest pending node (levels of the graph recorded so far)
    PinnedBuf<PbsDesc> h_desc_[2];  // pinned, double-buffered
    hipEvent_t desc_ev_[2] = {nullptr, nullptr};
    size_t desc_cap_ = 0;  // of h_desc_; 0 while either is not grown
    int desc_turn_ = 0;
    DeviceBuf<PbsDesc> d_desc_;
    // the eager ops' descriptors (oprf, the stored form), one chunk (the level descriptors above may be in flight)
    DeviceBuf<PbsDesc> d_oprf_desc_;
    void ensure_eager_desc(size_t chunk);
    DeviceBuf<uint32_t> d_sw_packed_;  // the stored form's packed rows, one chunk (switched.h)
    void ensure_desc(size_t n);
    void graph_stats(const std::vector<std::vector<int32_t>>& deps);
    void flush_tail(size_t k0);
    // a failed partial flush (flush_for, flush_tail): the nodes set aside go back into pending_ with what the
    // failed flush left there -- indices, producers and counters as if the split had not been made
    void restore_pending(std::vector<Pending>&& first_or_keep, const std::vector<uint8_t>* need);
    // drop the dead pending nodes (flush's first step; ranks agree by an all-reduce)
    void sweep_dead();
    void recount();  // pending_dependent_ / pending_depth_ / depths from pending_'s deps
    void clear_pending();  // flush's end: every node launched (or scheduled dry), the next batch may go eagerly
    bool sweep_next_ = false;  // flush_for left nodes pending: sweep them before the next recording
    void settle() {
        if (sweep_next_) {
            sweep_next_ = false;
            sweep_dead();
        }
    }
    PbsDesc* stage_desc(size_t n, PbsDesc** dev);
    // coefficients [first, first + n) of x sample-extracted into fresh slots (degrees as given, noise 1)
    Blocks compact_extract(const fhe_compact_list& x, size_t first, size_t n, const std::vector<uint32_t>& degrees);
};

void engine_check(bool ok, const char* what);
// a HIP status / a bounded stream wait (fhe_ctx::wait_stream) that failed: EngineError with its C-ABI status
void hip_check(hipError_t e, const char* what);
void wait_check(fhe_ctx* c, const char* what);
// 2 x the value a trivial block stands for (half_neg: value - 1/2)
inline int64_t trivial_half2(const Block& b) { return 2 * (int64_t)b.value - (b.half_neg ? 1 : 0); }
// An engine failure that carries its C-ABI status (e.g. FHE_ERR_TIMEOUT from a bounded stream wait):
// the C entry points return `code` instead of the generic FHE_ERR_INVALID.
struct EngineError : std::runtime_error {
    int code;
    EngineError(int c, const std::string& what) : std::runtime_error(what), code(c) {}
};
// The Engine's level scheduler (deps[i]: earlier nodes node i reads; mode 0 backward, 1 forward).
std::vector<std::vector<int32_t>> schedule_levels(const std::vector<std::vector<int32_t>>& deps, int mode,
                                                  size_t round = 256);

}  // namespace fhe
