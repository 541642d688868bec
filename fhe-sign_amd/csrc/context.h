// context.h -- per-thread device context: GPU stream, installed server key, LUT registry,
// PBS workspace.  The analogue of tfhe-rs's thread-local server key (src/schnorr.rs:443).  Every device
// buffer is a DeviceBuf (device_buf.h), the keys are key sets (key_sets.h) and every workspace is a group of
// buffers under one capacity (GroupCap, RowSpace): the context's destructor and the release_* functions wait,
// then the members free themselves.
#pragma once
#include <hip/hip_runtime.h>

#include <map>
#include <string>
#include <vector>

#include "compress.h"
#include "device_buf.h"
#include "key_sets.h"
#include "keys.h"
#include "kernels.h"

struct fhe_ctx;

namespace fhe {

class Engine;
void set_error(const std::string& msg);
const char* last_error();
// FHE_OK on a device context; on a simulated one FHE_ERR_INVALID with a message that names it and `what`
int refuse_simulated(const fhe_ctx* c, const char* what);
// FHE_OK if the context's installed key is of the radix layer's message space (Params::radix_space) or no key is
// installed (the entry point's own checks answer that); else FHE_ERR_INVALID with radix_space_refusal's text
int radix_space_check(const fhe_ctx* c);
#define FHE_HIP_CHECK(expr)                                                                   \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess) {                                                               \
            ::fhe::set_error(std::string(#expr) + ": " + hipGetErrorString(_e));              \
            return FHE_ERR_HIP;                                                               \
        }                                                                                     \
    } while (0)

// Host-side FFT tables (bit-identical to oracle/tfhe_oracle.c:fho_tables_init).
void fft_tables(std::vector<double2>* W, std::vector<double2>* psi);
// Per-lane twiddle table [slot][lane] (device_math.h:tw_slot) built from W.
void lane_twiddles(const std::vector<double2>& W, std::vector<double2>* Wl);
// Per-thread tables of the wide (latency) blind rotate: tw[12][256], psi[4][256] (br_wide.hip).
void quad_tables(const std::vector<double2>& W, const std::vector<double2>& psi, std::vector<double2>* tw,
                 std::vector<double2>* ps);
void wide_tables(const std::vector<double2>& W, const std::vector<double2>& psi, std::vector<double2>* tw,
                 std::vector<double2>* psiw);
// Accumulator polynomial of a univariate LUT (tfhe shortint box encoding, padding bit).
void make_lut_poly(const Params& p, const uint32_t* f, std::vector<uint64_t>* lut);
// E[k] = exp(i pi k / 2048), k < 4096, as i^(k >> 10) psi[k & 1023] exactly (oracle fho_monomials)
void mono_table(const std::vector<double2>& psi, std::vector<double2>* E);

}  // namespace fhe

struct fhe_ctx {
    fhe_ctx() = default;
    fhe_ctx(const fhe_ctx&) = delete;
    fhe_ctx& operator=(const fhe_ctx&) = delete;
    // waits for the stream, deletes the engine, releases the communicator, destroys events and the stream;
    // the buffers below then free themselves
    ~fhe_ctx();
    int device = 0;
    hipStream_t stream = nullptr;
    bool has_key = false;
    // fhe_host_sim_ctx_create: no device, no stream, no key material; the engine is Engine::kSim.  The radix
    // layer's entry points run on it, everything that needs device memory or a real key refuses (refuse_simulated)
    bool simulated = false;
    fhe::Params p;
    // The installed server key: the keyswitch and blind-rotate sets, which carry the n (and grouping) their
    // buffers were sized for, and `rows`, the keyswitched small LWE the one writes and the other reads, whose
    // stride follows the n it was grown for.  Replaced as a whole (install_key), never member by member.
    fhe::ServerKeySet key;
    fhe::RowSpace rows;
    fhe::DeviceBuf<double2> d_W;    // per-lane twiddle table [30][64]
    fhe::DeviceBuf<double2> d_psi;
    fhe::DeviceBuf<double2> d_tw_wide;   // [12][256]
    fhe::DeviceBuf<double2> d_psi_wide;  // [4][256]
    fhe::DeviceBuf<double2> d_zeta_full; // zeta(s, b) at [2^s + b], 1024 entries (br_qy.hip)
    fhe::DeviceBuf<double2> d_tw_quad;   // W[0..512)
    // [2][8][128] (quad_tables): the twist psi[128 r + t], which no kernel has read since the twisted
    // forward, then at [1024] the untwist conj(psi) 2^-51 that br_qy.hip's kernels multiply by
    fhe::DeviceBuf<double2> d_psi_quad;
    fhe::DeviceBuf<double2> d_zeta_wide; // [10][256] (context.cpp:wide_zetas)
    fhe::DeviceBuf<double2> d_mono;      // monomial table E[4096] of the multi-bit blind rotation (mono_table)
    int ks_kernel = FHE_KS_MFMA;
    // fhe_ctx_set_modulus_switch: FHE_MS_CENTERED makes keyswitch() follow its kernel with k_ms_center on
    // the rows it wrote (ms_center.hip), so every level launched from then on hands the blind rotation centered rows
    int ms_mode = FHE_MS_STANDARD;
    // classic throughput kernel (fhe_ctx_set_br_kernel): FHE_BR_AUTO = qz (two ciphertexts per workgroup,
    // one wave per polynomial; it replaced qy2 here, same quantisation) where its rounds of 1024 (256 CUs x
    // 2 workgroups x 2) fill well -- from kQy2Min bootstraps on, and above 960 when the last round is more
    // than three quarters full (qy2, 1012: 7.45 vs 7.9 ms) -- qy below and between (two per workgroup
    // quantises worse: profiles/r6/qy2_sizes_r6l.txt, qy_qy2_thresh_r6z.txt: 1024 -5 %, 2048 -2 %, 2560
    // even, 1280 / 1536 +19 / +2 %); FHE_BR_QY / _QY2 / _QY4 / _QZ force one kernel
    int br_kernel = FHE_BR_AUTO;
    static constexpr int kQy2Min = 3072;
    static bool qy2_fills(size_t count) {
        return count >= (size_t)kQy2Min || (count > 960 && (count % 1024 == 0 || count % 1024 > 768));
    }
    fhe::DeviceBuf<int8_t> d_ks_digits;  // keyswitch digits workspace
    fhe::DeviceBuf<uint64_t> d_ks_body;
    fhe::GroupCap ks_cap;           // ciphertexts
    // levels with at most this many bootstraps use the latency kernel (one ciphertext per CU at a
    // time -- >128 KB LDS -- so one round over the 256 CUs); the throughput kernel above, which holds
    // 2-3 per CU (profiles/r2/latency_sweep_r2b.txt: from 320 on it is as fast or faster)
    int wide_threshold = 256;
    // LUT registry: table contents -> id, device array of accumulator polynomials
    std::map<std::vector<uint32_t>, uint32_t> lut_ids;
    std::vector<uint64_t> h_luts;
    fhe::DeviceBuf<uint64_t> d_luts;  // capacity() / kPolySize tables
    bool luts_dirty = false;
    // staging of the raw batch entry points
    fhe::DeviceBuf<uint64_t> d_stage_in;
    fhe::DeviceBuf<uint64_t> d_stage_out;
    fhe::DeviceBuf<uint32_t> d_stage_lut;
    fhe::GroupCap stage_cap;  // ciphertexts
    // timing
    bool timing = false;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    float last_ks_ms = 0.f, last_br_ms = 0.f;
    // clock probe of the throughput blind rotate (fhe_ctx_enable_clock / fhe_ctx_read_clock)
    fhe::DeviceBuf<unsigned long long> d_clock;  // {sum of workgroup shader cycles, of 100 MHz ticks, workgroups}
    bool clock_probe = false;
    // radix-layer executor (created with the server key)
    fhe::Engine* engine = nullptr;
    // Multi-GPU fan-out (comm.cpp): every rank runs the same radix program on identical inputs;
    // a level with at least fanout_min bootstraps is split contiguously over the ranks and its
    // outputs are all-gathered (RCCL over xGMI) -- smaller levels are computed redundantly, since
    // one ciphertext per CU is already their latency floor.
    void* comm = nullptr;       // ncclComm_t
    int rank = 0, nranks = 1;
    uint32_t comm_timeout_ms = FHE_COMM_DEFAULT_TIMEOUT_MS;  // deadline of every collective's enqueue
    int fanout_emulate = 0;     // test hook: split levels over this many virtual ranks on one GPU
    size_t fanout_min = 257;  // above one ciphertext per CU (256 CUs) a level costs 2x the floor
    fhe::DeviceBuf<uint64_t> d_gather;   // [nranks * chunk][2049]
    fhe::GroupCap gather_cap;            // ciphertexts
    // test hook (fhe_ctx_attach_test_transport): the collectives through host buffers and callbacks
    fhe_test_transport tx{};
    bool has_tx = false;
    bool attached() const { return comm != nullptr || has_tx; }  // a real multi-rank transport
    int fanout_world() const { return attached() ? nranks : (fanout_emulate > 1 ? fanout_emulate : 1); }
    int ensure_gather(size_t ciphertexts);
    // in-place all-gather of nranks segments of `words` u64 each (segment `rank` is local)
    int allgather(uint64_t* buf, size_t words);
    void release_comm();
    // wait for the stream; with a communicator attached, bounded by comm_timeout_ms WITHOUT PROGRESS
    // (a collective whose peer died is aborted instead of hanging this rank; a long but healthy
    // flush keeps completing progress marks and is never cut off)
    int wait_stream(const char* what);
    // progress marks: an event recorded on the stream after every launched level while a
    // communicator is attached; wait_stream restarts its deadline whenever one completes.  At most
    // kProgRing marks are outstanding: when all are, the mark whose removal merges the two shortest
    // neighbouring intervals (in levels) is re-recorded at the newest level, so the outstanding marks
    // stay spread over everything queued -- the gaps between them grow evenly with the queue, never
    // one gap from mark kProgRing to the end (a long healthy flush keeps showing progress)
    static constexpr int kProgRing = 32;
    hipEvent_t prog_ev[kProgRing] = {};
    struct ProgMark {
        int ev;        // index into prog_ev
        uint64_t seq;  // levels launched when it was recorded
    };
    std::vector<ProgMark> prog_q;  // outstanding marks, oldest first
    uint64_t prog_seq = 0;
    void mark_progress();
    // drops the completed marks at the front of prog_q; true if any completed
    bool drain_progress();
    // *flags (one byte per entry) = min over the ranks, in place (one all-reduce; a no-op without a
    // communicator).  The engine's dead-node agreement.
    int allreduce_min_u8(uint8_t* flags, size_t n);
    fhe::DeviceBuf<uint8_t> d_flags;  // device staging of allreduce_min_u8 (grown, freed with the context)

    // at least `count` rows in `rs` for dimension n, regrown behind a wait on the stream
    int ensure_rows(fhe::RowSpace& rs, size_t n, size_t count);
    int ensure_ms(size_t count) { return ensure_rows(rows, p.n, count); }
    // the keys that belong to the installed server key and do not outlive it (compression, public, re-keying):
    // each one that is installed is released behind its own wait
    int release_dependants();
    // Commit point of every key install (fhe_set_server_key, the receivers of
    // fhe_ctx_broadcast_server_key), called once the new key's device buffers are in place: drops
    // what the previous key's parameters sized or encoded -- the dependent keys, the row space (row stride
    // from n: a stride kept across a change of dimension would overlap the keyswitch's rows) and, unless the
    // message space and delta are unchanged, the LUT tables (their ids then start again at 0) --
    // and makes `np` the context's parameters.
    int adopt_key_params(const fhe::Params& np, bool had_key);
    // the radix-layer executor, created with the first server key
    int ensure_engine();
    int ensure_ks(size_t count);
    // keyswitch of `count` inputs (contiguous big LWE in `in`, or descriptors) into `rows`; in centered mode
    // the rows' bodies are then corrected in place (k_ms_center), behind the keyswitch on the stream
    hipError_t keyswitch(const uint64_t* in, const fhe::PbsDesc* desc, size_t count);
    // What one keyswitch runs under (key_sets.h): a keyswitch set on the row space its rows go to.  main_ks() is
    // what every level uses; rekey_ks() the re-keying key (fhe_set_rekey_key: another small key and a row space
    // of its own, strided for its own n).
    using KsKeys = fhe::KsKeys;
    KsKeys main_ks() const { return key.ks.on(rows); }
    KsKeys rekey_ks() const { return rekey.on(rekey_rows); }
    hipError_t keyswitch(const KsKeys& ks, const uint64_t* in, const fhe::PbsDesc* desc, size_t count);
    int ensure_stage(size_t count);
    int sync_luts();
    int register_lut(const uint32_t* table, uint32_t* id);
    // LUT with outputs in half message steps (raw PbsItems): f(v) = half[v] * delta / 2, v < 16
    int register_lut_half(const int32_t* half, uint32_t* id);
    // the staircase accumulator of the oblivious pseudo-random values (oprf.cpp: oprf_lut_poly), one per `bits`
    int register_lut_oprf(uint32_t bits, uint32_t* id);
    // KS + BR(+SE) over device arrays, async on `stream`
    int pbs_device(const uint64_t* d_in, size_t count, const uint32_t* d_lut, uint64_t* d_out);
    // blind rotate (+SE) of `count` modulus-switched inputs in `rows`, kernel chosen by batch size
    hipError_t blind_rotate(const fhe::PbsDesc* desc, const uint32_t* lut_idx, uint64_t* out, size_t count);
    // What one blind rotation runs under (key_sets.h): a blind-rotate set on the row space holding the inputs.
    // main_keys() is what every bootstrap of the radix layer uses; comp_keys() the decompression key (classic,
    // n = k' N', a row space of its own).
    using BrKeys = fhe::BrKeys;
    BrKeys main_keys() const { return key.br.on(rows); }
    BrKeys comp_keys() const { return comp_br.on(comp_rows); }
    hipError_t blind_rotate(const BrKeys& ks, const fhe::PbsDesc* desc, const uint32_t* lut_idx, uint64_t* out,
                            size_t count);

    // Compression key (fhe_set_compression_key; dropped by every server-key install): the packing KSK as
    // byte planes (compress.hip), the decompression BSK as a blind-rotate set, and the workspaces.
    bool has_comp = false;
    fhe::CompParams cp;
    fhe::DeviceBuf<int8_t> d_pk_planes;
    fhe::BrKeySet comp_br;
    // compression workspace, `pk_cap` blocks: slot pointers, digits, bodies, contraction output, packed stream
    fhe::DeviceBuf<const uint64_t*> d_pk_src;
    fhe::DeviceBuf<int8_t> d_pk_digits;
    fhe::DeviceBuf<uint64_t> d_pk_body;
    fhe::DeviceBuf<uint64_t> d_pk_P;
    fhe::DeviceBuf<uint8_t> d_pk_out;
    fhe::GroupCap pk_cap;
    // decompression workspace, one group under comp_rows' capacity: the sample-extracted rows (dimension
    // k' N'), the uploaded 12-bit stream, one descriptor (LUT, destination slot) per block
    fhe::RowSpace comp_rows;
    fhe::DeviceBuf<uint8_t> d_cpacked;
    fhe::DeviceBuf<fhe::PbsDesc> d_cdesc;
    int ensure_pk(size_t count);
    int ensure_cms(size_t count);
    int release_compression();  // waits for the stream, frees all of the above

    // Public key of the re-randomization (fhe_set_public_key; dropped by every server-key install): A then B,
    // 2048 words each, and the zero encryptions' scratch, chunks of Z_A then Z_B (rerandomize.hip).
    bool has_pk = false;
    fhe::DeviceBuf<uint64_t> d_pk_ab;
    fhe::DeviceBuf<uint64_t> d_rr_z;
    int ensure_rr(size_t chunks);
    int release_public_key();  // waits for the stream, frees all of the above

    // Re-keying key (fhe_set_rekey_key; dropped by every server-key install): the expanded KSK to the destination's
    // small key as a keyswitch set, the destination's parameters (what a re-keyed list is labelled with), and a
    // row space strided for the destination's dimension.
    bool has_rekey = false;
    fhe::Params rkp;
    fhe::KsKeySet rekey;
    fhe::RowSpace rekey_rows;
    int ensure_rk_ms(size_t count) { return ensure_rows(rekey_rows, (size_t)rekey.n, count); }
    int release_rekey();  // waits for the stream, frees all of the above

    // Resident client key (fhe_ctx_set_client_key, client_ops.cpp): for a process that holds the
    // client key anyway.  d_client = client_ops::kClientWords u32: the big secret key as 2048 packed bits, then the
    // encryption stream's parameters of the call in flight (its key is as secret as the bits).  h_client is the
    // host copy in the same layout, pinned so that the copies go from it directly.  Nothing points at the
    // fhe_client_key the bits came from.  release_client_key overwrites both with zeros before it frees them; the
    // destructor and an install of a server key with other parameters (adopt_key_params) go through it.
    bool has_client = false;
    fhe::DeviceBuf<uint32_t> d_client;
    fhe::PinnedBuf<uint32_t> h_client;
    uint64_t client_enc_blocks = 0, client_phase_blocks = 0;  // blocks that took each device path
    // the device paths are taken only for the key whose packed bits are the resident ones
    bool client_resident(const fhe_client_key* ck) const;
    // the stream parameters of a call (the stream as it stands BEFORE the call's words) into h_client and d_client
    hipError_t client_stage_stream(const fhe::ChaChaStream& at, uint32_t noise_log2);
    int release_client_key();  // waits for the stream, wipes, frees
};

namespace fhe {

// The outline of every key install.  `fill` sizes the set's buffers and queues what fills them (an upload, an
// expansion from a seed, a collective); the set derives its second layout behind that (byte planes, E layout);
// the stream is drained; `commit` makes the key the context's.  On an error of any step `drop` waits for what
// was queued and frees the half-built key.  What is replaced, and when, is the caller's discipline: a direct
// install releases the old key before it calls this, a broadcast receiver swaps inside `commit`.
template <class Set, class Fill, class Commit, class Drop>
int install_key(fhe_ctx* c, Set& set, Fill&& fill, Commit&& commit, Drop&& drop) {
    auto body = [&]() -> int {
        if (const int rc = fill()) return rc;
        FHE_HIP_CHECK(set.derive(c->stream));
        FHE_HIP_CHECK(hipStreamSynchronize(c->stream));
        return commit();
    };
    const int rc = body();
    if (rc) (void)drop();
    return rc;
}

// What every install of a key that depends on the server key starts with, under the entry point's name `fn`:
// refuses a simulated context, a null argument (`args` false), a context without a server key, and, with `kp`,
// a key whose parameters differ from the server key's (`what`: "compression key", ...).  fhe_set_rekey_key
// passes no `kp`: it compares by its own rule after its own checks, and keeps its shorter no-key message.
int dependent_key_preamble(const fhe_ctx* c, bool args, const char* fn, const Params* kp = nullptr,
                           const char* what = nullptr);

}  // namespace fhe
