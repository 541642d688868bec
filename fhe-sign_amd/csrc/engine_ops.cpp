// engine_ops.cpp -- the engine's eager device operations (engine.h): uploads and downloads, the seeded,
// compact and compressed forms expanded into fresh slots, re-randomization, digests, oblivious pseudo-random
// blocks, the modulus-switched stored form, the broadcasts' adopt / gather.  Each runs at once on the context's stream, outside the deferred
// graph (engine.cpp), and follows one idiom:
//   * result blocks come from fresh_blocks(), their slot pointers from slot_ptrs();
//   * what goes through the upload staging is stated once, in order, on a Stage cursor that issues the copy,
//     hands back the typed device pointer and checks the total the operation asked staging() for;
//   * blocks that are read are made real first (realize), a trivial one enters as the body trivial_body().
#include "engine.h"
#include "client_ops.h"
#include "compress_kernels.h"
#include "ct_digest.h"
#include "keygen.h"
#include "oprf.h"
#include "switched.h"

#include <algorithm>
#include <cstring>
#include <string>

namespace fhe {

namespace {
// Cursor over the words an operation asked Engine::staging() for.  Every part is a multiple of 8 bytes, so each
// starts 8-byte aligned; a part that would pass the end is refused before anything is copied.
struct Stage {
    hipStream_t stream;
    uint8_t* at;
    uint8_t* end;
    Stage(hipStream_t s, uint64_t* base, size_t words)
        : stream(s), at(reinterpret_cast<uint8_t*>(base)), end(reinterpret_cast<uint8_t*>(base + words)) {}
    // device-only space for count elements (a gather's target, a kernel's output)
    template <class T>
    T* reserve(size_t count) {
        const size_t bytes = count * sizeof(T);
        engine_check(bytes % 8 == 0 && bytes <= (size_t)(end - at), "staging: a part outside the words asked for");
        T* const p = reinterpret_cast<T*>(at);
        at += bytes;
        return p;
    }
    // the same, filled from the host (asynchronously: `host` stays alive until the operation's sync)
    template <class T>
    T* put(const T* host, size_t count, const char* what) {
        T* const p = reserve<T>(count);
        hip_check(hipMemcpyAsync(p, host, count * sizeof(T), hipMemcpyHostToDevice, stream), what);
        return p;
    }
};

std::vector<uint64_t*> slot_ptrs(const Blocks& blocks) {
    std::vector<uint64_t*> p(blocks.size());
    for (size_t i = 0; i < blocks.size(); ++i) p[i] = blocks[i].slot->p;
    return p;
}

// the slots of blocks that must be real ciphertexts of this engine (`what`: the refusal)
std::vector<const uint64_t*> source_ptrs(const Engine& e, const std::vector<const Block*>& blocks, const char* what) {
    std::vector<const uint64_t*> p(blocks.size());
    for (size_t i = 0; i < blocks.size(); ++i) {
        engine_check(blocks[i]->slot != nullptr && !blocks[i]->lazy(), what);
        e.check_owner(*blocks[i]);
        p[i] = blocks[i]->slot->p;
    }
    return p;
}

// The blocks an operation reads, ready on the stream: a lazy block is combined into a slot of its own (lincomb
// flushes; its semantic degree carried over) in `real`, then the pending producers of all of them are launched.
std::vector<const Block*> realize(Engine& e, const std::vector<const Block*>& blocks, const std::string& op, Blocks& real) {
    e.check_owner(blocks);  // all of them, before the first lazy one is combined (a flush and a launch)
    real.assign(blocks.size(), Block());
    std::vector<const Block*> in(blocks);
    for (size_t i = 0; i < blocks.size(); ++i) {
        if (!blocks[i]->lazy()) continue;
        engine_check(blocks[i]->lin_cst >= 0, (op + " of a lazy block below zero").c_str());
        real[i] = e.lincomb(*blocks[i]->lin, (uint32_t)blocks[i]->lin_cst);
        real[i].degree = blocks[i]->degree;
        in[i] = &real[i];
    }
    e.flush_for(in);
    return in;
}

// the body of the ciphertext (0, delta value) a trivial block enters an operation as; 0 for any other block
uint64_t trivial_body(const Block& b, uint64_t delta, const std::string& op) {
    if (!b.trivial()) return 0;
    engine_check(!b.half_neg, (op + " of a half-step block").c_str());
    return (uint64_t)b.value * delta;
}

// descriptors without terms (no keyswitch: the rows are already in the bootstrap workspace), one per block
std::vector<PbsDesc> bare_descs(const Blocks& out, uint32_t lut, uint64_t cst) {
    std::vector<PbsDesc> desc(out.size());
    std::memset(desc.data(), 0, desc.size() * sizeof(PbsDesc));
    for (size_t i = 0; i < out.size(); ++i) {
        desc[i].lut = lut;
        desc[i].cst = cst;
        desc[i].dst = out[i].slot->p;
    }
    return desc;
}

void need_compression(const fhe_ctx* c) {
    if (!c->has_comp) throw EngineError(FHE_ERR_NO_KEY, "no compression key installed (fhe_set_compression_key)");
}

// the packing keyswitch over the rows `src` points at (the compression workspace holds src.size() rows)
void pack_keyswitch(fhe_ctx* c, const std::vector<const uint64_t*>& src) {
    const CompParams& cp = c->cp;
    const size_t n = src.size();
    hip_check(hipMemcpyAsync(c->d_pk_src, src.data(), n * sizeof(uint64_t*), hipMemcpyHostToDevice, c->stream), "compress slots");
    hip_check(launch_pack_keyswitch(c->d_pk_src, (int)n, (int)cp.beta, (int)cp.ell, (int)cp.k, (int)cp.N, (int)cp.L, c->d_pk_planes,
                                    c->d_pk_digits, c->d_pk_body, c->d_pk_P, c->d_pk_out, c->stream),
              "packing keyswitch");
}
}  // namespace

Blocks Engine::fresh_blocks(const std::vector<uint32_t>& degrees, int write_kind) {
    Blocks out(degrees.size());
    for (size_t i = 0; i < out.size(); ++i) {
        out[i].slot = pool_->alloc();
        out[i].degree = degrees[i];
        out[i].noise = 1;
    }
    if (ltrace_on_ && write_kind >= 0) {  // the op that asked for them fills them next on the stream
        const std::vector<uint64_t*> dst = slot_ptrs(out);
        trace_write((uint64_t)write_kind, dst.data(), dst.size());
    }
    return out;
}

Blocks Engine::fresh_blocks(size_t n, uint32_t degree, int write_kind) {
    return fresh_blocks(std::vector<uint32_t>(n, degree), write_kind);
}

// ------------------------------------------------------------------ uploads
Block Engine::upload(const uint64_t* ct, uint32_t degree) {
    Block b = fresh_blocks(1, degree, (int)kWriteUpload)[0];
    hip_check(hipMemcpyAsync(b.slot->p, ct, kBigCt * 8, hipMemcpyHostToDevice, ctx_->stream), "upload");
    hip_check(hipStreamSynchronize(ctx_->stream), "upload sync");
    return b;
}

void Engine::scatter_upload(const uint64_t* cts, const std::vector<uint64_t*>& dst) {
    const size_t n = dst.size();
    const size_t words = n * kBigCt + n;  // ciphertexts, then the slot pointers
    Stage st(ctx_->stream, staging(words), words);
    const uint64_t* d_cts = st.put(cts, n * kBigCt, "upload");
    uint64_t** d_dst = st.put(dst.data(), n, "upload");
    hip_check(launch_scatter_blocks(d_cts, d_dst, (int)n, ctx_->stream), "upload scatter");
    hip_check(hipStreamSynchronize(ctx_->stream), "upload sync");  // host buffers may go
}

Blocks Engine::upload_many(const uint64_t* cts, size_t n, uint32_t degree) {
    Blocks out = fresh_blocks(n, degree, (int)kWriteUpload);
    if (n) scatter_upload(cts, slot_ptrs(out));
    return out;
}

Blocks Engine::upload_deferred(size_t n, uint32_t degree, std::function<std::vector<uint64_t>()> fill) {
    run_before_launch();  // an earlier deferred upload first (one at a time)
    // a device engine records the write where it is enqueued (the deferred upload below), a host mode now
    Blocks out = fresh_blocks(n, degree, host_mode_ == kDevice ? -1 : (int)kWriteDeferred);
    if (n == 0 || host_mode_ != kDevice) return out;
    std::vector<std::shared_ptr<Slot>> held(n);  // alive until the upload, whatever the caller drops
    for (size_t i = 0; i < n; ++i) held[i] = out[i].slot;
    before_launch_ = [this, held = std::move(held), dst = slot_ptrs(out), fill = std::move(fill)]() {
        fault_point(kFaultDeferred, "DEFERRED");
        const std::vector<uint64_t> cts = fill();
        engine_check(cts.size() == dst.size() * kBigCt, "deferred upload: ciphertext count");
        if (ltrace_on_) trace_write(kWriteDeferred, dst.data(), dst.size());
        scatter_upload(cts.data(), dst);
    };
    return out;
}

Blocks Engine::expand_seeded(const uint8_t seed[32], const uint64_t* bodies, size_t n) {
    engine_check(host_mode_ == kDevice, "expand_seeded on a host-only engine");
    engine_check(n <= kSeededMaxBlocks, "seeded object of more than 2^24 blocks");
    if (n == 0) return {};
    const size_t words = 2 * n;  // the bodies, then the slot pointers
    Stage st(ctx_->stream, staging(words), words);
    Blocks out = fresh_blocks(n, 3);
    const std::vector<uint64_t*> dst = slot_ptrs(out);
    const uint64_t* d_bodies = st.put(bodies, n, "seeded bodies");
    uint64_t** d_dst = st.put(dst.data(), n, "seeded slots");
    const KeyWords key = bytes_key(seed);
    hip_check(launch_expand_seeded(chacha_stream_key(key.data(), kStreamSeededMask), d_dst, d_bodies, (int)n, ctx_->stream),
              "seeded expansion");
    hip_check(hipStreamSynchronize(ctx_->stream), "upload sync");  // host buffers may go, the staging be reused
    return out;
}

// ------------------------------------------------------------------ compressed computed ciphertexts
void Engine::compress(const std::vector<const Block*>& blocks, uint8_t* packed) {
    engine_check(host_mode_ == kDevice, "compress on a host-only engine");
    need_compression(ctx_);
    const size_t n = blocks.size();
    engine_check(n <= kCompressedMaxBlocks, "compressed list of more than 2^24 blocks");
    if (n == 0) return;
    check_owner(blocks);
    const CompParams& cp = ctx_->cp;
    // trivial blocks become ciphertexts (0, b) in slots of their own: the kernels see no special case
    std::vector<uint64_t> cts;
    for (const Block* b : blocks) {
        engine_check(!b->lazy(), "compress of a lazy block");
        if (!b->trivial()) continue;
        cts.resize(cts.size() + kBigCt, 0ull);
        cts[cts.size() - kBigCt + kBigDim] = trivial_body(*b, ctx_->p.delta(), "compress");
    }
    const Blocks tmp = upload_many(cts.data(), cts.size() / kBigCt, 0);
    flush();
    engine_check(ctx_->ensure_pk(n) == FHE_OK, "compression workspace");
    std::vector<const uint64_t*> src(n);
    for (size_t i = 0, q = 0; i < n; ++i) src[i] = blocks[i]->trivial() ? tmp[q++].slot->p : blocks[i]->slot->p;
    pack_keyswitch(ctx_, src);
    const size_t G = cp.glwes(n), stride = (size_t)pk_out_stride((int)cp.k, (int)cp.N);
    std::vector<uint8_t> stage(G * stride);
    hip_check(hipMemcpyAsync(stage.data(), ctx_->d_pk_out, stage.size(), hipMemcpyDeviceToHost, ctx_->stream),
              "compress download");
    wait_check(ctx_, "compress");
    // the device keeps every polynomial on a 32-bit word; the wire starts a GLWE on the next byte
    uint8_t* out = packed;
    for (size_t g = 0; g < G; ++g) {
        const size_t bytes = cp.glwe_bytes(cp.bodies(n, g));
        std::memcpy(out, stage.data() + g * stride, bytes);
        out += bytes;
    }
}

void Engine::pack_keyswitch_words(const uint64_t* cts, size_t n, uint64_t* P, uint64_t* body) {
    engine_check(host_mode_ == kDevice, "compress on a host-only engine");
    need_compression(ctx_);
    engine_check(n <= kCompressedMaxBlocks, "compressed list of more than 2^24 blocks");
    if (n == 0) return;
    const CompParams& cp = ctx_->cp;
    flush();
    engine_check(ctx_->ensure_stage(n) == FHE_OK, "staging buffer");
    engine_check(ctx_->ensure_pk(n) == FHE_OK, "compression workspace");
    std::vector<const uint64_t*> src(n);
    for (size_t i = 0; i < n; ++i) src[i] = ctx_->d_stage_in + i * kBigCt;
    hip_check(hipMemcpyAsync(ctx_->d_stage_in, cts, n * kBigCt * 8, hipMemcpyHostToDevice, ctx_->stream), "rows upload");
    pack_keyswitch(ctx_, src);
    hip_check(hipMemcpyAsync(P, ctx_->d_pk_P, n * cp.cols() * 8, hipMemcpyDeviceToHost, ctx_->stream), "words download");
    hip_check(hipMemcpyAsync(body, ctx_->d_pk_body, n * 8, hipMemcpyDeviceToHost, ctx_->stream), "bodies download");
    wait_check(ctx_, "packing keyswitch words");
}

void Engine::extract_rows(const fhe_compressed_list& x, uint64_t* rows) {
    engine_check(host_mode_ == kDevice, "decompress on a host-only engine");
    need_compression(ctx_);
    const size_t n = x.degrees.size();
    if (n == 0) return;
    const CompParams& cp = ctx_->cp;
    engine_check(ctx_->ensure_cms(n) == FHE_OK, "decompression workspace");
    hip_check(hipMemcpyAsync(ctx_->d_cpacked, x.packed.data(), x.packed.size(), hipMemcpyHostToDevice, ctx_->stream),
              "compressed upload");
    hip_check(launch_pk_unpack(ctx_->d_cpacked, (int)n, (int)cp.glwe_bytes(cp.L), (int)cp.L, (int)cp.N, (int)cp.k,
                               ctx_->comp_rows.rows(), ctx_->comp_rows.stride(), ctx_->stream),
              "unpack");
    if (rows) {
        const size_t row = ((size_t)cp.lwe_dim() + 1) * 8;
        hip_check(hipMemcpy2DAsync(rows, row, ctx_->comp_rows.rows(), (size_t)ctx_->comp_rows.stride() * 8, row, n, hipMemcpyDeviceToHost,
                                   ctx_->stream),
                  "rows download");
        hip_check(hipStreamSynchronize(ctx_->stream), "rows sync");
    }
}

Blocks Engine::decompress(const fhe_compressed_list& x) {
    const size_t n = x.degrees.size();
    engine_check(host_mode_ == kDevice, "decompress on a host-only engine");
    need_compression(ctx_);
    if (n == 0) return {};
    std::vector<uint32_t> ident(ctx_->p.msg_carry());
    for (uint32_t v = 0; v < ident.size(); ++v) ident[v] = v;
    uint32_t lut = 0;
    engine_check(ctx_->register_lut(ident.data(), &lut) == FHE_OK && ctx_->sync_luts() == FHE_OK, "identity table");
    extract_rows(x, nullptr);
    Blocks out = fresh_blocks(std::vector<uint32_t>(x.degrees.begin(), x.degrees.end()));
    const std::vector<PbsDesc> desc = bare_descs(out, lut, 0);
    hip_check(hipMemcpyAsync(ctx_->d_cdesc, desc.data(), n * sizeof(PbsDesc), hipMemcpyHostToDevice, ctx_->stream),
              "decompress descriptors");
    hip_check(ctx_->blind_rotate(ctx_->comp_keys(), ctx_->d_cdesc, nullptr, nullptr, n), "decompression blind rotate");
    hip_check(hipStreamSynchronize(ctx_->stream), "decompress sync");  // host buffers may go, the staging be reused
    pbs_count += n;
    return out;
}

// ------------------------------------------------------------------ oblivious pseudo-random values
Blocks Engine::oprf(const uint8_t seed[32], size_t count, uint32_t bits, uint32_t tail_bits) {
    engine_check(host_mode_ == kDevice, "oprf on a host-only engine");
    const Params& p = ctx_->p;
    const uint32_t max_bits = oprf_max_bits(p);
    if (bits < 1 || bits > max_bits || tail_bits > max_bits)
        throw std::runtime_error("oprf: bits must be 1 .. log2(message_modulus) = " + std::to_string(max_bits));
    const size_t n = count + (tail_bits ? 1 : 0);
    engine_check(n <= kOprfMaxRows, "oprf: more than 2^23 rows of one seed");
    if (n == 0) return {};
    uint32_t lut = 0, tail_lut = 0;
    engine_check(ctx_->register_lut_oprf(bits, &lut) == FHE_OK && (!tail_bits || ctx_->register_lut_oprf(tail_bits, &tail_lut) == FHE_OK) &&
                     ctx_->sync_luts() == FHE_OK,
                 "oprf accumulator");
    // the workspace as it stands (at least kOprfChunk rows) is the chunk: a large call does not grow it
    constexpr size_t kOprfChunk = 4096;
    const size_t chunk = std::min(n, std::max(ctx_->rows.cap(), kOprfChunk));
    engine_check(ctx_->ensure_ms(chunk) == FHE_OK, "bootstrap workspace");
    ensure_eager_desc(chunk);
    std::vector<uint32_t> degrees(n, (1u << bits) - 1);
    if (tail_bits) degrees[count] = (1u << tail_bits) - 1;
    Blocks out = fresh_blocks(degrees);
    // the blind rotation ignores the constant (no terms, no keyswitch): it is the body add's
    std::vector<PbsDesc> desc = bare_descs(out, lut, oprf_body_const(p, bits));
    if (tail_bits) {
        desc[count].lut = tail_lut;
        desc[count].cst = oprf_body_const(p, tail_bits);
    }
    const KeyWords key = bytes_key(seed);
    const ChaChaKey ck = chacha_stream_key(key.data(), kStreamOprf);
    for (size_t at = 0; at < n; at += chunk) {
        const size_t m = std::min(chunk, n - at);
        hip_check(launch_oprf_rows(ck, ctx_->rows.rows(), (uint32_t)at, (uint32_t)m, p.n, ctx_->stream), "oprf rows");
        hip_check(hipMemcpyAsync(d_oprf_desc_, desc.data() + at, m * sizeof(PbsDesc), hipMemcpyHostToDevice, ctx_->stream),
                  "oprf descriptors");
        hip_check(ctx_->blind_rotate(ctx_->main_keys(), d_oprf_desc_, nullptr, nullptr, m), "oprf blind rotate");
        hip_check(launch_oprf_body_add(d_oprf_desc_, (uint32_t)m, ctx_->stream), "oprf body constant");
    }
    hip_check(hipStreamSynchronize(ctx_->stream), "oprf sync");  // host buffers may go
    pbs_count += n;
    return out;
}

void Engine::ensure_eager_desc(size_t chunk) {
    if (d_oprf_desc_.fits(chunk)) return;
    hip_check(hipStreamSynchronize(ctx_->stream), "eager descriptors sync");
    hip_check(d_oprf_desc_.grow(std::max<size_t>(chunk, 256)), "eager descriptors");
}

// ------------------------------------------------------------------ modulus-switched stored ciphertexts
namespace {
// the workspace as it stands (at least this many rows) is the chunk of the stored form's two ops, as of oprf
constexpr size_t kSwitchedChunk = 4096;
}  // namespace

void Engine::switched_compress(const std::vector<const Block*>& blocks, uint8_t* rows, bool rekey) {
    engine_check(host_mode_ == kDevice, "compress_switched on a host-only engine");
    if (rekey && !ctx_->has_rekey) throw EngineError(FHE_ERR_NO_KEY, "no re-keying key installed (fhe_set_rekey_key)");
    const size_t n = blocks.size();
    engine_check(n <= kCompressedMaxBlocks, "stored list of more than 2^24 blocks");
    if (n == 0) return;
    const Params& p = ctx_->p;
    Blocks real;
    const std::vector<const Block*> in = realize(*this, blocks, "compress_switched", real);
    // one-term descriptors: the keyswitch reads the slot as it is; a trivial block is the constant alone
    std::vector<PbsDesc> desc(n);
    std::memset(desc.data(), 0, n * sizeof(PbsDesc));
    for (size_t i = 0; i < n; ++i) {
        const Block& b = *in[i];
        engine_check(b.noise <= kMaxNoise, "compress_switched: block noise above the budget of a lookup");
        if (b.trivial()) {
            desc[i].cst = trivial_body(b, p.delta(), "compress_switched");
            continue;
        }
        desc[i].src[0] = b.ptr();
        desc[i].coef[0] = 1;
        desc[i].nterms = 1;
    }
    const size_t chunk = std::min(n, std::max(rekey ? ctx_->rekey_rows.cap() : ctx_->rows.cap(), kSwitchedChunk));
    engine_check((rekey ? ctx_->ensure_rk_ms(chunk) : ctx_->ensure_ms(chunk)) == FHE_OK, "row workspace");
    ensure_eager_desc(chunk);
    const fhe_ctx::KsKeys ks = rekey ? ctx_->rekey_ks() : ctx_->main_ks();
    const uint32_t nd = (uint32_t)ks.n;  // the rows' dimension: the destination key's when re-keying
    const size_t dev_bytes = switched_dev_row_bytes(nd), bytes = switched_row_bytes(nd);
    if (!d_sw_packed_.fits(chunk * dev_bytes / 4)) {
        hip_check(hipStreamSynchronize(ctx_->stream), "stored rows sync");
        hip_check(d_sw_packed_.grow(std::max<size_t>(chunk, 256) * dev_bytes / 4), "stored rows");
    }
    std::vector<uint8_t> stage(chunk * dev_bytes);
    for (size_t at = 0; at < n; at += chunk) {
        const size_t m = std::min(chunk, n - at);
        hip_check(hipMemcpyAsync(d_oprf_desc_, desc.data() + at, m * sizeof(PbsDesc), hipMemcpyHostToDevice, ctx_->stream),
                  "compress_switched descriptors");
        hip_check(ctx_->keyswitch(ks, nullptr, d_oprf_desc_, m), "compress_switched keyswitch");
        hip_check(launch_ms_pack(ks.ms, d_sw_packed_, m, nd, ctx_->stream), "row packing");
        hip_check(hipMemcpyAsync(stage.data(), d_sw_packed_, m * dev_bytes, hipMemcpyDeviceToHost, ctx_->stream),
                  "compress_switched download");
        wait_check(ctx_, "compress_switched");
        // the device keeps every row on whole 12-byte groups; the wire starts a row on the next byte
        for (size_t i = 0; i < m; ++i) std::memcpy(rows + (at + i) * bytes, stage.data() + i * dev_bytes, bytes);
    }
}

Blocks Engine::switched_decompress(const fhe_switched_list& x) {
    engine_check(host_mode_ == kDevice, "decompress on a host-only engine");
    const size_t n = x.degrees.size();
    if (n == 0) return {};
    const Params& p = ctx_->p;
    const size_t dev_bytes = switched_dev_row_bytes(p.n), bytes = switched_row_bytes(p.n);
    engine_check(x.params.n == p.n && x.rows.size() == n * bytes, "stored list: rows of another LWE dimension");
    std::vector<uint32_t> ident(p.msg_carry());
    for (uint32_t v = 0; v < ident.size(); ++v) ident[v] = v;
    uint32_t lut = 0;
    engine_check(ctx_->register_lut(ident.data(), &lut) == FHE_OK && ctx_->sync_luts() == FHE_OK, "identity table");
    const size_t chunk = std::min(n, std::max(ctx_->rows.cap(), kSwitchedChunk));
    engine_check(ctx_->ensure_ms(chunk) == FHE_OK, "bootstrap workspace");
    ensure_eager_desc(chunk);
    if (!d_sw_packed_.fits(chunk * dev_bytes / 4)) {
        hip_check(hipStreamSynchronize(ctx_->stream), "stored rows sync");
        hip_check(d_sw_packed_.grow(std::max<size_t>(chunk, 256) * dev_bytes / 4), "stored rows");
    }
    Blocks out = fresh_blocks(std::vector<uint32_t>(x.degrees.begin(), x.degrees.end()));
    const std::vector<PbsDesc> desc = bare_descs(out, lut, 0);
    std::vector<uint8_t> stage(chunk * dev_bytes, 0);
    for (size_t at = 0; at < n; at += chunk) {
        const size_t m = std::min(chunk, n - at);
        for (size_t i = 0; i < m; ++i) std::memcpy(stage.data() + i * dev_bytes, x.rows.data() + (at + i) * bytes, bytes);
        hip_check(hipMemcpyAsync(d_sw_packed_, stage.data(), m * dev_bytes, hipMemcpyHostToDevice, ctx_->stream),
                  "stored rows upload");
        hip_check(launch_ms_unpack(d_sw_packed_, ctx_->rows.rows(), m, p.n, ctx_->stream), "row unpacking");
        hip_check(hipMemcpyAsync(d_oprf_desc_, desc.data() + at, m * sizeof(PbsDesc), hipMemcpyHostToDevice, ctx_->stream),
                  "decompress descriptors");
        hip_check(ctx_->blind_rotate(ctx_->main_keys(), d_oprf_desc_, nullptr, nullptr, m), "decompression blind rotate");
        hip_check(hipStreamSynchronize(ctx_->stream), "decompress sync");  // the stage and the descriptors may be reused
    }
    pbs_count += n;
    return out;
}

// ------------------------------------------------------------------ compact ciphertext lists (public key)
Blocks Engine::compact_extract(const fhe_compact_list& x, size_t first, size_t n, const std::vector<uint32_t>& degrees) {
    engine_check(host_mode_ == kDevice, "expand_compact on a host-only engine");
    engine_check(first + n <= x.ncoef() && x.ncoef() <= kCompactMaxCoefs && x.ca.size() == (x.ncoef() + kPolySize - 1) / kPolySize * kPolySize,
                 "compact list: coefficient range outside the list");
    if (n == 0) return {};
    const size_t c0 = first / kPolySize, c1 = (first + n - 1) / kPolySize + 1;  // the chunks the range touches
    const size_t ca_words = (c1 - c0) * kPolySize;
    const size_t words = ca_words + 2 * n;  // C_A of the chunks, the bodies, then the slot pointers
    Stage st(ctx_->stream, staging(words), words);
    Blocks out = fresh_blocks(degrees);
    const std::vector<uint64_t*> dst = slot_ptrs(out);
    const uint64_t* d_ca = st.put(x.ca.data() + c0 * kPolySize, ca_words, "compact masks");
    const uint64_t* d_cb = st.put(x.cb.data() + first, n, "compact bodies");
    uint64_t** d_dst = st.put(dst.data(), n, "compact slots");
    hip_check(launch_compact_extract(d_ca, d_cb, d_dst, (uint32_t)(first - c0 * kPolySize), (int)n, ctx_->stream),
              "compact extraction");
    hip_check(hipStreamSynchronize(ctx_->stream), "upload sync");  // host buffers may go, the staging be reused
    return out;
}

Blocks Engine::expand_compact(const fhe_compact_list& x, size_t value) {
    engine_check(value < x.values.size(), "compact list: value index out of range");
    const fhe_compact_list::Value& v = x.values[value];
    std::vector<uint32_t> degrees(v.ncoef);
    for (size_t q = 0; q < v.ncoef; ++q) degrees[q] = compact_degree(x, v, v.first + q);
    Blocks coefs = compact_extract(x, v.first, v.ncoef, degrees);
    if (!x.packed) return coefs;
    // one level: block 2 q = x_q & 3, block 2 q + 1 = x_q >> 2
    const uint32_t mc = ctx_->p.msg_carry();
    std::vector<uint32_t> lo(mc), hi(mc);
    for (uint32_t m = 0; m < mc; ++m) {
        lo[m] = m & 3;
        hi[m] = m >> 2;
    }
    std::vector<PbsItem> items(v.nblocks);
    for (size_t k = 0; k < v.nblocks; ++k) {
        items[k].terms = {{coefs[k / 2], 1}};
        items[k].table = (k & 1) ? hi : lo;
    }
    return run(items);
}

void Engine::extract_compact_rows(const fhe_compact_list& x, uint64_t* rows) {
    const size_t n = x.ncoef();
    if (n == 0) return;
    const Blocks all = compact_extract(x, 0, n, std::vector<uint32_t>(n, 3));
    std::vector<const Block*> ptrs(n);
    for (size_t i = 0; i < n; ++i) ptrs[i] = &all[i];
    download_many(ptrs, rows);
}

// ------------------------------------------------------------------ re-randomization (public key)
Blocks Engine::rerandomize(const std::vector<const Block*>& blocks, const uint8_t seed[32]) {
    engine_check(host_mode_ == kDevice, "rerandomize on a host-only engine");
    if (!ctx_->has_pk) throw EngineError(FHE_ERR_NO_KEY, "no public key installed (fhe_set_public_key)");
    const size_t n = blocks.size();
    engine_check(n <= kCompactMaxCoefs, "rerandomize of more than 2^24 blocks");
    if (n == 0) return {};
    Blocks real;
    const std::vector<const Block*> in = realize(*this, blocks, "rerandomize", real);
    const size_t chunks = (n + kPolySize - 1) / kPolySize;
    engine_check(ctx_->ensure_rr(chunks) == FHE_OK, "re-randomization workspace");
    const size_t words = 3 * n;  // the source slots, the trivial bodies, then the fresh slots
    Stage st(ctx_->stream, staging(words), words);
    std::vector<const uint64_t*> src(n);
    std::vector<uint64_t> tbody(n);
    std::vector<uint32_t> degrees(n);
    for (size_t i = 0; i < n; ++i) {
        const Block& b = *in[i];
        src[i] = b.ptr();
        tbody[i] = trivial_body(b, ctx_->p.delta(), "rerandomize");
        degrees[i] = b.trivial() ? std::max<uint32_t>(b.degree, kMsgMod - 1) : b.degree;
    }
    // real ciphertexts from here on: slot set, no value, no combination, no half step; the noise label stays
    Blocks out = fresh_blocks(degrees);
    for (size_t i = 0; i < n; ++i) out[i].noise = in[i]->noise;
    const std::vector<uint64_t*> dst = slot_ptrs(out);
    const uint64_t** d_src = st.put(src.data(), n, "rerandomize slots");
    const uint64_t* d_tbody = st.put(tbody.data(), n, "rerandomize bodies");
    uint64_t** d_dst = st.put(dst.data(), n, "rerandomize slots");
    KeyWords key = bytes_key(seed);
    ChaChaKey kbin = chacha_stream_key(key.data(), kStreamRerandBinary), knoise = chacha_stream_key(key.data(), kStreamRerandNoise);
    const hipError_t zrc = launch_rerand_zero(kbin, knoise, ctx_->d_pk_ab, ctx_->d_rr_z, (uint32_t)n, ctx_->p.glwe_noise_log2, ctx_->stream);
    // the launch has copied its arguments: the seed gives away R, no copy of it stays on the host
    for (volatile uint32_t& w : key) w = 0;
    for (ChaChaKey* k : {&kbin, &knoise})
        for (volatile uint32_t& w : k->key) w = 0;
    hip_check(zrc, "zero encryptions");
    hip_check(launch_rerand_add(ctx_->d_rr_z, d_src, d_tbody, d_dst, (uint32_t)n, ctx_->stream), "re-randomization");
    hip_check(hipStreamSynchronize(ctx_->stream), "upload sync");  // host buffers may go, the staging be reused
    return out;
}

// ------------------------------------------------------------------ ciphertext digests
void Engine::digest(const std::vector<const Block*>& blocks, uint8_t* out, std::vector<DigestMeta>* meta) {
    engine_check(host_mode_ == kDevice, "digest on a host-only engine");
    const size_t n = blocks.size();
    engine_check(n <= kCtDigestMaxRows, "digest of more than 2^24 blocks");
    if (meta) meta->assign(n, DigestMeta{0, 0, 0});
    if (n == 0) return;
    Blocks real;
    const std::vector<const Block*> in = realize(*this, blocks, "digest", real);
    const size_t words = 2 * n + 4 * n;  // the entries (16 B each), then the digests (32 B each, 16-byte aligned)
    Stage st(ctx_->stream, staging(words), words);
    std::vector<CtDigestEntry> entries(n);
    for (size_t i = 0; i < n; ++i) {
        const Block& b = *in[i];
        entries[i].src = b.ptr();
        entries[i].tbody = trivial_body(b, ctx_->p.delta(), "digest");
        if (meta) (*meta)[i] = b.trivial() ? DigestMeta{0, b.value, 0} : DigestMeta{1, b.degree, b.noise};
    }
    const CtDigestEntry* d_entries = st.put(entries.data(), n, "digest entries");
    uint8_t* d_out = st.reserve<uint8_t>(32 * n);
    hip_check(launch_ct_digest(d_entries, d_out, (uint32_t)n, ct_digest_midstates(), ctx_->stream), "ciphertext digest");
    hip_check(hipMemcpyAsync(out, d_out, n * 32, hipMemcpyDeviceToHost, ctx_->stream), "digest download");
    wait_check(ctx_, "digest");
}

// ------------------------------------------------------------------ downloads, the broadcasts' ends
void Engine::download(const Block& b, uint64_t* ct) {
    engine_check(!b.trivial() && !b.lazy(), "download of a trivial or lazy block");
    check_owner(b);
    flush();
    hip_check(hipMemcpyAsync(ct, b.slot->p, kBigCt * 8, hipMemcpyDeviceToHost, ctx_->stream), "download");
    wait_check(ctx_, "download");
}

void Engine::download_many(const std::vector<const Block*>& blocks, uint64_t* cts, bool only_needed) {
    const size_t n = blocks.size();
    if (n == 0) return;
    check_owner(blocks);  // before the flush: a refusal leaves what is pending pending
    if (only_needed)
        flush_for(blocks);
    else if (n == 1)
        return download(*blocks[0], cts);
    else
        flush();
    const size_t words = n * kBigCt + n;  // gathered ciphertexts, then the slot pointers
    Stage st(ctx_->stream, staging(words), words);
    const std::vector<const uint64_t*> src = source_ptrs(*this, blocks, "download of a trivial or lazy block");
    uint64_t* d_cts = st.reserve<uint64_t>(n * kBigCt);
    const uint64_t** d_src = st.put(src.data(), n, "download");
    hip_check(launch_gather_blocks(d_src, d_cts, (int)n, ctx_->stream), "download gather");
    hip_check(hipMemcpyAsync(cts, d_cts, n * kBigCt * 8, hipMemcpyDeviceToHost, ctx_->stream), "download");
    wait_check(ctx_, "download");
}

// ------------------------------------------------------------------ resident client key
bool Engine::encrypt_resident(fhe_client_key* ck, const uint64_t* pts, size_t n, Blocks* out) {
    engine_check(host_mode_ == kDevice, "encrypt_resident on a host-only engine");
    engine_check(ctx_->has_client, "encrypt_resident without a resident client key");
    out->clear();
    if (n == 0) return true;
    const ChaChaStream before = ck->enc_rng;
    engine_check(before.word_pos() % 2 == 0, "encryption stream off a 64-bit word");
    if (!encrypt_big_skip(ck, n)) return false;
    fault_point(kFaultClient, "CLIENT");
    const size_t words = 2 * n;  // the scaled plaintexts, then the slot pointers
    Stage st(ctx_->stream, staging(words), words);
    *out = fresh_blocks(n, 3);
    const std::vector<uint64_t*> dst = slot_ptrs(*out);
    const uint64_t* d_pts = st.put(pts, n, "client plaintexts");
    uint64_t** d_dst = st.put(dst.data(), n, "client slots");
    hip_check(ctx_->client_stage_stream(before, ck->params.glwe_noise_log2), "client stream parameters");
    hip_check(launch_client_encrypt(ctx_->d_client, d_dst, d_pts, n, ctx_->stream), "client encryption");
    hip_check(hipStreamSynchronize(ctx_->stream), "upload sync");  // host buffers may go, the staging be reused
    ctx_->client_enc_blocks += n;
    return true;
}

void Engine::phases_many(const std::vector<const Block*>& blocks, uint64_t* phases, bool only_needed) {
    engine_check(host_mode_ == kDevice, "phases_many on a host-only engine");
    engine_check(ctx_->has_client, "phases_many without a resident client key");
    const size_t n = blocks.size();
    if (n == 0) return;
    check_owner(blocks);  // before the flush: a refusal leaves what is pending pending
    if (only_needed)
        flush_for(blocks);
    else
        flush();
    fault_point(kFaultClient, "CLIENT");
    const size_t words = 2 * n;  // the slot pointers, then the phases
    Stage st(ctx_->stream, staging(words), words);
    const std::vector<const uint64_t*> src = source_ptrs(*this, blocks, "decryption of a trivial or lazy block");
    const uint64_t** d_src = st.put(src.data(), n, "phase slots");
    uint64_t* d_ph = st.reserve<uint64_t>(n);
    hip_check(launch_client_phase(ctx_->d_client, d_src, d_ph, n, ctx_->stream), "decryption phases");
    hip_check(hipMemcpyAsync(phases, d_ph, n * 8, hipMemcpyDeviceToHost, ctx_->stream), "phase download");
    wait_check(ctx_, "decryption phases");
    ctx_->client_phase_blocks += n;
}

void Engine::sync() {
    flush();
    wait_check(ctx_, "sync");
}

Blocks Engine::adopt_device(const uint64_t* d_cts, size_t n) {
    if (n == 0) return {};
    Stage st(ctx_->stream, staging(n), n);  // the slot pointers
    Blocks out = fresh_blocks(n, 0);        // degree and noise are the caller's to set
    const std::vector<uint64_t*> dst = slot_ptrs(out);
    uint64_t** d_dst = st.put(dst.data(), n, "adopt");
    hip_check(launch_scatter_blocks(d_cts, d_dst, (int)n, ctx_->stream), "adopt scatter");
    hip_check(hipStreamSynchronize(ctx_->stream), "adopt sync");  // the pointer staging may be reused
    return out;
}

void Engine::gather_device(const std::vector<const Block*>& blocks, uint64_t* d_out) {
    check_owner(blocks);
    flush();
    const size_t n = blocks.size();
    if (n == 0) return;
    Stage st(ctx_->stream, staging(n), n);  // the slot pointers
    const std::vector<const uint64_t*> src = source_ptrs(*this, blocks, "gather of a trivial or lazy block");
    const uint64_t** d_src = st.put(src.data(), n, "gather");
    hip_check(launch_gather_blocks(d_src, d_out, (int)n, ctx_->stream), "gather");
    hip_check(hipStreamSynchronize(ctx_->stream), "gather sync");
}

}  // namespace fhe
