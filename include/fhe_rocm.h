/*
 * fhe_rocm.h -- C ABI of the MI355X-native TFHE radix-integer engine.
 *
 * Drop-in boundary for the hot path of coset-io/fhe-sign: the tfhe-rs high-level API that
 * BigUintFHE (src/biguint.rs) and Schnorr::sign_fhe_with_k0 (src/schnorr.rs:235-290) call.
 * Every entry point cites the reference interface it replaces.  Plain pointers and sizes only;
 * no torch or HIP types cross this boundary.  All functions return FHE_OK (0) or a negative
 * status; fhe_last_error() gives the message (thread-local).  Nothing aborts across the ABI
 * (the reference panics via unwrap at src/biguint.rs:207; here that is FHE_ERR_*).
 *
 * Threading: like tfhe-rs's thread-local `set_server_key` (src/schnorr.rs:443), a server key is
 * installed per context and a context is used by one host thread at a time.  There is no lock
 * inside a context.  What that means, piece by piece:
 *  - Contexts are independent across threads: any number of threads may each drive a context of
 *    their own at once, device or simulated, on one GPU or several.  A context may move between
 *    threads as long as its uses do not overlap; every entry point selects the context's device
 *    itself, whatever the calling thread's current device is.
 *  - A context's handles (fhe_radix, fhe_biguint, column forms, lists made from its values) count
 *    as the context, their destroy calls included: destroying a handle from another thread while
 *    its context is in use is a misuse.
 *  - A client key carries a mutable encryption stream (fhe_client_key_seed_encryption) and belongs
 *    to one thread at a time.
 *  - Server, public, compression and re-keying key objects are read-only once made and may be
 *    installed into several contexts from several threads.
 *  - fhe_last_error() is per thread: a thread reads the message of its own last refusal.
 *  - fhe_host_set_tuning is process-wide (test hook): set before any op runs on any thread.
 * tools/threads_host_check.c drives four simulated contexts on four threads (under the host
 * ThreadSanitizer build: tools/tsan_host.sh); tests/test_threads.py and tests/test_threads_gpu.py
 * pin the same on the Python layer and on device contexts.
 *
 * Errors after validation: a call can fail after its arguments were accepted -- a HIP status, a bounded wait, an
 * engine check.  What such a failure leaves behind:
 *  - The context stays usable: the next call is served as if the failed one had not been made.
 *  - Every handle made before the call reads the same value afterwards, its reference value.  A failed call never
 *    makes a later read return anything else: a bootstrap that was recorded and not launched is still pending,
 *    never marked written.
 *  - Work recorded before the failure stays pending and is retried by the next flush, whole: levels the failed
 *    flush had launched are launched again, from inputs that are held until a flush completes, and the retried
 *    ciphertext words equal an unfailed run's.  fhe_ctx_stats, fhe_ctx_level_log and the launch trace count what
 *    was launched: a level launched twice counts twice, the level at which a flush failed does not count.  What
 *    the failed call itself recorded belongs to no handle and is dropped as dead.
 *  - When a signer entry point returns, with FHE_OK or with an error: no helper thread is running, no deferred
 *    upload is armed, and the client key's encryption stream is where a successful call with the same inputs
 *    leaves it -- the key may be used, or freed, at once.
 * Out of scope: under a communicator a failure is collective by design (the communicator is aborted), and a failed
 * key install leaves the context without that key, as each install documents.
 * tests/test_failure_paths.py and tests/test_failure_paths_gpu.py drive these paths through the host-side fault
 * point below (FHE_TUNE_FAULT_SITES); tools/faults_host_check.c does so under the host AddressSanitizer build
 * (tools/asan_faults_host.sh).
 *
 * Ciphertext layout (one radix block = one LWE ciphertext under the big key):
 *   uint64_t[2049] = mask[2048] then body.  A radix integer of B bits has B/2 blocks, LSB first.
 */
#ifndef FHE_ROCM_H
#define FHE_ROCM_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FHE_OK 0
#define FHE_ERR_INVALID (-1)
#define FHE_ERR_HIP (-2)
#define FHE_ERR_NO_KEY (-3)
#define FHE_ERR_ALLOC (-4)
#define FHE_ERR_UNSUPPORTED (-5)
#define FHE_ERR_TIMEOUT (-6) /* a collective's peers did not arrive before the deadline */

#define FHE_LWE_BIG_SIZE 2049u /* big LWE ciphertext words (k*N + 1) */

/* Parameter set.  Default = tfhe 0.10.0 ConfigBuilder::default() shape (2_2 radix blocks,
 * KS->PBS, TUniform); replaces `ConfigBuilder::default().build()` (src/schnorr.rs:441,
 * src/perf_test.rs:9).  polynomial_size 2048, glwe_dimension 1, pbs_level 1, ks_level 5,
 * ks_base_log 3 are fixed by the kernels; the others may vary. */
typedef struct fhe_params {
    uint32_t lwe_dimension;   /* n (834); 1 .. 2048, a multiple of the grouping.  Pinned word for word to the
                               * oracle at 834 and at 1, 2, 15, 16, 255, 256, 833, 2048 (2, 16, 256, 2048
                               * multi-bit too), every n <= 33 on the latency path
                               * (tests/test_lwe_dims_gpu.py); a context may be re-keyed between them */
    uint32_t glwe_dimension;  /* k (1) */
    uint32_t polynomial_size; /* N (2048) */
    uint32_t pbs_base_log;    /* 23 */
    uint32_t pbs_level;       /* 1 */
    uint32_t ks_base_log;     /* 3 */
    uint32_t ks_level;        /* 5 */
    uint32_t lwe_noise_log2;  /* TUniform bound, small key (45, recalled tfhe 0.10; 44 until r6) */
    uint32_t glwe_noise_log2; /* TUniform bound, big/GLWE key (17) */
    uint32_t message_modulus; /* 4; a power of two, 2 .. 64 -- the message space, below */
    uint32_t carry_modulus;   /* 4; a power of two, 1 .. 64, with message_modulus * carry_modulus <= 64 */
    uint32_t grouping;        /* blind rotation: 1 = classic (one CMUX per key bit, tfhe-rs'
                                 ClassicPBS, the default), 2 = multi-bit (tfhe-rs' MultiBitPBS shape:
                                 two key bits per external product, 3 GGSWs per pair; the client key
                                 and every decrypted result are unchanged).  0 is read as 1. */
} fhe_params;
/* The message space.  mc = message_modulus * carry_modulus values per block, delta = 2^63 / mc, one value's box
 * in the accumulator polynomial 2048 / mc coefficients wide.
 *   Any space: key generation and (de)serialization, fhe_encrypt_block(s) / fhe_decrypt_block, the resident
 *     client key, fhe_lut_register (a table of exactly mc entries), fhe_pbs_batch(_device), fhe_keyswitch_batch,
 *     fhe_pbs_lincomb_batch, fhe_oprf_blocks (bits <= log2 message_modulus), the compact public key, compression
 *     and re-keying keys, fhe_compress_host / fhe_switched_compress_host and their readers (a block's degree
 *     byte < mc), the row-level hooks.
 *   Message 4, carry 4 exactly: everything that makes, reads or computes on a radix value -- fhe_radix_*,
 *     fhe_biguint_*, fhe_columns_*, the seeded forms (fhe_*_encrypt_seeded, fhe_seeded_deserialize,
 *     fhe_seeded_expand_*), compact lists (fhe_compact_builder_push_*, fhe_compact_list_deserialize,
 *     fhe_compact_list_expand_*), fhe_compressed_expand_*, fhe_switched_expand_*, fhe_*_random*, and every
 *     fhe_schnorr_* that takes a context.  Under a key of any other space -- another split of 16 included --
 *     they return FHE_ERR_INVALID with a message that names message_modulus, before anything is encrypted,
 *     recorded or launched; the client key's encryption stream does not move.
 *   mc   box   half-box   half-box / sigma of the modulus switch at n = 834 (6.05 grid steps of 4096; derived)
 *   2    1024  512        84.6
 *   4    512   256        42.3
 *   8    256   128        21.2
 *   16   128   64         10.6
 *   32   64    32         5.3
 *   64   32    16         2.6  (about one wrong decode in 120 bootstraps: a space for small dimensions)
 * Pinned word for word to the oracle at 2x1, 2x2, 4x2, 2x8, 8x2, 16x1, 4x8, 8x8, 64x1 (tests/test_msg_spaces_gpu.py);
 * a context may be re-keyed between spaces: registered tables survive exactly when mc and delta do. */

typedef struct fhe_client_key fhe_client_key;
typedef struct fhe_server_key fhe_server_key;
typedef struct fhe_ctx fhe_ctx;
typedef struct fhe_radix fhe_radix;     /* FheUint<num_bits> (radix integers, below) */
typedef struct fhe_biguint fhe_biguint; /* BigUintFHE (below) */

const char* fhe_last_error(void);
int fhe_params_default(fhe_params* out);
/* The default parameters with the multi-bit blind rotation (grouping 2): same client key shape, same
 * keyswitch, 1.5x the bootstrapping-key size, half the serial CMUX chain (see fhe_params.grouping). */
int fhe_params_multi_bit(fhe_params* out);

/* ---------------------------------------------------------------------------------- keys */
/* Replaces tfhe::generate_keys(config) (src/schnorr.rs:441-442, src/biguint.rs:277,
 * src/perf_test.rs:12), which draws from the OS CSPRNG.  Every key stream (secret keys, KSK, BSK,
 * encryption) is ChaCha20 under one 256-bit key: pass 32 bytes of OS entropy (getrandom /
 * /dev/urandom) as `key`.  The key bytes are the client's secret -- whoever holds them can rebuild
 * the client key. */
int fhe_generate_keys_keyed(const fhe_params* params, const uint8_t key[32],
                            fhe_client_key** client_key, fhe_server_key** server_key);
/* DETERMINISTIC, INSECURE -- tests and golden vectors only: the 256-bit key is the public
 * expansion {seed, "FHES", 0...} of a 64-bit `seed`, so anyone can rebuild the client key. */
int fhe_generate_keys(const fhe_params* params, uint64_t seed, fhe_client_key** client_key,
                      fhe_server_key** server_key);
/* The same keys (identical words) generated on the GPU of `ctx` (keygen
 * dominates setup).  The ChaCha streams are counter-indexed, so the host's sequential draws become
 * one stream block per thread; the key is downloaded into the returned handle and not installed
 * (call fhe_set_server_key as after fhe_generate_keys).  ctx needs no server key. */
int fhe_generate_keys_device_keyed(fhe_ctx* ctx, const fhe_params* params, const uint8_t key[32],
                                   fhe_client_key** client_key, fhe_server_key** server_key);
/* the deterministic test-seed form (INSECURE, as fhe_generate_keys) */
int fhe_generate_keys_device(fhe_ctx* ctx, const fhe_params* params, uint64_t seed,
                             fhe_client_key** client_key, fhe_server_key** server_key);
void fhe_client_key_destroy(fhe_client_key* ck);
void fhe_server_key_destroy(fhe_server_key* sk);
/* The parameter set a key was generated for (e.g. after deserialization). */
int fhe_client_key_params(const fhe_client_key* ck, fhe_params* out);
int fhe_server_key_params(const fhe_server_key* sk, fhe_params* out);
/* Raw key material (tests / serialization): sizes in uint64 words. */
int fhe_client_key_export(const fhe_client_key* ck, uint64_t* lwe_sk, size_t lwe_len,
                          uint64_t* glwe_sk, size_t glwe_len);
int fhe_server_key_export(const fhe_server_key* sk, uint64_t* ksk, size_t ksk_len, uint64_t* bsk,
                          size_t bsk_len);
/* Serialization: this engine's own versioned, checksummed little-endian format
 * (magic "FHEROCM", serial.h).  The reference never serializes and tfhe-rs's bincode/versionable wire
 * format is not reproduced (no tfhe-rs fixture exists here to pin it).  Size query: call with
 * buf = NULL to get *len; a buffer smaller than *len gives FHE_ERR_INVALID.  Deserializers validate
 * magic, version, kind, length, checksum, parameters and every count; the client key carries its
 * encryption-stream state, so encryption continues exactly where the saved key left off. */
int fhe_client_key_serialize(const fhe_client_key* ck, uint8_t* buf, size_t cap, size_t* len);
int fhe_client_key_deserialize(const uint8_t* buf, size_t len, fhe_client_key** ck);
int fhe_server_key_serialize(const fhe_server_key* sk, uint8_t* buf, size_t cap, size_t* len);
int fhe_server_key_deserialize(const uint8_t* buf, size_t len, fhe_server_key** sk);
/* Re-seed the client key's encryption stream (deterministic tests). */
int fhe_client_key_seed_encryption(fhe_client_key* ck, uint64_t seed, uint32_t stream);

/* Shortint block encrypt/decrypt (the per-block step under FheUint32::try_encrypt,
 * src/biguint.rs:26, and FheDecrypt, src/biguint.rs:70).  value < message*carry modulus. */
int fhe_encrypt_block(fhe_client_key* ck, uint64_t value, uint64_t* ct /*2049*/);
/* n blocks at once (cts: n x 2049 words): the same ciphertexts and stream state as n calls of
 * fhe_encrypt_block, computed on several host threads (each on a seeked copy of the stream) */
int fhe_encrypt_blocks(fhe_client_key* ck, const uint64_t* values, size_t n, uint64_t* cts);
int fhe_decrypt_block(const fhe_client_key* ck, const uint64_t* ct, uint64_t* value /*msg+carry*/);

/* ------------------------------------------------------------------------------- context */
int fhe_ctx_create(int device, fhe_ctx** ctx);
void fhe_ctx_destroy(fhe_ctx* ctx);
/* Replaces tfhe::set_server_key(server_key) (src/schnorr.rs:443): uploads KSK + BSK to this
 * context's GPU and converts the BSK to the Fourier domain there. */
int fhe_set_server_key(fhe_ctx* ctx, const fhe_server_key* sk);
/* Fourier BSK as held on the device (tests: bit-exact check against the CPU restatement);
 * layout [n][row][poly][16][64] complex f64. */
int fhe_ctx_export_fourier_bsk(fhe_ctx* ctx, double* out, size_t len_doubles);
int fhe_ctx_sync(fhe_ctx* ctx);

/* ------------------------------------------------------------------- raw PBS boundary */
/* Register a univariate lookup table f: [0, msg*carry) -> [0, msg*carry). */
int fhe_lut_register(fhe_ctx* ctx, const uint32_t* table, uint32_t table_len, uint32_t* lut_id);
/* Keyswitch + bootstrap `count` big-key LWE blocks, block i through LUT lut_ids[i].
 * Host pointers; synchronous. */
int fhe_pbs_batch(fhe_ctx* ctx, const uint64_t* in, size_t count, const uint32_t* lut_ids,
                  uint64_t* out);
/* Same on device pointers, enqueued on the context stream (asynchronous). */
int fhe_pbs_batch_device(fhe_ctx* ctx, const uint64_t* d_in, size_t count,
                         const uint32_t* d_lut_ids, uint64_t* d_out);
/* Device memory helpers (so callers need no HIP types). */
void* fhe_device_alloc(fhe_ctx* ctx, size_t bytes);
int fhe_device_free(fhe_ctx* ctx, void* p);
int fhe_memcpy_h2d(fhe_ctx* ctx, void* dst, const void* src, size_t bytes);
int fhe_memcpy_d2h(fhe_ctx* ctx, void* dst, const void* src, size_t bytes);
/* Profiling: time of the last fhe_pbs_batch_device split by stage (ms, HIP events). */
int fhe_ctx_last_pbs_timing(fhe_ctx* ctx, float* ks_ms, float* br_ms);
int fhe_ctx_enable_timing(fhe_ctx* ctx, int enable);
/* Clock probe of the throughput blind rotate: while enabled, thread 0 of every workgroup adds its
 * lifetime in shader cycles (s_memtime) and in 100 MHz ticks (s_memrealtime); enabling resets the
 * sums.  read_clock waits for the stream: shader clock = cycles / ticks x 100 MHz. */
int fhe_ctx_enable_clock(fhe_ctx* ctx, int enable);
int fhe_ctx_read_clock(fhe_ctx* ctx, uint64_t* cycles, uint64_t* ticks, uint64_t* workgroups);
/* Batches of at most `threshold` bootstraps use the latency-optimised blind rotate (one
 * ciphertext per 512-thread workgroup); larger ones the throughput kernel.  Default 256. */
int fhe_ctx_set_wide_threshold(fhe_ctx* ctx, int threshold);
/* Throughput blind-rotate kernel for levels above the threshold, 4 waves per ciphertext: FHE_BR_QY
 * (br_qy.hip, two workgroup barriers per CMUX; classic and multi-bit parameters) is the only one.
 * The retired kernels -- FHE_BR_NARROW (round 1), FHE_BR_PAIR (rounds 2-3), FHE_BR_QUAD (rounds 1-4,
 * the multi-bit kernel until r4) and FHE_BR_QX (round 4, four barriers per CMUX; sources in
 * tools/retired/) -- are refused with FHE_ERR_INVALID.  Every blind-rotate kernel that ever ran here
 * produced identical bits. */
#define FHE_BR_NARROW 0
#define FHE_BR_QUAD 1
#define FHE_BR_PAIR 2
#define FHE_BR_QX 3
#define FHE_BR_QY 4
#define FHE_BR_QY2 5 /* br_qy.hip k_blind_rotate_qy2<1>: classic, two ciphertexts per workgroup sharing key slices */
#define FHE_BR_QY4 6 /* k_blind_rotate_qy2<2>: two such pairs per 8-wave workgroup (the pairs' key reads meet in L1) */
/* default.  Classic levels go to k_blind_rotate_qz where its rounds of 1024 bootstraps (256 CUs x 2
 * workgroups x 2 ciphertexts) fill well: every level of >= 3072, and a level above 960 whose last round
 * is full or more than three quarters full (count % 1024 == 0 or > 768).  Every other level above the
 * latency threshold, and every multi-bit level, goes to k_blind_rotate_qy. */
#define FHE_BR_AUTO 7
#define FHE_BR_QZ 9 /* br_qy.hip k_blind_rotate_qz: classic, two ciphertexts per workgroup, one wave per polynomial in the transforms (no lane transposes); 8 is not a kind */
int fhe_ctx_set_br_kernel(fhe_ctx* ctx, int kind);

/* Modulus switch of the bootstrap's input.  The blind rotation rounds every word of the keyswitched row to the
 * 2^52 grid (12 bits kept).  res(x) = (int64)((x + 2^51) & (2^52 - 1)) - 2^51 is the signed distance of x from
 * the multiple of 2^52 it is rounded to, in [-2^51, 2^51).  The rounding adds sum_i res(a[i]) s[i] to the
 * phase; for a binary key of weight hw that is a standard deviation of sqrt(hw / 12 + 1 / 12) grid steps
 * (5.9 at n = 834, of a decode margin of 64): the largest term of a bootstrap's failure probability.
 * FHE_MS_STANDARD (default) leaves the rows as the keyswitch wrote them.
 * FHE_MS_CENTERED removes the public half of that sum first (tfhe-rs' centered mean noise reduction): with
 *   S = sum_{i < n} res(a[i])  (int64; |S| <= n 2^51)      b' = b - (uint64)(S >> 1)  (arithmetic shift, wrapping)
 * the row (a, b') enters the unchanged modulus switch.  The remaining error sum_i res(a[i]) (s[i] - 1/2) has
 * standard deviation sqrt(n / 48 + 1 / 12) whatever the key is: 4.2 steps at n = 834.  Mask words are
 * unchanged; a row whose mask words are multiples of 2^52 is unchanged.  One more gfx950 kernel (k_ms_center,
 * ms_center.hip) runs on the stream right after every keyswitch kernel the context launches: fhe_pbs_batch
 * [_device], fhe_keyswitch_batch (the rows as the blind rotation will read them), fhe_pbs_lincomb_batch (its
 * `small` output included) and every level of the radix layer, fan-out slices included.  The decompression
 * bootstrap is not touched: its 12-bit stored words have no residue.  Same keys, LUTs, noise labels.
 * The mode applies to levels launched after the call; the call launches and flushes nothing.  Per context:
 * under a communicator every rank sets the same mode (as with fhe_ctx_set_br_kernel, nothing is broadcast),
 * or the ranks' slices of a level differ.  An unknown mode: FHE_ERR_INVALID with a message. */
#define FHE_MS_STANDARD 0
#define FHE_MS_CENTERED 1
int fhe_ctx_set_modulus_switch(fhe_ctx* ctx, int mode);
int fhe_ctx_get_modulus_switch(fhe_ctx* ctx, int* mode);
/* The definition on the host, in place on `count` rows of `stride` words (mask words 0 .. n-1, body at n, the
 * rest padding that is neither read nor written); no context, no GPU.  FHE_ERR_INVALID unless
 * 1 <= n <= FHE_MS_CENTER_MAX_N (the sum stays inside int64) and stride >= n + 1. */
#define FHE_MS_CENTER_MAX_N 2048u
int fhe_ms_center_host(uint64_t* rows, size_t count, uint32_t n, size_t stride);
/* Test hook: k_ms_center over host rows -- upload with the given stride, run, download.  Needs no server key,
 * so any n runs without a key generation.  Same validation; at most 2^31 - 1 rows.  Synchronous. */
int fhe_ms_center_rows(fhe_ctx* ctx, uint64_t* rows, size_t count, uint32_t n, size_t stride);
/* Measurement hook: k_ms_center alone, `reps` launches over count x stride scratch words between two HIP
 * events on the context's stream; *ms = the mean per launch. */
int fhe_ctx_time_ms_center(fhe_ctx* ctx, size_t count, uint32_t n, size_t stride, uint32_t reps, float* ms);

/* Keyswitch: int8 matrix-core contraction against the KSK's byte planes (FHE_KS_MFMA, default) or
 * the 64-bit VALU kernel (FHE_KS_VALU).  Both are exact: identical small LWE words. */
#define FHE_KS_VALU 0
#define FHE_KS_MFMA 1
int fhe_ctx_set_ks_kernel(fhe_ctx* ctx, int kind);
/* The keyswitch alone: `count` big-key LWE blocks (host, count x 2049) -> small-key LWE (host,
 * count x (n + 1) words, the 64-bit words before the modulus switch), on the kernel
 * fhe_ctx_set_ks_kernel selected -- the same launch fhe_pbs_batch makes.  Synchronous.  count == 0 is
 * fine; without a server key FHE_ERR_NO_KEY. */
int fhe_keyswitch_batch(fhe_ctx* ctx, const uint64_t* in, size_t count, uint64_t* small);
/* Bootstraps of linear combinations, as the radix layer issues them: item i is
 *   PBS_lut_ids[i]( sum_{t in [term_off[i], term_off[i+1])} term_coef[t] * blocks[term_src[t]] + cst[i] )
 * with cst[i] added to the body.  One descriptor per item: 1..6 terms in the inline form (coefficients
 * must fit int32), 7..32 terms through a term table staged after the descriptors, exactly what the
 * radix executor's flush stages and launches (keyswitch with the fused linear prologue, then the
 * blind rotate the batch size selects).  `small` (nullable, count x (n + 1)) receives the keyswitched
 * words, `out` (nullable, count x 2049) the bootstrapped blocks; the blind rotate runs only when
 * `out` is given.  Host pointers; synchronous.  FHE_ERR_INVALID, before any kernel runs, for: an item
 * with no term or more than 32, a block index >= nblocks, an inline coefficient outside int32, an
 * unknown LUT id, term_off not starting at 0 or decreasing. */
int fhe_pbs_lincomb_batch(fhe_ctx* ctx, const uint64_t* blocks, size_t nblocks, const uint32_t* term_off,
                          const uint32_t* term_src, const int64_t* term_coef, const uint64_t* cst,
                          const uint32_t* lut_ids, size_t count, uint64_t* small, uint64_t* out);

/* ------------------------------------------------------------------- multi-GPU fan-out */
/* One process per GPU.  All ranks run the same radix program on identical inputs
 * (same keys, same ciphertexts); a dependency level with at least `min_level` bootstraps is split
 * over the ranks and its outputs all-gathered with RCCL on the engine stream.  Smaller levels are
 * computed redundantly on every rank.  Rank 0 creates the id and shares it out of band. */
#define FHE_COMM_ID_BYTES 128
#define FHE_COMM_DEFAULT_TIMEOUT_MS 120000u
int fhe_comm_unique_id(uint8_t id[FHE_COMM_ID_BYTES]);
/* Non-blocking communicator init (RCCL ncclCommInitRankConfig, blocking = 0) polled against a
 * deadline: if a peer never joins, the communicator is aborted and FHE_ERR_TIMEOUT returned on the
 * ranks that did -- no rank is left waiting inside the library.  The same deadline bounds the
 * enqueue of every later collective (all-gather, key and operand broadcasts) and, while a
 * communicator is attached, every wait for the engine's stream (fhe_ctx_sync, downloads,
 * decryption): a stream that makes no progress for the deadline -- no launched level completes, e.g.
 * a peer died after a collective was enqueued -- gives FHE_ERR_TIMEOUT (or the communicator's error)
 * and an aborted, detached communicator instead of a hang; a long flush whose levels keep completing
 * is never cut off.  Callers should still agree out of band that every rank is ready before
 * attaching (fhe_sign/dist.py: attach_fanout).  All ranks must issue the same radix program and the
 * same host reads (downloads, syncs) in the same order, since every flush schedules collectively. */
int fhe_ctx_attach_comm_timeout(fhe_ctx* ctx, const uint8_t id[FHE_COMM_ID_BYTES], int nranks, int rank,
                                uint32_t timeout_ms);
/* change the attached communicator's deadline (ms, > 0); FHE_ERR_INVALID without a communicator */
int fhe_ctx_set_comm_timeout(fhe_ctx* ctx, uint32_t timeout_ms);
/* the same with FHE_COMM_DEFAULT_TIMEOUT_MS */
int fhe_ctx_attach_comm(fhe_ctx* ctx, const uint8_t id[FHE_COMM_ID_BYTES], int nranks, int rank);
/* Collective over the attached communicator: rank `root` (which has a server key installed)
 * replicates it to every rank device-to-device (RCCL broadcast over xGMI: parameters, KSK, Fourier
 * BSK; each receiver derives the kernels' layouts itself).  Afterwards every rank's context is as if
 * fhe_set_server_key had been called with the root's key.  A receiver keeps its previously installed
 * key (if any) until the collectives and conversions have succeeded: on any error it is unchanged. */
int fhe_ctx_broadcast_server_key(fhe_ctx* ctx, int root);
/* Collective operand distribution for the fan-out (config 5a): all ranks must run the radix
 * program on byte-identical ciphertexts, but an input such as sign_fhe_with_k0's encrypted private
 * key (src/schnorr.rs:235,270-277) arrives on one rank.  Rank `root` passes its handle in *x;
 * every other rank receives a new handle in *x (its previous value is not read) whose block
 * ciphertexts and metadata equal the root's (RCCL broadcast over xGMI, device to device).  Every
 * rank needs an installed server key of the same message/carry parameters.  Failures are agreed
 * before any data moves (every rank returns an error, none waits), and the final wait is bounded
 * by the communicator's timeout (then the communicator is aborted).  Without a communicator (one
 * GPU, emulated ranks) the root's blocks take the receiving path locally (gather, scatter into new
 * slots) and *x is replaced by the new handle; the caller still owns the one it passed. */
int fhe_ctx_broadcast_radix(fhe_ctx* ctx, fhe_radix** x, int root);
int fhe_ctx_broadcast_biguint(fhe_ctx* ctx, fhe_biguint** x, int root);
/* parameters of the server key installed in a context */
int fhe_ctx_params(const fhe_ctx* ctx, fhe_params* out);
int fhe_ctx_detach_comm(fhe_ctx* ctx);
/* TEST HOOK -- several ranks on one GPU (RCCL refuses two ranks per device).  Attaches a host-staged
 * transport in place of RCCL: the engine's collectives (the fan-out all-gather, the dead-node min
 * all-reduce, the key / operand broadcasts and their agreements) become stream syncs, host copies and
 * calls of these callbacks (the tests implement them over a gloo process group), so every rank-
 * dependent branch of the production fan-out runs with real rank slices.  Each callback returns 0 on
 * success; bytes/n are the same on every rank.  Detach with fhe_ctx_detach_comm.  RCCL stays the only
 * production transport: nothing else selects this one. */
typedef struct fhe_test_transport {
    void* user;
    /* host[0..bytes) of rank `root` to every rank, in place */
    int (*bcast)(void* user, void* host, size_t bytes, int root);
    /* host holds nranks segments of seg_bytes, this rank's filled: fill the others */
    int (*allgather)(void* user, void* host, size_t seg_bytes);
    /* host[0..n) = element-wise min over the ranks, in place */
    int (*allreduce_min_u8)(void* user, uint8_t* host, size_t n);
} fhe_test_transport;
int fhe_ctx_attach_test_transport(fhe_ctx* ctx, const fhe_test_transport* tx, int nranks, int rank);
/* split threshold (default 257: above one ciphertext per CU) and, for single-GPU tests, the number of emulated ranks (0 = off) */
int fhe_ctx_set_fanout(fhe_ctx* ctx, uint32_t min_level, int emulate_ranks);
/* rank, world (emulated ranks counted) and the number of levels split so far */
int fhe_ctx_fanout_info(const fhe_ctx* ctx, int* rank, int* nranks, uint64_t* fanout_levels);

/* ------------------------------------------------------------------- radix integers */
/* FheUint<num_bits> (num_bits even, <= FHE_RADIX_MAX_BITS): num_bits/2 radix blocks, device-resident.
 * Replaces tfhe's FheUint8/32/64 as used at src/biguint.rs:26,135-143,221-248 and
 * src/perf_test.rs:19-54.  Arithmetic wraps modulo 2^num_bits (tfhe semantics).
 *
 * Ownership.  An fhe_radix, fhe_biguint or fhe_columns handle is a value of the context that made it (encrypt,
 * expand, deserialize, random, a broadcast's copy, or an op on its values).  Every entry point that takes a context
 * and a handle refuses a handle made under another context -- simulated or device, live or destroyed -- with
 * FHE_ERR_INVALID and a message that says "another context" (with the operand's name where the entry point has
 * one), before anything is recorded, staged, launched or read: both contexts stay as they were.  Values made by
 * fhe_radix_trivial (and the trivial blocks of any value) have no owner and are accepted everywhere.  The entry
 * points without a context (fhe_radix_clone, fhe_radix_cast with ctx = NULL, *_num_bits, fhe_biguint_len / _digit /
 * _to_radix / _from_digits, *_destroy) look at no owner; what they return shares its source's blocks, and its owner.
 * A handle may outlive its context (it keeps its blocks' storage alive) and is destroyed like any other.
 * A value stays its context's across fhe_set_server_key on the SAME context: whether it still means anything
 * under the new key is the caller's business, as under tfhe-rs' set_server_key. */
#define FHE_RADIX_MAX_BITS 4096
/* FheUint::try_encrypt (src/biguint.rs:26, src/perf_test.rs:19-21); words little-endian */
int fhe_radix_encrypt(fhe_ctx* ctx, fhe_client_key* ck, const uint64_t* words, uint32_t num_bits,
                      fhe_radix** out);
/* trivial (unencrypted-noise-free) constant, e.g. FheUint::encrypt_trivial */
int fhe_radix_trivial(fhe_ctx* ctx, const uint64_t* words, uint32_t num_bits, fhe_radix** out);
/* FheDecrypt (src/biguint.rs:70): nwords >= ceil(num_bits/64) */
int fhe_radix_decrypt(fhe_ctx* ctx, const fhe_client_key* ck, const fhe_radix* x, uint64_t* words,
                      size_t nwords);
int fhe_radix_num_bits(const fhe_radix* x, uint32_t* num_bits);
int fhe_radix_clone(const fhe_radix* x, fhe_radix** out);
void fhe_radix_destroy(fhe_radix* x);
/* raw block ciphertexts (num_bits/2 x 2049 words; trivial blocks are materialized) */
int fhe_radix_export(fhe_ctx* ctx, const fhe_radix* x, uint64_t* cts, size_t nwords);
/* FheUint + FheUint (src/biguint.rs:138,236,243,248; src/perf_test.rs:28) */
int fhe_radix_add(fhe_ctx* ctx, const fhe_radix* a, const fhe_radix* b, fhe_radix** out);
int fhe_radix_sub(fhe_ctx* ctx, const fhe_radix* a, const fhe_radix* b, fhe_radix** out);
/* FheUint * FheUint (src/biguint.rs:223; src/perf_test.rs:32) */
int fhe_radix_mul(fhe_ctx* ctx, const fhe_radix* a, const fhe_radix* b, fhe_radix** out);
/* &FheUint & u64 (src/biguint.rs:116,143; src/perf_test.rs:48) */
int fhe_radix_scalar_and(fhe_ctx* ctx, const fhe_radix* a, uint64_t mask, fhe_radix** out);
/* &FheUint >> u64 (src/biguint.rs:110,141); shift taken mod num_bits (src/biguint.rs:494-498) */
int fhe_radix_scalar_shr(fhe_ctx* ctx, const fhe_radix* a, uint32_t shift, fhe_radix** out);
int fhe_radix_scalar_shl(fhe_ctx* ctx, const fhe_radix* a, uint32_t shift, fhe_radix** out);
int fhe_radix_scalar_add(fhe_ctx* ctx, const fhe_radix* a, uint64_t s, fhe_radix** out);
/* FheUint * clear (src/schnorr.rs:588) */
int fhe_radix_scalar_mul(fhe_ctx* ctx, const fhe_radix* a, uint64_t s, fhe_radix** out);
/* FheUint / clear (src/perf_test.rs:54); divisor 0 -> FHE_ERR_INVALID */
int fhe_radix_scalar_div(fhe_ctx* ctx, const fhe_radix* a, uint64_t d, fhe_radix** out);
int fhe_radix_scalar_rem(fhe_ctx* ctx, const fhe_radix* a, uint64_t d, fhe_radix** out);
/* The same scalar ops with a clear operand of any width (little-endian u64 words), as tfhe's
 * scalar ops on FheUint256 take U256/u128 scalars.  BASELINE config 3: 256-bit radix divided by a
 * clear u32 / 128-bit divisor (src/perf_test.rs:54 at 256 bits).  Divisor 0 -> FHE_ERR_INVALID. */
int fhe_radix_scalar_and_words(fhe_ctx* ctx, const fhe_radix* a, const uint64_t* s, size_t nwords, fhe_radix** out);
int fhe_radix_scalar_add_words(fhe_ctx* ctx, const fhe_radix* a, const uint64_t* s, size_t nwords, fhe_radix** out);
int fhe_radix_scalar_mul_words(fhe_ctx* ctx, const fhe_radix* a, const uint64_t* s, size_t nwords, fhe_radix** out);
/* a * m + k for clear m, k (wrapping at a's width) in one carry propagation */
int fhe_radix_scalar_mul_add_words(fhe_ctx* ctx, const fhe_radix* a, const uint64_t* m, size_t nm, const uint64_t* k,
                                   size_t nk, fhe_radix** out);
int fhe_radix_scalar_div_words(fhe_ctx* ctx, const fhe_radix* a, const uint64_t* d, size_t nwords, fhe_radix** out);
int fhe_radix_scalar_rem_words(fhe_ctx* ctx, const fhe_radix* a, const uint64_t* d, size_t nwords, fhe_radix** out);
/* a mod (2^k_bits - c) for a public pseudo-Mersenne modulus (both moduli of secp256k1 are of this shape): folds
 * x <- (x mod 2^k) + (x >> k) c, their number fixed by a's width, k and c (never by data), then one conditional
 * subtraction.  k_bits even, 2 <= k_bits <= FHE_RADIX_MAX_BITS - 2; 0 < c < 2^(k_bits - 2) (c_words LSB first);
 * anything else is FHE_ERR_INVALID with a message.  a of any width; out is an FheUint<k_bits> of clean blocks.
 * Far cheaper than fhe_radix_scalar_rem_words with the same modulus, whose general division this avoids. */
int fhe_radix_rem_pseudo_mersenne(fhe_ctx* ctx, const fhe_radix* a, uint32_t k_bits, const uint64_t* c_words, size_t nc,
                                  fhe_radix** out);
/* (k + m * a) mod (2^k_bits - c) for public m, k below the modulus: m * a is never formed, the sum of
 * a_i * (m 4^i mod n) over a's blocks is, which leaves a few-block fold. */
int fhe_radix_scalar_mul_add_rem_pseudo_mersenne(fhe_ctx* ctx, const fhe_radix* a, const uint64_t* m, size_t nm,
                                                 const uint64_t* k, size_t nk, uint32_t k_bits, const uint64_t* c_words,
                                                 size_t nc, fhe_radix** out);
/* Ciphertext serialization (radix integers and BigUintFHE limb vectors; same format as the keys).
 * Deserialization needs a context whose server key has the same parameters; block degree / noise
 * metadata travels with the ciphertext and is checked against the radix layer's budget. */
int fhe_radix_serialize(fhe_ctx* ctx, const fhe_radix* x, uint8_t* buf, size_t cap, size_t* len);
int fhe_radix_deserialize(fhe_ctx* ctx, const uint8_t* buf, size_t len, fhe_radix** out);
/* FheUint / FheUint, FheUint % FheUint (encrypted divisor; SURVEY 8d config 3 stretch, 8f rank 1).
 * Division by an encrypted zero yields quotient 2^num_bits - 1 and remainder a (tfhe's convention).
 * fhe_radix_divrem returns both (either output may be NULL). */
int fhe_radix_div(fhe_ctx* ctx, const fhe_radix* a, const fhe_radix* b, fhe_radix** out);
int fhe_radix_rem(fhe_ctx* ctx, const fhe_radix* a, const fhe_radix* b, fhe_radix** out);
int fhe_radix_divrem(fhe_ctx* ctx, const fhe_radix* a, const fhe_radix* b, fhe_radix** q, fhe_radix** r);
/* FheUint::cast_from / cast_into (src/biguint.rs:110,116,221; src/perf_test.rs:40) */
int fhe_radix_cast(fhe_ctx* ctx, const fhe_radix* a, uint32_t num_bits, fhe_radix** out);
/* FheUint::min (src/perf_test.rs:44), max, lt (encrypted bool returned as a 2-bit radix) */
int fhe_radix_min(fhe_ctx* ctx, const fhe_radix* a, const fhe_radix* b, fhe_radix** out);
int fhe_radix_max(fhe_ctx* ctx, const fhe_radix* a, const fhe_radix* b, fhe_radix** out);
int fhe_radix_lt(fhe_ctx* ctx, const fhe_radix* a, const fhe_radix* b, fhe_radix** out);
/* &FheUint >> &FheUint (src/perf_test.rs:36), and <<: a shifted by (amount's value) mod (a's num_bits), for
 * every width of a -- a power of two or not -- and an amount of any width of its own: a narrower amount
 * counts as zero-extended, a wider one is read at its full width before the reduction (34-bit a, 66-bit
 * amount 2^65 + 1: a shift by (2^65 + 1) mod 34).  out has a's width.  When a's width is a power of two the
 * amount's low log2(num_bits) bits are the shift; any other width first reduces the amount mod num_bits
 * under encryption (a narrow clear-divisor remainder: more bootstraps and levels). */
int fhe_radix_shr(fhe_ctx* ctx, const fhe_radix* a, const fhe_radix* amount, fhe_radix** out);
int fhe_radix_shl(fhe_ctx* ctx, const fhe_radix* a, const fhe_radix* amount, fhe_radix** out);
int fhe_radix_bitand(fhe_ctx* ctx, const fhe_radix* a, const fhe_radix* b, fhe_radix** out);
/* engine statistics since context creation: bootstraps executed and dependency levels */
int fhe_ctx_stats(fhe_ctx* ctx, uint64_t* pbs_count, uint64_t* levels);
/* The noise budget as enforced, over the bootstraps recorded since the last reset.  A bootstrap's input is a
 * linear combination of blocks; its label is sum coef^2 noise over the terms, its merged noise the same per SLOT
 * with a repeated slot's coefficients summed first (x * x, x & x, a value and its clone: 4x + x is 25 units, not
 * 17).  The engine holds the merged figure against its budget of 25.  max_label / max_merged: the largest of each;
 * n_above_label: bootstraps whose merged noise exceeds their label.  Outputs optional; reset != 0 clears the
 * counters.  Device and simulated contexts. */
int fhe_ctx_noise_audit(fhe_ctx* ctx, uint64_t* max_label, uint64_t* max_merged, uint64_t* n_above_label, int reset);
/* bootstraps per launched dependency level, in launch order, since the last reset (host-side
 * record, at most 2^20 levels): *n = the number recorded, min(cap, *n) written to sizes; reset != 0
 * clears the record.  bench.py replays these level sizes through the CPU restatement. */
int fhe_ctx_level_log(fhe_ctx* ctx, uint32_t* sizes, size_t cap, size_t* n, int reset);
/* Bit 31 of a level_log entry: the level was fanned out over the ranks (split + all-gather); the
 * low bits are its bootstrap count.  Only set while ranks are attached or emulated. */
#define FHE_LEVEL_SPLIT 0x80000000u
/* TEST HOOK -- the launch trace: what the engine enqueues on the context's stream, in that order, so that a test
 * can replay it against a reference of its own (tests/launch_replay.py).  Off by default (one branch per flush
 * and per eager op); fhe_ctx_trace turns it on and off, fhe_ctx_trace_read copies min(cap, *n) of the *n recorded
 * u64 words (reset != 0 clears the record).  The trace only reads: results, fhe_ctx_stats and fhe_ctx_level_log
 * are the same with it on or off.  At most 2^23 words are kept; a trace that would have passed them is refused
 * by fhe_ctx_trace_read with FHE_ERR_INVALID and a message (reset still clears it).  Records:
 *   FHE_TRACE_LEVEL    level number (as counted by fhe_ctx_stats), bootstraps, split flag; then one
 *   FHE_TRACE_NODE     per bootstrap, in launch order: dst address, LUT id, cst (the u64 added to the body),
 *                      nterms, then nterms x (src address, coefficient as int64)
 *   FHE_TRACE_LINCOMB  a linear combination without bootstrap: dst, cst, nterms, nterms x (src, coefficient)
 *   FHE_TRACE_WRITE    kind, n, n dst addresses: any other op that writes block slots -- kind 0 an upload
 *                      (a simulated context: an encryption's placeholder blocks), 1 a deferred upload (recorded
 *                      when it is enqueued, before the flush that follows it), 2 opaque: seeded / compact /
 *                      compressed / stored expansion, re-randomization, random values, a broadcast's copy
 * On a device context a node's fields are read back from the staged host buffer that is copied to the device:
 * the level's descriptors after the wide term tables and the scatter tables were written into them, a wide
 * combination's terms through the staged src[0] into the staged table, a fanned-out level's real destination
 * from its staged scatter table.  A dry or simulated engine stages nothing and records its scheduled nodes. */
#define FHE_TRACE_LEVEL 1
#define FHE_TRACE_NODE 2
#define FHE_TRACE_LINCOMB 3
#define FHE_TRACE_WRITE 4
int fhe_ctx_trace(fhe_ctx* ctx, int enable);
int fhe_ctx_trace_read(fhe_ctx* ctx, uint64_t* buf, size_t cap, size_t* n, int reset);
/* TEST HOOK, read-only: out[0] = bootstraps recorded and not launched, out[1] = 1 while a deferred upload is armed
 * (the signer's encryptions of e and k, uploaded before the next launch), out[2] = helper threads of such
 * encryptions still running.  A context without a key reports zeros. */
int fhe_ctx_pending_info(fhe_ctx* ctx, uint64_t out[3]);
/* Read-only hooks of the same tests.  *_block_addrs: *n = the value's block count (a BigUintFHE: its limbs' blocks,
 * 16 per limb, LSB first); with cap >= *n, addrs[k] = block k's device address (a simulated context: its
 * placeholder address), 0 for a trivial block, whose value goes to values[k] (optional).  cap == 0 only asks
 * for *n.  Nothing is flushed: a pending block's address is where its bootstrap will write. */
int fhe_radix_block_addrs(fhe_ctx* ctx, const fhe_radix* x, uint64_t* addrs, uint32_t* values, size_t cap, size_t* n);
int fhe_biguint_block_addrs(fhe_ctx* ctx, const fhe_biguint* x, uint64_t* addrs, uint32_t* values, size_t cap, size_t* n);
/* the registered table `id`: its kind and entries -- an integer table's 16 outputs, a half-step table's 16 signed
 * outputs in half message steps, an OPRF staircase's bit count in entries[0].  A hook of the radix layer's tests:
 * under a key of mc = message_modulus * carry_modulus <= 16 the first mc entries are the table and the rest 0;
 * under a larger space an integer or half-step table has more entries than the hook holds, and the call returns
 * FHE_ERR_INVALID with a message that says so ("the hook reports at most 16") */
#define FHE_LUT_INTEGER 0
#define FHE_LUT_HALF_STEP 1
#define FHE_LUT_OPRF 2
int fhe_ctx_lut_table(fhe_ctx* ctx, uint32_t id, int* kind, int32_t entries[16]);
/* tables [first, first + count) of the DEVICE table as it stands (a download of what the last launch saw, not the
 * host copy): count x 2048 words.  Device contexts only. */
int fhe_ctx_export_luts(fhe_ctx* ctx, uint32_t first, uint32_t count, uint64_t* polys);
/* Bootstraps this rank ran itself since context creation: its slice of every fanned-out level plus
 * every level it ran redundantly (with emulated ranks: rank 0's share). */
int fhe_ctx_rank_pbs(const fhe_ctx* ctx, uint64_t* pbs);
/* The engine's level scheduler on an explicit dependency graph (host only, no GPU): node i reads
 * nodes deps[dep_offsets[i] .. dep_offsets[i+1]) (all < i).  Writes each node's launch level
 * (1-based) to level_of[i] and the level count (= the critical path) to *nlevels.  mode 0: backward
 * list scheduling (the engine's default), 1: forward deadline-driven (FHE_SCHED=1). */
int fhe_schedule_levels(const int32_t* dep_offsets, const int32_t* deps, size_t n, int mode, int32_t* level_of,
                        int32_t* nlevels);
/* The same as the engine schedules under a fan-out over `ranks` GPUs: levels are filled to whole
 * latency rounds of every rank (multiples of 256 x ranks), so a filled level is split over the ranks
 * (fhe_ctx_set_fanout) and each rank's slice is at most one round. */
int fhe_schedule_levels_ranks(const int32_t* dep_offsets, const int32_t* deps, size_t n, int mode, int ranks,
                              int32_t* level_of, int32_t* nlevels);
/* Host-only check of the progress marks behind the bounded waits (fhe_ctx_sync with a communicator
 * attached): after `levels` launched levels with none completed, the largest number of levels
 * between consecutive outstanding marks (at most 32 are kept; their gaps stay even). */
int fhe_progress_marks_probe(uint32_t levels, uint32_t* max_gap);
/* Host-only check of the BigUintFHE limb algorithms (no GPU, no key): a * b (k == NULL) or k + a * b on
 * publicly known limbs (LSB first) through the engine's host folding -- the same radix code path as
 * fhe_biguint_mul / _mul_add, every lookup evaluated on the host.  Writes up to `cap` limbs to out
 * and the limb count to *n. */
int fhe_host_biguint_mul(const uint32_t* a, size_t la, const uint32_t* b, size_t lb, const uint32_t* k, size_t lk,
                         int mode, uint32_t* out, size_t cap, size_t* n);
/* Dry run (no GPU): the bootstraps and launch levels the engine schedules for the la x lb BigUintFHE mul
 * (or k + a * b with lk > 0 limbs of k) on encrypted limbs -- recorded and scheduled, nothing launched.
 * mode | FHE_HOST_STATS_COLUMNS: k + a * b in the signer's column form (fhe_biguint_mul_add_columns).
 * level_sizes (optional, up to cap entries): bootstraps per launched level. */
#define FHE_HOST_STATS_COLUMNS 0x100
/* mode | FHE_HOST_CALL_SITE (with lk > 0; fhe_host_biguint_mul_stats and fhe_host_sim_biguint_mul): the
 * reference's call site k + (a * b) as two ops -- fhe_biguint_mul, then fhe_biguint_add with the product
 * released before the flush -- instead of the one-call mul-add. */
#define FHE_HOST_CALL_SITE 0x200
/* mode | FHE_HOST_CALL_SITE | FHE_HOST_DECRYPT_SUM: the call site followed by fhe_biguint_decrypt of the
 * sum, which reads the sum's column form and launches only what that depends on -- the statistics stop
 * there (the sum's own carry propagation stays pending; the sim checks the columns' value = the digits'). */
#define FHE_HOST_DECRYPT_SUM 0x400
/* The same dry run's recording-order fingerprint: a hash of every scheduled level's nodes in order (LUT,
 * coefficients, constants, producers by recording index; no addresses).  The multi-GPU fan-out needs it
 * equal on every rank: ranks scatter the all-gathered slices by their own node order. */
int fhe_host_biguint_mul_fingerprint(size_t la, size_t lb, size_t lk, int mode, uint64_t* fp);
/* Test hooks: the radix algorithms' size rules, process-wide (defaults = the product; a test moves a
 * threshold so that a small case takes the path the product takes at 256 bits).  *previous (optional)
 * gets the old value.  Not for production use; no environment variable changes them. */
#define FHE_TUNE_KARA_MIN 1            /* Karatsuba from this many blocks (default 24; 0 never) */
#define FHE_TUNE_KARA_COMPAT_MIN 2     /* ... for the compat chain's limb products (default 16; 0 never) */
#define FHE_TUNE_KARA_FORCE 3          /* 1: split publicly known operands too (host-fold checks) */
#define FHE_TUNE_DIV_R16_LEAD 4        /* encrypted division: leading radix-16 dividend blocks (default 32) */
#define FHE_TUNE_SCALAR_DIV_RESIDUE 5  /* public divisors: -1 size rule (default), 0 never, 1 where valid */
#define FHE_TUNE_FLUSH_DEPTH 6         /* launch the deferred graph in slices of this many levels (default 64; 0: on demand) */
/* TEST HOOK -- a host-side fault point, off by default.  FHE_TUNE_FAULT_SITES: a mask of the sites below.
 * FHE_TUNE_FAULT_AFTER = k > 0: the k-th crossing of an enabled site from now on fails the call it is in with
 * FHE_ERR_HIP and the message "injected fault at <site>", and disarms; 0: off.  *previous of FHE_TUNE_FAULT_AFTER
 * is the number of crossings of enabled sites since the key was last set, so a clean run with k = 0 gives the
 * count to sweep.  A crossing that fires only throws on the host: no HIP call, synchronisation or launch argument
 * is skipped, replaced or altered.  One integer test per level or per call, none per bootstrap. */
#define FHE_TUNE_FAULT_SITES 7
#define FHE_TUNE_FAULT_AFTER 8
#define FHE_FAULT_LEVEL 1      /* before each level of a flush is launched (a simulated context: scheduled) */
#define FHE_FAULT_STAGE 2      /* before a flush stages its level descriptors (device contexts) */
#define FHE_FAULT_WORKSPACE 4  /* before a flush sizes the bootstrap workspace (device contexts) */
#define FHE_FAULT_DEFERRED 8   /* first statement of a deferred upload (the signer's e and k), before its data is taken */
#define FHE_FAULT_RECORD 16    /* the entry of the engine's recording call: an op fails before it records */
#define FHE_FAULT_CLIENT 32    /* resident client key: an encryption before it stages anything, a decryption after its flush and before its launch */
int fhe_host_set_tuning(int key, int64_t value, int64_t* previous);
int fhe_host_biguint_mul_stats(size_t la, size_t lb, size_t lk, int mode, uint64_t* pbs, uint64_t* levels,
                               uint32_t* level_sizes, size_t cap);
/* Dry run of one radix op on two encrypted `bits`-wide operands: bootstraps, launch levels and level
 * sizes as the engine schedules them (nothing launched). */
#define FHE_HOST_OP_DIVREM 0     /* a / b and a % b, encrypted divisor */
#define FHE_HOST_OP_MUL 1
#define FHE_HOST_OP_ADD 2
#define FHE_HOST_OP_SUB 3
#define FHE_HOST_OP_SHR 4        /* encrypted shift amount */
#define FHE_HOST_OP_LT 5
#define FHE_HOST_OP_DIV_SCALAR 6 /* a / 0xC0FFEE01 */
#define FHE_HOST_OP_SHL 7        /* encrypted shift amount */
#define FHE_HOST_OP_MUL_FULL 8   /* a * b, 2 * bits wide */
#define FHE_HOST_OP_AND 9
#define FHE_HOST_OP_MIN 10
#define FHE_HOST_OP_SCALAR_MAC_COLUMNS 11 /* a * b + b, b public, in column form (sim only) */
#define FHE_HOST_OP_DIVREM_CLEAR 12       /* a / b and a % b, b public (sim only) */
#define FHE_HOST_OP_DIVREM_CLEAR_MIXED 13 /* the same with a's odd blocks trivial (sim only) */
int fhe_host_radix_stats(int op, uint32_t bits, uint64_t* pbs, uint64_t* levels, uint32_t* level_sizes, size_t cap);
/* Simulated runs (no GPU, no key): operands are "encrypted" blocks whose plaintext the engine shadows
 * on the host, so every encrypted code path runs (no trivial folding) while each bootstrap is
 * evaluated from its lookup table and range-checked.  The BigUintFHE mul / mul-add (limbs LSB first,
 * as fhe_host_biguint_mul) and one radix op on `bits`-wide operands (words LSB first; out: the result,
 * 2 * bits wide for MUL_FULL, the bit for LT; out2: DIVREM's remainder).  pbs / levels optional. */
int fhe_host_sim_biguint_mul(const uint32_t* a, size_t la, const uint32_t* b, size_t lb, const uint32_t* k, size_t lk,
                             int mode, uint32_t* out, size_t cap, size_t* n, uint64_t* pbs, uint64_t* levels);
int fhe_host_sim_radix(int op, uint32_t bits, const uint64_t* a, const uint64_t* b, uint64_t* out, uint64_t* out2,
                       uint64_t* pbs, uint64_t* levels);
int fhe_host_sim_biguint_mul_add_columns(const uint32_t* a, size_t la, const uint32_t* b, size_t lb, const uint32_t* k,
                                         size_t lk, int mode, uint64_t* words, size_t nwords, uint32_t* bits,
                                         uint64_t* pbs, uint64_t* levels);
/* The compat chain's g = 15 - [K mod 2^32 >= 2^32 - 16] (K mod 16) (csrc/compat_chain.cpp) on simulated
 * prefix columns: vals holds nprefix records of 31 block values (each <= 3): column 0's block, then
 * the two blocks of each column 1..15; K = sum_m (column m's sum) 4^m.  g: nprefix outputs. */
int fhe_host_sim_chain_g(const uint8_t* vals, size_t nprefix, uint32_t* g, uint64_t* pbs, uint64_t* levels);
/* A simulated context (test hook): no device, no stream, the default parameters, a simulating engine.  The radix
 * and BigUintFHE entry points run on it through their real code: fhe_radix_encrypt / fhe_biguint_encrypt make
 * shadowed blocks of the plaintext (the client key is ignored and may be NULL), fhe_radix_trivial, _clone, _cast,
 * every binary, unary and scalar op (the _words forms included), the BigUintFHE add / mul / mul_add and column
 * forms, the pseudo-Mersenne reductions, and the decryptions, which make the flush a device decryption makes
 * (nothing is launched, the graph is scheduled) and read the shadow.  fhe_ctx_stats, fhe_ctx_level_log and
 * fhe_ctx_noise_audit report on it.  Everything that needs device memory or a real key -- export and serialize,
 * digest and re-randomize, compress and every expand, random, broadcast, the raw pbs / keyswitch / pbs_lincomb,
 * every fhe_set_*_key, the signer -- returns FHE_ERR_INVALID with a message that names the simulated context, and
 * leaves it usable.  fhe_ctx_destroy frees it.
 * The shadow evaluates a bootstrap when it is recorded, so a decryption on this context sees every recorded graph
 * and every value; what is launched afterwards, and in which order, is seen through the launch trace
 * (fhe_ctx_trace), which tests/test_launch_replay.py replays in plaintext on this context and
 * tests/test_launch_replay_gpu.py word for word on a device. */
int fhe_host_sim_ctx_create(fhe_ctx** ctx);
/* Pseudo-Mersenne reduction x mod (2^k_bits - c) (fhe_radix_rem_pseudo_mersenne below) without a GPU or a key.
 * Simulated run on a `bits`-wide operand x (words LSB first): out gets the k_bits-wide result (nout >=
 * ceil(k_bits / 64) words); pbs, levels, folds optional.  Refusals (odd k, c = 0, c >= 2^(k-2), bits above
 * FHE_RADIX_MAX_BITS) return FHE_ERR_INVALID with a message, as the device entry points do. */
int fhe_host_sim_rem_pseudo_mersenne(uint32_t bits, const uint64_t* x, uint32_t k_bits, const uint64_t* c_words, size_t nc,
                                     uint64_t* out, size_t nout, uint64_t* pbs, uint64_t* levels, uint32_t* folds);
/* Dry run of the same on an encrypted `bits`-wide operand: bootstraps, launch levels, level sizes (up to cap),
 * the number of folds (fixed by bits, k and c) and the recording-order fingerprint (optional). */
int fhe_host_rem_pseudo_mersenne_stats(uint32_t bits, uint32_t k_bits, const uint64_t* c_words, size_t nc, uint64_t* pbs,
                                       uint64_t* levels, uint32_t* level_sizes, size_t cap, uint32_t* folds,
                                       uint64_t* fingerprint);
/* The reduced signer's FHE block (k + a * b) mod (2^k_bits - c) on limbs (LSB first), simulated (sim != 0) or
 * dry (sim == 0: encrypted limbs' values are not read, only their counts matter; public a and k are read
 * in both, their digits shape the graph).
 *   mode FHE_BIGUINT_COMPAT / FHE_BIGUINT_FAST: a, b, k encrypted; fhe_biguint_mul_add_columns, then the
 *     column-form reduction.  cols_out (optional, ncols words) gets the value of the column form -- what the
 *     unreduced signer decrypts, the compat product's lost carries included -- and *col_bits its width:
 *     out == cols_out mod n.
 *   mode FHE_SIGN_PUBLIC_OPERANDS: a and k public, b encrypted; the product reduced as it is formed (what
 *     fhe_schnorr_eval_s_public records).
 *   mode FHE_SIGN_PUBLIC_OPERANDS | FHE_HOST_MUL_THEN_FOLD: the same through the unreduced public signer's
 *     column form and the column-form reduction (the alternative the former is measured against).
 * out: k_bits-wide result (sim only); pbs, levels, level_sizes, folds, fingerprint optional. */
#define FHE_HOST_MUL_THEN_FOLD 0x800
int fhe_host_biguint_mul_add_rem(int sim, const uint32_t* a, size_t la, const uint32_t* b, size_t lb, const uint32_t* k,
                                 size_t lk, int mode, uint32_t k_bits, const uint64_t* c_words, size_t nc, uint64_t* out,
                                 size_t nout, uint64_t* cols_out, size_t ncols, uint32_t* col_bits, uint64_t* pbs,
                                 uint64_t* levels, uint32_t* level_sizes, size_t cap, uint32_t* folds,
                                 uint64_t* fingerprint);

/* ------------------------------------------------------------------- BigUintFHE */
/* struct BigUintFHE { digits: Vec<FheUint32> } (src/biguint.rs:8-13), device-resident. */
#define FHE_BIGUINT_COMPAT 0 /* exact reference limb loop incl. src/biguint.rs:247-249 wrap */
#define FHE_BIGUINT_FAST 1   /* true sum/product, one wide carry propagation */
/* BigUintFHE::new (src/biguint.rs:17-31): limbs = value.to_u32_digits() (LSB first, no
 * leading zeros; nlimbs 0 encodes zero as an empty vector) */
int fhe_biguint_encrypt(fhe_ctx* ctx, fhe_client_key* ck, const uint32_t* limbs, size_t nlimbs,
                        fhe_biguint** out);
/* BigUintFHE::from_encrypted_digits (src/biguint.rs:46-48) */
int fhe_biguint_from_digits(const fhe_radix* const* digits, size_t n, fhe_biguint** out);
/* to_biguint (src/biguint.rs:61-76): decrypted limbs; *nlimbs = digit count */
int fhe_biguint_decrypt(fhe_ctx* ctx, const fhe_client_key* ck, const fhe_biguint* x, uint32_t* limbs,
                        size_t cap, size_t* nlimbs);
int fhe_biguint_len(const fhe_biguint* x, size_t* nlimbs);
int fhe_biguint_digit(const fhe_biguint* x, size_t i, fhe_radix** out);
/* the limbs' blocks as one FheUint<num_bits> (no bootstrap: blocks are concatenated, then
 * zero-extended or truncated), e.g. to run wide radix ops on a BigUintFHE value */
int fhe_biguint_to_radix(const fhe_biguint* x, uint32_t num_bits, fhe_radix** out);
int fhe_biguint_clone(const fhe_biguint* x, fhe_biguint** out);
void fhe_biguint_destroy(fhe_biguint* x);
/* impl Add / impl Mul for BigUintFHE (src/biguint.rs:120-265); inputs are not consumed */
int fhe_biguint_add(fhe_ctx* ctx, const fhe_biguint* a, const fhe_biguint* b, int mode, fhe_biguint** out);
int fhe_biguint_mul(fhe_ctx* ctx, const fhe_biguint* a, const fhe_biguint* b, int mode, fhe_biguint** out);
/* k + a * b with the limbs of fhe_biguint_add(k, fhe_biguint_mul(a, b)) -- the FHE block of
 * sign_fhe_with_k0 (src/schnorr.rs:274) in one schedule: no level spent on the add when the product
 * is exact (fast mode or a one-limb factor), one fewer otherwise */
int fhe_biguint_mul_add(fhe_ctx* ctx, const fhe_biguint* a, const fhe_biguint* b, const fhe_biguint* k, int mode,
                        fhe_biguint** out);
/* k + a * b (the limbs' value of fhe_biguint_mul_add) left in column form for decryption: the same
 * FHE work without the final carry propagation; fhe_columns_decrypt resolves the carries on the host
 * (as tfhe-rs's decrypt_radix does for blocks holding carries) and returns the value mod 2^bits. */
typedef struct fhe_columns fhe_columns;
int fhe_biguint_mul_add_columns(fhe_ctx* ctx, const fhe_biguint* a, const fhe_biguint* b, const fhe_biguint* k, int mode,
                                fhe_columns** out);
/* m * a + k (m, k public words) in column form, value mod 2^(a's bits) */
int fhe_radix_scalar_mul_add_columns(fhe_ctx* ctx, const fhe_radix* a, const uint64_t* m, size_t nm, const uint64_t* k,
                                     size_t nk, fhe_columns** out);
/* fhe_radix_rem_pseudo_mersenne on a column form: the folds are linear,
 * so the first one reads the columns unpropagated -- only the part above 2^k_bits is normalized, on its own. */
int fhe_columns_rem_pseudo_mersenne(fhe_ctx* ctx, const fhe_columns* x, uint32_t k_bits, const uint64_t* c_words,
                                    size_t nc, fhe_radix** out);
int fhe_columns_bits(const fhe_columns* x, uint32_t* bits);
int fhe_columns_decrypt(fhe_ctx* ctx, const fhe_client_key* ck, const fhe_columns* x, uint64_t* words, size_t nwords);
void fhe_columns_destroy(fhe_columns* x);
/* serialization of the limb vector (format of fhe_radix_serialize; every limb is a 32-bit radix) */
int fhe_biguint_serialize(fhe_ctx* ctx, const fhe_biguint* x, uint8_t* buf, size_t cap, size_t* len);
int fhe_biguint_deserialize(fhe_ctx* ctx, const uint8_t* buf, size_t len, fhe_biguint** out);

/* ------------------------------------------------- seeded (compressed) ciphertexts */
/* A fresh ciphertext is 2049 words per block, of which the 2048 mask words are uniformly random and
 * carry no information: a 256-bit value is 128 x 16,392 B = 2.1 MB.  The seeded form keeps a PUBLIC
 * 32-byte mask seed and one body word per block (about 1.1 KB for 256 bits); whoever holds it
 * regenerates the masks.  tfhe-rs' CompressedFheUint32::try_encrypt(..) / .decompress().  The handle
 * lives on the host and needs no context; the parameter set travels with it.
 *   masks   block i's 2048 mask words = u64 words [2048 i, 2048 (i + 1)) of the ChaCha20 stream whose key
 *           is the 32 seed bytes (little-endian words) and whose nonce is {101, "ROCM", 0} (the key
 *           streams' layout, block counter 256 i); it shares nothing with the client key's streams
 *   bodies  body_i = <mask_i, big key> + delta m_i + e_i, e_i drawn from the next 64-bit word of the client
 *           key's encryption stream: one word per block, so a serialized client key continues correctly
 * THE SEED IS PUBLIC AND MUST NEVER BE USED FOR TWO OBJECTS UNDER ONE CLIENT KEY: equal masks make the
 * difference of two bodies delta (m - m') + e - e', which leaks the difference of the messages.  Pass
 * mask_seed = NULL (32 bytes from getrandom()) outside tests.  An object holds at most 2^24 blocks
 * (the stream's 32-bit block counter); more is FHE_ERR_INVALID. */
typedef struct fhe_seeded fhe_seeded;
#define FHE_SEEDED_RADIX 0
#define FHE_SEEDED_BIGUINT 1
/* CompressedFheUint::try_encrypt: words little-endian, num_bits as fhe_radix_encrypt */
int fhe_radix_encrypt_seeded(fhe_client_key* ck, const uint64_t* words, uint32_t num_bits,
                             const uint8_t mask_seed[32] /* NULL: OS entropy */, fhe_seeded** out);
/* the same for BigUintFHE::new (limbs as fhe_biguint_encrypt; nlimbs 0 is the empty vector, 0 blocks) */
int fhe_biguint_encrypt_seeded(fhe_client_key* ck, const uint32_t* limbs, size_t nlimbs,
                               const uint8_t mask_seed[32] /* NULL: OS entropy */, fhe_seeded** out);
/* form (FHE_SEEDED_*), count (num_bits or nlimbs) and blocks; any output may be NULL */
int fhe_seeded_info(const fhe_seeded* x, uint32_t* form, uint32_t* count, size_t* nblocks);
/* Wire format (kind 5 of the keys' framed, checksummed format; size-query convention as above):
 * params, u32 form, u32 count, 32 seed bytes, nblocks u64 bodies -- 108 + 8 nblocks bytes.  The
 * reader checks magic, version, kind, length, checksum, parameter ranges, the form, num_bits (even,
 * <= FHE_RADIX_MAX_BITS) and that the block count matches the payload length and is <= 2^24, all
 * before it allocates.  tfhe-rs' wire format of compressed types is not reproduced (parity unpinned). */
int fhe_seeded_serialize(const fhe_seeded* x, uint8_t* buf, size_t cap, size_t* len);
int fhe_seeded_deserialize(const uint8_t* buf, size_t len, fhe_seeded** out);
/* CompressedFheUint::decompress on the host: cts = nblocks x 2049 words (masks regenerated, body
 * appended), nwords >= that.  The word-for-word definition of the GPU expansion, and what a client
 * without a GPU uses. */
int fhe_seeded_expand_host(const fhe_seeded* x, uint64_t* cts, size_t nwords);
/* CompressedFheUint::decompress on the GPU of ctx: fresh block slots whose masks a gfx950 kernel
 * regenerates (only seed and bodies cross the bus), stream-ordered like fhe_radix_encrypt's upload.
 * FHE_ERR_NO_KEY without an installed server key; FHE_ERR_INVALID for the other form, and for parameters
 * that differ from the installed key's (the message names the field), before anything is launched.  No
 * collective is issued: under the multi-GPU fan-out every rank must expand the same bytes. */
int fhe_seeded_expand_radix(fhe_ctx* ctx, const fhe_seeded* x, fhe_radix** out);
int fhe_seeded_expand_biguint(fhe_ctx* ctx, const fhe_seeded* x, fhe_biguint** out);
void fhe_seeded_destroy(fhe_seeded* x);

/* ------------------------------------------------- seeded (compressed) server key */
/* The server key is the largest object a client sends: 123,060,224 bytes at the default parameters, of
 * which n of every n + 1 KSK words and every second BSK polynomial are public random masks.  The seeded
 * key keeps a PUBLIC 32-byte seed and the bodies: 27,410,532 bytes (4.5x smaller; multi-bit 41.1 MB
 * against 150.4 MB).  tfhe-rs' CompressedServerKey::new(&client_key) / .decompress() /
 * .decompress_to_gpu().  The handle lives on the host and needs no context.
 *   masks   ChaCha20 keyed by the 32 seed bytes (little-endian words), nonce {id, "ROCM", 0}; every row
 *           starts on a stride of 256 ChaCha blocks (2048 u64 words):
 *           KSK (id 102) row r = j ks_level + l: mask word t < n = u64 word 2048 r + t;
 *           BSK (id 103) GGSW q, row rho in {0, 1}: mask coefficient m = u64 word 2048 (2 q + rho) + m
 *   noise   2048 ks_level + ggsw 2 2048 words of the client key's encryption stream, the KSK rows' first,
 *           then the BSK's in (q, rho, m) order, whatever the number of host threads: a serialized
 *           client key continues correctly afterwards
 *   bodies  KSK: <mask, s> + (S_j << (64 - ks_base_log (l + 1))) + e.  BSK, with g = 1 << (64 -
 *           pbs_base_log) and m_q the GGSW's message: B = A * S + e, then row 1: B[0] += g m_q, row 0:
 *           B[t] -= g m_q S_t for every t.  (fhe_generate_keys puts row 0's gadget into the mask, A[0] += g;
 *           a mask that is regenerated from a seed cannot hold it.  The phase B - A * S = e - g m_q S is
 *           the same, so the expanded key is consumed by every kernel unchanged -- but its words differ
 *           from fhe_generate_keys' for the same client key.)
 * THE SEED IS PUBLIC.  ONE SEED, ONE OBJECT: never reuse a seed for a second server key, or for a seeded
 * ciphertext, under the same client key (the stream ids differ from the ciphertexts' 101, so a reuse is
 * not the catastrophic case of equal ciphertext masks; the rule stands all the same).  Pass mask_seed =
 * NULL (32 bytes from getrandom()) outside tests. */
typedef struct fhe_seeded_server_key fhe_seeded_server_key;
int fhe_server_key_generate_seeded(fhe_client_key* ck, const uint8_t mask_seed[32] /* NULL: OS entropy */,
                                   fhe_seeded_server_key** out);
int fhe_seeded_server_key_params(const fhe_seeded_server_key* ssk, fhe_params* out);
/* Wire format (kind 6 of the keys' framed, checksummed format; size-query convention as above): params,
 * 32 seed bytes, KSK bodies, BSK bodies -- 100 + 8 (2048 ks_level + 4096 ggsw) bytes.  The reader checks
 * magic, version, kind, checksum, parameter ranges and that the payload length is exactly that of the
 * parsed parameters, all before it allocates.  A full key's bytes (kind 2) are refused here, and these
 * by fhe_server_key_deserialize.  tfhe-rs' wire format is not reproduced (parity unpinned). */
int fhe_seeded_server_key_serialize(const fhe_seeded_server_key* ssk, uint8_t* buf, size_t cap, size_t* len);
int fhe_seeded_server_key_deserialize(const uint8_t* buf, size_t len, fhe_seeded_server_key** ssk);
/* CompressedServerKey::decompress on the host: an ordinary server key (masks regenerated, bodies in
 * place; serializes with fhe_server_key_serialize).  The word-for-word definition of the GPU install,
 * and what a server without this engine's GPU path uses. */
int fhe_seeded_server_key_expand_host(const fhe_seeded_server_key* ssk, fhe_server_key** out);
/* CompressedServerKey::decompress_to_gpu: leaves ctx in exactly the device state of
 * fhe_set_server_key(ctx, expand_host(ssk)) -- KSK, byte planes, both Fourier BSK layouts, adopted
 * parameters, LUT ids surviving a re-key, engine -- but uploads only the bodies: gfx950 kernels
 * regenerate the KSK masks in place and the BSK mask polynomials inside the Fourier conversion, so the
 * standard-domain BSK never exists on the device.  No secret is needed and no collective is issued:
 * under the fan-out every rank may install the same bytes, or a root installed this way may
 * fhe_ctx_broadcast_server_key.  Errors as fhe_set_server_key: FHE_ERR_INVALID for a NULL argument
 * (context untouched), FHE_ERR_UNSUPPORTED for parameters the kernels do not take (context untouched),
 * FHE_ERR_HIP for a device failure -- then the previous key is already released and the context has
 * no key (FHE_ERR_NO_KEY from its operations) until a later install succeeds. */
int fhe_set_server_key_seeded(fhe_ctx* ctx, const fhe_seeded_server_key* ssk);
void fhe_seeded_server_key_destroy(fhe_seeded_server_key* ssk);

/* ------------------------------------------------- compressed computed ciphertexts */
/* Anything the server COMPUTES leaves the GPU as big-key LWE blocks of 2049 words: a 256-bit value is
 * 2.1 MB through fhe_radix_serialize.  tfhe-rs' CompressedCiphertextList: the blocks are packed into GLWEs
 * by a packing keyswitch under a dedicated compression key, every coefficient is modulus-switched to 12
 * bits, and a bootstrap under a decompression key restores usable blocks.  A 256-bit value becomes
 * 12 (1024 + 128) bits = 1,728 payload bytes + 128 degree bytes + the header.
 *
 * Parameters: tfhe-rs' COMP_PARAM_MESSAGE_2_CARRY_2_KS_PBS_TUNIFORM_2M64 AS RECALLED (no tfhe-rs source
 * is at hand to pin them).  The decompression bootstrap uses the main set's pbs_base_log x 1 level
 * (2^23 x 1) and glwe_noise_log2.  Accepted: polynomial_size a power of two in [8, 2048]; 1 <=
 * glwe_dimension <= 8 with glwe_dimension * polynomial_size <= 2048; 1 <= lwe_per_glwe <= polynomial_size;
 * pks_base_log * pks_level <= 32, 1 <= pks_base_log <= 7 (digits fit a signed byte);
 * storage_log_modulus exactly 12 = log2(2 * 2048), so the decompression bootstrap's own modulus switch of
 * a stored value is the identity.  Anything else: FHE_ERR_UNSUPPORTED with a named reason. */
typedef struct fhe_compression_params {
    uint32_t glwe_dimension;      /* k' (4) */
    uint32_t polynomial_size;     /* N' (256) */
    uint32_t lwe_per_glwe;        /* L  (256) */
    uint32_t pks_base_log;        /* 4 */
    uint32_t pks_level;           /* 4 */
    uint32_t pks_noise_log2;      /* TUniform bound of the packing key (42) */
    uint32_t storage_log_modulus; /* 12 */
} fhe_compression_params;
int fhe_compression_params_default(fhe_compression_params* out);
/* CompressionPrivateKeys (client): k' N' binary words s', independent of the GLWE key. */
typedef struct fhe_compression_private_key fhe_compression_private_key;
/* CompressionKey + DecompressionKey (server):
 *   packing KSK  u64[2048][pks_level][k' + 1][N']: row (j, l) is a GLWE encryption under s' of the constant
 *                polynomial S_j << (64 - pks_base_log (l + 1)), S the big key: masks A_c uniform,
 *                B = sum_c A_c * s'_c + e + const, e per coefficient from TUniform(2^pks_noise_log2)
 *   decompression BSK  a CLASSIC (grouping 1) bootstrapping key of LWE dimension k' N' encrypting the
 *                bits of s' (flat, polynomial-major) under the big GLWE key, in fhe_generate_keys' word
 *                layout and gadget form -- classic even when the main key is multi-bit.
 * 150,994,944 payload bytes at the defaults; its seeded form (fhe_seeded_compression_key below) is 3.0x
 * smaller on the wire. */
typedef struct fhe_compression_key fhe_compression_key;
/* Draws everything from ck's encryption stream, in this order and before any threaded pass: k' N' secret
 * words (bit 0 of each), the packing KSK's rows in order (k' N' mask words, then N' noise words, per row),
 * the BSK's (q, rho) rows in order (2048 mask words, then 2048 noise words):
 *   k' N' + 2048 pks_level (k' + 1) N' + 8192 k' N' stream words (u64)
 * whatever the number of host threads, so a serialized client key continues right after them.
 * params = NULL: the defaults. */
int fhe_compression_keys_generate(fhe_client_key* ck, const fhe_compression_params* params,
                                  fhe_compression_private_key** priv, fhe_compression_key** key);
int fhe_compression_key_params(const fhe_compression_key* key, fhe_params* main, fhe_compression_params* comp);
int fhe_compression_private_key_params(const fhe_compression_private_key* priv, fhe_params* main,
                                       fhe_compression_params* comp);
/* raw key material (tests): sizes in u64 words; either buffer may be NULL with length 0 */
int fhe_compression_key_export(const fhe_compression_key* key, uint64_t* pksk, size_t pksk_len, uint64_t* bsk,
                               size_t bsk_len);
int fhe_compression_private_key_export(const fhe_compression_private_key* priv, uint64_t* sk, size_t len);
void fhe_compression_private_key_destroy(fhe_compression_private_key* priv);
void fhe_compression_key_destroy(fhe_compression_key* key);
/* Wire formats: kinds 7 (private key), 8 (compression key), 9 (compressed list) of the keys' framed,
 * checksummed format; size-query convention as above.  Every reader checks the parameter ranges and the
 * exact payload length of the parsed parameters before it allocates, and refuses every other kind.
 * tfhe-rs' wire format is not reproduced (parity unpinned). */
int fhe_compression_private_key_serialize(const fhe_compression_private_key* priv, uint8_t* buf, size_t cap,
                                          size_t* len);
int fhe_compression_private_key_deserialize(const uint8_t* buf, size_t len, fhe_compression_private_key** priv);
int fhe_compression_key_serialize(const fhe_compression_key* key, uint8_t* buf, size_t cap, size_t* len);
int fhe_compression_key_deserialize(const uint8_t* buf, size_t len, fhe_compression_key** key);

/* CompressedCiphertextList holding ONE value.  Host object, needs no context.  Wire (kind 9): main params,
 * compression params (7 x u32), u32 form (FHE_SEEDED_RADIX / FHE_SEEDED_BIGUINT semantics), u32 count
 * (num_bits or nlimbs), u32 B (blocks), B degree bytes (each < mc of the main params), then per GLWE g = 0.. in order its
 * 12-bit values packed little-endian bit-contiguously (value i at bits [12 i, 12 i + 12)): k' N' mask
 * values, polynomial-major, then b_g = min(L, B - g L) bodies; every GLWE starts on a byte boundary:
 *   32 + 36 + 28 + 12 + B + sum_g ceil(12 (k' N' + b_g) / 8)  bytes. */
typedef struct fhe_compressed_list fhe_compressed_list;
/* The packing keyswitch on the host -- the word-for-word definition of the GPU path, and what a server
 * without a GPU uses: cts = nblocks x 2049 words, degrees = nblocks bytes (< mc of the key), form / count as above
 * (count / 2, or 16 count, must equal nblocks). */
int fhe_compress_host(const fhe_compression_key* key, const uint64_t* cts, size_t nblocks, const uint8_t* degrees,
                      uint32_t form, uint32_t count, fhe_compressed_list** out);
int fhe_compressed_info(const fhe_compressed_list* x, uint32_t* form, uint32_t* count, size_t* nblocks);
/* the parameter sets that travel with the list; either output may be NULL */
int fhe_compressed_params(const fhe_compressed_list* x, fhe_params* main, fhe_compression_params* comp);
int fhe_compressed_serialize(const fhe_compressed_list* x, uint8_t* buf, size_t cap, size_t* len);
int fhe_compressed_deserialize(const uint8_t* buf, size_t len, fhe_compressed_list** out);
void fhe_compressed_destroy(fhe_compressed_list* x);
/* Client side, no GPU and no context: per block, phase = body_t - sum_c (A_c * s'_c)[t] mod 2^12, value =
 * round(phase / 2^7) mod 16; assembled as fhe_radix_decrypt does (blocks above degree 3 carry into their
 * neighbours), mod 2^bits.  nwords >= ceil(bits / 64), bits = num_bits or 32 nlimbs. */
int fhe_compressed_decrypt(const fhe_compression_private_key* priv, const fhe_compressed_list* x, uint64_t* words,
                           size_t nwords);
/* Installs the key for fhe_*_compress / fhe_compressed_expand_* of this context: after fhe_set_server_key,
 * and dropped by the next server-key install (then FHE_ERR_NO_KEY from those calls).  FHE_ERR_INVALID, with
 * the differing field named, if the key's main parameters are not the installed server key's. */
int fhe_set_compression_key(fhe_ctx* ctx, const fhe_compression_key* key);
/* CompressedCiphertextListBuilder::push(x).build(): flushes what x depends on (no collective: rank-local
 * under a communicator), then three gfx950 kernels -- digits, int8 matrix-core contraction against the
 * packing key's byte planes, rotate / modulus switch / pack -- and one download.  Byte-identical to
 * fhe_compress_host on the exported blocks. */
int fhe_radix_compress(fhe_ctx* ctx, const fhe_radix* x, fhe_compressed_list** out);
int fhe_biguint_compress(fhe_ctx* ctx, const fhe_biguint* x, fhe_compressed_list** out);
/* CompressedCiphertextList::get: fresh block slots (noise 1, degree from the degree byte), stream-ordered
 * like fhe_seeded_expand_radix: one unpack + sample-extract kernel, then the existing blind rotate under the
 * decompression key with the identity table. */
int fhe_compressed_expand_radix(fhe_ctx* ctx, const fhe_compressed_list* x, fhe_radix** out);
int fhe_compressed_expand_biguint(fhe_ctx* ctx, const fhe_compressed_list* x, fhe_biguint** out);
/* Test hook: the unpack + sample-extract kernel alone.  rows = nblocks x (k' N' + 1) words (each stored value
 * << 52), host pointer; synchronous. */
int fhe_compressed_extract_rows(fhe_ctx* ctx, const fhe_compressed_list* x, uint64_t* rows, size_t nwords);
/* Test hook: the packing keyswitch's contraction alone, launched as fhe_radix_compress launches it (the same
 * choice of kernel by count).  cts = count rows of 2049 words, any words; P = count x (k' + 1) N' words, row i
 * = sum_{j, l} d[i, j, l] PKSK[j][l] mod 2^64, before the rotation, the bodies and the rounding to 12 bits
 * (p_words = the buffer's size in words); body = the count body words set aside.  Host pointers; flushes and
 * waits like a download.  FHE_ERR_NO_KEY without a compression key; FHE_ERR_INVALID for a NULL pointer with
 * count > 0, p_words too small, or more than 2^24 rows; count = 0 does nothing. */
int fhe_pack_keyswitch_words(fhe_ctx* ctx, const uint64_t* cts, size_t count, uint64_t* P, size_t p_words,
                             uint64_t* body);

/* ------------------------------------------------- seeded (compressed) compression key */
/* The compression key is the largest object left for a client to send: 150,994,944 payload bytes at the
 * defaults (packing KSK 83,886,080 + decompression BSK 67,108,864), of which k' of every k' + 1 packing-key
 * polynomials and every second BSK polynomial are public random masks.  The seeded key keeps a PUBLIC
 * 32-byte seed and the bodies: 50,331,776 bytes serialized (3.0x smaller).  tfhe-rs' CompressedCompressionKey
 * / CompressedDecompressionKey.  The handle lives on the host and needs no context.
 *   masks   ChaCha20 keyed by the 32 seed bytes (little-endian words), nonce {id, "ROCM", 0}; every row
 *           starts on a stride of 256 ChaCha blocks (2048 u64 words; k' N' <= 2048):
 *           packing KSK (id 107) row r = j pks_level + l: coefficient m of mask polynomial c < k' = u64 word
 *           2048 r + c N' + m;
 *           BSK (id 108) GGSW q < k' N', row rho in {0, 1}: mask coefficient m = u64 word 2048 (2 q + rho) + m
 *   noise   everything from the client key's encryption stream, before any threaded pass: k' N' secret words
 *           (bit 0 of each -- the s' fhe_compression_keys_generate draws from the same stream state), then N'
 *           noise words per packing-key row in row order, then 2048 noise words per BSK row in (q, rho) order:
 *             k' N' + 2048 pks_level N' + 4096 k' N'  stream words (u64), 6,292,480 at the defaults,
 *           whatever the number of host threads: a serialized client key continues correctly afterwards
 *   bodies  packing KSK: B = sum_c A_c * s'_c + e, e from TUniform(2^pks_noise_log2), then B[0] += S_j <<
 *           (64 - pks_base_log (l + 1)).  BSK, with g = 1 << (64 - pbs_base_log) and message s'_q (classic,
 *           whatever the main grouping): B = A * S + e, e from TUniform(2^glwe_noise_log2), then row 1:
 *           B[0] += g s'_q, row 0: B[t] -= g s'_q S_t for every t.  (fhe_compression_keys_generate puts row 0's
 *           gadget into the mask; a mask that is regenerated from a seed cannot hold it.  The phases are the
 *           same, so the expanded key is consumed by every kernel unchanged -- but its words differ from
 *           fhe_compression_keys_generate's for the same secrets.)
 * THE SEED IS PUBLIC.  ONE SEED, ONE OBJECT: never reuse a seed for a second compression key, a server key
 * or a seeded ciphertext under the same client key (the stream ids differ from 101 / 102 / 103, so a reuse
 * is not the catastrophic case of equal masks; the rule stands all the same).  Pass mask_seed = NULL
 * (32 bytes from getrandom()) outside tests. */
typedef struct fhe_seeded_compression_key fhe_seeded_compression_key;
int fhe_compression_keys_generate_seeded(fhe_client_key* ck, const fhe_compression_params* params /* NULL: defaults */,
                                         const uint8_t mask_seed[32] /* NULL: OS entropy */,
                                         fhe_compression_private_key** priv, fhe_seeded_compression_key** sck);
/* either output may be NULL */
int fhe_seeded_compression_key_params(const fhe_seeded_compression_key* sck, fhe_params* main,
                                      fhe_compression_params* comp);
/* Wire format (kind 12 of the keys' framed, checksummed format; size-query convention as above): main params,
 * compression params (7 x u32), 32 seed bytes, packing-key bodies u64[2048][pks_level][N'], BSK bodies
 * u64[k' N'][2][2048] -- 128 + 8 (2048 pks_level N' + 4096 k' N') bytes.  The reader checks magic, version,
 * kind, checksum, both parameter ranges and that the payload length is exactly that of the parsed parameters,
 * all before it allocates.  A full key's bytes (kind 8) are refused here, and these by
 * fhe_compression_key_deserialize.  tfhe-rs' wire format is not reproduced (parity unpinned). */
int fhe_seeded_compression_key_serialize(const fhe_seeded_compression_key* sck, uint8_t* buf, size_t cap,
                                         size_t* len);
int fhe_seeded_compression_key_deserialize(const uint8_t* buf, size_t len, fhe_seeded_compression_key** sck);
/* decompress on the host: an ordinary compression key (masks regenerated, bodies in place; serializes as
 * kind 8, installs through fhe_set_compression_key).  The word-for-word definition of the GPU install. */
int fhe_seeded_compression_key_expand_host(const fhe_seeded_compression_key* sck, fhe_compression_key** key);
void fhe_seeded_compression_key_destroy(fhe_seeded_compression_key* sck);
/* Leaves ctx in exactly the device state of fhe_set_compression_key(ctx, expand_host(sck)) -- the packing
 * key's byte planes, both Fourier layouts of the decompression BSK, the compression parameters -- but uploads
 * only the bodies: a gfx950 kernel writes the byte planes from seed + bodies (the u64 packing key never
 * exists on the device), and the BSK mask polynomials are generated inside the Fourier conversion.  No
 * secret is needed and no collective is issued.  Errors as fhe_set_compression_key: FHE_ERR_INVALID for a
 * NULL argument, FHE_ERR_NO_KEY without a server key, FHE_ERR_INVALID with the differing field named if the
 * main parameters are not the installed server key's, FHE_ERR_UNSUPPORTED if the body counts do not match
 * the parameters -- all before anything is launched, a previously installed compression key stays in place.
 * FHE_ERR_HIP for a device failure: then the context has no compression key.  Dropped by the next server-key
 * install. */
int fhe_set_compression_key_seeded(fhe_ctx* ctx, const fhe_seeded_compression_key* sck);
/* Test hook: the installed compression key's device state.  planes = the packing key's int8 byte planes
 * [8][ceil((k' + 1) N' / 16)][32 pks_level][64][16], bsk / bsk_e = the decompression BSK's two Fourier layouts,
 * k' N' x 4 x 1024 complex doubles each (sizes in doubles).  Each pair may be NULL / 0.  Waits for the
 * stream.  FHE_ERR_NO_KEY without a compression key. */
int fhe_ctx_export_compression_state(fhe_ctx* ctx, int8_t* planes, size_t planes_bytes, double* bsk,
                                     size_t bsk_doubles, double* bsk_e, size_t bsk_e_doubles);

/* ------------------------------------------------- public-key encryption (compact lists) */
/* Encryption by a party that does not hold the secret key: tfhe-rs' CompactPublicKey::new(&client_key),
 * CompactCiphertextList::builder(&pk).push(..).build_packed() and .expand().  The default parameters encrypt
 * under the big key of dimension k N = 2048, a power of two, so the compact scheme applies as it is (no
 * dedicated parameters, no casting keyswitch).  Polynomials live in Z_2^64[X] / (X^2048 + 1); S is the
 * client's big key as a polynomial (coefficient order = the big LWE key's).
 *   key     a PUBLIC 32-byte mask seed and a body polynomial: A = the first 2048 u64 words of the ChaCha20
 *           stream whose key is the seed and whose nonce is {104, "ROCM", 0}; B = A S + E, E_j from the j-th of
 *           the next 2048 words of the client key's encryption stream (tuniform at glwe_noise_log2): the key
 *           advances by exactly 2048 words, so a serialized client key continues correctly.  16,484 bytes.
 *   list    nvalues values, each a radix of num_bits or a BigUintFHE of nlimbs x 16 blocks.  A value's 2-bit
 *           blocks become coefficients in order: one block per coefficient (build), or m_2i + 4 m_(2i+1)
 *           (build_packed: an odd last block stands alone, every value starts on a fresh coefficient).
 *           Coefficients fill chunks of 2048.  Chunk c takes, from ChaCha20 streams keyed by the ENCRYPTION
 *           SEED: R (bit i = bit i & 63 of u64 word 32 c + (i >> 6), nonce {105, "ROCM", 0}), E1 (2048 words
 *           from u64 word 4096 c, nonce {106, "ROCM", 0}) and E2 (the words after E1, one per used
 *           coefficient), and holds C_A = A R + E1 and C_B[j] = (B R)[j] + E2[j] + delta m_j.  A packed 256-bit
 *           value is 2048 x 8 + 64 x 8 = 16,896 payload bytes, against 2.1 MB in the full form.
 *   expand  coefficient t of a chunk is the big LWE with mask word u = C_A[t - u] (u <= t), -C_A[t - u + 2048]
 *           (u > t) and body C_B[t]; its phase error E R + E2 - E1 S is below 2^30 in absolute value.
 * THE ENCRYPTION SEED IS SECRET: IT GIVES AWAY R, AND WITH R EVERY MESSAGE OF THE LIST.  IT IS NEVER STORED IN
 * THE LIST AND MUST NEVER BE USED TWICE.  Pass encryption_seed = NULL (32 bytes from getrandom()) outside
 * tests; a given seed is for tests only.  The key's mask seed is public, but one seed serves one key only
 * (mask_seed = NULL: getrandom()).  A list holds at most 2^16 values and 2^24 coefficients.  tfhe-rs' bytes
 * are not reproduced (parity unpinned), zero-knowledge proofs of encryption are out of scope. */
typedef struct fhe_public_key fhe_public_key;
typedef struct fhe_compact_builder fhe_compact_builder;
typedef struct fhe_compact_list fhe_compact_list;
/* CompactPublicKey::new */
int fhe_public_key_generate(fhe_client_key* ck, const uint8_t mask_seed[32] /* NULL: OS entropy */,
                            fhe_public_key** out);
int fhe_public_key_params(const fhe_public_key* pk, fhe_params* params);
/* the seed (32 bytes) and the body polynomial (nwords >= 2048); either output may be NULL */
int fhe_public_key_export(const fhe_public_key* pk, uint8_t seed[32], uint64_t* body, size_t nwords);
/* Wire format (kind 10 of the framed, checksummed format): params, 32 seed bytes, 2048 u64 bodies.  The
 * reader checks magic, version, kind, length, checksum, parameter ranges and the payload length before it
 * allocates. */
int fhe_public_key_serialize(const fhe_public_key* pk, uint8_t* buf, size_t cap, size_t* len);
int fhe_public_key_deserialize(const uint8_t* buf, size_t len, fhe_public_key** out);
void fhe_public_key_destroy(fhe_public_key* pk);
/* CompactCiphertextList::builder(&pk): takes a copy of the key; no client key, no context.  push: words and
 * num_bits as fhe_radix_encrypt, limbs as fhe_biguint_encrypt (nlimbs 0 is the empty vector, no coefficient). */
int fhe_compact_builder_new(const fhe_public_key* pk, fhe_compact_builder** out);
int fhe_compact_builder_push_radix(fhe_compact_builder* b, const uint64_t* words, uint32_t num_bits);
int fhe_compact_builder_push_biguint(fhe_compact_builder* b, const uint32_t* limbs, size_t nlimbs);
/* .build() (packed = 0) / .build_packed() (packed = 1); the builder may build again (use a fresh seed) */
int fhe_compact_builder_build(const fhe_compact_builder* b, int packed,
                              const uint8_t encryption_seed[32] /* SECRET; NULL: OS entropy */, fhe_compact_list** out);
void fhe_compact_builder_destroy(fhe_compact_builder* b);
/* any output may be NULL */
int fhe_compact_list_info(const fhe_compact_list* x, int* packed, uint32_t* nvalues, size_t* ncoef, size_t* nchunks);
/* value `index`: form (FHE_SEEDED_*), count (num_bits or nlimbs), its blocks, first coefficient and coefficients */
int fhe_compact_list_value_info(const fhe_compact_list* x, uint32_t index, uint32_t* form, uint32_t* count,
                                size_t* nblocks, size_t* first_coef, size_t* ncoef);
int fhe_compact_list_params(const fhe_compact_list* x, fhe_params* params);
/* C_A (2048 nchunks words) and C_B (ncoef words); either may be NULL */
int fhe_compact_list_export(const fhe_compact_list* x, uint64_t* ca, size_t ca_words, uint64_t* cb, size_t cb_words);
/* Wire format (kind 11): params, u32 packed, u32 nvalues, per value u32 form + u32 count, C_A, C_B --
 * 76 + 8 nvalues + 8 (2048 nchunks + ncoef) bytes.  The reader checks magic, version, kind, length, checksum,
 * parameter ranges, the flag, every form and count, and that the value table matches the payload length, all
 * before it allocates anything of the list's size. */
int fhe_compact_list_serialize(const fhe_compact_list* x, uint8_t* buf, size_t cap, size_t* len);
int fhe_compact_list_deserialize(const uint8_t* buf, size_t len, fhe_compact_list** out);
void fhe_compact_list_destroy(fhe_compact_list* x);
/* The sample extraction on the host: rows = ncoef x 2049 words.  The word-for-word definition of the GPU
 * kernel's output. */
int fhe_compact_list_expand_host(const fhe_compact_list* x, uint64_t* rows, size_t nwords);
/* Client side, no GPU: value `index` from its coefficients' phases (round, unpack), little-endian words
 * (BigUintFHE: limb i at bits 32 i); nwords >= ceil(bits / 64).  FHE_ERR_INVALID with the field named if the
 * list's parameters differ from the client key's. */
int fhe_compact_list_decrypt(const fhe_client_key* ck, const fhe_compact_list* x, uint32_t index, uint64_t* words,
                             size_t nwords);
/* CompactCiphertextList::expand of value `index` on the GPU of ctx: fresh block slots filled by a gfx950
 * sample-extraction kernel from the staged C_A / C_B (stream-ordered like fhe_seeded_expand_radix: no flush, no
 * collective -- under the multi-GPU fan-out every rank must expand the same bytes).  An unpacked list's
 * extracted blocks are the result (degree 3, noise 1).  A packed list's coefficients (degree 15, noise 1) are
 * split by two lookups each, x & 3 and x >> 2, recorded in the deferred bootstrap graph: one level, shared with
 * whatever else is pending.  FHE_ERR_NO_KEY without an installed server key; FHE_ERR_INVALID for an index out
 * of range, the other form, and parameters that differ from the installed key's (the message names the
 * field), before anything is launched. */
int fhe_compact_list_expand_radix(fhe_ctx* ctx, const fhe_compact_list* x, uint32_t index, fhe_radix** out);
int fhe_compact_list_expand_biguint(fhe_ctx* ctx, const fhe_compact_list* x, uint32_t index, fhe_biguint** out);
/* Test hook: the extraction kernel alone over every coefficient.  rows = ncoef x 2049 words, host pointer;
 * flushes and waits like a download. */
int fhe_compact_list_extract_rows(fhe_ctx* ctx, const fhe_compact_list* x, uint64_t* rows, size_t nwords);

/* ------------------------------------------------- re-randomization under the public key */
/* tfhe-rs' re_randomize under the CompactPublicKey: a fresh public-key encryption of ZERO is added to every
 * block of a value, so the ciphertext that enters a circuit has never been seen before -- the answer to the
 * IND-CPA-D setting of an engine whose decryptions become public (a signature is one).  Notation as above.
 * Blocks 0 .. n-1 of the value form chunks of 2048; from the 32-byte RE-RANDOMIZATION SEED, chunk c takes R
 * (bit i = bit i & 63 of u64 word 32 c + (i >> 6), nonce {109, "ROCM", 0}), E1 (2048 words from u64 word
 * 4096 c, nonce {110, "ROCM", 0}) and E2 (the words after E1, one per used block), the compact list's
 * positions under stream ids of their own, and forms Z_A = A R + E1, Z_B[j] = (B R)[j] + E2[j].  Block i
 * (t = i mod 2048 of chunk i / 2048): mask word u += Z_A[t - u] (u <= t), -= Z_A[t - u + 2048] (u > t), body +=
 * Z_B[t].  A trivial block enters as mask 0, body delta value.  At most 2^24 blocks.  The added phase error
 * E R + E2 - E1 S is below 2^30 in absolute value, against about 2^49.7 of a bootstrap's output: degree and
 * noise label of a block are unchanged.  No bootstrap.  tfhe-rs' bytes are not reproduced (parity unpinned).
 * SEED POLICY.  A seed is used for ONE call and then thrown away.  A seed that an adversary can predict before
 * choosing the ciphertext protects nothing: derive it from something fixed only after the ciphertext is (or
 * pass NULL).  seed = NULL draws 32 bytes from getrandom() and wipes them after the launch.  Under a
 * communicator of more than one rank NULL is refused (the ranks would diverge): every rank passes the same
 * seed, e.g. fhe_rerandomize_seed of a request id all ranks know. */
/* In place on nblocks rows of 2049 words; no context, no GPU.  The word-for-word definition of the device
 * path.  FHE_ERR_INVALID for a NULL argument or more than 2^24 blocks. */
int fhe_rerandomize_host(const fhe_public_key* pk, const uint8_t seed[32], uint64_t* cts, size_t nblocks);
/* Test hook: the zero encryptions alone.  za = Z_A of every chunk (2048 ceil(nblocks / 2048) words), zb = Z_B
 * of the used coefficients (nblocks words). */
int fhe_rerandomize_zero_host(const fhe_public_key* pk, const uint8_t seed[32], size_t nblocks, uint64_t* za,
                              size_t za_words, uint64_t* zb, size_t zb_words);
/* Uploads A and B (32 KB) once; after fhe_set_server_key, dropped by the next server-key install.  Rank-local:
 * under a communicator every rank installs the same key (the broadcast of a server key drops it on receivers).
 * FHE_ERR_NO_KEY without a server key; FHE_ERR_INVALID, the field named, if the key's parameters differ from
 * the installed server key's. */
int fhe_set_public_key(fhe_ctx* ctx, const fhe_public_key* pk);
/* Out of place: fresh slots; x and everyone who shares its slots are untouched.  Pending bootstraps x depends
 * on are launched first; then two gfx950 kernels (the zero encryptions; the extraction added to the source),
 * stream-ordered, no collective.  Only the seed and the slot pointers cross the bus.  The result's blocks are
 * real ciphertexts (a trivial block of x too).  BigUintFHE: the digits in order, 16 blocks each; the empty
 * vector gives the empty vector.  FHE_ERR_NO_KEY without an installed public key. */
int fhe_radix_rerandomize(fhe_ctx* ctx, const fhe_radix* x, const uint8_t seed[32] /* NULL: OS entropy */,
                          fhe_radix** out);
int fhe_biguint_rerandomize(fhe_ctx* ctx, const fhe_biguint* x, const uint8_t seed[32] /* NULL: OS entropy */,
                            fhe_biguint** out);
/* Test hook: the device path over nblocks host rows of 2049 words (any count up to 2^24, where a radix integer
 * stops at 2048 blocks): upload into slots, re-randomize, download into out; flushes and waits like a download. */
int fhe_rerandomize_rows(fhe_ctx* ctx, const uint8_t seed[32], const uint64_t* rows, size_t nblocks, uint64_t* out);
/* Measurement hook: the zero-encryption kernel alone, `reps` launches for nblocks blocks between two HIP events
 * on the context's stream; *ms = the mean per launch.  FHE_ERR_NO_KEY without an installed public key. */
int fhe_ctx_time_rerand_zero(fhe_ctx* ctx, const uint8_t seed[32], size_t nblocks, uint32_t reps, float* ms);
/* out = SHA-256(T || T || u64le(domain_len) || domain || data), T = SHA-256("fhe-rocm/rerandomize"): the
 * signer's tagged hash.  Replicas and ranks derive the same seed from public context (a request id, a message
 * hash); see the seed policy above for what that context must be. */
int fhe_rerandomize_seed(const uint8_t* domain, size_t domain_len, const uint8_t* data, size_t data_len,
                         uint8_t out[32]);

/* ------------------------------------------------------------------- ciphertext digests, bound seeds */
/* A re-randomization seed bound to the ciphertexts themselves (tfhe-rs' ReRandomizationContext): the seed is a
 * hash of the ciphertexts' own bytes plus domain separators, so nobody can choose a ciphertext knowing the seed
 * it will get, and every replica and every rank that holds the same ciphertexts derives the same seed -- no
 * NULL seed, no seed handed round.  The ciphertexts are hashed where they live: a gfx950 kernel, 32 bytes per
 * block across the bus.  SHA-256 throughout; H_t(m) = SHA-256(T || T || m), T = SHA-256(t), the signer's tagged
 * hash.  The hash and the framing are this engine's own (tfhe-rs' bytes are not reproduced: parity unpinned).
 * ROW DIGEST of a big LWE ciphertext (2049 u64 words, little-endian, 16,392 bytes):
 *   leaf[j]   = H_"fhe-rocm/ct-leaf"(row bytes [256 j, 256 j + 256)), j < 64;
 *   node[g]   = H_"fhe-rocm/ct-node"(leaf[8 g] || ... || leaf[8 g + 7]), g < 8;
 *   rowdigest = H_"fhe-rocm/ct-row"(node[0] || ... || node[7] || u64le(body)).
 * A trivial block enters as the row (mask 0, body delta value), fhe_radix_rerandomize's convention.
 * VALUE DIGEST  D(x) = H_"fhe-rocm/ct-value"(u8 kind || u32le(bits) || u32le(nblocks) || for each block in order:
 * u8 tag || u32le(degree) || u32le(noise) || rowdigest): kind FHE_CT_KIND_RADIX, or FHE_CT_KIND_BIGUINT with
 * bits = 32 digits, the digits in order, 16 blocks each (the empty vector: nblocks 0); tag 1 for a ciphertext
 * with its degree and noise label, tag 0 for a trivial block with its value in the degree field and noise 0 --
 * the per-block fields of the serialized form.
 * CONTEXT  a running SHA-256 over T_c || T_c || u64le(|domain|) || domain, T_c = SHA-256("fhe-rocm/rerandomize-
 * context"), then the items in call order as u8 kind || u64le(len) || payload: FHE_RERAND_ITEM_BYTES caller bytes
 * (a function description, a request id, a public key's serialization if the caller wants it bound),
 * FHE_RERAND_ITEM_DIGEST a 32-byte value digest.  root = the final digest; seed(i) = H_"fhe-rocm/rerandomize-
 * seed"(root || u64le(i)).  The first seed call finalizes the context: any later add returns FHE_ERR_INVALID,
 * because a seed must depend on everything that was added.  One index serves one re-randomization call. */
#define FHE_CT_KIND_RADIX 0
#define FHE_CT_KIND_BIGUINT 1
#define FHE_RERAND_ITEM_BYTES 1
#define FHE_RERAND_ITEM_DIGEST 2
typedef struct fhe_rerand_context fhe_rerand_context;
/* out = 32 bytes per row of 2049 words; no context, no GPU.  The word-for-word definition of the device path.
 * FHE_ERR_INVALID for a NULL argument or more than 2^24 rows. */
int fhe_ct_digest_host(const uint64_t* rows, size_t nblocks, uint8_t* out);
int fhe_ct_value_digest_host(uint8_t kind, uint32_t bits, const uint8_t* tags, const uint32_t* degrees,
                             const uint32_t* noises, const uint8_t* rowdigests, size_t nblocks, uint8_t out[32]);
int fhe_rerand_context_new(const uint8_t* domain, size_t domain_len, fhe_rerand_context** rc);
int fhe_rerand_context_add_bytes(fhe_rerand_context* rc, const uint8_t* data, size_t len);
int fhe_rerand_context_add_digest(fhe_rerand_context* rc, const uint8_t digest[32]);
int fhe_rerand_context_seed(fhe_rerand_context* rc, uint64_t index, uint8_t out[32]);
void fhe_rerand_context_destroy(fhe_rerand_context* rc);
/* D(x), the row digests computed on the GPU: pending bootstraps x depends on are launched first (under a
 * communicator the plain flush a decryption makes), a lazy block is made real; one kernel, one download of 32
 * bytes per block, one wait.  x is untouched.  No collective: every rank hashes its own replica of the operand
 * and gets the same bytes.  Needs a server key, not a public key. */
int fhe_radix_digest(fhe_ctx* ctx, const fhe_radix* x, uint8_t out[32]);
int fhe_biguint_digest(fhe_ctx* ctx, const fhe_biguint* x, uint8_t out[32]);
/* fhe_rerand_context_add_digest of fhe_radix_digest / fhe_biguint_digest */
int fhe_rerand_context_add_radix(fhe_ctx* ctx, fhe_rerand_context* rc, const fhe_radix* x);
int fhe_rerand_context_add_biguint(fhe_ctx* ctx, fhe_rerand_context* rc, const fhe_biguint* x);
/* Test hook: the device path over nblocks host rows of 2049 words (any count up to 2^24): upload into slots,
 * digest, download 32 bytes per row into out. */
int fhe_ct_digest_rows(fhe_ctx* ctx, const uint64_t* rows, size_t nblocks, uint8_t* out);
/* Measurement hook: the digest kernel alone, `reps` launches over nblocks resident rows between two HIP events
 * on the context's stream; *ms = the mean per launch. */
int fhe_ctx_time_ct_digest(fhe_ctx* ctx, size_t nblocks, uint32_t reps, float* ms);

/* ------------------------------------------------------------------- oblivious pseudo-random values */
/* tfhe-rs' FheUint::generate_oblivious_pseudo_random(seed, random_bits) and its bounded form: the server makes
 * an encrypted uniformly random value by itself, which nobody but the client-key holder can read -- blinding
 * values, random challenges, masks, without a round trip to the client.  No keyswitch, no upload: a gfx950
 * kernel writes LWE rows straight into the bootstrap workspace and one blind rotation does the rest.
 * With n the LWE dimension, N = 2048, delta = 2^63 / (message_modulus carry_modulus), 1 <= bits <=
 * log2(message_modulus), p = 2^bits:
 * ROWS         mask word j < n of row b = u64 word j of ChaCha blocks [b R, (b + 1) R), R = ceil(n / 8), of the
 *              stream (key = the 32 seed bytes, nonce {111, "ROCM", 0}, the seeded ciphertexts' word order); body
 *              word n = 0; in a layout of `stride` words per row the words above n hold 0xA5A55A5AC3C33C3C.  A row
 *              starts on a block boundary: the definition depends neither on the stride nor on the row count.
 * ACCUMULATOR  coefficient i < N = (2 floor(i p / 2N) + 1) delta / 2: no half-box rotation, no negated head.
 * BLOCK b      = sample extraction of the blind rotation of row b through the accumulator under the installed
 *              key set, then (p - 1) delta / 2 added to the body.  With m~ = -sum ms(a_i) s_i mod 2N (ms: the blind
 *              rotation's 12-bit rounding) it encrypts floor(m~ p / 2N) + p / 2 for m~ < N and p / 2 - 1 -
 *              floor((m~ - N) p / 2N) otherwise: in [0, p), uniform over the stream for a non-zero small key, and
 *              decided by the rounding alone (the bootstrap's noise does not move the selected coefficient's
 *              value).  Degree p - 1, noise 1: an ordinary clean block.  The rows are NOT centered and the result
 *              does not depend on fhe_ctx_set_modulus_switch: the phase is the randomness.
 * RADIX VALUE  of width_bits with random_bits r <= width_bits: blocks 0 .. floor(r / 2) - 1 at bits = 2 on the rows
 *              of their index, for an odd r block floor(r / 2) at bits = 1 on its row, trivial zeros above: uniform
 *              in [0, 2^r).
 * BOUNDED      random_below(bound, extra_bits): m = bit_length(bound - 1) + extra_bits; the result is
 *              (the m-bit value of the seed * bound) >> m at the caller's width, at most 2^-extra_bits from uniform
 *              on [0, bound).  Composed from the cast, the clear multiply and the clear shift of the radix layer.
 * SEEDS        A seed is PUBLIC.  The same seed, key and bits give the same words (replicas and ranks agree), so
 *              one seed serves one call; values drawn from one seed at different bits or widths are correlated.
 *              seed = NULL draws 32 bytes of OS entropy -- refused (FHE_ERR_INVALID) under a communicator of more
 *              than one rank, as fhe_radix_rerandomize's is: callers there derive the seed (fhe_rerandomize_seed,
 *              fhe_rerand_context_seed).
 * Eager: the kernels run on the context's stream behind whatever is launched; recorded but unflushed operations
 * stay pending.  Under a communicator every rank computes every block (no collective).  Classic and multi-bit
 * keys, every LWE dimension the key install accepts.  FHE_ERR_NO_KEY without a server key; FHE_ERR_INVALID with a
 * message for bits, widths or bounds out of range. */
/* The host definitions; no context, no GPU.  rows: count x stride words, stride >= n + 1, 1 <= n <= 2048, at most
 * 2^23 rows.  lut: the 2048 accumulator words for `params` and `bits`. */
int fhe_oprf_rows_host(const uint8_t seed[32], uint32_t n, size_t count, size_t stride, uint64_t* out);
int fhe_oprf_lut_host(const fhe_params* params, uint32_t bits, uint64_t* out);
/* Test hook: the row kernel (k_oprf_rows) over a scratch buffer in the bootstrap workspace's layout (n + 1 words
 * rounded up to 8 per row), each row's first min(stride, that) words copied to `out`, the marker above them.
 * Needs no server key, so any n runs without a key generation.  Same validation.  Synchronous. */
int fhe_oprf_rows(fhe_ctx* ctx, const uint8_t seed[32], uint32_t n, size_t count, size_t stride, uint64_t* out);
/* Measurement hook: the row kernel alone, `reps` launches over `count` workspace rows between two HIP events on
 * the context's stream; *ms = the mean per launch. */
int fhe_ctx_time_oprf_rows(fhe_ctx* ctx, size_t count, uint32_t n, uint32_t reps, float* ms);
/* Test hook: the raw blocks, count x 2049 words, blocks 0 .. count - 1 of the seed at `bits`. */
int fhe_oprf_blocks(fhe_ctx* ctx, const uint8_t seed[32], size_t count, uint32_t bits, uint64_t* out_words);
int fhe_radix_random(fhe_ctx* ctx, const uint8_t seed[32] /* NULL: OS entropy */, uint32_t width_bits,
                     uint32_t random_bits, fhe_radix** out);
/* bound: nwords little-endian u64 words, > 0, values below it fitting width_bits; FHE_ERR_INVALID when
 * bit_length(bound - 1) + extra_bits + bit_length(bound) exceeds FHE_RADIX_MAX_BITS */
int fhe_radix_random_below(fhe_ctx* ctx, const uint8_t seed[32] /* NULL: OS entropy */, uint32_t width_bits,
                           const uint64_t* bound_words, size_t nwords, uint32_t extra_bits, fhe_radix** out);
/* BigUintFHE of bits / 32 digits (bits a multiple of 32), block i of the whole on row i */
int fhe_biguint_random(fhe_ctx* ctx, const uint8_t seed[32] /* NULL: OS entropy */, uint32_t bits, fhe_biguint** out);

/* ------------------------------------------------------------------- modulus-switched stored ciphertexts */
/* tfhe-rs' FheUint::compress() -> CompressedModulusSwitchedCiphertext: a computed value parked or sent as the rows
 * its next bootstrap would read, n + 1 values of 12 bits per block -- 1,253 bytes per block at the defaults against
 * 16,392 of the full form (13x), with NO key beyond the server key.  Bringing it back costs one blind rotation
 * under the ordinary server key; the holder of the client key reads it with the small key alone, without a GPU.
 * With n the LWE dimension, for a block c of 2049 words:
 * ROW      r = keyswitch(c) (n + 1 words: body - sum_{j, l} d[j, l] KSK[j][l], balanced digits of the mask words
 *          rounded to their top ks_base_log ks_level bits); in FHE_MS_CENTERED the row's body then gives up the
 *          public half of the rounding residues, as fhe_ms_center_host does -- what every level of the mode does.
 * STORED   v[t] = (((r[t] >> 51) + 1) >> 1) & 4095 for t <= n, the blind rotation's own rounding; a row on the wire
 *          is the n + 1 values packed little-endian bit-contiguously (value t at bits [12 t, 12 t + 12)) from a
 *          byte boundary: ceil(12 (n + 1) / 8) bytes, the pad nibble of an odd n + 1 zero.
 * BACK     row words v[t] << 52 (no residue: the blind rotation's rounding returns v[t], and no centering runs on
 *          them), one blind rotation under the installed key set through the identity table over message_modulus
 *          carry_modulus values: fresh slots, noise 1, degree from the degree byte -- word for word what
 *          fhe_pbs_batch of c with that table gives in the same modulus-switch mode.
 * CLIENT   phase = (v[n] - sum_i v[i] s[i]) mod 4096, value = round(phase / 128) mod 16, assembled as
 *          fhe_radix_decrypt assembles blocks.  The decode margin and the rounding noise are those of a
 *          bootstrap's modulus switch (see fhe_ctx_set_modulus_switch).
 * Wire (kind 13): main params, u32 form (FHE_SEEDED_RADIX / FHE_SEEDED_BIGUINT semantics), u32 count (num_bits or
 * nlimbs), u32 B (blocks), B degree bytes (each < mc of the main params), B rows:  80 + B (1 + ceil(12 (n + 1) / 8))  bytes.  The
 * reader refuses truncation, non-zero pad bits, a degree >= mc, a block count that does not match form / count
 * and unsupported parameters. */
typedef struct fhe_switched_list fhe_switched_list;
/* The definitions on the host; no context, no GPU.  rows: count x stride words, stride >= n + 1, 1 <= n <= 2048,
 * words above n are not read (pack) / hold 0xA5A55A5AC3C33C3C (unpack: a bootstrap workspace row's padding).
 * packed: count rows at a distance of byte_stride >= ceil(12 (n + 1) / 8) bytes; the bytes between rows are
 * neither read nor written.  At most 2^24 rows. */
int fhe_switched_pack_host(const uint64_t* rows, size_t count, uint32_t n, size_t stride, uint8_t* packed,
                           size_t byte_stride);
int fhe_switched_unpack_host(const uint8_t* packed, size_t count, uint32_t n, size_t byte_stride, uint64_t* rows,
                             size_t stride);
/* The whole stored form on the host -- the word-for-word definition of fhe_radix_compress_switched, and what a
 * server without a GPU uses: ms_mode = FHE_MS_STANDARD / FHE_MS_CENTERED, cts = nblocks x 2049 words, degrees =
 * nblocks bytes (< mc = message_modulus * carry_modulus of the key), form / count as above (count / 2, or 16 count, must equal nblocks). */
int fhe_switched_compress_host(const fhe_server_key* sk, int ms_mode, const uint64_t* cts, size_t nblocks,
                               const uint8_t* degrees, uint32_t form, uint32_t count, fhe_switched_list** out);
int fhe_switched_list_info(const fhe_switched_list* x, uint32_t* form, uint32_t* count, size_t* nblocks);
int fhe_switched_list_params(const fhe_switched_list* x, fhe_params* main);
int fhe_switched_list_serialize(const fhe_switched_list* x, uint8_t* buf, size_t cap, size_t* len);
int fhe_switched_list_deserialize(const uint8_t* buf, size_t len, fhe_switched_list** out);
void fhe_switched_list_destroy(fhe_switched_list* x);
/* Client side, no GPU and no context; nwords >= ceil(bits / 64), bits = num_bits or 32 nlimbs.  FHE_ERR_INVALID,
 * with the differing field named, if the list's parameters are not the client key's. */
int fhe_switched_decrypt(const fhe_client_key* ck, const fhe_switched_list* x, uint64_t* words, size_t nwords);
/* FheUint::compress(): the value's blocks made real as for a download (pending producers launched -- a plain
 * flush, rank-local under a communicator; lazy blocks combined; a trivial block enters as (0, delta value)), then
 * per chunk of the bootstrap workspace the context's keyswitch (and centering, in that mode), the row-packing
 * kernel and one download.  Byte-identical to fhe_switched_compress_host on the exported blocks in the context's
 * mode.  FHE_ERR_INVALID for a block whose noise label admits no lookup, or of degree >= 16. */
int fhe_radix_compress_switched(fhe_ctx* ctx, const fhe_radix* x, fhe_switched_list** out);
int fhe_biguint_compress_switched(fhe_ctx* ctx, const fhe_biguint* x, fhe_switched_list** out);
/* decompress(): fresh block slots, stream-ordered like fhe_compressed_expand_radix (no flush, no collective: under
 * a communicator every rank expands the same bytes): upload, the row-unpacking kernel into the bootstrap
 * workspace, the blind rotate under the server key.  FHE_ERR_INVALID, with the differing field named, if the
 * list's parameters are not the installed server key's. */
int fhe_switched_expand_radix(fhe_ctx* ctx, const fhe_switched_list* x, fhe_radix** out);
int fhe_switched_expand_biguint(fhe_ctx* ctx, const fhe_switched_list* x, fhe_biguint** out);
/* Test hooks: the two kernels alone over scratch buffers in the device layouts (workspace rows of n + 1 words
 * rounded up to 8; packed rows of whole 12-byte groups), arguments and results as the host functions'.  They need
 * no server key, so any n runs without a key generation.  Same validation; FHE_ERR_INVALID too if a kernel wrote
 * behind its last device row.  Synchronous. */
int fhe_switched_pack_rows(fhe_ctx* ctx, const uint64_t* rows, size_t count, uint32_t n, size_t stride, uint8_t* packed,
                           size_t byte_stride);
int fhe_switched_unpack_rows(fhe_ctx* ctx, const uint8_t* packed, size_t count, uint32_t n, size_t byte_stride,
                             uint64_t* rows, size_t stride);
/* Measurement hook: each kernel alone, `reps` launches over `count` rows between HIP events on the context's
 * stream; the means per launch. */
int fhe_ctx_time_switched(fhe_ctx* ctx, size_t count, uint32_t n, uint32_t reps, float* pack_ms, float* unpack_ms);

/* ------------------------------------------------- re-keying through the stored form */
/* A stored row is the midpoint of a key change: keyswitched with a KSK from the big key of client key A to the
 * SMALL key of client key B, a value under A becomes a stored value under B -- B's client key reads it, a context
 * holding B's server key bootstraps it -- and the secret never appears in clear.  tfhe-rs' KeySwitchingKey; the
 * only way to rotate the FHE key over an Enc(d) whose owner no longer keeps d.  The owner of both client keys makes
 * the re-keying key; it is seeded only: the DESTINATION's parameters, a PUBLIC 32-byte seed and 2048 ks_level body
 * words, 82,020 bytes serialized at the defaults (kind 14: params | seed | bodies).
 *   masks   row r = j ks_level + l: mask word t < n_dst = u64 word 2048 r + t of the ChaCha20 stream keyed by the
 *           seed bytes, nonce {112, "ROCM", 0} -- the seeded server key's row stride under a stream id of its own
 *   noise   exactly 2048 ks_level words of the DESTINATION key's encryption stream, in row order:
 *           e = TUniform(lwe_noise_log2 of the destination) of the word
 *   body    bodies[r] = <mask_r, s_dst> + (S_src[j] << (64 - ks_base_log (l + 1))) + e
 * The two client keys must agree in message_modulus, carry_modulus, ks_base_log, ks_level, pbs_base_log and
 * glwe_noise_log2 (FHE_ERR_INVALID names the field); lwe_dimension, lwe_noise_log2 and grouping are the
 * destination's and may differ.  ONE SEED, ONE OBJECT, as for every seeded object.  A re-keyed row carries the
 * destination's keyswitch noise, and FHE_MS_CENTERED applies to it with the destination's dimension. */
typedef struct fhe_rekey_key fhe_rekey_key;
int fhe_rekey_key_generate(const fhe_client_key* src, fhe_client_key* dst, const uint8_t* mask_seed /* NULL: OS entropy */,
                           fhe_rekey_key** out);
int fhe_rekey_key_params(const fhe_rekey_key* key, fhe_params* out); /* the destination's */
int fhe_rekey_key_serialize(const fhe_rekey_key* key, uint8_t* buf, size_t cap, size_t* len);
int fhe_rekey_key_deserialize(const uint8_t* buf, size_t len, fhe_rekey_key** out);
/* the full KSK, [2048][ks_level][n_dst + 1] words in the server key's layout: the definition of the install */
int fhe_rekey_key_expand_host(const fhe_rekey_key* key, uint64_t* ksk, size_t len);
void fhe_rekey_key_destroy(fhe_rekey_key* key);
/* fhe_switched_compress_host with the expanded re-keying KSK in place of the server key's: the list carries the
 * destination's parameters.  The definition of fhe_*_compress_switched_rekeyed. */
int fhe_switched_compress_host_rekeyed(const fhe_rekey_key* key, int ms_mode, const uint64_t* cts, size_t nblocks,
                                       const uint8_t* degrees, uint32_t form, uint32_t count, fhe_switched_list** out);
/* After fhe_set_server_key; dropped by the next server-key install (then FHE_ERR_NO_KEY from the calls below).
 * FHE_ERR_INVALID, with the field named, unless the six shared fields equal the installed server key's.  Uploads
 * the bodies, regenerates the masks on the GPU, derives the byte planes; the key gets a row workspace of its own.
 * Nothing else of the context changes: every other call launches exactly as before. */
int fhe_set_rekey_key(fhe_ctx* ctx, const fhe_rekey_key* key);
/* fhe_*_compress_switched under the re-keying key: a stored value under the destination key. */
int fhe_radix_compress_switched_rekeyed(fhe_ctx* ctx, const fhe_radix* x, fhe_switched_list** out);
int fhe_biguint_compress_switched_rekeyed(fhe_ctx* ctx, const fhe_biguint* x, fhe_switched_list** out);

/* ------------------------------------------------------------------- Schnorr / BIP-340 */
/* The caller of the hot path (src/schnorr.rs).  32-byte scalars are big-endian.  The plaintext
 * EC / hash steps run on the host; the FHE block s = k + e*d runs on the GPU engine. */
int fhe_schnorr_public_key(const uint8_t privkey[32], uint8_t pubkey_x[32]);
/* compute_nonce (src/schnorr.rs:394-401) */
int fhe_schnorr_compute_nonce(const uint8_t privkey[32], const uint8_t* msg, size_t msg_len,
                              const uint8_t aux_rand[32], uint8_t k0[32]);
/* Schnorr::sign_with_k0 / sign (src/schnorr.rs:75-141), plaintext comparator */
int fhe_schnorr_sign_with_k0(const uint8_t* msg, size_t msg_len, const uint8_t k0[32],
                             const uint8_t privkey[32], uint8_t sig[64]);
int fhe_schnorr_sign(const uint8_t* msg, size_t msg_len, const uint8_t aux_rand[32],
                     const uint8_t privkey[32], uint8_t sig[64]);
/* The plaintext steps 1-5 of sign_fhe_with_k0 (src/schnorr.rs:239-267): k (k0, or n - k0 when R = k0 G
 * has odd y), the challenge e = H(R || P || m) and R's x -- so a caller can run the reference's own FHE
 * block (src/schnorr.rs:271-276) through fhe_biguint_encrypt / _mul / _add / _decrypt unchanged. */
int fhe_schnorr_sign_prologue(const uint8_t* msg, size_t msg_len, const uint8_t k0[32], const uint8_t privkey[32],
                              uint8_t k_out[32], uint8_t e_out[32], uint8_t rx_out[32]);
/* Schnorr::sign_fhe_with_k0 (src/schnorr.rs:235-290): privkey_fhe = BigUintFHE::new(privkey).
 * mode FHE_BIGUINT_COMPAT / FHE_BIGUINT_FAST run the reference's block (e and k encrypted, BigUintFHE
 * mul + add); FHE_SIGN_PUBLIC_OPERANDS keeps e and k in the clear (they are public values the
 * reference encrypts anyway, src/schnorr.rs:272-273): s = e * Enc(d') + k as one wide radix
 * scalar multiply-add.  All modes decrypt to the same s, hence byte-identical signatures. */
#define FHE_SIGN_PUBLIC_OPERANDS 2
int fhe_schnorr_sign_fhe_with_k0(fhe_ctx* ctx, fhe_client_key* ck, const uint8_t* msg, size_t msg_len,
                                 const uint8_t k0[32], const uint8_t privkey[32],
                                 const fhe_biguint* privkey_fhe, int mode, uint8_t sig[64]);
/* fhe_schnorr_sign_fhe_with_k0 on a re-randomized copy of privkey_fhe, the seed bound to the request: a
 * re-randomization context over `domain`, the bytes r_x || pubkey_x || msg and the value digest of privkey_fhe
 * added, privkey_fhe re-randomized with seed(0) before anything else of the call starts, then the existing
 * signing path on the result.  sig is byte for byte the existing call's; privkey_fhe is untouched.  Works under
 * a communicator (every rank derives the same seed).  FHE_ERR_NO_KEY without an installed public key. */
int fhe_schnorr_sign_fhe_with_k0_rerand(fhe_ctx* ctx, fhe_client_key* ck, const uint8_t* msg, size_t msg_len,
                                        const uint8_t k0[32], const uint8_t privkey[32],
                                        const fhe_biguint* privkey_fhe, int mode, const uint8_t* domain,
                                        size_t domain_len, uint8_t sig[64]);
/* count independent sign_fhe_with_k0 calls as ONE engine schedule (their bootstraps share launch
 * levels: a batch of signatures costs far less than count single calls on one GPU).  msgs[i] /
 * lens[i]; k0s, privkeys: count x 32 bytes; sigs: count x 64 bytes, each identical to the single call */
int fhe_schnorr_sign_fhe_with_k0_batch(fhe_ctx* ctx, fhe_client_key* ck, size_t count, const uint8_t* const* msgs,
                                       const size_t* lens, const uint8_t* k0s, const uint8_t* privkeys,
                                       const fhe_biguint* const* privkeys_fhe, int mode, uint8_t* sigs);
/* The signature with s reduced mod n UNDER ENCRYPTION.  The calls above decrypt s_without_mod = k + e d' (about
 * 513 bits) and reduce on the host, as the reference does; whoever sees that plaintext has d' (e is public and
 * floor(s_without_mod / e) is d' or a neighbour).  These decrypt 256 bits whose plaintext is exactly the
 * signature's s -- public anyway.  The column form goes through fhe_columns_rem_pseudo_mersenne (n = 2^256 - c,
 * c of 129 bits: three folds, then one propagation and select at 258 bits); FHE_SIGN_PUBLIC_OPERANDS reduces the product as
 * it is formed (fhe_radix_scalar_mul_add_rem_pseudo_mersenne).  No host % n: a decrypted value not below n is
 * FHE_ERR_INVALID.  Same arguments, modes and signature bytes as the unreduced calls. */
int fhe_schnorr_sign_fhe_with_k0_reduced(fhe_ctx* ctx, fhe_client_key* ck, const uint8_t* msg, size_t msg_len,
                                         const uint8_t k0[32], const uint8_t privkey[32],
                                         const fhe_biguint* privkey_fhe, int mode, uint8_t sig[64]);
int fhe_schnorr_sign_fhe_with_k0_rerand_reduced(fhe_ctx* ctx, fhe_client_key* ck, const uint8_t* msg, size_t msg_len,
                                                const uint8_t k0[32], const uint8_t privkey[32],
                                                const fhe_biguint* privkey_fhe, int mode, const uint8_t* domain,
                                                size_t domain_len, uint8_t sig[64]);
int fhe_schnorr_sign_fhe_with_k0_batch_reduced(fhe_ctx* ctx, fhe_client_key* ck, size_t count,
                                               const uint8_t* const* msgs, const size_t* lens, const uint8_t* k0s,
                                               const uint8_t* privkeys, const fhe_biguint* const* privkeys_fhe, int mode,
                                               uint8_t* sigs);
/* The server's half alone, for a deployment where another party decrypts: Enc(s), s = (k + e d') mod n, as an
 * FheUint256 of clean blocks (every radix op, compression, serialization and re-randomization applies).  Takes
 * no client key.  mode FHE_BIGUINT_COMPAT (the reference's limbs, lost carries included, then reduced) or
 * FHE_BIGUINT_FAST. */
int fhe_schnorr_eval_s(fhe_ctx* ctx, const fhe_biguint* e_fhe, const fhe_biguint* k_fhe, const fhe_biguint* privkey_fhe,
                       int mode, fhe_radix** s);
/* ... with e and k in the clear (big-endian, both below n) */
int fhe_schnorr_eval_s_public(fhe_ctx* ctx, const uint8_t e[32], const uint8_t k[32], const fhe_biguint* privkey_fhe,
                              fhe_radix** s);
/* Schnorr::sign_fhe (src/schnorr.rs:154-211) */
int fhe_schnorr_sign_fhe(fhe_ctx* ctx, fhe_client_key* ck, const uint8_t* msg, size_t msg_len,
                         const uint8_t aux_rand[32], const uint8_t privkey[32], int mode, uint8_t sig[64]);
/* Schnorr::verify (src/schnorr.rs:301-347): 1 valid, 0 invalid */
int fhe_schnorr_verify(const uint8_t* msg, size_t msg_len, const uint8_t* pubkey, size_t pubkey_len,
                       const uint8_t* sig, size_t sig_len);

/* ---- resident client key: encryption and decryption on the GPU ----
 *
 * For a process that holds the client key ANYWAY, as the reference's signer does (sign_fhe_with_k0 takes the
 * client key, encrypts e and k with it and decrypts the sum).  A server that only evaluates never calls this: it
 * has no client key, and nothing here gives it one.
 *
 * fhe_ctx_set_client_key copies the big secret key, as 2048 packed bits, to the device and keeps a host copy of
 * those bits; it keeps no pointer to ck.  It is the opt-in: with no key resident every path is byte for byte what
 * it is without this section.  With one, every call that takes a client key still takes it, and goes to the device
 * only when ck's packed key bits equal the resident ones:
 *   - fhe_radix_encrypt, fhe_biguint_encrypt and the signers' encryptions of e and k: only the scaled plaintexts,
 *     the slot pointers (16 B per block) and the encryption stream's key, nonce and position go up; the masks are
 *     generated, and the bodies computed, on the context's stream -- word for word fhe_encrypt_blocks' rows, and
 *     ck's encryption stream stands afterwards where the host path leaves it.  The signers start no helper thread
 *     and arm no deferred upload in this case.
 *   - fhe_radix_decrypt, fhe_biguint_decrypt, fhe_columns_decrypt and the signers' last step: body - <mask, key>
 *     is computed on the device and 8 bytes per block come back; the decoding stays on the host.
 * With another key (or a batch that would leave the stream's 32-bit block counter) the host path runs, as without
 * a resident key: same words, no error.  The seeded, compact, compressed and stored client paths take no context
 * and do not change.  Under a communicator every rank installs the key itself.
 * Errors: FHE_ERR_INVALID for a NULL argument, a simulated context, or a client key whose parameters differ from
 * the installed server key's; FHE_ERR_NO_KEY without a server key.
 * fhe_ctx_clear_client_key overwrites the device copy and the host copy with zeros, then frees them (FHE_OK when
 * none is resident); fhe_ctx_destroy and an install of a server key with other parameters do the same. */
int fhe_ctx_set_client_key(fhe_ctx* ctx, const fhe_client_key* ck);
int fhe_ctx_clear_client_key(fhe_ctx* ctx);
/* *resident: 1 while a key is resident; the blocks that took the device encryption / the device phase path
 * since the context was made */
int fhe_ctx_client_ops_info(fhe_ctx* ctx, int* resident, uint64_t* enc_blocks, uint64_t* phase_blocks);
/* HOST DEFINITIONS (no context, no GPU).  fhe_client_encrypt_rows_indexed_host: fhe_encrypt_blocks restated from
 * counter-indexed ChaCha blocks through the index arithmetic the kernel uses (csrc/client_ops_index.h) -- the same
 * n x 2049 words and the same stream state afterwards.  fhe_decrypt_phase_host: phases[i] = body - <mask, key> of
 * row i, the word fhe_decrypt_block decodes. */
int fhe_client_encrypt_rows_indexed_host(fhe_client_key* ck, const uint64_t* values, size_t n, uint64_t* cts);
int fhe_decrypt_phase_host(const fhe_client_key* ck, const uint64_t* cts, size_t n, uint64_t* phases);
/* TEST HOOKS: the two kernels over scratch rows under the resident key (FHE_ERR_NO_KEY without one).
 * fhe_client_encrypt_rows: n rows of 2049 words for the block values, downloaded; ck must be the resident key
 * (FHE_ERR_INVALID otherwise) and its stream advances as fhe_encrypt_blocks'.  fhe_client_phase_rows: the phases
 * of n uploaded rows.  At most 2^20 rows. */
int fhe_client_encrypt_rows(fhe_ctx* ctx, fhe_client_key* ck, const uint64_t* values, size_t n, uint64_t* cts);
int fhe_client_phase_rows(fhe_ctx* ctx, const uint64_t* cts, size_t n, uint64_t* phases);
/* MEASUREMENT HOOK: mean ms of one launch of each kernel over n scratch rows, `iters` launches each, under a fixed
 * public key of its own (needs no installed key) */
int fhe_ctx_time_client_ops(fhe_ctx* ctx, size_t n, uint32_t iters, float* enc_ms, float* phase_ms);

#ifdef __cplusplus
}
#endif
#endif
