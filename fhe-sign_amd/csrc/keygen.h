// keygen.h -- device server-key generation (keygen.hip), bit-identical to keys.cpp:generate_keys.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fhe {

// ChaCha20 key and nonce of one stream (keys.cpp ChaChaStream::reset); block counter = index
struct ChaChaKey {
    uint32_t key[8];
    uint32_t nonce[3];
};
ChaChaKey chacha_stream_key(const uint32_t key[8], uint32_t stream);

// out[q] = u64 word q of the stream (q < count; count / 8 blocks must stay below 2^32)
hipError_t launch_chacha_u64(const ChaChaKey& k, uint64_t* out, uint64_t count, hipStream_t s);
// seeded.hip: for b < nblocks, dst[b][0 .. 2048) = u64 words [2048 b, 2048 b + 2048) of the stream (ChaCha
// blocks 256 b ..; nblocks <= 2^24 keeps the counter in 32 bits) and dst[b][2048] = bodies[b]; dst and
// bodies are device arrays, every dst[b] a slot of 2049 words
hipError_t launch_expand_seeded(const ChaChaKey& k, uint64_t* const* dst, const uint64_t* bodies, int nblocks,
                                hipStream_t s);
// seeded_key.hip: for r < rows, ksk[r (n + 1) + t] = u64 word 2048 r + t of the stream for t < n (n <= 2048)
// and ksk[r (n + 1) + n] = bodies[r]; nothing else is written
hipError_t launch_expand_ksk(const ChaChaKey& k, uint64_t* ksk, const uint64_t* bodies, int rows, int n,
                             hipStream_t s);
// seeded_key.hip: launch_bsk_to_fourier (kernels.h) of the standard-domain key whose polynomial 2 r is u64
// words [2048 r, 2048 r + 2048) of the stream and whose polynomial 2 r + 1 is bodies[2048 r ..], without
// that key in memory; npoly = 4 ggsw, bodies holds npoly / 2 polynomials
hipError_t launch_expand_bsk_fourier(const ChaChaKey& k, const uint64_t* bodies, int npoly, const double2* W,
                                     const double2* psi, double2* out, hipStream_t s);
// public_key.hip: for i < count, dst[i][0 .. 2048] = the big LWE sample-extracted at coefficient first + i of
// the staged chunks (ca: 2048 words of C_A per chunk; coefficient g lies in chunk g / 2048 at t = g % 2048):
// mask word u = ca[t - u] for u <= t, -ca[t - u + 2048] for u > t, body cb[i].  ca, cb and dst are device
// arrays, every dst[i] a slot of 2049 words; the caller stages every chunk that [first, first + count) touches
hipError_t launch_compact_extract(const uint64_t* ca, const uint64_t* cb, uint64_t* const* dst, uint32_t first, int count,
                                  hipStream_t s);
// rerandomize.hip: the zero encryptions of nblocks blocks (public_key.h "re-randomization").  ab = the public
// key's A then B (2048 words each); z = ceil(nblocks / 2048) chunks of Z_A then Z_B (2048 words each), Z_B's
// noise on the used coefficients only; kbin / knoise = the re-randomization seed's two streams.  nblocks <= 2^24
hipError_t launch_rerand_zero(const ChaChaKey& kbin, const ChaChaKey& knoise, const uint64_t* ab, uint64_t* z, uint32_t nblocks,
                              uint32_t noise_log2, hipStream_t s);
// rerandomize.hip: for i < nblocks, dst[i][0 .. 2048] = the source block + the sample extraction of z at
// coefficient i; the source is the slot src[i], or for src[i] == null the trivial ciphertext (0, tbody[i]).
// src, tbody and dst are device arrays, every slot 2049 words
hipError_t launch_rerand_add(const uint64_t* z, const uint64_t* const* src, const uint64_t* tbody, uint64_t* const* dst,
                             uint32_t nblocks, hipStream_t s);
// ksk holds the KSK stream words ([rows][n + 1], rows = N * levels): bodies computed in place
hipError_t launch_ksk_bodies(uint64_t* ksk, const uint64_t* lwe_sk, const uint64_t* glwe_sk, int n, int rows,
                             int levels, int base_log, int noise_log2, hipStream_t s);
// bsk holds the BSK stream words ([nggsw][2][2][N]): bodies, then gadgets (msgs[i] << ...), in place
hipError_t launch_bsk_bodies(uint64_t* bsk, const uint64_t* msgs, const uint64_t* glwe_sk, int nggsw, int pbs_base_log,
                             int noise_log2, hipStream_t s);

}  // namespace fhe
