// client_ops.h -- encryption and the decryption phase on the device under a resident client key:
// the kernels' launchers (client_ops.hip) and the host definitions (client_ops.cpp).  The engine's two paths are
// Engine::encrypt_resident and Engine::phases_many (engine_ops.cpp); the residency itself is fhe_ctx's
// (context.h: d_client, fhe_ctx_set_client_key).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <stddef.h>

struct fhe_client_key;

namespace fhe {

// client = the resident buffer: 64 words of key bits, then client_ops::StreamParams of this call.
// For b < nblocks: dst[b][0 .. 2048) = u64 stream words [W0 + 2049 b, + 2048) of the stream the parameters name,
// dst[b][2048] = <mask, key> + pts[b] + tuniform(word W0 + 2049 b + 2048).  dst and pts are device arrays, every
// dst[b] a slot of 2049 words; the batch stays inside the stream's 32-bit block counter (the caller checks).
hipError_t launch_client_encrypt(const uint32_t* client, uint64_t* const* dst, const uint64_t* pts, size_t nblocks,
                                 hipStream_t s);
// phases[b] = src[b][2048] - <src[b][0 .. 2048), key> for b < nblocks; src and phases are device arrays
hipError_t launch_client_phase(const uint32_t* client, const uint64_t* const* src, uint64_t* phases, size_t nblocks,
                               hipStream_t s);

// the big secret key as 2048 packed bits: bit j of word j / 32 = glwe_sk[j]
void client_pack_key_bits(const fhe_client_key* ck, uint32_t bits[64]);
// encrypt_big_many restated from counter-indexed ChaCha blocks through client_ops_index.h, as the kernel computes
// it: same words, same stream state afterwards.  False (nothing done) if the batch leaves the counter epoch.
bool client_encrypt_rows_indexed_host(fhe_client_key* ck, const uint64_t* pts, size_t n, uint64_t* cts);

}  // namespace fhe
