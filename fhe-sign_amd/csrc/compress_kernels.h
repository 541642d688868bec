// compress_kernels.h -- host launchers of compress.hip (packing keyswitch, 12-bit pack / unpack).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "keygen.h"

namespace fhe {

int pk_col_tiles(int cols);
size_t pk_planes_bytes(int ell, int cols);
size_t pk_digits_bytes(int count, int ell);
// bytes between two GLWEs in the device's packed output: (k' + 1) 1.5 N' rounded up to 16, so that every
// polynomial's stream starts on a 32-bit word (the host compacts to byte boundaries after the one download)
int pk_out_stride(int k, int Np);
// pksk u64 [2048][ell][cols] -> int8 [8][column tiles][32 ell][64][16] (once, at fhe_set_compression_key)
hipError_t launch_pksk_to_planes(const uint64_t* pksk, int ell, int cols, int8_t* planes, hipStream_t s);
// seeded_compression.hip: the same planes, byte for byte, of the packing key whose row r has u64 words
// [2048 r, 2048 r + k Np) of the stream as its masks and bodies[r Np .. + Np) as its body, without that key
// in memory; bodies is a device array of 2048 ell Np words
hipError_t launch_expand_pksk_planes(const ChaChaKey& key, const uint64_t* bodies, int ell, int k, int Np,
                                     int8_t* planes, hipStream_t s);
// src[i] (device array of `count` slot pointers, 2049 words each) -> out[g * pk_out_stride + ..]: GLWE g's
// k' N' mask values, then L body slots (the unused ones zero), 12 bits each.  digits: pk_digits_bytes(count,
// ell); body: count words; P: count x (k' + 1) N' words.
hipError_t launch_pack_keyswitch(const uint64_t* const* src, int count, int beta, int ell, int k, int Np, int L,
                                 const int8_t* planes, int8_t* digits, uint64_t* body, uint64_t* P, uint8_t* out,
                                 hipStream_t s);
// packed (the wire layout: GLWE g at g * glwe_bytes) -> rows[i * stride + ..] = block i's k' N' + 1 sample-
// extracted values << 52; stride >= k' N' + 1
hipError_t launch_pk_unpack(const uint8_t* packed, int count, int glwe_bytes, int L, int Np, int k, uint64_t* rows,
                            int stride, hipStream_t s);

}  // namespace fhe
