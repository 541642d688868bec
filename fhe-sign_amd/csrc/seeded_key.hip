// seeded_key.hip -- installation of a seeded (compressed) server key on the GPU.
//
// A seeded server key carries a public 32-byte seed and the bodies only (keys.h fhe_seeded_server_key);
// the masks are ChaCha20 streams under the seed, one row per 256 ChaCha blocks (2048 u64 words):
//   KSK row r (stream kStreamSeededKsk): mask word t < n = u64 word 2048 r + t
//   BSK mask polynomial of GGSW q, row rho (stream kStreamSeededBsk): words [2048 (2 q + rho), + 2048)
// The two kernels here write, word for word, what keys.cpp:expand_seeded_server_key_host followed by the
// full install (context.cpp) leaves on the device:
//   k_expand_ksk          a KsKeySet's ksk [N ks_level][n + 1]: masks regenerated, body appended
//   k_expand_bsk_fourier  the Fourier BSK (k_bsk_to_fourier's layout and bits): a mask polynomial's
//                         coefficients are generated into LDS instead of loaded, so the standard-domain
//                         BSK never exists in device memory; a body polynomial is read from the upload
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "chacha_device.h"
#include "device_math.h"
#include "keygen.h"

namespace fhe {

namespace {

// a KSK row is n + 1 words: only 8-byte aligned (global dwordx4 stores accept that)
typedef __attribute__((address_space(1))) u32x4 g_u32x4_a8 __attribute__((aligned(8)));
typedef __attribute__((address_space(1))) uint64_t g_u64;

// One 256-lane workgroup per KSK row; wave w covers the row's ChaCha blocks 64 w .. 64 w + 63 = mask words
// [512 w, 512 w + 512) and leaves at once if the row ends before them.  Within a wave the quad exchange of
// chacha_device.h makes store s of lane l the words 512 w + 128 s + 2 l and + 1: consecutive lanes write
// consecutive 16-byte parts.  A row ends at word n, anywhere inside a block: a pair that lies below n is one
// dwordx4 store, the pair that straddles n (odd n) stores its first word alone, everything from n on -- the
// 8 ceil(n / 8) - n spare words of the row's last block, and the blocks the wave computed past it -- is
// dropped.  Lane 0 of wave 0 stores the body.
__global__ __launch_bounds__(256) void k_expand_ksk(ChaChaKey k, uint64_t* __restrict__ ksk,
                                                    const uint64_t* __restrict__ bodies, uint32_t n) {
    const uint32_t row = blockIdx.x;
    g_u64* dst = (g_u64*)ksk + (size_t)row * (n + 1);
    if (threadIdx.x == 0) dst[n] = bodies[row];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (wave * 512u >= n) return;  // wave-uniform
    const uint32_t p = lane & 3, q = lane >> 2;
    uint32_t o[16];
    chacha_block(k, row * 256u + wave * 64u + p * 16u + q, o);
    u32x4 w[4];
    chacha_quad_exchange(o, p, w);
#pragma unroll
    for (uint32_t s = 0; s < 4; ++s) {
        const uint32_t t = wave * 512u + s * 128u + lane * 2u;  // first of this store's two mask words
        if (t + 1 < n)
            *(g_u32x4_a8*)(dst + t) = w[s];
        else if (t < n)
            dst[t] = (uint64_t)w[s].x | (uint64_t)w[s].y << 32;
    }
}

// One wave per polynomial, as k_bsk_to_fourier: polynomial 2 r of the standard-domain key is row r's mask,
// 2 r + 1 its body.  For a mask, lane L computes the row's ChaCha blocks L, L + 64, L + 128, L + 192 (eight
// coefficients each) into a 16 KB LDS copy of the polynomial; from the loads on, the instructions are
// k_bsk_to_fourier's, so the Fourier words are bit-identical to its on the host-expanded key.
__global__ __launch_bounds__(64) void k_expand_bsk_fourier(ChaChaKey k, const uint64_t* __restrict__ bodies,
                                                           int npoly, const cplx* __restrict__ W,
                                                           const cplx* __restrict__ psi, cplx* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) cplx sc[FFT_SCRATCH];
    __shared__ __attribute__((aligned(16))) uint64_t stage[2048];
    const int q = blockIdx.x;
    if (q >= npoly) return;
    const int L = threadIdx.x;
    const uint32_t row = (uint32_t)q >> 1;
    cplx x[16];
    if (!(q & 1)) {
#pragma unroll 1  // one block's 32 registers at a time: four interleaved blocks spill into AGPRs
        for (int b = 0; b < 4; ++b) {
            uint32_t o[16];
            chacha_block(k, row * 256u + (uint32_t)(L + 64 * b), o);
            uint64_t* d = stage + 8 * (L + 64 * b);  // 64-byte aligned: the eight stores merge into wide ones
#pragma unroll
            for (int i = 0; i < 8; ++i) d[i] = (uint64_t)o[2 * i] | (uint64_t)o[2 * i + 1] << 32;
        }
        wave_sync();
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const double re = (double)(int64_t)stage[L + 64 * t];
            const double im = (double)(int64_t)stage[L + 64 * t + 1024];
            x[t] = cmul(make_double2(re, im), psi[L + 64 * t]);
        }
    } else {
        const uint64_t* p = bodies + (size_t)row * 2048;
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const double re = (double)(int64_t)p[L + 64 * t];
            const double im = (double)(int64_t)p[L + 64 * t + 1024];
            x[t] = cmul(make_double2(re, im), psi[L + 64 * t]);
        }
    }
    fft_forward(x, sc, L, as_global(W) + L);
    cplx* o = out + (size_t)q * 1024 + L;
#pragma unroll
    for (int R = 0; R < 16; ++R) o[R * 64] = x[R];
}

}  // namespace

hipError_t launch_expand_ksk(const ChaChaKey& k, uint64_t* ksk, const uint64_t* bodies, int rows, int n,
                             hipStream_t s) {
    if (rows <= 0 || n <= 0 || n > 2048) return hipErrorInvalidValue;
    k_expand_ksk<<<rows, 256, 0, s>>>(k, ksk, bodies, (uint32_t)n);
    return hipGetLastError();
}

hipError_t launch_expand_bsk_fourier(const ChaChaKey& k, const uint64_t* bodies, int npoly, const double2* W,
                                     const double2* psi, double2* out, hipStream_t s) {
    if (npoly <= 0) return hipErrorInvalidValue;
    k_expand_bsk_fourier<<<npoly, 64, 0, s>>>(k, bodies, npoly, W, psi, out);
    return hipGetLastError();
}

}  // namespace fhe
