// key_sets.h -- the device form of a key as one owned, move-only unit: the buffers, and next to them the dimension
// they were sized for.  A set is sized (size), filled by its install on a stream, and then derives its second
// layout from the first (derive); drop() frees it.  Like the DeviceBufs they are made of the sets never
// synchronise: the caller waits before it drops or replaces a set that queued work may still read.
#pragma once
#include "device_buf.h"
#include "kernels.h"

namespace fhe {

// What one keyswitch runs under: a keyswitch key set and the row space its rows go to
struct KsKeys {
    const uint64_t* ksk;
    const int8_t* planes;
    int n;
    uint64_t* ms;
    int ms_stride;
};
// What one blind rotation runs under: a blind-rotate key set and the row space holding its inputs
struct BrKeys {
    const double2 *bsk, *bsk_e;
    int n, grouping;
    const uint64_t* ms;
    int ms_stride;
};

// Keyswitch key to a small key of dimension n: u64 rows [2048 ks_level][n + 1] (FHE_KS_VALU reads them) and the
// balanced signed-byte planes derived from them (ks_mfma.hip)
struct KsKeySet {
    DeviceBuf<uint64_t> ksk;
    DeviceBuf<int8_t> planes;
    int n = 0;
    hipError_t size(int dim, int ks_level) {
        n = dim;
        return grow_each(ksk, (size_t)2048 * ks_level * (dim + 1), planes, ks_planes_bytes(dim));
    }
    hipError_t derive(hipStream_t s) const { return launch_ksk_to_planes(ksk, n, planes, s); }
    void drop() {
        (void)ksk.reset();
        (void)planes.reset();
        n = 0;
    }
    KsKeys on(const RowSpace& r) const { return {ksk, planes, n, r.rows(), r.stride()}; }
};

// Fourier bootstrapping key of `npoly` polynomials in two resident layouts: bsk for the latency kernel
// (br_wide.hip), bsk_e, derived from it, for the throughput kernel (br_qy.hip)
struct BrKeySet {
    DeviceBuf<double2> bsk, bsk_e;
    int n = 0, grouping = 1, npoly = 0;
    hipError_t size(int dim, int group, int polys) {
        n = dim;
        grouping = group;
        npoly = polys;
        return grow_each(bsk, (size_t)polys * 1024, bsk_e, (size_t)polys * 1024);
    }
    hipError_t derive(hipStream_t s) const { return launch_bsk_to_e(bsk, npoly, bsk_e, s); }
    void drop() {
        (void)bsk.reset();
        (void)bsk_e.reset();
        n = npoly = 0;
        grouping = 1;
    }
    BrKeys on(const RowSpace& r) const { return {bsk, bsk_e, n, grouping, r.rows(), r.stride()}; }
};

// A server key: what fhe_set_server_key installs and a receiver of fhe_ctx_broadcast_server_key builds aside
struct ServerKeySet {
    KsKeySet ks;
    BrKeySet br;
    hipError_t derive(hipStream_t s) const {
        const hipError_t e = ks.derive(s);
        return e != hipSuccess ? e : br.derive(s);
    }
    void drop() {
        ks.drop();
        br.drop();
    }
};

}  // namespace fhe
