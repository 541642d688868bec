// device_buf_host_check.cpp -- stand-alone driver of DeviceBuf, GroupCap and RowSpace (fhe-sign_amd/csrc/device_buf.h; no GPU call) over
// an allocator backed by malloc / free, for a host AddressSanitizer + UndefinedBehaviorSanitizer run with its own
// main: a double free, a use after free or a leak of the buffer's is then the sanitizer's to report.
//   clang++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -D__HIP_PLATFORM_AMD__ \
//           -I/opt/rocm/include -Ifhe-sign_amd/csrc tools/device_buf_host_check.cpp -o device_buf_host_check
// (clang++ = the ROCm toolchain's; only hipError_t comes from the HIP header, nothing links against the runtime).
// FakeAlloc counts the live allocations, records the byte counts asked for, and fails its k-th allocation or
// k-th free on request (a failed free still releases the memory: the sanitizer's leak check stays meaningful).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "device_buf.h"

struct FakeAlloc {
    static int live, allocs, frees, fail_alloc, fail_free;  // fail_*: countdown, 1 = the next call fails
    static std::vector<size_t> sizes;
    static hipError_t alloc(void** p, size_t bytes) {
        ++allocs;
        sizes.push_back(bytes);
        if (fail_alloc > 0 && --fail_alloc == 0) return hipErrorOutOfMemory;
        *p = std::malloc(bytes ? bytes : 1);
        if (!*p) return hipErrorOutOfMemory;
        std::memset(*p, 0xA5, bytes);
        ++live;
        return hipSuccess;
    }
    static hipError_t free(void* p) {
        ++frees;
        std::free(p);
        --live;
        if (fail_free > 0 && --fail_free == 0) return hipErrorInvalidValue;
        return hipSuccess;
    }
    static void start() {
        allocs = frees = fail_alloc = fail_free = 0;
        sizes.clear();
    }
};
int FakeAlloc::live = 0, FakeAlloc::allocs = 0, FakeAlloc::frees = 0, FakeAlloc::fail_alloc = 0, FakeAlloc::fail_free = 0;
std::vector<size_t> FakeAlloc::sizes;

using Buf = fhe::DeviceBuf<uint64_t, FakeAlloc>;
using F = FakeAlloc;

#define CHECK(x) do { if (!(x)) { std::printf("FAIL line %d: %s\n", __LINE__, #x); return 1; } } while (0)

// every word of the buffer is the allocator's fill and can be written: a stale or short buffer is the sanitizer's
static bool usable(const Buf& b) {
    uint64_t* p = b;
    for (size_t i = 0; i < b.capacity(); ++i) {
        if (p[i] != 0xA5A5A5A5A5A5A5A5ull) return false;
        p[i] = 0xA5A5A5A5A5A5A5A5ull;
    }
    return true;
}

// a workspace as the context builds one: three buffers under a GroupCap, floor 256 (fhe_ctx::ensure_stage)
struct Group {
    Buf a, b, c;
    fhe::GroupCap cap;
    hipError_t ensure(size_t count) {
        if (cap.fits(count)) return hipSuccess;
        return cap.regrow(count, 256, [&](size_t n) { return fhe::grow_each(a, n * 3, b, n * 3, c, n); });
    }
};
// a row space with two more buffers in its group (fhe_ctx::ensure_cms), rows of dimension n
struct Rows {
    fhe::RowSpaceOf<FakeAlloc> rs;
    Buf x, y;
    hipError_t ensure(size_t count, size_t n) {
        if (rs.fits(count)) return hipSuccess;
        return rs.regrow(count, n, [&](size_t cap) { return fhe::grow_each(x, cap * 2, y, cap); });
    }
};
// empty, or whole at the old or at the new count
static bool whole_or_empty(const Buf& b, size_t was, size_t now) {
    return (!b && b.capacity() == 0) || ((b.capacity() == was || b.capacity() == now) && usable(b));
}

static int checks() {
    F::start();
    {  // empty, grow from empty, grow larger, fits around the capacity
        Buf b;
        CHECK(b.get() == nullptr && b.capacity() == 0 && !b && b.fits(0) && !b.fits(1));
        CHECK(b.grow(10) == hipSuccess && b.get() && b.capacity() == 10 && F::live == 1 && F::frees == 0);
        CHECK(F::sizes.back() == 80 && usable(b));
        CHECK(b.fits(9) && b.fits(10) && !b.fits(11));
        uint64_t* const raw = b;
        CHECK(raw == b.get() && b + 3 == raw + 3);
        CHECK(b.grow(1000) == hipSuccess && b.capacity() == 1000 && F::live == 1 && F::frees == 1);
        CHECK(F::sizes.back() == 8000 && usable(b));
        CHECK(b.fits(999) && b.fits(1000) && !b.fits(1001));
        CHECK(b.grow(4) == hipSuccess && b.capacity() == 4 && F::live == 1 && usable(b));  // exactly what is asked
    }
    CHECK(F::live == 0 && F::allocs == 3 && F::frees == 3);  // the destructor freed the last one

    F::start();
    {  // the allocation fails: empty, nothing live, the next grow succeeds
        Buf b;
        CHECK(b.grow(16) == hipSuccess);
        F::fail_alloc = 1;
        CHECK(b.grow(32) == hipErrorOutOfMemory);
        CHECK(b.get() == nullptr && b.capacity() == 0 && !b.fits(1) && F::live == 0);
        CHECK(b.grow(32) == hipSuccess && b.capacity() == 32 && F::live == 1 && usable(b));
        F::fail_alloc = 1;  // from empty
        Buf e;
        CHECK(e.grow(8) == hipErrorOutOfMemory && !e && e.capacity() == 0 && F::live == 1);
    }
    CHECK(F::live == 0);

    F::start();
    {  // the free fails: the first error comes back, the buffer is empty, no allocation was tried
        Buf b;
        CHECK(b.grow(16) == hipSuccess);
        F::fail_free = 1;
        F::fail_alloc = 0;
        const int before = F::allocs;
        CHECK(b.grow(32) == hipErrorInvalidValue);
        CHECK(b.get() == nullptr && b.capacity() == 0 && F::allocs == before && F::live == 0);
        CHECK(b.grow(32) == hipSuccess && b.capacity() == 32 && usable(b));
        F::fail_free = 1;
        CHECK(b.reset() == hipErrorInvalidValue && !b && b.capacity() == 0 && F::live == 0);
        CHECK(b.reset() == hipSuccess);
    }
    CHECK(F::live == 0);

    F::start();
    {  // move construction, move assignment over a non-empty target (exactly one free), self-move
        Buf a;
        CHECK(a.grow(5) == hipSuccess);
        uint64_t* const pa = a;
        Buf m(std::move(a));
        CHECK(m.get() == pa && m.capacity() == 5 && a.get() == nullptr && a.capacity() == 0);
        CHECK(F::live == 1 && F::frees == 0);
        Buf t;
        CHECK(t.grow(7) == hipSuccess && F::live == 2);
        const int frees = F::frees;
        t = std::move(m);
        CHECK(F::frees == frees + 1 && F::live == 1);
        CHECK(t.get() == pa && t.capacity() == 5 && m.get() == nullptr && m.capacity() == 0 && usable(t));
        Buf& self = t;
        t = std::move(self);
        CHECK(t.get() == pa && t.capacity() == 5 && F::live == 1 && F::frees == frees + 1 && usable(t));
        Buf empty;
        t = std::move(empty);  // an empty source: the target frees and empties
        CHECK(!t && t.capacity() == 0 && F::live == 0);
    }  // a, m, empty: destruction of moved-from objects frees nothing
    CHECK(F::live == 0 && F::frees == 2);

    F::start();
    {  // reset twice, swap
        Buf a, b;
        CHECK(a.grow(3) == hipSuccess && b.grow(9) == hipSuccess);
        uint64_t *const pa = a, *const pb = b;
        a.swap(b);
        CHECK(a.get() == pb && a.capacity() == 9 && b.get() == pa && b.capacity() == 3 && F::live == 2 && F::frees == 0);
        CHECK(usable(a) && usable(b));
        Buf e;
        e.swap(a);  // the commit of a key install: the new buffer in, the old one out
        CHECK(e.get() == pb && e.capacity() == 9 && !a && a.capacity() == 0);
        CHECK(b.reset() == hipSuccess && !b && b.capacity() == 0 && F::live == 1 && F::frees == 1);
        CHECK(b.reset() == hipSuccess && F::live == 1 && F::frees == 1);
    }
    CHECK(F::live == 0 && F::frees == 2);

    F::start();
    {  // a three-buffer group: the second allocation of a regrowth fails, the next call regrows it whole
        Group g;
        CHECK(g.ensure(8) == hipSuccess && g.cap.get() == 256 && F::live == 3);
        CHECK(g.ensure(200) == hipSuccess && F::allocs == 3);  // inside the floor: nothing moves
        F::fail_alloc = 2;
        CHECK(g.ensure(300) == hipErrorOutOfMemory);
        CHECK(g.cap.get() == 0 && g.a.capacity() == 900 && !g.b && g.b.capacity() == 0 && g.c.capacity() == 256 && F::live == 2);
        CHECK(g.ensure(8) == hipSuccess);  // even a small request: the count says nothing is there
        CHECK(g.cap.get() == 256 && g.a.capacity() == 768 && g.b.capacity() == 768 && g.c.capacity() == 256 && F::live == 3);
        CHECK(usable(g.a) && usable(g.b) && usable(g.c));
        CHECK(g.ensure(300) == hipSuccess && g.cap.get() == 300 && g.c.capacity() == 300 && F::live == 3);
    }
    CHECK(F::live == 0 && F::allocs == F::frees + 1);  // one allocation failed, every other one was freed once

    for (int k = 1; k <= 3; ++k) {  // the k-th allocation of a regrowth fails, for every buffer of both groups
        F::start();
        {
            Group g;
            CHECK(g.ensure(8) == hipSuccess);
            F::fail_alloc = k;
            CHECK(g.ensure(300) == hipErrorOutOfMemory && g.cap.get() == 0 && !g.cap.fits(1) && F::live == 2);
            CHECK(whole_or_empty(g.a, 768, 900) && whole_or_empty(g.b, 768, 900) && whole_or_empty(g.c, 256, 300));
            CHECK(!(k == 1 ? g.a : k == 2 ? g.b : g.c));
            F::sizes.clear();
            CHECK(g.ensure(300) == hipSuccess && g.cap.get() == 300 && F::live == 3);
            CHECK(F::sizes == (std::vector<size_t>{900 * 8, 900 * 8, 300 * 8}));
            CHECK(usable(g.a) && usable(g.b) && usable(g.c));
        }
        CHECK(F::live == 0);
        F::start();
        {
            Rows r;  // n = 16: stride 24; n = 834: stride 840
            CHECK(r.rs.stride() == 0 && r.rs.cap() == 0 && r.rs.rows() == nullptr);
            CHECK(r.ensure(8, 16) == hipSuccess && r.rs.cap() == 256 && r.rs.stride() == 24 && F::live == 3);
            CHECK(F::sizes == (std::vector<size_t>{256 * 24 * 8, 512 * 8, 256 * 8}));
            F::fail_alloc = k;
            CHECK(r.ensure(300, 16) == hipErrorOutOfMemory && r.rs.cap() == 0 && r.rs.stride() == 0 && F::live == 2);
            CHECK(whole_or_empty(r.x, 512, 600) && whole_or_empty(r.y, 256, 300));
            CHECK(k == 1 ? r.rs.rows() == nullptr : !(k == 2 ? r.x : r.y));
            F::sizes.clear();
            CHECK(r.ensure(8, 16) == hipSuccess && r.rs.cap() == 256 && r.rs.stride() == 24 && F::live == 3);
            CHECK(F::sizes == (std::vector<size_t>{256 * 24 * 8, 512 * 8, 256 * 8}));
            CHECK(r.rs.drop() == hipSuccess && r.rs.cap() == 0 && r.rs.stride() == 0 && !r.rs.rows() && F::live == 2);
            F::sizes.clear();  // another dimension after a drop: the stride is the new one's
            CHECK(r.ensure(300, 834) == hipSuccess && r.rs.cap() == 300 && r.rs.stride() == 840);
            CHECK(F::sizes == (std::vector<size_t>{300 * 840 * 8, 600 * 8, 300 * 8}));
            for (size_t i = 0; i < 300 * 840; ++i) r.rs.rows()[i] = i;  // every row is the buffer's to write
        }
        CHECK(F::live == 0);
    }
    return 0;
}

int main() {
    if (checks()) return 1;
    std::printf("DeviceBuf host checks: ok\n");
    return 0;
}
