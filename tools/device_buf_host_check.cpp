// device_buf_host_check.cpp -- stand-alone driver of DeviceBuf (fhe-sign_amd/csrc/device_buf.h; no GPU call) over
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

// the ensure_* pattern of the context: one count over a group, 0 while the group is touched
struct Group {
    Buf a, b, c;
    size_t cap = 0;
    hipError_t ensure(size_t count) {
        if (count <= cap) return hipSuccess;
        cap = 0;
        const size_t want = count < 256 ? 256 : count;
        hipError_t e;
        if ((e = a.grow(want * 3)) != hipSuccess) return e;
        if ((e = b.grow(want * 3)) != hipSuccess) return e;
        if ((e = c.grow(want)) != hipSuccess) return e;
        cap = want;
        return hipSuccess;
    }
};

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
        CHECK(g.ensure(8) == hipSuccess && g.cap == 256 && F::live == 3);
        CHECK(g.ensure(200) == hipSuccess && F::allocs == 3);  // inside the floor: nothing moves
        F::fail_alloc = 2;
        CHECK(g.ensure(300) == hipErrorOutOfMemory);
        CHECK(g.cap == 0 && g.a.capacity() == 900 && !g.b && g.b.capacity() == 0 && g.c.capacity() == 256 && F::live == 2);
        CHECK(g.ensure(8) == hipSuccess);  // even a small request: the count says nothing is there
        CHECK(g.cap == 256 && g.a.capacity() == 768 && g.b.capacity() == 768 && g.c.capacity() == 256 && F::live == 3);
        CHECK(usable(g.a) && usable(g.b) && usable(g.c));
        CHECK(g.ensure(300) == hipSuccess && g.cap == 300 && g.c.capacity() == 300 && F::live == 3);
    }
    CHECK(F::live == 0 && F::allocs == F::frees + 1);  // one allocation failed, every other one was freed once
    return 0;
}

int main() {
    if (checks()) return 1;
    std::printf("DeviceBuf host checks: ok\n");
    return 0;
}
