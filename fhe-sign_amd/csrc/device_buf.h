// device_buf.h -- the one owner of device (and pinned host) memory: a pointer and a capacity in elements,
// move-only, freed by its destructor.  Every hipMalloc / hipFree / hipHostMalloc / hipHostFree of csrc/ is in
// this file.  A DeviceBuf never synchronises: the caller waits (on the stream, on an event, or not at all)
// before it lets go of memory that queued work may still touch.  Host-only C++: needs no hipcc.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <utility>

namespace fhe {

struct HipDeviceAlloc {
    static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
    static hipError_t free(void* p) { return hipFree(p); }
};
struct HipPinnedAlloc {
    static hipError_t alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static hipError_t free(void* p) { return hipHostFree(p); }
};

template <class T, class Alloc = HipDeviceAlloc>
class DeviceBuf {
public:
    DeviceBuf() = default;
    DeviceBuf(const DeviceBuf&) = delete;
    DeviceBuf& operator=(const DeviceBuf&) = delete;
    DeviceBuf(DeviceBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) {
        o.p_ = nullptr;
        o.cap_ = 0;
    }
    DeviceBuf& operator=(DeviceBuf&& o) noexcept {
        if (this != &o) {
            (void)reset();
            swap(o);
        }
        return *this;
    }
    ~DeviceBuf() { (void)reset(); }

    T* get() const { return p_; }
    operator T*() const { return p_; }
    size_t capacity() const { return cap_; }  // elements
    bool fits(size_t count) const { return count <= cap_; }
    void swap(DeviceBuf& o) noexcept {
        std::swap(p_, o.p_);
        std::swap(cap_, o.cap_);
    }
    // frees and empties; the free's error, if any
    hipError_t reset() {
        T* const old = p_;
        p_ = nullptr;
        cap_ = 0;
        return old ? Alloc::free(const_cast<void*>(static_cast<const void*>(old))) : hipSuccess;
    }
    // frees what is held, then allocates exactly `count` elements.  On an error of either the buffer is
    // left empty and the first error is returned.
    hipError_t grow(size_t count) {
        hipError_t e = reset();
        if (e != hipSuccess) return e;
        void* q = nullptr;
        e = Alloc::alloc(&q, count * sizeof(T));
        if (e != hipSuccess) return e;
        p_ = static_cast<T*>(q);
        cap_ = count;
        return hipSuccess;
    }

private:
    T* p_ = nullptr;
    size_t cap_ = 0;
};

template <class T>
using PinnedBuf = DeviceBuf<T, HipPinnedAlloc>;

// grow_each(a, na, b, nb, ...): grows each buffer to its count, in order; stops at the first error
inline hipError_t grow_each() { return hipSuccess; }
template <class B, class... Rest>
hipError_t grow_each(B& buf, size_t count, Rest&&... rest) {
    const hipError_t e = buf.grow(count);
    return e != hipSuccess ? e : grow_each(rest...);
}

// The capacity, in items, of a group of buffers that are grown together (a workspace).  It is 0 while any buffer
// of the group is not grown: a regrowth that fails half-way leaves some buffers new, some empty, and the next
// request, however small, regrows them all.  As with a DeviceBuf the caller waits first, when queued work may
// still touch the old buffers.
class GroupCap {
public:
    size_t get() const { return cap_; }
    bool fits(size_t count) const { return count <= cap_; }
    void drop() { cap_ = 0; }
    // regrows the group for max(count, floor) items: grow(cap) grows every buffer of the group for `cap` items
    // (grow_each) and returns the first error
    template <class Grow>
    hipError_t regrow(size_t count, size_t floor, Grow&& grow) {
        cap_ = 0;
        const size_t cap = count < floor ? floor : count;
        const hipError_t e = grow(cap);
        if (e == hipSuccess) cap_ = cap;
        return e;
    }

private:
    size_t cap_ = 0;
};

// Rows of u64 for LWE ciphertexts of one dimension: the buffer, how many rows it holds and the row stride, n + 1
// words rounded up to 64 bytes, that it was grown with.  The stride is 0 whenever the rows are not grown, so a
// stride never outlives the dimension it was derived from.
template <class Alloc = HipDeviceAlloc>
class RowSpaceOf {
public:
    static constexpr size_t kFloor = 256;
    static int stride_of(size_t n) { return (int)((n + 1 + 7) / 8 * 8); }
    uint64_t* rows() const { return rows_; }
    size_t cap() const { return cap_.get(); }
    int stride() const { return stride_; }
    bool fits(size_t count) const { return cap_.fits(count); }
    // at least `count` rows (and kFloor) for dimension n; more(cap) grows what else belongs to the group
    template <class More>
    hipError_t regrow(size_t count, size_t n, More&& more) {
        stride_ = 0;
        const hipError_t e = cap_.regrow(count, kFloor, [&](size_t cap) {
            const hipError_t g = rows_.grow(cap * (size_t)stride_of(n));
            return g != hipSuccess ? g : more(cap);
        });
        if (e == hipSuccess) stride_ = stride_of(n);
        return e;
    }
    hipError_t regrow(size_t count, size_t n) {
        return regrow(count, n, [](size_t) { return hipSuccess; });
    }
    hipError_t drop() {
        cap_.drop();
        stride_ = 0;
        return rows_.reset();
    }

private:
    DeviceBuf<uint64_t, Alloc> rows_;
    GroupCap cap_;
    int stride_ = 0;
};
using RowSpace = RowSpaceOf<>;

}  // namespace fhe
