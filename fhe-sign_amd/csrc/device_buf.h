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

}  // namespace fhe
