// Host-side owners of device memory: DevMem, one allocation (function-local scratch, grow-only staging), and
// DevPool, the allocations of one owner that live and die together (a plan's tables, a batch workspace).
// Everything outside runtime.cpp's raw allocation entry points allocates and frees through these two.
#pragma once
#include <algorithm>
#include <vector>

#include "common.hpp"

#pragma GCC visibility push(hidden)  // shared between the library's objects, not exported from it
namespace sg {

class DevMem {
    void *p_ = nullptr;
    size_t n_ = 0;

public:
    DevMem() = default;
    DevMem(DevMem &&o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    DevMem &operator=(DevMem &&o) noexcept {
        if (this != &o) {
            reset();
            std::swap(p_, o.p_);
            std::swap(n_, o.n_);
        }
        return *this;
    }
    ~DevMem() { reset(); }

    // Grow-only: a buffer that is large enough stays; else it is freed and exactly `bytes` allocated.  After a
    // failure the object is empty, so the next call tries again.
    int ensure(size_t bytes) {
        if (bytes <= n_) return SG_OK;
        reset();
        void *d = nullptr;
        SG_HIP(hipMalloc(&d, bytes));
        p_ = d;
        n_ = bytes;
        return SG_OK;
    }
    void reset() {
        if (p_) hipFree(p_);
        p_ = nullptr;
        n_ = 0;
    }
    size_t bytes() const { return n_; }
    template <class T = void>
    T *at(size_t byte_off = 0) const { return (T *)((char *)p_ + byte_off); }
};

// Records the addresses of the owner's pointer members (slots): the owner must not move while the pool holds
// any, so a pool never sits in anything a container can relocate.
class DevPool {
    std::vector<void **> slots_;

public:
    DevPool() = default;
    DevPool(const DevPool &) = delete;
    DevPool &operator=(const DevPool &) = delete;
    ~DevPool() { release(); }

    // max(1, bytes) into *slot.  A failure leaves the earlier allocations owned: the next release frees them.
    template <class T>
    int alloc(T **slot, size_t bytes) {
        void *d = nullptr;
        SG_HIP(hipMalloc(&d, std::max<size_t>(1, bytes)));
        *slot = (T *)d;
        slots_.push_back((void **)slot);
        return SG_OK;
    }
    template <class X>
    int upload(X **slot, const std::vector<X> &src) {
        SG_TRY(alloc(slot, src.size() * sizeof(X)));
        if (!src.empty()) SG_HIP(hipMemcpy(*slot, src.data(), src.size() * sizeof(X), hipMemcpyHostToDevice));
        return SG_OK;
    }
    // Frees everything and nulls every slot
    void release() {
        for (void **s : slots_) {
            hipFree(*s);
            *s = nullptr;
        }
        slots_.clear();
    }
};

}  // namespace sg
#pragma GCC visibility pop
