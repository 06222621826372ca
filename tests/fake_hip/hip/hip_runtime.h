// Host stand-in for <hip/hip_runtime.h>, for tests/device_mem_main.cpp only: what csrc/common.hpp and
// csrc/device_mem.hpp name, over malloc/free, with a live-allocation count and a "fail the k-th hipMalloc" switch.
#pragma once
#include <cstdlib>
#include <cstring>

typedef struct ihipStream_t *hipStream_t;
enum hipError_t { hipSuccess = 0, hipErrorInvalidValue = 1, hipErrorOutOfMemory = 2 };
enum hipMemcpyKind { hipMemcpyHostToDevice = 1 };
enum hipFuncAttribute { hipFuncAttributeMaxDynamicSharedMemorySize = 8 };

inline int fake_live = 0;     // allocations not yet freed
inline int fake_fail_in = 0;  // k > 0: the k-th hipMalloc from now fails with hipErrorOutOfMemory

inline hipError_t hipMalloc(void **p, size_t bytes) {
    *p = nullptr;
    if (fake_fail_in > 0 && --fake_fail_in == 0) return hipErrorOutOfMemory;
    if (bytes == 0) return hipSuccess;
    *p = std::malloc(bytes);
    ++fake_live;
    return hipSuccess;
}
template <class T>
hipError_t hipMalloc(T **p, size_t bytes) { return hipMalloc((void **)p, bytes); }
inline hipError_t hipFree(void *p) {
    if (p) --fake_live;
    std::free(p);
    return hipSuccess;
}
inline hipError_t hipMemcpy(void *dst, const void *src, size_t bytes, hipMemcpyKind) {
    std::memcpy(dst, src, bytes);
    return hipSuccess;
}
inline const char *hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory" : "error"; }
inline hipError_t hipFuncSetAttribute(const void *, hipFuncAttribute, int) { return hipSuccess; }
