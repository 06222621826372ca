// Device helpers shared by the kernels: the exponential of the real type,
// 64-lane butterfly reductions, the fixed-order workgroup sum, raw-buffer
// resources with their typed loads and stores, the lane-half swap.  All __forceinline__ and free of tuning: the
// kernels compile to the same code as with a private copy.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace sg {

// ---- the exponential of the kernels' real type: the fast intrinsic in single
// precision, the library function in double
template <typename T>
__device__ __forceinline__ T fexp(T x);
template <>
__device__ __forceinline__ float fexp<float>(float x) { return __expf(x); }
template <>
__device__ __forceinline__ double fexp<double>(double x) { return exp(x); }

// ---- one wavefront (64 lanes): every lane gets the result.  (Kernels that
// spell the butterfly out in place keep it: replaced by a call, the same
// instructions come out in another order.)
template <typename T>
__device__ __forceinline__ T wave_max(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}

// ---- one workgroup: wave sums, two barriers, then the waves' sums added in
// wave order by every thread (deterministic).  red: one double per wave.  The
// wave count from blockDim.x, or at compile time (NW).
__device__ __forceinline__ double block_sum(double v, double *red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if (lane == 0) red[wid] = v;
    __syncthreads();
    double t = 0.0;
    for (int w = 0; w < nw; ++w) t += red[w];
    return t;
}
template <int NW>
__device__ __forceinline__ double block_sum(double v, double *red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[wid] = v;
    __syncthreads();
    double t = 0.0;
    for (int w = 0; w < NW; ++w) t += red[w];
    return t;
}

// The thread index as a value the compiler cannot see through: the FFT's LDS
// addresses are then recomputed inside the loop over a column's transforms
// (or a codeword's classes) instead of being hoisted out of it and held (and
// spilled) across the loop.
__device__ __forceinline__ int opaque(int v) {
    asm volatile("" : "+v"(v));
    return v;
}

// ---- raw buffer resources: loads and stores address by a per-lane byte
// offset (vo) plus a scalar one (so), with no 64-bit address arithmetic on
// the vector ALUs, and the hardware range check (offset >= bytes) returns 0
// for loads and drops stores -- ragged ends need no clamps or branches.
// Vector-memory operations complete in order (vmcnt): request a load before
// the stores it should not wait for.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const void *p, int bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), 0, bytes > 0 ? bytes : 0, 0x00020000);
}
// workgroup-uniform values (class bounds) in scalar registers: a buffer
// resource built from them stays scalar (no waterfall loop)
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

typedef double d2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float buf_ldf(__amdgpu_buffer_rsrc_t r, int vo, int so) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, vo, so, 0));
}
__device__ __forceinline__ uint32_t buf_ldu(__amdgpu_buffer_rsrc_t r, int vo, int so) {
    return __builtin_amdgcn_raw_buffer_load_b32(r, vo, so, 0);
}
__device__ __forceinline__ double buf_ldd(__amdgpu_buffer_rsrc_t r, int vo, int so) {
    return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, vo, so, 0));
}
__device__ __forceinline__ d2 buf_ld2(__amdgpu_buffer_rsrc_t r, int vo, int so) {
    return __builtin_bit_cast(d2, __builtin_amdgcn_raw_buffer_load_b128(r, vo, so, 0));
}
__device__ __forceinline__ void buf_std(__amdgpu_buffer_rsrc_t r, double v, int vo, int so) {
    typedef uint32_t u2 __attribute__((ext_vector_type(2)));
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u2, v), r, vo, so, 0);
}

// lanes 32..63 of a <-> lanes 0..31 of b, every 32-bit word of T
// (v_permlane32_swap, no LDS)
template <typename T>
__device__ __forceinline__ void swap32(T &a, T &b) {
    typedef uint32_t words __attribute__((ext_vector_type(sizeof(T) / 4)));
    words ua = __builtin_bit_cast(words, a), ub = __builtin_bit_cast(words, b);
#pragma unroll
    for (int c = 0; c < (int)(sizeof(T) / 4); ++c) {
        const auto r = __builtin_amdgcn_permlane32_swap(ua[c], ub[c], false, false);
        ua[c] = r[0];
        ub[c] = r[1];
    }
    a = __builtin_bit_cast(T, ua);
    b = __builtin_bit_cast(T, ub);
}

}  // namespace sg
