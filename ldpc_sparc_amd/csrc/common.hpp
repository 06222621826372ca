// Shared host-side plumbing for libldpc_sparc_amd.so: error reporting across
// the C ABI, per-device library streams, checked HIP calls.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>

#include "../../include/ldpc_sparc_amd.h"

namespace sg {

void set_error(const char *fmt, ...);
int fail(int code, const char *fmt, ...);

// Ensures a device is present and selected; returns SG_OK or SG_ERR_NO_DEVICE.
int ensure_device();
hipStream_t lib_stream();
inline hipStream_t pick_stream(void *s) { return s ? reinterpret_cast<hipStream_t>(s) : lib_stream(); }
int device_cu_count();

// Per-phase device timing (sg_profile_enable): HIP events recorded on the
// stream a phase is launched on, resolved by sg_profile_collect.
int prof_begin(int phase, hipStream_t s);
void prof_end(int token, hipStream_t s);
// A decode that runs as two halves on two streams (capi_amp.cpp, pipelined split engine): prof_pipe_begin
// records the base event of the decode on s (before the fork); between prof_pipe_half(h) and prof_pipe_half(-1)
// every scope belongs to half h.  sg_profile_collect pairs the k-th scope of a phase in half 0 with the k-th in
// half 1, counts the pair once, and adds the part of the union of the two intervals (on the base event's time
// line) that no earlier pair of the phase covered, so overlapped time is counted once.
void prof_pipe_begin(hipStream_t s);
void prof_pipe_half(int half);
struct ProfScope {
    int tok;
    hipStream_t s;
    ProfScope(int phase, hipStream_t st) : tok(prof_begin(phase, st)), s(st) {}
    ~ProfScope() { prof_end(tok, s); }
};

// ceil(log2 v): log2 of a power of two (section sizes, transform lengths)
inline int ilog2(int v) {
    int l = 0;
    while ((1 << l) < v) ++l;
    return l;
}

// f(T{}) with T the real type of a precision (SG_F64: double, else float)
template <typename F>
int by_precision(int precision, F &&f) { return precision == SG_F64 ? f(double{}) : f(float{}); }

struct HipError {
    hipError_t err;
    const char *what;
};

}  // namespace sg

#define SG_HIP(call)                                                                        \
    do {                                                                                    \
        hipError_t e_ = (call);                                                             \
        if (e_ != hipSuccess)                                                               \
            return ::sg::fail(e_ == hipErrorOutOfMemory ? SG_ERR_NOMEM : SG_ERR_HIP,        \
                              "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_),        \
                              __FILE__, __LINE__);                                          \
    } while (0)

#define SG_CHECK_ARG(cond, ...)                                                             \
    do {                                                                                    \
        if (!(cond))                                                                        \
            return ::sg::fail(SG_ERR_INVALID, __VA_ARGS__);                                 \
    } while (0)

#define SG_TRY(expr)                                                                        \
    do {                                                                                    \
        int r_ = (expr);                                                                    \
        if (r_ != SG_OK)                                                                    \
            return r_;                                                                      \
    } while (0)

namespace sg {

// Raises kernel fn's dynamic-LDS limit to lds bytes.  *done is the caller's
// record of the limit already set for fn (a static of the launcher, one per
// kernel instance; grow-only); null: set it on every call.
static inline int set_max_lds(const void *fn, size_t lds, size_t *done) {
    if (done && *done >= lds) return SG_OK;
    SG_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    if (done) *done = lds;
    return SG_OK;
}

// The section range and the row length of a soft-output call: sections [l0, l0 + nl) inside [0, L] and rows of at
// least nl * per values (per bits per section, spelled per_name in the refusal).  Argument checks only: the callers
// run it before anything is launched or allocated.
static inline int section_range_check(int L, int l0, int nl, long long llr_ld, int per, const char *per_name) {
    SG_CHECK_ARG(l0 >= 0 && nl >= 0 && l0 <= L && nl <= L - l0, "sections [%d, %d + %d) outside [0, %d]", l0, l0, nl, L);
    SG_CHECK_ARG(llr_ld >= (long long)nl * per, "llr_ld = %lld < nl %s = %lld", llr_ld, per_name, (long long)nl * per);
    return SG_OK;
}

}  // namespace sg
