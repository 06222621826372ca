// Bit marginals of a section (DESIGN.md "Bit marginals of a section"): the one core of the soft-output kernels
// (amp_llr.hip, amp_bpsk_llr.hip, integrated_dct.hip, camp_llr.hip and the tail of glue_llr_kernel, dense.hip).
// All __forceinline__; every reduction is a fixed xor butterfly, no atomics: the same bits on every run.
#pragma once
#include <type_traits>

#include "common.hpp"
#include "device_util.hpp"

namespace sg {

// One wavefront holds a section: lane owns the entries j = lane + 64 i.  The six low bits of j are the lane, the
// bits above them are i.  So the weight of "location bit clear" is, for a low bit, a wave sum of the lanes' totals
// over the lanes whose bit is clear, and for a high bit a wave sum of per-lane partial sums over the i whose bit is
// clear.  A kernel that keeps VMAX = 1 / 8 / 32 entries per lane (M <= 64 / 512 / 2048) has 0 / 3 / 5 high bits.
constexpr int hi_bits(int vmax) { return vmax == 32 ? 5 : vmax == 8 ? 3 : 0; }

// A lane's sums of the weights w of its entries, in double: the total and, per high bit h, the part over the
// entries whose bit h of i is clear.  i is unrolled at compile time in the VMAX kernels (static indices into hp).
template <int NH>
struct LaneBits {
    double tot = 0.0, hp[NH > 0 ? NH : 1] = {0.0};
    __device__ __forceinline__ void add(int i, double w) {
        tot += w;
#pragma unroll
        for (int h = 0; h < NH; ++h)
            if (((i >> h) & 1) == 0) hp[h] += w;
    }
};

// Weight of "location bit clear" for the section's log2 M location bits, MSB first: position pos is left on
// lane == pos (0 on the lanes >= logM).  Symbol bits are further positions that the caller reduces with wave_sum
// and leaves on the lanes after these.
template <int NH>
__device__ __forceinline__ double location_bits(const LaneBits<NH> &acc, int logM, int lane) {
    double out = 0.0;
    for (int pos = 0; pos < logM; ++pos) {
        const int bit = logM - 1 - pos;
        double p = ((lane >> bit) & 1) == 0 ? acc.tot : 0.0;
#pragma unroll
        for (int h = 0; h < NH; ++h)
            if (bit == 6 + h) p = acc.hp[h];
        p = wave_sum(p);
        if (lane == pos) out = p;
    }
    return out;
}

// ldpc_bp's clip and log ratio (sparc_new.py:1167-1169) of P(bit = 0), in double: 1 - 1e-15 is not a float
__device__ __forceinline__ double clip_llr(double p) {
    const double eps = 1e-15;
    const double pc = fmin(fmax(p, eps), 1.0 - eps);
    return log(pc) - log(1.0 - pc);
}

// The soft output of one bit.  The LLR is that of the probability as probs_only returns it (rounded to T), so the
// two outputs of one state agree to the rounding of the logs; in float a p within 6e-8 of 1 is 1 and clips.
template <typename T>
__device__ __forceinline__ T bit_llr(T pt) { return (T)clip_llr((double)pt); }
template <typename T>
__device__ __forceinline__ T bit_out(double p, int probs_only) {
    const T pt = (T)p;
    return probs_only ? pt : bit_llr<T>(pt);
}

// f(integral_constant<int, VMAX>) with the entries per lane that hold a section of M: the kernels' instances
template <typename F>
int with_vmax(int M, F &&f) {
    if (M <= 64) return f(std::integral_constant<int, 1>{});
    if (M <= 512) return f(std::integral_constant<int, 8>{});
    if (M <= 2048) return f(std::integral_constant<int, 32>{});
    return fail(SG_ERR_UNSUPPORTED, "bit LLRs of sections of M = %d > 2048 entries", M);
}

}  // namespace sg
