// Bit LLRs of a section range from the final state of a regular-engine AMP
// decode (DESIGN.md "Soft output of the DCT engines"): the glue of
// beta_estimate_to_bp_probs (sparc_new.py:1118-1138) and the clip / log of
// ldpc_bp (:1167-1169), computed from s in class order and the per-codeword
// tau instead of a natural-order beta that the regular engines never store.
#include "amp.hpp"

namespace sg {

// One wavefront per section (as eta_kernel, amp_dct.hip): lane holds the
// entries j = lane + 64 i, i < V = ceil(M / 64) <= VMAX, gathered through
// qpos; lanes >= M idle when M < 64.  The six low bits of j are the lane, the
// high bits are i, so the bit-0 marginal of a low bit is a wave sum of the
// lanes' totals over the lanes whose bit is clear, and that of a high bit a
// wave sum of per-lane partial sums over the i whose bit is clear.  Sums of
// beta accumulate in double and the clip and the logs are double, as in
// glue_llr_kernel (dense.hip): 1 - 1e-15 is not a float.  Fixed butterfly
// reductions, no atomics: the output is the same bits on every run.
template <typename T, int VMAX>
__global__ __launch_bounds__(256) void reg_llr_kernel(RegTables<T> tb, const T *sbuf, const double *taubuf, int l0,
                                                      int nl, int logM, int llr_ld, int probs_only, T *llr) {
    constexpr int NH = VMAX == 32 ? 5 : VMAX == 8 ? 3 : 0;  // index bits above the lane bits
    const int lane = threadIdx.x & 63;
    const int li = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int cw = blockIdx.y;
    if (li >= nl) return;
    const int l = l0 + li, c = l / tb.Lblk, M = tb.M;
    const double tv = taubuf[(size_t)cw * tb.Lc + c];
    const T tau = (T)tv, inv_tau = (T)(1.0 / tv);
    const int32_t *qp = tb.qpos + (size_t)c * tb.Mc + (size_t)(l - c * tb.Lblk) * M;
    const T *s = sbuf + (size_t)cw * tb.LM + (size_t)c * tb.Mc;
    T v[VMAX];
    T m = -INFINITY;
#pragma unroll
    for (int i = 0; i < VMAX; ++i) {
        const int j = lane + 64 * i;
        v[i] = j < M ? s[qp[j]] : T(-INFINITY);
        m = fmax(m, v[i]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
    // x = s / tau less the section's own maximum (f64: the quotients' difference, as sm_arg of amp_fused.hip)
    T den = T(0);
#pragma unroll
    for (int i = 0; i < VMAX; ++i) {
        if (lane + 64 * i < M) {
            if constexpr (sizeof(T) == 8) v[i] = exp(v[i] / tau - m / tau);
            else v[i] = __expf((v[i] - m) * inv_tau);
            den += v[i];
        } else {
            v[i] = T(0);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) den += __shfl_xor(den, o, 64);
    double tot = 0.0, hp[NH > 0 ? NH : 1] = {0.0};
#pragma unroll
    for (int i = 0; i < VMAX; ++i) {
        const double b = (double)(v[i] / den);  // beta of entry lane + 64 i (0 past M)
        tot += b;
#pragma unroll
        for (int h = 0; h < NH; ++h)
            if (((i >> h) & 1) == 0) hp[h] += b;
    }
    double out = 0.0;
    for (int pos = 0; pos < logM; ++pos) {
        const int bit = logM - 1 - pos;  // MSB first
        double p = ((lane >> bit) & 1) == 0 ? tot : 0.0;
#pragma unroll
        for (int h = 0; h < NH; ++h)
            if (bit == 6 + h) p = hp[h];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) p += __shfl_xor(p, o, 64);
        if (lane == pos) out = p;
    }
    if (lane < logM) {
        // the LLR is that of the probability as probs_only returns it (rounded to T), so the two outputs of one
        // state agree to the rounding of the logs; in float a p within 6e-8 of 1 is 1 and clips to 1 - 1e-15
        const T pt = (T)out;
        const double eps = 1e-15;
        const double pc = fmin(fmax((double)pt, eps), 1.0 - eps);  // ldpc_bp's clip (sparc_new.py:1167)
        llr[(size_t)cw * llr_ld + (size_t)li * logM + lane] = probs_only ? pt : (T)(log(pc) - log(1.0 - pc));
    }
}

// s [B][LM] in class order and tau [B][Lc] as the decode left them; the caller has checked the section range,
// llr_ld >= nl log2 M and M a power of two in [2, 2048]
template <typename T>
int reg_launch_llr(const RegTables<T> &tb, const T *s, const double *tau, int B, int l0, int nl, int llr_ld,
                   int probs_only, T *llr, hipStream_t st) {
    if (B <= 0 || nl <= 0) return SG_OK;
    const int logM = ilog2(tb.M);
    const dim3 grid((nl + 3) / 4, B), block(256);
    if (tb.M <= 64)
        hipLaunchKernelGGL((reg_llr_kernel<T, 1>), grid, block, 0, st, tb, s, tau, l0, nl, logM, llr_ld, probs_only, llr);
    else if (tb.M <= 512)
        hipLaunchKernelGGL((reg_llr_kernel<T, 8>), grid, block, 0, st, tb, s, tau, l0, nl, logM, llr_ld, probs_only, llr);
    else if (tb.M <= 2048)
        hipLaunchKernelGGL((reg_llr_kernel<T, 32>), grid, block, 0, st, tb, s, tau, l0, nl, logM, llr_ld, probs_only, llr);
    else
        return fail(SG_ERR_UNSUPPORTED, "bit LLRs of sections of M = %d > 2048 entries", tb.M);
    SG_HIP(hipGetLastError());
    return SG_OK;
}

template int reg_launch_llr<float>(const RegTables<float> &, const float *, const double *, int, int, int, int, int,
                                   float *, hipStream_t);
template int reg_launch_llr<double>(const RegTables<double> &, const double *, const double *, int, int, int, int, int,
                                    double *, hipStream_t);

}  // namespace sg
