// Bit LLRs of a section range from the final state of a regular-engine AMP
// decode (DESIGN.md "Soft output of the DCT engines"): the glue of
// beta_estimate_to_bp_probs (sparc_new.py:1118-1138) and the clip / log of
// ldpc_bp (:1167-1169), computed from s in class order and the per-codeword
// tau instead of a natural-order beta that the regular engines never store.
#include "amp.hpp"
#include "section_bits.hpp"

namespace sg {

// One wavefront per section (as eta_kernel, amp_dct.hip), four per workgroup: lane holds the entries
// j = lane + 64 i, i < V = ceil(M / 64) <= VMAX, gathered through qpos; lanes >= M idle when M < 64.  beta is the
// section's softmax in T; its bit marginals and the tail are section_bits.hpp's.
template <typename T, int VMAX>
__global__ __launch_bounds__(256) void reg_llr_kernel(RegTables<T> tb, const T *sbuf, const double *taubuf, int l0,
                                                      int nl, int logM, int llr_ld, int probs_only, T *llr) {
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
    m = wave_max(m);
    // x = s / tau less the section's own maximum.  The two precisions differ on purpose, as the engines' own
    // softmax does (sm_arg, amp_fused.hip): f64 takes the difference of the quotients like the reference
    // (sparc.py:430-431), f32 multiplies the difference by 1 / tau.
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
    den = wave_sum(den);
    LaneBits<hi_bits(VMAX)> acc;
#pragma unroll
    for (int i = 0; i < VMAX; ++i) acc.add(i, (double)(v[i] / den));  // beta of entry lane + 64 i (0 past M)
    const double out = location_bits(acc, logM, lane);
    if (lane < logM) llr[(size_t)cw * llr_ld + (size_t)li * logM + lane] = bit_out<T>(out, probs_only);
}

// s [B][LM] in class order and tau [B][Lc] as the decode left them; the caller has checked the section range,
// llr_ld >= nl log2 M and M a power of two >= 2 (M > 2048: refused here)
template <typename T>
int reg_launch_llr(const RegTables<T> &tb, const T *s, const double *tau, int B, int l0, int nl, int llr_ld,
                   int probs_only, T *llr, hipStream_t st) {
    if (B <= 0 || nl <= 0) return SG_OK;
    SG_TRY(with_vmax(tb.M, [&](auto vmax) {
        hipLaunchKernelGGL((reg_llr_kernel<T, decltype(vmax)::value>), dim3((nl + 3) / 4, B), dim3(256), 0, st, tb, s,
                           tau, l0, nl, ilog2(tb.M), llr_ld, probs_only, llr);
        return SG_OK;
    }));
    SG_HIP(hipGetLastError());
    return SG_OK;
}

template int reg_launch_llr<float>(const RegTables<float> &, const float *, const double *, int, int, int, int, int,
                                   float *, hipStream_t);
template int reg_launch_llr<double>(const RegTables<double> &, const double *, const double *, int, int, int, int, int,
                                    double *, hipStream_t);

}  // namespace sg
