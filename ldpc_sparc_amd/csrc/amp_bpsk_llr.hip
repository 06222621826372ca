// Bit LLRs of a section range from the final state of a real K = 2 (BPSK) modulated AMP decode (DESIGN.md "Soft
// output of the K = 2 decoder"): the marginals of the joint posterior over (location j, symbol c = +-1) whose
// mean is the K = 2 denoiser (sparc.py:433-441, bpsk_section_kernel of amp_oploop.hip),
//   p(j, c) = e^{c x_j} / sum_k (e^{x_k} + e^{-x_k}),   x = s / tau,
// from the s that bpsk_section_kernel kept (OpLoopBufs::s_keep, natural order) and the tau of the section's
// column block, then ldpc_bp's clip and log (sparc_new.py:1167-1169).  A section carries log2 M location bits,
// MSB first, then its symbol bit (0: +1), the digits of the word (location << 1) | symbol.
#include "amp_oploop.hpp"
#include "section_bits.hpp"

namespace sg {

// One wavefront per section, four per workgroup (as reg_llr_kernel, amp_llr.hip): lane holds the entries
// j = lane + 64 i, i < V = ceil(M / 64) <= VMAX, read in natural order; lanes >= M idle when M < 64.  With
// a = |x| and m the section's maximum of a, an entry's larger exponential is e^{a - m} and its smaller one
// e^{a - m} e^{-2 a}: nothing overflows.  An entry's weight is the sum of the two, in double; the location bits
// and the tail are section_bits.hpp's, the symbol bit is one more position, the wave sum of the e^{x} terms, and
// the denominator is the wave sum of the lanes' totals.  The output does not depend on the batch.
template <typename T, int VMAX>
__global__ __launch_bounds__(256) void bpsk_llr_kernel(const T *sbuf, const double *taubuf, int L, int M, int Lc,
                                                       int l0, int nl, int logM, int llr_ld, int probs_only, T *llr) {
    const int lane = threadIdx.x & 63;
    const int li = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int cw = blockIdx.y;
    if (li >= nl) return;
    const int l = l0 + li;
    const T tau = (T)taubuf[(size_t)cw * Lc + l / (L / Lc)];  // (as bpsk_section_kernel rounds it)
    const T *s = sbuf + ((size_t)cw * L + l) * M;
    T x[VMAX];
    T m = T(0);
#pragma unroll
    for (int i = 0; i < VMAX; ++i) {
        const int j = lane + 64 * i;
        x[i] = j < M ? s[j] / tau : T(0);  // sparc.py:434
        m = fmax(m, fabs(x[i]));
    }
    m = wave_max(m);
    LaneBits<hi_bits(VMAX)> acc;
    double plus = 0.0;
#pragma unroll
    for (int i = 0; i < VMAX; ++i) {
        const T a = fabs(x[i]);
        const T big = fexp<T>(a - m), small = big * fexp<T>(T(-2) * a);
        const bool in = lane + 64 * i < M;
        plus += in ? (double)(x[i] < T(0) ? small : big) : 0.0;  // e^{x}
        acc.add(i, in ? (double)big + (double)small : 0.0);      // e^{x} + e^{-x}, less the shift
    }
    const double den = wave_sum(acc.tot);
    double out = location_bits(acc, logM, lane);
    plus = wave_sum(plus);
    if (lane == logM) out = plus;  // the symbol bit, after the location bits
    if (lane <= logM)
        llr[(size_t)cw * llr_ld + (size_t)li * (logM + 1) + lane] = bit_out<T>(out / den, probs_only);
}

template <typename T>
int bpsk_launch_llr(const T *s_keep, const double *tau, int B, int L, int M, int Lc, int l0, int nl, int llr_ld,
                    int probs_only, T *llr, hipStream_t st) {
    if (B <= 0 || nl <= 0) return SG_OK;
    if (M < 2 || (M & (M - 1)) != 0 || M > 2048)
        return fail(SG_ERR_UNSUPPORTED, "K = 2 bit LLRs: M = %d is not a power of two in [2, 2048]", M);
    if (B > 65535) return fail(SG_ERR_UNSUPPORTED, "K = 2 bit LLRs of %d codewords (at most 65535)", B);
    SG_TRY(with_vmax(M, [&](auto vmax) {
        hipLaunchKernelGGL((bpsk_llr_kernel<T, decltype(vmax)::value>), dim3((nl + 3) / 4, B), dim3(256), 0, st,
                           s_keep, tau, L, M, Lc, l0, nl, ilog2(M), llr_ld, probs_only, llr);
        return SG_OK;
    }));
    SG_HIP(hipGetLastError());
    return SG_OK;
}

template int bpsk_launch_llr<float>(const float *, const double *, int, int, int, int, int, int, int, int, float *,
                                    hipStream_t);
template int bpsk_launch_llr<double>(const double *, const double *, int, int, int, int, int, int, int, int, double *,
                                     hipStream_t);

}  // namespace sg
