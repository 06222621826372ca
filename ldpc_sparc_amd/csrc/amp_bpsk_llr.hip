// Bit LLRs of a section range from the final state of a real K = 2 (BPSK) modulated AMP decode (DESIGN.md "Soft
// output of the K = 2 decoder"): the marginals of the joint posterior over (location j, symbol c = +-1) whose
// mean is the K = 2 denoiser (sparc.py:433-441, bpsk_section_kernel of amp_oploop.hip),
//   p(j, c) = e^{c x_j} / sum_k (e^{x_k} + e^{-x_k}),   x = s / tau,
// from the s that bpsk_section_kernel kept (OpLoopBufs::s_keep, natural order) and the tau of the section's
// column block, then ldpc_bp's clip and log (sparc_new.py:1167-1169).  A section carries log2 M location bits,
// MSB first, then its symbol bit (0: +1), the digits of the word (location << 1) | symbol.
#include "amp_oploop.hpp"
#include "device_util.hpp"

namespace sg {

namespace {

template <typename T>
__device__ __forceinline__ T lexp(T x);
template <>
__device__ __forceinline__ float lexp<float>(float x) { return __expf(x); }
template <>
__device__ __forceinline__ double lexp<double>(double x) { return exp(x); }

}  // namespace

// One wavefront per section, four per workgroup (as reg_llr_kernel, amp_llr.hip): lane holds the entries
// j = lane + 64 i, i < V = ceil(M / 64) <= VMAX, read in natural order; lanes >= M idle when M < 64.  With
// a = |x| and m the section's maximum of a, an entry's larger exponential is e^{a - m} and its smaller one
// e^{a - m} e^{-2 a}: nothing overflows.  The six low bits of j are the lane, the high bits are i, so the bit-0
// weight of a low location bit is a wave sum of the lanes' totals over the lanes whose bit is clear, that of a high
// bit a wave sum of per-lane partial sums over the i whose bit is clear, and that of the symbol bit a wave sum of
// the e^{x} terms.  The weights and their sums are double, the denominator is the wave sum of the lanes' totals,
// and the clip and the logs are double (1 - 1e-15 is not a float).  Fixed butterfly reductions, no atomics: the
// output is the same bits on every run and does not depend on the batch.
template <typename T, int VMAX>
__global__ __launch_bounds__(256) void bpsk_llr_kernel(const T *sbuf, const double *taubuf, int L, int M, int Lc,
                                                       int l0, int nl, int logM, int llr_ld, int probs_only, T *llr) {
    constexpr int NH = VMAX == 32 ? 5 : VMAX == 8 ? 3 : 0;  // index bits above the lane bits
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
    double tot = 0.0, plus = 0.0, hp[NH > 0 ? NH : 1] = {0.0};
#pragma unroll
    for (int i = 0; i < VMAX; ++i) {
        const T a = fabs(x[i]);
        const T big = lexp<T>(a - m), small = big * lexp<T>(T(-2) * a);
        const bool in = lane + 64 * i < M;
        const double w = in ? (double)big + (double)small : 0.0;       // e^{x} + e^{-x}, less the shift
        plus += in ? (double)(x[i] < T(0) ? small : big) : 0.0;       // e^{x}
        tot += w;
#pragma unroll
        for (int h = 0; h < NH; ++h)
            if (((i >> h) & 1) == 0) hp[h] += w;
    }
    const double den = wave_sum(tot);
    double out = 0.0;
    for (int pos = 0; pos <= logM; ++pos) {
        const int bit = logM - 1 - pos;  // location bits MSB first; pos = logM: the symbol bit
        double p = pos == logM ? plus : ((lane >> bit) & 1) == 0 ? tot : 0.0;
#pragma unroll
        for (int h = 0; h < NH; ++h)
            if (bit == 6 + h) p = hp[h];
        p = wave_sum(p);
        if (lane == pos) out = p / den;
    }
    if (lane <= logM) {
        // the LLR is that of the probability as probs_only returns it (rounded to T), so the two outputs of one
        // state agree to the rounding of the logs (DESIGN.md "Soft output of the DCT engines", one contract)
        const T pt = (T)out;
        const double eps = 1e-15;
        const double pc = fmin(fmax((double)pt, eps), 1.0 - eps);  // ldpc_bp's clip (sparc_new.py:1167)
        llr[(size_t)cw * llr_ld + (size_t)li * (logM + 1) + lane] = probs_only ? pt : (T)(log(pc) - log(1.0 - pc));
    }
}

template <typename T>
int bpsk_launch_llr(const T *s_keep, const double *tau, int B, int L, int M, int Lc, int l0, int nl, int llr_ld,
                    int probs_only, T *llr, hipStream_t st) {
    if (B <= 0 || nl <= 0) return SG_OK;
    if (M < 2 || (M & (M - 1)) != 0 || M > 2048)
        return fail(SG_ERR_UNSUPPORTED, "K = 2 bit LLRs: M = %d is not a power of two in [2, 2048]", M);
    if (B > 65535) return fail(SG_ERR_UNSUPPORTED, "K = 2 bit LLRs of %d codewords (at most 65535)", B);
    const int logM = ilog2(M);
    const dim3 grid((nl + 3) / 4, B), block(256);
    if (M <= 64)
        hipLaunchKernelGGL((bpsk_llr_kernel<T, 1>), grid, block, 0, st, s_keep, tau, L, M, Lc, l0, nl, logM, llr_ld,
                           probs_only, llr);
    else if (M <= 512)
        hipLaunchKernelGGL((bpsk_llr_kernel<T, 8>), grid, block, 0, st, s_keep, tau, L, M, Lc, l0, nl, logM, llr_ld,
                           probs_only, llr);
    else
        hipLaunchKernelGGL((bpsk_llr_kernel<T, 32>), grid, block, 0, st, s_keep, tau, L, M, Lc, l0, nl, logM, llr_ld,
                           probs_only, llr);
    SG_HIP(hipGetLastError());
    return SG_OK;
}

template int bpsk_launch_llr<float>(const float *, const double *, int, int, int, int, int, int, int, int, float *,
                                    hipStream_t);
template int bpsk_launch_llr<double>(const double *, const double *, int, int, int, int, int, int, int, int, double *,
                                     hipStream_t);

}  // namespace sg
