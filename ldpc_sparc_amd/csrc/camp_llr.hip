// Soft output of the complex AMP engine (DESIGN.md "Soft output of the complex
// engine") and the small kernels a concatenated K-PSK SPARC + LDPC campaign
// needs around it (section bits, section words and back), double precision.
//
// For K >= 2 the engine's final beta is the conditional mean sum_k p(j,k) c_k,
// not a posterior, so the bit marginals come from the joint posterior over
// (location j, symbol k) of the last effective observation s (kept by camp_eta
// in CampBufs::s_keep) and its tau:
//   p(j,k) ~ exp(Re(x_j conj c_k)),  x = s / (tau / 2)   (sparc.py:402-465)
// A section carries log2 M MSB-first location bits, then log2 K Gray-coded
// symbol bits (msg_vector_2_bin_arr, sparc.py:366-400); P(bit = 0) is the sum
// of p over the (j, k) whose bit is clear.  The clip and the log are ldpc_bp's
// (sparc_new.py:1167-1169).
#include <algorithm>

#include "camp_section.hpp"
#include "section_bits.hpp"

namespace sg {
namespace {

constexpr int LLR_SYM = 6;  // symbol bits (K <= 64)

// exponent argument of (entry x, symbol k): Re x for K = 1, else Re(x conj c_k).  The host's constellation is
// exact for K = 2 and K = 4, so this one form equals the specialised ones of psk_terms (camp_section.hpp).
__device__ __forceinline__ double llr_arg(int K, const cxd *__restrict__ c, cxd x, int k) {
    return K == 1 ? x.x : x.x * c[k].x + x.y * c[k].y;
}

// One wavefront per section, lane owns entries e = lane, lane + 64, ...  Unlike the VMAX kernels of the real
// engines this one makes two passes over the section (the maximum, then the accumulation) and keeps no per-entry
// register array: K exponentials per entry would not fit one, and every M up to 2048 runs in the same few
// registers.  An entry's weight is its sum over the symbols; the location bits and the tail are
// section_bits.hpp's (all five high bits, index e >> 6), the symbol bits are log2 K more positions: per lane the
// sums over the k whose Gray code has the bit clear, then a wave sum each.
// s [B][LM] natural order; tau [B][Lc] (x = s / (tau / 2)) or null (x = s).
__global__ __launch_bounds__(256) void camp_llr_kernel(const cxd *__restrict__ sbuf, const double *__restrict__ taubuf,
                                                       int L, int Lc, int M, int K, const cxd *__restrict__ cs, int l0,
                                                       int nl, int logM, int logK, int llr_ld, int probs_only,
                                                       double *__restrict__ llr) {
    const int lane = threadIdx.x & 63;
    const int li = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int cw = blockIdx.y;
    if (li >= nl) return;
    const int l = l0 + li;
    const double th = taubuf ? taubuf[(size_t)cw * Lc + l / (L / Lc)] / 2 : 1.0;  // s is complex: sparc.py:417-418
    const cxd *s = sbuf + ((size_t)cw * L + l) * M;
    double m = -INFINITY;
    for (int e = lane; e < M; e += 64) {
        const cxd x{s[e].x / th, s[e].y / th};
        for (int k = 0; k < K; ++k) m = fmax(m, llr_arg(K, cs, x, k));
    }
    m = wave_max(m);
    LaneBits<hi_bits(32)> acc;
    double sp[LLR_SYM] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int e = lane; e < M; e += 64) {
        const cxd x{s[e].x / th, s[e].y / th};
        double we = 0.0;
        for (int k = 0; k < K; ++k) {
            const double w = exp(llr_arg(K, cs, x, k) - m);
            const int g = bin_to_gray(k);
            we += w;
#pragma unroll
            for (int i = 0; i < LLR_SYM; ++i)
                if (i < logK && ((g >> (logK - 1 - i)) & 1) == 0) sp[i] += w;  // MSB first
        }
        acc.add(e >> 6, we);
    }
    const double total = wave_sum(acc.tot);
    double out = location_bits(acc, logM, lane);
#pragma unroll
    for (int i = 0; i < LLR_SYM; ++i) {
        if (i < logK) {
            const double p = wave_sum(sp[i]);
            if (lane == logM + i) out = p;
        }
    }
    if (lane < logM + logK)
        llr[(size_t)cw * llr_ld + (size_t)li * (logM + logK) + lane] = bit_out<double>(out / total, probs_only);
}

// bits_to_psk_sections_kernel (camp_campaign.hip) with row strides: codeword b's bits at bits + b * bit_stride,
// its L locations / constellation indices at idx / sym + b * idx_stride
__global__ __launch_bounds__(256) void bits_to_psk_strided_kernel(const uint8_t *__restrict__ bits, size_t bit_stride,
                                                                  int L, int logM, int logK, int32_t *__restrict__ idx,
                                                                  int32_t *__restrict__ sym, size_t idx_stride) {
    const int b = blockIdx.y, per = logM + logK;
    for (int l = blockIdx.x * blockDim.x + threadIdx.x; l < L; l += gridDim.x * blockDim.x) {
        const uint8_t *x = bits + (size_t)b * bit_stride + (size_t)l * per;
        int v = 0, g = 0;
        for (int j = 0; j < logM; ++j) v = (v << 1) | (x[j] & 1);
        for (int j = 0; j < logK; ++j) g = (g << 1) | (x[logM + j] & 1);
        idx[(size_t)b * idx_stride + l] = v;
        if (sym) sym[(size_t)b * idx_stride + l] = gray_to_bin(g);
    }
}

// word = idx << logK | bin2gray(sym): the section's message bits as one integer
__global__ __launch_bounds__(256) void psk_pack_kernel(const int32_t *__restrict__ idx, const int32_t *__restrict__ sym,
                                                       size_t total, int logK, int32_t *__restrict__ word) {
    const unsigned mK = (1u << logK) - 1u;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const unsigned g = sym ? (unsigned)bin_to_gray(sym[i]) & mK : 0u;
        word[i] = (int32_t)(((unsigned)idx[i] << logK) | g);
    }
}

// word -> (idx, sym), the inverse of psk_pack_kernel; a negative word is "unknown": idx = -1, sym = 0
__global__ __launch_bounds__(256) void psk_unpack_kernel(const int32_t *__restrict__ word, size_t total, int logK,
                                                         int32_t *__restrict__ idx, int32_t *__restrict__ sym) {
    const int mK = (1 << logK) - 1;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int w = word[i];
        idx[i] = w < 0 ? -1 : w >> logK;
        if (sym) sym[i] = w < 0 ? 0 : gray_to_bin(w & mK);
    }
}

unsigned grid_of(size_t items) { return (unsigned)std::max<size_t>(1, std::min<size_t>(1024, (items + 255) / 256)); }

}  // namespace

// s [B][L*M] natural order and tau [B][Lc] (or null: s is already x) on the device; the caller has checked the
// section range, llr_ld >= nl (log2 M + log2 K), K a power of two <= CAMP_MAX_K and M a power of two >= 2
int camp_launch_llr(const cxd *s, const double *tau, int B, int L, int Lc, int M, int K, const cxd *constel, int l0,
                    int nl, int llr_ld, int probs_only, double *llr, hipStream_t st) {
    if (M > 2048) return fail(SG_ERR_UNSUPPORTED, "bit LLRs of sections of M = %d > 2048 entries", M);
    if (B <= 0 || nl <= 0) return SG_OK;
    hipLaunchKernelGGL(camp_llr_kernel, dim3((nl + 3) / 4, B), dim3(256), 0, st, s, tau, L, Lc, M, K, constel, l0, nl,
                       ilog2(M), ilog2(K), llr_ld, probs_only, llr);
    SG_HIP(hipGetLastError());
    return SG_OK;
}

int camp_launch_bits_to_psk_strided(const uint8_t *bits, size_t bit_stride, int B, int L, int logM, int logK,
                                    int32_t *idx, int32_t *sym, size_t idx_stride, hipStream_t s) {
    if (B <= 0 || L <= 0) return SG_OK;
    hipLaunchKernelGGL(bits_to_psk_strided_kernel, dim3(grid_of((size_t)L), B), dim3(256), 0, s, bits, bit_stride, L,
                       logM, logK, idx, sym, idx_stride);
    SG_HIP(hipGetLastError());
    return SG_OK;
}

int camp_launch_pack(const int32_t *idx, const int32_t *sym, int B, int L, int logK, int32_t *word, hipStream_t s) {
    const size_t total = (size_t)B * L;
    if (total == 0) return SG_OK;
    hipLaunchKernelGGL(psk_pack_kernel, dim3(grid_of(total)), dim3(256), 0, s, idx, sym, total, logK, word);
    SG_HIP(hipGetLastError());
    return SG_OK;
}

int camp_launch_unpack(const int32_t *word, int B, int L, int logK, int32_t *idx, int32_t *sym, hipStream_t s) {
    const size_t total = (size_t)B * L;
    if (total == 0) return SG_OK;
    hipLaunchKernelGGL(psk_unpack_kernel, dim3(grid_of(total)), dim3(256), 0, s, word, total, logK, idx, sym);
    SG_HIP(hipGetLastError());
    return SG_OK;
}

}  // namespace sg
