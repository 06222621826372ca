// Device-resident Monte-Carlo campaign of the complex AMP engine: the kernels
// around the decoder of amp_cfft.hip that keep a campaign on the GPU.
//
//   bits -> (location, constellation index) per section
//       (sparc.py:330-364 bin_arr_2_msg_vector: log2 M MSB-first location
//       bits, then log2 K Gray-coded K-PSK bits)
//   scatter of the one-hot K-PSK message vector beta0 into the plan's beta
//       workspace (the encoder is then the engine's own A beta)
//   error counters of calc_ler_ver / calc_ber (sparc_sim.py) from the MAP and
//       the transmitted (location, constellation index) pairs.
#include <algorithm>

#include "camp_section.hpp"

namespace sg {
namespace {

__global__ __launch_bounds__(256) void bits_to_psk_sections_kernel(const uint8_t *__restrict__ bits, int L, int logM,
                                                                   int logK, int32_t *__restrict__ idx,
                                                                   int32_t *__restrict__ sym) {
    const int b = blockIdx.y, per = logM + logK;
    for (int l = blockIdx.x * blockDim.x + threadIdx.x; l < L; l += gridDim.x * blockDim.x) {
        const uint8_t *x = bits + ((size_t)b * L + l) * per;
        int v = 0, g = 0;
        for (int j = 0; j < logM; ++j) v = (v << 1) | (x[j] & 1);
        for (int j = 0; j < logK; ++j) g = (g << 1) | (x[logM + j] & 1);
        idx[(size_t)b * L + l] = v;
        if (sym) sym[(size_t)b * L + l] = gray_to_bin(g);
    }
}

// beta0 (zeroed by the caller): constel[sym] (1 for K = 1) at entry idx of
// every section.  A location or a constellation index outside its range
// writes nothing.  Also marks the codeword active for the FFT passes.
__global__ __launch_bounds__(256) void camp_scatter_kernel(int L, int M, int K, const cxd *__restrict__ constel,
                                                           const int32_t *__restrict__ idx,
                                                           const int32_t *__restrict__ sym, cxd *__restrict__ beta,
                                                           int32_t *__restrict__ active) {
    const int b = blockIdx.y;
    if (blockIdx.x == 0 && threadIdx.x == 0) active[b] = 1;
    for (int l = blockIdx.x * blockDim.x + threadIdx.x; l < L; l += gridDim.x * blockDim.x) {
        const int i = idx[(size_t)b * L + l];
        if (i < 0 || i >= M) continue;
        cxd v{1.0, 0.0};
        if (K > 1) {
            const int k = sym[(size_t)b * L + l];
            if (k < 0 || k >= K) continue;
            v = constel[k];
        }
        beta[((size_t)b * L + l) * M + i] = v;
    }
}

// One workgroup per codeword.  counts += {section, location, value, bit,
// codeword errors, t_final}; rows[cw] = {bit, section, location, value errors}.
__global__ __launch_bounds__(256) void camp_count_kernel(const int32_t *__restrict__ map_idx,
                                                         const int32_t *__restrict__ map_sym,
                                                         const int32_t *__restrict__ true_idx,
                                                         const int32_t *__restrict__ true_sym,
                                                         const int32_t *__restrict__ t_final, int L, int logM, int logK,
                                                         unsigned long long *counts, int32_t *rows) {
    __shared__ int red[4][4];
    const int cw = blockIdx.x;
    const unsigned mM = (1u << logM) - 1u, mK = (1u << logK) - 1u;
    const bool psk = logK > 0 && map_sym && true_sym;
    int v[4] = {0, 0, 0, 0};  // section, location, value, bit errors
    for (int l = threadIdx.x; l < L; l += blockDim.x) {
        const size_t o = (size_t)cw * L + l;
        const int a = map_idx[o], b = true_idx[o];
        const int sa = psk ? map_sym[o] : 0, sb = psk ? true_sym[o] : 0;
        const int loc = a != b, val = sa != sb;
        v[0] += loc | val;
        v[1] += loc;
        v[2] += val;
        v[3] += __popc((unsigned)(a ^ b) & mM) + __popc((unsigned)(bin_to_gray(sa) ^ bin_to_gray(sb)) & mK);
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        for (int o = 32; o > 0; o >>= 1) v[q] += __shfl_xor(v[q], o, 64);
        if (lane == 0) red[q][wid] = v[q];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int t[4];
        for (int q = 0; q < 4; ++q) t[q] = red[q][0] + red[q][1] + red[q][2] + red[q][3];
        atomicAdd(&counts[0], (unsigned long long)t[0]);
        atomicAdd(&counts[1], (unsigned long long)t[1]);
        atomicAdd(&counts[2], (unsigned long long)t[2]);
        atomicAdd(&counts[3], (unsigned long long)t[3]);
        atomicAdd(&counts[4], (unsigned long long)(t[3] > 0));
        atomicAdd(&counts[5], (unsigned long long)t_final[cw]);
        if (rows) {
            rows[(size_t)cw * 4 + 0] = t[3];
            rows[(size_t)cw * 4 + 1] = t[0];
            rows[(size_t)cw * 4 + 2] = t[1];
            rows[(size_t)cw * 4 + 3] = t[2];
        }
    }
}

unsigned grid_of(int items) { return (unsigned)std::max(1, std::min(1024, (items + 255) / 256)); }

}  // namespace

int camp_launch_bits_to_psk(const uint8_t *bits, int B, int L, int logM, int logK, int32_t *idx, int32_t *sym,
                            hipStream_t s) {
    if (B <= 0 || L <= 0) return SG_OK;
    hipLaunchKernelGGL(bits_to_psk_sections_kernel, dim3(grid_of(L), B), dim3(256), 0, s, bits, L, logM, logK, idx, sym);
    SG_HIP(hipGetLastError());
    return SG_OK;
}

int camp_launch_scatter(const CampTables &tb, const CampBufs &bf, const int32_t *idx, const int32_t *sym,
                        hipStream_t s) {
    if (bf.B <= 0) return SG_OK;
    SG_HIP(hipMemsetAsync(bf.beta, 0, (size_t)bf.B * tb.LM * sizeof(cxd), s));
    hipLaunchKernelGGL(camp_scatter_kernel, dim3(grid_of(tb.L), bf.B), dim3(256), 0, s, tb.L, tb.M, bf.K, bf.constel,
                       idx, sym, bf.beta, bf.active);
    SG_HIP(hipGetLastError());
    return SG_OK;
}

int camp_launch_count(const int32_t *map_idx, const int32_t *map_sym, const int32_t *true_idx, const int32_t *true_sym,
                      const int32_t *t_final, int B, int L, int logM, int logK, int64_t *counts, int32_t *rows,
                      hipStream_t s) {
    if (B <= 0) return SG_OK;
    hipLaunchKernelGGL(camp_count_kernel, dim3(B), dim3(256), 0, s, map_idx, map_sym, true_idx, true_sym, t_final, L,
                       logM, logK, reinterpret_cast<unsigned long long *>(counts), rows);
    SG_HIP(hipGetLastError());
    return SG_OK;
}

}  // namespace sg
