// AMP <-> BP integrated decoders on the sub-sampled DCT design (sg_amp_integrated_decode, capi_amp.cpp): the
// two kernels between the plan's operators and the design-agnostic BP -> beta side of integrated.hip.
//
// The loop is oracle/integrated_ref.decode with A beta -> Ab(beta) / snp and A^T z -> Az(z) / snp,
// snp = sqrt(n P / L): the flat operator's columns are snp times unit-norm columns.  beta stays in the fork's
// scale (nonzero value snp).  All vectors are in natural order.
//
//   idct_residual_kernel   z <- y - xhat / snp + c_b z, tau^2_b = ||z||^2 / n   (sparc_new.py:975-990, :490, :693)
//   idct_section_kernel    s = beta + u / snp, weighted alpha = snp softmax(snp s / tau^2), the bit-0 marginals
//                          vk0 of the section's log2 M bits and their LLRs (eta :709-735, ldpc_bp :1167-1169):
//                          one pass for the dense loop's dense_launch_eta, glue_launch_llr, integ_launch_llr
// Fixed-order reductions, no atomics: the same bits on every run.
#include "dense.hpp"
#include "section_bits.hpp"

namespace sg {

namespace {

constexpr int RB = 256;  // block size of the residual kernel

}  // namespace

// One workgroup per codeword, striding over n.  ons_mode 0 (naive decoders): c_b = (P - ||beta||^2 / n) /
// tau^2_prev with ||beta||^2 the fixed-order sum of sec_bsq[b][.]; 1 (integrated): (z / n) ons[b]; 2 (integrated,
// posteriors): z (ons[b] / n) -- the forms of dense.hip residual_kernel.  t = 0: z = y.  tau^2 in double, each
// thread's strided partial sum first, then the block's fixed-order reduction; written to tau[b] (read by the
// section kernel and by the next iteration's deta / residual) and, when tau_hist is given, to tau_hist[b][t].
template <typename T>
__global__ __launch_bounds__(RB) void idct_residual_kernel(const T *y, const T *xhat, T *z, int n, int L, double snp,
                                                           double P, int ons_mode, const double *ons,
                                                           const double *sec_bsq, int t, double *tau,
                                                           double *tau_hist, int t_max) {
    __shared__ double red[RB / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const size_t o = (size_t)b * n;
    const T inv_snp = (T)(1.0 / snp);
    double bsq = 0.0;
    if (t > 0 && ons_mode == 0) {
        double v = 0.0;
        for (int l = tid; l < L; l += RB) v += sec_bsq[(size_t)b * L + l];
        bsq = block_sum<RB / 64>(v, red);
    }
    double zz = 0.0;
    for (int i = tid; i < n; i += RB) {
        T zn = y[o + i];
        if (t > 0) {
            const T zo = z[o + i];
            T on;
            if (ons_mode == 1) on = (zo / (T)n) * (T)ons[b];
            else if (ons_mode == 2) on = zo * (T)(ons[b] / n);
            else on = (zo / (T)tau[b]) * (T)(P - bsq / n);
            zn = (zn - xhat[o + i] * inv_snp) + on;
        }
        z[o + i] = zn;
        zz += (double)zn * (double)zn;
    }
    zz = block_sum<RB / 64>(zz, red);  // (its barriers: every thread has read tau[b] before thread 0 writes it)
    if (tid == 0) {
        const double t2 = zz / n;
        tau[b] = t2;
        if (tau_hist) tau_hist[(size_t)b * t_max + t] = t2;
    }
}

// One wavefront per section, four per workgroup (the shape of reg_llr_kernel, amp_llr.hip, on natural-order
// data): lane holds the entries j = lane + 64 i, i < VMAX; lanes >= M idle when M < 64.  ua holds u = Az(z) on
// entry and the weighted alpha on return (each lane rewrites the entries it read).  vk0 is the bit-0 marginal of
// alpha as stored in T and llr its LLR (section_bits.hpp).
template <typename T, int VMAX>
__global__ __launch_bounds__(256) void idct_section_kernel(T *ua, const T *beta, const double *tau, int L, int M,
                                                           int logM, double snp, T *vk0, T *llr) {
    const int lane = threadIdx.x & 63;
    const int l = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int b = blockIdx.y;
    if (l >= L) return;
    const T c = (T)snp, tau2 = (T)tau[b];
    const size_t o = ((size_t)b * L + l) * M;
    T v[VMAX];
    T m = -INFINITY;
#pragma unroll
    for (int i = 0; i < VMAX; ++i) {
        const int j = lane + 64 * i;
        v[i] = j < M ? c * ((beta[o + j] + ua[o + j] / c) / tau2) : T(-INFINITY);
        m = fmax(m, v[i]);
    }
    m = wave_max(m);
    T den = T(0);
#pragma unroll
    for (int i = 0; i < VMAX; ++i) {
        v[i] = lane + 64 * i < M ? fexp<T>(v[i] - m) : T(0);
        den += v[i];
    }
    den = wave_sum(den);
    LaneBits<hi_bits(VMAX)> acc;
#pragma unroll
    for (int i = 0; i < VMAX; ++i) {
        const int j = lane + 64 * i;
        const T a = v[i] / den;  // alpha of entry j (0 past M)
        if (j < M) ua[o + j] = c * a;
        acc.add(i, (double)a);
    }
    const double out = location_bits(acc, logM, lane);
    if (lane < logM) {
        const size_t k = ((size_t)b * L + l) * logM + lane;
        const T pt = (T)out;
        vk0[k] = pt;
        llr[k] = bit_llr<T>(pt);
    }
}

// app LLRs -> P(bit = 0) = exp(app) / (1 + exp(app)) (ldpc_bp, sparc_new.py:1190) written as 1 / (1 + exp(-app)):
// the same value, and finite for every app.  probs_from_app_kernel (integrated.hip) forms exp(app) first, which in
// single precision is inf from app = 88.8 on and gives inf / inf; the LLRs of this loop's section kernel reach
// +-34.5 per bit (the clip of clip_llr, section_bits.hpp), so a few BP iterations pass that.
template <typename T>
__global__ __launch_bounds__(256) void idct_probs_kernel(const T *app, size_t nn, T *p) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < nn; i += (size_t)gridDim.x * blockDim.x)
        p[i] = T(1) / (T(1) + fexp<T>(-app[i]));
}

// every codeword active and phi = 1: what the general engine's operator kernels read (apply_impl uploads them)
__global__ void idct_ones_kernel(int32_t *active, int B, double *phi, int nphi) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < max(B, nphi); i += gridDim.x * blockDim.x) {
        if (i < B) active[i] = 1;
        if (i < nphi) phi[i] = 1.0;
    }
}

template <typename T>
int idct_launch_residual(const T *y, const T *xhat, T *z, int B, int n, int L, double snp, double P, int ons_mode,
                         const double *ons, const double *sec_bsq, int t, double *tau, double *tau_hist, int t_max,
                         hipStream_t s) {
    ProfScope ps(SG_PH_CONTROL, s);
    hipLaunchKernelGGL((idct_residual_kernel<T>), dim3(B), dim3(RB), 0, s, y, xhat, z, n, L, snp, P, ons_mode, ons,
                       sec_bsq, t, tau, tau_hist, t_max);
    SG_HIP(hipGetLastError());
    return SG_OK;
}

// M a power of two in [2, 2048] (checked by the caller before anything is launched)
template <typename T>
int idct_launch_section(T *ua, const T *beta, const double *tau, int B, int L, int M, double snp, T *vk0, T *llr,
                        hipStream_t s) {
    const int logM = ilog2(M);
    if (M < 2 || (1 << logM) != M || M > 2048)
        return fail(SG_ERR_UNSUPPORTED, "integrated section kernel: M = %d is not a power of two in [2, 2048]", M);
    ProfScope ps(SG_PH_ETA, s);
    SG_TRY(with_vmax(M, [&](auto vmax) {
        hipLaunchKernelGGL((idct_section_kernel<T, decltype(vmax)::value>), dim3((L + 3) / 4, B), dim3(256), 0, s, ua,
                           beta, tau, L, M, logM, snp, vk0, llr);
        return SG_OK;
    }));
    SG_HIP(hipGetLastError());
    return SG_OK;
}

template <typename T>
int idct_launch_probs(const T *app, size_t nn, T *p, hipStream_t s) {
    if (nn == 0) return SG_OK;
    const size_t blocks = (nn + 255) / 256;
    hipLaunchKernelGGL((idct_probs_kernel<T>), dim3((unsigned)(blocks < 65535 ? blocks : 65535)), dim3(256), 0, s, app,
                       nn, p);
    SG_HIP(hipGetLastError());
    return SG_OK;
}

int idct_launch_ones(int32_t *active, int B, double *phi, int nphi, hipStream_t s) {
    hipLaunchKernelGGL(idct_ones_kernel, dim3(64), dim3(256), 0, s, active, B, phi, nphi);
    SG_HIP(hipGetLastError());
    return SG_OK;
}

#define SG_IDCT_INST(T)                                                                                          \
    template int idct_launch_residual<T>(const T *, const T *, T *, int, int, int, double, double, int,          \
                                         const double *, const double *, int, double *, double *, int,           \
                                         hipStream_t);                                                           \
    template int idct_launch_probs<T>(const T *, size_t, T *, hipStream_t);                                      \
    template int idct_launch_section<T>(T *, const T *, const double *, int, int, int, double, T *, T *, hipStream_t);
SG_IDCT_INST(float)
SG_IDCT_INST(double)
#undef SG_IDCT_INST

}  // namespace sg
