// Real K = 2 (BPSK) modulated AMP (sg_amp_decode_bpsk_device, capi_amp.cpp): the kernels between the plan's
// operators Ab / Az on natural-order vectors, as amp_partial.hip has them for the known-sections decoder.
//
// The loop is sparc_amp (sparc.py:883-999) with K = 2 for W of ndim 0, 1 or 2: the unmodulated loop with the
// denoiser of sparc.py:433-441 and the final decision of sparc.py:488-492.
//
//   bpsk_init_kernel      psi0 = 1, gamma0_r = sum_c W_rc / Lc, nmse = 1
//   bpsk_residual_kernel  z <- y - Ab(beta) + b_r z (t = 0: y - Ab(0)) and partial sums of z^2 per row block
//   bpsk_control_kernel   phase 0: phi_r (:949-955), tau_c (:958-969), zs = z / phi_r
//                         phase 1: psi, the NMSE row, the stop decision (:976-988), then gamma_r and
//                         b_r = gamma_r / phi_r of the next iteration (:936-942)
//   bpsk_section_kernel   s = beta + tau u (:972), beta = eta(s / tau), sum beta^2, the squared error against the
//                         true word's +-1 one-hot, the word (location << 1) | symbol of the first maximum of |s|
//
// The denoiser, with x = s / tau, a = |x| and m the section's maximum of a:
//   beta_j = sign(x_j) e^{a_j - m} q_j / sum_k e^{a_k - m} (2 - q_k),   q = -expm1(-2 a) = 1 - e^{-2 a},
// which is (e^{x_j} - e^{-x_j}) / sum_k (e^{x_k} + e^{-x_k}) without the cancellation at small |x| (2 - q is
// 1 + e^{-2 a} from the one expm1).
//
// A codeword that stopped is skipped by every kernel, so it keeps its state.  Fixed-order reductions, no atomics:
// a codeword's result does not depend on the batch it is decoded in.
#include "amp_bpsk.hpp"
#include "device_util.hpp"

namespace sg {

namespace {

constexpr int QB = 256;  // block size of the residual, control and init kernels

template <typename T>
__device__ __forceinline__ T qexp(T x);
template <>
__device__ __forceinline__ float qexp<float>(float x) { return __expf(x); }
template <>
__device__ __forceinline__ double qexp<double>(double x) { return exp(x); }
template <typename T>
__device__ __forceinline__ T qexpm1(T x);
template <>
__device__ __forceinline__ float qexpm1<float>(float x) { return expm1f(x); }
template <>
__device__ __forceinline__ double qexpm1<double>(double x) { return expm1(x); }

// gamma_r = dot(W_r, psi) / Lc (sparc.py:936-939; W psi for the one entry of a flat design)
__device__ __forceinline__ double gamma_row(const double *W, const double *psi, int r, int Lc) {
    double acc = 0.0;
    for (int c = 0; c < Lc; ++c) acc += W[(size_t)r * Lc + c] * psi[c];
    return acc / Lc;
}

}  // namespace

// One workgroup per codeword.  beta was zeroed by the caller.
template <typename T>
__global__ __launch_bounds__(QB) void bpsk_init_kernel(BpskBufs<T> bb) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int Lr = bb.Lr, Lc = bb.Lc;
    double *psi = bb.psi + (size_t)b * Lc;
    double *nmse = bb.nmse + (size_t)b * bb.t_max * Lc;
    for (int i = tid; i < bb.t_max * Lc; i += QB) nmse[i] = 1.0;
    for (int c = tid; c < Lc; c += QB) psi[c] = 1.0;
    __syncthreads();
    for (int r = tid; r < Lr; r += QB) {
        bb.gamma[(size_t)b * Lr + r] = gamma_row(bb.W, psi, r, Lc);
        bb.bco[(size_t)b * Lr + r] = 0.0;
    }
    if (tid == 0) {
        bb.active[b] = 1;
        bb.t_final[b] = 0;
    }
}

// np workgroups per row block and codeword, each striding over the row block's Mr entries from its own offset.
template <typename T>
__global__ __launch_bounds__(QB) void bpsk_residual_kernel(BpskBufs<T> bb, int t) {
    __shared__ double red[QB / 64];
    const int r = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
    if (!bb.active[b]) return;
    const size_t o = (size_t)b * bb.n + (size_t)r * bb.Mr;
    const T bc = (T)bb.bco[(size_t)b * bb.Lr + r];
    double zz = 0.0;
    for (int i = blockIdx.x * QB + tid; i < bb.Mr; i += bb.np * QB) {
        T zn = bb.y[o + i] - bb.r[o + i];
        if (t > 0) zn += bc * bb.z[o + i];
        bb.z[o + i] = zn;
        zz += (double)zn * (double)zn;
    }
    zz = block_sum<QB / 64>(zz, red);
    if (tid == 0) bb.zz[((size_t)b * bb.Lr + r) * bb.np + blockIdx.x] = zz;
}

// One workgroup per codeword, in double.
template <typename T>
__global__ __launch_bounds__(QB) void bpsk_control_kernel(BpskBufs<T> bb, int phase, int t) {
    __shared__ double red[QB / 64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    if (!bb.active[b]) return;
    const int L = bb.L, Lr = bb.Lr, Lc = bb.Lc, Mr = bb.Mr;
    double *psi = bb.psi + (size_t)b * Lc, *psi_prev = bb.psi_prev + (size_t)b * Lc;
    double *phi = bb.phi + (size_t)b * Lr, *gamma = bb.gamma + (size_t)b * Lr;
    if (phase == 0) {
        for (int r = tid; r < Lr; r += QB) {
            if (bb.phi_method == 1) {
                phi[r] = bb.awgn_var + gamma[r];
            } else {
                double acc = 0.0;
                for (int q = 0; q < bb.np; ++q) acc += bb.zz[((size_t)b * Lr + r) * bb.np + q];
                phi[r] = acc / Mr;
            }
        }
        __syncthreads();
        for (int c = tid; c < Lc; c += QB) {
            double tau;
            if (bb.ndim < 2) {
                tau = (L * phi[0] / bb.n) / bb.W[c];
            } else {
                double acc = 0.0;
                for (int r = 0; r < Lr; ++r) acc += bb.W[(size_t)r * Lc + c] * (1.0 / phi[r]);
                tau = ((double)L / Mr) / acc;
            }
            bb.tau[(size_t)b * Lc + c] = tau;
        }
        for (int r = 0; r < Lr; ++r) {
            const size_t o = (size_t)b * bb.n + (size_t)r * Mr;
            const T ph = (T)phi[r];
            for (int i = tid; i < Mr; i += QB) bb.zs[o + i] = bb.z[o + i] / ph;
        }
        return;
    }
    const int spc = L / Lc;
    const double denom = (double)spc;
    double *nmse = bb.nmse + (size_t)b * bb.t_max * Lc;
    const double *bsq = bb.bsq + (size_t)b * L, *err = bb.err + (size_t)b * L;
    if (Lc > 1) {  // one wavefront per column block
        for (int c = tid >> 6; c < Lc; c += QB / 64) {
            double a = 0.0, e = 0.0;
            for (int l = c * spc + lane; l < (c + 1) * spc; l += 64) {
                a += bsq[l];
                e += err[l];
            }
            a = wave_sum(a);
            e = wave_sum(e);
            if (lane == 0) {
                psi[c] = 1.0 - a / denom;
                nmse[(size_t)(t + 1) * Lc + c] = e / denom;
            }
        }
    } else {
        double a = 0.0, e = 0.0;
        for (int l = tid; l < L; l += QB) {
            a += bsq[l];
            e += err[l];
        }
        a = block_sum<QB / 64>(a, red);
        e = block_sum<QB / 64>(e, red);
        if (tid == 0) {
            psi[0] = 1.0 - a / denom;
            nmse[t + 1] = e / denom;
        }
    }
    __syncthreads();
    if (tid != 0) return;
    bool stop = false;
    if (t > 0) {
        stop = true;
        for (int c = 0; c < Lc; ++c)
            if (!(fabs(psi[c] - psi_prev[c]) <= bb.atol + bb.rtol * fabs(psi_prev[c]))) stop = false;
    }
    if (stop) {  // nmse[t:] = nmse[t]
        for (int tt = t + 1; tt < bb.t_max; ++tt)
            for (int c = 0; c < Lc; ++c) nmse[(size_t)tt * Lc + c] = nmse[(size_t)t * Lc + c];
        bb.t_final[b] = t + 1;
        bb.active[b] = 0;
    } else if (t == bb.t_max - 2) {
        bb.t_final[b] = t + 1;
        bb.active[b] = 0;
    } else {  // the next iteration's psi_prev, gamma and b = gamma / phi_prev
        for (int c = 0; c < Lc; ++c) psi_prev[c] = psi[c];
        for (int r = 0; r < Lr; ++r) {
            const double g = gamma_row(bb.W, psi, r, Lc);
            gamma[r] = g;
            bb.bco[(size_t)b * Lr + r] = g / phi[r];
        }
    }
}

// One wavefront per section, four per workgroup: lane holds the entries j = lane + 64 i, i < VMAX; lanes >= M idle
// when M < 64.
template <typename T, int VMAX>
__global__ __launch_bounds__(256) void bpsk_section_kernel(BpskBufs<T> bb) {
    const int lane = threadIdx.x & 63;
    const int l = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int b = blockIdx.y;
    const int L = bb.L, M = bb.M;
    if (l >= L || !bb.active[b]) return;
    const size_t sl = (size_t)b * L + l;
    const int truth = bb.true_word ? bb.true_word[sl] : -1;
    const int tloc = truth >= 0 ? truth >> 1 : -1;
    const T tval = (truth & 1) ? T(-1) : T(1);
    const T tau = (T)bb.tau[(size_t)b * bb.Lc + l / (L / bb.Lc)];
    const size_t o = sl * M;
    T x[VMAX];
    T amax = T(-1), xm = T(0);
    int word = 0x7fffffff;
#pragma unroll
    for (int i = 0; i < VMAX; ++i) {
        const int j = lane + 64 * i;
        if (j < M) {
            const T s = bb.beta[o + j] + tau * bb.u[o + j];  // sparc.py:972
            x[i] = s / tau;                                  // sparc.py:434
            xm = fmax(xm, fabs(x[i]));
            if (fabs(s) > amax) { amax = fabs(s); word = (j << 1) | (s < T(0) ? 1 : 0); }
        } else {
            x[i] = T(0);
        }
    }
    xm = wave_max(xm);
    const T gmax = wave_max(amax);
    const int cand = wave_min(amax == gmax ? word : 0x7fffffff);  // the first location attaining the maximum
    T den = T(0);
#pragma unroll
    for (int i = 0; i < VMAX; ++i) {
        const T a = fabs(x[i]);
        const T e = qexp<T>(a - xm), q = -qexpm1<T>(T(-2) * a);
        den += lane + 64 * i < M ? e * (T(2) - q) : T(0);
        x[i] = copysign(e * q, x[i]);
    }
    den = wave_sum(den);
    double ss = 0.0, se = 0.0;
#pragma unroll
    for (int i = 0; i < VMAX; ++i) {
        const int j = lane + 64 * i;
        if (j < M) {
            const T v = x[i] / den;
            bb.beta[o + j] = v;
            ss += (double)v * (double)v;
            const double d = (double)(v - (j == tloc ? tval : T(0)));
            se += d * d;
        }
    }
    ss = wave_sum(ss);
    se = wave_sum(se);
    if (lane == 0) {
        bb.bsq[sl] = ss;
        bb.err[sl] = se;
        bb.map[sl] = cand;
    }
}

template <typename T>
int bpsk_launch_init(const BpskBufs<T> &bb, hipStream_t s) {
    ProfScope ps(SG_PH_CONTROL, s);
    hipLaunchKernelGGL((bpsk_init_kernel<T>), dim3(bb.B), dim3(QB), 0, s, bb);
    SG_HIP(hipGetLastError());
    return SG_OK;
}

template <typename T>
int bpsk_launch_residual(const BpskBufs<T> &bb, int t, hipStream_t s) {
    if (bb.Lr > 65535 || bb.B > 65535)
        return fail(SG_ERR_UNSUPPORTED, "K = 2 residual kernel: %d row blocks, %d codewords (at most 65535 each)",
                    bb.Lr, bb.B);
    ProfScope ps(SG_PH_CONTROL, s);
    hipLaunchKernelGGL((bpsk_residual_kernel<T>), dim3(bb.np, bb.Lr, bb.B), dim3(QB), 0, s, bb, t);
    SG_HIP(hipGetLastError());
    return SG_OK;
}

template <typename T>
int bpsk_launch_control(const BpskBufs<T> &bb, int phase, int t, hipStream_t s) {
    ProfScope ps(SG_PH_CONTROL, s);
    hipLaunchKernelGGL((bpsk_control_kernel<T>), dim3(bb.B), dim3(QB), 0, s, bb, phase, t);
    SG_HIP(hipGetLastError());
    return SG_OK;
}

template <typename T>
int bpsk_launch_section(const BpskBufs<T> &bb, hipStream_t s) {
    const int M = bb.M;
    if (M < 2 || (M & (M - 1)) != 0 || M > 2048)
        return fail(SG_ERR_UNSUPPORTED, "K = 2 section kernel: M = %d is not a power of two in [2, 2048]", M);
    ProfScope ps(SG_PH_ETA, s);
    const dim3 grid((bb.L + 3) / 4, bb.B), block(256);
    if (M <= 64) hipLaunchKernelGGL((bpsk_section_kernel<T, 1>), grid, block, 0, s, bb);
    else if (M <= 512) hipLaunchKernelGGL((bpsk_section_kernel<T, 8>), grid, block, 0, s, bb);
    else hipLaunchKernelGGL((bpsk_section_kernel<T, 32>), grid, block, 0, s, bb);
    SG_HIP(hipGetLastError());
    return SG_OK;
}

#define SG_BPSK_INST(T)                                                          \
    template int bpsk_launch_init<T>(const BpskBufs<T> &, hipStream_t);          \
    template int bpsk_launch_residual<T>(const BpskBufs<T> &, int, hipStream_t); \
    template int bpsk_launch_control<T>(const BpskBufs<T> &, int, int, hipStream_t); \
    template int bpsk_launch_section<T>(const BpskBufs<T> &, hipStream_t);
SG_BPSK_INST(float)
SG_BPSK_INST(double)
#undef SG_BPSK_INST

}  // namespace sg
