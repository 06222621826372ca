// The operator-loop AMP decoder (oploop_impl, capi_amp.cpp): the kernels between the plan's operators Ab / Az on
// natural-order vectors, and the BP -> known-sections glue of the three-stage concatenated decoder.
//
// The loop is sparc_amp (sparc.py:883-999) for W of ndim 0, 1 or 2 (phi, gamma and b per row block).  Two
// families run it and differ in the section kernel alone (SectionRule):
//   Known  AMP with known sections (sg_amp_decode_partial_device): the denoiser of a known section is the one-hot
//          of its index, and the loop starts from beta0 = the known one-hots and z0 = y - Ab(beta0)
//   Bpsk   real K = 2 modulated AMP (sg_amp_decode_bpsk_device): the denoiser of sparc.py:433-441 and the final
//          decision of sparc.py:488-492; with OpLoopBufs::known (sg_amp_decode_bpsk_partial_device) the denoiser of
//          a known section is the +-1 one-hot of its word (location << 1) | symbol, and the loop starts from those
//
//   oploop_init_kernel      nmse = 1, psi0 = 1 or, with known sections, beta0 (the rule's one-hots: the rule is a
//                           kernel argument) and psi0_c = the share of unknown sections of column block c;
//                           gamma0_r = sum_c W_rc psi0_c / Lc
//   oploop_residual_kernel  z <- y - Ab(beta) + b_r z (t = 0: y - Ab(beta0)) and partial sums of z^2 per row block
//   oploop_control_kernel   phase 0: phi_r (:949-955), tau_c (:958-969), zs = z / phi_r
//                           phase 1: psi, the NMSE row, the stop decision (:976-988), then gamma_r and
//                           b_r = gamma_r / phi_r of the next iteration (:936-942)
//   known_section_kernel    s = beta + tau u (:972), beta = softmax(s / tau) or the one-hot, sum beta^2, the squared
//                           error against the true index, the first-maximum argmax of s (:997) or the known index
//   bpsk_section_kernel     s = beta + tau u, beta = eta(s / tau), sum beta^2, the squared error against the true
//                           word's +-1 one-hot, the word (location << 1) | symbol of the first maximum of |s|; with
//                           OpLoopBufs::s_keep it also stores s (the soft output's input, amp_bpsk_llr.hip); a known
//                           section keeps the +-1 one-hot of its word and reports that word (s_keep not written)
//   known_sections_kernel   hard decisions of a BP output -> section indices, -1 where a block did not converge
//
// The K = 2 denoiser, with x = s / tau, a = |x| and m the section's maximum of a:
//   beta_j = sign(x_j) e^{a_j - m} q_j / sum_k e^{a_k - m} (2 - q_k),   q = -expm1(-2 a) = 1 - e^{-2 a},
// which is (e^{x_j} - e^{-x_j}) / sum_k (e^{x_k} + e^{-x_k}) without the cancellation at small |x| (2 - q is
// 1 + e^{-2 a} from the one expm1).
//
// A codeword that stopped is skipped by every kernel, so it keeps its state.  Fixed-order reductions, no atomics:
// a codeword's result does not depend on the batch it is decoded in.
#include "amp_oploop.hpp"
#include "device_util.hpp"

namespace sg {

namespace {

constexpr int OB = 256;  // block size of the residual, control and init kernels

template <typename T>
__device__ __forceinline__ T oexpm1(T x);
template <>
__device__ __forceinline__ float oexpm1<float>(float x) { return expm1f(x); }
template <>
__device__ __forceinline__ double oexpm1<double>(double x) { return expm1(x); }

// gamma_r = dot(W_r, psi) / Lc (sparc.py:936-939; W psi for the one entry of a flat design)
__device__ __forceinline__ double gamma_row(const double *W, const double *psi, int r, int Lc) {
    double acc = 0.0;
    for (int c = 0; c < Lc; ++c) acc += W[(size_t)r * Lc + c] * psi[c];
    return acc / Lc;
}

}  // namespace

// One workgroup per codeword.  beta was zeroed by the caller.  A known entry is an index in [0, M) (rule Known)
// or a word in [0, 2M) (rule Bpsk: +1 for symbol 0, -1 for symbol 1 at the word's location).
template <typename T>
__global__ __launch_bounds__(OB) void oploop_init_kernel(OpLoopBufs<T> ob, SectionRule rule) {
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int L = ob.L, Lr = ob.Lr, Lc = ob.Lc, spc = L / Lc;
    const bool words = rule == SectionRule::Bpsk;
    const int kend = words ? 2 * ob.M : ob.M;  // known: an entry in [0, kend)
    double *psi = ob.psi + (size_t)b * Lc;
    double *nmse = ob.nmse + (size_t)b * ob.t_max * Lc;
    for (int i = tid; i < ob.t_max * Lc; i += OB) nmse[i] = 1.0;
    if (ob.known) {
        const int32_t *known = ob.known + (size_t)b * L;
        for (int l = tid; l < L; l += OB) {
            const int k = known[l];
            if (k >= 0 && k < kend) {
                const size_t at = (size_t)b * ob.LM + (size_t)l * ob.M + (words ? k >> 1 : k);
                ob.beta[at] = (words && (k & 1)) ? T(-1) : T(1);
            }
        }
        for (int c = tid >> 6; c < Lc; c += OB / 64) {  // one wavefront per column block
            double unk = 0.0;
            for (int l = c * spc + lane; l < (c + 1) * spc; l += 64) {
                const int k = known[l];
                unk += (k >= 0 && k < kend) ? 0.0 : 1.0;
            }
            unk = wave_sum(unk);
            if (lane == 0) psi[c] = unk / spc;
        }
    } else {
        for (int c = tid; c < Lc; c += OB) psi[c] = 1.0;
    }
    __syncthreads();
    for (int r = tid; r < Lr; r += OB) {
        ob.gamma[(size_t)b * Lr + r] = gamma_row(ob.W, psi, r, Lc);
        ob.bco[(size_t)b * Lr + r] = 0.0;
    }
    if (tid == 0) {
        ob.active[b] = 1;
        ob.t_final[b] = 0;
    }
}

// np workgroups per row block and codeword, each striding over the row block's Mr entries from its own offset.
template <typename T>
__global__ __launch_bounds__(OB) void oploop_residual_kernel(OpLoopBufs<T> ob, int t) {
    __shared__ double red[OB / 64];
    const int r = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
    if (!ob.active[b]) return;
    const size_t o = (size_t)b * ob.n + (size_t)r * ob.Mr;
    const T bc = (T)ob.bco[(size_t)b * ob.Lr + r];
    double zz = 0.0;
    for (int i = blockIdx.x * OB + tid; i < ob.Mr; i += ob.np * OB) {
        T zn = ob.y[o + i] - ob.r[o + i];
        if (t > 0) zn += bc * ob.z[o + i];
        ob.z[o + i] = zn;
        zz += (double)zn * (double)zn;
    }
    zz = block_sum<OB / 64>(zz, red);
    if (tid == 0) ob.zz[((size_t)b * ob.Lr + r) * ob.np + blockIdx.x] = zz;
}

// One workgroup per codeword, in double.
template <typename T>
__global__ __launch_bounds__(OB) void oploop_control_kernel(OpLoopBufs<T> ob, int phase, int t) {
    __shared__ double red[OB / 64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    if (!ob.active[b]) return;
    const int L = ob.L, Lr = ob.Lr, Lc = ob.Lc, Mr = ob.Mr;
    double *psi = ob.psi + (size_t)b * Lc, *psi_prev = ob.psi_prev + (size_t)b * Lc;
    double *phi = ob.phi + (size_t)b * Lr, *gamma = ob.gamma + (size_t)b * Lr;
    if (phase == 0) {
        for (int r = tid; r < Lr; r += OB) {
            if (ob.phi_method == 1) {
                phi[r] = ob.awgn_var + gamma[r];
            } else {
                double acc = 0.0;
                for (int q = 0; q < ob.np; ++q) acc += ob.zz[((size_t)b * Lr + r) * ob.np + q];
                phi[r] = acc / Mr;
            }
        }
        __syncthreads();
        for (int c = tid; c < Lc; c += OB) {
            double tau;
            if (ob.ndim < 2) {
                tau = (L * phi[0] / ob.n) / ob.W[c];
            } else {
                double acc = 0.0;
                for (int r = 0; r < Lr; ++r) acc += ob.W[(size_t)r * Lc + c] * (1.0 / phi[r]);
                tau = ((double)L / Mr) / acc;
            }
            ob.tau[(size_t)b * Lc + c] = tau;
        }
        for (int r = 0; r < Lr; ++r) {
            const size_t o = (size_t)b * ob.n + (size_t)r * Mr;
            const T ph = (T)phi[r];
            for (int i = tid; i < Mr; i += OB) ob.zs[o + i] = ob.z[o + i] / ph;
        }
        return;
    }
    const int spc = L / Lc;
    const double denom = (double)spc;
    double *nmse = ob.nmse + (size_t)b * ob.t_max * Lc;
    const double *bsq = ob.bsq + (size_t)b * L, *err = ob.err + (size_t)b * L;
    if (Lc > 1) {  // one wavefront per column block
        for (int c = tid >> 6; c < Lc; c += OB / 64) {
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
        for (int l = tid; l < L; l += OB) {
            a += bsq[l];
            e += err[l];
        }
        a = block_sum<OB / 64>(a, red);
        e = block_sum<OB / 64>(e, red);
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
            if (!(fabs(psi[c] - psi_prev[c]) <= ob.atol + ob.rtol * fabs(psi_prev[c]))) stop = false;
    }
    if (stop) {  // nmse[t:] = nmse[t]
        for (int tt = t + 1; tt < ob.t_max; ++tt)
            for (int c = 0; c < Lc; ++c) nmse[(size_t)tt * Lc + c] = nmse[(size_t)t * Lc + c];
        ob.t_final[b] = t + 1;
        ob.active[b] = 0;
    } else if (t == ob.t_max - 2) {
        ob.t_final[b] = t + 1;
        ob.active[b] = 0;
    } else {  // the next iteration's psi_prev, gamma and b = gamma / phi_prev
        for (int c = 0; c < Lc; ++c) psi_prev[c] = psi[c];
        for (int r = 0; r < Lr; ++r) {
            const double g = gamma_row(ob.W, psi, r, Lc);
            gamma[r] = g;
            ob.bco[(size_t)b * Lr + r] = g / phi[r];
        }
    }
}

// The section kernels: one wavefront per section, four per workgroup: lane holds the entries j = lane + 64 i,
// i < VMAX; lanes >= M idle when M < 64.

// SectionRule::Known.  The softmax is shifted by the section's maximum of s / tau.
template <typename T, int VMAX>
__global__ __launch_bounds__(256) void known_section_kernel(OpLoopBufs<T> ob) {
    const int lane = threadIdx.x & 63;
    const int l = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int b = blockIdx.y;
    const int L = ob.L, M = ob.M;
    if (l >= L || !ob.active[b]) return;
    const size_t sl = (size_t)b * L + l;
    const int k = ob.known[sl];
    const int truth = ob.truth ? ob.truth[sl] : -1;
    if (k >= 0 && k < M) {  // known: beta stays the one-hot that oploop_init_kernel wrote
        if (lane == 0) {
            ob.bsq[sl] = 1.0;
            ob.err[sl] = k == truth ? 0.0 : (truth >= 0 && truth < M ? 2.0 : 1.0);
            ob.map[sl] = k;
        }
        return;
    }
    const T tau = (T)ob.tau[(size_t)b * ob.Lc + l / (L / ob.Lc)];
    const size_t o = sl * M;
    T x[VMAX];
    T smax = -INFINITY, xmax = -INFINITY;
    int arg = 0x7fffffff;
#pragma unroll
    for (int i = 0; i < VMAX; ++i) {
        const int j = lane + 64 * i;
        if (j < M) {
            const T s = ob.beta[o + j] + tau * ob.u[o + j];  // sparc.py:972
            x[i] = s / tau;                                  // sparc.py:430
            xmax = fmax(xmax, x[i]);
            if (s > smax) { smax = s; arg = j; }
        } else {
            x[i] = -INFINITY;
        }
    }
    xmax = wave_max(xmax);
    const T gmax = wave_max(smax);
    const int cand = wave_min(smax == gmax ? arg : 0x7fffffff);  // the first index attaining the maximum
    T den = T(0);
#pragma unroll
    for (int i = 0; i < VMAX; ++i) {
        x[i] = lane + 64 * i < M ? fexp<T>(x[i] - xmax) : T(0);
        den += x[i];
    }
    den = wave_sum(den);
    T ss = T(0), se = T(0);
#pragma unroll
    for (int i = 0; i < VMAX; ++i) {
        const int j = lane + 64 * i;
        if (j < M) {
            const T v = x[i] / den;
            ob.beta[o + j] = v;
            ss += v * v;
            const T d = v - (j == truth ? T(1) : T(0));
            se += d * d;
        }
    }
    ss = wave_sum(ss);
    se = wave_sum(se);
    if (lane == 0) {
        ob.bsq[sl] = (double)ss;
        ob.err[sl] = (double)se;
        ob.map[sl] = cand;
    }
}

// SectionRule::Bpsk.  The section sums in double in both precisions.
template <typename T, int VMAX>
__global__ __launch_bounds__(256) void bpsk_section_kernel(OpLoopBufs<T> ob) {
    const int lane = threadIdx.x & 63;
    const int l = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int b = blockIdx.y;
    const int L = ob.L, M = ob.M;
    if (l >= L || !ob.active[b]) return;
    const size_t sl = (size_t)b * L + l;
    const int truth = ob.truth ? ob.truth[sl] : -1;
    const int k = ob.known ? ob.known[sl] : -1;
    if (k >= 0 && k < 2 * M) {  // known: beta stays the +-1 one-hot that oploop_init_kernel wrote
        if (lane == 0) {
            ob.bsq[sl] = 1.0;
            ob.err[sl] = k == truth ? 0.0 : (truth < 0 || truth >= 2 * M) ? 1.0 : (k >> 1) == (truth >> 1) ? 4.0 : 2.0;
            ob.map[sl] = k;
        }
        return;
    }
    const int tloc = truth >= 0 ? truth >> 1 : -1;
    const T tval = (truth & 1) ? T(-1) : T(1);
    const T tau = (T)ob.tau[(size_t)b * ob.Lc + l / (L / ob.Lc)];
    const size_t o = sl * M;
    T x[VMAX];
    T amax = T(-1), xm = T(0);
    int word = 0x7fffffff;
#pragma unroll
    for (int i = 0; i < VMAX; ++i) {
        const int j = lane + 64 * i;
        if (j < M) {
            const T s = ob.beta[o + j] + tau * ob.u[o + j];  // sparc.py:972
            if (ob.s_keep) ob.s_keep[o + j] = s;             // soft output (amp_bpsk_llr.hip)
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
        const T e = fexp<T>(a - xm), q = -oexpm1<T>(T(-2) * a);
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
            ob.beta[o + j] = v;
            ss += (double)v * (double)v;
            const double d = (double)(v - (j == tloc ? tval : T(0)));
            se += d * d;
        }
    }
    ss = wave_sum(ss);
    se = wave_sum(se);
    if (lane == 0) {
        ob.bsq[sl] = ss;
        ob.err[sl] = se;
        ob.map[sl] = cand;
    }
}

// One thread per section.  Bit i (MSB first) of protected section l is bit (l - L_unp) logM + i of the codeword's
// mults N protected bits; the section is known when every block that holds one of its bits stopped on its
// syndrome (it < max_it).
template <typename T>
__global__ __launch_bounds__(256) void known_sections_kernel(const T *app, const int32_t *it, int max_it, int B,
                                                             int mults, int N, int L, int L_unp, int logM,
                                                             int32_t *known) {
    const size_t total = (size_t)B * L;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int b = (int)(i / L), l = (int)(i - (size_t)b * L);
        int out = -1;
        if (l >= L_unp) {
            const int q0 = (l - L_unp) * logM;
            bool ok = true;
            for (int blk = q0 / N; blk <= (q0 + logM - 1) / N; ++blk) ok = ok && it[(size_t)b * mults + blk] < max_it;
            if (ok) {
                out = 0;
                for (int j = 0; j < logM; ++j) out = (out << 1) | (app[(size_t)b * mults * N + q0 + j] < T(0) ? 1 : 0);
            }
        }
        known[i] = out;
    }
}

template <typename T>
int oploop_launch_init(const OpLoopBufs<T> &ob, SectionRule rule, hipStream_t s) {
    ProfScope ps(SG_PH_CONTROL, s);
    hipLaunchKernelGGL((oploop_init_kernel<T>), dim3(ob.B), dim3(OB), 0, s, ob, rule);
    SG_HIP(hipGetLastError());
    return SG_OK;
}

template <typename T>
int oploop_launch_residual(const OpLoopBufs<T> &ob, int t, hipStream_t s) {
    if (ob.Lr > 65535 || ob.B > 65535)
        return fail(SG_ERR_UNSUPPORTED, "residual kernel: %d row blocks, %d codewords (at most 65535 each)", ob.Lr,
                    ob.B);
    ProfScope ps(SG_PH_CONTROL, s);
    hipLaunchKernelGGL((oploop_residual_kernel<T>), dim3(ob.np, ob.Lr, ob.B), dim3(OB), 0, s, ob, t);
    SG_HIP(hipGetLastError());
    return SG_OK;
}

template <typename T>
int oploop_launch_control(const OpLoopBufs<T> &ob, int phase, int t, hipStream_t s) {
    ProfScope ps(SG_PH_CONTROL, s);
    hipLaunchKernelGGL((oploop_control_kernel<T>), dim3(ob.B), dim3(OB), 0, s, ob, phase, t);
    SG_HIP(hipGetLastError());
    return SG_OK;
}

template <typename T, int VMAX>
static void launch_section(const OpLoopBufs<T> &ob, SectionRule rule, hipStream_t s) {
    const dim3 grid((ob.L + 3) / 4, ob.B), block(256);
    if (rule == SectionRule::Bpsk) hipLaunchKernelGGL((bpsk_section_kernel<T, VMAX>), grid, block, 0, s, ob);
    else hipLaunchKernelGGL((known_section_kernel<T, VMAX>), grid, block, 0, s, ob);
}

template <typename T>
int oploop_launch_section(const OpLoopBufs<T> &ob, SectionRule rule, hipStream_t s) {
    const int M = ob.M;
    if (M < 2 || (M & (M - 1)) != 0 || M > 2048)
        return fail(SG_ERR_UNSUPPORTED, "%s section kernel: M = %d is not a power of two in [2, 2048]",
                    rule_name(rule), M);
    ProfScope ps(SG_PH_ETA, s);
    if (M <= 64) launch_section<T, 1>(ob, rule, s);
    else if (M <= 512) launch_section<T, 8>(ob, rule, s);
    else launch_section<T, 32>(ob, rule, s);
    SG_HIP(hipGetLastError());
    return SG_OK;
}

template <typename T>
int part_launch_known(const T *app, const int32_t *it, int max_it, int B, int mults, int N, int L, int L_unp, int logM,
                      int32_t *known, hipStream_t s) {
    const size_t blocks = ((size_t)B * L + 255) / 256;
    hipLaunchKernelGGL((known_sections_kernel<T>), dim3((unsigned)(blocks < 65535 ? blocks : 65535)), dim3(256), 0, s,
                       app, it, max_it, B, mults, N, L, L_unp, logM, known);
    SG_HIP(hipGetLastError());
    return SG_OK;
}

#define SG_OPLOOP_INST(T)                                                                                     \
    template int oploop_launch_init<T>(const OpLoopBufs<T> &, SectionRule, hipStream_t);                      \
    template int oploop_launch_residual<T>(const OpLoopBufs<T> &, int, hipStream_t);                          \
    template int oploop_launch_control<T>(const OpLoopBufs<T> &, int, int, hipStream_t);                      \
    template int oploop_launch_section<T>(const OpLoopBufs<T> &, SectionRule, hipStream_t);                   \
    template int part_launch_known<T>(const T *, const int32_t *, int, int, int, int, int, int, int, int32_t *, \
                                      hipStream_t);
SG_OPLOOP_INST(float)
SG_OPLOOP_INST(double)
#undef SG_OPLOOP_INST

}  // namespace sg
