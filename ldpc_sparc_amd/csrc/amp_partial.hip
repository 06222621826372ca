// AMP with known sections (sg_amp_decode_partial_device, capi_amp.cpp): the kernels between the plan's operators
// Ab / Az on natural-order vectors, and the BP -> known-sections glue of the three-stage concatenated decoder.
//
// The loop is sparc_amp (sparc.py:883-999) for W of ndim 0 or 1 with the denoiser of a known section replaced
// by the one-hot of its index, started from beta0 = the known one-hots and z0 = y - Ab(beta0):
//
//   part_init_kernel      beta0, psi0_c = the share of unknown sections of column block c, gamma0, nmse = 1
//   part_residual_kernel  z <- y - Ab(beta) + b z (t = 0: y - Ab(beta0)) and partial sums of z^2
//   part_control_kernel   phase 0: phi (:949-955), tau_c = (L phi / n) / W_c (:958-965), zs = z / phi
//                         phase 1: psi, the NMSE row, the stop decision (:976-988), then gamma and b = gamma / phi
//                         of the next iteration (:936-942)
//   part_section_kernel   s = beta + tau u (:972), beta = softmax(s / tau) or the one-hot, sum beta^2, the squared
//                         error against true_idx, the first-maximum argmax of s (:997) or the known index
//   known_sections_kernel hard decisions of a BP output -> section indices, -1 where a block did not converge
//
// A codeword that stopped is skipped by every kernel, so it keeps its state.  Fixed-order reductions, no atomics:
// a codeword's result does not depend on the batch it is decoded in.
#include "amp_partial.hpp"
#include "device_util.hpp"

namespace sg {

namespace {

constexpr int PB = 256;  // block size of the residual, control and init kernels

template <typename T>
__device__ __forceinline__ T pexp(T x);
template <>
__device__ __forceinline__ float pexp<float>(float x) { return __expf(x); }
template <>
__device__ __forceinline__ double pexp<double>(double x) { return exp(x); }

// gamma = W psi (flat) or dot(W, psi) / Lc (power allocation), sparc.py:936-939
__device__ __forceinline__ double gamma_of(const double *W, const double *psi, int ndim, int Lc) {
    if (ndim == 0) return W[0] * psi[0];
    double acc = 0.0;
    for (int c = 0; c < Lc; ++c) acc += W[c] * psi[c];
    return acc / Lc;
}

}  // namespace

// One workgroup per codeword.  beta was zeroed by the caller.
template <typename T>
__global__ __launch_bounds__(PB) void part_init_kernel(PartBufs<T> pb) {
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int L = pb.L, Lc = pb.Lc, spc = L / Lc;
    const int32_t *known = pb.known + (size_t)b * L;
    double *psi = pb.psi + (size_t)b * Lc;
    double *nmse = pb.nmse + (size_t)b * pb.t_max * Lc;
    for (int i = tid; i < pb.t_max * Lc; i += PB) nmse[i] = 1.0;
    for (int l = tid; l < L; l += PB) {
        const int k = known[l];
        if (k >= 0 && k < pb.M) pb.beta[(size_t)b * pb.LM + (size_t)l * pb.M + k] = T(1);
    }
    for (int c = tid >> 6; c < Lc; c += PB / 64) {  // one wavefront per column block
        double unk = 0.0;
        for (int l = c * spc + lane; l < (c + 1) * spc; l += 64) {
            const int k = known[l];
            unk += (k >= 0 && k < pb.M) ? 0.0 : 1.0;
        }
        unk = wave_sum(unk);
        if (lane == 0) psi[c] = unk / spc;
    }
    __syncthreads();
    if (tid == 0) {
        pb.gamma[b] = gamma_of(pb.W, psi, pb.ndim, Lc);
        pb.bco[b] = 0.0;
        pb.active[b] = 1;
        pb.t_final[b] = 0;
    }
}

// np workgroups per codeword, each striding over n from its own offset.
template <typename T>
__global__ __launch_bounds__(PB) void part_residual_kernel(PartBufs<T> pb, int t) {
    __shared__ double red[PB / 64];
    const int b = blockIdx.y, tid = threadIdx.x;
    if (!pb.active[b]) return;
    const size_t o = (size_t)b * pb.n;
    const T bc = (T)pb.bco[b];
    double zz = 0.0;
    for (int i = blockIdx.x * PB + tid; i < pb.n; i += pb.np * PB) {
        T zn = pb.y[o + i] - pb.r[o + i];
        if (t > 0) zn += bc * pb.z[o + i];
        pb.z[o + i] = zn;
        zz += (double)zn * (double)zn;
    }
    zz = block_sum<PB / 64>(zz, red);
    if (tid == 0) pb.zz[(size_t)b * pb.np + blockIdx.x] = zz;
}

// One workgroup per codeword, in double.
template <typename T>
__global__ __launch_bounds__(PB) void part_control_kernel(PartBufs<T> pb, int phase, int t) {
    __shared__ double red[PB / 64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    if (!pb.active[b]) return;
    const int L = pb.L, Lc = pb.Lc, n = pb.n;
    double *psi = pb.psi + (size_t)b * Lc, *psi_prev = pb.psi_prev + (size_t)b * Lc;
    if (phase == 0) {
        double phi;  // (every thread the same sum in the same order)
        if (pb.phi_method == 1) {
            phi = pb.awgn_var + pb.gamma[b];
        } else {
            double acc = 0.0;
            for (int q = 0; q < pb.np; ++q) acc += pb.zz[(size_t)b * pb.np + q];
            phi = acc / n;
        }
        if (tid == 0) pb.phi[b] = phi;
        for (int c = tid; c < Lc; c += PB) pb.tau[(size_t)b * Lc + c] = (L * phi / n) / pb.W[c];
        const size_t o = (size_t)b * n;
        const T ph = (T)phi;
        for (int i = tid; i < n; i += PB) pb.zs[o + i] = pb.z[o + i] / ph;
        return;
    }
    const int spc = L / Lc;
    const double denom = (double)spc;
    double *nmse = pb.nmse + (size_t)b * pb.t_max * Lc;
    const double *bsq = pb.bsq + (size_t)b * L, *err = pb.err + (size_t)b * L;
    if (Lc > 1) {  // one wavefront per column block
        for (int c = tid >> 6; c < Lc; c += PB / 64) {
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
        for (int l = tid; l < L; l += PB) {
            a += bsq[l];
            e += err[l];
        }
        a = block_sum<PB / 64>(a, red);
        e = block_sum<PB / 64>(e, red);
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
            if (!(fabs(psi[c] - psi_prev[c]) <= pb.atol + pb.rtol * fabs(psi_prev[c]))) stop = false;
    }
    if (stop) {  // nmse[t:] = nmse[t]
        for (int tt = t + 1; tt < pb.t_max; ++tt)
            for (int c = 0; c < Lc; ++c) nmse[(size_t)tt * Lc + c] = nmse[(size_t)t * Lc + c];
        pb.t_final[b] = t + 1;
        pb.active[b] = 0;
    } else if (t == pb.t_max - 2) {
        pb.t_final[b] = t + 1;
        pb.active[b] = 0;
    } else {  // the next iteration's psi_prev, gamma and b = gamma / phi_prev
        for (int c = 0; c < Lc; ++c) psi_prev[c] = psi[c];
        const double g = gamma_of(pb.W, psi, pb.ndim, Lc);
        pb.gamma[b] = g;
        pb.bco[b] = g / pb.phi[b];
    }
}

// One wavefront per section, four per workgroup: lane holds the entries j = lane + 64 i, i < VMAX; lanes >= M idle
// when M < 64.  The softmax is shifted by the section's maximum of s / tau.
template <typename T, int VMAX>
__global__ __launch_bounds__(256) void part_section_kernel(PartBufs<T> pb) {
    const int lane = threadIdx.x & 63;
    const int l = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int b = blockIdx.y;
    const int L = pb.L, M = pb.M;
    if (l >= L || !pb.active[b]) return;
    const size_t sl = (size_t)b * L + l;
    const int k = pb.known[sl];
    const int truth = pb.true_idx ? pb.true_idx[sl] : -1;
    if (k >= 0 && k < M) {  // known: beta stays the one-hot that part_init_kernel wrote
        if (lane == 0) {
            pb.bsq[sl] = 1.0;
            pb.err[sl] = k == truth ? 0.0 : (truth >= 0 && truth < M ? 2.0 : 1.0);
            pb.map[sl] = k;
        }
        return;
    }
    const T tau = (T)pb.tau[(size_t)b * pb.Lc + l / (L / pb.Lc)];
    const size_t o = sl * M;
    T x[VMAX];
    T smax = -INFINITY, xmax = -INFINITY;
    int arg = 0x7fffffff;
#pragma unroll
    for (int i = 0; i < VMAX; ++i) {
        const int j = lane + 64 * i;
        if (j < M) {
            const T s = pb.beta[o + j] + tau * pb.u[o + j];  // sparc.py:972
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
        x[i] = lane + 64 * i < M ? pexp<T>(x[i] - xmax) : T(0);
        den += x[i];
    }
    den = wave_sum(den);
    T ss = T(0), se = T(0);
#pragma unroll
    for (int i = 0; i < VMAX; ++i) {
        const int j = lane + 64 * i;
        if (j < M) {
            const T v = x[i] / den;
            pb.beta[o + j] = v;
            ss += v * v;
            const T d = v - (j == truth ? T(1) : T(0));
            se += d * d;
        }
    }
    ss = wave_sum(ss);
    se = wave_sum(se);
    if (lane == 0) {
        pb.bsq[sl] = (double)ss;
        pb.err[sl] = (double)se;
        pb.map[sl] = cand;
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
int part_launch_init(const PartBufs<T> &pb, hipStream_t s) {
    ProfScope ps(SG_PH_CONTROL, s);
    hipLaunchKernelGGL((part_init_kernel<T>), dim3(pb.B), dim3(PB), 0, s, pb);
    SG_HIP(hipGetLastError());
    return SG_OK;
}

template <typename T>
int part_launch_residual(const PartBufs<T> &pb, int t, hipStream_t s) {
    ProfScope ps(SG_PH_CONTROL, s);
    hipLaunchKernelGGL((part_residual_kernel<T>), dim3(pb.np, pb.B), dim3(PB), 0, s, pb, t);
    SG_HIP(hipGetLastError());
    return SG_OK;
}

template <typename T>
int part_launch_control(const PartBufs<T> &pb, int phase, int t, hipStream_t s) {
    ProfScope ps(SG_PH_CONTROL, s);
    hipLaunchKernelGGL((part_control_kernel<T>), dim3(pb.B), dim3(PB), 0, s, pb, phase, t);
    SG_HIP(hipGetLastError());
    return SG_OK;
}

template <typename T>
int part_launch_section(const PartBufs<T> &pb, hipStream_t s) {
    const int M = pb.M;
    if (M < 2 || (M & (M - 1)) != 0 || M > 2048)
        return fail(SG_ERR_UNSUPPORTED, "partial section kernel: M = %d is not a power of two in [2, 2048]", M);
    ProfScope ps(SG_PH_ETA, s);
    const dim3 grid((pb.L + 3) / 4, pb.B), block(256);
    if (M <= 64) hipLaunchKernelGGL((part_section_kernel<T, 1>), grid, block, 0, s, pb);
    else if (M <= 512) hipLaunchKernelGGL((part_section_kernel<T, 8>), grid, block, 0, s, pb);
    else hipLaunchKernelGGL((part_section_kernel<T, 32>), grid, block, 0, s, pb);
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

#define SG_PART_INST(T)                                                                                       \
    template int part_launch_init<T>(const PartBufs<T> &, hipStream_t);                                       \
    template int part_launch_residual<T>(const PartBufs<T> &, int, hipStream_t);                              \
    template int part_launch_control<T>(const PartBufs<T> &, int, int, hipStream_t);                          \
    template int part_launch_section<T>(const PartBufs<T> &, hipStream_t);                                    \
    template int part_launch_known<T>(const T *, const int32_t *, int, int, int, int, int, int, int, int32_t *, \
                                      hipStream_t);
SG_PART_INST(float)
SG_PART_INST(double)
#undef SG_PART_INST

}  // namespace sg
