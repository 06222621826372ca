// Regular-design AMP engine on gfx950: SPARCs whose base matrix has one
// transform per column block (W.ndim 0 or 1 -- the regular design of the
// benchmark, sparc.py:777-849, and power allocation).
//
// Reference: sparc_public/sparc.py sparc_amp :883-999, sub_dct :648-701,
// msg_vector_mmse_estimator :402-465, msg_vector_map_estimator :467-512.
//
// One AMP iteration (DESIGN.md "AMP engine") is six launches:
//   ab_stage1  (class m2)   beta = softmax(s) from (s, section max, 1/sum) in
//                           class order -> LDS scatter -> P-point FFT ->
//                           twiddle -> needed rows T[m2][rho]
//   ab_stage2  (row block)  Q-point DFT of each needed row at the needed
//                           frequencies -> X[k] (k in the needed set)
//   ctrl0      (codeword)   z = y - Re(c1 X[a] + c2 conj X[b]) + b z,
//                           phi, tau (sparc.py:931-969)
//   az_stage1  (row block)  G[k] from z/phi (<= 4 terms), inverse Q-point
//                           DFT of the sparse rows, conjugate twiddle -> U
//   az_stage2  (class m2)   U rows -> LDS -> inverse P-point FFT -> u in
//                           class order; s = beta + tau u (sparc.py:972);
//                           per-(class, section) max / sum e / sum e^2
//   merge      (codeword)   section max and 1/sum, sum beta^2 = S2/S1^2,
//                           beta at the true index -> psi, NMSE, early stop
//                           (sparc.py:973-988)
// beta itself never reaches HBM: it is recomputed from s where needed.
#include "amp.hpp"

namespace sg {

// reg_az_stage2 statistics: segment entries per round of LDS reads (entries summed in segment order for any
// round size: bit-identical results)
constexpr int FUSED_RC = 16;

// Exponent argument (v - m) / tau of the section softmax.  Double precision
// follows the reference's x = s / tau, x - max(x) (sparc.py:430-431); single
// precision multiplies by 1/tau.
template <typename T>
__device__ __forceinline__ T sm_arg(T v, T m, T tau, T inv_tau);
template <>
__device__ __forceinline__ float sm_arg<float>(float v, float m, float, float inv_tau) { return (v - m) * inv_tau; }
template <>
__device__ __forceinline__ double sm_arg<double>(double v, double m, double tau, double) { return v / tau - m / tau; }
// The same with the maximum's term staged once per section (sm_stage: m / tau
// in double -- the reference's max(x) of x = s / tau, as division by tau > 0 is
// monotonic -- and m itself in single precision), and v / tau as Markstein's
// division by a fixed divisor: q = v r with r = RN(1 / tau) (inv_tau), then
// one exact-residual correction q + (v - q tau) r.  Markstein's theorem makes
// that the correctly rounded quotient when q is within one ulp of v / tau,
// which q = RN(v r) does not guarantee in every corner, so the claim is
// empirical: tools/markstein_check.c compares it with v / tau on 10^8 random
// pairs of the decoder's range, 1.2e8 corner pairs (divisor significands near
// 1 and 2, quotients just below and above powers of two) and every value of
// the divisor's low 16 significand bits at top-of-binade quotients, and none
// differ (for -0 it gives +0, which the exponent that follows cannot tell
// apart; a last-ulp difference elsewhere would move one exponent argument by
// one ulp, inside the f64 bars of DESIGN.md "Oracle and parity").  Three FMA-class
// instructions instead of the ~11 of the general IEEE division, and one
// division per entry instead of two.
template <typename T>
__device__ __forceinline__ T sm_stage(T m, T tau) {
    if constexpr (sizeof(T) == 8) return m / tau;
    else return m;
}
template <typename T>
__device__ __forceinline__ T sm_arg_st(T v, T ms, T tau, T inv_tau) {
    if constexpr (sizeof(T) == 8) {
        const double q = v * inv_tau;
        return __builtin_fma(__builtin_fma(-q, tau, v), inv_tau, q) - ms;
    } else {
        return (v - ms) * inv_tau;
    }
}

// Section statistics of the single-precision engine are kept as sums over
// every entry but the maximum (whose term is exactly 1), so 1 - sum beta^2
// and the NMSE of decoded sections, ~1e-7 and below, come without the
// cancellation of 1 - S2/S1^2 in float.  Double keeps the reference's sums.
template <typename T>
inline constexpr bool kRestSums = sizeof(T) == 4;

// w_N2^(m2 k1), m2 < Q, k1 < P, from two small tables (contiguous per m2)
template <typename T>
__device__ __forceinline__ cx<T> reg_tw2(const RegTables<T> &tb, int m2, int k1) {
    return cmul(tb.twa[m2 * 64 + (k1 & 63)], tb.twb[m2 * tb.nB + (k1 >> 6)]);
}

// diagnostics: wave 0 of a workgroup stamps the shader clock at phase k
// (and, at the first and last phase, the device-wide 100 MHz realtime clock)
#define SG_TP(buf, k)                                                                                           \
    do {                                                                                                        \
        if ((buf) && tid == 0) {                                                                                \
            const size_t it_ = ((size_t)cw * tb.nT + t) * tb.Q + m2;                                             \
            (buf)[it_ * 8 + (k)] = __builtin_readcyclecounter();                                                \
            if ((k) == 0 || (k) == 7)                                                                           \
                ((buf) == bf.tprof_ab ? bf.trt_ab : bf.trt_az)[it_ * 2 + ((k) == 7)] = __builtin_amdgcn_s_memrealtime(); \
        }                                                                                                       \
    } while (0)

// Workgroups of the first wave with an odd linear index start `cycles` late,
// so that half the CUs run their memory phases while the other half computes
// (the CUs would otherwise stay in phase and alternate between saturating HBM
// and leaving it idle).  Grids of fewer than two rounds of workgroups start
// at once (nothing to interleave with).
__device__ __forceinline__ void reg_stagger(int cycles) {
    if (cycles <= 0 || gridDim.x * gridDim.y * gridDim.z < 512) return;
    const int lin = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
    if (lin < 256 && (lin & 1)) {
        for (int c = 0; c < cycles; c += 8128) __builtin_amdgcn_s_sleep(127);
    }
}

constexpr int REG_CH = 8;  // entries a thread loads before using them

// block size of a stage-1 kernel: P / EPT for the compile-time sizes
constexpr int reg_s1_threads(int EPT, int LOG2P) { return LOG2P > 0 ? (1 << LOG2P) / EPT : 1024; }

// LDS of a stage-1 workgroup: the FFT / class image (img reals), the section
// statistics, the class twiddles
size_t reg_stage1_lds(int img, int P, int Lblk, size_t real_bytes) {
    return (size_t)img * real_bytes + (size_t)2 * Lblk * real_bytes + (size_t)(64 + (P + 63) / 64) * 2 * real_bytes;
}

// ------------------------------------------------------------------ ab stage 1
template <typename T, int EPT, int LOG2P>
__global__ __launch_bounds__(reg_s1_threads(EPT, LOG2P)) void reg_ab_stage1(RegTables<T> tb, RegBufs<T> bf) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    cx<T> *d = reinterpret_cast<cx<T> *>(smem);
    T *dr = reinterpret_cast<T *>(smem);
    T *sM = dr + tb.img;  // after the FFT image (fsw) / skewed class image (fpad)
    T *sI = sM + tb.Lblk;
    cx<T> *ta = reinterpret_cast<cx<T> *>(sI + tb.Lblk);  // w_N2^(m2 k1) factors of this class
    cx<T> *tbb = ta + 64;
    const int m2 = blockIdx.x, t = blockIdx.y, cw = blockIdx.z;
    if (bf.mode == 0 && !bf.active[cw] && !tb.skip) return;
    const int tid = threadIdx.x, nthr = blockDim.x;
    reg_stagger(tb.stagger);
    SG_TP(bf.tprof_ab, 0);
    if (!(tb.skip & 16))
        for (int i = tid; i < tb.P * (int)sizeof(cx<T>) / 16; i += nthr) reinterpret_cast<uint4 *>(smem)[i] = uint4{0, 0, 0, 0};
    for (int i = tid; i < 64 + tb.nB; i += nthr)
        ta[i] = i < 64 ? tb.twa[m2 * 64 + i] : tb.twb[m2 * tb.nB + i - 64];
    const size_t tc = (size_t)t * tb.Mc;
    T tau = T(1), inv_tau = T(1);
    if (bf.mode == 0) {
        const size_t lb = (size_t)cw * tb.L + (size_t)t * tb.Lblk;
        const double tv = bf.tau[(size_t)cw * tb.Lc + t];
        tau = (T)tv;
        inv_tau = (T)(1.0 / tv);
        for (int l = tid; l < tb.Lblk; l += nthr) {
            sM[l] = sm_stage<T>(bf.stM[lb + l], tau);
            sI[l] = bf.stI[lb + l];
        }
    }
    __syncthreads();
    SG_TP(bf.tprof_ab, 1);
    const int32_t *cp = tb.cls_ptr + (size_t)t * (tb.Q + 1);
    const int q0 = cp[m2], q1 = cp[m2 + 1];
    const uint32_t *ls = tb.cls_ls + tc;
    if (bf.mode == 0 && !(tb.skip & 2)) {
        const T *s = bf.s + (size_t)cw * tb.LM + tc;
        for (int base = q0 + tid; base < q1; base += REG_CH * nthr) {
            T v[REG_CH];
            uint32_t e[REG_CH];
#pragma unroll
            for (int i = 0; i < REG_CH; ++i) {  // issue every load of the chunk first
                const int q = base + i * nthr;
                if (q < q1) {
                    v[i] = s[q];
                    e[i] = ls[q];
                }
            }
#pragma unroll
            for (int i = 0; i < REG_CH; ++i)
                if (base + i * nthr < q1) {
                    const int l = e[i] >> 16;
                    dr[e[i] & 0xffffu] = fexp<T>(sm_arg_st<T>(v[i], sM[l], tau, inv_tau)) * sI[l];
                }
        }
    } else if (bf.mode != 0) {
        const T *x = bf.ext_in + (size_t)cw * tb.LM + tc;
        const int32_t *cj = tb.cls_j + tc;
        for (int q = q0 + tid; q < q1; q += nthr) dr[ls[q] & 0xffffu] = x[cj[q]];
    }
    // output row indices (16-bit pairs; at most P = EPT nthr rows), in flight
    // under the FFT
    const int nR = (tb.skip & 4) ? 0 : tb.nR[t];
    uint32_t kp[EPT / 2];
    const uint32_t *rkp = tb.row_k1p + (size_t)t * (tb.P / 2);
#pragma unroll
    for (int j = 0; j < EPT / 2; ++j) kp[j] = rkp[j * nthr + tid];
    __syncthreads();
    SG_TP(bf.tprof_ab, 2);
    if (!(tb.skip & 1)) {
        if constexpr (LOG2P > 0) lds_fft1_ct<T, false, EPT, LOG2P>(d, tb.stw, tid);
        else lds_fft1<T, false, EPT>(d, tb.log2P, tb.stw, tid, nthr);
    }
    SG_TP(bf.tprof_ab, 3);
    cx<T> *out = bf.tu + (((size_t)cw * tb.nT + t) * tb.Q + m2) * tb.nRmax;
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
        const int r = tid + i * nthr;
        const int k1 = (kp[i >> 1] >> (16 * (i & 1))) & 0xffff;
        if (r < nR) out[r] = cmul(d[fsw(k1)], cmul(ta[k1 & 63], tbb[k1 >> 6]));
    }
    if (bf.tprof_ab) {
        SG_TP(bf.tprof_ab, 4); SG_TP(bf.tprof_ab, 5); SG_TP(bf.tprof_ab, 6);
        __syncthreads();  // diagnostics only: the end stamp waits for every wavefront
        SG_TP(bf.tprof_ab, 7);
    }
}

// ------------------------------------------------------------------ ab stage 2
template <typename T>
__global__ __launch_bounds__(256) void reg_ab_stage2(RegTables<T> tb, RegBufs<T> bf) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    cx<T> *d = reinterpret_cast<cx<T> *>(smem);  // [Q][RB]
    cx<T> *twq = d + (size_t)tb.Q * tb.RB;       // [Q]
    const int rb = blockIdx.x, t = blockIdx.y, cw = blockIdx.z;
    if (bf.mode == 0 && !bf.active[cw] && !tb.skip) return;
    const int nR = tb.nR[t];
    const int r0 = rb * tb.RB;
    if (r0 >= nR) return;
    const int r1 = min(nR, r0 + tb.RB), nr = r1 - r0;
    const int tid = threadIdx.x, nthr = blockDim.x;
    for (int i = tid; i < tb.Q; i += nthr) twq[i] = tb.twQ[i];
    const cx<T> *src = bf.tu + ((size_t)cw * tb.nT + t) * tb.Q * tb.nRmax;
    // rows [r0, r1) of every m2 plane: thread -> (row rr, planes m2 = m2a +
    // j * mstep), REG_CH loads in flight (RB divides the block size)
    const int rr = tid % tb.RB, mstep = nthr / tb.RB;
    if (rr < nr) {
        const cx<T> *sp = src + r0 + rr;
        for (int m0 = tid / tb.RB; m0 < tb.Q; m0 += REG_CH * mstep) {
            cx<T> v[REG_CH];
#pragma unroll
            for (int i = 0; i < REG_CH; ++i)  // (clamped, unconditional: all REG_CH in one round trip)
                v[i] = sp[(size_t)min(m0 + i * mstep, tb.Q - 1) * tb.nRmax];
#pragma unroll
            for (int i = 0; i < REG_CH; ++i) {
                const int m2 = m0 + i * mstep;
                if (m2 < tb.Q) d[m2 * tb.RB + rr] = v[i];
            }
        }
    }
    __syncthreads();
    const int32_t *kp = tb.kptr + (size_t)t * (tb.nRmax + 1);
    const int ka = kp[r0], kb = kp[r1];
    const int32_t *kr = tb.krho + (size_t)t * tb.nKmax, *k2s = tb.kk2 + (size_t)t * tb.nKmax;
    cx<T> *xn = bf.xn + ((size_t)cw * tb.nT + t) * tb.nKmax;
    const int qm = tb.Q - 1;
    for (int k = ka + tid; k < kb; k += nthr) {
        const int rho = kr[k] - r0, k2 = k2s[k];
        cx<T> acc{T(0), T(0)};
        for (int m2 = 0; m2 < tb.Q; ++m2) {
            const cx<T> v = d[m2 * tb.RB + rho], w = twq[(m2 * k2) & qm];
            acc.x += v.x * w.x - v.y * w.y;
            acc.y += v.x * w.y + v.y * w.x;
        }
        xn[k] = acc;
    }
}

// Forward output i of the design operator from the needed X values.
template <typename T>
__device__ __forceinline__ T reg_ab_out(const RegTables<T> &tb, const cx<T> *X, int i) {
    T r = T(0);
    for (int t = 0; t < tb.nT; ++t) {
        const size_t o = (size_t)t * tb.n + i;
        const cx<T> ha = X[(size_t)t * tb.nKmax + tb.oa[o]], hb = X[(size_t)t * tb.nKmax + tb.ob[o]];
        const cx<T> c1 = tb.oc[2 * o], c2 = tb.oc[2 * o + 1];
        r += (c1.x * ha.x - c1.y * ha.y) + (c2.x * hb.x + c2.y * hb.y);
    }
    return r;
}

template <typename T>
__global__ __launch_bounds__(256) void reg_ab_finish(RegTables<T> tb, RegBufs<T> bf) {
    const int cw = blockIdx.y;
    const cx<T> *X = bf.xn + (size_t)cw * tb.nT * tb.nKmax;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < tb.n; i += gridDim.x * blockDim.x)
        bf.ext_out[(size_t)cw * tb.n + i] = reg_ab_out(tb, X, i);
}

// ------------------------------------------------------------------ az stage 1
template <typename T>
__global__ __launch_bounds__(256) void reg_az_stage1(RegTables<T> tb, RegBufs<T> bf) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    cx<T> *twq = reinterpret_cast<cx<T> *>(smem);  // [Q]
    cx<T> *g = twq + tb.Q;                           // G of the block's needed indices
    int *rkp = reinterpret_cast<int *>(g + tb.maxKb);  // [RB + 1] kptr - ka, [RB] k1, [maxKb] k2
    int *rk1 = rkp + tb.RB + 1;
    int *rk2 = rk1 + tb.RB;
    const int rb = blockIdx.x, t = blockIdx.y, cw = blockIdx.z;
    if (bf.mode == 0 && !bf.active[cw] && !tb.skip) return;
    const int nR = tb.nR[t];
    const int r0 = rb * tb.RB;
    if (r0 >= nR) return;
    const int r1 = min(nR, r0 + tb.RB), nr = r1 - r0;
    const int tid = threadIdx.x, nthr = blockDim.x;
    for (int i = tid; i < tb.Q; i += nthr) twq[i] = tb.twQ[i];
    const int32_t *kp = tb.kptr + (size_t)t * (tb.nRmax + 1);
    const int ka = kp[r0], kb = kp[r1];
    const T *z = (bf.mode == 0 ? bf.z : bf.ext_in) + (size_t)cw * tb.n;
    const T phi = bf.mode == 0 ? (T)bf.phi[cw] : T(1);
    const int32_t *gi = tb.gi + (size_t)t * tb.nKmax * 4;
    const cx<T> *gc = tb.gc + (size_t)t * tb.nKmax * 4;
    for (int k = ka + tid; k < kb; k += nthr) {
        // the four terms' table entries, then their z values (clamped index, no branch): two
        // rounds of loads instead of a wait per term
        int ii[4];
        cx<T> cc[4];
        T zv[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            ii[q] = gi[4 * k + q];
            cc[q] = gc[4 * k + q];
        }
        const int k2v = tb.kk2[(size_t)t * tb.nKmax + k];
#pragma unroll
        for (int q = 0; q < 4; ++q) zv[q] = z[max(ii[q], 0)];
        cx<T> acc{T(0), T(0)};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (ii[q] >= 0) {
                const T v = zv[q] / phi;  // Az(z / phi), sparc.py:972
                acc.x += cc[q].x * v;
                acc.y += cc[q].y * v;
            }
        }
        g[k - ka] = acc;
        rk2[k - ka] = k2v;
    }
    for (int r = tid; r <= nr; r += nthr) {
        rkp[r] = kp[r0 + r] - ka;
        if (r < nr) rk1[r] = tb.row_k1[(size_t)t * tb.nRmax + r0 + r];
    }
    __syncthreads();
    cx<T> *dst = bf.tu + ((size_t)cw * tb.nT + t) * tb.Q * tb.nRmax;
    const int qm = tb.Q - 1;
    const int rr = tid % tb.RB, mstep = nthr / tb.RB;  // thread -> (row rr, planes m2a + j mstep)
    if (rr < nr) {
        const int a = rkp[rr], b = rkp[rr + 1], k1 = rk1[rr];
        for (int m2 = tid / tb.RB; m2 < tb.Q; m2 += mstep) {
            cx<T> acc{T(0), T(0)};
            for (int k = a; k < b; ++k) {
                const cx<T> v = g[k], w = twq[(m2 * rk2[k]) & qm];  // v * conj(w)
                acc.x += v.x * w.x + v.y * w.y;
                acc.y += v.y * w.x - v.x * w.y;
            }
            dst[(size_t)m2 * tb.nRmax + r0 + rr] = cmul(acc, cconj(reg_tw2(tb, m2, k1)));
        }
    }
}

// ------------------------------------------------------------------ az stage 2
template <typename T, int EPT, int LOG2P>
__global__ __launch_bounds__(reg_s1_threads(EPT, LOG2P)) void reg_az_stage2(RegTables<T> tb, RegBufs<T> bf, int t_iter) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    cx<T> *d = reinterpret_cast<cx<T> *>(smem);
    T *dr = reinterpret_cast<T *>(smem);
    T *sM = dr + tb.img;  // after the FFT image (fsw) / skewed class image (fpad)
    T *sI = sM + tb.Lblk;
    const int m2 = blockIdx.x, t = blockIdx.y, cw = blockIdx.z;
    if (bf.mode == 0 && !bf.active[cw] && !tb.skip) return;
    const int tid = threadIdx.x, nthr = blockDim.x;
    reg_stagger(tb.stagger);
    SG_TP(bf.tprof_az, 0);
    // one round trip: the U rows of this class (at most P = EPT nthr; row
    // indices as 16-bit pairs) and the statistics of the previous beta
    const int nR = (tb.skip & 4) ? 0 : tb.nR[t];
    const uint32_t *rkp = tb.row_k1p + (size_t)t * (tb.P / 2);
    const cx<T> *src = bf.tu + (((size_t)cw * tb.nT + t) * tb.Q + m2) * tb.nRmax;
    uint32_t kp[EPT / 2];
    cx<T> u[EPT];
#pragma unroll
    for (int j = 0; j < EPT / 2; ++j) kp[j] = rkp[j * nthr + tid];
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
        const int r = tid + i * nthr;
        if (r < nR) u[i] = src[r];
    }
    if (!(tb.skip & 16))
        for (int i = tid; i < tb.P * (int)sizeof(cx<T>) / 16; i += nthr) reinterpret_cast<uint4 *>(smem)[i] = uint4{0, 0, 0, 0};
    T tp = T(1), inv_tp = T(1);
    const bool have_beta = bf.mode == 0 && t_iter > 0;
    if (have_beta) {  // beta of the previous iteration = softmax(s_prev) with tau_prev
        const size_t lb = (size_t)cw * tb.L + (size_t)t * tb.Lblk;
        const double tv = bf.tau_prev[(size_t)cw * tb.Lc + t];
        tp = (T)tv;
        inv_tp = (T)(1.0 / tv);
        for (int l = tid; l < tb.Lblk; l += nthr) {
            sM[l] = sm_stage<T>(bf.stM[lb + l], tp);
            sI[l] = bf.stI[lb + l];
        }
    }
    __syncthreads();
    SG_TP(bf.tprof_az, 1);
#pragma unroll
    for (int i = 0; i < EPT; ++i)
        if (tid + i * nthr < nR) d[fsw((kp[i >> 1] >> (16 * (i & 1))) & 0xffff)] = u[i];
    __syncthreads();
    SG_TP(bf.tprof_az, 2);
    if (!(tb.skip & 1)) {
        if constexpr (LOG2P > 0) lds_fft1_ct<T, true, EPT, LOG2P>(d, tb.stw, tid);
        else lds_fft1<T, true, EPT>(d, tb.log2P, tb.stw, tid, nthr);
    }
    SG_TP(bf.tprof_az, 3);
    const size_t tc = (size_t)t * tb.Mc;
    const int32_t *cp = tb.cls_ptr + (size_t)t * (tb.Q + 1);
    const int q0 = cp[m2], q1 = cp[m2 + 1];
    const uint32_t *ls = tb.cls_ls + tc;
    if (bf.mode != 0) {
        T *out = bf.ext_out + (size_t)cw * tb.LM + tc;
        const int32_t *cj = tb.cls_j + tc;
        for (int q = q0 + tid; q < q1; q += nthr) out[cj[q]] = dr[ls[q] & 0xffffu];
        return;
    }
    const double tv = bf.tau[(size_t)cw * tb.Lc + t];
    const T tau = (T)tv, inv_tau = (T)(1.0 / tv);
    T *s = bf.s + (size_t)cw * tb.LM + tc;
    // s = beta + tau * Az(z/phi) for the thread's entries (a class holds at
    // most 2P = 2 EPT nthr entries); kept in registers until every u is read
    T snv[2 * EPT];
    const int qe = (tb.skip & 2) ? q0 : q1;
#pragma unroll
    for (int c = 0; c < 2 * EPT; c += REG_CH) {
        T v[REG_CH];
        uint32_t e[REG_CH];
#pragma unroll
        for (int i = 0; i < REG_CH; ++i) {
            const int q = q0 + tid + (c + i) * nthr;
            if (q < qe) {
                e[i] = ls[q];
                if (have_beta) v[i] = s[q];
            }
        }
#pragma unroll
        for (int i = 0; i < REG_CH; ++i) {
            const int q = q0 + tid + (c + i) * nthr;
            if (q < qe) {
                T b = T(0);
                const int l = e[i] >> 16;
                if (have_beta) b = fexp<T>(sm_arg_st<T>(v[i], sM[l], tp, inv_tp)) * sI[l];
                snv[c + i] = b + tau * dr[e[i] & 0xffffu];
            }
        }
    }
    SG_TP(bf.tprof_az, 4);
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 2 * EPT; ++c) {  // s of the class in class order, skewed by fpad
        const int q = q0 + tid + c * nthr;
        if (q < qe) dr[fpad(q - q0)] = snv[c];
    }
    __syncthreads();
    SG_TP(bf.tprof_az, 5);
    // per (class, section) statistics of the softmax, deterministic order
    const uint16_t *sg = tb.seg + ((size_t)t * tb.Q + m2) * (tb.Lblk + 1);
    T *pm = bf.part + (((size_t)cw * tb.nT + t) * tb.Q + m2) * 3 * (size_t)tb.Lblk;
    // one thread per section over its contiguous segment (segments average
    // ~16 entries: the fpad skew spreads the threads over the LDS banks)
    constexpr int RC = FUSED_RC;  // LDS reads in flight per thread
    for (int l = tid; l < ((tb.skip & 8) ? 0 : tb.Lblk); l += nthr) {
        const int a = sg[l], b = sg[l + 1];
        if constexpr (kRestSums<T>) {
            // f32: one pass with a running maximum; the sums exclude the first
            // occurrence of the maximum and are rescaled when it moves
            // (S <- (S + 1) e^{(m_old - m_new)/tau}), one exp per entry
            T m = -INFINITY, S1 = T(0), S2 = T(0);
            for (int c = a; c < b; c += RC) {
                T v[RC];
#pragma unroll
                for (int i = 0; i < RC; ++i) v[i] = dr[fpad(c + i)];  // in bounds of the LDS image; masked below
#pragma unroll
                for (int i = 0; i < RC; ++i)
                    if (c + i < b) {
                        const bool up = v[i] > m;
                        // <= 0; -inf on the first entry, whose (S + 1) e then vanishes
                        const T dlt = up ? (m - v[i]) : (v[i] - m);
                        const T e = fexp<T>(dlt * inv_tau);
                        S1 = up ? (S1 + T(1)) * e : S1 + e;
                        S2 = up ? (S2 + T(1)) * (e * e) : S2 + e * e;
                        m = up ? v[i] : m;
                    }
            }
            pm[l] = m;
            pm[tb.Lblk + l] = S1;
            pm[2 * tb.Lblk + l] = S2;
            continue;
        }
        T m = -INFINITY;
        for (int c = a; c < b; c += RC) {
            T v[RC];
#pragma unroll
            for (int i = 0; i < RC; ++i) {
                const T x = dr[fpad(c + i)];  // in bounds of the LDS image; masked below
                v[i] = (c + i < b) ? x : T(-INFINITY);
            }
#pragma unroll
            for (int i = 0; i < RC; ++i) m = fmax(m, v[i]);
        }
        T S1 = T(0), S2 = T(0);
        const T mst = sm_stage<T>(m, tau);
        bool seen = !kRestSums<T>;  // f32: sums over the segment without its (first) maximum
        for (int c = a; c < b; c += RC) {
            T v[RC];
#pragma unroll
            for (int i = 0; i < RC; ++i) v[i] = dr[fpad(c + i)];
#pragma unroll
            for (int i = 0; i < RC; ++i)
                if (c + i < b) {
                    T e = fexp<T>(sm_arg_st<T>(v[i], mst, tau, inv_tau));
                    if (!seen && v[i] == m) {
                        seen = true;
                        e = T(0);
                    }
                    S1 += e;
                    S2 += e * e;
                }
        }
        pm[l] = m;
        pm[tb.Lblk + l] = S1;
        pm[2 * tb.Lblk + l] = S2;
    }
    SG_TP(bf.tprof_az, 6);
    // s to HBM last (from the class-ordered LDS copy): stores count in vmcnt,
    // so they stay out of the load loops
    for (int q = q0 + tid; q < qe; q += nthr) s[q] = dr[fpad(q - q0)];
    if (bf.tprof_az) __syncthreads();  // diagnostics only: the end stamp waits for every wavefront
    SG_TP(bf.tprof_az, 7);
}

// ------------------------------------------------------------------ control
// Before Az (sparc.py:931-969): Onsager residual, phi, tau.  Lr = 1.  One
// workgroup per codeword; scalars stay in registers (no global re-reads), the
// residual's table loads are issued a round ahead of their X gathers, and
// |z|^2 for phi accumulates as z is written.
template <typename T>
__global__ __launch_bounds__(1024) void reg_ctrl0(RegTables<T> tb, RegBufs<T> bf, AmpScalars sc, AmpParams pr,
                                                  int t) {
    __shared__ double red[16];
    __shared__ double sh_g;
    const int cw = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
    if (!bf.active[cw]) return;
    const int Lc = tb.Lc;
    double *psi = sc.psi + (size_t)cw * Lc, *psi_prev = sc.psi_prev + (size_t)cw * Lc;
    double *tau = bf.tau + (size_t)cw * Lc, *tau_prev = bf.tau_prev + (size_t)cw * Lc;
    T *z = bf.z + (size_t)cw * tb.n;
    const T *y = bf.y + (size_t)cw * tb.n;
    const bool sum_z = pr.phi_method != 1;
    double acc = 0.0;
    if (t > 0) {
        if (tid == 0) {
            double g = 0.0;  // ndim 0: W * psi; ndim 1: dot(W, psi) / Lc
            for (int c = 0; c < Lc; ++c) {
                const double ps = psi[c];
                psi_prev[c] = ps;
                tau_prev[c] = tau[c];
                g += pr.W[c] * ps;
            }
            const double ph = bf.phi[cw];
            g = g / Lc;
            sc.phi_prev[cw] = ph;
            sc.gamma[cw] = g;
            sc.bcoef[cw] = g / ph;
            sh_g = g;
            red[0] = g / ph;
        }
        __syncthreads();
        const T b = (T)red[0];
        const cx<T> *X = bf.xn + (size_t)cw * tb.nT * tb.nKmax;
        // reg_ab_out for CO outputs per thread at a time: every table load of
        // the round issued before the dependent X gathers (8 spilled at the
        // 1024-thread register limit: 24 VGPRs in f32, 150 in f64)
        constexpr int CO = sizeof(T) == 8 ? 2 : 4;
        for (int i0 = tid; i0 < tb.n; i0 += CO * nthr) {
            T r[CO], yv[CO], zv[CO];
#pragma unroll
            for (int k = 0; k < CO; ++k) {
                const int i = i0 + k * nthr;
                r[k] = T(0);
                if (i < tb.n) {
                    yv[k] = y[i];
                    zv[k] = z[i];
                }
            }
            for (int t2 = 0; t2 < tb.nT; ++t2) {
                int ia[CO], ib[CO];
                cx<T> c1[CO], c2[CO], ha[CO], hb[CO];
#pragma unroll
                for (int k = 0; k < CO; ++k) {
                    const size_t o = (size_t)t2 * tb.n + i0 + k * nthr;
                    if (i0 + k * nthr < tb.n) {
                        ia[k] = tb.oa[o];
                        ib[k] = tb.ob[o];
                        c1[k] = tb.oc[2 * o];
                        c2[k] = tb.oc[2 * o + 1];
                    }
                }
                const cx<T> *Xt = X + (size_t)t2 * tb.nKmax;
#pragma unroll
                for (int k = 0; k < CO; ++k)
                    if (i0 + k * nthr < tb.n) {
                        ha[k] = Xt[ia[k]];
                        hb[k] = Xt[ib[k]];
                    }
#pragma unroll
                for (int k = 0; k < CO; ++k)
                    if (i0 + k * nthr < tb.n)
                        r[k] += (c1[k].x * ha[k].x - c1[k].y * ha[k].y) + (c2[k].x * hb[k].x + c2[k].y * hb[k].y);
            }
#pragma unroll
            for (int k = 0; k < CO; ++k)
                if (i0 + k * nthr < tb.n) {
                    const T zn = (yv[k] - r[k]) + b * zv[k];
                    z[i0 + k * nthr] = zn;
                    if (sum_z) acc += (double)zn * (double)zn;
                }
        }
    } else {
        for (int i = tid; i < tb.n; i += nthr) {
            const T v = y[i];
            z[i] = v;
            if (sum_z) acc += (double)v * (double)v;
        }
        if (tid == 0) {
            double g = 0.0;
            for (int c = 0; c < Lc; ++c) g += pr.W[c];
            g = g / Lc;
            sc.gamma[cw] = g;
            sh_g = g;
        }
    }
    double phi;
    if (sum_z) {
        phi = block_sum(acc, red) / (double)tb.n;
    } else {
        __syncthreads();
        phi = pr.awgn_var + sh_g;
    }
    if (tid == 0) {
        bf.phi[cw] = phi;
        for (int c = 0; c < Lc; ++c) tau[c] = (tb.L * phi / tb.n) / pr.W[c];
    }
}

// After Az: section statistics, psi, NMSE, stopping (sparc.py:973-988).
template <typename T>
__global__ __launch_bounds__(1024) void reg_merge(RegTables<T> tb, RegBufs<T> bf, AmpScalars sc, AmpParams pr,
                                                  int t) {
    __shared__ double red[16];
    const int cw = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
    if (!bf.active[cw]) return;
    const int Lc = tb.Lc, Lb = tb.Lblk;
    double *psi = sc.psi + (size_t)cw * Lc, *psi_prev = sc.psi_prev + (size_t)cw * Lc;
    double *nmse = sc.nmse + (size_t)cw * pr.t_max * Lc;
    for (int c = 0; c < Lc; ++c) {
        const double tv = bf.tau[(size_t)cw * Lc + c];
        const T tau = (T)tv, inv_tau = (T)(1.0 / tv);
        const T *pm = bf.part + ((size_t)cw * tb.nT + c) * tb.Q * 3 * (size_t)Lb;
        const T *s = bf.s + (size_t)cw * tb.LM + (size_t)c * tb.Mc;
        double a = 0.0, e = 0.0;
        for (int ll = tid; ll < Lb; ll += nthr) {
            const int l = c * Lb + ll;
            int jt = -1;
            if (bf.true_idx) jt = tb.qpos[(size_t)c * tb.Mc + ll * tb.M + bf.true_idx[(size_t)cw * tb.L + l]];
            if constexpr (kRestSums<T>) {
                // partials hold (max, sums without the max); the section's
                // designated maximum is the first partial attaining M
                // MC partials per round trip (independent loads issued together)
                constexpr int MC = 8;
                T M = -INFINITY;
                int pmx = -1;
                for (int m0 = 0; m0 < tb.Q; m0 += MC) {
                    T mv[MC];
#pragma unroll
                    for (int i = 0; i < MC; ++i) mv[i] = m0 + i < tb.Q ? pm[(size_t)(m0 + i) * 3 * Lb + ll] : T(-INFINITY);
#pragma unroll
                    for (int i = 0; i < MC; ++i)
                        if (mv[i] > M) {
                            M = mv[i];
                            pmx = m0 + i;
                        }
                }
                T R1 = T(0), R2 = T(0);
                constexpr int MC2 = MC / 2;  // three loads a partial: half the chunk (at MC, 12 VGPRs spilled)
                for (int m0 = 0; m0 < tb.Q; m0 += MC2) {
                    T mv[MC2], s1[MC2], s2[MC2];
#pragma unroll
                    for (int i = 0; i < MC2; ++i) {
                        const T *p = pm + (size_t)(m0 + i) * 3 * Lb;
                        const bool in = m0 + i < tb.Q;
                        mv[i] = in ? p[ll] : T(-INFINITY);
                        s1[i] = in ? p[Lb + ll] : T(0);
                        s2[i] = in ? p[2 * Lb + ll] : T(0);
                    }
#pragma unroll
                    for (int i = 0; i < MC2; ++i) {
                        if (!(mv[i] > -INFINITY)) continue;  // empty segment
                        if (m0 + i == pmx) {
                            R1 += s1[i];
                            R2 += s2[i];
                        } else {
                            const T f = fexp<T>(sm_arg<T>(mv[i], M, tau, inv_tau));
                            R1 += (T(1) + s1[i]) * f;
                            R2 += (T(1) + s2[i]) * (f * f);
                        }
                    }
                }
                const T inv = T(1) / (T(1) + R1);
                bf.stM[(size_t)cw * tb.L + l] = M;
                bf.stI[(size_t)cw * tb.L + l] = inv;
                // 1 - sum beta^2 = (2 R1 + R1^2 - R2) / (1 + R1)^2, no cancellation
                const double i2 = (double)inv * (double)inv, r1 = R1, r2 = R2;
                a += (2.0 * r1 + r1 * r1 - r2) * i2;
                if (jt >= 0) {
                    const T st = s[jt];
                    if (st == M)  // the true entry is a maximum: |beta - beta0|^2 = R1^2 + R2 over (1 + R1)^2
                        e += (r1 * r1 + r2) * i2;
                    else {
                        const double bt = (double)(fexp<T>(sm_arg<T>(st, M, tau, inv_tau)) * inv);
                        e += (1.0 + r2) * i2 - 2.0 * bt + 1.0;
                    }
                }
            } else {
                T M = -INFINITY;
                for (int m2 = 0; m2 < tb.Q; ++m2) {
                    const T *p = pm + (size_t)m2 * 3 * Lb;
                    if (p[Lb + ll] > T(0)) M = fmax(M, p[ll]);
                }
                T S1 = T(0), S2 = T(0);
                for (int m2 = 0; m2 < tb.Q; ++m2) {
                    const T *p = pm + (size_t)m2 * 3 * Lb;
                    const T S = p[Lb + ll];
                    if (S > T(0)) {
                        const T f = fexp<T>(sm_arg<T>(p[ll], M, tau, inv_tau));
                        S1 += S * f;
                        S2 += p[2 * Lb + ll] * (f * f);
                    }
                }
                const T inv = T(1) / S1;
                bf.stM[(size_t)cw * tb.L + l] = M;
                bf.stI[(size_t)cw * tb.L + l] = inv;
                const double ss = (double)(S2 * inv * inv);
                double err = ss;
                if (jt >= 0) {
                    const double bt = (double)(fexp<T>(sm_arg<T>(s[jt], M, tau, inv_tau)) * inv);
                    err = ss - 2.0 * bt + 1.0;
                }
                a += ss;
                e += err;
            }
        }
        a = block_sum(a, red);
        e = block_sum(e, red);
        if (tid == 0) {
            const double denom = (Lc == 1) ? (double)tb.L : (double)Lb;
            // f32 accumulates 1 - sum beta^2 per section; f64 the reference's sum beta^2
            psi[c] = kRestSums<T> ? a / denom : 1.0 - a / denom;
            nmse[(size_t)(t + 1) * Lc + c] = e / denom;
        }
    }
    __syncthreads();
    if (tid == 0) {
        bool stop = false;
        if (t > 0) {
            stop = true;
            for (int c = 0; c < Lc; ++c)
                if (!(fabs(psi[c] - psi_prev[c]) <= pr.atol + pr.rtol * fabs(psi_prev[c]))) stop = false;
        }
        if (stop) {  // nmse[t:] = nmse[t] (sparc.py:985)
            for (int tt = t + 1; tt < pr.t_max; ++tt)
                for (int c = 0; c < Lc; ++c) nmse[(size_t)tt * Lc + c] = nmse[(size_t)t * Lc + c];
            sc.t_final[cw] = t + 1;
            bf.active[cw] = 0;
        } else if (t == pr.t_max - 2) {
            sc.t_final[cw] = t + 1;
            bf.active[cw] = 0;
        }
    }
}

// Final MAP decision (sparc.py:997, msg_vector_map_estimator :485-487): the
// first index of each section where s attains the section maximum.
template <typename T>
__global__ __launch_bounds__(256) void reg_map(RegTables<T> tb, RegBufs<T> bf) {
    const int m2 = blockIdx.x, t = blockIdx.y, cw = blockIdx.z;
    const size_t tc = (size_t)t * tb.Mc;
    const int32_t *cp = tb.cls_ptr + (size_t)t * (tb.Q + 1);
    const int q0 = cp[m2], q1 = cp[m2 + 1];
    const T *s = bf.s + (size_t)cw * tb.LM + tc;
    const uint32_t *lsq = tb.cls_ls + tc;
    const int32_t *cj = tb.cls_j + tc;
    // MU entries per thread at a time, every load requested before any atomic (an atomic between
    // them kept the next entry's loads behind it: one round trip per entry, 0.25 ms per C2 decode)
    constexpr int MU = 8;
    const size_t lb = (size_t)cw * tb.L + (size_t)t * tb.Lblk;
    for (int qb = q0 + (int)threadIdx.x; qb < q1; qb += MU * (int)blockDim.x) {
        uint32_t e[MU];
        int32_t jj[MU];
        T v[MU], m[MU];
#pragma unroll
        for (int u = 0; u < MU; ++u) {
            const int q = min(qb + u * (int)blockDim.x, q1 - 1);
            e[u] = lsq[q];
            v[u] = s[q];
            jj[u] = cj[q];
        }
#pragma unroll
        for (int u = 0; u < MU; ++u) m[u] = bf.stM[lb + (e[u] >> 16)];
#pragma unroll
        for (int u = 0; u < MU; ++u) {
            const int ls = (int)(e[u] >> 16);
            if (qb + u * (int)blockDim.x < q1 && v[u] == m[u]) atomicMin(&bf.map[lb + ls], jj[u] - ls * tb.M);
        }
    }
}

// Initial state (sparc.py:914-927): every codeword active, nmse[0..] = 1.
__global__ void reg_init_kernel(int Lc, int t_max, double *nmse, int32_t *active, int32_t *t_final) {
    const int cw = blockIdx.x;
    for (int i = threadIdx.x; i < t_max * Lc; i += blockDim.x) nmse[(size_t)cw * t_max * Lc + i] = 1.0;
    if (threadIdx.x == 0) {
        active[cw] = 1;
        t_final[cw] = 0;
    }
}

int reg_launch_init(int B, int Lc, int t_max, double *nmse, int32_t *active, int32_t *t_final, hipStream_t s) {
    if (B <= 0) return SG_OK;
    hipLaunchKernelGGL(reg_init_kernel, dim3(B), dim3(256), 0, s, Lc, t_max, nmse, active, t_final);
    SG_HIP(hipGetLastError());
    return SG_OK;
}

// ------------------------------------------------------------------ launchers
template <typename T, int EPT, int LOG2P>
static void launch_s1(const RegTables<T> &tb, const RegBufs<T> &bf, size_t lds, hipStream_t s) {
    hipLaunchKernelGGL((reg_ab_stage1<T, EPT, LOG2P>), dim3(tb.Q, tb.nT, bf.B), dim3(tb.P / EPT), lds, s, tb, bf);
}
template <typename T, int EPT, int LOG2P>
static void launch_s2i(const RegTables<T> &tb, const RegBufs<T> &bf, int t_iter, size_t lds, hipStream_t s) {
    hipLaunchKernelGGL((reg_az_stage2<T, EPT, LOG2P>), dim3(tb.Q, tb.nT, bf.B), dim3(tb.P / EPT), lds, s, tb, bf,
                       t_iter);
}
// compile-time FFT for the benchmark sizes (f32: P = 2^14 at EPT 16; f64:
// P = 2^13 at EPT 8)
constexpr int reg_hot_log2p(bool dbl) { return dbl ? 13 : 14; }
constexpr int reg_hot2_log2p(bool dbl) { return 13; }  // f32 at P = 2^13 (SG_AMP_PMAX=8192: two workgroups per CU)

template <typename T>
static int reg_set_attrs() {
    static bool done = false;
    if (done) return SG_OK;
    const int mx = 160 * 1024;
#define SG_LDS_ATTR(K) SG_HIP(hipFuncSetAttribute((const void *)(K), hipFuncAttributeMaxDynamicSharedMemorySize, mx))
    constexpr int H = reg_hot_log2p(sizeof(T) == 8), HE = sizeof(T) == 8 ? 8 : 16;
    SG_LDS_ATTR((reg_ab_stage1<T, 8, 0>)); SG_LDS_ATTR((reg_ab_stage1<T, 16, 0>));
    SG_LDS_ATTR((reg_az_stage2<T, 8, 0>)); SG_LDS_ATTR((reg_az_stage2<T, 16, 0>));
    SG_LDS_ATTR((reg_ab_stage1<T, HE, H>)); SG_LDS_ATTR((reg_az_stage2<T, HE, H>));
    if constexpr (sizeof(T) == 4) {
        constexpr int H2 = reg_hot2_log2p(false);
        SG_LDS_ATTR((reg_ab_stage1<T, HE, H2>)); SG_LDS_ATTR((reg_az_stage2<T, HE, H2>));
    }
    SG_LDS_ATTR((reg_ab_stage2<T>)); SG_LDS_ATTR((reg_az_stage1<T>));
#undef SG_LDS_ATTR
    done = true;
    return SG_OK;
}

template <typename T>
int reg_launch_ab(const RegTables<T> &tb, const RegBufs<T> &bf, hipStream_t s) {
    if (bf.B <= 0) return SG_OK;
    SG_TRY(reg_set_attrs<T>());
    const size_t lds1 = reg_stage1_lds(tb.img, tb.P, tb.Lblk, sizeof(T));
    const int ept = tb.ept;
    {
        ProfScope ps(SG_PH_AB_A, s);
        constexpr int H = reg_hot_log2p(sizeof(T) == 8), HE = sizeof(T) == 8 ? 8 : 16;
        if (tb.log2P == H && ept == HE) launch_s1<T, HE, H>(tb, bf, lds1, s);
        else if (sizeof(T) == 4 && tb.log2P == reg_hot2_log2p(false) && ept == HE)
            launch_s1<T, HE, reg_hot2_log2p(false)>(tb, bf, lds1, s);
        else if (ept == 8) launch_s1<T, 8, 0>(tb, bf, lds1, s);
        else if (ept == 16) launch_s1<T, 16, 0>(tb, bf, lds1, s);
        else return fail(SG_ERR_UNSUPPORTED, "stage-1 FFT length P=%d unsupported", tb.P);
    }
    SG_HIP(hipGetLastError());
    {
        ProfScope ps(SG_PH_AB_B, s);
        const size_t lds2 = sizeof(cx<T>) * ((size_t)tb.Q * tb.RB + tb.Q);
        hipLaunchKernelGGL((reg_ab_stage2<T>), dim3(tb.nrb, tb.nT, bf.B), dim3(256), lds2, s, tb, bf);
    }
    SG_HIP(hipGetLastError());
    return SG_OK;
}

template <typename T>
int reg_launch_ab_finish(const RegTables<T> &tb, const RegBufs<T> &bf, hipStream_t s) {
    if (bf.B <= 0) return SG_OK;
    hipLaunchKernelGGL((reg_ab_finish<T>), dim3((tb.n + 255) / 256, bf.B), dim3(256), 0, s, tb, bf);
    SG_HIP(hipGetLastError());
    return SG_OK;
}

template <typename T>
int reg_launch_az(const RegTables<T> &tb, const RegBufs<T> &bf, int t_iter, hipStream_t s) {
    if (bf.B <= 0) return SG_OK;
    SG_TRY(reg_set_attrs<T>());
    {
        ProfScope ps(SG_PH_AZ_A, s);
        const size_t ldsg = sizeof(cx<T>) * ((size_t)tb.maxKb + tb.Q) + sizeof(int) * (2 * (size_t)tb.RB + 1 + tb.maxKb);
        hipLaunchKernelGGL((reg_az_stage1<T>), dim3(tb.nrb, tb.nT, bf.B), dim3(256), ldsg, s, tb, bf);
    }
    SG_HIP(hipGetLastError());
    const size_t lds1 = reg_stage1_lds(tb.img, tb.P, tb.Lblk, sizeof(T));
    const int ept = tb.ept;
    {
        ProfScope ps(SG_PH_AZ_B, s);
        constexpr int H = reg_hot_log2p(sizeof(T) == 8), HE = sizeof(T) == 8 ? 8 : 16;
        if (tb.log2P == H && ept == HE) launch_s2i<T, HE, H>(tb, bf, t_iter, lds1, s);
        else if (sizeof(T) == 4 && tb.log2P == reg_hot2_log2p(false) && ept == HE)
            launch_s2i<T, HE, reg_hot2_log2p(false)>(tb, bf, t_iter, lds1, s);
        else if (ept == 8) launch_s2i<T, 8, 0>(tb, bf, t_iter, lds1, s);
        else if (ept == 16) launch_s2i<T, 16, 0>(tb, bf, t_iter, lds1, s);
        else return fail(SG_ERR_UNSUPPORTED, "stage-1 FFT length P=%d unsupported", tb.P);
    }
    SG_HIP(hipGetLastError());
    return SG_OK;
}

template <typename T>
int reg_launch_ctrl0(const RegTables<T> &tb, const RegBufs<T> &bf, const AmpScalars &sc, const AmpParams &pr, int t,
                     hipStream_t s) {
    if (bf.B <= 0) return SG_OK;
    ProfScope ps(SG_PH_CONTROL, s);
    hipLaunchKernelGGL((reg_ctrl0<T>), dim3(bf.B), dim3(1024), 0, s, tb, bf, sc, pr, t);
    SG_HIP(hipGetLastError());
    return SG_OK;
}

template <typename T>
int reg_launch_merge(const RegTables<T> &tb, const RegBufs<T> &bf, const AmpScalars &sc, const AmpParams &pr, int t,
                     hipStream_t s) {
    if (bf.B <= 0) return SG_OK;
    ProfScope ps(SG_PH_ETA, s);
    hipLaunchKernelGGL((reg_merge<T>), dim3(bf.B), dim3(1024), 0, s, tb, bf, sc, pr, t);
    SG_HIP(hipGetLastError());
    return SG_OK;
}

template <typename T>
int reg_launch_map(const RegTables<T> &tb, const RegBufs<T> &bf, hipStream_t s) {
    if (bf.B <= 0) return SG_OK;
    hipLaunchKernelGGL((reg_map<T>), dim3(tb.Q, tb.nT, bf.B), dim3(256), 0, s, tb, bf);
    SG_HIP(hipGetLastError());
    return SG_OK;
}

#define SG_REG_INST(T)                                                                                          \
    template int reg_launch_ab<T>(const RegTables<T> &, const RegBufs<T> &, hipStream_t);                       \
    template int reg_launch_az<T>(const RegTables<T> &, const RegBufs<T> &, int, hipStream_t);                  \
    template int reg_launch_ctrl0<T>(const RegTables<T> &, const RegBufs<T> &, const AmpScalars &,             \
                                     const AmpParams &, int, hipStream_t);                                     \
    template int reg_launch_merge<T>(const RegTables<T> &, const RegBufs<T> &, const AmpScalars &,             \
                                     const AmpParams &, int, hipStream_t);                                     \
    template int reg_launch_map<T>(const RegTables<T> &, const RegBufs<T> &, hipStream_t);                      \
    template int reg_launch_ab_finish<T>(const RegTables<T> &, const RegBufs<T> &, hipStream_t);
SG_REG_INST(float)
SG_REG_INST(double)

}  // namespace sg
