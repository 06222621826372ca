// AMP decoder for complex SPARCs with sub-sampled FFT designs and K-PSK
// modulated message vectors on gfx950, double precision.
//
// Reference: sparc_public/sparc.py sparc_amp :883-999 (loop), sparc_transforms
// :703-880 with sub_fft :593-646 (design operator), msg_vector_mmse_estimator
// :402-465 (denoisers, K branches), msg_vector_map_estimator :467-512 (MAP).
//
// Operator (DESIGN.md "Complex engine"): for each transform (nonzero block of W)
//   Ab:  r = sqrt(W_rc/L) * FFT_w(scatter(beta_c, order1))[order0]
//   Az:  u = sqrt(W_rc/L) * conj(FFT_w(conj(scatter(z_r/phi_r, order0))))[order1]
// The second is the unnormalised inverse transform, so both directions are one
// w-point complex FFT, run four-step with w = P Q, input m = Q m1 + m2, output
// k = k1 + P k2:
//   pass A  (per tile of CT columns m2): scatter the input into h[m1][m2],
//           P-point FFTs over m1, twiddle w_w^{m2 k1}, store T[k1][m2]
//   pass B  (per tile of RT rows k1): Q-point FFTs over m2, store X[k1][k2]
// 16 <= w <= 2^16: P = 2^floor(log2 w / 2), both passes 2048 values in at most
// 256 threads.  2^17 <= w <= 2^20: P = 256 and Q = w / 256 = 512 ... 4096, so
// pass A keeps its shape and its 8-wide runs, and pass B (cfft_passB_long)
// takes tiles of 4096 values -- rows are contiguous in buf0, so a long row
// costs nothing in coalescing -- in 512 threads and 64 KB of LDS.  The stage
// twiddles come from the Q-entry host table, the inter-pass ones from the
// w-entry host table (16 MB at 2^20); nothing uses device sincos.
// The needed outputs are single bins, read where they are used (the residual
// of the control kernel, the s update of eta) from X at (k mod P) Q + k / P.
//   eta     (one wavefront per section): s = beta + tau u (also stored in
//           CampBufs::s_keep when soft output is on), the K-PSK MMSE
//           denoiser (max-shifted per section: the same function as the
//           reference's global-max float128 form), the MAP decision of s and
//           the section statistics
//   control (one workgroup per codeword): Onsager residual, phi, tau, psi,
//           NMSE, early stop (sparc.py:931-988) with complex quantities.
// With known sections (CampBufs::known_idx, sg_camp_decode_partial*) the loop
// is the same with the denoiser of a known section replaced by its
// constellation one-hot, started from beta0 = the known one-hots and
// z0 = y - A beta0: control's initialisation writes beta0, psi0 and gamma0, its
// phase 0 of iteration 0 takes A beta0 off y, and eta reports a known section's
// sums and decision without touching its beta.
// A codeword that stopped is skipped by every kernel, so it keeps its state.
// Fixed-order reductions, no atomics: a codeword's result does not depend on
// the batch it is decoded in.
#include "camp_section.hpp"

namespace sg {
namespace {

// ------------------------------------------------------------------ pass A
// INV = false: input beta of the transform's column block scattered by order1;
// INV = true: input z / phi of its row block scattered by order0.
template <bool INV>
__global__ __launch_bounds__(256) void cfft_passA(CampTables tb, CampBufs bf) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    cxd *d = reinterpret_cast<cxd *>(smem_raw);
    const int cw = blockIdx.z, t = blockIdx.y;
    if (!bf.active[cw]) return;
    const int nthr = blockDim.x, tid = threadIdx.x;
    const int CT = tb.CT, m2_0 = blockIdx.x * CT, total = tb.P * CT;
    const int32_t *inmap = (INV ? tb.in0 : tb.in1) + (size_t)t * tb.w;
    const cxd *src = INV ? bf.z + (size_t)cw * tb.n + (size_t)tb.t_row[t] * tb.Mr
                         : bf.beta + (size_t)cw * tb.LM + (size_t)tb.t_col[t] * tb.Mc;
    const double phi = INV ? bf.phi[(size_t)cw * tb.Lr + tb.t_row[t]] : 1.0;
    for (int idx = tid; idx < total; idx += nthr) {
        const int m1 = idx / CT, c = idx - m1 * CT;
        const int j = inmap[tb.Q * m1 + m2_0 + c];
        cxd v{0.0, 0.0};
        if (j >= 0) {
            v = src[j];
            if (INV) { v.x /= phi; v.y /= phi; }  // z / phi_use, sparc.py:972
        }
        d[idx] = v;
    }
    __syncthreads();
    lds_fft<double, INV, CAMP_EPT, true>(d, tb.log2P, CT, CT, 1, tb.twP, tid, nthr);
    cxd *out = bf.buf0 + ((size_t)cw * tb.nT + t) * tb.w;
    for (int idx = tid; idx < total; idx += nthr) {
        const int k1 = idx / CT, c = idx - k1 * CT;
        const int m2 = m2_0 + c;
        cxd tw = tb.twW[m2 * k1];
        if (INV) tw.y = -tw.y;
        out[(size_t)k1 * tb.Q + m2] = cmul(d[idx], tw);
    }
}

// ------------------------------------------------------------------ pass B
template <bool INV>
__device__ __forceinline__ void passB_tile(const CampTables &tb, const CampBufs &bf) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    cxd *d = reinterpret_cast<cxd *>(smem_raw);
    const int cw = blockIdx.z, t = blockIdx.y;
    if (!bf.active[cw]) return;
    const int nthr = blockDim.x, tid = threadIdx.x;
    const int total = tb.RT * tb.Q;
    const size_t off = ((size_t)cw * tb.nT + t) * tb.w + (size_t)blockIdx.x * total;
    for (int idx = tid; idx < total; idx += nthr) d[idx] = bf.buf0[off + idx];
    __syncthreads();
    lds_fft<double, INV, CAMP_EPT, false>(d, tb.log2Q, tb.RT, 1, tb.Q, tb.twQ, tid, nthr);
    for (int idx = tid; idx < total; idx += nthr) bf.buf1[off + idx] = d[idx];
}
template <bool INV>
__global__ __launch_bounds__(256) void cfft_passB(CampTables tb, CampBufs bf) {
    passB_tile<INV>(tb, bf);
}
// Long rows (w >= 2^17: P = 256, Q = 512 ... 4096): tiles of 4096 values, one
// row of Q = 4096 or several shorter ones, in 512 threads and 64 KB of LDS.
template <bool INV>
__global__ __launch_bounds__(512) void cfft_passB_long(CampTables tb, CampBufs bf) {
    passB_tile<INV>(tb, bf);
}

// ------------------------------------------------------------------ eta
// One wavefront per section, lane owns entries lane, lane + 64, ...  The
// section's x and then its numerators are staged in the lane's own beta
// entries, so any M runs without per-lane register arrays.  A known section
// keeps the one-hot the initialisation wrote: sum |beta|^2 = 1, its squared
// error against the truth, and the known (idx, sym) as the MAP decision.
__global__ __launch_bounds__(256) void camp_eta(CampTables tb, CampBufs bf) {
    const int cw = blockIdx.y;
    if (!bf.active[cw]) return;
    const int lane = threadIdx.x & 63;
    const int l = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (l >= tb.L) return;
    int k, ks;
    if (known_of(bf, (size_t)cw * tb.L + l, tb.M, &k, &ks)) {
        if (lane != 0) return;
        const size_t o = (size_t)cw * tb.L + l;
        const int truth = bf.true_idx ? bf.true_idx[o] : -1;
        // another entry than the transmitted one: 2; no truth: sum |beta|^2, as below
        double se = truth >= 0 && truth < tb.M ? 2.0 : 1.0;
        if (k == truth) {
            se = 0.0;
            if (bf.K > 1 && bf.true_sym) {
                const cxd a = bf.constel[ks], b = bf.constel[bf.true_sym[o]];
                se = (a.x - b.x) * (a.x - b.x) + (a.y - b.y) * (a.y - b.y);
            }
        }
        bf.sec_sumsq[o] = 1.0;
        bf.sec_err[o] = se;
        bf.sec_idx[o] = k;
        bf.sec_sym[o] = ks;
        return;
    }
    const int c = l / (tb.L / tb.Lc);
    const double tau = bf.tau[(size_t)cw * tb.Lc + c];
    const double th = tau / 2;  // s is complex: sparc.py:417-418
    const int K = bf.K;
    const cxd *cs = bf.constel;
    cxd *beta = bf.beta + (size_t)cw * tb.LM + (size_t)l * tb.M;
    const int jl0 = l * tb.M - c * tb.Mc;
    cxd *keep = bf.s_keep ? bf.s_keep + (size_t)cw * tb.LM + (size_t)l * tb.M : nullptr;  // soft output: the last s
    double m = -INFINITY;
    MapBest mb = map_init();
    for (int e = lane; e < tb.M; e += 64) {
        const cxd u = gather_az(tb, bf, cw, c, jl0 + e);
        const cxd b = beta[e];
        const cxd s{b.x + tau * u.x, b.y + tau * u.y};  // sparc.py:972
        const cxd x{s.x / th, s.y / th};
        if (keep) keep[e] = s;
        beta[e] = x;
        m = fmax(m, psk_shift(K, cs, x));
        map_update(K, cs, s, e, mb);
    }
    m = wave_max(m);
    int midx, msym;
    map_finish(K, mb, &midx, &msym);
    double den = 0.0;
    for (int e = lane; e < tb.M; e += 64) {
        cxd top;
        double dn;
        psk_terms(K, cs, beta[e], m, &top, &dn);
        beta[e] = top;
        den += dn;
    }
    den = wave_sum(den);
    const int truth = bf.true_idx ? bf.true_idx[(size_t)cw * tb.L + l] : -1;
    cxd tv{1.0, 0.0};
    if (K > 1 && bf.true_sym && truth >= 0) tv = cs[bf.true_sym[(size_t)cw * tb.L + l]];
    double ss = 0.0, se = 0.0;
    for (int e = lane; e < tb.M; e += 64) {
        const cxd top = beta[e];
        const cxd b{top.x / den, top.y / den};
        beta[e] = b;
        ss += b.x * b.x + b.y * b.y;
        const double dx = b.x - (e == truth ? tv.x : 0.0), dy = b.y - (e == truth ? tv.y : 0.0);
        se += dx * dx + dy * dy;
    }
    ss = wave_sum(ss);
    se = wave_sum(se);
    if (lane == 0) {
        const size_t o = (size_t)cw * tb.L + l;
        bf.sec_sumsq[o] = ss;
        bf.sec_err[o] = se;
        bf.sec_idx[o] = midx;
        bf.sec_sym[o] = msym;
    }
}

// ------------------------------------------------------------------ control
// gamma_r of psi (sparc.py:936-939): W psi for a flat design, else dot(W_r, psi) / Lc
__device__ __forceinline__ double gamma_of_psi(const CampTables &tb, const AmpParams &pr, const double *psi, int r) {
    if (tb.ndim == 0) return pr.W[0] * psi[0];
    double acc = 0.0;
    for (int c = 0; c < tb.Lc; ++c) acc += pr.W[r * tb.Lc + c] * psi[c];
    return acc / tb.Lc;
}

// The initialisation of codeword cw by its workgroup: beta = 0 (memset on host), nmse = 1.  With known sections
// also beta0 = c[sym] at entry idx of each, psi0_c = the share of unknown sections of column block c, and gamma0
// from psi0 as phase 0 forms every later gamma.
__device__ __forceinline__ void camp_init(const CampTables &tb, const CampBufs &bf, const AmpScalars &sc,
                                          const AmpParams &pr, int cw, int tid) {
    const int Lr = tb.Lr, Lc = tb.Lc;
    double *psi = sc.psi + (size_t)cw * Lc, *gamma = sc.gamma + (size_t)cw * Lr;
    double *nmse = sc.nmse + (size_t)cw * pr.t_max * Lc;
    for (int i = tid; i < pr.t_max * Lc; i += blockDim.x) nmse[i] = 1.0;
    if (tid == 0) { bf.active[cw] = 1; sc.t_final[cw] = 0; }
    if (!bf.known_idx) return;
    const int lane = tid & 63, spc = tb.L / Lc;
    for (int l = tid; l < tb.L; l += blockDim.x) {
        int k, ks;
        if (known_of(bf, (size_t)cw * tb.L + l, tb.M, &k, &ks))
            bf.beta[(size_t)cw * tb.LM + (size_t)l * tb.M + k] = bf.K > 1 ? bf.constel[ks] : cxd{1.0, 0.0};
    }
    for (int c = tid >> 6; c < Lc; c += blockDim.x >> 6) {  // one wavefront per column block
        double unk = 0.0;
        for (int l = c * spc + lane; l < (c + 1) * spc; l += 64) {
            int k, ks;
            unk += known_of(bf, (size_t)cw * tb.L + l, tb.M, &k, &ks) ? 0.0 : 1.0;
        }
        unk = wave_sum(unk);
        if (lane == 0) psi[c] = unk / spc;
    }
    __syncthreads();
    for (int r = tid; r < Lr; r += blockDim.x) gamma[r] = gamma_of_psi(tb, pr, psi, r);
}

// phase 0 (before Az, iteration t): Onsager residual and phi / tau
// (sparc.py:932-969); phase 1 (after eta): psi, NMSE, stopping
// (sparc.py:976-988); phase 2: initialisation (camp_init; taken before the
// other phases form their pointers, which keeps the kernel within 100 SGPRs
// and eight waves per SIMD).
__global__ __launch_bounds__(1024) void camp_control(CampTables tb, CampBufs bf, AmpScalars sc, AmpParams pr, int phase,
                                                     int t) {
    __shared__ double red[16];
    const int cw = blockIdx.x, tid = threadIdx.x;
    if (phase == 2) return camp_init(tb, bf, sc, pr, cw, tid);
    const int Lr = tb.Lr, Lc = tb.Lc;
    double *psi = sc.psi + (size_t)cw * Lc, *psi_prev = sc.psi_prev + (size_t)cw * Lc;
    double *phi = bf.phi + (size_t)cw * Lr, *phi_prev = sc.phi_prev + (size_t)cw * Lr;
    double *gamma = sc.gamma + (size_t)cw * Lr, *bco = sc.bcoef + (size_t)cw * Lr;
    double *tau = bf.tau + (size_t)cw * Lc;
    double *nmse = sc.nmse + (size_t)cw * pr.t_max * Lc;
    if (!bf.active[cw]) return;
    if (phase == 0) {
        cxd *z = bf.z + (size_t)cw * tb.n;
        const cxd *y = bf.y + (size_t)cw * tb.n;
        if (t > 0) {
            for (int r = tid; r < Lr; r += blockDim.x) {
                phi_prev[r] = phi[r];
                const double g = gamma_of_psi(tb, pr, psi, r);
                gamma[r] = g;
                bco[r] = g / phi[r];
            }
            __syncthreads();
            for (int c = tid; c < Lc; c += blockDim.x) psi_prev[c] = psi[c];
            for (int i = tid; i < tb.n; i += blockDim.x) {  // z = y - A beta + b z
                const int r = i / tb.Mr;
                const cxd ab = gather_ab(tb, bf, cw, r, i - r * tb.Mr);
                const double b = bco[r];
                const cxd yv = y[i], zv = z[i];
                z[i] = cxd{(yv.x - ab.x) + b * zv.x, (yv.y - ab.y) + b * zv.y};
            }
        } else if (bf.known_idx) {  // z0 = y - A beta0, no Onsager term; gamma0 is the initialisation's
            for (int i = tid; i < tb.n; i += blockDim.x) {
                const int r = i / tb.Mr;
                const cxd ab = gather_ab(tb, bf, cw, r, i - r * tb.Mr);
                const cxd yv = y[i];
                z[i] = cxd{yv.x - ab.x, yv.y - ab.y};
            }
        } else {
            for (int i = tid; i < tb.n; i += blockDim.x) z[i] = y[i];
            if (tid == 0) {
                if (tb.ndim == 0) gamma[0] = pr.W[0];
                else
                    for (int r = 0; r < Lr; ++r) {
                        double acc = 0.0;
                        for (int c = 0; c < Lc; ++c) acc += pr.W[r * Lc + c];
                        gamma[r] = acc / Lc;
                    }
            }
        }
        __syncthreads();
        if (pr.phi_method == 1) {
            if (tid == 0)
                for (int r = 0; r < Lr; ++r) phi[r] = pr.awgn_var + gamma[r];
        } else {  // mean |z|^2 per row block
            for (int r = 0; r < Lr; ++r) {
                double acc = 0.0;
                for (int i = r * tb.Mr + tid; i < (r + 1) * tb.Mr; i += blockDim.x) acc += z[i].x * z[i].x + z[i].y * z[i].y;
                acc = block_sum(acc, red);
                if (tid == 0) phi[r] = acc / (double)tb.Mr;
            }
        }
        __syncthreads();
        for (int c = tid; c < (tb.ndim == 0 ? 1 : Lc); c += blockDim.x) {
            if (tb.ndim == 0) tau[0] = (tb.L * phi[0] / tb.n) / pr.W[0];
            else if (tb.ndim == 1) tau[c] = (tb.L * phi[0] / tb.n) / pr.W[c];
            else {
                double acc = 0.0;
                for (int r = 0; r < Lr; ++r) acc += pr.W[r * Lc + c] * (1.0 / phi[r]);
                tau[c] = ((double)tb.L / tb.Mr) / acc;
            }
        }
        return;
    }
    // phase 1: psi / NMSE / stop
    const int spc = tb.L / Lc;
    const double denom = (tb.ndim == 0) ? (double)tb.L : ((double)tb.L / Lc);
    for (int c = 0; c < Lc; ++c) {
        double a = 0.0, e = 0.0;
        for (int l = c * spc + tid; l < (c + 1) * spc; l += blockDim.x) {
            a += bf.sec_sumsq[(size_t)cw * tb.L + l];
            e += bf.sec_err[(size_t)cw * tb.L + l];
        }
        a = block_sum(a, red);
        e = block_sum(e, red);
        if (tid == 0) {
            psi[c] = 1.0 - a / denom;
            nmse[(size_t)(t + 1) * Lc + c] = e / denom;
        }
    }
    __syncthreads();
    if (tid == 0) {
        bool stop = false;
        if (t > 0) {  // np.allclose(psi, psi_prev, rtol, atol), sparc.py:984
            stop = true;
            for (int c = 0; c < Lc; ++c)
                if (!(fabs(psi[c] - psi_prev[c]) <= pr.atol + pr.rtol * fabs(psi_prev[c]))) stop = false;
        }
        if (stop) {  // nmse[t:] = nmse[t]
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

// ------------------------------------------------------------------ operator outputs
__global__ void camp_rowsum(CampTables tb, CampBufs bf, cxd *out) {
    const int cw = blockIdx.y;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < tb.n; i += gridDim.x * blockDim.x) {
        const int r = i / tb.Mr;
        out[(size_t)cw * tb.n + i] = gather_ab(tb, bf, cw, r, i - r * tb.Mr);
    }
}
__global__ void camp_colgather(CampTables tb, CampBufs bf, cxd *out) {
    const int cw = blockIdx.y;
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < tb.LM; j += gridDim.x * blockDim.x) {
        const int c = j / tb.Mc;
        out[(size_t)cw * tb.LM + j] = gather_az(tb, bf, cw, c, j - c * tb.Mc);
    }
}

// ------------------------------------------------------------------ stand-alone estimators
__global__ __launch_bounds__(256) void psk_mmse_kernel(const cxd *__restrict__ x, int L, int M, int K,
                                                       const cxd *__restrict__ cs, cxd *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int l = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (l >= L) return;
    const cxd *xs = x + (size_t)l * M;
    double m = -INFINITY;
    for (int e = lane; e < M; e += 64) m = fmax(m, psk_shift(K, cs, xs[e]));
    m = wave_max(m);
    double den = 0.0;
    for (int e = lane; e < M; e += 64) {
        cxd top;
        double dn;
        psk_terms(K, cs, xs[e], m, &top, &dn);
        out[(size_t)l * M + e] = top;
        den += dn;
    }
    den = wave_sum(den);
    for (int e = lane; e < M; e += 64) {
        cxd &o = out[(size_t)l * M + e];
        o = cxd{o.x / den, o.y / den};
    }
}

__global__ __launch_bounds__(256) void psk_map_kernel(const cxd *__restrict__ sv, int L, int M, int K,
                                                      const cxd *__restrict__ cs, int32_t *__restrict__ idx,
                                                      int32_t *__restrict__ sym) {
    const int lane = threadIdx.x & 63;
    const int l = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (l >= L) return;
    MapBest mb = map_init();
    for (int e = lane; e < M; e += 64) map_update(K, cs, sv[(size_t)l * M + e], e, mb);
    int i, k;
    map_finish(K, mb, &i, &k);
    if (lane == 0) { idx[l] = i; sym[l] = k; }
}

}  // namespace

// ------------------------------------------------------------------ launchers
// Pass B runs in at most 256 threads (w <= 2^16), or in the long-row shape:
// tiles of exactly CAMP_LONG_TILE values in 512 threads, P = 256.
static bool camp_long_b(const CampTables &tb) {
    return tb.RT * tb.Q == CAMP_LONG_TILE && tb.P == 256 && tb.Q >= 512;
}
static int camp_check_geometry(const CampTables &tb) {
    const int totA = tb.P * tb.CT, totB = tb.RT * tb.Q;
    if (tb.P <= 0 || tb.Q <= 0 || tb.CT <= 0 || tb.RT <= 0 || (long long)tb.P * tb.Q != tb.w ||
        tb.P != (1 << tb.log2P) || tb.Q != (1 << tb.log2Q) || totA % CAMP_EPT || totB % CAMP_EPT ||
        totA / CAMP_EPT > 256 || (!camp_long_b(tb) && totB / CAMP_EPT > 256) || tb.Q % tb.CT || tb.P % tb.RT)
        return fail(SG_ERR_UNSUPPORTED, "complex FFT geometry P=%d Q=%d CT=%d RT=%d unsupported", tb.P, tb.Q, tb.CT,
                    tb.RT);
    return SG_OK;
}

// Once per plan, on the plan's device: the long-row pass B takes 64 KB of
// dynamic LDS, so its kernels' limit is raised here and not between launches.
int camp_prepare_fft(const CampTables &tb) {
    SG_TRY(camp_check_geometry(tb));
    if (!camp_long_b(tb)) return SG_OK;
    const int lds = (int)(sizeof(cxd) * CAMP_LONG_TILE);
    SG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&cfft_passB_long<false>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    SG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&cfft_passB_long<true>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    return SG_OK;
}

int camp_launch_fft(const CampTables &tb, const CampBufs &bf, bool inverse, hipStream_t s) {
    if (bf.B <= 0) return SG_OK;
    SG_TRY(camp_check_geometry(tb));
    const int totA = tb.P * tb.CT, totB = tb.RT * tb.Q;
    const bool longB = camp_long_b(tb);
    const dim3 gA(tb.Q / tb.CT, tb.nT, bf.B), gB(tb.P / tb.RT, tb.nT, bf.B);
    const size_t ldsA = sizeof(cxd) * totA, ldsB = sizeof(cxd) * totB;
    {
        ProfScope ps(inverse ? SG_PH_AZ_A : SG_PH_AB_A, s);
        if (inverse) hipLaunchKernelGGL(cfft_passA<true>, gA, dim3(totA / CAMP_EPT), ldsA, s, tb, bf);
        else hipLaunchKernelGGL(cfft_passA<false>, gA, dim3(totA / CAMP_EPT), ldsA, s, tb, bf);
    }
    SG_HIP(hipGetLastError());
    {
        ProfScope ps(inverse ? SG_PH_AZ_B : SG_PH_AB_B, s);
        if (longB) {
            if (inverse) hipLaunchKernelGGL(cfft_passB_long<true>, gB, dim3(totB / CAMP_EPT), ldsB, s, tb, bf);
            else hipLaunchKernelGGL(cfft_passB_long<false>, gB, dim3(totB / CAMP_EPT), ldsB, s, tb, bf);
        } else if (inverse) hipLaunchKernelGGL(cfft_passB<true>, gB, dim3(totB / CAMP_EPT), ldsB, s, tb, bf);
        else hipLaunchKernelGGL(cfft_passB<false>, gB, dim3(totB / CAMP_EPT), ldsB, s, tb, bf);
    }
    SG_HIP(hipGetLastError());
    return SG_OK;
}

int camp_launch_eta(const CampTables &tb, const CampBufs &bf, hipStream_t s) {
    if (bf.B <= 0) return SG_OK;
    const int waves = 4;
    ProfScope ps(SG_PH_ETA, s);
    hipLaunchKernelGGL(camp_eta, dim3((tb.L + waves - 1) / waves, bf.B), dim3(64 * waves), 0, s, tb, bf);
    SG_HIP(hipGetLastError());
    return SG_OK;
}

int camp_launch_control(const CampTables &tb, const CampBufs &bf, const AmpScalars &sc, const AmpParams &pr, int phase,
                        int t, hipStream_t s) {
    if (bf.B <= 0) return SG_OK;
    ProfScope ps(SG_PH_CONTROL, s);
    hipLaunchKernelGGL(camp_control, dim3(bf.B), dim3(1024), 0, s, tb, bf, sc, pr, phase, t);
    SG_HIP(hipGetLastError());
    return SG_OK;
}

int camp_launch_rowsum(const CampTables &tb, const CampBufs &bf, cxd *out, hipStream_t s) {
    hipLaunchKernelGGL(camp_rowsum, dim3((tb.n + 255) / 256, bf.B), dim3(256), 0, s, tb, bf, out);
    SG_HIP(hipGetLastError());
    return SG_OK;
}

int camp_launch_colgather(const CampTables &tb, const CampBufs &bf, cxd *out, hipStream_t s) {
    int gx = (tb.LM + 255) / 256;
    if (gx > 4096) gx = 4096;
    hipLaunchKernelGGL(camp_colgather, dim3(gx, bf.B), dim3(256), 0, s, tb, bf, out);
    SG_HIP(hipGetLastError());
    return SG_OK;
}

int camp_launch_mmse(const cxd *x, int L, int M, int K, const cxd *constel, cxd *out, hipStream_t s) {
    hipLaunchKernelGGL(psk_mmse_kernel, dim3((L + 3) / 4), dim3(256), 0, s, x, L, M, K, constel, out);
    SG_HIP(hipGetLastError());
    return SG_OK;
}

int camp_launch_map(const cxd *sv, int L, int M, int K, const cxd *constel, int32_t *idx, int32_t *sym, hipStream_t s) {
    hipLaunchKernelGGL(psk_map_kernel, dim3((L + 3) / 4), dim3(256), 0, s, sv, L, M, K, constel, idx, sym);
    SG_HIP(hipGetLastError());
    return SG_OK;
}

}  // namespace sg
