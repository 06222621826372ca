// Complex AMP with known sections (sg_camp_decode_partial_device, capi_camp.cpp): the kernels that turn the
// complex engine's loop (amp_cfft.hip; sparc.py:883-999) into the final pass of the three-stage concatenated
// K-PSK decoder, and the inverse of the section-word packing.  Double precision.
//
// The loop is the plain one with the denoiser of a known section replaced by its constellation one-hot, started
// from beta0 = the known one-hots and z0 = y - Ab(beta0).  It runs on the engine's own transforms, phase 1 of its
// control kernel, and from iteration 1 on its phase 0:
//
//   camp_part_init    beta0 = c[sym] at entry idx of every known section, psi0_c = the share of unknown sections
//                     of column block c, gamma0 from psi0 as the loop forms gamma from psi, nmse = 1, active
//   camp_part_start   iteration 0 after Ab(beta0): z0 = y - Ab(beta0), no Onsager term; phi and tau as phase 0
//   camp_part_eta     camp_eta on an unknown section; a known one keeps its one-hot and reports sum |beta|^2 = 1,
//                     its squared error against the truth, and the known (idx, sym) as the MAP decision
//   psk_unpack_kernel word -> (idx, sym), the inverse of psk_pack_kernel; a negative word is "unknown"
//
// A codeword that stopped is skipped by every kernel, so it keeps its state.  Fixed-order reductions, no atomics:
// a codeword's result does not depend on the batch it is decoded in.
#include <algorithm>

#include "camp_section.hpp"

namespace sg {
namespace {

constexpr int PB = 256;  // block size of the init kernel

// known (location, constellation index) of a section, or false: a location outside [0, M) is unknown, the
// constellation index is taken modulo K
__device__ __forceinline__ bool known_of(const int32_t *idx, const int32_t *sym, size_t o, int M, int K, int *k,
                                         int *ks) {
    *k = idx[o];
    *ks = K > 1 ? sym[o] & (K - 1) : 0;
    return *k >= 0 && *k < M;
}

// camp_eta's section update and camp_control's phi / tau step (amp_cfft.hip), restated here: called from a shared
// function those two kernels compile to other code, and they must stay what they are.
//
// One wavefront, lane owns entries lane, lane + 64, ... of section l of codeword cw.  The section's x and then its
// numerators are staged in the lane's own beta entries, so any M runs without per-lane register arrays.
__device__ __forceinline__ void camp_eta_section(const CampTables &tb, const CampBufs &bf, int cw, int l, int lane) {
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

// The end of camp_control's phase 0 (sparc.py:949-969), by the whole workgroup after a barrier behind the writes
// of gamma and z: phi by either method, then tau per column block.  red: one double per wave.
__device__ __forceinline__ void camp_phi_tau(const CampTables &tb, const AmpParams &pr, const cxd *z,
                                             const double *gamma, double *phi, double *tau, double *red) {
    const int tid = threadIdx.x, Lr = tb.Lr, Lc = tb.Lc;
    if (pr.phi_method == 1) {
        if (tid == 0)
            for (int r = 0; r < Lr; ++r) phi[r] = pr.awgn_var + gamma[r];
    } else {  // mean |z|^2 per row block
        for (int r = 0; r < Lr; ++r) {
            double acc = 0.0;
            for (int i = r * tb.Mr + tid; i < (r + 1) * tb.Mr; i += blockDim.x)
                acc += z[i].x * z[i].x + z[i].y * z[i].y;
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
}

// One workgroup per codeword.  beta was zeroed by the caller.
__global__ __launch_bounds__(PB) void camp_part_init(CampTables tb, CampBufs bf, AmpScalars sc, AmpParams pr,
                                                     const int32_t *__restrict__ known_idx,
                                                     const int32_t *__restrict__ known_sym) {
    const int cw = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int L = tb.L, Lr = tb.Lr, Lc = tb.Lc, spc = L / Lc;
    double *psi = sc.psi + (size_t)cw * Lc, *gamma = sc.gamma + (size_t)cw * Lr;
    double *nmse = sc.nmse + (size_t)cw * pr.t_max * Lc;
    for (int i = tid; i < pr.t_max * Lc; i += PB) nmse[i] = 1.0;
    for (int l = tid; l < L; l += PB) {
        int k, ks;
        if (known_of(known_idx, known_sym, (size_t)cw * L + l, tb.M, bf.K, &k, &ks))
            bf.beta[(size_t)cw * tb.LM + (size_t)l * tb.M + k] = bf.K > 1 ? bf.constel[ks] : cxd{1.0, 0.0};
    }
    for (int c = tid >> 6; c < Lc; c += PB / 64) {  // one wavefront per column block
        double unk = 0.0;
        for (int l = c * spc + lane; l < (c + 1) * spc; l += 64) {
            int k, ks;
            unk += known_of(known_idx, known_sym, (size_t)cw * L + l, tb.M, bf.K, &k, &ks) ? 0.0 : 1.0;
        }
        unk = wave_sum(unk);
        if (lane == 0) psi[c] = unk / spc;
    }
    __syncthreads();
    for (int r = tid; r < Lr; r += PB) {  // gamma of psi0, as camp_control forms it from psi
        if (tb.ndim == 0) gamma[r] = pr.W[0] * psi[0];
        else {
            double acc = 0.0;
            for (int c = 0; c < Lc; ++c) acc += pr.W[r * Lc + c] * psi[c];
            gamma[r] = acc / Lc;
        }
    }
    if (tid == 0) { bf.active[cw] = 1; sc.t_final[cw] = 0; }
}

// One workgroup per codeword, iteration 0: buf1 holds the forward transforms of beta0.
__global__ __launch_bounds__(1024) void camp_part_start(CampTables tb, CampBufs bf, AmpScalars sc, AmpParams pr) {
    __shared__ double red[16];
    const int cw = blockIdx.x, tid = threadIdx.x;
    if (!bf.active[cw]) return;
    cxd *z = bf.z + (size_t)cw * tb.n;
    const cxd *y = bf.y + (size_t)cw * tb.n;
    for (int i = tid; i < tb.n; i += blockDim.x) {  // z0 = y - A beta0
        const int r = i / tb.Mr;
        const cxd ab = gather_ab(tb, bf, cw, r, i - r * tb.Mr);
        const cxd yv = y[i];
        z[i] = cxd{yv.x - ab.x, yv.y - ab.y};
    }
    __syncthreads();
    camp_phi_tau(tb, pr, z, sc.gamma + (size_t)cw * tb.Lr, bf.phi + (size_t)cw * tb.Lr, bf.tau + (size_t)cw * tb.Lc,
                 red);
}

// One wavefront per section, as camp_eta.
__global__ __launch_bounds__(256) void camp_part_eta(CampTables tb, CampBufs bf, const int32_t *__restrict__ known_idx,
                                                     const int32_t *__restrict__ known_sym) {
    const int cw = blockIdx.y;
    if (!bf.active[cw]) return;
    const int lane = threadIdx.x & 63;
    const int l = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (l >= tb.L) return;
    const size_t o = (size_t)cw * tb.L + l;
    int k, ks;
    if (!known_of(known_idx, known_sym, o, tb.M, bf.K, &k, &ks)) {
        camp_eta_section(tb, bf, cw, l, lane);
        return;
    }
    if (lane != 0) return;  // known: beta stays the one-hot that camp_part_init wrote
    const int truth = bf.true_idx ? bf.true_idx[o] : -1;
    // another entry than the transmitted one: 2; no truth: sum |beta|^2, as eta
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
}

__global__ __launch_bounds__(256) void psk_unpack_kernel(const int32_t *__restrict__ word, size_t total, int logK,
                                                         int32_t *__restrict__ idx, int32_t *__restrict__ sym) {
    const int mK = (1 << logK) - 1;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int w = word[i];
        idx[i] = w < 0 ? -1 : w >> logK;
        if (sym) sym[i] = w < 0 ? 0 : gray_to_bin(w & mK);
    }
}

}  // namespace

int camp_part_launch_init(const CampTables &tb, const CampBufs &bf, const AmpScalars &sc, const AmpParams &pr,
                          const int32_t *known_idx, const int32_t *known_sym, hipStream_t s) {
    if (bf.B <= 0) return SG_OK;
    ProfScope ps(SG_PH_CONTROL, s);
    hipLaunchKernelGGL(camp_part_init, dim3(bf.B), dim3(PB), 0, s, tb, bf, sc, pr, known_idx, known_sym);
    SG_HIP(hipGetLastError());
    return SG_OK;
}

int camp_part_launch_start(const CampTables &tb, const CampBufs &bf, const AmpScalars &sc, const AmpParams &pr,
                           hipStream_t s) {
    if (bf.B <= 0) return SG_OK;
    ProfScope ps(SG_PH_CONTROL, s);
    hipLaunchKernelGGL(camp_part_start, dim3(bf.B), dim3(1024), 0, s, tb, bf, sc, pr);
    SG_HIP(hipGetLastError());
    return SG_OK;
}

int camp_part_launch_eta(const CampTables &tb, const CampBufs &bf, const int32_t *known_idx, const int32_t *known_sym,
                         hipStream_t s) {
    if (bf.B <= 0) return SG_OK;
    const int waves = 4;
    ProfScope ps(SG_PH_ETA, s);
    hipLaunchKernelGGL(camp_part_eta, dim3((tb.L + waves - 1) / waves, bf.B), dim3(64 * waves), 0, s, tb, bf, known_idx,
                       known_sym);
    SG_HIP(hipGetLastError());
    return SG_OK;
}

int camp_launch_unpack(const int32_t *word, int B, int L, int logK, int32_t *idx, int32_t *sym, hipStream_t s) {
    const size_t total = (size_t)B * L;
    if (total == 0) return SG_OK;
    const unsigned grid = (unsigned)std::min<size_t>(1024, (total + 255) / 256);
    hipLaunchKernelGGL(psk_unpack_kernel, dim3(grid), dim3(256), 0, s, word, total, logK, idx, sym);
    SG_HIP(hipGetLastError());
    return SG_OK;
}

}  // namespace sg
