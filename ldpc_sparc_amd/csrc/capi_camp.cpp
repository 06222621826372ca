// Host plan and C ABI of the complex AMP engine (amp_cfft.hip): complex SPARCs
// with the sub-sampled FFT design and K-PSK modulated message vectors, double
// precision.  Complex arrays cross the ABI as interleaved double[2].
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "amp_cfft.hpp"
#include "device_mem.hpp"

using namespace sg;

struct sg_camp_plan {
    int device = 0;
    int ndim = 0, L = 0, M = 0, LM = 0, n = 0, Lr = 1, Lc = 1, Mr = 0, Mc = 0, nT = 0;
    int w = 0, P = 0, Q = 0, log2P = 0, log2Q = 0, CT = 0, RT = 0;
    DevPool tables;  // design tables
    int32_t *t_row = nullptr, *t_col = nullptr, *col_ptr = nullptr, *col_t = nullptr, *row_ptr = nullptr,
            *row_t = nullptr, *in0 = nullptr, *in1 = nullptr, *pos0 = nullptr, *pos1 = nullptr;
    double *t_scale = nullptr, *dW = nullptr;
    cxd *twP = nullptr, *twQ = nullptr, *twW = nullptr, *constel = nullptr;
    // workspace of the largest (B, t_max) seen: one allocation carved below
    DevMem ws;
    int ws_B = 0, ws_tmax = 0;
    cxd *beta = nullptr, *y = nullptr, *z = nullptr, *buf0 = nullptr, *buf1 = nullptr, *io = nullptr;
    double *phi = nullptr, *tau = nullptr, *sec_sumsq = nullptr, *sec_err = nullptr, *psi = nullptr,
           *psi_prev = nullptr, *phi_prev = nullptr, *gamma = nullptr, *bco = nullptr, *nmse = nullptr;
    int32_t *active = nullptr, *sec_idx = nullptr, *sec_sym = nullptr, *true_idx = nullptr, *true_sym = nullptr,
            *t_final = nullptr;
    std::vector<cxd> h_constel;  // what `constel` holds (set_constel)
    // soft output (sg_camp_soft_output): s_keep is carved from ws by the next ensure_ws; last_B / last_K of the
    // last decode that filled it, 0 before any and after whatever overwrites or may move the workspace
    bool soft = false;
    cxd *s_keep = nullptr;
    int last_B = 0, last_K = 0;
    // known sections of sg_camp_decode_partial's host arrays [B][L], grow-only per (plan, B) (ensure_known)
    DevPool part;
    int part_B = 0;
    int32_t *known_idx = nullptr, *known_sym = nullptr;
};

namespace {

std::vector<cxd> twiddles(int len) {  // exp(-2 pi i e / len)
    std::vector<cxd> t(len);
    for (int e = 0; e < len; ++e) {
        const double a = -2.0 * M_PI * (double)e / (double)len;
        t[e] = cxd{std::cos(a), std::sin(a)};
    }
    // exact values on the axes
    t[0] = cxd{1.0, 0.0};
    if (len % 4 == 0) {
        t[len / 4] = cxd{0.0, -1.0};
        t[len / 2] = cxd{-1.0, 0.0};
        t[3 * len / 4] = cxd{0.0, 1.0};
    } else if (len % 2 == 0) {
        t[len / 2] = cxd{-1.0, 0.0};
    }
    return t;
}

int ensure_ws(sg_camp_plan *p, int B, int t_max) {
    if (p->ws.bytes() && B <= p->ws_B && t_max <= p->ws_tmax && (!p->soft || p->s_keep)) return SG_OK;
    B = std::max(B, p->ws_B);
    t_max = std::max(t_max, p->ws_tmax);
    p->ws.reset();
    p->s_keep = nullptr;
    p->ws_B = p->ws_tmax = 0;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t o = off;
        off += (bytes + 255) & ~(size_t)255;
        return o;
    };
    const size_t sB = (size_t)B, big = sB * std::max(p->LM, p->n);
    const size_t o_beta = take(sB * p->LM * sizeof(cxd)), o_y = take(sB * p->n * sizeof(cxd)),
                 o_z = take(sB * p->n * sizeof(cxd)), o_b0 = take(sB * p->nT * p->w * sizeof(cxd)),
                 o_b1 = take(sB * p->nT * p->w * sizeof(cxd)), o_io = take(big * sizeof(cxd)),
                 o_phi = take(sB * p->Lr * 8), o_tau = take(sB * p->Lc * 8), o_ss = take(sB * p->L * 8),
                 o_se = take(sB * p->L * 8), o_psi = take(sB * p->Lc * 8), o_psp = take(sB * p->Lc * 8),
                 o_php = take(sB * p->Lr * 8), o_gam = take(sB * p->Lr * 8), o_bco = take(sB * p->Lr * 8),
                 o_nm = take(sB * t_max * p->Lc * 8), o_act = take(sB * 4), o_si = take(sB * p->L * 4),
                 o_sy = take(sB * p->L * 4), o_ti = take(sB * p->L * 4), o_ts = take(sB * p->L * 4),
                 o_tf = take(sB * 4);
    const size_t o_keep = p->soft ? take(sB * p->LM * sizeof(cxd)) : 0;  // 16 LM bytes per codeword, only when on
    SG_TRY(p->ws.ensure(off));
    char *b = p->ws.at<char>();
    p->beta = (cxd *)(b + o_beta); p->y = (cxd *)(b + o_y); p->z = (cxd *)(b + o_z);
    p->buf0 = (cxd *)(b + o_b0); p->buf1 = (cxd *)(b + o_b1); p->io = (cxd *)(b + o_io);
    p->phi = (double *)(b + o_phi); p->tau = (double *)(b + o_tau);
    p->sec_sumsq = (double *)(b + o_ss); p->sec_err = (double *)(b + o_se);
    p->psi = (double *)(b + o_psi); p->psi_prev = (double *)(b + o_psp); p->phi_prev = (double *)(b + o_php);
    p->gamma = (double *)(b + o_gam); p->bco = (double *)(b + o_bco); p->nmse = (double *)(b + o_nm);
    p->active = (int32_t *)(b + o_act); p->sec_idx = (int32_t *)(b + o_si); p->sec_sym = (int32_t *)(b + o_sy);
    p->true_idx = (int32_t *)(b + o_ti); p->true_sym = (int32_t *)(b + o_ts); p->t_final = (int32_t *)(b + o_tf);
    if (p->soft) p->s_keep = (cxd *)(b + o_keep);
    p->ws_B = B;
    p->ws_tmax = t_max;
    return SG_OK;
}

int ensure_known(sg_camp_plan *p, int B) {
    if (B <= p->part_B) return SG_OK;
    p->part.release();
    p->part_B = 0;
    SG_TRY(p->part.alloc(&p->known_idx, sizeof(int32_t) * B * p->L));
    SG_TRY(p->part.alloc(&p->known_sym, sizeof(int32_t) * B * p->L));
    p->part_B = B;
    return SG_OK;
}

CampTables tables(const sg_camp_plan *p) {
    CampTables tb;
    tb.nT = p->nT; tb.w = p->w; tb.P = p->P; tb.Q = p->Q; tb.log2P = p->log2P; tb.log2Q = p->log2Q;
    tb.CT = p->CT; tb.RT = p->RT;
    tb.L = p->L; tb.M = p->M; tb.LM = p->LM; tb.n = p->n; tb.Lr = p->Lr; tb.Lc = p->Lc; tb.Mr = p->Mr; tb.Mc = p->Mc;
    tb.ndim = p->ndim;
    tb.t_row = p->t_row; tb.t_col = p->t_col; tb.t_scale = p->t_scale;
    tb.col_ptr = p->col_ptr; tb.col_t = p->col_t; tb.row_ptr = p->row_ptr; tb.row_t = p->row_t;
    tb.in1 = p->in1; tb.in0 = p->in0; tb.pos0 = p->pos0; tb.pos1 = p->pos1;
    tb.twP = p->twP; tb.twQ = p->twQ; tb.twW = p->twW;
    return tb;
}

CampBufs bufs(const sg_camp_plan *p, int B, int K) {
    CampBufs bf;
    bf.B = B; bf.K = K; bf.constel = p->constel;
    bf.beta = p->beta; bf.y = p->y; bf.z = p->z; bf.buf0 = p->buf0; bf.buf1 = p->buf1;
    bf.phi = p->phi; bf.tau = p->tau; bf.active = p->active;
    bf.sec_sumsq = p->sec_sumsq; bf.sec_err = p->sec_err; bf.sec_idx = p->sec_idx; bf.sec_sym = p->sec_sym;
    bf.true_idx = nullptr; bf.true_sym = nullptr;
    bf.s_keep = nullptr;  // only a decode with soft output on sets it
    bf.known_idx = bf.known_sym = nullptr;  // only a decode with known sections sets them
    return bf;
}

bool psk_order_ok(int K) { return K >= 1 && (K & (K - 1)) == 0; }

int psk_max_check(int K) {
    if (K > CAMP_MAX_K) return fail(SG_ERR_UNSUPPORTED, "K=%d-PSK: at most %d symbols are supported", K, CAMP_MAX_K);
    return SG_OK;
}

int psk_order_checks(int K) {
    SG_CHECK_ARG(psk_order_ok(K), "K must be 1 or a power of two");
    return psk_max_check(K);
}

// The refusals every decode shares: the scalar parameters, then the PSK order
int decode_param_checks(int K, double awgn_var, int t_max, double rtol, int phi_method) {
    SG_CHECK_ARG(t_max > 1, "t_max must be > 1 (sparc.py:168)");
    SG_CHECK_ARG(rtol > 0 && rtol < 1, "rtol must be in (0, 1)");
    SG_CHECK_ARG(phi_method == 1 || phi_method == 2, "phi_est_method must be 1 or 2");
    SG_CHECK_ARG(awgn_var >= 0, "awgn_var must be >= 0");
    return psk_order_checks(K);
}

int bits_per_section(int M, int K) {  // log2 M + log2 K
    int per = ilog2(M);
    for (int k = 1; k < K; k <<= 1) ++per;
    return per;
}

// Staging of the sg_section_*_psk host functions: x[L*M] (interleaved complex if is_complex, else real) as cxd in
// d and the constellation in dc, uploaded on s, with `extra` bytes for the results behind them (res).  It holds the
// host copy the upload reads, so it lives until the caller has synchronised s.
struct SectionStage {
    std::vector<cxd> hx;
    DevMem mem;
    cxd *d = nullptr, *dc = nullptr;
    void *res = nullptr;
    int upload(const double *x, size_t N, int is_complex, int K, const double *constel, size_t extra, hipStream_t s) {
        hx.resize(N);
        for (size_t i = 0; i < N; ++i) hx[i] = is_complex ? cxd{x[2 * i], x[2 * i + 1]} : cxd{x[i], 0.0};
        SG_TRY(mem.ensure((N + CAMP_MAX_K) * sizeof(cxd) + extra));
        d = mem.at<cxd>(); dc = d + N; res = dc + CAMP_MAX_K;
        SG_HIP(hipMemcpyAsync(d, hx.data(), N * sizeof(cxd), hipMemcpyHostToDevice, s));
        if (K > 1) SG_HIP(hipMemcpyAsync(dc, constel, (size_t)K * sizeof(cxd), hipMemcpyHostToDevice, s));
        return SG_OK;
    }
};

constexpr int CAMP_MAX_B = 65535;  // the batch is a grid dimension of every kernel

// The plan's device constellation, uploaded from the plan's own host copy (an
// asynchronous copy must not outlive the caller's array) when it changes.
int set_constel(sg_camp_plan *p, int K, const double *constel, hipStream_t s) {
    if (K <= 1) return SG_OK;
    const cxd *c = reinterpret_cast<const cxd *>(constel);
    if ((int)p->h_constel.size() == K && std::memcmp(p->h_constel.data(), c, (size_t)K * sizeof(cxd)) == 0)
        return SG_OK;
    SG_HIP(hipStreamSynchronize(s));  // an earlier upload may still read h_constel
    p->h_constel.assign(c, c + K);
    SG_HIP(hipMemcpyAsync(p->constel, p->h_constel.data(), (size_t)K * sizeof(cxd), hipMemcpyHostToDevice, s));
    return SG_OK;
}

// What the four decode entry points share, then body(): the device, the plan, the reset of the soft-output state
// (every decode call makes it; a completed plain decode sets the state again), the refusals of the batch and the
// scalars, hipSetDevice.  The plain entries refuse a negative batch and return on an empty one before they look at
// anything else; those with known sections (part) refuse the scalars first and return on any B <= 0.  Either then
// wants the arrays that every K needs (have, or the refusal `missing`); the checks that depend on K are body()'s.
template <class Body>
int decode_entry(sg_camp_plan *p, bool part, int B, int K, const double *constel, double awgn_var, int t_max,
                 double rtol, int phi_method, bool have, const char *missing, Body &&body) {
    SG_TRY(ensure_device());
    SG_CHECK_ARG(p, "plan is NULL");
    p->last_B = p->last_K = 0;
    if (part) {
        SG_CHECK_ARG(B <= CAMP_MAX_B, "batch must be at most 65535");
        SG_TRY(decode_param_checks(K, awgn_var, t_max, rtol, phi_method));
        SG_CHECK_ARG(K == 1 || constel, "K > 1 needs the constellation");
    } else {
        SG_CHECK_ARG(B >= 0 && B <= CAMP_MAX_B, "batch must be in [0, 65535]");
    }
    if (B <= 0) return SG_OK;
    SG_CHECK_ARG(have, "%s", missing);
    if (!part) SG_TRY(decode_param_checks(K, awgn_var, t_max, rtol, phi_method));
    SG_HIP(hipSetDevice(p->device));
    return body();
}

// What a decode is asked for, in the order of sg_camp_decode_partial_device's arguments (results: null if not
// wanted).  d_known_idx null is the plain decode; given (with d_known_sym for K > 1), those sections are known.
struct CampArgs {
    const void *d_y; int B, K; const double *constel;
    const int32_t *d_known_idx, *d_known_sym, *d_true_idx, *d_true_sym;
    double awgn_var; int t_max; double rtol; int phi_method;
    int32_t *d_map_idx, *d_map_sym, *d_t_final; double *d_nmse, *d_psi;
};

// The AMP decode on device arrays, after the entry point's refusals.  The known sections reach the kernels through
// CampBufs (amp_cfft.hpp); the driver's part is the forward transform of beta0 at iteration 0, which the plain decode
// (beta0 = 0) skips, and s_keep, which a decode with known sections does not refill.
int decode_impl(sg_camp_plan *p, const CampArgs &a, hipStream_t s) {
    const int B = a.B, K = a.K, t_max = a.t_max;
    const bool part = a.d_known_idx != nullptr;
    SG_TRY(ensure_ws(p, B, t_max));
    SG_TRY(set_constel(p, K, a.constel, s));
    const CampTables tb = tables(p);
    // y is only read (z = y at t = 0); outputs the caller does not want land in the workspace
    CampBufs bf = bufs(p, B, K);
    bf.y = (const cxd *)a.d_y;
    bf.sec_idx = a.d_map_idx ? a.d_map_idx : p->sec_idx;
    bf.sec_sym = a.d_map_sym ? a.d_map_sym : p->sec_sym;
    bf.true_idx = a.d_true_idx;
    bf.true_sym = (K > 1 && a.d_true_idx) ? a.d_true_sym : nullptr;
    bf.s_keep = (p->soft && !part) ? p->s_keep : nullptr;
    bf.known_idx = a.d_known_idx;
    bf.known_sym = K > 1 ? a.d_known_sym : nullptr;
    AmpScalars sc;
    sc.psi = a.d_psi ? a.d_psi : p->psi; sc.psi_prev = p->psi_prev; sc.phi_prev = p->phi_prev; sc.gamma = p->gamma;
    sc.bcoef = p->bco;
    sc.nmse = a.d_nmse ? a.d_nmse : p->nmse; sc.t_final = a.d_t_final ? a.d_t_final : p->t_final;
    AmpParams pr;
    pr.W = p->dW; pr.awgn_var = a.awgn_var; pr.rtol = a.rtol;
    pr.atol = 2e-15;  // 2*np.finfo(float).resolution, sparc.py:916
    pr.phi_method = a.phi_method; pr.t_max = t_max;
    SG_HIP(hipMemsetAsync(p->beta, 0, (size_t)B * p->LM * sizeof(cxd), s));
    SG_HIP(hipMemsetAsync(bf.sec_idx, 0, sizeof(int32_t) * B * p->L, s));
    SG_HIP(hipMemsetAsync(bf.sec_sym, 0, sizeof(int32_t) * B * p->L, s));
    SG_TRY(camp_launch_control(tb, bf, sc, pr, 2, 0, s));
    std::vector<int32_t> act(B);
    for (int t = 0; t < t_max - 1; ++t) {
        if (t > 0 || part) SG_TRY(camp_launch_fft(tb, bf, false, s));
        SG_TRY(camp_launch_control(tb, bf, sc, pr, 0, t, s));
        SG_TRY(camp_launch_fft(tb, bf, true, s));
        SG_TRY(camp_launch_eta(tb, bf, s));
        SG_TRY(camp_launch_control(tb, bf, sc, pr, 1, t, s));
        if (t % 4 == 3 && t + 1 < t_max - 1) {  // skip the remaining launches once every codeword stopped
            SG_HIP(hipMemcpyAsync(act.data(), p->active, sizeof(int32_t) * B, hipMemcpyDeviceToHost, s));
            SG_HIP(hipStreamSynchronize(s));
            int na = 0;
            for (int b = 0; b < B; ++b) na += act[b] != 0;
            if (na == 0) break;
        }
    }
    return SG_OK;
}

// upload -> decode_impl on the plan's own buffers -> download, after the entry point's refusals; known_idx null is
// the plain decode
int decode_host(sg_camp_plan *p, const double *y, int B, int K, const double *constel, const int32_t *known_idx,
                const int32_t *known_sym, const int32_t *true_idx, const int32_t *true_sym, double awgn_var, int t_max,
                double rtol, int phi_method, int32_t *map_idx, int32_t *map_sym, int32_t *t_final, double *nmse,
                double *psi) {
    const size_t nsec = (size_t)B * p->L;
    hipStream_t s = lib_stream();
    SG_TRY(ensure_ws(p, B, t_max));
    if (known_idx) SG_TRY(ensure_known(p, B));
    SG_HIP(hipMemcpyAsync(p->y, y, (size_t)B * p->n * sizeof(cxd), hipMemcpyHostToDevice, s));
    if (known_idx) {
        SG_HIP(hipMemcpyAsync(p->known_idx, known_idx, sizeof(int32_t) * nsec, hipMemcpyHostToDevice, s));
        if (K > 1) SG_HIP(hipMemcpyAsync(p->known_sym, known_sym, sizeof(int32_t) * nsec, hipMemcpyHostToDevice, s));
    }
    if (true_idx) {
        SG_HIP(hipMemcpyAsync(p->true_idx, true_idx, sizeof(int32_t) * nsec, hipMemcpyHostToDevice, s));
        if (K > 1) SG_HIP(hipMemcpyAsync(p->true_sym, true_sym, sizeof(int32_t) * nsec, hipMemcpyHostToDevice, s));
    }
    const CampArgs a{p->y, B, K, constel, known_idx ? p->known_idx : nullptr, known_idx ? p->known_sym : nullptr,
                     true_idx ? p->true_idx : nullptr, (true_idx && K > 1) ? p->true_sym : nullptr, awgn_var, t_max,
                     rtol, phi_method, p->sec_idx, p->sec_sym, p->t_final, p->nmse, p->psi};
    SG_TRY(decode_impl(p, a, s));
    SG_HIP(hipMemcpyAsync(map_idx, p->sec_idx, sizeof(int32_t) * nsec, hipMemcpyDeviceToHost, s));
    if (map_sym) SG_HIP(hipMemcpyAsync(map_sym, p->sec_sym, sizeof(int32_t) * nsec, hipMemcpyDeviceToHost, s));
    SG_HIP(hipMemcpyAsync(t_final, p->t_final, sizeof(int32_t) * B, hipMemcpyDeviceToHost, s));
    SG_HIP(hipMemcpyAsync(nmse, p->nmse, sizeof(double) * B * t_max * p->Lc, hipMemcpyDeviceToHost, s));
    SG_HIP(hipMemcpyAsync(psi, p->psi, sizeof(double) * B * p->Lc, hipMemcpyDeviceToHost, s));
    SG_HIP(hipStreamSynchronize(s));
    return SG_OK;
}

}  // namespace

extern "C" {

int sg_camp_plan_destroy(sg_camp_plan *p) {
    delete p;
    return SG_OK;
}

int sg_camp_plan_create(int ndim, const double *W, int Lr_in, int Lc_in, int L, int M, int n, const uint32_t *order0,
                        const uint32_t *order1, sg_camp_plan **out) {
    SG_TRY(ensure_device());
    SG_CHECK_ARG(out && W && order0 && order1, "null argument");
    SG_CHECK_ARG(ndim >= 0 && ndim <= 2, "W.ndim must be 0, 1 or 2");
    SG_CHECK_ARG(L > 0 && M > 0 && n > 0 && (M & (M - 1)) == 0, "bad (L, M, n)");
    int Lr = 1, Lc = 1;
    if (ndim == 1) Lc = Lc_in;
    if (ndim == 2) { Lr = Lr_in; Lc = Lc_in; }
    SG_CHECK_ARG(Lr >= 1 && Lc >= 1, "bad base-matrix shape");
    const long long LM = (long long)L * M;
    SG_CHECK_ARG(LM < (1LL << 30), "L*M too large");
    SG_CHECK_ARG(L % Lc == 0, "Lc must divide L");
    SG_CHECK_ARG(ndim != 2 || n % Lr == 0, "Lr must divide n");
    const int Mr = (ndim == 2) ? n / Lr : n;
    const int Mc = (int)(LM / Lc);
    int lg = 0;
    while ((1LL << lg) < std::max(Mr + 2, Mc + 2)) ++lg;  // sparc.py:618,748
    if (lg < CAMP_MIN_LOG2W || lg > CAMP_MAX_LOG2W)
        return fail(SG_ERR_UNSUPPORTED, "complex transform size w=2^%d outside [2^%d, 2^%d]", lg, CAMP_MIN_LOG2W,
                    CAMP_MAX_LOG2W);
    std::unique_ptr<sg_camp_plan, int (*)(sg_camp_plan *)> p(new sg_camp_plan(), sg_camp_plan_destroy);
    hipGetDevice(&p->device);
    p->ndim = ndim; p->L = L; p->M = M; p->LM = (int)LM; p->n = n; p->Lr = Lr; p->Lc = Lc; p->Mr = Mr; p->Mc = Mc;
    const int w = 1 << lg;
    p->w = w;
    // square split up to 2^16; above, P stays 256 and pass B takes long rows (amp_cfft.hpp)
    p->log2P = lg <= CAMP_SQUARE_MAX_LOG2W ? lg / 2 : 8;
    p->log2Q = lg - p->log2P;
    p->P = 1 << p->log2P; p->Q = 1 << p->log2Q;
    p->CT = std::min(8, p->Q);
    p->RT = lg <= CAMP_SQUARE_MAX_LOG2W ? std::min(8, p->P) : CAMP_LONG_TILE / p->Q;
    std::vector<double> Wv(W, W + (ndim == 0 ? 1 : (size_t)Lr * Lc));
    // transforms = nonzero blocks in row-major order (sparc.py:758-771)
    std::vector<int32_t> t_row, t_col;
    std::vector<double> t_scale;
    for (int r = 0; r < Lr; ++r)
        for (int c = 0; c < Lc; ++c) {
            const double wv = (ndim == 0) ? Wv[0] : Wv[(size_t)r * Lc + c];
            SG_CHECK_ARG(wv >= 0.0, "negative base-matrix entry");
            if (wv != 0.0) {
                t_row.push_back(r); t_col.push_back(c);
                t_scale.push_back(std::sqrt(wv / L));  // np.sqrt(W/L)
            }
        }
    const int nT = p->nT = (int)t_row.size();
    SG_CHECK_ARG(nT > 0, "base matrix is all zero");
    SG_CHECK_ARG((long long)nT * w < (1LL << 31), "design too large");
    std::vector<int32_t> col_ptr(Lc + 1, 0), col_t, row_ptr(Lr + 1, 0), row_t;
    for (int c = 0; c < Lc; ++c) {
        for (int t = 0; t < nT; ++t)
            if (t_col[t] == c) col_t.push_back(t);
        col_ptr[c + 1] = (int32_t)col_t.size();
    }
    for (int r = 0; r < Lr; ++r) {
        for (int t = 0; t < nT; ++t)
            if (t_row[t] == r) row_t.push_back(t);
        row_ptr[r + 1] = (int32_t)row_t.size();
    }
    std::vector<int32_t> in0((size_t)nT * w, -1), in1((size_t)nT * w, -1), pos0((size_t)nT * Mr), pos1((size_t)nT * Mc);
    const int P = p->P, Q = p->Q;
    for (int t = 0; t < nT; ++t) {
        for (int i = 0; i < Mr; ++i) {
            const uint32_t k = order0[(size_t)t * Mr + i];
            SG_CHECK_ARG(k < (uint32_t)w && in0[(size_t)t * w + k] < 0, "order0 entry out of range or repeated");
            in0[(size_t)t * w + k] = i;
            pos0[(size_t)t * Mr + i] = (int32_t)((k % P) * Q + k / P);
        }
        for (int j = 0; j < Mc; ++j) {
            const uint32_t k = order1[(size_t)t * Mc + j];
            SG_CHECK_ARG(k < (uint32_t)w && in1[(size_t)t * w + k] < 0, "order1 entry out of range or repeated");
            in1[(size_t)t * w + k] = j;
            pos1[(size_t)t * Mc + j] = (int32_t)((k % P) * Q + k / P);
        }
    }
    sg_camp_plan *q = p.get();
    DevPool &tb = q->tables;
    SG_TRY(tb.upload(&q->t_row, t_row)); SG_TRY(tb.upload(&q->t_col, t_col)); SG_TRY(tb.upload(&q->t_scale, t_scale));
    SG_TRY(tb.upload(&q->col_ptr, col_ptr)); SG_TRY(tb.upload(&q->col_t, col_t));
    SG_TRY(tb.upload(&q->row_ptr, row_ptr)); SG_TRY(tb.upload(&q->row_t, row_t));
    SG_TRY(tb.upload(&q->in0, in0)); SG_TRY(tb.upload(&q->in1, in1));
    SG_TRY(tb.upload(&q->pos0, pos0)); SG_TRY(tb.upload(&q->pos1, pos1));
    SG_TRY(tb.upload(&q->dW, Wv));
    SG_TRY(tb.upload(&q->twP, twiddles(P))); SG_TRY(tb.upload(&q->twQ, twiddles(Q)));
    SG_TRY(tb.upload(&q->twW, twiddles(w)));
    SG_TRY(tb.upload(&q->constel, std::vector<cxd>(CAMP_MAX_K, cxd{1.0, 0.0})));
    SG_TRY(camp_prepare_fft(tables(q)));
    *out = p.release();
    return SG_OK;
}

int sg_camp_plan_info(const sg_camp_plan *p, int *w, int *nT, int *Mr, int *Mc, int *P, int *Q) {
    SG_CHECK_ARG(p, "plan is NULL");
    if (w) *w = p->w;
    if (nT) *nT = p->nT;
    if (Mr) *Mr = p->Mr;
    if (Mc) *Mc = p->Mc;
    if (P) *P = p->P;
    if (Q) *Q = p->Q;
    return SG_OK;
}

int sg_camp_apply(sg_camp_plan *p, int transpose, const double *in, int B, double *out) {
    SG_TRY(ensure_device());
    SG_CHECK_ARG(p && in && out, "null argument");
    SG_CHECK_ARG(B >= 0, "negative batch");
    if (B == 0) return SG_OK;
    p->last_B = p->last_K = 0;  // works in the decode's buffers
    SG_HIP(hipSetDevice(p->device));
    hipStream_t s = lib_stream();
    SG_TRY(ensure_ws(p, B, 2));
    const CampTables tb = tables(p);
    const CampBufs bf = bufs(p, B, 1);
    const size_t nin = (size_t)B * (transpose ? p->n : p->LM), nout = (size_t)B * (transpose ? p->LM : p->n);
    const std::vector<int32_t> ones(B, 1);
    SG_HIP(hipMemcpyAsync(p->active, ones.data(), sizeof(int32_t) * B, hipMemcpyHostToDevice, s));
    SG_HIP(hipMemcpyAsync(transpose ? p->z : p->beta, in, nin * sizeof(cxd), hipMemcpyHostToDevice, s));
    const std::vector<double> ph((size_t)B * p->Lr, 1.0);
    if (transpose) SG_HIP(hipMemcpyAsync(p->phi, ph.data(), sizeof(double) * ph.size(), hipMemcpyHostToDevice, s));
    SG_TRY(camp_launch_fft(tb, bf, transpose != 0, s));
    if (transpose) SG_TRY(camp_launch_colgather(tb, bf, p->io, s));
    else SG_TRY(camp_launch_rowsum(tb, bf, p->io, s));
    SG_HIP(hipMemcpyAsync(out, p->io, nout * sizeof(cxd), hipMemcpyDeviceToHost, s));
    SG_HIP(hipStreamSynchronize(s));  // (also keeps the host vectors above alive long enough)
    return SG_OK;
}

int sg_camp_decode_device(sg_camp_plan *p, const void *d_y, int B, int K, const double *constel,
                          const int32_t *d_true_idx, const int32_t *d_true_sym, double awgn_var, int t_max, double rtol,
                          int phi_method, int32_t *d_map_idx, int32_t *d_map_sym, int32_t *d_t_final, double *d_nmse,
                          double *d_psi, void *stream) {
    return decode_entry(p, false, B, K, constel, awgn_var, t_max, rtol, phi_method, d_y != nullptr,
                        "null received words", [&]() -> int {
        SG_CHECK_ARG(K == 1 || constel, "K > 1 needs the constellation");
        SG_CHECK_ARG(K == 1 || !d_true_idx || d_true_sym, "K > 1 with true_idx needs true_sym");
        const CampArgs a{d_y, B, K, constel, nullptr, nullptr, d_true_idx, d_true_sym, awgn_var, t_max, rtol,
                         phi_method, d_map_idx, d_map_sym, d_t_final, d_nmse, d_psi};
        SG_TRY(decode_impl(p, a, pick_stream(stream)));
        if (p->soft) { p->last_B = B; p->last_K = K; }
        return SG_OK;
    });
}

// The decode with the known sections given: sg_camp_decode_device's driver; the soft-output state stays cleared
// (the loop overwrites what a decode left, and s_keep is not refilled)
int sg_camp_decode_partial_device(sg_camp_plan *p, const void *d_y, int B, int K, const double *constel,
                                  const int32_t *d_known_idx, const int32_t *d_known_sym, const int32_t *d_true_idx,
                                  const int32_t *d_true_sym, double awgn_var, int t_max, double rtol, int phi_method,
                                  int32_t *d_map_idx, int32_t *d_map_sym, int32_t *d_t_final, double *d_nmse,
                                  double *d_psi, void *stream) {
    return decode_entry(p, true, B, K, constel, awgn_var, t_max, rtol, phi_method, d_y && d_known_idx,
                        "d_y or d_known_idx is NULL", [&]() -> int {
        SG_CHECK_ARG(K == 1 || d_known_sym, "K > 1 needs d_known_sym");
        SG_CHECK_ARG(K == 1 || !d_true_idx || d_true_sym, "K > 1 with true_idx needs true_sym");
        const CampArgs a{d_y, B, K, constel, d_known_idx, d_known_sym, d_true_idx, d_true_sym, awgn_var, t_max, rtol,
                         phi_method, d_map_idx, d_map_sym, d_t_final, d_nmse, d_psi};
        return decode_impl(p, a, pick_stream(stream));
    });
}

int sg_camp_decode(sg_camp_plan *p, const double *y, int B, int K, const double *constel, const int32_t *true_idx,
                   const int32_t *true_sym, double awgn_var, int t_max, double rtol, int phi_method, int32_t *map_idx,
                   int32_t *map_sym, int32_t *t_final, double *nmse, double *psi) {
    return decode_entry(p, false, B, K, constel, awgn_var, t_max, rtol, phi_method,
                        y && map_idx && t_final && nmse && psi, "null host buffer", [&]() -> int {
        SG_CHECK_ARG(K == 1 || (constel && map_sym), "K > 1 needs the constellation and map_sym");
        SG_CHECK_ARG(K == 1 || !true_idx || true_sym, "K > 1 with true_idx needs true_sym");
        if (true_idx)
            for (size_t i = 0; i < (size_t)B * p->L; ++i) {
                SG_CHECK_ARG(true_idx[i] >= 0 && true_idx[i] < p->M, "true_idx out of range");
                SG_CHECK_ARG(K == 1 || (true_sym[i] >= 0 && true_sym[i] < K), "true_sym out of range");
            }
        SG_TRY(decode_host(p, y, B, K, constel, nullptr, nullptr, true_idx, true_sym, awgn_var, t_max, rtol,
                           phi_method, map_idx, map_sym, t_final, nmse, psi));
        if (p->soft) { p->last_B = B; p->last_K = K; }
        return SG_OK;
    });
}

int sg_camp_decode_partial(sg_camp_plan *p, const double *y, int B, int K, const double *constel,
                           const int32_t *known_idx, const int32_t *known_sym, const int32_t *true_idx,
                           const int32_t *true_sym, double awgn_var, int t_max, double rtol, int phi_method,
                           int32_t *map_idx, int32_t *map_sym, int32_t *t_final, double *nmse, double *psi) {
    return decode_entry(p, true, B, K, constel, awgn_var, t_max, rtol, phi_method,
                        y && known_idx && map_idx && t_final && nmse && psi, "null host buffer", [&]() -> int {
        SG_CHECK_ARG(K == 1 || (known_sym && map_sym), "K > 1 needs known_sym and map_sym");
        SG_CHECK_ARG(K == 1 || !true_idx || true_sym, "K > 1 with true_idx needs true_sym");
        for (size_t i = 0; i < (size_t)B * p->L; ++i) {
            SG_CHECK_ARG(known_idx[i] >= -1 && known_idx[i] < p->M, "known_idx[%zu] = %d outside [-1, %d)", i,
                         (int)known_idx[i], p->M);
            SG_CHECK_ARG(K == 1 || known_idx[i] < 0 || (known_sym[i] >= 0 && known_sym[i] < K),
                         "known_sym[%zu] = %d outside [0, %d)", i, K > 1 ? (int)known_sym[i] : 0, K);
            if (true_idx) {
                SG_CHECK_ARG(true_idx[i] >= 0 && true_idx[i] < p->M, "true_idx out of range");
                SG_CHECK_ARG(K == 1 || (true_sym[i] >= 0 && true_sym[i] < K), "true_sym out of range");
            }
        }
        return decode_host(p, y, B, K, constel, known_idx, known_sym, true_idx, true_sym, awgn_var, t_max, rtol,
                           phi_method, map_idx, map_sym, t_final, nmse, psi);
    });
}

int sg_bits_to_psk_sections_device(const uint8_t *d_bits, int B, int L, int logM, int logK, int32_t *d_idx,
                                   int32_t *d_sym, void *stream) {
    SG_CHECK_ARG(d_bits && d_idx, "null device buffer");
    SG_CHECK_ARG(B >= 0 && B <= CAMP_MAX_B && L >= 0, "bad (B, L)");
    SG_CHECK_ARG(logM >= 0 && logM <= 30 && logK >= 0 && logK <= 30 && logM + logK >= 1, "bad (logM, logK)");
    SG_CHECK_ARG(logK == 0 || d_sym, "logK > 0 needs d_sym");
    if (!B || !L) return SG_OK;
    SG_TRY(ensure_device());
    return camp_launch_bits_to_psk(d_bits, B, L, logM, logK, d_idx, d_sym, pick_stream(stream));
}

int sg_camp_encode_device(sg_camp_plan *p, int K, const double *constel, const int32_t *d_idx, const int32_t *d_sym,
                          int B, void *d_x, void *stream) {
    SG_TRY(ensure_device());
    SG_CHECK_ARG(p && d_idx && d_x, "null argument");
    SG_CHECK_ARG(B >= 0 && B <= CAMP_MAX_B, "batch must be in [0, 65535]");
    if (B == 0) return SG_OK;
    SG_TRY(psk_order_checks(K));
    SG_CHECK_ARG(K == 1 || (constel && d_sym), "K > 1 needs the constellation and d_sym");
    p->last_B = p->last_K = 0;  // overwrites beta
    SG_HIP(hipSetDevice(p->device));
    hipStream_t s = pick_stream(stream);
    SG_TRY(ensure_ws(p, B, 2));
    SG_TRY(set_constel(p, K, constel, s));
    const CampTables tb = tables(p);
    const CampBufs bf = bufs(p, B, K);
    SG_TRY(camp_launch_scatter(tb, bf, d_idx, d_sym, s));
    SG_TRY(camp_launch_fft(tb, bf, false, s));
    return camp_launch_rowsum(tb, bf, (cxd *)d_x, s);
}

int sg_camp_count_errors_device(const int32_t *d_map_idx, const int32_t *d_map_sym, const int32_t *d_true_idx,
                                const int32_t *d_true_sym, const int32_t *d_t_final, int B, int L, int logM, int logK,
                                int64_t *d_counts, int32_t *d_rows, void *stream) {
    SG_CHECK_ARG(d_map_idx && d_true_idx && d_t_final && d_counts, "null device buffer");
    SG_CHECK_ARG(B >= 0 && L >= 0, "bad (B, L)");
    SG_CHECK_ARG(logM >= 0 && logM <= 30 && logK >= 0 && logK <= 30, "bad (logM, logK)");
    SG_CHECK_ARG(logK == 0 || (d_map_sym && d_true_sym), "logK > 0 needs the constellation indices");
    SG_TRY(ensure_device());
    return camp_launch_count(d_map_idx, d_map_sym, d_true_idx, d_true_sym, d_t_final, B, L, logM, logK, d_counts,
                             d_rows, pick_stream(stream));
}

// x[L*M] (interleaved complex if x_is_complex, else real) holds s / tau with
// tau already halved for complex s; out[L*M] is interleaved complex.
int sg_section_mmse_psk(const double *x, int L, int M, int K, const double *constel, int x_is_complex, double *out) {
    SG_CHECK_ARG(x && out && L >= 0 && M > 0, "bad arguments");
    SG_CHECK_ARG(psk_order_ok(K) && (K == 1 || constel), "K must be 1 or a power of two with its constellation");
    SG_TRY(psk_max_check(K));
    if (L == 0) return SG_OK;
    SG_TRY(ensure_device());
    hipStream_t s = lib_stream();
    const size_t N = (size_t)L * M;
    SectionStage st;
    SG_TRY(st.upload(x, N, x_is_complex, K, constel, N * sizeof(cxd), s));
    cxd *dout = (cxd *)st.res;
    SG_TRY(camp_launch_mmse(st.d, L, M, K, st.dc, dout, s));
    SG_HIP(hipMemcpyAsync(out, dout, N * sizeof(cxd), hipMemcpyDeviceToHost, s));
    SG_HIP(hipStreamSynchronize(s));
    return SG_OK;
}

// s[L*M] as above; idx[L] the MAP location, sym[L] the constellation index
// (0 for K = 1; may be NULL then).
int sg_section_map_psk(const double *sv, int L, int M, int K, const double *constel, int s_is_complex, int32_t *idx,
                       int32_t *sym) {
    SG_CHECK_ARG(sv && idx && L >= 0 && M > 0, "bad arguments");
    SG_CHECK_ARG(psk_order_ok(K) && (K == 1 || (constel && sym)), "K must be 1 or a power of two with its constellation");
    SG_TRY(psk_max_check(K));
    if (L == 0) return SG_OK;
    SG_TRY(ensure_device());
    hipStream_t s = lib_stream();
    std::vector<int32_t> hsym(L);
    SectionStage st;
    SG_TRY(st.upload(sv, (size_t)L * M, s_is_complex, K, constel, 2 * (size_t)L * sizeof(int32_t), s));
    int32_t *di = (int32_t *)st.res, *dsym = di + L;
    SG_TRY(camp_launch_map(st.d, L, M, K, st.dc, di, dsym, s));
    SG_HIP(hipMemcpyAsync(idx, di, (size_t)L * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    SG_HIP(hipMemcpyAsync(hsym.data(), dsym, (size_t)L * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    SG_HIP(hipStreamSynchronize(s));
    if (sym) std::memcpy(sym, hsym.data(), (size_t)L * sizeof(int32_t));
    return SG_OK;
}

// ------------------------------------------------------------------ soft output
int sg_camp_soft_output(sg_camp_plan *p, int on) {
    SG_TRY(ensure_device());
    SG_CHECK_ARG(p, "plan is NULL");
    p->soft = on != 0;
    p->last_B = p->last_K = 0;  // s_keep is filled by the next decode
    return SG_OK;
}

}  // extern "C"

// Every refusal of sg_camp_llr*: the state the last decode left must be the one asked for.
static int camp_llr_checks(sg_camp_plan *p, int B, int K, const double *constel, int l0, int nl, long long llr_ld,
                           int *per_out) {
    SG_CHECK_ARG(p->soft, "soft output is off: sg_camp_soft_output(plan, 1) before the decode");
    SG_CHECK_ARG(p->last_B > 0 && p->s_keep, "no decode through this plan yet (or its state was overwritten)");
    SG_CHECK_ARG(B == p->last_B, "B = %d, but the last decode held %d codewords", B, p->last_B);
    SG_CHECK_ARG(K == p->last_K, "K = %d, but the last decode ran K = %d", K, p->last_K);
    SG_CHECK_ARG(K == 1 || constel, "K > 1 needs the constellation");
    SG_CHECK_ARG(p->M >= 2, "section size M = %d must be a power of two >= 2", p->M);
    if (p->M > 2048) return fail(SG_ERR_UNSUPPORTED, "bit LLRs of sections of M = %d > 2048 entries", p->M);
    *per_out = bits_per_section(p->M, K);
    return section_range_check(p->L, l0, nl, llr_ld, *per_out, "(log2 M + log2 K)");
}

extern "C" {

int sg_camp_llr_device(sg_camp_plan *p, int B, int K, const double *constel, int l0, int nl, int llr_ld,
                       int probs_only, double *d_llr, void *stream) {
    SG_TRY(ensure_device());
    SG_CHECK_ARG(p && d_llr, "null argument");
    int per = 0;
    SG_TRY(camp_llr_checks(p, B, K, constel, l0, nl, llr_ld, &per));
    SG_HIP(hipSetDevice(p->device));
    hipStream_t s = pick_stream(stream);
    SG_TRY(set_constel(p, K, constel, s));  // the decode's own: nothing moves
    return camp_launch_llr(p->s_keep, p->tau, B, p->L, p->Lc, p->M, K, p->constel, l0, nl, llr_ld, probs_only, d_llr, s);
}

int sg_camp_llr(sg_camp_plan *p, int B, int K, const double *constel, int l0, int nl, int probs_only, double *out) {
    SG_TRY(ensure_device());
    SG_CHECK_ARG(p && out, "null argument");
    int per = 0;
    SG_TRY(camp_llr_checks(p, B, K, constel, l0, nl, INT32_MAX, &per));
    const size_t ld = (size_t)nl * per, nv = (size_t)B * ld;
    if (nv == 0) return SG_OK;
    SG_CHECK_ARG(ld <= (size_t)INT32_MAX, "too many bits per codeword");
    SG_HIP(hipSetDevice(p->device));
    hipStream_t s = lib_stream();
    DevMem mem;  // staging of its own: the plan's buffers hold the state being read
    SG_TRY(mem.ensure(nv * sizeof(double)));
    double *d = mem.at<double>();
    SG_TRY(set_constel(p, K, constel, s));
    SG_TRY(camp_launch_llr(p->s_keep, p->tau, B, p->L, p->Lc, p->M, K, p->constel, l0, nl, (int)ld, probs_only, d, s));
    SG_HIP(hipMemcpyAsync(out, d, nv * sizeof(double), hipMemcpyDeviceToHost, s));
    SG_HIP(hipStreamSynchronize(s));
    return SG_OK;
}

// x as sg_section_mmse_psk; out [L][log2 M + log2 K]: P(bit = 0) of the section bits, or their clipped LLRs
int sg_section_llr_psk(const double *x, int L, int M, int K, const double *constel, int x_is_complex, int probs_only,
                       double *out) {
    SG_TRY(ensure_device());
    SG_CHECK_ARG(x && out && L >= 0, "bad arguments");
    SG_CHECK_ARG(M >= 2 && (M & (M - 1)) == 0, "section size M = %d must be a power of two >= 2", M);
    SG_CHECK_ARG(psk_order_ok(K) && (K == 1 || constel), "K must be 1 or a power of two with its constellation");
    SG_TRY(psk_max_check(K));
    if (M > 2048) return fail(SG_ERR_UNSUPPORTED, "bit LLRs of sections of M = %d > 2048 entries", M);
    if (L == 0) return SG_OK;
    hipStream_t s = lib_stream();
    const size_t nout = (size_t)L * bits_per_section(M, K);
    SectionStage st;
    SG_TRY(st.upload(x, (size_t)L * M, x_is_complex, K, constel, nout * sizeof(double), s));
    double *dout = (double *)st.res;
    // one "codeword" of L sections, x given: no tau
    SG_TRY(camp_launch_llr(st.d, nullptr, 1, L, 1, M, K, st.dc, 0, L, (int)nout, probs_only, dout, s));
    SG_HIP(hipMemcpyAsync(out, dout, nout * sizeof(double), hipMemcpyDeviceToHost, s));
    SG_HIP(hipStreamSynchronize(s));
    return SG_OK;
}

int sg_bits_to_psk_sections_strided_device(const uint8_t *d_bits, size_t bit_stride, int B, int L, int logM, int logK,
                                           int32_t *d_idx, int32_t *d_sym, size_t idx_stride, void *stream) {
    SG_TRY(ensure_device());
    SG_CHECK_ARG(d_bits && d_idx, "null device buffer");
    SG_CHECK_ARG(B >= 0 && B <= CAMP_MAX_B && L >= 0, "bad (B, L)");
    SG_CHECK_ARG(logM >= 0 && logM <= 30 && logK >= 0 && logK <= 30 && logM + logK >= 1, "bad (logM, logK)");
    SG_CHECK_ARG(logK == 0 || d_sym, "logK > 0 needs d_sym");
    SG_CHECK_ARG(bit_stride >= (size_t)L * (logM + logK) && idx_stride >= (size_t)L, "strides shorter than a row");
    if (!B || !L) return SG_OK;
    return camp_launch_bits_to_psk_strided(d_bits, bit_stride, B, L, logM, logK, d_idx, d_sym, idx_stride,
                                           pick_stream(stream));
}

int sg_psk_pack_sections_device(const int32_t *d_idx, const int32_t *d_sym, int B, int L, int logK, int32_t *d_word,
                                void *stream) {
    SG_TRY(ensure_device());
    SG_CHECK_ARG(d_idx && d_word, "null device buffer");
    SG_CHECK_ARG(B >= 0 && L >= 0, "bad (B, L)");
    SG_CHECK_ARG(logK >= 0 && logK <= 30, "bad logK");
    SG_CHECK_ARG(logK == 0 || d_sym, "logK > 0 needs d_sym");
    return camp_launch_pack(d_idx, logK ? d_sym : nullptr, B, L, logK, d_word, pick_stream(stream));
}

int sg_psk_unpack_sections_device(const int32_t *d_word, int B, int L, int logK, int32_t *d_idx, int32_t *d_sym,
                                  void *stream) {
    SG_TRY(ensure_device());
    SG_CHECK_ARG(d_word && d_idx, "null device buffer");
    SG_CHECK_ARG(B >= 0 && L >= 0, "bad (B, L)");
    SG_CHECK_ARG(logK >= 0 && logK <= 30, "bad logK");
    SG_CHECK_ARG(logK == 0 || d_sym, "logK > 0 needs d_sym");
    return camp_launch_unpack(d_word, B, L, logK, d_idx, d_sym, pick_stream(stream));
}

}  // extern "C"
