// AMP design plans: the Makhoul / DCT coefficient math, build_plan with the general engine's tables, the
// batch workspace, plan creation and destruction.
#include <memory>

#include "amp_plan.hpp"

namespace sg {

template <typename R>
static int upload_cx_as(sg_amp_plan *p, void **dst, const std::vector<cd> &src) {
    std::vector<R> v(2 * src.size());
    for (size_t i = 0; i < src.size(); ++i) { v[2 * i] = (R)src[i].real(); v[2 * i + 1] = (R)src[i].imag(); }
    return p->tables.upload((R **)dst, v);
}

int upload_cx(sg_amp_plan *p, void **dst, const std::vector<cd> &src) {
    return by_precision(p->precision, [&](auto t) { return upload_cx_as<decltype(t)>(p, dst, src); });
}

cd expi(double a) { return cd(std::cos(a), std::sin(a)); }

cd tw(long long k, long long m) {
    k %= m;
    if (k < 0) k += m;
    return expi(-2.0 * M_PI * (double)k / (double)m);
}

// Forward output at DCT position k (sparc.py:687-692 via the Makhoul packed
// FFT): X_dct[k] = Re(c1 H[a] + c2 conj(H[b])), H = FFT_{N/2} of the packed
// sequence; sc = sqrt(W/L) of the block (sparc.py:786-794).
void fwd_coef(long long k, long long N, long long N2, double sc, long long *a, long long *b, cd *c1, cd *c2) {
    const long long kk = (k <= N2) ? k : N - k;
    *a = kk % N2;
    *b = (N2 - kk) % N2;
    const cd e = (k <= N2) ? expi(-M_PI * (double)k / (2.0 * N)) : expi(M_PI * (double)k / (2.0 * N));
    const cd wk = tw(kk, N);
    const cd I(0, 1);
    const double sqrt2 = std::sqrt(2.0);
    *c1 = e * (0.5 - 0.5 * I * wk) * (sqrt2 * sc);
    *c2 = e * (0.5 + 0.5 * I * wk) * (sqrt2 * sc);
}

std::vector<cd> stage_twiddles(int log2n, int ept) {
    std::vector<cd> stw;
    int radix[8];
    const int ns = fft1_plan(log2n, ept, radix);
    int lns = 0;
    for (int st = 0; st < ns; ++st) {
        const int R = radix[st];
        const long long Ns = 1LL << lns;
        for (long long k = 0; k < Ns; ++k)
            for (int q = 0; q < tw_per_k(R); ++q) stw.push_back(tw(tw_exp(R, q) * k, Ns * R));
        lns += ilog2(R);
    }
    return stw;
}

int check_order(const char *name, const uint32_t *order, int count, long long N) {
    std::vector<uint8_t> seen(N, 0);
    for (int i = 0; i < count; ++i) {
        const long long pos = order[i];
        SG_CHECK_ARG(pos >= 1 && pos < N, "%s entry %lld outside [1, w)", name, pos);
        SG_CHECK_ARG(!seen[pos], "%s has a repeated position", name);
        seen[pos] = 1;
    }
    return SG_OK;
}

int gather_gslots(const uint32_t *o0, int Mr, long long N, long long N2, double sc, std::vector<GSlot> *out) {
    std::vector<std::vector<std::pair<int, cd>>> gcon(N2);
    for (int i = 0; i < Mr; ++i)
        inv_contrib(o0[i], N, N2, sc, [&](long long k, cd c) { gcon[k].push_back({i, c}); });
    out->clear();
    for (int k = 0; k < N2; ++k) {
        if (gcon[k].empty()) continue;
        SG_CHECK_ARG(gcon[k].size() <= 4, "internal: >4 contributions to one G slot");
        GSlot g{k, {-1, -1, -1, -1}, {}};
        for (size_t q = 0; q < gcon[k].size(); ++q) {
            g.i[q] = gcon[k][q].first;
            g.c[q] = gcon[k][q].second;
        }
        out->push_back(g);
    }
    return SG_OK;
}

// Phase ablation for timing studies: compiled only into a diagnostic build (make DIAG=1), because the results
// are wrong when a phase is skipped.  The product library ignores SG_AMP_SKIP.
int diag_skip() {
#ifdef SG_DIAG
    const char *sk = std::getenv("SG_AMP_SKIP");
    return sk ? std::atoi(sk) : 0;
#else
    return 0;
#endif
}

// ---- workspace: every buffer is a slot of one of the plan's pools (device_mem.hpp), released together
int partial_ensure_ws(sg_amp_plan *p, int B) {
    // s_keep (K = 2 soft output) joins the pool at the first decode after sg_amp_bpsk_soft_output(p, 1) and stays
    const bool keep = p->bpsk_soft || p->wp_skeep;
    if (B <= p->cap_Bp && (p->wp_skeep || !keep)) return SG_OK;
    B = std::max(B, p->cap_Bp);
    p->wp.release();
    p->cap_Bp = 0;
    p->wp_skeep = nullptr;
    const size_t rs = p->precision == SG_F64 ? 8 : 4, Bz = (size_t)B;
    SG_TRY(p->wp.alloc(&p->wp_u, Bz * p->LM * rs));
    SG_TRY(p->wp.alloc(&p->wp_r, Bz * p->n * rs));
    SG_TRY(p->wp.alloc(&p->wp_z, Bz * p->n * rs));
    SG_TRY(p->wp.alloc(&p->wp_zz, Bz * oploop_zz_count(p->Lr, p->Mr) * sizeof(double)));
    SG_TRY(p->wp.alloc(&p->wp_bsq, Bz * p->L * sizeof(double)));
    SG_TRY(p->wp.alloc(&p->wp_err, Bz * p->L * sizeof(double)));
    SG_TRY(p->wp.alloc(&p->wp_tau, Bz * p->Lc * sizeof(double)));
    SG_TRY(p->wp.alloc(&p->wp_active, Bz * sizeof(int32_t)));
    SG_TRY(p->wp.alloc(&p->wp_known, Bz * p->L * sizeof(int32_t)));
    if (keep) SG_TRY(p->wp.alloc(&p->wp_skeep, Bz * p->LM * rs));
    p->cap_Bp = B;
    return SG_OK;
}

static void plan_free_ws(sg_amp_plan *p) {
    p->ws.release();
    p->io.reset();  // (its own grow rule, ensure_io; freed with the workspace)
    p->cap_B = p->cap_tmax = 0;
}

int ensure_ws(sg_amp_plan *p, int B, int t_max) {
    if (B <= p->cap_B && t_max <= p->cap_tmax) return SG_OK;
    plan_free_ws(p);
    const size_t rs = p->precision == SG_F64 ? 8 : 4;
    const size_t Bz = (size_t)B;
    auto take = [&](auto *slot, size_t bytes) { return p->ws.alloc(slot, std::max<size_t>(16, bytes)); };
    SG_TRY(take(&p->ws_y, Bz * p->n * rs));
    SG_TRY(take(&p->ws_z, Bz * p->n * rs));
    if (p->regular) {
        SG_TRY(take(&p->ws_s, Bz * p->LM * rs));
        SG_TRY(take(&p->ws_tu, Bz * p->nT * p->rQ * p->nRmax * 2 * rs));
        SG_TRY(take(&p->ws_xn, Bz * p->nT * p->nKmax * 2 * rs));
        SG_TRY(take(&p->ws_part, Bz * p->nT * p->rQ * 3 * p->Lblk * rs));
        if (std::getenv("SG_AMP_TPROF")) {  // diagnostics only (not a workspace slot: it lives until destroy)
            p->tprof.reset();
            p->tprof_items = Bz * p->nT * p->rQ;
            // [2 kernels][items][8] shader-clock stamps, then [2 kernels][items][2] realtime start / end
            SG_TRY(p->tprof.ensure(std::max<size_t>(16, p->tprof_items * 20 * sizeof(uint64_t))));
            SG_HIP(hipMemset(p->tprof.at(), 0, p->tprof_items * 20 * sizeof(uint64_t)));
        }
        if (p->cw2OT) {  // (reals of the plan's precision; partial statistics: four per section)
            SG_TRY(take(&p->ws_c2xp, Bz * std::max(CW2_NP, 2) * p->cw2OT * CW2_THREADS * rs));
            SG_TRY(take(&p->ws_c2vz, Bz * cw2_otp(p->cw2OT) * CW2_THREADS * 8));  // (f32: two reals per slot)
            SG_TRY(take(&p->ws_c2ys, Bz * p->cw2OT * CW2_THREADS * rs));
            SG_TRY(take(&p->ws_c2zs, Bz * p->cw2OT * CW2_THREADS * rs));
            SG_TRY(take(&p->ws_c2part, Bz * std::max(CW2_NP, 2) * p->Lblk * 4 * rs));
            if (p->precision == SG_F64) {
                SG_TRY(take(&p->ws_c2beta, Bz * p->LM * rs));
                SG_TRY(take(&p->ws_c2sec, Bz * p->L * 2 * rs));
            }
        }
        SG_TRY(take(&p->ws_stM, Bz * p->L * rs));
        SG_TRY(take(&p->ws_stI, Bz * p->L * rs));
        SG_TRY(take(&p->ws_tau_prev, Bz * p->Lc * 8));
    } else {
        SG_TRY(take(&p->ws_beta, Bz * p->LM * rs));
        SG_TRY(take(&p->ws_rbuf, Bz * p->nT * p->Mr * rs));
        SG_TRY(take(&p->ws_buf0, Bz * p->nT * p->N2 * 2 * rs));
        SG_TRY(take(&p->ws_buf1, Bz * p->nT * p->N2 * 2 * rs));
        SG_TRY(take(&p->ws_sumsq, Bz * p->L * 8));
        SG_TRY(take(&p->ws_err, Bz * p->L * 8));
    }
    if (p->block || p->block2) SG_TRY(take(&p->ws_gbuf, Bz * (size_t)p->b_ngs * 8));
    SG_TRY(take(&p->ws_phi, Bz * p->Lr * 8));
    SG_TRY(take(&p->ws_tau, Bz * p->Lc * 8));
    SG_TRY(take(&p->ws_psi, Bz * p->Lc * 8));
    SG_TRY(take(&p->ws_psi_prev, Bz * p->Lc * 8));
    SG_TRY(take(&p->ws_phi_prev, Bz * p->Lr * 8));
    SG_TRY(take(&p->ws_gamma, Bz * p->Lr * 8));
    SG_TRY(take(&p->ws_bco, Bz * p->Lr * 8));
    SG_TRY(take(&p->ws_nmse, Bz * std::max(t_max, 2) * p->Lc * 8));
    SG_TRY(take(&p->ws_active, Bz * 4));
    SG_TRY(take(&p->ws_argmax, Bz * p->L * 4));
    SG_TRY(take(&p->ws_true, Bz * p->L * 4));
    SG_TRY(take(&p->ws_tfinal, Bz * 4));
    p->cap_B = B;
    p->cap_tmax = std::max(t_max, 2);
    return SG_OK;
}

int ensure_io(sg_amp_plan *p, size_t bytes) { return p->io.ensure(bytes); }

template <typename T>
AmpTables<T> tables(const sg_amp_plan *p) {
    AmpTables<T> tb;
    tb.nT = p->nT; tb.w = p->w; tb.N2 = p->N2; tb.P = p->P; tb.Q = p->Q; tb.log2P = p->log2P; tb.log2Q = p->log2Q;
    tb.npairs = p->npairs; tb.L = p->L; tb.M = p->M; tb.LM = p->LM; tb.n = p->n; tb.Lr = p->Lr; tb.Lc = p->Lc;
    tb.Mr = p->Mr; tb.Mc = p->Mc; tb.ndim = p->ndim;
    tb.t_row = p->t_row; tb.t_col = p->t_col; tb.col_ptr = p->col_ptr; tb.col_t = p->col_t;
    tb.inmap = p->inmap; tb.outslot = p->outslot; tb.rp_ptr = p->rp_ptr; tb.rp_i = p->rp_i; tb.rp_ab = p->rp_ab;
    tb.rp_c = (const cx<T> *)p->rp_c; tb.gs_ptr = p->gs_ptr; tb.gs_loc = p->gs_loc; tb.gs_i = p->gs_i;
    tb.gs_c = (const cx<T> *)p->gs_c; tb.twP = (const cx<T> *)p->twP; tb.twQ = (const cx<T> *)p->twQ;
    tb.twHi = (const cx<T> *)p->twHi; tb.twLo = (const cx<T> *)p->twLo;
    tb.row_ptr = p->row_ptr; tb.row_t = p->row_t;
    return tb;
}
template AmpTables<float> tables<float>(const sg_amp_plan *);
template AmpTables<double> tables<double>(const sg_amp_plan *);

template <typename T>
AmpBufs<T> bufs(const sg_amp_plan *p, int B, const void *y) {
    AmpBufs<T> bf;
    bf.B = B;
    bf.beta = (T *)p->ws_beta; bf.y = (const T *)(y ? y : p->ws_y); bf.z = (T *)p->ws_z; bf.rbuf = (T *)p->ws_rbuf;
    bf.buf0 = (cx<T> *)p->ws_buf0; bf.buf1 = (cx<T> *)p->ws_buf1; bf.phi = p->ws_phi; bf.tau = p->ws_tau;
    bf.active = p->ws_active; bf.sec_sumsq = p->ws_sumsq; bf.sec_err = p->ws_err; bf.sec_argmax = p->ws_argmax;
    bf.true_idx = nullptr;
    return bf;
}
template AmpBufs<float> bufs<float>(const sg_amp_plan *, int, const void *);
template AmpBufs<double> bufs<double>(const sg_amp_plan *, int, const void *);

static int build_plan(int ndim, const double *W, int Lr_in, int Lc_in, int L, int M, int n, const uint32_t *order0,
                      const uint32_t *order1, int precision, bool no_cw, sg_amp_plan **out) {
    SG_CHECK_ARG(out && W && order0 && order1, "null argument");
    SG_CHECK_ARG(ndim >= 0 && ndim <= 2, "W.ndim must be 0, 1 or 2");
    SG_CHECK_ARG(precision == SG_F32 || precision == SG_F64, "precision must be SG_F32 or SG_F64");
    SG_CHECK_ARG(L > 0 && M > 0 && n > 0 && (M & (M - 1)) == 0, "bad (L, M, n)");
    SG_TRY(ensure_device());
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
    int w = 1;
    while (w < std::max(Mr + 1, Mc + 1)) w <<= 1;  // sparc.py:744
    SG_CHECK_ARG(w >= 16 && w <= (1 << 23), "transform size w=%d outside [16, 2^23]", w);
    std::unique_ptr<sg_amp_plan> p(new sg_amp_plan());
    hipGetDevice(&p->device);
    p->no_cw = no_cw;
    p->precision = precision; p->ndim = ndim; p->L = L; p->M = M; p->LM = (int)LM; p->n = n;
    p->Lr = Lr; p->Lc = Lc; p->Mr = Mr; p->Mc = Mc; p->w = w; p->N2 = w / 2;
    const int lg = ilog2(p->N2);
    p->log2P = lg / 2; p->log2Q = lg - p->log2P;
    p->P = 1 << p->log2P; p->Q = 1 << p->log2Q;
    p->npairs = p->P / 2 + 1;
    p->W.assign(W, W + (ndim == 0 ? 1 : (size_t)Lr * Lc));
    // transforms = nonzero blocks in row-major order (sparc.py:758-771)
    std::vector<int32_t> t_row, t_col;
    std::vector<double> t_scale;
    for (int r = 0; r < Lr; ++r)
        for (int c = 0; c < Lc; ++c) {
            const double wv = (ndim == 0) ? p->W[0] : p->W[(size_t)r * Lc + c];
            if (wv != 0.0) {
                t_row.push_back(r); t_col.push_back(c);
                t_scale.push_back(std::sqrt(wv / L));  // np.sqrt(W/L)
            }
        }
    p->nT = (int)t_row.size();
    SG_CHECK_ARG(p->nT > 0, "base matrix is all zero");
    std::vector<int32_t> col_ptr(Lc + 1, 0), col_t, row_ptr(Lr + 1, 0), row_t;
    for (int c = 0; c < Lc; ++c) {
        for (int t = 0; t < p->nT; ++t)
            if (t_col[t] == c) col_t.push_back(t);
        col_ptr[c + 1] = (int32_t)col_t.size();
    }
    for (int r = 0; r < Lr; ++r) {
        for (int t = 0; t < p->nT; ++t)
            if (t_row[t] == r) row_t.push_back(t);
        row_ptr[r + 1] = (int32_t)row_t.size();
    }
    // one transform per column block: the regular engine (amp_fused.hip);
    // SG_AMP_ENGINE=legacy keeps the general four-step path for comparison
    const char *eng = std::getenv("SG_AMP_ENGINE");
    // (the per-section softmax statistics of a column block must fit in LDS
    // beside the stage-1 FFT: at most 2048 (f64) / 4096 (f32) sections)
    const size_t sec_bytes = (size_t)2 * (L / Lc) * (precision == SG_F64 ? 8 : 4);
    p->regular = ndim <= 1 && p->nT == Lc && sec_bytes <= 32 * 1024 && !(eng && std::strcmp(eng, "legacy") == 0);
    // several transforms per column block, each small enough for one
    // workgroup's LDS: the block engine (single precision, w = 2^15)
    const bool no_blk = eng && (std::strcmp(eng, "legacy") == 0 || std::strcmp(eng, "general") == 0);
    // w = 2^15 with Mc = 2^14 (C4): the single-class engine (one 1024-thread workgroup per CU, 132 KB of LDS);
    // SG_AMP_BLOCK=two-class selects the two-class form at P = 2^13 (two 512-thread workgroups per CU), which
    // measured no faster (block engine)
    const char *bk = std::getenv("SG_AMP_BLOCK");
    const bool single = !(bk && std::strcmp(bk, "two-class") == 0);
    const bool c4 = !p->regular && precision == SG_F32 && p->N2 == (1 << 14) && Mc == (1 << 14) && M >= 64 && !no_blk;
    p->block = c4 && single && M <= 1024 && Mr < 65536;
    // w = 2^16 with Mc = 2^15 (the notebook geometry): the two-class form at P = 2^14
    const bool nb = !p->regular && precision == SG_F32 && p->N2 == (1 << 15) && Mc == (1 << 15) && M >= 64 &&
                    M <= 2048 && Mr <= 1024 && !no_blk;
    p->block2 = (c4 && !single && M <= 2048 && Mr <= 512) || nb;
    p->b2_log2p = p->block2 ? (nb ? 14 : 13) : 0;
    // the general engine's section kernel (amp_dct.hip eta_kernel) holds at most 32 entries per lane: a larger
    // section is refused here, before anything is uploaded, never in the middle of a decode (amp_launch_eta
    // keeps its own check as a guard).  The regular engine has no bound on M (DESIGN.md "Section sizes").
    if (!p->regular && !p->block && !p->block2 && M > 2048)
        return fail(SG_ERR_UNSUPPORTED, "section size M=%d > 2048 unsupported by the general engine", M);
    const int N = w, N2 = p->N2, P = p->P, Q = p->Q, np1 = p->npairs + 1;
    auto pair_of = [&](long long k) -> int {  // row pair of an N2-index
        const int row = (int)(k % P);
        return row <= P / 2 ? row : P - row;
    };
    auto local_of = [&](long long k) -> uint32_t {  // LDS index of N2-index k inside its pair's two rows
        const int row = (int)(k % P);
        const int pr = row <= P / 2 ? row : P - row;
        const int half = (row == pr) ? 0 : 1;
        return (uint32_t)(half * Q + (int)(k / P));
    };
    std::vector<int32_t> inmap((size_t)p->nT * N, -1), outslot((size_t)p->nT * Mc);
    std::vector<int32_t> rp_ptr((size_t)p->nT * np1), rp_i;
    std::vector<uint32_t> rp_ab;
    std::vector<cd> rp_c;
    std::vector<int32_t> gs_ptr((size_t)p->nT * np1), gs_loc, gs_i;
    std::vector<cd> gs_c;
    std::vector<GSlot> gs;
    for (int t = 0; t < p->nT && !p->regular; ++t) {
        const uint32_t *o0 = order0 + (size_t)t * Mr, *o1 = order1 + (size_t)t * Mc;
        SG_TRY(check_order("order1", o1, Mc, N));
        SG_TRY(check_order("order0", o0, Mr, N));
        for (int j = 0; j < Mc; ++j) {
            const long long sl = slot_of_pos(o1[j], N);
            inmap[(size_t)t * N + sl] = j;
            outslot[(size_t)t * Mc + j] = (int32_t)sl;
        }
        const double sc = t_scale[t];
        // ---- forward outputs X[k], k = order0[i], grouped by row pair
        std::vector<std::vector<int>> by_pair(p->npairs);
        for (int i = 0; i < Mr; ++i) {
            const long long k = o0[i], kk = (k <= N2) ? k : N - k;
            by_pair[pair_of(kk % N2)].push_back(i);
        }
        for (int pr = 0; pr < p->npairs; ++pr) {
            rp_ptr[(size_t)t * np1 + pr] = (int32_t)rp_i.size();
            for (int i : by_pair[pr]) {
                long long a, b;
                cd c1, c2;
                fwd_coef(o0[i], N, N2, sc, &a, &b, &c1, &c2);
                rp_i.push_back(i);
                rp_ab.push_back(local_of(a) | (local_of(b) << 16));
                rp_c.push_back(c1);
                rp_c.push_back(c2);
            }
        }
        rp_ptr[(size_t)t * np1 + p->npairs] = (int32_t)rp_i.size();
        // ---- inverse inputs: G[k] = A_k y[k] - i A_k y[N-k] + C_k y[N2+k] - i C_k y[N2-k], grouped by row pair
        SG_TRY(gather_gslots(o0, Mr, N, N2, sc, &gs));
        std::vector<std::vector<const GSlot *>> slots_by_pair(p->npairs);
        for (const GSlot &g : gs) slots_by_pair[pair_of(g.k)].push_back(&g);
        for (int pr = 0; pr < p->npairs; ++pr) {
            gs_ptr[(size_t)t * np1 + pr] = (int32_t)gs_loc.size();
            for (const GSlot *g : slots_by_pair[pr]) {
                gs_loc.push_back((int32_t)local_of(g->k));
                for (int q = 0; q < 4; ++q) gs_i.push_back(g->i[q]), gs_c.push_back(g->c[q]);
            }
        }
        gs_ptr[(size_t)t * np1 + p->npairs] = (int32_t)gs_loc.size();
    }
    std::vector<cd> twP(P), twQ(Q), twHi((N2 + 1023) / 1024), twLo(std::min(N2, 1024));
    for (int i = 0; i < P; ++i) twP[i] = tw(i, P);
    for (int i = 0; i < Q; ++i) twQ[i] = tw(i, Q);
    for (size_t i = 0; i < twHi.size(); ++i) twHi[i] = tw((long long)i * 1024, N2);
    for (size_t i = 0; i < twLo.size(); ++i) twLo[i] = tw((long long)i, N2);
    std::vector<double> Wd = p->W;
    sg_amp_plan *pp = p.release();
    int rc = [&]() -> int {
    SG_TRY(pp->tables.upload(&pp->t_row, t_row));
    SG_TRY(pp->tables.upload(&pp->t_col, t_col));
    SG_TRY(pp->tables.upload(&pp->col_ptr, col_ptr));
    SG_TRY(pp->tables.upload(&pp->col_t, col_t));
    SG_TRY(pp->tables.upload(&pp->row_ptr, row_ptr));
    SG_TRY(pp->tables.upload(&pp->row_t, row_t));
    SG_TRY(pp->tables.upload(&pp->inmap, inmap));
    SG_TRY(pp->tables.upload(&pp->outslot, outslot));
    SG_TRY(pp->tables.upload(&pp->rp_ptr, rp_ptr));
    SG_TRY(pp->tables.upload(&pp->rp_i, rp_i));
    SG_TRY(pp->tables.upload(&pp->rp_ab, rp_ab));
    SG_TRY(upload_cx(pp, &pp->rp_c, rp_c));
    SG_TRY(pp->tables.upload(&pp->gs_ptr, gs_ptr));
    SG_TRY(pp->tables.upload(&pp->gs_loc, gs_loc));
    SG_TRY(pp->tables.upload(&pp->gs_i, gs_i));
    SG_TRY(upload_cx(pp, &pp->gs_c, gs_c));
    SG_TRY(upload_cx(pp, &pp->twP, twP));
    SG_TRY(upload_cx(pp, &pp->twQ, twQ));
    SG_TRY(upload_cx(pp, &pp->twHi, twHi));
    SG_TRY(upload_cx(pp, &pp->twLo, twLo));
    SG_TRY(pp->tables.upload(&pp->dW, Wd));
    if (pp->regular) SG_TRY(build_regular(pp, order0, order1, t_scale));
    if (pp->block) SG_TRY(build_block(pp, order0, order1, t_scale, t_row));
    if (pp->block2) SG_TRY(build_block2(pp, order0, order1, t_scale, t_row));
    return SG_OK;
    }();
    if (rc != SG_OK) {
        sg_amp_plan_destroy(pp);
        return rc;
    }
    *out = pp;
    return SG_OK;
}

}  // namespace sg

using namespace sg;

extern "C" {

int sg_amp_plan_create(int ndim, const double *W, int Lr, int Lc, int L, int M, int n, const uint32_t *order0,
                       const uint32_t *order1, int precision, sg_amp_plan **out) {
    sg_amp_plan *p = nullptr;
    SG_TRY(build_plan(ndim, W, Lr, Lc, L, M, n, order0, order1, precision, false, &p));
    if (p->cw && precision == SG_F32) {
        const int rc = build_plan(ndim, W, Lr, Lc, L, M, n, order0, order1, precision, true, &p->alt);
        if (rc != SG_OK) {
            sg_amp_plan_destroy(p);
            return rc;
        }
    }
    *out = p;
    return SG_OK;
}

int sg_amp_plan_destroy(sg_amp_plan *p) {
    if (!p) return SG_OK;
    sg_amp_plan_destroy(p->alt);
    if (p->poll_ev) {
        hipEventSynchronize(p->poll_ev);  // (a copy into h_active may still be in flight)
        hipEventDestroy(p->poll_ev);
    }
    if (p->h_active) hipHostFree(p->h_active);
    if (p->pipe_stream) {
        hipStreamSynchronize(p->pipe_stream);
        hipStreamDestroy(p->pipe_stream);
    }
    for (hipEvent_t e : p->pipe_ev)
        if (e) hipEventDestroy(e);
    delete p;
    return SG_OK;
}

int sg_amp_plan_info(const sg_amp_plan *p, int *w, int *nT, int *Mr, int *Mc, int *P, int *Q) {
    SG_CHECK_ARG(p, "plan is NULL");
    if (w) *w = p->w;
    if (nT) *nT = p->nT;
    if (Mr) *Mr = p->Mr;
    if (Mc) *Mc = p->Mc;
    if (P) *P = p->regular ? p->rP : p->P;
    if (Q) *Q = p->regular ? p->rQ : p->Q;
    return SG_OK;
}

}  // extern "C"
