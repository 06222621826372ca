// Tables and views of the regular engine (amp_fused.hip): one transform per column block.
#include "amp_plan.hpp"

namespace sg {

// Tables of the regular engine (amp_fused.hip), one transform per column
// block: class order of each block's entries and the needed-row structure of
// the two FFT stages.  Sizes: P = stage-1 FFT length (LDS resident), Q = N2/P.
int build_regular(sg_amp_plan *p, const uint32_t *order0, const uint32_t *order1, const std::vector<double> &t_scale) {
    const long long N = p->w, N2 = p->N2;
    const int nT = p->nT, Mc = p->Mc, n = p->n, M = p->M;
    const int Lblk = p->L / p->Lc;
    SG_CHECK_ARG(Lblk < 65536, "too many sections per column block (%d)", Lblk);
    const size_t rb = p->precision == SG_F64 ? 8 : 4;
    long long Pmax = p->precision == SG_F64 ? 8192 : 16384;
    // Single-precision single-transform designs whose needed spectrum fits the
    // per-codeword engine's LDS (2 n <= 12288 indices, L <= 1024): P = 8192 and
    // its tables; SG_AMP_ENGINE=staged at plan creation keeps P = 16384
    const char *eng = getenv("SG_AMP_ENGINE");
    if (p->precision == SG_F32 && nT == 1 && 2 * n <= 14 * CW_THREADS && Lblk <= CW_THREADS && N2 >= (1 << 14) &&
        !p->no_cw && !(eng && std::strcmp(eng, "staged") == 0))
        Pmax = 8192;
    if (const char *e = getenv("SG_AMP_PMAX")) Pmax = std::max(8LL, std::min(16384LL, atoll(e)));  // tuning knob
    int P = (int)std::min<long long>(N2, Pmax);
    auto img_bound = [](int P) { return 2 * (P + (P >> 4)); };  // before the classes are known
    while (P > 8 && reg_stage1_lds(img_bound(P), P, Lblk, rb) > 160 * 1024) P >>= 1;
    SG_CHECK_ARG(reg_stage1_lds(img_bound(P), P, Lblk, rb) <= 160 * 1024, "section statistics exceed the LDS budget");
    const int Q = (int)(N2 / P);
    p->rP = P; p->rQ = Q; p->rlog2P = ilog2(P); p->Lblk = Lblk;
    p->rept = reg_ept(P, rb);
    const size_t cxb = 2 * rb;
    p->RB = (int)std::min<size_t>(128, std::max<size_t>(1, 32768 / ((size_t)Q * cxb)));
    SG_CHECK_ARG(256 % p->RB == 0, "row block %d must divide 256", p->RB);

    std::vector<std::vector<int32_t>> row_k1(nT), kptr(nT), kk2(nT), krho(nT), oa(nT), ob(nT), gi(nT);
    std::vector<std::vector<cd>> oc(nT), gc(nT);
    std::vector<int32_t> cls_ptr((size_t)nT * (Q + 1)), cls_j((size_t)nT * Mc), qpos((size_t)nT * Mc);
    std::vector<uint16_t> cls_sec((size_t)nT * Mc), seg((size_t)nT * Q * (Lblk + 1));
    std::vector<uint32_t> cls_ls((size_t)nT * Mc);
    std::vector<int32_t> kidx(N2, -1);
    std::vector<uint8_t> need(N2);
    for (int t = 0; t < nT; ++t) {
        const uint32_t *o0 = order0 + (size_t)t * n, *o1 = order1 + (size_t)t * Mc;
        SG_TRY(check_order("order1", o1, Mc, N));
        SG_TRY(check_order("order0", o0, n, N));
        // ---- class order of the column block: (class m2, section, j)
        std::vector<int32_t> cnt(Q + 1, 0), m2of(Mc), locof(Mc);
        for (int j = 0; j < Mc; ++j) {
            const long long sl = slot_of_pos(o1[j], N);
            const long long m = sl >> 1;
            m2of[j] = (int)(m % Q);
            locof[j] = (int)(2 * fsw((int)(m / Q)) + (sl & 1));  // swizzled LDS layout of lds_fft1
            cnt[m2of[j] + 1]++;
        }
        int32_t *cpt = cls_ptr.data() + (size_t)t * (Q + 1);
        cpt[0] = 0;
        for (int c = 0; c < Q; ++c) cpt[c + 1] = cpt[c] + cnt[c + 1];
        std::vector<int32_t> fill(cpt, cpt + Q);
        for (int j = 0; j < Mc; ++j) {  // ascending j: each class sorted by (section, j)
            const int q = fill[m2of[j]]++;
            const size_t o = (size_t)t * Mc + q;
            cls_sec[o] = (uint16_t)(j / M);
            cls_ls[o] = (uint32_t)locof[j] | ((uint32_t)(j / M) << 16);
            cls_j[o] = j;
            qpos[(size_t)t * Mc + j] = q;
        }
        for (int c = 0; c < Q; ++c) {
            uint16_t *sg = seg.data() + ((size_t)t * Q + c) * (Lblk + 1);
            const int q0 = cpt[c], q1 = cpt[c + 1];
            int q = q0;
            for (int l = 0; l <= Lblk; ++l) {
                while (q < q1 && cls_sec[(size_t)t * Mc + q] < l) ++q;
                sg[l] = (uint16_t)(q - q0);
                if (l > 0) p->rmaxseg = std::max(p->rmaxseg, (int)sg[l] - (int)sg[l - 1]);
            }
        }
        // ---- needed N/2-indices: forward outputs = inverse inputs
        std::fill(need.begin(), need.end(), 0);
        for (int i = 0; i < n; ++i) {
            const long long k = o0[i], kk = (k <= N2) ? k : N - k;
            need[kk % N2] = 1;
            need[(N2 - kk) % N2] = 1;
        }
        int nk = 0;
        for (int k1 = 0; k1 < P; ++k1) {
            bool any = false;
            for (int k2 = 0; k2 < Q; ++k2) {
                const long long idx = k1 + (long long)P * k2;
                if (!need[idx]) continue;
                if (!any) {
                    row_k1[t].push_back(k1);
                    kptr[t].push_back(nk);
                    any = true;
                }
                kk2[t].push_back(k2);
                krho[t].push_back((int)row_k1[t].size() - 1);
                kidx[idx] = nk++;
            }
        }
        kptr[t].push_back(nk);
        oa[t].resize(n);
        ob[t].resize(n);
        oc[t].resize(2 * (size_t)n);
        for (int i = 0; i < n; ++i) {
            long long a, b;
            cd c1, c2;
            fwd_coef(o0[i], N, N2, t_scale[t], &a, &b, &c1, &c2);
            oa[t][i] = kidx[a];
            ob[t][i] = kidx[b];
            oc[t][2 * i] = c1;
            oc[t][2 * i + 1] = c2;
        }
        gi[t].assign(4 * (size_t)nk, -1);
        gc[t].assign(4 * (size_t)nk, cd(0, 0));
        std::vector<int> ng(nk, 0);
        bool ok = true;
        for (int i = 0; i < n; ++i)
            inv_contrib(o0[i], N, N2, t_scale[t], [&](long long k, cd c) {
                const int kx = kidx[k];
                if (kx < 0 || ng[kx] >= 4) { ok = false; return; }
                gi[t][4 * (size_t)kx + ng[kx]] = i;
                gc[t][4 * (size_t)kx + ng[kx]] = c;
                ng[kx]++;
            });
        SG_CHECK_ARG(ok, "internal: inverse contribution outside the needed set");
        for (int i = 0; i < n; ++i) {  // reset the index map for the next transform
            const long long k = o0[i], kk = (k <= N2) ? k : N - k;
            kidx[kk % N2] = -1;
            kidx[(N2 - kk) % N2] = -1;
        }
    }
    int nRmax = 1, nKmax = 1;
    for (int t = 0; t < nT; ++t) {
        nRmax = std::max(nRmax, (int)row_k1[t].size());
        nKmax = std::max(nKmax, (int)kk2[t].size());
    }
    p->nRmax = nRmax; p->nKmax = nKmax;
    p->nrb = (nRmax + p->RB - 1) / p->RB;
    std::vector<int32_t> nR(nT), f_rk((size_t)nT * nRmax, 0), f_kp((size_t)nT * (nRmax + 1), 0);
    std::vector<int32_t> f_k2((size_t)nT * nKmax, 0), f_kr((size_t)nT * nKmax, 0), f_oa((size_t)nT * n),
        f_ob((size_t)nT * n), f_gi((size_t)nT * nKmax * 4, -1);
    std::vector<cd> f_oc((size_t)nT * n * 2), f_gc((size_t)nT * nKmax * 4, cd(0, 0));
    int maxKb = 0;
    for (int t = 0; t < nT; ++t) {
        const int r = (int)row_k1[t].size(), k = (int)kk2[t].size();
        nR[t] = r;
        std::copy(row_k1[t].begin(), row_k1[t].end(), f_rk.begin() + (size_t)t * nRmax);
        for (int i = 0; i <= nRmax; ++i) f_kp[(size_t)t * (nRmax + 1) + i] = kptr[t][std::min(i, r)];
        std::copy(kk2[t].begin(), kk2[t].end(), f_k2.begin() + (size_t)t * nKmax);
        std::copy(krho[t].begin(), krho[t].end(), f_kr.begin() + (size_t)t * nKmax);
        std::copy(oa[t].begin(), oa[t].end(), f_oa.begin() + (size_t)t * n);
        std::copy(ob[t].begin(), ob[t].end(), f_ob.begin() + (size_t)t * n);
        std::copy(oc[t].begin(), oc[t].end(), f_oc.begin() + (size_t)t * n * 2);
        std::copy(gi[t].begin(), gi[t].end(), f_gi.begin() + (size_t)t * nKmax * 4);
        std::copy(gc[t].begin(), gc[t].end(), f_gc.begin() + (size_t)t * nKmax * 4);
        for (int b = 0; b * p->RB < r; ++b)
            maxKb = std::max(maxKb, kptr[t][std::min(r, (b + 1) * p->RB)] - kptr[t][b * p->RB]);
        (void)k;
    }
    p->maxKb = maxKb;
    std::vector<cd> twP(P), twQ(Q);
    for (int i = 0; i < P; ++i) twP[i] = tw(i, P);
    for (int i = 0; i < Q; ++i) twQ[i] = tw(i, Q);
    // per-stage twiddles of the P-point FFT in thread order (fft.hpp lds_fft1)
    std::vector<cd> stw = stage_twiddles(p->rlog2P, p->rept);
    if (stw.empty()) stw.push_back(cd(1, 0));
    const int nB = (P + 63) / 64;
    p->nB = nB;
    std::vector<cd> twa((size_t)Q * 64), twb((size_t)Q * nB);
    for (int m2 = 0; m2 < Q; ++m2) {
        for (int a = 0; a < 64; ++a) twa[(size_t)m2 * 64 + a] = tw((long long)m2 * a, N2);
        for (int b = 0; b < nB; ++b) twb[(size_t)m2 * nB + b] = tw((long long)m2 * 64 * b, N2);
    }
    SG_TRY(p->tables.upload(&p->r_nR, nR));
    SG_TRY(p->tables.upload(&p->r_row_k1, f_rk));
    {  // stage-1 order: thread tid holds rows tid + i nthr, i < ept, packed in pairs
        const int ept = p->rept, nthr = P / ept;
        SG_CHECK_ARG(P <= 65536 && ept % 2 == 0, "stage-1 FFT length %d exceeds the 16-bit row index", P);
        std::vector<uint32_t> pk((size_t)nT * (P / 2), 0u);
        for (int t = 0; t < nT; ++t) {
            const int nr = (int)row_k1[t].size();
            for (int j = 0; j < ept / 2; ++j)
                for (int tid = 0; tid < nthr; ++tid) {
                    const int r0 = tid + 2 * j * nthr, r1 = r0 + nthr;
                    const uint32_t a = r0 < nr ? (uint32_t)row_k1[t][r0] : 0u, b = r1 < nr ? (uint32_t)row_k1[t][r1] : 0u;
                    pk[(size_t)t * (P / 2) + (size_t)j * nthr + tid] = a | (b << 16);
                }
        }
        SG_TRY(p->tables.upload(&p->r_row_k1p, pk));
    }
    SG_TRY(p->tables.upload(&p->r_kptr, f_kp));
    SG_TRY(p->tables.upload(&p->r_kk2, f_k2));
    SG_TRY(p->tables.upload(&p->r_krho, f_kr));
    SG_TRY(p->tables.upload(&p->r_oa, f_oa));
    SG_TRY(p->tables.upload(&p->r_ob, f_ob));
    SG_TRY(upload_cx(p, &p->r_oc, f_oc));
    SG_TRY(p->tables.upload(&p->r_gi, f_gi));
    SG_TRY(upload_cx(p, &p->r_gc, f_gc));
    for (int t = 0; t < nT; ++t)
        for (int m2 = 0; m2 < Q; ++m2)
            p->rmaxcls = std::max(p->rmaxcls, cls_ptr[(size_t)t * (Q + 1) + m2 + 1] - cls_ptr[(size_t)t * (Q + 1) + m2]);
    p->rimg = (std::max(2 * P, fpad(p->rmaxcls + 16) + 1) + 3) / 4 * 4;
    SG_CHECK_ARG(reg_stage1_lds(p->rimg, P, Lblk, rb) <= 160 * 1024, "a class exceeds the LDS budget");
    SG_TRY(p->tables.upload(&p->r_cls_ptr, cls_ptr));
    SG_TRY(p->tables.upload(&p->r_cls_ls, cls_ls));
    SG_TRY(p->tables.upload(&p->r_cls_j, cls_j));
    SG_TRY(p->tables.upload(&p->r_qpos, qpos));
    SG_TRY(p->tables.upload(&p->r_seg, seg));
    SG_TRY(upload_cx(p, &p->r_twP, twP));
    SG_TRY(upload_cx(p, &p->r_twQ, twQ));
    SG_TRY(upload_cx(p, &p->r_stw, stw));
    SG_TRY(upload_cx(p, &p->r_twa, twa));
    SG_TRY(upload_cx(p, &p->r_twb, twb));
    if (p->precision == SG_F32 && nT == 1 && P == (1 << 13) && Lblk <= CW_THREADS && n <= 8 * CW_THREADS &&
        Q <= 64 && p->rmaxcls <= 9 * CW_THREADS && p->rimg == 2 * P && fpad(p->rmaxcls + 16) < p->rimg)
    {
        SG_TRY(build_cw(p, row_k1[0], kptr[0], kk2[0], f_oa, f_ob, f_gi, f_gc, cls_ptr, cls_ls));
        if (p->cw) SG_TRY(build_cw2(p, order0, t_scale[0], row_k1[0], cls_ptr, cls_ls));
    }
    // double precision: the split engine only (amp_cw2d.hip), its tables built directly; the plan then
    // counts as a per-codeword plan (use_cw), without the companion (f64 keeps P = 8192 either way)
    // (the bounds of amp_cw2d.hip cw2d_launch_iter: its statistics launch takes a section's M <= 512 entries
    // over Q <= 64 class segments in one wavefront, four sections per workgroup)
    if (p->precision == SG_F64 && nT == 1 && P == (1 << 13) && Lblk <= 2 * CW2_THREADS && p->L <= 1024 &&
        p->L % 4 == 0 && M <= 512 && Q % 2 == 0 && Q <= 64 && p->rmaxcls <= CW2_SLICE && !p->no_cw) {
        SG_TRY(build_cw2(p, order0, t_scale[0], row_k1[0], cls_ptr, cls_ls));
        p->cw = p->cw2OT != 0 && cw2d_supported(c2dtables(p));  // else the staged engine, never a decode-time error
    }
    return SG_OK;
}

template <typename T>
RegTables<T> rtables(const sg_amp_plan *p) {
    RegTables<T> tb;
    tb.nT = p->nT; tb.L = p->L; tb.M = p->M; tb.LM = p->LM; tb.n = p->n; tb.Lc = p->Lc; tb.Mc = p->Mc;
    tb.Lblk = p->Lblk; tb.N2 = p->N2; tb.P = p->rP; tb.Q = p->rQ; tb.log2P = p->rlog2P; tb.ept = p->rept; tb.maxcls = p->rmaxcls; tb.img = p->rimg;
    {
        // measured best at C2: 20000 (f32 staged engine +1.4 %, f64 +0.9 %: profiles/r04_f64_env_sweep.txt)
        const char *st = std::getenv("SG_AMP_STAGGER");
        tb.stagger = st ? std::atoi(st) : 20000;
    }
    tb.nRmax = p->nRmax; tb.nKmax = p->nKmax; tb.RB = p->RB; tb.nrb = p->nrb; tb.maxKb = p->maxKb;
    tb.nR = p->r_nR; tb.row_k1 = p->r_row_k1; tb.row_k1p = p->r_row_k1p; tb.kptr = p->r_kptr; tb.kk2 = p->r_kk2; tb.krho = p->r_krho;
    tb.oa = p->r_oa; tb.ob = p->r_ob; tb.oc = (const cx<T> *)p->r_oc; tb.gi = p->r_gi; tb.gc = (const cx<T> *)p->r_gc;
    tb.cls_ptr = p->r_cls_ptr; tb.cls_ls = p->r_cls_ls; tb.cls_j = p->r_cls_j;
    tb.qpos = p->r_qpos; tb.seg = p->r_seg;
    tb.twP = (const cx<T> *)p->r_twP; tb.twQ = (const cx<T> *)p->r_twQ;
    tb.twHi = (const cx<T> *)p->twHi; tb.twLo = (const cx<T> *)p->twLo;
    tb.stw = (const cx<T> *)p->r_stw; tb.twa = (const cx<T> *)p->r_twa; tb.twb = (const cx<T> *)p->r_twb;
    tb.nB = p->nB;
    tb.skip = diag_skip();
    return tb;
}
template RegTables<float> rtables<float>(const sg_amp_plan *);
template RegTables<double> rtables<double>(const sg_amp_plan *);

template <typename T>
RegBufs<T> rbufs(const sg_amp_plan *p, int B, const void *y) {
    RegBufs<T> bf;
    bf.B = B; bf.mode = 0;
    bf.s = (T *)p->ws_s; bf.tu = (cx<T> *)p->ws_tu; bf.xn = (cx<T> *)p->ws_xn; bf.part = (T *)p->ws_part;
    bf.stM = (T *)p->ws_stM; bf.stI = (T *)p->ws_stI;
    bf.y = (const T *)(y ? y : p->ws_y); bf.z = (T *)p->ws_z;
    bf.phi = p->ws_phi; bf.tau = p->ws_tau; bf.tau_prev = p->ws_tau_prev; bf.active = p->ws_active;
    bf.true_idx = nullptr; bf.map = p->ws_argmax; bf.ext_in = nullptr; bf.ext_out = nullptr;
    bf.tprof_ab = bf.tprof_az = bf.trt_ab = bf.trt_az = nullptr;
    if (uint64_t *tp = p->tprof.at<uint64_t>(); tp && (size_t)B * p->nT * p->rQ <= p->tprof_items) {
        bf.tprof_ab = tp;
        bf.tprof_az = tp + p->tprof_items * 8;
        bf.trt_ab = tp + p->tprof_items * 16;
        bf.trt_az = tp + p->tprof_items * 18;
    }
    return bf;
}
template RegBufs<float> rbufs<float>(const sg_amp_plan *, int, const void *);
template RegBufs<double> rbufs<double>(const sg_amp_plan *, int, const void *);

}  // namespace sg
