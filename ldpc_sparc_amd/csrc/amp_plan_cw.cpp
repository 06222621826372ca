// Tables and views of the per-codeword engines: one workgroup per codeword (amp_cw.hip) and the split form
// (amp_cw2.hip, amp_cw2d.hip).
#include <random>

#include "amp_plan.hpp"

namespace sg {

// Bank-aware placement of items (rows, row pairs) on the threads, shared by the two engines.  own[t] lists
// thread t's items in slot order, item r filling len_of(r) consecutive slots of the thread's KT; cell(at, g, j)
// is the LDS cost of the reads of lane group g (threads 32 g .. 32 g + 31) at slot j, given the item at each
// (thread, slot) in at[t * KT + j] (-1: none).  Local search from the load-balanced placement: swap two items
// of the same length that start at the same slot of threads in different lane groups when the summed cost of
// the cells they touch does not grow.  Deterministic (fixed seed); the slot structure of every thread is unchanged.
template <typename Len, typename Cell>
static void bank_balance(std::vector<std::vector<int>> &own, int KT, Len len_of, Cell cell) {
    const int T = (int)own.size();
    std::vector<int> at((size_t)T * KT, -1), pos((size_t)T * KT, -1), start((size_t)T * KT, 0);
    for (int t = 0; t < T; ++t) {  // item / list position at each slot; items start where flagged
        int j = 0;
        for (int i = 0; i < (int)own[t].size(); ++i) {
            const int r = own[t][i], len = len_of(r);
            start[(size_t)t * KT + j] = len;
            for (int q = 0; q < len; ++q, ++j) {
                at[(size_t)t * KT + j] = r;
                pos[(size_t)t * KT + j] = i;
            }
        }
    }
    // candidates by (start slot, length)
    std::vector<std::vector<int>> by((size_t)KT * (KT + 1));
    for (int t = 0; t < T; ++t)
        for (int j = 0; j < KT; ++j)
            if (const int len = start[(size_t)t * KT + j]) by[(size_t)j * (KT + 1) + len].push_back(t);
    std::mt19937 rng(12345);
    const int iters = 8 * T * KT;
    for (int it = 0; it < iters; ++it) {
        const int A = (int)(rng() % T), j = (int)(rng() % KT), len = start[(size_t)A * KT + j];
        if (!len) continue;
        const auto &cand = by[(size_t)j * (KT + 1) + len];
        const int B = cand[rng() % cand.size()];
        const int gA = A / 32, gB = B / 32;
        if (gA == gB) continue;
        int before = 0, after = 0;
        for (int q = j; q < j + len; ++q) before += cell(at, gA, q) + cell(at, gB, q);
        for (int q = j; q < j + len; ++q) std::swap(at[(size_t)A * KT + q], at[(size_t)B * KT + q]);
        for (int q = j; q < j + len; ++q) after += cell(at, gA, q) + cell(at, gB, q);
        if (after > before) {
            for (int q = j; q < j + len; ++q) std::swap(at[(size_t)A * KT + q], at[(size_t)B * KT + q]);
            continue;
        }
        std::swap(own[A][pos[(size_t)A * KT + j]], own[B][pos[(size_t)B * KT + j]]);
    }
}

// The rows of the per-codeword engine (amp_cw.hip cw_accumulate: at slot j, lanes 0-31 and 32-63 of a
// wavefront each read one image value at fsw(k1) with ds_read_b64, whose bank pair is fsw(k1) mod 32; distinct
// rows on one bank pair serialise): the cost is the worst bank multiplicity over distinct addresses.
static void cw_bank_balance(std::vector<std::vector<int>> &own, const std::vector<int32_t> &row_k1,
                            const std::vector<int32_t> &kptr, int KT) {
    bank_balance(own, KT, [&](int r) { return kptr[r + 1] - kptr[r]; }, [&](const std::vector<int> &at, int g, int j) {
        int a[32], cnt[32] = {0}, worst = 0;
        for (int l = 0; l < 32; ++l) {
            const int r = at[(size_t)(g * 32 + l) * KT + j];
            a[l] = r < 0 ? 0 : fsw(row_k1[r]);
            bool dup = false;
            for (int m = 0; m < l && !dup; ++m) dup = a[m] == a[l];
            if (!dup) worst = std::max(worst, ++cnt[a[l] & 31]);
        }
        return worst;
    });
}

// Per-codeword engine tables (amp_cw.hip): the needed indices of each row go
// to one thread (longest rows first, to the least loaded thread), so a thread
// owns at most KT indices; slot (j, tid) at j * 1024 + tid; then
// cw_bank_balance.
int build_cw(sg_amp_plan *p, const std::vector<int32_t> &row_k1, const std::vector<int32_t> &kptr,
             const std::vector<int32_t> &kk2, const std::vector<int32_t> &oa, const std::vector<int32_t> &ob,
             const std::vector<int32_t> &gi, const std::vector<cd> &gc, const std::vector<int32_t> &cls_ptr,
             const std::vector<uint32_t> &cls_ls) {
    const int nr = (int)row_k1.size(), nk = kptr[nr];
    if (nk > 14 * CW_THREADS) return SG_OK;  // 12 slots per thread in LDS beside the image, 2 in registers
    std::vector<int> rows(nr);
    for (int r = 0; r < nr; ++r) rows[r] = r;
    std::stable_sort(rows.begin(), rows.end(),
                     [&](int a, int b) { return kptr[a + 1] - kptr[a] > kptr[b + 1] - kptr[b]; });
    std::vector<std::pair<int, int>> heap;  // (load, thread), min-heap
    for (int i = 0; i < CW_THREADS; ++i) heap.push_back({0, i});
    auto cmp = [](const std::pair<int, int> &a, const std::pair<int, int> &b) { return a > b; };
    std::make_heap(heap.begin(), heap.end(), cmp);
    std::vector<std::vector<int>> own(CW_THREADS);
    int KT = 0;
    for (int r : rows) {
        std::pop_heap(heap.begin(), heap.end(), cmp);
        auto &h = heap.back();
        own[h.second].push_back(r);
        h.first += kptr[r + 1] - kptr[r];
        KT = std::max(KT, h.first);
        std::push_heap(heap.begin(), heap.end(), cmp);
    }
    if (KT > 14) return SG_OK;  // the staged engine only
    KT = KT <= 12 ? 12 : 14;   // kernel instances (cw_iter<12>: all slots in LDS; <14>: two in registers)
    cw_bank_balance(own, row_k1, kptr, KT);
    const int P = p->rP, n = p->n;
    std::vector<uint32_t> kt((size_t)KT * CW_THREADS, 0u);
    std::vector<int32_t> cmap(nk, 0);
    for (int tid = 0; tid < CW_THREADS; ++tid) {
        int j = 0;
        for (int r : own[tid])
            for (int k = kptr[r]; k < kptr[r + 1]; ++k, ++j) {
                uint32_t e = ((uint32_t)row_k1[r] + (uint32_t)P * (uint32_t)kk2[k]) | CW_VALID;
                if (k == kptr[r]) e |= CW_NEWROW;
                if (k == kptr[r + 1] - 1) e |= CW_ENDROW;
                kt[(size_t)j * CW_THREADS + tid] = e;
                cmap[k] = j * CW_THREADS + tid;
            }
    }
    // forward outputs and inverse terms by slot; unused inverse terms: row 0
    // with coefficient 0 (the kernel reads all four)
    std::vector<int32_t> c_oa(n), c_ob(n), c_gi((size_t)KT * CW_THREADS * 4, 0);
    std::vector<cd> c_gc((size_t)KT * CW_THREADS * 4, cd(0, 0));
    for (int i = 0; i < n; ++i) {
        c_oa[i] = cmap[oa[i]];
        c_ob[i] = cmap[ob[i]];
    }
    for (int k = 0; k < nk; ++k)
        for (int q = 0; q < 4; ++q) {
            const int32_t i = gi[(size_t)k * 4 + q];
            if (i >= 0) {
                c_gi[(size_t)cmap[k] * 4 + q] = i;
                c_gc[(size_t)cmap[k] * 4 + q] = gc[(size_t)k * 4 + q];
            }
        }
    // stage twiddles of the P-point FFT at 8 elements per thread (fft.hpp layout)
    const std::vector<cd> stw = stage_twiddles(p->rlog2P, 8);
    // Which image values the class scatter (Ab, class m2 < Q) and the row
    // writes (Az, entry Q) leave behind, as bits of the thread that reads them
    // in the first FFT stage (amp_cw.hip cw_stage0_r16: thread of complex
    // index m1 = j + 512 g reads it as value g & 7, bit 2 (g & 7) + component),
    // so that stage masks stale values instead of the image being zeroed.
    const int Q = p->rQ;
    std::vector<uint16_t> cmask((size_t)(Q + 1) * CW_THREADS, 0);
    auto mbit = [&](int m2, int m1, int c) {
        const int j = m1 & 511, g = m1 >> 9;
        const int tid = ((j >> 5) << 6) | ((g >> 3) << 5) | (j & 31);
        cmask[(size_t)m2 * CW_THREADS + tid] |= (uint16_t)(1u << (2 * (g & 7) + c));
    };
    for (int m2 = 0; m2 < Q; ++m2)
        for (int q = cls_ptr[m2]; q < cls_ptr[m2 + 1]; ++q) {
            const int loc = (int)(cls_ls[q] & 0xffffu);
            mbit(m2, fsw(loc >> 1), loc & 1);  // fsw is its own inverse
        }
    for (int r = 0; r < nr; ++r) {
        mbit(Q, row_k1[r], 0);
        mbit(Q, row_k1[r], 1);
    }
    SG_TRY(p->tables.upload(&p->c_cmask, cmask));
    SG_TRY(p->tables.upload(&p->c_kt, kt));
    SG_TRY(p->tables.upload(&p->c_oa, c_oa));
    SG_TRY(p->tables.upload(&p->c_ob, c_ob));
    SG_TRY(p->tables.upload(&p->c_gi, c_gi));
    SG_TRY(upload_cx(p, &p->c_gc, c_gc));
    SG_TRY(upload_cx(p, &p->c_stw, stw));
    p->cwKT = KT;
    p->cw = true;
    return SG_OK;
}

// The conjugate row pairs of the split engine (amp_cw2.hip: at slot j the lanes of each 32-lane half of a
// wavefront read rows r and P - r of their slot's pair with ds_read_b64, bank pair c2pos(row) mod 32, in cw2_ab's
// accumulation, and write them in cw2_az's rows).  Every output keeps its arithmetic (same slot structure per
// thread, same class order); only the order of cw2_ctrl's sum of z^2 (phi) follows the placement.
static void cw2_bank_balance(std::vector<std::vector<int>> &own, const std::vector<std::vector<int>> &pair_of,
                             int OT, int P) {
    // the lanes of a group hold distinct pairs at a slot, so distinct rows; empty slots all read row 0
    bank_balance(own, OT, [&](int r) { return (int)pair_of[r].size(); }, [&](const std::vector<int> &at, int g, int j) {
        int ca[32] = {0}, cb[32] = {0}, wa = 0, wb = 0;
        bool empty = false;
        for (int l = 0; l < 32; ++l) {
            const int r = at[(size_t)(g * 32 + l) * OT + j];
            if (r < 0) {
                if (empty) continue;
                empty = true;
            }
            const int ra = r < 0 ? 0 : r, rb = r < 0 ? 0 : (P - r) % P;
            wa = std::max(wa, ++ca[c2pos(ra) & 31]);
            if (rb != ra) wb = std::max(wb, ++cb[c2pos(rb) & 31]);
        }
        return wa + wb;
    });
}

// Split per-codeword engine tables (amp_cw2.hip).  Output i at DCT position
// K reads H[a] and H[b], b = N2 - a (fwd_coef), and its inverse input adds to
// G[a] and G[b] (inv_contrib: first call a, second b): both touch only the
// conjugate row pair {a mod P, P - a mod P} of the P-point stage.  Each output
// is normalised so that a mod P is the smaller row of its pair (swapping a and
// b takes (c1, c2) to (conj c2, conj c1) and (al, be) to (be, al):
// Re(x) = Re(conj x)); the outputs of a pair go to one thread (the largest
// pairs first, each to the least loaded thread), at most OT per thread; a
// thread's slots list its pairs one after the other (CW_NEWROW on the first
// output of a pair, CW_ENDROW on the last, CW_SELF when the pair's rows
// coincide: r = 0 or P / 2).  Plus the first-FFT-stage masks of the
// 16-values-per-thread transform (amp_cw2.hip c2_stage0_r32).
int build_cw2(sg_amp_plan *p, const uint32_t *o0, double sc, const std::vector<int32_t> &row_k1,
              const std::vector<int32_t> &cls_ptr, const std::vector<uint32_t> &cls_ls) {
    const long long N = p->w, N2 = p->N2;
    const int P = p->rP, n = p->n, T = CW2_THREADS, Q = p->rQ;
    if (P != 8192 || Q % 2 || p->Lblk > 2 * T || p->rmaxcls > CW2_SLICE) return SG_OK;
    struct Out { long long a; cd c1, c2, al, be; };
    std::vector<Out> out(n);
    std::vector<std::vector<int>> pair_of(P / 2 + 1);
    for (int i = 0; i < n; ++i) {
        Out &o = out[i];
        long long b;
        fwd_coef(o0[i], N, N2, sc, &o.a, &b, &o.c1, &o.c2);
        int nc = 0;
        bool ok = true;
        o.al = o.be = cd(0, 0);
        inv_contrib(o0[i], N, N2, sc, [&](long long k, cd c) {
            if (nc++ == 0) {
                ok = ok && k % N2 == o.a;
                o.al = c;
            } else {
                ok = ok && k % N2 == b;
                o.be = c;
            }
        });
        SG_CHECK_ARG(ok && nc <= 2, "internal: inverse input of output %d outside its pair", i);
        const int r = (int)(o.a % P), r2 = (P - r) % P;
        if (r > r2) {  // normalise: a mod P is the smaller row of the pair
            o.a = b;
            const cd c1 = o.c1, al = o.al;
            o.c1 = std::conj(o.c2);
            o.c2 = std::conj(c1);
            o.al = o.be;
            o.be = al;
        }
        pair_of[(int)(o.a % P)].push_back(i);
    }
    std::vector<int> pairs;
    for (int r = 0; r <= P / 2; ++r)
        if (!pair_of[r].empty()) pairs.push_back(r);
    std::stable_sort(pairs.begin(), pairs.end(),
                     [&](int x, int y) { return pair_of[x].size() > pair_of[y].size(); });
    std::vector<std::pair<int, int>> heap;  // (load, thread), min-heap
    for (int i = 0; i < T; ++i) heap.push_back({0, i});
    auto cmp = [](const std::pair<int, int> &x, const std::pair<int, int> &y) { return x > y; };
    std::make_heap(heap.begin(), heap.end(), cmp);
    std::vector<std::vector<int>> own(T);
    int OT = 0;
    for (int r : pairs) {
        std::pop_heap(heap.begin(), heap.end(), cmp);
        auto &h = heap.back();
        own[h.second].push_back(r);
        h.first += (int)pair_of[r].size();
        OT = std::max(OT, h.first);
        std::push_heap(heap.begin(), heap.end(), cmp);
    }
    if (OT > 16) return SG_OK;  // kernel instances for 12, 13, 14 and 16 outputs per thread
    OT = OT <= 12 ? 12 : OT <= 14 ? OT : 16;
    cw2_bank_balance(own, pair_of, OT, P);
    std::vector<uint32_t> ka((size_t)OT * T, 0u);
    std::vector<int32_t> oi((size_t)OT * T, 0);
    std::vector<float> cf((size_t)OT * T * 4, 0.f);
    const bool f64 = p->precision == SG_F64;
    std::vector<double> cfd(f64 ? (size_t)OT * T * 4 : 0, 0.0), gfd(f64 ? (size_t)OT * T * 4 : 0, 0.0),
        sad(f64 ? (size_t)OT * T * 2 : 0, 0.0);
    for (size_t i = 0; i < sad.size(); i += 2) sad[i] = 1.0;  // invalid slots: S = 1
    // Polar form of the inverse coefficients (amp_cw2.hip Az rows): with U = 1 / (4N) revolutions,
    // inv_contrib's al and be are real multiples of unit phasors, al = |al| e^(2 pi i A U) and
    // be = |be| e^(2 pi i (N - A) U), A = 3a + o N/2 (o in {0, 1, 6, 7} by the output's case: q below or
    // above N2, normalised by a swap or not).  Then the rows' al conj(W) and be W (W = w_N2^(m2 a)) are
    // |al| (cos x, sin x) and |be| (sin x, cos x) of ONE angle x = ((3 + 8 m2) a + o N/2) U: the rows
    // need the slot word and z/phi scaled by |al|, |be| (cw2_ctrl), not the complex (al, be) per class.
    // Fitted and checked per output here (any mismatch: no split engine for the plan).
    std::vector<float> gm((size_t)OT * T * 2, 0.f);
    const bool pow2 = N >= 4 && (N & (N - 1)) == 0 && 4 * N <= (1ll << 24);
    auto polar = [&](const Out &o, uint32_t *code, double *ma, double *mb) -> bool {
        if (!pow2) return false;
        const long long N4 = 4 * N;
        double best = 1e300;
        for (uint32_t c : {0u, 1u, 6u, 7u}) {
            const long long A = ((3 * o.a + (long long)c * (N / 2)) % N4 + N4) % N4;
            const cd ra = o.al * expi(-2.0 * M_PI * (double)A / (double)N4);
            const cd rb = o.be * expi(-2.0 * M_PI * (double)(N - A) / (double)N4);
            const double err = std::abs(ra.imag()) + std::abs(rb.imag());
            if (err < best) {
                best = err;
                *code = c;
                *ma = ra.real();
                *mb = rb.real();
            }
        }
        return best <= 1e-12 * (std::abs(o.al) + std::abs(o.be) + 1e-300);
    };
    if (p->precision != SG_F64 && !pow2) return SG_OK;
    std::vector<uint32_t> last_word(T, 0u);
    for (int tid = 0; tid < T; ++tid) {
        int j = 0;
        // (f32 only: amp_cw2.hip's rows write where the thread's last pair is; the f64 form has no padding-slot rows)
        if (p->precision != SG_F64 && own[tid].empty()) return SG_OK;
        for (int r : own[tid]) {
            const auto &lst = pair_of[r];
            for (size_t q = 0; q < lst.size(); ++q, ++j) {
                const int i = lst[q];
                const Out &o = out[i];
                uint32_t e = (uint32_t)o.a | CW_VALID;
                if (q == 0) e |= CW_NEWROW;
                if (q + 1 == lst.size()) e |= CW_ENDROW;
                if (r == 0 || 2 * r == P) e |= CW_SELF;
                const size_t c = (size_t)j * T + tid;
                if (p->precision != SG_F64) {
                    uint32_t code = 0;
                    double ma = 0.0, mb = 0.0;
                    if (!polar(o, &code, &ma, &mb)) return SG_OK;  // (not the DCT's coefficients: no split engine)
                    e |= code << CW_OFFSHIFT;
                    gm[2 * c] = (float)ma;
                    gm[2 * c + 1] = (float)mb;
                }
                ka[c] = e;
                oi[c] = i;
                last_word[tid] = e & ~(CW_VALID | CW_NEWROW);  // (the padding slots below)
                const float v[4] = {(float)o.c1.real(), (float)o.c1.imag(), (float)o.c2.real(), (float)o.c2.imag()};
                std::copy(v, v + 4, cf.begin() + 4 * c);
                if (f64) {
                    const double d[8] = {o.c1.real(), o.c1.imag(), o.c2.real(), o.c2.imag(),
                                         o.al.real(), o.al.imag(), o.be.real(), o.be.imag()};
                    std::copy(d, d + 4, cfd.begin() + 4 * c);
                    std::copy(d + 4, d + 8, gfd.begin() + 4 * c);
                    const cd w = tw(o.a, N2);  // S = w_N2^a (amp_cw2d.hip: Horner / rotation step per class)
                    sad[2 * c] = w.real();
                    sad[2 * c + 1] = w.imag();
                }
            }
        }
    }
    // Padding slots (after a thread's pairs; zero coefficients, zero z/phi scale, not VALID) carry the word of
    // the thread's last output without CW_NEWROW: the f32 rows (amp_cw2.hip cw2_az) write every
    // slot's running sum at its pair's rows, so a padding slot adds 0 to the last pair's sums and writes them
    // again -- never a row of another thread's pair
    if (p->precision != SG_F64)
        for (int tid = 0; tid < T; ++tid)
            for (int j = 0; j < OT; ++j) {
                uint32_t &e = ka[(size_t)j * T + tid];
                if (!(e & CW_VALID)) e = last_word[tid];
            }
    // Which image values the class scatter (Ab, class m2 < Q) and the row
    // writes (Az, entry Q) leave behind, as bits of the thread that reads
    // them in the first FFT stage (c2_stage0_r32: complex index m1 = j + 256 g
    // is value g & 15 of lane half g >> 4 of butterfly j; bit 2 (g & 15) + c)
    std::vector<uint32_t> cmask((size_t)(Q + 1) * T, 0u);
    auto mbit = [&](int m2, int m1, int c) {
        const int j = m1 & 255, g = m1 >> 8;
        const int tid = ((j >> 5) << 6) | ((g >> 4) << 5) | (j & 31);
        cmask[(size_t)m2 * T + tid] |= 1u << (2 * (g & 15) + c);
    };
    for (int m2 = 0; m2 < Q; ++m2)
        for (int q = cls_ptr[m2]; q < cls_ptr[m2 + 1]; ++q) {
            const int loc = (int)(cls_ls[q] & 0xffffu);
            mbit(m2, fsw(loc >> 1), loc & 1);  // fsw is its own inverse
        }
    for (int r : row_k1) {
        mbit(Q, r, 0);
        mbit(Q, r, 1);
    }
    // class tables padded to CW2_SLICE entries per class, the padding pointing
    // at the trash slot (section 0), so the kernels need no range checks
    // (entries re-addressed from the one-workgroup engine's fsw image to the
    // split engine's padded one, c2pos)
    std::vector<uint32_t> cls2((size_t)Q * CW2_SLICE, CW2_TRASH);
    for (int m2 = 0; m2 < Q; ++m2)
        for (int q = cls_ptr[m2]; q < cls_ptr[m2 + 1]; ++q) {
            const uint32_t loc = cls_ls[q] & 0xffffu;
            const uint32_t pl = 2u * (uint32_t)c2pos(fsw((int)(loc >> 1))) + (loc & 1u);
            cls2[(size_t)m2 * CW2_SLICE + (q - cls_ptr[m2])] = (cls_ls[q] & ~0xffffu) | pl;
        }
    SG_TRY(p->tables.upload(&p->c2_cls, cls2));
    {  // image positions alone, two per word (cw2_az's gathers: entries tl + 512 i and tl + 512 (i + 9)), and
       // the same entries' sections in a table of their own (cw2_az's beta_prev, requested after its transform)
        constexpr int H = CW2_SLICE / 2;
        std::vector<uint32_t> clsp((size_t)Q * H), clss((size_t)Q * H);
        for (int m2 = 0; m2 < Q; ++m2)
            for (int q = 0; q < H; ++q) {
                const uint32_t *c = &cls2[(size_t)m2 * CW2_SLICE];
                clsp[(size_t)m2 * H + q] = (c[q] & 0xffffu) | (c[q + H] << 16);
                clss[(size_t)m2 * H + q] = (c[q] >> 16) | (c[q + H] & ~0xffffu);
            }
        SG_TRY(p->tables.upload(&p->c2_clsp, clsp));
        if (!f64) SG_TRY(p->tables.upload(&p->c2_clss, clss));
    }
    SG_TRY(p->tables.upload(&p->c2_cmask, cmask));
    SG_TRY(p->tables.upload(&p->c2_ka, ka));
    {  // thread-major copy: thread tid's slots at [tid][OTP] (amp_cw2.hip loads them 16 bytes at a time)
        const int OTP = cw2_otp(OT);
        std::vector<uint32_t> kat((size_t)OTP * T, 0u);
        for (int tid = 0; tid < T; ++tid)
            for (int j = 0; j < OT; ++j) kat[(size_t)tid * OTP + j] = ka[(size_t)j * T + tid];
        SG_TRY(p->tables.upload(&p->c2_kat, kat));
    }
    SG_TRY(p->tables.upload(&p->c2_oi, oi));
    SG_TRY(p->tables.upload((float **)&p->c2_cf, cf));
    SG_TRY(p->tables.upload(&p->c2_gm, gm));
    {  // thread-major copy of (|al|, |be|): thread tid's slots at [tid][OTP][2] (16-byte loads of two slots)
        const int OTP = cw2_otp(OT);
        std::vector<float> gmt((size_t)OTP * T * 2, 0.f);
        for (int tid = 0; tid < T; ++tid)
            for (int j = 0; j < OT; ++j)
                for (int c = 0; c < 2; ++c) gmt[((size_t)tid * OTP + j) * 2 + c] = gm[((size_t)j * T + tid) * 2 + c];
        SG_TRY(p->tables.upload(&p->c2_gmt, gmt));
    }
    p->c2_shoff = pow2 ? ilog2((int)(N / 2)) : 0;
    if (f64) {
        std::vector<double> twp((size_t)P * 2);
        for (int k = 0; k < P; ++k) {
            const cd w = tw(k, P);
            twp[2 * k] = w.real();
            twp[2 * k + 1] = w.imag();
        }
        SG_TRY(p->tables.upload(&p->c2d_cf, cfd));
        SG_TRY(p->tables.upload(&p->c2d_gf, gfd));
        SG_TRY(p->tables.upload(&p->c2d_sa, sad));
        SG_TRY(p->tables.upload(&p->c2d_twp, twp));
    }
    p->cw2OT = OT;
    return SG_OK;
}

CwTables ctables(const sg_amp_plan *p, int B) {
    CwTables tb;
    tb.L = p->L; tb.M = p->M; tb.LM = p->LM; tb.n = p->n; tb.N2 = p->N2; tb.Q = p->rQ; tb.Lblk = p->Lblk;
    tb.KT = p->cwKT; tb.log2P = p->rlog2P; tb.maxcls = p->rmaxcls; tb.maxseg = p->rmaxseg;
    tb.img = p->rimg;
    tb.cmask = p->c_cmask;
    tb.kt = p->c_kt; tb.oa = p->c_oa; tb.ob = p->c_ob; tb.oc = (const cx<float> *)p->r_oc;
    tb.gi = p->c_gi; tb.gc = (const cx<float> *)p->c_gc;
    tb.cls_ptr = p->r_cls_ptr; tb.cls_ls = p->r_cls_ls; tb.qpos = p->r_qpos; tb.seg = p->r_seg;
    tb.stw = (const cx<float> *)p->c_stw;
    tb.inv_n2 = 1.0f / (float)p->N2;
    // [B][32] stamps (one workgroup per codeword), only when the diagnostics buffer holds them
    tb.tprof = p->tprof_items * 20 >= (size_t)32 * B ? p->tprof.at<uint64_t>() : nullptr;  // (null when empty)
    return tb;
}

Cw2Tables c2tables(const sg_amp_plan *p, int B) {
    Cw2Tables tb;
    tb.L = p->L; tb.M = p->M; tb.LM = p->LM; tb.n = p->n; tb.N2 = p->N2; tb.Q = p->rQ; tb.Lblk = p->Lblk;
    tb.OT = p->cw2OT; tb.maxcls = p->rmaxcls;
    // (build_cw2: Q even; the decode loop asks for more than two once codewords have stopped)
    tb.np = p->c2_np >= 4 && CW2_NP >= 4 && p->rQ % 4 == 0 ? 4 : 2;
    tb.inv_n2 = 1.0f / (float)p->N2;
    tb.cmask = p->c2_cmask; tb.ka = p->c2_ka; tb.kat = p->c2_kat; tb.oi = p->c2_oi;
    tb.cf = (const float4 *)p->c2_cf; tb.gm = (const float2 *)p->c2_gm;
    tb.gmt = (const float4 *)p->c2_gmt;
    tb.sh_off = p->c2_shoff; tb.m4n = (uint32_t)(4 * p->w - 1); tb.inv_4n = (float)(1.0 / (4.0 * (double)p->w));
    tb.cls_ptr = p->r_cls_ptr; tb.cls_ls = p->r_cls_ls; tb.cls2 = p->c2_cls; tb.clsp = p->c2_clsp; tb.clss = p->c2_clss;
    tb.qpos = p->r_qpos; tb.seg = p->r_seg;
    tb.xr = (float *)p->ws_c2xp; tb.vz = (float *)p->ws_c2vz; tb.ys = (float *)p->ws_c2ys; tb.zs = (float *)p->ws_c2zs; tb.part = (float4 *)p->ws_c2part;
    // [np B][64] stamps (workgroup blockIdx.x < np B writes 64 blockIdx.x + k), only when the diagnostics
    // buffer holds them (build_cw2 accepts any even Q, and its B * Q * 20 entries are fewer for small Q)
    tb.tprof = p->tprof_items * 20 >= (size_t)64 * tb.np * B ? p->tprof.at<uint64_t>() : nullptr;
    return tb;
}

Cw2dTables c2dtables(const sg_amp_plan *p) {
    Cw2dTables tb;
    tb.L = p->L; tb.M = p->M; tb.LM = p->LM; tb.n = p->n; tb.N2 = p->N2; tb.Q = p->rQ; tb.Lblk = p->Lblk;
    tb.OT = p->cw2OT; tb.maxcls = p->rmaxcls;
    tb.cmask = p->c2_cmask; tb.ka = p->c2_ka; tb.kat = p->c2_kat; tb.oi = p->c2_oi;
    tb.cf = p->c2d_cf; tb.gf = p->c2d_gf; tb.sa = p->c2d_sa; tb.twp = p->c2d_twp;
    tb.cls_ptr = p->r_cls_ptr; tb.cls2 = p->c2_cls; tb.qpos = p->r_qpos; tb.seg = p->r_seg;
    tb.xr = (double *)p->ws_c2xp; tb.vz = (double *)p->ws_c2vz; tb.ys = (double *)p->ws_c2ys;
    tb.zs = (double *)p->ws_c2zs; tb.beta = (double *)p->ws_c2beta; tb.sec = (double *)p->ws_c2sec;
    return tb;
}

}  // namespace sg
