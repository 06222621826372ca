// Tables and view of the block engines: several transforms per column block, single-class (amp_block.hip) and
// two-class (amp_block2.hip).
#include "amp_plan.hpp"

namespace sg {

// Tables of the block engine (amp_block.hip): per transform, the LDS position
// of every column entry, the output gathers and the G slots, all in the
// natural-order FFT image in the padded layout (fft.hpp ppos).
int build_block(sg_amp_plan *p, const uint32_t *order0, const uint32_t *order1, const std::vector<double> &t_scale,
                const std::vector<int32_t> &row_of) {
    const long long N = p->w, N2 = p->N2;
    const int nT = p->nT, Mc = p->Mc, Mr = p->Mr;
    std::vector<uint16_t> gloc;
    std::vector<uint32_t> pos2((size_t)nT * 8 * 1024, 0u);
    std::vector<uint32_t> oab((size_t)nT * Mr);
    std::vector<cd> oc((size_t)nT * Mr * 8), gc;
    std::vector<int32_t> gptr(nT + 1, 0), gi, grow;
    std::vector<GSlot> gs;
    for (int t = 0; t < nT; ++t) {
        const uint32_t *o0 = order0 + (size_t)t * Mr, *o1 = order1 + (size_t)t * Mc;
        for (int j = 0; j < Mc; ++j) {
            const long long sl = slot_of_pos(o1[j], N);
            const uint32_t lds = (uint32_t)(2 * ppos((int)(sl >> 1)) + (int)(sl & 1));
            SG_CHECK_ARG(lds < 65536u, "internal: padded LDS index beyond 16 bits");
            // owner (thread, entry) of column entry j: amp_block_common.hpp blk_j at 16 entries per thread
            const int M = p->M, eps = M / 64, spw = 1024 / M;
            const int l = j / M, rr = j % M;
            const int tid = (l / spw) * 64 + rr / eps, i = (l % spw) * eps + rr % eps;
            pos2[((size_t)t * 8 + i / 2) * 1024 + tid] |= lds << (16 * (i & 1));
        }
        for (int i = 0; i < Mr; ++i) {
            long long a, b;
            cd c1, c2;
            fwd_coef(o0[i], N, N2, t_scale[t], &a, &b, &c1, &c2);
            // amp_block.hip blk_ab: the radix-4 stage of bins a, b folded into the output
            oab[(size_t)t * Mr + i] = (uint32_t)(a % 4096) | ((uint32_t)(b % 4096) << 16);
            for (int q = 0; q < 4; ++q) {
                oc[((size_t)t * Mr + i) * 8 + q] = c1 * tw((long long)q * a, N2);
                oc[((size_t)t * Mr + i) * 8 + 4 + q] = c2 * std::conj(tw((long long)q * b, N2));
            }
        }
        SG_TRY(gather_gslots(o0, Mr, N, N2, t_scale[t], &gs));
        for (const GSlot &g : gs) {
            gloc.push_back((uint16_t)ppos(g.k));
            grow.push_back(row_of[t]);
            for (int q = 0; q < 4; ++q) gi.push_back(g.i[q]), gc.push_back(g.c[q]);
        }
        gptr[t + 1] = (int32_t)gloc.size();
    }
    // per-stage twiddles of the N2-point FFT (fft.hpp lds_fft1_ct, EPT 16)
    const std::vector<cd> stw = stage_twiddles(ilog2((int)N2), 16);
    SG_TRY(p->tables.upload(&p->b_pos2, pos2));
    SG_TRY(p->tables.upload(&p->b_oab, oab));
    SG_TRY(upload_cx(p, &p->b_oc, oc));
    SG_TRY(p->tables.upload(&p->b_gptr, gptr));
    SG_TRY(p->tables.upload(&p->b_grow, grow));
    p->b_ngs = gptr[nT];
    SG_TRY(p->tables.upload(&p->b_gloc, gloc));
    SG_TRY(p->tables.upload(&p->b_gi, gi));
    SG_TRY(upload_cx(p, &p->b_gc, gc));
    SG_TRY(upload_cx(p, &p->b_stw, stw));
    SG_CHECK_ARG(blk_lds_bytes(Mc) <= 160 * 1024, "block engine LDS budget");
    return SG_OK;
}

// Tables of the two-class block engine (amp_block2.hip): N2 = 2 P with P = 2^14
// (w = 2^16) or 2^13 (w = 2^15).  Column entry j sits at packed slot
// m = 2 m1 + m2 of its transform: class m2, real LDS index 2 ppos(m1) +
// component in the class image; owned by (thread, entry) as blk_j at 32 entries per thread.  Output
// coefficients per class fold the class factor w_N2^(m2 k) and the last
// radix-RF stage (RF = P / 4096): al = c1 w_N2^((m2 + 2 r) a).
int build_block2(sg_amp_plan *p, const uint32_t *order0, const uint32_t *order1, const std::vector<double> &t_scale,
                 const std::vector<int32_t> &row_of) {
    const long long N = p->w, N2 = p->N2;
    const int nT = p->nT, Mc = p->Mc, Mr = p->Mr, M = p->M;
    const int LP = p->b2_log2p, T = (1 << LP) / 16, RF = (1 << LP) / 4096;  // amp_block2.hip B2G
    constexpr int J = 32;
    SG_CHECK_ARG((LP == 13 || LP == 14) && N2 == 2LL << LP && Mc == 2 << LP, "internal: two-class geometry");
    // per (transform, class): the real LDS index 2 ppos(m1) + component of each column entry of the class in
    // the padded image, the trash slot (a padding slot, amp_block2.hip B2_TRASH) for the other class's entries
    constexpr uint32_t TRASH = 2 * 32;
    static_assert(ppos(32) == 33, "complex position 32 is a padding slot");
    std::vector<uint32_t> pos2((size_t)nT * 2 * (J / 2) * T, TRASH | (TRASH << 16));
    std::vector<uint32_t> oab((size_t)nT * Mr);
    std::vector<cd> oc((size_t)nT * 2 * Mr * 8), gc;
    std::vector<int32_t> gptr(nT + 1, 0), gi, grow, gk;
    std::vector<uint16_t> gloc;
    std::vector<GSlot> gs;
    const int eps = M / 64, spw = 2048 / M;
    for (int t = 0; t < nT; ++t) {
        const uint32_t *o0 = order0 + (size_t)t * Mr, *o1 = order1 + (size_t)t * Mc;
        for (int j = 0; j < Mc; ++j) {
            const long long sl = slot_of_pos(o1[j], N);
            const long long m = sl >> 1;
            const uint32_t lds = (uint32_t)(2 * ppos((int)(m >> 1)) + (int)(sl & 1));
            SG_CHECK_ARG(lds < 65536u, "internal: padded LDS index beyond 16 bits");
            const int l = j / M, rr = j % M;
            const int tid = (l / spw) * 64 + rr / eps, i = (l % spw) * eps + rr % eps;
            uint32_t &w = pos2[(((size_t)t * 2 + (m & 1)) * (J / 2) + i / 2) * T + tid];
            w = (w & ~(0xffffu << (16 * (i & 1)))) | (lds << (16 * (i & 1)));
        }
        for (int i = 0; i < Mr; ++i) {
            long long a, b;
            cd c1, c2;
            fwd_coef(o0[i], N, N2, t_scale[t], &a, &b, &c1, &c2);
            oab[(size_t)t * Mr + i] = (uint32_t)(a % 4096) | ((uint32_t)(b % 4096) << 16);
            for (int m2 = 0; m2 < 2; ++m2)
                for (int r = 0; r < RF; ++r) {  // (the last radix-RF stage folded in; RF = 2 leaves 4 zeros)
                    cd *o = &oc[(((size_t)t * 2 + m2) * Mr + i) * 8];
                    o[r] = c1 * tw((long long)(m2 + 2 * r) * a, N2);
                    o[4 + r] = c2 * std::conj(tw((long long)(m2 + 2 * r) * b, N2));
                }
        }
        SG_TRY(gather_gslots(o0, Mr, N, N2, t_scale[t], &gs));
        for (const GSlot &g : gs) {
            gk.push_back(g.k);
            gloc.push_back((uint16_t)ppos(g.k & (int)(N2 / 2 - 1)));  // (blk2_az computes it from gk)
            grow.push_back(row_of[t]);
            for (int q = 0; q < 4; ++q) gi.push_back(g.i[q]), gc.push_back(g.c[q]);
        }
        gptr[t + 1] = (int32_t)gk.size();
    }
    // stage twiddles of the P-point FFT (fft.hpp lds_fft1_ct, EPT 16; unused by the sine / cosine stages of
    // amp_block2.hip)
    const std::vector<cd> stw = stage_twiddles(LP, 16);
    SG_TRY(p->tables.upload(&p->b_pos2, pos2));
    SG_TRY(p->tables.upload(&p->b_oab, oab));
    SG_TRY(upload_cx(p, &p->b_oc, oc));
    SG_TRY(p->tables.upload(&p->b_gptr, gptr));
    SG_TRY(p->tables.upload(&p->b_grow, grow));
    p->b_ngs = gptr[nT];
    SG_TRY(p->tables.upload(&p->b_gloc, gloc));
    SG_TRY(p->tables.upload(&p->b_gk, gk));
    SG_TRY(p->tables.upload(&p->b_gi, gi));
    SG_TRY(upload_cx(p, &p->b_gc, gc));
    SG_TRY(upload_cx(p, &p->b_stw, stw));
    SG_CHECK_ARG(blk2_lds_bytes(LP) <= 160 * 1024, "block engine LDS budget");
    return SG_OK;
}

BlkTables btables(const sg_amp_plan *p) {
    BlkTables tb;
    tb.nT = p->nT; tb.L = p->L; tb.M = p->M; tb.LM = p->LM; tb.n = p->n; tb.Lr = p->Lr; tb.Lc = p->Lc;
    tb.Mr = p->Mr; tb.Mc = p->Mc;
    tb.col_ptr = p->col_ptr; tb.col_t = p->col_t; tb.t_row = p->t_row;
    tb.pos2 = p->b_pos2; tb.oab = p->b_oab; tb.oc = (const cx<float> *)p->b_oc;
    tb.ngs = p->b_ngs; tb.gptr = p->b_gptr; tb.grow = p->b_grow; tb.gloc = p->b_gloc; tb.gi = p->b_gi; tb.gc = (const cx<float> *)p->b_gc;
    tb.gk = p->b_gk;
    tb.stw = (const cx<float> *)p->b_stw;
    tb.skip = diag_skip();
    tb.log2p = p->b2_log2p;
    return tb;
}

}  // namespace sg
