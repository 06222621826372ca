// The AMP <-> BP integrated decoders (sparc_new.py:257-282 naive, :411-439 naive posteriors, :472-502 integrated,
// :675-705 integrated posteriors) for a batch sharing one design: the one host loop of the dense Gaussian design
// (capi_dense.cpp) and of the sub-sampled DCT design (capi_amp.cpp).
#pragma once
#include "dense.hpp"
#include "integ_ws.hpp"

#pragma GCC visibility push(hidden)  // shared between the library's objects, not exported from it
namespace sg {

// Every LDPC block of every codeword goes through one batched BP launch per iteration; bits [B][nblk K] =
// app[:K] < 0 of the final its_final-iteration decode, whose BP output goes to d_app_out if given.  Nothing but
// launches and device-to-device copies.  `front` holds the steps in which the designs differ, enqueued on s:
//   forward(s)                xhat = A beta;
//   residual(t, ons_mode, s)  z and tau^2 = ||z||^2 / n, Onsager term as DenseBufs::ons_mode with ws.ons;
//   sections(t, s)            z -> weighted alpha (ws.alpha), P(bit = 0) (ws.vk0), LLRs (ws.llr); one of the two
//                             steps writes tau^2 of iteration t to the caller's history;
//   probs(app, nn, vk, s)     P(bit = 0) from the BP output;
//   beta(), tau(), snp        the estimate [B][LM], the tau^2 slot [B] the differentiated eta reads, sqrt(n P_l);
//   bsq_view()                the DenseBufs that dense_launch_bsq takes (beta, the shape, sec_bsq).
template <typename T, typename Front>
int integ_loop(Front &front, const IntegWs &ws, sg_graph *g, int mode, int N, int K, int B, int L, int M, int t_max,
               int its, int its_final, uint8_t *d_bits, void *d_app_out, hipStream_t s) {
    const bool naive = mode == SG_INT_NAIVE || mode == SG_INT_NAIVE_POST;
    const bool post = mode == SG_INT_NAIVE_POST || mode == SG_INT_DIFF_POST;
    const int ons_mode = naive ? 0 : (mode == SG_INT_DIFF ? 1 : 2);
    const int nbits = L * ilog2(M), nblk = nbits / N, prec = sizeof(T) == 8 ? SG_F64 : SG_F32;
    const size_t nb = (size_t)B * nbits;
    const double snp = front.snp;
    T *beta = front.beta(), *alpha_w = (T *)ws.alpha, *gamma = (T *)ws.gamma, *vk0 = (T *)ws.vk0, *vk = (T *)ws.vk;
    T *llr = (T *)ws.llr, *app = (T *)ws.app;
    for (int t = 0; t < t_max; ++t) {
        if (!naive && t > 0) {  // sum of the differentiated eta with the previous tau^2
            ProfScope ps(SG_PH_INT_DETA, s);
            SG_TRY(integ_launch_deta<T>(post ? 1 : 0, beta, gamma, alpha_w, snp, vk, vk0, front.tau(), B, L, M, snp,
                                        ws.part, ws.ons, (T *)nullptr, s));
        }
        if (t > 0) SG_TRY(front.forward(s));
        SG_TRY(front.residual(t, ons_mode, s));
        SG_TRY(front.sections(t, s));
        if (t == t_max - 1) {
            T *app_out = d_app_out ? (T *)d_app_out : app;
            SG_TRY(sg_ldpc_decode_device(g, SG_SUMPROD2, prec, llr, B * nblk, its_final, 0.7, app_out, ws.it, s));
            return integ_launch_hard_bits<T>(app_out, B * nblk, N, K, d_bits, s);
        }
        SG_TRY(sg_ldpc_decode_device(g, SG_SUMPROD2, prec, llr, B * nblk, its, 0.7, app, ws.it, s));
        ProfScope ps(SG_PH_INT_GLUE, s);
        SG_TRY(front.probs(app, nb, vk, s));
        if (!post) {
            SG_TRY(integ_launch_bp_to_beta<T>(vk, B, L, M, snp, 0, beta, s));
        } else {
            SG_TRY(integ_launch_bp_to_beta<T>(vk, B, L, M, snp, 1, gamma, s));
            SG_TRY(integ_launch_update<T>(gamma, alpha_w, snp, B, L, M, snp, beta, s));
        }
        if (naive) SG_TRY(dense_launch_bsq<T>(front.bsq_view(), s));  // ||beta||^2 of the BP-derived beta (Onsager)
    }
    return SG_OK;
}

}  // namespace sg
#pragma GCC visibility pop
