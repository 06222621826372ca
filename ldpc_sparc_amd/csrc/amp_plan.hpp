// The AMP design plan (sg_amp_plan), the host helpers its table builders share, and the kernel-facing views
// of a plan.  amp_plan.cpp: coefficient math, build_plan with the general engine's tables, workspace;
// amp_plan_regular.cpp, amp_plan_cw.cpp, amp_plan_block.cpp: the engines' builders; capi_amp.cpp: the drivers.
#pragma once
#include <algorithm>
#include <complex>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <vector>

#include "amp.hpp"
#include "amp_oploop.hpp"
#include "device_mem.hpp"
#include "integ_ws.hpp"

using cd = std::complex<double>;

struct sg_amp_plan {
    int precision = SG_F32;
    // what the last decode through this handle ran (sg_amp_last_decode): the
    // sub-plan (itself or the companion), its first engine, and the iteration
    // at which the per-codeword engine handed over to the staged one (-1: none)
    sg_amp_plan *last_ran = nullptr;
    int last_engine = -1, last_handover = -1;
    // batch size of the last decode through this handle whose final state (s / beta, tau) the sub-plan
    // last_ran still holds (sg_amp_llr_device); 0: none
    int last_B = 0;
    int device = 0;
    int ndim = 0, L = 0, M = 0, LM = 0, n = 0, Lr = 1, Lc = 1, Mr = 0, Mc = 0, nT = 0;
    int w = 0, N2 = 0, P = 0, Q = 0, log2P = 0, log2Q = 0, npairs = 0;
    std::vector<double> W;
    sg::DevPool tables;  // every device table of the plan (tables.upload into the members below)
    // general engine (four-step transform per nonzero block of W, amp_dct.hip) and the tables every engine reads
    int32_t *t_row = nullptr, *t_col = nullptr, *col_ptr = nullptr, *col_t = nullptr, *row_ptr = nullptr,
            *row_t = nullptr;
    int32_t *inmap = nullptr, *outslot = nullptr, *rp_ptr = nullptr, *rp_i = nullptr;
    uint32_t *rp_ab = nullptr;
    int32_t *gs_ptr = nullptr, *gs_loc = nullptr, *gs_i = nullptr;
    void *rp_c = nullptr, *gs_c = nullptr, *twP = nullptr, *twQ = nullptr, *twHi = nullptr, *twLo = nullptr;
    double *dW = nullptr;
    // batch workspace (grow-only, ensure_ws): every buffer below is a slot of ws, which plan_free_ws releases.
    // io (staging of the host entry points) grows by its own rule (ensure_io) and is freed with the workspace.
    sg::DevPool ws;
    int cap_B = 0, cap_tmax = 0;
    void *ws_beta = nullptr, *ws_y = nullptr, *ws_z = nullptr, *ws_rbuf = nullptr, *ws_buf0 = nullptr, *ws_buf1 = nullptr;
    sg::DevMem io;
    double *ws_phi = nullptr, *ws_tau = nullptr, *ws_sumsq = nullptr, *ws_err = nullptr;
    double *ws_psi = nullptr, *ws_psi_prev = nullptr, *ws_phi_prev = nullptr, *ws_gamma = nullptr, *ws_bco = nullptr;
    double *ws_nmse = nullptr;
    int32_t *ws_active = nullptr, *ws_argmax = nullptr, *ws_true = nullptr, *ws_tfinal = nullptr;
    // regular engine (one transform per column block, amp_fused.hip; build_regular)
    bool regular = false;
    int rP = 0, rQ = 0, rlog2P = 0, rept = 0, rmaxcls = 0, rmaxseg = 0, rimg = 0, nRmax = 0, nKmax = 0, RB = 0, nrb = 0, maxKb = 0, Lblk = 0, nB = 0;
    uint32_t *r_row_k1p = nullptr;
    int32_t *r_nR = nullptr, *r_row_k1 = nullptr, *r_kptr = nullptr, *r_kk2 = nullptr, *r_krho = nullptr;
    int32_t *r_oa = nullptr, *r_ob = nullptr, *r_gi = nullptr, *r_cls_ptr = nullptr, *r_cls_j = nullptr,
            *r_qpos = nullptr;
    uint32_t *r_cls_ls = nullptr;
    uint16_t *r_seg = nullptr;
    void *r_oc = nullptr, *r_gc = nullptr, *r_twP = nullptr, *r_twQ = nullptr, *r_stw = nullptr, *r_twa = nullptr,
         *r_twb = nullptr;
    // diagnostics: stage-1 phase timestamps; reallocated by ensure_ws while SG_AMP_TPROF is set, freed at destroy
    sg::DevMem tprof; size_t tprof_items = 0;
    // active-flag poll (ActivePoll): pinned host copy and its completion event
    int32_t *h_active = nullptr; int h_active_cap = 0;
    hipEvent_t poll_ev = nullptr;
    // pipelined split engine (capi_amp.cpp Cw2Pipe): the second half-batch's stream and the fork / join / lag /
    // poll events, created at the first pipelined decode and destroyed with the plan
    hipStream_t pipe_stream = nullptr;
    hipEvent_t pipe_ev[4] = {nullptr, nullptr, nullptr, nullptr};
    // CU count the engine choice of a decode assumes (0: the device's; sg_amp_plan_set_cus, tests of the
    // full-batch paths at small B)
    int cus_assumed = 0;
    int last_piped = 0;  // the last decode ran iterations as two half-batches on two streams (sg_amp_last_pipelined)
    void *ws_s = nullptr, *ws_tu = nullptr, *ws_xn = nullptr, *ws_part = nullptr, *ws_stM = nullptr,
         *ws_stI = nullptr;
    double *ws_tau_prev = nullptr;
    // per-codeword engine (amp_cw.hip; build_cw), built beside the regular tables when eligible
    bool cw = false;
    int cwKT = 0;
    // A per-codeword plan uses P = 8192 for both engines; batches below one
    // wave of the CUs decode on this companion plan instead: the staged
    // engine at P = 16384 (17-21 % faster there, profiles/README.md)
    bool no_cw = false;
    sg_amp_plan *alt = nullptr;
    uint32_t *c_kt = nullptr;
    uint16_t *c_cmask = nullptr;  // [Q + 1][1024] written image values per thread
    int32_t *c_oa = nullptr, *c_ob = nullptr, *c_gi = nullptr;
    void *c_gc = nullptr, *c_stw = nullptr;
    // split per-codeword engine (amp_cw2.hip; build_cw2): outputs per thread (0 = not built) and its tables
    int cw2OT = 0;
    int c2_np = 2;                // f32 split engine: workgroups per codeword for the next launches (decode_regular)
    uint32_t *c2_ka = nullptr, *c2_kat = nullptr, *c2_cmask = nullptr, *c2_cls = nullptr, *c2_clsp = nullptr,
             *c2_clss = nullptr;
    int32_t *c2_oi = nullptr;
    void *c2_cf = nullptr;
    float *c2_gm = nullptr;  // [OT][512][2] (|al|, |be|) of the polar row form (build_cw2)
    float *c2_gmt = nullptr; // [512][OTP][2] the same, thread-major
    int c2_shoff = 0;        // log2(N / 2): unit of the slot's phase offset
    // its double-precision form (amp_cw2d.hip): coefficients, the slots' w_N2^a, the P-point twiddles
    double *c2d_cf = nullptr, *c2d_gf = nullptr, *c2d_sa = nullptr, *c2d_twp = nullptr;
    void *ws_c2xp = nullptr, *ws_c2vz = nullptr, *ws_c2part = nullptr, *ws_c2ys = nullptr, *ws_c2zs = nullptr;
    void *ws_c2beta = nullptr, *ws_c2sec = nullptr;  // f64 form: beta in class order, per-section sums
    // block engine (several transforms per column block, amp_block.hip; build_block)
    bool block = false;
    bool block2 = false;         // two-class block engine (amp_block2.hip; build_block2): w = 2^16, or w = 2^15 in
    int b2_log2p = 0;            // two classes of 2^13 points (two workgroups per CU); class size P = 2^b2_log2p
    int32_t *b_gk = nullptr;
    uint16_t *b_gloc = nullptr;
    uint32_t *b_pos2 = nullptr, *b_oab = nullptr;
    int32_t *b_gptr = nullptr, *b_gi = nullptr, *b_grow = nullptr;
    int b_ngs = 0;
    void *ws_gbuf = nullptr;  // [B][b_ngs] G slots (block engine)
    void *b_oc = nullptr, *b_gc = nullptr, *b_stw = nullptr;
    // integrated AMP <-> BP decoders (integ_loop.hpp, integrated_dct.hip): their workspace, with the xhat slot
    sg::IntegWs wi;
    // The operator-loop decoder (amp_oploop.hip: AMP with known sections and real K = 2 modulated AMP), grow-only
    // per (plan, B) like the integrated buffers (partial_ensure_ws): u = Az(z / phi) [B][LM]; r = Ab(beta) and z
    // [B][n]; partial sums of z^2 per row block [B][oploop_zz_count(Lr, Mr)]; per-section sum beta^2 and squared
    // error [B][L]; tau [B][Lc]; the loop's own active flags [B] (the general engine's operators want ws_active all
    // ones) and the known indices of the host variant [B][L].  beta, z / phi and the per-codeword scalars (phi in
    // ws_phi_prev) live in the batch workspace.
    sg::DevPool wp;
    int cap_Bp = 0;
    void *wp_u = nullptr, *wp_r = nullptr, *wp_z = nullptr;
    double *wp_zz = nullptr, *wp_bsq = nullptr, *wp_err = nullptr, *wp_tau = nullptr;
    int32_t *wp_active = nullptr, *wp_known = nullptr;
    // Soft output of the K = 2 decoder (sg_amp_bpsk_soft_output, amp_bpsk_llr.hip): while on, partial_ensure_ws also
    // holds wp_skeep [B][LM] of the plan precision, where bpsk_section_kernel keeps s = beta + tau u.
    // last_bpsk_B: batch size of the last K = 2 decode through this plan that filled it and whose s / wp_tau are
    // still there (sg_amp_bpsk_llr_device); 0: none.  Whatever runs in the batch workspace or this pool clears it.
    bool bpsk_soft = false;
    void *wp_skeep = nullptr;
    int last_bpsk_B = 0;
};

#pragma GCC visibility push(hidden)  // shared between the library's objects, not exported from it
namespace sg {
// ---- coefficient math and uploads (amp_plan.cpp)
cd expi(double a);
cd tw(long long k, long long m);  // exp(-2 pi i k / m) with exact integer reduction of k mod m
void fwd_coef(long long k, long long N, long long N2, double sc, long long *a, long long *b, cd *c1, cd *c2);
inline long long slot_of_pos(long long pos, long long N) {  // w-space slot of DCT position pos
    return (pos % 2 == 0) ? pos / 2 : N - 1 - (pos - 1) / 2;
}

// Inverse input: a value v at DCT position q (sparc.py:694-699) contributes
// coef * v to the packed spectrum G at one or two N/2-indices:
// G[k] = A_k y[k] - i A_k y[N-k] + C_k y[N2+k] - i C_k y[N2-k].
template <typename F>
void inv_contrib(long long q, long long N, long long N2, double sc, F &&add) {
    const cd I(0, 1);
    auto Ak = [&](long long k) { return expi(M_PI * (double)k / (2.0 * N)) * (1.0 + I * tw(-k, N)); };
    auto Ck = [&](long long k) { return expi(M_PI * (double)(k + N2) / (2.0 * N)) * (1.0 - I * tw(-k, N)); };
    const double gsc = sc / std::sqrt(2.0);  // sqrt(2 W/L) * (1/2)
    if (q < N2) {
        add(q, Ak(q) * gsc);
        add(N2 - q, -I * Ck(N2 - q) * gsc);
    } else if (q > N2) {
        add(N - q, -I * Ak(N - q) * gsc);
        add(q - N2, Ck(q - N2) * gsc);
    } else {
        add(0, Ck(0) * (1.0 - I) * gsc);
    }
}

int upload_cx(sg_amp_plan *p, void **dst, const std::vector<cd> &src);  // as cx<T> of the plan's precision

// Per-stage twiddles of the 2^log2n-point FFT at ept elements per thread, in thread order (fft.hpp fft1_plan,
// tw_per_k / tw_exp layout)
std::vector<cd> stage_twiddles(int log2n, int ept);
// One order of a transform: every entry in [1, w), no position twice (name: "order0" / "order1")
int check_order(const char *name, const uint32_t *order, int count, long long N);
// The G slots of one transform in ascending k: the N/2-indices that the inverse inputs of outputs o0[0 .. Mr)
// reach (inv_contrib), each with its at most four (output, coefficient) pairs padded with (-1, 0)
struct GSlot { int k; int32_t i[4]; cd c[4]; };
int gather_gslots(const uint32_t *o0, int Mr, long long N, long long N2, double sc, std::vector<GSlot> *out);
int diag_skip();  // SG_AMP_SKIP phase ablation (diagnostic builds only; else 0)

// ---- table builders of the engines
int build_regular(sg_amp_plan *p, const uint32_t *order0, const uint32_t *order1, const std::vector<double> &t_scale);
int build_cw(sg_amp_plan *p, const std::vector<int32_t> &row_k1, const std::vector<int32_t> &kptr,
             const std::vector<int32_t> &kk2, const std::vector<int32_t> &oa, const std::vector<int32_t> &ob,
             const std::vector<int32_t> &gi, const std::vector<cd> &gc, const std::vector<int32_t> &cls_ptr,
             const std::vector<uint32_t> &cls_ls);
int build_cw2(sg_amp_plan *p, const uint32_t *o0, double sc, const std::vector<int32_t> &row_k1,
              const std::vector<int32_t> &cls_ptr, const std::vector<uint32_t> &cls_ls);
int build_block(sg_amp_plan *p, const uint32_t *order0, const uint32_t *order1, const std::vector<double> &t_scale,
                const std::vector<int32_t> &row_of);
int build_block2(sg_amp_plan *p, const uint32_t *order0, const uint32_t *order1, const std::vector<double> &t_scale,
                 const std::vector<int32_t> &row_of);

// ---- workspace, grow-only (amp_plan.cpp)
int ensure_ws(sg_amp_plan *p, int B, int t_max);
int ensure_io(sg_amp_plan *p, size_t bytes);
int partial_ensure_ws(sg_amp_plan *p, int B);

// ---- kernel-facing views of a plan and its workspace (T: float, double), each beside its engine's builder
template <typename T> AmpTables<T> tables(const sg_amp_plan *p);
template <typename T> AmpBufs<T> bufs(const sg_amp_plan *p, int B, const void *y);
template <typename T> RegTables<T> rtables(const sg_amp_plan *p);
template <typename T> RegBufs<T> rbufs(const sg_amp_plan *p, int B, const void *y);
CwTables ctables(const sg_amp_plan *p, int B);
Cw2Tables c2tables(const sg_amp_plan *p, int B);
Cw2dTables c2dtables(const sg_amp_plan *p);
BlkTables btables(const sg_amp_plan *p);

}  // namespace sg

#pragma GCC visibility pop
