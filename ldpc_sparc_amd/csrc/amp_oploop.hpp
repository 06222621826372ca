// The operator-loop AMP decoder (oploop_impl, capi_amp.cpp): sparc_amp on the plan's operators Ab / Az over
// natural-order vectors, for AMP with known sections (sg_amp_decode_partial), real K = 2 modulated AMP
// (sg_amp_decode_bpsk) and K = 2 with known words (sg_amp_decode_bpsk_partial), and the BP -> known-sections glue
// of the three-stage concatenated decoders: the launch interface of amp_oploop.hip.
#pragma once
#include <algorithm>

#include "common.hpp"

namespace sg {

constexpr int PART_MAX = 32;  // most partial sums of z^2 per row block and codeword

// What a section's denoiser and decision are: the only part of the loop that differs between the two families
enum class SectionRule {
    Known,  // softmax, or the one-hot of a known index; sections are indices in [0, M)
    Bpsk,   // the K = 2 denoiser, or the +-1 one-hot of a known word; sections are words (location << 1) | symbol
            // in [0, 2M)
};

inline const char *rule_name(SectionRule rule) { return rule == SectionRule::Bpsk ? "K = 2" : "partial"; }

// The state of one decode, device pointers (T: the plan precision).  Vectors in natural order.  W of ndim 0 and 1
// is one row block (Lr = 1, Mr = n).
template <typename T>
struct OpLoopBufs {
    int B, L, M, LM, n, Lr, Lc, Mr, ndim, t_max;
    int np;                     // partial sums of z^2 per row block: part_count(Mr), the same at every B
    const T *y;                 // [B][n]
    T *beta;                    // [B][LM]
    T *u;                       // [B][LM] Az(z / phi)
    T *s_keep;                  // [B][LM] K = 2 soft output: the section kernel's s = beta + tau u, or null (not kept)
    T *r;                       // [B][n]  Ab(beta)
    T *z, *zs;                  // [B][n]  residual, z / phi of the element's row block
    const int32_t *known;       // [B][L] rule Known: index in [0, M); rule Bpsk: word in [0, 2M); anything else:
                                // unknown; null: nothing is known (rule Bpsk only)
    const int32_t *truth;       // [B][L] the transmitted indices or words, or null
    double *zz;                 // [B][Lr][np] partial sums of z^2
    double *bsq, *err;          // [B][L] per section: sum beta^2, sum (beta - beta0)^2
    int32_t *map;               // [B][L] the section's decision: an index (the known one where given) or a word
    double *psi, *psi_prev;     // [B][Lc]
    double *gamma, *bco, *phi;  // [B][Lr]
    double *tau;                // [B][Lc]
    double *nmse;               // [B][t_max][Lc]
    int32_t *active, *t_final;  // [B]
    const double *W;            // [1] (ndim 0), [Lc] or [Lr][Lc]
    double awgn_var, rtol, atol;
    int phi_method;
};

inline int part_count(int n) { return std::min(PART_MAX, std::max(1, (n + 1023) / 1024)); }
// doubles of OpLoopBufs::zz per codeword; PART_MAX covers one row block
inline size_t oploop_zz_count(int Lr, int Mr) { return std::max<size_t>(PART_MAX, (size_t)Lr * part_count(Mr)); }

// nmse = 1, gamma0, b = 0, active = 1, t_final = 0, and psi0 = 1 or, with known sections, beta0 = their one-hots
// and psi0 = the share of unknown sections per column block.  The rule is a kernel argument (not a field of
// OpLoopBufs): it says whether a known entry is an index (one-hot +1) or a word (+1 / -1 at word >> 1).
template <typename T>
int oploop_launch_init(const OpLoopBufs<T> &ob, SectionRule rule, hipStream_t s);
// z = y - r + b z (t = 0: y - r) with b of the element's row block, and the partial sums of z^2
template <typename T>
int oploop_launch_residual(const OpLoopBufs<T> &ob, int t, hipStream_t s);
// phase 0 (after the residual): phi, tau, zs = z / phi; phase 1 (after the sections): psi, the NMSE row, the stop
// decision, and gamma and b of the next iteration
template <typename T>
int oploop_launch_control(const OpLoopBufs<T> &ob, int phase, int t, hipStream_t s);
// s = beta + tau u, beta = the rule's denoiser of s / tau, section sums, the rule's decision; M a power of two
// <= 2048
template <typename T>
int oploop_launch_section(const OpLoopBufs<T> &ob, SectionRule rule, hipStream_t s);

// Bit LLRs (or with probs_only P(bit = 0)) of sections [l0, l0 + nl) from the s and tau a K = 2 decode with
// OpLoopBufs::s_keep left (amp_bpsk_llr.hip): log2 M location bits, MSB first, then the symbol bit, to
// llr[b llr_ld + (l - l0) (log2 M + 1) + i].  The caller has checked the range, llr_ld and M a power of two in
// [2, 2048].  s_keep [B][L M] natural order, tau [B][Lc].
template <typename T>
int bpsk_launch_llr(const T *s_keep, const double *tau, int B, int L, int M, int Lc, int l0, int nl, int llr_ld,
                    int probs_only, T *llr, hipStream_t s);

// BP output -> known sections (sg_concat_known_sections_device)
template <typename T>
int part_launch_known(const T *app, const int32_t *it, int max_it, int B, int mults, int N, int L, int L_unp, int logM,
                      int32_t *known, hipStream_t s);

}  // namespace sg
