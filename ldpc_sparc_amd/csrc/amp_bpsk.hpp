// Real K = 2 (BPSK) modulated AMP (sg_amp_decode_bpsk, capi_amp.cpp): the launch interface of amp_bpsk.hip.
#pragma once
#include <algorithm>

#include "amp_partial.hpp"

namespace sg {

// The state of one K = 2 decode, device pointers (T: the plan precision).  Vectors in natural order.  W of ndim 0
// and 1 is one row block (Lr = 1, Mr = n).
template <typename T>
struct BpskBufs {
    int B, L, M, LM, n, Lr, Lc, Mr, ndim, t_max;
    int np;                    // partial sums of z^2 per row block: part_count(Mr), the same at every B
    const T *y;                // [B][n]
    T *beta;                   // [B][LM]
    T *u;                      // [B][LM] Az(z / phi)
    T *r;                      // [B][n]  Ab(beta)
    T *z, *zs;                 // [B][n]  residual, z / phi of the element's row block
    const int32_t *true_word;  // [B][L] (location << 1) | symbol, or null
    double *zz;                // [B][Lr][np] partial sums of z^2
    double *bsq, *err;         // [B][L] per section: sum beta^2, sum (beta - beta0)^2
    int32_t *map;              // [B][L] the word of the first maximum of |s| and its sign
    double *psi, *psi_prev;    // [B][Lc]
    double *gamma, *bco, *phi;  // [B][Lr]
    double *tau;               // [B][Lc]
    double *nmse;              // [B][t_max][Lc]
    int32_t *active, *t_final;  // [B]
    const double *W;           // [1] (ndim 0), [Lc] or [Lr][Lc]
    double awgn_var, rtol, atol;
    int phi_method;
};

// doubles of BpskBufs::zz per codeword; PART_MAX covers one row block
inline size_t bpsk_zz_count(int Lr, int Mr) { return std::max<size_t>(PART_MAX, (size_t)Lr * part_count(Mr)); }

// nmse = 1, psi = 1, gamma0, b = 0, active = 1, t_final = 0
template <typename T>
int bpsk_launch_init(const BpskBufs<T> &bb, hipStream_t s);
// z = y - r + b z (t = 0: y - r) with b of the element's row block, and the partial sums of z^2
template <typename T>
int bpsk_launch_residual(const BpskBufs<T> &bb, int t, hipStream_t s);
// phase 0 (after the residual): phi, tau, zs = z / phi; phase 1 (after the sections): psi, the NMSE row, the stop
// decision, and gamma and b of the next iteration
template <typename T>
int bpsk_launch_control(const BpskBufs<T> &bb, int phase, int t, hipStream_t s);
// s = beta + tau u, beta = the K = 2 denoiser of s / tau, section sums, the word of the MAP decision; M a power of
// two <= 2048
template <typename T>
int bpsk_launch_section(const BpskBufs<T> &bb, hipStream_t s);

}  // namespace sg
