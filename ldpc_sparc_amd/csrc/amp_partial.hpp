// AMP with known sections (sg_amp_decode_partial, capi_amp.cpp) and the BP -> known-sections glue of the
// three-stage concatenated decoder: the launch interface of amp_partial.hip.
#pragma once
#include <algorithm>

#include "common.hpp"

namespace sg {

constexpr int PART_MAX = 32;  // most partial sums of z^2 per codeword

// The state of one partial decode, device pointers (T: the plan precision).  Vectors in natural order.
template <typename T>
struct PartBufs {
    int B, L, M, LM, n, Lc, ndim, t_max;
    int np;                   // partial sums of z^2 per codeword: part_count(n), the same at every B
    const T *y;               // [B][n]
    T *beta;                  // [B][LM]
    T *u;                     // [B][LM] Az(z / phi)
    T *r;                     // [B][n]  Ab(beta)
    T *z, *zs;                // [B][n]  residual, z / phi
    const int32_t *known;     // [B][L] index in [0, M), anything else: unknown
    const int32_t *true_idx;  // [B][L] or null
    double *zz;               // [B][np] partial sums of z^2
    double *bsq, *err;        // [B][L] per section: sum beta^2, sum (beta - beta0)^2
    int32_t *map;             // [B][L] first-maximum argmax of s, or the known index
    double *psi, *psi_prev;   // [B][Lc]
    double *gamma, *bco, *phi;  // [B]
    double *tau;              // [B][Lc]
    double *nmse;             // [B][t_max][Lc]
    int32_t *active, *t_final;  // [B]
    const double *W;          // [1] (ndim 0) or [Lc]
    double awgn_var, rtol, atol;
    int phi_method;
};

inline int part_count(int n) { return std::min(PART_MAX, std::max(1, (n + 1023) / 1024)); }

// beta0 = the known one-hots, psi0 = the share of unknown sections per column block, gamma0, nmse = 1, active
template <typename T>
int part_launch_init(const PartBufs<T> &pb, hipStream_t s);
// z = y - r + b z (t = 0: y - r) and the partial sums of z^2
template <typename T>
int part_launch_residual(const PartBufs<T> &pb, int t, hipStream_t s);
// phase 0 (after the residual): phi, tau, zs = z / phi; phase 1 (after the sections): psi, the NMSE row, the stop
// decision, and gamma and b of the next iteration
template <typename T>
int part_launch_control(const PartBufs<T> &pb, int phase, int t, hipStream_t s);
// s = beta + tau u, beta = softmax(s / tau) or the known one-hot, section sums, argmax; M a power of two <= 2048
template <typename T>
int part_launch_section(const PartBufs<T> &pb, hipStream_t s);

// BP output -> known sections (sg_concat_known_sections_device)
template <typename T>
int part_launch_known(const T *app, const int32_t *it, int max_it, int B, int mults, int N, int L, int L_unp, int logM,
                      int32_t *known, hipStream_t s);

}  // namespace sg
