// Declarations shared by the complex AMP engine's kernels (amp_cfft.hip) and
// its host plan / C ABI (capi_camp.cpp): complex SPARCs with the sub-sampled
// FFT design (sparc.py:593-646) and K-PSK modulated message vectors, double
// precision only.
#pragma once
#include "amp.hpp"

namespace sg {

typedef cx<double> cxd;

constexpr int CAMP_MAX_K = 64;     // largest PSK constellation
constexpr int CAMP_EPT = 8;        // FFT elements per thread of every pass
constexpr int CAMP_MIN_LOG2W = 4;  // w = 16 ... 2^20
constexpr int CAMP_MAX_LOG2W = 20;
constexpr int CAMP_SQUARE_MAX_LOG2W = 16;  // up to here w = P Q with P = 2^floor(lg / 2); above, P = 256
constexpr int CAMP_LONG_TILE = 4096;       // values per pass-B workgroup of the long-row shape (512 threads, 64 KB)

// Design tables of one complex design, device pointers.  A "transform" is one
// nonzero block (r, c) of the base matrix W: a w-point complex FFT, w = P Q,
// with its own orders.  Bin k = k1 + P k2 of a transform's output sits at
// position k1 Q + k2 of the pass-B layout.  Up to w = 2^16 the split is the
// square one, P = 2^floor(log2 w / 2), and both passes run 2048 values in at
// most 256 threads.  For w = 2^17 ... 2^20 the split is asymmetric: P = 256,
// so pass A keeps its shape (CT = 8 columns), and Q = w / 256 = 512 ... 4096;
// pass B then runs tiles of CAMP_LONG_TILE values (RT = 4096 / Q whole rows,
// contiguous in buf0) in 512 threads.
struct CampTables {
    int nT, w, P, Q, log2P, log2Q;
    int CT, RT;  // pass A: columns m2 per workgroup; pass B: rows k1 per workgroup
    int L, M, LM, n, Lr, Lc, Mr, Mc, ndim;
    const int32_t *t_row, *t_col;    // [nT]
    const double *t_scale;           // [nT] sqrt(W_rc / L)
    const int32_t *col_ptr, *col_t;  // CSR: transforms of each column block, row-major order
    const int32_t *row_ptr, *row_t;  // CSR: transforms of each row block, row-major order
    const int32_t *in1;              // [nT][w] input index m -> local column index (order1 inverted), or -1
    const int32_t *in0;              // [nT][w] input index m -> local row index (order0 inverted), or -1
    const int32_t *pos0;             // [nT][Mr] pass-B position of bin order0[i]
    const int32_t *pos1;             // [nT][Mc] pass-B position of bin order1[j]
    const cxd *twP, *twQ, *twW;      // exp(-2 pi i e / len), e < len, len = P, Q, w
};

// Per-batch device buffers.
struct CampBufs {
    int B;
    int K;               // 1: unmodulated; else the K-PSK constellation size
    const cxd *constel;  // [K] (unused for K = 1)
    cxd *beta;           // [B][LM]
    const cxd *y;        // [B][n]
    cxd *z;              // [B][n]
    cxd *buf0;           // [B][nT][w] pass A output T[k1][m2]
    cxd *buf1;           // [B][nT][w] pass B output X[k1][k2]
    double *phi;         // [B][Lr]
    double *tau;         // [B][Lc]
    int32_t *active;     // [B]
    double *sec_sumsq;   // [B][L] sum |beta|^2 per section
    double *sec_err;     // [B][L] sum |beta - beta0|^2 per section
    int32_t *sec_idx;    // [B][L] MAP location of s per section
    int32_t *sec_sym;    // [B][L] MAP constellation index of s per section
    const int32_t *true_idx, *true_sym;  // [B][L] or null
    cxd *s_keep;         // [B][LM] natural order: eta also stores s = beta + tau u here (soft output), or null
    // Known sections (sg_camp_decode_partial*), or null: nothing given.  known_idx [B][L]: a location in [0, M),
    // anything else: a section to decode; known_sym [B][L]: its constellation index, taken modulo K (null for K = 1).
    // Given, the control kernel's initialisation writes their one-hots as beta0 with psi0 and gamma0, its phase 0 of
    // iteration 0 starts from z0 = y - A beta0 (buf1: the forward transforms of beta0), and eta keeps them as they are.
    const int32_t *known_idx, *known_sym;
};

int camp_prepare_fft(const CampTables &tb);  // once per plan: geometry check, LDS limit of the long-row pass B
int camp_launch_fft(const CampTables &tb, const CampBufs &bf, bool inverse, hipStream_t s);  // beta (or z/phi) -> buf1
int camp_launch_eta(const CampTables &tb, const CampBufs &bf, hipStream_t s);
int camp_launch_control(const CampTables &tb, const CampBufs &bf, const AmpScalars &sc, const AmpParams &pr, int phase,
                        int t, hipStream_t s);
int camp_launch_rowsum(const CampTables &tb, const CampBufs &bf, cxd *out, hipStream_t s);     // buf1 -> A x [B][n]
int camp_launch_colgather(const CampTables &tb, const CampBufs &bf, cxd *out, hipStream_t s);  // buf1 -> A^H y [B][LM]
// stand-alone section estimators on device arrays of L sections
int camp_launch_mmse(const cxd *x, int L, int M, int K, const cxd *constel, cxd *out, hipStream_t s);
int camp_launch_map(const cxd *sv, int L, int M, int K, const cxd *constel, int32_t *idx, int32_t *sym, hipStream_t s);
// campaign kernels (camp_campaign.hip): bits [B][L (logM + logK)] -> idx / sym [B][L] (sym may be null);
// one-hot K-PSK beta0 into bf.beta (and bf.active = 1); error counters (sg_camp_count_errors_device)
int camp_launch_bits_to_psk(const uint8_t *bits, int B, int L, int logM, int logK, int32_t *idx, int32_t *sym,
                            hipStream_t s);
int camp_launch_scatter(const CampTables &tb, const CampBufs &bf, const int32_t *idx, const int32_t *sym,
                        hipStream_t s);
int camp_launch_count(const int32_t *map_idx, const int32_t *map_sym, const int32_t *true_idx, const int32_t *true_sym,
                      const int32_t *t_final, int B, int L, int logM, int logK, int64_t *counts, int32_t *rows,
                      hipStream_t s);
// soft output (camp_llr.hip): bit probabilities / LLRs [B][llr_ld] of sections [l0, l0 + nl) from s [B][L M] and
// tau [B][Lc] (null: s is x = s / tau already); M > 2048 is SG_ERR_UNSUPPORTED
int camp_launch_llr(const cxd *s, const double *tau, int B, int L, int Lc, int M, int K, const cxd *constel, int l0,
                    int nl, int llr_ld, int probs_only, double *llr, hipStream_t st);
// camp_launch_bits_to_psk with row strides; word = idx << logK | bin2gray(sym) over [B][L] (sym may be null)
int camp_launch_bits_to_psk_strided(const uint8_t *bits, size_t bit_stride, int B, int L, int logM, int logK,
                                    int32_t *idx, int32_t *sym, size_t idx_stride, hipStream_t s);
int camp_launch_pack(const int32_t *idx, const int32_t *sym, int B, int L, int logK, int32_t *word, hipStream_t s);
// the inverse of camp_launch_pack: word < 0 -> idx = -1, sym = 0; else idx = word >> logK, sym = gray2bin of the low
// logK bits (sym may be null)
int camp_launch_unpack(const int32_t *word, int B, int L, int logK, int32_t *idx, int32_t *sym, hipStream_t s);

}  // namespace sg
