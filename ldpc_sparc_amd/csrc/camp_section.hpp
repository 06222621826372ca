// Device code shared by the complex AMP engine's kernels (amp_cfft.hip), its soft output (camp_llr.hip) and its
// campaign kernels (camp_campaign.hip): the operator's single-bin gathers, the known sections of a decode, the K-PSK
// section estimators, the Gray code of the symbol bits.  All __forceinline__: the kernels compile to the same code
// as with a private copy.
#pragma once
#include "amp_cfft.hpp"

namespace sg {

// known (location, constellation index) of section o = cw L + l, or false: nothing is known without
// CampBufs::known_idx, a location outside [0, M) is unknown, the constellation index is taken modulo K
__device__ __forceinline__ bool known_of(const CampBufs &bf, size_t o, int M, int *k, int *ks) {
    if (!bf.known_idx) return false;
    *k = bf.known_idx[o];
    *ks = bf.K > 1 ? bf.known_sym[o] & (bf.K - 1) : 0;
    return *k >= 0 && *k < M;
}

// (A beta)_i of row block r summed over the row's transforms in table order
__device__ __forceinline__ cxd gather_ab(const CampTables &tb, const CampBufs &bf, int cw, int r, int il) {
    cxd a{0.0, 0.0};
    for (int q = tb.row_ptr[r]; q < tb.row_ptr[r + 1]; ++q) {
        const int t = tb.row_t[q];
        const cxd v = bf.buf1[((size_t)cw * tb.nT + t) * tb.w + tb.pos0[(size_t)t * tb.Mr + il]];
        const double sc = tb.t_scale[t];
        a.x += sc * v.x;
        a.y += sc * v.y;
    }
    return a;
}
// (A^H z/phi)_j of column block c summed over the column's transforms in table order
__device__ __forceinline__ cxd gather_az(const CampTables &tb, const CampBufs &bf, int cw, int c, int jl) {
    cxd a{0.0, 0.0};
    for (int q = tb.col_ptr[c]; q < tb.col_ptr[c + 1]; ++q) {
        const int t = tb.col_t[q];
        const cxd v = bf.buf1[((size_t)cw * tb.nT + t) * tb.w + tb.pos1[(size_t)t * tb.Mc + jl]];
        const double sc = tb.t_scale[t];
        a.x += sc * v.x;
        a.y += sc * v.y;
    }
    return a;
}

// ------------------------------------------------------------------ K-PSK section estimators
// x = s / tau (tau already halved for complex s, sparc.py:417-418).  The
// exponent arguments of entry x are Re x (K = 1), +-Re x (K = 2), +-Re x and
// +-Im x (K = 4), Re(x conj c_k) (K >= 8); psk_shift is their largest.
__device__ __forceinline__ double psk_shift(int K, const cxd *__restrict__ c, cxd x) {
    if (K == 1) return x.x;
    if (K == 2) return fabs(x.x);
    if (K == 4) return fmax(fabs(x.x), fabs(x.y));
    double m = -INFINITY;
    for (int k = 0; k < K; ++k) m = fmax(m, x.x * c[k].x + x.y * c[k].y);
    return m;
}
// numerator of the entry's estimate and its part of the section's denominator
__device__ __forceinline__ void psk_terms(int K, const cxd *__restrict__ c, cxd x, double m, cxd *top, double *den) {
    if (K == 1) {
        const double e = exp(x.x - m);
        *top = cxd{e, 0.0};
        *den = e;
    } else if (K == 2) {
        const double e1 = exp(x.x - m), e2 = exp(-x.x - m);
        *top = cxd{e1 - e2, 0.0};
        *den = e1 + e2;
    } else if (K == 4) {
        const double x1 = exp(x.x - m), x2 = exp(-x.x - m), y1 = exp(x.y - m), y2 = exp(-x.y - m);
        *top = cxd{x1 - x2, y1 - y2};
        *den = (x1 + x2) + (y1 + y2);
    } else {
        cxd a{0.0, 0.0};
        double dn = 0.0;
        for (int k = 0; k < K; ++k) {
            const double e = exp(x.x * c[k].x + x.y * c[k].y - m);
            a.x += e * c[k].x;
            a.y += e * c[k].y;
            dn += e;
        }
        *top = a;
        *den = dn;
    }
}

// MAP decision of a section (sparc.py:485-510): the lane's running best
struct MapBest {
    double v;
    int flat;  // entry e (K < 8) or e K + k (K >= 8, row-major over (entry, symbol))
    cxd s;
};
__device__ __forceinline__ MapBest map_init() { return MapBest{-INFINITY, 0x7fffffff, cxd{0.0, 0.0}}; }
__device__ __forceinline__ void map_update(int K, const cxd *__restrict__ c, cxd s, int e, MapBest &b) {
    if (K < 8) {
        const double v = K == 1 ? s.x : K == 2 ? fabs(s.x) : fmax(fabs(s.x), fabs(s.y));
        if (b.flat == 0x7fffffff || v > b.v) b = MapBest{v, e, s};
    } else {
        for (int k = 0; k < K; ++k) {
            const double v = s.x * c[k].x + s.y * c[k].y;  // Re(conj(s) c_k)
            if (b.flat == 0x7fffffff || v > b.v) b = MapBest{v, e * K + k, s};
        }
    }
}
// the section's first maximum over the wavefront; entry e lives on lane e & 63
__device__ __forceinline__ void map_finish(int K, const MapBest &b, int *idx, int *sym) {
    const double g = wave_max(b.v);
    int cand = (b.flat != 0x7fffffff && b.v == g) ? b.flat : 0x7fffffff;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cand = min(cand, __shfl_xor(cand, o, 64));
    if (cand == 0x7fffffff) cand = 0;
    const int e = K >= 8 ? cand / K : cand;
    const double sx = __shfl(b.s.x, e & 63, 64), sy = __shfl(b.s.y, e & 63, 64);
    int k = 0;
    if (K == 2) k = sx < 0.0 ? 1 : 0;
    else if (K == 4) {
        k = (int)rint(4.0 * atan2(sy, sx) / (2.0 * 3.14159265358979323846));  // sparc.py:496-498
        if (k < 0) k += 4;
        k &= 3;
    } else if (K >= 8) k = cand - e * K;
    *idx = e;
    *sym = k;
}

// ------------------------------------------------------------------ Gray code of the K-PSK symbol bits
__device__ __forceinline__ int gray_to_bin(int g) {  // sparc.py:214-223
    for (int m = g >> 1; m; m >>= 1) g ^= m;
    return g;
}
__device__ __forceinline__ int bin_to_gray(int b) { return b ^ (b >> 1); }  // sparc.py:206-211

}  // namespace sg
