// State evolution of SPARC AMP (sparc_public/sparc_se.py:82-183) on gfx950:
// the Monte-Carlo expectation sparc_se_E (:82-115) over resident Gaussian
// samples u [mc][M], for many tau values at once (one per column block of
// the base matrix).  The tau / psi recursion itself is scalar host work.
//
//   K = 1:  E = mean_s  e^(1/tau + u_s0/sqrt(tau)) / (e^(1/tau + u_s0/sqrt(tau)) + sum_{j>0} e^(u_sj/sqrt(tau)))
//   K = 2:  sinh / cosh in place of exp (real modulated SPARCs, :91-94)
// Complex K-PSK SPARCs (complex samples u = randn + 1j randn, :154-155):
//   K = 4:  E = mean_s  sinh(x0) / (cosh(x0) + cosh(Im u_s0/sqrt(tau))
//                + sum_{j>0} cosh(Re u_sj/sqrt(tau)) + cosh(Im u_sj/sqrt(tau))),
//           x0 = 1/tau + Re u_s0/sqrt(tau)  (:95-98)
//   K >= 8: with g_0k = Re((1/tau + u_s0/sqrt(tau)) conj c_k) and
//           g_jk = Re(u_sj/sqrt(tau) conj c_k) over the constellation c,
//           E = mean_s  sum_k Re(c_k) e^(g_0k) / sum_{j>=0} sum_k e^(g_jk)
//           (:99-113; the reference's means over k cancel), every exponent
//           shifted by the sample's largest one so that no exp overflows.
//
// One wavefront per sample (lanes stride the M entries); per-block partial
// sums, then a fixed-order sum, so E is deterministic.
#include <algorithm>
#include <cmath>
#include <vector>

#include "device_mem.hpp"

constexpr int SE_MAX_K = 64;  // largest PSK constellation, as the complex AMP engine

struct sg_se_samples {
    int mc = 0, M = 0;
    bool cplx = false;       // u holds interleaved complex samples
    sg::DevMem u;            // doubles [mc][M], or [mc][M][2]
    sg::DevMem constel;      // doubles [SE_MAX_K][2]: K-PSK constellation of the last K >= 8 call
    sg::DevPool ws;          // part, taus, E: grow together with nt_cap
    double *part = nullptr;  // [nt_cap][nblk]
    int nt_cap = 0;
    double *taus = nullptr, *E = nullptr;
};

namespace sg {

namespace {

constexpr int SE_WAVES = 4;  // samples per 256-thread block

__global__ __launch_bounds__(256) void se_E_kernel(const double *__restrict__ u, int mc, int M, int K,
                                                   const double *taus, double *part, int nblk) {
    __shared__ double red[SE_WAVES];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int s = blockIdx.x * SE_WAVES + wid, t = blockIdx.y;
    const double itau = 1.0 / taus[t], rtau = sqrt(itau);
    double e = 0.0;
    if (s < mc) {
        const double *row = u + (size_t)s * M;
        double c = 0.0;
        for (int j = 1 + lane; j < M; j += 64) c += K == 1 ? exp(rtau * row[j]) : cosh(rtau * row[j]);
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
        const double a = K == 1 ? exp(itau + rtau * row[0]) : sinh(itau + rtau * row[0]);
        e = a / (a + c);  // expsB = expsA for K = 1, 2 (:88-94)
    }
    if (lane == 0) red[wid] = e;
    __syncthreads();
    if (threadIdx.x == 0) {
        double v = 0.0;
        for (int w = 0; w < SE_WAVES; ++w) v += red[w];
        part[(size_t)t * nblk + blockIdx.x] = v;
    }
}

// complex samples, K = 4 .. SE_MAX_K; c [K] is the constellation for K >= 8
__global__ __launch_bounds__(256) void se_E_cplx_kernel(const double2 *__restrict__ u, int mc, int M, int K,
                                                        const double2 *__restrict__ c, const double *taus, double *part,
                                                        int nblk) {
    __shared__ double red[SE_WAVES];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int s = blockIdx.x * SE_WAVES + wid, t = blockIdx.y;
    const double itau = 1.0 / taus[t], rtau = sqrt(itau);
    double e = 0.0;
    if (s < mc) {
        const double2 *row = u + (size_t)s * M;
        const double x0 = itau + rtau * row[0].x, y0 = rtau * row[0].y;
        if (K == 4) {
            double cs = 0.0;
            for (int j = 1 + lane; j < M; j += 64) cs += cosh(rtau * row[j].x) + cosh(rtau * row[j].y);
            for (int o = 32; o > 0; o >>= 1) cs += __shfl_xor(cs, o, 64);
            e = sinh(x0) / ((cosh(x0) + cosh(y0)) + cs);
        } else {
            double m = -INFINITY;
            for (int k = 0; k < K; ++k) m = fmax(m, x0 * c[k].x + y0 * c[k].y);
            for (int j = 1 + lane; j < M; j += 64) {
                const double xj = rtau * row[j].x, yj = rtau * row[j].y;
                for (int k = 0; k < K; ++k) m = fmax(m, xj * c[k].x + yj * c[k].y);
            }
            for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
            double cs = 0.0;
            for (int j = 1 + lane; j < M; j += 64) {
                const double xj = rtau * row[j].x, yj = rtau * row[j].y;
                for (int k = 0; k < K; ++k) cs += exp(xj * c[k].x + yj * c[k].y - m);
            }
            for (int o = 32; o > 0; o >>= 1) cs += __shfl_xor(cs, o, 64);
            double a = 0.0, b = 0.0;
            for (int k = 0; k < K; ++k) {
                const double w = exp(x0 * c[k].x + y0 * c[k].y - m);
                a += c[k].x * w;
                b += w;
            }
            e = a / (b + cs);
        }
    }
    if (lane == 0) red[wid] = e;
    __syncthreads();
    if (threadIdx.x == 0) {
        double v = 0.0;
        for (int w = 0; w < SE_WAVES; ++w) v += red[w];
        part[(size_t)t * nblk + blockIdx.x] = v;
    }
}

__global__ void se_finish_kernel(const double *part, int nblk, int mc, double *E) {
    __shared__ double red[4];
    const int t = blockIdx.x;
    double v = 0.0;
    for (int b = threadIdx.x; b < nblk; b += blockDim.x) v += part[(size_t)t * nblk + b];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) E[t] = (red[0] + red[1] + red[2] + red[3]) / mc;
}

}  // namespace

}  // namespace sg

using namespace sg;

extern "C" {

static int se_samples_create(const double *u, int mc, int M, bool cplx, sg_se_samples **out) {
    SG_CHECK_ARG(u && out && mc > 0 && M > 1, "bad argument");
    SG_TRY(ensure_device());
    sg_se_samples *h = new sg_se_samples();
    h->mc = mc;
    h->M = M;
    h->cplx = cplx;
    const size_t bytes = (size_t)mc * M * (cplx ? 16 : 8);
    if (h->u.ensure(bytes) != SG_OK) {
        delete h;
        return fail(SG_ERR_NOMEM, "cannot allocate %zu bytes of samples", bytes);
    }
    if (hipMemcpy(h->u.at(), u, bytes, hipMemcpyHostToDevice) != hipSuccess) {
        delete h;
        return fail(SG_ERR_HIP, "sample upload failed");
    }
    *out = h;
    return SG_OK;
}

int sg_se_samples_create(const double *u, int mc, int M, sg_se_samples **out) {
    return se_samples_create(u, mc, M, false, out);
}

int sg_se_samples_create_complex(const double *u, int mc, int M, sg_se_samples **out) {
    return se_samples_create(u, mc, M, true, out);
}

int sg_se_samples_destroy(sg_se_samples *h) {
    delete h;
    return SG_OK;
}

int sg_se_expectation(sg_se_samples *h, int K, const double *taus, int nt, double *E) {
    SG_CHECK_ARG(h && taus && E && nt >= 0, "bad argument");
    SG_CHECK_ARG(K >= 1 && (K & (K - 1)) == 0, "K must be 1 or a power of two");
    if (K > SE_MAX_K) return fail(SG_ERR_UNSUPPORTED, "K=%d-PSK: at most %d symbols are supported", K, SE_MAX_K);
    SG_CHECK_ARG(h->cplx == (K >= 4), "K = 1, 2 take real samples, K >= 4 complex samples");
    if (!nt) return SG_OK;
    SG_TRY(ensure_device());
    const int nblk = (h->mc + SE_WAVES - 1) / SE_WAVES;
    if (nt > h->nt_cap) {
        h->ws.release();
        h->nt_cap = 0;
        SG_TRY(h->ws.alloc(&h->part, (size_t)nt * nblk * 8));
        SG_TRY(h->ws.alloc(&h->taus, (size_t)nt * 8));
        SG_TRY(h->ws.alloc(&h->E, (size_t)nt * 8));
        h->nt_cap = nt;
    }
    hipStream_t s = lib_stream();
    SG_HIP(hipMemcpyAsync(h->taus, taus, (size_t)nt * 8, hipMemcpyHostToDevice, s));
    std::vector<double> c;  // psk_constel, sparc.py:225-239 (alive until the synchronize below)
    if (K >= 8) {
        SG_TRY(h->constel.ensure((size_t)SE_MAX_K * 16));
        for (int k = 0; k < K; ++k) {
            const double theta = 2.0 * M_PI * k / K;
            c.push_back(std::cos(theta));
            c.push_back(std::sin(theta));
        }
        SG_HIP(hipMemcpyAsync(h->constel.at(), c.data(), c.size() * 8, hipMemcpyHostToDevice, s));
    }
    if (h->cplx)
        hipLaunchKernelGGL(se_E_cplx_kernel, dim3(nblk, nt), dim3(256), 0, s, h->u.at<const double2>(), h->mc, h->M, K,
                           h->constel.at<const double2>(), h->taus, h->part, nblk);
    else
        hipLaunchKernelGGL(se_E_kernel, dim3(nblk, nt), dim3(256), 0, s, h->u.at<const double>(), h->mc, h->M, K, h->taus, h->part, nblk);
    hipLaunchKernelGGL(se_finish_kernel, dim3(nt), dim3(256), 0, s, h->part, nblk, h->mc, h->E);
    SG_HIP(hipGetLastError());
    SG_HIP(hipMemcpyAsync(E, h->E, (size_t)nt * 8, hipMemcpyDeviceToHost, s));
    SG_HIP(hipStreamSynchronize(s));
    return SG_OK;
}

}  // extern "C"
