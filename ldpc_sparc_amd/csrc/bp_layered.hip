// Batched layered (row-serial) belief propagation for QC-LDPC Tanner graphs on gfx950.
//
// The schedule (DESIGN.md "Layered schedule"): layer l is the checks [l S, (l + 1) S), which touch disjoint
// variables (S = z for a quasi-cyclic code).  An iteration takes the layers in ascending order; a check c with
// ports k on variables v_k computes Q_k = app[v_k] - R[c,k], the new check messages R'[c,.] from Q (Lxfb of
// c_ldpc.c:294-314: without correction and times the factor for min-sum, with Lxor's correction for sumprod2),
// and writes app[v_k] = Q_k + R'[c,k], R[c,k] = R'[c,k] at once.  After the last layer the syndrome of the
// hard decisions app < 0 decides whether the codeword stops.
//
// Shape: one workgroup per codeword, of one wave (S <= 64) or two (a lane per check of the layer, the lanes
// taking S > 128 in rounds).  The codeword's app and R stay in LDS for all iterations, beside the graph's
// slot -> variable table (16-bit), the layer offsets and the check degrees; HBM sees the channel LLRs once and
// the final app and iteration index.  Message slot (c = l S + i, k) = loff[l] + k S + i: the lanes of a wave
// read and write consecutive words of R, and for a quasi-cyclic layer consecutive words of app up to the
// circulant's wrap.  One barrier per layer, one (with the stop vote) after the syndrome pass.
//
// Arithmetic order follows the restatement (tests/bp_layered_ref.py) so that min-sum is bit-identical to it
// in both precisions; this file is built with -ffp-contract=off.
#include "bp.hpp"

namespace sg {

// One check of the current layer with its ports in registers (check degrees <= MAXDC).  Rc / evc point at the
// check's port-0 slot; port k is S slots further.
template <typename T, int KIND, int MAXDC>
__device__ __forceinline__ void layer_check_reg(T *__restrict__ app, T *__restrict__ Rc,
                                                const uint16_t *__restrict__ evc, int S, int d, T factor) {
    int v[MAXDC];
    T Q[MAXDC];
#pragma unroll
    for (int k = 0; k < MAXDC; ++k)
        if (k < d) v[k] = evc[k * S];
#pragma unroll
    for (int k = 0; k < MAXDC; ++k)
        if (k < d) Q[k] = app[v[k]] - Rc[k * S];
    if (KIND == SG_MINSUM) {
        // Lxfb(.., corr = 0) in its min / sign-parity form (bp.hip check_update_from): exact, so bit-identical
        // to the forward/backward trellis
        T m1 = T(INFINITY), m2 = T(INFINITY);
        int i1 = -1;
        unsigned sgn = 0u, sall = 0u;
#pragma unroll
        for (int k = 0; k < MAXDC; ++k) {
            if (k < d) {
                const T a = fabs(Q[k]);
                const unsigned s = signbit(Q[k]) ? 1u : 0u;
                sgn |= s << k;
                sall ^= s;
                if (a < m1) { m2 = m1; m1 = a; i1 = k; }
                else if (a < m2) { m2 = a; }
            }
        }
#pragma unroll
        for (int k = 0; k < MAXDC; ++k) {
            if (k < d) {
                const T mag = (k == i1) ? m2 : m1;
                const bool neg = (sall ^ ((sgn >> k) & 1u)) != 0u;
                const T out = (neg ? -mag : mag) * factor;
                Rc[k * S] = out;
                app[v[k]] = Q[k] + out;
            }
        }
    } else {  // SG_SUMPROD2
        T f[MAXDC], b[MAXDC];
        f[0] = Q[0];
#pragma unroll
        for (int k = 1; k < MAXDC; ++k)
            if (k < d) f[k] = lxor<T, true>(f[k - 1], Q[k]);
#pragma unroll
        for (int p = MAXDC - 1; p >= 0; --p) {
            if (p == d - 1) b[p] = Q[p];
            else if (p < d - 1) b[p] = lxor<T, true>(b[p + 1 < MAXDC ? p + 1 : p], Q[p]);
        }
#pragma unroll
        for (int k = 0; k < MAXDC; ++k) {
            if (k < d) {
                T out;
                if (k == 0) out = b[MAXDC > 1 ? 1 : 0];
                else if (k == d - 1) out = f[k > 0 ? k - 1 : 0];
                else out = lxor<T, true>(f[k > 0 ? k - 1 : 0], b[k + 1 < MAXDC ? k + 1 : k]);
                Rc[k * S] = out;
                app[v[k]] = Q[k] + out;
            }
        }
    }
}

// The same check with no per-port registers, for any degree: the first pass leaves Q_k in app[v_k] (no other
// check of the layer touches v_k) and, for sumprod2, the backward value b[k+1] in the slot of R[c,k], whose
// old value Q_k has consumed; the second pass writes R' and app.  Same arithmetic, in the same order.
template <typename T, int KIND>
__device__ __forceinline__ void layer_check_lean(T *__restrict__ app, T *__restrict__ Rc,
                                                 const uint16_t *__restrict__ evc, int S, int d, T factor) {
    if (KIND == SG_MINSUM) {
        T m1 = T(INFINITY), m2 = T(INFINITY);
        int i1 = -1;
        unsigned sgn = 0u, sall = 0u;
        for (int k = 0; k < d; ++k) {
            const int v = evc[k * S];
            const T q = app[v] - Rc[k * S];
            app[v] = q;
            const T a = fabs(q);
            const unsigned s = signbit(q) ? 1u : 0u;
            sgn |= s << k;
            sall ^= s;
            if (a < m1) { m2 = m1; m1 = a; i1 = k; }
            else if (a < m2) { m2 = a; }
        }
        for (int k = 0; k < d; ++k) {
            const int v = evc[k * S];
            const T mag = (k == i1) ? m2 : m1;
            const bool neg = (sall ^ ((sgn >> k) & 1u)) != 0u;
            const T out = (neg ? -mag : mag) * factor;
            Rc[k * S] = out;
            app[v] = app[v] + out;
        }
    } else {  // SG_SUMPROD2
        int v = evc[(d - 1) * S];
        T q = app[v] - Rc[(d - 1) * S];
        app[v] = q;
        T b = q;  // b[d-1]
        for (int k = d - 2; k >= 0; --k) {
            v = evc[k * S];
            q = app[v] - Rc[k * S];
            app[v] = q;
            Rc[k * S] = b;  // b[k+1]
            b = lxor<T, true>(b, q);
        }
        v = evc[0];
        T f = app[v];         // f[0] = Q_0
        app[v] = f + Rc[0];   // R'[c,0] = b[1], in its slot already
        for (int k = 1; k < d - 1; ++k) {
            v = evc[k * S];
            q = app[v];
            const T out = lxor<T, true>(f, Rc[k * S]);
            Rc[k * S] = out;
            app[v] = q + out;
            f = lxor<T, true>(f, q);
        }
        v = evc[(d - 1) * S];
        Rc[(d - 1) * S] = f;  // R'[c,d-1] = f[d-2]
        app[v] = app[v] + f;
    }
}

// MAXDC = 0: the register-free check for degrees above 8
template <typename T, int KIND, int MAXDC, int NT>
__global__ __launch_bounds__(NT) void bp_layered_kernel(BpLayArgs<T> a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lay_smem[];
    T *app = reinterpret_cast<T *>(lay_smem);
    T *R = app + a.nv;
    int32_t *loff = reinterpret_cast<int32_t *>(R + a.slots);
    uint16_t *ev = reinterpret_cast<uint16_t *>(loff + a.nlayers);
    uint8_t *cd = reinterpret_cast<uint8_t *>(ev + a.slots);
    const int tid = threadIdx.x, cw = blockIdx.x, S = a.S;
    const T *ch = a.ch + (size_t)cw * a.nv;
    for (int i = tid; i < a.nlayers; i += NT) loff[i] = a.loff[i];
    for (int i = tid; i < a.slots; i += NT) { ev[i] = a.evar[i]; R[i] = T(0); }
    for (int i = tid; i < a.nc; i += NT) cd[i] = a.cdeg[i];
    for (int i = tid; i < a.nv; i += NT) app[i] = ch[i];
    __syncthreads();
    int it = 0;
    for (; it < a.max_it; ++it) {
        for (int l = 0; l < a.nlayers; ++l) {
            const int base = loff[l];
            for (int i = tid; i < S; i += NT) {
                const int d = cd[l * S + i];
                if constexpr (MAXDC > 0)
                    layer_check_reg<T, KIND, MAXDC>(app, R + base + i, ev + base + i, S, d, a.factor);
                else
                    layer_check_lean<T, KIND>(app, R + base + i, ev + base + i, S, d, a.factor);
            }
            __syncthreads();
        }
        // syndrome of the hard decisions over all checks
        int unsat = 0;
        for (int l = 0; l < a.nlayers; ++l) {
            const int base = loff[l];
            for (int i = tid; i < S; i += NT) {
                const int d = cd[l * S + i];
                int par = 0;
                for (int k = 0; k < d; ++k) par ^= app[ev[base + k * S + i]] < T(0) ? 1 : 0;
                unsat |= par;
            }
        }
        if (!__syncthreads_or(unsat)) break;
    }
    T *out = a.app + (size_t)cw * a.nv;
    for (int i = tid; i < a.nv; i += NT) out[i] = app[i];
    if (tid == 0) a.it[cw] = it;
}

template <typename T, int KIND, int MAXDC, int NT>
static int launch_one(const BpLayArgs<T> &a, size_t lds, hipStream_t s) {
    auto kern = bp_layered_kernel<T, KIND, MAXDC, NT>;
    static size_t lds_set = 64 * 1024;
    SG_TRY(set_max_lds((const void *)kern, lds, &lds_set));
    ProfScope ps(SG_PH_BP, s);
    hipLaunchKernelGGL(kern, dim3(a.B), dim3(NT), lds, s, a);
    SG_HIP(hipGetLastError());
    return SG_OK;
}

template <typename T, int KIND>
static int dispatch(const BpLayArgs<T> &a, size_t lds, hipStream_t s) {
    const bool one_wave = bp_layered_threads(a.S) == 64;
    if (a.max_cdeg <= 8)
        return one_wave ? launch_one<T, KIND, 8, 64>(a, lds, s) : launch_one<T, KIND, 8, 128>(a, lds, s);
    return one_wave ? launch_one<T, KIND, 0, 64>(a, lds, s) : launch_one<T, KIND, 0, 128>(a, lds, s);
}

template <typename T>
int bp_layered_launch(const BpLayArgs<T> &a, int dectype, hipStream_t s) {
    if (dectype != SG_MINSUM && dectype != SG_SUMPROD2)
        return fail(SG_ERR_UNSUPPORTED, "the layered schedule decodes minsum and sumprod2 only (dectype=%d)", dectype);
    if (a.max_cdeg > LAY_MAXDC)
        return fail(SG_ERR_UNSUPPORTED, "check degree %d exceeds the supported maximum of %d", a.max_cdeg, LAY_MAXDC);
    if (a.nv > 65536)
        return fail(SG_ERR_UNSUPPORTED, "graph with %d variables exceeds the layered decoder's 16-bit LDS table", a.nv);
    const size_t lds = bp_layered_lds_bytes<T>(a.nv, a.nc, a.slots, a.nlayers);
    if (lds + LAY_STATIC_LDS > (size_t)BP_MAX_LDS)
        return fail(SG_ERR_UNSUPPORTED,
                    "graph needs %zu B of LDS per codeword (> %d B): too large for the LDS-resident layered decoder",
                    lds + LAY_STATIC_LDS, BP_MAX_LDS);
    if (a.B <= 0) return SG_OK;
    return dectype == SG_MINSUM ? dispatch<T, SG_MINSUM>(a, lds, s) : dispatch<T, SG_SUMPROD2>(a, lds, s);
}

template int bp_layered_launch<float>(const BpLayArgs<float> &, int, hipStream_t);
template int bp_layered_launch<double>(const BpLayArgs<double> &, int, hipStream_t);

}  // namespace sg
