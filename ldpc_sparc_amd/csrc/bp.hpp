// Kernel-side declarations of the batched BP decoder (bp.hip).
#pragma once
#include "common.hpp"

namespace sg {

constexpr int BP_THREADS = 512;
constexpr int BP_VJ = 8;                // variables per thread held in registers (nv <= BP_VJ * BP_THREADS)
constexpr int BP_MAX_LDS = 160 * 1024;  // one workgroup's LDS limit on gfx950

template <typename T>
struct BpArgs {
    const int32_t *voff;       // [nv+1] variable-port offsets
    const int32_t *port_slot;  // [nmsg] variable port -> LDS message slot (k*nc + c)
    const uint8_t *cdeg;       // [nc]
    int nv, nc, slots;         // slots = max_cdeg * nc
    int nports;                // variable ports = edges (voff[nv])
    const T *ch;               // [B][nv]
    T *app;                    // [B][nv]
    int32_t *it;               // [B]
    int B, max_it;
    T factor;
};

template <typename T>
int bp_launch(const BpArgs<T> &a, int dectype, int max_cdeg, hipStream_t s);

// Degree-grouped layout of a Tanner graph (bp.hip "grouped min-sum kernel"):
// variables and checks sorted by degree into groups of 64 (one wavefront
// lane each) of equal degree, so every wave loop is uniform.  Check group g
// of degree dc owns the dc x 64 message block at LDS byte address addr_g
// (slot = addr_g + 256 k + 4 lane); variable group g reads its ports' slot
// byte addresses from the global table at entry tab_g / 2 + 64 k + lane.
// Groups are assigned to the workgroup's 8 waves (at most 8 variable and 4
// check groups per wave).
constexpr int GRP_WAVES = BP_THREADS / 64;
constexpr int GRP_MAXDV = 16;  // variable degrees the unrolled variable groups take
constexpr int GRP_MAXDC = 8;   // check degrees the unrolled check groups take
constexpr int GRP_FLAG_BYTES = 2 * GRP_WAVES * 4;  // LDS stop flags after the messages (the whole image)
constexpr int GRP_PAIR = 1 << 8;  // degree-word flag: this variable group and the next one run as a pair
constexpr int GRP_PAIR_MAXD = 3;  // variable degrees whose groups pair up (the pair's slots and messages stay
                                  // within the <4, 2> kernel's 64 VGPRs)
struct BpGrpArgs {
    const int32_t *meta;      // [5][GRP_WAVES][VJ or CJ]: vdeg, vtab, cdeg, caddr, cvalid (see bp.hip)
    const int32_t *vmap;      // [GRP_WAVES][VJ][64] variable of each lane (-1: dummy)
    const uint16_t *vtab;     // [ntab] LDS slot byte addresses of the variable groups' ports (global)
    int ntab;                 // table entries
    int msg_bytes;            // message image incl. the trash slot (16-byte multiple)
    int vj, cj;               // groups per wave of the layout (<= the kernel's VJ, CJ)
    int nv;
    const float *ch;          // [B][nv]
    float *app;               // [B][nv]
    int32_t *it;              // [B]
    int B, max_it;
    float factor;
};
int bp_grouped_launch(const BpGrpArgs &a, hipStream_t s);
// groups per wave of the kernel instance that takes a layout of vj / cj groups
// per wave (the host lays meta / vmap out with these strides)
inline int grp_kvj(int vj, int cj) { return (vj <= 4 && cj <= 2) ? 4 : 8; }
inline int grp_kcj(int vj, int cj) { return (vj <= 4 && cj <= 2) ? 2 : 4; }
// Layered (row-serial) schedule (bp_layered.hip).  Layer l is the checks [l S, (l + 1) S); no variable occurs
// twice within a layer (capi_ldpc.cpp layer_validate), so a layer's checks run one per lane with no ordering
// among them.  Message slot of check c = l S + i, port k: loff[l] + k S + i (a layer's ports side by side,
// padded to the layer's largest degree); evar[slot] is the variable on that port.
constexpr int LAY_MAXDC = 32;  // check degrees accepted, as bp.hip dispatch_dc
constexpr int LAY_STATIC_LDS = 256;  // the kernel's static LDS (the stop vote), beside the dynamic image
template <typename T>
struct BpLayArgs {
    const uint16_t *evar;  // [slots] variable of each message slot (pad slots: 0, never read)
    const uint8_t *cdeg;   // [nc]
    const int32_t *loff;   // [nlayers] first slot of each layer
    int nv, nc, S, nlayers, slots, max_cdeg;
    const T *ch;           // [B][nv]
    T *app;                // [B][nv]
    int32_t *it;           // [B]
    int B, max_it;
    T factor;
};
// LDS bytes of one codeword's workgroup: app and R, then the tables
template <typename T>
inline size_t bp_layered_lds_bytes(int nv, int nc, int slots, int nlayers) {
    size_t b = sizeof(T) * ((size_t)nv + slots) + sizeof(int32_t) * (size_t)nlayers + sizeof(uint16_t) * (size_t)slots + nc;
    return (b + 15) / 16 * 16;
}
inline int bp_layered_threads(int S) { return S <= 64 ? 64 : 128; }
template <typename T>
int bp_layered_launch(const BpLayArgs<T> &a, int dectype, hipStream_t s);

template <typename T>
int bp_count_launch(const T *app, const uint8_t *x, const int32_t *its, int B, int nv, int k,
                    int64_t *counts, hipStream_t s, int32_t *per_cw = nullptr);
int lxfb_launch(double *dL, int dc, int corr, double *dagg, hipStream_t s);

// Device arithmetic shared by the flooding (bp.hip) and the layered (bp_layered.hip) kernels
template <typename T>
__device__ __forceinline__ T dev_log(T x);
template <>
__device__ __forceinline__ double dev_log<double>(double x) { return log(x); }
template <>
__device__ __forceinline__ float dev_log<float>(float x) { return __logf(x); }
template <typename T>
__device__ __forceinline__ T dev_exp(T x);
template <>
__device__ __forceinline__ double dev_exp<double>(double x) { return exp(x); }
template <>
__device__ __forceinline__ float dev_exp<float>(float x) { return __expf(x); }

// Pairwise XOR-LLR (reference Lxor, c_ldpc.c:234-251).
template <typename T, bool CORR>
__device__ __forceinline__ T lxor(T a, T b) {
    const bool same = (signbit(a) != 0) == (signbit(b) != 0);
    T out = (same ? T(1) : T(-1)) * fmin(fabs(a), fabs(b));
    if (CORR) {
        out += dev_log<T>(T(1) + dev_exp<T>(-fabs(a + b)));
        out -= dev_log<T>(T(1) + dev_exp<T>(-fabs(a - b)));
    }
    return out;
}

}  // namespace sg
