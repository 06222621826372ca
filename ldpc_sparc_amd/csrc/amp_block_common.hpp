// What the two block engines share (amp_block.hip: one class, 16 column
// entries per thread; amp_block2.hip: two classes, 32 per thread): the layout
// of a column block over the workgroup's threads, the position tables and the
// image clear.  The transforms, the load schedules and the per-section body
// stay with each engine: moved here, they compile to different code.
#pragma once
#include "amp.hpp"

namespace sg {

// Zeroes the IMG complex slots of the LDS image, 16 bytes per store
template <int THREADS, int IMG>
__device__ __forceinline__ void blk_clear(unsigned char *smem, int tid) {
    constexpr int N16 = IMG * (int)sizeof(cx<float>) / 16;  // (8 per thread and a quarter)
#pragma unroll
    for (int i = 0; i < (N16 + THREADS - 1) / THREADS; ++i)
        if (tid + i * THREADS < N16) reinterpret_cast<uint4 *>(smem)[tid + i * THREADS] = uint4{0, 0, 0, 0};
}

// Column entry i (< J) of thread tid: wavefront w owns sections
// w spw .. w spw + spw - 1 of the column block (spw = 64 J / M), lane l holds
// entries l eps .. l eps + eps - 1 of each (eps = M / 64).  Needs 64 J entries
// per wavefront and 64 <= M <= 64 J (host mirror in amp_plan_block.cpp
// build_block, build_block2).
template <int EPS, int J>
__device__ __forceinline__ int blk_j(int tid, int i) {
    constexpr int M = 64 * EPS, SPW = 64 * J / M;
    const int sq = i / EPS, e = i - sq * EPS;
    return ((tid >> 6) * SPW + sq) * M + (tid & 63) * EPS + e;
}

// LDS positions (real index) of the thread's column entries blk_j(tid, i) in
// image tq of the position table (the transform t, or transform and class
// 2 t + m2), packed in pairs (i = 2 i2, 2 i2 + 1) in thread order.  Called
// through each engine's one-line wrapper: called directly from the kernels'
// loops it compiles to different code.
template <int THREADS, int J>
__device__ __forceinline__ void blk_pos_load(const BlkTables &tb, size_t tq, int tid, uint32_t *pv) {
    const uint32_t *p2 = tb.pos2 + tq * (J / 2) * THREADS;
#pragma unroll
    for (int i = 0; i < J / 2; ++i) pv[i] = p2[i * THREADS + tid];
}
__device__ __forceinline__ uint32_t blk_pos(const uint32_t *pv, int i) { return (pv[i >> 1] >> (16 * (i & 1))) & 0xffffu; }

}  // namespace sg
