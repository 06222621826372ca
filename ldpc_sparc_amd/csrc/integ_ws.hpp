// Workspace of the integrated AMP <-> BP decoders (integ_loop.hpp), one member of a dense plan and of a DCT plan.
#pragma once
#include "device_mem.hpp"

#pragma GCC visibility push(hidden)  // shared between the library's objects, not exported from it
namespace sg {

// Grow-only per (plan, B), slots recorded like a batch workspace's: u = Az(z) / weighted alpha and gamma [B][LM];
// xhat = Ab(beta) [B][n] (DCT plan only); vk0, vk, LLRs, app [B][L log M]; BP iteration counts; per-section sums
// (differentiated eta, or beta^2 of the DCT plan's naive decoders) and their per-codeword sum.  The owner must not
// move (DevPool).
struct IntegWs {
    DevPool pool;
    int cap_B = 0;
    void *alpha = nullptr, *gamma = nullptr, *x = nullptr, *vk0 = nullptr, *vk = nullptr, *llr = nullptr,
         *app = nullptr;
    int32_t *it = nullptr;
    double *part = nullptr, *ons = nullptr;

    int ensure(int B, int L, int LM, int n, int nbits, size_t elem_bytes, bool want_x) {
        if (B <= cap_B) return SG_OK;
        pool.release();
        cap_B = 0;
        const size_t rs = elem_bytes, Bz = (size_t)B;
        SG_TRY(pool.alloc(&alpha, Bz * LM * rs));
        SG_TRY(pool.alloc(&gamma, Bz * LM * rs));
        if (want_x) SG_TRY(pool.alloc(&x, Bz * n * rs));
        for (void **slot : {&vk0, &vk, &llr, &app}) SG_TRY(pool.alloc(slot, Bz * nbits * rs));
        SG_TRY(pool.alloc(&it, Bz * nbits * sizeof(int32_t)));
        SG_TRY(pool.alloc(&part, Bz * L * sizeof(double)));
        SG_TRY(pool.alloc(&ons, Bz * sizeof(double)));
        cap_B = B;
        return SG_OK;
    }
};

}  // namespace sg
#pragma GCC visibility pop
