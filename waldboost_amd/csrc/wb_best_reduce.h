// The best candidate of a workgroup: the reduction both split searches (wb_fit.hip, wb_cart.hip) end their argmaxes with.
// The candidate type brings its own order as `static bool better(const Best &a, const Best &b)` -- a wins over b --, which
// must be a strict total order on distinct candidates so that the result does not depend on the order of the folds.
#pragma once
#include <type_traits>

#include "wb_common.h"

// Valid in thread 0 of a workgroup of WAVES waves; `part` (LDS) has one entry per wave.  A butterfly of __shfl_xor moves
// the candidate between lanes 32 bits at a time (a Best without padding costs sizeof(Best) / 4 shuffles per step), lane 0
// of every wave leaves its wave's best in `part`, thread 0 folds the waves in ascending order.
template <int WAVES, typename Best>
__device__ inline Best wb_best_reduce(Best c, Best *part) {
    static_assert(std::is_trivially_copyable<Best>::value && sizeof(Best) % 4 == 0, "a candidate is a whole number of dwords");
    constexpr int DWORDS = sizeof(Best) / 4;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        int32_t w[DWORDS];
        __builtin_memcpy(w, &c, sizeof(Best));
#pragma unroll
        for (int i = 0; i < DWORDS; ++i) w[i] = __shfl_xor(w[i], off);
        Best o;
        __builtin_memcpy(&o, w, sizeof(Best));
        if (Best::better(o, c)) c = o;
    }
    const int wave = threadIdx.x / WB_WAVE;
    __syncthreads();                            // (part may still be read from the previous reduction)
    if (threadIdx.x % WB_WAVE == 0) part[wave] = c;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < WAVES; ++w)
            if (Best::better(part[w], c)) c = part[w];
    return c;
}
