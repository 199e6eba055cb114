// The learning-rate schedule of the update kernels (cfg.agent.lr_schedule = "poly"), shared by the Adam (adam.h) and SGD (sgd.h)
// paths.  The host computes the whole schedule once, as a float32 table of lr_steps + 1 entries
//   lr_table[k] = float32(lr * (1 - min(k, N) / N) ** lr_pow),   N = lr_steps
// (torch's PolynomialLR closed form), and the scheduled kernels read entry min(k, N) with k = the optimizer's device step counter
// BEFORE the update: the same float the eager entries get as their `lr` argument at host step k, so every path agrees bit for bit.
#pragma once
#include "common.h"

namespace ivosw {

__device__ __forceinline__ float sched_lr(const float* __restrict__ lr_table, int lr_steps, int k) {
    return lr_table[k <= 0 ? 0 : (k < lr_steps ? k : lr_steps)];
}

// What every scheduled entry refuses (IVOSW_ERR_ARG) before it launches anything.
inline int check_lr_table(const char* who, const float* lr_table, int lr_steps) {
    if (!lr_table) {
        set_error("%s: null lr_table", who);
        return IVOSW_ERR_ARG;
    }
    if (lr_steps < 1) {
        set_error("%s: lr_steps must be >= 1, got %d", who, lr_steps);
        return IVOSW_ERR_ARG;
    }
    return IVOSW_OK;
}

}  // namespace ivosw
