// The target-network rule of the DQN step (cfg.agent.target_update = "soft" | "periodic").  ivosw_target_update (dqn.hip) and the one-call
// step's fused tails (dqn_step.hip) both apply it through target_group (dqn_update.h), so both evaluate the same expression.  After the
// policy update of a step, per element:
//   soft:      t = fmaf(tau, p_new - t, t)          (one rounding of the product-sum: torch.Tensor.lerp_(p, tau) on the CPU for tau < 0.5)
//   periodic:  t = p_new when k % period == 0, k = the number of steps since the counter was last written, this one included
// "coin", the reference's host coin flip, never reaches these kernels.
#pragma once
#include <cmath>

#include "common.h"

namespace ivosw {

constexpr int TARGET_SOFT = 1, TARGET_PERIODIC = 2;          // IVOSW_TARGET_* (include/ivosw.h)

// The step counter of the rule, on the device so that a captured graph replays it: every workgroup reads `step` (the steps before this
// one), the last workgroup of the launch (the ticket: last_workgroup, dqn_update.h) publishes step + 1.  The fused tails of an optimizer
// that has a ticket of its own advance `step` under that one.  Layout (16 bytes): the counter is the int32 at byte 0; a caller resumes
// from host step k by writing k there.
struct TargetDevState {
    int step;
    unsigned ticket;
    unsigned reserved[2];
};
static_assert(sizeof(TargetDevState) == 16, "TargetDevState layout (step at byte 0, ticket at byte 4)");

// Does the step that follows k earlier ones copy the policy?  (soft: not looked at)
__device__ __forceinline__ bool target_fires(int k, int period) { return ((unsigned)k + 1u) % (unsigned)period == 0u; }

// What every entry that takes the rule refuses (IVOSW_ERR_ARG) before it launches anything.
inline int check_target(const char* who, const void* target_state, int mode, float tau, int period) {
    if (!target_state) {
        set_error("%s: null target_state", who);
        return IVOSW_ERR_ARG;
    }
    if (mode != TARGET_SOFT && mode != TARGET_PERIODIC) {
        set_error("%s: unknown target mode %d (IVOSW_TARGET_SOFT or IVOSW_TARGET_PERIODIC)", who, mode);
        return IVOSW_ERR_ARG;
    }
    if (mode == TARGET_SOFT && !(std::isfinite(tau) && tau > 0.f && tau < 0.5f)) {
        set_error("%s: tau must be in (0, 0.5), got %g (a hard copy is the periodic mode)", who, (double)tau);
        return IVOSW_ERR_ARG;
    }
    if (mode == TARGET_PERIODIC && period < 1) {
        set_error("%s: period must be >= 1, got %d", who, period);
        return IVOSW_ERR_ARG;
    }
    return IVOSW_OK;
}

}  // namespace ivosw
