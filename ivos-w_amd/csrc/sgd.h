// The clamp + SGD update of one element, shared by every SGD path (clamp_sgd_kernel in dqn.hip, the one-call step's tail in
// dqn_step.hip, the data-parallel step's fused all-reduce + clamp + SGD in p2p.hip) so that all of them evaluate the same expression
// tree.  torch.optim.SGD(lr, momentum, dampening=0, weight_decay, nesterov), torch/optim/sgd.py:_single_tensor_sgd:
//   d = g + wd*p;  buf = buf*mu + d;  d = nesterov ? d + mu*buf : buf;  p = p - lr*d
// with the reference's clamp in front (models/agent.py:157-159) and gscale (= 1/world) before the clamp, as in clamp_adam_elem.
// torch's CPU rounding: `a.add(b, alpha=s)` rounds once (an fma with s in fp32), `buf.mul_(mu).add_(d)` rounds twice.  A zero-
// initialised buffer needs no first-step case: 0*mu + d == d (up to the sign of an exact zero), so there is no step counter at all.
#pragma once
#include <cmath>

#include "common.h"
#include "lr_sched.h"

namespace ivosw {

// The buffer update is written as a separate multiply and add with contraction switched off for this function: hipcc contracts
// a*b + c into an fma by default, and so would it the header forms of __fmul_rn / __fadd_rn once they are inlined.
__device__ __forceinline__ float clamp_sgd_elem(float g, float pi, float& bi, float lr, float mu, float wd, int nesterov, float clampv,
                                                float gscale) {
#pragma clang fp contract(off)
    float gi = g * gscale;
    gi = fminf(fmaxf(gi, -clampv), clampv);
    float d = fmaf(wd, pi, gi);
    const float bm = bi * mu;
    bi = bm + d;
    d = nesterov ? fmaf(mu, bi, d) : bi;
    return fmaf(-lr, d, pi);
}

// The step counter of a scheduled SGD update (cfg.agent.lr_schedule = "poly"), on the device so that a captured graph replays the
// schedule: the update reads lr_table[min(step, N)], and the last workgroup of the launch (the ticket: last_workgroup, dqn_update.h)
// publishes step + 1.  Layout (8 bytes): the counter is the int32 at byte 0; a caller resumes from host step k by writing k there.
// The constant-lr update keeps no counter.
struct SgdDevState {
    int step;
    unsigned ticket;
};
static_assert(sizeof(SgdDevState) == 8, "SgdDevState layout (step at byte 0, ticket at byte 4)");

// The hyper-parameters every SGD entry refuses (IVOSW_ERR_ARG) before it launches anything.
inline int check_sgd(const char* who, float lr, float momentum, float weight_decay, int nesterov) {
    const char* bad = nullptr;
    if (!(std::isfinite(lr) && lr >= 0.f)) bad = "lr must be finite and >= 0";
    else if (!(std::isfinite(momentum) && momentum >= 0.f)) bad = "momentum must be finite and >= 0";
    else if (!(std::isfinite(weight_decay) && weight_decay >= 0.f)) bad = "weight_decay must be finite and >= 0";
    else if (nesterov != 0 && nesterov != 1) bad = "nesterov must be 0 or 1";
    else if (nesterov && momentum == 0.f) bad = "nesterov needs a momentum > 0 (as torch.optim.SGD)";
    if (bad) {
        set_error("%s: %s (lr %g, momentum %g, weight_decay %g, nesterov %d)", who, bad, (double)lr, (double)momentum, (double)weight_decay,
                  nesterov);
        return IVOSW_ERR_ARG;
    }
    return IVOSW_OK;
}

}  // namespace ivosw
