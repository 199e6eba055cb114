// What the Brain's translation units share: the parameter arena's layout, the forward pass's buffers and their one workspace layout, and
// the forward drivers of brain.hip that the DQN step (dqn_step.hip) runs as its first stage.
#pragma once
#include "adam.h"
#include "common.h"

namespace ivosw {

// offsets (floats) into the parameter / gradient arena, state_dict order
constexpr int O_W1 = 0, O_B1 = 256, O_W2 = 384, O_B2 = 16768, O_WIH = 16896, O_WHH = 82432, O_W3 = 147968,
              O_B3 = 180736, O_W4 = 180864, O_B4 = 180992;
static_assert(O_B4 + 1 == IVOSW_BRAIN_NPARAMS, "arena layout");
constexpr int HD = 128;

struct FwdBufs {
    float *a1, *e, *gx, *hs, *d1, *q;
    float *gates, *cs, *hprev;  // nullable; indexed by (sample - keep_from)
    int keep_from;
};

// The forward workspace's one layout: over a workspace it carves the buffers, over a counting Arena it gives the size (Arena::bytes).
// Samples >= keep_from (if any) keep gates / cs / hprev for the backward pass.
inline FwdBufs carve_fwd(Arena& ar, int N, int T, int keep_from) {
    const size_t r = (size_t)N * T;
    FwdBufs b{};
    b.a1 = ar.take<float>(r * 128);
    b.e = ar.take<float>(r * 128);
    b.gx = ar.take<float>(r * 512);
    b.hs = ar.take<float>(r * 256);
    b.d1 = ar.take<float>(r * 128);
    b.q = ar.take<float>(r);
    b.keep_from = keep_from;
    const int nkeep = (keep_from >= 0 && keep_from < N) ? N - keep_from : 0;
    if (nkeep > 0) {
        b.gates = ar.take<float>((size_t)2 * nkeep * T * 512);
        b.cs = ar.take<float>((size_t)2 * nkeep * T * 128);
        b.hprev = ar.take<float>((size_t)2 * nkeep * T * 128);
    }
    return b;
}

// ---------------------------------------------------------------- fused forward (DQN_FUSED): three launches per pass,
// or three launches for a policy pass AND a target pass together (see brain_fused.h)
struct FwdPass {
    const float* prm;
    const float* x;      // samples [0, N0)
    const float* x2;     // samples [N0, N) (nullptr: all from x)
    int N, N0;
    const FwdBufs* b;
};

// The minibatch DRAWN AND GATHERED by the encoder launch itself (ivosw_dqn_step_drawn: one link less in the step's launch chain
// than ivosw_replay_draw_gather in front of it).  Row r of a job is frame r % T of sample r / T; the sample's replay row is the
// draw of slot r / T (adam.h: draw_mix), its two input scalars come straight from the replay columns, and the policy job leaves
// the gathered minibatch behind for the head / tail kernels and the caller.  ds == nullptr: rows come from EncJob::x / x2.
struct EncDraw {
    const float *old_iou, *new_iou, *ann, *nann;       // [n, T] replay columns
    const int64_t* action;                              // [n]
    const float *rstep, *rdone;
    DrawState* ds;
    int n, B, T;
    int64_t* idx_out;                                   // [B] rows drawn
    float *state, *new_state;                           // [B, T, 2]
    int64_t* action_out;
    float *rstep_out, *rdone_out;
};

// brain.hip
int rows_per_wg(int rows);
bool fused_forward_ok(const FwdPass* f, int n);
void brain_forward_fused(const FwdPass* f, int n, int T, hipStream_t st, const EncDraw* draw = nullptr);
// x2 != nullptr: samples [0, N0) come from x, [N0, N) from x2
void brain_forward_internal(const float* prm, const float* x, int N, int T, const FwdBufs& b, hipStream_t st, const float* x2 = nullptr,
                            int N0 = 0);
// set by ivosw_lstm_probe (tuning aid; never in a product call path): the forward recurrences' phase stamps and the BPTT kernel's
extern unsigned long long* g_lstm_probe;
extern unsigned long long* g_lstm_probe_bwd;

#ifdef IVOSW_PROBES
#define PROBE_COVERS(cond, what)                                             \
    do {                                                                     \
        if (!(cond)) {                                                       \
            set_error("%s: not covered: %s", __func__, what);                \
            return IVOSW_ERR_ARG;                                            \
        }                                                                    \
    } while (0)
#endif

}  // namespace ivosw
