/* ivosw.h — C ABI of libivosw_hip.so: the MI355X (gfx950) hot path of IVOS-W.
 *
 * The reference (svip-lab/IVOS-W) is pure Python over PyTorch ops and has NO FFI/plugin interface
 * (SURVEY.md §8b); the boundary it offers is the Python class surface models.agent.{Brain,Agent},
 * models.assessment.{Encoder,AssessNet}.  Each entry point below therefore cites the reference
 * *method* whose arithmetic it replaces (paths relative to the reference root).
 *
 * Conventions
 *   - extern "C", plain pointers + sizes.  No torch / HIP types in signatures: a stream is passed as
 *     void* (it is a hipStream_t; NULL = the null stream).
 *   - Every pointer is a DEVICE pointer owned by the caller unless a parameter says "host".
 *     Workspaces are sized by the *_ws_bytes queries and handed in by the caller; the library keeps no
 *     per-call state in them.  Two exceptions, both documented at their entry points: ivosw_p2p_alloc /
 *     ivosw_p2p_free allocate the fine-grained peer-to-peer arena (a kind of memory neither torch nor a
 *     caller can allocate), and ivosw_assess_forward keeps ONE helper stream + two events per device for
 *     the two-stream split of a batch (created on first use, never freed).
 *   - All calls are asynchronous on `stream`; nothing synchronises the device (except the entries that
 *     return a host value: ivosw_p2p_error, ivosw_profile_*).
 *   - Return 0 on success, negative on error; ivosw_last_error() gives a thread-local message.
 *   - Not thread-safe per workspace; distinct workspaces on distinct streams are independent.
 */
#ifndef IVOSW_H
#define IVOSW_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IVOSW_OK 0
#define IVOSW_ERR_ARG (-1)      /* bad argument (null pointer, non-positive size, bad enum)   */
#define IVOSW_ERR_WS (-2)       /* workspace too small                                         */
#define IVOSW_ERR_LAUNCH (-3)   /* HIP launch / runtime error                                  */

#define IVOSW_F32 0             /* fp32 operands, fp32 accumulate (parity mode)                */
#define IVOSW_BF16 1            /* bf16 operands, fp32 accumulate (throughput mode)            */
#define IVOSW_F32X3 2           /* fp32 activations and weights, contractions as THREE bf16 MFMA passes: x = hi + lo with hi, lo in bf16,
                                 * a b ~ ah bh + ah bl + al bh, fp32 accumulate (error ~ 2^-17 per product: scores within 1e-4 rtol of the
                                 * reference like IVOSW_F32, at 16 / 3 of its matrix rate).  Layout and workspaces are IVOSW_F32's;
                                 * the packed arena holds the conv weights pre-split, so it must be packed with this dtype.            */

/* Brain parameter arena: the 10 tensors of Brain.state_dict() concatenated in state_dict order
 * (models/agent.py:13-31): encoder_fc1.{weight[128,2],bias[128]}, encoder_fc2.{weight[128,128],bias[128]},
 * lstm_cell.{weight_ih[512,128],weight_hh[512,128]}, decoder_fc1.{weight[128,256],bias[128]},
 * decoder_fc2.{weight[1,128],bias[1]}.                                                         */
#define IVOSW_BRAIN_NPARAMS 180993

typedef void* ivosw_stream_t;

const char* ivosw_last_error(void);
int ivosw_version(void);

/* ------------------------------------------------------------------ agent: Brain (K7) --------- */
/* Replaces Brain.forward (models/agent.py:33-64): x [N,T,2] fp32 -> q [N,T] fp32.
 * One shared bias-free LSTM cell runs forward and backward over the T frames from a zero state. */
size_t ivosw_brain_ws_bytes(int N, int T);
int ivosw_brain_forward(const float* params, const float* x, int N, int T, float* q,
                        void* ws, size_t ws_bytes, ivosw_stream_t stream);
/* Replaces Q.argmax() in Agent.action (models/agent.py:187-188): first maximum per row -> idx[N]. */
int ivosw_brain_argmax(const float* q, int N, int T, int64_t* idx, ivosw_stream_t stream);
/* Ragged forward: n_seqs (1 .. IVOSW_MAX_SEQS) sequences, each of its OWN length, in one launch chain.  `lengths` is a HOST array, read
 * during the call only; the sequence table (row offsets) travels to the kernels inside their arguments (no allocation, no copy, no
 * synchronisation: capture-safe).  x [R,2] and q [R] are flat over the sequences in the order given, R = sum of lengths; sequence k owns
 * the rows [row_off[k], row_off[k] + lengths[k]).  Each sequence gets, bit for bit, what ivosw_brain_forward(N = 1, T = lengths[k])
 * computes on its slice: the encoder and the decoder are row-wise over the R flat rows, and the recurrence runs one workgroup per
 * (sequence, direction) with that sequence's own trip count - the backward direction starts at the sequence's own last frame, nothing
 * is padded.  Three launches; with DQN_FUSED or LSTM_QUAD switched off, the N = 1 path of ivosw_brain_forward per sequence.
 * ivosw_brain_ragged_rows: host only; R, or < 0 (IVOSW_ERR_ARG) if the call would be refused.
 * ivosw_brain_argmax_ragged: the first maximum of every sequence's slice of q (index inside the slice) -> idx[n_seqs]; one launch.
 * Refused (IVOSW_ERR_ARG) before anything is launched, the message names the sequence's index: a NULL pointer, n_seqs outside
 * [1, IVOSW_MAX_SEQS], a length < 1, R > 2^20.  A workspace below ivosw_brain_ragged_ws_bytes(R): IVOSW_ERR_WS.                     */
#define IVOSW_MAX_SEQS 128
long ivosw_brain_ragged_rows(const int* lengths, int n_seqs);
size_t ivosw_brain_ragged_ws_bytes(long rows);
int ivosw_brain_forward_ragged(const float* params, const float* x, const int* lengths, int n_seqs,
                               float* q, void* ws, size_t ws_bytes, ivosw_stream_t stream);
int ivosw_brain_argmax_ragged(const float* q, const int* lengths, int n_seqs, int64_t* idx, ivosw_stream_t stream);
/* Ragged, masked top-k: the k (1 .. IVOSW_MAX_CANDIDATES) strongest frames of every sequence's slice of q, in the place of the single
 * Q.argmax() of Agent.action (models/agent.py:168-196), with select_next_frame's rule for annotated frames (utils_agent.py:38-74) on the
 * device.  The frames of a sequence are ranked by this total order, the strongest first:
 *   1. the tier: with skip_annotated != 0, frames whose annotation count state[(r0 + t) * 2 + 1] is 0 come before all others (when
 *      every frame is annotated the ranking falls through to them, as select_next_frame does); with skip_annotated == 0 there is one
 *      tier, and `state` (the [R,2] state ivosw_quality_state[_ragged] writes) may be NULL;
 *   2. inside a tier the larger q first: -0 and +0 are equal, +inf and -inf are ordinary values, NaN ranks below every number;
 *   3. then the lower index first.
 * idx[s * k + j] = the j-th frame of sequence s in that order (index inside the slice, as ivosw_brain_argmax_ragged returns it), -1
 * for j >= lengths[s]; qv (nullable) [n_seqs, k] = the bits of q at that frame, 0.0f for a -1 slot.  With k = 1 and skip_annotated = 0
 * idx equals ivosw_brain_argmax_ragged on any NaN-free q.  One launch, one wave per sequence, no workspace; capture-safe.
 * Refused (IVOSW_ERR_ARG) before anything is launched, the message names the argument: a NULL q, lengths or idx, k outside
 * [1, IVOSW_MAX_CANDIDATES], skip_annotated != 0 with a NULL state, and what ivosw_brain_ragged_rows refuses.                          */
#define IVOSW_MAX_CANDIDATES 16
int ivosw_brain_topk_ragged(const float* q, const float* state, const int* lengths, int n_seqs, int k, int skip_annotated,
                            int64_t* idx, float* qv, ivosw_stream_t stream);

/* The same ranking with its k frames spread in time (agent.candidate_gap): Q sits on a bidirectional LSTM over the frame axis and is
 * smooth along it, so the k strongest frames are usually one peak and its neighbours.  The frames of a sequence are walked in the total
 * order of ivosw_brain_topk_ragged (tier, larger q, lower index) and a frame t is accepted if and only if |t - w| >= gap for every frame w
 * accepted so far; the walk stops after k accepted frames.  gap = 1 is ivosw_brain_topk_ragged, bit for bit.  Only accepted frames
 * suppress: annotated frames by themselves suppress nothing, and under skip_annotated the walk falls through to the annotated tier as
 * before, under the same distance rule.  When fewer than k frames can be accepted the remaining slots are -1 (nothing suppressed comes
 * back).  first (HOST memory, n_seqs ints, NULL = all -1): first[s] >= 0 is the forced first candidate of sequence s (the epsilon
 * branch's random pick): it is slot 0 whatever its q or tier, counts as accepted, and the walk fills slots 1 .. k - 1.  It is read
 * during the call and travels inside the kernel arguments, as lengths does: no allocation, no copy, no synchronisation.  idx and qv as
 * for ivosw_brain_topk_ragged (qv: the bits of q at each slot, 0.0f at a -1 slot).  One launch, one wave per sequence, no workspace;
 * capture-safe.  Refused (IVOSW_ERR_ARG) before anything is launched, the message names the argument: what ivosw_brain_topk_ragged
 * refuses, gap outside [1, IVOSW_MAX_CANDIDATE_GAP], and a first[s] outside [-1, lengths[s]) (the message names s).                    */
#define IVOSW_MAX_CANDIDATE_GAP (1 << 20)
int ivosw_brain_topk_spread_ragged(const float* q, const float* state, const int* lengths, int n_seqs, int k, int skip_annotated, int gap,
                                   const int* first, int64_t* idx, float* qv, ivosw_stream_t stream);

/* ------------------------------------------------------------------ agent: DQN step (K8-K10) -- */
/* Replaces the arithmetic of Agent.update_agent (models/agent.py:128-155):
 *   a* = argmax policy(s'); Qn = target(s')[a*]; y1 = gamma*Qn + 0.1*r_step; y2 = 0.1*r_done;
 *   Qsa = policy(s)[action]; loss = mean((Qsa-y1)^2) + mean((Qsa-y2)^2); grads = dLoss/dpolicy.
 * state/new_state [B,T,2] fp32, action [B] int64, reward_* [B] fp32.  grads [NPARAMS] is overwritten,
 * *loss is a device float.  The grads are NOT clamped here so that a data-parallel caller can
 * all-reduce them first (RCCL) and clamp afterwards.                                             */
size_t ivosw_dqn_ws_bytes(int B, int T);
int ivosw_dqn_loss_grad(const float* policy, const float* target,
                        const float* state, const float* new_state, const int64_t* action,
                        const float* reward_step, const float* reward_done,
                        int B, int T, float gamma, float* grads, float* loss,
                        void* ws, size_t ws_bytes, ivosw_stream_t stream);
/* The loss option of the _ex entries.  IVOSW_DQN_LOSS_MSE is the two-term MSE above (models/agent.py:149-151), bit for bit what
 * ivosw_dqn_loss_grad computes.  IVOSW_DQN_LOSS_HUBER generalises it term by term with torch.nn.functional.huber_loss(reduction="mean",
 * delta): e1 = Qsa-y1, e2 = Qsa-y2, h(e) = e^2/2 if |e| < delta else delta*(|e| - delta/2); loss = mean(h(e1)) + mean(h(e2));
 * dLoss/dQsa = (clamp(e1,-delta,delta) + clamp(e2,-delta,delta)) / B (delta -> inf: half of MSE).  The targets are unchanged.
 * huber_delta must be finite and > 0 (for either kind); anything else, or an unknown kind, returns IVOSW_ERR_ARG.              */
#define IVOSW_DQN_LOSS_MSE 0
#define IVOSW_DQN_LOSS_HUBER 1
int ivosw_dqn_loss_grad_ex(const float* policy, const float* target,
                           const float* state, const float* new_state, const int64_t* action,
                           const float* reward_step, const float* reward_done,
                           int B, int T, float gamma, int loss_kind, float huber_delta, float* grads, float* loss,
                           void* ws, size_t ws_bytes, ivosw_stream_t stream);
/* Prioritized replay (cfg.agent.replay = "prioritized"): ivosw_dqn_loss_grad_ex with the importance-sampling weights of the minibatch,
 * weights [B] (ivosw_per_draw_gather).  The same launches, with the weighted head: row b's loss terms become w_b * terms(e1, e2) (loss =
 * their sum / B, in the same order; w_b * terms is one rounded product) and dLoss/dQsa_b = (w_b * c) * s for dq = c * s (c = 2/B for
 * MSE, 1/B for Huber; s the sum of the two errors or of the two clamped errors); td_out [B] receives
 * |e1| + |e2|, what ivosw_per_update takes.  With every weight 1 the results equal ivosw_dqn_loss_grad_ex's bit for bit.  weights and
 * td_out must not be NULL; the other checks are ivosw_dqn_loss_grad_ex's.                                                          */
int ivosw_dqn_loss_grad_per(const float* policy, const float* target,
                            const float* state, const float* new_state, const int64_t* action,
                            const float* reward_step, const float* reward_done,
                            int B, int T, float gamma, int loss_kind, float huber_delta, const float* weights, float* td_out,
                            float* grads, float* loss, void* ws, size_t ws_bytes, ivosw_stream_t stream);
/* Replaces grad.clamp_(-1,1) + optim.Adam.step (models/agent.py:157-160, :101): g = clamp(grad*grad_scale);
 * g += wd*p; m,v update; p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps).  step = t >= 1.
 * grad_scale = 1/world_size after a sum all-reduce, 1 otherwise.                                 */
int ivosw_clamp_adam(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int n,
                     int step, float lr, float beta1, float beta2, float eps, float weight_decay,
                     float clamp, float grad_scale, ivosw_stream_t stream);
/* The same update with Adam's step counter and bias corrections kept on the device (adam_state: ivosw_adam_state_bytes()
 * bytes, zero-initialised = step 0; the step counter is the int32 at byte offset 16, which is all a caller writes to resume
 * from step k), so that a HIP graph that captured the call replays correctly: every call (or replay) advances the step by one.                                                 */
size_t ivosw_adam_state_bytes(void);
int ivosw_clamp_adam_dev(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int n, void* adam_state,
                         float lr, float beta1, float beta2, float eps, float weight_decay, float clamp,
                         float grad_scale, ivosw_stream_t stream);
/* cfg.agent.optimizer = "sgd": grad.clamp_(-1,1) + torch.optim.SGD(lr, momentum, dampening=0, weight_decay, nesterov).step in one
 * kernel: g = clamp(grad*grad_scale); d = g + wd*p; buf = buf*momentum + d; d = nesterov ? d + momentum*buf : buf; p -= lr*d.
 * momentum_buf [n] starts at zero (torch's first step, buf = d, is then the same update) and is the only state carried from one step
 * to the next: no step counter, so a captured HIP graph replays the call as it stands.  Refused (IVOSW_ERR_ARG) before any launch:
 * a NULL pointer, n <= 0, a negative or non-finite lr / momentum / weight_decay, nesterov other than 0 / 1, nesterov with
 * momentum 0.  grad_scale = 1/world_size after a sum all-reduce, 1 otherwise.                                                      */
int ivosw_clamp_sgd(float* params, const float* grads, float* momentum_buf, int n, float lr, float momentum, float weight_decay,
                    int nesterov, float clamp, float grad_scale, ivosw_stream_t stream);
/* cfg.agent.lr_schedule = "poly": the learning rate of each update comes from a float32 table on the device,
 *   lr_table[k] = float32(lr * (1 - min(k, N) / N) ** lr_pow),  k = 0 .. N = lr_steps   (torch's PolynomialLR closed form),
 * computed once by the caller.  The update that follows k earlier ones (the device step counter before it advances) reads
 * lr_table[min(k, N)]: the float the eager entries (ivosw_clamp_adam, ivosw_clamp_sgd, the P2P forms) get as lr at host step k, so the
 * paths agree bit for bit.  The _sched entries take (lr_table, lr_steps) in place of lr; each refuses (IVOSW_ERR_ARG, before any launch)
 * a NULL pointer or table, lr_steps < 1, and the bad hyper-parameters of its constant-lr form.
 * ivosw_clamp_adam_dev_sched: ivosw_clamp_adam_dev on the schedule (the same AdamDevState and ticket; betas outside [0, 1) and a
 * negative or non-finite eps / weight_decay are refused).                                                                              */
int ivosw_clamp_adam_dev_sched(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int n, void* adam_state,
                               const float* lr_table, int lr_steps, float beta1, float beta2, float eps, float weight_decay, float clamp,
                               float grad_scale, ivosw_stream_t stream);
/* ivosw_clamp_sgd on the schedule.  The constant-lr form keeps no step counter; this one keeps it in sgd_state (ivosw_sgd_state_bytes()
 * bytes, zeroed before the first step; the int32 at byte 0 is the counter, a caller resumes from host step k by writing k there),
 * advanced by the last workgroup of each launch so that a captured graph replays the schedule.                                        */
size_t ivosw_sgd_state_bytes(void);
int ivosw_clamp_sgd_dev_sched(float* params, const float* grads, float* momentum_buf, int n, void* sgd_state, const float* lr_table,
                              int lr_steps, float momentum, float weight_decay, int nesterov, float clamp, float grad_scale,
                              ivosw_stream_t stream);
/* Replaces target_net.load_state_dict(policy_net.state_dict()) (models/agent.py:163-165).        */
int ivosw_copy_f32(float* dst, const float* src, size_t n, ivosw_stream_t stream);
/* The target-network rule on the device (cfg.agent.target_update = "soft" | "periodic"), applied after the policy update of a step:
 *   IVOSW_TARGET_SOFT      target[i] = fmaf(tau, policy[i] - target[i], target[i]), tau in (0, 0.5): Polyak averaging, the bits of
 *                          torch.Tensor.lerp_(policy, tau) on the CPU (period is not looked at);
 *   IVOSW_TARGET_PERIODIC  target[i] = policy[i] when k % period == 0, k = the launches since the counter was last written, this one
 *                          included; otherwise nothing is touched (tau is not looked at).
 * target_state: ivosw_target_state_bytes() (16) bytes, zeroed before the first step.  The int32 at byte 0 is the step counter, a caller
 * resumes from host step k by writing k there; every workgroup reads it and the last one of the launch advances it, so a captured
 * graph replays the rule.  One launch.  Refused before anything is launched (IVOSW_ERR_ARG): a NULL state, an unknown mode, under soft a
 * tau outside (0, 0.5) or not finite, under periodic a period < 1, NULL or identical arenas, n < 1.                                   */
#define IVOSW_TARGET_SOFT 1
#define IVOSW_TARGET_PERIODIC 2
size_t ivosw_target_state_bytes(void);
int ivosw_target_update(float* target, const float* policy, int n, int mode, float tau, int period, void* target_state,
                        ivosw_stream_t stream);

/* ------------------------------------------------------------------ one-shot P2P all-reduce --- */
/* The data-parallel DQN step's gradient all-reduce (Agent.update_agent under torch.distributed; the reference is single
 * GPU) over xGMI peer-to-peer writes instead of a ring: every rank pushes its n floats into its slot of every peer's arena and
 * raises a flag there (7 links in parallel, one hop), then sums the `world` slots it received in rank order (bit-identical
 * on all ranks).  The arena is FINE-GRAINED device memory (coherent inside kernels across GPUs) — the one device allocation the
 * library makes itself: ivosw_p2p_alloc (returns the pointer and an IPC handle of ivosw_p2p_handle_bytes() bytes to send to
 * the peers) / ivosw_p2p_free; peers map it with ivosw_p2p_open / unmap with ivosw_p2p_close.  ivosw_p2p_allreduce:
 * arenas = HOST array of `world` device pointers (own arena at [rank]); epoch = 1, 2, 3, ... identical on every rank, one per
 * call; out may alias grads (16-byte aligned); a peer that does not arrive within timeout_ms sets the arena's error word
 * (ivosw_p2p_error) instead of hanging the GPU.  Two kernels per call, no host synchronisation.                           */
size_t ivosw_p2p_arena_bytes(int world, size_t n);
size_t ivosw_p2p_handle_bytes(void);
int ivosw_p2p_alloc(size_t bytes, void** arena, void* ipc_handle, size_t ipc_handle_bytes);
int ivosw_p2p_open(const void* ipc_handle, void** peer_arena);
int ivosw_p2p_close(void* peer_arena);
int ivosw_p2p_free(void* arena);
int ivosw_p2p_error(const void* arena, int* error);
int ivosw_p2p_allreduce(const float* grads, float* out, int n, int rank, int world, void* const* arenas, unsigned epoch,
                        int timeout_ms, ivosw_stream_t stream);
/* ivosw_p2p_allreduce followed by ivosw_clamp_adam(grad_scale = 1/world) as TWO launches: push, then wait + rank-ordered sum + clamp
 * + Adam (the reference's clamp / optim.Adam step, models/agent.py:157-160, on the gradient averaged over the ranks).  grads_out
 * (NULL allowed, may alias grads) receives the summed gradient; `step` is the 1-based Adam step.  On a timeout nothing is updated
 * (one verdict for the whole grid: workgroup 0 alone declares it) and the arena's error word is set (ivosw_p2p_error); once the
 * word is set every later call returns without touching its outputs until the arena is re-created.                                                                        */
int ivosw_p2p_allreduce_clamp_adam(const float* grads, float* grads_out, int n, int rank, int world, void* const* arenas,
                                   unsigned epoch, int timeout_ms, float* params, float* exp_avg, float* exp_avg_sq, int step,
                                   float lr, float beta1, float beta2, float eps, float weight_decay, float clamp,
                                   ivosw_stream_t stream);
/* ivosw_p2p_allreduce followed by ivosw_clamp_sgd(grad_scale = 1/world) as TWO launches: push, then wait + rank-ordered sum + clamp
 * + SGD.  The arguments, the timeout and the error word are those of ivosw_p2p_allreduce_clamp_adam, with momentum_buf and SGD's
 * hyper-parameters in place of Adam's state; the hyper-parameters are refused as by ivosw_clamp_sgd, before any launch.            */
int ivosw_p2p_allreduce_clamp_sgd(const float* grads, float* grads_out, int n, int rank, int world, void* const* arenas,
                                  unsigned epoch, int timeout_ms, float* params, float* momentum_buf, float lr, float momentum,
                                  float weight_decay, int nesterov, float clamp, ivosw_stream_t stream);

/* ------------------------------------------------------------------ replay gather (K11) ------- */
/* Replaces DataLoader shuffle+collate of memory_pool.csv rows (datasets/agent_dataset.py:71-115,
 * train_agent.py:177-182) for a device-resident SoA replay buffer: columns [cap,T] fp32 and [cap]
 * scalars; idx [B] int64 -> state/new_state [B,T,2] and the [B] columns of the minibatch.        */
int ivosw_replay_gather(const float* old_iou, const float* new_iou, const float* annotated,
                        const float* next_annotated, const int64_t* action, const float* reward_step,
                        const float* reward_done, const int64_t* idx, int B, int T,
                        float* state, float* new_state, int64_t* action_out, float* reward_step_out,
                        float* reward_done_out, ivosw_stream_t stream);
/* The same gather with the minibatch indices DRAWN ON THE DEVICE (uniform over [0, n) with replacement — the role of the
 * DataLoader's shuffle, train_agent.py:177-182 — from a counter-based generator), so that a captured HIP graph of a training
 * step needs no host-side RNG launch: draw_state is ivosw_replay_draw_state_bytes() bytes on the device {uint64 seed at byte
 * 0, uint32 draw counter at byte 8, 4 bytes the library owns (zero)}; every call (or graph replay) uses the current counter
 * and advances it by one.  Slot b of draw c reads row ivosw_replay_draw_index(seed, c, b, n) — the host mirror of the device
 * arithmetic (integer only, bit-exact).  idx_out [B] int64 receives the rows that were drawn.                                */
size_t ivosw_replay_draw_state_bytes(void);
unsigned long long ivosw_replay_draw_index(unsigned long long seed, unsigned counter, unsigned slot, int n);
int ivosw_replay_draw_gather(const float* old_iou, const float* new_iou, const float* annotated,
                             const float* next_annotated, const int64_t* action, const float* reward_step,
                             const float* reward_done, void* draw_state, int n, int B, int T, int64_t* idx_out,
                             float* state, float* new_state, int64_t* action_out, float* reward_step_out,
                             float* reward_done_out, ivosw_stream_t stream);

/* Prioritized experience replay (Schaul et al. 2016; cfg.agent.replay = "prioritized") on a device sum tree.  A replay of n rows
 * (1 <= n <= 2^24) keeps a float32 tree [ivosw_per_tree_floats(n)] = [2P], P = the next power of two >= max(n, 2): node 1 is the root,
 * the children of node i are 2i and 2i+1, the leaf of row r is node P + r (0 for r >= n), slot 0 is unused, and every internal node is
 * float32(left + right), always recomputed from its two children - the tree is a pure function of its leaves.  per_state is
 * ivosw_per_state_bytes() bytes on the device: {uint64 seed at byte 0, uint32 draw counter at byte 8 (write it to resume), float
 * max_priority at byte 16 (1.0 on a fresh replay), the rest the library's (zero)}.
 * ivosw_per_build: leaves [0, n_old) are copied from old_leaves (device, NULL when n_old = 0), leaves [n_old, n) - rows the tree has not
 *   seen - are max_priority^alpha, then every internal node is built (log2 P + 1 launches: setup and replay reloads, deterministic).
 * ivosw_per_draw_gather: draw c (the counter before it advances by one; every call or graph replay advances it) fills slot b < B with
 *   z = the 64-bit mix of ivosw_replay_draw_index(seed, c, b), u = float32(z >> 40) * 2^-24, x = (tree[1] / B) * (b + u) in fp32; from
 *   node 1 down: l = tree[2 node], x < l ? go left : (x -= l, go right); row = min(leaf - P, n - 1) (stratified sampling, P(row) =
 *   leaf / total).  beta_c = beta0 + (1 - beta0) * (min(c, N) / N) in fp32 (beta0 when N = beta_steps = 0), w'_b = (leaf_row * n /
 *   total)^-beta_c, weights_out[b] = w'_b / max w' (<= 1).  idx_out receives the rows, and the gather is ivosw_replay_gather's on them,
 *   bit for bit.  One workgroup; B <= 1024.
 * ivosw_per_update: p_b = td[b] + eps; where a row fills several slots the highest slot wins; its leaf becomes p_b^alpha, every
 *   ancestor of a touched leaf is recomputed from its children (the tree equals a full rebuild from its leaves, bit for bit), and
 *   max_priority = max(max_priority, max_b p_b).  One workgroup; rows outside [0, n) are skipped.
 * Refused (IVOSW_ERR_ARG) before any launch: a NULL pointer, n outside [1, 2^24], n_old outside [0, n], B outside [1, 1024], T < 1,
 * a negative or non-finite alpha, beta0 outside [0, 1], beta_steps < 0, an eps that is not finite and > 0.                           */
size_t ivosw_per_state_bytes(void);
size_t ivosw_per_tree_floats(int n);
int ivosw_per_build(float* tree, int n, const float* old_leaves, int n_old, void* per_state, float alpha, ivosw_stream_t stream);
int ivosw_per_draw_gather(const float* old_iou, const float* new_iou, const float* annotated, const float* next_annotated,
                          const int64_t* action, const float* reward_step, const float* reward_done, const float* tree, void* per_state,
                          int n, int B, int T, float beta0, int beta_steps, int64_t* idx_out, float* weights_out, float* state,
                          float* new_state, int64_t* action_out, float* reward_step_out, float* reward_done_out, ivosw_stream_t stream);
int ivosw_per_update(float* tree, int n, void* per_state, const int64_t* idx, const float* td, int B, float alpha, float eps,
                     ivosw_stream_t stream);

/* One single-GPU training step of Agent.update_agent's loop (models/agent.py:128-160 minus the host coin of the target sync) as ONE
 * call and EIGHT launches: ivosw_replay_draw_gather + ivosw_dqn_loss_grad + ivosw_clamp_adam_dev with the minibatch draw and gather
 * folded into the encoder launch and the split-K slab reduction folded into clamp + Adam.  Same arithmetic, same orders of summation:
 * parameters, Adam state, gradient arena, loss, idx_out / state / new_state / action_out / reward_*_out and both device counters end
 * up bit-identical to the three separate calls.  `policy` is updated in place.  (When a tunable takes the step off the fused launch
 * chain the entry runs the three calls itself.)                                                                                  */
int ivosw_dqn_step_drawn(float* policy, const float* target, const float* old_iou, const float* new_iou, const float* annotated,
                         const float* next_annotated, const int64_t* action, const float* reward_step, const float* reward_done,
                         void* draw_state, int n, int B, int T, float gamma, int64_t* idx_out, float* state, float* new_state,
                         int64_t* action_out, float* reward_step_out, float* reward_done_out, float* grads, float* loss, void* ws,
                         size_t ws_bytes, float* exp_avg, float* exp_avg_sq, void* adam_state, float lr, float beta1, float beta2,
                         float eps, float weight_decay, float clamp, float grad_scale, ivosw_stream_t stream);
/* The same step with the loss option of ivosw_dqn_loss_grad_ex (IVOSW_DQN_LOSS_MSE: the two-term MSE of models/agent.py:149-151;
 * IVOSW_DQN_LOSS_HUBER: loss = mean(h(e1)) + mean(h(e2)) with torch's huber_loss h and threshold huber_delta, dLoss/dQsa =
 * (clamp(e1,-delta,delta) + clamp(e2,-delta,delta)) / B).  A bad kind or delta is refused before anything is launched.            */
int ivosw_dqn_step_drawn_ex(float* policy, const float* target, const float* old_iou, const float* new_iou, const float* annotated,
                            const float* next_annotated, const int64_t* action, const float* reward_step, const float* reward_done,
                            void* draw_state, int n, int B, int T, float gamma, int loss_kind, float huber_delta, int64_t* idx_out,
                            float* state, float* new_state, int64_t* action_out, float* reward_step_out, float* reward_done_out,
                            float* grads, float* loss, void* ws, size_t ws_bytes, float* exp_avg, float* exp_avg_sq, void* adam_state,
                            float lr, float beta1, float beta2, float eps, float weight_decay, float clamp, float grad_scale,
                            ivosw_stream_t stream);
/* The same step with clamp + SGD (ivosw_clamp_sgd) in place of clamp + Adam: the arguments of ivosw_dqn_step_drawn_ex up to ws_bytes,
 * then momentum_buf and SGD's hyper-parameters.  Eight launches, the last one clamp + SGD with the slab reduction folded in; parameters,
 * momentum buffer, gradient arena, loss, the minibatch outputs and the draw counter end up bit-identical to ivosw_replay_draw_gather +
 * ivosw_dqn_loss_grad_ex + ivosw_clamp_sgd, which the entry runs itself when a tunable takes the step off the fused chain.  A bad loss
 * option or SGD hyper-parameter is refused before anything is launched (the draw counter does not move).                            */
int ivosw_dqn_step_drawn_sgd(float* policy, const float* target, const float* old_iou, const float* new_iou, const float* annotated,
                             const float* next_annotated, const int64_t* action, const float* reward_step, const float* reward_done,
                             void* draw_state, int n, int B, int T, float gamma, int loss_kind, float huber_delta, int64_t* idx_out,
                             float* state, float* new_state, int64_t* action_out, float* reward_step_out, float* reward_done_out,
                             float* grads, float* loss, void* ws, size_t ws_bytes, float* momentum_buf, float lr, float momentum,
                             float weight_decay, int nesterov, float clamp, float grad_scale, ivosw_stream_t stream);
/* The one-call steps on the poly schedule (see ivosw_clamp_adam_dev_sched): ivosw_dqn_step_drawn_ex / ivosw_dqn_step_drawn_sgd with
 * (lr_table, lr_steps) in place of lr (and sgd_state after momentum_buf).  The same eight launches, the last one the scheduled clamp +
 * Adam / SGD with the slab reduction folded in; bit-identical to ivosw_replay_draw_gather + ivosw_dqn_loss_grad_ex +
 * ivosw_clamp_{adam,sgd}_dev_sched, which they run themselves off the fused chain.                                                    */
int ivosw_dqn_step_drawn_sched(float* policy, const float* target, const float* old_iou, const float* new_iou, const float* annotated,
                               const float* next_annotated, const int64_t* action, const float* reward_step, const float* reward_done,
                               void* draw_state, int n, int B, int T, float gamma, int loss_kind, float huber_delta, int64_t* idx_out,
                               float* state, float* new_state, int64_t* action_out, float* reward_step_out, float* reward_done_out,
                               float* grads, float* loss, void* ws, size_t ws_bytes, float* exp_avg, float* exp_avg_sq, void* adam_state,
                               const float* lr_table, int lr_steps, float beta1, float beta2, float eps, float weight_decay, float clamp,
                               float grad_scale, ivosw_stream_t stream);
int ivosw_dqn_step_drawn_sgd_sched(float* policy, const float* target, const float* old_iou, const float* new_iou, const float* annotated,
                                   const float* next_annotated, const int64_t* action, const float* reward_step, const float* reward_done,
                                   void* draw_state, int n, int B, int T, float gamma, int loss_kind, float huber_delta, int64_t* idx_out,
                                   float* state, float* new_state, int64_t* action_out, float* reward_step_out, float* reward_done_out,
                                   float* grads, float* loss, void* ws, size_t ws_bytes, float* momentum_buf, void* sgd_state,
                                   const float* lr_table, int lr_steps, float momentum, float weight_decay, int nesterov, float clamp,
                                   float grad_scale, ivosw_stream_t stream);
/* The one-call step of either optimizer with the target-network rule (ivosw_target_update) fused into its last launch: the same eight
 * launches as ivosw_dqn_step_drawn_{ex,sgd,sched,sgd_sched}, the thread that produces a new policy element also writes the target
 * element, so `target` is written here.  optimizer = IVOSW_OPT_ADAM: opt_buf0 / opt_buf1 = exp_avg / exp_avg_sq, opt_state = the Adam
 * state, beta1 / beta2 / eps are read.  IVOSW_OPT_SGD: opt_buf0 = the momentum buffer (opt_buf1 unused), momentum / nesterov are read,
 * opt_state = the SGD state on the schedule (unused otherwise).  lr_table NULL: the constant `lr`; otherwise the poly table of
 * lr_steps + 1 entries (see ivosw_clamp_adam_dev_sched; `lr` unused).  Bit-identical to the corresponding entry above followed by
 * ivosw_target_update, which is what it runs off the fused chain.  Refuses what those entries and ivosw_target_update refuse, and an
 * unknown optimizer, before anything is launched.                                                                                     */
#define IVOSW_OPT_ADAM 0
#define IVOSW_OPT_SGD 1
int ivosw_dqn_step_drawn_tgt(float* policy, float* target, const float* old_iou, const float* new_iou, const float* annotated,
                             const float* next_annotated, const int64_t* action, const float* reward_step, const float* reward_done,
                             void* draw_state, int n, int B, int T, float gamma, int loss_kind, float huber_delta, int64_t* idx_out,
                             float* state, float* new_state, int64_t* action_out, float* reward_step_out, float* reward_done_out,
                             float* grads, float* loss, void* ws, size_t ws_bytes, int optimizer, float* opt_buf0, float* opt_buf1,
                             void* opt_state, float lr, const float* lr_table, int lr_steps, float beta1, float beta2, float eps,
                             float momentum, int nesterov, float weight_decay, float clamp, float grad_scale, int target_mode, float tau,
                             int target_period, void* target_state, ivosw_stream_t stream);

/* ------------------------------------------------------------------ assessment front end ------ */
/* Replaces (tp>0.5) + AssessNet.all2yxhw(scale=1.5) (models/assessment.py:165-166,110-161) with no D2H:
 * tp [B,H,W] fp32 -> yxhw [B,4] fp32 (y,x,h,w).  scratch: B*4 int32.                              */
int ivosw_mask_bbox(const float* tp, int B, int H, int W, float* yxhw, int32_t* scratch,
                    ivosw_stream_t stream);
/* Replaces get_ROI_grid + 2x F.grid_sample + the (f-mean)/std of Encoder.forward
 * (models/assessment.py:75-108,173-174,47): tf [B,3,H,W], tp [B,H,W] fp32 NCHW, yxhw [B,4] ->
 * roi [B,256,256,4] NHWC (R,G,B normalised, P raw) in `dtype`.                                    */
int ivosw_roi_sample(const float* tf, const float* tp, const float* yxhw, int B, int H, int W,
                     int dtype, void* roi, ivosw_stream_t stream);

/* 8-bit frames.  RGBX8 is the device format of a decoded video: uint8 [n,H,W,4], bytes 0..2 = R, G, B, byte 3 written as 0 and never
 * read, base 4-byte aligned.  The colour value of byte v is float32(v) / float32(255), correctly rounded (np.float32(v) / 255., torch's
 * uint8 -> float() / 255); everything behind that conversion is the fp32 entries' arithmetic in the same order, so each _u8 entry is
 * bit-identical to its fp32 counterpart run on float32(u8) / 255, in every dtype.  A quarter of the bytes of fp32 frames on the device
 * and over PCIe, and half the sampler's gathers (one 8-byte load brings both x taps of all three colours).
 * ivosw_frames_pack_u8: one pass, once per video, from a decoder layout to RGBX8: src = IVOSW_U8_HWC3 [n,H,W,3] (cv2 / PIL after the
 *   channel flip) or IVOSW_U8_CHW3 [n,3,H,W], device memory; rgbx [n,H,W,4].  16-byte stores when src is 4-byte and rgbx 16-byte
 *   aligned (and, for CHW, H*W % 4 == 0); any other alignment takes the per-pixel path.  Needs n, H, W >= 1.
 * ivosw_roi_sample_u8: ivosw_roi_sample with rgbx [B,H,W,4] in place of tf.
 * Refused (IVOSW_ERR_ARG) before anything is launched: a NULL pointer, an rgbx that is not 4-byte aligned, an unknown layout, and the
 * size limits of the fp32 entries (H, W > 1 for the sampler).  No device allocation; capture-safe like the fp32 entries.              */
#define IVOSW_U8_HWC3 0
#define IVOSW_U8_CHW3 1
int ivosw_frames_pack_u8(const uint8_t* src, int layout, int n, int H, int W, uint8_t* rgbx, ivosw_stream_t stream);
int ivosw_roi_sample_u8(const uint8_t* rgbx, const float* tp, const float* yxhw, int B, int H, int W,
                        int dtype, void* roi, ivosw_stream_t stream);

/* ------------------------------------------------------------------ assessment network -------- */
/* Packed weights (BN folded in fp32, K-major repack, stem conv1|conv1_p concatenated along Cin).
 * `tensors` is a HOST array of 326 DEVICE pointers, one per entry of AssessNet.state_dict() in
 * state_dict order (models/assessment.py:12-71 + torchvision ResNet-50); fp32
 * tensors as stored, num_batches_tracked entries are ignored (may be NULL).                       */
#define IVOSW_ASSESS_NTENSORS 326
size_t ivosw_assess_packed_bytes(int dtype);
int ivosw_assess_pack(void* packed, int dtype, const void* const* tensors, int ntensors,
                      ivosw_stream_t stream);
/* Replaces AssessNet.forward (models/assessment.py:164-182): tf [B,3,H,W], tp [B,H,W] fp32 ->
 * scores [B] fp32.  Frames are processed in chunks of `chunk` frames at res2, doubling per stage
 * (<=0: library default, 256 bf16 / 128 fp32 modes); the chunk bounds the workspace (ivosw_assess_ws_bytes).
 * tap_stage/tap_out (debug, tests): 0 = none; 1 roi[.,256,256,4] 2 stem[.,128,128,64] 3 pool[.,64,64,64]
 * 4..7 res2..res5 outputs, NHWC in `dtype`; 8 pooled [.,2048] fp32.  Only with B <= chunk.        */
size_t ivosw_assess_ws_bytes(int dtype, int B, int H, int W, int chunk);
/* 1 when ivosw_assess_forward(dtype, B, chunk) runs the batch as two independent halves on two streams (bf16, default chunk,
 * B >= 64, tunables STREAMS2 / STREAMS2_MIN; the workspace query above already covers both halves), else 0.  Scores do not depend on it. */
int ivosw_assess_split(int dtype, int B, int chunk);
/* What ivosw_assess_forward(dtype, B, chunk, tap_stage) would enqueue between the ROI sampler and the pooling head, as text and
 * without a device (no HIP call): one line "slot kernel frames direction" per launch, in enqueue order - slot = 0 the caller's stream,
 * 1 the side stream of a split call (taken whenever ivosw_assess_split says so); kernel = the function name a kernel trace prints,
 * cut at '<' ("bneck_wide" stands for whichever single-block kernel of bottleneck_wide.hip runs); frames in the launch; direction =
 * 1 for descending tile order.  The same selection code as the forward pass, under the tunables in force.  buf [cap] receives the
 * NUL-terminated text; IVOSW_ERR_WS (the message names the size) if it does not fit.                                          */
int ivosw_assess_describe(int dtype, int B, int chunk, int tap_stage, char* buf, size_t cap);
int ivosw_assess_forward(const void* packed, int dtype, const float* tf, const float* tp,
                         int B, int H, int W, float* scores, void* ws, size_t ws_bytes, int chunk,
                         int tap_stage, void* tap_out, ivosw_stream_t stream);
/* The same forward for the O objects of ONE n-frame video without replicating the frames (recommend_frame scores one object
 * at a time on the same all_F, utils/utils_agent.py:118-119): tf [n_frames,3,H,W]; unit u = obj * n_frames + frame reads
 * frame u % n_frames and the mask plane at masks + obj * mask_stride_obj + frame * mask_stride_frame (strides in elements;
 * for the reference's all_P [n,O+1,H,W]: masks = all_P + H*W, stride_frame = (O+1)*H*W, stride_obj = H*W).
 * scores [n_obj * n_frames] fp32, object-major.  Workspace: ivosw_assess_ws_bytes with B = n_obj * n_frames.            */
int ivosw_assess_forward_objects(const void* packed, int dtype, const float* tf, int n_frames, const float* masks,
                                 long mask_stride_frame, long mask_stride_obj, int n_obj, int H, int W, float* scores,
                                 void* ws, size_t ws_bytes, int chunk, ivosw_stream_t stream);
/* ivosw_assess_forward / ivosw_assess_forward_objects on RGBX8 frames (see ivosw_frames_pack_u8): rgbx [B,H,W,4] / [n_frames,H,W,4] in
 * place of tf, everything else - chunking, the two-stream split, taps, the workspace of ivosw_assess_ws_bytes, the refusals - unchanged,
 * plus the refusal of an rgbx that is not 4-byte aligned.  Scores and taps are bit-identical to the fp32 entries on float32(u8) / 255. */
int ivosw_assess_forward_u8(const void* packed, int dtype, const uint8_t* rgbx, const float* tp,
                            int B, int H, int W, float* scores, void* ws, size_t ws_bytes, int chunk,
                            int tap_stage, void* tap_out, ivosw_stream_t stream);
int ivosw_assess_forward_objects_u8(const void* packed, int dtype, const uint8_t* rgbx, int n_frames, const float* masks,
                                    long mask_stride_frame, long mask_stride_obj, int n_obj, int H, int W, float* scores,
                                    void* ws, size_t ws_bytes, int chunk, ivosw_stream_t stream);
/* ivosw_assess_forward[_u8] with the pooled features handed out: features [B,2048] fp32 = the 8 x 8 average pool of res5, the rows fc1
 * is applied to (scores[u] = features[u] . fc1.weight + fc1.bias, by the pooling head's own summation) - what ivosw_head_fit fits on.
 * The arguments of the forward entries without tap_stage / tap_out.  Any B and any chunk, the two-stream split included: the pooling
 * head of every chunk group stores its rows at features + first unit * 2048 itself, so there is no workspace copy and no extra
 * launch; scores and features are bit for bit the forward entry's scores and its tap 8 wherever that tap exists (B <= chunk).  The
 * existing entries enqueue exactly what they did.  Refused as the forward entries refuse, plus a NULL features.                      */
int ivosw_assess_forward_features(const void* packed, int dtype, const float* tf, const float* tp, int B, int H, int W,
                                  float* scores, float* features, void* ws, size_t ws_bytes, int chunk, ivosw_stream_t stream);
int ivosw_assess_forward_features_u8(const void* packed, int dtype, const uint8_t* rgbx, const float* tp, int B, int H, int W,
                                     float* scores, float* features, void* ws, size_t ws_bytes, int chunk, ivosw_stream_t stream);
/* Several videos in ONE pass: the front end reads every unit through a table of per-video descriptors, the tower behind it sees 256 x 256
 * tiles and does not care where one came from, so K sessions fill one full-size pass instead of K small ones.
 * `videos` is a HOST array of n_videos (1 .. IVOSW_MAX_VIDEOS) descriptors with DEVICE pointers; it is read during the call only and
 * travels to the kernels inside their arguments (no allocation, no copy: capture-safe like the entries above).  Per video: frames
 * (fp32 planes or RGBX8, see frames_kind), masks and the two mask strides exactly as ivosw_assess_forward_objects takes them, n_frames,
 * n_obj, H, W - each video its own.
 * UNIT ORDER: video-major, then object-major inside a video: u = first_unit[v] + obj * n_frames[v] + frame, with first_unit[v] = the
 * sum of n_frames * n_obj over the videos before v.  scores / yxhw / roi rows are in unit order.
 * Per unit the arithmetic is that of the single-video entries, operation for operation: results are bit-identical to running
 * ivosw_mask_bbox / ivosw_roi_sample(_u8) / ivosw_assess_forward_objects(_u8) per video and concatenating.
 * ivosw_assess_videos_units: host only; the total number of units, or < 0 (IVOSW_ERR_ARG) if the array would be refused.
 * ivosw_mask_bbox_videos: yxhw [units,4]; scratch units * 4 int32.   ivosw_roi_sample_videos: roi [units,256,256,4] in `dtype`.
 * ivosw_assess_forward_videos: scores [units]; chunking, the two-stream split and the taps (B = units <= chunk) as in
 * ivosw_assess_forward - a chunk or a stream half may begin and end inside a video.  Workspace: ivosw_assess_ws_bytes with B = units;
 * that query does not look at H and W beyond their sign (the workspace holds 256 x 256 tiles and tower activations only), so any
 * positive H, W serves for a mixed-size call.
 * Refused (IVOSW_ERR_ARG) before anything is launched, the message names the video's index: a NULL pointer, n_videos outside
 * [1, IVOSW_MAX_VIDEOS], an unknown frames_kind or dtype, n_frames or n_obj < 1, H or W <= 1, H * W > INT_MAX, a negative stride,
 * overlapping consecutive mask planes (mask_stride_frame < H * W with n_frames > 1), an RGBX8 pointer that is not 4-byte aligned,
 * 2^30 or more units in total, an arena packed for another dtype.                                                                     */
#define IVOSW_MAX_VIDEOS 32
#define IVOSW_FRAMES_F32 0      /* float32 [n_frames,3,H,W] in 0..1 */
#define IVOSW_FRAMES_RGBX8 1    /* uint8 [n_frames,H,W,4], 4-byte aligned (ivosw_frames_pack_u8) */
typedef struct ivosw_video {
    const void* frames;                          /* device */
    const float* masks;                          /* device */
    long mask_stride_frame, mask_stride_obj;     /* elements, as in ivosw_assess_forward_objects */
    int frames_kind, n_frames, n_obj, H, W;
} ivosw_video_t;
long ivosw_assess_videos_units(const ivosw_video_t* videos, int n_videos);
int ivosw_mask_bbox_videos(const ivosw_video_t* videos, int n_videos, float* yxhw, int32_t* scratch, ivosw_stream_t stream);
int ivosw_roi_sample_videos(const ivosw_video_t* videos, int n_videos, const float* yxhw, int dtype, void* roi,
                            ivosw_stream_t stream);
int ivosw_assess_forward_videos(const void* packed, int dtype, const ivosw_video_t* videos, int n_videos, float* scores,
                                void* ws, size_t ws_bytes, int chunk, int tap_stage, void* tap_out, ivosw_stream_t stream);
/* Incremental assessment: re-score only the (frame, object) units whose mask planes changed since the session was last scored.
 * `videos` is the descriptor array of ivosw_assess_forward_videos - the same unit order, the same refusals.
 * ivosw_mask_delta_videos compares every unit's plane with the session's copy of the planes it was last scored on and brings that copy
 * up to date.  cache[v] (DEVICE buffer, 4-byte aligned; dense [n_obj][n_frames][H*W] fp32, unit order inside the video) and cold[v] are
 * HOST arrays of n_videos entries, read during the call only (the pointers travel in the kernel arguments like the table).  A unit is
 * DIRTY when any 32-bit pattern of its plane differs from the cached plane - compared as integers: +0 against -0 is dirty, a NaN with the
 * same bits is clean; clean means the tower would see the same bits.  cold[v] != 0: the cache content is undefined, every unit of v is
 * dirty and its planes are copied without comparing.  On return (stream order) cache[v] equals the planes bit for bit; only elements
 * (16-byte vectors on the vector path) that differ are stored, so an unchanged session writes nothing.  flags: [units] int32 scratch
 * (zeroed by the call's own init launch).  unit_ids [units] int32: entries [0, *n_dirty) are the dirty units in ascending order, the rest
 * is unspecified; n_dirty: one int32 on the device.  Three launches (init, compare, compaction), no allocation, no atomics:
 * capture-safe and deterministic.  16-byte loads when the video's planes allow them (H * W % 4 == 0, 16-byte aligned masks and strides)
 * and cache[v] is 16-byte aligned; else the scalar path.
 * ivosw_mask_bbox_units / ivosw_roi_sample_units / ivosw_assess_forward_units: the *_videos entries over a unit LIST.  unit_ids is a
 * DEVICE array of n_ids units of the table (what ivosw_mask_delta_videos wrote); row i of yxhw [n_ids,4] / roi [n_ids,256,256,4]
 * belongs to unit unit_ids[i]; scratch n_ids * 4 int32.  Per unit the arithmetic is that of the *_videos entries, operation for operation.
 * ivosw_assess_forward_units: `scores` is the session's FULL [units] table; only scores[unit_ids[i]] is written.  Chunking and the
 * two-stream split work on list positions (B = n_ids).  Workspace: ivosw_assess_units_ws_bytes(dtype, n_ids, chunk) (0 for n_ids <= 0).
 * n_ids == 0 returns IVOSW_OK and launches nothing.  Refused before any launch: what the *_videos entries refuse, n_ids < 0, n_ids above
 * the table's units, a NULL list with n_ids > 0.  A row whose id lies outside [0, units) is skipped (an all-zero yxhw row / roi tile, no
 * score stored): no address is ever formed from such an id.                                                                            */
int ivosw_mask_delta_videos(const ivosw_video_t* videos, int n_videos, float* const* cache, const int* cold,
                            int32_t* flags, int32_t* unit_ids, int32_t* n_dirty, ivosw_stream_t stream);
int ivosw_mask_bbox_units(const ivosw_video_t* videos, int n_videos, const int32_t* unit_ids, int n_ids, float* yxhw,
                          int32_t* scratch, ivosw_stream_t stream);
int ivosw_roi_sample_units(const ivosw_video_t* videos, int n_videos, const int32_t* unit_ids, int n_ids, const float* yxhw,
                           int dtype, void* roi, ivosw_stream_t stream);
size_t ivosw_assess_units_ws_bytes(int dtype, int n_ids, int chunk);
int ivosw_assess_forward_units(const void* packed, int dtype, const ivosw_video_t* videos, int n_videos, const int32_t* unit_ids,
                               int n_ids, float* scores, void* ws, size_t ws_bytes, int chunk, ivosw_stream_t stream);
/* Label-map masks: a video's masks as ONE hard label map, uint8 [n_frames,H,W] (row-major planes, stride_frame elements between frames) -
 * what ivosw_seg_epilogue writes as label_u8 and ivosw_jf_counts reads - in place of n_obj float planes: 1 byte per pixel and frame
 * instead of 4 * (n_obj + 1).  Object obj (0-based, obj < n_obj <= 255) owns the value obj + 1; 0 and values above n_obj belong to no
 * object.  The mask plane of unit (frame, obj) is, by definition, tp[y,x] = (map[frame,y,x] == obj + 1) ? 1.0f : 0.0f, and every _lab
 * entry computes exactly what its plain twin computes on those planes, operation for operation: boxes, tiles, scores and dirty lists are
 * bit-identical.  (The bbox test tp > 0.5f becomes byte == obj + 1; the sampler turns its four byte taps into 1.0f / 0.0f before the same
 * tap selection, weights and FMA chain.)
 * `labels` is a HOST array of n_videos entries, read during the call only; it travels in the kernel arguments like the table (no
 * allocation, no copy: capture-safe).  labels[v].map != NULL: video v's masks come from the map, videos[v].masks and its two strides are
 * not looked at (the pointer may be NULL).  labels[v].map == NULL: video v is a float video exactly as in the plain entry - one call may
 * mix float and label videos, fp32 and RGBX8 frames.  labels == NULL: the plain entry.  Unit order, chunking, the two-stream split, taps,
 * the workspaces (ivosw_assess_ws_bytes, ivosw_assess_units_ws_bytes) and every refusal of the plain entries are unchanged.  Refused in
 * addition, before any launch, the message names the video: n_obj > 255 on a label video, a negative stride_frame, stride_frame < H * W
 * with n_frames > 1 (overlapping frames), a float video with NULL masks.
 * The scan reads 16 pixels per lane and load when H * W % 16 == 0 and the map's base and stride_frame are 16-byte aligned, else byte by
 * byte.  A call without a label video launches the kernels of the plain entry.
 * ivosw_mask_delta_videos_lab: cache[v] of a label video is a dense uint8 [n_frames][H*W] copy of the map (any alignment; 16-byte aligned
 * for the vector path), of a float video the fp32 planes as in ivosw_mask_delta_videos.  A cold label video marks every unit dirty and
 * copies the map; otherwise every pixel whose byte differs (cached a, now b) flags the units (frame, a - 1) and (frame, b - 1) whose labels
 * lie in 1 .. n_obj - the planes that pixel changed in - and only differing bytes (16-byte vectors on the vector path) are stored: an
 * unchanged session writes nothing.  One compare pass per FRAME (2 bytes read per pixel) instead of one per unit (8 bytes per pixel and
 * unit); a call that mixes float and label videos runs two compare launches.  flags, unit_ids and n_dirty as in the plain entry.       */
typedef struct ivosw_labels {
    const uint8_t* map;                          /* device; NULL: a float video */
    long stride_frame;                           /* elements */
} ivosw_labels_t;
int ivosw_mask_bbox_videos_lab(const ivosw_video_t* videos, const ivosw_labels_t* labels, int n_videos, float* yxhw, int32_t* scratch,
                               ivosw_stream_t stream);
int ivosw_roi_sample_videos_lab(const ivosw_video_t* videos, const ivosw_labels_t* labels, int n_videos, const float* yxhw, int dtype,
                                void* roi, ivosw_stream_t stream);
int ivosw_assess_forward_videos_lab(const void* packed, int dtype, const ivosw_video_t* videos, const ivosw_labels_t* labels,
                                    int n_videos, float* scores, void* ws, size_t ws_bytes, int chunk, int tap_stage, void* tap_out,
                                    ivosw_stream_t stream);
int ivosw_mask_delta_videos_lab(const ivosw_video_t* videos, const ivosw_labels_t* labels, int n_videos, void* const* cache,
                                const int* cold, int32_t* flags, int32_t* unit_ids, int32_t* n_dirty, ivosw_stream_t stream);
int ivosw_mask_bbox_units_lab(const ivosw_video_t* videos, const ivosw_labels_t* labels, int n_videos, const int32_t* unit_ids,
                              int n_ids, float* yxhw, int32_t* scratch, ivosw_stream_t stream);
int ivosw_roi_sample_units_lab(const ivosw_video_t* videos, const ivosw_labels_t* labels, int n_videos, const int32_t* unit_ids,
                               int n_ids, const float* yxhw, int dtype, void* roi, ivosw_stream_t stream);
int ivosw_assess_forward_units_lab(const void* packed, int dtype, const ivosw_video_t* videos, const ivosw_labels_t* labels,
                                   int n_videos, const int32_t* unit_ids, int n_ids, float* scores, void* ws, size_t ws_bytes,
                                   int chunk, ivosw_stream_t stream);
/* Replaces `mask_quality[:] = pred.mean(1); state = np.stack([mask_quality, counts], 1)` (utils/utils_agent.py:120-121) on
 * the device: scores [n_obj][n_frames] fp32 (as ivosw_assess_forward_objects writes them), counts [n_frames] fp32 ->
 * quality [n_frames] float64 (numpy's float64 mean of the float32 predictions, same summation order) and
 * state [n_frames,2] fp32 = (float32(quality), counts), the Brain's input.                                              */
int ivosw_quality_state(const float* scores, int n_obj, int n_frames, const float* counts, double* quality,
                        float* state, ivosw_stream_t stream);
/* ivosw_quality_state for n_seqs (1 .. IVOSW_MAX_SEQS) videos in ONE launch: `scores` is the flat score buffer of
 * ivosw_assess_forward_videos (unit order: video k's [n_obj[k]][lengths[k]] block starts at the sum of n_obj * lengths over the videos
 * before it), counts [R], quality [R] and state [R,2] are flat over the videos, R = sum of lengths.  n_obj and lengths are HOST arrays
 * (they travel inside the kernel's arguments).  Per video the float64 summation order is ivosw_quality_state's: results are bit-identical.
 * Refused (IVOSW_ERR_ARG) before the launch, naming the video's index: what ivosw_brain_ragged_rows refuses, and an n_obj < 1.       */
int ivosw_quality_state_ragged(const float* scores, const int* n_obj, const int* lengths, int n_seqs,
                               const float* counts, double* quality, float* state, ivosw_stream_t stream);
/* Kernel-name patterns of the dominant kernel family (the tower's contraction kernels) for profiling. */
const char* ivosw_assess_dominant_kernel(int dtype);

/* ------------------------------------------------------------------ J / F metrics - */
/* Replaces davisinteractive.metrics.batched_jaccard / batched_f_measure as utils/misc.py:136-160
 * (sequence_metric) calls them.  gt, pred: device uint8 label maps [N,H,W]; obj_ids: HOST array of the
 * n_obj (<= 32) label values to score; bound_pix = the F-measure tolerance in pixels, as the reference
 * derives it (bound_th if >= 1 else ceil(bound_th * |(H,W)|_2), bound_th = 0.008; <= 32).  Writes the six
 * INTEGER counts per (frame, object) to the device array counts [N][n_obj][6] =
 *   { |gt & pred|, |gt | pred|, #pred-boundary, #gt-boundary, #pred-boundary within dil(gt-boundary),
 *     #gt-boundary within dil(pred-boundary) };
 * the host forms J and F from them with the reference's float64 expressions (ivos_w_amd/metrics.py).    */
size_t ivosw_jf_ws_bytes(int N, int H, int W, int n_obj);
int ivosw_jf_counts(const uint8_t* gt, const uint8_t* pred, int N, int H, int W, const uint8_t* obj_ids,
                    int n_obj, int bound_pix, int64_t* counts, void* ws, size_t ws_bytes, ivosw_stream_t stream);
/* ivosw_jf_counts for several videos in ONE pass: one memset, one boundary launch and one match launch whatever their number.
 * `videos` is a HOST array of n_videos (1 .. IVOSW_MAX_JF_VIDEOS) descriptors with DEVICE label maps; it is read during the call only
 * and travels to the kernels inside their arguments (no allocation, no copy: capture-safe).  Per video: gt, pred uint8
 * [n_frames,H,W], the n_obj (1 .. 32) label values to score in obj_ids, and bound_pix (0 .. 32) - each video its own; the disk's half
 * widths are derived from bound_pix inside the kernel.  The frame / (frame, object) grid dimension runs flat over the videos, the row,
 * column and word dimensions are sized by the largest video; a workgroup beyond its own video's extent returns before it forms an address.
 * counts is flat and video-major: video v's [n_frames][n_obj][6] block follows those of the videos before it.  Per video the six
 * integers equal those of ivosw_jf_counts on that video alone, exactly.  Workspace: ivosw_jf_videos_ws_bytes(videos, n_videos) = the sum
 * of ivosw_jf_ws_bytes over the videos (0 if the array would be refused), owned by the caller.
 * Refused (IVOSW_ERR_ARG) before anything is launched, the message names the video's index: a NULL pointer, n_videos outside
 * [1, IVOSW_MAX_JF_VIDEOS], n_frames, H or W < 1, n_obj outside 1 .. 32, bound_pix outside 0 .. 32, H * ceil(W / 32) > 2^30, more than
 * 65535 frames in total (the boundary kernel's flat grid dimension) or more than 65535 (frame, object) pairs in total (the match
 * kernel's): the message says which, and the caller splits the group.  A short workspace: IVOSW_ERR_WS.                              */
#define IVOSW_MAX_JF_VIDEOS 32
typedef struct ivosw_jf_video {
    const uint8_t* gt;                           /* device */
    const uint8_t* pred;                         /* device */
    int n_frames, H, W, n_obj;
    uint8_t obj_ids[32];
    int bound_pix;
} ivosw_jf_video_t;
size_t ivosw_jf_videos_ws_bytes(const ivosw_jf_video_t* videos, int n_videos);
int ivosw_jf_counts_videos(const ivosw_jf_video_t* videos, int n_videos, int64_t* counts, void* ws, size_t ws_bytes,
                           ivosw_stream_t stream);
/* The last step of J / F on the device: the float64 ratios and their per-frame mean over the objects for n_seqs (1 .. IVOSW_MAX_SEQS)
 * videos in ONE launch, from the flat counts ivosw_jf_counts_videos (or ivosw_jf_counts per video, concatenated) wrote.  n_obj and
 * lengths are HOST arrays (they travel inside the kernel's arguments); R = the sum of lengths.
 * Per (frame, object), in float64 with every operation rounded by itself (no FMA contraction), the expressions of
 * ivos_w_amd/metrics.py: J = 1 when the union is 0, else inter / union; precision / recall = 1 / 0, 0 / 1, 1 / 1 when the pred
 * boundary, the gt boundary or both are empty, else matched / total; F = 0 when precision + recall == 0, else
 * ((2 * precision) * recall) / (precision + recall).  Per frame the mean over the objects is numpy's ndarray.mean(axis=1) on a
 * C-contiguous float64 [N,O] array: its pairwise summation order along the row (sequential below 8 objects) and one division by O.
 * IVOSW_METRIC_J_AND_F is .5 * mean(J) + .5 * mean(F).
 * quality [R] float64.  per_obj (nullable) [sum of n_obj * lengths] float64, flat in the order of counts: the un-averaged values (J,
 * F, or .5 * J + .5 * F).  state (nullable together with annot_counts [R] fp32) [R,2] fp32 = (float32(quality), annot_counts): the
 * Brain's input.  No atomics, no workspace; capture-safe.
 * Refused (IVOSW_ERR_ARG) before the launch, naming the video's index: what ivosw_brain_ragged_rows refuses, an n_obj outside
 * 1 .. 32, a metric outside the enum, a NULL counts / n_obj / lengths / quality, state without annot_counts or the reverse.          */
#define IVOSW_METRIC_J 0
#define IVOSW_METRIC_F 1
#define IVOSW_METRIC_J_AND_F 2
int ivosw_jf_reduce_ragged(const int64_t* counts, const int* n_obj, const int* lengths, int n_seqs, int metric,
                           const float* annot_counts, double* per_obj, double* quality, float* state, ivosw_stream_t stream);

/* ------------------------------------------------------------------ assessment samples: 8-bit prob maps, per-unit J&F targets - */
/* Replaces the two host steps by which the reference builds AssessNet's training samples and their targets: save_seg_preds
 * (utils/misc.py:165-181: all_P to the host as float32, cv2.imwrite(path, probs[i, n] * 255) per object plane) and the target /
 * loss / diff loop of quality_assessment.py:178-196, 235-263.
 *
 * ivosw_qa_quantize: all_P (fp32, device) -> planes uint8 [n_obj][n_frames][H][W], object-major, objects 1 .. n_obj only: element
 * (f, c, y, x) is read at probs[f * probs_stride_n + c * probs_stride_c + y * W + x] for c = 1 .. n_obj (strides in elements, as
 * ivosw_seg_epilogue's: (n_obj + 1) * H * W, H * W for the reference's [n, O+1, H, W]; H * W, n_total * H * W for an object-major
 * store); channel 0 is never read.  The rule is the definition: q = clamp(rint(fl32(p * 255.0f)), 0, 255) - one fp32 product, round
 * half to even, NaN -> 0, -inf -> 0, +inf -> 255.  It restates numpy's float32 `probs * 255` followed by OpenCV's saturating 8-bit
 * conversion (cvRound, then the clamp); OpenCV is not part of this project's environment, so parity with cv2 is restated, not recorded.
 * One streaming pass: no LDS, no atomics, no scratch, no allocation; capture-safe.  Four pixels per lane (16-byte load, 4-byte store)
 * when H * W % 4 == 0, both strides % 4 == 0, probs is 16-byte and planes 4-byte aligned; one pixel per lane otherwise and with
 * IVOSW_QA_SCALAR in the environment; both agree bit for bit.
 * Refused (IVOSW_ERR_ARG) before the launch: a NULL pointer, n_frames or n_obj outside 1 .. 65535, H or W < 1, H * W >= 2^31, a stride
 * below H * W.                                                                                                                       */
int ivosw_qa_quantize(const float* probs, int n_frames, int n_obj, int H, int W, long probs_stride_n, long probs_stride_c,
                      uint8_t* planes, ivosw_stream_t stream);
/* The six integer counts of ivosw_jf_counts_videos with the prediction read from byte planes instead of a label map: one memset and two
 * launches for up to IVOSW_MAX_JF_VIDEOS videos.  Per video: gt uint8 [n_frames,H,W] (label map), planes uint8 [n_obj][n_frames][H][W]
 * (what ivosw_qa_quantize writes), obj_ids, thr, bound_pix.  For unit (object o, frame f): gt mask = (gt[f] == obj_ids[o]), pred mask =
 * (planes[o][f] >= thr) - the planes of different objects may overlap, which no label map can express.  thr = 205 is the reference's
 * rule: byte / 255 > 0.8 first holds at 205, in float64 and in float32.  counts: video-major, [n_frames][n_obj][6] per video, as
 * ivosw_jf_counts_videos writes them; for planes that do not overlap they equal its counts on the equivalent label map.  Workspace:
 * ivosw_qa_counts_ws_bytes (0 if the array would be refused).  The same kernel bodies as the label-map pass; capture-safe.
 * Refused before anything is launched, the message names the video: what ivosw_jf_counts_videos refuses, and a NULL planes.          */
typedef struct ivosw_qa_video {
    const uint8_t* gt;                           /* device */
    const uint8_t* planes;                       /* device */
    int n_frames, H, W, n_obj;
    uint8_t obj_ids[32];
    int bound_pix;
    uint8_t thr;
} ivosw_qa_video_t;
size_t ivosw_qa_counts_ws_bytes(const ivosw_qa_video_t* videos, int n_videos);
int ivosw_qa_counts_videos(const ivosw_qa_video_t* videos, int n_videos, int64_t* counts, void* ws, size_t ws_bytes,
                           ivosw_stream_t stream);
/* Per-unit targets from those counts, in ONE launch for n_seqs (1 .. IVOSW_MAX_SEQS) videos, in the ASSESSMENT's unit order - the order
 * of ivosw_assess_forward_videos' scores: u = first_unit[v] + obj * lengths[v] + frame, first_unit[v] = the sum of n_obj * lengths over
 * the videos before v - while counts are frame-major inside a video.  n_obj and lengths are HOST arrays (kernel arguments).
 *   target [units] float64: J, F or .5 * J + .5 * F of the unit, by ivosw_jf_reduce_ragged's expressions, not averaged over objects.
 *   valid  [units] uint8:   union > 0 (the reference skips a sample whose label and mask are both empty).
 * With scores (fp32 [units], nullable together with loss, diff, n_valid), per video: loss, diff fp32 [n_seqs] and n_valid int32
 * [n_seqs] = the reference loop exactly: t = float32(target); the terms (s - t) * (s - t) and |s - t| in fp32, each operation rounded
 * by itself; added sequentially in ascending unit order over the valid units, in fp32, from 0; one fp32 division by n_valid.  A video
 * without a valid unit: loss = diff = 0, n_valid = 0.  No atomics, no workspace; capture-safe.
 * Refused (IVOSW_ERR_ARG) before the launch, naming the video: what ivosw_jf_reduce_ragged refuses; a NULL target or valid; scores
 * without loss / diff / n_valid or the reverse.                                                                                      */
int ivosw_qa_targets(const int64_t* counts, const int* n_obj, const int* lengths, int n_seqs, int metric, const float* scores,
                     double* target, uint8_t* valid, float* loss, float* diff, int* n_valid, ivosw_stream_t stream);

/* ------------------------------------------------------------------ augmented assessment samples: one fused warp per batch ---- */
/* Replaces what an AssessNet training loop does to its samples on the host (datasets/transforms_assess.py: Resize, RandomAffine with
 * its retry loop, AdditiveNoise, RandomContrast, RandomHorizontalFlip, ToTensor and the upload): every sample (video v, frame f, object
 * o) of a batch is resampled through ONE inverse affine map from sources that already live on the device, at one output size Ho x Wo.
 *
 * videos: a HOST array of n_videos (1 .. IVOSW_MAX_JF_VIDEOS) descriptors with DEVICE pointers: frames (IVOSW_FRAMES_F32 [n,3,H,W] or
 * IVOSW_FRAMES_RGBX8 [n,H,W,4]), gt uint8 [n,H,W], planes uint8 [n_obj][n][H][W] (what ivosw_qa_quantize writes), obj_ids.
 * samples_host: a HOST array of n_samples rows, read during the call only: v, f, o (o indexes obj_ids), n_cand (0 ..
 * IVOSW_QA_AUG_MAX_CAND) candidate inverse maps and one post map of six fp32 each (a b c d e f), noise, contrast.  The rows travel in the
 * kernel arguments, a group of samples per launch (at most 64; as many as fit the 4 KB a launch carries), so the call allocates
 * nothing, copies nothing and is capture-safe.
 *
 * THE SAMPLING RULE (the definition; every fp32 operation is rounded by itself, no FMA contraction):
 *   coordinates  destination pixel (x, y), inverse map M:  sx = fl(fl(fl(a*x) + fl(b*y)) + c),  sy = fl(fl(fl(d*x) + fl(e*y)) + f).
 *                The full map of a candidate is post applied to (x, y) first, then the candidate; the call composes the two in
 *                float64 - a' = a*pa + b*pd, b' = a*pb + b*pe, c' = (a*pc + b*pf) + c, the second row likewise, each float64 operation
 *                rounded by itself - and rounds to fp32 once.  "No candidate" is post alone.
 *   bilinear     (img, prob)  x0 = floor(sx), fx = sx - x0, the same in y; taps (x0 | x0+1, y0 | y0+1); a tap outside the source reads
 *                0.0; top = v00 + fx * (v10 - v00), bot = v01 + fx * (v11 - v01), v = top + fy * (bot - top).  Integer translations,
 *                the flip and the identity therefore copy source values exactly.
 *   sources      fp32 frames as they are; an RGBX8 byte and a plane byte b as float32(b) / 255.0f, correctly rounded (the ROI
 *                sampler's conversion; equal to float32(float64(b) / 255) for all 256 bytes).
 *   nearest      (label)  tap (floor(sx + 0.5f), floor(sy + 0.5f)); outside the source 0, inside gt[tap] == obj_ids[o].
 *   photometric  (img only)  t = clip(fl(v + noise), 0, 1), out = clip(fl(t * contrast), 0, 1).
 *   mask         255 where prob > 0.8f, else 0 (on an unwarped plane: byte >= 205, metrics' QA_THRESHOLD).
 * Where a map's coordinates overflow fp32 (an infinite or NaN sx or sy) the values of that pixel are undefined.
 *
 * Candidate selection (RandomAffine's retry loop without a host round trip): a first launch finds, for every candidate and for "no
 * candidate", whether the nearest-warped label over the Ho x Wo grid holds a 0 and whether it holds a 1 - one workgroup per pair, two
 * flag bytes stored by one lane, no atomics - into the caller's workspace (ivosw_qa_augment_ws_bytes(n_samples); 0 for a refused
 * count; ws may be NULL when every n_cand is 0, and the launch is skipped then).  The warp launch takes, per sample, the first
 * candidate whose number of distinct label values equals that of "no candidate" - the reference's len(np.unique(segmap_aug)) ==
 * num_objs - else "no candidate", its fallback to the untransformed sample, and writes its index (n_cand for none) to chosen.
 *
 * Outputs (device): img fp32 [N,3,Ho,Wo], prob fp32 [N,Ho,Wo], label uint8 [N,Ho,Wo] (1 = the object), mask uint8 [N,Ho,Wo], chosen
 * int32 [N].  label with obj_ids = [1] and mask with thr = 205 are what ivosw_qa_counts_videos takes as a 1-object video of N frames.
 * One destination pixel per lane is the only path: four pixels of a row per lane with float4 stores were built and measured slower
 * (the taps are gathers; profiles/augment_probe.txt of the change that added this entry), so there is no vector variant and no switch.
 * Refused (IVOSW_ERR_ARG) before any launch, nothing written, the message names the argument or the sample: a NULL pointer; n_videos
 * outside 1 .. 32; n_samples < 1 (or above IVOSW_QA_AUG_MAX_SAMPLES); Ho or Wo outside 1 .. 65535; Ho * Wo >= 2^31; a video with
 * n_frames, H or W < 1, H or W > 2^24, H * W >= 2^31 or n_obj outside 1 .. 32; an unknown frames_kind; frames off the 4-byte grid; a sample whose v,
 * f or o is out of range; n_cand outside 0 .. 12; a non-finite map entry, noise or contrast; a workspace that is too small; an output
 * that overlaps a source or the workspace; a workspace that overlaps a source.                                                                                          */
#define IVOSW_QA_AUG_MAX_CAND 12
#define IVOSW_QA_AUG_MAX_SAMPLES (1 << 20)
typedef struct ivosw_qa_aug_video {
    const void* frames;                          /* device */
    const uint8_t* gt;                           /* device */
    const uint8_t* planes;                       /* device */
    int frames_kind;                             /* IVOSW_FRAMES_* */
    int n_frames, H, W, n_obj;
    uint8_t obj_ids[32];
} ivosw_qa_aug_video_t;
typedef struct ivosw_qa_aug_sample {
    int v, f, o, n_cand;
    float cand[IVOSW_QA_AUG_MAX_CAND][6];
    float post[6];
    float noise, contrast;
} ivosw_qa_aug_sample_t;
size_t ivosw_qa_augment_ws_bytes(int n_samples);
int ivosw_qa_augment(const ivosw_qa_aug_video_t* videos, int n_videos, const ivosw_qa_aug_sample_t* samples_host, int n_samples,
                     int Ho, int Wo, float* img, float* prob, uint8_t* label, uint8_t* mask, int32_t* chosen, void* ws,
                     size_t ws_bytes, ivosw_stream_t stream);

/* ------------------------------------------------------------------ AssessNet's score head fitted on the device ---- */
/* Replaces the reference's AssessNet optimiser loop (quality_assessment.py:230-270 and :286: the per-sample loss loop with its
 * `union[n] > 0` filter and `continue`, loss.backward(), param.grad.data.clamp_(-1, 1), torch.optim.SGD with momentum and weight
 * decay, ExponentialLR once per epoch) for the HEAD: fc1 (2048 -> 1) on the pooled features of a frozen trunk
 * (ivosw_assess_forward_features).  The trunk runs with folded BatchNorm here, so training it is not representable on this path.
 * ONE launch runs n_steps minibatch steps of n_fits (1 .. IVOSW_HEAD_FIT_MAX_FITS) independent fits, one workgroup per fit; the fits
 * share the feature bank and differ in their hyper-parameters, index tables and state.
 *   feat [M,2048] fp32, target [M] fp32, valid [M] uint8 (the reference's union[n] > 0)                                   device
 *   order int32 [n_fits, n_steps, B]: the row indices of every minibatch, drawn by the host as the DataLoader's shuffle with drop_last
 *         would; 1 <= B <= IVOSW_HEAD_FIT_MAX_BATCH.  An index outside [0, M) is the caller's error (not checked on the device).  device
 *   lr    fp32 [n_fits, n_steps]: the rate of every step (lr0 * gamma**epoch formed in float64 by the host, rounded once).      device
 *   momentum, weight_decay fp32 [n_fits], zero_grad, eval_only int [n_fits] (0 / 1): HOST arrays, they travel in the kernel arguments.
 *   in / out state, so that a call continues the previous one: w [n_fits,2048], b [n_fits], the momentum buffers buf_w, buf_b and
 *         the gradient accumulators grad_w, grad_b of the same shapes (fp32), steps_taken int32 [n_fits] (taken steps so far).   device
 *   log   fp32 [n_fits, n_steps, 3]: loss, diff, counter of every step.                                                          device
 *
 * THE STEP (the definition; every fp32 operation is rounded by itself, no FMA contraction; tests/head_fit_ref.py restates it).
 * For the rows n = 0 .. B-1 of the step, idx = order[fit, step, n], x = feat[idx]:
 *   dot      64 partial sums, lane l = 0 .. 63: a_l = 0, then for j = 0 .. 7, q = 0 .. 3 in this order, k = 256 j + 4 l + q:
 *            a_l = fl(a_l + fl(x[k] * w[k])); then for o = 32, 16, 8, 4, 2, 1: a_l = fl(a_l + a_(l xor o)) for all l at once.
 *   pred_n = fl(a_0 + b);  e_n = fl(pred_n - target[idx]) where valid[idx] != 0, else the row takes no part.
 *   c = the number of valid rows.  c == 0: the reference's `continue` - w, b, buffers, accumulators and steps_taken stay as they
 *            are, bit for bit, and the log row is (0, 0, 0).
 *   sums     over the valid rows in ascending n, each from 0.0f: S2 += fl(e_n * e_n), S1 += |e_n|, Se += e_n, and per channel k
 *            Sk += fl(e_n * x[k]).
 *   log      loss = fl(S2 / c), diff = fl(S1 / c), counter = c (as fp32).  eval_only: the step ends here.
 *   gradient g_w[k] = fl(fl(2 / c) * Sk), g_b = fl(fl(2 / c) * Se).
 *   clamp    G = fl((zero_grad ? 0.0f : G_prev) + g), then G = min(max(G, -1), 1), stored back CLAMPED: what
 *            param.grad.data.clamp_ leaves behind for the next backward() when zero_grad() is never called, as in the reference.
 *   SGD      d = fl(G + fl(weight_decay * p)); buf = d if steps_taken == 0 else fl(fl(momentum * buf) + d);
 *            p = fl(p - fl(lr * buf)); after all parameters: steps_taken += 1.
 * No global atomics, no cross-workgroup synchronisation, no fences, no scratch, no allocation (capture-safe).  Results are
 * bit-identical run to run, and a fit's results are the same bits alone or as any member of a 32-fit launch.
 * Refused (IVOSW_ERR_ARG) before anything touches the GPU: a NULL pointer, M < 1, n_fits outside 1 .. 32, B outside 1 .. 256,
 * n_steps < 1, n_fits * n_steps * B >= 2^31, feat off the 16-byte grid, w / buf_w / grad_w off the 8-byte grid, a NaN momentum or
 * weight_decay.                                                                                                                   */
#define IVOSW_HEAD_FIT_MAX_FITS 32
#define IVOSW_HEAD_FIT_MAX_BATCH 256
int ivosw_head_fit(const float* feat, const float* target, const uint8_t* valid, int M, const int32_t* order, const float* lr,
                   int n_fits, int n_steps, int B, const float* momentum, const float* weight_decay, const int* zero_grad,
                   const int* eval_only, float* w, float* b, float* buf_w, float* buf_b, float* grad_w, float* grad_b,
                   int32_t* steps_taken, float* log, ivosw_stream_t stream);

/* ------------------------------------------------------------------ segmentation epilogue (8f-4) */
/* Replaces, per frame batch, F.interpolate(logits, (H,W), 'bilinear', align_corners=True) -> argmax(dim=1)
 * [-> .float()] and the final torch.softmax(cat(probs), 1) of utils/utils_manet.py:78-84,110-116,146-151,
 * 160-161.  logits: device [n,C,hs,ws] fp32.  Outputs (each optional, at least one): probs, element
 * (f,c,y,x) written at probs[f*probs_stride_n + c*probs_stride_c + y*W + x] (strides in elements: pass
 * C*H*W, H*W for the reference's [n,C,H,W]; n_total*H*W as the channel stride stores all_P object-major);
 * label_i64 / label_u8 / label_f32 [n,H,W] = argmax over channels (first maximum).                    */
int ivosw_seg_epilogue(const float* logits, int n, int C, int hs, int ws, int H, int W, float* probs,
                       long probs_stride_n, long probs_stride_c, int64_t* label_i64, uint8_t* label_u8,
                       float* label_f32, ivosw_stream_t stream);

/* ------------------------------------------------------------------ ATNet epilogue (8f-4, ATNet) */
/* Replaces, for ONE frame t of run_VOS_singleiact (utils/utils_atnet.py), torch.sigmoid(output_logit)[:, 0], the blend
 * (alpha * prob) + ((1 - alpha) * prob_map_of_frames[t]) and the store into prob_map_of_frames[t] (:100-101,123-124,146-150), and
 * that frame's share of the end-of-interaction combine_masks_with_batch(...)[:, 0, hpad1:-hpad2, wpad1:-wpad2] and
 * torch.cat([zeros, prob_map], 1)[..., hpad1:-hpad2, wpad1:-wpad2] (:152-159).  One launch, one streaming pass, no allocation and no
 * copy (capture-safe).  ATNet propagates frame by frame - each frame's input is the previous frame's output - so a call is one frame.
 *   logits      [n_obj,PH,PW] fp32 on the padded grid, or NULL.
 *   prob_map_t  [n_obj,PH,PW] fp32: frame t of prob_map_of_frames, read and written IN PLACE.
 *   crop        the window rows hpad1 .. hpad1+H-1, columns wpad1 .. wpad1+W-1 of the padded grid.
 * Per padded pixel and object: s = sigmoid(logit) in fp32 (1 / (1 + expf(-x)), IEEE division: sigmoid(0) == 0.5f exactly, finite in
 * [0, 1] for every finite logit); p = blend ? fadd_rn(fmul_rn(alpha32, s), fmul_rn(beta32, old)) : s - three separately rounded
 * operations, never an FMA, as torch's three ops are; pass alpha32 = (float)alpha and beta32 = (float)(1 - alpha) with 1 - alpha formed in
 * double, which is what torch makes of a Python scalar.  logits == NULL: p = old, nothing is blended, prob_map_t and prob_pad are NOT
 * written - the mode that rebuilds a store slot and labels from an existing map (a resumed session, a frame the loop did not visit).
 * Label of a pixel: o* = the FIRST index of max_o p[o]; the label is o* + 1 if p[o*] > th (strictly), else 0.  This rule is the
 * definition: it restates combine_masks_with_batch(prob, n_obj, th) of the ATNet clone's libs/utils_torch.py, which is not part of the
 * reference tree - parity with the clone is unpinned.  NaN logits: unspecified.
 * Outputs, each optional:
 *   prob_map_t  p over the whole padded grid (whenever logits != NULL).
 *   prob_pad    [n_obj,PH,PW]: the UNBLENDED s - output_prob_anno / output_prob_prop, the next forward_TNet call's predmask_prev.
 *   probs       window only: p of object o at (y, x) goes to probs[o * probs_stride_c + y * W + x]; pass the address of channel 1,
 *               frame t of an object-major store and n_total * H * W as the stride (channel 0, the reference's bg_dummy zeros, is
 *               zeroed once when the store is made).
 *   label_u8 / label_f32  [H,W]: the label at [y * W + x].
 * 16-byte loads and stores on the padded planes when PW % 4 == 0 and logits, prob_map_t and prob_pad are 16-byte aligned; the window
 * outputs are shifted by wpad1 against the padded rows, so they go out as vectors only when wpad1 % 4 == 0, W % 4 == 0,
 * probs_stride_c % 4 == 0 and probs / label_f32 (16 bytes) and label_u8 (4 bytes) are aligned, else element by element beside vector
 * loads.  Everything else takes a scalar kernel (IVOSW_ATNET_SCALAR in the environment forces it); all paths agree bit for bit.
 * Refused (IVOSW_ERR_ARG) before any launch, nothing written: a NULL prob_map_t, n_obj < 1, n_obj > 255 with label_u8, H or W < 1,
 * hpad1 or wpad1 < 0, hpad1 + H > PH or wpad1 + W > PW, probs_stride_c < H * W with probs and n_obj > 1, PH * PW or n_obj * PH * PW >
 * INT_MAX, a blend that is not 0 / 1, blend with NULL logits, and a call with nothing to write (NULL logits and no probs, label_u8 or
 * label_f32).                                                                                                                       */
int ivosw_atnet_epilogue(const float* logits, float* prob_map_t, int n_obj, int PH, int PW, int hpad1, int wpad1, int H, int W,
                         int blend, float alpha32, float beta32, float th, float* prob_pad, float* probs, long probs_stride_c,
                         uint8_t* label_u8, float* label_f32, ivosw_stream_t stream);

/* ------------------------------------------------------------------ IPN glue (8f-4, IPN) */
/* The host code between the IPN clone's model.Run and the tensors the rest of the loop consumes (utils/utils_ipn.py), on the device.
 * Both entries are one streaming pass each, allocate nothing and copy nothing (capture-safe); IVOSW_IPN_SCALAR in the environment
 * forces their element-by-element kernels, which agree with the vector ones bit for bit.
 *
 * ivosw_ipn_dilate: the whole of Dilate_mask (:26-34) for n scribble maps [n,H,W] int8 (sparse, indexed, -1 = ignore) in ONE launch.
 *   out[y,x] = the largest o in 0 .. num_objects found among the pixels (y+dy, x+dx) with |dy| + |dx| <= 2 that lie inside the image,
 *   -1 if there is none; input values outside -1 .. num_objects count as -1.
 * This is what the reference's loop yields: two iterations of the 3x3 cross are the radius-2 diamond, cv2's default border never
 * contributes to a dilation, and the ascending object loop with overwrite is a maximum.  4-byte loads and stores (4 pixels of a row per
 * lane) when W % 4 == 0 and mask and out are 4-byte aligned, else element by element.
 * Refused (IVOSW_ERR_ARG) before any launch, nothing written: a NULL mask or out, n, H or W < 1, num_objects outside 0 .. 126,
 * H * W > INT_MAX, out == mask.                                                                                                       */
int ivosw_ipn_dilate(const int8_t* mask, int n, int H, int W, int num_objects, int8_t* out, ivosw_stream_t stream);

/* ivosw_ipn_merge: one interaction's end for the whole session - the merge of the new estimate with the earlier rounds' by the
 * Get_weight weights (:37-72), To_np_label (:75-81) and all_P (eval_agent_ipn.py:261).
 *   all_E, prev_E  [K,T,H,W] fp32 on the device: IPN's 1,o,t,h,w without the batch axis, K = objects + background.
 *   w_new32, w_old32  HOST arrays of length T, read during the call; they travel inside the kernel arguments, in launches of at most 256
 *                  frames each.  Pass (float)w and (float)(1 - w) with 1 - w formed in double: what torch makes of Python scalars.
 *   index          HOST int[K], a permutation of 0 .. K-1, NULL = identity: index[j] is the canonical channel held at position j, so
 *                  canonical channel i is read from position inv[i].
 * With prev_E: e = fadd_rn(fmul_rn(w_new32[f], all_E), fmul_rn(w_old32[f], prev_E)) - three separately rounded operations, never an FMA,
 * on EVERY frame, those with weight 1 included - written back to all_E in place.  With prev_E == NULL nothing is blended, all_E is not
 * written and the weights may be NULL.  This blend rule is the definition: IPN's model.Run lives in the external clone, not in the
 * reference tree, so parity with the clone's own merge is unpinned.
 * Outputs, each optional:
 *   probs          canonical channel i of frame f goes to probs[i * probs_stride_c + f * H * W + p] (an object-major store).  Pass NULL
 *                  when index is the identity: all_E itself is then the store.
 *   label_u8 / label_f32  [T,H,W]: the FIRST maximum over i = 0 .. K-1 of the merged estimate, as numpy's argmax gives it: a NaN is the
 *                  maximum, and the first NaN wins; -0.0 and 0.0 tie.
 * 16-byte loads and stores when H * W % 4 == 0 and all_E, prev_E, probs, probs_stride_c and label_f32 are on the 16-byte grid (label_u8
 * on the 4-byte grid), else element by element.
 * Refused (IVOSW_ERR_ARG) before any launch, nothing written: a NULL all_E, K outside 1 .. 32 (and K > 256 with label_u8), T, H or W < 1,
 * H * W > INT_MAX or K * T * H * W > 2^40 (offsets are long; nothing larger is addressed), an index that is not a permutation, prev_E
 * without both weight arrays, probs overlapping all_E, probs_stride_c < T * H * W (or (K - 1) * probs_stride_c + T * H * W > 2^40) with
 * K > 1, and a call with nothing to write (no prev_E, probs, label_u8 or label_f32).                                                    */
int ivosw_ipn_merge(float* all_E, const float* prev_E, int K, int T, int H, int W, const float* w_new32, const float* w_old32,
                    const int* index, float* probs, long probs_stride_c, uint8_t* label_u8, float* label_f32, ivosw_stream_t stream);

/* ------------------------------------------------------------------ session overlays (8f-4, IPN) */
/* The pictures an annotator is shown - a frame with the current mask drawn on it - for the frames of ONE video, on the device.
 * Reference (utils/utils_ipn.py, each on one uint8 image and one binary mask, on the CPU in float64 and through
 * scipy.ndimage.binary_dilation): overlay_davis (:113-128), checkerboard / BIG_BOARD (:131-143), overlay_checker (:146-157),
 * overlay_color (:160-171), overlay_fade (:174-190).  Each style below is what the reference function yields on the binary mask, bit
 * for bit on uint8 images.
 *   frames     device: IVOSW_FRAMES_RGBX8 uint8 [n_frames,H,W,4] (4-byte aligned) or IVOSW_FRAMES_F32 float32 [n_frames,3,H,W].  The image
 *              byte of a float is rintf(f * 255.0f) clamped to 0 .. 255, a NaN giving 0: on u8 / 255 floats that is u8 again, so the
 *              two kinds give identical pictures.
 *   labels     device uint8 [n_frames,H,W]: value i + 1 is object i; 0 and values above n_objects are no object.
 *   frame_ids  HOST int[n_ids]: the frames to render, in any order, repeats allowed; NULL = all frames in order (n_ids is then not
 *              read).  The ids travel inside the kernel arguments, in launches of at most 256 pictures each.  m = the list's length.
 *   out        device: IVOSW_OUT_RGB8 uint8 [m,H,W,3] (the numpy / encoder image) or IVOSW_OUT_RGBX8 uint8 [m,H,W,4] (4-byte aligned, byte
 *              3 written 0).  It must not overlap frames or labels.
 *   opt        HOST, read during the call.  select picks the binary mask: o in 1 .. n_objects is (label == o), 0 is
 *              (1 <= label <= n_objects).  A pixel is on the CONTOUR of a mask when it is not in it and one of its four edge neighbours
 *              inside the image is (binary_dilation(mask) ^ mask, scipy's default cross, border_value = 0).
 *     IVOSW_OVERLAY_DAVIS    select = o: overlay_davis(image, label == o, rgb = palette[o - 1], alpha = alpha): inside, each channel is
 *                            (uint8) trunc(double(v) * alpha + k), k = (1.0 * (1 - alpha)) * double(c) formed on the host, the product and
 *                            the sum rounded separately; contour pixels are 0.  select = 0: that function applied once per object, in
 *                            ascending object order, to the running image - so a pixel of object 2 next to object 1 ends as
 *                            trunc(0 * alpha + k2) and a pixel of object 1 next to object 2 ends as 0.
 *     IVOSW_OVERLAY_FADE     outside the mask each channel is (uint8) trunc(0.4 * double(v)); contour pixels are (0, 255, 255).
 *     IVOSW_OVERLAY_CHECKER  outside the mask the board: 223 where (y / 20 + x / 20) is even, 32 where it is odd (BIG_BOARD).  The
 *                            reference raises above 1000 pixels a side; here the pattern simply continues.
 *     IVOSW_OVERLAY_COLOR    outside the mask opt->color (the reference's default is (255, 0, 255)).
 *                            (FADE, CHECKER and COLOR keep the image inside the mask; alpha and palette are read by DAVIS only.)
 * One streaming pass, asynchronous on `stream`, on the device that owns the buffers; allocates nothing, copies nothing (capture-safe).
 * Four pixels of a row per lane (one 16-byte RGBX8 load or three float4 plane loads, label words of the rows above, at and below, 12
 * or 16 bytes stored) when W % 4 == 0, labels and an RGB8 out are on the 4-byte grid, frames and an RGBX8 out on the 16-byte grid;
 * two pixels per lane (8-byte loads, 2-byte label words, 6 or 8 bytes stored) when that holds with 2, 2 and 8 in place of 4, 4 and
 * 16 - the case of W = 854, the width of DAVIS 480p; otherwise pixel by pixel (IVOSW_OVERLAY_SCALAR in the environment forces that).
 * All paths agree bit for bit.  ivosw_overlay_lane_pixels: host only; the pixels per lane (4, 2 or 1) of the kernel that a call with
 * these buffers runs.
 * Refused (IVOSW_ERR_ARG) before any launch, nothing written, the message says which check failed: a NULL frames, labels, opt or out,
 * an unknown frames_kind, out_kind or style, n_frames, H or W < 1, H * W > INT_MAX, n_objects outside 1 .. 32, select outside
 * 0 .. n_objects, alpha not in [0, 1] (a NaN included), a list of length < 1, a frame id outside [0, n_frames) (the message names its
 * position), frames or an RGBX8 out off the 4-byte grid, more than 2^40 pixels of pictures or of frames, out overlapping frames or
 * labels.                                                                                                                           */
#define IVOSW_OUT_RGB8 0
#define IVOSW_OUT_RGBX8 1
#define IVOSW_OVERLAY_DAVIS 0
#define IVOSW_OVERLAY_FADE 1
#define IVOSW_OVERLAY_CHECKER 2
#define IVOSW_OVERLAY_COLOR 3
typedef struct ivosw_overlay {
    int style;                                   /* IVOSW_OVERLAY_* */
    int n_objects;                               /* 1 .. 32 */
    int select;                                  /* 0 = every object, o = object o alone */
    double alpha;                                /* DAVIS: the image's share inside an object, in [0, 1] */
    uint8_t palette[32][3];                      /* DAVIS: the colour of object i + 1 */
    uint8_t color[3];                            /* COLOR: the colour outside the mask */
} ivosw_overlay_t;
int ivosw_overlay_lane_pixels(const void* frames, const uint8_t* labels, int W, const void* out, int out_kind);
int ivosw_overlay_frames(const void* frames, int frames_kind, const uint8_t* labels, int n_frames, int H, int W,
                         const int* frame_ids, int n_ids, const ivosw_overlay_t* opt, void* out, int out_kind, ivosw_stream_t stream);

/* ------------------------------------------------------------------ scribbles (8f-4, the input side) */
/* The scribbles an annotator (or the robot) has just drawn, as label maps on the device: what eval_agent_manet.py:368-374 builds with
 * davisinteractive's scribbles2mask, ToTensor and rough_ROI, and eval_agent_ipn.py with scribbles2mask and Dilate_mask.
 * scribbles2mask is not in the reference tree: the rules below are this project's DEFINITION (tests/scribble_ref.py), parity with the
 * library's own rasteriser is unpinned.  rough_ROI (utils/utils_manet.py:22-39) is in the tree and is kept bit for bit.
 *
 * Packing (the caller's, on the host; utils/scribbles.py): for a map of (H, W) a path point (x, y) in [0, 1]^2 becomes the pixel
 *   px = min((int)(x * W), W - 1), py = min((int)(y * H), H - 1), the products in double and truncated.  The kernels see integers only.
 * Line rule: consecutive points of a path are joined, the path is not closed.  For (x0,y0) -> (x1,y1): dx = |x1 - x0|, dy = |y1 - y0|,
 *   the signs are +1 if the difference is > 0, else -1.  x drives if dx > dy, otherwise (dx == dy included) y drives.  With the driving
 *   length a and the minor length b:   D = 2b - a; m = 0;  for s in 0 .. a: plot(driving = s, minor = m); if D >= 0: m += 1, D -= 2a;
 *   D += 2b.   The kernel uses the closed form m(s) = (2 b s + a) / (2 a) for a > 0 (the same pixels; tests/test_scribble_option.py
 *   compares them for all b <= a <= 64).  A one-point path plots that pixel, a zero-length segment one pixel; with bresenham == 0 only
 *   the points themselves are plotted.
 * Order: within a map the paths are drawn in table order, a later path overwrites an earlier one; untouched pixels hold default_value.
 * rough_ROI with distance d, per map / image: the box (hmin, hmax, wmin, wmax) is that of the pixels != -1 (a NaN counts as != -1); rows
 *   [max(hmin - d, 0), min(hmax + d, h - 1)) x columns [max(wmin - d, 0), min(wmax + d, w - 1)) keep their value, every other pixel
 *   becomes 0.  Both ends are exclusive: a scribble on the last row or column loses that row or column, as in the reference.  One
 *   difference: a map without such a pixel raises in the reference (torch.min of an empty tensor); here it comes out all 0, with no
 *   synchronisation.
 *
 * ivosw_scribble_raster:
 *   points      device int32 [n_points,2] = (px, py).
 *   paths       device int32 [n_paths,4] = {first point, number of points, object id, map index}.
 *   paths_host  a HOST copy of the same table, read during the call (as `lengths` is by the ragged entries): the table is validated
 *               from it before anything is launched.  The point ranges ascend and do not overlap (first[k] >= first[k-1] + n[k-1]):
 *               the draw kernel finds the path of a point by a binary search.  Points no path owns are ignored.
 *   out_i8      device int8 [n_maps,H,W], out_f32 device float32 [n_maps,H,W] with the same values (what MANet takes); either may be
 *               NULL, not both.
 *   roi_dist    < 0: off; >= 0: the rough_ROI rule with that distance applied to every map in the finalise pass.
 *   ws          caller-owned, ivosw_scribble_raster_ws_bytes(n_maps, H, W) bytes on the 16-byte grid (0 = the shape would be refused).
 * One memset (a uint32 key plane and four box integers per map), one draw launch (a wave per point, its lanes over the steps of the
 * segment that starts there: atomicMax of path index + 1 into the key plane - the highest path index on a pixel is the last
 * assignment, so the result does not depend on the schedule - and four atomicMax into the map's box), one finalise launch
 * (key ? object[key - 1] : default_value, the ROI, 16-byte stores when out_i8 and out_f32 are on the 16-byte grid, else and for the
 * last partial group element by element; IVOSW_SCRIBBLE_SCALAR in the environment forces that).  A segment with an end point outside
 * the map is not drawn.  Asynchronous on `stream`; allocates nothing, synchronises nothing (capture-safe).
 * Refused (IVOSW_ERR_ARG) before anything is launched, nothing written, the message names the argument: a NULL ws, a NULL points, paths
 * or paths_host with n_paths > 0, both outputs NULL, n_maps, H or W < 1, n_maps * H * W > INT_MAX, n_paths < 0 (0 is legal: every map
 * comes out at its default), n_points < 0, default_value outside int8, a ws off the 16-byte grid, and a path (the message names its
 * index) whose point range is empty, leaves [0, n_points) or does not lie behind the previous path's, whose object id is outside
 * [0, 126] or whose map index is outside [0, n_maps).  A short workspace: IVOSW_ERR_WS.
 *
 * ivosw_rough_roi: the stand-alone drop-in body on float32 [b,1,h,w] (out may be in): a memset of ws (ivosw_rough_roi_ws_bytes(b)), a
 * box scan (wave reductions, four atomics per wave into ws) and a fill (float4 when in and out are on the 16-byte grid), two launches.
 * Refused (IVOSW_ERR_ARG): a NULL in, out or ws, b, h or w < 1, b > 65535, b * h * w > INT_MAX, dist < 0.  A short ws: IVOSW_ERR_WS. */
size_t ivosw_scribble_raster_ws_bytes(int n_maps, int H, int W);
int ivosw_scribble_raster(const int32_t* points, int n_points, const int32_t* paths, const int32_t* paths_host, int n_paths,
                          int n_maps, int H, int W, int default_value, int bresenham, int roi_dist, int8_t* out_i8, float* out_f32,
                          void* ws, size_t ws_bytes, ivosw_stream_t stream);
size_t ivosw_rough_roi_ws_bytes(int b);
int ivosw_rough_roi(const float* in, float* out, int b, int h, int w, int dist, void* ws, size_t ws_bytes, ivosw_stream_t stream);

/* ------------------------------------------------------------------ scribble robot (8f-4, the annotator's side) */
/* The skeleton of the region where a prediction misses an object: what davisinteractive's scribble robot builds on the CPU at every
 * interaction (a skeletonisation of the error mask, then paths along it; produce_reward.py:133 sets its min_nb_nodes).  The robot is not
 * in the reference tree and neither davisinteractive nor skimage is a dependency: the rule below is this project's DEFINITION
 * (tests/robot_ref.py restates it per pixel), parity with the library's own skeletoniser is restated, not recorded.
 *
 * A unit is one (frame, object) pair.  Error plane: pixel (y, x) is set iff gt[frame][y][x] == object && pred[frame][y][x] != object; a
 *   NULL pred is all background (the first interaction: the error region is the object itself).
 * Thinning: Zhang and Suen, "A fast parallel algorithm for thinning digital patterns" (1984), as published.  The neighbours of P1 are named
 *   clockwise from north: P2 = N, P3 = NE, P4 = E, P5 = SE, P6 = S, P7 = SW, P8 = W, P9 = NW; everything outside the image is 0.
 *   B = the number of set neighbours, A = the number of 0 -> 1 steps around the cycle P2, P3, .., P9, P2.  A pixel is deleted iff it is
 *   set, 2 <= B <= 6, A == 1 and, in sub-iteration 1, P2 * P4 * P6 == 0 and P4 * P6 * P8 == 0; in sub-iteration 2, P2 * P4 * P8 == 0 and
 *   P2 * P6 * P8 == 0.  Every decision of a sub-iteration reads the plane as it was before that sub-iteration.  An iteration is
 *   sub-iteration 1, then 2; iterations run until one deletes nothing, at most max(H, W) of them.  iters = the number of iterations
 *   that deleted a pixel (an empty plane: 0), or -1 when the max(H, W)-th iteration still deleted one.  The algorithm's known artefacts
 *   stay: an isolated 2 x 2 block is deleted whole, a single pixel is kept.
 *
 * ivosw_robot_skeleton:
 *   gt, pred    device uint8 [n,H,W] label maps; pred may be NULL.
 *   units_host  a HOST int32 [m,2] = (frame, object), read during the call (as `lengths` is by the ragged entries): the table travels
 *               inside the kernel arguments, 64 units per launch, a longer list in groups of 64.
 *   points      device int32 [m,cap]: the skeleton pixels of unit k as (y << 16) | x in ascending raster order; nothing is written at or
 *               beyond cap.
 *   counts      device int32 [m]: the TRUE number of skeleton pixels, also when it exceeds cap.
 *   iters       device int32 [m].
 *   skel        NULL, or device uint32 [m,H,ceil(W/32)]: the skeleton's bit plane, bit (x & 31) of word (x >> 5) of row y; bits at
 *               x >= W are 0.
 * One workgroup of 1024 threads per unit thins the plane entirely in LDS (two bit planes, ping and pong; 32 pixels per lane and step
 * with word logic; no global pass, no atomics on global memory).  Asynchronous on `stream`; allocates nothing, copies nothing,
 * synchronises nothing (capture-safe).
 * Size limit: 2 * H * ceil(W/32) * 4 bytes + 256 must fit in the 160 KB of LDS of one gfx950 workgroup; ivosw_robot_skeleton_fits(H, W)
 * (host only) returns 1 if a size fits, else 0.  480 x 854 (DAVIS 480p: 103 936 bytes) fits, 720 x 1280 (230 656 bytes) does not: the
 * robot serves 480p.
 * Refused (IVOSW_ERR_ARG) before anything is launched, nothing written, the message names the argument: a NULL gt, units_host, points,
 * counts or iters, n < 1, m < 1, cap < 1, H or W outside [1, 65535], a size that does not fit (the message names H, W and the limit), a
 * unit (the message names its index) whose frame is outside [0, n) or whose object is outside [1, 255].                             */
int ivosw_robot_skeleton_fits(int H, int W);
int ivosw_robot_skeleton(const uint8_t* gt, const uint8_t* pred, int n, int H, int W, const int32_t* units_host, int m, int cap,
                         int32_t* points, int32_t* counts, int32_t* iters, uint32_t* skel, ivosw_stream_t stream);

/* ivosw_robot_skeleton_box: the same outputs by the same rule for ANY frame size in [1, 65535]^2 and for objects in [0, 255].
 * Windowing rule: the kernel first finds the bounding box of the unit's error region - rows by0 .. by1, 32-pixel words bw0 .. bw1 - and
 *   keeps two bit planes of that box only ((by1 - by0 + 1) x (bw1 - bw0 + 1) words), thinning them with everything outside the WINDOW read
 *   as 0.  The result is bit-identical to the full-frame rule: thinning only clears bits, so every pixel outside the box is 0 at the start
 *   and at every later sub-iteration; a decision inside the box therefore reads the same eight neighbours in both forms (a neighbour
 *   outside the box is 0 in the full plane and "outside" in the window), by induction over the sub-iterations the planes agree inside
 *   the box, the same sub-iterations delete something, and iters is the same (its cap stays max(H, W) of the FRAME).  points, counts,
 *   iters and skel are in frame coordinates (skel is written in full, 0 outside the box); a caller cannot tell that the window existed.
 *   An empty region: counts = 0, iters = 0, skel all zero, no point written.
 * Where the planes live, per unit: if 2 * box words * 4 + 256 bytes fit the launch's dynamic LDS - min(2 * H * ceil(W/32) * 4 + 256,
 *   160 KB), so a size ivosw_robot_skeleton accepts never needs more - in LDS; otherwise in the unit's slice of `workspace`, device
 *   memory of ivosw_robot_box_workspace_bytes(H, W, m) = m * 2 * H * ceil(W/32) * 4 bytes, 4-byte aligned, owned by the caller, content
 *   irrelevant before and undefined after.  That query (host only) returns 0 when ivosw_robot_skeleton_fits(H, W) - workspace may then be
 *   NULL - and a negative value for H or W outside [1, 65535] or m < 1.  Still one launch per 64 units, one workgroup per unit, no host
 *   loop, no grid-wide synchronisation, no atomics on global memory; asynchronous on `stream`, capture-safe.
 * Object 0 (the background) is a unit like any other: its plane is gt == 0 && pred != 0, the false positives.  A NULL pred means "nothing
 *   predicted", which has no false positive: a table that holds object 0 is refused when pred is NULL (the message names the unit).
 * Refused (IVOSW_ERR_ARG) before any pointer is used, nothing launched, nothing written: everything ivosw_robot_skeleton refuses except
 *   the size limit and object 0 (objects outside [0, 255]); object 0 with a NULL pred; a size that does not fit with a NULL workspace
 *   or workspace_bytes below the need (the message states the bytes needed).                                                     */
long ivosw_robot_box_workspace_bytes(int H, int W, int m);
int ivosw_robot_skeleton_box(const uint8_t* gt, const uint8_t* pred, int n, int H, int W, const int32_t* units_host, int m, int cap,
                             int32_t* points, int32_t* counts, int32_t* iters, uint32_t* skel, uint32_t* workspace,
                             size_t workspace_bytes, ivosw_stream_t stream);

/* ------------------------------------------------------------------ robot paths (the skeleton's pixels become node lists) */
/* ivosw_robot_paths: the paths the robot draws along a skeleton, on the device, from the outputs of ivosw_robot_skeleton[_box] as they
 * are.  The rule is tests/robot_ref.py's path step (components, bfs, farthest, longest_path, longest_paths, resample) and, level by
 * level, tests/robot_paths_ref.py; the result is bit for bit that of the restatement.  It is this project's DEFINITION.
 *
 * Nodes: the first counts[k] entries of points[k], decoded as UNSIGNED (y << 16) | x, in ascending raster order; node index = position.
 * Components: 8-connected.  A component's first pixel is its lowest node; components of fewer than min_nb_nodes nodes are dropped.
 * Directions: N, NE, E, SE, S, SW, W, NW = (dy, dx) (-1,0) (-1,1) (0,1) (1,1) (1,0) (1,-1) (0,-1) (-1,-1), numbered 0 .. 7.
 * BFS from a source s, stated without an order of execution: dist is the graph distance from s.  The queue holds s at position 0; the
 *   nodes of level d + 1 follow those of level d.  parent[q] is the neighbour of q at distance dist[q] - 1 that stands FIRST in the queue;
 *   the nodes of level d + 1 stand in ascending order of (queue position of parent, direction parent -> q).  This is the order in which a
 *   FIFO that visits every node's neighbours in the direction order appends them, and the parents it records.
 * Farthest node: the highest dist; a tie goes to the lower node index.
 * Path of a component: BFS from its first pixel gives the farthest node a; BFS from a gives the farthest node b; the path is a, ..., b
 *   with every node the parent of the next in the SECOND BFS.  len = dist[b] + 1.
 * Selection: the max_paths longest paths, longest first; a tie goes to the component with the lower first pixel.
 * Resampling, nb_points > 0: n = min(nb_points, len).  The kept positions are rint(fl64(i * fl64((len - 1) / (n - 1)))) for i < n - 1 and
 *   len - 1 for i = n - 1 (n == 1: position 0), in float64 with round-half-to-even; a position equal to its predecessor is dropped
 *   (np.linspace(0, len - 1, n).round() followed by np.unique).  nb_points <= 0 keeps every node.
 *
 *   points, counts  device int32 [m,cap] and [m], as written by ivosw_robot_skeleton[_box] (counts[k] <= 0 reads as an empty unit).
 *   H, W            the map size the points lie on (checked only: the points carry their coordinates).
 *   nodes           device int32 [m,max_paths,slot,2] = (px, py): ivosw_scribble_raster's point format, 8-byte aligned.  Slot r of unit k holds the nodes of
 *                   its r-th path; behind the path's last node the slot REPEATS that node up to `slot` entries.  A slot without a path,
 *                   every slot of a unit with status 1 and the offending slot under status 2 hold (-1, -1) throughout.
 *   lens            device int32 [m,max_paths]: the nodes of path r of unit k after resampling; 0 = no such path (also under status 1
 *                   and for the offending slot under status 2).
 *   status          device int32 [m]: 0 ok; 1 counts[k] > cap (the skeleton was truncated: no path is given); 2 a path longer than slot
 *                   (only with nb_points <= 0; the unit's other paths are given).
 * With that layout the static host table {(k * max_paths + r) * slot, slot, object_k, map} is valid for ivosw_scribble_raster as it
 * stands: a repeated node is a zero-length segment, which plots the same pixel under the same path index, and a segment with an end point
 * outside the map - (-1, -1) - is not drawn.
 * One workgroup per unit, 64 units per launch, a longer list in groups; every table lives in LDS (36 bytes per node of cap + 256), which
 * bounds cap: ivosw_robot_paths_max_cap() (host only) returns the largest cap whose tables fit the 160 KB of one gfx950 workgroup
 * (4544).  No global atomics, nothing allocated, nothing copied, asynchronous on `stream`, capture-safe.
 * Refused (IVOSW_ERR_ARG) before anything is launched, nothing written, the message names the argument: a NULL points, counts, nodes,
 * lens or status, nodes off the 8-byte grid, m < 1, cap outside [1, ivosw_robot_paths_max_cap()], H or W outside [1, 65535], min_nb_nodes < 1, max_paths outside
 * [1, 8], slot outside [1, cap], nb_points > slot.                                                                                  */
int ivosw_robot_paths_max_cap(void);
int ivosw_robot_paths(const int32_t* points, const int32_t* counts, int m, int cap, int H, int W, int min_nb_nodes, int max_paths,
                      int nb_points, int slot, int32_t* nodes, int32_t* lens, int32_t* status, ivosw_stream_t stream);

/* ------------------------------------------------------------------ launch-sequence capture ---- */
/* HIP-graph capture of any sequence of the calls above on one stream (not in the reference: it replaces the ~40 host
 * launches per Agent.update_agent step, models/agent.py:128-160, by ONE hipGraphLaunch).  begin puts `stream` (non-null)
 * into capture; every ivosw_* call made on it until end is recorded instead of executed; end instantiates the graph and
 * reports its kernel-node count.  All device pointers passed during capture must stay valid for the life of the handle;
 * per-step scalars that change (Adam's step) live on the device (ivosw_clamp_adam_dev).  The handle is a host object.  */
typedef void* ivosw_graph_t;
int ivosw_graph_begin(ivosw_stream_t stream);
int ivosw_graph_end(ivosw_stream_t stream, ivosw_graph_t* out, int* kernel_nodes);
int ivosw_graph_launch(ivosw_graph_t g, ivosw_stream_t stream);
int ivosw_graph_destroy(ivosw_graph_t g);

/* ------------------------------------------------------------------ measurement hooks ---------- */
/* Not part of the reference surface: bench.py's roofline leg.  Between start and stop every launch of
 * the dominant kernel family (conv_igemm*, conv1x1_wide*, conv3x3_patch*, bneck*, stem_pool*) is bracketed by hipEvents on the launch stream; stop
 * synchronises those events and returns the summed kernel time (ms) and the launch count.          */
int ivosw_profile_start(void);
/* Span mode (what bench.py's `roofline` uses, inside the timed region): ONE event pair around each uninterrupted run of
 * tower launches (stem .. the last res5 kernel of a pass; the ROI sampler and the pool+fc kernel are outside).  stop
 * synchronises the events and returns the summed span time (ms), the number of spans and of family launches in them. */
int ivosw_profile_span_start(void);
int ivosw_profile_span_stop(double* total_ms, int* spans, int* launches);
int ivosw_profile_stop(double* total_ms, int* launches);
/* Text table (one line per distinct conv layer shape: calls, avg us, TFLOP/s, GB/s) of the launches recorded
 * since ivosw_profile_start; call before ivosw_profile_stop.  buf is a HOST buffer of `cap` bytes.       */
int ivosw_profile_report(char* buf, size_t cap);
/* Tuning/test hook: override a named integer tunable (otherwise read from the environment variable
 * IVOSW_TUNE_<KEY>).  Keys: FUSE (1 = whole-bottleneck fused kernels in bf16 mode, 0 = layer by layer), WS, NK. */
int ivosw_tune_set(const char* key, int value);
/* 1 when the library was built with -DIVOSW_ABLATION=1 (the ablation switches IVOSW_DEBUG_CONV / BDBG are compiled in and can
 * skip MFMAs, loads or stores); the default build returns 0 and contains none of them.  bench.py refuses to run on 1.   */
int ivosw_ablation_build(void);
/* Profiling aid (bench.py roofline.sclk_mhz): one wave spins for spin_us of wall time and writes {shader cycles, 100 MHz wall
 * ticks} of that interval to out2 (2 x uint64, device): launched on a side stream beside the measured work, cycles / ticks x 100 MHz
 * is the shader clock the chip ran at under that load.                                                                       */
int ivosw_clock_probe(unsigned long long* out2, int spin_us, ivosw_stream_t stream);

/* The forward entry points refuse an arena packed for another dtype.  The tag of an arena is known to this process when it packed the
 * arena itself, or from the arena's own 4-byte device tag read on the first forward call that sees the address.  Call this when the
 * memory behind `packed` is freed or re-filled (device copy) with an arena of another precision, so that the cached tag is dropped. */
int ivosw_assess_forget(const void* packed);

/* The tuning probes (single-kernel launches with phase stamps, micro-benchmark kernels) are not part of this ABI: include/ivosw_probe.h,
 * libivosw_probe.so.                                                                                                              */

#ifdef __cplusplus
}
#endif
#endif /* IVOSW_H */
