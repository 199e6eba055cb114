/* Tuning probes of libivosw — NOT part of the product ABI (include/ivosw.h, libivosw_hip.so).
 *
 * libivosw_probe.so is a superset build of the same sources with -DIVOSW_PROBES: every entry of ivosw.h plus the entries below -
 * single-kernel launches with s_memtime phase stamps, the micro-benchmark contraction of round 5 and the single-launch entries of the per-kernel
 * tests.  tools/ and the per-kernel GPU tests load it;
 * nothing a reference maintainer binds lives here.                                                                               */
#ifndef IVOSW_PROBE_H
#define IVOSW_PROBE_H
#include "ivosw.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Tuning probe: the fused Brain forwards that follow stamp s_memtime at four points (step start, MFMAs done, state update
 * done, barrier passed) of recurrence step T/2 (slots 0-3) and at kernel entry / weights in registers / last step done (4-6),
 * per workgroup, into ts [workgroups,8] uint64 (device); NULL = off.                                                     */
int ivosw_lstm_probe(unsigned long long* ts, unsigned long long* ts_bwd);   /* ts_bwd: the same for the BPTT kernel of ivosw_dqn_loss_grad */
/* Tuning probe: ONE fused bottleneck (wd/bd NULL: identity block, else the stride-1 downsample block)
 * (x [B,H,W,Cin] bf16 -> y [B,H,W,4*Cmid] bf16; weights packed
 * K-major bf16 with fp32 biases as ivosw_assess_pack lays them out) with s_memtime stamps at the phase
 * boundaries of every workgroup: ts [B*(H/16)*(W/16)][16] uint64 on the device (may be NULL).             */
int ivosw_bneck_probe(const void* x, void* y, const void* wa, const float* ba, const void* wb, const float* bb,
                      const void* wc, const float* bc, const void* wd, const float* bd, const void* zeros,
                      int B, int H, int W, int Cin, int Cmid,
                      unsigned long long* ts, ivosw_stream_t stream);

/* Tuning probe: ONE wide fused bottleneck (res4 identity block: H = W = 16, Cin = 1024, Cmid = 256), weights K-major
 * packed bf16; `frag` is device scratch for their fragment-ordered copies; ts [B][8] uint64 phase stamps or NULL.   */
int ivosw_bneck_wide_probe(const void* x, void* y, const void* wa, const float* ba, const void* wb, const float* bb,
                           const void* wc, const float* bc, void* frag, int B, int H, int W, int Cin, int Cmid,
                           unsigned long long* ts, ivosw_stream_t stream);

/* Tuning probe: a RUN of n (1 .. 6) res4 identity blocks on B frames [B,16,16,1024].  w: n x (wa | wb | wc) K-major packed bf16,
 * bias: n x (ba[256] | bb[256] | bc[1024]); `frag`: device scratch of w's size + 256 B, the last 256 zero; y: n frame buffers, block j
 * writes y[j] and reads y[j - 1] (x for j = 0).  chain = 1: the chained stage kernel in one launch (with inplace = 1 the blocks between
 * the first and the last write over their input, only y[0] and y[n - 1] are written); chain = 0: one launch per block.
 * ts [n][B][8] uint64 phase stamps or NULL.                                                                              */
int ivosw_bneck_wide_stage_probe(const void* x, void* y, const void* w, const float* bias, void* frag, int n, int B, int chain,
                                 int inplace, unsigned long long* ts, ivosw_stream_t stream);

/* Tuning probe (round 5): the one-wave-per-SIMD, 4 x 4-register-tile contraction of the attainable-roof measurement
 * (csrc/gemm_bt.h; tools/ubench/gemm_tile_bench.hip times it): C [M][N] bf16 = act(A [M][K] . B [N][K]^T + bias [N]),
 * both operands K-major bf16, fp32 accumulation, act = ReLU when relu != 0.  M % 256 == 0, N % 256 == 0, K % 32 == 0, K >= 32.
 * No reference function stands behind it: the tower's 1x1 convolutions (models/assessment.py:58-61 through torchvision's
 * Bottleneck) are contractions of exactly this form, and the product path runs them in the 8-wave kernels that reach the same rate.
 * ts [M/256 * N/256][4] uint64 (may be NULL): s_memtime at start / after the K loop / at the end, s_memrealtime span.             */
int ivosw_gemm_bt_probe(const void* A, const void* B, const float* bias, void* C, int M, int N, int K, int relu,
                        unsigned long long* ts, ivosw_stream_t stream);

/* Tuning probe: ONE launch of the res2 stage kernel (the three bottlenecks of res2 + res3's forwarded conv1; reference
 * models/assessment.py:58-59) on x [B,64,64,64] bf16 with the weights of a packed bf16 arena (ivosw_assess_pack); y [B,64,64,256]
 * (y_s2 != 0: the even pixels, [B,32,32,256]), t1out [B,64,64,128]; ts [B*32][16] uint64 phase stamps or NULL.            */
int ivosw_res2_stage_probe(const void* packed, const void* x, void* y, void* t1out, int B, int y_s2, unsigned long long* ts,
                           ivosw_stream_t stream);

/* Test probe: ONE launch of one bf16 conv layer of the tower on caller-provided device tensors (tests/test_gpu_layer_kernels.py holds every
 * output element to the float64 restatement of tests/layer_ref.py).  Everything ConvArgs (csrc/conv.h) expresses for bf16:
 * x [B,H,W,Cin]; w K-major packed [Cout][ksize*ksize*Cin (+ Cin2)], K = (ky*ksize + kx)*Cin + c; fp32 bias [Cout]; res [B,Ho,Wo,Cout] or NULL;
 * x2 [B,H2,W2,Cin2] or NULL, sampled at (oy*stride2, ox*stride2) (1x1 only); ksize 1 or 3; Ho = (H + 2 pad - ksize) / stride + 1;
 * y [B,Ho,Wo,Cout]; zeros: >= 256 B of device zeros; rev: 1 = pixel tiles in descending order.
 * kernel = 0: the generic selector (conv_igemm_* / conv3x3_patch_kernel by shape, batch and tunables), *ran = its ConvKernel id (csrc/conv.h);
 * kernel = 1: conv1x1_wide_kernel - w is reordered into `frag` (device scratch of w's size) on the device first -, *ran = its NPT (8 or 4);
 * kernel = 2: the 8-phase contraction, *ran = 1 with a residual, else 0.
 * A shape the chosen kernel does not take is refused ("not covered"): nothing is launched, y and frag stay as they were.  frag may be NULL
 * for kernel 0 and 2; ran may be NULL. */
int ivosw_conv_probe(const void* x, const void* w, const float* bias, const void* res, const void* x2, void* y, const void* zeros,
                     void* frag, int B, int H, int W, int Cin, int Cout, int ksize, int stride, int pad, int relu, int rev,
                     int H2, int W2, int Cin2, int stride2, int kernel, int* ran, ivosw_stream_t stream);

/* Test probe: ONE launch of stage_first_kernel (res3's first block behind its conv1; csrc/stage_first.hip): t1 [B,64,64,128];
 * x2 [B,H2,W2,256] with (H2 = W2 = 64, stride2 = 2) or (H2 = W2 = 32, stride2 = 1); w2 K-major [128][9*128]; wc [512][128 + 256]
 * ([conv3 | downsample]); fp32 b2 [128], bc [512]; `frag`: device scratch of w2's + wc's size for their fragment-ordered copies, made on
 * the device; zeros: >= 256 B of device zeros; y [B,Ho,Wo,512].  Any other geometry (Ho = Wo = 32 is the kernel's only one) is refused
 * ("not covered") before anything is launched. */
int ivosw_stage_first_probe(const void* t1, const void* x2, const void* w2, const float* b2, const void* wc, const float* bc, void* frag,
                            const void* zeros, void* y, int B, int Ho, int Wo, int H2, int W2, int stride2, int rev,
                            ivosw_stream_t stream);

/* Test probe: ONE launch of res2 (three bottlenecks at 64 x 64) + res3's forwarded conv1 on caller-provided device tensors and weights
 * (tests/test_gpu_res2_stem_kernels.py holds every output element to the float64 restatement of tests/res2_ref.py).  x [B,64,64,64] bf16;
 * w, bias: HOST arrays of IVOSW_RES2_PROBE_NW device pointers, K-major bf16 weights and fp32 biases in the order
 *   conv1 of res2's blocks 0, 1, 2 and of res3's first block ([64][64], [64][256], [64][256], [128][256]),
 *   conv2 of blocks 0, 1, 2 ([64][9*64], K = (ky*3 + kx)*64 + c), conv3 of blocks 0, 1, 2 ([256][64]), block 0's downsample ([256][64]);
 * frag: IVOSW_RES2_PROBE_FRAG_BYTES of device scratch for what the kernels read, made on the device; zeros: >= 256 B of device zeros;
 * y [B,64,64,256] (y_s2 != 0: the even pixels, [B,32,32,256]); t1out [B,64,64,128]; rev: 1 = tiles in descending order.
 * form = 0: res2_stage_kernel on fragment-ordered copies (launch_fragpack; block 0's [conv3 | downsample] through launch_concat_k, as
 * ivosw_assess_pack makes them); form = 1: res2_chain_kernel on the fragment stream of launch_res2_chain_pack.
 * *ran (may be NULL) = kind + 4 * (y_s2 != 0), kind 0: res2_stage_kernel, 1: res2_chain_kernel one tile per workgroup (tunable
 * R2C_PERSIST = 0), 2: res2_chain_kernel persistent.  A NULL operand, B outside 1 .. 1024 or another form is refused before anything is
 * launched: y, t1out and frag stay as they were. */
#define IVOSW_RES2_PROBE_NW 11
#define IVOSW_RES2_PROBE_FRAG_BYTES 655360
int ivosw_res2_probe(const void* x, const void* const* w, const float* const* bias, void* frag, const void* zeros, void* y, void* t1out,
                     int B, int y_s2, int rev, int form, int* ran, ivosw_stream_t stream);

/* Test probe: ONE launch of stem_pool_kernel (7x7/2 convolution + folded BN + ReLU + 3x3/2 max-pool; csrc/stem.hip): roi [B,256,256,4] bf16;
 * w: the filter bank in the packed arena's layout, [64][8 ky][8 px][4 ch] bf16 with ky == 7 and px == 7 zero (as pack_stem_kernel writes
 * it); fp32 bias [64]; out [B,64,64,64]; rev: 1 = tiles in descending order.  A NULL operand or B outside 1 .. 1024 is refused before
 * anything is launched. */
int ivosw_stem_probe(const void* roi, const void* w, const float* bias, void* out, int B, int rev, ivosw_stream_t stream);

/* Test probe: ivosw_robot_skeleton_box's launcher with the launch's dynamic LDS size as an argument, lds_budget_bytes in [256, 163840]
 * (256: every non-empty box keeps its planes in the workspace), so that a test can send a 3 x 33 frame through the global planes and
 * tools/robot_box_probe.py can time the two plane homes on one region.  The workspace (m * 2 * H * ceil(W/32) * 4 bytes) is needed
 * whenever two full-frame planes + 256 bytes exceed the budget; every other argument and refusal as in ivosw_robot_skeleton_box. */
int ivosw_robot_box_probe(const uint8_t* gt, const uint8_t* pred, int n, int H, int W, const int32_t* units_host, int m, int cap,
                          int32_t* points, int32_t* counts, int32_t* iters, uint32_t* skel, uint32_t* workspace,
                          size_t workspace_bytes, int lds_budget_bytes, ivosw_stream_t stream);

/* Test probes of the DQN step's backward kernels (csrc/dqn_step.hip, dqn_head.h, lstm_bwd.h, brain_bwd.h), each the product's kernel unchanged on
 * caller-provided fp32 device tensors; tests/test_gpu_dqn_kernels.py holds their outputs to the float64 restatements of tests/dqn_ref.py.
 * Every entry refuses a NULL operand, and with "not covered" what its kernel does not take, before anything is launched: nothing is written. */

/* ONE bwd_tail_kernel launch holding one weight-gradient job: slab z of C [nslab][M][N] = sum over the K-rows k of slab z of
 * (A[k*lda + m] + A2[k*lda + m]) * B[k*ldb + n]; A2 may be NULL.  Slab z covers the rows [z*per, min(K, (z + 1)*per)) with
 * per = ceil(ceil(K / nslab) / 16) * 16; a slab without rows is written as zeros.  nslab > 0 is taken as given (at most 64); nslab == 0
 * asks for the step's own choice for `kind` (0: dW_hh, 1: dW_ih, 2: dW2).  *used (may be NULL) = the slab count that ran.
 * M % 64 == 0, N % 128 == 0, K >= 1, lda >= M, ldb >= N, both multiples of 4, 16-byte aligned operands; anything else is not covered. */
int ivosw_bwd_wgrad_probe(const float* A, const float* A2, const float* B, float* C, int lda, int ldb, int M, int N, int K, int nslab,
                          int kind, int* used, ivosw_stream_t stream);

/* ONE bwd_tail_kernel launch of the dgrad tiles alone (ceil(rows / 16) of them, the grid padded to a multiple of 8 as in the step):
 * de [rows,128] = (dG + dG2) [rows,512] . wih [512,128], da1 [rows,128] = (de . w2 [128,128]) * (a1 > 0).  rows >= 1. */
int ivosw_bwd_dgrad_probe(const float* dG, const float* dG2, const float* wih, const float* w2, const float* a1, float* de, float* da1,
                          int rows, ivosw_stream_t stream);

/* ONE bwd_tail_kernel launch holding one column-sum job: slab z of out [nsplit][N] = the sum of A[m*ld + n] over the rows m of split z,
 * and with x [M,2] (x and outw both given or both NULL) slab z of outw [nsplit][N][2] = the sums of A[m*ld + n] * x[m*2 + c].  Split z
 * covers the rows [z*per, min(M, (z + 1)*per)) with per = ceil(ceil(M / nsplit) / 8) * 8.  M >= 1, 1 <= N <= ld, 1 <= nsplit <= 64. */
int ivosw_bwd_csum_probe(const float* A, const float* x, float* out, float* outw, int M, int N, int ld, int nsplit, ivosw_stream_t stream);

/* The step's two bwd_tail_kernel launches and its slab reduction, built by the code the step runs (plan_bwd_tail): launch 1 = the dgrad
 * tiles beside dW_hh, dW_ih and dW3; launch 2 = dW2 beside the four column sums; then splitk_reduce_group_kernel.  rows = B*T;
 * dG [2][rows][512] (forward, then backward direction), hprev [2 rows,128], e, a1 [rows,128], dd1c, w4term [B,128], hcc [B,256],
 * state [rows,2], wih [512,128], w2 [128,128]; outputs de, da1 [rows,128] and the gradient arena grads [IVOSW_BRAIN_NPARAMS], of which
 * every tensor but decoder_fc2.bias (the head kernel's) is written; ws: IVOSW_BWD_GROUP_WS_FLOATS floats of device scratch for the slabs. */
#define IVOSW_BWD_GROUP_WS_FLOATS ((16 + 40 + 40) * 512 * 128 + 8 * 512)
int ivosw_bwd_group_probe(const float* dG, const float* hprev, const float* e, const float* a1, const float* dd1c, const float* hcc,
                          const float* w4term, const float* state, const float* wih, const float* w2, float* de, float* da1, float* grads,
                          float* ws, int B, int T, ivosw_stream_t stream);

/* ONE launch of head_fused_kernel<per != 0> (csrc/dqn_head.h) with the kernel's own arguments: prm + o_w3 = W3 [128,256],
 * prm + o_w4 = w4 [128]; q_np, q_nt, q_s [B,T]; action [B] int64; r_step, r_done [B]; d1_s [B,T,128]; hs_s [B,T,256]; outputs dq [B],
 * dd1c, w4term [B,128], hcc, dhc [B,256], loss [1], db4 [1]; per != 0: weights [B] in and td [B] out, else both are ignored.
 * B, T >= 1, o_w3, o_w4 >= 0, loss_kind IVOSW_DQN_LOSS_MSE or _HUBER. */
int ivosw_head_fused_probe(const float* prm, int o_w3, int o_w4, const float* q_np, const float* q_nt, const float* q_s, const int64_t* action,
                           const float* r_step, const float* r_done, int B, int T, float gamma, int loss_kind, float delta,
                           const float* d1_s, const float* hs_s, float* dq, float* dd1c, float* w4term, float* hcc, float* dhc, float* loss,
                           float* db4, int per, const float* weights, float* td, ivosw_stream_t stream);

/* ONE launch of the BPTT recurrence: whh [512,128]; gates [2,N,T,512] (post-activation i, f, g, o) and cs [2,N,T,128] as the forward
 * keeps them; dhc [N,256] = dL/d(h_fw | h_bw) at frame action[n]; dG [2,N,T,512] out, zero at the frames a direction consumes after its
 * loss frame.  form 0: lstm_bwd_quad_kernel<1> (the step's default); form 1, 2, 4: lstm_bwd_kernel<form>.  N, T >= 1. */
int ivosw_lstm_bwd_probe(const float* whh, const float* gates, const float* cs, const float* dhc, const int64_t* action, float* dG, int N, int T,
                         int form, ivosw_stream_t stream);

/* Test probes of the Brain forward kernels (csrc/brain_fused.h, csrc/lstm_fwd.h, launched by csrc/brain.hip), each the product's kernel unchanged on caller-provided fp32
 * device tensors; tests/test_gpu_dqn_fwd_kernels.py holds their outputs to the float64 restatements of tests/dqn_ref.py.  The recurrence
 * and the recurrence + decoder kernel are launched by the functions the forward drivers call (launch_lstm_fwd, launch_lstm_fwd_pair,
 * launch_lstm_fwd_ragged, launch_fwd_mega), the form by their rule (lstm_fwd_form_for).  Every entry refuses a NULL operand, and with
 * "not covered" what its kernel does not take, before anything is launched: nothing is written.  Per-job arguments are HOST arrays of njobs
 * entries (device pointers, ints); `prm` is a parameter arena in the state_dict layout (IVOSW_BRAIN_NPARAMS floats, 16-byte aligned). */

/* ONE enc_fused_kernel launch of njobs = 1 or 2 jobs (job 1's tiles behind job 0's), without a drawn minibatch.  Job i: its rows
 * [0, rows0) are x[row*2 + c], [rows0, rows) are x2[(row - rows0)*2 + c]; gx [rows,512] is written for every row, a1 and e [rows,128] for
 * the rows >= keep_row.  1 <= rows <= 2^20, 0 <= rows0 <= rows, 0 <= keep_row <= rows. */
int ivosw_enc_fused_probe(int njobs, const float* const* prm, const float* const* x, const float* const* x2, const int* rows0, const int* rows,
                          const int* keep_row, float* const* gx, float* const* a1, float* const* e, ivosw_stream_t stream);

/* ONE dec_fused_kernel launch of njobs = 1 or 2 jobs: hs [rows,256] (16-byte aligned) -> q [rows] for every row, d1 [rows,128] for the rows
 * >= keep_row. */
int ivosw_dec_fused_probe(int njobs, const float* const* prm, const float* const* hs, const int* rows, const int* keep_row, float* const* d1,
                          float* const* q, ivosw_stream_t stream);

/* ONE launch of the forward recurrence: whh [512,128] (16-byte aligned), gx [N,T,512] -> hs [N,T,256] (h_fw | h_bw after frame t) and, for
 * the samples >= keep_from and indexed from keep_from, gates [2,N-keep_from,T,512] (i, f, g, o after their activations), cs and hprev
 * [2,N-keep_from,T,128] (hprev: h before the frame).  gates, cs and hprev are given together or all NULL (nothing is kept).
 * form 1, 2, 4: lstm_fwd_kernel<form>; 11, 12, 14: lstm_fwd_quad_kernel<form - 10>; 20: lstm_fwd_mfma_kernel (refused below 2 N = 8, as the
 * product never sends it fewer rows); 0: the product's own choice at this N.  *ran (may be NULL) = the form that ran.
 * N, T >= 1, N*T <= 2^20, 0 <= keep_from <= N. */
int ivosw_lstm_fwd_probe(const float* whh, const float* gx, float* hs, float* gates, float* cs, float* hprev, int N, int T, int keep_from,
                         int form, int* ran, ivosw_stream_t stream);

/* ONE lstm_fwd_mfma_pair_kernel launch on two argument sets (host arrays of two entries each; T is shared): job 1's workgroups behind job
 * 0's.  Each job as in ivosw_lstm_fwd_probe with the mfma form (2 N >= 8). */
int ivosw_lstm_fwd_pair_probe(const float* const* whh, const float* const* gx, float* const* hs, float* const* gates, float* const* cs,
                              float* const* hprev, const int* N, int T, const int* keep_from, ivosw_stream_t stream);

/* ONE lstm_fwd_quad_ragged_kernel launch: n_seqs sequences of lengths[k] frames (host array) laid end to end in gx [rows,512] and
 * hs [rows,256]; the sequence table is built by the check ivosw_brain_forward_ragged runs on its lengths, with its refusals. */
int ivosw_lstm_fwd_ragged_probe(const float* whh, const float* gx, float* hs, const int* lengths, int n_seqs, ivosw_stream_t stream);

/* ONE brain_fwd_mega_kernel launch (recurrence + decoder; tunable FWD_MEGA) of njobs = 1 or 2 jobs with a shared T.  Job i: W_hh, W3, b3,
 * w4, b4 out of prm; gx [N,T,512]; hs [N,T,256] is written for the samples >= hs_from; gates, cs, hprev (together or all NULL) and
 * d1 [N*T,128] for the samples >= keep_from (with NULL gates nothing is kept, d1 included); q [N*T] for every row.  2 N >= 8 per job, and T
 * such that 2 T rows of 260 floats fit the kernel's 150 KB of dynamic LDS (T <= 73); 0 <= keep_from, hs_from <= N. */
int ivosw_fwd_mega_probe(int njobs, const float* const* prm, const float* const* gx, float* const* hs, float* const* gates, float* const* cs,
                         float* const* hprev, float* const* d1, float* const* q, const int* N, int T, const int* keep_from, const int* hs_from,
                         ivosw_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* IVOSW_PROBE_H */
