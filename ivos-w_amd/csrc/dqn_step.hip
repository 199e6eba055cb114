// The Double-DQN step on the Brain: loss and hand-derived backward (ivosw_dqn_loss_grad*), and the one-call step that also draws the
// minibatch and applies the update (ivosw_dqn_step_drawn*).  The forward pass is brain.hip's (brain_fwd.h).
//
// Reference arithmetic: Agent.update_agent (models/agent.py:128-155) over Brain.forward (:33-64).
#ifdef IVOSW_PROBES
#include "../../include/ivosw_probe.h"
#endif
#include <cmath>
#include <mutex>

#include "gemm_f32.h"
#include "dqn_head.h"
#include "lstm_bwd.h"
#include "brain_bwd.h"
#include "dqn_update.h"

namespace ivosw {

// ---------------------------------------------------------------- column sums
// out[n] = sum_m A[m*ld + n]; grid = ceil(N/32), block = 1024 (32 cols x 32 row groups)
__global__ __launch_bounds__(1024) void colsum_kernel(const float* __restrict__ A, int M, int N, int ld, float* __restrict__ out) {
    __shared__ float red[32][33];
    const int c = threadIdx.x & 31, rg = threadIdx.x >> 5;
    const int n = blockIdx.x * 32 + c;
    // four independent partial sums and 8 loads in flight per thread: the loop is a chain of global-load latencies
    // otherwise (M/32 = 100 dependent round trips, 15 us); the summation order stays fixed (deterministic)
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    if (n < N) {
        int m = rg;
        for (; m + 224 < M; m += 256) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = A[(size_t)(m + 32 * u) * ld + n];
            s0 += v[0]; s1 += v[1]; s2 += v[2]; s3 += v[3];
            s0 += v[4]; s1 += v[5]; s2 += v[6]; s3 += v[7];
        }
        for (; m < M; m += 32) s0 += A[(size_t)m * ld + n];
    }
    const float s = (s0 + s1) + (s2 + s3);
    red[rg][c] = s;
    __syncthreads();
    if (rg == 0 && n < N) {
        float t = 0.f;
#pragma unroll
        for (int i = 0; i < 32; ++i) t += red[i][c];
        out[n] = t;
    }
}

// The same reduction for up to two matrices in one launch (blockIdx.y = which), each optionally with two weighted sums on top:
// out[n] = sum_m A[m][n]; outw[n*2 + c] = sum_m A[m][n] * x[m*2 + c] (c = 0, 1) — encoder_fc1's weight gradient
// dW1[j][c] = sum_rows da1[row][j] * x[row][c] is a weighted column sum of the matrix whose plain column sum is db1.
struct ColsumJob {
    const float* A;
    const float* x;      // [M,2] or nullptr
    float* out;          // [N]            (split over blockIdx.z: slab z at out + z * N; the caller reduces the slabs)
    float* outw;         // [N,2] when x   (slab z at outw + z * 2N)
    int M, N, ld;
    int nsplit;          // row splits of this job (0 = gridDim.z); workgroups with blockIdx.z >= nsplit have nothing to do
};
struct ColsumGroup { ColsumJob j[4]; };
__global__ __launch_bounds__(1024) void colsum_group_kernel(ColsumGroup grp) {
    __shared__ float red[3][32][33];
    const ColsumJob& jb = grp.j[blockIdx.y];
    const int c = threadIdx.x & 31, rg = threadIdx.x >> 5;
    const int n = blockIdx.x * 32 + c;
    const int nsplit = jb.nsplit > 0 ? jb.nsplit : (int)gridDim.z;
    if (blockIdx.x * 32 >= jb.N || (int)blockIdx.z >= nsplit) return;
    float s[4] = {0.f, 0.f, 0.f, 0.f}, s0[4] = {0.f, 0.f, 0.f, 0.f}, s1[4] = {0.f, 0.f, 0.f, 0.f};
    const bool wx = jb.x != nullptr;
    // rows [mbeg, mend) of this split (multiples of 32 rows, so every row group sees whole strides)
    const int per = ((jb.M + nsplit - 1) / nsplit + 31) / 32 * 32;
    const int mbeg = blockIdx.z * per, mend = min(jb.M, mbeg + per);
    if (n < jb.N) {
        int m = mbeg + rg;
        for (; m + 224 < mend; m += 256) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = jb.A[(size_t)(m + 32 * u) * jb.ld + n];
#pragma unroll
            for (int u = 0; u < 8; ++u) s[u & 3] += v[u];
            if (wx) {
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const float2 xv = *reinterpret_cast<const float2*>(jb.x + (size_t)(m + 32 * u) * 2);
                    s0[u & 3] = fmaf(v[u], xv.x, s0[u & 3]);
                    s1[u & 3] = fmaf(v[u], xv.y, s1[u & 3]);
                }
            }
        }
        for (; m < mend; m += 32) {
            const float v = jb.A[(size_t)m * jb.ld + n];
            s[0] += v;
            if (wx) {
                const float2 xv = *reinterpret_cast<const float2*>(jb.x + (size_t)m * 2);
                s0[0] = fmaf(v, xv.x, s0[0]);
                s1[0] = fmaf(v, xv.y, s1[0]);
            }
        }
    }
    red[0][rg][c] = (s[0] + s[1]) + (s[2] + s[3]);
    red[1][rg][c] = (s0[0] + s0[1]) + (s0[2] + s0[3]);
    red[2][rg][c] = (s1[0] + s1[1]) + (s1[2] + s1[3]);
    __syncthreads();
    if (rg < 3 && n < jb.N && (rg == 0 || wx)) {
        float t = 0.f;
#pragma unroll
        for (int i = 0; i < 32; ++i) t += red[rg][i][c];
        if (rg == 0) jb.out[(size_t)blockIdx.z * jb.N + n] = t;
        else jb.outw[(size_t)blockIdx.z * 2 * jb.N + n * 2 + (rg - 1)] = t;
    }
}

__global__ void add2_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ o, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) o[i] = a[i] + b[i];
}

static constexpr int WG_SPLIT = 16;
static constexpr int WG_SPLIT_MAX = 40;   // slab sets of the two long-K weight gradients are sized for this (tunables DQN_SPLIT_HH / _IH)
static constexpr int CS_SPLIT = 8;        // row splits of the two long column sums (db2 <- de, {db1, dW1} <- da1)

// The four slab sets of the backward tail in workspace order, under TailIO's names.  The step's workspace and the group probe's scratch
// are both cut by carve_tail_slabs, from these sizes.
constexpr size_t SLABS_W2_FLOATS = (size_t)WG_SPLIT * 512 * 128;       // up to 64 slabs of 128*128
constexpr size_t SLABS_LONGK_FLOATS = (size_t)WG_SPLIT_MAX * 512 * 128;   // slabs_hh, slabs_ih
constexpr size_t SLABS_CS_FLOATS = (size_t)4 * CS_SPLIT * 128;         // db2 [CS_SPLIT][128] | db1 [CS_SPLIT][128] | dW1 [CS_SPLIT][256]
constexpr size_t TAIL_SLABS_FLOATS = SLABS_W2_FLOATS + 2 * SLABS_LONGK_FLOATS + SLABS_CS_FLOATS;
struct TailSlabs {
    float *slabs_w2, *slabs_hh, *slabs_ih, *slabs_cs;
};
static TailSlabs carve_tail_slabs(Arena& ar) {
    TailSlabs s{};
    s.slabs_w2 = ar.take<float>(SLABS_W2_FLOATS);
    s.slabs_hh = ar.take<float>(SLABS_LONGK_FLOATS);
    s.slabs_ih = ar.take<float>(SLABS_LONGK_FLOATS);
    s.slabs_cs = ar.take<float>(SLABS_CS_FLOATS);     // row-split column sums
    return s;
}

// K-slabs of the register-resident weight gradients (brain_bwd.h), a multiple of 48 rows where the sizes allow (the kernel's loop is
// unrolled by three 16-row steps): about K / want rows each, at most cap slabs.  B = 128, T = 25: 200 + 184 + 96 + 4 workgroups in the
// first launch, one round at two per CU; dW2's launch is latency-bound, so many small workgroups (48-row slabs).
enum TailSlabKind { TAIL_SLABS_HH = 0, TAIL_SLABS_IH = 1, TAIL_SLABS_W2 = 2 };
static int tail_slabs_for(int K, int kind) {
    static constexpr int WANT[3] = {23, 12, 32}, CAP[3] = {WG_SPLIT_MAX, WG_SPLIT_MAX, 64};
    const int per = std::max(48, (K / WANT[kind] + 47) / 48 * 48);
    return std::min(CAP[kind], std::max(1, (K + per - 1) / per));
}

// What the two launches of the backward tail read and write: the step's workspace (dqn_loss_grad_impl) or a test's own tensors
// (ivosw_bwd_group_probe).
struct TailIO {
    const float *dG, *dG_bw;     // [rows,512] each: dL/d(gate pre-activation), forward and backward direction (dG_bw = dG + rows*512)
    const float *hprev;          // [2 rows,128]
    const float *e, *a1;         // [rows,128]
    const float *dd1c, *hcc, *w4term;    // [B,128], [B,256], [B,128]
    const float *state;          // [rows,2]
    const float *wih, *w2;       // [512,128], [128,128]
    float *de, *da1;             // [rows,128]
    float *slabs_hh, *slabs_ih;  // WG_SPLIT_MAX x 512*128 each
    float *slabs_w2;             // WG_SPLIT x 512*128 (up to 64 slabs of 128*128)
    float *slabs_cs;             // 8*512: db2 [CS_SPLIT][128] | db1 [CS_SPLIT][128] | dW1 [CS_SPLIT][256]
    float *grads;                // the gradient arena: dW3, dW4 and db3 are written in place
    int B, T;
};
struct TailPlan {
    TailGroup t1, t2;
    int split_hh, split_ih, split_w2;
};
// 1. {dgrad chain de -> da1 per 16-row tile, dW_hh, dW_ih, dW3} in one launch, 2. dW2 (it needs de) and the four column sums beside it
static TailPlan plan_bwd_tail(const TailIO& io) {
    const int B = io.B, rows = io.B * io.T;
    auto tiles = [](const WgradJob& j) { return (j.M / 64) * (j.N / 128) * j.nslab; };
    TailPlan pl{};
    TailGroup& t1 = pl.t1;
    t1.dg = DgradArgs{io.dG, io.dG_bw, io.wih, io.w2, io.a1, io.de, io.da1, rows};
    t1.n_dgrad = ((rows + 15) / 16 + 7) / 8 * 8;        // padded to a multiple of 8 (XCD-aligned weight-gradient section)
    pl.split_hh = tail_slabs_for(2 * rows, TAIL_SLABS_HH);
    pl.split_ih = tail_slabs_for(rows, TAIL_SLABS_IH);
    t1.w[0] = WgradJob{io.dG, nullptr, io.hprev, io.slabs_hh, 512, 128, 512, 128, 2 * rows, pl.split_hh};
    t1.w[1] = WgradJob{io.dG, io.dG_bw, io.e, io.slabs_ih, 512, 128, 512, 128, rows, pl.split_ih};
    t1.w[2] = WgradJob{io.dd1c, nullptr, io.hcc, io.grads + O_W3, 128, 256, 128, 256, B, 1};
    t1.n = 3;
    for (int i = 0; i < 3; ++i) t1.first[i + 1] = t1.first[i] + tiles(t1.w[i]);
    for (int i = 4; i <= TAIL_MAX; ++i) t1.first[i] = t1.first[3];
    TailGroup& t2 = pl.t2;
    pl.split_w2 = tail_slabs_for(rows, TAIL_SLABS_W2);
    t2.w[0] = WgradJob{io.de, nullptr, io.a1, io.slabs_w2, 128, 128, 128, 128, rows, pl.split_w2};
    t2.n = 1;
    t2.first[1] = tiles(t2.w[0]);
    for (int i = 2; i <= TAIL_MAX; ++i) t2.first[i] = t2.first[1];
    // ... and the four column sums beside it (they used to be a launch of their own)
    float* s4 = io.slabs_cs;
    t2.cs[0] = CsumJob{io.de, nullptr, s4, nullptr, rows, 128, 128, CS_SPLIT};                                          // db2 slabs
    t2.cs[1] = CsumJob{io.da1, io.state, s4 + CS_SPLIT * 128, s4 + 2 * CS_SPLIT * 128, rows, 128, 128, CS_SPLIT};       // db1, dW1 slabs
    t2.cs[2] = CsumJob{io.w4term, nullptr, io.grads + O_W4, nullptr, B, 128, 128, 1};
    t2.cs[3] = CsumJob{io.dd1c, nullptr, io.grads + O_B3, nullptr, B, 128, 128, 1};
    t2.n_cs = 4;
    for (int i = 0; i < 4; ++i) t2.cs_first[i + 1] = t2.cs_first[i] + ((t2.cs[i].N + 31) / 32) * t2.cs[i].nsplit;
    return pl;
}
static void launch_bwd_tail(const TailPlan& pl, hipStream_t st) {
    hipLaunchKernelGGL(bwd_tail_kernel, dim3(pl.t1.n_dgrad + pl.t1.first[3]), dim3(256), 0, st, pl.t1);
    hipLaunchKernelGGL(bwd_tail_kernel, dim3(pl.t2.first[1] + pl.t2.cs_first[4]), dim3(256), 0, st, pl.t2);
}
// the fixed-order reduction of every slab set of the backward tail into the gradient arena
static ReduceGroup tail_reduce_group(const TailSlabs& s, float* grads, int split_hh, int split_ih, int split_w2) {
    ReduceGroup rg{};
    rg.slabs[0] = s.slabs_hh; rg.out[0] = grads + O_WHH; rg.n[0] = 512 * 128; rg.nslab[0] = split_hh;
    rg.slabs[1] = s.slabs_ih; rg.out[1] = grads + O_WIH; rg.n[1] = 512 * 128; rg.nslab[1] = split_ih;
    rg.slabs[2] = s.slabs_w2; rg.out[2] = grads + O_W2; rg.n[2] = 128 * 128; rg.nslab[2] = split_w2;
    rg.slabs[3] = s.slabs_cs; rg.out[3] = grads + O_B2; rg.n[3] = 128; rg.nslab[3] = CS_SPLIT;
    rg.slabs[4] = s.slabs_cs + CS_SPLIT * 128; rg.out[4] = grads + O_B1; rg.n[4] = 128; rg.nslab[4] = CS_SPLIT;
    rg.slabs[5] = s.slabs_cs + 2 * CS_SPLIT * 128; rg.out[5] = grads + O_W1; rg.n[5] = 256; rg.nslab[5] = CS_SPLIT;
    return rg;
}

// One helper stream + four events per device: the only state the library keeps between calls (documented in
// INTEGRATION.md).  Creation is serialised and all-or-nothing; ivosw_dqn_loss_grad holds the device's mutex while it
// enqueues, so two host threads (or two caller streams) on one device cannot interleave their fork / join pairs — an
// event re-recorded by a later call does not disturb waits that were already enqueued on it.
struct Side {
    std::mutex mu;
    hipStream_t stream = nullptr;
    hipEvent_t ev[4] = {};
    bool tried = false;
};
static Side* side_for_current_device() {
    static Side sides[64];
    static std::mutex init_mu;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    Side& s = sides[dev];
    std::lock_guard<std::mutex> lk(init_mu);
    if (!s.tried) {
        s.tried = true;
        bool ok = hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking) == hipSuccess;
        int made = 0;
        for (; ok && made < 4; ++made) ok = hipEventCreateWithFlags(&s.ev[made], hipEventDisableTiming) == hipSuccess;
        if (!ok) {      // partial failure: give everything back, the single-stream path is used from now on
            for (int i = 0; i < made; ++i) if (s.ev[i]) (void)hipEventDestroy(s.ev[i]);
            if (s.stream) (void)hipStreamDestroy(s.stream);
            s.stream = nullptr;
            (void)hipGetLastError();
        }
    }
    return s.stream ? &s : nullptr;
}

// The step's workspace and its one layout: over a workspace carve_dqn cuts the buffers, over a counting Arena it gives the size.
struct DqnWs : TailSlabs {
    FwdBufs pol, tgt;
    float *xcat, *dq, *dd1c, *w4term, *hcc, *dhc, *dG, *dgx, *de, *da1;
};
static DqnWs carve_dqn(Arena& ar, int B, int T) {
    const size_t rows = (size_t)B * T;
    DqnWs w{};
    w.pol = carve_fwd(ar, 2 * B, T, B);   // samples [0,B) = s', [B,2B) = s (kept for backward)
    w.tgt = carve_fwd(ar, B, T, -1);
    w.xcat = ar.take<float>(2 * rows * 2);
    w.dq = ar.take<float>(B);
    w.dd1c = ar.take<float>((size_t)B * 128);
    w.w4term = ar.take<float>((size_t)B * 128);
    w.hcc = ar.take<float>((size_t)B * 256);
    w.dhc = ar.take<float>((size_t)B * 256);
    w.dG = ar.take<float>(2 * rows * 512);
    w.dgx = ar.take<float>(rows * 512);
    w.de = ar.take<float>(rows * 128);
    w.da1 = ar.take<float>(rows * 128);
    static_cast<TailSlabs&>(w) = carve_tail_slabs(ar);   // split-K slabs: one set per concurrently reduced weight gradient
    return w;
}

}  // namespace ivosw

using namespace ivosw;

extern "C" size_t ivosw_dqn_ws_bytes(int B, int T) {
    if (B <= 0 || T <= 0) return 0;
    Arena count;
    carve_dqn(count, B, T);
    return count.bytes();
}

// The loss option of the _ex entries: IVOSW_DQN_LOSS_MSE, or IVOSW_DQN_LOSS_HUBER with a finite delta > 0 (checked for either kind).
static int check_dqn_loss(const char* who, int loss_kind, float delta) {
    if (loss_kind != IVOSW_DQN_LOSS_MSE && loss_kind != IVOSW_DQN_LOSS_HUBER) {
        set_error("%s: unknown loss kind %d (IVOSW_DQN_LOSS_MSE = 0, IVOSW_DQN_LOSS_HUBER = 1)", who, loss_kind);
        return IVOSW_ERR_ARG;
    }
    if (!(std::isfinite(delta) && delta > 0.f)) {
        set_error("%s: huber_delta must be finite and > 0, got %g", who, (double)delta);
        return IVOSW_ERR_ARG;
    }
    return IVOSW_OK;
}

// ---------------------------------------------------------------- loss + gradient in stages: forward and head, BPTT, backward tail
// One call's arguments (weights / td nullptr: the unweighted head), its workspace and its stream: what every stage reads.
struct LossGrad {
    const float *policy, *target, *state, *new_state;
    const int64_t* action;
    const float *reward_step, *reward_done;
    int B, T;
    float gamma;
    int loss_kind;
    float delta;
    float *grads, *loss;
    const float* weights;
    float* td;
    DqnWs w;
    hipStream_t st;
    int rows() const { return B * T; }
    // the backward pass reads the `state` half (samples [B, 2B)) of the policy pass's buffers
    const float* e_s() const { return w.pol.e + (size_t)rows() * 128; }
    const float* a1_s() const { return w.pol.a1 + (size_t)rows() * 128; }
    // dgx = dG[fw] + dG[bw] (the same e_t feeds both directions): summed on load by the kernels that consume it (GemmF32::A2)
    const float* dG_bw() const { return w.dG + (size_t)rows() * 512; }
};

// The step is a chain of launches that each occupy a fraction of the chip for 5-30 us: off the fused chain, independent branches run
// on the device's second stream (Side; tunable DQN_STREAMS), forked and joined with its events under its lock, so their kernels overlap
// instead of queueing behind each other.  Without one, s2 is the caller's stream and fork / join do nothing.
struct Fork {
    Side* sd;
    std::unique_lock<std::mutex> lock;
    hipStream_t st, s2;
    bool sync_ok = true;
    explicit Fork(hipStream_t st_) : sd(tune_get("DQN_STREAMS", 1) ? side_for_current_device() : nullptr), st(st_), s2(sd ? sd->stream : st_) {
        if (sd) lock = std::unique_lock<std::mutex>(sd->mu);
    }
    void fork(int k) {          // s2 continues after everything enqueued on st so far
        if (!sd) return;
        sync_ok &= hipEventRecord(sd->ev[k], st) == hipSuccess;
        sync_ok &= hipStreamWaitEvent(s2, sd->ev[k], 0) == hipSuccess;
    }
    void join(int k) {          // st continues after everything enqueued on s2 so far
        if (!sd) return;
        sync_ok &= hipEventRecord(sd->ev[k], s2) == hipSuccess;
        sync_ok &= hipStreamWaitEvent(st, sd->ev[k], 0) == hipSuccess;
    }
};

// 1. forward: policy on [s'; s] in one batch, target on s' (agent.py:135-137,144), then the head: Double-DQN targets, loss, dL/dQsa
// (:136-151), the decoder backward on the B rows that carry loss and dL/dh at the loss frame.  Fused: both nets per launch, then the
// head in one: 4 launches, one stream, no events.  Un-fused: the target pass runs beside the policy pass (host order matters: the
// policy chain is the critical path, so it is enqueued first), then three launches for the head.
static void forward_and_head(const LossGrad& a, const FwdPass* passes, bool fused, const EncDraw* draw, Fork& fk) {
    const DqnWs& w = a.w;
    const int B = a.B, T = a.T, rows = a.rows();
    hipStream_t st = a.st;
    const float* q_np = w.pol.q;
    const float* q_s = w.pol.q + rows;
    const float* d1_s = w.pol.d1 + (size_t)rows * 128;
    const float* hs_s = w.pol.hs + (size_t)rows * 256;
    if (fused) {
        brain_forward_fused(passes, 2, T, st, draw);
        hipLaunchKernelGGL(a.weights ? head_fused_kernel<true> : head_fused_kernel<false>, dim3(B), dim3(256), 0, st, a.policy, O_W3, O_W4, q_np,
                           w.tgt.q, q_s, a.action, a.reward_step, a.reward_done, B, T, a.gamma, a.loss_kind, a.delta, d1_s, hs_s, w.dq, w.dd1c,
                           w.w4term, w.hcc, w.dhc, a.loss, a.grads + O_B4, a.weights, a.td);
        return;
    }
    fk.fork(0);
    brain_forward_internal(a.policy, a.new_state, 2 * B, T, w.pol, st, a.state, B);
    brain_forward_internal(a.target, a.new_state, B, T, w.tgt, fk.s2);
    fk.join(1);
    hipLaunchKernelGGL(a.weights ? dqn_head_kernel<true> : dqn_head_kernel<false>, dim3(1), dim3(256), 0, st, q_np, w.tgt.q, q_s, a.action,
                       a.reward_step, a.reward_done, B, T, a.gamma, a.loss_kind, a.delta, w.dq, a.loss, a.grads + O_B4, a.weights, a.td);
    hipLaunchKernelGGL(dec_bwd_rows_kernel, dim3(B), dim3(128), 0, st, a.policy, w.dq, a.action, d1_s, hs_s, T, w.dd1c, w.w4term, w.hcc);
    // dhc[B,256] = (dd1c * W3) . (hcat > 0)
    GemmF32 g{};
    g.A = w.dd1c; g.sam = 128; g.sak = 1; g.B = a.policy + O_W3; g.sbk = 256; g.sbn = 1; g.C = w.dhc; g.ldc = 256;
    g.M = B; g.N = 256; g.K = 128; g.mask = w.hcc; g.splitk = 1;
    launch_gemm_f32(g, st);
}

// 2. BPTT through the shared cell
static void bptt(const LossGrad& a) {
    const int B = a.B;
    LstmBwd lb{};
    lb.whh = a.policy + O_WHH; lb.gates = a.w.pol.gates; lb.cs = a.w.pol.cs; lb.dhc = a.w.dhc; lb.action = a.action; lb.dG = a.w.dG;
    lb.N = B; lb.T = a.T; lb.ts = g_lstm_probe_bwd;
    const int R = rows_per_wg(2 * B);
    const int nwg = (2 * B + R - 1) / R;
    if (tune_get("LSTM_QUAD", 1)) {
        // one row per workgroup whatever the batch: with two or more rows the per-row state no longer fits beside W_hh
        // (hipcc spills 320+ registers), and a second round of workgroups costs what the second row would
        hipLaunchKernelGGL(lstm_bwd_quad_kernel<1>, dim3(2 * B), dim3(512), 0, a.st, lb);
    } else if (R == 1) hipLaunchKernelGGL(lstm_bwd_kernel<1>, dim3(nwg), dim3(512), 0, a.st, lb);
    else if (R == 2) hipLaunchKernelGGL(lstm_bwd_kernel<2>, dim3(nwg), dim3(512), 0, a.st, lb);
    else hipLaunchKernelGGL(lstm_bwd_kernel<4>, dim3(nwg), dim3(512), 0, a.st, lb);
}

// 3. the backward tail: everything after the recurrence, in one of three forms of the same step.  The first two leave their weight
// gradients in slab sets and return the fixed-order reduction that finishes them; the third reduces as it goes.
//
// 3a. register-resident kernels (brain_bwd.h; the product path), two launches: plan_bwd_tail
static ReduceGroup tail_resident(const LossGrad& a) {
    const DqnWs& w = a.w;
    const TailPlan pl = plan_bwd_tail(TailIO{w.dG, a.dG_bw(), w.pol.hprev, a.e_s(), a.a1_s(), w.dd1c, w.hcc, w.w4term, a.state, a.policy + O_WIH,
                                             a.policy + O_W2, w.de, w.da1, w.slabs_hh, w.slabs_ih, w.slabs_w2, w.slabs_cs, a.grads, a.B, a.T});
    launch_bwd_tail(pl, a.st);
    return tail_reduce_group(w, a.grads, pl.split_hh, pl.split_ih, pl.split_w2);
}

// The tail's six contractions as generic GEMMs, for the two forms below.  dgx / dgx2: dG and its backward half, summed on load, or the
// add2 pass's sum and nullptr.  The slab sets and split counts of the three long-K weight gradients are the launching form's.
struct TailGemms {
    GemmF32 dw3, dwhh, dwih, de, da1, dw2;
};
static TailGemms tail_gemms(const LossGrad& a, const float* dgx, const float* dgx2) {
    const DqnWs& w = a.w;
    const int B = a.B, rows = a.rows();
    TailGemms t{};
    // dW3[128,256] = dd1c^T * hcc
    t.dw3.A = w.dd1c; t.dw3.sam = 1; t.dw3.sak = 128; t.dw3.B = w.hcc; t.dw3.sbk = 256; t.dw3.sbn = 1; t.dw3.C = a.grads + O_W3; t.dw3.ldc = 256;
    t.dw3.M = 128; t.dw3.N = 256; t.dw3.K = B; t.dw3.splitk = 1;
    // dWhh[512,128] = sum_{d,n,t} dG^T * hprev          (K = 2*B*T), split-K slabs
    t.dwhh.A = w.dG; t.dwhh.sam = 1; t.dwhh.sak = 512; t.dwhh.B = w.pol.hprev; t.dwhh.sbk = 128; t.dwhh.sbn = 1; t.dwhh.ldc = 128;
    t.dwhh.M = 512; t.dwhh.N = 128; t.dwhh.K = 2 * rows;
    // dWih[512,128] = dgx^T * e
    t.dwih.A = dgx; t.dwih.A2 = dgx2; t.dwih.sam = 1; t.dwih.sak = 512; t.dwih.B = a.e_s(); t.dwih.sbk = 128; t.dwih.sbn = 1; t.dwih.ldc = 128;
    t.dwih.M = 512; t.dwih.N = 128; t.dwih.K = rows;
    // de[rows,128] = dgx * Wih
    t.de.A = dgx; t.de.A2 = dgx2; t.de.sam = 512; t.de.sak = 1; t.de.B = a.policy + O_WIH; t.de.sbk = 128; t.de.sbn = 1; t.de.C = w.de; t.de.ldc = 128;
    t.de.M = rows; t.de.N = 128; t.de.K = 512; t.de.splitk = 1;
    // da1[rows,128] = (de * W2) . (a1 > 0)
    t.da1.A = w.de; t.da1.sam = 128; t.da1.sak = 1; t.da1.B = a.policy + O_W2; t.da1.sbk = 128; t.da1.sbn = 1; t.da1.C = w.da1; t.da1.ldc = 128;
    t.da1.M = rows; t.da1.N = 128; t.da1.K = 128; t.da1.mask = a.a1_s(); t.da1.splitk = 1;
    // dW2[128,128] = de^T * a1 ; db2 = colsum(de)
    t.dw2.A = w.de; t.dw2.sam = 1; t.dw2.sak = 128; t.dw2.B = a.a1_s(); t.dw2.sbk = 128; t.dw2.sbn = 1; t.dw2.ldc = 128;
    t.dw2.M = 128; t.dw2.N = 128; t.dw2.K = rows;
    return t;
}
static int tuned_split(const char* key) { return std::min(WG_SPLIT_MAX, std::max(1, tune_get(key, WG_SPLIT))); }

// 3b. GEMM groups (DQN_TAIL off), on ONE stream as three launches (a fork / join pair costs ~20 us of stream time and the side
// stream's GEMMs took the CUs of the chain that everything else waits for):
//   1. {de (first in the grid: the chain below depends on it), dW3, dWhh slabs, dWih slabs}
//   2. {da1, dW2 slabs}: both read de and nothing of each other
//   3. column sums {dW4 <- w4term, db3 <- dd1c} and, split 8 ways over the rows, {db2 <- de} {db1, dW1 <- da1 weighted by x}
static ReduceGroup tail_gemm_groups(const LossGrad& a) {
    const DqnWs& w = a.w;
    const int B = a.B, rows = a.rows();
    TailGemms t = tail_gemms(a, w.dG, a.dG_bw());
    const int split_hh = tuned_split("DQN_SPLIT_HH"), split_ih = tuned_split("DQN_SPLIT_IH");
    t.dwhh.C = w.slabs_hh; t.dwhh.splitk = split_hh;
    t.dwih.C = w.slabs_ih; t.dwih.splitk = split_ih;
    t.dw2.C = w.slabs_w2; t.dw2.splitk = WG_SPLIT;
    const GemmF32 g1[4] = {t.de, t.dw3, t.dwhh, t.dwih};
    launch_gemm_f32_group(g1, 4, a.st);
    const GemmF32 g2[2] = {t.da1, t.dw2};
    launch_gemm_f32_group(g2, 2, a.st);
    constexpr int CS = CS_SPLIT;                    // row splits of the two long column sums
    float* cs_b2 = w.slabs_cs;                      // [CS][128]
    float* cs_b1 = w.slabs_cs + CS * 128;           // [CS][128]
    float* cs_w1 = w.slabs_cs + 2 * CS * 128;       // [CS][256]
    ColsumGroup c1{};                               // all four column sums in one launch (the two short ones unsplit)
    c1.j[0] = ColsumJob{w.de, nullptr, cs_b2, nullptr, rows, 128, 128, CS};
    c1.j[1] = ColsumJob{w.da1, a.state, cs_b1, cs_w1, rows, 128, 128, CS};
    c1.j[2] = ColsumJob{w.w4term, nullptr, a.grads + O_W4, nullptr, B, 128, 128, 1};
    c1.j[3] = ColsumJob{w.dd1c, nullptr, a.grads + O_B3, nullptr, B, 128, 128, 1};
    hipLaunchKernelGGL(colsum_group_kernel, dim3(4, 4, CS), dim3(1024), 0, a.st, c1);
    return tail_reduce_group(w, a.grads, split_hh, split_ih, WG_SPLIT);
}

// 3c. single launches on two streams (DQN_GROUP off): dgx is summed by a pass of its own, the decoder's and the recurrence's weight
// gradients run on the side stream beside the chain de -> da1, and every split-K GEMM is followed by its own reduction
static void tail_two_streams(const LossGrad& a, Fork& fk) {
    const DqnWs& w = a.w;
    const int B = a.B, rows = a.rows();
    hipStream_t st = a.st, s2 = fk.s2;
    float* grads = a.grads;
    const size_t n = (size_t)rows * 512;
    hipLaunchKernelGGL(add2_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, w.dG, a.dG_bw(), w.dgx, n);
    const TailGemms t = tail_gemms(a, w.dgx, nullptr);
    fk.fork(2);
    hipLaunchKernelGGL(colsum_kernel, dim3(4), dim3(1024), 0, s2, w.w4term, B, 128, 128, grads + O_W4);
    hipLaunchKernelGGL(colsum_kernel, dim3(4), dim3(1024), 0, s2, w.dd1c, B, 128, 128, grads + O_B3);
    launch_gemm_f32(t.dw3, s2);
    launch_gemm_f32_splitk(t.dwhh, grads + O_WHH, w.slabs_hh, tuned_split("DQN_SPLIT_HH"), s2);
    launch_gemm_f32_splitk(t.dwih, grads + O_WIH, w.slabs_hh, tuned_split("DQN_SPLIT_IH"), s2);
    launch_gemm_f32(t.de, st);
    launch_gemm_f32_splitk(t.dw2, grads + O_W2, w.slabs_w2, WG_SPLIT, st);
    hipLaunchKernelGGL(colsum_kernel, dim3(4), dim3(1024), 0, st, w.de, rows, 128, 128, grads + O_B2);
    launch_gemm_f32(t.da1, st);
    // dW1[128,2] = da1^T * x ; db1 = colsum(da1)
    GemmF32 g{};
    g.A = w.da1; g.sam = 1; g.sak = 128; g.B = a.state; g.sbk = 2; g.sbn = 1; g.ldc = 2;
    g.M = 128; g.N = 2; g.K = rows;
    launch_gemm_f32_splitk(g, grads + O_W1, w.slabs_w2, WG_SPLIT, st);
    hipLaunchKernelGGL(colsum_kernel, dim3(4), dim3(1024), 0, st, w.da1, rows, 128, 128, grads + O_B1);
    fk.join(3);
}

// defer != nullptr: the slab reduction is NOT launched; *defer describes it and the caller folds it into its update
static void backward_tail(const LossGrad& a, Fork& fk, ReduceGroup* defer) {
    if (!tune_get("DQN_GROUP", 1)) return tail_two_streams(a, fk);
    const ReduceGroup rg = tune_get("DQN_TAIL", 1) ? tail_resident(a) : tail_gemm_groups(a);
    if (defer) *defer = rg;
    else launch_reduce_group(rg, a.st);
}

// draw != nullptr: the minibatch is drawn and gathered by the encoder launch (state / new_state / action / rewards are then OUTPUTS
// of the step, written before anything reads them).  defer != nullptr: the fixed-order slab reduction is NOT launched; *defer
// describes it and the caller folds it into clamp + Adam (ivosw_dqn_step_drawn).  Either needs the fused launch chain
// (DQN_FUSED / DQN_GROUP / DQN_TAIL at their defaults): *folded says whether it was taken.
static int dqn_loss_grad_impl(LossGrad a, void* ws, size_t ws_bytes, ivosw_stream_t stream, const EncDraw* draw, ReduceGroup* defer,
                              bool* folded) {
    IVOSW_REQUIRE(a.policy && a.target && a.state && a.new_state && a.action && a.reward_step && a.reward_done && a.grads && a.loss && ws,
                  "null pointer");
    IVOSW_REQUIRE(a.B > 0 && a.T > 0, "B and T must be positive");
    if (const int rc = check_dqn_loss("ivosw_dqn_loss_grad", a.loss_kind, a.delta)) return rc;
    if (ws_bytes < ivosw_dqn_ws_bytes(a.B, a.T)) {
        set_error("ivosw_dqn_loss_grad: workspace %zu < %zu", ws_bytes, ivosw_dqn_ws_bytes(a.B, a.T));
        return IVOSW_ERR_WS;
    }
    if (folded) *folded = false;
    Arena ar(ws);
    a.w = carve_dqn(ar, a.B, a.T);
    a.st = as_stream(stream);
    Fork fk(a.st);
    const FwdPass passes[2] = {{a.policy, a.new_state, a.state, 2 * a.B, a.B, &a.w.pol}, {a.target, a.new_state, nullptr, a.B, 0, &a.w.tgt}};
    const bool fused = fused_forward_ok(passes, 2);
    const bool fold = (draw || defer) && fused && tune_get("DQN_GROUP", 1) && tune_get("DQN_TAIL", 1);
    if ((draw || defer) && !fold) return IVOSW_OK;    // the caller runs the un-folded sequence instead (nothing was launched)
    if (folded) *folded = fold;
    forward_and_head(a, passes, fused, draw, fk);
    bptt(a);
    backward_tail(a, fk, defer);
    if (!fk.sync_ok) {
        (void)hipGetLastError();
        set_error("ivosw_dqn_loss_grad: a fork/join event between the two streams failed");
        return IVOSW_ERR_LAUNCH;
    }
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}

extern "C" int ivosw_dqn_loss_grad_ex(const float* policy, const float* target, const float* state,
                                      const float* new_state, const int64_t* action, const float* reward_step,
                                      const float* reward_done, int B, int T, float gamma, int loss_kind, float huber_delta,
                                      float* grads, float* loss, void* ws, size_t ws_bytes, ivosw_stream_t stream) {
    IVOSW_REQUIRE(grads, "null pointer");
    IVOSW_ON_DEVICE_OF(grads);
    return dqn_loss_grad_impl(LossGrad{policy, target, state, new_state, action, reward_step, reward_done, B, T, gamma, loss_kind, huber_delta,
                                       grads, loss},
                              ws, ws_bytes, stream, nullptr, nullptr, nullptr);
}

extern "C" int ivosw_dqn_loss_grad_per(const float* policy, const float* target, const float* state,
                                       const float* new_state, const int64_t* action, const float* reward_step,
                                       const float* reward_done, int B, int T, float gamma, int loss_kind, float huber_delta,
                                       const float* weights, float* td_out, float* grads, float* loss, void* ws, size_t ws_bytes,
                                       ivosw_stream_t stream) {
    IVOSW_REQUIRE(grads && weights && td_out, "null pointer");
    IVOSW_ON_DEVICE_OF(grads);
    return dqn_loss_grad_impl(LossGrad{policy, target, state, new_state, action, reward_step, reward_done, B, T, gamma, loss_kind, huber_delta,
                                       grads, loss, weights, td_out},
                              ws, ws_bytes, stream, nullptr, nullptr, nullptr);
}

extern "C" int ivosw_dqn_loss_grad(const float* policy, const float* target, const float* state,
                                   const float* new_state, const int64_t* action, const float* reward_step,
                                   const float* reward_done, int B, int T, float gamma, float* grads, float* loss,
                                   void* ws, size_t ws_bytes, ivosw_stream_t stream) {
    return ivosw_dqn_loss_grad_ex(policy, target, state, new_state, action, reward_step, reward_done, B, T, gamma, IVOSW_DQN_LOSS_MSE, 1.0f,
                                  grads, loss, ws, ws_bytes, stream);
}

// The one-call step's tails: clamp_update (dqn_update.h) with the step's split-K slab reduction folded into the gradient load (SlabGrad:
// reduce_on_load), one wrapper per combination of rule, lr source and target; the stand-alone kernels of dqn.hip are the same body over
// ArenaGrad, so both give the same bits.  One element per lane, 177 workgroups: the slabs (13.5 MB at B = 128, T = 25, fresh in L2) are
// pulled by the whole chip — with the 45 workgroups of the 16-byte form the launch took 11 us, more than the reduction + update launches
// it replaces (5.3 + 5.1).
struct ReduceOffsets { int off[REDUCE_MAX]; };       // off[k] = element offset of slab set k in the gradient arena

__global__ __launch_bounds__(1024) void clamp_adam_dev_reduce_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                                     float* __restrict__ v, int n, AdamDevState* __restrict__ st, ReduceGroup rg,
                                                                     ReduceOffsets ro, float lr, float beta1, float beta2, float eps, float wd,
                                                                     float clampv, float gscale) {
    clamp_update<false>(p, n, AdamRule{m, v, st, beta1, beta2, eps, wd, clampv, gscale}, SlabGrad{g, rg, ro.off}, Lr<false>{lr}, NoTarget{});
}

// cfg.agent.lr_schedule = "poly"
__global__ __launch_bounds__(1024) void clamp_adam_dev_reduce_sched_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                                           float* __restrict__ v, int n, AdamDevState* __restrict__ st,
                                                                           ReduceGroup rg, ReduceOffsets ro, const float* __restrict__ lr_table,
                                                                           int lr_steps, float beta1, float beta2, float eps, float wd,
                                                                           float clampv, float gscale) {
    clamp_update<false>(p, n, AdamRule{m, v, st, beta1, beta2, eps, wd, clampv, gscale}, SlabGrad{g, rg, ro.off}, Lr<true>{0.f, lr_table, lr_steps},
                        NoTarget{});
}

// cfg.agent.optimizer = "sgd": no step counter, so no ticket; on the schedule the SGD state's
__global__ __launch_bounds__(1024) void clamp_sgd_reduce_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ buf, int n,
                                                                ReduceGroup rg, ReduceOffsets ro, float lr, float mu, float wd, int nesterov,
                                                                float clampv, float gscale) {
    clamp_update<false>(p, n, SgdRule{buf, nullptr, mu, wd, nesterov, clampv, gscale}, SlabGrad{g, rg, ro.off}, Lr<false>{lr}, NoTarget{});
}

__global__ __launch_bounds__(1024) void clamp_sgd_reduce_sched_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ buf,
                                                                      int n, SgdDevState* __restrict__ st, ReduceGroup rg, ReduceOffsets ro,
                                                                      const float* __restrict__ lr_table, int lr_steps, float mu, float wd,
                                                                      int nesterov, float clampv, float gscale) {
    clamp_update<false>(p, n, SgdRule{buf, st, mu, wd, nesterov, clampv, gscale}, SlabGrad{g, rg, ro.off}, Lr<true>{0.f, lr_table, lr_steps},
                        NoTarget{});
}

// The tails with the target-network rule fused in (cfg.agent.target_update = "soft" | "periodic", target.h): the thread that has just
// produced p_new also writes the target element, so the step keeps its eight launches.  The target arena was last read by the head
// kernel, earlier in the stream.  Both counters advance under one ticket: the Adam state's, the SGD state's on the schedule, and the
// target state's for the constant-lr SGD update, which has no counter of its own.
struct TargetArgs {
    float* t;
    TargetDevState* st;
    int mode;
    float tau;
    int period;
};

template <bool SCHED>
__global__ __launch_bounds__(1024) void adam_tail_tgt_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                             float* __restrict__ v, int n, AdamDevState* __restrict__ st, ReduceGroup rg,
                                                             ReduceOffsets ro, float lr_const, const float* __restrict__ lr_table, int lr_steps,
                                                             float beta1, float beta2, float eps, float wd, float clampv, float gscale,
                                                             TargetArgs ta) {
    clamp_update<false>(p, n, AdamRule{m, v, st, beta1, beta2, eps, wd, clampv, gscale}, SlabGrad{g, rg, ro.off},
                        Lr<SCHED>{lr_const, lr_table, lr_steps}, ta);
}

template <bool SCHED>
__global__ __launch_bounds__(1024) void sgd_tail_tgt_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ buf, int n,
                                                            SgdDevState* __restrict__ st, ReduceGroup rg, ReduceOffsets ro, float lr_const,
                                                            const float* __restrict__ lr_table, int lr_steps, float mu, float wd, int nesterov,
                                                            float clampv, float gscale, TargetArgs ta) {
    clamp_update<false>(p, n, SgdRule{buf, st, mu, wd, nesterov, clampv, gscale}, SlabGrad{g, rg, ro.off}, Lr<SCHED>{lr_const, lr_table, lr_steps},
                        ta);
}

// the tails' geometry: IVOSW_BRAIN_NPARAMS lanes in workgroups of 1024
template <class... Params, class... Args>
static void launch_tail(void (*kernel)(Params...), ivosw_stream_t stream, Args... args) {
    hipLaunchKernelGGL(kernel, dim3((IVOSW_BRAIN_NPARAMS + 1023) / 1024), dim3(1024), 0, as_stream(stream), args...);
}

// What the six one-call entries share, in the order of their signatures (include/ivosw.h).
struct StepIO {
    float* policy;
    const float *target, *old_iou, *new_iou, *annotated, *next_annotated;
    const int64_t* action;
    const float *reward_step, *reward_done;
    void* draw_state;
    int n, B, T;
    float gamma;
    int loss_kind;
    float huber_delta;
    int64_t* idx_out;
    float *state, *new_state;
    int64_t* action_out;
    float *reward_step_out, *reward_done_out, *grads, *loss;
    void* ws;
    size_t ws_bytes;
    ivosw_stream_t stream;
};

// The checks every entry makes of them, reported under the entry's name (the loss option under loss_who where that differs).
static int check_step_io(const char* who, const StepIO& io, const char* loss_who = nullptr) {
    const char* bad = nullptr;
    if (!(io.policy && io.target && io.old_iou && io.new_iou && io.annotated && io.next_annotated && io.action && io.reward_step &&
          io.reward_done && io.draw_state && io.idx_out && io.state && io.new_state && io.action_out && io.reward_step_out &&
          io.reward_done_out && io.grads && io.loss && io.ws))
        bad = "null pointer";
    else if (!(io.n > 0 && io.B > 0 && io.T > 0))
        bad = "n, B and T must be positive";
    if (bad) {
        set_error("%s: %s", who, bad);
        return IVOSW_ERR_ARG;
    }
    return check_dqn_loss(loss_who ? loss_who : who, io.loss_kind, io.huber_delta);
}

// The one path of every one-call step (the entry `who` has checked its arguments; `aligned`: its arenas are 16-byte aligned): the fused
// chain with the draw + gather in the encoder launch, then fold(rg, ro) launches the entry's tail; or, off the fused chain (a tunable
// moved the step off it), the same entries the caller would have made: draw + gather, loss + gradient, then unfold(), the update's own.
template <class Fold, class Unfold>
static int dqn_step_drawn_run(const char* who, bool aligned, const StepIO& io, Fold fold, Unfold unfold) {
    bool folded = false;
    if (aligned && tune_get("DQN_ONECALL", 1)) {
        const EncDraw dr{io.old_iou, io.new_iou, io.annotated, io.next_annotated, io.action, io.reward_step, io.reward_done,
                         static_cast<DrawState*>(io.draw_state), io.n, io.B, io.T, io.idx_out, io.state, io.new_state, io.action_out,
                         io.reward_step_out, io.reward_done_out};
        ReduceGroup rg{};
        const int rc = dqn_loss_grad_impl(LossGrad{io.policy, io.target, io.state, io.new_state, io.action_out, io.reward_step_out,
                                                   io.reward_done_out, io.B, io.T, io.gamma, io.loss_kind, io.huber_delta, io.grads, io.loss},
                                          io.ws, io.ws_bytes, io.stream, &dr, &rg, &folded);
        if (rc != IVOSW_OK) return rc;
        if (folded) {
            ReduceOffsets ro{};
            for (int k = 0; k < REDUCE_MAX; ++k) ro.off[k] = rg.out[k] ? (int)(rg.out[k] - io.grads) : 0;
            fold(rg, ro);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) {
                set_error("%s: HIP error %s", who, hipGetErrorString(e));
                return IVOSW_ERR_LAUNCH;
            }
            return IVOSW_OK;
        }
    }
    int rc = ivosw_replay_draw_gather(io.old_iou, io.new_iou, io.annotated, io.next_annotated, io.action, io.reward_step, io.reward_done,
                                      io.draw_state, io.n, io.B, io.T, io.idx_out, io.state, io.new_state, io.action_out, io.reward_step_out,
                                      io.reward_done_out, io.stream);
    if (rc == IVOSW_OK)
        rc = ivosw_dqn_loss_grad_ex(io.policy, io.target, io.state, io.new_state, io.action_out, io.reward_step_out, io.reward_done_out, io.B, io.T,
                                    io.gamma, io.loss_kind, io.huber_delta, io.grads, io.loss, io.ws, io.ws_bytes, io.stream);
    if (rc == IVOSW_OK) rc = unfold();
    return rc;
}

// Every entry below refuses bad arguments before anything is launched (the un-folded sequence would otherwise advance the draw counter first).
extern "C" int ivosw_dqn_step_drawn_ex(float* policy, const float* target, const float* old_iou, const float* new_iou, const float* annotated,
                                       const float* next_annotated, const int64_t* action, const float* reward_step, const float* reward_done,
                                       void* draw_state, int n, int B, int T, float gamma, int loss_kind, float huber_delta, int64_t* idx_out,
                                       float* state, float* new_state, int64_t* action_out, float* reward_step_out, float* reward_done_out,
                                       float* grads, float* loss, void* ws, size_t ws_bytes, float* exp_avg, float* exp_avg_sq, void* adam_state,
                                       float lr, float beta1, float beta2, float eps, float weight_decay, float clamp, float grad_scale,
                                       ivosw_stream_t stream) {
    const StepIO io{policy, target, old_iou, new_iou, annotated, next_annotated, action, reward_step, reward_done, draw_state, n, B, T, gamma,
                    loss_kind, huber_delta, idx_out, state, new_state, action_out, reward_step_out, reward_done_out, grads, loss, ws, ws_bytes, stream};
    IVOSW_REQUIRE(exp_avg && exp_avg_sq && adam_state, "null pointer");
    if (const int rc = check_step_io(__func__, io, "ivosw_dqn_step_drawn")) return rc;
    IVOSW_ON_DEVICE_OF(grads);
    const int nprm = IVOSW_BRAIN_NPARAMS;
    return dqn_step_drawn_run(
        __func__, aligned16({policy, grads, exp_avg, exp_avg_sq}), io,
        [&](const ReduceGroup& rg, const ReduceOffsets& ro) {
            launch_tail(clamp_adam_dev_reduce_kernel, stream, policy, grads, exp_avg, exp_avg_sq, nprm, static_cast<AdamDevState*>(adam_state), rg, ro,
                        lr, beta1, beta2, eps, weight_decay, clamp, grad_scale);
        },
        [&] {
            return ivosw_clamp_adam_dev(policy, grads, exp_avg, exp_avg_sq, nprm, adam_state, lr, beta1, beta2, eps, weight_decay, clamp, grad_scale,
                                        stream);
        });
}

// ivosw_dqn_step_drawn_ex with clamp + SGD in place of clamp + Adam: the same eight launches, the last one clamp_sgd_reduce_kernel.
extern "C" int ivosw_dqn_step_drawn_sgd(float* policy, const float* target, const float* old_iou, const float* new_iou, const float* annotated,
                                        const float* next_annotated, const int64_t* action, const float* reward_step, const float* reward_done,
                                        void* draw_state, int n, int B, int T, float gamma, int loss_kind, float huber_delta, int64_t* idx_out,
                                        float* state, float* new_state, int64_t* action_out, float* reward_step_out, float* reward_done_out,
                                        float* grads, float* loss, void* ws, size_t ws_bytes, float* momentum_buf, float lr, float momentum,
                                        float weight_decay, int nesterov, float clamp, float grad_scale, ivosw_stream_t stream) {
    const StepIO io{policy, target, old_iou, new_iou, annotated, next_annotated, action, reward_step, reward_done, draw_state, n, B, T, gamma,
                    loss_kind, huber_delta, idx_out, state, new_state, action_out, reward_step_out, reward_done_out, grads, loss, ws, ws_bytes, stream};
    IVOSW_REQUIRE(momentum_buf, "null pointer");
    if (const int rc = check_step_io(__func__, io)) return rc;
    if (const int rc = check_sgd(__func__, lr, momentum, weight_decay, nesterov)) return rc;
    IVOSW_ON_DEVICE_OF(grads);
    const int nprm = IVOSW_BRAIN_NPARAMS;
    return dqn_step_drawn_run(
        __func__, aligned16({policy, grads, momentum_buf}), io,
        [&](const ReduceGroup& rg, const ReduceOffsets& ro) {
            launch_tail(clamp_sgd_reduce_kernel, stream, policy, grads, momentum_buf, nprm, rg, ro, lr, momentum, weight_decay, nesterov, clamp,
                        grad_scale);
        },
        [&] { return ivosw_clamp_sgd(policy, grads, momentum_buf, nprm, lr, momentum, weight_decay, nesterov, clamp, grad_scale, stream); });
}

// ivosw_dqn_step_drawn_ex with the poly learning-rate schedule: the same eight launches, the last one clamp_adam_dev_reduce_sched_kernel.
extern "C" int ivosw_dqn_step_drawn_sched(float* policy, const float* target, const float* old_iou, const float* new_iou, const float* annotated,
                                          const float* next_annotated, const int64_t* action, const float* reward_step, const float* reward_done,
                                          void* draw_state, int n, int B, int T, float gamma, int loss_kind, float huber_delta, int64_t* idx_out,
                                          float* state, float* new_state, int64_t* action_out, float* reward_step_out, float* reward_done_out,
                                          float* grads, float* loss, void* ws, size_t ws_bytes, float* exp_avg, float* exp_avg_sq, void* adam_state,
                                          const float* lr_table, int lr_steps, float beta1, float beta2, float eps, float weight_decay, float clamp,
                                          float grad_scale, ivosw_stream_t stream) {
    const StepIO io{policy, target, old_iou, new_iou, annotated, next_annotated, action, reward_step, reward_done, draw_state, n, B, T, gamma,
                    loss_kind, huber_delta, idx_out, state, new_state, action_out, reward_step_out, reward_done_out, grads, loss, ws, ws_bytes, stream};
    IVOSW_REQUIRE(exp_avg && exp_avg_sq && adam_state, "null pointer");
    if (const int rc = check_step_io(__func__, io)) return rc;
    if (const int rc = check_lr_table(__func__, lr_table, lr_steps)) return rc;
    if (const int rc = check_adam(__func__, beta1, beta2, eps, weight_decay)) return rc;
    IVOSW_ON_DEVICE_OF(grads);
    const int nprm = IVOSW_BRAIN_NPARAMS;
    return dqn_step_drawn_run(
        __func__, aligned16({policy, grads, exp_avg, exp_avg_sq}), io,
        [&](const ReduceGroup& rg, const ReduceOffsets& ro) {
            launch_tail(clamp_adam_dev_reduce_sched_kernel, stream, policy, grads, exp_avg, exp_avg_sq, nprm, static_cast<AdamDevState*>(adam_state),
                        rg, ro, lr_table, lr_steps, beta1, beta2, eps, weight_decay, clamp, grad_scale);
        },
        [&] {
            return ivosw_clamp_adam_dev_sched(policy, grads, exp_avg, exp_avg_sq, nprm, adam_state, lr_table, lr_steps, beta1, beta2, eps,
                                              weight_decay, clamp, grad_scale, stream);
        });
}

// ivosw_dqn_step_drawn_sgd with the poly learning-rate schedule: the same eight launches, the last one clamp_sgd_reduce_sched_kernel.
extern "C" int ivosw_dqn_step_drawn_sgd_sched(float* policy, const float* target, const float* old_iou, const float* new_iou,
                                              const float* annotated, const float* next_annotated, const int64_t* action, const float* reward_step,
                                              const float* reward_done, void* draw_state, int n, int B, int T, float gamma, int loss_kind,
                                              float huber_delta, int64_t* idx_out, float* state, float* new_state, int64_t* action_out,
                                              float* reward_step_out, float* reward_done_out, float* grads, float* loss, void* ws, size_t ws_bytes,
                                              float* momentum_buf, void* sgd_state, const float* lr_table, int lr_steps, float momentum,
                                              float weight_decay, int nesterov, float clamp, float grad_scale, ivosw_stream_t stream) {
    const StepIO io{policy, target, old_iou, new_iou, annotated, next_annotated, action, reward_step, reward_done, draw_state, n, B, T, gamma,
                    loss_kind, huber_delta, idx_out, state, new_state, action_out, reward_step_out, reward_done_out, grads, loss, ws, ws_bytes, stream};
    IVOSW_REQUIRE(momentum_buf && sgd_state, "null pointer");
    if (const int rc = check_step_io(__func__, io)) return rc;
    if (const int rc = check_lr_table(__func__, lr_table, lr_steps)) return rc;
    if (const int rc = check_sgd(__func__, 0.f, momentum, weight_decay, nesterov)) return rc;
    IVOSW_ON_DEVICE_OF(grads);
    const int nprm = IVOSW_BRAIN_NPARAMS;
    return dqn_step_drawn_run(
        __func__, aligned16({policy, grads, momentum_buf}), io,
        [&](const ReduceGroup& rg, const ReduceOffsets& ro) {
            launch_tail(clamp_sgd_reduce_sched_kernel, stream, policy, grads, momentum_buf, nprm, static_cast<SgdDevState*>(sgd_state), rg, ro,
                        lr_table, lr_steps, momentum, weight_decay, nesterov, clamp, grad_scale);
        },
        [&] {
            return ivosw_clamp_sgd_dev_sched(policy, grads, momentum_buf, nprm, sgd_state, lr_table, lr_steps, momentum, weight_decay, nesterov,
                                             clamp, grad_scale, stream);
        });
}

// The one-call step of any optimizer with the target-network rule in its last launch (cfg.agent.target_update = "soft" | "periodic"): the
// eight launches of ivosw_dqn_step_drawn_{ex,sgd,sched,sgd_sched}, the last one adam_tail_tgt_kernel / sgd_tail_tgt_kernel, which also
// writes `target`.  optimizer: IVOSW_OPT_ADAM (opt_buf0 / opt_buf1 = exp_avg / exp_avg_sq, opt_state = the Adam state; beta1, beta2, eps) or
// IVOSW_OPT_SGD (opt_buf0 = the momentum buffer, opt_buf1 unused; momentum, nesterov; opt_state = the SGD state, needed on the schedule
// only).  lr_table NULL: the constant `lr`; else the poly schedule's table of lr_steps + 1 entries (`lr` unused).  Off the fused chain: the
// draw + gather, loss + gradient and update entries, then ivosw_target_update — the same results.
extern "C" int ivosw_dqn_step_drawn_tgt(float* policy, float* target, const float* old_iou, const float* new_iou, const float* annotated,
                                        const float* next_annotated, const int64_t* action, const float* reward_step, const float* reward_done,
                                        void* draw_state, int n, int B, int T, float gamma, int loss_kind, float huber_delta, int64_t* idx_out,
                                        float* state, float* new_state, int64_t* action_out, float* reward_step_out, float* reward_done_out,
                                        float* grads, float* loss, void* ws, size_t ws_bytes, int optimizer, float* opt_buf0, float* opt_buf1,
                                        void* opt_state, float lr, const float* lr_table, int lr_steps, float beta1, float beta2, float eps,
                                        float momentum, int nesterov, float weight_decay, float clamp, float grad_scale, int target_mode,
                                        float tau, int target_period, void* target_state, ivosw_stream_t stream) {
    static const char* who = "ivosw_dqn_step_drawn_tgt";
    const StepIO io{policy, target, old_iou, new_iou, annotated, next_annotated, action, reward_step, reward_done, draw_state, n, B, T, gamma,
                    loss_kind, huber_delta, idx_out, state, new_state, action_out, reward_step_out, reward_done_out, grads, loss, ws, ws_bytes, stream};
    if (const int rc = check_target(who, target_state, target_mode, tau, target_period)) return rc;
    IVOSW_REQUIRE(optimizer == IVOSW_OPT_ADAM || optimizer == IVOSW_OPT_SGD, "unknown optimizer (IVOSW_OPT_ADAM or IVOSW_OPT_SGD)");
    const bool adam = optimizer == IVOSW_OPT_ADAM, sched = lr_table != nullptr;
    IVOSW_REQUIRE(opt_buf0, "null pointer");
    IVOSW_REQUIRE(!adam || (opt_buf1 && opt_state), "null pointer (Adam needs exp_avg_sq and its state)");
    IVOSW_REQUIRE(adam || !sched || opt_state, "null pointer (scheduled SGD needs its state)");
    if (const int rc = check_step_io(who, io)) return rc;
    IVOSW_REQUIRE(target != policy, "target and policy must be different arenas");
    if (sched)
        if (const int rc = check_lr_table(who, lr_table, lr_steps)) return rc;
    if (adam) {
        if (const int rc = check_adam(who, beta1, beta2, eps, weight_decay)) return rc;
    } else {
        if (const int rc = check_sgd(who, sched ? 0.f : lr, momentum, weight_decay, nesterov)) return rc;
    }
    IVOSW_ON_DEVICE_OF(grads);
    const bool aligned = aligned16({policy, grads, opt_buf0, adam ? opt_buf1 : nullptr});
    if (target_mode == TARGET_SOFT) target_period = 1;      // not looked at under soft; keeps any value off the kernel's modulo
    const TargetArgs ta{target, static_cast<TargetDevState*>(target_state), target_mode, tau, target_period};
    const int nprm = IVOSW_BRAIN_NPARAMS;
    return dqn_step_drawn_run(
        who, aligned, io,
        [&](const ReduceGroup& rg, const ReduceOffsets& ro) {
            if (adam)
                launch_tail(sched ? adam_tail_tgt_kernel<true> : adam_tail_tgt_kernel<false>, stream, policy, grads, opt_buf0, opt_buf1, nprm,
                            static_cast<AdamDevState*>(opt_state), rg, ro, lr, lr_table, lr_steps, beta1, beta2, eps, weight_decay, clamp, grad_scale,
                            ta);
            else
                launch_tail(sched ? sgd_tail_tgt_kernel<true> : sgd_tail_tgt_kernel<false>, stream, policy, grads, opt_buf0, nprm,
                            static_cast<SgdDevState*>(opt_state), rg, ro, lr, lr_table, lr_steps, momentum, weight_decay, nesterov, clamp,
                            grad_scale, ta);
        },
        [&] {
            int rc;
            if (adam && sched)
                rc = ivosw_clamp_adam_dev_sched(policy, grads, opt_buf0, opt_buf1, nprm, opt_state, lr_table, lr_steps, beta1, beta2, eps, weight_decay,
                                                clamp, grad_scale, stream);
            else if (adam)
                rc = ivosw_clamp_adam_dev(policy, grads, opt_buf0, opt_buf1, nprm, opt_state, lr, beta1, beta2, eps, weight_decay, clamp, grad_scale,
                                          stream);
            else if (sched)
                rc = ivosw_clamp_sgd_dev_sched(policy, grads, opt_buf0, nprm, opt_state, lr_table, lr_steps, momentum, weight_decay, nesterov, clamp,
                                               grad_scale, stream);
            else
                rc = ivosw_clamp_sgd(policy, grads, opt_buf0, nprm, lr, momentum, weight_decay, nesterov, clamp, grad_scale, stream);
            if (rc == IVOSW_OK) rc = ivosw_target_update(target, policy, nprm, target_mode, tau, target_period, target_state, stream);
            return rc;
        });
}

extern "C" int ivosw_dqn_step_drawn(float* policy, const float* target, const float* old_iou, const float* new_iou, const float* annotated,
                                    const float* next_annotated, const int64_t* action, const float* reward_step, const float* reward_done,
                                    void* draw_state, int n, int B, int T, float gamma, int64_t* idx_out, float* state, float* new_state,
                                    int64_t* action_out, float* reward_step_out, float* reward_done_out, float* grads, float* loss, void* ws,
                                    size_t ws_bytes, float* exp_avg, float* exp_avg_sq, void* adam_state, float lr, float beta1, float beta2,
                                    float eps, float weight_decay, float clamp, float grad_scale, ivosw_stream_t stream) {
    return ivosw_dqn_step_drawn_ex(policy, target, old_iou, new_iou, annotated, next_annotated, action, reward_step, reward_done, draw_state, n, B,
                                   T, gamma, IVOSW_DQN_LOSS_MSE, 1.0f, idx_out, state, new_state, action_out, reward_step_out, reward_done_out,
                                   grads, loss, ws, ws_bytes, exp_avg, exp_avg_sq, adam_state, lr, beta1, beta2, eps, weight_decay, clamp,
                                   grad_scale, stream);
}

#ifdef IVOSW_PROBES
// ---------------------------------------------------------------- test probes of the backward kernels (include/ivosw_probe.h)
extern "C" int ivosw_bwd_wgrad_probe(const float* A, const float* A2, const float* B, float* C, int lda, int ldb, int M, int N, int K,
                                     int nslab, int kind, int* used, ivosw_stream_t stream) {
    IVOSW_REQUIRE(A && B && C, "null pointer");
    PROBE_COVERS(M >= 64 && M % 64 == 0, "M must be a multiple of 64");
    PROBE_COVERS(N >= 128 && N % 128 == 0, "N must be a multiple of 128");
    PROBE_COVERS(K >= 1, "K must be at least 1");
    PROBE_COVERS(lda >= M && ldb >= N && lda % 4 == 0 && ldb % 4 == 0, "lda >= M, ldb >= N, both multiples of 4");
    PROBE_COVERS(aligned16({A, A2, B, C}), "operands must be 16-byte aligned");
    PROBE_COVERS(nslab >= 0 && nslab <= 64, "nslab must be 0 .. 64");
    PROBE_COVERS(nslab > 0 || (kind >= 0 && kind <= 2), "kind must be 0 (dW_hh), 1 (dW_ih) or 2 (dW2) when nslab == 0");
    IVOSW_ON_DEVICE_OF(C);
    if (nslab == 0) nslab = tail_slabs_for(K, kind);
    TailGroup t{};
    t.w[0] = WgradJob{A, A2, B, C, lda, ldb, M, N, K, nslab};
    t.n = 1;
    for (int i = 1; i <= TAIL_MAX; ++i) t.first[i] = (M / 64) * (N / 128) * nslab;
    hipLaunchKernelGGL(bwd_tail_kernel, dim3(t.first[1]), dim3(256), 0, as_stream(stream), t);
    IVOSW_CHECK_LAUNCH();
    if (used) *used = nslab;
    return IVOSW_OK;
}

extern "C" int ivosw_bwd_dgrad_probe(const float* dG, const float* dG2, const float* wih, const float* w2, const float* a1, float* de,
                                     float* da1, int rows, ivosw_stream_t stream) {
    IVOSW_REQUIRE(dG && dG2 && wih && w2 && a1 && de && da1, "null pointer");
    PROBE_COVERS(rows >= 1, "rows must be at least 1");
    PROBE_COVERS(aligned16({dG, dG2, wih, w2, a1, de, da1}), "operands must be 16-byte aligned");
    IVOSW_ON_DEVICE_OF(de);
    TailGroup t{};
    t.dg = DgradArgs{dG, dG2, wih, w2, a1, de, da1, rows};
    t.n_dgrad = ((rows + 15) / 16 + 7) / 8 * 8;
    hipLaunchKernelGGL(bwd_tail_kernel, dim3(t.n_dgrad), dim3(256), 0, as_stream(stream), t);
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}

extern "C" int ivosw_bwd_csum_probe(const float* A, const float* x, float* out, float* outw, int M, int N, int ld, int nsplit,
                                    ivosw_stream_t stream) {
    IVOSW_REQUIRE(A && out, "null pointer");
    IVOSW_REQUIRE((x == nullptr) == (outw == nullptr), "x and outw go together");
    PROBE_COVERS(M >= 1 && N >= 1 && ld >= N, "M >= 1 and 1 <= N <= ld");
    PROBE_COVERS(nsplit >= 1 && nsplit <= 64, "nsplit must be 1 .. 64");
    PROBE_COVERS((reinterpret_cast<uintptr_t>(x) & 7) == 0, "x must be 8-byte aligned");
    IVOSW_ON_DEVICE_OF(out);
    TailGroup t{};
    t.cs[0] = CsumJob{A, x, out, outw, M, N, ld, nsplit};
    t.n_cs = 1;
    for (int i = 1; i <= TAIL_MAX; ++i) t.cs_first[i] = ((N + 31) / 32) * nsplit;
    hipLaunchKernelGGL(bwd_tail_kernel, dim3(t.cs_first[1]), dim3(256), 0, as_stream(stream), t);
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}

static_assert(IVOSW_BWD_GROUP_WS_FLOATS == TAIL_SLABS_FLOATS, "the group probe's scratch holds the step's slab sets");
static_assert(SLABS_W2_FLOATS % 64 == 0 && SLABS_LONGK_FLOATS % 64 == 0, "the slab sets follow each other without padding");
extern "C" int ivosw_bwd_group_probe(const float* dG, const float* hprev, const float* e, const float* a1, const float* dd1c, const float* hcc,
                                     const float* w4term, const float* state, const float* wih, const float* w2, float* de, float* da1,
                                     float* grads, float* ws, int B, int T, ivosw_stream_t stream) {
    IVOSW_REQUIRE(dG && hprev && e && a1 && dd1c && hcc && w4term && state && wih && w2 && de && da1 && grads && ws, "null pointer");
    PROBE_COVERS(B >= 1 && T >= 1 && (long long)B * T <= (1 << 20), "B, T >= 1 and B*T <= 2^20");
    PROBE_COVERS(aligned16({dG, hprev, e, a1, dd1c, hcc, w4term, wih, w2, de, da1, grads, ws}) && (reinterpret_cast<uintptr_t>(state) & 7) == 0,
                 "operands must be 16-byte aligned (state: 8)");
    IVOSW_ON_DEVICE_OF(grads);
    hipStream_t st = as_stream(stream);
    Arena ar(ws);
    const TailSlabs s = carve_tail_slabs(ar);
    const TailPlan pl = plan_bwd_tail(TailIO{dG, dG + (size_t)B * T * 512, hprev, e, a1, dd1c, hcc, w4term, state, wih, w2, de, da1, s.slabs_hh,
                                             s.slabs_ih, s.slabs_w2, s.slabs_cs, grads, B, T});
    launch_bwd_tail(pl, st);
    launch_reduce_group(tail_reduce_group(s, grads, pl.split_hh, pl.split_ih, pl.split_w2), st);
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}

extern "C" int ivosw_head_fused_probe(const float* prm, int o_w3, int o_w4, const float* q_np, const float* q_nt, const float* q_s,
                                      const int64_t* action, const float* r_step, const float* r_done, int B, int T, float gamma, int loss_kind,
                                      float delta, const float* d1_s, const float* hs_s, float* dq, float* dd1c, float* w4term, float* hcc,
                                      float* dhc, float* loss, float* db4, int per, const float* weights, float* td, ivosw_stream_t stream) {
    IVOSW_REQUIRE(prm && q_np && q_nt && q_s && action && r_step && r_done && d1_s && hs_s && dq && dd1c && w4term && hcc && dhc && loss && db4,
                  "null pointer");
    IVOSW_REQUIRE(!per || (weights && td), "null pointer (weights, td)");
    PROBE_COVERS(B >= 1 && T >= 1 && o_w3 >= 0 && o_w4 >= 0, "B, T >= 1 and offsets >= 0");
    if (const int rc = check_dqn_loss(__func__, loss_kind, delta)) return rc;
    IVOSW_ON_DEVICE_OF(dq);
    hipStream_t st = as_stream(stream);
    if (per)
        hipLaunchKernelGGL(head_fused_kernel<true>, dim3(B), dim3(256), 0, st, prm, o_w3, o_w4, q_np, q_nt, q_s, action, r_step, r_done, B, T, gamma,
                           loss_kind, delta, d1_s, hs_s, dq, dd1c, w4term, hcc, dhc, loss, db4, weights, td);
    else
        hipLaunchKernelGGL(head_fused_kernel<false>, dim3(B), dim3(256), 0, st, prm, o_w3, o_w4, q_np, q_nt, q_s, action, r_step, r_done, B, T, gamma,
                           loss_kind, delta, d1_s, hs_s, dq, dd1c, w4term, hcc, dhc, loss, db4, nullptr, nullptr);
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}

extern "C" int ivosw_lstm_bwd_probe(const float* whh, const float* gates, const float* cs, const float* dhc, const int64_t* action, float* dG,
                                    int N, int T, int form, ivosw_stream_t stream) {
    IVOSW_REQUIRE(whh && gates && cs && dhc && action && dG, "null pointer");
    PROBE_COVERS(N >= 1 && T >= 1 && (long long)N * T <= (1 << 20), "N, T >= 1 and N*T <= 2^20");
    PROBE_COVERS(form == 0 || form == 1 || form == 2 || form == 4, "form must be 0 (quad), 1, 2 or 4 (rows per workgroup)");
    IVOSW_ON_DEVICE_OF(dG);
    hipStream_t st = as_stream(stream);
    LstmBwd lb{};
    lb.whh = whh; lb.gates = gates; lb.cs = cs; lb.dhc = dhc; lb.action = action; lb.dG = dG; lb.N = N; lb.T = T; lb.ts = nullptr;
    const int R = form ? form : 1, nwg = (2 * N + R - 1) / R;
    if (form == 0) hipLaunchKernelGGL(lstm_bwd_quad_kernel<1>, dim3(2 * N), dim3(512), 0, st, lb);
    else if (form == 1) hipLaunchKernelGGL(lstm_bwd_kernel<1>, dim3(nwg), dim3(512), 0, st, lb);
    else if (form == 2) hipLaunchKernelGGL(lstm_bwd_kernel<2>, dim3(nwg), dim3(512), 0, st, lb);
    else hipLaunchKernelGGL(lstm_bwd_kernel<4>, dim3(nwg), dim3(512), 0, st, lb);
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}
#endif  // IVOSW_PROBES
