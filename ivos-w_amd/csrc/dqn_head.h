// The Double-DQN head of a step (dqn_step.hip launches it): the loss terms, the head of the fused chain (tunable DQN_FUSED, see
// brain_fused.h) and the two kernels of the un-fused chain.
#pragma once
#include "brain_fwd.h"

namespace ivosw {

// The per-sample loss terms of the DQN head (IVOSW_DQN_LOSS_*, include/ivosw.h).  MSE: e1^2 + e2^2 and dL/dQsa = 2 (e1 + e2) / B, the
// expressions models/agent.py:149-151 differentiates.  Huber with threshold delta (torch.nn.functional.huber_loss, mean): h(e) = e^2 / 2
// for |e| < delta, else delta (|e| - delta / 2), and dL/dQsa = (clamp(e1) + clamp(e2)) / B with clamp to [-delta, delta].
__device__ __forceinline__ float dqn_huber(float e, float delta) {
    const float a = fabsf(e);
    return a < delta ? 0.5f * e * e : delta * (a - 0.5f * delta);
}
__device__ __forceinline__ float dqn_loss_terms(int kind, float delta, float e1, float e2) {
    if (kind == IVOSW_DQN_LOSS_HUBER) return dqn_huber(e1, delta) + dqn_huber(e2, delta);
    return e1 * e1 + e2 * e2;
}
__device__ __forceinline__ float dqn_dq(int kind, float delta, int B, float e1, float e2) {
    if (kind == IVOSW_DQN_LOSS_HUBER) return (1.0f / (float)B) * (fminf(fmaxf(e1, -delta), delta) + fminf(fmaxf(e2, -delta), delta));
    return (2.0f / (float)B) * (e1 + e2);
}
// Prioritized replay: a row's importance-sampling weight w scales its loss terms as one rounded product (never an fma with the sum it
// feeds), and its dL/dQsa as dqn_dq with w folded into the constant factor, (w c) s: the expression shape of dqn_dq, so that w = 1 gives
// dqn_dq's bits wherever the compiler contracts the sum the value feeds (the db4 sums do).
__device__ __forceinline__ float per_weighted(float w, float x) {
#pragma clang fp contract(off)
    return w * x;
}
// td = |e1| + |e2| for the priority update.  The errors pass through an empty asm first: without it the two-element sum lets the SLP
// vectorizer pair the computations of e1 and e2, which drops a contraction the unweighted head has (and moves e2 by an ulp).
__device__ __forceinline__ float per_td(float e1, float e2) {
    asm volatile("" : "+v"(e1), "+v"(e2));
    return fabsf(e1) + fabsf(e2);
}
__device__ __forceinline__ float dqn_dq_w(int kind, float delta, int B, float e1, float e2, float w) {
    if (kind == IVOSW_DQN_LOSS_HUBER) return (w * (1.0f / (float)B)) * (fminf(fmaxf(e1, -delta), delta) + fminf(fmaxf(e2, -delta), delta));
    return (w * (2.0f / (float)B)) * (e1 + e2);
}

// One workgroup per sample b: Double-DQN target (first maximum of the policy's Q over s', the target net's Q there), the two
// loss terms' gradient dL/dQ(s, a) (dqn_dq), then the decoder backward on row (b, a): dd1 = dq w4 . (d1 > 0), the dW4 term dq d1,
// relu(h) for dW3, and dL/dh = (dd1 W3) . (h > 0) as a 128-long dot product per thread.  Block 0 also forms the batch
// sums (loss, db4) with the reduction tree of dqn_head_kernel.
// PER (prioritized replay): row b's loss terms and dL/dQsa are scaled by weights[b], and td[b] = |e1| + |e2|; PER = false is the
// unweighted kernel, unchanged (weights and td are not read).
template <bool PER>
__global__ __launch_bounds__(256) void head_fused_kernel(const float* __restrict__ prm, int o_w3, int o_w4,
                                                         const float* __restrict__ q_np, const float* __restrict__ q_nt,
                                                         const float* __restrict__ q_s, const int64_t* __restrict__ action,
                                                         const float* __restrict__ r_step, const float* __restrict__ r_done,
                                                         int B, int T, float gamma, int loss_kind, float delta,
                                                         const float* __restrict__ d1_s,
                                                         const float* __restrict__ hs_s, float* __restrict__ dq,
                                                         float* __restrict__ dd1c, float* __restrict__ w4term,
                                                         float* __restrict__ hcc, float* __restrict__ dhc,
                                                         float* __restrict__ loss, float* __restrict__ db4,
                                                         const float* __restrict__ weights, float* __restrict__ td) {
    __shared__ float dd_s[128];
    __shared__ float d_sh;
    __shared__ float red[2][256];
    const int b = blockIdx.x, tid = threadIdx.x;
    int a = (int)action[b];
    a = min(max(a, 0), T - 1);
    // Everything that does not depend on the argmax is requested up front (the kernel is a chain of L2 round trips
    // otherwise): this thread's column of W3 (128 registers), the loss row of d1 / h, the scalars of the targets.
    float w3c[128];
    {
        const float* w = prm + o_w3 + tid;
#pragma unroll
        for (int j = 0; j < 128; ++j) w3c[j] = w[(size_t)j * 256];
    }
    const size_t row = (size_t)b * T + a;
    const float hv = hs_s[row * 256 + tid];
    const float d1v = tid < 128 ? d1_s[row * 128 + tid] : 0.f;
    const float w4v = tid < 128 ? prm[o_w4 + tid] : 0.f;
    const float rs = r_step[b], rd = r_done[b], qsa = q_s[(size_t)b * T + a];
    __builtin_amdgcn_sched_barrier(0);
    if (tid < 64) {
        const float* qp = q_np + (size_t)b * T;
        float best = -INFINITY;
        int am = 0x7fffffff;
        for (int t = tid; t < T; t += 64) {
            const float v = qp[t];
            if (v > best || am == 0x7fffffff) { best = v; am = t; }     // first maximum of this lane's frames
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ob = __shfl_xor(best, o, 64);
            const int oa = __shfl_xor(am, o, 64);
            if (oa != 0x7fffffff && (am == 0x7fffffff || ob > best || (ob == best && oa < am))) { best = ob; am = oa; }
        }
        if (tid == 0) {
            const float qn = q_nt[(size_t)b * T + am];
            const float y1 = qn * gamma + rs * 0.1f;
            const float y2 = rd * 0.1f;
            const float e1 = qsa - y1, e2 = qsa - y2;
            float d;
            if (PER) {
                d = dqn_dq_w(loss_kind, delta, B, e1, e2, weights[b]);
                td[b] = per_td(e1, e2);
            } else {
                d = dqn_dq(loss_kind, delta, B, e1, e2);
            }
            d_sh = d;
            dq[b] = d;
        }
    }
    __syncthreads();
    const float d = d_sh;
    if (tid < 128) {
        w4term[(size_t)b * 128 + tid] = d * d1v;
        const float dd = (d1v > 0.f) ? d * w4v : 0.f;
        dd1c[(size_t)b * 128 + tid] = dd;
        dd_s[tid] = dd;
    }
    const float h = fmaxf(hv, 0.f);
    hcc[(size_t)b * 256 + tid] = h;
    __syncthreads();
    {
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
        for (int j = 0; j < 128; j += 4) {
            a0 = fmaf(dd_s[j], w3c[j], a0);
            a1 = fmaf(dd_s[j + 1], w3c[j + 1], a1);
            a2 = fmaf(dd_s[j + 2], w3c[j + 2], a2);
            a3 = fmaf(dd_s[j + 3], w3c[j + 3], a3);
        }
        dhc[(size_t)b * 256 + tid] = (h > 0.f) ? (a0 + a1) + (a2 + a3) : 0.f;
    }
    if (b != 0) return;
    // batch sums, the arithmetic and order of dqn_head_kernel
    float l = 0.f, sdq = 0.f;
    for (int s = tid; s < B; s += 256) {
        const float* qp = q_np + (size_t)s * T;
        int am = 0;
        float best = qp[0];
        for (int t = 1; t < T; ++t) {
            const float v = qp[t];
            if (v > best) { best = v; am = t; }
        }
        const float qn = q_nt[(size_t)s * T + am];
        const float y1 = qn * gamma + r_step[s] * 0.1f;
        const float y2 = r_done[s] * 0.1f;
        int as = (int)action[s];
        as = min(max(as, 0), T - 1);
        const float qsa = q_s[(size_t)s * T + as];
        const float e1 = qsa - y1, e2 = qsa - y2;
        if (PER) {
            const float w = weights[s];
            l += per_weighted(w, dqn_loss_terms(loss_kind, delta, e1, e2));
            sdq += dqn_dq_w(loss_kind, delta, B, e1, e2, w);
        } else {
            l += dqn_loss_terms(loss_kind, delta, e1, e2);
            sdq += dqn_dq(loss_kind, delta, B, e1, e2);
        }
    }
    red[0][tid] = l;
    red[1][tid] = sdq;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            red[0][tid] += red[0][tid + o];
            red[1][tid] += red[1][tid + o];
        }
        __syncthreads();
    }
    if (tid == 0) {
        *loss = red[0][0] / (float)B;
        *db4 = red[1][0];
    }
}

// ---------------------------------------------------------------- DQN head: targets, loss, dQ
// one block; q_next_pol/q_next_tgt/q_state are [B,T].  PER: the weighted head of head_fused_kernel<true> (weights [B] in, td [B] out).
template <bool PER>
__global__ __launch_bounds__(256) void dqn_head_kernel(const float* __restrict__ q_np, const float* __restrict__ q_nt,
                                                       const float* __restrict__ q_s, const int64_t* __restrict__ action,
                                                       const float* __restrict__ r_step, const float* __restrict__ r_done,
                                                       int B, int T, float gamma, int loss_kind, float delta,
                                                       float* __restrict__ dq, float* __restrict__ loss, float* __restrict__ db4,
                                                       const float* __restrict__ weights, float* __restrict__ td) {
    __shared__ float red[2][256];
    float l = 0.f, sdq = 0.f;
    for (int b = threadIdx.x; b < B; b += 256) {
        const float* qp = q_np + (size_t)b * T;
        int am = 0;
        float best = qp[0];
        for (int t = 1; t < T; ++t) {
            const float v = qp[t];
            if (v > best) { best = v; am = t; }  // first maximum (torch CPU max(1)[1])
        }
        const float qn = q_nt[(size_t)b * T + am];
        const float y1 = qn * gamma + r_step[b] * 0.1f;
        const float y2 = r_done[b] * 0.1f;
        int a = (int)action[b];
        a = min(max(a, 0), T - 1);
        const float qsa = q_s[(size_t)b * T + a];
        const float e1 = qsa - y1, e2 = qsa - y2;
        if (PER) {
            const float w = weights[b];
            l += per_weighted(w, dqn_loss_terms(loss_kind, delta, e1, e2));
            const float d = dqn_dq_w(loss_kind, delta, B, e1, e2, w);
            dq[b] = d;
            sdq += d;
            td[b] = per_td(e1, e2);
            continue;
        }
        l += dqn_loss_terms(loss_kind, delta, e1, e2);
        const float d = dqn_dq(loss_kind, delta, B, e1, e2);
        dq[b] = d;
        sdq += d;
    }
    red[0][threadIdx.x] = l;
    red[1][threadIdx.x] = sdq;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) {
            red[0][threadIdx.x] += red[0][threadIdx.x + o];
            red[1][threadIdx.x] += red[1][threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        *loss = red[0][0] / (float)B;
        *db4 = red[1][0];
    }
}

// per sample b (grid B, 128 threads): the decoder backward touches only row (b, action[b])
__global__ __launch_bounds__(128) void dec_bwd_rows_kernel(const float* __restrict__ prm, const float* __restrict__ dq,
                                                           const int64_t* __restrict__ action, const float* __restrict__ d1,
                                                           const float* __restrict__ hs, int T, float* __restrict__ dd1c,
                                                           float* __restrict__ w4term, float* __restrict__ hcc) {
    const int b = blockIdx.x, j = threadIdx.x;
    int a = (int)action[b];
    a = min(max(a, 0), T - 1);
    const size_t row = (size_t)b * T + a;
    const float d = dq[b], v = d1[row * HD + j];
    w4term[(size_t)b * HD + j] = d * v;
    dd1c[(size_t)b * HD + j] = (v > 0.f) ? d * prm[O_W4 + j] : 0.f;
    hcc[(size_t)b * 256 + j] = fmaxf(hs[row * 256 + j], 0.f);
    hcc[(size_t)b * 256 + HD + j] = fmaxf(hs[row * 256 + HD + j], 0.f);
}

}  // namespace ivosw
