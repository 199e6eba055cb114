// The backward LSTM recurrence (BPTT through the shared cell) of the DQN step: what autograd derives for Brain.forward
// (models/agent.py:52-58) under Agent.update_agent's loss.  dqn_step.hip launches it.
#pragma once
#include "brain_fwd.h"

namespace ivosw {

// ---------------------------------------------------------------- backward recurrence (BPTT)
struct LstmBwd {
    const float* whh;    // [512,128]
    const float* gates;  // [2,Nk,T,512]   (Nk kept samples, sample index relative to keep_from)
    const float* cs;     // [2,Nk,T,128]
    const float* dhc;    // [Nk,256] dL/d(h_fw|h_bw) at frame action[n] (the only frame with loss)
    const int64_t* action;  // [Nk]
    float* dG;           // [2,Nk,T,512] dL/d(gate pre-activation)
    int N, T;            // N = Nk
    unsigned long long* ts;   // phase probe (ivosw_lstm_probe): stamps of the step 3 below the row's first, per workgroup, or nullptr
};

template <int R>
__global__ __launch_bounds__(512) void lstm_bwd_kernel(LstmBwd p) {
    __shared__ __attribute__((aligned(16))) float dp_s[R][4 * HD];
    __shared__ float part_s[R][4][HD];
    const int tid = threadIdx.x, k = tid & 127, part = tid >> 7;
    float w[HD];
#pragma unroll
    for (int j = 0; j < HD; ++j) w[j] = p.whh[(size_t)(part * HD + j) * HD + k];
    int dn[R], nn[R], s0[R];
    bool ok[R];
    int smax = -1;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int row = blockIdx.x * R + r;
        ok[r] = row < 2 * p.N;
        dn[r] = ok[r] ? row / p.N : 0;
        nn[r] = ok[r] ? row % p.N : 0;
        int a = ok[r] ? (int)p.action[nn[r]] : 0;
        a = min(max(a, 0), p.T - 1);
        s0[r] = ok[r] ? (dn[r] ? p.T - 1 - a : a) : -1;  // step at which frame `action` is consumed
        smax = max(smax, s0[r]);
    }
    // steps after the loss frame carry no gradient
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (!ok[r]) continue;
        for (int s = s0[r] + 1; s < p.T; ++s) {
            const int t = dn[r] ? p.T - 1 - s : s;
            p.dG[(((size_t)dn[r] * p.N + nn[r]) * p.T + t) * 512 + tid] = 0.f;
        }
    }
    float dh_rec[R], dc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) { dh_rec[r] = 0.f; dc[r] = 0.f; }

    for (int s = smax; s >= 0; --s) {
        if (tid < HD) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                float di = 0.f, df = 0.f, dg = 0.f, dO = 0.f;
                if (ok[r] && s <= s0[r]) {
                    const int t = dn[r] ? p.T - 1 - s : s;
                    const size_t rt = ((size_t)dn[r] * p.N + nn[r]) * p.T + t;
                    const float* gp = p.gates + rt * 512;
                    const float gi = gp[tid], gf = gp[HD + tid], gg = gp[2 * HD + tid], go = gp[3 * HD + tid];
                    const float cc = p.cs[rt * HD + tid];
                    const int tprev = dn[r] ? t + 1 : t - 1;
                    const float cprev = (s > 0) ? p.cs[(((size_t)dn[r] * p.N + nn[r]) * p.T + tprev) * HD + tid] : 0.f;
                    float dh = dh_rec[r];
                    if (s == s0[r]) dh += p.dhc[(size_t)nn[r] * 256 + dn[r] * HD + tid];
                    const float tc = tanhf_(cc);
                    dc[r] = fmaf(dh * go, 1.f - tc * tc, dc[r]);
                    di = dc[r] * gg * gi * (1.f - gi);
                    df = dc[r] * cprev * gf * (1.f - gf);
                    dg = dc[r] * gi * (1.f - gg * gg);
                    dO = dh * tc * go * (1.f - go);
                    dc[r] *= gf;
                    float* o = p.dG + rt * 512;
                    o[tid] = di; o[HD + tid] = df; o[2 * HD + tid] = dg; o[3 * HD + tid] = dO;
                }
                dp_s[r][tid] = di; dp_s[r][HD + tid] = df; dp_s[r][2 * HD + tid] = dg; dp_s[r][3 * HD + tid] = dO;
            }
        }
        __syncthreads();
        if (s > 0) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                float a = 0.f;
#pragma unroll
                for (int jc = 0; jc < HD / 4; ++jc) {
                    const float4 d4 = *reinterpret_cast<const float4*>(&dp_s[r][part * HD + jc * 4]);
                    a = fmaf(d4.x, w[4 * jc], a);
                    a = fmaf(d4.y, w[4 * jc + 1], a);
                    a = fmaf(d4.z, w[4 * jc + 2], a);
                    a = fmaf(d4.w, w[4 * jc + 3], a);
                    if ((jc & 7) == 7) __builtin_amdgcn_sched_barrier(0);
                }
                part_s[r][part][k] = a;
            }
        }
        __syncthreads();
        if (s > 0 && tid < HD) {
#pragma unroll
            for (int r = 0; r < R; ++r)
                dh_rec[r] = (part_s[r][0][tid] + part_s[r][1][tid]) + (part_s[r][2][tid] + part_s[r][3][tid]);
        }
    }
}

// ---------------------------------------------------------------- backward recurrence, quad layout
// Thread = (hidden unit k, gate q); the four threads of a unit are a DPP quad.  Lane q computes dL/d(pre-activation) of
// gate q of unit k (the kernel above leaves that to 128 of its 512 threads, each behind a chain of global loads), keeps
// W_hh[q*128 + j][k] (j = 0..127) in registers, and the quad sums the four gates' contributions to dL/dh_prev[k] with DPP
// adds: one barrier per step (the gate gradients are double-buffered in LDS), no partial-sum round trip.  The
// activations of step s-1 are requested before the matvec of step s.  Same arithmetic per element as lstm_bwd_kernel;
// the 512-long dot product is summed as four interleaved 32-long chains per gate, gates combined (i + f) + (g + o).
template <int R>
__global__ __launch_bounds__(512) void lstm_bwd_quad_kernel(LstmBwd p) {
    constexpr int GQ = HD + 4;                               // one gate's 128 gradients + 4 floats of padding (bank spread)
    __shared__ __attribute__((aligned(16))) float dp_s[2][R][4 * GQ];
    const int tid = threadIdx.x, k = tid >> 2, q = tid & 3;
    float w[HD];
#pragma unroll
    for (int j = 0; j < HD; ++j) w[j] = p.whh[(size_t)(q * HD + j) * HD + k];
    int dn[R], nn[R], s0[R];
    bool ok[R];
    int smax = -1;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int row = blockIdx.x * R + r;
        ok[r] = row < 2 * p.N;
        dn[r] = ok[r] ? row / p.N : 0;
        nn[r] = ok[r] ? row % p.N : 0;
        int a = ok[r] ? (int)p.action[nn[r]] : 0;
        a = min(max(a, 0), p.T - 1);
        s0[r] = ok[r] ? (dn[r] ? p.T - 1 - a : a) : -1;      // step at which frame `action` is consumed
        smax = max(smax, s0[r]);
    }
    // steps after the loss frame carry no gradient
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (!ok[r]) continue;
        for (int s = s0[r] + 1; s < p.T; ++s) {
            const int t = dn[r] ? p.T - 1 - s : s;
            p.dG[(((size_t)dn[r] * p.N + nn[r]) * p.T + t) * 512 + q * HD + k] = 0.f;
        }
    }
    auto rt_of = [&](int r, int s) {                          // (direction, sample, frame) row of the kept activations at step s
        const int sc = min(max(s, 0), p.T - 1);
        const int t = dn[r] ? p.T - 1 - sc : sc;
        return ((size_t)dn[r] * p.N + nn[r]) * p.T + t;
    };
    // The kept activations of a step (its gate, its cell state, the cell state before it) are requested TWO steps ahead into
    // a ring of three register sets with fixed roles — the loop is unrolled by three, so nothing is copied: a rotating copy
    // (g_cur = g_nx) reads the load's destination, i.e. waits for a load that was issued at the top of the same step.
    struct Kept { float g, c, cp; };
    Kept ring[3][R];
    auto fetch = [&](int s, Kept (&dst)[R]) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            dst[r].g = p.gates[rt_of(r, s) * 512 + q * HD + k];
            dst[r].c = p.cs[rt_of(r, s) * HD + k];
            dst[r].cp = p.cs[rt_of(r, s - 1) * HD + k];
        }
    };
    float dh_rec[R], dc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) { dh_rec[r] = 0.f; dc[r] = 0.f; }
    fetch(smax, ring[0]);
    fetch(smax - 1, ring[1]);
    if (p.ts && tid == 0) p.ts[(size_t)blockIdx.x * 8 + 4] = __builtin_amdgcn_s_memtime() + (unsigned long long)(w[0] == 1.2345e33f);
    auto step = [&](int s, Kept (&cur)[R], Kept (&ahead)[R]) {
        const int buf = s & 1;
        const bool probe = p.ts && tid == 0 && s == smax - 3;
        if (probe) p.ts[(size_t)blockIdx.x * 8 + 0] = __builtin_amdgcn_s_memtime();
        fetch(s - 2, ahead);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const bool act = ok[r] && s <= s0[r];
            const float gq = cur[r].g;
            const float gi = QuadDpp::mov<0x00>(gq), gf = QuadDpp::mov<0x55>(gq), gg = QuadDpp::mov<0xAA>(gq), go = QuadDpp::mov<0xFF>(gq);
            const float cc = cur[r].c;
            const float cprev = (s > 0) ? cur[r].cp : 0.f;
            float dh = dh_rec[r];
            if (s == s0[r]) dh += p.dhc[(size_t)nn[r] * 256 + dn[r] * HD + k];
            const float tc = fast_tanh(cc);
            const float dcn = fmaf(dh * go, 1.f - tc * tc, dc[r]);
            const float di = dcn * gg * gi * (1.f - gi);
            const float df = dcn * cprev * gf * (1.f - gf);
            const float dg = dcn * gi * (1.f - gg * gg);
            const float dO = dh * tc * go * (1.f - go);
            float mine = q == 0 ? di : q == 1 ? df : q == 2 ? dg : dO;
            mine = act ? mine : 0.f;
            if (act) {
                dc[r] = dcn * gf;
                p.dG[rt_of(r, s) * 512 + q * HD + k] = mine;
            }
            dp_s[buf][r][q * GQ + k] = mine;
        }
        if (probe) p.ts[(size_t)blockIdx.x * 8 + 1] = __builtin_amdgcn_s_memtime();
        __syncthreads();                                       // gate gradients of step s complete; buffer buf^1 (step s+1) is free
        if (probe) p.ts[(size_t)blockIdx.x * 8 + 2] = __builtin_amdgcn_s_memtime();
        if (s > 0) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
                const float* dq = &dp_s[buf][r][q * GQ];
#pragma unroll
                for (int jc = 0; jc < HD / 4; ++jc) {
                    const float4 d4 = *reinterpret_cast<const float4*>(dq + 4 * jc);
                    a0 = fmaf(d4.x, w[4 * jc], a0);
                    a1 = fmaf(d4.y, w[4 * jc + 1], a1);
                    a2 = fmaf(d4.z, w[4 * jc + 2], a2);
                    a3 = fmaf(d4.w, w[4 * jc + 3], a3);
                    if ((jc & 7) == 7) __builtin_amdgcn_sched_barrier(0);   // keeps hipcc from hoisting all 32 reads (128 registers) at once
                }
                float a = (a0 + a1) + (a2 + a3);
                a += QuadDpp::mov<0xB1>(a);
                a += QuadDpp::mov<0x4E>(a);
                dh_rec[r] = a;
            }
        }
        if (probe) p.ts[(size_t)blockIdx.x * 8 + 3] = __builtin_amdgcn_s_memtime() + (unsigned long long)(dh_rec[0] == 1.2345e33f);
    };
    for (int s = smax; s >= 0; s -= 3) {
        step(s, ring[0], ring[2]);
        if (s - 1 >= 0) step(s - 1, ring[1], ring[0]);
        if (s - 2 >= 0) step(s - 2, ring[2], ring[1]);
    }
    if (p.ts && tid == 0) { p.ts[(size_t)blockIdx.x * 8 + 5] = __builtin_amdgcn_s_memtime(); p.ts[(size_t)blockIdx.x * 8 + 6] = (unsigned long long)(smax + 1); }
}

}  // namespace ivosw
