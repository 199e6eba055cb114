// The forward LSTM recurrence of the Brain (Brain.forward, models/agent.py:52-58) in its four forms: one gate column per thread, the
// quad layout (batched and ragged), the 4x4x1 MFMA kernel (single and pair) and recurrence + decoder in one kernel.  brain.hip chooses
// and launches them (lstm_fwd_form_for, launch_lstm_fwd).
#pragma once
#include "brain_fused.h"

namespace ivosw {

// ---------------------------------------------------------------- forward recurrence
struct LstmFwd {
    const float* whh;  // [512,128]
    const float* gx;   // [N,T,512]  W_ih*e_t
    float* hs;         // [N,T,256]  (fw | bw) h after consuming frame t
    float* gates;      // [2,N,T,512] post-activation i,f,g,o   (nullable)
    float* cs;         // [2,N,T,128]                           (nullable)
    float* hprev;      // [2,N,T,128] h before consuming frame t (nullable)
    int N, T;
    int keep_from;     // samples >= keep_from store gates/cs/hprev
    unsigned long long* ts;   // phase probe (ivosw_lstm_probe, tools/lstm_probe.py): s_memtime stamps of step T/2 per workgroup, or nullptr
};

template <int R>
__global__ __launch_bounds__(512) void lstm_fwd_kernel(LstmFwd p) {
    __shared__ __attribute__((aligned(16))) float h_s[R][HD];
    __shared__ float c_s[R][HD];
    __shared__ float g_s[R][4 * HD];
    const int tid = threadIdx.x;
    float w[HD];
    {
        const float4* wp = reinterpret_cast<const float4*>(p.whh + (size_t)tid * HD);
#pragma unroll
        for (int i = 0; i < HD / 4; ++i) {
            const float4 v = wp[i];
            w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
        }
    }
    if (tid < HD) {
#pragma unroll
        for (int r = 0; r < R; ++r) { h_s[r][tid] = 0.f; c_s[r][tid] = 0.f; }
    }
    __syncthreads();
    // g gate: tanh(x) = 2*sigmoid(2x) - 1, so all four gate types share one branch-free exp path
    const float gk = ((tid >> 7) == 2) ? 2.0f : 1.0f;
    const int Nk = p.N - p.keep_from;  // kept buffers are indexed by (sample - keep_from)
    const int row0 = blockIdx.x * R;
    // the input-side gate term of the NEXT step is fetched while this step computes: its global-load latency sat at the
    // head of every step's fma chain (the arithmetic order is unchanged: the chain still starts from that term)
    float a_nx[R];
    auto gx_fetch = [&](int s) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int row = min(row0 + r, 2 * p.N - 1);
            const int d = row / p.N, n = row - d * p.N;
            const int t = d ? p.T - 1 - s : s;
            a_nx[r] = p.gx[((size_t)n * p.T + t) * 512 + tid];
        }
    };
    gx_fetch(0);
    for (int s = 0; s < p.T; ++s) {
        float a_cur[R];
#pragma unroll
        for (int r = 0; r < R; ++r) a_cur[r] = a_nx[r];
        if (s + 1 < p.T) gx_fetch(s + 1);
        // rows one at a time: W_hh owns the register file, per-row state lives in LDS
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int row = row0 + r;
            if (row >= 2 * p.N) break;
            const int d = row / p.N, n = row - d * p.N;
            const int t = d ? p.T - 1 - s : s;
            float a = a_cur[r];
            // h == 0 at s == 0, so the first step needs no special case (fma(0,w,a) == a)
#pragma unroll
            for (int kc = 0; kc < HD / 4; ++kc) {
                const float4 h4 = *reinterpret_cast<const float4*>(&h_s[r][kc * 4]);
                a = fmaf(h4.x, w[4 * kc], a);
                a = fmaf(h4.y, w[4 * kc + 1], a);
                a = fmaf(h4.z, w[4 * kc + 2], a);
                a = fmaf(h4.w, w[4 * kc + 3], a);
            }
            const float sg = 1.0f / (1.0f + expf(-gk * a));
            const float act = fmaf(sg, gk, 1.0f - gk);
            g_s[r][tid] = act;
            if (p.gates && n >= p.keep_from)
                p.gates[(((size_t)d * Nk + (n - p.keep_from)) * p.T + t) * 512 + tid] = act;
        }
        __syncthreads();
        {
            // state update: 128 threads per row, the R rows side by side (they used to queue behind one another on the
            // first two waves while the other six idled)
            const int r = tid >> 7, j = tid & (HD - 1);
            const int row = row0 + r;
            if (r < R && row < 2 * p.N) {
                const int d = row / p.N, n = row - d * p.N;
                const int t = d ? p.T - 1 - s : s;
                const float gi = g_s[r][j], gf = g_s[r][HD + j], gg = g_s[r][2 * HD + j], go = g_s[r][3 * HD + j];
                const bool keep = p.gates && n >= p.keep_from;
                const size_t sidx = (((size_t)d * Nk + (n - p.keep_from)) * p.T + t) * HD + j;
                if (keep) p.hprev[sidx] = h_s[r][j];
                const float c = fmaf(gf, c_s[r][j], gi * gg);
                const float h = go * tanhf_(c);
                c_s[r][j] = c;
                h_s[r][j] = h;
                p.hs[((size_t)n * p.T + t) * 256 + d * HD + j] = h;
                if (keep) p.cs[sidx] = c;
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------- forward recurrence, quad layout
// The same recurrence with the work of a step laid out so that nothing but h crosses a thread: thread = (hidden unit j,
// K-quarter q), the four threads of a unit are the four lanes of a DPP quad.  A thread keeps W_hh[g*128 + j][32q .. 32q+31]
// for all four gates g (128 registers, like the kernel above), reads ITS quarter of h (8 ds_read_b128 instead of 32: the LDS
// return path was the bound), runs four independent 32-long fma chains, and the quad sums the partials with DPP adds — no
// LDS, no barrier.  Lane q then activates gate q (one exp per lane), the quad broadcasts the four activations back, and
// every lane updates the unit's cell state, which lives in a REGISTER.  One barrier per step (h is double-buffered),
// against two barriers + a 2 KB LDS round trip of the gates before.  Summation order: four K-quarters in k order, combined
// as (q0 + q1) + (q2 + q3), then + the input-side term.
// (QuadDpp: common.h, shared with the backward recurrence)

// Where the rows of a quad workgroup live.  lstm_fwd_quad_body below is the recurrence; an addressing says how many steps the workgroup
// runs, which frame step s consumes, where that frame's input-side gates and its h are, and whether the backward pass's buffers are
// kept.  Two instances: the [N,T] batch (R rows per workgroup, training and inference) and the sequence table of the ragged
// forward (one row per workgroup, its own length).
template <int R>
struct QuadBatchRows {
    static constexpr bool KEEPS = true;
    const LstmFwd& p;
    int Nk;
    int dd[R], nn[R];
    bool ok[R], keep[R];
    __device__ __forceinline__ explicit QuadBatchRows(const LstmFwd& p_) : p(p_) {
        Nk = p.N - p.keep_from;
        const int row0 = blockIdx.x * R;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int row = row0 + r;
            ok[r] = row < 2 * p.N;
            const int rc = ok[r] ? row : 2 * p.N - 1;
            dd[r] = rc / p.N;
            nn[r] = rc - dd[r] * p.N;
            keep[r] = ok[r] && p.gates && nn[r] >= p.keep_from;
        }
    }
    __device__ __forceinline__ int steps() const { return p.T; }
    __device__ __forceinline__ int frame(int r, int s) const { return dd[r] ? p.T - 1 - s : s; }
    __device__ __forceinline__ const float* gx(int r, int t) const { return p.gx + ((size_t)nn[r] * p.T + t) * 512; }
    __device__ __forceinline__ float* hs(int r, int t) const { return p.hs + ((size_t)nn[r] * p.T + t) * 256 + dd[r] * HD; }
    __device__ __forceinline__ size_t kept(int r, int t) const { return ((size_t)dd[r] * Nk + (nn[r] - p.keep_from)) * p.T + t; }
};

struct QuadRaggedRow {                     // R = 1: workgroup 2k + d runs direction d of sequence k
    static constexpr bool KEEPS = false;   // inference only: no gates / cs / hprev
    const float* gx_;                      // [rows,512]
    float* hs_;                            // [rows,256]
    int row0, T, d;
    bool ok[1] = {true}, keep[1] = {false};
    __device__ __forceinline__ QuadRaggedRow(const float* gx, float* hs, const SeqTable& tab) : gx_(gx), hs_(hs) {
        const int k = blockIdx.x >> 1;
        d = blockIdx.x & 1;
        row0 = tab.row_off[k];
        T = tab.row_off[k + 1] - row0;
    }
    __device__ __forceinline__ int steps() const { return T; }
    __device__ __forceinline__ int frame(int, int s) const { return d ? T - 1 - s : s; }
    __device__ __forceinline__ const float* gx(int, int t) const { return gx_ + (size_t)(row0 + t) * 512; }
    __device__ __forceinline__ float* hs(int, int t) const { return hs_ + (size_t)(row0 + t) * 256 + d * HD; }
    __device__ __forceinline__ size_t kept(int, int) const { return 0; }
};

template <int R, class Rows>
__device__ __forceinline__ void lstm_fwd_quad_body(const float* whh, float* gates, float* cs, float* hprev, const Rows& rows) {
    constexpr int HQ = 36;                                   // a K-quarter of h: 32 floats + 4 of padding (the four quarters of a
    __shared__ __attribute__((aligned(16))) float h_s[2][R][4 * HQ];   // wave's reads fall on disjoint banks)
    const int tid = threadIdx.x, j = tid >> 2, q = tid & 3;
    float w[4][32];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float4* wp = reinterpret_cast<const float4*>(whh + (size_t)(g * HD + j) * HD + 32 * q);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float4 v = wp[i];
            w[g][4 * i] = v.x; w[g][4 * i + 1] = v.y; w[g][4 * i + 2] = v.z; w[g][4 * i + 3] = v.w;
        }
    }
    for (int i = tid; i < R * 4 * HQ; i += 512) (&h_s[0][0][0])[i] = 0.f;
    __syncthreads();
    const float gk = (q == 2) ? 2.0f : 1.0f;                  // tanh(x) = 2*sigmoid(2x) - 1: one branch-free exp path for all gates
    const int T = rows.steps();
    float c[R];
#pragma unroll
    for (int r = 0; r < R; ++r) c[r] = 0.f;
    float a_nx[R];
    auto gx_fetch = [&](int s) {                              // lane q fetches the input-side term of gate q
#pragma unroll
        for (int r = 0; r < R; ++r) a_nx[r] = rows.gx(r, rows.frame(r, s))[q * HD + j];
    };
    gx_fetch(0);
    for (int s = 0; s < T; ++s) {
        const int cur = s & 1;
        float a_cur[R];
#pragma unroll
        for (int r = 0; r < R; ++r) a_cur[r] = a_nx[r];
        if (s + 1 < T) gx_fetch(s + 1);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int t = rows.frame(r, s);
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
            const float* hq = &h_s[cur][r][q * HQ];
#pragma unroll
            for (int kc = 0; kc < 8; ++kc) {
                const float4 h4 = *reinterpret_cast<const float4*>(hq + 4 * kc);
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    acc[g] = fmaf(h4.x, w[g][4 * kc], acc[g]);
                    acc[g] = fmaf(h4.y, w[g][4 * kc + 1], acc[g]);
                    acc[g] = fmaf(h4.z, w[g][4 * kc + 2], acc[g]);
                    acc[g] = fmaf(h4.w, w[g][4 * kc + 3], acc[g]);
                }
            }
            // quad all-reduce of the four partial sums (lanes q ^ 1, then q ^ 2): every lane ends with the same four totals
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                acc[g] += QuadDpp::mov<0xB1>(acc[g]);         // quad_perm [1,0,3,2]
                acc[g] += QuadDpp::mov<0x4E>(acc[g]);         // quad_perm [2,3,0,1]
            }
            const float mine = q == 0 ? acc[0] : q == 1 ? acc[1] : q == 2 ? acc[2] : acc[3];
            const float pre = mine + a_cur[r];
            const float sg = fast_rcp(1.0f + fast_exp(-gk * pre));
            const float act = fmaf(sg, gk, 1.0f - gk);        // lane q: gate q (i, f, g, o) of unit j
            const float gi = QuadDpp::mov<0x00>(act), gf = QuadDpp::mov<0x55>(act), gg = QuadDpp::mov<0xAA>(act), go = QuadDpp::mov<0xFF>(act);
            const float cn = fmaf(gf, c[r], gi * gg);
            const float h = go * fast_tanh(cn);
            c[r] = cn;
            if (rows.ok[r]) {
                if (q == 0) {
                    h_s[cur ^ 1][r][(j >> 5) * HQ + (j & 31)] = h;
                    rows.hs(r, t)[j] = h;
                }
                if constexpr (Rows::KEEPS) {
                    if (rows.keep[r]) {
                        const size_t base = rows.kept(r, t);
                        gates[base * 512 + q * HD + j] = act;
                        if (q == 1) hprev[base * HD + j] = h_s[cur][r][(j >> 5) * HQ + (j & 31)];   // h before this frame
                        if (q == 2) cs[base * HD + j] = cn;
                    }
                }
            }
        }
        __syncthreads();                                      // h of step s+1 is complete; buffer `cur` is free for step s+2
    }
}

template <int R>
__global__ __launch_bounds__(512) void lstm_fwd_quad_kernel(LstmFwd p) {
    lstm_fwd_quad_body<R>(p.whh, p.gates, p.cs, p.hprev, QuadBatchRows<R>(p));
}

// The ragged forward's recurrence (ivosw_brain_forward_ragged): grid = 2 n_seqs, workgroup 2k + d = direction d of sequence k over ITS
// rows of the flat gx / hs and ITS number of steps - the arithmetic of lstm_fwd_quad_kernel<1> on that slice (the same body).
__global__ __launch_bounds__(512) void lstm_fwd_quad_ragged_kernel(const float* __restrict__ whh, const float* __restrict__ gx,
                                                                   float* __restrict__ hs, SeqTable tab) {
    lstm_fwd_quad_body<1>(whh, nullptr, nullptr, nullptr, QuadRaggedRow(gx, hs, tab));
}

// ---------------------------------------------------------------- forward recurrence on the 4x4x1 matrix instruction
// The quad kernel above is VALU-bound (SQ counters: 340 VALU instructions per wave and step for two rows, 262 of them the fma
// chains, each a 4-cycle issue; two waves per SIMD keep the VALU 76 % busy).  v_mfma_f32_4x4x1_16b_f32 computes sixteen
// independent 4x4 outer products (K = 1) in 8 cycles: with block = hidden unit, the four B lanes of a block = that unit's four
// gate columns (the DPP quad of the kernel above) and the four A rows = FOUR rows of the batch, one instruction does for four
// rows what four v_fmac do for one — 128 instructions per wave and step (K = 128) for 4 rows x 64 columns against 524 fmas,
// exact fp32 (an fma chain in k order per accumulator).  A lane keeps its column's 128 weights in registers as before; h comes
// from LDS ([4 rows][128 + 4 pad]: lane (block, i) reads row i — four addresses per wave read, on disjoint banks); four
// accumulators (k mod 4) break the 128-deep dependent chain.  The result layout IS the quad layout: lane (b, j) holds gate j of
// unit b for the four rows in four registers, so activation, quad broadcast and state update are the code above per row.
// 4 rows per workgroup: 128 workgroups for the policy pass (2B = 256 samples x 2 directions), 64 for the target: one round.
typedef float f32x4v __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void lstm_fwd_mfma_body(const LstmFwd& p, const int bid) {
    constexpr int R = 4, HP = HD + 4;
    __shared__ __attribute__((aligned(16))) float h_s[2][R][HP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (p.ts && tid == 0) p.ts[(size_t)bid * 8 + 4] = __builtin_amdgcn_s_memtime();
    const int q = lane & 3, j = wave * 16 + (lane >> 2);      // gate q of hidden unit j; as an A lane: batch row q
    // (tried: the wave's rows through coalesced 8-KB reads + a wave-local LDS transpose instead of one row per lane — 18.1 k
    // against 15.9 k cycles for these loads: what they wait for is 256 KB per workgroup out of L2 lines that all 192
    // workgroups want at the same moment, not the access pattern)
    float w[HD];
    {
        const float4* wp = reinterpret_cast<const float4*>(p.whh + (size_t)(q * HD + j) * HD);
#pragma unroll
        for (int i = 0; i < HD / 4; ++i) {
            const float4 v = wp[i];
            w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
        }
    }
    for (int i = tid; i < 2 * R * HP; i += 512) (&h_s[0][0][0])[i] = 0.f;
    __syncthreads();
    const float gk = (q == 2) ? 2.0f : 1.0f;
    const int Nk = p.N - p.keep_from;
    const int row0 = bid * R;
    int dd[R], nn[R];
    bool ok[R], keep[R];
    float c[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int row = row0 + r;
        ok[r] = row < 2 * p.N;
        const int rc = ok[r] ? row : 2 * p.N - 1;
        dd[r] = rc / p.N;
        nn[r] = rc - dd[r] * p.N;
        keep[r] = ok[r] && p.gates && nn[r] >= p.keep_from;
        c[r] = 0.f;
    }
    // After the gate activations a 4 x 4 transpose inside the quad hands lane q the four gates of batch row q, so the cell
    // update (two of the four transcendentals per element, the state register, the h / c stores) is done ONCE per (unit, row)
    // by that lane instead of by every lane of the quad for every row: 64 VALU instructions (10 transcendental) per step and
    // lane instead of 88 (16) in a phase that is VALU-throughput-bound.  This lane's row:
    const bool my_ok = q == 0 ? ok[0] : q == 1 ? ok[1] : q == 2 ? ok[2] : ok[3];
    const bool my_keep = q == 0 ? keep[0] : q == 1 ? keep[1] : q == 2 ? keep[2] : keep[3];
    const int my_d = q == 0 ? dd[0] : q == 1 ? dd[1] : q == 2 ? dd[2] : dd[3];
    const int my_n = q == 0 ? nn[0] : q == 1 ? nn[1] : q == 2 ? nn[2] : nn[3];
    const bool q_odd = (q & 1) != 0, q_hi = (q & 2) != 0;
    float cq = 0.f;                                            // cell state of (unit j, row q)
    float a_nx[R];
    auto gx_fetch = [&](int s) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int t = dd[r] ? p.T - 1 - s : s;
            a_nx[r] = p.gx[((size_t)nn[r] * p.T + t) * 512 + q * HD + j];
        }
    };
    gx_fetch(0);
    if (p.ts && tid == 0) p.ts[(size_t)bid * 8 + 5] = __builtin_amdgcn_s_memtime() + (unsigned long long)(w[0] == 1.2345e33f);
    for (int s = 0; s < p.T; ++s) {
        const int cur = s & 1;
        float a_cur[R];
#pragma unroll
        for (int r = 0; r < R; ++r) a_cur[r] = a_nx[r];
        if (s + 1 < p.T) gx_fetch(s + 1);
        const bool probe = p.ts && tid == 0 && s == p.T / 2;
        if (probe) p.ts[(size_t)bid * 8 + 0] = __builtin_amdgcn_s_memtime();
        f32x4v acc[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = f32x4v{0.f, 0.f, 0.f, 0.f};
        const float* hrow = &h_s[cur][q][0];                   // A operand: this lane supplies h[row q][k]
        // h in four batches of eight 16-byte reads, a batch ahead of the MFMAs that use it (left to itself hipcc keeps two reads
        // in flight: ~70 cycles of MFMAs against an LDS round trip of twice that)
        float4 hb[2][8];
#pragma unroll
        for (int i = 0; i < 8; ++i) hb[0][i] = *reinterpret_cast<const float4*>(hrow + 4 * i);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            if (g + 1 < 4) {
#pragma unroll
                for (int i = 0; i < 8; ++i) hb[(g + 1) & 1][i] = *reinterpret_cast<const float4*>(hrow + 4 * (8 * (g + 1) + i));
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int kc = 8 * g + i;
                const float4 h4 = hb[g & 1][i];
                acc[0] = __builtin_amdgcn_mfma_f32_4x4x1f32(h4.x, w[4 * kc], acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_4x4x1f32(h4.y, w[4 * kc + 1], acc[1], 0, 0, 0);
                acc[2] = __builtin_amdgcn_mfma_f32_4x4x1f32(h4.z, w[4 * kc + 2], acc[2], 0, 0, 0);
                acc[3] = __builtin_amdgcn_mfma_f32_4x4x1f32(h4.w, w[4 * kc + 3], acc[3], 0, 0, 0);
            }
        }
        if (probe) p.ts[(size_t)bid * 8 + 1] = __builtin_amdgcn_s_memtime() + (unsigned long long)(acc[0][0] == 1.2345e33f);   // (waits for the MFMAs)
        // (VALU-throughput-bound with two waves per SIMD — ~650 issue cycles each, 16 transcendentals at quarter rate among
        // them — not latency-bound: computing the four rows as one branch-free block ahead of the stores changed nothing)
        float m0[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float pre = ((acc[0][r] + acc[1][r]) + (acc[2][r] + acc[3][r])) + a_cur[r];
            const float sg = fast_rcp(1.0f + fast_exp(-gk * pre));
            m0[r] = fmaf(sg, gk, 1.0f - gk);                  // lane q: gate q (i, f, g, o) of unit j, batch row r
        }
        // transpose: m2[k] of lane q = gate k of row q (2 x 2 blocks across lane ^ 1, then blocks across lane ^ 2)
        float m1[R], m2[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float x = QuadDpp::mov<0xB1>(m0[r ^ 1]);     // quad_perm [1,0,3,2]
            m1[r] = (((r & 1) != 0) == q_odd) ? m0[r] : x;
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float x = QuadDpp::mov<0x4E>(m1[r ^ 2]);     // quad_perm [2,3,0,1]
            m2[r] = (((r & 2) != 0) == q_hi) ? m1[r] : x;
        }
        cq = fmaf(m2[1], cq, m2[0] * m2[2]);
        const float hq = m2[3] * fast_tanh(cq);
        const int tq = my_d ? p.T - 1 - s : s;
        if (my_ok) {
            const float hold = h_s[cur][q][j];                 // h before this frame
            h_s[cur ^ 1][q][j] = hq;
            p.hs[((size_t)my_n * p.T + tq) * 256 + my_d * HD + j] = hq;
            if (my_keep) {
                const size_t base = ((size_t)my_d * Nk + (my_n - p.keep_from)) * p.T + tq;
                p.hprev[base * HD + j] = hold;
                p.cs[base * HD + j] = cq;
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (keep[r]) {
                const int t = dd[r] ? p.T - 1 - s : s;
                const size_t base = ((size_t)dd[r] * Nk + (nn[r] - p.keep_from)) * p.T + t;
                p.gates[base * 512 + q * HD + j] = m0[r];
            }
        }
        if (probe) p.ts[(size_t)bid * 8 + 2] = __builtin_amdgcn_s_memtime();
        __syncthreads();
        if (probe) p.ts[(size_t)bid * 8 + 3] = __builtin_amdgcn_s_memtime();
    }
    if (p.ts && tid == 0) p.ts[(size_t)bid * 8 + 6] = __builtin_amdgcn_s_memtime();
}

__global__ __launch_bounds__(512) void lstm_fwd_mfma_kernel(LstmFwd p) { lstm_fwd_mfma_body(p, blockIdx.x); }

// the policy pass and the target pass of a DQN step in ONE launch (they used to run side by side on two streams, with an
// event fork / join around them): workgroups [0, first1) run job 0, the rest job 1
struct LstmFwdPair {
    LstmFwd j[2];
    int first1;
};
__global__ __launch_bounds__(512) void lstm_fwd_mfma_pair_kernel(LstmFwdPair pr) {
    const int which = (int)blockIdx.x >= pr.first1;
    lstm_fwd_mfma_body(pr.j[which], (int)blockIdx.x - (which ? pr.first1 : 0));
}

// ---------------------------------------------------------------- recurrence + decoder in one kernel ("sample-pair" layout)
// A workgroup owns BOTH directions of TWO samples (rows: (fw, n0) (bw, n0) (fw, n1) (bw, n1)) instead of four rows of one
// direction, so when the recurrence ends it holds [h_fw | h_bw] of its samples' frames — the decoder's input — in LDS and
// runs relu -> decoder_fc1 -> relu -> decoder_fc2 on them itself (the W_hh registers are free by then): the decoder launch
// and the round trip of hs through memory are gone.  Same recurrence arithmetic as lstm_fwd_mfma_kernel; the decoder is
// dec_fused_kernel's (16x16x4 MFMAs, a wave owns 16 output columns).  hs goes to memory only for the samples a consumer
// reads them from (the loss rows of the policy's `state` half).
struct FwdMega {
    const float* prm;
    const float* gx;            // [N,T,512]
    float* hs;                  // [N,T,256], written for samples >= hs_from
    float *gates, *cs, *hprev;  // kept for samples >= keep_from (nullable)
    float* d1;                  // [N*T,128], written for samples >= keep_from
    float* q;                   // [N*T]
    int N, T, keep_from, hs_from;
    int dbg;
};
struct FwdMegaPair {
    FwdMega j[2];
    int first1;
};
constexpr int MEGA_HLD = 2 * HD + 4;                                  // padded [h_fw | h_bw] row in LDS
static size_t mega_lds_bytes(int T) { return (size_t)2 * T * MEGA_HLD * sizeof(float); }      // dynamic part: the pair's hs rows

__global__ __launch_bounds__(512) void brain_fwd_mega_kernel(FwdMegaPair pr) {
    extern __shared__ __attribute__((aligned(16))) float mega_lds[];
    constexpr int R = 4, HP = HD + 4;
    const int which = (int)blockIdx.x >= pr.first1;
    const FwdMega& p = pr.j[which];
    const int bid = (int)blockIdx.x - (which ? pr.first1 : 0);
    __shared__ __attribute__((aligned(16))) float h_s[2][R][HP];
    __shared__ float q_s[8][64];
    float (*hs_l)[MEGA_HLD] = reinterpret_cast<float (*)[MEGA_HLD]>(mega_lds);     // [2T][260]: row a*T + t of sample a
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = lane & 3, j = wave * 16 + (lane >> 2);      // gate q of hidden unit j; after the transpose: row q
    const float* __restrict__ prm = p.prm;
    float w[HD];
    {
        const float4* wp = reinterpret_cast<const float4*>(prm + O_WHH + (size_t)(q * HD + j) * HD);
#pragma unroll
        for (int i = 0; i < HD / 4; ++i) {
            const float4 v = wp[i];
            w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
        }
    }
    for (int i = tid; i < 2 * R * HP; i += 512) (&h_s[0][0][0])[i] = 0.f;
    __syncthreads();
    const float gk = (q == 2) ? 2.0f : 1.0f;
    const int Nk = p.N - p.keep_from;
    int dd[R], nn[R];
    bool ok[R], keep[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int n = 2 * bid + (r >> 1);
        ok[r] = n < p.N;
        nn[r] = ok[r] ? n : p.N - 1;
        dd[r] = r & 1;
        keep[r] = ok[r] && p.gates && nn[r] >= p.keep_from;
    }
    const int my_a = q >> 1, my_d = q & 1;                    // this lane's row after the transpose: sample my_a of the pair, direction my_d
    const int my_n = 2 * bid + my_a;
    const bool my_ok = my_n < p.N;
    const bool my_keep = my_ok && p.gates && my_n >= p.keep_from;
    const bool my_hs = my_ok && my_n >= p.hs_from;
    const bool q_odd = (q & 1) != 0, q_hi = (q & 2) != 0;
    float cq = 0.f;
    float a_nx[R];
    auto gx_fetch = [&](int s) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int t = dd[r] ? p.T - 1 - s : s;
            a_nx[r] = p.gx[((size_t)nn[r] * p.T + t) * 512 + q * HD + j];
        }
    };
    gx_fetch(0);
    for (int s = 0; s < p.T; ++s) {
        const int cur = s & 1;
        float a_cur[R];
#pragma unroll
        for (int r = 0; r < R; ++r) a_cur[r] = a_nx[r];
        if (s + 1 < p.T) gx_fetch(s + 1);
        f32x4v acc[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = f32x4v{0.f, 0.f, 0.f, 0.f};
        const float* hrow = &h_s[cur][q][0];
        float4 hb[2][8];
#pragma unroll
        for (int i = 0; i < 8; ++i) hb[0][i] = *reinterpret_cast<const float4*>(hrow + 4 * i);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            if (g + 1 < 4) {
#pragma unroll
                for (int i = 0; i < 8; ++i) hb[(g + 1) & 1][i] = *reinterpret_cast<const float4*>(hrow + 4 * (8 * (g + 1) + i));
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int kc = 8 * g + i;
                const float4 h4 = hb[g & 1][i];
                acc[0] = __builtin_amdgcn_mfma_f32_4x4x1f32(h4.x, w[4 * kc], acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_4x4x1f32(h4.y, w[4 * kc + 1], acc[1], 0, 0, 0);
                acc[2] = __builtin_amdgcn_mfma_f32_4x4x1f32(h4.z, w[4 * kc + 2], acc[2], 0, 0, 0);
                acc[3] = __builtin_amdgcn_mfma_f32_4x4x1f32(h4.w, w[4 * kc + 3], acc[3], 0, 0, 0);
            }
        }
        float m0[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float pre = ((acc[0][r] + acc[1][r]) + (acc[2][r] + acc[3][r])) + a_cur[r];
            const float sg = fast_rcp(1.0f + fast_exp(-gk * pre));
            m0[r] = fmaf(sg, gk, 1.0f - gk);
        }
        float m1[R], m2[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float x = QuadDpp::mov<0xB1>(m0[r ^ 1]);
            m1[r] = (((r & 1) != 0) == q_odd) ? m0[r] : x;
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float x = QuadDpp::mov<0x4E>(m1[r ^ 2]);
            m2[r] = (((r & 2) != 0) == q_hi) ? m1[r] : x;
        }
        cq = fmaf(m2[1], cq, m2[0] * m2[2]);
        const float hq = m2[3] * fast_tanh(cq);
        const int tq = my_d ? p.T - 1 - s : s;
        if (my_ok) {
            const float hold = h_s[cur][q][j];
            h_s[cur ^ 1][q][j] = hq;
            hs_l[my_a * p.T + tq][my_d * HD + j] = hq;
            if (my_hs) p.hs[((size_t)my_n * p.T + tq) * 256 + my_d * HD + j] = hq;
            if (my_keep) {
                const size_t base = ((size_t)my_d * Nk + (my_n - p.keep_from)) * p.T + tq;
                p.hprev[base * HD + j] = hold;
                p.cs[base * HD + j] = cq;
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (keep[r]) {
                const int t = dd[r] ? p.T - 1 - s : s;
                const size_t base = ((size_t)dd[r] * Nk + (nn[r] - p.keep_from)) * p.T + t;
                p.gates[base * 512 + q * HD + j] = m0[r];
            }
        }
        __syncthreads();
    }
    // ---- decoder on the pair's 2 T rows (row m = a * T + t), 64 rows at a time; wave w owns output columns [16 w, 16 w + 16)
    if (p.dbg) return;
    const int m16 = lane & 15, kq = lane >> 4;
    const int M = (2 * bid + 1 < p.N ? 2 : 1) * p.T;
    float4 w3r[16];
    {
        const float* wb = prm + O_W3 + (size_t)(16 * wave + m16) * 256 + 4 * kq;
#pragma unroll
        for (int c = 0; c < 16; ++c) w3r[c] = *reinterpret_cast<const float4*>(wb + 16 * c);
    }
    const float b3v = prm[O_B3 + 16 * wave + m16], w4v = prm[O_W4 + 16 * wave + m16], b4v = prm[O_B4];
    for (int g0 = 0; g0 < M; g0 += 64) {
        f32x4 acc[4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
        const float* arow[4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) arow[mt] = &hs_l[min(g0 + mt * 16 + m16, M - 1)][4 * kq];
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            float4 a[4];
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                const float4 v = *reinterpret_cast<const float4*>(arow[mt] + 16 * c);
                a[mt] = make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f));
            }
            const float4 b = w3r[c];
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) acc[mt] = MFMA16(a[mt].x, b.x, acc[mt]);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) acc[mt] = MFMA16(a[mt].y, b.y, acc[mt]);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) acc[mt] = MFMA16(a[mt].z, b.z, acc[mt]);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) acc[mt] = MFMA16(a[mt].w, b.w, acc[mt]);
        }
        const int col = 16 * wave + m16;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = g0 + mt * 16 + 4 * kq + r;
                const float v = fmaxf(acc[mt][r] + b3v, 0.f);
                if (m < M) {
                    const int n = 2 * bid + m / p.T, t = m - (m / p.T) * p.T;
                    if (p.d1 && n >= p.keep_from) p.d1[((size_t)n * p.T + t) * HD + col] = v;
                }
                const float sum = row16_sum(v * w4v);
                if (m16 == 0) q_s[wave][mt * 16 + 4 * kq + r] = sum;
            }
        __syncthreads();
        if (tid < 64 && g0 + tid < M) {
            const int m = g0 + tid, a = m / p.T;
            p.q[((size_t)(2 * bid + a)) * p.T + (m - a * p.T)] =
                (((q_s[0][tid] + q_s[1][tid]) + (q_s[2][tid] + q_s[3][tid])) + ((q_s[4][tid] + q_s[5][tid]) + (q_s[6][tid] + q_s[7][tid]))) + b4v;
        }
        __syncthreads();
    }
}

}  // namespace ivosw
