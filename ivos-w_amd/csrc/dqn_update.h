// The one body of the DQN update kernels, and the pieces it is made of: the last-workgroup ticket, the 16-byte arena traversal, the
// gradient sources, the lr sources, the two optimizer rules and the target rule.  dqn.hip (the stand-alone update entries) and dqn_step.hip
// (the one-call step's tails) instantiate it; every kernel there is a thin __global__ wrapper that names its four choices:
//   rule     AdamRule | SgdRule                    (clamp_adam_elem / clamp_sgd_elem and the state each keeps)
//   gradient ArenaGrad | SlabGrad                  (the gradient arena as it stands, or reduce_on_load)
//   lr       Lr<false> | Lr<true>                  (an argument, or lr_table[min(k, lr_steps)] of the rule's counter k)
//   target   NoTarget | the rule's arguments       (nothing, or the target-network rule on the element just produced)
// All four are compile-time choices: a wrapper holds exactly the code of the combination it names.
#pragma once
#include <initializer_list>
#include <type_traits>

#include "adam.h"
#include "sgd.h"
#include "target.h"

namespace ivosw {

// The ticket: the LAST workgroup of a launch to get here — after its own reads and writes, hence the barrier — runs publish() and
// leaves the ticket at 0 for the next launch.  No other workgroup can still be reading what publish() writes (each read it before it
// took its own ticket), and nothing but the ticket crosses workgroups, so no fence is needed.  Few, large workgroups: the tickets of
// one launch serialise on one address (708 of them took longer than the update).
template <class Publish>
__device__ __forceinline__ void last_workgroup(unsigned* ticket, Publish publish) {
    __syncthreads();
    if (threadIdx.x == 0 && atomicAdd(ticket, 1u) == gridDim.x - 1) {
        publish();
        atomicExch(ticket, 0u);
    }
}

// W consecutive floats of one array at element i: one 16-byte (W = 4, i a multiple of 4, the array 16-byte aligned) or one 4-byte load or store
template <int W>
struct fvec {
    float x[W];
    __device__ __forceinline__ float& operator[](int j) { return x[j]; }
    __device__ __forceinline__ float operator[](int j) const { return x[j]; }
};
template <int W> using Width = std::integral_constant<int, W>;
template <int W> __device__ __forceinline__ fvec<W> load_group(const float* a, int i);
template <> __device__ __forceinline__ fvec<1> load_group<1>(const float* a, int i) { return {{a[i]}}; }
template <> __device__ __forceinline__ fvec<4> load_group<4>(const float* a, int i) {
    const float4 q = *reinterpret_cast<const float4*>(a + i);
    return {{q.x, q.y, q.z, q.w}};
}
__device__ __forceinline__ void store_group(float* a, int i, const fvec<1>& x) { a[i] = x[0]; }
__device__ __forceinline__ void store_group(float* a, int i, const fvec<4>& x) {
    *reinterpret_cast<float4*>(a + i) = make_float4(x[0], x[1], x[2], x[3]);
}

// The traversal of an n-element arena, one group per lane: f(i, Width<W>) with W the number of elements at i.  VEC (every array
// 16-byte aligned): lane t < n / 4 gets elements [4t, 4t + 4), the n % 4 tail elements go one each to the first lanes past the vector
// part, so the grid is ceil((n / 4 + 3) / lanes) workgroups.  Otherwise one element per lane.
template <bool VEC, class F>
__device__ __forceinline__ void for_each_group(int n, F f) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if constexpr (VEC) {
        const int n4 = n >> 2;
        if (t < n4) f(4 * t, Width<4>{});
        else if (t - n4 < (n & 3)) f(4 * n4 + (t - n4), Width<1>{});
    } else {
        if (t < n) f(t, Width<1>{});
    }
}

// ---------------------------------------------------------------- the gradient source
struct ArenaGrad {
    const float* g;
    template <int W>
    __device__ __forceinline__ fvec<W> load(int i) const { return load_group<W>(g, i); }
};

// The gradient of arena element i with the step's split-K slab reduction folded in: an element of a slabbed tensor is summed from its
// slabs ON LOAD in splitk_reduce_group_kernel's order (four interleaved partial sums over z, eight loads in flight, (s0 + s1) + (s2 + s3))
// and written to g[i] on the way, so the arena holds what the separate reduction would have left there; any other element is read
// from the arena.  off[k] = element offset of slab set k in the arena.
__device__ __forceinline__ float reduce_on_load(float* __restrict__ g, const ReduceGroup& rg, const int (&off)[REDUCE_MAX], int i) {
    int w = -1;
#pragma unroll
    for (int k = 0; k < REDUCE_MAX; ++k)
        if (rg.nslab[k] > 0 && i >= off[k] && i < off[k] + rg.n[k]) w = k;
    if (w < 0) return g[i];
    const float* sl = rg.slabs[w] + (i - off[w]);
    const size_t nn = rg.n[w];
    const int ns = rg.nslab[w];
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int z = 0;
    for (; z + 8 <= ns; z += 8) {
        float q[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) q[u] = sl[(size_t)(z + u) * nn];
        s0 += q[0]; s1 += q[1]; s2 += q[2]; s3 += q[3];
        s0 += q[4]; s1 += q[5]; s2 += q[6]; s3 += q[7];
    }
    for (; z < ns; ++z) s0 += sl[(size_t)z * nn];
    const float gi = (s0 + s1) + (s2 + s3);
    g[i] = gi;
    return gi;
}

struct SlabGrad {               // one element per lane only
    float* g;
    const ReduceGroup& rg;
    const int (&off)[REDUCE_MAX];
    template <int W>
    __device__ __forceinline__ fvec<1> load(int i) const { return {{reduce_on_load(g, rg, off, i)}}; }
};

// ---------------------------------------------------------------- the lr source (k = the rule's counter before the update)
template <bool SCHED_>           // false: the argument `lr`; true: lr_table[min(k, lr_steps)], one scalar load per wave in its place
struct Lr {
    static constexpr bool SCHED = SCHED_;
    float lr;
    const float* lr_table;
    int lr_steps;
    __device__ __forceinline__ float at(int k) const { return SCHED ? sched_lr(lr_table, lr_steps, k) : lr; }
};
using ConstLr = Lr<false>;      // Lr<false>{lr}

// ---------------------------------------------------------------- the rules
// Clamp + Adam with the step counter advanced by the same launch: every thread reads the counter k left by the previous launch and
// evaluates step k + 1's bias corrections itself (the float64 expressions of ivosw_clamp_adam: identical bits); publish() leaves k + 1.
struct AdamRule {
    static constexpr bool COUNTS = true;            // with any lr source
    float *m, *v;
    AdamDevState* st;
    float beta1, beta2, eps, wd, clampv, gscale;
    struct Step { int step; double b1t, b2t; float step_size, bc2_sqrt; };
    __device__ __forceinline__ Step begin(int k, float lr) const {
        const int step = k + 1;
        const double b1t = ipow((double)beta1, step), b2t = ipow((double)beta2, step);
        return {step, b1t, b2t, (float)((double)lr / (1.0 - b1t)), (float)sqrt(1.0 - b2t)};
    }
    template <int W>
    __device__ __forceinline__ fvec<W> apply(const Step& s, fvec<W> g, fvec<W> p, int i) const {
        fvec<W> m_ = load_group<W>(m, i), v_ = load_group<W>(v, i);
#pragma unroll
        for (int j = 0; j < W; ++j) p[j] = clamp_adam_elem(g[j], p[j], m_[j], v_[j], s.step_size, s.bc2_sqrt, beta1, beta2, eps, wd, clampv, gscale);
        store_group(m, i, m_); store_group(v, i, v_);
        return p;
    }
    __device__ __forceinline__ void publish(const Step& s) const {
        st->b1t = s.b1t; st->b2t = s.b2t; st->step = s.step; st->step_size = s.step_size; st->bc2_sqrt = s.bc2_sqrt;
    }
};

// Clamp + SGD.  Nothing but the momentum buffer carries over from one step to the next, so under a constant lr there is no counter
// (st is not looked at) and, without a target, no ticket either: the launch simply repeats under a captured graph.
struct SgdRule {
    static constexpr bool COUNTS = false;           // on the schedule only
    float* buf;
    SgdDevState* st;
    float mu, wd;
    int nesterov;
    float clampv, gscale;
    struct Step { int k; float lr; };
    __device__ __forceinline__ Step begin(int k, float lr) const { return {k, lr}; }
    template <int W>
    __device__ __forceinline__ fvec<W> apply(const Step& s, fvec<W> g, fvec<W> p, int i) const {
        fvec<W> b_ = load_group<W>(buf, i);
#pragma unroll
        for (int j = 0; j < W; ++j) p[j] = clamp_sgd_elem(g[j], p[j], b_[j], s.lr, mu, wd, nesterov, clampv, gscale);
        store_group(buf, i, b_);
        return p;
    }
    __device__ __forceinline__ void publish(const Step& s) const { st->step = s.k + 1; }
};

// ---------------------------------------------------------------- the target
// NoTarget, or the rule's arguments: {float* t; TargetDevState* st; int mode; float tau; int period;} (dqn_step.hip's TargetArgs)
struct NoTarget {};

// The rule on the W elements at i, in the thread that holds p_new.  A periodic step reads nothing of t, and touches nothing unless it fires.
template <int W>
__device__ __forceinline__ void target_group(float* __restrict__ t, int i, fvec<W> p_new, int mode, float tau, bool fires) {
    if (mode == TARGET_SOFT) {
        fvec<W> t_ = load_group<W>(t, i);
#pragma unroll
        for (int j = 0; j < W; ++j) t_[j] = fmaf(tau, p_new[j] - t_[j], t_[j]);
        store_group(t, i, t_);
    } else if (fires) {
        store_group(t, i, p_new);
    }
}

// ---------------------------------------------------------------- the body
// Every workgroup reads the counters it needs (the rule's: Adam always, SGD on the schedule; the target's) before anything else, updates
// its groups, and takes ONE ticket, under which the last workgroup advances every counter read: the rule's state's where the rule
// counts, else the target's; a launch that reads no counter takes none.
template <bool VEC, class Rule, class Grad, class LrSrc, class Target>
__device__ __forceinline__ void clamp_update(float* __restrict__ p, int n, const Rule& rule, const Grad& grad, const LrSrc& lr, const Target& tgt) {
    constexpr bool COUNTS = Rule::COUNTS || LrSrc::SCHED, TARGET = !std::is_same<Target, NoTarget>::value;
    int k = 0, kt = 0;
    bool fires = false;
    if constexpr (COUNTS) k = rule.st->step;
    const auto step = rule.begin(k, lr.at(k));
    if constexpr (TARGET) {
        kt = tgt.st->step;
        fires = target_fires(kt, tgt.period);
    }
    for_each_group<VEC>(n, [&](int i, auto w) {
        constexpr int W = decltype(w)::value;
        const fvec<W> g = grad.template load<W>(i);
        const fvec<W> p_new = rule.template apply<W>(step, g, load_group<W>(p, i), i);
        store_group(p, i, p_new);
        if constexpr (TARGET) target_group<W>(tgt.t, i, p_new, tgt.mode, tgt.tau, fires);
    });
    if constexpr (COUNTS || TARGET) {
        unsigned* ticket;
        if constexpr (COUNTS) ticket = &rule.st->ticket;
        else ticket = &tgt.st->ticket;
        last_workgroup(ticket, [&] {
            if constexpr (COUNTS) rule.publish(step);
            if constexpr (TARGET) tgt.st->step = kt + 1;
        });
    }
}

// ---------------------------------------------------------------- host side
// Launches a traversal kernel over n elements in workgroups of `lanes`: its <true> instantiation when every array is 16-byte aligned,
// else its <false> one, each with for_each_group's grid.
template <class... Params, class... Args>
inline void launch_traversal(void (*vec)(Params...), void (*scalar)(Params...), std::initializer_list<const void*> arrays, int n, int lanes,
                             hipStream_t stream, Args... args) {
    if (aligned16(arrays)) hipLaunchKernelGGL(vec, dim3((n / 4 + 3 + lanes - 1) / lanes), dim3(lanes), 0, stream, args...);
    else hipLaunchKernelGGL(scalar, dim3((n + lanes - 1) / lanes), dim3(lanes), 0, stream, args...);
}

}  // namespace ivosw
