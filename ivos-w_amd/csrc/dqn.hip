// Fused clamp + Adam over the flat parameter arena (K9; clamp + SGD with momentum beside it), hard target sync (K10), replay gather (K11).
// Reference: models/agent.py:157-165 (clamp, optim.Adam(lr, weight_decay) step, target sync),
// datasets/agent_dataset.py:71-115 + train_agent.py:177-182 (minibatch assembly).
#include "dqn_update.h"

namespace ivosw {

// torch.optim.Adam (non-amsgrad, coupled L2): g += wd*p; m.lerp_(g, 1-b1); v = b2*v + (1-b2)*g*g;
// p -= (lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps).  The clamp comes first (agent.py:157-159);
// grad_scale (=1/world) is applied before the clamp so the clamp sees the averaged gradient.
__global__ void clamp_adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                  float* __restrict__ v, int n, float step_size, float bc2_sqrt, float beta1, float beta2,
                                  float eps, float wd, float clampv, float gscale) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float mi = m[i], vi = v[i];
    p[i] = clamp_adam_elem(g[i], p[i], mi, vi, step_size, bc2_sqrt, beta1, beta2, eps, wd, clampv, gscale);
    m[i] = mi;
    v[i] = vi;
}

// Row `src` of the replay into slot b of the minibatch: the (iou, annotated) pairs of its T steps, by the whole workgroup.
__device__ __forceinline__ void replay_copy_row(const float* __restrict__ old_iou, const float* __restrict__ new_iou,
                                                const float* __restrict__ ann, const float* __restrict__ nann, int64_t src, int b, int T,
                                                float* __restrict__ state, float* __restrict__ new_state) {
    for (int t = threadIdx.x; t < T; t += blockDim.x) {
        const size_t s = (size_t)src * T + t, d = ((size_t)b * T + t) * 2;
        state[d] = old_iou[s];
        state[d + 1] = ann[s];
        new_state[d] = new_iou[s];
        new_state[d + 1] = nann[s];
    }
}

__global__ void replay_gather_kernel(const float* __restrict__ old_iou, const float* __restrict__ new_iou,
                                     const float* __restrict__ ann, const float* __restrict__ nann,
                                     const int64_t* __restrict__ action, const float* __restrict__ rstep,
                                     const float* __restrict__ rdone, const int64_t* __restrict__ idx, int B, int T,
                                     float* __restrict__ state, float* __restrict__ new_state,
                                     int64_t* __restrict__ action_out, float* __restrict__ rstep_out,
                                     float* __restrict__ rdone_out) {
    const int b = blockIdx.x;
    const int64_t src = idx[b];
    replay_copy_row(old_iou, new_iou, ann, nann, src, b, T, state, new_state);
    if (threadIdx.x == 0) {
        action_out[b] = action[src];
        rstep_out[b] = rstep[src];
        rdone_out[b] = rdone[src];
    }
}

// The minibatch draw on the device (uniform with replacement, what torch.randint gave the eager loop): the index of slot b
// of draw number c is a splitmix64 finaliser of (seed, c, b) scaled to [0, n) by a 64 x 64 -> high-64 multiply — integer
// arithmetic only, so tests/ and a host mirror (ivos_w_amd.models.momory_pool.draw_indices) reproduce it bit for bit.  The
// draw counter lives on the device and is advanced by the LAST workgroup of the launch (last_workgroup, dqn_update.h), so a
// captured HIP graph replays a fresh minibatch each time with no host-side RNG launch in front of it (that launch and the
// bubble it left before the graph cost ~9.5 us of a 204 us step).
__global__ void replay_draw_gather_kernel(const float* __restrict__ old_iou, const float* __restrict__ new_iou,
                                          const float* __restrict__ ann, const float* __restrict__ nann,
                                          const int64_t* __restrict__ action, const float* __restrict__ rstep,
                                          const float* __restrict__ rdone, DrawState* __restrict__ ds, int n, int B, int T,
                                          int64_t* __restrict__ idx_out, float* __restrict__ state, float* __restrict__ new_state,
                                          int64_t* __restrict__ action_out, float* __restrict__ rstep_out,
                                          float* __restrict__ rdone_out) {
    const int b = blockIdx.x;
    const unsigned counter = ds->counter;
    const int64_t src = (int64_t)__umul64hi(draw_mix(ds->seed, counter, (unsigned)b), (unsigned long long)n);
    replay_copy_row(old_iou, new_iou, ann, nann, src, b, T, state, new_state);
    if (threadIdx.x == 0) {
        idx_out[b] = src;
        action_out[b] = action[src];
        rstep_out[b] = rstep[src];
        rdone_out[b] = rdone[src];
    }
    last_workgroup(&ds->ticket, [&] { ds->counter = counter + 1; });
}

// mask_quality[:] = pred.mean(1); state = stack([mask_quality, counts], 1) (utils/utils_agent.py:120-121) without leaving the
// device.  pred is a float64 [n_frames, n_obj] array filled with the float32 scores, so the mean is a float64 sum in numpy's
// order (add.reduce along the contiguous axis: sequential below 8 elements, else 8 interleaved partial sums combined
// pairwise plus a sequential tail) divided by n_obj; the Brain then sees float32(mean) (torch.Tensor(state), agent.py:176).
// One frame of it: `col` points at the frame's score of object 0, the objects are `stride` floats apart.
__device__ __forceinline__ void quality_state_row(const float* __restrict__ col, int n_obj, size_t stride, float count,
                                                  double* __restrict__ quality, float* __restrict__ state) {
    auto at = [&](int o) { return (double)col[(size_t)o * stride]; };
    double sum;
    if (n_obj < 8) {
        sum = at(0);        // numpy's reduce starts from the first element (no 0.0 + x)
        for (int o = 1; o < n_obj; ++o) sum += at(o);
    } else {
        double r[8];
        for (int j = 0; j < 8; ++j) r[j] = at(j);
        int i = 8;
        for (; i + 8 <= n_obj; i += 8)
            for (int j = 0; j < 8; ++j) r[j] += at(i + j);
        sum = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n_obj; ++i) sum += at(i);
    }
    const double q = sum / (double)n_obj;
    *quality = q;
    state[0] = (float)q;
    state[1] = count;
}

__global__ void quality_state_kernel(const float* __restrict__ scores, int n_obj, int n_frames, const float* __restrict__ counts,
                                     double* __restrict__ quality, float* __restrict__ state) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n_frames) return;
    quality_state_row(scores + f, n_obj, (size_t)n_frames, counts[f], quality + f, state + 2 * (size_t)f);
}

// The same for several videos in one launch (ivosw_quality_state_ragged): one thread per flat row; the row's video is found in the
// table (row_off is ascending: the last k with row_off[k] <= row), whose scores are the [n_obj[k], T_k] block at unit_off[k].
struct QualityTable {
    SeqTable seq;
    int n_obj[IVOSW_MAX_SEQS];
    long long unit_off[IVOSW_MAX_SEQS];
};
__global__ void quality_state_ragged_kernel(const float* __restrict__ scores, QualityTable tab, int n_seqs, int rows,
                                            const float* __restrict__ counts, double* __restrict__ quality, float* __restrict__ state) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= rows) return;
    int lo = 0, hi = n_seqs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab.seq.row_off[mid] <= f) lo = mid;
        else hi = mid - 1;
    }
    const int r0 = tab.seq.row_off[lo], T = tab.seq.row_off[lo + 1] - r0;
    quality_state_row(scores + tab.unit_off[lo] + (f - r0), tab.n_obj[lo], (size_t)T, counts[f], quality + f, state + 2 * (size_t)f);
}

// The update kernels: thin wrappers of clamp_update (dqn_update.h), which documents the body, the ticket and the traversal.  VEC: 16 bytes
// per lane and array.  clamp_adam_dev_kernel: clamp + Adam with the step counter advanced by the SAME launch (a one-thread tick kernel
// in front of it cost a link of the step's launch chain, ~5 us).
template <bool VEC>
__global__ __launch_bounds__(1024) void clamp_adam_dev_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                              float* __restrict__ v, int n, AdamDevState* __restrict__ st, float lr, float beta1,
                                                              float beta2, float eps, float wd, float clampv, float gscale) {
    clamp_update<VEC>(p, n, AdamRule{m, v, st, beta1, beta2, eps, wd, clampv, gscale}, ArenaGrad{g}, Lr<false>{lr}, NoTarget{});
}

// The scheduled form (cfg.agent.lr_schedule = "poly"): lr = lr_table[min(k, lr_steps)] with k the counter left by the previous launch.
template <bool VEC>
__global__ __launch_bounds__(1024) void clamp_adam_dev_sched_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                                    float* __restrict__ v, int n, AdamDevState* __restrict__ st,
                                                                    const float* __restrict__ lr_table, int lr_steps, float beta1, float beta2,
                                                                    float eps, float wd, float clampv, float gscale) {
    clamp_update<VEC>(p, n, AdamRule{m, v, st, beta1, beta2, eps, wd, clampv, gscale}, ArenaGrad{g}, Lr<true>{0.f, lr_table, lr_steps}, NoTarget{});
}

// Clamp + SGD: capture-safe as it stands, no step counter, no ticket (256-lane workgroups: there is nothing to serialise).
template <bool VEC>
__global__ __launch_bounds__(256) void clamp_sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, int n,
                                                        float lr, float mu, float wd, int nesterov, float clampv, float gscale) {
    clamp_update<VEC>(p, n, SgdRule{buf, nullptr, mu, wd, nesterov, clampv, gscale}, ArenaGrad{g}, Lr<false>{lr}, NoTarget{});
}

// The scheduled form: the SGD state's counter picks lr and is advanced under its ticket.  1024-lane workgroups, as clamp_adam_dev_kernel
// (45 tickets at n = 180 993).
template <bool VEC>
__global__ __launch_bounds__(1024) void clamp_sgd_sched_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                                               int n, SgdDevState* __restrict__ st, const float* __restrict__ lr_table,
                                                               int lr_steps, float mu, float wd, int nesterov, float clampv, float gscale) {
    clamp_update<VEC>(p, n, SgdRule{buf, st, mu, wd, nesterov, clampv, gscale}, ArenaGrad{g}, Lr<true>{0.f, lr_table, lr_steps}, NoTarget{});
}

// The target-network rule as a launch of its own (target_group: soft = t += tau * (p - t) in one fma, periodic = copy every period-th
// step), for every chain that does not end in the one-call step's fused tail.  Every workgroup reads the counter, the last one to
// finish publishes counter + 1 (1024-lane workgroups for the ticket's sake).  A periodic step that does not fire loads nothing.
template <bool VEC>
__global__ __launch_bounds__(1024) void target_update_kernel(float* __restrict__ t, const float* __restrict__ p, int n, int mode, float tau,
                                                             int period, TargetDevState* __restrict__ st) {
    const int k = st->step;
    const bool fires = target_fires(k, period);
    if (mode == TARGET_SOFT || fires)
        for_each_group<VEC>(n, [&](int i, auto w) {
            constexpr int W = decltype(w)::value;
            target_group<W>(t, i, load_group<W>(p, i), mode, tau, fires);
        });
    last_workgroup(&st->ticket, [&] { st->step = k + 1; });
}

// ---------------------------------------------------------------- prioritized replay (cfg.agent.replay = "prioritized")
// The sum tree of a replay of n rows: P = the next power of two >= max(n, 2), a float32 array [2P].  Node 1 is the root, the children
// of node i are 2i and 2i + 1, the leaf of row r is node P + r (0 for r >= n), slot 0 is unused, and every internal node is
// float32(left + right), always recomputed from its two children: the tree is a pure function of its leaves.
inline int per_leaves(int n) {
    int P = 2;
    while (P < n) P <<= 1;
    return P;
}

__global__ void per_leaves_kernel(float* __restrict__ tree, int P, int n, const float* __restrict__ old_leaves, int n_old,
                                  const PerState* __restrict__ st, float alpha) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= P) return;
    float v = 0.f;
    if (r < n_old) v = old_leaves[r];
    else if (r < n) v = powf(st->max_priority, alpha);      // a row the tree has not seen
    tree[P + r] = v;
    if (r == 0) tree[0] = 0.f;
}

__global__ void per_level_kernel(float* __restrict__ tree, int lo) {          // nodes [lo, 2 lo) from their children
    const int i = lo + blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 2 * lo) tree[i] = tree[2 * i] + tree[2 * i + 1];
}

// beta of draw c: beta0 + (1 - beta0) * (min(c, N) / N) in fp32, beta0 when N = 0 (momory_pool.per_beta is the host mirror)
__device__ __forceinline__ float per_beta(float beta0, int beta_steps, unsigned c) {
#pragma clang fp contract(off)
    if (beta_steps == 0) return beta0;
    const unsigned k = min(c, (unsigned)beta_steps);
    return beta0 + (1.0f - beta0) * ((float)k / (float)beta_steps);
}

constexpr int PER_LDS_NODES = 2048;     // nodes [0, 2048): the top 11 levels of the tree, staged in LDS by the draw

// One workgroup.  Draw c = the counter before it advances: slot b descends the tree from the root with
// x = (total / B) * (b + u), u = float32(draw_mix(seed, c, b) >> 40) * 2^-24 (stratified sampling, P(row) = leaf / total); the top
// levels come from LDS (one coalesced load), only the last ones are dependent global loads.  Weights w'_b = (leaf * n / total)^-beta_c
// over their maximum.  Then the gather of replay_gather_kernel for the drawn rows (the same copies: the same bits).
__global__ __launch_bounds__(1024) void per_draw_gather_kernel(const float* __restrict__ old_iou, const float* __restrict__ new_iou,
                                                               const float* __restrict__ ann, const float* __restrict__ nann,
                                                               const int64_t* __restrict__ action, const float* __restrict__ rstep,
                                                               const float* __restrict__ rdone, const float* __restrict__ tree,
                                                               PerState* __restrict__ st, int n, int P, int B, int T, float beta0,
                                                               int beta_steps, int64_t* __restrict__ idx_out, float* __restrict__ weights_out,
                                                               float* __restrict__ state, float* __restrict__ new_state,
                                                               int64_t* __restrict__ action_out, float* __restrict__ rstep_out,
                                                               float* __restrict__ rdone_out) {
#pragma clang fp contract(off)
    __shared__ float top[PER_LDS_NODES];
    __shared__ int rows[PER_B_MAX];
    __shared__ float wmax[PER_B_MAX / 64];
    const int tid = threadIdx.x;
    const int ntop = min(PER_LDS_NODES, 2 * P);
    for (int i = tid; i < ntop; i += blockDim.x) top[i] = tree[i];
    const unsigned c = st->counter;
    const unsigned long long seed = st->seed;
    __syncthreads();
    float wp = 0.f;
    if (tid < B) {
        const float u = (float)(draw_mix(seed, c, (unsigned)tid) >> 40) * 0x1p-24f;
        const float total = top[1];
        float x = (total / (float)B) * ((float)tid + u);
        int node = 1;
        while (node < P) {
            const int l_at = 2 * node;
            const float l = l_at < ntop ? top[l_at] : tree[l_at];
            if (x < l) {
                node = l_at;
            } else {
                x -= l;
                node = l_at + 1;
            }
        }
        const int row = min(node - P, n - 1);
        const float leaf = P + row < ntop ? top[P + row] : tree[P + row];
        wp = powf(leaf * (float)n / total, -per_beta(beta0, beta_steps, c));
        rows[tid] = row;
        idx_out[tid] = row;
    }
    float m = wp;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((tid & 63) == 0) wmax[tid >> 6] = m;
    __syncthreads();
    if (tid < B) {
        float mx = wmax[0];
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w) mx = fmaxf(mx, wmax[w]);
        weights_out[tid] = wp / mx;
        const int src = rows[tid];
        action_out[tid] = action[src];
        rstep_out[tid] = rstep[src];
        rdone_out[tid] = rdone[src];
    }
    for (int i = tid; i < B * T; i += blockDim.x) {
        const int b = i / T;
        const size_t s = (size_t)rows[b] * T + (i - b * T), d = (size_t)i * 2;
        state[d] = old_iou[s];
        state[d + 1] = ann[s];
        new_state[d] = new_iou[s];
        new_state[d + 1] = nann[s];
    }
    if (tid == 0) st->counter = c + 1;      // every thread read c before the barrier above
}

// One workgroup.  Slot b's priority is p_b = td_b + eps; the highest slot of a row wins, and its leaf becomes p_b^alpha;
// max_priority = max(max_priority, max_b p_b).  The winners' rows are ranked (sorted), so that at every level the touched nodes form a
// sorted list in which a touched sibling is the next entry: entry i (thread i) owns its node while it lives, absorbs its right sibling
// when that is touched too, and takes an untouched sibling from registers - all of those were loaded from the tree up front, before
// anything was written (a node this launch writes is never read back from memory).  Every touched node, leaves included, is written
// once at the end, so the tree equals a full rebuild from its leaves bit for bit.  Rows outside [0, n) are skipped.
__global__ __launch_bounds__(1024) void per_update_kernel(float* __restrict__ tree, PerState* __restrict__ st, int n, int P, int L,
                                                          const int64_t* __restrict__ idx, const float* __restrict__ td, int B, float alpha,
                                                          float eps) {
#pragma clang fp contract(off)
    constexpr int LMAX = 24;                 // log2 of the largest P (PER_N_MAX rows)
    __shared__ int slot_row[PER_B_MAX];
    __shared__ int win_s[PER_B_MAX];
    __shared__ int node_s[PER_B_MAX];
    __shared__ float val_s[PER_B_MAX];
    __shared__ int nxt_s[PER_B_MAX];
    __shared__ int dead_s[PER_B_MAX];
    __shared__ float pmax[PER_B_MAX / 64];
    __shared__ int m_s;
    const int tid = threadIdx.x;
    int row = -1;
    float p = -INFINITY;
    if (tid < B) {
        const int64_t r = idx[tid];
        row = (r >= 0 && r < n) ? (int)r : -1;
        p = td[tid] + eps;
        slot_row[tid] = row;
    }
    const float old_max = st->max_priority;
    float m = p;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((tid & 63) == 0) pmax[tid >> 6] = m;
    if (tid == 0) m_s = 0;
    __syncthreads();
    bool win = row >= 0;
    for (int b2 = tid + 1; win && b2 < B; ++b2) win = slot_row[b2] != row;
    if (tid < B) win_s[tid] = win;
    __syncthreads();
    if (win) {
        int rank = 0;
        for (int b2 = 0; b2 < B; ++b2) rank += (win_s[b2] && slot_row[b2] < row);
        node_s[rank] = P + row;
        val_s[rank] = powf(p, alpha);
        atomicAdd(&m_s, 1);
    }
    __syncthreads();
    const int cnt = m_s;
    const bool act = tid < cnt;
    const int leaf = act ? node_s[tid] : 0;
    float v = act ? val_s[tid] : 0.f;
    float sib[LMAX];
#pragma unroll
    for (int k = 0; k < LMAX; ++k) sib[k] = tree[(leaf >> k) ^ 1];     // unconditional, all in flight at once: always in bounds
                                                                        // (leaf >> k < 2 past the root, and leaf = 0 off the list)
    if (act) {
        nxt_s[tid] = tid + 1 < cnt ? tid + 1 : -1;
        dead_s[tid] = 0;
    }
    float outv[LMAX + 1];
    outv[0] = v;
    unsigned live_levels = act ? 1u : 0u;
    bool alive = act;
    int nd = leaf;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < LMAX; ++k) {
        if (k >= L) continue;                // uniform: every thread sees the same L
        int j = -1, jn = -1;
        float sv = 0.f;
        bool absorb = false;
        if (alive) {
            j = nxt_s[tid];
            if (!(nd & 1) && j >= 0 && node_s[j] == nd + 1) {
                absorb = true;
                sv = val_s[j];
                jn = nxt_s[j];
            }
        }
        __syncthreads();
        if (absorb) {
            dead_s[j] = 1;
            nxt_s[tid] = jn;
        }
        __syncthreads();
        if (alive) {
            if (dead_s[tid]) {
                alive = false;
            } else {
                v = (nd & 1) ? sib[k] + v : v + (absorb ? sv : sib[k]);
                nd >>= 1;
                node_s[tid] = nd;
                val_s[tid] = v;
                outv[k + 1] = v;
                live_levels |= 1u << (k + 1);
            }
        }
        __syncthreads();
    }
    if (act) {
#pragma unroll
        for (int k = 0; k <= LMAX; ++k)
            if (live_levels & (1u << k)) tree[leaf >> k] = outv[k];
    }
    if (tid == 0) {
        float mx = old_max;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) mx = fmaxf(mx, pmax[w]);
        st->max_priority = mx;
    }
}

}  // namespace ivosw

using namespace ivosw;

// ---------------------------------------------------------------- prioritized replay: entries
static int check_per_n(const char* who, int n) {
    if (n < 1 || n > PER_N_MAX) {
        set_error("%s: n must be in [1, 2^24], got %d", who, n);
        return IVOSW_ERR_ARG;
    }
    return IVOSW_OK;
}

static int check_per_alpha(const char* who, float alpha) {
    if (!(std::isfinite(alpha) && alpha >= 0.f)) {
        set_error("%s: alpha must be finite and >= 0, got %g", who, (double)alpha);
        return IVOSW_ERR_ARG;
    }
    return IVOSW_OK;
}

static int check_per_batch(const char* who, int B) {
    if (B < 1 || B > PER_B_MAX) {
        set_error("%s: B must be in [1, %d], got %d", who, PER_B_MAX, B);
        return IVOSW_ERR_ARG;
    }
    return IVOSW_OK;
}

static int per_block(int B) { return std::max(256, (B + 63) / 64 * 64); }

static int per_log2(int P) {
    int L = 0;
    while ((1 << L) < P) ++L;
    return L;
}

extern "C" size_t ivosw_per_state_bytes(void) { return sizeof(PerState); }

extern "C" size_t ivosw_per_tree_floats(int n) { return (n < 1 || n > PER_N_MAX) ? 0 : 2 * (size_t)per_leaves(n); }

extern "C" int ivosw_per_build(float* tree, int n, const float* old_leaves, int n_old, void* per_state, float alpha, ivosw_stream_t stream) {
    IVOSW_REQUIRE(tree && per_state, "null pointer");
    if (const int rc = check_per_n("ivosw_per_build", n)) return rc;
    IVOSW_REQUIRE(n_old >= 0 && n_old <= n, "n_old must be in [0, n]");
    IVOSW_REQUIRE(n_old == 0 || old_leaves, "null old_leaves with n_old > 0");
    if (const int rc = check_per_alpha("ivosw_per_build", alpha)) return rc;
    IVOSW_ON_DEVICE_OF(tree);
    hipStream_t st = as_stream(stream);
    const int P = per_leaves(n);
    hipLaunchKernelGGL(per_leaves_kernel, dim3((P + 255) / 256), dim3(256), 0, st, tree, P, n, old_leaves, n_old,
                       static_cast<const PerState*>(per_state), alpha);
    for (int lo = P / 2; lo >= 1; lo >>= 1)
        hipLaunchKernelGGL(per_level_kernel, dim3((lo + 255) / 256), dim3(256), 0, st, tree, lo);
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}

extern "C" int ivosw_per_draw_gather(const float* old_iou, const float* new_iou, const float* annotated, const float* next_annotated,
                                     const int64_t* action, const float* reward_step, const float* reward_done, const float* tree,
                                     void* per_state, int n, int B, int T, float beta0, int beta_steps, int64_t* idx_out,
                                     float* weights_out, float* state, float* new_state, int64_t* action_out, float* reward_step_out,
                                     float* reward_done_out, ivosw_stream_t stream) {
    IVOSW_REQUIRE(old_iou && new_iou && annotated && next_annotated && action && reward_step && reward_done && tree && per_state,
                  "null input pointer");
    IVOSW_REQUIRE(idx_out && weights_out && state && new_state && action_out && reward_step_out && reward_done_out, "null output pointer");
    if (const int rc = check_per_n("ivosw_per_draw_gather", n)) return rc;
    if (const int rc = check_per_batch("ivosw_per_draw_gather", B)) return rc;
    IVOSW_REQUIRE(T >= 1, "T must be positive");
    IVOSW_REQUIRE(beta0 >= 0.f && beta0 <= 1.f, "beta0 must be in [0, 1]");
    IVOSW_REQUIRE(beta_steps >= 0, "beta_steps must be >= 0");
    IVOSW_ON_DEVICE_OF(state);
    hipLaunchKernelGGL(per_draw_gather_kernel, dim3(1), dim3(per_block(B)), 0, as_stream(stream), old_iou, new_iou, annotated,
                       next_annotated, action, reward_step, reward_done, tree, static_cast<PerState*>(per_state), n, per_leaves(n), B, T,
                       beta0, beta_steps, idx_out, weights_out, state, new_state, action_out, reward_step_out, reward_done_out);
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}

extern "C" int ivosw_per_update(float* tree, int n, void* per_state, const int64_t* idx, const float* td, int B, float alpha, float eps,
                                ivosw_stream_t stream) {
    IVOSW_REQUIRE(tree && per_state && idx && td, "null pointer");
    if (const int rc = check_per_n("ivosw_per_update", n)) return rc;
    if (const int rc = check_per_batch("ivosw_per_update", B)) return rc;
    if (const int rc = check_per_alpha("ivosw_per_update", alpha)) return rc;
    IVOSW_REQUIRE(std::isfinite(eps) && eps > 0.f, "eps must be finite and > 0");
    IVOSW_ON_DEVICE_OF(tree);
    const int P = per_leaves(n);
    hipLaunchKernelGGL(per_update_kernel, dim3(1), dim3(per_block(B)), 0, as_stream(stream), tree, static_cast<PerState*>(per_state), n, P,
                       per_log2(P), idx, td, B, alpha, eps);
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}

extern "C" int ivosw_clamp_sgd(float* params, const float* grads, float* momentum_buf, int n, float lr, float momentum, float weight_decay,
                               int nesterov, float clamp, float grad_scale, ivosw_stream_t stream) {
    IVOSW_REQUIRE(params && grads && momentum_buf, "null pointer");
    IVOSW_REQUIRE(n > 0, "n must be positive");
    if (const int rc = check_sgd("ivosw_clamp_sgd", lr, momentum, weight_decay, nesterov)) return rc;
    IVOSW_ON_DEVICE_OF(params);
    launch_traversal(clamp_sgd_kernel<true>, clamp_sgd_kernel<false>, {params, grads, momentum_buf}, n, 256, as_stream(stream), params, grads,
                     momentum_buf, n, lr, momentum, weight_decay, nesterov, clamp, grad_scale);
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}

extern "C" size_t ivosw_sgd_state_bytes(void) { return sizeof(SgdDevState); }

extern "C" int ivosw_clamp_sgd_dev_sched(float* params, const float* grads, float* momentum_buf, int n, void* sgd_state, const float* lr_table,
                                         int lr_steps, float momentum, float weight_decay, int nesterov, float clamp, float grad_scale,
                                         ivosw_stream_t stream) {
    IVOSW_REQUIRE(params && grads && momentum_buf && sgd_state, "null pointer");
    IVOSW_REQUIRE(n > 0, "n must be positive");
    if (const int rc = check_lr_table("ivosw_clamp_sgd_dev_sched", lr_table, lr_steps)) return rc;
    if (const int rc = check_sgd("ivosw_clamp_sgd_dev_sched", 0.f, momentum, weight_decay, nesterov)) return rc;
    IVOSW_ON_DEVICE_OF(params);
    launch_traversal(clamp_sgd_sched_kernel<true>, clamp_sgd_sched_kernel<false>, {params, grads, momentum_buf}, n, 1024, as_stream(stream),
                     params, grads, momentum_buf, n, static_cast<SgdDevState*>(sgd_state), lr_table, lr_steps, momentum, weight_decay, nesterov,
                     clamp, grad_scale);
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}

extern "C" size_t ivosw_adam_state_bytes(void) { return sizeof(AdamDevState); }

extern "C" int ivosw_clamp_adam_dev_sched(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int n, void* adam_state,
                                          const float* lr_table, int lr_steps, float beta1, float beta2, float eps, float weight_decay,
                                          float clamp, float grad_scale, ivosw_stream_t stream) {
    IVOSW_REQUIRE(params && grads && exp_avg && exp_avg_sq && adam_state, "null pointer");
    IVOSW_REQUIRE(n > 0, "n must be positive");
    if (const int rc = check_lr_table("ivosw_clamp_adam_dev_sched", lr_table, lr_steps)) return rc;
    if (const int rc = check_adam("ivosw_clamp_adam_dev_sched", beta1, beta2, eps, weight_decay)) return rc;
    IVOSW_ON_DEVICE_OF(params);
    launch_traversal(clamp_adam_dev_sched_kernel<true>, clamp_adam_dev_sched_kernel<false>, {params, grads, exp_avg, exp_avg_sq}, n, 1024,
                     as_stream(stream), params, grads, exp_avg, exp_avg_sq, n, static_cast<AdamDevState*>(adam_state), lr_table, lr_steps, beta1,
                     beta2, eps, weight_decay, clamp, grad_scale);
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}

extern "C" int ivosw_clamp_adam_dev(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int n, void* adam_state,
                                    float lr, float beta1, float beta2, float eps, float weight_decay, float clamp,
                                    float grad_scale, ivosw_stream_t stream) {
    IVOSW_REQUIRE(params && grads && exp_avg && exp_avg_sq && adam_state, "null pointer");
    IVOSW_ON_DEVICE_OF(params);
    IVOSW_REQUIRE(n > 0, "n must be positive");
    launch_traversal(clamp_adam_dev_kernel<true>, clamp_adam_dev_kernel<false>, {params, grads, exp_avg, exp_avg_sq}, n, 1024, as_stream(stream),
                     params, grads, exp_avg, exp_avg_sq, n, static_cast<AdamDevState*>(adam_state), lr, beta1, beta2, eps, weight_decay, clamp,
                     grad_scale);
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}

extern "C" int ivosw_quality_state(const float* scores, int n_obj, int n_frames, const float* counts, double* quality,
                                   float* state, ivosw_stream_t stream) {
    IVOSW_REQUIRE(scores && counts && quality && state, "null pointer");
    IVOSW_ON_DEVICE_OF(state);
    IVOSW_REQUIRE(n_obj > 0 && n_frames > 0, "n_obj and n_frames must be positive");
    hipLaunchKernelGGL(quality_state_kernel, dim3((n_frames + 63) / 64), dim3(64), 0, as_stream(stream), scores, n_obj, n_frames,
                       counts, quality, state);
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}

extern "C" int ivosw_quality_state_ragged(const float* scores, const int* n_obj, const int* lengths, int n_seqs, const float* counts,
                                          double* quality, float* state, ivosw_stream_t stream) {
    IVOSW_REQUIRE(scores && n_obj && lengths && counts && quality && state, "null pointer");
    QualityTable tab;
    const long rows = ragged_rows(__func__, lengths, n_seqs, &tab.seq);
    if (rows < 0) return IVOSW_ERR_ARG;
    long long units = 0;
    for (int k = 0; k < IVOSW_MAX_SEQS; ++k) {
        tab.n_obj[k] = k < n_seqs ? n_obj[k] : 1;
        tab.unit_off[k] = units;
        if (k >= n_seqs) continue;
        if (n_obj[k] < 1) {
            set_error("%s: sequence %d: n_obj %d must be positive", __func__, k, n_obj[k]);
            return IVOSW_ERR_ARG;
        }
        units += (long long)n_obj[k] * lengths[k];
    }
    IVOSW_ON_DEVICE_OF(state);
    hipLaunchKernelGGL(quality_state_ragged_kernel, dim3((unsigned)((rows + 63) / 64)), dim3(64), 0, as_stream(stream), scores, tab, n_seqs,
                       (int)rows, counts, quality, state);
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}

extern "C" int ivosw_clamp_adam(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int n, int step,
                                float lr, float beta1, float beta2, float eps, float weight_decay, float clamp,
                                float grad_scale, ivosw_stream_t stream) {
    IVOSW_REQUIRE(params && grads && exp_avg && exp_avg_sq, "null pointer");
    IVOSW_ON_DEVICE_OF(params);
    IVOSW_REQUIRE(n > 0 && step >= 1, "n must be positive and step >= 1");
    const double bc1 = 1.0 - ipow((double)beta1, step);
    const double bc2 = 1.0 - ipow((double)beta2, step);
    const float step_size = (float)((double)lr / bc1);
    const float bc2_sqrt = (float)sqrt(bc2);
    hipLaunchKernelGGL(clamp_adam_kernel, dim3((n + 255) / 256), dim3(256), 0, as_stream(stream), params, grads, exp_avg,
                       exp_avg_sq, n, step_size, bc2_sqrt, beta1, beta2, eps, weight_decay, clamp, grad_scale);
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}

extern "C" int ivosw_copy_f32(float* dst, const float* src, size_t n, ivosw_stream_t stream) {
    IVOSW_REQUIRE(dst && src, "null pointer");
    IVOSW_ON_DEVICE_OF(dst);
    if (n == 0) return IVOSW_OK;
    hipError_t e = hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, as_stream(stream));
    if (e != hipSuccess) {
        set_error("ivosw_copy_f32: %s", hipGetErrorString(e));
        return IVOSW_ERR_LAUNCH;
    }
    return IVOSW_OK;
}

extern "C" size_t ivosw_target_state_bytes(void) { return sizeof(TargetDevState); }

extern "C" int ivosw_target_update(float* target, const float* policy, int n, int mode, float tau, int period, void* target_state,
                                   ivosw_stream_t stream) {
    if (const int rc = check_target("ivosw_target_update", target_state, mode, tau, period)) return rc;
    IVOSW_REQUIRE(target && policy, "null pointer");
    IVOSW_REQUIRE(target != policy, "target and policy must be different arenas");
    IVOSW_REQUIRE(n > 0, "n must be positive");
    IVOSW_ON_DEVICE_OF(target);
    if (mode == TARGET_SOFT) period = 1;         // not looked at under soft: any value is accepted, none reaches the kernel's modulo
    launch_traversal(target_update_kernel<true>, target_update_kernel<false>, {target, policy}, n, 1024, as_stream(stream), target, policy, n, mode,
                     tau, period, static_cast<TargetDevState*>(target_state));
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}

extern "C" int ivosw_replay_gather(const float* old_iou, const float* new_iou, const float* annotated,
                                   const float* next_annotated, const int64_t* action, const float* reward_step,
                                   const float* reward_done, const int64_t* idx, int B, int T, float* state,
                                   float* new_state, int64_t* action_out, float* reward_step_out, float* reward_done_out,
                                   ivosw_stream_t stream) {
    IVOSW_REQUIRE(old_iou && new_iou && annotated && next_annotated && action && reward_step && reward_done && idx,
                  "null input pointer");
    IVOSW_REQUIRE(state && new_state && action_out && reward_step_out && reward_done_out, "null output pointer");
    IVOSW_ON_DEVICE_OF(state);
    IVOSW_REQUIRE(B > 0 && T > 0, "B and T must be positive");
    hipLaunchKernelGGL(replay_gather_kernel, dim3(B), dim3(64), 0, as_stream(stream), old_iou, new_iou, annotated,
                       next_annotated, action, reward_step, reward_done, idx, B, T, state, new_state, action_out,
                       reward_step_out, reward_done_out);
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}

extern "C" size_t ivosw_replay_draw_state_bytes(void) { return sizeof(DrawState); }

extern "C" unsigned long long ivosw_replay_draw_index(unsigned long long seed, unsigned counter, unsigned slot, int n) {
    if (n <= 0) return 0;
    return (unsigned long long)(((unsigned __int128)draw_mix(seed, counter, slot) * (unsigned long long)n) >> 64);
}

extern "C" int ivosw_replay_draw_gather(const float* old_iou, const float* new_iou, const float* annotated,
                                        const float* next_annotated, const int64_t* action, const float* reward_step,
                                        const float* reward_done, void* draw_state, int n, int B, int T, int64_t* idx_out,
                                        float* state, float* new_state, int64_t* action_out, float* reward_step_out,
                                        float* reward_done_out, ivosw_stream_t stream) {
    IVOSW_REQUIRE(old_iou && new_iou && annotated && next_annotated && action && reward_step && reward_done && draw_state,
                  "null input pointer");
    IVOSW_REQUIRE(idx_out && state && new_state && action_out && reward_step_out && reward_done_out, "null output pointer");
    IVOSW_ON_DEVICE_OF(state);
    IVOSW_REQUIRE(n > 0 && B > 0 && T > 0, "n, B and T must be positive");
    hipLaunchKernelGGL(replay_draw_gather_kernel, dim3(B), dim3(64), 0, as_stream(stream), old_iou, new_iou, annotated,
                       next_annotated, action, reward_step, reward_done, static_cast<DrawState*>(draw_state), n, B, T, idx_out,
                       state, new_state, action_out, reward_step_out, reward_done_out);
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}
