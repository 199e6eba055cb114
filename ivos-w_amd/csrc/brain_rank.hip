// Ranking the Brain's Q values (Agent.action, models/agent.py:168-196): the argmax of every row or sequence, and the k strongest frames
// of every sequence, masked and optionally spread in time.  Reads Q (and the state's annotation column); of the forward pass it shares
// the sequence table only.
#include <cmath>

#include "common.h"

using namespace ivosw;

// first maximum of each row (numpy / torch-CPU argmax): one wave per row, lanes stride the frames, ties go to the lower index
__global__ __launch_bounds__(64) void argmax_rows_kernel(const float* __restrict__ q, int N, int T, int64_t* __restrict__ idx) {
    const int n = blockIdx.x, lane = threadIdx.x;
    const float* r = q + (size_t)n * T;
    float best = -INFINITY;
    int am = 0x7fffffff;
    for (int t = lane; t < T; t += 64) {
        const float v = r[t];
        if (v > best || am == 0x7fffffff) { best = v; am = t; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int oa = __shfl_xor(am, o, 64);
        if (oa != 0x7fffffff && (am == 0x7fffffff || ob > best || (ob == best && oa < am))) { best = ob; am = oa; }
    }
    if (lane == 0) idx[n] = am;
}

extern "C" int ivosw_brain_argmax(const float* q, int N, int T, int64_t* idx, ivosw_stream_t stream) {
    IVOSW_REQUIRE(q && idx, "null pointer");
    IVOSW_ON_DEVICE_OF(idx);
    IVOSW_REQUIRE(N > 0 && T > 0, "N and T must be positive");
    hipLaunchKernelGGL(argmax_rows_kernel, dim3(N), dim3(64), 0, as_stream(stream), q, N, T, idx);
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}

// argmax_rows_kernel over a sequence table: one wave per sequence, the same scan and the same tie rule (the lower index wins)
__global__ __launch_bounds__(64) void argmax_ragged_kernel(const float* __restrict__ q, SeqTable tab, int64_t* __restrict__ idx) {
    const int k = blockIdx.x, lane = threadIdx.x;
    const int r0 = tab.row_off[k], T = tab.row_off[k + 1] - r0;
    const float* r = q + r0;
    float best = -INFINITY;
    int am = 0x7fffffff;
    for (int t = lane; t < T; t += 64) {
        const float v = r[t];
        if (v > best || am == 0x7fffffff) { best = v; am = t; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int oa = __shfl_xor(am, o, 64);
        if (oa != 0x7fffffff && (am == 0x7fffffff || ob > best || (ob == best && oa < am))) { best = ob; am = oa; }
    }
    if (lane == 0) idx[k] = am;
}

extern "C" int ivosw_brain_argmax_ragged(const float* q, const int* lengths, int n_seqs, int64_t* idx, ivosw_stream_t stream) {
    IVOSW_REQUIRE(q && lengths && idx, "null pointer");
    SeqTable tab;
    if (ragged_rows(__func__, lengths, n_seqs, &tab) < 0) return IVOSW_ERR_ARG;
    IVOSW_ON_DEVICE_OF(idx);
    hipLaunchKernelGGL(argmax_ragged_kernel, dim3(n_seqs), dim3(64), 0, as_stream(stream), q, tab, idx);
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}

// ---------------------------------------------------------------- ragged masked top-k: the k strongest frames of every sequence
// One 64-bit key per frame, larger = stronger, unique inside a sequence:
//   bit 53      always set (0 is "no frame")
//   bit 52      the tier: set for a frame that is not annotated when annotated frames are to come last
//   bits 51-20  the float as an order-preserving uint32: -0 canonicalised to +0, NaN mapped to 0 (below -inf, which maps to 0x007fffff)
//   bits 19-0   2^20 - 1 - t (RAGGED_MAX_ROWS = 2^20): among equal values the lower index wins
__device__ __forceinline__ uint64_t topk_key(float v, bool strong, int t) {
    uint32_t u = __float_as_uint(v);
    if ((u & 0x7fffffffu) > 0x7f800000u) {
        u = 0;
    } else {
        if (u == 0x80000000u) u = 0;
        u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    }
    return (1ull << 53) | ((uint64_t)strong << 52) | ((uint64_t)u << 20) | (uint64_t)(0xfffff - t);
}

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o, 64);
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, 64);
        const uint64_t other = ((uint64_t)hi << 32) | lo;
        v = other > v ? other : v;
    }
    return v;
}

// One wave per sequence.  Round j finds the largest key strictly below round j - 1's winner (lanes stride the frames, then a 64-lane
// butterfly on the key): the keys are unique, so nothing is marked as taken, and there is no LDS and no atomic.  A sequence of up to
// 64 TOPK_TRIPS frames keeps its keys in registers over the rounds (q and state are read once); a longer one rebuilds them from memory
// every round.  Lane j keeps round j's winner; at the end the first k lanes store their slot (and fetch its q).
//
// SPREAD (ivosw_brain_topk_spread_ragged): the same order walked greedily, a frame accepted only if it lies `gap` or more frames from every
// frame accepted before it.  What is accepted only ever suppresses more, so the next frame of the walk is the largest key that is not
// suppressed yet, and a round stays one scan and one butterfly; a winner suppresses itself, so there is no bound.  In registers a
// suppressed key is zeroed in place.  On the rescan path lane j also keeps round j's frame index (TOPK_FAR while it has none), the rounds
// read the IVOSW_MAX_CANDIDATES lanes back with v_readlane at constant lane numbers (wave-uniform, no array that is indexed at run time)
// and test every rebuilt key against them.  `first` >= 0 is accepted before the walk as slot 0, whatever its key.
constexpr int TOPK_TRIPS = 4;
constexpr int TOPK_FAR = -(1 << 22);                                        // further than any gap (at most 2^20) from every frame
// What the spread instantiation takes besides: the gap and the forced first candidates, like the sequence table inside the kernel arguments.
template <bool SPREAD> struct SpreadArgs {};
template <> struct SpreadArgs<true> {
    int gap;
    int first[IVOSW_MAX_SEQS];
};
template <bool SPREAD>
__global__ __launch_bounds__(64) void topk_ragged_kernel(const float* __restrict__ q, const float* __restrict__ state, SeqTable tab, int k,
                                                         int skip, int64_t* __restrict__ idx, float* __restrict__ qv, SpreadArgs<SPREAD> sp) {
    const int s = blockIdx.x, lane = threadIdx.x;
    const int r0 = tab.row_off[s], T = tab.row_off[s + 1] - r0;
    const float* r = q + r0;
    const float* c = skip ? state + (size_t)r0 * 2 + 1 : nullptr;           // column 1 of the state: how often the frame was annotated
    uint64_t bound = ~0ull, mine = 0;
    int gap = 1, first = -1, j0 = 0;
    if constexpr (SPREAD) {
        gap = sp.gap;
        first = sp.first[s];
        if (first >= 0) {                                                   // (wave-uniform) slot 0 is given
            if (lane == 0) mine = (1ull << 53) | (uint64_t)(0xfffff - first);
            j0 = 1;
        }
    }
    if (T <= 64 * TOPK_TRIPS) {
        uint64_t key[TOPK_TRIPS];
#pragma unroll
        for (int i = 0; i < TOPK_TRIPS; ++i) {
            const int t = lane + 64 * i;
            key[i] = t < T ? topk_key(r[t], skip && c[2 * t] == 0.f, t) : 0;
            if constexpr (SPREAD)
                if (first >= 0 && abs(t - first) < gap) key[i] = 0;
        }
        for (int j = j0; j < k; ++j) {
            uint64_t best = 0;
#pragma unroll
            for (int i = 0; i < TOPK_TRIPS; ++i)
                if ((SPREAD || key[i] < bound) && key[i] > best) best = key[i];
            best = wave_max_u64(best);
            if (best == 0) break;                                           // (wave-uniform) every frame is ranked: the rest stays -1
            if (lane == j) mine = best;
            if constexpr (SPREAD) {
                const int w = 0xfffff - (int)(best & 0xfffff);
#pragma unroll
                for (int i = 0; i < TOPK_TRIPS; ++i)
                    if (abs(lane + 64 * i - w) < gap) key[i] = 0;
            } else {
                bound = best;
            }
        }
    } else {
        int taken = TOPK_FAR;                                               // SPREAD: lane j holds the frame of slot j
        if constexpr (SPREAD)
            if (first >= 0 && lane == 0) taken = first;
        for (int j = j0; j < k; ++j) {
            uint64_t best = 0;
            if constexpr (SPREAD) {
                int w[IVOSW_MAX_CANDIDATES];
#pragma unroll
                for (int a = 0; a < IVOSW_MAX_CANDIDATES; ++a) w[a] = __builtin_amdgcn_readlane(taken, a);
                for (int t = lane; t < T; t += 64) {
                    const uint64_t key = topk_key(r[t], skip && c[2 * t] == 0.f, t);
                    bool open = true;
#pragma unroll
                    for (int a = 0; a < IVOSW_MAX_CANDIDATES; ++a) open = open && abs(t - w[a]) >= gap;
                    if (open && key > best) best = key;
                }
            } else {
                for (int t = lane; t < T; t += 64) {
                    const uint64_t key = topk_key(r[t], skip && c[2 * t] == 0.f, t);
                    if (key < bound && key > best) best = key;
                }
            }
            best = wave_max_u64(best);
            if (best == 0) break;
            if (lane == j) mine = best;
            if constexpr (SPREAD) {
                if (lane == j) taken = 0xfffff - (int)(best & 0xfffff);
            } else {
                bound = best;
            }
        }
    }
    if (lane < k) {
        const int t = mine ? 0xfffff - (int)(mine & 0xfffff) : -1;
        idx[(size_t)s * k + lane] = t;
        if (qv) qv[(size_t)s * k + lane] = t >= 0 ? r[t] : 0.f;
    }
}

extern "C" int ivosw_brain_topk_ragged(const float* q, const float* state, const int* lengths, int n_seqs, int k, int skip_annotated,
                                       int64_t* idx, float* qv, ivosw_stream_t stream) {
    IVOSW_REQUIRE(q, "q is a null pointer");
    IVOSW_REQUIRE(lengths, "lengths is a null pointer");
    IVOSW_REQUIRE(idx, "idx is a null pointer");
    if (k < 1 || k > IVOSW_MAX_CANDIDATES) {
        set_error("%s: k %d outside [1, %d]", __func__, k, IVOSW_MAX_CANDIDATES);
        return IVOSW_ERR_ARG;
    }
    IVOSW_REQUIRE(!skip_annotated || state, "skip_annotated needs state, which is a null pointer");
    SeqTable tab;
    if (ragged_rows(__func__, lengths, n_seqs, &tab) < 0) return IVOSW_ERR_ARG;
    IVOSW_ON_DEVICE_OF(idx);
    hipLaunchKernelGGL(topk_ragged_kernel<false>, dim3(n_seqs), dim3(64), 0, as_stream(stream), q, state, tab, k, skip_annotated ? 1 : 0, idx, qv,
                       SpreadArgs<false>{});
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}

extern "C" int ivosw_brain_topk_spread_ragged(const float* q, const float* state, const int* lengths, int n_seqs, int k, int skip_annotated,
                                              int gap, const int* first, int64_t* idx, float* qv, ivosw_stream_t stream) {
    IVOSW_REQUIRE(q, "q is a null pointer");
    IVOSW_REQUIRE(lengths, "lengths is a null pointer");
    IVOSW_REQUIRE(idx, "idx is a null pointer");
    if (k < 1 || k > IVOSW_MAX_CANDIDATES) {
        set_error("%s: k %d outside [1, %d]", __func__, k, IVOSW_MAX_CANDIDATES);
        return IVOSW_ERR_ARG;
    }
    IVOSW_REQUIRE(!skip_annotated || state, "skip_annotated needs state, which is a null pointer");
    if (gap < 1 || gap > IVOSW_MAX_CANDIDATE_GAP) {
        set_error("%s: gap %d outside [1, 2^20]", __func__, gap);
        return IVOSW_ERR_ARG;
    }
    SeqTable tab;
    if (ragged_rows(__func__, lengths, n_seqs, &tab) < 0) return IVOSW_ERR_ARG;
    SpreadArgs<true> forced;
    forced.gap = gap;
    for (int s = 0; s < IVOSW_MAX_SEQS; ++s) forced.first[s] = -1;
    for (int s = 0; first && s < n_seqs; ++s) {
        if (first[s] < -1 || first[s] >= lengths[s]) {
            set_error("%s: first[%d] = %d outside [-1, %d), the frames of sequence %d", __func__, s, first[s], lengths[s], s);
            return IVOSW_ERR_ARG;
        }
        forced.first[s] = first[s];
    }
    IVOSW_ON_DEVICE_OF(idx);
    hipLaunchKernelGGL(topk_ragged_kernel<true>, dim3(n_seqs), dim3(64), 0, as_stream(stream), q, state, tab, k, skip_annotated ? 1 : 0, idx, qv,
                       forced);
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}
