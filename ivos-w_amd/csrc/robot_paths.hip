// The path step of the scribble robot on the device: the skeleton pixels of ivosw_robot_skeleton[_box] become the node lists that
// ivosw_scribble_raster draws - components, double BFS, selection and resampling by ONE workgroup per unit, entirely in LDS.
//
// Reference: davisinteractive's InteractiveScribblesRobot (not in the reference tree) builds a graph of the skeleton pixels with networkx
// and takes longest shortest paths on the CPU; utils/robot.py's paths_from_points is this project's host form of it.  The rule
// (include/ivosw.h, "robot paths") is tests/robot_ref.py's path step and, level by level, tests/robot_paths_ref.py: this project's
// DEFINITION; parity with the library's own robot is restated, not recorded.
//
// ivosw_robot_paths: one workgroup per unit, 64 units per launch (the units are dense, so a group is a base pointer: the call allocates
// nothing, copies nothing and is capture-safe).  n = counts[k] <= cap nodes, node i = the i-th pixel in raster order.
//   A  keys        the points as unsigned (y << 16) | x, one LDS word per node.
//   B  neighbours  uint16 nbr[i][8] in the order N, NE, E, SE, S, SW, W, NW (0xffff: none): E and W are i + 1 and i - 1 when their keys
//                  fit; for the row above and the row below ONE binary search each (the lower bound of (y', x - 1) in the raster-ordered
//                  keys) and at most three entries behind it.  Built once; the BFS never touches a key again.
//   C  components  lock-free union-find on the node indices (atomicMin hooks the larger root below the smaller one, so a component's root
//                  is its FIRST pixel), then one flattening pass and a size count per root.  Roots of fewer than min_nb_nodes nodes die.
//   D  BFS, twice  level-synchronous and multi-source over ALL living components at once (first from the roots, then from the farthest
//                  nodes a).  queue[p] = the node at queue position p.  Per level every (frontier position p, direction d) pair is one
//                  lane: it offers the key ((p + 1) << 3) | d to its neighbour with an LDS atomicMin - a node reached at an earlier
//                  level holds a smaller key and ignores it, the sources hold 0 - and behind a barrier the pair whose key stands IS the
//                  parent edge.  The pairs are visited in ascending key order, so a ballot / prefix count over the winners hands out the
//                  next level's queue positions in exactly the order a FIFO would have appended them.  parent(q) = queue[(mk[q] >> 3) - 1]:
//                  no parent, distance or visited array.  The farthest node per component is an LDS atomicMax of
//                  (level << 16) | (0xffff - node) at the component's root: the highest level, then the lowest raster index.
//   E  selection   max_paths rounds of an LDS atomicMax over the living roots of (length << 16) | (0xffff - root).
//   F  walk        one lane per selected path walks b -> a along the parents into an LDS node list (the lists of different components
//                  are disjoint: n entries serve all of them).
//   G  outputs     one wave per slot: the kept indices rint(i * step) in float64 (this unit is compiled without FMA contraction; the
//                  expression has no addition anyway), equal neighbours dropped by a ballot scan, the tail padded with the last node.
// LDS: 36 bytes per node of cap + 256; no static LDS, no scratch, no global atomics, vector memory operations only.
#include "common.h"
#include <atomic>

namespace ivosw {

int tune_get(const char* key, int dflt);   // capi.cpp

namespace {
constexpr int RP_GROUP = 64;                           // units per launch
constexpr int RP_MAX_PATHS = 8;
constexpr size_t RP_LDS_LIMIT = 160 * 1024;            // what one gfx950 workgroup may have
constexpr size_t RP_LDS_FIXED = 256;                   // counters, wave totals, the selected paths
constexpr size_t RP_NODE_BYTES = 36;                   // nbr 16, key 4, lab 4, mk 4, far 4, queue 2, path list 2
constexpr uint32_t RP_NONE = 0xffffu, RP_UNSET = 0xffffffffu;
constexpr int RP_DEFAULT_THREADS = 64;               // measured (tools/robot_paths_probe.py): 64 < 256 < 1024 threads in every case - the levels are
                                                       // a dependent chain of a few nodes each, and one wave pays nothing for its barriers

// fixed[]: [0] a counter / the round's best, [1] the status, [16..32) wave totals, [32..40) selected length, [40..48) selected b,
// [48..56) selected offset in the path list
constexpr int FX_COUNT = 0, FX_STATUS = 1, FX_WAVE = 16, FX_LEN = 32, FX_B = 40, FX_OFF = 48;

struct RobotPathsArgs {
    const int32_t* points;   // [units][cap]
    const int32_t* counts;   // [units]
    int32_t* nodes;          // [units][max_paths][slot][2]
    int32_t* lens;           // [units][max_paths]
    int32_t* status;         // [units]
    int cap, min_nb_nodes, max_paths, nb_points, slot;
};

__device__ __forceinline__ uint32_t rp_find(const uint32_t* lab, uint32_t i) {
    const volatile uint32_t* l = lab;
    uint32_t p;
    while ((p = l[i]) != i) i = p;
    return i;
}

// the entries of row yy next to column x: the lower bound of (yy, x - 1) in key[lo, hi), then at most three entries; dm / d0 / dp take
// the indices of the neighbours at x - 1, x, x + 1
__device__ __forceinline__ void rp_row(const uint32_t* key, int lo, int hi, uint32_t yy, int x, uint32_t& dm, uint32_t& d0, uint32_t& dp) {
    const uint32_t target = (yy << 16) | (uint32_t)(x > 0 ? x - 1 : 0);
    const int end = hi;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (key[mid] < target) lo = mid + 1; else hi = mid;               // (unsigned: y >= 32768 sets the top bit)
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        if (lo + j >= end) break;
        const uint32_t kk = key[lo + j];
        if ((kk >> 16) != yy) break;
        const int dx = (int)(kk & 0xffffu) - x;
        if (dx > 1) break;
        if (dx == -1) dm = (uint32_t)(lo + j);
        if (dx == 0) d0 = (uint32_t)(lo + j);
        if (dx == 1) dp = (uint32_t)(lo + j);
    }
}

// the level-synchronous sweep from the sources queue[0, ns) (their mk is 0, every other node's RP_UNSET)
template <int T>
__device__ __forceinline__ void rp_bfs(int ns, const uint16_t* nbr, const uint32_t* lab, uint32_t* mk, uint32_t* far, uint16_t* queue,
                                       int* fixed) {
    constexpr int NW = T / 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int p0 = 0, p1 = ns;
    uint32_t level = 0;
    while (p1 > p0) {                                                     // (uniform: every thread holds the same p0, p1)
        ++level;
        const int slots = (p1 - p0) * 8;
        for (int s = tid; s < slots; s += T) {
            const int p = p0 + (s >> 3);
            const uint32_t q = nbr[(int)queue[p] * 8 + (s & 7)];
            if (q != RP_NONE) atomicMin(&mk[q], ((uint32_t)(p + 1) << 3) | (uint32_t)(s & 7));
        }
        __syncthreads();
        int base = p1;
        for (int s0 = 0; s0 < slots; s0 += T) {
            const int s = s0 + tid;
            bool win = false;
            uint32_t q = RP_NONE;
            if (s < slots) {
                const int p = p0 + (s >> 3);
                q = nbr[(int)queue[p] * 8 + (s & 7)];
                win = q != RP_NONE && mk[q] == (((uint32_t)(p + 1) << 3) | (uint32_t)(s & 7));
            }
            const unsigned long long b = __ballot(win);
            int off = base + __popcll(b & ((1ull << lane) - 1ull));
            if constexpr (NW == 1) {
                base += __popcll(b);
            } else {
                if (lane == 0) fixed[FX_WAVE + wave] = __popcll(b);
                __syncthreads();
                int total = 0;
#pragma unroll
                for (int w = 0; w < NW; ++w) {
                    const int t = fixed[FX_WAVE + w];
                    if (w < wave) off += t;
                    total += t;
                }
                base += total;
                __syncthreads();                                          // (the totals are rewritten by the next chunk)
            }
            if (win) {
                queue[off] = (uint16_t)q;
                atomicMax(&far[lab[q]], (level << 16) | (0xffffu - q));
            }
        }
        __syncthreads();
        p0 = p1;
        p1 = base;
    }
}

__device__ __forceinline__ void rp_fill(int2* dst, int slot, int lane) {
    for (int e = lane; e < slot; e += 64) dst[e] = make_int2(-1, -1);
}

template <int T>
__global__ __launch_bounds__(T) void robot_paths_kernel(RobotPathsArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t rp_lds[];
    constexpr int NW = T / 64;
    const int tid = threadIdx.x, u = blockIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cap = a.cap, slot = a.slot, max_paths = a.max_paths;
    int* fixed = reinterpret_cast<int*>(rp_lds);
    uint16_t* nbr = reinterpret_cast<uint16_t*>(rp_lds + RP_LDS_FIXED / 4);          // [cap][8]
    uint32_t* key = rp_lds + RP_LDS_FIXED / 4 + 4 * (size_t)cap;
    uint32_t* lab = key + cap;
    uint32_t* mk = lab + cap;
    uint32_t* far = mk + cap;
    uint16_t* queue = reinterpret_cast<uint16_t*>(far + cap);
    uint16_t* plist = queue + cap;
    int2* out = reinterpret_cast<int2*>(a.nodes) + (size_t)u * max_paths * slot;
    int32_t* lens = a.lens + (size_t)u * max_paths;

    const int count = a.counts[u];
    if (count > cap) {                                                    // the skeleton was truncated: no path is right
        for (int r = wave; r < max_paths; r += NW) {
            rp_fill(out + (size_t)r * slot, slot, lane);
            if (lane == 0) lens[r] = 0;
        }
        if (tid == 0) a.status[u] = 1;
        return;
    }
    const int n = count > 0 ? count : 0;
    const int32_t* pts = a.points + (size_t)u * cap;

    // ---- A: keys, every node its own component
    for (int i = tid; i < n; i += T) {
        key[i] = (uint32_t)pts[i];
        lab[i] = (uint32_t)i;
        mk[i] = 0u;                                                       // (phase C counts the component sizes here)
    }
    if (tid == 0) { fixed[FX_COUNT] = 0; fixed[FX_STATUS] = 0; }
    if (tid < RP_MAX_PATHS) { fixed[FX_LEN + tid] = 0; fixed[FX_OFF + tid] = 0; }
    __syncthreads();

    // ---- B: the neighbour table
    for (int i = tid; i < n; i += T) {
        const uint32_t k = key[i], y = k >> 16;
        const int x = (int)(k & 0xffffu);
        uint32_t dN = RP_NONE, dNE = RP_NONE, dE = RP_NONE, dSE = RP_NONE, dS = RP_NONE, dSW = RP_NONE, dW = RP_NONE, dNW = RP_NONE;
        if (i + 1 < n && x < 65535 && key[i + 1] == k + 1u) dE = (uint32_t)(i + 1);
        if (i > 0 && x > 0 && key[i - 1] == k - 1u) dW = (uint32_t)(i - 1);
        if (y > 0u) rp_row(key, 0, i, y - 1u, x, dNW, dN, dNE);
        if (y < 65535u) rp_row(key, i + 1, n, y + 1u, x, dSW, dS, dSE);
        *reinterpret_cast<uint4*>(nbr + 8 * (size_t)i) = make_uint4(dN | (dNE << 16), dE | (dSE << 16), dS | (dSW << 16), dW | (dNW << 16));
    }
    __syncthreads();

    // ---- C: components (the neighbours with a lower index: N, NE, W, NW)
    for (int i = tid; i < n; i += T) {
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const int dir = d == 0 ? 0 : d == 1 ? 1 : d == 2 ? 6 : 7;
            const uint32_t j = nbr[8 * (size_t)i + dir];
            if (j == RP_NONE) continue;
            uint32_t x = (uint32_t)i, y = j;
            for (;;) {
                x = rp_find(lab, x);
                y = rp_find(lab, y);
                if (x == y) break;
                if (x < y) { const uint32_t t = x; x = y; y = t; }
                const uint32_t old = atomicMin(&lab[x], y);               // hook the larger root below the smaller one
                if (old == x) break;
                x = old;
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < n; i += T) {
        const uint32_t r = rp_find(lab, (uint32_t)i);
        atomicAdd(&mk[r], 1u);
        far[i] = r;                                                       // (parked: lab is still being read)
    }
    __syncthreads();
    for (int i = tid; i < n; i += T) {
        const uint32_t r = far[i];
        lab[i] = r;
        const bool alive = r == (uint32_t)i && mk[i] >= (uint32_t)a.min_nb_nodes;
        far[i] = alive ? 0xffffu - (uint32_t)i : 0u;                      // level 0, the root itself; 0: no living root
        mk[i] = alive ? 0u : RP_UNSET;
        if (alive) queue[atomicAdd(&fixed[FX_COUNT], 1)] = (uint16_t)i;   // (the order of the sources does not reach the outputs)
    }
    __syncthreads();
    const int ns = fixed[FX_COUNT];

    // ---- D: from the roots to a, from a to b
    rp_bfs<T>(ns, nbr, lab, mk, far, queue, fixed);
    if (tid == 0) fixed[FX_COUNT] = 0;
    for (int i = tid; i < n; i += T) mk[i] = RP_UNSET;
    __syncthreads();
    for (int i = tid; i < n; i += T) {
        if (lab[i] == (uint32_t)i && far[i] != 0u) {
            const uint32_t src = 0xffffu - (far[i] & 0xffffu);
            far[i] = 0xffffu - src;
            mk[src] = 0u;
            queue[atomicAdd(&fixed[FX_COUNT], 1)] = (uint16_t)src;
        }
    }
    __syncthreads();
    rp_bfs<T>(ns, nbr, lab, mk, far, queue, fixed);

    // ---- E: the max_paths longest, longest first, ties to the lower root
    int taken = 0;
    for (int r = 0; r < max_paths; ++r) {
        if (tid == 0) fixed[FX_COUNT] = 0;
        __syncthreads();
        for (int i = tid; i < n; i += T)
            if (lab[i] == (uint32_t)i && far[i] != 0u)
                atomicMax(reinterpret_cast<uint32_t*>(&fixed[FX_COUNT]), (((far[i] >> 16) + 1u) << 16) | (0xffffu - (uint32_t)i));
        __syncthreads();
        const uint32_t best = (uint32_t)fixed[FX_COUNT];
        if (best == 0u) break;                                            // (uniform)
        const uint32_t root = 0xffffu - (best & 0xffffu);
        const int len = (int)(best >> 16);
        if (tid == 0) {
            fixed[FX_LEN + r] = len;
            fixed[FX_B + r] = (int)(0xffffu - (far[root] & 0xffffu));
            fixed[FX_OFF + r] = taken;
            far[root] = 0u;
        }
        taken += len;
        __syncthreads();
    }
    __syncthreads();

    // ---- F: the node lists, b -> a along the parents, stored a -> b
    if (tid < max_paths && fixed[FX_LEN + tid] > 0) {
        const int len = fixed[FX_LEN + tid], off = fixed[FX_OFF + tid];
        uint32_t node = (uint32_t)fixed[FX_B + tid];
        for (int j = len - 1; j >= 0; --j) {
            plist[off + j] = (uint16_t)node;
            const uint32_t m = mk[node];
            if (m < 8u || m == RP_UNSET) break;                           // the source (j == 0)
            node = queue[(m >> 3) - 1u];
        }
    }
    __syncthreads();

    // ---- G: the slots
    for (int r = wave; r < max_paths; r += NW) {
        int2* dst = out + (size_t)r * slot;
        const int len = fixed[FX_LEN + r];
        const uint16_t* pl = plist + fixed[FX_OFF + r];
        int written = 0;
        if (len == 0) {
            rp_fill(dst, slot, lane);
        } else if (a.nb_points <= 0) {
            if (len > slot) {
                rp_fill(dst, slot, lane);
                if (lane == 0) fixed[FX_STATUS] = 2;
            } else {
                for (int e = lane; e < slot; e += 64) {
                    const uint32_t k = key[pl[e < len ? e : len - 1]];
                    dst[e] = make_int2((int)(k & 0xffffu), (int)(k >> 16));
                }
                written = len;
            }
        } else {
            const int m = a.nb_points < len ? a.nb_points : len;
            const double step = m > 1 ? (double)(len - 1) / (double)(m - 1) : 0.0;
            for (int i0 = 0; i0 < m; i0 += 64) {
                const int i = i0 + lane;
                bool keep = false;
                int idx = 0;
                if (i < m) {
                    idx = m > 1 && i == m - 1 ? len - 1 : (int)rint((double)i * step);
                    keep = i == 0 || idx != (int)rint((double)(i - 1) * step);
                }
                const unsigned long long b = __ballot(keep);
                if (keep) {
                    const uint32_t k = key[pl[idx]];
                    dst[written + __popcll(b & ((1ull << lane) - 1ull))] = make_int2((int)(k & 0xffffu), (int)(k >> 16));
                }
                written += __popcll(b);
            }
            const uint32_t k = key[pl[m > 1 ? len - 1 : 0]];              // the last KEPT node (one kept node: the first of the path)
            for (int e = written + lane; e < slot; e += 64) dst[e] = make_int2((int)(k & 0xffffu), (int)(k >> 16));
        }
        if (lane == 0) lens[r] = written;
    }
    __syncthreads();
    if (tid == 0) a.status[u] = fixed[FX_STATUS];
}

template <int T>
void rp_launch(const RobotPathsArgs& a, int cnt, size_t lds, hipStream_t st, int dev) {
    static std::atomic<bool> attr_set[64];                                 // per device: the kernel may take more than the default 64 KB
    if (dev >= 0 && dev < 64 && !attr_set[dev].load(std::memory_order_acquire)) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(robot_paths_kernel<T>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)RP_LDS_LIMIT);
        (void)hipGetLastError();
        attr_set[dev].store(true, std::memory_order_release);
    }
    hipLaunchKernelGGL(robot_paths_kernel<T>, dim3((unsigned)cnt), dim3(T), lds, st, a);
}
}  // namespace
}  // namespace ivosw

extern "C" int ivosw_robot_paths_max_cap(void) {
    using namespace ivosw;
    return (int)((RP_LDS_LIMIT - RP_LDS_FIXED) / RP_NODE_BYTES);
}

extern "C" int ivosw_robot_paths(const int32_t* points, const int32_t* counts, int m, int cap, int H, int W, int min_nb_nodes, int max_paths,
                                 int nb_points, int slot, int32_t* nodes, int32_t* lens, int32_t* status, ivosw_stream_t stream) {
    using namespace ivosw;
    IVOSW_REQUIRE(points, "null points");
    IVOSW_REQUIRE(counts, "null counts");
    IVOSW_REQUIRE(nodes, "null nodes");
    IVOSW_REQUIRE(lens, "null lens");
    IVOSW_REQUIRE(status, "null status");
    IVOSW_REQUIRE(((uintptr_t)nodes & 7) == 0, "nodes off the 8-byte grid (a node is stored as one (px, py) pair)");
    IVOSW_REQUIRE(m >= 1, "m < 1");
    if (cap < 1 || cap > ivosw_robot_paths_max_cap()) {
        set_error("%s: cap %d outside [1, %d]: the tables of one unit are %zu bytes per node and %zu fixed bytes of the %zu bytes of LDS of "
                  "one workgroup (ivosw_robot_paths_max_cap)", __func__, cap, ivosw_robot_paths_max_cap(), RP_NODE_BYTES, RP_LDS_FIXED,
                  RP_LDS_LIMIT);
        return IVOSW_ERR_ARG;
    }
    IVOSW_REQUIRE(H >= 1 && H <= 65535, "H outside [1, 65535]");
    IVOSW_REQUIRE(W >= 1 && W <= 65535, "W outside [1, 65535]");
    IVOSW_REQUIRE(min_nb_nodes >= 1, "min_nb_nodes < 1");
    IVOSW_REQUIRE(max_paths >= 1 && max_paths <= RP_MAX_PATHS, "max_paths outside [1, 8]");
    IVOSW_REQUIRE(slot >= 1 && slot <= cap, "slot outside [1, cap]");
    IVOSW_REQUIRE(nb_points <= slot, "nb_points > slot");
    IVOSW_ON_DEVICE_OF(points);
    hipStream_t st = as_stream(stream);
    const size_t lds = RP_LDS_FIXED + RP_NODE_BYTES * (size_t)cap;
    const int threads = tune_get("RPATHS_T", RP_DEFAULT_THREADS);          // 64, 256 or 1024 (tools/robot_paths_probe.py); else the default
    for (int g0 = 0; g0 < m; g0 += RP_GROUP) {
        const int cnt = m - g0 < RP_GROUP ? m - g0 : RP_GROUP;
        RobotPathsArgs a{points + (size_t)g0 * cap, counts + g0, nodes + (size_t)g0 * max_paths * slot * 2, lens + (size_t)g0 * max_paths,
                         status + g0, cap, min_nb_nodes, max_paths, nb_points, slot};
        if (threads == 256) rp_launch<256>(a, cnt, lds, st, dscope__.dev);
        else if (threads == 1024) rp_launch<1024>(a, cnt, lds, st, dscope__.dev);
        else rp_launch<64>(a, cnt, lds, st, dscope__.dev);
        IVOSW_CHECK_LAUNCH();
    }
    return IVOSW_OK;
}
