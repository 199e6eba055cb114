// The error-driven scribble robot on the device: the skeleton of the region where a prediction misses an object, thinned by ONE
// workgroup entirely in LDS - no global pass, no host iteration loop, no grid-wide synchronisation.
//
// Reference: davisinteractive's InteractiveScribblesRobot (not in the reference tree; produce_reward.py:133 sets its min_nb_nodes) skeletonises
// the error region on the CPU at every interaction of every episode (the drivers are "bound by ATNet + robot scribbles").
// The thinning rule here is Zhang-Suen (1984) as published; include/ivosw.h states it in full and tests/robot_ref.py restates it per
// pixel.  It is this project's DEFINITION: parity with the library's own skeletoniser (skimage's) is restated, not recorded.
//
// ivosw_robot_skeleton: one workgroup of 1024 threads per unit = (frame, object); the units travel as a host table inside the kernel
// arguments (64 per launch, longer lists in groups), so the call allocates nothing, copies nothing and is capture-safe.
//   A  error plane   bit (x & 31) of word (x >> 5) of row y = gt == o && pred != o, built with LDS ORs from 16-byte loads of the frame's
//                    16-byte-aligned body (a 16-pixel group may span a row end: it is split there); the ragged head and tail of the frame,
//                    and a frame whose gt and pred are not on the same 16-byte phase, go byte by byte.  The box of the non-zero words
//                    (LDS min / max) bounds the work of phase B: thinning only ever clears bits.
//   B  thinning      32 pixels per lane and step with word logic: the eight neighbour planes are shifts of the three rows' words with
//                    carries from the words to the left and right, B (2 <= B <= 6) from a bit-sliced adder tree, A == 1 from a
//                    one / two-or-more pair over the eight 0 -> 1 steps.  Sub-iteration 1 reads plane 0 and writes plane 1, sub-iteration 2
//                    the other way, a barrier between; a workgroup-wide OR of "something was deleted" steers the loop (at most
//                    max(H, W) iterations): a flag word in LDS, two of them in turn, so that one barrier per iteration serves it.
//                    (__syncthreads_or would bring 256 bytes of static LDS of its own, which the size limit does not count.)
//   C  outputs       the skeleton pixels in raster order: a contiguous run of words per thread, a workgroup scan of the runs' popcounts,
//                    then every thread writes its pixels behind its offset - no atomics.
// LDS: two planes of H * ceil(W / 32) words + 256 bytes; no scratch, no global atomics, vector memory operations only.
#include "common.h"
#include <atomic>

namespace ivosw {

namespace {
constexpr int ROBOT_THREADS = 1024;
constexpr int ROBOT_GROUP = 64;                       // units per launch
constexpr size_t ROBOT_LDS_LIMIT = 160 * 1024;        // what one gfx950 workgroup may have
constexpr size_t ROBOT_LDS_FIXED = 256;               // box, deletion flags, wave totals (the kernel has NO static LDS: tests/test_robot_option.py)

struct RobotArgs {
    const uint8_t* gt;       // [n][H][W]
    const uint8_t* pred;     // [n][H][W] or nullptr (all background)
    int32_t* points;         // [units][cap]
    int32_t* counts;         // [units]
    int32_t* iters;          // [units]
    uint32_t* skel;          // [units][H][WW] or nullptr
    int H, W, WW, cap, max_iters;
    int frame[ROBOT_GROUP];
    uint8_t object[ROBOT_GROUP];
};

// bytes of `g` equal to o and of `p` different from o, 4 pixels -> 4 bits
__device__ __forceinline__ uint32_t err4(uint32_t g, uint32_t p, uint32_t o) {
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t gb = (g >> (8 * j)) & 0xffu, pb = (p >> (8 * j)) & 0xffu;
        m |= (uint32_t)(gb == o && pb != o) << j;
    }
    return m;
}

// one word of one sub-iteration: the new value of c (bits may only be cleared)
__device__ __forceinline__ uint32_t thin_word(const uint32_t* __restrict__ src, int y, int wx, int H, int WW, int sub, uint32_t c) {
    const uint32_t* row = src + y * WW + wx;
    const bool up = y > 0, dn = y + 1 < H, lf = wx > 0, rt = wx + 1 < WW;
    const uint32_t ml = lf ? row[-1] : 0u, mr = rt ? row[1] : 0u;
    const uint32_t uc = up ? row[-WW] : 0u, ul = up && lf ? row[-WW - 1] : 0u, ur = up && rt ? row[-WW + 1] : 0u;
    const uint32_t dc = dn ? row[WW] : 0u, dl = dn && lf ? row[WW - 1] : 0u, dr = dn && rt ? row[WW + 1] : 0u;
    // the neighbour at x - 1 sits one bit below: shift up, carry from the left word's top bit; x + 1 the other way
    const uint32_t p2 = uc, p3 = (uc >> 1) | (ur << 31), p4 = (c >> 1) | (mr << 31), p5 = (dc >> 1) | (dr << 31);
    const uint32_t p6 = dc, p7 = (dc << 1) | (dl >> 31), p8 = (c << 1) | (ml >> 31), p9 = (uc << 1) | (ul >> 31);
    // B: 8 one-bit addends -> b3 b2 b1 b0
    const uint32_t s1 = p2 ^ p3 ^ p4, c1 = (p2 & p3) | (p4 & (p2 ^ p3));
    const uint32_t s2 = p5 ^ p6 ^ p7, c2 = (p5 & p6) | (p7 & (p5 ^ p6));
    const uint32_t s3 = p8 ^ p9, c3 = p8 & p9;
    const uint32_t b0 = s1 ^ s2 ^ s3, c4 = (s1 & s2) | (s3 & (s1 ^ s2));
    const uint32_t s5 = c1 ^ c2 ^ c3, c5 = (c1 & c2) | (c3 & (c1 ^ c2));
    const uint32_t b1 = s5 ^ c4, c6 = s5 & c4;
    const uint32_t b2 = c5 ^ c6, b3 = c5 & c6;
    const uint32_t b_ok = (b1 | b2) & ~b3 & ~(b2 & b1 & b0);                // 2 <= B <= 6
    // A: the 0 -> 1 steps around P2 .. P9, P2; exactly one of the eight
    const uint32_t t[8] = {~p2 & p3, ~p3 & p4, ~p4 & p5, ~p5 & p6, ~p6 & p7, ~p7 & p8, ~p8 & p9, ~p9 & p2};
    uint32_t one = 0, two = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        two |= one & t[k];
        one |= t[k];
    }
    const uint32_t a_ok = one & ~two;
    const uint32_t cond = sub == 0 ? ~(p2 & p4 & p6) & ~(p4 & p6 & p8) : ~(p2 & p4 & p8) & ~(p2 & p6 & p8);
    return c & ~(b_ok & a_ok & cond);
}
}  // namespace

__global__ __launch_bounds__(ROBOT_THREADS) void robot_skeleton_kernel(RobotArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t robot_lds[];
    const int tid = threadIdx.x, u = blockIdx.x;
    const int H = a.H, W = a.W, WW = a.WW, N = H * WW;
    uint32_t* p0 = robot_lds;
    uint32_t* p1 = robot_lds + N;
    int* fixed = reinterpret_cast<int*>(robot_lds + 2 * N);               // [0..3] box = min y, max y, min word, max word; [8..9] deletion flags; [16..31] wave totals
    const uint32_t o = a.object[u];
    const size_t HW = (size_t)H * W;
    const uint8_t* gt = a.gt + (size_t)a.frame[u] * HW;
    const uint8_t* pr = a.pred ? a.pred + (size_t)a.frame[u] * HW : nullptr;

    for (int i = tid; i < 2 * N; i += ROBOT_THREADS) robot_lds[i] = 0u;
    if (tid == 0) { fixed[0] = H; fixed[1] = -1; fixed[2] = WW; fixed[3] = -1; fixed[8] = 0; fixed[9] = 0; }
    __syncthreads();

    // ---- A: the error plane
    const bool vec = !pr || (((uintptr_t)gt ^ (uintptr_t)pr) & 15) == 0;
    const size_t head = vec ? min((size_t)((16 - ((uintptr_t)gt & 15)) & 15), HW) : HW;      // bytes before the first aligned group
    const size_t groups = (HW - head) / 16, tail0 = head + groups * 16;
    for (size_t g = tid; g < groups; g += ROBOT_THREADS) {
        const size_t pix = head + g * 16;
        const uint4 gv = *reinterpret_cast<const uint4*>(gt + pix);
        uint4 pv = make_uint4(0, 0, 0, 0);
        if (pr) pv = *reinterpret_cast<const uint4*>(pr + pix);
        uint32_t m = err4(gv.x, pv.x, o) | (err4(gv.y, pv.y, o) << 4) | (err4(gv.z, pv.z, o) << 8) | (err4(gv.w, pv.w, o) << 12);
        if (!m) continue;
        int y = (int)(pix / (size_t)W), x = (int)(pix - (size_t)y * W), left = 16;
        while (m) {                                                       // a run per row the group touches
            const int r = min(left, W - x);
            const uint64_t bits = (uint64_t)(m & ((1u << r) - 1u)) << (x & 31);
            uint32_t* w = p0 + y * WW + (x >> 5);
            if ((uint32_t)bits) atomicOr(w, (uint32_t)bits);
            if ((uint32_t)(bits >> 32)) atomicOr(w + 1, (uint32_t)(bits >> 32));      // only when the run itself reaches the next word
            m >>= r;
            left -= r;
            ++y;
            x = 0;
        }
    }
    for (size_t k = tid; k < head + (HW - tail0); k += ROBOT_THREADS) {   // the ragged ends (all of a frame off the common phase)
        const size_t pix = k < head ? k : tail0 + (k - head);
        if (gt[pix] == o && (!pr || pr[pix] != o)) {
            const int y = (int)(pix / (size_t)W), x = (int)(pix - (size_t)y * W);
            atomicOr(p0 + y * WW + (x >> 5), 1u << (x & 31));
        }
    }
    __syncthreads();
    {
        int y0 = H, y1 = -1, w0 = WW, w1 = -1;
        for (int i = tid; i < N; i += ROBOT_THREADS) {
            if (p0[i]) {
                const int y = i / WW, wx = i - y * WW;
                y0 = min(y0, y); y1 = max(y1, y); w0 = min(w0, wx); w1 = max(w1, wx);
            }
        }
        y0 = wave_min(y0); y1 = wave_max(y1); w0 = wave_min(w0); w1 = wave_max(w1);
        if ((tid & 63) == 0 && y1 >= 0) {
            atomicMin(&fixed[0], y0); atomicMax(&fixed[1], y1); atomicMin(&fixed[2], w0); atomicMax(&fixed[3], w1);
        }
    }
    __syncthreads();

    // ---- B: Zhang-Suen inside the box (both planes are zero outside it)
    const int by0 = fixed[0], bh = fixed[1] - by0 + 1, bw0 = fixed[2], bw = fixed[3] - bw0 + 1;
    const int items = bh > 0 ? bh * bw : 0;
    int iters = -1;
    for (int it = 0; it < a.max_iters; ++it) {
        uint32_t gone = 0;
        for (int i = tid; i < items; i += ROBOT_THREADS) {
            const int yy = i / bw, y = by0 + yy, wx = bw0 + (i - yy * bw);
            const uint32_t c = p0[y * WW + wx];
            const uint32_t v = c ? thin_word(p0, y, wx, H, WW, 0, c) : 0u;
            p1[y * WW + wx] = v;
            gone |= c ^ v;
        }
        __syncthreads();
        for (int i = tid; i < items; i += ROBOT_THREADS) {
            const int yy = i / bw, y = by0 + yy, wx = bw0 + (i - yy * bw);
            const uint32_t c = p1[y * WW + wx];
            const uint32_t v = c ? thin_word(p1, y, wx, H, WW, 1, c) : 0u;
            p0[y * WW + wx] = v;
            gone |= c ^ v;
        }
        // flag (it & 1) is written here, behind this iteration's middle barrier, and read behind the closing one; thread 0 then clears
        // the OTHER flag, which was last read before the middle barrier and is next written behind the next one
        int* flag = fixed + 8 + (it & 1);
        if (gone) *flag = 1;
        __syncthreads();                                                  // (the barrier that orders this iteration's plane stores, too)
        const int any = *flag;
        if (tid == 0) fixed[8 + ((it + 1) & 1)] = 0;
        if (!any) {
            iters = it;
            break;
        }
    }

    // ---- C: the outputs, from plane 0
    if (a.skel) {
        uint32_t* out = a.skel + (size_t)u * N;
        for (int i = tid; i < N; i += ROBOT_THREADS) out[i] = p0[i];
    }
    const int chunk = (N + ROBOT_THREADS - 1) / ROBOT_THREADS;
    const int i0 = min(tid * chunk, N), i1 = min(i0 + chunk, N);
    int mine = 0;
    for (int i = i0; i < i1; ++i) mine += __popc(p0[i]);
    int incl = mine;                                                      // inclusive scan inside the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int v = __shfl_up(incl, d, 64);
        if ((tid & 63) >= d) incl += v;
    }
    if ((tid & 63) == 63) fixed[16 + (tid >> 6)] = incl;
    __syncthreads();
    int base = incl - mine, total = 0;
    for (int w = 0; w < ROBOT_THREADS / 64; ++w) {
        const int t = fixed[16 + w];
        if (w < (tid >> 6)) base += t;
        total += t;
    }
    int32_t* pts = a.points + (size_t)u * a.cap;
    if (mine) {
        int y = i0 / WW, wx = i0 - y * WW;
        for (int i = i0; i < i1; ++i) {
            uint32_t bits = p0[i];
            while (bits) {
                const int b = __ffs((int)bits) - 1;
                bits &= bits - 1u;
                if (base < a.cap) pts[base] = (y << 16) | (wx * 32 + b);
                ++base;
            }
            if (++wx == WW) { wx = 0; ++y; }
        }
    }
    if (tid == 0) {
        a.counts[u] = total;
        a.iters[u] = iters;
    }
}

}  // namespace ivosw

extern "C" int ivosw_robot_skeleton_fits(int H, int W) {
    using namespace ivosw;
    if (H < 1 || W < 1 || H > 65535 || W > 65535) return 0;
    return 2 * (size_t)H * (size_t)((W + 31) / 32) * sizeof(uint32_t) + ROBOT_LDS_FIXED <= ROBOT_LDS_LIMIT ? 1 : 0;
}

extern "C" int ivosw_robot_skeleton(const uint8_t* gt, const uint8_t* pred, int n, int H, int W, const int32_t* units_host, int m, int cap,
                                    int32_t* points, int32_t* counts, int32_t* iters, uint32_t* skel, ivosw_stream_t stream) {
    using namespace ivosw;
    IVOSW_REQUIRE(gt, "null gt");
    IVOSW_REQUIRE(units_host, "null units_host");
    IVOSW_REQUIRE(points, "null points");
    IVOSW_REQUIRE(counts, "null counts");
    IVOSW_REQUIRE(iters, "null iters");
    IVOSW_REQUIRE(n >= 1, "n < 1");
    IVOSW_REQUIRE(m >= 1, "m < 1");
    IVOSW_REQUIRE(cap >= 1, "cap < 1");
    IVOSW_REQUIRE(H >= 1 && H <= 65535, "H outside [1, 65535]");
    IVOSW_REQUIRE(W >= 1 && W <= 65535, "W outside [1, 65535]");
    const int WW = (W + 31) / 32;
    const size_t lds = 2 * (size_t)H * WW * sizeof(uint32_t) + ROBOT_LDS_FIXED;
    if (lds > ROBOT_LDS_LIMIT) {
        set_error("%s: H = %d, W = %d: two bit planes of H * ceil(W / 32) words and %zu fixed bytes are %zu bytes of LDS, the limit of one "
                  "workgroup is %zu (the robot serves 480p; see ivosw_robot_skeleton_fits)", __func__, H, W, ROBOT_LDS_FIXED, lds,
                  ROBOT_LDS_LIMIT);
        return IVOSW_ERR_ARG;
    }
    for (int k = 0; k < m; ++k) {
        const int f = units_host[2 * (long)k], o = units_host[2 * (long)k + 1];
        if (f < 0 || f >= n) {
            set_error("%s: units_host: unit %d: frame %d outside [0, %d)", __func__, k, f, n);
            return IVOSW_ERR_ARG;
        }
        if (o < 1 || o > 255) {
            set_error("%s: units_host: unit %d: object %d outside [1, 255]", __func__, k, o);
            return IVOSW_ERR_ARG;
        }
    }
    IVOSW_ON_DEVICE_OF(gt);
    static std::atomic<bool> attr_set[64];                                 // per device: the kernel may take more than the default 64 KB
    if (dscope__.dev >= 0 && dscope__.dev < 64 && !attr_set[dscope__.dev].load(std::memory_order_acquire)) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(robot_skeleton_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)ROBOT_LDS_LIMIT);
        (void)hipGetLastError();
        attr_set[dscope__.dev].store(true, std::memory_order_release);
    }
    hipStream_t st = as_stream(stream);
    const size_t N = (size_t)H * WW;
    for (int g0 = 0; g0 < m; g0 += ROBOT_GROUP) {
        const int cnt = m - g0 < ROBOT_GROUP ? m - g0 : ROBOT_GROUP;
        RobotArgs a{};
        a.gt = gt;
        a.pred = pred;
        a.points = points + (size_t)g0 * cap;
        a.counts = counts + g0;
        a.iters = iters + g0;
        a.skel = skel ? skel + (size_t)g0 * N : nullptr;
        a.H = H; a.W = W; a.WW = WW; a.cap = cap; a.max_iters = H > W ? H : W;
        for (int k = 0; k < cnt; ++k) {
            a.frame[k] = units_host[2 * (long)(g0 + k)];
            a.object[k] = (uint8_t)units_host[2 * (long)(g0 + k) + 1];
        }
        hipLaunchKernelGGL(robot_skeleton_kernel, dim3((unsigned)cnt), dim3(ROBOT_THREADS), lds, st, a);
        IVOSW_CHECK_LAUNCH();
    }
    return IVOSW_OK;
}
