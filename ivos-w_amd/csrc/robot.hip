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
//
// ivosw_robot_skeleton_box (further down): the same rule on planes of the error region's bounding box only - any frame size, object 0 -
// with the planes in LDS or, for a box beyond it, in a global workspace; bit-identical outputs.
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

// ================================================================================================ the boxed form: any frame size, object 0
// ivosw_robot_skeleton_box: the same rule on planes that cover ONLY the bounding box of the error region (rows by0 .. by1, 32-pixel words
// bw0 .. bw1).  Zhang-Suen only ever clears bits and reads everything outside the image as 0; every pixel outside the box is 0 from the
// start and stays 0, so a plane of the box alone, with "outside the window" read as 0, holds at every sub-iteration exactly the bits the
// full-frame plane holds inside the box: the same deletions in the same sub-iterations, the same iteration count, the same skeleton.
//   0  the box       one pass over the frame with phase A's loads (16-byte body, byte-wise ragged ends, the byte path for a frame whose gt
//                    and pred are on different 16-byte phases): min / max row and word of gt == o && pred != o in registers, a wave
//                    reduction, LDS min / max.  Nothing is stored.  An empty region ends here: counts = 0, iters = 0, skel all zero.
//   A  the window    one thread per window word: the 32 pixels of the word from aligned 4-byte loads of gt and pred (a dword that is not
//                    wholly inside the frame goes byte by byte), shifted into place, bits at x >= W masked; ONE plain store per word,
//                    zero words included, so the planes need no clearing pass and no atomics.
//   B  thinning      thin_word on window-relative coordinates with (bh, bw) as the bounds.
//   C  outputs       absolute coordinates: window raster order restricted to the box rows is frame raster order.
// Where the planes live is decided per workgroup, uniformly: 2 * bh * bw * 4 + 256 <= the launch's dynamic LDS -> LDS, else this unit's
// slice (2 * H * WW words) of a caller-owned global workspace.  robot_box_body<GLOBAL> is the one body of both.
//
// The global planes and the memory model.  A plane word is written by one thread and read, one sub-iteration later, by up to nine threads
// of the SAME workgroup, never by another workgroup (each unit has its own slice; a later launch on the stream starts after this one).
// Between a sub-iteration's stores and the next one's loads stands a __syncthreads(), which HIP defines as a workgroup-scope release
// fence, s_barrier, and a workgroup-scope acquire fence over global memory as over LDS.  The compiler turns the release into
// s_waitcnt vmcnt(0) in front of the barrier: every store of every wave has been acknowledged by L2 before any wave leaves the barrier.
// All waves of a workgroup run on one CU and share its vector L1, which is write-through and keeps no dirty line: a store updates L2 and
// leaves no stale copy in that L1, so a load issued behind the barrier returns the new word from L1 or L2.  Workgroup scope is exactly
// the scope of this exchange (it would NOT reach another CU, and nothing here asks it to), so there is no device-scope fence, no atomic on
// global memory, and the loads and stores are plain (no non-temporal or read-only hint: a hint could route a load past the L1 state
// the argument rests on).  The deletion flags, the box and the wave totals are in the 256 fixed bytes of LDS in both forms.
struct RobotBoxArgs {
    const uint8_t* gt;       // [n][H][W]
    const uint8_t* pred;     // [n][H][W] or nullptr (all background; no unit of object 0 then)
    int32_t* points;         // [units][cap]
    int32_t* counts;         // [units]
    int32_t* iters;          // [units]
    uint32_t* skel;          // [units][H][WW] or nullptr
    uint32_t* workspace;     // [units][2][H][WW] or nullptr (then every box fits `budget`)
    int H, W, WW, cap, max_iters, budget;                                 // budget: the launch's dynamic LDS bytes
    int frame[ROBOT_GROUP];
    uint8_t object[ROBOT_GROUP];
};

namespace {
// the aligned dword at byte offset `off` of a frame of HW bytes (frame + off is 4-byte aligned; off may reach 3 bytes in front of or behind
// the frame): bytes outside the frame read as 0 and are never touched
__device__ __forceinline__ uint32_t frame_dword(const uint8_t* frame, long off, long HW) {
    if (off >= 0 && off + 4 <= HW) return *reinterpret_cast<const uint32_t*>(frame + off);
    uint32_t v = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (off + j >= 0 && off + j < HW) v |= (uint32_t)frame[off + j] << (8 * j);
    return v;
}

// phases A, B and C on planes p0 / p1 of bh x bw words (LDS, or GLOBAL: the unit's workspace slice)
template <bool GLOBAL>
__device__ __forceinline__ void robot_box_body(const RobotBoxArgs& a, int u, uint32_t* p0, uint32_t* p1, int* fixed, const uint8_t* gt,
                                               const uint8_t* pr, uint32_t o, int by0, int bh, int bw0, int bw) {
    const int tid = threadIdx.x;
    const int H = a.H, W = a.W, WW = a.WW, N = H * WW, items = bh * bw;
    const long HW = (long)H * W;

    // ---- A: the window's words
    const int gsh = (int)((uintptr_t)gt & 3), psh = pr ? (int)((uintptr_t)pr & 3) : 0;
    for (int i = tid; i < items; i += ROBOT_THREADS) {
        const int yy = i / bw, wx = bw0 + (i - yy * bw);
        const long pix = (long)(by0 + yy) * W + 32 * wx;
        const int gs = (int)((gsh + pix) & 3), ps = (int)((psh + pix) & 3);
        const long goff = pix - gs, poff = pix - ps;
        uint32_t glo = frame_dword(gt, goff, HW), plo = pr ? frame_dword(pr, poff, HW) : 0u, bits = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint32_t ghi = gs || j < 7 ? frame_dword(gt, goff + 4 * (j + 1), HW) : 0u;
            const uint32_t phi = pr && (ps || j < 7) ? frame_dword(pr, poff + 4 * (j + 1), HW) : 0u;
            const uint32_t g4 = (uint32_t)((((uint64_t)ghi << 32) | glo) >> (8 * gs));
            const uint32_t p4 = (uint32_t)((((uint64_t)phi << 32) | plo) >> (8 * ps));
            bits |= err4(g4, p4, o) << (4 * j);
            glo = ghi;
            plo = phi;
        }
        const int valid = W - 32 * wx;                                    // bytes behind the row's end belong to the next row (or to nobody)
        if (valid < 32) bits &= (1u << valid) - 1u;
        p0[i] = bits;
    }
    __syncthreads();

    // ---- B: Zhang-Suen on the window (everything outside it is zero and stays zero)
    int iters = -1;
    for (int it = 0; it < a.max_iters; ++it) {
        uint32_t gone = 0;
        for (int i = tid; i < items; i += ROBOT_THREADS) {
            const int yy = i / bw, wx = i - yy * bw;
            const uint32_t c = p0[i];
            const uint32_t v = c ? thin_word(p0, yy, wx, bh, bw, 0, c) : 0u;
            p1[i] = v;
            gone |= c ^ v;
        }
        __syncthreads();
        for (int i = tid; i < items; i += ROBOT_THREADS) {
            const int yy = i / bw, wx = i - yy * bw;
            const uint32_t c = p1[i];
            const uint32_t v = c ? thin_word(p1, yy, wx, bh, bw, 1, c) : 0u;
            p0[i] = v;
            gone |= c ^ v;
        }
        int* flag = fixed + 8 + (it & 1);                                 // the two flags in turn, as in robot_skeleton_kernel
        if (gone) *flag = 1;
        __syncthreads();                                                  // (orders this iteration's plane stores, in LDS and in global memory)
        const int any = *flag;
        if (tid == 0) fixed[8 + ((it + 1) & 1)] = 0;
        if (!any) {
            iters = it;
            break;
        }
    }

    // ---- C: the outputs, from plane 0, in frame coordinates
    if (a.skel) {
        uint32_t* out = a.skel + (size_t)u * N;
        for (int i = tid; i < N; i += ROBOT_THREADS) {
            const int yy = i / WW - by0, wx = i % WW - bw0;
            out[i] = yy >= 0 && yy < bh && wx >= 0 && wx < bw ? p0[yy * bw + wx] : 0u;
        }
    }
    const int chunk = (items + ROBOT_THREADS - 1) / ROBOT_THREADS;
    const int i0 = min(tid * chunk, items), i1 = min(i0 + chunk, items);
    int mine = 0;
    for (int i = i0; i < i1; ++i) mine += __popc(p0[i]);
    int incl = mine;
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
        int yy = i0 / bw, wx = i0 - yy * bw;
        for (int i = i0; i < i1; ++i) {
            uint32_t bits = p0[i];
            while (bits) {
                const int b = __ffs((int)bits) - 1;
                bits &= bits - 1u;
                if (base < a.cap) pts[base] = ((by0 + yy) << 16) | ((bw0 + wx) * 32 + b);
                ++base;
            }
            if (++wx == bw) { wx = 0; ++yy; }
        }
    }
    if (tid == 0) {
        a.counts[u] = total;
        a.iters[u] = iters;
    }
}
}  // namespace

__global__ __launch_bounds__(ROBOT_THREADS) void robot_skeleton_box_kernel(RobotBoxArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t robot_box_lds[];
    const int tid = threadIdx.x, u = blockIdx.x;
    const int H = a.H, W = a.W, WW = a.WW;
    int* fixed = reinterpret_cast<int*>(robot_box_lds);                   // the 256 fixed bytes come FIRST here (the planes' size is not known yet); same slots
    const uint32_t o = a.object[u];
    const size_t HW = (size_t)H * W;
    const uint8_t* gt = a.gt + (size_t)a.frame[u] * HW;
    const uint8_t* pr = a.pred ? a.pred + (size_t)a.frame[u] * HW : nullptr;

    if (tid == 0) { fixed[0] = H; fixed[1] = -1; fixed[2] = WW; fixed[3] = -1; fixed[8] = 0; fixed[9] = 0; }
    __syncthreads();

    // ---- 0: the box of the error region, nothing stored
    int y0 = H, y1 = -1, w0 = WW, w1 = -1;
    const bool vec = !pr || (((uintptr_t)gt ^ (uintptr_t)pr) & 15) == 0;
    const size_t head = vec ? min((size_t)((16 - ((uintptr_t)gt & 15)) & 15), HW) : HW;
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
            const uint32_t run = m & ((1u << r) - 1u);
            if (run) {
                y0 = min(y0, y); y1 = max(y1, y);
                w0 = min(w0, (x + __ffs((int)run) - 1) >> 5); w1 = max(w1, (x + 31 - __clz((int)run)) >> 5);
            }
            m >>= r;
            left -= r;
            ++y;
            x = 0;
        }
    }
    for (size_t k = tid; k < head + (HW - tail0); k += ROBOT_THREADS) {   // the ragged ends (all of a frame off the common phase)
        const size_t pix = k < head ? k : tail0 + (k - head);
        if (gt[pix] == o && (!pr || pr[pix] != o)) {
            const int y = (int)(pix / (size_t)W), wx = (int)(pix - (size_t)y * W) >> 5;
            y0 = min(y0, y); y1 = max(y1, y); w0 = min(w0, wx); w1 = max(w1, wx);
        }
    }
    y0 = wave_min(y0); y1 = wave_max(y1); w0 = wave_min(w0); w1 = wave_max(w1);
    if ((tid & 63) == 0 && y1 >= 0) {
        atomicMin(&fixed[0], y0); atomicMax(&fixed[1], y1); atomicMin(&fixed[2], w0); atomicMax(&fixed[3], w1);
    }
    __syncthreads();
    const int by0 = fixed[0], bh = fixed[1] - by0 + 1, bw0 = fixed[2], bw = fixed[3] - bw0 + 1;
    if (bh <= 0) {                                                        // an empty region: what robot_skeleton_kernel yields for it
        if (a.skel) {
            uint32_t* out = a.skel + (size_t)u * H * WW;
            for (int i = tid; i < H * WW; i += ROBOT_THREADS) out[i] = 0u;
        }
        if (tid == 0) {
            a.counts[u] = 0;
            a.iters[u] = 0;
        }
        return;
    }
    const size_t items = (size_t)bh * bw;
    if (2 * items * sizeof(uint32_t) + ROBOT_LDS_FIXED <= (size_t)a.budget) {
        uint32_t* p0 = robot_box_lds + ROBOT_LDS_FIXED / sizeof(uint32_t);
        robot_box_body<false>(a, u, p0, p0 + items, fixed, gt, pr, o, by0, bh, bw0, bw);
    } else {                                                              // (the entry has made sure that there is a workspace then)
        uint32_t* p0 = a.workspace + (size_t)u * 2 * H * WW;
        robot_box_body<true>(a, u, p0, p0 + items, fixed, gt, pr, o, by0, bh, bw0, bw);
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

// ------------------------------------------------------------------------------------------------ the boxed entry
namespace ivosw {
namespace {
#define ROBOT_BOX_REQUIRE(cond, msg)                \
    do {                                            \
        if (!(cond)) {                              \
            set_error("%s: %s", who, msg);          \
            return IVOSW_ERR_ARG;                   \
        }                                           \
    } while (0)

// the one launcher of ivosw_robot_skeleton_box (budget 0: the product's, min(two full planes + 256, the limit)) and of the probe
int robot_box_launch(const char* who, const uint8_t* gt, const uint8_t* pred, int n, int H, int W, const int32_t* units_host, int m, int cap,
                     int32_t* points, int32_t* counts, int32_t* iters, uint32_t* skel, uint32_t* workspace, size_t workspace_bytes,
                     size_t budget, ivosw_stream_t stream) {
    ROBOT_BOX_REQUIRE(gt, "null gt");
    ROBOT_BOX_REQUIRE(units_host, "null units_host");
    ROBOT_BOX_REQUIRE(points, "null points");
    ROBOT_BOX_REQUIRE(counts, "null counts");
    ROBOT_BOX_REQUIRE(iters, "null iters");
    ROBOT_BOX_REQUIRE(n >= 1, "n < 1");
    ROBOT_BOX_REQUIRE(m >= 1, "m < 1");
    ROBOT_BOX_REQUIRE(cap >= 1, "cap < 1");
    ROBOT_BOX_REQUIRE(H >= 1 && H <= 65535, "H outside [1, 65535]");
    ROBOT_BOX_REQUIRE(W >= 1 && W <= 65535, "W outside [1, 65535]");
    const int WW = (W + 31) / 32;
    const size_t N = (size_t)H * WW, full = 2 * N * sizeof(uint32_t) + ROBOT_LDS_FIXED;
    if (budget == 0) budget = full < ROBOT_LDS_LIMIT ? full : ROBOT_LDS_LIMIT;
    for (int k = 0; k < m; ++k) {
        const int f = units_host[2 * (long)k], o = units_host[2 * (long)k + 1];
        if (f < 0 || f >= n) {
            set_error("%s: units_host: unit %d: frame %d outside [0, %d)", who, k, f, n);
            return IVOSW_ERR_ARG;
        }
        if (o < 0 || o > 255) {
            set_error("%s: units_host: unit %d: object %d outside [0, 255]", who, k, o);
            return IVOSW_ERR_ARG;
        }
        if (o == 0 && !pred) {
            set_error("%s: units_host: unit %d: object 0 (the background) with a null pred: a null pred is all background, so the background "
                      "has no false positive to draw on", who, k);
            return IVOSW_ERR_ARG;
        }
    }
    if (full > budget) {                                                   // a box may be the whole frame: the global planes must exist
        const size_t need = (size_t)m * 2 * N * sizeof(uint32_t);
        if (!workspace || workspace_bytes < need) {
            set_error("%s: H = %d, W = %d: two bit planes of H * ceil(W / 32) words and %zu fixed bytes are %zu bytes, more than the %zu bytes "
                      "of LDS of this launch: a box that large keeps its planes in the workspace, which needs %zu bytes for %d units "
                      "(ivosw_robot_box_workspace_bytes), got %s%zu", who, H, W, ROBOT_LDS_FIXED, full, budget, need, m,
                      workspace ? "" : "a null pointer of ", workspace_bytes);
            return IVOSW_ERR_ARG;
        }
    }
    IVOSW_ON_DEVICE_OF(gt);
    static std::atomic<bool> attr_set[64];                                 // per device: the kernel may take more than the default 64 KB
    if (dscope__.dev >= 0 && dscope__.dev < 64 && !attr_set[dscope__.dev].load(std::memory_order_acquire)) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(robot_skeleton_box_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)ROBOT_LDS_LIMIT);
        (void)hipGetLastError();
        attr_set[dscope__.dev].store(true, std::memory_order_release);
    }
    hipStream_t st = as_stream(stream);
    for (int g0 = 0; g0 < m; g0 += ROBOT_GROUP) {
        const int cnt = m - g0 < ROBOT_GROUP ? m - g0 : ROBOT_GROUP;
        RobotBoxArgs a{};
        a.gt = gt;
        a.pred = pred;
        a.points = points + (size_t)g0 * cap;
        a.counts = counts + g0;
        a.iters = iters + g0;
        a.skel = skel ? skel + (size_t)g0 * N : nullptr;
        a.workspace = full > budget ? workspace + (size_t)g0 * 2 * N : nullptr;
        a.H = H; a.W = W; a.WW = WW; a.cap = cap; a.max_iters = H > W ? H : W; a.budget = (int)budget;
        for (int k = 0; k < cnt; ++k) {
            a.frame[k] = units_host[2 * (long)(g0 + k)];
            a.object[k] = (uint8_t)units_host[2 * (long)(g0 + k) + 1];
        }
        hipLaunchKernelGGL(robot_skeleton_box_kernel, dim3((unsigned)cnt), dim3(ROBOT_THREADS), budget, st, a);
        if (hipGetLastError() != hipSuccess) {
            set_error("%s: the launch of robot_skeleton_box_kernel failed", who);
            return IVOSW_ERR_LAUNCH;
        }
    }
    return IVOSW_OK;
}
#undef ROBOT_BOX_REQUIRE
}  // namespace
}  // namespace ivosw

extern "C" long ivosw_robot_box_workspace_bytes(int H, int W, int m) {
    using namespace ivosw;
    if (H < 1 || W < 1 || H > 65535 || W > 65535 || m < 1) return -1;
    if (ivosw_robot_skeleton_fits(H, W)) return 0;
    return (long)m * 2 * (long)H * (long)((W + 31) / 32) * (long)sizeof(uint32_t);
}

extern "C" int ivosw_robot_skeleton_box(const uint8_t* gt, const uint8_t* pred, int n, int H, int W, const int32_t* units_host, int m, int cap,
                                        int32_t* points, int32_t* counts, int32_t* iters, uint32_t* skel, uint32_t* workspace,
                                        size_t workspace_bytes, ivosw_stream_t stream) {
    return ivosw::robot_box_launch(__func__, gt, pred, n, H, W, units_host, m, cap, points, counts, iters, skel, workspace, workspace_bytes, 0,
                                   stream);
}

#ifdef IVOSW_PROBES
extern "C" int ivosw_robot_box_probe(const uint8_t* gt, const uint8_t* pred, int n, int H, int W, const int32_t* units_host, int m, int cap,
                                     int32_t* points, int32_t* counts, int32_t* iters, uint32_t* skel, uint32_t* workspace,
                                     size_t workspace_bytes, int lds_budget_bytes, ivosw_stream_t stream) {
    using namespace ivosw;
    if (lds_budget_bytes < (int)ROBOT_LDS_FIXED || (size_t)lds_budget_bytes > ROBOT_LDS_LIMIT) {
        set_error("%s: lds_budget_bytes %d outside [%zu, %zu]", __func__, lds_budget_bytes, ROBOT_LDS_FIXED, ROBOT_LDS_LIMIT);
        return IVOSW_ERR_ARG;
    }
    return robot_box_launch(__func__, gt, pred, n, H, W, units_host, m, cap, points, counts, iters, skel, workspace, workspace_bytes,
                            (size_t)lds_budget_bytes, stream);
}
#endif  // IVOSW_PROBES
