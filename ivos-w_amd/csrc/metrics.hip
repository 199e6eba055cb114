// DAVIS region similarity J (Jaccard) and contour accuracy F (boundary F-measure) on the device — SURVEY §8(f) row 3,
// the step right before the hot path in every interaction loop (oracle state, rewards, J&F logging).
//
// Reference call site: utils/misc.py:118-162 (sequence_metric) -> davisinteractive.metrics.batched_jaccard /
// batched_f_measure (davisinteractive==1.0.4, requirements.txt:14; the package is NOT under /root/reference, so the
// algorithm below follows its published definition — the DAVIS evaluation code — and parity is unpinned, see
// oracle/jf_oracle.py).  Per frame and object id:
//   J: |gt & pred| / |gt | pred|, 1 when the union is empty
//   F: boundary maps b = (seg ^ east) | (seg ^ south) | (seg ^ south-east) with the last row / column special-cased;
//      each boundary is dilated by a disk of radius bound_pix = ceil(0.008 * |(H, W)|) (8 at 480p); precision = matched
//      pred-boundary pixels / pred-boundary pixels, recall likewise for gt; F = 2PR / (P + R)
//
// This is integer / bit work bound by HBM (two label maps in) and latency: the kernels produce the six INTEGER counts per
// (frame, object); the float64 ratios are formed on the host with the reference's own expressions, so results are
// bit-identical whenever the counts are.
//   jf_boundary_row_kernel  one lane = 16 pixels of a row (16-byte loads contiguous across the wave), four rows per wave:
//                       object masks by a SWAR byte compare -> boundary words (bit-packed, ws) + intersection / union /
//                       boundary-pixel counts (DPP wave reduction, one atomic per counter and block)
//   jf_match_kernel     one thread = one boundary word of map A: skipped when empty (boundaries are sparse), otherwise
//                       ORs the (2r+1) row-smears of map B around it (disk = per-row half widths) and counts A & dil(B)
// Several sessions (ivosw_jf_counts_videos, ivosw_jf_reduce_ragged; the oracle chain of utils_agent.oracle_recommend): the same two
// bodies over a table of per-video descriptors in the kernel arguments (jf_*_videos_kernel), and
//   jf_reduce_ragged_kernel  one thread = one frame: the host's float64 ratio expressions and numpy's row mean on the device, so the
//                       counts no longer travel to the host between the J / F pass and the Brain
#include "common.h"
#include <stdlib.h>

namespace ivosw {

namespace {
constexpr int JF_MAX_OBJ = 32;
constexpr int JF_MAX_R = 32;

struct JfArgs {
    const uint8_t* gt;
    const uint8_t* pred;
    int N, H, W, WW;              // WW = words per bitmap row
    int n_obj;
    uint8_t ids[JF_MAX_OBJ];
    int r;
    uint8_t hw[JF_MAX_R + 1];     // half width of the disk at |dy|: floor(sqrt(r^2 - dy^2))
    uint32_t* bg;                 // gt boundary bitmaps   [n_obj][N][H][WW]
    uint32_t* bp;                 // pred boundary bitmaps
    unsigned long long* counts;   // [N][n_obj][6]: inter, union, n_fg (pred boundary), n_gt, fg_match, gt_match
};

// One video of ivosw_jf_counts_videos as the kernels see it, and the table that travels in their arguments (32 x 88 + 2 x 132 + 32
// bytes = 3112 of the 4 KB budget).  The field names are JfArgs's, so one body serves both.
struct JfVideo {
    const uint8_t* gt;
    const uint8_t* pred;
    int N, H, W, WW, n_obj, r;
    uint8_t ids[JF_MAX_OBJ];
    unsigned long long bm_off;        // words from the workspace base to the video's gt bitmaps; its pred bitmaps follow plane_words later
    unsigned long long plane_words;
    unsigned long long cnt_off;       // elements from counts to the video's [N][n_obj][6] block
};
struct JfTable {
    JfVideo v[IVOSW_MAX_JF_VIDEOS];
    int frame_off[IVOSW_MAX_JF_VIDEOS + 1];     // video k owns the flat frames [frame_off[k], frame_off[k + 1])
    int fo_off[IVOSW_MAX_JF_VIDEOS + 1];        // ... and the flat (frame, object) pairs [fo_off[k], fo_off[k + 1])
    int n_videos;
    uint32_t* bitmaps;
    unsigned long long* counts;
};
static_assert(sizeof(JfTable) <= 3584, "the table must fit the kernel-argument budget (4 KB) with room to spare");

}  // namespace

// Boundary kernel: a wave owns one row segment of up to 1024 pixels, lane l the 16 pixels [16 l, 16 l + 16) — the label
// loads of a lane are 16-byte loads that are CONTIGUOUS across the wave (every byte used once).  East / south-east
// neighbours come from the next lane; a lane pair forms one bitmap word.  History (100 frames x 3 objects at 480p):
// one thread per 32-pixel word with 36-byte windows at a 32-byte lane stride 111 us -> this layout 94 us (the loads were
// never the limit: the kernel is VALU-bound) -> two counters per 32-bit word through the reduction 57 us -> DPP instead
// of ds_bpermute shuffles 53 us -> four rows per wave with the south row's masks reused 47 us.
//
// DPP cross-lane moves (one VALU instruction each; __shfl_down is a ds_bpermute plus address arithmetic, and this kernel
// is VALU-bound).  wave_shl:1 = every lane reads lane + 1 (0 past the end); the reduction is the row_shr 1/2/4/8 scan
// followed by row_bcast15 / row_bcast31, total in lane 63.
__device__ __forceinline__ uint32_t lane_next(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x130, 0xf, 0xf, true);
}
__device__ __forceinline__ uint32_t wave_total_in_lane63(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);   // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);   // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true);   // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true);   // row_shr:8 -> lane 15 of each row holds the row sum
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);  // row_bcast15 into rows 1, 3
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);  // row_bcast31 into rows 2, 3
    return v;
}

__device__ __forceinline__ uint32_t mask16(const uint32_t (&w)[4], uint32_t id4) {
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t v = w[k] ^ id4;
        const uint32_t t = ~((((v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | v) | 0x7F7F7F7Fu);    // 0x80 in every zero byte of v
        m |= ((((t >> 7) * 0x00204081u) >> 21) & 0xFu) << (4 * k);
    }
    return m;
}

// The byte-plane source's mask: bit k = (byte k of w >= the byte repeated in thr4), by a SWAR unsigned compare.  Per byte, with x7 / t7
// the low seven bits: d = (x7 + 128) - t7 stays inside the byte (1 .. 255, no borrow crosses), and its bit 7 says x7 >= t7; where the
// top bits of x and t differ the top bit of x decides, where they agree bit 7 of d does.
__device__ __forceinline__ uint32_t ge16(const uint32_t (&w)[4], uint32_t thr4) {
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t x = w[k];
        const uint32_t d = (x | 0x80808080u) - (thr4 & 0x7F7F7F7Fu);
        const uint32_t t = ((x & ~thr4) | (~(x ^ thr4) & d)) & 0x80808080u;            // 0x80 in every byte of x that is >= its threshold
        m |= ((((t >> 7) * 0x00204081u) >> 21) & 0xFu) << (4 * k);
    }
    return m;
}

__device__ __forceinline__ void load16(const uint8_t* base, size_t off, size_t total, bool on, uint32_t (&w)[4]) {
    w[0] = w[1] = w[2] = w[3] = 0u;
    if (!on) return;
    if (off + 16 <= total) {
        __builtin_memcpy(w, base + off, 16);          // bytes past the row end belong to the next row: masked by the caller
    } else {
        for (int k = 0; k < 16; ++k)
            if (off + k < total) w[k >> 2] |= (uint32_t)base[off + k] << (8 * (k & 3));
    }
}

// A wave walks JF_RPW consecutive rows: the south row of one step is the own row of the next, so JF_RPW + 1 row loads and
// mask computations serve JF_RPW rows, and the counts are reduced once per object and wave (the kernel is VALU-bound).
constexpr int JF_RPW = 4;
// The body serves both descriptor sources: `a` is the single video's JfArgs (ivosw_jf_counts) or one JfVideo of the table
// (ivosw_jf_counts_videos) - the same field names; bgm / bpm / counts are that video's bitmaps and count block, n its frame.
//
// The prediction source is a compile-time parameter.  JF_PRED_LABELS: a.pred is a label map [N][H][W] like a.gt, loaded once in front of
// the object loop, the mask of object o is pred == ids[o].  JF_PRED_PLANES (ivosw_qa_counts_videos): a.pred is a stack of byte planes
// [n_obj][N][H][W], the mask of object o is planes[o] >= thr - the planes of two objects may overlap, which no label map can express -
// so the 16 bytes are loaded INSIDE the object loop and compared by ge16 in the place of mask16.  Everything behind the masks is shared.
constexpr int JF_PRED_LABELS = 0, JF_PRED_PLANES = 1;
template <int SRC, class A>
__device__ __forceinline__ void jf_boundary_body(const A& a, uint32_t* __restrict__ bgm, uint32_t* __restrict__ bpm,
                                                 unsigned long long* __restrict__ counts, int n, int seg, int yblk, uint32_t thr) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int y0 = (yblk * 4 + wave) * JF_RPW;
    const int x0 = seg * 1024 + lane * 16;
    const bool col_live = x0 < a.W;
    const size_t total = (size_t)a.N * a.H * a.W;
    uint32_t g[JF_RPW + 1][4], p[JF_RPW + 1][4];
    uint8_t tg[JF_RPW + 1], tp[JF_RPW + 1];          // the pixel right of this lane's 16 at the end of a 1024-pixel segment
    const bool tail = (lane == 63) && col_live && x0 + 16 < a.W;
#pragma unroll
    for (int r = 0; r <= JF_RPW; ++r) {
        const int y = y0 + r;
        const bool on = col_live && y < a.H;
        const size_t off = ((size_t)n * a.H + (y < a.H ? y : 0)) * a.W + x0;
        load16(a.gt, off, total, on, g[r]);
        if constexpr (SRC == JF_PRED_LABELS) load16(a.pred, off, total, on, p[r]);
        tg[r] = (tail && on) ? a.gt[off + 16] : 0;
        if constexpr (SRC == JF_PRED_LABELS) tp[r] = (tail && on) ? a.pred[off + 16] : 0;
    }
    const int nvalid = col_live ? min(16, a.W - x0) : 0;
    const uint32_t vm = (1u << nvalid) - 1u;
    const int lastbit = a.W - 1 - x0;
    const uint32_t lastcol = (lastbit >= 0 && lastbit < 16) ? (1u << lastbit) : 0u;
    __shared__ unsigned long long red[4][4];
    for (int o = 0; o < a.n_obj; ++o) {
        const uint8_t id = a.ids[o];
        const uint32_t id4 = id * 0x01010101u;
        if constexpr (SRC == JF_PRED_PLANES) {
            const size_t plane0 = ((size_t)o * a.N + n) * a.H;               // this object's plane of frame n, in rows from a.pred
#pragma unroll
            for (int r = 0; r <= JF_RPW; ++r) {
                const int y = y0 + r;
                const bool on = col_live && y < a.H;
                const size_t off = (plane0 + (y < a.H ? y : 0)) * a.W + x0;
                load16(a.pred, off, total * a.n_obj, on, p[r]);
                tp[r] = (tail && on) ? a.pred[off + 16] : 0;
            }
        }
        // bits 0..15 = this lane's pixels, bit 16 = the east neighbour of pixel 15 (rows >= H load zeros: no match for id > 0,
        // and the valid mask clears id == 0 matches of rows that do not exist through `rows` below)
        uint32_t mg[JF_RPW + 1], mp[JF_RPW + 1];
#pragma unroll
        for (int r = 0; r <= JF_RPW; ++r) {
            const bool row_ok = y0 + r < a.H;
            const uint32_t m0 = row_ok ? (mask16(g[r], id4) & vm) : 0u;
            const uint32_t m1 = row_ok ? ((SRC == JF_PRED_PLANES ? ge16(p[r], thr * 0x01010101u) : mask16(p[r], id4)) & vm) : 0u;
            // the shuffle runs in EVERY lane, outside the lane-63 select: inside its `lane != 63` arm lane 63 is switched off, and a DPP
            // read of a switched-off lane returns 0 - lane 62 then lost the east neighbour of its last pixel (column 1007 | 1008 of a segment)
            const uint32_t n0 = lane_next(m0) & 1u, n1 = lane_next(m1) & 1u;
            const uint32_t e0 = lane == 63 ? ((tail && row_ok && tg[r] == id) ? 1u : 0u) : n0;
            const uint32_t e1 = lane == 63 ? ((tail && row_ok && (SRC == JF_PRED_PLANES ? tp[r] >= thr : tp[r] == id)) ? 1u : 0u) : n1;
            mg[r] = m0 | (e0 << 16);
            mp[r] = m1 | (e1 << 16);
        }
        uint32_t c01 = 0, c23 = 0;
#pragma unroll
        for (int r = 0; r < JF_RPW; ++r) {
            const int y = y0 + r;
            const bool lastrow = (y == a.H - 1);
            auto bmap = [&](uint32_t m0, uint32_t m1) {
                const uint32_t seg16 = m0 & 0xffffu, e = (m0 >> 1) & 0xffffu, s = m1 & 0xffffu, se = (m1 >> 1) & 0xffffu;
                uint32_t b;
                if (lastrow) b = (seg16 ^ e) & ~lastcol;                                   // b[-1, :] = seg ^ e ; b[-1, -1] = 0
                else b = (((seg16 ^ e) | (seg16 ^ s) | (seg16 ^ se)) & ~lastcol) | ((seg16 ^ s) & lastcol);   // b[:, -1] = seg ^ s
                return b & vm;
            };
            const bool row_ok = y < a.H;
            const uint32_t bgw = row_ok ? bmap(mg[r], mg[r + 1]) : 0u, bpw = row_ok ? bmap(mp[r], mp[r + 1]) : 0u;
            // lanes 2k, 2k+1 -> bitmap word k of the segment
            const uint32_t hg = lane_next(bgw), hp = lane_next(bpw);
            if (row_ok && col_live && !(lane & 1)) {
                const size_t widx = (((size_t)o * a.N + n) * a.H + y) * a.WW + (x0 >> 5);
                bgm[widx] = bgw | (hg << 16);
                bpm[widx] = bpw | (hp << 16);
            }
            const uint32_t sg = mg[r] & 0xffffu, sp = mp[r] & 0xffffu;
            // each count is <= 16 per lane and row, <= 4096 per wave: two counters share one 32-bit word through the reduction
            c01 += __popc(sg & sp) | (__popc(sg | sp) << 16);
            c23 += __popc(bpw) | (__popc(bgw) << 16);
        }
        c01 = wave_total_in_lane63(c01);
        c23 = wave_total_in_lane63(c23);
        if (lane == 63) { red[wave][0] = c01 & 0xffffu; red[wave][1] = c01 >> 16; red[wave][2] = c23 & 0xffffu; red[wave][3] = c23 >> 16; }
        __syncthreads();
        if (threadIdx.x < 4) {
            const unsigned long long v = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
            if (v) atomicAdd(counts + ((size_t)n * a.n_obj + o) * 6 + threadIdx.x, v);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void jf_boundary_row_kernel(JfArgs a) {
    jf_boundary_body<JF_PRED_LABELS>(a, a.bg, a.bp, a.counts, blockIdx.z, blockIdx.y, blockIdx.x, 0u);
}

// Several videos in one launch (ivosw_jf_counts_videos): grid.z runs flat over the frames of all videos, grid.x / grid.y are sized by
// the tallest / widest video.  A block finds its video in the prefix table and returns, before it forms any address, when it lies beyond
// that video's own rows or columns (block-uniform: no barrier is skipped by part of a block).
__device__ __forceinline__ int jf_find_video(const int* off, int n_videos, int i) {
    int lo = 0, hi = n_videos - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= i) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(256) void jf_boundary_row_videos_kernel(JfTable t) {
    const int v = jf_find_video(t.frame_off, t.n_videos, blockIdx.z);
    const JfVideo& a = t.v[v];
    if ((int)blockIdx.x * (4 * JF_RPW) >= a.H || (int)blockIdx.y * 1024 >= a.W) return;
    uint32_t* bgm = t.bitmaps + a.bm_off;
    jf_boundary_body<JF_PRED_LABELS>(a, bgm, bgm + a.plane_words, t.counts + a.cnt_off, (int)blockIdx.z - t.frame_off[v], blockIdx.y,
                                     blockIdx.x, 0u);
}

// The same launch shape with the prediction read from byte planes (ivosw_qa_counts_videos): JfVideo::pred is the video's
// [n_obj][N][H][W] plane stack; the per-video thresholds travel beside the table (JfTable itself keeps its size for the label kernels).
struct JfThresholds {
    uint8_t thr[IVOSW_MAX_JF_VIDEOS];
};
__global__ __launch_bounds__(256) void jf_boundary_row_planes_videos_kernel(JfTable t, JfThresholds th) {
    const int v = jf_find_video(t.frame_off, t.n_videos, blockIdx.z);
    const JfVideo& a = t.v[v];
    if ((int)blockIdx.x * (4 * JF_RPW) >= a.H || (int)blockIdx.y * 1024 >= a.W) return;
    uint32_t* bgm = t.bitmaps + a.bm_off;
    jf_boundary_body<JF_PRED_PLANES>(a, bgm, bgm + a.plane_words, t.counts + a.cnt_off, (int)blockIdx.z - t.frame_off[v], blockIdx.y,
                                     blockIdx.x, (uint32_t)th.thr[v]);
}

// grid (blocks over H*WW, N * n_obj, 2): z = 0 counts pred-boundary pixels inside dil(gt boundary) (fg_match),
// z = 1 gt-boundary pixels inside dil(pred boundary) (gt_match)
// `hw(d)`: the disk's half width at |dy| = d - the table in the single video's arguments, or the one a block of the multi-video
// kernel derives from bound_pix.  on = o * N + n inside the video, z = 0 / 1 as above.
template <class A, class HW>
__device__ __forceinline__ void jf_match_body(const A& a, const uint32_t* __restrict__ bgm, const uint32_t* __restrict__ bpm,
                                              unsigned long long* __restrict__ counts, HW hw, int on, int xblk, int z) {
    const int o = on / a.N, n = on - o * a.N;
    const int item = xblk * 256 + threadIdx.x;
    const int y = item / a.WW, j = item - y * a.WW;
    const uint32_t* own = (z == 0 ? bpm : bgm) + (size_t)on * a.H * a.WW;
    const uint32_t* oth = (z == 0 ? bgm : bpm) + (size_t)on * a.H * a.WW;
    unsigned long long c = 0;
    if (y < a.H) {
        const uint32_t mine = own[(size_t)y * a.WW + j];
        if (mine) {
            uint32_t dil = 0;
            // rows in groups of 8: the 24 loads of a group are issued together (one dependent L2 round trip per group instead
            // of one per row)
            for (int d0 = -a.r; d0 <= a.r; d0 += 8) {
                uint32_t cu[8], pv[8], nx[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const int dy = d0 + k, yy = y + dy;
                    const bool ok = dy <= a.r && yy >= 0 && yy < a.H;
                    const uint32_t* row = oth + (size_t)(ok ? yy : y) * a.WW;
                    cu[k] = ok ? row[j] : 0u;
                    pv[k] = (ok && j > 0) ? row[j - 1] : 0u;
                    nx[k] = (ok && j + 1 < a.WW) ? row[j + 1] : 0u;
                }
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    if (!(cu[k] | pv[k] | nx[k])) continue;
                    const int dy = d0 + k;
                    const int w = hw(dy < 0 ? -dy : dy);
                    // a set bit at x covers x-w .. x+w: smear towards higher x inside [prev | cur], towards lower x inside [cur | next]
                    uint64_t sl = (uint64_t)pv[k] | ((uint64_t)cu[k] << 32), sr = (uint64_t)cu[k] | ((uint64_t)nx[k] << 32);
                    for (int covered = 0; covered < w;) {
                        const int sh = min(covered + 1, w - covered);
                        sl |= sl << sh;
                        sr |= sr >> sh;
                        covered += sh;
                    }
                    dil |= (uint32_t)(sl >> 32) | (uint32_t)sr;
                }
            }
            c = __popc(mine & dil);
        }
    }
    // boundaries are sparse: most waves have nothing to add and skip the reduction; a word contributes <= 32
    if (__ballot(c != 0) != 0ull) {
        const uint32_t t = wave_total_in_lane63((uint32_t)c);
        if ((threadIdx.x & 63) == 63 && t) atomicAdd(counts + ((size_t)n * a.n_obj + o) * 6 + 4 + z, (unsigned long long)t);
    }
}

__global__ __launch_bounds__(256) void jf_match_kernel(JfArgs a) {
    jf_match_body(a, a.bg, a.bp, a.counts, [&](int d) { return (int)a.hw[d]; }, blockIdx.y, blockIdx.x, blockIdx.z);
}

// grid (blocks over the largest H * WW, all (frame, object) pairs of all videos, 2).  The disk's half widths are not carried per video
// (33 bytes x 32 videos would not fit the argument budget): the first r + 1 threads of a block derive them from bound_pix.
__global__ __launch_bounds__(256) void jf_match_videos_kernel(JfTable t) {
    const int v = jf_find_video(t.fo_off, t.n_videos, blockIdx.y);
    const JfVideo& a = t.v[v];
    if ((long long)blockIdx.x * 256 >= (long long)a.H * a.WW) return;
    __shared__ uint8_t hw_s[JF_MAX_R + 1];
    if ((int)threadIdx.x <= a.r) {
        const int d = threadIdx.x;
        int w = 0;
        while ((w + 1) * (w + 1) + d * d <= a.r * a.r) ++w;
        hw_s[d] = (uint8_t)w;
    }
    __syncthreads();
    const uint32_t* bgm = t.bitmaps + a.bm_off;
    jf_match_body(a, bgm, bgm + a.plane_words, t.counts + a.cnt_off, [&](int d) { return (int)hw_s[d]; }, (int)blockIdx.y - t.fo_off[v],
                  blockIdx.x, blockIdx.z);
}

}  // namespace ivosw

extern "C" size_t ivosw_jf_ws_bytes(int N, int H, int W, int n_obj) {
    if (N <= 0 || H <= 0 || W <= 0 || n_obj <= 0) return 0;
    const size_t ww = (size_t)(W + 31) / 32;
    return 2 * ivosw::align_up((size_t)n_obj * N * H * ww * sizeof(uint32_t), 256);
}

extern "C" int ivosw_jf_counts(const uint8_t* gt, const uint8_t* pred, int N, int H, int W, const uint8_t* obj_ids,
                               int n_obj, int bound_pix, int64_t* counts, void* ws, size_t ws_bytes,
                               ivosw_stream_t stream) {
    using namespace ivosw;
    IVOSW_REQUIRE(gt && pred && obj_ids && counts && ws, "null pointer");
    IVOSW_ON_DEVICE_OF(counts);
    IVOSW_REQUIRE(N > 0 && H > 0 && W > 0, "N, H, W must be positive");
    IVOSW_REQUIRE(n_obj > 0 && n_obj <= JF_MAX_OBJ, "1..32 object ids");
    IVOSW_REQUIRE((long)N * n_obj <= 65535, "N * n_obj must fit one grid dimension (65535): split the sequence");
    IVOSW_REQUIRE(W <= 65535 * 16, "image too wide");
    IVOSW_REQUIRE(bound_pix >= 0 && bound_pix <= JF_MAX_R, "boundary tolerance 0..32 pixels");
    if (ws_bytes < ivosw_jf_ws_bytes(N, H, W, n_obj)) {
        set_error("ivosw_jf_counts: workspace %zu < %zu", ws_bytes, ivosw_jf_ws_bytes(N, H, W, n_obj));
        return IVOSW_ERR_WS;
    }
    hipStream_t st = as_stream(stream);
    JfArgs a{};
    a.gt = gt; a.pred = pred; a.N = N; a.H = H; a.W = W; a.WW = (W + 31) / 32; a.n_obj = n_obj; a.r = bound_pix;
    for (int o = 0; o < n_obj; ++o) a.ids[o] = obj_ids[o];
    for (int d = 0; d <= bound_pix; ++d) {        // skimage.morphology.disk(r): x^2 + y^2 <= r^2 (integer arithmetic)
        int w = 0;
        while ((w + 1) * (w + 1) + d * d <= bound_pix * bound_pix) ++w;
        a.hw[d] = (uint8_t)w;
    }
    Arena ar(ws);
    a.bg = ar.take<uint32_t>((size_t)n_obj * N * H * a.WW);
    a.bp = ar.take<uint32_t>((size_t)n_obj * N * H * a.WW);
    a.counts = reinterpret_cast<unsigned long long*>(counts);
    (void)hipMemsetAsync(counts, 0, (size_t)N * n_obj * 6 * sizeof(int64_t), st);
    const unsigned nblk = (unsigned)(((size_t)H * a.WW + 255) / 256);
    hipLaunchKernelGGL(jf_boundary_row_kernel, dim3((H + 4 * JF_RPW - 1) / (4 * JF_RPW), (W + 1023) / 1024, N), dim3(256), 0, st, a);
    hipLaunchKernelGGL(jf_match_kernel, dim3(nblk, N * n_obj, 2), dim3(256), 0, st, a);
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}

// ------------------------------------------------------------------------------------------------ several videos in one pass
namespace ivosw {
namespace {

// Host-side check of a descriptor array (the caller has checked the pointer and names itself): fills the table (nullable) and the
// totals, or returns IVOSW_ERR_ARG with the message set.  Nothing is launched before it has passed.
int jf_videos_table(const char* who, const ivosw_jf_video_t* videos, int n_videos, JfTable* t, size_t* ws_bytes, size_t* n_counts,
                    int* max_h, int* max_w, long long* max_words) {
    if (n_videos < 1 || n_videos > IVOSW_MAX_JF_VIDEOS) {
        set_error("%s: n_videos %d outside [1, %d]", who, n_videos, IVOSW_MAX_JF_VIDEOS);
        return IVOSW_ERR_ARG;
    }
    size_t bytes = 0, cnt = 0;
    long long frames = 0, pairs = 0, words = 0;
    int mh = 0, mw = 0;
    for (int k = 0; k < n_videos; ++k) {
        const ivosw_jf_video_t& d = videos[k];
        const char* why = nullptr;
        if (!d.gt || !d.pred) why = "a NULL label map";
        else if (d.n_frames < 1 || d.H < 1 || d.W < 1) why = "n_frames, H and W must be positive";
        else if (d.n_obj < 1 || d.n_obj > JF_MAX_OBJ) why = "1..32 object ids";
        else if (d.bound_pix < 0 || d.bound_pix > JF_MAX_R) why = "boundary tolerance 0..32 pixels";
        else if ((long long)d.H * ((d.W + 31) / 32) > (1LL << 30)) why = "H * W too large";
        if (why) {
            set_error("%s: video %d: %s", who, k, why);
            return IVOSW_ERR_ARG;
        }
        const int ww = (d.W + 31) / 32;
        const size_t plane = align_up((size_t)d.n_obj * d.n_frames * d.H * ww * sizeof(uint32_t), 256);
        if (t) {
            JfVideo& v = t->v[k];
            v.gt = d.gt; v.pred = d.pred; v.N = d.n_frames; v.H = d.H; v.W = d.W; v.WW = ww; v.n_obj = d.n_obj; v.r = d.bound_pix;
            memcpy(v.ids, d.obj_ids, JF_MAX_OBJ);
            v.bm_off = bytes / sizeof(uint32_t);
            v.plane_words = plane / sizeof(uint32_t);
            v.cnt_off = cnt;
            t->frame_off[k] = (int)frames;
            t->fo_off[k] = (int)pairs;
        }
        bytes += 2 * plane;
        cnt += (size_t)d.n_frames * d.n_obj * 6;
        frames += d.n_frames;
        pairs += (long long)d.n_frames * d.n_obj;
        if (frames > 65535) {
            set_error("%s: video %d: more than 65535 frames in total (the boundary kernel's flat grid dimension): split the group", who, k);
            return IVOSW_ERR_ARG;
        }
        if (pairs > 65535) {
            set_error("%s: video %d: more than 65535 (frame, object) pairs in total (the match kernel's flat grid dimension): split the group",
                      who, k);
            return IVOSW_ERR_ARG;
        }
        mh = d.H > mh ? d.H : mh;
        mw = d.W > mw ? d.W : mw;
        words = (long long)d.H * ww > words ? (long long)d.H * ww : words;
    }
    if (t) {
        for (int k = n_videos; k <= IVOSW_MAX_JF_VIDEOS; ++k) {
            t->frame_off[k] = (int)frames;
            t->fo_off[k] = (int)pairs;
        }
        for (int k = n_videos; k < IVOSW_MAX_JF_VIDEOS; ++k) t->v[k] = JfVideo{};
        t->n_videos = n_videos;
    }
    if (ws_bytes) *ws_bytes = bytes;
    if (n_counts) *n_counts = cnt;
    if (max_h) *max_h = mh;
    if (max_w) *max_w = mw;
    if (max_words) *max_words = words;
    return IVOSW_OK;
}

// J and F of one (frame, object) from its six counts, with the expressions of ivos_w_amd/metrics.py (_jaccard_from, _f_from) in float64.
// Contraction is off in everything below: every product, sum and quotient is rounded by itself, as on the host.
#pragma clang fp contract(off)
__device__ __forceinline__ double jf_jaccard(const long long* c) {
    return c[1] == 0 ? 1.0 : (double)c[0] / (double)c[1];         // np.isclose(union, 0) on an integer count: union == 0
}
__device__ __forceinline__ double jf_fmeasure(const long long* c) {
    const long long n_fg = c[2], n_gt = c[3];
    double precision, recall;
    if (n_fg == 0 && n_gt > 0) { precision = 1.0; recall = 0.0; }
    else if (n_fg > 0 && n_gt == 0) { precision = 0.0; recall = 1.0; }
    else if (n_fg == 0 && n_gt == 0) { precision = 1.0; recall = 1.0; }
    else { precision = (double)c[4] / (double)n_fg; recall = (double)c[5] / (double)n_gt; }
    const double s = precision + recall;
    if (s == 0.0) return 0.0;
    const double twice = 2.0 * precision;
    const double prod = twice * recall;
    return prod / s;
}
// ndarray.mean(axis=1) of a C-contiguous float64 row: numpy's pairwise add.reduce (sequential below 8 elements, else 8 interleaved
// partial sums combined pairwise plus a sequential tail; rows are at most 32 long, below its 128-element block) and ONE division by n.
__device__ __forceinline__ double jf_row_mean(const double* v, int n) {
    double sum;
    if (n < 8) {
        sum = v[0];
        for (int o = 1; o < n; ++o) sum = sum + v[o];
    } else {
        double r[8];
        for (int j = 0; j < 8; ++j) r[j] = v[j];
        int i = 8;
        for (; i + 8 <= n; i += 8)
            for (int j = 0; j < 8; ++j) r[j] = r[j] + v[i + j];
        sum = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) sum = sum + v[i];
    }
    return sum / (double)n;
}

struct JfReduceTable {
    SeqTable seq;
    uint8_t n_obj[IVOSW_MAX_SEQS];
    long long pair_off[IVOSW_MAX_SEQS];       // (frame, object) pairs in front of video k
};

// One thread per flat row (frame): the row's video from the table, its n_obj count sextets -> J / F per object -> the row mean(s).
__global__ __launch_bounds__(64) void jf_reduce_ragged_kernel(const long long* __restrict__ counts, JfReduceTable tab, int n_seqs, int rows,
                                                              int metric, const float* __restrict__ annot, double* __restrict__ per_obj,
                                                              double* __restrict__ quality, float* __restrict__ state) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= rows) return;
    int lo = 0, hi = n_seqs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab.seq.row_off[mid] <= f) lo = mid;
        else hi = mid - 1;
    }
    const int O = tab.n_obj[lo];
    const long long pair0 = tab.pair_off[lo] + (long long)(f - tab.seq.row_off[lo]) * O;
    double vj[JF_MAX_OBJ], vf[JF_MAX_OBJ];
    for (int o = 0; o < O; ++o) {
        const long long* c = counts + (pair0 + o) * 6;
        const double j = metric != IVOSW_METRIC_F ? jf_jaccard(c) : 0.0;
        const double fm = metric != IVOSW_METRIC_J ? jf_fmeasure(c) : 0.0;
        vj[o] = j;
        vf[o] = fm;
        if (per_obj) {
            const double hj = .5 * j, hf = .5 * fm;
            per_obj[pair0 + o] = metric == IVOSW_METRIC_J ? j : metric == IVOSW_METRIC_F ? fm : hj + hf;
        }
    }
    double q;
    if (metric == IVOSW_METRIC_J) q = jf_row_mean(vj, O);
    else if (metric == IVOSW_METRIC_F) q = jf_row_mean(vf, O);
    else {
        const double hj = .5 * jf_row_mean(vj, O), hf = .5 * jf_row_mean(vf, O);
        q = hj + hf;
    }
    quality[f] = q;
    if (state) {
        state[2 * (size_t)f] = (float)q;
        state[2 * (size_t)f + 1] = annot[f];
    }
}

// Assessment targets (ivosw_qa_targets).  The first `unit_blocks` blocks: one thread per unit u, in the ASSESSMENT's unit order - video
// v's units start at pair_off[v] and run object-major, u = pair_off[v] + obj * N + frame - while its count sextets lie frame-major at
// pair_off[v] + frame * O + obj.  The blocks behind them (only with scores): one thread per video walks that video's units in ascending
// order and forms the reference loop's fp32 sums (quality_assessment.py:251-263); it recomputes each target from the counts with the
// same device function, so it does not wait for the unit threads.
__device__ __forceinline__ double qa_unit_target(const long long* c, int metric) {
    if (metric == IVOSW_METRIC_J) return jf_jaccard(c);
    if (metric == IVOSW_METRIC_F) return jf_fmeasure(c);
    const double hj = .5 * jf_jaccard(c), hf = .5 * jf_fmeasure(c);
    return hj + hf;
}

__global__ __launch_bounds__(64) void qa_targets_kernel(const long long* __restrict__ counts, JfReduceTable tab, int n_seqs, long long units,
                                                        int unit_blocks, int metric, const float* __restrict__ scores,
                                                        double* __restrict__ target, uint8_t* __restrict__ valid, float* __restrict__ loss,
                                                        float* __restrict__ diff, int* __restrict__ n_valid) {
    if ((int)blockIdx.x < unit_blocks) {
        const long long u = (long long)blockIdx.x * blockDim.x + threadIdx.x;
        if (u >= units) return;
        int lo = 0, hi = n_seqs - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (tab.pair_off[mid] <= u) lo = mid;
            else hi = mid - 1;
        }
        const int O = tab.n_obj[lo], N = tab.seq.row_off[lo + 1] - tab.seq.row_off[lo];
        const long long local = u - tab.pair_off[lo];
        const int obj = (int)(local / N), frame = (int)(local - (long long)obj * N);
        const long long* c = counts + (tab.pair_off[lo] + (long long)frame * O + obj) * 6;
        target[u] = qa_unit_target(c, metric);
        valid[u] = c[1] > 0 ? 1 : 0;
        return;
    }
    const int v = ((int)blockIdx.x - unit_blocks) * blockDim.x + threadIdx.x;
    if (v >= n_seqs) return;
    const int O = tab.n_obj[v], N = tab.seq.row_off[v + 1] - tab.seq.row_off[v];
    const long long u0 = tab.pair_off[v];
    float l = 0.f, d = 0.f;
    int cnt = 0;
    for (int obj = 0; obj < O; ++obj)
        for (int frame = 0; frame < N; ++frame) {
            const long long* c = counts + (u0 + (long long)frame * O + obj) * 6;
            if (c[1] <= 0) continue;
            const float t = (float)qa_unit_target(c, metric);
            const float e = scores[u0 + (long long)obj * N + frame] - t;
            const float sq = e * e;
            l = l + sq;
            d = d + fabsf(e);
            ++cnt;
        }
    loss[v] = cnt ? l / (float)cnt : 0.f;
    diff[v] = cnt ? d / (float)cnt : 0.f;
    n_valid[v] = cnt;
}

}  // namespace
}  // namespace ivosw

extern "C" size_t ivosw_jf_videos_ws_bytes(const ivosw_jf_video_t* videos, int n_videos) {
    size_t bytes = 0;
    if (!videos || ivosw::jf_videos_table(__func__, videos, n_videos, nullptr, &bytes, nullptr, nullptr, nullptr, nullptr) != IVOSW_OK) return 0;
    return bytes;
}

extern "C" int ivosw_jf_counts_videos(const ivosw_jf_video_t* videos, int n_videos, int64_t* counts, void* ws, size_t ws_bytes,
                                      ivosw_stream_t stream) {
    using namespace ivosw;
    IVOSW_REQUIRE(videos && counts && ws, "null pointer");
    JfTable t;
    size_t need = 0, n_counts = 0;
    int max_h = 0, max_w = 0;
    long long max_words = 0;
    if (jf_videos_table(__func__, videos, n_videos, &t, &need, &n_counts, &max_h, &max_w, &max_words) != IVOSW_OK) return IVOSW_ERR_ARG;
    IVOSW_ON_DEVICE_OF(counts);
    if (ws_bytes < need) {
        set_error("ivosw_jf_counts_videos: workspace %zu < %zu", ws_bytes, need);
        return IVOSW_ERR_WS;
    }
    hipStream_t st = as_stream(stream);
    t.bitmaps = static_cast<uint32_t*>(ws);
    t.counts = reinterpret_cast<unsigned long long*>(counts);
    const int frames = t.frame_off[n_videos], pairs = t.fo_off[n_videos];
    (void)hipMemsetAsync(counts, 0, n_counts * sizeof(int64_t), st);
    hipLaunchKernelGGL(jf_boundary_row_videos_kernel, dim3((max_h + 4 * JF_RPW - 1) / (4 * JF_RPW), (max_w + 1023) / 1024, frames), dim3(256),
                       0, st, t);
    hipLaunchKernelGGL(jf_match_videos_kernel, dim3((unsigned)((max_words + 255) / 256), pairs, 2), dim3(256), 0, st, t);
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}

extern "C" int ivosw_jf_reduce_ragged(const int64_t* counts, const int* n_obj, const int* lengths, int n_seqs, int metric,
                                      const float* annot_counts, double* per_obj, double* quality, float* state, ivosw_stream_t stream) {
    using namespace ivosw;
    IVOSW_REQUIRE(counts && n_obj && lengths && quality, "null pointer");
    IVOSW_REQUIRE((state == nullptr) == (annot_counts == nullptr), "state and annot_counts go together: both or neither");
    if (metric != IVOSW_METRIC_J && metric != IVOSW_METRIC_F && metric != IVOSW_METRIC_J_AND_F) {
        set_error("%s: unknown metric %d (IVOSW_METRIC_J = 0, IVOSW_METRIC_F = 1, IVOSW_METRIC_J_AND_F = 2)", __func__, metric);
        return IVOSW_ERR_ARG;
    }
    JfReduceTable tab;
    const long rows = ragged_rows(__func__, lengths, n_seqs, &tab.seq);
    if (rows < 0) return IVOSW_ERR_ARG;
    long long pairs = 0;
    for (int k = 0; k < IVOSW_MAX_SEQS; ++k) {
        tab.n_obj[k] = 1;
        tab.pair_off[k] = pairs;
        if (k >= n_seqs) continue;
        if (n_obj[k] < 1 || n_obj[k] > JF_MAX_OBJ) {
            set_error("%s: video %d: n_obj %d outside [1, %d]", __func__, k, n_obj[k], JF_MAX_OBJ);
            return IVOSW_ERR_ARG;
        }
        tab.n_obj[k] = (uint8_t)n_obj[k];
        pairs += (long long)n_obj[k] * lengths[k];
    }
    IVOSW_ON_DEVICE_OF(quality);
    hipLaunchKernelGGL(jf_reduce_ragged_kernel, dim3((unsigned)((rows + 63) / 64)), dim3(64), 0, as_stream(stream),
                       reinterpret_cast<const long long*>(counts), tab, n_seqs, (int)rows, metric, annot_counts, per_obj, quality, state);
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}

// ------------------------------------------------------------------------------------------------ assessment samples (8-bit planes)
namespace ivosw {
namespace {
// ivosw_qa_video_t -> the label-map descriptors jf_videos_table checks and lays out (pred = the plane stack); thresholds beside them.
int qa_videos_as_jf(const char* who, const ivosw_qa_video_t* videos, int n_videos, ivosw_jf_video_t* out, JfThresholds* th) {
    if (n_videos < 1 || n_videos > IVOSW_MAX_JF_VIDEOS) {
        set_error("%s: n_videos %d outside [1, %d]", who, n_videos, IVOSW_MAX_JF_VIDEOS);
        return IVOSW_ERR_ARG;
    }
    for (int k = 0; k < n_videos; ++k) {
        const ivosw_qa_video_t& d = videos[k];
        if (!d.planes) {
            set_error("%s: video %d: NULL planes", who, k);
            return IVOSW_ERR_ARG;
        }
        ivosw_jf_video_t& j = out[k];
        j.gt = d.gt; j.pred = d.planes; j.n_frames = d.n_frames; j.H = d.H; j.W = d.W; j.n_obj = d.n_obj; j.bound_pix = d.bound_pix;
        memcpy(j.obj_ids, d.obj_ids, sizeof j.obj_ids);
        if (th) th->thr[k] = d.thr;
    }
    if (th)
        for (int k = n_videos; k < IVOSW_MAX_JF_VIDEOS; ++k) th->thr[k] = 0;
    return IVOSW_OK;
}
}  // namespace
}  // namespace ivosw

extern "C" size_t ivosw_qa_counts_ws_bytes(const ivosw_qa_video_t* videos, int n_videos) {
    using namespace ivosw;
    ivosw_jf_video_t jv[IVOSW_MAX_JF_VIDEOS];
    size_t bytes = 0;
    if (!videos || qa_videos_as_jf(__func__, videos, n_videos, jv, nullptr) != IVOSW_OK) return 0;
    if (jf_videos_table(__func__, jv, n_videos, nullptr, &bytes, nullptr, nullptr, nullptr, nullptr) != IVOSW_OK) return 0;
    return bytes;
}

extern "C" int ivosw_qa_counts_videos(const ivosw_qa_video_t* videos, int n_videos, int64_t* counts, void* ws, size_t ws_bytes,
                                      ivosw_stream_t stream) {
    using namespace ivosw;
    IVOSW_REQUIRE(videos && counts && ws, "null pointer");
    ivosw_jf_video_t jv[IVOSW_MAX_JF_VIDEOS];
    JfThresholds th;
    if (qa_videos_as_jf(__func__, videos, n_videos, jv, &th) != IVOSW_OK) return IVOSW_ERR_ARG;
    JfTable t;
    size_t need = 0, n_counts = 0;
    int max_h = 0, max_w = 0;
    long long max_words = 0;
    if (jf_videos_table(__func__, jv, n_videos, &t, &need, &n_counts, &max_h, &max_w, &max_words) != IVOSW_OK) return IVOSW_ERR_ARG;
    IVOSW_ON_DEVICE_OF(counts);
    if (ws_bytes < need) {
        set_error("ivosw_qa_counts_videos: workspace %zu < %zu", ws_bytes, need);
        return IVOSW_ERR_WS;
    }
    hipStream_t st = as_stream(stream);
    t.bitmaps = static_cast<uint32_t*>(ws);
    t.counts = reinterpret_cast<unsigned long long*>(counts);
    const int frames = t.frame_off[n_videos], pairs = t.fo_off[n_videos];
    (void)hipMemsetAsync(counts, 0, n_counts * sizeof(int64_t), st);
    hipLaunchKernelGGL(jf_boundary_row_planes_videos_kernel, dim3((max_h + 4 * JF_RPW - 1) / (4 * JF_RPW), (max_w + 1023) / 1024, frames),
                       dim3(256), 0, st, t, th);
    hipLaunchKernelGGL(jf_match_videos_kernel, dim3((unsigned)((max_words + 255) / 256), pairs, 2), dim3(256), 0, st, t);
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}

extern "C" int ivosw_qa_targets(const int64_t* counts, const int* n_obj, const int* lengths, int n_seqs, int metric, const float* scores,
                                double* target, uint8_t* valid, float* loss, float* diff, int* n_valid, ivosw_stream_t stream) {
    using namespace ivosw;
    IVOSW_REQUIRE(counts && n_obj && lengths && target && valid, "null pointer");
    IVOSW_REQUIRE(scores ? (loss && diff && n_valid) : (!loss && !diff && !n_valid),
                  "scores, loss, diff and n_valid go together: all or none");
    if (metric != IVOSW_METRIC_J && metric != IVOSW_METRIC_F && metric != IVOSW_METRIC_J_AND_F) {
        set_error("%s: unknown metric %d (IVOSW_METRIC_J = 0, IVOSW_METRIC_F = 1, IVOSW_METRIC_J_AND_F = 2)", __func__, metric);
        return IVOSW_ERR_ARG;
    }
    JfReduceTable tab;
    const long rows = ragged_rows(__func__, lengths, n_seqs, &tab.seq);
    if (rows < 0) return IVOSW_ERR_ARG;
    long long units = 0;
    for (int k = 0; k < IVOSW_MAX_SEQS; ++k) {
        tab.n_obj[k] = 1;
        tab.pair_off[k] = units;
        if (k >= n_seqs) continue;
        if (n_obj[k] < 1 || n_obj[k] > JF_MAX_OBJ) {
            set_error("%s: video %d: n_obj %d outside [1, %d]", __func__, k, n_obj[k], JF_MAX_OBJ);
            return IVOSW_ERR_ARG;
        }
        tab.n_obj[k] = (uint8_t)n_obj[k];
        units += (long long)n_obj[k] * lengths[k];
    }
    IVOSW_ON_DEVICE_OF(target);
    const int unit_blocks = (int)((units + 63) / 64), video_blocks = scores ? (n_seqs + 63) / 64 : 0;      // units <= 32 * 2^20
    hipLaunchKernelGGL(qa_targets_kernel, dim3((unsigned)(unit_blocks + video_blocks)), dim3(64), 0, as_stream(stream),
                       reinterpret_cast<const long long*>(counts), tab, n_seqs, units, unit_blocks, metric, scores, target, valid, loss, diff,
                       n_valid);
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}
