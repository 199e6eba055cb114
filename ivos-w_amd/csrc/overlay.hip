// Session overlays on the device: the pictures an annotator is shown - a frame with the current mask drawn on it.
//
// Reference (utils/utils_ipn.py), each on ONE uint8 image and ONE binary mask, on the CPU, in float64 and through
// scipy.ndimage.binary_dilation:
//     overlay_davis(image, mask, rgb, cscale, alpha)   :113-128    inside: trunc(v * alpha + (1.0 * (1 - alpha)) * c); contour: 0
//     checkerboard / BIG_BOARD                         :131-143    20 x 20 squares of 223 and 32, 223 in the top-left one
//     overlay_checker(image, mask)                     :146-157    outside: the board
//     overlay_color(image, mask, rgb)                  :160-171    outside: rgb
//     overlay_fade(image, mask)                        :174-190    outside: trunc(0.4 * v); contour: (0, 255, 255)
// The contour is binary_dilation(mask) ^ mask with scipy's default cross and border_value = 0: a pixel NOT in the mask with an edge
// neighbour inside the image that is.
//
// overlay_kernel: ONE launch renders up to OVL_MAX_FRAMES frames of a video from its frames (RGBX8 bytes, or fp32 planes whose byte is
// rintf(f * 255) clamped, NaN = 0) and its uint8 label map (value i + 1 = object i) into RGB8 or RGBX8 pictures.  `select` picks the
// binary mask: o = (label == o), 0 = every object 1 .. n_objects.  A label value becomes the object it stands for (0 = none) and every
// style is a function of a pixel's own object and those of its four neighbours.
// DAVIS with select = 0 is the reference function applied once per object in ascending order to the running image; per pixel that walk
// collapses to: a neighbour of a LARGER object (or any object, for a pixel of none) draws its contour last -> 0; otherwise a pixel of
// object L is trunc(v' * alpha + k[L]) with v' = 0 when a neighbour belongs to a SMALLER object (its contour ran first), else the image
// byte.  k[o][c] = (1.0 * (1 - alpha)) * c is formed on the host in float64; the product and the sum are rounded separately
// (#pragma clang fp contract(off)).
//
// The frame list and the k table travel inside the kernel arguments, as the weights of ipn_merge_kernel do: no allocation, no copy,
// capture-safe.  A plain streaming kernel: no LDS, no atomics, no scratch.  Per pixel it moves 4 B (RGBX8) or 12 B (fp32) of frame,
// 1 B of label (the rows above and below come from the caches) and 3 or 4 B of picture; how far each path is from the memory roof is
// measured by tools/overlay_probe.py (profiles/overlay_probe.txt).
#include "lane_group.h"
#include <limits.h>
#include <string.h>

namespace ivosw {

namespace {
constexpr int OVL_MAX_FRAMES = 256;                  // frames per launch (their ids are kernel arguments)
constexpr int OVL_MAX_OBJECTS = 32;

struct OverlayArgs {
    const void* frames;    // RGBX8 [n][H][W][4] or fp32 [n][3][H][W]
    const uint8_t* labels; // [n][H][W]
    uint8_t* out;          // RGB8 [m][H][W][3] or RGBX8 [m][H][W][4]
    int H, W, m0;          // this launch writes the pictures m0 .. m0 + gridDim.y - 1
    int style, n_objects, select;
    double alpha;
    uint8_t color[4];
    int frame[OVL_MAX_FRAMES];                       // picture m0 + j shows frame frame[j]
    double k[OVL_MAX_OBJECTS][3];                    // DAVIS: (1.0 * (1 - alpha)) * palette[o][c]
};

// the object a label value stands for, 0 = none
__device__ __forceinline__ int effective(unsigned v, int n_objects, int select) {
    return select ? ((int)v == select ? select : 0) : (v - 1u < (unsigned)n_objects ? (int)v : 0);
}

// the image byte of an fp32 colour value: rintf(f * 255) clamped to 0 .. 255, NaN -> 0 (u8 / 255 gives u8 back)
__device__ __forceinline__ unsigned byte_of(float f) {
#pragma clang fp contract(off)
    const float r = rintf(f * 255.0f);
    return r >= 0.0f ? (r > 255.0f ? 255u : (unsigned)r) : 0u;                 // a NaN fails r >= 0
}

__device__ __forceinline__ unsigned trunc_u8(double v) { return (unsigned)(int)v & 255u; }

template <int V> struct LabelWord { using type = uint8_t; };
template <> struct LabelWord<2> { using type = uint16_t; };
template <> struct LabelWord<4> { using type = uint32_t; };
}  // namespace

// V = pixels per thread, consecutive in a row: 4, 2 or 1.  V > 1 needs W % V == 0, labels on the V-byte grid, frames on the 4 V-byte
// grid and out on the V-byte (RGB8) or 4 V-byte (RGBX8) grid (ivosw_overlay_lane_pixels).  W = 854, the width of DAVIS 480p, takes V = 2.  F32: fp32 planes, else RGBX8 bytes.  X: RGBX8 pictures, else RGB8.
// blockIdx.y is the picture within the launch: its frame id is wave-uniform.
template <int V, bool F32, bool X>
__global__ __launch_bounds__(256) void overlay_kernel(OverlayArgs a) {
#pragma clang fp contract(off)
    const unsigned wq = (unsigned)a.W / V;
    const unsigned item = blockIdx.x * 256u + threadIdx.x;                     // H * W <= INT_MAX (checked by the launcher)
    if (item >= (unsigned)a.H * wq) return;
    const int y = (int)(item / wq), x0 = (int)(item - (unsigned)y * wq) * V;
    const long HW = (long)a.H * a.W;
    const long f = a.frame[blockIdx.y];
    const long pix = (long)y * a.W + x0;                                       // offset inside a frame

    // ---- labels: e[1 + p] = the object of pixel x0 + p, e[0] and e[V + 1] its row neighbours, up / dn the rows above and below
    const uint8_t* lrow = a.labels + f * HW + pix;
    int e[V + 2], up[V], dn[V];
    e[0] = e[V + 1] = 0;
#pragma unroll
    for (int p = 0; p < V; ++p) up[p] = dn[p] = 0;
    using LW = typename LabelWord<V>::type;                                   // V label bytes: one aligned word
    const LW mid = *reinterpret_cast<const LW*>(lrow);
#pragma unroll
    for (int p = 0; p < V; ++p) e[1 + p] = effective(((unsigned)mid >> (8 * p)) & 255u, a.n_objects, a.select);
    if (x0 >= V) e[0] = effective((unsigned)*reinterpret_cast<const LW*>(lrow - V) >> (8 * (V - 1)), a.n_objects, a.select);
    if (x0 + V < a.W) e[V + 1] = effective((unsigned)*reinterpret_cast<const LW*>(lrow + V) & 255u, a.n_objects, a.select);
    if (y >= 1) {
        const LW w = *reinterpret_cast<const LW*>(lrow - a.W);
#pragma unroll
        for (int p = 0; p < V; ++p) up[p] = effective(((unsigned)w >> (8 * p)) & 255u, a.n_objects, a.select);
    }
    if (y + 1 < a.H) {
        const LW w = *reinterpret_cast<const LW*>(lrow + a.W);
#pragma unroll
        for (int p = 0; p < V; ++p) dn[p] = effective(((unsigned)w >> (8 * p)) & 255u, a.n_objects, a.select);
    }

    // ---- the image bytes: c[p][ch]
    unsigned c[V][3];
    if constexpr (F32) {
        const float* fr = static_cast<const float*>(a.frames) + f * 3 * HW + pix;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            float q[V];
            load_group(fr + ch * HW, q);
#pragma unroll
            for (int p = 0; p < V; ++p) c[p][ch] = byte_of(q[p]);
        }
    } else {
        uint32_t w[V];
        load_group(static_cast<const uint32_t*>(a.frames) + f * HW + pix, w);
#pragma unroll
        for (int p = 0; p < V; ++p) { c[p][0] = w[p] & 255u; c[p][1] = (w[p] >> 8) & 255u; c[p][2] = (w[p] >> 16) & 255u; }
    }

    // ---- the style, pixel by pixel
    uint32_t px[V];                                                            // R | G << 8 | B << 16, byte 3 = 0
#pragma unroll
    for (int p = 0; p < V; ++p) {
        const int own = e[1 + p];
        const int l = e[p], r = e[2 + p], u = up[p], d = dn[p];
        const int near = max(max(l, r), max(u, d));
        unsigned o0 = c[p][0], o1 = c[p][1], o2 = c[p][2];
        if (a.style == IVOSW_OVERLAY_DAVIS) {
            if (near > own) {
                o0 = o1 = o2 = 0;
            } else if (own) {
                const bool below = (l && l < own) || (r && r < own) || (u && u < own) || (d && d < own);
                const double* k = a.k[own - 1];
                const double v0 = below ? 0.0 : (double)o0, v1 = below ? 0.0 : (double)o1, v2 = below ? 0.0 : (double)o2;
                const double p0 = v0 * a.alpha, p1 = v1 * a.alpha, p2 = v2 * a.alpha;
                o0 = trunc_u8(p0 + k[0]); o1 = trunc_u8(p1 + k[1]); o2 = trunc_u8(p2 + k[2]);
            }
        } else if (a.style == IVOSW_OVERLAY_FADE) {
            if (!own) {
                if (near) { o0 = 0; o1 = 255; o2 = 255; }
                else { o0 = trunc_u8(0.4 * (double)o0); o1 = trunc_u8(0.4 * (double)o1); o2 = trunc_u8(0.4 * (double)o2); }
            }
        } else if (a.style == IVOSW_OVERLAY_CHECKER) {
            if (!own) o0 = o1 = o2 = ((y / 20 + (x0 + p) / 20) & 1) ? 32u : 223u;
        } else {
            if (!own) { o0 = a.color[0]; o1 = a.color[1]; o2 = a.color[2]; }
        }
        px[p] = o0 | (o1 << 8) | (o2 << 16);
    }

    // ---- the picture
    const long opix = (long)(a.m0 + (int)blockIdx.y) * HW + pix;
    if constexpr (X) {
        store_group(reinterpret_cast<uint32_t*>(a.out) + opix, px);
    } else {
        uint8_t* o = a.out + 3 * opix;
        if constexpr (V == 4) {                                                // 12 bytes: R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3
            uint32_t* o32 = reinterpret_cast<uint32_t*>(o);
            o32[0] = px[0] | (px[1] << 24);
            o32[1] = (px[1] >> 8) | (px[2] << 16);
            o32[2] = (px[2] >> 16) | (px[V - 1] << 8);
        } else if constexpr (V == 2) {                                         // 6 bytes: R0 G0 | B0 R1 | G1 B1
            uint16_t* o16 = reinterpret_cast<uint16_t*>(o);
            o16[0] = (uint16_t)px[0];
            o16[1] = (uint16_t)((px[0] >> 16) | (px[V - 1] << 8));
            o16[2] = (uint16_t)(px[V - 1] >> 8);
        } else {
            o[0] = (uint8_t)px[0]; o[1] = (uint8_t)(px[0] >> 8); o[2] = (uint8_t)(px[0] >> 16);
        }
    }
}

}  // namespace ivosw

// pixels per lane of the kernel a call with these buffers runs: 4, 2 or 1 - the widest whose words all lie on their grids
extern "C" int ivosw_overlay_lane_pixels(const void* frames, const uint8_t* labels, int W, const void* out, int out_kind) {
    if (ivosw::scalar_forced("IVOSW_OVERLAY_SCALAR") || W < 1) return 1;
    for (int v = 4; v > 1; v >>= 1)                      // per lane: v label bytes, 4 v bytes of frame (of each plane), 3 v or 4 v bytes of picture
        if (W % v == 0 && ivosw::on_grid(v, labels) && ivosw::on_grid(4 * v, frames) && ivosw::on_grid(out_kind == IVOSW_OUT_RGBX8 ? 4 * v : v, out)) return v;
    return 1;
}

extern "C" int ivosw_overlay_frames(const void* frames, int frames_kind, const uint8_t* labels, int n_frames, int H, int W,
                                    const int* frame_ids, int n_ids, const ivosw_overlay_t* opt, void* out, int out_kind,
                                    ivosw_stream_t stream) {
    using namespace ivosw;
    IVOSW_REQUIRE(frames, "null frames");
    IVOSW_REQUIRE(labels, "null labels");
    IVOSW_REQUIRE(opt, "null opt");
    IVOSW_REQUIRE(out, "null out");
    IVOSW_REQUIRE(frames_kind == IVOSW_FRAMES_F32 || frames_kind == IVOSW_FRAMES_RGBX8, "unknown frames_kind");
    IVOSW_REQUIRE(out_kind == IVOSW_OUT_RGB8 || out_kind == IVOSW_OUT_RGBX8, "unknown out_kind");
    IVOSW_REQUIRE(opt->style >= IVOSW_OVERLAY_DAVIS && opt->style <= IVOSW_OVERLAY_COLOR, "unknown style");
    IVOSW_REQUIRE(n_frames >= 1 && H >= 1 && W >= 1, "bad shape (n_frames, H or W < 1)");
    IVOSW_REQUIRE((long)H * W <= INT_MAX, "frame too large for 32-bit pixel indices (H * W > INT_MAX)");
    IVOSW_REQUIRE(opt->n_objects >= 1 && opt->n_objects <= OVL_MAX_OBJECTS, "n_objects outside [1, 32]");
    IVOSW_REQUIRE(opt->select >= 0 && opt->select <= opt->n_objects, "select outside [0, n_objects]");
    IVOSW_REQUIRE(opt->alpha >= 0.0 && opt->alpha <= 1.0, "alpha not in [0, 1]");          // a NaN fails both
    IVOSW_REQUIRE(!frame_ids || n_ids >= 1, "frame list of length < 1");
    const long m = frame_ids ? n_ids : n_frames;
    if (frame_ids)
        for (long j = 0; j < m; ++j)
            if (frame_ids[j] < 0 || frame_ids[j] >= n_frames) {
                set_error("%s: frame_ids[%ld] = %d outside [0, %d)", __func__, j, frame_ids[j], n_frames);
                return IVOSW_ERR_ARG;
            }
    IVOSW_REQUIRE(((uintptr_t)frames & 3) == 0, frames_kind == IVOSW_FRAMES_RGBX8 ? "RGBX8 frames are not 4-byte aligned" : "fp32 frames are not 4-byte aligned");
    IVOSW_REQUIRE(out_kind != IVOSW_OUT_RGBX8 || ((uintptr_t)out & 3) == 0, "RGBX8 out is not 4-byte aligned");
    const long HW = (long)H * W;
    IVOSW_REQUIRE(m <= (1L << 40) / HW, "more than 2^40 pixels of pictures");
    IVOSW_REQUIRE(n_frames <= (1L << 40) / HW, "more than 2^40 pixels of frames");               // (the byte extents below cannot wrap)
    const uintptr_t o0 = (uintptr_t)out, o1 = o0 + (uintptr_t)m * HW * (out_kind == IVOSW_OUT_RGBX8 ? 4 : 3);
    const uintptr_t f0 = (uintptr_t)frames, f1 = f0 + (uintptr_t)n_frames * HW * (frames_kind == IVOSW_FRAMES_F32 ? 12 : 4);
    const uintptr_t l0 = (uintptr_t)labels, l1 = l0 + (uintptr_t)n_frames * HW;
    IVOSW_REQUIRE(o1 <= f0 || f1 <= o0, "out overlaps frames");
    IVOSW_REQUIRE(o1 <= l0 || l1 <= o0, "out overlaps labels");
    IVOSW_ON_DEVICE_OF(labels);

    OverlayArgs a{};
    a.frames = frames; a.labels = labels; a.out = static_cast<uint8_t*>(out);
    a.H = H; a.W = W; a.style = opt->style; a.n_objects = opt->n_objects; a.select = opt->select; a.alpha = opt->alpha;
    memcpy(a.color, opt->color, 3);
    const double rest = 1.0 * (1 - opt->alpha);
    for (int o = 0; o < OVL_MAX_OBJECTS; ++o)
        for (int ch = 0; ch < 3; ++ch) a.k[o][ch] = rest * (double)opt->palette[o][ch];
    const bool f32 = frames_kind == IVOSW_FRAMES_F32, x = out_kind == IVOSW_OUT_RGBX8;
    const int V = ivosw_overlay_lane_pixels(frames, labels, W, out, out_kind);
    const unsigned gx = lane_blocks(HW, V);
    hipStream_t st = as_stream(stream);
    for (long m0 = 0; m0 < m; m0 += OVL_MAX_FRAMES) {
        const int nf = (int)(m - m0 < OVL_MAX_FRAMES ? m - m0 : OVL_MAX_FRAMES);
        a.m0 = (int)m0;
        for (int j = 0; j < nf; ++j) a.frame[j] = frame_ids ? frame_ids[m0 + j] : (int)(m0 + j);
        const dim3 grid(gx, nf), block(256);
        dispatch_lanes<4, 2, 1>(V, [&](auto v) {
            constexpr int LV = decltype(v)::value;
            if (f32 && x) hipLaunchKernelGGL((overlay_kernel<LV, true, true>), grid, block, 0, st, a);
            else if (f32) hipLaunchKernelGGL((overlay_kernel<LV, true, false>), grid, block, 0, st, a);
            else if (x) hipLaunchKernelGGL((overlay_kernel<LV, false, true>), grid, block, 0, st, a);
            else hipLaunchKernelGGL((overlay_kernel<LV, false, false>), grid, block, 0, st, a);
        });
        IVOSW_CHECK_LAUNCH();
    }
    return IVOSW_OK;
}
