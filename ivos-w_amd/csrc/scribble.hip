// The input side of an interaction on the device: the scribbles the annotator (or the robot) has just drawn become the label maps that
// MANet's scribble_label, IPN's dilation (ivosw_ipn_dilate) and the overlays read - no [n_frames,H,W] host array, no upload of one.
//
// Reference: eval_agent_manet.py:368-374 (scribbles2mask at the embedding resolution, ToTensor, rough_ROI on the first interaction,
// .cuda()), eval_agent_ipn.py (scribbles2mask at full resolution, Dilate_mask) and utils/utils_manet.py:22-39 (rough_ROI).
// davisinteractive's scribbles2mask is not in the reference tree: the line rule below (include/ivosw.h states it in full) is this
// project's DEFINITION, parity with the library's own rasteriser is unpinned.  rough_ROI is in the tree: its rule, the exclusive ends
// of its slices included, is kept bit for bit (tests/golden/scribble_fixtures.npz).
//
// ivosw_scribble_raster, three steps on one stream, no allocation, no synchronisation (capture-safe):
//   clear     ONE memset over the workspace: a uint32 key plane per map and four box integers per map.
//   draw      ONE launch, one WAVE per point i of the point array: the wave finds the path that owns i (a binary search in the path
//             table, wave-uniform) and its 64 lanes share the steps s = 0 .. a of the segment i -> i + 1 through the closed form
//             m(s) = (2 b s + a) / (2 a) of the Bresenham loop, so a two-point path across 854 pixels takes 14 rounds of one wave, not
//             855 steps of one lane.  Each plot is an atomicMax of (path index + 1) into the key plane: the highest path index on a pixel
//             is the host's LAST assignment, whatever the schedule.  The map's box takes four atomicMax per segment from lane 0: a
//             segment never leaves the box of its two end points, so the wave's reduction over its plots is that of the end points.  All
//             four box integers are kept in the form a maximum can build from 0 (H - y, y + 1, W - x, x + 1: 0 = nothing plotted).
//   finalise  ONE launch: key ? object[key - 1] : default, the rough_ROI rule from the box in the same pass when roi_dist >= 0, 16 pixels
//             per lane with 16-byte loads and stores (one for the int8 map, four for the float planes) when the outputs are on the
//             16-byte grid; the last lane's partial group, and every group when an output is off that grid, goes element by element.
// ivosw_rough_roi, the stand-alone body: a memset of four integers per image, a box scan (per-lane running maxima, a wave reduction, four
// atomics per wave) and a fill (float4 when in and out are on the 16-byte grid), two launches.
// Vector memory operations only; no LDS, no scratch.
#include "lane_group.h"
#include <limits.h>

namespace ivosw {

namespace {
constexpr long SCR_MAX_PIXELS = INT_MAX;             // n_maps * H * W: flat pixel indices are 32-bit in the kernels

struct DrawArgs {
    const int* points;     // [P][2] = x, y
    const int* paths;      // [n_paths][4] = first point, n points, object id, map
    uint32_t* keys;        // [n_maps][H][W]
    uint32_t* box;         // [n_maps][4] = max(H - y), max(y + 1), max(W - x), max(x + 1)
    int P, n_paths, n_maps, H, W, bresenham;
};

struct FinalArgs {
    const uint32_t* keys;
    const uint32_t* box;
    const int* paths;
    int8_t* out_i8;        // [n_maps][H][W] or nullptr
    float* out_f32;        // [n_maps][H][W] or nullptr
    int N, HW, H, W, n_maps, default_value, roi_dist;          // N = n_maps * HW
};

struct RoiArgs {
    const float* in;       // [b][h][w]
    float* out;
    uint32_t* box;         // [b][4]
    int b, H, W, HW, dist;
};

// rows [r0, r1) x columns [c0, c1) keep their value, everything else becomes 0
struct Roi { int r0, r1, c0, c1; };

// utils/utils_manet.py:36 from a box in the maxima form: [max(hmin - dist, 0), min(hmax + dist, h - 1)) and the same for the columns -
// BOTH ends exclusive, so a box on the last row or column loses it.  dist <= max(H, W) (the launcher clamps it: the same slices).
__device__ __forceinline__ Roi roi_of_box(const uint32_t* box, int H, int W, int dist) {
    const int b0 = (int)box[0], b1 = (int)box[1], b2 = (int)box[2], b3 = (int)box[3];
    if (b1 == 0) return Roi{0, 0, 0, 0};                                   // no pixel != -1: all 0 (the reference raises here)
    return Roi{max(H - b0 - dist, 0), min(b1 - 1 + dist, H - 1), max(W - b2 - dist, 0), min(b3 - 1 + dist, W - 1)};
}

__device__ __forceinline__ Roi roi_of_map(const FinalArgs& a, int m) {
    if (a.roi_dist < 0) return Roi{0, a.H, 0, a.W};                        // off: everything stays
    if (a.default_value != -1)                                             // every pixel is != -1: the box is the whole map
        return Roi{0, a.H - 1, 0, a.W - 1};
    return roi_of_box(a.box + 4 * (long)m, a.H, a.W, a.roi_dist);
}

__device__ __forceinline__ int label_of(const FinalArgs& a, uint32_t key, int y, int x, const Roi& r) {
    const int v = key ? a.paths[4 * (long)(key - 1) + 2] : a.default_value;
    return (y >= r.r0 && y < r.r1 && x >= r.c0 && x < r.c1) ? v : 0;
}
}  // namespace

// One wave per point i; blockDim = 256 = 4 points per block.
__global__ __launch_bounds__(256) void scribble_draw_kernel(DrawArgs a) {
    const int lane = threadIdx.x & 63;
    const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= a.P) return;
    int lo = 0, hi = a.n_paths;                                            // the last path whose first point is <= i (first is ascending)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.paths[4 * (long)mid] <= i) lo = mid; else hi = mid;
    }
    const int* row = a.paths + 4 * (long)lo;
    const int first = row[0], n = row[1], map = row[3];
    if (i < first || i >= (long)first + n) return;                         // a point no path owns
    if ((unsigned)map >= (unsigned)a.n_maps) return;                       // (the host copy was validated; the device table is the caller's)
    const bool single = !a.bresenham || n == 1;
    if (!single && i + 1 == (long)first + n) return;                       // the last point of a polyline: its segment's last step
    const int x0 = a.points[2 * i], y0 = a.points[2 * i + 1];
    int x1 = x0, y1 = y0;
    if (!single) { x1 = a.points[2 * i + 2]; y1 = a.points[2 * i + 3]; }
    if ((unsigned)x0 >= (unsigned)a.W || (unsigned)y0 >= (unsigned)a.H || (unsigned)x1 >= (unsigned)a.W || (unsigned)y1 >= (unsigned)a.H)
        return;                                                            // an end point outside the map: nothing of the segment is drawn
    const int dx = abs(x1 - x0), dy = abs(y1 - y0);
    const int sx = x1 - x0 > 0 ? 1 : -1, sy = y1 - y0 > 0 ? 1 : -1;
    const bool xdrive = dx > dy;                                           // dx == dy: y drives
    const unsigned la = xdrive ? dx : dy, lb = xdrive ? dy : dx;           // driving and minor length
    uint32_t* plane = a.keys + (long)map * a.H * a.W;
    for (unsigned s = lane; s <= la; s += 64) {
        const unsigned m = la ? (unsigned)((2ull * lb * s + la) / (2ull * la)) : 0u;
        const int x = xdrive ? x0 + sx * (int)s : x0 + sx * (int)m;
        const int y = xdrive ? y0 + sy * (int)m : y0 + sy * (int)s;
        atomicMax(plane + (long)y * a.W + x, (uint32_t)lo + 1u);
    }
    if (lane == 0) {
        uint32_t* box = a.box + 4 * (long)map;
        atomicMax(box + 0, (uint32_t)(a.H - min(y0, y1)));
        atomicMax(box + 1, (uint32_t)(max(y0, y1) + 1));
        atomicMax(box + 2, (uint32_t)(a.W - min(x0, x1)));
        atomicMax(box + 3, (uint32_t)(max(x0, x1) + 1));
    }
}

// V = pixels per lane, consecutive in the flat [n_maps * H * W] order (V = 16 needs out_i8 and out_f32 on the 16-byte grid; the keys
// are: they start the workspace, which the entry requires on the 16-byte grid, and a group starts at a multiple of 16 keys).  A group
// that crosses the end goes element by element.
template <int V>
__global__ __launch_bounds__(256) void scribble_final_kernel(FinalArgs a) {
    const long g = ((long)blockIdx.x * 256 + threadIdx.x) * V;
    if (g >= a.N) return;
    const int g0 = (int)g;
    int m = g0 / a.HW;
    const int p = g0 - m * a.HW;
    int y = p / a.W, x = p - y * a.W;
    Roi r = roi_of_map(a, m);
    if constexpr (V > 1) if (g0 <= a.N - V) {
        uint32_t key[V];
        load_group(a.keys + g0, key);
        int v[V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            v[j] = label_of(a, key[j], y, x, r);
            if (++x == a.W) {
                x = 0;
                if (++y == a.H) {
                    y = 0;
                    if (++m < a.n_maps) r = roi_of_map(a, m);
                }
            }
        }
        if (a.out_i8) store_bytes(a.out_i8 + g0, v);
        if (a.out_f32) store_group_as(a.out_f32 + g0, v);
        return;
    }
    const int cnt = min(V, a.N - g0);
    for (int j = 0; j < cnt; ++j) {                                        // the scalar tail (and the whole of the V = 1 kernel)
        const int v = label_of(a, a.keys[g0 + j], y, x, r);
        if (a.out_i8) a.out_i8[g0 + j] = (int8_t)v;
        if (a.out_f32) a.out_f32[g0 + j] = (float)v;
        if (++x == a.W) {
            x = 0;
            if (++y == a.H) {
                y = 0;
                if (++m < a.n_maps) r = roi_of_map(a, m);
            }
        }
    }
}

// blockIdx.y = image; the lanes stride over its pixels; a NaN is != -1.
__global__ __launch_bounds__(256) void rough_roi_scan_kernel(RoiArgs a) {
    const float* img = a.in + (long)blockIdx.y * a.HW;
    int b0 = 0, b1 = 0, b2 = 0, b3 = 0;
    for (unsigned p = blockIdx.x * 256u + threadIdx.x; p < (unsigned)a.HW; p += gridDim.x * 256u) {
        if (img[p] != -1.0f) {
            const int y = (int)(p / (unsigned)a.W), x = (int)(p - (unsigned)y * (unsigned)a.W);
            b0 = max(b0, a.H - y); b1 = max(b1, y + 1); b2 = max(b2, a.W - x); b3 = max(b3, x + 1);
        }
    }
    b0 = wave_max(b0); b1 = wave_max(b1); b2 = wave_max(b2); b3 = wave_max(b3);
    if ((threadIdx.x & 63) == 0 && b1 > 0) {
        uint32_t* box = a.box + 4 * (long)blockIdx.y;
        atomicMax(box + 0, (uint32_t)b0); atomicMax(box + 1, (uint32_t)b1); atomicMax(box + 2, (uint32_t)b2); atomicMax(box + 3, (uint32_t)b3);
    }
}

// V = pixels per lane, consecutive in the flat [b * h * w] order (V = 4 needs in and out on the 16-byte grid); out may be in.
template <int V>
__global__ __launch_bounds__(256) void rough_roi_fill_kernel(RoiArgs a) {
    const long N = (long)a.b * a.HW;
    const long g0 = ((long)blockIdx.x * 256 + threadIdx.x) * V;
    if (g0 >= N) return;
    int m = (int)(g0 / a.HW);
    const int p = (int)(g0 - (long)m * a.HW);
    int y = p / a.W, x = p - y * a.W;
    Roi r = roi_of_box(a.box + 4 * (long)m, a.H, a.W, a.dist);
    float v[V];
    const bool full = g0 + V <= N;
    if constexpr (V == 4) if (full) load_group(a.in + g0, v);
    const int cnt = full ? V : (int)(N - g0);
#pragma unroll
    for (int j = 0; j < V; ++j) {
        if (j < cnt) {
            if (!(V == 4 && full)) v[j] = a.in[g0 + j];
            if (!(y >= r.r0 && y < r.r1 && x >= r.c0 && x < r.c1)) v[j] = 0.0f;
            if (!(V == 4 && full)) a.out[g0 + j] = v[j];
            if (++x == a.W) {
                x = 0;
                if (++y == a.H) {
                    y = 0;
                    if (++m < a.b) r = roi_of_box(a.box + 4 * (long)m, a.H, a.W, a.dist);
                }
            }
        }
    }
    if constexpr (V == 4) if (full) store_group(a.out + g0, v);
}

}  // namespace ivosw

extern "C" size_t ivosw_scribble_raster_ws_bytes(int n_maps, int H, int W) {
    using namespace ivosw;
    if (n_maps < 1 || H < 1 || W < 1 || (long)H * W > SCR_MAX_PIXELS || n_maps > SCR_MAX_PIXELS / ((long)H * W)) return 0;
    return align_up((size_t)n_maps * H * W * sizeof(uint32_t), 256) + (size_t)n_maps * 4 * sizeof(uint32_t);
}

extern "C" int ivosw_scribble_raster(const int32_t* points, int n_points, const int32_t* paths, const int32_t* paths_host, int n_paths,
                                     int n_maps, int H, int W, int default_value, int bresenham, int roi_dist, int8_t* out_i8,
                                     float* out_f32, void* ws, size_t ws_bytes, ivosw_stream_t stream) {
    using namespace ivosw;
    IVOSW_REQUIRE(n_paths >= 0, "n_paths < 0");
    IVOSW_REQUIRE(n_points >= 0, "n_points < 0");
    IVOSW_REQUIRE(n_paths == 0 || points, "null points");
    IVOSW_REQUIRE(n_paths == 0 || paths, "null paths");
    IVOSW_REQUIRE(n_paths == 0 || paths_host, "null paths_host");
    IVOSW_REQUIRE(out_i8 || out_f32, "null out_i8 and out_f32 (no output requested)");
    IVOSW_REQUIRE(ws, "null ws");
    IVOSW_REQUIRE(((uintptr_t)ws & 15) == 0, "ws off the 16-byte grid");
    IVOSW_REQUIRE(n_maps >= 1 && H >= 1 && W >= 1, "n_maps, H and W must be positive");
    IVOSW_REQUIRE((long)H * W <= SCR_MAX_PIXELS && n_maps <= SCR_MAX_PIXELS / ((long)H * W), "n_maps * H * W above 2^31 - 1 pixels");
    IVOSW_REQUIRE(default_value >= -128 && default_value <= 127, "default_value outside int8");
    long next = 0;                                                         // the first point a path may start at
    for (int k = 0; k < n_paths; ++k) {
        const int32_t* row = paths_host + 4 * (long)k;
        const char* why = nullptr;
        if (row[1] < 1 || row[0] < 0 || (long)row[0] + row[1] > n_points) why = "its point range lies outside [0, n_points)";
        else if (row[0] < next) why = "its point range is not behind the previous path's (ranges ascend and do not overlap)";
        else if (row[2] < 0 || row[2] > 126) why = "its object id lies outside [0, 126]";
        else if (row[3] < 0 || row[3] >= n_maps) why = "its map index lies outside [0, n_maps)";
        if (why) {
            set_error("%s: paths_host: path %d: %s", __func__, k, why);
            return IVOSW_ERR_ARG;
        }
        next = (long)row[0] + row[1];
    }
    const size_t need = ivosw_scribble_raster_ws_bytes(n_maps, H, W);
    if (ws_bytes < need) {
        set_error("%s: workspace %zu < %zu", __func__, ws_bytes, need);
        return IVOSW_ERR_WS;
    }
    IVOSW_ON_DEVICE_OF(ws);
    const long HW = (long)H * W, N = HW * n_maps;
    Arena arena(ws);
    uint32_t* keys = arena.take<uint32_t>((size_t)N);
    uint32_t* box = arena.take<uint32_t>((size_t)n_maps * 4);
    hipStream_t st = as_stream(stream);
    if (hipMemsetAsync(ws, 0, need, st) != hipSuccess) {
        set_error("%s: HIP error in the workspace memset", __func__);
        return IVOSW_ERR_LAUNCH;
    }
    if (n_paths > 0) {
        DrawArgs d{points, paths, keys, box, n_points, n_paths, n_maps, H, W, bresenham != 0};
        hipLaunchKernelGGL(scribble_draw_kernel, dim3((unsigned)(((long)n_points + 3) / 4)), dim3(256), 0, st, d);
        IVOSW_CHECK_LAUNCH();
    }
    const int max_side = H > W ? H : W;
    FinalArgs f{keys, box, paths, out_i8, out_f32, (int)N, (int)HW, H, W, n_maps, default_value,
                roi_dist < 0 ? -1 : (roi_dist < max_side ? roi_dist : max_side)};
    const int V = !scalar_forced("IVOSW_SCRIBBLE_SCALAR") && on_grid(16, out_i8, out_f32) ? 16 : 1;
    dispatch_lanes<16, 1>(V, [&](auto v) { hipLaunchKernelGGL((scribble_final_kernel<decltype(v)::value>), dim3(lane_blocks(N, V)), dim3(256), 0, st, f); });
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}

extern "C" size_t ivosw_rough_roi_ws_bytes(int b) { return b < 1 ? 0 : (size_t)b * 4 * sizeof(uint32_t); }

extern "C" int ivosw_rough_roi(const float* in, float* out, int b, int h, int w, int dist, void* ws, size_t ws_bytes,
                               ivosw_stream_t stream) {
    using namespace ivosw;
    IVOSW_REQUIRE(in, "null in");
    IVOSW_REQUIRE(out, "null out");
    IVOSW_REQUIRE(ws, "null ws");
    IVOSW_REQUIRE(b >= 1 && h >= 1 && w >= 1, "b, h and w must be positive");
    IVOSW_REQUIRE(b <= 65535, "b above 65535 images (the scan's grid dimension)");
    IVOSW_REQUIRE((long)h * w <= SCR_MAX_PIXELS && b <= SCR_MAX_PIXELS / ((long)h * w), "b * h * w above 2^31 - 1 pixels");
    IVOSW_REQUIRE(dist >= 0, "dist < 0");
    const size_t need = ivosw_rough_roi_ws_bytes(b);
    if (ws_bytes < need) {
        set_error("%s: workspace %zu < %zu", __func__, ws_bytes, need);
        return IVOSW_ERR_WS;
    }
    IVOSW_ON_DEVICE_OF(in);
    const int HW = h * w, max_side = h > w ? h : w;
    RoiArgs a{in, out, static_cast<uint32_t*>(ws), b, h, w, HW, dist < max_side ? dist : max_side};
    hipStream_t st = as_stream(stream);
    if (hipMemsetAsync(ws, 0, need, st) != hipSuccess) {
        set_error("%s: HIP error in the workspace memset", __func__);
        return IVOSW_ERR_LAUNCH;
    }
    const unsigned gx = (unsigned)((HW + 255) / 256);
    hipLaunchKernelGGL(rough_roi_scan_kernel, dim3(gx < 256u ? gx : 256u, (unsigned)b), dim3(256), 0, st, a);
    IVOSW_CHECK_LAUNCH();
    const long N = (long)b * HW;
    const int V = !scalar_forced("IVOSW_SCRIBBLE_SCALAR") && on_grid(16, in, out) ? 4 : 1;
    dispatch_lanes<4, 1>(V, [&](auto v) { hipLaunchKernelGGL((rough_roi_fill_kernel<decltype(v)::value>), dim3(lane_blocks(N, V)), dim3(256), 0, st, a); });
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}
