// Assessment front end: mask -> bounding box (K1/K2) and fused ROI resample + normalise (K3).
//
// Reference: AssessNet.forward/all2yxhw/get_ROI_grid (models/assessment.py:164-174,110-161,75-108) and
// Encoder.forward's (f-mean)/std (:47).  The reference copies the mask to the host and loops in numpy;
// here a coalesced scan reduces min/max per sample with wavefront reductions + one atomic per block, the
// float64 box arithmetic runs in a per-sample epilogue thread, and the 256x256x2 sampling grid (and the
// unused inverse grid) is never materialised: sample coordinates are recomputed from (y,x,h,w) per pixel.
// Both kernels are HBM-bound streaming/gather work; no LDS staging is needed (each input byte is read once).
#include <limits.h>

#include <algorithm>
#include <type_traits>

#include "common.h"
#include "front.h"

namespace ivosw {

__global__ void bbox_init_kernel(int32_t* __restrict__ box, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    box[b * 4 + 0] = INT_MAX;  // ymin
    box[b * 4 + 1] = -1;       // ymax
    box[b * 4 + 2] = INT_MAX;  // xmin
    box[b * 4 + 3] = -1;       // xmax
}

// grid (S, B): block s scans elements [s*chunk, (s+1)*chunk) of sample b's flat H*W plane.
__global__ __launch_bounds__(256) void bbox_scan_kernel(const float* __restrict__ tp, int b0, SampleMap sm, int H, int W, int chunk,
                                                        int vec_ok, int32_t* __restrict__ box) {
    const int b = blockIdx.y;            // box / yxhw rows are local to the launch; the sample map uses the global index
    const size_t plane = (size_t)H * W;
    const int bg = b0 + b;
    const float* p = tp + (size_t)(bg / sm.n_frames) * sm.stride_obj + (size_t)(bg % sm.n_frames) * sm.stride_frame;
    const size_t beg = (size_t)blockIdx.x * chunk;
    const size_t end = min(plane, beg + (size_t)chunk);
    int ymin = INT_MAX, ymax = -1, xmin = INT_MAX, xmax = -1;
    if (vec_ok) {  // plane % 4 == 0, chunk % 4 == 0, base 16-B aligned: 16 B per lane, fully coalesced
        // four 16-byte loads per lane in flight, (y, x) carried incrementally (no 64-bit division per load), and the per-element
        // work only for a float4 that holds a foreground pixel at all
        size_t i = beg + (size_t)threadIdx.x * 4;
        int y = (int)(i / W), x = (int)(i - (size_t)y * W);
        const int sy = 1024 / W, sx = 1024 % W;                      // one block stride = 1024 elements
        auto visit = [&](const float4& v, int yy, int xx) {
            if (fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)) > 0.5f) {   // tm = (tp > 0.5); mask >= 0.49 on {0,1} is the same set (assessment.py:165,115)
                const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (e[j] > 0.5f) {
                        ymin = min(ymin, yy); ymax = max(ymax, yy);
                        xmin = min(xmin, xx); xmax = max(xmax, xx);
                    }
                    if (++xx == W) { xx = 0; ++yy; }
                }
            }
        };
        auto step = [&](int& yy, int& xx) { yy += sy; xx += sx; if (xx >= W) { xx -= W; ++yy; } };
        for (; i + 3 * 1024 < end; i += 4 * 1024) {
            const float4 v0 = *reinterpret_cast<const float4*>(p + i), v1 = *reinterpret_cast<const float4*>(p + i + 1024);
            const float4 v2 = *reinterpret_cast<const float4*>(p + i + 2048), v3 = *reinterpret_cast<const float4*>(p + i + 3072);
            visit(v0, y, x); step(y, x);
            visit(v1, y, x); step(y, x);
            visit(v2, y, x); step(y, x);
            visit(v3, y, x); step(y, x);
        }
        for (; i < end; i += 1024) {
            visit(*reinterpret_cast<const float4*>(p + i), y, x);
            step(y, x);
        }
    } else {
        for (size_t i = beg + threadIdx.x; i < end; i += 256) {
            if (p[i] > 0.5f) {
                const int y = (int)(i / W), x = (int)(i - (size_t)y * W);
                ymin = min(ymin, y); ymax = max(ymax, y);
                xmin = min(xmin, x); xmax = max(xmax, x);
            }
        }
    }
    ymin = wave_min(ymin); ymax = wave_max(ymax);
    xmin = wave_min(xmin); xmax = wave_max(xmax);
    __shared__ int red[4][4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) { red[wave][0] = ymin; red[wave][1] = ymax; red[wave][2] = xmin; red[wave][3] = xmax; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) {
            ymin = min(ymin, red[w][0]); ymax = max(ymax, red[w][1]);
            xmin = min(xmin, red[w][2]); xmax = max(xmax, red[w][3]);
        }
        if (ymax >= 0) {
            atomicMin(&box[b * 4 + 0], ymin); atomicMax(&box[b * 4 + 1], ymax);
            atomicMin(&box[b * 4 + 2], xmin); atomicMax(&box[b * 4 + 3], xmax);
        }
    }
}

// integer box -> (y,x,h,w) fp32 with the reference's mixed int/float64 arithmetic (assessment.py:118-157)
__global__ void bbox_finalize_kernel(const int32_t* __restrict__ box, int B, int H, int W, float* __restrict__ yxhw) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int y0 = box[b * 4 + 0], y1 = box[b * 4 + 1], x0 = box[b * 4 + 2], x1 = box[b * 4 + 3];
    if (y1 < 0) { y0 = 0; y1 = H; x0 = 0; x1 = W; }  // empty mask: whole frame, H and W (not H-1, W-1)
    if (y1 - y0 < 128) { const int half = (int)((128.0 - (double)(y1 - y0)) / 2.0); y0 -= half; y1 += half; }
    if (x1 - x0 < 128) { const int half = (int)((128.0 - (double)(x1 - x0)) / 2.0); x0 -= half; x1 += half; }
    const double oh = (double)(y1 - y0 + 1), ow = (double)(x1 - x0 + 1);
    const double k = (1.5 - 1.0) / 2.0;
    const double fy0 = fmax(-5.0, (double)y0 - k * oh), fy1 = fmin((double)H + 5.0, (double)y1 + k * oh);
    const double fx0 = fmax(-5.0, (double)x0 - k * ow), fx1 = fmin((double)W + 5.0, (double)x1 + k * ow);
    yxhw[b * 4 + 0] = (float)((fy1 + fy0) / 2.0);
    yxhw[b * 4 + 1] = (float)((fx1 + fx0) / 2.0);
    yxhw[b * 4 + 2] = (float)(fy1 - fy0 + 1.0);
    yxhw[b * 4 + 3] = (float)(fx1 - fx0 + 1.0);
}

void launch_mask_bbox(const float* tp, int b0, int B, int H, int W, const SampleMap& sm, float* yxhw, int32_t* scratch, hipStream_t st) {
    hipLaunchKernelGGL(bbox_init_kernel, dim3((B + 63) / 64), dim3(64), 0, st, scratch, B);
    const size_t plane = (size_t)H * W;
    int S = (int)max((size_t)1, min((size_t)64, (size_t)2048 / (size_t)B));
    size_t chunk = (plane + S - 1) / S;
    chunk = (chunk + 1023) / 1024 * 1024;  // multiple of 4 (and of the 1024-element block stride)
    S = (int)((plane + chunk - 1) / chunk);
    const int vec_ok = (plane % 4 == 0) && ((reinterpret_cast<uintptr_t>(tp) & 15) == 0) && sm.stride_frame % 4 == 0 && sm.stride_obj % 4 == 0;
    hipLaunchKernelGGL(bbox_scan_kernel, dim3(S, B), dim3(256), 0, st, tp, b0, sm, H, W, (int)chunk, vec_ok, scratch);
    hipLaunchKernelGGL(bbox_finalize_kernel, dim3((B + 63) / 64), dim3(64), 0, st, scratch, B, H, W, yxhw);
}

// ---------------------------------------------------------------- ROI sampler
__device__ __forceinline__ float lin_m1_1(int j, int n) {  // torch.linspace(-1,1,n)[j] in fp32
    const float step = 2.0f / (float)(n - 1);
    return (j < n / 2) ? __fadd_rn(-1.0f, __fmul_rn((float)j, step)) : __fsub_rn(1.0f, __fmul_rn((float)(n - 1 - j), step));
}

// grid B * 256 / ROI_R, block 256: thread j owns output column j of ROI_R consecutive output rows of one sample,
// roi[b][i][j][0..3] = (R,G,B normalised, P).  Everything that depends on the sample and the column only (theta, the source
// x, its two taps, their weights and validity) is computed once per thread instead of once per output pixel, and the rows are
// processed two at a time (32 gathers in flight): one output pixel per thread ran ~250 vector instructions for 16 loads and
// 8 B of output, VALU-bound at 180 us per 256 frames.  Per pixel the arithmetic and its order are unchanged.
constexpr int ROI_R = 8;
// two neighbouring fp32 pixels with one 8-byte load from a 4-byte-aligned address (global memory takes unaligned dwordx2)
struct __attribute__((packed, aligned(4))) PairF32 { float x, y; };
__device__ __forceinline__ float2 ld_pair(const float* p) {
    const PairF32 v = *reinterpret_cast<const PairF32*>(p);
    return make_float2(v.x, v.y);
}

template <typename T>
__global__ __launch_bounds__(256) void roi_sample_kernel(const float* __restrict__ tf, const float* __restrict__ tp,
                                                         const float* __restrict__ yxhw, int b0, SampleMap sm, int H, int W, RoiNorm nrm,
                                                         T* __restrict__ roi) {
    constexpr int GPS = 256 / ROI_R;                               // row groups per sample
    const int b = blockIdx.x / GPS, i0 = (blockIdx.x % GPS) * ROI_R, j = threadIdx.x;     // yxhw / roi rows are local to the launch
    const int bg = b0 + b, fr = bg % sm.n_frames;
    const float ry = yxhw[b * 4 + 0], rx = yxhw[b * 4 + 1], rh = yxhw[b * 4 + 2], rw = yxhw[b * 4 + 3];
    // get_ROI_grid (assessment.py:79-92), fp32, same operation order as the reference.  NOTE: HIP's __fmul_rn / __fadd_rn
    // are plain operators inside header functions, so hipcc still contracts mul+add pairs into FMAs here (as the GEMM
    // behind torch's affine_grid does); the golden-slice tests bound the resulting sample-point error (<= 3e-4 on the
    // ROI tiles, 8e-7 on the fp32 scores).  seg_epilogue.hip shows the pragma that really switches contraction off.
    const float ymin = __fsub_rn(ry, rh / 2.0f), ymax = __fadd_rn(ry, rh / 2.0f);
    const float xmin = __fsub_rn(rx, rw / 2.0f), xmax = __fadd_rn(rx, rw / 2.0f);
    const float wm = (float)(W - 1), hm = (float)(H - 1);
    const float t00 = __fsub_rn(xmax, xmin) / wm, t02 = __fsub_rn(__fadd_rn(xmin, xmax), wm) / wm;
    const float t11 = __fsub_rn(ymax, ymin) / hm, t12 = __fsub_rn(__fadd_rn(ymin, ymax), hm) / hm;
    // affine_grid + grid_sample(align_corners=True): pixel = ((g + 1) / 2) * (size - 1)
    const float gx = __fadd_rn(__fmul_rn(lin_m1_1(j, 256), t00), t02);
    const float sx = __fmul_rn(__fmul_rn(__fadd_rn(gx, 1.0f), 0.5f), wm);
    const float x0f = floorf(sx);
    const int x0 = (int)x0f;
    const float wx1 = __fsub_rn(sx, x0f), wx0 = __fsub_rn(__fadd_rn(x0f, 1.0f), sx);
    const bool vx0 = x0 >= 0 && x0 < W, vx1 = x0 + 1 >= 0 && x0 + 1 < W;
    // All 16 taps are loaded unconditionally from clamped addresses and out-of-range taps get weight 0 (zero padding:
    // they contribute +0, which leaves the fp32 sum bit-identical): predicated loads made hipcc branch around every
    // load and wait for it, 16 dependent round trips per pixel.
    // The two x taps of a row are neighbours in memory: ONE 8-byte load at xb = clamp(x0, 0, W - 2) brings both (the texture-
    // cache access count, ~19 per gathered dword load of a wave, bounds this kernel - rocprofv3 TCP_TOTAL_CACHE_ACCESSES).
    // At the frame's edges one of the taps has weight 0 and takes whichever in-range pixel the pair holds.
    const int xb = min(max(x0, 0), W - 2);
    const bool t0_hi = x0 >= W - 1, t1_lo = x0 < 0;                // tap0 = pair.y at the right edge, tap1 = pair.x at the left edge
    const size_t plane = (size_t)H * W;
    const float* src[4];
#pragma unroll
    for (int c = 0; c < 3; ++c) src[c] = tf + ((size_t)fr * 3 + c) * plane;
    src[3] = tp + (size_t)(bg / sm.n_frames) * sm.stride_obj + (size_t)fr * sm.stride_frame;
    float mu[3], sd[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {      // (f - mean) / std after the zero pad (assessment.py:47)
        mu[c] = nrm.dev ? nrm.dev[c] : nrm.mean[c];
        sd[c] = nrm.dev ? nrm.dev[3 + c] : nrm.std[c];
    }
    T* dst = roi + (((size_t)b * 256 + i0) * 256 + j) * 4;
#pragma unroll 1
    for (int r0 = 0; r0 < ROI_R; r0 += 2) {
        float v[2][4][4], k[2][4];
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
            const int i = i0 + r0 + rr;
            const float gy = __fadd_rn(__fmul_rn(lin_m1_1(i, 256), t11), t12);
            const float sy = __fmul_rn(__fmul_rn(__fadd_rn(gy, 1.0f), 0.5f), hm);
            const float y0f = floorf(sy);
            const int y0 = (int)y0f;
            const float wy1 = __fsub_rn(sy, y0f), wy0 = __fsub_rn(__fadd_rn(y0f, 1.0f), sy);
            const bool vy0 = y0 >= 0 && y0 < H, vy1 = y0 + 1 >= 0 && y0 + 1 < H;
            const int yc0 = min(max(y0, 0), H - 1), yc1 = min(max(y0 + 1, 0), H - 1);
            const int o0 = yc0 * W + xb, o1 = yc1 * W + xb;        // < H * W <= INT_MAX (checked by the host)
            const float w_nw = __fmul_rn(wx0, wy0), w_ne = __fmul_rn(wx1, wy0), w_sw = __fmul_rn(wx0, wy1), w_se = __fmul_rn(wx1, wy1);
            k[rr][0] = (vy0 && vx0) ? w_nw : 0.f; k[rr][1] = (vy0 && vx1) ? w_ne : 0.f;
            k[rr][2] = (vy1 && vx0) ? w_sw : 0.f; k[rr][3] = (vy1 && vx1) ? w_se : 0.f;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float2 p0 = ld_pair(src[c] + o0), p1 = ld_pair(src[c] + o1);
                v[rr][c][0] = t0_hi ? p0.y : p0.x; v[rr][c][1] = t1_lo ? p0.x : p0.y;
                v[rr][c][2] = t0_hi ? p1.y : p1.x; v[rr][c][3] = t1_lo ? p1.x : p1.y;
            }
        }
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
            float out[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float acc = 0.f;
                acc = __fadd_rn(acc, __fmul_rn(v[rr][c][0], k[rr][0]));
                acc = __fadd_rn(acc, __fmul_rn(v[rr][c][1], k[rr][1]));
                acc = __fadd_rn(acc, __fmul_rn(v[rr][c][2], k[rr][2]));
                acc = __fadd_rn(acc, __fmul_rn(v[rr][c][3], k[rr][3]));
                if (c < 3) acc = __fsub_rn(acc, mu[c]) / sd[c];
                out[c] = acc;
            }
            T* d = dst + (size_t)(r0 + rr) * 256 * 4;
            if constexpr (sizeof(T) == 4) {
                *reinterpret_cast<float4*>(d) = make_float4(out[0], out[1], out[2], out[3]);
            } else {
                *reinterpret_cast<uint2*>(d) = make_uint2(pack2_bf16(out[0], out[1]), pack2_bf16(out[2], out[3]));
            }
        }
    }
}

// ---------------------------------------------------------------- 8-bit frames (RGBX8: uint8 [n,H,W,4], bytes R, G, B, 0)
// byte k of w as float32(v) / float32(255), correctly rounded - what np.float32(v) / 255. and torch's uint8 -> float() / 255 give on the host.
// Division by the constant as a reciprocal product plus one Newton step on the exact residual (q = v r, e = v - 255 q, q + e r: the
// tail of the hardware's own fp32 division, 3 VALU instructions instead of ~11 and no denormal-mode switch); that it rounds like the
// division for every one of the 256 bytes is checked in exact arithmetic by tests/test_frames_u8_option.py and on the device by
// tests/test_gpu_frames_u8.py.  The byte extraction and the conversion are one instruction (v_cvt_f32_ubyte<k>).
__device__ __forceinline__ float u8_unit(uint32_t w, int k) {
    const float v = (float)((w >> (8 * k)) & 0xffu);
    constexpr float r = 1.0f / 255.0f;
    const float q = v * r;
    const float e = __builtin_fmaf(-q, 255.0f, v);
    return __builtin_fmaf(e, r, q);
}

// grid ceil(max(groups, tail) / 256), block 256: a byte-shuffling copy from a decoder layout to RGBX8, once per video.  The n frames are
// one flat run of P = n*H*W pixels.  Fast path (vec: 4-byte aligned source, 16-byte aligned destination, and for CHW planes of a multiple
// of 4 pixels): thread g turns three dword loads (HWC: 12 consecutive bytes; CHW: 4 bytes of each plane) into ONE 16-byte store of four
// pixels; the P % 4 pixels behind the last group - or, without vec, every pixel - take the scalar path (3 byte loads, one dword store).
__global__ __launch_bounds__(256) void frames_pack_u8_kernel(const uint8_t* __restrict__ src, int layout, int vec, size_t P, size_t plane,
                                                             uint8_t* __restrict__ dst) {
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t groups = vec ? P / 4 : 0;
    if (g < groups) {
        uint4 o;
        if (layout == IVOSW_U8_HWC3) {
            const uint32_t* s = reinterpret_cast<const uint32_t*>(src + g * 12);
            const uint32_t w0 = s[0], w1 = s[1], w2 = s[2];        // r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
            o.x = w0 & 0xffffffu;
            o.y = (w0 >> 24) | ((w1 & 0xffffu) << 8);
            o.z = (w1 >> 16) | ((w2 & 0xffu) << 16);
            o.w = w2 >> 8;
        } else {
            const size_t q = g * 4, f = q / plane, i = q - f * plane;      // plane % 4 == 0: the group lies inside one frame
            const uint8_t* s = src + f * 3 * plane + i;
            const uint32_t r = *reinterpret_cast<const uint32_t*>(s), gg = *reinterpret_cast<const uint32_t*>(s + plane),
                           b = *reinterpret_cast<const uint32_t*>(s + 2 * plane);
            o.x = (r & 0xffu) | ((gg & 0xffu) << 8) | ((b & 0xffu) << 16);
            o.y = ((r >> 8) & 0xffu) | (((gg >> 8) & 0xffu) << 8) | (((b >> 8) & 0xffu) << 16);
            o.z = ((r >> 16) & 0xffu) | (((gg >> 16) & 0xffu) << 8) | (((b >> 16) & 0xffu) << 16);
            o.w = (r >> 24) | ((gg >> 24) << 8) | ((b >> 24) << 16);
        }
        *reinterpret_cast<uint4*>(dst + g * 16) = o;
    }
    const size_t q = groups * 4 + g;
    if (q < P) {
        uint32_t r, gg, b;
        if (layout == IVOSW_U8_HWC3) {
            r = src[q * 3]; gg = src[q * 3 + 1]; b = src[q * 3 + 2];
        } else {
            const size_t f = q / plane, i = q - f * plane;
            const uint8_t* s = src + f * 3 * plane + i;
            r = s[0]; gg = s[plane]; b = s[2 * plane];
        }
        *reinterpret_cast<uint32_t*>(dst + q * 4) = r | (gg << 8) | (b << 16);
    }
}

// two neighbouring RGBX8 pixels with one 8-byte load from a 4-byte-aligned address
struct __attribute__((packed, aligned(4))) PairU32 { uint32_t x, y; };
__device__ __forceinline__ uint2 ld_pair_u32(const uint8_t* p) {
    const PairU32 v = *reinterpret_cast<const PairU32*>(p);
    return make_uint2(v.x, v.y);
}

// roi_sample_kernel with the colours read from RGBX8 frames: the same geometry (thread = output column, ROI_R rows per workgroup, two
// rows in flight), theta, taps, weights, zero padding, products, sums and (f - mean) / std, in the same order.  The three colour pair
// loads of a source row become ONE 8-byte load at 4 * (yc * W + xb) that holds both x taps of all colours (4 pair loads per output
// pixel with the mask's instead of 8); the edge selection (t0_hi / t1_lo) picks a whole pixel word before its bytes are converted.
// The mask plane stays fp32 with its own pair load.  Results are bit-identical to roi_sample_kernel on float32(u8) / 255.
template <typename T>
__global__ __launch_bounds__(256) void roi_sample_u8_kernel(const uint8_t* __restrict__ rgbx, const float* __restrict__ tp,
                                                            const float* __restrict__ yxhw, int b0, SampleMap sm, int H, int W, RoiNorm nrm,
                                                            T* __restrict__ roi) {
    constexpr int GPS = 256 / ROI_R;
    const int b = blockIdx.x / GPS, i0 = (blockIdx.x % GPS) * ROI_R, j = threadIdx.x;
    const int bg = b0 + b, fr = bg % sm.n_frames;
    const float ry = yxhw[b * 4 + 0], rx = yxhw[b * 4 + 1], rh = yxhw[b * 4 + 2], rw = yxhw[b * 4 + 3];
    const float ymin = __fsub_rn(ry, rh / 2.0f), ymax = __fadd_rn(ry, rh / 2.0f);
    const float xmin = __fsub_rn(rx, rw / 2.0f), xmax = __fadd_rn(rx, rw / 2.0f);
    const float wm = (float)(W - 1), hm = (float)(H - 1);
    const float t00 = __fsub_rn(xmax, xmin) / wm, t02 = __fsub_rn(__fadd_rn(xmin, xmax), wm) / wm;
    const float t11 = __fsub_rn(ymax, ymin) / hm, t12 = __fsub_rn(__fadd_rn(ymin, ymax), hm) / hm;
    const float gx = __fadd_rn(__fmul_rn(lin_m1_1(j, 256), t00), t02);
    const float sx = __fmul_rn(__fmul_rn(__fadd_rn(gx, 1.0f), 0.5f), wm);
    const float x0f = floorf(sx);
    const int x0 = (int)x0f;
    const float wx1 = __fsub_rn(sx, x0f), wx0 = __fsub_rn(__fadd_rn(x0f, 1.0f), sx);
    const bool vx0 = x0 >= 0 && x0 < W, vx1 = x0 + 1 >= 0 && x0 + 1 < W;
    const int xb = min(max(x0, 0), W - 2);
    const bool t0_hi = x0 >= W - 1, t1_lo = x0 < 0;
    const uint8_t* srcf = rgbx + (size_t)fr * H * W * 4;
    const float* srcp = tp + (size_t)(bg / sm.n_frames) * sm.stride_obj + (size_t)fr * sm.stride_frame;
    float mu[3], sd[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        mu[c] = nrm.dev ? nrm.dev[c] : nrm.mean[c];
        sd[c] = nrm.dev ? nrm.dev[3 + c] : nrm.std[c];
    }
    T* dst = roi + (((size_t)b * 256 + i0) * 256 + j) * 4;
#pragma unroll 1
    for (int r0 = 0; r0 < ROI_R; r0 += 2) {
        uint32_t px[2][4];                                         // the four taps' pixel words: nw, ne, sw, se
        float m[2][4], k[2][4];
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
            const int i = i0 + r0 + rr;
            const float gy = __fadd_rn(__fmul_rn(lin_m1_1(i, 256), t11), t12);
            const float sy = __fmul_rn(__fmul_rn(__fadd_rn(gy, 1.0f), 0.5f), hm);
            const float y0f = floorf(sy);
            const int y0 = (int)y0f;
            const float wy1 = __fsub_rn(sy, y0f), wy0 = __fsub_rn(__fadd_rn(y0f, 1.0f), sy);
            const bool vy0 = y0 >= 0 && y0 < H, vy1 = y0 + 1 >= 0 && y0 + 1 < H;
            const int yc0 = min(max(y0, 0), H - 1), yc1 = min(max(y0 + 1, 0), H - 1);
            const int o0 = yc0 * W + xb, o1 = yc1 * W + xb;        // pixels o0, o0 + 1 < H * W <= INT_MAX (checked by the host)
            const float w_nw = __fmul_rn(wx0, wy0), w_ne = __fmul_rn(wx1, wy0), w_sw = __fmul_rn(wx0, wy1), w_se = __fmul_rn(wx1, wy1);
            k[rr][0] = (vy0 && vx0) ? w_nw : 0.f; k[rr][1] = (vy0 && vx1) ? w_ne : 0.f;
            k[rr][2] = (vy1 && vx0) ? w_sw : 0.f; k[rr][3] = (vy1 && vx1) ? w_se : 0.f;
            const uint2 c0 = ld_pair_u32(srcf + (size_t)o0 * 4), c1 = ld_pair_u32(srcf + (size_t)o1 * 4);
            const float2 p0 = ld_pair(srcp + o0), p1 = ld_pair(srcp + o1);
            px[rr][0] = t0_hi ? c0.y : c0.x; px[rr][1] = t1_lo ? c0.x : c0.y;
            px[rr][2] = t0_hi ? c1.y : c1.x; px[rr][3] = t1_lo ? c1.x : c1.y;
            m[rr][0] = t0_hi ? p0.y : p0.x; m[rr][1] = t1_lo ? p0.x : p0.y;
            m[rr][2] = t0_hi ? p1.y : p1.x; m[rr][3] = t1_lo ? p1.x : p1.y;
        }
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
            float out[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float v[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) v[t] = c < 3 ? u8_unit(px[rr][t], c) : m[rr][t];
                // roi_sample_kernel's four product-sums compile to a chain of four FMAs in both instantiations (see the NOTE there:
                // __fmul_rn / __fadd_rn contract).  Written with the same operators here, hipcc packed the products of two channels
                // (v_pk_mul_f32) in the bf16 instantiation and added them unfused, one rounding more per tap than the float kernel.
                // The explicit FMAs pin the float kernel's arithmetic; tests/test_gpu_frames_u8.py holds the two bit-identical.
                float acc = 0.f;
                acc = __builtin_fmaf(v[0], k[rr][0], acc);
                acc = __builtin_fmaf(v[1], k[rr][1], acc);
                acc = __builtin_fmaf(v[2], k[rr][2], acc);
                acc = __builtin_fmaf(v[3], k[rr][3], acc);
                if (c < 3) acc = __fsub_rn(acc, mu[c]) / sd[c];
                out[c] = acc;
            }
            T* d = dst + (size_t)(r0 + rr) * 256 * 4;
            if constexpr (sizeof(T) == 4) {
                *reinterpret_cast<float4*>(d) = make_float4(out[0], out[1], out[2], out[3]);
            } else {
                *reinterpret_cast<uint2*>(d) = make_uint2(pack2_bf16(out[0], out[1]), pack2_bf16(out[2], out[3]));
            }
        }
    }
}

void launch_roi_sample(const FrameSrc& fs, const float* tp, const float* yxhw, int b0, int B, int H, int W, int dtype,
                       const SampleMap& sm, const RoiNorm& nrm, void* roi, hipStream_t st) {
    const dim3 grid(B * (256 / ROI_R)), block(256);
    if (fs.u8) {
        const uint8_t* rgbx = static_cast<const uint8_t*>(fs.p);
        if (dtype != IVOSW_BF16)
            hipLaunchKernelGGL(roi_sample_u8_kernel<float>, grid, block, 0, st, rgbx, tp, yxhw, b0, sm, H, W, nrm, static_cast<float*>(roi));
        else
            hipLaunchKernelGGL(roi_sample_u8_kernel<bf16_t>, grid, block, 0, st, rgbx, tp, yxhw, b0, sm, H, W, nrm, static_cast<bf16_t*>(roi));
        return;
    }
    const float* tf = static_cast<const float*>(fs.p);
    if (dtype != IVOSW_BF16)
        hipLaunchKernelGGL(roi_sample_kernel<float>, grid, block, 0, st, tf, tp, yxhw, b0, sm, H, W, nrm, static_cast<float*>(roi));
    else
        hipLaunchKernelGGL(roi_sample_kernel<bf16_t>, grid, block, 0, st, tf, tp, yxhw, b0, sm, H, W, nrm, static_cast<bf16_t*>(roi));
}

// ---------------------------------------------------------------- several videos in one launch (front.h: VideoTable)
// The video of unit u: how many videos start at or before u, minus one.  No loop-carried load: the compares run on two scalar loads.
__device__ __forceinline__ int video_of_unit(const VideoTable& vt, int u) {
    int v = 0;
#pragma unroll
    for (int i = 1; i < IVOSW_MAX_VIDEOS; ++i) v += (u >= vt.first[i]) ? 1 : 0;
    return v;
}

// Which unit row b of a launch works on: the b-th unit of a range (unit = b0 + b: what the *_videos entries launch), or the b-th entry of
// a unit list (unit = ids[b0 + b]: the *_units entries; ids is a device array).  The kernels below take either one as their `Units`
// template parameter, so both variants come from one body.  A list entry outside [0, units) is never turned into an address: valid()
// is false and the row is skipped (the box stays empty, the tile is zero).
struct UnitRange {
    int b0;
    __device__ __forceinline__ int at(int b) const { return b0 + b; }
    __device__ __forceinline__ bool valid(int, int) const { return true; }
};
struct UnitList {
    const int32_t* ids;
    int b0;
    __device__ __forceinline__ int at(int b) const { return ids[b0 + b]; }
    __device__ __forceinline__ bool valid(int u, int units) const { return (unsigned)u < (unsigned)units; }
};

// bbox_scan_kernel over the units [b0, b0 + gridDim.y) of a video table.  grid (S, B) with S sized for the LARGEST plane of the range:
// a workgroup whose chunk lies behind its own video's plane leaves before the barrier (the whole workgroup: the test is uniform).
// Integer min / max: the box does not depend on how the plane is cut into chunks.
//
// Lab (compile time, like Units): the table holds at least one label video (front.h: VideoDesc::lab).  The choice is then made per video,
// uniform per workgroup; a float-only table runs the Lab = false instantiation, whose code is what it was before label maps existed.
// A label video's unit (frame, obj) scans the frame's uint8 map for the value obj + 1 - `tp > 0.5f` on the one-hot plane is that test.
// Vector path: one 16-byte load = 16 pixels per lane (block stride 4096 pixels; chunk % 1024 == 0 and plane % 16 == 0 keep every vector
// inside the chunk), a vector without a byte equal to the label is skipped by a zero-byte test on the four words XOR the label.

// any byte of w equal to the byte replicated in `rep`?  (the classic zero-byte test on w ^ rep: exact as a yes / no answer)
__device__ __forceinline__ uint32_t has_byte(uint32_t w, uint32_t rep) {
    const uint32_t x = w ^ rep;
    return (x - 0x01010101u) & ~x & 0x80808080u;
}

template <typename Units, bool Lab>
__global__ __launch_bounds__(256) void bbox_scan_multi_kernel(const VideoTable vt, Units un, int chunk, int32_t* __restrict__ box) {
    const int b = blockIdx.y;
    const int u = un.at(b);
    if (!un.valid(u, vt.units)) return;                            // (uniform: the whole workgroup leaves)
    const int vi = video_of_unit(vt, u);
    const VideoDesc& d = vt.v[vi];
    const int W = d.W;
    const size_t plane = (size_t)d.H * W;
    const size_t beg = (size_t)blockIdx.x * chunk;
    if (beg >= plane) return;
    const int lu = u - vt.first[vi], nf = d.n_frames;
    const float* p = d.masks + (size_t)(lu / nf) * d.stride_obj + (size_t)(lu % nf) * d.stride_frame;
    const size_t end = min(plane, beg + (size_t)chunk);
    int ymin = INT_MAX, ymax = -1, xmin = INT_MAX, xmax = -1;
    bool is_lab = false;
    if constexpr (Lab) is_lab = d.lab != nullptr;                  // (uniform)
    if (Lab && is_lab) {
        const uint8_t* q = d.lab + (size_t)(lu % nf) * d.lab_stride;
        const uint32_t lab = (uint32_t)(lu / nf) + 1u;             // n_obj <= 255 on a label video (checked by the host)
        if (d.vec_ok) {  // plane % 16 == 0, map base and frame stride 16-B aligned
            const uint32_t rep = lab * 0x01010101u;
            size_t i = beg + (size_t)threadIdx.x * 16;
            int y = (int)(i / W), x = (int)(i - (size_t)y * W);
            const int sy = 4096 / W, sx = 4096 % W;                // one block stride = 4096 pixels
            auto visit = [&](const uint4& v, int yy, int xx) {
                if (has_byte(v.x, rep) | has_byte(v.y, rep) | has_byte(v.z, rep) | has_byte(v.w, rep)) {
                    const uint32_t e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int j = 0; j < 16; ++j) {
                        if (((e[j >> 2] >> (8 * (j & 3))) & 0xffu) == lab) {
                            ymin = min(ymin, yy); ymax = max(ymax, yy);
                            xmin = min(xmin, xx); xmax = max(xmax, xx);
                        }
                        if (++xx == W) { xx = 0; ++yy; }
                    }
                }
            };
            auto step = [&](int& yy, int& xx) { yy += sy; xx += sx; if (xx >= W) { xx -= W; ++yy; } };
            for (; i + 3 * 4096 < end; i += 4 * 4096) {
                const uint4 v0 = *reinterpret_cast<const uint4*>(q + i), v1 = *reinterpret_cast<const uint4*>(q + i + 4096);
                const uint4 v2 = *reinterpret_cast<const uint4*>(q + i + 8192), v3 = *reinterpret_cast<const uint4*>(q + i + 12288);
                visit(v0, y, x); step(y, x);
                visit(v1, y, x); step(y, x);
                visit(v2, y, x); step(y, x);
                visit(v3, y, x); step(y, x);
            }
            for (; i < end; i += 4096) {
                visit(*reinterpret_cast<const uint4*>(q + i), y, x);
                step(y, x);
            }
        } else {
            for (size_t i = beg + threadIdx.x; i < end; i += 256) {
                if (q[i] == lab) {
                    const int y = (int)(i / W), x = (int)(i - (size_t)y * W);
                    ymin = min(ymin, y); ymax = max(ymax, y);
                    xmin = min(xmin, x); xmax = max(xmax, x);
                }
            }
        }
    } else if (d.vec_ok) {  // this video: plane % 4 == 0, base and strides 16-B aligned (chunk % 1024 == 0 for every video)
        size_t i = beg + (size_t)threadIdx.x * 4;
        int y = (int)(i / W), x = (int)(i - (size_t)y * W);
        const int sy = 1024 / W, sx = 1024 % W;
        auto visit = [&](const float4& v, int yy, int xx) {
            if (fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)) > 0.5f) {
                const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (e[j] > 0.5f) {
                        ymin = min(ymin, yy); ymax = max(ymax, yy);
                        xmin = min(xmin, xx); xmax = max(xmax, xx);
                    }
                    if (++xx == W) { xx = 0; ++yy; }
                }
            }
        };
        auto step = [&](int& yy, int& xx) { yy += sy; xx += sx; if (xx >= W) { xx -= W; ++yy; } };
        for (; i + 3 * 1024 < end; i += 4 * 1024) {
            const float4 v0 = *reinterpret_cast<const float4*>(p + i), v1 = *reinterpret_cast<const float4*>(p + i + 1024);
            const float4 v2 = *reinterpret_cast<const float4*>(p + i + 2048), v3 = *reinterpret_cast<const float4*>(p + i + 3072);
            visit(v0, y, x); step(y, x);
            visit(v1, y, x); step(y, x);
            visit(v2, y, x); step(y, x);
            visit(v3, y, x); step(y, x);
        }
        for (; i < end; i += 1024) {
            visit(*reinterpret_cast<const float4*>(p + i), y, x);
            step(y, x);
        }
    } else {
        for (size_t i = beg + threadIdx.x; i < end; i += 256) {
            if (p[i] > 0.5f) {
                const int y = (int)(i / W), x = (int)(i - (size_t)y * W);
                ymin = min(ymin, y); ymax = max(ymax, y);
                xmin = min(xmin, x); xmax = max(xmax, x);
            }
        }
    }
    ymin = wave_min(ymin); ymax = wave_max(ymax);
    xmin = wave_min(xmin); xmax = wave_max(xmax);
    __shared__ int red[4][4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) { red[wave][0] = ymin; red[wave][1] = ymax; red[wave][2] = xmin; red[wave][3] = xmax; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) {
            ymin = min(ymin, red[w][0]); ymax = max(ymax, red[w][1]);
            xmin = min(xmin, red[w][2]); xmax = max(xmax, red[w][3]);
        }
        if (ymax >= 0) {
            atomicMin(&box[b * 4 + 0], ymin); atomicMax(&box[b * 4 + 1], ymax);
            atomicMin(&box[b * 4 + 2], xmin); atomicMax(&box[b * 4 + 3], xmax);
        }
    }
}

// bbox_finalize_kernel with the H, W of the unit's own video (a per-thread lookup: neighbouring units may belong to different videos)
template <typename Units>
__global__ void bbox_finalize_multi_kernel(const int32_t* __restrict__ box, const VideoTable vt, Units un, int B, float* __restrict__ yxhw) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int u = un.at(b);
    if (!un.valid(u, vt.units)) {
        yxhw[b * 4 + 0] = 0.f; yxhw[b * 4 + 1] = 0.f; yxhw[b * 4 + 2] = 0.f; yxhw[b * 4 + 3] = 0.f;
        return;
    }
    const int vi = video_of_unit(vt, u);
    const int H = vt.v[vi].H, W = vt.v[vi].W;
    int y0 = box[b * 4 + 0], y1 = box[b * 4 + 1], x0 = box[b * 4 + 2], x1 = box[b * 4 + 3];
    if (y1 < 0) { y0 = 0; y1 = H; x0 = 0; x1 = W; }
    if (y1 - y0 < 128) { const int half = (int)((128.0 - (double)(y1 - y0)) / 2.0); y0 -= half; y1 += half; }
    if (x1 - x0 < 128) { const int half = (int)((128.0 - (double)(x1 - x0)) / 2.0); x0 -= half; x1 += half; }
    const double oh = (double)(y1 - y0 + 1), ow = (double)(x1 - x0 + 1);
    const double k = (1.5 - 1.0) / 2.0;
    const double fy0 = fmax(-5.0, (double)y0 - k * oh), fy1 = fmin((double)H + 5.0, (double)y1 + k * oh);
    const double fx0 = fmax(-5.0, (double)x0 - k * ow), fx1 = fmin((double)W + 5.0, (double)x1 + k * ow);
    yxhw[b * 4 + 0] = (float)((fy1 + fy0) / 2.0);
    yxhw[b * 4 + 1] = (float)((fx1 + fx0) / 2.0);
    yxhw[b * 4 + 2] = (float)(fy1 - fy0 + 1.0);
    yxhw[b * 4 + 3] = (float)(fx1 - fx0 + 1.0);
}

void launch_mask_bbox_multi(const VideoTable& vt, int b0, int B, float* yxhw, int32_t* scratch, hipStream_t st, const int32_t* ids) {
    hipLaunchKernelGGL(bbox_init_kernel, dim3((B + 63) / 64), dim3(64), 0, st, scratch, B);
    size_t plane = 0;                                              // the largest plane among the videos of [b0, b0 + B)
    for (int i = 0; i < vt.n; ++i) {                               // (a list: of all videos - the host does not know which ones it names)
        const long lo = vt.first[i], hi = lo + (long)vt.v[i].n_frames * vt.v[i].n_obj;
        if (ids || (hi > b0 && lo < (long)b0 + B)) plane = max(plane, (size_t)vt.v[i].H * vt.v[i].W);
    }
    int S = (int)max((size_t)1, min((size_t)64, (size_t)2048 / (size_t)B));
    size_t chunk = (plane + S - 1) / S;
    chunk = (chunk + 1023) / 1024 * 1024;
    S = (int)((plane + chunk - 1) / chunk);
    if (ids) {
        if (vt.any_lab)
            hipLaunchKernelGGL((bbox_scan_multi_kernel<UnitList, true>), dim3(S, B), dim3(256), 0, st, vt, UnitList{ids, b0}, (int)chunk, scratch);
        else
            hipLaunchKernelGGL((bbox_scan_multi_kernel<UnitList, false>), dim3(S, B), dim3(256), 0, st, vt, UnitList{ids, b0}, (int)chunk, scratch);
        hipLaunchKernelGGL(bbox_finalize_multi_kernel<UnitList>, dim3((B + 63) / 64), dim3(64), 0, st, scratch, vt, UnitList{ids, b0}, B, yxhw);
        return;
    }
    if (vt.any_lab)
        hipLaunchKernelGGL((bbox_scan_multi_kernel<UnitRange, true>), dim3(S, B), dim3(256), 0, st, vt, UnitRange{b0}, (int)chunk, scratch);
    else
        hipLaunchKernelGGL((bbox_scan_multi_kernel<UnitRange, false>), dim3(S, B), dim3(256), 0, st, vt, UnitRange{b0}, (int)chunk, scratch);
    hipLaunchKernelGGL(bbox_finalize_multi_kernel<UnitRange>, dim3((B + 63) / 64), dim3(64), 0, st, scratch, vt, UnitRange{b0}, B, yxhw);
}

// One unit's ROI_R output rows: the body of roi_sample_kernel (U8 = false) / roi_sample_u8_kernel (U8 = true) behind their pointer
// setup - the same theta, taps, weights, clamped pair loads, zero weights, product-sums and (f - mean) / std, in the same order.  The
// four product-sums are written as the FMA chain that both single-video kernels compile to (see roi_sample_u8_kernel).
// Lab = true: the P channel comes from a label map (srcp = the frame's uint8 plane, labv = the unit's label): its four taps are BYTE
// loads at the same clamped offsets o0, o0 + 1, o1, o1 + 1 (no 2-byte load: o0 may be odd), each turned into the one-hot plane's value
// (byte == labv) ? 1.0f : 0.0f before the same tap selection, weights and FMA chain - bit-identical to the float path on that plane.
template <typename T, bool U8, bool Lab = false>
__device__ __forceinline__ void roi_unit_rows(const void* __restrict__ frame, const void* __restrict__ srcp, const float* __restrict__ yx,
                                              int H, int W, const RoiNorm& nrm, int i0, int j, T* __restrict__ dst, uint32_t labv = 0u) {
    const float ry = yx[0], rx = yx[1], rh = yx[2], rw = yx[3];
    const float ymin = __fsub_rn(ry, rh / 2.0f), ymax = __fadd_rn(ry, rh / 2.0f);
    const float xmin = __fsub_rn(rx, rw / 2.0f), xmax = __fadd_rn(rx, rw / 2.0f);
    const float wm = (float)(W - 1), hm = (float)(H - 1);
    const float t00 = __fsub_rn(xmax, xmin) / wm, t02 = __fsub_rn(__fadd_rn(xmin, xmax), wm) / wm;
    const float t11 = __fsub_rn(ymax, ymin) / hm, t12 = __fsub_rn(__fadd_rn(ymin, ymax), hm) / hm;
    const float gx = __fadd_rn(__fmul_rn(lin_m1_1(j, 256), t00), t02);
    const float sx = __fmul_rn(__fmul_rn(__fadd_rn(gx, 1.0f), 0.5f), wm);
    const float x0f = floorf(sx);
    const int x0 = (int)x0f;
    const float wx1 = __fsub_rn(sx, x0f), wx0 = __fsub_rn(__fadd_rn(x0f, 1.0f), sx);
    const bool vx0 = x0 >= 0 && x0 < W, vx1 = x0 + 1 >= 0 && x0 + 1 < W;
    const int xb = min(max(x0, 0), W - 2);
    const bool t0_hi = x0 >= W - 1, t1_lo = x0 < 0;
    const size_t plane = (size_t)H * W;
    float mu[3], sd[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        mu[c] = nrm.dev ? nrm.dev[c] : nrm.mean[c];
        sd[c] = nrm.dev ? nrm.dev[3 + c] : nrm.std[c];
    }
#pragma unroll 1
    for (int r0 = 0; r0 < ROI_R; r0 += 2) {
        float v[2][4][4], k[2][4];                                 // [row][channel][tap: nw, ne, sw, se]
        uint32_t px[2][4];                                         // U8: the four taps' pixel words
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
            const int i = i0 + r0 + rr;
            const float gy = __fadd_rn(__fmul_rn(lin_m1_1(i, 256), t11), t12);
            const float sy = __fmul_rn(__fmul_rn(__fadd_rn(gy, 1.0f), 0.5f), hm);
            const float y0f = floorf(sy);
            const int y0 = (int)y0f;
            const float wy1 = __fsub_rn(sy, y0f), wy0 = __fsub_rn(__fadd_rn(y0f, 1.0f), sy);
            const bool vy0 = y0 >= 0 && y0 < H, vy1 = y0 + 1 >= 0 && y0 + 1 < H;
            const int yc0 = min(max(y0, 0), H - 1), yc1 = min(max(y0 + 1, 0), H - 1);
            const int o0 = yc0 * W + xb, o1 = yc1 * W + xb;        // pixels o0, o0 + 1 < H * W <= INT_MAX (checked by the host)
            const float w_nw = __fmul_rn(wx0, wy0), w_ne = __fmul_rn(wx1, wy0), w_sw = __fmul_rn(wx0, wy1), w_se = __fmul_rn(wx1, wy1);
            k[rr][0] = (vy0 && vx0) ? w_nw : 0.f; k[rr][1] = (vy0 && vx1) ? w_ne : 0.f;
            k[rr][2] = (vy1 && vx0) ? w_sw : 0.f; k[rr][3] = (vy1 && vx1) ? w_se : 0.f;
            if constexpr (U8) {
                const uint8_t* srcf = static_cast<const uint8_t*>(frame);
                const uint2 c0 = ld_pair_u32(srcf + (size_t)o0 * 4), c1 = ld_pair_u32(srcf + (size_t)o1 * 4);
                px[rr][0] = t0_hi ? c0.y : c0.x; px[rr][1] = t1_lo ? c0.x : c0.y;
                px[rr][2] = t0_hi ? c1.y : c1.x; px[rr][3] = t1_lo ? c1.x : c1.y;
            }
#pragma unroll
            for (int c = U8 ? 3 : 0; c < 4; ++c) {
                float2 p0, p1;
                if (Lab && c == 3) {
                    const uint8_t* m = static_cast<const uint8_t*>(srcp);
                    const uint32_t b00 = m[o0], b01 = m[o0 + 1], b10 = m[o1], b11 = m[o1 + 1];
                    p0 = make_float2(b00 == labv ? 1.0f : 0.0f, b01 == labv ? 1.0f : 0.0f);
                    p1 = make_float2(b10 == labv ? 1.0f : 0.0f, b11 == labv ? 1.0f : 0.0f);
                } else {
                    const float* s = c < 3 ? static_cast<const float*>(frame) + (size_t)c * plane : static_cast<const float*>(srcp);
                    p0 = ld_pair(s + o0); p1 = ld_pair(s + o1);
                }
                v[rr][c][0] = t0_hi ? p0.y : p0.x; v[rr][c][1] = t1_lo ? p0.x : p0.y;
                v[rr][c][2] = t0_hi ? p1.y : p1.x; v[rr][c][3] = t1_lo ? p1.x : p1.y;
            }
        }
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
            float out[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float t[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if constexpr (U8) t[q] = c < 3 ? u8_unit(px[rr][q], c) : v[rr][3][q];
                    else t[q] = v[rr][c][q];
                }
                float acc = 0.f;
                acc = __builtin_fmaf(t[0], k[rr][0], acc);
                acc = __builtin_fmaf(t[1], k[rr][1], acc);
                acc = __builtin_fmaf(t[2], k[rr][2], acc);
                acc = __builtin_fmaf(t[3], k[rr][3], acc);
                if (c < 3) acc = __fsub_rn(acc, mu[c]) / sd[c];
                out[c] = acc;
            }
            T* d = dst + (size_t)(r0 + rr) * 256 * 4;
            if constexpr (sizeof(T) == 4) {
                *reinterpret_cast<float4*>(d) = make_float4(out[0], out[1], out[2], out[3]);
            } else {
                *reinterpret_cast<uint2*>(d) = make_uint2(pack2_bf16(out[0], out[1]), pack2_bf16(out[2], out[3]));
            }
        }
    }
}

// roi_sample_kernel / roi_sample_u8_kernel over the units [b0, b0 + B) of a video table: grid B * 256 / ROI_R, block 256, thread j =
// output column j of ROI_R rows of one unit.  The workgroup resolves its unit's video once (uniform), then runs that video's sampler.
// Lab: as in bbox_scan_multi_kernel - compiled in only for tables with a label video, chosen per video (uniform) inside.
template <typename T, typename Units, bool Lab>
__global__ __launch_bounds__(256) void roi_sample_multi_kernel(const VideoTable vt, const float* __restrict__ yxhw, Units un, RoiNorm nrm,
                                                               T* __restrict__ roi) {
    constexpr int GPS = 256 / ROI_R;
    const int b = blockIdx.x / GPS, i0 = (blockIdx.x % GPS) * ROI_R, j = threadIdx.x;
    const int u = un.at(b);
    T* dst = roi + (((size_t)b * 256 + i0) * 256 + j) * 4;
    if (!un.valid(u, vt.units)) {                                  // (uniform) a zero tile
        for (int r = 0; r < ROI_R; ++r) {
            T* d0 = dst + (size_t)r * 256 * 4;
            if constexpr (sizeof(T) == 4) *reinterpret_cast<float4*>(d0) = make_float4(0.f, 0.f, 0.f, 0.f);
            else *reinterpret_cast<uint2*>(d0) = make_uint2(0u, 0u);
        }
        return;
    }
    const int vi = video_of_unit(vt, u);
    const VideoDesc& d = vt.v[vi];
    const int H = d.H, W = d.W, nf = d.n_frames;
    const int lu = u - vt.first[vi], fr = lu % nf;
    if constexpr (Lab) {
        if (d.lab) {                                               // (uniform)
            const uint8_t* srcm = d.lab + (size_t)fr * d.lab_stride;
            const uint32_t labv = (uint32_t)(lu / nf) + 1u;
            if (d.u8) {
                const uint8_t* srcf = static_cast<const uint8_t*>(d.frames) + (size_t)fr * H * W * 4;
                roi_unit_rows<T, true, true>(srcf, srcm, yxhw + b * 4, H, W, nrm, i0, j, dst, labv);
            } else {
                const float* srcf = static_cast<const float*>(d.frames) + (size_t)fr * 3 * H * W;
                roi_unit_rows<T, false, true>(srcf, srcm, yxhw + b * 4, H, W, nrm, i0, j, dst, labv);
            }
            return;
        }
    }
    const float* srcp = d.masks + (size_t)(lu / nf) * d.stride_obj + (size_t)fr * d.stride_frame;
    if (d.u8) {
        const uint8_t* srcf = static_cast<const uint8_t*>(d.frames) + (size_t)fr * H * W * 4;
        roi_unit_rows<T, true>(srcf, srcp, yxhw + b * 4, H, W, nrm, i0, j, dst);
    } else {
        const float* srcf = static_cast<const float*>(d.frames) + (size_t)fr * 3 * H * W;
        roi_unit_rows<T, false>(srcf, srcp, yxhw + b * 4, H, W, nrm, i0, j, dst);
    }
}

void launch_roi_sample_multi(const VideoTable& vt, const float* yxhw, int b0, int B, int dtype, const RoiNorm& nrm, void* roi, hipStream_t st,
                             const int32_t* ids) {
    const dim3 grid(B * (256 / ROI_R)), block(256);
    auto launch = [&](auto un, auto lab) {
        constexpr bool Lab = decltype(lab)::value;
        using Units = decltype(un);
        if (dtype != IVOSW_BF16)
            hipLaunchKernelGGL((roi_sample_multi_kernel<float, Units, Lab>), grid, block, 0, st, vt, yxhw, un, nrm, static_cast<float*>(roi));
        else
            hipLaunchKernelGGL((roi_sample_multi_kernel<bf16_t, Units, Lab>), grid, block, 0, st, vt, yxhw, un, nrm, static_cast<bf16_t*>(roi));
    };
    if (ids) {
        if (vt.any_lab) launch(UnitList{ids, b0}, std::true_type{});
        else launch(UnitList{ids, b0}, std::false_type{});
        return;
    }
    if (vt.any_lab) launch(UnitRange{b0}, std::true_type{});
    else launch(UnitRange{b0}, std::false_type{});
}

static void set_video_error(const char* who, int i, const char* msg) { set_error("%s: video %d: %s", who, i, msg); }

int video_table_build(const ivosw_video_t* videos, int n_videos, const char* who, VideoTable* out, const ivosw_labels_t* labels) {
    if (!videos) { set_error("%s: null pointer (videos)", who); return IVOSW_ERR_ARG; }
    if (n_videos < 1 || n_videos > IVOSW_MAX_VIDEOS) {
        set_error("%s: n_videos = %d is outside [1, %d]", who, n_videos, IVOSW_MAX_VIDEOS);
        return IVOSW_ERR_ARG;
    }
    VideoTable t{};
    long units = 0;
    for (int i = 0; i < IVOSW_MAX_VIDEOS; ++i) t.first[i] = INT_MAX;
    for (int i = 0; i < n_videos; ++i) {
        const ivosw_video_t& s = videos[i];
#define VIDEO_REQUIRE(cond, msg) do { if (!(cond)) { set_video_error(who, i, msg); return IVOSW_ERR_ARG; } } while (0)
        const bool lab = labels && labels[i].map;                   // a label video: masks and its strides are not looked at
        VIDEO_REQUIRE(s.frames && (lab || s.masks), "null pointer");
        VIDEO_REQUIRE(s.frames_kind == IVOSW_FRAMES_F32 || s.frames_kind == IVOSW_FRAMES_RGBX8, "frames_kind must be IVOSW_FRAMES_F32 or IVOSW_FRAMES_RGBX8");
        VIDEO_REQUIRE(s.n_frames > 0 && s.n_obj > 0, "n_frames and n_obj must be positive");
        VIDEO_REQUIRE(s.H > 1 && s.W > 1, "H, W > 1 wanted");
        VIDEO_REQUIRE((long)s.H * s.W <= INT_MAX, "frame too large (H * W <= INT_MAX)");
        if (lab) {
            VIDEO_REQUIRE(s.n_obj <= 255, "a label map holds at most 255 objects (n_obj <= 255)");
            VIDEO_REQUIRE(labels[i].stride_frame >= 0, "negative label stride");
            VIDEO_REQUIRE(labels[i].stride_frame >= (long)s.H * s.W || s.n_frames == 1, "label maps of consecutive frames overlap");
        } else {
            VIDEO_REQUIRE(s.mask_stride_obj >= 0 && s.mask_stride_frame >= 0, "negative mask stride");
            VIDEO_REQUIRE(s.mask_stride_frame >= (long)s.H * s.W || s.n_frames == 1, "mask planes of consecutive frames overlap");
        }
        VIDEO_REQUIRE(s.frames_kind != IVOSW_FRAMES_RGBX8 || (reinterpret_cast<uintptr_t>(s.frames) & 3) == 0, "rgbx must be 4-byte aligned");
        units += (long)s.n_frames * s.n_obj;
        VIDEO_REQUIRE(units < (1L << 30), "too many (frame, object) units for one call (2^30 or more up to this video)");
#undef VIDEO_REQUIRE
        VideoDesc& d = t.v[i];
        d.frames = s.frames;
        if (!lab) { d.masks = s.masks; d.stride_frame = s.mask_stride_frame; d.stride_obj = s.mask_stride_obj; }
        d.n_frames = s.n_frames; d.n_obj = s.n_obj; d.H = s.H; d.W = s.W;
        d.u8 = s.frames_kind == IVOSW_FRAMES_RGBX8;
        d.vec_ok = ((size_t)s.H * s.W) % 4 == 0 && (reinterpret_cast<uintptr_t>(s.masks) & 15) == 0 && s.mask_stride_frame % 4 == 0 &&
                   s.mask_stride_obj % 4 == 0;
        if (lab) {
            d.lab = labels[i].map; d.lab_stride = labels[i].stride_frame;
            d.vec_ok = ((size_t)s.H * s.W) % 16 == 0 && (reinterpret_cast<uintptr_t>(d.lab) & 15) == 0 && d.lab_stride % 16 == 0;
            t.any_lab = 1;
        }
        t.first[i] = (int)(units - (long)s.n_frames * s.n_obj);
    }
    t.n = n_videos;
    t.units = (int)units;
    if (out) *out = t;
    return IVOSW_OK;
}


// ---------------------------------------------------------------- which units changed (incremental assessment)
// The session's copy of the planes it was last scored on against the planes of now: a pure streaming pass, two 16-byte loads per lane
// and a store only where the bit patterns differ (per 16-byte vector when any lane differs; per element on the scalar path), so a session
// whose masks did not change writes nothing.  Bytes per unit: 2 x 4 x H x W read (4 x H x W when the video is cold: the cache is not
// looked at), up to 4 x H x W written.  cache[v] is dense [n_obj][n_frames][H*W] in unit order.  The pointers travel in the kernel
// arguments like the table.
struct DeltaArgs {
    float* cache[IVOSW_MAX_VIDEOS];
    int cold[IVOSW_MAX_VIDEOS];
    int vec[IVOSW_MAX_VIDEOS];           // 16-byte path: the video's vec_ok and a 16-byte aligned cache
};
constexpr int DELTA_CHUNK = 8192;        // elements of a plane per workgroup: two rounds of four 16-byte loads per lane and side

__global__ void delta_init_kernel(int32_t* __restrict__ flags, int n) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u < n) flags[u] = 0;
}

__device__ __forceinline__ bool differs(const uint4& a, const uint4& b) { return ((a.x ^ b.x) | (a.y ^ b.y) | (a.z ^ b.z) | (a.w ^ b.w)) != 0u; }

// grid units * S (S = slices of the largest plane), block 256: workgroup (u, s) compares elements [s * DELTA_CHUNK, (s + 1) * DELTA_CHUNK)
// of unit u's plane.  A workgroup whose slice lies behind its own video's plane leaves before the barrier (uniform).  Every workgroup that
// finds a difference stores the same 1 into flags[u]: no atomics.
// Lab (a call that mixes float and label videos): the units of the label videos leave at once - mask_delta_lab_kernel compares those.
template <bool Lab>
__global__ __launch_bounds__(256) void mask_delta_kernel(const VideoTable vt, const DeltaArgs da, int S, int32_t* __restrict__ flags) {
    const int u = blockIdx.x / S, s = blockIdx.x % S;
    const int vi = video_of_unit(vt, u);
    const VideoDesc& d = vt.v[vi];
    if constexpr (Lab) {
        if (d.lab) return;                                         // (uniform)
    }
    const size_t plane = (size_t)d.H * d.W;
    const size_t beg = (size_t)s * DELTA_CHUNK;
    if (beg >= plane) return;
    const size_t end = min(plane, beg + (size_t)DELTA_CHUNK);
    const int lu = u - vt.first[vi], nf = d.n_frames;
    const uint32_t* p = reinterpret_cast<const uint32_t*>(d.masks + (size_t)(lu / nf) * d.stride_obj + (size_t)(lu % nf) * d.stride_frame);
    uint32_t* c = reinterpret_cast<uint32_t*>(da.cache[vi]) + (size_t)lu * plane;
    const bool cold = da.cold[vi] != 0;
    int dirty = cold ? 1 : 0;
    if (da.vec[vi]) {                     // plane % 4 == 0: end is a multiple of 4 and every vector lies inside the plane
        size_t i = beg + (size_t)threadIdx.x * 4;
        if (cold) {
            for (; i < end; i += 1024) *reinterpret_cast<uint4*>(c + i) = *reinterpret_cast<const uint4*>(p + i);
        } else {
            for (; i + 3 * 1024 < end; i += 4 * 1024) {            // eight 16-byte loads in flight per lane
                uint4 a[4], b[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) a[k] = *reinterpret_cast<const uint4*>(p + i + k * 1024);
#pragma unroll
                for (int k = 0; k < 4; ++k) b[k] = *reinterpret_cast<const uint4*>(c + i + k * 1024);
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (differs(a[k], b[k])) { *reinterpret_cast<uint4*>(c + i + k * 1024) = a[k]; dirty = 1; }
            }
            for (; i < end; i += 1024) {
                const uint4 a = *reinterpret_cast<const uint4*>(p + i), b = *reinterpret_cast<const uint4*>(c + i);
                if (differs(a, b)) { *reinterpret_cast<uint4*>(c + i) = a; dirty = 1; }
            }
        }
    } else {
        for (size_t i = beg + threadIdx.x; i < end; i += 256) {
            const uint32_t a = p[i];
            if (cold || a != c[i]) { c[i] = a; dirty = 1; }
        }
    }
    if (__syncthreads_or(dirty) && threadIdx.x == 0) flags[u] = 1;
}

// The same for label videos, one pass per FRAME instead of one per unit: cache[v] is a dense uint8 [n_frames][H*W] copy of the map, and a
// pixel whose byte went from a to b dirties the units (frame, a - 1) and (frame, b - 1) - the two planes that pixel changed in - when those
// labels lie in 1 .. n_obj.  Bytes per frame: 2 x H x W read (H x W when cold), against 2 x 4 x H x W per UNIT of the float pass.
// grid (frames of the label videos) * S, block 256: workgroup (f, s) compares bytes [s * LAB_DELTA_CHUNK, (s + 1) * LAB_DELTA_CHUNK) of
// frame f.  Vector path (the video's vec_ok and a 16-byte aligned cache): 16-byte loads of both sides, a store only where the vector
// differs; else byte by byte, a store only where the byte differs.  Every lane collects the labels 1 .. 64 it saw change in a 64-bit mask,
// OR-reduced over the workgroup; one lane then stores the same 1 per set bit (no atomics).  Labels above 64 are flagged by a plain store
// where they are met.
struct LabDeltaArgs {
    uint8_t* cache[IVOSW_MAX_VIDEOS];
    int cold[IVOSW_MAX_VIDEOS];
    int vec[IVOSW_MAX_VIDEOS];
    int ffirst[IVOSW_MAX_VIDEOS];        // first frame of video i among the frames of the label videos (a float video holds none); INT_MAX for i >= n
};
static_assert(sizeof(VideoTable) + sizeof(LabDeltaArgs) + 64 <= 4096, "mask_delta_lab_kernel's arguments no longer fit");
static_assert(sizeof(VideoTable) + sizeof(DeltaArgs) + 64 <= 4096, "mask_delta_kernel's arguments no longer fit");
constexpr int LAB_DELTA_CHUNK = 16384;   // bytes of a frame per workgroup: four 16-byte loads per lane and side

__global__ __launch_bounds__(256) void mask_delta_lab_kernel(const VideoTable vt, const LabDeltaArgs da, int S, int32_t* __restrict__ flags) {
    const int f = blockIdx.x / S, s = blockIdx.x % S;
    int vi = 0;
#pragma unroll
    for (int i = 1; i < IVOSW_MAX_VIDEOS; ++i) vi += (f >= da.ffirst[i]) ? 1 : 0;
    const VideoDesc& d = vt.v[vi];
    const size_t plane = (size_t)d.H * d.W;
    const size_t beg = (size_t)s * LAB_DELTA_CHUNK;
    if (beg >= plane) return;
    const size_t end = min(plane, beg + (size_t)LAB_DELTA_CHUNK);
    const int fr = f - da.ffirst[vi], nf = d.n_frames, n_obj = d.n_obj;
    const uint8_t* p = d.lab + (size_t)fr * d.lab_stride;
    uint8_t* c = da.cache[vi] + (size_t)fr * plane;
    int32_t* fl = flags + vt.first[vi] + fr;                       // unit (fr, obj) of this video: fl[obj * nf]
    const bool cold = da.cold[vi] != 0;
    unsigned long long seen = 0ull;                                // bit l - 1: label l changed somewhere in this lane's bytes
    auto note = [&](uint32_t l) {
        if (l - 1u < (uint32_t)n_obj) {
            if (l <= 64u) seen |= 1ull << (l - 1u);
            else fl[(size_t)(l - 1u) * nf] = 1;
        }
    };
    if (da.vec[vi]) {                     // plane % 16 == 0: end is a multiple of 16 and every vector lies inside the frame
        size_t i = beg + (size_t)threadIdx.x * 16;
        if (cold) {
            for (; i < end; i += 4096) *reinterpret_cast<uint4*>(c + i) = *reinterpret_cast<const uint4*>(p + i);
        } else {
            auto visit = [&](const uint4 a, const uint4 b, size_t at) {      // (by value: b may be loaded from c + at, which is stored to)
                if (differs(a, b)) {
                    *reinterpret_cast<uint4*>(c + at) = a;
                    const uint32_t wa[4] = {a.x, a.y, a.z, a.w}, wb[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        if (wa[k] != wb[k]) {
#pragma unroll
                            for (int j = 0; j < 4; ++j) {
                                const uint32_t x = (wa[k] >> (8 * j)) & 0xffu, y = (wb[k] >> (8 * j)) & 0xffu;
                                if (x != y) { note(x); note(y); }
                            }
                        }
                    }
                }
            };
            for (; i + 3 * 4096 < end; i += 4 * 4096) {            // eight 16-byte loads in flight per lane
                uint4 a[4], b[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) a[k] = *reinterpret_cast<const uint4*>(p + i + k * 4096);
#pragma unroll
                for (int k = 0; k < 4; ++k) b[k] = *reinterpret_cast<const uint4*>(c + i + k * 4096);
#pragma unroll
                for (int k = 0; k < 4; ++k) visit(a[k], b[k], i + k * 4096);
            }
            for (; i < end; i += 4096) visit(*reinterpret_cast<const uint4*>(p + i), *reinterpret_cast<const uint4*>(c + i), i);
        }
    } else {
        for (size_t i = beg + threadIdx.x; i < end; i += 256) {
            const uint32_t a = p[i];
            if (cold) { c[i] = (uint8_t)a; continue; }
            const uint32_t b = c[i];
            if (a != b) { c[i] = (uint8_t)a; note(a); note(b); }
        }
    }
    if (cold) {                                                    // every unit of the frame, whatever the map holds (n_obj <= 255 < 256 lanes)
        if ((int)threadIdx.x < n_obj) fl[(size_t)threadIdx.x * nf] = 1;
        return;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) seen |= __shfl_xor(seen, o, 64);
    __shared__ unsigned long long red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = seen;
    __syncthreads();
    if (threadIdx.x < 64) {                                        // lane l - 1 stores label l's flag
        const unsigned long long all = red[0] | red[1] | red[2] | red[3];
        if ((all >> threadIdx.x) & 1ull) fl[(size_t)threadIdx.x * nf] = 1;
    }
}

// flags [n] -> the set entries' indices in ascending order, and their number: one workgroup walks the flags 1024 at a time, a ballot gives
// every wave its count and every lane its rank inside the wave, the 16 wave counts are summed through LDS.
__global__ __launch_bounds__(1024) void delta_compact_kernel(const int32_t* __restrict__ flags, int n, int32_t* __restrict__ ids,
                                                             int32_t* __restrict__ n_out) {
    __shared__ int wsum[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int total = 0;
    for (int base = 0; base < n; base += 1024) {
        const int u = base + (int)threadIdx.x;
        const bool f = u < n && flags[u] != 0;
        const unsigned long long m = __ballot(f);
        const int rank = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[wave] = __popcll(m);
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            const int c = wsum[w];
            before += w < wave ? c : 0;
            all += c;
        }
        if (f) ids[total + before + rank] = u;
        total += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) *n_out = total;
}

// scores[ids[i]] = compact[i]: the last launch of a forward over a unit list.  An id outside [0, units) is dropped.
__global__ void scatter_units_kernel(const float* __restrict__ compact, const int32_t* __restrict__ ids, int n, int units,
                                     float* __restrict__ scores) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int u = ids[i];
    if ((unsigned)u < (unsigned)units) scores[u] = compact[i];
}

void launch_scatter_units(const float* compact, const int32_t* ids, int n, int units, float* scores, hipStream_t st) {
    hipLaunchKernelGGL(scatter_units_kernel, dim3((n + 255) / 256), dim3(256), 0, st, compact, ids, n, units, scores);
}

}  // namespace ivosw

using namespace ivosw;

extern "C" int ivosw_mask_bbox(const float* tp, int B, int H, int W, float* yxhw, int32_t* scratch,
                               ivosw_stream_t stream) {
    IVOSW_REQUIRE(tp && yxhw && scratch, "null pointer");
    IVOSW_ON_DEVICE_OF(yxhw);
    IVOSW_REQUIRE(B > 0 && H > 0 && W > 0, "B, H, W must be positive");
    launch_mask_bbox(tp, 0, B, H, W, SampleMap{B, (long)H * W, 0}, yxhw, scratch, as_stream(stream));
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}

extern "C" int ivosw_roi_sample(const float* tf, const float* tp, const float* yxhw, int B, int H, int W, int dtype,
                                void* roi, ivosw_stream_t stream) {
    IVOSW_REQUIRE(tf && tp && yxhw && roi, "null pointer");
    IVOSW_ON_DEVICE_OF(roi);
    IVOSW_REQUIRE(B > 0 && H > 1 && W > 1, "B must be positive and H, W > 1");
    IVOSW_REQUIRE((long)H * W <= INT_MAX && B <= (1 << 24), "frame or batch too large (H * W <= INT_MAX, B <= 2^24)");
    IVOSW_REQUIRE(dtype == IVOSW_F32 || dtype == IVOSW_BF16 || dtype == IVOSW_F32X3, "dtype must be IVOSW_F32, IVOSW_BF16 or IVOSW_F32X3");
    RoiNorm nrm{{0.485f, 0.456f, 0.406f}, {0.229f, 0.224f, 0.225f}, nullptr};  // Encoder.mean/std (assessment.py:41-44)
    launch_roi_sample(FrameSrc{tf, 0}, tp, yxhw, 0, B, H, W, dtype, SampleMap{B, (long)H * W, 0}, nrm, roi, as_stream(stream));
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}

extern "C" int ivosw_frames_pack_u8(const uint8_t* src, int layout, int n, int H, int W, uint8_t* rgbx, ivosw_stream_t stream) {
    IVOSW_REQUIRE(src && rgbx, "null pointer");
    IVOSW_REQUIRE(layout == IVOSW_U8_HWC3 || layout == IVOSW_U8_CHW3, "layout must be IVOSW_U8_HWC3 or IVOSW_U8_CHW3");
    IVOSW_REQUIRE(n > 0 && H > 0 && W > 0, "n, H, W must be positive");
    IVOSW_REQUIRE((long)H * W <= INT_MAX && n <= (1 << 24), "frame or video too large (H * W <= INT_MAX, n <= 2^24)");
    IVOSW_REQUIRE((reinterpret_cast<uintptr_t>(rgbx) & 3) == 0, "rgbx must be 4-byte aligned");
    IVOSW_ON_DEVICE_OF(rgbx);
    const size_t plane = (size_t)H * W, P = plane * (size_t)n;
    const int vec = (reinterpret_cast<uintptr_t>(src) & 3) == 0 && (reinterpret_cast<uintptr_t>(rgbx) & 15) == 0 &&
                    (layout == IVOSW_U8_HWC3 || plane % 4 == 0);
    const size_t threads = vec ? std::max(P / 4, P % 4) : P;
    hipLaunchKernelGGL(frames_pack_u8_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, as_stream(stream), src, layout, vec, P,
                       plane, rgbx);
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}

extern "C" int ivosw_roi_sample_u8(const uint8_t* rgbx, const float* tp, const float* yxhw, int B, int H, int W, int dtype,
                                   void* roi, ivosw_stream_t stream) {
    IVOSW_REQUIRE(rgbx && tp && yxhw && roi, "null pointer");
    IVOSW_REQUIRE((reinterpret_cast<uintptr_t>(rgbx) & 3) == 0, "rgbx must be 4-byte aligned");
    IVOSW_REQUIRE(B > 0 && H > 1 && W > 1, "B must be positive and H, W > 1");
    IVOSW_REQUIRE((long)H * W <= INT_MAX && B <= (1 << 24), "frame or batch too large (H * W <= INT_MAX, B <= 2^24)");
    IVOSW_REQUIRE(dtype == IVOSW_F32 || dtype == IVOSW_BF16 || dtype == IVOSW_F32X3, "dtype must be IVOSW_F32, IVOSW_BF16 or IVOSW_F32X3");
    IVOSW_ON_DEVICE_OF(roi);
    RoiNorm nrm{{0.485f, 0.456f, 0.406f}, {0.229f, 0.224f, 0.225f}, nullptr};  // Encoder.mean/std (assessment.py:41-44)
    launch_roi_sample(FrameSrc{rgbx, 1}, tp, yxhw, 0, B, H, W, dtype, SampleMap{B, (long)H * W, 0}, nrm, roi, as_stream(stream));
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}

extern "C" long ivosw_assess_videos_units(const ivosw_video_t* videos, int n_videos) {
    VideoTable vt;
    const int rc = video_table_build(videos, n_videos, __func__, &vt);
    return rc == IVOSW_OK ? (long)vt.units : (long)rc;
}

// The table entries and their _lab twins (include/ivosw.h) share one body each: `labels` is NULL for the plain entry.
// (IVOSW_REQUIRE with the entry's own name in the message instead of the shared body's)
#define REQUIRE_AS(who, cond, msg) do { if (!(cond)) { ::ivosw::set_error("%s: %s", who, msg); return IVOSW_ERR_ARG; } } while (0)
static int mask_bbox_videos_impl(const char* who, const ivosw_video_t* videos, const ivosw_labels_t* labels, int n_videos, float* yxhw,
                                 int32_t* scratch, ivosw_stream_t stream) {
    VideoTable vt;
    if (const int rc = video_table_build(videos, n_videos, who, &vt, labels)) return rc;
    REQUIRE_AS(who, yxhw && scratch, "null pointer");
    IVOSW_ON_DEVICE_OF(yxhw);
    launch_mask_bbox_multi(vt, 0, vt.units, yxhw, scratch, as_stream(stream));
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}

extern "C" int ivosw_mask_bbox_videos(const ivosw_video_t* videos, int n_videos, float* yxhw, int32_t* scratch, ivosw_stream_t stream) {
    return mask_bbox_videos_impl(__func__, videos, nullptr, n_videos, yxhw, scratch, stream);
}

extern "C" int ivosw_mask_bbox_videos_lab(const ivosw_video_t* videos, const ivosw_labels_t* labels, int n_videos, float* yxhw,
                                          int32_t* scratch, ivosw_stream_t stream) {
    return mask_bbox_videos_impl(__func__, videos, labels, n_videos, yxhw, scratch, stream);
}

static int roi_sample_videos_impl(const char* who, const ivosw_video_t* videos, const ivosw_labels_t* labels, int n_videos, const float* yxhw,
                                  int dtype, void* roi, ivosw_stream_t stream) {
    VideoTable vt;
    if (const int rc = video_table_build(videos, n_videos, who, &vt, labels)) return rc;
    REQUIRE_AS(who, yxhw && roi, "null pointer");
    REQUIRE_AS(who, vt.units <= (1 << 24), "batch too large (units <= 2^24)");
    REQUIRE_AS(who, dtype == IVOSW_F32 || dtype == IVOSW_BF16 || dtype == IVOSW_F32X3, "dtype must be IVOSW_F32, IVOSW_BF16 or IVOSW_F32X3");
    IVOSW_ON_DEVICE_OF(roi);
    RoiNorm nrm{{0.485f, 0.456f, 0.406f}, {0.229f, 0.224f, 0.225f}, nullptr};  // Encoder.mean/std (assessment.py:41-44)
    launch_roi_sample_multi(vt, yxhw, 0, vt.units, dtype, nrm, roi, as_stream(stream));
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}

extern "C" int ivosw_roi_sample_videos(const ivosw_video_t* videos, int n_videos, const float* yxhw, int dtype, void* roi,
                                       ivosw_stream_t stream) {
    return roi_sample_videos_impl(__func__, videos, nullptr, n_videos, yxhw, dtype, roi, stream);
}

extern "C" int ivosw_roi_sample_videos_lab(const ivosw_video_t* videos, const ivosw_labels_t* labels, int n_videos, const float* yxhw,
                                           int dtype, void* roi, ivosw_stream_t stream) {
    return roi_sample_videos_impl(__func__, videos, labels, n_videos, yxhw, dtype, roi, stream);
}

static int mask_delta_videos_impl(const char* who, const ivosw_video_t* videos, const ivosw_labels_t* labels, int n_videos,
                                  void* const* cache, const int* cold, int32_t* flags, int32_t* unit_ids, int32_t* n_dirty,
                                  ivosw_stream_t stream) {
    VideoTable vt;
    if (const int rc = video_table_build(videos, n_videos, who, &vt, labels)) return rc;
    REQUIRE_AS(who, cache && cold && flags && unit_ids && n_dirty, "null pointer");
    DeltaArgs da{};
    LabDeltaArgs la{};
    size_t plane = 0, lab_plane = 0;
    long lab_frames = 0;
    int n_float = 0;
    for (int i = 0; i < IVOSW_MAX_VIDEOS; ++i) la.ffirst[i] = INT_MAX;
    for (int i = 0; i < vt.n; ++i) {
        if (!cache[i]) { set_video_error(who, i, "null pointer (cache)"); return IVOSW_ERR_ARG; }
        la.ffirst[i] = (int)lab_frames;
        if (vt.v[i].lab) {                                         // a uint8 [n_frames][H*W] copy of the map: any alignment
            la.cache[i] = static_cast<uint8_t*>(cache[i]);
            la.cold[i] = cold[i] != 0;
            la.vec[i] = vt.v[i].vec_ok && (reinterpret_cast<uintptr_t>(cache[i]) & 15) == 0;
            lab_plane = std::max(lab_plane, (size_t)vt.v[i].H * vt.v[i].W);
            lab_frames += vt.v[i].n_frames;
            continue;
        }
        if (reinterpret_cast<uintptr_t>(cache[i]) & 3) { set_video_error(who, i, "cache must be 4-byte aligned"); return IVOSW_ERR_ARG; }
        da.cache[i] = static_cast<float*>(cache[i]);
        da.cold[i] = cold[i] != 0;
        da.vec[i] = vt.v[i].vec_ok && (reinterpret_cast<uintptr_t>(cache[i]) & 15) == 0;
        plane = std::max(plane, (size_t)vt.v[i].H * vt.v[i].W);
        ++n_float;
    }
    IVOSW_ON_DEVICE_OF(flags);
    const int S = (int)((plane + DELTA_CHUNK - 1) / DELTA_CHUNK);
    const int SL = (int)((lab_plane + LAB_DELTA_CHUNK - 1) / LAB_DELTA_CHUNK);
    REQUIRE_AS(who, (long)vt.units * S <= INT_MAX && lab_frames * SL <= INT_MAX, "too many (unit, plane slice) workgroups for one launch");
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(delta_init_kernel, dim3((vt.units + 255) / 256), dim3(256), 0, st, flags, vt.units);
    if (!vt.any_lab) {
        hipLaunchKernelGGL(mask_delta_kernel<false>, dim3((unsigned)(vt.units * S)), dim3(256), 0, st, vt, da, S, flags);
    } else {                                                       // up to two compare launches: the float videos' units, the label videos' frames
        if (n_float) hipLaunchKernelGGL(mask_delta_kernel<true>, dim3((unsigned)(vt.units * S)), dim3(256), 0, st, vt, da, S, flags);
        hipLaunchKernelGGL(mask_delta_lab_kernel, dim3((unsigned)(lab_frames * SL)), dim3(256), 0, st, vt, la, SL, flags);
    }
    hipLaunchKernelGGL(delta_compact_kernel, dim3(1), dim3(1024), 0, st, flags, vt.units, unit_ids, n_dirty);
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}

extern "C" int ivosw_mask_delta_videos(const ivosw_video_t* videos, int n_videos, float* const* cache, const int* cold, int32_t* flags,
                                       int32_t* unit_ids, int32_t* n_dirty, ivosw_stream_t stream) {
    return mask_delta_videos_impl(__func__, videos, nullptr, n_videos, reinterpret_cast<void* const*>(cache), cold, flags, unit_ids, n_dirty,
                                  stream);
}

extern "C" int ivosw_mask_delta_videos_lab(const ivosw_video_t* videos, const ivosw_labels_t* labels, int n_videos, void* const* cache,
                                           const int* cold, int32_t* flags, int32_t* unit_ids, int32_t* n_dirty, ivosw_stream_t stream) {
    return mask_delta_videos_impl(__func__, videos, labels, n_videos, cache, cold, flags, unit_ids, n_dirty, stream);
}

// what the *_units entries refuse about their list, before any launch
static int unit_list_check(const char* who, const VideoTable& vt, const int32_t* unit_ids, int n_ids) {
    if (n_ids < 0) { set_error("%s: n_ids = %d is negative", who, n_ids); return IVOSW_ERR_ARG; }
    if (n_ids > vt.units) { set_error("%s: n_ids = %d is above the table's %d units", who, n_ids, vt.units); return IVOSW_ERR_ARG; }
    if (n_ids > 0 && !unit_ids) { set_error("%s: null pointer (unit_ids)", who); return IVOSW_ERR_ARG; }
    return IVOSW_OK;
}

static int mask_bbox_units_impl(const char* who, const ivosw_video_t* videos, const ivosw_labels_t* labels, int n_videos,
                                const int32_t* unit_ids, int n_ids, float* yxhw, int32_t* scratch, ivosw_stream_t stream) {
    VideoTable vt;
    if (const int rc = video_table_build(videos, n_videos, who, &vt, labels)) return rc;
    if (const int rc = unit_list_check(who, vt, unit_ids, n_ids)) return rc;
    if (n_ids == 0) return IVOSW_OK;
    REQUIRE_AS(who, yxhw && scratch, "null pointer");
    IVOSW_ON_DEVICE_OF(yxhw);
    launch_mask_bbox_multi(vt, 0, n_ids, yxhw, scratch, as_stream(stream), unit_ids);
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}

extern "C" int ivosw_mask_bbox_units(const ivosw_video_t* videos, int n_videos, const int32_t* unit_ids, int n_ids, float* yxhw,
                                     int32_t* scratch, ivosw_stream_t stream) {
    return mask_bbox_units_impl(__func__, videos, nullptr, n_videos, unit_ids, n_ids, yxhw, scratch, stream);
}

extern "C" int ivosw_mask_bbox_units_lab(const ivosw_video_t* videos, const ivosw_labels_t* labels, int n_videos, const int32_t* unit_ids,
                                         int n_ids, float* yxhw, int32_t* scratch, ivosw_stream_t stream) {
    return mask_bbox_units_impl(__func__, videos, labels, n_videos, unit_ids, n_ids, yxhw, scratch, stream);
}

static int roi_sample_units_impl(const char* who, const ivosw_video_t* videos, const ivosw_labels_t* labels, int n_videos,
                                 const int32_t* unit_ids, int n_ids, const float* yxhw, int dtype, void* roi, ivosw_stream_t stream) {
    VideoTable vt;
    if (const int rc = video_table_build(videos, n_videos, who, &vt, labels)) return rc;
    if (const int rc = unit_list_check(who, vt, unit_ids, n_ids)) return rc;
    REQUIRE_AS(who, dtype == IVOSW_F32 || dtype == IVOSW_BF16 || dtype == IVOSW_F32X3, "dtype must be IVOSW_F32, IVOSW_BF16 or IVOSW_F32X3");
    if (n_ids == 0) return IVOSW_OK;
    REQUIRE_AS(who, yxhw && roi, "null pointer");
    REQUIRE_AS(who, n_ids <= (1 << 24), "batch too large (n_ids <= 2^24)");
    IVOSW_ON_DEVICE_OF(roi);
    RoiNorm nrm{{0.485f, 0.456f, 0.406f}, {0.229f, 0.224f, 0.225f}, nullptr};  // Encoder.mean/std (assessment.py:41-44)
    launch_roi_sample_multi(vt, yxhw, 0, n_ids, dtype, nrm, roi, as_stream(stream), unit_ids);
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}

extern "C" int ivosw_roi_sample_units(const ivosw_video_t* videos, int n_videos, const int32_t* unit_ids, int n_ids, const float* yxhw,
                                      int dtype, void* roi, ivosw_stream_t stream) {
    return roi_sample_units_impl(__func__, videos, nullptr, n_videos, unit_ids, n_ids, yxhw, dtype, roi, stream);
}

extern "C" int ivosw_roi_sample_units_lab(const ivosw_video_t* videos, const ivosw_labels_t* labels, int n_videos, const int32_t* unit_ids,
                                          int n_ids, const float* yxhw, int dtype, void* roi, ivosw_stream_t stream) {
    return roi_sample_units_impl(__func__, videos, labels, n_videos, unit_ids, n_ids, yxhw, dtype, roi, stream);
}
#undef REQUIRE_AS

// ---------------------------------------------------------------- shader-clock probe (measurement aid, bench.py roofline.sclk_mhz)
// One wave spins for `spin_us` of wall time and reports {shader cycles (s_memtime), 100 MHz wall ticks (s_memrealtime)} of the
// interval: launched on a side stream beside a forward pass it gives the shader clock the chip actually ran at under that load
// (the chip clocks to its power budget: DESIGN section 5).  out: 2 x uint64 on the device.
namespace ivosw {
__global__ void clock_probe_kernel(unsigned long long* __restrict__ out, unsigned long long spin_ticks) {
    if (threadIdx.x != 0) return;
    const unsigned long long r0 = wall_clock64();
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    unsigned long long r1 = r0;
    while (r1 - r0 < spin_ticks) {
        __builtin_amdgcn_s_sleep(32);
        r1 = wall_clock64();
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    out[0] = t1 - t0;
    out[1] = wall_clock64() - r0;
}
}  // namespace ivosw

extern "C" int ivosw_clock_probe(unsigned long long* out2, int spin_us, ivosw_stream_t stream) {
    using namespace ivosw;
    IVOSW_REQUIRE(out2 && spin_us > 0 && spin_us <= 1000000, "null pointer / spin_us out of range");
    IVOSW_ON_DEVICE_OF(out2);
    hipLaunchKernelGGL(clock_probe_kernel, dim3(1), dim3(64), 0, as_stream(stream), out2, (unsigned long long)spin_us * 100ull);
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}
