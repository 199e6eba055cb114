// Assessment samples on the device, step one: the probability maps as 8-bit planes.
//
// Reference (generate_data.py:240 -> utils/misc.py:165-181, save_seg_preds): after every interaction the whole all_P goes to the host as
// float32 and every object plane is written through cv2.imwrite(path, probs[i, n] * 255) - numpy's float32 product, then OpenCV's
// saturating 8-bit conversion (saturate_cast<uchar>(float): cvRound = round half to even, then the clamp to 0 .. 255).  Here one streaming
// kernel forms those bytes where all_P lives, object-major [n_obj][n_frames][H][W] (objects 1 .. O, channel 0 is never read), so one
// uint8 copy - a quarter of the reference's bytes - reaches the host, and the J / F count pass (metrics.hip, the byte-plane prediction
// source) reads the same planes without any copy at all.
//
// The rule is the definition: q = clamp(rint(fl32(p * 255.0f)), 0, 255) with one fp32 product, round half to even, NaN -> 0.  OpenCV is
// not available where this was written, so parity with cv2 is restated, not recorded (tests/qa_ref.py restates it in numpy).
//
// 5 bytes per pixel (4 in, 1 out), no reuse: HBM-bound.  No LDS, no atomics, no scratch, no allocation; capture-safe.
#include "lane_group.h"

namespace ivosw {

namespace {
struct QaQuantArgs {
    const float* probs;      // element (f, c, pixel) at probs[f * sn + c * sc + pixel]
    long sn, sc;
    uint8_t* planes;         // [n_obj][n][HW]
    int n, hw;
};

__device__ __forceinline__ uint32_t qa_byte(float p) {
#pragma clang fp contract(off)
    const float t = rintf(p * 255.0f);                    // one fp32 product, then v_rndne_f32 (half to even)
    if (!(t > 0.f)) return 0u;                            // negatives, -0, and NaN (every comparison with NaN is false)
    return t >= 255.f ? 255u : (uint32_t)t;
}
}  // namespace

// grid (blocks over the plane, frames, objects); V = pixels per lane: 4 = one 16-byte load and one 4-byte store, consecutive across the wave
template <int V>
__global__ __launch_bounds__(256) void qa_quantize_kernel(QaQuantArgs a) {
    const unsigned i0 = (blockIdx.x * 256u + threadIdx.x) * V;            // H * W < 2^31 (checked by the launcher)
    if (i0 >= (unsigned)a.hw) return;
    const int f = blockIdx.y, o = blockIdx.z;
    const float* src = a.probs + (size_t)f * a.sn + (size_t)(o + 1) * a.sc + i0;
    uint8_t* dst = a.planes + ((size_t)o * a.n + f) * a.hw + i0;
    float v[V];
    int q[V];
    load_group(src, v);
#pragma unroll
    for (int p = 0; p < V; ++p) q[p] = (int)qa_byte(v[p]);
    store_bytes(dst, q);
}

}  // namespace ivosw

extern "C" int ivosw_qa_quantize(const float* probs, int n_frames, int n_obj, int H, int W, long probs_stride_n, long probs_stride_c,
                                 uint8_t* planes, ivosw_stream_t stream) {
    using namespace ivosw;
    IVOSW_REQUIRE(probs && planes, "null pointer");
    IVOSW_REQUIRE(n_frames > 0 && n_frames <= 65535 && n_obj > 0 && n_obj <= 65535 && H > 0 && W > 0, "bad shape");
    IVOSW_REQUIRE((long)H * W < (1L << 31), "frame too large for 32-bit pixel indices");
    IVOSW_REQUIRE(probs_stride_c >= (long)H * W && probs_stride_n >= (long)H * W, "probability strides overlap");
    IVOSW_ON_DEVICE_OF(planes);
    QaQuantArgs a{};
    a.probs = probs; a.sn = probs_stride_n; a.sc = probs_stride_c; a.planes = planes; a.n = n_frames; a.hw = H * W;
    const int V = !scalar_forced("IVOSW_QA_SCALAR") && multiples_of(4, a.hw, probs_stride_n, probs_stride_c) && on_grid(16, probs) && on_grid(4, planes) ? 4 : 1;
    const dim3 grid(lane_blocks(a.hw, V), n_frames, n_obj);
    hipStream_t st = as_stream(stream);
    dispatch_lanes<4, 1>(V, [&](auto v) { hipLaunchKernelGGL(qa_quantize_kernel<decltype(v)::value>, grid, dim3(256), 0, st, a); });
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}
