// Assessment training samples, step three: the augmentation of datasets/transforms_assess.py as ONE fused warp on the device.
//
// Reference (datasets/transforms_assess.py): Resize (three cv2.resize), RandomAffine (imgaug crop + affine in a retry loop of up to 12
// tries, np.unique over the warped label after each), AdditiveNoise, RandomContrast, RandomHorizontalFlip, ToTensor - five per-frame host
// loops and a pinned upload per sample.  Here every geometric step is an inverse affine map, the host composes them, and one kernel
// resamples frame, probability plane and label of every sample of a batch through that one map and applies the photometric step; the retry
// loop becomes a selection launch that looks at every candidate's warped label at once, so nothing returns to the host.
//
// The sampling rule of include/ivosw.h ("augmented assessment samples") is the definition; tests/augment_ref.py restates it in numpy.
// Every fp32 operation is rounded by itself (fp contract off, IEEE division), so device and restatement agree bit for bit.
//
// Kernel arguments: the per-sample rows (source pointers resolved on the host from the video table, 13 composed maps of six fp32) travel
// BY VALUE, so the call allocates nothing and copies nothing and is capture-safe.  A row is 360 bytes: AUG_GROUP = 11 rows fill the 4 KB a
// launch carries, so a batch runs in groups of 11 samples (the interface allows up to 64 per launch; the maps do not fit more).  A batch of
// 32 is therefore three selection launches of at most 143 workgroups and three to six warp launches, one after the other: each
// selection launch underfills a 256-CU device (profiles/augment_probe.txt holds what that costs).
// No LDS in the warp pass, no atomics, no scratch.
#include "lane_group.h"

namespace ivosw {

namespace {
constexpr int AUG_MAX_CAND = IVOSW_QA_AUG_MAX_CAND;      // 12
constexpr int AUG_MAPS = AUG_MAX_CAND + 1;               // candidates 0 .. n_cand - 1, then "no candidate" (post alone) at n_cand
constexpr int AUG_GROUP = 11;
constexpr int AUG_SEL_THREADS = 1024;
constexpr int AUG_MAX_SIDE = 1 << 24;                    // source H and W: the kernels compare tap coordinates with them as floats, exact up to here

struct AugRow {
    const void* frame;       // the sample's frame: fp32 [3][H][W] or RGBX8 [H][W][4]
    const uint8_t* gt;       // [H][W]
    const uint8_t* plane;    // [H][W], the object's byte plane
    float m[AUG_MAPS][6];    // composed inverse maps a b c d e f; m[n_cand] is post alone
    float noise, contrast;
    int H, W;
    uint8_t id, kind, n_cand, pad;
};
struct AugArgs {
    AugRow s[AUG_GROUP];
    float *img, *prob;       // of sample 0 of the call
    uint8_t *label, *mask;
    int32_t* chosen;
    uint8_t* flags;          // [N][AUG_MAPS][2] (has a 0, has a 1): written by the selection launch, read by the warp; NULL when no sample
                             // of the call has a candidate
    int s0, ns;              // first sample of this group, samples in it
    int Ho, Wo;
};
static_assert(sizeof(AugArgs) <= 4096, "the sample rows no longer fit the kernel arguments");

struct AugMap { float a, b, c, d, e, f; };

// sx = fl(fl(fl(a x) + fl(b y)) + c), sy likewise
__device__ __forceinline__ void aug_coords(const AugMap& m, float x, float y, float& sx, float& sy) {
#pragma clang fp contract(off)
    sx = (m.a * x + m.b * y) + m.c;
    sy = (m.d * x + m.e * y) + m.f;
}

// nearest tap of the label: (floor(sx + .5), floor(sy + .5)); outside the source 0, inside gt == id
__device__ __forceinline__ int aug_label(const uint8_t* gt, int H, int W, int id, float sx, float sy) {
#pragma clang fp contract(off)
    const float tx = floorf(sx + 0.5f), ty = floorf(sy + 0.5f);
    if (!(tx >= 0.f && tx <= (float)(W - 1) && ty >= 0.f && ty <= (float)(H - 1))) return 0;       // (false for NaN too)
    return gt[(size_t)(int)ty * W + (int)tx] == id;
}

__device__ __forceinline__ float aug_byte(uint32_t b) { return (float)b / 255.0f; }      // IEEE division, correctly rounded

__device__ __forceinline__ float aug_lerp(float v00, float v10, float v01, float v11, float fx, float fy) {
#pragma clang fp contract(off)
    const float top = v00 + fx * (v10 - v00);
    const float bot = v01 + fx * (v11 - v01);
    return top + fy * (bot - top);
}

__device__ __forceinline__ float aug_photo(float v, float noise, float contrast) {
#pragma clang fp contract(off)
    const float t = fminf(fmaxf(v + noise, 0.f), 1.f);
    return fminf(fmaxf(t * contrast, 0.f), 1.f);
}

// the candidate the warp uses: the first whose count of distinct label values equals that of "no candidate", else n_cand
__device__ __forceinline__ int aug_choose(const uint8_t* flags, int s, int n_cand) {
    if (n_cand == 0) return 0;
    const uint8_t* fl = flags + (size_t)s * AUG_MAPS * 2;
    const int want = fl[2 * n_cand] + fl[2 * n_cand + 1];
    int c = 0;
    while (c < n_cand && fl[2 * c] + fl[2 * c + 1] != want) ++c;
    return c;
}
}  // namespace

// Selection: grid (AUG_MAPS, samples of the group); one workgroup per (sample, map) pair walks the Ho x Wo grid through the nearest warp
// and finds whether the label holds a 0 and whether it holds a 1; lane 0 stores the two flag bytes.
__global__ __launch_bounds__(AUG_SEL_THREADS) void qa_augment_select_kernel(AugArgs a) {
    const AugRow& r = a.s[blockIdx.y];
    const int c = blockIdx.x;
    if (r.n_cand == 0 || c > r.n_cand) return;
    const AugMap m{r.m[c][0], r.m[c][1], r.m[c][2], r.m[c][3], r.m[c][4], r.m[c][5]};
    const int n = a.Ho * a.Wo;
    int has0 = 0, has1 = 0;
    for (unsigned i = threadIdx.x; i < (unsigned)n; i += AUG_SEL_THREADS) {
        const int y = i / a.Wo, x = i - y * a.Wo;
        float sx, sy;
        aug_coords(m, (float)x, (float)y, sx, sy);
        const int l = aug_label(r.gt, r.H, r.W, r.id, sx, sy);
        has1 |= l;
        has0 |= l ^ 1;
    }
    has0 = __syncthreads_or(has0);
    has1 = __syncthreads_or(has1);
    if (threadIdx.x == 0) {
        uint8_t* fl = a.flags + ((size_t)(a.s0 + blockIdx.y) * AUG_MAPS + c) * 2;
        fl[0] = has0 ? 1 : 0;
        fl[1] = has1 ? 1 : 0;
    }
}

// Warp: grid (blocks over the Ho x Wo grid, samples of the group), one destination pixel per lane.  KIND = the frame source of the samples
// this launch serves (a workgroup whose sample is of the other kind leaves at once).  Four pixels of a row per lane with float4 stores
// were built and measured: a lane's four taps spread a wave's gathers over four times the addresses per load, 220 against 121 us at
// 480 x 856 x 32 samples on fp32 frames, so one pixel per lane is the only path.
template <int KIND>
__global__ __launch_bounds__(256) void qa_augment_warp_kernel(AugArgs a) {
    const AugRow& r = a.s[blockIdx.y];
    if (r.kind != KIND) return;
    const int s = a.s0 + blockIdx.y;
    const int n = a.Ho * a.Wo;
    const int pick = aug_choose(a.flags, s, r.n_cand);
    if (blockIdx.x == 0 && threadIdx.x == 0) a.chosen[s] = pick;
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (unsigned)n) return;
    const AugMap m{r.m[pick][0], r.m[pick][1], r.m[pick][2], r.m[pick][3], r.m[pick][4], r.m[pick][5]};
    const int H = r.H, W = r.W;                                            // both <= 2^24 (checked by the launcher): exact as floats
    const int y = i / a.Wo, x = i - y * a.Wo;
    const float xmax = (float)(W - 1), ymax = (float)(H - 1);
    const size_t hw = (size_t)H * W;
    float sx, sy;
    aug_coords(m, (float)x, (float)y, sx, sy);
    const int lab = aug_label(r.gt, H, W, r.id, sx, sy);
    const float x0f = floorf(sx), y0f = floorf(sy);
    const float fx = sx - x0f, fy = sy - y0f;
    // tap validity in float (a far-away or NaN coordinate converts to no int); the int taps are formed from clamped values
    const bool xin0 = x0f >= 0.f && x0f <= xmax, xin1 = x0f >= -1.f && x0f <= xmax - 1.f;
    const bool yin0 = y0f >= 0.f && y0f <= ymax, yin1 = y0f >= -1.f && y0f <= ymax - 1.f;
    const int x0 = (int)fminf(fmaxf(x0f, -1.f), xmax), y0 = (int)fminf(fmaxf(y0f, -1.f), ymax);
    const bool in[4] = {xin0 && yin0, xin1 && yin0, xin0 && yin1, xin1 && yin1};
    size_t at[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) at[t] = in[t] ? (size_t)(y0 + (t >> 1)) * W + (x0 + (t & 1)) : 0;
    float v[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) v[t] = in[t] ? aug_byte(r.plane[at[t]]) : 0.f;
    const float pr = aug_lerp(v[0], v[1], v[2], v[3], fx, fy);
    float col[3];
    if constexpr (KIND == IVOSW_FRAMES_RGBX8) {
        uint32_t w[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) w[t] = in[t] ? reinterpret_cast<const uint32_t*>(r.frame)[at[t]] : 0u;      // bytes R G B X: one load per tap
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
#pragma unroll
            for (int t = 0; t < 4; ++t) v[t] = aug_byte((w[t] >> (8 * ch)) & 255u);          // (byte 0 of an outside tap: 0 / 255 = 0)
            col[ch] = aug_photo(aug_lerp(v[0], v[1], v[2], v[3], fx, fy), r.noise, r.contrast);
        }
    } else {
        const float* fr = reinterpret_cast<const float*>(r.frame);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
#pragma unroll
            for (int t = 0; t < 4; ++t) v[t] = in[t] ? fr[ch * hw + at[t]] : 0.f;
            col[ch] = aug_photo(aug_lerp(v[0], v[1], v[2], v[3], fx, fy), r.noise, r.contrast);
        }
    }
    const size_t o1 = (size_t)s * n + i;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) a.img[((size_t)s * 3 + ch) * n + i] = col[ch];
    a.prob[o1] = pr;
    a.label[o1] = (uint8_t)lab;
    a.mask[o1] = pr > 0.8f ? 255 : 0;
}

namespace {
bool aug_video_ok(const ivosw_qa_aug_video_t& v) {
    return v.frames && v.gt && v.planes && v.n_frames >= 1 && v.H >= 1 && v.W >= 1 && v.H <= AUG_MAX_SIDE && v.W <= AUG_MAX_SIDE && (long)v.H * v.W < (1L << 31) && v.n_obj >= 1 && v.n_obj <= 32;
}
bool aug_finite(float v) {                     // exponent bits not all ones
    uint32_t u;
    memcpy(&u, &v, 4);
    return (u & 0x7f800000u) != 0x7f800000u;
}
bool ranges_overlap(const void* p, size_t n, const void* q, size_t k) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + k && b < a + n;
}
}  // namespace

}  // namespace ivosw

extern "C" size_t ivosw_qa_augment_ws_bytes(int n_samples) {
    if (n_samples < 1 || n_samples > IVOSW_QA_AUG_MAX_SAMPLES) return 0;
    return (size_t)n_samples * ivosw::AUG_MAPS * 2;
}

extern "C" int ivosw_qa_augment(const ivosw_qa_aug_video_t* videos, int n_videos, const ivosw_qa_aug_sample_t* samples_host, int n_samples,
                                int Ho, int Wo, float* img, float* prob, uint8_t* label, uint8_t* mask, int32_t* chosen, void* ws,
                                size_t ws_bytes, ivosw_stream_t stream) {
#pragma clang fp contract(off)
    using namespace ivosw;
    IVOSW_REQUIRE(videos, "null videos");
    IVOSW_REQUIRE(samples_host, "null samples_host");
    IVOSW_REQUIRE(img, "null img");
    IVOSW_REQUIRE(prob, "null prob");
    IVOSW_REQUIRE(label, "null label");
    IVOSW_REQUIRE(mask, "null mask");
    IVOSW_REQUIRE(chosen, "null chosen");
    if (n_videos < 1 || n_videos > IVOSW_MAX_JF_VIDEOS) {
        set_error("%s: n_videos %d outside [1, %d]", __func__, n_videos, IVOSW_MAX_JF_VIDEOS);
        return IVOSW_ERR_ARG;
    }
    if (n_samples < 1 || n_samples > IVOSW_QA_AUG_MAX_SAMPLES) {
        set_error("%s: n_samples %d outside [1, %d]", __func__, n_samples, IVOSW_QA_AUG_MAX_SAMPLES);
        return IVOSW_ERR_ARG;
    }
    if (Ho < 1 || Ho > 65535 || Wo < 1 || Wo > 65535) {
        set_error("%s: Ho x Wo = %d x %d: each must lie in [1, 65535]", __func__, Ho, Wo);
        return IVOSW_ERR_ARG;
    }
    IVOSW_REQUIRE((long)Ho * Wo < (1L << 31), "Ho * Wo: output too large for 32-bit pixel indices");
    const size_t n = (size_t)Ho * Wo, N = (size_t)n_samples;
    const void* outs[5] = {img, prob, label, mask, chosen};
    const size_t out_bytes[5] = {N * 3 * n * 4, N * n * 4, N * n, N * n, N * 4};
    const char* out_names[5] = {"img", "prob", "label", "mask", "chosen"};
    for (int v = 0; v < n_videos; ++v) {
        const ivosw_qa_aug_video_t& d = videos[v];
        if (d.frames_kind != IVOSW_FRAMES_F32 && d.frames_kind != IVOSW_FRAMES_RGBX8) {
            set_error("%s: videos: video %d: unknown frames_kind %d", __func__, v, d.frames_kind);
            return IVOSW_ERR_ARG;
        }
        if (!aug_video_ok(d)) {
            set_error("%s: videos: video %d: null frames / gt / planes, n_frames, H or W < 1, H or W > 2^24, H * W >= 2^31, or n_obj outside 1 .. 32", __func__, v);
            return IVOSW_ERR_ARG;
        }
        if (!on_grid(4, (const char*)d.frames)) {
            set_error("%s: videos: video %d: frames off the 4-byte grid", __func__, v);
            return IVOSW_ERR_ARG;
        }
        const size_t hw = (size_t)d.H * d.W;
        const void* src[3] = {d.frames, d.gt, d.planes};
        const size_t src_bytes[3] = {hw * d.n_frames * (d.frames_kind == IVOSW_FRAMES_F32 ? 12 : 4), hw * d.n_frames, hw * d.n_frames * d.n_obj};
        const char* src_names[3] = {"frames", "gt", "planes"};
        for (int o = 0; o < 5; ++o)
            for (int k = 0; k < 3; ++k)
                if (ranges_overlap(outs[o], out_bytes[o], src[k], src_bytes[k])) {
                    set_error("%s: %s overlaps the %s of video %d", __func__, out_names[o], src_names[k], v);
                    return IVOSW_ERR_ARG;
                }
    }
    bool any_cand = false;
    for (int k = 0; k < n_samples; ++k) {
        const ivosw_qa_aug_sample_t& q = samples_host[k];
        if (q.v < 0 || q.v >= n_videos) {
            set_error("%s: samples_host: sample %d: video %d outside [0, %d)", __func__, k, q.v, n_videos);
            return IVOSW_ERR_ARG;
        }
        if (q.f < 0 || q.f >= videos[q.v].n_frames) {
            set_error("%s: samples_host: sample %d: frame %d outside [0, %d)", __func__, k, q.f, videos[q.v].n_frames);
            return IVOSW_ERR_ARG;
        }
        if (q.o < 0 || q.o >= videos[q.v].n_obj) {
            set_error("%s: samples_host: sample %d: object %d outside [0, %d)", __func__, k, q.o, videos[q.v].n_obj);
            return IVOSW_ERR_ARG;
        }
        if (q.n_cand < 0 || q.n_cand > AUG_MAX_CAND) {
            set_error("%s: samples_host: sample %d: n_cand %d outside [0, %d]", __func__, k, q.n_cand, AUG_MAX_CAND);
            return IVOSW_ERR_ARG;
        }
        bool finite = aug_finite(q.noise) && aug_finite(q.contrast);
        for (int j = 0; j < 6; ++j) finite = finite && aug_finite(q.post[j]);
        for (int c = 0; c < q.n_cand; ++c)
            for (int j = 0; j < 6; ++j) finite = finite && aug_finite(q.cand[c][j]);
        if (!finite) {
            set_error("%s: samples_host: sample %d: a map entry, noise or contrast is not finite", __func__, k);
            return IVOSW_ERR_ARG;
        }
        any_cand = any_cand || q.n_cand > 0;
    }
    const size_t need = any_cand ? ivosw_qa_augment_ws_bytes(n_samples) : 0;
    if (any_cand && (!ws || ws_bytes < need)) {
        set_error("%s: ws: workspace %zu < %zu", __func__, ws ? ws_bytes : (size_t)0, need);
        return IVOSW_ERR_ARG;
    }
    for (int o = 0; any_cand && o < 5; ++o)
        if (ranges_overlap(outs[o], out_bytes[o], ws, need)) {
            set_error("%s: %s overlaps ws", __func__, out_names[o]);
            return IVOSW_ERR_ARG;
        }
    for (int v = 0; any_cand && v < n_videos; ++v) {                       // the selection launch writes ws: it may alias no source either
        const ivosw_qa_aug_video_t& d = videos[v];
        const size_t hw = (size_t)d.H * d.W;
        const void* src[3] = {d.frames, d.gt, d.planes};
        const size_t src_bytes[3] = {hw * d.n_frames * (d.frames_kind == IVOSW_FRAMES_F32 ? 12 : 4), hw * d.n_frames, hw * d.n_frames * d.n_obj};
        const char* src_names[3] = {"frames", "gt", "planes"};
        for (int k = 0; k < 3; ++k)
            if (ranges_overlap(ws, need, src[k], src_bytes[k])) {
                set_error("%s: ws overlaps the %s of video %d", __func__, src_names[k], v);
                return IVOSW_ERR_ARG;
            }
    }
    IVOSW_ON_DEVICE_OF(img);

    hipStream_t st = as_stream(stream);
    AugArgs a{};
    a.img = img; a.prob = prob; a.label = label; a.mask = mask; a.chosen = chosen;
    a.flags = any_cand ? static_cast<uint8_t*>(ws) : nullptr;
    a.Ho = Ho; a.Wo = Wo;
    for (int g0 = 0; g0 < n_samples; g0 += AUG_GROUP) {
        a.s0 = g0;
        a.ns = n_samples - g0 < AUG_GROUP ? n_samples - g0 : AUG_GROUP;
        bool kinds[2] = {false, false}, cand = false;
        for (int k = 0; k < a.ns; ++k) {
            const ivosw_qa_aug_sample_t& q = samples_host[g0 + k];
            const ivosw_qa_aug_video_t& d = videos[q.v];
            const size_t hw = (size_t)d.H * d.W;
            AugRow& r = a.s[k];
            r.frame = (const char*)d.frames + hw * q.f * (d.frames_kind == IVOSW_FRAMES_F32 ? 12 : 4);
            r.gt = d.gt + hw * q.f;
            r.plane = d.planes + hw * ((size_t)q.o * d.n_frames + q.f);
            r.noise = q.noise; r.contrast = q.contrast;
            r.H = d.H; r.W = d.W;
            r.id = d.obj_ids[q.o]; r.kind = (uint8_t)d.frames_kind; r.n_cand = (uint8_t)q.n_cand; r.pad = 0;
            // full = candidate after post: composed in float64, rounded to fp32 once
            const double pa = q.post[0], pb = q.post[1], pc = q.post[2], pd = q.post[3], pe = q.post[4], pf = q.post[5];
            for (int c = 0; c < q.n_cand; ++c) {
                const double ca = q.cand[c][0], cb = q.cand[c][1], cc = q.cand[c][2], cd = q.cand[c][3], ce = q.cand[c][4], cf = q.cand[c][5];
                r.m[c][0] = (float)(ca * pa + cb * pd);
                r.m[c][1] = (float)(ca * pb + cb * pe);
                r.m[c][2] = (float)((ca * pc + cb * pf) + cc);
                r.m[c][3] = (float)(cd * pa + ce * pd);
                r.m[c][4] = (float)(cd * pb + ce * pe);
                r.m[c][5] = (float)((cd * pc + ce * pf) + cf);
            }
            for (int j = 0; j < 6; ++j) r.m[q.n_cand][j] = q.post[j];
            kinds[d.frames_kind] = true;
            cand = cand || q.n_cand > 0;
        }
        if (cand)
            hipLaunchKernelGGL(qa_augment_select_kernel, dim3(AUG_MAPS, a.ns), dim3(AUG_SEL_THREADS), 0, st, a);
        const dim3 grid(lane_blocks((long)n, 1), a.ns);
        if (kinds[IVOSW_FRAMES_F32]) hipLaunchKernelGGL(qa_augment_warp_kernel<IVOSW_FRAMES_F32>, grid, dim3(256), 0, st, a);
        if (kinds[IVOSW_FRAMES_RGBX8]) hipLaunchKernelGGL(qa_augment_warp_kernel<IVOSW_FRAMES_RGBX8>, grid, dim3(256), 0, st, a);
    }
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}
