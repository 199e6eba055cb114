// ATNet segmentation epilogue feeding the assessment path — the ATNet twin of seg_epilogue.hip.
//
// Reference (utils/utils_atnet.py), per visited frame t:
//     output_prob = torch.sigmoid(output_logit); prob_onehot_t = output_prob[:, 0].detach()                     :100-101,123-124
//     prob_onehot_t = (alpha * prob_onehot_t) + ((1 - alpha) * prob_map_of_frames[t])    (propagated frames)    :146-147
//     prob_map_of_frames[t] = prob_onehot_t                                                                     :150
// and per interaction, over the whole propagated range:
//     combine_masks_with_batch(prob_map_of_frames[fore:rear+1], n_obj, th)[:, 0, hpad1:-hpad2, wpad1:-wpad2].cpu().numpy().astype(float)   :152-155
//     all_P = torch.cat([zeros_like(prob_map[:, 0:1]), prob_map], 1)[:, :, hpad1:-hpad2, wpad1:-wpad2]          :158-159
// Here ONE launch per frame reads the logits and the frame's slice of prob_map_of_frames once and writes every consumer's
// copy once: the blended map in place (padded grid), the unblended sigmoid the next forward_TNet call takes as predmask_prev
// (padded grid), and inside the crop window the probability planes straight into an object-major store (channel 1 + o), the
// uint8 label map and the float label plane.  The zero channel, the cat, the strided crop and the float64 host copy go away.
//
// Arithmetic: s = 1 / (1 + expf(-x)) with the library expf and an IEEE division (sigmoid(0) == 0.5f exactly; 1 for large x,
// 0 once expf overflows: finite in [0, 1] for every finite logit).  The blend is three separately rounded fp32 operations,
// as torch's three ops are: no FMA contraction (#pragma clang fp contract(off), bare operators: see seg_epilogue.hip).
// Label of a pixel: o* = the first index of max_o p[o]; o* + 1 if p[o*] > th (strictly), else 0.  This rule is the DEFINITION
// here: it restates combine_masks_with_batch of the ATNet clone's libs/utils_torch.py, which is not part of the reference
// tree, so parity with the clone is unpinned (as the J/F kernels' parity with davisinteractive is).  NaN logits: unspecified.
//
// HBM-bound: 4 B x n_obj x (2 reads + 2 writes on the padded grid + 1 write in the crop) + 5 B of labels per pixel.
#include "lane_group.h"
#include <limits.h>

namespace ivosw {

namespace {
struct AtnetArgs {
    const float* logits;   // [n_obj][PH][PW] or nullptr (p = old, the map is not written)
    float* map;            // [n_obj][PH][PW], read (blend / no logits) and written (logits) in place
    float* prob_pad;       // [n_obj][PH][PW] or nullptr: the unblended sigmoid
    float* probs;          // object o's crop plane at probs + o * sc, or nullptr
    long sc;
    uint8_t* label_u8;     // [H][W] or nullptr
    float* label_f32;      // [H][W] or nullptr
    int n_obj, PH, PW, hpad1, wpad1, H, W, blend;
    float alpha, beta, th;
};

__device__ __forceinline__ float sigmoidf(float x) { return 1.0f / (1.0f + expf(-x)); }
}  // namespace

// V = padded pixels per thread, consecutive in a padded row (V = 4 needs PW % 4 == 0 and 16-byte aligned padded planes).
// CROPV: the cropped outputs of a V = 4 group go out as one 16 / 16 / 4-byte store - the launcher grants it only when wpad1
// and W are multiples of 4 (a group is then wholly inside or wholly outside the window, and its cropped index is a multiple
// of 4) and the cropped pointers and the channel stride are aligned; otherwise the padded streams stay 16-byte wide and the
// cropped ones are written element by element.
template <int V, bool CROPV>
__global__ __launch_bounds__(256) void atnet_epilogue_kernel(AtnetArgs a) {
#pragma clang fp contract(off)
    const unsigned idx0 = (blockIdx.x * 256u + threadIdx.x) * V;          // PH * PW <= INT_MAX (checked by the launcher)
    const unsigned plane = (unsigned)a.PH * (unsigned)a.PW;
    if (idx0 >= plane) return;
    const unsigned y = idx0 / (unsigned)a.PW, x0 = idx0 - y * (unsigned)a.PW;          // a V = 4 group never leaves its row
    const int cy = (int)y - a.hpad1;
    const bool row_in = cy >= 0 && cy < a.H;
    const bool any_out = a.probs || a.label_u8 || a.label_f32;
    if (!a.logits && !row_in) return;                                    // rebuild mode touches the window only
    bool in[V];
    bool some = false;
#pragma unroll
    for (int p = 0; p < V; ++p) {
        const int cx = (int)x0 + p - a.wpad1;
        in[p] = row_in && cx >= 0 && cx < a.W;
        some |= in[p];
    }
    if (!a.logits && !some) return;
    const long cidx0 = (long)cy * a.W + ((int)x0 - a.wpad1);             // cropped index of pixel 0 (used where in[p] only)
    float best[V];
    int am[V];
    for (int o = 0; o < a.n_obj; ++o) {
        const size_t off = (size_t)o * plane + idx0;
        float pv[V];
        if (a.logits) {
            float s[V];
            load_group(a.logits + off, s);
#pragma unroll
            for (int p = 0; p < V; ++p) s[p] = sigmoidf(s[p]);
            if (a.blend) {
                float old[V];
                load_group(a.map + off, old);
#pragma unroll
                for (int p = 0; p < V; ++p) {
                    const float m1 = a.alpha * s[p];
                    const float m2 = a.beta * old[p];
                    pv[p] = m1 + m2;
                }
            } else {
#pragma unroll
                for (int p = 0; p < V; ++p) pv[p] = s[p];
            }
            store_group(a.map + off, pv);
            if (a.prob_pad) store_group(a.prob_pad + off, s);
        } else {
            load_group(a.map + off, pv);
        }
        if (!some || !any_out) continue;
#pragma unroll
        for (int p = 0; p < V; ++p)
            if (o == 0 || pv[p] > best[p]) { best[p] = pv[p]; am[p] = o; }           // running FIRST maximum
        if (a.probs) {
            float* out = a.probs + (size_t)o * a.sc + cidx0;
            if (CROPV) {
                store_group(out, pv);
            } else {
#pragma unroll
                for (int p = 0; p < V; ++p)
                    if (in[p]) out[p] = pv[p];
            }
        }
    }
    if (!some || !any_out) return;
    int lab[V];
#pragma unroll
    for (int p = 0; p < V; ++p) lab[p] = best[p] > a.th ? am[p] + 1 : 0;
    if (CROPV) {
        if (a.label_u8) store_bytes(a.label_u8 + cidx0, lab);
        if (a.label_f32) store_group_as(a.label_f32 + cidx0, lab);
    } else {
#pragma unroll
        for (int p = 0; p < V; ++p)
            if (in[p]) {
                if (a.label_u8) a.label_u8[cidx0 + p] = (uint8_t)lab[p];
                if (a.label_f32) a.label_f32[cidx0 + p] = (float)lab[p];
            }
    }
}

}  // namespace ivosw

extern "C" int ivosw_atnet_epilogue(const float* logits, float* prob_map_t, int n_obj, int PH, int PW, int hpad1, int wpad1,
                                    int H, int W, int blend, float alpha32, float beta32, float th, float* prob_pad,
                                    float* probs, long probs_stride_c, uint8_t* label_u8, float* label_f32,
                                    ivosw_stream_t stream) {
    using namespace ivosw;
    IVOSW_REQUIRE(prob_map_t, "null prob_map_t");
    IVOSW_REQUIRE(n_obj >= 1, "n_obj < 1");
    IVOSW_REQUIRE(!label_u8 || n_obj <= 255, "uint8 labels need n_obj <= 255");
    IVOSW_REQUIRE(H >= 1 && W >= 1 && PH >= 1 && PW >= 1, "bad shape");
    IVOSW_REQUIRE(hpad1 >= 0 && wpad1 >= 0, "negative pad");
    IVOSW_REQUIRE((long)hpad1 + H <= PH && (long)wpad1 + W <= PW, "crop window outside the padded grid");
    IVOSW_REQUIRE((long)PH * PW <= INT_MAX && (long)n_obj * PH * PW <= INT_MAX, "frame too large for 32-bit pixel indices");
    IVOSW_REQUIRE(!probs || n_obj == 1 || probs_stride_c >= (long)H * W, "probability planes overlap");
    IVOSW_REQUIRE(blend == 0 || blend == 1, "blend must be 0 or 1");
    IVOSW_REQUIRE(logits || !blend, "blend needs logits");
    IVOSW_REQUIRE(logits || probs || label_u8 || label_f32, "no output requested");
    IVOSW_ON_DEVICE_OF(prob_map_t);
    AtnetArgs a{};
    a.logits = logits; a.map = prob_map_t; a.prob_pad = logits ? prob_pad : nullptr; a.probs = probs; a.sc = probs_stride_c;
    a.label_u8 = label_u8; a.label_f32 = label_f32;
    a.n_obj = n_obj; a.PH = PH; a.PW = PW; a.hpad1 = hpad1; a.wpad1 = wpad1; a.H = H; a.W = W; a.blend = blend;
    a.alpha = alpha32; a.beta = beta32; a.th = th;
    hipStream_t st = as_stream(stream);
    const int V = !scalar_forced("IVOSW_ATNET_SCALAR") && PW % 4 == 0 && on_grid(16, logits, prob_map_t, a.prob_pad) ? 4 : 1;
    const bool cropv = V == 4 && multiples_of(4, wpad1, W) && on_grid(4, label_u8) && on_grid(16, label_f32, probs) &&
                       (!probs || n_obj == 1 || probs_stride_c % 4 == 0);
    const dim3 grid(lane_blocks((long)PH * PW, V));
    if (cropv) hipLaunchKernelGGL((atnet_epilogue_kernel<4, true>), grid, dim3(256), 0, st, a);
    else dispatch_lanes<4, 1>(V, [&](auto v) { hipLaunchKernelGGL((atnet_epilogue_kernel<decltype(v)::value, false>), grid, dim3(256), 0, st, a); });
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}
