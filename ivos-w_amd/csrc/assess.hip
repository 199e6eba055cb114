// AssessNet.forward on the MI355X: plan of the 54-conv tower, weight packing, chunked execution.
//
// Reference: AssessNet.forward (models/assessment.py:164-182), Encoder (:12-63), torchvision ResNet-50 v1.5.
// Frames run through the tower in chunks (default 256 bf16 / 64 fp32 frames at res2, doubling per stage).  Chunks
// bound the workspace; they are NOT a cache-residency device: an Infinity-Cache-sized working set streams at
// ~7 TB/s against ~6 TB/s from HBM (tools/ubench/dma_bench), while small launches cost occupancy, so the bf16
// default is as large as the benchmark batch.  In bf16 mode the stride-1 bottlenecks of res2 run as ONE fused kernel
// each (bottleneck.hip); everything else is layer by layer (conv.hip).
#ifdef IVOSW_PROBES
#include "../../include/ivosw_probe.h"
#endif
#include <limits.h>
#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "conv.h"
#include "front.h"

namespace ivosw {

struct ConvPlan {
    int Cin, Cout, K, stride, pad;  // K = kernel size (1 or 3)
    int t_w, t_bn;                  // state_dict indices: conv weight; bn weight (bias, mean, var follow)
    size_t w_off, b_off;            // byte offsets into the packed arena
    size_t fw_off;                  // bf16: 1x1 weights in MFMA-operand order for conv1x1_wide_kernel (0 = none)
};

struct BlockPlan {
    int c1, c2, c3, ds;  // indices into convs (ds = -1 if none)
    size_t cat_fw_off;            // bf16: the concatenated weights in MFMA-operand order
    size_t cat_w_off, cat_b_off;  // first blocks: conv3 | downsample concatenated along K, bias sum (conv3 absorbs the downsample conv)
    size_t f1_off, f2_off, f3_off;  // bf16, identity blocks: conv1/2/3 weights in MFMA-operand order (0 = none)
    size_t fwd1_off;                // bf16, res3's first block: conv1 in MFMA-operand order for res2's last block (conv1 forwarding)
};

struct Plan {
    std::vector<ConvPlan> convs;
    std::vector<BlockPlan> blocks;
    size_t norm_off, zero_off, fcw_off, fcb_off, stem_w_off, stem_b_off, total;
    size_t chain_off = 0;           // bf16: res2's weight-fragment stream for res2_chain_kernel (0 = none)
    int t_stem_w3, t_stem_w1, t_stem_bn, t_fcw, t_fcb, t_mean, t_std;
};

static Plan make_plan(int dtype) {
    Plan P;
    const size_t es = (dtype == IVOSW_BF16) ? 2 : 4;
    size_t off = 0;
    auto take = [&](size_t bytes) { off = align_up(off, 256); const size_t o = off; off += bytes; return o; };
    P.norm_off = take(8 * sizeof(float));
    P.zero_off = take(256);  // page of zeros: source of zero-padding taps for the LDS-DMA conv loader
    P.fcw_off = take(2048 * sizeof(float));
    P.fcb_off = take(sizeof(float));
    P.stem_w_off = take((size_t)64 * ((dtype == IVOSW_BF16) ? 256 : 224) * es);
    P.stem_b_off = take(64 * sizeof(float));
    // state_dict order: 0 mean, 1 std, 2 conv1_m.w, 3 conv1_m.b, 4 conv1_p.w, 5 conv1_n.w,
    // 6 conv1.w, 7..11 bn1.{w,b,rm,rv,nbt}, then per block conv1.w, bn1x5, conv2.w, bn2x5, conv3.w, bn3x5,
    // [downsample.0.w, downsample.1x5], finally fc1.w, fc1.b
    P.t_mean = 0; P.t_std = 1; P.t_stem_w1 = 4; P.t_stem_w3 = 6; P.t_stem_bn = 7;
    int t = 12;
    const int nblk[4] = {3, 4, 6, 3}, planes[4] = {64, 128, 256, 512}, strides[4] = {1, 2, 2, 2};
    int inpl = 64;
    auto add = [&](int cin, int cout, int k, int stride) {
        ConvPlan c{};
        c.Cin = cin; c.Cout = cout; c.K = k; c.stride = stride; c.pad = (k == 3) ? 1 : 0;
        c.t_w = t; c.t_bn = t + 1; t += 6;
        c.w_off = take((size_t)cout * k * k * cin * es);
        c.b_off = take((size_t)cout * sizeof(float));
        if (dtype == IVOSW_BF16 && k == 1 && cout % 256 == 0 && cin >= 384) c.fw_off = take((size_t)cout * cin * es);
        P.convs.push_back(c);
        return (int)P.convs.size() - 1;
    };
    for (int s = 0; s < 4; ++s)
        for (int b = 0; b < nblk[s]; ++b) {
            const int st = (b == 0) ? strides[s] : 1;
            BlockPlan bp{};
            bp.c1 = add(inpl, planes[s], 1, 1);
            bp.c2 = add(planes[s], planes[s], 3, st);
            bp.c3 = add(planes[s], planes[s] * 4, 1, 1);
            bp.ds = (b == 0) ? add(inpl, planes[s] * 4, 1, st) : -1;
            if (b == 0) {
                bp.cat_w_off = take((size_t)planes[s] * 4 * (planes[s] + inpl) * es);
                bp.cat_b_off = take((size_t)planes[s] * 4 * sizeof(float));
                if (dtype == IVOSW_BF16 && (planes[s] + inpl >= 384 || s == 0)) bp.cat_fw_off = take((size_t)planes[s] * 4 * (planes[s] + inpl) * es);
                if (dtype == IVOSW_BF16 && s == 0) {     // res2's first block (stride 1) is fused as a whole, too
                    bp.f1_off = take((size_t)planes[s] * inpl * es);
                    bp.f2_off = take((size_t)planes[s] * 9 * planes[s] * es);
                }
                if (dtype == IVOSW_BF16 && s == 1) {     // res3's first 1x1 runs inside res2's last block (conv1 forwarding)
                    bp.fwd1_off = take((size_t)planes[s] * inpl * es);
                    bp.f2_off = take((size_t)planes[s] * 9 * planes[s] * es);    // ... and the rest of the block in stage_first_kernel
                }
            } else if (dtype == IVOSW_BF16) {
                bp.f1_off = take((size_t)planes[s] * inpl * es);
                bp.f2_off = take((size_t)planes[s] * 9 * planes[s] * es);
                bp.f3_off = take((size_t)planes[s] * 4 * planes[s] * es);
            }
            P.blocks.push_back(bp);
            inpl = planes[s] * 4;
        }
    P.t_fcw = t; P.t_fcb = t + 1;
    if (dtype == IVOSW_BF16) P.chain_off = take(res2_chain_stream_bytes());
    P.total = align_up(off, 256);
    return P;
}

// weights of the res2 stage kernel (res2_stage.hip) out of the packed bf16 arena
// A fragment copy the plan does not hold has offset 0: its pointer stays NULL (base + 0 would silently be the first weights of the
// arena), which is what res2_stage_ok() looks at before the per-block kernels / the probe's error take over.
static Res2StageArgs res2_stage_args(const Plan& P, const char* base) {
    Res2StageArgs q{};
    auto at = [&](size_t off) -> const void* { return off ? base + off : nullptr; };
    q.zeros = at(P.zero_off);
    for (int b = 0; b < 3; ++b) {
        const BlockPlan& bp = P.blocks[b];
        const BlockPlan& nx = P.blocks[b + 1];
        q.fb[b] = at(bp.f2_off); q.bb[b] = reinterpret_cast<const float*>(base + P.convs[bp.c2].b_off);
        q.fc[b] = at(b == 0 ? bp.cat_fw_off : bp.f3_off);
        q.bc[b] = static_cast<const float*>(b == 0 ? at(bp.cat_b_off) : base + P.convs[bp.c3].b_off);
        q.fd[b] = at(b == 2 ? nx.fwd1_off : nx.f1_off); q.bd[b] = reinterpret_cast<const float*>(base + P.convs[nx.c1].b_off);
    }
    q.fa0 = at(P.blocks[0].f1_off); q.ba0 = reinterpret_cast<const float*>(base + P.convs[P.blocks[0].c1].b_off);
    return q;
}

static const Plan& plan_for(int dtype) {
    static const Plan pb = make_plan(IVOSW_BF16), pf = make_plan(IVOSW_F32);
    return dtype == IVOSW_BF16 ? pb : pf;
}

__global__ void copy_small_kernel(const float* __restrict__ a, int na, const float* __restrict__ b, int nb, float* __restrict__ o) {
    const int i = threadIdx.x;
    if (i < na) o[i] = a[i];
    if (i < nb) o[na + i] = b[i];
}

// per-frame element counts
constexpr size_t E_ROI = 256 * 256 * 4, E_BIG = 64 * 64 * 256;
// per-frame output elements of res2..res5
constexpr size_t E_OUT[4] = {64 * 64 * 256, 32 * 32 * 512, 16 * 16 * 1024, 8 * 8 * 2048};

// Chunk schedule.  Stage s (res2..res5) runs on c0 * 2^s frames at a time: every stage halves H and W and
// doubles C, so doubling the frames per launch keeps the per-stage tensor size constant (c0 * 2 MB bf16) and every
// conv launch keeps >= 512 workgroups for the 256 CUs.
// fp32 modes: 16 -> 64 frames per res2 launch = 6.8 k -> 9.9 k frames/s; 128 (round 6): fp32 9.96 k, the three-pass mode 21.32 -> 21.57 k (two alternating rounds), at
// twice the workspace (11.5 instead of 5.75 GiB at batch 256 - of 288 GB)
static int default_chunk(int dtype) { return dtype == IVOSW_BF16 ? 256 : std::max(1, tune_get("F32_CHUNK", 128)); }

struct Bufs {
    float* yxhw; int32_t* box; float* pooled;
    char *roi, *stem, *pa, *pb, *m1, *m2, *ds;
    char* in[4];  // in[s]: input of stage s+1 = output of stage s, for the frames of the enclosing chunk (s = 0..2)
};

static size_t carve(Arena& ar, int dtype, int B, int c0, Bufs* out) {
    const size_t es = (dtype == IVOSW_BF16) ? 2 : 4;
    Bufs b{};
    const size_t c3 = (size_t)std::min(B, c0 * 8);
    b.yxhw = ar.take<float>((size_t)B * 4);
    b.box = ar.take<int32_t>((size_t)B * 4);
    b.pooled = ar.take<float>(c3 * 2048);
    b.roi = ar.take<char>(c0 * E_ROI * es);
    b.stem = ar.take<char>(c0 * E_BIG * es);
    b.pa = ar.take<char>(c0 * E_BIG * es);
    b.pb = ar.take<char>(c0 * E_BIG * es);
    b.ds = ar.take<char>(c0 * E_BIG * es);
    b.m1 = ar.take<char>(c0 * E_BIG * es);
    b.m2 = ar.take<char>(c0 * E_BIG / 4 * es);
    for (int s = 0; s < 3; ++s) b.in[s] = ar.take<char>((size_t)c0 * 2 * E_BIG * es);
    b.in[3] = nullptr;
    if (out) *out = b;
    return align_up(ar.off, 256);
}

}  // namespace ivosw

using namespace ivosw;

// Which precision an arena was packed for (IVOSW_F32 and IVOSW_F32X3 share plan, sizes and layout, but the x3 pack
// rewrites every weight K-tile in place as [hi | lo] bf16 - a forward call with the other dtype passed every check and returned
// garbage).  The tag lives in two places: float slot 6 of the arena's 8-float normalisation block (for whoever inspects or copies
// an arena) and a host-side table keyed by the arena's address, which the forward entry points check without touching the device.
static std::mutex g_pack_mu;
static std::vector<std::pair<const void*, int>> g_pack_dtype;
static void pack_dtype_record(const void* packed, int dtype) {
    std::lock_guard<std::mutex> lock(g_pack_mu);
    for (auto& e : g_pack_dtype)
        if (e.first == packed) { e.second = dtype; return; }
    g_pack_dtype.emplace_back(packed, dtype);
}
// The check covers arenas whose tag this process knows: packed here (recorded at pack time) or seen before.  An address the table does not
// hold - an arena filled by a device copy, or through the C ABI from another library instance - is looked up ONCE in the arena itself (the
// 4-byte device tag, a blocking copy on the caller's stream: first use only) and cached.  -1: no valid tag, not checkable.
// ivosw_assess_forget() drops an address when its memory is freed or reused for an arena of another precision by a device copy.
static int pack_dtype_lookup(const void* packed, hipStream_t st = nullptr) {
    {
        std::lock_guard<std::mutex> lock(g_pack_mu);
        for (auto& e : g_pack_dtype)
            if (e.first == packed) return e.second;
    }
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (st && hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) return -1;      // no blocking copy inside a capture
    unsigned tag = 0;
    const char* slot = static_cast<const char*>(packed) + plan_for(IVOSW_BF16).norm_off + 6 * sizeof(float);     // (norm_off is the same in every plan)
    if (hipMemcpyAsync(&tag, slot, sizeof(tag), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) { (void)hipGetLastError(); return -1; }
    const int dtype = (tag >> 16) == 0x4956u && (int)(tag & 0xffffu) <= IVOSW_F32X3 ? (int)(tag & 0xffffu) : -1;
    if (dtype >= 0) pack_dtype_record(packed, dtype);
    return dtype;
}
extern "C" int ivosw_assess_forget(const void* packed) {
    std::lock_guard<std::mutex> lock(g_pack_mu);
    for (size_t i = 0; i < g_pack_dtype.size(); ++i)
        if (g_pack_dtype[i].first == packed) { g_pack_dtype.erase(g_pack_dtype.begin() + i); return IVOSW_OK; }
    return IVOSW_OK;
}

extern "C" size_t ivosw_assess_packed_bytes(int dtype) {
    if (dtype != IVOSW_F32 && dtype != IVOSW_BF16 && dtype != IVOSW_F32X3) return 0;
    return plan_for(dtype).total;
}

extern "C" int ivosw_assess_pack(void* packed, int dtype, const void* const* tensors, int ntensors, ivosw_stream_t stream) {
    IVOSW_REQUIRE(packed && tensors, "null pointer");
    IVOSW_ON_DEVICE_OF(packed);
    IVOSW_REQUIRE(dtype == IVOSW_F32 || dtype == IVOSW_BF16 || dtype == IVOSW_F32X3, "dtype must be IVOSW_F32, IVOSW_BF16 or IVOSW_F32X3");
    IVOSW_REQUIRE(ntensors == IVOSW_ASSESS_NTENSORS, "expected the 326 tensors of AssessNet.state_dict()");
    const Plan& P = plan_for(dtype);
    IVOSW_REQUIRE(P.t_fcb == IVOSW_ASSESS_NTENSORS - 1, "internal: plan/state_dict mismatch");
    hipStream_t st = as_stream(stream);
    char* base = static_cast<char*>(packed);
    auto T = [&](int i) { return static_cast<const float*>(tensors[i]); };
    for (int i : {P.t_mean, P.t_std, P.t_stem_w1, P.t_stem_w3, P.t_fcw, P.t_fcb}) IVOSW_REQUIRE(tensors[i], "null tensor");
    (void)hipMemsetAsync(base + P.zero_off, 0, 256, st);
    hipLaunchKernelGGL(copy_small_kernel, dim3(1), dim3(64), 0, st, T(P.t_mean), 3, T(P.t_std), 3,
                       reinterpret_cast<float*>(base + P.norm_off));
    (void)hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(base + P.norm_off + 6 * sizeof(float)), 0x49560000 | dtype, 1, st);   // 'IV' | dtype
    pack_dtype_record(packed, dtype);
    (void)hipMemcpyAsync(base + P.fcw_off, T(P.t_fcw), 2048 * sizeof(float), hipMemcpyDeviceToDevice, st);
    (void)hipMemcpyAsync(base + P.fcb_off, T(P.t_fcb), sizeof(float), hipMemcpyDeviceToDevice, st);
    launch_pack_stem(T(P.t_stem_w3), T(P.t_stem_w1), T(P.t_stem_bn), T(P.t_stem_bn + 1), T(P.t_stem_bn + 2),
                     T(P.t_stem_bn + 3), dtype, base + P.stem_w_off, reinterpret_cast<float*>(base + P.stem_b_off), st);
    for (const ConvPlan& c : P.convs) {
        for (int j = 0; j < 4; ++j) IVOSW_REQUIRE(tensors[c.t_bn + j] && tensors[c.t_w], "null tensor");
        launch_pack_conv(T(c.t_w), T(c.t_bn), T(c.t_bn + 1), T(c.t_bn + 2), T(c.t_bn + 3), c.Cout, c.Cin, c.K, c.K, dtype,
                         base + c.w_off, reinterpret_cast<float*>(base + c.b_off), st);
    }
    for (const ConvPlan& c : P.convs)
        if (c.fw_off) launch_fragpack(base + c.w_off, c.Cout, c.Cin, base + c.fw_off, st);
    for (const BlockPlan& bp : P.blocks)
        if (bp.f1_off) {
            const ConvPlan &c1 = P.convs[bp.c1], &c2 = P.convs[bp.c2], &c3 = P.convs[bp.c3];
            launch_fragpack(base + c1.w_off, c1.Cout, c1.Cin, base + bp.f1_off, st);
            launch_fragpack(base + c2.w_off, c2.Cout, 9 * c2.Cin, base + bp.f2_off, st);
            if (bp.f3_off) launch_fragpack(base + c3.w_off, c3.Cout, c3.Cin, base + bp.f3_off, st);
        }
    for (const BlockPlan& bp : P.blocks)
        if (bp.fwd1_off) {
            launch_fragpack(base + P.convs[bp.c1].w_off, P.convs[bp.c1].Cout, P.convs[bp.c1].Cin, base + bp.fwd1_off, st);
            if (bp.f2_off && !bp.f1_off) launch_fragpack(base + P.convs[bp.c2].w_off, P.convs[bp.c2].Cout, 9 * P.convs[bp.c2].Cin, base + bp.f2_off, st);
        }
    for (const BlockPlan& bp : P.blocks)
        if (bp.ds >= 0) {
            const ConvPlan &c3 = P.convs[bp.c3], &cd = P.convs[bp.ds];
            launch_concat_k(base + c3.w_off, reinterpret_cast<const float*>(base + c3.b_off), c3.Cin, base + cd.w_off,
                            reinterpret_cast<const float*>(base + cd.b_off), cd.Cin, c3.Cout, dtype, base + bp.cat_w_off,
                            reinterpret_cast<float*>(base + bp.cat_b_off), st);
            if (bp.cat_fw_off) launch_fragpack(base + bp.cat_w_off, c3.Cout, c3.Cin + cd.Cin, base + bp.cat_fw_off, st);
        }
    if (P.chain_off) {
        Res2ChainPackArgs q{};
        auto W = [&](int ci) { return reinterpret_cast<const bf16_t*>(base + P.convs[ci].w_off); };
        auto Bi = [&](int ci) { return reinterpret_cast<const float*>(base + P.convs[ci].b_off); };
        for (int b = 0; b < 4; ++b) { q.w1[b] = W(P.blocks[b].c1); q.b1[b] = Bi(P.blocks[b].c1); }
        for (int b = 0; b < 3; ++b) { q.w2[b] = W(P.blocks[b].c2); q.b2[b] = Bi(P.blocks[b].c2); q.w3[b] = W(P.blocks[b].c3); q.b3[b] = Bi(P.blocks[b].c3); }
        q.wd = W(P.blocks[0].ds); q.bd = Bi(P.blocks[0].ds);
        q.out = base + P.chain_off;
        launch_res2_chain_pack(q, st);
    }
    if (dtype == IVOSW_F32X3) {
        // the three-pass mode reads pre-split weights (conv.hip: ktile_mma_x3): every conv's K-major array and the concatenated
        // [conv3 | downsample] arrays, in place, AFTER everything that read them as fp32 (the concatenation above)
        launch_split_weights_x3(base + P.stem_w_off, 64, 224, st);       // the stem: 7 filter rows x 8 pixels x 4 channels per output channel
        for (const ConvPlan& c : P.convs) launch_split_weights_x3(base + c.w_off, c.Cout, c.K * c.K * c.Cin, st);
        for (const BlockPlan& bp : P.blocks)
            if (bp.ds >= 0) launch_split_weights_x3(base + bp.cat_w_off, P.convs[bp.c3].Cout, P.convs[bp.c3].Cin + P.convs[bp.ds].Cin, st);
    }
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}

static size_t ws_single(int dtype, int B, int chunk) {
    if (chunk <= 0) chunk = default_chunk(dtype);
    if (chunk > B) chunk = B;
    Arena ar(nullptr);
    return carve(ar, dtype, B, chunk, nullptr) + 256;
}
// Two-stream split (tunable STREAMS2, default on; fp32 too - STREAMS2_F32, 9.84 k -> 10.2 k frames/s): a default-chunk batch of >= STREAMS2_MIN (64) units runs as two
// independent halves, the second on the library's side stream — the fabric-bound phases of one half's kernels meet the
// MFMA-bound phases of the other's (2 x 128 frames: 63.2 k -> 65.8 k frames/s on one box, tools/two_stream_probe.py; four
// quarters are slower; at eval sizes: B = 100 + 7 %, 160 + 13 %, 300 + 12 %, 64 + 0.3 %, tools/split_min_sweep.sh).  Per-frame results do not depend on the batch a frame travels in (tests: chunk schedules, batch
// permutations, B = 256 against B = 8 / 64), so the split is invisible in the scores.  Each half gets its own workspace.
static int split_first_half(int B) { return (B / 2 + 7) / 8 * 8; }
static bool split_wanted(int dtype, int B, int chunk, int tap_stage) {
    // both halves must be non-empty whatever STREAMS2_MIN is tuned to: ceil8(B / 2) reaches B for B <= 8
    return (dtype == IVOSW_BF16 || tune_get("STREAMS2_F32", 1)) && chunk <= 0 && tap_stage == 0 && tune_get("STREAMS2", 1) &&
           B >= std::max(2, tune_get("STREAMS2_MIN", 64)) && split_first_half(B) < B;
}
static size_t ws_split(int dtype, int B) {
    const int B0 = split_first_half(B);
    return align_up(ws_single(dtype, B0, 0), 256) + ws_single(dtype, B - B0, 0);
}

extern "C" size_t ivosw_assess_ws_bytes(int dtype, int B, int H, int W, int chunk) {
    if ((dtype != IVOSW_F32 && dtype != IVOSW_BF16 && dtype != IVOSW_F32X3) || B <= 0 || H <= 0 || W <= 0) return 0;
    const size_t one = ws_single(dtype, B, chunk);
    return split_wanted(dtype, B, chunk, 0) ? std::max(one, ws_split(dtype, B)) : one;
}

extern "C" int ivosw_assess_split(int dtype, int B, int chunk) { return split_wanted(dtype, B, chunk, 0) ? 1 : 0; }

extern "C" const char* ivosw_assess_dominant_kernel(int dtype) {
    return dtype == IVOSW_BF16 ? "conv_igemm*|conv1x1_wide*|conv3x3_patch*|bneck*|res2_stage*|res2_chain_kernel*|gemm_8phase*|stage_first*|stem_pool*" : dtype == IVOSW_F32X3 ? "conv_igemm*|stem_pool_x3*" : "conv_igemm*";   // the tower's contraction kernels (one family)
}

// vt != NULL: the units are those of a video table (front.h) and fs / tp / sm / H / W are not looked at
// ids != NULL (with vt): the B rows of the pass are the entries of a unit list, row i = unit ids[i]; chunks and stream halves cut the LIST
static int assess_forward_impl(const void* packed, int dtype, const FrameSrc& fs, const float* tp, const SampleMap& sm, int B, int H, int W,
                               float* scores, void* ws, size_t ws_bytes, int chunk, int tap_stage, void* tap_out,
                               ivosw_stream_t stream, const VideoTable* vt = nullptr, const int32_t* ids = nullptr, float* features = nullptr);

extern "C" int ivosw_assess_forward(const void* packed, int dtype, const float* tf, const float* tp, int B, int H, int W,
                                    float* scores, void* ws, size_t ws_bytes, int chunk, int tap_stage, void* tap_out,
                                    ivosw_stream_t stream) {
    return assess_forward_impl(packed, dtype, FrameSrc{tf, 0}, tp, SampleMap{B, (long)H * W, 0}, B, H, W, scores, ws, ws_bytes, chunk, tap_stage,
                               tap_out, stream);
}

static int assess_forward_objects_impl(const void* packed, int dtype, const FrameSrc& fs, int n_frames, const float* masks,
                                       long mask_stride_frame, long mask_stride_obj, int n_obj, int H, int W, float* scores, void* ws,
                                       size_t ws_bytes, int chunk, ivosw_stream_t stream) {
    IVOSW_REQUIRE(n_frames > 0 && n_obj > 0, "n_frames and n_obj must be positive");
    IVOSW_REQUIRE((long)n_frames * n_obj < (1L << 30), "too many (frame, object) units for one call");
    IVOSW_REQUIRE(mask_stride_frame >= (long)H * W || n_frames == 1, "mask planes of consecutive frames overlap");
    IVOSW_REQUIRE(mask_stride_obj >= 0 && mask_stride_frame >= 0, "negative mask stride");
    return assess_forward_impl(packed, dtype, fs, masks, SampleMap{n_frames, mask_stride_frame, mask_stride_obj}, n_frames * n_obj, H,
                               W, scores, ws, ws_bytes, chunk, 0, nullptr, stream);
}

extern "C" int ivosw_assess_forward_objects(const void* packed, int dtype, const float* tf, int n_frames, const float* masks,
                                            long mask_stride_frame, long mask_stride_obj, int n_obj, int H, int W, float* scores,
                                            void* ws, size_t ws_bytes, int chunk, ivosw_stream_t stream) {
    return assess_forward_objects_impl(packed, dtype, FrameSrc{tf, 0}, n_frames, masks, mask_stride_frame, mask_stride_obj, n_obj, H, W,
                                       scores, ws, ws_bytes, chunk, stream);
}

// the same two entries on RGBX8 frames (ivosw_frames_pack_u8): only the sampler's colour source differs
extern "C" int ivosw_assess_forward_u8(const void* packed, int dtype, const uint8_t* rgbx, const float* tp, int B, int H, int W,
                                       float* scores, void* ws, size_t ws_bytes, int chunk, int tap_stage, void* tap_out,
                                       ivosw_stream_t stream) {
    return assess_forward_impl(packed, dtype, FrameSrc{rgbx, 1}, tp, SampleMap{B, (long)H * W, 0}, B, H, W, scores, ws, ws_bytes, chunk,
                               tap_stage, tap_out, stream);
}

extern "C" int ivosw_assess_forward_objects_u8(const void* packed, int dtype, const uint8_t* rgbx, int n_frames, const float* masks,
                                               long mask_stride_frame, long mask_stride_obj, int n_obj, int H, int W, float* scores,
                                               void* ws, size_t ws_bytes, int chunk, ivosw_stream_t stream) {
    return assess_forward_objects_impl(packed, dtype, FrameSrc{rgbx, 1}, n_frames, masks, mask_stride_frame, mask_stride_obj, n_obj, H, W,
                                       scores, ws, ws_bytes, chunk, stream);
}

// The same pass with the pooled features handed out (include/ivosw.h): any B and chunk, the two-stream split included - the pooling head
// of every chunk group writes its rows at features + first unit * 2048, nothing is copied.
extern "C" int ivosw_assess_forward_features(const void* packed, int dtype, const float* tf, const float* tp, int B, int H, int W,
                                             float* scores, float* features, void* ws, size_t ws_bytes, int chunk, ivosw_stream_t stream) {
    IVOSW_REQUIRE(features, "null pointer (features)");
    return assess_forward_impl(packed, dtype, FrameSrc{tf, 0}, tp, SampleMap{B, (long)H * W, 0}, B, H, W, scores, ws, ws_bytes, chunk, 0,
                               nullptr, stream, nullptr, nullptr, features);
}

extern "C" int ivosw_assess_forward_features_u8(const void* packed, int dtype, const uint8_t* rgbx, const float* tp, int B, int H, int W,
                                                float* scores, float* features, void* ws, size_t ws_bytes, int chunk,
                                                ivosw_stream_t stream) {
    IVOSW_REQUIRE(features, "null pointer (features)");
    return assess_forward_impl(packed, dtype, FrameSrc{rgbx, 1}, tp, SampleMap{B, (long)H * W, 0}, B, H, W, scores, ws, ws_bytes, chunk, 0,
                               nullptr, stream, nullptr, nullptr, features);
}

// Several videos in one pass (include/ivosw.h): the table is validated and built on the host, then the chunk loop, the two-stream split
// and the workspace are those of the single-video entries with B = the table's units - a chunk or a stream half may begin and end inside
// a video and span several, the front-end launches find each unit's video themselves.  (H = W = 2 below only keeps the workspace query of
// the "workspace too small" message answerable; nothing else reads them.)
extern "C" int ivosw_assess_forward_videos(const void* packed, int dtype, const ivosw_video_t* videos, int n_videos, float* scores, void* ws,
                                           size_t ws_bytes, int chunk, int tap_stage, void* tap_out, ivosw_stream_t stream) {
    VideoTable vt;
    if (const int rc = video_table_build(videos, n_videos, __func__, &vt)) return rc;
    return assess_forward_impl(packed, dtype, FrameSrc{nullptr, 0}, nullptr, SampleMap{1, 0, 0}, vt.units, 2, 2, scores, ws, ws_bytes, chunk,
                               tap_stage, tap_out, stream, &vt);
}

// ... with label-map masks (include/ivosw.h: ivosw_labels_t): the table carries each label video's map, the front-end launches pick their
// Lab instantiations, and everything behind the ROI tile is the pass above.
extern "C" int ivosw_assess_forward_videos_lab(const void* packed, int dtype, const ivosw_video_t* videos, const ivosw_labels_t* labels,
                                               int n_videos, float* scores, void* ws, size_t ws_bytes, int chunk, int tap_stage, void* tap_out,
                                               ivosw_stream_t stream) {
    VideoTable vt;
    if (const int rc = video_table_build(videos, n_videos, __func__, &vt, labels)) return rc;
    return assess_forward_impl(packed, dtype, FrameSrc{nullptr, 0}, nullptr, SampleMap{1, 0, 0}, vt.units, 2, 2, scores, ws, ws_bytes, chunk,
                               tap_stage, tap_out, stream, &vt);
}

// The same pass over a unit LIST (include/ivosw.h): row i of the pass is unit unit_ids[i] of the table, so B = n_ids and the chunk loop,
// the two-stream split and the workspace are those of a pass of n_ids units.  The tower writes its scores into a compact [n_ids] buffer
// at the head of the workspace; one scatter launch behind the join stores them at scores[unit_ids[i]] and touches nothing else.
static size_t units_head_bytes(int n_ids) { return align_up((size_t)n_ids * sizeof(float), 256); }

extern "C" size_t ivosw_assess_units_ws_bytes(int dtype, int n_ids, int chunk) {
    if (n_ids <= 0) return 0;
    const size_t body = ivosw_assess_ws_bytes(dtype, n_ids, 2, 2, chunk);
    return body ? units_head_bytes(n_ids) + body : 0;
}

static int assess_forward_units_impl(const char* who, const void* packed, int dtype, const ivosw_video_t* videos, const ivosw_labels_t* labels,
                                     int n_videos, const int32_t* unit_ids, int n_ids, float* scores, void* ws, size_t ws_bytes, int chunk,
                                     ivosw_stream_t stream);

extern "C" int ivosw_assess_forward_units(const void* packed, int dtype, const ivosw_video_t* videos, int n_videos, const int32_t* unit_ids,
                                          int n_ids, float* scores, void* ws, size_t ws_bytes, int chunk, ivosw_stream_t stream) {
    return assess_forward_units_impl(__func__, packed, dtype, videos, nullptr, n_videos, unit_ids, n_ids, scores, ws, ws_bytes, chunk, stream);
}

extern "C" int ivosw_assess_forward_units_lab(const void* packed, int dtype, const ivosw_video_t* videos, const ivosw_labels_t* labels,
                                              int n_videos, const int32_t* unit_ids, int n_ids, float* scores, void* ws, size_t ws_bytes,
                                              int chunk, ivosw_stream_t stream) {
    return assess_forward_units_impl(__func__, packed, dtype, videos, labels, n_videos, unit_ids, n_ids, scores, ws, ws_bytes, chunk, stream);
}

static int assess_forward_units_impl(const char* who, const void* packed, int dtype, const ivosw_video_t* videos, const ivosw_labels_t* labels,
                                     int n_videos, const int32_t* unit_ids, int n_ids, float* scores, void* ws, size_t ws_bytes, int chunk,
                                     ivosw_stream_t stream) {
    VideoTable vt;
    if (const int rc = video_table_build(videos, n_videos, who, &vt, labels)) return rc;
    IVOSW_REQUIRE(n_ids >= 0, "n_ids is negative");
    IVOSW_REQUIRE(n_ids <= vt.units, "n_ids is above the table's units");
    IVOSW_REQUIRE(n_ids == 0 || unit_ids, "null pointer (unit_ids)");
    IVOSW_REQUIRE(dtype == IVOSW_F32 || dtype == IVOSW_BF16 || dtype == IVOSW_F32X3, "dtype must be IVOSW_F32, IVOSW_BF16 or IVOSW_F32X3");
    if (n_ids == 0) return IVOSW_OK;
    IVOSW_REQUIRE(packed && scores && ws, "null pointer");
    IVOSW_ON_DEVICE_OF(scores);
    const size_t head = units_head_bytes(n_ids);
    if (ws_bytes < head) {
        set_error("ivosw_assess_forward_units: workspace %zu < %zu", ws_bytes, ivosw_assess_units_ws_bytes(dtype, n_ids, chunk));
        return IVOSW_ERR_WS;
    }
    float* compact = static_cast<float*>(ws);
    if (const int rc = assess_forward_impl(packed, dtype, FrameSrc{nullptr, 0}, nullptr, SampleMap{1, 0, 0}, n_ids, 2, 2, compact,
                                           static_cast<char*>(ws) + head, ws_bytes - head, chunk, 0, nullptr, stream, &vt, unit_ids))
        return rc;
    launch_scatter_units(compact, unit_ids, n_ids, vt.units, scores, as_stream(stream));
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}

// units [u0, u0 + B) of the batch on stream st with their own workspace; `slot` = which of the (up to two) concurrent profiler spans
// script != NULL: nothing is enqueued, the tower launches the range would make are appended as text (ivosw_assess_describe)
static void assess_forward_range(const void* packed, int dtype, const FrameSrc& fs, const float* tp, const SampleMap& sm, int u0, int B,
                                 int H, int W, float* scores, void* ws, int chunk, int tap_stage, void* tap_out, int slot, hipStream_t st,
                                 const VideoTable* vt, const int32_t* ids, std::string* script = nullptr, float* features = nullptr);

// One helper stream + two events per device for the two-stream split (created on first use, all-or-nothing; the call holds
// the device's mutex while it enqueues so two host threads cannot interleave their fork / join pairs).
namespace {
struct Side2 {
    std::mutex mu;
    hipStream_t stream = nullptr;
    hipEvent_t ev[2] = {};
    bool tried = false;
};
Side2* side2_for_current_device() {
    static Side2 sides[64];
    static std::mutex init_mu;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    Side2& s = sides[dev];
    std::lock_guard<std::mutex> lk(init_mu);
    if (!s.tried) {
        s.tried = true;
        bool ok = hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking) == hipSuccess;
        int made = 0;
        for (; ok && made < 2; ++made) ok = hipEventCreateWithFlags(&s.ev[made], hipEventDisableTiming) == hipSuccess;
        if (!ok) {
            for (int i = 0; i < made; ++i) if (s.ev[i]) (void)hipEventDestroy(s.ev[i]);
            if (s.stream) (void)hipStreamDestroy(s.stream);
            s.stream = nullptr;
            (void)hipGetLastError();
        }
    }
    return s.stream ? &s : nullptr;
}
}  // namespace

static int assess_forward_impl(const void* packed, int dtype, const FrameSrc& fs, const float* tp, const SampleMap& sm, int B, int H, int W,
                               float* scores, void* ws, size_t ws_bytes, int chunk, int tap_stage, void* tap_out,
                               ivosw_stream_t stream, const VideoTable* vt, const int32_t* ids, float* features) {
    IVOSW_REQUIRE(packed && (vt || (fs.p && tp)) && scores && ws, "null pointer");
    IVOSW_REQUIRE(vt || !fs.u8 || (reinterpret_cast<uintptr_t>(fs.p) & 3) == 0, "rgbx must be 4-byte aligned");
    IVOSW_ON_DEVICE_OF(scores);
    IVOSW_REQUIRE(dtype == IVOSW_F32 || dtype == IVOSW_BF16 || dtype == IVOSW_F32X3, "dtype must be IVOSW_F32, IVOSW_BF16 or IVOSW_F32X3");
    IVOSW_REQUIRE(vt || (B > 0 && H > 1 && W > 1), "B must be positive and H, W > 1");      // (a table's videos were checked when it was built)
    IVOSW_REQUIRE(vt || (long)H * W <= INT_MAX, "frame too large (H * W <= INT_MAX)");
    IVOSW_REQUIRE(tap_stage >= 0 && tap_stage <= 8, "tap_stage out of range");
    IVOSW_REQUIRE(tap_stage == 0 || tap_out, "tap_out is null");
    {
        const int packed_for = pack_dtype_lookup(packed, as_stream(stream));
        IVOSW_REQUIRE(packed_for < 0 || packed_for == dtype, "the arena was packed for another dtype (ivosw_assess_pack's dtype must be the forward call's)");
    }
    const bool want_split = split_wanted(dtype, B, chunk, tap_stage);
    if (chunk <= 0) chunk = default_chunk(dtype);
    if (chunk > B) chunk = B;
    IVOSW_REQUIRE(tap_stage == 0 || B <= chunk, "taps need B <= chunk");
    if (ws_bytes < ws_single(dtype, B, chunk)) {
        set_error("ivosw_assess_forward: workspace %zu < %zu", ws_bytes, ivosw_assess_ws_bytes(dtype, B, H, W, chunk));  // B = units
        return IVOSW_ERR_WS;
    }
    hipStream_t st = as_stream(stream);
    Side2* sd = (want_split && ws_bytes >= ws_split(dtype, B)) ? side2_for_current_device() : nullptr;
    if (sd) {
        std::lock_guard<std::mutex> lk(sd->mu);
        const int B0 = split_first_half(B), B1 = B - B0;
        char* ws1 = static_cast<char*>(ws) + align_up(ws_single(dtype, B0, 0), 256);
        bool ok = hipEventRecord(sd->ev[0], st) == hipSuccess && hipStreamWaitEvent(sd->stream, sd->ev[0], 0) == hipSuccess;
        if (ok) {
            span_group_begin();
            assess_forward_range(packed, dtype, fs, tp, sm, 0, B0, H, W, scores, ws, std::min(default_chunk(dtype), B0), 0, nullptr, 0, st, vt, ids, nullptr, features);
            assess_forward_range(packed, dtype, fs, tp, sm, B0, B1, H, W, scores + B0, ws1, std::min(default_chunk(dtype), B1), 0, nullptr, 1, sd->stream, vt, ids, nullptr,
                                 features ? features + (size_t)B0 * 2048 : nullptr);
            span_group_end();
            ok = hipEventRecord(sd->ev[1], sd->stream) == hipSuccess && hipStreamWaitEvent(st, sd->ev[1], 0) == hipSuccess;
            if (!ok) {
                (void)hipGetLastError();
                set_error("ivosw_assess_forward: the join of the two streams failed");
                return IVOSW_ERR_LAUNCH;
            }
            IVOSW_CHECK_LAUNCH();
            return IVOSW_OK;
        }
        (void)hipGetLastError();        // the fork failed before anything was enqueued on the side stream: run on one stream
    }
    assess_forward_range(packed, dtype, fs, tp, sm, 0, B, H, W, scores, ws, chunk, tap_stage, tap_out, 0, st, vt, ids, nullptr, features);
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}

// ---------------------------------------------------------------- the tower's schedule
// Every switch a range of the tower reads, resolved ONCE from the precision, the range's units, the tap, the plan and the tunables.
// (The predicates of other files - bneck_wide_fusable, conv1x1_wide_ok, ... - read the tunables of their own kernels themselves.)
struct TowerKnobs {
    bool fwd2, ys2, stage2, chain, snake;
    bool fuse, fuse_wide, fuse_ds, first3, inplace4, g8, wide1x1, fuse_stem, fuse_stem_x3, fuse_tail_x3, fuse_tail3_x3, ys2abl;
    int df3, df3_min;
};
static TowerKnobs tower_knobs(int dtype, int B, int tap_stage, const Plan& P) {
    TowerKnobs k{};
    k.fuse = tune_get("FUSE", 1); k.fuse_wide = tune_get("FUSE_WIDE", 1); k.fuse_ds = tune_get("FUSE_DS", 1); k.first3 = tune_get("FIRST3", 1);
    k.inplace4 = tune_get("INPLACE4", 1); k.g8 = tune_get("G8", 0); k.wide1x1 = tune_get("WIDE1X1", 1);
    k.fuse_stem = tune_get("FUSE_STEM", 1); k.fuse_stem_x3 = tune_get("FUSE_STEM_X3", 1);
    k.fuse_tail_x3 = tune_get("FUSE_TAIL_X3", 1); k.fuse_tail3_x3 = tune_get("FUSE_TAIL3_X3", 1);
    k.ys2abl = IVOSW_ABLATION && tune_get("YS2ABL", 0);      // ablation: a stage's last block writes even pixels only
    k.df3 = tune_get("DF3", 2); k.df3_min = tune_get("DF3_MIN", 128);
    // conv1 forwarding through res2 (tunable FWD2): block b of res2 also applies block b+1's first 1x1 to its output tile while
    // it is on chip; the last block applies res3's first 1x1, so that layer (a 0.8 GB pass over HBM) is never launched
    k.fwd2 = dtype == IVOSW_BF16 && tune_get("FWD2", 1) && k.fuse_wide && tune_get("FUSE_WIDE2", 1) && tune_get("HALO64S", 1) &&
             tune_get("HALO64S_DS", 1) && P.blocks[3].fwd1_off;
    // ... and res2's last block then writes its output at the even pixels only (compact [nb,32,32,256]): with conv1 forwarded, the
    // only reader left is res3's stride-2 downsample.  Off when an intermediate is tapped (the res2 tap wants the whole tensor).
    k.ys2 = k.fwd2 && tap_stage == 0 && k.fuse_ds && tune_get("YS2", 1);
    // ... or the whole of res2 in ONE launch (res2_stage.hip, tunable RES2_STAGE, default on): a workgroup carries its 8 x 16 tile
    // through the three blocks, y0 / y1 never reach HBM.  Same summation orders as the per-block kernels: bit-identical stage output, so
    // the choice moves no score.  In time the two are level (frames/s at B = 32 / 64 / 100 / 160 / 256: +0.8 / -1.2 / +1.9 / -0.6 /
    // -0.8 %, alternating runs on one box; 946 against 983 us on one stream); the stage kernel moves 2.55 GB less HBM traffic per
    // 256-frame pass (9.23 against 11.77 GB) in four launches fewer, which is why it is the default.
    k.stage2 = k.fwd2 && tune_get("RES2_STAGE", 1);
    // round 6: the register-chained form of the stage kernel (res2_chain.hip); RES2_CHAIN=0 is the round-3 stage kernel
    k.chain = k.stage2 && P.chain_off && tune_get("RES2_CHAIN", 1);
    // Snake order (tunable SNAKE, default on): consecutive launches of the tower walk their pixel tiles in OPPOSITE directions, so a
    // launch starts with the tiles its producer wrote last - still in the memory-side cache (256 MB for ~128 MB tensors per stream) -
    // instead of the ones written first and long evicted.  Tiles are independent: the order cannot change a result.
    // From SNAKE_MIN (96) frames per stream: below that the tensors fit the cache either way (B = 32 / 100 / 160: +-0 / -0.6 / +0.4 %).
    k.snake = dtype == IVOSW_BF16 && tune_get("SNAKE", 1) != 0 && B >= tune_get("SNAKE_MIN", 96);
    return k;
}

// What the launches of one range share.  With `script` set (ivosw_assess_describe) the walk is the same and every launch becomes a
// line "slot kernel frames direction" instead: packed and ws are then never-read stand-ins and no HIP call is made.
struct Tower {
    const Plan& P; TowerKnobs k; int dtype; size_t es; const char* base; Bufs bf; hipStream_t st; int slot; std::string* script;
    int dir = 1;                 // the stem walks backward (its producer, the ROI crop, walks forward), the launch behind it forward ...
    int next_dir() { const int d = k.snake ? dir : 0; dir ^= 1; return d; }
    const float* f32(size_t off) const { return reinterpret_cast<const float*>(base + off); }
    const float* bias(const ConvPlan& c) const { return f32(c.b_off); }
    char* other(const char* x) const { return x == bf.pa ? bf.pb : bf.pa; }     // the ping-pong buffer x is not in
    template <class F> void run(const char* kernel, int frames, int rev, F&& launch) {
        if (!script) return launch();
        char line[96];
        snprintf(line, sizeof(line), "%d %s %d %d\n", slot, kernel, frames, rev);
        *script += line;
    }
};
constexpr int NBLK[4] = {3, 4, 6, 3}, FIRST_BLK[4] = {0, 3, 7, 13}, HW_IN[4] = {64, 64, 32, 16};
static int block_hw(int s, int b) { return (s > 0 && b > 0) ? HW_IN[s] / 2 : HW_IN[s]; }      // res3..res5 halve H and W in their first block

// a generic layer: the 8-phase / wide 1x1 kernels where they apply, else conv.hip's selector
static void launch_layer(Tower& T, const ConvArgs& q, size_t fw_off) {
    if (T.dtype == IVOSW_BF16 && T.k.g8 && T.k.wide1x1 && conv1x1_g8_ok(q)) T.run("gemm_8phase_kernel", q.B, q.rev, [&] { launch_conv1x1_g8(q, T.st); });
    else if (T.dtype == IVOSW_BF16 && fw_off && conv1x1_wide_ok(q) && T.k.wide1x1) T.run("conv1x1_wide_kernel", q.B, q.rev, [&] { launch_conv1x1_wide(q, T.base + fw_off, T.st); });
    else T.run(conv_kernel_name(conv_select(q, T.dtype, false)), q.B, q.rev, [&] { launch_conv(q, T.dtype, false, T.st); });
}
static ConvArgs conv_args(Tower& T, const ConvPlan& c, const void* in, int hin, int hout, const void* res, void* o, int relu, int nb) {
    ConvArgs q{};
    q.zeros = T.base + T.P.zero_off; q.x = in; q.w = T.base + c.w_off; q.bias = T.bias(c); q.res = res; q.y = o;
    q.B = nb; q.H = hin; q.W = hin; q.Cin = c.Cin; q.Ho = hout; q.Wo = hout; q.Cout = c.Cout;
    q.KH = c.K; q.KW = c.K; q.stride = c.stride; q.pad = c.pad; q.relu = relu;
    q.rev = T.next_dir();
    return q;
}

// the fragment / bias pointers of a wide block's three convs
static void wide_weights(const Tower& T, const BlockPlan& bp, BneckWideArgs& q) {
    q.fa = T.base + bp.f1_off; q.ba = T.bias(T.P.convs[bp.c1]);
    q.fb = T.base + bp.f2_off; q.bb = T.bias(T.P.convs[bp.c2]);
    q.fc = T.base + bp.f3_off; q.bc = T.bias(T.P.convs[bp.c3]);
}
static bool wide_offered(const Tower& T, const BlockPlan& bp) { return T.dtype == IVOSW_BF16 && bp.f1_off && T.k.fuse_wide; }
// block b of stage s as a wide block: everything but x, y and the direction
static BneckWideArgs wide_args(const Tower& T, int s, int b, int nb, int foff) {
    const Plan& P = T.P;
    const BlockPlan& bp = P.blocks[FIRST_BLK[s] + b];
    BneckWideArgs q{};
    q.zeros = T.base + P.zero_off;
    wide_weights(T, bp, q);
    if (bp.ds >= 0) { q.ds = 1; q.fc = T.base + bp.cat_fw_off; q.bc = T.f32(bp.cat_b_off); }
    q.B = nb; q.H = q.W = block_hw(s, b); q.Cin = P.convs[bp.c1].Cin; q.Cmid = P.convs[bp.c1].Cout;
    if (s == 0 && T.k.fwd2) {
        // t1 ping-pong: b0 -> m2 -> b1 -> ds -> b2 -> m1 (res3's t1 for the frames of the enclosing res3 chunk)
        const BlockPlan& nx = P.blocks[b + 1];           // the next block (res3's first after b == 2)
        q.t1in = b == 0 ? nullptr : (b == 1 ? T.bf.m2 : T.bf.ds);
        q.t1out = b == 0 ? T.bf.m2 : (b == 1 ? T.bf.ds : T.bf.m1 + (size_t)foff * 64 * 64 * 128 * T.es);
        q.fd = T.base + (b == 2 ? nx.fwd1_off : nx.f1_off); q.bd = T.bias(P.convs[nx.c1]);
        q.nd = P.convs[nx.c1].Cout;
        q.y_s2 = (b == 2 && T.k.ys2) ? 1 : 0;
    }
    return q;
}
static BneckArgs bneck_args(const Tower& T, const BlockPlan& bp, int hw, int nb, const void* x, void* y) {
    const Plan& P = T.P;
    const ConvPlan &c1 = P.convs[bp.c1], &c2 = P.convs[bp.c2], &c3 = P.convs[bp.c3];
    BneckArgs q{};
    q.x = x; q.y = y; q.zeros = T.base + P.zero_off;
    q.wa = T.base + c1.w_off; q.ba = T.bias(c1); q.wb = T.base + c2.w_off; q.bb = T.bias(c2); q.wc = T.base + c3.w_off; q.bc = T.bias(c3);
    if (bp.ds >= 0) { q.wd = T.base + P.convs[bp.ds].w_off; q.bd = T.bias(P.convs[bp.ds]); }
    q.B = nb; q.H = hw; q.W = hw; q.Cin = c1.Cin; q.Cmid = c1.Cout;
    return q;
}
// res3's first block (input x at hw = 64, or 32 where res2 stored even pixels only) behind its forwarded conv1 in m1
static StageFirstArgs stage_first_args(const Tower& T, const BlockPlan& bp, int nb, const void* x, void* y) {
    const ConvPlan& c2 = T.P.convs[bp.c2];
    StageFirstArgs q{};
    q.t1 = T.bf.m1; q.x2 = x; q.y = y; q.zeros = T.base + T.P.zero_off;
    q.fw2 = T.base + bp.f2_off; q.b2 = T.bias(c2);
    q.fwc = T.base + bp.cat_fw_off; q.bc = T.f32(bp.cat_b_off);
    q.B = nb; q.Ho = q.Wo = HW_IN[1] / c2.stride; q.Cm = c2.Cout; q.C2 = T.P.convs[bp.ds].Cin;
    q.H2 = q.W2 = T.k.ys2 ? HW_IN[1] / 2 : HW_IN[1]; q.stride2 = T.k.ys2 ? 1 : 2;
    return q;
}

// The form that runs block b of stage s in a launch of nb frames, and how many blocks it consumes (1, or the rest of the stage - for
// b == 0 the whole of it).  The order of the tests is the priority.  A predicate that is asked on an argument struct gets the struct
// the launch gets, weights included (an offset the plan does not hold turns the form down); only the activations, which no
// predicate distinguishes beyond non-null, are workspace stand-ins.
enum Form { F_RES2_CHAIN, F_RES2_STAGE, F_WIDE_DF3, F_WIDE_CHAIN, F_WIDE, F_BNECK64, F_STAGE_FIRST, F_TAIL2_X3, F_TAIL3_X3, F_TAIL2_X3_DS, F_LAYERS_CAT, F_LAYERS };
struct Choice { Form form; int blocks; };
static Choice choose_form(const Tower& T, int s, int b, int nb) {
    const Plan& P = T.P;
    const TowerKnobs& k = T.k;
    const BlockPlan& bp = P.blocks[FIRST_BLK[s] + b];
    const ConvPlan &c2 = P.convs[bp.c2], &c3 = P.convs[bp.c3];
    const int hw = block_hw(s, b), rest = NBLK[s] - b;
    const bool bf16 = T.dtype == IVOSW_BF16, x3 = T.dtype == IVOSW_F32X3;
    if (s == 0 && b == 0 && k.chain) return {F_RES2_CHAIN, rest};
    if (s == 0 && b == 0 && k.stage2) {
        Res2StageArgs q = res2_stage_args(P, T.base);
        q.x = T.bf.pa; q.y = q.t1out = T.bf.m1; q.B = nb;
        if (res2_stage_ok(q)) return {F_RES2_STAGE, rest};
    }
    if (wide_offered(T, bp)) {
        const BneckWideArgs q = wide_args(T, s, b, nb, 0);
        // res3's three identity blocks depth first (run_wide_df3): only under the snake order, from DF3_MIN frames per launch
        if (s == 1 && b == 1 && bp.ds < 0 && k.snake && bneck_wide_fusable(q) && k.df3 > 1 && nb >= k.df3_min) return {F_WIDE_DF3, rest};
        // the rest of the stage is identity blocks of this shape: chain them inside one launch
        if (bp.ds < 0 && bneck_wide_fusable(q) && bneck_stage_fusable(q) && rest > 1) return {F_WIDE_CHAIN, rest};
        if (bneck_wide_fusable(q)) return {F_WIDE, 1};
    }
    if (bf16 && (bp.ds < 0 || c2.stride == 1) && k.fuse && bneck_fusable(bneck_args(T, bp, hw, nb, T.bf.pa, T.bf.pb))) return {F_BNECK64, 1};
    // res3's first block behind its forwarded conv1 as ONE launch: t2 never leaves LDS (stage_first.hip; bit-identical to the two
    // layer launches it replaces)
    if (bf16 && s == 1 && b == 0 && k.fwd2 && bp.ds >= 0 && bp.f2_off && bp.cat_fw_off && k.first3 &&
        stage_first_ok(stage_first_args(T, bp, nb, T.bf.in[0], T.bf.pa)))
        return {F_STAGE_FIRST, 1};
    // the three-pass mode behind a block's conv1: 3x3 -> conv3 + residual as one launch (conv.hip: t2 stays on the CU), for the
    // identity blocks of res2 (64 channels at 64 x 64) and res3 (128 at 32 x 32) ...
    auto tail = [&](int h, int c) { return x3 && hw == h && c2.K == 3 && c2.stride == 1 && c2.Cin == c && c2.Cout == c && c3.Cin == c && c3.Cout == 4 * c; };
    if (s == 0 && bp.ds < 0 && tail(64, 64) && k.fuse_tail_x3) return {F_TAIL2_X3, 1};
    if (s == 1 && bp.ds < 0 && tail(32, 128) && k.fuse_tail3_x3) return {F_TAIL3_X3, 1};
    // ... and res2's first block: 3x3 -> [conv3 | downsample] (K = 64 + 64, the block input as the second half)
    if (s == 0 && bp.ds >= 0 && tail(64, 64) && P.convs[bp.ds].Cin == 64 && P.convs[bp.ds].stride == 1 && k.fuse_ds && k.fuse_tail_x3) return {F_TAIL2_X3_DS, 1};
    // first block of a stage, layer by layer: relu(conv3(t2) + downsample(x)) as ONE GEMM over K = C + Cin (the block input, sampled at
    // the downsample stride, is the second A source): the 4C-channel downsample output never goes to HBM and back
    if (bp.ds >= 0 && k.fuse_ds) return {F_LAYERS_CAT, 1};
    return {F_LAYERS, 1};
}

// res3's three identity blocks DEPTH FIRST over DF3 (2) groups of the launch's frames: b1 b2 b3 for the first half, then for the
// second.  Every block's input was written by the launch right before it and its x + y (64 + 64 MB per stream instead of 128 + 128)
// fit the memory-side cache together with the other stream's.  Costs the tail balancing of a 512-workgroup launch (256 workgroups are
// a single round): + 0.8 % frames/s on average over five boxes at 128 frames per stream (- 0.2 .. + 2.5 %), - 0.5 % with four groups;
// a frame's result does not depend on the launch it travels in.
static void run_wide_df3(Tower& T, int nb, const char* x, char* out) {
    const BneckWideArgs q = wide_args(T, 1, 1, nb, 0);
    const size_t fe = (size_t)q.H * q.W * q.Cin * T.es;
    char* const y1 = T.other(x);
    char* const bufs[4] = {const_cast<char*>(x), y1, T.other(y1), out};
    for (int g = 0; g < T.k.df3; ++g) {
        const int lo = (int)((long)nb * g / T.k.df3), hi = (int)((long)nb * (g + 1) / T.k.df3);
        for (int bb = 1; bb <= 3; ++bb) {
            BneckWideArgs r = q;
            wide_weights(T, T.P.blocks[FIRST_BLK[1] + bb], r);
            r.x = bufs[bb - 1] + (size_t)lo * fe; r.y = bufs[bb] + (size_t)lo * fe;
            r.B = hi - lo;
            r.rev = T.next_dir();
            if (bb == 3 && T.k.ys2abl) r.debug |= 16;
            T.run("bneck_wide", r.B, r.rev, [&] { launch_bneck_wide(r, T.st); });
        }
    }
}
// blocks b .. of a stage (res4's identity blocks) chained inside one launch
static void run_wide_chain(Tower& T, int s, int b, int nb, const char* x, char* out) {
    BneckWideArgs q = wide_args(T, s, b, nb, 0);
    q.rev = T.next_dir();
    BneckStageArgs sa{};
    for (int bb = b; bb < NBLK[s]; ++bb) {
        // in place (tunable INPLACE4): a frame belongs to ONE workgroup, phase A has consumed x before phase C writes, and an
        // element of y goes where the residual it was formed from came from - half the footprint of the chain in the caches
        char* y = (bb == NBLK[s] - 1) ? out : ((T.k.inplace4 && bb > b) ? const_cast<char*>(x) : T.other(x));
        BneckWideArgs& r = sa.blk[sa.n++];
        r = q;
        r.x = x; r.y = y;
        wide_weights(T, T.P.blocks[FIRST_BLK[s] + bb], r);
        if (s == 2 && bb == NBLK[s] - 1 && T.k.ys2abl) r.debug |= 16;
        x = y;
    }
    T.run("bneck_wide_stage_kernel", nb, q.rev, [&] { launch_bneck_wide_stage(sa, T.st); });
}

// one bottleneck stage (K5) on nb frames: x -> out (the stage's last block writes straight into `out`); foff: the launch's first
// frame inside the enclosing res3 chunk (where res2 leaves res3's forwarded conv1)
static void run_stage(Tower& T, int s, const char* x, int nb, char* out, int foff) {
    const Plan& P = T.P;
    const char* base = T.base;
    hipStream_t st = T.st;
    for (int b = 0; b < NBLK[s];) {
        const Choice ch = choose_form(T, s, b, nb);
        const BlockPlan& bp = P.blocks[FIRST_BLK[s] + b];
        const ConvPlan &c1 = P.convs[bp.c1], &c2 = P.convs[bp.c2], &c3 = P.convs[bp.c3];
        const int hw = block_hw(s, b), ho = hw / c2.stride;
        char* y = (b + ch.blocks == NBLK[s]) ? out : T.other(x);
        char* t1f = T.bf.m1 + (size_t)foff * 64 * 64 * 128 * T.es;
        // a block that was offered to the wide kernels and turned down (res5's identity blocks, by default) has taken a direction
        // all the same, ever since the snake order exists: the launches behind it keep the directions they were measured with
        if (ch.form > F_WIDE && wide_offered(T, bp)) T.next_dir();
        auto conv1 = [&] { if (!(s == 1 && b == 0 && T.k.fwd2)) launch_layer(T, conv_args(T, c1, x, hw, hw, nullptr, T.bf.m1, 1, nb), c1.fw_off); };  // forwarded: res2's last block wrote it
        switch (ch.form) {
        case F_RES2_CHAIN: {
            Res2ChainArgs q{};
            q.x = x; q.y = out; q.t1out = t1f; q.wstream = base + P.chain_off; q.zeros = base + P.zero_off;
            q.B = nb; q.y_s2 = T.k.ys2 ? 1 : 0; q.rev = T.next_dir();
            T.run("res2_chain_kernel", nb, q.rev, [&] { launch_res2_chain(q, st); });
            break;
        }
        case F_RES2_STAGE: {
            Res2StageArgs q = res2_stage_args(P, base);
            q.x = x; q.y = out; q.t1out = t1f; q.B = nb; q.y_s2 = T.k.ys2 ? 1 : 0; q.rev = T.next_dir();
            T.run("res2_stage_kernel", nb, q.rev, [&] { launch_res2_stage(q, st); });
            break;
        }
        case F_WIDE_DF3: run_wide_df3(T, nb, x, out); break;
        case F_WIDE_CHAIN: run_wide_chain(T, s, b, nb, x, out); break;
        case F_WIDE: {
            BneckWideArgs q = wide_args(T, s, b, nb, foff);
            q.x = x; q.y = y; q.rev = T.next_dir();
            T.run("bneck_wide", nb, q.rev, [&] { launch_bneck_wide(q, st); });
            break;
        }
        case F_BNECK64: T.run("bneck64_kernel", nb, 0, [&] { launch_bneck(bneck_args(T, bp, hw, nb, x, y), st); }); break;
        case F_STAGE_FIRST: {
            StageFirstArgs q = stage_first_args(T, bp, nb, x, y);
            q.rev = T.next_dir();
            T.run("stage_first_kernel", nb, q.rev, [&] { launch_stage_first(q, st); });
            break;
        }
        case F_TAIL2_X3: case F_TAIL3_X3: case F_TAIL2_X3_DS: {
            conv1();
            const bool ds = ch.form == F_TAIL2_X3_DS, r3 = ch.form == F_TAIL3_X3;
            const void *w2 = base + c2.w_off, *w3 = base + (ds ? bp.cat_w_off : c3.w_off), *zeros = base + P.zero_off;
            const float* b3 = ds ? T.f32(bp.cat_b_off) : T.bias(c3);
            const int d = T.next_dir();
            T.run(r3 ? "res3_tail_x3_kernel" : "res2_tail_x3_kernel", nb, d, [&] {
                if (r3) launch_res3_tail_x3(T.bf.m1, x, w2, T.bias(c2), w3, b3, zeros, y, nb, hw, hw, d, st);
                else launch_res2_tail_x3(T.bf.m1, ds ? nullptr : x, w2, T.bias(c2), w3, b3, zeros, y, nb, hw, hw, d, st, ds ? x : nullptr);
            });
            break;
        }
        case F_LAYERS_CAT: case F_LAYERS: {
            conv1();
            launch_layer(T, conv_args(T, c2, T.bf.m1, hw, ho, nullptr, T.bf.m2, 1, nb), c2.fw_off);
            const ConvPlan* cd = bp.ds >= 0 ? &P.convs[bp.ds] : nullptr;
            if (ch.form == F_LAYERS_CAT) {
                ConvArgs q = conv_args(T, c3, T.bf.m2, ho, ho, nullptr, y, 1, nb);
                q.w = base + bp.cat_w_off; q.bias = T.f32(bp.cat_b_off);
                q.x2 = x; q.Cin2 = cd->Cin; q.H2 = hw; q.W2 = hw; q.stride2 = cd->stride;
                if (s == 1 && T.k.ys2) { q.H2 = hw / 2; q.W2 = hw / 2; q.stride2 = 1; }      // res2's output arrives already subsampled
                launch_layer(T, q, bp.cat_fw_off);
                break;
            }
            if (cd) launch_layer(T, conv_args(T, *cd, x, hw, ho, nullptr, T.bf.ds, 0, nb), cd->fw_off);
            launch_layer(T, conv_args(T, c3, T.bf.m2, ho, ho, cd ? T.bf.ds : x, y, 1, nb), c3.fw_off);  // relu(bn3(conv3) + identity)
            break;
        }
        }
        x = y;
        b += ch.blocks;
    }
}

static void assess_forward_range(const void* packed, int dtype, const FrameSrc& fs, const float* tp, const SampleMap& sm, int u0, int B,
                                 int H, int W, float* scores, void* ws, int chunk, int tap_stage, void* tap_out, int slot, hipStream_t st,
                                 const VideoTable* vt, const int32_t* ids, std::string* script, float* features) {
    const Plan& P = plan_for(dtype);
    const size_t es = (dtype == IVOSW_BF16) ? 2 : 4;
    const char* base = static_cast<const char*>(packed);
    Tower T{P, tower_knobs(dtype, B, tap_stage, P), dtype, es, base, Bufs{}, st, slot, script};
    Arena ar(ws);
    carve(ar, dtype, B, chunk, &T.bf);
    const Bufs& bf = T.bf;
    const bool live = !script;               // describing: no front end, no taps, no spans, no head
    auto tap = [&](int stage, const void* src, size_t bytes) {
        if (!live || tap_stage != stage) return;
        (void)hipMemcpyAsync(tap_out, src, bytes, hipMemcpyDeviceToDevice, st);
        // IVOSW_F32X3 keeps its activations (stem output .. res5) in the split hi | lo layout: the tap hands out plain fp32
        if (dtype == IVOSW_F32X3 && stage >= 2 && stage <= 7) launch_unsplit_x3(tap_out, bytes / sizeof(float), st);
    };

    // K1/K2: mask -> (y,x,h,w) for the whole batch, on device
    if (live && vt) launch_mask_bbox_multi(*vt, u0, B, bf.yxhw, bf.box, st, ids);
    else if (live) launch_mask_bbox(tp, u0, B, H, W, sm, bf.yxhw, bf.box, st);
    // Encoder.mean/std come from the checkpoint: the sampler reads them from the packed arena
    RoiNorm nrm{{0.f, 0.f, 0.f}, {1.f, 1.f, 1.f}, reinterpret_cast<const float*>(base + P.norm_off)};
    const int cs[4] = {chunk, chunk * 2, chunk * 4, chunk * 8};
    const float* stem_b = reinterpret_cast<const float*>(base + P.stem_b_off);

    for (int f3 = 0; f3 < B; f3 += cs[3]) {
        const int n3 = std::min(cs[3], B - f3);
        for (int f2 = f3; f2 < f3 + n3; f2 += cs[2]) {
            const int n2 = std::min(cs[2], f3 + n3 - f2);
            for (int f1 = f2; f1 < f2 + n2; f1 += cs[1]) {
                const int n1 = std::min(cs[1], f2 + n2 - f1);
                for (int f0 = f1; f0 < f1 + n1; f0 += cs[0]) {
                    const int nb = std::min(cs[0], f1 + n1 - f0);
                    if (live) {
                        // K3: ROI crop-resize + normalise -> NHWC4
                        span_close(st, slot);
                        if (vt) launch_roi_sample_multi(*vt, bf.yxhw + (size_t)f0 * 4, u0 + f0, nb, dtype, nrm, bf.roi, st, ids);
                        else launch_roi_sample(fs, tp, bf.yxhw + (size_t)f0 * 4, u0 + f0, nb, H, W, dtype, sm, nrm, bf.roi, st);
                        tap(1, bf.roi, nb * E_ROI * es);
                        span_open(st, slot);
                    }
                    // K4: stem 7x7/2 (RGB|P) + BN + ReLU, then 3x3/2 max pool (bf16: one fused kernel unless the stem tap is wanted)
                    if (dtype == IVOSW_BF16 && tap_stage != 2 && T.k.fuse_stem) {
                        T.dir = 1;               // every res2 chunk starts the alternation anew at its stem
                        const int d = T.next_dir();
                        T.run("stem_pool_kernel", nb, d, [&] { launch_stem_pool(bf.roi, base + P.stem_w_off, stem_b, nb, bf.pa, st, d); });
                    } else if (dtype == IVOSW_F32X3 && tap_stage != 2 && T.k.fuse_stem_x3) {
                        // the three-pass mode's stem + pool as one launch (stem.hip): fp32 ROI tile in, split pooled map out
                        T.run("stem_pool_x3_kernel", nb, 0, [&] { launch_stem_pool_x3(bf.roi, base + P.stem_w_off, stem_b, nb, bf.pa, st, 0); });
                    } else {
                        ConvArgs a{};
                        a.zeros = base + P.zero_off; a.x = bf.roi; a.w = base + P.stem_w_off; a.bias = stem_b;
                        a.res = nullptr; a.y = bf.stem; a.B = nb; a.H = 256; a.W = 256; a.Cin = 4; a.Ho = 128; a.Wo = 128;
                        a.Cout = 64; a.KH = 7; a.KW = 7; a.stride = 2; a.pad = 3; a.relu = 1;
                        T.run(conv_kernel_name(conv_select(a, dtype, true)), nb, 0, [&] { launch_conv(a, dtype, true, st); });
                        tap(2, bf.stem, (size_t)nb * 128 * 128 * 64 * es);
                        T.run(dtype == IVOSW_F32X3 ? "maxpool_x3_kernel" : "maxpool_kernel", nb, 0, [&] { launch_maxpool(bf.stem, nb, 128, 128, 64, dtype, bf.pa, st); });
                    }
                    tap(3, bf.pa, (size_t)nb * 64 * 64 * 64 * es);
                    char* o2 = bf.in[0] + (size_t)(f0 - f1) * (T.k.ys2 ? E_OUT[0] / 4 : E_OUT[0]) * es;
                    run_stage(T, 0, bf.pa, nb, o2, f0 - f1);
                    tap(4, o2, nb * E_OUT[0] * es);
                }
                char* o3 = bf.in[1] + (size_t)(f1 - f2) * E_OUT[1] * es;
                run_stage(T, 1, bf.in[0], n1, o3, 0);
                tap(5, o3, n1 * E_OUT[1] * es);
            }
            char* o4 = bf.in[2] + (size_t)(f2 - f3) * E_OUT[2] * es;
            run_stage(T, 2, bf.in[1], n2, o4, 0);
            tap(6, o4, n2 * E_OUT[2] * es);
        }
        run_stage(T, 3, bf.in[2], n3, bf.pa, 0);  // c0*8 frames x 131k elements == c0 * E_BIG: fits a ping-pong buffer
        tap(7, bf.pa, n3 * E_OUT[3] * es);
        if (!live) continue;
        // K6: 8x8 average pool + fc1
        span_close(st, slot);
        launch_pool_fc(bf.pa, n3, dtype, reinterpret_cast<const float*>(base + P.fcw_off),
                       reinterpret_cast<const float*>(base + P.fcb_off), scores + f3,
                       features ? features + (size_t)f3 * 2048 : tap_stage == 8 ? bf.pooled : nullptr, st);      // features: each pool group's rows straight to the caller
        tap(8, bf.pooled, (size_t)n3 * 2048 * sizeof(float));
    }
}

// The launches of ivosw_assess_forward(dtype, B, chunk, tap_stage) behind the ROI sampler and before the pooling head, as text (include/ivosw.h): the
// same split decision and the same walk, asked without a device.  Stand-in arena and workspace addresses: nothing reads through them.
extern "C" int ivosw_assess_describe(int dtype, int B, int chunk, int tap_stage, char* buf, size_t cap) {
    IVOSW_REQUIRE(dtype == IVOSW_F32 || dtype == IVOSW_BF16 || dtype == IVOSW_F32X3, "dtype must be IVOSW_F32, IVOSW_BF16 or IVOSW_F32X3");
    IVOSW_REQUIRE(B > 0 && tap_stage >= 0 && tap_stage <= 8 && buf && cap > 0, "B must be positive, tap_stage in 0 .. 8, buf non-null");
    const bool split = split_wanted(dtype, B, chunk, tap_stage);
    if (chunk <= 0) chunk = default_chunk(dtype);
    if (chunk > B) chunk = B;
    IVOSW_REQUIRE(tap_stage == 0 || B <= chunk, "taps need B <= chunk");
    char* const packed = reinterpret_cast<char*>(uintptr_t(1) << 40);
    char* const ws = reinterpret_cast<char*>(uintptr_t(1) << 41);
    std::string s;
    auto range = [&](int u0, int n, int c, int slot) {
        assess_forward_range(packed, dtype, FrameSrc{nullptr, 0}, nullptr, SampleMap{1, 0, 0}, u0, n, 2, 2, nullptr, ws, c, tap_stage, nullptr, slot, nullptr, nullptr, nullptr, &s);
    };
    if (split) {
        const int B0 = split_first_half(B);
        range(0, B0, std::min(default_chunk(dtype), B0), 0);
        range(B0, B - B0, std::min(default_chunk(dtype), B - B0), 1);
    } else {
        range(0, B, chunk, 0);
    }
    if (s.size() + 1 > cap) {
        set_error("ivosw_assess_describe: buffer %zu < %zu", cap, s.size() + 1);
        return IVOSW_ERR_WS;
    }
    memcpy(buf, s.c_str(), s.size() + 1);
    return IVOSW_OK;
}

#ifdef IVOSW_PROBES
// Tuning probe: one launch of the res2 stage kernel on x [B,64,64,64] bf16 with the weights of a packed bf16 arena; y [B,64,64,256]
// (y_s2: [B,32,32,256]), t1out [B,64,64,128]; ts (may be NULL): [B*32][16] s_memtime stamps at the phase boundaries.
extern "C" int ivosw_res2_stage_probe(const void* packed, const void* x, void* y, void* t1out, int B, int y_s2, unsigned long long* ts,
                                      ivosw_stream_t stream) {
    IVOSW_REQUIRE(packed && x && y && t1out && B > 0, "null pointer");
    IVOSW_ON_DEVICE_OF(y);
    if (tune_get("RES2_CHAIN", 1) && plan_for(IVOSW_BF16).chain_off) {      // ts: [B * 32][8] stamps (res2_chain.hip) instead of [B * 32][16]
        const Plan& P = plan_for(IVOSW_BF16);
        Res2ChainArgs c{};
        c.x = x; c.y = y; c.t1out = t1out; c.wstream = static_cast<const char*>(packed) + P.chain_off; c.zeros = static_cast<const char*>(packed) + P.zero_off;
        c.B = B; c.y_s2 = y_s2; c.ts = ts;
        launch_res2_chain(c, as_stream(stream));
        IVOSW_CHECK_LAUNCH();
        return IVOSW_OK;
    }
    Res2StageArgs q = res2_stage_args(plan_for(IVOSW_BF16), static_cast<const char*>(packed));
    q.x = x; q.y = y; q.t1out = t1out; q.B = B; q.y_s2 = y_s2; q.ts = ts;
    q.debug = tune_get("R2DBG", 0);
    IVOSW_REQUIRE(res2_stage_ok(q), "the packed arena lacks the fragment-ordered res2 weights");
    launch_res2_stage(q, as_stream(stream));
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}

// Test probe: one bf16 layer launch on the caller's tensors through one of the three paths of launch_layer above; *ran = the instantiation.
extern "C" int ivosw_conv_probe(const void* x, const void* w, const float* bias, const void* res, const void* x2, void* y, const void* zeros,
                                void* frag, int B, int H, int W, int Cin, int Cout, int ksize, int stride, int pad, int relu, int rev,
                                int H2, int W2, int Cin2, int stride2, int kernel, int* ran, ivosw_stream_t stream) {
    IVOSW_REQUIRE(x && w && bias && y && zeros, "null pointer");
    IVOSW_REQUIRE(kernel >= 0 && kernel <= 2 && (kernel != 1 || frag), "kernel is 0 (selector), 1 (wide, needs frag) or 2 (8-phase)");
    IVOSW_REQUIRE(B > 0 && H > 0 && W > 0 && (ksize == 1 || ksize == 3) && stride >= 1 && stride <= 2 && pad >= 0 && pad <= ksize / 2 &&
                  Cin > 0 && Cin % 64 == 0 && Cout > 0 && Cout % 64 == 0 && (Cout == 64 || Cout % 128 == 0),
                  "shape is not covered by the bf16 layer kernels (Cin % 64, Cout 64 or % 128, ksize 1 / 3, stride 1 / 2)");
    IVOSW_REQUIRE(!x2 || (ksize == 1 && Cin2 > 0 && Cin2 % 64 == 0 && stride2 >= 1 && H2 > 0 && W2 > 0),
                  "shape is not covered: the K-extension belongs to 1x1 layers, Cin2 % 64 == 0");
    IVOSW_ON_DEVICE_OF(y);
    hipStream_t st = as_stream(stream);
    ConvArgs q{};
    q.x = x; q.w = w; q.bias = bias; q.res = res; q.y = y; q.zeros = zeros;
    q.B = B; q.H = H; q.W = W; q.Cin = Cin; q.Cout = Cout; q.KH = q.KW = ksize; q.stride = stride; q.pad = pad; q.relu = relu; q.rev = rev;
    q.Ho = (H + 2 * pad - ksize) / stride + 1; q.Wo = (W + 2 * pad - ksize) / stride + 1;
    if (x2) { q.x2 = x2; q.Cin2 = Cin2; q.H2 = H2; q.W2 = W2; q.stride2 = stride2; }
    // every kernel samples x2 at (oy * stride2, ox * stride2) without a bounds test: the last sample must lie inside the frame
    IVOSW_REQUIRE(!x2 || ((q.Ho - 1) * stride2 < H2 && (q.Wo - 1) * stride2 < W2), "shape is not covered: x2 is sampled outside its frame");
    const int K = ksize * ksize * Cin + (x2 ? Cin2 : 0);
    const long M = (long)B * q.Ho * q.Wo;
    IVOSW_REQUIRE(M * std::max(Cout, K) < (1L << 31), "too many frames for a probe launch");
    int id = 0;
    if (kernel == 1) {
        IVOSW_REQUIRE(conv1x1_wide_ok(q), "layer is not covered by conv1x1_wide_kernel");
        // launch_conv1x1_wide's own rule (bottleneck_wide.hip): fewer 256-pixel tiles than WIDE_SMALL -> 128-pixel tiles
        id = (int)((M + 255) / 256) * (Cout / 256) < tune_get("WIDE_SMALL", 0) ? 4 : 8;
        launch_fragpack(w, Cout, K, frag, st);
        launch_conv1x1_wide(q, frag, st);
    } else if (kernel == 2) {
        IVOSW_REQUIRE(conv1x1_g8_ok(q), "layer is not covered by the 8-phase contraction");
        id = res ? 1 : 0;
        launch_conv1x1_g8(q, st);
    } else {
        id = (int)conv_select(q, IVOSW_BF16, false);
        launch_conv(q, IVOSW_BF16, false, st);
    }
    if (ran) *ran = id;
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}

// Test probe: one launch of stage_first_kernel on the caller's tensors, the K-major weights reordered into `frag` on the device first.
extern "C" int ivosw_stage_first_probe(const void* t1, const void* x2, const void* w2, const float* b2, const void* wc, const float* bc,
                                       void* frag, const void* zeros, void* y, int B, int Ho, int Wo, int H2, int W2, int stride2, int rev,
                                       ivosw_stream_t stream) {
    IVOSW_REQUIRE(t1 && x2 && w2 && b2 && wc && bc && frag && zeros && y, "null pointer");
    IVOSW_ON_DEVICE_OF(y);
    hipStream_t st = as_stream(stream);
    constexpr int Cm = 128, C2 = 256;
    char* f = static_cast<char*>(frag);
    const size_t n2 = (size_t)Cm * 9 * Cm * 2;
    StageFirstArgs q{};
    q.t1 = t1; q.x2 = x2; q.y = y; q.zeros = zeros; q.fw2 = f; q.b2 = b2; q.fwc = f + n2; q.bc = bc;
    q.B = B; q.Ho = Ho; q.Wo = Wo; q.Cm = Cm; q.C2 = C2; q.H2 = H2; q.W2 = W2; q.stride2 = stride2; q.rev = rev;
    // refuse BEFORE the weight reordering: a refused call launches nothing and leaves `frag` as it was
    IVOSW_REQUIRE(B > 0 && B <= 1024 && stage_first_ok(q), "shape is not covered by stage_first_kernel");
    launch_fragpack(w2, Cm, 9 * Cm, f, st);
    launch_fragpack(wc, 4 * Cm, Cm + C2, f + n2, st);
    launch_stage_first(q, st);
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}

// Test probe: one launch of res2 + res3's forwarded conv1 on the caller's tensors and K-major weights; what the chosen kernel reads is
// made in `frag` on the device first, by the launches ivosw_assess_pack makes it with.  *ran = the instantiation.
extern "C" int ivosw_res2_probe(const void* x, const void* const* w, const float* const* bias, void* frag, const void* zeros, void* y,
                                void* t1out, int B, int y_s2, int rev, int form, int* ran, ivosw_stream_t stream) {
    IVOSW_REQUIRE(x && w && bias && frag && zeros && y && t1out, "null pointer");
    for (int i = 0; i < IVOSW_RES2_PROBE_NW; ++i) IVOSW_REQUIRE(w[i] && bias[i], "null pointer among the weights or biases");
    IVOSW_REQUIRE(form == 0 || form == 1, "form is 0 (res2_stage_kernel) or 1 (res2_chain_kernel)");
    IVOSW_REQUIRE(B > 0 && B <= 1024, "B must be in 1 .. 1024");
    IVOSW_ON_DEVICE_OF(y);
    hipStream_t st = as_stream(stream);
    // w / bias: conv1 x 4 | conv2 x 3 | conv3 x 3 | downsample
    const void* const* w1 = w; const void* const* w2 = w + 4; const void* const* w3 = w + 7; const void* wd = w[10];
    const float* const* b1 = bias; const float* const* b2 = bias + 4; const float* const* b3 = bias + 7; const float* bd = bias[10];
    char* f = static_cast<char*>(frag);
    int id = 0;
    if (form == 1) {
        IVOSW_REQUIRE(res2_chain_stream_bytes() <= IVOSW_RES2_PROBE_FRAG_BYTES, "internal: the fragment stream outgrew the probe's scratch");
        Res2ChainPackArgs q{};
        for (int b = 0; b < 4; ++b) { q.w1[b] = static_cast<const bf16_t*>(w1[b]); q.b1[b] = b1[b]; }
        for (int b = 0; b < 3; ++b) { q.w2[b] = static_cast<const bf16_t*>(w2[b]); q.b2[b] = b2[b]; q.w3[b] = static_cast<const bf16_t*>(w3[b]); q.b3[b] = b3[b]; }
        q.wd = static_cast<const bf16_t*>(wd); q.bd = bd; q.out = f;
        Res2ChainArgs c{};
        c.x = x; c.y = y; c.t1out = t1out; c.wstream = f; c.zeros = zeros; c.B = B; c.y_s2 = y_s2 ? 1 : 0; c.rev = rev ? 1 : 0;
        IVOSW_REQUIRE(res2_chain_ok(c), "internal: res2_chain_ok");
        id = tune_get("R2C_PERSIST", 1) != 0 ? 2 : 1;            // launch_res2_chain's own rule (res2_chain.hip)
        launch_res2_chain_pack(q, st);
        launch_res2_chain(c, st);
    } else {
        size_t off = 0;
        auto take = [&](size_t bytes) { char* p = f + off; off += align_up(bytes, 256); return p; };
        constexpr size_t E = 2;                                   // bytes per bf16
        char* fa0 = take(64 * 64 * E);
        char* fb[3]; for (int b = 0; b < 3; ++b) fb[b] = take(64 * 576 * E);
        char* cat_w = take(256 * 128 * E);
        char* cat_fw = take(256 * 128 * E);
        float* cat_b = reinterpret_cast<float*>(take(256 * sizeof(float)));
        char* fc[3] = {cat_fw, take(256 * 64 * E), take(256 * 64 * E)};
        char* fd[3] = {take(64 * 256 * E), take(64 * 256 * E), take(128 * 256 * E)};
        IVOSW_REQUIRE(off <= IVOSW_RES2_PROBE_FRAG_BYTES, "internal: the fragment copies outgrew the probe's scratch");
        Res2StageArgs q{};
        q.x = x; q.y = y; q.t1out = t1out; q.zeros = zeros; q.B = B; q.y_s2 = y_s2 ? 1 : 0; q.rev = rev ? 1 : 0;
        q.fa0 = fa0; q.ba0 = b1[0];
        for (int b = 0; b < 3; ++b) {
            q.fb[b] = fb[b]; q.bb[b] = b2[b];
            q.fc[b] = fc[b]; q.bc[b] = b == 0 ? cat_b : b3[b];
            q.fd[b] = fd[b]; q.bd[b] = b1[b + 1];
        }
        IVOSW_REQUIRE(res2_stage_ok(q), "internal: res2_stage_ok");
        launch_fragpack(w1[0], 64, 64, fa0, st);
        for (int b = 0; b < 3; ++b) launch_fragpack(w2[b], 64, 576, fb[b], st);
        launch_concat_k(w3[0], b3[0], 64, wd, bd, 64, 256, IVOSW_BF16, cat_w, cat_b, st);
        launch_fragpack(cat_w, 256, 128, cat_fw, st);
        for (int b = 1; b < 3; ++b) launch_fragpack(w3[b], 256, 64, fc[b], st);
        for (int b = 0; b < 3; ++b) launch_fragpack(w1[b + 1], b == 2 ? 128 : 64, 256, fd[b], st);
        launch_res2_stage(q, st);
    }
    if (ran) *ran = id + (y_s2 ? 4 : 0);
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}

// Test probe: one launch of stem_pool_kernel on the caller's ROI tiles and packed filter bank.
extern "C" int ivosw_stem_probe(const void* roi, const void* w, const float* bias, void* out, int B, int rev, ivosw_stream_t stream) {
    IVOSW_REQUIRE(roi && w && bias && out, "null pointer");
    IVOSW_REQUIRE(B > 0 && B <= 1024, "B must be in 1 .. 1024");
    IVOSW_ON_DEVICE_OF(out);
    launch_stem_pool(roi, w, bias, B, out, as_stream(stream), rev ? 1 : 0);
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}
#endif  // IVOSW_PROBES
