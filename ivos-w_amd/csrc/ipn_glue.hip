// IPN session glue feeding the assessment path — the IPN twin of seg_epilogue.hip and atnet_epilogue.hip.
//
// Reference (utils/utils_ipn.py):
//     Dilate_mask(mask, num_objects): per object o = 0 .. num_objects one cv2.dilate of (mask == o) with the 3x3 cross, 2 iterations,
//         new_mask[dmask == 1] = o                                                                                       :26-34
//     To_np_label(all_E, K, index): all_E[0].cpu().numpy()[inv_index] -> np.argmax(axis=0).astype(uint8)                 :75-81
// and, around the IPN clone's model.Run, the merge of an interaction's estimate with the earlier rounds' by the Get_weight weights
// (:37-72), frame by frame, and all_P = probs[0].transpose(1, 0) (eval_agent_ipn.py:261).
//
// ipn_dilate_kernel: ONE launch for n scribble maps.  Two iterations of the 3x3 cross are the radius-2 diamond |dy| + |dx| <= 2; cv2's
// default border never contributes to a dilation (pixels outside the image are skipped); the ascending object loop with overwrite is a
// maximum; -1 (and every value outside 0 .. num_objects, which no (mask == o) sees) is the identity of that maximum.
//
// ipn_merge_kernel: one interaction's end for the whole session, one streaming pass.  Per frame f, pixel p and canonical channel i,
// read from position inv[i]:  e = fadd_rn(fmul_rn(w_new[f], all_E), fmul_rn(w_old[f], prev_E)) written back in place - three separately
// rounded fp32 operations on every frame, never an FMA (#pragma clang fp contract(off), bare operators: see seg_epilogue.hip) - then
// the canonical probability plane (only when the channel order is not the identity: otherwise all_E IS the object-major store) and the
// label: the first maximum over i, a NaN counting as the maximum and the first NaN winning, as numpy's argmax has it.
// The blend rule is the DEFINITION here: IPN's model.Run lives in the external clone, not in the reference tree, so parity with the
// clone's own merge is unpinned (as the ATNet label rule's parity with its clone is).
//
// The per-frame weights travel inside the kernel arguments, IPN_MAX_FRAMES frames per launch, as the sequence table of the ragged
// entries does: no allocation, no copy, capture-safe.  Both kernels are plain streaming kernels: no LDS, no atomics, no scratch.
// HBM-bound: the merge moves 4 B x K x (2 reads + 1 write [+ 1 write with probs]) + 5 B of labels per pixel and frame.
#include "lane_group.h"
#include <limits.h>

namespace ivosw {

namespace {
constexpr int IPN_MAX_K = 32;
constexpr int IPN_MAX_FRAMES = 256;                  // frames per merge launch (their weights are kernel arguments)
constexpr long IPN_MAX_ELEMS = 1L << 40;             // K * T * H * W and (K - 1) * probs_stride_c + T * H * W: offsets are long, bytes fit by far

struct DilateArgs {
    const int8_t* mask;    // [n][H][W]
    int8_t* out;           // [n][H][W]
    int n, H, W, num_objects;
};

struct MergeArgs {
    float* E;              // [K][T][HW]: read, and written when prev
    const float* prev;     // [K][T][HW] or nullptr
    float* probs;          // canonical channel i at probs + i * sc, or nullptr
    long sc;
    uint8_t* label_u8;     // [T][HW] or nullptr
    float* label_f32;      // [T][HW] or nullptr
    long chan;             // T * HW: the channel stride of E and prev
    int K, HW, f0;         // this launch covers the frames f0 .. f0 + gridDim.y - 1
    uint8_t inv[IPN_MAX_K];                          // canonical channel i sits at position inv[i]
    float w_new[IPN_MAX_FRAMES], w_old[IPN_MAX_FRAMES];
};

// a scribble value as the reference's (mask == o) loop sees it: o in 0 .. num_objects, everything else -1
__device__ __forceinline__ int scribble(int v, int num_objects) { return (unsigned)v <= (unsigned)num_objects ? v : -1; }

// One row of the diamond: best[p] = max(best[p], row[x0 + p + d]) over |d| <= R, columns outside the image skipped.  V = 4 reads the
// aligned 4-byte words left of, at and right of x0 (W % 4 == 0: a word is wholly inside the row or wholly outside); V = 1 reads bytes.
template <int V, int R>
__device__ __forceinline__ void dilate_row(const int8_t* row, int x0, int W, int num_objects, int (&best)[V]) {
    int c[V + 4];                                    // c[k]: the value at column x0 - 2 + k
#pragma unroll
    for (int k = 0; k < V + 4; ++k) c[k] = -1;
    if constexpr (V == 4) {
        const uint32_t mid = *reinterpret_cast<const uint32_t*>(row + x0);
#pragma unroll
        for (int k = 0; k < 4; ++k) c[2 + k] = scribble((int)(int8_t)(mid >> (8 * k)), num_objects);
        if (R > 0 && x0 >= 4) {
            const uint32_t left = *reinterpret_cast<const uint32_t*>(row + x0 - 4);
            c[0] = scribble((int)(int8_t)(left >> 16), num_objects);
            c[1] = scribble((int)(int8_t)(left >> 24), num_objects);
        }
        if (R > 0 && x0 + 4 < W) {
            const uint32_t right = *reinterpret_cast<const uint32_t*>(row + x0 + 4);
            c[V + 2] = scribble((int)(int8_t)right, num_objects);
            c[V + 3] = scribble((int)(int8_t)(right >> 8), num_objects);
        }
    } else {
#pragma unroll
        for (int k = 2 - R; k <= 2 + R; ++k) {
            const int x = x0 - 2 + k;
            if (x >= 0 && x < W) c[k] = scribble((int)row[x], num_objects);
        }
    }
#pragma unroll
    for (int p = 0; p < V; ++p)
#pragma unroll
        for (int d = -R; d <= R; ++d) best[p] = max(best[p], c[p + 2 + d]);
}
}  // namespace

// V = pixels per thread, consecutive in a row (V = 4 needs W % 4 == 0 and 4-byte aligned mask and out).  blockIdx.y walks the maps.
template <int V>
__global__ __launch_bounds__(256) void ipn_dilate_kernel(DilateArgs a) {
    const unsigned wq = (unsigned)a.W / V;
    const unsigned item = blockIdx.x * 256u + threadIdx.x;                 // H * W <= INT_MAX (checked by the launcher)
    if (item >= (unsigned)a.H * wq) return;
    const int y = (int)(item / wq), x0 = (int)(item - (unsigned)y * wq) * V;
    const long plane = (long)a.H * a.W;
    for (int m = blockIdx.y; m < a.n; m += gridDim.y) {
        const int8_t* row = a.mask + m * plane + (long)y * a.W;
        int best[V];
#pragma unroll
        for (int p = 0; p < V; ++p) best[p] = -1;
        if (y >= 2) dilate_row<V, 0>(row - 2 * (long)a.W, x0, a.W, a.num_objects, best);
        if (y >= 1) dilate_row<V, 1>(row - a.W, x0, a.W, a.num_objects, best);
        dilate_row<V, 2>(row, x0, a.W, a.num_objects, best);
        if (y + 1 < a.H) dilate_row<V, 1>(row + a.W, x0, a.W, a.num_objects, best);
        if (y + 2 < a.H) dilate_row<V, 0>(row + 2 * (long)a.W, x0, a.W, a.num_objects, best);
        store_bytes(a.out + m * plane + (long)y * a.W + x0, best);
    }
}

// V = pixels per thread, consecutive in a frame (V = 4 needs HW % 4 == 0 and every pointer and stride on the 16-byte grid; label_u8 on
// the 4-byte grid).  blockIdx.y is the frame within the launch: its weights are wave-uniform.
template <int V>
__global__ __launch_bounds__(256) void ipn_merge_kernel(MergeArgs a) {
#pragma clang fp contract(off)
    const unsigned p0 = (blockIdx.x * 256u + threadIdx.x) * V;             // HW <= INT_MAX: below 2^32 with the grid's round-up
    if (p0 >= (unsigned)a.HW) return;
    const long fo = (long)(a.f0 + (int)blockIdx.y) * a.HW + p0;            // offset inside a channel
    const float wn = a.w_new[blockIdx.y], wo = a.w_old[blockIdx.y];
    const bool want_label = a.label_u8 || a.label_f32;
    float best[V];
    int am[V];
    for (int i = 0; i < a.K; ++i) {
        const long off = (long)a.inv[i] * a.chan + fo;
        float v[V];
        load_group(a.E + off, v);
        if (a.prev) {
            float q[V];
            load_group(a.prev + off, q);
#pragma unroll
            for (int p = 0; p < V; ++p) {
                const float m1 = wn * v[p];
                const float m2 = wo * q[p];
                v[p] = m1 + m2;
            }
            store_group(a.E + off, v);
        }
        if (a.probs) store_group(a.probs + (long)i * a.sc + fo, v);
        if (want_label) {
#pragma unroll
            for (int p = 0; p < V; ++p)                                    // running FIRST maximum; a NaN is the maximum and is never replaced
                if (i == 0 || (best[p] == best[p] && (v[p] > best[p] || v[p] != v[p]))) { best[p] = v[p]; am[p] = i; }
        }
    }
    if (!want_label) return;
    if (a.label_u8) store_bytes(a.label_u8 + fo, am);
    if (a.label_f32) store_group_as(a.label_f32 + fo, am);
}

}  // namespace ivosw

extern "C" int ivosw_ipn_dilate(const int8_t* mask, int n, int H, int W, int num_objects, int8_t* out, ivosw_stream_t stream) {
    using namespace ivosw;
    IVOSW_REQUIRE(mask, "null mask");
    IVOSW_REQUIRE(out, "null out");
    IVOSW_REQUIRE(n >= 1 && H >= 1 && W >= 1, "bad shape");
    IVOSW_REQUIRE(num_objects >= 0 && num_objects <= 126, "num_objects outside [0, 126]");
    IVOSW_REQUIRE((long)H * W <= INT_MAX, "frame too large for 32-bit pixel indices");
    IVOSW_REQUIRE(out != mask, "out must not be mask (a pixel reads its neighbours)");
    IVOSW_ON_DEVICE_OF(mask);
    DilateArgs a{mask, out, n, H, W, num_objects};
    const int V = !scalar_forced("IVOSW_IPN_SCALAR") && W % 4 == 0 && on_grid(4, mask, out) ? 4 : 1;
    const dim3 grid(lane_blocks((long)H * W, V), (unsigned)(n < 65535 ? n : 65535));
    hipStream_t st = as_stream(stream);
    dispatch_lanes<4, 1>(V, [&](auto v) { hipLaunchKernelGGL((ipn_dilate_kernel<decltype(v)::value>), grid, dim3(256), 0, st, a); });
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}

extern "C" int ivosw_ipn_merge(float* all_E, const float* prev_E, int K, int T, int H, int W, const float* w_new32, const float* w_old32,
                               const int* index, float* probs, long probs_stride_c, uint8_t* label_u8, float* label_f32,
                               ivosw_stream_t stream) {
    using namespace ivosw;
    IVOSW_REQUIRE(all_E, "null all_E");
    IVOSW_REQUIRE(K >= 1 && K <= IPN_MAX_K, "K outside [1, 32]");
    IVOSW_REQUIRE(!label_u8 || K <= 256, "uint8 labels need K <= 256");
    IVOSW_REQUIRE(T >= 1 && H >= 1 && W >= 1, "bad shape");
    IVOSW_REQUIRE((long)H * W <= INT_MAX, "frame too large for 32-bit pixel indices");
    const long HW = (long)H * W;
    IVOSW_REQUIRE(T <= IPN_MAX_ELEMS / HW / K, "K * T * H * W above 2^40 elements");
    const long chan = (long)T * HW;
    MergeArgs a{};
    if (index) {
        bool seen[IPN_MAX_K] = {};
        for (int j = 0; j < K; ++j) {
            IVOSW_REQUIRE(index[j] >= 0 && index[j] < K && !seen[index[j]], "index is not a permutation of 0 .. K-1");
            seen[index[j]] = true;
            a.inv[index[j]] = (uint8_t)j;
        }
    } else {
        for (int j = 0; j < K; ++j) a.inv[j] = (uint8_t)j;
    }
    IVOSW_REQUIRE(!prev_E || (w_new32 && w_old32), "prev_E needs w_new32 and w_old32");
    if (probs) {
        IVOSW_REQUIRE(K == 1 || probs_stride_c >= chan, "probability channels overlap");
        IVOSW_REQUIRE(K == 1 || probs_stride_c <= (IPN_MAX_ELEMS - chan) / (K - 1), "probs_stride_c too large");
        const uintptr_t e0 = (uintptr_t)all_E, e1 = e0 + (uintptr_t)K * chan * sizeof(float);
        const uintptr_t p0 = (uintptr_t)probs, p1 = p0 + (uintptr_t)((K - 1) * (K == 1 ? 0 : probs_stride_c) + chan) * sizeof(float);
        IVOSW_REQUIRE(p1 <= e0 || e1 <= p0, "probs overlaps all_E");
    }
    IVOSW_REQUIRE(prev_E || probs || label_u8 || label_f32, "no output requested");
    IVOSW_ON_DEVICE_OF(all_E);
    a.E = all_E; a.prev = prev_E; a.probs = probs; a.sc = K == 1 ? 0 : probs_stride_c; a.label_u8 = label_u8; a.label_f32 = label_f32;
    a.chan = chan; a.K = K; a.HW = (int)HW;
    const int V = !scalar_forced("IVOSW_IPN_SCALAR") && HW % 4 == 0 && (a.sc % 4 == 0 || !probs) && on_grid(16, all_E, prev_E, probs, label_f32) &&
                          on_grid(4, label_u8) ? 4 : 1;
    const unsigned gx = lane_blocks(HW, V);
    hipStream_t st = as_stream(stream);
    for (int f0 = 0; f0 < T; f0 += IPN_MAX_FRAMES) {
        const int nf = T - f0 < IPN_MAX_FRAMES ? T - f0 : IPN_MAX_FRAMES;
        a.f0 = f0;
        if (prev_E) {
            memcpy(a.w_new, w_new32 + f0, nf * sizeof(float));
            memcpy(a.w_old, w_old32 + f0, nf * sizeof(float));
        }
        dispatch_lanes<4, 1>(V, [&](auto v) { hipLaunchKernelGGL((ipn_merge_kernel<decltype(v)::value>), dim3(gx, nf), dim3(256), 0, st, a); });
        IVOSW_CHECK_LAUNCH();
    }
    return IVOSW_OK;
}
