// AssessNet's score head fitted on the device: the reference's optimiser loop (quality_assessment.py:230-270, 286) applied to fc1
// (2048 -> 1) on the pooled features of a frozen trunk, n_steps minibatch steps of up to 32 independent fits in ONE launch.
//
// The loop is a latency chain of dependent steps over a few MB of L2-resident rows - the shape of the LSTM recurrence kernels of
// brain.hip: one persistent workgroup per chain (fit), many chains side by side, nothing shared between them but the read-only
// feature bank.  1024 threads; thread t owns channels 2t and 2t + 1 of w, the momentum buffer and the gradient accumulator in
// registers for the whole call, every thread carries the bias state redundantly (all threads compute the same bits), and w is mirrored
// in 8 KB of LDS for the row dots.  Per step:
//   phase 1  wave v takes rows v, v + 16, ...: 8 x 16-byte loads of the row per lane against w in LDS, a wave butterfly, e_n to LDS
//   barrier
//   phase 2  every thread walks n = 0 .. B-1 in order: the step's sums (every thread the same) and its two channels of sum e_n x_n
//            (8-byte loads, 512 B per wave and row, L2-hot from phase 1), then clamp + SGD and the refreshed LDS mirror
//   barrier
// The arithmetic is the definition stated in include/ivosw.h (every fp32 operation rounded by itself: this unit is compiled with
// -ffp-contract=off, ivos-w_amd/build.py) and restated in numpy in tests/head_fit_ref.py.
// No global atomics, no cross-workgroup synchronisation, no fences, no scratch, no allocation: capture-safe, bit-identical run to run,
// and a fit computes the same bits alone or as member k of a 32-fit launch (a workgroup reads nothing another one writes).
#include "common.h"

namespace ivosw {

namespace {
constexpr int HF_C = 2048, HF_THREADS = 1024, HF_WAVES = HF_THREADS / 64;

struct HeadFitArgs {
    const float* feat;        // [M][2048]
    const float* target;      // [M]
    const uint8_t* valid;     // [M]
    const int32_t* order;     // [n_fits][n_steps][B]
    const float* lr;          // [n_fits][n_steps]
    float *w, *b, *buf_w, *buf_b, *grad_w, *grad_b;      // [n_fits][2048] / [n_fits]
    int32_t* steps_taken;     // [n_fits]
    float* log;               // [n_fits][n_steps][3]
    int n_steps, B;
    float momentum[IVOSW_HEAD_FIT_MAX_FITS], weight_decay[IVOSW_HEAD_FIT_MAX_FITS];
    uint32_t zero_grad, eval_only;      // bit k = fit k
};

__device__ __forceinline__ float hf_clamp(float g) { return fminf(fmaxf(g, -1.0f), 1.0f); }

// one parameter's clamp + SGD step (include/ivosw.h); s = the step's sum of e_n x_n for this parameter, k = fl(2 / c)
__device__ __forceinline__ void hf_update(float s, float k, bool zero_grad, bool first, float mom, float wd, float lr, float& p, float& buf,
                                          float& G) {
    const float g = k * s;
    G = hf_clamp((zero_grad ? 0.0f : G) + g);
    const float d = G + wd * p;
    buf = first ? d : mom * buf + d;
    p = p - lr * buf;
}
}  // namespace

__global__ __launch_bounds__(HF_THREADS) void head_fit_kernel(HeadFitArgs a) {
    __shared__ float w_s[HF_C];
    __shared__ float e_s[IVOSW_HEAD_FIT_MAX_BATCH];
    __shared__ uint8_t v_s[IVOSW_HEAD_FIT_MAX_BATCH];
    const int fit = blockIdx.x, t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int B = a.B, n_steps = a.n_steps;
    const bool zero_grad = (a.zero_grad >> fit) & 1u, eval_only = (a.eval_only >> fit) & 1u;
    const float mom = a.momentum[fit], wd = a.weight_decay[fit];
    const size_t c0 = (size_t)fit * HF_C + 2 * t;

    float2 w = *reinterpret_cast<const float2*>(a.w + c0);
    float2 buf = *reinterpret_cast<const float2*>(a.buf_w + c0);
    float2 G = *reinterpret_cast<const float2*>(a.grad_w + c0);
    float b = a.b[fit], buf_b = a.buf_b[fit], G_b = a.grad_b[fit];
    int taken = a.steps_taken[fit];
    *reinterpret_cast<float2*>(w_s + 2 * t) = w;
    __syncthreads();

    const int32_t* order = a.order + (size_t)fit * n_steps * B;
    const float* lr_tab = a.lr + (size_t)fit * n_steps;
    float* log = a.log + (size_t)fit * n_steps * 3;

    for (int step = 0; step < n_steps; ++step, order += B) {
        // ---- phase 1: e_n = (x_n . w + b) - target_n for the valid rows
        for (int n = wave; n < B; n += HF_WAVES) {
            const int idx = order[n];
            const float4* row = reinterpret_cast<const float4*>(a.feat + (size_t)idx * HF_C);
            float4 x[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) x[j] = row[j * 64 + lane];
            float acc = 0.0f;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float4 ww = *reinterpret_cast<const float4*>(w_s + (j * 64 + lane) * 4);
                acc = acc + x[j].x * ww.x;
                acc = acc + x[j].y * ww.y;
                acc = acc + x[j].z * ww.z;
                acc = acc + x[j].w * ww.w;
            }
            acc = wave_sum(acc);
            if (lane == 0) {
                const bool ok = a.valid[idx] != 0;
                v_s[n] = ok ? 1 : 0;
                e_s[n] = ok ? (acc + b) - a.target[idx] : 0.0f;
            }
        }
        __syncthreads();

        // ---- phase 2: the step's sums in row order, then clamp + SGD on this thread's two channels (and the bias, by every thread)
        float se2 = 0.0f, sabs = 0.0f, se = 0.0f, s0 = 0.0f, s1 = 0.0f;
        int c = 0;
        const float* col = a.feat + 2 * t;
#pragma unroll 4
        for (int n = 0; n < B; ++n) {
            const float2 x = *reinterpret_cast<const float2*>(col + (size_t)order[n] * HF_C);
            const float e = e_s[n];
            if (v_s[n]) {
                se2 = se2 + e * e;
                sabs = sabs + fabsf(e);
                se = se + e;
                s0 = s0 + e * x.x;
                s1 = s1 + e * x.y;
                ++c;
            }
        }
        float l0 = 0.0f, l1 = 0.0f, l2 = 0.0f;
        if (c > 0) {
            const float cf = (float)c;
            l0 = se2 / cf; l1 = sabs / cf; l2 = cf;
            if (!eval_only) {
                const float k = 2.0f / cf, lr = lr_tab[step];
                const bool first = taken == 0;
                hf_update(s0, k, zero_grad, first, mom, wd, lr, w.x, buf.x, G.x);
                hf_update(s1, k, zero_grad, first, mom, wd, lr, w.y, buf.y, G.y);
                hf_update(se, k, zero_grad, first, mom, wd, lr, b, buf_b, G_b);
                ++taken;
                *reinterpret_cast<float2*>(w_s + 2 * t) = w;
            }
        }
        if (t == 0) { log[step * 3] = l0; log[step * 3 + 1] = l1; log[step * 3 + 2] = l2; }
        __syncthreads();
    }

    if (!eval_only) {
        *reinterpret_cast<float2*>(a.w + c0) = w;
        *reinterpret_cast<float2*>(a.buf_w + c0) = buf;
        *reinterpret_cast<float2*>(a.grad_w + c0) = G;
        if (t == 0) { a.b[fit] = b; a.buf_b[fit] = buf_b; a.grad_b[fit] = G_b; a.steps_taken[fit] = taken; }
    }
}

}  // namespace ivosw

extern "C" int ivosw_head_fit(const float* feat, const float* target, const uint8_t* valid, int M, const int32_t* order, const float* lr,
                              int n_fits, int n_steps, int B, const float* momentum, const float* weight_decay, const int* zero_grad,
                              const int* eval_only, float* w, float* b, float* buf_w, float* buf_b, float* grad_w, float* grad_b,
                              int32_t* steps_taken, float* log, ivosw_stream_t stream) {
    using namespace ivosw;
    IVOSW_REQUIRE(feat && target && valid && order && lr, "null pointer (feat, target, valid, order or lr)");
    IVOSW_REQUIRE(momentum && weight_decay && zero_grad && eval_only, "null pointer (a per-fit host table)");
    IVOSW_REQUIRE(w && b && buf_w && buf_b && grad_w && grad_b && steps_taken && log, "null pointer (state or log)");
    IVOSW_REQUIRE(M >= 1, "M must be at least 1");
    IVOSW_REQUIRE(n_fits >= 1 && n_fits <= IVOSW_HEAD_FIT_MAX_FITS, "n_fits outside 1 .. 32");
    IVOSW_REQUIRE(B >= 1 && B <= IVOSW_HEAD_FIT_MAX_BATCH, "B outside 1 .. 256");
    IVOSW_REQUIRE(n_steps >= 1 && (long)n_fits * n_steps * B < (1L << 31), "n_steps must be positive and n_fits * n_steps * B below 2^31");
    IVOSW_REQUIRE((reinterpret_cast<uintptr_t>(feat) & 15) == 0, "feat must be 16-byte aligned");
    IVOSW_REQUIRE(((reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(buf_w) | reinterpret_cast<uintptr_t>(grad_w)) & 7) == 0,
                  "w, buf_w and grad_w must be 8-byte aligned");
    HeadFitArgs a{};
    for (int k = 0; k < n_fits; ++k) {
        IVOSW_REQUIRE(momentum[k] == momentum[k] && weight_decay[k] == weight_decay[k], "a momentum or weight_decay is NaN");
        a.momentum[k] = momentum[k]; a.weight_decay[k] = weight_decay[k];
        if (zero_grad[k]) a.zero_grad |= 1u << k;
        if (eval_only[k]) a.eval_only |= 1u << k;
    }
    IVOSW_ON_DEVICE_OF(w);
    a.feat = feat; a.target = target; a.valid = valid; a.order = order; a.lr = lr;
    a.w = w; a.b = b; a.buf_w = buf_w; a.buf_b = buf_b; a.grad_w = grad_w; a.grad_b = grad_b;
    a.steps_taken = steps_taken; a.log = log; a.n_steps = n_steps; a.B = B;
    hipLaunchKernelGGL(head_fit_kernel, dim3(n_fits), dim3(HF_THREADS), 0, as_stream(stream), a);
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}
