// Brain (bidirectional shared-cell LSTM Q-network) forward: the form choice and launchers of the recurrence (lstm_fwd.h), both forward
// drivers and the batched and ragged forward entries.  The ranking entries are brain_rank.hip, the Double-DQN loss, the hand-derived
// backward and the one-call step dqn_step.hip.
//
// Reference arithmetic: Brain.forward (models/agent.py:33-64).
//
// Layout: the shared cell's input-side gates W_ih*e_t do not depend on the direction, so they are one
// batched GEMM over all (n,t); only h*W_hh^T is sequential.  The recurrence kernel keeps the whole
// 512x128 fp32 W_hh in VGPRs (one gate column per thread, 512 threads = the CU's register file) and
// walks the T steps with h broadcast from LDS: rows (sample x direction) map to workgroups, so a
// 128-sample minibatch fills all 256 CUs.  fp32 throughout (exact fma chains); MFMA is used for the
// dense batched contractions only (gemm_f32.h).
#ifdef IVOSW_PROBES
#include "../../include/ivosw_probe.h"
#endif
#include <mutex>

#include "gemm_f32.h"
#include "lstm_fwd.h"

namespace ivosw {

// ---------------------------------------------------------------- small kernels
// a1[row][j] = relu(W1[j,:].x[row] + b1[j])        (encoder_fc1 + relu, agent.py:49)
// rows [0, rows0) read x, rows [rows0, rows) read x2 (the policy pass runs [s'; s] as one batch without concatenating them)
__global__ void enc1_kernel(const float* __restrict__ prm, const float* __restrict__ x, const float* __restrict__ x2, int rows0, int rows,
                            float* __restrict__ a1) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * HD) return;
    const int row = i >> 7, j = i & 127;
    const float* xr = row < rows0 ? x + (size_t)row * 2 : x2 + (size_t)(row - rows0) * 2;
    const float x0 = xr[0], x1 = xr[1];
    const float v = fmaf(x1, prm[O_W1 + j * 2 + 1], fmaf(x0, prm[O_W1 + j * 2], prm[O_B1 + j]));
    a1[i] = fmaxf(v, 0.f);
}

// q[row] = d1[row,:].w4 + b4                       (decoder_fc2, agent.py:61)
__global__ void dec2_kernel(const float* __restrict__ prm, const float* __restrict__ d1, int rows, float* __restrict__ q) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float* r = d1 + (size_t)row * HD;
    float s = r[lane] * prm[O_W4 + lane] + r[lane + 64] * prm[O_W4 + lane + 64];
    s = wave_sum(s);
    if (lane == 0) q[row] = s + prm[O_B4];
}

// ---------------------------------------------------------------- forward driver (FwdBufs, FwdPass: brain_fwd.h)
int rows_per_wg(int rows) {
    // one workgroup per CU holds W_hh in registers; more rows than CUs -> several rows share a WG
    if (rows <= 256) return 1;
    if (rows <= 512) return 2;
    return 4;
}

unsigned long long* g_lstm_probe_bwd = nullptr;
unsigned long long* g_lstm_probe = nullptr;
static LstmFwd lstm_fwd_args(const FwdPass& f, int T) {
    LstmFwd lf{};
    lf.ts = g_lstm_probe;
    lf.whh = f.prm + O_WHH; lf.gx = f.b->gx; lf.hs = f.b->hs; lf.N = f.N; lf.T = T;
    lf.keep_from = f.b->gates ? f.b->keep_from : f.N;
    lf.gates = f.b->gates; lf.cs = f.b->cs; lf.hprev = f.b->hprev;
    return lf;
}
// The recurrence's form is chosen in ONE place and launched in ONE place: both forward drivers below and the test probe
// (ivosw_lstm_fwd_probe) go through these.  A form's number: R = 1, 2, 4 rows per workgroup of lstm_fwd_kernel<R>, 10 + R of
// lstm_fwd_quad_kernel<R>, LSTM_FORM_MFMA the 4x4x1 MFMA kernel (four rows per workgroup, at least eight rows).
constexpr int LSTM_FORM_QUAD = 10, LSTM_FORM_MFMA = 20;
static bool lstm_fwd_form_known(int form) {
    const int R = form > LSTM_FORM_QUAD ? form - LSTM_FORM_QUAD : form;
    return form == LSTM_FORM_MFMA || R == 1 || R == 2 || R == 4;
}
static int lstm_fwd_form_for(int N) {
    const int R = rows_per_wg(2 * N);
    if (!tune_get("LSTM_QUAD", 1)) return R;
    if (tune_get("LSTM_MFMA", 1) && 2 * N >= 8) return LSTM_FORM_MFMA;
    return LSTM_FORM_QUAD + R;
}
static void launch_lstm_fwd(int form, const LstmFwd& lf, hipStream_t st) {
    const int rows = 2 * lf.N;
    const int R = form == LSTM_FORM_MFMA ? 4 : form > LSTM_FORM_QUAD ? form - LSTM_FORM_QUAD : form, nwg = (rows + R - 1) / R;
    switch (form) {
        case LSTM_FORM_MFMA: hipLaunchKernelGGL(lstm_fwd_mfma_kernel, dim3(nwg), dim3(512), 0, st, lf); break;
        case LSTM_FORM_QUAD + 1: hipLaunchKernelGGL(lstm_fwd_quad_kernel<1>, dim3(nwg), dim3(512), 0, st, lf); break;
        case LSTM_FORM_QUAD + 2: hipLaunchKernelGGL(lstm_fwd_quad_kernel<2>, dim3(nwg), dim3(512), 0, st, lf); break;
        case LSTM_FORM_QUAD + 4: hipLaunchKernelGGL(lstm_fwd_quad_kernel<4>, dim3(nwg), dim3(512), 0, st, lf); break;
        case 1: hipLaunchKernelGGL(lstm_fwd_kernel<1>, dim3(nwg), dim3(512), 0, st, lf); break;
        case 2: hipLaunchKernelGGL(lstm_fwd_kernel<2>, dim3(nwg), dim3(512), 0, st, lf); break;
        default: hipLaunchKernelGGL(lstm_fwd_kernel<4>, dim3(nwg), dim3(512), 0, st, lf); break;
    }
}
// the policy pass and the target pass in one launch of the MFMA recurrence (each pass has at least eight rows)
static void launch_lstm_fwd_pair(const LstmFwd& a, const LstmFwd& b, hipStream_t st) {
    LstmFwdPair pr{};
    pr.j[0] = a;
    pr.j[1] = b;
    pr.first1 = (2 * a.N + 3) / 4;
    hipLaunchKernelGGL(lstm_fwd_mfma_pair_kernel, dim3(pr.first1 + (2 * b.N + 3) / 4), dim3(512), 0, st, pr);
}
static void launch_lstm_fwd_ragged(const float* whh, const float* gx, float* hs, const SeqTable& tab, int n_seqs, hipStream_t st) {
    hipLaunchKernelGGL(lstm_fwd_quad_ragged_kernel, dim3(2 * n_seqs), dim3(512), 0, st, whh, gx, hs, tab);
}
// recurrence + decoder in one kernel: a pair of samples' 2 T rows of [h_fw | h_bw] must fit the kernel's dynamic LDS
constexpr size_t MEGA_LDS_LIMIT = 150 * 1024;
static bool fwd_mega_fits(int T) { return mega_lds_bytes(T) <= MEGA_LDS_LIMIT; }
static void launch_fwd_mega(const FwdMega* jobs, int n, hipStream_t st) {
    static std::once_flag once;
    std::call_once(once, [] { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(brain_fwd_mega_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)MEGA_LDS_LIMIT); (void)hipGetLastError(); });
    FwdMegaPair mp{};
    int wgs[2] = {0, 0};
    for (int i = 0; i < n; ++i) {
        mp.j[i] = jobs[i];
        wgs[i] = (jobs[i].N + 1) / 2;
    }
    mp.first1 = wgs[0];
    hipLaunchKernelGGL(brain_fwd_mega_kernel, dim3(wgs[0] + wgs[1]), dim3(512), mega_lds_bytes(jobs[0].T), st, mp);
}

bool fused_forward_ok(const FwdPass* f, int n) {
    if (!tune_get("DQN_FUSED", 1) || !tune_get("LSTM_QUAD", 1)) return false;
    if (n == 2) return tune_get("LSTM_MFMA", 1) && 2 * f[0].N >= 8 && 2 * f[1].N >= 8;   // the pair launch is the MFMA recurrence
    return true;
}
void brain_forward_fused(const FwdPass* f, int n, int T, hipStream_t st, const EncDraw* draw) {
    EncGroup eg{};
    if (draw) eg.dr = *draw;
    DecGroup dg{};
    int tiles[2] = {0, 0};
    for (int i = 0; i < n; ++i) {
        const int rows = f[i].N * T, keep_row = f[i].b->gates ? f[i].b->keep_from * T : rows;
        tiles[i] = (rows + FM - 1) / FM;
        eg.j[i] = EncJob{f[i].prm, f[i].x, f[i].x2 ? f[i].x2 : f[i].x, f[i].b->gx, f[i].b->a1, f[i].b->e,
                         f[i].x2 ? f[i].N0 * T : rows, rows, keep_row};
        dg.j[i] = DecJob{f[i].prm, f[i].b->hs, f[i].b->d1, f[i].b->q, rows, keep_row};
    }
    eg.first1 = dg.first1 = tiles[0];
    hipLaunchKernelGGL(enc_fused_kernel, dim3(tiles[0] + tiles[1]), dim3(256), 0, st, eg, O_W1, O_B1, O_W2, O_B2, O_WIH);
    // recurrence + decoder in one kernel (FWD_MEGA, default OFF: measured 201 us per DQN step against 185.5 us for the separate
    // decoder launch - the decoder's 16 us run on 192 workgroups after their recurrences instead of on the whole chip) when every
    // pass is batched enough for the MFMA recurrence and the pair's 2 T rows of [h_fw | h_bw] fit LDS
    bool mega = tune_get("FWD_MEGA", 0) && tune_get("LSTM_MFMA", 1) && fwd_mega_fits(T);
    for (int i = 0; i < n; ++i) mega = mega && 2 * f[i].N >= 8;
    if (mega) {
        FwdMega jobs[2] = {};
        for (int i = 0; i < n; ++i) {
            const FwdBufs& b = *f[i].b;
            const int keep_from = b.gates ? b.keep_from : f[i].N;
            jobs[i] = FwdMega{f[i].prm, b.gx, b.hs, b.gates, b.cs, b.hprev, b.d1, b.q, f[i].N, T, keep_from, keep_from, tune_get("MEGA_DBG", 0)};
        }
        launch_fwd_mega(jobs, n, st);
        return;
    }
    // (fused_forward_ok: LSTM_QUAD is on here, so the form is a quad or the MFMA one)
    if (n == 2) launch_lstm_fwd_pair(lstm_fwd_args(f[0], T), lstm_fwd_args(f[1], T), st);
    else launch_lstm_fwd(lstm_fwd_form_for(f[0].N), lstm_fwd_args(f[0], T), st);
    hipLaunchKernelGGL(dec_fused_kernel, dim3(tiles[0] + tiles[1]), dim3(256), 0, st, dg, O_W3, O_B3, O_W4, O_B4);
}

// the un-fused chain (DQN_FUSED or LSTM_QUAD off); x2 != nullptr: samples [0, N0) come from x, [N0, N) from x2
void brain_forward_internal(const float* prm, const float* x, int N, int T, const FwdBufs& b, hipStream_t st, const float* x2, int N0) {
    const int rows = N * T;
    hipLaunchKernelGGL(enc1_kernel, dim3((rows * HD + 255) / 256), dim3(256), 0, st, prm, x, x2 ? x2 : x, x2 ? N0 * T : rows, rows, b.a1);
    GemmF32 g{};
    // e = a1 * W2^T + b2
    g.A = b.a1; g.sam = 128; g.sak = 1; g.B = prm + O_W2; g.sbk = 1; g.sbn = 128; g.C = b.e; g.ldc = 128;
    g.M = rows; g.N = 128; g.K = 128; g.bias = prm + O_B2; g.splitk = 1;
    launch_gemm_f32(g, st);
    // gx = e * Wih^T
    g = GemmF32{};
    g.A = b.e; g.sam = 128; g.sak = 1; g.B = prm + O_WIH; g.sbk = 1; g.sbn = 128; g.C = b.gx; g.ldc = 512;
    g.M = rows; g.N = 512; g.K = 128; g.splitk = 1;
    launch_gemm_f32(g, st);
    launch_lstm_fwd(lstm_fwd_form_for(N), lstm_fwd_args(FwdPass{prm, x, x2, N, N0, &b}, T), st);
    // d1 = relu(relu(hcat) * W3^T + b3)
    g = GemmF32{};
    g.A = b.hs; g.sam = 256; g.sak = 1; g.relu_a = 1; g.B = prm + O_W3; g.sbk = 1; g.sbn = 256; g.C = b.d1; g.ldc = 128;
    g.M = rows; g.N = 128; g.K = 256; g.bias = prm + O_B3; g.relu = 1; g.splitk = 1;
    launch_gemm_f32(g, st);
    hipLaunchKernelGGL(dec2_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, prm, b.d1, rows, b.q);
}

}  // namespace ivosw

using namespace ivosw;

// a forward pass's workspace: the end of a counting run of its one carve
static size_t fwd_ws_bytes(int N, int T) {
    Arena count;
    carve_fwd(count, N, T, -1);
    return count.bytes();
}

extern "C" size_t ivosw_brain_ws_bytes(int N, int T) {
    if (N <= 0 || T <= 0) return 0;
    return fwd_ws_bytes(N, T);
}

extern "C" int ivosw_brain_forward(const float* params, const float* x, int N, int T, float* q, void* ws,
                                   size_t ws_bytes, ivosw_stream_t stream) {
    IVOSW_REQUIRE(params && x && q && ws, "null pointer");
    IVOSW_ON_DEVICE_OF(q);
    IVOSW_REQUIRE(N > 0 && T > 0, "N and T must be positive");
    if (ws_bytes < ivosw_brain_ws_bytes(N, T)) {
        set_error("ivosw_brain_forward: workspace %zu < %zu", ws_bytes, ivosw_brain_ws_bytes(N, T));
        return IVOSW_ERR_WS;
    }
    hipStream_t st = as_stream(stream);
    Arena ar(ws);
    FwdBufs b = carve_fwd(ar, N, T, -1);
    b.q = q;                              // the decoder writes the caller's buffer (a device-to-device copy was a launch of its own)
    const FwdPass fp{params, x, nullptr, N, 0, &b};
    if (fused_forward_ok(&fp, 1)) brain_forward_fused(&fp, 1, T, st);
    else brain_forward_internal(params, x, N, T, b, st);
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}

// ---------------------------------------------------------------- ragged forward: K sequences, each of its own length
extern "C" long ivosw_brain_ragged_rows(const int* lengths, int n_seqs) {
    IVOSW_REQUIRE(lengths, "null pointer");
    return ragged_rows(__func__, lengths, n_seqs, nullptr);
}

extern "C" size_t ivosw_brain_ragged_ws_bytes(long rows) {
    if (rows <= 0 || rows > RAGGED_MAX_ROWS) return 0;
    return fwd_ws_bytes(1, (int)rows);
}

extern "C" int ivosw_brain_forward_ragged(const float* params, const float* x, const int* lengths, int n_seqs, float* q, void* ws,
                                          size_t ws_bytes, ivosw_stream_t stream) {
    IVOSW_REQUIRE(params && x && lengths && q && ws, "null pointer");
    SeqTable tab;
    const long rows = ragged_rows(__func__, lengths, n_seqs, &tab);
    if (rows < 0) return IVOSW_ERR_ARG;
    IVOSW_ON_DEVICE_OF(q);
    if (ws_bytes < ivosw_brain_ragged_ws_bytes(rows)) {
        set_error("ivosw_brain_forward_ragged: workspace %zu < %zu", ws_bytes, ivosw_brain_ragged_ws_bytes(rows));
        return IVOSW_ERR_WS;
    }
    hipStream_t st = as_stream(stream);
    Arena ar(ws);
    FwdBufs b = carve_fwd(ar, 1, (int)rows, -1);          // the flat rows are one [1, R] batch to the row-wise encoder and decoder
    b.q = q;
    const FwdPass fp{params, x, nullptr, 1, 0, &b};
    if (fused_forward_ok(&fp, 1)) {
        const int R = (int)rows, tiles = (R + FM - 1) / FM;
        EncGroup eg{};
        DecGroup dg{};
        eg.j[0] = EncJob{params, x, x, b.gx, b.a1, b.e, R, R, R};
        dg.j[0] = DecJob{params, b.hs, b.d1, q, R, R};
        eg.first1 = dg.first1 = tiles;
        hipLaunchKernelGGL(enc_fused_kernel, dim3(tiles), dim3(256), 0, st, eg, O_W1, O_B1, O_W2, O_B2, O_WIH);
        launch_lstm_fwd_ragged(params + O_WHH, b.gx, b.hs, tab, n_seqs, st);
        hipLaunchKernelGGL(dec_fused_kernel, dim3(tiles), dim3(256), 0, st, dg, O_W3, O_B3, O_W4, O_B4);
    } else {
        // DQN_FUSED or LSTM_QUAD switched off: the N = 1 path of ivosw_brain_forward per sequence, on that sequence's slices
        for (int k = 0; k < n_seqs; ++k) {
            const size_t r0 = (size_t)tab.row_off[k];
            FwdBufs bk = b;
            bk.a1 += r0 * 128; bk.e += r0 * 128; bk.gx += r0 * 512; bk.hs += r0 * 256; bk.d1 += r0 * 128; bk.q += r0;
            const FwdPass fk{params, x + r0 * 2, nullptr, 1, 0, &bk};
            if (fused_forward_ok(&fk, 1)) brain_forward_fused(&fk, 1, lengths[k], st);
            else brain_forward_internal(params, x + r0 * 2, 1, lengths[k], bk, st);
        }
    }
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}

/* Tuning probe: subsequent fused forwards stamp s_memtime at four points of recurrence step T/2 per workgroup into ts
 * ([workgroups, 8] uint64 on the device: 0-3 the step's four points, 4 kernel entry, 5 weights in registers, 6 last step done; NULL switches the probe off).  tools/lstm_probe.py. */
#ifdef IVOSW_PROBES
extern "C" int ivosw_lstm_probe(unsigned long long* ts, unsigned long long* ts_bwd) {
    g_lstm_probe = ts;
    g_lstm_probe_bwd = ts_bwd;          // BPTT kernel: 0 step start, 1 gate gradients written, 2 barrier passed, 3 matvec done, 4 / 5 loop start / end, 6 steps
    return IVOSW_OK;
}

// ---------------------------------------------------------------- test probes of the forward kernels (include/ivosw_probe.h)
extern "C" int ivosw_enc_fused_probe(int njobs, const float* const* prm, const float* const* x, const float* const* x2, const int* rows0,
                                     const int* rows, const int* keep_row, float* const* gx, float* const* a1, float* const* e,
                                     ivosw_stream_t stream) {
    IVOSW_REQUIRE(prm && x && x2 && rows0 && rows && keep_row && gx && a1 && e, "null pointer");
    PROBE_COVERS(njobs == 1 || njobs == 2, "one or two jobs");
    EncGroup eg{};
    int tiles[2] = {0, 0};
    for (int i = 0; i < njobs; ++i) {
        IVOSW_REQUIRE(prm[i] && x[i] && x2[i] && gx[i] && a1[i] && e[i], "null pointer");
        PROBE_COVERS(rows[i] >= 1 && rows[i] <= (1 << 20), "rows must be 1 .. 2^20");
        PROBE_COVERS(rows0[i] >= 0 && rows0[i] <= rows[i] && keep_row[i] >= 0 && keep_row[i] <= rows[i], "0 <= rows0, keep_row <= rows");
        PROBE_COVERS(aligned16({prm[i]}), "the parameter arena must be 16-byte aligned");
        eg.j[i] = EncJob{prm[i], x[i], x2[i], gx[i], a1[i], e[i], rows0[i], rows[i], keep_row[i]};
        tiles[i] = (rows[i] + FM - 1) / FM;
    }
    IVOSW_ON_DEVICE_OF(gx[0]);
    eg.first1 = tiles[0];
    hipLaunchKernelGGL(enc_fused_kernel, dim3(tiles[0] + tiles[1]), dim3(256), 0, as_stream(stream), eg, O_W1, O_B1, O_W2, O_B2, O_WIH);
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}

extern "C" int ivosw_dec_fused_probe(int njobs, const float* const* prm, const float* const* hs, const int* rows, const int* keep_row,
                                     float* const* d1, float* const* q, ivosw_stream_t stream) {
    IVOSW_REQUIRE(prm && hs && rows && keep_row && d1 && q, "null pointer");
    PROBE_COVERS(njobs == 1 || njobs == 2, "one or two jobs");
    DecGroup dg{};
    int tiles[2] = {0, 0};
    for (int i = 0; i < njobs; ++i) {
        IVOSW_REQUIRE(prm[i] && hs[i] && d1[i] && q[i], "null pointer");
        PROBE_COVERS(rows[i] >= 1 && rows[i] <= (1 << 20), "rows must be 1 .. 2^20");
        PROBE_COVERS(keep_row[i] >= 0 && keep_row[i] <= rows[i], "0 <= keep_row <= rows");
        PROBE_COVERS(aligned16({prm[i], hs[i]}), "the parameter arena and hs must be 16-byte aligned");
        dg.j[i] = DecJob{prm[i], hs[i], d1[i], q[i], rows[i], keep_row[i]};
        tiles[i] = (rows[i] + FM - 1) / FM;
    }
    IVOSW_ON_DEVICE_OF(q[0]);
    dg.first1 = tiles[0];
    hipLaunchKernelGGL(dec_fused_kernel, dim3(tiles[0] + tiles[1]), dim3(256), 0, as_stream(stream), dg, O_W3, O_B3, O_W4, O_B4);
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}

// what every recurrence probe checks of one argument set; 0 or the error code with the message set
static int lstm_fwd_probe_args(const char* who, const float* whh, const float* gx, float* hs, float* gates, float* cs, float* hprev, int N, int T,
                               int keep_from, LstmFwd* lf) {
    if (!(whh && gx && hs)) { set_error("%s: null pointer", who); return IVOSW_ERR_ARG; }
    if ((gates == nullptr) != (cs == nullptr) || (gates == nullptr) != (hprev == nullptr)) {
        set_error("%s: not covered: gates, cs and hprev are given together or not at all", who);
        return IVOSW_ERR_ARG;
    }
    if (!(N >= 1 && T >= 1 && (long long)N * T <= (1 << 20))) { set_error("%s: not covered: N, T >= 1 and N*T <= 2^20", who); return IVOSW_ERR_ARG; }
    if (!(keep_from >= 0 && keep_from <= N)) { set_error("%s: not covered: 0 <= keep_from <= N", who); return IVOSW_ERR_ARG; }
    if (!aligned16({whh})) { set_error("%s: not covered: whh must be 16-byte aligned", who); return IVOSW_ERR_ARG; }
    *lf = LstmFwd{};
    lf->whh = whh; lf->gx = gx; lf->hs = hs; lf->gates = gates; lf->cs = cs; lf->hprev = hprev; lf->N = N; lf->T = T;
    lf->keep_from = gates ? keep_from : N;               // (as lstm_fwd_args)
    return IVOSW_OK;
}

extern "C" int ivosw_lstm_fwd_probe(const float* whh, const float* gx, float* hs, float* gates, float* cs, float* hprev, int N, int T,
                                    int keep_from, int form, int* ran, ivosw_stream_t stream) {
    LstmFwd lf;
    if (const int rc = lstm_fwd_probe_args(__func__, whh, gx, hs, gates, cs, hprev, N, T, keep_from, &lf)) return rc;
    PROBE_COVERS(form == 0 || lstm_fwd_form_known(form), "form must be 0 (the product's choice), 1, 2, 4 (plain), 11, 12, 14 (quad) or 20 (mfma)");
    PROBE_COVERS(form != LSTM_FORM_MFMA || 2 * N >= 8, "the mfma form needs at least eight rows (2 N >= 8)");
    IVOSW_ON_DEVICE_OF(hs);
    if (form == 0) form = lstm_fwd_form_for(N);
    launch_lstm_fwd(form, lf, as_stream(stream));
    IVOSW_CHECK_LAUNCH();
    if (ran) *ran = form;
    return IVOSW_OK;
}

extern "C" int ivosw_lstm_fwd_pair_probe(const float* const* whh, const float* const* gx, float* const* hs, float* const* gates, float* const* cs,
                                         float* const* hprev, const int* N, int T, const int* keep_from, ivosw_stream_t stream) {
    IVOSW_REQUIRE(whh && gx && hs && gates && cs && hprev && N && keep_from, "null pointer");
    LstmFwd lf[2];
    for (int i = 0; i < 2; ++i) {
        if (const int rc = lstm_fwd_probe_args(__func__, whh[i], gx[i], hs[i], gates[i], cs[i], hprev[i], N[i], T, keep_from[i], &lf[i])) return rc;
        PROBE_COVERS(2 * N[i] >= 8, "the pair launch is the mfma form: each job needs at least eight rows (2 N >= 8)");
    }
    IVOSW_ON_DEVICE_OF(hs[0]);
    launch_lstm_fwd_pair(lf[0], lf[1], as_stream(stream));
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}

extern "C" int ivosw_lstm_fwd_ragged_probe(const float* whh, const float* gx, float* hs, const int* lengths, int n_seqs, ivosw_stream_t stream) {
    IVOSW_REQUIRE(whh && gx && hs && lengths, "null pointer");
    PROBE_COVERS(aligned16({whh}), "whh must be 16-byte aligned");
    SeqTable tab;
    if (ragged_rows(__func__, lengths, n_seqs, &tab) < 0) return IVOSW_ERR_ARG;
    IVOSW_ON_DEVICE_OF(hs);
    launch_lstm_fwd_ragged(whh, gx, hs, tab, n_seqs, as_stream(stream));
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}

extern "C" int ivosw_fwd_mega_probe(int njobs, const float* const* prm, const float* const* gx, float* const* hs, float* const* gates,
                                    float* const* cs, float* const* hprev, float* const* d1, float* const* q, const int* N, int T,
                                    const int* keep_from, const int* hs_from, ivosw_stream_t stream) {
    IVOSW_REQUIRE(prm && gx && hs && gates && cs && hprev && d1 && q && N && keep_from && hs_from, "null pointer");
    PROBE_COVERS(njobs == 1 || njobs == 2, "one or two jobs");
    FwdMega jobs[2] = {};
    for (int i = 0; i < njobs; ++i) {
        IVOSW_REQUIRE(prm[i] && d1[i] && q[i], "null pointer");
        LstmFwd lf;
        if (const int rc = lstm_fwd_probe_args(__func__, prm[i] + O_WHH, gx[i], hs[i], gates[i], cs[i], hprev[i], N[i], T, keep_from[i], &lf)) return rc;
        PROBE_COVERS(2 * N[i] >= 8, "each job needs at least eight rows (2 N >= 8)");
        PROBE_COVERS(hs_from[i] >= 0 && hs_from[i] <= N[i], "0 <= hs_from <= N");
        PROBE_COVERS(fwd_mega_fits(T), "2 T rows of [h_fw | h_bw] exceed the kernel's LDS");
        jobs[i] = FwdMega{prm[i], gx[i], hs[i], gates[i], cs[i], hprev[i], d1[i], q[i], N[i], T, lf.keep_from, hs_from[i], 0};
    }
    IVOSW_ON_DEVICE_OF(q[0]);
    launch_fwd_mega(jobs, njobs, as_stream(stream));
    IVOSW_CHECK_LAUNCH();
    return IVOSW_OK;
}
#endif  // IVOSW_PROBES
