// The ONE body of the halo bottleneck kernels (bottleneck_wide.hip: bneck_halo_kernel<C, WL>, bneck_halo128s_kernel,
// bneck_half16_kernel).  NOT a header in the usual sense: it is the text of a __global__ function's body and is included
// INSIDE each entry, after `using F = <form>;` (HaloTile16<C, WL> | HaloTile8x128 | HalfFrame16, see there), with the
// kernel argument named `p` (BneckWideArgs).
//
// Why text and not a __device__ __forceinline__ function template: these kernels sit at 255 / 128 VGPRs with hand-counted
// waits, and hipcc's code for them is not stable under inlining.  Moving the unchanged body of bneck_halo_kernel into a
// force-inlined function alone (no other edit) reorders block predecessors and use lists in the inliner's clone, and from
// there 600 - 1300 of ~3000 instructions per kernel change (operand order, register assignment, schedule, one
// compiler-placed s_waitcnt).  Included as text every entry compiles to exactly the instructions it had as a hand copy.
constexpr int C = F::C, CIN = F::CIN, HW = F::HW, BTY = F::BTY, BTX = F::BTX, HT = F::HTX, HR = F::HR, NGA = F::NGA, NXG = F::NXG;
constexpr int TPX = F::TPX, TPF = F::TPF, NSL = F::NSL, NCT = F::NCT, NG = F::NG;
constexpr int TPG = F::TPG, HA0 = F::HA0, HA1 = F::HA1, PB = F::PB, HB = F::HB, NPO = F::NPO, HC = NPO / 2;
constexpr int SLOT = F::SLOT, T1S = F::T1S, T2S = F::T2S, STG_OFF = F::STG_OFF, BIAS_OFF = F::BIAS_OFF;
constexpr bool WL = F::WL;
constexpr int HABL = F::TUNING ? HALO_ABL : 0;
__shared__ __attribute__((aligned(16))) unsigned char lds[F::LDS_BYTES];
const int tid = threadIdx.x, lane = tid & 63;
const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
const int lrow = lane & 31, lhalf = lane >> 5;
const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)lds;
const int L = (F::REV && p.rev) ? (int)gridDim.x - 1 - xcd_remap(blockIdx.x, gridDim.x) : xcd_remap(blockIdx.x, gridDim.x);
const int b = L / TPF, tl = L - b * TPF;
const int y0 = (TPX == 1 ? tl : tl / TPX) * BTY, x0 = TPX == 1 ? 0 : (tl % TPX) * BTX;   // TPX = 1: the half-frame walk, x0 = 0
const bf16_t* X = static_cast<const bf16_t*>(p.x) + (size_t)b * HW * HW * CIN;
bf16_t* Y = static_cast<bf16_t*>(p.y) + (size_t)b * HW * HW * CIN;
const bf16_t* zeros = static_cast<const bf16_t*>(p.zeros);
const int ctw = NG == 1 ? wave : wave % NCT, grp = NG == 1 ? 0 : wave / NCT;
// ba | bb | bc (2 C + 4 C floats) into the bias block by the 512 threads; visible after phase A's barriers.  (The 16-row form
// keeps its always-true guard tid < 4 C = 512 at C = 128, as its hand copy had it: hipcc lays the prologue out around it.)
static_assert(4 * C <= 1024, "bias block fill");
if (2 * C >= 512 || tid < 2 * C) *reinterpret_cast<float*>(lds + BIAS_OFF + tid * 4) = tid < C ? p.ba[tid] : p.bb[tid - C];
if ((4 * C >= 512 && BTY == 8) || tid < 4 * C) *reinterpret_cast<float*>(lds + BIAS_OFF + 2 * C * 4 + tid * 4) = p.bc[tid];
if constexpr (4 * C > 512) *reinterpret_cast<float*>(lds + BIAS_OFF + 2 * C * 4 + (tid + 512) * 4) = p.bc[tid + 512];
uint4 wn[4];                                     // first weight fragments of the next phase, requested one phase early
auto stamp = [&](int k) {
    if constexpr (F::STAMPS)
        if (p.ts && tid == 0) p.ts[(size_t)blockIdx.x * 8 + k] = __builtin_amdgcn_s_memtime();
};
stamp(0);
// WL: double step d of phase B = steps 2d, 2d + 1 = 8 consecutive fragments (8 KB) of each of the 4 channel tiles -> ring slot d & 1
auto wb_issue = [&](int d) {
    if constexpr (WL) {
        unsigned char* slot = lds + ((d & 1) ? F::WB1_OFF : F::WB0_OFF);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ct = wave >> 1, sub = (wave & 1) * 4 + j;
            dma16(wfrag(p.fb, ct, 9 * C / 16, d * 8 + sub, lane), slot + (ct * 8 + sub) * 1024);
        }
    }
};
// (Tried: picking the residual of output chunk 0 out of the ring while its x K-tile is resident in phase A, to save
// re-reading half of x in phase C — 64 more live registers on top of phase A's 96 accumulator + 32 weight registers
// = 141 VGPR spills.  Dropped.)

// ================================================================ phase A: t1 = relu(Wa x + ba) on the halo, K = CIN
{
    constexpr int NK = CIN / 64;
    f32x16 acc[TPG];
#pragma unroll
    for (int i = 0; i < TPG; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    const int rsub = lane >> 3, cpos = lane & 7;
    const int np = (NGA - wave + 7) / 8;         // row groups of this wave: wave, wave+8, ... < NGA (41: 6 for wave 0, else 5; 23: 3, wave 7: 2)
    const bf16_t* xsrc[NXG];
    unsigned okmask = 0;
#pragma unroll
    for (int i = 0; i < NXG; ++i) {
        const int g = wave + 8 * i;
        const int hr = g * 8 + rsub;
        const int hy = hr / HT, hx = hr - hy * HT;
        const int y = y0 - 1 + hy, x = x0 - 1 + hx;
        const bool ok = g < NGA && hr < HR && y >= 0 && y < HW && x >= 0 && x < HW;
        xsrc[i] = ok ? X + ((size_t)y * HW + x) * CIN + (cpos ^ ((hr >> 1) & 7)) * 8 : zeros;
        okmask |= ok ? (1u << i) : 0u;
    }
    auto issue_x = [&](int kt) {
        unsigned char* sb = lds + (kt % 3) * SLOT;
#pragma unroll
        for (int i = 0; i < NXG; ++i) {
            const int g = wave + 8 * i;
            if (g < NGA) dma16((HABL & 4) ? zeros : xsrc[i] + (((okmask >> i) & 1u) ? kt * 64 : 0), sb + g * 1024);
        }
    };
    u32x4 wq[2][4];
    auto load_w = [&](int kt, int set) {
        if constexpr (WL) {
            // K-tile kt of all NCT channel tiles = 16 fragments = 16 KB into ring slot kt & 1: wave w copies fragments (ct = w >> 1,
            // ks = 2 (w & 1), + 1); the queue order W(kt + 1) | X(kt + 2) per iteration is that of the register path
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int ct = wave >> 1, ks = (wave & 1) * 2 + j;
                dma16(wfrag(p.fa, ct, CIN / 16, kt * 4 + ks, lane), lds + STG_OFF + (kt & 1) * 16384 + (ct * 4 + ks) * 1024);
            }
        } else {
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
                asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(wq[set][ks]) : "v"(wfrag(p.fa, ctw, CIN / 16, kt * 4 + ks, lane)) : "memory");
        }
    };
    const int pt0 = grp * TPG;                   // pixel tiles pt0 .. ; of 11 the last group lacks its final tile
    const bool full = F::EVEN || grp + 1 < NG;   // a compile-time `true` for the 8-row tiles (6 = 2 x 3 = 1 x 6)
    load_w(0, 0);
    issue_x(0);
    issue_x(1);
    for (int kt2 = 0; kt2 < NK; kt2 += 2)
#pragma unroll
    for (int par = 0; par < 2; ++par) {
        const int kt = kt2 + par;
        if (kt + 1 < NK) wait_vmcnt_n(np); else wait_vmcnt<0>();   // only X(kt+1) is younger than W(kt)
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (kt + 1 < NK) load_w(kt + 1, par ^ 1);
        if (kt + 2 < NK) issue_x(kt + 2);        // slot (kt+2) % 3 == slot of tile kt-1: done for every wave
        const unsigned xb = lds_base + (kt % 3) * SLOT;
        u32x4 pf[TPG];
        // pixel tile pt0 + t of this lane = row (pt0 + t)*32 + lrow: one swizzle key for every t -> one address per k-step,
        // the tile as an immediate offset
        const unsigned xrow = xb + (pt0 * 32 + lrow) * ROWB;
        auto rd = [&](int ks, int half) {
            const unsigned a = xrow + (((2 * ks + lhalf) ^ ((lrow >> 1) & 7)) << 4);
            for_tiles<TPG>([&](auto tc) {
                constexpr int t = decltype(tc)::value;
                if (t >= (half ? HA0 : 0) && t < (half ? TPG : HA0) && (t < TPG - 1 || full)) pf[t] = lds_read_b128_o<t * 4096>(a);
            });
        };
        if constexpr (WL) {                      // this wave's four fragments of the K-tile: issued first, so every counted wait below covers them
            const unsigned wa = lds_base + STG_OFF + (kt & 1) * 16384 + ctw * 4096 + lane * 16;
            wq[par][0] = lds_read_b128_o<0>(wa); wq[par][1] = lds_read_b128_o<1024>(wa);
            wq[par][2] = lds_read_b128_o<2048>(wa); wq[par][3] = lds_read_b128_o<3072>(wa);
        }
        rd(0, 0);
        rd(0, 1);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const u32x4 w = wq[par][ks];
            if (full) lgkm_wait<HA1>(); else lgkm_wait<HA1 - 1>();       // half 0 landed (half 1 may be in flight)
#pragma unroll
            for (int t = 0; t < HA0; ++t) acc[t] = mfma_bf16(w, pf[t], acc[t]);
            if (ks < 3) rd(ks + 1, 0);
            if (ks < 3) lgkm_wait<HA0>(); else lgkm_wait<0>();
#pragma unroll
            for (int t = HA0; t < TPG; ++t)
                if (t < TPG - 1 || full) acc[t] = mfma_bf16(w, pf[t], acc[t]);
            if (ks < 3) rd(ks + 1, 1);
        }
    }
    __builtin_amdgcn_s_barrier();                // the ring is dead: its space becomes t1
    asm volatile("" ::: "memory");
    stamp(1);
    if constexpr (WL) {
        // phase B's first two double steps go out under the t1 epilogue: slot 0 = [t1 end, bias block) - part of the x ring until
        // the barrier above -, slot 1 = the staging area (phase A's weight ring, dead as well)
        wb_issue(0);
        wb_issue(1);
    } else {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) wn[ks] = *wfrag(p.fb, ctw, 9 * C / 16, ks, lane);
    }
    float4 bq[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) bq[g] = *reinterpret_cast<const float4*>(lds + BIAS_OFF + (ctw * 32 + 8 * g + 4 * lhalf) * 4);
#pragma unroll
    for (int i = 0; i < TPG; ++i) {
        if (i == TPG - 1 && !full) break;
        const int hr = (pt0 + i) * 32 + lrow;
        const int hy = hr / HT, hx = hr - hy * HT;
        const int y = y0 - 1 + hy, x = x0 - 1 + hx;
        const bool in = y >= 0 && y < HW && x >= 0 && x < HW;
        if (hr < HR) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                u32x2 pk;
                pk.x = relu2_bf16(acc[i][4 * g] + bq[g].x, acc[i][4 * g + 1] + bq[g].y) & (in ? 0xffffffffu : 0u);
                pk.y = relu2_bf16(acc[i][4 * g + 2] + bq[g].z, acc[i][4 * g + 3] + bq[g].w) & (in ? 0xffffffffu : 0u);
                // swizzle key from the COLUMN of the halo raster, not from the row index (round 5): phase B's 16-lane read groups are
                // {x .. x+3, x+12 .. x+15} of one raster line and {x+4 .. x+11} of the next - 16 consecutive columns, so (hx & 1, hx >> 1)
                // puts them on 16 different 16-byte slots (the line pitch 18 is even: a row's 128-byte half is its column's parity);
                // with (hr >> 1) & 7 two pairs of every group shared a slot (PMC: 32 % of the kernel's LDS cycles were conflicts).
                // ROWKEY: the form that still keys on the row.
                const int key = F::ROWKEY ? (hr >> 1) & 7 : (hx >> 1) & 7;
                lds_write_b64(lds_base + (ctw >> 1) * T1S + hr * ROWB + ((((ctw & 1) * 4 + g) ^ key) << 4) + 8 * lhalf, pk);
            }
        }
    }
    lds_wait();
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    stamp(2);
}

// ================================================================ phase B: t2 = relu(Wb (*) t1 + bb), 9 taps x NSL slices
{
    constexpr int KSB = 9 * C / 16, NSTEP = 9 * NSL;
    f32x16 acc[PB];
#pragma unroll
    for (int i = 0; i < PB; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    int hb[PB];                                  // halo row of this lane's output pixel at tap (0,0)
#pragma unroll
    for (int i = 0; i < PB; ++i) {
        const int q = (grp * PB + i) * 32 + lrow;
        hb[i] = (q >> 4) * HT + (q & 15);
    }
    if constexpr (WL) {
        // Software-pipelined form (round 5): the fragment reads of a k-step - 4 pixel tiles - are issued a WHOLE k-step ahead into the
        // other of two register sets, and across the step boundary the next step's four weight fragments and first pixel fragments
        // go out under the last k-step's MFMAs; the workgroup barrier of a double step sits in front of that prefetch.  (The
        // half-step lookahead of the register-weights form left every step opening with ~10 exposed LDS reads.)
        static_assert(!WL || (NSTEP % 2 == 0 && PB == 4 && !F::ROWKEY), "double steps of four pixel tiles, column key");
        u32x4 pfb[2][PB], wcb[2][4];
        auto rd_all = [&](int buf, int step, int ks) {
            const int tap = step / NSL, sl = step - tap * NSL;
            const unsigned key = (((lrow & 15) + tap % 3) >> 1) & 7;     // the raster column of every pixel tile of this lane: (q & 15) + kx
            const unsigned x = ((2 * ks + lhalf) ^ key) << 4;
#pragma unroll
            for (int i = 0; i < PB; ++i) pfb[buf][i] = lds_read_b128(lds_base + sl * T1S + (hb[i] + (tap / 3) * HT + (tap % 3)) * ROWB + x);
        };
        auto rd_w = [&](int buf, int step) {
            const unsigned wa = lds_base + (((step >> 1) & 1) ? F::WB1_OFF : F::WB0_OFF) + (ctw * 8 + (step & 1) * 4) * 1024 + lane * 16;
            wcb[buf][0] = lds_read_b128_o<0>(wa); wcb[buf][1] = lds_read_b128_o<1024>(wa);
            wcb[buf][2] = lds_read_b128_o<2048>(wa); wcb[buf][3] = lds_read_b128_o<3072>(wa);
        };
        // double step 0 has landed for this wave (double step 1's four pieces may be younger); the barrier publishes it
        wait_vmcnt<4>();
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        rd_w(0, 0);
        rd_all(0, 0, 0);
#pragma unroll 1
        for (int d = 0; d < NSTEP / 2; ++d) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int step = 2 * d + h;
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    if (ks < 3) {
                        rd_all((ks + 1) & 1, step, ks + 1);
                        lgkm_wait<PB>();
                    } else if (step + 1 < NSTEP) {
                        if (h == 1) {
                            // double step d + 1: this wave's pieces have landed (nothing younger is in flight), the barrier publishes
                            // them and says every wave has read the last weights of double step d: its slot takes d + 2
                            wait_vmcnt<0>();
                            __builtin_amdgcn_s_barrier();
                            asm volatile("" ::: "memory");
                            if (d + 2 < NSTEP / 2) wb_issue(d + 2);
                        }
                        rd_w(h ^ 1, step + 1);
                        rd_all(0, step + 1, 0);
                        lgkm_wait<PB + 4>();
                    } else {
                        lgkm_wait<0>();
                    }
#pragma unroll
                    for (int i = 0; i < PB; ++i) acc[i] = mfma_bf16(wcb[h][ks], pfb[ks & 1][i], acc[i]);
                }
            }
        }
    } else {
#pragma unroll 1
    for (int step = 0; step < NSTEP; ++step) {   // step = tap * NSL + slice
        const int tap = step / NSL, sl = step - tap * NSL;
        u32x4 wc[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) wc[ks] = as_u32x4(wn[ks]);
        if (step + 1 < NSTEP) {
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) wn[ks] = *wfrag(p.fb, ctw, KSB, (step + 1) * 4 + ks, lane);
        }
        unsigned rowa[PB], rkey[PB];             // rkey: per pixel tile, ROWKEY only
#pragma unroll
        for (int i = 0; i < PB; ++i) {
            const int hr = hb[i] + (tap / 3) * HT + (tap % 3);
            rowa[i] = lds_base + sl * T1S + hr * ROWB;
            rkey[i] = (hr >> 1) & 7;
        }
        const unsigned ckey = (((lrow & 15) + tap % 3) >> 1) & 7;    // the raster column of every pixel tile of this lane: (q & 15) + kx
        u32x4 pf[PB];
        auto rd = [&](int ks, int half) {
            const int ch = 2 * ks + lhalf;
#pragma unroll
            for (int i = 0; i < HB; ++i) pf[half * HB + i] = lds_read_b128(rowa[half * HB + i] + ((ch ^ (F::ROWKEY ? rkey[half * HB + i] : ckey)) << 4));
        };
        rd(0, 0);
        rd(0, 1);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            lgkm_wait<HB>();
#pragma unroll
            for (int i = 0; i < HB; ++i) acc[i] = mfma_bf16(wc[ks], pf[i], acc[i]);
            if (ks < 3) rd(ks + 1, 0);
            if (ks < 3) lgkm_wait<HB>(); else lgkm_wait<0>();
#pragma unroll
            for (int i = HB; i < PB; ++i) acc[i] = mfma_bf16(wc[ks], pf[i], acc[i]);
            if (ks < 3) rd(ks + 1, 1);
        }
    }
    }
    __builtin_amdgcn_s_barrier();                // every wave is done reading t1: t2 takes its place
    asm volatile("" ::: "memory");
    stamp(3);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) wn[ks] = *wfrag(p.fc, wave, C / 16, ks, lane);
    float4 bq[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) bq[g] = *reinterpret_cast<const float4*>(lds + BIAS_OFF + (C + ctw * 32 + 8 * g + 4 * lhalf) * 4);
#pragma unroll
    for (int i = 0; i < PB; ++i) {
        const int px = (grp * PB + i) * 32 + lrow;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            u32x2 pk;
            pk.x = relu2_bf16(acc[i][4 * g] + bq[g].x, acc[i][4 * g + 1] + bq[g].y);
            pk.y = relu2_bf16(acc[i][4 * g + 2] + bq[g].z, acc[i][4 * g + 3] + bq[g].w);
            lds_write_b64(lds_base + (ctw >> 1) * T2S + px * ROWB + ((((ctw & 1) * 4 + g) ^ ((px >> 1) & 7)) << 4) + 8 * lhalf, pk);
        }
    }
    lds_wait();
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    stamp(4);
}

// ================================================================ phase C: y = relu(Wc t2 + bc + x), NCH chunks of 8 channel tiles
{
    constexpr int KSC = C / 16, NCH = F::NCH, NSTEP = NCH * NSL;
    f32x16 acc[NPO];
    float* stg = reinterpret_cast<float*>(lds + STG_OFF + wave * 4096);
    const int u = lane & 3, prr = lane >> 2;
    auto pix = [&](int q) { return (size_t)((y0 + (q >> 4)) * HW + x0 + (q & 15)) * CIN; };   // tile pixel q -> frame offset
#pragma unroll 1
    for (int chunk = 0; chunk < NCH; ++chunk) {
        const int ct = chunk * 8 + wave;
        const size_t cofs = (size_t)ct * 32 + 8 * u;
        uint4 rr[2];                             // residual of the first pixel tile: in flight under the chunk's MFMAs
#pragma unroll
        for (int it = 0; it < 2; ++it) rr[it] = (HABL & 1) ? make_uint4(0, 0, 0, 0) : *reinterpret_cast<const uint4*>(X + pix(it * 16 + prr) + cofs);
        {
            float4 bq[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) bq[g] = *reinterpret_cast<const float4*>(lds + BIAS_OFF + (2 * C + ct * 32 + 8 * g + 4 * lhalf) * 4);
#pragma unroll
            for (int i = 0; i < NPO; ++i)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    acc[i][4 * g] = bq[g].x; acc[i][4 * g + 1] = bq[g].y; acc[i][4 * g + 2] = bq[g].z; acc[i][4 * g + 3] = bq[g].w;
                }
        }
#pragma unroll 1
        for (int sl = 0; sl < NSL; ++sl) {
            u32x4 wc[4];
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) wc[ks] = as_u32x4(wn[ks]);
            const int nxt = chunk * NSL + sl + 1;
            if (nxt < NSTEP) {
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) wn[ks] = *wfrag(p.fc, (nxt / NSL) * 8 + wave, KSC, (nxt % NSL) * 4 + ks, lane);
            }
            const unsigned tb = lds_base + sl * T2S;
            u32x4 pf[NPO];
            const unsigned trow = tb + lrow * ROWB;
            auto rd = [&](int ks, int half) {
                const unsigned a = trow + (((2 * ks + lhalf) ^ ((lrow >> 1) & 7)) << 4);
                for_tiles<NPO>([&](auto tc) {
                    constexpr int t = decltype(tc)::value;
                    if (t >= (half ? HC : 0) && t < (half ? NPO : HC)) pf[t] = lds_read_b128_o<t * 4096>(a);
                });
            };
            rd(0, 0);
            rd(0, 1);
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                lgkm_wait<HC>();
#pragma unroll
                for (int i = 0; i < HC; ++i) acc[i] = mfma_bf16(wc[ks], pf[i], acc[i]);
                if (ks < 3) rd(ks + 1, 0);
                if (ks < 3) lgkm_wait<HC>(); else lgkm_wait<0>();
#pragma unroll
                for (int i = HC; i < NPO; ++i) acc[i] = mfma_bf16(wc[ks], pf[i], acc[i]);
                if (ks < 3) rd(ks + 1, 1);
            }
        }
        if (chunk == NCH - 1) stamp(5);
#pragma unroll
        for (int i = 0; i < NPO; ++i) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int slot = (2 * g + lhalf) ^ (lrow & 7);
                *reinterpret_cast<float4*>(stg + lrow * 32 + slot * 4) = make_float4(acc[i][4 * g], acc[i][4 * g + 1], acc[i][4 * g + 2], acc[i][4 * g + 3]);
            }
            uint4 rn[2];
            if (i < NPO - 1) {
#pragma unroll
                for (int it = 0; it < 2; ++it) rn[it] = (HABL & 1) ? make_uint4(0, 0, 0, 0) : *reinterpret_cast<const uint4*>(X + pix((i + 1) * 32 + it * 16 + prr) + cofs);
            }
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                const int pr = it * 16 + prr;
                const float4 v0 = *reinterpret_cast<const float4*>(stg + pr * 32 + (((2 * u) ^ (pr & 7)) << 2));
                const float4 v1 = *reinterpret_cast<const float4*>(stg + pr * 32 + (((2 * u + 1) ^ (pr & 7)) << 2));
                const unsigned w4[4] = {rr[it].x, rr[it].y, rr[it].z, rr[it].w};
                const float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
                unsigned pk[4];
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    pk[k] = relu2_bf16(v[2 * k] + __uint_as_float(w4[k] << 16), v[2 * k + 1] + __uint_as_float(w4[k] & 0xffff0000u));
                if ((HABL & 2) && pk[0] != 0x12345678u) continue;
                if (F::TUNING && ABL(p.debug, 16) && ((((i * 32 + pr) >> 4) | (i * 32 + pr)) & 1)) continue;      // ablation YS2ABL: even pixels only (see bneck_wide_body)
                *reinterpret_cast<uint4*>(Y + pix(i * 32 + pr) + cofs) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
            }
            if (i < NPO - 1) { rr[0] = rn[0]; rr[1] = rn[1]; }
        }
    }
    stamp(6);
}
