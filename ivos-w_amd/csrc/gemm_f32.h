// Small-shape fp32 GEMM on the f32-input matrix cores: the descriptor and the launchers (kernels and notes: gemm_f32.hip).
// Serves the Brain's batched (non-recurrent) contractions off the fused chain (brain.hip, dqn_step.hip).
#pragma once
#include "adam.h"
#include "common.h"

namespace ivosw {

struct GemmF32 {
    const float* A;   // A(m,k) = A[m*sam + k*sak]
    const float* A2;  // optional: A(m,k) += A2[m*sam + k*sak] on load (dgx = dG[fw] + dG[bw] without a pass of its own)
    const float* B;   // B(k,n) = B[k*sbk + n*sbn]
    float* C;         // C[m*ldc + n]   (split-K: slab z at C + z*M*ldc)
    int M, N, K;
    long sam, sak, sbk, sbn;
    int ldc;
    const float* bias;   // [N] added in the epilogue, or nullptr
    const float* mask;   // same indexing as C; result *= (mask > 0), or nullptr
    int relu;            // max(.,0) epilogue
    int relu_a;          // max(.,0) applied to A on load
    int splitk;          // gridDim.z
};

void launch_gemm_f32(const GemmF32& g, hipStream_t st);
// C[M,N] (contiguous) = A^T-style wgrad through split-K slabs.
void launch_gemm_f32_splitk(GemmF32 g, float* out, float* slabs, int nsplit, hipStream_t st);
// n GEMMs (every one eligible for the 16-byte path, else they are launched one by one) as one grouped launch
void launch_gemm_f32_group(const GemmF32* gs, int n, hipStream_t st);
// the fixed-order reduction of up to six slab sets (adam.h: ReduceGroup) in one launch
void launch_reduce_group(const ReduceGroup& rg, hipStream_t st);

}  // namespace ivosw
