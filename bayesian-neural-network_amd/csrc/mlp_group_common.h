// Shared by the one-workgroup-per-agent group kernels (mlp_group.hip F6, bbb_group.hip F7): the thread grid, the block
// GEMM (one fma chain per output element, k ascending) and Adam's per-element update.
#pragma once
#include "bnn_device.h"
#include "../../include/bnn_hip.h"

namespace bnn {

constexpr int kMgThreads = 512;
constexpr int kMgTy = kMgThreads / 16;           // the GEMM thread grid: 16 columns x 32 rows
constexpr int kMgX = BNN_MLP_GROUP_MAX_BATCH * BNN_MLP_GROUP_MAX_IN;
constexpr int kMgH = BNN_MLP_GROUP_MAX_BATCH * BNN_MLP_GROUP_MAX_HIDDEN;

// C[m][n] = sum_k A(m, k) B(k, n) for m < M, n < N: tiles of (kMgTy TM) x (16 TN); thread (ty, tx) holds rows
// m0 + ty + kMgTy r and columns n0 + tx + 16 c.  k runs 0 .. K-1 in one fma chain per element.  Out-of-range rows and
// columns load a clamped (valid) index and are not written.
template <int TM, int TN, class FA, class FB, class FE>
__device__ __forceinline__ void block_gemm(int M, int N, int K, FA a, FB b, FE epi) {
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  for (int m0 = 0; m0 < M; m0 += kMgTy * TM) {
    for (int n0 = 0; n0 < N; n0 += 16 * TN) {
      int mi[TM], ni[TN];
#pragma unroll
      for (int r = 0; r < TM; ++r) mi[r] = min(m0 + ty + kMgTy * r, M - 1);
#pragma unroll
      for (int c = 0; c < TN; ++c) ni[c] = min(n0 + tx + 16 * c, N - 1);
      float acc[TM][TN];
#pragma unroll
      for (int r = 0; r < TM; ++r)
#pragma unroll
        for (int c = 0; c < TN; ++c) acc[r][c] = 0.f;
#pragma unroll 2
      for (int k = 0; k < K; ++k) {
        float av[TM], bv[TN];
#pragma unroll
        for (int r = 0; r < TM; ++r) av[r] = a(mi[r], k);
#pragma unroll
        for (int c = 0; c < TN; ++c) bv[c] = b(k, ni[c]);
#pragma unroll
        for (int r = 0; r < TM; ++r)
#pragma unroll
          for (int c = 0; c < TN; ++c) acc[r][c] = __builtin_fmaf(av[r], bv[c], acc[r][c]);
      }
#pragma unroll
      for (int r = 0; r < TM; ++r)
#pragma unroll
        for (int c = 0; c < TN; ++c) {
          const int m = m0 + ty + kMgTy * r, n = n0 + tx + 16 * c;
          if (m < M && n < N) epi(m, n, acc[r][c]);
        }
    }
  }
}

// Adam's per-element update: the arithmetic of adam_kernel (optim.hip), torch.optim.Adam's _single_tensor_adam.
struct AdamScalars {
  float step_size, sqrt_bc2, omb1, omb2, beta2f, eps, wd;
};
__device__ __forceinline__ void adam_elem(float* p, float* m, float* v, int i, float g, const AdamScalars& s) {
  const float pv = p[i];
  float mv = m[i], vv = v[i];
  const float gg = s.wd != 0.f ? __builtin_fmaf(s.wd, pv, g) : g;
  mv = mv + (gg - mv) * s.omb1;                              // exp_avg.lerp_(grad, 1 - beta1)
  vv = vv * s.beta2f + s.omb2 * gg * gg;                     // exp_avg_sq.mul_(beta2).addcmul_(g, g, 1 - beta2)
  const float denom = __builtin_sqrtf(vv) / s.sqrt_bc2 + s.eps;
  p[i] = pv - s.step_size * (mv / denom);
  m[i] = mv;
  v[i] = vv;
}

}  // namespace bnn
