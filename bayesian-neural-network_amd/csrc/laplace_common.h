// What the diagonal (laplace.hip: F17, F18) and the Kronecker-factored (kfac.hip: F20) Laplace posteriors share on the device:
// the masked-delta operand gz, the tile of the deltas of the layer below g_x = gz . W (ONE device function, so every kernel
// that hands deltas down gives the same bits), the squared-input operand, and the final stage of the fp64 evidence.
#pragma once

#include "bnn_device.h"
#include "dense_tile.h"
#include "../../include/bnn_hip.h"

namespace bnn {
namespace {

// B(i, n) = x[n, i]^2
struct SqOpnd {
  Opnd o;
};

template <bool KC>
__device__ __forceinline__ void fetch_seg(const SqOpnd& q, int K, int r0, int k0, int s, float v[8]) {
  fetch_seg<KC>(q.o, K, r0, k0, s, v);
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] *= v[j];
}

// A(r, o) = gz[r, o] = (y == NULL || y[r mod B, o] > 0) ? gy[r, o] : 0 (k = o contiguous)
struct GzOpnd {
  const float* gy;
  const float* y;
  int B, ld, rows, vec;
};

template <bool KC>
__device__ __forceinline__ void fetch_seg(const GzOpnd& q, int K, int r0, int k0, int s, float v[8]) {
  static_assert(KC, "gz is read along its contiguous (out) dimension");
  const int r = r0 + (s >> 2), k = k0 + 8 * (s & 3);
  const int valid = r < q.rows ? min(8, max(0, K - k)) : 0;
  const Opnd g{q.gy, nullptr, 1.f, q.ld, q.rows, q.vec};
  load8(g, (long)r * q.ld + k, 1, valid, q.vec, v);
  if (q.y && valid > 0) {
    float m[8];
    const Opnd y{q.y, nullptr, 1.f, q.ld, q.B, q.vec};
    load8(y, (long)(r % q.B) * q.ld + k, 1, valid, q.vec, m);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = m[j] > 0.f ? v[j] : 0.f;
  }
}

// One 64 x 64 tile of g_x [R, IN] = gz [R, OUT] . W [OUT, IN], masked by the input of data row r mod B: the item of
// bnn_laplace_layer, bnn_laplace_glm_layer, bnn_kfac_layer and bnn_kfac_glm_rotate (P: the kernel's parameters; the same
// code, so the same bits).  A(r, o) = gz, k (= o) contiguous; B(i, o) = W[o, i], i contiguous
template <typename TX, typename P>
__device__ __forceinline__ void gx_tile(const P& p, int item, uint4* lds, f32x4 acc[2][2]) {
  const int tm = item / p.tiles_n, tn = item - tm * p.tiles_n;
  const GzOpnd A{p.gy, p.y, p.B, p.OUT, p.R, p.vec_g};
  const Opnd Bo{p.w, nullptr, 1.f, p.IN, p.IN, p.vec_w};
  gemm_tile<TX, true, false>(A, Bo, tm * kT, tn * kT, p.OUT, lds, acc);
  tile_epilogue(lds, acc, tm * kT, tn * kT, p.R, p.IN, [&](int row, int col0, int ncol, float o[4]) {
    if (p.gx_mask) {
      const long mat = (long)(row % p.B) * p.IN + col0;
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (c < ncol) o[c] = p.x[mat + c] > 0.f ? o[c] : 0.f;
    }
    store_group(p.gx + (long)row * p.IN + col0, o, ncol, p.vec_gx != 0);
  });
}

struct Precisions {
  double tau[BNN_LAPLACE_MAX_PRECISIONS];
  int n;
};

// The evidence's stage 2: one block.  ws[q * blocks + b]: quantity q of stage-1 block b; q < n the log-determinant sums of
// the candidates, q == n the sum of w^2.  Thread t sums blocks t, t + 256, ... in order, then the tree; thread 0 forms the
// evidences and the maximum.
__global__ __launch_bounds__(kThreads) void laplace_evidence_final(const Precisions pr, const double* __restrict__ ws, int blocks,
                                                                   double n_params, const double* __restrict__ record,
                                                                   double* __restrict__ log_evidence, int* __restrict__ best_index,
                                                                   double* __restrict__ best) {
  __shared__ double part[kThreads];
  __shared__ double tot[BNN_LAPLACE_MAX_PRECISIONS + 1];
#pragma unroll 1
  for (int q = 0; q <= pr.n; ++q) {
    double s = 0.0;
    for (int b = threadIdx.x; b < blocks; b += kThreads) s += ws[(long)q * blocks + b];
    const double v = tree_sum<kThreads>(s, part);
    if (threadIdx.x == 0) tot[q] = v;
  }
  if (threadIdx.x != 0) return;
  const double loglik = record[0], w2 = tot[pr.n];
  int bi = 0;
  double bv = 0.0;
  for (int g = 0; g < pr.n; ++g) {
    const double tau = pr.tau[g];
    const double v = loglik - 0.5 * tau * w2 + 0.5 * n_params * log(tau) - 0.5 * tot[g];
    log_evidence[g] = v;
    if (g == 0 || v > bv) {                                    // the lowest index on ties
      bv = v;
      bi = g;
    }
  }
  if (best_index) *best_index = bi;
  if (best) {
    best[0] = bv;
    best[1] = pr.tau[bi];
  }
}

}  // namespace
}  // namespace bnn
