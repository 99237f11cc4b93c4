// The gradient of one row's NLL w.r.t. its logits, for every kernel that forms it: bnn_nll_bwd (optim.hip),
// bnn_elbo_loss_nll_bwd (reduce.hip), the loss tail of K1r / K3r (bnn_fin.h), bnn_dense_loss (dense_train.hip) and the
// empirical-Fisher seed of bnn_laplace_seed (laplace.hip).  One operation order, so the same bits from all of them.
#pragma once
#include "bnn_device.h"

namespace bnn {

// mx = max_c row[c] (from row[0]), se = sum_c exp(row[c] - mx) (from 0, in class order)
__device__ __forceinline__ void row_max_sumexp(const float* row, int C, float& mx, float& se) {
  mx = row[0];
  for (int c = 1; c < C; ++c) mx = fmaxf(mx, row[c]);
  se = 0.f;
  for (int c = 0; c < C; ++c) se += expf(row[c] - mx);
}

// out[c] = (softmax(row)[c] - [c == tc]) * gs.  A label outside [0, C) poisons the row's gradient (and the forward's NLL)
// with NaN instead of training silently on a wrong loss (nn.CrossEntropyLoss, networks.py:186, raises there; ignore_index
// is not supported); row[tc] is never read.
__device__ __forceinline__ void softmax_row_grad(const float* row, int C, long long tc, float mx, float se, float gs, float* out) {
  const float inv = (tc >= 0 && tc < C) ? 1.0f / se : __builtin_nanf("");
  for (int c = 0; c < C; ++c) out[c] = (expf(row[c] - mx) * inv - (c == tc ? 1.f : 0.f)) * gs;
}

// the Gaussian likelihood's: out[c] = (row[c] - tg[c]) / sigma^2 * gs
__device__ __forceinline__ void gauss_row_grad(const float* row, const float* tg, int C, float inv_var, float gs, float* out) {
  for (int c = 0; c < C; ++c) out[c] = (row[c] - tg[c]) * inv_var * gs;
}

// Batch row b of either mode: target is the int64 labels [B] (classification) or the fp32 targets [B, C] (regression).
__device__ __forceinline__ void nll_row_grad(const float* row, int C, int mode, const void* target, int b, float gs, float inv_var,
                                             float* out) {
  if (mode == BNN_NLL_CLASSIFICATION) {
    float mx, se;
    row_max_sumexp(row, C, mx, se);
    softmax_row_grad(row, C, reinterpret_cast<const long long*>(target)[b], mx, se, gs, out);
  } else {
    gauss_row_grad(row, reinterpret_cast<const float*>(target) + (size_t)b * C, C, inv_var, gs, out);
  }
}

// bnn_dense_loss's row loop (dense_train.hip; one block per member in bnn_ens_loss, ensemble.hip): thread t of THREADS owns rows
// t, t + THREADS, ... of z [B, C]; writes their gradient rows g (times gs) and returns the thread's partial of the SUM loss
// (cross_entropy / mse_loss, reduction='sum'), which the caller adds up in a fixed-order tree.
template <int THREADS>
__device__ __forceinline__ float dense_loss_rows(const float* __restrict__ z, const void* __restrict__ target, int B, int C, int mode,
                                                 float gs, float* __restrict__ g) {
  float acc = 0.f;
#pragma unroll 1
  for (int b = threadIdx.x; b < B; b += THREADS) {
    const float* row = z + (long)b * C;
    float* grow = g + (long)b * C;
    if (mode == BNN_NLL_CLASSIFICATION) {
      const long long tc = reinterpret_cast<const long long*>(target)[b];
      const bool ok = tc >= 0 && tc < C;
      float mx, se;
      row_max_sumexp(row, C, mx, se);
      // an out-of-range label: NaN loss and row gradient, and z[label] is never read
      acc += ok ? (mx + logf(se)) - row[ok ? tc : 0] : __builtin_nanf("");
      softmax_row_grad(row, C, tc, mx, se, gs, grow);
    } else {
      const float* tg = reinterpret_cast<const float*>(target) + (long)b * C;
      for (int c = 0; c < C; ++c) {
        const float d = row[c] - tg[c];
        acc = __builtin_fmaf(d, d, acc);
        grow[c] = 2.f * d * gs;
      }
    }
  }
  return acc;
}

}  // namespace bnn
