// K6 training of MLP / MLP_Dropout: bnn_dense_loss (loss value + logits gradient), bnn_dense_bwd (one Linear ->
// [ReLU] -> [Dropout] group's weight, bias and input gradients in one launch) and bnn_sgd_step.  The forward is K5's
// bnn_dense_fwd (mlp_dropout.hip) with one sample and fp32 outputs.
//
// bnn_dense_bwd.  Two GEMMs share one grid: blocks [0, tiles_x) own 64 x 64 tiles of g_x = gz . W (K = out), the rest
// 64 x 64 tiles of g_w = gz^T . x (K = batch).  The g_x tiles come first: at the MNIST shape they have ~10 x the k
// stages of a weight-gradient tile, so they start in the first dispatch wave.  The GEMM core, the tile epilogue and the
// column sum are dense_tile.h's, shared with the Laplace curvature; the stage image is K5's.  What differs from K5 is
// the operands' memory order: gz^T, x and W are read along their contiguous (row) dimension -- a thread loads 8
// consecutive rows of one k and writes them into the [row][k] image element by element -- and gz is formed on load
// from gy (and the layer's saved output y: gz = y > 0 ? gy * y_scale : 0), so no masked copy is materialised.
// g_b = colsum(gz) rides on the weight-gradient blocks of tile column 0.  No float atomics, no K-split: every element is
// one fixed chain, whatever the grid.
#include <math.h>

#include "bnn_device.h"
#include "bnn_nll_row.h"
#include "bnn_stream.h"
#include "dense_tile.h"
#include "../../include/bnn_hip.h"

namespace bnn {
namespace {

struct BwdParams {
  const float* x;
  const float* gy;
  const float* y;
  const float* w;
  float* gw;
  float* gb;
  float* gx;
  int B, IN, OUT;
  float y_scale, gx_scale;
  int gx_mask;
  int tiles_x, tiles_x_n, tiles_w_n;
  int vec_x, vec_g, vec_w, vec_out;
};

template <typename TX>
__global__ __launch_bounds__(kThreads) void dense_bwd_kernel(BwdParams p) {
  __shared__ uint4 lds[kLdsUint4];
  f32x4 acc[2][2];
  int item = blockIdx.x;
  if (item < p.tiles_x) {
    // g_x [B, IN] = gz [B, OUT] . W [OUT, IN]: A(b, o) = gz, k (= o) contiguous; B(i, o) = W[o, i], i contiguous
    const int tm = item / p.tiles_x_n, tn = item - tm * p.tiles_x_n;
    const Opnd A{p.gy, p.y, p.y_scale, p.OUT, p.B, p.vec_g};
    const Opnd Bo{p.w, nullptr, 1.f, p.IN, p.IN, p.vec_w};
    gemm_tile<TX, true, false>(A, Bo, tm * kT, tn * kT, p.OUT, lds, acc);
    // times (x > 0 ? gx_scale : 0) when masked
    tile_epilogue(lds, acc, tm * kT, tn * kT, p.B, p.IN, [&](int row, int col0, int ncol, float o[4]) {
      const long at = (long)row * p.IN + col0;
      if (p.gx_mask) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (c < ncol) o[c] = p.x[at + c] > 0.f ? o[c] * p.gx_scale : 0.f;
      }
      store_group(p.gx + at, o, ncol, p.vec_out);
    });
    return;
  }
  item -= p.tiles_x;
  // g_w [OUT, IN] = gz^T . x: A(o, b) = gz[b, o], o contiguous; B(i, b) = x[b, i], i contiguous; K = B
  const int tm = item / p.tiles_w_n, tn = item - tm * p.tiles_w_n;
  const int m0 = tm * kT;
  const Opnd A{p.gy, p.y, p.y_scale, p.OUT, p.OUT, p.vec_g};
  const Opnd Bo{p.x, nullptr, 1.f, p.IN, p.IN, p.vec_x};
  gemm_tile<float, false, false>(A, Bo, m0, tn * kT, p.B, lds, acc);
  tile_epilogue(lds, acc, m0, tn * kT, p.OUT, p.IN, [&](int row, int col0, int ncol, float o[4]) {
    store_group(p.gw + (long)row * p.IN + col0, o, ncol, p.vec_out);
  });
  // g_b[o] = sum_b gz[b, o] for the tile's 64 rows
  if (tn == 0 && p.gb)
    col_sum4<4>(lds, m0, p.OUT, p.B, nullptr, p.gb, [&](int b, int o) { return gz_of(p.gy[(long)b * p.OUT + o], p.y, (long)b * p.OUT + o, p.y_scale); });
}

// one block; thread t owns rows t, t + 256, ...; the per-thread sums then meet in a fixed-order tree
__global__ __launch_bounds__(kThreads) void dense_loss_kernel(const float* __restrict__ z, const void* __restrict__ target, int B,
                                                              int C, int mode, float gs, float* __restrict__ loss,
                                                              float* __restrict__ g) {
  __shared__ float part[kThreads];
  const float total = tree_sum<kThreads>(dense_loss_rows<kThreads>(z, target, B, C, mode, gs, g), part);
  if (threadIdx.x == 0) *loss = total;
}

struct SgdK {
  float* p[BNN_SGD_MAX_TENSORS];
  const float* g[BNN_SGD_MAX_TENSORS];
  ChunkList<BNN_SGD_MAX_TENSORS> list;
  float lr, wd;
  const float* lr_dev;
};

// one block = one chunk of one tensor (bnn_stream.h)
__global__ __launch_bounds__(kThreads) void sgd_kernel(const SgdK k) {
  static_assert(kThreads == 256, "bnn_stream.h's walk");
  long base;
  const int t = k.list.find((int)blockIdx.x, kStreamChunk, base);
  const long n = k.list.numel[t];
  float* __restrict__ p = k.p[t];
  const float* __restrict__ g = k.g[t];
  const float nlr = -(k.lr_dev ? *k.lr_dev : k.lr);
  const float wd = k.wd;
#pragma unroll
  for (int it = 0; it < kStreamIters; ++it) {
    const long i = base + ((long)it * kThreads + threadIdx.x) * 4;
    if (i >= n) break;
    const bool full = i + 3 < n;
    float pv[4], gv[4];
    ld4(p, i, n, full, pv);
    ld4(g, i, n, full, gv);
#pragma unroll
    for (int j = 0; j < 4; ++j) pv[j] = __builtin_fmaf(nlr, wd != 0.f ? __builtin_fmaf(wd, pv[j], gv[j]) : gv[j], pv[j]);
    st4(p, i, n, full, pv);
  }
}

}  // namespace
}  // namespace bnn

using namespace bnn;

extern "C" int bnn_dense_loss(const bnn_dense_loss_args* a, void* stream_) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_dense_loss_args)) return BNN_ERR_ABI;
  if (a->batch <= 0 || a->classes <= 0) return BNN_ERR_SHAPE;
  if ((long)a->batch * a->classes > ((long)1 << 31)) return BNN_ERR_SHAPE;
  if (a->loss_mode != BNN_NLL_CLASSIFICATION && a->loss_mode != BNN_NLL_REGRESSION) return BNN_ERR_ENUM;
  if (!a->logits || !a->target || !a->loss || !a->g_logits) return BNN_ERR_NULL;
  if (misaligned(a->logits, 4) || misaligned(a->loss, 4) || misaligned(a->g_logits, 4) ||
      misaligned(a->target, a->loss_mode == BNN_NLL_CLASSIFICATION ? 8 : 4))
    return BNN_ERR_ALIGN;
  hipLaunchKernelGGL(dense_loss_kernel, dim3(1), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream_), a->logits, a->target,
                     a->batch, a->classes, a->loss_mode, a->grad_scale, a->loss, a->g_logits);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}

extern "C" int bnn_dense_bwd(const bnn_dense_bwd_args* a, void* stream_) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_dense_bwd_args)) return BNN_ERR_ABI;
  if (a->batch <= 0 || a->in_features <= 0 || a->out_features <= 0) return BNN_ERR_SHAPE;
  if ((long)a->batch * a->in_features > ((long)1 << 31) || (long)a->batch * a->out_features > ((long)1 << 31) ||
      (long)a->in_features * a->out_features > ((long)1 << 31))
    return BNN_ERR_SHAPE;
  if (a->math != BNN_MATH_F32 && a->math != BNN_MATH_BF16 && a->math != BNN_MATH_BF16X3) return BNN_ERR_ENUM;
  if (!a->x || !a->gy || !a->w || !a->g_w) return BNN_ERR_NULL;
  if (misaligned(a->x, 4) || misaligned(a->gy, 4) || misaligned(a->y, 4) || misaligned(a->w, 4) || misaligned(a->g_w, 4) ||
      misaligned(a->g_b, 4) || misaligned(a->g_x, 4))
    return BNN_ERR_ALIGN;
  BwdParams p;
  p.x = a->x; p.gy = a->gy; p.y = a->y; p.w = a->w;
  p.gw = a->g_w; p.gb = a->g_b; p.gx = a->g_x;
  p.B = a->batch; p.IN = a->in_features; p.OUT = a->out_features;
  p.y_scale = a->y_scale; p.gx_scale = a->gx_scale; p.gx_mask = a->gx_mask ? 1 : 0;
  const int tin = (p.IN + kT - 1) / kT, tout = (p.OUT + kT - 1) / kT, tb = (p.B + kT - 1) / kT;
  p.tiles_x_n = tin;
  p.tiles_x = a->g_x ? tb * tin : 0;
  p.tiles_w_n = tin;
  const long blocks = (long)p.tiles_x + (long)tout * tin;
  if (blocks > INT32_MAX) return BNN_ERR_SHAPE;
  // 16-byte loads / stores: rows of a multiple of 4 floats from 16-byte aligned bases
  p.vec_x = p.IN % 4 == 0 && !misaligned(a->x, 16);
  p.vec_w = p.IN % 4 == 0 && !misaligned(a->w, 16);
  p.vec_g = p.OUT % 4 == 0 && !misaligned(a->gy, 16) && !misaligned(a->y, 16);
  p.vec_out = p.IN % 4 == 0 && !misaligned(a->g_w, 16) && !misaligned(a->g_x, 16);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream_);
  if (a->math == BNN_MATH_BF16)
    hipLaunchKernelGGL(dense_bwd_kernel<__bf16>, dim3((unsigned)blocks), dim3(kThreads), 0, st, p);
  else
    hipLaunchKernelGGL(dense_bwd_kernel<float>, dim3((unsigned)blocks), dim3(kThreads), 0, st, p);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}

extern "C" int bnn_sgd_step(const bnn_sgd_args* a, void* stream_) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_sgd_args)) return BNN_ERR_ABI;
  if (a->n_tensors <= 0 || a->n_tensors > BNN_SGD_MAX_TENSORS) return BNN_ERR_SHAPE;
  if (!(a->lr >= 0.0) || !(a->weight_decay >= 0.0)) return BNN_ERR_SHAPE;
  SgdK k;
  for (int t = 0; t < BNN_SGD_MAX_TENSORS; ++t) {
    k.p[t] = nullptr; k.g[t] = nullptr;
  }
  for (int t = 0; t < a->n_tensors; ++t) {
    if (!a->param[t] || !a->grad[t]) return BNN_ERR_NULL;
    const int st = k.list.add(a->numel[t], kStreamChunk);
    if (st != BNN_OK) return st;
    if (misaligned(a->param[t], 16) || misaligned(a->grad[t], 16)) return BNN_ERR_ALIGN;
    k.p[t] = a->param[t];
    k.g[t] = a->grad[t];
  }
  if (misaligned(a->lr_device, 4)) return BNN_ERR_ALIGN;
  const int chunks = k.list.finish();
  k.lr = (float)a->lr;
  k.wd = (float)a->weight_decay;
  k.lr_dev = a->lr_device;
  hipLaunchKernelGGL(sgd_kernel, dim3((unsigned)chunks), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream_), k);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}
