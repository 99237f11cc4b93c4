// F21  training a deep ensemble: one K6 training step of all M members of an F19 weight bank in a fixed chain of launches,
// whatever M -- bnn_ens_fwd per layer (K5's product, bias, ReLU and kind-3 dropout mask per member), bnn_ens_loss (one block
// per member), bnn_ens_bwd per layer (K6's two GEMMs and column sum per member).  The optimiser is the existing bnn_sgd_step /
// bnn_adam_step over the bank buffer and the gradient bucket as flat tensors.
//
// All three sit on dense_tile.h's 64 x 64 core and add nothing to an element's chain: a block owns one tile of ONE member and
// runs exactly what bnn_dense_fwd / bnn_dense_loss / bnn_dense_bwd run on that member's operands, so every member's outputs
// are bit-equal to the single-network kernels'.  What is new is the work list: (member, tile), member-major, dealt to the XCDs
// in contiguous ranges (xcd_work_item), so that the tiles that share a member's weights and activations run on one XCD and
// meet in its L2.  In the backward a member's g_x items (K = out: the long ones) come ahead of its g_w items (K = batch), as
// in the single-network kernel.  The order affects speed only.  No float atomics, no K-split.
#include <math.h>

#include "bnn_device.h"
#include "bnn_nll_row.h"
#include "dense_tile.h"
#include "../../include/bnn_hip.h"

namespace bnn {
namespace {

// ------------------------------------------------------------------------------------------------------ the forward
struct EnsFwdK {
  const float* x;
  const float* w;
  const float* b;
  float* y;
  long w_stride, b_stride;
  int M, first, B, N, K, tiles_m, tiles_n, total;
  int x_shared, relu, drop, vec_x, vec_w, vec_y;
  uint32_t thr, k0, k1, tensor_id, sample_base, inc;
  float scale;
  uint32_t* counter;
};

// T: the staged type (the math); activations fp32 in memory (the backward reads them)
template <typename T>
__global__ __launch_bounds__(kThreads) void ens_fwd_kernel(const EnsFwdK k) {
  __shared__ uint4 lds[tile_lds_uint4<T, 2, 2>()];
  if (k.inc && blockIdx.x == 0 && threadIdx.x == 0) *k.counter += k.inc;   // no block of this launch reads the counter
  int item;
  if (!xcd_work_item(k.total, item)) return;
  // (member, column tile, row tile), the row tile fastest: an XCD's consecutive items share the member's weight tile
  const int tm = item % k.tiles_m, rest = item / k.tiles_m;
  const int tn = rest % k.tiles_n, j = rest / k.tiles_n;
  const int m0 = tm * kT, n0 = tn * kT;
  const float* __restrict__ w = k.w + (long)(k.first + j) * k.w_stride;
  const float* __restrict__ b = k.b ? k.b + (long)(k.first + j) * k.b_stride : nullptr;
  float* __restrict__ y = k.y + (long)j * k.B * k.N;
  const Opnd A{k.x + (k.x_shared ? 0 : (long)j * k.B * k.K), nullptr, 1.f, k.K, k.B, k.vec_x};
  const Opnd Bo{w, nullptr, 1.f, k.K, k.N, k.vec_w};
  f32x4 acc[2][2];
  gemm_tile<T, true, true>(A, Bo, m0, n0, k.K, lds, acc);
  // K5's epilogue: + b, ReLU, the mask of member j's global sample index (one Philox call per group of 4), store
  const uint32_t gpr = (uint32_t)(k.N + 3) >> 2;
  const uint32_t sample = k.sample_base + ((k.drop && k.counter) ? *k.counter : 0u) + (uint32_t)j;
  tile_epilogue(lds, acc, m0, n0, k.B, k.N, [&](int row, int col0, int ncol, float o[4]) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      o[c] += (b && c < ncol) ? b[col0 + c] : 0.f;
      if (k.relu) o[c] = fmaxf(o[c], 0.f);
    }
    if (k.drop) {
      const uint4 rr = philox4x32<>(make_uint4(eps_group((uint32_t)row, (uint32_t)col0, gpr), sample, k.tensor_id, 0u), k.k0, k.k1);
      o[0] = rr.x >= k.thr ? o[0] * k.scale : 0.f;
      o[1] = rr.y >= k.thr ? o[1] * k.scale : 0.f;
      o[2] = rr.z >= k.thr ? o[2] * k.scale : 0.f;
      o[3] = rr.w >= k.thr ? o[3] * k.scale : 0.f;
    }
    store_group(y + (long)row * k.N + col0, o, ncol, k.vec_y);
  });
}

// ------------------------------------------------------------------------------------------------------ the loss
// one block per member: bnn_dense_loss's row loop and fixed-order tree on the member's logits
__global__ __launch_bounds__(kThreads) void ens_loss_kernel(const float* __restrict__ z, const void* __restrict__ target,
                                                            long target_stride_bytes, int B, int C, int mode, float gs,
                                                            float* __restrict__ loss, float* __restrict__ g) {
  __shared__ float part[kThreads];
  const int j = blockIdx.x;
  const long at = (long)j * B * C;
  const void* tg = reinterpret_cast<const char*>(target) + (long)j * target_stride_bytes;
  const float total = tree_sum<kThreads>(dense_loss_rows<kThreads>(z + at, tg, B, C, mode, gs, g + at), part);
  if (threadIdx.x == 0) loss[j] = total;
}

// ------------------------------------------------------------------------------------------------------ the backward
struct EnsBwdK {
  const float* x;
  const float* gy;
  const float* y;
  const float* w;
  float* gw;
  float* gb;
  float* gx;
  long w_stride, g_stride;
  int M, first, B, IN, OUT;
  float y_scale, gx_scale;
  int x_shared, gx_mask;
  int tiles_x, tiles_n, per_member, total;      // g_x tiles of a member, tiles across IN, items of a member, all items
  int vec_x, vec_g, vec_w, vec_out;
};

// dense_bwd_kernel (dense_train.hip) on member j = item / per_member: the member's g_x tiles first, then its g_w tiles
template <typename TX>
__global__ __launch_bounds__(kThreads) void ens_bwd_kernel(const EnsBwdK p) {
  __shared__ uint4 lds[kLdsUint4];
  int item;
  if (!xcd_work_item(p.total, item)) return;
  const int j = item / p.per_member;
  item -= j * p.per_member;
  const long act_in = (long)j * p.B * p.IN, act_out = (long)j * p.B * p.OUT;
  const float* __restrict__ x = p.x + (p.x_shared ? 0 : act_in);
  const float* __restrict__ gy = p.gy + act_out;
  const float* __restrict__ y = p.y ? p.y + act_out : nullptr;
  const float* __restrict__ w = p.w + (long)(p.first + j) * p.w_stride;
  f32x4 acc[2][2];
  if (item < p.tiles_x) {
    // g_x [B, IN] = gz [B, OUT] . W [OUT, IN]: A(b, o) = gz, k (= o) contiguous; B(i, o) = W[o, i], i contiguous
    const int tm = item / p.tiles_n, tn = item - tm * p.tiles_n;
    float* __restrict__ gx = p.gx + act_in;
    const Opnd A{gy, y, p.y_scale, p.OUT, p.B, p.vec_g};
    const Opnd Bo{w, nullptr, 1.f, p.IN, p.IN, p.vec_w};
    gemm_tile<TX, true, false>(A, Bo, tm * kT, tn * kT, p.OUT, lds, acc);
    // times (x > 0 ? gx_scale : 0) when masked
    tile_epilogue(lds, acc, tm * kT, tn * kT, p.B, p.IN, [&](int row, int col0, int ncol, float o[4]) {
      const long at = (long)row * p.IN + col0;
      if (p.gx_mask) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (c < ncol) o[c] = x[at + c] > 0.f ? o[c] * p.gx_scale : 0.f;
      }
      store_group(gx + at, o, ncol, p.vec_out);
    });
    return;
  }
  item -= p.tiles_x;
  // g_w [OUT, IN] = gz^T . x: A(o, b) = gz[b, o], o contiguous; B(i, b) = x[b, i], i contiguous; K = B
  const int tm = item / p.tiles_n, tn = item - tm * p.tiles_n;
  const int m0 = tm * kT;
  float* __restrict__ gw = p.gw + (long)j * p.g_stride;
  const Opnd A{gy, y, p.y_scale, p.OUT, p.OUT, p.vec_g};
  const Opnd Bo{x, nullptr, 1.f, p.IN, p.IN, p.vec_x};
  gemm_tile<float, false, false>(A, Bo, m0, tn * kT, p.B, lds, acc);
  tile_epilogue(lds, acc, m0, tn * kT, p.OUT, p.IN, [&](int row, int col0, int ncol, float o[4]) {
    store_group(gw + (long)row * p.IN + col0, o, ncol, p.vec_out);
  });
  // g_b[o] = sum_b gz[b, o] for the tile's 64 rows
  if (tn == 0 && p.gb)
    col_sum4<4>(lds, m0, p.OUT, p.B, nullptr, p.gb + (long)j * p.g_stride,
                [&](int b, int o) { return gz_of(gy[(long)b * p.OUT + o], y, (long)b * p.OUT + o, p.y_scale); });
}

bool math_ok(int m) { return m == BNN_MATH_F32 || m == BNN_MATH_BF16 || m == BNN_MATH_BF16X3; }
unsigned xcd_grid(int total) { return 8u * (unsigned)((total + 7) / 8); }      // (xcd_work_item: 8 equal ranges)

constexpr long kMaxItems = 0x3fffffff;
constexpr long k2p31 = (long)1 << 31;

}  // namespace
}  // namespace bnn

using namespace bnn;

extern "C" int bnn_ens_fwd(const bnn_ens_fwd_args* a, void* stream_) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_ens_fwd_args)) return BNN_ERR_ABI;
  if (a->members <= 0 || a->first < 0 || a->batch <= 0 || a->in_features <= 0 || a->out_features <= 0 || a->layer_id < 0 ||
      a->w_stride < 0 || a->b_stride < 0 || a->batch > INT32_MAX / 2 || (long)a->first + a->members > INT32_MAX)
    return BNN_ERR_SHAPE;
  EnsFwdK k;
  if (!drop_params(a->drop_p, k.thr, k.scale)) return BNN_ERR_SHAPE;
  if (a->sample_counter_inc && a->drop_p != 0.0) return BNN_ERR_SHAPE;
  const long tiles_m = ((long)a->batch + kT - 1) / kT, tiles_n = ((long)a->out_features + kT - 1) / kT;
  const long total = tiles_m * tiles_n * a->members;
  if (total > kMaxItems || (long)a->members * a->batch * a->out_features > ((long)1 << 40) ||
      (long)a->members * a->batch * a->in_features > ((long)1 << 40))
    return BNN_ERR_SHAPE;
  if (!math_ok(a->math)) return BNN_ERR_ENUM;
  if (!a->x || !a->w || !a->y) return BNN_ERR_NULL;
  if (a->sample_counter_inc && !a->sample_counter) return BNN_ERR_NULL;
  if (misaligned(a->x, 4) || misaligned(a->w, 4) || misaligned(a->b, 4) || misaligned(a->y, 4) || misaligned(a->sample_counter, 4))
    return BNN_ERR_ALIGN;
  k.x = a->x; k.w = a->w; k.b = a->b; k.y = a->y;
  k.w_stride = a->w_stride; k.b_stride = a->b_stride;
  k.M = a->members; k.first = a->first; k.B = a->batch; k.N = a->out_features; k.K = a->in_features;
  k.tiles_m = (int)tiles_m; k.tiles_n = (int)tiles_n; k.total = (int)total;
  k.x_shared = a->x_shared ? 1 : 0; k.relu = a->relu ? 1 : 0; k.drop = a->drop_p != 0.0;
  // 16-byte accesses: rows of a multiple of 4 floats from 16-byte aligned bases, in every member
  k.vec_x = a->in_features % 4 == 0 && !misaligned(a->x, 16);
  k.vec_w = a->in_features % 4 == 0 && a->w_stride % 4 == 0 && !misaligned(a->w, 16);
  k.vec_y = a->out_features % 4 == 0 && !misaligned(a->y, 16);
  k.k0 = (uint32_t)a->seed; k.k1 = (uint32_t)(a->seed >> 32);
  k.tensor_id = eps_tensor_id((uint32_t)a->layer_id, kEpsDropout);
  k.sample_base = a->sample_offset; k.inc = a->sample_counter_inc; k.counter = a->sample_counter;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream_);
  if (a->math == BNN_MATH_BF16) hipLaunchKernelGGL(ens_fwd_kernel<__bf16>, dim3(xcd_grid(k.total)), dim3(kThreads), 0, st, k);
  else hipLaunchKernelGGL(ens_fwd_kernel<float>, dim3(xcd_grid(k.total)), dim3(kThreads), 0, st, k);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}

extern "C" int bnn_ens_loss(const bnn_ens_loss_args* a, void* stream_) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_ens_loss_args)) return BNN_ERR_ABI;
  if (a->members <= 0 || a->batch <= 0 || a->classes <= 0) return BNN_ERR_SHAPE;
  if ((long)a->batch * a->classes > k2p31) return BNN_ERR_SHAPE;
  if (a->loss_mode != BNN_NLL_CLASSIFICATION && a->loss_mode != BNN_NLL_REGRESSION) return BNN_ERR_ENUM;
  if (!a->logits || !a->target || !a->loss || !a->g_logits) return BNN_ERR_NULL;
  const bool cls = a->loss_mode == BNN_NLL_CLASSIFICATION;
  if (misaligned(a->logits, 4) || misaligned(a->loss, 4) || misaligned(a->g_logits, 4) || misaligned(a->target, cls ? 8 : 4))
    return BNN_ERR_ALIGN;
  const long tstride = a->target_shared ? 0 : (cls ? 8L * a->batch : 4L * a->batch * a->classes);
  hipLaunchKernelGGL(ens_loss_kernel, dim3((unsigned)a->members), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream_),
                     a->logits, a->target, tstride, a->batch, a->classes, a->loss_mode, a->grad_scale, a->loss, a->g_logits);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}

extern "C" int bnn_ens_bwd(const bnn_ens_bwd_args* a, void* stream_) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_ens_bwd_args)) return BNN_ERR_ABI;
  if (a->members <= 0 || a->first < 0 || a->batch <= 0 || a->in_features <= 0 || a->out_features <= 0 || a->w_stride < 0 ||
      a->g_stride < 0 || (long)a->first + a->members > INT32_MAX)
    return BNN_ERR_SHAPE;
  if ((long)a->batch * a->in_features > k2p31 || (long)a->batch * a->out_features > k2p31 ||
      (long)a->in_features * a->out_features > k2p31)
    return BNN_ERR_SHAPE;
  const long tin = ((long)a->in_features + kT - 1) / kT, tout = ((long)a->out_features + kT - 1) / kT, tb = ((long)a->batch + kT - 1) / kT;
  const long tiles_x = a->g_x ? tb * tin : 0;
  const long per_member = tiles_x + tout * tin;
  if (per_member > kMaxItems || per_member * a->members > kMaxItems) return BNN_ERR_SHAPE;
  if (!math_ok(a->math)) return BNN_ERR_ENUM;
  if (!a->x || !a->gy || !a->w || !a->g_w) return BNN_ERR_NULL;
  if (misaligned(a->x, 4) || misaligned(a->gy, 4) || misaligned(a->y, 4) || misaligned(a->w, 4) || misaligned(a->g_w, 4) ||
      misaligned(a->g_b, 4) || misaligned(a->g_x, 4))
    return BNN_ERR_ALIGN;
  EnsBwdK p;
  p.x = a->x; p.gy = a->gy; p.y = a->y; p.w = a->w;
  p.gw = a->g_w; p.gb = a->g_b; p.gx = a->g_x;
  p.w_stride = a->w_stride; p.g_stride = a->g_stride;
  p.M = a->members; p.first = a->first; p.B = a->batch; p.IN = a->in_features; p.OUT = a->out_features;
  p.y_scale = a->y_scale; p.gx_scale = a->gx_scale;
  p.x_shared = a->x_shared ? 1 : 0; p.gx_mask = a->gx_mask ? 1 : 0;
  p.tiles_x = (int)tiles_x; p.tiles_n = (int)tin; p.per_member = (int)per_member; p.total = (int)(per_member * a->members);
  // 16-byte loads / stores: rows of a multiple of 4 floats from 16-byte aligned bases, in every member
  p.vec_x = p.IN % 4 == 0 && !misaligned(a->x, 16);
  p.vec_w = p.IN % 4 == 0 && a->w_stride % 4 == 0 && !misaligned(a->w, 16);
  p.vec_g = p.OUT % 4 == 0 && !misaligned(a->gy, 16) && !misaligned(a->y, 16);
  p.vec_out = p.IN % 4 == 0 && a->g_stride % 4 == 0 && !misaligned(a->g_w, 16) && !misaligned(a->g_x, 16);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream_);
  if (a->math == BNN_MATH_BF16) hipLaunchKernelGGL(ens_bwd_kernel<__bf16>, dim3(xcd_grid(p.total)), dim3(kThreads), 0, st, p);
  else hipLaunchKernelGGL(ens_bwd_kernel<float>, dim3(xcd_grid(p.total)), dim3(kThreads), 0, st, p);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}
