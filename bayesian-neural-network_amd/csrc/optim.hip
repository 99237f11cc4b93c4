// F2  fused Adam over all parameter tensors of the network in one launch (the update the
// reference's trainers run after loss.backward(): torch.optim.Adam, class_task.py:60/:79,
// reg_task.py:53) and the NLL backward that seeds the layer backward kernels.
//
// Adam is pure streaming: 16 B read + 12 B written per parameter (p, g, m, v -> p, m, v), no
// reuse: HBM-bound, 28 B/param.  One block = one 4096-element chunk of one tensor; the
// chunk -> tensor table rides in the kernel arguments; 16-byte accesses.
#include "bnn_device.h"
#include "bnn_nll_row.h"
#include "bnn_stream.h"
#include "../../include/bnn_hip.h"
#include <math.h>
#include <type_traits>

namespace bnn {

struct AdamK {
  float* p[BNN_ADAM_MAX_TENSORS];
  const float* g[BNN_ADAM_MAX_TENSORS];
  float* m[BNN_ADAM_MAX_TENSORS];
  float* v[BNN_ADAM_MAX_TENSORS];
  ChunkList<BNN_ADAM_MAX_TENSORS> list;
  double lr, beta1, beta2;
  float beta2f, omb1, omb2, eps, wd;
  uint32_t step;
  const float* lr_dev;
  uint32_t* step_dev;         // already advanced by adam_tick_kernel when set and ticket == nullptr
  uint32_t* ticket;           // set: this launch advances *step_dev itself (last arriver), no tick launch
  uint32_t* bump;             // optional word the last arriver adds bump_by to (the step's MC-sample counter)
  uint32_t bump_by;
};

__global__ void adam_tick_kernel(uint32_t* step) { *step += 1u; }

// GBF16: the gradients arrive in bf16 (a data-parallel step's all-reduced 2-byte bucket)
template <bool GBF16>
__global__ __launch_bounds__(256) void adam_kernel(const AdamK k) {
  using G = typename std::conditional<GBF16, __bf16, float>::type;
  long base;
  const int t = k.list.find((int)blockIdx.x, kStreamChunk, base);
  const long n = k.list.numel[t];
  float* __restrict__ p = k.p[t];
  const G* __restrict__ g = reinterpret_cast<const G*>(k.g[t]);
  float* __restrict__ m = k.m[t];
  float* __restrict__ v = k.v[t];
  // a whole chunk (all but the last block of a tensor): its 16 loads go out before anything else -- the double-precision
  // bias corrections below are a few hundred instructions per thread, and behind them the first load round trip of every
  // wave was exposed at the head of the launch
  const bool whole = base + kStreamChunk <= n;
  float pw[kStreamIters][4], gw[kStreamIters][4], mw[kStreamIters][4], vw[kStreamIters][4];
  if (whole) {
#pragma unroll
    for (int it = 0; it < kStreamIters; ++it) {
      const long i = base + ((long)it * 256 + threadIdx.x) * 4;
      ld4(p, i, n, true, pw[it]);
      ld4(g, i, n, true, gw[it]);
      ld4(m, i, n, true, mw[it]);
      ld4(v, i, n, true, vw[it]);
    }
  }
  const double lr = k.lr_dev ? (double)*k.lr_dev : k.lr;
  // with a ticket word every block reads the old step and uses step + 1; the launch's last block stores it (last_block)
  const uint32_t step = k.step_dev ? *k.step_dev + (k.ticket ? 1u : 0u) : k.step;
  // bias corrections in double, as torch computes them on the host (1 - beta ** step)
  const double bc1 = 1.0 - pow(k.beta1, (double)step);
  const double bc2 = 1.0 - pow(k.beta2, (double)step);
  const float step_size = (float)(lr / bc1);
  const float sqrt_bc2 = (float)sqrt(bc2);
  const float omb1 = k.omb1, omb2 = k.omb2;
  // the arithmetic and the stores of one float4 whose operands are loaded; `full`: all four elements exist
  auto finish = [&](const long i, const bool full, float pv[4], const float gv[4], float mv[4], float vv[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float gg = k.wd != 0.f ? __builtin_fmaf(k.wd, pv[j], gv[j]) : gv[j];
      mv[j] = __builtin_fmaf(gg - mv[j], omb1, mv[j]);           // exp_avg.lerp_(grad, 1 - beta1); stated, like the next one
      // exp_avg_sq.mul_(beta2).addcmul_(g, g, 1 - beta2).  The fma is stated: left to -ffp-contract=fast the compiler forms
      // fma(v, beta2, (omb2 g) g) or fma(omb2 g, g, v beta2), and which one has flipped with unrelated code around it
      vv[j] = __builtin_fmaf(vv[j], k.beta2f, omb2 * gg * gg);
      const float denom = __builtin_sqrtf(vv[j]) / sqrt_bc2 + k.eps;
      pv[j] = pv[j] - step_size * (mv[j] / denom);
    }
    st4(p, i, n, full, pv);
    st4(m, i, n, full, mv);
    st4(v, i, n, full, vv);
  };
  if (whole) {
#pragma unroll
    for (int it = 0; it < kStreamIters; ++it)
      finish(base + ((long)it * 256 + threadIdx.x) * 4, true, pw[it], gw[it], mw[it], vw[it]);
  } else {
#pragma unroll
    for (int it = 0; it < kStreamIters; ++it) {
      const long i = base + ((long)it * 256 + threadIdx.x) * 4;
      if (i >= n) break;
      const bool full = i + 3 < n;
      float pv[4], gv[4], mv[4], vv[4];
      ld4(p, i, n, full, pv);
      ld4(g, i, n, full, gv);
      ld4(m, i, n, full, mv);
      ld4(v, i, n, full, vv);
      finish(i, full, pv, gv, mv, vv);
    }
  }
  if (k.ticket)
    last_block(k.ticket, [&] {
      *k.step_dev = step;
      if (k.bump) *k.bump += k.bump_by;
    });
}

// one thread per (sample, batch row)
__global__ void nll_bwd_kernel(const float* __restrict__ logits, const void* __restrict__ target,
                               const float* __restrict__ g_nll, float* __restrict__ g_logits, int S, int B, int C, int mode,
                               float inv_var) {
  const long total = (long)S * B;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const int b = (int)(idx % B), s = (int)(idx / B);
    nll_row_grad(logits + idx * C, C, mode, target, b, g_nll[s], inv_var, g_logits + idx * C);
  }
}

}  // namespace bnn

using namespace bnn;

extern "C" int bnn_adam_step(const bnn_adam_args* a, void* stream_) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_adam_args)) return BNN_ERR_ABI;
  if (a->n_tensors <= 0 || a->n_tensors > BNN_ADAM_MAX_TENSORS) return BNN_ERR_SHAPE;
  if (!a->step_device && a->step == 0) return BNN_ERR_SHAPE;
  if (!(a->beta1 >= 0.0 && a->beta1 < 1.0) || !(a->beta2 >= 0.0 && a->beta2 < 1.0) || !(a->eps >= 0.0)) return BNN_ERR_SHAPE;
  AdamK k;
  for (int t = 0; t < BNN_ADAM_MAX_TENSORS; ++t) {
    k.p[t] = nullptr; k.g[t] = nullptr; k.m[t] = nullptr; k.v[t] = nullptr;
  }
  for (int t = 0; t < a->n_tensors; ++t) {
    if (!a->param[t] || !a->grad[t] || !a->exp_avg[t] || !a->exp_avg_sq[t]) return BNN_ERR_NULL;
    const int st = k.list.add(a->numel[t], kStreamChunk);
    if (st != BNN_OK) return st;
    const uintptr_t al = reinterpret_cast<uintptr_t>(a->param[t]) | reinterpret_cast<uintptr_t>(a->grad[t]) |
                         reinterpret_cast<uintptr_t>(a->exp_avg[t]) | reinterpret_cast<uintptr_t>(a->exp_avg_sq[t]);
    if (al & 15) return BNN_ERR_ALIGN;
    k.p[t] = a->param[t]; k.g[t] = a->grad[t]; k.m[t] = a->exp_avg[t]; k.v[t] = a->exp_avg_sq[t];
  }
  const int chunks = k.list.finish();
  k.lr = a->lr; k.beta1 = a->beta1; k.beta2 = a->beta2; k.eps = (float)a->eps; k.wd = (float)a->weight_decay;
  k.beta2f = (float)a->beta2; k.omb1 = (float)(1.0 - a->beta1); k.omb2 = (float)(1.0 - a->beta2);
  k.step = a->step; k.lr_dev = a->lr_device; k.step_dev = a->step_device;
  const bool ticketed = a->step_device && a->step_advance && a->ticket;
  if (a->bump_counter && !ticketed) return BNN_ERR_NULL;   // the counter rides on the ticketed hand-off only
  k.ticket = ticketed ? a->ticket : nullptr;
  k.bump = a->bump_counter; k.bump_by = a->bump_by;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (a->step_device && a->step_advance && !ticketed)
    hipLaunchKernelGGL(adam_tick_kernel, dim3(1), dim3(1), 0, stream, a->step_device);
  if ((unsigned)a->grad_dtype > 1u) return BNN_ERR_ENUM;
  if (a->grad_dtype == BNN_BF16) hipLaunchKernelGGL(adam_kernel<true>, dim3((unsigned)chunks), dim3(256), 0, stream, k);
  else hipLaunchKernelGGL(adam_kernel<false>, dim3((unsigned)chunks), dim3(256), 0, stream, k);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}

extern "C" int bnn_nll_bwd(const float* logits, const void* target, const float* g_nll, float* g_logits, int32_t n_samples,
                           int32_t batch, int32_t classes, int32_t nll_mode, float nll_sigma, void* stream_) {
  if (!logits || !target || !g_nll || !g_logits) return BNN_ERR_NULL;
  if (n_samples <= 0 || batch <= 0 || classes <= 0) return BNN_ERR_SHAPE;
  if ((unsigned)nll_mode > 1u) return BNN_ERR_ENUM;
  if (nll_mode == BNN_NLL_REGRESSION && !(nll_sigma > 0.f)) return BNN_ERR_SHAPE;
  const long total = (long)n_samples * batch;
  long nb = (total + 127) / 128;
  nb = nb > 2048 ? 2048 : nb;
  const float inv_var = nll_mode == BNN_NLL_REGRESSION ? (float)(1.0 / ((double)nll_sigma * nll_sigma)) : 0.f;
  hipLaunchKernelGGL(nll_bwd_kernel, dim3((unsigned)nb), dim3(128), 0, reinterpret_cast<hipStream_t>(stream_), logits, target,
                     g_nll, g_logits, n_samples, batch, classes, nll_mode, inv_var);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}
