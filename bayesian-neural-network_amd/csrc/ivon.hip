// F24  IVON for MLP (Shen et al. 2024): natural-gradient variational learning of a diagonal Gaussian N(m, 1 / (ess (h + delta)))
// per weight.  A training step is, per MC sample, one draw launch in front of the forward pass (bnn_ivon_draw: theta = m + sigma
// eps into the parameter tensors; at sample 0 the mean is filed into the state, at sample >= 1 the previous sample's gradient is
// folded into two accumulators) and, behind the last backward pass, one step launch (bnn_ivon_step: gradient momentum, the
// Hessian estimate with its positivity correction, the Newton-like update of the mean).  The same draw launch in its bank form
// writes up to 64 members of a weight bank, a thread holding its float4 of m and sigma in registers.
//
// All three kernels are pure streaming like bnn_swag_step: one block = one 4096-element chunk of one tensor, 16-byte accesses
// with scalar tails, no float atomics.  Per parameter at S = 1 the draw reads p, h and writes mean, p (16 B); the step reads g,
// mean, h, gm and writes p, h, gm (28 B, bnn_adam_step's).  Per float4 the draw runs one Philox call, 4 sqrt and 4 divisions;
// the step regenerates the same Philox call (theta - m is never formed) and runs 4 sqrt and 8 divisions.  The step word and the
// fp64 product beta1^t are advanced by the step launch's last block (bnn_stream.h's ticketed hand-off).
// The step kernel issues a whole chunk's loads ahead of its arithmetic (as bnn_adam_step's unrolled loop does); the draw and
// the bank kernel make one load / compute / store round per iteration.
//
// Every multiply-add below is written out (the build contracts what is left to it): a product that feeds an add is either an
// explicit fma or does not exist.
#include "bnn_device.h"
#include "bnn_stream.h"
#include "../../include/bnn_hip.h"

namespace bnn {
namespace {

constexpr uint32_t kIvWord3 = 6u;       // counter word 3 of the IVON noise stream (include/bnn_hip.h F24)
constexpr int kMaxT = BNN_SGMCMC_MAX_TENSORS;

// the noise of draw q (on chip) or of row `row` of the noise in memory; 0 in BNN_EPS_ZERO
__device__ __forceinline__ void ivon_noise(int eps_mode, const float* __restrict__ rows, long stride, long row, long i, long n,
                                           bool full, uint32_t q, uint32_t t, uint32_t k0, uint32_t k1, float e[4]) {
  if (eps_mode == BNN_EPS_PHILOX) {
    philox_normal4((uint32_t)(i >> 2), q, t, k0, k1, e, kIvWord3);
  } else if (eps_mode == BNN_EPS_MEMORY) {
    ld4(rows + row * stride, i, n, full, e);
  } else {
    e[0] = e[1] = e[2] = e[3] = 0.f;
  }
}

// r = sqrt(ess (h + delta)) and sigma = 1 / r: the one form the draw, the fold and the step share
__device__ __forceinline__ void ivon_scale(float h, float ess, float delta, float& hd, float& r, float& sigma) {
  hd = h + delta;
  r = __builtin_sqrtf(ess * hd);
  sigma = 1.0f / r;
}

struct IvDrawK {
  float* p[kMaxT];
  const float* g[kMaxT];
  long off[kMaxT];
  ChunkList<kMaxT> list;
  float ess, delta;
  uint32_t S, s, m, mgroup, first, sample_base, k0, k1;
  int eps_mode;
  long stride;
  float* mean;
  const float* hess;
  float* acc_g;
  float* acc_h;
  const uint32_t* step;
  const float* noise;
  float* bank;
};

// training form.  FOLD: sample >= 1
template <bool FOLD>
__global__ __launch_bounds__(256) void ivon_draw_kernel(const IvDrawK k) {
  long base;
  const int t = k.list.find((int)blockIdx.x, kStreamChunk, base);
  const long n = k.list.numel[t];
  float* __restrict__ p = k.p[t];
  const float* __restrict__ g = k.g[t];
  float* __restrict__ mean = k.mean + k.off[t];
  const float* __restrict__ hess = k.hess + k.off[t];
  float* __restrict__ acc_g = FOLD ? k.acc_g + k.off[t] : nullptr;
  float* __restrict__ acc_h = FOLD ? k.acc_h + k.off[t] : nullptr;
  const float* __restrict__ noise = k.noise + k.off[t];
  const uint32_t q = *k.step * k.S + k.s;
  const float ess = k.ess, delta = k.delta;
#pragma unroll 1
  for (int it = 0; it < kStreamIters; ++it) {
    const long i = base + ((long)it * 256 + threadIdx.x) * 4;
    if (i >= n) break;
    const bool full = i + 3 < n;
    float mv[4], hv[4], e[4], th[4], rv[4];
    ld4(hess, i, n, full, hv);
    if (FOLD) {
      ld4(mean, i, n, full, mv);
    } else {
      ld4(p, i, n, full, mv);
      st4(mean, i, n, full, mv);
    }
    ivon_noise(k.eps_mode, noise, k.stride, (long)k.s, i, n, full, q, (uint32_t)t, k.k0, k.k1, e);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float hd, sigma;
      ivon_scale(hv[j], ess, delta, hd, rv[j], sigma);
      th[j] = __builtin_fmaf(sigma, e[j], mv[j]);
    }
    st4(p, i, n, full, th);
    if (FOLD) {
      float gv[4], ag[4], ah[4];
      ld4(g, i, n, full, gv);
      ivon_noise(k.eps_mode, noise, k.stride, (long)k.s - 1, i, n, full, q - 1u, (uint32_t)t, k.k0, k.k1, e);
      if (k.s == 1u) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          ag[j] = gv[j];
          ah[j] = gv[j] * (e[j] * rv[j]);
        }
      } else {
        ld4(acc_g, i, n, full, ag);
        ld4(acc_h, i, n, full, ah);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          ag[j] = ag[j] + gv[j];
          ah[j] = __builtin_fmaf(gv[j], e[j] * rv[j], ah[j]);
        }
      }
      st4(acc_g, i, n, full, ag);
      st4(acc_h, i, n, full, ah);
    }
  }
}

// bank form: members q0 .. q0 + mq - 1 of the launch per block (blockIdx.y takes a group of them)
__global__ __launch_bounds__(256) void ivon_bank_kernel(const IvDrawK k) {
  long base;
  const int t = k.list.find((int)blockIdx.x, kStreamChunk, base);
  const long n = k.list.numel[t];
  const float* __restrict__ p = k.p[t];
  const float* __restrict__ hess = k.hess + k.off[t];
  const float* __restrict__ noise = k.noise + k.off[t];
  float* __restrict__ out = k.bank + (long)k.first * k.stride + k.off[t];
  const uint32_t q0 = blockIdx.y * k.mgroup;
  const uint32_t mq = k.m - q0 < k.mgroup ? k.m - q0 : k.mgroup;
  const float ess = k.ess, delta = k.delta;
#pragma unroll 1
  for (int it = 0; it < kStreamIters; ++it) {
    const long i = base + ((long)it * 256 + threadIdx.x) * 4;
    if (i >= n) break;
    const bool full = i + 3 < n;
    float mv[4], hv[4], sg[4];
    ld4(p, i, n, full, mv);
    ld4(hess, i, n, full, hv);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float hd, r;
      ivon_scale(hv[j], ess, delta, hd, r, sg[j]);
    }
#pragma unroll 1
    for (uint32_t qq = 0; qq < mq; ++qq) {
      const uint32_t q = q0 + qq;
      float e[4], th[4];
      ivon_noise(k.eps_mode, noise, k.stride, (long)q, i, n, full, k.sample_base + q, (uint32_t)t, k.k0, k.k1, e);
#pragma unroll
      for (int j = 0; j < 4; ++j) th[j] = __builtin_fmaf(sg[j], e[j], mv[j]);
      st4(out + (long)q * k.stride, i, n, full, th);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------- the step
struct IvStepK {
  float* p[kMaxT];
  const float* g[kMaxT];
  long off[kMaxT];
  ChunkList<kMaxT> list;
  float lr, ess, delta, beta1, c1, cS, rho, c2, clip;
  double beta1_d;
  const float* lr_dev;
  uint32_t S, k0, k1;
  int eps_mode;
  long stride;
  const float* mean;
  float* hess;
  float* gm;
  const float* acc_g;
  const float* acc_h;
  const float* noise;
  uint32_t* step;
  double* prod;
  uint32_t* ticket;
};

template <bool MULTI, bool CLIP>
__global__ __launch_bounds__(256) void ivon_step_kernel(const IvStepK k) {
  long base;
  const int t = k.list.find((int)blockIdx.x, kStreamChunk, base);
  const long n = k.list.numel[t];
  float* __restrict__ p = k.p[t];
  const float* __restrict__ g = k.g[t];
  const float* __restrict__ mean = k.mean + k.off[t];
  float* __restrict__ hess = k.hess + k.off[t];
  float* __restrict__ gm = k.gm + k.off[t];
  const float* __restrict__ acc_g = MULTI ? k.acc_g + k.off[t] : nullptr;
  const float* __restrict__ acc_h = MULTI ? k.acc_h + k.off[t] : nullptr;
  const float* __restrict__ noise = k.noise + k.off[t];
  // every block reads the OLD step and product words; the block that arrives last advances them (below)
  const uint32_t step = *k.step;
  const double prod = *k.prod;
  const uint32_t q = step * k.S + (k.S - 1u);
  const float ib = (float)(1.0 / __builtin_fma(-prod, k.beta1_d, 1.0));
  const float nlr = -(k.lr_dev ? *k.lr_dev : k.lr);
  const float ess = k.ess, delta = k.delta, beta1 = k.beta1, c1 = k.c1, ncS = -k.cS, nrho = -k.rho, c2 = k.c2, clip = k.clip;
  // the arithmetic and the stores of one float4 whose operands are loaded; `full`: all four elements exist
  auto finish = [&](const long i, const bool full, const float gv[4], const float mv[4], float hv[4], float av[4], const float ag[4],
                    const float ah[4]) {
    float e[4], pv[4];
    ivon_noise(k.eps_mode, noise, k.stride, (long)k.S - 1, i, n, full, q, (uint32_t)t, k.k0, k.k1, e);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float hd, r, sigma;
      ivon_scale(hv[j], ess, delta, hd, r, sigma);
      const float er = e[j] * r;
      const float gs = MULTI ? ag[j] + gv[j] : gv[j];
      const float hs = MULTI ? __builtin_fmaf(gv[j], er, ah[j]) : gv[j] * er;
      av[j] = __builtin_fmaf(beta1, av[j], c1 * gs);
      const float d = __builtin_fmaf(ncS, hs, hv[j]);
      hv[j] = __builtin_fmaf(c2, (d * d) / hd, __builtin_fmaf(nrho, d, hv[j]));
      float u = __builtin_fmaf(delta, mv[j], av[j] * ib) / (hv[j] + delta);
      if (CLIP) u = fminf(fmaxf(u, -clip), clip);
      pv[j] = __builtin_fmaf(nlr, u, mv[j]);
    }
    st4(p, i, n, full, pv);
    st4(hess, i, n, full, hv);
    st4(gm, i, n, full, av);
  };
  if (base + kStreamChunk <= n) {
    // a whole chunk (all but a tensor's last): every load of the four iterations is issued before the first result is needed,
    // as bnn_adam_step's unrolled loop does; the stores follow each iteration's arithmetic
    float gv[kStreamIters][4], mv[kStreamIters][4], hv[kStreamIters][4], av[kStreamIters][4], ag[kStreamIters][4], ah[kStreamIters][4];
#pragma unroll
    for (int it = 0; it < kStreamIters; ++it) {
      const long i = base + ((long)it * 256 + threadIdx.x) * 4;
      ld4(g, i, n, true, gv[it]);
      ld4(mean, i, n, true, mv[it]);
      ld4(hess, i, n, true, hv[it]);
      ld4(gm, i, n, true, av[it]);
      if (MULTI) {
        ld4(acc_g, i, n, true, ag[it]);
        ld4(acc_h, i, n, true, ah[it]);
      }
    }
#pragma unroll
    for (int it = 0; it < kStreamIters; ++it)
      finish(base + ((long)it * 256 + threadIdx.x) * 4, true, gv[it], mv[it], hv[it], av[it], ag[it], ah[it]);
  } else {
#pragma unroll 1
    for (int it = 0; it < kStreamIters; ++it) {
      const long i = base + ((long)it * 256 + threadIdx.x) * 4;
      if (i >= n) break;
      const bool full = i + 3 < n;
      float gv[4], mv[4], hv[4], av[4], ag[4], ah[4];
      ld4(g, i, n, full, gv);
      ld4(mean, i, n, full, mv);
      ld4(hess, i, n, full, hv);
      ld4(gm, i, n, full, av);
      if (MULTI) {
        ld4(acc_g, i, n, full, ag);
        ld4(acc_h, i, n, full, ah);
      }
      finish(i, full, gv, mv, hv, av, ag, ah);
    }
  }
  last_block(k.ticket, [&] {
    *k.step = step + 1u;
    *k.prod = prod * k.beta1_d;
  });
}

// the chunk list and the state offsets of a tensor list; BNN_OK or the refusal
template <class K>
int lay_out(K& k, int n_tensors, const int64_t* numel) {
  for (int t = 0; t < kMaxT; ++t) {
    k.p[t] = nullptr; k.g[t] = nullptr;
  }
  return state_offsets(k.list, n_tensors, numel, k.off, k.stride);
}

}  // namespace
}  // namespace bnn

using namespace bnn;

extern "C" int bnn_ivon_draw(const bnn_ivon_draw_args* a, void* stream_) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_ivon_draw_args)) return BNN_ERR_ABI;
  const bool bank = a->bank != nullptr;
  if (a->n_tensors <= 0 || a->n_tensors > BNN_SGMCMC_MAX_TENSORS || a->samples < 1 || a->samples > BNN_IVON_MAX_SAMPLES ||
      a->sample < 0 || a->sample >= a->samples)
    return BNN_ERR_SHAPE;
  if (bank && (a->members <= 0 || a->members > BNN_IVON_MAX_MEMBERS || a->first < 0 || a->capacity <= 0 ||
               (long)a->first + a->members > a->capacity))
    return BNN_ERR_SHAPE;
  if (!(a->ess > 0.0) || !(a->weight_decay > 0.0)) return BNN_ERR_SHAPE;
  IvDrawK k;
  const int st = lay_out(k, a->n_tensors, a->numel);
  if (st != BNN_OK) return st;
  if ((unsigned)a->eps_mode > (unsigned)BNN_EPS_ZERO) return BNN_ERR_ENUM;
  const bool mem = a->eps_mode == BNN_EPS_MEMORY, fold = !bank && a->sample >= 1;
  if (!a->hess || (!bank && (!a->mean || !a->step)) || (fold && (!a->acc_g || !a->acc_h)) || (mem && !a->noise)) return BNN_ERR_NULL;
  uintptr_t al = bits(a->hess) | (bank ? bits(a->bank) : bits(a->mean)) | (fold ? bits(a->acc_g) | bits(a->acc_h) : 0) |
                 (mem ? bits(a->noise) : 0);
  for (int t = 0; t < a->n_tensors; ++t) {
    if (!a->param[t] || (fold && !a->grad[t])) return BNN_ERR_NULL;
    k.p[t] = a->param[t];
    k.g[t] = fold ? a->grad[t] : nullptr;
    al |= bits(k.p[t]) | bits(k.g[t]);
  }
  if ((al & 15) || (!bank && misaligned(a->step, 4))) return BNN_ERR_ALIGN;
  const int chunks = k.list.finish();
  k.ess = (float)a->ess; k.delta = (float)a->weight_decay;
  k.S = (uint32_t)a->samples; k.s = (uint32_t)a->sample;
  k.m = bank ? (uint32_t)a->members : 0u; k.first = bank ? (uint32_t)a->first : 0u; k.sample_base = a->sample_base;
  k.k0 = (uint32_t)a->seed; k.k1 = (uint32_t)(a->seed >> 32);
  k.eps_mode = a->eps_mode;
  k.mean = bank ? nullptr : a->mean; k.hess = a->hess;
  k.acc_g = fold ? a->acc_g : nullptr; k.acc_h = fold ? a->acc_h : nullptr;
  k.step = bank ? nullptr : a->step; k.noise = mem ? a->noise : nullptr; k.bank = a->bank;
  k.mgroup = 1;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (bank) {
    // a small network has few chunks: the members are then split over blockIdx.y (bnn_swag_sample's rule), each group re-reading
    // m and h out of the caches.  Speed only: a member's values do not depend on the split.
    unsigned groups = 1;
    while ((long)chunks * groups < 512 && (a->members + 2 * groups - 1) / (2 * groups) >= 2) groups *= 2;
    k.mgroup = ((uint32_t)a->members + groups - 1) / groups;
    hipLaunchKernelGGL(ivon_bank_kernel, dim3((unsigned)chunks, (k.m + k.mgroup - 1) / k.mgroup), dim3(256), 0, stream, k);
  } else if (fold) {
    hipLaunchKernelGGL(ivon_draw_kernel<true>, dim3((unsigned)chunks), dim3(256), 0, stream, k);
  } else {
    hipLaunchKernelGGL(ivon_draw_kernel<false>, dim3((unsigned)chunks), dim3(256), 0, stream, k);
  }
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}

extern "C" int bnn_ivon_step(const bnn_ivon_step_args* a, void* stream_) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_ivon_step_args)) return BNN_ERR_ABI;
  if (a->n_tensors <= 0 || a->n_tensors > BNN_SGMCMC_MAX_TENSORS || a->samples < 1 || a->samples > BNN_IVON_MAX_SAMPLES)
    return BNN_ERR_SHAPE;
  if (!(a->ess > 0.0) || !(a->weight_decay > 0.0) || !(a->lr >= 0.0) || !(a->beta1 >= 0.0 && a->beta1 < 1.0) ||
      !(a->beta2 >= 0.0 && a->beta2 <= 1.0) || !(a->loss_scale > 0.0) || !(a->clip_radius > 0.0))
    return BNN_ERR_SHAPE;
  IvStepK k;
  const int st = lay_out(k, a->n_tensors, a->numel);
  if (st != BNN_OK) return st;
  if ((unsigned)a->eps_mode > (unsigned)BNN_EPS_ZERO) return BNN_ERR_ENUM;
  const bool mem = a->eps_mode == BNN_EPS_MEMORY, multi = a->samples > 1;
  if (!a->step || !a->beta1_prod || !a->ticket || !a->mean || !a->hess || !a->avg_grad || (multi && (!a->acc_g || !a->acc_h)) ||
      (mem && !a->noise))
    return BNN_ERR_NULL;
  uintptr_t al = bits(a->mean) | bits(a->hess) | bits(a->avg_grad) | (multi ? bits(a->acc_g) | bits(a->acc_h) : 0) |
                 (mem ? bits(a->noise) : 0);
  for (int t = 0; t < a->n_tensors; ++t) {
    if (!a->param[t] || !a->grad[t]) return BNN_ERR_NULL;
    k.p[t] = a->param[t]; k.g[t] = a->grad[t];
    al |= bits(k.p[t]) | bits(k.g[t]);
  }
  if ((al & 15) || misaligned(a->lr_device, 4) || misaligned(a->step, 4) || misaligned(a->beta1_prod, 8) || misaligned(a->ticket, 4))
    return BNN_ERR_ALIGN;
  const int chunks = k.list.finish();
  const double S = (double)a->samples, rho = 1.0 - a->beta2;
  k.lr = (float)a->lr; k.ess = (float)a->ess; k.delta = (float)a->weight_decay; k.beta1 = (float)a->beta1;
  k.c1 = (float)((1.0 - a->beta1) * a->loss_scale / S); k.cS = (float)(a->loss_scale / S);
  k.rho = (float)rho; k.c2 = (float)(0.5 * rho * rho); k.clip = (float)a->clip_radius;
  k.beta1_d = a->beta1; k.lr_dev = a->lr_device;
  k.S = (uint32_t)a->samples; k.k0 = (uint32_t)a->seed; k.k1 = (uint32_t)(a->seed >> 32);
  k.eps_mode = a->eps_mode;
  k.mean = a->mean; k.hess = a->hess; k.gm = a->avg_grad;
  k.acc_g = multi ? a->acc_g : nullptr; k.acc_h = multi ? a->acc_h : nullptr; k.noise = mem ? a->noise : nullptr;
  k.step = a->step; k.prod = a->beta1_prod; k.ticket = a->ticket;
  const bool clip = a->clip_radius < __builtin_inf();
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const dim3 grid((unsigned)chunks), block(256);
  if (multi) {
    if (clip) hipLaunchKernelGGL((ivon_step_kernel<true, true>), grid, block, 0, stream, k);
    else hipLaunchKernelGGL((ivon_step_kernel<true, false>), grid, block, 0, stream, k);
  } else {
    if (clip) hipLaunchKernelGGL((ivon_step_kernel<false, true>), grid, block, 0, stream, k);
    else hipLaunchKernelGGL((ivon_step_kernel<false, false>), grid, block, 0, stream, k);
  }
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}
