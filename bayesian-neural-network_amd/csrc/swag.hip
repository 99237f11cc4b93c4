// F22  SWAG for MLP (Maddox et al. 2019): the SGD step that also folds the new iterate into running moments and a ring of
// deviations in the same pass over the parameters (bnn_swag_step: torch.optim.SGD with momentum and weight decay, Welford's
// mean / second-moment update and row n % K of the deviation matrix on a collecting step), and the draw of m bank members
// from the fitted Gaussian in one launch (bnn_swag_sample: the mean, the second-moment statistic and the K deviation rows
// read once, the normals generated on chip).
//
// The step is pure streaming like bnn_sgd_step: p, g read and p written (12 B / parameter), + 8 B with a momentum buffer,
// + 16 B (mean, m2 read and written) + 4 B (one row of D) on a collecting step.  One block = one 4096-element chunk of one
// tensor, 16-byte accesses, the step and count words advanced by the launch's last block (bnn_stream.h's ticketed hand-off).
//
// The draw holds a thread's float4 of mean, sqrt(var) and the Keff rows of D in registers and loops over the members:
// (2 + Keff + m) * 4 B per element and launch whatever m; per member and float4 one Philox call, 4 (Keff + 2) fmas and one
// 16-byte store.  z2 (m x Keff, shared by every element) is formed once per block into LDS.  A network of few chunks has its
// members split over blockIdx.y (each group re-reads the moments, out of the caches at that size) so that the grid fills the chip.
#include "bnn_device.h"
#include "bnn_stream.h"
#include "../../include/bnn_hip.h"

namespace bnn {
namespace {

constexpr uint32_t kSwWord3 = 5u;       // counter word 3 of the SWAG noise streams (include/bnn_hip.h F22)
constexpr int kMaxT = BNN_SGMCMC_MAX_TENSORS;

struct SwStepK {
  float* p[kMaxT];
  const float* g[kMaxT];
  float* v[kMaxT];
  long off[kMaxT];                         // the tensor's first element in mean / m2 / a row of D
  ChunkList<kMaxT> list;
  float lr, mu, wd;
  const float* lr_dev;
  uint32_t start, every, K;
  long stride;
  float* mean;
  float* m2;
  float* dev;
  uint32_t* step;
  uint32_t* count;
  uint32_t* ticket;
};

template <bool MOM>
__global__ __launch_bounds__(256) void swag_step_kernel(const SwStepK k) {
  long base;
  const int t = k.list.find((int)blockIdx.x, kStreamChunk, base);
  const long n = k.list.numel[t];
  float* __restrict__ p = k.p[t];
  const float* __restrict__ g = k.g[t];
  float* __restrict__ v = k.v[t];
  // every block reads the OLD step and count words (independent loads: one round trip); the block that arrives last advances
  // them (below)
  const uint32_t step = *k.step;
  const uint32_t cnt = *k.count;
  const bool collect = step >= k.start && (step - k.start + 1u) % k.every == 0u;
  const float r = 1.0f / (float)(cnt + 1u);
  float* __restrict__ mean = k.mean + k.off[t];
  float* __restrict__ m2 = k.m2 + k.off[t];
  float* __restrict__ row = (collect && k.K) ? k.dev + (long)(cnt % k.K) * k.stride + k.off[t] : nullptr;
  const float nlr = -(k.lr_dev ? *k.lr_dev : k.lr);
  const float wd = k.wd, mu = k.mu;
#pragma unroll
  for (int it = 0; it < kStreamIters; ++it) {
    const long i = base + ((long)it * 256 + threadIdx.x) * 4;
    if (i >= n) break;
    const bool full = i + 3 < n;
    float pv[4], gv[4], vv[4] = {0.f, 0.f, 0.f, 0.f}, av[4] = {0.f, 0.f, 0.f, 0.f}, sv[4] = {0.f, 0.f, 0.f, 0.f}, dv[4];
    ld4(p, i, n, full, pv);
    ld4(g, i, n, full, gv);
    if (MOM) ld4(v, i, n, full, vv);
    if (collect) {
      ld4(mean, i, n, full, av);
      ld4(m2, i, n, full, sv);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float gg = wd != 0.f ? __builtin_fmaf(wd, pv[j], gv[j]) : gv[j];
      float u = gg;
      if (MOM) u = vv[j] = __builtin_fmaf(mu, vv[j], gg);
      pv[j] = __builtin_fmaf(nlr, u, pv[j]);
      if (collect) {                                        // Welford: the deviation uses the updated mean
        const float d = pv[j] - av[j];
        av[j] = __builtin_fmaf(d, r, av[j]);
        dv[j] = pv[j] - av[j];
        sv[j] = __builtin_fmaf(d, dv[j], sv[j]);
      }
    }
    st4(p, i, n, full, pv);
    if (MOM) st4(v, i, n, full, vv);
    if (collect) {
      st4(mean, i, n, full, av);
      st4(m2, i, n, full, sv);
      if (row) st4(row, i, n, full, dv);
    }
  }
  last_block(k.ticket, [&] {
    *k.step = step + 1u;
    if (collect) *k.count = cnt + 1u;
  });
}

// ---------------------------------------------------------------------------------------------------------- the draw
struct SwSampleK {
  long off[kMaxT];
  ChunkList<kMaxT> list;
  const float* mean;
  const float* m2;
  const float* dev;
  const uint32_t* count;
  const float* z1;                       // BNN_EPS_MEMORY: [m, stride]
  const float* z2;                       // BNN_EPS_MEMORY: [m, K]
  float* bank;
  long stride;
  uint32_t K, m, mgroup, first, sample_base, k0, k1;   // mgroup: members per block (blockIdx.y takes a group of them)
  int eps_mode, low_rank;
  float c_d, var_clamp;
  float c_lr[BNN_SWAG_MAX_RANK + 1];
};

// KB: a compile-time bound of the rank (a multiple of 4): the rows of D a thread holds are registers, never an indexed array
template <int KB>
__global__ __launch_bounds__(256) void swag_sample_kernel(const SwSampleK k) {
  __shared__ float4 z2s[BNN_SWAG_MAX_MEMBERS][BNN_SWAG_MAX_RANK / 4];
  long base;
  const int t = k.list.find((int)blockIdx.x, kStreamChunk, base);
  const long n = k.list.numel[t];
  const uint32_t cnt = *k.count;
  const uint32_t Keff = k.low_rank ? (cnt < k.K ? cnt : k.K) : 0u;
  const float r = cnt ? 1.0f / (float)cnt : 0.f;
  const float clr = k.c_lr[Keff];
  // the block's members q0 .. q0 + mq - 1 of the launch
  const uint32_t q0 = blockIdx.y * k.mgroup;
  const uint32_t mq = k.m - q0 < k.mgroup ? k.m - q0 : k.mgroup;
  if (KB > 0) {
    // z2[q][4 g .. 4 g + 3], g < KB / 4, for the block's members: once per block
    for (uint32_t w = threadIdx.x; w < mq * (uint32_t)(KB / 4); w += 256u) {
      const uint32_t qq = w / (uint32_t)(KB / 4), q = q0 + qq, gq = w % (uint32_t)(KB / 4);
      float e[4] = {0.f, 0.f, 0.f, 0.f};
      if (k.eps_mode == BNN_EPS_PHILOX) {
        philox_normal4(gq, k.sample_base + q, (uint32_t)kMaxT, k.k0, k.k1, e, kSwWord3);   // stream kMaxT: z2
      } else if (k.eps_mode == BNN_EPS_MEMORY) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (4u * gq + j < Keff) e[j] = k.z2[(long)q * k.K + 4u * gq + j];
      }
      z2s[qq][gq] = make_float4(e[0], e[1], e[2], e[3]);
    }
    __syncthreads();
  }
  const float* __restrict__ mean = k.mean + k.off[t];
  const float* __restrict__ m2 = k.m2 + k.off[t];
  const float* __restrict__ dev = k.dev + k.off[t];
  const float* __restrict__ z1 = k.z1 + k.off[t];
  float* __restrict__ out = k.bank + (long)k.first * k.stride + k.off[t];
#pragma unroll 1
  for (int it = 0; it < kStreamIters; ++it) {
    const long i = base + ((long)it * 256 + threadIdx.x) * 4;
    if (i >= n) break;
    const bool full = i + 3 < n;
    float av[4], cs[4];
    float4 D[KB > 0 ? KB : 1];
    ld4(mean, i, n, full, av);
    ld4(m2, i, n, full, cs);
    if (full) {
#pragma unroll
      for (int j = 0; j < KB; ++j)
        if ((uint32_t)j < Keff) D[j] = *reinterpret_cast<const float4*>(dev + (long)j * k.stride + i);
    } else {
#pragma unroll
      for (int j = 0; j < KB; ++j)
        if ((uint32_t)j < Keff) {
          const float* __restrict__ dr = dev + (long)j * k.stride + i;
          D[j] = make_float4(dr[0], i + 1 < n ? dr[1] : 0.f, i + 2 < n ? dr[2] : 0.f, 0.f);
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) cs[e] = k.c_d * __builtin_sqrtf(fmaxf(cs[e] * r, k.var_clamp));
#pragma unroll 1
    for (uint32_t qq = 0; qq < mq; ++qq) {
      const uint32_t q = q0 + qq;
      float th[4];
      if (k.eps_mode == BNN_EPS_ZERO) {
#pragma unroll
        for (int e = 0; e < 4; ++e) th[e] = av[e];
      } else {
        float z[4];
        if (k.eps_mode == BNN_EPS_PHILOX) {
          philox_normal4((uint32_t)(i >> 2), k.sample_base + q, (uint32_t)t, k.k0, k.k1, z, kSwWord3);
        } else {
          ld4(z1 + (long)q * k.stride, i, n, full, z);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) th[e] = __builtin_fmaf(cs[e], z[e], av[e]);
        if (KB > 0 && k.low_rank) {
          float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int jg = 0; jg < KB / 4; ++jg) {
            if ((uint32_t)(4 * jg) < Keff) {
              const float4 zz = z2s[qq][jg];
              const float zj[4] = {zz.x, zz.y, zz.z, zz.w};
#pragma unroll
              for (int jj = 0; jj < 4; ++jj) {
                const int j = 4 * jg + jj;
                if ((uint32_t)j < Keff) {
                  acc[0] = __builtin_fmaf(D[j].x, zj[jj], acc[0]);
                  acc[1] = __builtin_fmaf(D[j].y, zj[jj], acc[1]);
                  acc[2] = __builtin_fmaf(D[j].z, zj[jj], acc[2]);
                  acc[3] = __builtin_fmaf(D[j].w, zj[jj], acc[3]);
                }
              }
            }
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) th[e] = __builtin_fmaf(clr, acc[e], th[e]);
        }
      }
      st4(out + (long)q * k.stride, i, n, full, th);
    }
  }
}

template <int KB>
void launch_sample(const SwSampleK& k, int chunks, hipStream_t st) {
  hipLaunchKernelGGL(swag_sample_kernel<KB>, dim3((unsigned)chunks, (k.m + k.mgroup - 1) / k.mgroup), dim3(256), 0, st, k);
}

}  // namespace
}  // namespace bnn

using namespace bnn;

extern "C" int bnn_swag_step(const bnn_swag_step_args* a, void* stream_) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_swag_step_args)) return BNN_ERR_ABI;
  if (a->n_tensors <= 0 || a->n_tensors > BNN_SGMCMC_MAX_TENSORS || a->rank < 0 || a->rank > BNN_SWAG_MAX_RANK || a->every == 0)
    return BNN_ERR_SHAPE;
  if (!(a->momentum_factor >= 0.0) || !(a->weight_decay >= 0.0) || !(a->lr >= 0.0)) return BNN_ERR_SHAPE;
  SwStepK k;
  for (int t = 0; t < BNN_SGMCMC_MAX_TENSORS; ++t) {
    k.p[t] = nullptr; k.g[t] = nullptr; k.v[t] = nullptr;
  }
  if (const int st = state_offsets(k.list, a->n_tensors, a->numel, k.off, k.stride); st != BNN_OK) return st;
  if (!a->step || !a->count || !a->ticket || !a->mean || !a->m2 || (a->rank > 0 && !a->dev)) return BNN_ERR_NULL;
  const bool mom = a->momentum[0] != nullptr;
  uintptr_t al = reinterpret_cast<uintptr_t>(a->mean) | reinterpret_cast<uintptr_t>(a->m2) |
                 (a->rank > 0 ? reinterpret_cast<uintptr_t>(a->dev) : 0);
  for (int t = 0; t < a->n_tensors; ++t) {
    if (!a->param[t] || !a->grad[t] || (a->momentum[t] != nullptr) != mom) return BNN_ERR_NULL;
    k.p[t] = a->param[t]; k.g[t] = a->grad[t]; k.v[t] = a->momentum[t];
    al |= reinterpret_cast<uintptr_t>(k.p[t]) | reinterpret_cast<uintptr_t>(k.g[t]) | reinterpret_cast<uintptr_t>(k.v[t]);
  }
  if ((al & 15) || misaligned(a->lr_device, 4) || misaligned(a->step, 4) || misaligned(a->count, 4) || misaligned(a->ticket, 4))
    return BNN_ERR_ALIGN;
  const int chunks = k.list.finish();
  k.lr = (float)a->lr; k.mu = (float)a->momentum_factor; k.wd = (float)a->weight_decay; k.lr_dev = a->lr_device;
  k.start = a->start; k.every = a->every; k.K = (uint32_t)a->rank;
  k.mean = a->mean; k.m2 = a->m2; k.dev = a->rank > 0 ? a->dev : nullptr;
  k.step = a->step; k.count = a->count; k.ticket = a->ticket;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (mom) hipLaunchKernelGGL(swag_step_kernel<true>, dim3((unsigned)chunks), dim3(256), 0, stream, k);
  else hipLaunchKernelGGL(swag_step_kernel<false>, dim3((unsigned)chunks), dim3(256), 0, stream, k);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}

extern "C" int bnn_swag_sample(const bnn_swag_sample_args* a, void* stream_) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_swag_sample_args)) return BNN_ERR_ABI;
  if (a->n_tensors <= 0 || a->n_tensors > BNN_SGMCMC_MAX_TENSORS || a->rank < 0 || a->rank > BNN_SWAG_MAX_RANK ||
      a->members <= 0 || a->members > BNN_SWAG_MAX_MEMBERS || a->first < 0 || a->capacity <= 0 ||
      (long)a->first + a->members > a->capacity || (a->low_rank && a->rank == 0) || !(a->var_clamp >= 0.f))
    return BNN_ERR_SHAPE;
  SwSampleK k;
  if (const int st = state_offsets(k.list, a->n_tensors, a->numel, k.off, k.stride); st != BNN_OK) return st;
  if ((unsigned)a->eps_mode > (unsigned)BNN_EPS_ZERO) return BNN_ERR_ENUM;
  const bool mem = a->eps_mode == BNN_EPS_MEMORY, lowr = a->low_rank != 0;
  if (!a->mean || !a->m2 || !a->count || !a->bank || (lowr && !a->dev) || (mem && !a->z1) || (mem && lowr && !a->z2))
    return BNN_ERR_NULL;
  const uintptr_t al = reinterpret_cast<uintptr_t>(a->mean) | reinterpret_cast<uintptr_t>(a->m2) |
                       reinterpret_cast<uintptr_t>(a->bank) | (lowr ? reinterpret_cast<uintptr_t>(a->dev) : 0) |
                       (mem ? reinterpret_cast<uintptr_t>(a->z1) : 0);
  if ((al & 15) || misaligned(a->count, 4) || (mem && lowr && misaligned(a->z2, 4))) return BNN_ERR_ALIGN;
  const int chunks = k.list.finish();
  k.mean = a->mean; k.m2 = a->m2; k.dev = lowr ? a->dev : nullptr; k.count = a->count;
  k.z1 = mem ? a->z1 : nullptr; k.z2 = mem && lowr ? a->z2 : nullptr;
  k.bank = a->bank;
  // a small network has few chunks: the members are then split over blockIdx.y (halved while under two blocks per CU and two
  // members per block), each group re-reading the moments -- out of L2 / the Infinity Cache at that size.  Speed only: a
  // member's values do not depend on the split.
  unsigned groups = 1;
  while ((long)chunks * groups < 512 && (a->members + 2 * groups - 1) / (2 * groups) >= 2) groups *= 2;
  k.mgroup = ((uint32_t)a->members + groups - 1) / groups;
  k.K = (uint32_t)a->rank; k.m = (uint32_t)a->members; k.first = (uint32_t)a->first; k.sample_base = a->sample_base;
  k.k0 = (uint32_t)a->seed; k.k1 = (uint32_t)(a->seed >> 32);
  k.eps_mode = a->eps_mode; k.low_rank = lowr ? 1 : 0;
  k.c_d = a->c_d; k.var_clamp = a->var_clamp;
  for (int e = 0; e <= BNN_SWAG_MAX_RANK; ++e) k.c_lr[e] = a->c_lr[e];
  hipStream_t st = reinterpret_cast<hipStream_t>(stream_);
  switch (lowr ? (a->rank + 3) / 4 : 0) {
    case 0: launch_sample<0>(k, chunks, st); break;
    case 1: launch_sample<4>(k, chunks, st); break;
    case 2: launch_sample<8>(k, chunks, st); break;
    case 3: launch_sample<12>(k, chunks, st); break;
    case 4: launch_sample<16>(k, chunks, st); break;
    case 5: launch_sample<20>(k, chunks, st); break;
    case 6: launch_sample<24>(k, chunks, st); break;
    case 7: launch_sample<28>(k, chunks, st); break;
    default: launch_sample<32>(k, chunks, st); break;
  }
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}
