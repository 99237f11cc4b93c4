// F19  stochastic-gradient MCMC for MLP: the sampler step that takes the optimiser's place in K6's captured training step
// (bnn_sgmcmc_step: SGLD / SGHMC over every parameter tensor in one launch, the chain's samples filed into a device-resident
// ring of weight snapshots in the same pass), its noise stream materialised for tests (bnn_sgmcmc_noise), and the forward of
// one Linear -> [ReLU] layer for M members of such a bank in one launch (bnn_bank_fwd).
//
// The step is pure streaming like Adam's: SGLD reads p, g and writes p (12 B / parameter), SGHMC adds v read and written
// (20 B), a collecting step 4 B more; the noise is generated on chip.  One block = one 4096-element chunk of one tensor,
// 16-byte accesses, the step word advanced by the launch's last block (bnn_stream.h's ticketed hand-off).
//
// The bank forward is K5's product per member: dense_tile.h's 64 x 64 tile core (the same stage image, the same MFMA chain
// over 32-wide k stages as K5, so a member's output equals bnn_dense_fwd on that member's weights bit for bit), one tile of
// ONE member per block.  Every member brings its own weights, so the launch streams the bank from HBM once; the work list
// is ordered (member, column tile, row tile) and dealt to the XCDs in contiguous ranges, so that the row tiles that share a
// weight tile run on one XCD and meet in its L2.
#include "bnn_device.h"
#include "bnn_stream.h"
#include "dense_tile.h"
#include "../../include/bnn_hip.h"

namespace bnn {
namespace {

constexpr uint32_t kSgWord3 = 3u;       // counter word 3 of the SG-MCMC noise stream (include/bnn_hip.h F19)

struct SgK {
  float* p[BNN_SGMCMC_MAX_TENSORS];
  const float* g[BNN_SGMCMC_MAX_TENSORS];
  float* v[BNN_SGMCMC_MAX_TENSORS];
  const float* eps[BNN_SGMCMC_MAX_TENSORS];
  long off[BNN_SGMCMC_MAX_TENSORS];       // the tensor's first element in a bank member
  ChunkList<BNN_SGMCMC_MAX_TENSORS> list;
  const float4* table;                    // [L]: (a, b, c, collect flag)
  uint32_t L, burn_in, capacity, k0, k1;
  int eps_mode;
  float grad_scale, tau;
  long stride;
  float* bank;
  uint32_t* step;
  uint32_t* collected;
  uint32_t* ticket;
};

__device__ __forceinline__ void sg_update(float& p, float& v, float g, float e, float grad_scale, float tau, float a, float b,
                                          float c) {
  const float gg = __builtin_fmaf(grad_scale, g, tau * p);
  v = __builtin_fmaf(c, e, __builtin_fmaf(-a, gg, b * v));
  p = p + v;
}

template <bool MOM>
__global__ __launch_bounds__(256) void sgmcmc_kernel(const SgK k) {
  long base;
  const int t = k.list.find((int)blockIdx.x, kStreamChunk, base);
  const long n = k.list.numel[t];
  float* __restrict__ p = k.p[t];
  const float* __restrict__ g = k.g[t];
  float* __restrict__ v = k.v[t];
  const float* __restrict__ ep = k.eps[t];
  // every block reads the OLD step word and collected count; the block that arrives last advances them (below)
  const uint32_t step = *k.step;
  const float4 row = k.table[step % k.L];
  const bool collect = k.bank && step >= k.burn_in && row.w != 0.f;
  const uint32_t collected = collect ? *k.collected : 0u;
  float* __restrict__ slot = collect ? k.bank + (long)(collected % k.capacity) * k.stride + k.off[t] : nullptr;
  const float a = row.x, b = row.y, c = row.z;
#pragma unroll
  for (int it = 0; it < kStreamIters; ++it) {
    const long i = base + ((long)it * 256 + threadIdx.x) * 4;
    if (i >= n) break;
    const bool full = i + 3 < n;
    float pv[4], gv[4], vv[4] = {0.f, 0.f, 0.f, 0.f}, ev[4] = {0.f, 0.f, 0.f, 0.f};
    ld4(p, i, n, full, pv);
    ld4(g, i, n, full, gv);
    if (MOM) ld4(v, i, n, full, vv);
    if (k.eps_mode == BNN_EPS_MEMORY) ld4(ep, i, n, full, ev);
    if (k.eps_mode == BNN_EPS_PHILOX) philox_normal4((uint32_t)(i >> 2), step, (uint32_t)t, k.k0, k.k1, ev, kSgWord3);
#pragma unroll
    for (int j = 0; j < 4; ++j) sg_update(pv[j], vv[j], gv[j], ev[j], k.grad_scale, k.tau, a, b, c);
    st4(p, i, n, full, pv);
    if (MOM) st4(v, i, n, full, vv);
    if (collect) st4(slot, i, n, full, pv);
  }
  last_block(k.ticket, [&] {
    *k.step = step + 1u;
    if (collect) *k.collected = collected + 1u;
  });
}

__global__ void sgmcmc_noise_kernel(float* __restrict__ out, uint32_t k0, uint32_t k1, uint32_t tensor, uint32_t step, long numel) {
  const long groups = (numel + 3) >> 2;
  for (long gi = (long)blockIdx.x * blockDim.x + threadIdx.x; gi < groups; gi += (long)gridDim.x * blockDim.x) {
    float e[4];
    philox_normal4((uint32_t)gi, step, tensor, k0, k1, e, kSgWord3);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (4 * gi + j < numel) out[4 * gi + j] = e[j];
  }
}

// ---------------------------------------------------------------------------------------------------- the bank forward
// bf16 activations as an operand of dense_tile.h's gemm_tile (k contiguous; exact in fp32, rounded back unchanged)
struct Opnd16 {
  const __bf16* p;
  int ld, rows, vec;
};

template <bool KC>
__device__ __forceinline__ void fetch_seg(const Opnd16& o, int K, int r0, int k0, int s, float v[8]) {
  static_assert(KC, "bf16 activations are read along k");
  const int r = r0 + (s >> 2), k = k0 + 8 * (s & 3);
  const int valid = r < o.rows ? min(8, max(0, K - k)) : 0;
  const long base = (long)r * o.ld + k;
  if (o.vec && valid == 8) {
    const bf16x8 h = *reinterpret_cast<const bf16x8*>(o.p + base);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (float)h[j];
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = j < valid ? (float)o.p[base + j] : 0.f;
  }
}

struct BankK {
  const void* x;
  const float* w;
  const float* b;
  void* y;
  long w_stride, b_stride;
  int M, first, B, N, K, tiles_m, tiles_n, total;
  int x_shared, relu, vec_x, vec_w, vec_y;
};

__device__ __forceinline__ void put(float* dst, float v) { *dst = v; }
__device__ __forceinline__ void put(__bf16* dst, float v) { *dst = (__bf16)v; }
__device__ __forceinline__ void put4(float* dst, const float o[4]) { *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2], o[3]); }
__device__ __forceinline__ void put4(__bf16* dst, const float o[4]) {
  *reinterpret_cast<bf16x4*>(dst) = bf16x4{(__bf16)o[0], (__bf16)o[1], (__bf16)o[2], (__bf16)o[3]};
}

// T: the staged type (the math), XT / YT: the activations in memory
template <typename T, typename XT, typename YT>
__global__ __launch_bounds__(kThreads) void bank_fwd_kernel(const BankK k) {
  __shared__ uint4 lds[tile_lds_uint4<T, 2, 2>()];         // (bf16 stages: 17 KiB, 8 blocks per CU instead of 5)
  int item;
  if (!xcd_work_item(k.total, item)) return;
  // (member, column tile, row tile), the row tile fastest: an XCD's consecutive items share the member's weight tile
  const int tm = item % k.tiles_m, rest = item / k.tiles_m;
  const int tn = rest % k.tiles_n, j = rest / k.tiles_n;
  const int m0 = tm * kT, n0 = tn * kT;
  const long xoff = k.x_shared ? 0 : (long)j * k.B * k.K;
  const float* __restrict__ w = k.w + (long)(k.first + j) * k.w_stride;
  const float* __restrict__ b = k.b ? k.b + (long)(k.first + j) * k.b_stride : nullptr;
  YT* __restrict__ y = static_cast<YT*>(k.y) + (long)j * k.B * k.N;
  const Opnd Bo{w, nullptr, 1.f, k.K, k.N, k.vec_w};
  f32x4 acc[2][2];
  if constexpr (sizeof(XT) == 4) {
    const Opnd A{static_cast<const float*>(k.x) + xoff, nullptr, 1.f, k.K, k.B, k.vec_x};
    gemm_tile<T, true, true>(A, Bo, m0, n0, k.K, lds, acc);
  } else {
    const Opnd16 A{static_cast<const __bf16*>(k.x) + xoff, k.K, k.B, k.vec_x};
    gemm_tile<T, true, true>(A, Bo, m0, n0, k.K, lds, acc);
  }
  tile_epilogue(lds, acc, m0, n0, k.B, k.N, [&](int row, int col0, int ncol, float o[4]) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      o[c] += (b && c < ncol) ? b[col0 + c] : 0.f;
      if (k.relu) o[c] = fmaxf(o[c], 0.f);
    }
    YT* dst = y + (long)row * k.N + col0;
    if (ncol == 4 && k.vec_y) {
      put4(dst, o);
    } else {
      for (int c = 0; c < ncol; ++c) put(dst + c, o[c]);
    }
  });
}

template <typename T, typename XT, typename YT>
void launch_bank(const BankK& k, hipStream_t st) {
  const unsigned blocks = 8u * (unsigned)((k.total + 7) / 8);      // (xcd_work_item: 8 equal ranges)
  hipLaunchKernelGGL((bank_fwd_kernel<T, XT, YT>), dim3(blocks), dim3(kThreads), 0, st, k);
}

}  // namespace
}  // namespace bnn

using namespace bnn;

extern "C" int bnn_sgmcmc_noise(float* out, uint64_t seed, uint32_t tensor, uint32_t step, int64_t numel, void* stream_) {
  if (!out) return BNN_ERR_NULL;
  if (numel <= 0 || numel > ((int64_t)1 << 34) || tensor >= BNN_SGMCMC_MAX_TENSORS) return BNN_ERR_SHAPE;
  if (misaligned(out, 4)) return BNN_ERR_ALIGN;
  long nb = ((numel + 3) / 4 + 255) / 256;
  if (nb > 4096) nb = 4096;
  hipLaunchKernelGGL(sgmcmc_noise_kernel, dim3((unsigned)nb), dim3(256), 0, reinterpret_cast<hipStream_t>(stream_), out,
                     (uint32_t)seed, (uint32_t)(seed >> 32), tensor, step, (long)numel);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}

extern "C" int bnn_sgmcmc_step(const bnn_sgmcmc_args* a, void* stream_) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_sgmcmc_args)) return BNN_ERR_ABI;
  if (a->n_tensors <= 0 || a->n_tensors > BNN_SGMCMC_MAX_TENSORS || a->table_rows <= 0) return BNN_ERR_SHAPE;
  if (a->bank && a->capacity <= 0) return BNN_ERR_SHAPE;
  SgK k;
  for (int t = 0; t < BNN_SGMCMC_MAX_TENSORS; ++t) {
    k.p[t] = nullptr; k.g[t] = nullptr; k.v[t] = nullptr; k.eps[t] = nullptr;
  }
  if (const int st = state_offsets(k.list, a->n_tensors, a->numel, k.off, k.stride); st != BNN_OK) return st;
  if ((unsigned)a->eps_mode > (unsigned)BNN_EPS_ZERO) return BNN_ERR_ENUM;
  if (!a->table || !a->step || !a->ticket || (a->bank && !a->collected)) return BNN_ERR_NULL;
  const bool mom = a->momentum[0] != nullptr;
  uintptr_t al = reinterpret_cast<uintptr_t>(a->table) | reinterpret_cast<uintptr_t>(a->bank);
  for (int t = 0; t < a->n_tensors; ++t) {
    if (!a->param[t] || !a->grad[t] || (a->momentum[t] != nullptr) != mom || (a->eps_mode == BNN_EPS_MEMORY && !a->noise[t]))
      return BNN_ERR_NULL;
    k.p[t] = a->param[t]; k.g[t] = a->grad[t]; k.v[t] = a->momentum[t];
    k.eps[t] = a->eps_mode == BNN_EPS_MEMORY ? a->noise[t] : nullptr;
    al |= reinterpret_cast<uintptr_t>(k.p[t]) | reinterpret_cast<uintptr_t>(k.g[t]) | reinterpret_cast<uintptr_t>(k.v[t]) |
          reinterpret_cast<uintptr_t>(k.eps[t]);
  }
  if ((al & 15) || misaligned(a->step, 4) || misaligned(a->collected, 4) || misaligned(a->ticket, 4)) return BNN_ERR_ALIGN;
  const int chunks = k.list.finish();
  k.table = reinterpret_cast<const float4*>(a->table);
  k.L = (uint32_t)a->table_rows; k.burn_in = a->burn_in; k.capacity = a->bank ? (uint32_t)a->capacity : 1u;
  k.k0 = (uint32_t)a->seed; k.k1 = (uint32_t)(a->seed >> 32);
  k.eps_mode = a->eps_mode; k.grad_scale = a->grad_scale; k.tau = a->tau;
  k.bank = a->bank; k.step = a->step; k.collected = a->collected; k.ticket = a->ticket;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (mom) hipLaunchKernelGGL(sgmcmc_kernel<true>, dim3((unsigned)chunks), dim3(256), 0, stream, k);
  else hipLaunchKernelGGL(sgmcmc_kernel<false>, dim3((unsigned)chunks), dim3(256), 0, stream, k);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}

extern "C" int bnn_bank_fwd(const bnn_bank_fwd_args* a, void* stream_) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_bank_fwd_args)) return BNN_ERR_ABI;
  if (a->members <= 0 || a->first < 0 || a->batch <= 0 || a->in_features <= 0 || a->out_features <= 0 || a->w_stride < 0 ||
      a->b_stride < 0 || a->batch > INT32_MAX / 2 || (long)a->first + a->members > INT32_MAX)
    return BNN_ERR_SHAPE;
  const long tiles_m = (a->batch + kT - 1) / kT, tiles_n = (a->out_features + kT - 1) / kT;
  const long total = tiles_m * tiles_n * a->members;
  if (total > 0x3fffffff || (long)a->members * a->batch * a->out_features > ((long)1 << 40)) return BNN_ERR_SHAPE;
  if (a->math != BNN_MATH_F32 && a->math != BNN_MATH_BF16 && a->math != BNN_MATH_BF16X3) return BNN_ERR_ENUM;
  if ((a->x_dtype != BNN_F32 && a->x_dtype != BNN_BF16) || (a->y_dtype != BNN_F32 && a->y_dtype != BNN_BF16)) return BNN_ERR_ENUM;
  const bool bf16 = a->math == BNN_MATH_BF16;
  if (!bf16 && (a->x_dtype != BNN_F32 || a->y_dtype != BNN_F32)) return BNN_ERR_ENUM;
  if (!a->x || !a->w || !a->y) return BNN_ERR_NULL;
  const int xb = a->x_dtype == BNN_BF16 ? 2 : 4, yb = a->y_dtype == BNN_BF16 ? 2 : 4;
  if (misaligned(a->x, xb) || misaligned(a->w, 4) || misaligned(a->b, 4) || misaligned(a->y, yb)) return BNN_ERR_ALIGN;
  BankK k;
  k.x = a->x; k.w = a->w; k.b = a->b; k.y = a->y;
  k.w_stride = a->w_stride; k.b_stride = a->b_stride;
  k.M = a->members; k.first = a->first; k.B = a->batch; k.N = a->out_features; k.K = a->in_features;
  k.tiles_m = (int)tiles_m; k.tiles_n = (int)tiles_n; k.total = (int)total;
  k.x_shared = a->x_shared ? 1 : 0; k.relu = a->relu ? 1 : 0;
  // vector accesses: 8 consecutive elements of a row from a 16-byte aligned address, in every member
  k.vec_x = a->in_features % (16 / xb) == 0 && !misaligned(a->x, 16);
  k.vec_w = a->in_features % 4 == 0 && a->w_stride % 4 == 0 && !misaligned(a->w, 16);
  k.vec_y = a->out_features % 4 == 0 && !misaligned(a->y, 4 * yb);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream_);
  const bool xb16 = a->x_dtype == BNN_BF16, yb16 = a->y_dtype == BNN_BF16;
  if (!bf16) launch_bank<float, float, float>(k, st);
  else if (xb16 && yb16) launch_bank<__bf16, __bf16, __bf16>(k, st);
  else if (xb16) launch_bank<__bf16, __bf16, float>(k, st);
  else if (yb16) launch_bank<__bf16, float, __bf16>(k, st);
  else launch_bank<__bf16, float, float>(k, st);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}
