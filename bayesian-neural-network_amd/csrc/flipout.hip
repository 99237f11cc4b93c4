// F16: the Flipout estimator (include/bnn_hip.h F16).  One base draw Delta_d = sigma o eps_d per layer and draw; every batch
// row sees it through its own rank-one sign pattern, so S samples of a minibatch cost D <= S passes of the Philox / Box-Muller
// generator and plain shared-weight products over the stacked rows.
//
//   bnn_flipout_signs    the sign map, materialised (tests and tools).
//   bnn_flipout_prepare  one thread per epsilon group of four weights: (mu, rho) are read and softplus is taken ONCE for all D
//                        draws; Delta, b_d, the bf16 copies and the statistics partials (one entry per wave, no atomics; a
//                        second launch folds them in fp64 in a fixed order).  Bound by its D * 4..6 bytes written per weight.
//   bnn_flipout_fwd      a 4-wave block owns 64 batch rows x 64 outputs and walks a chunk of samples.  Per k-step of 32 the
//                        x tile (plain and r-flipped), the mu tile and the Delta_d tile go through LDS, one 8-element unit per
//                        thread and tile (16-byte loads where the reduction length and the pointers allow); a wave holds eight
//                        fp32 accumulator tiles (mean and perturbation of its 16 outputs x four 16-row tiles).  The r words
//                        of the block's rows are drawn per 128 columns (one Philox call per row) into LDS, the s words once per
//                        sample; the mean tiles of a shared x are computed for the first sample of the chunk only.
//   bnn_flipout_bwd      exact fp32 on the vector unit, one thread per weight / per input-gradient element, 16 x 16 tiles
//                        through LDS, rows in ascending (s, n) order: no atomics, one summation order per shape.
#include "bnn_device.h"
#include "bnn_prior.h"
#include <type_traits>

namespace bnn {
namespace {

constexpr int kFlThreads = 256;
constexpr uint32_t kSignWord3 = 2u;      // counter word 3 of the sign stream (eps streams: 0; bandit / epoch / acquire / BatchBALD: 1)

// eps_global_sample's value (bnn_device.h) as these kernels were built: s % sgrp is a second division sequence, kept with their device code
__device__ __forceinline__ uint32_t fl_gsample(uint32_t base, uint32_t s, uint32_t sgrp, uint32_t stride) {
  return sgrp == 0u ? base + s : base + (s / sgrp) * stride + s % sgrp;
}

// the four sign words of (row, 128-column group)
__device__ __forceinline__ uint4 sign_words(uint32_t row, uint32_t groups_per_row, uint32_t grp, uint32_t gs, uint32_t tensor_id,
                                            uint32_t k0, uint32_t k1) {
  return philox4x32<>(make_uint4(row * groups_per_row + grp, gs, tensor_id, kSignWord3), k0, k1);
}
// 0x80000000 where sign[row, col] = -1, else 0
__device__ __forceinline__ uint32_t sign_mask(uint32_t row, uint32_t cols, uint32_t col, uint32_t gs, uint32_t tensor_id, uint32_t k0,
                                              uint32_t k1) {
  const uint4 w = sign_words(row, (cols + 127u) >> 7, col >> 7, gs, tensor_id, k0, k1);
  const uint32_t b = col & 127u, q = b >> 5;
  const uint32_t word = q == 0u ? w.x : q == 1u ? w.y : q == 2u ? w.z : w.w;
  return ((word >> (b & 31u)) & 1u) << 31;
}
__device__ __forceinline__ float flip(float v, uint32_t mask) { return __uint_as_float(__float_as_uint(v) ^ mask); }

// ---------------------------------------------------------------------------------------------------- signs
__global__ __launch_bounds__(kFlThreads) void flipout_signs_kernel(bnn_flipout_signs_args a, long total) {
  const long i = (long)blockIdx.x * kFlThreads + threadIdx.x;
  if (i >= total) return;
  const long per = (long)a.rows * a.cols;
  const uint32_t smp = (uint32_t)(i / per);
  const long rem = i - (long)smp * per;
  const uint32_t row = (uint32_t)(rem / a.cols), col = (uint32_t)(rem - (long)row * a.cols);
  const uint32_t m = sign_mask(a.row_offset + row, (uint32_t)a.cols, col, a.sample_offset + smp, eps_tensor_id(a.layer_id, (uint32_t)a.kind),
                               (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
  a.out[i] = m ? (int8_t)-1 : (int8_t)1;
}

// ---------------------------------------------------------------------------------------------------- prepare
struct PrepK {
  const float *w_mu, *w_rho, *b_mu, *b_rho, *eps_w, *eps_b;
  float *delta, *b_draw, *eps_w_dump, *eps_b_dump;
  __bf16 *delta_bf16, *mu_bf16;
  float* part;           // [D][entries][3], entries = blocks * waves
  int K, N, D, spd;      // spd = S / D
  int eps_mode, want_stats, gauss;
  uint32_t layer_id, sample_offset, sgrp, sgrp_stride, k0, k1;
  const uint32_t* sample_counter;
  PriorMix mix;
};

__global__ __launch_bounds__(kFlThreads) void flipout_prepare_kernel(PrepK p) {
  const int K = p.K, N = p.N;
  const int gpr = (K + 3) >> 2;
  const long gw = (long)N * gpr, gb = (N + 3) >> 2;
  const long item = (long)blockIdx.x * kFlThreads + threadIdx.x;
  const bool is_w = item < gw, is_b = !is_w && item < gw + gb;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t base = p.sample_offset + (p.sample_counter ? *p.sample_counter : 0u);
  // the (up to) four parameters of this thread's epsilon group
  int row = 0, col = 0, cnt = 0;
  uint32_t grp = 0;
  const float *mu_p = p.w_mu, *rho_p = p.w_rho;
  if (is_w) {
    row = (int)(item / gpr);
    col = (int)(item - (long)row * gpr) << 2;
    grp = (uint32_t)item;
    cnt = min(4, K - col);
  } else if (is_b) {
    col = (int)(item - gw) << 2;
    grp = (uint32_t)(item - gw);
    cnt = min(4, N - col);
    mu_p = p.b_mu;
    rho_p = p.b_rho;
  }
  const size_t off = is_w ? (size_t)row * K + col : (size_t)col;     // element offset inside one [out, in] / [out] tensor
  const size_t per = is_w ? (size_t)N * K : (size_t)N;
  float mu[4] = {0.f, 0.f, 0.f, 0.f}, sg[4] = {0.f, 0.f, 0.f, 0.f};
  float s_ls = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (j < cnt) {
      mu[j] = mu_p[off + j];
      sg[j] = softplus(rho_p[off + j]);
      s_ls = add_log(s_ls, sg[j]);
      if (is_w && p.mu_bf16) p.mu_bf16[off + j] = (__bf16)mu[j];
    }
  const float ls_wave = p.want_stats ? wave_sum(s_ls) : 0.f;
  const uint32_t tid = eps_tensor_id(p.layer_id, is_w ? kEpsWeight : kEpsBias);
  const long entries = (long)gridDim.x * (kFlThreads / 64);
#pragma unroll 1
  for (int d = 0; d < p.D; ++d) {
    float e[4] = {0.f, 0.f, 0.f, 0.f};
    if (p.eps_mode == BNN_EPS_PHILOX) {
      const uint32_t gs = fl_gsample(base, (uint32_t)(d * p.spd), p.sgrp, p.sgrp_stride);
      philox_normal4(grp, gs, tid, p.k0, p.k1, e);
    } else if (p.eps_mode == BNN_EPS_MEMORY) {
      const float* src = is_w ? p.eps_w : p.eps_b;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < cnt) e[j] = src[(size_t)d * per + off + j];
    }
    float s_e2 = 0.f, s_a = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j >= cnt) continue;
      const float w = __builtin_fmaf(sg[j], e[j], mu[j]);
      s_e2 = __builtin_fmaf(e[j], e[j], s_e2);
      s_a = p.gauss ? __builtin_fmaf(w, w, s_a) : add_log(s_a, prior_mix_p(p.mix, w));
      const size_t o = (size_t)d * per + off + j;
      if (is_w) {
        const float dl = __fmul_rn(sg[j], e[j]);
        p.delta[o] = dl;
        if (p.delta_bf16) p.delta_bf16[o] = (__bf16)dl;
        if (p.eps_w_dump) p.eps_w_dump[o] = e[j];
      } else {
        p.b_draw[o] = w;
        if (p.eps_b_dump) p.eps_b_dump[o] = e[j];
      }
    }
    if (p.want_stats) {                                  // (uniform: every lane of every wave takes part)
      const float a0 = wave_sum(s_e2), a1 = wave_sum(s_a);
      if (lane == 0) {
        float* q = p.part + ((size_t)d * entries + (size_t)blockIdx.x * (kFlThreads / 64) + wave) * 3;
        q[0] = a0;
        q[1] = a1;
        q[2] = ls_wave;
      }
    }
  }
}

// one block per draw: the entries in a fixed order (thread t takes t, t + 256, ...; then a tree over the threads), fp64
__global__ __launch_bounds__(kFlThreads) void flipout_fold_kernel(const float* __restrict__ part, long entries, int gauss, double cnt_c0,
                                                                  double lp_const, double inv2var, float* __restrict__ log_prior,
                                                                  float* __restrict__ log_q) {
  __shared__ double red[3][kFlThreads];
  const int d = blockIdx.x, t = threadIdx.x;
  double r[3] = {0.0, 0.0, 0.0};
  for (long i = t; i < entries; i += kFlThreads) {
    const float* q = part + ((size_t)d * entries + i) * 3;
    r[0] += (double)q[0];
    r[1] += (double)q[1];
    r[2] += (double)q[2];
  }
  for (int j = 0; j < 3; ++j) red[j][t] = r[j];
  __syncthreads();
  for (int w = kFlThreads / 2; w > 0; w >>= 1) {
    if (t < w)
      for (int j = 0; j < 3; ++j) red[j][t] += red[j][t + w];
    __syncthreads();
  }
  if (t == 0) {
    log_q[d] = (float)fold_log_q(cnt_c0, red[2][0], red[0][0]);
    log_prior[d] = (float)fold_log_p(gauss ? BNN_PRIOR_GAUSS : BNN_PRIOR_MIXTURE, lp_const, inv2var, red[1][0]);
  }
}

// ---------------------------------------------------------------------------------------------------- forward
struct FwdK {
  const void* x;
  const void *mu, *delta;      // fp32 (f32 math) or bf16 (bf16 math): [out, in], [D, out, in]
  const float* b_draw;
  void* y;
  int S, D, B, K, N;
  int x_bf16, x_per_sample, y_bf16, relu, zero;
  int chunk;                   // samples a block walks
  int g128;                    // ceil(K / 128)
  int vec;                     // K % 8 == 0 and x, mu, Delta 16-byte aligned: 16-byte loads
  uint32_t layer_id, sample_offset, sgrp, sgrp_stride, row_offset, k0, k1;
  const uint32_t* sample_counter;
};

// eight consecutive elements of a row as floats (bf16 -> fp32 is exact): one or two 16-byte loads where `vec`, else one by
// one with the tail past `n_ok` left zero
__device__ __forceinline__ void load8(const void* base, bool bf16, size_t idx, int n_ok, bool vec, float v[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = 0.f;
  if (n_ok <= 0) return;
  if (vec) {                                                          // (n_ok == 8: the reduction length is a multiple of 8)
    if (bf16) {
      const bf16x8 h = *reinterpret_cast<const bf16x8*>(static_cast<const __bf16*>(base) + idx);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (float)h[j];
    } else {
      const float4 a = *reinterpret_cast<const float4*>(static_cast<const float*>(base) + idx);
      const float4 b = *reinterpret_cast<const float4*>(static_cast<const float*>(base) + idx + 4);
      v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (j < n_ok) v[j] = bf16 ? (float)static_cast<const __bf16*>(base)[idx + j] : static_cast<const float*>(base)[idx + j];
}
// ... into an LDS row: fp32 as is, or rounded to bf16 (RNE; exact for values that were bf16) as one 16-byte store; `flips`:
// bit j set = element j changes sign
template <bool BF16>
__device__ __forceinline__ void store8(void* dst, const float v[8], uint32_t flips) {
  if constexpr (BF16) {
    bf16x8 h;
#pragma unroll
    for (int j = 0; j < 8; ++j) h[j] = (__bf16)flip(v[j], ((flips >> j) & 1u) << 31);
    *reinterpret_cast<bf16x8*>(dst) = h;
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) static_cast<float*>(dst)[j] = flip(v[j], ((flips >> j) & 1u) << 31);
  }
}

constexpr int kFwdRows = 64;                              // batch rows of a block: four 16-row MFMA tiles per wave
template <bool BF16>
__global__ __launch_bounds__(kFlThreads) void flipout_fwd_kernel(FwdK p) {
  using T = typename std::conditional<BF16, uint16_t, float>::type;
  constexpr int KS = BF16 ? 40 : 33;                      // LDS row stride: 16-byte aligned rows (bf16) / odd (fp32: no bank conflicts)
  __shared__ __align__(16) T xs[kFwdRows * KS];           // x
  __shared__ __align__(16) T xrs[kFwdRows * KS];          // x o r
  __shared__ __align__(16) T ms[64 * KS];                 // mu
  __shared__ __align__(16) T dls[64 * KS];                // Delta_d
  __shared__ uint32_t sR[kFwdRows * 4];                   // r words of the current 128-column group
  __shared__ uint32_t sS[kFwdRows * 4];                   // s words of this block's 128-output group
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, q = lane >> 4;
  const int K = p.K, N = p.N, B = p.B;
  const int o_blk = blockIdx.x * 64, n0 = blockIdx.y * kFwdRows;
  const int s_begin = blockIdx.z * p.chunk, s_end = min(p.S, s_begin + p.chunk);
  const uint32_t base = p.sample_offset + (p.sample_counter ? *p.sample_counter : 0u);
  const int spd = p.S / p.D;
  const bool vec = p.vec != 0;
  const int urow = tid >> 2, ukq = tid & 3;               // staging: thread -> (tile row, 8-element unit of the k-step)
  f32x4 accM[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) accM[m] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
  for (int s = s_begin; s < s_end; ++s) {
    const int d = s / spd;
    const bool need_mean = p.x_per_sample || s == s_begin;            // block-uniform
    const uint32_t gs = fl_gsample(base, (uint32_t)s, p.sgrp, p.sgrp_stride);
    __syncthreads();                                                  // the previous sample's epilogue has read sS
    if (!p.zero && tid < kFwdRows) {
      const uint4 w = sign_words(p.row_offset + (uint32_t)(n0 + tid), (uint32_t)((N + 127) >> 7), (uint32_t)(o_blk >> 7), gs,
                                 eps_tensor_id(p.layer_id, kEpsBias), p.k0, p.k1);
      uint32_t* o = sS + tid * 4;
      o[0] = w.x; o[1] = w.y; o[2] = w.z; o[3] = w.w;
    }
    if (need_mean) {
#pragma unroll
      for (int m = 0; m < 4; ++m) accM[m] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    f32x4 accP[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) accP[m] = f32x4{0.f, 0.f, 0.f, 0.f};
    const size_t xrow0 = p.x_per_sample ? (size_t)s * B : 0;
#pragma unroll 1
    for (int k0 = 0; k0 < K; k0 += 32) {
      // (every thread is past the previous k-step's staging, the only reader of sR: its words may be replaced here)
      if (!p.zero && (k0 & 127) == 0 && tid < kFwdRows) {
        const uint4 w = sign_words(p.row_offset + (uint32_t)(n0 + tid), (uint32_t)p.g128, (uint32_t)(k0 >> 7), gs, eps_tensor_id(p.layer_id, kEpsWeight), p.k0, p.k1);
        uint32_t* o = sR + tid * 4;
        o[0] = w.x; o[1] = w.y; o[2] = w.z; o[3] = w.w;
      }
      __syncthreads();                                                // sign words written; the previous k-step's fragments read
      const int k = k0 + 8 * ukq;
      const int n_ok = min(8, K - k);
      float v[8];
      {                                                               // x tile: 64 rows x 32, plain and r-flipped
        const int n = n0 + urow;
        load8(p.x, BF16 && p.x_bf16, (xrow0 + n) * K + k, n < B ? n_ok : 0, vec, v);
        store8<BF16>(xs + urow * KS + 8 * ukq, v, 0u);
        if (!p.zero) store8<BF16>(xrs + urow * KS + 8 * ukq, v, (sR[urow * 4 + ((k0 >> 5) & 3)] >> (8 * ukq)) & 0xffu);
      }
      {                                                               // mu and Delta_d tiles: 64 outputs x 32
        const int o = o_blk + urow;
        const size_t idx = (size_t)o * K + k;
        if (need_mean) {
          load8(p.mu, BF16, idx, o < N ? n_ok : 0, vec, v);
          store8<BF16>(ms + urow * KS + 8 * ukq, v, 0u);
        }
        if (!p.zero) {
          load8(p.delta, BF16, (size_t)d * N * K + idx, o < N ? n_ok : 0, vec, v);
          store8<BF16>(dls + urow * KS + 8 * ukq, v, 0u);
        }
      }
      __syncthreads();
      if constexpr (BF16) {
        const bf16x8 b = *reinterpret_cast<const bf16x8*>(ms + (16 * wave + c) * KS + 8 * q);
        const bf16x8 bd = *reinterpret_cast<const bf16x8*>(dls + (16 * wave + c) * KS + 8 * q);
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          if (need_mean)
            accM[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8*>(xs + (16 * m + c) * KS + 8 * q), b, accM[m], 0, 0, 0);
          if (!p.zero)
            accP[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8*>(xrs + (16 * m + c) * KS + 8 * q), bd, accP[m], 0, 0, 0);
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float b = ms[(16 * wave + c) * KS + 4 * j + q], bd = dls[(16 * wave + c) * KS + 4 * j + q];
#pragma unroll
          for (int m = 0; m < 4; ++m) {
            if (need_mean) accM[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(xs[(16 * m + c) * KS + 4 * j + q], b, accM[m], 0, 0, 0);
            if (!p.zero) accP[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(xrs[(16 * m + c) * KS + 4 * j + q], bd, accP[m], 0, 0, 0);
          }
        }
      }
    }
    // epilogue: lane (c, q) holds rows 16 m + 4 q + v of output column c of the wave's tile
    const int o = o_blk + 16 * wave + c;
    if (o < N) {
      const float bias = p.b_draw[(size_t)(p.zero ? 0 : d) * N + o];
      const int ob = o & 127;
#pragma unroll
      for (int m = 0; m < 4; ++m) {
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int row = 16 * m + 4 * q + v, n = n0 + row;
          if (n >= B) continue;
          float pert = 0.f;
          if (!p.zero) pert = flip(accP[m][v], ((sS[row * 4 + (ob >> 5)] >> (ob & 31)) & 1u) << 31);
          float r = (accM[m][v] + pert) + bias;
          if (p.relu) r = r > 0.f ? r : 0.f;
          const size_t idx = ((size_t)s * B + n) * N + o;
          if (p.y_bf16) static_cast<__bf16*>(p.y)[idx] = (__bf16)r;
          else static_cast<float*>(p.y)[idx] = r;
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------- backward
struct BwdK {
  const float *x, *gy, *y, *w_mu, *w_rho, *b_mu, *b_rho, *eps_w, *eps_b, *glp, *glq;
  float *g_w_mu, *g_w_rho, *g_b_mu, *g_b_rho, *g_x;
  float *gz, *gzs, *xr;        // workspace: [S, B, N], [S, B, N], [S, B, K]
  int S, D, B, K, N, x_per_sample, relu;
  uint32_t layer_id, sample_offset, sgrp, sgrp_stride, row_offset, k0, k1;
  const uint32_t* sample_counter;
  int prior_kind;
  float inv_var_p, a1, a2, inv2var1, inv2var2, invvar1, invvar2;
};

// (1) gz = gy o (y > 0), gz o s, x o r
__global__ __launch_bounds__(kFlThreads) void flipout_bwd_flip_kernel(BwdK p) {
  const long e1 = (long)p.S * p.B * p.N, e2 = (long)p.S * p.B * p.K;
  const long i = (long)blockIdx.x * kFlThreads + threadIdx.x;
  if (i >= e1 + e2) return;
  const uint32_t base = p.sample_offset + (p.sample_counter ? *p.sample_counter : 0u);
  if (i < e1) {
    const long sn = i / p.N;
    const uint32_t o = (uint32_t)(i - sn * p.N), s = (uint32_t)(sn / p.B), n = (uint32_t)(sn - (long)s * p.B);
    float g = p.gy[i];
    if (p.relu && !(p.y[i] > 0.f)) g = 0.f;
    p.gz[i] = g;
    p.gzs[i] = flip(g, sign_mask(p.row_offset + n, (uint32_t)p.N, o, fl_gsample(base, s, p.sgrp, p.sgrp_stride), eps_tensor_id(p.layer_id, kEpsBias),
                                 p.k0, p.k1));
  } else {
    const long j = i - e1, sn = j / p.K;
    const uint32_t k = (uint32_t)(j - sn * p.K), s = (uint32_t)(sn / p.B), n = (uint32_t)(sn - (long)s * p.B);
    const float v = p.x[p.x_per_sample ? j : (long)n * p.K + k];
    p.xr[j] = flip(v, sign_mask(p.row_offset + n, (uint32_t)p.K, k, fl_gsample(base, s, p.sgrp, p.sgrp_stride), eps_tensor_id(p.layer_id, kEpsWeight), p.k0, p.k1));
  }
}

// (2) one thread per weight (tx -> k, ty -> o); the threads tx == 0 of the blocks blockIdx.x == 0 also carry their output's bias
__global__ __launch_bounds__(256) void flipout_bwd_w_kernel(BwdK p) {
  __shared__ float gzt[16][17], gzst[16][17], xt[16][17], xrt[16][17];
  const int tx = threadIdx.x, ty = threadIdx.y;
  const int k0 = blockIdx.x * 16, o0 = blockIdx.y * 16;
  const int k = k0 + tx, o = o0 + ty;
  const int K = p.K, N = p.N, B = p.B, spd = p.S / p.D;
  const bool valid = k < K && o < N;
  const bool bias_thread = blockIdx.x == 0 && tx == 0 && o < N;
  float mu = 0.f, rho = 0.f, sg = 1.f;
  if (valid) {
    mu = p.w_mu[(size_t)o * K + k];
    rho = p.w_rho[(size_t)o * K + k];
    sg = softplus(rho);
  }
  float bmu = 0.f, brho = 0.f, bsg = 1.f;
  if (bias_thread) {
    bmu = p.b_mu[o];
    brho = p.b_rho[o];
    bsg = softplus(brho);
  }
  float G = 0.f, pri = 0.f, racc = 0.f, glq_sum = 0.f;
  float bG = 0.f, bracc = 0.f;
#pragma unroll 1
  for (int d = 0; d < p.D; ++d) {
    float H = 0.f, cs = 0.f;
#pragma unroll 1
    for (int s = d * spd; s < (d + 1) * spd; ++s) {
      const size_t xrow0 = p.x_per_sample ? (size_t)s * B : 0;
#pragma unroll 1
      for (int nb = 0; nb < B; nb += 16) {
        __syncthreads();
        const int n = nb + ty;                              // staging: thread (ty, tx) loads row ty, column tx of each tile
        const bool nok = n < B;
        const size_t go = ((size_t)s * B + n) * N + o0 + tx;
        gzt[ty][tx] = (nok && o0 + tx < N) ? p.gz[go] : 0.f;
        gzst[ty][tx] = (nok && o0 + tx < N) ? p.gzs[go] : 0.f;
        xt[ty][tx] = (nok && k < K) ? p.x[(xrow0 + n) * K + k] : 0.f;
        xrt[ty][tx] = (nok && k < K) ? p.xr[((size_t)s * B + n) * K + k] : 0.f;
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          G = __builtin_fmaf(gzt[r][ty], xt[r][tx], G);
          H = __builtin_fmaf(gzst[r][ty], xrt[r][tx], H);
          cs += gzt[r][ty];
        }
      }
    }
    const float glp = p.glp ? p.glp[d] : 0.f;
    glq_sum += p.glq ? p.glq[d] : 0.f;
    if (valid) {
      const float e = p.eps_w[((size_t)d * N + o) * K + k];
      const float pr = glp * prior_dlogp(p, __builtin_fmaf(sg, e, mu));
      pri += pr;
      racc = __builtin_fmaf(H + pr, e, racc);
    }
    if (bias_thread) {
      const float e = p.eps_b[(size_t)d * N + o];
      const float t = cs + glp * prior_dlogp(p, __builtin_fmaf(bsg, e, bmu));
      bG += t;
      bracc = __builtin_fmaf(t, e, bracc);
    }
  }
  if (valid) {
    p.g_w_mu[(size_t)o * K + k] = G + pri;
    p.g_w_rho[(size_t)o * K + k] = (racc - glq_sum / sg) * sigmoidf(rho);
  }
  if (bias_thread) {
    p.g_b_mu[o] = bG;
    p.g_b_rho[o] = (bracc - glq_sum / bsg) * sigmoidf(brho);
  }
}

// (3) g_x[s, n, k] = sum_o gz mu + r * sum_o (gz o s) Delta_d   (tx -> k, ty -> n; grid.z = sample)
__global__ __launch_bounds__(256) void flipout_bwd_x_kernel(BwdK p) {
  __shared__ float gzt[16][17], gzst[16][17], mt[16][17], dt[16][17];
  const int tx = threadIdx.x, ty = threadIdx.y;
  const int k = blockIdx.x * 16 + tx, n = blockIdx.y * 16 + ty, s = blockIdx.z;
  const int K = p.K, N = p.N, B = p.B;
  const int d = s / (p.S / p.D);
  float a1 = 0.f, a2 = 0.f;
#pragma unroll 1
  for (int o0 = 0; o0 < N; o0 += 16) {
    __syncthreads();
    const bool gok = n < B && o0 + tx < N;
    const size_t go = ((size_t)s * B + n) * N + o0 + tx;
    gzt[ty][tx] = gok ? p.gz[go] : 0.f;
    gzst[ty][tx] = gok ? p.gzs[go] : 0.f;
    const int o = o0 + ty;                                   // weight tiles: row ty = output, column tx = k
    float m = 0.f, dl = 0.f;
    if (o < N && k < K) {
      const size_t wi = (size_t)o * K + k;
      m = p.w_mu[wi];
      dl = __fmul_rn(softplus(p.w_rho[wi]), p.eps_w[(size_t)d * N * K + wi]);
    }
    mt[ty][tx] = m;
    dt[ty][tx] = dl;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      a1 = __builtin_fmaf(gzt[ty][j], mt[j][tx], a1);
      a2 = __builtin_fmaf(gzst[ty][j], dt[j][tx], a2);
    }
  }
  if (n < B && k < K) {
    const uint32_t base = p.sample_offset + (p.sample_counter ? *p.sample_counter : 0u);
    const uint32_t m = sign_mask(p.row_offset + (uint32_t)n, (uint32_t)K, (uint32_t)k, fl_gsample(base, (uint32_t)s, p.sgrp, p.sgrp_stride),
                                 eps_tensor_id(p.layer_id, kEpsWeight), p.k0, p.k1);
    p.g_x[((size_t)s * B + n) * K + k] = a1 + flip(a2, m);
  }
}

bool bad_features(int v) { return v < 1 || v > BNN_FLIPOUT_MAX_FEATURES; }
long prepare_blocks(int K, int N) {
  const long items = (long)N * ((K + 3) >> 2) + ((N + 3) >> 2);
  return (items + kFlThreads - 1) / kFlThreads;
}

}  // namespace
}  // namespace bnn

using namespace bnn;

extern "C" int bnn_flipout_signs(const bnn_flipout_signs_args* a, void* stream_) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_flipout_signs_args)) return BNN_ERR_ABI;
  if (a->n_samples < 1 || a->rows < 1 || a->cols < 1) return BNN_ERR_SHAPE;
  const long total = (long)a->n_samples * a->rows * a->cols;
  if (total > (1L << 40)) return BNN_ERR_SHAPE;
  if ((unsigned)a->kind > 1u) return BNN_ERR_ENUM;
  if (!a->out) return BNN_ERR_NULL;
  const long blocks = (total + kFlThreads - 1) / kFlThreads;
  if (blocks > 0x7fffffffL) return BNN_ERR_SHAPE;
  hipLaunchKernelGGL(flipout_signs_kernel, dim3((unsigned)blocks), dim3(kFlThreads), 0, reinterpret_cast<hipStream_t>(stream_), *a, total);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}

extern "C" size_t bnn_flipout_prepare_workspace_bytes(int32_t n_draws, int32_t in_features, int32_t out_features) {
  if (n_draws < 1 || bad_features(in_features) || bad_features(out_features)) return 0;
  return (size_t)n_draws * (size_t)prepare_blocks(in_features, out_features) * (kFlThreads / 64) * 3 * sizeof(float);
}

extern "C" int bnn_flipout_prepare(const bnn_flipout_prepare_args* a, void* stream_) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_flipout_prepare_args)) return BNN_ERR_ABI;
  if (a->n_samples < 1 || a->n_draws < 1 || a->n_samples % a->n_draws != 0 || bad_features(a->in_features) ||
      bad_features(a->out_features))
    return BNN_ERR_SHAPE;
  if (a->want_stats && prior_check(a->prior) == BNN_ERR_SHAPE) return BNN_ERR_SHAPE;
  if ((unsigned)a->eps_mode > 2u || (a->math != BNN_MATH_F32 && a->math != BNN_MATH_BF16) || prior_check(a->prior) == BNN_ERR_ENUM)
    return BNN_ERR_ENUM;
  const bool bf16 = a->math == BNN_MATH_BF16, mem = a->eps_mode == BNN_EPS_MEMORY;
  if (!a->w_mu || !a->w_rho || !a->b_mu || !a->b_rho || !a->delta || !a->b_draw || (mem && (!a->eps_w || !a->eps_b)) ||
      (bf16 && (!a->delta_bf16 || !a->mu_bf16)) || (a->want_stats && (!a->log_prior || !a->log_q)))
    return BNN_ERR_NULL;
  const size_t need = bnn_flipout_prepare_workspace_bytes(a->n_draws, a->in_features, a->out_features);
  if (a->want_stats && (!a->workspace || a->workspace_bytes < need)) return BNN_ERR_WORKSPACE;
  const void* f32s[] = {a->w_mu, a->w_rho, a->b_mu, a->b_rho, a->eps_w, a->eps_b, a->delta, a->b_draw, a->log_prior, a->log_q,
                        a->eps_w_dump, a->eps_b_dump, a->sample_counter};
  for (const void* q : f32s)
    if (misaligned(q, 4)) return BNN_ERR_ALIGN;
  if (misaligned(a->delta_bf16, 2) || misaligned(a->mu_bf16, 2) || (a->want_stats && misaligned(a->workspace, 8))) return BNN_ERR_ALIGN;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  PrepK k;
  k.w_mu = a->w_mu; k.w_rho = a->w_rho; k.b_mu = a->b_mu; k.b_rho = a->b_rho; k.eps_w = a->eps_w; k.eps_b = a->eps_b;
  k.delta = a->delta; k.b_draw = a->b_draw; k.eps_w_dump = a->eps_w_dump; k.eps_b_dump = a->eps_b_dump;
  k.delta_bf16 = bf16 ? static_cast<__bf16*>(a->delta_bf16) : nullptr;
  k.mu_bf16 = bf16 ? static_cast<__bf16*>(a->mu_bf16) : nullptr;
  k.part = static_cast<float*>(a->workspace);
  k.K = a->in_features; k.N = a->out_features; k.D = a->n_draws; k.spd = a->n_samples / a->n_draws;
  k.eps_mode = a->eps_mode; k.want_stats = a->want_stats ? 1 : 0; k.gauss = a->prior.kind == BNN_PRIOR_GAUSS;
  k.layer_id = a->layer_id; k.sample_offset = a->sample_offset; k.sgrp = a->sample_group; k.sgrp_stride = a->sample_group_stride;
  k.k0 = (uint32_t)a->seed; k.k1 = (uint32_t)(a->seed >> 32);
  k.sample_counter = a->sample_counter;
  k.mix = PriorMix{};
  if (a->want_stats && a->prior.kind == BNN_PRIOR_MIXTURE) k.mix = prior_mix_make(a->prior);
  const long blocks = prepare_blocks(a->in_features, a->out_features);
  hipLaunchKernelGGL(flipout_prepare_kernel, dim3((unsigned)blocks), dim3(kFlThreads), 0, stream, k);
  if (a->want_stats) {
    const PriorFold f = prior_fold_make(a->prior, (double)a->out_features * a->in_features + a->out_features);
    hipLaunchKernelGGL(flipout_fold_kernel, dim3((unsigned)a->n_draws), dim3(kFlThreads), 0, stream, k.part, blocks * (kFlThreads / 64),
                       k.gauss, f.cnt_c0, f.lp_const, f.inv2var, a->log_prior, a->log_q);
  }
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}

extern "C" int bnn_flipout_fwd(const bnn_flipout_fwd_args* a, void* stream_) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_flipout_fwd_args)) return BNN_ERR_ABI;
  const bool zero = a->eps_mode == BNN_EPS_ZERO;
  if (a->n_samples < 1 || a->n_draws < 1 || a->batch < 1 || a->n_samples % a->n_draws != 0 || bad_features(a->in_features) ||
      bad_features(a->out_features) || (unsigned)a->x_per_sample > 1u || (zero && a->n_samples != 1))
    return BNN_ERR_SHAPE;
  if ((a->math != BNN_MATH_F32 && a->math != BNN_MATH_BF16) || (unsigned)a->eps_mode > 2u || (unsigned)a->x_dtype > 1u ||
      (unsigned)a->y_dtype > 1u)
    return BNN_ERR_ENUM;
  const bool bf16 = a->math == BNN_MATH_BF16;
  if (!bf16 && (a->x_dtype != BNN_F32 || a->y_dtype != BNN_F32)) return BNN_ERR_ENUM;
  const void* mu = bf16 ? a->mu_bf16 : static_cast<const void*>(a->w_mu);
  const void* delta = bf16 ? a->delta_bf16 : static_cast<const void*>(a->delta);
  if (!a->x || !a->y || !a->b_draw || !mu || (!zero && !delta)) return BNN_ERR_NULL;
  if (misaligned(a->x, a->x_dtype == BNN_BF16 ? 2 : 4) || misaligned(a->y, a->y_dtype == BNN_BF16 ? 2 : 4) || misaligned(a->b_draw, 4) ||
      misaligned(mu, bf16 ? 2 : 4) || misaligned(delta, bf16 ? 2 : 4) || misaligned(a->sample_counter, 4))
    return BNN_ERR_ALIGN;
  FwdK k;
  k.x = a->x; k.mu = mu; k.delta = delta; k.b_draw = a->b_draw; k.y = a->y;
  k.S = a->n_samples; k.D = a->n_draws; k.B = a->batch; k.K = a->in_features; k.N = a->out_features;
  k.x_bf16 = a->x_dtype == BNN_BF16; k.x_per_sample = a->x_per_sample; k.y_bf16 = a->y_dtype == BNN_BF16; k.relu = a->relu ? 1 : 0;
  k.zero = zero ? 1 : 0;
  k.g128 = (a->in_features + 127) >> 7;
  k.layer_id = a->layer_id; k.sample_offset = a->sample_offset; k.sgrp = a->sample_group; k.sgrp_stride = a->sample_group_stride;
  k.row_offset = a->row_offset; k.k0 = (uint32_t)a->seed; k.k1 = (uint32_t)(a->seed >> 32);
  k.sample_counter = a->sample_counter;
  // the samples a block walks: all of them once the (row tile, output tile) grid alone fills the chip, else as many chunks as
  // bring the grid to ~1024 blocks.  A pure function of the shape; every chunk forms the mean tile in the same order, so the
  // split changes no bit.
  const int row_tiles = (a->batch + kFwdRows - 1) / kFwdRows;
  const long tiles = (long)((a->out_features + 63) / 64) * row_tiles;
  if (tiles > 0x7fffffffL || row_tiles > 65535) return BNN_ERR_SHAPE;
  long chunks = (1024 + tiles - 1) / tiles;
  if (chunks > a->n_samples) chunks = a->n_samples;
  if (chunks < 1) chunks = 1;
  k.chunk = (int)((a->n_samples + chunks - 1) / chunks);
  const unsigned gz = (unsigned)((a->n_samples + k.chunk - 1) / k.chunk);
  if (gz > 65535u) return BNN_ERR_SHAPE;
  k.vec = (a->in_features % 8 == 0 && !misaligned(a->x, 16) && !misaligned(mu, 16) && !misaligned(delta, 16)) ? 1 : 0;
  const dim3 grid((unsigned)((a->out_features + 63) / 64), (unsigned)row_tiles, gz);
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (bf16) hipLaunchKernelGGL(flipout_fwd_kernel<true>, grid, dim3(kFlThreads), 0, stream, k);
  else hipLaunchKernelGGL(flipout_fwd_kernel<false>, grid, dim3(kFlThreads), 0, stream, k);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}

extern "C" size_t bnn_flipout_bwd_workspace_bytes(int32_t n_samples, int32_t batch, int32_t in_features, int32_t out_features) {
  if (n_samples < 1 || batch < 1 || bad_features(in_features) || bad_features(out_features)) return 0;
  return (size_t)n_samples * batch * (2 * (size_t)out_features + in_features) * sizeof(float);
}

extern "C" int bnn_flipout_bwd(const bnn_flipout_bwd_args* a, void* stream_) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_flipout_bwd_args)) return BNN_ERR_ABI;
  if (a->n_samples < 1 || a->n_draws < 1 || a->batch < 1 || a->n_samples % a->n_draws != 0 || bad_features(a->in_features) ||
      bad_features(a->out_features) || (unsigned)a->x_per_sample > 1u || a->n_samples > 65535)
    return BNN_ERR_SHAPE;
  if (const int rc = prior_check(a->prior)) return rc;
  if (!a->x || !a->gy || !a->w_mu || !a->w_rho || !a->b_mu || !a->b_rho || !a->eps_w || !a->eps_b || !a->g_w_mu || !a->g_w_rho ||
      !a->g_b_mu || !a->g_b_rho || (a->relu && !a->y))
    return BNN_ERR_NULL;
  const size_t need = bnn_flipout_bwd_workspace_bytes(a->n_samples, a->batch, a->in_features, a->out_features);
  if (!a->workspace || a->workspace_bytes < need) return BNN_ERR_WORKSPACE;
  const void* ptrs[] = {a->x, a->gy, a->y, a->w_mu, a->w_rho, a->b_mu, a->b_rho, a->eps_w, a->eps_b, a->g_log_prior, a->g_log_q,
                        a->g_w_mu, a->g_w_rho, a->g_b_mu, a->g_b_rho, a->g_x, a->workspace, a->sample_counter};
  for (const void* q : ptrs)
    if (misaligned(q, 4)) return BNN_ERR_ALIGN;
  BwdK k;
  prior_dlogp_fill(a->prior, k);
  k.x = a->x; k.gy = a->gy; k.y = a->y; k.w_mu = a->w_mu; k.w_rho = a->w_rho; k.b_mu = a->b_mu; k.b_rho = a->b_rho;
  k.eps_w = a->eps_w; k.eps_b = a->eps_b; k.glp = a->g_log_prior; k.glq = a->g_log_q;
  k.g_w_mu = a->g_w_mu; k.g_w_rho = a->g_w_rho; k.g_b_mu = a->g_b_mu; k.g_b_rho = a->g_b_rho; k.g_x = a->g_x;
  const size_t rows = (size_t)a->n_samples * a->batch;
  k.gz = static_cast<float*>(a->workspace);
  k.gzs = k.gz + rows * a->out_features;
  k.xr = k.gzs + rows * a->out_features;
  k.S = a->n_samples; k.D = a->n_draws; k.B = a->batch; k.K = a->in_features; k.N = a->out_features;
  k.x_per_sample = a->x_per_sample; k.relu = a->relu ? 1 : 0;
  k.layer_id = a->layer_id; k.sample_offset = a->sample_offset; k.sgrp = a->sample_group; k.sgrp_stride = a->sample_group_stride;
  k.row_offset = a->row_offset; k.k0 = (uint32_t)a->seed; k.k1 = (uint32_t)(a->seed >> 32);
  k.sample_counter = a->sample_counter;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const long elems = (long)rows * ((long)a->out_features + a->in_features);
  const long fb = (elems + kFlThreads - 1) / kFlThreads;
  if (fb > 0x7fffffffL || (a->batch + 15) / 16 > 65535 || (a->out_features + 15) / 16 > 65535) return BNN_ERR_SHAPE;
  hipLaunchKernelGGL(flipout_bwd_flip_kernel, dim3((unsigned)fb), dim3(kFlThreads), 0, stream, k);
  hipLaunchKernelGGL(flipout_bwd_w_kernel, dim3((unsigned)((a->in_features + 15) / 16), (unsigned)((a->out_features + 15) / 16)),
                     dim3(16, 16), 0, stream, k);
  if (a->g_x)
    hipLaunchKernelGGL(flipout_bwd_x_kernel,
                       dim3((unsigned)((a->in_features + 15) / 16), (unsigned)((a->batch + 15) / 16), (unsigned)a->n_samples), dim3(16, 16),
                       0, stream, k);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}
