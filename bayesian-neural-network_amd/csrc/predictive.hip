// F3 bnn_mc_predictive: the predictive summaries of S MC outputs per (minibatch, row) -- class probabilities, their
// argmax and the entropy decomposition for classification; mean, variance and quantiles for regression (the
// statistics regression/reg_task.py:76-83 + utils/plot_utils.py:8-29 take on the host with numpy).
#include <math.h>

#include "bnn_device.h"
#include "../../include/bnn_hip.h"

namespace bnn {

constexpr int kPredBlock = 256;
constexpr int kQuantLdsFloats = 16384;          // 64 KB: the per-column sorts of one quantile block
constexpr int kQuantMaxCols = 64;

// ----------------------------------------------------------------------------- classification
// One wave per (minibatch g, batch row b), as mc_softmax_mean_kernel (reduce.hip): lane c owns classes c, c + 64, ...;
// the mean probability is kept in registers (C <= 64) and the samples' logits are fetched eight at a time.  Per sample,
// with d_c = z_c - max z and e_c = exp(d_c):
//     p_c = e_c / sum e,      H(p) = logsumexp(z) - sum_c p_c z_c = log(sum e) - sum_c e_c d_c / sum e
// (the shifted form: no log 0, no cancellation against a large max z).
__global__ __launch_bounds__(kPredBlock) void mc_predictive_class_kernel(const float* __restrict__ logits, int G, int S, int B,
                                                                         int C, float scale, float* __restrict__ probs,
                                                                         long long* __restrict__ preds, float* __restrict__ pent,
                                                                         float* __restrict__ eent, float* __restrict__ mi) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * (kPredBlock / 64) + (threadIdx.x >> 6);    // g * B + b
  if (row >= (long)G * B) return;                                                 // wave-uniform
  const long g = row / B, b = row - g * B;
  const size_t sstride = (size_t)B * C;                                           // one sample's [B, C] block
  const float* base = logits + (size_t)g * S * sstride + (size_t)b * C;
  float* out = probs + (size_t)row * C;
  double hsum = 0.0;                                                              // fp64 sums over the samples: S in the
  float best = -1.f, pe = 0.f;                                                    // hundreds stays at fp32 rounding
  int bi = 0x7fffffff;
  if (C <= 64) {
    double acc = 0.0;
    for (int s0 = 0; s0 < S; s0 += 8) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (s0 + j < S && lane < C) ? base[(size_t)(s0 + j) * sstride + lane] : -3.0e38f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (s0 + j < S) {                                                         // wave-uniform
          const float mx = wave_max(v[j]);
          const float d = lane < C ? v[j] - mx : 0.f;
          const float e = lane < C ? expf(d) : 0.f;
          const float se = wave_sum(e);
          const float ed = wave_sum(e * d);
          acc += (double)(e * (scale / se));
          hsum += (double)(logf(se) - ed / se);
        }
      }
    }
    if (lane < C) {
      const float pm = (float)acc;
      out[lane] = pm;
      best = pm;
      bi = lane;
      if (pm > 0.f) pe = -pm * logf(pm);
    }
  } else {
    for (int c = lane; c < C; c += 64) out[c] = 0.f;
    for (int s = 0; s < S; ++s) {
      const float* lg = base + (size_t)s * sstride;
      float mx = -3.0e38f;
      for (int c = lane; c < C; c += 64) mx = fmaxf(mx, lg[c]);
      mx = wave_max(mx);
      float se = 0.f, ed = 0.f;
      for (int c = lane; c < C; c += 64) {
        const float d = lg[c] - mx, e = expf(d);
        se += e;
        ed += e * d;
      }
      se = wave_sum(se);
      ed = wave_sum(ed);
      const float inv = scale / se;
      for (int c = lane; c < C; c += 64) out[c] += expf(lg[c] - mx) * inv;     // lane c owns out[c]: no race
      hsum += (double)(logf(se) - ed / se);
    }
    for (int c = lane; c < C; c += 64) {
      const float v = out[c];
      if (v > best) { best = v; bi = c; }
      if (v > 0.f) pe -= v * logf(v);                                             // 0 log 0 = 0
    }
  }
  const float ee = (float)(scale * hsum);
  if (pent || mi) {                                                               // wave-uniform
    pe = wave_sum(pe);
    if (lane == 0) {
      if (pent) pent[row] = pe;
      if (mi) mi[row] = fmaxf(pe - ee, 0.f);      // >= 0 in exact arithmetic (Jensen); rounding can leave -1e-7
    }
  }
  if (lane == 0) eent[row] = ee;
  if (preds) {                                                                    // argmax, lowest index on ties
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_xor(best, off, 64);
      const int oi = __shfl_xor(bi, off, 64);
      if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    }
    if (lane == 0) preds[row] = bi;
  }
}

// ----------------------------------------------------------------------------- regression: moments
// A thread per output element (g, j), j = b * C + c: lanes run along the contiguous B*C index, so every sample's loads
// coalesce.  Two passes over the S values in fp64 (mean, then sum of squared deviations): never E[y^2] - E[y]^2.
__global__ __launch_bounds__(kPredBlock) void mc_predictive_moments_kernel(const float* __restrict__ logits, int S, long N,
                                                                           long total, double sig2, float* __restrict__ mean,
                                                                           float* __restrict__ var, float* __restrict__ pvar) {
  const long i = (long)blockIdx.x * kPredBlock + threadIdx.x;                     // g * N + j
  if (i >= total) return;
  const long g = i / N, j = i - g * N;
  const float* p = logits + (size_t)g * S * N + j;
  double s1 = 0.0;
  for (int s0 = 0; s0 < S; s0 += 8) {
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = s0 + k < S ? p[(size_t)(s0 + k) * N] : 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) s1 += (double)v[k];
  }
  const double m = s1 / S;
  double m2 = 0.0;
  for (int s0 = 0; s0 < S; s0 += 8) {
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = s0 + k < S ? p[(size_t)(s0 + k) * N] : 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const double d = (double)v[k] - m;
      if (s0 + k < S) m2 += d * d;
    }
  }
  const double vr = m2 / S;                                                       // ddof 0
  mean[i] = (float)m;
  var[i] = (float)vr;
  if (pvar) pvar[i] = (float)(vr + sig2);
}

// ----------------------------------------------------------------------------- regression: quantiles
struct QuantLevels {
  double q[BNN_PREDICTIVE_MAX_QUANTILES];
};

// A block per `cols` consecutive output elements of one minibatch.  The S samples of each column are loaded (column index
// fastest: coalesced) into an LDS segment of spad = next power of two >= S floats, padded with +inf, NaN replaced by +inf
// and flagged; a bitonic sort runs on all segments at once; then every (level, column) is numpy.percentile's linear
// interpolation: pos = q (S - 1), a = v[floor pos], b = v[floor pos + 1], gamma = pos - floor pos,
//     gamma < 0.5:  a + (b - a) gamma      else:  b - (b - a)(1 - gamma)         (numpy's _lerp, b - a in fp32)
// and NaN for a column with any NaN sample.
__global__ __launch_bounds__(kPredBlock) void mc_predictive_quantile_kernel(const float* __restrict__ logits, int S, long N,
                                                                            int spad, int cols, int nq, QuantLevels lv,
                                                                            float* __restrict__ quant, long GN) {
  extern __shared__ float seg[];                                                  // [cols][spad]
  __shared__ int has_nan[kQuantMaxCols];
  const long blocks_per_g = (N + cols - 1) / cols;
  const long g = blockIdx.x / blocks_per_g;
  const long j0 = (blockIdx.x - g * blocks_per_g) * (long)cols;
  const int ncol = (int)((N - j0) < cols ? (N - j0) : cols);
  const int total = cols * spad;
  for (int c = threadIdx.x; c < cols; c += kPredBlock) has_nan[c] = 0;
  __syncthreads();
  const float* src = logits + (size_t)g * S * N + j0;
  for (int e = threadIdx.x; e < total; e += kPredBlock) {
    const int s = e / cols, c = e - s * cols;
    float x = INFINITY;
    if (s < S && c < ncol) {
      x = src[(size_t)s * N + c];
      if (x != x) {
        has_nan[c] = 1;
        x = INFINITY;
      }
    }
    seg[c * spad + s] = x;
  }
  __syncthreads();
  for (int k = 2; k <= spad; k <<= 1) {
    for (int jj = k >> 1; jj > 0; jj >>= 1) {
      for (int e = threadIdx.x; e < (total >> 1); e += kPredBlock) {
        const int i = 2 * jj * (e / jj) + (e % jj);                               // lower element of the pair; partner i + jj
        const bool asc = ((i & (spad - 1)) & k) == 0;                             // position inside its column's segment
        const float x = seg[i], y = seg[i + jj];
        if ((x > y) == asc) {
          seg[i] = y;
          seg[i + jj] = x;
        }
      }
      __syncthreads();
    }
  }
  for (int t = threadIdx.x; t < nq * ncol; t += kPredBlock) {
    const int qi = t / ncol, c = t - qi * ncol;
    const double pos = lv.q[qi] * (double)(S - 1);
    int lo = (int)floor(pos);
    lo = lo < 0 ? 0 : (lo > S - 1 ? S - 1 : lo);
    const int hi = lo + 1 < S ? lo + 1 : S - 1;
    const double gam = pos - (double)lo;
    const float a = seg[c * spad + lo], b = seg[c * spad + hi];
    const float d = b - a;
    const double r = gam < 0.5 ? (double)a + (double)d * gam : (double)b - (double)d * (1.0 - gam);
    quant[(size_t)qi * GN + (size_t)g * N + j0 + c] = has_nan[c] ? NAN : (float)r;
  }
}

}  // namespace bnn

using namespace bnn;

extern "C" int bnn_mc_predictive(const bnn_mc_predictive_args* a, void* stream_) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_mc_predictive_args)) return BNN_ERR_ABI;
  if (a->mode != BNN_NLL_CLASSIFICATION && a->mode != BNN_NLL_REGRESSION) return BNN_ERR_ENUM;
  const int G = a->groups, S = a->n_samples, B = a->batch, C = a->classes;
  if (G <= 0 || S <= 0 || B <= 0 || C <= 0) return BNN_ERR_SHAPE;
  if ((int64_t)G * B > INT32_MAX || (int64_t)B * C > INT32_MAX) return BNN_ERR_SHAPE;
  if (!a->logits) return BNN_ERR_NULL;
  const bool cls = a->mode == BNN_NLL_CLASSIFICATION;
  if (cls) {
    if (!a->probs || !a->expected_entropy) return BNN_ERR_NULL;
    if (!(a->scale > 0.f) || !isfinite(a->scale) || a->n_quantiles != 0) return BNN_ERR_SHAPE;
  } else {
    if (!a->mean || !a->variance) return BNN_ERR_NULL;
    if (a->predictive_variance && !isfinite(a->sigma)) return BNN_ERR_SHAPE;
    if (a->n_quantiles < 0 || a->n_quantiles > BNN_PREDICTIVE_MAX_QUANTILES) return BNN_ERR_SHAPE;
    if (a->n_quantiles > 0) {
      if (!a->quantiles) return BNN_ERR_NULL;
      if (S > BNN_PREDICTIVE_MAX_QUANTILE_SAMPLES) return BNN_ERR_SHAPE;
      for (int i = 0; i < a->n_quantiles; ++i)
        if (!(a->quantile[i] >= 0.0 && a->quantile[i] <= 1.0)) return BNN_ERR_SHAPE;    // NaN fails both
    }
  }
  const void* f32s[] = {a->logits, a->probs, a->predictive_entropy, a->expected_entropy, a->mutual_information,
                        a->mean, a->variance, a->predictive_variance, a->quantiles};
  for (const void* p : f32s)
    if (misaligned(p, 4)) return BNN_ERR_ALIGN;
  if (misaligned(a->preds, 8)) return BNN_ERR_ALIGN;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (cls) {
    const long rows = (long)G * B;
    hipLaunchKernelGGL(mc_predictive_class_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(kPredBlock), 0, stream, a->logits,
                       G, S, B, C, a->scale, a->probs, reinterpret_cast<long long*>(a->preds), a->predictive_entropy, a->expected_entropy,
                       a->mutual_information);
  } else {
    const long N = (long)B * C, total = (long)G * N;
    const double sig = (double)a->sigma;
    hipLaunchKernelGGL(mc_predictive_moments_kernel, dim3((unsigned)((total + kPredBlock - 1) / kPredBlock)), dim3(kPredBlock),
                       0, stream, a->logits, S, N, total, sig * sig, a->mean, a->variance, a->predictive_variance);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return (int)err;
    if (a->n_quantiles > 0) {
      int spad = 1;
      while (spad < S) spad <<= 1;
      int cols = kQuantLdsFloats / spad;
      cols = cols > kQuantMaxCols ? kQuantMaxCols : cols;
      QuantLevels lv{};
      for (int i = 0; i < a->n_quantiles; ++i) lv.q[i] = a->quantile[i];
      const long nb = (long)G * ((N + cols - 1) / cols);
      hipLaunchKernelGGL(mc_predictive_quantile_kernel, dim3((unsigned)nb), dim3(kPredBlock), (size_t)cols * spad * sizeof(float),
                         stream, a->logits, S, N, spad, cols, a->n_quantiles, lv, a->quantiles, total);
    }
  }
  hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}
