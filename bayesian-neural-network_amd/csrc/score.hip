// F12 bnn_mc_score (include/bnn_hip.h F12): the held-out scores of S MC outputs against their targets -- the log posterior
// predictive density, the expected NLL, Brier / top-label reliability bins (classification), RMSE / MAE / the PIT histogram
// (regression) -- accumulated into one small device record.
//   score kernel (every sample read once, fp64 per row, one partial record per block) -> fold (block partials in block order)
//   [-> rows (regression row_lpd / row_nll: the C staged outputs of a row, in order)]
// No floating-point atomics anywhere: a block reduces by a fixed lane and wave order, the fold adds the blocks in index
// order, so a call repeated returns the same bits.
//
// Shape, as predictive.hip: classification is a wave per row (lane c owns classes c, c + 64, ...; the mean probability in a
// register for C <= 64, in a per-wave slot of the workspace beyond), regression a thread per output element along B * C.
// A wave walks kRowsPerWave consecutive rows so that a data set of 10^4 rows folds a few hundred partials, not thousands.
// The kernels are bound by fp64 transcendentals (one exp per logit, one exp + one erfc per regression sample), not by the
// 4 bytes per logit they read.
#include <math.h>

#include "bnn_device.h"
#include "../../include/bnn_hip.h"

namespace bnn {
namespace {

constexpr int kScoreBlock = 256;
constexpr int kScoreWaves = kScoreBlock / kWave;
constexpr int kRowsPerWave = 8;
constexpr int kRowsPerBlock = kScoreWaves * kRowsPerWave;
constexpr int kHeadWords = 8;
constexpr int kMaxWords = kHeadWords + 3 * BNN_SCORE_MAX_BINS;
constexpr double kHalfLog2Pi = -kNegLogSqrt2Pi;
constexpr double kInvSqrt2 = 0.70710678118654752440;

struct ScoreK {
  const float* logits;
  const void* targets;
  float* row_lpd;
  float* row_nll;
  unsigned long long* partial;     // [blocks][words]
  double* scratch;                 // classification C > 64: a mean-probability slot per wave; regression rows: staged lpd, nll
  long n_valid;                    // rows
  int G, S, B, C, n_bins, words;
  double sigma;
};

__device__ __forceinline__ unsigned long long bits(double v) { return (unsigned long long)__double_as_longlong(v); }

// running logsumexp (M, A): sum_s exp(lp_s) = A exp(M).  -inf terms add nothing, a NaN term makes A NaN.
__device__ __forceinline__ void lse_push(double lp, double& M, double& A) {
  if (lp > M) {
    A = A * exp(M - lp) + 1.0;
    M = lp;
  } else if (lp != lp) {
    A = NAN;
  } else if (lp > -INFINITY) {
    A += exp(lp - M);
  }
}

// ----------------------------------------------------------------------------- classification
__global__ __launch_bounds__(kScoreBlock) void mc_score_class_kernel(ScoreK k) {
  __shared__ double s_lpd[kRowsPerBlock], s_nll[kRowsPerBlock], s_brier[kRowsPerBlock], s_conf[kRowsPerBlock];
  __shared__ int s_bin[kRowsPerBlock], s_ok[kRowsPerBlock];      // bin: -2 padding, -1 no bin (NaN row or no bins)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int S = k.S, C = k.C;
  const size_t sstride = (size_t)k.B * C;
  const long long* labels = static_cast<const long long*>(k.targets);
  double* pb = k.scratch ? k.scratch + ((size_t)blockIdx.x * kScoreWaves + wave) * C : nullptr;

#pragma unroll 1
  for (int r = 0; r < kRowsPerWave; ++r) {
    const int slot = wave * kRowsPerWave + r;
    const long row = (long)blockIdx.x * kRowsPerBlock + slot;    // g * B + b
    if (row >= k.n_valid) {                                       // wave-uniform: padding is never loaded
      if (lane == 0) s_bin[slot] = -2;
      continue;
    }
    const long g = row / k.B, b = row - g * k.B;
    const float* base = k.logits + (size_t)g * S * sstride + (size_t)b * C;
    const long long y = labels[row];
    double M = -INFINITY, A = 0.0, nsum = 0.0, brier = 0.0, best = -1.0;
    int bi = 0x7fffffff;
    if (C <= 64) {
      double acc = 0.0;
#pragma unroll 1
      for (int s0 = 0; s0 < S; s0 += 8) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (s0 + j < S && lane < C) ? base[(size_t)(s0 + j) * sstride + lane] : -INFINITY;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          if (s0 + j < S) {                                       // wave-uniform
            const float mx = wave_max(v[j]);
            const double e = lane < C ? exp((double)v[j] - (double)mx) : 0.0;
            const double se = wave_sum(e);
            const unsigned long long hit = __ballot(lane < C && (long long)lane == y);
            double lp = -INFINITY;                                // a label outside [0, C) matches no lane
            if (hit) lp = ((double)__shfl(v[j], __ffsll((long long)hit) - 1, kWave) - (double)mx) - log(se);
            lse_push(lp, M, A);
            nsum += lp;
            acc += e / se;
          }
        }
      }
      if (lane < C) {
        const double pm = acc / (double)S;
        const double t = pm - ((long long)lane == y ? 1.0 : 0.0);
        brier = t * t;
        best = pm;
        bi = lane;
      }
    } else {
      for (int c = lane; c < C; c += 64) pb[c] = 0.0;             // lane c owns pb[c]: no race
#pragma unroll 1
      for (int s = 0; s < S; ++s) {
        const float* lg = base + (size_t)s * sstride;
        float mx = -INFINITY, zy = 0.f;
        bool mine = false;
        for (int c = lane; c < C; c += 64) {
          const float z = lg[c];
          mx = fmaxf(mx, z);
          if ((long long)c == y) {
            zy = z;
            mine = true;
          }
        }
        mx = wave_max(mx);
        double se = 0.0;
        for (int c = lane; c < C; c += 64) se += exp((double)lg[c] - (double)mx);
        se = wave_sum(se);
        const unsigned long long hit = __ballot(mine);
        double lp = -INFINITY;
        if (hit) lp = ((double)__shfl(zy, __ffsll((long long)hit) - 1, kWave) - (double)mx) - log(se);
        lse_push(lp, M, A);
        nsum += lp;
        for (int c = lane; c < C; c += 64) pb[c] += exp((double)lg[c] - (double)mx) / se;
      }
      for (int c = lane; c < C; c += 64) {
        const double pm = pb[c] / (double)S;
        const double t = pm - ((long long)c == y ? 1.0 : 0.0);
        brier += t * t;
        if (pm > best) {
          best = pm;
          bi = c;
        }
      }
    }
    brier = wave_sum(brier);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {                      // argmax, lowest index on ties
      const double ov = __shfl_xor(best, off, kWave);
      const int oi = __shfl_xor(bi, off, kWave);
      if (ov > best || (ov == best && oi < bi)) {
        best = ov;
        bi = oi;
      }
    }
    if (lane == 0) {
      const double lpd = M + log(A) - log((double)S);
      const double nll = -nsum / (double)S;
      const bool nan_row = brier != brier;                        // a NaN logit makes every mean probability NaN
      int bin = -1;
      if (!nan_row && k.n_bins > 0) {
        bin = (int)ceil(best * (double)k.n_bins) - 1;
        bin = bin < 0 ? 0 : (bin > k.n_bins - 1 ? k.n_bins - 1 : bin);
      }
      s_lpd[slot] = lpd;
      s_nll[slot] = nll;
      s_brier[slot] = brier;
      s_conf[slot] = best;
      s_bin[slot] = bin;
      s_ok[slot] = (!nan_row && (long long)bi == y) ? 1 : 0;
      if (k.row_lpd) k.row_lpd[row] = (float)lpd;
      if (k.row_nll) k.row_nll[row] = (float)nll;
    }
  }
  __syncthreads();
  // the block's partial record: its rows in order
  unsigned long long* out = k.partial + (size_t)blockIdx.x * k.words;
  if (tid == 0) {
    long long rows = 0, ok = 0;
    double lpd = 0.0, nll = 0.0, br = 0.0;
    for (int i = 0; i < kRowsPerBlock; ++i) {
      if (s_bin[i] == -2) continue;
      ++rows;
      ok += s_ok[i];
      lpd += s_lpd[i];
      nll += s_nll[i];
      br += s_brier[i];
    }
    out[0] = (unsigned long long)rows;
    out[1] = (unsigned long long)ok;
    out[2] = bits(lpd);
    out[3] = bits(nll);
    out[4] = bits(br);
    out[5] = out[6] = out[7] = 0ull;
  }
  if (tid >= kWave && tid < kWave + k.n_bins) {
    const int bn = tid - kWave;
    long long cnt = 0, ok = 0;
    double cf = 0.0;
    for (int i = 0; i < kRowsPerBlock; ++i) {
      if (s_bin[i] != bn) continue;
      ++cnt;
      ok += s_ok[i];
      cf += s_conf[i];
    }
    out[kHeadWords + 3 * bn] = (unsigned long long)cnt;
    out[kHeadWords + 3 * bn + 1] = (unsigned long long)ok;
    out[kHeadWords + 3 * bn + 2] = bits(cf);
  }
}

// ----------------------------------------------------------------------------- regression
// A thread per output element i = g * (B C) + j, as mc_predictive_moments_kernel: a row's elements are i / C, so the valid
// elements are i < n_valid * C.  Two passes over the S samples: the sums, the smallest exponent and the PIT; then the
// shifted exponentials.
__global__ __launch_bounds__(kScoreBlock) void mc_score_reg_kernel(ScoreK k) {
  __shared__ int s_cnt[BNN_SCORE_MAX_BINS];
  __shared__ double s_sum[4][kScoreWaves];
  __shared__ int s_n[2][kScoreWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int S = k.S;
  const long N = (long)k.B * k.C, total = k.n_valid * k.C;
  const long i = (long)blockIdx.x * kScoreBlock + tid;
  for (int t = tid; t < k.n_bins; t += kScoreBlock) s_cnt[t] = 0;
  __syncthreads();
  double lpd = 0.0, nll = 0.0, sq = 0.0, ab = 0.0;
  int elem = 0, first = 0;
  if (i < total) {
    const long g = i / N, j = i - g * N;
    const float* p = k.logits + (size_t)g * S * N + j;
    const double y = (double)static_cast<const float*>(k.targets)[i];
    const double inv_sig = 1.0 / k.sigma, half_inv_var = 0.5 * inv_sig * inv_sig;
    double fsum = 0.0, qsum = 0.0, qmin = INFINITY, usum = 0.0;
#pragma unroll 1
    for (int s0 = 0; s0 < S; s0 += 8) {
      float v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = s0 + q < S ? p[(size_t)(s0 + q) * N] : 0.f;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        if (s0 + q < S) {
          const double d = y - (double)v[q];
          const double e = d * d * half_inv_var;
          fsum += (double)v[q];
          qsum += e;
          qmin = fmin(qmin, e);
          usum += 0.5 * erfc(-(d * inv_sig) * kInvSqrt2);
        }
      }
    }
    double A = 0.0;
#pragma unroll 1
    for (int s0 = 0; s0 < S; s0 += 8) {
      float v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = s0 + q < S ? p[(size_t)(s0 + q) * N] : 0.f;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        if (s0 + q < S) {
          const double d = y - (double)v[q];
          A += exp(qmin - d * d * half_inv_var);                   // a NaN sample makes A NaN
        }
      }
    }
    const double norm = log(k.sigma) + kHalfLog2Pi;
    lpd = (log(A) - qmin) - log((double)S) - norm;
    nll = qsum / (double)S + norm;
    const double err = y - fsum / (double)S;
    sq = err * err;
    ab = fabs(err);
    const double u = usum / (double)S;
    elem = 1;
    first = (i % k.C) == 0 ? 1 : 0;
    if (k.n_bins > 0 && u == u) {
      int bin = (int)floor(u * (double)k.n_bins);
      bin = bin < 0 ? 0 : (bin > k.n_bins - 1 ? k.n_bins - 1 : bin);
      atomicAdd(&s_cnt[bin], 1);                                  // integer: exact in any order
    }
    if (k.row_lpd || k.row_nll) {                                 // staged for the rows launch
      k.scratch[2 * i] = lpd;
      k.scratch[2 * i + 1] = nll;
    }
  }
  lpd = wave_sum(lpd);
  nll = wave_sum(nll);
  sq = wave_sum(sq);
  ab = wave_sum(ab);
  const int n_elem = __popcll(__ballot(elem)), n_first = __popcll(__ballot(first));
  if (lane == 0) {
    s_sum[0][wave] = lpd;
    s_sum[1][wave] = nll;
    s_sum[2][wave] = sq;
    s_sum[3][wave] = ab;
    s_n[0][wave] = n_first;
    s_n[1][wave] = n_elem;
  }
  __syncthreads();
  unsigned long long* out = k.partial + (size_t)blockIdx.x * k.words;
  if (tid == 0) {
    long long rows = 0, elems = 0;
    double t[4] = {0.0, 0.0, 0.0, 0.0};
    for (int w = 0; w < kScoreWaves; ++w) {                       // waves in order
      rows += s_n[0][w];
      elems += s_n[1][w];
      for (int q = 0; q < 4; ++q) t[q] += s_sum[q][w];
    }
    out[0] = (unsigned long long)rows;
    out[1] = (unsigned long long)elems;
    for (int q = 0; q < 4; ++q) out[2 + q] = bits(t[q]);
    out[6] = out[7] = 0ull;
  }
  for (int t = tid; t < k.n_bins; t += kScoreBlock) {
    out[kHeadWords + 3 * t] = (unsigned long long)s_cnt[t];
    out[kHeadWords + 3 * t + 1] = 0ull;
    out[kHeadWords + 3 * t + 2] = 0ull;
  }
}

// regression row_lpd / row_nll: the C staged values of a row, in order
__global__ __launch_bounds__(kScoreBlock) void mc_score_rows_kernel(ScoreK k) {
  const long row = (long)blockIdx.x * kScoreBlock + threadIdx.x;
  if (row >= k.n_valid) return;
  double lpd = 0.0, nll = 0.0;
  for (int c = 0; c < k.C; ++c) {
    lpd += k.scratch[2 * (row * k.C + c)];
    nll += k.scratch[2 * (row * k.C + c) + 1];
  }
  if (k.row_lpd) k.row_lpd[row] = (float)lpd;
  if (k.row_nll) k.row_nll[row] = (float)nll;
}

// one block: word w of the record = the blocks' word w in block order (words 2 .. 5 and every third bin word are fp64)
__global__ __launch_bounds__(kScoreBlock) void mc_score_fold_kernel(const unsigned long long* __restrict__ partial, int blocks, int words,
                                                                    int accumulate, unsigned long long* __restrict__ record) {
  const int w = threadIdx.x;
  if (w >= words) return;
  const bool f64 = (w >= 2 && w <= 5) || (w >= kHeadWords && (w - kHeadWords) % 3 == 2);
  if (f64) {
    double t = 0.0;
    for (int b = 0; b < blocks; ++b) t += __longlong_as_double((long long)partial[(size_t)b * words + w]);
    if (accumulate) t = __longlong_as_double((long long)record[w]) + t;
    record[w] = bits(t);
  } else {
    unsigned long long t = 0ull;
    for (int b = 0; b < blocks; ++b) t += partial[(size_t)b * words + w];
    record[w] = accumulate ? record[w] + t : t;
  }
}
static_assert(kMaxWords <= kScoreBlock, "the fold is one word per thread");

bool shape_ok(int G, int B, int C) {
  return G > 0 && B > 0 && C > 0 && (int64_t)G * B <= INT32_MAX && (int64_t)B * C <= INT32_MAX && (int64_t)G * B * C <= ((int64_t)1 << 40);
}

size_t class_blocks(int64_t rows) { return (size_t)((rows + kRowsPerBlock - 1) / kRowsPerBlock); }
size_t reg_blocks(int64_t elems) { return (size_t)((elems + kScoreBlock - 1) / kScoreBlock); }

// the partial records of either mode's blocks, then the larger of the two scratch areas
size_t partial_bytes(int G, int B, int C) {
  const size_t cb = class_blocks((int64_t)G * B), rb = reg_blocks((int64_t)G * B * C);
  return (cb > rb ? cb : rb) * kMaxWords * sizeof(unsigned long long);
}
size_t scratch_bytes(int G, int B, int C) {
  const size_t cls = C > 64 ? class_blocks((int64_t)G * B) * kScoreWaves * (size_t)C * sizeof(double) : 0;
  const size_t reg = 2 * (size_t)G * B * C * sizeof(double);
  return cls > reg ? cls : reg;
}

}  // namespace
}  // namespace bnn

using namespace bnn;

extern "C" size_t bnn_mc_score_workspace_bytes(int32_t groups, int32_t batch, int32_t classes) {
  if (!shape_ok(groups, batch, classes)) return 0;
  return partial_bytes(groups, batch, classes) + scratch_bytes(groups, batch, classes);
}

extern "C" int bnn_mc_score(const bnn_mc_score_args* a, void* stream_) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_mc_score_args)) return BNN_ERR_ABI;
  if (a->mode != BNN_NLL_CLASSIFICATION && a->mode != BNN_NLL_REGRESSION) return BNN_ERR_ENUM;
  const int G = a->groups, S = a->n_samples, B = a->batch, C = a->classes;
  if (S <= 0 || !shape_ok(G, B, C)) return BNN_ERR_SHAPE;
  if (a->n_valid < 1 || a->n_valid > (int64_t)G * B) return BNN_ERR_SHAPE;
  if (a->n_bins < 0 || a->n_bins > BNN_SCORE_MAX_BINS) return BNN_ERR_SHAPE;
  const bool cls = a->mode == BNN_NLL_CLASSIFICATION;
  if (!cls && !(a->sigma > 0.f && isfinite(a->sigma))) return BNN_ERR_SHAPE;
  if (!a->logits || !a->targets || !a->record) return BNN_ERR_NULL;
  if (!a->workspace || a->workspace_bytes < bnn_mc_score_workspace_bytes(G, B, C)) return BNN_ERR_NULL;
  if (misaligned(a->record, 8) || misaligned(a->workspace, 8)) return BNN_ERR_ALIGN;
  if (misaligned(a->targets, cls ? 8 : 4)) return BNN_ERR_ALIGN;
  if (misaligned(a->logits, 4) || misaligned(a->row_lpd, 4) || misaligned(a->row_nll, 4)) return BNN_ERR_ALIGN;

  ScoreK k;
  k.logits = a->logits;
  k.targets = a->targets;
  k.row_lpd = a->row_lpd;
  k.row_nll = a->row_nll;
  k.partial = static_cast<unsigned long long*>(a->workspace);
  double* scratch = reinterpret_cast<double*>(static_cast<char*>(a->workspace) + partial_bytes(G, B, C));
  k.n_valid = (long)a->n_valid;
  k.G = G;
  k.S = S;
  k.B = B;
  k.C = C;
  k.n_bins = a->n_bins;
  k.words = kHeadWords + 3 * a->n_bins;
  k.sigma = (double)a->sigma;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  size_t blocks;
  if (cls) {
    k.scratch = C > 64 ? scratch : nullptr;
    blocks = class_blocks(a->n_valid);
    hipLaunchKernelGGL(mc_score_class_kernel, dim3((unsigned)blocks), dim3(kScoreBlock), 0, stream, k);
  } else {
    k.scratch = scratch;
    blocks = reg_blocks(a->n_valid * C);
    hipLaunchKernelGGL(mc_score_reg_kernel, dim3((unsigned)blocks), dim3(kScoreBlock), 0, stream, k);
    if (a->row_lpd || a->row_nll)
      hipLaunchKernelGGL(mc_score_rows_kernel, dim3((unsigned)((a->n_valid + kScoreBlock - 1) / kScoreBlock)), dim3(kScoreBlock), 0,
                         stream, k);
  }
  hipLaunchKernelGGL(mc_score_fold_kernel, dim3(1), dim3(kScoreBlock), 0, stream, k.partial, (int)blocks, k.words,
                     a->accumulate ? 1 : 0, static_cast<unsigned long long*>(a->record));
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}
