// F17 diagonal Laplace posterior of MLP / MLP_Dropout (include/bnn_hip.h): bnn_laplace_seed (the output-layer deltas of the
// GGN / empirical Fisher and the data term), bnn_laplace_layer (one Linear -> [ReLU] group's curvature diagonal and the
// deltas of the layer below, one launch), bnn_laplace_evidence (the Laplace marginal likelihood at every candidate prior
// precision in one pass) and bnn_laplace_posterior ((mu, rho) of a BayesianLinear from (w, F, tau)).
//
// bnn_laplace_layer.  Two products share one grid, as in bnn_dense_bwd: blocks [0, tiles_x) own 64 x 64 tiles of
// g_x [R, in] = gz . W (K = out), the rest 64 x 64 tiles of F_w [out, in] += S^T . x^2 (K = batch) on the exact-fp32 matrix
// core.  The GEMM core is dense_tile.h's; the operands here are formed while they are staged: gz from gy and the saved output
// of data row r mod B, S[n, o] = sum_c gz[c B + n, o]^2 as an fmaf chain in c order, x^2 from x.  The accumulator of an F_w
// tile starts from the stored F_w, so a curvature element is ONE chain over every minibatch accumulated so far: no K-split,
// no float atomics, the same bits whatever the grid.  F_b += colsum(S) rides on the tile column 0 blocks: four strided
// partial sums per column (the first starting from the stored F_b), added in K6's order.
//
// F18 the linearised (GLM) predictive of that posterior: bnn_laplace_glm_layer (the same g_x tiles, through one device function,
// beside 64 x 64 tiles of V [B, out] = x^2 . (s^2_w)^T + s^2_b with s^2 = 1 / (F + tau) formed while staging, whose epilogue sums
// gz_c gz_c' V over the tile's columns for every pair c <= c' of a data row: one fixed fmaf chain per partial),
// bnn_laplace_glm_finish (a thread per data row: the fp64 sum of the partials, cov, var, the Cholesky factor, the probit or
// the Gaussian summaries) and bnn_laplace_glm_sample (logits = mean + chol . eps on the Philox stream (5, 1)).
#include <math.h>

#include "bnn_device.h"
#include "bnn_nll_row.h"
#include "dense_tile.h"
#include "laplace_common.h"
#include "../../include/bnn_hip.h"

namespace bnn {
namespace {

constexpr int kChunk = BNN_LAPLACE_CHUNK;
static_assert(kChunk % kThreads == 0, "a chunk is a whole number of elements per thread");
constexpr int kPerThread = kChunk / kThreads;

// S[n, o] = sum_c gz[c B + n, o]^2 with gz = (y == NULL || y[n, o] > 0) ? gy : 0: one fmaf chain from 0 in c order
__device__ __forceinline__ float s_of(const float* gy, const float* y, long at, long cstride, int C) {
  float s = 0.f;
  for (int c = 0; c < C; ++c) {
    const float g = gy[at + c * cstride];
    s = __builtin_fmaf(g, g, s);
  }
  return (y && !(y[at] > 0.f)) ? 0.f : s;
}

// A(o, n) = S[n, o] (k = n; o contiguous)
struct SOpnd {
  Opnd gy, y;          // y.p == NULL: no mask
  long cstride;        // B * out
  int C;
};

template <bool KC>
__device__ __forceinline__ void fetch_seg(const SOpnd& q, int K, int r0, int k0, int s, float v[8]) {
  static_assert(!KC, "S is read along its contiguous (out) dimension");
  float t[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = 0.f;
#pragma unroll 1
  for (int c = 0; c < q.C; ++c) {
    Opnd g = q.gy;
    g.p += c * q.cstride;
    fetch_seg<false>(g, K, r0, k0, s, t);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = __builtin_fmaf(t[j], t[j], v[j]);
  }
  if (q.y.p) {
    fetch_seg<false>(q.y, K, r0, k0, s, t);        // (zero beyond the edge: those elements were zero already)
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = t[j] > 0.f ? v[j] : 0.f;
  }
}

struct LayerParams {
  const float* x;
  const float* gy;
  const float* y;
  const float* w;
  float* fw;
  float* fb;
  float* gx;
  float* s_out;
  int B, R, C, IN, OUT;
  int gx_mask;
  int tiles_x, tiles_n;
  int vec_x, vec_g, vec_w, vec_gx, vec_fw;
};

// (the g_x tile of both layer kernels: gx_tile, laplace_common.h)
template <typename TX>
__global__ __launch_bounds__(kThreads) void laplace_layer_kernel(LayerParams p) {
  __shared__ uint4 lds[kLdsUint4];
  f32x4 acc[2][2];
  int item = blockIdx.x;
  if (item < p.tiles_x) {
    gx_tile<TX>(p, item, lds, acc);
    return;
  }
  item -= p.tiles_x;
  // F_w [OUT, IN] += S^T . x^2: A(o, n) = S[n, o], o contiguous; B(i, n) = x[n, i]^2, i contiguous; K = B.  The chain of an
  // element starts from its stored value.
  const int tm = item / p.tiles_n, tn = item - tm * p.tiles_n;
  const int m0 = tm * kT, n0 = tn * kT;
  {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave >> 1, wn = wave & 1, fr = lane & 15, fg = lane >> 4;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int row = m0 + wm * 32 + i * 16 + fg * 4 + e, col = n0 + wn * 32 + j * 16 + fr;
          acc[i][j][e] = (row < p.OUT && col < p.IN) ? p.fw[(long)row * p.IN + col] : 0.f;
        }
  }
  const long cstride = (long)p.B * p.OUT;
  const SOpnd A{Opnd{p.gy, nullptr, 1.f, p.OUT, p.OUT, p.vec_g}, Opnd{p.y, nullptr, 1.f, p.OUT, p.OUT, p.vec_g}, cstride, p.C};
  const SqOpnd Bo{Opnd{p.x, nullptr, 1.f, p.IN, p.IN, p.vec_x}};
  gemm_tile<float, false, false, false>(A, Bo, m0, n0, p.B, lds, acc);
  tile_epilogue(lds, acc, m0, n0, p.OUT, p.IN, [&](int row, int col0, int ncol, float o[4]) {
    store_group(p.fw + (long)row * p.IN + col0, o, ncol, p.vec_fw != 0);
  });
  // F_b[o] += sum_n S[n, o] for the tile's 64 rows, partial 0 from the stored F_b.  The same blocks write S where it is asked for.
  if (tn == 0 && (p.fb || p.s_out))
    col_sum4<1>(lds, m0, p.OUT, p.B, p.fb, p.fb, [&](int n, int o) {
      const float sv = s_of(p.gy, p.y, (long)n * p.OUT + o, cstride, p.C);
      if (p.s_out) p.s_out[(long)n * p.OUT + o] = sv;
      return sv;
    });
}

constexpr double kHalfLog2Pi = -kNegLogSqrt2Pi;

// one block; thread t owns data rows t, t + 256, ...; virtual row r = c B + n
__global__ __launch_bounds__(kThreads) void laplace_seed_kernel(const float* __restrict__ z, const void* __restrict__ target, int B,
                                                                int C, int mode, int curvature, double sigma,
                                                                float* __restrict__ gy, double* __restrict__ record) {
  __shared__ double part[kThreads];
  const float nanf_ = __builtin_nanf("");
  const float inv_sigma = (float)(1.0 / sigma), inv_var = (float)(1.0 / (sigma * sigma));
  double ll = 0.0;
#pragma unroll 1
  for (int n = threadIdx.x; n < B; n += kThreads) {
    const float* row = z + (long)n * C;
    if (mode == BNN_NLL_CLASSIFICATION) {
      const long long tc = target ? reinterpret_cast<const long long*>(target)[n] : 0;
      const bool ok = tc >= 0 && tc < C;                       // an out-of-range label: NaN row, and z[label] is never read
      float mx = row[0];                                       // (row_max_sumexp's order, with the fp64 sum riding along)
      for (int c = 1; c < C; ++c) mx = fmaxf(mx, row[c]);
      float se = 0.f;
      double sed = 0.0;
      for (int c = 0; c < C; ++c) {
        se += expf(row[c] - mx);
        sed += exp((double)row[c] - (double)mx);
      }
      const float inv = ok ? 1.0f / se : nanf_;
      if (target) ll += ok ? ((double)row[tc] - (double)mx) - log(sed) : (double)nanf_;
      if (curvature == BNN_LAPLACE_GGN) {
        for (int c = 0; c < C; ++c) {
          const float pc = expf(row[c] - mx) * inv, sq = sqrtf(pc);
          float* g = gy + ((long)c * B + n) * C;
          for (int k = 0; k < C; ++k) g[k] = sq * ((k == c ? 1.f : 0.f) - expf(row[k] - mx) * inv);
        }
      } else {
        softmax_row_grad(row, C, tc, mx, se, 1.f, gy + (long)n * C);
      }
    } else {
      const float* tg = target ? reinterpret_cast<const float*>(target) + (long)n * C : nullptr;
      if (tg) {
        for (int c = 0; c < C; ++c) {
          const double d = ((double)row[c] - (double)tg[c]) / sigma;
          ll += -0.5 * d * d - log(sigma) - kHalfLog2Pi;
        }
      }
      if (curvature == BNN_LAPLACE_GGN) {
        for (int c = 0; c < C; ++c) {
          float* g = gy + ((long)c * B + n) * C;
          for (int k = 0; k < C; ++k) g[k] = k == c ? inv_sigma : 0.f;
        }
      } else {
        gauss_row_grad(row, tg, C, inv_var, 1.f, gy + (long)n * C);
      }
    }
  }
  const double total = tree_sum<kThreads>(ll, part);
  if (threadIdx.x == 0) {
    if (target) record[0] += total;
    record[1] += (double)B;
  }
}

struct TensorList {
  const float* p[BNN_LAPLACE_MAX_TENSORS];
  const float* f[BNN_LAPLACE_MAX_TENSORS];
  float* mu[BNN_LAPLACE_MAX_TENSORS];
  float* rho[BNN_LAPLACE_MAX_TENSORS];
  ChunkList<BNN_LAPLACE_MAX_TENSORS> list;
};

// stage 1: one block = one 4096-element chunk of one tensor.  ws[g * blocks + block] = sum over the chunk of log(F + tau_g)
// (g < G), ws[G * blocks + block] = sum of w^2: per-thread sums of elements tid, tid + 256, ... then the fixed-order tree.
__global__ __launch_bounds__(kThreads) void laplace_evidence_partials(const TensorList k, const Precisions pr, double* __restrict__ ws) {
  __shared__ double part[kThreads];
  long base;
  const int t = k.list.find((int)blockIdx.x, kChunk, base);
  const long n = k.list.numel[t];
  const float* __restrict__ w = k.p[t];
  const float* __restrict__ f = k.f[t];
  double fv[kPerThread];
  double sw = 0.0;
#pragma unroll
  for (int it = 0; it < kPerThread; ++it) {
    const long i = base + (long)it * kThreads + threadIdx.x;
    const bool in = i < n;
    const double wv = in ? (double)w[i] : 0.0;
    fv[it] = in ? (double)f[i] : 1.0;
    sw = fma(wv, wv, sw);
  }
  const long blocks = gridDim.x;
  const double tot_w = tree_sum<kThreads>(sw, part);
  if (threadIdx.x == 0) ws[(long)pr.n * blocks + blockIdx.x] = tot_w;
#pragma unroll 1
  for (int g = 0; g < pr.n; ++g) {
    const double tau = pr.tau[g];
    double s = 0.0;
#pragma unroll
    for (int it = 0; it < kPerThread; ++it)
      if (base + (long)it * kThreads + threadIdx.x < n) s += log(fv[it] + tau);
    const double tot = tree_sum<kThreads>(s, part);
    if (threadIdx.x == 0) ws[(long)g * blocks + blockIdx.x] = tot;
  }
}

// stage 2 (one block sums the blocks and forms the evidences): laplace_evidence_final, laplace_common.h

// softplus^-1(s) = log(expm1(s)): log s as s -> 0 (expm1 keeps the small end), s itself once exp(-s) is below fp64's epsilon
__device__ __forceinline__ double inv_softplus(double s) { return s > 40.0 ? s : log(expm1(s)); }

// one block = one 4096-element chunk of one tensor: mu = w, rho = softplus^-1((F + tau)^-1/2), formed in fp64
__global__ __launch_bounds__(kThreads) void laplace_posterior_kernel(const TensorList k, double tau_host, const double* __restrict__ tau_dev) {
  long base;
  const int t = k.list.find((int)blockIdx.x, kChunk, base);
  const long n = k.list.numel[t];
  const float* __restrict__ w = k.p[t];
  const float* __restrict__ f = k.f[t];
  float* __restrict__ mu = k.mu[t];
  float* __restrict__ rho = k.rho[t];
  const double tau = tau_dev ? *tau_dev : tau_host;
#pragma unroll
  for (int it = 0; it < kPerThread; ++it) {
    const long i = base + (long)it * kThreads + threadIdx.x;
    if (i >= n) break;
    mu[i] = w[i];
    rho[i] = (float)inv_softplus(1.0 / sqrt((double)f[i] + tau));
  }
}

// ---------------------------------------------------------------------------------------------- F18: the GLM predictive
// s^2 = fl32(1.0 / ((double)F + tau)): one fp64 add, one fp64 division, rounded once (include/bnn_hip.h F18)
__device__ __forceinline__ float var_of(float f, double tau) { return (float)(1.0 / ((double)f + tau)); }

// B(o, i) = s^2_w[o, i] from the stored curvature (k = i contiguous); zero beyond the edges, as every operand is
struct VarOpnd {
  Opnd o;
  double tau;
};

template <bool KC>
__device__ __forceinline__ void fetch_seg(const VarOpnd& q, int K, int r0, int k0, int s, float v[8]) {
  static_assert(KC, "F_w is read along its contiguous (in) dimension");
  fetch_seg<true>(q.o, K, r0, k0, s, v);
  const int r = r0 + (s >> 2), k = k0 + 8 * (s & 3);
  const int valid = r < q.o.rows ? min(8, max(0, K - k)) : 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = j < valid ? var_of(v[j], q.tau) : 0.f;
}

struct GlmLayerParams {
  const float* x;
  const float* gy;
  const float* y;
  const float* w;
  const float* fw;
  const float* fb;
  float* gx;
  float* cov_part;
  float* v_out;
  double tau;
  const double* tau_dev;
  int B, R, C, IN, OUT;
  int gx_mask;
  int tiles_x, tiles_n, tiles_o;
  int vec_x, vec_g, vec_w, vec_gx, vec_fw, vec_v;
};

template <typename TX>
__global__ __launch_bounds__(kThreads) void laplace_glm_layer_kernel(GlmLayerParams p) {
  __shared__ uint4 lds[kLdsUint4];
  f32x4 acc[2][2];
  int item = blockIdx.x;
  if (item < p.tiles_x) {
    gx_tile<TX>(p, item, lds, acc);
    return;
  }
  item -= p.tiles_x;
  // V [B, OUT] = x^2 . (s^2_w)^T: A(n, i) = x[n, i]^2, B(o, i) = s^2_w[o, i], both k (= i) contiguous; K = IN
  const int tm = item / p.tiles_o, to = item - tm * p.tiles_o;
  const int m0 = tm * kT, n0 = to * kT;
  const double tau = p.tau_dev ? *p.tau_dev : p.tau;
  const SqOpnd A{Opnd{p.x, nullptr, 1.f, p.IN, p.B, p.vec_x}};
  const VarOpnd Bo{Opnd{p.fw, nullptr, 1.f, p.IN, p.OUT, p.vec_fw}, tau};
  gemm_tile<float, true, true>(A, Bo, m0, n0, p.IN, lds, acc);
  // + s^2_b; the finished V goes back into the epilogue's LDS tile (a thread rewrites the group it read) for the pair sums
  float* t = reinterpret_cast<float*>(lds);
  tile_epilogue(lds, acc, m0, n0, p.B, p.OUT, [&](int row, int col0, int ncol, float o[4]) {
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < ncol) {
        o[c] += var_of(p.fb[col0 + c], tau);
        t[(row - m0) * kOutLd + (col0 - n0) + c] = o[c];
      }
    if (p.v_out) store_group(p.v_out + (long)row * p.OUT + col0, o, ncol, p.vec_v != 0);
  });
  __syncthreads();
  // cov_part[to, n, pair]: one fmaf chain over the tile's columns per (data row, pair c <= c'); consecutive threads share a row
  const int pairs = p.C * (p.C + 1) / 2, ncol = min(kT, p.OUT - n0);
#pragma unroll 1
  for (int q = threadIdx.x; q < kT * pairs; q += kThreads) {
    const int r = q / pairs, pr = q - r * pairs, n = m0 + r;
    if (n >= p.B) break;
    int cb = 0;
    while ((cb + 1) * (cb + 2) / 2 <= pr) ++cb;
    const int ca = pr - cb * (cb + 1) / 2;
    const float* ga = p.gy + ((long)ca * p.B + n) * p.OUT + n0;
    const float* gb = p.gy + ((long)cb * p.B + n) * p.OUT + n0;
    const float* yr = p.y ? p.y + (long)n * p.OUT + n0 : nullptr;
    const float* vr = t + r * kOutLd;
    float s = 0.f;
    if (p.vec_g) {
      // 16-byte loads, four groups in flight (the loop is bound by their latency); the chain keeps its column order
#pragma unroll 4
      for (int o = 0; o < ncol; o += 4) {                       // (OUT % 4 == 0: every group is whole)
        const float4 a4 = *reinterpret_cast<const float4*>(ga + o), b4 = *reinterpret_cast<const float4*>(gb + o);
        const float4 y4 = yr ? *reinterpret_cast<const float4*>(yr + o) : make_float4(1.f, 1.f, 1.f, 1.f);
        const float4 v4 = *reinterpret_cast<const float4*>(vr + o);
        const float av[4] = {a4.x, a4.y, a4.z, a4.w}, bv[4] = {b4.x, b4.y, b4.z, b4.w};
        const float yv[4] = {y4.x, y4.y, y4.z, y4.w}, vv[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float nx = __builtin_fmaf(av[e] * bv[e], vv[e], s);
          s = yv[e] > 0.f ? nx : s;
        }
      }
    } else {
#pragma unroll 4
      for (int o = 0; o < ncol; ++o) {
        const float g2 = ga[o] * gb[o];
        const float nx = __builtin_fmaf(g2, vr[o], s);
        s = (yr && !(yr[o] > 0.f)) ? s : nx;
      }
    }
    p.cov_part[((long)to * p.B + n) * pairs + pr] = s;
  }
}

constexpr int kGlmC = BNN_LAPLACE_GLM_MAX_CLASSES;
constexpr int kGlmPairs = kGlmC * (kGlmC + 1) / 2;
constexpr int kFinishRows = 8;                                  // data rows per block of bnn_laplace_glm_finish

struct GlmFinishParams {
  const float* part[BNN_LAPLACE_GLM_MAX_LAYERS];
  int tiles[BNN_LAPLACE_GLM_MAX_LAYERS];
  double z[BNN_PREDICTIVE_MAX_QUANTILES];
  double sigma;
  const float* mean;
  float* cov;
  float* var;
  float* chol;
  float* probs;
  long long* preds;
  float* entropy;
  float* pvar;
  float* quant;
  uint32_t* counter;
  int n_layers, B, C, mode, nq, n_samples;
};

// A block owns kFinishRows data rows.  First every thread sums the partials of its (row, pair) items -- one fixed chain per
// item, layers in list order, tiles ascending, consecutive threads on consecutive pairs (contiguous loads) -- into the row's
// fp64 lower triangle in LDS (pair = i (i + 1) / 2 + j, j <= i); then one thread per row does the row's small serial work there.
__global__ __launch_bounds__(kThreads) void laplace_glm_finish_kernel(GlmFinishParams p) {
  __shared__ double sh[kFinishRows][kGlmPairs + kGlmC];
  if (p.counter && blockIdx.x == 0 && threadIdx.x == 0) *p.counter += (uint32_t)p.n_samples;   // no block of this launch reads it
  const int C = p.C, pairs = C * (C + 1) / 2, row0 = blockIdx.x * kFinishRows;
#pragma unroll 1
  for (int q = threadIdx.x; q < kFinishRows * pairs; q += kThreads) {
    const int r = q / pairs, pr = q - r * pairs;
    if (row0 + r >= p.B) break;
    double s = 0.0;
#pragma unroll 1
    for (int l = 0; l < p.n_layers; ++l) {
      const float* src = p.part[l] + (long)(row0 + r) * pairs + pr;
      const long step = (long)p.B * pairs;
#pragma unroll 4
      for (int tl = 0; tl < p.tiles[l]; ++tl) s += (double)src[tl * step];
    }
    sh[r][pr] = s;
  }
  __syncthreads();
  const int n = row0 + threadIdx.x;
  if (threadIdx.x >= kFinishRows || n >= p.B) return;
  double* a = sh[threadIdx.x];
  double* vr = a + kGlmPairs;
  float* cov = p.cov + (long)n * C * C;
  for (int i = 0; i < C; ++i) {
    for (int j = 0; j <= i; ++j) {
      const float v = (float)a[i * (i + 1) / 2 + j];
      cov[i * C + j] = v;
      cov[j * C + i] = v;
    }
    vr[i] = a[i * (i + 1) / 2 + i];
    p.var[(long)n * C + i] = (float)vr[i];
  }
  // the lower Cholesky factor, in place, column by column; no pivoting (Cov >= min s^2_b I)
  bool ok = true;
  for (int j = 0; j < C; ++j) {
    const int jj = j * (j + 1) / 2;
    double d = a[jj + j];
    for (int k = 0; k < j; ++k) d = fma(-a[jj + k], a[jj + k], d);
    ok = ok && d > 0.0;
    const double ljj = sqrt(d);
    a[jj + j] = ljj;
    for (int i = j + 1; i < C; ++i) {
      const int ii = i * (i + 1) / 2;
      double s = a[ii + j];
      for (int k = 0; k < j; ++k) s = fma(-a[ii + k], a[jj + k], s);
      a[ii + j] = s / ljj;
    }
  }
  float* chol = p.chol + (long)n * C * C;
  const float nanf_ = __builtin_nanf("");
  for (int i = 0; i < C; ++i)
    for (int j = 0; j < C; ++j) chol[i * C + j] = j > i ? 0.f : (ok ? (float)a[i * (i + 1) / 2 + j] : nanf_);
  const float* mean = p.mean + (long)n * C;
  if (p.mode == BNN_NLL_CLASSIFICATION) {
    if (!p.probs && !p.preds && !p.entropy) return;
    constexpr double kPi8 = 0.39269908169872415481;             // pi / 8
    double* tt = a;                                             // (the factor has been written out)
    double mx = -INFINITY;
    for (int c = 0; c < C; ++c) {
      tt[c] = (double)mean[c] / sqrt(1.0 + kPi8 * vr[c]);
      mx = fmax(mx, tt[c]);
    }
    double se = 0.0;
    for (int c = 0; c < C; ++c) {
      tt[c] = exp(tt[c] - mx);
      se += tt[c];
    }
    double h = 0.0;
    float best = 0.f;
    int bi = 0;
    for (int c = 0; c < C; ++c) {
      const double pc = tt[c] / se;
      h -= pc == 0.0 ? 0.0 : pc * log(pc);
      const float pf = (float)pc;
      if (p.probs) p.probs[(long)n * C + c] = pf;
      if (c == 0 || pf > best) {                                  // the lowest index on ties; a NaN row keeps 0
        best = pf;
        bi = c;
      }
    }
    if (p.preds) p.preds[n] = bi;
    if (p.entropy) p.entropy[n] = (float)h;
  } else {
    for (int c = 0; c < C; ++c) {
      if (p.pvar) p.pvar[(long)n * C + c] = (float)(vr[c] + p.sigma * p.sigma);
      const double sd = sqrt(vr[c]);
      for (int q = 0; q < p.nq; ++q) p.quant[((long)q * p.B + n) * C + c] = (float)((double)mean[c] + p.z[q] * sd);
    }
  }
}

// The two N(0, 1) of a Box-Muller pair by the epsilon map's formula (include/bnn_hip.h), evaluated in fp64 from the fp32
// uniforms and rounded once: this launch is tiny, and its draws then equal the CPU restatement to the last bit or so.
__device__ __forceinline__ void box_muller_f64(uint32_t ra, uint32_t rb, float& n0, float& n1) {
  const double u1 = (double)u01(ra), u2 = (double)u01(rb);
  const double rad = sqrt(-2.0 * log(u1));
  double sn, cs;
  sincospi(2.0 * u2, &sn, &cs);
  n0 = (float)(rad * cs);
  n1 = (float)(rad * sn);
}

// one thread = one (sample, data row): its C normals, then one fmaf chain per output
__global__ __launch_bounds__(kThreads) void laplace_glm_sample_kernel(const float* __restrict__ mean, const float* __restrict__ chol,
                                                                      float* __restrict__ logits, int S, int B, int C, uint32_t k0,
                                                                      uint32_t k1, uint32_t sample_base,
                                                                      const uint32_t* __restrict__ counter) {
  const long idx = (long)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= (long)S * B) return;
  const int s = (int)(idx / B), n = (int)(idx - (long)s * B);
  const uint32_t g = sample_base + (counter ? *counter - (uint32_t)S : 0u) + (uint32_t)s;
  const int gpr = (C + 3) >> 2;
  float z[kGlmC];
#pragma unroll
  for (int q = 0; q < kGlmC / 4; ++q) {
    z[4 * q] = z[4 * q + 1] = z[4 * q + 2] = z[4 * q + 3] = 0.f;
    if (q < gpr) {
      const uint4 r = philox4x32<>(make_uint4((uint32_t)(n * gpr + q), g, 5u, 1u), k0, k1);
      box_muller_f64(r.x, r.y, z[4 * q], z[4 * q + 1]);
      box_muller_f64(r.z, r.w, z[4 * q + 2], z[4 * q + 3]);
    }
  }
#pragma unroll
  for (int c = 0; c < kGlmC; ++c) {
    if (c < C) {
      const float* l = chol + ((long)n * C + c) * C;
      float f = mean[(long)n * C + c];
#pragma unroll
      for (int j = 0; j <= c; ++j) f = __builtin_fmaf(l[j], z[j], f);
      logits[idx * C + c] = f;
    }
  }
}

}  // namespace
}  // namespace bnn

using namespace bnn;

extern "C" int bnn_laplace_seed(const bnn_laplace_seed_args* a, void* stream_) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_laplace_seed_args)) return BNN_ERR_ABI;
  if (a->batch <= 0 || a->classes <= 0) return BNN_ERR_SHAPE;
  if (!(a->sigma > 0.0) || !(a->sigma < INFINITY)) return BNN_ERR_SHAPE;
  const long rows = a->curvature == BNN_LAPLACE_EMPIRICAL ? (long)a->batch : (long)a->batch * a->classes;
  if (rows * a->classes > ((long)1 << 31)) return BNN_ERR_SHAPE;
  if (a->loss_mode != BNN_NLL_CLASSIFICATION && a->loss_mode != BNN_NLL_REGRESSION) return BNN_ERR_ENUM;
  if (a->curvature != BNN_LAPLACE_GGN && a->curvature != BNN_LAPLACE_EMPIRICAL) return BNN_ERR_ENUM;
  if (!a->logits || !a->gy || !a->record) return BNN_ERR_NULL;
  if (a->curvature == BNN_LAPLACE_EMPIRICAL && !a->target) return BNN_ERR_NULL;
  if (misaligned(a->logits, 4) || misaligned(a->gy, 4) || misaligned(a->record, 8) ||
      misaligned(a->target, a->loss_mode == BNN_NLL_CLASSIFICATION ? 8 : 4))
    return BNN_ERR_ALIGN;
  hipLaunchKernelGGL(laplace_seed_kernel, dim3(1), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream_), a->logits, a->target,
                     a->batch, a->classes, a->loss_mode, a->curvature, a->sigma, a->gy, a->record);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}

extern "C" int bnn_laplace_layer(const bnn_laplace_layer_args* a, void* stream_) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_laplace_layer_args)) return BNN_ERR_ABI;
  if (a->batch <= 0 || a->rows <= 0 || a->in_features <= 0 || a->out_features <= 0) return BNN_ERR_SHAPE;
  if (a->rows % a->batch != 0) return BNN_ERR_SHAPE;
  if ((long)a->rows * a->in_features > ((long)1 << 31) || (long)a->rows * a->out_features > ((long)1 << 31) ||
      (long)a->in_features * a->out_features > ((long)1 << 31))
    return BNN_ERR_SHAPE;
  if (a->math != BNN_MATH_F32 && a->math != BNN_MATH_BF16 && a->math != BNN_MATH_BF16X3) return BNN_ERR_ENUM;
  if (!a->x || !a->gy || !a->f_w) return BNN_ERR_NULL;
  if (a->g_x && !a->w) return BNN_ERR_NULL;
  if (misaligned(a->x, 4) || misaligned(a->gy, 4) || misaligned(a->y, 4) || misaligned(a->w, 4) || misaligned(a->f_w, 4) ||
      misaligned(a->f_b, 4) || misaligned(a->g_x, 4) || misaligned(a->s_out, 4))
    return BNN_ERR_ALIGN;
  LayerParams p;
  p.x = a->x; p.gy = a->gy; p.y = a->y; p.w = a->w;
  p.fw = a->f_w; p.fb = a->f_b; p.gx = a->g_x; p.s_out = a->s_out;
  p.B = a->batch; p.R = a->rows; p.C = a->rows / a->batch; p.IN = a->in_features; p.OUT = a->out_features;
  p.gx_mask = a->gx_mask ? 1 : 0;
  const int tin = (p.IN + kT - 1) / kT, tout = (p.OUT + kT - 1) / kT, tr = (p.R + kT - 1) / kT;
  p.tiles_n = tin;
  p.tiles_x = a->g_x ? tr * tin : 0;
  const long blocks = (long)p.tiles_x + (long)tout * tin;
  if (blocks > INT32_MAX) return BNN_ERR_SHAPE;
  // 16-byte loads / stores: rows of a multiple of 4 floats from 16-byte aligned bases
  p.vec_x = p.IN % 4 == 0 && !misaligned(a->x, 16);
  p.vec_w = p.IN % 4 == 0 && !misaligned(a->w, 16);
  p.vec_g = p.OUT % 4 == 0 && !misaligned(a->gy, 16) && !misaligned(a->y, 16);
  p.vec_gx = p.IN % 4 == 0 && !misaligned(a->g_x, 16);
  p.vec_fw = p.IN % 4 == 0 && !misaligned(a->f_w, 16);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream_);
  if (a->math == BNN_MATH_BF16)
    hipLaunchKernelGGL(laplace_layer_kernel<__bf16>, dim3((unsigned)blocks), dim3(kThreads), 0, st, p);
  else
    hipLaunchKernelGGL(laplace_layer_kernel<float>, dim3((unsigned)blocks), dim3(kThreads), 0, st, p);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}

namespace {

// the chunk table of a tensor list; BNN_OK or the status of the first bad entry
int chunk_table(int n_tensors, const int64_t* numel, TensorList* k, long* chunks_out) {
  for (int t = 0; t < n_tensors; ++t) {
    const int st = k->list.add(numel[t], kChunk);
    if (st != BNN_OK) return st;
  }
  for (int t = 0; t < BNN_LAPLACE_MAX_TENSORS; ++t) {
    k->p[t] = nullptr; k->f[t] = nullptr; k->mu[t] = nullptr; k->rho[t] = nullptr;
  }
  *chunks_out = k->list.finish();
  return BNN_OK;
}

}  // namespace

extern "C" size_t bnn_laplace_evidence_workspace_bytes(const bnn_laplace_evidence_args* a) {
  if (!a || a->struct_bytes != sizeof(bnn_laplace_evidence_args)) return 0;
  if (a->n_tensors <= 0 || a->n_tensors > BNN_LAPLACE_MAX_TENSORS) return 0;
  if (a->n_precisions <= 0 || a->n_precisions > BNN_LAPLACE_MAX_PRECISIONS) return 0;
  TensorList k;
  long chunks = 0;
  if (chunk_table(a->n_tensors, a->numel, &k, &chunks) != BNN_OK) return 0;
  return (size_t)chunks * (size_t)(a->n_precisions + 1) * sizeof(double);
}

extern "C" int bnn_laplace_evidence(const bnn_laplace_evidence_args* a, void* stream_) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_laplace_evidence_args)) return BNN_ERR_ABI;
  if (a->n_tensors <= 0 || a->n_tensors > BNN_LAPLACE_MAX_TENSORS) return BNN_ERR_SHAPE;
  if (a->n_precisions <= 0 || a->n_precisions > BNN_LAPLACE_MAX_PRECISIONS) return BNN_ERR_SHAPE;
  TensorList k;
  long chunks = 0;
  const int st = chunk_table(a->n_tensors, a->numel, &k, &chunks);
  if (st != BNN_OK) return st;
  Precisions pr;
  pr.n = a->n_precisions;
  double n_params = 0.0;
  for (int t = 0; t < a->n_tensors; ++t) n_params += (double)a->numel[t];
  for (int g = 0; g < BNN_LAPLACE_MAX_PRECISIONS; ++g) {
    pr.tau[g] = g < pr.n ? a->precision[g] : 1.0;
    if (g < pr.n && (!(pr.tau[g] > 0.0) || !(pr.tau[g] < INFINITY))) return BNN_ERR_SHAPE;
  }
  for (int t = 0; t < a->n_tensors; ++t)
    if (!a->param[t] || !a->curv[t]) return BNN_ERR_NULL;
  if (!a->record || !a->log_evidence) return BNN_ERR_NULL;
  if (!a->workspace || a->workspace_bytes < (size_t)chunks * (size_t)(pr.n + 1) * sizeof(double)) return BNN_ERR_WORKSPACE;
  for (int t = 0; t < a->n_tensors; ++t) {
    if (misaligned(a->param[t], 4) || misaligned(a->curv[t], 4)) return BNN_ERR_ALIGN;
    k.p[t] = a->param[t];
    k.f[t] = a->curv[t];
  }
  if (misaligned(a->record, 8) || misaligned(a->workspace, 8) || misaligned(a->log_evidence, 8) || misaligned(a->best_index, 4) ||
      misaligned(a->best, 8))
    return BNN_ERR_ALIGN;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  hipLaunchKernelGGL(laplace_evidence_partials, dim3((unsigned)chunks), dim3(kThreads), 0, stream, k, pr, static_cast<double*>(a->workspace));
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return (int)err;
  hipLaunchKernelGGL(laplace_evidence_final, dim3(1), dim3(kThreads), 0, stream, pr, static_cast<const double*>(a->workspace), (int)chunks, n_params,
                     a->record, a->log_evidence, a->best_index, a->best);
  err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}

extern "C" int bnn_laplace_posterior(const bnn_laplace_posterior_args* a, void* stream_) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_laplace_posterior_args)) return BNN_ERR_ABI;
  if (a->n_tensors <= 0 || a->n_tensors > BNN_LAPLACE_MAX_TENSORS) return BNN_ERR_SHAPE;
  TensorList k;
  long chunks = 0;
  const int st = chunk_table(a->n_tensors, a->numel, &k, &chunks);
  if (st != BNN_OK) return st;
  if (!a->precision_device && (!(a->precision > 0.0) || !(a->precision < INFINITY))) return BNN_ERR_SHAPE;
  for (int t = 0; t < a->n_tensors; ++t)
    if (!a->param[t] || !a->curv[t] || !a->mu[t] || !a->rho[t]) return BNN_ERR_NULL;
  for (int t = 0; t < a->n_tensors; ++t) {
    if (misaligned(a->param[t], 4) || misaligned(a->curv[t], 4) || misaligned(a->mu[t], 4) || misaligned(a->rho[t], 4)) return BNN_ERR_ALIGN;
    k.p[t] = a->param[t];
    k.f[t] = a->curv[t];
    k.mu[t] = a->mu[t];
    k.rho[t] = a->rho[t];
  }
  if (misaligned(a->precision_device, 8)) return BNN_ERR_ALIGN;
  hipLaunchKernelGGL(laplace_posterior_kernel, dim3((unsigned)chunks), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream_), k,
                     a->precision, a->precision_device);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}

extern "C" int bnn_laplace_glm_layer(const bnn_laplace_glm_layer_args* a, void* stream_) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_laplace_glm_layer_args)) return BNN_ERR_ABI;
  if (a->batch <= 0 || a->rows <= 0 || a->in_features <= 0 || a->out_features <= 0) return BNN_ERR_SHAPE;
  if (a->rows % a->batch != 0 || a->rows / a->batch > BNN_LAPLACE_GLM_MAX_CLASSES) return BNN_ERR_SHAPE;
  if ((long)a->rows * a->in_features > ((long)1 << 31) || (long)a->rows * a->out_features > ((long)1 << 31) ||
      (long)a->in_features * a->out_features > ((long)1 << 31))
    return BNN_ERR_SHAPE;
  if (!a->precision_device && (!(a->precision > 0.0) || !(a->precision < INFINITY))) return BNN_ERR_SHAPE;
  if (a->math != BNN_MATH_F32 && a->math != BNN_MATH_BF16 && a->math != BNN_MATH_BF16X3) return BNN_ERR_ENUM;
  if (!a->x || !a->gy || !a->f_w || !a->f_b || !a->cov_part) return BNN_ERR_NULL;
  if (a->g_x && !a->w) return BNN_ERR_NULL;
  if (misaligned(a->x, 4) || misaligned(a->gy, 4) || misaligned(a->y, 4) || misaligned(a->w, 4) || misaligned(a->f_w, 4) ||
      misaligned(a->f_b, 4) || misaligned(a->g_x, 4) || misaligned(a->cov_part, 4) || misaligned(a->v_out, 4) ||
      misaligned(a->precision_device, 8))
    return BNN_ERR_ALIGN;
  GlmLayerParams p;
  p.x = a->x; p.gy = a->gy; p.y = a->y; p.w = a->w; p.fw = a->f_w; p.fb = a->f_b;
  p.gx = a->g_x; p.cov_part = a->cov_part; p.v_out = a->v_out;
  p.tau = a->precision_device ? 1.0 : a->precision;
  p.tau_dev = a->precision_device;
  p.B = a->batch; p.R = a->rows; p.C = a->rows / a->batch; p.IN = a->in_features; p.OUT = a->out_features;
  p.gx_mask = a->gx_mask ? 1 : 0;
  const int tin = (p.IN + kT - 1) / kT, tout = (p.OUT + kT - 1) / kT, tr = (p.R + kT - 1) / kT, tb = (p.B + kT - 1) / kT;
  p.tiles_n = tin;
  p.tiles_o = tout;
  p.tiles_x = a->g_x ? tr * tin : 0;
  const long blocks = (long)p.tiles_x + (long)tb * tout;
  if (blocks > INT32_MAX) return BNN_ERR_SHAPE;
  p.vec_x = p.IN % 4 == 0 && !misaligned(a->x, 16);
  p.vec_w = p.IN % 4 == 0 && !misaligned(a->w, 16);
  p.vec_g = p.OUT % 4 == 0 && !misaligned(a->gy, 16) && !misaligned(a->y, 16);
  p.vec_gx = p.IN % 4 == 0 && !misaligned(a->g_x, 16);
  p.vec_fw = p.IN % 4 == 0 && !misaligned(a->f_w, 16);
  p.vec_v = p.OUT % 4 == 0 && !misaligned(a->v_out, 16);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream_);
  if (a->math == BNN_MATH_BF16)
    hipLaunchKernelGGL(laplace_glm_layer_kernel<__bf16>, dim3((unsigned)blocks), dim3(kThreads), 0, st, p);
  else
    hipLaunchKernelGGL(laplace_glm_layer_kernel<float>, dim3((unsigned)blocks), dim3(kThreads), 0, st, p);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}

extern "C" int bnn_laplace_glm_finish(const bnn_laplace_glm_finish_args* a, void* stream_) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_laplace_glm_finish_args)) return BNN_ERR_ABI;
  if (a->batch <= 0 || a->classes <= 0 || a->classes > BNN_LAPLACE_GLM_MAX_CLASSES) return BNN_ERR_SHAPE;
  if (a->n_layers <= 0 || a->n_layers > BNN_LAPLACE_GLM_MAX_LAYERS) return BNN_ERR_SHAPE;
  for (int l = 0; l < a->n_layers; ++l)
    if (a->tiles[l] <= 0) return BNN_ERR_SHAPE;
  if (a->n_quantiles < 0 || a->n_quantiles > BNN_PREDICTIVE_MAX_QUANTILES || a->n_samples < 0) return BNN_ERR_SHAPE;
  if ((long)a->batch * a->classes * a->classes > ((long)1 << 31)) return BNN_ERR_SHAPE;
  if (a->mode == BNN_NLL_REGRESSION) {
    if (!(a->sigma > 0.0) || !(a->sigma < INFINITY)) return BNN_ERR_SHAPE;
    for (int q = 0; q < a->n_quantiles; ++q)
      if (a->z[q] != a->z[q]) return BNN_ERR_SHAPE;
  }
  if (a->mode != BNN_NLL_CLASSIFICATION && a->mode != BNN_NLL_REGRESSION) return BNN_ERR_ENUM;
  for (int l = 0; l < a->n_layers; ++l)
    if (!a->cov_part[l]) return BNN_ERR_NULL;
  if (!a->mean || !a->cov || !a->var || !a->chol) return BNN_ERR_NULL;
  const int nq = a->mode == BNN_NLL_REGRESSION ? a->n_quantiles : 0;
  if (nq > 0 && !a->quantiles) return BNN_ERR_NULL;
  for (int l = 0; l < a->n_layers; ++l)
    if (misaligned(a->cov_part[l], 4)) return BNN_ERR_ALIGN;
  if (misaligned(a->mean, 4) || misaligned(a->cov, 4) || misaligned(a->var, 4) || misaligned(a->chol, 4) || misaligned(a->probs, 4) ||
      misaligned(a->preds, 8) || misaligned(a->entropy, 4) || misaligned(a->predictive_variance, 4) || misaligned(a->quantiles, 4) ||
      misaligned(a->sample_counter, 4))
    return BNN_ERR_ALIGN;
  GlmFinishParams p;
  for (int l = 0; l < BNN_LAPLACE_GLM_MAX_LAYERS; ++l) {
    p.part[l] = l < a->n_layers ? a->cov_part[l] : nullptr;
    p.tiles[l] = l < a->n_layers ? a->tiles[l] : 0;
  }
  for (int q = 0; q < BNN_PREDICTIVE_MAX_QUANTILES; ++q) p.z[q] = q < nq ? a->z[q] : 0.0;
  p.sigma = a->sigma;
  p.mean = a->mean; p.cov = a->cov; p.var = a->var; p.chol = a->chol;
  p.probs = a->probs; p.preds = reinterpret_cast<long long*>(a->preds); p.entropy = a->entropy;
  p.pvar = a->predictive_variance; p.quant = a->quantiles; p.counter = a->sample_counter;
  p.n_layers = a->n_layers; p.B = a->batch; p.C = a->classes; p.mode = a->mode; p.nq = nq; p.n_samples = a->n_samples;
  const int blocks = (a->batch + kFinishRows - 1) / kFinishRows;
  hipLaunchKernelGGL(laplace_glm_finish_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream_), p);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}

extern "C" int bnn_laplace_glm_sample(const bnn_laplace_glm_sample_args* a, void* stream_) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_laplace_glm_sample_args)) return BNN_ERR_ABI;
  if (a->n_samples <= 0 || a->batch <= 0 || a->classes <= 0 || a->classes > BNN_LAPLACE_GLM_MAX_CLASSES) return BNN_ERR_SHAPE;
  if ((long)a->n_samples * a->batch * a->classes > ((long)1 << 31)) return BNN_ERR_SHAPE;
  if (!a->mean || !a->chol || !a->logits) return BNN_ERR_NULL;
  if (misaligned(a->mean, 4) || misaligned(a->chol, 4) || misaligned(a->logits, 4) || misaligned(a->sample_counter, 4)) return BNN_ERR_ALIGN;
  const long threads = (long)a->n_samples * a->batch;
  const long blocks = (threads + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(laplace_glm_sample_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream_), a->mean,
                     a->chol, a->logits, a->n_samples, a->batch, a->classes, (uint32_t)(a->seed & 0xFFFFFFFFu), (uint32_t)(a->seed >> 32),
                     a->sample_base, a->sample_counter);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}
