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
#include <math.h>

#include "bnn_device.h"
#include "bnn_nll_row.h"
#include "dense_tile.h"
#include "../../include/bnn_hip.h"

namespace bnn {
namespace {

constexpr int kChunk = BNN_LAPLACE_CHUNK;
static_assert(kChunk % kThreads == 0, "a chunk is a whole number of elements per thread");
constexpr int kPerThread = kChunk / kThreads;

// B(i, n) = x[n, i]^2
struct SqOpnd {
  Opnd o;
};

template <bool KC>
__device__ __forceinline__ void fetch_seg(const SqOpnd& q, int K, int r0, int k0, int s, float v[8]) {
  fetch_seg<KC>(q.o, K, r0, k0, s, v);
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] *= v[j];
}

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

// A(r, o) = gz[r, o] = (y == NULL || y[r mod B, o] > 0) ? gy[r, o] : 0 (k = o contiguous)
struct GzOpnd {
  const float* gy;
  const float* y;
  int B, ld, rows, vec;
};

template <bool KC>
__device__ __forceinline__ void fetch_seg(const GzOpnd& q, int K, int r0, int k0, int s, float v[8]) {
  static_assert(KC, "gz is read along its contiguous (out) dimension");
  const int r = r0 + (s >> 2), k = k0 + 8 * (s & 3);
  const int valid = r < q.rows ? min(8, max(0, K - k)) : 0;
  const Opnd g{q.gy, nullptr, 1.f, q.ld, q.rows, q.vec};
  load8(g, (long)r * q.ld + k, 1, valid, q.vec, v);
  if (q.y && valid > 0) {
    float m[8];
    const Opnd y{q.y, nullptr, 1.f, q.ld, q.B, q.vec};
    load8(y, (long)(r % q.B) * q.ld + k, 1, valid, q.vec, m);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = m[j] > 0.f ? v[j] : 0.f;
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

template <typename TX>
__global__ __launch_bounds__(kThreads) void laplace_layer_kernel(LayerParams p) {
  __shared__ uint4 lds[kLdsUint4];
  f32x4 acc[2][2];
  int item = blockIdx.x;
  if (item < p.tiles_x) {
    // g_x [R, IN] = gz [R, OUT] . W [OUT, IN]: A(r, o) = gz, k (= o) contiguous; B(i, o) = W[o, i], i contiguous
    const int tm = item / p.tiles_n, tn = item - tm * p.tiles_n;
    const GzOpnd A{p.gy, p.y, p.B, p.OUT, p.R, p.vec_g};
    const Opnd Bo{p.w, nullptr, 1.f, p.IN, p.IN, p.vec_w};
    gemm_tile<TX, true, false>(A, Bo, tm * kT, tn * kT, p.OUT, lds, acc);
    // masked by the input of data row r mod B
    tile_epilogue(lds, acc, tm * kT, tn * kT, p.R, p.IN, [&](int row, int col0, int ncol, float o[4]) {
      if (p.gx_mask) {
        const long mat = (long)(row % p.B) * p.IN + col0;
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (c < ncol) o[c] = p.x[mat + c] > 0.f ? o[c] : 0.f;
      }
      store_group(p.gx + (long)row * p.IN + col0, o, ncol, p.vec_gx != 0);
    });
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

constexpr double kHalfLog2Pi = 0.91893853320467274178;

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

struct Precisions {
  double tau[BNN_LAPLACE_MAX_PRECISIONS];
  int n;
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

// stage 2: one block.  Quantity q: thread t sums blocks t, t + 256, ... in order, then the tree; thread 0 forms the evidences.
__global__ __launch_bounds__(kThreads) void laplace_evidence_final(const Precisions pr, const double* __restrict__ ws, int blocks,
                                                                   double n_params, const double* __restrict__ record,
                                                                   double* __restrict__ log_evidence, int* __restrict__ best_index,
                                                                   double* __restrict__ best) {
  __shared__ double part[kThreads];
  __shared__ double tot[BNN_LAPLACE_MAX_PRECISIONS + 1];
#pragma unroll 1
  for (int q = 0; q <= pr.n; ++q) {
    double s = 0.0;
    for (int b = threadIdx.x; b < blocks; b += kThreads) s += ws[(long)q * blocks + b];
    const double v = tree_sum<kThreads>(s, part);
    if (threadIdx.x == 0) tot[q] = v;
  }
  if (threadIdx.x != 0) return;
  const double loglik = record[0], w2 = tot[pr.n];
  int bi = 0;
  double bv = 0.0;
  for (int g = 0; g < pr.n; ++g) {
    const double tau = pr.tau[g];
    const double v = loglik - 0.5 * tau * w2 + 0.5 * n_params * log(tau) - 0.5 * tot[g];
    log_evidence[g] = v;
    if (g == 0 || v > bv) {                                    // the lowest index on ties
      bv = v;
      bi = g;
    }
  }
  if (best_index) *best_index = bi;
  if (best) {
    best[0] = bv;
    best[1] = pr.tau[bi];
  }
}

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

bool misaligned(const void* q, uintptr_t al) { return (reinterpret_cast<uintptr_t>(q) & (al - 1)) != 0; }

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
