// F20 Kronecker-factored (KFAC) Laplace posterior of MLP / MLP_Dropout (include/bnn_hip.h): bnn_kfac_layer (one Linear ->
// [ReLU] group's two Kronecker factors, the input column sums and the deltas of the layer below, one launch),
// bnn_kfac_evidence (the Laplace marginal likelihood in the Kronecker eigenbasis at every candidate prior precision),
// bnn_kfac_glm_rotate (inputs and deltas rotated into the eigenbasis, beside the deltas of the layer below),
// bnn_kfac_glm_var (the variance product in that basis and the per-class-pair partial sums bnn_laplace_glm_finish reads) and
// bnn_kfac_sample (matrix-normal weight draws for a chunk of bank members: the scaled noise rotated back, two launches).
//
// bnn_kfac_layer.  Three item kinds share one grid: blocks [0, tiles_x) own 64 x 64 tiles of g_x [R, in] = gz . W (gx_tile of
// laplace_common.h: bnn_laplace_layer's code, so its bits), the next tri(in) the tiles tn <= tm of A [in, in] += x^T x
// (K = batch), the rest the tiles tn <= tm of G [out, out] += gz^T gz (K = rows), both on the exact-fp32 matrix core with
// dense_tile.h's GEMM core.  gz is formed from gy and the saved output while staging.  An accumulator starts from the stored
// factor, so an element is ONE chain over every minibatch accumulated so far: no K-split, no float atomics.  A tile is
// written to both halves of its factor from the same registers (a diagonal tile writes its lower triangle to both), so a
// factor is bit-symmetric.  s += colsum(x) rides on the A tiles of tile column 0 (col_sum4, K6's order).
//
// In the eigenbasis of its two factors a Kronecker-factored Gaussian is a diagonal one with precisions lG_j lA_i + tau: the
// evidence is bnn_laplace_evidence's two fp64 stages over that grid, and the GLM variance is bnn_laplace_glm_layer's V product
// on rotated operands, its reciprocal precisions formed while staging from the two eigenvalue vectors.
#include <math.h>

#include "bnn_device.h"
#include "dense_tile.h"
#include "laplace_common.h"
#include "../../include/bnn_hip.h"

namespace bnn {
namespace {

constexpr int kChunk = BNN_LAPLACE_CHUNK;
constexpr int kPerThread = kChunk / kThreads;
constexpr int kLayers = BNN_LAPLACE_GLM_MAX_LAYERS;

// A(o, r) = gz[r, o] = (y == NULL || y[r mod B, o] > 0) ? gy[r, o] : 0 (k = r; o contiguous, ld = the row of gy)
struct GzTOpnd {
  const float* gy;
  const float* y;
  int B, ld, vec;
};

template <bool KC>
__device__ __forceinline__ void fetch_seg(const GzTOpnd& q, int K, int r0, int k0, int s, float v[8]) {
  static_assert(!KC, "gz^T is read along its contiguous (out) dimension");
  const int k = k0 + (s >> 3), r = r0 + 8 * (s & 7);
  const int valid = k < K ? min(8, max(0, q.ld - r)) : 0;
  const Opnd g{q.gy, nullptr, 1.f, q.ld, q.ld, q.vec};
  load8(g, (long)k * q.ld + r, 1, valid, q.vec, v);
  if (q.y && valid > 0) {
    float m[8];
    const Opnd y{q.y, nullptr, 1.f, q.ld, q.ld, q.vec};
    load8(y, (long)(k % q.B) * q.ld + r, 1, valid, q.vec, m);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = m[j] > 0.f ? v[j] : 0.f;
  }
}

// tile (tm, tn), tn <= tm, of the lower triangle's tiles in row order: item = tm (tm + 1) / 2 + tn
__device__ __forceinline__ void tri_tile(int item, int& tm, int& tn) {
  int m = (int)((sqrtf(8.f * (float)item + 1.f) - 1.f) * 0.5f);
  while ((m + 1) * (m + 2) / 2 <= item) ++m;
  while (m * (m + 1) / 2 > item) --m;
  tm = m;
  tn = item - m * (m + 1) / 2;
}

// F [n, n] += sum_k O(., k) O(., k)^T for the tile (tm, tn), tn <= tm: the accumulator starts from the stored tile, the tile
// and its mirror image are written from the same values (a diagonal tile: its lower triangle to both halves)
template <typename OP>
__device__ __forceinline__ void sym_tile(const OP& op, float* __restrict__ F, int n, int K, int tm, int tn, int vec, uint4* lds,
                                         f32x4 acc[2][2]) {
  const int m0 = tm * kT, n0 = tn * kT;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, fr = lane & 15, fg = lane >> 4;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = m0 + wm * 32 + i * 16 + fg * 4 + e, col = n0 + wn * 32 + j * 16 + fr;
        acc[i][j][e] = (row < n && col < n) ? F[(long)row * n + col] : 0.f;
      }
  gemm_tile<float, false, false, false>(op, op, m0, n0, K, lds, acc);
  float* t = reinterpret_cast<float*>(lds);
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) t[(wm * 32 + i * 16 + fg * 4 + e) * kOutLd + wn * 32 + j * 16 + fr] = acc[i][j][e];
  __syncthreads();
  const bool diag = tm == tn;
#pragma unroll 1
  for (int q = tid; q < kT * (kT / 4); q += kThreads) {
    const int r = q / (kT / 4), c4 = (q % (kT / 4)) * 4;
    float o[4];
    if (m0 + r < n && n0 + c4 < n) {
#pragma unroll
      for (int c = 0; c < 4; ++c) o[c] = (!diag || c4 + c <= r) ? t[r * kOutLd + c4 + c] : t[(c4 + c) * kOutLd + r];
      store_group(F + (long)(m0 + r) * n + n0 + c4, o, min(4, n - n0 - c4), vec != 0);
    }
    if (!diag && n0 + r < n && m0 + c4 < n) {                   // the mirror image: F[n0 + r, m0 + c] = tile[c, r]
#pragma unroll
      for (int c = 0; c < 4; ++c) o[c] = t[(c4 + c) * kOutLd + r];
      store_group(F + (long)(n0 + r) * n + m0 + c4, o, min(4, n - m0 - c4), vec != 0);
    }
  }
}

struct KfacLayerParams {
  const float* x;
  const float* gy;
  const float* y;
  const float* w;
  float* fa;
  float* fs;
  float* fg;
  float* gx;
  int B, R, IN, OUT;
  int gx_mask;
  int tiles_x, tiles_n, tiles_a;
  int vec_x, vec_g, vec_w, vec_gx, vec_fa, vec_fg;
};

template <typename TX>
__global__ __launch_bounds__(kThreads) void kfac_layer_kernel(KfacLayerParams p) {
  __shared__ uint4 lds[kLdsUint4];
  f32x4 acc[2][2];
  int item = blockIdx.x;
  if (item < p.tiles_x) {
    gx_tile<TX>(p, item, lds, acc);
    return;
  }
  item -= p.tiles_x;
  int tm, tn;
  if (item < p.tiles_a) {
    // A [IN, IN] += x^T x: O(i, n) = x[n, i], i contiguous; K = B
    tri_tile(item, tm, tn);
    const Opnd X{p.x, nullptr, 1.f, p.IN, p.IN, p.vec_x};
    sym_tile(X, p.fa, p.IN, p.B, tm, tn, p.vec_fa, lds, acc);
    // s[i] += sum_n x[n, i] for the tile's 64 rows, partial 0 from the stored s
    if (tn == 0)
      col_sum4<4>(lds, tm * kT, p.IN, p.B, p.fs, p.fs, [&](int n, int i) { return p.x[(long)n * p.IN + i]; });
    return;
  }
  // G [OUT, OUT] += gz^T gz: O(o, r) = gz[r, o], o contiguous; K = R
  tri_tile(item - p.tiles_a, tm, tn);
  const GzTOpnd Gz{p.gy, p.y, p.B, p.OUT, p.vec_g};
  sym_tile(Gz, p.fg, p.OUT, p.R, tm, tn, p.vec_fg, lds, acc);
}

// ------------------------------------------------------------------------------------------------------------ the evidence
struct KfacEvK {
  const double* la[kLayers];
  const double* lg[kLayers];
  const float* w[kLayers];
  const float* b[kLayers];
  int in1[kLayers];
  ChunkList<kLayers> list;
};

// stage 1: one block = one 4096-element chunk of one layer's [out, in + 1] eigenbasis grid (element e: j = e / (in + 1),
// i = e mod (in + 1)).  ws[g * blocks + block] = sum over the chunk of log(lG_j lA_i + tau_g), ws[G * blocks + block] = sum of
// Wbar[j, i]^2 (the weight, or the bias in the last column): per-thread sums of elements tid, tid + 256, ... then the tree.
__global__ __launch_bounds__(kThreads) void kfac_evidence_partials(const KfacEvK k, const Precisions pr, double* __restrict__ ws) {
  __shared__ double part[kThreads];
  long base;
  const int t = k.list.find((int)blockIdx.x, kChunk, base);
  const long n = k.list.numel[t];
  const int in1 = k.in1[t];
  const float* __restrict__ w = k.w[t];
  const float* __restrict__ b = k.b[t];
  const double* __restrict__ la = k.la[t];
  const double* __restrict__ lg = k.lg[t];
  double fv[kPerThread];
  double sw = 0.0;
#pragma unroll
  for (int it = 0; it < kPerThread; ++it) {
    const long e = base + (long)it * kThreads + threadIdx.x;
    const bool in = e < n;
    const long j = in ? e / in1 : 0;
    const int i = in ? (int)(e - j * in1) : 0;
    const double wv = in ? (double)(i < in1 - 1 ? w[j * (in1 - 1) + i] : b[j]) : 0.0;
    fv[it] = in ? lg[j] * la[i] : 1.0;
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

// ------------------------------------------------------------------------------------------------------- the GLM predictive
// A(n, k) = abar[n, k] = k < IN ? x[n, k] : (k == IN ? 1 : 0): the homogeneous input, k contiguous; no padded copy exists
struct AbarOpnd {
  Opnd o;              // x [B, IN]
  int IN;
};

template <bool KC>
__device__ __forceinline__ void fetch_seg(const AbarOpnd& q, int K, int r0, int k0, int s, float v[8]) {
  static_assert(KC, "abar is read along its contiguous (in) dimension");
  fetch_seg<true>(q.o, q.IN, r0, k0, s, v);                      // (zero from column IN on)
  const int r = r0 + (s >> 2), one = q.IN - (k0 + 8 * (s & 3));
  if (r < q.o.rows) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = j == one ? 1.f : v[j];
  }
}

struct RotateParams {
  const float* x;
  const float* gy;
  const float* y;
  const float* w;
  const float* qa;
  const float* qg;
  float* at;
  float* gt;
  float* gx;
  int B, R, IN, OUT;
  int gx_mask;
  int tiles_x, tiles_n, tiles_at, tiles_i1, tiles_o;
  int vec_x, vec_g, vec_w, vec_gx, vec_qa, vec_qg, vec_at, vec_gt;
};

template <typename TX>
__global__ __launch_bounds__(kThreads) void kfac_rotate_kernel(RotateParams p) {
  __shared__ uint4 lds[kLdsUint4];
  f32x4 acc[2][2];
  int item = blockIdx.x;
  if (item < p.tiles_x) {
    gx_tile<TX>(p, item, lds, acc);
    return;
  }
  item -= p.tiles_x;
  const int IN1 = p.IN + 1;
  if (item < p.tiles_at) {
    // at [B, IN + 1] = abar . Q_A: A(n, k) = abar, k contiguous; B(i, k) = Q_A[k, i], i contiguous; K = IN + 1
    const int tm = item / p.tiles_i1, tn = item - tm * p.tiles_i1;
    const AbarOpnd A{Opnd{p.x, nullptr, 1.f, p.IN, p.B, p.vec_x}, p.IN};
    const Opnd Bo{p.qa, nullptr, 1.f, IN1, IN1, p.vec_qa};
    gemm_tile<float, true, false>(A, Bo, tm * kT, tn * kT, IN1, lds, acc);
    tile_epilogue(lds, acc, tm * kT, tn * kT, p.B, IN1, [&](int row, int col0, int ncol, float o[4]) {
      store_group(p.at + (long)row * IN1 + col0, o, ncol, p.vec_at != 0);
    });
    return;
  }
  item -= p.tiles_at;
  // gt [R, OUT] = gz . Q_G: A(r, k) = gz, k contiguous; B(j, k) = Q_G[k, j], j contiguous; K = OUT
  const int tm = item / p.tiles_o, tn = item - tm * p.tiles_o;
  const GzOpnd A{p.gy, p.y, p.B, p.OUT, p.R, p.vec_g};
  const Opnd Bo{p.qg, nullptr, 1.f, p.OUT, p.OUT, p.vec_qg};
  gemm_tile<float, true, false>(A, Bo, tm * kT, tn * kT, p.OUT, lds, acc);
  tile_epilogue(lds, acc, tm * kT, tn * kT, p.R, p.OUT, [&](int row, int col0, int ncol, float o[4]) {
    store_group(p.gt + (long)row * p.OUT + col0, o, ncol, p.vec_gt != 0);
  });
}

// B(j, i) = D[j, i] = fl32(1.0 / (lG_j lA_i + tau)) from the two eigenvalue vectors (k = i): one fp64 product-and-add, one fp64
// division, rounded once; zero beyond the edges, as every operand is
struct DOpnd {
  const double* lg;
  const double* la;
  double tau;
  int rows;
};

template <bool KC>
__device__ __forceinline__ void fetch_seg(const DOpnd& q, int K, int r0, int k0, int s, float v[8]) {
  static_assert(KC, "D is formed along the eigenvalues of A");
  const int r = r0 + (s >> 2), k = k0 + 8 * (s & 3);
  const int valid = r < q.rows ? min(8, max(0, K - k)) : 0;
  const double g = valid > 0 ? q.lg[r] : 0.0;
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = j < valid ? (float)(1.0 / fma(g, q.la[k + j], q.tau)) : 0.f;
}

struct VarParams {
  const float* at;
  const float* gt;
  const double* la;
  const double* lg;
  float* cov_part;
  float* v_out;
  double tau;
  const double* tau_dev;
  int B, C, IN1, OUT;
  int tiles_o;
  int vec_at, vec_gt, vec_v;
};

__global__ __launch_bounds__(kThreads) void kfac_var_kernel(VarParams p) {
  __shared__ uint4 lds[kLdsUint4];
  f32x4 acc[2][2];
  // V [B, OUT] = at^2 . D^T: A(n, i) = at[n, i]^2, B(j, i) = D[j, i], both k (= i) contiguous; K = IN + 1
  const int item = blockIdx.x;
  const int tm = item / p.tiles_o, to = item - tm * p.tiles_o;
  const int m0 = tm * kT, n0 = to * kT;
  const double tau = p.tau_dev ? *p.tau_dev : p.tau;
  const SqOpnd A{Opnd{p.at, nullptr, 1.f, p.IN1, p.B, p.vec_at}};
  const DOpnd Bo{p.lg, p.la, tau, p.OUT};
  gemm_tile<float, true, true>(A, Bo, m0, n0, p.IN1, lds, acc);
  // the epilogue's LDS tile keeps V for the pair sums
  tile_epilogue(lds, acc, m0, n0, p.B, p.OUT, [&](int row, int col0, int ncol, float o[4]) {
    if (p.v_out) store_group(p.v_out + (long)row * p.OUT + col0, o, ncol, p.vec_v != 0);
  });
  const float* t = reinterpret_cast<const float*>(lds);
  // cov_part[to, n, pair]: one fmaf chain over the tile's columns per (data row, pair c <= c'); consecutive threads share a row
  const int pairs = p.C * (p.C + 1) / 2, ncol = min(kT, p.OUT - n0);
#pragma unroll 1
  for (int q = threadIdx.x; q < kT * pairs; q += kThreads) {
    const int r = q / pairs, pr = q - r * pairs, n = m0 + r;
    if (n >= p.B) break;
    int cb = 0;
    while ((cb + 1) * (cb + 2) / 2 <= pr) ++cb;
    const int ca = pr - cb * (cb + 1) / 2;
    const float* ga = p.gt + ((long)ca * p.B + n) * p.OUT + n0;
    const float* gb = p.gt + ((long)cb * p.B + n) * p.OUT + n0;
    const float* vr = t + r * kOutLd;
    float s = 0.f;
    if (p.vec_gt) {
#pragma unroll 4
      for (int o = 0; o < ncol; o += 4) {                       // (OUT % 4 == 0: every group is whole)
        const float4 a4 = *reinterpret_cast<const float4*>(ga + o), b4 = *reinterpret_cast<const float4*>(gb + o);
        const float4 v4 = *reinterpret_cast<const float4*>(vr + o);
        s = __builtin_fmaf(a4.x * b4.x, v4.x, s);
        s = __builtin_fmaf(a4.y * b4.y, v4.y, s);
        s = __builtin_fmaf(a4.z * b4.z, v4.z, s);
        s = __builtin_fmaf(a4.w * b4.w, v4.w, s);
      }
    } else {
#pragma unroll 4
      for (int o = 0; o < ncol; ++o) s = __builtin_fmaf(ga[o] * gb[o], vr[o], s);
    }
    p.cov_part[((long)to * p.B + n) * pairs + pr] = s;
  }
}

// ------------------------------------------------------------------------------------------------------- the weight draw
constexpr uint32_t kKfacWord3 = 4u;       // counter word 3 of the KFAC weight-draw stream (include/bnn_hip.h F20)

// A(j, i) = E[j, i] Sigma[j, i] of one member (k = i contiguous): E the N(0, 1) of element e = j (IN + 1) + i -- counter
// (e >> 2, global sample, layer, 4), slot e & 3 -- and Sigma = fl32((lG_j lA_i + tau)^-1/2) formed in fp64
struct NoiseOpnd {
  const double* lg;
  const double* la;
  double tau;
  uint32_t k0, k1, sample, layer;
  int rows, IN1;
};

template <bool KC>
__device__ __forceinline__ void fetch_seg(const NoiseOpnd& q, int K, int r0, int k0, int s, float v[8]) {
  static_assert(KC, "the noise is formed along the eigenvalues of A");
  const int r = r0 + (s >> 2), k = k0 + 8 * (s & 3);
  const int valid = r < q.rows ? min(8, max(0, K - k)) : 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = 0.f;
  if (valid == 0) return;
  const long e0 = (long)r * q.IN1 + k;
  const uint32_t g0 = (uint32_t)(e0 >> 2);
  const int off = (int)(e0 & 3);
  float n[12];
#pragma unroll
  for (int gi = 0; gi < 3; ++gi) {
    philox_normal4(g0 + (uint32_t)gi, q.sample, q.layer, q.k0, q.k1, n + 4 * gi, kKfacWord3);
  }
  const double g = q.lg[r];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (j < valid) {
      const float e = off == 0 ? n[j] : (off == 1 ? n[j + 1] : (off == 2 ? n[j + 2] : n[j + 3]));
      v[j] = e * (float)(1.0 / sqrt(fma(g, q.la[k + j], q.tau)));
    }
  }
}

struct SampleParams {
  const float* w;
  const float* b;
  const float* qa;
  const float* qg;
  const double* la;
  const double* lg;
  float* ws;           // T [members, OUT, IN + 1]
  float* bank;
  double tau;
  const double* tau_dev;
  long stride, w_off, b_off;
  uint32_t k0, k1, sample_base, layer;
  int M, first, IN, OUT;
  int tiles_o, tiles_i1;
  int vec_qa, vec_qg, vec_t;
};

// launch 1: T_m [OUT, IN + 1] = (E_m o Sigma) . Q_A^T: A(j, i) the scaled noise, B(i', i) = Q_A[i', i], both k (= i)
// contiguous; K = IN + 1.  item = (member, tile row, tile column)
__global__ __launch_bounds__(kThreads) void kfac_sample_t_kernel(SampleParams p) {
  __shared__ uint4 lds[kLdsUint4];
  f32x4 acc[2][2];
  const int IN1 = p.IN + 1, per = p.tiles_o * p.tiles_i1;
  const int m = blockIdx.x / per, rest = blockIdx.x - m * per;
  const int tm = rest / p.tiles_i1, tn = rest - tm * p.tiles_i1;
  const NoiseOpnd A{p.lg, p.la, p.tau_dev ? *p.tau_dev : p.tau, p.k0, p.k1, p.sample_base + (uint32_t)m, p.layer, p.OUT, IN1};
  const Opnd Bo{p.qa, nullptr, 1.f, IN1, IN1, p.vec_qa};
  gemm_tile<float, true, true>(A, Bo, tm * kT, tn * kT, IN1, lds, acc);
  float* __restrict__ T = p.ws + (long)m * p.OUT * IN1;
  tile_epilogue(lds, acc, tm * kT, tn * kT, p.OUT, IN1, [&](int row, int col0, int ncol, float o[4]) {
    store_group(T + (long)row * IN1 + col0, o, ncol, p.vec_t != 0);
  });
}

// launch 2: Wbar_m = Wbar + Q_G . T_m: A(j, j') = Q_G[j, j'], k (= j') contiguous; B(i, j') = T_m[j', i], i contiguous;
// K = OUT.  The epilogue adds Wbar and splits the weight and the bias columns into the bank's member layout.
__global__ __launch_bounds__(kThreads) void kfac_sample_w_kernel(SampleParams p) {
  __shared__ uint4 lds[kLdsUint4];
  f32x4 acc[2][2];
  const int IN1 = p.IN + 1, per = p.tiles_o * p.tiles_i1;
  const int m = blockIdx.x / per, rest = blockIdx.x - m * per;
  const int tm = rest / p.tiles_i1, tn = rest - tm * p.tiles_i1;
  const Opnd A{p.qg, nullptr, 1.f, p.OUT, p.OUT, p.vec_qg};
  const Opnd Bo{p.ws + (long)m * p.OUT * IN1, nullptr, 1.f, IN1, IN1, p.vec_t};
  gemm_tile<float, true, false>(A, Bo, tm * kT, tn * kT, p.OUT, lds, acc);
  float* __restrict__ member = p.bank + (long)(p.first + m) * p.stride;
  tile_epilogue(lds, acc, tm * kT, tn * kT, p.OUT, IN1, [&](int row, int col0, int ncol, float o[4]) {
    for (int c = 0; c < ncol; ++c) {
      const int col = col0 + c;
      if (col < p.IN) member[p.w_off + (long)row * p.IN + col] = p.w[(long)row * p.IN + col] + o[c];
      else member[p.b_off + row] = p.b[row] + o[c];
    }
  });
}

long tiles(long n) { return (n + kT - 1) / kT; }

// the chunk table of the layers' eigenbasis grids; BNN_OK or the status of the first bad entry
int kfac_chunks(const bnn_kfac_evidence_args* a, KfacEvK* k, long* chunks_out, double* n_params) {
  *n_params = 0.0;
  for (int l = 0; l < a->n_layers; ++l) {
    if (a->in_features[l] <= 0 || a->out_features[l] <= 0) return BNN_ERR_SHAPE;
    const long numel = ((long)a->in_features[l] + 1) * a->out_features[l];
    const int st = k->list.add(numel, kChunk);
    if (st != BNN_OK) return st;
    *n_params += (double)numel;
  }
  for (int l = 0; l < kLayers; ++l) {
    k->la[l] = nullptr; k->lg[l] = nullptr; k->w[l] = nullptr; k->b[l] = nullptr;
    k->in1[l] = l < a->n_layers ? a->in_features[l] + 1 : 1;
  }
  *chunks_out = k->list.finish();
  return BNN_OK;
}

}  // namespace
}  // namespace bnn

using namespace bnn;

extern "C" int bnn_kfac_layer(const bnn_kfac_layer_args* a, void* stream_) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_kfac_layer_args)) return BNN_ERR_ABI;
  if (a->batch <= 0 || a->rows <= 0 || a->in_features <= 0 || a->out_features <= 0) return BNN_ERR_SHAPE;
  if (a->rows % a->batch != 0) return BNN_ERR_SHAPE;
  if ((long)a->rows * a->in_features > ((long)1 << 31) || (long)a->rows * a->out_features > ((long)1 << 31) ||
      (long)a->in_features * a->out_features > ((long)1 << 31) || (long)a->in_features * a->in_features > ((long)1 << 31) ||
      (long)a->out_features * a->out_features > ((long)1 << 31))
    return BNN_ERR_SHAPE;
  if (a->math != BNN_MATH_F32 && a->math != BNN_MATH_BF16 && a->math != BNN_MATH_BF16X3) return BNN_ERR_ENUM;
  if (!a->x || !a->gy || !a->a || !a->s || !a->g) return BNN_ERR_NULL;
  if (a->g_x && !a->w) return BNN_ERR_NULL;
  if (misaligned(a->x, 4) || misaligned(a->gy, 4) || misaligned(a->y, 4) || misaligned(a->w, 4) || misaligned(a->a, 4) ||
      misaligned(a->s, 4) || misaligned(a->g, 4) || misaligned(a->g_x, 4))
    return BNN_ERR_ALIGN;
  KfacLayerParams p;
  p.x = a->x; p.gy = a->gy; p.y = a->y; p.w = a->w;
  p.fa = a->a; p.fs = a->s; p.fg = a->g; p.gx = a->g_x;
  p.B = a->batch; p.R = a->rows; p.IN = a->in_features; p.OUT = a->out_features;
  p.gx_mask = a->gx_mask ? 1 : 0;
  const long tin = tiles(p.IN), tout = tiles(p.OUT), tr = tiles(p.R);
  p.tiles_n = (int)tin;
  p.tiles_x = a->g_x ? (int)(tr * tin) : 0;
  p.tiles_a = (int)(tin * (tin + 1) / 2);
  const long blocks = (a->g_x ? tr * tin : 0) + tin * (tin + 1) / 2 + tout * (tout + 1) / 2;
  if (blocks > INT32_MAX) return BNN_ERR_SHAPE;
  // 16-byte loads / stores: rows of a multiple of 4 floats from 16-byte aligned bases
  p.vec_x = p.IN % 4 == 0 && !misaligned(a->x, 16);
  p.vec_w = p.IN % 4 == 0 && !misaligned(a->w, 16);
  p.vec_g = p.OUT % 4 == 0 && !misaligned(a->gy, 16) && !misaligned(a->y, 16);
  p.vec_gx = p.IN % 4 == 0 && !misaligned(a->g_x, 16);
  p.vec_fa = p.IN % 4 == 0 && !misaligned(a->a, 16);
  p.vec_fg = p.OUT % 4 == 0 && !misaligned(a->g, 16);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream_);
  if (a->math == BNN_MATH_BF16)
    hipLaunchKernelGGL(kfac_layer_kernel<__bf16>, dim3((unsigned)blocks), dim3(kThreads), 0, st, p);
  else
    hipLaunchKernelGGL(kfac_layer_kernel<float>, dim3((unsigned)blocks), dim3(kThreads), 0, st, p);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}

extern "C" size_t bnn_kfac_evidence_workspace_bytes(const bnn_kfac_evidence_args* a) {
  if (!a || a->struct_bytes != sizeof(bnn_kfac_evidence_args)) return 0;
  if (a->n_layers <= 0 || a->n_layers > kLayers) return 0;
  if (a->n_precisions <= 0 || a->n_precisions > BNN_LAPLACE_MAX_PRECISIONS) return 0;
  KfacEvK k;
  long chunks = 0;
  double n_params;
  if (kfac_chunks(a, &k, &chunks, &n_params) != BNN_OK) return 0;
  return (size_t)chunks * (size_t)(a->n_precisions + 1) * sizeof(double);
}

extern "C" int bnn_kfac_evidence(const bnn_kfac_evidence_args* a, void* stream_) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_kfac_evidence_args)) return BNN_ERR_ABI;
  if (a->n_layers <= 0 || a->n_layers > kLayers) return BNN_ERR_SHAPE;
  if (a->n_precisions <= 0 || a->n_precisions > BNN_LAPLACE_MAX_PRECISIONS) return BNN_ERR_SHAPE;
  KfacEvK k;
  long chunks = 0;
  double n_params = 0.0;
  const int st = kfac_chunks(a, &k, &chunks, &n_params);
  if (st != BNN_OK) return st;
  Precisions pr;
  pr.n = a->n_precisions;
  for (int g = 0; g < BNN_LAPLACE_MAX_PRECISIONS; ++g) {
    pr.tau[g] = g < pr.n ? a->precision[g] : 1.0;
    if (g < pr.n && (!(pr.tau[g] > 0.0) || !(pr.tau[g] < INFINITY))) return BNN_ERR_SHAPE;
  }
  for (int l = 0; l < a->n_layers; ++l)
    if (!a->weight[l] || !a->bias[l] || !a->lambda_a[l] || !a->lambda_g[l]) return BNN_ERR_NULL;
  if (!a->record || !a->log_evidence) return BNN_ERR_NULL;
  if (!a->workspace || a->workspace_bytes < (size_t)chunks * (size_t)(pr.n + 1) * sizeof(double)) return BNN_ERR_WORKSPACE;
  for (int l = 0; l < a->n_layers; ++l) {
    if (misaligned(a->weight[l], 4) || misaligned(a->bias[l], 4) || misaligned(a->lambda_a[l], 8) || misaligned(a->lambda_g[l], 8))
      return BNN_ERR_ALIGN;
    k.w[l] = a->weight[l]; k.b[l] = a->bias[l]; k.la[l] = a->lambda_a[l]; k.lg[l] = a->lambda_g[l];
  }
  if (misaligned(a->record, 8) || misaligned(a->workspace, 8) || misaligned(a->log_evidence, 8) || misaligned(a->best_index, 4) ||
      misaligned(a->best, 8))
    return BNN_ERR_ALIGN;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  hipLaunchKernelGGL(kfac_evidence_partials, dim3((unsigned)chunks), dim3(kThreads), 0, stream, k, pr, static_cast<double*>(a->workspace));
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return (int)err;
  hipLaunchKernelGGL(laplace_evidence_final, dim3(1), dim3(kThreads), 0, stream, pr, static_cast<const double*>(a->workspace), (int)chunks,
                     n_params, a->record, a->log_evidence, a->best_index, a->best);
  err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}

extern "C" int bnn_kfac_glm_rotate(const bnn_kfac_glm_rotate_args* a, void* stream_) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_kfac_glm_rotate_args)) return BNN_ERR_ABI;
  if (a->batch <= 0 || a->rows <= 0 || a->in_features <= 0 || a->out_features <= 0) return BNN_ERR_SHAPE;
  if (a->rows % a->batch != 0 || a->rows / a->batch > BNN_LAPLACE_GLM_MAX_CLASSES) return BNN_ERR_SHAPE;
  if ((long)a->rows * ((long)a->in_features + 1) > ((long)1 << 31) || (long)a->rows * a->out_features > ((long)1 << 31) ||
      (long)a->in_features * a->out_features > ((long)1 << 31) ||
      ((long)a->in_features + 1) * ((long)a->in_features + 1) > ((long)1 << 31) ||
      (long)a->out_features * a->out_features > ((long)1 << 31))
    return BNN_ERR_SHAPE;
  if (a->math != BNN_MATH_F32 && a->math != BNN_MATH_BF16 && a->math != BNN_MATH_BF16X3) return BNN_ERR_ENUM;
  if (!a->x || !a->gy || !a->q_a || !a->q_g || !a->at || !a->gt) return BNN_ERR_NULL;
  if (a->g_x && !a->w) return BNN_ERR_NULL;
  if (misaligned(a->x, 4) || misaligned(a->gy, 4) || misaligned(a->y, 4) || misaligned(a->w, 4) || misaligned(a->q_a, 4) ||
      misaligned(a->q_g, 4) || misaligned(a->at, 4) || misaligned(a->gt, 4) || misaligned(a->g_x, 4))
    return BNN_ERR_ALIGN;
  RotateParams p;
  p.x = a->x; p.gy = a->gy; p.y = a->y; p.w = a->w; p.qa = a->q_a; p.qg = a->q_g;
  p.at = a->at; p.gt = a->gt; p.gx = a->g_x;
  p.B = a->batch; p.R = a->rows; p.IN = a->in_features; p.OUT = a->out_features;
  p.gx_mask = a->gx_mask ? 1 : 0;
  const int IN1 = p.IN + 1;
  const long tin = tiles(p.IN), ti1 = tiles(IN1), tout = tiles(p.OUT), tr = tiles(p.R), tb = tiles(p.B);
  p.tiles_n = (int)tin;
  p.tiles_x = a->g_x ? (int)(tr * tin) : 0;
  p.tiles_i1 = (int)ti1;
  p.tiles_at = (int)(tb * ti1);
  p.tiles_o = (int)tout;
  const long blocks = (a->g_x ? tr * tin : 0) + tb * ti1 + tr * tout;
  if (blocks > INT32_MAX) return BNN_ERR_SHAPE;
  p.vec_x = p.IN % 4 == 0 && !misaligned(a->x, 16);
  p.vec_w = p.IN % 4 == 0 && !misaligned(a->w, 16);
  p.vec_g = p.OUT % 4 == 0 && !misaligned(a->gy, 16) && !misaligned(a->y, 16);
  p.vec_gx = p.IN % 4 == 0 && !misaligned(a->g_x, 16);
  p.vec_qa = IN1 % 4 == 0 && !misaligned(a->q_a, 16);
  p.vec_qg = p.OUT % 4 == 0 && !misaligned(a->q_g, 16);
  p.vec_at = IN1 % 4 == 0 && !misaligned(a->at, 16);
  p.vec_gt = p.OUT % 4 == 0 && !misaligned(a->gt, 16);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream_);
  if (a->math == BNN_MATH_BF16)
    hipLaunchKernelGGL(kfac_rotate_kernel<__bf16>, dim3((unsigned)blocks), dim3(kThreads), 0, st, p);
  else
    hipLaunchKernelGGL(kfac_rotate_kernel<float>, dim3((unsigned)blocks), dim3(kThreads), 0, st, p);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}

extern "C" int bnn_kfac_glm_var(const bnn_kfac_glm_var_args* a, void* stream_) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_kfac_glm_var_args)) return BNN_ERR_ABI;
  if (a->batch <= 0 || a->rows <= 0 || a->in_features <= 0 || a->out_features <= 0) return BNN_ERR_SHAPE;
  if (a->rows % a->batch != 0 || a->rows / a->batch > BNN_LAPLACE_GLM_MAX_CLASSES) return BNN_ERR_SHAPE;
  if ((long)a->batch * ((long)a->in_features + 1) > ((long)1 << 31) || (long)a->rows * a->out_features > ((long)1 << 31))
    return BNN_ERR_SHAPE;
  if (!a->precision_device && (!(a->precision > 0.0) || !(a->precision < INFINITY))) return BNN_ERR_SHAPE;
  if (!a->at || !a->gt || !a->lambda_a || !a->lambda_g || !a->cov_part) return BNN_ERR_NULL;
  if (misaligned(a->at, 4) || misaligned(a->gt, 4) || misaligned(a->lambda_a, 8) || misaligned(a->lambda_g, 8) ||
      misaligned(a->cov_part, 4) || misaligned(a->v_out, 4) || misaligned(a->precision_device, 8))
    return BNN_ERR_ALIGN;
  VarParams p;
  p.at = a->at; p.gt = a->gt; p.la = a->lambda_a; p.lg = a->lambda_g; p.cov_part = a->cov_part; p.v_out = a->v_out;
  p.tau = a->precision_device ? 1.0 : a->precision;
  p.tau_dev = a->precision_device;
  p.B = a->batch; p.C = a->rows / a->batch; p.IN1 = a->in_features + 1; p.OUT = a->out_features;
  const long tout = tiles(p.OUT), tb = tiles(p.B);
  p.tiles_o = (int)tout;
  if (tb * tout > INT32_MAX) return BNN_ERR_SHAPE;
  p.vec_at = p.IN1 % 4 == 0 && !misaligned(a->at, 16);
  p.vec_gt = p.OUT % 4 == 0 && !misaligned(a->gt, 16);
  p.vec_v = p.OUT % 4 == 0 && !misaligned(a->v_out, 16);
  hipLaunchKernelGGL(kfac_var_kernel, dim3((unsigned)(tb * tout)), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream_), p);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}

extern "C" size_t bnn_kfac_sample_workspace_bytes(int32_t members, int32_t in_features, int32_t out_features) {
  if (members <= 0 || in_features <= 0 || out_features <= 0) return 0;
  return (size_t)members * (size_t)out_features * ((size_t)in_features + 1) * sizeof(float);
}

extern "C" int bnn_kfac_sample(const bnn_kfac_sample_args* a, void* stream_) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_kfac_sample_args)) return BNN_ERR_ABI;
  if (a->members <= 0 || a->first < 0 || a->in_features <= 0 || a->out_features <= 0) return BNN_ERR_SHAPE;
  if (a->bank_stride < 0 || a->w_offset < 0 || a->b_offset < 0) return BNN_ERR_SHAPE;
  const long IN1 = (long)a->in_features + 1;
  if (IN1 * a->out_features > ((long)1 << 31) || IN1 * IN1 > ((long)1 << 31) ||
      (long)a->out_features * a->out_features > ((long)1 << 31))
    return BNN_ERR_SHAPE;
  const long per = tiles(a->out_features) * tiles(IN1), blocks = per * a->members;
  if (blocks > INT32_MAX) return BNN_ERR_SHAPE;
  if (!a->precision_device && (!(a->precision > 0.0) || !(a->precision < INFINITY))) return BNN_ERR_SHAPE;
  if (!a->w || !a->b || !a->q_a || !a->q_g || !a->lambda_a || !a->lambda_g || !a->bank) return BNN_ERR_NULL;
  if (!a->workspace || a->workspace_bytes < bnn_kfac_sample_workspace_bytes(a->members, a->in_features, a->out_features))
    return BNN_ERR_WORKSPACE;
  if (misaligned(a->w, 4) || misaligned(a->b, 4) || misaligned(a->q_a, 4) || misaligned(a->q_g, 4) || misaligned(a->lambda_a, 8) ||
      misaligned(a->lambda_g, 8) || misaligned(a->bank, 4) || misaligned(a->workspace, 4) || misaligned(a->precision_device, 8))
    return BNN_ERR_ALIGN;
  SampleParams p;
  p.w = a->w; p.b = a->b; p.qa = a->q_a; p.qg = a->q_g; p.la = a->lambda_a; p.lg = a->lambda_g;
  p.ws = static_cast<float*>(a->workspace); p.bank = a->bank;
  p.tau = a->precision_device ? 1.0 : a->precision;
  p.tau_dev = a->precision_device;
  p.stride = a->bank_stride; p.w_off = a->w_offset; p.b_off = a->b_offset;
  p.k0 = (uint32_t)(a->seed & 0xFFFFFFFFu); p.k1 = (uint32_t)(a->seed >> 32);
  p.sample_base = a->sample_base; p.layer = a->layer;
  p.M = a->members; p.first = a->first; p.IN = a->in_features; p.OUT = a->out_features;
  p.tiles_o = (int)tiles(p.OUT); p.tiles_i1 = (int)tiles(IN1);
  p.vec_qa = IN1 % 4 == 0 && !misaligned(a->q_a, 16);
  p.vec_qg = p.OUT % 4 == 0 && !misaligned(a->q_g, 16);
  p.vec_t = IN1 % 4 == 0 && ((long)p.OUT * IN1) % 4 == 0 && !misaligned(a->workspace, 16);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream_);
  hipLaunchKernelGGL(kfac_sample_t_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, st, p);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return (int)err;
  hipLaunchKernelGGL(kfac_sample_w_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, st, p);
  err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}
