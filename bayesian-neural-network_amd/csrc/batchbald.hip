// F15 BatchBALD (include/bnn_hip.h F15): greedy joint mutual-information batches on the device.
//   bnn_batchbald_probs    MC logits -> the pool-wide softmax P [S, N, C], per-row conditional and marginal entropies
//   bnn_batchbald_joint    H[i] = -sum_m w[m] sum_y pt (log pt + o[m]), pt = (1/S) Phat . P, fused: the product is never stored
//   bnn_batchbald_begin    the empty batch
//   bnn_batchbald_extend   the winner folded into (Phat, E, w, o, base), every configuration or importance-sampled ones
// No float atomics and no block waits for another: every sum has a fixed order, the same inputs give the same bits.
#include <float.h>
#include "bnn_device.h"
#include "../../include/bnn_hip.h"

namespace bnn {
namespace {

constexpr double kLn2d = 0x1.62e42fefa39efp-1;

// ---------------------------------------------------------------------------------------------------- probs
constexpr int kBbBlock = 256;

// a thread per row: the softmax of every sample into P, then both entropies from the fp32 values it wrote
__global__ __launch_bounds__(kBbBlock) void bb_probs_kernel(bnn_batchbald_probs_args a) {
  const int b = blockIdx.x * kBbBlock + threadIdx.x;
  if (b >= a.chunk_rows) return;
  const int S = a.n_samples, C = a.n_classes;
  const size_t N = (size_t)a.n_rows, row = (size_t)a.row0 + b;
  double cond = 0.0;
  for (int s = 0; s < S; ++s) {
    const float* __restrict__ x = a.logits + ((size_t)s * a.chunk_rows + b) * C;
    float* p = a.probs + ((size_t)s * N + row) * C;
    float mx = x[0];
    for (int c = 1; c < C; ++c) mx = fmaxf(mx, x[c]);
    float sum = 0.f;
    for (int c = 0; c < C; ++c) {
      const float e = expf(x[c] - mx);
      p[c] = e;
      sum += e;
    }
    for (int c = 0; c < C; ++c) {
      const float v = p[c] / sum;
      p[c] = v;
      if (v > 0.f) cond -= (double)v * log((double)v);
    }
  }
  a.cond[row] = cond / (double)S;
  double marg = 0.0;
  for (int c = 0; c < C; ++c) {
    double m = 0.0;
    for (int s = 0; s < S; ++s) m += (double)a.probs[((size_t)s * N + row) * C + c];      // this thread's own stores
    m /= (double)S;
    if (m > 0.0) marg -= m * log(m);
  }
  a.marg[row] = marg;
}

// ---------------------------------------------------------------------------------------------------- joint
constexpr int kJBlock = 256;                      // four waves, a 16-column tile each
constexpr int kJCols = 16 * (kJBlock / kWave);    // 64 columns (row, class) of P per block
constexpr int kJTileM = 64;                       // rows of Phat per LDS stage
constexpr int kJTargetBlocks = 2048;              // eight blocks per compute unit before M is split

struct JointPlan {
  int rows_per_block, row_blocks, tiles_per_split, splits;
};
JointPlan joint_plan(int N, int C, int M) {
  JointPlan p;
  p.rows_per_block = kJCols / C;
  p.row_blocks = (N + p.rows_per_block - 1) / p.rows_per_block;
  const int tiles = (M + kJTileM - 1) / kJTileM;
  int want = (kJTargetBlocks + p.row_blocks - 1) / p.row_blocks;
  if (want > tiles) want = tiles;
  p.tiles_per_split = (tiles + want - 1) / want;
  p.splits = (tiles + p.tiles_per_split - 1) / p.tiles_per_split;
  return p;
}

// KQ: groups of 16 samples (S <= 16 KQ).  Sample s = 16 Q + 4 g + j sits in k-slot g = lane >> 4 of MFMA (Q, j): one
// 16-byte LDS read gives a lane its A operands of four MFMAs.  P's operands stay in registers for the whole M loop.
template <int KQ>
__global__ __launch_bounds__(kJBlock) void bb_joint_kernel(bnn_batchbald_joint_args a, JointPlan plan, double* __restrict__ partial) {
  constexpr int kSp = 16 * KQ + 4;                // padded row of the Phat tile: 16-byte aligned rows, 4-bank skew
  __shared__ __attribute__((aligned(16))) float s_a[kJTileM * kSp];
  __shared__ double s_w[kJTileM], s_o[kJTileM];
  __shared__ double s_red[4][kJCols];
  __shared__ double s_col[kJCols];
  const int S = a.n_samples, C = a.n_classes, N = a.n_rows, M = a.n_configs;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 15, g = lane >> 4;
  const int i0 = blockIdx.x * plan.rows_per_block;
  const int rows = min(plan.rows_per_block, N - i0);
  const int col = wave * 16 + r;
  const bool col_ok = col < rows * C;
  const size_t NC = (size_t)N * C;
  float b[4 * KQ];
#pragma unroll
  for (int q = 0; q < 4 * KQ; ++q) {
    const int s = 16 * (q >> 2) + 4 * g + (q & 3);
    b[q] = (col_ok && s < S) ? a.probs[(size_t)s * NC + (size_t)i0 * C + col] : 0.f;
  }
  const double inv_s = 1.0 / (double)S, ln_s = log((double)S);
  const int tile0 = blockIdx.y * plan.tiles_per_split;
  const int tile1 = min(tile0 + plan.tiles_per_split, (M + kJTileM - 1) / kJTileM);
  double acc = 0.0;
  for (int tile = tile0; tile < tile1; ++tile) {
    const int m0 = tile * kJTileM;
    __syncthreads();                                                               // the tile before has been read
    for (int idx = t; idx < kJTileM * kSp; idx += kJBlock) {
      const int mr = idx / kSp, s = idx - mr * kSp;
      s_a[idx] = (m0 + mr < M && s < S) ? a.phat[(size_t)(m0 + mr) * S + s] : 0.f;
    }
    if (t < kJTileM) {
      const bool ok = m0 + t < M;
      s_w[t] = ok ? -a.weight[m0 + t] * inv_s : 0.0;                               // -w / S: the term's sign and the mean over s
      s_o[t] = ok ? a.offset[m0 + t] - ln_s : 0.0;                                 // log(sum / S) = log sum - log S
    }
    __syncthreads();
#pragma unroll
    for (int sub = 0; sub < kJTileM / 16; ++sub) {
      f32x4 c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int Q = 0; Q < KQ; ++Q) {
        const float4 a4 = *reinterpret_cast<const float4*>(&s_a[(sub * 16 + r) * kSp + 16 * Q + 4 * g]);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.x, b[4 * Q + 0], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.y, b[4 * Q + 1], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.z, b[4 * Q + 2], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.w, b[4 * Q + 3], c, 0, 0, 0);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {                                                // c[j]: configuration 4 g + j of the sub-tile, column r
        const int mr = sub * 16 + 4 * g + j;
        const float v = c[j];
        if (v >= FLT_MIN) {
          const double lg = fma((double)__builtin_amdgcn_logf(v), kLn2d, s_o[mr]);
          acc = fma(s_w[mr] * (double)v, lg, acc);
        }
      }
    }
  }
  s_red[g][col] = acc;
  __syncthreads();
  if (t < kJCols) s_col[t] = ((s_red[0][t] + s_red[1][t]) + s_red[2][t]) + s_red[3][t];
  __syncthreads();
  if (t < rows) {
    double h = 0.0;
    for (int y = 0; y < C; ++y) h += s_col[t * C + y];
    partial[(size_t)blockIdx.y * N + i0 + t] = h;
  }
}

__global__ __launch_bounds__(kBbBlock) void bb_joint_fold_kernel(bnn_batchbald_joint_args a, int splits, const double* __restrict__ partial) {
  const int i = blockIdx.x * kBbBlock + threadIdx.x;
  if (i >= a.n_rows) return;
  double h = 0.0;
  for (int sp = 0; sp < splits; ++sp) h += partial[(size_t)sp * a.n_rows + i];
  const double sc = h - a.cond[i] - *a.base;
  if (a.joint64) a.joint64[i] = h;
  if (a.scores64) a.scores64[i] = sc;
  a.scores[i] = (float)sc;
}

// ---------------------------------------------------------------------------------------------------- the state
__global__ void bb_begin_kernel(bnn_batchbald_state_args a) {
  const int s = threadIdx.x;
  if (s < a.n_samples) a.phat_out[s] = 1.f;
  if (s == 0) {
    a.expo_out[0] = 0;
    a.weight[0] = 1.0;
    a.offset[0] = 0.0;
    *a.base = 0.0;
  }
}

// chosen row j of n (the winner: j = n - 1): labelled[*n_labelled - n + j], position and row clamped
__device__ __forceinline__ int bb_chosen(const bnn_batchbald_state_args& a, int j) {
  long pos = (long)*a.n_labelled - a.n_chosen + j;
  pos = pos < 0 ? 0 : (pos >= a.n_rows ? a.n_rows - 1 : pos);
  int i = a.labelled[pos];
  return i < 0 ? 0 : (i >= a.n_rows ? a.n_rows - 1 : i);
}

// thread 0 of block 0: base and the value of the batch so far
__device__ __forceinline__ void bb_book(const bnn_batchbald_state_args& a) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const int i = bb_chosen(a, a.n_chosen - 1);
  *a.base += a.cond[i];
  if (a.batch_scores) a.batch_scores[a.n_chosen - 1] = a.scores64[i];
}

// the last row of a batch: no further step reads a state
__global__ void bb_book_kernel(bnn_batchbald_state_args a) { bb_book(a); }

// the power-of-two exponent that brings a row's largest entry into [0.5, 1); 0 for an all-zero row
__device__ __forceinline__ int bb_exponent(float mx) {
  int e = 0;
  if (mx > 0.f) frexpf(mx, &e);
  return e;
}

// EXACT: new row m C + c = row m times P[s, i*, c]
__global__ __launch_bounds__(kBbBlock) void bb_extend_exact_kernel(bnn_batchbald_state_args a, int M_new) {
  bb_book(a);
  const int mn = blockIdx.x * kBbBlock + threadIdx.x;
  if (mn >= M_new) return;
  const int S = a.n_samples, C = a.n_classes;
  const int m = mn / C, c = mn - m * C;
  const size_t NC = (size_t)a.n_rows * C, at = (size_t)bb_chosen(a, a.n_chosen - 1) * C + c;
  const float* __restrict__ in = a.phat_in + (size_t)m * S;
  float* __restrict__ out = a.phat_out + (size_t)mn * S;
  float mx = 0.f;
  for (int s = 0; s < S; ++s) {
    const float v = __fmul_rn(in[s], a.probs[(size_t)s * NC + at]);
    out[s] = v;
    mx = fmaxf(mx, v);
  }
  const int e = bb_exponent(mx);
  if (e != 0)
    for (int s = 0; s < S; ++s) out[s] = ldexpf(out[s], -e);
  const int E = a.expo_in[m] + e;
  a.expo_out[mn] = E;
  a.weight[mn] = ldexp(1.0, E);
  a.offset[mn] = (double)E * kLn2d;
}

// SAMPLED: row m follows weight draw m mod S; factors j0 .. n-1 (j0 = 0 from ones: the first sampled step)
__global__ __launch_bounds__(kBbBlock) void bb_extend_sampled_kernel(bnn_batchbald_state_args a, int M, int j0) {
  bb_book(a);
  const int m = blockIdx.x * kBbBlock + threadIdx.x;
  if (m >= M) return;
  const int S = a.n_samples, C = a.n_classes, n = a.n_chosen;
  const size_t NC = (size_t)a.n_rows * C;
  const int sm = m % S;
  float* row = a.phat_out + (size_t)m * S;
  int E = 0;
  if (j0 == 0) {
    for (int s = 0; s < S; ++s) row[s] = 1.f;
  } else {
    for (int s = 0; s < S; ++s) row[s] = a.phat_in[(size_t)m * S + s];
    E = a.expo_in[m];
  }
  const uint32_t k0 = (uint32_t)a.seed, k1 = (uint32_t)(a.seed >> 32);
  for (int j = j0; j < n; ++j) {
    const size_t at = (size_t)bb_chosen(a, j) * C;
    const float* __restrict__ p = a.probs + (size_t)sm * NC + at;
    const uint4 w = philox4x32<>(make_uint4((uint32_t)m, (uint32_t)j | (a.round << 8), 4u, 1u), k0, k1);
    const float u = (float)(w.x >> 8) * 0x1p-24f;
    float total = 0.f;
    for (int c = 0; c < C; ++c) total = __fadd_rn(total, p[c]);
    const float thr = __fmul_rn(u, total);
    float cum = 0.f;
    int y = 0;
    for (int c = 0; c < C; ++c) {
      cum = __fadd_rn(cum, p[c]);
      y += cum <= thr ? 1 : 0;
    }
    if (y > C - 1) y = C - 1;
    float mx = 0.f;
    for (int s = 0; s < S; ++s) {
      const float v = __fmul_rn(row[s], a.probs[(size_t)s * NC + at + y]);
      row[s] = v;
      mx = fmaxf(mx, v);
    }
    const int e = bb_exponent(mx);
    if (e != 0)
      for (int s = 0; s < S; ++s) row[s] = ldexpf(row[s], -e);
    E += e;
  }
  a.expo_out[m] = E;
  double sum = 0.0;
  for (int s = 0; s < S; ++s) sum += (double)row[s];
  const double qt = sum / (double)S;
  a.weight[m] = qt > 0.0 ? 1.0 / ((double)M * qt) : 0.0;
  a.offset[m] = (double)E * kLn2d;
}

bool bad_dims(int C, int S, int N) {
  return C < 2 || C > BNN_BATCHBALD_MAX_CLASSES || S < 1 || S > BNN_BATCHBALD_MAX_SAMPLES || N < 1 || N > BNN_EPOCH_MAX_ROWS;
}
// C^n when it does not exceed cap, else 0
long exact_configs(int C, int n, int cap) {
  long m = 1;
  for (int j = 0; j < n; ++j) {
    m *= C;
    if (m > cap) return 0;
  }
  return m;
}

}  // namespace
}  // namespace bnn

using namespace bnn;

extern "C" int32_t bnn_batchbald_configs(int32_t n_classes, int32_t n_chosen, int32_t max_configs) {
  if (n_classes < 2 || n_classes > BNN_BATCHBALD_MAX_CLASSES || n_chosen < 0 || n_chosen > BNN_BATCHBALD_MAX_K || max_configs < 1 ||
      max_configs > BNN_BATCHBALD_MAX_CONFIGS)
    return 0;
  const long m = exact_configs(n_classes, n_chosen, max_configs);
  return (int32_t)(m ? m : max_configs);
}

extern "C" size_t bnn_batchbald_joint_workspace_bytes(int32_t n_rows, int32_t n_classes, int32_t n_configs) {
  if (bad_dims(n_classes, 1, n_rows) || n_configs < 1 || n_configs > BNN_BATCHBALD_MAX_CONFIGS) return 0;
  const int rows_per_block = kJCols / n_classes, row_blocks = (n_rows + rows_per_block - 1) / rows_per_block;
  const int tiles = (n_configs + kJTileM - 1) / kJTileM, want = (kJTargetBlocks + row_blocks - 1) / row_blocks;
  return sizeof(double) * (size_t)(want < tiles ? want : tiles) * (size_t)n_rows;      // joint_plan's splits never exceed either
}

extern "C" int bnn_batchbald_probs(const bnn_batchbald_probs_args* a, void* stream_) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_batchbald_probs_args)) return BNN_ERR_ABI;
  if (bad_dims(a->n_classes, a->n_samples, a->n_rows) || a->chunk_rows < 1 || a->row0 < 0 ||
      (long)a->row0 + a->chunk_rows > (long)a->n_rows)
    return BNN_ERR_SHAPE;
  if (!a->logits || !a->probs || !a->cond || !a->marg) return BNN_ERR_NULL;
  if (misaligned(a->logits, 4) || misaligned(a->probs, 4) || misaligned(a->cond, 8) || misaligned(a->marg, 8)) return BNN_ERR_ALIGN;
  hipLaunchKernelGGL(bb_probs_kernel, dim3((unsigned)((a->chunk_rows + kBbBlock - 1) / kBbBlock)), dim3(kBbBlock), 0,
                     reinterpret_cast<hipStream_t>(stream_), *a);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}

extern "C" int bnn_batchbald_joint(const bnn_batchbald_joint_args* a, void* stream_) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_batchbald_joint_args)) return BNN_ERR_ABI;
  if (bad_dims(a->n_classes, a->n_samples, a->n_rows) || a->n_configs < 1 || a->n_configs > BNN_BATCHBALD_MAX_CONFIGS)
    return BNN_ERR_SHAPE;
  if (!a->probs || !a->phat || !a->weight || !a->offset || !a->cond || !a->base || !a->scores) return BNN_ERR_NULL;
  const JointPlan plan = joint_plan(a->n_rows, a->n_classes, a->n_configs);
  if (!a->workspace || a->workspace_bytes < sizeof(double) * (size_t)plan.splits * (size_t)a->n_rows) return BNN_ERR_WORKSPACE;
  if (misaligned(a->probs, 4) || misaligned(a->phat, 4) || misaligned(a->scores, 4) || misaligned(a->weight, 8) ||
      misaligned(a->offset, 8) || misaligned(a->cond, 8) || misaligned(a->base, 8) || misaligned(a->scores64, 8) ||
      misaligned(a->joint64, 8) || misaligned(a->workspace, 8))
    return BNN_ERR_ALIGN;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  double* partial = static_cast<double*>(a->workspace);
  const dim3 grid((unsigned)plan.row_blocks, (unsigned)plan.splits);
  const int S = a->n_samples;
  if (S <= 16)
    hipLaunchKernelGGL(bb_joint_kernel<1>, grid, dim3(kJBlock), 0, stream, *a, plan, partial);
  else if (S <= 32)
    hipLaunchKernelGGL(bb_joint_kernel<2>, grid, dim3(kJBlock), 0, stream, *a, plan, partial);
  else if (S <= 64)
    hipLaunchKernelGGL(bb_joint_kernel<4>, grid, dim3(kJBlock), 0, stream, *a, plan, partial);
  else
    hipLaunchKernelGGL(bb_joint_kernel<8>, grid, dim3(kJBlock), 0, stream, *a, plan, partial);
  hipLaunchKernelGGL(bb_joint_fold_kernel, dim3((unsigned)((a->n_rows + kBbBlock - 1) / kBbBlock)), dim3(kBbBlock), 0, stream, *a,
                     plan.splits, partial);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}

extern "C" int bnn_batchbald_begin(const bnn_batchbald_state_args* a, void* stream_) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_batchbald_state_args)) return BNN_ERR_ABI;
  if (a->n_samples < 1 || a->n_samples > BNN_BATCHBALD_MAX_SAMPLES) return BNN_ERR_SHAPE;
  if (!a->phat_out || !a->expo_out || !a->weight || !a->offset || !a->base) return BNN_ERR_NULL;
  if (misaligned(a->phat_out, 4) || misaligned(a->expo_out, 4) || misaligned(a->weight, 8) || misaligned(a->offset, 8) ||
      misaligned(a->base, 8))
    return BNN_ERR_ALIGN;
  hipLaunchKernelGGL(bb_begin_kernel, dim3(1), dim3(BNN_BATCHBALD_MAX_SAMPLES), 0, reinterpret_cast<hipStream_t>(stream_), *a);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}

extern "C" int bnn_batchbald_extend(const bnn_batchbald_state_args* a, void* stream_) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_batchbald_state_args)) return BNN_ERR_ABI;
  if (bad_dims(a->n_classes, a->n_samples, a->n_rows) || a->max_configs < 1 || a->max_configs > BNN_BATCHBALD_MAX_CONFIGS ||
      a->n_chosen < 1 || a->n_chosen > BNN_BATCHBALD_MAX_K)
    return BNN_ERR_SHAPE;
  if (!a->probs || !a->cond || !a->labelled || !a->n_labelled || !a->phat_in || !a->expo_in || !a->phat_out || !a->expo_out ||
      !a->weight || !a->offset || !a->base || (a->batch_scores && !a->scores64))
    return BNN_ERR_NULL;
  if (misaligned(a->probs, 4) || misaligned(a->labelled, 4) || misaligned(a->n_labelled, 4) || misaligned(a->phat_in, 4) ||
      misaligned(a->expo_in, 4) || misaligned(a->phat_out, 4) || misaligned(a->expo_out, 4) || misaligned(a->cond, 8) ||
      misaligned(a->scores64, 8) || misaligned(a->weight, 8) || misaligned(a->offset, 8) || misaligned(a->base, 8) ||
      misaligned(a->batch_scores, 8))
    return BNN_ERR_ALIGN;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const int n = a->n_chosen;
  const long exact = exact_configs(a->n_classes, n, a->max_configs);
  if (a->last) {
    hipLaunchKernelGGL(bb_book_kernel, dim3(1), dim3(1), 0, stream, *a);
  } else if (exact) {
    hipLaunchKernelGGL(bb_extend_exact_kernel, dim3((unsigned)((exact + kBbBlock - 1) / kBbBlock)), dim3(kBbBlock), 0, stream, *a,
                       (int)exact);
  } else {
    const int M = a->max_configs;
    const int j0 = exact_configs(a->n_classes, n - 1, a->max_configs) ? 0 : n - 1;   // the step before enumerated: rebuild from ones
    hipLaunchKernelGGL(bb_extend_sampled_kernel, dim3((unsigned)((M + kBbBlock - 1) / kBbBlock)), dim3(kBbBlock), 0, stream, *a, M, j0);
  }
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}
