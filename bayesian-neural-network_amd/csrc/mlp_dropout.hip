// K5 bnn_dense_fwd: one nn.Linear of MLP_Dropout for S MC-dropout samples in one launch -- a small-tile MFMA GEMM
// against the shared fp32 weights with the bias, ReLU and the kind-3 dropout mask (include/bnn_hip.h) in the epilogue --
// and bnn_dropout_mask, the mask stream materialised for tests.
//
// Tiling.  A 256-thread block (4 waves, 2 x 2) owns a BM x BN output tile, BM = 32 TM, BN = 32 TN (TM = TN = 2: 64 x 64;
// 4: 128 x 128); a wave owns TM x TN accumulators of 16 x 16.  K is walked in 32-wide stages through two LDS buffers:
// every thread loads its 8-element row segments of the next stage into registers (fp32 x / W converted to bf16 there in
// bf16 math: no cast launch) while the waves run the MFMAs of the current stage, then stores them into the other buffer;
// one barrier per stage.  The stage image (swz) and the LDS buffer's size are dense_tile.h's, shared with K6 and the
// Laplace curvature; the k loop and the epilogue are this kernel's own measured forms.  The shapes that matter are small
// in M (S * B = 1280 rows against 1200 x 1200 at the reference's test_samples = 10), where K1g's 256 x 256 tile would
// leave most CUs idle.
//
// Reduction order.  An output element is the same chain of MFMAs over the same 32-wide k stages whatever the tile size,
// M and the sample split, so results do not depend on how samples are split over calls or on the plan's tile.
#include <math.h>

#include "bnn_device.h"
#include "dense_tile.h"
#include "../../include/bnn_hip.h"

namespace bnn {
namespace {

constexpr int kMinBlocks = 512;         // 2 blocks per CU: below this the larger tile / fewer sample runs would idle CUs
constexpr int kMinSamplesPerRun = 4;    // shared x: a block applies its tile to at least this many samples when it can

struct DenseParams {
  const void* x;
  const float* w;
  const float* b;
  void* y;
  int M, N, K;            // GEMM rows (batch if x is shared, else S * batch), features, reduction
  int B, S, runs, tiles_n, tiles;
  int x_shared, relu, drop, vec_x, vec_w, vec_y;
  uint32_t thr, k0, k1, tensor_id, sample_base, inc;
  float scale;
  uint32_t* counter;
};

// the 8 elements [k, k + 8) of row `row` of a [rows, K] source, zero outside, converted to T (bf16: RNE)
template <typename XT, typename T>
__device__ __forceinline__ void load_seg(const XT* __restrict__ src, int rows, int K, int row, int k, int vec, T out[8]) {
  if (row < rows && vec && k + 8 <= K) {
    const XT* p = src + (long)row * K + k;
    if constexpr (sizeof(XT) == 4) {
      const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
      const float f[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
      for (int j = 0; j < 8; ++j) out[j] = (T)f[j];
    } else {
      const bf16x8 v = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
      for (int j = 0; j < 8; ++j) out[j] = (T)v[j];
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) out[j] = (row < rows && k + j < K) ? (T)src[(long)row * K + k + j] : (T)0.0f;
  }
}

// store a row segment (8 elements: k = 8 seg .. 8 seg + 7) into the stage image (uint4 = one 16-byte chunk)
template <typename T>
__device__ __forceinline__ void store_seg(uint4* img, int row, int seg, const T v[8]) {
  if constexpr (sizeof(T) == 2) {
    bf16x8 p;
#pragma unroll
    for (int j = 0; j < 8; ++j) p[j] = v[j];
    img[swz<T>(row, seg)] = __builtin_bit_cast(uint4, p);
  } else {
    img[swz<T>(row, 2 * seg)] = make_uint4(__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3]));
    img[swz<T>(row, 2 * seg + 1)] = make_uint4(__float_as_uint(v[4]), __float_as_uint(v[5]), __float_as_uint(v[6]), __float_as_uint(v[7]));
  }
}

// 4 consecutive outputs (16-byte aligned fp32 / 8-byte aligned bf16)
__device__ __forceinline__ void store4(float* dst, const float o[4]) { *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2], o[3]); }
__device__ __forceinline__ void store4(__bf16* dst, const float o[4]) {
  *reinterpret_cast<bf16x4*>(dst) = bf16x4{(__bf16)o[0], (__bf16)o[1], (__bf16)o[2], (__bf16)o[3]};
}

template <typename T, typename XT, typename YT, int TM, int TN>
__global__ __launch_bounds__(kThreads) void dense_fwd_kernel(DenseParams p) {
  constexpr int BM = 32 * TM, BN = 32 * TN;
  constexpr int ROW_CHUNKS = kBK * (int)sizeof(T) / 16;
  constexpr int STAGE = (BM + BN) * ROW_CHUNKS;            // uint4 per stage buffer
  __shared__ uint4 lds_raw[tile_lds_uint4<T, TM, TN>()];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int item = blockIdx.x;
  const int run = item / p.tiles, tile = item - run * p.tiles;
  const int tm = tile / p.tiles_n, tn = tile - tm * p.tiles_n;
  const int m0 = tm * BM, n0 = tn * BN;
  if (p.inc && item == 0 && tid == 0 && p.counter) *p.counter += p.inc;   // no block of this launch reads the counter

  const XT* __restrict__ x = static_cast<const XT*>(p.x);
  const float* __restrict__ w = p.w;

  // this thread's staging segments: segment i < BM * 4 of A is (row i / 4, k 8 (i % 4)); of B likewise over BN rows
  constexpr int A_SEGS = BM * 4 / kThreads, B_SEGS = BN * 4 / kThreads;
  T ra[A_SEGS][8], rb[B_SEGS][8];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int i = 0; i < A_SEGS; ++i) {
      const int s = tid + i * kThreads;
      load_seg<XT, T>(x, p.M, p.K, m0 + (s >> 2), k0 + 8 * (s & 3), p.vec_x, ra[i]);
    }
#pragma unroll
    for (int i = 0; i < B_SEGS; ++i) {
      const int s = tid + i * kThreads;
      load_seg<float, T>(w, p.N, p.K, n0 + (s >> 2), k0 + 8 * (s & 3), p.vec_w, rb[i]);
    }
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int i = 0; i < A_SEGS; ++i) {
      const int s = tid + i * kThreads;
      store_seg<T>(lds_raw + buf * STAGE, s >> 2, s & 3, ra[i]);
    }
#pragma unroll
    for (int i = 0; i < B_SEGS; ++i) {
      const int s = tid + i * kThreads;
      store_seg<T>(lds_raw + buf * STAGE + BM * ROW_CHUNKS, s >> 2, s & 3, rb[i]);
    }
  };

  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = (p.K + kBK - 1) / kBK;
  const int fr = lane & 15, fg = lane >> 4;
  fetch(0);
  stash(0);
  __syncthreads();
#pragma unroll 1
  for (int kt = 0; kt < nk; ++kt) {
    if (kt + 1 < nk) fetch((kt + 1) * kBK);
    const uint4* img = lds_raw + (kt & 1) * STAGE;
    if constexpr (sizeof(T) == 2) {
      bf16x8 af[TM], bf[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i)
        af[i] = __builtin_bit_cast(bf16x8, img[swz<T>(wm * 16 * TM + i * 16 + fr, fg)]);
#pragma unroll
      for (int j = 0; j < TN; ++j)
        bf[j] = __builtin_bit_cast(bf16x8, img[BM * ROW_CHUNKS + swz<T>(wn * 16 * TN + j * 16 + fr, fg)]);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bf[j], acc[i][j], 0, 0, 0);
    } else {
      f32x4 af[TM][2], bf[TN][2];
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int r = wm * 16 * TM + i * 16 + fr;
        af[i][0] = __builtin_bit_cast(f32x4, img[swz<T>(r, fg)]);
        af[i][1] = __builtin_bit_cast(f32x4, img[swz<T>(r, fg + 4)]);
      }
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int r = wn * 16 * TN + j * 16 + fr;
        bf[j][0] = __builtin_bit_cast(f32x4, img[BM * ROW_CHUNKS + swz<T>(r, fg)]);
        bf[j][1] = __builtin_bit_cast(f32x4, img[BM * ROW_CHUNKS + swz<T>(r, fg + 4)]);
      }
#pragma unroll
      for (int e = 0; e < 8; ++e)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i][e >> 2][e & 3], bf[j][e >> 2][e & 3], acc[i][j], 0, 0, 0);
    }
    if (kt + 1 < nk) stash((kt + 1) & 1);
    __syncthreads();
  }

  // epilogue.  The accumulators go through LDS (lane: column lane & 15, rows 4 (lane >> 4) + e of each 16 x 16 tile) so
  // that a thread then owns 4 consecutive columns of a row: one Philox call per 4 elements (one mask group) and
  // coalesced stores.  Then bias, ReLU, the mask, store; a shared-x block repeats the last step for its run of samples.
  constexpr int OUT_LD = BN + 4;                           // fp32 output tile row (tile_lds_uint4 counts it), 16-byte rows
  float* tile_out = reinterpret_cast<float*>(lds_raw);
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        tile_out[(wm * 16 * TM + i * 16 + fg * 4 + e) * OUT_LD + wn * 16 * TN + j * 16 + fr] = acc[i][j][e];
  __syncthreads();

  YT* __restrict__ y = static_cast<YT*>(p.y);
  const uint32_t gpr = (uint32_t)(p.N + 3) >> 2;
  const uint32_t base = p.sample_base + ((p.drop && p.counter) ? *p.counter : 0u);   // (a launch with inc drops nothing)
  int s_lo = 0, s_hi = 1;
  if (p.x_shared) {
    const int per = (p.S + p.runs - 1) / p.runs;
    s_lo = run * per;
    s_hi = min(p.S, s_lo + per);
  }
  constexpr int GROUPS = BM * (BN / 4);
#pragma unroll 1
  for (int q = tid; q < GROUPS; q += kThreads) {
    const int r = q / (BN / 4), c4 = (q % (BN / 4)) * 4;
    const int row = m0 + r, col0 = n0 + c4;
    if (row >= p.M || col0 >= p.N) continue;
    const float4 a4 = *reinterpret_cast<const float4*>(tile_out + r * OUT_LD + c4);
    float v[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      v[c] += (p.b && col0 + c < p.N) ? p.b[col0 + c] : 0.f;
      if (p.relu) v[c] = fmaxf(v[c], 0.f);
    }
    const int ncol = min(4, p.N - col0);
#pragma unroll 1
    for (int s = s_lo; s < s_hi; ++s) {           // one pass unless x is shared (then: the run's samples)
      const int sm = p.x_shared ? s : row / p.B, brow = p.x_shared ? row : row - sm * p.B;
      float o[4];
      if (p.drop) {
        const uint4 rr = philox4x32<>(make_uint4(eps_group((uint32_t)brow, (uint32_t)col0, gpr), base + (uint32_t)sm, p.tensor_id, 0u),
                                      p.k0, p.k1);
        o[0] = rr.x >= p.thr ? v[0] * p.scale : 0.f;
        o[1] = rr.y >= p.thr ? v[1] * p.scale : 0.f;
        o[2] = rr.z >= p.thr ? v[2] * p.scale : 0.f;
        o[3] = rr.w >= p.thr ? v[3] * p.scale : 0.f;
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) o[c] = v[c];
      }
      YT* dst = y + ((long)sm * p.B + brow) * p.N + col0;
      if (ncol == 4 && p.vec_y) {
        store4(dst, o);
      } else {
        for (int c = 0; c < ncol; ++c) dst[c] = (YT)o[c];
      }
    }
  }
}

__global__ void dropout_mask_kernel(float* __restrict__ mask, uint32_t k0, uint32_t k1, uint32_t tensor_id,
                                    uint32_t sample_offset, int S, int rows, int cols, uint32_t thr, float scale) {
  const int gpr = (cols + 3) >> 2;
  const long groups = (long)rows * gpr;
  const long total = groups * S;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int s = (int)(i / groups);
    const long g = i - (long)s * groups;
    const int row = (int)(g / gpr), c0 = (int)(g - (long)row * gpr) * 4;
    const uint4 r = philox4x32<>(make_uint4((uint32_t)g, sample_offset + (uint32_t)s, tensor_id, 0u), k0, k1);
    const uint32_t v[4] = {r.x, r.y, r.z, r.w};
    float* out = mask + ((size_t)s * rows + row) * cols + c0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (c0 + j < cols) out[j] = v[j] >= thr ? scale : 0.f;
  }
}

// Argument checks and the launch geometry of bnn_dense_fwd (a pure function of the arguments' values and alignment).
struct DenseLaunch {
  int big;          // 128 x 128 tiles (bf16 math only)
  int runs, tiles_m, tiles_n, blocks, lds_bytes, bm;
  int math_bf16;
};

int dense_check(const bnn_dense_fwd_args* a, DenseLaunch& L) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_dense_fwd_args)) return BNN_ERR_ABI;
  if (a->n_samples <= 0 || a->batch <= 0 || a->in_features <= 0 || a->out_features <= 0 || a->layer_id < 0)
    return BNN_ERR_SHAPE;
  if (a->math != BNN_MATH_F32 && a->math != BNN_MATH_BF16 && a->math != BNN_MATH_BF16X3) return BNN_ERR_ENUM;
  if ((a->x_dtype != BNN_F32 && a->x_dtype != BNN_BF16) || (a->y_dtype != BNN_F32 && a->y_dtype != BNN_BF16)) return BNN_ERR_ENUM;
  L.math_bf16 = a->math == BNN_MATH_BF16;
  if (!L.math_bf16 && (a->x_dtype != BNN_F32 || a->y_dtype != BNN_F32)) return BNN_ERR_ENUM;
  uint32_t thr;
  float scale;
  if (!drop_params(a->drop_p, thr, scale)) return BNN_ERR_SHAPE;
  if (a->sample_counter_inc && a->drop_p != 0.0) return BNN_ERR_SHAPE;
  const long rows = a->x_shared ? (long)a->batch : (long)a->n_samples * a->batch;
  if (rows > INT32_MAX / 2 || (long)a->n_samples * a->batch * a->out_features > ((long)1 << 40)) return BNN_ERR_SHAPE;
  const int M = (int)rows, N = a->out_features;
  L.big = 0;
  if (L.math_bf16) {
    const long big_tiles = (long)((M + 127) / 128) * ((N + 127) / 128);
    L.big = big_tiles >= kMinBlocks;
  }
  L.bm = L.big ? 128 : 64;
  L.tiles_m = (M + L.bm - 1) / L.bm;
  L.tiles_n = (N + L.bm - 1) / L.bm;
  const long tiles = (long)L.tiles_m * L.tiles_n;
  L.runs = 1;
  if (a->x_shared) {
    long want = (kMinBlocks + tiles - 1) / tiles;
    const long most = (a->n_samples + kMinSamplesPerRun - 1) / kMinSamplesPerRun;
    L.runs = (int)(want < most ? want : most);
    if (L.runs < 1) L.runs = 1;
    const int per = (a->n_samples + L.runs - 1) / L.runs;          // no empty run
    L.runs = (a->n_samples + per - 1) / per;
  }
  if (tiles * L.runs > INT32_MAX) return BNN_ERR_SHAPE;
  L.blocks = (int)(tiles * L.runs);
  L.lds_bytes = 16 * (!L.math_bf16 ? tile_lds_uint4<float, 2, 2>()
                      : L.big      ? tile_lds_uint4<__bf16, 4, 4>()
                                   : tile_lds_uint4<__bf16, 2, 2>());
  return BNN_OK;
}

template <typename T, typename XT, typename YT, int TM>
void launch(const DenseParams& p, int blocks, hipStream_t st) {
  hipLaunchKernelGGL((dense_fwd_kernel<T, XT, YT, TM, TM>), dim3((unsigned)blocks), dim3(kThreads), 0, st, p);
}

}  // namespace
}  // namespace bnn

using namespace bnn;

extern "C" int bnn_dense_plan(const bnn_dense_fwd_args* a, bnn_plan* plan) {
  if (!plan) return BNN_ERR_NULL;
  DenseLaunch L;
  const int rc = dense_check(a, L);
  if (rc) return rc;
  plan->form = BNN_FORM_GEMM;
  plan->k_classes = 1;
  plan->waves = kThreads / 64;
  plan->batch_rows = L.bm;
  plan->k_slices = L.runs;
  plan->blocks = L.blocks;
  plan->lds_bytes = L.lds_bytes;
  plan->features_per_block = L.bm;
  return BNN_OK;
}

extern "C" int bnn_dense_fwd(const bnn_dense_fwd_args* a, void* stream_) {
  DenseLaunch L;
  const int rc = dense_check(a, L);
  if (rc) return rc;
  if (!a->x || !a->w || !a->y) return BNN_ERR_NULL;
  if (a->sample_counter_inc && !a->sample_counter) return BNN_ERR_NULL;
  const int xb = a->x_dtype == BNN_BF16 ? 2 : 4, yb = a->y_dtype == BNN_BF16 ? 2 : 4;
  if (misaligned(a->x, xb) || misaligned(a->w, 4) || misaligned(a->b, 4) || misaligned(a->y, yb) ||
      misaligned(a->sample_counter, 4))
    return BNN_ERR_ALIGN;
  DenseParams p;
  p.x = a->x;
  p.w = a->w;
  p.b = a->b;
  p.y = a->y;
  p.M = a->x_shared ? a->batch : a->n_samples * a->batch;
  p.N = a->out_features;
  p.K = a->in_features;
  p.B = a->batch;
  p.S = a->n_samples;
  p.runs = L.runs;
  p.tiles_n = L.tiles_n;
  p.tiles = L.tiles_m * L.tiles_n;
  p.x_shared = a->x_shared ? 1 : 0;
  p.relu = a->relu ? 1 : 0;
  p.drop = a->drop_p != 0.0;
  drop_params(a->drop_p, p.thr, p.scale);
  // vector loads: 8 consecutive elements of a row from a 16-byte aligned address
  p.vec_x = xb == 4 ? (a->in_features % 4 == 0 && !misaligned(a->x, 16)) : (a->in_features % 8 == 0 && !misaligned(a->x, 16));
  p.vec_w = a->in_features % 4 == 0 && !misaligned(a->w, 16);
  p.vec_y = a->out_features % 4 == 0 && !misaligned(a->y, 4 * yb);
  p.k0 = (uint32_t)a->seed;
  p.k1 = (uint32_t)(a->seed >> 32);
  p.tensor_id = eps_tensor_id((uint32_t)a->layer_id, kEpsDropout);
  p.sample_base = a->sample_offset;
  p.inc = a->sample_counter_inc;
  p.counter = a->sample_counter;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream_);
  const bool xb16 = a->x_dtype == BNN_BF16, yb16 = a->y_dtype == BNN_BF16;
  if (!L.math_bf16) {
    launch<float, float, float, 2>(p, L.blocks, st);
  } else if (L.big) {
    if (xb16) {
      if (yb16) launch<__bf16, __bf16, __bf16, 4>(p, L.blocks, st);
      else launch<__bf16, __bf16, float, 4>(p, L.blocks, st);
    } else {
      if (yb16) launch<__bf16, float, __bf16, 4>(p, L.blocks, st);
      else launch<__bf16, float, float, 4>(p, L.blocks, st);
    }
  } else {
    if (xb16) {
      if (yb16) launch<__bf16, __bf16, __bf16, 2>(p, L.blocks, st);
      else launch<__bf16, __bf16, float, 2>(p, L.blocks, st);
    } else {
      if (yb16) launch<__bf16, float, __bf16, 2>(p, L.blocks, st);
      else launch<__bf16, float, float, 2>(p, L.blocks, st);
    }
  }
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}

extern "C" int bnn_dropout_mask(float* mask, uint64_t seed, uint32_t layer_id, uint32_t sample_offset, int32_t n_samples,
                                int32_t rows, int32_t cols, double p, void* stream_) {
  if (!mask) return BNN_ERR_NULL;
  if (n_samples <= 0 || rows <= 0 || cols <= 0 || layer_id > 0x3FFFFFFFu) return BNN_ERR_SHAPE;
  uint32_t thr;
  float scale;
  if (!drop_params(p, thr, scale)) return BNN_ERR_SHAPE;
  if (misaligned(mask, 4)) return BNN_ERR_ALIGN;
  const long total = (long)n_samples * rows * ((cols + 3) / 4);
  long nb = (total + 255) / 256;
  if (nb > 4096) nb = 4096;
  hipLaunchKernelGGL(dropout_mask_kernel, dim3((unsigned)nb), dim3(256), 0, reinterpret_cast<hipStream_t>(stream_), mask,
                     (uint32_t)seed, (uint32_t)(seed >> 32), eps_tensor_id(layer_id, kEpsDropout), sample_offset, n_samples, rows, cols, thr, scale);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}
