// The 64 x 64 tile GEMM core, tile epilogue and column sum of K6's backward (dense_train.hip) and of the Laplace curvature
// (laplace.hip); K5's forward (mlp_dropout.hip) shares the stage image (swz), the constants and the LDS size.  A 256-thread
// block of 2 x 2 waves, 2 x 2 accumulators of 16 x 16 per wave, K walked in 32-wide stages through two LDS buffers (next
// stage loaded into registers during the current stage's MFMAs), the XOR-swizzled [row][k] image of K5.  Operands are
// read along their contiguous dimension -- a thread loads 8 consecutive elements and writes them into the [row][k] image
// element by element.  An operand is any type with a fetch_seg<KC>(o, K, r0, k0, s, v) overload: Opnd below (a matrix,
// optionally masked on load), or a caller's own (laplace.hip: squares and sums of squares formed on load).
#pragma once

#include <math.h>

#include "bnn_device.h"

namespace bnn {
namespace {

constexpr int kThreads = 256;
constexpr int kBK = 32;      // k per LDS stage
constexpr int kT = 64;       // tile rows and columns (2 waves x 2 accumulators x 16)

// An operand of C[m, n] = sum_k A(m, k) B(n, k): element (r, k) at p[r * ld + k] (kc: k contiguous) or p[k * ld + r].
// msk (optional): the value is p[.] * (msk[.] > 0 ? s : 0) -- gz formed from gy and the saved output y.
struct Opnd {
  const float* p;
  const float* msk;
  float s;
  int ld, rows, vec;
};

__device__ __forceinline__ float gz_of(float g, const float* msk, long i, float s) {
  return msk ? (msk[i] > 0.f ? g * s : 0.f) : g;
}

template <typename T>
__device__ __forceinline__ int swz(int row, int chunk) {
  constexpr int CH = kBK * (int)sizeof(T) / 16;
  return row * CH + (chunk ^ ((row >> 1) & (CH - 1)));
}

// the element index (in T) of (row, k) in the stage image
template <typename T>
__device__ __forceinline__ int elem(int row, int k) {
  constexpr int PER = 16 / (int)sizeof(T);
  return swz<T>(row, k / PER) * PER + (k % PER);
}

// 8 elements p[base + j * step] (j < valid; zero beyond), masked; vec: two 16-byte loads (step 1, valid == 8)
__device__ __forceinline__ void load8(const Opnd& o, long base, long step, int valid, bool vec, float v[8]) {
  if (vec && valid == 8) {
    const float4 a = *reinterpret_cast<const float4*>(o.p + base), b = *reinterpret_cast<const float4*>(o.p + base + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    if (o.msk) {
      const float4 c = *reinterpret_cast<const float4*>(o.msk + base), d = *reinterpret_cast<const float4*>(o.msk + base + 4);
      const float m[8] = {c.x, c.y, c.z, c.w, d.x, d.y, d.z, d.w};
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = m[j] > 0.f ? v[j] * o.s : 0.f;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = j < valid ? gz_of(o.p[base + j * step], o.msk, base + j * step, o.s) : 0.f;
  }
}

// One thread's segment of an operand's stage: 8 elements.  kc: row r = s / 4, k = 8 (s % 4) .. +7 (along k);
// otherwise k = s / 8, rows 8 (s % 8) .. +7 (along the rows).  r0: the tile's first row, k0: the stage's first k.
template <bool KC>
__device__ __forceinline__ void fetch_seg(const Opnd& o, int K, int r0, int k0, int s, float v[8]) {
  if constexpr (KC) {
    const int r = r0 + (s >> 2), k = k0 + 8 * (s & 3);
    const int valid = r < o.rows ? min(8, max(0, K - k)) : 0;
    load8(o, (long)r * o.ld + k, 1, valid, o.vec, v);
  } else {
    const int k = k0 + (s >> 3), r = r0 + 8 * (s & 7);
    const int valid = k < K ? min(8, max(0, o.rows - r)) : 0;
    load8(o, (long)k * o.ld + r, 1, valid, o.vec, v);
  }
}

template <typename T, bool KC>
__device__ __forceinline__ void stash_seg(T* img, int s, const float v[8]) {
  if constexpr (KC) {
    const int r = s >> 2, k = 8 * (s & 3);
#pragma unroll
    for (int j = 0; j < 8; ++j) img[elem<T>(r, k + j)] = (T)v[j];
  } else {
    const int k = s >> 3, r = 8 * (s & 7);
#pragma unroll
    for (int j = 0; j < 8; ++j) img[elem<T>(r + j, k)] = (T)v[j];
  }
}

// acc[i][j] (rows wm 32 + 16 i, columns wn 32 + 16 j of the tile) = sum_k A(m0 + ., k) B(n0 + ., k) over k < K, added
// in k order to zero (ZERO) or to what the caller put into acc
template <typename T, bool AKC, bool BKC, bool ZERO = true, typename OA, typename OB>
__device__ __forceinline__ void gemm_tile(const OA& A, const OB& Bo, int m0, int n0, int K, uint4* lds, f32x4 acc[2][2]) {
  constexpr int ROW_CHUNKS = kBK * (int)sizeof(T) / 16;
  constexpr int STAGE = 2 * kT * ROW_CHUNKS;                  // uint4 per stage buffer (A rows, then B rows)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int fr = lane & 15, fg = lane >> 4;
  float ra[8], rb[8];
  if constexpr (ZERO) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  auto stash = [&](int buf) {
    T* img = reinterpret_cast<T*>(lds + buf * STAGE);
    stash_seg<T, AKC>(img, tid, ra);
    stash_seg<T, BKC>(img + kT * ROW_CHUNKS * (16 / (int)sizeof(T)), tid, rb);
  };
  const int nk = (K + kBK - 1) / kBK;
  fetch_seg<AKC>(A, K, m0, 0, tid, ra);
  fetch_seg<BKC>(Bo, K, n0, 0, tid, rb);
  stash(0);
  __syncthreads();
#pragma unroll 1
  for (int kt = 0; kt < nk; ++kt) {
    if (kt + 1 < nk) {
      fetch_seg<AKC>(A, K, m0, (kt + 1) * kBK, tid, ra);
      fetch_seg<BKC>(Bo, K, n0, (kt + 1) * kBK, tid, rb);
    }
    const uint4* img = lds + (kt & 1) * STAGE;
    if constexpr (sizeof(T) == 2) {
      bf16x8 af[2], bf[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) af[i] = __builtin_bit_cast(bf16x8, img[swz<T>(wm * 32 + i * 16 + fr, fg)]);
#pragma unroll
      for (int j = 0; j < 2; ++j) bf[j] = __builtin_bit_cast(bf16x8, img[kT * ROW_CHUNKS + swz<T>(wn * 32 + j * 16 + fr, fg)]);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bf[j], acc[i][j], 0, 0, 0);
    } else {
      f32x4 af[2][2], bf[2][2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int r = wm * 32 + i * 16 + fr;
        af[i][0] = __builtin_bit_cast(f32x4, img[swz<T>(r, fg)]);
        af[i][1] = __builtin_bit_cast(f32x4, img[swz<T>(r, fg + 4)]);
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int r = wn * 32 + j * 16 + fr;
        bf[j][0] = __builtin_bit_cast(f32x4, img[kT * ROW_CHUNKS + swz<T>(r, fg)]);
        bf[j][1] = __builtin_bit_cast(f32x4, img[kT * ROW_CHUNKS + swz<T>(r, fg + 4)]);
      }
#pragma unroll
      for (int e = 0; e < 8; ++e)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i][e >> 2][e & 3], bf[j][e >> 2][e & 3], acc[i][j], 0, 0, 0);
    }
    if (kt + 1 < nk) stash((kt + 1) & 1);
    __syncthreads();
  }
}

constexpr int cmax(int a, int b) { return a > b ? a : b; }

// uint4 words of the LDS buffer of a kernel that owns a 32 TM x 32 TN tile staged as T: the union of the two stage buffers
// and the epilogue's fp32 tile (rows of 32 TN + 4 floats).  K5 (mlp_dropout.hip) sizes its own tiles with it too.
template <typename T, int TM, int TN>
constexpr int tile_lds_uint4() {
  return cmax(2 * 32 * (TM + TN) * (kBK * (int)sizeof(T) / 16), 32 * TM * (32 * TN + 4) / 4);
}

constexpr int kOutLd = kT + 4;                                  // the epilogue's fp32 tile row, 16-byte rows
constexpr int kLdsUint4 = tile_lds_uint4<float, 2, 2>();        // (fp32 stages: the larger image)

// The epilogue.  The accumulators go through LDS (lane: column lane & 15, rows 4 (lane >> 4) + e of each 16 x 16 accumulator)
// so that a thread then owns 4 consecutive columns of a row: f(row, col0, ncol, o) for every group inside [rows, cols), o the
// group's 4 values (the first ncol of them inside).  Follows gemm_tile's last barrier.
template <typename F>
__device__ __forceinline__ void tile_epilogue(uint4* lds, f32x4 acc[2][2], int m0, int n0, int rows, int cols, F&& f) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, fr = lane & 15, fg = lane >> 4;
  float* t = reinterpret_cast<float*>(lds);
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) t[(wm * 32 + i * 16 + fg * 4 + e) * kOutLd + wn * 32 + j * 16 + fr] = acc[i][j][e];
  __syncthreads();
#pragma unroll 1
  for (int q = tid; q < kT * (kT / 4); q += kThreads) {
    const int r = q / (kT / 4), c4 = (q % (kT / 4)) * 4;
    const int row = m0 + r, col0 = n0 + c4;
    if (row >= rows || col0 >= cols) continue;
    const float4 a4 = *reinterpret_cast<const float4*>(t + r * kOutLd + c4);
    float o[4] = {a4.x, a4.y, a4.z, a4.w};
    f(row, col0, min(4, cols - col0), o);
  }
}

// 4 consecutive fp32 of a row: one 16-byte store (vec, all 4 inside) or the first ncol one by one
__device__ __forceinline__ void store_group(float* dst, const float o[4], int ncol, bool vec) {
  if (ncol == 4 && vec) {
    *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2], o[3]);
  } else {
    for (int c = 0; c < ncol; ++c) dst[c] = o[c];
  }
}

// out[o] = sum_n value(n, o) over n < N for the columns o = m0 .. m0 + 63 below cols: partial g of four sums n = g, g + 4, ...
// in order (partial 0 starting from init[o] when init is given), then ((0 + 1) + 2) + 3.  value may store on the side; out
// may be NULL (then that is all it is called for).  All 256 threads; no float atomics, one fixed chain per column.
// UNROLL: of the loop over n (loads in flight against code size: value is inlined into it).
template <int UNROLL, typename V>
__device__ __forceinline__ void col_sum4(uint4* lds, int m0, int cols, int N, const float* init, float* out, V&& value) {
  __syncthreads();
  float* part = reinterpret_cast<float*>(lds);
  const int c = threadIdx.x & 63, g = threadIdx.x >> 6, o = m0 + c;
  float s = 0.f;
  if (o < cols) {
    if (g == 0 && init) s = init[o];
#pragma unroll UNROLL
    for (int n = g; n < N; n += 4) s += value(n, o);
  }
  part[g * 64 + c] = s;
  __syncthreads();
  if (threadIdx.x < 64 && o < cols && out) out[o] = ((part[c] + part[64 + c]) + part[128 + c]) + part[192 + c];
}

// The kind-3 dropout map's threshold and scale (K5's forward and the ensemble's training forward): thr = min(floor(p 2^32),
// 2^32 - 1), scale = (float)(1 / (1 - p)) in fp64; false unless 0 <= p < 1 (NaN fails)
inline bool drop_params(double p, uint32_t& thr, float& scale) {
  if (!(p >= 0.0 && p < 1.0)) return false;
  const double t = floor(p * 4294967296.0);
  thr = t >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)t;
  scale = (float)(1.0 / (1.0 - p));
  return true;
}

}  // namespace
}  // namespace bnn
