// F9 bnn_pruned_fwd: one mean-weight layer of a network pruned at PL drop levels, all levels in one launch
// (include/bnn_hip.h F9):  y[p] = act(x[p] . (mu (.) [code > p])^T + b (.) [bcode > p]).
//
// The levels differ only in a mask, so the parameter bytes are read once.  A 256-thread block (4 waves) owns a 32-row x
// 64-column output tile of EVERY level; wave w owns columns 16 w .. 16 w + 15: 2 row tiles x PL levels of 16 x 16
// accumulators.  K is walked in 32-wide stages through two LDS buffers: every thread loads its 16-byte pieces of the
// next stage's 64 x 32 mu tile and its 64 x 32 code bytes into registers while the waves work on the current stage, then
// stores them into the other buffer; one barrier per stage.  In a stage a lane reads its mu fragment and its code bytes
// from LDS ONCE, and per level forms the masked fragment in registers (bf16: a byte-wise compare by carry into bit 7, two
// v_perm_b32 and an AND per four elements; fp32: a select per element) and feeds that level's accumulators against that
// level's x fragments.  x is not staged: a lane's x fragment is 16 (bf16) or 2 x 16 (fp32) contiguous bytes of one row,
// loaded straight from global one stage ahead (the four waves of a block read the same rows: the later ones hit in L1/L2).
//
// Tile choice.  At the sizes this serves (128-row minibatches against 1200 x 1200) the launch is a few GFLOP spread over
// ~80 blocks of 38 k-stages: latency bound, not MFMA bound (not measured).  32 x 64 keeps the accumulators of 8 levels at
// 64 VGPRs and the block count at ceil(rows / 32) x ceil(out / 64); a larger tile would leave still more CUs idle, a
// smaller one would halve the MFMAs fed per masked fragment.
//
// LDS image: mu rows of 32 k = 4 (bf16) or 8 (fp32) 16-byte chunks, chunk c of row r at c ^ ((r >> 1) & (chunks - 1)) as in
// mlp_dropout.hip (every 16-lane group of a ds_read_b128 covers the banks once); code rows of 32 bytes, unswizzled (a
// wave's 8-byte reads cover 512 contiguous bytes).
//
// Reduction order: an output element is the same chain of MFMAs over the same k stages whatever PL and the launch split.
#include "bnn_device.h"
#include "../../include/bnn_hip.h"

namespace bnn {
namespace {

constexpr int kThreads = 256;
constexpr int kBK = 32;
constexpr int kBM = 32, kBN = 64;
constexpr int kTM = kBM / 16;

struct PrunedParams {
  const void* x;
  const void* w;
  const uint8_t* code;
  const float* b;
  const uint8_t* bcode;
  void* y;
  long x_lstride, y_lstride;      // elements between levels (x: 0 when shared)
  int M, N, K, ld, ldx, ldy;
  int level0, relu, vec_x;
};

template <typename T>
__device__ __forceinline__ int swz(int row, int chunk) {
  constexpr int CH = kBK * (int)sizeof(T) / 16;
  return row * CH + (chunk ^ ((row >> 1) & (CH - 1)));
}

// 16 bytes of row `row` of x from element k on (bf16: 8 elements, fp32: 4), zero past K
template <typename T>
__device__ __forceinline__ uint4 load_x16(const T* __restrict__ x, int ldx, int K, int row, int k, int vec) {
  constexpr int E = 16 / (int)sizeof(T);
  const T* p = x + (long)row * ldx + k;
  if (vec && k + E <= K) return *reinterpret_cast<const uint4*>(p);
  uint4 r;
  if constexpr (sizeof(T) == 4) {
    r.x = k + 0 < K ? __float_as_uint(p[0]) : 0u;
    r.y = k + 1 < K ? __float_as_uint(p[1]) : 0u;
    r.z = k + 2 < K ? __float_as_uint(p[2]) : 0u;
    r.w = k + 3 < K ? __float_as_uint(p[3]) : 0u;
  } else {
    const unsigned short* q = reinterpret_cast<const unsigned short*>(p);
    auto two = [&](int j) { return (k + j < K ? (uint32_t)q[j] : 0u) | (k + j + 1 < K ? (uint32_t)q[j + 1] << 16 : 0u); };
    r.x = two(0); r.y = two(2); r.z = two(4); r.w = two(6);
  }
  return r;
}

// bytes 0x00 / 0xFF per code byte: code > level.  codes <= 16 and level <= 15, so code + (127 - level) carries into bit 7
// exactly when code > level and never into the next byte.
__device__ __forceinline__ uint32_t keep_bytes(uint32_t codes, uint32_t add) {
  const uint32_t k = ((codes + add) >> 7) & 0x01010101u;
  return (k << 8) - k;
}

template <typename T, typename YT, int PL>
__global__ __launch_bounds__(kThreads) void pruned_fwd_kernel(PrunedParams p) {
  constexpr bool BF = sizeof(T) == 2;
  constexpr int ROW_CHUNKS = kBK * (int)sizeof(T) / 16;           // 4 | 8
  constexpr int W_STAGE = kBN * ROW_CHUNKS;                       // uint4 per stage
  constexpr int C_STAGE = kBN * 2;
  constexpr int W_LOADS = W_STAGE / kThreads;                     // 1 | 2
  constexpr int XF = BF ? 1 : 2;                                  // uint4 per x fragment
  __shared__ uint4 s_w[2 * W_STAGE];
  __shared__ uint4 s_c[2 * C_STAGE];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fg = lane >> 4;
  const int n0 = blockIdx.x * kBN, m0 = blockIdx.y * kBM;
  const T* __restrict__ x = static_cast<const T*>(p.x) + (long)p.level0 * p.x_lstride;
  const uint4* __restrict__ w16 = static_cast<const uint4*>(p.w);
  const uint4* __restrict__ c16 = reinterpret_cast<const uint4*>(p.code);
  const int ld_w16 = p.ld * (int)sizeof(T) / 16, ld_c16 = p.ld / 16;

  // this thread's 16-byte pieces of a stage: one (bf16) or two (fp32) of the mu tile, one of the code tile (threads < 128)
  const int wrow0 = tid / ROW_CHUNKS, wch = tid % ROW_CHUNKS, wrow1 = wrow0 + kThreads / ROW_CHUNKS;
  const uint4* wsrc0 = w16 + (long)(n0 + wrow0) * ld_w16 + wch;
  const uint4* wsrc1 = w16 + (long)(n0 + (W_LOADS == 2 ? wrow1 : wrow0)) * ld_w16 + wch;
  const uint4* csrc = c16 + (long)(n0 + ((tid & (C_STAGE - 1)) >> 1)) * ld_c16 + (tid & 1);
  uint4 rw0, rw1, rc;
  auto fetch = [&](int k0) __attribute__((always_inline)) {       // the canonical images are padded: no bounds
    const int kc = k0 * (int)sizeof(T) / 16;
    rw0 = wsrc0[kc];
    if constexpr (W_LOADS == 2) rw1 = wsrc1[kc];
    if (tid < C_STAGE) rc = csrc[k0 / 16];
  };
  auto stash = [&](int buf) __attribute__((always_inline)) {
    s_w[buf * W_STAGE + swz<T>(wrow0, wch)] = rw0;
    if constexpr (W_LOADS == 2) s_w[buf * W_STAGE + swz<T>(wrow1, wch)] = rw1;
    if (tid < C_STAGE) s_c[buf * C_STAGE + tid] = rc;
  };

  int xrow[kTM];
#pragma unroll
  for (int i = 0; i < kTM; ++i) xrow[i] = min(m0 + 16 * i + fr, p.M - 1);   // rows past M: a valid row, never stored
  auto load_x = [&](int k0, uint4 (&xf)[PL][kTM][XF]) __attribute__((always_inline)) {
#pragma unroll
    for (int lv = 0; lv < PL; ++lv)
#pragma unroll
      for (int i = 0; i < kTM; ++i) {
        const T* xl = x + (long)lv * p.x_lstride;
        if constexpr (BF) {
          xf[lv][i][0] = load_x16<T>(xl, p.ldx, p.K, xrow[i], k0 + 8 * fg, p.vec_x);
        } else {
          xf[lv][i][0] = load_x16<T>(xl, p.ldx, p.K, xrow[i], k0 + 4 * fg, p.vec_x);
          xf[lv][i][1] = load_x16<T>(xl, p.ldx, p.K, xrow[i], k0 + 16 + 4 * fg, p.vec_x);
        }
      }
  };

  f32x4 acc[PL][kTM];
#pragma unroll
  for (int lv = 0; lv < PL; ++lv)
#pragma unroll
    for (int i = 0; i < kTM; ++i) acc[lv][i] = f32x4{0.f, 0.f, 0.f, 0.f};

  const uint32_t add0 = (0x7Fu - (uint32_t)p.level0) * 0x01010101u;
  const int wr = wave * 16 + fr;                                  // this lane's row of the mu / code tile
  auto compute = [&](int buf, const uint4 (&xf)[PL][kTM][XF]) __attribute__((always_inline)) {
    const uint4* img = s_w + buf * W_STAGE;
    const uint32_t* cimg = reinterpret_cast<const uint32_t*>(s_c + buf * C_STAGE);
    if constexpr (BF) {
      const uint4 wv = img[swz<T>(wr, fg)];
      const uint32_t c0 = cimg[wr * 8 + 2 * fg], c1 = cimg[wr * 8 + 2 * fg + 1];
#pragma unroll
      for (int lv = 0; lv < PL; ++lv) {
        const uint32_t add = add0 - (uint32_t)lv * 0x01010101u;
        const uint32_t k0 = keep_bytes(c0, add), k1 = keep_bytes(c1, add);
        uint4 m;
        m.x = wv.x & __builtin_amdgcn_perm(k0, k0, 0x01010000u);
        m.y = wv.y & __builtin_amdgcn_perm(k0, k0, 0x03030202u);
        m.z = wv.z & __builtin_amdgcn_perm(k1, k1, 0x01010000u);
        m.w = wv.w & __builtin_amdgcn_perm(k1, k1, 0x03030202u);
        const bf16x8 bfrag = __builtin_bit_cast(bf16x8, m);
#pragma unroll
        for (int i = 0; i < kTM; ++i)
          acc[lv][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, xf[lv][i][0]), bfrag, acc[lv][i], 0, 0, 0);
      }
    } else {
      const f32x4 w0 = __builtin_bit_cast(f32x4, img[swz<T>(wr, fg)]), w1 = __builtin_bit_cast(f32x4, img[swz<T>(wr, fg + 4)]);
      const uint32_t cc0 = cimg[wr * 8 + fg], cc1 = cimg[wr * 8 + 4 + fg];
#pragma unroll
      for (int lv = 0; lv < PL; ++lv) {
        const uint32_t add = add0 - (uint32_t)lv * 0x01010101u;
        const uint32_t t0 = cc0 + add, t1 = cc1 + add;             // bit 7 of byte j: code_j > level
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const uint32_t keep = ((e < 4 ? t0 : t1) >> (8 * (e & 3) + 7)) & 1u;
          const float wm = keep ? (e < 4 ? w0[e & 3] : w1[e & 3]) : 0.f;
#pragma unroll
          for (int i = 0; i < kTM; ++i)
            acc[lv][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(__builtin_bit_cast(f32x4, xf[lv][i][e >> 2])[e & 3], wm, acc[lv][i], 0, 0, 0);
        }
      }
    }
  };

  const int nk = (p.K + kBK - 1) / kBK;
  uint4 xa[PL][kTM][XF], xb[PL][kTM][XF];
  fetch(0);
  load_x(0, xa);
  stash(0);
  __syncthreads();
  auto stage = [&](int kt, const uint4 (&cur)[PL][kTM][XF], uint4 (&nxt)[PL][kTM][XF]) __attribute__((always_inline)) {
    const bool more = kt + 1 < nk;
    if (more) {
      fetch((kt + 1) * kBK);
      load_x((kt + 1) * kBK, nxt);
    }
    compute(kt & 1, cur);
    if (more) stash((kt + 1) & 1);
    __syncthreads();
  };
#pragma unroll 1
  for (int kt = 0; kt < nk; kt += 2) {                             // two stages per trip: the x fragments swap roles, no copies
    stage(kt, xa, xb);
    if (kt + 1 < nk) stage(kt + 1, xb, xa);
  }

  // epilogue: lane = column fr of its wave's 16, rows 4 fg + e of each row tile; bias (masked like the weights), ReLU
  YT* __restrict__ y = static_cast<YT*>(p.y) + (long)p.level0 * p.y_lstride;
  const int col = n0 + wave * 16 + fr;
  if (col < p.N) {
    const float bias = p.b ? p.b[col] : 0.f;
    const int bc = p.b ? (int)p.bcode[col] : 0;
#pragma unroll
    for (int lv = 0; lv < PL; ++lv) {
      const float bl = bc > p.level0 + lv ? bias : 0.f;
#pragma unroll
      for (int i = 0; i < kTM; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int row = m0 + 16 * i + 4 * fg + e;
          if (row < p.M) {
            float v = acc[lv][i][e] + bl;
            if (p.relu) v = fmaxf(v, 0.f);
            y[(long)lv * p.y_lstride + (long)row * p.ldy + col] = (YT)v;
          }
        }
    }
  }
}

template <typename T, typename YT>
void launch_levels(const PrunedParams& p, int levels, dim3 grid, hipStream_t st) {
  switch (levels) {
    case 1: hipLaunchKernelGGL((pruned_fwd_kernel<T, YT, 1>), grid, dim3(kThreads), 0, st, p); break;
    case 2: hipLaunchKernelGGL((pruned_fwd_kernel<T, YT, 2>), grid, dim3(kThreads), 0, st, p); break;
    case 3: hipLaunchKernelGGL((pruned_fwd_kernel<T, YT, 3>), grid, dim3(kThreads), 0, st, p); break;
    case 4: hipLaunchKernelGGL((pruned_fwd_kernel<T, YT, 4>), grid, dim3(kThreads), 0, st, p); break;
    case 5: hipLaunchKernelGGL((pruned_fwd_kernel<T, YT, 5>), grid, dim3(kThreads), 0, st, p); break;
    case 6: hipLaunchKernelGGL((pruned_fwd_kernel<T, YT, 6>), grid, dim3(kThreads), 0, st, p); break;
    case 7: hipLaunchKernelGGL((pruned_fwd_kernel<T, YT, 7>), grid, dim3(kThreads), 0, st, p); break;
    default: hipLaunchKernelGGL((pruned_fwd_kernel<T, YT, 8>), grid, dim3(kThreads), 0, st, p); break;
  }
}

}  // namespace
}  // namespace bnn

using namespace bnn;

extern "C" int bnn_pruned_fwd(const bnn_pruned_fwd_args* a, void* stream_) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_pruned_fwd_args)) return BNN_ERR_ABI;
  if (a->n_levels < 1 || a->n_levels > BNN_PRUNE_MAX_LEVELS || a->rows < 1 || a->in_features < 1 || a->out_features < 1 ||
      a->ld % 32 || a->ld < a->in_features || a->ldx < a->in_features || a->ldy < a->out_features)
    return BNN_ERR_SHAPE;
  if (a->math != BNN_MATH_F32 && a->math != BNN_MATH_BF16 && a->math != BNN_MATH_BF16X3) return BNN_ERR_ENUM;
  if ((a->x_dtype != BNN_F32 && a->x_dtype != BNN_BF16) || (a->y_dtype != BNN_F32 && a->y_dtype != BNN_BF16)) return BNN_ERR_ENUM;
  const bool bf = a->math == BNN_MATH_BF16;
  if (bf ? a->x_dtype != BNN_BF16 : (a->x_dtype != BNN_F32 || a->y_dtype != BNN_F32)) return BNN_ERR_ENUM;
  if (!a->x || !a->mu || !a->code || !a->y || (!a->b) != (!a->bcode)) return BNN_ERR_NULL;
  const int xb = bf ? 2 : 4, yb = a->y_dtype == BNN_BF16 ? 2 : 4;
  if (misaligned(a->mu, 16) || misaligned(a->code, 16) || misaligned(a->x, xb) || misaligned(a->y, yb) || misaligned(a->b, 4))
    return BNN_ERR_ALIGN;
  PrunedParams p;
  p.x = a->x;
  p.w = a->mu;
  p.code = a->code;
  p.b = a->b;
  p.bcode = a->bcode;
  p.y = a->y;
  p.x_lstride = a->x_shared ? 0 : (long)a->rows * a->ldx;
  p.y_lstride = (long)a->rows * a->ldy;
  p.M = a->rows;
  p.N = a->out_features;
  p.K = a->in_features;
  p.ld = a->ld;
  p.ldx = a->ldx;
  p.ldy = a->ldy;
  p.relu = a->relu ? 1 : 0;
  p.vec_x = !misaligned(a->x, 16) && (a->ldx * xb) % 16 == 0;     // every 16-byte piece of every row is aligned
  const dim3 grid((unsigned)((a->out_features + kBN - 1) / kBN), (unsigned)((a->rows + kBM - 1) / kBM));
  if (grid.y > 65535u) return BNN_ERR_SHAPE;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream_);
  for (int l0 = 0; l0 < a->n_levels; l0 += BNN_PRUNE_LEVELS_PER_LAUNCH) {
    const int levels = a->n_levels - l0 < BNN_PRUNE_LEVELS_PER_LAUNCH ? a->n_levels - l0 : BNN_PRUNE_LEVELS_PER_LAUNCH;
    p.level0 = l0;
    if (!bf) launch_levels<float, float>(p, levels, grid, st);
    else if (a->y_dtype == BNN_BF16) launch_levels<__bf16, __bf16>(p, levels, grid, st);
    else launch_levels<__bf16, float>(p, levels, grid, st);
  }
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}
