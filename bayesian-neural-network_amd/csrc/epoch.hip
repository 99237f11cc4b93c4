// F8 device-resident training epochs: the data-loader half of the reference's epoch loop (classification/class_task.py:67-79,
// regression/reg_task.py:60-74 over a DataLoader(shuffle=True, drop_last=True)) -- the epoch's permutation
// (bnn_epoch_permutation) and, per minibatch, ONE launch that gathers the rows into a captured training step's static
// buffers, casts them and looks beta up (bnn_epoch_stage).  The minibatch number and the epoch number are device words, so
// the host neither reads nor writes data between the first and the last step of an epoch.
#include "bnn_device.h"
#include "../../include/bnn_hip.h"

namespace bnn {

constexpr int kPermBlock = 256;                   // a key per thread
constexpr int kPermTile = 2048;                   // (key, position) pairs staged in LDS per round: 16 KiB
constexpr int kStageBlock = 256;                  // 4 waves: a wave per minibatch row

// Rank by counting: thread p counts the pairs (key_q << 32 | q) below its own over LDS-staged tiles of all N pairs (every
// block forms them itself: N / 4 Philox calls per block against N comparisons per thread) and writes order[rank] = p.
// key_q = word (q & 3) of Philox4x32-R((q >> 2, epoch, 2, 1), seed): include/bnn_hip.h F8.  The pairs are distinct (they
// end in q), so the ranks are a permutation of 0 .. N-1 whatever the keys.
__global__ __launch_bounds__(kPermBlock) void epoch_permutation_kernel(bnn_epoch_perm_args a) {
  __shared__ unsigned long long tile[kPermTile];
  const uint32_t N = (uint32_t)a.n_rows, epoch = *a.epoch;
  const uint32_t k0 = (uint32_t)a.seed, k1 = (uint32_t)(a.seed >> 32);
  const uint32_t p = blockIdx.x * kPermBlock + threadIdx.x;
  unsigned long long mine = 0ull;                                                  // (a thread past N counts nothing)
  if (p < N) {
    const uint4 r = philox4x32<>(make_uint4(p >> 2, epoch, 2u, 1u), k0, k1);
    const uint32_t key = (p & 3) == 0 ? r.x : (p & 3) == 1 ? r.y : (p & 3) == 2 ? r.z : r.w;
    mine = ((unsigned long long)key << 32) | p;
  }
  uint32_t rank = 0;
  for (uint32_t base = 0; base < N; base += kPermTile) {
    __syncthreads();                                                               // the previous tile has been read
    for (uint32_t g = threadIdx.x; g < kPermTile / 4; g += kPermBlock) {           // a thread per Philox call: four pairs
      const uint32_t q = base + 4 * g;
      const uint4 r = philox4x32<>(make_uint4(q >> 2, epoch, 2u, 1u), k0, k1);
      const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
      for (int i = 0; i < 4; ++i)                                                  // padding sorts above every pair
        tile[4 * g + i] = q + i < N ? (((unsigned long long)w[i] << 32) | (q + i)) : ~0ull;
    }
    __syncthreads();
    const uint32_t left = N - base;
    const uint32_t n = left < (uint32_t)kPermTile ? (left + 7u) & ~7u : (uint32_t)kPermTile;   // <= kPermTile
#pragma unroll 1
    for (uint32_t i = 0; i < n; i += 8) {
#pragma unroll
      for (int u = 0; u < 8; ++u) rank += tile[i + u] < mine ? 1u : 0u;           // wave-uniform address: an LDS broadcast
    }
  }
  if (p < N && rank < N) a.order[rank] = (int32_t)p;
}

// A wave per minibatch row r: row order[j B + r] (or j B + r) of the data set into x_out[r] (+ its bf16 copy), its target
// into targets_out[r].  Block 0 also files the previous step's loss words and writes beta.  The block that arrives last
// advances the minibatch word (every block has read it by then) and, at the end of the epoch, the epoch word.
template <bool U8, bool VEC>
__global__ __launch_bounds__(kStageBlock) void epoch_stage_kernel(bnn_epoch_stage_args a) {
  const uint32_t j = *a.batch_index;
  const uint32_t B = (uint32_t)a.batch_size, M = (uint32_t)a.num_batches;
  if (j >= M) return;                                                              // (never left so by this kernel) block-uniform
  const int lane = threadIdx.x & 63, d = a.row_dim;
  const uint32_t r = blockIdx.x * (kStageBlock / 64) + (threadIdx.x >> 6);
  if (r < B) {                                                                     // wave-uniform
    const uint32_t q = j * B + r;                                                  // < B M <= N
    long i = a.order ? (long)a.order[q] : (long)q;
    if (i < 0 || i >= a.n_rows) i = q;                                             // a caller's order is not trusted with addresses
    float* dst = a.x_out + (size_t)r * d;
    __bf16* dst16 = a.x_bf16_out ? reinterpret_cast<__bf16*>(a.x_bf16_out) + (size_t)r * d : nullptr;
    const uint8_t* src8 = reinterpret_cast<const uint8_t*>(a.x) + (size_t)i * d;
    const float* src = reinterpret_cast<const float*>(a.x) + (size_t)i * d;
    if (VEC) {                                                                     // d % 4 == 0: 16-byte stores
      for (int c = lane; c < (d >> 2); c += 64) {
        float4 v;
        if (U8) {
          const uchar4 u = reinterpret_cast<const uchar4*>(src8)[c];
          v = make_float4(__fdiv_rn((float)u.x, 255.0f), __fdiv_rn((float)u.y, 255.0f), __fdiv_rn((float)u.z, 255.0f),
                          __fdiv_rn((float)u.w, 255.0f));
        } else {
          v = reinterpret_cast<const float4*>(src)[c];
        }
        reinterpret_cast<float4*>(dst)[c] = v;
        if (dst16) {
          bf16x4 o;
          o[0] = (__bf16)v.x; o[1] = (__bf16)v.y; o[2] = (__bf16)v.z; o[3] = (__bf16)v.w;
          reinterpret_cast<bf16x4*>(dst16)[c] = o;
        }
      }
    } else {
      for (int c = lane; c < d; c += 64) {
        const float v = U8 ? __fdiv_rn((float)src8[c], 255.0f) : src[c];
        dst[c] = v;
        if (dst16) dst16[c] = (__bf16)v;
      }
    }
    if (a.target_dim == 0) {
      if (lane == 0) reinterpret_cast<int64_t*>(a.targets_out)[r] = reinterpret_cast<const int64_t*>(a.targets)[i];
    } else {
      const int k = a.target_dim;
      for (int c = lane; c < k; c += 64)
        reinterpret_cast<float*>(a.targets_out)[(size_t)r * k + c] = reinterpret_cast<const float*>(a.targets)[(size_t)i * k + c];
    }
  }
  if (blockIdx.x == 0) {
    if (a.loss_history && j > 0 && (int)threadIdx.x < a.loss_cols)
      a.loss_history[(size_t)(j - 1) * a.loss_cols + threadIdx.x] = *a.loss_src[threadIdx.x];
    if (a.beta_table && threadIdx.x == 64) *a.beta = a.beta_table[j];
  }
  // arrival ticket: j is in a register of every thread of this block before its thread 0 arrives
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t arrived = atomicAdd(a.ticket, 1u);
    if (arrived == gridDim.x - 1) {
      atomicExch(a.ticket, 0u);
      if (j + 1 == M) {
        *a.batch_index = 0u;
        *a.epoch += 1u;
      } else {
        *a.batch_index = j + 1u;
      }
    }
  }
}

}  // namespace bnn

using namespace bnn;

extern "C" int bnn_epoch_permutation(const bnn_epoch_perm_args* a, void* stream_) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_epoch_perm_args)) return BNN_ERR_ABI;
  if (a->n_rows < 1 || a->n_rows > BNN_EPOCH_MAX_ROWS) return BNN_ERR_SHAPE;
  if (!a->epoch || !a->order) return BNN_ERR_NULL;
  if (misaligned(a->epoch, 4) || misaligned(a->order, 4)) return BNN_ERR_ALIGN;
  const unsigned blocks = (unsigned)((a->n_rows + kPermBlock - 1) / kPermBlock);
  hipLaunchKernelGGL(epoch_permutation_kernel, dim3(blocks), dim3(kPermBlock), 0, reinterpret_cast<hipStream_t>(stream_), *a);
  hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}

extern "C" int bnn_epoch_stage(const bnn_epoch_stage_args* a, void* stream_) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_epoch_stage_args)) return BNN_ERR_ABI;
  if (a->n_rows < 1 || a->n_rows > BNN_EPOCH_MAX_ROWS || a->row_dim < 1 || a->batch_size < 1 || a->num_batches < 1 ||
      a->target_dim < 0 || (int64_t)a->batch_size * a->num_batches > a->n_rows)
    return BNN_ERR_SHAPE;
  if (a->loss_cols < 0 || a->loss_cols > BNN_EPOCH_MAX_LOSS_COLS || (a->loss_history && a->loss_cols < 1)) return BNN_ERR_SHAPE;
  if (a->x_dtype != BNN_EPOCH_X_F32 && a->x_dtype != BNN_EPOCH_X_U8) return BNN_ERR_ENUM;
  const void* req[] = {a->x, a->targets, a->batch_index, a->epoch, a->ticket, a->x_out, a->targets_out};
  for (const void* p : req)
    if (!p) return BNN_ERR_NULL;
  if (a->beta_table && !a->beta) return BNN_ERR_NULL;
  if (a->loss_history)
    for (int c = 0; c < a->loss_cols; ++c)
      if (!a->loss_src[c]) return BNN_ERR_NULL;
  const bool u8 = a->x_dtype == BNN_EPOCH_X_U8;
  const void* w4[] = {a->order, a->beta_table, a->batch_index, a->epoch, a->ticket, a->x_out, a->beta, a->loss_history,
                      a->loss_src[0], a->loss_src[1], a->loss_src[2], a->loss_src[3], u8 ? nullptr : a->x};
  for (const void* p : w4)
    if (misaligned(p, 4)) return BNN_ERR_ALIGN;
  const uintptr_t tal = a->target_dim ? 4 : 8;
  if (misaligned(a->x_bf16_out, 2) || misaligned(a->targets, tal) || misaligned(a->targets_out, tal)) return BNN_ERR_ALIGN;
  // rows start on the vector's boundary when the base does and d % 4 == 0 (uint8: 4-byte loads; fp32: 16-byte loads)
  const bool vec = a->row_dim % 4 == 0 && !misaligned(a->x, u8 ? 4 : 16) && !misaligned(a->x_out, 16) && !misaligned(a->x_bf16_out, 8);
  const dim3 grid((unsigned)((a->batch_size + kStageBlock / 64 - 1) / (kStageBlock / 64))), block(kStageBlock);
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (u8 && vec) hipLaunchKernelGGL((epoch_stage_kernel<true, true>), grid, block, 0, stream, *a);
  else if (u8) hipLaunchKernelGGL((epoch_stage_kernel<true, false>), grid, block, 0, stream, *a);
  else if (vec) hipLaunchKernelGGL((epoch_stage_kernel<false, true>), grid, block, 0, stream, *a);
  else hipLaunchKernelGGL((epoch_stage_kernel<false, false>), grid, block, 0, stream, *a);
  hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}
