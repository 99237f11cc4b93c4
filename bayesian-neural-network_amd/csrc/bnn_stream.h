// The pieces every streaming step over a list of parameter tensors shares (bnn_adam_step, bnn_sgd_step, bnn_sgmcmc_step,
// bnn_swag_step / bnn_swag_sample, bnn_ivon_draw / bnn_ivon_step): the chunk size, the float4 walk of a chunk with its
// masked tail, the ticketed hand-off by which a launch's last block advances the device words, and the layout of the
// per-tensor state inside one buffer.  One block = one kStreamChunk-element chunk of one tensor (ChunkList of
// bnn_device.h), 256 threads, kStreamIters rounds of one float4 per thread.
#pragma once
#include "bnn_device.h"

namespace bnn {

constexpr int kStreamChunk = 4096;
constexpr int kStreamIters = kStreamChunk / (256 * 4);

// elements i .. i + 3 of a tensor of n elements: one 16-byte access when all four exist, scalars (0 beyond n) otherwise
__device__ __forceinline__ void ld4(const float* __restrict__ src, long i, long n, bool full, float v[4]) {
  if (full) {
    const float4 q = *reinterpret_cast<const float4*>(src + i);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = i + j < n ? src[i + j] : 0.f;
  }
}

// the same of a bf16 tensor, widened: one 8-byte access when all four exist
__device__ __forceinline__ void ld4(const __bf16* __restrict__ src, long i, long n, bool full, float v[4]) {
  if (full) {
    const bf16x4 h = *reinterpret_cast<const bf16x4*>(src + i);
    v[0] = (float)h[0]; v[1] = (float)h[1]; v[2] = (float)h[2]; v[3] = (float)h[3];
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = i + j < n ? (float)src[i + j] : 0.f;
  }
}

__device__ __forceinline__ void st4(float* __restrict__ dst, long i, long n, bool full, const float v[4]) {
  if (full) {
    *reinterpret_cast<float4*>(dst + i) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (i + j < n) dst[i + j] = v[j];
  }
}

// The ticketed hand-off: every block of the launch has read the device words (a step, a count, a product) at its top and
// works with their OLD values; the block that arrives last runs advance(), which stores the new ones, so that a step is ONE
// launch and nobody waits.  Called by every thread of every block, at the end of the kernel.
//   The barrier: every wave of the block has read the words before thread 0 announces the block's arrival -- the last
// arriver overwrites them, and a wave that had not loaded them yet would work with the advanced values.
//   Two levels: device-scope atomics on ONE word serialise at the memory side (1170 of them were a ~4 us tail on the 24 us
// Adam launch); blocks count in 8 groups (ticket word 1 + blockIdx % 8, which block b shares with b + 8, b + 16, ...: group
// g has (grid - g + 7) / 8 members), each group's last arriver counts once on word 0, and the last of those is the
// launch's last block.  Both levels are left at zero for the next launch: ticket is 9 words, zero before the first launch.
template <class F>
__device__ __forceinline__ void last_block(uint32_t* ticket, F advance) {
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t g = blockIdx.x & 7u;
    const uint32_t in_group = (gridDim.x - g + 7u) >> 3;
    const uint32_t tk = __hip_atomic_fetch_add(ticket + 1 + g, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tk == in_group - 1u) {
      ticket[1 + g] = 0u;                                 // ready for the next launch
      const uint32_t groups = gridDim.x < 8u ? gridDim.x : 8u;
      const uint32_t top = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (top == groups - 1u) {
        advance();
        ticket[0] = 0u;
      }
    }
  }
}

// Host: the chunk list of a tensor list and where each tensor's state starts in a buffer that holds them all -- every tensor
// at a multiple of 64 elements (256 bytes), `stride` the elements of the whole.  BNN_OK, or BNN_ERR_SHAPE for an empty
// tensor, one of more than 2^34 elements (a noise stream's group index is 32 bits) or more chunks than a grid takes.
template <int MAX>
inline int state_offsets(ChunkList<MAX>& list, int n_tensors, const int64_t* numel, long (&off)[MAX], long& stride) {
  stride = 0;
  for (int t = 0; t < MAX; ++t) off[t] = 0;
  for (int t = 0; t < n_tensors; ++t) {
    if (numel[t] > ((int64_t)1 << 34)) return BNN_ERR_SHAPE;
    const int st = list.add(numel[t], kStreamChunk);
    if (st != BNN_OK) return st;
    off[t] = stride;
    stride += (numel[t] + 63) / 64 * 64;
  }
  return BNN_OK;
}

}  // namespace bnn
