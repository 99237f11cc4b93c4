// F5 contextual bandit: the device half of Bandit.update (reinforcement_learning/base_bandit.py:37-99) -- the decision
// rows, the decision itself, reward, regret, replay ring (bnn_bandit_rows / bnn_bandit_act) and the shuffled replay
// minibatches (bnn_bandit_replay).  Small latency-bound launches: one block each except the gather; the step number t
// is a device word, so nothing here needs the host between bandit steps.
#include "bnn_device.h"
#include "../../include/bnn_hip.h"

namespace bnn {

constexpr int kRowsBlock = 256;
constexpr int kSortBlock = 1024;
constexpr int kGatherBlock = 256;                 // 4 waves: a wave per slab row

// The bandit's random stream of step t: counter (0, t, 0, 1) -- word 3 = 1 keeps it apart from every eps counter.
__device__ __forceinline__ uint4 bandit_draw(uint32_t t, uint64_t seed) {
  return philox4x32<>(make_uint4(0u, t, 0u, 1u), (uint32_t)seed, (uint32_t)(seed >> 32));
}

// min(floor(u n), n - 1) in fp32, as the host restates it
__device__ __forceinline__ long pick(uint32_t r, long n) {
  const long v = (long)floorf(u01(r) * (float)n);
  return v < n - 1 ? v : n - 1;
}

// The kernel bodies take the argument block by reference: the F5 kernels pass their by-value argument, the F6 group kernels
// (bnn_bandit_*_group) block g of the device array -- the same code on either.
__device__ __forceinline__ void bandit_rows_body(const bnn_bandit_act_args& a) {
  __shared__ long s_idx;
  const uint32_t t = *a.step;
  if ((int64_t)t >= a.max_steps) return;                                          // block-uniform
  if (threadIdx.x == 0) {
    long i = -1;
    if (a.indices && (int64_t)t < a.n_indices) i = (long)a.indices[t];
    if (i < 0 || i >= a.n_contexts) i = pick(bandit_draw(t, a.seed).w, a.n_contexts);
    s_idx = i;
    *a.cur_index = (int32_t)i;
  }
  __syncthreads();
  const long i = s_idx;
  const int d = a.context_dim, A = a.n_actions, w = d + A;
  const float* src = a.x + (size_t)i * d;
  for (int e = threadIdx.x; e < A * w; e += kRowsBlock) {
    const int r = e / w, c = e - r * w;
    a.rows[e] = c < d ? src[c] : (c - d == r ? 1.f : 0.f);
  }
}

__global__ __launch_bounds__(kRowsBlock) void bandit_rows_kernel(bnn_bandit_act_args a) { bandit_rows_body(a); }
__global__ __launch_bounds__(kRowsBlock) void bandit_rows_group_kernel(const bnn_bandit_act_args* g) {
  bandit_rows_body(g[blockIdx.x]);
}

// One wave: lane a sums its action's S outputs, the wave takes the argmax (ties to the highest index), lane 0 does the rest.
__device__ __forceinline__ void bandit_act_body(const bnn_bandit_act_args& a) {
  const uint32_t t = *a.step;
  if ((int64_t)t >= a.max_steps) return;                                          // wave-uniform
  const int lane = threadIdx.x, A = a.n_actions;
  float v = -INFINITY;
  int bi = -1;
  if (lane < A) {
    v = a.outputs[lane];
    for (int s = 1; s < a.n_samples; ++s) v += a.outputs[(size_t)s * a.output_sample_stride + lane];
    bi = lane;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(v, off, 64);
    const int oi = __shfl_xor(bi, off, 64);
    if (ov > v || (ov == v && oi > bi)) {
      v = ov;
      bi = oi;
    }
  }
  if (lane != 0) return;
  const uint4 r = bandit_draw(t, a.seed);
  int act = bi < 0 ? A - 1 : bi;                                                  // (all outputs NaN: the last action)
  if (u01(r.x) < a.epsilon) act = (int)pick(r.y, A);
  const long i = *a.cur_index;
  const long k = (long)a.labels[i];
  if (k < 0 || k >= a.n_labels) return;                                          // (the host checks the labels up front)
  const float* rw = a.rewards + ((size_t)k * A + act) * 3;
  const float reward = u01(r.z) > rw[2] ? rw[0] : rw[1];
  a.actions[t] = act;
  a.reward_out[t] = reward;
  a.regrets[t + 1] = a.regrets[t] + ((double)a.oracle[k] - (double)reward);
  a.counts[k * A + act] += 1;
  const uint32_t slot = t % (uint32_t)a.buffer_size;
  a.ring_index[slot] = (int32_t)i;
  a.ring_action[slot] = act;
  a.ring_reward[slot] = reward;
  *a.step = t + 1;
  if (a.sample_counter) *a.sample_counter += a.sample_counter_inc;
}

__global__ __launch_bounds__(64) void bandit_act_kernel(bnn_bandit_act_args a) { bandit_act_body(a); }
__global__ __launch_bounds__(64) void bandit_act_group_kernel(const bnn_bandit_act_args* g) { bandit_act_body(g[blockIdx.x]); }

// The pool of base_bandit.py:77-84 for l entries: its size, and the entry at position p.
__device__ __forceinline__ uint32_t pool_size(uint32_t l, uint32_t bs, uint32_t buf) {
  if (l <= bs) return l ? bs : 0u;
  if (l < buf) return l / bs * bs;
  return buf;
}
__device__ __forceinline__ uint32_t pool_entry(uint32_t p, uint32_t l, uint32_t bs, uint32_t P) {
  if (l <= bs) {
    const uint32_t m = bs / l + 1u;
    return (m * l - bs + p) % l;
  }
  return l - P + p;
}

// One block: keys (Philox word of the position) ++ position, bitonic-sorted ascending in LDS, then the ring slot of every
// shuffled position into the workspace.
__device__ __forceinline__ void bandit_shuffle_body(const bnn_bandit_replay_args& a) {
  __shared__ unsigned long long kv[BNN_BANDIT_MAX_BUFFER];                        // 64 KiB
  const uint32_t l = *a.step, t = l - 1u;
  const uint32_t bs = (uint32_t)a.batch_size, buf = (uint32_t)a.buffer_size;
  const uint32_t P = pool_size(l, bs, buf);
  if (threadIdx.x == 0 && a.n_batches) *a.n_batches = (int32_t)(P / bs);
  if (P == 0) return;                                                             // block-uniform
  uint32_t n2 = 1;
  while (n2 < P) n2 <<= 1;
  const uint32_t k0 = (uint32_t)a.seed, k1 = (uint32_t)(a.seed >> 32);
  for (uint32_t p = threadIdx.x; p < n2; p += kSortBlock) {
    unsigned long long v = ~0ull;                                                 // padding sorts last
    if (p < P) {
      const uint4 r = philox4x32<>(make_uint4(p >> 2, t, 1u, 1u), k0, k1);
      const uint32_t key = (p & 3) == 0 ? r.x : (p & 3) == 1 ? r.y : (p & 3) == 2 ? r.z : r.w;
      v = ((unsigned long long)key << 32) | p;
    }
    kv[p] = v;
  }
  __syncthreads();
  for (uint32_t k = 2; k <= n2; k <<= 1) {
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t e = threadIdx.x; e < (n2 >> 1); e += kSortBlock) {
        const uint32_t i = 2 * j * (e / j) + (e % j);                            // lower element of the pair; partner i + j
        const bool asc = (i & k) == 0;
        const unsigned long long x = kv[i], y = kv[i + j];
        if ((x > y) == asc) {
          kv[i] = y;
          kv[i + j] = x;
        }
      }
      __syncthreads();
    }
  }
  for (uint32_t q = threadIdx.x; q < P; q += kSortBlock) {
    const uint32_t p = (uint32_t)kv[q];
    a.workspace[q] = (int32_t)(pool_entry(p, l, bs, P) % buf);
  }
}

__global__ __launch_bounds__(kSortBlock) void bandit_shuffle_kernel(bnn_bandit_replay_args a) { bandit_shuffle_body(a); }
__global__ __launch_bounds__(kSortBlock) void bandit_shuffle_group_kernel(const bnn_bandit_replay_args* g) {
  bandit_shuffle_body(g[blockIdx.x]);
}

// A wave per slab row q < pool: x[i] ++ one_hot(action) and the reward of the entry in ring slot workspace[q].
__device__ __forceinline__ void bandit_gather_body(const bnn_bandit_replay_args& a, uint32_t bx) {
  const uint32_t l = *a.step;
  const uint32_t P = pool_size(l, (uint32_t)a.batch_size, (uint32_t)a.buffer_size);
  const uint32_t q = bx * (kGatherBlock / 64) + (threadIdx.x >> 6);
  if (q >= P) return;                                                             // wave-uniform
  const int lane = threadIdx.x & 63, d = a.context_dim, A = a.n_actions, w = d + A;
  const int slot = a.workspace[q];
  const long i = a.ring_index[slot];
  const int act = a.ring_action[slot];
  const float* src = a.x + (size_t)i * d;
  float* dst = a.slab + (size_t)q * w;
  for (int c = lane; c < w; c += 64) dst[c] = c < d ? src[c] : (c - d == act ? 1.f : 0.f);
  if (lane == 0) a.targets[q] = a.ring_reward[slot];
}

__global__ __launch_bounds__(kGatherBlock) void bandit_gather_kernel(bnn_bandit_replay_args a) { bandit_gather_body(a, blockIdx.x); }
// grid (blocks of the largest agent's buffer, G): row g gathers agent g
__global__ __launch_bounds__(kGatherBlock) void bandit_gather_group_kernel(const bnn_bandit_replay_args* g) {
  bandit_gather_body(g[blockIdx.y], blockIdx.x);
}

}  // namespace bnn

using namespace bnn;

static int check_act(const bnn_bandit_act_args* a) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_bandit_act_args)) return BNN_ERR_ABI;
  if (a->n_actions < 2 || a->n_actions > BNN_BANDIT_MAX_ACTIONS || a->n_labels < 1 || a->n_samples < 1) return BNN_ERR_SHAPE;
  if (a->output_sample_stride != 0 && a->output_sample_stride != a->n_actions) return BNN_ERR_SHAPE;
  if (a->context_dim < 1 || a->n_contexts < 1 || a->n_contexts > INT32_MAX || a->max_steps < 1 || a->max_steps > UINT32_MAX - 1u)
    return BNN_ERR_SHAPE;
  if (a->buffer_size < 1 || a->buffer_size > BNN_BANDIT_MAX_BUFFER || a->n_indices < 0) return BNN_ERR_SHAPE;
  if (!(a->epsilon >= 0.f && a->epsilon <= 1.f)) return BNN_ERR_SHAPE;                 // NaN fails both
  const void* req[] = {a->x, a->labels, a->rewards, a->oracle, a->outputs, a->step, a->cur_index, a->rows, a->actions,
                       a->reward_out, a->regrets, a->counts, a->ring_index, a->ring_action, a->ring_reward};
  for (const void* p : req)
    if (!p) return BNN_ERR_NULL;
  if (a->n_indices > 0 && !a->indices) return BNN_ERR_NULL;
  const void* w8[] = {a->labels, a->indices, a->actions, a->regrets, a->counts};
  for (const void* p : w8)
    if (misaligned(p, 8)) return BNN_ERR_ALIGN;
  const void* w4[] = {a->x, a->rewards, a->oracle, a->outputs, a->step, a->cur_index, a->rows, a->reward_out, a->ring_index,
                      a->ring_action, a->ring_reward, a->sample_counter};
  for (const void* p : w4)
    if (misaligned(p, 4)) return BNN_ERR_ALIGN;
  return BNN_OK;
}

extern "C" int bnn_bandit_rows(const bnn_bandit_act_args* a, void* stream_) {
  const int rc = check_act(a);
  if (rc) return rc;
  hipLaunchKernelGGL(bandit_rows_kernel, dim3(1), dim3(kRowsBlock), 0, reinterpret_cast<hipStream_t>(stream_), *a);
  hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}

extern "C" int bnn_bandit_act(const bnn_bandit_act_args* a, void* stream_) {
  const int rc = check_act(a);
  if (rc) return rc;
  hipLaunchKernelGGL(bandit_act_kernel, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream_), *a);
  hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}

static int check_replay(const bnn_bandit_replay_args* a) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_bandit_replay_args)) return BNN_ERR_ABI;
  if (a->batch_size < 1 || a->num_batches < 1 || a->buffer_size < 1 || a->buffer_size > BNN_BANDIT_MAX_BUFFER) return BNN_ERR_SHAPE;
  if (a->buffer_size % a->batch_size != 0 || (int64_t)a->num_batches * a->batch_size < a->buffer_size) return BNN_ERR_SHAPE;
  if (a->context_dim < 1 || a->n_actions < 2 || a->n_actions > BNN_BANDIT_MAX_ACTIONS || a->n_contexts < 1 ||
      a->n_contexts > INT32_MAX)
    return BNN_ERR_SHAPE;
  const void* req[] = {a->step, a->x, a->ring_index, a->ring_action, a->ring_reward, a->workspace, a->slab, a->targets};
  for (const void* p : req)
    if (!p) return BNN_ERR_NULL;
  const void* w4[] = {a->step, a->x, a->ring_index, a->ring_action, a->ring_reward, a->workspace, a->slab, a->targets, a->n_batches};
  for (const void* p : w4)
    if (misaligned(p, 4)) return BNN_ERR_ALIGN;
  return BNN_OK;
}

extern "C" int bnn_bandit_replay(const bnn_bandit_replay_args* a, void* stream_) {
  const int rc = check_replay(a);
  if (rc) return rc;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  hipLaunchKernelGGL(bandit_shuffle_kernel, dim3(1), dim3(kSortBlock), 0, stream, *a);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return (int)err;
  const unsigned blocks = (unsigned)((a->buffer_size + kGatherBlock / 64 - 1) / (kGatherBlock / 64));
  hipLaunchKernelGGL(bandit_gather_kernel, dim3(blocks), dim3(kGatherBlock), 0, stream, *a);
  err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}

// ---------------------------------------------------------------------------------------------------- F6 group forms
// The host copy of the blocks is validated block by block; the kernels read the device copy (include/bnn_hip.h F6).
template <class Block>
static int check_group(const bnn_bandit_group_args* g, int (*check)(const Block*)) {
  if (!g) return BNN_ERR_NULL;
  if (g->struct_bytes != sizeof(bnn_bandit_group_args)) return BNN_ERR_ABI;
  if (g->n_agents < 1 || g->n_agents > BNN_MLP_GROUP_MAX_AGENTS) return BNN_ERR_SHAPE;
  if (!g->blocks_host || !g->blocks) return BNN_ERR_NULL;
  if (g->blocks_bytes != (int64_t)g->n_agents * (int64_t)sizeof(Block)) return BNN_ERR_SHAPE;
  if (misaligned(g->blocks, 8)) return BNN_ERR_ALIGN;
  const Block* h = static_cast<const Block*>(g->blocks_host);
  for (int i = 0; i < g->n_agents; ++i) {
    const int rc = check(h + i);
    if (rc) return rc;
  }
  return BNN_OK;
}

extern "C" int bnn_bandit_rows_group(const bnn_bandit_group_args* g, void* stream_) {
  const int rc = check_group<bnn_bandit_act_args>(g, check_act);
  if (rc) return rc;
  hipLaunchKernelGGL(bandit_rows_group_kernel, dim3((unsigned)g->n_agents), dim3(kRowsBlock), 0,
                     reinterpret_cast<hipStream_t>(stream_), static_cast<const bnn_bandit_act_args*>(g->blocks));
  hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}

extern "C" int bnn_bandit_act_group(const bnn_bandit_group_args* g, void* stream_) {
  const int rc = check_group<bnn_bandit_act_args>(g, check_act);
  if (rc) return rc;
  hipLaunchKernelGGL(bandit_act_group_kernel, dim3((unsigned)g->n_agents), dim3(64), 0,
                     reinterpret_cast<hipStream_t>(stream_), static_cast<const bnn_bandit_act_args*>(g->blocks));
  hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}

extern "C" int bnn_bandit_replay_group(const bnn_bandit_group_args* g, void* stream_) {
  const int rc = check_group<bnn_bandit_replay_args>(g, check_replay);
  if (rc) return rc;
  const bnn_bandit_replay_args* h = static_cast<const bnn_bandit_replay_args*>(g->blocks_host);
  int32_t buf = 1;
  for (int i = 0; i < g->n_agents; ++i) buf = h[i].buffer_size > buf ? h[i].buffer_size : buf;
  const bnn_bandit_replay_args* d = static_cast<const bnn_bandit_replay_args*>(g->blocks);
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  hipLaunchKernelGGL(bandit_shuffle_group_kernel, dim3((unsigned)g->n_agents), dim3(kSortBlock), 0, stream, d);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return (int)err;
  const unsigned blocks = (unsigned)((buf + kGatherBlock / 64 - 1) / (kGatherBlock / 64));
  hipLaunchKernelGGL(bandit_gather_group_kernel, dim3(blocks, (unsigned)g->n_agents), dim3(kGatherBlock), 0, stream, d);
  err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}
