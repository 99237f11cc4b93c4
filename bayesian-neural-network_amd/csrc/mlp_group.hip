// F6 groups of epsilon-greedy MLP bandits: the decision forward (bnn_mlp_group_fwd) and the whole training half of one
// bandit update (bnn_mlp_group_train) of Greedy_Bandit (reinforcement_learning/bandits.py:59-85) for G agents, one
// workgroup per agent, in one launch each.
//
// An agent's update is a chain of up to 64 dependent minibatch steps, each a few small GEMMs (119-100-100-1 at batch 64:
// about 3.5 M FMAs); the chain, not the chip, is the bound, so the steps run back to back inside one workgroup, separated
// by workgroup barriers only.  Agents never wait on each other: no grid-wide seam, spin or counter.
//
// Exact fp32 in every math mode: fp32 FMA (v_fma_f32) only, bnn_set_math does not reach these kernels -- the per-CU chain
// is latency-bound, so bf16 operands would buy little and cost the reference's arithmetic.  Every output element is one
// fma chain over k in ascending order, every other sum a fixed sequential loop: no float atomics, replays are bit-for-bit.
//
// Per minibatch, in LDS: x [batch, in], h1 and h2 [batch, hidden] (h2 becomes dL/dh2 in place), dL/dh1 [batch, hidden]:
// 4 x 32 KiB at the limits.  The weights (88 KB at 119-100-100-1) stay in L2 / L1: they are read by the GEMMs and
// written by the Adam epilogues of the same workgroup.
#include "mlp_group_common.h"

namespace bnn {

// The forward of rows [B, I] (xs, LDS) through Linear -> ReLU -> Linear -> ReLU -> Linear(H -> 1): h1s, h2s [B, H] (LDS),
// zs [B] (LDS).  Ends with a barrier.
__device__ __forceinline__ void mlp_forward(const bnn_mlp_group_agent& ag, int B, int I, int H, const float* xs, float* h1s,
                                            float* h2s, float* zs) {
  const float* w1 = ag.param[0];
  const float* b1 = ag.param[1];
  const float* w2 = ag.param[2];
  const float* b2 = ag.param[3];
  const float* w3 = ag.param[4];
  const float* b3 = ag.param[5];
  block_gemm<2, 8>(B, H, I, [&](int m, int k) { return xs[m * I + k]; }, [&](int k, int n) { return w1[n * I + k]; },
                   [&](int m, int n, float v) { h1s[m * H + n] = fmaxf(v + b1[n], 0.f); });
  __syncthreads();
  block_gemm<2, 8>(B, H, H, [&](int m, int k) { return h1s[m * H + k]; }, [&](int k, int n) { return w2[n * H + k]; },
                   [&](int m, int n, float v) { h2s[m * H + n] = fmaxf(v + b2[n], 0.f); });
  __syncthreads();
  for (int b = threadIdx.x; b < B; b += kMgThreads) {
    float z = 0.f;
    for (int k = 0; k < H; ++k) z = __builtin_fmaf(h2s[b * H + k], w3[k], z);
    zs[b] = z + b3[0];
  }
  __syncthreads();
}

__global__ __launch_bounds__(kMgThreads) void mlp_group_fwd_kernel(const bnn_mlp_group_agent* agents, int A, int I, int H) {
  __shared__ float xs[kMgX];
  __shared__ float h1s[kMgH];
  __shared__ float h2s[kMgH];
  __shared__ float zs[BNN_MLP_GROUP_MAX_BATCH];
  const bnn_mlp_group_agent& ag = agents[blockIdx.x];
  for (int e = threadIdx.x; e < A * I; e += kMgThreads) xs[e] = ag.rows[e];
  __syncthreads();
  mlp_forward(ag, A, I, H, xs, h1s, h2s, zs);
  for (int r = threadIdx.x; r < A; r += kMgThreads) ag.outputs[r] = zs[r];
}

struct MgHyper {
  double beta1, beta2;
  float beta2f, omb1, omb2, eps, wd;
};

__global__ __launch_bounds__(kMgThreads) void mlp_group_train_kernel(const bnn_mlp_group_agent* agents, int B, int I, int H,
                                                                      int max_batches, MgHyper hp) {
  __shared__ float xs[kMgX];
  __shared__ float h1s[kMgH];
  __shared__ float h2s[kMgH];                                 // h2, then dL/dh2 in place
  __shared__ float gh1s[kMgH];                                // dL/dh1
  __shared__ float zs[BNN_MLP_GROUP_MAX_BATCH];
  __shared__ float ys[BNN_MLP_GROUP_MAX_BATCH];
  __shared__ float gzs[BNN_MLP_GROUP_MAX_BATCH];
  __shared__ float gw3s[BNN_MLP_GROUP_MAX_HIDDEN + 1];        // dL/dw3, then dL/db3
  const bnn_mlp_group_agent& ag = agents[blockIdx.x];
  int nb = *ag.n_batches;
  nb = nb < 0 ? 0 : (nb > max_batches ? max_batches : nb);
  if (nb == 0) return;                                        // block-uniform
  const uint32_t step0 = *ag.step;
  const double lr = (double)*ag.lr;
  float* w1 = ag.param[0];
  float* b1 = ag.param[1];
  float* w2 = ag.param[2];
  float* b2 = ag.param[3];
  float* w3 = ag.param[4];
  float* b3 = ag.param[5];
  const int tid = threadIdx.x;
  float loss = 0.f;                                           // thread 0's
  for (int j = 0; j < nb; ++j) {
    // The previous minibatch's Adam stores of the weights were followed by a __syncthreads() (its vector stores
    // complete -- s_waitcnt vmcnt(0) -- before the barrier, and all waves of the workgroup share this CU's L1), so
    // the loads of this minibatch see the updated weights.  The order is: global stores, barrier, next loads.
    const float* xg = ag.slab + (size_t)j * B * I;
    for (int e = tid; e < B * I; e += kMgThreads) xs[e] = xg[e];
    for (int b = tid; b < B; b += kMgThreads) ys[b] = ag.targets[(size_t)j * B + b];
    __syncthreads();
    mlp_forward(ag, B, I, H, xs, h1s, h2s, zs);

    // mse_loss(z.squeeze(), y, reduction='sum') and dL/dz = 2 (z - y)
    for (int b = tid; b < B; b += kMgThreads) gzs[b] = 2.f * (zs[b] - ys[b]);
    if (tid == 0) {
      float s = 0.f;
      for (int b = 0; b < B; ++b) {
        const float r = zs[b] - ys[b];
        s = __builtin_fmaf(r, r, s);
      }
      loss = s;
    }
    __syncthreads();
    // dL/dw3 = dz^T h2, dL/db3 = sum dz (read h2 before it turns into its gradient)
    for (int h = tid; h <= H; h += kMgThreads) {
      float s = 0.f;
      if (h < H)
        for (int b = 0; b < B; ++b) s = __builtin_fmaf(gzs[b], h2s[b * H + h], s);
      else
        for (int b = 0; b < B; ++b) s += gzs[b];
      gw3s[h] = s;
    }
    __syncthreads();
    // dL/dh2 = dz w3 where h2 > 0 (each element rewritten by the thread that reads it)
    for (int e = tid; e < B * H; e += kMgThreads) {
      const int b = e / H, h = e - b * H;
      h2s[e] = h2s[e] > 0.f ? gzs[b] * w3[h] : 0.f;
    }
    __syncthreads();

    // Adam's scalars of step t = step0 + j + 1: bias corrections in fp64, as torch forms them on the host
    const uint32_t t = step0 + (uint32_t)j + 1u;
    const double bc1 = 1.0 - pow(hp.beta1, (double)t);
    const double bc2 = 1.0 - pow(hp.beta2, (double)t);
    const AdamScalars as{(float)(lr / bc1), (float)sqrt(bc2), hp.omb1, hp.omb2, hp.beta2f, hp.eps, hp.wd};

    // dL/dh1 = dL/dh2 W2 where h1 > 0 (reads W2 before its update below); w3 and b3 (read above) are updated here
    block_gemm<2, 8>(B, H, H, [&](int m, int k) { return h2s[m * H + k]; }, [&](int k, int n) { return w2[k * H + n]; },
                     [&](int m, int n, float v) { gh1s[m * H + n] = h1s[m * H + n] > 0.f ? v : 0.f; });
    for (int h = tid; h <= H; h += kMgThreads) {
      if (h < H) adam_elem(w3, ag.exp_avg[4], ag.exp_avg_sq[4], h, gw3s[h], as);
      else adam_elem(b3, ag.exp_avg[5], ag.exp_avg_sq[5], 0, gw3s[H], as);
    }
    __syncthreads();
    // dL/dW2 = dh2^T h1 and dL/dW1 = dh1^T x, each element's Adam update in the GEMM's epilogue; the bias gradients are
    // column sums of dh2 / dh1.  Nothing in this phase reads a weight.
    block_gemm<4, 8>(H, H, B, [&](int m, int k) { return h2s[k * H + m]; }, [&](int k, int n) { return h1s[k * H + n]; },
                     [&](int m, int n, float v) { adam_elem(w2, ag.exp_avg[2], ag.exp_avg_sq[2], m * H + n, v, as); });
    block_gemm<4, 8>(H, I, B, [&](int m, int k) { return gh1s[k * H + m]; }, [&](int k, int n) { return xs[k * I + n]; },
                     [&](int m, int n, float v) { adam_elem(w1, ag.exp_avg[0], ag.exp_avg_sq[0], m * I + n, v, as); });
    for (int o = tid; o < 2 * H; o += kMgThreads) {
      const float* g = o < H ? h2s : gh1s;
      const int c = o < H ? o : o - H;
      float s = 0.f;
      for (int b = 0; b < B; ++b) s += g[b * H + c];
      if (o < H) adam_elem(b2, ag.exp_avg[3], ag.exp_avg_sq[3], c, s, as);
      else adam_elem(b1, ag.exp_avg[1], ag.exp_avg_sq[1], c, s, as);
    }
    __syncthreads();                                          // the weight stores above, then the next minibatch's loads
  }
  if (tid == 0) {
    *ag.loss = loss;
    *ag.step = step0 + (uint32_t)nb;
  }
}

}  // namespace bnn

using namespace bnn;

// The shared shape and the host copy of the agent blocks (include/bnn_hip.h F6); train additionally needs the optimiser
// and minibatch pointers, fwd the rows and outputs.
static int check_mlp_group(const bnn_mlp_group_args* a, bool train) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_mlp_group_args)) return BNN_ERR_ABI;
  if (a->n_agents < 1 || a->n_agents > BNN_MLP_GROUP_MAX_AGENTS) return BNN_ERR_SHAPE;
  if (a->in_features < 1 || a->in_features > BNN_MLP_GROUP_MAX_IN || a->hidden < 1 || a->hidden > BNN_MLP_GROUP_MAX_HIDDEN ||
      a->out_features != BNN_MLP_GROUP_MAX_OUT)
    return BNN_ERR_SHAPE;
  if (train) {
    if (a->batch < 1 || a->batch > BNN_MLP_GROUP_MAX_BATCH || a->max_batches < 1 || a->max_batches > BNN_MLP_GROUP_MAX_BATCHES)
      return BNN_ERR_SHAPE;
    if (!(a->beta1 >= 0.0 && a->beta1 < 1.0) || !(a->beta2 >= 0.0 && a->beta2 < 1.0) || !(a->eps >= 0.0) ||
        !(a->weight_decay >= 0.0))
      return BNN_ERR_SHAPE;
  } else if (a->n_rows < 1 || a->n_rows > BNN_MLP_GROUP_MAX_BATCH) {
    return BNN_ERR_SHAPE;
  }
  if (!a->agents_host || !a->agents) return BNN_ERR_NULL;
  if (a->agents_bytes != (int64_t)a->n_agents * (int64_t)sizeof(bnn_mlp_group_agent)) return BNN_ERR_SHAPE;
  if (misaligned(a->agents, 8)) return BNN_ERR_ALIGN;
  for (int g = 0; g < a->n_agents; ++g) {
    const bnn_mlp_group_agent& ag = a->agents_host[g];
    for (int i = 0; i < 6; ++i) {
      if (!ag.param[i]) return BNN_ERR_NULL;
      if (misaligned(ag.param[i], 4)) return BNN_ERR_ALIGN;
      if (train) {
        if (!ag.exp_avg[i] || !ag.exp_avg_sq[i]) return BNN_ERR_NULL;
        if (misaligned(ag.exp_avg[i], 4) || misaligned(ag.exp_avg_sq[i], 4)) return BNN_ERR_ALIGN;
      }
    }
    if (train) {
      const void* req[] = {ag.step, ag.lr, ag.slab, ag.targets, ag.n_batches, ag.loss};
      for (const void* p : req) {
        if (!p) return BNN_ERR_NULL;
        if (misaligned(p, 4)) return BNN_ERR_ALIGN;
      }
    } else {
      if (!ag.rows || !ag.outputs) return BNN_ERR_NULL;
      if (misaligned(ag.rows, 4) || misaligned(ag.outputs, 4)) return BNN_ERR_ALIGN;
    }
  }
  return BNN_OK;
}

extern "C" int bnn_mlp_group_fwd(const bnn_mlp_group_args* a, void* stream_) {
  const int rc = check_mlp_group(a, false);
  if (rc) return rc;
  hipLaunchKernelGGL(mlp_group_fwd_kernel, dim3((unsigned)a->n_agents), dim3(kMgThreads), 0,
                     reinterpret_cast<hipStream_t>(stream_), a->agents, a->n_rows, a->in_features, a->hidden);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}

extern "C" int bnn_mlp_group_train(const bnn_mlp_group_args* a, void* stream_) {
  const int rc = check_mlp_group(a, true);
  if (rc) return rc;
  MgHyper hp;
  hp.beta1 = a->beta1;
  hp.beta2 = a->beta2;
  hp.beta2f = (float)a->beta2;
  hp.omb1 = (float)(1.0 - a->beta1);
  hp.omb2 = (float)(1.0 - a->beta2);
  hp.eps = (float)a->eps;
  hp.wd = (float)a->weight_decay;
  hipLaunchKernelGGL(mlp_group_train_kernel, dim3((unsigned)a->n_agents), dim3(kMgThreads), 0,
                     reinterpret_cast<hipStream_t>(stream_), a->agents, a->batch, a->in_features, a->hidden, a->max_batches, hp);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}
