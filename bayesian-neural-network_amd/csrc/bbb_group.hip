// F7 groups of Thompson-sampling BNN bandits: the decision forward under posterior draws (bnn_bbb_group_fwd) and the whole
// training half of one bandit update (bnn_bbb_group_train) of BNN_Bandit (reinforcement_learning/bandits.py:17-54) for G
// agents, one workgroup per agent, in one launch each.  The structure is F6's (mlp_group.hip): an agent's update is a chain
// of up to 64 dependent minibatch steps, each S passes of a few small GEMMs, so the chain runs inside one workgroup,
// separated by workgroup barriers only, and agents never wait on each other.
//
// Exact fp32 (v_fma_f32) in every math mode.  Every GEMM element is one fma chain over k ascending (block_gemm, shared with
// F6), every other sum a fixed loop or a fixed-shape reduction: no float atomics, replays are bit-for-bit, and an agent's
// bits do not depend on G or on its place in the group.
//
// Per minibatch and draw s: the weights are sampled ONCE into the agent's global workspace (w = mu + softplus(rho) eps)
// and the GEMMs read them from there -- the forward of layers 0 and 1 from a transposed copy [in, out], so that the 16
// columns a quarter-wave reads at one k are 64 contiguous bytes (F6's forward reads them stride `in` apart), the hidden
// gradient of layer 1 from the copy as stored.  eps is kept beside them: the weight-gradient epilogues need it again
// (d/drho), and regenerating it there would cost a whole Philox group per element (a thread's tile columns are 16 apart).
// The per-draw gradients are summed over s in two accumulators of the workspace, G = sum_s t_s and H = sum_s t_s eps_s
// (include/bnn_hip.h F7), each element always touched by the same thread of a phase, the phases separated by barriers; one
// linear pass then forms g_mu, g_rho and runs Adam on the twenty-four (mu, rho) x (parameter, moments) streams.
//
// LDS, as F6: x [batch, in], h1, h2 [batch, hidden] (h2 becomes dL/dh2 in place), dL/dh1 [batch, hidden]: 4 x 32 KiB at
// the limits, plus the per-row vectors.
#include "mlp_group_common.h"
#include "bnn_prior.h"

namespace bnn {

struct BgHyper {
  double beta1, beta2;
  float beta2f, omb1, omb2, eps, wd;
};

struct BgK {
  const bnn_bbb_group_agent* agents;
  int B, I, H, S, A, max_batches;
  BgHyper hp;
  PriorAll prior;
  float beta[BNN_MLP_GROUP_MAX_BATCHES];
};

// Flat element offsets of the six sampled tensors (w1 b1 w2 b2 w3 b3) and the workspace's planes (floats).
struct BgLayout {
  int o[6], n[6];
  int P;          // elements of one plane, padded to 4
  __host__ __device__ BgLayout(int I, int H) {
    n[0] = H * I; n[1] = H; n[2] = H * H; n[3] = H; n[4] = H; n[5] = 1;
    int acc = 0;
    for (int q = 0; q < 6; ++q) {
      o[q] = acc;
      acc += n[q];
    }
    P = (acc + 3) & ~3;
  }
  // planes: w (weights transposed), eps, G, H: P each; then layer 1's weights as stored
  __host__ __device__ size_t floats() const { return (size_t)4 * P + (size_t)((n[2] + 3) & ~3); }
};

// One draw of one tensor of logical shape [N, K] (a bias: [1, out]): thread per Philox group (4 consecutive k of a row).
// wt[k * N + n] = w (the transposed copy), wn[n * K + k] = w when wn; TRAIN: eps kept, and the prior's share of t_s,
// pt = scale * d log_p / dw, starts (first) or joins the accumulators G, Hh.  stats: log q and log p of the draw are added
// to the thread's lq, lp in the thread's fixed order.
template <bool TRAIN>
__device__ __forceinline__ void bg_sample_tensor(const float* mu, const float* rho, int N, int K, uint32_t tensor_id,
                                                 uint32_t gsample, uint32_t k0, uint32_t k1, bool zero_eps, const PriorAll& pr,
                                                 float scale, bool first, bool stats, float* wt, float* wn, float* epso,
                                                 float* G, float* Hh, float& lq, float& lp) {
  const int gpr = (K + 3) >> 2;
  const int groups = N * gpr;
  for (int grp = threadIdx.x; grp < groups; grp += kMgThreads) {
    const int n = grp / gpr, kq = grp - n * gpr;
    float e[4] = {0.f, 0.f, 0.f, 0.f};
    if (!zero_eps) philox_normal4((uint32_t)grp, gsample, tensor_id, k0, k1, e);
#pragma unroll
    for (int slot = 0; slot < 4; ++slot) {
      const int k = kq * 4 + slot;
      if (k < K) {
        const int i = n * K + k;
        const float m = mu[i];
        const float sg = zero_eps ? 0.f : softplus(rho[i]);
        const float w = __builtin_fmaf(sg, e[slot], m);
        wt[k * N + n] = w;
        if (wn) wn[i] = w;
        if (TRAIN) {
          epso[i] = e[slot];
          const float pt = scale * prior_dlogp(pr, w);
          if (first) {
            G[i] = pt;
            Hh[i] = pt * e[slot];
          } else {
            G[i] += pt;
            Hh[i] = __builtin_fmaf(pt, e[slot], Hh[i]);
          }
          if (stats) {
            // log N(w; mu, sigma) with w - mu = sigma eps: c0 - log sigma - eps^2 / 2
            lq += __builtin_fmaf(-0.5f * e[slot], e[slot], kC0 - fast_log(sg));
            lp += prior_logp(pr, w);
          }
        }
      }
    }
  }
}

// One draw of the whole network into the workspace.
template <bool TRAIN>
__device__ __forceinline__ void bg_sample(const bnn_bbb_group_agent& ag, const BgLayout& L, int I, int H, uint32_t gsample,
                                          bool zero_eps, const PriorAll& pr, float scale, bool first, bool stats, float& lq,
                                          float& lp) {
  const uint32_t k0 = (uint32_t)ag.eps_seed, k1 = (uint32_t)(ag.eps_seed >> 32);
  float* wt = ag.workspace;
  float* epso = wt + L.P;
  float* G = epso + L.P;
  float* Hh = G + L.P;
  float* w2n = Hh + L.P;
#pragma unroll
  for (int q = 0; q < 6; ++q) {
    const int l = q >> 1, isb = q & 1;
    const int N = isb ? 1 : (l == 2 ? 1 : H);
    const int K = isb ? (l == 2 ? 1 : H) : (l == 0 ? I : H);
    const int o = L.o[q];
    bg_sample_tensor<TRAIN>(ag.param[4 * l + 2 * isb], ag.param[4 * l + 2 * isb + 1], N, K, (uint32_t)(4 * l + isb), gsample,
                            k0, k1, zero_eps, pr, scale, first, stats, wt + o, q == 2 ? w2n : nullptr, epso + o, G + o, Hh + o,
                            lq, lp);
  }
}

// The forward of rows [B, I] (xs, LDS) through the sampled network of the workspace: h1s, h2s [B, H], zs [B] (LDS).  The
// caller has put a barrier between the draw's stores and this.  Ends with a barrier.
__device__ __forceinline__ void bg_forward(const float* ws, const BgLayout& L, int B, int I, int H, const float* xs, float* h1s,
                                           float* h2s, float* zs) {
  const float* w1t = ws + L.o[0];
  const float* b1 = ws + L.o[1];
  const float* w2t = ws + L.o[2];
  const float* b2 = ws + L.o[3];
  const float* w3 = ws + L.o[4];
  const float* b3 = ws + L.o[5];
  block_gemm<2, 8>(B, H, I, [&](int m, int k) { return xs[m * I + k]; }, [&](int k, int n) { return w1t[k * H + n]; },
                   [&](int m, int n, float v) { h1s[m * H + n] = fmaxf(v + b1[n], 0.f); });
  __syncthreads();
  block_gemm<2, 8>(B, H, H, [&](int m, int k) { return h1s[m * H + k]; }, [&](int k, int n) { return w2t[k * H + n]; },
                   [&](int m, int n, float v) { h2s[m * H + n] = fmaxf(v + b2[n], 0.f); });
  __syncthreads();
  for (int b = threadIdx.x; b < B; b += kMgThreads) {
    float z = 0.f;
    for (int k = 0; k < H; ++k) z = __builtin_fmaf(h2s[b * H + k], w3[k], z);
    zs[b] = z + b3[0];
  }
  __syncthreads();
}

__global__ __launch_bounds__(kMgThreads) void bbb_group_fwd_kernel(BgK p) {
  __shared__ float xs[kMgX];
  __shared__ float h1s[kMgH];
  __shared__ float h2s[kMgH];
  __shared__ float zs[BNN_MLP_GROUP_MAX_BATCH];
  const bnn_bbb_group_agent& ag = p.agents[blockIdx.x];
  const int A = p.A, I = p.I, H = p.H;
  const BgLayout L(I, H);
  for (int e = threadIdx.x; e < A * I; e += kMgThreads) xs[e] = ag.rows[e];
  const bool zero = ag.eps_mode == BNN_EPS_ZERO;                // block-uniform
  const int ns = zero ? 1 : p.S;
  const uint32_t c = zero ? 0u : *ag.sample_counter;
  float lq = 0.f, lp = 0.f;
  for (int s = 0; s < ns; ++s) {
    bg_sample<false>(ag, L, I, H, c + (uint32_t)s, zero, p.prior, 0.f, false, false, lq, lp);
    __syncthreads();                                            // the draw's stores (and xs), then the GEMMs' loads
    bg_forward(ag.workspace, L, A, I, H, xs, h1s, h2s, zs);
    for (int r = threadIdx.x; r < A; r += kMgThreads) ag.outputs[s * A + r] = zs[r];
    __syncthreads();                                            // zs and the workspace are rewritten by the next draw
  }
}

__global__ __launch_bounds__(kMgThreads) void bbb_group_train_kernel(BgK p) {
  __shared__ float xs[kMgX];
  __shared__ float h1s[kMgH];
  __shared__ float h2s[kMgH];                                   // h2, then dL/dh2 in place
  __shared__ float gh1s[kMgH];                                  // dL/dh1
  __shared__ float zs[BNN_MLP_GROUP_MAX_BATCH];
  __shared__ float ys[BNN_MLP_GROUP_MAX_BATCH];
  __shared__ float gzs[BNN_MLP_GROUP_MAX_BATCH];
  __shared__ float red[kMgThreads / 64];
  const bnn_bbb_group_agent& ag = p.agents[blockIdx.x];
  int nb = *ag.n_batches;
  nb = nb < 0 ? 0 : (nb > p.max_batches ? p.max_batches : nb);
  if (nb == 0) return;                                          // block-uniform
  const int B = p.B, I = p.I, H = p.H, S = p.S;
  const BgLayout L(I, H);
  const uint32_t step0 = *ag.step;
  const uint32_t c0 = *ag.sample_counter;
  const double lr = (double)*ag.lr;
  const float inv_s = 1.0f / (float)S;
  float* ws = ag.workspace;
  const float* epsw = ws + L.P;
  float* G = ws + 2 * L.P;
  float* Hh = ws + 3 * L.P;
  const float* w2n = ws + 4 * L.P;
  const int tid = threadIdx.x;
  float slq = 0.f, slp = 0.f, snll = 0.f;                       // thread 0's sums over the draws of the last minibatch
  for (int j = 0; j < nb; ++j) {
    // The previous minibatch's Adam stores were followed by a __syncthreads() (vector stores complete before the barrier,
    // all waves of the workgroup share this CU's L1): this minibatch's loads see the updated parameters.
    const float* xg = ag.slab + (size_t)j * B * I;
    for (int e = tid; e < B * I; e += kMgThreads) xs[e] = xg[e];
    for (int b = tid; b < B; b += kMgThreads) ys[b] = ag.targets[(size_t)j * B + b];
    const float beta = p.beta[j];
    const bool last = j == nb - 1;                              // block-uniform: the statistics are reported for it only
    for (int s = 0; s < S; ++s) {
      float lq = 0.f, lp = 0.f;
      // t_s's prior share: -(beta / S) d log_p / dw
      bg_sample<true>(ag, L, I, H, c0 + (uint32_t)(j * S + s), false, p.prior, -beta * inv_s, s == 0, last, lq, lp);
      __syncthreads();                                          // the draw's stores (and xs, ys), then the loads below
      if (last) {
        const float tq = block_sum(lq, red);
        const float tp = block_sum(lp, red);
        if (tid == 0) {
          slq += tq;
          slp += tp;
        }
      }
      bg_forward(ws, L, B, I, H, xs, h1s, h2s, zs);

      // nll_s = -sum_b log N(y_b; z_b, 1); d(nll_s / S) / dz_b = (z_b - y_b) / S
      for (int b = tid; b < B; b += kMgThreads) gzs[b] = (zs[b] - ys[b]) * inv_s;
      if (last && tid == 0) {
        float a = 0.f;
        for (int b = 0; b < B; ++b) {
          const float r = zs[b] - ys[b];
          a += __builtin_fmaf(0.5f * r, r, -kC0);
        }
        snll += a;
      }
      __syncthreads();
      // layer 2: dw3 = dz^T h2, db3 = sum dz (read h2 before it turns into its gradient)
      for (int h = tid; h <= H; h += kMgThreads) {
        float a = 0.f;
        if (h < H)
          for (int b = 0; b < B; ++b) a = __builtin_fmaf(gzs[b], h2s[b * H + h], a);
        else
          for (int b = 0; b < B; ++b) a += gzs[b];
        const int i = h < H ? L.o[4] + h : L.o[5];
        G[i] += a;
        Hh[i] = __builtin_fmaf(a, epsw[i], Hh[i]);
      }
      __syncthreads();
      // dL/dh2 = dz w3 where h2 > 0 (each element rewritten by the thread that reads it)
      const float* w3 = ws + L.o[4];
      for (int e = tid; e < B * H; e += kMgThreads) {
        const int b = e / H, h = e - b * H;
        h2s[e] = h2s[e] > 0.f ? gzs[b] * w3[h] : 0.f;
      }
      __syncthreads();
      // dL/dh1 = dL/dh2 W2 where h1 > 0: W2 as stored, [out = k][in = n]
      block_gemm<2, 8>(B, H, H, [&](int m, int k) { return h2s[m * H + k]; }, [&](int k, int n) { return w2n[k * H + n]; },
                       [&](int m, int n, float v) { gh1s[m * H + n] = h1s[m * H + n] > 0.f ? v : 0.f; });
      __syncthreads();
      // dW2 = dh2^T h1 and dW1 = dh1^T x join the accumulators in the GEMMs' epilogues; the bias gradients are column sums
      block_gemm<4, 8>(H, H, B, [&](int m, int k) { return h2s[k * H + m]; }, [&](int k, int n) { return h1s[k * H + n]; },
                       [&](int m, int n, float v) {
                         const int i = L.o[2] + m * H + n;
                         G[i] += v;
                         Hh[i] = __builtin_fmaf(v, epsw[i], Hh[i]);
                       });
      block_gemm<4, 8>(H, I, B, [&](int m, int k) { return gh1s[k * H + m]; }, [&](int k, int n) { return xs[k * I + n]; },
                       [&](int m, int n, float v) {
                         const int i = L.o[0] + m * I + n;
                         G[i] += v;
                         Hh[i] = __builtin_fmaf(v, epsw[i], Hh[i]);
                       });
      for (int o = tid; o < 2 * H; o += kMgThreads) {
        const float* g = o < H ? h2s : gh1s;
        const int cidx = o < H ? o : o - H;
        float a = 0.f;
        for (int b = 0; b < B; ++b) a += g[b * H + cidx];
        const int i = (o < H ? L.o[3] : L.o[1]) + cidx;
        G[i] += a;
        Hh[i] = __builtin_fmaf(a, epsw[i], Hh[i]);
      }
      __syncthreads();                                          // the accumulators, then the next draw or Adam
    }

    // Adam's scalars of step t = step0 + j + 1: bias corrections in fp64, as torch forms them on the host
    const uint32_t t = step0 + (uint32_t)j + 1u;
    const double bc1 = 1.0 - pow(p.hp.beta1, (double)t);
    const double bc2 = 1.0 - pow(p.hp.beta2, (double)t);
    const AdamScalars as{(float)(lr / bc1), (float)sqrt(bc2), p.hp.omb1, p.hp.omb2, p.hp.beta2f, p.hp.eps, p.hp.wd};
    // g_mu = G, g_rho = (H - beta / sigma) sigmoid(rho): the log_q terms in closed form (through w they cancel in mu)
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      const int pm = 4 * (q >> 1) + 2 * (q & 1), pr = pm + 1;
      float* mu = ag.param[pm];
      float* rho = ag.param[pr];
      const int o = L.o[q];
      for (int e = tid; e < L.n[q]; e += kMgThreads) {
        const float r = rho[e];
        const float g_rho = (Hh[o + e] - beta * __builtin_amdgcn_rcpf(softplus(r))) * sigmoidf(r);
        adam_elem(mu, ag.exp_avg[pm], ag.exp_avg_sq[pm], e, G[o + e], as);
        adam_elem(rho, ag.exp_avg[pr], ag.exp_avg_sq[pr], e, g_rho, as);
      }
    }
    __syncthreads();                                            // the parameter stores above, then the next minibatch's loads
  }
  if (tid == 0) {
    const float beta = p.beta[nb - 1];
    const float mlp = slp * inv_s, mlq = slq * inv_s, mnll = snll * inv_s;
    ag.loss_info[0] = beta * mlq - beta * mlp + mnll;
    ag.loss_info[1] = mlp;
    ag.loss_info[2] = mlq;
    ag.loss_info[3] = mnll;
    *ag.step = step0 + (uint32_t)nb;
    *ag.sample_counter = c0 + (uint32_t)(nb * S);
  }
}

}  // namespace bnn

using namespace bnn;

static bool bg_shape_ok(int in_features, int hidden) {
  return in_features >= 1 && in_features <= BNN_MLP_GROUP_MAX_IN && hidden >= 1 && hidden <= BNN_MLP_GROUP_MAX_HIDDEN;
}

extern "C" size_t bnn_bbb_group_workspace_bytes(int32_t in_features, int32_t hidden) {
  if (!bg_shape_ok(in_features, hidden)) return 0;
  const BgLayout L(in_features, hidden);
  return (L.floats() * sizeof(float) + 255) & ~(size_t)255;
}

// The shared shape, the prior and the host copy of the agent blocks (include/bnn_hip.h F7).
static int check_bbb_group(const bnn_bbb_group_args* a, bool train) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_bbb_group_args)) return BNN_ERR_ABI;
  if (a->n_agents < 1 || a->n_agents > BNN_MLP_GROUP_MAX_AGENTS) return BNN_ERR_SHAPE;
  if (!bg_shape_ok(a->in_features, a->hidden) || a->out_features != BNN_MLP_GROUP_MAX_OUT) return BNN_ERR_SHAPE;
  if (a->n_samples < 1 || a->n_samples > BNN_BBB_GROUP_MAX_SAMPLES) return BNN_ERR_SHAPE;
  if (train) {
    if (a->batch < 1 || a->batch > BNN_MLP_GROUP_MAX_BATCH || a->max_batches < 1 || a->max_batches > BNN_MLP_GROUP_MAX_BATCHES)
      return BNN_ERR_SHAPE;
    if (!(a->beta1 >= 0.0 && a->beta1 < 1.0) || !(a->beta2 >= 0.0 && a->beta2 < 1.0) || !(a->eps >= 0.0) ||
        !(a->weight_decay >= 0.0))
      return BNN_ERR_SHAPE;
    if (const int rc = prior_check(a->prior)) return rc;
    if (a->prior.kind == BNN_PRIOR_MIXTURE && (!(a->prior.pi >= 0.f) || !(a->prior.pi <= 1.f))) return BNN_ERR_SHAPE;
  } else if (a->n_rows < 1 || a->n_rows > BNN_MLP_GROUP_MAX_BATCH) {
    return BNN_ERR_SHAPE;
  }
  if (!a->agents_host || !a->agents) return BNN_ERR_NULL;
  if (a->agents_bytes != (int64_t)a->n_agents * (int64_t)sizeof(bnn_bbb_group_agent)) return BNN_ERR_SHAPE;
  if (misaligned(a->agents, 8)) return BNN_ERR_ALIGN;
  if (a->workspace_bytes < (int64_t)bnn_bbb_group_workspace_bytes(a->in_features, a->hidden)) return BNN_ERR_WORKSPACE;
  for (int g = 0; g < a->n_agents; ++g) {
    const bnn_bbb_group_agent& ag = a->agents_host[g];
    for (int i = 0; i < 12; ++i) {
      if (!ag.param[i]) return BNN_ERR_NULL;
      if (misaligned(ag.param[i], 4)) return BNN_ERR_ALIGN;
      if (train) {
        if (!ag.exp_avg[i] || !ag.exp_avg_sq[i]) return BNN_ERR_NULL;
        if (misaligned(ag.exp_avg[i], 4) || misaligned(ag.exp_avg_sq[i], 4)) return BNN_ERR_ALIGN;
      }
    }
    if (!ag.workspace) return BNN_ERR_WORKSPACE;
    if (misaligned(ag.workspace, 16)) return BNN_ERR_ALIGN;
    if (train) {
      const void* req[] = {ag.step, ag.lr, ag.slab, ag.targets, ag.n_batches, ag.loss_info, ag.sample_counter};
      for (const void* p : req) {
        if (!p) return BNN_ERR_NULL;
        if (misaligned(p, 4)) return BNN_ERR_ALIGN;
      }
    } else {
      if (ag.eps_mode != BNN_EPS_PHILOX && ag.eps_mode != BNN_EPS_ZERO) return BNN_ERR_ENUM;
      if (!ag.rows || !ag.outputs || (ag.eps_mode == BNN_EPS_PHILOX && !ag.sample_counter)) return BNN_ERR_NULL;
      if (misaligned(ag.rows, 4) || misaligned(ag.outputs, 4) || misaligned(ag.sample_counter, 4)) return BNN_ERR_ALIGN;
    }
  }
  return BNN_OK;
}

static void bg_fill(BgK& k, const bnn_bbb_group_args* a) {
  k.agents = a->agents;
  k.B = a->batch; k.I = a->in_features; k.H = a->hidden; k.S = a->n_samples; k.A = a->n_rows; k.max_batches = a->max_batches;
  k.hp.beta1 = a->beta1;
  k.hp.beta2 = a->beta2;
  k.hp.beta2f = (float)a->beta2;
  k.hp.omb1 = (float)(1.0 - a->beta1);
  k.hp.omb2 = (float)(1.0 - a->beta2);
  k.hp.eps = (float)a->eps;
  k.hp.wd = (float)a->weight_decay;
  k.prior = prior_all_make(a->prior);          // (the forward validates no prior: an unusable one gives zeros it never reads)
  for (int j = 0; j < BNN_MLP_GROUP_MAX_BATCHES; ++j) k.beta[j] = a->beta[j];
}

extern "C" int bnn_bbb_group_fwd(const bnn_bbb_group_args* a, void* stream_) {
  const int rc = check_bbb_group(a, false);
  if (rc) return rc;
  BgK k;
  bg_fill(k, a);
  hipLaunchKernelGGL(bbb_group_fwd_kernel, dim3((unsigned)a->n_agents), dim3(kMgThreads), 0,
                     reinterpret_cast<hipStream_t>(stream_), k);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}

extern "C" int bnn_bbb_group_train(const bnn_bbb_group_args* a, void* stream_) {
  const int rc = check_bbb_group(a, true);
  if (rc) return rc;
  BgK k;
  bg_fill(k, a);
  hipLaunchKernelGGL(bbb_group_train_kernel, dim3((unsigned)a->n_agents), dim3(kMgThreads), 0,
                     reinterpret_cast<hipStream_t>(stream_), k);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}
