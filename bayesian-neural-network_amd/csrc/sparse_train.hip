// F14 training the compressed network (include/bnn_hip.h F14): what a Bayes-by-backprop step over the survivors of an F13
// network needs beside bnn_sparse_fwd, the finalize / loss launches and bnn_adam_step.
//   bnn_sparse_elbo_terms     log q and log p of the kept weights and biases of up to 8 layers, per MC sample
//   bnn_sparse_bwd            one layer: g_mu_val, g_rho_val, g_b_mu, g_b_rho and optionally g_x
//   bnn_sparse_sigma_refresh  sigma = keep ? softplus(rho) : 0 over up to 8 segments
// Epsilon is the dense weight-space Philox map of F13 and is regenerated wherever it is needed; no float atomics; every sum
// has one order fixed by the shape alone.
//
// The partitions, and what bounds them (derived; the measured step times are in DESIGN.md F14).
// Terms.  A block is 1024 consecutive entries (or 256 biases) of one (layer, sample), threads over ENTRIES as in stage A of the
//   forward: the first survivor of a Philox group draws for the group.  Per entry: a binary search of row_ptr (11 cached loads at
//   1200 rows), a share of a Philox call, ~10 flops.  It is the generator that bounds it: one call per occupied group.
// Weights.  The unit of work is the entry: a wave owns 16 consecutive entries whatever rows they belong to, so rows of unequal
//   length cost what they hold.  A run = the (up to four) consecutive survivors of one row and one Philox group; per run and per 64
//   samples the wave makes ONE Philox call with lane = sample, and the sample loop reads a sample's four epsilons by readlane.
//   An entry's G_e,s is a dot over the batch of gz_s[o, :] (shared by the run) and x_s[c, :], both contiguous feature-major
//   rows: per entry, sample and 64 batch rows one 256-byte read of x (+ a quarter of one of gz at level 0) and one fma -- the
//   same gathered-row traffic as stage B of the forward, so the vector L1 rate bounds it where the forward's does, and the
//   Philox call per run and the wave's DPP sum (six dependent steps per entry and sample) are the fixed cost that shows at
//   high drop levels, where a run is one entry.
// Input gradient.  The forward over the transposed pattern: a block is (column group, sample, batch block <= 256 rows), stage A
//   (threads over the CSC entries) regenerates w into LDS, stage B (threads over batch rows) runs one ascending-o chain per
//   g_x element with (w, o) broadcast from LDS and gz feature-major.  The survivors of one Philox group lie in adjacent COLUMNS
//   here, so stage A makes one Philox call per entry (four times the forward's at level 0): the generator bounds stage A, the
//   L1 read rate stage B, as in the forward.
#include "bnn_device.h"
#include "bnn_prior.h"
#include "../../include/bnn_hip.h"
#include <math.h>

namespace bnn {
namespace {

constexpr int kTermSpan = 1024;        // entries per block of the terms kernel
constexpr int kTermThreads = 256;
constexpr int kWaveEntries = 16;       // entries per wave of the weight-gradient kernel
constexpr int kGxChunk = 512;          // entries per stage of the input-gradient kernel: 2 x 512 x 8 bytes of LDS
constexpr int kMaxCG = 32;

// eps_slot's value (bnn_device.h) with the loads left under the branches, where the compiler sinks the Box-Muller half a thread
// does not need: with eps_slot's select over four values the captured sparse step measured 0.5 - 1 % slower, so this form stays
__device__ __forceinline__ float pick4(const float n4[4], int slot) {
  return slot == 0 ? n4[0] : slot == 1 ? n4[1] : slot == 2 ? n4[2] : n4[3];
}

// the row of CSR entry j: the largest o in [0, n) with ptr[o] <= j (empty rows are stepped over)
__device__ __forceinline__ int row_of(const int* __restrict__ ptr, int n, int j) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (ptr[mid] <= j) lo = mid; else hi = mid;
  }
  return lo;
}

// ------------------------------------------------------------------------------------------------------------ ELBO terms
struct TermsL {
  const int* row_ptr;
  const uint16_t* col;
  const float* mu;
  const float* sigma;
  const float* b_mu;
  const float* b_sigma;
  const uint8_t* b_keep;
  int in, out, nnz;
  uint32_t layer_id;
  int first_block, entry_blocks, blocks;     // the layer's blocks: entry blocks, then bias blocks
};

struct TermsK {
  TermsL L[BNN_SPARSE_MAX_LAYERS];
  int n_layers, S, total_blocks;
  uint32_t k0, k1, sample_offset;
  const uint32_t* sample_counter;
  int prior_kind;
  PriorMix mix;
  double lp_const, inv2var;                  // Gaussian: c0 - log sigma_p, 1 / (2 sigma_p^2)
  float4* part;                              // [S][total_blocks]: (sum eps^2, sum w^2 | log mixture, sum log sigma, kept biases)
  float* log_prior;
  float* log_q;
};

__global__ __launch_bounds__(kTermThreads) void sparse_terms_kernel(const TermsK p) {
#pragma clang fp contract(off)
  __shared__ float red[kTermThreads / 64][4];
  const int b = blockIdx.x, s = blockIdx.y;
  int l = 0;
#pragma unroll 1
  while (l + 1 < p.n_layers && b >= p.L[l + 1].first_block) ++l;
  const TermsL& L = p.L[l];
  const int local = b - L.first_block;
  const uint32_t gs = p.sample_offset + (p.sample_counter ? *p.sample_counter : 0u) + (uint32_t)s;
  const bool gauss = p.prior_kind == BNN_PRIOR_GAUSS;
  const bool do_ls = s == 0;                                           // log sigma does not depend on the sample
  float e2 = 0.f, a = 0.f, ls = 0.f, cnt = 0.f;
  if (local < L.entry_blocks) {
    const int nnz = min(L.nnz, L.row_ptr[L.out]);
    const int span0 = local * kTermSpan, span1 = min(span0 + kTermSpan, nnz);
    const uint32_t gpr = eps_groups_per_row(L.in);
    for (int j = span0 + (int)threadIdx.x; j < span1; j += kTermThreads) {
      const int c = (int)L.col[j];
      const int o = row_of(L.row_ptr, L.out, j);
      const int row_lo = L.row_ptr[o], row_hi = L.row_ptr[o + 1];
      // the first survivor of a Philox group inside this span draws for the whole group
      const bool follower = j > span0 && j - 1 >= row_lo && ((int)L.col[j - 1] >> 2) == (c >> 2);
      if (follower) continue;
      float n4[4];
      philox_normal4((uint32_t)o * gpr + (uint32_t)(c >> 2), gs, eps_tensor_id(L.layer_id, kEpsWeight), p.k0, p.k1, n4);   // eps_group(o, c, gpr)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int jq = j + q;
        if (q > 0 && (jq >= span1 || jq >= row_hi)) break;
        const int cq = q == 0 ? c : (int)L.col[jq];
        if ((cq >> 2) != (c >> 2)) break;
        const float ev = pick4(n4, cq & 3);
        const float sg = L.sigma[jq];
        const float w = __builtin_fmaf(sg, ev, L.mu[jq]);
        e2 = __builtin_fmaf(ev, ev, e2);
        a = gauss ? __builtin_fmaf(w, w, a) : add_log(a, prior_mix_p(p.mix, w));
        if (do_ls) ls = add_log(ls, sg);
      }
    }
  } else {
    const int o = (local - L.entry_blocks) * kTermThreads + (int)threadIdx.x;
    if (o < L.out && L.b_keep[o]) {
      float n4[4];                                                     // eps_bias, with pick4
      philox_normal4((uint32_t)(o >> 2), gs, eps_tensor_id(L.layer_id, kEpsBias), p.k0, p.k1, n4);
      const float ev = pick4(n4, o & 3);
      const float sg = L.b_sigma[o];
      const float w = __builtin_fmaf(sg, ev, L.b_mu[o]);
      e2 = __builtin_fmaf(ev, ev, e2);
      a = gauss ? __builtin_fmaf(w, w, a) : add_log(a, prior_mix_p(p.mix, w));
      if (do_ls) ls = add_log(ls, sg);
      cnt = 1.f;
    }
  }
  // thread -> wave (DPP, fixed) -> block (wave order)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float r0 = wave_sum(e2), r1 = wave_sum(a), r2 = wave_sum(ls), r3 = wave_sum(cnt);
  if (lane == 0) {
    red[wave][0] = r0; red[wave][1] = r1; red[wave][2] = r2; red[wave][3] = r3;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float t0 = 0.f, t1 = 0.f, t2 = 0.f, t3 = 0.f;
    for (int w = 0; w < kTermThreads / 64; ++w) {
      t0 += red[w][0]; t1 += red[w][1]; t2 += red[w][2]; t3 += red[w][3];
    }
    p.part[(size_t)s * p.total_blocks + b] = make_float4(t0, t1, t2, t3);
  }
}

// one block per sample: each layer's partials in fp64, thread-strided then a fixed tree; per-layer fp32 rounding, then
// fp32 adds in layer order (what K4 does with the dense layers' statistics)
__global__ __launch_bounds__(kTermThreads) void sparse_terms_fold_kernel(const TermsK p) {
  __shared__ double sh[kTermThreads][4];
  const int s = blockIdx.x, t = threadIdx.x;
  float a_tot = 0.f, b_tot = 0.f;
  for (int l = 0; l < p.n_layers; ++l) {
    const TermsL& L = p.L[l];
    double v0 = 0, v1 = 0, v2 = 0, v3 = 0;
    for (int i = t; i < L.blocks; i += kTermThreads) {
      const float4 q = p.part[(size_t)s * p.total_blocks + L.first_block + i];
      const float4 q0 = p.part[(size_t)L.first_block + i];            // sample 0's: log sigma
      v0 += (double)q.x; v1 += (double)q.y; v2 += (double)q0.z; v3 += (double)q.w;
    }
    sh[t][0] = v0; sh[t][1] = v1; sh[t][2] = v2; sh[t][3] = v3;
    __syncthreads();
    for (int st = kTermThreads / 2; st > 0; st >>= 1) {
      if (t < st) {
#pragma unroll
        for (int k = 0; k < 4; ++k) sh[t][k] += sh[t + st][k];
      }
      __syncthreads();
    }
    if (t == 0) {
      const double cnt = (double)min(L.nnz, L.row_ptr[L.out]) + sh[0][3];
      const double lq = fold_log_q(cnt * kNegLogSqrt2Pi, sh[0][2], sh[0][0]);
      // fold_log_p's value, the count applied under the branch as this kernel was built (it counts the survivors itself)
      const double lp = p.prior_kind == BNN_PRIOR_GAUSS ? cnt * p.lp_const - sh[0][1] * p.inv2var : sh[0][1];
      a_tot += (float)lp;
      b_tot += (float)lq;
    }
    __syncthreads();
  }
  if (t == 0) {
    p.log_prior[s] = a_tot;
    p.log_q[s] = b_tot;
  }
}

// ------------------------------------------------------------------------------------------------------------ backward
struct BwdS {
  const int* row_ptr;
  const uint16_t* col;
  const float* mu;
  const float* rho;
  const int* col_ptr;
  const uint16_t* row;
  const int* perm;
  const float* b_mu;
  const float* b_rho;
  const uint8_t* b_keep;
  const float* x;
  const float* gz;
  const float* glp;
  const float* glq;
  float* g_mu;
  float* g_rho;
  float* g_bmu;
  float* g_brho;
  float* gx;
  int S, rows, in, out, nnz, x_per_sample, gx_relu_mask, entry_blocks;
  uint32_t k0, k1, layer_id, sample_offset;
  const uint32_t* sample_counter;
  int prior_kind;
  float inv_var_p, a1, a2, inv2var1, inv2var2, invvar1, invvar2;
};

// gz [S, out, rows] = gy (row-major [S, rows, out] or feature-major) * (y > 0)
__global__ __launch_bounds__(256) void sparse_gz_kernel(const float* __restrict__ gy, const float* __restrict__ y, float* __restrict__ gz,
                                                        int S, int rows, int out, int relu, int row_major) {
  const long n = (long)S * out * rows;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float g;
    if (row_major) {
      const int r = (int)(i % rows);
      const long so = i / rows;
      const int o = (int)(so % out);
      const long s = so / out;
      g = gy[((size_t)s * rows + r) * out + o];
    } else {
      g = gy[i];
    }
    gz[i] = (!relu || y[i] > 0.f) ? g : 0.f;
  }
}

__device__ __forceinline__ float lane_value(float v, int lane) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}

__global__ __launch_bounds__(256) void sparse_bwd_weights_kernel(const BwdS p) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int S = p.S, rows = p.rows, in = p.in, out = p.out;
  const uint32_t gs0 = p.sample_offset + (p.sample_counter ? *p.sample_counter : 0u);
  float cq = 0.f;                                                       // sum_s g_log_q[s], ascending
  if (p.glq)
    for (int s = 0; s < S; ++s) cq += p.glq[s];
  const size_t plane = (size_t)in * rows;

  if ((int)blockIdx.x >= p.entry_blocks) {
    // ---- bias: a wave per output feature, G = the row sum of gz
    const int o = ((int)blockIdx.x - p.entry_blocks) * 4 + wave;
    if (o >= out) return;                                               // wave-uniform; the kernel has no barrier
    if (!p.b_keep[o]) {
      if (lane == 0) {
        p.g_bmu[o] = 0.f;
        p.g_brho[o] = 0.f;
      }
      return;
    }
    const float bmu = p.b_mu[o], brh = p.b_rho[o];
    const float bsg = softplus(brh);
    float G = 0.f, H = 0.f;
    for (int sb = 0; sb < S; sb += 64) {
      float n4[4];                                                     // eps_bias, with pick4; lane = sample
      philox_normal4((uint32_t)(o >> 2), gs0 + (uint32_t)(sb + lane), eps_tensor_id(p.layer_id, kEpsBias), p.k0, p.k1, n4);
      const float el = pick4(n4, o & 3);
      const int ns = min(64, S - sb);
      for (int si = 0; si < ns; ++si) {
        const int s = sb + si;
        const float* __restrict__ gzr = p.gz + ((size_t)s * out + o) * rows;
        float acc = 0.f;
        for (int r = lane; r < rows; r += 64) acc += gzr[r];
        const float colsum = wave_sum(acc);
        const float ev = lane_value(el, si);
        const float glp = p.glp ? p.glp[s] : 0.f;
        const float w = __builtin_fmaf(bsg, ev, bmu);
        const float t = colsum + glp * prior_dlogp(p, w);
        G += t;
        H = __builtin_fmaf(t, ev, H);
      }
    }
    if (lane == 0) {
      p.g_bmu[o] = G;
      p.g_brho[o] = (H - cq * __builtin_amdgcn_rcpf(bsg)) * sigmoidf(brh);
    }
    return;
  }

  // ---- weights: this wave's 16 entries, run by run
  const int nnz = min(p.nnz, p.row_ptr[out]);
  int e = ((int)blockIdx.x * 4 + wave) * kWaveEntries;
  const int e_end = min(e + kWaveEntries, nnz);
  if (e >= e_end) return;                                               // wave-uniform
  int o = row_of(p.row_ptr, out, e);
  int row_end = p.row_ptr[o + 1];
  const uint32_t gpr = eps_groups_per_row(in);
  while (e < e_end) {
    while (row_end <= e && o + 1 < out) {                               // rows that end here (empty ones among them)
      ++o;
      row_end = p.row_ptr[o + 1];
    }
    const int lim = min(e_end, row_end);
    // the run: up to four consecutive survivors of row o in one Philox group (everything here is wave-uniform)
    int cc[4];
    bool ok[4];
    float mu[4], rh[4], sg[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int jq = min(e + q, nnz - 1);
      cc[q] = min((int)p.col[jq], in - 1);
      ok[q] = q == 0 || (ok[q - 1] && e + q < lim && (cc[q] >> 2) == (cc[0] >> 2));
      mu[q] = p.mu[jq];
      rh[q] = p.rho[jq];
      sg[q] = 1.f;
      if (ok[q]) sg[q] = softplus(rh[q]);                               // wave-uniform: a one-entry run takes one softplus
    }
    const int n = 1 + (int)ok[1] + (int)ok[2] + (int)ok[3];
    float G[4] = {0.f, 0.f, 0.f, 0.f}, H[4] = {0.f, 0.f, 0.f, 0.f};
    for (int sb = 0; sb < S; sb += 64) {
      float n4[4];
      philox_normal4(eps_group((uint32_t)o, cc[0], gpr), gs0 + (uint32_t)(sb + lane), eps_tensor_id(p.layer_id, kEpsWeight), p.k0, p.k1, n4);
      const int ns = min(64, S - sb);
      for (int si = 0; si < ns; ++si) {
        const int s = sb + si;
        const float* __restrict__ gzr = p.gz + ((size_t)s * out + o) * rows;
        const float* __restrict__ xs = p.x + (size_t)(p.x_per_sample > 0 ? s / p.x_per_sample : 0) * plane;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int r = lane; r < rows; r += 64) {
          const float g = gzr[r];
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (ok[q]) acc[q] = __builtin_fmaf(g, xs[(size_t)cc[q] * rows + r], acc[q]);
        }
        const float glp = p.glp ? p.glp[s] : 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if (!ok[q]) continue;                                         // wave-uniform: every lane is in the sum
          const float Gd = wave_sum(acc[q]);
          const float ev = lane_value(pick4(n4, cc[q] & 3), si);
          const float w = __builtin_fmaf(sg[q], ev, mu[q]);
          const float t = Gd + glp * prior_dlogp(p, w);
          G[q] += t;
          H[q] = __builtin_fmaf(t, ev, H[q]);
        }
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (ok[q] && lane == q) {
        p.g_mu[e + q] = G[q];
        p.g_rho[e + q] = (H[q] - cq * __builtin_amdgcn_rcpf(sg[q])) * sigmoidf(rh[q]);
      }
    }
    e += n;
  }
}

struct GxEntry {
  float w;
  int o;
};

__global__ __launch_bounds__(256) void sparse_bwd_input_kernel(const BwdS p, int CG) {
#pragma clang fp contract(off)
  __shared__ int s_cp[kMaxCG + 1];
  __shared__ GxEntry s_e[2][kGxChunk];
  const int t = threadIdx.x, nt = blockDim.x;
  const int out = p.out, in = p.in, rows = p.rows;
  const int c0 = blockIdx.x * CG;
  const int nc = min(CG, in - c0);
  const int s = blockIdx.y;
  const int r = blockIdx.z * nt + t;
  const bool live = r < rows;
  const uint32_t gs = p.sample_offset + (p.sample_counter ? *p.sample_counter : 0u) + (uint32_t)s;
  const int nnz = min(p.nnz, p.col_ptr[in]);
  if (t <= nc) s_cp[t] = min(max(p.col_ptr[c0 + t], 0), nnz);
  __syncthreads();
  const int j0 = s_cp[0], j1 = s_cp[nc];
  const float* __restrict__ gzp = p.gz + (size_t)s * out * rows;
  const float* __restrict__ xp = p.x + (size_t)(p.x_per_sample > 0 ? s / p.x_per_sample : 0) * in * rows;
  float* __restrict__ gxp = p.gx + (size_t)s * in * rows;
  const uint32_t gpr = eps_groups_per_row(in);
  auto emit = [&](int cl, float acc) {
    if (live) {
      const size_t at = (size_t)(c0 + cl) * rows + r;
      float v = acc;
      if (p.gx_relu_mask) v = xp[at] > 0.f ? v : 0.f;
      gxp[at] = v;
    }
  };
  int cl = 0;                                                           // the column the chain in `acc` belongs to (block-uniform)
  float acc = 0.f;
  int buf = 0;
  for (int ch0 = j0; ch0 < j1; ch0 += kGxChunk, buf ^= 1) {
    const int n = min(kGxChunk, j1 - ch0);
    GxEntry* __restrict__ se = s_e[buf];
    // ---- stage A: threads over the CSC entries
    for (int e = t; e < n; e += nt) {
      const int k = ch0 + e;
      const int o = min((int)p.row[k], out - 1);
      const int pm = min(max(p.perm[k], 0), nnz - 1);
      const int c = c0 + row_of(s_cp, nc, k);
      float n4[4];
      philox_normal4(eps_group((uint32_t)o, c, gpr), gs, eps_tensor_id(p.layer_id, kEpsWeight), p.k0, p.k1, n4);
      se[e].w = __builtin_fmaf(softplus(p.rho[pm]), pick4(n4, c & 3), p.mu[pm]);
      se[e].o = o;
    }
    __syncthreads();
    // ---- stage B: threads over batch rows, the chunk's entries in order
    int e = ch0;
    const int cend = ch0 + n;
    while (e < cend) {
      while (__builtin_amdgcn_readfirstlane(s_cp[cl + 1]) <= e) {       // columns that end here (empty ones among them)
        emit(cl, acc);
        acc = 0.f;
        ++cl;
      }
      const int hi = min(__builtin_amdgcn_readfirstlane(s_cp[cl + 1]), cend);
      if (live) {
#pragma unroll 8
        for (int q = e; q < hi; ++q) {
          const GxEntry en = se[q - ch0];
          acc = __builtin_fmaf(en.w, gzp[(size_t)en.o * rows + r], acc);
        }
      }
      e = hi;
    }
  }
  for (; cl < nc; ++cl) {                                               // the last column of the group, and empty ones after it
    emit(cl, acc);
    acc = 0.f;
  }
}

__global__ __launch_bounds__(256) void sparse_sigma_kernel(const bnn_sparse_sigma_args a) {
  const int g = blockIdx.y;
  const float* __restrict__ rho = a.rho[g];
  float* __restrict__ sigma = a.sigma[g];
  const uint8_t* __restrict__ keep = a.keep[g];
  const long n = (long)a.n[g];
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    sigma[i] = (!keep || keep[i]) ? softplus(rho[i]) : 0.f;
}

// columns of a group: the largest of 32, 16, 8, 4 that gives the launch >= 1024 blocks (4 if none does)
int col_group(int in, long other_blocks) {
  for (int cg = kMaxCG; cg > 4; cg >>= 1)
    if ((long)((in + cg - 1) / cg) * other_blocks >= 1024) return cg;
  return 4;
}

long terms_blocks(int nnz, int out) {
  return (long)((nnz + kTermSpan - 1) / kTermSpan) + (long)((out + kTermThreads - 1) / kTermThreads);
}

}  // namespace
}  // namespace bnn

using namespace bnn;

extern "C" size_t bnn_sparse_elbo_terms_workspace_bytes(int32_t n_layers, int32_t n_samples, const int32_t* nnz, const int32_t* out_features) {
  if (n_layers < 1 || n_layers > BNN_SPARSE_MAX_LAYERS || n_samples < 1 || n_samples > 65535 || !nnz || !out_features) return 0;
  long blocks = 0;
  for (int l = 0; l < n_layers; ++l) {
    if (nnz[l] < 0 || out_features[l] < 1) return 0;
    blocks += terms_blocks(nnz[l], out_features[l]);
  }
  return (size_t)blocks * (size_t)n_samples * sizeof(float4);
}

extern "C" int bnn_sparse_elbo_terms(const bnn_sparse_elbo_args* a, void* stream_) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_sparse_elbo_args)) return BNN_ERR_ABI;
  if (a->n_layers < 1 || a->n_layers > BNN_SPARSE_MAX_LAYERS || a->n_samples < 1 || a->n_samples > 65535) return BNN_ERR_SHAPE;
  int32_t nnzs[BNN_SPARSE_MAX_LAYERS], outs[BNN_SPARSE_MAX_LAYERS];
  for (int l = 0; l < a->n_layers; ++l) {
    const bnn_sparse_elbo_layer& y = a->layer[l];
    if (y.in_features < 1 || y.in_features > 65536 || y.out_features < 1 || y.nnz < 0 ||
        (int64_t)y.nnz > (int64_t)y.out_features * y.in_features)
      return BNN_ERR_SHAPE;
    nnzs[l] = y.nnz;
    outs[l] = y.out_features;
  }
  if (const int rc = prior_check(a->prior)) return rc;
  if (!a->log_prior || !a->log_q) return BNN_ERR_NULL;
  for (int l = 0; l < a->n_layers; ++l) {
    const bnn_sparse_elbo_layer& y = a->layer[l];
    if (!y.row_ptr || !y.col || !y.mu_val || !y.sigma_val || !y.b_mu || !y.b_sigma || !y.b_keep) return BNN_ERR_NULL;
  }
  const size_t need = bnn_sparse_elbo_terms_workspace_bytes(a->n_layers, a->n_samples, nnzs, outs);
  if (!a->workspace || a->workspace_bytes < need) return BNN_ERR_WORKSPACE;
  if (misaligned(a->workspace, 16) || misaligned(a->log_prior, 4) || misaligned(a->log_q, 4) || misaligned(a->sample_counter, 4))
    return BNN_ERR_ALIGN;
  TermsK k;
  long blocks = 0;
  for (int l = 0; l < a->n_layers; ++l) {
    const bnn_sparse_elbo_layer& y = a->layer[l];
    if (misaligned(y.row_ptr, 4) || misaligned(y.col, 2) || misaligned(y.mu_val, 4) || misaligned(y.sigma_val, 4) ||
        misaligned(y.b_mu, 4) || misaligned(y.b_sigma, 4))
      return BNN_ERR_ALIGN;
    TermsL& o = k.L[l];
    o.row_ptr = y.row_ptr; o.col = y.col; o.mu = y.mu_val; o.sigma = y.sigma_val; o.b_mu = y.b_mu; o.b_sigma = y.b_sigma;
    o.b_keep = y.b_keep;
    o.in = y.in_features; o.out = y.out_features; o.nnz = y.nnz; o.layer_id = y.layer_id;
    o.first_block = (int)blocks;
    o.entry_blocks = (y.nnz + kTermSpan - 1) / kTermSpan;
    o.blocks = (int)terms_blocks(y.nnz, y.out_features);
    blocks += o.blocks;
  }
  if (blocks > 0x3fffffff) return BNN_ERR_SHAPE;
  for (int l = a->n_layers; l < BNN_SPARSE_MAX_LAYERS; ++l) {
    k.L[l] = k.L[0];
    k.L[l].first_block = (int)blocks;
    k.L[l].blocks = 0;
  }
  k.n_layers = a->n_layers; k.S = a->n_samples; k.total_blocks = (int)blocks;
  k.k0 = (uint32_t)a->seed; k.k1 = (uint32_t)(a->seed >> 32);
  k.sample_offset = a->sample_offset; k.sample_counter = a->sample_counter;
  k.prior_kind = a->prior.kind;
  k.mix = prior_mix_make(a->prior);
  k.lp_const = 0; k.inv2var = 0;
  if (a->prior.kind == BNN_PRIOR_GAUSS) {
    const PriorFold f = prior_fold_make(a->prior, 1.0);                  // per element: the kernel knows the count
    k.lp_const = f.lp_const;
    k.inv2var = f.inv2var;
  }
  k.part = reinterpret_cast<float4*>(a->workspace);
  k.log_prior = a->log_prior; k.log_q = a->log_q;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  hipLaunchKernelGGL(sparse_terms_kernel, dim3((unsigned)blocks, (unsigned)a->n_samples), dim3(kTermThreads), 0, stream, k);
  hipLaunchKernelGGL(sparse_terms_fold_kernel, dim3((unsigned)a->n_samples), dim3(kTermThreads), 0, stream, k);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}

extern "C" size_t bnn_sparse_bwd_workspace_bytes(int32_t n_samples, int32_t rows, int32_t out_features) {
  if (n_samples < 1 || n_samples > 65535 || rows < 1 || out_features < 1) return 0;
  return (size_t)n_samples * (size_t)rows * (size_t)out_features * sizeof(float);
}

extern "C" int bnn_sparse_bwd(const bnn_sparse_bwd_args* a, void* stream_) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_sparse_bwd_args)) return BNN_ERR_ABI;
  if (a->n_samples < 1 || a->n_samples > 65535 || a->rows < 1 || a->in_features < 1 || a->in_features > 65536 ||
      a->out_features < 1 || (a->g_x && a->out_features > 65536) || a->nnz < 0 ||
      (int64_t)a->nnz > (int64_t)a->out_features * a->in_features || a->x_per_sample < 0)
    return BNN_ERR_SHAPE;
  const int waves = a->rows >= 256 ? 4 : (a->rows + 63) / 64;
  const int bdim = 64 * waves;
  const long batch_blocks = (a->rows + bdim - 1) / bdim;
  if (a->g_x && batch_blocks > 65535) return BNN_ERR_SHAPE;             // the input gradient's grid: 256 rows per block
  if (const int rc = prior_check(a->prior)) return rc;
  BwdS k;
  prior_dlogp_fill(a->prior, k);
  if (!a->row_ptr || !a->col || !a->mu_val || !a->rho_val || !a->b_mu || !a->b_rho || !a->b_keep || !a->x || !a->gy ||
      !a->g_mu_val || !a->g_rho_val || !a->g_b_mu || !a->g_b_rho)
    return BNN_ERR_NULL;
  if (a->relu && !a->y) return BNN_ERR_NULL;
  if (a->g_x && (!a->col_ptr || !a->row || !a->perm)) return BNN_ERR_NULL;
  const bool gz_launch = a->relu || a->gy_row_major;                     // else gz is gy itself and no workspace is read
  const size_t need = bnn_sparse_bwd_workspace_bytes(a->n_samples, a->rows, a->out_features);
  if (gz_launch && (!a->workspace || a->workspace_bytes < need)) return BNN_ERR_WORKSPACE;
  if (misaligned(a->row_ptr, 4) || misaligned(a->col, 2) || misaligned(a->mu_val, 4) || misaligned(a->rho_val, 4) ||
      misaligned(a->col_ptr, 4) || misaligned(a->row, 2) || misaligned(a->perm, 4) || misaligned(a->b_mu, 4) ||
      misaligned(a->b_rho, 4) || misaligned(a->x, 4) || misaligned(a->y, 4) || misaligned(a->gy, 4) ||
      misaligned(a->g_log_prior, 4) || misaligned(a->g_log_q, 4) || misaligned(a->g_mu_val, 4) || misaligned(a->g_rho_val, 4) ||
      misaligned(a->g_b_mu, 4) || misaligned(a->g_b_rho, 4) || misaligned(a->g_x, 4) || misaligned(a->workspace, 4) ||
      misaligned(a->sample_counter, 4))
    return BNN_ERR_ALIGN;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const float* gz = a->gy;
  if (gz_launch) {
    float* gzw = reinterpret_cast<float*>(a->workspace);
    const long cnt = (long)a->n_samples * a->rows * a->out_features;
    long nb = (cnt + 255) / 256;
    nb = nb > 2048 ? 2048 : nb;
    hipLaunchKernelGGL(sparse_gz_kernel, dim3((unsigned)nb), dim3(256), 0, stream, a->gy, a->y, gzw, a->n_samples, a->rows,
                       a->out_features, a->relu ? 1 : 0, a->gy_row_major ? 1 : 0);
    gz = gzw;
  }
  k.row_ptr = a->row_ptr; k.col = a->col; k.mu = a->mu_val; k.rho = a->rho_val;
  k.col_ptr = a->col_ptr; k.row = a->row; k.perm = a->perm;
  k.b_mu = a->b_mu; k.b_rho = a->b_rho; k.b_keep = a->b_keep;
  k.x = a->x; k.gz = gz; k.glp = a->g_log_prior; k.glq = a->g_log_q;
  k.g_mu = a->g_mu_val; k.g_rho = a->g_rho_val; k.g_bmu = a->g_b_mu; k.g_brho = a->g_b_rho; k.gx = a->g_x;
  k.S = a->n_samples; k.rows = a->rows; k.in = a->in_features; k.out = a->out_features; k.nnz = a->nnz;
  k.x_per_sample = a->x_per_sample; k.gx_relu_mask = a->gx_relu_mask ? 1 : 0;
  k.entry_blocks = (a->nnz + 4 * kWaveEntries - 1) / (4 * kWaveEntries);
  k.k0 = (uint32_t)a->seed; k.k1 = (uint32_t)(a->seed >> 32);
  k.layer_id = a->layer_id; k.sample_offset = a->sample_offset; k.sample_counter = a->sample_counter;
  const unsigned wblocks = (unsigned)k.entry_blocks + (unsigned)((a->out_features + 3) / 4);
  hipLaunchKernelGGL(sparse_bwd_weights_kernel, dim3(wblocks), dim3(256), 0, stream, k);
  if (a->g_x) {
    const int cg = col_group(a->in_features, (long)a->n_samples * batch_blocks);
    const dim3 grid((unsigned)((a->in_features + cg - 1) / cg), (unsigned)a->n_samples, (unsigned)batch_blocks);
    hipLaunchKernelGGL(sparse_bwd_input_kernel, grid, dim3(bdim), 0, stream, k, cg);
  }
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}

extern "C" int bnn_sparse_sigma_refresh(const bnn_sparse_sigma_args* a, void* stream_) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_sparse_sigma_args)) return BNN_ERR_ABI;
  if (a->n_segments < 1 || a->n_segments > BNN_SPARSE_MAX_SEGMENTS) return BNN_ERR_SHAPE;
  int64_t most = 0;
  for (int g = 0; g < a->n_segments; ++g) {
    if (a->n[g] < 0) return BNN_ERR_SHAPE;
    most = a->n[g] > most ? a->n[g] : most;
  }
  for (int g = 0; g < a->n_segments; ++g)
    if (a->n[g] > 0 && (!a->rho[g] || !a->sigma[g])) return BNN_ERR_NULL;
  for (int g = 0; g < a->n_segments; ++g)
    if (misaligned(a->rho[g], 4) || misaligned(a->sigma[g], 4)) return BNN_ERR_ALIGN;
  if (most == 0) return BNN_OK;
  int64_t nb = (most + 255) / 256;
  nb = nb > 1024 ? 1024 : nb;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  hipLaunchKernelGGL(sparse_sigma_kernel, dim3((unsigned)nb, (unsigned)a->n_segments), dim3(256), 0, stream, *a);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}
