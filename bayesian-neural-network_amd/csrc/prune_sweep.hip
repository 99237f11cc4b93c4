// F9 pruning sweep, the streaming parts (include/bnn_hip.h F9): weight_pruning.py:89-115 for P drop levels at once.
//   bnn_snr_select        the P percentile thresholds by radix selection over the SNR segments (no sort, no host read)
//   bnn_prune_codes       one byte per parameter: how many of the ascending thresholds its SNR exceeds, + a matmul-ready mu
//   bnn_prune_sweep_tail  softmax / argmax / cross-entropy (or squared error) of the P logit sets of a minibatch
// Integer atomics only, fp64 sums in a fixed order: bitwise reproducible.  The masked forward is pruned_fwd.hip.
#include <math.h>

#include "bnn_device.h"
#include "bnn_snr.h"
#include "../../include/bnn_hip.h"

namespace bnn {
namespace {

// ------------------------------------------------------------------------------------------------------------ selection
constexpr int kSelTargets = 2 * BNN_PRUNE_MAX_LEVELS;   // the two order statistics around (n - 1) p of every level
constexpr int kSelBins = 256;                           // 8 key bits per pass, 4 passes
constexpr int kSelBlock = 256;
constexpr int kSelMaxBlocks = 1024;

// Per target t: the key bits found so far and its rank among the elements that share them.  Targets with equal prefixes
// form a group (one histogram per group); lead_prefix lists the groups' prefixes.
struct SelState {
  uint32_t prefix[kSelTargets], rank[kSelTargets], group[kSelTargets], lead_prefix[kSelTargets];
  uint32_t n_groups, pad[3];
};
struct SelSegs {
  const float* p[BNN_PRUNE_MAX_SEGMENTS];
  long n[BNN_PRUNE_MAX_SEGMENTS];
  int n_segs;
};
struct SelRanks {
  uint32_t rank[kSelTargets];          // lo_p, hi_p at 2 p, 2 p + 1
  double frac[BNN_PRUNE_MAX_LEVELS];   // pos - lo
  int n_levels;
};

// order-preserving key: -inf < ... < -0 < +0 < ... < +inf < every NaN (torch.sort puts NaNs last)
__device__ __forceinline__ uint32_t snr_key(float v) {
  const uint32_t u = __float_as_uint(v);
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return 0xFFFFFFFFu;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float snr_unkey(uint32_t k) {
  if (k == 0xFFFFFFFFu) return __uint_as_float(0x7FC00000u);
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

__global__ __launch_bounds__(kSelBlock) void select_init_kernel(SelState* st, uint32_t* hist, SelRanks r) {
  for (int i = threadIdx.x; i < kSelTargets * kSelBins; i += kSelBlock) hist[i] = 0u;
  if (threadIdx.x < kSelTargets) {
    const int t = threadIdx.x;
    st->prefix[t] = 0u;
    st->rank[t] = t < 2 * r.n_levels ? r.rank[t] : 0u;
    st->group[t] = 0u;
    st->lead_prefix[t] = 0u;
  }
  if (threadIdx.x == 0) st->n_groups = 1u;
}

// pass q: the histogram of key bits [24 - 8 q, 32 - 8 q) of the elements whose higher bits equal a group's prefix
__global__ __launch_bounds__(kSelBlock) void select_hist_kernel(SelSegs segs, const SelState* st, uint32_t* hist, int pass) {
  __shared__ uint32_t s_hist[kSelTargets * kSelBins];
  __shared__ uint32_t s_lead[kSelTargets];
  const uint32_t G = st->n_groups;                                 // <= kSelTargets
  for (uint32_t i = threadIdx.x; i < G * kSelBins; i += kSelBlock) s_hist[i] = 0u;
  if (threadIdx.x < kSelTargets) s_lead[threadIdx.x] = st->lead_prefix[threadIdx.x];
  __syncthreads();
  const int shift = 24 - 8 * pass;
  const long tid = (long)blockIdx.x * kSelBlock + threadIdx.x, nt = (long)gridDim.x * kSelBlock;
  for (int s = 0; s < segs.n_segs; ++s) {
    const float* __restrict__ v = segs.p[s];
    for (long i = tid; i < segs.n[s]; i += nt) {
      const uint32_t key = snr_key(v[i]);
      const uint32_t hi = pass == 0 ? 0u : key >> (shift + 8);
      for (uint32_t g = 0; g < G; ++g)
        if (hi == s_lead[g]) {                                     // the groups' prefixes are distinct: one match at most
          atomicAdd(&s_hist[g * kSelBins + ((key >> shift) & 255u)], 1u);
          break;
        }
    }
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < G * kSelBins; i += kSelBlock)
    if (s_hist[i]) atomicAdd(&hist[i], s_hist[i]);
}

// one block: every target walks its group's histogram to the bin that holds its rank, the targets are regrouped, the
// histograms are cleared for the next pass; after the last pass the prefixes are the order statistics' keys
__global__ __launch_bounds__(kSelBlock) void select_scan_kernel(SelState* st, uint32_t* hist, int pass, SelRanks r,
                                                                double* __restrict__ thresholds) {
  const int t = threadIdx.x, T = 2 * r.n_levels;
  if (t < T) {
    const uint32_t* h = hist + st->group[t] * kSelBins;
    const uint32_t rank = st->rank[t];
    uint32_t cum = 0u, digit = kSelBins - 1;
    for (uint32_t d = 0; d < (uint32_t)kSelBins; ++d) {
      const uint32_t c = h[d];
      if (rank < cum + c) { digit = d; break; }
      cum += c;
    }
    st->prefix[t] = (st->prefix[t] << 8) | digit;
    st->rank[t] = rank - cum;
  }
  __syncthreads();
  if (t == 0) {
    uint32_t G = 0;
    for (int a = 0; a < T; ++a) {
      uint32_t g = G;
      for (uint32_t b = 0; b < G; ++b)
        if (st->lead_prefix[b] == st->prefix[a]) { g = b; break; }
      if (g == G) st->lead_prefix[G++] = st->prefix[a];
      st->group[a] = g;
    }
    st->n_groups = G;
  }
  for (int i = t; i < kSelTargets * kSelBins; i += kSelBlock) hist[i] = 0u;
  if (pass == 3 && t < r.n_levels) {
#pragma clang fp contract(off)
    const double a = (double)snr_unkey(st->prefix[2 * t]), b = (double)snr_unkey(st->prefix[2 * t + 1]);
    const double d = (b - a) * r.frac[t];                          // a product and a sum, each rounded: not an fma
    thresholds[t] = a == b ? a : a + d;
  }
}

// ------------------------------------------------------------------------------------------------------------ level codes
constexpr int kCodeTile = 32;
constexpr int kCodeBlock = 256;

template <bool TRANSPOSED, typename MT>
__global__ __launch_bounds__(kCodeBlock) void prune_codes_kernel(bnn_prune_codes_args a) {
  __shared__ float s_thr[BNN_PRUNE_MAX_LEVELS];
  __shared__ unsigned int s_hist[BNN_PRUNE_MAX_LEVELS + 1];
  __shared__ float s_mu[kCodeTile][kCodeTile + 1];
  __shared__ unsigned char s_code[kCodeTile][kCodeTile + 1];
  const int P = a.n_levels;
  if (threadIdx.x < (unsigned)P) s_thr[threadIdx.x] = (float)a.thresholds[threadIdx.x];   // the rounding bnn_snr_prune's caller makes
  if (threadIdx.x <= (unsigned)BNN_PRUNE_MAX_LEVELS) s_hist[threadIdx.x] = 0u;
  __syncthreads();
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int o0 = blockIdx.y * kCodeTile, i0 = blockIdx.x * kCodeTile;
  MT* __restrict__ mu_out = static_cast<MT*>(a.mu_out);
  auto code_of = [&](float m, float r) {
    const float s = snr_db(m, r);
    int c = 0;
    for (int p = 0; p < P; ++p) c += s > s_thr[p] ? 1 : 0;
    atomicAdd(&s_hist[c], 1u);                                      // integers: exact in any order
    return c;
  };
  if (!TRANSPOSED) {
#pragma unroll
    for (int j = 0; j < kCodeTile / 8; ++j) {
      const int o = o0 + ty + 8 * j, i = i0 + tx;
      if (o < a.out_features && i < a.in_features) {
        const long src = (long)o * a.in_features + i, dst = (long)o * a.ld + i;
        const float m = a.mu[src];
        a.code[dst] = (unsigned char)code_of(m, a.rho[src]);
        mu_out[dst] = (MT)m;
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < kCodeTile / 8; ++j) {                       // source [in, out]: tx runs along out
      const int i = i0 + ty + 8 * j, o = o0 + tx;
      if (o < a.out_features && i < a.in_features) {
        const long src = (long)i * a.out_features + o;
        const float m = a.mu[src];
        s_mu[ty + 8 * j][tx] = m;
        s_code[ty + 8 * j][tx] = (unsigned char)code_of(m, a.rho[src]);
      }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kCodeTile / 8; ++j) {                       // canonical [out, in]: tx runs along in
      const int o = o0 + ty + 8 * j, i = i0 + tx;
      if (o < a.out_features && i < a.in_features) {
        const long dst = (long)o * a.ld + i;
        a.code[dst] = s_code[tx][ty + 8 * j];
        mu_out[dst] = (MT)s_mu[tx][ty + 8 * j];
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < (unsigned)P) {                                   // survivors of level p: code > p
    unsigned long long k = 0;
    for (int c = threadIdx.x + 1; c <= P; ++c) k += s_hist[c];
    if (k) atomicAdd(reinterpret_cast<unsigned long long*>(a.kept) + threadIdx.x, k);
  }
}

// ------------------------------------------------------------------------------------------------------------ tail
constexpr int kTailBlock = 256;

// block p = level p: a row per thread at a time; the fp64 sums go lane tree -> wave order, the same for every launch
__global__ __launch_bounds__(kTailBlock) void prune_tail_kernel(bnn_prune_tail_args a) {
  __shared__ double s_sum[kTailBlock / 64];
  __shared__ unsigned int s_cor[kTailBlock / 64];
  const int p = blockIdx.x, C = a.classes;
  const float* __restrict__ z = a.logits + (size_t)p * a.rows * C;
  const bool cls = a.mode == BNN_NLL_CLASSIFICATION;
  double loss = 0.0;
  unsigned int cor = 0u;
  for (int r = threadIdx.x; r < a.rows; r += kTailBlock) {
    const float* zr = z + (size_t)r * C;
    if (cls) {
      const long long lab = static_cast<const long long*>(a.target)[r];
      float best = zr[0];
      int arg = 0;
      for (int c = 1; c < C; ++c)
        if (zr[c] > best) { best = zr[c]; arg = c; }                 // first maximum, as torch.argmax / np.argmax
      float sum = 0.f;
      for (int c = 0; c < C; ++c) sum += expf(zr[c] - best);
      float* pr = a.probs + ((size_t)p * a.n_total + a.row0 + r) * C;
      for (int c = 0; c < C; ++c) pr[c] = expf(zr[c] - best) / sum;
      if (lab >= 0 && lab < C) {
        loss += (double)(logf(sum) + best - zr[lab]);
        cor += lab == arg ? 1u : 0u;
      }
    } else {
      const float* tr = static_cast<const float*>(a.target) + (size_t)r * C;
      for (int c = 0; c < C; ++c) {
        const double d = (double)zr[c] - (double)tr[c];
        loss += d * d;
      }
    }
  }
  loss = wave_sum(loss);
  for (int off = 32; off > 0; off >>= 1) cor += __shfl_xor(cor, off, 64);
  if ((threadIdx.x & 63) == 0) {
    s_sum[threadIdx.x >> 6] = loss;
    s_cor[threadIdx.x >> 6] = cor;
  }
  __syncthreads();
  if (threadIdx.x == 0) {                                            // the only writer of level p's words in this launch
    double t = 0.0;
    unsigned int k = 0u;
    for (int w = 0; w < kTailBlock / 64; ++w) { t += s_sum[w]; k += s_cor[w]; }
    a.loss[p] += t;
    if (cls) a.correct[p] += (long long)k;
  }
}

constexpr size_t kSelStateBytes = (sizeof(SelState) + 15) & ~size_t(15);

}  // namespace
}  // namespace bnn

using namespace bnn;

extern "C" size_t bnn_snr_select_workspace_bytes(void) { return kSelStateBytes + sizeof(uint32_t) * kSelTargets * kSelBins; }

extern "C" int bnn_snr_select(const bnn_snr_select_args* a, void* stream_) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_snr_select_args)) return BNN_ERR_ABI;
  if (a->n_segments < 1 || a->n_segments > BNN_PRUNE_MAX_SEGMENTS || a->n_levels < 1 || a->n_levels > BNN_PRUNE_MAX_LEVELS)
    return BNN_ERR_SHAPE;
  if (!a->thresholds) return BNN_ERR_NULL;
  SelSegs segs;
  int64_t n = 0;
  for (int s = 0; s < BNN_PRUNE_MAX_SEGMENTS; ++s) {
    segs.p[s] = nullptr;
    segs.n[s] = 0;
  }
  for (int s = 0; s < a->n_segments; ++s) {
    if (!a->snr[s]) return BNN_ERR_NULL;
    if (a->n[s] < 1 || a->n[s] >= ((int64_t)1 << 31)) return BNN_ERR_SHAPE;
    if (misaligned(a->snr[s], 4)) return BNN_ERR_ALIGN;
    segs.p[s] = a->snr[s];
    segs.n[s] = (long)a->n[s];
    n += a->n[s];
  }
  if (n >= ((int64_t)1 << 31)) return BNN_ERR_SHAPE;
  segs.n_segs = a->n_segments;
  SelRanks r;
  r.n_levels = a->n_levels;
  for (int p = 0; p < BNN_PRUNE_MAX_LEVELS; ++p) {
    r.rank[2 * p] = r.rank[2 * p + 1] = 0u;
    r.frac[p] = 0.0;
  }
  for (int p = 0; p < a->n_levels; ++p) {
    const double f = a->fraction[p];
    if (!(f >= 0.0 && f <= 1.0)) return BNN_ERR_SHAPE;
    const double pos = (double)(n - 1) * f;                         // posthoc.snr_threshold, in the same fp64 operations
    const double lo = floor(pos);
    int64_t ilo = (int64_t)lo;
    if (ilo > n - 1) ilo = n - 1;
    const int64_t ihi = ilo + 1 < n ? ilo + 1 : n - 1;
    r.rank[2 * p] = (uint32_t)ilo;
    r.rank[2 * p + 1] = (uint32_t)ihi;
    r.frac[p] = pos - lo;
  }
  if (!a->workspace || a->workspace_bytes < bnn_snr_select_workspace_bytes()) return BNN_ERR_WORKSPACE;
  if (misaligned(a->workspace, 8) || misaligned(a->thresholds, 8)) return BNN_ERR_ALIGN;
  SelState* st = static_cast<SelState*>(a->workspace);
  uint32_t* hist = reinterpret_cast<uint32_t*>(static_cast<char*>(a->workspace) + kSelStateBytes);
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  long nb = (n + kSelBlock * 8 - 1) / (kSelBlock * 8);
  nb = nb < 1 ? 1 : (nb > kSelMaxBlocks ? kSelMaxBlocks : nb);
  hipLaunchKernelGGL(select_init_kernel, dim3(1), dim3(kSelBlock), 0, stream, st, hist, r);
  for (int pass = 0; pass < 4; ++pass) {
    hipLaunchKernelGGL(select_hist_kernel, dim3((unsigned)nb), dim3(kSelBlock), 0, stream, segs, st, hist, pass);
    hipLaunchKernelGGL(select_scan_kernel, dim3(1), dim3(kSelBlock), 0, stream, st, hist, pass, r, a->thresholds);
  }
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}

extern "C" int bnn_prune_codes(const bnn_prune_codes_args* a, void* stream_) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_prune_codes_args)) return BNN_ERR_ABI;
  if (a->out_features < 1 || a->in_features < 1 || a->ld < a->in_features || a->n_levels < 1 || a->n_levels > BNN_PRUNE_MAX_LEVELS)
    return BNN_ERR_SHAPE;
  if (a->mu_dtype != BNN_F32 && a->mu_dtype != BNN_BF16) return BNN_ERR_ENUM;
  if (!a->mu || !a->rho || !a->thresholds || !a->code || !a->mu_out || !a->kept) return BNN_ERR_NULL;
  if (misaligned(a->mu, 4) || misaligned(a->rho, 4) || misaligned(a->thresholds, 8) || misaligned(a->kept, 8) ||
      misaligned(a->mu_out, a->mu_dtype == BNN_BF16 ? 2 : 4))
    return BNN_ERR_ALIGN;
  const dim3 grid((unsigned)((a->in_features + kCodeTile - 1) / kCodeTile), (unsigned)((a->out_features + kCodeTile - 1) / kCodeTile));
  if (grid.y > 65535u) return BNN_ERR_SHAPE;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const bool tr = a->transposed != 0, b16 = a->mu_dtype == BNN_BF16;
  if (tr && b16) hipLaunchKernelGGL((prune_codes_kernel<true, __bf16>), grid, dim3(kCodeBlock), 0, stream, *a);
  else if (tr) hipLaunchKernelGGL((prune_codes_kernel<true, float>), grid, dim3(kCodeBlock), 0, stream, *a);
  else if (b16) hipLaunchKernelGGL((prune_codes_kernel<false, __bf16>), grid, dim3(kCodeBlock), 0, stream, *a);
  else hipLaunchKernelGGL((prune_codes_kernel<false, float>), grid, dim3(kCodeBlock), 0, stream, *a);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}

extern "C" int bnn_prune_sweep_tail(const bnn_prune_tail_args* a, void* stream_) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_prune_tail_args)) return BNN_ERR_ABI;
  if (a->mode != BNN_NLL_REGRESSION && a->mode != BNN_NLL_CLASSIFICATION) return BNN_ERR_ENUM;
  if (a->n_levels < 1 || a->n_levels > BNN_PRUNE_MAX_LEVELS || a->rows < 1 || a->classes < 1 || a->row0 < 0 || a->n_total < 1 ||
      a->row0 + a->rows > a->n_total)
    return BNN_ERR_SHAPE;
  const bool cls = a->mode == BNN_NLL_CLASSIFICATION;
  if (!a->logits || !a->target || !a->loss || (cls && (!a->probs || !a->correct))) return BNN_ERR_NULL;
  if (misaligned(a->logits, 4) || misaligned(a->loss, 8) || misaligned(a->target, cls ? 8 : 4)) return BNN_ERR_ALIGN;
  if (cls && (misaligned(a->probs, 4) || misaligned(a->correct, 8))) return BNN_ERR_ALIGN;
  hipLaunchKernelGGL(prune_tail_kernel, dim3((unsigned)a->n_levels), dim3(kTailBlock), 0, reinterpret_cast<hipStream_t>(stream_), *a);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}
