// F11 posterior statistics (include/bnn_hip.h F11): utils/logger_utils.py:13-26 (write_weight_histograms) and the weight /
// SNR histograms of weight_pruning.py:16-79, for up to BNN_HIST_MAX_JOBS tensors in one pass.
//   bnn_param_hist   clear the records -> bin (one block per BNN_HIST_CHUNK elements of one job) -> fold the block partials
// Every parameter is read once; the transform (softplus, SNR, a posterior sample on the frozen epsilon map) is the
// definition the other kernels use.  Integer atomics for the counts, fp64 sums in a fixed order: bitwise reproducible.
//
// Shape.  The binning load is skewed: a trained layer's sigma falls into ~10 adjacent bins of the 1.1-ratio table, its mu
// into ~30, a constant tensor into one.  One LDS histogram per block with an atomic per element would queue the block's
// 256 lanes on a handful of words, so (a) every wave owns a sub-histogram and (b) a wave first combines its equal bins:
// up to kPeel times the first pending lane's bin is broadcast, the lanes holding it are counted by a ballot and ONE lane
// adds the count; what is still pending after kPeel rounds sits in thinly populated bins and adds one by one.  The
// sub-histograms are summed into the job's uint64 counts once per block, non-empty bins only.  The bin of a value is an
// upper-bound search of the fp64 edge table in LDS (<= 11 wave-uniform steps, four values per lane in flight).
// Loads and the values_out stores are dwords, a wave's 64 consecutive: a job starts at any 4-byte address and the kernel
// is bound by the search and the LDS adds, not by the 8 bytes per element it reads.
#include <math.h>

#include "bnn_device.h"
#include "bnn_snr.h"
#include "../../include/bnn_hip.h"

namespace bnn {
namespace {

constexpr int kHistBlock = 256;
constexpr int kHistWaves = kHistBlock / kWave;
constexpr int kHistBins = BNN_HIST_MAX_EDGES - 1 + 3;        // the bins, then below / above / NaN
constexpr int kHistUnroll = 4;                               // values per lane in flight
constexpr int kPeel = 8;
static_assert(BNN_HIST_CHUNK % (kHistBlock * kHistUnroll) == 0, "a chunk is a whole number of block passes");

struct HistPartial {                                          // of one block
  double sum, sum_sq;
  float mn, mx;
};

struct HistJobK {
  const float* src0;
  const float* src1;
  float* values_out;
  unsigned long long* record;                                 // counts[nb], then the summary
  long n;
  int kind, cols, gpr;                                        // SAMPLE: columns, epsilon groups per row
  uint32_t tensor_id, sample, k0, k1;
};
struct HistK {
  HistJobK job[BNN_HIST_MAX_JOBS];
  int first_block[BNN_HIST_MAX_JOBS + 1];
  const double* edges;
  HistPartial* partial;
  int n_jobs, n_edges;
};

__device__ __forceinline__ float hist_value(const HistJobK& j, long i) {
  const float a = j.src0[i];
  switch (j.kind) {
    case BNN_HIST_SIGMA: return softplus(a);
    case BNN_HIST_SNR_DB: return snr_db(a, j.src1[i]);
    case BNN_HIST_SAMPLE: {
      const long row = i / j.cols;
      const int col = (int)(i - row * j.cols);
      float e[4];
      philox_normal4((uint32_t)(row * j.gpr + (col >> 2)), j.sample, j.tensor_id, j.k0, j.k1, e);
      const int s = col & 3;
      const float eps = s == 0 ? e[0] : (s == 1 ? e[1] : (s == 2 ? e[2] : e[3]));
      return __builtin_fmaf(softplus(j.src1[i]), eps, a);
    }
    default: return a;
  }
}

__global__ __launch_bounds__(kHistBlock) void hist_clear_kernel(HistK k) {
  unsigned long long* rec = k.job[blockIdx.y].record;
  const int words = k.n_edges - 1 + 4;                        // the counts and the four counters; the fold writes the rest
  for (int i = blockIdx.x * kHistBlock + threadIdx.x; i < words; i += gridDim.x * kHistBlock) rec[i] = 0ull;
}

__global__ __launch_bounds__(kHistBlock) void hist_bin_kernel(HistK k) {
  __shared__ double s_edge[BNN_HIST_MAX_EDGES];
  __shared__ unsigned int s_hist[kHistWaves][kHistBins];
  __shared__ double s_sum[kHistWaves], s_sq[kHistWaves];
  __shared__ float s_mn[kHistWaves], s_mx[kHistWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ne = k.n_edges, nb = ne - 1;
  int ji = 0;
#pragma unroll 1
  while (ji + 1 < k.n_jobs && (int)blockIdx.x >= k.first_block[ji + 1]) ++ji;   // block-uniform
  const HistJobK& j = k.job[ji];
  for (int i = tid; i < ne; i += kHistBlock) s_edge[i] = k.edges[i];
  for (int i = lane; i < nb + 3; i += kWave) s_hist[wave][i] = 0u;
  __syncthreads();
  const double e_first = s_edge[0], e_last = s_edge[nb];
  int top = 1;
  while (top * 2 <= nb) top *= 2;                             // the largest power of two <= nb
  unsigned int* hist = s_hist[wave];

  const long lo = (long)((int)blockIdx.x - k.first_block[ji]) * BNN_HIST_CHUNK;
  const long hi = min(lo + (long)BNN_HIST_CHUNK, j.n);
  double sum = 0.0, sq = 0.0;
  float mn = INFINITY, mx = -INFINITY;
#pragma unroll 1
  for (long base = lo; base < hi; base += kHistBlock * kHistUnroll) {         // block-uniform trip count
    float v[kHistUnroll];
    double d[kHistUnroll];
    int bin[kHistUnroll], pos[kHistUnroll];
    bool live[kHistUnroll];
#pragma unroll
    for (int u = 0; u < kHistUnroll; ++u) {
      const long i = base + u * kHistBlock + tid;
      live[u] = i < hi;
      v[u] = live[u] ? hist_value(j, i) : 0.f;
      if (live[u] && j.values_out) j.values_out[i] = v[u];
      d[u] = (double)v[u];
      pos[u] = 0;
    }
#pragma unroll 1
    for (int step = top; step > 0; step >>= 1) {              // the largest p with e_p <= d (p = 0 when there is none)
#pragma unroll
      for (int u = 0; u < kHistUnroll; ++u) {
        const int p = pos[u] + step;
        if (p <= nb && s_edge[p] <= d[u]) pos[u] = p;
      }
    }
#pragma unroll
    for (int u = 0; u < kHistUnroll; ++u) {
      const bool nan = v[u] != v[u];
      bin[u] = nan ? nb + 2 : (d[u] < e_first ? nb : (d[u] > e_last ? nb + 1 : (pos[u] == nb ? nb - 1 : pos[u])));
      if (live[u] && !nan) {                                   // a thread's elements in index order
        mn = fminf(mn, v[u]);
        mx = fmaxf(mx, v[u]);
        if (fabsf(v[u]) != INFINITY) {
          sum += d[u];
          sq = fma(d[u], d[u], sq);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kHistUnroll; ++u) {
      bool pend = live[u];
#pragma unroll 1
      for (int it = 0; it < kPeel; ++it) {
        const unsigned long long m = __ballot(pend);
        if (!m) break;                                         // wave-uniform
        const int leader = __ffsll((long long)m) - 1;
        const int lb = __shfl(bin[u], leader, kWave);
        const bool same = pend && bin[u] == lb;
        const unsigned long long sm = __ballot(same);
        if (lane == leader) atomicAdd(&hist[lb], (unsigned int)__popcll(sm));
        pend = pend && !same;
      }
      if (pend) atomicAdd(&hist[bin[u]], 1u);
    }
  }

  // the block's partial: lanes by the shuffle tree, waves in order
  sum = wave_sum(sum);
  sq = wave_sum(sq);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, off, kWave));
    mx = fmaxf(mx, __shfl_xor(mx, off, kWave));
  }
  if (lane == 0) {
    s_sum[wave] = sum;
    s_sq[wave] = sq;
    s_mn[wave] = mn;
    s_mx[wave] = mx;
  }
  __syncthreads();                                             // also: every wave's sub-histogram is complete
  if (tid == 0) {
    HistPartial p;
    p.sum = s_sum[0];
    p.sum_sq = s_sq[0];
    p.mn = s_mn[0];
    p.mx = s_mx[0];
    for (int w = 1; w < kHistWaves; ++w) {
      p.sum += s_sum[w];
      p.sum_sq += s_sq[w];
      p.mn = fminf(p.mn, s_mn[w]);
      p.mx = fmaxf(p.mx, s_mx[w]);
    }
    k.partial[blockIdx.x] = p;
  }
  // the sub-histograms into the record: word b < nb = bin b, word nb = n_in, then n_below, n_above, n_nan
  unsigned int outside = 0u;
  for (int i = tid; i < nb + 3; i += kHistBlock) {
    unsigned int c = 0u;
#pragma unroll
    for (int w = 0; w < kHistWaves; ++w) c += s_hist[w][i];
    if (i >= nb) outside += c;
    if (c) atomicAdd(&j.record[i < nb ? i : i + 1], (unsigned long long)c);
  }
  __syncthreads();                                             // s_hist[0][0 .. 3) is free now: the three outside counts meet there
  if (tid < 3) s_hist[0][tid] = 0u;
  __syncthreads();
  if (outside) atomicAdd(&s_hist[0][0], outside);
  __syncthreads();
  if (tid == 0 && hi > lo) atomicAdd(&j.record[nb], (unsigned long long)(hi - lo) - s_hist[0][0]);
}

// one block per job: the block partials by a fixed tree (thread t takes partials t, t + 256, ... in order, then halves)
__global__ __launch_bounds__(kHistBlock) void hist_fold_kernel(HistK k) {
  __shared__ double s_sum[kHistBlock], s_sq[kHistBlock];
  __shared__ float s_mn[kHistBlock], s_mx[kHistBlock];
  const int tid = threadIdx.x, ji = blockIdx.x;
  const int b0 = k.first_block[ji], b1 = k.first_block[ji + 1];
  double sum = 0.0, sq = 0.0;
  float mn = INFINITY, mx = -INFINITY;
  for (int b = b0 + tid; b < b1; b += kHistBlock) {
    const HistPartial p = k.partial[b];
    sum += p.sum;
    sq += p.sum_sq;
    mn = fminf(mn, p.mn);
    mx = fmaxf(mx, p.mx);
  }
  s_sum[tid] = sum;
  s_sq[tid] = sq;
  s_mn[tid] = mn;
  s_mx[tid] = mx;
  for (int off = kHistBlock / 2; off > 0; off >>= 1) {
    __syncthreads();
    if (tid < off) {
      s_sum[tid] += s_sum[tid + off];
      s_sq[tid] += s_sq[tid + off];
      s_mn[tid] = fminf(s_mn[tid], s_mn[tid + off]);
      s_mx[tid] = fmaxf(s_mx[tid], s_mx[tid + off]);
    }
  }
  if (tid == 0) {
    bnn_hist_summary* out = reinterpret_cast<bnn_hist_summary*>(k.job[ji].record + (k.n_edges - 1));
    out->min = s_mn[0];
    out->max = s_mx[0];
    out->sum = s_sum[0];
    out->sum_sq = s_sq[0];
  }
}

// the argument checks shared by the query and the launch; fills the kernels' block (first_block) on success
int hist_plan(const bnn_param_hist_args* a, HistK& k) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_param_hist_args)) return BNN_ERR_ABI;
  if (a->n_jobs < 1 || a->n_jobs > BNN_HIST_MAX_JOBS || a->n_edges < 2 || a->n_edges > BNN_HIST_MAX_EDGES) return BNN_ERR_SHAPE;
  if (a->edges_host)
    for (int i = 0; i < a->n_edges; ++i) {
      const double e = a->edges_host[i];
      if (!(e - e == 0.0) || (i > 0 && !(a->edges_host[i - 1] < e))) return BNN_ERR_SHAPE;   // finite, strictly increasing
    }
  long blocks = 0;
  for (int i = 0; i < BNN_HIST_MAX_JOBS + 1; ++i) k.first_block[i] = 0;
  for (int i = 0; i < BNN_HIST_MAX_JOBS; ++i) k.job[i] = HistJobK{};
  for (int i = 0; i < a->n_jobs; ++i) {
    const bnn_param_hist_job& j = a->jobs[i];
    if (j.kind < BNN_HIST_VALUE || j.kind > BNN_HIST_SAMPLE) return BNN_ERR_ENUM;
    if (j.n < 0 || j.n >= ((int64_t)1 << 31)) return BNN_ERR_SHAPE;
    const bool two = j.kind == BNN_HIST_SNR_DB || j.kind == BNN_HIST_SAMPLE;
    if (j.kind == BNN_HIST_SAMPLE && j.n > 0 && (j.rows < 1 || j.cols < 1 || (int64_t)j.rows * j.cols != j.n)) return BNN_ERR_SHAPE;
    if (!j.record || (j.n > 0 && (!j.src0 || (two && !j.src1)))) return BNN_ERR_NULL;
    if (misaligned(j.src0, 4) || misaligned(j.src1, 4) || misaligned(j.values_out, 4) || misaligned(j.record, 8)) return BNN_ERR_ALIGN;
    HistJobK& o = k.job[i];
    o.src0 = j.src0;
    o.src1 = j.src1;
    o.values_out = j.values_out;
    o.record = static_cast<unsigned long long*>(j.record);
    o.n = (long)j.n;
    o.kind = j.kind;
    o.cols = j.kind == BNN_HIST_SAMPLE && j.cols > 0 ? j.cols : 1;
    o.gpr = (o.cols + 3) >> 2;
    o.tensor_id = j.tensor_id;
    o.sample = j.sample;
    o.k0 = (uint32_t)j.seed;
    o.k1 = (uint32_t)(j.seed >> 32);
    k.first_block[i] = (int)blocks;
    blocks += (j.n + BNN_HIST_CHUNK - 1) / BNN_HIST_CHUNK;
  }
  for (int i = a->n_jobs; i < BNN_HIST_MAX_JOBS + 1; ++i) k.first_block[i] = (int)blocks;   // 16 x 2^18 blocks at most
  k.n_jobs = a->n_jobs;
  k.n_edges = a->n_edges;
  return BNN_OK;
}

size_t hist_workspace_bytes(const HistK& k) {
  const int blocks = k.first_block[k.n_jobs];
  return sizeof(HistPartial) * (size_t)(blocks < 1 ? 1 : blocks);
}

}  // namespace
}  // namespace bnn

using namespace bnn;

extern "C" size_t bnn_param_hist_workspace_bytes(const bnn_param_hist_args* a) {
  HistK k;
  return hist_plan(a, k) == BNN_OK ? hist_workspace_bytes(k) : 0;
}

extern "C" int bnn_param_hist(const bnn_param_hist_args* a, void* stream_) {
  HistK k;
  const int rc = hist_plan(a, k);
  if (rc != BNN_OK) return rc;
  if (!a->edges) return BNN_ERR_NULL;
  if (!a->workspace || a->workspace_bytes < hist_workspace_bytes(k)) return BNN_ERR_WORKSPACE;
  if (misaligned(a->edges, 8) || misaligned(a->workspace, 8)) return BNN_ERR_ALIGN;
  k.edges = a->edges;
  k.partial = static_cast<HistPartial*>(a->workspace);
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const int words = k.n_edges - 1 + 4, blocks = k.first_block[k.n_jobs];
  hipLaunchKernelGGL(hist_clear_kernel, dim3((unsigned)((words + kHistBlock - 1) / kHistBlock), (unsigned)k.n_jobs), dim3(kHistBlock), 0,
                     stream, k);
  if (blocks > 0) hipLaunchKernelGGL(hist_bin_kernel, dim3((unsigned)blocks), dim3(kHistBlock), 0, stream, k);
  hipLaunchKernelGGL(hist_fold_kernel, dim3((unsigned)k.n_jobs), dim3(kHistBlock), 0, stream, k);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}
