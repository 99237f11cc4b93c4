// F10 pool-based active learning (include/bnn_hip.h F10): the acquisition step on the device.
//   bnn_acquire_topk     the k best candidates of a scored pool in a total order, the mask and the labelled list updated
//   bnn_acquire_compose  the labelled subset's epoch order from a permutation of its positions
//   bnn_acquire_random   one Philox uniform per row: the "random" acquisition
// Integer atomics only; no block waits for another (separate launches behind the one entry): bitwise reproducible.
#include "bnn_device.h"
#include "../../include/bnn_hip.h"

namespace bnn {
namespace {

constexpr int kAcqBits = 12;                      // key bits per pass
constexpr int kAcqBins = 1 << kAcqBits;           // 16 KiB of LDS counters
constexpr int kAcqPasses = 4;                     // 48 key bits: 32 of the score, 16 of the row index
constexpr int kAcqBlock = 256;
constexpr int kAcqRowsPerThread = 8;
constexpr int kSortBlock = 512;
static_assert(BNN_EPOCH_MAX_ROWS <= (1 << 16), "the row index takes 16 key bits");
static_assert(kAcqBins % kAcqBlock == 0, "a thread scans a whole run of bins");

// workspace: the four passes' histograms, the compaction counter (+ padding), the winners' keys
constexpr size_t kAcqHistBytes = sizeof(uint32_t) * kAcqPasses * kAcqBins;
constexpr size_t kAcqZeroBytes = kAcqHistBytes + 16;
constexpr size_t kAcqWorkspaceBytes = kAcqZeroBytes + sizeof(unsigned long long) * BNN_ACQUIRE_MAX_K;

// Ascending 48-bit key of (score descending, index ascending): the order-preserving image of the score (bnn_snr_select's),
// inverted; -0.0 as +0.0; every NaN above every number.
__device__ __forceinline__ unsigned long long acquire_key(float v, uint32_t i) {
  uint32_t u = __float_as_uint(v);
  uint32_t d;
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) {
    d = 0xFFFFFFFFu;
  } else {
    if ((u & 0x7FFFFFFFu) == 0u) u = 0u;
    d = ~((u & 0x80000000u) ? ~u : (u | 0x80000000u));                            // <= 0xFFFFFFFE: only a NaN's bits give 0
  }
  return ((unsigned long long)d << 16) | i;
}

// What the histograms of passes 0 .. passes-1 say about the m-th smallest key, m = min(k, candidates): its leading digits
// (`prefix`), its rank among the keys that share them, and m.  Every thread of the block returns the same values.
struct AcqTarget {
  unsigned long long prefix;
  uint32_t rank, m;
};
__device__ AcqTarget acquire_replay(const uint32_t* __restrict__ hist, int passes, uint32_t k, uint32_t* s_scan, uint32_t* s_res) {
  constexpr int kRun = kAcqBins / kAcqBlock;
  const int t = threadIdx.x;
  AcqTarget tg{0ull, 0u, k};
  for (int q = 0; q < passes; ++q) {
    const uint32_t* h = hist + q * kAcqBins + t * kRun;
    uint32_t part = 0;
#pragma unroll
    for (int b = 0; b < kRun; ++b) part += h[b];
    uint32_t v = part;
    __syncthreads();                                                               // s_scan, s_res of the round before are read
    s_scan[t] = v;
    __syncthreads();
    for (int off = 1; off < kAcqBlock; off <<= 1) {
      const uint32_t add = t >= off ? s_scan[t - off] : 0u;
      __syncthreads();
      v += add;
      s_scan[t] = v;
      __syncthreads();
    }
    if (q == 0) {                                                                  // pass 0 counts every candidate
      const uint32_t total = s_scan[kAcqBlock - 1];
      tg.m = k < total ? k : total;
      if (tg.m == 0u) return tg;                                                   // block-uniform
      tg.rank = tg.m - 1u;
    }
    const uint32_t excl = v - part;
    if (tg.rank >= excl && tg.rank < v) {                                          // one thread: the rank lies in its run
      uint32_t cum = excl, digit = kRun - 1;
      for (int b = 0; b < kRun; ++b) {
        const uint32_t c = h[b];
        if (tg.rank < cum + c) { digit = b; break; }
        cum += c;
      }
      s_res[0] = (uint32_t)(t * kRun) + digit;
      s_res[1] = tg.rank - cum;
    }
    __syncthreads();
    tg.prefix = (tg.prefix << kAcqBits) | s_res[0];
    tg.rank = s_res[1];
  }
  return tg;
}

// pass p: the histogram of digit p of the candidates' keys that share the target's leading p digits
__global__ __launch_bounds__(kAcqBlock) void acquire_hist_kernel(const float* __restrict__ scores, const uint8_t* __restrict__ candidate,
                                                                 uint32_t N, uint32_t k, uint32_t* hist, int pass) {
  __shared__ uint32_t s_hist[kAcqBins];
  __shared__ uint32_t s_scan[kAcqBlock];
  __shared__ uint32_t s_res[2];
  const AcqTarget tg = acquire_replay(hist, pass, k, s_scan, s_res);
  if (pass > 0 && tg.m == 0u) return;                                              // block-uniform: an empty pool
  for (int i = threadIdx.x; i < kAcqBins; i += kAcqBlock) s_hist[i] = 0u;
  __syncthreads();
  const int shift = kAcqBits * (kAcqPasses - 1 - pass);
  const uint32_t nt = gridDim.x * kAcqBlock;
  for (uint32_t i = blockIdx.x * kAcqBlock + threadIdx.x; i < N; i += nt) {
    if (!candidate[i]) continue;
    const unsigned long long key = acquire_key(scores[i], i);
    if (pass == 0 || (key >> (shift + kAcqBits)) == tg.prefix) atomicAdd(&s_hist[(uint32_t)(key >> shift) & (kAcqBins - 1)], 1u);
  }
  __syncthreads();
  uint32_t* out = hist + pass * kAcqBins;
  for (int i = threadIdx.x; i < kAcqBins; i += kAcqBlock)
    if (s_hist[i]) atomicAdd(&out[i], s_hist[i]);
}

// the keys up to the m-th smallest, in any order (the keys are distinct: exactly m of them)
__global__ __launch_bounds__(kAcqBlock) void acquire_compact_kernel(const float* __restrict__ scores, const uint8_t* __restrict__ candidate,
                                                                    uint32_t N, uint32_t k, const uint32_t* hist, uint32_t* count,
                                                                    unsigned long long* __restrict__ keys) {
  __shared__ uint32_t s_scan[kAcqBlock];
  __shared__ uint32_t s_res[2];
  const AcqTarget tg = acquire_replay(hist, kAcqPasses, k, s_scan, s_res);
  if (tg.m == 0u) return;
  const uint32_t nt = gridDim.x * kAcqBlock;
  for (uint32_t i = blockIdx.x * kAcqBlock + threadIdx.x; i < N; i += nt) {
    if (!candidate[i]) continue;
    const unsigned long long key = acquire_key(scores[i], i);
    if (key <= tg.prefix) {
      const uint32_t pos = atomicAdd(count, 1u);
      if (pos < (uint32_t)BNN_ACQUIRE_MAX_K) keys[pos] = key;
    }
  }
}

// one block: bitonic sort of the winners' keys in LDS, then everything the launch promises
__global__ __launch_bounds__(kSortBlock) void acquire_finish_kernel(bnn_acquire_topk_args a, const uint32_t* count,
                                                                    const unsigned long long* __restrict__ keys) {
  __shared__ unsigned long long s_key[BNN_ACQUIRE_MAX_K];
  uint32_t m = *count;
  if (m > (uint32_t)a.k) m = (uint32_t)a.k;                                        // (never: the keys are distinct)
  uint32_t n = 2;
  while (n < m) n <<= 1;                                                           // <= BNN_ACQUIRE_MAX_K
  for (uint32_t i = threadIdx.x; i < n; i += kSortBlock) s_key[i] = i < m ? keys[i] : ~0ull;
  __syncthreads();
  for (uint32_t size = 2; size <= n; size <<= 1) {
    for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
      for (uint32_t i = threadIdx.x; i < (n >> 1); i += kSortBlock) {
        const uint32_t lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
        const unsigned long long x = s_key[lo], y = s_key[hi];
        if ((x > y) == ((lo & size) == 0u)) {
          s_key[lo] = y;
          s_key[hi] = x;
        }
      }
      __syncthreads();
    }
  }
  int32_t n0 = *a.n_labelled;
  if (n0 < 0) n0 = 0;
  for (uint32_t i = threadIdx.x; i < (uint32_t)a.k; i += kSortBlock) {
    if (i < m) {
      const int32_t row = (int32_t)(s_key[i] & 0xFFFFu);                           // < N: formed from a row of this launch
      a.selected[i] = row;
      a.candidate[row] = 0;
      if ((long)n0 + i < (long)a.n_rows) a.labelled[n0 + i] = row;
    } else {
      a.selected[i] = -1;
    }
  }
  __syncthreads();                                                                 // every thread has read *n_labelled
  if (threadIdx.x == 0) {
    *a.n_labelled = n0 + (int32_t)m;
    if (a.n_selected) *a.n_selected = (int32_t)m;
  }
}

__global__ __launch_bounds__(kAcqBlock) void acquire_compose_kernel(const int32_t* __restrict__ labelled, const int32_t* __restrict__ perm,
                                                                    int32_t* __restrict__ order, int32_t n) {
  const int32_t i = blockIdx.x * kAcqBlock + threadIdx.x;
  if (i >= n) return;
  int32_t p = perm[i];
  if (p < 0 || p >= n) p = i;                                                      // a caller's permutation is not trusted with addresses
  order[i] = labelled[p];
}

// a thread per Philox call: four rows
__global__ __launch_bounds__(kAcqBlock) void acquire_random_kernel(float* __restrict__ scores, uint32_t N, uint32_t k0, uint32_t k1,
                                                                   uint32_t round) {
  const uint32_t g = blockIdx.x * kAcqBlock + threadIdx.x;
  if (4u * g >= N) return;
  const uint4 r = philox4x32<>(make_uint4(g, round, 3u, 1u), k0, k1);
  const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (4u * g + i < N) scores[4u * g + i] = (float)(w[i] >> 8) * 0x1p-24f;          // 24 bits: exact in fp32
}

}  // namespace
}  // namespace bnn

using namespace bnn;

extern "C" size_t bnn_acquire_topk_workspace_bytes(void) { return kAcqWorkspaceBytes; }

extern "C" int bnn_acquire_topk(const bnn_acquire_topk_args* a, void* stream_) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_acquire_topk_args)) return BNN_ERR_ABI;
  if (a->n_rows < 1 || a->n_rows > BNN_EPOCH_MAX_ROWS || a->k < 1 || a->k > BNN_ACQUIRE_MAX_K) return BNN_ERR_SHAPE;
  if (!a->scores || !a->candidate || !a->selected || !a->labelled || !a->n_labelled) return BNN_ERR_NULL;
  if (!a->workspace || a->workspace_bytes < kAcqWorkspaceBytes) return BNN_ERR_WORKSPACE;
  if (misaligned(a->scores, 4) || misaligned(a->selected, 4) || misaligned(a->labelled, 4) || misaligned(a->n_labelled, 4) ||
      misaligned(a->n_selected, 4) || misaligned(a->workspace, 8))
    return BNN_ERR_ALIGN;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  char* ws = static_cast<char*>(a->workspace);
  uint32_t* hist = reinterpret_cast<uint32_t*>(ws);
  uint32_t* count = reinterpret_cast<uint32_t*>(ws + kAcqHistBytes);
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(ws + kAcqZeroBytes);
  hipError_t err = hipMemsetAsync(ws, 0, kAcqZeroBytes, stream);
  if (err != hipSuccess) return (int)err;
  const uint32_t N = (uint32_t)a->n_rows, k = (uint32_t)a->k;
  const unsigned blocks = (N + kAcqBlock * kAcqRowsPerThread - 1) / (kAcqBlock * kAcqRowsPerThread);
  for (int pass = 0; pass < kAcqPasses; ++pass)
    hipLaunchKernelGGL(acquire_hist_kernel, dim3(blocks), dim3(kAcqBlock), 0, stream, a->scores, a->candidate, N, k, hist, pass);
  hipLaunchKernelGGL(acquire_compact_kernel, dim3(blocks), dim3(kAcqBlock), 0, stream, a->scores, a->candidate, N, k, hist, count, keys);
  hipLaunchKernelGGL(acquire_finish_kernel, dim3(1), dim3(kSortBlock), 0, stream, *a, count, keys);
  err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}

extern "C" int bnn_acquire_compose(const int32_t* labelled, const int32_t* perm, int32_t* order, int32_t n, void* stream_) {
  if (!labelled || !perm || !order) return BNN_ERR_NULL;
  if (n < 1 || n > BNN_EPOCH_MAX_ROWS) return BNN_ERR_SHAPE;
  if (misaligned(labelled, 4) || misaligned(perm, 4) || misaligned(order, 4)) return BNN_ERR_ALIGN;
  hipLaunchKernelGGL(acquire_compose_kernel, dim3((unsigned)((n + kAcqBlock - 1) / kAcqBlock)), dim3(kAcqBlock), 0,
                     reinterpret_cast<hipStream_t>(stream_), labelled, perm, order, n);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}

extern "C" int bnn_acquire_random(float* scores, int32_t n_rows, uint64_t seed, uint32_t round, void* stream_) {
  if (!scores) return BNN_ERR_NULL;
  if (n_rows < 1 || n_rows > BNN_EPOCH_MAX_ROWS) return BNN_ERR_SHAPE;
  if (misaligned(scores, 4)) return BNN_ERR_ALIGN;
  const unsigned groups = ((unsigned)n_rows + 3u) / 4u;
  hipLaunchKernelGGL(acquire_random_kernel, dim3((groups + kAcqBlock - 1) / kAcqBlock), dim3(kAcqBlock), 0,
                     reinterpret_cast<hipStream_t>(stream_), scores, (uint32_t)n_rows, (uint32_t)seed, (uint32_t)(seed >> 32), round);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}
