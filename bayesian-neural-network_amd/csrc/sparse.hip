// F13 compressed pruned network (include/bnn_hip.h F13): the network pruned at one level of an F9 sweep as CSR, and its
// forward -- posterior mean or MC over the surviving weights only.  A pruned weight is never stored, read or drawn.
//   bnn_sparse_count   row_ptr = exclusive scan of the per-row survivor counts of a level-code image (integers only)
//   bnn_sparse_fill    col / mu_val / rho_val of the survivors, ascending within a row, placed by ballot + prefix count
//   bnn_sparse_fwd     y[s, r, o] = act(sum_e x[r, col_e] w_e + b_o), one ascending fmaf chain per output element
//
// bnn_sparse_fwd, the partition.  A block is (row group, MC sample, batch block):
//   row group    RG consecutive output features (RG in {4, 8, 16, 32}: the largest that still gives the launch >= 1024 blocks,
//                a pure function of the shape), i.e. the contiguous CSR entries row_ptr[o0] .. row_ptr[o0 + RG];
//   sample       blockIdx.y;
//   batch block  up to 256 batch rows, one per thread (blockDim = 64 .. 256, a multiple of 64).
// The block walks its entries in chunks of kChunk.  Stage A, threads over ENTRIES: w_e = fmaf(sigma_e, eps_e, mu_e) and col_e
// into LDS (double buffered: one barrier per chunk).  The first survivor of each Philox group (4 columns) makes the one
// Philox call and serves every survivor of the group from it.  Stage B, threads over BATCH ROWS: each thread runs its own
// chain acc = fmaf(x[col_e][r], w_e, acc) reading (w_e, col_e) by LDS broadcast (one ds_read_b64, all lanes one address) and x
// feature-major, so the gather of a column is one coalesced 256-byte read per wave; at a row's last entry the thread adds
// the bias, applies the ReLU and stores y.  One chain per output element, in entry order: the result depends on no
// partition.
// Balance.  The unit of work is the ENTRY, not the row: a chunk runs across row boundaries, so within a block an empty
// row costs one store and a full one its length; no wave waits for another's long row.  Between blocks the row groups
// differ by their nnz; with >= 1024 blocks on 256 CUs the dispatcher evens that out (no sorting or splitting of groups:
// SNR pruning of a trained layer leaves rows of similar density -- an assumption, not a measurement).
// What bounds it.  Derived: stage B issues per entry and wave one LDS broadcast read, one 256-byte global read and one fma; the
// vector L1 (64 B / clk / CU) serves a 256-byte read in 4 clocks, so at 50 % of 784-1200-1200-10 (1.2 M entries x 128 rows) the
// L1 read rate would bound the mean forward, with the x panel of a batch block (in x 256 x 4 bytes) resident in L2.  Measured
// (DESIGN.md F13): the mean forward runs at about 0.74 T fma/s, some 25 x below that bound -- a 128-row minibatch with one
// sample is 300 blocks of two waves, each a dependent chain of one gathered load per fma: load latency and too little
// parallelism, by the launch shape (no counter run is recorded).  At 98 % stage B shrinks 25-fold and the fixed costs show:
// a barrier per chunk, the row_ptr walk, the y stores, the launches and, for MC, stage A -- one Philox call per occupied
// group, about one per survivor at that density (survivors rarely share a group), against four weights per call in the
// dense kernels.
#include "bnn_device.h"
#include "../../include/bnn_hip.h"

namespace bnn {
namespace {

constexpr int kWavesPerBlock = 4;
constexpr int kScanBlock = 256;

// one wave per row: the survivors of 64 columns at a time by ballot
__global__ __launch_bounds__(64 * kWavesPerBlock) void sparse_count_kernel(bnn_sparse_count_args a) {
  const int lane = threadIdx.x & 63;
  const int o = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if (o >= a.out_features) return;                                  // wave-uniform
  const uint8_t* __restrict__ c = a.code + (size_t)o * a.ld;
  int n = 0;
  for (int i0 = 0; i0 < a.in_features; i0 += 64) {
    const int i = i0 + lane;
    const bool keep = i < a.in_features && (int)c[i] > a.level;
    n += __popcll(__ballot(keep));
  }
  if (lane == 0) {
    a.row_ptr[o + 1] = n;
    if (o == 0) a.row_ptr[0] = 0;
  }
}

// one block, in place: row_ptr[1 .. out] counts -> inclusive prefix sums (row_ptr[0] = 0 stays)
__global__ __launch_bounds__(kScanBlock) void sparse_scan_kernel(int* __restrict__ row_ptr, int out) {
  __shared__ int s_part[kScanBlock];
  const int per = (out + kScanBlock - 1) / kScanBlock;
  const int lo = threadIdx.x * per, hi = min(lo + per, out);
  int sum = 0;
  for (int i = lo; i < hi; ++i) sum += row_ptr[1 + i];
  s_part[threadIdx.x] = sum;
  __syncthreads();
  int base = 0;
  for (int t = 0; t < (int)threadIdx.x; ++t) base += s_part[t];
  for (int i = lo; i < hi; ++i) {
    base += row_ptr[1 + i];
    row_ptr[1 + i] = base;
  }
}

template <bool TRANSPOSED>
__global__ __launch_bounds__(64 * kWavesPerBlock) void sparse_fill_kernel(bnn_sparse_fill_args a) {
  const int lane = threadIdx.x & 63;
  const int o = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if (o >= a.out_features) return;                                  // wave-uniform
  const uint8_t* __restrict__ c = a.code + (size_t)o * a.ld;
  const int end = a.row_ptr[o + 1];
  int base = a.row_ptr[o];
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int i0 = 0; i0 < a.in_features; i0 += 64) {
    const int i = i0 + lane;
    const bool keep = i < a.in_features && (int)c[i] > a.level;
    const unsigned long long m = __ballot(keep);
    const int e = base + __popcll(m & below);
    if (keep && e < end) {                                          // (e < end: a row_ptr of another level cannot push a store out)
      const size_t src = TRANSPOSED ? (size_t)i * a.out_features + o : (size_t)o * a.in_features + i;
      a.col[e] = (uint16_t)i;
      a.mu_val[e] = a.mu[src];
      a.rho_val[e] = a.rho[src];
    }
    base += __popcll(m);
  }
}

// ------------------------------------------------------------------------------------------------------------ forward
constexpr int kChunk = 512;      // entries per stage: 2 x 512 x 8 bytes of LDS
constexpr int kMaxRG = 32;

struct Entry {
  float w;
  int col;
};

// x [X, rows, in] -> xt [X, in, rows]
__global__ __launch_bounds__(256) void sparse_transpose_kernel(const float* __restrict__ x, float* __restrict__ xt, int rows, int in) {
  __shared__ float s[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int r0 = blockIdx.y * 32, i0 = blockIdx.x * 32;
  const size_t plane = (size_t)blockIdx.z * rows * in;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int r = r0 + ty + 8 * j, i = i0 + tx;
    if (r < rows && i < in) s[ty + 8 * j][tx] = x[plane + (size_t)r * in + i];
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = i0 + ty + 8 * j, r = r0 + tx;
    if (r < rows && i < in) xt[plane + (size_t)i * rows + r] = s[tx][ty + 8 * j];
  }
}

template <int EPS, bool XFM>
__global__ __launch_bounds__(256) void sparse_fwd_kernel(bnn_sparse_fwd_args a, const float* __restrict__ x, int RG) {
#pragma clang fp contract(off)
  __shared__ int s_rp[kMaxRG + 1];
  __shared__ float s_b[kMaxRG];
  __shared__ Entry s_e[2][kChunk];
  const int t = threadIdx.x, nt = blockDim.x;
  const int out = a.out_features, in = a.in_features, rows = a.rows;
  const int o0 = blockIdx.x * RG;
  const int nr = min(RG, out - o0);
  const int s = blockIdx.y;
  const int r = blockIdx.z * nt + t;
  const bool live = r < rows;
  const bool first_batch_block = blockIdx.z == 0;
  uint32_t g = a.sample_offset + (a.sample_counter ? *a.sample_counter : 0u);
  g += a.sample_group ? ((uint32_t)s / a.sample_group) * a.sample_group_stride + (uint32_t)s % a.sample_group : (uint32_t)s;
  const uint32_t k0 = (uint32_t)a.seed, k1 = (uint32_t)(a.seed >> 32);
  const int nnz = a.row_ptr[out];
  if (t <= nr) s_rp[t] = a.row_ptr[o0 + t];
  if (t < nr) {
    const int o = o0 + t;
    float b = a.b_mu[o];
    if (EPS != BNN_EPS_ZERO) {
      float e;
      if (EPS == BNN_EPS_MEMORY) {
        e = a.eps_b[(size_t)s * out + o];
      } else {
        float n4[4];
        philox_normal4((uint32_t)(o >> 2), g, 4u * a.layer_id + 1u, k0, k1, n4);   // eps_b [1, out]: row 0, group o >> 2
        e = n4[o & 3];
      }
      if (a.eps_b_dump && first_batch_block) a.eps_b_dump[(size_t)s * out + o] = e;
      b = __builtin_fmaf(a.b_sigma[o], e, b);
    }
    s_b[t] = b;
  }
  __syncthreads();
  const int j0 = s_rp[0], j1 = s_rp[nr];
  const int xs = a.x_per_sample > 0 ? s / a.x_per_sample : 0;
  const float* __restrict__ xp = x + (size_t)xs * rows * in;
  float* __restrict__ yp = a.y + (size_t)s * rows * out;
  const uint32_t groups_per_row = (uint32_t)((in + 3) >> 2);
  auto emit = [&](int oc, float acc) {
    float v = acc + s_b[oc];
    if (a.relu) v = v > 0.f ? v : 0.f;
    if (live) {
      if (a.y_feature_major) yp[(size_t)(o0 + oc) * rows + r] = v;
      else yp[(size_t)r * out + (o0 + oc)] = v;
    }
  };
  int oc = 0;                                                         // the row the chain in `acc` belongs to (block-uniform)
  float acc = 0.f;
  int buf = 0;
  for (int c0 = j0; c0 < j1; c0 += kChunk, buf ^= 1) {
    const int n = min(kChunk, j1 - c0);
    Entry* __restrict__ se = s_e[buf];
    // ---- stage A: threads over entries
    for (int e = t; e < n; e += nt) {
      const int j = c0 + e;
      const int c = (int)a.col[j];
      if (EPS == BNN_EPS_ZERO) {
        se[e].w = a.mu_val[j];
        se[e].col = c;
      } else if (EPS == BNN_EPS_MEMORY) {
        const float ev = a.eps[(size_t)s * nnz + j];
        if (a.eps_dump && first_batch_block) a.eps_dump[(size_t)s * nnz + j] = ev;
        se[e].w = __builtin_fmaf(a.sigma_val[j], ev, a.mu_val[j]);
        se[e].col = c;
      } else {
        int lo = 0, hi = nr;                                          // the row of entry j: s_rp[lo] <= j < s_rp[lo + 1]
        while (hi - lo > 1) {
          const int mid = (lo + hi) >> 1;
          if (s_rp[mid] <= j) lo = mid; else hi = mid;
        }
        const int row_lo = s_rp[lo], row_hi = s_rp[lo + 1];
        // the first survivor of a Philox group inside this chunk draws for the whole group
        const bool follower = e > 0 && j - 1 >= row_lo && ((int)a.col[j - 1] >> 2) == (c >> 2);
        if (!follower) {
          float n4[4];
          philox_normal4((uint32_t)(o0 + lo) * groups_per_row + (uint32_t)(c >> 2), g, 4u * a.layer_id, k0, k1, n4);
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int jq = j + q;
            if (q > 0 && (e + q >= n || jq >= row_hi)) break;
            const int cq = q == 0 ? c : (int)a.col[jq];
            if ((cq >> 2) != (c >> 2)) break;
            const float ev = (cq & 3) == 0 ? n4[0] : (cq & 3) == 1 ? n4[1] : (cq & 3) == 2 ? n4[2] : n4[3];
            if (a.eps_dump && first_batch_block) a.eps_dump[(size_t)s * nnz + jq] = ev;
            se[e + q].w = __builtin_fmaf(a.sigma_val[jq], ev, a.mu_val[jq]);
            se[e + q].col = cq;
          }
        }
      }
    }
    __syncthreads();
    // ---- stage B: threads over batch rows, the chunk's entries in order
    int e = c0;
    const int cend = c0 + n;
    while (e < cend) {
      while (__builtin_amdgcn_readfirstlane(s_rp[oc + 1]) <= e) {     // rows that end here (empty ones among them)
        emit(oc, acc);
        acc = 0.f;
        ++oc;
      }
      const int hi = min(__builtin_amdgcn_readfirstlane(s_rp[oc + 1]), cend);
      if (live) {
#pragma unroll 8
        for (int q = e; q < hi; ++q) {
          const Entry en = se[q - c0];
          const float xv = XFM ? xp[(size_t)en.col * rows + r] : xp[(size_t)r * in + en.col];
          acc = __builtin_fmaf(xv, en.w, acc);
        }
      }
      e = hi;
    }
  }
  for (; oc < nr; ++oc) {                                             // the last row of the group, and empty rows after it
    emit(oc, acc);
    acc = 0.f;
  }
}

// rows of a group: the largest of 32, 16, 8, 4 that gives the launch >= 1024 blocks (4 if none does)
int row_group(int out, long other_blocks) {
  for (int rg = kMaxRG; rg > 4; rg >>= 1)
    if ((long)((out + rg - 1) / rg) * other_blocks >= 1024) return rg;
  return 4;
}

template <int EPS>
void launch_fwd(const bnn_sparse_fwd_args& a, const float* x, bool xfm, dim3 grid, dim3 block, int rg, hipStream_t stream) {
  if (xfm) hipLaunchKernelGGL((sparse_fwd_kernel<EPS, true>), grid, block, 0, stream, a, x, rg);
  else hipLaunchKernelGGL((sparse_fwd_kernel<EPS, false>), grid, block, 0, stream, a, x, rg);
}

}  // namespace
}  // namespace bnn

using namespace bnn;

extern "C" int bnn_sparse_count(const bnn_sparse_count_args* a, void* stream_) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_sparse_count_args)) return BNN_ERR_ABI;
  if (a->out_features < 1 || a->in_features < 1 || a->ld < a->in_features || a->level < 0 || a->level >= BNN_PRUNE_MAX_LEVELS ||
      (int64_t)a->out_features * a->in_features >= ((int64_t)1 << 31))
    return BNN_ERR_SHAPE;
  if (!a->code || !a->row_ptr) return BNN_ERR_NULL;
  if (misaligned(a->row_ptr, 4)) return BNN_ERR_ALIGN;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const unsigned nb = (unsigned)((a->out_features + kWavesPerBlock - 1) / kWavesPerBlock);
  hipLaunchKernelGGL(sparse_count_kernel, dim3(nb), dim3(64 * kWavesPerBlock), 0, stream, *a);
  hipLaunchKernelGGL(sparse_scan_kernel, dim3(1), dim3(kScanBlock), 0, stream, a->row_ptr, a->out_features);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}

extern "C" int bnn_sparse_fill(const bnn_sparse_fill_args* a, void* stream_) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_sparse_fill_args)) return BNN_ERR_ABI;
  if (a->out_features < 1 || a->in_features < 1 || a->ld < a->in_features || a->in_features > 65536 || a->level < 0 ||
      a->level >= BNN_PRUNE_MAX_LEVELS)
    return BNN_ERR_SHAPE;
  if (!a->code || !a->row_ptr || !a->mu || !a->rho || !a->col || !a->mu_val || !a->rho_val) return BNN_ERR_NULL;
  if (misaligned(a->row_ptr, 4) || misaligned(a->mu, 4) || misaligned(a->rho, 4) || misaligned(a->mu_val, 4) ||
      misaligned(a->rho_val, 4) || misaligned(a->col, 2))
    return BNN_ERR_ALIGN;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const unsigned nb = (unsigned)((a->out_features + kWavesPerBlock - 1) / kWavesPerBlock);
  if (a->transposed) hipLaunchKernelGGL((sparse_fill_kernel<true>), dim3(nb), dim3(64 * kWavesPerBlock), 0, stream, *a);
  else hipLaunchKernelGGL((sparse_fill_kernel<false>), dim3(nb), dim3(64 * kWavesPerBlock), 0, stream, *a);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}

extern "C" int bnn_sparse_fwd(const bnn_sparse_fwd_args* a, void* stream_) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_sparse_fwd_args)) return BNN_ERR_ABI;
  if (a->n_samples < 1 || a->n_samples > 65535 || a->rows < 1 || a->in_features < 1 || a->in_features > 65536 || a->out_features < 1 ||
      a->x_per_sample < 0)
    return BNN_ERR_SHAPE;
  if (a->eps_mode != BNN_EPS_PHILOX && a->eps_mode != BNN_EPS_MEMORY && a->eps_mode != BNN_EPS_ZERO) return BNN_ERR_ENUM;
  if (!a->row_ptr || !a->col || !a->mu_val || !a->x || !a->y || !a->b_mu) return BNN_ERR_NULL;
  if (a->eps_mode != BNN_EPS_ZERO && (!a->sigma_val || !a->b_sigma)) return BNN_ERR_NULL;
  if (a->eps_mode == BNN_EPS_MEMORY && (!a->eps || !a->eps_b)) return BNN_ERR_NULL;
  if (misaligned(a->row_ptr, 4) || misaligned(a->col, 2) || misaligned(a->mu_val, 4) || misaligned(a->sigma_val, 4) ||
      misaligned(a->b_mu, 4) || misaligned(a->b_sigma, 4) || misaligned(a->x, 4) || misaligned(a->y, 4) || misaligned(a->eps, 4) ||
      misaligned(a->eps_b, 4) || misaligned(a->eps_dump, 4) || misaligned(a->eps_b_dump, 4) || misaligned(a->x_scratch, 4) ||
      misaligned(a->sample_counter, 4))
    return BNN_ERR_ALIGN;
  const int waves = a->rows >= 256 ? 4 : (a->rows + 63) / 64;
  const int bdim = 64 * waves;
  const long batch_blocks = (a->rows + bdim - 1) / bdim;
  if (batch_blocks > 65535) return BNN_ERR_SHAPE;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const float* x = a->x;
  bool xfm = a->x_feature_major != 0;
  if (!xfm && a->x_scratch) {
    const int x_rows = a->x_per_sample > 0 ? (a->n_samples + a->x_per_sample - 1) / a->x_per_sample : 1;
    const dim3 tg((unsigned)((a->in_features + 31) / 32), (unsigned)((a->rows + 31) / 32), (unsigned)x_rows);
    if (tg.y > 65535u) return BNN_ERR_SHAPE;
    hipLaunchKernelGGL(sparse_transpose_kernel, tg, dim3(256), 0, stream, a->x, a->x_scratch, a->rows, a->in_features);
    x = a->x_scratch;
    xfm = true;
  }
  const int rg = row_group(a->out_features, (long)a->n_samples * batch_blocks);
  const dim3 grid((unsigned)((a->out_features + rg - 1) / rg), (unsigned)a->n_samples, (unsigned)batch_blocks);
  if (a->eps_mode == BNN_EPS_ZERO) launch_fwd<BNN_EPS_ZERO>(*a, x, xfm, grid, dim3(bdim), rg, stream);
  else if (a->eps_mode == BNN_EPS_MEMORY) launch_fwd<BNN_EPS_MEMORY>(*a, x, xfm, grid, dim3(bdim), rg, stream);
  else launch_fwd<BNN_EPS_PHILOX>(*a, x, xfm, grid, dim3(bdim), rg, stream);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}
