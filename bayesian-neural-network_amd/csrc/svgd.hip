// F23  SVGD (Liu & Wang 2016) and the kde-WGD repulsive ensemble (D'Angelo & Fortuin 2021) over the members of an F19 weight
// bank: the gradient bucket of F21's step is rewritten in place into the Stein direction  d = A g + B theta  (include/bnn_hip.h
// F23 has the definition).  Three launches, no float atomics, no arrival ticket:
//
//   bnn_svgd_dist       one block per chunk of the bank (whole 64-column tiles, at most 4096 columns, about 512 chunks of a
//                       smaller bank).  A 64-column tile of all members is staged in LDS (column-major, so four members of
//                       a column are one 16-byte read); a thread owns a 4 x 4 block of pairs (i in 4 bi .., j in 4 bj ..,
//                       bi <= bj) and every CL-th column of the tile: two 16-byte LDS reads feed 16 subtract + fma, two
//                       pairs per packed instruction.  The sums are sums of squared DIFFERENCES, never the Gram identity.  A tile's
//                       sum is folded into the chunk's after every tile (chain: <= 64 columns, then <= 64 tiles), the CL
//                       column lanes of a pair are added in lane order at the end: L = 129 (BNN_SVGD_CHAIN).
//   bnn_svgd_coef       one block of 1024 threads, fp64: chunk partials -> D2, bitonic sort of the M^2 entries in LDS -> median
//                       -> h -> K, r -> [A | B] rounded to fp32 once; the fp64 record.
//   bnn_svgd_direction  bucket[:, p] <- [A | B] . [bucket[:, p] ; bank[:, p]] on v_mfma_f32_16x16x4_f32.  A wave owns 64
//                       columns: lane (c = lane & 15, q = lane >> 4) loads the 16 bytes of row 4 ks + q at columns 4 c .. 4 c + 3
//                       -- component e of that load is the B operand (k = q, column c) of the MFMA that produces output
//                       columns 4 c + e, so the D fragments of the four components are again 16 contiguous bytes of a row.
//                       [A | B] sits in LDS as [k][row] with the row rotated by 16 (k & 3): the 64 lanes of an A-operand read
//                       hit 64 different banks.  All 2 M operand rows are read before the first store; columns are owned by
//                       one wave, so in place is safe.
#include "bnn_device.h"
#include "../../include/bnn_hip.h"

#include <cmath>

namespace bnn {
namespace {

constexpr int kSvTile = 64;                       // columns of a staged tile
constexpr int kSvChunk = BNN_SVGD_CHUNK;          // columns of a block of bnn_svgd_dist
constexpr int kSvMaxM = BNN_SVGD_MAX_MEMBERS;
static_assert(kSvChunk % kSvTile == 0 && kSvTile + kSvChunk / kSvTile + 1 == BNN_SVGD_CHAIN, "L of include/bnn_hip.h F23");

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// columns of a block of bnn_svgd_dist: whole 64-column tiles, at most BNN_SVGD_CHUNK, fewer for a small bank so that about 512
// blocks share it (bnn_svgd_chunks)
long chunk_columns(long stride) {
  const long tiles = (stride + 32767) / 32768;
  return 64 * (tiles < kSvChunk / kSvTile ? tiles : (long)(kSvChunk / kSvTile));
}

__host__ __device__ inline int pair_index(int i, int j, int M) { return i * (2 * M - i - 1) / 2 + (j - i - 1); }   // i < j

// ------------------------------------------------------------------------------------------------------------- distances
struct SvDistK {
  const float* bank;
  float* partials;
  long stride;
  int chunk;                         // columns per block
  int M, nb, npb, CL, npairs;        // nb = ceil(M / 4); npb = nb (nb + 1) / 2 pair blocks; CL column lanes per pair block
};

__device__ __forceinline__ void pair_block(int pb, int nb, int& bi, int& bj) {
  bi = 0;
  while (pb >= nb - bi) { pb -= nb - bi; ++bi; }
  bj = bi + pb;
}

__global__ __launch_bounds__(256) void svgd_dist_kernel(const SvDistK k) {
  // the tile [64 columns][LD], LD = 4 nb + 4 floats; after the last tile the same words hold the threads' sums [256][16]
  __shared__ __attribute__((aligned(16))) float lds[kSvTile * (kSvMaxM + 4)];
  const int tid = threadIdx.x, M = k.M, Mp = 4 * k.nb, LD = Mp + 4;
  const long c0 = (long)blockIdx.x * k.chunk;
  const int ntiles = (int)(((k.stride - c0 < k.chunk) ? k.stride - c0 : (long)k.chunk) / kSvTile);
  const int pb = tid / k.CL, cl = tid - pb * k.CL;
  const bool active = pb < k.npb;
  int bi = 0, bj = 0;
  if (active) pair_block(pb, k.nb, bi, bj);
  const int lrow = tid >> 4, lc4 = tid & 15, passes = (Mp + 15) >> 4;
  float4 pre[4];
  auto fetch = [&](int t) {
    const float* __restrict__ src = k.bank + c0 + (long)t * kSvTile + 4 * lc4;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int m = lrow + 16 * p;
      pre[p] = (p < passes && m < M) ? *reinterpret_cast<const float4*>(src + (long)m * k.stride) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  f32x2 acc[8];                        // pairs (u, v), u, v < 4, at [2 u + (v >> 1)][v & 1]: two per packed instruction
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = f32x2{0.f, 0.f};
  if (ntiles > 0) fetch(0);
  for (int t = 0; t < ntiles; ++t) {
    __syncthreads();                               // the previous tile has been consumed
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int m = lrow + 16 * p;
      if (p < passes && m < Mp) {
        lds[(4 * lc4 + 0) * LD + m] = pre[p].x;
        lds[(4 * lc4 + 1) * LD + m] = pre[p].y;
        lds[(4 * lc4 + 2) * LD + m] = pre[p].z;
        lds[(4 * lc4 + 3) * LD + m] = pre[p].w;
      }
    }
    __syncthreads();
    if (t + 1 < ntiles) fetch(t + 1);
    if (active) {
      f32x2 ta[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) ta[e] = f32x2{0.f, 0.f};
      for (int c = cl; c < kSvTile; c += k.CL) {
        const float4 a4 = *reinterpret_cast<const float4*>(&lds[c * LD + 4 * bi]);
        const float4 b4 = *reinterpret_cast<const float4*>(&lds[c * LD + 4 * bj]);
        const float a[4] = {a4.x, a4.y, a4.z, a4.w};
        const f32x2 b[2] = {f32x2{b4.x, b4.y}, f32x2{b4.z, b4.w}};
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int w = 0; w < 2; ++w) {
            const f32x2 d = f32x2{a[u], a[u]} - b[w];
            ta[2 * u + w] = __builtin_elementwise_fma(d, d, ta[2 * u + w]);
          }
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += ta[e];
    }
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < 16; ++e) lds[tid * 16 + e] = acc[e >> 1][e & 1];
  __syncthreads();
  for (int e = tid; e < k.npb * 16; e += 256) {
    const int qb = e >> 4, uv = e & 15;
    int qi, qj;
    pair_block(qb, k.nb, qi, qj);
    const int i = 4 * qi + (uv >> 2), j = 4 * qj + (uv & 3);
    if (i < j && j < M) {
      float s = 0.f;
      for (int l = 0; l < k.CL; ++l) s += lds[(qb * k.CL + l) * 16 + uv];
      k.partials[(long)blockIdx.x * k.npairs + pair_index(i, j, M)] = s;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------- coefficients
struct SvCoefK {
  const float* partials;
  float* coef;
  double* record;
  int M, chunks, method, npairs;
  double s, tau, bandwidth, log_m1;
};

__global__ __launch_bounds__(1024) void svgd_coef_kernel(const SvCoefK k) {
  __shared__ double buf[kSvMaxM * kSvMaxM];        // D2, then the sort's keys, then K
  __shared__ double gsum[1024];
  __shared__ double rs[kSvMaxM];
  __shared__ double hs[2];
  const int t = threadIdx.x, M = k.M, n = M * M, np = k.npairs;
  // 1. the chunk partials, in chunk order, in fp64
  for (int e = t; e < n; e += 1024) buf[e] = 0.0;
  __syncthreads();
  if (np > 0 && np <= 512) {
    const int G = 1024 / np, g = t / np, p = t - g * np, per = (k.chunks + G - 1) / G;
    if (g < G) {
      const int lo = g * per, hi = lo + per < k.chunks ? lo + per : k.chunks;
      double s = 0.0;
#pragma unroll 8
      for (int c = lo; c < hi; ++c) s += (double)k.partials[(long)c * np + p];
      gsum[g * np + p] = s;
    }
    __syncthreads();
    if (t < np) {
      double s = 0.0;
      for (int q = 0; q < G; ++q) s += gsum[q * np + t];
      gsum[t] = s;                                  // (thread t alone reads column t)
    }
    __syncthreads();
  }
  for (int p = t; p < np; p += 1024) {
    double s;
    if (np <= 512) {
      s = gsum[p];
    } else {
      s = 0.0;
#pragma unroll 8
      for (int c = 0; c < k.chunks; ++c) s += (double)k.partials[(long)c * np + p];
    }
    // pair p -> (i, j)
    int i = 0, rem = p;
    while (rem >= M - 1 - i) { rem -= M - 1 - i; ++i; }
    const int j = i + 1 + rem;
    buf[i * M + j] = s;
    buf[j * M + i] = s;
  }
  __syncthreads();
  double d2[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int e = t + 1024 * u;
    d2[u] = e < n ? buf[e] : 0.0;
    if (e < n) k.record[e] = d2[u];
  }
  __syncthreads();
  // 2. the median of all M^2 entries: bitonic sort of N = 2^ceil(log2 n) keys, the tail padded with +inf
  int N = 2;
  while (N < n) N <<= 1;
  for (int e = n + t; e < N; e += 1024) buf[e] = __builtin_huge_val();
  __syncthreads();
  for (int kk = 2; kk <= N; kk <<= 1)
    for (int j = kk >> 1; j > 0; j >>= 1) {
      for (int pi = t; pi < (N >> 1); pi += 1024) {
        const int lo = ((pi & ~(j - 1)) << 1) | (pi & (j - 1)), hi = lo | j;
        const bool asc = (lo & kk) == 0;
        const double a = buf[lo], b = buf[hi];
        if ((a > b) == asc) { buf[lo] = b; buf[hi] = a; }
      }
      __syncthreads();
    }
  if (t == 0) {
    const double med = (n & 1) ? buf[n >> 1] : (buf[(n >> 1) - 1] + buf[n >> 1]) * 0.5;
    double h = k.bandwidth > 0.0 ? k.bandwidth : med / k.log_m1;
    if (h == 0.0) h = 1.0;
    hs[0] = med; hs[1] = h;
    k.record[n] = med;
    k.record[n + 1] = h;
  }
  __syncthreads();
  // 3. K, r
  const double h = hs[1], c2 = 2.0 / h, invM = 1.0 / (double)M;
  double kv[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int e = t + 1024 * u;
    kv[u] = exp(-d2[u] / h);
    if (e < n) buf[e] = kv[u];
  }
  __syncthreads();
  if (t < M) {
    double r = 0.0;
    for (int j = 0; j < M; ++j) r += buf[t * M + j];
    rs[t] = r;
    k.record[n + 2 + t] = r;
  }
  __syncthreads();
  // 4. [A | B], each entry rounded to fp32 once
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int e = t + 1024 * u;
    if (e < n) {
      const int i = e / M, j = e - i * M;
      const double kij = kv[u], r = rs[i], dl = i == j ? 1.0 : 0.0;
      double A, B;
      if (k.method == BNN_SVGD_SVGD) {
        A = k.s * kij * invM;
        B = (k.tau * kij + c2 * (kij - dl * r)) * invM;
      } else {
        A = k.s * dl;
        B = k.tau * dl - c2 * (dl - kij / r);
      }
      k.coef[(long)i * 2 * M + j] = (float)A;
      k.coef[(long)i * 2 * M + M + j] = (float)B;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------- direction
struct SvDirK {
  const float* coef;
  const float* bank;
  float* bucket;
  long stride;
  int M, KG, iters;                  // KG groups of 4 k-steps of 4: the reduction padded to 16 KG >= 2 M
};

template <int MB>
__global__ __launch_bounds__(256) void svgd_direction_kernel(const SvDirK k) {
  extern __shared__ float cs[];      // [16 KG][64]: coefficient (row, kk) at kk * 64 + ((row + 16 (kk & 3)) & 63)
  const int tid = threadIdx.x, M = k.M, K2 = 2 * M, Kp = 16 * k.KG;
  for (int e = tid; e < Kp * 64; e += 256) cs[e] = 0.f;
  __syncthreads();
  for (int e = tid; e < M * K2; e += 256) {
    const int row = e / K2, kk = e - row * K2;
    cs[kk * 64 + ((row + 16 * (kk & 3)) & 63)] = k.coef[e];
  }
  __syncthreads();
  const int wave = tid >> 6, lane = tid & 63, c = lane & 15, q = lane >> 4;
  const float* bank = k.bank;
  float* bucket = k.bucket;            // read and written: no __restrict__
  for (int it = 0; it < k.iters; ++it) {
    const long col = (((long)blockIdx.x * k.iters + it) * 4 + wave) * 64 + 4 * c;
    if (col >= k.stride) break;        // (stride % 64 == 0: a wave's 64 columns are all inside or all outside)
    f32x4 acc[MB][4];
#pragma unroll
    for (int mi = 0; mi < MB; ++mi)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[mi][e] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kg = 0; kg < k.KG; ++kg) {
      float4 v[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int kk = 16 * kg + 4 * s + q;
        v[s] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (kk < M) v[s] = *reinterpret_cast<const float4*>(bucket + (long)kk * k.stride + col);
        else if (kk < K2) v[s] = *reinterpret_cast<const float4*>(bank + (long)(kk - M) * k.stride + col);
      }
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int kk = 16 * kg + 4 * s + q;
#pragma unroll
        for (int mi = 0; mi < MB; ++mi) {
          const float a = cs[kk * 64 + ((16 * mi + c + 16 * q) & 63)];
          acc[mi][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, v[s].x, acc[mi][0], 0, 0, 0);
          acc[mi][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, v[s].y, acc[mi][1], 0, 0, 0);
          acc[mi][2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, v[s].z, acc[mi][2], 0, 0, 0);
          acc[mi][3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, v[s].w, acc[mi][3], 0, 0, 0);
        }
      }
    }
    // lane (c, q), register v of block mi: row 16 mi + 4 q + v, columns col .. col + 3 (one per component)
#pragma unroll
    for (int mi = 0; mi < MB; ++mi)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * mi + 4 * q + r;
        if (row < M)
          *reinterpret_cast<float4*>(bucket + (long)row * k.stride + col) =
              make_float4(acc[mi][0][r], acc[mi][1][r], acc[mi][2][r], acc[mi][3][r]);
      }
  }
}

template <int MB>
void launch_direction(const SvDirK& k, unsigned blocks, size_t lds, hipStream_t st) {
  hipLaunchKernelGGL(svgd_direction_kernel<MB>, dim3(blocks), dim3(256), lds, st, k);
}

bool bad_members(int m) { return m < 1 || m > BNN_SVGD_MAX_MEMBERS; }
bool bad_stride(int64_t s) { return s < 64 || (s & 63) != 0 || s > ((int64_t)1 << 34); }

}  // namespace
}  // namespace bnn

using namespace bnn;

extern "C" int bnn_svgd_dist(const bnn_svgd_dist_args* a, void* stream_) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_svgd_dist_args)) return BNN_ERR_ABI;
  if (bad_members(a->members) || bad_stride(a->stride)) return BNN_ERR_SHAPE;
  if (!a->bank || !a->partials) return BNN_ERR_NULL;
  if (misaligned(a->bank, 16) || misaligned(a->partials, 4)) return BNN_ERR_ALIGN;
  SvDistK k;
  k.bank = a->bank; k.partials = a->partials; k.stride = a->stride; k.M = a->members;
  k.nb = (k.M + 3) / 4;
  k.npb = k.nb * (k.nb + 1) / 2;
  k.CL = 256 / k.npb < kSvTile ? 256 / k.npb : kSvTile;
  k.npairs = k.M * (k.M - 1) / 2;
  k.chunk = (int)chunk_columns(a->stride);
  const long chunks = (a->stride + k.chunk - 1) / k.chunk;
  hipLaunchKernelGGL(svgd_dist_kernel, dim3((unsigned)chunks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream_), k);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}

extern "C" int32_t bnn_svgd_chunks(int64_t stride) {
  if (bad_stride(stride)) return 0;
  const long c = chunk_columns(stride);
  return (int32_t)((stride + c - 1) / c);
}

extern "C" int bnn_svgd_coef(const bnn_svgd_coef_args* a, void* stream_) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_svgd_coef_args)) return BNN_ERR_ABI;
  if (bad_members(a->members) || a->chunks < 1 || a->chunks > (1 << 22)) return BNN_ERR_SHAPE;
  if (!(a->grad_scale > 0.0) || !(a->grad_scale < HUGE_VAL) || !(a->tau >= 0.0) || !(a->tau < HUGE_VAL) || !(a->bandwidth >= 0.0) ||
      !(a->bandwidth < HUGE_VAL))
    return BNN_ERR_SHAPE;
  if (a->method != BNN_SVGD_SVGD && a->method != BNN_SVGD_WGD) return BNN_ERR_ENUM;
  if (!a->partials || !a->coef || !a->record) return BNN_ERR_NULL;
  if (misaligned(a->partials, 4) || misaligned(a->coef, 4) || misaligned(a->record, 8)) return BNN_ERR_ALIGN;
  SvCoefK k;
  k.partials = a->partials; k.coef = a->coef; k.record = a->record;
  k.M = a->members; k.chunks = a->chunks; k.method = a->method; k.npairs = k.M * (k.M - 1) / 2;
  k.s = a->grad_scale; k.tau = a->tau; k.bandwidth = a->bandwidth; k.log_m1 = std::log((double)(k.M + 1));
  hipLaunchKernelGGL(svgd_coef_kernel, dim3(1), dim3(1024), 0, reinterpret_cast<hipStream_t>(stream_), k);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}

extern "C" int bnn_svgd_direction(const bnn_svgd_direction_args* a, void* stream_) {
  if (!a) return BNN_ERR_NULL;
  if (a->struct_bytes != sizeof(bnn_svgd_direction_args)) return BNN_ERR_ABI;
  if (bad_members(a->members) || bad_stride(a->stride)) return BNN_ERR_SHAPE;
  if (!a->coef || !a->bank || !a->bucket) return BNN_ERR_NULL;
  if (misaligned(a->coef, 4) || misaligned(a->bank, 16) || misaligned(a->bucket, 16)) return BNN_ERR_ALIGN;
  SvDirK k;
  k.coef = a->coef; k.bank = a->bank; k.bucket = a->bucket; k.stride = a->stride; k.M = a->members;
  k.KG = (2 * k.M + 15) / 16;
  // a block restages [A | B] (up to 32 KB out of L2): it takes 4 waves x iters tiles of 64 columns, iters growing with the bank
  const long tiles = a->stride / 64;
  k.iters = tiles >= 16 * 4096 ? 4 : tiles >= 8 * 2048 ? 2 : 1;
  const unsigned blocks = (unsigned)((tiles + 4 * k.iters - 1) / (4 * k.iters));
  const size_t lds = (size_t)16 * k.KG * 64 * sizeof(float);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream_);
  switch ((k.M + 15) / 16) {
    case 1: launch_direction<1>(k, blocks, lds, st); break;
    case 2: launch_direction<2>(k, blocks, lds, st); break;
    case 3: launch_direction<3>(k, blocks, lds, st); break;
    default: launch_direction<4>(k, blocks, lds, st); break;
  }
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? BNN_OK : (int)err;
}
