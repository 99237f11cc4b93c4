/*
 * bnn_hip.h — C ABI of libbnn_hip.so: the MI355X (gfx950) kernels behind the
 * Bayes-by-backprop hot path of tennisonliu/bayesian-neural-network.
 *
 * The reference has no FFI of its own: its boundary is the Python nn.Module surface of
 * networks.py.  This header is the build-side boundary underneath that surface; every
 * entry point names the reference lines (paths relative to the reference tree) whose
 * arithmetic it replaces.  Callers: bayesian-neural-network_amd/bnn_hip/_lib.py (ctypes).
 *
 * Conventions (all entry points)
 *   - extern "C", plain pointers and sizes, no C++/torch types, no exceptions.
 *   - Return int: 0 = BNN_OK, <0 = argument error (enum below), >0 = a hipError_t.
 *   - Every pointer is a caller-owned DEVICE pointer (contiguous, row-major, fp32 unless a
 *     dtype field says otherwise).  The library never allocates, frees, copies, synchronises
 *     or retains a pointer: launch functions only enqueue kernels on `stream`
 *     (a hipStream_t passed as void*; NULL = the null stream), so they are hipGraph-capturable.
 *   - Workspaces are caller-allocated; sizes come from the *_workspace_bytes queries.
 *   - Re-entrant for distinct streams/buffers; no global mutable state.
 *   - Structs start with `struct_bytes` = sizeof(the struct) as the caller compiled it;
 *     a mismatch returns BNN_ERR_ABI.
 *
 * Epsilon generator (map version BNN_EPS_MAP_VERSION; results must not depend on tiling, launch shape or #GPUs)
 *   Philox4x32 with BNN_PHILOX_ROUNDS = 7 rounds (Salmon et al., SC'11: the round function and key schedule of
 *   rocRAND's PHILOX4_32_10; 7 rounds is the variant the paper reports as passing BigCrush, 10 its default safety
 *   margin) keyed by the 64-bit seed.  Map version 1 (rounds 1-2 of this repository) ran 10 rounds: the kernels that
 *   draw eps per weight are bound by this integer arithmetic (20 -> 14 v_mad_u64_u32 per 4 normals; measured
 *   238 -> 197 cycles per 4 normals per SIMD, the per-8-weights body of K1b 533 -> 424: DESIGN.md 4), so version 2
 *   trades the margin for 20 % of the generator.  tests/test_oracle_golden.py checks the 10-round form of the SAME code
 *   against the Random123 known-answer vectors and the 7-round outputs for avalanche, bit balance, moments, a
 *   Kolmogorov-Smirnov distance and cross-stream correlation.
 *   For an epsilon tensor of logical shape [rows, cols] belonging to
 *   GLOBAL MC sample index g (= sample_offset + local sample), tensor id
 *   t = 4*layer_id + kind  (kind 0: BBB weight eps [out,in]; 1: bias eps [1,out];
 *   2: LR activation eps [batch,out]):
 *       group  = row * ceil(cols/4) + (col >> 2)           (uint32)
 *       counter = (group, g, t, 0), key = (seed_lo, seed_hi)
 *       (r0,r1,r2,r3) = Philox4x32-R(counter, key), R = BNN_PHILOX_ROUNDS
 *       u(r) = fma((float)r, 2^-32, 2^-33)                  in (0,1]
 *       slot 0,1 = sqrt(-2 ln u(r0)) * {cos, sin}(2 pi u(r1)); slot 2,3 likewise from r2,r3
 *       eps[row, col] = slot (col & 3)
 *   oracle/bnn_oracle.py:philox_normal restates this on the CPU.  On the device the map is stated once, next to the generator
 *   in csrc/bnn_device.h: kEpsWeight .. kEpsDropout, eps_tensor_id, eps_groups_per_row, eps_group, eps_slot, eps_bias,
 *   eps_global_sample; every kernel's forward and backward call those.
 *   Kind 3: the MC-dropout uniform of the activations that leave Linear layer l (an MLP_Dropout's nn.Dropout after the
 *   ReLU of Linear l), logical shape [batch, features], same counter layout, t = 4*l + 3:
 *       (r0,r1,r2,r3) = Philox4x32-R((group, g, 4*l + 3, 0), key)
 *       keep[row, col] = r_(col & 3) >= thr,   thr = min(floor(p * 2^32), 2^32 - 1)   (host, fp64; p in [0, 1))
 *       out = keep ? a * scale : 0,            scale = (float)(1.0 / (1.0 - p))
 *   (p = 0.5: thr = 2^31, scale = 2.)  No other stream uses word 2 = 4l + 3 with word 3 = 0 (the bandit's stream has
 *   word 3 = 1), so adding kind 3 left every earlier stream, and the map version, as they were.  bnn_dropout_mask
 *   materialises it; tests/test_mc_dropout_cpu.py restates it on the CPU.
 */
#ifndef BNN_HIP_H_
#define BNN_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BNN_HIP_ABI_VERSION 9
#define BNN_EPS_MAP_VERSION 2     /* 1: Philox4x32-10 (rounds 1-2); 2: Philox4x32-7 */
#ifndef BNN_PHILOX_ROUNDS          /* build-time choice (csrc/Makefile: make PHILOX_ROUNDS=10): 7 = map version 2 (the product), */
#define BNN_PHILOX_ROUNDS 7        /* 10 = rocRAND's PHILOX4_32_10 / map version 1.  bnn_philox_rounds() tells what a library runs */
#endif

enum bnn_status {
  BNN_OK = 0,
  BNN_ERR_NULL = -1,        /* required pointer is NULL */
  BNN_ERR_SHAPE = -2,       /* non-positive or unsupported dimension */
  BNN_ERR_ENUM = -3,        /* unknown dtype / mode / prior kind */
  BNN_ERR_WORKSPACE = -4,   /* workspace missing or too small */
  BNN_ERR_ABI = -5,         /* struct_bytes mismatch */
  BNN_ERR_ALIGN = -6        /* pointer not aligned to its element type */
};

enum bnn_dtype { BNN_F32 = 0, BNN_BF16 = 1 };

/* Arithmetic of the matmul.  BNN_MATH_F32: exact fp32 MFMA (v_mfma_f32_16x16x4_f32, a
 * k-ordered fmaf chain) — the parity mode.  BNN_MATH_BF16: operands rounded to bf16 (RNE),
 * fp32 accumulate (v_mfma_f32_16x16x32_bf16) — the throughput mode.  Statistics (log-probs,
 * KL) are always formed in fp32 from the un-rounded fp32 weights.  The x^2 operand of the LR variance product
 * (networks.py:121) in BNN_MATH_BF16 is bf16(bf16(x)^2) — the square of the rounded activation, rounded — for every kernel
 * form: the x_sq / y_sq / cast_dst_sq streams hold exactly what a kernel squaring the bf16 x it loaded computes, so which
 * forms a launch plan picks never changes a result bit. */
enum bnn_math { BNN_MATH_F32 = 0, BNN_MATH_BF16 = 1, BNN_MATH_BF16X3 = 2 };
/* BNN_MATH_BF16X3 (BBB forward): split-bf16 operands on the bf16 matrix core.  Every matmul operand v is carried as the pair
 *     hi = bf16(v),   lo = bf16(v - hi)            (both round-to-nearest-even; v - hi is exact in fp32)
 * and a product a . b is accumulated in fp32 as  a_hi b_hi + a_lo b_hi + a_hi b_lo  (three v_mfma_f32_16x16x32_bf16 per tile
 * and k-step; the lo.lo term, 2^-16 of the product, is dropped): |a b - (...)| <= ~2^-15 |a b| per product against 2^-8 for
 * BNN_MATH_BF16, i.e. the reference's fp32 F.linear (networks.py:88) to ~1e-5 of the output scale -- ELBO rtol 1e-4 at every
 * beta of classification/class_task.py:70 -- at 3/16 of the matrix-core time of the exact-fp32 MFMA.  bf16 activations of
 * this mode are PAIRS of planes: x / x_lo and y / y_lo below (fp32 activations are split in registers).  Statistics are
 * fp32 from the un-rounded weights as in every mode. */

enum bnn_eps_mode {
  BNN_EPS_PHILOX = 0,   /* generated on chip (map above); never touches HBM */
  BNN_EPS_MEMORY = 1,   /* read from eps_* buffers: identical-eps parity with the reference */
  BNN_EPS_ZERO = 2      /* eps = 0: w = mu (networks.py:78-79, eval & sample=False) */
};

enum bnn_prior_kind {
  BNN_PRIOR_GAUSS = 0,    /* Normal(0, sigma_p)                 networks.py:67-68 */
  BNN_PRIOR_MIXTURE = 1   /* pi N(0,sigma1) + (1-pi) N(0,sigma2) networks.py:14-27 */
};

enum bnn_nll_mode { BNN_NLL_REGRESSION = 0, BNN_NLL_CLASSIFICATION = 1 };

/* Kernel forms of a layer launch.  TILE: one block per (feature tile, sample, batch block), the block's
 * waves split the reduction and meet in LDS -- few samples in flight.  GEMM: block GEMM, the x tile shared
 * through LDS by LDS-DMA, a wave owns 16 features for all of K -- many samples.  GEMM_KSLICE (BBB): the GEMM
 * form with the reduction cut into slices whose fp32 partial tiles a second kernel sums in slice order.
 * BLOCK256 (BBB, matmul half over w_sampled only): one 8-wave block per 256 x 256 output tile, both operands
 * through LDS by LDS-DMA, ping-pong MFMA / load segments -- layers fed >= 512 batch rows, where the bf16
 * matrix cores, not the sampling, bound the layer (K1g, csrc/bbb_block_gemm.h). */
enum bnn_form { BNN_FORM_AUTO = 0, BNN_FORM_TILE = 1, BNN_FORM_GEMM = 2, BNN_FORM_GEMM_KSLICE = 3, BNN_FORM_BLOCK256 = 4 };

typedef struct bnn_prior {
  int32_t kind;      /* bnn_prior_kind */
  float sigma_p;     /* Gaussian prior scale (prior_init[0])            */
  float pi;          /* mixture weight       (prior_init[0] if mixture) */
  float sigma1;      /* exp(prior_init[1])                              */
  float sigma2;      /* exp(prior_init[2])                              */
} bnn_prior;

/* ------------------------------------------------------------------------------------
 * Launch plans.  The geometry of a forward layer launch is a pure function of the shape and of what the
 * arguments allow -- never of pointers' values, streams or the environment -- so one shape always runs one
 * summation order (bitwise reproducible), and the function is testable without a device.
 * bnn_bbb_plan / bnn_lr_plan return what bnn_bbb_linear_fwd / bnn_lr_linear_fwd will launch for `a`
 * (only the shape, dtype, math, form, alignment of the pointers and presence of the optional buffers are read).
 * ---------------------------------------------------------------------------------- */
typedef struct bnn_plan {
  int32_t form;          /* bnn_form taken */
  int32_t k_classes;     /* TILE: R k-range classes of the 16 MFMA rows; a tile holds 16 / R features */
  int32_t waves;         /* waves per block */
  int32_t batch_rows;    /* batch rows per block */
  int32_t k_slices;      /* GEMM_KSLICE: reduction slices (1 otherwise) */
  int32_t blocks;        /* work items (the grid is padded to a multiple of 8) */
  int32_t lds_bytes;     /* LDS per block */
  int32_t features_per_block;
} bnn_plan;

/* ------------------------------------------------------------------------------------
 * K1  bnn_bbb_linear_fwd — BayesianLinear.forward for n_samples MC samples in ONE launch.
 * Replaces networks.py:73-88 (+ :39-46 GaussianNode, :14-27 / :67-68 priors) and the
 * serial MC loop over it (networks.py:199-200) for one layer:
 *     w_s = mu + softplus(rho) * eps_s       (per weight and bias, never stored)
 *     y_s = x_s . w_s^T + b_s  [-> ReLU]     (networks.py:88, :169-171)
 *     stats partials for log p(w_s), log q(w_s)   (networks.py:82-83)
 * Shapes: x [x_rows, batch, in] (x_rows = 1 if x_per_sample == 0, else ceil(n_samples / x_per_sample));
 * w_mu,w_rho [out,in]; b_mu,b_rho [out]; eps_w [n_samples,out,in]; eps_b [n_samples,out];
 * y [n_samples, batch, out].
 *
 * Sample groups.  The n_samples of a launch may be G independent minibatches x S MC samples each
 * (sample s = minibatch s / S, MC sample s % S): the reference evaluates minibatches one after the
 * other (classification/class_task.py:66-79 trains, :89-103 evaluates), but given the parameters
 * their forward passes are independent, so a stream of minibatches is batched into one launch per
 * layer exactly like the MC samples of one minibatch.  x_per_sample = S then gives the first layer
 * one x per minibatch, and (sample_group = S_local, sample_group_stride = S_global) keeps the Philox
 * index of (minibatch m, global MC sample j) at sample_offset + m * S_global + j whatever share of
 * the S_global samples this rank owns (results independent of the number of GPUs).
 *
 * Stats workspace (want_stats != 0): opaque to the caller, produced here and consumed only
 * by this library (the optional per-layer reduction below and bnn_elbo_finalize).  It holds,
 * per (sample, feature tile), the fp32 partial sums {sum eps^2, sum w^2 (Gaussian prior) or
 * sum log p_mix(w) (mixture prior), sum log sigma} over the tile's weights and biases, plus a
 * one-entry header with the tile count, so the launch geometry may change between library
 * versions without touching callers.  One partial per block, no atomics.
 * If log_prior/log_q are non-NULL a second tiny kernel reduces the partials to the
 * layer's per-sample scalars float[n_samples] (the values BayesianLinear stores in
 * self.log_prior / self.log_variational_posterior).
 * ---------------------------------------------------------------------------------- */
struct bnn_bbb_sample_args;

/* Piece order of a bf16 activation tensor [rows, batch, features] (bnn_bbb_fwd_args.x_layout / y_layout, bnn_prepare_args.cast_layout):
 * the order in which the pair block GEMM (the BNN_FORM_GEMM plan of 8 waves, bf16 math) stages x, so that each of its LDS-DMA pieces
 * -- 16 batch rows x 32 features, one 16-byte chunk per lane -- is 1 KiB of whole, 128-byte aligned lines instead of sixteen 64-byte
 * row segments at a 2 * features byte stride:
 *     [row][batch block of 128][k-step t = feature / 32][batch tile m (8)][lane (64)][8 bf16]
 * lane (r = lane & 15, q = lane >> 4) of piece (t, m) holds x[128 * block + 16 * m + r][32 * t + 8 * q .. + 7].  Features are padded to
 * a multiple of 32 and batch rows to a multiple of 128 with ZEROS -- rows * ceil(batch / 128) * ceil(features / 32) * 8192 bytes in
 * all, 16-byte aligned: the caller allocates the buffer zeroed and no launch writes a pad position.  That plan reads and writes the layout,
 * and the one-launch output layer of bnn_bbb_final_fwd (one 16-feature tile, batch <= 128, bf16 math, sampling in the launch) READS
 * it as its x -- the lane geometry of its fragments is the piece's; every other launch handed a BNN_LAYOUT_PIECES operand returns
 * BNN_ERR_ENUM -- bnn_bbb_final_fwd for a piece-order y or w_pieces, over pre-sampled weights, in fp32 or split-bf16 math and wherever
 * it would run as two launches -- (the plan itself, bnn_bbb_plan, does not depend on the layouts); the split-bf16 form of the plan
 * refuses it too (its operands are plane pairs). */
typedef enum bnn_layout { BNN_LAYOUT_ROWS = 0, BNN_LAYOUT_PIECES = 1 } bnn_layout;

typedef struct bnn_bbb_fwd_args {
  uint32_t struct_bytes;
  int32_t n_samples, batch, in_features, out_features;
  const void* x;
  int32_t x_dtype;          /* bnn_dtype */
  int32_t x_per_sample;     /* 0: one x for all samples; g >= 1: sample s reads x[s / g] (1: one x per sample) */
  const float* w_mu;
  const float* w_rho;
  const float* b_mu;
  const float* b_rho;
  int32_t eps_mode;         /* bnn_eps_mode */
  int32_t math;             /* bnn_math */
  const float* eps_w;       /* BNN_EPS_MEMORY only */
  const float* eps_b;
  uint64_t seed;            /* BNN_EPS_PHILOX */
  uint32_t layer_id;
  uint32_t sample_offset;   /* global MC index of local sample 0 (multi-GPU shards) */
  const uint32_t* sample_counter; /* optional DEVICE word added to sample_offset at run time, so a
                               captured hipGraph draws fresh eps on every replay (see K4) */
  uint32_t sample_group;    /* 0: global index of local sample s = sample_offset + counter + s.  g > 0: */
  uint32_t sample_group_stride; /* sample_offset + counter + (s / g) * sample_group_stride + s % g      */
  float* eps_w_dump;        /* optional: the eps actually used, [n_samples,out,in] */
  float* eps_b_dump;        /* optional: [n_samples,out] */
  bnn_prior prior;
  int32_t want_stats;
  int32_t relu;             /* fuse ReLU (networks.py:161,163) */
  void* workspace;          /* stats partials, see above */
  size_t workspace_bytes;
  float* log_prior;         /* optional [n_samples] */
  float* log_q;             /* optional [n_samples] */
  void* y;
  int32_t y_dtype;          /* bnn_dtype */
  int32_t form;             /* bnn_form preference: BNN_FORM_AUTO lets the plan choose; another value is taken when
                               the arguments allow that form (bnn_bbb_plan tells), else the plan's own choice.
                               Tests compare the forms with each other through it; bnn_bbb_final_fwd fuses the
                               finalize only under BNN_FORM_AUTO */
  void* split_scratch;      /* optional, 16-byte aligned, >= bnn_bbb_split_scratch_bytes(n_samples, batch, out_features),
                               its first bnn_bbb_split_scratch_zero_bytes(...) bytes zero before the first launch that
                               uses it (launches leave them zero): lets a mid-sized launch (4 .. ~100 samples) split its
                               K range over several blocks; the block of a slice that finishes last adds the slices'
                               fp32 partial tiles up in slice order (bitwise reproducible), in the same launch.  One
                               scratch serves one launch at a time */
  size_t split_scratch_bytes;
  const float* w_sigma;     /* optional [out,in]: softplus(w_rho) from bnn_softplus, computed once per
                               evaluation; the throughput kernel then skips the per-sample softplus */
  const void* w_sampled;    /* optional bf16 [n_samples,out,in] from bnn_bbb_sample_weights: the launch is then the
                               matmul half only, y = act(x . w_sampled^T + b_sampled) -- no sampling, no statistics
                               (want_stats must be 0; w_mu .. eps_* are ignored and may be NULL).  bf16 math,
                               in_features % 8 == 0, 16-byte aligned x and w_sampled */
  const float* b_sampled;   /* with w_sampled: fp32 [n_samples,out] */
  const struct bnn_bbb_sample_args* rider; /* optional: an INDEPENDENT bnn_bbb_sample_weights(rider) job, carried by this
                               launch as extra blocks when it takes the tile form in bf16 math (launched on its own
                               ahead of the layer otherwise: same results).  Sampling depends on no activation: the
                               output layer's weights are drawn beside the layer before it, and the output layer of a
                               few-sample evaluation becomes a matmul-only launch (bnn_bbb_final_fwd, w_sampled) */
  void* y_bf16_copy;        /* optional bf16 [n_samples,batch,out], with y_dtype == BNN_F32: y also in bf16 (for the next
                               layer's forward of a training step, whose backward reads the fp32 y).  Tile form only:
                               selects it */
  void* w_sampled_t_out;    /* optional, with w_sampled and bf16 x: bf16 [n_samples,in,out], the same weights TRANSPOSED,
                               written by this launch.  The layer's backward (bnn_bbb_bwd_args.w_sampled_t) then computes its input
                               gradient as this same matmul-only launch instead of gathering along the reduction */
  const void* x_lo;         /* BNN_MATH_BF16X3 with x_dtype == BNN_BF16: the low plane of x (shaped and strided like x), i.e.
                               bf16(x_fp32 - x) as bnn_eval_prepare (cast_dst_lo) or a previous layer's y_lo left it */
  void* y_lo;               /* BNN_MATH_BF16X3 with y_dtype == BNN_BF16: the low plane of y, bf16(y_fp32 - y) after bias / ReLU */
  int32_t x_layout;         /* bnn_layout of a bf16 x: BNN_LAYOUT_PIECES = piece order (below) */
  int32_t y_layout;         /* bnn_layout of a bf16 y: BNN_LAYOUT_PIECES = the piece order of the NEXT layer's x; the pad positions of the
                               buffer are never written (the caller zeroes it once) */
  const void* w_pieces;     /* optional, with w_sigma: (w_mu, w_sigma) once more in the piece order of the same plan, as bnn_eval_prepare
                               (pieces) wrote it from the CURRENT parameters: fp32 [ceil(out / 16) feature tiles][ceil(in / 32) k-steps]
                               [mu lo | mu hi | sigma lo | sigma hi][64 lanes][4] -- lane (r, q) of tile T, k-step t holds
                               mu | sigma [16 T + r][32 t + 8 q + 0..3] in the lo piece and + 4..7 in the hi piece, zero-padded; 16-byte
                               aligned.  The launch then stages its parameters from here (4 KiB contiguous per tile and k-step) and reads
                               w_mu / w_sigma for nothing; same refusals as the piece-order activations */
} bnn_bbb_fwd_args;

size_t bnn_bbb_linear_fwd_workspace_bytes(int32_t n_samples, int32_t out_features);
size_t bnn_bbb_split_scratch_bytes(int32_t n_samples, int32_t batch, int32_t out_features);
size_t bnn_bbb_split_scratch_zero_bytes(int32_t n_samples, int32_t batch, int32_t out_features);
int bnn_bbb_linear_fwd(const bnn_bbb_fwd_args* args, void* stream);
int bnn_bbb_plan(const bnn_bbb_fwd_args* args, bnn_plan* plan);

/* ------------------------------------------------------------------------------------
 * K1s  bnn_bbb_sample_weights — the sampling half of BayesianLinear.forward (networks.py:73-86) for up to
 * BNN_SAMPLE_MAX_LAYERS layers and n_samples MC samples in ONE launch:
 *     w_out[s] = bf16(mu + softplus(rho) * eps_s)  [n_samples,out,in],   b_out[s] likewise, fp32 [n_samples,out]
 * with eps from the Philox map at the top (the same elements K1 would draw for these layer_ids / sample
 * indices), and the per-sample statistics {sum eps^2, sum w^2 | sum log p_mix, sum log sigma} (taken from the
 * fp32 w, as K1 does) in each layer's workspace in K1's format, so bnn_elbo_finalize / bnn_bbb_final_fwd consume
 * them unchanged.  The matmuls then run as bnn_bbb_linear_fwd(w_sampled, b_sampled).  Sampling depends on no
 * activation: out of the layer-after-layer chain of a few-sample evaluation it is one streaming pass over the
 * parameters (8 B read per weight and group of four samples -- a block serves the group from one read and one softplus --
 * + 2 B written per weight and sample).  in_features % 8 == 0; 16-byte aligned pointers.
 * ---------------------------------------------------------------------------------- */
#define BNN_SAMPLE_MAX_LAYERS 8
typedef struct bnn_bbb_sample_layer {
  int32_t in_features, out_features;
  uint32_t layer_id;
  int32_t reserved;
  const float* w_mu;        /* [out,in] */
  const float* w_rho;
  const float* b_mu;        /* [out] */
  const float* b_rho;
  void* w_out;              /* bf16 [n_samples,out,in] */
  float* b_out;             /* [n_samples,out] */
  void* workspace;          /* >= bnn_bbb_sample_workspace_bytes(n_samples, in, out) */
  size_t workspace_bytes;
  bnn_prior prior;
  int32_t reserved2;
} bnn_bbb_sample_layer;

typedef struct bnn_bbb_sample_args {
  uint32_t struct_bytes;
  int32_t n_layers;
  int32_t n_samples;
  uint32_t sample_offset;
  uint64_t seed;
  const uint32_t* sample_counter;   /* optional device word, as in bnn_bbb_fwd_args */
  uint32_t sample_group;            /* sample groups, as in bnn_bbb_fwd_args; 0 = none */
  uint32_t sample_group_stride;
  bnn_bbb_sample_layer layer[BNN_SAMPLE_MAX_LAYERS];
  const float* cast_src;            /* optional rider on the same launch: cast_dst[i] = bf16(cast_src[i]), */
  void* cast_dst;                   /* i < cast_n -- the evaluation's input batch for the bf16 matmuls      */
  int64_t cast_n;                   /* (16-byte aligned pointers); 0 = none                                  */
} bnn_bbb_sample_args;

/* >= bnn_bbb_linear_fwd_workspace_bytes(n_samples, out_features): one workspace serves either form; 0 when
 * in_features % 8 != 0 (the split form does not apply) */
size_t bnn_bbb_sample_workspace_bytes(int32_t n_samples, int32_t in_features, int32_t out_features);
int bnn_bbb_sample_weights(const bnn_bbb_sample_args* args, void* stream);

/* ------------------------------------------------------------------------------------
 * K3  bnn_lr_linear_fwd — BayesianLinearLR.forward (networks.py:116-138) for n_samples
 * MC samples in one launch: two MFMA GEMMs sharing the x tile,
 *     m = x . M,   v = x^2 . softplus(rho)^2          (networks.py:120-121)
 *     y = m + sqrt(v) * eps_act + (b_mu + softplus(b_rho) * eps_b)   (:123-128)
 * with the closed-form KL(q||p) partial sums (networks.py:109-114, :134-136) taken from
 * the same pass over (M, rho).  Weights are [in, out] (networks.py:95-96).
 * eps_act [n_samples,batch,out], eps_b [n_samples,out].
 * KL workspace (want_kl != 0): opaque, as for K1; per feature tile the fp32 partial sums
 * {sum log sigma, sum sigma^2, sum mu^2} over the tile's weights and biases.
 * kl_out (optional, float[3]) = {weight_kl + bias_kl, weight_kl, bias_kl}.
 * ---------------------------------------------------------------------------------- */
/* bnn_lr_rider — what bnn_lr_prepare does for one NARROW layer (out_features <= 16: the output layer of the reference's
 * networks, networks.py:160-164), carried by another layer's launch: the K-sliced form of bnn_lr_linear_fwd (K3s) runs it as a
 * few extra blocks on CUs its own blocks leave idle; any other form launches bnn_lr_prepare ahead of itself.  Either way,
 * after bnn_lr_linear_fwd returns (in stream order) `w_frag` holds the bf16 (M, sigma^2) operands in fragment order and
 * `kl_workspace` the layer's closed-form KL sums -- what bnn_lr_final_fwd takes as bnn_lr_fwd_args.w_frag / .workspace, so
 * that its row blocks park nothing (the one-evaluation chain: 12.4 -> 8 us for the 1200 x 10 layer). */
typedef struct bnn_lr_rider {
  uint32_t struct_bytes;
  int32_t in_features, out_features;
  const float* w_mu;        /* [in, out] */
  const float* w_rho;
  const float* b_mu;        /* [out] */
  const float* b_rho;
  void* w_frag;             /* >= bnn_lr_prepare_bytes(in, out), 16-byte aligned */
  size_t w_frag_bytes;
  void* kl_workspace;       /* >= bnn_lr_linear_fwd_workspace_bytes(out), 16-byte aligned */
  size_t kl_workspace_bytes;
} bnn_lr_rider;

typedef struct bnn_lr_fwd_args {
  uint32_t struct_bytes;
  int32_t n_samples, batch, in_features, out_features;
  const void* x;
  int32_t x_dtype;
  int32_t x_per_sample;     /* as in bnn_bbb_fwd_args */
  const float* w_mu;        /* [in,out] */
  const float* w_rho;
  const float* b_mu;
  const float* b_rho;
  int32_t eps_mode;
  int32_t math;
  const float* eps_act;
  const float* eps_b;
  uint64_t seed;
  uint32_t layer_id;
  uint32_t sample_offset;
  const uint32_t* sample_counter; /* optional device word, as in bnn_bbb_fwd_args */
  uint32_t sample_group;    /* as in bnn_bbb_fwd_args */
  uint32_t sample_group_stride;
  float* eps_act_dump;
  float* eps_b_dump;
  float sigma_p;            /* prior_init[0]; prior mean is 0 (networks.py:103-104) */
  int32_t want_kl;
  int32_t relu;
  int32_t form;             /* bnn_form, as in bnn_bbb_fwd_args */
  void* workspace;
  size_t workspace_bytes;
  float* kl_out;
  void* y;
  int32_t y_dtype;
  int32_t reserved2;
  const void* x_sq;         /* optional bf16 [x_samples,batch,in]: the squares of x as a previous layer's y_sq or
                               bnn_cast_bf16 wrote them (BNN_MATH_BF16: bf16(bf16(x)^2), see bnn_math); lets the throughput kernel
                               stream both GEMM operands of networks.py:120-121 by LDS-DMA */
  void* y_sq;               /* optional bf16 [n_samples,batch,out]: also write the squares of y (after ReLU) for the next layer's x_sq */
  const void* w_frag;       /* optional output of bnn_lr_prepare for these weights: the throughput
                               kernel then streams ready bf16 (M, sigma^2) fragments and the KL
                               workspace is the one bnn_lr_prepare filled (want_kl still set) */
  float* v_out;             /* optional fp32 [n_samples,batch,out]: the pre-activation variance v
                               (networks.py:121) as the kernel computed it; bnn_lr_linear_bwd needs
                               it.  Selects the latency form of the kernel. */
  float* hfac_out;          /* optional fp32 [n_samples,batch,out]: eps_act / (2 sqrt(v)) (0 where v == 0), the factor
                               the backward multiplies the upstream gradient with (h = gz * hfac, see bnn_lr_bwd_args):
                               a hidden layer of a training step saves THIS instead of v and its backward needs no
                               preparation launch.  Selects the latency form of the kernel. */
  void* y_bf16_copy;        /* optional bf16 [n_samples,batch,out], with y_dtype == BNN_F32: y also in bf16.  A training
                               step keeps fp32 activations for the backward and feeds the next layer's forward
                               the bf16 ones (half the bytes through the CU, no conversion in its k loop).
                               Selects the latency form of the kernel. */
  const struct bnn_lr_rider* rider; /* optional: prepare ANOTHER (narrow) LR layer's operands beside this launch -- see bnn_lr_rider */
  void* split_scratch;      /* optional, 16-byte aligned, >= bnn_lr_split_scratch_bytes(n_samples, batch, out_features), its
                               first bnn_lr_split_scratch_zero_bytes(...) bytes zero before the first launch that uses it
                               (the kernel leaves them zero): lets a launch of 1-3 samples on a wide layer split the K
                               range of a 32-feature group over several blocks that meet through it (BNN_FORM_GEMM_KSLICE;
                               bf16 math on bf16 x, in_features % 8 == 0, out_features % 4 == 0).  One launch at a time
                               per scratch.
                               With x_per_sample == 0 and 2 .. 64 samples (no sample groups) -- the first layer of
                               sample_elbo_lr / predict, where the reference runs forward(x) per sample on the same x
                               (networks.py:211-225) -- the two products x M and x^2 sigma^2 are made ONCE per launch and
                               only the bias, the activation noise and the stores run per sample; the scratch then only
                               needs the sizes of n_samples = 1. */
  size_t split_scratch_bytes;
  const void* x_lo;         /* BNN_MATH_BF16X3: the low plane of x (as in bnn_bbb_fwd_args).  In that mode the layer runs the
                               block-GEMM form only: bf16 x with x_lo AND x_sq (in this mode bf16 of the fp32 squares), w_frag from
                               bnn_lr_prepare_x3; the mean product x . M (networks.py:120) in split-bf16 (three MFMAs), the
                               variance product x^2 . sigma^2 (:121) on bf16 operands as in BNN_MATH_BF16 -- the activation
                               noise is a few per cent of the output, its 2^-9 error below the mean's 2^-15 */
  void* y_lo;               /* BNN_MATH_BF16X3 with y_dtype == BNN_BF16: the low plane of y */
} bnn_lr_fwd_args;

size_t bnn_lr_linear_fwd_workspace_bytes(int32_t out_features);
size_t bnn_lr_split_scratch_bytes(int32_t n_samples, int32_t batch, int32_t out_features);
size_t bnn_lr_split_scratch_zero_bytes(int32_t n_samples, int32_t batch, int32_t out_features);
int bnn_lr_linear_fwd(const bnn_lr_fwd_args* args, void* stream);
int bnn_lr_plan(const bnn_lr_fwd_args* args, bnn_plan* plan);


/* bnn_lr_prepare — the eps-independent half of BayesianLinearLR.forward, once per ELBO
 * evaluation instead of once per MC sample (the reference recomputes it inside its sample loop,
 * networks.py:118-119, :134-136): sigma^2 = softplus(rho)^2, both GEMM operands rounded to bf16
 * and stored in MFMA fragment order, plus the closed-form KL sums into kl_workspace (optional). */
size_t bnn_lr_prepare_bytes(int32_t in_features, int32_t out_features);
int bnn_lr_prepare(const float* w_mu, const float* w_rho, const float* b_mu, const float* b_rho,
                   int32_t in_features, int32_t out_features, void* w_frag, size_t w_frag_bytes,
                   void* kl_workspace, size_t kl_workspace_bytes, void* stream);
/* The same for BNN_MATH_BF16X3: the fragments additionally carry the low part bf16(M - bf16(M)) of the mean operand
 * ([mean hi | variance | mean lo] per feature tile and k-step: 1.5 x the bytes). */
size_t bnn_lr_prepare_x3_bytes(int32_t in_features, int32_t out_features);
/* (ABI 7) The prepared operands of several layers in ONE launch: an evaluation's prepare launches depend on no activation, and
 * one launch per layer put ~4 us of launch boundary per layer ahead of the first layer's kernel.  Bitwise the fragments and KL
 * entries of n_jobs bnn_lr_prepare (x3 != 0: bnn_lr_prepare_x3) calls; n_jobs <= 8. */
typedef struct {
  const float* w_mu;
  const float* w_rho;
  const float* b_mu;
  const float* b_rho;
  int32_t in_features, out_features;
  void* w_frag;
  size_t w_frag_bytes;
  void* kl_workspace;        /* optional, as in bnn_lr_prepare */
  size_t kl_workspace_bytes;
} bnn_lr_prepare_job;
int bnn_lr_prepare_many(const bnn_lr_prepare_job* jobs, int32_t n_jobs, int32_t x3, void* stream);
int bnn_lr_prepare_x3(const float* w_mu, const float* w_rho, const float* b_mu, const float* b_rho,
                      int32_t in_features, int32_t out_features, void* w_frag, size_t w_frag_bytes,
                      void* kl_workspace, size_t kl_workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * K2  bnn_gauss_kl — one streaming pass over (mu, rho)[n]: the eps-independent sums of
 * log q (networks.py:46, the -log sigma term) and the closed-form KL against
 * Normal(0, sigma_p) (networks.py:113).  out = float[4]:
 *   [0] KL = 0.5*sum(2 log(sigma_p/sigma) - 1 + (sigma/sigma_p)^2 + (mu/sigma_p)^2)
 *   [1] sum log sigma   [2] sum sigma^2   [3] sum mu^2
 * 8 algorithmic bytes per element; wavefront-shuffle + LDS block reduction, one partial
 * per block, fp64 final sum by a second one-block kernel (no float atomics: bitwise
 * reproducible).
 * ---------------------------------------------------------------------------------- */
size_t bnn_gauss_kl_workspace_bytes(int64_t n);
int bnn_gauss_kl(const float* mu, const float* rho, int64_t n, float sigma_p, void* workspace,
                 size_t workspace_bytes, float* out4, void* stream);

/* ------------------------------------------------------------------------------------
 * K4  bnn_elbo_finalize — per-sample scalars of one ELBO evaluation in one launch:
 * sums the stats partials of up to 8 BBB layers into log p / log q
 * (networks.py:174-178), or the KL partials of LR layers (networks.py:180-181), and the
 * NLL of the logits (networks.py:183-190: CrossEntropyLoss(reduction='sum') or the
 * Gaussian NLL with scale nll_sigma).  Outputs float[n_samples] each; any may be NULL.
 * For LR layers kl[] receives the same (eps-independent) value for every sample.
 * target: int64[batch] (classification) or float[batch,classes] (regression).
 * sample_counter: the launch functions bake their arguments into a captured hipGraph; the
 * Philox sample index therefore has a device-resident part that the layer kernels read and
 * this kernel (the last of an evaluation, stream-ordered after them) advances.
 * ---------------------------------------------------------------------------------- */
/* The tail of a training step's forward, optional in bnn_finalize_args: what bnn_elbo_loss_nll_bwd computes (loss
 * assembly networks.py:205-208, the backward seeds, d nll / d logits), done by the launch that finalizes when that
 * launch is bnn_bbb_final_fwd's row-split form (each row block differentiates its own rows' NLL, the last block to
 * arrive assembles the loss), else by a follow-up launch.  Arguments as for bnn_elbo_loss_nll_bwd. */
typedef struct bnn_loss_args {
  const float* beta;                /* device scalar */
  float total_samples;
  float grad_scale;
  float* out4;
  float* g_a;                       /* [n_samples]: d loss / d log p[s] (zeros for LR) */
  float* g_b;                       /* [n_samples]: d loss / d log q[s] */
  float* g_kl3;                     /* float[3] or NULL */
  float* g_logits;                  /* [n_samples,batch,classes] */
} bnn_loss_args;

typedef struct bnn_finalize_args {
  uint32_t struct_bytes;
  int32_t n_layers;                 /* 0..8 */
  int32_t local_reparam;            /* 0: BBB stats workspaces, 1: LR KL workspaces */
  int32_t n_samples, batch, classes;
  const void* layer_workspace[8];
  int32_t layer_in[8];
  int32_t layer_out[8];
  bnn_prior prior;
  const float* logits;              /* [n_samples,batch,classes] fp32, or NULL */
  const void* target;
  int32_t nll_mode;                 /* bnn_nll_mode */
  float nll_sigma;
  float* log_prior;                 /* BBB */
  float* log_q;                     /* BBB */
  float* kl;                        /* LR  */
  float* nll;
  uint32_t* sample_counter;         /* optional device word: += sample_counter_inc when done */
  uint32_t sample_counter_inc;      /* normally the GLOBAL number of MC samples of the evaluation */
  uint32_t reserved;
  float* sums;                      /* optional float[4] (float[G][4] with group_samples): sums over the local samples
                                       (of each minibatch) of {log p | KL, log q | 0, nll, sample count}: the vector
                                       a sharded job all-reduces (fixed summation order) */
  uint32_t* ticket;                 /* optional zero-initialised device word (left at zero again): lets 2..64 samples be
                                       finalized by one block each IN ONE launch, the last arriver folding `sums`
                                       (bnn_elbo_finalize and the fused last-layer form bnn_bbb_final_fwd) */
  void* scratch;                    /* optional, bnn_bbb_final_scratch_bytes(n_samples) bytes, 16-byte
                                       aligned, ZEROED ONCE by the caller: lets the fused last layer
                                       split its K range over several blocks per sample */
  size_t scratch_bytes;
  int32_t group_samples;            /* 0: the n_samples are one evaluation.  g > 0: n_samples = G * g, G independent
                                       minibatches of g MC samples each (see bnn_bbb_fwd_args): `sums` is then
                                       float[G][4], one 4-vector per minibatch */
  int32_t target_per_group;         /* with group_samples: 0 = one target for all, 1 = target[G][batch(,classes)] */
  const bnn_loss_args* loss;        /* optional (host pointer, read during the call): see bnn_loss_args.  Honoured by
                                       bnn_bbb_final_fwd; one evaluation only (group_samples == 0) */
} bnn_finalize_args;

int bnn_elbo_finalize(const bnn_finalize_args* args, void* stream);

/* bnn_lr_final_fwd — the LAST BayesianLinearLR layer of an evaluation together with its finalize
 * (networks.py:116-138 + :179-190): the same results as bnn_lr_linear_fwd(layer) followed by bnn_elbo_finalize(fin)
 * with fin->logits == layer->y, in ONE launch when the layer is narrow (<= 16 outputs, batch <= 128, bf16 math and x, on-chip
 * eps; <= 16 samples -- or, over prepared operands (layer->w_frag from bnn_lr_prepare[_many] / a rider), up to 4096 (minibatch,
 * sample) pairs, a block then taking two 16-row tiles and, beyond 64 pairs, the sums of the per-sample scalars made by a one-block
 * follow-up launch; fin->scratch as for bnn_bbb_final_fwd and, from 2 to 64 samples, fin->ticket): row blocks
 * compute the logits and the rows' NLL, one more block per sample the KL of all layers (this layer's from its
 * parameters: fin->layer_workspace[n_layers-1] is not read), the last block to arrive folds them.  Otherwise the two
 * launches. */
struct bnn_finalize_args;
int bnn_lr_final_fwd(const bnn_lr_fwd_args* layer, const struct bnn_finalize_args* fin, void* stream);

/* bnn_bbb_final_fwd — the LAST BBB layer of an evaluation together with its finalize: the
 * same results as bnn_bbb_linear_fwd(layer) followed by bnn_elbo_finalize(fin) with
 * fin->logits == layer->y and fin->layer_workspace[n_layers-1] == layer->workspace, but in ONE
 * launch when the layer is a single feature tile (out_features <= 16, batch <= 128): the block
 * that produced a sample's logits also forms its NLL (networks.py:183-190) and log p / log q
 * (networks.py:174-178).  Falls back to the two launches otherwise.
 * With layer->w_sampled / b_sampled (the layer's weights drawn earlier by bnn_bbb_sample_weights, its statistics in
 * fin->layer_workspace[n_layers-1]; bf16 math, <= 4096 samples (beyond 64 the sums come from a one-block follow-up launch),
 * fin->scratch given): the row-split form -- every
 * 16-row batch block of a sample is a block of its own (plain bf16 matmul + the rows' NLL), one more block sums the
 * layers' statistics, and the last block of the sample to finish folds the handful of scalars (write-through
 * stores + one arrival counter: no block waits, no fence). */
size_t bnn_bbb_final_scratch_bytes(int32_t n_samples);
int bnn_bbb_final_fwd(const bnn_bbb_fwd_args* layer, const bnn_finalize_args* fin, void* stream);

/* ------------------------------------------------------------------------------------
 * bnn_bbb_linear_bwd — backward of BayesianLinear for n_samples MC samples (what autograd
 * derives from networks.py:73-88 under classification/class_task.py:78 `loss.backward()`;
 * closed forms in SURVEY Appendix A.5).  eps is REGENERATED from the Philox map (or re-read
 * in BNN_EPS_MEMORY mode): no eps- or weight-sized tensor is kept from the forward pass.
 *   gz = gy * (y > 0) if relu;  gW_s = gz_s^T x_s;  t_s = gW_s + g_log_prior[s] * dlogp/dw(w_s)
 *   g_w_mu = sum_s t_s;  g_w_rho = (sum_s t_s eps_s - (sum_s g_log_q[s]) / sigma) * sigmoid(rho)
 *   (bias likewise with column sums of gz);  g_x[s] = gz_s . w_s  (optional).
 * All tensors fp32.  x [x_samples,batch,in]; gy, y [n_samples,batch,out]; g_x
 * [n_samples,batch,in].  workspace: bnn_bbb_linear_bwd_workspace_bytes (holds gz).
 * Weight gradients use the exact-fp32 matrix core; `math` selects the arithmetic of g_x only.
 * ---------------------------------------------------------------------------------- */
typedef struct bnn_bbb_bwd_args {
  uint32_t struct_bytes;
  int32_t n_samples, batch, in_features, out_features;
  const float* x;
  int32_t x_per_sample;
  int32_t relu;
  const float* gy;
  const float* y;             /* forward output (after ReLU); required when relu != 0 */
  const float* w_mu;
  const float* w_rho;
  const float* b_mu;
  const float* b_rho;
  int32_t eps_mode;
  int32_t math;
  const float* eps_w;
  const float* eps_b;
  uint64_t seed;
  uint32_t layer_id;
  uint32_t sample_offset;
  bnn_prior prior;
  int32_t gx_relu_mask;       /* != 0: g_x is multiplied by (x > 0).  x is then the output of the ReLU layer below,
                                 whose own backward takes this g_x as gy with relu = 0 (no separate mask pass) */
  const float* g_log_prior;   /* [n_samples] or NULL (zeros) */
  const float* g_log_q;       /* [n_samples] or NULL (zeros) */
  float* g_w_mu;
  float* g_w_rho;
  float* g_b_mu;
  float* g_b_rho;
  float* g_x;                 /* optional */
  void* workspace;
  size_t workspace_bytes;
  const uint32_t* sample_counter; /* optional device word added to sample_offset at run time (the value
                                     the forward of the same step read), as in bnn_bbb_fwd_args */
  const void* w_sampled;      /* optional bf16 [n_samples,out,in]: the weights the forward of this step sampled
                                 (bnn_bbb_sample_weights).  g_x = gz . w_sampled is then a plain matmul instead of
                                 regenerating w through the transposed generator (bf16 math only); the weight
                                 gradients still regenerate eps */
  const void* w_sampled_t;    /* optional bf16 [n_samples,in,out] (the forward's w_sampled_t_out), with g_x: the input
                                 gradient is then the forward's matmul-only launch over it (bf16 math) */
  const void* gy_bf16;        /* optional bf16 copy of gy (the layer above's g_x_bf16): read by that launch when relu == 0 */
  void* g_x_bf16;             /* optional bf16 [n_samples,batch,in]: g_x also in bf16, for the layer below's gy_bf16 */
} bnn_bbb_bwd_args;

size_t bnn_bbb_linear_bwd_workspace_bytes(int32_t n_samples, int32_t batch, int32_t out_features);
int bnn_bbb_linear_bwd(const bnn_bbb_bwd_args* args, void* stream);

/* ------------------------------------------------------------------------------------
 * bnn_lr_linear_bwd — backward of BayesianLinearLR for n_samples MC samples (what autograd
 * derives from networks.py:116-138 under class_task.py:78 `loss.backward()`; closed forms in
 * SURVEY Appendix A.5).  eps_act / eps_b are REGENERATED from the Philox map.
 *   gz = gy * (y > 0) if relu;   h = gz * eps_act / (2 sqrt(v))
 *   g_w_mu  = sum_s x_s^T gz_s + c_w M / sigma_p^2
 *   g_w_rho = (2 sigma sum_s (x_s^2)^T h_s + c_w (sigma / sigma_p^2 - 1 / sigma)) * sigmoid(rho)
 *   g_b_mu  = sum_s colsum(gz_s) + c_b b_mu / sigma_p^2;   g_b_rho likewise with eps_b
 *   g_x[s]  = gz_s M^T + 2 x_s * (h_s (sigma^2)^T)          (optional)
 * with c_w = g_kl[0] + g_kl[1], c_b = g_kl[0] + g_kl[2]: the upstream gradients of the layer's
 * kl_out triple {kl, weight_kl, bias_kl} (device float[3]; NULL = zeros).
 * All tensors fp32.  x [x_samples,batch,in]; gy, y, v [n_samples,batch,out] (v = the v_out of
 * the forward call); weights [in,out]; g_x [n_samples,batch,in].  Exact-fp32 matrix core.
 * ---------------------------------------------------------------------------------- */
typedef struct bnn_lr_bwd_args {
  uint32_t struct_bytes;
  int32_t n_samples, batch, in_features, out_features;
  const float* x;
  int32_t x_per_sample;
  int32_t relu;
  const float* gy;
  const float* y;             /* forward output (after ReLU); required when relu != 0 */
  const float* v;             /* pre-activation variance saved by bnn_lr_linear_fwd (v_out) */
  const float* w_mu;
  const float* w_rho;
  const float* b_mu;
  const float* b_rho;
  int32_t eps_mode;
  int32_t math;               /* bnn_math.  BNN_MATH_BF16: the input gradient's two products take bf16-rounded operands
                                 (fp32 accumulation), as the forward of that mode does (out_features % 8 == 0); the
                                 weight gradients stay on the exact-fp32 matrix core.  A narrow output layer
                                 (<= 16 outputs, batch <= 128, on-chip eps, g_x wanted) is one launch of plain fp32
                                 FMAs in either mode */
  const float* eps_act;       /* BNN_EPS_MEMORY */
  const float* eps_b;
  uint64_t seed;
  uint32_t layer_id;
  uint32_t sample_offset;
  float sigma_p;
  int32_t gx_relu_mask;       /* as in bnn_bbb_bwd_args */
  const float* g_kl;          /* device float[3] or NULL */
  float* g_w_mu;
  float* g_w_rho;
  float* g_b_mu;
  float* g_b_rho;
  float* g_x;                 /* optional */
  void* workspace;
  size_t workspace_bytes;
  const uint32_t* sample_counter; /* optional device word, as in bnn_bbb_bwd_args */
  const float* hfac;              /* optional, instead of v (which may then be NULL), with relu == 0: the forward's
                                     hfac_out.  gz = gy and h = gy * hfac are formed as the kernels load them: no
                                     preparation launch, eps_act is not regenerated, the workspace is not used */
} bnn_lr_bwd_args;

size_t bnn_lr_linear_bwd_workspace_bytes(int32_t n_samples, int32_t batch, int32_t in_features,
                                         int32_t out_features, int32_t want_gx);
int bnn_lr_linear_bwd(const bnn_lr_bwd_args* args, void* stream);

/* ------------------------------------------------------------------------------------
 * F2  bnn_adam_step — torch.optim.Adam.step() (the optimiser the reference's trainers build,
 * classification/class_task.py:60, :79; regression/reg_task.py:53) over up to
 * BNN_ADAM_MAX_TENSORS parameter tensors in ONE launch:
 *     g = grad + weight_decay * p;  m += (g - m)(1 - beta1);  v = beta2 v + (1 - beta2) g^2
 *     p -= lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
 * t = step (host) or, when step_device != NULL, the device word *step_device, advanced first if
 * step_advance != 0 (so a captured hipGraph of the training step counts by itself).  lr_device (optional device float)
 * overrides lr, so StepLR (class_task.py:61) can change the rate of a captured graph.
 * All tensors fp32 (grad: fp32 or bf16, grad_dtype), contiguous, 16-byte aligned.
 * ---------------------------------------------------------------------------------- */
#define BNN_ADAM_MAX_TENSORS 16
typedef struct bnn_adam_args {
  uint32_t struct_bytes;
  int32_t n_tensors;
  float* param[BNN_ADAM_MAX_TENSORS];
  const float* grad[BNN_ADAM_MAX_TENSORS];
  float* exp_avg[BNN_ADAM_MAX_TENSORS];
  float* exp_avg_sq[BNN_ADAM_MAX_TENSORS];
  int64_t numel[BNN_ADAM_MAX_TENSORS];
  double lr, beta1, beta2, eps, weight_decay;   /* doubles, as torch holds them: 1 - beta2 must not be
                                                   formed from a float-rounded beta2 */
  uint32_t step;                 /* 1-based step number when step_device == NULL */
  uint32_t bump_by;              /* see bump_counter */
  const float* lr_device;
  uint32_t* step_device;
  int32_t step_advance;          /* with step_device: 1 = ++(*step_device) before the update, 0 = use it
                                    as it is (second and later launches of one optimiser step) */
  int32_t grad_dtype;            /* bnn_dtype of grad[]: BNN_F32, or BNN_BF16 -- grad[t] then points at bf16 values (the
                                    gradient bucket a data-parallel step all-reduces in 2-byte elements) */
  uint32_t* ticket;              /* optional zero-initialised device array of 16 words.  With step_advance: the update uses
                                    *step_device + 1 and the block that finishes last stores it (and re-zeroes the
                                    ticket) -- the step counts inside the one launch, no separate tick launch */
  uint32_t* bump_counter;        /* optional (needs ticket): *bump_counter += bump_by by that same last block, e.g. the
                                    MC-sample counter of a captured training step, advanced after the backward read it */
} bnn_adam_args;

int bnn_adam_step(const bnn_adam_args* args, void* stream);

/* bnn_elbo_loss — the ELBO of networks.py:205-208 (BBB: a = log p, b = log q per sample) or
 * :222-224 (LR: a = KL per sample, b = NULL) from per-sample scalars and a DEVICE beta, with
 * total_samples = S of the whole job:  out4 = {loss, mean a, mean b, mean nll}, and the seeds of the
 * backward chain g_a[s] = -beta/S (0 for LR), g_b[s] = beta/S, g_nll[s] = 1/S, g_kl3 = {beta, 0, 0}
 * (what bnn_*_linear_bwd / bnn_nll_bwd take), all times grad_scale (1, or 1 / ranks when the
 * gradients of data-parallel minibatches are then SUM-all-reduced).  Any seed pointer may be NULL. */
int bnn_elbo_loss(const float* a, const float* b, const float* nll, const float* beta, int32_t n_samples,
                  float total_samples, float grad_scale, int32_t local_reparam, float* out4, float* g_a, float* g_b,
                  float* g_nll, float* g_kl3, void* stream);

/* bnn_nll_bwd — gradient of the summed NLL (networks.py:183-190) w.r.t. the logits of every MC
 * sample, scaled by g_nll[s] (device float[n_samples]):
 *   classification: (softmax(logits_s) - onehot(target)) * g_nll[s]
 *   regression:     (logits_s - target) / nll_sigma^2 * g_nll[s]
 * logits, g_logits fp32 [n_samples,batch,classes]; target as for bnn_elbo_finalize. */
int bnn_nll_bwd(const float* logits, const void* target, const float* g_nll, float* g_logits, int32_t n_samples,
                int32_t batch, int32_t classes, int32_t nll_mode, float nll_sigma, void* stream);

/* bnn_elbo_loss_nll_bwd — bnn_elbo_loss and bnn_nll_bwd of one training step in ONE launch: the NLL seed is the
 * constant grad_scale / total_samples, so the logits' gradient does not wait for the loss arithmetic.
 * Arguments as for the two functions (no g_nll: it is not materialised). */
int bnn_elbo_loss_nll_bwd(const float* a, const float* b, const float* nll, const float* beta, int32_t n_samples,
                          float total_samples, float grad_scale, int32_t local_reparam, float* out4, float* g_a, float* g_b,
                          float* g_kl3, const float* logits, const void* target, float* g_logits, int32_t batch,
                          int32_t classes, int32_t nll_mode, float nll_sigma, void* stream);

/* bnn_stage_inputs — the per-step inputs of a captured training step (the minibatch the reference's loop hands
 * to sample_elbo, class_task.py:72-77, and its KL weight beta) copied into the graph's static device buffers
 * in one launch: dst0 <- src0 (bytes0), dst1 <- src1 (bytes1), *word = value.  Device pointers; any part may be
 * empty (bytes = 0 / word = NULL). */
int bnn_stage_inputs(const void* src0, void* dst0, size_t bytes0, const void* src1, void* dst1, size_t bytes1,
                     float* word, float value, void* stream);
/* The same with src0 an fp32 tensor whose bf16 copy (bytes0 / 2 bytes) is also written to cast0_bf16: the first layer's
 * forward of a bf16-math step reads that one.  16-byte aligned pointers and sizes. */
int bnn_stage_inputs_cast(const void* src0, void* dst0, size_t bytes0, const void* src1, void* dst1, size_t bytes1,
                          float* word, float value, void* cast0_bf16, void* stream);

/* ------------------------------------------------------------------------------------
 * F3  bnn_mc_softmax_mean — the MC-averaged prediction of classification/class_task.py:81-87:
 *     probs[b, :] = scale * sum_s softmax(logits[s, b, :]),   preds[b] = argmax_c probs[b, c]
 * (scale = 1 / test_samples; a rank of a sharded job passes its local samples and the global
 * scale, then sum-all-reduces probs).  logits fp32 [n_samples,batch,classes]; probs fp32
 * [batch,classes]; preds int64[batch] or NULL.
 * ---------------------------------------------------------------------------------- */
int bnn_mc_softmax_mean(const float* logits, int32_t n_samples, int32_t batch, int32_t classes, float scale,
                        float* probs, long long* preds, void* stream);

/* ------------------------------------------------------------------------------------
 * F3  bnn_mc_predictive — the predictive summaries of S MC outputs (what a user of the network reads off the samples
 * the reference collects in regression/reg_task.py:76-83 and classification/class_task.py:81-87).
 * logits fp32 [groups, n_samples, batch, classes], g-major: G minibatches of S local samples each, the layout of a
 * stacked evaluation's output.  Every output is per (g, b) [groups, batch] or per (g, b, c) [groups, batch, classes].
 *   BNN_NLL_CLASSIFICATION, p_s = softmax(z_s):
 *     probs              = scale * sum_s p_s                          (required; scale = 1 / n_samples for the mean)
 *     expected_entropy   = scale * sum_s H(p_s), H = logsumexp(z) - sum_c p_c z_c       (required: the aleatoric part)
 *     preds              int64 argmax_c probs, lowest index on ties    (optional)
 *     predictive_entropy = -sum_c probs_c log probs_c, 0 log 0 = 0     (optional)
 *     mutual_information = max(predictive_entropy - expected_entropy, 0)   (optional: the epistemic part, BALD.  It is
 *                          >= 0 in exact arithmetic; the clamp removes the rounding-level negatives)
 *     A rank of a sample-sharded job passes its local samples and scale = 1 / (global samples), sum-all-reduces probs
 *     and expected_entropy, and forms the optional outputs from the sums.
 *   BNN_NLL_REGRESSION, over the S samples of each (g, b, c):
 *     mean, variance (ddof 0; two passes in fp64)                      (required)
 *     predictive_variance = variance + sigma^2                         (optional; sigma: the NLL's noise scale)
 *     quantiles [n_quantiles, groups, batch, classes] at the levels quantile[] in [0, 1] (n_quantiles 0 .. 8;
 *       n_samples <= BNN_PREDICTIVE_MAX_QUANTILE_SAMPLES): numpy.percentile(y, 100 q, axis=0) with its linear
 *       interpolation -- sort, pos = q (S - 1), v[floor pos] + frac (v[floor pos + 1] - v[floor pos]) -- and NaN for a
 *       column with a NaN sample.
 * Output buffers must not overlap logits.  One launch (two with quantiles).
 * ---------------------------------------------------------------------------------- */
#define BNN_PREDICTIVE_MAX_QUANTILES 8
#define BNN_PREDICTIVE_MAX_QUANTILE_SAMPLES 1024   /* a column's samples are sorted in LDS */
typedef struct bnn_mc_predictive_args {
  uint32_t struct_bytes;
  int32_t mode;                   /* bnn_nll_mode */
  int32_t groups, n_samples, batch, classes;
  const float* logits;
  float scale;                    /* classification */
  float sigma;                    /* regression, with predictive_variance */
  float* probs;
  int64_t* preds;
  float* predictive_entropy;
  float* expected_entropy;
  float* mutual_information;
  float* mean;
  float* variance;
  float* predictive_variance;
  int32_t n_quantiles;
  int32_t reserved;
  double quantile[BNN_PREDICTIVE_MAX_QUANTILES];
  float* quantiles;
} bnn_mc_predictive_args;
int bnn_mc_predictive(const bnn_mc_predictive_args* args, void* stream);

/* ------------------------------------------------------------------------------------
 * F3  bnn_ece — ECELoss.forward of compute_ece.py:14-57 over the MC-averaged class probabilities the predict path
 * produces (classification/class_task.py:81-87 -> compute_ece.py:62-78): every one of the n x classes probabilities
 * is binned (np.digitize(p, bin_edges, right=True) - 1), a probability is "correct" when it is its row's argmax and
 * that argmax is the label; ece = sum_b |mean confidence_b - accuracy_b| * count_b / sum_b count_b.
 * probs fp32 [n, classes]; labels int64[n]; bin_edges: HOST float64 array of n_edges <= 65 increasing values
 * (np.arange(0, 1.1, bin_step) for the reference's bins);  out fp32 [1 + 3 * (n_edges - 1)] = {ece, then per bin
 * count, corrects, confidence sum}.  Bins without data contribute nothing (the reference's loop breaks there).
 * Integer counts by LDS atomics, fp64 confidence sums in a fixed order: bitwise reproducible.
 * ---------------------------------------------------------------------------------- */
size_t bnn_ece_workspace_bytes(void);
int bnn_ece(const float* probs, const long long* labels, int64_t n, int32_t classes, const double* bin_edges,
            int32_t n_edges, void* workspace, size_t workspace_bytes, float* out, void* stream);

/* ------------------------------------------------------------------------------------
 * F4  signal-to-noise pruning of weight_pruning.py:85-115 over n contiguous fp32 (mu, rho) pairs:
 *   bnn_snr_db     out[i] = 10 log10(|mu[i]| / log1p(exp(rho[i])))           (:85-87 compute_snr, :100, :109)
 *   bnn_snr_prune  in place mu[i] *= m, rho[i] *= m with m = (snr_db > threshold)   (:101-105, :110-114);
 *                  a pruned weight is left at rho = 0 (sigma = log 2), as the reference leaves it.
 *                  kept (optional device uint64, caller-zeroed): += number of survivors.
 * The threshold is the caller's np.percentile(snrs, 100 * drop_percentage) (:92).
 * ---------------------------------------------------------------------------------- */
int bnn_snr_db(const float* mu, const float* rho, int64_t n, float* out, void* stream);
int bnn_snr_prune(float* mu, float* rho, int64_t n, float threshold, unsigned long long* kept, void* stream);

/* ------------------------------------------------------------------------------------
 * F5  contextual bandit — the device half of Bandit.update (reinforcement_learning/base_bandit.py:37-99): decide, reward,
 * regret, replay buffer, shuffle and minibatch gather, with nothing read back by the host.  Per bandit step t:
 *   bnn_bandit_rows    i_t = indices[t] when indices != NULL, t < n_indices and indices[t] >= 0, else drawn
 *                      (min(floor(u(r3) N), N - 1)); writes *cur_index = i_t and the A decision rows
 *                      rows[a] = x[i_t] ++ one_hot(a)  ([A, d + A] fp32: action a's encoding, base_bandit.py:39-40)
 *   (the caller's forward of the rows: outputs[S, A])
 *   bnn_bandit_act     v_a = o_0(a) + o_1(a) + ... + o_{S-1}(a), left to right in fp32 (Python's sum, :45-46), with
 *                      o_s = outputs + s * output_sample_stride (stride 0: the one deterministic forward, S times);
 *                      action = argmax_a v_a, ties to the HIGHEST index (the reference eats only when eat > reject);
 *                      u(r0) < epsilon: action = min(floor(u(r1) A), A - 1) (:48-50);
 *                      with k = labels[i_t] and (hi, lo, thr) = rewards[k][action]: reward = u(r2) > thr ? hi : lo;
 *                      regrets[t + 1] = regrets[t] + (oracle[k] - reward) in fp64 (regrets[0] = 0 is the caller's);
 *                      counts[k][action] += 1; ring slot t mod buffer_size <- (i_t, action, reward); *step = t + 1;
 *                      *sample_counter += sample_counter_inc (the MC-sample indices a sampled decision used).
 *   bandit random stream: (r0, r1, r2, r3) = Philox4x32-R((0, t, 0, 1), key = (seed_lo, seed_hi)), u() as for eps: word 3
 *   is 1, every eps counter's is 0.  t = *step, read on the device; a step at or past max_steps writes nothing.
 * Both launches take the same argument block; one block each. */
#define BNN_BANDIT_MAX_ACTIONS 64
#define BNN_BANDIT_MAX_BUFFER 8192     /* the replay permutation sorts (key, position) pairs in 64 KiB of LDS */
typedef struct bnn_bandit_act_args {
  uint32_t struct_bytes;
  int32_t n_actions;              /* A, 2 .. BNN_BANDIT_MAX_ACTIONS */
  int32_t n_labels;               /* K >= 1 */
  int32_t n_samples;              /* S >= 1 */
  int32_t output_sample_stride;   /* A (one output row per draw) or 0 */
  int32_t context_dim;            /* d */
  int64_t n_contexts;             /* N */
  int32_t buffer_size;            /* ring entries, 1 .. BNN_BANDIT_MAX_BUFFER */
  uint32_t sample_counter_inc;
  int64_t max_steps;              /* entries of actions / reward_out, max_steps + 1 of regrets */
  int64_t n_indices;
  float epsilon;
  uint32_t reserved;
  uint64_t seed;
  const float* x;                 /* [N, d] */
  const int64_t* labels;          /* [N], values in [0, K) */
  const float* rewards;           /* [K, A, 3]: (hi, lo, thr) */
  const float* oracle;            /* [K] */
  const int64_t* indices;         /* optional [n_indices] */
  const float* outputs;           /* act: [S, A] (stride A) or [A] (stride 0) */
  uint32_t* step;                 /* device word t */
  int32_t* cur_index;             /* device word i_t */
  float* rows;                    /* rows: [A, d + A] */
  int64_t* actions;               /* act: [max_steps] */
  float* reward_out;              /* act: [max_steps] */
  double* regrets;                /* act: [max_steps + 1] */
  int64_t* counts;                /* act: [K, A] */
  int32_t* ring_index;            /* act: [buffer_size] */
  int32_t* ring_action;           /* act: [buffer_size] */
  float* ring_reward;             /* act: [buffer_size] */
  uint32_t* sample_counter;       /* optional */
} bnn_bandit_act_args;
int bnn_bandit_rows(const bnn_bandit_act_args* args, void* stream);
int bnn_bandit_act(const bnn_bandit_act_args* args, void* stream);

/* bnn_bandit_replay — the replay pool of base_bandit.py:77-84 after step t's append (l = t + 1 = *step entries):
 *   l <= bs:               pool position p in [0, bs) holds entry (m l - bs + p) mod l, m = bs / l + 1
 *   bs < l < buffer_size:  the last floor(l / bs) bs entries;  otherwise the last buffer_size entries
 * shuffled by sorting the positions by (key, p), key of p = word (p & 3) of Philox4x32-R((p >> 2, t, 1, 1), seed), and
 * gathered into minibatches: row q of the shuffled pool is x[i] ++ one_hot(action) of its entry, its target the reward.
 *   slab [num_batches, bs, d + A], targets [num_batches, bs]; *n_batches = pool / bs (optional).  Rows past the pool
 *   are left as they were.  workspace: int32 [buffer_size] (the shuffled ring slots).
 * buffer_size % batch_size == 0 (else the reference's last minibatch is short), buffer_size <= BNN_BANDIT_MAX_BUFFER,
 * num_batches * batch_size >= buffer_size.  Two launches: the sort (one block), the gather. */
typedef struct bnn_bandit_replay_args {
  uint32_t struct_bytes;
  int32_t batch_size;
  int32_t num_batches;            /* slab capacity */
  int32_t buffer_size;
  int32_t context_dim;            /* d */
  int32_t n_actions;              /* A */
  int64_t n_contexts;             /* N */
  uint64_t seed;
  const uint32_t* step;           /* device word l = t + 1 (what bnn_bandit_act left) */
  const float* x;                 /* [N, d] */
  const int32_t* ring_index;
  const int32_t* ring_action;
  const float* ring_reward;
  int32_t* workspace;             /* [buffer_size] */
  float* slab;
  float* targets;
  int32_t* n_batches;             /* optional device word */
} bnn_bandit_replay_args;
int bnn_bandit_replay(const bnn_bandit_replay_args* args, void* stream);

/* ------------------------------------------------------------------------------------
 * F6  groups of epsilon-greedy MLP bandits — Greedy_Bandit (reinforcement_learning/bandits.py:59-85: an MLP
 * in-(hidden)-(hidden)-1 trained by torch.optim.Adam on mse_loss(net(x).squeeze(), y, reduction='sum')) for G independent
 * agents, each update a fixed number of launches whatever G: rows, fwd, act, replay (2), train.
 *
 * Grouped F5 entries: bnn_bandit_rows_group / bnn_bandit_act_group run exactly bnn_bandit_rows / bnn_bandit_act on each of
 * n_agents bnn_bandit_act_args blocks (block g of the grid on block g), bnn_bandit_replay_group exactly bnn_bandit_replay on
 * n_agents bnn_bandit_replay_args blocks (sort: block g; gather: grid row g).  Per agent the semantics are F5's.
 * Validation without a device: the caller passes the blocks twice -- `blocks_host`, a HOST array the entry validates block
 * by block with F5's checks, and `blocks`, a DEVICE copy of the same bytes that the kernels read (the caller copies it once;
 * the launches read it on every replay, so a captured graph keeps working as long as the copy is left in place).
 * blocks_bytes must be n_agents * sizeof(block) (else BNN_ERR_SHAPE); the library does not compare the two copies.
 *
 * bnn_mlp_group_fwd — the decision forward: for each agent g, outputs[r] = net_g(rows[r]) for the n_rows rows
 *   [n_rows, in] (what bnn_bandit_rows wrote): Linear, ReLU, Linear, ReLU, Linear.  One launch, one workgroup per agent.
 * bnn_mlp_group_train — the training half of one update (base_bandit.py:86-88 with bandits.py:77-83) for every agent in
 *   ONE launch, one workgroup per agent: nb = min(*n_batches, max_batches) (the word bnn_bandit_replay writes); for
 *   j = 0 .. nb - 1 on slab[j] [batch, in] / targets[j] [batch]:
 *     forward; loss = sum_b (z_b - y_b)^2, dz_b = 2 (z_b - y_b); backward (weight, bias and hidden-input gradients);
 *     Adam (F2's arithmetic, torch.optim.Adam): t = *step + j + 1, lr = *lr (device words: a captured graph counts by
 *     itself, StepLR reaches it), bias corrections in fp64, then every parameter of the agent updated.
 *   *step += nb, and *loss = the loss of minibatch nb - 1 (the reference's loss_info).  nb == 0 writes nothing.
 *   The minibatches are separated by workgroup barriers only: agents never wait on each other.
 * Math: exact fp32 in every math mode (fp32 FMA; bnn_set_math / BNN_MATH_* do not apply: the shapes are per-CU latency-bound
 *   chains, where bf16 operands would buy little and cost the reference's arithmetic).  Every sum runs in one fixed order
 *   (no float atomics): a replay is bit-reproducible, and an agent's results do not depend on G or on its place in the group.
 * Limits: in <= BNN_MLP_GROUP_MAX_IN, hidden <= BNN_MLP_GROUP_MAX_HIDDEN, out == 1, batch and n_rows <=
 *   BNN_MLP_GROUP_MAX_BATCH (x, both hidden activations and one gradient live in LDS: 4 x 32 KiB of the CU's 160),
 *   max_batches <= BNN_MLP_GROUP_MAX_BATCHES, n_agents <= BNN_MLP_GROUP_MAX_AGENTS; else BNN_ERR_SHAPE.
 * Per-agent data lives in an array of bnn_mlp_group_agent blocks, passed host + device as above (agents_host validated,
 *   agents read by the kernel, agents_bytes = n_agents * sizeof(bnn_mlp_group_agent)).  Parameters in nn.Linear's layout
 *   (weight [out, in], bias [out]); param / exp_avg / exp_avg_sq in the order w1 b1 w2 b2 w3 b3.  fwd reads param, rows,
 *   outputs only; train everything but rows / outputs.
 * ---------------------------------------------------------------------------------- */
#define BNN_MLP_GROUP_MAX_IN 128
#define BNN_MLP_GROUP_MAX_HIDDEN 128
#define BNN_MLP_GROUP_MAX_OUT 1
#define BNN_MLP_GROUP_MAX_BATCH 64
#define BNN_MLP_GROUP_MAX_BATCHES 128
#define BNN_MLP_GROUP_MAX_AGENTS 4096
typedef struct bnn_bandit_group_args {
  uint32_t struct_bytes;
  int32_t n_agents;               /* G, 1 .. BNN_MLP_GROUP_MAX_AGENTS */
  const void* blocks_host;        /* HOST: G bnn_bandit_act_args blocks for rows / act, G bnn_bandit_replay_args for replay */
  const void* blocks;             /* DEVICE copy of blocks_host */
  int64_t blocks_bytes;           /* bytes of the device copy */
} bnn_bandit_group_args;
int bnn_bandit_rows_group(const bnn_bandit_group_args* args, void* stream);
int bnn_bandit_act_group(const bnn_bandit_group_args* args, void* stream);
int bnn_bandit_replay_group(const bnn_bandit_group_args* args, void* stream);

typedef struct bnn_mlp_group_agent {
  float* param[6];                /* w1 [hidden, in], b1 [hidden], w2 [hidden, hidden], b2 [hidden], w3 [1, hidden], b3 [1] */
  float* exp_avg[6];              /* train: Adam's moments, same shapes */
  float* exp_avg_sq[6];
  uint32_t* step;                 /* train: Adam's device step word */
  const float* lr;                /* train: device learning rate */
  const float* slab;              /* train: [max_batches, batch, in] */
  const float* targets;           /* train: [max_batches, batch] */
  const int32_t* n_batches;       /* train: device word nb */
  float* loss;                    /* train: device scalar */
  const float* rows;              /* fwd: [n_rows, in] */
  float* outputs;                 /* fwd: [n_rows] */
} bnn_mlp_group_agent;
typedef struct bnn_mlp_group_args {
  uint32_t struct_bytes;
  int32_t n_agents;               /* G, 1 .. BNN_MLP_GROUP_MAX_AGENTS */
  int32_t in_features, hidden, out_features;
  int32_t batch;                  /* train: minibatch rows */
  int32_t max_batches;            /* train: slab capacity */
  int32_t n_rows;                 /* fwd: rows per agent */
  double beta1, beta2, eps, weight_decay;
  const bnn_mlp_group_agent* agents_host;   /* HOST array of G blocks (validated) */
  const bnn_mlp_group_agent* agents;        /* DEVICE copy (read by the kernel) */
  int64_t agents_bytes;                     /* bytes of the device copy */
} bnn_mlp_group_args;
int bnn_mlp_group_fwd(const bnn_mlp_group_args* args, void* stream);
int bnn_mlp_group_train(const bnn_mlp_group_args* args, void* stream);

/* ------------------------------------------------------------------------------------
 * F7  groups of Thompson-sampling BNN bandits — BNN_Bandit (reinforcement_learning/bandits.py:17-54: a Bayes-by-Backprop
 * network in-(hidden)-(hidden)-1 of BayesianLinear layers, networks.py:48-88, trained by torch.optim.Adam on sample_elbo,
 * networks.py:192-209) for G independent agents, each update a fixed number of launches whatever G:
 *     bnn_bandit_rows_group -> bnn_bbb_group_fwd -> bnn_bandit_act_group -> bnn_bandit_replay_group (2) -> bnn_bbb_group_train
 * One workgroup per agent in both entries; agents never wait on each other (no grid-wide barrier, no polled counter).
 *
 * bnn_bbb_group_fwd — the decision forward.  For agent g and its n_rows rows [n_rows, in] (what bnn_bandit_rows wrote):
 *   eps_mode == BNN_EPS_PHILOX: outputs[s * n_rows + r] = net_g(rows[r]) under posterior draw s, s < n_samples: one weight
 *     draw w = mu + log1p(exp(rho)) * eps shared by all rows, eps from the map at the top with GLOBAL MC-sample index
 *     *sample_counter + s and the agent's own eps_seed as key.  The counter is read, not advanced (bnn_bandit_act does that
 *     through sample_counter_inc).
 *   eps_mode == BNN_EPS_ZERO: the one deterministic forward w = mu, outputs[r] (bnn_bandit_act reads it with stride 0);
 *     sample_counter is not read.
 * bnn_bbb_group_train — the training half of one update (base_bandit.py:86-88 with bandits.py:39-51) for every agent in
 *   ONE launch: nb = min(*n_batches, max_batches) (the word bnn_bandit_replay writes), c = *sample_counter; for
 *   j = 0 .. nb - 1 on slab[j] [batch, in] / targets[j] [batch]:
 *     for s < n_samples, GLOBAL MC-sample index c + j * n_samples + s: w = mu + log1p(exp(rho)) * eps for the weight
 *       (kind 0) and bias (kind 1) of layers 0, 1, 2; forward Linear-ReLU-Linear-ReLU-Linear;
 *       log_q = sum log N(w; mu, sigma), log_p = sum log prior(w) (BNN_PRIOR_GAUSS / BNN_PRIOR_MIXTURE, one prior for the
 *       launch); nll_s = -sum_b log N(y_b; z_b, 1), element by element;
 *     loss = beta[j] (mean_s log_q - mean_s log_p) + mean_s nll_s; beta[] is a host-made table in the argument block:
 *       bandits.py:44's value formed in fp64 and rounded once to fp32 (what train.GraphedTrainStep.step hands its device
 *       word), beta[j] for j < max_batches;
 *     the gradient of loss with respect to the twelve tensors, with the log_q terms in closed form as F1 has them
 *       (g_mu = sum_s t_s, g_rho = (sum_s t_s eps_s - beta / sigma) sigmoid(rho), t_s = (d nll_s / dw - beta d log_p / dw) / S);
 *     Adam (F2's arithmetic): t = *step + j + 1, lr = *lr (device words), bias corrections in fp64; the next minibatch
 *       reads the updated parameters.
 *   At the end *step += nb, *sample_counter += nb * n_samples and loss_info[0..3] = (loss, mean log_p, mean log_q,
 *   mean nll) of minibatch nb - 1 (sample_elbo's tuple: the reference's loss_info).  nb == 0 writes nothing.
 * Math: exact fp32 (fp32 FMA) in every math mode, as F6.  Every sum (GEMM elements: one fma chain, k ascending; log_q, log_p,
 *   nll, the bias gradients' column sums) runs in one fixed order, no float atomics: an agent's bits do not depend on G, on
 *   its place in the group or on graph replay against eager launches.
 * Workspace: per agent, bnn_bbb_group_workspace_bytes(in, hidden) bytes of global memory (16-byte aligned), shared by the
 *   two entries: the current draw's weights (layers 0 and 1 transposed, layer 1 also as stored), its eps, and the two
 *   gradient accumulators sum_s t_s, sum_s t_s eps_s.  Contents between launches are scratch.
 * Limits: F6's (in, hidden, out == 1, batch and n_rows, max_batches, n_agents) and 1 <= n_samples <=
 *   BNN_BBB_GROUP_MAX_SAMPLES; else BNN_ERR_SHAPE.  prior.kind outside bnn_prior_kind, or an agent's eps_mode other than
 *   BNN_EPS_PHILOX / BNN_EPS_ZERO: BNN_ERR_ENUM.  workspace NULL or workspace_bytes below the query: BNN_ERR_WORKSPACE.
 * Agent blocks are passed host + device as in F6.  param / exp_avg / exp_avg_sq in networks.BayesianNetwork.parameters()
 *   order: (weight_mu [out, in], weight_rho, bias_mu [out], bias_rho) of l1, l2, l3.  fwd reads param, rows, outputs,
 *   sample_counter (BNN_EPS_PHILOX), workspace, eps_seed, eps_mode; train everything but rows / outputs / eps_mode.
 * ---------------------------------------------------------------------------------- */
#define BNN_BBB_GROUP_MAX_SAMPLES 8
typedef struct bnn_bbb_group_agent {
  float* param[12];               /* (weight_mu, weight_rho, bias_mu, bias_rho) x (l1, l2, l3) */
  float* exp_avg[12];             /* train: Adam's moments, same shapes */
  float* exp_avg_sq[12];
  uint32_t* step;                 /* train: Adam's device step word */
  const float* lr;                /* train: device learning rate */
  const float* slab;              /* train: [max_batches, batch, in] */
  const float* targets;           /* train: [max_batches, batch] */
  const int32_t* n_batches;       /* train: device word nb */
  float* loss_info;               /* train: [4] (loss, mean log_p, mean log_q, mean nll) */
  const float* rows;              /* fwd: [n_rows, in] */
  float* outputs;                 /* fwd: [n_samples, n_rows] (BNN_EPS_PHILOX) or [n_rows] (BNN_EPS_ZERO) */
  uint32_t* sample_counter;       /* device word: next unused MC-sample index of this agent */
  float* workspace;               /* bnn_bbb_group_workspace_bytes(in, hidden) bytes */
  uint64_t eps_seed;              /* the agent's key of the epsilon map */
  int32_t eps_mode;               /* fwd: BNN_EPS_PHILOX (a draw per sample) or BNN_EPS_ZERO (w = mu) */
  int32_t reserved;
} bnn_bbb_group_agent;
typedef struct bnn_bbb_group_args {
  uint32_t struct_bytes;
  int32_t n_agents;               /* G, 1 .. BNN_MLP_GROUP_MAX_AGENTS */
  int32_t in_features, hidden, out_features;
  int32_t batch;                  /* train: minibatch rows */
  int32_t max_batches;            /* train: slab capacity */
  int32_t n_rows;                 /* fwd: rows per agent */
  int32_t n_samples;              /* S, 1 .. BNN_BBB_GROUP_MAX_SAMPLES */
  bnn_prior prior;                /* train */
  double beta1, beta2, eps, weight_decay;   /* train: Adam */
  float beta[BNN_MLP_GROUP_MAX_BATCHES];    /* train: KL weight of minibatch j */
  int64_t workspace_bytes;                  /* bytes behind every agent's workspace */
  const bnn_bbb_group_agent* agents_host;   /* HOST array of G blocks (validated) */
  const bnn_bbb_group_agent* agents;        /* DEVICE copy (read by the kernel) */
  int64_t agents_bytes;                     /* bytes of the device copy */
} bnn_bbb_group_args;
size_t bnn_bbb_group_workspace_bytes(int32_t in_features, int32_t hidden);   /* 0 outside the limits */
int bnn_bbb_group_fwd(const bnn_bbb_group_args* args, void* stream);
int bnn_bbb_group_train(const bnn_bbb_group_args* args, void* stream);

/* ------------------------------------------------------------------------------------
 * bnn_philox_normal — materialise the on-chip epsilon stream (map at the top) into
 * eps[n_samples, rows, cols]: used by the backward pass to regenerate eps instead of
 * storing it, and by tests to check the frozen counter->element map.
 * ---------------------------------------------------------------------------------- */
int bnn_philox_normal(float* eps, uint64_t seed, uint32_t tensor_id, uint32_t sample_offset,
                      int32_t n_samples, int32_t rows, int32_t cols, void* stream);

/* ------------------------------------------------------------------------------------
 * K5  MC dropout of MLP_Dropout (networks.py:253-285 kept in train mode at test time, main.py:42/:138,
 * regression/reg_task.py:186-195, classification/class_task.py:230-236): S stochastic passes of
 *     y[s] = drop_s(act(x[s'] . W^T + b))
 * for one nn.Linear (W fp32 [out,in], b fp32 [out], SHARED by all samples) in ONE launch.
 *   x_shared = 1: x [batch, in] for every sample (the first layer: the dropout acts after it): the block computes its
 *                 output tile once and writes the masked copies of a run of samples.
 *   x_shared = 0: x [n_samples, batch, in]: one GEMM of n_samples * batch rows against W; row r is sample r / batch.
 *   drop_p in [0, 1): the kind-3 mask of layer layer_id (map at the top) for global sample index
 *                 g = sample_offset + *sample_counter + s; drop_p = 0 applies none (keep all, scale 1: the same values).
 *   relu: ReLU before the dropout.  y [n_samples, batch, out] of y_dtype (bf16 between layers in bf16 math).
 * Math: BNN_MATH_BF16: x and W rounded to bf16 (RNE) while they are staged, fp32 accumulate (v_mfma_f32_16x16x32_bf16);
 * BNN_MATH_F32 and BNN_MATH_BF16X3: exact fp32 (v_mfma_f32_16x16x4_f32; x and y fp32).  An output element's reduction
 * runs K in 32-wide steps in one fixed order whatever n_samples, batch and the tile: results do not depend on how the
 * samples are split over calls.  Parameters are read on every call (no cached copies).  Any shape >= 1.
 * sample_counter_inc: added to *sample_counter by the launch (so a captured chain advances its own counter); only with
 * drop_p == 0, i.e. by a launch that does not read the counter (the output layer).
 * bnn_dense_plan returns what bnn_dense_fwd launches: form BNN_FORM_GEMM, batch_rows x features_per_block output tiles
 * (64 x 64, or 128 x 128 for bf16 math when they still give >= 512 blocks), k_slices = the sample runs of a shared-x
 * launch (1 otherwise), blocks, lds_bytes; a pure function of the shape, math, dtypes and alignment.
 * ---------------------------------------------------------------------------------- */
typedef struct bnn_dense_fwd_args {
  uint32_t struct_bytes;
  int32_t n_samples, batch, in_features, out_features;
  int32_t x_shared;         /* 1: x [batch,in] for all samples; 0: x [n_samples,batch,in] */
  const void* x;
  int32_t x_dtype;          /* bnn_dtype; BNN_BF16 only with BNN_MATH_BF16 */
  int32_t math;             /* bnn_math */
  const float* w;           /* [out,in] */
  const float* b;           /* [out], or NULL for no bias */
  int32_t relu;
  int32_t layer_id;         /* >= 0: the mask's tensor id is 4 * layer_id + 3 */
  double drop_p;            /* in [0, 1) */
  uint64_t seed;
  uint32_t sample_offset;
  uint32_t sample_counter_inc;
  uint32_t* sample_counter; /* optional DEVICE word, as in bnn_bbb_fwd_args */
  void* y;                  /* [n_samples,batch,out] */
  int32_t y_dtype;          /* bnn_dtype; BNN_BF16 only with BNN_MATH_BF16 */
  int32_t reserved;
} bnn_dense_fwd_args;
int bnn_dense_fwd(const bnn_dense_fwd_args* args, void* stream);
int bnn_dense_plan(const bnn_dense_fwd_args* args, bnn_plan* plan);

/* bnn_dropout_mask — the kind-3 stream of layer layer_id, materialised: mask[n_samples, rows, cols] = scale where
 * the element is kept and 0 where it is dropped, samples sample_offset .. sample_offset + n_samples - 1.  p in [0, 1)
 * (else BNN_ERR_SHAPE).  For tests; bnn_dense_fwd never reads it. */
int bnn_dropout_mask(float* mask, uint64_t seed, uint32_t layer_id, uint32_t sample_offset, int32_t n_samples,
                     int32_t rows, int32_t cols, double p, void* stream);

/* ------------------------------------------------------------------------------------
 * K6  Training MLP / MLP_Dropout (networks.py:227-285 under the reference's train_step: zero_grad, forward, loss,
 * backward, optimiser step; classification/class_task.py:150-157, regression/reg_task.py:176-183).  The forward is
 * bnn_dense_fwd with n_samples = 1 and fp32 outputs; these three finish the step.
 *
 * bnn_dense_loss — the loss value and the logits' gradient in ONE launch (one block; no float atomics):
 *   BNN_NLL_CLASSIFICATION: cross_entropy(z, y, reduction='sum'):  loss = sum_b (logsumexp z_b - z_b[y_b]),
 *                           g_logits = (softmax(z) - onehot(y)) * grad_scale.  target int64 [batch].  A label outside
 *                           [0, classes) makes the loss and its row's gradient NaN (never read out of bounds).
 *   BNN_NLL_REGRESSION:     mse_loss(z, y, reduction='sum'):  loss = sum (z - y)^2,  g_logits = 2 (z - y) * grad_scale.
 *                           target fp32 [batch, classes].
 * The loss is a per-thread sum over a fixed set of rows, then a fixed-order tree: the same bits on every call. */
typedef struct bnn_dense_loss_args {
  uint32_t struct_bytes;
  int32_t batch, classes;
  int32_t loss_mode;        /* bnn_nll_mode */
  const float* logits;      /* [batch, classes] */
  const void* target;       /* int64 [batch] (classification) or fp32 [batch, classes] (regression) */
  float grad_scale;
  int32_t reserved;
  float* loss;              /* device scalar (unscaled) */
  float* g_logits;          /* [batch, classes] */
} bnn_dense_loss_args;
int bnn_dense_loss(const bnn_dense_loss_args* args, void* stream);

/* bnn_dense_bwd — the backward of one Linear -> [ReLU] -> [Dropout] group in ONE launch:
 *   gz   = gy                                   (y == NULL: the output layer, or gy already masked by the layer above)
 *        = y > 0 ? gy * y_scale : 0             (y: this layer's saved output; with ReLU then Dropout, y > 0 exactly
 *                                                where the element was kept and the ReLU open; y_scale = 1 / (1 - p))
 *   g_w  = gz^T . x  [out, in],   g_b = colsum(gz)  [out]: always the exact-fp32 matrix core (v_mfma_f32_16x16x4_f32)
 *   g_x  = gz . W    [batch, in]  (optional; BNN_MATH_BF16: gz and W rounded to bf16 (RNE), fp32 accumulate; other
 *                                  modes exact fp32), times (x > 0 ? gx_scale : 0) when gx_mask: the gradient mask of the
 *                                  layer below (x is that layer's output), so its backward takes g_x as gy directly.
 * x fp32 [batch, in] (this layer's input), gy / y fp32 [batch, out], W fp32 [out, in].  No K-split: every output element
 * is one fixed chain of MFMAs over 32-wide k stages (g_b: four fixed strided partial sums, added in order), so results
 * do not depend on the grid.  Any shape >= 1; 4-byte aligned pointers. */
typedef struct bnn_dense_bwd_args {
  uint32_t struct_bytes;
  int32_t batch, in_features, out_features;
  int32_t math;             /* bnn_math of the g_x product */
  int32_t gx_mask;
  const float* x;
  const float* gy;
  const float* y;           /* optional */
  float y_scale;
  float gx_scale;
  const float* w;
  float* g_w;
  float* g_b;               /* optional */
  float* g_x;               /* optional */
} bnn_dense_bwd_args;
int bnn_dense_bwd(const bnn_dense_bwd_args* args, void* stream);

/* bnn_sgd_step — torch.optim.SGD.step() without momentum (the optimiser of classification/class_task.py:149) over up to
 * BNN_SGD_MAX_TENSORS fp32 tensors in ONE launch:  p -= lr * (g + weight_decay * p)  (two fmas in fp32).  lr_device
 * (optional device float) overrides lr, so StepLR can change the rate of a captured graph.  Contiguous tensors,
 * 16-byte aligned. */
#define BNN_SGD_MAX_TENSORS 16
typedef struct bnn_sgd_args {
  uint32_t struct_bytes;
  int32_t n_tensors;
  float* param[BNN_SGD_MAX_TENSORS];
  const float* grad[BNN_SGD_MAX_TENSORS];
  int64_t numel[BNN_SGD_MAX_TENSORS];
  double lr, weight_decay;
  const float* lr_device;
} bnn_sgd_args;
int bnn_sgd_step(const bnn_sgd_args* args, void* stream);

/* ------------------------------------------------------------------------------------
 * F8  device-resident training epochs — the data-loader half of the reference's epoch loop (classification/class_task.py:67-79,
 * regression/reg_task.py:60-74 over DataLoader(shuffle=True, drop_last=True)): the data set stays on the device, the epoch's
 * permutation is drawn there, and ONE launch per minibatch gathers its rows into a captured training step's static buffers.
 * The minibatch number j and the epoch number e are device words: the same argument blocks serve every launch.
 *
 * bnn_epoch_permutation   order[0 .. N-1] (int32) = the positions p sorted by (key_p, p), with
 *     key_p = word (p & 3) of Philox4x32-R((p >> 2, e, 2, 1), key = (seed_lo, seed_hi)), R = bnn_philox_rounds(), e = *epoch.
 *   Counter words 2 and 3 are (2, 1): every eps counter's word 3 is 0, and among the word-3 = 1 streams the bandit's coins use
 *   (.., 0, 1) and its replay permutation (.., 1, 1), so this stream shares a counter with none (F10's random scores: (.., 3, 1)).  The result is fixed by this
 *   definition, not by the algorithm (rank by counting over LDS-staged key tiles; one launch, N <= BNN_EPOCH_MAX_ROWS).
 *
 * bnn_epoch_stage   minibatch j = *batch_index of an epoch of M = num_batches minibatches of B = batch_size rows:
 *     i_r = order[j B + r] (order == NULL: j B + r, the unshuffled loader), r < B;
 *     x_out[r, :] = x[i_r, :] in fp32: an fp32 source is copied, a uint8 source converted as (float)u / 255.0f (IEEE division:
 *       torchvision's ToTensor);  x_bf16_out[r, :] (optional) = bf16 of that, round to nearest even, as bnn_stage_inputs_cast;
 *     targets_out[r] = targets[i_r]: int64 labels (target_dim == 0) or target_dim fp32 values per row;
 *     *beta = beta_table[j] when beta_table != NULL;
 *     loss_history[(j - 1) loss_cols + c] = *loss_src[c], c < loss_cols, when loss_history != NULL and j > 0: the loss words the
 *       training step of minibatch j - 1 left (the caller files row M - 1 after the last step);
 *     then *batch_index = j + 1, or at j + 1 == M: *batch_index = 0 and *epoch += 1.
 *   An order entry outside [0, N) reads row j B + r instead.  *ticket must be 0 before the first launch; the launch leaves it 0.
 *   *batch_index >= M: nothing is written.  Rows are gathered with 16-byte stores when row_dim % 4 == 0 and x, x_out,
 *   x_bf16_out are aligned to 16 / 16 / 8 bytes (uint8 x: 4), element by element otherwise: the same values either way.
 * Errors: N outside [1, BNN_EPOCH_MAX_ROWS], B M > N, a non-positive dimension, loss_cols outside [0, BNN_EPOCH_MAX_LOSS_COLS]
 * (0 with loss_history): BNN_ERR_SHAPE; x_dtype outside bnn_epoch_x_dtype: BNN_ERR_ENUM; x, targets, batch_index, epoch,
 * ticket, x_out, targets_out (stage) or epoch, order (permutation) NULL, beta NULL with beta_table, a NULL loss_src[c < loss_cols]
 * with loss_history: BNN_ERR_NULL.
 * ---------------------------------------------------------------------------------- */
#define BNN_EPOCH_MAX_ROWS 65536       /* rows of a data set (MNIST: 60 000) */
#define BNN_EPOCH_MAX_LOSS_COLS 4
typedef enum bnn_epoch_x_dtype { BNN_EPOCH_X_F32 = 0, BNN_EPOCH_X_U8 = 1 } bnn_epoch_x_dtype;
typedef struct bnn_epoch_perm_args {
  uint32_t struct_bytes;
  int32_t n_rows;                 /* N */
  uint64_t seed;
  const uint32_t* epoch;          /* device word e */
  int32_t* order;                 /* [N] */
} bnn_epoch_perm_args;
int bnn_epoch_permutation(const bnn_epoch_perm_args* args, void* stream);

typedef struct bnn_epoch_stage_args {
  uint32_t struct_bytes;
  int32_t n_rows;                 /* N */
  int32_t row_dim;                /* d */
  int32_t batch_size;             /* B */
  int32_t num_batches;            /* M, B M <= N */
  int32_t x_dtype;                /* bnn_epoch_x_dtype */
  int32_t target_dim;             /* 0: int64 labels; k >= 1: fp32 [N, k] */
  int32_t loss_cols;              /* 0 .. BNN_EPOCH_MAX_LOSS_COLS */
  const void* x;                  /* [N, d] fp32 or uint8 */
  const void* targets;            /* [N] int64 or [N, k] fp32 */
  const int32_t* order;           /* optional [N] */
  const float* beta_table;        /* optional [M] */
  uint32_t* batch_index;          /* device word j */
  uint32_t* epoch;                /* device word e */
  uint32_t* ticket;               /* device word, 0 between launches */
  float* x_out;                   /* [B, d] */
  void* x_bf16_out;               /* optional bf16 [B, d] */
  void* targets_out;              /* [B] int64 or [B, k] fp32 */
  float* beta;                    /* device word (with beta_table) */
  const float* loss_src[BNN_EPOCH_MAX_LOSS_COLS];   /* device words of the training step (with loss_history) */
  float* loss_history;            /* optional [M, loss_cols] */
} bnn_epoch_stage_args;
int bnn_epoch_stage(const bnn_epoch_stage_args* args, void* stream);

/* ------------------------------------------------------------------------------------
 * F9  SNR pruning sweep — weight_pruning.py:89-115 for P drop levels at once, without touching or copying the model:
 * thresholds by selection, a one-byte level code per parameter, a masked mean-weight forward for all levels, and the
 * evaluation tail.  Nothing here reads anything back to the host.
 *
 * bnn_snr_select   thresholds[p] (fp64, device) = np.percentile(snr, 100 fraction[p]) over the n = sum_s n[s] fp32 values of
 *     the segments snr[s][0 .. n[s]-1] (one segment per parameter tensor: the vector is never concatenated):
 *       pos = (n - 1) fraction[p] (fp64, on the host), lo = floor(pos), hi = min(lo + 1, n - 1), a = v_(lo), b = v_(hi) the
 *       order statistics, thresholds[p] = a when a == b, else a + (b - a) (pos - lo) -- two roundings, never fused.
 *     NaNs order last (torch.sort).  A 4-pass radix selection over order-preserving 32-bit keys for all 2 P ranks together,
 *     integer atomics only: bitwise reproducible.  fraction[] is a HOST array, in any order.  n < 2^31.
 *     Workspace: bnn_snr_select_workspace_bytes() bytes, 8-byte aligned, any contents.
 *   Errors: args, a segment, thresholds NULL: BNN_ERR_NULL; n_segments outside [1, BNN_PRUNE_MAX_SEGMENTS], n_levels outside
 *   [1, BNN_PRUNE_MAX_LEVELS], n[s] < 1, n >= 2^31, a fraction outside [0, 1] (or NaN): BNN_ERR_SHAPE; workspace NULL or short:
 *   BNN_ERR_WORKSPACE; a segment not 4-byte, thresholds / workspace not 8-byte aligned: BNN_ERR_ALIGN.
 *
 * bnn_prune_codes   one parameter tensor: code[o, i] = #{p < n_levels : snr_db(mu, rho) > (float)thresholds[p]} (thresholds
 *     ascending: the parameter survives level p exactly when code > p -- the comparison bnn_snr_prune makes with the same
 *     snr_db and the same fp32-rounded threshold), mu_out[o, i] = mu (fp32, or bf16 round to nearest even), both in the
 *     canonical [out_features, in_features] layout with row stride ld; kept[p] += #{code > p} (int64, integer atomics).
 *     The source is [out, in] (transposed = 0: BayesianLinear) or [in, out] (transposed = 1: BayesianLinearLR); a bias vector
 *     is out_features = 1, in_features = its length.  Elements of a row past in_features are not written.
 *   Errors: NULL mu, rho, thresholds, code, mu_out, kept: BNN_ERR_NULL; a dimension < 1, ld < in_features, n_levels outside
 *   [1, BNN_PRUNE_MAX_LEVELS]: BNN_ERR_SHAPE; mu_dtype outside bnn_dtype: BNN_ERR_ENUM; mu / rho not 4-byte, thresholds / kept not
 *   8-byte, mu_out not element aligned: BNN_ERR_ALIGN.
 *
 * bnn_pruned_fwd   y[p] = act(x[p] . (mu (.) [code > p])^T + b (.) [bcode > p]) for the levels p < n_levels of one layer.
 *     x: [rows, ldx] shared by all levels (x_shared != 0) or [n_levels, rows, ldx]; y: [n_levels, rows, ldy].  mu / code: the
 *     canonical images bnn_prune_codes writes, here with round_up(out_features, 64) rows of ld elements, ld % 32 == 0, both
 *     16-byte aligned, padding rows and columns zero (code 0 masks them at every level).  A block stages a 64 x 32 tile of mu
 *     and its codes once per k step and forms each level's masked fragment in registers: parameter bytes are read once per
 *     launch, whatever n_levels.  math BNN_MATH_BF16: x, mu bf16, v_mfma_f32_16x16x32_bf16, y bf16 or fp32; BNN_MATH_F32 and
 *     BNN_MATH_BF16X3: x, mu, y fp32, the exact v_mfma_f32_16x16x4_f32.  More than BNN_PRUNE_LEVELS_PER_LAUNCH levels run as
 *     several launches.  b / bcode: fp32 [out] and its codes, both or neither.
 *   Errors: NULL x, mu, code, y, or one of b / bcode without the other: BNN_ERR_NULL; a dimension < 1, n_levels outside
 *   [1, BNN_PRUNE_MAX_LEVELS], ld % 32, ld < in_features, ldx < in_features, ldy < out_features: BNN_ERR_SHAPE; math outside
 *   bnn_math, a dtype outside bnn_dtype or not the math mode's: BNN_ERR_ENUM; mu / code not 16-byte, x / y not element,
 *   b not 4-byte aligned: BNN_ERR_ALIGN.
 *
 * bnn_prune_sweep_tail   per level p and row r of a minibatch of `rows` rows starting at row `row0` of a data set of n_total:
 *     classification (BNN_NLL_CLASSIFICATION): probs[p, row0 + r, :] = softmax(logits[p, r, :]), correct[p] += (first-maximum
 *       argmax == target[r]), loss[p] += sum_r (logsumexp(logits[p, r, :]) - logits[p, r, target[r]])  (cross_entropy, sum);
 *     regression (BNN_NLL_REGRESSION): loss[p] += sum_{r, c} (logits[p, r, c] - target[r, c])^2; probs, correct unused.
 *     One block per level sums its rows in fp64 in a fixed order and is the only writer of its level's words: no float
 *     atomics, bitwise reproducible.  target: int64 [rows] or fp32 [rows, classes].  probs: [n_levels, n_total, classes].
 *   Errors: NULL logits, target, loss (and probs, correct in classification): BNN_ERR_NULL; a dimension < 1, n_levels outside
 *   [1, BNN_PRUNE_MAX_LEVELS], row0 < 0, row0 + rows > n_total: BNN_ERR_SHAPE; mode outside bnn_nll_mode: BNN_ERR_ENUM; logits /
 *   probs not 4-byte, target (labels) / correct / loss not 8-byte aligned: BNN_ERR_ALIGN.
 * ---------------------------------------------------------------------------------- */
#define BNN_PRUNE_MAX_LEVELS 16
#define BNN_PRUNE_MAX_SEGMENTS 16
#define BNN_PRUNE_LEVELS_PER_LAUNCH 8
/* layout: 4 x 4-byte words, 16 pointers, 16 int64, 16 doubles, pointer, size_t, pointer */
typedef struct bnn_snr_select_args {
  uint32_t struct_bytes;
  int32_t n_segments;                          /* 1 .. BNN_PRUNE_MAX_SEGMENTS */
  int32_t n_levels;                            /* P, 1 .. BNN_PRUNE_MAX_LEVELS */
  int32_t reserved;
  const float* snr[BNN_PRUNE_MAX_SEGMENTS];    /* device fp32 */
  int64_t n[BNN_PRUNE_MAX_SEGMENTS];
  double fraction[BNN_PRUNE_MAX_LEVELS];       /* host values in [0, 1] */
  void* workspace;
  size_t workspace_bytes;
  double* thresholds;                          /* device [P] */
} bnn_snr_select_args;
size_t bnn_snr_select_workspace_bytes(void);
int bnn_snr_select(const bnn_snr_select_args* args, void* stream);

/* layout: 8 x 4-byte words, then 6 pointers */
typedef struct bnn_prune_codes_args {
  uint32_t struct_bytes;
  int32_t out_features;
  int32_t in_features;
  int32_t ld;                                  /* row stride of code and mu_out, elements */
  int32_t transposed;                          /* 0: source [out, in]; 1: source [in, out] */
  int32_t n_levels;
  int32_t mu_dtype;                            /* bnn_dtype of mu_out */
  int32_t reserved;
  const float* mu;
  const float* rho;
  const double* thresholds;                    /* device [P], ascending */
  uint8_t* code;                               /* [out, ld] */
  void* mu_out;                                /* [out, ld] fp32 or bf16 */
  int64_t* kept;                               /* device [P], added to */
} bnn_prune_codes_args;
int bnn_prune_codes(const bnn_prune_codes_args* args, void* stream);

/* layout: 14 x 4-byte words, then 6 pointers */
typedef struct bnn_pruned_fwd_args {
  uint32_t struct_bytes;
  int32_t n_levels;
  int32_t rows;
  int32_t in_features;
  int32_t out_features;
  int32_t math;                                /* bnn_math */
  int32_t relu;
  int32_t x_shared;                            /* != 0: one x for all levels */
  int32_t x_dtype;                             /* bnn_dtype */
  int32_t y_dtype;                             /* bnn_dtype */
  int32_t ldx, ldy;                            /* row strides of x and y, elements */
  int32_t ld;                                  /* row stride of mu and code, elements, % 32 == 0 */
  int32_t reserved;
  const void* x;
  const void* mu;                              /* canonical [round_up(out, 64), ld] fp32 or bf16 */
  const uint8_t* code;                         /* same shape */
  const float* b;                              /* optional [out] */
  const uint8_t* bcode;                        /* with b */
  void* y;
} bnn_pruned_fwd_args;
int bnn_pruned_fwd(const bnn_pruned_fwd_args* args, void* stream);

/* layout: 6 x 4-byte words, 2 int64, then 5 pointers */
typedef struct bnn_prune_tail_args {
  uint32_t struct_bytes;
  int32_t mode;                                /* bnn_nll_mode */
  int32_t n_levels;
  int32_t rows;
  int32_t classes;
  int32_t reserved;
  int64_t n_total;
  int64_t row0;
  const float* logits;                         /* [P, rows, classes] */
  const void* target;                          /* int64 [rows] or fp32 [rows, classes] */
  float* probs;                                /* [P, n_total, classes] (classification) */
  int64_t* correct;                            /* [P] (classification), added to */
  double* loss;                                /* [P], added to */
} bnn_prune_tail_args;
int bnn_prune_sweep_tail(const bnn_prune_tail_args* args, void* stream);

/* ------------------------------------------------------------------------------------
 * F10  pool-based active learning — score an unlabelled pool, take the k rows the model is least sure about, add them to the
 * labelled subset, train on the subset: the selection and the subset's epoch order, without the host reading or writing data.
 *
 * bnn_acquire_topk   the candidates (rows i < N with candidate[i] != 0) in the TOTAL order
 *       score descending, then row index ascending; a NaN score after every other score; -0.0 equal to +0.0
 *     -- np.lexsort((index, key)) of key = the order-preserving integer image of -score, NaN last.  With C candidates and
 *     m = min(k, C):  selected[0 .. m) = the first m candidates in that order, selected[m .. k) = -1;
 *       candidate[selected[i]] = 0 and labelled[*n_labelled + i] = selected[i], i < m (entries past labelled[N - 1] are not
 *       written);  *n_labelled += m;  *n_selected = m (optional).
 *     Method: every candidate has the distinct 48-bit key (32 score bits, 16 index bits); a radix selection of the m-th
 *     smallest key in four 12-bit passes (LDS histograms, integer atomics; every block re-derives the earlier passes' digits
 *     from their histograms, so no block waits for another), a compaction of the keys up to it and a one-block bitonic sort
 *     in LDS: separate launches on the stream behind this one entry.  Integer atomics only: bitwise reproducible.
 *     Workspace: bnn_acquire_topk_workspace_bytes() bytes, 8-byte aligned, any contents.
 *   Errors: args, scores, candidate, selected, labelled, n_labelled NULL: BNN_ERR_NULL; N outside [1, BNN_EPOCH_MAX_ROWS], k
 *   outside [1, BNN_ACQUIRE_MAX_K]: BNN_ERR_SHAPE; workspace NULL or short: BNN_ERR_WORKSPACE; scores, selected, labelled,
 *   n_labelled, n_selected not 4-byte, workspace not 8-byte aligned: BNN_ERR_ALIGN.
 *
 * bnn_acquire_compose   order[i] = labelled[perm[i]], i < n (a perm entry outside [0, n) reads labelled[i]): the epoch order
 *     of the labelled subset from bnn_epoch_permutation's permutation of its n positions -- what bnn_epoch_stage gathers
 *     through, over the whole data set's rows.  No row is copied.
 *   Errors: a NULL pointer: BNN_ERR_NULL; n outside [1, BNN_EPOCH_MAX_ROWS]: BNN_ERR_SHAPE; a pointer not 4-byte aligned:
 *   BNN_ERR_ALIGN.
 *
 * bnn_acquire_random   scores[i] = (w_i >> 8) 2^-24 in [0, 1), i < N, with
 *     w_i = word (i & 3) of Philox4x32-R((i >> 2, round, 3, 1), key = (seed_lo, seed_hi)), R = bnn_philox_rounds():
 *   the "random" acquisition.  Counter words 2 and 3 are (3, 1): off the eps counters (word 3 = 0), the bandit's streams
 *   ((.., 0, 1), (.., 1, 1)) and F8's epoch permutation ((.., 2, 1)).  F15's label stream takes (.., 4, 1).
 *   Errors: scores NULL: BNN_ERR_NULL; N outside [1, BNN_EPOCH_MAX_ROWS]: BNN_ERR_SHAPE; scores not 4-byte aligned: BNN_ERR_ALIGN.
 * ---------------------------------------------------------------------------------- */
#define BNN_ACQUIRE_MAX_K 4096         /* winners of one launch: 4096 8-byte keys sort in 32 KiB of one block's LDS */
/* layout: 4 x 4-byte words, 7 pointers, size_t */
typedef struct bnn_acquire_topk_args {
  uint32_t struct_bytes;
  int32_t n_rows;                 /* N, 1 .. BNN_EPOCH_MAX_ROWS */
  int32_t k;                      /* 1 .. BNN_ACQUIRE_MAX_K */
  int32_t reserved;
  const float* scores;            /* device [N] */
  uint8_t* candidate;             /* device [N], 1 = still in the pool */
  int32_t* selected;              /* device [k] */
  int32_t* labelled;              /* device [N] */
  int32_t* n_labelled;            /* device word */
  int32_t* n_selected;            /* optional device word */
  void* workspace;
  size_t workspace_bytes;
} bnn_acquire_topk_args;
size_t bnn_acquire_topk_workspace_bytes(void);
int bnn_acquire_topk(const bnn_acquire_topk_args* args, void* stream);
int bnn_acquire_compose(const int32_t* labelled, const int32_t* perm, int32_t* order, int32_t n, void* stream);
int bnn_acquire_random(float* scores, int32_t n_rows, uint64_t seed, uint32_t round, void* stream);

/* ------------------------------------------------------------------------------------
 * F11  posterior statistics — the histograms of utils/logger_utils.py:13-26 (write_weight_histograms: twelve add_histogram
 * calls per epoch, each a device-to-host copy of a parameter tensor and a numpy binning) and of weight_pruning.py's figures
 * (collect_weights + sample_bnn_weights :16-44, the SNR density and CDF :59-79), for up to BNN_HIST_MAX_JOBS tensors in one
 * pass: every parameter is read once, the transform is fused in, a few KB are written, nothing is read back.
 *
 * Job j bins v_i, i < n, with
 *     BNN_HIST_VALUE    v = src0[i]                                     any fp32 tensor
 *     BNN_HIST_SIGMA    v = log1p(exp(src0[i]))                         src0 = rho; bit for bit bnn_softplus
 *     BNN_HIST_SNR_DB   v = 10 log10(|src0[i]| / log1p(exp(src1[i])))   src0 = mu, src1 = rho; bit for bit bnn_snr_db
 *     BNN_HIST_SAMPLE   v = fmaf(log1p(exp(src1[i])), eps_i, src0[i])   one fused multiply-add; eps_i = element i of what
 *                                                                       bnn_philox_normal(seed, tensor_id, sample, 1, rows, cols)
 *                                                                       writes (rows * cols = n)
 * against ONE table of n_edges strictly increasing finite fp64 edges, as np.histogram(v.astype(float64), bins=edges): bin b
 * is [e_b, e_b+1), the last bin is closed on the right, every comparison is made in fp64.  values_out (optional) receives
 * the n transformed fp32 values.
 *
 * Record of a job (device, 8-byte aligned, BNN_HIST_RECORD_BYTES(n_edges) bytes, overwritten by every call):
 *     uint64 counts[n_edges - 1], then a bnn_hist_summary:
 *     n_in (values inside [e_0, e_last]), n_below (< e_0, -inf included), n_above (> e_last, +inf included), n_nan;
 *     min, max over the non-NaN values (+inf, -inf when there are none); sum, sum_sq in fp64 over the finite values.
 * Counts are integer sums: exact.  The fp64 sums take a fixed order -- a block owns BNN_HIST_CHUNK consecutive elements of
 * one job, a thread adds its elements in index order, the block reduces by a fixed lane and wave tree, and a second launch
 * folds a job's block partials by a fixed tree -- so two calls over the same data return the same bits.  No floating-point
 * atomics.  Tensors are neither padded nor copied; no alignment beyond 4 bytes is asked of src0 / src1 / values_out; n = 0
 * is valid.  Workspace: bnn_param_hist_workspace_bytes(args) bytes, 8-byte aligned, any contents.  Three launches on the
 * stream (clear, bin, fold); hipGraph-capturable like every entry point.
 *   Errors: args, edges, a record, src0 (n > 0), src1 (SNR_DB / SAMPLE, n > 0) NULL: BNN_ERR_NULL; n_jobs outside
 *   [1, BNN_HIST_MAX_JOBS], n_edges outside [2, BNN_HIST_MAX_EDGES], n outside [0, 2^31), SAMPLE (n > 0) with rows or cols < 1
 *   or rows * cols != n, edges_host (optional HOST copy of the table, checked when given) not finite and strictly increasing:
 *   BNN_ERR_SHAPE; kind outside bnn_hist_kind: BNN_ERR_ENUM; workspace NULL or short: BNN_ERR_WORKSPACE; src0 / src1 /
 *   values_out not 4-byte, edges / record / workspace not 8-byte aligned: BNN_ERR_ALIGN.
 * ---------------------------------------------------------------------------------- */
#define BNN_HIST_MAX_JOBS 16           /* the twelve tensors of a network in one call */
#define BNN_HIST_MAX_EDGES 2048        /* 16 KiB of fp64 edges + four per-wave sub-histograms fit one block's LDS */
#define BNN_HIST_CHUNK 8192            /* consecutive elements of a job per block */
enum bnn_hist_kind { BNN_HIST_VALUE = 0, BNN_HIST_SIGMA = 1, BNN_HIST_SNR_DB = 2, BNN_HIST_SAMPLE = 3 };
typedef struct bnn_hist_summary {
  uint64_t n_in, n_below, n_above, n_nan;
  float min, max;
  double sum, sum_sq;
} bnn_hist_summary;
#define BNN_HIST_RECORD_BYTES(n_edges) (8u * ((size_t)(n_edges) - 1u) + sizeof(bnn_hist_summary))
/* layout: 6 x 4-byte words, int64, uint64, 4 pointers */
typedef struct bnn_param_hist_job {
  int32_t kind;                   /* bnn_hist_kind */
  int32_t rows, cols;             /* SAMPLE: the logical shape of the epsilon tensor */
  uint32_t tensor_id;             /* SAMPLE: 4 * layer_id + kind of the epsilon map */
  uint32_t sample;                /* SAMPLE: global MC sample index */
  uint32_t reserved;
  int64_t n;                      /* elements, 0 .. 2^31 - 1 */
  uint64_t seed;                  /* SAMPLE */
  const float* src0;              /* device [n] */
  const float* src1;              /* device [n]: SNR_DB, SAMPLE */
  float* values_out;              /* optional device [n] */
  void* record;                   /* device, BNN_HIST_RECORD_BYTES(n_edges) bytes */
} bnn_param_hist_job;
typedef struct bnn_param_hist_args {
  uint32_t struct_bytes;
  int32_t n_jobs;                 /* 1 .. BNN_HIST_MAX_JOBS */
  int32_t n_edges;                /* 2 .. BNN_HIST_MAX_EDGES */
  int32_t reserved;
  const double* edges;            /* device [n_edges] */
  const double* edges_host;       /* optional HOST copy (validated) */
  void* workspace;
  size_t workspace_bytes;
  bnn_param_hist_job jobs[BNN_HIST_MAX_JOBS];
} bnn_param_hist_args;
size_t bnn_param_hist_workspace_bytes(const bnn_param_hist_args* args);   /* 0 outside the limits */
int bnn_param_hist(const bnn_param_hist_args* args, void* stream);

/* ------------------------------------------------------------------------------------
 * F12  held-out predictive scores — how good the predictive distribution of S MC outputs is on labelled data: what a
 * caller otherwise composes per minibatch from forward_mc's [S, B, C] tensor with torch ops in fp32 (where a softmax that
 * underflows turns the log density into -inf).  One entry reads every sample once, evaluates in the log domain in fp64 and
 * accumulates a data-set-level record on the device; nothing is read back.
 *
 * bnn_mc_score   logits [G, S, B, C] (the layout of a stacked evaluation's output); rows with flat index g * B + b <
 * n_valid are scored, the others are padding: their logits and targets are never loaded and they add nothing.
 *
 *   BNN_NLL_CLASSIFICATION, per valid row, p_s = softmax(z_s), pbar = mean_s p_s, y the int64 label:
 *     lpd     = logsumexp_s(log p_{s,y}) - log S,   log p_{s,y} = z_{s,y} - logsumexp_c z_s      (log posterior predictive
 *               density; log domain throughout: finite when every p_{s,y} underflows)
 *     nll     = -(1/S) sum_s log p_{s,y}            (summed over rows: the mean over s of get_nll(output_s, target),
 *               networks.py:183-190 -- the expected NLL of the ELBO)
 *     brier   = sum_c (pbar_c - [c == y])^2
 *     correct = (argmax_c pbar == y), lowest index on ties (as preds of bnn_mc_predictive);  conf = max_c pbar_c
 *     bin i   = min(M - 1, ceil(conf M) - 1), the interval (i / M, (i + 1) / M]:  TOP-LABEL reliability bins of the
 *               MC-mean prediction -- not bnn_ece's bins, which are the reference's all-classes binning over a
 *               materialised probability table (every (row, class) probability is binned there).
 *     The label is compared against c and never used as an index: a label outside [0, C) reads nothing out of bounds and
 *     gives lpd = -inf (nll = +inf).
 *   BNN_NLL_REGRESSION, per valid (row, output), f_s the samples, y the fp32 target, under the N(f_s, sigma^2) mixture:
 *     lpd     = logsumexp_s(-(y - f_s)^2 / (2 sigma^2)) - log S - log sigma - log(2 pi) / 2
 *     nll     = (1/S) sum_s (y - f_s)^2 / (2 sigma^2) + log sigma + log(2 pi) / 2
 *     sq_err  = (y - mean_s f_s)^2,   abs_err = |y - mean_s f_s|
 *     PIT u   = (1/S) sum_s Phi((y - f_s) / sigma),  Phi(t) = erfc(-t / sqrt 2) / 2;   bin i = min(M - 1, floor(u M))
 *   All per-row arithmetic is fp64 (exp, log, erfc); the inputs are fp32.  A NaN logit in a valid row makes that row's
 *   terms NaN and the NaN goes into the sums; such a row (element) goes to no bin, is not counted correct, and still
 *   counts in rows (elements).
 *
 * Record (device, 8-byte aligned, BNN_SCORE_RECORD_BYTES(n_bins) bytes), in 8-byte words:
 *     word   classification                                regression
 *     0      int64 rows                                    int64 rows
 *     1      int64 correct                                 int64 elements (rows * C)
 *     2      f64 sum lpd                                   f64 sum lpd
 *     3      f64 sum nll                                   f64 sum nll
 *     4      f64 sum brier                                 f64 sum sq_err
 *     5      0                                             f64 sum abs_err
 *     6, 7   reserved (0)                                  reserved (0)
 *     then per bin, 3 words:  {int64 count, int64 correct, f64 sum conf}    {int64 count, 0, 0}
 *   accumulate = 0 overwrites the record, 1 adds the call's totals to it (in stream order).
 * row_lpd / row_nll (optional, fp32 [G, B]): the per-row values, for regression summed over the C outputs of the row;
 * padding rows are left unwritten.
 * Determinism: a block writes one partial record to the workspace (its rows in order; lanes and waves by a fixed tree), a
 * second one-block launch adds the partials in block-index order and writes / adds to the record.  No floating-point
 * atomics: the same call repeated gives a bit-identical record.  Workspace: bnn_mc_score_workspace_bytes(G, B, C) bytes,
 * 8-byte aligned, any contents.  Two launches (three for regression with row outputs); hipGraph-capturable.
 *   Errors, checked in this order before any launch: struct_bytes: BNN_ERR_ABI; mode outside bnn_nll_mode: BNN_ERR_ENUM; a
 *   dimension < 1, n_valid outside [1, G B], n_bins outside [0, BNN_SCORE_MAX_BINS], regression sigma not > 0:
 *   BNN_ERR_SHAPE; args, logits, targets, record NULL, workspace NULL or short: BNN_ERR_NULL; record / workspace / int64
 *   targets not 8-byte, logits / fp32 targets / row outputs not 4-byte aligned: BNN_ERR_ALIGN.
 * ---------------------------------------------------------------------------------- */
#define BNN_SCORE_MAX_BINS 64
#define BNN_SCORE_RECORD_BYTES(n_bins) (8 * (8 + 3 * (n_bins)))   /* 8-byte words */
/* layout: 6 x 4-byte words, 2 pointers, int64, 4 x 4-byte words, 4 pointers, size_t */
typedef struct bnn_mc_score_args {
  uint32_t struct_bytes;
  int32_t mode;                   /* bnn_nll_mode */
  int32_t groups, n_samples, batch, classes;
  const float* logits;            /* device [G, S, B, C] */
  const void* targets;            /* classification int64 [G, B]; regression fp32 [G, B, C] */
  int64_t n_valid;                /* 1 .. G * B */
  float sigma;                    /* regression, > 0 */
  int32_t n_bins;                 /* 0 .. BNN_SCORE_MAX_BINS */
  int32_t accumulate;             /* 0 overwrites the record, 1 adds to it */
  int32_t reserved;
  float* row_lpd;                 /* optional device [G, B] */
  float* row_nll;                 /* optional device [G, B] */
  void* record;                   /* device, BNN_SCORE_RECORD_BYTES(n_bins) bytes */
  void* workspace;
  size_t workspace_bytes;
} bnn_mc_score_args;
size_t bnn_mc_score_workspace_bytes(int32_t groups, int32_t batch, int32_t classes);   /* 0 outside the limits */
int bnn_mc_score(const bnn_mc_score_args* args, void* stream);

/* ------------------------------------------------------------------------------------
 * F13  compressed pruned network — the network F9 prunes at ONE level, kept as CSR (one row per output feature, the surviving
 * columns ascending) and run over the survivors only: a pruned weight is neither stored, read nor drawn.  The posterior this
 * samples: a survivor is N(mu, softplus(rho)^2), a pruned weight is a point mass at exactly zero -- not the sigma = ln 2 that
 * sampling a prune_weights copy (mu = rho = 0) gives.
 *
 * bnn_sparse_count   one parameter tensor at level `level` of the canonical [out, ld] code image bnn_prune_codes writes:
 *     row_ptr[0 .. out] (int32) = the exclusive scan of the per-row survivor counts #{i < in : code[o, i] > level};
 *     row_ptr[out] is nnz.  Two launches (counts, then a one-block scan in place); integers only: bitwise reproducible.
 *   Errors: NULL code, row_ptr: BNN_ERR_NULL; a dimension < 1, ld < in_features, out * in >= 2^31, level outside
 *   [0, BNN_PRUNE_MAX_LEVELS): BNN_ERR_SHAPE; row_ptr not 4-byte aligned: BNN_ERR_ALIGN.
 *
 * bnn_sparse_fill   the second pass: for row o and its j-th survivor (columns ascending), at e = row_ptr[o] + j,
 *     col[e] (uint16) = the column, mu_val[e] / rho_val[e] = the ORIGINAL fp32 parameters mu / rho (source [out, in], or
 *     [in, out] with transposed = 1, as in bnn_prune_codes) -- not the sweep's mu_out, which is bf16 under bf16 math.
 *     A wave owns a row and places its survivors by ballot and prefix count: the order depends on no scheduling.
 *     sigma_val is not written here: the caller forms it with bnn_softplus over rho_val, so it holds the bits every
 *     other kernel uses for that weight.  row_ptr must be what bnn_sparse_count wrote for the same code and level.
 *   Errors: NULL code, row_ptr, mu, rho, col, mu_val, rho_val: BNN_ERR_NULL; a dimension < 1, ld < in_features,
 *   in_features > 65536 (uint16 columns), level outside [0, BNN_PRUNE_MAX_LEVELS): BNN_ERR_SHAPE; row_ptr / mu / rho / mu_val /
 *   rho_val not 4-byte, col not 2-byte aligned: BNN_ERR_ALIGN.
 *
 * bnn_sparse_fwd   one layer, n_samples MC samples, `rows` batch rows, exact fp32, one fixed chain per output element:
 *       acc = 0;  for e = row_ptr[o] .. row_ptr[o+1]-1 (ascending):  acc = fmaf(x[xs, r, col[e]], w_e, acc)
 *       y[s, r, o] = act(acc + b_o)
 *     w_e = fmaf(sigma_val[e], eps_e, mu_val[e]) (mu_val[e] under BNN_EPS_ZERO); b_o = fmaf(b_sigma[o], eps_b, b_mu[o])
 *     (b_mu[o] under BNN_EPS_ZERO) on dense [out] bias vectors the caller has multiplied by the bias mask (pruned bias:
 *     b_mu = 0, b_sigma = 0).  The result depends on no tiling, on no cut of a batch into calls, and not on n_samples.
 *     Epsilon: eps_e is element (row o, col col[e]) of the Philox map at the head of this file for tensor id 4 * layer_id + 0
 *     and the global sample g, computed as for the DENSE [out, in] tensor -- group = o * ceil(in / 4) + (col >> 2), slot
 *     col & 3 -- so a kept weight draws exactly the epsilon the dense network draws for it; the survivors that share a
 *     group share one Philox call.  eps_b is kind 1, as in K1.  For a BayesianLinearLR network the SAME weight-space map is
 *     used on the canonical [out, in] indices: a draw from the same factorised posterior over the weights, not the
 *     activation-space draw (kind 2) the local-reparameterisation layers make.  sample_offset, sample_counter,
 *     sample_group and sample_group_stride behave as in K1's argument block.  BNN_EPS_MEMORY reads eps [n_samples, nnz] and
 *     eps_b [n_samples, out]; eps_dump / eps_b_dump (optional, same shapes) return what was used.
 *     Layout: x is [x_rows, rows, in] (x_feature_major = 0) or [x_rows, in, rows] (1); x_rows = 1 when x_per_sample == 0,
 *     else sample s reads x[s / x_per_sample].  y is [n_samples, rows, out] (y_feature_major = 0) or [n_samples, out, rows]
 *     (1).  The lanes of a wave are batch rows and a row's CSR entries are wave-uniform, so a feature-major x makes a
 *     column's gather one coalesced read: keep activations feature-major between layers.  With a row-major x and
 *     x_scratch (fp32 [x_rows, in, rows]) a transpose launch ahead of the layer writes x there and the layer reads that.
 *   Errors: NULL row_ptr, col, mu_val, x, y, b_mu (sigma_val, b_sigma unless BNN_EPS_ZERO; eps, eps_b under
 *   BNN_EPS_MEMORY): BNN_ERR_NULL; a dimension < 1, n_samples > 65535, in_features > 65536, x_per_sample < 0:
 *   BNN_ERR_SHAPE; eps_mode outside bnn_eps_mode: BNN_ERR_ENUM; a pointer not aligned to its element: BNN_ERR_ALIGN.
 * ---------------------------------------------------------------------------------- */
/* layout: 6 x 4-byte words, then 2 pointers */
typedef struct bnn_sparse_count_args {
  uint32_t struct_bytes;
  int32_t out_features;
  int32_t in_features;
  int32_t ld;                                  /* row stride of code, elements */
  int32_t level;                               /* the survivors have code > level */
  int32_t reserved;
  const uint8_t* code;                         /* [out, ld] */
  int32_t* row_ptr;                            /* [out + 1] */
} bnn_sparse_count_args;
int bnn_sparse_count(const bnn_sparse_count_args* args, void* stream);

/* layout: 6 x 4-byte words, then 7 pointers */
typedef struct bnn_sparse_fill_args {
  uint32_t struct_bytes;
  int32_t out_features;
  int32_t in_features;
  int32_t ld;
  int32_t level;
  int32_t transposed;                          /* 0: mu / rho are [out, in]; 1: [in, out] */
  const uint8_t* code;                         /* [out, ld] */
  const int32_t* row_ptr;                      /* [out + 1], from bnn_sparse_count */
  const float* mu;
  const float* rho;
  uint16_t* col;                               /* [nnz] */
  float* mu_val;                               /* [nnz] */
  float* rho_val;                              /* [nnz] */
} bnn_sparse_fill_args;
int bnn_sparse_fill(const bnn_sparse_fill_args* args, void* stream);

/* layout: 12 x 4-byte words, the 8-byte seed, 4 x 4-byte words, then 14 pointers */
typedef struct bnn_sparse_fwd_args {
  uint32_t struct_bytes;
  int32_t n_samples;
  int32_t rows;                                /* batch rows */
  int32_t in_features;
  int32_t out_features;
  int32_t eps_mode;                            /* bnn_eps_mode */
  int32_t relu;
  int32_t x_per_sample;                        /* 0: one x for all samples; g >= 1: sample s reads x[s / g] */
  int32_t x_feature_major;                     /* x is [x_rows, in, rows] */
  int32_t y_feature_major;                     /* y is [n_samples, out, rows] */
  uint32_t layer_id;
  uint32_t sample_offset;
  uint64_t seed;
  uint32_t sample_group;                       /* as in K1 */
  uint32_t sample_group_stride;
  int32_t reserved0, reserved1;
  const uint32_t* sample_counter;              /* optional device word added to sample_offset at run time */
  const int32_t* row_ptr;                      /* [out + 1] */
  const uint16_t* col;                         /* [nnz] */
  const float* mu_val;                         /* [nnz] */
  const float* sigma_val;                      /* [nnz], bnn_softplus over rho_val */
  const float* b_mu;                           /* [out], masked */
  const float* b_sigma;                        /* [out], masked */
  const float* x;
  float* y;
  const float* eps;                            /* BNN_EPS_MEMORY: [n_samples, nnz] */
  const float* eps_b;                          /* BNN_EPS_MEMORY: [n_samples, out] */
  float* eps_dump;                             /* optional [n_samples, nnz] */
  float* eps_b_dump;                           /* optional [n_samples, out] */
  float* x_scratch;                            /* optional [x_rows, in, rows]: the transposed copy of a row-major x */
} bnn_sparse_fwd_args;
int bnn_sparse_fwd(const bnn_sparse_fwd_args* args, void* stream);

/* ------------------------------------------------------------------------------------
 * F14  training the compressed network — the Bayes-by-backprop step over the SURVIVORS of an F13 network only: the pattern
 * (row_ptr, col) is fixed, a pruned weight or bias is a point mass at exactly zero in every sample, is in neither ELBO sum
 * and receives no gradient.  The forward is bnn_sparse_fwd, the NLL / loss / seeds are bnn_elbo_finalize (n_layers = 0)
 * and bnn_elbo_loss_nll_bwd, the update is bnn_adam_step over the value arrays; the entry points below add the rest.
 * Per layer and global MC sample g (sample_offset + *sample_counter + s, as in bnn_sparse_fwd), with e = (o, c) a CSR entry:
 *     w_e = fmaf(sigma_e, eps_e, mu_e),  sigma_e = softplus(rho_e);    b_o = fmaf(b_sigma_o, eps_b, b_mu_o) for a kept bias
 *     eps_e: the dense weight-space map of F13 (tensor id 4 * layer_id + 0, group o * ceil(in / 4) + (c >> 2), slot c & 3);
 *     eps_b: kind 1, group o >> 2, slot o & 3.
 * No float atomics anywhere and one fixed summation order per shape: a step repeated from one state gives the same bits.
 *
 * bnn_sparse_elbo_terms   log_q[s] and log_prior[s] (float [n_samples]) of up to BNN_SPARSE_MAX_LAYERS layers:
 *       log_q[s]     = sum over kept weights and kept biases of  -log sqrt(2 pi) - log sigma - eps^2 / 2
 *       log_prior[s] = sum over kept weights and kept biases of  log prior(w)          (Gaussian or scale mixture)
 *     per layer as K1 / K4 form them (sums of eps^2, of w^2 or log mixture density, of log sigma; the constants times the
 *     count in fp64; one fp32 rounding per layer, then fp32 adds in layer order).  Two launches: blocks of 1024 entries
 *     (or 256 biases) of one (layer, sample) write one partial each -- thread, wave (DPP), block in a fixed order -- then one
 *     block per sample folds the partials of each layer in fp64 in a fixed tree.  b_keep (uint8 [out]): 1 = the bias is kept.
 *     nnz must be the layer's row_ptr[out] (the host knows it from construction; the kernels never run past the smaller).
 *   Errors, in this order: args NULL: BNN_ERR_NULL; struct_bytes: BNN_ERR_ABI; n_layers outside [1, BNN_SPARSE_MAX_LAYERS],
 *   n_samples outside [1, 65535], a layer with a dimension < 1, in_features > 65536, nnz < 0 or nnz > out * in:
 *   BNN_ERR_SHAPE; prior.kind outside bnn_prior_kind: BNN_ERR_ENUM; a prior scale <= 0: BNN_ERR_SHAPE; log_prior, log_q or a
 *   layer's row_ptr, col, mu_val, sigma_val, b_mu, b_sigma, b_keep NULL: BNN_ERR_NULL; workspace NULL or below
 *   bnn_sparse_elbo_terms_workspace_bytes: BNN_ERR_WORKSPACE; a pointer not aligned to its element, the workspace not
 *   16-byte aligned: BNN_ERR_ALIGN.
 *
 * bnn_sparse_bwd   the backward of ONE layer: the closed forms of bnn_bbb_linear_bwd restricted to the survivors.
 *       gz_s = gy_s * (y_s > 0) if relu
 *       G_e,s = sum_r gz_s[o, r] x_s[c, r];   t_e,s = G_e,s + g_log_prior[s] * dlogp/dw(w_e,s)
 *       g_mu_val[e]  = sum_s t_e,s
 *       g_rho_val[e] = (sum_s t_e,s eps_e,s - (sum_s g_log_q[s]) / sigma_e) * sigmoid(rho_e)
 *       g_b_mu / g_b_rho likewise with the row sums of gz in place of G; 0 for a pruned bias (b_keep[o] == 0)
 *       g_x[s, c, r] = sum_o w_(o,c),s gz_s[o, r]   (ascending o; times (x > 0) with gx_relu_mask), optional
 *     Layouts: x [x_rows, in, rows] and y [n_samples, out, rows] feature-major, as bnn_sparse_fwd leaves them (x_rows and
 *     x_per_sample as there; y is read only with relu); gy [n_samples, rows, out] with gy_row_major (the output layer:
 *     bnn_elbo_loss_nll_bwd's g_logits), else [n_samples, out, rows]; g_x [n_samples, in, rows].  Epsilon is REGENERATED:
 *     nothing of size [n_samples, nnz] is kept from the forward.  Up to three launches:
 *       gz      into the workspace, feature-major (skipped when gy is feature-major and relu == 0);
 *       weights a wave owns 16 consecutive entries and walks them in runs of up to four survivors of one row and one Philox
 *               group: per run ONE Philox call serves 64 samples (lane = sample), the samples run in ascending order
 *               inside the kernel with sum_s t and sum_s t eps in registers, and an entry's G is the dot of two coalesced
 *               rows (lane l takes batch rows l, l + 64, ... ascending, then the wave's fixed DPP sum).  The biases are
 *               further blocks of the same launch, a wave per output feature;
 *       g_x     bnn_sparse_fwd's structure over the CSC view: a block is (column group, sample, batch block), stage A
 *               regenerates w from mu_val[perm], rho_val[perm] and the epsilon at (o, c) into LDS, stage B runs one
 *               ascending-o fmaf chain per g_x element, lanes over batch rows.
 *     The CSC view (only with g_x): col_ptr int32 [in + 1], row uint16 [nnz] (the output feature), perm int32 [nnz] (the
 *     CSR position), rows ascending within a column -- a stable sort of col.
 *   Errors, in this order: args NULL: BNN_ERR_NULL; struct_bytes: BNN_ERR_ABI; a dimension < 1, n_samples > 65535,
 *   in_features > 65536, out_features > 65536 or rows > 65535 * 256 with g_x, nnz < 0 or nnz > out * in, x_per_sample < 0: BNN_ERR_SHAPE;
 *   prior.kind outside bnn_prior_kind: BNN_ERR_ENUM; a prior scale <= 0: BNN_ERR_SHAPE; row_ptr, col, mu_val, rho_val, b_mu, b_rho, b_keep, x,
 *   gy, g_mu_val, g_rho_val, g_b_mu, g_b_rho NULL, y NULL with relu, col_ptr / row / perm NULL with g_x: BNN_ERR_NULL;
 *   workspace NULL or below bnn_sparse_bwd_workspace_bytes when the gz launch runs (relu or gy_row_major; it is not read
 *   otherwise and may be NULL): BNN_ERR_WORKSPACE; a pointer not aligned to its element:
 *   BNN_ERR_ALIGN.
 *
 * bnn_sparse_sigma_refresh   after the optimiser: sigma[i] = keep[i] ? softplus(rho[i]) : 0 over up to
 *     BNN_SPARSE_MAX_SEGMENTS segments in one launch (keep NULL: every element kept) -- the bits bnn_softplus gives.
 *   Errors: args NULL: BNN_ERR_NULL; struct_bytes: BNN_ERR_ABI; n_segments outside [1, BNN_SPARSE_MAX_SEGMENTS], n[i] < 0:
 *   BNN_ERR_SHAPE; rho or sigma of a segment with n > 0 NULL: BNN_ERR_NULL; rho / sigma not 4-byte aligned: BNN_ERR_ALIGN.
 * ---------------------------------------------------------------------------------- */
#define BNN_SPARSE_MAX_LAYERS 8
#define BNN_SPARSE_MAX_SEGMENTS 8

/* layout: 4 x 4-byte words, then 7 pointers */
typedef struct bnn_sparse_elbo_layer {
  int32_t in_features;
  int32_t out_features;
  int32_t nnz;
  uint32_t layer_id;
  const int32_t* row_ptr;                      /* [out + 1] */
  const uint16_t* col;                         /* [nnz] */
  const float* mu_val;                         /* [nnz] */
  const float* sigma_val;                      /* [nnz] */
  const float* b_mu;                           /* [out] */
  const float* b_sigma;                        /* [out] */
  const uint8_t* b_keep;                       /* [out] */
} bnn_sparse_elbo_layer;

/* layout: 4 x 4-byte words, the 8-byte seed, the prior (5 words), 1 word, a pointer, the layers, 3 pointers, a size */
typedef struct bnn_sparse_elbo_args {
  uint32_t struct_bytes;
  int32_t n_layers;
  int32_t n_samples;
  uint32_t sample_offset;
  uint64_t seed;
  bnn_prior prior;
  int32_t reserved;
  const uint32_t* sample_counter;              /* optional device word added to sample_offset at run time */
  bnn_sparse_elbo_layer layer[BNN_SPARSE_MAX_LAYERS];
  float* log_prior;                            /* [n_samples] */
  float* log_q;                                /* [n_samples] */
  void* workspace;
  size_t workspace_bytes;
} bnn_sparse_elbo_args;
/* nnz, out_features: [n_layers]; 0 outside the limits */
size_t bnn_sparse_elbo_terms_workspace_bytes(int32_t n_layers, int32_t n_samples, const int32_t* nnz, const int32_t* out_features);
int bnn_sparse_elbo_terms(const bnn_sparse_elbo_args* args, void* stream);

/* layout: 12 x 4-byte words, the 8-byte seed, the prior (5 words), 1 word, 22 pointers, a size */
typedef struct bnn_sparse_bwd_args {
  uint32_t struct_bytes;
  int32_t n_samples;
  int32_t rows;                                /* batch rows */
  int32_t in_features;
  int32_t out_features;
  int32_t nnz;
  int32_t relu;
  int32_t gy_row_major;                        /* gy is [n_samples, rows, out] */
  int32_t x_per_sample;                        /* as in bnn_sparse_fwd */
  int32_t gx_relu_mask;                        /* g_x is multiplied by (x > 0) */
  uint32_t layer_id;
  uint32_t sample_offset;
  uint64_t seed;
  bnn_prior prior;
  int32_t reserved;
  const uint32_t* sample_counter;              /* optional: the value the forward of the same step read */
  const int32_t* row_ptr;                      /* [out + 1] */
  const uint16_t* col;                         /* [nnz] */
  const float* mu_val;                         /* [nnz] */
  const float* rho_val;                        /* [nnz] */
  const int32_t* col_ptr;                      /* [in + 1]   (with g_x) */
  const uint16_t* row;                         /* [nnz]      (with g_x) */
  const int32_t* perm;                         /* [nnz]      (with g_x) */
  const float* b_mu;                           /* [out] */
  const float* b_rho;                          /* [out] */
  const uint8_t* b_keep;                       /* [out] */
  const float* x;
  const float* y;                              /* with relu */
  const float* gy;
  const float* g_log_prior;                    /* [n_samples] or NULL (zeros) */
  const float* g_log_q;                        /* [n_samples] or NULL (zeros) */
  float* g_mu_val;                             /* [nnz] */
  float* g_rho_val;                            /* [nnz] */
  float* g_b_mu;                               /* [out] */
  float* g_b_rho;                              /* [out] */
  float* g_x;                                  /* optional [n_samples, in, rows] */
  void* workspace;
  size_t workspace_bytes;
} bnn_sparse_bwd_args;
size_t bnn_sparse_bwd_workspace_bytes(int32_t n_samples, int32_t rows, int32_t out_features);   /* 0 outside the limits */
int bnn_sparse_bwd(const bnn_sparse_bwd_args* args, void* stream);

/* layout: 2 x 4-byte words, then 3 x 8 pointers and 8 x 8-byte counts */
typedef struct bnn_sparse_sigma_args {
  uint32_t struct_bytes;
  int32_t n_segments;
  const float* rho[BNN_SPARSE_MAX_SEGMENTS];
  float* sigma[BNN_SPARSE_MAX_SEGMENTS];
  const uint8_t* keep[BNN_SPARSE_MAX_SEGMENTS];   /* optional per segment */
  int64_t n[BNN_SPARSE_MAX_SEGMENTS];
} bnn_sparse_sigma_args;
int bnn_sparse_sigma_refresh(const bnn_sparse_sigma_args* args, void* stream);

/* ------------------------------------------------------------------------------------
 * F15  BatchBALD — a batch of k pool rows chosen JOINTLY (Kirsch, van Amersfoort, Gal 2019): F10's top-k of per-row mutual
 * information picks near-duplicates, because every row is scored as if it were acquired alone.  The batch score is
 *     I(y_1 .. y_n ; w) = H(y_1 .. y_n) - sum_j E_w H(y_j | w),
 * built greedily: step n scores every pool row i together with the n-1 rows already chosen, bnn_acquire_topk (k = 1) takes
 * the winner, bnn_batchbald_extend folds it into the state.  S weight draws are shared by ALL rows (weight-space epsilon is
 * keyed by the sample index and not by x), so P[s, i, :] of different rows are conditionally independent given s.
 * State of a batch: Phat [M, S] fp32 (row m: one label configuration of the chosen rows, entry s: its probability under
 * draw s, times 2^-E[m]), E int32 [M], weight w and offset o fp64 [M], base fp64 (sum of cond over the chosen rows).
 *   M = bnn_batchbald_configs(C, n, max_configs) = C^n while C^n <= max_configs (every configuration: EXACT mode), else
 *   max_configs (SAMPLED mode); 0 for arguments outside the limits below.  A host value: grids are sized without a read.
 *
 * bnn_batchbald_probs   one chunk of MC logits [S, B, C] (rows row0 .. row0 + B - 1 of the pool):
 *     P[s, row0 + b, c] = e_c / sum_c' e_c', e_c = expf(logit_c - max_c' logit_c'), all fp32, into the pool-wide P [S, N, C];
 *     cond[row] = -(1/S) sum_s sum_c P log P and marg[row] = - sum_c pbar_c log pbar_c, pbar_c = (1/S) sum_s P[s, row, c]:
 *     fp64 sums in ascending (s, c) of the fp32 P, fp64 log, 0 log 0 = 0.
 *   Errors: args, logits, probs, cond, marg NULL: BNN_ERR_NULL; C outside [2, BNN_BATCHBALD_MAX_CLASSES], S outside
 *   [1, BNN_BATCHBALD_MAX_SAMPLES], N outside [1, BNN_EPOCH_MAX_ROWS], B < 1, row0 < 0 or row0 + B > N: BNN_ERR_SHAPE;
 *   logits, probs not 4-byte, cond, marg not 8-byte aligned: BNN_ERR_ALIGN.
 *
 * bnn_batchbald_joint   for every row i < N, with pt[m, i, y] = (1/S) sum_s Phat[m, s] P[s, i, y]:
 *     joint64[i]  = H[i] = - sum_m w[m] sum_y pt (log pt + o[m])        (pt = 0 contributes 0)
 *     scores64[i] = H[i] - cond[i] - *base;   scores[i] = (float)scores64[i]        -- what bnn_acquire_topk ranks.
 *   The M x (N C) product is never stored: v_mfma_f32_16x16x4_f32 tiles (exact fp32 operands; one fp32 fmaf chain over
 *   the samples in the order s = 16 Q + 4 g + j for Q, then j, then g = 0 .. 3 ascending, samples past S skipped)
 *   whose accumulators go straight into log (fp32 v_log_f32, widened) and an fp64 sum.  A block owns floor(64 / C) rows and
 *   a contiguous range of M ("split"); every lane adds its terms in ascending m, the lanes of a row are folded in a fixed
 *   order, the splits [splits, N] (fp64, in the workspace) by a second launch in ascending split: no float atomics, the same
 *   inputs give the same bits.  The split count is a function of (N, C, M) alone.  An s-sum below FLT_MIN (1.2e-38)
 *   contributes 0 like an exact zero (its term is below 1e-35).  Never NaN for finite inputs.
 *   Workspace: bnn_batchbald_joint_workspace_bytes(N, C, M) bytes, 8-byte aligned, any contents: enough for every n_configs
 *   up to M, so one buffer serves all steps of a batch (0 for arguments outside the limits).
 *   Errors: args, probs, phat, weight, offset, cond, base, scores NULL: BNN_ERR_NULL; C, S, N as above, M outside
 *   [1, BNN_BATCHBALD_MAX_CONFIGS]: BNN_ERR_SHAPE; workspace NULL or short: BNN_ERR_WORKSPACE; probs, phat, scores not
 *   4-byte, weight, offset, cond, base, scores64, joint64, workspace not 8-byte aligned: BNN_ERR_ALIGN.
 *
 * bnn_batchbald_begin   the empty batch: phat_out[0, 0 .. S) = 1, expo_out[0] = 0, weight[0] = 1, offset[0] = 0, *base = 0
 *     (M = 1).  The first bnn_batchbald_joint then gives marg - cond: plain BALD.
 *   Errors: args, phat_out, expo_out, weight, offset, base NULL: BNN_ERR_NULL; S outside its limits: BNN_ERR_SHAPE; phat_out,
 *   expo_out not 4-byte, weight, offset, base not 8-byte aligned: BNN_ERR_ALIGN.
 *
 * bnn_batchbald_extend   after bnn_acquire_topk appended the winner of step n = n_chosen: i* = labelled[*n_labelled - 1]
 *     (the position and the row clamped into [0, N): a bad word never indexes outside P or labelled), chosen row j < n:
 *     i_j = labelled[*n_labelled - n + j] likewise.  Writes the state of step n + 1 from (phat_in, expo_in) into (phat_out,
 *     expo_out, weight, offset) -- in and out must not overlap --, *base += cond[i*] and, with batch_scores,
 *     batch_scores[n - 1] = scores64[i*]: the BatchBALD value of the first n rows.
 *     With `last` set nothing else is written: no further step reads a state (phat_out and its companions are untouched).
 *     A FACTOR f[s] multiplies a row: v[s] = fl32(row[s] * f[s]); then the row is RESCALED by an exact power of two: with
 *     x = max_s v[s] > 0 and frexp(x) = (f, e), f in [0.5, 1): row[s] = ldexpf(v[s], -e), E += e; an all-zero row keeps e = 0.
 *     EXACT (C^n <= max_configs):  row m C + c of the M C new rows = row m times the factor P[s, i*, c], E from E[m];
 *       weight = 2^E (ldexp(1.0, E)), offset = E ln 2 (fp64 product with 0x1.62e42fefa39efp-1).
 *     SAMPLED (otherwise), M = max_configs rows, row m tied to weight draw s_m = m mod S: its label for chosen row j is
 *       y = min(C - 1, #{c : cum_c <= t}), cum_c the fp32 running sums of P[s_m, i_j, :] in ascending c, t = fl32(u cum_{C-1}),
 *       u = (word 0 >> 8) 2^-24 of Philox4x32-R((m, j | round << 8, 4, 1), key = (seed_lo, seed_hi)), R = bnn_philox_rounds():
 *       counter words 2 and 3 are (4, 1), beside F10's (3, 1).  A pure function of (seed, round, m, j, that row of P).
 *       At the first sampled step the rows are rebuilt from ones by the factors P[s, i_j, y_mj] of j = 0 .. n - 1 in
 *       ascending j, rescaled after each; later steps multiply the rows of phat_in by the one factor j = n - 1.
 *       weight = 1 / (M qt), qt = (sum_s row[s]) / S in fp64, ascending s (0 where qt = 0); offset = E ln 2: the paper's
 *       importance-weighted estimator  H ~ -(1/M) sum_m sum_y (p(yhat_m, y) / p(yhat_m)) log p(yhat_m, y).
 *   Errors: args, probs, cond, labelled, n_labelled, phat_in, expo_in, phat_out, expo_out, weight, offset, base NULL,
 *   scores64 NULL with batch_scores: BNN_ERR_NULL; C, S, N as above, max_configs outside [1, BNN_BATCHBALD_MAX_CONFIGS],
 *   n_chosen outside [1, BNN_BATCHBALD_MAX_K]: BNN_ERR_SHAPE; a 4-byte (probs, labelled, n_labelled, phat_*, expo_*) or
 *   8-byte (cond, scores64, weight, offset, base, batch_scores) pointer misaligned: BNN_ERR_ALIGN.
 * ---------------------------------------------------------------------------------- */
#define BNN_BATCHBALD_MAX_CLASSES 32
#define BNN_BATCHBALD_MAX_SAMPLES 128     /* the K dimension of the joint product; a block's Phat tile is 64 x 132 fp32 = 33 KiB of LDS */
#define BNN_BATCHBALD_MAX_K 64            /* rows of one batch (j takes 8 bits of the label stream's counter) */
#define BNN_BATCHBALD_MAX_CONFIGS 65536
/* layout: 6 x 4-byte words, 4 pointers */
typedef struct bnn_batchbald_probs_args {
  uint32_t struct_bytes;
  int32_t n_samples;              /* S */
  int32_t n_rows;                 /* N: rows of the pool */
  int32_t n_classes;              /* C */
  int32_t row0;                   /* first pool row of the chunk */
  int32_t chunk_rows;             /* B */
  const float* logits;            /* device [S, B, C] */
  float* probs;                   /* device [S, N, C] */
  double* cond;                   /* device [N] */
  double* marg;                   /* device [N] */
} bnn_batchbald_probs_args;
/* layout: 6 x 4-byte words, 10 pointers, size_t */
typedef struct bnn_batchbald_joint_args {
  uint32_t struct_bytes;
  int32_t n_samples;              /* S */
  int32_t n_rows;                 /* N */
  int32_t n_classes;              /* C */
  int32_t n_configs;              /* M */
  int32_t reserved;
  const float* probs;             /* device [S, N, C] */
  const float* phat;              /* device [M, S] */
  const double* weight;           /* device [M] */
  const double* offset;           /* device [M] */
  const double* cond;             /* device [N] */
  const double* base;             /* device word */
  float* scores;                  /* device [N] */
  double* scores64;               /* optional device [N] */
  double* joint64;                /* optional device [N] */
  void* workspace;
  size_t workspace_bytes;
} bnn_batchbald_joint_args;
/* layout: 8 x 4-byte words, uint64, 13 pointers */
typedef struct bnn_batchbald_state_args {
  uint32_t struct_bytes;
  int32_t n_samples;              /* S */
  int32_t n_rows;                 /* N */
  int32_t n_classes;              /* C */
  int32_t max_configs;
  int32_t n_chosen;               /* extend: n, the rows chosen so far, the winner included */
  uint32_t round;                 /* extend: the acquisition round, word 1 of the label stream's counter (<< 8) */
  uint32_t last;                  /* extend: nonzero = the last row of a batch: only *base and batch_scores are written */
  uint64_t seed;
  const float* probs;             /* device [S, N, C] */
  const double* cond;             /* device [N] */
  const int32_t* labelled;        /* device [N]: bnn_acquire_topk's list */
  const int32_t* n_labelled;      /* device word */
  const double* scores64;         /* optional device [N]: the step's bnn_batchbald_joint scores */
  const float* phat_in;           /* device [M(n - 1), S] */
  const int32_t* expo_in;         /* device [M(n - 1)] */
  float* phat_out;                /* device [M(n), S] */
  int32_t* expo_out;              /* device [M(n)] */
  double* weight;                 /* device [M(n)] */
  double* offset;                 /* device [M(n)] */
  double* base;                   /* device word */
  double* batch_scores;           /* optional device [>= n] */
} bnn_batchbald_state_args;
int32_t bnn_batchbald_configs(int32_t n_classes, int32_t n_chosen, int32_t max_configs);
size_t bnn_batchbald_joint_workspace_bytes(int32_t n_rows, int32_t n_classes, int32_t n_configs);
int bnn_batchbald_probs(const bnn_batchbald_probs_args* args, void* stream);
int bnn_batchbald_joint(const bnn_batchbald_joint_args* args, void* stream);
int bnn_batchbald_begin(const bnn_batchbald_state_args* args, void* stream);
int bnn_batchbald_extend(const bnn_batchbald_state_args* args, void* stream);

/* ------------------------------------------------------------------------------------
 * F16  Flipout (Wen, Vicol, Ba, Tran, Grosse, ICLR 2018): the third estimator of a factorised Gaussian posterior, beside
 * weight sampling (K1) and local reparameterisation (K3).  One BASE DRAW Delta = sigma o eps per layer is seen by every batch
 * row through its own rank-one sign pattern, W_n = mu + Delta o (s_n r_n^T): two dense products give each row of the minibatch
 * its own, marginally exact, weight sample.  Weights are [out, in] (the BayesianLinear layout).  A call evaluates S = n_samples
 * MC samples from D = n_draws base draws, D | S; sample s belongs to draw d = s / (S / D); the global index of sample s is
 * g_s = sample_offset + *sample_counter + s (sample groups as in K1).
 *
 * Base draw.  eps_d [out, in] and eps_b,d [out] are the kind-0 and kind-1 epsilon maps of this layer (top of this file) at the
 *   global index of the FIRST sample of block d -- with D = S every sample draws exactly the epsilon K1 draws for it.
 *   sigma = softplus(rho) (bnn_softplus's bits), Delta_d = fl32(sigma * eps_d), b_d = fmaf(b_sigma, eps_b,d, b_mu): the bias is
 *   not flipped.
 * Signs.  A sign tensor of logical shape [rows, cols]; kind 0: the input signs r (cols = in), kind 1: the output signs s
 *   (cols = out):
 *       group = (row_offset + row) * ceil(cols / 128) + (col >> 7)                  (uint32)
 *       (w0, w1, w2, w3) = Philox4x32-R((group, g_s, 4 * layer_id + kind, 2), key = (seed_lo, seed_hi))
 *       b = col & 127;   sign[row, col] = -1 iff bit (b & 31) of w_(b >> 5) is set, else +1
 *   Counter word 3 = 2: every epsilon stream has word 3 = 0, the bandit / epoch / acquisition / BatchBALD streams word 3 = 1, so
 *   no existing stream moved and BNN_EPS_MAP_VERSION stays 2.  row_offset makes the signs of a batch independent of how it is
 *   cut into calls; they depend on neither tiling nor S.  bnn_flipout_signs materialises the map (tests and tools).
 * Forward.  y[s, n, o] = act( sum_k x[n, k] mu[o, k]  +  s[s, n, o] * sum_k (x[n, k] r[s, n, k]) Delta_d[o, k]  +  b_d[o] ).
 *   Sign flips are sign-bit XORs, never multiplies.  BNN_EPS_ZERO: y = act(x mu^T + b_mu).
 * ELBO terms.  log_q[d], log_prior[d] are evaluated at the base draw w = fmaf(sigma, eps_d, mu) and b_d, from fp32 block
 *   partials {sum eps^2, sum w^2 | sum log p_mix(w), sum log sigma} folded in fp64 as bnn_elbo_finalize folds K1's: unbiased,
 *   since every row's marginal is that distribution.
 * Backward.  gz = gy o (y > 0) where ReLU applies;  G = sum_{s,n} gz^T x;  H_d = sum_{s in d, n} (gz o s)^T (x o r);
 *   t_d = H_d + g_log_prior[d] dlogp/dw(mu + Delta_d);   g_mu = G + sum_d g_log_prior[d] dlogp/dw(mu + Delta_d);
 *   g_rho = (sum_d t_d o eps_d - (sum_d g_log_q[d]) / sigma) sigmoid(rho);  the bias likewise from the row sums of gz (not
 *   flipped);  g_x = gz mu + ((gz o s) Delta_d) o r.
 *
 * bnn_flipout_prepare   everything that depends on no activation, one read of (mu, rho) for all D draws: delta [D, out, in]
 *     fp32, b_draw [D, out], with BNN_MATH_BF16 also delta_bf16 [D, out, in] and mu_bf16 [out, in] (RNE), with want_stats
 *     log_prior[D] / log_q[D], and optionally the epsilon used (eps_w_dump [D, out, in], eps_b_dump [D, out]: what
 *     bnn_flipout_bwd reads).  eps_mode: BNN_EPS_PHILOX, BNN_EPS_MEMORY (eps_w [D, out, in], eps_b [D, out]) or BNN_EPS_ZERO.
 *     Workspace (want_stats): bnn_flipout_prepare_workspace_bytes(D, in, out), 8-byte aligned, any contents.
 *   Errors, in this order: args NULL: BNN_ERR_NULL; struct_bytes: BNN_ERR_ABI; S, D < 1, S % D != 0, in / out outside
 *   [1, BNN_FLIPOUT_MAX_FEATURES], Gaussian sigma_p or a mixture sigma <= 0: BNN_ERR_SHAPE; eps_mode, math (BNN_MATH_BF16X3 is
 *   refused: use bf16 or f32), prior kind: BNN_ERR_ENUM; w_mu, w_rho, b_mu, b_rho, delta, b_draw, (MEMORY) eps_w, eps_b, (bf16)
 *   delta_bf16, mu_bf16, (want_stats) log_prior, log_q NULL: BNN_ERR_NULL; workspace NULL or short with want_stats:
 *   BNN_ERR_WORKSPACE; an fp32 pointer not 4-byte, a bf16 pointer not 2-byte, the workspace not 8-byte aligned: BNN_ERR_ALIGN.
 *
 * bnn_flipout_fwd   the layer on the matrix core: v_mfma_f32_16x16x4_f32 (BNN_MATH_F32, x and y fp32) or
 *     v_mfma_f32_16x16x32_bf16 (BNN_MATH_BF16: mu_bf16 / delta_bf16, x fp32 or bf16 -- rounded RNE as it is staged --, y fp32 or
 *     bf16), operands staged through LDS, two fp32 accumulator tiles per output tile (mean and perturbation).  r is XORed into
 *     the staged x tile, s into the perturbation accumulator before it joins the mean accumulator; then bias, ReLU, store.
 *     x [x_rows, batch, in], x_rows = 1 (x_per_sample = 0: x mu^T is computed once per block and shared by the samples the
 *     block walks) or S (x_per_sample = 1).  y [S, batch, out].  BNN_EPS_ZERO: delta is not read, b_draw = b_mu, S = D = 1.
 *     One fixed summation order per shape: ascending k inside each accumulator, then mean + perturbation + bias.
 *   Errors, in this order: NULL args; ABI; S, D, batch < 1, S % D != 0, in / out outside [1, BNN_FLIPOUT_MAX_FEATURES],
 *   x_per_sample not 0 / 1, (BNN_EPS_ZERO) S != 1: BNN_ERR_SHAPE; math (BF16X3 refused), eps_mode, x_dtype, y_dtype (fp32 only
 *   in BNN_MATH_F32): BNN_ERR_ENUM; x, y, b_draw, (f32) w_mu, (bf16) mu_bf16, and unless BNN_EPS_ZERO delta / delta_bf16 NULL:
 *   BNN_ERR_NULL; misaligned (element size) pointers: BNN_ERR_ALIGN.
 *
 * bnn_flipout_bwd   exact fp32, no float atomics, one fixed summation order per shape (rows in ascending (s, n) order per
 *     weight; a repeated call gives the same bits).  Three launches: (1) gz, gz o s and x o r into the workspace; (2) one
 *     thread per weight: G, H_d for d = 0 .. D-1 in turn, the prior / posterior terms and the rho chain, and per output the
 *     bias gradients; (3) with g_x: the input gradient [S, batch, in] (sum it over S where x_per_sample = 0).  eps_w / eps_b are
 *     the forward's epsilon as bnn_flipout_prepare dumped it (D |W| floats kept between forward and backward instead of a
 *     second pass of the generator); Delta_d = fl32(sigma * eps_d) is re-formed from them.  g_log_prior / g_log_q: optional [D].
 *     gx_relu_mask is not offered: the previous layer's backward applies its own ReLU mask through `y`.
 *     Workspace: bnn_flipout_bwd_workspace_bytes(S, batch, in, out), 4-byte aligned, any contents.
 *   Errors, in this order: NULL args; ABI; S, D, batch < 1, S % D != 0, in / out outside the limits, x_per_sample not 0 / 1, a
 *   prior sigma <= 0: BNN_ERR_SHAPE; prior kind: BNN_ERR_ENUM; x, gy, w_mu, w_rho, b_mu, b_rho, eps_w, eps_b, g_w_mu, g_w_rho,
 *   g_b_mu, g_b_rho, (relu) y NULL: BNN_ERR_NULL; workspace NULL or short: BNN_ERR_WORKSPACE; a pointer not 4-byte aligned:
 *   BNN_ERR_ALIGN.
 *
 * bnn_flipout_signs   out[n_samples, rows, cols] int8 = +1 / -1, sample i at global index sample_offset + i.
 *   Errors, in this order: NULL args; ABI; n_samples, rows, cols < 1: BNN_ERR_SHAPE; kind not 0 / 1: BNN_ERR_ENUM; out NULL.
 * ---------------------------------------------------------------------------------- */
#define BNN_FLIPOUT_MAX_FEATURES 16384   /* in / out features of a Flipout layer */
/* layout: 8 x 4-byte words, uint64, pointer */
typedef struct bnn_flipout_signs_args {
  uint32_t struct_bytes;
  int32_t n_samples, rows, cols;
  int32_t kind;                   /* 0: r (input signs), 1: s (output signs) */
  uint32_t layer_id;
  uint32_t sample_offset, row_offset;
  uint64_t seed;
  int8_t* out;                    /* device [n_samples, rows, cols] */
} bnn_flipout_signs_args;
/* layout: 12 x 4-byte words, uint64, 7 pointers, prior (5 words) + want_stats, 8 pointers, size_t */
typedef struct bnn_flipout_prepare_args {
  uint32_t struct_bytes;
  int32_t n_samples, n_draws;     /* S, D */
  int32_t in_features, out_features;
  int32_t eps_mode, math;
  uint32_t layer_id, sample_offset, sample_group, sample_group_stride;
  int32_t reserved;
  uint64_t seed;
  const uint32_t* sample_counter; /* optional device word (K1) */
  const float* w_mu;
  const float* w_rho;
  const float* b_mu;
  const float* b_rho;
  const float* eps_w;             /* BNN_EPS_MEMORY: [D, out, in] */
  const float* eps_b;             /* BNN_EPS_MEMORY: [D, out] */
  bnn_prior prior;
  int32_t want_stats;
  float* delta;                   /* [D, out, in] */
  float* b_draw;                  /* [D, out] */
  void* delta_bf16;               /* BNN_MATH_BF16: [D, out, in] */
  void* mu_bf16;                  /* BNN_MATH_BF16: [out, in] */
  float* log_prior;               /* want_stats: [D] */
  float* log_q;                   /* want_stats: [D] */
  float* eps_w_dump;              /* optional [D, out, in] */
  float* eps_b_dump;              /* optional [D, out] */
  void* workspace;
  size_t workspace_bytes;
} bnn_flipout_prepare_args;
/* layout: 18 x 4-byte words, uint64, 8 pointers */
typedef struct bnn_flipout_fwd_args {
  uint32_t struct_bytes;
  int32_t n_samples, n_draws;     /* S, D */
  int32_t batch, in_features, out_features;
  int32_t x_dtype, x_per_sample;  /* bnn_dtype; 0: one x for all samples, 1: one per sample */
  int32_t math, eps_mode;
  int32_t relu, y_dtype;
  uint32_t layer_id, sample_offset, sample_group, sample_group_stride;
  uint32_t row_offset;            /* first batch row's index in the sign maps */
  int32_t reserved;
  uint64_t seed;
  const uint32_t* sample_counter;
  const void* x;
  const float* w_mu;              /* BNN_MATH_F32 */
  const float* delta;             /* BNN_MATH_F32: [D, out, in] */
  const void* mu_bf16;            /* BNN_MATH_BF16 */
  const void* delta_bf16;         /* BNN_MATH_BF16 */
  const float* b_draw;            /* [D, out]; BNN_EPS_ZERO: b_mu */
  void* y;                        /* [S, batch, out] */
} bnn_flipout_fwd_args;
/* layout: 14 x 4-byte words, uint64, 10 pointers, prior (5 words) + reserved2, 7 pointers, workspace, size_t */
typedef struct bnn_flipout_bwd_args {
  uint32_t struct_bytes;
  int32_t n_samples, n_draws;
  int32_t batch, in_features, out_features;
  int32_t x_per_sample, relu;
  uint32_t layer_id, sample_offset, sample_group, sample_group_stride;
  uint32_t row_offset;
  int32_t reserved;
  uint64_t seed;
  const uint32_t* sample_counter;
  const float* x;                 /* [x_rows, batch, in] */
  const float* gy;                /* [S, batch, out] */
  const float* y;                 /* relu: the forward's output */
  const float* w_mu;
  const float* w_rho;
  const float* b_mu;
  const float* b_rho;
  const float* eps_w;             /* [D, out, in]: the forward's epsilon */
  const float* eps_b;             /* [D, out] */
  bnn_prior prior;
  int32_t reserved2;
  const float* g_log_prior;       /* optional [D] */
  const float* g_log_q;           /* optional [D] */
  float* g_w_mu;
  float* g_w_rho;
  float* g_b_mu;
  float* g_b_rho;
  float* g_x;                     /* optional [S, batch, in] */
  void* workspace;
  size_t workspace_bytes;
} bnn_flipout_bwd_args;
size_t bnn_flipout_prepare_workspace_bytes(int32_t n_draws, int32_t in_features, int32_t out_features);   /* 0 outside the limits */
size_t bnn_flipout_bwd_workspace_bytes(int32_t n_samples, int32_t batch, int32_t in_features, int32_t out_features);
int bnn_flipout_signs(const bnn_flipout_signs_args* args, void* stream);
int bnn_flipout_prepare(const bnn_flipout_prepare_args* args, void* stream);
int bnn_flipout_fwd(const bnn_flipout_fwd_args* args, void* stream);
int bnn_flipout_bwd(const bnn_flipout_bwd_args* args, void* stream);

/* ------------------------------------------------------------------------------------
 * F17  Diagonal Laplace posterior of MLP / MLP_Dropout (MacKay 1992; Ritter et al. 2018; Daxberger et al. 2021): a Gaussian
 * centred on the trained weights w with precision diag(F) + tau, F the diagonal of the generalised Gauss-Newton matrix (or of
 * the empirical Fisher) of the data term summed over the data set, tau a prior precision chosen by the Laplace estimate of
 * the marginal likelihood.  A mean-field Gaussian: (mu, rho) of a BayesianLinear.  The forward is bnn_dense_fwd (one sample,
 * fp32 outputs, no dropout); these four do the rest.  No float atomics anywhere: the same inputs give the same bits.
 *
 * Virtual rows.  The GGN of softmax cross-entropy is J^T (diag(p) - p p^T) J and diag(p) - p p^T = sum_c p_c (e_c - p)(e_c - p)^T,
 * so data row n contributes C back-propagations with output deltas sqrt(p_c) (e_c - p); a Gaussian likelihood N(z, sigma^2)
 * gives e_c / sigma.  Virtual row r = c * batch + n, R = batch * C rows; the empirical Fisher has R = batch (the gradient of
 * the row's log-likelihood).  For a linear layer the diagonal is a product of squares, and the input x of a data row is shared
 * by its C virtual rows:
 *     F_w[o, i] = sum_n S[n, o] x[n, i]^2,   F_b[o] = sum_n S[n, o],   S[n, o] = sum_c gz[c * batch + n, o]^2
 * -- a K = batch product whatever C.  Only the deltas of the layer below, g_x = gz . W, need all R rows.
 *
 * bnn_laplace_seed — ONE block (as bnn_dense_loss).  From logits [batch, classes]:
 *   BNN_LAPLACE_GGN,       classification: gy[c * batch + n, :] = sqrt(p_nc) (e_c - p_n);  regression: e_c / sigma
 *   BNN_LAPLACE_EMPIRICAL, classification: gy[n, :] = p_n - onehot(y_n);                    regression: (z_n - y_n) / sigma^2
 *   record[0] += sum_n log p(y_n | x_n) (fp64; classification log softmax(z_n)[y_n], regression the Gaussian log density with
 *   its normaliser, summed over the outputs), record[1] += batch: one read-modify-write by the one block, per-thread fp64 sums
 *   of a fixed set of rows met in a fixed-order tree.  target (int64 [batch] | fp32 [batch, classes]) is optional under
 *   BNN_LAPLACE_GGN (record[0] is left alone then).  A label outside [0, classes) makes every delta of its row and record[0]
 *   NaN and never reads out of bounds.
 *   Errors, in this order: args NULL; struct_bytes: BNN_ERR_ABI; batch, classes < 1, sigma not in (0, inf), more than 2^31
 *   deltas: BNN_ERR_SHAPE; loss_mode, curvature: BNN_ERR_ENUM; logits, gy, record, (empirical) target NULL: BNN_ERR_NULL;
 *   alignment (4 bytes; record and int64 labels 8): BNN_ERR_ALIGN.
 *
 * bnn_laplace_layer — one Linear -> [ReLU] group in ONE launch; two products share the grid as in bnn_dense_bwd:
 *   gz   = gy [rows, out]                        (y == NULL), or  y[r mod batch, o] > 0 ? gy : 0  (y [batch, out]: the saved output)
 *   S    = sum_c gz^2: an fmaf chain from 0 in c order; x^2 and gz^2 are formed while staging, no squared copy exists
 *   F_w += S^T . x^2  [out, in] on v_mfma_f32_16x16x4_f32, the accumulator INITIALISED FROM THE STORED F_w: an element is one
 *          fixed chain over every minibatch accumulated; no K-split.  F_b += colsum(S): four strided partial sums per column,
 *          the first starting from the stored F_b, added in bnn_dense_bwd's order.  Always exact fp32.
 *   g_x  = gz . W [rows, in] (optional), times (x[r mod batch, i] > 0) when gx_mask: the deltas of the layer below (x is its
 *          output).  BNN_MATH_BF16: gz and W rounded to bf16 (RNE), fp32 accumulate; other modes exact fp32.
 *   s_out (optional, [batch, out]): S itself, for tests.
 *   rows = batch * C, C >= 1.  Any shape >= 1; 4-byte aligned pointers, 16-byte loads / stores where rows and bases allow.
 *   Errors, in this order: NULL args; ABI; batch, rows, in, out < 1, rows % batch != 0, a matrix over 2^31 elements:
 *   BNN_ERR_SHAPE; math: BNN_ERR_ENUM; x, gy, f_w, (g_x) w NULL: BNN_ERR_NULL; BNN_ERR_ALIGN.
 *
 * bnn_laplace_evidence — log_evidence[g] = loglik - tau_g |w|^2 / 2 + P log(tau_g) / 2 - sum_i log(F_i + tau_g) / 2 for up
 *   to BNN_LAPLACE_MAX_PRECISIONS candidates in one pass over up to BNN_LAPLACE_MAX_TENSORS (parameter, curvature) pairs; P the
 *   number of parameters, loglik = record[0].  fp64 throughout, two stages: a block sums one BNN_LAPLACE_CHUNK of one tensor
 *   (thread t the elements t, t + 256, ...; then a fixed tree), one final block sums the blocks (thread t blocks t, t + 256,
 *   ...; the tree), writes log_evidence [n_precisions] and the maximum: *best_index (the lowest index on ties), best[0] its
 *   value, best[1] its precision -- device words; nothing is read back.  Workspace: bnn_laplace_evidence_workspace_bytes(args)
 *   (0 for arguments the call would refuse), 8-byte aligned, any contents.
 *   Errors, in this order: NULL args; ABI; n_tensors outside [1, BNN_LAPLACE_MAX_TENSORS], n_precisions outside
 *   [1, BNN_LAPLACE_MAX_PRECISIONS], a numel < 1, a precision not in (0, inf): BNN_ERR_SHAPE; a param / curv, record,
 *   log_evidence NULL: BNN_ERR_NULL; workspace NULL or short: BNN_ERR_WORKSPACE; BNN_ERR_ALIGN (fp64 words 8 bytes).
 *
 * bnn_laplace_posterior — for every tensor pair: mu = w (the bits), rho = softplus^-1((F + tau)^-1/2) in ONE launch; tau =
 *   *precision_device (best + 1 of bnn_laplace_evidence) or `precision`.  s = (F + tau)^-1/2 and log(expm1(s)) are formed in
 *   fp64 (expm1 keeps the small-sigma end: rho -> log s; s > 40: rho = s, where exp(-s) is below fp64's epsilon), so rho
 *   neither overflows nor loses small sigmas; finite for every F >= 0.
 *   Errors, in this order: NULL args; ABI; n_tensors, numel, a host precision not in (0, inf): BNN_ERR_SHAPE; a tensor NULL:
 *   BNN_ERR_NULL; BNN_ERR_ALIGN.
 * ---------------------------------------------------------------------------------- */
#define BNN_LAPLACE_MAX_PRECISIONS 64
#define BNN_LAPLACE_MAX_TENSORS 16
#define BNN_LAPLACE_CHUNK 4096           /* consecutive elements of a tensor per block (evidence, posterior) */
#define BNN_LAPLACE_RECORD_DOUBLES 2     /* {sum of log-likelihoods, rows} */
enum bnn_laplace_curvature { BNN_LAPLACE_GGN = 0, BNN_LAPLACE_EMPIRICAL = 1 };

typedef struct bnn_laplace_seed_args {
  uint32_t struct_bytes;
  int32_t batch, classes;
  int32_t loss_mode;        /* bnn_nll_mode */
  int32_t curvature;        /* bnn_laplace_curvature */
  int32_t reserved;
  double sigma;             /* the Gaussian likelihood's scale (regression) */
  const float* logits;      /* [batch, classes] */
  const void* target;       /* int64 [batch] | fp32 [batch, classes]; optional under BNN_LAPLACE_GGN */
  float* gy;                /* [R, classes] */
  double* record;           /* [BNN_LAPLACE_RECORD_DOUBLES], device */
} bnn_laplace_seed_args;

typedef struct bnn_laplace_layer_args {
  uint32_t struct_bytes;
  int32_t batch, rows, in_features, out_features;
  int32_t math;             /* bnn_math of the g_x product */
  int32_t gx_mask;
  int32_t reserved;
  const float* x;           /* [batch, in] */
  const float* gy;          /* [rows, out] */
  const float* y;           /* optional [batch, out] */
  const float* w;           /* [out, in]; read for g_x only */
  float* f_w;               /* [out, in], accumulated */
  float* f_b;               /* optional [out], accumulated */
  float* g_x;               /* optional [rows, in] */
  float* s_out;             /* optional [batch, out] */
} bnn_laplace_layer_args;

typedef struct bnn_laplace_evidence_args {
  uint32_t struct_bytes;
  int32_t n_tensors, n_precisions;
  int32_t reserved;
  const float* param[BNN_LAPLACE_MAX_TENSORS];
  const float* curv[BNN_LAPLACE_MAX_TENSORS];
  int64_t numel[BNN_LAPLACE_MAX_TENSORS];
  double precision[BNN_LAPLACE_MAX_PRECISIONS];
  const double* record;
  void* workspace;
  size_t workspace_bytes;
  double* log_evidence;     /* [n_precisions] */
  int32_t* best_index;      /* optional device word */
  double* best;             /* optional [2]: the maximum, its precision */
} bnn_laplace_evidence_args;

typedef struct bnn_laplace_posterior_args {
  uint32_t struct_bytes;
  int32_t n_tensors;
  const float* param[BNN_LAPLACE_MAX_TENSORS];
  const float* curv[BNN_LAPLACE_MAX_TENSORS];
  float* mu[BNN_LAPLACE_MAX_TENSORS];
  float* rho[BNN_LAPLACE_MAX_TENSORS];
  int64_t numel[BNN_LAPLACE_MAX_TENSORS];
  double precision;               /* host value; ignored with precision_device */
  const double* precision_device; /* optional */
} bnn_laplace_posterior_args;

size_t bnn_laplace_evidence_workspace_bytes(const bnn_laplace_evidence_args* args);
int bnn_laplace_seed(const bnn_laplace_seed_args* args, void* stream);
int bnn_laplace_layer(const bnn_laplace_layer_args* args, void* stream);
int bnn_laplace_evidence(const bnn_laplace_evidence_args* args, void* stream);
int bnn_laplace_posterior(const bnn_laplace_posterior_args* args, void* stream);

/* ------------------------------------------------------------------------------------
 * F18  The linearised (GLM) predictive of the F17 posterior (Immer et al. 2021): with theta ~ N(theta*, diag(s^2)),
 * s^2_p = 1 / (F_p + tau), the output of the network linearised at theta*, f(x, theta*) + J(x)(theta - theta*), is Gaussian
 * with mean f(x_n, theta*) and covariance J diag(s^2) J^T.  For a chain of Linear -> [ReLU] groups that is, layer by layer,
 *     Cov[n, c, c'] = sum_l sum_o gz_l[c, n, o] gz_l[c', n, o] V_l[n, o],   V_l[n, o] = sum_i a_l[n, i]^2 s^2_w,l[o, i] + s^2_b,l[o]
 * a_l the layer's input, gz_l[c, n, :] = d f_c(x_n) / d z_l the deltas of virtual row c * batch + n: the recursion of
 * bnn_laplace_layer's g_x product started from bnn_laplace_seed in regression mode, BNN_LAPLACE_GGN, sigma = 1, target NULL
 * (gy[c * batch + n, k] = delta_kc).  Cov >= min_o s^2_b,last[o] I (the last layer's bias term), so it is positive definite
 * for every finite (F, tau).  No float atomics anywhere: the same inputs give the same bits.
 *
 * The variance rule.  s^2 = fl32(1.0 / ((double)F + tau)): the stored fp32 curvature widened, ONE fp64 add of tau (a host
 * double, or *precision_device = best + 1 of bnn_laplace_evidence), ONE fp64 IEEE division, rounded once to fp32 (RNE).  It
 * is formed while the operand is staged (weights) or in the epilogue (biases); no variance tensor exists.
 *
 * bnn_laplace_glm_layer — one Linear -> [ReLU] group in ONE launch; two item kinds share the grid:
 *   g_x  (optional; blocks [0, tiles_x)): bnn_laplace_layer's g_x = gz . W tiles, the same device code, the same bits.
 *   V    [batch, out] = x^2 . (s^2_w)^T, K = in, 64 x 64 tiles on v_mfma_f32_16x16x4_f32 (always exact fp32), x^2 and s^2_w
 *        formed while staging; then V = fl32(acc + s^2_b[o]).  v_out (optional, [batch, out]): V itself, for tests.
 *   cov_part[tile_o, n, pair] for the tile's data rows n and the pairs c <= c' (pair = c' (c' + 1) / 2 + c, C (C + 1) / 2 of
 *        them): s = 0; for o in the tile's columns, ascending: s = fmaf(fl32(gy[c B + n, o] * gy[c' B + n, o]), V[n, o], s),
 *        the term of a column with y[n, o] <= 0 (y given) LEFT OUT, not multiplied by zero -- so a non-finite V[n, o]
 *        reaches exactly the rows whose unit o is active.  One fixed chain per partial; [ceil(out / 64), batch, pairs] fp32.
 *   rows = batch * C, 1 <= C <= BNN_LAPLACE_GLM_MAX_CLASSES.
 *   Errors, in this order: NULL args; ABI; batch, rows, in, out < 1, rows % batch != 0, C > BNN_LAPLACE_GLM_MAX_CLASSES, a
 *   matrix over 2^31 elements, a host precision not in (0, inf) without precision_device: BNN_ERR_SHAPE; math: BNN_ERR_ENUM;
 *   x, gy, f_w, f_b, cov_part, (g_x) w NULL: BNN_ERR_NULL; BNN_ERR_ALIGN (4 bytes; precision_device 8).
 *
 * bnn_laplace_glm_finish — a block per 8 data rows: a thread per (row, pair) for the sums, then a thread per row.  In fp64:
 *   a[pair] = sum over the layers in list order, over each layer's tiles ascending, of cov_part (one fixed chain).  cov [batch, C, C] = fl32(a), symmetric; var [batch, C] its diagonal;
 *   chol [batch, C, C] the lower Cholesky factor of a, computed in fp64 (no pivoting: see above), rounded once to fp32, zeros
 *   above the diagonal.  A pivot that is not > 0 (non-finite inputs only) makes the row's whole lower triangle NaN.
 *   BNN_NLL_CLASSIFICATION: probs = softmax(mean / sqrt(1 + pi / 8 var)) (MacKay's probit approximation; fp64 from a, rounded
 *   once), preds = argmax of the fp32 probs (int64, the lowest index on ties; 0 for a NaN row), entropy = -sum p log p (fp64
 *   of the unrounded p).  BNN_NLL_REGRESSION: predictive_variance = var + sigma^2, quantiles [n_quantiles, batch, C] = mean +
 *   z[q] sqrt(var) with z[q] = Phi^-1(level q) from the host (fp64; -inf / +inf at levels 0 / 1).  sample_counter (optional):
 *   thread 0 of block 0 adds n_samples; no block of this launch reads it (bnn_dense_fwd's rule).
 *   Errors, in this order: NULL args; ABI; batch < 1, classes outside [1, BNN_LAPLACE_GLM_MAX_CLASSES], n_layers outside
 *   [1, BNN_LAPLACE_GLM_MAX_LAYERS], a tiles < 1, n_quantiles outside [0, BNN_PREDICTIVE_MAX_QUANTILES], n_samples < 0, more
 *   than 2^31 covariance entries, (regression) sigma not in (0, inf) or a NaN z: BNN_ERR_SHAPE; mode: BNN_ERR_ENUM; a
 *   cov_part, mean, cov, var, chol, (n_quantiles > 0) quantiles NULL: BNN_ERR_NULL; BNN_ERR_ALIGN (4 bytes; preds 8).
 *
 * bnn_laplace_glm_sample — logits [n_samples, batch, C]: f[s, n, c] = mean[n, c] + sum_{j <= c} chol[n, c, j] z_j as an fmaf
 *   chain in j order starting from the mean.  z = eps[s, n, :] from the epsilon generator above on its own stream: counter
 *   words 2 and 3 are (5, 1) -- every eps counter's word 3 is 0 and the word-3 = 1 streams use words 2 = 0..4, so no existing
 *   stream moved and BNN_EPS_MAP_VERSION stays 2.  Element (n, j) of global sample g: counter = (n * ceil(C / 4) + (j >> 2),
 *   g, 5, 1), slot j & 3; g = sample_base + (*sample_counter - n_samples, when a counter is given) + s (uint32 arithmetic).
 *   A pure function of (seed, g, n, j): the grid and the batch size do not enter.
 *   Errors, in this order: NULL args; ABI; n_samples, batch < 1, classes outside [1, BNN_LAPLACE_GLM_MAX_CLASSES], more than
 *   2^31 logits: BNN_ERR_SHAPE; mean, chol, logits NULL: BNN_ERR_NULL; BNN_ERR_ALIGN (4 bytes).
 * ---------------------------------------------------------------------------------- */
#define BNN_LAPLACE_GLM_MAX_CLASSES 16
#define BNN_LAPLACE_GLM_MAX_LAYERS (BNN_LAPLACE_MAX_TENSORS / 2)

typedef struct bnn_laplace_glm_layer_args {
  uint32_t struct_bytes;
  int32_t batch, rows, in_features, out_features;
  int32_t math;             /* bnn_math of the g_x product */
  int32_t gx_mask;
  int32_t reserved;
  double precision;               /* tau, host value; ignored with precision_device */
  const double* precision_device; /* optional */
  const float* x;           /* [batch, in] */
  const float* gy;          /* [rows, out] */
  const float* y;           /* optional [batch, out] */
  const float* w;           /* [out, in]; read for g_x only */
  const float* f_w;         /* [out, in], the curvature (read) */
  const float* f_b;         /* [out] */
  float* g_x;               /* optional [rows, in] */
  float* cov_part;          /* [ceil(out / 64), batch, C (C + 1) / 2] */
  float* v_out;             /* optional [batch, out] */
} bnn_laplace_glm_layer_args;

typedef struct bnn_laplace_glm_finish_args {
  uint32_t struct_bytes;
  int32_t batch, classes, n_layers;
  int32_t mode;             /* bnn_nll_mode */
  int32_t n_quantiles;
  int32_t n_samples;        /* added to *sample_counter */
  int32_t reserved;
  double sigma;             /* the Gaussian likelihood's scale (regression) */
  double z[BNN_PREDICTIVE_MAX_QUANTILES];                  /* Phi^-1 of the quantile levels */
  const float* cov_part[BNN_LAPLACE_GLM_MAX_LAYERS];
  int32_t tiles[BNN_LAPLACE_GLM_MAX_LAYERS];               /* ceil(out / 64) of each layer */
  const float* mean;        /* [batch, classes]: the network's output */
  float* cov;               /* [batch, classes, classes] */
  float* var;               /* [batch, classes] */
  float* chol;              /* [batch, classes, classes] */
  float* probs;             /* optional [batch, classes]   (classification) */
  int64_t* preds;           /* optional [batch] */
  float* entropy;           /* optional [batch] */
  float* predictive_variance; /* optional [batch, classes] (regression) */
  float* quantiles;         /* [n_quantiles, batch, classes] */
  uint32_t* sample_counter; /* optional device word */
} bnn_laplace_glm_finish_args;

typedef struct bnn_laplace_glm_sample_args {
  uint32_t struct_bytes;
  int32_t n_samples, batch, classes;
  uint64_t seed;
  uint32_t sample_base;
  int32_t reserved;
  const float* mean;        /* [batch, classes] */
  const float* chol;        /* [batch, classes, classes] */
  float* logits;            /* [n_samples, batch, classes] */
  const uint32_t* sample_counter; /* optional device word */
} bnn_laplace_glm_sample_args;

int bnn_laplace_glm_layer(const bnn_laplace_glm_layer_args* args, void* stream);
int bnn_laplace_glm_finish(const bnn_laplace_glm_finish_args* args, void* stream);
int bnn_laplace_glm_sample(const bnn_laplace_glm_sample_args* args, void* stream);

/* ------------------------------------------------------------------------------------
 * F19  stochastic-gradient MCMC for MLP / MLP_Dropout (not in the reference: SGLD, Welling & Teh 2011; SGHMC, Chen et al. 2014;
 * the cyclical schedule of Zhang et al. 2020) and a device-resident bank of weight snapshots that predicts as an ensemble.
 *
 * The SG-MCMC noise stream.  Element i of parameter tensor t (its index in the launch's tensor list, 0 ..
 *   BNN_SGMCMC_MAX_TENSORS - 1) at chain step k:
 *       counter = (i >> 2, k, t, 3), key = (seed_lo, seed_hi), slot i & 3 by the map's Box-Muller (top of this file)
 *   Counter word 3 = 3: every epsilon stream has word 3 = 0, the bandit / epoch / acquisition / BatchBALD / GLM streams word
 *   3 = 1 and Flipout's signs word 3 = 2, so no existing stream moved and BNN_EPS_MAP_VERSION stays 2.  A pure function of
 *   (seed, k, t, i): the other tensors of the launch and the grid do not enter.
 * bnn_sgmcmc_noise — the stream materialised, out[i] for i < numel (for tests; the sampler never reads it).
 *   Errors: out NULL: BNN_ERR_NULL; numel outside [1, 2^34] or tensor >= BNN_SGMCMC_MAX_TENSORS: BNN_ERR_SHAPE; BNN_ERR_ALIGN.
 *
 * bnn_sgmcmc_step — one sampler step over up to BNN_SGMCMC_MAX_TENSORS fp32 tensors in ONE launch.  With k the value of the
 *   device word *step before the launch and (a, b, c, flag) = table[k % table_rows], every element does, in fp32 with the
 *   fused multiply-adds written out,
 *       g  = fma(grad_scale, grad, tau * p)        grad: of the SUM loss over the minibatch; grad_scale = N_data / batch
 *       v' = fma(c, eps, fma(-a, g, b * v))        v = 0 and v' not stored when momentum[0] == NULL
 *       p' = p + v'
 *   SGLD is the table a = lr / 2, b = 0, c = sqrt(lr T) without momentum; SGHMC a = lr, b = 1 - alpha, c = sqrt(2 alpha lr T).
 *   The host builds the table in fp64 and rounds once; no transcendental of the rule runs on the device.  eps by eps_mode:
 *   BNN_EPS_PHILOX the stream above at step k, BNN_EPS_MEMORY noise[t][i], BNN_EPS_ZERO 0.
 *   Every block reads *step before its update; the block that arrives last stores k + 1 (the ticketed hand-off of
 *   bnn_adam_step; ticket: 16 zeroed uint32 words, left zeroed).  No tick launch, no float atomics.
 *   The bank (optional): fp32 [capacity, stride], stride = sum_t round_up(numel[t], 64); element i of tensor t of member m at
 *   bank[m * stride + off_t + i], off_t = sum_{u < t} round_up(numel[u], 64).  When k >= burn_in and flag != 0 every thread
 *   also stores p' into member *collected % capacity (*collected read before the update), and the last block advances
 *   *collected with *step: a ring that overwrites its oldest member; the padding words are never written.
 *   Errors, in this order: NULL args; ABI; n_tensors outside [1, BNN_SGMCMC_MAX_TENSORS], table_rows < 1, (bank) capacity < 1, a
 *   numel outside [1, 2^34]: BNN_ERR_SHAPE; eps_mode: BNN_ERR_ENUM; table, step, ticket, (bank) collected, a param, a grad, a
 *   momentum when momentum[0] is given (or one given when it is not), (BNN_EPS_MEMORY) a noise NULL: BNN_ERR_NULL; BNN_ERR_ALIGN
 *   (tensors, table and bank 16 bytes, words 4).
 *
 * bnn_bank_fwd — one Linear -> [ReLU] layer for `members` members of a bank in ONE launch:
 *       y[j] = act(x[j or shared] . W[first + j]^T + b[first + j]),   j < members
 *   W[m] = w + m * w_stride ([out, in] fp32), b[m] = b + m * b_stride (fp32 [out]; b may be NULL); x [batch, in] shared by the
 *   members (x_shared = 1: layer 1) or [members, batch, in]; y [members, batch, out].  x and y fp32 or bf16 by bnn_dense_fwd's
 *   rules (bf16 only in BNN_MATH_BF16).  One block owns a 64 x 64 tile of ONE member's batch x out problem; a row tile never
 *   straddles two members.  An output element is bnn_dense_fwd's chain: 32-wide k stages in order, v_mfma_f32_16x16x32_bf16
 *   per stage in bf16 math, eight v_mfma_f32_16x16x4_f32 in exact-fp32 math, accumulators from zero, then + b, then max(., 0)
 *   -- member j's output is bit-equal to bnn_dense_fwd on (x[j], W[first + j], b[first + j]) with n_samples = 1, drop_p = 0.
 *   Members outside [first, first + members) are not read.
 *   Errors, in this order: NULL args; ABI; members, batch, in_features, out_features < 1, first < 0, a negative stride, more
 *   than 2^30 tiles: BNN_ERR_SHAPE; math, dtypes, bf16 activations outside BNN_MATH_BF16: BNN_ERR_ENUM; x, w, y NULL:
 *   BNN_ERR_NULL; BNN_ERR_ALIGN (element size).
 * ---------------------------------------------------------------------------------- */
#define BNN_SGMCMC_MAX_TENSORS 16
#define BNN_SGMCMC_TABLE_COLS 4           /* a, b, c, collect flag */

typedef struct bnn_sgmcmc_args {
  uint32_t struct_bytes;
  int32_t n_tensors;
  float* param[BNN_SGMCMC_MAX_TENSORS];
  const float* grad[BNN_SGMCMC_MAX_TENSORS];
  float* momentum[BNN_SGMCMC_MAX_TENSORS];       /* all NULL: no momentum buffer (SGLD) */
  const float* noise[BNN_SGMCMC_MAX_TENSORS];    /* BNN_EPS_MEMORY */
  int64_t numel[BNN_SGMCMC_MAX_TENSORS];
  float grad_scale, tau;
  int32_t eps_mode;         /* bnn_eps_mode */
  int32_t table_rows;       /* L */
  const float* table;       /* device [L, BNN_SGMCMC_TABLE_COLS] */
  uint64_t seed;
  uint32_t* step;           /* device word k */
  uint32_t* collected;      /* device word; with a bank */
  uint32_t* ticket;         /* 16 device words, zero between launches */
  uint32_t burn_in;
  int32_t capacity;         /* members of the bank */
  float* bank;              /* optional [capacity, stride] */
} bnn_sgmcmc_args;

typedef struct bnn_bank_fwd_args {
  uint32_t struct_bytes;
  int32_t members, first, batch, in_features, out_features;
  int32_t x_shared;         /* 1: x [batch,in] for all members; 0: x [members,batch,in] */
  int32_t relu;
  const void* x;
  int32_t x_dtype;          /* bnn_dtype */
  int32_t math;             /* bnn_math */
  const float* w;           /* member m's [out,in] at w + m * w_stride */
  const float* b;           /* member m's [out] at b + m * b_stride, or NULL */
  int64_t w_stride, b_stride;
  void* y;                  /* [members,batch,out] */
  int32_t y_dtype;          /* bnn_dtype */
  int32_t reserved;
} bnn_bank_fwd_args;

int bnn_sgmcmc_noise(float* out, uint64_t seed, uint32_t tensor, uint32_t step, int64_t numel, void* stream);
int bnn_sgmcmc_step(const bnn_sgmcmc_args* args, void* stream);
int bnn_bank_fwd(const bnn_bank_fwd_args* args, void* stream);

/* ------------------------------------------------------------------------------------
 * F20  Kronecker-factored (KFAC) Laplace posterior of MLP / MLP_Dropout (Martens & Grosse 2015; Ritter et al. 2018; Immer et
 * al. 2021): the posterior family that keeps the correlations inside a layer.  Per layer, weight W [out, in] and bias b taken
 * jointly as Wbar = [W | b] [out, in + 1], abar_n = [a_n ; 1] the homogeneous input of data row n, gz the masked deltas of the
 * virtual rows (F17's, seeded by bnn_laplace_seed: r = c * batch + n), summed over every accumulated minibatch:
 *     A = sum_n a_n a_n^T [in, in],   s = sum_n a_n [in],   G = sum_r gz_r gz_r^T [out, out],   N = record[1] (data rows)
 *     Abar = [[A, s], [s^T, N]],      H ~= (Abar (x) G) / N                    (exact for N = 1)
 * Once per fit (on the host side of the ABI: an fp64 symmetric eigendecomposition): Abar / N = Q_A diag(lA) Q_A^T,
 * G = Q_G diag(lG) Q_G^T, eigenvalues below 0 set to 0.  In that basis the posterior is diagonal with precisions
 * d_ji = lG_j lA_i + tau.  No float atomics anywhere: the same inputs give the same bits.
 *
 * bnn_kfac_layer — bnn_laplace_layer with the diagonal product replaced by the factors; one Linear -> [ReLU] group in ONE
 *   launch, three item kinds sharing the grid:
 *   gz   = gy [rows, out] (y == NULL), or y[r mod batch, o] > 0 ? gy : 0, formed while staging
 *   a   += x^T x   [in, in],  K = batch;   g += gz^T gz  [out, out],  K = rows: 64 x 64 tiles on v_mfma_f32_16x16x4_f32, always
 *          exact fp32, the accumulator INITIALISED FROM THE STORED FACTOR (one fixed chain per element over every minibatch; no
 *          K-split).  Only tiles with tn <= tm are computed; each is written to both halves from the same registers (a
 *          diagonal tile writes its lower triangle to both), so a factor is bit-symmetric.
 *   s   += colsum(x) [in]: four strided partial sums per column, the first starting from the stored s, added in
 *          bnn_dense_bwd's order.
 *   g_x  = gz . W [rows, in] (optional), times (x[r mod batch, i] > 0) when gx_mask: bnn_laplace_layer's device code, so its
 *          bits; BNN_MATH_BF16 rounds gz and W to bf16, other modes are exact fp32.
 *   Any shape >= 1; every load is bounded by the shape; 4-byte aligned pointers, 16-byte loads / stores where rows and bases
 *   allow.
 *   Errors, in this order: NULL args; ABI; batch, rows, in, out < 1, rows % batch != 0, a matrix over 2^31 elements:
 *   BNN_ERR_SHAPE; math: BNN_ERR_ENUM; x, gy, a, s, g, (g_x) w NULL: BNN_ERR_NULL; BNN_ERR_ALIGN.
 *
 * bnn_kfac_evidence — log_evidence[g] = loglik - tau_g |w|^2 / 2 + P log(tau_g) / 2 - 1/2 sum_l sum_ji log(lG_j lA_i + tau_g)
 *   for up to BNN_LAPLACE_MAX_PRECISIONS candidates over up to BNN_LAPLACE_GLM_MAX_LAYERS layers; P = sum_l out (in + 1),
 *   loglik = record[0], |w|^2 from the parameters.  fp64 throughout, bnn_laplace_evidence's two stages: a block sums one
 *   BNN_LAPLACE_CHUNK of one layer's [out, in + 1] grid (element e: j = e / (in + 1), i = e mod (in + 1), the parameter
 *   beside it W[j, i] or b[j]; thread t the elements t, t + 256, ...; then a fixed tree), one final block sums the blocks and
 *   writes log_evidence, *best_index (the lowest index on ties), best[0] the maximum, best[1] its precision -- device words;
 *   nothing is read back.  Workspace: bnn_kfac_evidence_workspace_bytes(args) (0 for arguments the call would refuse).
 *   Errors, in this order: NULL args; ABI; n_layers outside [1, BNN_LAPLACE_GLM_MAX_LAYERS], n_precisions outside
 *   [1, BNN_LAPLACE_MAX_PRECISIONS], an in / out < 1, a precision not in (0, inf): BNN_ERR_SHAPE; a weight / bias / lambda,
 *   record, log_evidence NULL: BNN_ERR_NULL; workspace NULL or short: BNN_ERR_WORKSPACE; BNN_ERR_ALIGN (fp64 words 8 bytes).
 *
 * The GLM covariance of data row n is cov[c, c'] = sum_l sum_j gt_cj gt_c'j V_nj with gt = g Q_G (g the Jacobian deltas of
 * output c, seeded as F18 does), at = abar Q_A and V_nj = sum_i at_ni^2 / (lG_j lA_i + tau): two launches per layer, then
 * bnn_laplace_glm_finish / bnn_laplace_glm_sample unchanged.
 *
 * bnn_kfac_glm_rotate — ONE launch, three item kinds: g_x tiles (as above, the math mode's), at [batch, in + 1] = abar . Q_A
 *   (K = in + 1; the homogeneous 1 is appended while staging, no padded copy of x exists) and gt [rows, out] = gz . Q_G
 *   (K = out).  The rotations are always exact fp32 (a bf16 eigenvector matrix is not orthogonal to better than 4e-3).
 *   q_a [in + 1, in + 1], q_g [out, out]: eigenvectors in columns.  rows = batch * C, C <= BNN_LAPLACE_GLM_MAX_CLASSES.
 *   Errors, in this order: NULL args; ABI; a dimension < 1, rows % batch != 0, more than BNN_LAPLACE_GLM_MAX_CLASSES virtual
 *   rows per data row, a matrix over 2^31 elements: BNN_ERR_SHAPE; math: BNN_ERR_ENUM; x, gy, q_a, q_g, at, gt, (g_x) w NULL:
 *   BNN_ERR_NULL; BNN_ERR_ALIGN.
 *
 * bnn_kfac_glm_var — ONE launch: 64 x 64 tiles of V [batch, out] = at^2 . D^T (K = in + 1, exact fp32), D_ji =
 *   fl32(1.0 / (lG_j lA_i + tau)) formed while staging from the two fp64 eigenvalue vectors: one fp64 fma, one fp64 division,
 *   rounded once.  tau = *precision_device or `precision`.  The epilogue sums gt_c gt_c' V over the tile's columns for every
 *   pair c <= c' of a data row, one fixed fmaf chain per partial: cov_part [ceil(out / 64), batch, C (C + 1) / 2] in the layout
 *   bnn_laplace_glm_finish reads (pair = c' (c' + 1) / 2 + c).  v_out (optional, [batch, out]): V itself, for tests.
 *   Errors, in this order: NULL args; ABI; a dimension < 1, rows % batch != 0, more than BNN_LAPLACE_GLM_MAX_CLASSES virtual
 *   rows per data row, a matrix over 2^31 elements, a host precision not in (0, inf): BNN_ERR_SHAPE; at, gt, lambda_a,
 *   lambda_g, cov_part NULL: BNN_ERR_NULL; BNN_ERR_ALIGN (fp64 words 8 bytes).
 *
 * bnn_kfac_sample — matrix-normal weight draws of one layer for `members` bank members, TWO launches:
 *   T_m    = (E_m o Sigma) . Q_A^T [out, in + 1] (K = in + 1), Sigma_ji = fl32((lG_j lA_i + tau)^-1/2) formed in fp64 and the
 *            noise formed while staging: element e = j (in + 1) + i of Wbar draws from the Philox counter (e >> 2, global sample
 *            index sample_base + m, layer, 4), key = seed, slot e & 3, through the epsilon map's Box-Muller (counter word 3:
 *            0 .. 3 are taken -- the epsilon streams, the bandit / epoch / acquisition / GLM streams, Flipout's signs and
 *            SG-MCMC's noise).  BNN_EPS_MAP_VERSION stays 2: a new stream, no old one moves.
 *   Wbar_m = Wbar + Q_G . T_m (K = out); the epilogue writes the weight columns to bank[(first + m) bank_stride + w_offset +
 *            j in + i] and the bias column to bank[(first + m) bank_stride + b_offset + j]: WeightBank's member layout.
 *   Always exact fp32.  Workspace: bnn_kfac_sample_workspace_bytes(members, in, out) = members out (in + 1) floats (0 for
 *   arguments the call would refuse) -- bounded by the chunk of members a call draws.
 *   Errors, in this order: NULL args; ABI; members, in, out < 1, first or a bank offset < 0, a matrix over 2^31 elements, a
 *   host precision not in (0, inf): BNN_ERR_SHAPE; w, b, q_a, q_g, lambda_a, lambda_g, bank NULL: BNN_ERR_NULL; workspace NULL
 *   or short: BNN_ERR_WORKSPACE; BNN_ERR_ALIGN (fp64 words 8 bytes).
 * ---------------------------------------------------------------------------------- */
typedef struct bnn_kfac_layer_args {
  uint32_t struct_bytes;
  int32_t batch, rows, in_features, out_features;
  int32_t math;             /* bnn_math of the g_x product */
  int32_t gx_mask;
  int32_t reserved;
  const float* x;           /* [batch, in] */
  const float* gy;          /* [rows, out] */
  const float* y;           /* optional [batch, out] */
  const float* w;           /* [out, in]; read for g_x only */
  float* a;                 /* [in, in], accumulated */
  float* s;                 /* [in], accumulated */
  float* g;                 /* [out, out], accumulated */
  float* g_x;               /* optional [rows, in] */
} bnn_kfac_layer_args;

typedef struct bnn_kfac_evidence_args {
  uint32_t struct_bytes;
  int32_t n_layers, n_precisions;
  int32_t reserved;
  const float* weight[BNN_LAPLACE_GLM_MAX_LAYERS];     /* [out, in] */
  const float* bias[BNN_LAPLACE_GLM_MAX_LAYERS];       /* [out] */
  const double* lambda_a[BNN_LAPLACE_GLM_MAX_LAYERS];  /* [in + 1] */
  const double* lambda_g[BNN_LAPLACE_GLM_MAX_LAYERS];  /* [out] */
  int32_t in_features[BNN_LAPLACE_GLM_MAX_LAYERS], out_features[BNN_LAPLACE_GLM_MAX_LAYERS];
  double precision[BNN_LAPLACE_MAX_PRECISIONS];
  const double* record;
  void* workspace;
  size_t workspace_bytes;
  double* log_evidence;     /* [n_precisions] */
  int32_t* best_index;      /* optional device word */
  double* best;             /* optional [2]: the maximum, its precision */
} bnn_kfac_evidence_args;

typedef struct bnn_kfac_glm_rotate_args {
  uint32_t struct_bytes;
  int32_t batch, rows, in_features, out_features;
  int32_t math;             /* bnn_math of the g_x product */
  int32_t gx_mask;
  int32_t reserved;
  const float* x;           /* [batch, in] */
  const float* gy;          /* [rows, out] */
  const float* y;           /* optional [batch, out] */
  const float* w;           /* [out, in]; read for g_x only */
  const float* q_a;         /* [in + 1, in + 1] */
  const float* q_g;         /* [out, out] */
  float* at;                /* [batch, in + 1] */
  float* gt;                /* [rows, out] */
  float* g_x;               /* optional [rows, in] */
} bnn_kfac_glm_rotate_args;

typedef struct bnn_kfac_glm_var_args {
  uint32_t struct_bytes;
  int32_t batch, rows, in_features, out_features;
  int32_t reserved[3];
  double precision;               /* host value; ignored with precision_device */
  const double* precision_device; /* optional */
  const float* at;          /* [batch, in + 1] */
  const float* gt;          /* [rows, out] */
  const double* lambda_a;   /* [in + 1] */
  const double* lambda_g;   /* [out] */
  float* cov_part;          /* [ceil(out / 64), batch, C (C + 1) / 2] */
  float* v_out;             /* optional [batch, out] */
} bnn_kfac_glm_var_args;

typedef struct bnn_kfac_sample_args {
  uint32_t struct_bytes;
  int32_t members;          /* draws of this call */
  int32_t first;            /* the bank slot of the first of them */
  int32_t in_features, out_features;
  uint32_t layer;           /* counter word 2 */
  uint32_t sample_base;     /* the global sample index of the first draw */
  int32_t reserved;
  uint64_t seed;
  double precision;               /* host value; ignored with precision_device */
  const double* precision_device; /* optional */
  const float* w;           /* [out, in] */
  const float* b;           /* [out] */
  const float* q_a;         /* [in + 1, in + 1] */
  const float* q_g;         /* [out, out] */
  const double* lambda_a;   /* [in + 1] */
  const double* lambda_g;   /* [out] */
  float* bank;              /* member m's weight at bank[m * bank_stride + w_offset ...], its bias at ... + b_offset */
  int64_t bank_stride, w_offset, b_offset;
  void* workspace;          /* T of the call's members */
  size_t workspace_bytes;
} bnn_kfac_sample_args;

size_t bnn_kfac_evidence_workspace_bytes(const bnn_kfac_evidence_args* args);
size_t bnn_kfac_sample_workspace_bytes(int32_t members, int32_t in_features, int32_t out_features);
int bnn_kfac_sample(const bnn_kfac_sample_args* args, void* stream);
int bnn_kfac_layer(const bnn_kfac_layer_args* args, void* stream);
int bnn_kfac_evidence(const bnn_kfac_evidence_args* args, void* stream);
int bnn_kfac_glm_rotate(const bnn_kfac_glm_rotate_args* args, void* stream);
int bnn_kfac_glm_var(const bnn_kfac_glm_var_args* args, void* stream);

/* ------------------------------------------------------------------------------------
 * F21  Training a deep ensemble (Lakshminarayanan et al. 2017; not in the reference): one K6 training step of ALL `members`
 * members of an F19 weight bank as a fixed chain of launches -- bnn_ens_fwd per layer, bnn_ens_loss, bnn_ens_bwd per layer,
 * then ONE bnn_sgd_step / bnn_adam_step over the bank buffer and the gradient bucket taken as flat tensors of
 * members * stride elements -- whatever `members` is.  Member j's tensor lives at base + (first + j) * stride (the bank:
 * bnn_bank_fwd_args' w / w_stride) or base + j * stride (the gradient bucket [members, stride] in the bank's layout; its padding
 * words are never written).  All three sit on the 64 x 64 tile core of bnn_dense_bwd and bnn_bank_fwd; a block owns one tile of
 * ONE member, work items are dealt to the XCDs in contiguous ranges of the (member, tile) list.  Every activation is fp32.
 *
 * bnn_ens_fwd — the training forward of one Linear -> [ReLU] -> [Dropout] group for all members:
 *       y[j] = drop_j(act(x[j or shared] . W[first + j]^T + b[first + j])),   j < members
 *   x fp32 [batch, in] shared by the members (x_shared = 1) or [members, batch, in]; y fp32 [members, batch, out].  The kind-3
 *   mask of layer layer_id (K5's map) at global sample index sample_offset + *sample_counter + j; drop_p = 0 applies none.
 *   sample_counter_inc is added to *sample_counter by the launch and only allowed with drop_p == 0 (K5's rule: a launch that
 *   increments reads no counter); the output layer's launch of a captured step passes `members`.  Math as bnn_dense_fwd
 *   (BNN_MATH_BF16: operands rounded to bf16 while staged; BNN_MATH_F32 / BNN_MATH_BF16X3: exact fp32).  Member j's output is
 *   bit-equal to bnn_dense_fwd on (x[j], W[first + j], b[first + j]) with n_samples = 1 and sample_offset = that index.
 *   Errors, in this order: NULL args; ABI; members, batch, in_features, out_features < 1, first < 0, layer_id < 0, a negative
 *   stride, drop_p outside [0, 1), sample_counter_inc with drop_p != 0, more than 2^30 tiles: BNN_ERR_SHAPE; math: BNN_ERR_ENUM;
 *   x, w, y NULL, sample_counter NULL with sample_counter_inc: BNN_ERR_NULL; a pointer not 4-byte aligned: BNN_ERR_ALIGN.
 *
 * bnn_ens_loss — bnn_dense_loss for every member, ONE block per member (the same row loop and fixed-order tree: bit-equal
 *   per member): loss[j] and g_logits[j] of logits[j] [batch, classes] against target (target_shared = 1: one int64 [batch] /
 *   fp32 [batch, classes] for all members; 0: [members, ...]).  An out-of-range label makes THAT member's loss and its row's
 *   gradient NaN, reads nothing out of range and leaves the other members untouched.
 *   Errors, in this order: NULL args; ABI; members, batch, classes < 1, batch * classes > 2^31: BNN_ERR_SHAPE; loss_mode:
 *   BNN_ERR_ENUM; logits, target, loss, g_logits NULL: BNN_ERR_NULL; logits / loss / g_logits / fp32 targets not 4-byte, int64
 *   targets not 8-byte aligned: BNN_ERR_ALIGN.
 *
 * bnn_ens_bwd — bnn_dense_bwd for every member in ONE launch over (member, tile): per member the input-gradient tiles
 *   g_x[j] = gz[j] . W[first + j] (optional; the long-K items, ahead of the member's weight-gradient items), g_w[j] = gz[j]^T .
 *   x[j or shared] and g_b[j] = colsum(gz[j]); gz formed on load from gy[j] and (optionally) the saved output y[j], the g_x
 *   mask read off x[j] (the layer below's saved output) -- bnn_dense_bwd's rules and math.  g_w / g_b are member j's tensors at
 *   g_w + j * g_stride / g_b + j * g_stride.  No float atomics, no K-split: every output element is bnn_dense_bwd's fixed
 *   chain, so member j's g_w, g_b and g_x are bit-equal to bnn_dense_bwd on that member's operands whatever `members` and
 *   the grid order.
 *   Errors, in this order: NULL args; ABI; members, batch, in_features, out_features < 1, first < 0, a negative stride, a
 *   product of two dimensions above 2^31, more than 2^30 work items: BNN_ERR_SHAPE; math: BNN_ERR_ENUM; x, gy, w, g_w NULL:
 *   BNN_ERR_NULL; a pointer not 4-byte aligned: BNN_ERR_ALIGN.
 * ---------------------------------------------------------------------------------- */
typedef struct bnn_ens_fwd_args {
  uint32_t struct_bytes;
  int32_t members, first, batch, in_features, out_features;
  int32_t x_shared;         /* 1: x [batch,in] for all members; 0: x [members,batch,in] */
  int32_t relu;
  int32_t math;             /* bnn_math */
  int32_t layer_id;         /* >= 0: the mask's tensor id is 4 * layer_id + 3 */
  const float* x;
  const float* w;           /* member m's [out,in] at w + m * w_stride */
  const float* b;           /* member m's [out] at b + m * b_stride, or NULL */
  int64_t w_stride, b_stride;
  double drop_p;            /* in [0, 1) */
  uint64_t seed;
  uint32_t sample_offset;
  uint32_t sample_counter_inc;
  uint32_t* sample_counter; /* optional DEVICE word */
  float* y;                 /* [members,batch,out] */
} bnn_ens_fwd_args;

typedef struct bnn_ens_loss_args {
  uint32_t struct_bytes;
  int32_t members, batch, classes;
  int32_t loss_mode;        /* bnn_nll_mode */
  int32_t target_shared;    /* 1: one target for all members; 0: a target per member */
  float grad_scale;
  int32_t reserved;
  const float* logits;      /* [members, batch, classes] */
  const void* target;       /* int64 [(members,) batch] or fp32 [(members,) batch, classes] */
  float* loss;              /* [members] (unscaled) */
  float* g_logits;          /* [members, batch, classes] */
} bnn_ens_loss_args;

typedef struct bnn_ens_bwd_args {
  uint32_t struct_bytes;
  int32_t members, first, batch, in_features, out_features;
  int32_t x_shared;         /* 1: x [batch,in] for all members; 0: x [members,batch,in] */
  int32_t math;             /* bnn_math of the g_x product */
  int32_t gx_mask;
  float y_scale;
  float gx_scale;
  int32_t reserved;
  const float* x;
  const float* gy;          /* [members,batch,out] */
  const float* y;           /* optional [members,batch,out] */
  const float* w;           /* member m's [out,in] at w + m * w_stride */
  int64_t w_stride;
  int64_t g_stride;         /* of g_w and g_b */
  float* g_w;               /* member j's [out,in] at g_w + j * g_stride */
  float* g_b;               /* optional: member j's [out] at g_b + j * g_stride */
  float* g_x;               /* optional [members,batch,in] */
} bnn_ens_bwd_args;

int bnn_ens_fwd(const bnn_ens_fwd_args* args, void* stream);
int bnn_ens_loss(const bnn_ens_loss_args* args, void* stream);
int bnn_ens_bwd(const bnn_ens_bwd_args* args, void* stream);

/* ------------------------------------------------------------------------------------
 * F22  SWAG for MLP / MLP_Dropout (Maddox et al. 2019, "A Simple Baseline for Bayesian Uncertainty in Deep Learning"; not in
 * the reference): a Gaussian with a diagonal-plus-low-rank covariance fitted to the iterates of plain SGD.  The tensor list is
 * F19's: up to BNN_SGMCMC_MAX_TENSORS fp32 tensors; the moments (mean [stride], m2 [stride], dev [rank, stride]) hold element i
 * of tensor t at off_t + i, off_t = sum_{u < t} round_up(numel[u], 64), stride = sum_t round_up(numel[t], 64) -- the layout of
 * one member of an F19 bank.  Padding words are never written.
 *
 * bnn_swag_step — one SGD step (torch.optim.SGD, dampening 0, no nesterov; the momentum buffer starts at 0) over all tensors in
 *   ONE launch that also folds the new iterate into the moments when the step collects.  With k = *step and n = *count, both
 *   read before the update, every element does, in fp32 with the fused multiply-adds written out,
 *       g' = weight_decay != 0 ? fma(weight_decay, p, g) : g
 *       u  = momentum[0] != NULL ? (v' = fma(momentum_factor, v, g')) : g'
 *       p' = fma(-lr, u, p)                              lr: *lr_device when given
 *   (without momentum buffers p' is bnn_sgd_step's bits), and when k >= start && (k - start + 1) % every == 0, with
 *   r = 1 / (float)(n + 1) correctly rounded,
 *       d = p' - mean;   mean' = fma(d, r, mean);   m2' = fma(d, p' - mean', m2);   dev[n % rank][i] = p' - mean'   (rank > 0)
 *   Welford's update: m2 / n is the population variance of the collected iterates without the cancellation of
 *   mean(theta^2) - mean(theta)^2; the deviation uses the updated mean, as the paper's does.  rank = 0: no dev (SWAG-Diagonal).
 *   Every block reads *step and *count before its update; the block that arrives last stores k + 1 and, on a collecting step,
 *   n + 1 (the ticketed hand-off of bnn_adam_step; ticket: 16 zeroed uint32 words, left zeroed).  No float atomics, no tick
 *   launch.
 *   Errors, in this order: NULL args; ABI; n_tensors outside [1, BNN_SGMCMC_MAX_TENSORS], rank outside [0, BNN_SWAG_MAX_RANK],
 *   every < 1, a negative or NaN lr / momentum_factor / weight_decay, a numel outside [1, 2^34]: BNN_ERR_SHAPE; step, count,
 *   ticket, mean, m2, (rank > 0) dev, a param, a grad, a momentum when momentum[0] is given (or one given when it is not) NULL:
 *   BNN_ERR_NULL; BNN_ERR_ALIGN (tensors, mean, m2 and dev 16 bytes, words 4).
 *
 * bnn_swag_sample — members first .. first + members - 1 of a bank [capacity, stride] in ONE launch, members <=
 *   BNN_SWAG_MAX_MEMBERS.  With n = *count, Keff = low_rank ? min(n, rank) : 0 and q = sample_base + member index within the
 *   launch, every element does
 *       s     = sqrt(max(m2 * (1 / (float)n), var_clamp))            correctly rounded sqrt and reciprocal (n = 0: 1 / n := 0)
 *       theta = fma(c_d * s, z1, mean)
 *       acc   = 0;  for j = 0 .. Keff - 1 ascending:  acc = fma(dev[j][i], z2[q][j], acc)
 *       theta = fma(c_lr[Keff], acc, theta)                          low_rank only
 *   The host forms c_d (sqrt(scale / 2) with the low-rank term, sqrt(scale) without) and c_lr[e] = sqrt(scale / (2 (e - 1))),
 *   c_lr[0] = c_lr[1] = 0, in fp64 and rounds them once: no transcendental of the rule beyond the one sqrt runs on the device.
 *   The noise, by eps_mode.  BNN_EPS_PHILOX: counter word 3 = 5 (0 eps, 1 bandit / epoch / acquisition / BatchBALD / GLM, 2
 *   Flipout, 3 SG-MCMC, 4 KFAC: no existing stream moved, BNN_EPS_MAP_VERSION stays 2), key = (seed_lo, seed_hi), the map's
 *   Box-Muller: z1 of element i of tensor t from counter (i >> 2, q, t, 5) slot i & 3, z2[q][j] from counter
 *   (j >> 2, q, BNN_SGMCMC_MAX_TENSORS, 5) slot j & 3 -- pure functions of (seed, q, t, i) and (seed, q, j); the launch's other
 *   members, the grid and rank do not enter.  BNN_EPS_MEMORY: z1 [members, stride] in the bank's layout and z2 [members, rank]
 *   (low_rank).  BNN_EPS_ZERO: every member is the mean's bits.
 *   Members outside [first, first + members) and the padding words are not written.
 *   Errors, in this order: NULL args; ABI; n_tensors outside [1, BNN_SGMCMC_MAX_TENSORS], rank outside [0, BNN_SWAG_MAX_RANK],
 *   members outside [1, BNN_SWAG_MAX_MEMBERS], first < 0, capacity < 1, first + members > capacity, low_rank with rank 0, a
 *   negative or NaN var_clamp, a numel outside [1, 2^34]: BNN_ERR_SHAPE; eps_mode: BNN_ERR_ENUM; mean, m2, count, bank,
 *   (low_rank) dev, (BNN_EPS_MEMORY) z1, (BNN_EPS_MEMORY and low_rank) z2 NULL: BNN_ERR_NULL; BNN_ERR_ALIGN (mean, m2, dev, bank
 *   and z1 16 bytes, count and z2 4).
 * ---------------------------------------------------------------------------------- */
#define BNN_SWAG_MAX_RANK 32
#define BNN_SWAG_MAX_MEMBERS 64           /* per launch */

typedef struct bnn_swag_step_args {
  uint32_t struct_bytes;
  int32_t n_tensors;
  float* param[BNN_SGMCMC_MAX_TENSORS];
  const float* grad[BNN_SGMCMC_MAX_TENSORS];
  float* momentum[BNN_SGMCMC_MAX_TENSORS];       /* all NULL: no momentum buffer */
  int64_t numel[BNN_SGMCMC_MAX_TENSORS];
  double lr, momentum_factor, weight_decay;
  const float* lr_device;   /* optional device float: overrides lr */
  uint32_t start, every;    /* collect when k >= start && (k - start + 1) % every == 0 */
  int32_t rank;             /* K: rows of dev */
  int32_t reserved;
  float* mean;              /* [stride] */
  float* m2;                /* [stride] */
  float* dev;               /* [rank, stride]; unread when rank == 0 */
  uint32_t* step;           /* device word k */
  uint32_t* count;          /* device word n */
  uint32_t* ticket;         /* 16 device words, zero between launches */
} bnn_swag_step_args;

typedef struct bnn_swag_sample_args {
  uint32_t struct_bytes;
  int32_t n_tensors;
  int64_t numel[BNN_SGMCMC_MAX_TENSORS];
  int32_t rank, members, first, capacity;
  int32_t low_rank;         /* 1: full SWAG; 0: SWAG-Diagonal */
  int32_t eps_mode;         /* bnn_eps_mode */
  float c_d, var_clamp;
  float c_lr[BNN_SWAG_MAX_RANK + 1];             /* indexed by Keff */
  uint32_t sample_base;
  uint64_t seed;
  const float* mean;
  const float* m2;
  const float* dev;         /* low_rank */
  const uint32_t* count;    /* device word n */
  const float* z1;          /* BNN_EPS_MEMORY: [members, stride] */
  const float* z2;          /* BNN_EPS_MEMORY and low_rank: [members, rank] */
  float* bank;              /* [capacity, stride] */
} bnn_swag_sample_args;

int bnn_swag_step(const bnn_swag_step_args* args, void* stream);
int bnn_swag_sample(const bnn_swag_sample_args* args, void* stream);

/* ------------------------------------------------------------------------------------
 * F23  SVGD (Liu & Wang 2016, "Stein Variational Gradient Descent") and the weight-space repulsive ensemble kde-WGD (D'Angelo &
 * Fortuin 2021, "Repulsive Deep Ensembles are Bayesian"; neither is in the reference): the gradient bucket of F21's step is
 * rewritten in place into a direction in which every member's gradient is mixed with the others' through an RBF kernel matrix
 * and a repulsion term keeps the members apart.  Three launches between the last bnn_ens_bwd and the optimiser's launch; no
 * float atomics, no arrival ticket.
 *
 * Definition.  theta_i = row i of the bank buffer [members, stride] (padding included), g_i = row i of the bucket (the gradient
 * of K6's sum loss), M = members.  With FusedSGMCMC's energy conventions s = dataset_size / (batch_size T) (grad_scale) and
 * tau' = prior_precision / T (tau), grad U_j = s g_j + tau' theta_j:
 *     D2_ij = sum_p (theta_i[p] - theta_j[p])^2                  symmetric, the diagonal exactly 0
 *     med   = the median of all M^2 entries of D2, diagonal included (an even count: the mean of the two middle values)
 *     h     = bandwidth > 0 ? bandwidth : med / log(M + 1);      h == 0 -> h = 1
 *     k_ij  = exp(-D2_ij / h),   r_i = sum_j k_ij  (j ascending)
 *     d     = A g + B theta  per parameter column, the direction the optimiser SUBTRACTS:
 *       BNN_SVGD_SVGD:  A_ij = s k_ij / M                        B_ij = (tau' k_ij + (2 / h)(k_ij - delta_ij r_i)) / M
 *       BNN_SVGD_WGD:   A_ij = s delta_ij                        B_ij = tau' delta_ij - (2 / h)(delta_ij - k_ij / r_i)
 *   so that -d_i = (1 / M) sum_j k_ij [-grad U_j + (2 / h)(theta_i - theta_j)] (SVGD): member i is pushed away from member j.
 *   M = 1 gives A = [s], B = [tau'] exactly in both methods.
 *
 * bnn_svgd_dist — one block per chunk of C = 64 min(BNN_SVGD_CHUNK / 64, ceil(stride / 32768)) columns (whole 64-column tiles,
 *   at most BNN_SVGD_CHUNK; a smaller bank is cut into about 512 chunks so that the chip is filled) writes partials[chunk][pair], pair (i, j), i < j, at index
 *   i (2 M - i - 1) / 2 + (j - i - 1): the fp32 sum over the chunk's columns of fma(d, d, .) with d = theta_i[p] - theta_j[p]
 *   rounded once -- sums of squared differences, never |a|^2 + |b|^2 - 2 a.b.  The longest fp32 addition chain behind a partial
 *   is L = BNN_SVGD_CHAIN = 129: at most 64 columns of a 64-column tile per thread, the tile sums of the chunk's 64 tiles, and
 *   the per-thread sums of up to 64 column lanes in lane order (the three never exceed 129 together).  Every term is
 *   non-negative: a partial is within (L + 2) 2^-24 relative of the exact sum (2 for the rounded difference, squared).
 *   chunks = ceil(stride / C) = bnn_svgd_chunks(stride) (0 for a stride bnn_svgd_dist refuses); members == 1 writes nothing.
 *   Errors, in this order: NULL args; ABI; members outside [1, BNN_SVGD_MAX_MEMBERS], stride < 64, not a multiple of 64 or above
 *   2^34: BNN_ERR_SHAPE; bank, partials NULL: BNN_ERR_NULL; BNN_ERR_ALIGN (bank 16 bytes, partials 4).
 *
 * bnn_svgd_coef — ONE block, fp64 throughout: D2_ij = the chunk partials added in chunk order (with at most 512 pairs the
 *   chunks are split into contiguous ranges whose sums are then added in order); the M^2 entries sorted in LDS, med, h, k, r as above
 *   (log(M + 1) formed on the host in fp64, exp the device's fp64 exp); A and B formed in fp64 by the expressions above as
 *   written and rounded to fp32 ONCE; coef = [A | B], fp32 [M, 2 M] row-major.  record (fp64, BNN_SVGD_RECORD_DOUBLES(M)):
 *   D2 [M, M], med, h, r [M].
 *   Errors, in this order: NULL args; ABI; members outside [1, BNN_SVGD_MAX_MEMBERS], chunks outside [1, 2^22], grad_scale not
 *   in (0, inf), tau or bandwidth (0: the median heuristic) not in [0, inf): BNN_ERR_SHAPE; method: BNN_ERR_ENUM; partials, coef,
 *   record NULL: BNN_ERR_NULL; BNN_ERR_ALIGN (partials, coef 4 bytes, record 8).
 *
 * bnn_svgd_direction — bucket[i][p] <- sum_k coef[i][k] v[k][p], v = [bucket ; bank] ([2 M, stride]), for every column p, in
 *   place, on the exact-fp32 matrix core (v_mfma_f32_16x16x4_f32): per output ONE accumulator that starts at +0 and takes the
 *   2 M products, padded with zeros to a multiple of 16, in ascending k, four per instruction -- |err| <= (2 M + 2) 2^-24
 *   sum_k |coef_ik| |v_kp|.  A wave owns 64 columns and reads all 2 M rows of them before it stores any; the bank is not
 *   written.  Where both operands are zero (the padding columns) the output is exactly zero.
 *   Errors, in this order: NULL args; ABI; members, stride as bnn_svgd_dist: BNN_ERR_SHAPE; coef, bank, bucket NULL:
 *   BNN_ERR_NULL; BNN_ERR_ALIGN (coef 4 bytes, bank and bucket 16).
 * ---------------------------------------------------------------------------------- */
#define BNN_SVGD_MAX_MEMBERS 64
#define BNN_SVGD_CHUNK 4096               /* the most columns per block (and per partial) of bnn_svgd_dist */
#define BNN_SVGD_CHAIN 129                /* L: the longest fp32 addition chain behind a partial */
#define BNN_SVGD_RECORD_DOUBLES(M) ((M) * (M) + (M) + 2)
typedef enum { BNN_SVGD_SVGD = 0, BNN_SVGD_WGD = 1 } bnn_svgd_method;

typedef struct bnn_svgd_dist_args {
  uint32_t struct_bytes;
  int32_t members;
  int64_t stride;           /* of the bank: a multiple of 64 */
  const float* bank;        /* [members, stride] */
  float* partials;          /* [bnn_svgd_chunks(stride), members (members - 1) / 2] */
} bnn_svgd_dist_args;

typedef struct bnn_svgd_coef_args {
  uint32_t struct_bytes;
  int32_t members;
  int32_t chunks;           /* rows of partials */
  int32_t method;           /* bnn_svgd_method */
  double grad_scale;        /* s */
  double tau;               /* tau' */
  double bandwidth;         /* h; 0: the median heuristic */
  const float* partials;
  float* coef;              /* [members, 2 members] */
  double* record;           /* BNN_SVGD_RECORD_DOUBLES(members) */
} bnn_svgd_coef_args;

typedef struct bnn_svgd_direction_args {
  uint32_t struct_bytes;
  int32_t members;
  int64_t stride;
  const float* coef;        /* [members, 2 members] */
  const float* bank;        /* [members, stride] */
  float* bucket;            /* [members, stride], rewritten in place */
} bnn_svgd_direction_args;

int32_t bnn_svgd_chunks(int64_t stride);
int bnn_svgd_dist(const bnn_svgd_dist_args* args, void* stream);
int bnn_svgd_coef(const bnn_svgd_coef_args* args, void* stream);
int bnn_svgd_direction(const bnn_svgd_direction_args* args, void* stream);

/* ------------------------------------------------------------------------------------
 * F24  IVON for MLP / MLP_Dropout (Shen et al. 2024, "Variational Learning is Effective for Large Deep Networks"; not in the
 * reference): natural-gradient variational learning of a diagonal Gaussian N(m, 1 / (ess (h + delta))) per weight at the cost
 * of an Adam step.  The tensor list is F19's (up to BNN_SGMCMC_MAX_TENSORS fp32 tensors); the state (mean, hess, avg_grad, acc_g,
 * acc_h: [stride] each) and the rows of noise / bank hold element i of tensor t at off_t + i in the layout of one member of an
 * F19 bank.  Padding words are never written.  Between steps the parameter tensors hold the mean m.
 *
 * Step t = *step (a uint32 word) runs samples s = 0 .. S - 1: bnn_ivon_draw(s) before sample s's forward / backward pass and
 * bnn_ivon_step after the last.  Host constants, formed in fp64 and rounded once to fp32: ess, delta = weight_decay, beta1,
 * c1 = (1 - beta1) loss_scale / S, cS = loss_scale / S, rho = 1 - beta2, c2 = 0.5 (1 - beta2)^2, clip_radius, lr.  Everything
 * per element is fp32 with the multiply-adds written out; sqrt and / are the correctly rounded ones.
 *       hd = h + delta;   r = sqrt(ess * hd);   sigma = 1 / r                        (draw, fold and step alike)
 *
 * bnn_ivon_draw, training form (bank NULL) — theta of draw q = t * S + sample (uint32, wraps) into the parameter tensors:
 *       m     = sample == 0 ? param : mean;      sample == 0: mean = m  (the mean is filed)
 *       param = fma(sigma, eps_q, m)
 *   and for sample >= 1 the fold of the previous sample's gradient g, er = eps_(q-1) * r:
 *       acc_g = sample == 1 ? g : acc_g + g;     acc_h = sample == 1 ? g * er : fma(g, er, acc_h)
 *   Reads *step, changes no word.  Traffic at S = 1: reads p, h, writes mean, p: 16 B / parameter.
 * bnn_ivon_draw, bank form (bank given) — members first .. first + members - 1 of bank [capacity, stride], members <=
 *   BNN_IVON_MAX_MEMBERS: bank[first + j] = fma(sigma, eps_q, param), q = sample_base + j; the mean is read from the parameter
 *   tensors (where it lives between steps), m and sigma once per launch whatever `members`.  Reads no word.
 *   The noise, by eps_mode.  BNN_EPS_PHILOX: eps_q of element i of tensor k from counter (i >> 2, q, k, 6) slot i & 3, key =
 *   (seed_lo, seed_hi), the map's Box-Muller -- counter word 3 = 6 is a new stream (0 .. 5 taken: F22), BNN_EPS_MAP_VERSION
 *   stays 2.  BNN_EPS_MEMORY: noise [rows, stride]; the training form reads row `sample` (the fold row sample - 1), the bank
 *   form row j.  BNN_EPS_ZERO: eps = 0.  Given the same q and noise both forms write the same bits.
 *   Errors, in this order: NULL args; ABI; n_tensors outside [1, BNN_SGMCMC_MAX_TENSORS], samples outside [1,
 *   BNN_IVON_MAX_SAMPLES], sample outside [0, samples), (bank form) members outside [1, BNN_IVON_MAX_MEMBERS], first < 0,
 *   capacity < 1, first + members > capacity, ess <= 0 or NaN, weight_decay <= 0 or NaN, a numel outside [1, 2^34]:
 *   BNN_ERR_SHAPE; eps_mode: BNN_ERR_ENUM; hess, a param, (training form) mean, step, (sample >= 1) a grad, acc_g, acc_h,
 *   (BNN_EPS_MEMORY) noise NULL: BNN_ERR_NULL; BNN_ERR_ALIGN (tensors, state, noise and bank 16 bytes, step 4).
 *
 * bnn_ivon_step — the natural-gradient step over all tensors in ONE launch, with g the last sample's gradient, q = t * S +
 *   S - 1 (eps regenerated, theta - m never formed), er = eps_q * r, P = *beta1_prod (fp64, beta1^t) read before the update:
 *       gs  = S == 1 ? g : acc_g + g;            hs = S == 1 ? g * er : fma(g, er, acc_h)
 *       gm' = fma(beta1, gm, c1 * gs)
 *       d   = fma(-cS, hs, h)                                       (h - hhat, hhat = cS hs)
 *       h'  = fma(c2, (d * d) / hd, fma(-rho, d, h))                (the correction divides by the OLD h + delta)
 *       ib  = (float)(1 / fma(-P, beta1, 1))                        (fp64, 1 / bc1 with bc1 = 1 - beta1^(t+1); once per thread)
 *       u   = fma(delta, m, gm' * ib) / (h' + delta);   u = min(max(u, -clip_radius), clip_radius) when clip_radius < inf
 *       p   = fma(-lr, u, m)                                        m read from mean; lr: *lr_device when given
 *   Every block reads *step and *beta1_prod before its update; the block that arrives last stores t + 1 and P * beta1 (the
 *   ticketed hand-off of bnn_swag_step; ticket: 16 zeroed uint32 words, left zeroed).  No pow, no float atomics.
 *   Traffic at S = 1: reads g, mean, h, gm, writes p, h, gm: 28 B / parameter (bnn_adam_step's).
 *   Errors, in this order: NULL args; ABI; n_tensors outside [1, BNN_SGMCMC_MAX_TENSORS], samples outside [1,
 *   BNN_IVON_MAX_SAMPLES], ess <= 0, weight_decay <= 0, lr < 0, beta1 outside [0, 1), beta2 outside [0, 1], loss_scale or
 *   clip_radius <= 0 (or any of them NaN), a numel outside [1, 2^34]: BNN_ERR_SHAPE; eps_mode: BNN_ERR_ENUM; step,
 *   beta1_prod, ticket, mean, hess, avg_grad, a param, a grad, (samples > 1) acc_g, acc_h, (BNN_EPS_MEMORY) noise NULL:
 *   BNN_ERR_NULL; BNN_ERR_ALIGN (tensors, state and noise 16 bytes, beta1_prod 8, words 4).
 * ---------------------------------------------------------------------------------- */
#define BNN_IVON_MAX_SAMPLES 8
#define BNN_IVON_MAX_MEMBERS 64           /* per launch */

typedef struct bnn_ivon_draw_args {
  uint32_t struct_bytes;
  int32_t n_tensors;
  float* param[BNN_SGMCMC_MAX_TENSORS];          /* training form: read at sample 0, written; bank form: the mean, read only */
  const float* grad[BNN_SGMCMC_MAX_TENSORS];     /* training form, sample >= 1: the previous sample's gradient */
  int64_t numel[BNN_SGMCMC_MAX_TENSORS];
  int32_t samples;          /* S */
  int32_t sample;           /* s; 0 files the mean (training form) */
  int32_t members, first, capacity;              /* bank form */
  int32_t eps_mode;         /* bnn_eps_mode */
  uint32_t sample_base;     /* bank form */
  int32_t reserved;
  double ess, weight_decay;
  uint64_t seed;
  float* mean;              /* [stride]; training form */
  const float* hess;        /* [stride] */
  float* acc_g;             /* [stride]; sample >= 1 */
  float* acc_h;             /* [stride]; sample >= 1 */
  const uint32_t* step;     /* device word t; training form */
  const float* noise;       /* BNN_EPS_MEMORY: [samples, stride] (training form), [members, stride] (bank form) */
  float* bank;              /* [capacity, stride]: selects the bank form */
} bnn_ivon_draw_args;

typedef struct bnn_ivon_step_args {
  uint32_t struct_bytes;
  int32_t n_tensors;
  float* param[BNN_SGMCMC_MAX_TENSORS];
  const float* grad[BNN_SGMCMC_MAX_TENSORS];
  int64_t numel[BNN_SGMCMC_MAX_TENSORS];
  int32_t samples;          /* S */
  int32_t eps_mode;         /* bnn_eps_mode */
  double lr, ess, weight_decay, beta1, beta2, loss_scale, clip_radius;   /* lr: the rate used (any rescaling done by the caller) */
  const float* lr_device;   /* optional device float: overrides lr */
  uint64_t seed;
  const float* mean;        /* [stride] */
  float* hess;              /* [stride] */
  float* avg_grad;          /* [stride] */
  const float* acc_g;       /* [stride]; samples > 1 */
  const float* acc_h;       /* [stride]; samples > 1 */
  const float* noise;       /* BNN_EPS_MEMORY: [samples, stride]; row samples - 1 is read */
  uint32_t* step;           /* device word t */
  double* beta1_prod;       /* device fp64 word beta1^t */
  uint32_t* ticket;         /* 16 device words, zero between launches */
} bnn_ivon_step_args;

int bnn_ivon_draw(const bnn_ivon_draw_args* args, void* stream);
int bnn_ivon_step(const bnn_ivon_step_args* args, void* stream);

/* ------------------------------------------------------------------------------------
 * bnn_cast_bf16 — fp32 -> bf16 (round to nearest even) of n contiguous elements: the input
 * batch is cast once per ELBO evaluation when bf16 math runs many MC samples, so every
 * layer streams 2-byte activations.  (The reference keeps x in fp32, main.py / class_task.py:71.)
 * ---------------------------------------------------------------------------------- */
/* sigma[i] = log1p(exp(rho[i])) (networks.py:39), n contiguous fp32 elements. */
int bnn_softplus(const float* rho, float* sigma, int64_t n, void* stream);

int bnn_cast_bf16(const float* src, void* dst_bf16, void* dst_sq_bf16 /* optional: bf16(bf16(x)^2) */, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------
 * bnn_eval_prepare — the two passes above for a whole evaluation in ONE launch: everything that depends on no
 * activation.  sigma[i] = softplus(rho[i]) for up to BNN_PREPARE_MAX parameter tensors (networks.py:37-39 evaluates
 * it three times per node and forward; here once per evaluation, then shared by all MC samples through
 * bnn_bbb_fwd_args.w_sigma) and, optionally, the bf16 cast (+ squares) of the input batch.  Elementwise: the same
 * values as bnn_softplus / bnn_cast_bf16.
 * ---------------------------------------------------------------------------------- */
#define BNN_PREPARE_MAX 8
typedef struct bnn_prepare_args {
  uint32_t struct_bytes;
  int32_t n_softplus;                     /* 0 .. BNN_PREPARE_MAX */
  const float* rho[BNN_PREPARE_MAX];
  float* sigma[BNN_PREPARE_MAX];
  int64_t n[BNN_PREPARE_MAX];             /* elements of each tensor */
  const float* cast_src;                  /* optional (cast_n > 0) */
  void* cast_dst;                         /* bf16 */
  void* cast_dst_sq;                      /* optional bf16 squares: bf16(bf16(src)^2); with cast_dst_lo (BNN_MATH_BF16X3) bf16(src^2) */
  int64_t cast_n;
  void* cast_dst_lo;                      /* optional bf16: the low plane bf16(src - cast_dst) of BNN_MATH_BF16X3 */
  int32_t cast_layout;                    /* bnn_layout of cast_dst: BNN_LAYOUT_PIECES = the same values in piece order (see
                                             bnn_bbb_fwd_args), src being [cast_n / (cast_batch * cast_features)][cast_batch]
                                             [cast_features], cast_features % 8 == 0, cast_dst 16-byte aligned and zeroed by the
                                             caller; no cast_dst_sq / cast_dst_lo then */
  int32_t cast_batch, cast_features;      /* BNN_LAYOUT_PIECES only */
  const float* mu[BNN_PREPARE_MAX];       /* with pieces[i]: the [rows[i], cols[i]] mean tensor beside rho[i] (n[i] = rows[i] * cols[i]) */
  void* pieces[BNN_PREPARE_MAX];          /* optional per tensor: (mu, sigma) in piece order (bnn_bbb_fwd_args.w_pieces), written by the
                                             same launch; zeroed by the caller once (pads are never written); cols[i] % 8 == 0,
                                             mu / rho / pieces 16-byte aligned */
  int32_t rows[BNN_PREPARE_MAX], cols[BNN_PREPARE_MAX];
} bnn_prepare_args;
int bnn_eval_prepare(const bnn_prepare_args* args, void* stream);

int bnn_version(void);                    /* BNN_HIP_ABI_VERSION the library was built with */
int bnn_philox_rounds(void);              /* BNN_PHILOX_ROUNDS the library was built with (7, or 10 for rocRAND's generator) */
const char* bnn_status_string(int status); /* static string for a negative status */

#ifdef __cplusplus
}
#endif
#endif /* BNN_HIP_H_ */
