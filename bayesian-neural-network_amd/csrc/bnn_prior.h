// The weight prior, in one place: the only file that knows a bnn_prior.  Its density (the Gaussian and the scale
// mixture), its derivative d log p(w) / dw, the host-side constants of both, the validation of a bnn_prior, and the fold
// of a layer's partial sums into log_prior / log_q / KL.  Every forward and every backward calls these, so a weight gets the
// same bits for the same w whichever kernel touches it.
#pragma once
#include "bnn_device.h"
#include "../../include/bnn_hip.h"
#include <math.h>

namespace bnn {

// ---------------------------------------------------------------------------- density
// mixture: log N(w; 0, sigma_i) = c_i - w^2 * inv2var_i, c_i = c0 - log sigma_i
struct PriorMix { float inv2var1, c1, inv2var2, c2, pi; };

// the mixture density itself (argument of the log; accumulated with add_log: explicit contraction, see bnn_device.h).
// M: PriorMix, or any block with its five fields.
template <class M>
__device__ __forceinline__ float prior_mix_p(const M& m, float w) {
  const float w2 = w * w;
  const float p1 = fast_exp(__builtin_fmaf(-w2, m.inv2var1, m.c1));
  const float p2 = fast_exp(__builtin_fmaf(-w2, m.inv2var2, m.c2));
  return __builtin_fmaf(m.pi, p1, (1.0f - m.pi) * p2);
}

// every constant of either kind: what a kernel that takes log p AND its derivative per weight carries (bbb_group.hip)
struct PriorAll {
  int prior_kind;
  float inv_var_p, inv2var_p, c_p;                                  // Gaussian: 1 / sigma_p^2, 1 / (2 sigma_p^2), c0 - log sigma_p
  float pi, c1, c2, a1, a2, inv2var1, inv2var2, invvar1, invvar2;   // mixture: c_i as above, a_i = pi_i / sigma_i
};

__device__ __forceinline__ float prior_logp(const PriorAll& p, float w) {
  if (p.prior_kind == BNN_PRIOR_GAUSS) return __builtin_fmaf(-(w * w), p.inv2var_p, p.c_p);
  return fast_log(prior_mix_p(p, w));
}

// d log p(w) / dw.  P: a kernel parameter block with prior_kind, inv_var_p (Gaussian: 1 / sigma_p^2) and a1, a2, inv2var1,
// inv2var2, invvar1, invvar2 (mixture: a_i = pi_i / sigma_i).
template <class P>
__device__ __forceinline__ float prior_dlogp(const P& p, float w) {
  if (p.prior_kind == BNN_PRIOR_GAUSS) return -w * p.inv_var_p;
  const float w2 = w * w;
  const float n1 = p.a1 * fast_exp(-w2 * p.inv2var1);
  const float n2 = p.a2 * fast_exp(-w2 * p.inv2var2);
  return -w * (n1 * p.invvar1 + n2 * p.invvar2) * __builtin_amdgcn_rcpf(n1 + n2);
}

// ---------------------------------------------------------------------------- host: a bnn_prior -> constants
// BNN_ERR_ENUM for an unknown kind, then BNN_ERR_SHAPE for a non-positive scale of the kind in use.  need_sigma_p = false:
// a Gaussian prior whose sigma_p nothing will read (no statistics wanted) passes.
inline int prior_check(const bnn_prior& pr, bool need_sigma_p = true) {
  if ((unsigned)pr.kind > 1u) return BNN_ERR_ENUM;
  if (pr.kind == BNN_PRIOR_MIXTURE ? (!(pr.sigma1 > 0.f) || !(pr.sigma2 > 0.f)) : (need_sigma_p && !(pr.sigma_p > 0.f)))
    return BNN_ERR_SHAPE;
  return BNN_OK;
}

// the density constants (a Gaussian prior: zeros, pi kept)
inline PriorMix prior_mix_make(const bnn_prior& pr) {
  PriorMix m = {0.f, 0.f, 0.f, 0.f, pr.pi};
  if (pr.kind != BNN_PRIOR_MIXTURE) return m;
  const double s1 = pr.sigma1, s2 = pr.sigma2;
  m.inv2var1 = (float)(1.0 / (2.0 * s1 * s1));
  m.inv2var2 = (float)(1.0 / (2.0 * s2 * s2));
  m.c1 = (float)(kNegLogSqrt2Pi - log(s1));
  m.c2 = (float)(kNegLogSqrt2Pi - log(s2));
  return m;
}

// the derivative constants of prior_dlogp into a parameter block (a checked prior)
template <class P>
inline void prior_dlogp_fill(const bnn_prior& pr, P& k) {
  k.prior_kind = pr.kind;
  k.inv_var_p = 0.f; k.a1 = k.a2 = k.inv2var1 = k.inv2var2 = k.invvar1 = k.invvar2 = 0.f;
  if (pr.kind == BNN_PRIOR_MIXTURE) {
    const double s1 = pr.sigma1, s2 = pr.sigma2;
    k.a1 = (float)(pr.pi / s1);
    k.a2 = (float)((1.0 - pr.pi) / s2);
    k.inv2var1 = (float)(1.0 / (2.0 * s1 * s1));
    k.inv2var2 = (float)(1.0 / (2.0 * s2 * s2));
    k.invvar1 = (float)(1.0 / (s1 * s1));
    k.invvar2 = (float)(1.0 / (s2 * s2));
  } else {
    k.inv_var_p = (float)(1.0 / ((double)pr.sigma_p * pr.sigma_p));
  }
}

// both (a Gaussian prior with sigma_p <= 0, which only a caller that skipped prior_check passes: zeros)
inline PriorAll prior_all_make(const bnn_prior& pr) {
  PriorAll o = PriorAll{};
  if (pr.kind == BNN_PRIOR_MIXTURE || pr.sigma_p > 0.f) prior_dlogp_fill(pr, o);
  o.prior_kind = pr.kind;
  if (pr.kind == BNN_PRIOR_MIXTURE) {
    const PriorMix m = prior_mix_make(pr);
    o.pi = m.pi; o.c1 = m.c1; o.c2 = m.c2;
  } else if (pr.sigma_p > 0.f) {
    const double sp = pr.sigma_p;
    o.inv2var_p = (float)(1.0 / (2.0 * sp * sp));
    o.c_p = (float)(kNegLogSqrt2Pi - log(sp));
  }
  return o;
}

// ---------------------------------------------------------------------------- the fold of a layer's sums
// The constants for a tensor set of `cnt` elements (a mixture prior counts as sigma_p = 1: only cnt_c0 is read then).
struct PriorFold {
  double cnt_c0;      // cnt * c0                                (log q)
  double lp_const;    // cnt * (c0 - log sigma_p)                (Gaussian log p)
  double kl_const;    // 0.5 * (2 cnt log sigma_p - cnt)         (LR: the closed-form KL)
  double inv2var;     // 1 / (2 sigma_p^2)
};
inline PriorFold prior_fold_make(const bnn_prior& pr, double cnt) {
  const double sp = (pr.kind == BNN_PRIOR_MIXTURE) ? 1.0 : (double)pr.sigma_p;
  PriorFold f;
  f.cnt_c0 = cnt * kNegLogSqrt2Pi;
  f.lp_const = cnt * (kNegLogSqrt2Pi - log(sp));
  f.kl_const = 0.5 * (2.0 * cnt * log(sp) - cnt);
  f.inv2var = 1.0 / (2.0 * sp * sp);
  return f;
}

// log q = cnt c0 - sum log sigma - sum eps^2 / 2
__device__ __forceinline__ double fold_log_q(double cnt_c0, double sum_log_sigma, double sum_eps2) {
  return cnt_c0 - sum_log_sigma - 0.5 * sum_eps2;
}
// log p from the kernels' second sum: Gaussian: sum w^2 -> lp_const - sum / (2 sigma_p^2); mixture: sum log mix, as it is
__device__ __forceinline__ double fold_log_p(int prior_kind, double lp_const, double inv2var, double sum_a) {
  return prior_kind == BNN_PRIOR_GAUSS ? lp_const - sum_a * inv2var : sum_a;
}
// The same from the bnn_prior itself, for a kernel that carries no host constants (bbb_layer_scalars_kernel): it DIVIDES
// by 2 sigma_p^2 where the others multiply by the host's reciprocal, so the two forms round differently and both stay.
__device__ __forceinline__ double fold_log_p(const bnn_prior& pr, double cnt, double sum_a) {
  if (pr.kind != BNN_PRIOR_GAUSS) return sum_a;
  return cnt * (kNegLogSqrt2Pi - log((double)pr.sigma_p)) - sum_a / (2.0 * (double)pr.sigma_p * (double)pr.sigma_p);
}

}  // namespace bnn
