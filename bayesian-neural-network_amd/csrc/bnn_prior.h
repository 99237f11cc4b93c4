// The prior's share of the backward, shared by the dense layer backward (bbb_bwd.hip) and the sparse one
// (sparse_train.hip): d log p(w) / dw of the Gaussian and the scale-mixture prior, and the
// host-side fill of their constants.  Both backward paths give a weight the same bits for the same w.  (bbb_group.hip keeps
// its own BgPrior, which also carries the log-prior constants.)
#pragma once
#include "bnn_device.h"
#include "../../include/bnn_hip.h"

namespace bnn {

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

// The constants above from a bnn_prior.  BNN_ERR_SHAPE for a non-positive scale.
template <class P>
inline int prior_dlogp_fill(const bnn_prior& pr, P& k) {
  k.prior_kind = pr.kind;
  k.inv_var_p = 0.f; k.a1 = k.a2 = k.inv2var1 = k.inv2var2 = k.invvar1 = k.invvar2 = 0.f;
  if (pr.kind == BNN_PRIOR_MIXTURE) {
    if (!(pr.sigma1 > 0.f) || !(pr.sigma2 > 0.f)) return BNN_ERR_SHAPE;
    const double s1 = pr.sigma1, s2 = pr.sigma2;
    k.a1 = (float)(pr.pi / s1);
    k.a2 = (float)((1.0 - pr.pi) / s2);
    k.inv2var1 = (float)(1.0 / (2.0 * s1 * s1));
    k.inv2var2 = (float)(1.0 / (2.0 * s2 * s2));
    k.invvar1 = (float)(1.0 / (s1 * s1));
    k.invvar2 = (float)(1.0 / (s2 * s2));
  } else {
    if (!(pr.sigma_p > 0.f)) return BNN_ERR_SHAPE;
    k.inv_var_p = (float)(1.0 / ((double)pr.sigma_p * pr.sigma_p));
  }
  return BNN_OK;
}

}  // namespace bnn
