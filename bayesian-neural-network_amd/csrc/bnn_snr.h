// The SNR of one (mu, rho) pair: ONE definition for bnn_snr_db, bnn_snr_prune (posthoc.hip) and bnn_prune_codes
// (prune_sweep.hip), whose masks must agree bit for bit.
#pragma once
#include "bnn_device.h"

namespace bnn {

// 10 * log10(|mu| / softplus(rho)) in fp32, as torch evaluates weight_pruning.py:100 / :109 (softplus = log1p(exp(rho))).
// The fast form -- the hardware log2 of the fp32 ratio -- holds the 3e-5 dB bound of the tests up to 128 dB in magnitude:
// beyond that its three roundings are ulps of 1.5e-5 and 3e-5 dB, and the hardware log2 takes a subnormal ratio as 0
// (mu = -1e-40 at rho = -0.25 gave -inf where the reference has -397.6 dB; tests/golden/posthoc.npz, the edge network).
// So a finite non-zero ratio whose fast result is not below 128 dB in magnitude takes the fp64 log of the fp64 ratio
// (the fp32 ratio itself would carry a subnormal's few bits).  The CLASS of the result stays that of the fp32 ratio, the
// reference's: 0 (mu = 0, or sigma = +inf from rho >= 89) gives -inf, +inf gives +inf, NaN gives NaN.  No trained
// network comes near 128 dB, so ordinary values keep their bits and the branch is never taken on them.
__device__ __forceinline__ float snr_db(float mu, float rho) {
  const float a = fabsf(mu), s = softplus(rho);
  const float q = a / s;
  const float fast = 10.0f * (__builtin_amdgcn_logf(q) * 0.30102999566398120f);   // log2 -> log10
  if (!(fabsf(fast) < 128.0f) && q > 0.0f && q < __builtin_inff()) return (float)(10.0 * log10((double)a / (double)s));
  return fast;
}

}  // namespace bnn
