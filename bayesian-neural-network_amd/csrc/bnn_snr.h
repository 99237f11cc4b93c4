// The SNR of one (mu, rho) pair: ONE definition for bnn_snr_db, bnn_snr_prune (posthoc.hip) and bnn_prune_codes
// (prune_sweep.hip), whose masks must agree bit for bit.
#pragma once
#include "bnn_device.h"

namespace bnn {

// 10 * log10(|mu| / softplus(rho)) in fp32, as torch evaluates weight_pruning.py:100 / :109 (softplus = log1p(exp(rho)))
__device__ __forceinline__ float snr_db(float mu, float rho) {
  return 10.0f * (__builtin_amdgcn_logf(fabsf(mu) / softplus(rho)) * 0.30102999566398120f);   // log2 -> log10
}

}  // namespace bnn
