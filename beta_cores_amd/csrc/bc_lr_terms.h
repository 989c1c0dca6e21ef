// The per-row terms of the logistic log-likelihood, shared by K5 (bc_laplace.hip) and the multi-chain rows pass (bc_hmc.hip).
#pragma once
#include <hip/hip_runtime.h>

// the per-row terms for one m = -z . theta: log-likelihood, p, c -- overflow-free (exp of a non-positive argument only)
__device__ __forceinline__ void lr_terms(double m, double& ll, double& p, double& c) {
  if (m < 100.) {
    const double e = exp(-fabs(m)), ope = 1. + e;
    ll = -(fmax(m, 0.) + log1p(e));
    p = m >= 0. ? 1. / ope : e / ope;
    c = e / (ope * ope);
  } else {
    ll = -m;
    p = 1.;
    c = 0.;
  }
}
