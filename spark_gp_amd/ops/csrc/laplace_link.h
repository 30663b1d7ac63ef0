// The response link of fused_laplace_kernel (laplace.hip): what Algorithms
// 3.1 and 5.1 take from the likelihood, elementwise over the k rows — log p
// and its first three derivatives in f.  The kernel is a template over
// LINK (a LAP_LINK_* code of kernel_geom.h) and asks for them here.
//
//   logistic  the kernel's own fp32 statements (pi = sigmoid(f) and what
//             follows from it); only log p is spelled here, as it always was
//   probit    p(y = 1 | f) = Phi(f).  With t = 2y - 1 and z = t f
//             (R&W section 3.9; likelihoods.py::ProbitLikelihood):
//               h     = phi(z) / Phi(z)           inverse Mills ratio
//               dlogp = t h
//               W     = h (h + z)                 in (0, 1)
//               dW/df = t [h + (z + 2h) h'],  h' = -(z h + h^2) = -W
//               log p = log Phi(z)
//
// The probit tails are where an fp32 evaluation goes wrong: for z << 0,
// h ~ -z and W = h (h + z) is a difference of two numbers that agree to
// 1/z^2 (four digits gone at z = -30), b = W f + dlogp cancels the same
// way, and Phi(z) itself underflows fp32 at z = -13.  So a row's link terms
// are evaluated in fp64 through the scaled complementary error function,
// which has no tail to lose,
//   z <  0:  h = sqrt(2/pi) / erfcx(-z/sqrt2)
//            log Phi = -z^2/2 + log(erfcx(-z/sqrt2) / 2)
//   z >= 0:  h = phi(z) / (1 - erfc(z/sqrt2) / 2)
//            log Phi = log1p(-erfc(z/sqrt2) / 2)
// and only the results are rounded to fp32 for LDS.  That is k fp64
// evaluations per Newton iteration next to an O(k^3) factorization.
//
// A third link adds a code, a branch in lap_log_lik and a *_terms function.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "kernel_geom.h"

__device__ inline double log_sigmoid(double v) {
  // log(1/(1+exp(-v))) = -log1p(exp(-v)), stable for both signs
  if (v < -30.0) return v;
  return -log1p(exp(-v));
}

// h(z) = phi(z) / Phi(z)
__device__ inline double probit_h(const double z) {
  if (z < 0.0)
    return 0.7978845608028654 / erfcx(-z * 0.7071067811865476);
  return 0.3989422804014327 * exp(-0.5 * z * z)
         / (1.0 - 0.5 * erfc(z * 0.7071067811865476));
}

__device__ inline double probit_log_cdf(const double z) {
  if (z < 0.0)
    return -0.5 * z * z + log(0.5 * erfcx(-z * 0.7071067811865476));
  return log1p(-0.5 * erfc(z * 0.7071067811865476));
}

// log p(y | f) of one row at z = (2y - 1) f
template <int LINK>
__device__ __forceinline__ double lap_log_lik(const double z) {
  if constexpr (LINK == LAP_LINK_PROBIT)
    return probit_log_cdf(z);
  else
    return log_sigmoid(z);
}

// The probit terms of one row at the latent f, y in {0, 1}: W, dlogp,
// b = W f + dlogp and (D3) dW/df, each computed in fp64 and rounded once.
template <bool D3>
__device__ inline void probit_terms(const float f, const float y, float& w,
                                    float& dlogp, float& b, float& d3) {
  const double t = 2.0 * (double)y - 1.0;
  const double z = t * (double)f;
  const double h = probit_h(z);
  // W > 0 in exact arithmetic; past z = -1e7 the fp64 sum h + z rounds to
  // zero or below, and sqrt(W) must stay a number
  const double W = fmax(h * (h + z), 0.0);
  w = (float)W;
  dlogp = (float)(t * h);
  b = (float)(W * (double)f + t * h);
  if constexpr (D3) d3 = (float)(t * (h - (z + 2.0 * h) * W));
}
