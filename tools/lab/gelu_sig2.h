// The two-transcendental sigmoid GELU of the fused MLP kernels of rounds 2-4 (the product runs cn_gelu_e1_half, csrc/common.h,
// since round 5): kept for the lab kernels that were measured with it (mlp_f8.h, mlp_rc2_skew.h, mlp_lab.hip) and as the form
// oracle/fp8_ref.py restates.
#pragma once
#include "common.h"

// GELU as x * sigmoid(x (a + b x^2 + c x^4)): minimax fit of the logit of the normal CDF on [-8, 8], max |error|
// against the exact erf form 2.5e-5 (tanh form: 4.7e-4).  x^2 is clamped at 64, where the quartic would bend back.
__device__ __forceinline__ float cn_gelu_sig2(float x) {
  constexpr float L2E = 1.4426950408889634f;
  const float x2 = fminf(x * x, 64.0f);
  float p = fmaf(x2, 0.0007030350670982541f * L2E, -0.07401130190658815f * L2E);
  p = fmaf(p, x2, -1.5950157568571721f * L2E);
  const float e = __builtin_amdgcn_exp2f(x * p);
  return x * __builtin_amdgcn_rcpf(1.0f + e);
}

// two elements at once: v_pk_mul / v_pk_fma / v_pk_add carry both (the two min, exp2 and rcp stay scalar)
__device__ __forceinline__ f32x2 cn_gelu_sig2_pk(f32x2 x) {
  constexpr float L2E = 1.4426950408889634f;
  f32x2 x2 = x * x;
  x2 = f32x2{fminf(x2[0], 64.0f), fminf(x2[1], 64.0f)};
  f32x2 p = x2 * (0.0007030350670982541f * L2E) + (-0.07401130190658815f * L2E);
  p = p * x2 + (-1.5950157568571721f * L2E);
  const f32x2 u = x * p;
  const f32x2 d = f32x2{__builtin_amdgcn_exp2f(u[0]), __builtin_amdgcn_exp2f(u[1])} + 1.0f;
  return x * f32x2{__builtin_amdgcn_rcpf(d[0]), __builtin_amdgcn_rcpf(d[1])};
}
