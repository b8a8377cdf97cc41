// The fp32 box-plus, the one statement of it for the flooding BP check node (float_kernels.hip fl_cn) and the
// layered BP check core (layered_bp_kernels.hip lay_bp). Device code only; include after common.h.
#pragma once

namespace ibl {

// fp32: |a [+] b| = min(|a|,|b|) + ln(1 + e^-(|a|+|b|)) - ln(1 + e^-||a|-|b||)  (>= 0), sign =
// sgn(a) sgn(b). Evaluated on the hardware base-2 exp/log (v_exp_f32 / v_log_f32, ~1 ulp): no
// range reduction or denormal fix-ups, 4 transcendentals + ~12 VALU per operation. a or b = 0
// gives sum == dif, so the two log terms cancel exactly and the result is 0, as in the reference.
// The product and sum of the last step are one explicit fmaf, so the value does not depend on the
// translation unit's -ffp-contract setting: no other step has a product feeding a sum.
__device__ __forceinline__ float boxplus(float a, float b, float lm) {
  constexpr float kLog2e = 1.4426950408889634f, kLn2 = 0.6931471805599453f;
  const float aa = fabsf(a), ab = fabsf(b);
  const float mn = fminf(aa, ab);
  const float u = __builtin_amdgcn_exp2f(-(aa + ab) * kLog2e);
  const float v = __builtin_amdgcn_exp2f(-fabsf(aa - ab) * kLog2e);
  float mag = fmaf(kLn2, __builtin_amdgcn_logf(1.f + u) - __builtin_amdgcn_logf(1.f + v), mn);
  mag = __builtin_amdgcn_fmed3f(mag, 0.f, lm);  // rounding may leave -ulp for tiny min; clamp to [0, lm] (:69)
  return ((a < 0.f) != (b < 0.f)) ? -mag : mag;
}

}  // namespace ibl
