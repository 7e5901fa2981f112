// The empirical quantile delta mapping of one value against one table row
// (Cannon et al. 2015, eqs. 3-6, as rex's QuantileDeltaMapping with linear
// sampling): shared by the correction of chunks (kernels_bias.hip) and by
// PresRat's corrected future series (kernels_bias_calc.hip), which must map
// values the way the correction later will.
#pragma once
#include "common.h"

namespace {

// np.minimum / np.maximum: a NaN on either side comes out
__device__ __forceinline__ float np_min(float a, float b) {
  return a != a ? a : (b != b ? b : (a < b ? a : b));
}
__device__ __forceinline__ float np_max(float a, float b) {
  return a != a ? a : (b != b ? b : (a > b ? a : b));
}

// x * y rounded on its own: the product is pinned in a register, so that no
// multiply-add contraction can reach it (affine_channels_kernel's idiom; the
// header's __fmul_rn is a plain product that the optimiser may still fuse)
__device__ __forceinline__ float mul_rn(float x, float y) {
  float m = x * y;
  asm volatile("" : "+v"(m));
  return m;
}

// numpy.interp(x, xp, fp) with fp[k] = k / (Q - 1): clamped at both ends, on
// repeated knots the segment is the last j with xp[j] <= x (binary search)
__device__ __forceinline__ float quantile_of(float x, const float* __restrict__ xp, int Q, float qm1) {
#pragma clang fp contract(off)
  if (x != x) return x;
  if (x < xp[0]) return 0.f;
  if (!(x < xp[Q - 1])) return 1.f;
  int lo = 0, hi = Q - 1;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (xp[mid] <= x) lo = mid; else hi = mid;
  }
  const float q0 = __fdiv_rn((float)lo, qm1), q1 = __fdiv_rn((float)(lo + 1), qm1);
  const float x0 = xp[lo], x1 = xp[lo + 1];
  const float slope = __fdiv_rn(__fsub_rn(q1, q0), __fsub_rn(x1, x0));
  return __fadd_rn(mul_rn(slope, __fsub_rn(x, x0)), q0);
}

// numpy.interp(q, k / (Q - 1), fp): the levels are evenly spaced, so the
// segment is found at q (Q - 1) and settled against the levels themselves
__device__ __forceinline__ float value_at(float q, const float* __restrict__ fp, int Q, float qm1) {
#pragma clang fp contract(off)
  if (q != q) return q;
  if (q < 0.f) return fp[0];
  if (!(q < 1.f)) return fp[Q - 1];
  int j = (int)(q * qm1);
  if (j > Q - 2) j = Q - 2;
  if (j < 0) j = 0;
  while (j > 0 && q < __fdiv_rn((float)j, qm1)) --j;
  while (j < Q - 2 && q >= __fdiv_rn((float)(j + 1), qm1)) ++j;
  const float q0 = __fdiv_rn((float)j, qm1), q1 = __fdiv_rn((float)(j + 1), qm1);
  const float f0 = fp[j], f1 = fp[j + 1];
  const float slope = __fdiv_rn(__fsub_rn(f1, f0), __fsub_rn(q1, q0));
  return __fadd_rn(mul_rn(slope, __fsub_rn(q, q0)), f0);
}

__device__ __forceinline__ float qdm_value(const s3_bias_channel& d, float x, size_t row, size_t tp) {
#pragma clang fp contract(off)
  const int Q = d.n_q;
  const float qm1 = (float)(Q - 1);
  const float* xp = ((d.flags & S3_BC_NO_TREND) ? d.mh : d.mf) + row * Q;
  const float q = quantile_of(x, xp, Q, qm1);
  const float x_oh = value_at(q, d.oh + row * Q, Q, qm1);
  float x_mh = value_at(q, d.mh + row * Q, Q, qm1);
  float v;
  if (d.flags & S3_BC_RELATIVE) {
    if ((d.flags & S3_BC_DENOM_ZERO) && x_mh == 0.f) x_mh = d.denom_zero;
    if (d.flags & S3_BC_DENOM_MIN) x_mh = np_max(x_mh, d.denom_min);
    float delta = __fdiv_rn(x, x_mh);
    if (d.flags & S3_BC_DELTA_RANGE) delta = np_min(np_max(delta, d.delta_lo), d.delta_hi);
    v = mul_rn(x_oh, delta);
  } else {
    float delta = __fsub_rn(x, x_mh);
    if (d.flags & S3_BC_DELTA_RANGE) delta = np_min(np_max(delta, d.delta_lo), d.delta_hi);
    v = __fadd_rn(x_oh, delta);
  }
  if ((d.flags & S3_BC_PRESRAT) && !(d.flags & S3_BC_NO_TREND))
    v = v < d.tau[tp] ? 0.f : mul_rn(v, d.kfac[row]);
  return v;
}

}  // namespace
