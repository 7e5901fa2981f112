// Computing bias-correction factors on the device: the per-pixel work of
// sup3r/bias/bias_calc.py (linear family), qdm.py and presrat.py.  The
// reference hands every low-res pixel to a process pool (abstract.py:79-97);
// here a pixel is a workgroup (or a lane, where the work is a short loop):
//   s3_bc_base_series       site mean + daily reduction of the hi-res base data
//                           (base.py:453-554, 631, 683-686, 694-780)
//   s3_bc_moments           count, nanmean, nanstd per (pixel, group)
//                           (bias_calc.py:76-90 over the months of :354-368)
//   s3_bc_window_quantiles  np.quantile of a day-of-year window (qdm.py:447-453)
//   s3_bc_match_zero_rate   base.py:557-599
//   s3_bc_presrat           PresRat's corrected future series, zero rate, tau_fut
//                           and k_factor (presrat.py:96-360)
//   s3_bc_skill             SkillAssessment's annual part: moments, zero rate,
//                           percentiles and the two-sample KS counts
//                           (bias_calc.py:431-481)
// All series are (P, T), pixel-major.  Sums are fp64 and rounded to fp32 once;
// every output value is produced by one thread or by one workgroup's fixed
// reduction tree, so nothing depends on the launch geometry.  No float
// atomics.  The sorts run in LDS on order-preserving integer keys; every
// barrier of the sort loops is reached by the whole workgroup (the loop bounds
// depend on the segment length and blockDim only, short segments are padded
// with sentinel keys).
#include "common.h"
#include "bias_qdm.h"

#include <algorithm>

namespace {

constexpr int kBlk = 256;
constexpr int kSortBlk = 1024;
constexpr int kMaxSort = S3_BCC_MAX_SORT;
constexpr int kMaxGroups = S3_BCC_MAX_GROUPS;
constexpr uint32_t kNanKey = 0xFFFFFFFEu;   // behind +inf
constexpr uint32_t kPadKey = 0xFFFFFFFFu;   // behind the NaNs

// float -> unsigned key with the order of the floats: -inf < .. < -0 < +0 <
// .. < +inf < NaN (every NaN gets one key: none is ever compared as a float)
__device__ __forceinline__ uint32_t sort_key(float v) {
  if (v != v) return kNanKey;
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_value(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// smallest power of two >= max(n, 2)
__host__ __device__ __forceinline__ int pow2_ceil(int n) {
  int p = 2;
  while (p < n) p <<= 1;
  return p;
}

// bitonic sort of keys[0 .. n2), n2 a power of two, ascending.  Called by the
// whole workgroup with a workgroup-uniform n2; a barrier after every stage.
__device__ void bitonic_sort(uint32_t* keys, int n2) {
  for (int k = 2; k <= n2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < (n2 >> 1); i += blockDim.x) {
        const int lo = 2 * i - (i & (j - 1));
        const int hi = lo | j;
        const bool up = (lo & k) == 0;
        const uint32_t a = keys[lo], b = keys[hi];
        if ((a > b) == up) { keys[lo] = b; keys[hi] = a; }
      }
      __syncthreads();
    }
  }
}

// np.around(x, decimals) of a float32 (numpy multiplies, rints and divides in
// the array's type; negative decimals divide first)
__device__ __forceinline__ float np_around(float x, float p10, int negative) {
#pragma clang fp contract(off)
  if (negative) return __fmul_rn(rintf(__fdiv_rn(x, p10)), p10);
  return __fdiv_rn(rintf(__fmul_rn(x, p10)), p10);
}

struct BaseArgs {
  const float* base;
  const float* cs;
  int64_t T, n_sites;
  int P, n_days, reduction, nanskip, cs_ratio, round_on, round_neg;
  float p10;
  const int32_t* site_ptr;
  const int32_t* site_idx;
  const int32_t* day_ptr;
  const int32_t* step_idx;
  int64_t D_total, day_offset;
  float* out;
};

// mean over the pixel's sites of one step: NaN-skipping (np.nanmean: NaN when
// every site is NaN) or plain
__device__ __forceinline__ double site_mean(const float* __restrict__ row, const int32_t* __restrict__ idx,
                                            int s0, int s1, int nanskip) {
  double sum = 0.0;
  int cnt = 0;
  for (int s = s0; s < s1; ++s) {
    const float v = row[idx[s]];
    if (nanskip && v != v) continue;
    sum += (double)v;
    ++cnt;
  }
  return cnt ? sum / (double)cnt : (double)NAN;
}

// one thread per (day, pixel): the day's steps, each averaged over the sites.
// The lanes of a wave are neighbouring pixels of ONE day: they walk the same
// base rows, and where neighbouring pixels' sites are neighbours in the row
// (sites sorted by location) their loads share cache lines.  The daily
// reductions skip NaN steps as pandas' groupby does: avg / max / min of a day
// without a valid step are NaN, its sum is 0.
__global__ void __launch_bounds__(kBlk) base_series_kernel(BaseArgs a) {
  const int chunks = (a.P + kBlk - 1) / kBlk;
  const int d = blockIdx.x / chunks;
  const int p = (blockIdx.x - d * chunks) * kBlk + threadIdx.x;
  if (p >= a.P) return;                          // (no barrier in this kernel)
  const int s0 = a.site_ptr[p], s1 = a.site_ptr[p + 1];
  float r = NAN;
  if (s1 > s0) {
    double acc = 0.0, acc_cs = 0.0;
    int cnt = 0;
    if (a.reduction == S3_BCC_MAX) acc = -INFINITY;
    if (a.reduction == S3_BCC_MIN) acc = INFINITY;
    for (int e = a.day_ptr[d]; e < a.day_ptr[d + 1]; ++e) {
      const int64_t t = a.step_idx[e];
      const double m = site_mean(a.base + t * a.n_sites, a.site_idx, s0, s1, a.nanskip);
      if (a.cs_ratio) {
        const double c = site_mean(a.cs + t * a.n_sites, a.site_idx, s0, s1, a.nanskip);
        if (c == c) acc_cs += c;
      }
      if (m != m) continue;
      ++cnt;
      if (a.reduction == S3_BCC_MAX) acc = m > acc ? m : acc;
      else if (a.reduction == S3_BCC_MIN) acc = m < acc ? m : acc;
      else acc += m;
    }
    if (a.cs_ratio) {
      // base.py:745-749
      if (acc_cs == 0.0) { acc = 0.0; acc_cs = 1.0; }
      r = (float)(acc / acc_cs);
    } else if (a.reduction == S3_BCC_SUM) {
      r = (float)acc;
    } else if (cnt) {
      r = a.reduction == S3_BCC_AVG ? (float)(acc / (double)cnt) : (float)acc;
    }
    if (a.round_on) r = np_around(r, a.p10, a.round_neg);
  }
  a.out[(int64_t)p * a.D_total + a.day_offset + d] = r;
}

// one workgroup per pixel.  Lanes accumulate their steps per group in LDS
// columns of their own, a fixed tree sums the columns: mean first, then the
// mean of the squared deviations from it (numpy's two passes, ddof = 0).
__global__ void __launch_bounds__(kBlk)
moments_kernel(const float* __restrict__ series, int64_t T, const int32_t* __restrict__ group, int NT,
               int32_t* __restrict__ count, float* __restrict__ mean, float* __restrict__ sd) {
  __shared__ double acc[kMaxGroups][kBlk];
  __shared__ int cnt[kMaxGroups][kBlk];
  __shared__ double mu[kMaxGroups];
  const int tid = threadIdx.x;
  const float* x = series + (int64_t)blockIdx.x * T;
  for (int pass = 0; pass < 2; ++pass) {
    for (int g = 0; g < NT; ++g) { acc[g][tid] = 0.0; cnt[g][tid] = 0; }
    for (int64_t t = tid; t < T; t += kBlk) {
      const int g = group[t];
      const float v = x[t];
      if (g < 0 || v != v) continue;
      if (pass == 0) {
        acc[g][tid] += (double)v;
      } else {
        const double dv = (double)v - mu[g];
        acc[g][tid] += dv * dv;
      }
      ++cnt[g][tid];
    }
    __syncthreads();
    for (int s = kBlk >> 1; s > 0; s >>= 1) {
      if (tid < s)
        for (int g = 0; g < NT; ++g) { acc[g][tid] += acc[g][tid + s]; cnt[g][tid] += cnt[g][tid + s]; }
      __syncthreads();
    }
    if (tid < NT) {
      const int n = cnt[tid][0];
      const int64_t o = (int64_t)blockIdx.x * NT + tid;
      if (pass == 0) {
        mu[tid] = n ? acc[tid][0] / (double)n : (double)NAN;
        count[o] = n;
        mean[o] = (float)mu[tid];
      } else {
        sd[o] = n ? (float)sqrt(acc[tid][0] / (double)n) : NAN;
      }
    }
    __syncthreads();
  }
}

// one workgroup per (pixel, window): gather, sort, interpolate the order
// statistics at (n - 1) q_k, q_k = np.linspace(0, 1, Q)[k]
__global__ void __launch_bounds__(kSortBlk)
window_quantiles_kernel(const float* __restrict__ series, int64_t T, int W, const int32_t* __restrict__ win_ptr,
                        const int32_t* __restrict__ member, int Q, float* __restrict__ out) {
#pragma clang fp contract(off)
  extern __shared__ uint32_t keys[];
  __shared__ int has_nan;
  const int p = blockIdx.x / W, w = blockIdx.x - p * W;
  const int m0 = win_ptr[w], n = win_ptr[w + 1] - m0;
  const int n2 = pow2_ceil(n);                   // workgroup-uniform
  if (threadIdx.x == 0) has_nan = 0;
  __syncthreads();
  const float* x = series + (int64_t)p * T;
  int bad = 0;
  for (int i = threadIdx.x; i < n2; i += blockDim.x) {
    uint32_t k = kPadKey;
    if (i < n) {
      k = sort_key(x[member[m0 + i]]);
      bad |= k == kNanKey;
    }
    keys[i] = k;
  }
  if (bad) atomicOr(&has_nan, 1);
  __syncthreads();
  bitonic_sort(keys, n2);
  float* row = out + (int64_t)blockIdx.x * Q;
  const bool empty = n == 0 || has_nan;          // np.quantile: a NaN member -> NaN
  const double step = Q > 1 ? 1.0 / (double)(Q - 1) : 0.0;
  for (int k = threadIdx.x; k < Q; k += blockDim.x) {
    float v = NAN;
    if (!empty) {
      const double q = k == Q - 1 && Q > 1 ? 1.0 : (double)k * step;
      const double pos = (double)(n - 1) * q;
      int lo = (int)pos;
      if (lo > n - 1) lo = n - 1;
      const double frac = pos - (double)lo;
      const double a = (double)key_value(keys[lo]);
      // (equal neighbours are returned as they are: a zero keeps its sign)
      const uint32_t kb = keys[lo + 1 > n - 1 ? lo : lo + 1];
      if (frac == 0.0 || kb == keys[lo]) {
        v = (float)a;
      } else {
        const double b = (double)key_value(kb);
        v = (float)(a + (b - a) * frac);
      }
    }
    row[k] = v;
  }
}

// np.interp(x, np.linspace(0, 1, n), sorted) in float64, numpy's own branches
// (compiled_base.c arr_interp): x on a knot returns the knot's value
__device__ double interp_linspace(double x, const uint32_t* keys, int n) {
#pragma clang fp contract(off)
  if (n == 1) return (double)key_value(keys[0]);
  const double step = 1.0 / (double)(n - 1);
  auto xp = [&](int i) { return i == n - 1 ? 1.0 : (double)i * step; };
  int j = (int)(x * (double)(n - 1));
  j = j < 0 ? 0 : (j > n - 1 ? n - 1 : j);
  while (j > 0 && xp(j) > x) --j;
  while (j < n - 1 && xp(j + 1) <= x) ++j;
  const double f0 = (double)key_value(keys[j]);
  if (j == n - 1 || x == xp(j)) return f0;
  const double f1 = (double)key_value(keys[j + 1]);
  const double slope = (f1 - f0) / (xp(j + 1) - xp(j));
  double r = slope * (x - xp(j)) + f0;
  if (r != r) {
    r = slope * (x - xp(j + 1)) + f1;
    if (r != r && f0 == f1) r = f0;
  }
  return r;
}

// one workgroup per pixel: share of exact zeros in the base row, sorted bias
// row, np.interp, zero what lies below.  A pixel with a non-finite bias value
// is counted and left as it is.
__global__ void __launch_bounds__(kSortBlk)
match_zero_rate_kernel(const float* __restrict__ base, int64_t D, float* bias, int64_t T,
                       double* __restrict__ min_value, int32_t* __restrict__ nonfinite) {
  extern __shared__ uint32_t keys[];
  __shared__ int zeros, bad;
  __shared__ double mv;
  const int n = (int)T;
  const int n2 = pow2_ceil(n);                   // workgroup-uniform
  if (threadIdx.x == 0) { zeros = 0; bad = 0; }
  __syncthreads();
  const float* b = base + (int64_t)blockIdx.x * D;
  float* x = bias + (int64_t)blockIdx.x * T;
  int z = 0, nf = 0;
  for (int64_t d = threadIdx.x; d < D; d += blockDim.x) z += b[d] == 0.f;
  for (int i = threadIdx.x; i < n2; i += blockDim.x) {
    uint32_t k = kPadKey;
    if (i < n) {
      const float v = x[i];
      nf += !(fabsf(v) <= 3.402823466e38f);
      k = sort_key(v);
    }
    keys[i] = k;
  }
  if (z) atomicAdd(&zeros, z);
  if (nf) atomicAdd(&bad, nf);
  __syncthreads();
  bitonic_sort(keys, n2);
  if (threadIdx.x == 0) {
    mv = bad ? (double)NAN : interp_linspace((double)zeros / (double)D, keys, n);
    if (min_value) min_value[blockIdx.x] = mv;
    if (bad) atomicAdd(nonfinite, bad);
  }
  __syncthreads();
  const double m = mv;
  if (m == m)
    for (int i = threadIdx.x; i < n; i += blockDim.x)
      if ((double)x[i] < m) x[i] = 0.f;
}

struct PresratArgs {
  const float* base;      // (P, D)
  const float* bias;      // (P, Tb)
  const float* fut;       // (P, Tf)
  int64_t D, Tb, Tf;
  int W;
  const int32_t* last_window;   // (Tf): the last window that holds the step, -1 none
  s3_bias_channel qdm;    // the three tables (P, W, Q), flags, denom_min
  float thr;              // the threshold as numpy compares it with float32 data
  float* corrected;       // (P, Tf)
  float* zero_rate;       // (P)
  float* tau;             // (P), optional
  float* z_fg;            // (P), optional
  float* tau_fut;         // (P)
  int32_t* status;        // S3_BCC_PR_* counters
};

// presrat.py:297-333 + calc_tau_fut (:138-163), one workgroup per pixel
__global__ void __launch_bounds__(kSortBlk) presrat_kernel(PresratArgs a) {
  extern __shared__ uint32_t keys[];
  __shared__ int n_fin, n_le, n_bad, n_below;
  __shared__ float s_tau;
  const int p = blockIdx.x;
  const int nb = (int)a.Tb, nf = (int)a.Tf;
  const int n2b = pow2_ceil(nb), n2f = pow2_ceil(nf);   // workgroup-uniform
  if (threadIdx.x == 0) { n_fin = 0; n_le = 0; n_bad = 0; n_below = 0; }
  __syncthreads();
  // 1) zero rate of the observations: finite values only
  const float* b = a.base + (int64_t)p * a.D;
  int fin = 0, le = 0, bad = 0;
  for (int64_t d = threadIdx.x; d < a.D; d += blockDim.x) {
    const float v = b[d];
    if (fabsf(v) <= 3.402823466e38f) { ++fin; le += v <= a.thr; }
  }
  // 2) tau: an order statistic of the historical series
  const float* h = a.bias + (int64_t)p * a.Tb;
  for (int i = threadIdx.x; i < n2b; i += blockDim.x) {
    uint32_t k = kPadKey;
    if (i < nb) {
      const float v = h[i];
      bad += !(fabsf(v) <= 3.402823466e38f);
      k = sort_key(v);
    }
    keys[i] = k;
  }
  if (fin) atomicAdd(&n_fin, fin);
  if (le) atomicAdd(&n_le, le);
  if (bad) atomicAdd(&n_bad, bad);
  __syncthreads();
  bitonic_sort(keys, n2b);
  if (threadIdx.x == 0) {
    const double rate = n_fin ? (double)n_le / (double)n_fin : (double)NAN;
    a.zero_rate[p] = (float)rate;
    float tau = NAN;
    if (rate == rate) {
      // round(rate * size): Python rounds half to even
      int64_t nth = (int64_t)rint(rate * (double)nb);
      if (nth > nb - 1) nth = nb - 1;
      tau = key_value(keys[nth]);
    }
    s_tau = tau;
    if (a.tau) a.tau[p] = tau;
    if (n_bad) atomicAdd(&a.status[S3_BCC_PR_BIAS_NONFINITE], n_bad);
  }
  __syncthreads();                               // (also: everyone is done with the keys)
  // 3) z_fg and the corrected future series, which is sorted next
  const float tau = s_tau;
  const float* f = a.fut + (int64_t)p * a.Tf;
  float* c = a.corrected + (int64_t)p * a.Tf;
  int below = 0;
  bad = 0;
  for (int i = threadIdx.x; i < n2f; i += blockDim.x) {
    uint32_t k = kPadKey;
    if (i < nf) {
      const float v = f[i];
      bad += !(fabsf(v) <= 3.402823466e38f);
      below += v < tau;
      const int w = a.last_window[i];
      const float y = w < 0 ? NAN : qdm_value(a.qdm, v, (size_t)p * a.W + w, 0);
      c[i] = y;
      k = sort_key(y);
    }
    keys[i] = k;
  }
  if (below) atomicAdd(&n_below, below);
  if (bad) atomicAdd(&a.status[S3_BCC_PR_FUT_NONFINITE], bad);
  __syncthreads();
  bitonic_sort(keys, n2f);
  if (threadIdx.x == 0) {
    const double z = (double)n_below / (double)nf;
    if (a.z_fg) a.z_fg[p] = (float)z;
    const int64_t idx = (int64_t)rint(z * (double)nf);
    if (idx > nf - 1) {                          // the reference's IndexError
      a.tau_fut[p] = NAN;
      atomicAdd(&a.status[S3_BCC_PR_INDEX], 1);
    } else {
      a.tau_fut[p] = key_value(keys[idx]);
    }
  }
}

struct KFactorArgs {
  const float* series[4];   // base, bias, fut, corrected
  int64_t len[4];
  const int32_t* ptr[3];    // window lists of base, bias, fut (corrected shares fut's)
  const int32_t* member[3];
  int W;
  double thr;
  float* k_factor;          // (P, W)
};

// presrat.py:228-249, one workgroup per pixel: four plain means per window,
// each floored at the threshold
__global__ void __launch_bounds__(kBlk) k_factor_kernel(KFactorArgs a) {
  __shared__ double red[4][kBlk];
  const int p = blockIdx.x, tid = threadIdx.x;
  for (int w = 0; w < a.W; ++w) {
    for (int s = 0; s < 4; ++s) {
      const int l = s < 3 ? s : 2;
      const int m0 = a.ptr[l][w], m1 = a.ptr[l][w + 1];
      const float* x = a.series[s] + (int64_t)p * a.len[s];
      double acc = 0.0;
      for (int i = m0 + tid; i < m1; i += kBlk) acc += (double)x[a.member[l][i]];
      red[s][tid] = acc;
    }
    __syncthreads();
    for (int st = kBlk >> 1; st > 0; st >>= 1) {
      if (tid < st)
        for (int s = 0; s < 4; ++s) red[s][tid] += red[s][tid + st];
      __syncthreads();
    }
    if (tid == 0) {
      double m[4];
      for (int s = 0; s < 4; ++s) {
        const int l = s < 3 ? s : 2;
        const int n = a.ptr[l][w + 1] - a.ptr[l][w];
        m[s] = n ? red[s][0] / (double)n : (double)NAN;    // (np.mean of nothing)
        if (m[s] == m[s] && m[s] < a.thr) m[s] = a.thr;    // np.maximum keeps a NaN
      }
      const double x = m[2] / m[1], x_hat = m[3] / m[0];
      a.k_factor[(int64_t)p * a.W + w] = (float)(x / x_hat);
    }
    __syncthreads();
  }
}

struct SkillArgs {
  const float* series[2];   // base (P, D), bias (P, T)
  int n[2];                 // D, T
  int demean;
  uint32_t* sorted_base;    // (P, D) workspace: the base row's sorted KS keys
  float* stats;             // (P, 2, S3_BCC_SK_STATS)
  int32_t* ks;              // (P, S3_BCC_SK_KS_WORDS)
  int32_t* status;          // (P, S3_BCC_SK_STATUS_WORDS)
};

// sum / maximum over the workgroup in a fixed tree (blockDim a power of two);
// called by the whole workgroup, everyone gets the result
__device__ double block_sum(double v, double* red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
  for (int s = blockDim.x >> 1; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}
__device__ long long block_max(long long v, long long* red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
  for (int s = blockDim.x >> 1; s > 0; s >>= 1) {
    if (tid < s && red[tid + s] > red[tid]) red[tid] = red[tid + s];
    __syncthreads();
  }
  const long long r = red[0];
  __syncthreads();
  return r;
}

// the key that the KS test compares: the value less the series' own fp32 mean
// (one rounding, as numpy subtracts a float32 scalar from a float32 array),
// -0 as +0 (compared as floats they tie).  Monotone: sorted keys stay sorted,
// and values that the rounding merges get one key.
__device__ __forceinline__ uint32_t ks_key(uint32_t k, float m32, int demean) {
  float v = key_value(k);
  if (demean) v = __fsub_rn(v, m32);
  if (v == 0.f) v = 0.f;
  return sort_key(v);
}

// first index in [0, n) whose key is >= b (lower) or > b (upper); n if none
__device__ __forceinline__ int lower_bound(const uint32_t* keys, int n, uint32_t b) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (keys[mid] < b) lo = mid + 1; else hi = mid;
  }
  return lo;
}
__device__ __forceinline__ int upper_bound(const uint32_t* keys, int n, uint32_t b) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (keys[mid] <= b) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// bias_calc.py:431-481, one workgroup per pixel.  Per series: the moments in
// two passes (the second over the keys in LDS), the sort, the percentiles; the
// base row's sorted KS keys go out to the workspace, the bias row's stay in
// LDS.  Then the KS counts: with c1(x) = #(base <= x), c2(x) = #(bias <= x)
// the numerator c1 T - c2 D is evaluated at every data point that can hold an
// extremum.  c1 is constant between two distinct base values while c2 grows,
// so on the stretch [b, b_next) the maximum sits at b itself (c1 = the run's
// end, c2 = upper_bound(bias, b)) and the minimum at the last bias value
// below b_next (c2 = lower_bound(bias, b_next); where there is none this is
// the value at b again).  Before the first base value c1 = 0.
__global__ void __launch_bounds__(kSortBlk) skill_kernel(SkillArgs a) {
#pragma clang fp contract(off)
  extern __shared__ uint32_t keys[];
  __shared__ double red[kSortBlk];
  __shared__ long long redi[kSortBlk];
  __shared__ int cnt[2][3];                      // per series: NaN, non-finite, zeros
  const int p = blockIdx.x, tid = threadIdx.x;
  static constexpr int pct[S3_BCC_SK_PERCENTILES] = {1, 5, 25, 50, 75, 95, 99};
  if (tid < 6) (&cnt[0][0])[tid] = 0;
  __syncthreads();
  double mu_base = 0.0;
  for (int s = 0; s < 2; ++s) {
    const int n = a.n[s];
    const int n2 = pow2_ceil(n);                 // workgroup-uniform
    const float* x = a.series[s] + (int64_t)p * n;
    // 1) keys, counts and the sum of what is not NaN
    double sum = 0.0;
    int nan = 0, nf = 0, z = 0;
    for (int i = tid; i < n2; i += blockDim.x) {
      uint32_t k = kPadKey;
      if (i < n) {
        const float v = x[i];
        k = sort_key(v);
        if (v != v) ++nan; else sum += (double)v;
        nf += !(fabsf(v) <= 3.402823466e38f);
        z += v == 0.f;
      }
      keys[i] = k;
    }
    if (nan) atomicAdd(&cnt[s][0], nan);
    if (nf) atomicAdd(&cnt[s][1], nf);
    if (z) atomicAdd(&cnt[s][2], z);
    sum = block_sum(sum, red);                   // (its barriers publish keys and counts)
    const int n_nan = cnt[s][0], n_ok = n - n_nan;
    const double mu = n_ok ? sum / (double)n_ok : (double)NAN;
    const float m32 = (float)mu;
    // 2) central moments about the fp64 mean
    double s2 = 0.0, s3 = 0.0, s4 = 0.0;
    for (int i = tid; i < n; i += blockDim.x) {
      const uint32_t k = keys[i];
      if (k == kNanKey) continue;
      const double d = (double)key_value(k) - mu, d2 = d * d;
      s2 += d2;
      s3 += d2 * d;
      s4 += d2 * d2;
    }
    s2 = block_sum(s2, red);
    s3 = block_sum(s3, red);
    s4 = block_sum(s4, red);
    bitonic_sort(keys, n2);
    float* out = a.stats + ((int64_t)p * 2 + s) * S3_BCC_SK_STATS;
    if (tid < S3_BCC_SK_PERCENTILES) {
      // np.percentile: window_quantiles_kernel's interpolation at (n - 1) p / 100
      float v = NAN;
      if (!n_nan) {
        const double pos = (double)(n - 1) * ((double)pct[tid] / 100.0);
        int lo = (int)pos;
        if (lo > n - 1) lo = n - 1;
        const double frac = pos - (double)lo;
        const double va = (double)key_value(keys[lo]);
        const uint32_t kb = keys[lo + 1 > n - 1 ? lo : lo + 1];
        if (frac == 0.0 || kb == keys[lo]) {
          v = (float)va;
        } else {
          const double vb = (double)key_value(kb);
          v = (float)(va + (vb - va) * frac);
        }
      }
      out[S3_BCC_SK_PCT0 + tid] = v;
    } else if (tid == 64) {                       // (a wave of its own)
      out[S3_BCC_SK_MEAN] = m32;
      out[S3_BCC_SK_STD] = n_ok ? (float)sqrt(s2 / (double)n_ok) : NAN;
      // scipy.stats.skew / kurtosis (biased, Fisher) of float32 data: every
      // value counts, so a NaN gives NaN; NaN too where m2 <= (eps32 mean)^2
      float skew = NAN, kurt = NAN;
      if (!n_nan) {
        const double m2 = s2 / (double)n, m3 = s3 / (double)n, m4 = s4 / (double)n;
        const double tiny = 1.1920928955078125e-07 * mu;
        if (!(m2 <= tiny * tiny)) {
          skew = (float)(m3 / (m2 * sqrt(m2)));
          kurt = (float)(m4 / (m2 * m2) - 3.0);
        }
      }
      out[S3_BCC_SK_SKEW] = skew;
      out[S3_BCC_SK_KURTOSIS] = kurt;
      out[S3_BCC_SK_ZERO_RATE] = (float)((double)cnt[s][2] / (double)n);
      if (s == 1) {
        // the bias of the means from the fp64 means, rounded once
        const float diff = (float)(mu - mu_base);
        out[S3_BCC_SK_BIAS] = diff;
        out[S3_BCC_SK_BIAS - S3_BCC_SK_STATS] = diff;
      }
      a.status[(int64_t)p * S3_BCC_SK_STATUS_WORDS + 2 * s] = n_nan;
      a.status[(int64_t)p * S3_BCC_SK_STATUS_WORDS + 2 * s + 1] = cnt[s][1];
    }
    // 3) the KS keys: base out to the workspace, bias in place
    if (s == 0) {
      mu_base = mu;
      uint32_t* ws = a.sorted_base + (int64_t)p * n;
      for (int i = tid; i < n; i += blockDim.x) ws[i] = ks_key(keys[i], m32, a.demean);
    } else {
      __syncthreads();                           // the percentiles have read the keys
      for (int i = tid; i < n; i += blockDim.x) keys[i] = ks_key(keys[i], m32, a.demean);
    }
    __syncthreads();                             // (also makes the workspace row visible to the workgroup)
  }
  // 4) the KS counts
  const int D = a.n[0], T = a.n[1];
  const uint32_t* ws = a.sorted_base + (int64_t)p * D;
  constexpr long long kFar = 1ll << 62;
  long long hi = -kFar, lo = kFar, c1_hi = kFar, c1_lo = kFar;
  for (int i = tid; i < D; i += blockDim.x) {
    const uint32_t b = ws[i];
    const bool last = i == D - 1;
    const uint32_t bn = last ? 0u : ws[i + 1];
    if (i == 0) {
      lo = -(long long)lower_bound(keys, T, b) * D;
      c1_lo = 0;
    }
    if (!last && bn == b) continue;              // not the end of a run of equal keys
    const long long c1 = i + 1;
    const long long up = c1 * T - (long long)upper_bound(keys, T, b) * D;
    const long long dn = c1 * T - (long long)(last ? T : lower_bound(keys, T, bn)) * D;
    if (up > hi) { hi = up; c1_hi = c1; }
    const long long m = up < dn ? up : dn;
    if (m < lo) { lo = m; c1_lo = c1; }
  }
  // the extrema, then the smallest c1 that reaches each: c2 follows from both
  const long long n_hi = block_max(hi, redi);
  const long long n_lo = -block_max(-lo, redi);
  const long long w_hi = -block_max(hi == n_hi ? -c1_hi : -kFar, redi);
  const long long w_lo = -block_max(lo == n_lo ? -c1_lo : -kFar, redi);
  if (tid == 0) {
    int32_t* ks = a.ks + (int64_t)p * S3_BCC_SK_KS_WORDS;
    const bool bad = cnt[0][0] || cnt[1][0] || (a.demean && (cnt[0][1] || cnt[1][1]));
    ks[0] = bad ? S3_BCC_SK_NO_KS : (int32_t)w_hi;
    ks[1] = bad ? S3_BCC_SK_NO_KS : (int32_t)((w_hi * T - n_hi) / D);
    ks[2] = bad ? S3_BCC_SK_NO_KS : (int32_t)w_lo;
    ks[3] = bad ? S3_BCC_SK_NO_KS : (int32_t)((w_lo * T - n_lo) / D);
  }
}

// 0 <= ptr[0] <= ptr[1] <= .. <= ptr[n] == total, every idx in [0, limit)
bool csr_ok(const int32_t* ptr, int n, const int32_t* idx, int64_t limit) {
  if (ptr[0] != 0) return false;
  for (int i = 0; i < n; ++i)
    if (ptr[i + 1] < ptr[i]) return false;
  for (int i = 0; i < ptr[n]; ++i)
    if (idx[i] < 0 || idx[i] >= limit) return false;
  return true;
}

int allow_big_lds(s3_ctx* ctx) {
  static S3DeviceOnce attr_set;
  if (int rc = s3_lds_optin(ctx, attr_set,
                            window_quantiles_kernel, kMaxSort * 4,
                            match_zero_rate_kernel, kMaxSort * 4,
                            presrat_kernel, kMaxSort * 4,
                            skill_kernel, kMaxSort * 4)) return rc;
  return S3_OK;
}

constexpr int64_t kI31 = (int64_t)1 << 31;

}  // namespace

extern "C" int s3_bc_base_series(s3_ctx* ctx, const float* base, const float* cs_ghi, int64_t T, int64_t n_sites,
                                 int P, const int32_t* site_ptr_host, const int32_t* site_idx_host,
                                 const int32_t* site_ptr, const int32_t* site_idx, int n_days,
                                 const int32_t* day_ptr_host, const int32_t* step_idx_host,
                                 const int32_t* day_ptr, const int32_t* step_idx, int reduction, uint32_t flags,
                                 int decimals, int64_t D_total, int64_t day_offset, float* out) {
  if (!ctx) return S3_EINVAL;
  if (!base || !out || !site_ptr_host || !site_idx_host || !site_ptr || !site_idx || !day_ptr_host ||
      !step_idx_host || !day_ptr || !step_idx)
    S3_FAIL(ctx, S3_EINVAL, "bc_base_series: base, out and both copies of the site and day lists are needed");
  if (T < 1 || n_sites < 1 || P < 1 || n_days < 1 || D_total < 1)
    S3_FAIL(ctx, S3_EINVAL, "bc_base_series: empty extent");
  if (T * n_sites >= kI31 || (int64_t)P * D_total >= kI31)
    S3_FAIL(ctx, S3_EINVAL, "bc_base_series: 2^31 or more elements");
  if (reduction < S3_BCC_AVG || reduction > S3_BCC_NONE)
    S3_FAIL(ctx, S3_EINVAL, "bc_base_series: unknown daily reduction");
  if ((flags & S3_BCC_CS_RATIO) && (!cs_ghi || reduction != S3_BCC_AVG))
    S3_FAIL(ctx, S3_EINVAL, "bc_base_series: the clearsky ratio needs cs_ghi and the avg reduction");
  if (day_offset < 0 || day_offset + n_days > D_total)
    S3_FAIL(ctx, S3_EINVAL, "bc_base_series: the days leave the output series");
  if ((flags & S3_BCC_ROUND) && (decimals < -9 || decimals > 9))
    S3_FAIL(ctx, S3_EINVAL, "bc_base_series: decimals outside -9 .. 9");
  if (!csr_ok(site_ptr_host, P, site_idx_host, n_sites))
    S3_FAIL(ctx, S3_EINVAL, "bc_base_series: site list out of range");
  if (!csr_ok(day_ptr_host, n_days, step_idx_host, T))
    S3_FAIL(ctx, S3_EINVAL, "bc_base_series: day list out of range");
  if (reduction == S3_BCC_NONE)
    for (int d = 0; d < n_days; ++d)
      if (day_ptr_host[d + 1] - day_ptr_host[d] != 1)
        S3_FAIL(ctx, S3_EINVAL, "bc_base_series: without a reduction every output step is one input step");
  const int64_t chunks = (P + kBlk - 1) / kBlk;
  if (chunks * n_days >= kI31) S3_FAIL(ctx, S3_EINVAL, "bc_base_series: 2^31 or more elements");
  BaseArgs a;
  a.base = base; a.cs = cs_ghi; a.T = T; a.n_sites = n_sites; a.P = P; a.n_days = n_days;
  a.reduction = reduction == S3_BCC_NONE ? S3_BCC_AVG : reduction;
  a.nanskip = (flags & S3_BCC_NANSKIP) != 0;
  a.cs_ratio = (flags & S3_BCC_CS_RATIO) != 0;
  a.round_on = (flags & S3_BCC_ROUND) != 0;
  a.round_neg = decimals < 0;
  float p10 = 1.f;
  for (int i = 0; i < (decimals < 0 ? -decimals : decimals); ++i) p10 *= 10.f;
  a.p10 = p10;
  a.site_ptr = site_ptr; a.site_idx = site_idx; a.day_ptr = day_ptr; a.step_idx = step_idx;
  a.D_total = D_total; a.day_offset = day_offset; a.out = out;
  hipLaunchKernelGGL(base_series_kernel, dim3((unsigned)(chunks * n_days)), dim3(kBlk), 0, ctx->stream, a);
  S3_HIP(ctx, hipGetLastError());
  return S3_OK;
}

extern "C" int s3_bc_moments(s3_ctx* ctx, const float* series, int P, int64_t T, const int32_t* group_host,
                             const int32_t* group, int NT, int32_t* count, float* mean, float* sd) {
  if (!ctx) return S3_EINVAL;
  if (!series || !group_host || !group || !count || !mean || !sd)
    S3_FAIL(ctx, S3_EINVAL, "bc_moments: series, both copies of the group ids and the three outputs are needed");
  if (P < 1 || T < 1) S3_FAIL(ctx, S3_EINVAL, "bc_moments: empty extent");
  if (NT < 1 || NT > kMaxGroups) S3_FAIL(ctx, S3_EINVAL, "bc_moments: 1 .. 12 groups");
  if ((int64_t)P * T >= kI31) S3_FAIL(ctx, S3_EINVAL, "bc_moments: 2^31 or more elements");
  for (int64_t t = 0; t < T; ++t)
    if (group_host[t] < -1 || group_host[t] >= NT) S3_FAIL(ctx, S3_EINVAL, "bc_moments: group id out of range");
  hipLaunchKernelGGL(moments_kernel, dim3((unsigned)P), dim3(kBlk), 0, ctx->stream, series, T, group, NT, count,
                     mean, sd);
  S3_HIP(ctx, hipGetLastError());
  return S3_OK;
}

extern "C" int s3_bc_window_quantiles(s3_ctx* ctx, const float* series, int P, int64_t T, int W,
                                      const int32_t* win_ptr_host, const int32_t* member_host,
                                      const int32_t* win_ptr, const int32_t* member, int Q, float* out) {
  if (!ctx) return S3_EINVAL;
  if (Q < 1) S3_FAIL(ctx, S3_EINVAL, "bc_window_quantiles: at least one quantile");
  if (!series || !win_ptr_host || !member_host || !win_ptr || !member || !out)
    S3_FAIL(ctx, S3_EINVAL, "bc_window_quantiles: series, out and both copies of the member lists are needed");
  if (P < 1 || T < 1 || W < 1) S3_FAIL(ctx, S3_EINVAL, "bc_window_quantiles: empty extent");
  if ((int64_t)P * T >= kI31 || (int64_t)P * W * Q >= kI31 || (int64_t)P * W >= kI31)
    S3_FAIL(ctx, S3_EINVAL, "bc_window_quantiles: 2^31 or more elements");
  if (!csr_ok(win_ptr_host, W, member_host, T))
    S3_FAIL(ctx, S3_EINVAL, "bc_window_quantiles: window member out of range");
  int longest = 0;
  for (int w = 0; w < W; ++w) longest = std::max(longest, win_ptr_host[w + 1] - win_ptr_host[w]);
  if (longest > kMaxSort)
    S3_FAIL(ctx, S3_EINVAL, "bc_window_quantiles: a window has more than S3_BCC_MAX_SORT (32768) members");
  const int n2 = pow2_ceil(longest);
  if (int rc = allow_big_lds(ctx)) return rc;
  const int blk = n2 > 8192 ? kSortBlk : kBlk;
  hipLaunchKernelGGL(window_quantiles_kernel, dim3((unsigned)((int64_t)P * W)), dim3(blk), (size_t)n2 * 4,
                     ctx->stream, series, T, W, win_ptr, member, Q, out);
  S3_HIP(ctx, hipGetLastError());
  return S3_OK;
}

extern "C" int s3_bc_match_zero_rate(s3_ctx* ctx, const float* base, int64_t D, float* bias, int P, int64_t T,
                                     double* min_value, int32_t* nonfinite) {
  if (!ctx) return S3_EINVAL;
  if (!base || !bias || !nonfinite)
    S3_FAIL(ctx, S3_EINVAL, "bc_match_zero_rate: base, bias and the counter are needed");
  if (P < 1 || T < 1 || D < 1) S3_FAIL(ctx, S3_EINVAL, "bc_match_zero_rate: empty extent");
  if (T > kMaxSort)
    S3_FAIL(ctx, S3_EINVAL, "bc_match_zero_rate: a series has more than S3_BCC_MAX_SORT (32768) steps");
  if ((int64_t)P * D >= kI31) S3_FAIL(ctx, S3_EINVAL, "bc_match_zero_rate: 2^31 or more elements");
  const int n2 = pow2_ceil((int)T);
  if (int rc = allow_big_lds(ctx)) return rc;
  const int blk = n2 > 8192 ? kSortBlk : kBlk;
  hipLaunchKernelGGL(match_zero_rate_kernel, dim3((unsigned)P), dim3(blk), (size_t)n2 * 4, ctx->stream, base, D,
                     bias, T, min_value, nonfinite);
  S3_HIP(ctx, hipGetLastError());
  return S3_OK;
}

extern "C" int s3_bc_presrat(s3_ctx* ctx, const float* base, int64_t D, const float* bias, int64_t Tb,
                             const float* fut, int64_t Tf, int P, int W, int Q, const float* base_params,
                             const float* bias_params, const float* fut_params, int relative,
                             double zero_rate_threshold, const int32_t* last_window_host,
                             const int32_t* last_window, const int32_t* const* win_ptr_host,
                             const int32_t* const* member_host, const int32_t* const* win_ptr,
                             const int32_t* const* member, float* corrected, float* zero_rate, float* tau,
                             float* z_fg, float* tau_fut, float* k_factor, int32_t* status) {
  if (!ctx) return S3_EINVAL;
  if (!base || !bias || !fut || !base_params || !bias_params || !fut_params || !last_window_host ||
      !last_window || !win_ptr_host || !member_host || !win_ptr || !member || !corrected || !zero_rate ||
      !tau_fut || !k_factor || !status)
    S3_FAIL(ctx, S3_EINVAL, "bc_presrat: the three series, their tables, the window lists and the outputs are needed");
  if (P < 1 || W < 1 || D < 1 || Tb < 1 || Tf < 1) S3_FAIL(ctx, S3_EINVAL, "bc_presrat: empty extent");
  if (Q < 2) S3_FAIL(ctx, S3_EINVAL, "bc_presrat: the mapping needs two quantiles");
  if (Tb > kMaxSort || Tf > kMaxSort)
    S3_FAIL(ctx, S3_EINVAL, "bc_presrat: a series has more than S3_BCC_MAX_SORT (32768) steps");
  if ((int64_t)P * D >= kI31 || (int64_t)P * W * Q >= kI31)
    S3_FAIL(ctx, S3_EINVAL, "bc_presrat: 2^31 or more elements");
  for (int64_t t = 0; t < Tf; ++t)
    if (last_window_host[t] < -1 || last_window_host[t] >= W)
      S3_FAIL(ctx, S3_EINVAL, "bc_presrat: window index out of range");
  const int64_t len[3] = {D, Tb, Tf};
  for (int l = 0; l < 3; ++l)
    if (!win_ptr_host[l] || !member_host[l] || !win_ptr[l] || !member[l] ||
        !csr_ok(win_ptr_host[l], W, member_host[l], len[l]))
      S3_FAIL(ctx, S3_EINVAL, "bc_presrat: window member out of range");
  if (int rc = allow_big_lds(ctx)) return rc;
  PresratArgs a = {};
  a.base = base; a.bias = bias; a.fut = fut; a.D = D; a.Tb = Tb; a.Tf = Tf; a.W = W;
  a.last_window = last_window;
  a.qdm.kind = S3_BC_QDM;
  a.qdm.flags = relative ? (S3_BC_RELATIVE | S3_BC_DENOM_MIN) : 0u;
  a.qdm.n_t = W; a.qdm.n_q = Q;
  a.qdm.oh = base_params; a.qdm.mh = bias_params; a.qdm.mf = fut_params;
  a.qdm.denom_min = (float)zero_rate_threshold;
  a.thr = (float)zero_rate_threshold;
  a.corrected = corrected; a.zero_rate = zero_rate; a.tau = tau; a.z_fg = z_fg; a.tau_fut = tau_fut;
  a.status = status;
  S3_HIP(ctx, hipMemsetAsync(status, 0, S3_BCC_PR_STATUS_WORDS * sizeof(int32_t), ctx->stream));
  const int n2 = pow2_ceil((int)std::max(Tb, Tf));
  const int blk = n2 > 8192 ? kSortBlk : kBlk;
  hipLaunchKernelGGL(presrat_kernel, dim3((unsigned)P), dim3(blk), (size_t)n2 * 4, ctx->stream, a);
  S3_HIP(ctx, hipGetLastError());
  KFactorArgs k = {};
  k.series[0] = base; k.series[1] = bias; k.series[2] = fut; k.series[3] = corrected;
  k.len[0] = D; k.len[1] = Tb; k.len[2] = Tf; k.len[3] = Tf;
  for (int l = 0; l < 3; ++l) { k.ptr[l] = win_ptr[l]; k.member[l] = member[l]; }
  k.W = W; k.thr = zero_rate_threshold; k.k_factor = k_factor;
  hipLaunchKernelGGL(k_factor_kernel, dim3((unsigned)P), dim3(kBlk), 0, ctx->stream, k);
  S3_HIP(ctx, hipGetLastError());
  return S3_OK;
}

extern "C" int s3_bc_skill(s3_ctx* ctx, const float* base, int64_t D, const float* bias, int64_t T, int P,
                           int demean, uint32_t* sorted_base, float* stats, int32_t* ks, int32_t* status) {
  if (!ctx) return S3_EINVAL;
  if (!base || !bias || !sorted_base || !stats || !ks || !status)
    S3_FAIL(ctx, S3_EINVAL, "bc_skill: base, bias, the workspace and the three outputs are needed");
  if (P < 1 || D < 1 || T < 1) S3_FAIL(ctx, S3_EINVAL, "bc_skill: empty extent");
  if (D > kMaxSort || T > kMaxSort)
    S3_FAIL(ctx, S3_EINVAL, "bc_skill: a series has more than S3_BCC_MAX_SORT (32768) steps");
  if ((int64_t)P * D >= kI31 || (int64_t)P * T >= kI31)
    S3_FAIL(ctx, S3_EINVAL, "bc_skill: 2^31 or more elements");
  if (int rc = allow_big_lds(ctx)) return rc;
  SkillArgs a = {};
  a.series[0] = base; a.series[1] = bias; a.n[0] = (int)D; a.n[1] = (int)T; a.demean = demean != 0;
  a.sorted_base = sorted_base; a.stats = stats; a.ks = ks; a.status = status;
  const int n2 = pow2_ceil((int)std::max(D, T));
  const int blk = n2 > 8192 ? kSortBlk : kBlk;
  hipLaunchKernelGGL(skill_kernel, dim3((unsigned)P), dim3(blk), (size_t)n2 * 4, ctx->stream, a);
  S3_HIP(ctx, hipGetLastError());
  return S3_OK;
}
