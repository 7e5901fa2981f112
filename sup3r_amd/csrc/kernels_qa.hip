// QA of a forward pass on the device (sup3r/qa/qa.py, sup3r/qa/utilities.py):
//   s3_qa_recoarsen   the high-resolution output re-coarsened onto the source
//                     grid, the error against the source and its five summary
//                     words, one read of the field;
//   s3_qa_select      the two order statistics of |d| that np.percentile
//                     (method='linear') interpolates between: an exact radix
//                     select over the bit patterns of |d|;
//   s3_qa_hist        count, sum d^2, min, max of the kept values and
//                     np.histogram's counts over uniform bins;
//   s3_qa_power_sum   sum of re^2 + im^2 over the axes a spectrum averages.
// This file is compiled with -ffp-contract=off: every fp32 operation below is
// one correctly rounded numpy operation, in the order tests/qa_ref.py states.
//
// Re-coarsening order (per output element): per high-resolution time step the
// s row sums over j in order, their sum over i in order, one true division by
// float(s^2); then the t_enhance steps in order by the S3_TC_* method (total /
// average count NaN as +0, max / min hand NaN on).
//
// Sums that cross lanes are fp64 and folded in a fixed order: lanes by a
// butterfly, waves through LDS, workgroups by a second kernel.  No float
// atomics; the histograms use integer atomics only.  Two runs give equal bits.
#include "common.h"

namespace {

constexpr int kBlk = kBlock;
constexpr int kWaves = kBlk / 64;
constexpr int kMaxF = S3_QA_MAX_FEATURES;
constexpr int kWords = S3_QA_SUMMARY_WORDS;
constexpr int kCubeTile = 4096;           // floats of one pixel's row a cube workgroup keeps in LDS
constexpr int kMaxBins = S3_QA_MAX_BINS;

__device__ __forceinline__ float nan0(float v) { return v != v ? 0.f : v; }

// the t_enhance values p[0], p[stride], ... folded in order
__device__ __forceinline__ float tfold(const float* p, int stride, int te, int method) {
  float a = p[0];
  switch (method) {
    case S3_TC_SUBSAMPLE:
      return a;
    case S3_TC_MAX:                     // np.maximum: (a >= b || isnan(a)) ? a : b
      for (int k = 1; k < te; ++k) { const float b = p[k * stride]; a = (a >= b || a != a) ? a : b; }
      return a;
    case S3_TC_MIN:
      for (int k = 1; k < te; ++k) { const float b = p[k * stride]; a = (a <= b || a != a) ? a : b; }
      return a;
    default:                            // np.nansum, then the division of 'average'
      a = nan0(a);
      for (int k = 1; k < te; ++k) a = __fadd_rn(a, nan0(p[k * stride]));
      return method == S3_TC_AVERAGE ? __fdiv_rn(a, (float)te) : a;
  }
}

// the summary of the finite errors a lane met
struct Acc {
  double n, s, sa, sq;
  float mx;
};
__device__ __forceinline__ Acc acc_zero() { return Acc{0.0, 0.0, 0.0, 0.0, 0.f}; }
__device__ __forceinline__ void acc_add(Acc& a, float e) {
  if (!__builtin_isfinite(e)) return;
  const double d = (double)e;
  a.n += 1.0; a.s += d; a.sa += __builtin_fabs(d); a.sq += d * d;
  a.mx = __builtin_fmaxf(a.mx, __builtin_fabsf(e));
}
__device__ __forceinline__ void acc_merge(Acc& a, const Acc& b) {
  a.n += b.n; a.s += b.s; a.sa += b.sa; a.sq += b.sq;
  a.mx = __builtin_fmaxf(a.mx, b.mx);
}
// butterfly over the 64 lanes: a fixed tree, every lane ends with the wave's total
__device__ __forceinline__ Acc acc_wave(Acc a) {
  for (int o = 32; o > 0; o >>= 1) {
    Acc b;
    b.n = __shfl_xor(a.n, o); b.s = __shfl_xor(a.s, o); b.sa = __shfl_xor(a.sa, o);
    b.sq = __shfl_xor(a.sq, o); b.mx = __shfl_xor(a.mx, o);
    acc_merge(a, b);
  }
  return a;
}

struct RcArgs {
  const float* tru[kMaxF];
  float* syn[kMaxF];
  float* err[kMaxF];
  int ch[kMaxF];
  int method[kMaxF];
};

// one output element: store, subtract, summarise
__device__ __forceinline__ void rc_finish(const RcArgs& a, int f, int64_t idx, float v, bool stats, Acc& acc) {
  if (a.syn[f]) a.syn[f][idx] = v;
  if (a.tru[f]) {
    const float e = __fsub_rn(v, a.tru[f][idx]);
    if (a.err[f]) a.err[f][idx] = e;
    if (stats) acc_add(acc, e);
  }
}

// the waves' summaries of feature f -> sm; after the workgroup's last feature
// rc_flush folds them in wave order
__device__ __forceinline__ void rc_stash(Acc (*sm)[kWaves], int f, Acc acc) {
  acc = acc_wave(acc);
  if ((threadIdx.x & 63) == 0) sm[f][threadIdx.x >> 6] = acc;
}
__device__ __forceinline__ void rc_flush(Acc (*sm)[kWaves], int F, double* __restrict__ partial) {
  __syncthreads();
  if ((int)threadIdx.x < F) {
    Acc a = sm[threadIdx.x][0];
    for (int w = 1; w < kWaves; ++w) acc_merge(a, sm[threadIdx.x][w]);
    double* p = partial + ((int64_t)blockIdx.x * F + threadIdx.x) * kWords;
    p[0] = a.n; p[1] = a.s; p[2] = a.sa; p[3] = a.sq; p[4] = (double)a.mx;
  }
}

// Cube (H1, H2, HT, C): a workgroup owns one low-res pixel and TT of its steps.
// Pass 1: lanes along the contiguous (step, channel) run, s^2 loads each, the
// spatial means to LDS.  Pass 2: lanes along the low-res steps of one feature.
// SS = s_enhance at compile time (the s^2 loads of an element are then issued
// together), 0 = any.
template <int SS>
__global__ void __launch_bounds__(kBlk)
qa_recoarsen_cube_kernel(const float* __restrict__ hr, int64_t H2, int64_t HT, int C, int S2, int T, int F, int s_rt,
                         int te, int TT, int nchunk, RcArgs a, double* __restrict__ partial) {
  __shared__ float lds[kCubeTile];
  __shared__ Acc sm[kMaxF][kWaves];
  const int s = SS ? SS : s_rt;
  const int tid = threadIdx.x;
  const int64_t pix = blockIdx.x / nchunk;
  const int chunk = blockIdx.x % nchunk;
  const int64_t I = pix / S2, J = pix % S2;
  const int tt0 = chunk * TT;
  const int ttn = T - tt0 < TT ? T - tt0 : TT;
  const int n_el = ttn * te * C;
  const int64_t row_j = HT * C, row_i = H2 * row_j;
  const float* base = hr + (I * s) * row_i + (J * s) * row_j + (int64_t)tt0 * te * C;
  const float s2f = (float)(s * s);
  for (int e = tid; e < n_el; e += kBlk) {
    float tot = 0.f;
    for (int i = 0; i < s; ++i) {
      const float* r = base + i * row_i + e;
      float rs = r[0];
      for (int j = 1; j < s; ++j) rs = __fadd_rn(rs, r[j * row_j]);
      tot = i == 0 ? rs : __fadd_rn(tot, rs);
    }
    lds[e] = __fdiv_rn(tot, s2f);
  }
  __syncthreads();
  for (int f = 0; f < F; ++f) {
    Acc acc = acc_zero();
    const int ch = a.ch[f], method = a.method[f];
    for (int tl = tid; tl < ttn; tl += kBlk) {
      const float v = tfold(&lds[tl * te * C + ch], C, te, method);
      rc_finish(a, f, pix * T + tt0 + tl, v, partial != nullptr, acc);
    }
    if (partial) rc_stash(sm, f, acc);
  }
  if (partial) rc_flush(sm, F, partial);
}

// Time-first (HT, H1, H2): a workgroup owns low-res row I, JW = 64 / s columns
// and TT steps; its four waves share the steps.  A wave loads one hi-res row
// segment of JW s floats per (step, i), a lane per float; the lane at the head
// of each group of s takes its neighbours' values by shuffles and adds them in
// j order, then the s rows in i order, and writes the mean to tile[J][k] (odd
// row stride).  Then lanes along the low-res steps fold the t_enhance means
// and store runs of T.
template <int SS>
__global__ void __launch_bounds__(kBlk)
qa_recoarsen_tfirst_kernel(const float* __restrict__ hr, int64_t H1, int64_t H2, int S2, int T, int s_rt, int te,
                           int TT, int nJ, int nchunk, RcArgs a, double* __restrict__ partial) {
  extern __shared__ float tile[];            // [JW][RS]
  __shared__ Acc sm[1][kWaves];
  const int s = SS ? SS : s_rt;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int JW = 64 / s, RS = (TT * te) | 1;
  const int chunk = blockIdx.x % nchunk;
  const int jb = (blockIdx.x / nchunk) % nJ;
  const int64_t I = blockIdx.x / nchunk / nJ;
  const int J0 = jb * JW, tt0 = chunk * TT;
  const int jn = S2 - J0 < JW ? S2 - J0 : JW;
  const int ttn = T - tt0 < TT ? T - tt0 : TT;
  const int kn = ttn * te, wn = jn * s;
  const int64_t k0 = (int64_t)tt0 * te;
  const float s2f = (float)(s * s);
  const bool act = lane < wn;
  const bool head = act && lane % s == 0;
  const float* col = hr + (I * s) * H2 + (int64_t)J0 * s + lane;
  for (int k = wave; k < kn; k += kWaves) {
    const float* p = col + (k0 + k) * H1 * H2;
    float tot = 0.f;
    for (int i = 0; i < s; ++i) {
      const float x = act ? p[i * H2] : 0.f;
      float rs = x;
      for (int j = 1; j < s; ++j) rs = __fadd_rn(rs, __shfl_down(x, j));
      tot = i == 0 ? rs : __fadd_rn(tot, rs);
    }
    if (head) tile[(lane / s) * RS + k] = __fdiv_rn(tot, s2f);
  }
  __syncthreads();
  Acc acc = acc_zero();
  const int method = a.method[0];
  for (int o = tid; o < jn * ttn; o += kBlk) {
    const int jl = o / ttn, tl = o - jl * ttn;
    const float v = tfold(&tile[jl * RS + tl * te], 1, te, method);
    rc_finish(a, 0, (I * S2 + J0 + jl) * T + tt0 + tl, v, partial != nullptr, acc);
  }
  if (partial) {
    rc_stash(sm, 0, acc);
    rc_flush(sm, 1, partial);
  }
}

// workgroup f: the workgroups' partials of feature f, lane b % 256 takes
// workgroup b, then a fixed tree
__global__ void __launch_bounds__(kBlk)
qa_summary_fold_kernel(const double* __restrict__ partial, int nblk, int F, double* __restrict__ out) {
  __shared__ Acc sm[kBlk];
  const int f = blockIdx.x, tid = threadIdx.x;
  Acc a = acc_zero();
  for (int b = tid; b < nblk; b += kBlk) {
    const double* p = partial + ((int64_t)b * F + f) * kWords;
    acc_merge(a, Acc{p[0], p[1], p[2], p[3], (float)p[4]});
  }
  sm[tid] = a;
  __syncthreads();
  for (int st = kBlk / 2; st > 0; st >>= 1) {
    if (tid < st) { Acc p = sm[tid]; acc_merge(p, sm[tid + st]); sm[tid] = p; }
    __syncthreads();
  }
  if (tid == 0) {
    double* o = out + (int64_t)f * kWords;
    o[0] = sm[0].n; o[1] = sm[0].s; o[2] = sm[0].sa; o[3] = sm[0].sq; o[4] = (double)sm[0].mx;
  }
}

// ---- the transformed value d of the distributions, never stored -------------
struct QaX {
  int diff, has_period;
  float period, half, scale;
  FastDiv inner_out;             // element e of d reads v[(e / inner_out) inner_in + e % inner_out (+ delta)]
  int64_t inner_in, delta;
};

// numpy's float32 `%` (npy_remainderf): fmodf, then the divisor's sign
__device__ __forceinline__ float np_mod(float x, float b) {
  float m = fmodf(x, b);
  if (b == 0.f) return m;
  if (m != 0.f) { if ((b < 0.f) != (m < 0.f)) m = __fadd_rn(m, b); }
  else m = copysignf(0.f, b);
  return m;
}

__device__ __forceinline__ float qa_value(const QaX& x, const float* __restrict__ v, uint32_t e) {
  float d;
  if (x.diff) {
    const uint32_t q = x.inner_out(e);
    const int64_t src = (int64_t)q * x.inner_in + (e - q * x.inner_out.d);
    d = __fsub_rn(v[src + x.delta], v[src]);
    if (x.has_period) d = __fsub_rn(np_mod(__fadd_rn(d, x.half), x.period), x.half);
  } else {
    d = v[e];
    if (x.has_period) d = np_mod(__fadd_rn(d, x.period), x.period);
  }
  return __fdiv_rn(d, x.scale);
}

// +1 to h[bin] for the lanes with `on`: the lanes that share the first such
// lane's bin add once, together (a field that falls into few bins would
// otherwise serialise on one LDS word)
__device__ __forceinline__ void lds_count(uint32_t* h, uint32_t bin, bool on) {
  const uint64_t m = __ballot(on);
  if (!m) return;
  const int lane = threadIdx.x & 63;
  const int leader = __ffsll((unsigned long long)m) - 1;
  const uint32_t lb = __shfl(bin, leader);
  const bool same = on && bin == lb;
  const uint64_t sm = __ballot(same);
  if (lane == leader) atomicAdd(&h[lb], (uint32_t)__popcll(sm));
  if (on && !same) atomicAdd(&h[bin], 1u);
}

// select state in the context's scratch: words 0, 1 the two prefixes, 2, 3 the
// two ranks, 4 the NaN count, 8 .. 519 the two histograms of a pass
constexpr int kSelHist = 8, kSelWords = kSelHist + 512;

__global__ void qa_select_init_kernel(uint32_t* __restrict__ st, uint32_t r0, uint32_t r1) {
  for (int i = threadIdx.x; i < kSelWords; i += blockDim.x) st[i] = i == 2 ? r0 : i == 3 ? r1 : 0u;
}

__global__ void __launch_bounds__(kBlk)
qa_select_hist_kernel(QaX x, const float* __restrict__ v, uint32_t n, int pass, uint32_t* __restrict__ st) {
  __shared__ uint32_t h[512];
  const int tid = threadIdx.x;
  h[tid] = 0; h[tid + 256] = 0;
  const uint32_t p0 = st[0], p1 = st[1];
  const int shift = 24 - 8 * pass;
  const uint32_t hi = pass == 0 ? 0u : 0xFFFFFFFFu << (shift + 8);
  const bool two = p0 != p1;
  __syncthreads();
  uint32_t nan = 0;
  const uint32_t stride = gridDim.x * kBlk;
  // (every lane of a wave runs every trip: the ballots of lds_count need them)
  for (uint32_t base = blockIdx.x * kBlk; base < n; base += stride) {
    const uint32_t e = base + tid;
    const bool valid = e < n;
    const float d = valid ? qa_value(x, v, e) : 0.f;
    if (pass == 0 && d != d) ++nan;
    const uint32_t key = __float_as_uint(__builtin_fabsf(d));
    const uint32_t dig = (key >> shift) & 255u;
    lds_count(h, dig, valid && (key & hi) == p0);
    if (two && valid && (key & hi) == p1) atomicAdd(&h[256 + dig], 1u);
    if (stride > 0xFFFFFFFFu - base) break;               // (base + stride would wrap)
  }
  __syncthreads();
  if (h[tid]) atomicAdd(&st[kSelHist + tid], h[tid]);
  if (two && h[tid + 256]) atomicAdd(&st[kSelHist + 256 + tid], h[tid + 256]);
  if (nan) atomicAdd(&st[4], nan);
}

// one workgroup: the digit of each rank from the pass's histograms, which are
// zeroed for the next pass; after the last pass the 16 bytes of the result
__global__ void __launch_bounds__(256)
qa_select_scan_kernel(uint32_t* __restrict__ st, int pass, uint32_t* __restrict__ out) {
  __shared__ uint32_t h[512];
  const int tid = threadIdx.x;
  h[tid] = st[kSelHist + tid]; h[tid + 256] = st[kSelHist + 256 + tid];
  __syncthreads();
  st[kSelHist + tid] = 0; st[kSelHist + 256 + tid] = 0;
  if (tid != 0) return;
  const int shift = 24 - 8 * pass;
  const bool two = st[0] != st[1];
  for (int q = 0; q < 2; ++q) {
    const uint32_t* hq = h + (two && q ? 256 : 0);
    uint32_t r = st[2 + q], cum = 0;
    int b = 0;
    for (; b < 255; ++b) {
      if (r < cum + hq[b]) break;
      cum += hq[b];
    }
    st[q] |= (uint32_t)b << shift;
    st[2 + q] = r - cum;
  }
  if (pass == 3) { out[0] = st[0]; out[1] = st[1]; out[2] = st[4]; out[3] = 0; }
}

// ---- pass 1 / pass 2 of a distribution --------------------------------------
struct HistP {
  float first, last;     // the outer edges as the comparisons see them
  double denom;          // last - first as numpy holds it
  int wide;              // the scaled index is taken in fp64 (range given) or fp32
  int nb;
};
struct HAcc {
  double n, sq;
  float mn, mx;
};
__device__ __forceinline__ void hacc_merge(HAcc& a, const HAcc& b) {
  a.n += b.n; a.sq += b.sq;
  a.mn = __builtin_fminf(a.mn, b.mn); a.mx = __builtin_fmaxf(a.mx, b.mx);
}

constexpr int kHistPart = 4;      // doubles of a workgroup's partial

__global__ void __launch_bounds__(kBlk)
qa_hist_kernel(QaX x, const float* __restrict__ v, uint32_t n, int flags, float diff_max, HistP hp,
               const float* __restrict__ edges, uint32_t* __restrict__ ghist, double* __restrict__ partial,
               uint32_t* __restrict__ nan_word) {
  __shared__ uint32_t h[kMaxBins];
  __shared__ HAcc sm[kWaves];
  const int tid = threadIdx.x;
  const bool do_stats = flags & S3_QA_HIST_STATS, do_hist = flags & S3_QA_HIST_COUNTS;
  const bool keep_all = flags & S3_QA_HIST_KEEP_ALL;
  if (do_hist) {
    for (int b = tid; b < hp.nb; b += kBlk) h[b] = 0;
    __syncthreads();
  }
  HAcc acc{0.0, 0.0, __builtin_inff(), -__builtin_inff()};
  uint32_t nan = 0;
  const uint32_t stride = gridDim.x * kBlk;
  for (uint32_t base = blockIdx.x * kBlk; base < n; base += stride) {
    const uint32_t e = base + tid;
    const bool valid = e < n;
    const float d = valid ? qa_value(x, v, e) : 0.f;
    if (d != d) ++nan;
    const bool kept = valid && d == d && (keep_all || __builtin_fabsf(d) < diff_max);
    if (kept && do_stats) {
      acc.n += 1.0; acc.sq += (double)d * (double)d;
      acc.mn = __builtin_fminf(acc.mn, d); acc.mx = __builtin_fmaxf(acc.mx, d);
    }
    if (do_hist) {
      const bool in = kept && d >= hp.first && d <= hp.last;
      int64_t idx = 0;
      if (in) {
        const float num = __fsub_rn(d, hp.first);
        if (hp.wide) idx = (int64_t)(((double)num / hp.denom) * (double)hp.nb);
        else idx = (int64_t)__fmul_rn(__fdiv_rn(num, (float)hp.denom), (float)hp.nb);
        if (idx >= hp.nb) idx = hp.nb - 1;
        if (idx < 0) idx = 0;
        if (idx > 0 && d < edges[idx]) --idx;
        if (idx != hp.nb - 1 && d >= edges[idx + 1]) ++idx;
      }
      lds_count(h, (uint32_t)idx, in);
    }
    if (stride > 0xFFFFFFFFu - base) break;
  }
  if (do_hist) {
    __syncthreads();
    for (int b = tid; b < hp.nb; b += kBlk)
      if (h[b]) atomicAdd(&ghist[b], h[b]);
  }
  if (nan) atomicAdd(nan_word, nan);
  if (do_stats) {
    for (int o = 32; o > 0; o >>= 1) {
      HAcc b;
      b.n = __shfl_xor(acc.n, o); b.sq = __shfl_xor(acc.sq, o);
      b.mn = __shfl_xor(acc.mn, o); b.mx = __shfl_xor(acc.mx, o);
      hacc_merge(acc, b);
    }
    if ((tid & 63) == 0) sm[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
      HAcc a = sm[0];
      for (int w = 1; w < kWaves; ++w) hacc_merge(a, sm[w]);
      double* p = partial + (int64_t)blockIdx.x * kHistPart;
      p[0] = a.n; p[1] = a.sq; p[2] = (double)a.mn; p[3] = (double)a.mx;
    }
  }
}

// out = (count, sum d^2, min, max, NaN count) as five doubles
__global__ void __launch_bounds__(kBlk)
qa_hist_fold_kernel(const double* __restrict__ partial, int nblk, const uint32_t* __restrict__ nan_word,
                    double* __restrict__ out) {
  __shared__ HAcc sm[kBlk];
  const int tid = threadIdx.x;
  HAcc a{0.0, 0.0, __builtin_inff(), -__builtin_inff()};
  for (int b = tid; b < nblk; b += kBlk) {
    const double* p = partial + (int64_t)b * kHistPart;
    hacc_merge(a, HAcc{p[0], p[1], (float)p[2], (float)p[3]});
  }
  sm[tid] = a;
  __syncthreads();
  for (int st = kBlk / 2; st > 0; st >>= 1) {
    if (tid < st) { HAcc p = sm[tid]; hacc_merge(p, sm[tid + st]); sm[tid] = p; }
    __syncthreads();
  }
  if (tid == 0) {
    out[0] = sm[0].n; out[1] = sm[0].sq; out[2] = (double)sm[0].mn; out[3] = (double)sm[0].mx;
    out[4] = (double)nan_word[0];
  }
}

// ---- sum of |X|^2 over the outer and inner axes of an (outer, L, inner) view -
// workgroup (l tile, slice of the rows): inner == 1 puts 64 lanes along l and 4
// rows side by side; inner > 1 puts the lanes along the (row, inner) pairs of
// one l.  partial[slice][l], folded by qa_power_fold_kernel in slice order.
__device__ __forceinline__ double pw(const float* re, const float* im, int64_t i) {
  const double a = (double)re[i], b = (double)im[i];
  return a * a + b * b;
}

__global__ void __launch_bounds__(kBlk)
qa_power_rows_kernel(const float* __restrict__ re0, const float* __restrict__ im0, const float* __restrict__ re1,
                     const float* __restrict__ im1, int64_t outer, int L, double* __restrict__ partial) {
  __shared__ double sm[kBlk];
  const int tid = threadIdx.x, lx = tid & 63, ry = tid >> 6;
  const int l = blockIdx.x * 64 + lx;
  double acc = 0.0;
  if (l < L)
    for (int64_t o = (int64_t)blockIdx.y * kWaves + ry; o < outer; o += (int64_t)gridDim.y * kWaves) {
      acc += pw(re0, im0, o * L + l);
      if (re1) acc += pw(re1, im1, o * L + l);
    }
  sm[tid] = acc;
  __syncthreads();
  if (ry == 0 && l < L) partial[(int64_t)blockIdx.y * L + l] = ((sm[lx] + sm[64 + lx]) + sm[128 + lx]) + sm[192 + lx];
}

__global__ void __launch_bounds__(kBlk)
qa_power_inner_kernel(const float* __restrict__ re0, const float* __restrict__ im0, const float* __restrict__ re1,
                      const float* __restrict__ im1, int64_t outer, int L, int64_t inner,
                      double* __restrict__ partial) {
  __shared__ double sm[kBlk];
  const int tid = threadIdx.x, l = blockIdx.x;
  const int64_t total = outer * inner;
  double acc = 0.0;
  for (int64_t p = (int64_t)blockIdx.y * kBlk + tid; p < total; p += (int64_t)gridDim.y * kBlk) {
    const int64_t o = p / inner, i = p - o * inner;
    const int64_t at = (o * L + l) * inner + i;
    acc += pw(re0, im0, at);
    if (re1) acc += pw(re1, im1, at);
  }
  sm[tid] = acc;
  __syncthreads();
  for (int st = kBlk / 2; st > 0; st >>= 1) {
    if (tid < st) sm[tid] += sm[tid + st];
    __syncthreads();
  }
  if (tid == 0) partial[(int64_t)blockIdx.y * L + l] = sm[0];
}

__global__ void qa_power_fold_kernel(const double* __restrict__ partial, int nslice, int L, double* __restrict__ out) {
  const int l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= L) return;
  double a = 0.0;
  for (int b = 0; b < nslice; ++b) a += partial[(int64_t)b * L + l];
  out[l] = a;
}

int qa_xform(s3_ctx* ctx, const char* who, int diff, int64_t n, int64_t inner_out, int64_t inner_in, int64_t delta,
             int has_period, float period, float half, float scale, QaX& x) {
  if (n < 1 || n > (int64_t)INT32_MAX) S3_FAIL(ctx, S3_EINVAL, std::string(who) + ": 1 .. 2^31 - 1 values");
  if (diff && (inner_out < 1 || inner_out > (int64_t)INT32_MAX || inner_in <= inner_out || delta < 1 ||
               delta != inner_in - inner_out))
    S3_FAIL(ctx, S3_EINVAL, std::string(who) + ": the difference's extents do not fit");
  x.diff = diff ? 1 : 0; x.has_period = has_period ? 1 : 0;
  x.period = period; x.half = half; x.scale = scale;
  x.inner_out = FastDiv(diff ? (uint32_t)inner_out : 1u);
  x.inner_in = inner_in; x.delta = delta;
  return S3_OK;
}

}  // namespace

extern "C" int s3_qa_recoarsen(s3_ctx* ctx, const float* hr, int layout, int64_t H1, int64_t H2, int64_t HT, int C,
                               const int* channel_host, const int* method_host, int F, int s_enhance, int t_enhance,
                               const float* const* true_host, float* const* syn_host, float* const* err_host,
                               double* summary) {
  if (!ctx) return S3_EINVAL;
  if (!hr) S3_FAIL(ctx, S3_EINVAL, "s3_qa_recoarsen: hr is needed");
  if (layout != S3_QA_CUBE && layout != S3_QA_TIME_FIRST) S3_FAIL(ctx, S3_EINVAL, "s3_qa_recoarsen: unknown layout");
  if (F < 1 || F > kMaxF) S3_FAIL(ctx, S3_EINVAL, "s3_qa_recoarsen: 1 .. 16 features per launch");
  if (layout == S3_QA_TIME_FIRST && (F != 1 || C != 1))
    S3_FAIL(ctx, S3_EINVAL, "s3_qa_recoarsen: a time-first field is one feature");
  if (H1 < 1 || H2 < 1 || HT < 1 || C < 1 || s_enhance < 1 || t_enhance < 1)
    S3_FAIL(ctx, S3_EINVAL, "s3_qa_recoarsen: extents and factors are at least 1");
  if (H1 % s_enhance || H2 % s_enhance) S3_FAIL(ctx, S3_EINVAL, "s3_qa_recoarsen: s_enhance must divide H1 and H2");
  if (HT % t_enhance) S3_FAIL(ctx, S3_EINVAL, "s3_qa_recoarsen: t_enhance must divide HT");
  if (!method_host || (layout == S3_QA_CUBE && !channel_host))
    S3_FAIL(ctx, S3_EINVAL, "s3_qa_recoarsen: the methods and the channel map are needed");
  if (summary && !true_host) S3_FAIL(ctx, S3_EINVAL, "s3_qa_recoarsen: the summary needs the true fields");
  if (err_host && !true_host) S3_FAIL(ctx, S3_EINVAL, "s3_qa_recoarsen: the error needs the true fields");
  RcArgs a;
  for (int f = 0; f < kMaxF; ++f) {
    a.tru[f] = nullptr; a.syn[f] = nullptr; a.err[f] = nullptr; a.ch[f] = 0; a.method[f] = 0;
    if (f >= F) continue;
    a.method[f] = method_host[f];
    if (a.method[f] < S3_TC_SUBSAMPLE || a.method[f] > S3_TC_MIN)
      S3_FAIL(ctx, S3_EINVAL, "s3_qa_recoarsen: unknown temporal coarsening method");
    a.ch[f] = layout == S3_QA_CUBE ? channel_host[f] : 0;
    if (a.ch[f] < 0 || a.ch[f] >= C) S3_FAIL(ctx, S3_EINVAL, "s3_qa_recoarsen: a channel outside the cube");
    a.tru[f] = true_host ? true_host[f] : nullptr;
    a.syn[f] = syn_host ? syn_host[f] : nullptr;
    a.err[f] = err_host ? err_host[f] : nullptr;
    if ((summary || a.err[f]) && !a.tru[f]) S3_FAIL(ctx, S3_EINVAL, "s3_qa_recoarsen: a true field is missing");
  }
  const int64_t S1 = H1 / s_enhance, S2 = H2 / s_enhance, T = HT / t_enhance;
  if (S2 > INT32_MAX || T > INT32_MAX || s_enhance > 1024 || t_enhance > kCubeTile || H1 > INT64_MAX / H2 / HT / C / 8)
    S3_FAIL(ctx, S3_EINVAL, "s3_qa_recoarsen: extents out of range");
  int64_t nblk;
  if (layout == S3_QA_CUBE) {
    if ((int64_t)t_enhance * C > kCubeTile)
      S3_FAIL(ctx, S3_EINVAL, "s3_qa_recoarsen: t_enhance * C above 4096 (one pixel's steps are staged in LDS)");
    int TT = kCubeTile / (t_enhance * C);
    if (TT > T) TT = (int)T;
    const int nchunk = (int)((T + TT - 1) / TT);
    nblk = S1 * S2 * nchunk;
    if (nblk > INT32_MAX) S3_FAIL(ctx, S3_EINVAL, "s3_qa_recoarsen: more than 2^31 - 1 workgroups");
    if (summary) if (int rc = ensure_scratch(ctx, (size_t)nblk * F * kWords * sizeof(double))) return rc;
    double* partial = summary ? reinterpret_cast<double*>(ctx->scratch) : nullptr;
#define QA_CUBE_LAUNCH(SS)                                                                                        \
  hipLaunchKernelGGL(qa_recoarsen_cube_kernel<SS>, dim3((unsigned)nblk), dim3(kBlk), 0, ctx->stream, hr, H2, HT, C, \
                     (int)S2, (int)T, F, s_enhance, t_enhance, TT, nchunk, a, partial)
    switch (s_enhance) {
      case 1: QA_CUBE_LAUNCH(1); break;
      case 2: QA_CUBE_LAUNCH(2); break;
      case 3: QA_CUBE_LAUNCH(3); break;
      case 4: QA_CUBE_LAUNCH(4); break;
      case 5: QA_CUBE_LAUNCH(5); break;
      default: QA_CUBE_LAUNCH(0); break;
    }
#undef QA_CUBE_LAUNCH
  } else {
    if (s_enhance > 64) S3_FAIL(ctx, S3_EINVAL, "s3_qa_recoarsen: s_enhance above 64 in the time-first layout");
    int TT = 128 / t_enhance;
    if (TT < 1) TT = 1;
    if (TT > T) TT = (int)T;
    const int JW = 64 / s_enhance;
    const size_t lds = (size_t)JW * ((TT * t_enhance) | 1) * sizeof(float);
    if (lds > ctx->lds_max)
      S3_FAIL(ctx, S3_EINVAL, "s3_qa_recoarsen: t_enhance needs more LDS than a workgroup has");
    const int nJ = (int)((S2 + JW - 1) / JW), nchunk = (int)((T + TT - 1) / TT);
    nblk = S1 * nJ * nchunk;
    if (nblk > INT32_MAX) S3_FAIL(ctx, S3_EINVAL, "s3_qa_recoarsen: more than 2^31 - 1 workgroups");
    if (summary) if (int rc = ensure_scratch(ctx, (size_t)nblk * kWords * sizeof(double))) return rc;
    double* partial = summary ? reinterpret_cast<double*>(ctx->scratch) : nullptr;
    // (the LDS limit follows the factors: set per call, not once)
#define QA_TFIRST_LAUNCH(SS)                                                                                   \
  do {                                                                                                         \
    if (lds > 64 * 1024)                                                                                       \
      if (int rc = s3_lds_set(ctx, qa_recoarsen_tfirst_kernel<SS>, lds)) return rc;                            \
    hipLaunchKernelGGL(qa_recoarsen_tfirst_kernel<SS>, dim3((unsigned)nblk), dim3(kBlk), lds, ctx->stream, hr, \
                       H1, H2, (int)S2, (int)T, s_enhance, t_enhance, TT, nJ, nchunk, a, partial);             \
  } while (0)
    switch (s_enhance) {
      case 1: QA_TFIRST_LAUNCH(1); break;
      case 2: QA_TFIRST_LAUNCH(2); break;
      case 3: QA_TFIRST_LAUNCH(3); break;
      case 4: QA_TFIRST_LAUNCH(4); break;
      case 5: QA_TFIRST_LAUNCH(5); break;
      default: QA_TFIRST_LAUNCH(0); break;
    }
#undef QA_TFIRST_LAUNCH
  }
  S3_HIP(ctx, hipGetLastError());
  if (summary) {
    hipLaunchKernelGGL(qa_summary_fold_kernel, dim3(F), dim3(kBlk), 0, ctx->stream,
                       reinterpret_cast<const double*>(ctx->scratch), (int)nblk, F, summary);
    S3_HIP(ctx, hipGetLastError());
  }
  return S3_OK;
}

extern "C" int s3_qa_select(s3_ctx* ctx, const float* v, int diff, int64_t n, int64_t inner_out, int64_t inner_in,
                            int64_t delta, int has_period, float period, float half_period, float scale,
                            int64_t rank0, int64_t rank1, uint32_t* out) {
  if (!ctx) return S3_EINVAL;
  if (!v || !out) S3_FAIL(ctx, S3_EINVAL, "s3_qa_select: v and out are needed");
  QaX x;
  if (int rc = qa_xform(ctx, "s3_qa_select", diff, n, inner_out, inner_in, delta, has_period, period, half_period,
                        scale, x))
    return rc;
  if (rank0 < 0 || rank0 >= n || rank1 < rank0 || rank1 >= n)
    S3_FAIL(ctx, S3_EINVAL, "s3_qa_select: ranks outside 0 <= rank0 <= rank1 < n");
  if (int rc = ensure_scratch(ctx, kSelWords * sizeof(uint32_t))) return rc;
  uint32_t* st = reinterpret_cast<uint32_t*>(ctx->scratch);
  hipLaunchKernelGGL(qa_select_init_kernel, dim3(1), dim3(kBlk), 0, ctx->stream, st, (uint32_t)rank0, (uint32_t)rank1);
  const int grid = grid_for(n, ctx->num_cu, 8);
  for (int pass = 0; pass < 4; ++pass) {
    hipLaunchKernelGGL(qa_select_hist_kernel, dim3(grid), dim3(kBlk), 0, ctx->stream, x, v, (uint32_t)n, pass, st);
    hipLaunchKernelGGL(qa_select_scan_kernel, dim3(1), dim3(256), 0, ctx->stream, st, pass, out);
  }
  S3_HIP(ctx, hipGetLastError());
  return S3_OK;
}

extern "C" int s3_qa_hist(s3_ctx* ctx, const float* v, int diff, int64_t n, int64_t inner_out, int64_t inner_in,
                          int64_t delta, int has_period, float period, float half_period, float scale, int flags,
                          float diff_max, float first_edge, float last_edge, double denom, int wide, int n_bins,
                          const float* edges, uint32_t* counts, double* stats) {
  if (!ctx) return S3_EINVAL;
  if (!v || !stats) S3_FAIL(ctx, S3_EINVAL, "s3_qa_hist: v and stats are needed");
  QaX x;
  if (int rc = qa_xform(ctx, "s3_qa_hist", diff, n, inner_out, inner_in, delta, has_period, period, half_period,
                        scale, x))
    return rc;
  if (!(flags & (S3_QA_HIST_STATS | S3_QA_HIST_COUNTS))) S3_FAIL(ctx, S3_EINVAL, "s3_qa_hist: nothing asked for");
  HistP hp{first_edge, last_edge, denom, wide, n_bins};
  if (flags & S3_QA_HIST_COUNTS) {
    if (n_bins < 1 || n_bins > kMaxBins) S3_FAIL(ctx, S3_EINVAL, "s3_qa_hist: 1 .. 4096 bins");
    if (!edges || !counts) S3_FAIL(ctx, S3_EINVAL, "s3_qa_hist: the edge table and the counts are needed");
    if (!(denom > 0.0) || !(first_edge < last_edge)) S3_FAIL(ctx, S3_EINVAL, "s3_qa_hist: an empty range");
    S3_HIP(ctx, hipMemsetAsync(counts, 0, (size_t)n_bins * sizeof(uint32_t), ctx->stream));
  } else {
    hp.nb = 0;
  }
  const int grid = grid_for(n, ctx->num_cu, 8);
  // scratch: the NaN word (a 16-byte cell), then the workgroups' partials
  if (int rc = ensure_scratch(ctx, 16 + (size_t)grid * kHistPart * sizeof(double))) return rc;
  uint32_t* nan_word = reinterpret_cast<uint32_t*>(ctx->scratch);
  double* partial = reinterpret_cast<double*>(reinterpret_cast<char*>(ctx->scratch) + 16);
  S3_HIP(ctx, hipMemsetAsync(nan_word, 0, 16, ctx->stream));
  // the fold reads every workgroup's partial: without the statistics they are zeroed
  if (!(flags & S3_QA_HIST_STATS))
    S3_HIP(ctx, hipMemsetAsync(partial, 0, (size_t)grid * kHistPart * sizeof(double), ctx->stream));
  hipLaunchKernelGGL(qa_hist_kernel, dim3(grid), dim3(kBlk), 0, ctx->stream, x, v, (uint32_t)n, flags, diff_max, hp,
                     edges, counts, partial, nan_word);
  hipLaunchKernelGGL(qa_hist_fold_kernel, dim3(1), dim3(kBlk), 0, ctx->stream, partial, grid, nan_word, stats);
  S3_HIP(ctx, hipGetLastError());
  return S3_OK;
}

extern "C" int s3_qa_power_sum(s3_ctx* ctx, const float* re0, const float* im0, const float* re1, const float* im1,
                               int64_t outer, int L, int64_t inner, double* out) {
  if (!ctx) return S3_EINVAL;
  if (!re0 || !im0 || !out || (re1 == nullptr) != (im1 == nullptr))
    S3_FAIL(ctx, S3_EINVAL, "s3_qa_power_sum: re, im and out are needed, the second field whole or not at all");
  if (outer < 1 || L < 1 || inner < 1 || outer > INT64_MAX / L / inner / 8)
    S3_FAIL(ctx, S3_EINVAL, "s3_qa_power_sum: extents out of range");
  if (L > 65535) S3_FAIL(ctx, S3_EINVAL, "s3_qa_power_sum: an axis above 65535");
  const int64_t per = inner == 1 ? kWaves : kBlk;           // pairs one slice takes per sweep
  int64_t want = (outer * inner + per - 1) / per;
  const int lblk = inner == 1 ? (L + 63) / 64 : L;
  int64_t cap = ((int64_t)ctx->num_cu * 8 + lblk - 1) / lblk;
  if (cap > 1024) cap = 1024;
  const int ns = (int)(want < cap ? want : cap);
  if (int rc = ensure_scratch(ctx, (size_t)ns * L * sizeof(double))) return rc;
  double* partial = reinterpret_cast<double*>(ctx->scratch);
  if (inner == 1)
    hipLaunchKernelGGL(qa_power_rows_kernel, dim3(lblk, ns), dim3(kBlk), 0, ctx->stream, re0, im0, re1, im1, outer, L,
                       partial);
  else
    hipLaunchKernelGGL(qa_power_inner_kernel, dim3(lblk, ns), dim3(kBlk), 0, ctx->stream, re0, im0, re1, im1, outer, L,
                       inner, partial);
  hipLaunchKernelGGL(qa_power_fold_kernel, dim3((L + kBlk - 1) / kBlk), dim3(kBlk), 0, ctx->stream, partial, ns, L, out);
  S3_HIP(ctx, hipGetLastError());
  return S3_OK;
}
