// Per-feature statistics and normalisation of a resident data cube.
// StatsCollection (sup3r/preprocessing/collections/stats.py) takes
// .mean(skipna=True) / .std(skipna=True) of every feature over all of space and
// time, then Sup3rX.normalize (accessor.py:356-361) writes (x - mean) / std
// back.  Both are one pass over a channels-last (n_pos, C) fp32 cube:
//   s3_channel_moments      count, mean and sum of squared deviations per
//                           channel in fp64, NaN skipped, one read of the cube;
//   s3_normalize_channels   x = (x - m) / s in place for the flagged channels,
//                           two correctly rounded fp32 operations.
//
// How a lane knows its channels.  The cube is walked as float4 (after a head of
// up to 3 floats that brings the pointer to a 16-byte line).  Element e of the
// walk is channel (head + e) % C, so the four channels of float4 number v repeat
// with period L = C / gcd(C, 4) in v.  The grid is sized so that the number of
// threads — the stride from one float4 of a lane to its next — is a multiple of
// L: 256 threads per workgroup supply the power of two in L, the workgroup
// count is a multiple of its odd part.  The four channels of a lane are then
// fixed for the whole launch: accumulators and normalisation constants stay in
// registers, every load is 16 bytes per lane, and no C divides anything.  (A
// cube short enough for one float4 per lane takes any grid.)  The up to 6 floats
// before and behind the float4 run are folded in by the second stage (moments)
// or written by workgroup 0 (normalise).
//
// The moments are accumulated shifted: a lane keeps, per channel, K (the first
// finite value it met), n, s1 = sum(x - K) and s2 = sum((x - K)^2) with the
// differences and sums in fp64.  x - K is exact in fp64 for fp32 x and K within
// 2^29 of each other, and K lies inside the data, so s2 - s1^2 / n loses no more
// than a few bits where sum(x^2) - sum(x)^2 / n loses all of them for data far
// from 0 (1e5 +- 0.1: 12 digits of 16).  Two partials merge without a division
// by moving one to the other's shift,
//   s1 += s1' + n' dK,  s2 += s2' + 2 dK s1' + n' dK^2,  dK = K' - K,
// and only the last step of all divides: mean = K + s1 / n, M2 = s2 - s1^2 / n.
// +-inf is never taken as a shift: it makes s1 +-inf (NaN when both signs occur)
// and M2 NaN, which is what numpy's mean and std give.
// Partials are folded in a fixed order — lanes through LDS, workgroups by a
// second kernel, no atomics — so a cube gives the same bits every time.
#include "common.h"

namespace {

constexpr int kBlk = kBlock;
constexpr int kMaxC = S3_STATS_MAX_CHANNELS;
constexpr int kEnt = kBlk * 4;           // (lane, component) accumulators of a workgroup

struct Part {                            // a partial of one channel; K is NaN while no finite value was met
  double n, K, s1, s2;
};

__device__ __forceinline__ Part part_empty() { return Part{0.0, __builtin_nan(""), 0.0, 0.0}; }

// a <- a merged with b: b's sums moved to a's shift (a takes b's if it has none)
__device__ __forceinline__ void part_merge(Part& a, const Part& b) {
  if (b.n == 0.0) return;
  double dK = 0.0;
  if (a.K != a.K) a.K = b.K;
  else if (b.K == b.K) dK = b.K - a.K;
  a.s2 += b.s2 + (2.0 * dK * b.s1 + b.n * dK * dK);
  a.s1 += b.s1 + b.n * dK;
  a.n += b.n;
}

__device__ __forceinline__ Part part_of(float x) {
  Part p = part_empty();
  if (x != x) return p;
  p.n = 1.0;
  if (__builtin_isfinite(x)) p.K = (double)x;
  else { p.s1 = (double)x; p.s2 = (double)x * (double)x; }
  return p;
}

uint32_t to_align16(const void* p) {      // floats up to the next 16-byte line
  return (uint32_t)((4u - (((uintptr_t)p >> 2) & 3u)) & 3u);
}

// one lane's running sums of one float4 component
struct LaneAcc {
  double K, s1, s2;     // K: 0 until `have`
  uint32_t n;
  bool have;
  __device__ __forceinline__ void init() { K = 0.0; s1 = 0.0; s2 = 0.0; n = 0; have = false; }
  __device__ __forceinline__ void add(float x) {
    const bool valid = x == x;
    if (!have && __builtin_isfinite(x)) { K = (double)x; have = true; }
    const double d = valid ? (double)x - K : 0.0;
    n += valid ? 1u : 0u;
    s1 += d;
    s2 = __builtin_fma(d, d, s2);
  }
  __device__ __forceinline__ float shift() const { return have ? (float)K : __builtin_nanf(""); }
};

// A non-finite value that a lane meets BEFORE its first finite one is summed
// against shift 0 and the later ones against K: harmless, s1 is +-inf or NaN
// from there on and stays so under any finite shift.

__global__ void __launch_bounds__(kBlk)
channel_moments_kernel(const float4* __restrict__ x4, int64_t nvec, int C, uint32_t head, Part* __restrict__ partial) {
  __shared__ uint32_t s_n[kEnt];
  __shared__ float s_K[kEnt];
  __shared__ double s_s1[kEnt], s_s2[kEnt];
  const uint32_t tid = threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kBlk;
  LaneAcc a0, a1, a2, a3;
  a0.init(); a1.init(); a2.init(); a3.init();
  int64_t v = (int64_t)blockIdx.x * kBlk + tid;
  for (; v + 3 * stride < nvec; v += 4 * stride) {           // four loads in flight per lane
    const float4 p = x4[v], q = x4[v + stride], r = x4[v + 2 * stride], s = x4[v + 3 * stride];
    a0.add(p.x); a1.add(p.y); a2.add(p.z); a3.add(p.w);
    a0.add(q.x); a1.add(q.y); a2.add(q.z); a3.add(q.w);
    a0.add(r.x); a1.add(r.y); a2.add(r.z); a3.add(r.w);
    a0.add(s.x); a1.add(s.y); a2.add(s.z); a3.add(s.w);
  }
  for (; v < nvec; v += stride) {
    const float4 p = x4[v];
    a0.add(p.x); a1.add(p.y); a2.add(p.z); a3.add(p.w);
  }
  // entry e = 4 tid + k of this workgroup is channel (phase + e) % C
  const uint32_t e0 = tid * 4;
  s_n[e0] = a0.n; s_K[e0] = a0.shift(); s_s1[e0] = a0.s1; s_s2[e0] = a0.s2;
  s_n[e0 + 1] = a1.n; s_K[e0 + 1] = a1.shift(); s_s1[e0 + 1] = a1.s1; s_s2[e0 + 1] = a1.s2;
  s_n[e0 + 2] = a2.n; s_K[e0 + 2] = a2.shift(); s_s1[e0 + 2] = a2.s1; s_s2[e0 + 2] = a2.s2;
  s_n[e0 + 3] = a3.n; s_K[e0 + 3] = a3.shift(); s_s1[e0 + 3] = a3.s1; s_s2[e0 + 3] = a3.s2;
  // fold entries a multiple of C apart, the distance halving: after the step
  // of distance s C everything lives in entries below s C
  uint32_t s = 1;
  while (2 * s * (uint32_t)C < (uint32_t)kEnt) s *= 2;
  for (; s >= 1; s >>= 1) {
    __syncthreads();
    const uint32_t span = s * (uint32_t)C;
    const uint32_t cnt = kEnt - span < span ? kEnt - span : span;   // (span < kEnt: s is the least with 2 s C >= kEnt)
    for (uint32_t e = tid; e < cnt; e += kBlk) {
      Part a{(double)s_n[e], (double)s_K[e], s_s1[e], s_s2[e]};
      const Part b{(double)s_n[e + span], (double)s_K[e + span], s_s1[e + span], s_s2[e + span]};
      part_merge(a, b);
      // (n of a workgroup fits 32 bits: a lane meets fewer than 2^32 / 1024 values
      // per component, see the launcher; K stays an fp32 value, it is one of them)
      s_n[e] = (uint32_t)a.n; s_K[e] = (float)a.K; s_s1[e] = a.s1; s_s2[e] = a.s2;
    }
  }
  __syncthreads();
  if (tid < (uint32_t)C) {
    const uint32_t phase = (uint32_t)((head + (uint64_t)blockIdx.x * kEnt) % (uint32_t)C);
    const uint32_t ch = (phase + tid) % (uint32_t)C;
    partial[(int64_t)blockIdx.x * C + ch] = Part{(double)s_n[tid], (double)s_K[tid], s_s1[tid], s_s2[tid]};
  }
}

// workgroup c: the partials of channel c, workgroup 0 first, then the floats
// outside the float4 run; out[c] = (n, mean, M2)
__global__ void __launch_bounds__(kBlk)
channel_moments_fold_kernel(const Part* __restrict__ partial, int nblk, int C, const float* __restrict__ x,
                            int64_t n_elem, uint32_t head, int64_t tail0, double* __restrict__ out) {
  __shared__ Part sm[kBlk];
  const int c = blockIdx.x;
  const uint32_t tid = threadIdx.x;
  Part a = part_empty();
  for (int b = tid; b < nblk; b += kBlk) part_merge(a, partial[(int64_t)b * C + c]);
  sm[tid] = a;
  __syncthreads();
  for (uint32_t s = kBlk / 2; s > 0; s >>= 1) {
    if (tid < s) { Part p = sm[tid]; part_merge(p, sm[tid + s]); sm[tid] = p; }
    __syncthreads();
  }
  if (tid != 0) return;
  a = sm[0];
  for (int64_t i = 0; i < (int64_t)head; ++i)
    if (i % C == c) part_merge(a, part_of(x[i]));
  for (int64_t i = tail0; i < n_elem; ++i)
    if (i % C == c) part_merge(a, part_of(x[i]));
  double mean = 0.0, m2 = 0.0;
  if (a.n > 0.0) {
    const double d = a.s1 / a.n;
    mean = (a.K == a.K ? a.K : 0.0) + d;
    m2 = a.s2 - a.s1 * d;
    if (m2 < 0.0) m2 = 0.0;                  // (rounding of a constant channel; NaN stays NaN)
  }
  out[3 * c] = a.n; out[3 * c + 1] = mean; out[3 * c + 2] = m2;
}

struct NormArgs {
  float m[kMaxC], s[kMaxC];
  uint64_t mask;
};

// numpy's float32 (x - m) / s: a correctly rounded subtraction, then a correctly
// rounded division (__fdiv_rn: the IEEE expansion, not v_rcp_f32 and a
// multiply).  An unflagged channel is stored back untouched.
__device__ __forceinline__ float norm1(float x, float m, float s, bool on) {
  return on ? __fdiv_rn(__fsub_rn(x, m), s) : x;
}

// float4 in flight per lane, workgroups per CU: 4 or 8 loads and 4 workgroups
// measured the same as these (profiles/stats/NOTES.md)
constexpr int kNormLoads = 2, kNormPerCu = 8;

__global__ void __launch_bounds__(kBlk)
normalize_channels_kernel(float* __restrict__ x, int64_t n_elem, int64_t nvec, int C, uint32_t head, NormArgs a) {
  const uint32_t tid = threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kBlk;
  const int64_t v0 = (int64_t)blockIdx.x * kBlk + tid;
  float4* x4 = reinterpret_cast<float4*>(x + head);
  float m[4], s[4];
  bool on[4];
  const uint32_t c0 = (uint32_t)((head + (uint64_t)v0 * 4) % (uint32_t)C);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t c = (c0 + k) % (uint32_t)C;
    m[k] = a.m[c]; s[k] = a.s[c]; on[k] = (a.mask >> c) & 1u;
  }
  int64_t v = v0;
  for (; v + (kNormLoads - 1) * stride < nvec; v += kNormLoads * stride) {
    float4 p[kNormLoads];
#pragma unroll
    for (int u = 0; u < kNormLoads; ++u) p[u] = x4[v + u * stride];
#pragma unroll
    for (int u = 0; u < kNormLoads; ++u) {
      p[u].x = norm1(p[u].x, m[0], s[0], on[0]); p[u].y = norm1(p[u].y, m[1], s[1], on[1]);
      p[u].z = norm1(p[u].z, m[2], s[2], on[2]); p[u].w = norm1(p[u].w, m[3], s[3], on[3]);
    }
#pragma unroll
    for (int u = 0; u < kNormLoads; ++u) x4[v + u * stride] = p[u];
  }
  for (; v < nvec; v += stride) {
    float4 p = x4[v];
    p.x = norm1(p.x, m[0], s[0], on[0]); p.y = norm1(p.y, m[1], s[1], on[1]);
    p.z = norm1(p.z, m[2], s[2], on[2]); p.w = norm1(p.w, m[3], s[3], on[3]);
    x4[v] = p;
  }
  // the floats outside the float4 run: at most 3 + 3
  if (blockIdx.x == 0 && tid < 8) {
    const int64_t tail0 = (int64_t)head + nvec * 4;
    const int64_t i = tid < 4 ? (int64_t)tid : tail0 + (tid - 4);
    const bool mine = tid < 4 ? tid < head : i < n_elem;
    if (mine) {
      const uint32_t c = (uint32_t)(i % C);
      x[i] = norm1(x[i], a.m[c], a.s[c], (a.mask >> c) & 1u);
    }
  }
}

// workgroups of a float4 walk whose lanes keep their channels (see the top):
// all the walk needs if that is within the cap, else the largest multiple of
// the odd part of C / gcd(C, 4) within it
int fixed_phase_grid(int64_t nvec, int C, int num_cu, int per_cu) {
  const int grid = grid_for(nvec, num_cu, per_cu);
  if ((int64_t)grid * kBlk >= nvec) return grid;   // one float4 per lane at the most
  int odd = C;
  while (odd % 2 == 0) odd /= 2;
  return grid / odd * odd;         // (grid is the cap: num_cu * per_cu >= 64 > odd, see the entry points)
}

}  // namespace

extern "C" int s3_channel_moments(s3_ctx* ctx, const float* x, int64_t n_pos, int c, double* out) {
  if (!ctx) return S3_EINVAL;
  if (!x || !out) S3_FAIL(ctx, S3_EINVAL, "s3_channel_moments: x and out are needed");
  if (n_pos < 1) S3_FAIL(ctx, S3_EINVAL, "s3_channel_moments: empty cube");
  if (c < 1 || c > kMaxC) S3_FAIL(ctx, S3_EINVAL, "s3_channel_moments: 1 .. 64 channels");
  if (((uintptr_t)x & 3u) || ((uintptr_t)out & 7u)) S3_FAIL(ctx, S3_EINVAL, "s3_channel_moments: misaligned x or out");
  if (n_pos > INT64_MAX / c / 8) S3_FAIL(ctx, S3_EINVAL, "s3_channel_moments: the cube's size overflows");
  if (ctx->num_cu < 16) S3_FAIL(ctx, S3_EINVAL, "s3_channel_moments: fewer than 16 compute units");
  const int64_t n_elem = n_pos * c;
  uint32_t head = to_align16(x);
  if ((int64_t)head > n_elem) head = (uint32_t)n_elem;
  const int64_t nvec = (n_elem - head) / 4;
  // (82 registers and 24 KiB of LDS: 5 workgroups fit a CU; 4 keep the whole grid resident)
  const int grid = fixed_phase_grid(nvec, c, ctx->num_cu, 4);
  // a lane's count of one component is 32 bits, a workgroup's sum of 1024 / C of them too
  if (nvec / ((int64_t)grid * kBlk) >= ((int64_t)1 << 21))
    S3_FAIL(ctx, S3_EINVAL, "s3_channel_moments: more than 2^21 float4 per lane");
  if (int rc = ensure_scratch(ctx, (size_t)grid * c * sizeof(Part))) return rc;
  Part* partial = reinterpret_cast<Part*>(ctx->scratch);
  hipLaunchKernelGGL(channel_moments_kernel, dim3(grid), dim3(kBlk), 0, ctx->stream,
                     reinterpret_cast<const float4*>(x + head), nvec, c, head, partial);
  S3_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL(channel_moments_fold_kernel, dim3(c), dim3(kBlk), 0, ctx->stream, partial, grid, c, x, n_elem,
                     head, (int64_t)head + nvec * 4, out);
  S3_HIP(ctx, hipGetLastError());
  return S3_OK;
}

extern "C" int s3_normalize_channels(s3_ctx* ctx, float* x, int64_t n_pos, int c, const float* mean_host,
                                     const float* std_host, const unsigned char* flag_host) {
  if (!ctx) return S3_EINVAL;
  if (!x || !mean_host || !std_host || !flag_host)
    S3_FAIL(ctx, S3_EINVAL, "s3_normalize_channels: x, the means, the stds and the flags are needed");
  if (n_pos < 1) S3_FAIL(ctx, S3_EINVAL, "s3_normalize_channels: empty cube");
  if (c < 1 || c > kMaxC) S3_FAIL(ctx, S3_EINVAL, "s3_normalize_channels: 1 .. 64 channels");
  if ((uintptr_t)x & 3u) S3_FAIL(ctx, S3_EINVAL, "s3_normalize_channels: misaligned x");
  if (n_pos > INT64_MAX / c / 8) S3_FAIL(ctx, S3_EINVAL, "s3_normalize_channels: the cube's size overflows");
  if (ctx->num_cu < 8) S3_FAIL(ctx, S3_EINVAL, "s3_normalize_channels: fewer than 8 compute units");
  NormArgs a;
  a.mask = 0;
  for (int i = 0; i < kMaxC; ++i) {
    a.m[i] = i < c ? mean_host[i] : 0.f;
    a.s[i] = i < c ? std_host[i] : 1.f;
    if (i < c && flag_host[i]) a.mask |= (uint64_t)1 << i;
  }
  if (a.mask == 0) return S3_OK;
  const int64_t n_elem = n_pos * c;
  uint32_t head = to_align16(x);
  if ((int64_t)head > n_elem) head = (uint32_t)n_elem;
  const int64_t nvec = (n_elem - head) / 4;
  const int grid = fixed_phase_grid(nvec, c, ctx->num_cu, kNormPerCu);
  hipLaunchKernelGGL(normalize_channels_kernel, dim3(grid), dim3(kBlk), 0, ctx->stream, x, n_elem, nvec, c, head, a);
  S3_HIP(ctx, hipGetLastError());
  return S3_OK;
}
