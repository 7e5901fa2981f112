// What DualSamplerCC (sup3r/preprocessing/samplers/cc.py:185-203) does to a
// batch of hourly data after cutting it, on the device:
//   * nn_fill_array (sup3r/utilities/utilities.py:55-75): every NaN of the
//     clearsky-ratio channel takes the value of the nearest non-NaN element of
//     the (n, s1, s2, t) block, scipy's distance_transform_edt with indices —
//     s3_nn_fill;
//   * nsrdb_reduce_daily_data (samplers/utilities.py:258-297): the hours of a
//     24-hour window in which the channel is NaN anywhere are "night"; the
//     batch keeps t hours centred on the daylight — s3_cc_night_mask here, the
//     gather that starts at the data-dependent hour in kernels_sample.hip.
//
// The fill.  Among the sources at the minimal squared distance scipy returns
// the one with the smallest column-major index F = m + n (i + s1 (j + s2 k)).
// So every element carries the 64-bit key (d2 << 32) | F of the best source
// found so far (all ones: none), and one min-plus pass per axis,
//   key'[p] = min over q of the line ( key[q] + ((p - q)^2 << 32) ),
// leaves the lexicographic minimum of (d2, F) over the whole block: adding the
// same (p - q)^2 to the d2 of every candidate behind q keeps their order, and
// d2 cannot carry into bit 64 (extents <= kMaxAxis: d2 <= 4 * 2047^2).  Integer
// arithmetic throughout; the values move as bit patterns.
//
// One kernel serves the four axes.  The key array is (n, s1, s2, t), time
// fastest, seen as (outer, L, inner) around the axis of the pass.  A workgroup
// stages `no` x L x `wi` keys — whole lines, `wi` consecutive inner positions of
// each — in LDS, so the pass is in place, and consecutive lanes are consecutive
// inner positions (consecutive k for the passes along n, s1, s2): global
// accesses run along memory and the ds_read_b64 of a wave are consecutive
// 8-byte words or one word for all lanes (the pass along t, inner = 1, where
// the lanes of a line read the same candidate).  Lines are short (t = 72, s = 20
// in production): each element takes the minimum over its line by brute force.
// The last pass stores no key: it copies the source's value over the NaN.
#include "common.h"

namespace {

constexpr int kBlk = kBlock;   // grid_for counts workgroups of this size
constexpr int kTile = 2048;              // keys staged per workgroup (16 KiB)
constexpr int kMaxAxis = S3_NN_FILL_MAX_AXIS;
constexpr uint64_t kNone = ~0ull;
constexpr int kMaxN = S3_SAMPLE_MAX_ORIGINS;

static_assert(kMaxAxis <= kTile, "a whole line is staged");

__device__ __forceinline__ bool nan_bits(uint32_t b) { return (b & 0x7FFFFFFFu) > 0x7F800000u; }

struct FillGeom {
  uint32_t n, s1, s2, t;                 // extents of the block
  uint32_t C, channel;
  uint32_t total;                        // n * s1 * s2 * t
  FastDiv dT, dS2, dS1;                  // row-major decomposition of an element
};

// key of every element: itself at distance 0, or none; *count += NaNs
__global__ void __launch_bounds__(kBlk)
nn_fill_init_kernel(FillGeom g, const uint32_t* __restrict__ x, uint64_t* __restrict__ key,
                    int* __restrict__ count) {
  __shared__ int s_cnt;
  if (threadIdx.x == 0) s_cnt = 0;
  __syncthreads();
  int mine = 0;
  for (uint32_t e = blockIdx.x * kBlk + threadIdx.x; e < g.total; e += gridDim.x * kBlk) {
    const uint32_t r2 = g.dT(e), k = e - r2 * g.t;
    const uint32_t r1 = g.dS2(r2), j = r2 - r1 * g.s2;
    const uint32_t m = g.dS1(r1), i = r1 - m * g.s1;
    const bool hole = nan_bits(x[(size_t)e * g.C + g.channel]);
    key[e] = hole ? kNone : (uint64_t)(m + g.n * (i + g.s1 * (j + g.s2 * k)));
    mine += hole;
  }
  // lanes of a wave first, then one atomic per wave into LDS, one per workgroup out
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&s_cnt, mine);
  __syncthreads();
  if (threadIdx.x == 0 && s_cnt) atomicAdd(count, s_cnt);
}

struct PassGeom {
  uint32_t L, inner, outer;              // the key array as (outer, L, inner)
  uint32_t wi, no;                       // tile: no x L x wi keys
  uint32_t tiles_in;                     // ceil(inner / wi)
  uint32_t total;                        // outer * L * inner
  uint32_t apply;                        // last pass: write the values, not the keys
  FastDiv dWi, dL, dTin;
};

__global__ void __launch_bounds__(kBlk)
nn_fill_pass_kernel(PassGeom p, FillGeom g, uint64_t* __restrict__ key, uint32_t* __restrict__ x,
                    const int* __restrict__ count) {
  __shared__ uint64_t s_key[kTile];
  const int holes = *count;              // (the same word for every lane: one scalar load)
  if (holes == 0 || (uint32_t)holes == p.total) return;   // nothing to fill / nothing to fill from
  const uint32_t to = p.dTin(blockIdx.x), ti = blockIdx.x - to * p.tiles_in;
  const uint32_t o0 = to * p.no, w0 = ti * p.wi;
  const uint32_t no = p.outer - o0 < p.no ? p.outer - o0 : p.no;
  const uint32_t wi = p.inner - w0 < p.wi ? p.inner - w0 : p.wi;
  // the tile is laid out with ITS widths (p.wi, not the clipped wi): the index
  // arithmetic below divides by launch constants only
  const uint32_t cnt = no * p.L * p.wi;
  for (uint32_t e = threadIdx.x; e < cnt; e += kBlk) {
    const uint32_t row = p.dWi(e), w = e - row * p.wi;        // row = o * L + q
    if (w < wi) s_key[e] = key[((size_t)o0 * p.L + row) * p.inner + w0 + w];
  }
  __syncthreads();
  for (uint32_t e = threadIdx.x; e < cnt; e += kBlk) {
    const uint32_t row = p.dWi(e), w = e - row * p.wi;
    if (w >= wi) continue;
    const uint32_t o = p.dL(row), pos = row - o * p.L;
    const uint64_t* line = s_key + (size_t)o * p.L * p.wi + w;
    uint64_t best = kNone;
    for (uint32_t q = 0; q < p.L; ++q) {
      const uint64_t kq = line[q * p.wi];
      const int32_t d = (int32_t)pos - (int32_t)q;
      const uint64_t cand = kq + ((uint64_t)(uint32_t)(d * d) << 32);
      if (kq != kNone && cand < best) best = cand;
    }
    const size_t at = ((size_t)o0 * p.L + row) * p.inner + w0 + w;
    if (!p.apply) {
      key[at] = best;
    } else if ((best >> 32) != 0 && best != kNone) {
      // F -> (m, i, j, k) -> row-major element of the source
      uint32_t f = (uint32_t)best;
      const uint32_t m = f % g.n; f /= g.n;
      const uint32_t i = f % g.s1; f /= g.s1;
      const uint32_t j = f % g.s2, k = f / g.s2;
      const size_t src = (((size_t)m * g.s1 + i) * g.s2 + j) * g.t + k;
      x[at * g.C + g.channel] = x[src * g.C + g.channel];
    }
  }
}

struct MaskGeom {
  int64_t S2, TC;                        // cube: columns, floats per pixel (T * C)
  uint32_t s1, s2, C, channel;
  uint32_t total;                        // n * s1 * s2 * 24 of THIS launch
  FastDiv d24, dS2, dS1;
  int org[kMaxN][3];
};

__global__ void __launch_bounds__(kBlk)
cc_night_mask_kernel(MaskGeom g, const uint32_t* __restrict__ data, unsigned* __restrict__ word) {
  __shared__ unsigned s_word;
  if (threadIdx.x == 0) s_word = 0;
  __syncthreads();
  unsigned mine = 0;
  for (uint32_t e = blockIdx.x * kBlk + threadIdx.x; e < g.total; e += gridDim.x * kBlk) {
    const uint32_t pix = g.d24(e), k = e - pix * 24;
    const uint32_t mi = g.dS2(pix), j = pix - mi * g.s2;
    const uint32_t m = g.dS1(mi), i = mi - m * g.s1;
    const int64_t at = ((int64_t)(g.org[m][0] + (int)i) * g.S2 + (g.org[m][1] + (int)j)) * g.TC +
                       (int64_t)(g.org[m][2] + (int)k) * g.C + g.channel;
    if (nan_bits(data[at])) mine |= 1u << k;
  }
  for (int o = 32; o > 0; o >>= 1) mine |= (unsigned)__shfl_xor((int)mine, o);
  if ((threadIdx.x & 63) == 0 && mine) atomicOr(&s_word, mine);
  __syncthreads();
  if (threadIdx.x == 0 && s_word) atomicOr(word, s_word);
}

}  // namespace

extern "C" int s3_nn_fill(s3_ctx* ctx, float* x, int n, int s1, int s2, int t, int C, int channel,
                          void* work, int* count) {
  if (!ctx) return S3_EINVAL;
  if (!x || !work || !count) S3_FAIL(ctx, S3_EINVAL, "s3_nn_fill: x, the workspace and the count word are needed");
  if (n < 1 || s1 < 1 || s2 < 1 || t < 1) S3_FAIL(ctx, S3_EINVAL, "s3_nn_fill: empty block");
  if (C < 1 || channel < 0 || channel >= C) S3_FAIL(ctx, S3_EINVAL, "s3_nn_fill: channel outside [0, C)");
  if (n > kMaxAxis || s1 > kMaxAxis || s2 > kMaxAxis || t > kMaxAxis)
    S3_FAIL(ctx, S3_EINVAL, "s3_nn_fill: an extent above S3_NN_FILL_MAX_AXIS (2048)");
  const int64_t total = (int64_t)n * s1 * s2 * t;
  if (total >= ((int64_t)1 << 31)) S3_FAIL(ctx, S3_EINVAL, "s3_nn_fill: 2^31 or more elements of the channel");
  if (((uintptr_t)work & 7u) != 0) S3_FAIL(ctx, S3_EINVAL, "s3_nn_fill: the workspace must be 8-byte aligned");
  S3_HIP(ctx, hipMemsetAsync(count, 0, sizeof(int), ctx->stream));
  FillGeom g;
  g.n = n; g.s1 = s1; g.s2 = s2; g.t = t; g.C = C; g.channel = channel;
  g.total = (uint32_t)total;
  g.dT = FastDiv(t); g.dS2 = FastDiv(s2); g.dS1 = FastDiv(s1);
  uint64_t* key = static_cast<uint64_t*>(work);
  uint32_t* bits = reinterpret_cast<uint32_t*>(x);
  hipLaunchKernelGGL(nn_fill_init_kernel, dim3(grid_for(total, ctx->num_cu)), dim3(kBlk), 0, ctx->stream, g, bits, key, count);
  S3_HIP(ctx, hipGetLastError());
  // the pass along t first (its lines lie along memory), then s2, s1, n;
  // an axis of extent 1 has nothing to look at
  const uint32_t ext[4] = {(uint32_t)t, (uint32_t)s2, (uint32_t)s1, (uint32_t)n};
  int last = -1;
  for (int a = 0; a < 4; ++a)
    if (ext[a] > 1) last = a;
  uint32_t inner = 1;
  for (int a = 0; a < 4; ++a) {
    const uint32_t L = ext[a];
    if (L > 1) {
      PassGeom p;
      p.L = L; p.inner = inner; p.outer = (uint32_t)(total / ((int64_t)L * inner));
      p.wi = (uint32_t)kTile / L < inner ? (uint32_t)kTile / L : inner;     // >= 1: L <= kTile
      p.no = (uint32_t)kTile / (L * p.wi);
      if (p.no > p.outer) p.no = p.outer;
      p.tiles_in = (inner + p.wi - 1) / p.wi;
      p.total = (uint32_t)total;
      p.apply = a == last ? 1u : 0u;
      p.dWi = FastDiv(p.wi); p.dL = FastDiv(L); p.dTin = FastDiv(p.tiles_in);
      const int64_t tiles = (int64_t)((p.outer + p.no - 1) / p.no) * p.tiles_in;   // < 2^31: <= total
      hipLaunchKernelGGL(nn_fill_pass_kernel, dim3((unsigned)tiles), dim3(kBlk), 0, ctx->stream, p, g, key,
                         bits, count);
      S3_HIP(ctx, hipGetLastError());
    }
    inner *= L;
  }
  return S3_OK;
}

extern "C" int s3_cc_night_mask(s3_ctx* ctx, const float* data, int64_t S1, int64_t S2, int64_t T, int C,
                                const int* origins_host, int n, int s1, int s2, int channel, int* status) {
  if (!ctx) return S3_EINVAL;
  if (!data || !origins_host || !status)
    S3_FAIL(ctx, S3_EINVAL, "s3_cc_night_mask: data, the origins and the status words are needed");
  if (S1 < 1 || S2 < 1 || T < 1 || C < 1) S3_FAIL(ctx, S3_EINVAL, "s3_cc_night_mask: empty cube");
  if (T > INT32_MAX || S1 > INT32_MAX || S2 > INT32_MAX)
    S3_FAIL(ctx, S3_EINVAL, "s3_cc_night_mask: 32-bit cube extents (offsets are 64-bit)");
  if (n < 1 || s1 < 1 || s2 < 1) S3_FAIL(ctx, S3_EINVAL, "s3_cc_night_mask: empty batch");
  if (channel < 0 || channel >= C) S3_FAIL(ctx, S3_EINVAL, "s3_cc_night_mask: channel outside [0, C)");
  if (s1 > S1 || s2 > S2 || T < 24) S3_FAIL(ctx, S3_EINVAL, "s3_cc_night_mask: the 24-hour box is larger than the cube");
  for (int m = 0; m < n; ++m) {
    const int* o = origins_host + (size_t)m * 3;
    if (o[0] < 0 || o[1] < 0 || o[2] < 0 || o[0] > S1 - s1 || o[1] > S2 - s2 || o[2] > T - 24)
      S3_FAIL(ctx, S3_EINVAL, "s3_cc_night_mask: a 24-hour box leaves the cube");
  }
  if ((int64_t)s1 * s2 * 24 * kMaxN >= ((int64_t)1 << 31))
    S3_FAIL(ctx, S3_EINVAL, "s3_cc_night_mask: 32-bit element indices of a launch");
  S3_HIP(ctx, hipMemsetAsync(status, 0, S3_CC_STATUS_WORDS * sizeof(int), ctx->stream));
  MaskGeom g;
  g.S2 = S2; g.TC = T * C;
  g.s1 = s1; g.s2 = s2; g.C = C; g.channel = channel;
  g.d24 = FastDiv(24); g.dS2 = FastDiv(s2); g.dS1 = FastDiv(s1);
  for (int m0 = 0; m0 < n; m0 += kMaxN) {
    const int nl = n - m0 < kMaxN ? n - m0 : kMaxN;
    for (int m = 0; m < kMaxN; ++m)
      for (int a = 0; a < 3; ++a) g.org[m][a] = m < nl ? origins_host[(size_t)(m0 + m) * 3 + a] : 0;
    g.total = (uint32_t)((int64_t)nl * s1 * s2 * 24);
    hipLaunchKernelGGL(cc_night_mask_kernel, dim3(grid_for(g.total, ctx->num_cu)), dim3(kBlk), 0, ctx->stream, g,
                       reinterpret_cast<const uint32_t*>(data), reinterpret_cast<unsigned*>(status));
    S3_HIP(ctx, hipGetLastError());
  }
  return S3_OK;
}
