// The arithmetic of the data handlers (sup3r/preprocessing/data_handlers/
// base.py, nc_cc.py over rasterizers/base.py, extended.py) on resident planes:
//   s3_raster_gather      Rasterizer.rasterize_data / _rasterize_flat_data: a
//                         window of a gridded (s1, s2, t [, L]) plane, or the
//                         raster of a time-first (t, sites) plane, as planar
//                         (n_i, n_j, n_k) fields; bit patterns are copied
//   s3_daily_reduce       DailyDataHandler._deriver_hook: the windows of a day
//                         reduced to mean / max / min / sum / ratio of sums
//   s3_site_day_mean      DataHandlerNCforCC.get_clearsky_ghi: mean over the k
//                         nearest sites, then over the steps of a day, then the
//                         '%m.%d' re-index as a day map
//   s3_scale_to_time_max  DataHandlerNCforCC.scale_clearsky_ghi
// The file is compiled with -ffp-contract=off: a sum, a division and a product
// are each rounded once, as numpy rounds them.
//
// s3_raster_gather, flat source.  out[p, k] = src[t0 + k step, site[p]] is a
// gather along the source's fast axis and a transpose.  A workgroup moves a
// tile of 64 raster cells x 64 steps through LDS: a wave reads one step of the
// 64 cells per instruction (one 256-byte line where neighbouring cells are
// neighbouring sites), and writes one cell's 64 steps per instruction (256
// contiguous bytes of the t-contiguous output).  The tile's rows are 65 dwords
// apart: the row-wise ds_write_b32 (lane = cell) and the column-wise
// ds_read_b32 (lane = step, addresses 65 apart) both touch 32 distinct banks
// per 32-lane half.
//
// s3_daily_reduce.  A plane (n_pix, D w) is D n_pix windows of w floats back to
// back, so a workgroup takes a run of `wpb` windows (wpb w floats, contiguous),
// loads it with 16-byte loads per lane — a scalar head and tail where the run
// does not start or end on a 16-byte line — into LDS with the windows an odd
// number of dwords apart, and lane i then walks window i in hour order (lanes
// 32 apart in one half: conflict-free for any odd pitch).  One walk gives the
// count, the fp64 sum, the maximum and the minimum of the non-NaN values, and
// every output of that source is written from them: a source is read once per
// launch however many outputs it serves.  The fp32-rounded sums stay in LDS for
// the ratios, which are written after the last source.
#include "common.h"

namespace {

constexpr int kBlk = kBlock;
constexpr int kMaxPlanes = S3_STACK_MAX_PLANES;
constexpr int kTile = 64, kTilePitch = kTile + 1;

struct GatherPlanes {
  const uint32_t* src[kMaxPlanes];
  uint32_t* out[kMaxPlanes];
};

// gridded: out[pix, r] for r in [0, n_k L): src[((r0 + i) S2 + c0 + j) T L + (t0 + k step) L + l]
__global__ void __launch_bounds__(kBlk)
raster_grid_kernel(GatherPlanes pl, int64_t n_pix, int64_t n_j, int64_t n_k, int64_t n_lev, int64_t src_s2,
                   int64_t src_t, int64_t r0, int64_t c0, int64_t t0, int64_t step) {
  const uint32_t* __restrict__ src = pl.src[blockIdx.y];
  uint32_t* __restrict__ out = pl.out[blockIdx.y];
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * (kBlk / 64) + (threadIdx.x >> 6);
  const int64_t n_wave = (int64_t)gridDim.x * (kBlk / 64);
  const int64_t inner = n_k * n_lev;
  for (int64_t pix = wave; pix < n_pix; pix += n_wave) {
    const int64_t i = pix / n_j, j = pix - i * n_j;
    const uint32_t* __restrict__ s = src + ((r0 + i) * src_s2 + (c0 + j)) * src_t * n_lev + t0 * n_lev;
    uint32_t* __restrict__ o = out + pix * inner;
    if (step == 1) {
      for (int64_t r = lane; r < inner; r += 64) o[r] = s[r];
    } else if (n_lev == 1) {
      for (int64_t r = lane; r < inner; r += 64) o[r] = s[r * step];
    } else {
      for (int64_t r = lane; r < inner; r += 64) {
        const int64_t k = r / n_lev, l = r - k * n_lev;
        o[r] = s[k * step * n_lev + l];
      }
    }
  }
}

// few values per pixel (a 2-D plane, a window of one step): one lane per value
__global__ void __launch_bounds__(kBlk)
raster_grid_small_kernel(GatherPlanes pl, int64_t n_pix, int64_t n_j, int64_t n_k, int64_t n_lev, int64_t src_s2,
                         int64_t src_t, int64_t r0, int64_t c0, int64_t t0, int64_t step) {
  const uint32_t* __restrict__ src = pl.src[blockIdx.y];
  uint32_t* __restrict__ out = pl.out[blockIdx.y];
  const int64_t inner = n_k * n_lev, n = n_pix * inner;
  const int64_t stride = (int64_t)gridDim.x * kBlk;
  for (int64_t e = (int64_t)blockIdx.x * kBlk + threadIdx.x; e < n; e += stride) {
    const int64_t pix = e / inner, r = e - pix * inner;
    const int64_t k = r / n_lev, l = r - k * n_lev;
    const int64_t i = pix / n_j, j = pix - i * n_j;
    out[e] = src[(((r0 + i) * src_s2 + (c0 + j)) * src_t + t0 + k * step) * n_lev + l];
  }
}

// flat: tile (cells p0 .. p0 + 63) x (steps k0 .. k0 + 63), see the top
__global__ void __launch_bounds__(kBlk)
raster_flat_kernel(GatherPlanes pl, const int32_t* __restrict__ site, int64_t n_pix, int64_t n_k, int64_t n_sites,
                   int64_t t0, int64_t step, int64_t tiles_k) {
  __shared__ uint32_t tile[kTile * kTilePitch];
  const uint32_t* __restrict__ src = pl.src[blockIdx.y];
  uint32_t* __restrict__ out = pl.out[blockIdx.y];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t tp = (int64_t)blockIdx.x / tiles_k, tk = (int64_t)blockIdx.x - tp * tiles_k;
  const int64_t p0 = tp * kTile, k0 = tk * kTile;
  const int64_t p = p0 + lane;
  const bool cell = p < n_pix;
  const int64_t s = cell ? (int64_t)site[p] : 0;
#pragma unroll 4
  for (int kk = wave; kk < kTile; kk += kBlk / 64) {
    const int64_t k = k0 + kk;
    uint32_t v = 0;
    if (cell && k < n_k && s >= 0 && s < n_sites) v = src[(t0 + k * step) * n_sites + s];
    tile[kk * kTilePitch + lane] = v;
  }
  __syncthreads();
  const int64_t k = k0 + lane;
#pragma unroll 4
  for (int pp = wave; pp < kTile; pp += kBlk / 64) {
    const int64_t q = p0 + pp;
    if (q < n_pix && k < n_k) out[q * n_k + k] = tile[lane * kTilePitch + pp];
  }
}

// flat, a feature without a time axis: out[p] = src[site[p]]
__global__ void __launch_bounds__(kBlk)
raster_flat1d_kernel(GatherPlanes pl, const int32_t* __restrict__ site, int64_t n_pix, int64_t n_sites) {
  const uint32_t* __restrict__ src = pl.src[blockIdx.y];
  uint32_t* __restrict__ out = pl.out[blockIdx.y];
  const int64_t stride = (int64_t)gridDim.x * kBlk;
  for (int64_t p = (int64_t)blockIdx.x * kBlk + threadIdx.x; p < n_pix; p += stride) {
    const int64_t s = site[p];
    out[p] = s >= 0 && s < n_sites ? src[s] : 0u;
  }
}

// ------------------------------------------------------------ daily reduction
constexpr int kMaxSrc = S3_DAILY_MAX_SRC, kMaxOut = S3_DAILY_MAX_OUT;
constexpr int kDailyLdsFloats = 8192;     // the windows of a workgroup, padded

struct DailyArgs {
  const float* src[kMaxSrc];
  float* out[kMaxOut];
  int8_t osrc[kMaxOut], osrc2[kMaxOut], op[kMaxOut];
  int n_src, n_out;
};

__global__ void __launch_bounds__(kBlk)
daily_reduce_kernel(DailyArgs a, int64_t n_win, int w, int wpb, int pitch, FastDiv by_w) {
  __shared__ float win[kDailyLdsFloats];
  __shared__ float tot[kMaxSrc][kBlk];
  const int tid = threadIdx.x;
  const int64_t g0 = (int64_t)blockIdx.x * wpb;
  const int n_here = (int)(n_win - g0 < wpb ? n_win - g0 : wpb);     // windows of this workgroup
  const int n = n_here * w;                                          // floats of its run
  const int64_t g = g0 + tid;
  const bool mine = tid < n_here;

  auto put = [&](int e, float x) {
    const int q = (int)by_w((uint32_t)e);
    win[q * pitch + (e - q * w)] = x;
  };

  for (int s = 0; s < a.n_src; ++s) {
    const float* __restrict__ p = a.src[s] + g0 * w;
    int head = (int)((4u - (((uintptr_t)p >> 2) & 3u)) & 3u);
    if (head > n) head = n;
    const int nvec = (n - head) / 4;
    const float4* __restrict__ p4 = reinterpret_cast<const float4*>(p + head);
    if (tid < head) put(tid, p[tid]);
#pragma unroll 4
    for (int v = tid; v < nvec; v += kBlk) {
      const float4 q = p4[v];
      const int e = head + 4 * v;
      put(e, q.x); put(e + 1, q.y); put(e + 2, q.z); put(e + 3, q.w);
    }
    {
      const int e = head + 4 * nvec + tid;
      if (e < n) put(e, p[e]);                                       // at most 3
    }
    __syncthreads();
    double sum = 0.0;
    int cnt = 0;
    float mx = __builtin_nanf(""), mn = __builtin_nanf("");
    if (mine) {
      const float* __restrict__ r = win + tid * pitch;
      for (int h = 0; h < w; ++h) {
        const float x = r[h];
        if (x == x) {
          sum += (double)x;
          ++cnt;
          if (!(mx >= x)) mx = x;          // (mx NaN: the first value)
          if (!(mn <= x)) mn = x;
        }
      }
    }
    const float fsum = (float)sum;
    tot[s][tid] = fsum;
    if (mine) {
      for (int o = 0; o < a.n_out; ++o) {
        if (a.osrc[o] != s) continue;
        const int op = a.op[o];
        if (op == S3_DAILY_RATIO) continue;
        float v = fsum;
        if (op == S3_DAILY_MEAN) v = (float)(sum / (double)cnt);     // 0 / 0: NaN for an all-NaN window
        else if (op == S3_DAILY_MAX) v = mx;
        else if (op == S3_DAILY_MIN) v = mn;
        a.out[o][g] = v;
      }
    }
    __syncthreads();                       // (win is overwritten by the next source)
  }
  if (mine) {
    for (int o = 0; o < a.n_out; ++o)
      if (a.op[o] == S3_DAILY_RATIO) a.out[o][g] = __fdiv_rn(tot[a.osrc[o]][tid], tot[a.osrc2[o]][tid]);
  }
}

// ------------------------------------------------------- site mean, day mean
__global__ void __launch_bounds__(kBlk)
site_day_mean_kernel(const float* __restrict__ src, int64_t t_src, int64_t n_sites, const int32_t* __restrict__ idx,
                     int64_t n_pix, int k, int64_t t_lo, int m, int64_t n_src_days,
                     const int32_t* __restrict__ day_map, int64_t d_out, float* __restrict__ out) {
  const int64_t n = n_pix * d_out;
  const int64_t stride = (int64_t)gridDim.x * kBlk;
  for (int64_t e = (int64_t)blockIdx.x * kBlk + threadIdx.x; e < n; e += stride) {
    const int64_t p = e / d_out, d = e - p * d_out;
    const int64_t day = day_map[d];
    float r = __builtin_nanf("");
    if (day >= 0 && day < n_src_days) {
      double acc = 0.0;
      int steps = 0;
      for (int s = 0; s < m; ++s) {
        const int64_t t = t_lo + day * m + s;
        double a = 0.0;
        int sites = 0;
        for (int q = 0; q < k; ++q) {
          const int64_t site = idx[p * k + q];
          if (site < 0 || site >= n_sites || t >= t_src) continue;
          const float x = src[t * n_sites + site];
          if (x == x) { a += (double)x; ++sites; }
        }
        if (sites) {
          const double mean = a / (double)sites;
          if (mean == mean) { acc += mean; ++steps; }    // (+inf and -inf among the sites)
        }
      }
      r = (float)(acc / (double)steps);
    }
    out[e] = r;
  }
}

// -------------------------------------------------------- scale to time max
__device__ __forceinline__ float wave_nanmax(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float o = __shfl_xor(v, off, 64);
    if (!(v >= o) && o == o) v = o;
  }
  return v;
}

// a wave per pixel
__global__ void __launch_bounds__(kBlk)
scale_to_time_max_kernel(const float* __restrict__ a, float* __restrict__ b, int64_t n_pix, int64_t t,
                         float* __restrict__ scale) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * (kBlk / 64) + (threadIdx.x >> 6);
  const int64_t n_wave = (int64_t)gridDim.x * (kBlk / 64);
  for (int64_t p = wave; p < n_pix; p += n_wave) {
    const float* __restrict__ ap = a + p * t;
    float* __restrict__ bp = b + p * t;
    float ma = __builtin_nanf(""), mb = __builtin_nanf("");
    for (int64_t j = lane; j < t; j += 64) {
      const float x = ap[j], y = bp[j];
      if (x == x && !(ma >= x)) ma = x;
      if (y == y && !(mb >= y)) mb = y;
    }
    ma = wave_nanmax(ma);
    mb = wave_nanmax(mb);
    const float sc = __fdiv_rn(ma, mb);
    if (lane == 0) scale[p] = sc;
    for (int64_t j = lane; j < t; j += 64) bp[j] = __fmul_rn(bp[j], sc);
  }
}

bool mul_fits(int64_t a, int64_t b, int64_t limit = INT64_MAX / 8) { return a == 0 || b <= limit / a; }

}  // namespace

extern "C" int s3_raster_gather(s3_ctx* ctx, int layout, int n_planes, const float* const* src_host,
                                float* const* out_host, int64_t n_i, int64_t n_j, int64_t n_k, int64_t n_lev,
                                int64_t src_s1, int64_t src_s2, int64_t src_t, int64_t r0, int64_t c0, int64_t t0,
                                int64_t step, const int32_t* site) {
  if (!ctx) return S3_EINVAL;
  if (!src_host || !out_host) S3_FAIL(ctx, S3_EINVAL, "s3_raster_gather: the plane tables are needed");
  if (n_planes < 1 || n_planes > kMaxPlanes) S3_FAIL(ctx, S3_EINVAL, "s3_raster_gather: 1 .. 32 planes per launch");
  if (n_i < 1 || n_j < 1 || n_k < 1 || n_lev < 1) S3_FAIL(ctx, S3_EINVAL, "s3_raster_gather: empty raster");
  if (src_s1 < 1 || src_s2 < 1 || src_t < 1) S3_FAIL(ctx, S3_EINVAL, "s3_raster_gather: empty source");
  if (!mul_fits(n_i, n_j) || !mul_fits(n_i * n_j, n_k) || !mul_fits(n_i * n_j * n_k, n_lev) ||
      !mul_fits(src_s1, src_s2) || !mul_fits(src_s1 * src_s2, src_t) || !mul_fits(src_s1 * src_s2 * src_t, n_lev))
    S3_FAIL(ctx, S3_EINVAL, "s3_raster_gather: a plane's size overflows");
  GatherPlanes pl;
  for (int i = 0; i < kMaxPlanes; ++i) {
    pl.src[i] = nullptr;
    pl.out[i] = nullptr;
  }
  for (int i = 0; i < n_planes; ++i) {
    if (!src_host[i] || !out_host[i]) S3_FAIL(ctx, S3_EINVAL, "s3_raster_gather: a plane is missing");
    if (((uintptr_t)src_host[i] & 3u) || ((uintptr_t)out_host[i] & 3u))
      S3_FAIL(ctx, S3_EINVAL, "s3_raster_gather: a misaligned plane");
    pl.src[i] = reinterpret_cast<const uint32_t*>(src_host[i]);
    pl.out[i] = reinterpret_cast<uint32_t*>(out_host[i]);
  }
  const int64_t n_pix = n_i * n_j;
  // the steps read: t0, t0 + step, .., t0 + (n_k - 1) step
  const bool steps_ok = step >= 1 && t0 >= 0 && t0 < src_t && mul_fits(n_k - 1, step, INT64_MAX / 2) &&
                        t0 + (n_k - 1) * step < src_t;
  if (layout == S3_RG_GRID) {
    if (!steps_ok) S3_FAIL(ctx, S3_EINVAL, "s3_raster_gather: the time steps leave the source");
    if (r0 < 0 || c0 < 0 || r0 + n_i > src_s1 || c0 + n_j > src_s2)
      S3_FAIL(ctx, S3_EINVAL, "s3_raster_gather: the window leaves the source grid");
    const int64_t inner = n_k * n_lev;
    if (inner >= 32) {
      const int grid = grid_for(n_pix * 64, ctx->num_cu, 8);
      hipLaunchKernelGGL(raster_grid_kernel, dim3(grid, n_planes), dim3(kBlk), 0, ctx->stream, pl, n_pix, n_j, n_k,
                         n_lev, src_s2, src_t, r0, c0, t0, step);
    } else {
      const int grid = grid_for(n_pix * inner, ctx->num_cu, 8);
      hipLaunchKernelGGL(raster_grid_small_kernel, dim3(grid, n_planes), dim3(kBlk), 0, ctx->stream, pl, n_pix, n_j,
                         n_k, n_lev, src_s2, src_t, r0, c0, t0, step);
    }
  } else if (layout == S3_RG_FLAT || layout == S3_RG_FLAT_1D) {
    // the source is (src_t, src_s2) [FLAT] or (src_s2) [FLAT_1D]; a cell whose
    // entry of `site` is outside [0, src_s2) is written as zero bits
    if (!site) S3_FAIL(ctx, S3_EINVAL, "s3_raster_gather: a flat source needs the site table");
    if ((uintptr_t)site & 3u) S3_FAIL(ctx, S3_EINVAL, "s3_raster_gather: misaligned site table");
    if (n_lev != 1 || src_s1 != 1) S3_FAIL(ctx, S3_EINVAL, "s3_raster_gather: a flat source has no level axis");
    if (src_s2 > INT32_MAX) S3_FAIL(ctx, S3_EINVAL, "s3_raster_gather: more than 2^31 - 1 sites");
    if (layout == S3_RG_FLAT_1D) {
      if (n_k != 1) S3_FAIL(ctx, S3_EINVAL, "s3_raster_gather: a 1-D feature has one value per site");
      const int grid = grid_for(n_pix, ctx->num_cu, 8);
      hipLaunchKernelGGL(raster_flat1d_kernel, dim3(grid, n_planes), dim3(kBlk), 0, ctx->stream, pl, site, n_pix,
                         src_s2);
    } else {
      if (!steps_ok) S3_FAIL(ctx, S3_EINVAL, "s3_raster_gather: the time steps leave the source");
      const int64_t tiles_p = (n_pix + kTile - 1) / kTile, tiles_k = (n_k + kTile - 1) / kTile;
      if (!mul_fits(tiles_p, tiles_k, INT32_MAX)) S3_FAIL(ctx, S3_EINVAL, "s3_raster_gather: more than 2^31 - 1 tiles");
      hipLaunchKernelGGL(raster_flat_kernel, dim3((unsigned)(tiles_p * tiles_k), n_planes), dim3(kBlk), 0, ctx->stream,
                         pl, site, n_pix, n_k, src_s2, t0, step, tiles_k);
    }
  } else {
    S3_FAIL(ctx, S3_EINVAL, "s3_raster_gather: unknown layout");
  }
  S3_HIP(ctx, hipGetLastError());
  return S3_OK;
}

extern "C" int s3_daily_reduce(s3_ctx* ctx, int n_src, const float* const* src_host, int64_t n_pix, int64_t n_days,
                               int w, int n_out, const int* out_src_host, const int* out_src2_host,
                               const int* out_op_host, float* const* out_host) {
  if (!ctx) return S3_EINVAL;
  if (!src_host || !out_src_host || !out_op_host || !out_host)
    S3_FAIL(ctx, S3_EINVAL, "s3_daily_reduce: the source and output tables are needed");
  if (n_src < 1 || n_src > kMaxSrc) S3_FAIL(ctx, S3_EINVAL, "s3_daily_reduce: 1 .. S3_DAILY_MAX_SRC sources");
  if (n_out < 1 || n_out > kMaxOut) S3_FAIL(ctx, S3_EINVAL, "s3_daily_reduce: 1 .. S3_DAILY_MAX_OUT outputs");
  if (n_pix < 1 || n_days < 1 || w < 1) S3_FAIL(ctx, S3_EINVAL, "s3_daily_reduce: empty planes");
  const int pitch = w | 1;
  if (pitch > kDailyLdsFloats) S3_FAIL(ctx, S3_EINVAL, "s3_daily_reduce: a window of more than 8191 steps");
  if (!mul_fits(n_pix, n_days) || !mul_fits(n_pix * n_days, w))
    S3_FAIL(ctx, S3_EINVAL, "s3_daily_reduce: a plane's size overflows");
  DailyArgs a;
  a.n_src = n_src;
  a.n_out = n_out;
  for (int i = 0; i < kMaxSrc; ++i) a.src[i] = nullptr;
  for (int i = 0; i < kMaxOut; ++i) {
    a.out[i] = nullptr;
    a.osrc[i] = a.osrc2[i] = a.op[i] = 0;
  }
  for (int i = 0; i < n_src; ++i) {
    if (!src_host[i] || ((uintptr_t)src_host[i] & 3u)) S3_FAIL(ctx, S3_EINVAL, "s3_daily_reduce: a missing or misaligned source");
    a.src[i] = src_host[i];
  }
  for (int o = 0; o < n_out; ++o) {
    const int op = out_op_host[o];
    if (op < S3_DAILY_MEAN || op > S3_DAILY_RATIO) S3_FAIL(ctx, S3_EINVAL, "s3_daily_reduce: unknown op");
    if (out_src_host[o] < 0 || out_src_host[o] >= n_src) S3_FAIL(ctx, S3_EINVAL, "s3_daily_reduce: an output's source is outside the table");
    int second = 0;
    if (op == S3_DAILY_RATIO) {
      if (!out_src2_host || out_src2_host[o] < 0 || out_src2_host[o] >= n_src)
        S3_FAIL(ctx, S3_EINVAL, "s3_daily_reduce: a ratio's second source is outside the table");
      second = out_src2_host[o];
    }
    if (!out_host[o] || ((uintptr_t)out_host[o] & 3u)) S3_FAIL(ctx, S3_EINVAL, "s3_daily_reduce: a missing or misaligned output");
    a.out[o] = out_host[o];
    a.osrc[o] = (int8_t)out_src_host[o];
    a.osrc2[o] = (int8_t)second;
    a.op[o] = (int8_t)op;
  }
  const int64_t n_win = n_pix * n_days;
  int wpb = kDailyLdsFloats / pitch;
  if (wpb > kBlk) wpb = kBlk;
  const int64_t grid = (n_win + wpb - 1) / wpb;
  if (grid > INT32_MAX) S3_FAIL(ctx, S3_EINVAL, "s3_daily_reduce: more than 2^31 - 1 workgroups");
  hipLaunchKernelGGL(daily_reduce_kernel, dim3((unsigned)grid), dim3(kBlk), 0, ctx->stream, a, n_win, w, wpb, pitch,
                     FastDiv((uint32_t)w));
  S3_HIP(ctx, hipGetLastError());
  return S3_OK;
}

extern "C" int s3_site_day_mean(s3_ctx* ctx, const float* src, int64_t t_src, int64_t n_sites, const int32_t* idx,
                                int64_t n_pix, int k, int64_t t_lo, int m, const int32_t* day_map, int64_t d_out,
                                float* out) {
  if (!ctx) return S3_EINVAL;
  if (!src || !idx || !day_map || !out) S3_FAIL(ctx, S3_EINVAL, "s3_site_day_mean: src, idx, day_map and out are needed");
  if (((uintptr_t)src & 3u) || ((uintptr_t)idx & 3u) || ((uintptr_t)day_map & 3u) || ((uintptr_t)out & 3u))
    S3_FAIL(ctx, S3_EINVAL, "s3_site_day_mean: a misaligned pointer");
  if (t_src < 1 || n_sites < 1 || n_pix < 1 || d_out < 1 || k < 1 || m < 1)
    S3_FAIL(ctx, S3_EINVAL, "s3_site_day_mean: empty input");
  if (t_lo < 0 || t_lo >= t_src) S3_FAIL(ctx, S3_EINVAL, "s3_site_day_mean: t_lo outside the source");
  if (!mul_fits(t_src, n_sites) || !mul_fits(n_pix, d_out) || !mul_fits(n_pix, k))
    S3_FAIL(ctx, S3_EINVAL, "s3_site_day_mean: a plane's size overflows");
  const int64_t n_src_days = (t_src - t_lo) / m;       // whole days behind t_lo: a map entry beyond them gives NaN
  const int grid = grid_for(n_pix * d_out, ctx->num_cu, 8);
  hipLaunchKernelGGL(site_day_mean_kernel, dim3(grid), dim3(kBlk), 0, ctx->stream, src, t_src, n_sites, idx, n_pix, k,
                     t_lo, m, n_src_days, day_map, d_out, out);
  S3_HIP(ctx, hipGetLastError());
  return S3_OK;
}

extern "C" int s3_scale_to_time_max(s3_ctx* ctx, const float* a, float* b, int64_t n_pix, int64_t t, float* scale) {
  if (!ctx) return S3_EINVAL;
  if (!a || !b || !scale) S3_FAIL(ctx, S3_EINVAL, "s3_scale_to_time_max: a, b and scale are needed");
  if (((uintptr_t)a & 3u) || ((uintptr_t)b & 3u) || ((uintptr_t)scale & 3u))
    S3_FAIL(ctx, S3_EINVAL, "s3_scale_to_time_max: a misaligned pointer");
  if (n_pix < 1 || t < 1) S3_FAIL(ctx, S3_EINVAL, "s3_scale_to_time_max: empty planes");
  if (!mul_fits(n_pix, t)) S3_FAIL(ctx, S3_EINVAL, "s3_scale_to_time_max: a plane's size overflows");
  const int grid = grid_for(n_pix * 64, ctx->num_cu, 8);
  hipLaunchKernelGGL(scale_to_time_max_kernel, dim3(grid), dim3(kBlk), 0, ctx->stream, a, b, n_pix, t, scale);
  S3_HIP(ctx, hipGetLastError());
  return S3_OK;
}
