// The fork-join hand-over of SolarMultiStepGan
// (sup3r/models/multi_step.py:733-822) and its reflect pad along time.
//
// s3_branch_join: the two spatial branches (solar: clearsky_ratio, wind: u / v)
// end in 2-D generators, whose outputs ya = (t, h, w, ca) and yb = (t, h, w, cb)
// are time-FIRST and normalised; the temporal chain takes ONE normalised sample
// x = (1, h, w, t, na + nb), time-LAST.  Per destination channel k:
//   k <  na : x[0,i,j,s,k] = norm_k(unnorm_a(ya[s,i,j,map_a[k]]))
//   k >= na : x[0,i,j,s,k] = norm_k(unnorm_b(yb[s,i,j,map_b[k - na]]))
// un_norm_output of either branch (y * std + mean per SOURCE channel), the
// channel selection hi_res_wind[..., idf_wind_out], np.concatenate, the
// transpose (1, 2, 0, 3) and norm_input of the first temporal step ((v - mean)
// / std per DESTINATION channel) — numpy's fp32 arithmetic, one rounding per
// operation, no fused multiply-add, the same for every bit pattern.
//
// Layout.  The sources are contiguous along (w, c) at fixed (s, i), the
// destination along (s, k) at fixed (i, j): with 1 - 3 channels a lane per
// element would touch 4 - 12 bytes per row on one of the two sides.  A block
// therefore stages a tile of kTileW columns x kTileT time steps of one image
// row i in LDS, as finished destination values tile[s][j * nc + k]:
//   * fill: lanes run along (j, k) of one time step, then the next: the loads
//     of either source walk a contiguous run of kTileW * c floats per time step
//     (128 B and more per source and wave for c >= 1) and the LDS writes are
//     consecutive words;
//   * drain: lanes run along (s, k) of one column, then the next column: the
//     stores walk the destination in memory order — the tile's columns are one
//     contiguous run when it covers all of t, runs of kTileT * nc floats (64 B
//     and more) otherwise.
// The LDS row stride is kTileW * nc + nc words: stepping s moves nc banks, as
// stepping k within the run does, so a drain over one column reads consecutive
// banks ((s * nc + k) mod 32).  Where a column's run is shorter than 32 words
// (t * nc < 32) the next column starts nc banks on and a wave half sees a
// 2-way conflict on part of its lanes; the kernel is bound by its global
// traffic, not by LDS.
//
// s3_time_pad_reflect: np.pad(..., mode='reflect') along the time axis of the
// last step's output, any pad width, fused with un_norm_output.
#include "common.h"

namespace {

constexpr int kBlk = kBlock;   // grid_for counts workgroups of this size
constexpr int kTileW = 32;     // columns of one image row per tile
constexpr int kTileT = 16;     // time steps per tile
constexpr int kMaxC = 16;

struct JoinGeom {
  int64_t t, h, w;
  int64_t wt, tt, ntiles;      // tiles along w, along t, in all (h * wt * tt)
  int ca, cb, na, nc;          // source channels, channels kept of a, destination channels
  int un_a, un_b, nrm;
  int map[kMaxC];              // destination channel -> source channel (of a: k < na, of b: the rest)
  float scale[kMaxC], shift[kMaxC], mean[kMaxC], sd[kMaxC];   // all per DESTINATION channel
};

__global__ void __launch_bounds__(kBlk)
branch_join_kernel(JoinGeom g, const float* __restrict__ ya, const float* __restrict__ yb,
                   float* __restrict__ x) {
  extern __shared__ float tile[];
  // (the tables are indexed per lane: out of LDS, not out of a private copy
  // of the kernel arguments)
  __shared__ int s_map[kMaxC];
  __shared__ float s_scale[kMaxC], s_shift[kMaxC], s_mean[kMaxC], s_sd[kMaxC];
  if (threadIdx.x < kMaxC) {
    s_map[threadIdx.x] = g.map[threadIdx.x];
    s_scale[threadIdx.x] = g.scale[threadIdx.x];
    s_shift[threadIdx.x] = g.shift[threadIdx.x];
    s_mean[threadIdx.x] = g.mean[threadIdx.x];
    s_sd[threadIdx.x] = g.sd[threadIdx.x];
  }
  __syncthreads();
  const int nc = g.nc;
  const int rs = kTileW * nc + nc;               // LDS row stride (words)
  for (int64_t tid = blockIdx.x; tid < g.ntiles; tid += gridDim.x) {
    int64_t r = tid;
    const int64_t tj = r % g.wt; r /= g.wt;
    const int64_t ts = r % g.tt; r /= g.tt;
    const int64_t i = r;
    const int64_t w0 = tj * kTileW, s0 = ts * kTileT;
    const int nw = (int)(g.w - w0 < kTileW ? g.w - w0 : kTileW);
    const int nt = (int)(g.t - s0 < kTileT ? g.t - s0 : kTileT);
    const int row = nw * nc;                     // destination words per time step of the tile
    // fill: e runs over (s, j, k)
    for (int e = threadIdx.x; e < nt * row; e += kBlk) {
      const int s = e / row, q = e - s * row;
      const int j = q / nc, k = q - j * nc;
      const int64_t pos = ((s0 + s) * g.h + i) * g.w + w0 + j;     // (s, i, j) of the sources
      float v;
      bool un;
      if (k < g.na) { v = ya[pos * g.ca + s_map[k]]; un = g.un_a; }
      else { v = yb[pos * g.cb + s_map[k]]; un = g.un_b; }
      if (un) {
        // two roundings, as numpy's (y * std) + mean
        float m = v * s_scale[k];
        asm volatile("" : "+v"(m));
        v = m + s_shift[k];
      }
      if (g.nrm) {
        float d = v - s_mean[k];
        asm volatile("" : "+v"(d));
        v = __fdiv_rn(d, s_sd[k]);
      }
      tile[s * rs + q] = v;
    }
    __syncthreads();
    // drain: e runs over (j, s, k), the destination's memory order
    const int run = nt * nc;
    for (int e = threadIdx.x; e < nw * run; e += kBlk) {
      const int j = e / run, q = e - j * run;
      const int s = q / nc, k = q - s * nc;
      x[(((i * g.w + w0 + j) * g.t) + s0) * nc + q] = tile[s * rs + j * nc + k];
    }
    __syncthreads();
  }
}

struct PadGeom {
  int64_t outer, t, pad;
  int c, affine;
  float scale[kMaxC], shift[kMaxC];
};

// numpy's mode='reflect' for any pad width: repeated reflection about the two
// ends is the triangle wave of period 2 (t - 1); a length-1 axis repeats its
// one value
__device__ __forceinline__ int64_t reflect_index(int64_t j, int64_t t) {
  if (t == 1) return 0;
  const int64_t p = 2 * (t - 1);
  const int64_t m = ((j % p) + p) % p;
  return m < t ? m : p - m;
}

__global__ void __launch_bounds__(kBlk)
time_pad_reflect_kernel(PadGeom g, const float* __restrict__ y, float* __restrict__ out) {
  const int64_t tp = g.t + 2 * g.pad;
  const int64_t total = g.outer * tp * g.c;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    int64_t r = i / g.c;
    const int q = (int)(i - r * g.c);
    const int64_t o = r / tp;
    const int64_t k = r - o * tp;
    float v = y[(o * g.t + reflect_index(k - g.pad, g.t)) * g.c + q];
    if (g.affine) {
      float m = v * g.scale[q];
      asm volatile("" : "+v"(m));
      v = m + g.shift[q];
    }
    out[i] = v;
  }
}

}  // namespace

extern "C" int s3_branch_join(s3_ctx* ctx, const float* ya, int ca, const int* map_a_host, int na,
                              const float* scale_a_host, const float* shift_a_host,
                              const float* yb, int cb, const int* map_b_host, int nb,
                              const float* scale_b_host, const float* shift_b_host,
                              int64_t t, int64_t h, int64_t w,
                              const float* mean_host, const float* std_host, float* x) {
  if (!ctx || !x) return S3_EINVAL;
  if (ca < 0 || cb < 0 || na < 0 || nb < 0 || ca > kMaxC || cb > kMaxC || na + nb > kMaxC || na + nb < 1)
    S3_FAIL(ctx, S3_EINVAL, "branch_join: at most 16 channels per source, 1 .. 16 at the destination");
  if (t < 1 || h < 1 || w < 1) S3_FAIL(ctx, S3_EINVAL, "branch_join: empty extent");
  if ((na > 0 && (!ya || !map_a_host || ca < 1)) || (nb > 0 && (!yb || !map_b_host || cb < 1)))
    S3_FAIL(ctx, S3_EINVAL, "branch_join: channels kept of a source that is not there");
  JoinGeom g;
  g.t = t; g.h = h; g.w = w;
  g.wt = (w + kTileW - 1) / kTileW;
  g.tt = (t + kTileT - 1) / kTileT;
  g.ntiles = h * g.wt * g.tt;
  g.ca = ca; g.cb = cb; g.na = na; g.nc = na + nb;
  g.un_a = scale_a_host && shift_a_host;
  g.un_b = scale_b_host && shift_b_host;
  g.nrm = mean_host && std_host;
  for (int k = 0; k < kMaxC; ++k) {
    g.map[k] = 0; g.scale[k] = 1.f; g.shift[k] = 0.f; g.mean[k] = 0.f; g.sd[k] = 1.f;
    if (k >= g.nc) continue;
    const bool a = k < na;
    const int src = a ? map_a_host[k] : map_b_host[k - na];
    if (src < 0 || src >= (a ? ca : cb)) S3_FAIL(ctx, S3_EINVAL, "branch_join: channel map out of range");
    g.map[k] = src;
    if (a ? g.un_a : g.un_b) {
      g.scale[k] = (a ? scale_a_host : scale_b_host)[src];
      g.shift[k] = (a ? shift_a_host : shift_b_host)[src];
    }
    if (g.nrm) { g.mean[k] = mean_host[k]; g.sd[k] = std_host[k]; }
  }
  const int grid = grid_for(g.ntiles * kBlock, ctx->num_cu);   // a workgroup per tile, the rest by grid stride
  const size_t lds = (size_t)kTileT * (kTileW * g.nc + g.nc) * sizeof(float);   // <= 33 KiB
  hipLaunchKernelGGL(branch_join_kernel, dim3(grid), dim3(kBlk), lds, ctx->stream, g, ya, yb, x);
  S3_HIP(ctx, hipGetLastError());
  return S3_OK;
}

extern "C" int s3_time_pad_reflect(s3_ctx* ctx, const float* y, int64_t outer, int64_t t, int c,
                                   int64_t pad, const float* scale_host, const float* shift_host,
                                   float* out) {
  if (!ctx || !y || !out) return S3_EINVAL;
  if (c < 1 || c > kMaxC) S3_FAIL(ctx, S3_EINVAL, "time_pad_reflect: 1 .. 16 channels");
  if (outer < 1 || t < 1 || pad < 0) S3_FAIL(ctx, S3_EINVAL, "time_pad_reflect: empty extent or negative pad");
  PadGeom g;
  g.outer = outer; g.t = t; g.pad = pad; g.c = c;
  g.affine = scale_host && shift_host;
  for (int k = 0; k < kMaxC; ++k) {
    g.scale[k] = g.affine && k < c ? scale_host[k] : 1.f;
    g.shift[k] = g.affine && k < c ? shift_host[k] : 0.f;
  }
  const int64_t total = outer * (t + 2 * pad) * c;
  hipLaunchKernelGGL(time_pad_reflect_kernel, dim3(grid_for(total, ctx->num_cu)), dim3(kBlk), 0,
                     ctx->stream, g, y, out);
  S3_HIP(ctx, hipGetLastError());
  return S3_OK;
}
