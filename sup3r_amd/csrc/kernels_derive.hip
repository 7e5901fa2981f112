// Deriving input features on the device: the arithmetic of
// sup3r/preprocessing/derivers (methods.py, utilities.py) and of
// Interpolator.interp_to_level (sup3r/utilities/interpolation.py:13-173).
//   s3_level_interp      all variables and all target levels of one level
//                        structure in one pass
//   s3_derive_pointwise  the elementwise compute() methods, planar
//   s3_time_flags        per step: any value <= threshold / any NaN
//   s3_stack_features    planar (s1 s2, t) planes -> (s1 s2, t, C), time roll fused
//   s3_level_stats       the counts and extrema behind the level check's warnings
// The reference makes about fifteen full-size dask passes per interpolated
// feature (four masked arrays, four masked argmins, where / nanmean passes),
// again for every height and variable.  Here a wave owns 64 columns: their
// levels are ONE contiguous run of 256 L bytes, loaded 16 bytes per lane and
// handed to the lanes through LDS (row stride odd: the 64 lanes of a read hit
// 64 different banks); each lane then scans its column once per target and
// keeps (i1, i2, lev1, lev2) in LDS; every variable's run is staged through
// the same tile and costs two LDS reads per target.  Each input element is
// read from memory once, each output written once, both coalesced.  The
// scattering LDS stores of a staged run (4 consecutive elements per lane) are
// 4-way conflicted ds_write_b32, twice their conflict-free cost.  Measured
// (profiles/derive/NOTES.md): 0.62 of a copy's rate for one variable and one
// target, 0.40 for two variables and three targets — the per-target scans and
// the barriers around them, not memory, are what the larger launch waits for.
// Every output value is produced by one lane from its own column: nothing
// depends on the launch geometry.  No float atomics (s3_time_flags ORs ints).
#include "common.h"

namespace {

constexpr int kBlk = kBlock;
constexpr int kWave = 64;
constexpr int kMaxLev = S3_LI_MAX_LEVELS;
constexpr int kMaxSl = S3_LI_MAX_SINGLE;
constexpr int kMaxVar = S3_LI_MAX_VARS;
constexpr int kMaxOut = S3_LI_MAX_TARGETS;

struct LevelArgs {
  int64_t P, t;
  int L_ml, n_sl, n_var, n_out, method, lev_vector, topo_per_step, vec4;
  FastDiv divL;
  const float* lev_ml;
  const float* topo;
  float lev_vec[kMaxLev];
  float sl_level[kMaxSl];
  float target[kMaxOut];
  const float* var_ml[kMaxVar];
  const float* var_sl[kMaxVar * kMaxSl];
  float* out[kMaxVar * kMaxOut];
};

// the wave's run src[0 .. n) (n = columns x L_ml) into tile[column][level]
__device__ __forceinline__ void stage_run(float* tile, const float* __restrict__ src, int n, int L_ml, int Ls,
                                          const FastDiv& divL, int lane, int vec4) {
  int done = 0;
  if (vec4) {
    const int n4 = n >> 2;
    const float4* src4 = reinterpret_cast<const float4*>(src);
#pragma unroll 4
    for (int q = lane; q < n4; q += kWave) {
      const float4 v = src4[q];
      const float e4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t e = (uint32_t)(4 * q + j);
        const uint32_t c = divL(e);
        tile[c * Ls + (e - c * L_ml)] = e4[j];
      }
    }
    done = n4 << 2;
  }
  for (int e = done + lane; e < n; e += kWave) {
    const uint32_t c = divL((uint32_t)e);
    tile[c * Ls + ((uint32_t)e - c * L_ml)] = src[e];
  }
}

// level i of a lane's column: a single-level constant, the shared vector, or
// the staged column value minus the topography (one fp32 subtraction, as numpy's)
__device__ __forceinline__ float level_at(const LevelArgs& a, const float* mine, int i, bool has_topo, float topo) {
  if (i >= a.L_ml) return a.sl_level[i - a.L_ml];
  if (a.lev_vector) return a.lev_vec[i];
  return has_topo ? __fsub_rn(mine[i], topo) : mine[i];
}

struct Pick {
  int idx;
  float lev;
  bool found;
};
__device__ __forceinline__ void pick(Pick& p, int i, float lv, float d, float& best) {
  if (!p.found || d < best) { p.found = true; p.idx = i; p.lev = lv; best = d; }
}

// Dynamic LDS per wave: tile[64][Ls] floats, then per target sel[64] (i1 | i2
// << 8), lev1[64], lev2[64].  The loop bounds are workgroup-uniform: every
// barrier is reached by the whole workgroup (a wave past the last tile has no
// columns and only keeps the barriers company).
__global__ void __launch_bounds__(kBlk) level_interp_kernel(LevelArgs a) {
#pragma clang fp contract(off)
  extern __shared__ float lds[];
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6, waves = blockDim.x >> 6;
  const int L = a.L_ml + a.n_sl, Ls = L | 1;
  const int per_wave = kWave * Ls + 3 * kWave * a.n_out;
  float* tile = lds + (size_t)w * per_wave;
  uint32_t* sel = reinterpret_cast<uint32_t*>(tile + kWave * Ls);
  float* lev1 = tile + kWave * Ls + kWave * a.n_out;
  float* lev2 = lev1 + kWave * a.n_out;
  const int64_t n_tiles = (a.P + kWave - 1) / kWave;
  for (int64_t tile0 = (int64_t)blockIdx.x * waves; tile0 < n_tiles; tile0 += (int64_t)gridDim.x * waves) {
    const int64_t col0 = (tile0 + w) * kWave;
    const int ncols = col0 >= a.P ? 0 : (a.P - col0 < kWave ? (int)(a.P - col0) : kWave);
    const int64_t col = col0 + lane;
    const bool live = lane < ncols;
    // 1) the levels of the 64 columns
    if (!a.lev_vector && a.L_ml > 0 && ncols > 0)
      stage_run(tile, a.lev_ml + col0 * a.L_ml, ncols * a.L_ml, a.L_ml, Ls, a.divL, lane, a.vec4);
    __syncthreads();
    if (live) {
      float topo = 0.f;
      const bool has_topo = !a.lev_vector && a.topo != nullptr;
      if (has_topo) topo = a.topo[a.topo_per_step ? col : col / a.t];
      const float* mine = tile + lane * Ls;
      for (int k = 0; k < a.n_out; ++k) {
        const float target = a.target[k];
        Pick below = {0, 0.f, false}, above = {0, 0.f, false}, all = {0, 0.f, false};
        float bb = 0.f, ba = 0.f, bl = 0.f;
        for (int i = 0; i < L; ++i) {
          const float lv = level_at(a, mine, i, has_topo, topo);
          if (lv != lv) continue;
          const float d = fabsf(__fsub_rn(lv, target));
          if (lv < target) pick(below, i, lv, d, bb); else pick(above, i, lv, d, ba);
          pick(all, i, lv, d, bl);
        }
        // (no valid level at all: index 0, whose level is NaN or, for L = 1
        // with a valid level, found above)
        Pick p1 = below.found ? below : all, p2 = above;
        const float lv0 = level_at(a, mine, 0, has_topo, topo);
        if (!p1.found) { p1.idx = 0; p1.lev = lv0; }
        if (!above.found) {
          Pick alt = {0, lv0, false};
          float bt = 0.f;
          for (int i = 0; i < L; ++i) {
            if (i == p1.idx) continue;
            const float lv = level_at(a, mine, i, has_topo, topo);
            if (lv != lv) continue;
            pick(alt, i, lv, fabsf(__fsub_rn(lv, target)), bt);
          }
          p2 = alt;
        }
        sel[k * kWave + lane] = (uint32_t)p1.idx | ((uint32_t)p2.idx << 8);
        lev1[k * kWave + lane] = p1.lev;
        lev2[k * kWave + lane] = p2.lev;
      }
    }
    // 2) every variable through the same tile
    for (int v = 0; v < a.n_var; ++v) {
      __syncthreads();                               // the tile's readers are done
      if (a.L_ml > 0 && ncols > 0)
        stage_run(tile, a.var_ml[v] + col0 * a.L_ml, ncols * a.L_ml, a.L_ml, Ls, a.divL, lane, a.vec4);
      if (live)
        for (int s = 0; s < a.n_sl; ++s) tile[lane * Ls + a.L_ml + s] = a.var_sl[v * a.n_sl + s][col];
      __syncthreads();
      if (!live) continue;
      for (int k = 0; k < a.n_out; ++k) {
        const uint32_t se = sel[k * kWave + lane];
        const float l1 = lev1[k * kWave + lane], l2 = lev2[k * kWave + lane];
        const float v1 = tile[lane * Ls + (se & 255u)], v2 = tile[lane * Ls + (se >> 8)];
        const float target = a.target[k];
        float r;
        if (a.method == S3_LI_LOG) {
          const bool m = l1 < l2;
          const float h0 = m ? l1 : l2, h1 = m ? l2 : l1, w0 = m ? v1 : v2, w1 = m ? v2 : v1;
          float coeff = h1 == h0 ? 0.f : __fdiv_rn(__fsub_rn(w1, w0), logf(__fadd_rn(__fsub_rn(h1, h0), 1.f)));
          if (target < h0) coeff = -coeff;
          r = __fadd_rn(__fmul_rn(coeff, logf(__fadd_rn(fabsf(__fsub_rn(target, h0)), 1.f))), w0);
        } else {
          const float diff = __fsub_rn(l2, l1);
          const float alpha = fabsf(diff) < 1e-3f ? 0.f : __fdiv_rn(__fsub_rn(target, l1), diff);
          r = __fadd_rn(__fmul_rn(v1, __fsub_rn(1.f, alpha)), __fmul_rn(v2, alpha));
        }
        a.out[v * a.n_out + k][col] = r;
      }
    }
    __syncthreads();                                 // before the next tile's levels
  }
}

struct PointArgs {
  int op;
  int64_t n_pix, t;
  const float* in0;
  const float* in1;
  const float* cos_t;
  const float* sin_t;
  const int32_t* flag;
  float p0;
  float* out0;
  float* out1;
};

__global__ void __launch_bounds__(kBlk) derive_pointwise_kernel(PointArgs a) {
#pragma clang fp contract(off)
  const int64_t total = a.n_pix * a.t;
  for (int64_t idx = (int64_t)blockIdx.x * kBlk + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * kBlk) {
    const int64_t p = idx / a.t;
    const int64_t step = idx - p * a.t;
    switch (a.op) {
      case S3_DP_UV_FROM_WSWD: {
        const float ws = a.in0[idx], wd = a.in1[idx] * 0.017453292519943295f;
        const float cs = a.cos_t[p], sn = a.sin_t[p];
        const float s = sinf(wd), c = cosf(wd);
        a.out0[idx] = cs * ws * s + sn * ws * c;
        a.out1[idx] = -sn * ws * s + cs * ws * c;
        break;
      }
      case S3_DP_WSWD_FROM_UV: {
        const float u = a.in0[idx], v = a.in1[idx];
        const float cs = a.cos_t[p], sn = a.sin_t[p];
        const float ur = cs * u - sn * v, vr = sn * u + cs * v;
        a.out0[idx] = hypotf(ur, vr);
        a.out1[idx] = fmodf(atan2f(ur, vr) * 57.29577951308232f + 360.f, 360.f);
        break;
      }
      case S3_DP_SURFACE_RH: {
        const float d = a.in0[idx], tc = a.in1[idx];
        const float wv = 6.1078f * expf(17.1f * d / (235.f + d));
        const float sat = 6.1078f * expf(17.1f * tc / (235.f + tc));
        a.out0[idx] = 100.f * wv / sat;
        break;
      }
      case S3_DP_RATIO_MASKED:
        a.out0[idx] = a.flag[step] ? NAN : __fdiv_rn(a.in0[idx], a.in1[idx]);
        break;
      case S3_DP_CLOUD_MASK:
        a.out0[idx] = a.flag[step] ? NAN : (a.in0[idx] < a.in1[idx] ? 1.f : 0.f);
        break;
      case S3_DP_RATIO_CLIP01: {
        // np.minimum / np.maximum keep a NaN; of two equal operands they return
        // the second, as the x86 min / max they run on do: -0 comes out as +0
        float r = __fdiv_rn(a.in0[idx], a.in1[idx]);
        r = (r < 1.f || r != r) ? r : 1.f;
        a.out0[idx] = (r > 0.f || r != r) ? r : 0.f;
        break;
      }
      case S3_DP_ADD: a.out0[idx] = __fadd_rn(a.in0[idx], a.in1[idx]); break;
      case S3_DP_SCALE: a.out0[idx] = __fmul_rn(a.in0[idx], a.p0); break;
      case S3_DP_OFFSET: a.out0[idx] = __fadd_rn(a.in0[idx], a.p0); break;
      case S3_DP_BCAST_PIXEL: a.out0[idx] = a.in0[p]; break;
      default: a.out0[idx] = a.in0[step]; break;     // S3_DP_BCAST_TIME
    }
  }
}

// x is (n_pix, t c): a thread owns one position j of the row (step j / c) and a
// share of the pixels; neighbouring threads read neighbouring addresses.  One
// integer OR per thread that found something.
__global__ void __launch_bounds__(kBlk)
time_flags_kernel(const float* __restrict__ x, int64_t n_pix, int64_t row, int c, int mode, float thr,
                  int32_t* __restrict__ flags) {
  const int64_t j = (int64_t)blockIdx.x * kBlk + threadIdx.x;
  if (j >= row) return;                              // (no barrier in this kernel)
  int hit = 0;
  for (int64_t p = blockIdx.y; p < n_pix; p += gridDim.y) {
    const float v = x[p * row + j];
    hit |= mode == S3_TF_NAN ? (v != v) : (v <= thr);
  }
  if (hit) atomicOr(&flags[j / c], 1);
}

struct StackArgs {
  const float* plane[S3_STACK_MAX_PLANES];
  int c;
  int64_t n_pix, t, shift;    // shift = roll mod t in [0, t)
  float* out;
};

// one thread per (pixel, step): C coalesced plane reads, one C-run written
__global__ void __launch_bounds__(kBlk) stack_features_kernel(StackArgs a) {
  const int64_t total = a.n_pix * a.t;
  for (int64_t idx = (int64_t)blockIdx.x * kBlk + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * kBlk) {
    const int64_t p = idx / a.t;
    int64_t j = idx - p * a.t - a.shift;
    if (j < 0) j += a.t;
    const int64_t src = p * a.t + j;
    float* cell = a.out + idx * a.c;
    for (int ch = 0; ch < a.c; ++ch) cell[ch] = a.plane[ch][src];
  }
}

// float -> unsigned key in the order of the floats (no NaN comes here)
__device__ __forceinline__ unsigned long long order_key(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? (uint32_t)~u : (u | 0x80000000u);
}

__device__ __forceinline__ unsigned long long wave_total(unsigned long long v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;                                          // valid on lane 0
}

// Interpolator._check_lev_array's figures (interpolation.py:176-237), a lane
// per column: the check is an option, off by default, and reads the array
// once.  A lane reads its L floats at a stride of 4 * L bytes, the access
// shape the head of this file says to avoid and level_interp_kernel stages
// away; it is kept here for an opt-in check only, and was not timed.
// Integer atomics only, one set per wave: sums, extrema as order keys (minima
// as the maximum of the inverted key, so that zeroed words are the start).
__global__ void __launch_bounds__(kBlk)
level_stats_kernel(const float* __restrict__ lev, int64_t P, int64_t t, int L, const float* __restrict__ topo,
                   int topo_per_step, float lo, float hi, unsigned long long* __restrict__ st) {
  unsigned long long n_nan = 0, n_min = 0, n_max = 0, n_all = 0;
  unsigned long long first_max = 0, first_min = 0, last_max = 0, last_min = 0;
  auto keep = [](unsigned long long& best, unsigned long long k) { best = k > best ? k : best; };
  for (int64_t col = (int64_t)blockIdx.x * kBlk + threadIdx.x; col < P; col += (int64_t)gridDim.x * kBlk) {
    const float* x = lev + col * L;
    const float tp = topo ? topo[topo_per_step ? col : col / t] : 0.f;
    float mn = INFINITY, mx = -INFINITY;
    int nans = 0;
    for (int i = 0; i < L; ++i) {
      const float v = topo ? __fsub_rn(x[i], tp) : x[i];
      if (v != v) { ++nans; continue; }
      mn = v < mn ? v : mn;
      mx = v > mx ? v : mx;
      if (i == 0) { keep(first_max, order_key(v)); keep(first_min, 0xFFFFFFFFull - order_key(v)); }
      if (i == L - 1) { keep(last_max, order_key(v)); keep(last_min, 0xFFFFFFFFull - order_key(v)); }
    }
    n_nan += nans;
    n_all += nans == L;
    // (np.min / np.max of a column with a NaN is NaN: it compares false)
    n_min += nans == 0 && lo < mn;
    n_max += nans == 0 && hi > mx;
  }
  n_nan = wave_total(n_nan); n_min = wave_total(n_min); n_max = wave_total(n_max); n_all = wave_total(n_all);
  for (int off = 32; off > 0; off >>= 1) {
    keep(first_max, __shfl_down(first_max, off, 64));
    keep(first_min, __shfl_down(first_min, off, 64));
    keep(last_max, __shfl_down(last_max, off, 64));
    keep(last_min, __shfl_down(last_min, off, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    if (first_max) atomicMax(&st[S3_LS_FIRST_MAX], first_max);
    if (first_min) atomicMax(&st[S3_LS_FIRST_MIN], first_min);
    if (last_max) atomicMax(&st[S3_LS_LAST_MAX], last_max);
    if (last_min) atomicMax(&st[S3_LS_LAST_MIN], last_min);
    if (n_nan) atomicAdd(&st[S3_LS_NAN], n_nan);
    if (n_min) atomicAdd(&st[S3_LS_BAD_MIN], n_min);
    if (n_max) atomicAdd(&st[S3_LS_BAD_MAX], n_max);
    if (n_all) atomicAdd(&st[S3_LS_ALL_NAN], n_all);
  }
}

}  // namespace

extern "C" int s3_level_stats(s3_ctx* ctx, const float* lev_ml, int64_t n_col, int64_t t, int l_ml, const float* topo,
                              int topo_per_step, float lo_target, float hi_target, uint64_t* stats) {
  if (!ctx) return S3_EINVAL;
  if (!lev_ml || !stats) S3_FAIL(ctx, S3_EINVAL, "level_stats: the levels and the output are needed");
  if (n_col < 1 || t < 1 || n_col % t || l_ml < 1)
    S3_FAIL(ctx, S3_EINVAL, "level_stats: empty extent, or columns that are no multiple of the steps");
  S3_HIP(ctx, hipMemsetAsync(stats, 0, S3_LS_WORDS * sizeof(uint64_t), ctx->stream));
  hipLaunchKernelGGL(level_stats_kernel, dim3(grid_for(n_col, ctx->num_cu)), dim3(kBlk), 0, ctx->stream, lev_ml,
                     n_col, t, l_ml, topo, topo_per_step != 0, lo_target, hi_target,
                     reinterpret_cast<unsigned long long*>(stats));
  S3_HIP(ctx, hipGetLastError());
  return S3_OK;
}

extern "C" int s3_level_interp(s3_ctx* ctx, int64_t n_col, int64_t t, int l_ml, int n_sl, int lev_source,
                               const float* lev_ml, const float* lev_vec_host, const float* topo,
                               int topo_per_step, const float* sl_level_host, int n_var,
                               const float* const* var_ml_host, const float* const* var_sl_host, int n_out,
                               const float* target_host, int method, float* const* out_host) {
  if (!ctx) return S3_EINVAL;
  if (n_col < 1 || t < 1 || n_col % t) S3_FAIL(ctx, S3_EINVAL, "level_interp: empty extent, or columns that are no multiple of the steps");
  if (l_ml < 0 || n_sl < 0 || l_ml + n_sl < 1 || l_ml + n_sl > kMaxLev)
    S3_FAIL(ctx, S3_EINVAL, "level_interp: 1 .. S3_LI_MAX_LEVELS (64) levels in all");
  if (n_sl > kMaxSl) S3_FAIL(ctx, S3_EINVAL, "level_interp: at most S3_LI_MAX_SINGLE (8) single-level planes");
  if (n_var < 1 || n_var > kMaxVar) S3_FAIL(ctx, S3_EINVAL, "level_interp: 1 .. S3_LI_MAX_VARS (8) variables");
  if (n_out < 1 || n_out > kMaxOut) S3_FAIL(ctx, S3_EINVAL, "level_interp: 1 .. S3_LI_MAX_TARGETS (16) target levels");
  if (method != S3_LI_LINEAR && method != S3_LI_LOG) S3_FAIL(ctx, S3_EINVAL, "level_interp: unknown method");
  if (lev_source != S3_LI_LEV_COLUMN && lev_source != S3_LI_LEV_VECTOR)
    S3_FAIL(ctx, S3_EINVAL, "level_interp: unknown level source");
  if (!target_host || !out_host || (n_sl && (!sl_level_host || !var_sl_host)) || (l_ml && !var_ml_host) ||
      (l_ml && lev_source == S3_LI_LEV_COLUMN && !lev_ml) || (l_ml && lev_source == S3_LI_LEV_VECTOR && !lev_vec_host))
    S3_FAIL(ctx, S3_EINVAL, "level_interp: targets, outputs, levels and variables are needed");
  LevelArgs a = {};
  a.P = n_col; a.t = t; a.L_ml = l_ml; a.n_sl = n_sl; a.n_var = n_var; a.n_out = n_out; a.method = method;
  a.lev_vector = lev_source == S3_LI_LEV_VECTOR;
  a.topo_per_step = topo_per_step != 0;
  a.divL = FastDiv((uint32_t)(l_ml > 0 ? l_ml : 1));
  a.lev_ml = lev_ml;
  a.topo = a.lev_vector ? nullptr : topo;
  uintptr_t align = a.lev_vector ? 0 : reinterpret_cast<uintptr_t>(lev_ml);
  for (int i = 0; i < l_ml && a.lev_vector; ++i) a.lev_vec[i] = lev_vec_host[i];
  for (int i = 0; i < n_sl; ++i) a.sl_level[i] = sl_level_host[i];
  for (int i = 0; i < n_out; ++i) a.target[i] = target_host[i];
  for (int v = 0; v < n_var; ++v) {
    if (l_ml) {
      if (!var_ml_host[v]) S3_FAIL(ctx, S3_EINVAL, "level_interp: a multi-level variable is missing");
      a.var_ml[v] = var_ml_host[v];
      align |= reinterpret_cast<uintptr_t>(var_ml_host[v]);
    }
    for (int s = 0; s < n_sl; ++s) {
      if (!var_sl_host[v * n_sl + s]) S3_FAIL(ctx, S3_EINVAL, "level_interp: a single-level plane is missing");
      a.var_sl[v * n_sl + s] = var_sl_host[v * n_sl + s];
    }
    for (int k = 0; k < n_out; ++k) {
      if (!out_host[v * n_out + k]) S3_FAIL(ctx, S3_EINVAL, "level_interp: an output plane is missing");
      a.out[v * n_out + k] = out_host[v * n_out + k];
    }
  }
  a.vec4 = (align & 15u) == 0;                       // (a wave's run starts 256 L bytes into the array)
  const int Ls = (l_ml + n_sl) | 1;
  const size_t per_wave = ((size_t)kWave * Ls + 3 * (size_t)kWave * n_out) * sizeof(float);
  int waves = kBlk / kWave;
  while (waves > 1 && per_wave * waves > ctx->lds_max) --waves;
  if (per_wave * waves > ctx->lds_max) S3_FAIL(ctx, S3_EINVAL, "level_interp: the column tile does not fit the LDS");
  const size_t lds_bytes = per_wave * waves;
  // (the largest request: 64 levels, 16 targets: 28 928 bytes per wave, 113 KiB for 4 waves)
  static S3DeviceOnce attr_set;
  if (int rc = s3_lds_optin(ctx, attr_set, level_interp_kernel, (int)ctx->lds_max)) return rc;
  const int64_t n_tiles = (n_col + kWave - 1) / kWave;
  const int grid = grid_for((n_tiles + waves - 1) / waves * kBlk, ctx->num_cu);
  hipLaunchKernelGGL(level_interp_kernel, dim3(grid), dim3(waves * kWave), lds_bytes, ctx->stream, a);
  S3_HIP(ctx, hipGetLastError());
  return S3_OK;
}

extern "C" int s3_derive_pointwise(s3_ctx* ctx, int op, int64_t n_pix, int64_t t, const float* in0,
                                   const float* in1, const float* cos_theta, const float* sin_theta,
                                   const int32_t* step_flag, float p0, float* out0, float* out1) {
  if (!ctx) return S3_EINVAL;
  if (op < S3_DP_UV_FROM_WSWD || op > S3_DP_BCAST_TIME) S3_FAIL(ctx, S3_EINVAL, "derive_pointwise: unknown op");
  if (n_pix < 1 || t < 1) S3_FAIL(ctx, S3_EINVAL, "derive_pointwise: empty extent");
  const bool two_in = op <= S3_DP_ADD, two_out = op <= S3_DP_WSWD_FROM_UV;
  if (!in0 || !out0 || (two_in && !in1) || (two_out && (!out1 || !cos_theta || !sin_theta)))
    S3_FAIL(ctx, S3_EINVAL, "derive_pointwise: an input, an output or the angle tables are missing");
  if ((op == S3_DP_RATIO_MASKED || op == S3_DP_CLOUD_MASK) && !step_flag)
    S3_FAIL(ctx, S3_EINVAL, "derive_pointwise: the step flags are missing");
  PointArgs a = {op, n_pix, t, in0, in1, cos_theta, sin_theta, step_flag, p0, out0, out1};
  hipLaunchKernelGGL(derive_pointwise_kernel, dim3(grid_for(n_pix * t, ctx->num_cu, 16)), dim3(kBlk), 0,
                     ctx->stream, a);
  S3_HIP(ctx, hipGetLastError());
  return S3_OK;
}

extern "C" int s3_time_flags(s3_ctx* ctx, int mode, const float* x, int64_t n_pix, int64_t t, int c,
                             float threshold, int32_t* flags) {
  if (!ctx) return S3_EINVAL;
  if (!x || !flags) S3_FAIL(ctx, S3_EINVAL, "time_flags: the data and the flags are needed");
  if (mode != S3_TF_LE && mode != S3_TF_NAN) S3_FAIL(ctx, S3_EINVAL, "time_flags: unknown mode");
  if (n_pix < 1 || t < 1 || c < 1) S3_FAIL(ctx, S3_EINVAL, "time_flags: empty extent");
  const int64_t row = t * c;
  const int64_t bx = (row + kBlk - 1) / kBlk;
  if (bx >= ((int64_t)1 << 31)) S3_FAIL(ctx, S3_EINVAL, "time_flags: 2^31 or more row blocks");
  // pixel shares: fill the grid_for budget, at most 65535 (gridDim.y), at most one per pixel
  int64_t by = ((int64_t)ctx->num_cu * 16 + bx - 1) / bx;
  if (by > n_pix) by = n_pix;
  if (by > 65535) by = 65535;
  if (by < 1) by = 1;
  S3_HIP(ctx, hipMemsetAsync(flags, 0, (size_t)t * sizeof(int32_t), ctx->stream));
  hipLaunchKernelGGL(time_flags_kernel, dim3((unsigned)bx, (unsigned)by), dim3(kBlk), 0, ctx->stream, x, n_pix,
                     row, c, mode, threshold, flags);
  S3_HIP(ctx, hipGetLastError());
  return S3_OK;
}

extern "C" int s3_stack_features(s3_ctx* ctx, const float* const* planes_host, int c, int64_t n_pix, int64_t t,
                                 int64_t roll, float* out) {
  if (!ctx) return S3_EINVAL;
  if (!planes_host || !out) S3_FAIL(ctx, S3_EINVAL, "stack_features: the planes and the output are needed");
  if (c < 1 || c > S3_STACK_MAX_PLANES) S3_FAIL(ctx, S3_EINVAL, "stack_features: 1 .. S3_STACK_MAX_PLANES (32) planes");
  if (n_pix < 1 || t < 1) S3_FAIL(ctx, S3_EINVAL, "stack_features: empty extent");
  StackArgs a = {};
  for (int ch = 0; ch < c; ++ch) {
    if (!planes_host[ch]) S3_FAIL(ctx, S3_EINVAL, "stack_features: a plane is missing");
    a.plane[ch] = planes_host[ch];
  }
  a.c = c; a.n_pix = n_pix; a.t = t; a.out = out;
  a.shift = ((roll % t) + t) % t;
  hipLaunchKernelGGL(stack_features_kernel, dim3(grid_for(n_pix * t, ctx->num_cu, 16)), dim3(kBlk), 0, ctx->stream, a);
  S3_HIP(ctx, hipGetLastError());
  return S3_OK;
}
