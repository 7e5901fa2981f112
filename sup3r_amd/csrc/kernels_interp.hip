// Non-neural downscalers on the device: the reference's
// LinearInterp and SurfaceSpatialMetModel (sup3r/models/linear.py,
// sup3r/models/surface.py), which it runs on the host with scipy's
// RegularGridInterpolator and PIL.Image.resize one 2-D slice at a time.
//
//   st_interp     trilinear interpolation with linear extrapolation of a
//                 channels-last 5-D batch (models/utilities.py:161-212).
//                 Bound by its output writes: the input is s^2 t times smaller
//                 and stays in L2; float4 stores along the contiguous
//                 (time, channel) row.
//   surface       Pillow's separable resize in mode 'F' (horizontal pass
//                 rounded to fp32, then the vertical pass; per-axis coefficient
//                 tables built by the host in float64 with Pillow's
//                 precompute_coeffs) fused with the per-feature physics of
//                 SurfaceSpatialMetModel.generate and its bias fix
//                 hr -= R(C(hr) - lr).  A tile is a whole number of s x s
//                 blocks; it keeps the horizontal-pass rows of every field it
//                 reads (low-res rows x high-res columns) in LDS and recomputes
//                 the high-res values from them, so the high-res field is
//                 written ONCE:
//                   pass 1: T / P / other channels -> block means -> bias
//                           planes C(hr) - lr (low-res sized)
//                   pass 2: RH channels, T_hr_final recomputed from T's bias
//                           plane -> RH's bias planes
//                   pass 0: every channel minus R(bias), plus noise -> output.
//                 Cross-tile dependencies go through kernel boundaries only; no
//                 atomics, so repeated calls are bit-identical.
#include "wave_prims.h"

#include <math.h>
#include <string.h>

namespace {

constexpr int kBlk = kBlock;   // grid_for counts workgroups of this size
constexpr int kMaxCh = 32;                  // channels of one surface call
constexpr int kMaxFields = 3 * kMaxCh + 1;  // planes a tile may stage
constexpr int kMaxTaps = 8;                 // upscaling: LANCZOS has 7
constexpr size_t kMaxLds = 63 * 1024;       // dynamic LDS of a tile (+ 1 KB static)

// ---- st_interp --------------------------------------------------------------
// axes: int32 i0 of the O1, O2, OT output indices, then their fp32 fractions
// (host float64, rounded once): value = a[i0] + f (a[i0 + 1] - a[i0]); f < 0 or
// > 1 extrapolates from the edge interval like RegularGridInterpolator with
// fill_value=None
struct AxisRefs {
  const int* i1; const int* i2; const int* it;
  const float* f1; const float* f2; const float* ft;
};

__device__ __forceinline__ float lerp_f(float a, float b, float f) { return a + f * (b - a); }

template <int V>
__global__ void __launch_bounds__(kBlk) st_interp_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                         int N, int S1, int S2, int T, int C, int O1, int O2,
                                                         int OT, AxisRefs ax) {
  const int R = OT * C, RV = R / V;
  const int64_t total = (int64_t)N * O1 * O2 * RV;
  const int64_t sa = (int64_t)S2 * T * C, sb = (int64_t)T * C;
  for (int64_t idx = (int64_t)blockIdx.x * kBlk + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * kBlk) {
    const int64_t cell = idx / RV;
    const int q = (int)(idx - cell * RV);
    const int b = (int)(cell % O2);
    const int64_t r = cell / O2;
    const int a = (int)(r % O1), n = (int)(r / O1);
    const int a0 = ax.i1[a], b0 = ax.i2[b];
    const float fa = ax.f1[a], fb = ax.f2[b];
    const float* p00 = x + ((int64_t)n * S1 + a0) * sa + (int64_t)b0 * sb;
    float v[V];
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const int k = q * V + e;
      const int tt = k / C, c = k - tt * C;
      const int t0 = ax.it[tt];
      const float ft = ax.ft[tt];
      const float* p = p00 + t0 * C + c;
      const float v00 = lerp_f(p[0], p[C], ft);
      const float v01 = lerp_f(p[sb], p[sb + C], ft);
      const float v10 = lerp_f(p[sa], p[sa + C], ft);
      const float v11 = lerp_f(p[sa + sb], p[sa + sb + C], ft);
      v[e] = lerp_f(lerp_f(v00, v01, fb), lerp_f(v10, v11, fb), fa);
    }
    if constexpr (V == 4) {
      *reinterpret_cast<float4*>(y + idx * 4) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
      y[idx] = v[0];
    }
  }
}

// ---- surface model ----------------------------------------------------------
// Pillow coefficient table of one axis (host-built, float64 -> fp32 weights):
// int lo[O], int cnt[O], float w[O][K]; output o = sum_{k < cnt[o]} w[o][k] *
// in[lo[o] + k]; lo and lo + cnt are non-decreasing in o (host-checked)
struct Tab {
  const int* lo; const int* cnt; const float* w;
};
__device__ __forceinline__ Tab tab_of(const void* base, int O) {
  const int* p = static_cast<const int*>(base);
  return Tab{p, p + O, reinterpret_cast<const float*>(p + 2 * O)};
}

struct SurfKinds {
  int k[kMaxCh];
};

struct SurfArgs {
  int N, H, W, C, s, K;   // low-res (N, H, W, C) -> high-res (N, H s, W s, C); K taps per table row
  int TBY, TBX;           // tile in s x s blocks
  int nrows;              // LDS rows per staged field
  int ncols;              // LDS low-res columns per staged row
  int nty, ntx;           // tiles per image
  int mode;               // 0 final output, 1 bias of T / P / other, 2 bias of RH
  int fix_bias;
  int nf;                 // staged fields
  int plane[kMaxFields];  // plane id of LDS slot f (planes: A[C] | B[C] | X[C] | topo)
  int kind[kMaxCh];       // S3_SURF_*
  int sA[kMaxCh], sB[kMaxCh], sAT[kMaxCh], sBT[kMaxCh], sXT[kMaxCh];  // LDS slots, -1 = not staged
  int sTopo;
  float lapse, wT, wZ;
  float noise[kMaxCh];    // uniform [0, noise) added to the channel; 0 = none
  uint32_t key0, key1, call;
};

// planes A (pre-field), X (the input channel) and topo from the channels-last
// low-res batch; float64 arithmetic rounded once, like the reference's float64
// topography terms followed by Image.fromarray's cast to mode 'F'
__global__ void surface_prep_kernel(const float* __restrict__ x, const float* __restrict__ topo_lr,
                                    float* __restrict__ planes, int N, int H, int W, int C, SurfKinds kinds,
                                    double lapse, double pdiv, double pexp) {
  const int64_t HW = (int64_t)H * W, NHW = (int64_t)N * HW, total = NHW * C;
  for (int64_t idx = (int64_t)blockIdx.x * kBlk + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * kBlk) {
    const int c = (int)(idx % C);
    const int64_t pos = idx / C;            // n * HW + r * W + q
    const float v = x[idx];
    const double z = topo_lr ? (double)topo_lr[pos % HW] : 0.0;
    double a = v;
    if (kinds.k[c] == S3_SURF_TEMP) a = (double)v + z * lapse;
    else if (kinds.k[c] == S3_SURF_PRES) a = (double)v + 101325.0 * (1.0 - pow(1.0 - z / pdiv, pexp));
    planes[(int64_t)c * NHW + pos] = (float)a;
    planes[(int64_t)(2 * C + c) * NHW + pos] = v;
    if (c == 0 && topo_lr) planes[(int64_t)(3 * C) * NHW + pos] = (float)z;
  }
}

// g(topo_hr) = 101325 (1 - (1 - z / div)^exp) once per call, float64 rounded once
__global__ void pres_hr_kernel(const float* __restrict__ topo_hr, float* __restrict__ g, int64_t n,
                               double pdiv, double pexp) {
  for (int64_t i = (int64_t)blockIdx.x * kBlk + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlk)
    g[i] = (float)(101325.0 * (1.0 - pow(1.0 - (double)topo_hr[i] / pdiv, pexp)));
}

__global__ void __launch_bounds__(kBlk) surface_tile_kernel(
    SurfArgs A, const float* __restrict__ x, float* __restrict__ planes, const void* __restrict__ tab_h,
    const void* __restrict__ tab_w, const float* __restrict__ topo_hr, const float* __restrict__ g_hr,
    float* __restrict__ y, float* __restrict__ pmin_part) {
  extern __shared__ float sm[];
  __shared__ float red[kBlk];
  const int Y = A.H * A.s, X = A.W * A.s, C = A.C, s = A.s;
  const Tab ty = tab_of(tab_h, Y), tx = tab_of(tab_w, X);
  const int tiles = A.nty * A.ntx;
  const int n = blockIdx.x / tiles, tr = blockIdx.x % tiles;
  const int by0 = (tr / A.ntx) * A.TBY, bx0 = (tr % A.ntx) * A.TBX;
  const int Y0 = by0 * s, X0 = bx0 * s;
  const int TBYv = min(A.TBY, A.H - by0), TBXv = min(A.TBX, A.W - bx0);
  const int TYv = TBYv * s, TXv = TBXv * s, TX = A.TBX * s;
  const int rlo = ty.lo[Y0];
  const int nr = ty.lo[Y0 + TYv - 1] + ty.cnt[Y0 + TYv - 1] - rlo;   // <= A.nrows (host)
  const int64_t HW = (int64_t)A.H * A.W, NHW = (int64_t)A.N * HW;
  // staged rows [nrows][TX][nfp]: the fields of one cell side by side, an odd
  // stride so that lanes of consecutive columns hit distinct banks
  const int nfp = A.nf | 1;
  float* Hs = sm;
  float* Lr = Hs + (size_t)nfp * A.nrows * TX;            // [nf][nrows][ncols]
  float* Hv = Lr + (size_t)A.nf * A.nrows * A.ncols;      // [TY][TX][C] (passes 1, 2)

  // the low-res patch the tile reads: rows [rlo, rlo + nr) x columns [qlo,
  // qlo + qn) of every staged field, independent loads
  const int qlo = tx.lo[X0];
  const int qn = tx.lo[X0 + TXv - 1] + tx.cnt[X0 + TXv - 1] - qlo;   // <= A.ncols (host)
  const int sitems = A.nf * nr * qn;
  for (int it = threadIdx.x; it < sitems; it += kBlk) {
    const int q = it % qn, rest = it / qn;
    const int rr = rest % nr, f = rest / nr;
    Lr[((size_t)f * A.nrows + rr) * A.ncols + q] =
        planes[(int64_t)A.plane[f] * NHW + n * HW + (int64_t)(rlo + rr) * A.W + qlo + q];
  }
  __syncthreads();

  // horizontal pass of every staged field: low-res rows [rlo, rlo + nr) x the
  // tile's high-res columns, rounded to fp32 like Pillow's intermediate image
  // (one (row, column) per item, every field: the index arithmetic and the
  // column's taps are shared by the nf fields)
  const int hitems = nr * TXv;
  for (int it = threadIdx.x; it < hitems; it += kBlk) {
    const int xc = it % TXv, rr = it / TXv;
    const int xo = X0 + xc, lo = tx.lo[xo] - qlo, cnt = tx.cnt[xo];
    float w[kMaxTaps];
#pragma unroll
    for (int j = 0; j < kMaxTaps; ++j) w[j] = j < cnt ? tx.w[(int64_t)xo * A.K + j] : 0.f;
    float* dst = Hs + ((size_t)rr * TX + xc) * nfp;
    for (int f = 0; f < A.nf; ++f) {
      const float* row = Lr + ((size_t)f * A.nrows + rr) * A.ncols + lo;
      float acc = 0.f;
#pragma unroll
      for (int j = 0; j < kMaxTaps; ++j)
        if (j < cnt) acc = fmaf(w[j], row[j], acc);
      dst[f] = acc;
    }
  }
  __syncthreads();

  // vertical pass: a thread owns one (column, channel) of the tile's rows
  // (consecutive threads = consecutive addresses of an output row)
  float pmin = INFINITY;
  const int ritems = TXv * C;
  const size_t rstep = (size_t)TX * nfp;
  for (int it = threadIdx.x; it < ritems; it += kBlk) {
    const int c = it % C, xc = it / C;
    const int kd = A.kind[c];
    if (A.mode == 1 && kd == S3_SURF_RH) continue;
    if (A.mode == 2 && kd != S3_SURF_RH) continue;
    const int xo = X0 + xc;
    const int sA = A.sA[c], sB = A.sB[c], sAT = A.sAT[c], sBT = A.sBT[c], sXT = A.sXT[c];
    const float noise = A.noise[c];
    for (int yc = 0; yc < TYv; ++yc) {
      const int yo = Y0 + yc;
      const int r0 = ty.lo[yo] - rlo, cnt = ty.cnt[yo];
      float wv[kMaxTaps];
#pragma unroll
      for (int i = 0; i < kMaxTaps; ++i) wv[i] = i < cnt ? ty.w[(int64_t)yo * A.K + i] : 0.f;
      const float* cell = Hs + ((size_t)r0 * TX + xc) * nfp;
      // vertical pass of staged field `slot` at (yo, xo)
      auto R = [&](int slot) {
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < kMaxTaps; ++i)
          if (i < cnt) acc = fmaf(wv[i], cell[i * rstep + slot], acc);
        return acc;
      };
      const int64_t hp = (int64_t)yo * X + xo;
      const float zt = topo_hr ? topo_hr[hp] : 0.f;
      float v;
      if (kd == S3_SURF_TEMP) {
        v = R(sA) - A.lapse * zt;
      } else if (kd == S3_SURF_PRES) {
        v = R(sA) - g_hr[hp];
      } else if (kd == S3_SURF_RH) {
        float tf = R(sAT) - A.lapse * zt;     // the paired temperature, bias-fixed
        if (A.fix_bias) tf -= R(sBT);
        const float dt = tf - R(sXT);
        const float dz = zt - R(A.sTopo);
        v = R(sA) + A.wT * dt + A.wZ * dz;
      } else {
        v = R(sA);
      }
      if (A.mode != 0) {
        Hv[((size_t)yc * TX + xc) * C + c] = v;
        continue;
      }
      if (A.fix_bias) v -= R(sB);
      if (kd == S3_SURF_PRES) pmin = fminf(pmin, v);
      const int64_t pix = ((int64_t)n * Y + yo) * X + xo;
      if (noise != 0.f) {
        uint32_t rnd[4];
        philox4((uint32_t)pix, (uint32_t)(pix >> 32), (uint32_t)c, A.call, A.key0, A.key1, rnd);
        v += (float)(rnd[0] >> 8) * (1.f / 16777216.f) * noise;
      }
      y[pix * C + c] = v;
    }
  }

  if (A.mode == 0) {
    if (pmin_part) {
      red[threadIdx.x] = pmin;
      __syncthreads();
      for (int h = kBlk / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] = fminf(red[threadIdx.x], red[threadIdx.x + h]);
        __syncthreads();
      }
      if (threadIdx.x == 0) pmin_part[blockIdx.x] = red[0];
    }
    return;
  }
  // block means of the tile's high-res values -> bias planes B = C(hr) - lr
  __syncthreads();
  const int mitems = TBYv * TBXv * C;
  const double inv = 1.0 / ((double)s * s);
  for (int it = threadIdx.x; it < mitems; it += kBlk) {
    const int c = it % C, rest = it / C;
    const int bx = rest % TBXv, by = rest / TBXv;
    if ((A.mode == 1) == (A.kind[c] == S3_SURF_RH)) continue;
    double sum = 0.0;
    for (int i = 0; i < s; ++i)
      for (int j = 0; j < s; ++j)
        sum += Hv[((size_t)(by * s + i) * TX + bx * s + j) * C + c];
    const int64_t lp = n * HW + (int64_t)(by0 + by) * A.W + bx0 + bx;
    planes[(int64_t)(C + c) * NHW + lp] = (float)(sum * inv) - x[lp * C + c];
  }
}

__global__ void min_reduce_kernel(const float* __restrict__ part, int n, float* __restrict__ out) {
  __shared__ float red[kBlk];
  float m = INFINITY;
  for (int i = threadIdx.x; i < n; i += kBlk) m = fminf(m, part[i]);
  red[threadIdx.x] = m;
  __syncthreads();
  for (int h = kBlk / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) red[threadIdx.x] = fminf(red[threadIdx.x], red[threadIdx.x + h]);
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = red[0];
}

// dynamic LDS bytes of a (TBY x TBX)-block tile staging nf fields
size_t tile_lds(int nf, int nrows, int ncols, int TBY, int TBX, int s, int C, bool means) {
  size_t b = ((size_t)(nf | 1) * nrows * TBX * s + (size_t)nf * nrows * ncols) * sizeof(float);
  if (means) b += (size_t)TBY * s * TBX * s * C * sizeof(float);
  return b;
}

// low-res rows the vertical pass of any TBY-block tile row reads
int tile_rows(const int* lo, const int* cnt, int H, int s, int TBY) {
  int m = 0;
  for (int b0 = 0; b0 < H; b0 += TBY) {
    const int y0 = b0 * s, y1 = (b0 + TBY < H ? b0 + TBY : H) * s - 1;
    const int r = lo[y1] + cnt[y1] - lo[y0];
    m = r > m ? r : m;
  }
  return m;
}

int surface_run(s3_ctx* ctx, const float* x, int n, int h, int w, int c, int s, const void* tab_h,
                const void* tab_w, const int* lo_h_host, const int* cnt_h_host, int k, const int* kinds,
                const int* pair, const float* consts, int fix_bias, const float* noise, uint64_t seed,
                uint32_t call, const float* topo_lr, const float* topo_hr, float* planes, float* g_hr, float* y,
                float* min_pres) {
  if (!x || !y || !planes || !tab_h || !tab_w || !lo_h_host || !cnt_h_host) return S3_EINVAL;
  if (n < 1 || h < 1 || w < 1 || c < 1 || s < 1) S3_FAIL(ctx, S3_EINVAL, "surface: empty shape");
  if (c > kMaxCh) S3_FAIL(ctx, S3_EINVAL, "surface: at most 32 channels");
  if (k < 1 || k > kMaxTaps) S3_FAIL(ctx, S3_EINVAL, "surface: 1 .. 8 taps per output (upscaling only)");
  if ((int64_t)h * s >= (1 << 24) || (int64_t)w * s >= (1 << 24))
    S3_FAIL(ctx, S3_EINVAL, "surface: image too large");
  bool any_rh = false, any_tp = false, any_pres = false, need_topo = false;
  for (int i = 0; i < c; ++i) {
    if (kinds[i] < S3_SURF_OTHER || kinds[i] > S3_SURF_RH) S3_FAIL(ctx, S3_EINVAL, "surface: bad channel kind");
    if (kinds[i] == S3_SURF_RH) {
      if (pair[i] < 0 || pair[i] >= c || kinds[pair[i]] != S3_SURF_TEMP)
        S3_FAIL(ctx, S3_EINVAL, "surface: a humidity channel needs a temperature channel");
      any_rh = true;
    } else {
      any_tp = true;
    }
    if (kinds[i] == S3_SURF_PRES) any_pres = true;
    if (kinds[i] != S3_SURF_OTHER) need_topo = true;
  }
  if (need_topo && (!topo_lr || !topo_hr)) S3_FAIL(ctx, S3_EINVAL, "surface: topography missing");
  if (any_pres && !g_hr) S3_FAIL(ctx, S3_EINVAL, "surface: pressure needs the g(topo_hr) buffer");

  SurfKinds kk;
  for (int i = 0; i < kMaxCh; ++i) kk.k[i] = i < c ? kinds[i] : S3_SURF_OTHER;
  const int64_t lr_total = (int64_t)n * h * w * c;
  hipLaunchKernelGGL(surface_prep_kernel, dim3(grid_for(lr_total, ctx->num_cu, 16)), dim3(kBlk), 0, ctx->stream,
                     x, need_topo ? topo_lr : nullptr, planes, n, h, w, c, kk, (double)consts[0],
                     (double)consts[3], (double)consts[4]);
  S3_HIP(ctx, hipGetLastError());
  const int64_t hr_pix = (int64_t)h * s * w * s;
  if (any_pres) {
    hipLaunchKernelGGL(pres_hr_kernel, dim3(grid_for(hr_pix, ctx->num_cu, 16)), dim3(kBlk), 0, ctx->stream,
                       topo_hr, g_hr, hr_pix, (double)consts[3], (double)consts[4]);
    S3_HIP(ctx, hipGetLastError());
  }

  // the passes: 1 and 2 only with the bias fix (2 only with humidity)
  int modes[3], nm = 0;
  if (fix_bias && any_tp) modes[nm++] = 1;
  if (fix_bias && any_rh) modes[nm++] = 2;
  modes[nm++] = 0;
  int nblocks_final = 0;
  float* part = nullptr;
  for (int mi = 0; mi < nm; ++mi) {
    const int mode = modes[mi];
    SurfArgs A;
    memset(&A, 0, sizeof A);
    A.N = n; A.H = h; A.W = w; A.C = c; A.s = s; A.K = k;
    A.mode = mode; A.fix_bias = fix_bias;
    A.lapse = consts[0]; A.wT = consts[1]; A.wZ = consts[2];
    A.key0 = (uint32_t)seed; A.key1 = (uint32_t)(seed >> 32); A.call = call;
    int slot_of[kMaxFields];
    for (int i = 0; i < kMaxFields; ++i) slot_of[i] = -1;
    auto stage = [&](int plane) {
      if (slot_of[plane] < 0) { slot_of[plane] = A.nf; A.plane[A.nf++] = plane; }
      return slot_of[plane];
    };
    A.sTopo = -1;
    for (int i = 0; i < c; ++i) {
      A.kind[i] = kinds[i];
      A.sA[i] = A.sB[i] = A.sAT[i] = A.sBT[i] = A.sXT[i] = -1;
      A.noise[i] = (mode == 0 && noise) ? noise[i] : 0.f;
      const bool rh = kinds[i] == S3_SURF_RH;
      if ((mode == 1 && rh) || (mode == 2 && !rh)) continue;
      A.sA[i] = stage(i);
      if (mode == 0 && fix_bias) A.sB[i] = stage(c + i);
      if (rh) {
        const int t = pair[i];
        A.sAT[i] = stage(t);
        if (fix_bias) A.sBT[i] = stage(c + t);
        A.sXT[i] = stage(2 * c + t);
        A.sTopo = stage(3 * c);
      }
    }
    // tile: whole s x s blocks, ~16 high-res rows x ~32 columns, halved while
    // the staged rows (+ the tile's values in the bias passes) exceed the LDS.
    // A tile's low-res columns span < TBX + k (the taps cover the support)
    int TBY = s >= 16 ? 1 : 16 / s, TBX = s >= 32 ? 1 : 32 / s;
    TBY = TBY > h ? h : TBY;
    TBX = TBX > w ? w : TBX;
    int nrows = tile_rows(lo_h_host, cnt_h_host, h, s, TBY);
    while (tile_lds(A.nf, nrows, TBX + k + 1, TBY, TBX, s, c, mode != 0) > kMaxLds && (TBY > 1 || TBX > 1)) {
      if (TBX >= TBY && TBX > 1) TBX = (TBX + 1) / 2; else TBY = (TBY + 1) / 2;
      nrows = tile_rows(lo_h_host, cnt_h_host, h, s, TBY);
    }
    const size_t lds = tile_lds(A.nf, nrows, TBX + k + 1, TBY, TBX, s, c, mode != 0);
    if (lds > kMaxLds) S3_FAIL(ctx, S3_EINVAL, "surface: one s x s block does not fit in LDS");
    A.TBY = TBY; A.TBX = TBX; A.nrows = nrows; A.ncols = TBX + k + 1;
    A.nty = (h + TBY - 1) / TBY; A.ntx = (w + TBX - 1) / TBX;
    const int64_t nblk = (int64_t)n * A.nty * A.ntx;
    if (nblk >= ((int64_t)1 << 31)) S3_FAIL(ctx, S3_EINVAL, "surface: too many tiles");
    if (mode == 0 && any_pres && min_pres) {
      int rc = ensure_scratch(ctx, (size_t)(nblk + 1) * sizeof(float));
      if (rc) return rc;
      part = ctx->scratch;
      nblocks_final = (int)nblk;
    }
    hipLaunchKernelGGL(surface_tile_kernel, dim3((unsigned)nblk), dim3(kBlk), lds, ctx->stream, A, x, planes,
                       tab_h, tab_w, need_topo ? topo_hr : nullptr, g_hr, y, part);
    S3_HIP(ctx, hipGetLastError());
  }
  if (min_pres) {
    if (!part) {
      *min_pres = INFINITY;
    } else {
      hipLaunchKernelGGL(min_reduce_kernel, dim3(1), dim3(kBlk), 0, ctx->stream, part, nblocks_final,
                         part + nblocks_final);
      S3_HIP(ctx, hipGetLastError());
      S3_HIP(ctx, hipMemcpyAsync(min_pres, part + nblocks_final, sizeof(float), hipMemcpyDeviceToHost,
                                 ctx->stream));
      S3_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
  }
  return S3_OK;
}

}  // namespace

extern "C" int s3_st_interp(s3_ctx* ctx, const float* x, int n, int s1, int s2, int t, int c, int s_enhance,
                            int t_enhance, const void* axes, float* y) {
  if (!ctx || !x || !y || !axes) return S3_EINVAL;
  if (n < 1 || s1 < 2 || s2 < 2 || t < 2 || c < 1 || s_enhance < 1 || t_enhance < 1)
    S3_FAIL(ctx, S3_EINVAL, "st_interp: every spatial and time axis needs length >= 2");
  const int O1 = s1 * s_enhance, O2 = s2 * s_enhance, OT = t * t_enhance;
  const int* ip = static_cast<const int*>(axes);
  const float* fp = reinterpret_cast<const float*>(ip + O1 + O2 + OT);
  AxisRefs ax{ip, ip + O1, ip + O1 + O2, fp, fp + O1, fp + O1 + O2};
  const int R = OT * c;
  const bool vec = R % 4 == 0 && (reinterpret_cast<uintptr_t>(y) & 15) == 0;
  const int64_t items = (int64_t)n * O1 * O2 * (vec ? R / 4 : R);
  if (vec)
    hipLaunchKernelGGL(st_interp_kernel<4>, dim3(grid_for(items, ctx->num_cu, 16)), dim3(kBlk), 0, ctx->stream, x, y,
                       n, s1, s2, t, c, O1, O2, OT, ax);
  else
    hipLaunchKernelGGL(st_interp_kernel<1>, dim3(grid_for(items, ctx->num_cu, 16)), dim3(kBlk), 0, ctx->stream, x, y,
                       n, s1, s2, t, c, O1, O2, OT, ax);
  S3_HIP(ctx, hipGetLastError());
  return S3_OK;
}

extern "C" int s3_resize2d(s3_ctx* ctx, const float* x, int n, int h, int w, int c, int s_enhance,
                           const void* tab_h, const void* tab_w, const int* lo_h_host, const int* cnt_h_host,
                           int k, float* planes, float* y) {
  if (!ctx) return S3_EINVAL;
  if (c > kMaxCh) S3_FAIL(ctx, S3_EINVAL, "resize2d: at most 32 channels per call");
  int kinds[kMaxCh], pair[kMaxCh];
  for (int i = 0; i < kMaxCh; ++i) { kinds[i] = S3_SURF_OTHER; pair[i] = -1; }
  const float consts[5] = {0.f, 0.f, 0.f, 1.f, 1.f};
  return surface_run(ctx, x, n, h, w, c, s_enhance, tab_h, tab_w, lo_h_host, cnt_h_host, k, kinds, pair, consts,
                     0, nullptr, 0, 0, nullptr, nullptr, planes, nullptr, y, nullptr);
}

extern "C" int s3_surface_downscale(s3_ctx* ctx, const float* x, int n, int h, int w, int c, int s_enhance,
                                    const void* tab_h, const void* tab_w, const int* lo_h_host,
                                    const int* cnt_h_host, int k, const int* kinds_host, const int* pair_host,
                                    const float* consts_host, int fix_bias, const float* noise_host,
                                    uint64_t seed, uint32_t call, const float* topo_lr, const float* topo_hr,
                                    float* planes, float* g_hr, float* y, float* min_pres_host) {
  if (!ctx || !kinds_host || !pair_host || !consts_host) return S3_EINVAL;
  return surface_run(ctx, x, n, h, w, c, s_enhance, tab_h, tab_w, lo_h_host, cnt_h_host, k, kinds_host,
                     pair_host, consts_host, fix_bias, noise_host, seed, call, topo_lr, topo_hr, planes, g_hr,
                     y, min_pres_host);
}
