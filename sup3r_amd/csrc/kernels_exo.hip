// Rasterising exogenous fields on the device: the nearest-target query and the
// group mean of BaseExoRasterizer (sup3r/preprocessing/rasterizers/exo.py:
// 294-458: KDTree.query with a distance bound, then a pandas group mean).
//   s3_exo_nearest     nearest target of every source point under the bound r
//   s3_exo_group_mean  per target and column: mean of the non-NaN values mapped
//                      to it, times a scale factor
// Nearest: a uniform cell grid over the targets' bounding box, built here on
// every call (five small launches: box, grid, count, scan, scatter), cell side
// a little above r, so that every target within r of a source lies in the
// 3 x 3 cells around the source's own.  A lane owns a source; rasters arrive
// row-major, so the lanes of a wave walk the same few cells and their reads
// hit in L1 / L2.  Distances are float64 on the widened inputs, nothing
// contracted; ties go to the smallest target id, so the order inside a cell —
// and the order in which the scan's blocks claim their ranges — cannot show.
// Group mean: no float atomics.  A value becomes a 63-bit integer multiple of
// 2^(E - 61), E from a max-|x| pre-pass; its low 32 bits and the rest go to
// two 64-bit limbs per (target, column) with integer atomics, which hold 2^31
// terms without a carry; integer addition commutes, so the bits do not depend
// on arrival.  Lists are very uneven (an 'input' step collects 10^4 - 10^5
// sources per target, a 'layer' step tens): runs of lanes with one target are
// summed in the wave first, a long list then costs one atomic per wave and
// column instead of 64.  (DESIGN.md "Exogenous rasterisation")
#include "common.h"

namespace {

constexpr int kBlk = kBlock;
constexpr int kScanPer = 4;                           // cells per thread of the scan
constexpr int64_t kSlabBudget = (int64_t)256 << 20;   // bytes of limbs and counts per slab
constexpr int64_t kLimit = (int64_t)1 << 31;

// the head of `work` for s3_exo_nearest
struct ExoGrid {
  uint32_t key[4];        // order keys: max lat, max of inverted lat, max lon, max of inverted lon
  int32_t nx, ny;
  uint32_t cursor;        // entries claimed by the scan's blocks so far
  uint32_t pad;
  double lat0, lon0, inv_side;
  double spare;
};
static_assert(sizeof(ExoGrid) == 64, "ExoGrid is the 64-byte head of the workspace");

// most cells of a grid: 2 n_tgt + 1024, and a cell index stays an int
inline int64_t cell_cap(int64_t m) { return 2 * m + 1024 < ((int64_t)1 << 30) ? 2 * m + 1024 : (int64_t)1 << 30; }

// float -> unsigned key in the order of the floats (finite values only)
__device__ __forceinline__ uint32_t order_key(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_value(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}
__device__ __forceinline__ bool finite_f(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }

__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t o = __shfl_down(v, off, 64);
    v = o > v ? o : v;
  }
  return v;                                          // valid on lane 0
}

// cell of coordinate x along an axis of n cells starting at x0: monotone in x,
// clamped; NaN and -inf go to 0, +inf to n - 1
__device__ __forceinline__ int cell_of(double x, double x0, double inv_side, int n) {
  const double a = (x - x0) * inv_side;
  if (!(a >= 0.0)) return 0;
  if (a >= (double)(n - 1)) return n - 1;
  return (int)a;
}

__global__ void __launch_bounds__(kBlk) exo_box_kernel(const float2* __restrict__ tgt, int64_t M, ExoGrid* g) {
  uint32_t k0 = 0, k1 = 0, k2 = 0, k3 = 0;
  for (int64_t j = (int64_t)blockIdx.x * kBlk + threadIdx.x; j < M; j += (int64_t)gridDim.x * kBlk) {
    const float2 p = tgt[j];
    if (!finite_f(p.x) || !finite_f(p.y)) continue;
    const uint32_t a = order_key(p.x), b = order_key(p.y);
    k0 = a > k0 ? a : k0;
    k1 = ~a > k1 ? ~a : k1;
    k2 = b > k2 ? b : k2;
    k3 = ~b > k3 ? ~b : k3;
  }
  k0 = wave_max(k0); k1 = wave_max(k1); k2 = wave_max(k2); k3 = wave_max(k3);
  if ((threadIdx.x & 63) == 0 && k0) {               // (a key of a finite value is never 0)
    atomicMax(&g->key[0], k0);
    atomicMax(&g->key[1], k1);
    atomicMax(&g->key[2], k2);
    atomicMax(&g->key[3], k3);
  }
}

// one thread: the grid from the box.  side = r (1 + 2^-16): the margin covers
// the rounding of cell_of (an index below 2^27, its relative error a few
// 2^-53), so that |x_s - x_t| < r puts the two at most one cell apart.
__global__ void exo_grid_kernel(ExoGrid* g, double r, double cap) {
#pragma clang fp contract(off)
  if (g->key[0] == 0) {                              // no finite target
    g->nx = g->ny = 1;
    g->lat0 = g->lon0 = 0.0;
    g->inv_side = 0.0;
    return;
  }
  const double lat1 = key_value(g->key[0]), lat0 = key_value(~g->key[1]);
  const double lon1 = key_value(g->key[2]), lon0 = key_value(~g->key[3]);
  const double h = lat1 - lat0, w = lon1 - lon0;
  double side = r * (1.0 + 1.0 / 65536.0);
  auto cells = [&](double s) { return (floor(w / s) + 1.0) * (floor(h / s) + 1.0); };
  if (!(cells(side) <= cap)) {
    const double s1 = (w > h ? w : h) / cap, s2 = sqrt(w / cap * h);
    side = side > s1 ? side : s1;
    side = side > s2 ? side : s2;
    while (!(cells(side) <= cap)) side *= 1.0625;
  }
  const double inv = 1.0 / side;
  g->lat0 = lat0;
  g->lon0 = lon0;
  g->inv_side = inv;
  // the last cell is the one cell_of gives the far edge of the box
  int ny = (int)((lat1 - lat0) * inv) + 1, nx = (int)((lon1 - lon0) * inv) + 1;
  while ((double)nx * (double)ny > cap) { if (nx > ny) --nx; else --ny; }   // (cell_of clamps)
  g->nx = nx;
  g->ny = ny;
}

__device__ __forceinline__ int target_cell(const ExoGrid* g, float2 p) {
  return cell_of(p.x, g->lat0, g->inv_side, g->ny) * g->nx + cell_of(p.y, g->lon0, g->inv_side, g->nx);
}

__global__ void __launch_bounds__(kBlk)
exo_count_kernel(const float2* __restrict__ tgt, int64_t M, const ExoGrid* __restrict__ g, uint32_t* count) {
  for (int64_t j = (int64_t)blockIdx.x * kBlk + threadIdx.x; j < M; j += (int64_t)gridDim.x * kBlk) {
    const float2 p = tgt[j];
    if (finite_f(p.x) && finite_f(p.y)) atomicAdd(&count[target_cell(g, p)], 1u);
  }
}

// end[c] <- first entry of cell c.  A block scans its 1024 consecutive cells
// and claims their entries as one range with one atomic: ranges of different
// blocks lie in the order the blocks arrive, cells of a block in cell order.
__global__ void __launch_bounds__(kBlk)
exo_scan_kernel(const uint32_t* __restrict__ count, ExoGrid* g, uint32_t* __restrict__ end) {
  __shared__ uint32_t part[kBlk];
  __shared__ uint32_t base;
  const int64_t n_cells = (int64_t)g->nx * g->ny;
  const int64_t tiles = (n_cells + kBlk * kScanPer - 1) / (kBlk * kScanPer);
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {   // workgroup-uniform
    const int64_t c0 = (tile * kBlk + threadIdx.x) * kScanPer;
    uint32_t v[kScanPer], sum = 0;
    for (int q = 0; q < kScanPer; ++q) {
      v[q] = c0 + q < n_cells ? count[c0 + q] : 0u;
      sum += v[q];
    }
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int off = 1; off < kBlk; off <<= 1) {
      const uint32_t add = (int)threadIdx.x >= off ? part[threadIdx.x - off] : 0u;
      __syncthreads();
      part[threadIdx.x] += add;
      __syncthreads();
    }
    if (threadIdx.x == kBlk - 1) base = atomicAdd(&g->cursor, part[kBlk - 1]);
    __syncthreads();
    uint32_t at = base + part[threadIdx.x] - sum;
    for (int q = 0; q < kScanPer; ++q) {
      if (c0 + q < n_cells) end[c0 + q] = at;
      at += v[q];
    }
    __syncthreads();                                 // before part / base are written again
  }
}

// entries into cell order; end[c] is left one past the cell's last entry
__global__ void __launch_bounds__(kBlk)
exo_scatter_kernel(const float2* __restrict__ tgt, int64_t M, const ExoGrid* __restrict__ g, uint32_t* end,
                   float2* __restrict__ cell_ll, int32_t* __restrict__ cell_id) {
  for (int64_t j = (int64_t)blockIdx.x * kBlk + threadIdx.x; j < M; j += (int64_t)gridDim.x * kBlk) {
    const float2 p = tgt[j];
    if (!finite_f(p.x) || !finite_f(p.y)) continue;
    const uint32_t at = atomicAdd(&end[target_cell(g, p)], 1u);
    if (at < (uint32_t)M) {                          // (always: the counts sum to at most M)
      cell_ll[at] = p;
      cell_id[at] = (int32_t)j;
    }
  }
}

__global__ void __launch_bounds__(kBlk)
exo_query_kernel(const float2* __restrict__ src, int64_t N, int64_t M, const ExoGrid* __restrict__ g,
                 const uint32_t* __restrict__ count, const uint32_t* __restrict__ end,
                 const float2* __restrict__ cell_ll, const int32_t* __restrict__ cell_id, double r2,
                 int32_t* __restrict__ nn, double* __restrict__ dist) {
#pragma clang fp contract(off)
  const int nx = g->nx, ny = g->ny;
  const double lat0 = g->lat0, lon0 = g->lon0, inv = g->inv_side;
  for (int64_t i = (int64_t)blockIdx.x * kBlk + threadIdx.x; i < N; i += (int64_t)gridDim.x * kBlk) {
    const float2 p = src[i];
    const double la = p.x, lo = p.y;
    const int cy = cell_of(la, lat0, inv, ny), cx = cell_of(lo, lon0, inv, nx);
    const int y0 = cy > 0 ? cy - 1 : 0, y1 = cy < ny - 1 ? cy + 1 : ny - 1;
    const int x0 = cx > 0 ? cx - 1 : 0, x1 = cx < nx - 1 ? cx + 1 : nx - 1;
    int32_t best = -1;
    double best_d2 = 0.0;
    for (int y = y0; y <= y1; ++y) {
      for (int x = x0; x <= x1; ++x) {
        const int c = y * nx + x;
        const uint32_t e = end[c], b = e - count[c];
        for (uint32_t q = b; q < e; ++q) {
          const float2 t = cell_ll[q];
          const double dla = __dsub_rn(la, (double)t.x), dlo = __dsub_rn(lo, (double)t.y);
          const double d2 = __dadd_rn(__dmul_rn(dla, dla), __dmul_rn(dlo, dlo));
          if (!(d2 < r2)) continue;
          const int32_t id = cell_id[q];
          if (best < 0 || d2 < best_d2 || (d2 == best_d2 && id < best)) {
            best = id;
            best_d2 = d2;
          }
        }
      }
    }
    nn[i] = best < 0 ? (int32_t)M : best;
    if (dist) dist[i] = best < 0 ? (double)INFINITY : __dsqrt_rn(best_d2);
  }
}

// ---- group mean ---------------------------------------------------------------
__device__ __forceinline__ double exp2i(int e) {     // 2^e, -1022 <= e <= 1023
  return __longlong_as_double((long long)(e + 1023) << 52);
}
// E = floor(log2(v)) of the float with the bits u (positive, finite); 0 for 0
__device__ __forceinline__ int floor_log2_bits(uint32_t u) {
  if (u >> 23) return (int)(u >> 23) - 127;
  return u ? (31 - __clz((int)u)) - 149 : 0;
}

__global__ void __launch_bounds__(kBlk) exo_absmax_kernel(const float* __restrict__ val, int64_t n, uint32_t* word) {
  uint32_t mx = 0;
  for (int64_t i = (int64_t)blockIdx.x * kBlk + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlk) {
    const uint32_t u = __float_as_uint(val[i]) & 0x7FFFFFFFu;
    if (u < 0x7F800000u && u > mx) mx = u;           // finite; the bits of |x| order as |x|
  }
  mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0 && mx) atomicMax(word, mx);
}

struct MeanArgs {
  const int32_t* nn;
  const float* val;
  int64_t N, M, t_used, t_out;
  int k0, S;                                         // the slab: columns k0 .. k0 + S of val
  int col[S3_EXO_MAX_SLAB];                          // their columns of out
  double scale;
  const uint32_t* absmax;
  unsigned long long* lo;
  unsigned long long* hi;
  uint32_t* cnt;
  float* out;
  unsigned long long* nan_count;
};

// A lane owns a source; the loop bound is wave-uniform (whole waves take part
// in the shuffles; a lane past the end, a miss and an id outside [0, M) carry
// the id -1 and add nothing).
__global__ void __launch_bounds__(kBlk) exo_accumulate_kernel(MeanArgs a) {
  const int lane = threadIdx.x & 63;
  const double to_fixed = exp2i(61 - floor_log2_bits(*a.absmax));
  for (int64_t base = (int64_t)blockIdx.x * kBlk + (threadIdx.x - lane); base < a.N;
       base += (int64_t)gridDim.x * kBlk) {
    const int64_t i = base + lane;
    int32_t id = i < a.N ? a.nn[i] : -1;
    if ((uint32_t)id >= (uint32_t)a.M) id = -1;
    const int32_t prev = __shfl_up(id, 1, 64);
    const bool head = lane == 0 || prev != id;
    const unsigned long long heads = __ballot(head);
    const int run = __popcll(heads & ((2ull << lane) - 1ull));   // runs are consecutive lanes
    const float* row = a.val + i * a.t_used + a.k0;
    for (int k = 0; k < a.S; ++k) {
      const float x = id >= 0 ? row[k] : 0.f;
      const bool ok = id >= 0 && x == x;
      const long long v = ok ? __double2ll_rn((double)x * to_fixed) : 0ll;   // |v| <= 2^62
      unsigned long long lo = (unsigned long long)v & 0xFFFFFFFFull;
      long long hi = v >> 32;
      uint32_t n = ok;
      for (int off = 1; off < 64; off <<= 1) {
        const int r2 = __shfl_down(run, off, 64);
        const unsigned long long lo2 = __shfl_down(lo, off, 64);
        const long long hi2 = __shfl_down(hi, off, 64);
        const uint32_t n2 = __shfl_down(n, off, 64);
        if (lane + off < 64 && r2 == run) { lo += lo2; hi += hi2; n += n2; }
      }
      if (head && n) {
        const int64_t cell = (int64_t)id * a.S + k;
        atomicAdd(&a.lo[cell], lo);
        atomicAdd(&a.hi[cell], (unsigned long long)hi);
        atomicAdd(&a.cnt[cell], n);
      }
    }
  }
}

__global__ void __launch_bounds__(kBlk) exo_finalize_kernel(MeanArgs a) {
#pragma clang fp contract(off)
  const int E = floor_log2_bits(*a.absmax);
  const double unit = exp2i(E - 61);
  const int64_t total = a.M * a.S;
  unsigned long long nans = 0;
  for (int64_t idx = (int64_t)blockIdx.x * kBlk + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * kBlk) {
    const int64_t m = idx / a.S;
    const int k = (int)(idx - m * a.S);
    const uint32_t n = a.cnt[idx];
    float r;
    if (n == 0) {
      r = __uint_as_float(0x7FC00000u);
      ++nans;
    } else {
      // hi 2^32 + lo, exactly, then ONE rounding to float64 (nearest even: the
      // top 64 bits with everything below them ORed into the last)
      const __int128 tot = ((__int128)(long long)a.hi[idx] << 32) + (__int128)a.lo[idx];
      const bool neg = tot < 0;
      const unsigned __int128 mag = neg ? (unsigned __int128)(-tot) : (unsigned __int128)tot;
      const unsigned long long mh = (unsigned long long)(mag >> 64), ml = (unsigned long long)mag;
      double d;
      if (mh == 0) {
        d = __ull2double_rn(ml);
      } else {
        const int sh = 64 - __clzll((long long)mh);
        unsigned long long top = (unsigned long long)(mag >> sh);
        if (mag & ((((unsigned __int128)1) << sh) - 1)) top |= 1ull;
        d = __ull2double_rn(top) * exp2i(sh);
      }
      d = d * unit;                                  // a power of two: exact
      if (neg) d = -d;
      r = __double2float_rn(__dmul_rn(__ddiv_rn(d, (double)n), a.scale));
    }
    a.out[m * a.t_out + a.col[k]] = r;
  }
  for (int off = 32; off > 0; off >>= 1) nans += __shfl_down(nans, off, 64);
  if ((threadIdx.x & 63) == 0 && nans) atomicAdd(a.nan_count, nans);
}

inline int64_t round8(int64_t b) { return (b + 7) & ~(int64_t)7; }

inline int slab_columns(int64_t m, int64_t t_used) {
  int64_t s = kSlabBudget / (20 * m);
  if (s > S3_EXO_MAX_SLAB) s = S3_EXO_MAX_SLAB;
  if (s > t_used) s = t_used;
  return s < 1 ? 1 : (int)s;
}

}  // namespace

extern "C" int64_t s3_exo_nearest_work_bytes(int64_t n_tgt) {
  if (n_tgt < 1 || n_tgt >= kLimit) return -1;
  // head, count and end per cell, (lat, lon) and id per target
  return round8((int64_t)sizeof(ExoGrid) + 8 * cell_cap(n_tgt) + 12 * n_tgt);
}

extern "C" int s3_exo_nearest(s3_ctx* ctx, const float* src, int64_t n_src, const float* tgt, int64_t n_tgt, double r,
                              void* work, int64_t work_bytes, int32_t* nn, double* dist) {
  if (!ctx) return S3_EINVAL;
  if (n_src < 1 || n_tgt < 1) S3_FAIL(ctx, S3_EINVAL, "s3_exo_nearest: n_src and n_tgt start at 1");
  if (n_src >= kLimit || n_tgt >= kLimit) S3_FAIL(ctx, S3_EINVAL, "s3_exo_nearest: 2^31 or more sources or targets");
  if (!(r > 0.0) || !(r < (double)INFINITY)) S3_FAIL(ctx, S3_EINVAL, "s3_exo_nearest: r must be finite and above 0");
  if (!src || !tgt || !work || !nn) S3_FAIL(ctx, S3_EINVAL, "s3_exo_nearest: sources, targets, work and nn are needed");
  if (work_bytes < s3_exo_nearest_work_bytes(n_tgt))
    S3_FAIL(ctx, S3_EINVAL, "s3_exo_nearest: work is smaller than s3_exo_nearest_work_bytes(n_tgt)");
  if (reinterpret_cast<uintptr_t>(work) & 7u) S3_FAIL(ctx, S3_EINVAL, "s3_exo_nearest: work must be 8-byte aligned");
  const int64_t cap = cell_cap(n_tgt);
  char* base = static_cast<char*>(work);
  ExoGrid* g = reinterpret_cast<ExoGrid*>(base);
  float2* cell_ll = reinterpret_cast<float2*>(base + sizeof(ExoGrid));
  uint32_t* count = reinterpret_cast<uint32_t*>(cell_ll + n_tgt);
  uint32_t* end = count + cap;
  int32_t* cell_id = reinterpret_cast<int32_t*>(end + cap);
  const float2* tgt2 = reinterpret_cast<const float2*>(tgt);
  const int cu = ctx->num_cu;
  // head and counts to zero (the cells the grid does not use stay unread)
  S3_HIP(ctx, hipMemsetAsync(g, 0, sizeof(ExoGrid), ctx->stream));
  S3_HIP(ctx, hipMemsetAsync(count, 0, (size_t)cap * sizeof(uint32_t), ctx->stream));
  hipLaunchKernelGGL(exo_box_kernel, dim3(grid_for(n_tgt, cu)), dim3(kBlk), 0, ctx->stream, tgt2, n_tgt, g);
  hipLaunchKernelGGL(exo_grid_kernel, dim3(1), dim3(1), 0, ctx->stream, g, r, (double)cap);
  hipLaunchKernelGGL(exo_count_kernel, dim3(grid_for(n_tgt, cu)), dim3(kBlk), 0, ctx->stream, tgt2, n_tgt, g, count);
  hipLaunchKernelGGL(exo_scan_kernel, dim3(grid_for((cap + kScanPer - 1) / kScanPer, cu)), dim3(kBlk), 0, ctx->stream,
                     count, g, end);
  hipLaunchKernelGGL(exo_scatter_kernel, dim3(grid_for(n_tgt, cu)), dim3(kBlk), 0, ctx->stream, tgt2, n_tgt, g, end,
                     cell_ll, cell_id);
  hipLaunchKernelGGL(exo_query_kernel, dim3(grid_for(n_src, cu)), dim3(kBlk), 0, ctx->stream,
                     reinterpret_cast<const float2*>(src), n_src, n_tgt, g, count, end, cell_ll, cell_id, r * r, nn,
                     dist);
  S3_HIP(ctx, hipGetLastError());
  return S3_OK;
}

extern "C" int64_t s3_exo_group_mean_work_bytes(int64_t n_tgt, int64_t t_used) {
  if (n_tgt < 1 || n_tgt >= kLimit || t_used < 1) return -1;
  return round8(64 + 20 * n_tgt * slab_columns(n_tgt, t_used));
}

extern "C" int s3_exo_group_mean(s3_ctx* ctx, const int32_t* nn, const float* val, int64_t n_src, int64_t n_tgt,
                                 int64_t t_used, int64_t t_out, const int32_t* col_host, double scale, void* work,
                                 int64_t work_bytes, float* out, uint64_t* nan_count) {
  if (!ctx) return S3_EINVAL;
  if (n_src < 1 || n_tgt < 1) S3_FAIL(ctx, S3_EINVAL, "s3_exo_group_mean: n_src and n_tgt start at 1");
  if (n_src >= kLimit || n_tgt >= kLimit)
    S3_FAIL(ctx, S3_EINVAL, "s3_exo_group_mean: 2^31 or more sources or targets");
  if (t_used < 1 || t_out < 1 || t_used > t_out)
    S3_FAIL(ctx, S3_EINVAL, "s3_exo_group_mean: 1 <= t_used <= t_out is needed");
  if (!nn || !val || !col_host || !work || !out || !nan_count)
    S3_FAIL(ctx, S3_EINVAL, "s3_exo_group_mean: nn, values, column map, work, out and nan_count are needed");
  for (int64_t k = 0; k < t_used; ++k)
    if (col_host[k] < 0 || col_host[k] >= t_out)
      S3_FAIL(ctx, S3_EINVAL, "s3_exo_group_mean: a column map entry outside [0, t_out)");
  if (work_bytes < s3_exo_group_mean_work_bytes(n_tgt, t_used))
    S3_FAIL(ctx, S3_EINVAL, "s3_exo_group_mean: work is smaller than s3_exo_group_mean_work_bytes(n_tgt, t_used)");
  if (reinterpret_cast<uintptr_t>(work) & 7u)
    S3_FAIL(ctx, S3_EINVAL, "s3_exo_group_mean: work must be 8-byte aligned");
  const int S = slab_columns(n_tgt, t_used);
  char* base = static_cast<char*>(work);
  uint32_t* absmax = reinterpret_cast<uint32_t*>(base);
  MeanArgs a = {};
  a.nn = nn; a.val = val; a.N = n_src; a.M = n_tgt; a.t_used = t_used; a.t_out = t_out;
  a.scale = scale;
  a.absmax = absmax;
  a.lo = reinterpret_cast<unsigned long long*>(base + 64);
  a.hi = a.lo + n_tgt * S;
  a.cnt = reinterpret_cast<uint32_t*>(a.hi + n_tgt * S);
  a.out = out;
  a.nan_count = reinterpret_cast<unsigned long long*>(nan_count);
  const int cu = ctx->num_cu;
  S3_HIP(ctx, hipMemsetAsync(absmax, 0, 64, ctx->stream));
  S3_HIP(ctx, hipMemsetAsync(nan_count, 0, sizeof(uint64_t), ctx->stream));
  hipLaunchKernelGGL(exo_absmax_kernel, dim3(grid_for(n_src * t_used, cu)), dim3(kBlk), 0, ctx->stream, val,
                     n_src * t_used, absmax);
  for (int64_t k0 = 0; k0 < t_used; k0 += S) {
    a.k0 = (int)k0;
    a.S = (int)(t_used - k0 < S ? t_used - k0 : S);
    for (int k = 0; k < a.S; ++k) a.col[k] = col_host[k0 + k];
    // (a shorter last slab uses the front of the limbs, at its own stride)
    S3_HIP(ctx, hipMemsetAsync(a.lo, 0, (size_t)n_tgt * S * 20, ctx->stream));
    hipLaunchKernelGGL(exo_accumulate_kernel, dim3(grid_for(n_src, cu)), dim3(kBlk), 0, ctx->stream, a);
    hipLaunchKernelGGL(exo_finalize_kernel, dim3(grid_for(n_tgt * a.S, cu)), dim3(kBlk), 0, ctx->stream, a);
  }
  S3_HIP(ctx, hipGetLastError());
  return S3_OK;
}
