// Regridding the low-res member of a dual pair onto the coarsened hi-res grid:
// DualRasterizer.update_lr_data (sup3r/preprocessing/rasterizers/dual.py:
// 187-222), which hands the work to rex's Regridder — a BallTree over the
// source points in the haversine metric, the k = 4 nearest sources of every
// target, inverse-distance weights, a weighted sum of whole time rows.
//   s3_regrid_knn    the k nearest sources of every target, exactly, with the
//                    distances and the normalised weights
//   s3_regrid_apply  out[j, :] = sum_k w[j, k] src[idx[j, k], :] for up to
//                    eight variables per launch, with the NaN count of the QA
// k-NN: the sources are binned into a cell grid over their bounding box, as
// kernels_exo.hip bins its targets (box by integer-atomic order keys, count,
// scan, scatter), the grid itself is laid out by the host from a 64-byte
// read-back of the box.  A lane owns a target and searches square rings of
// cells outward from its own; it stops when its k-th best distance lies
// below a lower bound on everything outside the rectangle searched so far:
// the latitude difference to the rectangle's edges, and the distance to the
// meridians of its edges, asin(cos(lat_t) sin(dlon)).  The second needs all
// longitudes within 180 degrees of one another and is useless near a pole:
// otherwise the grid has ONE longitude cell (latitude bands).  Every
// candidate is measured with the full haversine in float64, so neither the
// date line nor a pole is a special case.  Candidates are ordered by
// (distance, source id): neither the order inside a cell nor the order of the
// cells can show.  Nothing is contracted (the Makefile compiles this file
// with -ffp-contract=off).
// Apply: a workgroup owns a run of consecutive targets — row-major, so
// neighbours share source rows, which then hit in L1 / L2 — and a slab of
// 1024 steps; the indices and weights of a target are wave-uniform (scalar
// loads), a lane owns four steps.  gfx950 takes a 16-byte global access at any
// 4-byte alignment, so rows of a T that is no multiple of 4 are read and
// written with 16-byte accesses too; only the last T_out % 4 steps of a row
// go one by one.  
#include "common.h"

namespace {

constexpr int kBlk = kBlock;
constexpr int kScanPer = 4;                           // cells per thread of the scan
constexpr int64_t kLimit = (int64_t)1 << 31;
constexpr int kMaxK = S3_REGRID_MAX_K;
constexpr int kMaxVar = 8;                            // variables of one apply launch
constexpr int kSlab = 4 * kBlk;                       // steps of a workgroup
constexpr double kDeg = 0.017453292519943295;         // numpy's deg2rad factor, pi / 180

// the head of `work`
struct RegridHead {
  uint32_t key[8];        // sources, then targets: max lat, max of inverted lat, max lon, max of inverted lon
  uint32_t bad;           // a coordinate that is not finite was seen
  uint32_t cursor;        // entries claimed by the scan's blocks so far
  uint32_t pad[6];
};
static_assert(sizeof(RegridHead) == 64, "RegridHead is the 64-byte head of the workspace");

// the cell grid over the sources' box, laid out by the host
struct RegridGrid {
  double lat0, lon0, inv_lat, inv_lon, side_lat, side_lon;   // degrees
  int32_t ny, nx;
};

// most cells of a grid: about two sources per cell
inline int64_t cell_cap(int64_t n) { return n / 2 + 1024 < ((int64_t)1 << 28) ? n / 2 + 1024 : (int64_t)1 << 28; }

// (the next five as in kernels_exo.hip)
// float -> unsigned key in the order of the floats (finite values only)
__host__ __device__ inline uint32_t order_key_bits(uint32_t u) { return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__host__ __device__ inline uint32_t key_bits(uint32_t k) { return (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k; }
__device__ __forceinline__ uint32_t order_key(float v) { return order_key_bits(__float_as_uint(v)); }
__device__ __forceinline__ bool finite_f(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t o = __shfl_down(v, off, 64);
    v = o > v ? o : v;
  }
  return v;                                          // valid on lane 0
}
// cell of coordinate x along an axis of n cells starting at x0: monotone in x, clamped
__device__ __forceinline__ int cell_of(double x, double x0, double inv_side, int n) {
  const double a = (x - x0) * inv_side;
  if (!(a >= 0.0)) return 0;
  if (a >= (double)(n - 1)) return n - 1;
  return (int)a;
}

// the boxes of the sources (key[0..4)) and of the targets (key[4..8))
__global__ void __launch_bounds__(kBlk)
regrid_box_kernel(const float2* __restrict__ src, int64_t N, const float2* __restrict__ tgt, int64_t M,
                  RegridHead* g) {
  for (int set = 0; set < 2; ++set) {
    const float2* p = set ? tgt : src;
    const int64_t n = set ? M : N;
    uint32_t k0 = 0, k1 = 0, k2 = 0, k3 = 0, bad = 0;
    for (int64_t j = (int64_t)blockIdx.x * kBlk + threadIdx.x; j < n; j += (int64_t)gridDim.x * kBlk) {
      const float2 q = p[j];
      if (!finite_f(q.x) || !finite_f(q.y)) { bad = 1; continue; }
      const uint32_t a = order_key(q.x), b = order_key(q.y);
      k0 = a > k0 ? a : k0;
      k1 = ~a > k1 ? ~a : k1;
      k2 = b > k2 ? b : k2;
      k3 = ~b > k3 ? ~b : k3;
    }
    k0 = wave_max(k0); k1 = wave_max(k1); k2 = wave_max(k2); k3 = wave_max(k3);
    bad = wave_max(bad);
    if ((threadIdx.x & 63) == 0) {
      if (k0) {                                      // (a key of a finite value is never 0)
        atomicMax(&g->key[4 * set + 0], k0);
        atomicMax(&g->key[4 * set + 1], k1);
        atomicMax(&g->key[4 * set + 2], k2);
        atomicMax(&g->key[4 * set + 3], k3);
      }
      if (bad) atomicMax(&g->bad, 1u);
    }
  }
}

__device__ __forceinline__ int source_cell(const RegridGrid& g, float2 p) {
  return cell_of(p.x, g.lat0, g.inv_lat, g.ny) * g.nx + cell_of(p.y, g.lon0, g.inv_lon, g.nx);
}

__global__ void __launch_bounds__(kBlk)
regrid_count_kernel(const float2* __restrict__ src, int64_t N, RegridGrid g, uint32_t* count) {
  for (int64_t i = (int64_t)blockIdx.x * kBlk + threadIdx.x; i < N; i += (int64_t)gridDim.x * kBlk)
    atomicAdd(&count[source_cell(g, src[i])], 1u);
}

// end[c] <- first entry of cell c.  A block scans its 1024 consecutive cells
// and claims their entries as one range with one atomic: ranges of different
// blocks lie in the order the blocks arrive, cells of a block in cell order.
__global__ void __launch_bounds__(kBlk)
regrid_scan_kernel(const uint32_t* __restrict__ count, int64_t n_cells, RegridHead* g, uint32_t* __restrict__ end) {
  __shared__ uint32_t part[kBlk];
  __shared__ uint32_t base;
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

// entries into cell order, with the cosine of the latitude every distance to
// the source needs; end[c] is left one past the cell's last entry
__global__ void __launch_bounds__(kBlk)
regrid_scatter_kernel(const float2* __restrict__ src, int64_t N, RegridGrid g, uint32_t* end,
                      float2* __restrict__ cell_ll, double* __restrict__ cell_cos, int32_t* __restrict__ cell_id) {
  for (int64_t i = (int64_t)blockIdx.x * kBlk + threadIdx.x; i < N; i += (int64_t)gridDim.x * kBlk) {
    const float2 p = src[i];
    const uint32_t at = atomicAdd(&end[source_cell(g, p)], 1u);
    if (at < (uint32_t)N) {                          // (always: the counts sum to N)
      cell_ll[at] = p;
      cell_cos[at] = cos((double)p.x * kDeg);
      cell_id[at] = (int32_t)i;
    }
  }
}

struct KnnArgs {
  const float2* tgt;
  int64_t M;
  RegridGrid g;
  const uint32_t* count;
  const uint32_t* end;
  const float2* cell_ll;
  const double* cell_cos;
  const int32_t* cell_id;
  int k;
  int32_t* idx;
  double* dist;
  float* w;
};

// the best list of a lane: kMaxK slots in (distance, id) order, h = the
// haversine term of each (the distance is 2 asin(sqrt(h)))
struct Best {
  double d[kMaxK], h[kMaxK];
  int32_t id[kMaxK];
};

__device__ __forceinline__ bool before(double d, int32_t id, double d2, int32_t id2) {
  return d < d2 || (d == d2 && id < id2);
}

// the sources of cell c against the target (la, lo radians, cos_t)
__device__ __forceinline__ void visit_cell(const KnnArgs& a, int c, double la, double lo, double cos_t, Best& b) {
  const int last = a.k - 1;
  const uint32_t e = a.end[c], first = e - a.count[c];
  for (uint32_t q = first; q < e; ++q) {
    const float2 s = a.cell_ll[q];
    const double s0 = sin(0.5 * (la - (double)s.x * kDeg)), s1 = sin(0.5 * (lo - (double)s.y * kDeg));
    double h = s0 * s0 + cos_t * a.cell_cos[q] * s1 * s1;
    h = h > 1.0 ? 1.0 : h;
    double dk = b.d[0], hk = b.h[0];
    int32_t idk = b.id[0];
#pragma unroll
    for (int i = 1; i < kMaxK; ++i)
      if (i == last) { dk = b.d[i]; hk = b.h[i]; idk = b.id[i]; }
    // sqrt and asin grow with h: a term above the k-th's by more than their
    // rounding cannot give a distance at or below the k-th's
    if (h > hk * (1.0 + 1.0 / 1073741824.0)) continue;
    const double d = 2.0 * asin(sqrt(h));
    const int32_t id = a.cell_id[q];
    if (!before(d, id, dk, idk)) continue;
#pragma unroll
    for (int i = kMaxK - 1; i >= 1; --i) {           // slot i - 1 is still the old one
      if (before(d, id, b.d[i - 1], b.id[i - 1])) {
        b.d[i] = b.d[i - 1]; b.h[i] = b.h[i - 1]; b.id[i] = b.id[i - 1];
      } else if (before(d, id, b.d[i], b.id[i])) {
        b.d[i] = d; b.h[i] = h; b.id[i] = id;
      }
    }
    if (before(d, id, b.d[0], b.id[0])) { b.d[0] = d; b.h[0] = h; b.id[0] = id; }
  }
}

__global__ void __launch_bounds__(kBlk) regrid_query_kernel(KnnArgs a) {
  const RegridGrid& g = a.g;
  const int nx = g.nx, ny = g.ny, k = a.k;
  for (int64_t j = (int64_t)blockIdx.x * kBlk + threadIdx.x; j < a.M; j += (int64_t)gridDim.x * kBlk) {
    const float2 p = a.tgt[j];
    const double lat = p.x, lon = p.y;
    const double la = lat * kDeg, lo = lon * kDeg, cos_t = cos(la);
    const int cy = cell_of(lat, g.lat0, g.inv_lat, ny), cx = cell_of(lon, g.lon0, g.inv_lon, nx);
    Best b;
#pragma unroll
    for (int i = 0; i < kMaxK; ++i) { b.d[i] = (double)INFINITY; b.h[i] = (double)INFINITY; b.id[i] = INT32_MAX; }
    const int up = ny - 1 - cy, right = nx - 1 - cx;
    int r_max = cy > up ? cy : up;
    r_max = cx > r_max ? cx : r_max;
    r_max = right > r_max ? right : r_max;
    for (int r = 0; r <= r_max; ++r) {
      const int ya = cy - r, yb = cy + r, xa = cx - r, xb = cx + r;
      const int x0 = xa > 0 ? xa : 0, x1 = xb < nx - 1 ? xb : nx - 1;
      const int y0 = ya > 0 ? ya : 0, y1 = yb < ny - 1 ? yb : ny - 1;
      if (ya >= 0)
        for (int x = x0; x <= x1; ++x) visit_cell(a, ya * nx + x, la, lo, cos_t, b);
      if (r > 0 && yb <= ny - 1)
        for (int x = x0; x <= x1; ++x) visit_cell(a, yb * nx + x, la, lo, cos_t, b);
      if (r > 0 && (xa >= 0 || xb <= nx - 1)) {
        const int ym0 = ya + 1 > 0 ? ya + 1 : 0, ym1 = yb - 1 < ny - 1 ? yb - 1 : ny - 1;
        for (int y = ym0; y <= ym1; ++y) {
          if (xa >= 0) visit_cell(a, y * nx + xa, la, lo, cos_t, b);
          if (xb <= nx - 1) visit_cell(a, y * nx + xb, la, lo, cos_t, b);
        }
      }
      if (r == r_max) break;
      double dk = b.d[0];
#pragma unroll
      for (int i = 1; i < kMaxK; ++i)
        if (i == k - 1) dk = b.d[i];
      if (!(dk < (double)INFINITY)) continue;
      // a lower bound on the distance to every source outside rows y0 .. y1,
      // columns x0 .. x1 (a side on the grid's border has nothing beyond it)
      double bound = (double)INFINITY;
      if (y0 > 0) {
        const double dl = lat - (g.lat0 + (double)y0 * g.side_lat);
        bound = fmin(bound, (dl > 0.0 ? dl : 0.0) * kDeg);
      }
      if (y1 < ny - 1) {
        const double dl = g.lat0 + (double)(y1 + 1) * g.side_lat - lat;
        bound = fmin(bound, (dl > 0.0 ? dl : 0.0) * kDeg);
      }
      if (x0 > 0) {
        double dl = lon - (g.lon0 + (double)x0 * g.side_lon);
        dl = dl > 0.0 ? (dl < 180.0 ? dl : 180.0) : 0.0;
        bound = fmin(bound, asin(fmin(1.0, cos_t * fabs(sin(dl * kDeg)))));
      }
      if (x1 < nx - 1) {
        double dl = g.lon0 + (double)(x1 + 1) * g.side_lon - lon;
        dl = dl > 0.0 ? (dl < 180.0 ? dl : 180.0) : 0.0;
        bound = fmin(bound, asin(fmin(1.0, cos_t * fabs(sin(dl * kDeg)))));
      }
      // the margin covers the rounding of cell_of against the edges (a few
      // 2^-53 of a coordinate) and of the distances (a few 2^-53 of each)
      if (dk < bound * (1.0 - 1.0 / 1048576.0) - 1e-12) break;
    }
    // rex: d float32, floored at 1e-12, w = 1 / d, w /= sum(w) (left to right)
    float wk[kMaxK], sum = 0.f;
#pragma unroll
    for (int i = 0; i < kMaxK; ++i) {
      if (i < k) {
        float d32 = __double2float_rn(b.d[i]);
        d32 = d32 < 1e-12f ? 1e-12f : d32;
        wk[i] = __fdiv_rn(1.0f, d32);
        sum = i ? __fadd_rn(sum, wk[i]) : wk[i];
      }
    }
#pragma unroll
    for (int i = 0; i < kMaxK; ++i) {
      if (i < k) {
        a.idx[j * k + i] = b.id[i];
        if (a.dist) a.dist[j * k + i] = b.d[i];
        a.w[j * k + i] = __fdiv_rn(wk[i], sum);
      }
    }
  }
}

// ---- apply --------------------------------------------------------------------
struct ApplyArgs {
  const float* src[kMaxVar];
  float* out[kMaxVar];
  const int32_t* idx;
  const float* w;
  unsigned long long* nan_count;
  int64_t n_tgt, T_src, T_out, n_slab;
  int run;                                           // targets of a workgroup
};

// 16 bytes at any 4-byte alignment
__device__ __forceinline__ float4 load4(const float* p) {
  float4 v;
  __builtin_memcpy(&v, p, sizeof(v));
  return v;
}
__device__ __forceinline__ void store4(float* p, float4 v) { __builtin_memcpy(p, &v, sizeof(v)); }

// one target's four steps (N = 4: 16-byte accesses) or the last N < 4 steps of
// its row; returns the NaNs written
template <int K, int N>
__device__ __forceinline__ uint32_t apply_steps(const float* __restrict__ src, float* __restrict__ dst,
                                                const int32_t* __restrict__ idx, const float* __restrict__ w,
                                                int64_t T_src, int64_t t0, int n) {
  int32_t id[K];
  double wq[K];
  float x[K][4];
#pragma unroll
  for (int q = 0; q < K; ++q) { id[q] = idx[q]; wq[q] = (double)w[q]; }
#pragma unroll
  for (int q = 0; q < K; ++q) {
    const float* row = src + (int64_t)id[q] * T_src + t0;
    if (N == 4) {
      const float4 f = load4(row);
      x[q][0] = f.x; x[q][1] = f.y; x[q][2] = f.z; x[q][3] = f.w;
    } else {
#pragma unroll
      for (int e = 0; e < 3; ++e) x[q][e] = e < n ? row[e] : 0.f;
      x[q][3] = 0.f;
    }
  }
  float y[4];
  uint32_t nans = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    double acc = __dmul_rn(wq[0], (double)x[0][e]);  // rank order; every product is exact
#pragma unroll
    for (int q = 1; q < K; ++q) acc = __dadd_rn(acc, __dmul_rn(wq[q], (double)x[q][e]));
    y[e] = __double2float_rn(acc);
    nans += (e < n && y[e] != y[e]) ? 1u : 0u;
  }
  if (N == 4) {
    store4(dst, make_float4(y[0], y[1], y[2], y[3]));
  } else {
#pragma unroll
    for (int e = 0; e < 3; ++e)
      if (e < n) dst[e] = y[e];
  }
  return nans;
}

// blockIdx.x = (run of targets, slab of steps), blockIdx.y = variable
template <int K>
__global__ void __launch_bounds__(kBlk) regrid_apply_kernel(ApplyArgs a) {
  __shared__ uint32_t wave_nans[kBlk / 64];
  const int v = blockIdx.y;
  const float* __restrict__ src = a.src[v];
  float* __restrict__ out = a.out[v];
  const int64_t slab = (int64_t)blockIdx.x % a.n_slab, run = (int64_t)blockIdx.x / a.n_slab;
  const int64_t t0 = slab * kSlab + 4 * (int64_t)threadIdx.x;
  const int64_t left = a.T_out - t0;
  const int64_t j0 = run * a.run, j1 = j0 + a.run < a.n_tgt ? j0 + a.run : a.n_tgt;
  uint32_t nans = 0;
  if (left >= 4) {
    for (int64_t j = j0; j < j1; ++j)                // workgroup-uniform
      nans += apply_steps<K, 4>(src, out + j * a.T_out + t0, a.idx + j * K, a.w + j * K, a.T_src, t0, 4);
  } else if (left > 0) {
    for (int64_t j = j0; j < j1; ++j)
      nans += apply_steps<K, 3>(src, out + j * a.T_out + t0, a.idx + j * K, a.w + j * K, a.T_src, t0, (int)left);
  }
  for (int off = 32; off > 0; off >>= 1) nans += __shfl_down(nans, off, 64);
  if ((threadIdx.x & 63) == 0) wave_nans[threadIdx.x >> 6] = nans;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long total = 0;
    for (int q = 0; q < kBlk / 64; ++q) total += wave_nans[q];
    if (total) atomicAdd(&a.nan_count[v], total);
  }
}

template <int K>
void launch_apply(s3_ctx* ctx, const ApplyArgs& a, int64_t blocks, int n_var) {
  hipLaunchKernelGGL(regrid_apply_kernel<K>, dim3((unsigned)blocks, (unsigned)n_var), dim3(kBlk), 0, ctx->stream, a);
}

inline int64_t round8(int64_t b) { return (b + 7) & ~(int64_t)7; }

}  // namespace

extern "C" int64_t s3_regrid_knn_work_bytes(int64_t n_src) {
  if (n_src < 1 || n_src >= kLimit) return -1;
  // head, count and end per cell, (lat, lon), cos(lat) and id per source
  return round8((int64_t)sizeof(RegridHead) + 8 * cell_cap(n_src) + 20 * n_src);
}

extern "C" int s3_regrid_knn(s3_ctx* ctx, const float* src, int64_t n_src, const float* tgt, int64_t n_tgt, int k,
                             void* work, int64_t work_bytes, int32_t* idx_out, double* dist_out, float* w_out) {
  if (!ctx) return S3_EINVAL;
  if (n_src < 1 || n_tgt < 1) S3_FAIL(ctx, S3_EINVAL, "s3_regrid_knn: n_src and n_tgt start at 1");
  if (n_src >= kLimit || n_tgt >= kLimit) S3_FAIL(ctx, S3_EINVAL, "s3_regrid_knn: 2^31 or more sources or targets");
  if (k < 1 || k > kMaxK) S3_FAIL(ctx, S3_EINVAL, "s3_regrid_knn: k outside 1 .. S3_REGRID_MAX_K (8)");
  if (n_src < k) S3_FAIL(ctx, S3_EINVAL, "s3_regrid_knn: fewer sources than k");
  if (!src || !tgt || !work || !idx_out || !w_out)
    S3_FAIL(ctx, S3_EINVAL, "s3_regrid_knn: sources, targets, work, idx_out and w_out are needed");
  if (work_bytes < s3_regrid_knn_work_bytes(n_src))
    S3_FAIL(ctx, S3_EINVAL, "s3_regrid_knn: work is smaller than s3_regrid_knn_work_bytes(n_src)");
  if (reinterpret_cast<uintptr_t>(work) & 7u) S3_FAIL(ctx, S3_EINVAL, "s3_regrid_knn: work must be 8-byte aligned");
  const int64_t cap = cell_cap(n_src);
  char* base = static_cast<char*>(work);
  RegridHead* head = reinterpret_cast<RegridHead*>(base);
  double* cell_cos = reinterpret_cast<double*>(base + sizeof(RegridHead));
  float2* cell_ll = reinterpret_cast<float2*>(cell_cos + n_src);
  uint32_t* count = reinterpret_cast<uint32_t*>(cell_ll + n_src);
  uint32_t* end = count + cap;
  int32_t* cell_id = reinterpret_cast<int32_t*>(end + cap);
  const float2* src2 = reinterpret_cast<const float2*>(src);
  const float2* tgt2 = reinterpret_cast<const float2*>(tgt);
  const int cu = ctx->num_cu;
  // the boxes, read back: the one pass ahead of the coordinate check
  S3_HIP(ctx, hipMemsetAsync(head, 0, sizeof(RegridHead), ctx->stream));
  hipLaunchKernelGGL(regrid_box_kernel, dim3(grid_for(n_src > n_tgt ? n_src : n_tgt, cu)), dim3(kBlk), 0,
                     ctx->stream, src2, n_src, tgt2, n_tgt, head);
  S3_HIP(ctx, hipGetLastError());
  RegridHead h;
  S3_HIP(ctx, hipMemcpyAsync(&h, head, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
  S3_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (h.bad || !h.key[0] || !h.key[4]) S3_FAIL(ctx, S3_EINVAL, "s3_regrid_knn: a coordinate that is not finite");
  auto value = [](uint32_t key) {
    const uint32_t bits = key_bits(key);
    float f;
    __builtin_memcpy(&f, &bits, sizeof(f));
    return (double)f;
  };
  double lo[2][2], hi[2][2];                         // [set][lat, lon]
  for (int s = 0; s < 2; ++s)
    for (int c = 0; c < 2; ++c) {
      hi[s][c] = value(h.key[4 * s + 2 * c]);
      lo[s][c] = value(~h.key[4 * s + 2 * c + 1]);
    }
  const double lon_span = (hi[0][1] > hi[1][1] ? hi[0][1] : hi[1][1]) - (lo[0][1] < lo[1][1] ? lo[0][1] : lo[1][1]);
  double lat_abs = 0.0;
  for (int s = 0; s < 2; ++s) {
    lat_abs = fabs(lo[s][0]) > lat_abs ? fabs(lo[s][0]) : lat_abs;
    lat_abs = fabs(hi[s][0]) > lat_abs ? fabs(hi[s][0]) : lat_abs;
  }
  const bool bands = lon_span > 180.0 || lat_abs > 85.0;
  // about two sources per cell, cells as square (in degrees) as the box allows
  RegridGrid g = {};
  g.lat0 = lo[0][0];
  g.lon0 = lo[0][1];
  const double hgt = hi[0][0] - lo[0][0], wid = bands ? 0.0 : hi[0][1] - lo[0][1];
  double want = (double)(n_src / 2 < 1 ? 1 : n_src / 2);
  want = want > (double)cap ? (double)cap : want;
  double ny = 1.0, nx = 1.0;
  if (hgt > 0.0 && wid > 0.0) {
    const double side = sqrt(hgt * wid / want);
    ny = floor(hgt / side) + 1.0;
    nx = floor(wid / side) + 1.0;
    ny = ny > want ? want : ny;
    nx = nx > want ? want : nx;
    while (ny * nx > (double)cap) { if (nx > ny) nx -= 1.0; else ny -= 1.0; }
  } else if (hgt > 0.0) {
    ny = want;
  } else if (wid > 0.0) {
    nx = want;
  }
  g.ny = (int32_t)ny;
  g.nx = (int32_t)nx;
  g.side_lat = g.ny > 1 ? hgt / ny : 0.0;
  g.side_lon = g.nx > 1 ? wid / nx : 0.0;
  g.inv_lat = g.ny > 1 ? ny / hgt : 0.0;
  g.inv_lon = g.nx > 1 ? nx / wid : 0.0;
  const int64_t n_cells = (int64_t)g.ny * g.nx;
  S3_HIP(ctx, hipMemsetAsync(count, 0, (size_t)n_cells * sizeof(uint32_t), ctx->stream));
  hipLaunchKernelGGL(regrid_count_kernel, dim3(grid_for(n_src, cu)), dim3(kBlk), 0, ctx->stream, src2, n_src, g, count);
  hipLaunchKernelGGL(regrid_scan_kernel, dim3(grid_for((n_cells + kScanPer - 1) / kScanPer, cu)), dim3(kBlk), 0,
                     ctx->stream, count, n_cells, head, end);
  hipLaunchKernelGGL(regrid_scatter_kernel, dim3(grid_for(n_src, cu)), dim3(kBlk), 0, ctx->stream, src2, n_src, g, end,
                     cell_ll, cell_cos, cell_id);
  KnnArgs a = {};
  a.tgt = tgt2; a.M = n_tgt; a.g = g; a.count = count; a.end = end;
  a.cell_ll = cell_ll; a.cell_cos = cell_cos; a.cell_id = cell_id;
  a.k = k; a.idx = idx_out; a.dist = dist_out; a.w = w_out;
  hipLaunchKernelGGL(regrid_query_kernel, dim3(grid_for(n_tgt, cu, 16)), dim3(kBlk), 0, ctx->stream, a);
  S3_HIP(ctx, hipGetLastError());
  return S3_OK;
}

extern "C" int s3_regrid_apply(s3_ctx* ctx, int n_var, const float* const* src_planes_host,
                               float* const* out_planes_host, int64_t n_src, int64_t n_tgt, int64_t T_src,
                               int64_t T_out, int k, const int32_t* idx, const float* w, int64_t* nan_count) {
  if (!ctx) return S3_EINVAL;
  if (n_var < 1) S3_FAIL(ctx, S3_EINVAL, "s3_regrid_apply: n_var starts at 1");
  if (k < 1 || k > kMaxK) S3_FAIL(ctx, S3_EINVAL, "s3_regrid_apply: k outside 1 .. S3_REGRID_MAX_K (8)");
  if (n_src < 1 || n_tgt < 1 || n_src >= kLimit || n_tgt >= kLimit)
    S3_FAIL(ctx, S3_EINVAL, "s3_regrid_apply: n_src and n_tgt are 1 .. 2^31 - 1");
  if (T_out < 1 || T_out > T_src) S3_FAIL(ctx, S3_EINVAL, "s3_regrid_apply: 1 <= T_out <= T_src is needed");
  if (!src_planes_host || !out_planes_host || !idx || !w || !nan_count)
    S3_FAIL(ctx, S3_EINVAL, "s3_regrid_apply: the plane tables, idx, w and nan_count are needed");
  for (int v = 0; v < n_var; ++v) {
    if (!src_planes_host[v] || !out_planes_host[v]) S3_FAIL(ctx, S3_EINVAL, "s3_regrid_apply: a plane is missing");
    if (((uintptr_t)src_planes_host[v] | (uintptr_t)out_planes_host[v]) & 3u)
      S3_FAIL(ctx, S3_EINVAL, "s3_regrid_apply: a misaligned plane");
  }
  if (T_src > INT64_MAX / n_src || T_out > INT64_MAX / n_tgt)
    S3_FAIL(ctx, S3_EINVAL, "s3_regrid_apply: a plane's size overflows");
  ApplyArgs a = {};
  a.idx = idx; a.w = w; a.n_tgt = n_tgt; a.T_src = T_src; a.T_out = T_out;
  a.n_slab = (T_out + kSlab - 1) / kSlab;
  a.run = 16;
  auto blocks = [&] { return (n_tgt + a.run - 1) / a.run * a.n_slab; };
  while (blocks() > INT32_MAX && a.run < (1 << 30)) a.run *= 2;
  if (blocks() > INT32_MAX) S3_FAIL(ctx, S3_EINVAL, "s3_regrid_apply: more than 2^31 - 1 workgroups");
  S3_HIP(ctx, hipMemsetAsync(nan_count, 0, (size_t)n_var * sizeof(int64_t), ctx->stream));
  for (int v0 = 0; v0 < n_var; v0 += kMaxVar) {
    const int n = n_var - v0 < kMaxVar ? n_var - v0 : kMaxVar;
    for (int v = 0; v < n; ++v) {
      a.src[v] = src_planes_host[v0 + v];
      a.out[v] = out_planes_host[v0 + v];
    }
    a.nan_count = reinterpret_cast<unsigned long long*>(nan_count) + v0;
    switch (k) {
      case 1: launch_apply<1>(ctx, a, blocks(), n); break;
      case 2: launch_apply<2>(ctx, a, blocks(), n); break;
      case 3: launch_apply<3>(ctx, a, blocks(), n); break;
      case 4: launch_apply<4>(ctx, a, blocks(), n); break;
      case 5: launch_apply<5>(ctx, a, blocks(), n); break;
      case 6: launch_apply<6>(ctx, a, blocks(), n); break;
      case 7: launch_apply<7>(ctx, a, blocks(), n); break;
      default: launch_apply<8>(ctx, a, blocks(), n); break;
    }
  }
  S3_HIP(ctx, hipGetLastError());
  return S3_OK;
}
