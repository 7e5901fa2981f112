// The forward-pass chunk executor's I/O surface: channel copies and affine
// maps, chunk windows, the output epilogue (un-normalise, crop, statistics),
// the 2-D models' time-first / time-last transposes, the MultiStepGan step
// hand-over and the device -> host placement of finished chunks.
#include "kernels_support.h"
#include "wave_prims.h"

namespace {

__global__ void copy_channels_kernel(const float* __restrict__ src, int c_src,
                                     int c0_src, float* __restrict__ dst,
                                     int c_dst, int c0_dst, int nc,
                                     int64_t n_pos, int accumulate) {
  const int64_t total = n_pos * nc;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    int64_t p = i / nc;
    int c = (int)(i % nc);
    float v = src[p * c_src + c0_src + c];
    float* d = dst + p * c_dst + c0_dst + c;
    *d = accumulate ? *d + v : v;
  }
}

struct Affine8 { float scale[16]; float shift[16]; };
__global__ void affine_channels_kernel(const float* __restrict__ src,
                                       float* __restrict__ dst, int c,
                                       int64_t n, Affine8 a) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    int ch = (int)(i % c);
    // two roundings, as numpy's (x * scale) + shift: the empty asm keeps the
    // compiler from contracting the pair into one fma
    float t = src[i] * a.scale[ch];
    asm volatile("" : "+v"(t));
    dst[i] = t + a.shift[ch];
  }
}

// per-(chunk, slab) min / max / NaN count of every channel: the device half of
// ForwardPass._output_check (forward_pass.py:384-425)
constexpr int kStatSlabs = 64;
__global__ void chunk_stats_kernel(const float* __restrict__ x, int64_t pos_per_chunk,
                                   int c, float* __restrict__ partial) {
  const int chunk = blockIdx.y, slab = blockIdx.x;
  const float* xc = x + (int64_t)chunk * pos_per_chunk * c;
  __shared__ float smin[256], smax[256], snan[256];
  for (int ch = 0; ch < c; ++ch) {
    float mn = INFINITY, mx = -INFINITY, nn = 0.f;
    for (int64_t p = (int64_t)slab * blockDim.x + threadIdx.x; p < pos_per_chunk;
         p += (int64_t)kStatSlabs * blockDim.x) {
      const float v = xc[p * c + ch];
      if (v != v) nn += 1.f;
      else { mn = fminf(mn, v); mx = fmaxf(mx, v); }
    }
    smin[threadIdx.x] = mn; smax[threadIdx.x] = mx; snan[threadIdx.x] = nn;
    __syncthreads();
    for (int s = blockDim.x / 2; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) {
        smin[threadIdx.x] = fminf(smin[threadIdx.x], smin[threadIdx.x + s]);
        smax[threadIdx.x] = fmaxf(smax[threadIdx.x], smax[threadIdx.x + s]);
        snan[threadIdx.x] += snan[threadIdx.x + s];
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      float* o = partial + (((int64_t)chunk * kStatSlabs + slab) * c + ch) * 3;
      o[0] = smin[0]; o[1] = smax[0]; o[2] = snan[0];
    }
    __syncthreads();
  }
}

// The same statistics at memory speed for dense, 16-byte aligned chunks with
// 1024 % c == 0 (c = 1, 2, 4, 8, 16: every real output feature count): the
// chunk is walked as float4 with four loads in flight per lane; component k of
// float4 number q = slab * 256 + tid + j * (64 * 256) is channel (4 tid + k) % c
// for every j, so the running triples sit in fixed registers.  (The plain
// kernel above reads the chunk once PER CHANNEL with a stride of c floats:
// 423 us for the 368 MB of a C3 batch of 16; this one 70 - 90 us.)
__global__ __launch_bounds__(256) void chunk_stats4_kernel(const float* __restrict__ x, int64_t n4_per_chunk,
                                                           int c, float* __restrict__ partial) {
  const int chunk = blockIdx.y, slab = blockIdx.x, tid = threadIdx.x;
  const float4* xc = reinterpret_cast<const float4*>(x) + (int64_t)chunk * n4_per_chunk;
  float mn[4], mx[4], nn[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) { mn[k] = INFINITY; mx[k] = -INFINITY; nn[k] = 0.f; }
  auto fold = [&](const float4& v4) {
    const float v[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (v[k] != v[k]) nn[k] += 1.f;
      else { mn[k] = fminf(mn[k], v[k]); mx[k] = fmaxf(mx[k], v[k]); }
    }
  };
  const int64_t step = (int64_t)kStatSlabs * 256;
  int64_t q = (int64_t)slab * 256 + tid;
  for (; q + 3 * step < n4_per_chunk; q += 4 * step) {
    const float4 a = xc[q], b = xc[q + step], d = xc[q + 2 * step], e = xc[q + 3 * step];
    fold(a); fold(b); fold(d); fold(e);
  }
  for (; q < n4_per_chunk; q += step) fold(xc[q]);
  __shared__ float smin[256], smax[256], snan[256];
  for (int ch = 0; ch < c; ++ch) {
    float m0 = INFINITY, m1 = -INFINITY, m2 = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if ((4 * tid + k) % c == ch) { m0 = fminf(m0, mn[k]); m1 = fmaxf(m1, mx[k]); m2 += nn[k]; }
    smin[tid] = m0; smax[tid] = m1; snan[tid] = m2;
    __syncthreads();
    for (int s_ = 128; s_ > 0; s_ >>= 1) {
      if (tid < s_) {
        smin[tid] = fminf(smin[tid], smin[tid + s_]);
        smax[tid] = fmaxf(smax[tid], smax[tid + s_]);
        snan[tid] += snan[tid + s_];
      }
      __syncthreads();
    }
    if (tid == 0) {
      float* o = partial + (((int64_t)chunk * kStatSlabs + slab) * c + ch) * 3;
      o[0] = smin[0]; o[1] = smax[0]; o[2] = snan[0];
    }
    __syncthreads();
  }
}

// ---- the chunk executor's output epilogue in ONE pass over the hi-res batch:
// un-normalisation (s3_affine_channels' two roundings), halo crop
// (chunk.hr_crop_slice) and the output check's statistics (chunk_stats_kernel's
// partial[chunk][64][c][3]; min / max / NaN count do not depend on the order
// they are folded in).  Separately these were an in-place pass over the
// un-cropped 483 MB, eight block copies and a re-read of the 368 MB result per
// batch of eight C3 chunks (0.86 ms); fused, the cropped window is read once
// and written once.  Workgroup (slab, chunk) walks the cropped rows slab,
// slab + 64, ...; a row is c3 * c contiguous floats moved as float4.  With
// 1024 % c == 0 (c = 1, 2, 4, 8, ...) the channel of component k of thread t is
// (4 t + k) % c for every row and every stride of 256 float4, so the running
// min / max / NaN count live in four fixed register triples per thread.
struct ChunkEpi {
  int64_t y_chunk, y_s0, y_s1;     // element strides of the un-cropped batch
  int64_t y_org;                   // element offset of the crop origin in a chunk
  int c0, c1;                      // cropped rows: c0 x c1
  int row4;                        // float4 per cropped row (c2 * c / 4)
  int c;
  int affine;
  float scale[16], shift[16];
};
__global__ __launch_bounds__(256) void chunk_epilogue_kernel(const float* __restrict__ y,
                                                             float* __restrict__ yc,
                                                             float* __restrict__ partial, ChunkEpi e) {
  const int chunk = blockIdx.y, slab = blockIdx.x, tid = threadIdx.x;
  const float* yb = y + (int64_t)chunk * e.y_chunk + e.y_org;
  float* ob = yc + (int64_t)chunk * e.c0 * e.c1 * e.row4 * 4;
  float mn[4], mx[4], nn[4], sc[4], sh[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int ch = (4 * tid + k) % e.c;
    mn[k] = INFINITY; mx[k] = -INFINITY; nn[k] = 0.f;
    sc[k] = e.scale[ch]; sh[k] = e.shift[ch];
  }
  const int rows = e.c0 * e.c1;
  for (int r = slab; r < rows; r += kStatSlabs) {
    const int a = r / e.c1, b = r - a * e.c1;
    const float4* src = reinterpret_cast<const float4*>(yb + a * e.y_s0 + b * e.y_s1);
    float4* dst = reinterpret_cast<float4*>(ob + (int64_t)r * e.row4 * 4);
    for (int q = tid; q < e.row4; q += 256) {
      const float4 v4 = src[q];
      float v[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (e.affine) {
          float t = v[k] * sc[k];
          asm volatile("" : "+v"(t));          // (x * scale) + shift, two roundings
          v[k] = t + sh[k];
        }
        if (v[k] != v[k]) nn[k] += 1.f;
        else { mn[k] = fminf(mn[k], v[k]); mx[k] = fmaxf(mx[k], v[k]); }
      }
      dst[q] = make_float4(v[0], v[1], v[2], v[3]);
    }
  }
  __shared__ float smin[256], smax[256], snan[256];
  for (int ch = 0; ch < e.c; ++ch) {
    float m0 = INFINITY, m1 = -INFINITY, m2 = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if ((4 * tid + k) % e.c == ch) { m0 = fminf(m0, mn[k]); m1 = fmaxf(m1, mx[k]); m2 += nn[k]; }
    smin[tid] = m0; smax[tid] = m1; snan[tid] = m2;
    __syncthreads();
    for (int s_ = 128; s_ > 0; s_ >>= 1) {
      if (tid < s_) {
        smin[tid] = fminf(smin[tid], smin[tid + s_]);
        smax[tid] = fmaxf(smax[tid], smax[tid + s_]);
        snan[tid] += snan[tid + s_];
      }
      __syncthreads();
    }
    if (tid == 0) {
      float* o = partial + (((int64_t)chunk * kStatSlabs + slab) * e.c + ch) * 3;
      o[0] = smin[0]; o[1] = smax[0]; o[2] = snan[0];
    }
    __syncthreads();
  }
}

}  // namespace

extern "C" int s3_copy_channels(s3_ctx* ctx, const float* src, int c_src,
                                int c0_src, float* dst, int c_dst, int c0_dst,
                                int nc, int64_t n_pos, int accumulate) {
  if (!ctx) return S3_EINVAL;
  hipLaunchKernelGGL(copy_channels_kernel, dim3(grid_for(n_pos * nc, ctx->num_cu)), dim3(kBlock), 0, ctx->stream, src, c_src, c0_src, dst, c_dst, c0_dst, nc, n_pos, accumulate);
  S3_HIP(ctx, hipGetLastError());
  return S3_OK;
}

extern "C" int s3_affine_channels(s3_ctx* ctx, const float* src, float* dst,
                                  int c, int64_t n_pos, const float* scale_host,
                                  const float* shift_host) {
  if (!ctx) return S3_EINVAL;
  if (c > 16) S3_FAIL(ctx, S3_EINVAL, "affine_channels supports at most 16 channels");
  Affine8 a;
  for (int i = 0; i < c; ++i) { a.scale[i] = scale_host[i]; a.shift[i] = shift_host[i]; }
  int64_t n = n_pos * c;
  hipLaunchKernelGGL(affine_channels_kernel, dim3(grid_for(n, ctx->num_cu)), dim3(kBlock), 0, ctx->stream, src, dst, c, n, a);
  S3_HIP(ctx, hipGetLastError());
  return S3_OK;
}

// strided (d0, d1, row) block copy, fp32, device -> device: the chunk windows
// cut out of the resident lo-res domain and the halo crop of the hi-res output
__global__ void copy_block_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                  int64_t d1, int64_t row, int64_t ss0, int64_t ss1,
                                  int64_t ds0, int64_t ds1, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i % row, q = i / row;
    const int64_t b = q % d1, a = q / d1;
    dst[a * ds0 + b * ds1 + r] = src[a * ss0 + b * ss1 + r];
  }
}

extern "C" int s3_copy_block(s3_ctx* ctx, const float* src, float* dst, int64_t d0, int64_t d1,
                             int64_t row_elems, int64_t src_stride0, int64_t src_stride1,
                             int64_t dst_stride0, int64_t dst_stride1) {
  if (!ctx || !src || !dst) return S3_EINVAL;
  if (d0 < 1 || d1 < 1 || row_elems < 1) S3_FAIL(ctx, S3_EINVAL, "copy_block: empty block");
  const int64_t total = d0 * d1 * row_elems;
  hipLaunchKernelGGL(copy_block_kernel, dim3(grid_for(total, ctx->num_cu)), dim3(kBlock), 0, ctx->stream,
                     src, dst, d1, row_elems, src_stride0, src_stride1, dst_stride0, dst_stride1, total);
  S3_HIP(ctx, hipGetLastError());
  return S3_OK;
}

// 2-D (spatial) models see a chunk's time steps as their batch axis: the
// generated batch is (n_chunks * T, H, W, c); the chunk the executor delivers is
// hi_res[0][hr_crop_slices] of its transpose to (H, W, T, c)
// (sup3r/pipeline/forward_pass.py:274-337,272) — un-normalised on the way
struct ChunkTL { int64_t T, H, W; int64_t lo[3], n[3]; int c, affine; float scale[16], shift[16]; };
__global__ void chunk_time_last_kernel(const float* __restrict__ y, float* __restrict__ yc, ChunkTL e) {
  const int64_t per = e.n[0] * e.n[1] * e.n[2] * e.c;
  const int k = blockIdx.y;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < per;
       i += (int64_t)gridDim.x * blockDim.x) {
    int64_t r = i;
    const int ch = (int)(r % e.c); r /= e.c;
    const int64_t t = r % e.n[2]; r /= e.n[2];
    const int64_t w = r % e.n[1]; r /= e.n[1];
    const int64_t h = r;
    float v = y[((((int64_t)k * e.T + e.lo[2] + t) * e.H + e.lo[0] + h) * e.W + e.lo[1] + w) * e.c + ch];
    if (e.affine) {
      // two roundings, as numpy's (x * scale) + shift (affine_channels_kernel)
      float m = v * e.scale[ch];
      asm volatile("" : "+v"(m));
      v = m + e.shift[ch];
    }
    yc[(int64_t)k * per + i] = v;
  }
}

// ... and the way in: n chunks (s1, s2, t, c) -> the (n t, s1, s2, c) batch of a
// 2-D model, normalised (x - mean) / std with numpy's arithmetic: in fp32 when
// the statistics are fp32 arrays, in fp64 (then rounded to fp32) when they are
// fp64 — the two cases of Sup3rGan.norm_input (abstract.py:197-238)
struct ChunkTF { int64_t H, W, T; int c, mode; float mean[16], sd[16]; double dmean[16], dsd[16]; };
__global__ void chunk_time_first_kernel(const float* __restrict__ x, float* __restrict__ out, ChunkTF e) {
  const int64_t per = e.H * e.W * e.T * e.c;
  const int k = blockIdx.y;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < per;
       i += (int64_t)gridDim.x * blockDim.x) {
    // i runs over the OUTPUT (t, h, w, ch) of chunk k
    int64_t r = i;
    const int ch = (int)(r % e.c); r /= e.c;
    const int64_t w = r % e.W; r /= e.W;
    const int64_t h = r % e.H; r /= e.H;
    const int64_t t = r;
    float v = x[(int64_t)k * per + ((h * e.W + w) * e.T + t) * e.c + ch];
    if (e.mode == 1) {
      float d = v - e.mean[ch];
      asm volatile("" : "+v"(d));
      v = __fdiv_rn(d, e.sd[ch]);
    } else if (e.mode == 2) {
      v = (float)(((double)v - e.dmean[ch]) / e.dsd[ch]);
    }
    out[(int64_t)k * per + i] = v;
  }
}

extern "C" int s3_chunk_time_first(s3_ctx* ctx, const float* x, int n_chunks, const int64_t* hwt, int c,
                                   const double* mean_host, const double* std_host, int stats_fp32,
                                   float* out) {
  if (!ctx || !x || !out || !hwt) return S3_EINVAL;
  if (n_chunks < 1 || c < 1 || c > 16) S3_FAIL(ctx, S3_EINVAL, "chunk_time_first: 1 .. 16 channels");
  ChunkTF e;
  e.H = hwt[0]; e.W = hwt[1]; e.T = hwt[2]; e.c = c;
  e.mode = (mean_host && std_host) ? (stats_fp32 ? 1 : 2) : 0;
  for (int i = 0; i < 16; ++i) {
    const double m = e.mode && i < c ? mean_host[i] : 0.0, sd = e.mode && i < c ? std_host[i] : 1.0;
    e.mean[i] = (float)m; e.sd[i] = (float)sd; e.dmean[i] = m; e.dsd[i] = sd;
  }
  const int64_t per = e.H * e.W * e.T * c;
  hipLaunchKernelGGL(chunk_time_first_kernel, dim3(grid_for(per, ctx->num_cu), n_chunks), dim3(kBlock), 0,
                     ctx->stream, x, out, e);
  S3_HIP(ctx, hipGetLastError());
  return S3_OK;
}

extern "C" int s3_chunk_time_last(s3_ctx* ctx, const float* y, int n_chunks, const int64_t* thw,
                                  const int64_t* crop_lo, const int64_t* crop_n, int c,
                                  const float* scale_host, const float* shift_host, float* yc) {
  if (!ctx || !y || !yc || !thw || !crop_lo || !crop_n) return S3_EINVAL;
  if (n_chunks < 1 || c < 1 || c > 16) S3_FAIL(ctx, S3_EINVAL, "chunk_time_last: 1 .. 16 channels");
  // crop axes are (H, W, T): the chunk's (s1, s2, t)
  const int64_t ext[3] = {thw[1], thw[2], thw[0]};
  for (int d = 0; d < 3; ++d)
    if (crop_lo[d] < 0 || crop_n[d] < 1 || crop_lo[d] + crop_n[d] > ext[d])
      S3_FAIL(ctx, S3_EINVAL, "chunk_time_last: the crop window leaves the chunk");
  ChunkTL e;
  e.T = thw[0]; e.H = thw[1]; e.W = thw[2];
  for (int d = 0; d < 3; ++d) { e.lo[d] = crop_lo[d]; e.n[d] = crop_n[d]; }
  e.c = c;
  e.affine = scale_host && shift_host;
  for (int i = 0; i < 16; ++i) {
    e.scale[i] = e.affine && i < c ? scale_host[i] : 1.f;
    e.shift[i] = e.affine && i < c ? shift_host[i] : 0.f;
  }
  const int64_t per = crop_n[0] * crop_n[1] * crop_n[2] * c;
  int gx = grid_for(per, ctx->num_cu);
  hipLaunchKernelGGL(chunk_time_last_kernel, dim3(gx, n_chunks), dim3(kBlock), 0, ctx->stream, y, yc, e);
  S3_HIP(ctx, hipGetLastError());
  return S3_OK;
}

// dst[o][a][r][b] = src[o][a][b], r < reps: a time-invariant exo field
// (topography) uploaded once per chunk and laid over the chunk's time steps —
// (n, H W c) -> (n reps, H W c) for a 2-D model (a = 1), (n, H W, c) ->
// (n, H W, reps, c) for a 3-D one (ForwardPass.pad_source_data,
// sup3r/pipeline/forward_pass.py:160-186, does this with np.repeat on the host)
__global__ void broadcast_axis_kernel(const float* __restrict__ src, float* __restrict__ dst, int64_t oa,
                                      int64_t reps, int64_t b) {
  const int64_t total = oa * reps * b;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t bi = i % b;
    const int64_t q = i / (b * reps);
    dst[i] = src[q * b + bi];
  }
}

extern "C" int s3_broadcast_axis(s3_ctx* ctx, const float* src, int64_t outer, int64_t a, int64_t b, int64_t reps,
                                 float* dst) {
  if (!ctx || !src || !dst) return S3_EINVAL;
  if (outer < 1 || a < 1 || b < 1 || reps < 1) S3_FAIL(ctx, S3_EINVAL, "broadcast_axis: empty extent");
  hipLaunchKernelGGL(broadcast_axis_kernel, dim3(grid_for(outer * a * reps * b, ctx->num_cu)), dim3(kBlock), 0,
                     ctx->stream, src, dst, outer * a, reps, b);
  S3_HIP(ctx, hipGetLastError());
  return S3_OK;
}

// One model step's output -> the next step's input of a MultiStepGan chain
// (sup3r/models/multi_step.py:233-259), position by position:
// un_norm_output of step i (y * std + mean, abstract.py:240-275),
// _match_model_input's channel selection (multi_step.py:148-194), the 'input'
// exo channels _combine_fwp_input appends (interface.py:259-356), norm_input
// of step i + 1 ((x - mean) / std, abstract.py:197-238) — numpy's fp32
// arithmetic: one rounding per operation, no fused multiply-add.
struct StepHO { int c_src, c_sel, n_exo, un, nrm; int map[16]; float scale[16], shift[16], mean[16], sd[16]; };
__global__ void step_handover_kernel(const float* __restrict__ y, const float* __restrict__ exo,
                                     float* __restrict__ x, int64_t n_pos, StepHO e) {
  const int c_dst = e.c_sel + e.n_exo;
  const int64_t total = n_pos * c_dst;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = i / c_dst;
    const int ch = (int)(i - p * c_dst);
    float v;
    if (ch < e.c_sel) {
      const int sc = e.map[ch];
      v = y[p * e.c_src + sc];
      if (e.un) {
        float m = v * e.scale[sc];
        asm volatile("" : "+v"(m));
        v = m + e.shift[sc];
      }
    } else {
      v = exo[p * e.n_exo + (ch - e.c_sel)];
    }
    if (e.nrm) {
      float d = v - e.mean[ch];
      asm volatile("" : "+v"(d));
      v = __fdiv_rn(d, e.sd[ch]);
    }
    x[i] = v;
  }
}

extern "C" int s3_step_handover(s3_ctx* ctx, const float* y, int64_t n_pos, int c_src, const int* map_host,
                                int c_sel, const float* scale_host, const float* shift_host, const float* exo,
                                int n_exo, const float* mean_host, const float* std_host, float* x) {
  if (!ctx || !y || !x || !map_host) return S3_EINVAL;
  if (n_pos < 1 || c_src < 1 || c_src > 16 || c_sel < 1 || n_exo < 0 || c_sel + n_exo > 16)
    S3_FAIL(ctx, S3_EINVAL, "step_handover: 1 .. 16 channels on either side");
  if (n_exo > 0 && !exo) S3_FAIL(ctx, S3_EINVAL, "step_handover: exo channels without an exo tensor");
  StepHO e;
  e.c_src = c_src; e.c_sel = c_sel; e.n_exo = n_exo;
  e.un = scale_host && shift_host;
  e.nrm = mean_host && std_host;
  for (int i = 0; i < 16; ++i) {
    e.map[i] = 0;
    if (i < c_sel) {
      if (map_host[i] < 0 || map_host[i] >= c_src) S3_FAIL(ctx, S3_EINVAL, "step_handover: channel map out of range");
      e.map[i] = map_host[i];
    }
    e.scale[i] = e.un && i < c_src ? scale_host[i] : 1.f;
    e.shift[i] = e.un && i < c_src ? shift_host[i] : 0.f;
    e.mean[i] = e.nrm && i < c_sel + n_exo ? mean_host[i] : 0.f;
    e.sd[i] = e.nrm && i < c_sel + n_exo ? std_host[i] : 1.f;
  }
  hipLaunchKernelGGL(step_handover_kernel, dim3(grid_for(n_pos * (c_sel + n_exo), ctx->num_cu)), dim3(kBlock), 0,
                     ctx->stream, y, exo, x, n_pos, e);
  S3_HIP(ctx, hipGetLastError());
  return S3_OK;
}

extern "C" int s3_chunk_stats(s3_ctx* ctx, const float* x, int n_chunks,
                              int64_t pos_per_chunk, int c, float* partial) {
  if (!ctx) return S3_EINVAL;
  if (n_chunks < 1 || c < 1) S3_FAIL(ctx, S3_EINVAL, "chunk_stats: empty input");
  const int64_t per = pos_per_chunk * c;
  if (c <= 16 && 1024 % c == 0 && per % 4 == 0 && !((uintptr_t)x & 15))
    hipLaunchKernelGGL(chunk_stats4_kernel, dim3(kStatSlabs, n_chunks), dim3(256), 0, ctx->stream, x, per / 4, c,
                       partial);
  else
    hipLaunchKernelGGL(chunk_stats_kernel, dim3(kStatSlabs, n_chunks), dim3(256), 0,
                       ctx->stream, x, pos_per_chunk, c, partial);
  S3_HIP(ctx, hipGetLastError());
  return S3_OK;
}

extern "C" int s3_chunk_epilogue(s3_ctx* ctx, const float* y, int n_chunks, const int64_t* dims,
                                 const int64_t* crop_lo, const int64_t* crop_n, int c,
                                 const float* scale_host, const float* shift_host, float* yc,
                                 float* partial) {
  if (!ctx || !y || !yc || !partial || !dims || !crop_lo || !crop_n) return S3_EINVAL;
  if (n_chunks < 1 || c < 1 || c > 16 || 1024 % c != 0)
    S3_FAIL(ctx, S3_EINVAL, "chunk_epilogue: 1 .. 16 channels, a divisor of 1024");
  for (int d = 0; d < 3; ++d)
    if (crop_lo[d] < 0 || crop_n[d] < 1 || crop_lo[d] + crop_n[d] > dims[d])
      S3_FAIL(ctx, S3_EINVAL, "chunk_epilogue: the crop window leaves the chunk");
  // float4 rows: 16-byte aligned row starts and lengths (else the caller takes
  // the three-kernel path)
  if ((crop_n[2] * c) % 4 || (crop_lo[2] * c) % 4 || (dims[2] * c) % 4 || ((uintptr_t)y & 15) ||
      ((uintptr_t)yc & 15))
    S3_FAIL(ctx, S3_EINVAL, "chunk_epilogue: rows are not 16-byte aligned");
  ChunkEpi e;
  e.y_s1 = dims[2] * c;
  e.y_s0 = dims[1] * e.y_s1;
  e.y_chunk = dims[0] * e.y_s0;
  e.y_org = crop_lo[0] * e.y_s0 + crop_lo[1] * e.y_s1 + crop_lo[2] * c;
  e.c0 = (int)crop_n[0]; e.c1 = (int)crop_n[1];
  e.row4 = (int)(crop_n[2] * c / 4);
  e.c = c;
  e.affine = scale_host && shift_host;
  for (int i = 0; i < 16; ++i) {
    e.scale[i] = e.affine && i < c ? scale_host[i] : 1.f;
    e.shift[i] = e.affine && i < c ? shift_host[i] : 0.f;
  }
  hipLaunchKernelGGL(chunk_epilogue_kernel, dim3(kStatSlabs, n_chunks), dim3(256), 0, ctx->stream, y, yc,
                     partial, e);
  S3_HIP(ctx, hipGetLastError());
  return S3_OK;
}

// ---- direct device -> host placement of a cropped chunk -------------------
extern "C" int s3_host_register(s3_ctx* ctx, void* ptr, size_t bytes) {
  if (!ctx || !ptr) return S3_EINVAL;
  S3_HIP(ctx, hipHostRegister(ptr, bytes, hipHostRegisterDefault));
  return S3_OK;
}

extern "C" int s3_host_unregister(s3_ctx* ctx, void* ptr) {
  if (!ctx || !ptr) return S3_EINVAL;
  S3_HIP(ctx, hipHostUnregister(ptr));
  return S3_OK;
}

extern "C" int s3_d2h_window(s3_ctx* ctx, const float* src, float* dst_host, int64_t d0,
                             int64_t d1, int64_t row_elems, int64_t dst_stride0,
                             int64_t dst_stride1, void* stream) {
  if (!ctx || !src || !dst_host) return S3_EINVAL;
  if (d0 < 1 || d1 < 1 || row_elems < 1 || dst_stride1 < row_elems ||
      dst_stride0 % dst_stride1 != 0 || dst_stride0 / dst_stride1 < d1)
    S3_FAIL(ctx, S3_EINVAL, "d2h_window: the destination is not a pitched (d0, d1, row) window");
  hipMemcpy3DParms p = {};
  const size_t row_bytes = (size_t)row_elems * sizeof(float);
  p.srcPtr = make_hipPitchedPtr(const_cast<float*>(src), row_bytes, row_bytes, (size_t)d1);
  p.dstPtr = make_hipPitchedPtr(dst_host, (size_t)dst_stride1 * sizeof(float), row_bytes,
                                (size_t)(dst_stride0 / dst_stride1));
  p.extent = make_hipExtent(row_bytes, (size_t)d1, (size_t)d0);
  p.kind = hipMemcpyDeviceToHost;
  S3_HIP(ctx, hipMemcpy3DAsync(&p, stream ? (hipStream_t)stream : ctx->stream));
  return S3_OK;
}

// ---- throttled device -> pinned-host stream (the C3 executor's hi-res chunks)
// hipMemcpyAsync(DeviceToHost) of a large buffer runs as a full-grid blit
// kernel on this runtime (__amd_rocclr_copyBuffer): its waves park on PCIe
// write credit in every wave slot of the chip, and the NEXT batch's first
// kernels — on the compute stream, meant to overlap it — queue behind them
// (the 4 -> 64 head conv of a C3 batch took 3.0 ms instead of 20 us next to
// it).  PCIe Gen5 x16 moves ~55 GB/s: a handful of workgroups with a few
// 16-B stores in flight per lane saturate it, so the copy is a grid of
// `blocks` workgroups (default 16 of the 256 CUs' worth) writing through the
// host-mapped pointer; everything else of the chip stays with the forward pass.
__global__ __launch_bounds__(256) void d2h_stream_kernel(const u32x4* __restrict__ src,
                                                         u32x4* __restrict__ dst, size_t n16) {
  const size_t stride = (size_t)gridDim.x * 256 * 4;
  for (size_t i = (size_t)blockIdx.x * 256 * 4 + threadIdx.x; i < n16; i += stride) {
    u32x4 v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (i + q * 256 < n16) v[q] = __builtin_nontemporal_load(src + i + q * 256);
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (i + q * 256 < n16) dst[i + q * 256] = v[q];
  }
}

extern "C" int s3_d2h_stream(s3_ctx* ctx, const void* src, void* dst_host, size_t bytes,
                             void* stream, int blocks) {
  if (!ctx || !src || !dst_host) return S3_EINVAL;
  if ((bytes & 15) || ((uintptr_t)src & 15) || ((uintptr_t)dst_host & 15))
    S3_FAIL(ctx, S3_EINVAL, "d2h_stream: 16-byte aligned buffers of a multiple of 16 bytes");
  if (bytes == 0) return S3_OK;
  void* dptr = nullptr;
  // (pinned host memory: the device-side alias of the host pointer)
  if (hipHostGetDevicePointer(&dptr, dst_host, 0) != hipSuccess) {
    (void)hipGetLastError();
    S3_FAIL(ctx, S3_EINVAL, "d2h_stream: the destination is not pinned (mapped) host memory");
  }
  if (blocks < 1) blocks = 16;
  const size_t n16 = bytes / 16;
  const size_t need = (n16 + 1023) / 1024;
  if ((size_t)blocks > need) blocks = (int)need;
  hipLaunchKernelGGL(d2h_stream_kernel, dim3(blocks), dim3(256), 0,
                     stream ? (hipStream_t)stream : ctx->stream, (const u32x4*)src, (u32x4*)dptr, n16);
  S3_HIP(ctx, hipGetLastError());
  return S3_OK;
}

extern "C" int s3_host_alloc(s3_ctx* ctx, size_t bytes, int noncoherent, void** out) {
  if (!ctx || !out || bytes == 0) return S3_EINVAL;
  *out = nullptr;
  const unsigned flags = hipHostMallocPortable | hipHostMallocMapped |
                         (noncoherent ? hipHostMallocNonCoherent : hipHostMallocCoherent);
  S3_HIP(ctx, hipHostMalloc(out, bytes, flags));
  return S3_OK;
}

extern "C" int s3_host_free(s3_ctx* ctx, void* ptr) {
  if (!ctx) return S3_EINVAL;
  if (ptr) S3_HIP(ctx, hipHostFree(ptr));
  return S3_OK;
}

extern "C" int s3_d2h_async(s3_ctx* ctx, const void* src, void* dst_host, size_t bytes, void* stream) {
  if (!ctx || !src || !dst_host) return S3_EINVAL;
  S3_HIP(ctx, hipMemcpyAsync(dst_host, src, bytes, hipMemcpyDeviceToHost,
                             stream ? (hipStream_t)stream : ctx->stream));
  return S3_OK;
}
