// Reductions of the training step: the bias gradient (two deterministic
// stages, or stage 2 alone over channel sums a fold / mask pass left behind),
// mean |p|, and the scratch buffer their partials live in.
#include "kernels_support.h"

namespace {

// bias gradient: db[c] = sum over positions of dy[pos][c].  Two stages:
// stage 1: grid of blocks, each reduces a slab of positions to partial[blk][c]
// stage 2: one block sums the partials in fixed order (deterministic)
__global__ void bias_grad_stage1(const float* __restrict__ dy, int64_t n_pos,
                                 int c, float* __restrict__ partial) {
  // thread t handles channel (t % c_pad) for positions strided by rows
  extern __shared__ float sm[];
  const int rows = blockDim.x / c;           // positions handled per sweep
  const int my_c = threadIdx.x % c, my_r = threadIdx.x / c;
  float acc = 0.f;
  if (my_r < rows) {
    // four loads in flight per lane (fixed order: still deterministic)
    const int64_t step = (int64_t)gridDim.x * rows;
    int64_t p = (int64_t)blockIdx.x * rows + my_r;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (; p + 3 * step < n_pos; p += 4 * step) {
      a0 += dy[p * c + my_c];
      a1 += dy[(p + step) * c + my_c];
      a2 += dy[(p + 2 * step) * c + my_c];
      a3 += dy[(p + 3 * step) * c + my_c];
    }
    for (; p < n_pos; p += step) a0 += dy[p * c + my_c];
    acc = (a0 + a1) + (a2 + a3);
  }
  sm[threadIdx.x] = (my_r < rows) ? acc : 0.f;
  __syncthreads();
  if (threadIdx.x < c) {
    float t = 0.f;
    for (int r = 0; r < rows; ++r) t += sm[r * c + threadIdx.x];
    partial[(int64_t)blockIdx.x * c + threadIdx.x] = t;
  }
}

// four channels per lane (c % 4 == 0): a row of c floats is c / 4 lanes wide
__global__ void bias_grad_stage1_v4(const float4* __restrict__ dy, int64_t n_pos, int c4,
                                    float* __restrict__ partial) {
  extern __shared__ float4 sm4[];
  const int rows = blockDim.x / c4;
  const int my_c = threadIdx.x % c4, my_r = threadIdx.x / c4;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (my_r < rows) {
    const int64_t step = (int64_t)gridDim.x * rows;
    int64_t p = (int64_t)blockIdx.x * rows + my_r;
    float4 a0 = acc, a1 = acc;
    auto add4 = [](float4& a, const float4 v) { a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w; };
    for (; p + step < n_pos; p += 2 * step) {
      const float4 v0 = dy[p * c4 + my_c];
      const float4 v1 = dy[(p + step) * c4 + my_c];
      add4(a0, v0); add4(a1, v1);
    }
    if (p < n_pos) add4(a0, dy[p * c4 + my_c]);
    acc = make_float4(a0.x + a1.x, a0.y + a1.y, a0.z + a1.z, a0.w + a1.w);
  }
  sm4[threadIdx.x] = acc;
  __syncthreads();
  if ((int)threadIdx.x < c4) {
    float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int r = 0; r < rows; ++r) {
      const float4 v = sm4[r * c4 + threadIdx.x];
      t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w;
    }
    reinterpret_cast<float4*>(partial)[(int64_t)blockIdx.x * c4 + threadIdx.x] = t;
  }
}

// one block per channel: 256 lanes stride over the slabs, fixed-shape tree
// (deterministic)
__global__ void bias_grad_stage2(const float* __restrict__ partial, int nblk,
                                 int c, float* __restrict__ db, int accumulate) {
  __shared__ float sm[256];
  s3_bias_stage2_body(partial, nblk, c, blockIdx.x, db, accumulate, sm);
}

// wide-channel variant (dense layers: few rows, thousands of channels): one
// thread per channel walks the rows, lanes coalesce along channels
__global__ void bias_grad_cols(const float* __restrict__ dy, int64_t n_pos,
                               int c, float* __restrict__ db, int accumulate) {
  int ch = blockIdx.x * blockDim.x + threadIdx.x;
  if (ch >= c) return;
  float t = 0.f;
  for (int64_t p = 0; p < n_pos; ++p) t += dy[p * c + ch];
  db[ch] = accumulate ? db[ch] + t : t;
}

// ... the same for MANY rows and > 256 channels (the 64 -> 512 / 576 / 768 /
// 1600 expansion convs of the shipped generators: one serial walk per channel
// took 4 ms at 46 000 positions): blockIdx.y owns a slice of the rows and
// writes one partial row; bias_grad_stage2 sums the slices
__global__ void bias_grad_cols_split(const float* __restrict__ dy, int64_t n_pos, int c,
                                     float* __restrict__ partial) {
  const int ch = blockIdx.x * blockDim.x + threadIdx.x;
  if (ch >= c) return;
  const int64_t per = (n_pos + gridDim.y - 1) / gridDim.y;
  const int64_t p0 = (int64_t)blockIdx.y * per;
  const int64_t p1 = p0 + per < n_pos ? p0 + per : n_pos;
  float t0 = 0.f, t1 = 0.f, t2 = 0.f, t3 = 0.f;
  int64_t p = p0;
  for (; p + 4 <= p1; p += 4) {
    t0 += dy[p * c + ch]; t1 += dy[(p + 1) * c + ch];
    t2 += dy[(p + 2) * c + ch]; t3 += dy[(p + 3) * c + ch];
  }
  for (; p < p1; ++p) t0 += dy[p * c + ch];
  partial[(int64_t)blockIdx.y * c + ch] = (t0 + t1) + (t2 + t3);
}

__global__ void mean_abs_stage1(const float* __restrict__ p, int64_t n,
                                float* __restrict__ partial) {
  __shared__ float sm[8];
  float acc = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    acc += fabsf(p[i]);
  float t = block_sum(acc, sm);
  if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

__global__ void sum_stage2(const float* __restrict__ partial, int nblk,
                           float scale, float* __restrict__ out,
                           int accumulate) {
  __shared__ float sm[8];
  float acc = 0.f;
  for (int i = threadIdx.x; i < nblk; i += blockDim.x) acc += partial[i];
  float t = block_sum(acc, sm);
  if (threadIdx.x == 0) out[0] = accumulate ? out[0] + t * scale : t * scale;
}

}  // namespace

int ensure_scratch(s3_ctx* ctx, size_t bytes) {
  if (ctx->scratch_bytes >= bytes) return S3_OK;
  if (ctx->capturing) S3_FAIL(ctx, S3_EINVAL, "scratch would grow inside a capture (run the step eagerly once first)");
  if (ctx->scratch) {
    if (ctx->graphs_made) {
      ctx->retired.push_back(ctx->scratch);
    } else {
      S3_HIP(ctx, hipStreamSynchronize(ctx->stream));
      S3_HIP(ctx, hipFree(ctx->scratch));
    }
    ctx->scratch = nullptr; ctx->scratch_bytes = 0;
  }
  size_t want = bytes < (size_t)(1 << 20) ? (size_t)(1 << 20) : bytes;
  S3_HIP(ctx, hipMalloc((void**)&ctx->scratch, want));
  S3_HIP(ctx, hipMemsetAsync(ctx->scratch, ctx->opt.has[S3O_POISON_ALLOC] ? 0xFF : 0, want, ctx->stream));
  ctx->scratch_bytes = want;
  return S3_OK;
}

// stage 2 of the bias gradient from channel sums a fold kernel left behind
int launch_bias_grad_from_partial(s3_ctx* ctx, const float* partial, int nblk, int c, float* db, int accumulate,
                                  bool defer) {
  if (ctx->pend_bias.partial) {
    int rc = s3_flush_pending_bias(ctx);
    if (rc) return rc;
  }
  if (defer && !s3_opt_has(S3O_NO_SEG_REDUCE)) {
    // (the 5 us launch rides along the weight gradient's reduction: 44 of the
    // 56 per C2 training step)
    ctx->pend_bias.partial = partial; ctx->pend_bias.nblk = nblk; ctx->pend_bias.c = c;
    ctx->pend_bias.db = db; ctx->pend_bias.accumulate = accumulate;
    return S3_OK;
  }
  hipLaunchKernelGGL(bias_grad_stage2, dim3(c), dim3(256), 0, ctx->stream, partial, nblk, c, db, accumulate);
  ++ctx->stat[S3_STAT_BIAS_PARTIAL];
  S3_HIP(ctx, hipGetLastError());
  return S3_OK;
}

int s3_flush_pending_bias(s3_ctx* ctx) {
  if (!ctx->pend_bias.partial) return S3_OK;
  const s3_ctx::PendingBias j = ctx->pend_bias;
  ctx->pend_bias.partial = nullptr;
  hipLaunchKernelGGL(bias_grad_stage2, dim3(j.c), dim3(256), 0, ctx->stream, j.partial, j.nblk, j.c, j.db, j.accumulate);
  ++ctx->stat[S3_STAT_BIAS_PARTIAL_FLUSH];
  S3_HIP(ctx, hipGetLastError());
  return S3_OK;
}

int launch_bias_grad(s3_ctx* ctx, const float* dy, int64_t n_pos, int c,
                     float* db, int accumulate) {
  if (c > 256) {
    if (n_pos >= 256) {
      // conv layers: split the rows over ~4 blocks per CU, then the fixed-shape tree
      const int cb = (c + 255) / 256;
      int ns = (4 * ctx->num_cu + cb - 1) / cb;
      if ((int64_t)ns * 32 > n_pos) ns = (int)((n_pos + 31) / 32);
      int rc = ensure_scratch(ctx, (size_t)ns * c * sizeof(float));
      if (rc) return rc;
      hipLaunchKernelGGL(bias_grad_cols_split, dim3(cb, ns), dim3(256), 0, ctx->stream, dy, n_pos, c, ctx->scratch);
      ++ctx->stat[S3_STAT_BIAS_COLS_SPLIT];
      hipLaunchKernelGGL(bias_grad_stage2, dim3(c), dim3(256), 0, ctx->stream, ctx->scratch, ns, c, db, accumulate);
      S3_HIP(ctx, hipGetLastError());
      return S3_OK;
    }
    hipLaunchKernelGGL(bias_grad_cols, dim3((c + 255) / 256), dim3(256), 0, ctx->stream, dy, n_pos, c, db, accumulate);
    ++ctx->stat[S3_STAT_BIAS_COLS];
    S3_HIP(ctx, hipGetLastError());
    return S3_OK;
  }
  int block = c <= 256 ? 256 : 1024;
  int rows = block / c;
  int64_t want = (n_pos + rows - 1) / rows;
  // stage 2 walks the partial slabs serially per channel (deterministic);
  // enough slabs to put four blocks on every CU
  const int cap = 4 * ctx->num_cu;
  int nblk = (int)(want < cap ? (want < 1 ? 1 : want) : cap);
  int rc = ensure_scratch(ctx, (size_t)nblk * c * sizeof(float));
  if (rc) return rc;
  if ((c & 3) == 0 && (((uintptr_t)dy) & 15) == 0) {
    const int c4 = c / 4, rows4 = block / c4;
    int64_t want4 = (n_pos + rows4 - 1) / rows4;
    if (want4 < nblk) nblk = (int)(want4 < 1 ? 1 : want4);
    hipLaunchKernelGGL(bias_grad_stage1_v4, dim3(nblk), dim3(block), block * sizeof(float4), ctx->stream,
                       (const float4*)dy, n_pos, c4, ctx->scratch);
    ++ctx->stat[S3_STAT_BIAS_STAGE1_V4];
  } else {
    hipLaunchKernelGGL(bias_grad_stage1, dim3(nblk), dim3(block), block * sizeof(float), ctx->stream, dy, n_pos, c, ctx->scratch);
    ++ctx->stat[S3_STAT_BIAS_STAGE1];
  }
  hipLaunchKernelGGL(bias_grad_stage2, dim3(c), dim3(256), 0, ctx->stream, ctx->scratch, nblk, c, db, accumulate);
  S3_HIP(ctx, hipGetLastError());
  return S3_OK;
}

int launch_mean_abs(s3_ctx* ctx, const float* p, int64_t n, float* out_dev) {
  int nblk = grid_for(n, ctx->num_cu);
  if (nblk > 1024) nblk = 1024;
  int rc = ensure_scratch(ctx, (size_t)(nblk + 4) * sizeof(float));
  if (rc) return rc;
  hipLaunchKernelGGL(mean_abs_stage1, dim3(nblk), dim3(kBlock), 0, ctx->stream, p, n, ctx->scratch);
  launch_sum_stage2(ctx, ctx->scratch, nblk, 1.f / (float)n, out_dev, 0);
  S3_HIP(ctx, hipGetLastError());
  return S3_OK;
}

void launch_sum_stage2(s3_ctx* ctx, const float* partial, int nblk, float scale, float* out, int accumulate) {
  hipLaunchKernelGGL(sum_stage2, dim3(1), dim3(kBlock), 0, ctx->stream, partial, nblk, scale, out, accumulate);
}
