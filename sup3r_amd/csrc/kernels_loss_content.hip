// Content losses (MAE / MSE / ExpLoss over a channel subset, optionally
// masked) and the relativistic BCE of the adversarial loss, value and gradient
// in one pass.  (kernels_loss.hip holds the feature maps of the structured
// content losses, which end in s3_loss_content.)
#include "kernels_support.h"

namespace {

// ------------------------------------------------------------------ losses
// content loss over the first c_used channels; grad wrt a (c_a channels)
__global__ void loss_content_kernel(int kind, const float* __restrict__ a,
                                    int c_a, const float* __restrict__ b,
                                    int c_b, const float* __restrict__ mask,
                                    int c_m, int c_used, int64_t n_pos,
                                    float gscale, float* __restrict__ partial,
                                    float* __restrict__ d_a, int accumulate) {
  __shared__ float sm[8];
  const int64_t total = n_pos * c_used;
  float acc = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    int64_t p = i / c_used;
    int c = (int)(i % c_used);
    const float mk = mask ? mask[p * c_m + c] : 1.f;
    float d = (a[p * c_a + c] - b[p * c_b + c]) * mk;
    float g;
    if (kind == S3_LOSS_MAE) {
      acc += fabsf(d);
      g = (d > 0.f) ? 1.f : (d < 0.f ? -1.f : 0.f);
    } else if (kind == S3_LOSS_EXP) {
      // ExpLoss: mean(1 - exp(-(x1 - x2)^2)) (loss_metrics.py:98-118)
      const float e = __expf(-d * d);
      acc += 1.f - e;
      g = 2.f * d * e;
    } else {
      acc += d * d;
      g = 2.f * d;
    }
    if (d_a) {
      float v = g * gscale * mk;
      d_a[p * c_a + c] = accumulate ? d_a[p * c_a + c] + v : v;
    }
  }
  float t = block_sum(acc, sm);
  if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

// the dense case (every channel used, no mask, n % 4 == 0): 16-B loads and
// stores, no per-element division (the C2 hi-res batch — 29.5 M elements —
// took 146 us on the walk above: 2 x what its 354 MB cost at 5 TB/s)
__global__ void loss_content4_kernel(int kind, const float4* __restrict__ a, const float4* __restrict__ b,
                                     int64_t n4, float gscale, float* __restrict__ partial,
                                     float4* __restrict__ d_a, int accumulate) {
  __shared__ float sm[8];
  float acc = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4;
       i += (int64_t)gridDim.x * blockDim.x) {
    const float4 va = a[i], vb = b[i];
    const float d[4] = {va.x - vb.x, va.y - vb.y, va.z - vb.z, va.w - vb.w};
    float g[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (kind == S3_LOSS_MAE) {
        acc += fabsf(d[q]);
        g[q] = (d[q] > 0.f) ? 1.f : (d[q] < 0.f ? -1.f : 0.f);
      } else if (kind == S3_LOSS_EXP) {
        const float e = __expf(-d[q] * d[q]);
        acc += 1.f - e;
        g[q] = 2.f * d[q] * e;
      } else {
        acc += d[q] * d[q];
        g[q] = 2.f * d[q];
      }
      g[q] *= gscale;
    }
    if (d_a) {
      float4 v = make_float4(g[0], g[1], g[2], g[3]);
      if (accumulate) {
        const float4 o = d_a[i];
        v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w;
      }
      d_a[i] = v;
    }
  }
  float t = block_sum(acc, sm);
  if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

// relativistic BCE (single block; n is the batch size, small)
__global__ void rel_bce_kernel(const float* __restrict__ dt,
                               const float* __restrict__ dg, int n, float scale,
                               float* __restrict__ loss_out,
                               float* __restrict__ d_true,
                               float* __restrict__ d_gen) {
  __shared__ float sm[8];
  __shared__ float s_mt, s_mg, s_gt, s_gf;
  float at = 0.f, ag = 0.f;
  for (int i = threadIdx.x; i < n; i += blockDim.x) { at += dt[i]; ag += dg[i]; }
  float t = block_sum(at, sm);
  if (threadIdx.x == 0) s_mt = t / n;
  t = block_sum(ag, sm);
  if (threadIdx.x == 0) s_mg = t / n;
  __syncthreads();
  const float mt = s_mt, mg = s_mg;
  float loss = 0.f, sgt = 0.f, sgf = 0.f;
  const float inv = 1.f / (2.f * n);
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    float xt = dt[i] - mg;  // label 1
    float xf = dg[i] - mt;  // label 0
    float et = expf(-fabsf(xt)), ef = expf(-fabsf(xf));
    loss += fmaxf(xt, 0.f) - xt + log1pf(et);
    loss += fmaxf(xf, 0.f) + log1pf(ef);
    float st = xt >= 0.f ? 1.f / (1.f + et) : et / (1.f + et);
    float sf = xf >= 0.f ? 1.f / (1.f + ef) : ef / (1.f + ef);
    sgt += (st - 1.f) * inv;
    sgf += sf * inv;
  }
  t = block_sum(loss, sm);
  if (threadIdx.x == 0) loss_out[0] = t * inv;
  t = block_sum(sgt, sm);
  if (threadIdx.x == 0) s_gt = t;
  t = block_sum(sgf, sm);
  if (threadIdx.x == 0) s_gf = t;
  __syncthreads();
  if (d_true || d_gen) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
      float xt = dt[i] - mg, xf = dg[i] - mt;
      float et = expf(-fabsf(xt)), ef = expf(-fabsf(xf));
      float st = xt >= 0.f ? 1.f / (1.f + et) : et / (1.f + et);
      float sf = xf >= 0.f ? 1.f / (1.f + ef) : ef / (1.f + ef);
      float gt = (st - 1.f) * inv, gf = sf * inv;
      if (d_true) d_true[i] = scale * (gt - s_gf / n);
      if (d_gen) d_gen[i] = scale * (gf - s_gt / n);
    }
  }
}

}  // namespace

static int loss_content_impl(s3_ctx* ctx, int kind, const float* a, int c_a,
                             const float* b, int c_b, const float* mask,
                             int c_m, int c_used, int64_t n_pos, float weight,
                             float* loss_out, float* d_a, int accumulate) {
  if (!ctx) return S3_EINVAL;
  if (c_used > c_a || c_used > c_b) S3_FAIL(ctx, S3_EINVAL, "loss_content: c_used exceeds channel counts");
  int64_t total = n_pos * c_used;
  int nblk = grid_for(total, ctx->num_cu);
  if (nblk > 1024) nblk = 1024;
  int rc = ensure_scratch(ctx, (size_t)(nblk + 4) * sizeof(float));
  if (rc) return rc;
  float gscale = weight / (float)total;
  const bool dense = !mask && c_a == c_used && c_b == c_used && (total & 3) == 0 &&
                     (((uintptr_t)a | (uintptr_t)b | (uintptr_t)d_a) & 15) == 0;
  if (dense)
    hipLaunchKernelGGL(loss_content4_kernel, dim3(nblk), dim3(kBlock), 0, ctx->stream, kind, (const float4*)a,
                       (const float4*)b, total / 4, gscale, ctx->scratch, (float4*)d_a, accumulate);
  else
    hipLaunchKernelGGL(loss_content_kernel, dim3(nblk), dim3(kBlock), 0, ctx->stream, kind, a, c_a, b, c_b, mask, c_m, c_used, n_pos, gscale, ctx->scratch, d_a, accumulate);
  launch_sum_stage2(ctx, ctx->scratch, nblk, 1.f / (float)total, loss_out, 0);
  S3_HIP(ctx, hipGetLastError());
  return S3_OK;
}

extern "C" int s3_loss_content(s3_ctx* ctx, int kind, const float* a, int c_a,
                               const float* b, int c_b, int c_used,
                               int64_t n_pos, float weight, float* loss_out,
                               float* d_a, int accumulate) {
  return loss_content_impl(ctx, kind, a, c_a, b, c_b, nullptr, 0, c_used, n_pos,
                           weight, loss_out, d_a, accumulate);
}

extern "C" int s3_loss_content_masked(s3_ctx* ctx, int kind, const float* a,
                                      int c_a, const float* b, int c_b,
                                      const float* mask, int c_m, int c_used,
                                      int64_t n_pos, float weight,
                                      float* loss_out, float* d_a,
                                      int accumulate) {
  if (!mask || c_used > c_m) { if (ctx) ctx->err = "loss_content_masked: bad mask"; return S3_EINVAL; }
  return loss_content_impl(ctx, kind, a, c_a, b, c_b, mask, c_m, c_used, n_pos,
                           weight, loss_out, d_a, accumulate);
}

extern "C" int s3_loss_rel_bce(s3_ctx* ctx, const float* disc_true,
                               const float* disc_gen, int n, float scale,
                               float* loss_out, float* d_true, float* d_gen) {
  if (!ctx) return S3_EINVAL;
  hipLaunchKernelGGL(rel_bce_kernel, dim3(1), dim3(kBlock), 0, ctx->stream, disc_true, disc_gen, n, scale, loss_out, d_true, d_gen);
  S3_HIP(ctx, hipGetLastError());
  return S3_OK;
}
