// The parameter store (weights, gradients and the two optimizer moments in four
// flat fp32 buffers), the optimizer steps over it and the arming of the
// bucketed gradient all-reduce that the backward pass feeds (plan_backward.cpp,
// comm.cpp).
#include <cmath>

#include "plan_internal.h"

// ------------------------------------------------------------------- params
extern "C" int s3_params_create(s3_ctx* ctx, int n, const int64_t* sizes,
                                s3_params** out) {
  if (!ctx || !out || n < 0) return S3_EINVAL;
  s3_params* p = new s3_params();
  p->ctx = ctx;
  int64_t off = 0;
  for (int i = 0; i < n; ++i) {
    if (sizes[i] <= 0) { delete p; S3_FAIL(ctx, S3_EINVAL, "params_create: non-positive size"); }
    p->p.push_back({off, sizes[i]});
    off += (sizes[i] + 3) / 4 * 4;  // keep every tensor 16-B aligned
  }
  p->total = off;
  size_t bytes = (size_t)(off > 0 ? off : 4) * sizeof(float);
  for (int k = 0; k < 4; ++k) {
    hipError_t e = hipMalloc((void**)&p->buf[k], bytes);
    if (e != hipSuccess) {
      ctx->err = std::string("params hipMalloc: ") + hipGetErrorString(e);
      for (int q = 0; q < k; ++q) (void)hipFree(p->buf[q]);
      delete p;
      return S3_ENOMEM;
    }
    S3_HIP(ctx, hipMemsetAsync(p->buf[k], 0, bytes, ctx->stream));
  }
  *out = p;
  return S3_OK;
}

extern "C" void s3_params_destroy(s3_params* p) {
  if (!p) return;
  (void)hipStreamSynchronize(p->ctx->stream);
  for (int k = 0; k < 4; ++k)
    if (p->buf[k]) (void)hipFree(p->buf[k]);
  if (p->hyper_dev) (void)hipFree(p->hyper_dev);
  delete p;
}

extern "C" int64_t s3_params_total(const s3_params* p) { return p ? p->total : 0; }

static int params_check(s3_params* p, int which, int idx) {
  if (!p) return S3_EINVAL;
  if (which < 0 || which > 3 || idx < 0 || idx >= (int)p->p.size())
    S3_FAIL(p->ctx, S3_EINVAL, "params: bad buffer / index");
  return S3_OK;
}

extern "C" int s3_params_set(s3_params* p, int which, int idx, const float* host) {
  int rc = params_check(p, which, idx);
  if (rc) return rc;
  s3_ctx* ctx = p->ctx;
  S3_HIP(ctx, hipMemcpyAsync(p->buf[which] + p->p[idx].offset, host,
                             p->p[idx].size * sizeof(float),
                             hipMemcpyHostToDevice, ctx->stream));
  S3_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (which == S3_BUF_W) p->version++;
  return S3_OK;
}

extern "C" int s3_params_get(s3_params* p, int which, int idx, float* host) {
  int rc = params_check(p, which, idx);
  if (rc) return rc;
  s3_ctx* ctx = p->ctx;
  S3_HIP(ctx, hipMemcpyAsync(host, p->buf[which] + p->p[idx].offset,
                             p->p[idx].size * sizeof(float),
                             hipMemcpyDeviceToHost, ctx->stream));
  S3_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return S3_OK;
}

extern "C" void* s3_params_dptr(s3_params* p, int which, int idx) {
  if (!p || which < 0 || which > 3) return nullptr;
  if (idx < 0) return p->buf[which];
  if (idx >= (int)p->p.size()) return nullptr;
  return p->buf[which] + p->p[idx].offset;
}


extern "C" uint64_t s3_params_version(const s3_params* p) { return p ? p->version : 0; }

extern "C" int s3_params_zero_grad(s3_params* p) {
  if (!p) return S3_EINVAL;
  s3_ctx* ctx = p->ctx;
  S3_HIP(ctx, hipMemsetAsync(p->buf[S3_BUF_G], 0, (size_t)p->total * sizeof(float), ctx->stream));
  return S3_OK;
}

extern "C" int s3_params_mean_abs(s3_params* p, int which, int idx, float* host_out) {
  int rc = params_check(p, which, idx);
  if (rc) return rc;
  s3_ctx* ctx = p->ctx;
  rc = ensure_scratch(ctx, 1 << 20);
  if (rc) return rc;
  // result lands in the last float of the 1 MiB minimum scratch
  float* out_dev = ctx->scratch + (ctx->scratch_bytes / sizeof(float)) - 1;
  rc = launch_mean_abs(ctx, p->buf[which] + p->p[idx].offset, p->p[idx].size, out_dev);
  if (rc) return rc;
  S3_HIP(ctx, hipMemcpyAsync(host_out, out_dev, sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  S3_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return S3_OK;
}

extern "C" int s3_adam_step(s3_params* p, float lr, float beta1, float beta2,
                            float eps, int64_t t) {
  const double hp[4] = {lr, beta1, beta2, eps};
  return s3_optimizer_step(p, S3_OPT_ADAM, hp, 4, t);
}

extern "C" int s3_params_arm_allreduce(s3_params* p, int64_t bucket_bytes) {
  if (!p) return S3_EINVAL;
  // bucket_bytes < 0 disarms (the caller's try / finally around the backward
  // pass it armed for); without a communicator there is nothing to overlap —
  // an armed store would only leave a flag behind for a later backward pass
  p->reduced = false;
  if (bucket_bytes < 0 || !p->ctx || !p->ctx->comm) {
    p->armed = false;
    p->reduce_end = 0;
    p->buckets_issued = 0;
    return S3_OK;
  }
  p->armed = true;
  p->reduce_end = p->total;
  p->bucket_elems = bucket_bytes > 0 ? bucket_bytes / (int64_t)sizeof(float) : p->total;
  p->buckets_issued = 0;
  return S3_OK;
}

// called by s3_params_allreduce_grads (comm.cpp): 1 = the armed, bucketed
// reduction covered the whole buffer (the caller only joins the streams),
// 0 = nothing was armed (reduce the whole buffer now), -1 = armed but the
// backward pass did not reach the start of the buffer
extern "C" S3_INTERNAL int s3_params_take_armed(s3_params* p, int* n_buckets) {
  if (!p) return 0;
  if (n_buckets) *n_buckets = p->buckets_issued;
  if (p->reduced) {        // an armed backward pass covered the buffer
    p->reduced = false;
    return 1;
  }
  if (!p->armed) return 0;
  p->armed = false;        // armed, but no backward pass wrote the gradients
  return -1;
}

// Hyper-parameters arrive as doubles (they are Python floats in the keras
// configs) and are cast the way keras casts them: `1 - beta` is evaluated in
// double and THEN rounded to fp32 (keras multiplies the fp32 tensor by the
// Python scalar 1 - beta), the powers beta^t in fp32 (tf.pow of the cast
// beta).  fp32(1) - fp32(0.999) would be off by 4.7e-5 of itself.
// the step's scalars h[0..4] as the kernels take them
static int optimizer_scalars(s3_ctx* ctx, int kind, const double* hp, int n_hp, int64_t t, float* h) {
  for (int q = 0; q < 5; ++q) h[q] = 0.f;
  auto need = [&](int n) { return n_hp >= n; };
  switch (kind) {
    case S3_OPT_ADAM: {
      if (!need(4)) S3_FAIL(ctx, S3_EINVAL, "optimizer_step(Adam): {lr, beta_1, beta_2, epsilon}");
      const float b1p = powf((float)hp[1], (float)t), b2p = powf((float)hp[2], (float)t);
      h[0] = (float)hp[0] * sqrtf(1.f - b2p) / (1.f - b1p);
      h[1] = (float)(1.0 - hp[1]); h[2] = (float)(1.0 - hp[2]); h[3] = (float)hp[3];
      break;
    }
    case S3_OPT_SGD:
      if (!need(3)) S3_FAIL(ctx, S3_EINVAL, "optimizer_step(SGD): {lr, momentum, nesterov}");
      h[0] = (float)hp[0]; h[1] = (float)hp[1]; h[2] = (float)hp[2];
      break;
    case S3_OPT_RMSPROP:
      if (!need(4)) S3_FAIL(ctx, S3_EINVAL, "optimizer_step(RMSprop): {lr, rho, momentum, epsilon}");
      h[0] = (float)hp[0]; h[1] = (float)hp[1]; h[2] = (float)hp[2]; h[3] = (float)hp[3];
      h[4] = (float)(1.0 - hp[1]);
      break;
    case S3_OPT_ADAGRAD:
      if (!need(3)) S3_FAIL(ctx, S3_EINVAL, "optimizer_step(Adagrad): {lr, epsilon, initial_accumulator_value}");
      h[0] = (float)hp[0]; h[1] = (float)hp[1];
      break;
    case S3_OPT_ADAMAX: {
      if (!need(4)) S3_FAIL(ctx, S3_EINVAL, "optimizer_step(Adamax): {lr, beta_1, beta_2, epsilon}");
      const float b1p = powf((float)hp[1], (float)t);
      h[0] = (float)hp[0] / (1.f - b1p); h[1] = (float)(1.0 - hp[1]); h[2] = (float)hp[2]; h[3] = (float)hp[3];
      break;
    }
    case S3_OPT_ADAMW: {
      if (!need(5)) S3_FAIL(ctx, S3_EINVAL, "optimizer_step(AdamW): {lr, beta_1, beta_2, epsilon, weight_decay}");
      const float b1p = powf((float)hp[1], (float)t), b2p = powf((float)hp[2], (float)t);
      h[0] = (float)hp[0] * sqrtf(1.f - b2p) / (1.f - b1p);
      h[1] = (float)(1.0 - hp[1]); h[2] = (float)(1.0 - hp[2]); h[3] = (float)hp[3];
      h[4] = (float)hp[4] * (float)hp[0];
      break;
    }
    default: S3_FAIL(ctx, S3_EINVAL, "optimizer_step: unknown optimizer kind");
  }
  return S3_OK;
}

static int optimizer_launch(s3_params* p, int kind, const float* h, const float* h_dev) {
  s3_ctx* ctx = p->ctx;
  int rc;
  if (kind == S3_OPT_ADAM)
    rc = launch_adam(ctx, p->buf[S3_BUF_W], p->buf[S3_BUF_G], p->buf[S3_BUF_M], p->buf[S3_BUF_V], p->total,
                     h[0], h[1], h[2], h[3], h_dev);
  else
    rc = launch_optimizer(ctx, kind, p->buf[S3_BUF_W], p->buf[S3_BUF_G], p->buf[S3_BUF_M], p->buf[S3_BUF_V],
                          p->total, h, h_dev);
  if (rc) return rc;
  p->version++;
  return S3_OK;
}

extern "C" int s3_optimizer_step(s3_params* p, int kind, const double* hp, int n_hp, int64_t t) {
  if (!p || !hp || t < 1) return S3_EINVAL;
  s3_ctx* ctx = p->ctx;
  float h[5];
  int rc = optimizer_scalars(ctx, kind, hp, n_hp, t, h);
  if (rc) return rc;
  if (kind == S3_OPT_ADAGRAD && t == 1) {   // keras creates the accumulator filled with its initial value
    rc = launch_fill(ctx, p->buf[S3_BUF_V], p->total, (float)hp[2]);
    if (rc) return rc;
  }
  return optimizer_launch(p, kind, h, nullptr);
}

// The same step in two halves, for a captured graph: the scalars of step t are
// written to the device by a 1-thread launch OUTSIDE the graph (kernel
// arguments: no host buffer has to outlive the call), the update launch inside
// it reads them from there and is identical every step.
extern "C" int s3_optimizer_stage(s3_params* p, int kind, const double* hp, int n_hp, int64_t t) {
  if (!p || !hp || t < 1) return S3_EINVAL;
  s3_ctx* ctx = p->ctx;
  if (kind == S3_OPT_ADAGRAD && t == 1)
    S3_FAIL(ctx, S3_EINVAL, "optimizer_stage(Adagrad): the first step creates the accumulator, run it with s3_optimizer_step");
  float h[5];
  int rc = optimizer_scalars(ctx, kind, hp, n_hp, t, h);
  if (rc) return rc;
  if (!p->hyper_dev) S3_HIP(ctx, hipMalloc((void**)&p->hyper_dev, 8 * sizeof(float)));
  return launch_stage_hyper(ctx, p->hyper_dev, h);
}

extern "C" int s3_optimizer_step_staged(s3_params* p, int kind) {
  if (!p) return S3_EINVAL;
  s3_ctx* ctx = p->ctx;
  // (recorded before the first stage: the replay stages before it launches)
  if (!p->hyper_dev) S3_HIP(ctx, hipMalloc((void**)&p->hyper_dev, 8 * sizeof(float)));
  if (kind < S3_OPT_ADAM || kind > S3_OPT_ADAMW) S3_FAIL(ctx, S3_EINVAL, "optimizer_step: unknown optimizer kind");
  const float h[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  return optimizer_launch(p, kind, h, p->hyper_dev);
}

// the weights changed behind the host's back (a replayed graph stepped the
// optimizer): packed filter images of every plan are stale
extern "C" int s3_params_touch(s3_params* p) {
  if (!p) return S3_EINVAL;
  p->version++;
  return S3_OK;
}
