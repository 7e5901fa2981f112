// Element passes of the Sup3rGan path: activations and their adjoints, the
// mask pass of a conv (activation adjoint + depth-to-space store permutation,
// optionally with a bf16 copy and riding channel sums), residual adds, fill.
#include "kernels_support.h"
#include "wave_prims.h"

namespace {

// ------------------------------------------------------------- elementwise
__device__ inline float act_d(float y, int act, float alpha) {
  if (act == S3_ACT_RELU) return y > 0.f ? 1.f : 0.f;
  if (act == S3_ACT_LEAKY) return y > 0.f ? 1.f : alpha;
  return 1.f;
}

__global__ void act_kernel(const float* __restrict__ x, float* __restrict__ y,
                           int64_t n, int act, float alpha) {
  int64_t n4 = n / 4;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4;
       i += stride) {
    float4 v = reinterpret_cast<const float4*>(x)[i];
    v.x = act_f(v.x, act, alpha); v.y = act_f(v.y, act, alpha);
    v.z = act_f(v.z, act, alpha); v.w = act_f(v.w, act, alpha);
    reinterpret_cast<float4*>(y)[i] = v;
  }
  for (int64_t i = n4 * 4 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       i < n; i += stride)
    y[i] = act_f(x[i], act, alpha);
}

__global__ void act_bwd_kernel(const float* __restrict__ y,
                               const float* __restrict__ dy,
                               float* __restrict__ dx, int64_t n, int act,
                               float alpha) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride)
    dx[i] = dy[i] * act_d(y[i], act, alpha);
}

// dpre[n,o0,o1,o2,c] = dy[perm] * act'(y[perm]) with the d2s store permutation
template <bool Y16>
__global__ void conv_epilogue_bwd_kernel(const float* __restrict__ y,
                                         const float* __restrict__ dy,
                                         float* __restrict__ dpre, ConvGeom g) {
  const int64_t total = (int64_t)g.N * g.O[0] * g.O[1] * g.O[2] * g.Cout;
  const int b = g.d2s;
  const int co = g.Cout / (b * b);
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    int64_t src = idx;
    if (b > 1) {
      int64_t r = idx;
      int c = (int)(r % g.Cout); r /= g.Cout;
      int o2 = (int)(r % g.O[2]); r /= g.O[2];
      int o1 = (int)(r % g.O[1]); r /= g.O[1];
      int o0 = (int)(r % g.O[0]); r /= g.O[0];
      int n = (int)r;
      int blk = c / co, cc = c % co;
      src = ((((int64_t)n * g.O[0] * b + o0 * b + blk / b) * (g.O[1] * b) +
              o1 * b + blk % b) * g.O[2] + o2) * co + cc;
    }
    // (Y16: the saved activation is a bf16 tensor; only its sign matters
    // for ReLU / LeakyReLU)
    const float yv = Y16 ? __uint_as_float((unsigned)reinterpret_cast<const unsigned short*>(y)[src] << 16)
                         : y[src];
    dpre[idx] = dy[src] * act_d(yv, g.act, g.alpha);
  }
}

// depth-to-space variant, four channels per lane, walking dPre (the
// DESTINATION) in order: the generic kernel above spends 89 % of the SIMD
// cycles on five 64-bit divisions per ELEMENT (PMC, 64 -> 200 + d2s 5 conv of
// C2: 0.59 ms).  Here a lane owns 4 consecutive channels of one (cell, block):
// 32-bit index math when the tensor allows, one division chain per four
// elements, fully coalesced 16-B stores (whole 128-B lines per wave) and 16-B /
// 8-B gathers of dy / y from the hi-res layout (32-B sectors, nothing wasted).
// (Walking the hi-res layout instead scatters 16-B pieces of every dPre line
// over 25 far-apart moments: 0.52 ms.)
template <bool Y16, bool D16 = false>
__global__ void conv_epilogue_bwd_d2s4_kernel(const void* __restrict__ y, const float4* __restrict__ dy,
                                              float4* __restrict__ dpre, ConvGeom g, float slope,
                                              unsigned short* __restrict__ d16 = nullptr,
                                              float* __restrict__ bsum = nullptr) {
  // dpre (nullable with D16): every reader of this dPre takes the bf16 copy.
  // bsum (nullable): per-workgroup channel sums of dpre = the conv's bias
  // gradient for bias_grad_stage2; the launch then uses a block size that is
  // a multiple of C_out / 4, so that a lane keeps one channel group
  // (conv_epilogue_bwd_d2s4_block) — with the fp32 store gone too the 64 ->
  // 200 conv of C2 (118 M elements) saves 0.47 GB of stores and the 0.47 GB
  // bias_grad_stage1 read them back with.
  float4 bs = make_float4(0.f, 0.f, 0.f, 0.f);
  const unsigned b = (unsigned)g.d2s, co4 = ((unsigned)g.Cout / (b * b)) >> 2, C4 = (unsigned)g.Cout >> 2;
  const unsigned O0 = (unsigned)g.O[0], O1 = (unsigned)g.O[1], O2 = (unsigned)g.O[2];
  const int64_t total = (int64_t)g.N * O0 * O1 * O2 * C4;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    unsigned c4, o2, o1, o0, n;
    if (total <= 0xffffffffLL) {
      unsigned r = (unsigned)idx, q;
      q = r / C4; c4 = r - q * C4; r = q;
      q = r / O2; o2 = r - q * O2; r = q;
      q = r / O1; o1 = r - q * O1; r = q;
      q = r / O0; o0 = r - q * O0; n = q;
    } else {
      int64_t r = idx;
      c4 = (unsigned)(r % C4); r /= C4;
      o2 = (unsigned)(r % O2); r /= O2;
      o1 = (unsigned)(r % O1); r /= O1;
      o0 = (unsigned)(r % O0); r /= O0;
      n = (unsigned)r;
    }
    const unsigned blk = c4 / co4, cc4 = c4 - blk * co4, p0 = blk / b, p1 = blk - p0 * b;
    // float4 index of the hi-res cell (n, o0 b + p0, o1 b + p1, o2), channels 4 cc4 ..
    const int64_t src = ((((int64_t)n * O0 * b + o0 * b + p0) * (O1 * b) + o1 * b + p1) * O2 + o2) * co4 + cc4;
    float4 d = dy[src];
    if (Y16) {
      const uint2 h = reinterpret_cast<const uint2*>(y)[src];
      auto pos = [](unsigned v) { return (v & 0x8000u) == 0 && (v & 0x7FFFu) != 0; };
      d.x *= pos(h.x & 0xFFFFu) ? 1.f : slope; d.y *= pos(h.x >> 16) ? 1.f : slope;
      d.z *= pos(h.y & 0xFFFFu) ? 1.f : slope; d.w *= pos(h.y >> 16) ? 1.f : slope;
    } else {
      const float4 v = reinterpret_cast<const float4*>(y)[src];
      d.x *= v.x > 0.f ? 1.f : slope; d.y *= v.y > 0.f ? 1.f : slope;
      d.z *= v.z > 0.f ? 1.f : slope; d.w *= v.w > 0.f ? 1.f : slope;
    }
    if (dpre) dpre[idx] = d;
    bs.x += d.x; bs.y += d.y; bs.z += d.z; bs.w += d.w;
    if constexpr (D16) {   // bf16 copy for the MFMA gradient kernels
      reinterpret_cast<uint2*>(d16)[idx] = make_uint2(pk2(d.x, d.y), pk2(d.z, d.w));
    }
  }
  if (bsum) {
    __shared__ float4 bred[256];
    bred[threadIdx.x] = bs;
    __syncthreads();
    if (threadIdx.x < C4) {
      float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
      for (unsigned q = threadIdx.x; q < blockDim.x; q += C4) {
        const float4 v = bred[q];
        t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w;
      }
      reinterpret_cast<float4*>(bsum)[(int64_t)blockIdx.x * C4 + threadIdx.x] = t;
    }
  }
}

// the same without a store permutation, four channels per lane
template <bool Y16>
__global__ void conv_epilogue_bwd4_kernel(const void* __restrict__ y, const float4* __restrict__ dy,
                                          float4* __restrict__ dpre, int64_t n4, float slope,
                                          unsigned short* __restrict__ d16, float* __restrict__ bsum,
                                          int c4n) {
  // bsum (nullable, needs c4n | 256): per-workgroup channel sums of dpre — the
  // conv's bias gradient — for bias_grad_stage2 (a lane keeps one channel
  // group: the grid stride is a multiple of c4n), as in gather_bwd_pad4_kernel
  float4 bs = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    float4 d = dy[i];
    if (Y16) {
      const uint2 h = reinterpret_cast<const uint2*>(y)[i];
      auto pos = [](unsigned v) { return (v & 0x8000u) == 0 && (v & 0x7FFFu) != 0; };
      d.x *= pos(h.x & 0xFFFFu) ? 1.f : slope; d.y *= pos(h.x >> 16) ? 1.f : slope;
      d.z *= pos(h.y & 0xFFFFu) ? 1.f : slope; d.w *= pos(h.y >> 16) ? 1.f : slope;
    } else {
      const float4 v = reinterpret_cast<const float4*>(y)[i];
      d.x *= v.x > 0.f ? 1.f : slope; d.y *= v.y > 0.f ? 1.f : slope;
      d.z *= v.z > 0.f ? 1.f : slope; d.w *= v.w > 0.f ? 1.f : slope;
    }
    // (dpre == nullptr: every reader of this dPre takes the bf16 copy and the
    // bias gradient rides along in bsum — the 151 MB fp32 store is skipped)
    if (dpre) dpre[i] = d;
    bs.x += d.x; bs.y += d.y; bs.z += d.z; bs.w += d.w;
    if (d16) {   // bf16 copy for the MFMA gradient kernels (see gather_bwd_pad4_kernel)
      reinterpret_cast<uint2*>(d16)[i] = make_uint2(pk2(d.x, d.y), pk2(d.z, d.w));
    }
  }
  if (bsum) {
    __shared__ float4 bred[256];
    bred[threadIdx.x] = bs;
    __syncthreads();
    if ((int)threadIdx.x < c4n) {
      float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int q = threadIdx.x; q < 256; q += c4n) {
        const float4 v = bred[q];
        t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w;
      }
      reinterpret_cast<float4*>(bsum)[(int64_t)blockIdx.x * c4n + threadIdx.x] = t;
    }
  }
}

__global__ void add_kernel(const float* __restrict__ a,
                           const float* __restrict__ b, float* __restrict__ y,
                           int64_t n, int c, int bcast_c) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride)
    y[i] = a[i] + (bcast_c ? b[i / c] : b[i]);
}

// bf16 cells: y = bf16(a + b), eight channels per lane (inference plans: a
// SkipConnection add that no conv epilogue absorbed — the second of two adds
// behind one conv in sup3rcc/gen_*_5x_1x_* at hi-res — stays in bf16 so that
// the convs on either side keep their bf16 kernels)
__global__ void add16_kernel(const uint4* __restrict__ a, const uint4* __restrict__ b, uint4* __restrict__ y,
                             int64_t n8) {
  auto add2 = [](unsigned u, unsigned v) { return pk2(bf_lo(u) + bf_lo(v), bf_hi(u) + bf_hi(v)); };
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += stride) {
    const uint4 p = a[i], q = b[i];
    y[i] = make_uint4(add2(p.x, q.x), add2(p.y, q.y), add2(p.z, q.z), add2(p.w, q.w));
  }
}

__global__ void axpy_kernel(const float* __restrict__ x, float* __restrict__ y,
                            int64_t n) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride)
    y[i] += x[i];
}
__global__ void axpy4_kernel(const float4* __restrict__ x, float4* __restrict__ y, int64_t n4) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const float4 a = x[i];
    float4 b = y[i];
    b.x += a.x; b.y += a.y; b.z += a.z; b.w += a.w;
    y[i] = b;
  }
}

__global__ void fill_kernel(float* __restrict__ p, int64_t n, float v) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride)
    p[i] = v;
}

}  // namespace

int launch_act(s3_ctx* ctx, const float* x, float* y, int64_t n, int act,
               float alpha) {
  hipLaunchKernelGGL(act_kernel, dim3(grid_for(n / 4 + 1, ctx->num_cu)), dim3(kBlock), 0, ctx->stream, x, y, n, act, alpha);
  S3_HIP(ctx, hipGetLastError());
  return S3_OK;
}

int launch_act_bwd(s3_ctx* ctx, const float* y, const float* dy, float* dx,
                   int64_t n, int act, float alpha) {
  hipLaunchKernelGGL(act_bwd_kernel, dim3(grid_for(n, ctx->num_cu)), dim3(kBlock), 0, ctx->stream, y, dy, dx, n, act, alpha);
  S3_HIP(ctx, hipGetLastError());
  return S3_OK;
}

static bool conv_epilogue_bwd_d2s4_geom(const ConvGeom& g) {
  return g.d2s > 1 && ((g.Cout / (g.d2s * g.d2s)) & 3) == 0 && (g.Cout & 3) == 0 &&
         (g.act == S3_ACT_LEAKY || g.act == S3_ACT_RELU || g.act == S3_ACT_NONE);
}
// the 4-channel mask pass: no store permutation, four elements per lane
static bool conv_epilogue_bwd_c4_geom(const ConvGeom& g) {
  const int64_t n = (int64_t)g.N * g.O[0] * g.O[1] * g.O[2] * g.Cout;
  return g.d2s <= 1 && (n & 3) == 0 && (g.act == S3_ACT_LEAKY || g.act == S3_ACT_RELU);
}
bool conv_epilogue_bwd_d16_ok(const ConvGeom& g) {
  return conv_epilogue_bwd_d2s4_geom(g) /* (the depth-to-space walk, bf16 y) */ || conv_epilogue_bwd_c4_geom(g);
}

// channel sums can ride along the mask pass (bias gradient): C_out / 4 | 256
// (depth-to-space walk: any C_out / 4 <= 256, with a bf16 y and the bf16 copy)
static int conv_epilogue_bwd_d2s4_block(const ConvGeom& g) {
  const int c4n = g.Cout >> 2;
  return c4n >= 1 && c4n <= 256 ? (256 / c4n) * c4n : 0;
}
bool conv_epilogue_bwd_bsum_ok(const ConvGeom& g) {
  const int c4n = g.Cout >> 2;
  if (conv_epilogue_bwd_d2s4_geom(g)) return conv_epilogue_bwd_d2s4_block(g) > 0 && kBlock == 256;
  return conv_epilogue_bwd_c4_geom(g) && (g.Cout & 3) == 0 && c4n >= 1 && c4n <= 64 && (256 % c4n) == 0 && kBlock == 256;
}
int conv_epilogue_bwd_blocks(const s3_ctx* ctx, const ConvGeom& g, bool with_bsum) {
  const int64_t n4 = (int64_t)g.N * g.O[0] * g.O[1] * g.O[2] * g.Cout / 4;
  const int blk = (with_bsum && conv_epilogue_bwd_d2s4_geom(g)) ? conv_epilogue_bwd_d2s4_block(g) : kBlock;
  const int64_t want = (n4 + blk - 1) / blk;
  const int64_t cap = with_bsum ? 16 * ctx->num_cu : 32 * ctx->num_cu;   // (bsum rows: <= 4096)
  return (int)(want < cap ? (want < 1 ? 1 : want) : cap);
}

int launch_conv_epilogue_bwd(s3_ctx* ctx, const ConvGeom& g, const float* y,
                             const float* dy, float* dpre, int y_bf16, void* d16, float* bsum) {
  int64_t n = (int64_t)g.N * g.O[0] * g.O[1] * g.O[2] * g.Cout;
  const bool c4 = conv_epilogue_bwd_c4_geom(g);
  if (!dpre && !(d16 && (c4 || (conv_epilogue_bwd_d2s4_geom(g) && y_bf16))))
    S3_FAIL(ctx, S3_EINVAL, "conv_epilogue_bwd: a bf16-only dPre needs the 4-channel mask pass");
  if (c4) {
    const float slope = g.act == S3_ACT_LEAKY ? g.alpha : 0.f;
    const int64_t n4 = n / 4;
    if (bsum && !conv_epilogue_bwd_bsum_ok(g)) S3_FAIL(ctx, S3_EINVAL, "conv_epilogue_bwd: channel sums need C_out / 4 | 256");
    const dim3 grid((unsigned)conv_epilogue_bwd_blocks(ctx, g, bsum != nullptr));
    if (y_bf16)
      hipLaunchKernelGGL(conv_epilogue_bwd4_kernel<true>, grid, dim3(kBlock), 0, ctx->stream, (const void*)y,
                         (const float4*)dy, (float4*)dpre, n4, slope, (unsigned short*)d16, bsum, g.Cout >> 2);
    else
      hipLaunchKernelGGL(conv_epilogue_bwd4_kernel<false>, grid, dim3(kBlock), 0, ctx->stream, (const void*)y,
                         (const float4*)dy, (float4*)dpre, n4, slope, (unsigned short*)d16, bsum, g.Cout >> 2);
    ++ctx->stat[S3_STAT_EPI_C4];
    if (bsum) ++ctx->stat[S3_STAT_EPI_C4_BSUM];
    S3_HIP(ctx, hipGetLastError());
    return S3_OK;
  }
  if ((bsum || d16) && !(conv_epilogue_bwd_d2s4_geom(g) && y_bf16 && d16 && (!bsum || conv_epilogue_bwd_bsum_ok(g))))
    S3_FAIL(ctx, S3_EINVAL, "conv_epilogue_bwd: side outputs need the 4-channel path");
  if (conv_epilogue_bwd_d2s4_geom(g)) {
    const float slope = g.act == S3_ACT_LEAKY ? g.alpha : (g.act == S3_ACT_RELU ? 0.f : 1.f);
    const dim3 grid(grid_for(n / 4, ctx->num_cu));
    if (y_bf16 && d16 && bsum)
      hipLaunchKernelGGL((conv_epilogue_bwd_d2s4_kernel<true, true>), dim3((unsigned)conv_epilogue_bwd_blocks(ctx, g, true)),
                         dim3(conv_epilogue_bwd_d2s4_block(g)), 0, ctx->stream, (const void*)y, (const float4*)dy,
                         (float4*)dpre, g, slope, (unsigned short*)d16, bsum);
    else if (y_bf16 && d16)
      hipLaunchKernelGGL((conv_epilogue_bwd_d2s4_kernel<true, true>), grid, dim3(kBlock), 0, ctx->stream,
                         (const void*)y, (const float4*)dy, (float4*)dpre, g, slope, (unsigned short*)d16);
    else if (y_bf16)
      hipLaunchKernelGGL(conv_epilogue_bwd_d2s4_kernel<true>, grid, dim3(kBlock), 0, ctx->stream, (const void*)y,
                         (const float4*)dy, (float4*)dpre, g, slope);
    else
      hipLaunchKernelGGL(conv_epilogue_bwd_d2s4_kernel<false>, grid, dim3(kBlock), 0, ctx->stream, (const void*)y,
                         (const float4*)dy, (float4*)dpre, g, slope);
    ++ctx->stat[S3_STAT_EPI_D2S4];
    if (y_bf16 && d16 && bsum) ++ctx->stat[S3_STAT_EPI_D2S4_BSUM];
    S3_HIP(ctx, hipGetLastError());
    return S3_OK;
  }
  if (y_bf16)
    hipLaunchKernelGGL(conv_epilogue_bwd_kernel<true>, dim3(grid_for(n, ctx->num_cu)), dim3(kBlock), 0, ctx->stream, y, dy, dpre, g);
  else
    hipLaunchKernelGGL(conv_epilogue_bwd_kernel<false>, dim3(grid_for(n, ctx->num_cu)), dim3(kBlock), 0, ctx->stream, y, dy, dpre, g);
  ++ctx->stat[S3_STAT_EPI_GENERIC];
  S3_HIP(ctx, hipGetLastError());
  return S3_OK;
}

int launch_add(s3_ctx* ctx, const float* a, const float* b, float* y, int64_t n,
               int c, int bcast_c) {
  hipLaunchKernelGGL(add_kernel, dim3(grid_for(n, ctx->num_cu)), dim3(kBlock), 0, ctx->stream, a, b, y, n, c, bcast_c);
  S3_HIP(ctx, hipGetLastError());
  return S3_OK;
}

int launch_add16(s3_ctx* ctx, const void* a, const void* b, void* y, int64_t n) {
  if (n & 7) S3_FAIL(ctx, S3_EINVAL, "add16: element count must be a multiple of 8");
  hipLaunchKernelGGL(add16_kernel, dim3(grid_for(n / 8, ctx->num_cu)), dim3(kBlock), 0, ctx->stream,
                     (const uint4*)a, (const uint4*)b, (uint4*)y, n / 8);
  S3_HIP(ctx, hipGetLastError());
  return S3_OK;
}

int launch_axpy(s3_ctx* ctx, const float* x, float* y, int64_t n) {
  if ((n & 3) == 0 && (((uintptr_t)x | (uintptr_t)y) & 15) == 0) {
    hipLaunchKernelGGL(axpy4_kernel, dim3(grid_for(n / 4, ctx->num_cu)), dim3(kBlock), 0, ctx->stream,
                       (const float4*)x, (float4*)y, n / 4);
    ++ctx->stat[S3_STAT_AXPY4];
    S3_HIP(ctx, hipGetLastError());
    return S3_OK;
  }
  hipLaunchKernelGGL(axpy_kernel, dim3(grid_for(n, ctx->num_cu)), dim3(kBlock), 0, ctx->stream, x, y, n);
  ++ctx->stat[S3_STAT_AXPY];
  S3_HIP(ctx, hipGetLastError());
  return S3_OK;
}

int launch_fill(s3_ctx* ctx, float* p, int64_t n, float v) {
  hipLaunchKernelGGL(fill_kernel, dim3(grid_for(n, ctx->num_cu)), dim3(kBlock), 0, ctx->stream, p, n, v);
  S3_HIP(ctx, hipGetLastError());
  return S3_OK;
}

extern "C" int s3_fill(s3_ctx* ctx, float* dst, int64_t n, float value) {
  if (!ctx) return S3_EINVAL;
  return launch_fill(ctx, dst, n, value);
}
