// Training targets of the conditional-moment batch queues on the device.
// ConditionalBatchQueue.post_proc (sup3r/preprocessing/batch_queues/
// conditional.py:151-166) derives, on the host, from every (low_res, high_res)
// batch
//   make_output  one of six rules (:169-288): HR, HR - LR^, (HR - <HR|LR>)^2,
//                HR^2, (HR - LR^ - <SF|LR>)^2, (HR - LR^)^2, where LR^ is the
//                low-res batch enhanced back to the hi-res grid with
//                scipy.ndimage.zoom(order=0) in space and zoom(order=0) or
//                interp1d(fill_value='extrapolate') in time
//                (batch_queues/utilities.py:12-54, :106-173), and <.|LR> the
//                output of the first-moment model joined with the exogenous
//                channels of the truth (_combine_loss_input, abstract.py:438-459);
//   make_mask    1 inside a box of the hi-res grid, 0 outside (:79-127).
// Here that is ONE streaming pass over the hi-res batch: 16-byte loads of hr
// (and of the first moment), 16-byte stores of the target (and of the mask);
// the low-res batch is 1 / (s^2 t_enhance) of the traffic and is read through
// the cache.  No LDS, no atomics.
#include "common.h"

namespace {

constexpr int kBlk = kBlock;   // grid_for counts workgroups of this size
constexpr int kMaxC = 32;

// (the index arithmetic of a vector is six divisions by run-time constants:
// FastDiv, common.h)
struct CmGeom {
  uint32_t total;                 // elements of hr
  uint32_t S1, S2, T, C;          // hr extents (n is implied)
  uint32_t L1, L2, TL, CL;        // lr extents
  uint32_t CM;                    // channels of mom1
  uint32_t te;
  uint32_t s_pad, t_lo, t_hi;     // mask box
  uint32_t flags;
  FastDiv dR, dC, dS2, dS1, ds, dte;   // by T*C, C, S2, S1, s_enhance, t_enhance
  int cmap[kMaxC];                // lr channel of every hr channel
};

// the (n, s1, s2) cell `row` of the hi-res batch: its low-res cell (as the
// offset of that cell's first time step, in cells) and whether it lies inside
// the spatial part of the mask box
__device__ __forceinline__ void row_info(const CmGeom& g, uint32_t row, uint32_t& lrrow,
                                         bool& sp_in) {
  const uint32_t q = g.dS2(row), j = row - q * g.S2;
  const uint32_t n = g.dS1(q), i = q - n * g.S1;
  lrrow = ((n * g.L1 + g.ds(i)) * g.L2 + g.ds(j)) * g.TL;
  sp_in = i >= g.s_pad && i + g.s_pad < g.S1 && j >= g.s_pad && j + g.s_pad < g.S2;
}

// v = hr -> v - e (subfilter) -> v - m (first moment) -> v * v (square); the
// single roundings are pinned so that no contraction can change a bit
__device__ __forceinline__ float target_value(const CmGeom& g, float h, float m, uint32_t lrrow,
                                              uint32_t k, uint32_t c,
                                              const float* __restrict__ lr) {
#pragma clang fp contract(off)
  float v = h;
  if (g.flags & S3_CM_SUBFILTER) {
    const float* p = lr + (size_t)lrrow * g.CL + g.cmap[c];
    float e;
    if (g.flags & S3_CM_LINEAR) {
      // between the landmarks i0 te and (i0 + 1) te; past the last one the
      // last segment is extended (interp1d(fill_value='extrapolate'))
      uint32_t i0 = g.dte(k);
      if (i0 > g.TL - 2) i0 = g.TL - 2;
      const float lo = p[(size_t)i0 * g.CL], hi = p[(size_t)(i0 + 1) * g.CL];
      const float frac = __fdiv_rn((float)(k - i0 * g.te), (float)g.te);
      e = __fadd_rn(lo, __fmul_rn(__fsub_rn(hi, lo), frac));
    } else {
      e = p[(size_t)g.dte(k) * g.CL];
    }
    v = __fsub_rn(v, e);
  }
  if (g.flags & S3_CM_MOM1) v = __fsub_rn(v, m);
  if (g.flags & S3_CM_SQUARE) v = __fmul_rn(v, v);
  return v;
}

// the first moment at element (row, k, c): mom1's channel c where it has one,
// the truth's own (exogenous) channel behind them
__device__ __forceinline__ float mom1_at(const CmGeom& g, const float* __restrict__ mom1, float h,
                                         uint32_t row, uint32_t k, uint32_t c) {
  return c < g.CM ? mom1[((size_t)row * g.T + k) * g.CM + c] : h;
}

__device__ __forceinline__ void one_element(const CmGeom& g, uint32_t e,
                                            const float* __restrict__ hr,
                                            const float* __restrict__ lr,
                                            const float* __restrict__ mom1,
                                            float* __restrict__ out, float* __restrict__ mask) {
  const uint32_t row = g.dR(e), r = e - row * (g.T * g.C);
  const uint32_t k = g.dC(r), c = r - k * g.C;
  uint32_t lrrow;
  bool sp_in;
  row_info(g, row, lrrow, sp_in);
  const float h = hr[e];
  if (out) {
    const float m = (g.flags & S3_CM_MOM1) ? mom1_at(g, mom1, h, row, k, c) : 0.f;
    out[e] = target_value(g, h, m, lrrow, k, c, lr);
  }
  if (mask) mask[e] = (sp_in && k >= g.t_lo && k < g.t_hi) ? 1.f : 0.f;
}

// four consecutive elements of the flat (n, s1, s2, t, c) order per lane: the
// position is decomposed once and carried element by element; the total % 4
// elements behind the last vector are done one by one by the first lanes
__global__ void __launch_bounds__(kBlk)
condmom_target_vec_kernel(CmGeom g, const float* __restrict__ hr, const float* __restrict__ lr,
                          const float* __restrict__ mom1, float* __restrict__ out,
                          float* __restrict__ mask) {
  const uint32_t nvec = g.total / 4;
  const uint32_t gid = blockIdx.x * kBlk + threadIdx.x, stride = gridDim.x * kBlk;
  const bool with_m = (g.flags & S3_CM_MOM1) != 0;
  const bool m_vec = with_m && g.CM == g.C;
  for (uint32_t v = gid; v < nvec; v += stride) {
    const uint32_t e0 = v * 4;
    uint32_t row = g.dR(e0);
    const uint32_t r = e0 - row * (g.T * g.C);
    uint32_t k = g.dC(r), c = r - k * g.C;
    uint32_t lrrow;
    bool sp_in;
    row_info(g, row, lrrow, sp_in);
    const float4 h4 = reinterpret_cast<const float4*>(hr)[v];
    float4 m4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (out && m_vec) m4 = reinterpret_cast<const float4*>(mom1)[v];
    const float h[4] = {h4.x, h4.y, h4.z, h4.w};
    const float mv[4] = {m4.x, m4.y, m4.z, m4.w};
    float o[4], mk[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (out) {
        float m = mv[q];
        if (with_m && !m_vec) m = mom1_at(g, mom1, h[q], row, k, c);
        o[q] = target_value(g, h[q], m, lrrow, k, c, lr);
      }
      mk[q] = (sp_in && k >= g.t_lo && k < g.t_hi) ? 1.f : 0.f;
      if (++c == g.C) {
        c = 0;
        if (++k == g.T) {
          k = 0;
          ++row;
          row_info(g, row, lrrow, sp_in);
        }
      }
    }
    if (out) reinterpret_cast<float4*>(out)[v] = make_float4(o[0], o[1], o[2], o[3]);
    if (mask) reinterpret_cast<float4*>(mask)[v] = make_float4(mk[0], mk[1], mk[2], mk[3]);
  }
  const uint32_t tail0 = nvec * 4;
  if (gid < g.total - tail0) one_element(g, tail0 + gid, hr, lr, mom1, out, mask);
}

// pointers that are not 16-byte aligned (views into a larger buffer)
__global__ void __launch_bounds__(kBlk)
condmom_target_scalar_kernel(CmGeom g, const float* __restrict__ hr, const float* __restrict__ lr,
                             const float* __restrict__ mom1, float* __restrict__ out,
                             float* __restrict__ mask) {
  for (uint32_t e = blockIdx.x * kBlk + threadIdx.x; e < g.total; e += gridDim.x * kBlk)
    one_element(g, e, hr, lr, mom1, out, mask);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

extern "C" int s3_condmom_target(s3_ctx* ctx, const float* hr, const float* lr, const float* mom1,
                                 int n, int s1, int s2, int t, int c_hr, int c_lr, int c_m,
                                 const int* lr_channel_host, int s_enhance, int t_enhance,
                                 unsigned flags, int s_pad, int t_lo, int t_hi, float* out,
                                 float* mask) {
  if (!ctx) return S3_EINVAL;
  if (!hr || (!out && !mask)) S3_FAIL(ctx, S3_EINVAL, "condmom_target: hr and one of out / mask are needed");
  if (n < 1 || s1 < 1 || s2 < 1 || t < 1 || c_hr < 1)
    S3_FAIL(ctx, S3_EINVAL, "condmom_target: empty hi-res batch");
  if (c_hr > kMaxC) S3_FAIL(ctx, S3_EINVAL, "condmom_target supports at most 32 channels");
  if (flags & ~(unsigned)(S3_CM_SUBFILTER | S3_CM_LINEAR | S3_CM_MOM1 | S3_CM_SQUARE))
    S3_FAIL(ctx, S3_EINVAL, "condmom_target: unknown flag bits");
  if (s_enhance < 1 || s1 % s_enhance || s2 % s_enhance)
    S3_FAIL(ctx, S3_EINVAL, "s_enhance must evenly divide grid size");
  const int te = t_enhance < 1 ? 1 : t_enhance;
  if (t % te) S3_FAIL(ctx, S3_EINVAL, "t_enhance must evenly divide the time axis");
  const int64_t total = (int64_t)n * s1 * s2 * t * c_hr;
  if (total >= ((int64_t)1 << 31)) S3_FAIL(ctx, S3_EINVAL, "condmom_target: 32-bit element indices");
  if (!out) flags = 0;                                // mask only: nothing else is read
  if (te == 1) flags &= ~(unsigned)S3_CM_LINEAR;      // temporal_simple_enhancing: data as it is
  CmGeom g;
  if (flags & S3_CM_SUBFILTER) {
    if (!lr || !lr_channel_host) S3_FAIL(ctx, S3_EINVAL, "condmom_target: subfilter needs lr and its channel map");
    if (c_lr < 1) S3_FAIL(ctx, S3_EINVAL, "condmom_target: lr has no channels");
    for (int i = 0; i < c_hr; ++i) {
      if (lr_channel_host[i] < 0 || lr_channel_host[i] >= c_lr)
        S3_FAIL(ctx, S3_EINVAL, "condmom_target: channel map entry outside the low-res channels");
      g.cmap[i] = lr_channel_host[i];
    }
    if ((flags & S3_CM_LINEAR) && t / te < 2)
      S3_FAIL(ctx, S3_EINVAL, "condmom_target: linear time mode needs two low-res time steps");
  } else {
    flags &= ~(unsigned)S3_CM_LINEAR;
    for (int i = 0; i < c_hr; ++i) g.cmap[i] = 0;
  }
  for (int i = c_hr; i < kMaxC; ++i) g.cmap[i] = 0;
  if (flags & S3_CM_MOM1) {
    if (!mom1) S3_FAIL(ctx, S3_EINVAL, "condmom_target: first-moment flag without mom1");
    if (c_m < 1 || c_m > c_hr)
      S3_FAIL(ctx, S3_EINVAL, "condmom_target: mom1 has more channels than the hi-res batch (or none)");
  }
  if (s_pad < 0) s_pad = 0;
  if (t_lo < 0) t_lo = 0;
  if (t_hi > t) t_hi = t;
  if (t_hi < t_lo) t_hi = t_lo;
  g.total = (uint32_t)total;
  g.S1 = s1; g.S2 = s2; g.T = t; g.C = c_hr;
  g.L1 = s1 / s_enhance; g.L2 = s2 / s_enhance; g.TL = t / te; g.CL = c_lr < 1 ? 1 : c_lr;
  g.CM = (flags & S3_CM_MOM1) ? c_m : c_hr;
  g.te = te;
  g.s_pad = s_pad; g.t_lo = t_lo; g.t_hi = t_hi;
  g.flags = flags;
  g.dR = FastDiv((uint32_t)t * c_hr); g.dC = FastDiv(c_hr);
  g.dS2 = FastDiv(s2); g.dS1 = FastDiv(s1);
  g.ds = FastDiv(s_enhance); g.dte = FastDiv(te);
  const bool vec = aligned16(hr) && aligned16(out) && aligned16(mask) &&
                   (!(flags & S3_CM_MOM1) || c_m != c_hr || aligned16(mom1));
  // memory bound: at most 8 workgroups per CU, the rest by grid stride
  const int64_t items = vec ? (total + 3) / 4 : total;
  const int grid = grid_for(items, ctx->num_cu);
  if (vec)
    hipLaunchKernelGGL(condmom_target_vec_kernel, dim3(grid), dim3(kBlk), 0, ctx->stream,
                       g, hr, lr, mom1, out, mask);
  else
    hipLaunchKernelGGL(condmom_target_scalar_kernel, dim3(grid), dim3(kBlk), 0,
                       ctx->stream, g, hr, lr, mom1, out, mask);
  S3_HIP(ctx, hipGetLastError());
  return S3_OK;
}
