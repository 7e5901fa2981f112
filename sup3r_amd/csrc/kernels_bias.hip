// Bias correction of forward-pass chunks on the device.
// ForwardPassStrategy.prep_chunk_data (sup3r/pipeline/strategy.py:502-517)
// corrects every chunk's low-res window on the host, feature by feature,
// through sup3r/bias/bias_transforms.py: the linear family (global_linear_bc
// :224-248, local_linear_bc :251-348, monthly_local_linear_bc :351-487) and
// quantile delta mapping (local_qdm_bc :622-824, local_presrat_bc :958-1137,
// whose per-site mapping is rex.utilities.bc_utils.QuantileDeltaMapping, a
// Python loop over sites).  Here that is ONE streaming pass over a batch of
// equal-shaped, already reflect-padded chunks (n, s1, s2, t, c):
//   * one wave per pixel (n, i, j): the pixel's contiguous (t, c) run is
//     loaded coalesced into the wave's slice of LDS, corrected there channel
//     by channel (the channel loop is wave-uniform: descriptors and table
//     bases live in scalar registers, the lanes run over time), and stored
//     back coalesced;
//   * the reference corrects the un-padded window and reflect-pads the result
//     (forward_pass.py:66-72,122-186); correcting the padded chunk with
//     MIRRORED factor indices gives the same values, so a pixel reads the table
//     row of the in-window pixel it mirrors;
//   * all lanes of a wave read the same table rows (one pixel, one channel,
//     one or two time windows): a row comes from HBM once and is reused from
//     the cache by that pixel's time steps;
//   * optionally the result is written normalised, (x - mean) / std, with the
//     arithmetic of s3_chunk_time_first (kernels_chunk_io.hip).
// Non-finite results are counted per channel: lanes count in a register, the
// wave sums by shuffles and issues one integer atomic — only if it met one.
// No float atomics.
#include "common.h"
#include "bias_qdm.h"

namespace {

constexpr int kBlk = 256;
constexpr int kWaves = kBlk / 64;
constexpr int kMaxC = S3_BC_MAX_CHANNELS;
constexpr int kMaxN = S3_BC_MAX_CHUNKS;
constexpr int kSeg = 1024;               // floats of LDS per wave

struct BcGeom {
  int n, s1, s2, t, c;
  int S1, S2;                            // extents of the domain tables
  int tseg;                              // time steps per LDS segment
  int norm;                              // 0 none, 1 fp32, 2 fp64
  int geo[kMaxN][6];                     // o1, o2, lo1, lo2, e1, e2 per chunk
  s3_bias_channel ch[kMaxC];
  float mean[kMaxC], sd[kMaxC];
  double dmean[kMaxC], dsd[kMaxC];
};

// index of np.pad(mode='reflect') into the un-padded extent e
__device__ __forceinline__ int reflect(int u, int e) {
  if (e <= 1) return 0;
  const int p = 2 * (e - 1);
  int m = u % p;
  if (m < 0) m += p;
  return m < e ? m : p - m;
}

__global__ void __launch_bounds__(kBlk)
bias_correct_kernel(BcGeom g, const float* x, float* out, const int* __restrict__ month,
                    const int* __restrict__ window, const double* __restrict__ weights,
                    int* __restrict__ nonfinite) {
#pragma clang fp contract(off)
  __shared__ float lds[kWaves][kSeg];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float* buf = lds[wave];
  const int npix = g.n * g.s1 * g.s2;
  const int pix = blockIdx.x * kWaves + wave;
  const bool active = pix < npix;            // (no early return: barriers below)
  const int pc = active ? pix : 0;
  const int k = pc / (g.s1 * g.s2);
  const int ij = pc - k * (g.s1 * g.s2);
  const int i = ij / g.s2, j = ij - i * g.s2;
  const int e1 = g.geo[k][4], e2 = g.geo[k][5];
  const int m1 = reflect(i - g.geo[k][2], e1), m2 = reflect(j - g.geo[k][3], e2);
  const size_t tp_dom = (size_t)(g.geo[k][0] + m1) * g.S2 + (g.geo[k][1] + m2);
  const size_t tp_own = (size_t)pc;          // per-chunk tables come padded like the chunk
  const size_t base = (size_t)pc * g.t * g.c;
  for (int t0 = 0; t0 < g.t; t0 += g.tseg) {
    const int nt = g.t - t0 < g.tseg ? g.t - t0 : g.tseg;
    const int cnt = nt * g.c;
    if (active)
      for (int e = lane; e < cnt; e += 64) buf[e] = x[base + (size_t)t0 * g.c + e];
    __syncthreads();
    if (active) {
      for (int c = 0; c < g.c; ++c) {
        const s3_bias_channel& d = g.ch[c];
        const size_t tp = (d.flags & S3_BC_GLOBAL) ? 0 : ((d.flags & S3_BC_PER_CHUNK) ? tp_own : tp_dom);
        float s_c = 1.f, a_c = 0.f;
        if (d.kind == S3_BC_LINEAR && !(d.flags & S3_BC_MONTH)) {
          if (d.flags & S3_BC_WEIGHTS) {
            // sum_m w_m table[i, j, m] over the months the chunk touches
            double s = 0.0, a = 0.0;
            for (int m = 0; m < d.n_t; ++m) {
              const double w = weights[k * d.n_t + m];
              if (w != 0.0) {
                s += w * (double)d.scalar[tp * d.n_t + m];
                a += w * (double)d.adder[tp * d.n_t + m];
              }
            }
            s_c = (float)s; a_c = (float)a;
          } else {
            s_c = d.scalar[tp * d.n_t];
            a_c = d.adder[tp * d.n_t];
          }
        }
        int bad = 0;
        for (int tt = lane; tt < nt; tt += 64) {
          const int tg = k * g.t + t0 + tt;
          float v = buf[tt * g.c + c];
          if (d.kind == S3_BC_LINEAR) {
            float s = s_c, a = a_c;
            if (d.flags & S3_BC_MONTH) {
              int m = month[tg];
              m = m < 0 ? 0 : (m >= d.n_t ? d.n_t - 1 : m);
              s = d.scalar[tp * d.n_t + m];
              a = d.adder[tp * d.n_t + m];
            }
            // bias_transforms.py:474-486
            if (d.flags & S3_BC_SCALAR_RANGE) s = np_max(np_min(s, d.scalar_hi), d.scalar_lo);
            if (d.flags & S3_BC_ADDER_RANGE) a = np_max(np_min(a, d.adder_hi), d.adder_lo);
            v = __fadd_rn(mul_rn(v, s), a);
          } else if (d.kind == S3_BC_QDM) {
            int w = window[tg];
            w = w < 0 ? 0 : (w >= d.n_t ? d.n_t - 1 : w);
            v = qdm_value(d, v, tp * d.n_t + w, tp);
          }
          if (d.kind != S3_BC_NONE) {
            if (d.flags & S3_BC_OUT_RANGE) v = np_min(np_max(v, d.out_lo), d.out_hi);
            // PresRat: NaN only (bias_transforms.py:1128), else NaN and inf (:816)
            if ((d.flags & S3_BC_PRESRAT) ? v != v : !(fabsf(v) <= 3.402823466e38f)) ++bad;
          }
          if (g.norm == 1) {
            v = __fdiv_rn(__fsub_rn(v, g.mean[c]), g.sd[c]);
          } else if (g.norm == 2) {
            v = (float)(((double)v - g.dmean[c]) / g.dsd[c]);
          }
          buf[tt * g.c + c] = v;
        }
        // one integer atomic per wave and channel, and only when there is something to count
        const unsigned long long any = __ballot(bad != 0);
        if (any) {
          for (int off = 32; off > 0; off >>= 1) bad += __shfl_down(bad, off, 64);
          if (lane == 0) atomicAdd(&nonfinite[c], bad);
        }
      }
    }
    __syncthreads();
    if (active)
      for (int e = lane; e < cnt; e += 64) out[base + (size_t)t0 * g.c + e] = buf[e];
    __syncthreads();
  }
}

}  // namespace

extern "C" int s3_bias_correct(s3_ctx* ctx, const float* x, int n, int s1, int s2, int t, int c,
                               const s3_bias_channel* channels_host, int S1, int S2,
                               const int32_t* geom_host, const int32_t* month, const int32_t* window,
                               const double* weights, const double* mean_host,
                               const double* std_host, int stats_fp32, float* out,
                               int32_t* nonfinite) {
  if (!ctx) return S3_EINVAL;
  if (!x || !out || !channels_host || !geom_host || !nonfinite)
    S3_FAIL(ctx, S3_EINVAL, "bias_correct: x, out, channels, geometry and the counters are needed");
  if (n < 1 || n > kMaxN) S3_FAIL(ctx, S3_EINVAL, "bias_correct: 1 .. 32 chunks per call");
  if (c < 1 || c > kMaxC) S3_FAIL(ctx, S3_EINVAL, "bias_correct: 1 .. 16 channels");
  if (s1 < 1 || s2 < 1 || t < 1) S3_FAIL(ctx, S3_EINVAL, "bias_correct: empty chunk");
  if ((int64_t)n * s1 * s2 * t * c >= ((int64_t)1 << 31) || (int64_t)n * s1 * s2 > (int64_t)1 << 30)
    S3_FAIL(ctx, S3_EINVAL, "bias_correct: 32-bit element indices");
  BcGeom g;
  g.n = n; g.s1 = s1; g.s2 = s2; g.t = t; g.c = c; g.S1 = S1; g.S2 = S2;
  g.tseg = kSeg / c;
  bool domain_tables = false;
  for (int i = 0; i < kMaxC; ++i) {
    s3_bias_channel d = {};
    if (i < c) d = channels_host[i];
    if (d.kind == S3_BC_LINEAR) {
      if (!d.scalar || !d.adder || d.n_t < 1)
        S3_FAIL(ctx, S3_EINVAL, "bias_correct: a linear channel needs scalar and adder tables");
      if ((d.flags & S3_BC_MONTH) && !month)
        S3_FAIL(ctx, S3_EINVAL, "bias_correct: per-step months without the month index");
      if ((d.flags & S3_BC_WEIGHTS) && !weights)
        S3_FAIL(ctx, S3_EINVAL, "bias_correct: month weights flagged but not given");
      if ((d.flags & S3_BC_MONTH) && (d.flags & S3_BC_WEIGHTS))
        S3_FAIL(ctx, S3_EINVAL, "bias_correct: per-step months and month weights exclude each other");
    } else if (d.kind == S3_BC_QDM) {
      if (!d.oh || !d.mh || (!d.mf && !(d.flags & S3_BC_NO_TREND)) || !window)
        S3_FAIL(ctx, S3_EINVAL, "bias_correct: a QDM channel needs its three tables and the window index");
      if (d.n_q < 2 || d.n_t < 1)
        S3_FAIL(ctx, S3_EINVAL, "bias_correct: QDM tables need two quantiles and one window");
      if ((d.flags & S3_BC_PRESRAT) && !(d.flags & S3_BC_NO_TREND) && (!d.tau || !d.kfac))
        S3_FAIL(ctx, S3_EINVAL, "bias_correct: PresRat needs tau_fut and k_factor");
    } else if (d.kind != S3_BC_NONE) {
      S3_FAIL(ctx, S3_EINVAL, "bias_correct: unknown channel kind");
    }
    if (d.kind != S3_BC_NONE && !(d.flags & (S3_BC_PER_CHUNK | S3_BC_GLOBAL))) domain_tables = true;
    g.ch[i] = d;
  }
  for (int k = 0; k < kMaxN; ++k)
    for (int q = 0; q < 6; ++q) g.geo[k][q] = k < n ? geom_host[k * 6 + q] : (q >= 4 ? 1 : 0);
  for (int k = 0; k < n; ++k) {
    const int* e = g.geo[k];
    if (e[2] < 0 || e[3] < 0 || e[4] < 1 || e[5] < 1 || e[2] + e[4] > s1 || e[3] + e[5] > s2)
      S3_FAIL(ctx, S3_EINVAL, "bias_correct: the un-padded window does not lie inside the padded chunk");
    if (domain_tables && (e[0] < 0 || e[1] < 0 || e[0] + e[4] > S1 || e[1] + e[5] > S2))
      S3_FAIL(ctx, S3_EINVAL, "bias_correct: a chunk window leaves the factor tables");
  }
  g.norm = (mean_host && std_host) ? (stats_fp32 ? 1 : 2) : 0;
  for (int i = 0; i < kMaxC; ++i) {
    const double m = g.norm && i < c ? mean_host[i] : 0.0, sd = g.norm && i < c ? std_host[i] : 1.0;
    g.mean[i] = (float)m; g.sd[i] = (float)sd; g.dmean[i] = m; g.dsd[i] = sd;
  }
  const int64_t npix = (int64_t)n * s1 * s2;
  const int64_t grid = (npix + kWaves - 1) / kWaves;
  hipLaunchKernelGGL(bias_correct_kernel, dim3((unsigned)grid), dim3(kBlk), 0, ctx->stream, g, x, out,
                     month, window, weights, nonfinite);
  S3_HIP(ctx, hipGetLastError());
  return S3_OK;
}
