// Training samples cut out of a data cube that lives on the device.
// Sampler.__next__ (sup3r/preprocessing/samplers/base.py:228-262) slices every
// batch out of its container on the host — one box of batch_size * t time
// steps that is reshaped (_fast_batch), or batch_size independent boxes that
// are stacked (_slow_batch) — and the queue then uploads the batch.  Here the
// container is a resident (S1, S2, T, C) cube and either kind of batch is one
// gather
//   out[m, i, j, k, q] = data[i0[m] + i, j0[m] + j, k0[m] + k, channel[q]]
// whose origins and channel map ride in the kernel arguments: nothing is
// uploaded, nothing synchronises.
// The contiguous unit of the source is one pixel's run of t * C floats, which
// starts k0 * C floats into the pixel: 4-byte aligned, no more.  The unit of the
// destination is t * c_out floats, and the destination as a whole is one
// contiguous array.  Two kernels:
//   * runs of kLongRun floats or more: a wave per pixel.  The run is loaded into
//     the wave's slice of LDS with 16-byte loads between a peeled head and tail
//     (the slice is shifted so that the aligned part of the run lands 16-byte
//     aligned in LDS too), the channels are picked while reading LDS, and the
//     pixel's destination run is stored with 16-byte stores between a head and
//     tail of its own;
//   * shorter runs (t = 1: C floats per pixel, pitch T * C): a lane per four
//     consecutive floats of the DESTINATION, so that a wave stores 1 KiB in
//     one piece however the loads scatter; the position is decomposed once per
//     lane and carried from element to element.
// A pure copy: no arithmetic touches a value, NaN payloads arrive as they are.
// s3_cc_window_gather is the second kernel with one more step: its boxes are
// 24-hour windows and the t hours it keeps start where the night mask that
// s3_cc_night_mask (kernels_cc.hip) left on the device says.
#include "common.h"

namespace {

constexpr int kBlk = kBlock;   // grid_for counts workgroups of this size
constexpr int kWaves = kBlk / 64;
constexpr int kMaxN = S3_SAMPLE_MAX_ORIGINS;
constexpr int kMaxC = S3_SAMPLE_MAX_CHANNELS;
constexpr int kSeg = 2048;               // floats of a run staged per pass
constexpr int kSlice = kSeg + 4;         // ... + room for the alignment shift
constexpr int kLongRun = 128;            // floats; below: the short-run kernel
constexpr int kLongMaxC = 256;           // a staged pass holds >= 8 time steps

struct SgGeom {
  int64_t S2, TC;                        // cube: columns, floats per pixel (T * C)
  uint32_t s1, s2, t, C, c_out;          // box extents, cube channels, channels kept
  uint32_t npix;                         // n * s1 * s2 of THIS launch
  uint32_t total;                        // npix * t * c_out
  uint32_t tseg;                         // time steps per staged pass
  uint32_t identity;                     // channel map is 0 .. C - 1
  FastDiv dRun, dCo, dS2, dS1;           // by t * c_out, c_out, s2, s1
  int org[kMaxN][3];                     // i0, j0, k0 per sample
  int ch[kMaxC];
};

// floats from `data` to the first float the box of sample m keeps of pixel
// (i, j): 64-bit, cubes are larger than 2^31 elements
__device__ __forceinline__ int64_t pixel_offset(const SgGeom& g, uint32_t m, uint32_t i, uint32_t j) {
  return ((int64_t)(g.org[m][0] + (int)i) * g.S2 + (g.org[m][1] + (int)j)) * g.TC +
         (int64_t)g.org[m][2] * g.C;
}

__device__ __forceinline__ uint32_t to_align16(const void* p) {
  return (uint32_t)((4u - (((uintptr_t)p >> 2) & 3u)) & 3u);   // floats up to the next 16-byte line
}

__global__ void __launch_bounds__(kBlk)
sample_gather_long_kernel(SgGeom g, const float* __restrict__ data, float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float lds[kWaves][kSlice];
  __shared__ int s_ch[kMaxC];
  if (threadIdx.x < kMaxC) s_ch[threadIdx.x] = g.ch[threadIdx.x];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float* buf = lds[wave];
  const uint32_t pix = blockIdx.x * kWaves + wave;
  const bool active = pix < g.npix;          // (no early return: barriers below)
  const uint32_t pc = active ? pix : 0;
  const uint32_t mi = g.dS2(pc), j = pc - mi * g.s2;
  const uint32_t m = g.dS1(mi), i = mi - m * g.s1;
  const float* src_pix = data + pixel_offset(g, m, i, j);
  float* dst_pix = out + (size_t)pc * g.t * g.c_out;
  __syncthreads();
  for (uint32_t t0 = 0; t0 < g.t; t0 += g.tseg) {
    const uint32_t nt = g.t - t0 < g.tseg ? g.t - t0 : g.tseg;
    const uint32_t cnt = nt * g.C;
    const float* src = src_pix + (size_t)t0 * g.C;
    uint32_t head = to_align16(src);
    if (head > cnt) head = cnt;
    const uint32_t shift = (4u - head) & 3u;       // buf + shift + head is a 16-byte line
    if (active) {
      if (lane < head) buf[shift + lane] = src[lane];
      const uint32_t nv = (cnt - head) >> 2;
      const float4* src4 = reinterpret_cast<const float4*>(src + head);
      float4* buf4 = reinterpret_cast<float4*>(buf + shift + head);
      uint32_t v = lane;
      for (; v + 192 < nv; v += 256) {             // four loads in flight per lane
        const float4 a = src4[v], b = src4[v + 64], c = src4[v + 128], d = src4[v + 192];
        buf4[v] = a; buf4[v + 64] = b; buf4[v + 128] = c; buf4[v + 192] = d;
      }
      for (; v < nv; v += 64) buf4[v] = src4[v];
      const uint32_t done = head + nv * 4;
      if (lane < cnt - done) buf[shift + done + lane] = src[done + lane];
    }
    __syncthreads();
    if (active) {
      const float* run = buf + shift;
      float* dst = dst_pix + (size_t)t0 * g.c_out;
      const uint32_t cnt_o = nt * g.c_out;
      uint32_t head_o = to_align16(dst);
      if (head_o > cnt_o) head_o = cnt_o;
      const uint32_t nv = (cnt_o - head_o) >> 2;
      const uint32_t done = head_o + nv * 4;
      if (g.identity) {
        if (lane < head_o) dst[lane] = run[lane];
        for (uint32_t v = lane; v < nv; v += 64) {
          const float* r = run + head_o + v * 4;
          reinterpret_cast<float4*>(dst + head_o)[v] = make_float4(r[0], r[1], r[2], r[3]);
        }
        if (lane < cnt_o - done) dst[done + lane] = run[done + lane];
      } else {
        // element e of the destination run is time step e / c_out, kept channel e % c_out
        if (lane < head_o) {
          const uint32_t k = g.dCo(lane), q = lane - k * g.c_out;
          dst[lane] = run[k * g.C + s_ch[q]];
        }
        for (uint32_t v = lane; v < nv; v += 64) {
          const uint32_t e = head_o + v * 4;
          uint32_t k = g.dCo(e), q = e - k * g.c_out;
          float o[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            o[u] = run[k * g.C + s_ch[q]];
            if (++q == g.c_out) { q = 0; ++k; }
          }
          reinterpret_cast<float4*>(dst + head_o)[v] = make_float4(o[0], o[1], o[2], o[3]);
        }
        if (lane < cnt_o - done) {
          const uint32_t e = done + lane;
          const uint32_t k = g.dCo(e), q = e - k * g.c_out;
          dst[e] = run[k * g.C + s_ch[q]];
        }
      }
    }
    __syncthreads();
  }
}

// where element e of the destination comes from
__device__ __forceinline__ void decompose(const SgGeom& g, uint32_t e, uint32_t& m, uint32_t& i,
                                          uint32_t& j, uint32_t& k, uint32_t& q) {
  const uint32_t pix = g.dRun(e), r = e - pix * (g.t * g.c_out);
  k = g.dCo(r); q = r - k * g.c_out;
  const uint32_t mi = g.dS2(pix);
  j = pix - mi * g.s2;
  m = g.dS1(mi); i = mi - m * g.s1;
}

// first hour kept of a 24-hour window whose night hours are the set bits of
// `mask` (nsrdb_reduce_daily_data, samplers/utilities.py:281-297): the first
// daylight hour minus half of what t exceeds the daylight hours by, the half
// rounded towards +inf; `raw` is that start as the reference computes it.
// Deviations (include/sup3r_hip.h): the start is clamped into [0, 24 - t], and
// 24 hours of night give the centred window.
__device__ __forceinline__ int window_start(unsigned mask, int t, int& raw) {
  const unsigned day = ~mask & 0xFFFFFFu;
  if (day == 0) return raw = (24 - t) / 2;
  const int pad = t - __popc(day);
  const int half = pad >= 0 ? (pad + 1) / 2 : -((-pad) / 2);
  raw = (__ffs((int)day) - 1) - half;
  return raw < 0 ? 0 : raw > 24 - t ? 24 - t : raw;
}

// WIN: the boxes are 24-hour windows and the copy starts window_start() hours
// into them, computed by every workgroup from the night mask in status[0]
template <bool VEC, bool WIN>
__global__ void __launch_bounds__(kBlk)
sample_gather_short_kernel(SgGeom g, const float* __restrict__ data, float* __restrict__ out,
                           int* __restrict__ status) {
  __shared__ int s_ch[kMaxC];
  __shared__ int s_start;
  if (threadIdx.x < kMaxC) s_ch[threadIdx.x] = g.ch[threadIdx.x];
  if (WIN && threadIdx.x == 0) {
    int raw;
    s_start = window_start((unsigned)status[S3_CC_NIGHT_MASK], (int)g.t, raw);
    if (blockIdx.x == 0) { status[S3_CC_START_RAW] = raw; status[S3_CC_START] = s_start; }
  }
  __syncthreads();
  if (WIN) data += (int64_t)s_start * g.C;
  const uint32_t gid = blockIdx.x * kBlk + threadIdx.x, stride = gridDim.x * kBlk;
  uint32_t m, i, j, k, q;
  if (VEC) {
    const uint32_t nvec = g.total / 4;
    for (uint32_t v = gid; v < nvec; v += stride) {
      decompose(g, v * 4, m, i, j, k, q);
      const float* src = data + pixel_offset(g, m, i, j);
      float o[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        o[u] = src[(size_t)k * g.C + s_ch[q]];
        if (++q == g.c_out) {
          q = 0;
          if (++k == g.t) {
            k = 0;
            if (++j == g.s2) {
              j = 0;
              if (++i == g.s1) { i = 0; ++m; }
            }
            if (u < 3) src = data + pixel_offset(g, m, i, j);   // (a next element exists: m < n)
          }
        }
      }
      reinterpret_cast<float4*>(out)[v] = make_float4(o[0], o[1], o[2], o[3]);
    }
    const uint32_t tail0 = nvec * 4;
    if (gid < g.total - tail0) {
      decompose(g, tail0 + gid, m, i, j, k, q);
      out[tail0 + gid] = data[pixel_offset(g, m, i, j) + (int64_t)k * g.C + s_ch[q]];
    }
  } else {
    // a destination that is not 16-byte aligned (a view into a larger buffer)
    for (uint32_t e = gid; e < g.total; e += stride) {
      decompose(g, e, m, i, j, k, q);
      out[e] = data[pixel_offset(g, m, i, j) + (int64_t)k * g.C + s_ch[q]];
    }
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

// status == nullptr: s3_sample_gather.  Otherwise s3_cc_window_gather: the
// boxes that must fit the cube are the 24-hour windows
static int gather_impl(s3_ctx* ctx, const char* who, const float* data, int64_t S1, int64_t S2, int64_t T,
                       int C, const int* origins_host, int n, int s1, int s2, int t,
                       const int* channel_host, int c_out, int* status, float* out) {
  const bool win = status != nullptr;
  const int t_box = win ? 24 : t;
  if (!data || !out || !origins_host || !channel_host)
    S3_FAIL(ctx, S3_EINVAL, std::string(who) + ": data, out, the origins and the channel map are needed");
  if (S1 < 1 || S2 < 1 || T < 1 || C < 1) S3_FAIL(ctx, S3_EINVAL, std::string(who) + ": empty cube");
  if (n < 1 || s1 < 1 || s2 < 1 || t < 1) S3_FAIL(ctx, S3_EINVAL, std::string(who) + ": empty batch");
  if (c_out < 1 || c_out > kMaxC) S3_FAIL(ctx, S3_EINVAL, std::string(who) + ": 1 .. 32 channels are kept");
  if (win && t >= 24)
    S3_FAIL(ctx, S3_EINVAL, std::string(who) + ": 1 .. 23 hours are kept of a 24-hour window");
  if (s1 > S1 || s2 > S2 || t_box > T) S3_FAIL(ctx, S3_EINVAL, std::string(who) + ": the box is larger than the cube");
  if (T > INT32_MAX || S1 > INT32_MAX || S2 > INT32_MAX)
    S3_FAIL(ctx, S3_EINVAL, std::string(who) + ": 32-bit cube extents (offsets are 64-bit)");
  bool identity = c_out == C;
  for (int q = 0; q < c_out; ++q) {
    if (channel_host[q] < 0 || channel_host[q] >= C)
      S3_FAIL(ctx, S3_EINVAL, std::string(who) + ": channel map entry outside the cube's channels");
    identity = identity && channel_host[q] == q;
  }
  for (int m = 0; m < n; ++m) {
    const int* o = origins_host + (size_t)m * 3;
    if (o[0] < 0 || o[1] < 0 || o[2] < 0 || o[0] > S1 - s1 || o[1] > S2 - s2 || o[2] > T - t_box)
      S3_FAIL(ctx, S3_EINVAL, std::string(who) + ": a box leaves the cube");
  }
  const int64_t per_sample = (int64_t)s1 * s2 * t * c_out;
  if (per_sample >= ((int64_t)1 << 31) || per_sample * n >= ((int64_t)1 << 31))
    S3_FAIL(ctx, S3_EINVAL, std::string(who) + ": 32-bit element indices of out");
  SgGeom g;
  g.S2 = S2; g.TC = T * C;
  g.s1 = s1; g.s2 = s2; g.t = t; g.C = C; g.c_out = c_out;
  g.identity = identity ? 1u : 0u;
  g.dRun = FastDiv((uint32_t)t * c_out); g.dCo = FastDiv(c_out);
  g.dS2 = FastDiv(s2); g.dS1 = FastDiv(s1);
  for (int q = 0; q < kMaxC; ++q) g.ch[q] = q < c_out ? channel_host[q] : 0;
  const bool long_runs = !win && (int64_t)t * C >= kLongRun && C <= kLongMaxC;
  g.tseg = long_runs ? kSeg / C : 1;
  for (int m0 = 0; m0 < n; m0 += kMaxN) {
    const int nl = n - m0 < kMaxN ? n - m0 : kMaxN;
    for (int m = 0; m < kMaxN; ++m)
      for (int a = 0; a < 3; ++a) g.org[m][a] = m < nl ? origins_host[(size_t)(m0 + m) * 3 + a] : 0;
    g.npix = (uint32_t)((int64_t)nl * s1 * s2);
    g.total = (uint32_t)(per_sample * nl);
    float* dst = out + per_sample * m0;
    if (long_runs) {
      const unsigned grid = (g.npix + kWaves - 1) / kWaves;
      hipLaunchKernelGGL(sample_gather_long_kernel, dim3(grid), dim3(kBlk), 0, ctx->stream, g, data, dst);
    } else {
      // memory bound: at most 8 workgroups per CU, the rest by grid stride
      const bool vec = aligned16(dst);
      const int64_t items = vec ? ((int64_t)g.total + 3) / 4 : (int64_t)g.total;
      const int grid = grid_for(items, ctx->num_cu);
      auto kernel = win ? (vec ? sample_gather_short_kernel<true, true> : sample_gather_short_kernel<false, true>)
                        : (vec ? sample_gather_short_kernel<true, false> : sample_gather_short_kernel<false, false>);
      hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlk), 0, ctx->stream, g, data, dst, status);
    }
    S3_HIP(ctx, hipGetLastError());
  }
  return S3_OK;
}

extern "C" int s3_sample_gather(s3_ctx* ctx, const float* data, int64_t S1, int64_t S2, int64_t T,
                                int C, const int* origins_host, int n, int s1, int s2, int t,
                                const int* channel_host, int c_out, float* out) {
  if (!ctx) return S3_EINVAL;
  return gather_impl(ctx, "sample_gather", data, S1, S2, T, C, origins_host, n, s1, s2, t, channel_host, c_out,
                     nullptr, out);
}

extern "C" int s3_cc_window_gather(s3_ctx* ctx, const float* data, int64_t S1, int64_t S2, int64_t T,
                                   int C, const int* origins_host, int n, int s1, int s2, int t,
                                   const int* channel_host, int c_out, int* status, float* out) {
  if (!ctx) return S3_EINVAL;
  if (!status) S3_FAIL(ctx, S3_EINVAL, "s3_cc_window_gather: the status words are needed");
  return gather_impl(ctx, "s3_cc_window_gather", data, S1, S2, T, C, origins_host, n, s1, s2, t, channel_host,
                     c_out, status, out);
}
