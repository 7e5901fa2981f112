// Index-permutation ops of the Sup3rGan path (temporal nearest repeat,
// depth-to-space, pad, crop, roll, dilate, concat) and their adjoints; the
// adjoint of a pad over a whole frame is the FOLD of a conv's padded-frame data
// gradient, with the variants launch_fold chooses between.  One-pass streaming
// kernels: coalesced 16-B accesses where the channel count allows.
#include "kernels_support.h"
#include "wave_prims.h"

namespace {

// ------------------------------------------------------------------ gather
// out[n, o0, o1, o2, c] = in[map(...)]; V = channels per thread (1 or 4)
template <int V, typename T>
__global__ void gather_kernel(const T* __restrict__ in, T* __restrict__ out,
                              GatherGeom g) {
  const int cg_out = g.Co / V;
  const int64_t total = (int64_t)g.N * g.Do[0] * g.Do[1] * g.Do[2] * cg_out;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    int64_t r = idx;
    int cg = (int)(r % cg_out); r /= cg_out;
    int o2 = (int)(r % g.Do[2]); r /= g.Do[2];
    int o1 = (int)(r % g.Do[1]); r /= g.Do[1];
    int o0 = (int)(r % g.Do[0]); r /= g.Do[0];
    int n = (int)r;
    int c = cg * V;
    int i0 = o0, i1 = o1, i2 = o2, ci = c;
    bool zero = false;
    int64_t out_c = c;
    switch (g.kind) {
      case S3_OP_REPEAT_T: i2 = o2 / g.rep; break;
      case S3_OP_ROLL_T: {
        int s = g.rep % g.Do[2]; if (s < 0) s += g.Do[2];   // tf.roll: any sign
        i2 = o2 - s; if (i2 < 0) i2 += g.Do[2];
      } break;
      case S3_OP_D2S: {
        int b = g.d2s;
        i0 = o0 / b; i1 = o1 / b;
        ci = ((o0 % b) * b + (o1 % b)) * g.Co + c;
      } break;
      case S3_OP_CROP: i0 = o0 + g.lo[0]; i1 = o1 + g.lo[1]; i2 = o2 + g.lo[2]; break;
      case S3_OP_DILATE:   // lo[] = stride: out[i s] = in[i], zeros in between
        zero = (o0 % g.lo[0]) || (o1 % g.lo[1]) || (o2 % g.lo[2]);
        i0 = o0 / g.lo[0]; i1 = o1 / g.lo[1]; i2 = o2 / g.lo[2];
        break;
      case S3_OP_PAD: {
        i0 = o0 - g.lo[0]; i1 = o1 - g.lo[1]; i2 = o2 - g.lo[2];
        if (g.pad_mode == S3_PAD_REFLECT) {
          i0 = s3_reflect(i0, g.Di[0]); i1 = s3_reflect(i1, g.Di[1]);
          i2 = s3_reflect(i2, g.Di[2]);
        } else {
          zero = i0 < 0 || i0 >= g.Di[0] || i1 < 0 || i1 >= g.Di[1] ||
                 i2 < 0 || i2 >= g.Di[2];
        }
      } break;
      case S3_OP_CONCAT: {
        // thread indexes the INPUT channel range; output channel is offset
        // (Do == Di, Co here is the number of channels copied)
        out_c = c + g.c_off;
      } break;
      default: break;
    }
    int64_t src = ((((int64_t)n * g.Di[0] + i0) * g.Di[1] + i1) * g.Di[2] + i2) *
                      g.Ci + ci;
    int co_total = (g.kind == S3_OP_CONCAT) ? g.rep : g.Co;  // rep = C of out
    int64_t dst = ((((int64_t)n * g.Do[0] + o0) * g.Do[1] + o1) * g.Do[2] + o2) *
                      co_total + out_c;
    if (V * sizeof(T) == 16) {
      uint4 v = zero ? make_uint4(0, 0, 0, 0)
                     : *reinterpret_cast<const uint4*>(in + src);
      *reinterpret_cast<uint4*>(out + dst) = v;
    } else {
      out[dst] = zero ? (T)0 : in[src];
    }
  }
}

// backward of the gather ops: one thread per din element (gathers its
// pre-images from dout; no atomics, deterministic)
__global__ void gather_bwd_kernel(const float* __restrict__ dout,
                                  float* __restrict__ din, GatherGeom g) {
  const int64_t total = (int64_t)g.N * g.Di[0] * g.Di[1] * g.Di[2] * g.Ci;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    int64_t r = idx;
    int c = (int)(r % g.Ci); r /= g.Ci;
    int i2 = (int)(r % g.Di[2]); r /= g.Di[2];
    int i1 = (int)(r % g.Di[1]); r /= g.Di[1];
    int i0 = (int)(r % g.Di[0]); r /= g.Di[0];
    int n = (int)r;
    auto at = [&](int o0, int o1, int o2, int co, int ctot) -> float {
      return dout[((((int64_t)n * g.Do[0] + o0) * g.Do[1] + o1) * g.Do[2] + o2) *
                      ctot + co];
    };
    float acc = 0.f;
    switch (g.kind) {
      case S3_OP_REPEAT_T:
        for (int j = 0; j < g.rep; ++j) acc += at(i0, i1, i2 * g.rep + j, c, g.Co);
        break;
      case S3_OP_ROLL_T: {
        int s = g.rep % g.Do[2]; if (s < 0) s += g.Do[2];
        int o2 = i2 + s; if (o2 >= g.Do[2]) o2 -= g.Do[2];
        acc = at(i0, i1, o2, c, g.Co);
      } break;
      case S3_OP_D2S: {
        int b = g.d2s;
        int blk = c / g.Co, co = c % g.Co;
        acc = at(i0 * b + blk / b, i1 * b + blk % b, i2, co, g.Co);
      } break;
      case S3_OP_CROP: {
        int o0 = i0 - g.lo[0], o1 = i1 - g.lo[1], o2 = i2 - g.lo[2];
        if (o0 >= 0 && o0 < g.Do[0] && o1 >= 0 && o1 < g.Do[1] && o2 >= 0 &&
            o2 < g.Do[2])
          acc = at(o0, o1, o2, c, g.Co);
      } break;
      case S3_OP_PAD: {
        // pre-images of i under reflect: i+lo, lo-i (1<=i<=lo), and the
        // mirror about the far edge
        int cand[3][3], cnt[3];
        const int ii[3] = {i0, i1, i2};
        for (int d = 0; d < 3; ++d) {
          int nI = g.Di[d], lo = g.lo[d], nO = g.Do[d];
          cnt[d] = 0;
          cand[d][cnt[d]++] = ii[d] + lo;
          if (g.pad_mode == S3_PAD_REFLECT) {
            if (ii[d] >= 1 && ii[d] <= lo) cand[d][cnt[d]++] = lo - ii[d];
            int m = 2 * (nI - 1) - ii[d] + lo;  // mirrored padded index
            if (ii[d] <= nI - 2 && m < nO && m >= nI + lo) cand[d][cnt[d]++] = m;
          }
        }
        for (int a = 0; a < cnt[0]; ++a)
          for (int b = 0; b < cnt[1]; ++b)
            for (int e = 0; e < cnt[2]; ++e)
              acc += at(cand[0][a], cand[1][b], cand[2][e], c, g.Co);
      } break;
      case S3_OP_DILATE:
        acc = at(i0 * g.lo[0], i1 * g.lo[1], i2 * g.lo[2], c, g.Co);
        break;
      case S3_OP_CONCAT:
        acc = at(i0, i1, i2, c + g.c_off, g.rep);
        break;
      default: break;
    }
    din[idx] = acc;
  }
}

// fold of a reflect / zero padded frame (adjoint of S3_OP_PAD) on float4
// channel groups: the index math of a cell is shared by 4 channels
// MASK: 0 none, 1 fp32 y, 2 bf16 y — multiplies by the activation adjoint of the
// conv that produced the folded tensor (y = act(pre): 1 where y > 0, else slope);
// 3: mask_y is an fp32 tensor ADDED to the fold (an earlier gradient contribution)
// OUT16: the folded tensor is stored as bf16 ONLY (din is then an unsigned
// short buffer): dPre of a conv whose data / weight gradient kernels take bf16
// and whose bias gradient rides along in bsum — nothing reads it as fp32
// SIDE16: fp32 store to din AND a bf16 copy to side16 (a tensor that stays
// fp32 for the skip path but whose producer conv stages bf16)
// FR16: the frame `dout` is stored as bf16 (round 4: the persistent data
// gradient kernel writes its padded frame that way — half the round trip)
template <int MASK, bool OUT16 = false, bool SIDE16 = false, bool FR16 = false>
__global__ void gather_bwd_pad4_kernel(const float* __restrict__ dout,
                                       float* __restrict__ din, GatherGeom g,
                                       const void* __restrict__ mask_y, float slope,
                                       float* __restrict__ bsum,
                                       unsigned short* __restrict__ side16 = nullptr) {
  // bsum (nullable, needs c4n | 256): per-workgroup channel sums of the stored
  // values, partial[block][Ci] — the bias gradient of the conv that produced
  // the folded tensor, for bias_grad_stage2 (a lane keeps one channel group:
  // the grid stride is a multiple of c4n)
  float4 bs = make_float4(0.f, 0.f, 0.f, 0.f);
  const int c4n = g.Ci >> 2;
  const int64_t total = (int64_t)g.N * g.Di[0] * g.Di[1] * g.Di[2] * c4n;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    // (32-bit divisions whenever the element count allows: the 64-bit ones
    // cost more than the memory traffic of this kernel)
    int c4, i2, i1, i0, n;
    if (total <= 0x7fffffffLL) {
      unsigned r = (unsigned)idx, q;
      q = r / (unsigned)c4n; c4 = (int)(r - q * (unsigned)c4n); r = q;
      q = r / (unsigned)g.Di[2]; i2 = (int)(r - q * (unsigned)g.Di[2]); r = q;
      q = r / (unsigned)g.Di[1]; i1 = (int)(r - q * (unsigned)g.Di[1]); r = q;
      q = r / (unsigned)g.Di[0]; i0 = (int)(r - q * (unsigned)g.Di[0]); n = (int)q;
    } else {
      int64_t r = idx;
      c4 = (int)(r % c4n); r /= c4n;
      i2 = (int)(r % g.Di[2]); r /= g.Di[2];
      i1 = (int)(r % g.Di[1]); r /= g.Di[1];
      i0 = (int)(r % g.Di[0]); r /= g.Di[0];
      n = (int)r;
    }
    int cand[3][3], cnt[3];
    const int ii[3] = {i0, i1, i2};
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const int nI = g.Di[d], lo = g.lo[d], nO = g.Do[d];
      cnt[d] = 0;
      cand[d][cnt[d]++] = ii[d] + lo;
      if (g.pad_mode == S3_PAD_REFLECT) {
        if (ii[d] >= 1 && ii[d] <= lo) cand[d][cnt[d]++] = lo - ii[d];
        const int m = 2 * (nI - 1) - ii[d] + lo;
        if (ii[d] <= nI - 2 && m < nO && m >= nI + lo) cand[d][cnt[d]++] = m;
      }
    }
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int a = 0; a < cnt[0]; ++a)
      for (int b = 0; b < cnt[1]; ++b)
        for (int e = 0; e < cnt[2]; ++e) {
          const int64_t fo = ((((int64_t)n * g.Do[0] + cand[0][a]) * g.Do[1] + cand[1][b]) * g.Do[2] +
                              cand[2][e]) * g.Co + c4 * 4;
          float4 v;
          if constexpr (FR16) {
            const uint2 h = *reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned short*>(dout) + fo);
            v = make_float4(__uint_as_float(h.x << 16), __uint_as_float(h.x & 0xFFFF0000u),
                            __uint_as_float(h.y << 16), __uint_as_float(h.y & 0xFFFF0000u));
          } else {
            v = *reinterpret_cast<const float4*>(dout + fo);
          }
          acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
        }
    if (MASK == 1) {
      const float4 y = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(mask_y) + idx * 4);
      acc.x *= y.x > 0.f ? 1.f : slope; acc.y *= y.y > 0.f ? 1.f : slope;
      acc.z *= y.z > 0.f ? 1.f : slope; acc.w *= y.w > 0.f ? 1.f : slope;
    } else if (MASK == 2) {
      // bf16: the sign bit is bit 15 of each half word; zero is not > 0
      const uint2 y = *reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned short*>(mask_y) + idx * 4);
      auto pos = [](unsigned h) { return (h & 0x8000u) == 0 && (h & 0x7FFFu) != 0; };
      acc.x *= pos(y.x & 0xFFFFu) ? 1.f : slope; acc.y *= pos(y.x >> 16) ? 1.f : slope;
      acc.z *= pos(y.y & 0xFFFFu) ? 1.f : slope; acc.w *= pos(y.y >> 16) ? 1.f : slope;
    }
    if (MASK == 3) {
      const float4 y = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(mask_y) + idx * 4);
      acc.x += y.x; acc.y += y.y; acc.z += y.z; acc.w += y.w;
    }
    if constexpr (OUT16) {
      *reinterpret_cast<uint2*>(reinterpret_cast<unsigned short*>(din) + idx * 4) =
          make_uint2(pk2(acc.x, acc.y), pk2(acc.z, acc.w));
    } else {
      *reinterpret_cast<float4*>(din + idx * 4) = acc;
      if constexpr (SIDE16)
        *reinterpret_cast<uint2*>(side16 + idx * 4) = make_uint2(pk2(acc.x, acc.y), pk2(acc.z, acc.w));
    }
    bs.x += acc.x; bs.y += acc.y; bs.z += acc.z; bs.w += acc.w;
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

// The bf16-frame fold on EIGHT channels per lane (C % 8 == 0): with the 4-wide
// walk above a lane moved 8 B per frame cell and the index arithmetic (four
// divisions, up to eight candidate cells) set the pace — the masked fold ran
// 246 MB in 69 us where the fp32 frame's 342 MB had taken 70.  16-B loads of
// the frame / the bf16 mask, 16-B bf16 stores, half the index math per byte.
// Same MASK / OUT16 / SIDE16 meaning and the same bsum layout
// (partial[block][C]); launched with the 4-wide walk's grid so that the
// consumers of bsum see the block count they expect.
template <int MASK, bool OUT16, bool SIDE16>
__global__ void fold16x8_kernel(const unsigned short* __restrict__ frame, float* __restrict__ din,
                                GatherGeom g, const void* __restrict__ mask_y, float slope,
                                float* __restrict__ bsum, unsigned short* __restrict__ side16) {
  float bs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const int c8n = g.Ci >> 3;
  const int64_t total = (int64_t)g.N * g.Di[0] * g.Di[1] * g.Di[2] * c8n;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    unsigned r = (unsigned)idx, q;           // (launcher: total < 2^31)
    q = r / (unsigned)c8n; const int c8 = (int)(r - q * (unsigned)c8n); r = q;
    q = r / (unsigned)g.Di[2]; const int i2 = (int)(r - q * (unsigned)g.Di[2]); r = q;
    q = r / (unsigned)g.Di[1]; const int i1 = (int)(r - q * (unsigned)g.Di[1]); r = q;
    q = r / (unsigned)g.Di[0]; const int i0 = (int)(r - q * (unsigned)g.Di[0]);
    const int n = (int)q;
    int cand[3][3], cnt[3];
    const int ii[3] = {i0, i1, i2};
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const int nI = g.Di[d], lo = g.lo[d], nO = g.Do[d];
      cnt[d] = 0;
      cand[d][cnt[d]++] = ii[d] + lo;
      if (g.pad_mode == S3_PAD_REFLECT) {
        if (ii[d] >= 1 && ii[d] <= lo) cand[d][cnt[d]++] = lo - ii[d];
        const int m = 2 * (nI - 1) - ii[d] + lo;
        if (ii[d] <= nI - 2 && m < nO && m >= nI + lo) cand[d][cnt[d]++] = m;
      }
    }
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int a = 0; a < cnt[0]; ++a)
      for (int b = 0; b < cnt[1]; ++b)
        for (int e = 0; e < cnt[2]; ++e) {
          const int64_t fo = ((((int64_t)n * g.Do[0] + cand[0][a]) * g.Do[1] + cand[1][b]) * g.Do[2] +
                              cand[2][e]) * g.Co + c8 * 8;
          const uint4 h = *reinterpret_cast<const uint4*>(frame + fo);
          acc[0] += __uint_as_float(h.x << 16); acc[1] += __uint_as_float(h.x & 0xFFFF0000u);
          acc[2] += __uint_as_float(h.y << 16); acc[3] += __uint_as_float(h.y & 0xFFFF0000u);
          acc[4] += __uint_as_float(h.z << 16); acc[5] += __uint_as_float(h.z & 0xFFFF0000u);
          acc[6] += __uint_as_float(h.w << 16); acc[7] += __uint_as_float(h.w & 0xFFFF0000u);
        }
    if (MASK == 1) {
      const float4* yp = reinterpret_cast<const float4*>(reinterpret_cast<const float*>(mask_y) + idx * 8);
      const float4 y0 = yp[0], y1 = yp[1];
      const float yv[8] = {y0.x, y0.y, y0.z, y0.w, y1.x, y1.y, y1.z, y1.w};
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[k] *= yv[k] > 0.f ? 1.f : slope;
    } else if (MASK == 2) {
      const uint4 y = *reinterpret_cast<const uint4*>(reinterpret_cast<const unsigned short*>(mask_y) + idx * 8);
      const unsigned yw[4] = {y.x, y.y, y.z, y.w};
      auto pos = [](unsigned h) { return (h & 0x8000u) == 0 && (h & 0x7FFFu) != 0; };
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        acc[2 * k] *= pos(yw[k] & 0xFFFFu) ? 1.f : slope;
        acc[2 * k + 1] *= pos(yw[k] >> 16) ? 1.f : slope;
      }
    } else if (MASK == 3) {
      const float4* yp = reinterpret_cast<const float4*>(reinterpret_cast<const float*>(mask_y) + idx * 8);
      const float4 y0 = yp[0], y1 = yp[1];
      acc[0] += y0.x; acc[1] += y0.y; acc[2] += y0.z; acc[3] += y0.w;
      acc[4] += y1.x; acc[5] += y1.y; acc[6] += y1.z; acc[7] += y1.w;
    }
    const uint4 o16 = make_uint4(pk2(acc[0], acc[1]), pk2(acc[2], acc[3]), pk2(acc[4], acc[5]), pk2(acc[6], acc[7]));
    if constexpr (OUT16) {
      *reinterpret_cast<uint4*>(reinterpret_cast<unsigned short*>(din) + idx * 8) = o16;
    } else {
      float4* dp = reinterpret_cast<float4*>(din + idx * 8);
      dp[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
      dp[1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
      if constexpr (SIDE16) *reinterpret_cast<uint4*>(side16 + idx * 8) = o16;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) bs[k] += acc[k];
  }
  if (bsum) {
    __shared__ float bred[256 * 8];
#pragma unroll
    for (int k = 0; k < 8; ++k) bred[threadIdx.x * 8 + k] = bs[k];
    __syncthreads();
    // (a lane keeps one channel group: the grid stride is a multiple of c8n)
    for (int item = threadIdx.x; item < c8n * 8; item += 256) {
      const int grp = item >> 3, k = item & 7;
      float t = 0.f;
      for (int q = grp; q < 256; q += c8n) t += bred[q * 8 + k];
      bsum[(int64_t)blockIdx.x * g.Ci + grp * 8 + k] = t;
    }
  }
}

}  // namespace

int launch_gather(s3_ctx* ctx, const GatherGeom& g, const void* in, void* out,
                  int esize) {
  const int vw = 16 / esize;   // elements per 16-B access
  bool vec = (g.Co % vw == 0) && (g.Ci % vw == 0) &&
             (g.kind != S3_OP_CONCAT || (g.c_off % vw == 0 && g.rep % vw == 0));
  int64_t n = (int64_t)g.N * g.Do[0] * g.Do[1] * g.Do[2] * (g.Co / (vec ? vw : 1));
  int grid = grid_for(n, ctx->num_cu);
  if (esize == 4) {
    if (vec) hipLaunchKernelGGL((gather_kernel<4, float>), dim3(grid), dim3(kBlock), 0, ctx->stream, (const float*)in, (float*)out, g);
    else hipLaunchKernelGGL((gather_kernel<1, float>), dim3(grid), dim3(kBlock), 0, ctx->stream, (const float*)in, (float*)out, g);
  } else {
    if (vec) hipLaunchKernelGGL((gather_kernel<8, unsigned short>), dim3(grid), dim3(kBlock), 0, ctx->stream, (const unsigned short*)in, (unsigned short*)out, g);
    else hipLaunchKernelGGL((gather_kernel<1, unsigned short>), dim3(grid), dim3(kBlock), 0, ctx->stream, (const unsigned short*)in, (unsigned short*)out, g);
  }
  S3_HIP(ctx, hipGetLastError());
  return S3_OK;
}

bool gather_bwd_mask_ok(const GatherGeom& g) {
  return g.kind == S3_OP_PAD && g.Ci == g.Co && (g.Ci & 3) == 0;
}

// channel sums of a masked / added fold ride along when the geometry allows
// (see the kernel); plan.cpp sizes and claims their buffer with these two
bool gather_bwd_bsum_ok(const GatherGeom& g) {
  const int c4n = g.Ci >> 2;
  return gather_bwd_mask_ok(g) && c4n >= 1 && c4n <= 64 && (256 % c4n) == 0 && kBlock == 256;
}
int gather_bwd_bsum_blocks(const s3_ctx* ctx, const GatherGeom& g) {
  int64_t n = (int64_t)g.N * g.Di[0] * g.Di[1] * g.Di[2] * g.Ci;
  return grid_for(n / 4, ctx->num_cu);
}

// the 8-channel walk of a bf16 frame: C % 8 == 0, 32-bit item count, and the
// bsum contract (one channel group per lane: c8n | 256, grid stride | c8n)
static bool fold16x8_ok(const s3_ctx* ctx, const GatherGeom& g, const float* bsum) {
  const int64_t n = (int64_t)g.N * g.Di[0] * g.Di[1] * g.Di[2] * g.Ci;
  const int c8n = g.Ci >> 3;
  if ((g.Ci & 7) || c8n < 1 || n / 8 > 0x7fffffffLL) return false;
  if (bsum && (c8n > 64 || 256 % c8n != 0 || kBlock != 256)) return false;
  return true;
}

// ------------------------------------------------------------ launch_fold
// One (MASK, OUT16, SIDE16) row on the walk chosen.  The rows launch_fold names
// are everything a FoldJob can ask for: 8 x {fp32 frame, bf16 frame} of the
// 4-wide kernel and 8 of the 8-wide one, no cross product.
// (Every frame the plan writes as bf16 today has 64 channels —
// conv_mfma_persist_dgrad_geom_ok, conv2d_ws_frame_geom_ok — so the 8-wide walk
// takes it; the bf16-frame 4-wide walk is what is left behind fold16x8_ok's
// 32-bit item guard and stays for that.)
enum FoldWalk { FOLD_X8, FOLD_PAD4_FR16, FOLD_PAD4, FOLD_GATHER };

template <int MASK, bool OUT16, bool SIDE16>
static void fold_launch(s3_ctx* ctx, FoldWalk walk, const GatherGeom& g, const FoldJob& j, const void* aux,
                        float slope, float* bsum) {
  const int64_t n = (int64_t)g.N * g.Di[0] * g.Di[1] * g.Di[2] * g.Ci;
  // (n / 4 on the 8-wide walk too: the block count the readers of bsum expect)
  const dim3 grid(grid_for(n / 4, ctx->num_cu)), blk(kBlock);
  if (walk == FOLD_X8)
    hipLaunchKernelGGL((fold16x8_kernel<MASK, OUT16, SIDE16>), grid, blk, 0, ctx->stream,
                       (const unsigned short*)j.frame, j.din, g, aux, slope, bsum, j.side16);
  else if (walk == FOLD_PAD4_FR16)
    hipLaunchKernelGGL((gather_bwd_pad4_kernel<MASK, OUT16, SIDE16, true>), grid, blk, 0, ctx->stream,
                       (const float*)j.frame, j.din, g, aux, slope, bsum, j.side16);
  else
    hipLaunchKernelGGL((gather_bwd_pad4_kernel<MASK, OUT16, SIDE16, false>), grid, blk, 0, ctx->stream,
                       (const float*)j.frame, j.din, g, aux, slope, bsum, j.side16);
}

int launch_fold(s3_ctx* ctx, const GatherGeom& g, const FoldJob& j) {
  const bool plain = j.mode == FoldJob::PLAIN, masked = j.mode == FoldJob::MASKED;
  // the bf16-only store and a bf16 aux belong to the masked fold, the bf16 side copy to the other two
  if (masked ? j.side16 != nullptr : (j.out_bf16 || j.aux_bf16))
    S3_FAIL(ctx, S3_EINVAL, "fold: no kernel stores this way in this mode");
  const bool wide = gather_bwd_mask_ok(g);
  if (!wide && masked) S3_FAIL(ctx, S3_EINVAL, "gather_bwd_masked: unsupported geometry");
  if (!wide && !plain) S3_FAIL(ctx, S3_EINVAL, "gather_bwd_add: unsupported geometry");
  if (!wide && j.frame16) S3_FAIL(ctx, S3_EINVAL, "gather_bwd: a bf16 frame needs the float4 fold");
  if (!wide && j.side16) S3_FAIL(ctx, S3_EINVAL, "gather_bwd: bf16 side copy needs the float4 fold");
  // (a plain fold has no aux and leaves no channel sums)
  const void* aux = plain ? nullptr : j.aux;
  float* bsum = plain ? nullptr : j.bsum;
  const float slope = masked ? j.slope : 0.f;
  const FoldWalk walk = !wide ? FOLD_GATHER
                        : !j.frame16 ? FOLD_PAD4
                        : fold16x8_ok(ctx, g, bsum) ? FOLD_X8 : FOLD_PAD4_FR16;
  if (walk == FOLD_GATHER) {   // the adjoint of any gather op, one element per lane: no mode
    const int64_t n = (int64_t)g.N * g.Di[0] * g.Di[1] * g.Di[2] * g.Ci;
    hipLaunchKernelGGL(gather_bwd_kernel, dim3(grid_for(n, ctx->num_cu)), dim3(kBlock), 0, ctx->stream,
                       (const float*)j.frame, j.din, g);
  } else {
    const int mask = plain ? 0 : masked ? (j.aux_bf16 ? 2 : 1) : 3;
#define S3_FOLD_ROW(M, O16, S16)                                                     \
    case M * 4 + O16 * 2 + S16: fold_launch<M, O16, S16>(ctx, walk, g, j, aux, slope, bsum); break
    switch (mask * 4 + (j.out_bf16 ? 2 : 0) + (j.side16 ? 1 : 0)) {
      S3_FOLD_ROW(0, false, false); S3_FOLD_ROW(0, false, true);     // plain (+ bf16 side copy)
      S3_FOLD_ROW(1, false, false); S3_FOLD_ROW(1, true, false);     // masked by an fp32 y (bf16-only store)
      S3_FOLD_ROW(2, false, false); S3_FOLD_ROW(2, true, false);     // masked by a bf16 y
      S3_FOLD_ROW(3, false, false); S3_FOLD_ROW(3, false, true);     // added to the first contribution
      default: S3_FAIL(ctx, S3_EINVAL, "fold: no kernel stores this way in this mode");
    }
#undef S3_FOLD_ROW
    static const int mode_stat[] = {S3_STAT_FOLD_PLAIN, S3_STAT_FOLD_MASKED, S3_STAT_FOLD_ADD};
    ++ctx->stat[mode_stat[j.mode]];
  }
  // (in FoldWalk's order)
  static const int walk_stat[] = {S3_STAT_FOLD16X8, S3_STAT_FOLD_PAD4_FR16, S3_STAT_FOLD_PAD4, S3_STAT_FOLD_GATHER};
  ++ctx->stat[walk_stat[walk]];
  S3_HIP(ctx, hipGetLastError());
  return S3_OK;
}
