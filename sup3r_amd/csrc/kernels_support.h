// What the streaming support kernels share (kernels_fold, kernels_pointwise,
// kernels_reduce, kernels_optim, kernels_loss_content, kernels_chunk_io): the
// block sum.  The launch shape of their grid-stride passes (kBlock, grid_for)
// is launch_shape.h's, through common.h.  For .hip files only.
#pragma once
#include "common.h"

namespace {

__device__ inline float wave_sum(float v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

__device__ inline float block_sum(float v, float* sm) {
  v = wave_sum(v);
  int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) sm[w] = v;
  __syncthreads();
  float t = 0.f;
  if (threadIdx.x == 0) {
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += sm[i];
  }
  return t;  // valid on thread 0
}

}  // namespace
