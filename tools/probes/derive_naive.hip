// The shape s3_level_interp avoids, for tools/derive_probe.py only: one lane
// per column, one variable, one target, linear.  A lane reads its L levels at
// a stride of 4 L bytes, so a wave's load touches 64 different cache lines.
// Same selection rule and arithmetic as csrc/kernels_derive.hip.
//   hipcc --offload-arch=gfx950 -O3 -shared -fPIC derive_naive.hip -o derive_naive.so
#include <hip/hip_runtime.h>
#include <stdint.h>

__global__ void __launch_bounds__(256)
naive_kernel(const float* __restrict__ lev, const float* __restrict__ var, int64_t P, int L, float target,
             float* __restrict__ out) {
#pragma clang fp contract(off)
  for (int64_t col = (int64_t)blockIdx.x * 256 + threadIdx.x; col < P; col += (int64_t)gridDim.x * 256) {
    const float* lv = lev + col * L;
    const float* vr = var + col * L;
    int ib = -1, ia = -1, il = -1;
    float db = 0.f, da = 0.f, dl = 0.f;
    for (int i = 0; i < L; ++i) {
      const float x = lv[i];
      if (x != x) continue;
      const float d = fabsf(__fsub_rn(x, target));
      if (x < target) { if (ib < 0 || d < db) { ib = i; db = d; } }
      else if (ia < 0 || d < da) { ia = i; da = d; }
      if (il < 0 || d < dl) { il = i; dl = d; }
    }
    int i1 = ib >= 0 ? ib : (il >= 0 ? il : 0), i2 = ia;
    if (i2 < 0) {
      i2 = 0;
      float dt = 0.f;
      bool found = false;
      for (int i = 0; i < L; ++i) {
        const float x = lv[i];
        if (i == i1 || x != x) continue;
        const float d = fabsf(__fsub_rn(x, target));
        if (!found || d < dt) { found = true; i2 = i; dt = d; }
      }
    }
    const float l1 = lv[i1], l2 = lv[i2];
    const float diff = __fsub_rn(l2, l1);
    const float alpha = fabsf(diff) < 1e-3f ? 0.f : __fdiv_rn(__fsub_rn(target, l1), diff);
    out[col] = __fadd_rn(__fmul_rn(vr[i1], __fsub_rn(1.f, alpha)), __fmul_rn(vr[i2], alpha));
  }
}

extern "C" int naive_level_interp(void* stream, const float* lev, const float* var, int64_t P, int L, float target,
                                  float* out, int grid) {
  if (!lev || !var || !out || P < 1 || L < 1 || grid < 1) return -1;
  hipLaunchKernelGGL(naive_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, lev, var, P, L, target, out);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
