// What the kernels share below the level of a tile: vector types, the bf16
// pack / split arithmetic, the activation selects, Philox, the slab row map,
// and the hand-written barriers and waits.  Each is defined here once; for
// .hip files and conv_mfma_tile.h only (no .cpp includes it).
#pragma once
#include <hip/hip_runtime.h>

#include "common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));     // MFMA accumulator
typedef short bf16x8 __attribute__((ext_vector_type(8)));    // MFMA bf16 operand, 16 B
typedef short s16x4 __attribute__((ext_vector_type(4)));     // ds_read_b64_tr_b16 result
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));  // 16-B load of inline asm
typedef float hf32x2 __attribute__((ext_vector_type(2)));    // the pair pk2 converts from
typedef __bf16 hbf16x2 __attribute__((ext_vector_type(2)));  // ... and to

// two fp32 -> one dword of two bf16, a in the low half: v_cvt_pk_bf16_f32,
// round to nearest even
__device__ __forceinline__ unsigned pk2(float a, float b) {
  hf32x2 v = {a, b};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, hbf16x2));
}
// low / high bf16 half of a dword -> fp32, exact (no rounding)
__device__ __forceinline__ float bf_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf_hi(unsigned u) { return __uint_as_float(u & 0xFFFF0000u); }

// eight fp32 values -> two 16-B chunks: hi = bf16(v) rounded as pk2 does,
// lo = bf16(v - hi), the residue rounded the same way
__device__ __forceinline__ void split8(const float4& a, const float4& b, uint4& hi, uint4& lo) {
  hi = make_uint4(pk2(a.x, a.y), pk2(a.z, a.w), pk2(b.x, b.y), pk2(b.z, b.w));
  lo = make_uint4(pk2(a.x - bf_lo(hi.x), a.y - bf_hi(hi.x)), pk2(a.z - bf_lo(hi.y), a.w - bf_hi(hi.y)),
                  pk2(b.x - bf_lo(hi.z), b.y - bf_hi(hi.z)), pk2(b.z - bf_lo(hi.w), b.w - bf_hi(hi.w)));
}

// leaky select with the slope already chosen (1 identity, 0 ReLU, alpha Leaky);
// one multiply, rounded once; a negative v under slope 0 gives -0
__device__ __forceinline__ float act_sel(float v, float slope) { return v > 0.f ? v : slope * v; }
// (v * sc) + sh with TWO roundings, like numpy's un-normalisation (and
// s3_chunk_epilogue), for the windowed forward of the chunk executor: the
// empty asm keeps the compiler from contracting the pair into one fma
__device__ __forceinline__ float affine2(float v, float sc, float sh) {
  float t = v * sc;
  asm volatile("" : "+v"(t));
  return t + sh;
}
// Activation, select form: act_sel with the slope taken from the kind, so a
// wave never branches on the kind per value.  ReLU of a negative v is 0 * v =
// -0.  Used by the halo-tile convs (conv_mfma_tile.h), kernels_pointwise.hip
// and kernels_conv_generic.hip; act_f_branch must not replace it there: the
// sign of a zero would change and so would the code (two scalar branches).
__device__ __forceinline__ float act_f(float v, int act, float alpha) {
  const float s = act == S3_ACT_LEAKY ? alpha : (act == S3_ACT_RELU ? 0.f : 1.f);
  return act_sel(v, s);
}
// Activation, branch form: ReLU of a negative v is +0, identity multiplies
// nothing.  Used by kernels_conv_fewpos.hip, kernels_conv_fewpos_mfma.hip and
// kernels_dense.hip; act_f must not replace it there: their ReLU zeros would
// turn from +0 into -0.
__device__ __forceinline__ float act_f_branch(float v, int act, float alpha) {
  if (act == S3_ACT_RELU) return v > 0.f ? v : 0.f;
  if (act == S3_ACT_LEAKY) return v > 0.f ? v : alpha * v;
  return v;
}

// Philox4x32-10, counter (c0..c3), key (k0, k1): integer only, nothing rounds
__device__ __forceinline__ void philox4(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                        uint32_t k0, uint32_t k1, uint32_t out[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// LDS slab row rho = nf*16 + kq*4 + r  <->  output channel of the 64-wide tile
//   (nf >> 1)*32 + kq*8 + (nf & 1)*4 + r
// so that lane (pos, kq) owns channels h*32 + kq*8 .. +7 for h = nf >> 1.
__host__ __device__ __forceinline__ int slab_row_cout(int rho) {
  const int nf = rho >> 4, kq = (rho >> 2) & 3, r = rho & 3;
  return (nf >> 1) * 32 + kq * 8 + (nf & 1) * 4 + r;
}

// Workgroup barriers without the fence of __syncthreads() ("memory": no
// compiler motion across them).
// WG_BARRIER waits for NOTHING: what the hand-over needs (LDS reads drained,
// loads landed) is ordered by the explicit waits next to it.
#define WG_BARRIER() asm volatile("s_barrier" ::: "memory")
// WG_BARRIER_LDS first waits for this wave's LDS (and scalar) operations.
#define WG_BARRIER_LDS() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")

// Counted waits; n is a literal.  Sites whose asm statement carries operands
// or no "memory" clobber are not these and stay spelled out where they are.
// at most n vector-memory operations (loads, LDS-DMA) still in flight
#define WAIT_VM(n) asm volatile("s_waitcnt vmcnt(" #n ")" ::: "memory")
// every LDS / scalar-memory operation of this wave has returned
#define WAIT_LGKM0() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
// both: at most n vector-memory operations in flight, LDS drained
#define WAIT_VM_LGKM0(n) asm volatile("s_waitcnt vmcnt(" #n ") lgkmcnt(0)" ::: "memory")
