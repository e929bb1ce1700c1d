// The frame the backward kernels share (kernels_grad.hip, kernels_grad_cos.hip):
// powers by multiplication, the chunks of a time axis with the two lane-to-time maps, and the
// additive block scan in two phases around the caller's ONE barrier.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "walk_scan.h"

namespace fr {

// x^e for e >= 0 by multiplication (e - 1 roundings; x^0 = 1 for every x, a zero included)
__device__ __forceinline__ double ipow(double x, int e) {
  if (e == 0) return 1.0;
  double p = x;
  for (int i = 1; i < e; ++i) p *= x;
  return p;
}

// d/dx x^e = e x^(e-1), the power by multiplication (never m / x: a zero input is an ordinary
// one); e < 0: e / x^(|e|+1)
__device__ __forceinline__ double dpow(double x, int e) {
  return e > 0 ? (double)e * ipow(x, e - 1) : (double)e * (1.0 / ipow(x, 1 - e));
}

// The chunks of a time axis and the first of the four steps of this lane in chunk c.
__device__ __forceinline__ int64_t grad_chunks(int64_t T) { return (T + kGradChunk - 1) / kGradChunk; }
__device__ __forceinline__ int64_t forward_t0(int64_t c) { return c * kGradChunk + 4 * (int64_t)threadIdx.x; }
__device__ __forceinline__ int64_t reversed_t0(int64_t c) {
  return c * kGradChunk + (kGradChunk - 4) - 4 * (int64_t)threadIdx.x;
}

// The additive block scan over the lanes' totals, lane 0 first.  Publish: the wave scan; lane 63
// leaves the wave's total in slot[wave]; returns the sum of the lanes in front within the wave.
__device__ __forceinline__ double scan_publish(double total, double *slot) {
  const double incl = wave_inclusive_scan<0>(total);
  const double excl = wave_shift_right1<0>(incl);
  if ((threadIdx.x & 63) == 63) slot[threadIdx.x >> 6] = incl;
  return excl;
}

// Offset, after the barrier: the wave totals join `carry` in wave order; returns the sum of
// everything in front of this lane - the chunks before, the waves before, `excl` - and leaves
// the carry of the next chunk.
__device__ __forceinline__ double scan_offset(const double *slot, double excl, double &carry) {
  const int wave = threadIdx.x >> 6;
  double run = carry, off = carry;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    if (w == wave) off = run;
    run += slot[w];
  }
  carry = run;
  return off + excl;
}

// The lane's own inclusive sums, towards its first step (the reversed map: suffix sums over time).
__device__ __forceinline__ void lane_suffix(double (&b)[4]) {
  b[2] += b[3];
  b[1] += b[2];
  b[0] += b[1];
}

}  // namespace fr
