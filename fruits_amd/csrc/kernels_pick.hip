// fr_sieve_pick: the selecting sieves END / MAX / MIN over every row of a materialised (K, N, T)
// buffer in one launch - the forward pass of the differentiable features.  Of
// each feature the value and the position of the element it selects: a backward pass needs
// nothing else of it.
//
// One workgroup of 256 lanes per row (k, n), every sieve, segment and band in turn (pick_end,
// pick_extreme of sieve_rows.h).  The value path is that of band_sieve_kernel / sieve_kernel
// (kernels_sieve.hip): MAX / MIN reduce band_key()s - 0 is the empty band and gives 0.0 -, END
// reads the element at cut - 1 with numpy's wrap of -1.  The position of a MAX / MIN is reduced in
// a second pass over the segment, once the whole workgroup knows the value: the smallest in-band t
// whose element EQUALS it as a double - np.argmax's rule, under which -0.0 and +0.0 tie (their
// keys differ).  The row was written by the walk just before: both passes read it from the cache.
// Plain loads and stores; all offsets are 64-bit; every access is guarded by 0 <= t < T.  The
// spec table is workgroup-uniform and read through the constant address space (scalar loads).
// PER-SERIES CUTS (FR_SIEVE_SERIES_CUTS on every kind): series n reads the cut
// rows at cuts + n * cut_stride - resolved on the host for its own length, END's wrap included -,
// so a band ends at the series' end and no position lies behind it; cut_stride 0: one table.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "sieve_rows.h"
#include "walk_scan.h"

namespace fr {

__global__ __launch_bounds__(256) void sieve_pick_kernel(const double *__restrict__ A, int64_t K,
                                                         int64_t N, int64_t T,
                                                         const PickSieve *__restrict__ spec,
                                                         int n_sieves,
                                                         const int64_t *__restrict__ cuts,
                                                         int64_t cut_stride,
                                                         const double *__restrict__ q, int F,
                                                         double *__restrict__ feat,
                                                         int32_t *__restrict__ pos) {
  __shared__ unsigned long long sm_key[4];
  __shared__ int sm_pos[4];
  const int64_t r = blockIdx.x;   // row k * N + n of A
  const int64_t k = r / N, n = r - k * N;
  const double *__restrict__ row = A + r * T;
  const int64_t out = (n * K + k) * (int64_t)F;
  const int tid = threadIdx.x;
  const int32_t *__restrict__ sp = reinterpret_cast<const int32_t *>(spec);
  for (int s = 0; s < n_sieves; ++s) {
    const int kind = as_const(sp)[6 * s] & 0xff, cut_begin = as_const(sp)[6 * s + 1], C1 = as_const(sp)[6 * s + 2];
    const int q_begin = as_const(sp)[6 * s + 3], Q = as_const(sp)[6 * s + 4] - 1;
    const int64_t f0 = out + as_const(sp)[6 * s + 5];
    const int64_t *__restrict__ cut = cuts + n * cut_stride + cut_begin;
    if (kind == FR_SIEVE_END_K) {
      pick_end(row, T, cut, C1, feat + f0, pos + f0, tid);
      continue;
    }
    const bool is_min = kind == FR_SIEVE_MIN_K;
    for (int j = 0; j < C1 - 1; ++j) {
      int64_t lo = cut[j], hi = cut[j + 1];
      if (lo < 0) lo = 0;
      if (hi > T) hi = T;
      for (int b = 0; b < Q; ++b)
        pick_extreme(row, lo, hi, q[q_begin + b], q[q_begin + b + 1], is_min, sm_key, sm_pos,
                     feat + f0 + (int64_t)j * Q + b, pos + f0 + (int64_t)j * Q + b, tid);
    }
  }
}

hipError_t launch_sieve_pick(const double *A, int64_t K, int64_t N, int64_t T, const PickSieve *spec,
                             int n_sieves, const int64_t *cuts, int64_t cut_stride, const double *q,
                             int F, double *feat, int32_t *pos, hipStream_t st) {
  if (K <= 0 || N <= 0 || n_sieves <= 0) return hipSuccess;
  if (K * N > 0x7fffffffLL || T < 1 || T > 0x7fffffffLL || F < 1 || F > kPickMaxFeatures || cut_stride < 0)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(sieve_pick_kernel, dim3((unsigned)(K * N)), dim3(256), 0, st, A, K, N, T, spec,
                     n_sieves, cuts, cut_stride, q, F, feat, pos);
  return hipGetLastError();
}

}  // namespace fr
