// What the row sieves share on the device: the differencing of a row (kernels_sieve.hip,
// kernels_heads.hip) and the selecting sieves with the position of the element they select
// (kernels_pick.hip, kernels_heads.hip).  One workgroup of 256 lanes per row.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace fr {

// value of the inc-times differenced series at t (IncrementSieve._pre_transform,
// fruits/sieving/increment.py:63-71 with _increments of fruits/cache.py:8-13):
// D_0 = A, D_k[t] = D_{k-1}[t] - D_{k-1}[t-1] for t >= 1, D_k[0] = 0.
__device__ __forceinline__ double diff_at(const double *__restrict__ row, int64_t t, int inc) {
  double v[kMaxInc + 1];
#pragma unroll
  for (int j = 0; j <= kMaxInc; ++j) v[j] = (j <= inc && t - j >= 0) ? row[t - j] : 0.0;
#pragma unroll
  for (int lvl = 1; lvl <= kMaxInc; ++lvl) {
    if (lvl <= inc) {
#pragma unroll
      for (int j = 0; j + lvl <= kMaxInc; ++j)
        if (j <= inc - lvl) v[j] = (t - j >= 1) ? v[j] - v[j + 1] : 0.0;
    }
  }
  return v[0];
}

// END over one cut row: feature j is the element at cut[j + 1] - 1 with numpy's wrap of -1, and
// its position; out of range: NaN as in sieve_kernel (the host validates integer cuts), position -1.
__device__ __forceinline__ void pick_end(const double *__restrict__ row, int64_t T,
                                         const int64_t *__restrict__ cut, int C1,
                                         double *__restrict__ feat, int32_t *__restrict__ pos, int tid) {
  for (int j = tid; j < C1 - 1; j += 256) {
    int64_t idx = cut[j + 1] - 1;
    if (idx < 0) idx += T;
    const bool in = idx >= 0 && idx < T;
    feat[j] = in ? row[idx] : __builtin_nan("");
    pos[j] = in ? (int32_t)idx : -1;
  }
}

// MAX / MIN of the elements of [lo, hi) inside the band qlo < v <= qhi, and the FIRST step that
// attains it: thread 0 writes both (0.0 and -1 for an empty band).  The value is the largest
// band_key of the band, as band_sieve_kernel reduces it; the position a second pass, once the
// whole workgroup knows the value: the smallest in-band t whose element EQUALS it as a double.
// Called by all 256 lanes; sm_key and sm_pos hold four entries each.
__device__ __forceinline__ void pick_extreme(const double *__restrict__ row, int64_t lo, int64_t hi,
                                             double qlo, double qhi, bool is_min,
                                             unsigned long long *sm_key, int *sm_pos,
                                             double *__restrict__ feat, int32_t *__restrict__ pos,
                                             int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  unsigned long long key = 0;
  for (int64_t t = lo + tid; t < hi; t += 256) {
    const double v = row[t];
    if (qlo < v && v <= qhi) {
      const unsigned long long kv = band_key(v, is_min);
      key = kv > key ? kv : key;
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long w = __shfl_xor(key, o);
    key = w > key ? w : key;
  }
  __syncthreads();   // (the slots are reused band after band)
  if (lane == 0) sm_key[wave] = key;
  __syncthreads();
  for (int w = 0; w < 4; ++w) key = sm_key[w] > key ? sm_key[w] : key;
  const double res = band_key_value(key, is_min);
  // the position: the first in-band step that attains it (an empty band has none)
  int first = 0x7fffffff;
  if (key != 0) {
    for (int64_t t = lo + tid; t < hi; t += 256) {
      const double v = row[t];
      if (qlo < v && v <= qhi && v == res) {
        first = (int)t;
        break;   // (a lane's steps rise)
      }
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    const int w = __shfl_xor(first, o);
    first = w < first ? w : first;
  }
  if (lane == 0) sm_pos[wave] = first;
  __syncthreads();
  if (tid == 0) {
    for (int w = 0; w < 4; ++w) first = sm_pos[w] < first ? sm_pos[w] : first;
    *feat = res;
    *pos = first == 0x7fffffff ? -1 : first;
  }
}

}  // namespace fr
