// fr_sieve_heads / fr_sieve_heads_adjoint: the heads END, MAX, MIN, MPI and CUR over every row of
// the iterated sums in one launch, and the expansion of their (N, K, F) feature gradients into the
// dense (N, K, T) gradient of the rows - the band features of DESIGN.md 4.14.9.
//
// FORWARD.  One workgroup of 256 lanes per row (k, n) of a contiguous (K, N, T) buffer, every sieve,
// segment and band of the spec table in turn.  END / MAX / MIN are sieve_pick_kernel's (pick_end,
// pick_extreme of sieve_rows.h): value and position.  MPI / CUR are sieve_kernel's: thread-strided
// partial sums of the in-band elements of D = E^inc row (diff_uniform: diff_at's bits), the __shfl_xor tree, the four
// wave totals added in wave order by thread 0, c > 0 ? s / c : 0 - the bits of fr_sieve for MPI -,
// and the in-band count as the feature's int32 companion.
//
// ADJOINT.  One workgroup per row (n, k); it writes every element of the row's gradient once, no
// memset, no atomics.  The weight of feature f on D[t] is g_f / (double)c_f (MPI) or (2.0 g_f) D[t]
// (CUR) for the t of its segment and band - the band test runs on the row again -; per sieve
// u[t] = +0.0 plus those weights in column order, and the sieve's contribution is (E^T)^inc u with
//   (E^T u)[s] = (s >= 1 ? u[s] : 0.0) - (s + 1 < L ? u[s + 1] : 0.0).
// A workgroup works in tiles of kHeadsTile steps: u of the tile and of a right halo of inc <= 8
// steps in LDS, the inc levels from one LDS buffer into the other behind a barrier each.  A
// selecting sieve adds its (position, g_f) pairs as gather_picked does: the pairs are
// workgroup-uniform loads, every lane compares them with its four steps.  G[s] = +0.0 plus the
// sieves' contributions in head order; +0.0 at s >= L.
// Compiled without contraction: the product of a CUR weight is rounded before it is added.
// All offsets are 64-bit; every access to a row is guarded by 0 <= t < T.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "sieve_rows.h"
#include "walk_scan.h"

namespace fr {

namespace {

struct SieveEntry {
  int kind, cut_begin, C1, q_begin, Q, feat_begin, inc;
};
// entry s of the spec table: workgroup-uniform, read through the constant address space
__device__ __forceinline__ SieveEntry spec_entry(const HeadSieve *__restrict__ spec, int s) {
  const int32_t *__restrict__ sp = reinterpret_cast<const int32_t *>(spec) + 7 * (int64_t)s;
  SieveEntry e;
  e.kind = as_const(sp)[0] & 0xff;
  e.cut_begin = as_const(sp)[1];
  e.C1 = as_const(sp)[2];
  e.q_begin = as_const(sp)[3];
  e.Q = as_const(sp)[4] - 1;
  e.feat_begin = as_const(sp)[5];
  e.inc = as_const(sp)[6];
  return e;
}

// diff_at for a workgroup-uniform order: the same subtractions in the same order - the same
// bits -, but the order is a compile-time constant behind one uniform branch, so the only masks
// are the guards on t.  diff_at's `j <= inc` tests, each combined with a guard on t, kept so many
// lane masks live in these kernels' loops that scalar registers spilled.
template <int I>
__device__ __forceinline__ double diff_order(const double *__restrict__ row, int64_t t) {
  double v[I + 1];
#pragma unroll
  for (int j = 0; j <= I; ++j) v[j] = t - j >= 0 ? row[t - j] : 0.0;
#pragma unroll
  for (int lvl = 1; lvl <= I; ++lvl) {
#pragma unroll
    for (int j = 0; j + lvl <= I; ++j) v[j] = t - j >= 1 ? v[j] - v[j + 1] : 0.0;
  }
  return v[0];
}
__device__ __forceinline__ double diff_uniform(const double *__restrict__ row, int64_t t, int inc) {
  switch (inc) {
    case 0: return row[t];
    case 1: return diff_order<1>(row, t);
    case 2: return diff_order<2>(row, t);
    case 3: return diff_order<3>(row, t);
    case 4: return diff_order<4>(row, t);
    case 5: return diff_order<5>(row, t);
    case 6: return diff_order<6>(row, t);
    case 7: return diff_order<7>(row, t);
    default: return diff_order<8>(row, t);
  }
}

}  // namespace

__global__ __launch_bounds__(256) void sieve_heads_kernel(const double *__restrict__ A, int64_t K,
                                                          int64_t N, int64_t T,
                                                          const HeadSieve *__restrict__ spec,
                                                          int n_sieves,
                                                          const int64_t *__restrict__ cuts,
                                                          int64_t cut_stride,
                                                          const double *__restrict__ q, int F,
                                                          double *__restrict__ feat,
                                                          int32_t *__restrict__ comp) {
  __shared__ unsigned long long sm_key[4];
  __shared__ int sm_pos[4];
  __shared__ double sm_sum[4];
  __shared__ double sm_cnt[4];
  const int64_t r = blockIdx.x;   // row k * N + n of A
  const int64_t k = r / N, n = r - k * N;
  const double *__restrict__ row = A + r * T;
  const int64_t out = (n * K + k) * (int64_t)F;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int s = 0; s < n_sieves; ++s) {
    const SieveEntry e = spec_entry(spec, s);
    const int64_t f0 = out + e.feat_begin;
    const int64_t *__restrict__ cut = cuts + n * cut_stride + e.cut_begin;
    if (e.kind == FR_SIEVE_END_K) {
      pick_end(row, T, cut, e.C1, feat + f0, comp + f0, tid);
      continue;
    }
    const bool selects = e.kind == FR_SIEVE_MAX_K || e.kind == FR_SIEVE_MIN_K;
    const bool cur = e.kind == FR_SIEVE_CUR_K;
    for (int j = 0; j < e.C1 - 1; ++j) {
      int64_t lo = cut[j], hi = cut[j + 1];
      if (lo < 0) lo = 0;
      if (hi > T) hi = T;
      for (int b = 0; b < e.Q; ++b) {
        const double qlo = q[e.q_begin + b], qhi = q[e.q_begin + b + 1];
        const int64_t f = f0 + (int64_t)j * e.Q + b;
        if (selects) {
          pick_extreme(row, lo, hi, qlo, qhi, e.kind == FR_SIEVE_MIN_K, sm_key, sm_pos, feat + f, comp + f,
                       tid);
          continue;
        }
        // MPI / CUR: sieve_kernel's sums, in its association
        double sum = 0.0, cnt = 0.0;
        for (int64_t t = lo + tid; t < hi; t += 256) {
          const double v = diff_uniform(row, t, e.inc);
          if (qlo < v && v <= qhi) {
            sum += cur ? v * v : v;
            cnt += 1.0;
          }
        }
        for (int o = 32; o > 0; o >>= 1) {
          sum += __shfl_xor(sum, o);
          cnt += __shfl_xor(cnt, o);
        }
        __syncthreads();   // (the slots are reused band after band)
        if (lane == 0) {
          sm_sum[wave] = sum;
          sm_cnt[wave] = cnt;
        }
        __syncthreads();
        if (tid == 0) {
          double sv = 0.0, c = 0.0;
          for (int w = 0; w < 4; ++w) {
            sv += sm_sum[w];
            c += sm_cnt[w];
          }
          feat[f] = cur ? sv : (c > 0.0 ? sv / c : 0.0);
          comp[f] = (int32_t)c;   // (c <= T < 2^31, an integer)
        }
      }
    }
  }
}

__global__ __launch_bounds__(256) void sieve_heads_adjoint_kernel(
    const double *__restrict__ rows, const int32_t *__restrict__ row_map, int64_t K, int64_t N, int64_t T,
    const HeadSieve *__restrict__ spec, int n_sieves, const int64_t *__restrict__ cuts, int64_t cut_stride,
    const double *__restrict__ q, int F, const int32_t *__restrict__ comp, const double *__restrict__ g,
    const int32_t *__restrict__ len, double *__restrict__ G) {
  __shared__ double sm_w[kPickMaxFeatures];
  __shared__ double sm_u[2][kHeadsTile + kMaxInc];
  const int64_t r = blockIdx.x;   // row n * K + k of comp, g and G
  const int64_t n = r / K, k = r - n * K;
  const int64_t v = row_map != nullptr ? (int64_t)as_const(row_map)[k] : k;
  const double *__restrict__ row = rows + (v * N + n) * T;
  int64_t L = T;
  if (len != nullptr) {
    L = as_const(len)[n];
    L = L < 0 ? 0 : (L > T ? T : L);
  }
  const int32_t *__restrict__ crow = comp + r * (int64_t)F;
  const double *__restrict__ grow = g + r * (int64_t)F;
  const int64_t *__restrict__ cut_row = cuts + n * cut_stride;
  const int tid = threadIdx.x;

  // the weight of every feature: what it adds per element it holds (CUR: times D[t])
  for (int s = 0; s < n_sieves; ++s) {
    const SieveEntry e = spec_entry(spec, s);
    const int nf = (e.C1 - 1) * (e.kind == FR_SIEVE_END_K ? 1 : e.Q);
    for (int i = tid; i < nf; i += 256) {
      const int f = e.feat_begin + i;
      const double gf = grow[f];
      double w = gf;
      if (e.kind == FR_SIEVE_MPI_K) {
        const int32_t c = crow[f];
        w = c > 0 ? gf / (double)c : 0.0;   // (an empty band holds no element: never added)
      } else if (e.kind == FR_SIEVE_CUR_K) {
        w = 2.0 * gf;
      }
      sm_w[f] = w;
    }
  }
  __syncthreads();

  for (int64_t t0 = 0; t0 < T; t0 += kHeadsTile) {
    if (t0 >= L) {   // a tile wholly behind the series' end: +0.0, nothing formed
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const int64_t t = t0 + 256 * m + tid;
        if (t < T) G[r * T + t] = 0.0;
      }
      continue;
    }
    double acc[4] = {0.0, 0.0, 0.0, 0.0};   // G at t0 + 256 m + tid
    for (int s = 0; s < n_sieves; ++s) {
      const SieveEntry e = spec_entry(spec, s);
      if (e.kind == FR_SIEVE_END_K || e.kind == FR_SIEVE_MAX_K || e.kind == FR_SIEVE_MIN_K) {
        const int nf = (e.C1 - 1) * (e.kind == FR_SIEVE_END_K ? 1 : e.Q);
        for (int i = 0; i < nf; ++i) {
          const int64_t p = as_const(crow)[e.feat_begin + i];   // (uniform: every lane sees every pair)
          if (p < t0 || p >= t0 + kHeadsTile || p >= L) continue;
          const double w = sm_w[e.feat_begin + i];
#pragma unroll
          for (int m = 0; m < 4; ++m)
            if (p == t0 + 256 * m + tid) acc[m] += w;
        }
        continue;
      }
      const bool cur = e.kind == FR_SIEVE_CUR_K;
      const int64_t *__restrict__ cut = cut_row + e.cut_begin;
      const int width = kHeadsTile + e.inc;   // the tile and its right halo
      for (int i = tid; i < width; i += 256) {
        const int64_t t = t0 + i;
        double u = 0.0;
        if (t < L) {
          const double d = diff_uniform(row, t, e.inc);
          for (int j = 0; j < e.C1 - 1; ++j) {
            int64_t lo = as_const(cut)[j], hi = as_const(cut)[j + 1];
            if (lo < 0) lo = 0;
            if (hi > T) hi = T;
            if (t < lo || t >= hi) continue;
            for (int b = 0; b < e.Q; ++b) {
              if (as_const(q)[e.q_begin + b] < d && d <= as_const(q)[e.q_begin + b + 1]) {
                const double w = sm_w[e.feat_begin + j * e.Q + b];
                u += cur ? w * d : w;
              }
            }
          }
        }
        sm_u[0][i] = u;
      }
      __syncthreads();
      // (E^T)^inc: level l reads buffer l & 1, whose first width - l entries are valid
      for (int l = 0; l < e.inc; ++l) {
        const double *src = sm_u[l & 1];
        double *dst = sm_u[(l + 1) & 1];
        for (int i = tid; i < width - l - 1; i += 256) {
          const int64_t t = t0 + i;
          const double a = t >= 1 ? src[i] : 0.0;
          const double c = t + 1 < L ? src[i + 1] : 0.0;
          dst[i] = a - c;
        }
        __syncthreads();
      }
      const double *res = sm_u[e.inc & 1];
#pragma unroll
      for (int m = 0; m < 4; ++m) acc[m] += res[256 * m + tid];
      __syncthreads();   // (the next sieve writes the buffers again)
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int64_t t = t0 + 256 * m + tid;
      if (t < T) G[r * T + t] = t < L ? acc[m] : 0.0;
    }
  }
}

hipError_t launch_sieve_heads(const double *A, int64_t K, int64_t N, int64_t T, const HeadSieve *spec,
                              int n_sieves, const int64_t *cuts, int64_t cut_stride, const double *q,
                              int F, double *feat, int32_t *comp, hipStream_t st) {
  if (K <= 0 || N <= 0 || n_sieves <= 0) return hipSuccess;
  if (K * N > 0x7fffffffLL || T < 1 || T > 0x7fffffffLL || F < 1 || F > kPickMaxFeatures || cut_stride < 0)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(sieve_heads_kernel, dim3((unsigned)(K * N)), dim3(256), 0, st, A, K, N, T, spec,
                     n_sieves, cuts, cut_stride, q, F, feat, comp);
  return hipGetLastError();
}

hipError_t launch_sieve_heads_adjoint(const double *rows, const int32_t *row_map, int64_t K, int64_t N,
                                      int64_t T, const HeadSieve *spec, int n_sieves, const int64_t *cuts,
                                      int64_t cut_stride, const double *q, int F, const int32_t *comp,
                                      const double *g, const int32_t *len, double *G, hipStream_t st) {
  if (K <= 0 || N <= 0 || n_sieves <= 0) return hipSuccess;
  if (K * N > 0x7fffffffLL || T < 1 || T > 0x7fffffffLL || F < 1 || F > kPickMaxFeatures || cut_stride < 0)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(sieve_heads_adjoint_kernel, dim3((unsigned)(K * N)), dim3(256), 0, st, rows, row_map, K,
                     N, T, spec, n_sieves, cuts, cut_stride, q, F, comp, g, len, G);
  return hipGetLastError();
}

}  // namespace fr
