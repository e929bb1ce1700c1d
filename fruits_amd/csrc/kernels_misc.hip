// Small streaming HIP kernels around the trie walk and their launchers: exp / trig tables, INC,
// path-length lookups, STD and the row statistics, the feature finalizers, CosWISS ffn / combine.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "walk_scan.h"
#include "pairwise.h"

namespace fr {

// ---------------------------------------------------------------- exp tables
// aux[2a]   = exp( g * alpha_a)   (np.exp(weights * alpha[k]),  semiring.py:123,150)
// aux[2a+1] = exp(-g * alpha_a)   (np.exp(-weights * alpha[k]), semiring.py:119,153,157)
// Arctic (linear = 1): aux[a] = g * alpha_a   (weights * alpha[k], semiring.py:297,306,330)
__global__ void exp_tables_kernel(const double *__restrict__ g, int64_t count,
                                  const float *__restrict__ alphas, int n_alpha,
                                  double *__restrict__ aux, int linear) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const double w = g[i];
  if (linear) {
    for (int a = 0; a < n_alpha; ++a) aux[(int64_t)a * count + i] = w * (double)alphas[a];
    return;
  }
  for (int a = 0; a < n_alpha; ++a) {
    const double al = (double)alphas[a];
    aux[(int64_t)(2 * a) * count + i] = exp(w * al);
    aux[(int64_t)(2 * a + 1) * count + i] = exp(-w * al);
  }
}

// ---------------------------------------------------------------- increments
__global__ void increments_kernel(const double *__restrict__ X, int64_t rows, int64_t T,
                                  int64_t shift, double *__restrict__ out,
                                  const double *__restrict__ head_src, int64_t head) {
  const int64_t total = rows * T;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t t = i % T;
    double v = (t >= shift) ? X[i] - X[i - shift] : 0.0;
    if (head_src != nullptr && t < head) v = head_src[i];
    out[i] = v;
  }
}

// ---------------------------------------------------------------- path-length lookup
// One workgroup per series: r = cumsum_t |dx_0| (or dx_0^2), optional /(last+1e-5),
// min-max normalise, * scale.  fruits/iss/weighting.py:148-160, cache.py:25-40,
// preparation/transform.py:184-198.
__device__ __forceinline__ double block_reduce_minmax(double v, bool is_max, double *sm) {
  for (int o = 32; o > 0; o >>= 1) {
    double w = __shfl_xor(v, o);
    v = is_max ? fmax(v, w) : fmin(v, w);
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();
  if (lane == 0) sm[wave] = v;
  __syncthreads();
  double r = sm[0];
  for (int w = 1; w < (int)(blockDim.x >> 6); ++w) r = is_max ? fmax(r, sm[w]) : fmin(r, sm[w]);
  return r;
}

__global__ __launch_bounds__(256) void pathlen_lookup_kernel(const double *__restrict__ X,
                                                              int64_t D, int64_t T, int norm,
                                                              int relative, double scale,
                                                              int exact,
                                                              double *__restrict__ out) {
  __shared__ double sm_red[4];
  __shared__ double sm_last;
  __shared__ double sm_tot[2][4];
  const int64_t n = blockIdx.x;
  const double *x = X + n * D * T;  // dimension 0 only
  double *o = out + n * T;
  const int tid = threadIdx.x;
  // The cumulative path length is summed SEQUENTIALLY (one lane per series) like
  // np.cumsum in the reference (fruits/cache.py:25-40): the lookup is then bit-identical
  // to the reference's, and with it every max-plus (Arctic) result - a running maximum
  // has long plateaus, and a fitted quantile that equals a plateau value is an exact tie
  // for all of its elements (a 1-ulp difference in g would move the whole plateau to the
  // other band).  O(T) dependent adds per series, all series in parallel: ~20 us at T = 4096.
  // (the summands are formed and the results stored by the whole workgroup through LDS;
  // only the adds themselves are serial)
  // exact == 0 (Reals plans, whose sums are re-associated anyway): a parallel scan.
  constexpr int kSeg = 4096;
  __shared__ double seg[kSeg];
  double acc = 0.0;  // meaningful in thread 0 only
  if (!exact) {
    const int lane = tid & 63, wave = tid >> 6;
    double run_carry = 0.0;
    int buf = 0;
    for (int64_t t0 = 0; t0 < T; t0 += 512) {
      double s2[2];
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int64_t t = t0 + tid * 2 + e;
        double d = 0.0;
        if (t < T && t >= 1) d = x[t] - x[t - 1];
        s2[e] = (norm == 1) ? fabs(d) : d * d;
        if (t >= T) s2[e] = 0.0;
      }
      const double l1 = s2[0] + s2[1];
      const double incl = wave_inclusive_scan(l1);
      const double excl = wave_shift_right1(incl);
      if (lane == 63) sm_tot[buf][wave] = incl;
      __syncthreads();
      double run = run_carry, base = 0.0;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        if (w == wave) base = run;
        run += sm_tot[buf][w];
      }
      run_carry = run;
      buf ^= 1;
      const double off = base + excl;
      const int64_t t = t0 + tid * 2;
      if (t < T) o[t] = off + s2[0];
      if (t + 1 < T) o[t + 1] = off + l1;
    }
    acc = run_carry;  // the same value in every thread
  }
  for (int64_t c0 = 0; exact && c0 < T; c0 += kSeg) {
    const int len = (int)((T - c0) < kSeg ? (T - c0) : kSeg);
    for (int i = tid; i < len; i += blockDim.x) {
      const int64_t t = c0 + i;
      const double d = t >= 1 ? x[t] - x[t - 1] : 0.0;
      seg[i] = (norm == 1) ? fabs(d) : d * d;
    }
    __syncthreads();
    if (tid == 0) {
      int i = 0;
      for (; i + 8 <= len; i += 8) {  // 8 LDS reads in flight, then the 8 dependent adds
        double v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = seg[i + j];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          acc += v[j];
          v[j] = acc;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) seg[i + j] = v[j];
      }
      for (; i < len; ++i) {
        acc += seg[i];
        seg[i] = acc;
      }
    }
    __syncthreads();
    for (int i = tid; i < len; i += blockDim.x) o[c0 + i] = seg[i];
    __syncthreads();
  }
  if (tid == 0) sm_last = acc;
  __syncthreads();  // (also: every thread re-reads elements other threads wrote)
  const double carry = sm_last;
  if (relative == 2) return;  // raw cumulative path length (SharedSeedCache entry)
  const double last = carry;
  double mn = INFINITY, mx = -INFINITY;
  for (int64_t t0 = 0; t0 < T; t0 += 512)
    for (int e = 0; e < 2; ++e) {
      const int64_t t = t0 + tid * 2 + e;
      if (t < T) {
        double v = o[t];
        if (relative) v = v / (last + 1e-5);
        mn = fmin(mn, v);
        mx = fmax(mx, v);
      }
    }
  mn = block_reduce_minmax(mn, false, sm_red);
  mx = block_reduce_minmax(mx, true, sm_red);
  for (int64_t t0 = 0; t0 < T; t0 += 512)
    for (int e = 0; e < 2; ++e) {
      const int64_t t = t0 + tid * 2 + e;
      if (t < T) {
        double v = o[t];
        if (relative) v = v / (last + 1e-5);
        o[t] = (mn != mx) ? ((v - mn) / (mx - mn)) * scale : 0.0 * scale;
      }
    }
}

// STD preparateur, separately=True (fruits/preparation/transform.py:141-147):
// per (series, dimension) row: (x - mean) / (std + eps), std = population std
// (np.std), or 1 when var=False.  mean = np.add.reduce(x) / T and
// std = sqrt(np.add.reduce((x - mean)^2) / T) in NUMPY'S summation order (pairwise.h):
// the statistics, and with them every standardised value, are bit-identical to the
// reference's - a last-bit difference here flips the plateau ties of the max-plus
// semirings behind it.
// `lengths` (per series, D rows each; nullptr: every row is T long): the statistics of row r are
// those of its first L = lengths[r / D] elements, summed in numpy's order FOR THAT LENGTH - what a
// call on the truncated series computes, bit for bit; the tail [L, T) of the output is 0.
__global__ __launch_bounds__(256) void standardize_kernel(const double *__restrict__ X, int64_t row_len,
                                                           const int32_t *__restrict__ lengths, int64_t D,
                                                           int div_std, double eps,
                                                           double *__restrict__ out) {
#pragma clang fp contract(off)
  __shared__ PairwiseShared sh;
  const double *x = X + (int64_t)blockIdx.x * row_len;
  double *o = out + (int64_t)blockIdx.x * row_len;
  const int64_t T = lengths ? (int64_t)lengths[(int64_t)blockIdx.x / D] : row_len;
  const double mean = np_sum_row([&](int64_t t) { return x[t]; }, T, sh) / (double)T;
  double sd = 1.0;
  if (div_std) {
    const double v = np_sum_row(
        [&](int64_t t) {
          const double d = x[t] - mean;
          return d * d;
        },
        T, sh);
    sd = sqrt(v / (double)T);
  }
  const double den = sd + eps;
  for (int64_t t = threadIdx.x; t < T; t += blockDim.x) o[t] = (x[t] - mean) / den;
  for (int64_t t = T + threadIdx.x; t < row_len; t += blockDim.x) o[t] = 0.0;
}

// Statistics of the PREPARED rows for the fused preparation of the walk kernel (walk.h):
// prepared dimension d' = prep[4 d'] (raw dimension), prep[4 d' + 1] (increment lag, 0 none).
// The same sums in the same order as standardize_kernel over the materialised rows (numpy's),
// so the fused pipeline reproduces the unfused one, and both the reference, bit for bit.
// stats[(n * n_prep + d') * 2] = mean, [.. + 1] = std + eps (1 + eps when div_std == 0).
// `lengths` (nullptr: none): series n is its first lengths[n] elements (standardize_kernel).
__global__ __launch_bounds__(256) void row_stats_kernel(const double *__restrict__ X, int64_t D,
                                                         int64_t row_len, const int32_t *__restrict__ lengths,
                                                         const int32_t *__restrict__ prep,
                                                         int n_prep, int div_std, double eps,
                                                         double *__restrict__ stats) {
#pragma clang fp contract(off)
  __shared__ PairwiseShared sh;
  const int64_t n = blockIdx.x / n_prep;
  const int dp = (int)(blockIdx.x % n_prep);
  const int raw = prep[4 * dp], lag = prep[4 * dp + 1];
  const double *x = X + (n * D + raw) * row_len;
  const int64_t T = lengths ? (int64_t)lengths[n] : row_len;
  auto value = [&](int64_t t) -> double {
    if (lag <= 0) return x[t];
    return t >= lag ? x[t] - x[t - lag] : 0.0;
  };
  const double mean = np_sum_row(value, T, sh) / (double)T;
  double sd = 1.0;
  if (div_std) {
    const double v = np_sum_row(
        [&](int64_t t) {
          const double d = value(t) - mean;
          return d * d;
        },
        T, sh);
    sd = sqrt(v / (double)T);
  }
  if (threadIdx.x == 0) {
    stats[(n * n_prep + dp) * 2] = mean;
    stats[(n * n_prep + dp) * 2 + 1] = sd + eps;
  }
}

hipError_t launch_row_stats(const double *X, int64_t N, int64_t D, int64_t T, const int32_t *lengths,
                            const int32_t *prep, int n_prep, int div_std, double eps, double *stats,
                            hipStream_t st) {
  if (N <= 0 || T <= 0 || n_prep <= 0) return hipSuccess;
  if (N * n_prep > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(row_stats_kernel, dim3((unsigned)(N * n_prep)), dim3(256), 0, st, X, D, T,
                     lengths, prep, n_prep, div_std, eps, stats);
  return hipGetLastError();
}

// _ffn of fruits/iss/cos.py:93-113 for one (word, frequency): per time step
// Z = C relu(A x + b), sums over the input / hidden dimension in index order (numba's
// np.sum), Y * (Y > 0) as the ReLU.  One thread per (series, time step).
constexpr int kFfnMaxHidden = 64, kFfnMaxDims = 16;
__global__ void coswiss_ffn_kernel(const double *__restrict__ X, int64_t N, int64_t D, int64_t T,
                                   const double *__restrict__ A, const double *__restrict__ b,
                                   const double *__restrict__ Cm, int hidden,
                                   double *__restrict__ Z) {
#pragma clang fp contract(off)
  const int64_t total = N * T;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t n = i / T, t = i - n * T;
    double x[kFfnMaxDims], y[kFfnMaxHidden];
    for (int d = 0; d < D; ++d) x[d] = X[(n * D + d) * T + t];
    for (int h = 0; h < hidden; ++h) {
      double acc = 0.0;
      for (int d = 0; d < D; ++d) acc = acc + A[h * D + d] * x[d];
      const double v = acc + b[h];
      y[h] = v * (v > 0.0 ? 1.0 : 0.0);
    }
    for (int d = 0; d < D; ++d) {
      double acc = 0.0;
      for (int h = 0; h < hidden; ++h) acc = acc + Cm[d * hidden + h] * y[h];
      Z[(n * D + d) * T + t] = acc;
    }
  }
}

hipError_t launch_coswiss_ffn(const double *X, int64_t N, int64_t D, int64_t T, const double *A,
                              const double *b, const double *Cm, int hidden, double *Z,
                              hipStream_t st) {
  const int64_t total = N * T;
  if (total <= 0) return hipSuccess;
  if (hidden < 1 || hidden > kFfnMaxHidden || D < 1 || D > kFfnMaxDims) return hipErrorInvalidValue;
  hipLaunchKernelGGL(coswiss_ffn_kernel, dim3(grid_blocks(total, 256 * 16)), dim3(256), 0, st, X, N, D, T, A, b,
                     Cm, hidden, Z);
  return hipGetLastError();
}

// sin / cos tables of fruits/iss/cos.py:23-24; the float32 frequency is promoted to
// double before the product with T-1 (numba's typing of the reference's f4 argument)
__global__ void trig_tables_kernel(const float *__restrict__ freqs, int F, int64_t T,
                                   double *__restrict__ out) {
  const int64_t total = (int64_t)F * T;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t f = i / T, t = i % T;
    const double ang = (3.14159265358979323846 * (double)t) / ((double)freqs[f] * (double)(T - 1));
    out[(f * 2) * T + t] = sin(ang);
    out[(f * 2 + 1) * T + t] = cos(ang);
  }
}

hipError_t launch_trig_tables(const float *freqs, int F, int64_t T, double *out, hipStream_t st) {
  const int64_t total = (int64_t)F * T;
  if (total <= 0) return hipSuccess;
  hipLaunchKernelGGL(trig_tables_kernel, dim3(grid_blocks(total, 1024)), dim3(256), 0, st, freqs, F, T,
                     out);
  return hipGetLastError();
}

// MPI features: mean = sum / population (0 for an empty band, increment.py:158-161).
// `pairs` (npi column, mpi column inside one iterated sum's block): NPI features whose
// band, cut and differencing order equal an MPI feature's ARE that population - the walk
// kernel skipped them (fr_pipeline_set_quantiles) and they are filled in here.
__global__ void mpi_finalize_kernel(double *__restrict__ feats, const double *__restrict__ cnt,
                                    int64_t N, int64_t stride, const int32_t *__restrict__ cols,
                                    int n_cols, const int32_t *__restrict__ pairs, int n_pairs,
                                    int per_sum, int K) {
  const int64_t per_n = (int64_t)K * (n_cols + n_pairs);
  const int64_t total = N * per_n;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t n = i / per_n;
    const int64_t r = i % per_n;
    const int64_t k = r / (n_cols + n_pairs);
    const int j = (int)(r % (n_cols + n_pairs));
    if (j < n_cols) {
      const int64_t f = k * per_sum + cols[j];
      const double c = cnt[n * stride + f];
      feats[n * stride + f] = c > 0.0 ? feats[n * stride + f] / c : 0.0;
    } else {
      const int p = j - n_cols;
      feats[n * stride + k * per_sum + pairs[2 * p]] = cnt[n * stride + k * per_sum + pairs[2 * p + 1]];
    }
  }
}

hipError_t launch_mpi_finalize(double *feats, const double *cnt, int64_t N, int64_t stride,
                               const int32_t *cols, int n_cols, const int32_t *pairs, int n_pairs,
                               int per_sum, int K, hipStream_t st) {
  const int64_t total = N * (int64_t)K * (n_cols + n_pairs);
  if (total <= 0) return hipSuccess;
  hipLaunchKernelGGL(mpi_finalize_kernel, dim3(grid_blocks(total, 4096)), dim3(256), 0, st, feats, cnt, N,
                     stride, cols, n_cols, pairs, n_pairs, per_sum, K);
  return hipGetLastError();
}

// MAX / MIN features of the fused walk: the band keys (walk_types.h) it left as the columns' bits
// become values, key 0 (an empty band or segment) 0.0.  cols: the MAX columns inside one
// iterated sum's block, ~column for MIN.
__global__ void band_key_finalize_kernel(double *__restrict__ feats, int64_t N, int64_t stride,
                                         const int32_t *__restrict__ cols, int n_cols, int per_sum,
                                         int K) {
  const int64_t per_n = (int64_t)K * n_cols;
  const int64_t total = N * per_n;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t n = i / per_n, r = i % per_n;
    const int64_t k = r / n_cols;
    const int c = cols[r % n_cols];
    double *f = feats + n * stride + k * per_sum + (c < 0 ? ~c : c);
    *f = band_key_value(__builtin_bit_cast(uint64_t, *f), c < 0);
  }
}

hipError_t launch_band_key_finalize(double *feats, int64_t N, int64_t stride, const int32_t *cols,
                                    int n_cols, int per_sum, int K, hipStream_t st) {
  const int64_t total = N * (int64_t)K * n_cols;
  if (total <= 0) return hipSuccess;
  hipLaunchKernelGGL(band_key_finalize_kernel, dim3(grid_blocks(total, 4096)), dim3(256), 0, st, feats, N,
                     stride, cols, n_cols, per_sum, K);
  return hipGetLastError();
}

// PPV / CPV columns of a fused launch hold COUNTS (the indicator's population, ~column: its
// rising edges): the one division of fruits/sieving/implicit.py:124-128, 182 - count / T, or
// 2 * count / n with n = T rounded up to even - exactly as the standalone kernel forms it.
// `lengths` (nullptr: none): series n was counted over its first lengths[n] elements, which is
// then the T of its divisions.
__global__ void implicit_finalize_kernel(double *__restrict__ feats, int64_t N, int64_t stride,
                                         const int32_t *__restrict__ cols, int n_cols, int per_sum,
                                         int K, int64_t row_len, const int32_t *__restrict__ lengths) {
  const int64_t per_n = (int64_t)K * n_cols;
  const int64_t total = N * per_n;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t n = i / per_n, r = i % per_n;
    const int64_t k = r / n_cols;
    const int c = cols[r % n_cols];
    const int64_t T = lengths ? (int64_t)lengths[n] : row_len;
    double *f = feats + n * stride + k * per_sum + (c < 0 ? ~c : c);
    *f = c < 0 ? (2.0 * *f) / (double)(T + (T & 1)) : *f / (double)T;
  }
}

hipError_t launch_implicit_finalize(double *feats, int64_t N, int64_t stride, const int32_t *cols,
                                    int n_cols, int per_sum, int K, int64_t T, const int32_t *lengths,
                                    hipStream_t st) {
  const int64_t total = N * (int64_t)K * n_cols;
  if (total <= 0) return hipSuccess;
  hipLaunchKernelGGL(implicit_finalize_kernel, dim3(grid_blocks(total, 4096)), dim3(256), 0, st, feats, N,
                     stride, cols, n_cols, per_sum, K, T, lengths);
  return hipGetLastError();
}

// A plan in pieces leaves its features in WALK order (plan.h, PiecedProgram): the blocks of
// `per_sum` columns of one iterated sum back into the reference's row order,
// dst[n, k * per_sum + j] = src[n, walk_of_row[k] * per_sum + j].  Writes are coalesced, reads
// gather 8 * per_sum byte runs inside the series' row (a few KB: cache hits).
__global__ __launch_bounds__(256) void gather_row_blocks_kernel(const double *__restrict__ src,
                                                                 double *__restrict__ dst, int64_t N,
                                                                 int64_t src_stride, int64_t dst_stride,
                                                                 int K, int per_sum,
                                                                 const int32_t *__restrict__ walk_of_row) {
  const int64_t F = (int64_t)K * per_sum;
  const int64_t total = N * F;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t n = i / F;
    const int c = (int)(i - n * F);
    const int k = c / per_sum, j = c - k * per_sum;
    dst[n * dst_stride + c] = src[n * src_stride + (int64_t)walk_of_row[k] * per_sum + j];
  }
}

hipError_t launch_gather_row_blocks(const double *src, double *dst, int64_t N, int64_t src_stride,
                                    int64_t dst_stride, int K, int per_sum, const int32_t *walk_of_row,
                                    hipStream_t st) {
  const int64_t total = N * (int64_t)K * per_sum;
  if (total <= 0) return hipSuccess;
  hipLaunchKernelGGL(gather_row_blocks_kernel, dim3(grid_blocks(total, 256 * 32)), dim3(256), 0, st, src, dst, N,
                     src_stride, dst_stride, K, per_sum, walk_of_row);
  return hipGetLastError();
}

hipError_t launch_exp_tables(const double *g, int64_t count, const float *alphas, int n_alpha,
                             double *aux, bool linear, hipStream_t st) {
  if (count <= 0 || n_alpha <= 0) return hipSuccess;
  const int bs = 256;
  hipLaunchKernelGGL(exp_tables_kernel, dim3((unsigned)((count + bs - 1) / bs)), dim3(bs), 0, st,
                     g, count, alphas, n_alpha, aux, linear ? 1 : 0);
  return hipGetLastError();
}

hipError_t launch_increments(const double *X, int64_t rows, int64_t T, int64_t shift, double *out,
                             const double *head_src, int64_t head, hipStream_t st) {
  const int64_t total = rows * T;
  if (total <= 0) return hipSuccess;
  hipLaunchKernelGGL(increments_kernel, dim3(grid_blocks(total, 256 * 16)), dim3(256), 0, st, X, rows, T,
                     shift, out, head_src, head);
  return hipGetLastError();
}

hipError_t launch_pathlen_lookup(const double *X, int64_t N, int64_t D, int64_t T, int norm,
                                 int relative, double scale, int exact, double *out,
                                 hipStream_t st) {
  if (N <= 0 || T <= 0) return hipSuccess;
  hipLaunchKernelGGL(pathlen_lookup_kernel, dim3((unsigned)N), dim3(256), 0, st, X, D, T, norm,
                     relative, scale, exact, out);
  return hipGetLastError();
}

// CosWISS term reduction (fruits/iss/cos.py:38-48): block (j, n) sums the terms of output
// row j for series n in the reference's order, `res += coeff * (tmp * sin^a * cos^b)`.
__global__ __launch_bounds__(256) void coswiss_combine_kernel(
    const double *__restrict__ A, int64_t N, int64_t T, const int32_t *__restrict__ begin,
    const double *__restrict__ coeff, const int32_t *__restrict__ desc,
    const double *__restrict__ trig, double *__restrict__ out, int64_t out_row_stride) {
#pragma clang fp contract(off)
  const int64_t j = blockIdx.x / N, n = blockIdx.x % N;
  const int i0 = begin[j], i1 = begin[j + 1];
  for (int64_t t = threadIdx.x; t < T; t += 256) {
    const double sn = trig[t], cs = trig[T + t];
    double acc = 0.0;
    for (int i = i0; i < i1; ++i) {
      double v = A[((int64_t)desc[3 * i] * N + n) * T + t];
      for (int k = desc[3 * i + 1]; k > 0; --k) v = v * sn;
      for (int k = desc[3 * i + 2]; k > 0; --k) v = v * cs;
      acc += coeff[i] * v;
    }
    out[j * out_row_stride + n * T + t] = acc;
  }
}

hipError_t launch_coswiss_combine(const double *A, int64_t N, int64_t T, int n_out,
                                  const int32_t *begin, const double *coeff, const int32_t *desc,
                                  const double *trig, double *out, int64_t out_row_stride,
                                  hipStream_t st) {
  if (N <= 0 || T <= 0 || n_out <= 0) return hipSuccess;
  hipLaunchKernelGGL(coswiss_combine_kernel, dim3((unsigned)(N * n_out)), dim3(256), 0, st, A, N,
                     T, begin, coeff, desc, trig, out, out_row_stride);
  return hipGetLastError();
}

// np.nan_to_num(features, nan=0.0) of Fruit.transform (fruits/fruit.py:172): NaN -> 0,
// +-inf -> the largest / lowest finite double
__global__ void nan_to_num_kernel(double *__restrict__ x, int64_t count) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count;
       i += (int64_t)gridDim.x * blockDim.x) {
    const double v = x[i];
    if (v != v) x[i] = 0.0;
    else if (v == __builtin_inf()) x[i] = 1.7976931348623157e308;
    else if (v == -__builtin_inf()) x[i] = -1.7976931348623157e308;
  }
}

hipError_t launch_nan_to_num(double *x, int64_t count, hipStream_t st) {
  if (count <= 0) return hipSuccess;
  hipLaunchKernelGGL(nan_to_num_kernel, dim3(grid_blocks(count, 256 * 16)), dim3(256), 0, st, x, count);
  return hipGetLastError();
}

hipError_t launch_standardize(const double *X, int64_t rows, int64_t T, const int32_t *lengths,
                              int64_t D, int div_std, double eps, double *out, hipStream_t st) {
  if (rows <= 0 || T <= 0) return hipSuccess;
  hipLaunchKernelGGL(standardize_kernel, dim3((unsigned)rows), dim3(256), 0, st, X, T, lengths,
                     D > 0 ? D : 1, div_std, eps, out);
  return hipGetLastError();
}

}  // namespace fr
