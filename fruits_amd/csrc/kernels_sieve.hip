// The standalone sieves on (N, T) rows and the Arctic argmax kernels, whose epilogue evaluates the
// same band tests and differencing, with their launchers.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "sieve_rows.h"

namespace fr {

// ---------------------------------------------------------------- sieves on (N,T)
// (diff_at, the value of the inc-times differenced series at t: sieve_rows.h)
__global__ __launch_bounds__(256) void sieve_kernel(int kind, const double *__restrict__ A,
                                                     int64_t T, int64_t a_stride, int inc,
                                                     const int64_t *__restrict__ cuts,
                                                     int64_t cut_rows, int C1,
                                                     const double *__restrict__ q, int Q1,
                                                     double *__restrict__ out,
                                                     int64_t out_stride) {
  __shared__ double sm_sum[4];
  __shared__ double sm_cnt[4];
  const int64_t n = blockIdx.x;
  const double *row = A + n * a_stride;
  const int64_t *cut = cuts + (cut_rows == 1 ? 0 : n * C1);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (kind == FR_SIEVE_END_K) {
    // out[n, j] = A[n, cut_{j+1} - 1]; index -1 wraps like numpy (segment.py:213-218)
    for (int j = tid; j < C1 - 1; j += blockDim.x) {
      int64_t idx = cut[j + 1] - 1;
      if (idx < 0) idx += T;
      // out of range: the reference raises IndexError (the host validates integer cuts);
      // a device cut table that slipped through yields NaN, never a stray read
      out[n * out_stride + j] = (idx >= 0 && idx < T) ? row[idx] : __builtin_nan("");
    }
    return;
  }
  const int Q = Q1 - 1;
  for (int j = 0; j < C1 - 1; ++j) {
    int64_t lo = cut[j], hi = cut[j + 1];
    if (lo < 0) lo = 0;
    if (hi > T) hi = T;
    for (int k = 0; k < Q; ++k) {
      const double qlo = q[k], qhi = q[k + 1];
      double sum = 0.0, cnt = 0.0;
      for (int64_t t = lo + tid; t < hi; t += blockDim.x) {
        const double v = diff_at(row, t, inc);
        if (qlo < v && v <= qhi) {
          // CUR (segment.py:242-260): the squares; no population, nothing divides the sum
          sum += kind == FR_SIEVE_CUR_K ? v * v : v;
          cnt += 1.0;
        }
      }
      for (int o = 32; o > 0; o >>= 1) {
        sum += __shfl_xor(sum, o);
        cnt += __shfl_xor(cnt, o);
      }
      __syncthreads();
      if (lane == 0) {
        sm_sum[wave] = sum;
        sm_cnt[wave] = cnt;
      }
      __syncthreads();
      if (tid == 0) {
        double s = 0.0, c = 0.0;
        for (int w = 0; w < 4; ++w) {
          s += sm_sum[w];
          c += sm_cnt[w];
        }
        out[n * out_stride + j * Q + k] =
            (kind == FR_SIEVE_NPI_K) ? c : (kind == FR_SIEVE_CUR_K ? s : (c > 0.0 ? s / c : 0.0));
      }
    }
  }
}

// MAX / MIN / XPI / LPI (segment.py:107-200, increment.py:166-239) on the same (N,T) rows:
// one workgroup per series, every (segment, band) in turn.  MAX / MIN reduce band_key()s (an
// order-preserving integer form of the value, walk_types.h: 0 = empty), XPI sums the in-band
// positions relative to the segment start (integers: exact in any order) and their count.
// LPI gives every thread a CONTIGUOUS tile of the segment and merges (leading run, trailing
// run, longest run, length, all in band) summaries in thread order, then in wave order.
struct RunSummary {
  int64_t pre, suf, best, len;   // (all in band  <=>  pre == len)
};
__device__ __forceinline__ RunSummary run_merge(const RunSummary &a, const RunSummary &b) {
  RunSummary r;
  r.pre = a.pre == a.len ? a.len + b.pre : a.pre;
  r.suf = b.suf == b.len ? b.len + a.suf : b.suf;
  r.best = a.best > b.best ? a.best : b.best;
  if (a.suf + b.pre > r.best) r.best = a.suf + b.pre;
  r.len = a.len + b.len;
  return r;
}

__global__ __launch_bounds__(256) void band_sieve_kernel(int kind, const double *__restrict__ A,
                                                         int64_t T, int64_t a_stride, int inc,
                                                         const int64_t *__restrict__ cuts,
                                                         int64_t cut_rows, int C1,
                                                         const double *__restrict__ q, int Q1,
                                                         double *__restrict__ out,
                                                         int64_t out_stride) {
  __shared__ unsigned long long sm_key[4];
  __shared__ double sm_sum[4], sm_cnt[4];
  __shared__ RunSummary sm_run[4];
  const int64_t n = blockIdx.x;
  const double *row = A + n * a_stride;
  const int64_t *cut = cuts + (cut_rows == 1 ? 0 : n * C1);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Q = Q1 - 1;
  for (int j = 0; j < C1 - 1; ++j) {
    int64_t lo = cut[j], hi = cut[j + 1];
    if (lo < 0) lo = 0;
    if (hi > T) hi = T;
    for (int k = 0; k < Q; ++k) {
      const double qlo = q[k], qhi = q[k + 1];
      double res = 0.0;
      if (kind == FR_SIEVE_MAX_K || kind == FR_SIEVE_MIN_K) {
        unsigned long long key = 0;
        for (int64_t t = lo + tid; t < hi; t += blockDim.x) {
          const double v = diff_at(row, t, inc);
          if (qlo < v && v <= qhi) {
            const unsigned long long kv = band_key(v, kind == FR_SIEVE_MIN_K);
            key = kv > key ? kv : key;
          }
        }
        for (int o = 32; o > 0; o >>= 1) {
          const unsigned long long w = __shfl_xor(key, o);
          key = w > key ? w : key;
        }
        __syncthreads();
        if (lane == 0) sm_key[wave] = key;
        __syncthreads();
        if (tid == 0) {
          for (int w = 0; w < 4; ++w) key = sm_key[w] > key ? sm_key[w] : key;
          res = band_key_value(key, kind == FR_SIEVE_MIN_K);
        }
      } else if (kind == FR_SIEVE_XPI_K) {
        double sum = 0.0, cnt = 0.0;
        for (int64_t t = lo + tid; t < hi; t += blockDim.x) {
          const double v = diff_at(row, t, inc);
          if (qlo < v && v <= qhi) {
            sum += (double)(t - lo);
            cnt += 1.0;
          }
        }
        for (int o = 32; o > 0; o >>= 1) {
          sum += __shfl_xor(sum, o);
          cnt += __shfl_xor(cnt, o);
        }
        __syncthreads();
        if (lane == 0) {
          sm_sum[wave] = sum;
          sm_cnt[wave] = cnt;
        }
        __syncthreads();
        if (tid == 0) {
          double s = 0.0, c = 0.0;
          for (int w = 0; w < 4; ++w) {
            s += sm_sum[w];
            c += sm_cnt[w];
          }
          res = c > 0.0 ? s / c : 0.0;
        }
      } else {   // LPI
        const int64_t len = hi > lo ? hi - lo : 0;
        const int64_t tile = (len + blockDim.x - 1) / blockDim.x;
        int64_t a = lo + tid * tile, b = a + tile;
        if (a > hi) a = hi;
        if (b > hi) b = hi;
        RunSummary r{0, 0, 0, b - a};
        int64_t cur = 0;
        bool lead = true;
        for (int64_t t = a; t < b; ++t) {
          const double v = diff_at(row, t, inc);
          if (qlo < v && v <= qhi) {
            ++cur;
            if (cur > r.best) r.best = cur;
          } else {
            if (lead) r.pre = cur;
            lead = false;
            cur = 0;
          }
        }
        r.pre = lead ? r.len : r.pre;
        r.suf = cur;
        // lane order: lane l takes lane l + o's summary from its right
        for (int o = 1; o < 64; o <<= 1) {
          RunSummary s;
          s.pre = __shfl_down(r.pre, o);
          s.suf = __shfl_down(r.suf, o);
          s.best = __shfl_down(r.best, o);
          s.len = __shfl_down(r.len, o);
          if ((lane & (2 * o - 1)) == 0) r = run_merge(r, s);
        }
        __syncthreads();
        if (lane == 0) sm_run[wave] = r;
        __syncthreads();
        if (tid == 0) {
          r = sm_run[0];
          for (int w = 1; w < 4; ++w) r = run_merge(r, sm_run[w]);
          res = (double)r.best;
        }
      }
      if (tid == 0) out[n * out_stride + j * Q + k] = res;
    }
  }
}

// PPV / CPV (fruits/sieving/implicit.py:114-129, 169-190) on the same (N,T) rows: one workgroup
// per series, EVERY threshold of the sieve in one pass over the row.  The indicator of feature j
// is closed below - v >= q_j, or with `segments` q_j <= v < q_(j+1) evaluated per element (the
// fitted thresholds are not sorted: a band with q_j > q_(j+1) is empty) - so a NaN never counts
// and +inf counts against a finite threshold, as in numpy.  PPV counts the indicator, CPV its
// rising edges at t >= 1 (the first difference is zero-padded, fruits/cache.py:8-13: a component
// that starts at t = 0 is not counted).  Counts are integers: a wave adds its ballot's population
// to a counter of its own, the four are added in wave order, and one division forms the feature.
// `lengths` (nullptr: none): series n is its first lengths[n] elements - counted there, divided
// by that length (CPV: rounded up to even).
__device__ __forceinline__ bool implicit_in(double v, const double *__restrict__ q, int j, bool segments) {
  return segments ? (q[j] <= v && v < q[j + 1]) : (v >= q[j]);
}

__global__ __launch_bounds__(256) void implicit_sieve_kernel(int kind, const double *__restrict__ A,
                                                              int64_t row_len, int64_t a_stride,
                                                              const int32_t *__restrict__ lengths,
                                                              const double *__restrict__ q, int F,
                                                              int segments, double *__restrict__ out,
                                                              int64_t out_stride) {
  __shared__ unsigned long long sm_cnt[4][kImplicitMaxFeatures];
  const int64_t n = blockIdx.x;
  const double *row = A + n * a_stride;
  const int64_t T = lengths ? (int64_t)lengths[n] : row_len;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool cpv = kind == FR_SIEVE_CPV_K;
  for (int j = tid; j < 4 * F; j += blockDim.x) sm_cnt[j / F][j % F] = 0;
  __syncthreads();
  // (every lane takes every trip: the ballots are of whole waves)
  for (int64_t base = 0; base < T; base += blockDim.x) {
    const int64_t t = base + tid;
    const bool valid = t < T;
    const double v = valid ? row[t] : 0.0;
    const double prev = (valid && t >= 1) ? row[t - 1] : 0.0;
    for (int j = 0; j < F; ++j) {
      bool hit = valid && implicit_in(v, q, j, segments != 0);
      if (cpv) hit = hit && t >= 1 && !implicit_in(prev, q, j, segments != 0);
      const int c = __popcll(__ballot(hit));
      if (lane == 0) sm_cnt[wave][j] += (unsigned long long)c;   // (the wave's own counter)
    }
  }
  __syncthreads();
  // PPV: count / T; CPV: 2 * count / n with n = T rounded up to even (implicit.py:173-175)
  const double denom = cpv ? (double)(T + (T & 1)) : (double)T;
  for (int j = tid; j < F; j += blockDim.x) {
    const unsigned long long c = ((sm_cnt[0][j] + sm_cnt[1][j]) + sm_cnt[2][j]) + sm_cnt[3][j];
    out[n * out_stride + j] = (double)(cpv ? 2 * c : c) / denom;
  }
}

hipError_t launch_sieve_implicit(int kind, const double *A, int64_t N, int64_t T, int64_t a_stride,
                                 const int32_t *lengths, const double *q, int Q, int segments,
                                 double *out, int64_t out_stride, hipStream_t st) {
  if (N <= 0) return hipSuccess;
  const int F = segments ? Q - 1 : Q;
  if (N > 0x7fffffffLL || F < 1 || F > kImplicitMaxFeatures) return hipErrorInvalidValue;
  hipLaunchKernelGGL(implicit_sieve_kernel, dim3((unsigned)N), dim3(256), 0, st, kind, A, T, a_stride,
                     lengths, q, F, segments, out, out_stride);
  return hipGetLastError();
}

// IncrementSieve._pre_transform (inc >= 0) materialised: out[n,t] = D_inc[n,t]
__global__ void pre_transform_kernel(const double *__restrict__ A, int64_t N, int64_t T,
                                     int64_t a_stride, int inc, double *__restrict__ out) {
  const int64_t total = N * T;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t n = i / T, t = i % T;
    out[i] = diff_at(A + n * a_stride, t, inc);
  }
}

// ---------------------------------------------------------------- Arctic argmax
// Arctic(argmax=True), fruits/iss/semiring.py:239-284.  The running maxima V of every
// prefix of every word come from the walk kernel (bit-exact); this is the rest:
// (1) positions: result[2k+1, i] of the reference is the index at which the running
//     maximum was last raised (`>=` keeps the earlier index), i.e. a running maximum of
//     i * [V[i] > V[i-1]] - computable from the materialised row alone;
// (2) the back-tracking of :275-283: for prefix k (index = k + k(k+1)/2) row index is V_k,
//     row index+k+1 is P_k, and for s = k..1 row index+s is P_(s-1) frozen from the final
//     position of row index+s+1 on: R_s[t] = P_(s-1)[min(t, m_s)], m_(k+1) = T-1,
//     m_s = P_s[m_(s+1)].
__global__ __launch_bounds__(256) void argmax_positions_kernel(const double *__restrict__ V,
                                                                int64_t T,
                                                                double *__restrict__ P) {
  __shared__ double sm[256];
  const double *v = V + (int64_t)blockIdx.x * T;
  double *p = P + (int64_t)blockIdx.x * T;
  const int tid = threadIdx.x;
  const int64_t per = (T + 255) / 256, lo = tid * per, hi = lo + per < T ? lo + per : T;
  double best = 0.0;   // positions are exact small integers in a double
  for (int64_t t = lo > 0 ? lo : 1; t < hi; ++t)
    if (v[t] > v[t - 1]) best = (double)t;
  sm[tid] = best;
  __syncthreads();
  double before = 0.0;
  for (int i = 0; i < tid; ++i) before = fmax(before, sm[i]);
  double run = before;
  for (int64_t t = lo; t < hi; ++t) {
    if (t > 0 && v[t] > v[t - 1]) run = (double)t;
    p[t] = run;
  }
}

// jobs (n_jobs, 3) int32: {first V / P row of the word, level k, first output row of prefix k}
__global__ __launch_bounds__(256) void argmax_assemble_kernel(
    const double *__restrict__ V, const double *__restrict__ P, int64_t N, int64_t T,
    const int32_t *__restrict__ jobs, double *__restrict__ out) {
  __shared__ int64_t m[64];   // m_s for s = 1..k+1 (words of <= 63 letters)
  const int64_t n = blockIdx.x;
  const int32_t *jb = jobs + 3 * (int64_t)blockIdx.y;
  const int64_t row0 = jb[0], index = jb[2];
  const int k = jb[1];
  auto prow = [&](int level) { return P + ((row0 + level) * N + n) * T; };
  if (threadIdx.x == 0) {
    m[k + 1] = T - 1;
    for (int s_ = k; s_ >= 1; --s_) m[s_] = (int64_t)prow(s_)[m[s_ + 1]];
  }
  __syncthreads();
  const double *v = V + ((row0 + k) * N + n) * T;
  for (int64_t t = threadIdx.x; t < T; t += blockDim.x) {
    out[(index * N + n) * T + t] = v[t];
    for (int s_ = 1; s_ <= k + 1; ++s_) {
      const int64_t tt = t < m[s_] ? t : m[s_];
      out[((index + s_) * N + n) * T + t] = prow(s_ - 1)[tt];
    }
  }
}

hipError_t launch_arctic_argmax(const double *V, int64_t rows, int64_t N, int64_t T, int n_jobs,
                                const int32_t *jobs, double *P, double *out, hipStream_t st) {
  if (rows <= 0 || N <= 0 || T <= 0 || n_jobs <= 0) return hipSuccess;
  if (rows * N > 0x7fffffffLL || N > 0x7fffffffLL || n_jobs > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(argmax_positions_kernel, dim3((unsigned)(rows * N)), dim3(256), 0, st, V, T, P);
  hipLaunchKernelGGL(argmax_assemble_kernel, dim3((unsigned)N, (unsigned)n_jobs), dim3(256), 0, st,
                     V, P, N, T, jobs, out);
  return hipGetLastError();
}

// ---------------------------------------------------------------- Arctic argmax + sieves
// The rows of Arctic(argmax=True) straight into NPI / MPI / END features (fr_pipeline_set_argmax):
// one workgroup per (series, word).  Of a word of L letters the running maxima V_0 .. V_(L-1) of
// its prefixes exist (the walk kernel wrote them); prefix k contributes the row V_k and k + 1
// position rows (see above), L + L (L + 1) / 2 rows in all, every one a function of V alone - so
// none of them is written: V_k is staged in LDS, its positions P_k join the positions of the
// prefixes in front (LDS, 16 bits each: T < 65536), and every row is formed element by element
// for the feature ops that look at it - R_s[t] = P_(s-1)[min(t, m_s)].
struct ArgmaxWord {
  int32_t v_row0, L, out_row0, pad;
};
// values of a row: V_k, or a frozen position row
struct ArgmaxRow {
  const double *v;            // LDS: V_k, or nullptr
  const unsigned short *p;    // LDS: P_(s-1)
  int m;                      // frozen from here on
  __device__ __forceinline__ double operator()(int t) const {
    if (v) return v[t];
    return (double)p[t < m ? t : m];
  }
};
// the inc-th zero-padded difference at t (fruits/cache.py:8-13; the triangle of the selection)
template <int INC>
__device__ __forceinline__ double argmax_diff(const ArgmaxRow &r, int t) {
  double v[INC + 1];
#pragma unroll
  for (int j = 0; j <= INC; ++j) v[j] = t - j >= 0 ? r(t - j) : 0.0;
#pragma unroll
  for (int lvl = 1; lvl <= INC; ++lvl)
#pragma unroll
    for (int j = 0; j + lvl <= INC; ++j) v[j] = (t - j >= 1) ? v[j] - v[j + 1] : 0.0;
  return v[0];
}
// one band op over the row: the sum and the number of the elements t in [lo, hi) whose
// difference lies in (qlo, qhi]; the whole workgroup takes part, thread 0 gets the totals
template <int INC>
__device__ __forceinline__ void argmax_band(const ArgmaxRow &r, int lo, int hi, double qlo, double qhi,
                                            double *red, double &sum, double &cnt) {
  double s = 0.0, c = 0.0;
  for (int t = lo + (int)threadIdx.x; t < hi; t += (int)blockDim.x) {
    const double d = argmax_diff<INC>(r, t);
    if (qlo < d && d <= qhi) {
      s += d;
      c += 1.0;
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_xor(s, o);
    c += __shfl_xor(c, o);
  }
  __syncthreads();   // (red is reused op after op)
  if ((threadIdx.x & 63) == 0) {
    red[2 * (threadIdx.x >> 6)] = s;
    red[2 * (threadIdx.x >> 6) + 1] = c;
  }
  __syncthreads();
  sum = cnt = 0.0;
  if (threadIdx.x == 0)
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) {
      sum += red[2 * w];
      cnt += red[2 * w + 1];
    }
}

__global__ __launch_bounds__(256) void argmax_sieve_kernel(
    const double *__restrict__ V, int64_t N, int64_t T, const ArgmaxWord *__restrict__ words,
    const FeatOp *__restrict__ ops, int n_ops, int n_ops_padded, double *__restrict__ feats,
    double *__restrict__ cnt, int64_t feat_stride, const int32_t *__restrict__ series_cuts,
    int cut_slots) {
  extern __shared__ double dyn_lds[];
  __shared__ double red[8];
  __shared__ int part[256];
  __shared__ int m[66];   // m_s for s = 1 .. k + 1 (words of <= 63 letters)
  const int64_t n = blockIdx.x;
  const ArgmaxWord w = words[blockIdx.y];
  const int Ti = (int)T, tid = (int)threadIdx.x;
  double *vrow = dyn_lds;
  unsigned short *pos = reinterpret_cast<unsigned short *>(dyn_lds + T);   // [L][T]
  const int32_t *cut_row = series_cuts ? series_cuts + n * cut_slots : nullptr;
  double *frow = feats + n * feat_stride, *crow = cnt + n * feat_stride;
  int out_row = w.out_row0;
  for (int k = 0; k < w.L; ++k) {
    // V_k into LDS; P_k[t] = the index at which the running maximum was last raised
    const double *v = V + ((int64_t)(w.v_row0 + k) * N + n) * T;
    __syncthreads();   // (the previous prefix's ops are done with vrow)
    for (int t = tid; t < Ti; t += 256) vrow[t] = v[t];
    __syncthreads();
    unsigned short *pk = pos + (int64_t)k * T;
    const int per = (Ti + 255) / 256, lo = tid * per, hi = lo + per < Ti ? lo + per : Ti;
    int best = 0;
    for (int t = lo > 0 ? lo : 1; t < hi; ++t)
      if (vrow[t] > vrow[t - 1]) best = t;
    part[tid] = best;
    __syncthreads();
    int run = 0;
    for (int i = 0; i < tid; ++i) run = part[i] > run ? part[i] : run;
    for (int t = lo; t < hi; ++t) {
      if (t > 0 && vrow[t] > vrow[t - 1]) run = t;
      pk[t] = (unsigned short)run;
    }
    __syncthreads();
    if (tid == 0) {
      m[k + 1] = Ti - 1;
      for (int s = k; s >= 1; --s) m[s] = pos[(int64_t)s * T + m[s + 1]];
    }
    __syncthreads();
    // the k + 2 rows of this prefix: V_k, then R_1 .. R_(k+1)
    for (int s = 0; s <= k + 1; ++s, ++out_row) {
      ArgmaxRow r{s == 0 ? vrow : nullptr, s == 0 ? nullptr : pos + (int64_t)(s - 1) * T, s == 0 ? 0 : m[s]};
      const FeatOp *row_ops = ops + (int64_t)out_row * n_ops_padded;
      for (int i = 0; i < n_ops; ++i) {
        const FeatOp op = row_ops[i];
        const int kind = op.kind_inc & 0xff, inc = (int)(int8_t)((op.kind_inc >> 8) & 0xff);
        const bool cuts = (op.kind_inc & (1 << 16)) != 0;
        if (kind == FR_SIEVE_END_K) {
          int pick = op.lo;
          if (cuts) {   // X[:, cut - 1], index -1 wrapping like numpy
            pick = cut_row[op.lo] - 1;
            if (pick < 0) pick += Ti;
          }
          if (tid == 0 && pick >= 0 && pick < Ti) frow[op.col] = r(pick);   // (else: a padding op)
          continue;
        }
        int lo_t = op.lo, hi_t = op.hi;
        if (cuts) {
          lo_t = cut_row[op.lo];
          hi_t = cut_row[op.hi];
        }
        lo_t = lo_t < 0 ? 0 : lo_t;
        hi_t = hi_t > Ti ? Ti : hi_t;
        double sum, c;
        if (inc == 0) argmax_band<0>(r, lo_t, hi_t, op.qlo, op.qhi, red, sum, c);
        else if (inc == 1) argmax_band<1>(r, lo_t, hi_t, op.qlo, op.qhi, red, sum, c);
        else argmax_band<2>(r, lo_t, hi_t, op.qlo, op.qhi, red, sum, c);
        if (tid == 0) {
          if (kind == FR_SIEVE_MPI_K) {
            frow[op.col] = sum;
            crow[op.col] = c;
          } else {
            frow[op.col] = c;
          }
        }
      }
    }
  }
}

size_t argmax_sieve_lds(int64_t T, int max_len) {
  return (size_t)T * 8 + (size_t)max_len * (size_t)T * 2 + 16;
}

hipError_t launch_argmax_sieves(const double *V, int64_t N, int64_t T, const void *words, int n_words,
                                int max_len, const FeatOp *ops, int n_ops, int n_ops_padded,
                                double *feats, double *cnt, int64_t feat_stride,
                                const int32_t *series_cuts, int cut_slots, hipStream_t st) {
  if (N <= 0 || T <= 0 || n_words <= 0) return hipSuccess;
  if (N > 0x7fffffffLL || n_words > 65535 || T > 65535 || max_len > 63) return hipErrorInvalidValue;
  const size_t lds = argmax_sieve_lds(T, max_len);
  if (lds > kArgmaxSieveLds) return hipErrorInvalidValue;
  hipLaunchKernelGGL(argmax_sieve_kernel, dim3((unsigned)N, (unsigned)n_words), dim3(256), lds, st, V, N, T,
                     static_cast<const ArgmaxWord *>(words), ops, n_ops, n_ops_padded, feats, cnt,
                     feat_stride, series_cuts, cut_slots);
  return hipGetLastError();
}

hipError_t launch_sieve(int kind, const double *A, int64_t N, int64_t T, int64_t a_stride, int inc,
                        const int64_t *cuts, int64_t cut_rows, int C1, const double *q, int Q1,
                        double *out, int64_t out_stride, hipStream_t st) {
  if (N <= 0) return hipSuccess;
  if (kind >= FR_SIEVE_MAX_K && kind != FR_SIEVE_CUR_K)   // (CUR: a sum per band, like NPI / MPI)
    hipLaunchKernelGGL(band_sieve_kernel, dim3((unsigned)N), dim3(256), 0, st, kind, A, T, a_stride,
                       inc, cuts, cut_rows, C1, q, Q1, out, out_stride);
  else
    hipLaunchKernelGGL(sieve_kernel, dim3((unsigned)N), dim3(256), 0, st, kind, A, T, a_stride, inc,
                       cuts, cut_rows, C1, q, Q1, out, out_stride);
  return hipGetLastError();
}

hipError_t launch_pre_transform(const double *A, int64_t N, int64_t T, int64_t a_stride, int inc,
                                double *out, hipStream_t st) {
  const int64_t total = N * T;
  if (total <= 0) return hipSuccess;
  hipLaunchKernelGGL(pre_transform_kernel, dim3(grid_blocks(total, 256 * 16)), dim3(256), 0, st, A, N, T,
                     a_stride, inc, out);
  return hipGetLastError();
}

}  // namespace fr
