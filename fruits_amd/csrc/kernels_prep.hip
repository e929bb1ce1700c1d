// The preparateurs beyond INC / STD: RIN and MAV (one grouped causal FIR), JLD and FFN (one
// per-time-step map across dimensions), NRM (row min / max + rescale) and LAG (lead-lag
// interleave).  fruits/preparation/transform.py:161-568, 616-746.  fp64, no a*b+c contraction
// (the reference rounds every product before it adds it).  All kernels read (N, D, T) C-order
// rows and never write their input.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "pairwise.h"
#include "walk_scan.h"

namespace fr {

// ---------------------------------------------------------------- RIN / MAV: grouped causal FIR
// RIN._backend (transform.py:447-468): output dimension o owns the slots j in [start_o, end_o)
// (prefix sums of ndim) and
//   out[n,o,k] = sum_j ( X[n, j, k] - sum_{l<w} X[n, dims[j], k-w+l] * kernel[j,l] ),  k >= w,
// 0 for k < w.  The self term is X[i, j, k] - dimension j, NOT dims[j] (transform.py:465).
// The additions run in the reference's order: slot by slot, tap by tap, then the self term.
// adaptive (transform.py:536-543): the same on an input with w leading zeros, the first w
// outputs dropped - an index offset and a bounds select, no padded copy.
// MAV._backend (transform.py:233-239), mode 1: no self term, all taps 1, one slot per
// dimension, out[k-1] = (sum of X[k-w .. k-1]) / w for k = w .. T; the window is summed
// directly (a difference of prefix sums cancels on long series).
//
// One workgroup per (series, output dimension, tile of kFirTile outputs); a lane owns two
// consecutive outputs (one 16-byte store where the row is aligned).  Of every source row the
// tile + taps window goes through LDS, kFirTaps taps at a time, so w is unbounded with a
// fixed 8 KB of LDS.  Taps, ndim and dims are wave-uniform and read through the constant
// address space: scalar loads, which do not wait for the stores in flight (walk_scan.h).
constexpr int kFirTile = 512, kFirTaps = 512;

__global__ __launch_bounds__(256) void prep_fir_kernel(
    const double *__restrict__ X, int64_t D, int64_t T, const double *__restrict__ taps_, int w,
    const int32_t *__restrict__ ndim_, int O, const int32_t *__restrict__ dims_, int mode,
    int adaptive, double *__restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double buf[kFirTile + kFirTaps];
  const cptr<double> taps = as_const(taps_);
  const cptr<int32_t> ndim = as_const(ndim_), dims = as_const(dims_);
  const int64_t n = (int64_t)blockIdx.x / O;
  const int o = (int)((int64_t)blockIdx.x % O);
  const int64_t t0 = (int64_t)blockIdx.y * kFirTile;
  const int tid = (int)threadIdx.x;
  const int64_t t = t0 + 2 * tid;
  int j0 = o, j1 = o + 1;
  if (mode == 0) {
    j0 = 0;
    for (int i = 0; i < o; ++i) j0 += ndim[i];
    j1 = j0 + ndim[o];
  }
  const int shift = mode == 1 ? 1 : 0;   // MAV's window ends AT the output element
  double acc0 = 0.0, acc1 = 0.0;
  for (int j = j0; j < j1; ++j) {
    const int src = mode == 0 ? dims[j] : j;
    const double *__restrict__ x = X + (n * D + src) * T;
    for (int l0 = 0; l0 < w; l0 += kFirTaps) {
      const int wc = w - l0 < kFirTaps ? w - l0 : kFirTaps;
      // buf[p] = x[g0 + p], p < tile + wc - 1; zero outside the row (the padded head of the
      // adaptive form; everything else out of range belongs to outputs that are not stored)
      const int64_t g0 = t0 - w + l0 + shift;
      __syncthreads();
      for (int p = tid; p < kFirTile + wc - 1; p += 256) {
        const int64_t g = g0 + p;
        buf[p] = (g >= 0 && g < T) ? x[g] : 0.0;
      }
      __syncthreads();
      double v0 = buf[2 * tid], v1;
      if (mode == 0) {
        for (int li = 0; li < wc; ++li) {
          v1 = buf[2 * tid + li + 1];
          const double k = taps[(int64_t)j * w + l0 + li];
          acc0 = acc0 - v0 * k;
          acc1 = acc1 - v1 * k;
          v0 = v1;
        }
      } else {
        for (int li = 0; li < wc; ++li) {
          v1 = buf[2 * tid + li + 1];
          acc0 = acc0 + v0;
          acc1 = acc1 + v1;
          v0 = v1;
        }
      }
    }
    if (mode == 0) {
      const double *__restrict__ self = X + (n * D + j) * T;   // (transform.py:465: j, not dims[j])
      if (t < T) acc0 = acc0 + self[t];
      if (t + 1 < T) acc1 = acc1 + self[t + 1];
    }
  }
  if (mode == 1) {
    acc0 = acc0 / (double)w;
    acc1 = acc1 / (double)w;
  }
  const int64_t first = mode == 1 ? (int64_t)w - 1 : (adaptive ? 0 : (int64_t)w);
  if (t < first) acc0 = 0.0;
  if (t + 1 < first) acc1 = 0.0;
  double *__restrict__ orow = out + (n * O + o) * T;
  if (t + 1 < T && (T & 1) == 0 && (reinterpret_cast<uintptr_t>(out) & 15u) == 0) {
    vd2 v;
    v.x = acc0;
    v.y = acc1;
    *reinterpret_cast<vd2 *>(orow + t) = v;
  } else {
    if (t < T) orow[t] = acc0;
    if (t + 1 < T) orow[t + 1] = acc1;
  }
}

hipError_t launch_prep_fir(const double *X, int64_t N, int64_t D, int64_t T, const double *taps,
                           int w, const int32_t *ndim, int O, const int32_t *dims, int mode,
                           int adaptive, double *out, hipStream_t st) {
  if (N <= 0 || T <= 0 || O <= 0) return hipSuccess;
  const int64_t tiles = (T + kFirTile - 1) / kFirTile;
  if (N * O > 0x7fffffffLL || tiles > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(prep_fir_kernel, dim3((unsigned)(N * O), (unsigned)tiles), dim3(256), 0, st, X,
                     D, T, taps, w, ndim, O, dims, mode, adaptive, out);
  return hipGetLastError();
}

// ---------------------------------------------------------------- JLD / FFN: map across dimensions
// JLD._backend (transform.py:651-670), hidden == 0:
//   out[n,o,t] = sum_{j in group o} ( X[n, dims[j], t] * kernel[j] + bias[o] )
// - the bias sits INSIDE the sum over j (a group of c slots adds c * bias[o], :666-668).
// FFN._transform (transform.py:362-376), hidden > 0: h = relu(W1 (x - mean) + b),
// out = W2 h, optional output relu; relu(v) = v * (v > 0), a multiply like the reference's
// (it keeps -0.0 and NaN).  mean = np.mean over time per row in numpy's summation order
// (pairwise.h), so the centred input is the reference's bit for bit.
// VALU, no MFMA: for the D <= 16 of every shape in this project the kernel is bound by
// reading X once and writing the O output rows; a matrix-core path for JLD at hundreds of
// dimensions is a different kernel.
// One workgroup per (series, tile of kProjTile time steps), a lane per time step.  For
// D <= kProjMaxDims the tile of every input dimension is staged in LDS once (centred for FFN)
// and each output reads it from there; a wider JLD reads its rows from global memory.
constexpr int kProjTile = 256, kProjMaxDims = 16, kProjMaxOut = 16;

__global__ __launch_bounds__(256) void prep_project_kernel(
    const double *__restrict__ X, int64_t D, int64_t T, const double *__restrict__ kernel_,
    const double *__restrict__ bias_, const int32_t *__restrict__ ndim_, int O,
    const int32_t *__restrict__ dims_, const double *__restrict__ W1_, const double *__restrict__ b1_,
    const double *__restrict__ W2_, int hidden, int flags, int64_t tile_len,
    double *__restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double xs[kProjMaxDims * kProjTile];
  __shared__ double mean[kProjMaxDims];
  __shared__ PairwiseShared sh;
  const cptr<double> kernel = as_const(kernel_), bias = as_const(bias_);
  const cptr<double> W1 = as_const(W1_), b1 = as_const(b1_), W2 = as_const(W2_);
  const cptr<int32_t> ndim = as_const(ndim_), dims = as_const(dims_);
  const int64_t n = blockIdx.x;
  const int tid = (int)threadIdx.x;
  const double *__restrict__ xn = X + n * D * T;
  const bool staged = D <= kProjMaxDims;
  const bool center = hidden > 0 && (flags & 1);
  if (center) {
    for (int d = 0; d < (int)D; ++d) {
      const double *row = xn + (int64_t)d * T;
      const double m = np_sum_row([&](int64_t i) { return row[i]; }, T, sh) / (double)T;
      if (tid == 0) mean[d] = m;
    }
  }
  const int64_t begin = (int64_t)blockIdx.y * tile_len;
  const int64_t end = begin + tile_len < T ? begin + tile_len : T;
  for (int64_t t0 = begin; t0 < end; t0 += kProjTile) {
    const int64_t t = t0 + tid;
    __syncthreads();
    if (staged && t < end)
      for (int d = 0; d < (int)D; ++d) {
        const double v = xn[(int64_t)d * T + t];
        xs[d * kProjTile + tid] = center ? v - mean[d] : v;
      }
    // (a lane reads only what it staged itself: no barrier behind the staging)
    if (t >= end) continue;
    if (hidden == 0) {
      int j = 0;
      for (int o = 0; o < O; ++o) {
        const int je = j + ndim[o];
        const double b = bias[o];
        double acc = 0.0;
        for (; j < je; ++j) {
          const int d = dims[j];
          const double v = staged ? xs[d * kProjTile + tid] : xn[(int64_t)d * T + t];
          acc = acc + (v * kernel[j] + b);
        }
        out[(n * O + o) * T + t] = acc;
      }
    } else {
      double acc[kProjMaxOut];
#pragma unroll
      for (int o = 0; o < kProjMaxOut; ++o) acc[o] = 0.0;
      for (int h = 0; h < hidden; ++h) {
        double s = 0.0;
        for (int d = 0; d < (int)D; ++d) s = s + W1[(int64_t)h * D + d] * xs[d * kProjTile + tid];
        const double v = s + b1[h];
        const double y = v * (v > 0.0 ? 1.0 : 0.0);
#pragma unroll
        for (int o = 0; o < kProjMaxOut; ++o)
          if (o < O) acc[o] = acc[o] + W2[(int64_t)o * hidden + h] * y;
      }
#pragma unroll
      for (int o = 0; o < kProjMaxOut; ++o)
        if (o < O) {
          double v = acc[o];
          if (flags & 2) v = v * (v > 0.0 ? 1.0 : 0.0);
          out[(n * O + o) * T + t] = v;
        }
    }
  }
}

hipError_t launch_prep_project(const double *X, int64_t N, int64_t D, int64_t T,
                               const double *kernel, const double *bias, const int32_t *ndim, int O,
                               const int32_t *dims, const double *W1, const double *b1,
                               const double *W2, int hidden, int flags, double *out,
                               hipStream_t st) {
  if (N <= 0 || T <= 0 || O <= 0) return hipSuccess;
  if (hidden > 0 && (D > kProjMaxDims || O > kProjMaxOut)) return hipErrorInvalidValue;
  // a centred FFN needs the row means first: one workgroup walks the whole series
  const bool center = hidden > 0 && (flags & 1);
  const int64_t tile_len = center ? T : 4 * kProjTile;
  const int64_t tiles = (T + tile_len - 1) / tile_len;
  if (N > 0x7fffffffLL || tiles > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(prep_project_kernel, dim3((unsigned)N, (unsigned)tiles), dim3(256), 0, st, X, D,
                     T, kernel, bias, ndim, O, dims, W1, b1, W2, hidden, flags, tile_len, out);
  return hipGetLastError();
}

// ---------------------------------------------------------------- NRM
// NRM._transform (transform.py:184-198): (x - min) / (max - min) per row of `len` elements
// (a (series, dimension) row, or with scale_dim the D * T contiguous elements of a series);
// rows with min == max become 0.  np.min / np.max propagate NaN, so do these.  A row of up to
// kNrmChunk elements stays in LDS between the reduction and the rescale: X is read once.
// Subtraction and division are correctly rounded: bit-identical to the reference.
constexpr int kNrmChunk = 4096;
__device__ __forceinline__ double nan_min(double a, double b) { return (a != a || a < b) ? a : b; }
__device__ __forceinline__ double nan_max(double a, double b) { return (a != a || a > b) ? a : b; }

__global__ __launch_bounds__(256) void prep_normalize_kernel(const double *__restrict__ X,
                                                              int64_t len,
                                                              double *__restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double row[kNrmChunk];
  __shared__ double red[2][4];
  const double *__restrict__ x = X + (int64_t)blockIdx.x * len;
  double *__restrict__ o = out + (int64_t)blockIdx.x * len;
  const int tid = (int)threadIdx.x;
  const bool fits = len <= kNrmChunk;
  double mn = x[0], mx = mn;   // (len >= 1)
  for (int64_t i = tid; i < len; i += 256) {
    const double v = x[i];
    if (fits) row[i] = v;
    mn = nan_min(mn, v);
    mx = nan_max(mx, v);
  }
  for (int s = 32; s > 0; s >>= 1) {
    mn = nan_min(mn, __shfl_xor(mn, s));
    mx = nan_max(mx, __shfl_xor(mx, s));
  }
  if ((tid & 63) == 0) {
    red[0][tid >> 6] = mn;
    red[1][tid >> 6] = mx;
  }
  __syncthreads();
  mn = red[0][0];
  mx = red[1][0];
  for (int wv = 1; wv < 4; ++wv) {
    mn = nan_min(mn, red[0][wv]);
    mx = nan_max(mx, red[1][wv]);
  }
  const bool flat = !(mn != mx);
  const double den = mx - mn;
  for (int64_t i = tid; i < len; i += 256) {
    const double v = fits ? row[i] : x[i];
    o[i] = flat ? 0.0 : (v - mn) / den;
  }
}

hipError_t launch_prep_normalize(const double *X, int64_t rows, int64_t len, double *out,
                                 hipStream_t st) {
  if (rows <= 0 || len <= 0) return hipSuccess;
  if (rows > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(prep_normalize_kernel, dim3((unsigned)rows), dim3(256), 0, st, X, len, out);
  return hipGetLastError();
}

// ---------------------------------------------------------------- LAG
// LAG._transform (transform.py:291-298): (N, D, T) -> (N, 2D, 2T - 1); row 2i is the lead
// x[(s + 1) / 2], row 2i + 1 the lag x[s / 2] of input row i.  Pure data movement: consecutive
// lanes store consecutive output elements (the rows are 2T - 1 long, so 8-byte stores), the
// two reads per input element hit the same cache line.
constexpr int kLagTile = 1024;
__global__ __launch_bounds__(256) void prep_leadlag_kernel(const double *__restrict__ X, int64_t T,
                                                            double *__restrict__ out) {
  const int64_t r = blockIdx.x;         // output row: (n * D + i) * 2 + lag
  const int64_t len = 2 * T - 1;
  const double *__restrict__ x = X + (r >> 1) * T;
  double *__restrict__ o = out + r * len;
  const int lead = (r & 1) == 0 ? 1 : 0;
  const int64_t s0 = (int64_t)blockIdx.y * kLagTile;
#pragma unroll
  for (int e = 0; e < kLagTile / 256; ++e) {
    const int64_t s = s0 + e * 256 + (int)threadIdx.x;
    if (s < len) o[s] = x[(s + lead) >> 1];
  }
}

hipError_t launch_prep_leadlag(const double *X, int64_t rows, int64_t T, double *out,
                               hipStream_t st) {
  if (rows <= 0 || T <= 0) return hipSuccess;
  const int64_t tiles = (2 * T - 1 + kLagTile - 1) / kLagTile;
  if (2 * rows > 0x7fffffffLL || tiles > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(prep_leadlag_kernel, dim3((unsigned)(2 * rows), (unsigned)tiles), dim3(256), 0,
                     st, X, T, out);
  return hipGetLastError();
}

}  // namespace fr
