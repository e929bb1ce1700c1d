// The streaming preparateurs: the time masks of fruits/preparation/filter.py (DIL, WIN, DOT,
// PDD) and CTS(pseudo_shift=True), and the pointwise maps SPE, RPE, RDW, CTS and QTC of
// fruits/preparation/transform.py:571-613, 749-1015.  fp64, no a*b+c contraction (RPE rounds
// both products before it adds them, like the reference).  All kernels read (N, D, T) C-order
// rows and never write their input.
//
// One workgroup of 256 lanes per (row, tile of kStreamTile time steps); a lane owns two
// consecutive time steps per pass - one 16-byte access where the rows are 16-byte aligned (even
// T and an aligned base), 8-byte accesses otherwise.  Tables that are the same for a whole wave
// (a series' window, a dimension's exponent) are read through the constant address space:
// scalar loads (walk_scan.h).
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "walk_scan.h"

namespace fr {

constexpr int kStreamTile = 1024;   // two passes of 256 lane pairs

struct Pair {
  double a, b;
};

__device__ __forceinline__ bool rows_aligned(const void *p, int64_t T) {
  return (T & 1) == 0 && (reinterpret_cast<uintptr_t>(p) & 15u) == 0;
}

// elements t and t + 1 of a row (t even, t < T); b is 0 where t + 1 is outside the row
__device__ __forceinline__ Pair load_pair(const double *__restrict__ row, int64_t t, int64_t T,
                                          bool vec) {
  Pair p{0.0, 0.0};
  if (vec) {
    const vd2 v = *reinterpret_cast<const vd2 *>(row + t);
    p.a = v.x;
    p.b = v.y;
  } else {
    p.a = row[t];
    if (t + 1 < T) p.b = row[t + 1];
  }
  return p;
}

__device__ __forceinline__ void store_pair(double *__restrict__ row, int64_t t, int64_t T, bool vec,
                                           Pair p) {
  if (vec) {
    vd2 v;
    v.x = p.a;
    v.y = p.b;
    *reinterpret_cast<vd2 *>(row + t) = v;
  } else {
    row[t] = p.a;
    if (t + 1 < T) row[t + 1] = p.b;
  }
}

// ---------------------------------------------------------------- time masks
// out = keep ? X : +0.0 - a select, never a multiply: a dropped NaN, infinity or negative value
// becomes +0.0 exactly (the reference assigns 0, or copies the kept values into zeros).
// keep is the AND of two optional sources: bit t of `mask` (ceil(T / 32) words shared by all
// series: DIL, DOT, PDD, CTS(pseudo_shift=True)) and the per-series window [cs[n] - 1, ce[n])
// under Python's slice rules (WIN, filter.py:102-107: a start of -1 is T - 1).  A lane whose two
// elements are both dropped issues no load of X.
__global__ __launch_bounds__(256) void prep_mask_kernel(const double *__restrict__ X, int64_t D,
                                                         int64_t T,
                                                         const uint32_t *__restrict__ mask,
                                                         const int64_t *__restrict__ cs_,
                                                         const int64_t *__restrict__ ce_,
                                                         double *__restrict__ out) {
  const int64_t r = blockIdx.x;
  int64_t lo = 0, hi = T;
  if (cs_ != nullptr) {
    const int64_t n = r / D;
    lo = as_const(cs_)[n] - 1;
    hi = as_const(ce_)[n];
    if (lo < 0) lo += T;
    if (lo < 0) lo = 0;
    if (hi < 0) hi += T;
    if (hi < 0) hi = 0;
    if (hi > T) hi = T;
  }
  const double *__restrict__ x = X + r * T;
  double *__restrict__ o = out + r * T;
  const bool vec = rows_aligned(X, T) && rows_aligned(out, T);
  const int64_t t0 = (int64_t)blockIdx.y * kStreamTile + 2 * (int)threadIdx.x;
#pragma unroll
  for (int e = 0; e < kStreamTile / 512; ++e) {
    const int64_t t = t0 + e * 512;
    if (t >= T) continue;
    bool k0 = t >= lo && t < hi;
    bool k1 = t + 1 < T && t + 1 >= lo && t + 1 < hi;
    if (mask != nullptr && (k0 || k1)) {
      const uint32_t word = mask[t >> 5] >> (uint32_t)(t & 31);   // (t is even: bit 1 is t + 1)
      k0 = k0 && (word & 1u);
      k1 = k1 && (word & 2u);
    }
    Pair p{0.0, 0.0};
    if (vec) {
      if (k0 || k1) {
        const Pair v = load_pair(x, t, T, true);
        p.a = k0 ? v.a : 0.0;
        p.b = k1 ? v.b : 0.0;
      }
    } else {
      if (k0) p.a = x[t];
      if (k1) p.b = x[t + 1];
    }
    store_pair(o, t, T, vec, p);
  }
}

hipError_t launch_prep_mask(const double *X, int64_t N, int64_t D, int64_t T, const uint32_t *mask,
                            const int64_t *cs, const int64_t *ce, double *out, hipStream_t st) {
  if (N <= 0 || D <= 0 || T <= 0) return hipSuccess;
  const int64_t tiles = (T + kStreamTile - 1) / kStreamTile;
  if (N * D > 0x7fffffffLL || tiles > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(prep_mask_kernel, dim3((unsigned)(N * D), (unsigned)tiles), dim3(256), 0, st, X,
                     D, T, mask, cs, ce, out);
  return hipGetLastError();
}

// ---------------------------------------------------------------- pointwise maps
// One instantiation per mode (kernels.h, PW_*); the run-time switch is in the launch alone.
//   PW_MUL / PW_ADD (SPE, transform.py:789-812): X * w or X + w with w (Nw, T); the series
//     strides of X and w are 0 where that side has ONE series (numpy's broadcast of
//     X * wave[:, None, :]).  PW_FLAG_SIN: w holds the phase and the kernel takes its sine (the
//     step_transform path).  A workgroup walks all D dimensions of its series and tile, so a
//     table entry is read - and its sine taken - once per (series, time step).
//   PW_ROTATE (RPE, transform.py:859-875), D == 2: out0 = c x0 - s x1, out1 = s x0 + c x1, both
//     rows of a time step read once; c = w, s = w2, (T) each.
//   PW_POW (RDW, transform.py:601-602): X ** w[d]; a negative base with a fractional exponent
//     gives NaN, as in numpy.
//   PW_SHIFT (CTS, transform.py:939-945): out[t] = X[min(t + shift, T - 1)].
//   PW_CLIP (QTC, transform.py:990-1001): X > q ? v : X, with PW_FLAG_LOWER X < q ? v : X; a NaN
//     compares false and passes through, as with np.where.
template <int MODE>
__global__ __launch_bounds__(256) void prep_pointwise_kernel(PointwiseArgs a) {
#pragma clang fp contract(off)
  const int64_t T = a.T, D = a.D;
  const int64_t t0 = (int64_t)blockIdx.y * kStreamTile + 2 * (int)threadIdx.x;
  const bool vec = rows_aligned(a.X, T) && rows_aligned(a.out, T);
  if constexpr (MODE == PW_MUL || MODE == PW_ADD) {
    const int64_t n = blockIdx.x;
    const double *__restrict__ xn = a.X + n * a.x_stride;
    const double *__restrict__ w = a.w + n * a.w_stride;
    double *__restrict__ on = a.out + n * D * T;
    const bool wvec = rows_aligned(a.w, T);
#pragma unroll
    for (int e = 0; e < kStreamTile / 512; ++e) {
      const int64_t t = t0 + e * 512;
      if (t >= T) continue;
      Pair k = load_pair(w, t, T, wvec);
      if (a.flags & PW_FLAG_SIN) {
        k.a = sin(k.a);
        k.b = sin(k.b);
      }
      for (int64_t d = 0; d < D; ++d) {
        Pair v = load_pair(xn + d * T, t, T, vec);
        if constexpr (MODE == PW_MUL) {
          v.a = v.a * k.a;
          v.b = v.b * k.b;
        } else {
          v.a = v.a + k.a;
          v.b = v.b + k.b;
        }
        store_pair(on + d * T, t, T, vec, v);
      }
    }
  } else if constexpr (MODE == PW_ROTATE) {
    const int64_t n = blockIdx.x;
    const double *__restrict__ x0 = a.X + n * 2 * T;
    double *__restrict__ o0 = a.out + n * 2 * T;
    const bool cvec = rows_aligned(a.w, T), svec = rows_aligned(a.w2, T);
#pragma unroll
    for (int e = 0; e < kStreamTile / 512; ++e) {
      const int64_t t = t0 + e * 512;
      if (t >= T) continue;
      const Pair c = load_pair(a.w, t, T, cvec), s = load_pair(a.w2, t, T, svec);
      const Pair u = load_pair(x0, t, T, vec), v = load_pair(x0 + T, t, T, vec);
      Pair p, q;
      p.a = c.a * u.a - s.a * v.a;
      p.b = c.b * u.b - s.b * v.b;
      q.a = s.a * u.a + c.a * v.a;
      q.b = s.b * u.b + c.b * v.b;
      store_pair(o0, t, T, vec, p);
      store_pair(o0 + T, t, T, vec, q);
    }
  } else {
    const int64_t r = blockIdx.x;
    const double *__restrict__ x = a.X + r * T;
    double *__restrict__ o = a.out + r * T;
    double wd = 0.0;
    if constexpr (MODE == PW_POW) wd = as_const(a.w)[r % D];
#pragma unroll
    for (int e = 0; e < kStreamTile / 512; ++e) {
      const int64_t t = t0 + e * 512;
      if (t >= T) continue;
      Pair v;
      if constexpr (MODE == PW_SHIFT) {
        // (the source pair starts at any parity: 8-byte loads; the loads of neighbouring
        // lanes still cover whole cache lines)
        const int64_t i0 = t + a.shift < T - 1 ? t + a.shift : T - 1;
        const int64_t i1 = t + 1 + a.shift < T - 1 ? t + 1 + a.shift : T - 1;
        v.a = x[i0];
        v.b = x[i1];
      } else {
        v = load_pair(x, t, T, vec);
      }
      if constexpr (MODE == PW_POW) {
        v.a = pow(v.a, wd);
        v.b = pow(v.b, wd);
      } else if constexpr (MODE == PW_CLIP) {
        if (a.flags & PW_FLAG_LOWER) {
          v.a = v.a < a.q ? a.v : v.a;
          v.b = v.b < a.q ? a.v : v.b;
        } else {
          v.a = v.a > a.q ? a.v : v.a;
          v.b = v.b > a.q ? a.v : v.b;
        }
      }
      store_pair(o, t, T, vec, v);
    }
  }
}

hipError_t launch_prep_pointwise(int mode, const PointwiseArgs &a, int64_t N, hipStream_t st) {
  if (N <= 0 || a.D <= 0 || a.T <= 0) return hipSuccess;
  const int64_t rows = mode <= PW_ROTATE ? N : N * a.D;
  const int64_t tiles = (a.T + kStreamTile - 1) / kStreamTile;
  if (rows > 0x7fffffffLL || tiles > 65535) return hipErrorInvalidValue;
  const dim3 grid((unsigned)rows, (unsigned)tiles), block(256);
  switch (mode) {
    case PW_MUL: hipLaunchKernelGGL(prep_pointwise_kernel<PW_MUL>, grid, block, 0, st, a); break;
    case PW_ADD: hipLaunchKernelGGL(prep_pointwise_kernel<PW_ADD>, grid, block, 0, st, a); break;
    case PW_ROTATE: hipLaunchKernelGGL(prep_pointwise_kernel<PW_ROTATE>, grid, block, 0, st, a); break;
    case PW_POW: hipLaunchKernelGGL(prep_pointwise_kernel<PW_POW>, grid, block, 0, st, a); break;
    case PW_SHIFT: hipLaunchKernelGGL(prep_pointwise_kernel<PW_SHIFT>, grid, block, 0, st, a); break;
    case PW_CLIP: hipLaunchKernelGGL(prep_pointwise_kernel<PW_CLIP>, grid, block, 0, st, a); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace fr
