// The two streaming kernels of lowered generic words (fruits/iss/words/letters.py, the slow path
// of fruits/iss/semiring.py:54-75; fruits_amd/iss/lowering.py): the virtual input rows a lowered
// exponent table refers to, and the unshift of the rows a max-plus / max-times plan produced
// over left-shifted inputs.  Both move fp64 values and take fabs, nothing else: bit-exact.
//
// Like kernels_filter.hip: one workgroup of 256 lanes per (row, tile of kTile time steps), a lane
// owns two consecutive time steps per pass and stores them with ONE 16-byte access where the
// output rows are 16-byte aligned (even T, aligned base).  The source pair starts at t + shift
// (rows) or t - shift (unshift), any parity: one 16-byte load where that is aligned too, 8-byte
// loads otherwise - the loads of neighbouring lanes still cover whole cache lines.  No LDS; a
// row's {kind, source, shift} is the same for the whole workgroup and is read through the
// constant address space (scalar loads).  All offsets are 64-bit.
#include <hip/hip_runtime.h>

#include "../../include/fruits_hip.h"   // FR_ROW_*
#include "kernels.h"
#include "walk_scan.h"

namespace fr {

constexpr int kTile = 1024;   // two passes of 256 lane pairs

__device__ __forceinline__ bool aligned16_rows(const void *p, int64_t T) {
  return (T & 1) == 0 && (reinterpret_cast<uintptr_t>(p) & 15u) == 0;
}

__device__ __forceinline__ void store2(double *__restrict__ row, int64_t t, int64_t T, bool vec,
                                       double a, double b) {
  if (vec) {
    vd2 v;
    v.x = a;
    v.y = b;
    *reinterpret_cast<vd2 *>(row + t) = v;
  } else {
    row[t] = a;
    if (t + 1 < T) row[t + 1] = b;
  }
}

// out[n, r, t] = f(src[n, source_r, t + shift_r]) where t + shift_r < T, else +0.0
__global__ __launch_bounds__(256) void letter_rows_kernel(const double *__restrict__ X, int64_t D,
                                                          int64_t T,
                                                          const double *__restrict__ ext, int64_t H,
                                                          const int32_t *__restrict__ spec,
                                                          int64_t Dv, double one,
                                                          double *__restrict__ out) {
  const int64_t r = blockIdx.x;
  const int64_t n = r / Dv, v = r - n * Dv;
  const int kind = as_const(spec)[3 * v];
  const int64_t source = as_const(spec)[3 * v + 1];
  const int64_t shift = as_const(spec)[3 * v + 2];
  double *__restrict__ o = out + r * T;
  const bool ovec = aligned16_rows(out, T);
  const int64_t t0 = (int64_t)blockIdx.y * kTile + 2 * (int)threadIdx.x;

  // the source row; none for ONE, nor for an entry the host check would have refused
  const double *__restrict__ x = nullptr;
  if (kind == FR_ROW_DIM || kind == FR_ROW_ABS) {
    if (source >= 0 && source < D) x = X + (n * D + source) * T;
  } else if (kind == FR_ROW_EXT) {
    if (ext != nullptr && source >= 0 && source < H) x = ext + (n * H + source) * T;
  }
  const bool is_one = kind == FR_ROW_ONE;
  const bool take_abs = kind == FR_ROW_ABS;
  // (an even shift keeps the pair's parity: the load is as aligned as the row)
  const bool xvec = x != nullptr && (shift & 1) == 0 &&
                    aligned16_rows(kind == FR_ROW_EXT ? ext : X, T);
#pragma unroll
  for (int e = 0; e < kTile / 512; ++e) {
    const int64_t t = t0 + e * 512;
    if (t >= T) continue;
    const int64_t s = t + shift;
    double a = 0.0, b = 0.0;
    if (is_one) {
      if (s < T) a = one;
      if (s + 1 < T) b = one;
    } else if (x != nullptr && shift >= 0) {
      if (xvec && s + 1 < T) {
        const vd2 p = *reinterpret_cast<const vd2 *>(x + s);
        a = p.x;
        b = p.y;
      } else {
        if (s < T) a = x[s];
        if (s + 1 < T) b = x[s + 1];
      }
      if (take_abs) {
        // (fabs of the padding is +0.0 too)
        a = fabs(a);
        b = fabs(b);
      }
    }
    store2(o, t, T, ovec, a, b);
  }
}

hipError_t launch_letter_rows(const double *X, int64_t N, int64_t D, int64_t T, const double *ext,
                              int64_t H, const int32_t *spec, int Dv, double one, double *out,
                              hipStream_t st) {
  if (N <= 0 || Dv <= 0 || T <= 0) return hipSuccess;
  const int64_t tiles = (T + kTile - 1) / kTile;
  if (N * Dv > 0x7fffffffLL || tiles > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(letter_rows_kernel, dim3((unsigned)(N * Dv), (unsigned)tiles), dim3(256), 0, st,
                     X, D, T, ext, H, spec, (int64_t)Dv, one, out);
  return hipGetLastError();
}

// out[k, n, t] = t >= s_k ? A[k, n, t - s_k] : +0.0
__global__ __launch_bounds__(256) void rows_unshift_kernel(const double *__restrict__ A, int64_t N,
                                                           int64_t T,
                                                           const int32_t *__restrict__ shift,
                                                           double *__restrict__ out) {
  const int64_t r = blockIdx.x;
  int64_t s = as_const(shift)[r / N];
  if (s < 0 || s > T) s = T;   // (beyond the row, or refused by the host check: all zeros)
  const double *__restrict__ x = A + r * T;
  double *__restrict__ o = out + r * T;
  const bool ovec = aligned16_rows(out, T);
  const bool xvec = (s & 1) == 0 && aligned16_rows(A, T);
  const int64_t t0 = (int64_t)blockIdx.y * kTile + 2 * (int)threadIdx.x;
#pragma unroll
  for (int e = 0; e < kTile / 512; ++e) {
    const int64_t t = t0 + e * 512;
    if (t >= T) continue;
    double a = 0.0, b = 0.0;
    if (xvec && t >= s) {
      // (t, s even and t + 1 < T with an even T: both elements are inside the row)
      const vd2 p = *reinterpret_cast<const vd2 *>(x + (t - s));
      a = p.x;
      b = p.y;
    } else {
      if (t >= s) a = x[t - s];
      if (t + 1 >= s && t + 1 < T) b = x[t + 1 - s];
    }
    store2(o, t, T, ovec, a, b);
  }
}

hipError_t launch_rows_unshift(const double *A, int64_t K, int64_t N, int64_t T,
                               const int32_t *shift, double *out, hipStream_t st) {
  if (K <= 0 || N <= 0 || T <= 0) return hipSuccess;
  const int64_t tiles = (T + kTile - 1) / kTile;
  if (K * N > 0x7fffffffLL || tiles > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(rows_unshift_kernel, dim3((unsigned)(K * N), (unsigned)tiles), dim3(256), 0, st,
                     A, N, T, shift, out);
  return hipGetLastError();
}

}  // namespace fr
