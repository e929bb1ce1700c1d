// The backward pass of the factorised CosWISS kernels (coswiss.h): the gradient of the cosine
// weighted iterated sums with respect to their input.
//
// THE ARITHMETIC.  One unit = (series n, word w of L letters, frequency f), exponent S.  With
// q_m[t] = sin^(S-m)[t] cos^m[t] (formed as build_q of coswiss.h forms it), b_m = C(S, m) and
// z_k[t] = prod_d x_d[t]^e_kd the forward pass of a unit is (coswiss_unit)
//     s_0 = z_0;   k >= 1:  u_k[t] = sum_m b_m q_m[t] A_{k-1,m}[t-1]  (0 at t = 0),  s_k = u_k z_k
//     A_{k,m} = cumsum(s_k q_m)
//     non-total:  Y = cumsum(s_{L-1});      total:  Y[t] = sum_m b_m q_m[t] A_{L-1,m}[t]
// and its adjoint, G the upstream gradient of the unit's row and a_k = dL/ds_k,
//     non-total:  a_{L-1}[t] = sum_{t' >= t} G[t']
//     total:      a_{L-1}[t] = sum_m b_m q_m[t] sum_{t' >= t} q_m[t'] G[t']
//     k = L-1 ... 1:   dz_k = a_k u_k,   du_k = a_k z_k
//                      a_{k-1}[t] = sum_m b_m q_m[t] sum_{t' > t} q_m[t'] du_k[t']
//     dz_0 = a_0
// The shift between two letters - A[t-1] forward - is the EXCLUSIVE suffix sum backward: the sum
// over t' > t is what lies in front of a step in the reversed scan, so no value crosses a chunk
// edge besides the carries.
//
// THE KERNELS.  grad_cos_unit_kernel<S>: one workgroup of 256 lanes per (unit, series), two
// sweeps over the time chunks of kGradChunk steps in the frame of kernels_grad.hip (grad_frame.h).
//   * Ascending, forward lane map: the forward recursion again; u_k, k = 1 ... L-1, goes to the
//     scratch U.  Per letter S+1 prefix scans behind ONE barrier (the shape of cos_scan_all).
//   * Descending, reversed lane map (a suffix sum over time is a prefix scan over lanes): per
//     chunk the letters from L-1 down to 0, per letter S+1 suffix scans with S+1 carries from the
//     right behind ONE barrier; dz_k goes to the scratch DZ.
// The carries of a sweep - one per (letter, m) - live in LDS, double-buffered by the chunk's
// parity: every lane forms the next carry, lane 0 leaves it in the other buffer, and a buffer is
// read again only behind a later barrier.  The wave totals are double-buffered by a toggle per
// barrier.  grad_cos_input_kernel: one thread per element of dX adds dz_k * d(z_k)/dx_d of the
// (unit, letter) pairs whose letter names the dimension, in the fixed order of the table.
// Every sum has one association, whatever the grid.  Plain loads and stores only; all offsets are
// 64-bit; every access is guarded by t < T; the tables are wave-uniform and read through the
// constant address space.  Steps past T hold exact zeros in every scan.
#include <hip/hip_runtime.h>

#include "grad_frame.h"
#include "kernels.h"
#include "walk_scan.h"

namespace fr {

// The letter prod_d x_d[t]^e_d of the factors [fb, fe) at time t, without factor `skip` (-1: the
// whole letter).
__device__ __forceinline__ double cos_letter_value(const CosGradArgs &a, const double *__restrict__ xn,
                                                   int fb, int fe, int64_t t, int skip) {
  double m = 1.0;
  for (int f = fb; f < fe; ++f) {
    if (f == skip) continue;
    const int64_t d = as_const(a.fac)[2 * f];
    const int e = as_const(a.fac)[2 * f + 1];
    const double p = ipow(xn[d * a.T + t], e < 0 ? -e : e);
    m = e < 0 ? m / p : m * p;
  }
  return m;
}

// q_m = sin^(S-m) cos^m at the lane's four steps, 1.0 times the sines first, then the cosines
// (build_q); steps past T: sin = cos = 0, so every q_m is 0 there.
template <int S>
__device__ __forceinline__ void cos_grad_q(const double *__restrict__ sn_row, const double *__restrict__ cs_row,
                                           int64_t t0, int64_t T, double (&q)[S + 1][4]) {
  double sn[4], cs[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    sn[j] = t0 + j < T ? sn_row[t0 + j] : 0.0;
    cs[j] = t0 + j < T ? cs_row[t0 + j] : 0.0;
  }
#pragma unroll
  for (int m = 0; m <= S; ++m)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double v = 1.0;
#pragma unroll
      for (int i = 0; i < S - m; ++i) v = v * sn[j];
#pragma unroll
      for (int i = 0; i < m; ++i) v = v * cs[j];
      q[m][j] = v;
    }
}

// b_m = C(S, m), exact (cos_binom of coswiss.h)
constexpr double cos_grad_binom(int s, int m) {
  double c = 1.0;
  for (int k = 0; k < m; ++k) c = c * (s - k) / (k + 1);
  return c;
}

// sum_m b_m (q_m x_m) per step, m ascending (the association of cos_combine)
template <int S>
__device__ __forceinline__ void cos_grad_combine(const double (&q)[S + 1][4], const double (&x)[S + 1][4],
                                                 double (&out)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) out[j] = 0.0;
#pragma unroll
  for (int m = 0; m <= S; ++m)
#pragma unroll
    for (int j = 0; j < 4; ++j) out[j] += cos_grad_binom(S, m) * (x[m][j] * q[m][j]);
}

template <int S>
__global__ __launch_bounds__(256) void grad_cos_unit_kernel(CosGradArgs a, int first) {
  constexpr int M = S + 1;
  __shared__ double wave_total[2][M][4];
  __shared__ double carry[2][kCosGradLetters + 1][M];
  const int64_t n = blockIdx.x;
  const int unit = as_const(a.units)[first + (int)blockIdx.y];
  const int64_t N = a.N, T = a.T;
  const int F = a.F;
  const int w = unit / F, f = unit - w * F;
  const int lb = as_const(a.letter_begin)[w], L = as_const(a.letter_begin)[w + 1] - lb;
  const bool total = a.total != 0;
  const double *__restrict__ xn = a.X + n * a.D * T;
  const double *__restrict__ gn = a.G + n * a.g_n;
  const double *__restrict__ sn_row = a.trig + (int64_t)f * 2 * T;
  const double *__restrict__ cs_row = sn_row + T;
  const int gb = as_const(a.g_begin)[unit], ge = as_const(a.g_begin)[unit + 1];
  // letter k of the unit: its rows of U (k >= 1) and of DZ
  const auto u_row = [&](int k) { return a.U + (((int64_t)(lb + k - w - 1) * F + f) * N + n) * T; };
  const auto dz_row = [&](int k) { return a.DZ + (((int64_t)(lb + k) * F + f) * N + n) * T; };
  const auto clear_carries = [&] {
    __syncthreads();   // (nobody still reads the carries of the sweep before)
    for (int i = threadIdx.x; i < 2 * (kCosGradLetters + 1) * M; i += 256) (&carry[0][0][0])[i] = 0.0;
    __syncthreads();
  };
  const int64_t chunks = grad_chunks(T);
  int buf = 0;

  // ---- ascending: u_k of the letters behind the first
  clear_carries();
  for (int64_t c = 0; c < chunks && L > 1; ++c) {
    const int64_t t0 = forward_t0(c);
    const int par = (int)(c & 1);
    double q[M][4], xa[M][4];
    cos_grad_q<S>(sn_row, cs_row, t0, T, q);
    for (int k = 0; k < L; ++k) {
      const int fb = as_const(a.fac_begin)[lb + k], fe = as_const(a.fac_begin)[lb + k + 1];
      double s[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) s[j] = t0 + j < T ? cos_letter_value(a, xn, fb, fe, t0 + j, -1) : 0.0;
      if (k > 0) {
        double u[4];
        cos_grad_combine<S>(q, xa, u);
        double *__restrict__ ur = u_row(k);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (t0 + j < T) ur[t0 + j] = u[j];
          s[j] = u[j] * s[j];
        }
      }
      if (k == L - 1) break;
      // A_{k,m} = cumsum(s q_m): the lane's own prefix sums, then the lanes from the left
      double l[M][4], excl[M];
#pragma unroll
      for (int m = 0; m < M; ++m) {
        l[m][0] = s[0] * q[m][0];
#pragma unroll
        for (int j = 1; j < 4; ++j) l[m][j] = l[m][j - 1] + s[j] * q[m][j];
        excl[m] = scan_publish(l[m][3], wave_total[buf][m]);
      }
      __syncthreads();   // (one barrier serves the S+1 scans)
#pragma unroll
      for (int m = 0; m < M; ++m) {
        double cr = carry[par][k][m];
        const double off = scan_offset(wave_total[buf][m], excl[m], cr);
        if (threadIdx.x == 0) carry[par ^ 1][k][m] = cr;
        // what the next letter reads: the sums up to the step before
        xa[m][0] = off;
#pragma unroll
        for (int j = 1; j < 4; ++j) xa[m][j] = off + l[m][j - 1];
      }
      buf ^= 1;
    }
  }

  // ---- descending: a_k and dz_k, the letters from the last to the first
  clear_carries();
  for (int64_t c = chunks - 1; c >= 0; --c) {
    const int64_t t0 = reversed_t0(c);
    const int par = (int)(c & 1);
    double q[M][4];
    if (total || L > 1) cos_grad_q<S>(sn_row, cs_row, t0, T, q);
    double g[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = gb; i < ge; ++i) {
      const double *__restrict__ gk = gn + (int64_t)as_const(a.g_row)[i] * a.g_k;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (t0 + j < T) g[j] += gk[(t0 + j) * a.g_t];
    }
    double ak[4];   // a_k at the lane's steps
    if (!total) {
      // a_{L-1} = suffix(G): carry slot 0 (letter 0 has no scan of its own below)
      lane_suffix(g);
      const double excl = scan_publish(g[0], wave_total[buf][0]);
      __syncthreads();
      double cr = carry[par][0][0];
      const double off = scan_offset(wave_total[buf][0], excl, cr);
      if (threadIdx.x == 0) carry[par ^ 1][0][0] = cr;
#pragma unroll
      for (int j = 0; j < 4; ++j) ak[j] = off + g[j];
      buf ^= 1;
    } else {
      // a_{L-1}[t] = sum_m b_m q_m[t] suffix(q_m G)[t]: carry slots [0][m]
      double l[M][4], excl[M];
#pragma unroll
      for (int m = 0; m < M; ++m) {
#pragma unroll
        for (int j = 0; j < 4; ++j) l[m][j] = q[m][j] * g[j];
        lane_suffix(l[m]);
        excl[m] = scan_publish(l[m][0], wave_total[buf][m]);
      }
      __syncthreads();
#pragma unroll
      for (int m = 0; m < M; ++m) {
        double cr = carry[par][0][m];
        const double off = scan_offset(wave_total[buf][m], excl[m], cr);
        if (threadIdx.x == 0) carry[par ^ 1][0][m] = cr;
#pragma unroll
        for (int j = 0; j < 4; ++j) l[m][j] = off + l[m][j];
      }
      cos_grad_combine<S>(q, l, ak);
      buf ^= 1;
    }
    for (int k = L - 1; k >= 0; --k) {
      double *__restrict__ dz = dz_row(k);
      if (k == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (t0 + j < T) dz[t0 + j] = ak[j];
        break;
      }
      const int fb = as_const(a.fac_begin)[lb + k], fe = as_const(a.fac_begin)[lb + k + 1];
      const double *__restrict__ ur = u_row(k);
      double du[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool in = t0 + j < T;
        if (in) dz[t0 + j] = ak[j] * ur[t0 + j];
        du[j] = in ? ak[j] * cos_letter_value(a, xn, fb, fe, t0 + j, -1) : 0.0;
      }
      // a_{k-1}[t] = sum_m b_m q_m[t] sum_{t' > t} q_m[t'] du_k[t']: carry slots [k][m]
      double l[M][4], excl[M];
#pragma unroll
      for (int m = 0; m < M; ++m) {
#pragma unroll
        for (int j = 0; j < 4; ++j) l[m][j] = q[m][j] * du[j];
        lane_suffix(l[m]);
        excl[m] = scan_publish(l[m][0], wave_total[buf][m]);
      }
      __syncthreads();   // (one barrier serves the S+1 scans)
#pragma unroll
      for (int m = 0; m < M; ++m) {
        double cr = carry[par][k][m];
        const double off = scan_offset(wave_total[buf][m], excl[m], cr);
        if (threadIdx.x == 0) carry[par ^ 1][k][m] = cr;
        // the sums over the steps BEHIND each step: what lies in front of it in the scan
#pragma unroll
        for (int j = 0; j < 3; ++j) l[m][j] = off + l[m][j + 1];
        l[m][3] = off;
      }
      cos_grad_combine<S>(q, l, ak);
      buf ^= 1;
    }
  }
}

template <int S>
static hipError_t launch_units(const CosGradArgs &a, int first, int count, hipStream_t st) {
  for (int done = 0; done < count; done += 65535) {
    const int part = count - done < 65535 ? count - done : 65535;
    hipLaunchKernelGGL(grad_cos_unit_kernel<S>, dim3((unsigned)a.N, (unsigned)part), dim3(256), 0, st, a,
                       first + done);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_grad_cos_units(const CosGradArgs &a, int exponent, int first, int count, hipStream_t st) {
  if (exponent < 1 || exponent > kCosMaxExponent) return hipErrorInvalidValue;
  if (a.N <= 0 || a.T <= 0 || count <= 0) return hipSuccess;
  if (a.N > 0x7fffffffLL) return hipErrorInvalidValue;
  switch (exponent) {
    case 1: return launch_units<1>(a, first, count, st);
    case 2: return launch_units<2>(a, first, count, st);
    case 3: return launch_units<3>(a, first, count, st);
    case 4: return launch_units<4>(a, first, count, st);
    case 5: return launch_units<5>(a, first, count, st);
    case 6: return launch_units<6>(a, first, count, st);
    case 7: return launch_units<7>(a, first, count, st);
    default: return launch_units<8>(a, first, count, st);
  }
}

// ------------------------------------------------------------------ the input kernel
constexpr int kCosGradTile = 1024;   // time steps of a workgroup (4 per lane, strided)

__global__ __launch_bounds__(256) void grad_cos_input_kernel(CosGradArgs a) {
  const int64_t row = blockIdx.x;   // (series, dimension)
  const int64_t N = a.N, D = a.D, T = a.T;
  const int64_t n = row / D, d = row - n * D;
  const double *__restrict__ xn = a.X + n * D * T;
  const int ib = as_const(a.dim_begin)[d], ie = as_const(a.dim_begin)[d + 1];
#pragma unroll
  for (int e = 0; e < kCosGradTile / 256; ++e) {
    const int64_t t = (int64_t)blockIdx.y * kCosGradTile + e * 256 + (int)threadIdx.x;
    if (t >= T) continue;
    const double x = xn[d * T + t];
    double acc = 0.0;
    for (int i = ib; i < ie; ++i) {
      const int r = as_const(a.dim_item)[2 * i];
      const int fi = as_const(a.dim_item)[2 * i + 1];
      const int letter = r / a.F;
      const double dz = a.DZ[((int64_t)r * N + n) * T + t];
      const double others = cos_letter_value(a, xn, as_const(a.fac_begin)[letter],
                                             as_const(a.fac_begin)[letter + 1], t, fi);
      acc += dz * (dpow(x, as_const(a.fac)[2 * fi + 1]) * others);
    }
    a.dX[row * T + t] = acc;
  }
}

hipError_t launch_grad_cos_input(const CosGradArgs &a, hipStream_t st) {
  if (a.N <= 0 || a.D <= 0 || a.T <= 0) return hipSuccess;
  const int64_t tiles = (a.T + kCosGradTile - 1) / kCosGradTile;
  if (a.N * a.D > 0x7fffffffLL || tiles > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(grad_cos_input_kernel, dim3((unsigned)(a.N * a.D), (unsigned)tiles), dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace fr
