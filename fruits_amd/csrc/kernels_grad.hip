// The backward pass of the Reals trie walk: the gradient of unweighted iterated sums with respect
// to their input.  The forward pass is, node by node of the prefix trie,
//     S_v = cumsum(m_v * shift(S_p)),   m_v[t] = prod_d x_d[t]^e_vd
// (fruits/iss/semiring.py:98-125); its adjoint walks the trie leaves-to-root with SUFFIX sums:
//     B_v[t] = G_v[t] + sum over children c of m_c[t+1] A_c[t+1]        (nothing at t = T-1)
//     A_v[t] = sum over s >= t of B_v[s]
//     dX_d[t] = sum over v of A_v[t] shift(S_p)[t] dm_v/dx_d[t]
//
// Two kernels.  grad_suffix_kernel: one workgroup of 256 lanes per (node, series), launched depth
// by depth, the deepest nodes first, so a node GATHERS the finished A of its children (no atomics).
// It walks the time axis in chunks of kGradChunk steps from the last chunk to the first with a
// carry from the right.  Lane i owns the four time steps [c0 + 1020 - 4 i, c0 + 1023 - 4 i] of a
// chunk: the lane-to-time map is REVERSED, so the suffix sum over time is an inclusive prefix scan
// over the lanes - wave_inclusive_scan of walk_scan.h as it is - with the four wave totals through
// LDS.  grad_input_kernel: one thread per element of dX, which adds the terms of the nodes whose
// letter holds its dimension in the fixed order of the table.  Every sum has one association,
// whatever the grid: the result is the same bits from run to run.
//
// Plain loads and stores only; all offsets are 64-bit; every access is guarded by t < T.  The
// tables are wave-uniform and read through the constant address space (scalar loads).
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

// The letter prod_d x_d[t]^e_d of the factors [fb, fe) at time t of the series whose rows start
// at `xn`, without factor `skip` (-1: the whole letter): |e_d| roundings per dimension at most.
__device__ __forceinline__ double letter_value(const GradArgs &a, const double *__restrict__ xn,
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

__global__ __launch_bounds__(256) void grad_suffix_kernel(GradArgs a, int first) {
  __shared__ double wave_total[2][4];
  const int64_t n = blockIdx.x;
  const int v = as_const(a.level_nodes)[first + (int)blockIdx.y];
  const int64_t N = a.N, T = a.T;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double *__restrict__ xn = a.X + n * a.D * T;
  const double *__restrict__ gn = a.G + n * a.g_n;
  double *__restrict__ av = a.A + ((int64_t)v * N + n) * T;
  const int gb = as_const(a.g_begin)[v], ge = as_const(a.g_begin)[v + 1];
  const int cb = as_const(a.child_begin)[v], ce = as_const(a.child_begin)[v + 1];

  double carry = 0.0;   // sum of B_v over the chunks to the right
  const int64_t chunks = (T + kGradChunk - 1) / kGradChunk;
  for (int64_t c = chunks - 1; c >= 0; --c) {
    const int64_t t0 = c * kGradChunk + (kGradChunk - 4) - 4 * (int64_t)threadIdx.x;
    double b[4] = {0.0, 0.0, 0.0, 0.0};
    for (int g = gb; g < ge; ++g) {
      const double *__restrict__ gk = gn + (int64_t)as_const(a.g_row)[g] * a.g_k;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (t0 + j < T) b[j] += gk[(t0 + j) * a.g_t];
    }
    for (int ci = cb; ci < ce; ++ci) {
      const int ch = as_const(a.child)[ci];
      const int fb = as_const(a.fac_begin)[ch], fe = as_const(a.fac_begin)[ch + 1];
      const double *__restrict__ ac = a.A + ((int64_t)ch * N + n) * T;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (t0 + j + 1 < T) b[j] += letter_value(a, xn, fb, fe, t0 + j + 1, -1) * ac[t0 + j + 1];
    }
    // the lane's own suffix sums (steps past T hold exact zeros), then the lanes from the right
    b[2] += b[3];
    b[1] += b[2];
    b[0] += b[1];
    const double incl = wave_inclusive_scan<0>(b[0]);
    const double excl = wave_shift_right1<0>(incl);
    if (lane == 63) wave_total[c & 1][wave] = incl;
    // (two buffers: a wave that runs ahead writes the other one, and nobody reaches the chunk
    // after that before every wave has passed this barrier)
    __syncthreads();
    double run = carry, off = carry;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      if (w == wave) off = run;
      run += wave_total[c & 1][w];
    }
    carry = run;
    off += excl;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (t0 + j < T) av[t0 + j] = off + b[j];
  }
}

hipError_t launch_grad_suffix(const GradArgs &a, int first, int count, hipStream_t st) {
  if (a.N <= 0 || a.T <= 0 || count <= 0) return hipSuccess;
  if (a.N > 0x7fffffffLL) return hipErrorInvalidValue;
  for (int done = 0; done < count; done += 65535) {
    const int part = count - done < 65535 ? count - done : 65535;
    hipLaunchKernelGGL(grad_suffix_kernel, dim3((unsigned)a.N, (unsigned)part), dim3(256), 0, st, a,
                       first + done);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

constexpr int kGradTile = 1024;   // time steps of a workgroup of grad_input_kernel (4 per lane, strided)

__global__ __launch_bounds__(256) void grad_input_kernel(GradArgs a) {
  const int64_t row = blockIdx.x;   // (series, dimension)
  const int64_t N = a.N, D = a.D, T = a.T;
  const int64_t n = row / D, d = row - n * D;
  const double *__restrict__ xn = a.X + n * D * T;
  const int ib = as_const(a.dim_begin)[d], ie = as_const(a.dim_begin)[d + 1];
#pragma unroll
  for (int e = 0; e < kGradTile / 256; ++e) {
    const int64_t t = (int64_t)blockIdx.y * kGradTile + e * 256 + (int)threadIdx.x;
    if (t >= T) continue;
    const double x = xn[d * T + t];
    double acc = 0.0;
    for (int i = ib; i < ie; ++i) {
      const int v = as_const(a.dim_item)[2 * i];
      const int f = as_const(a.dim_item)[2 * i + 1];
      const int ps = as_const(a.parent_srow)[v];
      // dm_v = A_v * shift(S_p); shift(S)[0] = 0
      double dm = a.A[((int64_t)v * N + n) * T + t];
      if (ps >= 0) dm *= t > 0 ? a.S[((int64_t)ps * N + n) * T + t - 1] : 0.0;
      // d/dx x^e = e x^(e-1), the power by multiplication (never m / x: a zero input is an
      // ordinary one); e < 0: e / x^(|e|+1)
      const int ex = as_const(a.fac)[2 * f + 1];
      const double dpow = ex > 0 ? (double)ex * ipow(x, ex - 1) : (double)ex * (1.0 / ipow(x, 1 - ex));
      const double others = letter_value(a, xn, as_const(a.fac_begin)[v], as_const(a.fac_begin)[v + 1], t, f);
      acc += dm * (dpow * others);
    }
    a.dX[row * T + t] = acc;
  }
}

hipError_t launch_grad_input(const GradArgs &a, hipStream_t st) {
  if (a.N <= 0 || a.D <= 0 || a.T <= 0) return hipSuccess;
  const int64_t tiles = (a.T + kGradTile - 1) / kGradTile;
  if (a.N * a.D > 0x7fffffffLL || tiles > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(grad_input_kernel, dim3((unsigned)(a.N * a.D), (unsigned)tiles), dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace fr
