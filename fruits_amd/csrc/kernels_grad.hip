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
//
// Below them, the same pair for the max semirings Arctic and Bayesian (grad_max_suffix_kernel,
// grad_max_input_kernel): the suffix sums become SEGMENTED sums between the heads of S_v.  And at
// the end the kernels of weighted Reals plans (grad_w_prefix_kernel, grad_w_suffix_kernel,
// grad_w_input_kernel): the exp factors join the products, and a prefix scan forms the sums the
// forward pass carries from letter to letter.
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

// ------------------------------------------------------------------ the max semirings
// Arctic (max, +) and Bayesian (max, x), fruits/iss/semiring.py:282-309 and :461-493: per node
//     z_v = m_v (x) S_p (no shift; m_v alone at depth 1),   S_v = running maximum of z_v
// with m_v[t] = sum_d e_vd x_d[t] (Arctic) or prod_d x_d[t]^e_vd (Bayesian).  A HEAD of v is a
// time s with s == 0 or S_v[s] > S_v[s-1] - strictly, the first of equal maxima wins - and opens
// the segment [s, next head): S_v[t] = z_v[s] for every t of it.  The adjoint, leaves to root:
//     B_v[t] = G_v[t] + sum over children c of w_c[t] A_c[t]      (w_c = 1 Arctic, m_c[t] Bayesian)
//     A_v[s] = sum of B_v over the segment of s at a head s, 0.0 elsewhere
//     Arctic: dX_d[s] = sum_v e_vd A_v[s];   Bayesian: dX_d[s] = sum_v A_v[s] S_p[s] dm_v/dx_d[s]
//
// grad_max_suffix_kernel has the launch shape, the chunks and the reversed lane-to-time map of
// grad_suffix_kernel; its scan is SEGMENTED.  Walking time downwards, what crosses from t + 1 to
// t is the open sum carry(t + 1) = head(t + 1) ? 0 : R[t + 1] with R[t] = B[t] + carry(t + 1),
// and A[t] = head(t) ? R[t] : 0.  A run of time steps [lo, hi] acts on the carry that enters it
// from the right as  c -> f ? o : o + c  with f = "a head in the run" and o = the sum of B from
// lo up to the run's first head (the whole run without one); a run `a` to the right of a run `b`
// compose as  (o_a, f_a) o (o_b, f_b) = (f_b ? o_b : o_a + o_b, f_a | f_b).  So a segment's sum is
// only ever formed from that segment's B - never as a difference of two suffix sums - and every
// partial sum joins disjoint runs of one segment.  The flags of the 64 lanes are one ballot: a
// lane decides each step of the wave scan with a bit test, only the sums travel by DPP.  Across
// waves and chunks the carry is the value c alone (a pair applied to it gives a value).

// One step of the wave scan: the open sum of the lanes to the right (0.0 where the lane has no
// source) joins unless the lanes this one covers so far hold a head.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double seg_step(double v, bool blocked) {
  const double src = dpp_fetch<CTRL, ROW_MASK, 0>(v);
  return blocked ? v : v + src;
}

// Inclusive segmented scan over the lanes, lane 0 first (the latest time steps): `o` the lane's
// open sum, `heads` the ballot of the lanes that hold a head.  The steps are those of
// wave_inclusive_scan; before each, a lane covers the lanes [lo, lane] named beside it.
__device__ __forceinline__ double wave_segmented_scan(double o, unsigned long long heads, int lane) {
  const unsigned long long le = heads & ((2ull << lane) - 1ull);   // heads of the lanes [0, lane]
  const int row = lane & 48;
  const auto from = [&](int back) { return lane - back > row ? lane - back : row; };
  o = seg_step<0x111, 0xf>(o, (le >> lane) != 0);      // row_shr:1   [lane, lane]
  o = seg_step<0x112, 0xf>(o, (le >> from(1)) != 0);   // row_shr:2   [lane - 1, lane] within the row
  o = seg_step<0x114, 0xf>(o, (le >> from(3)) != 0);   // row_shr:4   [lane - 3, lane]
  o = seg_step<0x118, 0xf>(o, (le >> from(7)) != 0);   // row_shr:8   [lane - 7, lane]
  o = seg_step<0x142, 0xa>(o, (le >> row) != 0);       // row_bcast:15 -> rows 1,3   [row, lane]
  o = seg_step<0x143, 0xc>(o, (le >> 32) != 0);        // row_bcast:31 -> rows 2,3   [32, lane]
  return o;
}

template <int SEMI>
__global__ __launch_bounds__(256) void grad_max_suffix_kernel(GradArgs a, int first) {
  __shared__ double wave_total[2][4];
  __shared__ int wave_head[2][4];
  const int64_t n = blockIdx.x;
  const int v = as_const(a.level_nodes)[first + (int)blockIdx.y];
  const int64_t N = a.N, T = a.T;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double *__restrict__ xn = a.X + n * a.D * T;
  const double *__restrict__ gn = a.G + n * a.g_n;
  const double *__restrict__ sv = a.S + ((int64_t)as_const(a.self_srow)[v] * N + n) * T;
  double *__restrict__ av = a.A + ((int64_t)v * N + n) * T;
  const int gb = as_const(a.g_begin)[v], ge = as_const(a.g_begin)[v + 1];
  const int cb = as_const(a.child_begin)[v], ce = as_const(a.child_begin)[v + 1];

  double carry = 0.0;   // the open sum that enters the chunk from the right
  const int64_t chunks = (T + kGradChunk - 1) / kGradChunk;
  for (int64_t c = chunks - 1; c >= 0; --c) {
    const int64_t t0 = c * kGradChunk + (kGradChunk - 4) - 4 * (int64_t)threadIdx.x;
    // the heads, read off the recomputed S_v alone (steps past T hold none)
    double s[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) s[j] = (t0 + j >= 1 && t0 + j - 1 < T) ? sv[t0 + j - 1] : 0.0;
    bool h[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) h[j] = t0 + j < T && (t0 + j == 0 || s[j + 1] > s[j]);
    double b[4] = {0.0, 0.0, 0.0, 0.0};
    for (int g = gb; g < ge; ++g) {
      const double *__restrict__ gk = gn + (int64_t)as_const(a.g_row)[g] * a.g_k;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (t0 + j < T) b[j] += gk[(t0 + j) * a.g_t];
    }
    for (int ci = cb; ci < ce; ++ci) {
      const int ch = as_const(a.child)[ci];
      const double *__restrict__ ac = a.A + ((int64_t)ch * N + n) * T;
      if constexpr (SEMI == kSemiArctic) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (t0 + j < T) b[j] += ac[t0 + j];
      } else {
        const int fb = as_const(a.fac_begin)[ch], fe = as_const(a.fac_begin)[ch + 1];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (t0 + j < T) b[j] += letter_value(a, xn, fb, fe, t0 + j, -1) * ac[t0 + j];
      }
    }
    // the lane's own run, from its last step to its first
    double o = 0.0;
    bool f = false;
#pragma unroll
    for (int j = 3; j >= 0; --j) {
      o = h[j] ? 0.0 : b[j] + o;
      f = f || h[j];
    }
    const unsigned long long heads = __ballot(f);
    const double incl = wave_segmented_scan(o, heads, lane);
    const double excl = wave_shift_right1<0>(incl);
    if (lane == 63) {
      wave_total[c & 1][wave] = incl;
      wave_head[c & 1][wave] = heads != 0;
    }
    // (two buffers, as in grad_suffix_kernel)
    __syncthreads();
    double run = carry, off = carry;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      if (w == wave) off = run;
      run = wave_head[c & 1][w] ? wave_total[c & 1][w] : wave_total[c & 1][w] + run;
    }
    carry = run;
    // what enters this lane from the right, then its four steps
    double in = (heads & ((1ull << lane) - 1ull)) != 0 ? excl : excl + off;
#pragma unroll
    for (int j = 3; j >= 0; --j) {
      const double r = b[j] + in;
      if (t0 + j < T) av[t0 + j] = h[j] ? r : 0.0;
      in = h[j] ? 0.0 : r;
    }
  }
}

hipError_t launch_grad_max_suffix(const GradArgs &a, int semiring, int first, int count, hipStream_t st) {
  if (semiring != kSemiArctic && semiring != kSemiBayesian) return hipErrorInvalidValue;
  if (a.N <= 0 || a.T <= 0 || count <= 0) return hipSuccess;
  if (a.N > 0x7fffffffLL) return hipErrorInvalidValue;
  for (int done = 0; done < count; done += 65535) {
    const int part = count - done < 65535 ? count - done : 65535;
    const dim3 grid((unsigned)a.N, (unsigned)part);
    if (semiring == kSemiArctic)
      hipLaunchKernelGGL(grad_max_suffix_kernel<kSemiArctic>, grid, dim3(256), 0, st, a, first + done);
    else
      hipLaunchKernelGGL(grad_max_suffix_kernel<kSemiBayesian>, grid, dim3(256), 0, st, a, first + done);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

template <int SEMI>
__global__ __launch_bounds__(256) void grad_max_input_kernel(GradArgs a) {
  const int64_t row = blockIdx.x;   // (series, dimension)
  const int64_t N = a.N, D = a.D, T = a.T;
  const int64_t n = row / D, d = row - n * D;
  const double *__restrict__ xn = a.X + n * D * T;
  const int ib = as_const(a.dim_begin)[d], ie = as_const(a.dim_begin)[d + 1];
#pragma unroll
  for (int e = 0; e < kGradTile / 256; ++e) {
    const int64_t t = (int64_t)blockIdx.y * kGradTile + e * 256 + (int)threadIdx.x;
    if (t >= T) continue;
    double acc = 0.0;
    if constexpr (SEMI == kSemiArctic) {
      // the letter is linear: its coefficient times A_v
      for (int i = ib; i < ie; ++i) {
        const int v = as_const(a.dim_item)[2 * i];
        const int f = as_const(a.dim_item)[2 * i + 1];
        acc += (double)as_const(a.fac)[2 * f + 1] * a.A[((int64_t)v * N + n) * T + t];
      }
    } else {
      const double x = xn[d * T + t];
      for (int i = ib; i < ie; ++i) {
        const int v = as_const(a.dim_item)[2 * i];
        const int f = as_const(a.dim_item)[2 * i + 1];
        const int ps = as_const(a.parent_srow)[v];
        // dm_v = A_v * S_p at the SAME step (no shift between the letters of a max semiring)
        double dm = a.A[((int64_t)v * N + n) * T + t];
        if (ps >= 0) dm *= a.S[((int64_t)ps * N + n) * T + t];
        const int ex = as_const(a.fac)[2 * f + 1];
        const double dpow = ex > 0 ? (double)ex * ipow(x, ex - 1) : (double)ex * (1.0 / ipow(x, 1 - ex));
        const double others = letter_value(a, xn, as_const(a.fac_begin)[v], as_const(a.fac_begin)[v + 1], t, f);
        acc += dm * (dpow * others);
      }
    }
    a.dX[row * T + t] = acc;
  }
}

hipError_t launch_grad_max_input(const GradArgs &a, int semiring, hipStream_t st) {
  if (semiring != kSemiArctic && semiring != kSemiBayesian) return hipErrorInvalidValue;
  if (a.N <= 0 || a.D <= 0 || a.T <= 0) return hipSuccess;
  const int64_t tiles = (a.T + kGradTile - 1) / kGradTile;
  if (a.N * a.D > 0x7fffffffLL || tiles > 65535) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(a.N * a.D), (unsigned)tiles);
  if (semiring == kSemiArctic)
    hipLaunchKernelGGL(grad_max_input_kernel<kSemiArctic>, grid, dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL(grad_max_input_kernel<kSemiBayesian>, grid, dim3(256), 0, st, a);
  return hipGetLastError();
}

// ------------------------------------------------------------------ weighted Reals plans
// Both weighted bodies of fruits/iss/semiring.py:98-158 carry the same sums from letter to letter
// (E+_v = exp(g alpha_v), E-_v = exp(-g alpha_v) of the node's last letter):
//     y_v[t] = m_v[t] E-_p[t] E+_v[t] C_p[t-1]   (depth 1: m_v[t] E+_v[t]),   C_v = cumsum(y_v)
// and differ in what a node emits: S_v = C_v E-_v (total) or S_v = cumsum(z_v), y_v = z_v E+_v
// (non-total).  The adjoint, leaves to root, children c reading C_v[s] at time s + 1:
//     total:      B_v[s] = G_v[s] E-_v[s] + sum_c m_c[s+1] E-_v[s+1] E+_c[s+1] A_c[s+1]
//                 A_v = suffix(B_v);                          dm_v = A_v E-_p E+_v shift(C_p)
//     non-total:  Q_v[s] = sum_c m_c[s+1] E-_v[s+1] A_c[s+1]
//                 A_v = suffix(G_v) + E+_v suffix(Q_v);       dm_v = A_v E-_p shift(C_p)
// Nothing is divided by an exp factor.  The forward walk of a non-total plan emits S, not C, so
// grad_w_prefix_kernel forms C of the nodes that have children; the exp tables are read from
// global memory (launch_exp_tables filled them on the same stream).

// Table `tb` (-1: none, the factor 1.0) of the series whose tables start at `aux_n` at time t.
__device__ __forceinline__ double exp_factor(const double *__restrict__ aux_n, int64_t aux_tab, int tb,
                                             int64_t t) {
  return tb < 0 ? 1.0 : aux_n[(int64_t)tb * aux_tab + t];
}

// (one kernel for both bodies: they carry the same sums)
__global__ __launch_bounds__(256) void grad_w_prefix_kernel(GradWArgs w, int first) {
  __shared__ double wave_total[2][4];
  const GradArgs &a = w.g;
  const int64_t n = blockIdx.x;
  const int v = as_const(w.inner_nodes)[first + (int)blockIdx.y];
  const int64_t N = a.N, T = a.T;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double *__restrict__ xn = a.X + n * a.D * T;
  const double *__restrict__ en = w.aux + n * w.aux_n;
  const int fb = as_const(a.fac_begin)[v], fe = as_const(a.fac_begin)[v + 1];
  const int ps = as_const(a.parent_srow)[v];
  const int t_plus = as_const(w.tab)[3 * v], t_pminus = as_const(w.tab)[3 * v + 2];
  const double *__restrict__ cp = ps >= 0 ? w.C + ((int64_t)ps * N + n) * T : nullptr;
  double *__restrict__ cv = w.C + ((int64_t)as_const(a.self_srow)[v] * N + n) * T;

  double carry = 0.0;   // sum of y_v over the chunks to the left
  const int64_t chunks = (T + kGradChunk - 1) / kGradChunk;
  for (int64_t c = 0; c < chunks; ++c) {
    const int64_t t0 = c * kGradChunk + 4 * (int64_t)threadIdx.x;
    double y[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t t = t0 + j;
      if (t >= T) continue;
      double val = letter_value(a, xn, fb, fe, t, -1);
      if (ps >= 0) val = t > 0 ? val * cp[t - 1] * exp_factor(en, w.aux_tab, t_pminus, t) : 0.0;
      y[j] = val * exp_factor(en, w.aux_tab, t_plus, t);
    }
    // the lane's own prefix sums (steps past T hold exact zeros), then the lanes from the left
    y[1] += y[0];
    y[2] += y[1];
    y[3] += y[2];
    const double incl = wave_inclusive_scan<0>(y[3]);
    const double excl = wave_shift_right1<0>(incl);
    if (lane == 63) wave_total[c & 1][wave] = incl;
    // (two buffers, as in grad_suffix_kernel)
    __syncthreads();
    double run = carry, off = carry;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k == wave) off = run;
      run += wave_total[c & 1][k];
    }
    carry = run;
    off += excl;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (t0 + j < T) cv[t0 + j] = off + y[j];
  }
}

hipError_t launch_grad_w_prefix(const GradWArgs &w, int first, int count, hipStream_t st) {
  if (w.g.N <= 0 || w.g.T <= 0 || count <= 0) return hipSuccess;
  if (w.g.N > 0x7fffffffLL) return hipErrorInvalidValue;
  for (int done = 0; done < count; done += 65535) {
    const int part = count - done < 65535 ? count - done : 65535;
    hipLaunchKernelGGL(grad_w_prefix_kernel, dim3((unsigned)w.g.N, (unsigned)part), dim3(256), 0, st, w,
                       first + done);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// The launch shape, the chunks and the reversed lane-to-time map of grad_suffix_kernel.  Total: one
// scan over B_v.  Non-total: the suffix sums of G_v and of Q_v are two scans with two carries,
// joined as suffix(G) + E+ suffix(Q); a scan whose operand is empty - a node that is no output
// row, a node without children - is skipped (block-uniform branches).
template <bool TOTAL>
__global__ __launch_bounds__(256) void grad_w_suffix_kernel(GradWArgs w, int first) {
  __shared__ double wave_total[2][2][4];
  const GradArgs &a = w.g;
  const int64_t n = blockIdx.x;
  const int v = as_const(a.level_nodes)[first + (int)blockIdx.y];
  const int64_t N = a.N, T = a.T;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double *__restrict__ xn = a.X + n * a.D * T;
  const double *__restrict__ gn = a.G + n * a.g_n;
  const double *__restrict__ en = w.aux + n * w.aux_n;
  double *__restrict__ av = a.A + ((int64_t)v * N + n) * T;
  const int gb = as_const(a.g_begin)[v], ge = as_const(a.g_begin)[v + 1];
  const int cb = as_const(a.child_begin)[v], ce = as_const(a.child_begin)[v + 1];
  const int t_plus = as_const(w.tab)[3 * v], t_minus = as_const(w.tab)[3 * v + 1];
  const bool has_g = ge > gb, has_c = ce > cb;
  // which sums are scanned: total - B alone (slot 0); non-total - G (slot 0) and Q (slot 1)
  const bool scan0 = TOTAL ? (has_g || has_c) : has_g;
  const bool scan1 = !TOTAL && has_c;

  double carry0 = 0.0, carry1 = 0.0;   // the sums over the chunks to the right
  const int64_t chunks = (T + kGradChunk - 1) / kGradChunk;
  for (int64_t c = chunks - 1; c >= 0; --c) {
    const int64_t t0 = c * kGradChunk + (kGradChunk - 4) - 4 * (int64_t)threadIdx.x;
    double b[4] = {0.0, 0.0, 0.0, 0.0};   // total: B_v; non-total: G_v
    double q[4] = {0.0, 0.0, 0.0, 0.0};   // non-total: Q_v
    for (int g = gb; g < ge; ++g) {
      const double *__restrict__ gk = gn + (int64_t)as_const(a.g_row)[g] * a.g_k;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (t0 + j < T) b[j] += gk[(t0 + j) * a.g_t];
    }
    if (TOTAL && has_g) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (t0 + j < T) b[j] *= exp_factor(en, w.aux_tab, t_minus, t0 + j);
    }
    for (int ci = cb; ci < ce; ++ci) {
      const int ch = as_const(a.child)[ci];
      const int fb = as_const(a.fac_begin)[ch], fe = as_const(a.fac_begin)[ch + 1];
      const int c_plus = as_const(w.tab)[3 * ch];
      const double *__restrict__ ac = a.A + ((int64_t)ch * N + n) * T;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t s = t0 + j + 1;
        if (s >= T) continue;
        double term = letter_value(a, xn, fb, fe, s, -1) * exp_factor(en, w.aux_tab, t_minus, s);
        if constexpr (TOTAL) {
          term *= exp_factor(en, w.aux_tab, c_plus, s);
          b[j] += term * ac[s];
        } else {
          q[j] += term * ac[s];
        }
      }
    }
    // the lane's own suffix sums (steps past T hold exact zeros), then the lanes from the right
    double excl0 = 0.0, excl1 = 0.0;
    if (scan0) {
      b[2] += b[3];
      b[1] += b[2];
      b[0] += b[1];
      const double incl = wave_inclusive_scan<0>(b[0]);
      excl0 = wave_shift_right1<0>(incl);
      if (lane == 63) wave_total[c & 1][0][wave] = incl;
    }
    if (scan1) {
      q[2] += q[3];
      q[1] += q[2];
      q[0] += q[1];
      const double incl = wave_inclusive_scan<0>(q[0]);
      excl1 = wave_shift_right1<0>(incl);
      if (lane == 63) wave_total[c & 1][1][wave] = incl;
    }
    // (two buffers, as in grad_suffix_kernel; one barrier serves both scans)
    __syncthreads();
    double off0 = 0.0, off1 = 0.0;
    if (scan0) {
      double run = carry0;
      off0 = carry0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k == wave) off0 = run;
        run += wave_total[c & 1][0][k];
      }
      carry0 = run;
      off0 += excl0;
    }
    if (scan1) {
      double run = carry1;
      off1 = carry1;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k == wave) off1 = run;
        run += wave_total[c & 1][1][k];
      }
      carry1 = run;
      off1 += excl1;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (t0 + j >= T) continue;
      double out = scan0 ? off0 + b[j] : 0.0;
      if (scan1) {
        const double sq = (off1 + q[j]) * exp_factor(en, w.aux_tab, t_plus, t0 + j);
        out = scan0 ? out + sq : sq;
      }
      av[t0 + j] = out;
    }
  }
}

hipError_t launch_grad_w_suffix(const GradWArgs &w, bool total, int first, int count, hipStream_t st) {
  if (w.g.N <= 0 || w.g.T <= 0 || count <= 0) return hipSuccess;
  if (w.g.N > 0x7fffffffLL) return hipErrorInvalidValue;
  for (int done = 0; done < count; done += 65535) {
    const int part = count - done < 65535 ? count - done : 65535;
    const dim3 grid((unsigned)w.g.N, (unsigned)part);
    if (total)
      hipLaunchKernelGGL(grad_w_suffix_kernel<true>, grid, dim3(256), 0, st, w, first + done);
    else
      hipLaunchKernelGGL(grad_w_suffix_kernel<false>, grid, dim3(256), 0, st, w, first + done);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

template <bool TOTAL>
__global__ __launch_bounds__(256) void grad_w_input_kernel(GradWArgs w) {
  const GradArgs &a = w.g;
  const int64_t row = blockIdx.x;   // (series, dimension)
  const int64_t N = a.N, D = a.D, T = a.T;
  const int64_t n = row / D, d = row - n * D;
  const double *__restrict__ xn = a.X + n * D * T;
  const double *__restrict__ en = w.aux + n * w.aux_n;
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
      // total: dm_v = A_v E-_p E+_v shift(C_p); non-total: dm_v = A_v E-_p shift(C_p); shift(C)[0] = 0
      double dm = a.A[((int64_t)v * N + n) * T + t];
      if (ps >= 0)
        dm = t > 0 ? dm * exp_factor(en, w.aux_tab, as_const(w.tab)[3 * v + 2], t) *
                         w.C[((int64_t)ps * N + n) * T + t - 1]
                   : 0.0;
      if constexpr (TOTAL) dm *= exp_factor(en, w.aux_tab, as_const(w.tab)[3 * v], t);
      const int ex = as_const(a.fac)[2 * f + 1];
      const double dpow = ex > 0 ? (double)ex * ipow(x, ex - 1) : (double)ex * (1.0 / ipow(x, 1 - ex));
      const double others = letter_value(a, xn, as_const(a.fac_begin)[v], as_const(a.fac_begin)[v + 1], t, f);
      acc += dm * (dpow * others);
    }
    a.dX[row * T + t] = acc;
  }
}

hipError_t launch_grad_w_input(const GradWArgs &w, bool total, hipStream_t st) {
  const GradArgs &a = w.g;
  if (a.N <= 0 || a.D <= 0 || a.T <= 0) return hipSuccess;
  const int64_t tiles = (a.T + kGradTile - 1) / kGradTile;
  if (a.N * a.D > 0x7fffffffLL || tiles > 65535) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(a.N * a.D), (unsigned)tiles);
  if (total)
    hipLaunchKernelGGL(grad_w_input_kernel<true>, grid, dim3(256), 0, st, w);
  else
    hipLaunchKernelGGL(grad_w_input_kernel<false>, grid, dim3(256), 0, st, w);
  return hipGetLastError();
}

}  // namespace fr
