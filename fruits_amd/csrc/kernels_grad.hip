// The backward pass of the trie walk: the gradient of iterated sums with respect to their input
// (DESIGN.md 4.14), for five adjoints - GradKind of kernels.h: unweighted Reals, weighted Reals
// total and non-total, Arctic, Bayesian.
//
// THE SHARED FRAME.  Every adjoint walks the prefix trie leaves-to-root: per node v a row B_v of
// what reaches it - the rows of the upstream gradient G it emitted plus a term of each child's
// finished A_c - and A_v = a scan of B_v over time; then per element of dX a sum over the nodes
// whose letter holds its dimension.
//   * Scan kernels: one workgroup of 256 lanes per (node, series), launched depth by depth
//     (launch_per_depth), the deepest nodes first, so a node GATHERS the finished A of its children
//     (no atomics).  A workgroup walks the time axis in chunks of kGradChunk steps with a carry
//     from chunk to chunk; a lane owns four adjacent steps of a chunk.  For the suffix kernels the
//     chunks run from the last to the first and the lane-to-time map is REVERSED (reversed_t0:
//     lane i owns [c0 + 1020 - 4 i, c0 + 1023 - 4 i]), so the suffix sum over time is an inclusive
//     prefix scan over the lanes - wave_inclusive_scan of walk_scan.h as it is.  The block scan has
//     two phases around the caller's ONE barrier: scan_publish (the wave scan; lane 63 leaves the
//     wave's total in an LDS slot) and scan_offset (the four wave totals join the carry in wave
//     order).  The slots are double-buffered by the chunk's parity: a wave that runs ahead writes
//     the other buffer, and nobody reaches the chunk after that before every wave has passed this
//     chunk's barrier.
//   * gather_upstream adds the node's rows of G - or gather_picked the pairs (position, weight) of
//     a sparse upstream, a compile-time switch of the scan kernels -; the
//     children's terms are the adjoint's own.
//   * grad_input_kernel: one thread per element of dX, which adds the terms dm_v * d(letter)/dx of
//     the nodes in the fixed order of the table (dim_item); the adjoints differ in dm_v alone.
// Every sum has one association, whatever the grid: the result is the same bits from run to run.
// Plain loads and stores only; all offsets are 64-bit; every access is guarded by t < T.  The
// tables are wave-uniform and read through the constant address space (scalar loads).
//
// PER-SERIES LENGTHS (a.len).  T stays the row stride; the extent of series n is
// T_n = len[n] (series_extent: workgroup-uniform, one scalar load; T without lengths).  The adjoint
// is anti-causal - A_v[t] sums over s >= t - so the scans START at the series' own last chunk,
// grad_chunks(T_n) - 1, and every guard on a time step is t < T_n: the chunks are aligned at t = 0
// and the steps past the extent hold exact zeros, so the lane sums, wave totals and carries - and
// the bits - are those of the call on the truncated series.  Nothing of A, S, C or G is read at
// t >= T_n (A and C are never written there), and grad_input_kernel stores +0.0 there.  The guards
// select; nothing is masked by a multiplication.
//
// WHAT EACH ADJOINT ADDS.
// Reals, unweighted (fruits/iss/semiring.py:98-125): S_v = cumsum(m_v * shift(S_p)),
// m_v[t] = prod_d x_d[t]^e_vd.
//     B_v[t] = G_v[t] + sum over children c of m_c[t+1] A_c[t+1]        (nothing at t = T-1)
//     A_v[t] = sum over s >= t of B_v[s];      dm_v = A_v shift(S_p)
// S is the caller's: one more forward walk of the prefix plan.
//
// Reals, weighted (semiring.py:98-158; E+_v = exp(g alpha_v), E-_v =
// exp(-g alpha_v) of the node's last letter).  Both bodies carry the same sums from letter to
// letter,
//     y_v[t] = m_v[t] E-_p[t] E+_v[t] C_p[t-1]   (depth 1: m_v[t] E+_v[t]),   C_v = cumsum(y_v)
// and differ in what a node emits: S_v = C_v E-_v (total) or S_v = cumsum(z_v), y_v = z_v E+_v
// (non-total).  The adjoint, children c reading C_v[s] at time s + 1:
//     total:      B_v[s] = G_v[s] E-_v[s] + sum_c m_c[s+1] E-_v[s+1] E+_c[s+1] A_c[s+1]
//                 A_v = suffix(B_v);                          dm_v = A_v E-_p E+_v shift(C_p)
//     non-total:  Q_v[s] = sum_c m_c[s+1] E-_v[s+1] A_c[s+1]
//                 A_v = suffix(G_v) + E+_v suffix(Q_v);       dm_v = A_v E-_p shift(C_p)
// Nothing is divided by an exp factor.  Non-total is two scans with two carries behind the one
// barrier; a scan whose operand is empty - a node that is no output row, a node without children -
// is skipped (block-uniform branches).  The forward walk of a non-total plan emits S, not C, so
// grad_prefix_kernel forms C of the nodes that have children, root first, with the forward lane
// map; the exp tables are read from global memory (launch_exp_tables filled them on the stream).
//
// A lookup that is a function of the input (L1 / L2): a plan armed with
// fr_plan_set_grad_pathlen makes the prefix kernel form C of the output rows without children too
// (total) and the suffix kernel keep R_v = suffix(Q_v) (non-total); grad_lookup_kernel then
// gathers dL/dg over the nodes and grad_pathlen_kernel carries it through the normalised
// cumulative path length into dimension 0 of dX, behind the input kernel.
//
// Arctic (max, +) and Bayesian (max, x), semiring.py:282-309 and :461-493: per node
//     z_v = m_v (x) S_p (no shift; m_v alone at depth 1),   S_v = running maximum of z_v
// with m_v[t] = sum_d e_vd x_d[t] (Arctic) or prod_d x_d[t]^e_vd (Bayesian).  A HEAD of v is a
// time s with s == 0 or S_v[s] > S_v[s-1] - strictly, the first of equal maxima wins - and opens
// the segment [s, next head): S_v[t] = z_v[s] for every t of it.
//     B_v[t] = G_v[t] + sum over children c of w_c[t] A_c[t]      (w_c = 1 Arctic, m_c[t] Bayesian)
//     A_v[s] = sum of B_v over the segment of s at a head s, 0.0 elsewhere
//     Arctic: dX_d[s] = sum_v e_vd A_v[s];   Bayesian: dm_v = A_v S_p at the same step
// grad_max_suffix_kernel stands in the frame of grad_suffix_kernel - chunks, reversed map, slot
// parity, one barrier -; its scan is SEGMENTED and keeps its own operator.  Walking time
// downwards, what crosses from t + 1 to t is the open sum carry(t + 1) = head(t + 1) ? 0 : R[t + 1]
// with R[t] = B[t] + carry(t + 1), and A[t] = head(t) ? R[t] : 0.  A run of time steps [lo, hi]
// acts on the carry that enters it from the right as  c -> f ? o : o + c  with f = "a head in the
// run" and o = the sum of B from lo up to the run's first head (the whole run without one); a run
// `a` to the right of a run `b` compose as  (o_a, f_a) o (o_b, f_b) = (f_b ? o_b : o_a + o_b,
// f_a | f_b).  So a segment's sum is only ever formed from that segment's B - never as a
// difference of two suffix sums - and every partial sum joins disjoint runs of one segment.  The
// flags of the 64 lanes are one ballot: a lane decides each step of the wave scan with a bit test,
// only the sums travel by DPP.  Across waves and chunks the carry is the value c alone (a pair
// applied to it gives a value).
#include <hip/hip_runtime.h>

#include "grad_frame.h"
#include "kernels.h"
#include "walk_scan.h"

namespace fr {

constexpr bool grad_weighted(int kind) { return kind == kGradTotal || kind == kGradNonTotal; }

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

// Table `tb` (-1: none, the factor 1.0) of the series whose tables start at `aux_n` at time t.
__device__ __forceinline__ double exp_factor(const double *__restrict__ aux_n, int64_t aux_tab, int tb,
                                             int64_t t) {
  return tb < 0 ? 1.0 : aux_n[(int64_t)tb * aux_tab + t];
}

// ------------------------------------------------------------------ the shared frame
// (the powers, the chunks, the lane maps and the block scan: grad_frame.h)
// The extent of series n.
__device__ __forceinline__ int64_t series_extent(const GradArgs &a, int64_t n) {
  return a.len ? (int64_t)as_const(a.len)[n] : a.T;
}

// b[j] += the rows [gb, ge) of the upstream gradient of the series at `gn`, at the steps t0 + j
// below the series' extent Tn.
__device__ __forceinline__ void gather_upstream(const GradArgs &a, const double *__restrict__ gn, int gb,
                                                int ge, int64_t t0, int64_t Tn, double (&b)[4]) {
  for (int g = gb; g < ge; ++g) {
    const double *__restrict__ gk = gn + (int64_t)as_const(a.g_row)[g] * a.g_k;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (t0 + j < Tn) b[j] += gk[(t0 + j) * a.g_t];
  }
}

// The same from the SPARSE upstream of picked features: a row of the series
// `n` is a.F pairs (position, weight), and a pair adds its weight to b[j] where its position is
// the step t0 + j.  The order is fixed - the rows in g_row order, a row's pairs in column order,
// each added in turn - and so are the bits.  A position < 0 (an empty band) matches no step.
// n and the node are workgroup-uniform: the pairs are scalar loads, every lane sees every pair.
__device__ __forceinline__ void gather_picked(const GradArgs &a, int64_t n, int gb, int ge, int64_t t0,
                                              int64_t Tn, double (&b)[4]) {
  for (int g = gb; g < ge; ++g) {
    const int64_t at = n * a.g_n + (int64_t)as_const(a.g_row)[g] * a.g_k;
    for (int f = 0; f < a.F; ++f) {
      const int64_t p = as_const(a.pos)[at + f];
      const double w = as_const(a.w)[at + f];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (p == t0 + j && t0 + j < Tn) b[j] += w;
    }
  }
}

// `count` workgroups per series, blockIdx.y < 65535 each launch: nodes [first, first + count) of
// a per-depth table.
template <typename Args>
hipError_t launch_per_depth(void (*kernel)(Args, int), const Args &a, int first, int count, hipStream_t st) {
  if (a.N <= 0 || a.T <= 0 || count <= 0) return hipSuccess;
  if (a.N > 0x7fffffffLL) return hipErrorInvalidValue;
  for (int done = 0; done < count; done += 65535) {
    const int part = count - done < 65535 ? count - done : 65535;
    hipLaunchKernelGGL(kernel, dim3((unsigned)a.N, (unsigned)part), dim3(256), 0, st, a, first + done);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// ------------------------------------------------------------------ the additive suffix scans
// KIND: kGradReals, kGradTotal or kGradNonTotal.  Slot 0 scans B_v (non-total: G_v), slot 1 - of
// the non-total body alone - Q_v; the unweighted kernel has no exp factor and always scans.
// SPARSE: the upstream is the pairs of picked features (gather_picked), not G.
template <int KIND, bool SPARSE>
__global__ __launch_bounds__(256) void grad_suffix_kernel(GradArgs a, int first) {
  constexpr bool WEIGHTED = grad_weighted(KIND), TOTAL = KIND == kGradTotal;
  __shared__ double wave_total[2][KIND == kGradNonTotal ? 2 : 1][4];
  const int64_t n = blockIdx.x;
  const int v = as_const(a.level_nodes)[first + (int)blockIdx.y];
  const int64_t N = a.N, T = a.T, Tn = series_extent(a, n);
  const double *__restrict__ xn = a.X + n * a.D * T;
  const double *__restrict__ gn = SPARSE ? nullptr : a.G + n * a.g_n;
  const double *__restrict__ en = WEIGHTED ? a.aux + n * a.aux_n : nullptr;
  double *__restrict__ av = a.A + ((int64_t)v * N + n) * T;
  const int gb = as_const(a.g_begin)[v], ge = as_const(a.g_begin)[v + 1];
  const int cb = as_const(a.child_begin)[v], ce = as_const(a.child_begin)[v + 1];
  int t_plus = -1, t_minus = -1;
  if constexpr (WEIGHTED) {
    t_plus = as_const(a.tab)[3 * v];
    t_minus = as_const(a.tab)[3 * v + 1];
  }
  const bool has_g = ge > gb, has_c = ce > cb;
  const bool scan0 = !WEIGHTED || (TOTAL ? (has_g || has_c) : has_g);
  const bool scan1 = KIND == kGradNonTotal && has_c;

  double carry0 = 0.0, carry1 = 0.0;   // the sums over the chunks to the right
  for (int64_t c = grad_chunks(Tn) - 1; c >= 0; --c) {
    const int64_t t0 = reversed_t0(c);
    double b[4] = {0.0, 0.0, 0.0, 0.0};   // B_v; non-total: G_v
    double q[4] = {0.0, 0.0, 0.0, 0.0};   // non-total: Q_v
    if constexpr (SPARSE)
      gather_picked(a, n, gb, ge, t0, Tn, b);
    else
      gather_upstream(a, gn, gb, ge, t0, Tn, b);
    if (TOTAL && has_g) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (t0 + j < Tn) b[j] *= exp_factor(en, a.aux_tab, t_minus, t0 + j);
    }
    for (int ci = cb; ci < ce; ++ci) {
      const int ch = as_const(a.child)[ci];
      const int fb = as_const(a.fac_begin)[ch], fe = as_const(a.fac_begin)[ch + 1];
      const double *__restrict__ ac = a.A + ((int64_t)ch * N + n) * T;
      int c_plus = -1;
      if constexpr (TOTAL) c_plus = as_const(a.tab)[3 * ch];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t s = t0 + j + 1;
        if (s >= Tn) continue;
        double term = letter_value(a, xn, fb, fe, s, -1);
        if constexpr (WEIGHTED) term *= exp_factor(en, a.aux_tab, t_minus, s);
        if constexpr (TOTAL) term *= exp_factor(en, a.aux_tab, c_plus, s);
        if constexpr (KIND == kGradNonTotal)
          q[j] += term * ac[s];
        else
          b[j] += term * ac[s];
      }
    }
    // the lane's own suffix sums (steps past the extent hold exact zeros), then the lanes from the right
    double excl0 = 0.0, excl1 = 0.0;
    if (scan0) {
      lane_suffix(b);
      excl0 = scan_publish(b[0], wave_total[c & 1][0]);
    }
    if constexpr (KIND == kGradNonTotal) {
      if (scan1) {
        lane_suffix(q);
        excl1 = scan_publish(q[0], wave_total[c & 1][1]);
      }
    }
    __syncthreads();   // (one barrier serves both scans)
    double off0 = 0.0, off1 = 0.0;
    if (scan0) off0 = scan_offset(wave_total[c & 1][0], excl0, carry0);
    if constexpr (KIND == kGradNonTotal) {
      if (scan1) off1 = scan_offset(wave_total[c & 1][1], excl1, carry1);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (t0 + j >= Tn) continue;
      double out = scan0 ? off0 + b[j] : 0.0;
      if (scan1) {
        const double r = off1 + q[j];   // R_v = dL/dy_v, kept for the gradient through the lookup
        if (a.R) a.R[((int64_t)v * N + n) * T + t0 + j] = r;
        const double sq = r * exp_factor(en, a.aux_tab, t_plus, t0 + j);
        out = scan0 ? out + sq : sq;
      }
      av[t0 + j] = out;
    }
  }
}

// The form of the upstream a call brings: pairs when a.pos is set (1 <= F <= kPickMaxFeatures,
// both tables there), G otherwise.
static bool sparse_upstream(const GradArgs &a, bool &ok) {
  ok = !a.pos || (a.w && a.F >= 1 && a.F <= kPickMaxFeatures);
  return a.pos != nullptr;
}

hipError_t launch_grad_suffix(const GradArgs &a, int kind, int first, int count, hipStream_t st) {
  bool ok;
  const bool sparse = sparse_upstream(a, ok);
  if (!ok) return hipErrorInvalidValue;
  switch (kind) {
    case kGradReals:
      return sparse ? launch_per_depth(grad_suffix_kernel<kGradReals, true>, a, first, count, st)
                    : launch_per_depth(grad_suffix_kernel<kGradReals, false>, a, first, count, st);
    case kGradTotal:
      return sparse ? launch_per_depth(grad_suffix_kernel<kGradTotal, true>, a, first, count, st)
                    : launch_per_depth(grad_suffix_kernel<kGradTotal, false>, a, first, count, st);
    case kGradNonTotal:
      return sparse ? launch_per_depth(grad_suffix_kernel<kGradNonTotal, true>, a, first, count, st)
                    : launch_per_depth(grad_suffix_kernel<kGradNonTotal, false>, a, first, count, st);
    default: return hipErrorInvalidValue;
  }
}

// ------------------------------------------------------------------ the carried sums of a weighted plan
// (one kernel for both bodies: they carry the same sums)
__global__ __launch_bounds__(256) void grad_prefix_kernel(GradArgs a, int first) {
  __shared__ double wave_total[2][4];
  const int64_t n = blockIdx.x;
  const int v = as_const(a.inner_nodes)[first + (int)blockIdx.y];
  const int64_t N = a.N, T = a.T, Tn = series_extent(a, n);
  const double *__restrict__ xn = a.X + n * a.D * T;
  const double *__restrict__ en = a.aux + n * a.aux_n;
  const int fb = as_const(a.fac_begin)[v], fe = as_const(a.fac_begin)[v + 1];
  const int ps = as_const(a.parent_srow)[v];
  const int t_plus = as_const(a.tab)[3 * v], t_pminus = as_const(a.tab)[3 * v + 2];
  const double *__restrict__ cp = ps >= 0 ? a.C + ((int64_t)ps * N + n) * T : nullptr;
  double *__restrict__ cv = a.C + ((int64_t)as_const(a.self_srow)[v] * N + n) * T;

  double carry = 0.0;   // sum of y_v over the chunks to the left
  const int64_t chunks = grad_chunks(Tn);
  for (int64_t c = 0; c < chunks; ++c) {
    const int64_t t0 = forward_t0(c);
    double y[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t t = t0 + j;
      if (t >= Tn) continue;
      double val = letter_value(a, xn, fb, fe, t, -1);
      if (ps >= 0) val = t > 0 ? val * cp[t - 1] * exp_factor(en, a.aux_tab, t_pminus, t) : 0.0;
      y[j] = val * exp_factor(en, a.aux_tab, t_plus, t);
    }
    // the lane's own prefix sums (steps past the extent hold exact zeros), then the lanes from the left
    y[1] += y[0];
    y[2] += y[1];
    y[3] += y[2];
    const double excl = scan_publish(y[3], wave_total[c & 1]);
    __syncthreads();
    const double off = scan_offset(wave_total[c & 1], excl, carry);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (t0 + j < Tn) cv[t0 + j] = off + y[j];
  }
}

hipError_t launch_grad_prefix(const GradArgs &a, int kind, int first, int count, hipStream_t st) {
  if (!grad_weighted(kind)) return hipErrorInvalidValue;
  return launch_per_depth(grad_prefix_kernel, a, first, count, st);
}

// ------------------------------------------------------------------ the segmented suffix scans
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

// KIND: kGradArctic or kGradBayesian; SPARSE as in grad_suffix_kernel.
template <int KIND, bool SPARSE>
__global__ __launch_bounds__(256) void grad_max_suffix_kernel(GradArgs a, int first) {
  __shared__ double wave_total[2][4];
  __shared__ int wave_head[2][4];
  const int64_t n = blockIdx.x;
  const int v = as_const(a.level_nodes)[first + (int)blockIdx.y];
  const int64_t N = a.N, T = a.T, Tn = series_extent(a, n);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double *__restrict__ xn = a.X + n * a.D * T;
  const double *__restrict__ gn = SPARSE ? nullptr : a.G + n * a.g_n;
  const double *__restrict__ sv = a.S + ((int64_t)as_const(a.self_srow)[v] * N + n) * T;
  double *__restrict__ av = a.A + ((int64_t)v * N + n) * T;
  const int gb = as_const(a.g_begin)[v], ge = as_const(a.g_begin)[v + 1];
  const int cb = as_const(a.child_begin)[v], ce = as_const(a.child_begin)[v + 1];

  double carry = 0.0;   // the open sum that enters the chunk from the right
  for (int64_t c = grad_chunks(Tn) - 1; c >= 0; --c) {
    const int64_t t0 = reversed_t0(c);
    // the heads, read off the recomputed S_v alone (steps past the extent hold none)
    double s[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) s[j] = (t0 + j >= 1 && t0 + j - 1 < Tn) ? sv[t0 + j - 1] : 0.0;
    bool h[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) h[j] = t0 + j < Tn && (t0 + j == 0 || s[j + 1] > s[j]);
    double b[4] = {0.0, 0.0, 0.0, 0.0};
    if constexpr (SPARSE)
      gather_picked(a, n, gb, ge, t0, Tn, b);
    else
      gather_upstream(a, gn, gb, ge, t0, Tn, b);
    for (int ci = cb; ci < ce; ++ci) {
      const int ch = as_const(a.child)[ci];
      const double *__restrict__ ac = a.A + ((int64_t)ch * N + n) * T;
      if constexpr (KIND == kGradArctic) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (t0 + j < Tn) b[j] += ac[t0 + j];
      } else {
        const int fb = as_const(a.fac_begin)[ch], fe = as_const(a.fac_begin)[ch + 1];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (t0 + j < Tn) b[j] += letter_value(a, xn, fb, fe, t0 + j, -1) * ac[t0 + j];
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
      if (t0 + j < Tn) av[t0 + j] = h[j] ? r : 0.0;
      in = h[j] ? 0.0 : r;
    }
  }
}

hipError_t launch_grad_max_suffix(const GradArgs &a, int kind, int first, int count, hipStream_t st) {
  bool ok;
  const bool sparse = sparse_upstream(a, ok);
  if (!ok) return hipErrorInvalidValue;
  switch (kind) {
    case kGradArctic:
      return sparse ? launch_per_depth(grad_max_suffix_kernel<kGradArctic, true>, a, first, count, st)
                    : launch_per_depth(grad_max_suffix_kernel<kGradArctic, false>, a, first, count, st);
    case kGradBayesian:
      return sparse ? launch_per_depth(grad_max_suffix_kernel<kGradBayesian, true>, a, first, count, st)
                    : launch_per_depth(grad_max_suffix_kernel<kGradBayesian, false>, a, first, count, st);
    default: return hipErrorInvalidValue;
  }
}

// ------------------------------------------------------------------ the input kernel
constexpr int kGradTile = 1024;   // time steps of a workgroup of grad_input_kernel (4 per lane, strided)

// dm_v[t]: A_v times what the node's letter multiplies in the forward pass.
template <int KIND>
__device__ __forceinline__ double input_dm(const GradArgs &a, const double *__restrict__ en, int v,
                                           int64_t n, int64_t t) {
  const int64_t N = a.N, T = a.T;
  const int ps = as_const(a.parent_srow)[v];
  double dm = a.A[((int64_t)v * N + n) * T + t];
  if constexpr (KIND == kGradReals) {
    // A_v * shift(S_p); shift(S)[0] = 0
    if (ps >= 0) dm *= t > 0 ? a.S[((int64_t)ps * N + n) * T + t - 1] : 0.0;
  } else if constexpr (KIND == kGradBayesian) {
    // A_v * S_p at the SAME step (no shift between the letters of a max semiring)
    if (ps >= 0) dm *= a.S[((int64_t)ps * N + n) * T + t];
  } else {
    // total: A_v E-_p E+_v shift(C_p); non-total: A_v E-_p shift(C_p); shift(C)[0] = 0
    if (ps >= 0)
      dm = t > 0 ? dm * exp_factor(en, a.aux_tab, as_const(a.tab)[3 * v + 2], t) *
                       a.C[((int64_t)ps * N + n) * T + t - 1]
                 : 0.0;
    if constexpr (KIND == kGradTotal) dm *= exp_factor(en, a.aux_tab, as_const(a.tab)[3 * v], t);
  }
  return dm;
}

template <int KIND>
__global__ __launch_bounds__(256) void grad_input_kernel(GradArgs a) {
  const int64_t row = blockIdx.x;   // (series, dimension)
  const int64_t N = a.N, D = a.D, T = a.T;
  const int64_t n = row / D, d = row - n * D;
  const int64_t Tn = series_extent(a, n);
  const double *__restrict__ xn = a.X + n * D * T;
  const double *__restrict__ en = grad_weighted(KIND) ? a.aux + n * a.aux_n : nullptr;
  const int ib = as_const(a.dim_begin)[d], ie = as_const(a.dim_begin)[d + 1];
#pragma unroll
  for (int e = 0; e < kGradTile / 256; ++e) {
    const int64_t t = (int64_t)blockIdx.y * kGradTile + e * 256 + (int)threadIdx.x;
    if (t >= T) continue;
    if (t >= Tn) {
      // behind the series' end: nothing was written there, nothing is read
      a.dX[row * T + t] = 0.0;
      continue;
    }
    double acc = 0.0;
    if constexpr (KIND == kGradArctic) {
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
        const double dm = input_dm<KIND>(a, en, v, n, t);
        const double others = letter_value(a, xn, as_const(a.fac_begin)[v], as_const(a.fac_begin)[v + 1], t, f);
        acc += dm * (dpow(x, as_const(a.fac)[2 * f + 1]) * others);
      }
    }
    a.dX[row * T + t] = acc;
  }
}

hipError_t launch_grad_input(const GradArgs &a, int kind, hipStream_t st) {
  void (*kernel)(GradArgs) = nullptr;
  switch (kind) {
    case kGradReals: kernel = grad_input_kernel<kGradReals>; break;
    case kGradTotal: kernel = grad_input_kernel<kGradTotal>; break;
    case kGradNonTotal: kernel = grad_input_kernel<kGradNonTotal>; break;
    case kGradArctic: kernel = grad_input_kernel<kGradArctic>; break;
    case kGradBayesian: kernel = grad_input_kernel<kGradBayesian>; break;
    default: return hipErrorInvalidValue;
  }
  if (a.N <= 0 || a.D <= 0 || a.T <= 0) return hipSuccess;
  const int64_t tiles = (a.T + kGradTile - 1) / kGradTile;
  if (a.N * a.D > 0x7fffffffLL || tiles > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kernel, dim3((unsigned)(a.N * a.D), (unsigned)tiles), dim3(256), 0, st, a);
  return hipGetLastError();
}

// ------------------------------------------------------------------ the gradient through the lookup
// (L1 / L2, whose g is a function of the series itself)
// dg[n, t] = dL/dg: g reaches L through the exp factors alone, and every term is a product of what
// the pass holds by now - one thread per (series, step), the nodes in the table's order.
//     total:      sum_v (alpha_v - alpha_p) dm_v m_v  -  sum over rows v of alpha_v G_v (C_v E-_v)
//     non-total:  sum over v with children of alpha_v R_v y_v  -  sum over v below depth 1 of alpha_p dm_v m_v
// dm_v is input_dm, y_v = m_v E-_p E+_v shift(C_p); nothing is divided by an exp factor.  C_v of the
// rows without children (total) and R_v (non-total) exist because the plan is armed.
template <int KIND>
__global__ __launch_bounds__(256) void grad_lookup_kernel(GradArgs a) {
  constexpr bool TOTAL = KIND == kGradTotal;
  const int64_t n = blockIdx.x;
  const int64_t N = a.N, T = a.T;
  const double *__restrict__ xn = a.X + n * a.D * T;
  const double *__restrict__ en = a.aux + n * a.aux_n;
  const double *__restrict__ gn = a.G + n * a.g_n;
#pragma unroll
  for (int e = 0; e < kGradTile / 256; ++e) {
    const int64_t t = (int64_t)blockIdx.y * kGradTile + e * 256 + (int)threadIdx.x;
    if (t >= T) continue;
    double acc = 0.0;
    for (int v = 0; v < a.V; ++v) {
      const int t_plus = as_const(a.tab)[3 * v], t_minus = as_const(a.tab)[3 * v + 1];
      const int t_pminus = as_const(a.tab)[3 * v + 2];
      const int ps = as_const(a.parent_srow)[v];
      const int fb = as_const(a.fac_begin)[v], fe = as_const(a.fac_begin)[v + 1];
      const double alpha_p = t_pminus >= 0 ? (double)as_const(a.alphas)[t_pminus >> 1] : 0.0;
      if constexpr (TOTAL) {
        const double alpha_v = (double)as_const(a.alphas)[t_plus >> 1];
        const double m = letter_value(a, xn, fb, fe, t, -1);
        acc += (alpha_v - alpha_p) * (input_dm<KIND>(a, en, v, n, t) * m);
        const int gb = as_const(a.g_begin)[v], ge = as_const(a.g_begin)[v + 1];
        if (ge > gb) {
          double gv = 0.0;
          for (int g = gb; g < ge; ++g) gv += gn[(int64_t)as_const(a.g_row)[g] * a.g_k + t * a.g_t];
          const double s = a.C[((int64_t)as_const(a.self_srow)[v] * N + n) * T + t] *
                           exp_factor(en, a.aux_tab, t_minus, t);
          acc -= alpha_v * (gv * s);
        }
      } else {
        if (as_const(a.child_begin)[v + 1] > as_const(a.child_begin)[v]) {
          const double alpha_v = (double)as_const(a.alphas)[t_plus >> 1];
          double y = letter_value(a, xn, fb, fe, t, -1) * exp_factor(en, a.aux_tab, t_plus, t);
          if (ps >= 0)
            y = t > 0 ? y * exp_factor(en, a.aux_tab, t_pminus, t) * a.C[((int64_t)ps * N + n) * T + t - 1] : 0.0;
          acc += alpha_v * (a.R[((int64_t)v * N + n) * T + t] * y);
        }
        if (ps >= 0) acc -= alpha_p * (input_dm<KIND>(a, en, v, n, t) * letter_value(a, xn, fb, fe, t, -1));
      }
    }
    a.dg[n * T + t] = acc;
  }
}

hipError_t launch_grad_lookup(const GradArgs &a, int kind, hipStream_t st) {
  if (!grad_weighted(kind) || !a.dg || !a.alphas || (kind == kGradNonTotal && !a.R)) return hipErrorInvalidValue;
  if (a.N <= 0 || a.T <= 0) return hipSuccess;
  const int64_t tiles = (a.T + kGradTile - 1) / kGradTile;
  if (a.N > 0x7fffffffLL || tiles > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kind == kGradTotal ? grad_lookup_kernel<kGradTotal> : grad_lookup_kernel<kGradNonTotal>,
                     dim3((unsigned)a.N, (unsigned)tiles), dim3(256), 0, st, a);
  return hipGetLastError();
}

// f'(dx_t) of the path length's summand at step t of dimension 0 `x`: sign(dx_t) (norm 1;
// sign(0) = 0, the subgradient of torch.abs) or 2 dx_t (norm 2); 0 at t = 0 and at t = T.
__device__ __forceinline__ double pathlen_weight(const double *__restrict__ x, int64_t t, int64_t T, int norm) {
  if (t < 1 || t >= T) return 0.0;
  const double d = x[t] - x[t - 1];
  if (norm == 1) return d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0);
  return 2.0 * d;
}

// dg through g = scale r / r_L, r = cumsum(f(dx_0)), r_L = r[T-1], into dimension 0 of dX: one
// workgroup per series.
//     dr[t] = scale dg[t] / r_L,   dr[T-1] -= (sum_s dg[s] g[s]) / r_L,   D[t] = sum over s >= t of dr[s]
//     dX_0[t] += w_t D[t] - w_(t+1) D[t+1]
// The two sums are block reductions - a lane's steps in rising order, the lanes by the wave scan,
// the four wave totals in wave order -; r_L is recomputed from X.  D is the suffix scan of the
// frame, chunks from the last to the first with a carry; D[t+1] of a lane's last step is what lies
// in front of the lane - scan_offset's value, chunk boundary included - so nothing is exchanged.
// A series with r_L = 0 (a constant dimension 0; T = 1) has g = 0 whatever the input does nearby
// as the forward pass defines it: it gets nothing, no 0 / 0.
__global__ __launch_bounds__(256) void grad_pathlen_kernel(GradArgs a) {
  __shared__ double total[2][4];
  __shared__ double wave_total[2][4];
  const int64_t n = blockIdx.x;
  const int64_t T = a.T;
  const double *__restrict__ x = a.X + n * a.D * T;
  const double *__restrict__ dgn = a.dg + n * T;
  const double *__restrict__ gn = a.lookup + n * T;
  double *__restrict__ dx = a.dX + n * a.D * T;
  const int64_t chunks = grad_chunks(T);

  double rl = 0.0, p = 0.0;
  for (int64_t c = 0; c < chunks; ++c) {
    const int64_t t0 = forward_t0(c);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t t = t0 + j;
      if (t >= T) continue;
      if (t >= 1) {
        const double d = x[t] - x[t - 1];
        rl += a.norm == 1 ? fabs(d) : d * d;
      }
      p += dgn[t] * gn[t];
    }
  }
  (void)scan_publish(rl, total[0]);
  (void)scan_publish(p, total[1]);
  __syncthreads();
  rl = ((total[0][0] + total[0][1]) + total[0][2]) + total[0][3];
  p = ((total[1][0] + total[1][1]) + total[1][2]) + total[1][3];
  if (rl == 0.0) return;   // (workgroup-uniform)
  const double tail = p / rl;

  double carry = 0.0;   // the sum of dr over the chunks to the right
  for (int64_t c = chunks - 1; c >= 0; --c) {
    const int64_t t0 = reversed_t0(c);
    double b[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t t = t0 + j;
      if (t >= T) continue;
      b[j] = a.scale * dgn[t] / rl;
      if (t == T - 1) b[j] -= tail;
    }
    lane_suffix(b);
    const double excl = scan_publish(b[0], wave_total[c & 1]);
    __syncthreads();
    const double off = scan_offset(wave_total[c & 1], excl, carry);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t t = t0 + j;
      if (t >= T) continue;
      const double d_here = off + b[j], d_next = j < 3 ? off + b[j + 1] : off;
      dx[t] += pathlen_weight(x, t, T, a.norm) * d_here - pathlen_weight(x, t + 1, T, a.norm) * d_next;
    }
  }
}

hipError_t launch_grad_pathlen(const GradArgs &a, hipStream_t st) {
  if (!a.dg || !a.lookup || (a.norm != 1 && a.norm != 2)) return hipErrorInvalidValue;
  if (a.N <= 0 || a.T <= 0) return hipSuccess;
  if (a.N > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(grad_pathlen_kernel, dim3((unsigned)a.N), dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace fr
