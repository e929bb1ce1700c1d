// Internal interface between the C ABI (capi_*.cpp) and the HIP kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "launch_choice.h"   // walk_chunk_elems, packed_supported
#include "plan.h"
#include "walk_types.h"

namespace fr {

// deepest differencing order of a sieve (IncrementSieve): the sieves and the selection unroll to it
constexpr int kMaxInc = 8;
// blocks of 256 threads of a grid-stride launch over `total` elements, at most `cap`
inline unsigned grid_blocks(int64_t total, int64_t cap) {
  const int64_t blocks = (total + 255) / 256;
  return (unsigned)(blocks > cap ? cap : blocks);
}

int static_program_for(const NodeRec *recs, int n, int groups, const int32_t *row_src, int rows);
int static_program_tail_groups(int prog);
hipError_t launch_iss_walk(IssArgs &a, int levels, hipStream_t st);
hipError_t launch_mpi_finalize(double *feats, const double *cnt, int64_t N, int64_t stride,
                               const int32_t *cols, int n_cols, const int32_t *pairs, int n_pairs,
                               int per_sum, int K, hipStream_t st);
hipError_t launch_band_key_finalize(double *feats, int64_t N, int64_t stride, const int32_t *cols,
                                    int n_cols, int per_sum, int K, hipStream_t st);
hipError_t launch_implicit_finalize(double *feats, int64_t N, int64_t stride, const int32_t *cols,
                                    int n_cols, int per_sum, int K, int64_t T, const int32_t *lengths,
                                    hipStream_t st);
hipError_t launch_gather_row_blocks(const double *src, double *dst, int64_t N, int64_t src_stride,
                                    int64_t dst_stride, int K, int per_sum, const int32_t *walk_of_row,
                                    hipStream_t st);
hipError_t launch_exp_tables(const double *g, int64_t count, const float *alphas, int n_alpha,
                             double *aux, bool linear, hipStream_t st);
hipError_t launch_increments(const double *X, int64_t rows, int64_t T, int64_t shift, double *out,
                             const double *head_src, int64_t head, hipStream_t st);
hipError_t launch_pathlen_lookup(const double *X, int64_t N, int64_t D, int64_t T, int norm,
                                 int relative, double scale, int exact, double *out,
                                 hipStream_t st);
hipError_t launch_sieve(int kind, const double *A, int64_t N, int64_t T, int64_t a_stride, int inc,
                        const int64_t *cuts, int64_t cut_rows, int C1, const double *q, int Q1,
                        double *out, int64_t out_stride, hipStream_t st);
// PPV / CPV: Q thresholds, Q - 1 features with `segments`
constexpr int kImplicitMaxFeatures = 256;   // (8 KiB of integer counters per workgroup)
// (`lengths`, here and below: per-series lengths in [1, T], or nullptr - every series is T long)
hipError_t launch_sieve_implicit(int kind, const double *A, int64_t N, int64_t T, int64_t a_stride,
                                 const int32_t *lengths, const double *q, int Q, int segments,
                                 double *out, int64_t out_stride, hipStream_t st);
// jobs sorted so that the jobs of one group (<= kSelGroupMax, same row block) are adjacent;
// groups = int2 {first job, count}
constexpr int kSelGroupMax = 8;
constexpr int kSelTrackJobs = 2;     // jobs per group and differencing order whose successor the gather pass tracks
// (fruit_reduced's fit: 2048 23.0 ms - a few jobs per slice went on through five more digits -
// 4096 20.1, 8192 20.3, 16384 20.3)
constexpr int kSelSmallCap = 4096;   // candidates a job settles inside one workgroup (kernels_select.hip)
// job.pad bit 0: also return the next order statistic (succ[job] = its order key; all-ones
// when there is none); succ must be preset to all-ones
hipError_t launch_select_ranks(void *jobs, int n_jobs, const void *groups, int n_groups,
                               const int32_t *h_groups, void *groups_scratch, int max_inc,
                               bool untracked, int64_t N, int64_t T, unsigned int *hist, double *out,
                               unsigned long long *succ,
                               unsigned long long *cand, unsigned int *cand_count, hipStream_t st);
constexpr int kSelJobBytes = 32;
hipError_t launch_pre_transform(const double *A, int64_t N, int64_t T, int64_t a_stride, int inc,
                                double *out, hipStream_t st);
constexpr int kCosMaxExponent = 8;
hipError_t launch_coswiss(IssArgs &a, int exponent, hipStream_t st);
hipError_t launch_coswiss_ffn(const double *X, int64_t N, int64_t D, int64_t T, const double *A,
                              const double *b, const double *Cm, int hidden, double *Z,
                              hipStream_t st);
hipError_t launch_trig_tables(const float *freqs, int F, int64_t T, double *out, hipStream_t st);
hipError_t launch_coswiss_combine(const double *A, int64_t N, int64_t T, int n_out,
                                  const int32_t *begin, const double *coeff, const int32_t *desc,
                                  const double *trig, double *out, int64_t out_row_stride,
                                  hipStream_t st);
hipError_t launch_nan_to_num(double *x, int64_t count, hipStream_t st);
// (rows = series x D; `lengths` is per series)
hipError_t launch_standardize(const double *X, int64_t rows, int64_t T, const int32_t *lengths,
                              int64_t D, int div_std, double eps, double *out, hipStream_t st);
// Arctic argmax rows -> features (kernels_sieve.hip, argmax_sieve_kernel): `words` = device
// (n_words, 4) int32 {first V row, letters, first output row, 0}; the dynamic LDS of a workgroup
// (one row of V, the positions of a word's prefixes) must fit kArgmaxSieveLds
constexpr size_t kArgmaxSieveLds = 64 * 1024 - 4096;
size_t argmax_sieve_lds(int64_t T, int max_len);
hipError_t launch_argmax_sieves(const double *V, int64_t N, int64_t T, const void *words, int n_words,
                                int max_len, const FeatOp *ops, int n_ops, int n_ops_padded,
                                double *feats, double *cnt, int64_t feat_stride,
                                const int32_t *series_cuts, int cut_slots, hipStream_t st);
hipError_t launch_arctic_argmax(const double *V, int64_t rows, int64_t N, int64_t T, int n_jobs,
                                const int32_t *jobs, double *P, double *out, hipStream_t st);
hipError_t launch_row_stats(const double *X, int64_t N, int64_t D, int64_t T, const int32_t *lengths,
                            const int32_t *prep, int n_prep, int div_std, double eps, double *stats,
                            hipStream_t st);
// the preparateurs of kernels_prep.hip (RIN / MAV, JLD / FFN, NRM, LAG); hipErrorInvalidValue:
// a grid limit, or an FFN of more than 16 input / output dimensions
hipError_t launch_prep_fir(const double *X, int64_t N, int64_t D, int64_t T, const double *taps,
                           int w, const int32_t *ndim, int O, const int32_t *dims, int mode,
                           int adaptive, double *out, hipStream_t st);
hipError_t launch_prep_project(const double *X, int64_t N, int64_t D, int64_t T,
                               const double *kernel, const double *bias, const int32_t *ndim, int O,
                               const int32_t *dims, const double *W1, const double *b1,
                               const double *W2, int hidden, int flags, double *out,
                               hipStream_t st);
hipError_t launch_prep_normalize(const double *X, int64_t rows, int64_t len, double *out,
                                 hipStream_t st);
hipError_t launch_prep_leadlag(const double *X, int64_t rows, int64_t T, double *out,
                               hipStream_t st);
// the streaming preparateurs of kernels_filter.hip: time masks (DIL, WIN, DOT, PDD, CTS pseudo)
// and pointwise maps (SPE, RPE, RDW, CTS, QTC); hipErrorInvalidValue: a grid limit or an
// unknown mode.  The modes and flags are those of FR_PW_* in fruits_hip.h.
enum { PW_MUL = 0, PW_ADD = 1, PW_ROTATE = 2, PW_POW = 3, PW_SHIFT = 4, PW_CLIP = 5 };
enum { PW_FLAG_SIN = 1, PW_FLAG_LOWER = 1 };
struct PointwiseArgs {
  const double *X, *w, *w2;
  double *out;
  int64_t D, T;
  int64_t x_stride, w_stride;   // series strides of X and of the SPE table (0: one series)
  int64_t shift;
  double q, v;
  int flags;
};
hipError_t launch_prep_mask(const double *X, int64_t N, int64_t D, int64_t T, const uint32_t *mask,
                            const int64_t *cs, const int64_t *ce, double *out, hipStream_t st);
hipError_t launch_prep_pointwise(int mode, const PointwiseArgs &a, int64_t N, hipStream_t st);
// the virtual input rows of lowered generic words and the output unshift (kernels_letters.hip);
// `spec` = device (Dv, 3) int32 {kind, source, shift}, kinds = FR_ROW_* in fruits_hip.h;
// hipErrorInvalidValue: a grid limit
hipError_t launch_letter_rows(const double *X, int64_t N, int64_t D, int64_t T, const double *ext,
                              int64_t H, const int32_t *spec, int Dv, double one, double *out,
                              hipStream_t st);
hipError_t launch_rows_unshift(const double *A, int64_t K, int64_t N, int64_t T,
                               const int32_t *shift, double *out, hipStream_t st);
// The selecting sieves END / MAX / MIN over every row of a (K, N, T) buffer at once
// (kernels_pick.hip): value and position of each feature.  One sieve of the spec table.
struct PickSieve {
  int32_t kind;         // FR_SIEVE_END, FR_SIEVE_MAX or FR_SIEVE_MIN
  int32_t cut_begin;    // its sorted cut row with the leading 0: cuts[cut_begin ... cut_begin + C1)
  int32_t C1;
  int32_t q_begin;      // its sorted thresholds q[q_begin ... q_begin + Q1) (END: none, Q1 = 0)
  int32_t Q1;
  int32_t feat_begin;   // its first feature among the F of a row
};
// feat, pos: (N, K, F), row (k, n) of A at (n * K + k) * F; hipErrorInvalidValue: a grid limit.
// cut_stride: elements from one series' cut rows to the next (per-series cuts, every END row
// wrapped for its series already), 0: one table for all.
hipError_t launch_sieve_pick(const double *A, int64_t K, int64_t N, int64_t T, const PickSieve *spec,
                             int n_sieves, const int64_t *cuts, int64_t cut_stride, const double *q,
                             int F, double *feat, int32_t *pos, hipStream_t st);
// The heads END / MAX / MIN / MPI / CUR over every row of a (K, N, T) buffer at once and the
// expansion of their feature gradients into the rows' dense gradient (kernels_heads.hip, DESIGN.md
// 4.14.9).  One sieve of the spec table: a PickSieve and the differencing order.
struct HeadSieve {
  int32_t kind;         // FR_SIEVE_END, _MAX, _MIN, _MPI or _CUR
  int32_t cut_begin, C1, q_begin, Q1, feat_begin;   // as in PickSieve
  int32_t inc;          // D = E^inc row: MPI 0 ... kMaxInc, CUR 2, the selecting sieves 0
};
constexpr int kHeadsTile = 1024;   // time steps a workgroup of the expansion forms at once (256 lanes x 4)
// feat, comp: (N, K, F), row (k, n) of A at (n * K + k) * F; comp: the position of a selecting
// feature, the in-band count of an MPI / CUR one.  cut_stride as in launch_sieve_pick.
hipError_t launch_sieve_heads(const double *A, int64_t K, int64_t N, int64_t T, const HeadSieve *spec,
                              int n_sieves, const int64_t *cuts, int64_t cut_stride, const double *q,
                              int F, double *feat, int32_t *comp, hipStream_t st);
// G (N, K, T) contiguous, every element written.  Row (n, k) is rows[(row_map[k] * N + n) * T ...],
// row_map null: row k.  comp, g: (N, K, F); len: (N) int32 or null, clamped to [0, T].
hipError_t launch_sieve_heads_adjoint(const double *rows, const int32_t *row_map, int64_t K, int64_t N,
                                      int64_t T, const HeadSieve *spec, int n_sieves, const int64_t *cuts,
                                      int64_t cut_stride, const double *q, int F, const int32_t *comp,
                                      const double *g, const int32_t *len, double *G, hipStream_t st);
// the backward pass of the trie walk (kernels_grad.hip): which adjoint, and the
// tables of the prefix trie, all on the device.  Node v is the plan's node v (DFS preorder); CSR
// tables have V + 1 (D + 1) offsets.
enum GradKind : int {
  kGradReals = 0,   // unweighted Reals
  kGradTotal,       // weighted Reals, total
  kGradNonTotal,    // weighted Reals, non-total
  kGradArctic,      // (max, +): the exponent of a `fac` pair is the letter's coefficient
  kGradBayesian,    // (max, x)
};
struct GradArgs {
  const double *X;      // (N, D, T)
  const double *S;      // (V, N, T): row r = the iterated sum of the prefix with output row r (unweighted kinds)
  const double *G;      // upstream gradient, element (n, k, t) at n * g_n + k * g_k + t * g_t
  // ... or, with `pos` set, the SPARSE upstream of picked features: row (n, k)
  // is F pairs, pair f at n * g_n + k * g_k + f of both tables (G is null and g_t unused): the
  // weight w reaches step pos of the row, a pair with pos < 0 nothing
  const int32_t *pos;   // (N, K, F) positions in [-1, T)
  const double *w;      // (N, K, F) weights
  int F;                // pairs per row, 1 ... kPickMaxFeatures
  double *A;            // (V, N, T) scratch: the suffix sums, by node
  double *dX;           // (N, D, T), every element written
  int64_t N, D, T;
  int64_t g_n, g_k, g_t;
  const int32_t *parent_srow;             // row of S of the node's parent, -1 at depth 1
  const int32_t *child_begin, *child;     // the node's children
  const int32_t *fac_begin, *fac;         // the node's letter: pairs {dimension, exponent != 0}
  const int32_t *g_begin, *g_row;         // rows k of G that the node emitted in the forward pass
  const int32_t *level_nodes;             // the nodes by falling depth
  const int32_t *dim_begin, *dim_item;    // per input dimension: pairs {node, index into fac}
  const int32_t *self_srow;               // row of S of the node itself (the max semirings' heads)
  // what the exp weights add; null or 0 for the unweighted kinds.  C holds the
  // CARRIED sums C_v = cumsum(y_v), which the kernels form themselves; rows of C are numbered
  // like the rows of S (self_srow, parent_srow).
  double *C;            // (V, N, T) scratch: the carried sums of the nodes that have children
  const double *aux;    // (2 n_alpha, rows, T): table 2a = exp(+g alpha_a), 2a + 1 = exp(-g alpha_a)
  int64_t aux_tab;      // doubles from one table to the next (rows * T)
  int64_t aux_n;        // doubles from one series' row to the next (T; 0: one row for all)
  const int32_t *tab;   // three tables per node: its own E+, its own E-, its parent's E- (-1: unused)
  const int32_t *inner_nodes;   // the nodes that have children, by rising depth
  // per-series lengths, or null: series n is its first len[n] steps, 1 <=
  // len[n] <= T.  T stays the row stride of every buffer; the kernels walk, read and write A, S
  // and C below len[n] alone, and dX behind it is +0.0.
  const int32_t *len;           // (N)
  // the gradient through a path-length lookup: g = scale r / r[T-1], r the
  // cumulative |dx_0| (norm 1) or dx_0^2 (norm 2) of the series itself.  Null or 0 unless the plan
  // is armed (fr_plan_set_grad_pathlen); `len` is null then and the lookup has N rows.
  double *R;              // (V, N, T) scratch, non-total: R_v = suffix(Q_v) of the nodes that have children
  double *dg;             // (N, T) scratch: dL/dg
  const double *lookup;   // (N, T): g
  const float *alphas;    // the plan's distinct alphas: the exp tables 2a and 2a + 1 are alpha a's
  int V;                  // nodes of the trie
  int norm;
  double scale;
};
constexpr int kPickMaxFeatures = 256;   // features of a row of fr_sieve_pick, pairs of a row of the sparse upstream
constexpr int kGradChunk = 1024;   // time steps a workgroup scans at once (256 lanes x 4)
// Every launcher: hipErrorInvalidValue for a kind that is not its own, or a grid limit.
// A of `count` nodes of one depth, level_nodes[first ...]: their children's A must be complete.
// The scan launchers take the sparse upstream when a.pos is set, the dense one otherwise.
// Additive suffix sums (kGradReals, kGradTotal, kGradNonTotal) ...
hipError_t launch_grad_suffix(const GradArgs &a, int kind, int first, int count, hipStream_t st);
// ... and SEGMENTED ones between the heads of S_v, the gather without a shift (kGradArctic, kGradBayesian)
hipError_t launch_grad_max_suffix(const GradArgs &a, int kind, int first, int count, hipStream_t st);
// C of `count` nodes of one depth, inner_nodes[first ...]: their parents' C must be complete
// (kGradTotal, kGradNonTotal)
hipError_t launch_grad_prefix(const GradArgs &a, int kind, int first, int count, hipStream_t st);
// dX from the finished A (every kind)
hipError_t launch_grad_input(const GradArgs &a, int kind, hipStream_t st);
// dg from the finished A, C and - non-total - R (kGradTotal, kGradNonTotal; a.dg, a.alphas, a.V set)
hipError_t launch_grad_lookup(const GradArgs &a, int kind, hipStream_t st);
// dg through the normalised cumulative path length, ADDED into dX[:, 0, :]: behind launch_grad_input
// and launch_grad_lookup on the same stream (a.dg, a.lookup, a.norm, a.scale set)
hipError_t launch_grad_pathlen(const GradArgs &a, hipStream_t st);

// The backward pass of the factorised CosWISS kernels (kernels_grad_cos.hip).
// Unit j = w * F + f is (word w, frequency f); letter g is a letter of the whole program,
// letter_begin[w] <= g < letter_begin[w + 1].  Row g * F + f of DZ holds dL/dz of letter g in
// unit (w, f); row (g - w - 1) * F + f of U the recomputed u of a word's letters behind its first.
struct CosGradArgs {
  const double *X;      // (N, D, T)
  const double *G;      // upstream gradient, element (n, k, t) at n * g_n + k * g_k + t * g_t
  const double *trig;   // (F, 2, T): sin and cos rows of launch_trig_tables
  double *U;            // ((letters - W) * F, N, T) scratch
  double *DZ;           // (letters * F, N, T) scratch
  double *dX;           // (N, D, T), every element written
  int64_t N, D, T;
  int64_t g_n, g_k, g_t;
  int F, total;
  const int32_t *letter_begin;           // W + 1
  const int32_t *fac_begin, *fac;        // a letter: pairs {dimension, exponent != 0}
  const int32_t *g_begin, *g_row;        // per unit: the rows k of G that name it
  const int32_t *units;                  // the units some row of G names, ascending
  const int32_t *dim_begin, *dim_item;   // per input dimension: pairs {row of DZ, index into fac}
};
constexpr int kCosGradLetters = 16;   // letters of a word the unit kernel keeps carries for
// U and DZ of `count` units, units[first ...], for every series; exponent 1 ... kCosMaxExponent
hipError_t launch_grad_cos_units(const CosGradArgs &a, int exponent, int first, int count, hipStream_t st);
// dX from the finished DZ
hipError_t launch_grad_cos_input(const CosGradArgs &a, hipStream_t st);

}  // namespace fr
