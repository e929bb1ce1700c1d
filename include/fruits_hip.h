/*
 * fruits_hip.h - C ABI of libfruits_hip.so: the MI355X (gfx950) implementation
 * of the FRUITS iterated-sums hot path (INC -> Reals ISS over SimpleWords ->
 * NPI / END [+ MPI]).
 *
 * Plain C: pointers, sizes, opaque handles.  No torch / HIP types in any
 * signature.  Every entry point names the reference interface it replaces
 * (paths relative to the irkri/fruits tree @ 2025-09-05).
 *
 * Conventions
 *   - "d_" pointers are DEVICE pointers (hipMalloc / torch CUDA tensors);
 *     "h_" pointers are HOST pointers.  All float data is IEEE binary64,
 *     C-contiguous, exactly like the reference's numba signatures
 *     (f8 arrays; i4 word tables; f4 alpha; i8 cuts).
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).
 *     Device entry points only ENQUEUE work once their plan has been PREPARED
 *     for the shape (fr_plan_prepare / fr_pipeline_prepare: the one-time upload
 *     of the plan's tables): they then never allocate, free or synchronise, so
 *     they may be captured into a hipGraph.  An unprepared plan is uploaded by
 *     its first run (an allocation + a synchronous copy); while the stream is
 *     being captured that run fails with FR_E_ARG instead of breaking the
 *     capture.  A plan's tables live on the device that was current at the
 *     first upload; running it with another device current fails with FR_E_ARG.
 *     Entry points are safe to call from several host threads (plans guard
 *     their own tables; launch-time caches are per device).
 *   - Return value: 0 = ok, <0 = error (FR_E_*); fr_last_error() returns a
 *     thread-local message.  Nothing here ever falls back to a CPU path: with
 *     no HIP device every compute call fails with FR_E_HIP.
 */
#ifndef FRUITS_HIP_H
#define FRUITS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FR_OK 0
#define FR_E_ARG (-1)    /* bad shape / null pointer / out-of-range value      */
#define FR_E_DIM (-2)    /* a word names a dimension > D (the reference reads
                            out of bounds silently, fruits/iss/semiring.py:146) */
#define FR_E_HIP (-3)    /* HIP runtime error (no device, launch failure, ...)  */
#define FR_E_NOMEM (-4)  /* workspace too small / allocation failure            */
#define FR_E_LIMIT (-5)  /* plan exceeds a compiled-in limit                    */
#define FR_E_INDEX (-6)  /* an index the reference would raise IndexError for
                            (END cut outside the series, fruits/sieving/segment.py:213-218) */

/* weighting modes of fr_plan_create */
#define FR_W_NONE 0      /* weighting is None  -> semiring.py:27-28,35 (alpha=0, lookup=0, total) */
#define FR_W_NONTOTAL 1  /* Weighting(total=False) -> _reals_single, semiring.py:93-125           */
#define FR_W_TOTAL 2     /* Weighting(total=True)  -> _total_weighted_reals_single, :128-158      */

/* plan flags */
#define FR_PLAN_SHARE_PREFIXES 1 /* walk the prefix trie (K scans); 0 = one chain
                                    per word, prefixes recomputed like the reference */
#define FR_PLAN_ARCTIC 2         /* (max, +) semiring instead of (+, x):
                                    Arctic._iterated_sum_fast, fruits/iss/semiring.py:282-400
                                    (argmax=False); "next" row of SURVEY.md 8f */
#define FR_PLAN_BAYESIAN 4       /* (max, x) semiring: Bayesian._iterated_sum_fast,
                                    fruits/iss/semiring.py:461-571 - the letters and exp
                                    weights of Reals, a running maximum, no shift */

#define FR_PLAN_ARCTIC_LETTER_SUM 8 /* with FR_PLAN_ARCTIC: the terms of one extended letter are
                                    summed first and their sum added to the prefix - the
                                    rounding of the argmax body (semiring.py:252-256) */

/* fr_plan_info selectors */
#define FR_INFO_ROWS 0       /* K = number of output rows (iterated sums)        */
#define FR_INFO_NODES 1      /* scan passes the device performs                  */
#define FR_INFO_LEVELS 2     /* register frames the walk needs                   */
#define FR_INFO_DIMS_USED 3  /* distinct input dimensions referenced             */
#define FR_INFO_MAX_DIM 4    /* highest dimension referenced (1-based)           */
#define FR_INFO_ALPHAS 5     /* distinct alpha values (exp tables = 2 per alpha) */
#define FR_INFO_GROUPS 6     /* independent sub-tries (upper bound of `groups`)  */
#define FR_INFO_SHARED 7     /* 1 if prefixes are shared                         */
#define FR_INFO_STAGED_ROWS 8 /* rows a workgroup stages in LDS per time chunk (input dimensions +
                                exp tables); fr_iss_run returns FR_E_LIMIT when they do not fit -
                                the caller then splits the word list */
#define FR_INFO_JIT_PROGRAMS 9 /* run-time compiled static programs loaded for this plan (fr_plan_jit) */
#define FR_INFO_AOT_PROGRAM 10 /* 1 + index of the pre-compiled static program (one group per series)
                                  the plan's records equal, 0: none */
#define FR_INFO_STATIC_TAIL 11 /* series that the plan's most recent fr_iss_run launch ran as the finer
                                  units of a tail program behind the whole-series units (the mixed
                                  static launch), 0: none */
#define FR_INFO_LAST_LAUNCH 12 /* how the plan's most recent fr_iss_run / fr_pipeline_run launched its
                                  walk, 0: it has not run one.  From bit 0: the kernel family (4 bits;
                                  1 interpreter, 2 ahead-of-time static program, 3 run-time compiled
                                  static program, 4 lean walk, 5 wave per series, 6 fused, 7 fused wave
                                  per series, 8 fused run-time compiled, 9 fused in pieces), groups per
                                  series (8), persistent grid (4), then one bit each: XCD-aware
                                  numbering, non-temporal input loads, write-through instance, an LDS
                                  pad was asked for, chunk carries in LDS; from bit 21 the resident
                                  round the groups were chosen from, from bit 41 that of the mixed
                                  static instance (20 bits each, 0: not asked) */
#define FR_INFO_LAST_WHOLE 13  /* ... and the series it ran as whole-series units (all of them unless
                                  FR_INFO_STATIC_TAIL reports finer ones behind them) */
#define FR_INFO_GRAD_ROWS 14   /* a CosWISS plan: the scratch fr_iss_backward needs, in rows of N * T
                                  doubles - bits 0 ... 31 the rows of d_A (F * (letters + 2): dL/dz of
                                  every letter of every word, then the trig tables), bits 32 and up
                                  the rows of d_S (F * (letters - W)); 0 for any other plan */

/* sieve kinds of fr_sieve_* and the fused pipeline */
#define FR_SIEVE_NPI 0 /* fruits/sieving/increment.py:101-129 */
#define FR_SIEVE_MPI 1 /* fruits/sieving/increment.py:132-163 */
#define FR_SIEVE_END 2 /* fruits/sieving/segment.py:203-225   */
#define FR_SIEVE_MAX 3 /* fruits/sieving/segment.py:107-153   */
#define FR_SIEVE_MIN 4 /* fruits/sieving/segment.py:155-200   */
#define FR_SIEVE_XPI 5 /* fruits/sieving/increment.py:166-198 */
#define FR_SIEVE_LPI 6 /* fruits/sieving/increment.py:201-239 */
#define FR_SIEVE_CUR 7 /* fruits/sieving/segment.py:228-272: sum of v*v over the in-band elements of the
                          inc-times differenced row (CUR itself: inc = 2); AVG / STD return the same */
/* the sieves of fruits/sieving/implicit.py: numbers of their own, valid in fr_sieve_implicit and
 * fr_pipeline_create only (fr_sieve knows neither) */
#define FR_SIEVE_PPV 16 /* fruits/sieving/implicit.py:11-153  */
#define FR_SIEVE_CPV 17 /* fruits/sieving/implicit.py:156-213 */
/* OR-ed into FR_SIEVE_PPV / FR_SIEVE_CPV at fr_pipeline_create: the `segments` form, Q1 - 1
 * bands q_j <= v < q_(j+1) instead of Q1 tests v >= q_j */
#define FR_SIEVE_SEGMENTS 0x200
/* OR-ed into a sieve's kind at fr_pipeline_create: its cuts are PER SERIES (coquantile
 * cuts, fruits/sieving/segment.py:51-64) - the sieve's `cuts` entries then name columns
 * ("slots") of the table given to fr_pipeline_set_series_cuts */
#define FR_SIEVE_SERIES_CUTS 0x100

typedef struct fr_plan fr_plan_t;
typedef struct fr_pipeline fr_pipeline_t;

/* ------------------------------------------------------------------ misc */
const char *fr_last_error(void);
int fr_version(void);
/* Number of HIP devices (0 when there is none; never an error). */
int fr_device_count(void);
/* Convenience for callers without their own allocator (cgo, plain ctypes). */
int fr_malloc(void **d_ptr, int64_t bytes);
int fr_free(void *d_ptr);
int fr_memcpy_h2d(void *d_dst, const void *h_src, int64_t bytes, void *stream);
int fr_memcpy_d2h(void *h_dst, const void *d_src, int64_t bytes, void *stream);
int fr_stream_sync(void *stream);

/* ------------------------------------------------------------------ plan
 * Replaces the word loop of _calculate_ISS (fruits/iss/iss.py:21-67) plus the
 * per-word marshalling of Semiring.iterated_sums (fruits/iss/semiring.py:14-41)
 * and CachePlan's depths (fruits/iss/cache.py:17-43).
 *
 *   W        number of words
 *   exps     concatenated exponent tables; word i is (L[i], Dw[i]) int32
 *            row-major == np.array(list(word), dtype=np.int32) (semiring.py:31)
 *   alpha    concatenated per-letter alphas (sum of L[i] floats) == word.alpha
 *            (fruits/iss/words/word.py:71-82); NULL when weighting == FR_W_NONE
 *   depth    depth[i] = CachePlan.unique_el_depth(i) in EXTENDED mode, 1 in
 *            SINGLE mode: number of trailing prefixes of word i that are output
 *            (0 is legal: CachePlan gives 0 to a word that is a prefix of an
 *            earlier word; it then contributes no rows)
 *   Output row order is the reference's: words in order, within a word the
 *   shortest emitted prefix first (iss.py:55-63).
 */
fr_plan_t *fr_plan_create(int32_t W, const int32_t *exps, const int32_t *L,
                          const int32_t *Dw, const float *alpha,
                          const int32_t *depth, int32_t weighting, int32_t flags);
void fr_plan_destroy(fr_plan_t *plan);
int64_t fr_plan_info(const fr_plan_t *plan, int32_t what);
/* Debug / test view of the compiled program: writes up to `cap` int32 words
 * (8 per node: level, flags, n_factors, n_emit, first_emit_row, emit_mul,
 * z_mul, group) and returns the number of nodes. */
int32_t fr_plan_dump(const fr_plan_t *plan, int32_t *buf, int32_t cap);
/* Debug / test view of the DEVICE program for `groups` groups per series: the
 * 64-byte node records (16 int32 words each, sentinel records included) in walk
 * order.  Returns the number of records; copies them when `cap_words` holds them. */
int32_t fr_plan_records(fr_plan_t *plan, int32_t groups, int32_t *buf, int64_t cap_words);
/* Debug / test view of the plan IN PIECES (csrc/plan.h, PiecedProgram): what the fused walk of a
 * large plan runs - the trie covered by items (a chain from the root, walked by the record loop,
 * and a body, a forest of whole sub-tries compiled as straight-line code), equal bodies one
 * piece TYPE with a kernel of its own, the output rows renumbered in walk order.  `max_piece`:
 * nodes of the largest body (0: the default).  Words: {types, K, node executions in chains,
 * nodes}; per type {body nodes, body rows, frames, units, items, nodes of the largest unit,
 * records, rows of the largest unit}, its records (16 words each: the body's - levels counted
 * from the chain's end, output rows from the body's first - then the chains, each closed by a
 * sentinel), its items (4 words: chain byte offset, walk position of the body's first row, nodes
 * of the unit in front, 0), units + 1 item offsets, a walk position per unit; then the output
 * row at every walk position.  Returns the number of words (copied when `cap_words` holds
 * them), 0 when the plan has no such cover. */
int64_t fr_plan_pieces(fr_plan_t *plan, int32_t max_piece, int32_t *buf, int64_t cap_words);
/* Debug / test view of the plan's STATIC schedule for `groups` groups per series (small
 * unweighted plans whose walk is compiled as straight-line code): 32 header words {entries,
 * staged rows, frames, groups, row sources [4..8), first entry of each group [8..16), rows
 * read by each group as bit masks [16..24)} followed by 16 words per entry (node records
 * with the input / output frame in words 14 / 15, "complete row r" entries of kind 0xfe,
 * "load the next unit's rows" 0xfd, a sentinel per group).  Returns the number of entries,
 * 0 when the plan does not qualify. */
int32_t fr_plan_static_schedule(fr_plan_t *plan, int32_t groups, int32_t *buf, int64_t cap_words);
/* Bytes of device workspace fr_iss_run needs for this plan and shape
 * (exp tables for weighted plans, chunk carries for T > one chunk). */
int64_t fr_plan_workspace_bytes(const fr_plan_t *plan, int64_t N, int64_t T,
                                int64_t lookup_rows);
/* 1 when a workgroup can stage the plan's rows (input dimensions + exp tables) of one
 * time chunk of a length-T series in LDS, 0 when fr_iss_run would return FR_E_LIMIT
 * (the caller then splits the word list). */
/* Run-time compiled static program of a small plan (hipRTC): what fr_plan_prepare does for a
 * materialising plan of at most 32 nodes that has no ahead-of-time program.  compile_only != 0:
 * compiles the schedule for `groups` groups per series WITHOUT touching a GPU and returns the
 * size of the code object (0: the plan has no static schedule; FR_E_LIMIT + message: hipRTC
 * missing or the compilation failed).  compile_only == 0: compiles and loads the programs on
 * the current device and returns how many the plan now has; `msg` receives why not. */
int32_t fr_plan_jit(fr_plan_t *plan, int32_t groups, int32_t compile_only, char *msg,
                    int64_t msg_cap);
int32_t fr_plan_fits(const fr_plan_t *plan, int64_t T);
/* One-time upload of the plan's device tables for batches of N series of length T
 * (`groups` as in fr_iss_run).  Allocates and synchronises - call it OUTSIDE a stream
 * capture; afterwards fr_iss_run for that (N, T, groups) only enqueues work.  The
 * reference's callers are synchronous and stateless (fruits/iss/semiring.py:43-52):
 * this is the explicit form of the state a device plan needs.  Idempotent. */
int fr_plan_prepare(fr_plan_t *plan, int64_t N, int64_t T, int32_t groups);

/* ------------------------------------------------------------------ ISS
 * Replaces Reals._iterated_sum_fast for ALL words of the plan in one launch
 * (fruits/iss/semiring.py:167-201, called per word from iss.py:55-63).
 *
 *   d_X            (N, D, T) f64
 *   d_lookup       (lookup_rows, T) f64, lookup_rows in {1, N}: Weighting.get_lookup
 *                  (fruits/iss/weighting.py:100-110, 148-160); a 1-row lookup is
 *                  broadcast over N (Indices); NULL iff the plan is FR_W_NONE
 *   d_out          element (k, n, t) is written at
 *                  d_out[k*out_k_stride + n*out_n_stride + t];
 *                  (K,N,T) results of iss.py:46 => strides (N*T, T);
 *                  (N,E,T) result of semiring.py:177 => strides (T, E*T)
 *   d_work         workspace of >= fr_plan_workspace_bytes() bytes (may be NULL
 *                  when that is 0)
 *   groups         0 = choose; otherwise number of sub-trie groups per series
 */
int fr_iss_run(fr_plan_t *plan, const double *d_X, int64_t N, int64_t D, int64_t T,
               const double *d_lookup, int64_t lookup_rows, double *d_out,
               int64_t out_k_stride, int64_t out_n_stride, void *d_work,
               int64_t work_bytes, int32_t groups, void *stream);

/* Drop-in for Semiring.iterated_sum_fast (fruits/iss/semiring.py:43-52,203-219),
 * host arrays in, host array out, synchronous:
 *   Z (N,D,T) f64, word (L,Dw) i32, alpha (L) f32, lookup (N,T) f64 or NULL
 *   (NULL = the unweighted call of semiring.py:27-28), extended in [1,L],
 *   total_weighting (bit 0; bit 1 set = Arctic semiring, semiring.py:354-400; bit 2 set =
 *   Bayesian semiring, semiring.py:530-571)
 *   -> out (N, extended, T) f64 (caller allocated). */
int fr_iterated_sum_fast_host(const double *h_Z, int64_t N, int64_t D, int64_t T,
                              const int32_t *word, int32_t L, int32_t Dw,
                              const float *alpha, const double *h_lookup,
                              int64_t extended, int32_t total_weighting,
                              double *h_out);

/* ------------------------------------------------------------------ INC
 * Replaces _increments (fruits/cache.py:8-13) as used by INC._transform
 * (fruits/preparation/transform.py:60-75): rows = N*D series of length T,
 * out[r, t] = x[r, t] - x[r, t-shift] for t >= shift, else 0; when
 * keep_head != 0 the first `head` values are copied from d_head_src instead
 * (zero_padding=False, transform.py:73-74). */
int fr_increments(const double *d_X, int64_t rows, int64_t T, int64_t shift,
                  double *d_out, const double *d_head_src, int64_t head, void *stream);

/* ------------------------------------------------------------------ lookups
 * L1.get_lookup (fruits/iss/weighting.py:148-160) on top of _L1_sum
 * (fruits/cache.py:25-31) and NRM (fruits/preparation/transform.py:184-198):
 * g[n,t] = scale * minmax_t(cumsum_t |x_0[t]-x_0[t-1]|), optionally divided by
 * (last + 1e-5) first (relative = 1); constant rows give 0.  relative = 2 returns
 * the raw cumulative path length (the SharedSeedCache entry, cache.py:108-112).
 * d_X is (N, D, T), only dimension 0 is read (cache.py:27).
 * norm: 1 = L1 (abs), 2 = L2 (square).  The path length is summed sequentially like
 * np.cumsum, so the lookup is bit-identical to the reference's (it decides exact ties of
 * max-plus results against fitted quantiles); norm | FR_LOOKUP_FAST uses a parallel scan
 * instead (re-associated sums, ~1e-16 relative) - enough for Reals plans. */
#define FR_LOOKUP_FAST 16
int fr_pathlen_lookup(const double *d_X, int64_t N, int64_t D, int64_t T,
                      int32_t norm, int32_t relative, double scale,
                      double *d_out /* (N,T) */, void *stream);

/* ------------------------------------------------------------------ sieves
 * Replace IncrementSieve._pre_transform + NPI/MPI/XPI/LPI._backend
 * (fruits/sieving/increment.py:63-71, 107-129, 138-163, 172-198, 207-239), MAX/MIN._backend
 * (fruits/sieving/segment.py:113-153, 161-200) and END._transform (segment.py:210-219) on a
 * materialised (N, T) iterated sum.  MAX / MIN: 0 for an empty segment AND for an empty band
 * (the reference raises ValueError there); XPI / LPI: 0 for an empty band.  FR_SIEVE_CUR
 * (CUR._backend, segment.py:242-260, with inc = 2): the sum of squares inside the band, 0 for
 * an empty one.
 *
 *   d_A      (N, T) f64, row stride a_stride elements
 *   inc      >= 0: number of increment passes fused into the load
 *   d_cuts   (cut_rows, C1) i64, cut_rows in {1, N}; sorted, leading 0
 *            (segment.py:51-64); a 1-row table is broadcast over N
 *   d_q      (Q1) f64 sorted quantile thresholds (segment.py:66-85)
 *   d_out    feature (n, j*(Q1-1)+k) at d_out[n*out_stride + j*(Q1-1)+k]
 *            (END: Q1 is ignored, feature j at d_out[n*out_stride + j])
 */
int fr_sieve(int32_t kind, const double *d_A, int64_t N, int64_t T, int64_t a_stride,
             int32_t inc, const int64_t *d_cuts, int64_t cut_rows, int32_t C1,
             const double *d_q, int32_t Q1, double *d_out, int64_t out_stride,
             void *stream);

/* Replaces PPV._transform and CPV._transform (fruits/sieving/implicit.py:114-129, 169-190) on a
 * materialised (N, T) iterated sum: one pass over a row for all thresholds of the sieve.  The
 * indicator is closed BELOW - v >= q_j, or with `segments` q_j <= v < q_(j+1), evaluated per
 * element (the thresholds are taken as given, not sorted: a band with q_j > q_(j+1) is empty); a
 * NaN never counts, +inf counts against a finite threshold.  FR_SIEVE_PPV: count / T.
 * FR_SIEVE_CPV: 2 * (rising edges of the indicator at t >= 1) / n, n = T rounded up to even (the
 * first difference is zero-padded, fruits/cache.py:8-13: a component that starts at t = 0 is not
 * counted).  The counts are integers; the one division is correctly rounded.
 *
 *   kind     FR_SIEVE_PPV or FR_SIEVE_CPV (fr_sieve knows neither)
 *   d_A      (N, T) f64, row stride a_stride elements
 *   d_q      (Q) f64 thresholds in the sieve's order (implicit.py:99-112), Q >= 1
 *   segments 0: Q features; else Q - 1 (Q >= 2); at most 256 features (FR_E_LIMIT)
 *   d_out    feature (n, j) at d_out[n*out_stride + j]
 */
int fr_sieve_implicit(int32_t kind, const double *d_A, int64_t N, int64_t T, int64_t a_stride,
                      const double *d_q, int32_t Q, int32_t segments, double *d_out,
                      int64_t out_stride, void *stream);
/* The same on series of their own lengths: series n is d_A[n, :d_lengths[n]] ((N) int32 on the
 * device, 1 <= d_lengths[n] <= T, not checked); the indicator is counted there, PPV divides by
 * d_lengths[n], CPV by d_lengths[n] rounded up to even - what fr_sieve_implicit returns for the
 * truncated row.  The elements behind a series' length are never read. */
int fr_sieve_implicit_lengths(int32_t kind, const double *d_A, int64_t N, int64_t T, int64_t a_stride,
                              const int32_t *d_lengths, const double *d_q, int32_t Q,
                              int32_t segments, double *d_out, int64_t out_stride, void *stream);

/* ------------------------------------------------------------------ fused pipeline
 * ISS + sieves in ONE launch: replaces the loop of FruitSlice.transform
 * (fruits/fruit.py:538-550) - for every iterated sum, for every sieve,
 * sieve.transform(itsum) - without ever materialising the (K, N, T) tensor.
 * Sieves: NPI / MPI / XPI / CUR and MAX / MIN with inc -8 to 8, and END; integer cuts or
 * per-series cuts (FR_SIEVE_SERIES_CUTS).  LPI is not fused (FR_E_LIMIT).  FR_SIEVE_PPV /
 * FR_SIEVE_CPV (| FR_SIEVE_SEGMENTS): inc 0, C1 = 2 with the cuts {0, T}, Q1 = the number of
 * thresholds (>= 1; with segments >= 2), which h_quant holds in the SIEVE's order - they are not
 * sorted; Q1 features, Q1 - 1 with segments, as fr_sieve_implicit computes them.  With
 * FR_SIEVE_SERIES_CUTS the two cuts of a PPV / CPV are slots of the per-series table, the second
 * one holding the series' own length (fr_pipeline_set_lengths).  Feature (n, k*per_sum + col_s + j*(Q1_s-1) + q) is the reference's
 * column order (iterated sum, then sieve, then segment, then band).
 *
 *   kinds/incs/C1/Q1   per sieve; Q1 is ignored for END
 *   cuts               concatenated transformed cut rows (C1[s] values each: sorted,
 *                      leading 0, negative cuts already resolved for length T -
 *                      fruits/sieving/segment.py:51-64); an END cut c with c - 1 outside
 *                      [-T, T-1] fails with FR_E_INDEX (the reference raises IndexError)
 *   h_quant            HOST (K, q_stride) thresholds of every iterated sum (the fitted
 *                      sieve copies of fruit.py:484-496), q_stride =
 *                      fr_pipeline_info(p, 1) = sum of Q1 over all sieves but END;
 *                      fr_pipeline_set_quantiles resolves them with the cuts into a
 *                      device table of per-row feature ops (call once after fit; it
 *                      allocates and synchronises)
 *   d_feats            (N, feat_stride >= F) output, F = fr_pipeline_info(p, 2)
 * Returns FR_E_LIMIT from create when a sieve is outside the fused set (the caller
 * then uses fr_iss_run + fr_sieve).  fr_pipeline_info: 0 features per iterated sum,
 * 1 q_stride, 2 total features, 3 run-time compiled kernels the pipeline holds
 * (fr_pipeline_prepare), 4 those of them with the plan as straight-line code, 5 the kernels
 * of piece types loaded (a large plan in pieces, fr_pipeline_compile_plan). */
fr_pipeline_t *fr_pipeline_create(fr_plan_t *plan, int32_t n_sieves, const int32_t *kinds,
                                  const int32_t *incs, const int32_t *C1, const int32_t *Q1,
                                  const int64_t *cuts, int64_t T);
void fr_pipeline_destroy(fr_pipeline_t *pipeline);
int64_t fr_pipeline_info(const fr_pipeline_t *pipeline, int32_t what);
int64_t fr_pipeline_workspace_bytes(const fr_pipeline_t *pipeline, int64_t N,
                                    int64_t lookup_rows);
int fr_pipeline_set_quantiles(fr_pipeline_t *pipeline, const double *h_quant);
/* Build-time companion of fr_pipeline_prepare / fr_pipeline_compile_plan: compiles the kernels
 * a pipeline with thresholds of this KIND would get at run time - `h_quant` (K, q_stride) needs
 * the right infinities only (a band's shape is an immediate), every finite value stands for any
 * other - into the directory `dir` in the cache's file format, without a device: the sieves as
 * immediates, and the plan (a small one as straight-line code for `groups` groups per series, a
 * large one in pieces).  fruits_amd/gen_bundle.py builds fruits_amd/jit_bundle with it; the
 * library looks there behind the user's cache and in front of the compiler.  Returns the number
 * of code objects the directory now holds for this pipeline, < 0 on error (`msg`). */
int32_t fr_pipeline_bundle(fr_pipeline_t *pipeline, const double *h_quant, int32_t groups,
                           const char *dir, char *msg, int64_t msg_cap);
/* Fuses the slice's preparateurs into the launch: fr_pipeline_run then takes the RAW
 * (N, D, T) input and forms the prepared rows while it stages them - no prepared tensor is
 * written or read.  Covers the chains of the experiment fruits:
 *   inc_lag > 0, as_new == 0   INC(shift=inc_lag)           fruits/preparation/transform.py:60-75
 *   inc_lag > 0, as_new != 0   NEW(INC(shift=inc_lag))      fruits/preparation/wrapper.py:78-93
 *                              (2 D prepared dimensions: the raw ones, then their increments)
 *   standardize 1 / 2          followed by STD(var=False / True), std_eps
 *                                                           fruits/preparation/transform.py:141-147
 * (INC with depth 1 and zero padding, _increments of fruits/cache.py:8-13; STD per series
 * and dimension).  With STD one small pre-pass computes the row statistics into the
 * workspace (np.mean / np.std in numpy's own summation order: bit-identical); everything else
 * is the one fused launch.  D = raw input dimensions.  Every fused kernel forms the rows itself
 * (the cooperative walk and the wave-per-series kernels in their staging, CosWISS where it reads
 * a letter's rows); FR_E_LIMIT only for a CosWISS with per-unit inputs (the randomised ffn): the
 * caller then materialises the prepared input as before.
 * Call before fr_pipeline_workspace_bytes / fr_pipeline_prepare; (0, 0, 0) switches it off. */
int fr_pipeline_set_preparation(fr_pipeline_t *pipeline, int32_t D, int32_t inc_lag,
                                int32_t as_new, int32_t standardize, double std_eps);
/* fr_plan_prepare for the pipeline's plan and series length (after
 * fr_pipeline_set_quantiles): fr_pipeline_run for batches of N series then only
 * enqueues work (the exp-table kernel, the walk, the MPI finalize).  It also compiles the
 * pipeline's OWN walk kernel - the fused walk with the sieves' kinds, differencing orders
 * and cuts as immediates (hipRTC, one code object per sieve list and kernel instantiation,
 * cached on disk; ~2 s the first time on a machine, FRUITS_HIP_JIT=0: not) - which later
 * runs on this device launch instead of the generic instance; results are identical
 * (fr_pipeline_compile_plan: a second kernel that knows the plan too).  No
 * hipRTC, per-series cuts or rows with different op lists: the generic instance stays.
 * May be called from another thread than the one that runs the pipeline (a caller that does
 * not want to wait for the compiler): fr_pipeline_run takes the compiled kernel once it is
 * there. */
int fr_pipeline_prepare(fr_pipeline_t *pipeline, int64_t N, int32_t groups);
/* The second kernel of a pipeline: one that also knows the PLAN, for the group program a
 * batch of N series selects.  A plan of at most 128 nodes becomes straight-line code - nothing
 * of a node is loaded or decoded at run time (BASELINE configs[2]: 243 -> 177 us); of a larger
 * one the kernel knows the node SHAPES (level, flags, output rows: a body per shape, the record
 * loop stays; configs[3] / [4] on one GPU: 9.3 -> 8.7 ms, 17.7 -> 15.9 ms).  Apart from
 * fr_pipeline_prepare because of what it costs: seconds to tens of seconds of hipRTC per plan
 * (115 nodes as straight-line code: ~15 s), cached on disk like the other.  Same results; safe
 * from another thread like fr_pipeline_prepare. */
int fr_pipeline_compile_plan(fr_pipeline_t *pipeline, int64_t N, int32_t groups);
/* fr_pipeline_prepare + fr_pipeline_compile_plan with what the disk cache holds and nothing
 * else: the one-time uploads, and the pipeline's own kernels when an earlier process on this
 * machine compiled them (milliseconds); a miss compiles nothing and leaves no trace. */
int fr_pipeline_prepare_cached(fr_pipeline_t *pipeline, int64_t N, int32_t groups);
/* Per-series segment boundaries for the sieves created with FR_SIEVE_SERIES_CUTS: device
 * table (N, slots) int32, row n = the boundaries of series n (values in [0, T]; the slots of
 * one sieve sorted ascending, the first one its leading 0) - what
 * SegmentSieve._get_transformed_cuts (fruits/sieving/segment.py:51-64) returns for float
 * ("coquantile") cuts.  The table belongs to the caller and must stay valid until the runs
 * that use it have finished; it applies to the following fr_pipeline_run calls with exactly
 * N series. */
int fr_pipeline_set_series_cuts(fr_pipeline_t *pipeline, const int32_t *d_cuts, int64_t N,
                                int32_t slots);
/* Per-series lengths for the following fr_pipeline_run calls with exactly N series: device (N)
 * int32, 1 <= d_lengths[n] <= T (not checked); series n is its first d_lengths[n] elements, what
 * lies behind them must be finite and influences no feature.  The iterated sums need nothing (they
 * are causal); the lengths are read by
 *   - the statistics pre-pass of a fused STD (fr_pipeline_set_preparation): mean and deviation of
 *     the first d_lengths[n] prepared elements, in numpy's summation order for that length;
 *   - the divisions of PPV / CPV sieves created with FR_SIEVE_SERIES_CUTS (C1 = 2; the second
 *     slot holds the series' length, up to which the indicator is counted): count / length, and
 *     2 * count / (length rounded up to even).  Running such a pipeline without lengths fails.
 * The band sieves and END take a series' extent from the cut table alone
 * (fr_pipeline_set_series_cuts: cuts resolved for that length).  A pipeline with per-series cuts
 * has no run-time compiled kernel: it runs the generic instance.  The array belongs to the caller
 * and must stay valid until the runs that use it have finished; NULL: every series is T long. */
int fr_pipeline_set_lengths(fr_pipeline_t *pipeline, const int32_t *d_lengths, int64_t N);
int fr_pipeline_run(fr_pipeline_t *pipeline, const double *d_X, int64_t N, int64_t D, int64_t T,
                    const double *d_lookup, int64_t lookup_rows, double *d_feats,
                    int64_t feat_stride, void *d_work, int64_t work_bytes, int32_t groups,
                    void *stream);

/* IncrementSieve._pre_transform alone (fruits/sieving/increment.py:63-71, inc >= 0),
 * materialised: d_out (N, T) contiguous.  Used by fit, which needs the values for
 * np.quantile (fruits/sieving/segment.py:66-75). */
int fr_pre_transform(const double *d_A, int64_t N, int64_t T, int64_t a_stride, int32_t inc,
                     double *d_out, void *stream);

/* ------------------------------------------------------------------ fit ("next" row)
 * Order statistics for SegmentSieve._fit / IncrementSieve._fit
 * (fruits/sieving/segment.py:66-75, increment.py:73-74): np.quantile(X, q)
 * interpolates between the two order statistics around q*(n-1); job j returns the
 * job_rank[j]-th smallest (0-based) of the job_inc[j]-times differenced
 * (N, T) block number job_row[j] of the device tensor d_A (rows, N, T).  Exact
 * (radix select); synchronous (fit is not a capture path); its scratch is kept between calls -
 * fr_release_scratch frees it. */
int fr_select_ranks(const double *d_A, int64_t rows, int64_t N, int64_t T, int32_t n_jobs,
                    const int32_t *job_row, const int32_t *job_inc, const int64_t *job_rank,
                    double *h_out, void *stream);
/* The same in two halves, for a fit of several slices (fruits/fruit.py:110-121 fits them one after
 * the other): _begin queues every pass of the selection on `stream` and returns at once - nothing
 * is read back between the passes - so the caller can queue the next slice's iterated sums behind
 * it; _end waits for exactly this selection (an event), writes the n_jobs values and frees the
 * handle (h_out NULL: only waits and frees).  d_A must stay valid until _end.  A selection in
 * flight owns one of 8 scratch blobs per device (device memory + page-locked host memory);
 * FR_E_LIMIT (NULL, fr_last_error) when all are taken.  fr_select_ranks = _begin + _end. */
typedef struct fr_selection fr_selection_t;
fr_selection_t *fr_select_ranks_begin(const double *d_A, int64_t rows, int64_t N, int64_t T,
                                      int32_t n_jobs, const int32_t *job_row, const int32_t *job_inc,
                                      const int64_t *job_rank, void *stream);
int fr_select_ranks_end(fr_selection_t *selection, double *h_out);

/* frees the scratch blobs no selection is using */
int fr_release_scratch(void);

/* ------------------------------------------------------------------ STD ("next" row)
 * STD._transform with separately=True (fruits/preparation/transform.py:141-147):
 * every one of the rows = N*D series becomes (x - mean) / (std + eps); std is the
 * population standard deviation (np.std), or 1 when div_std == 0. */
int fr_standardize(const double *d_X, int64_t rows, int64_t T, int32_t div_std, double eps,
                   double *d_out, void *stream);
/* The same on series of their own lengths: d_X is (N, D, T), row (n, d) is standardised with the
 * mean and deviation of its first d_lengths[n] elements ((N) int32 on the device, 1 <=
 * d_lengths[n] <= T, not checked), summed in numpy's order for that length - bit for bit what
 * fr_standardize returns for the truncated row.  The tail [d_lengths[n], T) of d_out is 0. */
int fr_standardize_lengths(const double *d_X, int64_t N, int64_t D, int64_t T,
                           const int32_t *d_lengths, int32_t div_std, double eps, double *d_out,
                           void *stream);

/* ------------------------------------------------------------------ CosWISS ("next" row)
 * CosWISS.batch_transform without ffn / dropout (fruits/iss/cos.py:11-49,167-181,
 * 289-330): the cosine weighted iterated sums of W simple words (exps / L / Dw as in
 * fr_plan_create) for n_freqs frequencies (float32 like the reference's f4 argument),
 * cosine exponent 1..8, optionally with total weighting.  The result is a plan like
 * any other: fr_iss_run writes its K = W*n_freqs rows (row = word*n_freqs + freq,
 * cos.py:167-181; d_lookup is ignored), fr_plan_workspace_bytes sizes the sin / cos
 * tables the run computes, and fr_pipeline_create fuses the sieves onto it.  The device
 * kernel sums the reference's (exponent+1)^(p-1) terms in factorised form, letter by
 * letter ((exponent+1) scans per letter) - equal up to re-association rounding. */
fr_plan_t *fr_plan_create_coswiss(int32_t W, const int32_t *exps, const int32_t *L,
                                  const int32_t *Dw, int32_t n_freqs, const float *freqs,
                                  int32_t exponent, int32_t total_weighting);

/* The randomised variants of CosWISS (fruits/iss/cos.py:51-164; state drawn by
 * CosWISS._fit :248-263).
 * dropout: _leaky_coswiss_single zeroes the summand of letter k at dropout[k] before its
 *   cumsum (:80).  h_indices (W, n_freqs, Lmax, rate) int32 HOST array =
 *   CosWISS._dropout_indices; T = series length the indices were drawn for.  The plan keeps
 *   a device mask; fr_iss_run / fr_pipeline_run then apply it (Lmax = 0 switches it off).
 *   Allocates and synchronises (call it after fit, outside a capture).
 * ffn: _ffn_coswiss sends the input of every (word, frequency) through _ffn first (:93-113,
 *   :128-135): fr_coswiss_ffn computes Z = C relu(A x + b) per time step for ONE (word,
 *   frequency) (d_A (hidden, D), d_b (hidden), d_C (D, hidden), d_Z (N, D, T); <= 64
 *   hidden units, <= 16 dimensions; enqueues one kernel), and
 *   fr_coswiss_set_input_stride(plan, s) makes unit j = word * n_freqs + freq of the plan
 *   read its input at d_X + j * s (s = N*D*T for the stacked Z's; 0 = all units share d_X). */
int fr_coswiss_set_dropout(fr_plan_t *plan, const int32_t *h_indices, int32_t Lmax, int32_t rate,
                           int64_t T);
int fr_coswiss_set_input_stride(fr_plan_t *plan, int64_t unit_stride);
int fr_coswiss_ffn(const double *d_X, int64_t N, int64_t D, int64_t T, const double *d_A,
                   const double *d_b, const double *d_C, int32_t hidden, double *d_Z,
                   void *stream);

/* The reference's own formulation, term by term, for exponents beyond the kernels above:
 * the cosine weighted ISS (fruits/iss/cos.py:11-49) expands cos(a-b)^s into products of
 * sin / cos powers (cos.py:265-287); every product ("term") is an ordinary Reals ISS of
 * the word over the input extended by one sin and one cos row per frequency, i.e. a
 * fr_plan_create / fr_iss_run program (the terms of all words share prefixes).  This
 * entry point is the remaining reduction `result += weightings[i,0] * tmp` with the
 * total-weighting factors of cos.py:38-48:
 *   d_out[j*out_row_stride + n*T + t] =
 *       sum_{i in [d_begin[j], d_begin[j+1])} d_coeff[i] * d_terms[d_desc[3i], n, t]
 *                                             * sin[t]^d_desc[3i+1] * cos[t]^d_desc[3i+2]
 * summed in ascending i.  d_terms (n_terms, N, T); d_trig (2, T) = sin, cos of one
 * frequency; all pointers device memory.  Enqueues one kernel, no allocation. */
int fr_coswiss_combine(const double *d_terms, int64_t n_terms, int64_t N, int64_t T,
                       int32_t n_out, const int32_t *d_begin, const double *d_coeff,
                       const int32_t *d_desc, const double *d_trig, double *d_out,
                       int64_t out_row_stride, void *stream);

/* ------------------------------------------------------------------ Arctic argmax ("next" row)
 * Arctic(argmax=True): _arctic_argmax_single (fruits/iss/semiring.py:239-284, dispatched
 * from Arctic._iterated_sum_fast :370-378).  The running maxima of EVERY prefix of every word
 * come from an FR_PLAN_ARCTIC plan whose depths are the word lengths (fr_iss_run ->
 * d_V (rows, N, T), rows = sum of L); this entry point derives the positions of the maxima
 * (d_P, scratch of the same shape: the index at which the running maximum was last raised)
 * and assembles the reference's rows: per word and prefix k the values, then the positions
 * of letters 1..k+1 back-tracked from the final position of the next letter (:275-283).
 * d_jobs (n_jobs, 3) int32 on the device, one job per (word, prefix k):
 * {first row of the word in d_V, k, first output row of the prefix = base_w + k + k(k+1)/2};
 * d_out (sum of L + L(L+1)/2, N, T).  Words of <= 63 letters.  Enqueues two kernels. */
int fr_arctic_argmax(const double *d_V, int64_t rows, int64_t N, int64_t T, int32_t n_jobs,
                     const int32_t *d_jobs, double *d_P, double *d_out, void *stream);

/* The same rows straight into features: a pipeline over an FR_PLAN_ARCTIC |
 * FR_PLAN_ARCTIC_LETTER_SUM plan whose rows are all prefixes of `n_words` words of `lengths[w]`
 * letters (in the plan's order) then has sum of L + L(L+1)/2 OUTPUT rows - what FruitSlice.transform
 * sieves for ISS(semiring=Arctic(argmax=True)), fruits/fruit.py:538-550 over iss.py:140-146 - and
 * fr_pipeline_set_quantiles takes one row of thresholds per output row.  fr_pipeline_run materialises
 * the running maxima (sum of L rows, in the workspace) and ONE more kernel forms every argmax row
 * in LDS for the NPI / MPI / END ops that look at it: neither the positions nor the argmax rows are
 * written.  Call between fr_pipeline_create and fr_pipeline_set_quantiles.  FR_E_LIMIT (the caller
 * keeps fr_arctic_argmax + fr_sieve): a sieve differences more than twice or cumulates, or a row
 * of maxima and the positions of a word's prefixes (8 T + 2 L T bytes) exceed 60 KB of LDS. */
int fr_pipeline_set_argmax(fr_pipeline_t *pipeline, int32_t n_words, const int32_t *lengths);

/* ------------------------------------------------------------------ preparateurs
 * RIN / MAV, JLD / FFN, NRM and LAG of fruits/preparation/transform.py on (N, D, T) device
 * rows; each enqueues ONE kernel, allocates nothing and never writes d_X (d_out must be another
 * buffer).  T >= 1.  The grouping tables of RIN / JLD are given twice: d_ndim (O) / d_dims (J)
 * for the kernel and the same values on the host (h_ndim / h_dims), which are checked here -
 * group sizes that do not add up to J fail with FR_E_ARG, a dimension outside [0, D) with
 * FR_E_DIM - so no kernel ever reads outside its input. */

/* Grouped causal FIR.  mode 0 = RIN._backend (transform.py:447-468): output dimension o owns
 * the slots j in [start_o, end_o) (prefix sums of ndim), d_kernel is (J, w), J <= D and
 *   out[n,o,k] = sum_j ( X[n,j,k] - sum_{l<w} X[n,dims[j],k-w+l] * kernel[j,l] )  for k >= w,
 * 0 for k < w (the self term is dimension j, not dims[j]: transform.py:465); 0 <= w < T
 * (w = 0, the kernel of a series of length 1: the self terms alone).
 * adaptive != 0 (transform.py:536-543): the input counts as padded with w leading zeros and
 * the first w outputs are dropped (any w).
 * mode 1 = MAV._backend (transform.py:233-239): out[n,d,k-1] = sum(X[n,d,k-w:k]) / w for
 * k = w .. T, 0 in front; 1 <= w <= T; the tables and J, O are ignored.  d_out (N, O, T). */
int fr_prep_fir(const double *d_X, int64_t N, int64_t D, int64_t T, const double *d_kernel,
                int32_t J, int32_t w, const int32_t *d_ndim, int32_t O, const int32_t *d_dims,
                const int32_t *h_ndim, const int32_t *h_dims, int32_t mode, int32_t adaptive,
                double *d_out, void *stream);

/* Per-time-step map across dimensions.  hidden == 0 = JLD._backend (transform.py:651-670):
 *   out[n,o,t] = sum_{j in group o} ( X[n,dims[j],t] * kernel[j] + bias[o] )
 * (the bias inside the sum, like the reference).  hidden > 0 = FFN._transform
 * (transform.py:362-376): out = W2 relu(W1 (x - mean) + b1) with d_W1 (hidden, D), d_b1
 * (hidden), d_W2 (O, hidden); flags & 1: centre every row by its np.mean over time (numpy's
 * summation order), flags & 2: relu on the output; relu(v) = v * (v > 0).  The JLD tables are
 * then ignored; FR_E_LIMIT beyond 16 input or 16 output dimensions.  d_out (N, O, T). */
int fr_prep_project(const double *d_X, int64_t N, int64_t D, int64_t T, const double *d_kernel,
                    const double *d_bias, const int32_t *d_ndim, int32_t O, const int32_t *d_dims,
                    int32_t J, const int32_t *h_ndim, const int32_t *h_dims, const double *d_W1,
                    const double *d_b1, const double *d_W2, int32_t hidden, int32_t flags,
                    double *d_out, void *stream);

/* NRM._transform (transform.py:184-198): (x - min) / (max - min) per (series, dimension) row,
 * or per series over all its dimensions (scale_dim != 0); rows with min == max become 0.
 * Bit-identical to the reference.  d_out (N, D, T). */
int fr_prep_normalize(const double *d_X, int64_t N, int64_t D, int64_t T, int32_t scale_dim,
                      double *d_out, void *stream);

/* LAG._transform (transform.py:291-298): d_out (N, 2D, 2T - 1), row 2i = x_i[(s + 1) / 2]
 * (lead), row 2i + 1 = x_i[s / 2] (lag). */
int fr_prep_leadlag(const double *d_X, int64_t N, int64_t D, int64_t T, double *d_out,
                    void *stream);

/* Time masks: out = keep ? X : +0.0 (a select: a dropped NaN / infinity / negative value becomes
 * +0.0 exactly).  Replaces DIL._transform (fruits/preparation/filter.py:56-62), DOT._transform
 * (:189-194), PDD._transform (:252-258), the pseudo_shift branch of CTS._transform
 * (transform.py:940-941) and WIN._transform (filter.py:93-108).  keep is the AND of two sources,
 * either of which may be absent (both absent: a copy):
 *   d_mask: bit t % 32 of word t / 32 of `mask_words` = ceil(T / 32) 32-bit words, shared by all
 *     series (bits at and beyond T are ignored);
 *   d_cs / d_ce (both or neither): int64 per series, `n_windows` >= N of them; series n keeps
 *     the Python slice [cs[n] - 1 : ce[n]] of its rows - a start of -1 (cs = 0) is T - 1, an
 *     empty slice keeps nothing.  Any values are safe: the bounds are clamped to the row.
 * A lane pair that is dropped entirely is not read.  d_out (N, D, T). */
int fr_prep_mask(const double *d_X, int64_t N, int64_t D, int64_t T, const uint32_t *d_mask,
                 int64_t mask_words, const int64_t *d_cs, const int64_t *d_ce, int64_t n_windows,
                 double *d_out, void *stream);

/* Pointwise maps; `mode` picks one kernel instantiation:
 *   FR_PW_MUL / FR_PW_ADD - SPE._transform (transform.py:789-812): X * w or X + w with d_w
 *     (Nw, T).  X has Nx series and w has Nw; the two are equal or one of them is 1 (numpy's
 *     broadcast of X * wave[:, None, :], else FR_E_ARG) and d_out has max(Nx, Nw) series.
 *     flags & FR_PW_FLAG_SIN: d_w holds the phase and the kernel takes its sine.
 *   FR_PW_ROTATE - RPE._backend (transform.py:859-875), D == 2: out0 = c x0 - s x1,
 *     out1 = s x0 + c x1 with c = d_w (T), s = d_w2 (T); every product is rounded.
 *   FR_PW_POW - RDW._transform (transform.py:601-602): X ** w[d], d_w (D).
 *   FR_PW_SHIFT - CTS._transform (transform.py:943-944): out[t] = X[min(t + shift, T - 1)],
 *     shift >= 0 (at or beyond T: every value is the row's last).
 *   FR_PW_CLIP - QTC._transform (transform.py:990-1001): X > q ? v : X, with
 *     flags & FR_PW_FLAG_LOWER X < q ? v : X; NaN passes through.
 * Arguments a mode does not name are ignored.  d_out (max(Nx, Nw), D, T). */
#define FR_PW_MUL 0
#define FR_PW_ADD 1
#define FR_PW_ROTATE 2
#define FR_PW_POW 3
#define FR_PW_SHIFT 4
#define FR_PW_CLIP 5
#define FR_PW_FLAG_SIN 1
#define FR_PW_FLAG_LOWER 1
int fr_prep_pointwise(int32_t mode, const double *d_X, int64_t Nx, int64_t D, int64_t T,
                      const double *d_w, int64_t Nw, const double *d_w2, int64_t shift, double q,
                      double v, int32_t flags, double *d_out, void *stream);

/* ------------------------------------------------------------------ generic words
 * A generic word (fruits/iss/words/word.py, Word: extended letters of named letter functions)
 * is lowered on the host to an ordinary exponent table over VIRTUAL input rows
 * (fruits_amd/iss/lowering.py); these two entries form those rows and undo the time shift the
 * lowering gives the max-plus / max-times semirings.  Both only move data and take fabs.
 *
 * fr_letter_rows: d_out (N, Dv, T) with, for row r = (kind, source, shift) of the table,
 *   out[n,r,t] = f(src[n,source,t + shift])  where t + shift < T,  +0.0 past the end;
 *   FR_ROW_DIM: f = identity on d_X (N, D, T);  FR_ROW_ABS: f = fabs on d_X;
 *   FR_ROW_EXT: f = identity on d_ext (N, H, T), values a letter function gave on the host;
 *   FR_ROW_ONE: f = 1.0, or 0.0 with one_is_zero != 0 (the semiring's one of an empty extended
 *     letter); `source` is ignored.
 * The table is (Dv, 3) int32, given twice like the tables of fr_prep_fir: h_spec on the host
 * (every entry is checked: FR_E_ARG for an unknown kind, a negative shift or an EXT row without
 * d_ext, FR_E_DIM for a source outside its tensor) and d_spec, the copy the kernel reads.
 * d_out must not alias d_X or d_ext. */
#define FR_ROW_DIM 0
#define FR_ROW_ABS 1
#define FR_ROW_EXT 2
#define FR_ROW_ONE 3
int fr_letter_rows(const double *d_X, int64_t N, int64_t D, int64_t T, const double *d_ext,
                   int64_t H, const int32_t *d_spec, const int32_t *h_spec, int32_t Dv,
                   int32_t one_is_zero, double *d_out, void *stream);

/* fr_rows_unshift: d_A (K, N, T) -> d_out (K, N, T), a distinct buffer, with
 *   out[k,n,t] = t >= s_k ? A[k,n,t - s_k] : +0.0;
 * s_k >= 0 per row k (h_shift on the host, checked; d_shift the device copy), s_k >= T gives an
 * all-zero row.  FR_E_ARG when the two buffers overlap. */
int fr_rows_unshift(const double *d_A, int64_t K, int64_t N, int64_t T, const int32_t *d_shift,
                    const int32_t *h_shift, double *d_out, void *stream);

/* ------------------------------------------------------------------ backward pass
 * The gradient of unweighted Reals iterated sums with respect to their input: the adjoint of
 * the recursion of fruits/iss/semiring.py:98-125 (per letter: tmp = tmp * prod_d Z[d]^el,
 * cumsum, then the shift by one step in front of the next letter).  Not in the reference.
 *
 * `prefix_plan`: an unweighted FR_W_NONE Reals plan whose words are the DISTINCT prefixes of
 *   the differentiated words, each with depth 1 - every node of its trie then emits exactly one
 *   row (FR_E_ARG otherwise); the trie, its parents, children and letters are read off it.
 * d_S (V, N, T), V = its rows: the output of fr_iss_run of that plan on d_X (layout K, N, T).
 * d_G: the upstream gradient of the K differentiated rows, element (n, k, t) at
 *   n * g_n_stride + k * g_k_stride + t * g_t_stride doubles (any strides >= 0, 0 included).
 * h_row_prefix (K, host): the row of `prefix_plan` that output row k is the iterated sum of;
 *   several k may name one prefix, a prefix may have none.
 * d_A (V, N, T): scratch.  d_dX (N, D, T): the gradient, every element written (dimensions no
 *   word names get zeros); must not alias d_X.
 * With B_v = G_v + sum over children c of (m_c A_c)[t+1], A_v = suffix sum of B_v:
 *   dX_d[t] = sum over nodes v of A_v[t] S_parent(v)[t-1] d m_v / d x_d [t]
 * (S_parent = 1 at depth 1).  x^(e-1) is formed by multiplication, so an input of 0 under a
 * positive exponent has a finite gradient.  The sums have one association whatever the grid:
 * the result is bit-identical from run to run.  The first call for a plan (or for another
 * h_row_prefix / D) uploads tables - it allocates and synchronises, so it cannot be captured
 * into a hipGraph; later calls only enqueue one launch per trie depth and one more.
 * FR_E_DIM: a word names a dimension beyond D.  FR_E_LIMIT: N, N * D or T beyond the grid.
 * A plan armed with fr_plan_set_grad_lengths: series n is its first L_n steps, T the row stride -
 * d_dX[n, :, :L_n] is the gradient of the call on the truncated series (its bits), d_dX[n, :, L_n:]
 * is +0.0, and d_G, d_S and d_X are not read at t >= L_n.  FR_E_ARG when N is not the N the
 * lengths were set for.
 *
 * THE SECOND CONTRACT: a CosWISS plan.  Handed a plan of fr_plan_create_coswiss - the plan itself,
 * no prefix plan - the entry runs the adjoint of the factorised CosWISS kernels: the gradient of
 * the plan's W * F rows (word-major, F rows per word) with respect to d_X, the sin / cos tables
 * being constants.  The arguments then mean:
 * d_G, its strides and d_dX: as above.  h_row_prefix (K, host): the row of the PLAN, 0 ... W * F - 1,
 *   that row k of d_G is the gradient of; several k may name one row, a row may have none - such a
 *   (word, frequency) unit is neither launched nor gathered.
 * d_S and d_A: scratch of the sizes FR_INFO_GRAD_ROWS reports, in rows of N * T doubles - d_S
 *   (bits 32 and up of the word) takes the recomputed forward rows u of every letter behind a
 *   word's first, d_A (bits 0 ... 31) dL/dz of every letter and the trig tables.  d_S is WRITTEN by
 *   the entry, despite its type, and not read before; the two must be distinct buffers.
 * Per (series, word, frequency) unit one workgroup recomputes the forward recursion in an
 * ascending sweep over the time chunks, then runs the adjoint in a descending one, S + 1 suffix
 * scans per letter behind one barrier; a second launch gathers d_dX.  One association per sum:
 * the same bits from run to run and however a batch is split into calls.  The first call for a
 * plan (or another h_row_prefix / D) uploads tables, as above; later calls enqueue three launches.
 * FR_E_DIM: a word names a dimension beyond D.  FR_E_LIMIT: N, N * D or T beyond the grid, an
 * exponent above 8 or a word of more than 16 letters.  FR_E_ARG: a row name outside the plan; a
 * plan with a dropout mask (fr_coswiss_set_dropout), with a per-unit input stride
 * (fr_coswiss_set_input_stride) or armed with fr_plan_set_grad_lengths - the CosWISS angle is a
 * function of T, per-series lengths have no meaning for it.  N == 0 or T == 0: FR_OK after the
 * same checks.  Every other plan that is not an unweighted Reals trie plan is refused (FR_E_ARG). */
int fr_iss_backward(fr_plan_t *prefix_plan, const double *d_X, int64_t N, int64_t D, int64_t T,
                    const double *d_S, const double *d_G, int64_t K, int64_t g_n_stride,
                    int64_t g_k_stride, int64_t g_t_stride, const int32_t *h_row_prefix,
                    double *d_A, double *d_dX, void *stream);

/* The same for the two max semirings: the gradient of unweighted Arctic (max, +) or Bayesian
 * (max, x) iterated sums with respect to their input - the adjoint of the recursions of
 * fruits/iss/semiring.py:282-309 (Arctic: tmp = tmp + el * Z[d] per dimension, running maximum,
 * NO shift between letters) and fruits/iss/semiring.py:461-493 (Bayesian: the letters of Reals,
 * running maximum, no shift).  Not in the reference.
 *
 * The arguments are those of fr_iss_backward; `prefix_plan` is the plan of the distinct
 * prefixes (depth 1 each) created with FR_PLAN_ARCTIC or FR_PLAN_BAYESIAN, unweighted, and d_S
 * its output on d_X.  FR_E_ARG, on the host and before any launch, for a Reals plan, a
 * weighted plan, an FR_PLAN_ARCTIC_LETTER_SUM plan, a CosWISS plan, a plan that is no prefix
 * plan, a bad row map, a null pointer or d_dX == d_X.
 *
 * With z_v = m_v (x) S_parent(v) (m_v alone at depth 1) and S_v the running maximum of z_v, a
 * HEAD of node v is a time s with s == 0 or S_v[s] > S_v[s-1] - strictly: of equal maxima the
 * FIRST wins, the rule of Arctic(argmax=True), fruits/iss/semiring.py:239-284 - read off d_S
 * alone; a head opens the segment [s, next head).  Deepest nodes first:
 *   B_v[t] = G_v[t] + sum over children c of w_c[t] A_c[t]     (w = 1 Arctic, m_c[t] Bayesian)
 *   A_v[s] = sum of B_v over the segment of s at a head s, 0.0 elsewhere
 *   Arctic:   dX_d[s] = sum over nodes v of e_vd A_v[s]
 *   Bayesian: dX_d[s] = sum over nodes v of A_v[s] S_parent(v)[s] d m_v / d x_d [s]
 * A segment's sum is formed from that segment's B alone.  For Arctic this is a subgradient of
 * max over i_1 <= ... <= i_p <= t of sum_k m_k[i_k] (at ties: the maximiser with the smallest
 * reversed index tuple); for Bayesian the same on positive inputs, and the gradient of the
 * reference's recursion as it stands elsewhere.  Bit-identical from run to run and whatever the
 * batch split; the tables are kept with the plan as fr_iss_backward keeps them.  Per-series
 * lengths (fr_plan_set_grad_lengths) as in fr_iss_backward: no head lies behind a series' end. */
int fr_iss_backward_max(fr_plan_t *prefix_plan, const double *d_X, int64_t N, int64_t D, int64_t T,
                        const double *d_S, const double *d_G, int64_t K, int64_t g_n_stride,
                        int64_t g_k_stride, int64_t g_t_stride, const int32_t *h_row_prefix,
                        double *d_A, double *d_dX, void *stream);

/* The same for WEIGHTED Reals iterated sums, total or not: the adjoint of both bodies of
 * fruits/iss/semiring.py:98-158 (_reals_single with alpha, :98-125; _total_weighted_reals_single,
 * :128-158) with respect to the input, the lookup g being a constant.  Not in the reference.
 *
 * `prefix_plan`: an FR_W_NONTOTAL or FR_W_TOTAL Reals plan whose words are the DISTINCT
 *   (letters, alphas) prefixes of the differentiated words, each with its slice of the alphas and
 *   depth 1.  FR_E_ARG, on the host and before any launch, for an unweighted plan (its entry is
 *   fr_iss_backward), an Arctic or Bayesian plan (fr_iss_backward_max takes the unweighted ones),
 *   a CosWISS plan, a plan that is no prefix plan, a bad row map, a null pointer, d_dX == d_X.
 * d_lookup (lookup_rows, T), lookup_rows in {1, N}: g, as fr_iss_run takes it.
 * d_G, K, the strides, h_row_prefix, d_dX: as in fr_iss_backward.
 * d_C (V, N, T), d_A (V, N, T), d_aux (2 * alphas * lookup_rows * T; alphas = FR_INFO_ALPHAS of
 *   the plan): scratch, distinct buffers.
 * With E+_v = exp(g alpha_v), E-_v = exp(-g alpha_v) of the node's last letter, p its parent and
 * the carried sums C_v = cumsum(y_v), y_v[t] = m_v[t] E-_p[t] E+_v[t] C_p[t-1] (depth 1:
 * m_v E+_v), which this entry forms itself - it does not need the plan's output - deepest first:
 *   total:      B_v[s] = G_v[s] E-_v[s] + sum_c m_c[s+1] E-_v[s+1] E+_c[s+1] A_c[s+1]
 *               A_v = suffix sum of B_v;   dm_v = A_v E-_p E+_v shift(C_p)
 *   non-total:  Q_v[s] = sum_c m_c[s+1] E-_v[s+1] A_c[s+1]
 *               A_v = suffix(G_v) + E+_v suffix(Q_v);   dm_v = A_v E-_p shift(C_p)
 *   dX_d[t] = sum over nodes v of dm_v[t] d m_v / d x_d [t]   (powers by multiplication)
 * Nothing is divided by an exp factor.  One association per sum whatever the grid: bit-identical
 * from run to run and whatever the batch split.  The plan need not fit a workgroup's LDS
 * (fr_plan_fits): the exp tables are read from d_aux.  Tables are kept with the plan as
 * fr_iss_backward keeps them; later calls enqueue the exp tables, two launches per trie depth
 * at most and one more.  FR_E_DIM / FR_E_LIMIT as fr_iss_backward.  Per-series lengths
 * (fr_plan_set_grad_lengths) as in fr_iss_backward; row n of an (N, T) d_lookup is then the
 * weighting's row for a series of L_n steps, and is not read behind them. */
int fr_iss_backward_weighted(fr_plan_t *prefix_plan, const double *d_X, int64_t N, int64_t D,
                             int64_t T, const double *d_lookup, int64_t lookup_rows,
                             const double *d_G, int64_t K, int64_t g_n_stride, int64_t g_k_stride,
                             int64_t g_t_stride, const int32_t *h_row_prefix, double *d_C,
                             double *d_A, double *d_aux, double *d_dX, void *stream);

/* ------------------------------------------------------------------ differentiable features
 * fr_sieve_pick: the SELECTING sieves END, MAX and MIN (fruits/sieving/segment.py:107-225) over
 * every row of a materialised (K, N, T) buffer of iterated sums in one launch: of each feature
 * its value - the bits fr_sieve returns for that row - and the position of the element it
 * selects, which is all a backward pass needs of it.  Not in the reference.
 *
 *   d_A      (K, N, T) f64, contiguous (the layout of fr_iss_run)
 *   h_spec, d_spec  (n_sieves, 6) i32, the same table on the host (every entry is checked
 *            there) and on the device: per sieve
 *              {kind, cut_begin, C1, q_begin, Q1, feat_begin}
 *            kind: FR_SIEVE_END, FR_SIEVE_MAX or FR_SIEVE_MIN; its cut row - sorted, leading 0,
 *            as fr_sieve takes it - is d_cuts[cut_begin ... cut_begin + C1), C1 >= 2; its sorted
 *            thresholds are d_q[q_begin ... q_begin + Q1), Q1 >= 2 (END: ignored); feat_begin:
 *            its first feature among the F of a row - the sieves' features follow each other
 *            without a gap, END has C1 - 1, MAX / MIN (C1 - 1) * (Q1 - 1) in (segment, band) order
 *   d_cuts   (n_cuts) i64, d_q (n_q) f64: the cut rows and thresholds of all sieves
 *   F        features of a row, 1 ... 256 (FR_E_LIMIT beyond)
 *   d_feat   (N, K, F) f64 and d_pos (N, K, F) i32: feature f of row (k, n) at (n * K + k) * F + f
 * END: the element at cut - 1, index -1 wrapping to T - 1; out of range: NaN and position -1.
 * MAX / MIN: of the elements t of the segment [cut_j, cut_(j+1)) with q_k < v <= q_(k+1) the
 * largest / smallest, and the FIRST t whose value equals it (np.argmax's rule; -0.0 equals +0.0);
 * an empty segment or band: 0.0 and position -1.  FR_E_ARG for a bad table, on the host and before
 * the launch.
 * PER-SERIES CUTS: a kind may carry FR_SIEVE_SERIES_CUTS - every sieve of the spec or none (a mix
 * is FR_E_ARG).  d_cuts is then an (N, n_cuts / N) table (FR_E_ARG when n_cuts is no multiple of
 * N), series n reads its own row, and cut_begin / C1 index into that row (the cut-row check is
 * made against the row's length).  Rows ascend in [0, T] behind their leading 0; an END row holds
 * the index plus one, wrapped for the series' own length already.  With cuts resolved for lengths
 * L_n every position is < L_n. */
int fr_sieve_pick(const double *d_A, int64_t K, int64_t N, int64_t T, const int32_t *d_spec,
                  const int32_t *h_spec, int32_t n_sieves, const int64_t *d_cuts, int64_t n_cuts,
                  const double *d_q, int64_t n_q, int32_t F, double *d_feat, int32_t *d_pos,
                  void *stream);

/* fr_iss_backward_picked: the backward pass of fr_iss_backward, fr_iss_backward_max or
 * fr_iss_backward_weighted - whichever the plan's kind names - with a SPARSE upstream gradient:
 * row (n, k) of the differentiated rows has F pairs (position, weight), pair f at
 * (n * K + k) * F + f of d_pos (i32) and d_w (f64), instead of T gradient values.  The weight
 * reaches step `position` of the row; a pair with a position < 0 reaches nothing.  No dense
 * (N, K, T) gradient exists anywhere.  What a node gathers is formed in a fixed order - its rows
 * in the order of h_row_prefix, a row's pairs in the order f = 0 ... F - 1, each added in turn -
 * so the result is the same bits from run to run and whatever the batch split, and the bits of
 * the dense entry on the scattered gradient wherever those sums are exact.
 *
 *   prefix_plan   a prefix plan of any of the three entries; it decides which adjoint runs
 *   d_S           (V, N, T): the plan's output on d_X - an unweighted plan's; else null
 *   d_lookup, lookup_rows, d_C, d_aux   a weighted plan's, as fr_iss_backward_weighted takes
 *                 them; else null / 0
 *   d_pos, d_w, K, F   the pairs; 1 <= F <= 256 (FR_E_LIMIT beyond); positions < T
 *   the rest      as in fr_iss_backward
 * FR_E_ARG, on the host and before any launch, for what the plan's own entry refuses and for a
 * null d_pos / d_w.  Per-series lengths (fr_plan_set_grad_lengths) as in fr_iss_backward: a pair
 * whose position is not below L_n reaches nothing. */
int fr_iss_backward_picked(fr_plan_t *prefix_plan, const double *d_X, int64_t N, int64_t D, int64_t T,
                           const double *d_S, const double *d_lookup, int64_t lookup_rows,
                           const int32_t *d_pos, const double *d_w, int64_t K, int32_t F,
                           const int32_t *h_row_prefix, double *d_C, double *d_A, double *d_aux,
                           double *d_dX, void *stream);

/* fr_sieve_heads: the heads a classifier is fed - END, MAX, MIN (as fr_sieve_pick) and the band
 * sieves MPI (fruits/sieving/increment.py:132-163) and CUR (fruits/sieving/segment.py:228-272; AVG
 * and STD return its numbers) - over every row of a materialised (K, N, T) buffer in ONE launch.
 * Not in the reference.  Everything is as in fr_sieve_pick except:
 *   h_spec, d_spec  (n_sieves, 7) i32: {kind, cut_begin, C1, q_begin, Q1, feat_begin, inc} per
 *            sieve.  inc: the differencing order of the rows the sieve looks at, D = E^inc row with
 *            (E a)[t] = a[t] - a[t-1], (E a)[0] = 0: 0 ... 8 for FR_SIEVE_MPI, 2 for FR_SIEVE_CUR,
 *            0 for the selecting sieves (anything else: FR_E_ARG).  MPI / CUR have
 *            (C1 - 1) * (Q1 - 1) features in (segment, band) order.
 *   d_comp   (N, K, F) i32, the companion of d_feat: the position of a selecting feature, the
 *            number of in-band elements c of an MPI / CUR feature.
 * MPI: the mean of the D[t] of the segment with q_k < D[t] <= q_(k+1), 0 for none - the bits
 * fr_sieve returns for that row.  CUR: the sum of their squares, each product rounded.
 *   hip_stream   the hipStream_t the launch is enqueued on, what the other entries call `stream`
 *            (here and in fr_sieve_heads_adjoint; both are run on a side stream behind an
 *            unfinished producer by tests/test_heads_gpu.py) */
int fr_sieve_heads(const double *d_A, int64_t K, int64_t N, int64_t T, const int32_t *d_spec,
                   const int32_t *h_spec, int32_t n_sieves, const int64_t *d_cuts, int64_t n_cuts,
                   const double *d_q, int64_t n_q, int32_t F, double *d_feat, int32_t *d_comp,
                   void *hip_stream);

/* fr_sieve_heads_adjoint: the gradient of the features of fr_sieve_heads with respect to the
 * rows: d_G (N, K, T) f64 contiguous, EVERY element written once (no memset, no atomics), to be
 * handed to fr_iss_backward / _max / _weighted as their upstream.  Thresholds and cuts are
 * constants.  With L = T, or d_lengths[n] clamped to [0, T]:
 *   MPI feature f:  weight w_f = d_g[f] / (double)c_f on D[t] for the t of its segment and band
 *   CUR feature f:  weight (2.0 * d_g[f]) * D[t]
 *   per sieve       u[t] = +0.0 plus the weights of the features that hold t, in column order;
 *                   its contribution is (E^T)^inc u,
 *                   (E^T u)[s] = (s >= 1 ? u[s] : 0.0) - (s + 1 < L ? u[s + 1] : 0.0)
 *   END, MAX, MIN   the pairs (position d_comp[f], d_g[f]) as fr_iss_backward_picked adds them
 *   d_G[s]          +0.0 plus the sieves' contributions in the order of the spec; +0.0 at s >= L
 * The band test runs on the rows again, which have to be the bits fr_sieve_heads saw: the elements
 * that receive weight are then exactly the c_f it counted.
 *   d_rows   (V, N, T) f64 contiguous; row (n, k) of the features is row h_row_map[k] of it
 *   h_row_map, d_row_map   (K) i32 in [0, V) on the host (checked) and on the device - the
 *            `h_row_prefix` of a backward entry, so that its prefix sums d_S serve as the rows; both
 *            NULL: V == K and row k is row k
 *   d_comp, d_g   (N, K, F): the companion fr_sieve_heads wrote and the feature gradients
 *   d_lengths     (N) i32 per-series lengths or NULL; the tables are then those of
 *                 fr_sieve_heads' call with per-series cuts
 *   the rest      as in fr_sieve_heads
 * FR_E_ARG / FR_E_LIMIT for what fr_sieve_heads refuses, a row map with one copy, an entry outside
 * [0, V), V != K without a map, a null pointer, d_G aliasing d_rows or d_g: on the host, before the
 * launch. */
int fr_sieve_heads_adjoint(const double *d_rows, int64_t V, const int32_t *d_row_map,
                           const int32_t *h_row_map, int64_t K, int64_t N, int64_t T,
                           const int32_t *d_spec, const int32_t *h_spec, int32_t n_sieves,
                           const int64_t *d_cuts, int64_t n_cuts, const double *d_q, int64_t n_q, int32_t F,
                           const int32_t *d_comp, const double *d_g, const int32_t *d_lengths, double *d_G,
                           void *hip_stream);

/* fr_plan_set_grad_lengths: per-series lengths for the backward passes that follow on this plan
 * - fr_iss_backward, fr_iss_backward_max, fr_iss_backward_weighted, fr_iss_backward_picked - with
 * exactly N series.  d_lengths: device (N) int32, 1 <= d_lengths[n] <= T (not checked); NULL
 * clears it.  A plan that was never armed, or is cleared, behaves exactly as before.
 * It takes no stream: it is state of the plan, delivered like fr_pipeline_set_lengths delivers a
 * pipeline's.  The pointer is stored under the plan's mutex; a backward entry reads it once, under
 * the same mutex, and hands it to its kernels by value - so replacing or clearing the lengths
 * while an earlier backward pass is still queued or running changes nothing of that pass.  The
 * table belongs to the caller and must stay valid, and unchanged, until the kernels that read it
 * have run.  FR_E_ARG, on the host: a null plan, N < 0; and from a backward entry, before any
 * launch, when its N is not the N the lengths were set for (the text names both). */
int fr_plan_set_grad_lengths(fr_plan_t *prefix_plan, const int32_t *d_lengths, int64_t N);

/* fr_plan_set_grad_pathlen: the gradient THROUGH the lookup for the fr_iss_backward_weighted calls
 * that follow on this plan with exactly N series - the weightings L1 and L2
 * (fruits/iss/weighting.py:113-210), whose g is the normalised cumulative path length of dimension
 * 0 of the input itself: g[t] = scale r[t] / r[T-1], r = cumsum(|dx_0|) (norm 1) or cumsum(dx_0^2)
 * (norm 2), r[0] = 0 - what fr_pathlen_lookup forms with `relative` 0 or 1 alike (the + 1e-5
 * cancels in the min-max normalisation).  Not in the reference.
 *   d_dg (N, T)     scratch: dL/dg, left there for the caller to read.  NULL clears the plan.
 *   d_R  (V, N, T)  scratch of a non-total plan (R_v below); ignored for a total one
 * It takes no stream and is delivered exactly like fr_plan_set_grad_lengths: stored under the
 * plan's mutex, read once by the entry under the same mutex and handed to its kernels by value.
 * A plan that was never armed, or is cleared, behaves exactly as before, bit for bit.
 * An armed fr_iss_backward_weighted wants lookup_rows == N, forms C_v of the output rows without
 * children too (total) or keeps R_v = suffix(Q_v) = dL/dy_v of the nodes with children (non-total),
 * and behind the input gather enqueues two more kernels on its stream.  With alpha_v the float32
 * alpha of node v's last letter, alpha_p its parent's (0 at depth 1), dm_v and m_v as above:
 *   total:      dg[t] = sum_v (alpha_v - alpha_p) dm_v[t] m_v[t]
 *                       - sum over output rows v of alpha_v G_v[t] S_v[t],   S_v = C_v E-_v
 *   non-total:  dg[t] = sum over v with children of alpha_v R_v[t] y_v[t]
 *                       - sum over v of depth >= 2 of alpha_p dm_v[t] m_v[t],   y_v = z_v E+_v
 *   dr[t] = scale dg[t] / r_L,   dr[T-1] -= sum_s dg[s] g[s] / r_L,   r_L = r[T-1]
 *   D[t] = sum over s >= t of dr[s]
 *   dX_0[t] += w_t D[t] - w_(t+1) D[t+1],   w_t = sign(dx_t) (norm 1) | 2 dx_t (norm 2), w_0 = w_T = 0
 * sign(0) = 0; a series with r_L = 0 (a constant dimension 0, T = 1) has g = 0 and gets nothing
 * from the lookup.  Nothing is divided by an exp factor; one association per sum whatever the grid.
 * FR_E_ARG, on the host: a null plan; with a d_dg, N < 0, a norm that is not 1 or 2, a scale that
 * is not finite, a plan that is not a weighted Reals trie plan, a non-total plan without d_R,
 * d_R == d_dg.  From an armed fr_iss_backward_weighted, before any launch: another N, lookup_rows
 * != N, a plan armed with fr_plan_set_grad_lengths too, a scratch that is one of the call's
 * buffers.  fr_iss_backward_picked refuses an armed plan. */
int fr_plan_set_grad_pathlen(fr_plan_t *prefix_plan, int64_t N, int32_t norm, double scale, double *d_dg,
                             double *d_R);

/* ------------------------------------------------------------------ Fruit.transform epilogue
 * np.nan_to_num(result, copy=False, nan=0.0) of Fruit.transform (fruits/fruit.py:172) on the
 * device-resident feature matrix, in place: NaN -> 0, +inf / -inf -> the largest / lowest
 * finite double (numpy's defaults).  d_x: `count` contiguous doubles. */
int fr_nan_to_num(double *d_x, int64_t count, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* FRUITS_HIP_H */
