// A fused pipeline (ISS -> sieves in one launch): its state, and what the walk runner
// (capi_walk.cpp) and the pipeline's entries (capi_pipeline.cpp) call of each other.
#pragma once
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <vector>

#include "capi_common.h"
#include "jit.h"
#include "kernels.h"

namespace fr::capi {

struct PipeSieve {
  int32_t kind, inc, Q1, col, q_off;
  bool series_cuts = false;    // cuts are slots of the per-series table (coquantile cuts)
  bool segments = false;       // PPV / CPV: Q1 - 1 bands q_j <= v < q_(j+1) instead of Q1 tests v >= q_j
  std::vector<int32_t> cuts;   // transformed, clamped to [0, T]
};

struct FusedArgs {          // non-null feats selects the fused sieve kernels
  const fr::FeatOp *ops = nullptr;
  double *feats = nullptr, *cnt = nullptr;
  int64_t feat_stride = 0;
  int32_t n_ops = 0, n_ops_padded = 0;
  bool has_mpi = false;     // cnt is a population table of its own
  fr_pipeline *pl = nullptr;   // the pipeline (its run-time compiled kernels), if any
  const int32_t *series_cuts = nullptr;   // device (N, cut_slots) per-series boundaries
  int32_t cut_slots = 0;
  bool total_inc = false;   // a differencing sieve on a totally weighted plan
  int carry_per_node = 3;   // chunk-carry slots of a node: 3, + 2 per differencing order >= 3
  // fused preparation: d_X is the raw input, the staging forms the prepared rows
  const int32_t *prep = nullptr;   // device (n_prep, 4) table
  const double *stats = nullptr;   // device (N, n_prep, 2) or nullptr (no STD)
  int32_t n_prep = 0;
  // a plan in pieces writes its features in walk order: (N, K * per_sum) scratch, and says so
  double *walk_feats = nullptr;
  const int32_t **walk_of_row = nullptr;   // set by the launch: the walk position of every output row
};

// The instantiation of the fused walk a (plan, series length, sieves) selects - what
// walk_inst.hip's dispatch picks at launch time, as a key for the run-time compiled variants.
inline fr::FusedKey fused_key_for(const fr::Plan &p, int64_t T, bool total_inc, bool high_order) {
  const int64_t chunk = fr::walk_chunk_elems(T);
  fr::FusedKey k{};
  k.E = chunk == 512 ? 2 : 4;
  k.LV = p.levels <= 2 ? 2 : (p.levels <= 4 ? 4 : (p.levels <= 6 ? 6 : 8));
  k.MULTI = T > chunk ? 1 : 0;
  k.W = p.weighting != 0 ? 1 : 0;
  k.SEMI = p.semiring;
  k.TI = (k.W && total_inc && p.weighting == FR_W_TOTAL) ? 1 : 0;
  k.TOTAL = (k.W && p.weighting == FR_W_TOTAL) ? 1 : 0;
  k.HO = (k.MULTI && high_order) ? 1 : 0;
  return k;
}

// LDS of a launch of piece type `pt` next to the feature window, and the window (0: none fits)
inline size_t piece_other_lds(const fr::Plan &p, const fr::PieceType &pt, int64_t T, int carry_per_node) {
  const int64_t chunk = fr::walk_chunk_elems(T);
  return ((size_t)p.rows_staged() * chunk + 24 + (T > chunk ? (size_t)carry_per_node * pt.max_unit_nodes : 0)) * 8;
}
inline int piece_window(const fr::Plan &p, const fr::PieceType &pt, int64_t T, int carry_per_node, int n_ops,
                        bool mpi, bool &fits) {
  return fr::feat_window_sized(pt.widest_node * n_ops, pt.max_unit_rows * n_ops,
                           piece_other_lds(p, pt, T, carry_per_node), mpi, fits);
}

// Shared body of fr_iss_run and fr_pipeline_run (capi_walk.cpp).
int run_walk(const char *who, fr::Plan &p, const double *d_X, int64_t N, int64_t D, int64_t T,
             const double *d_lookup, int64_t lookup_rows, double *d_out, int64_t out_k_stride,
             int64_t out_n_stride, void *d_work, int64_t work_bytes, int32_t groups,
             hipStream_t st, const FusedArgs *fu);

}  // namespace fr::capi

struct fr_pipeline {
  fr_plan_t *plan = nullptr;
  int64_t T = 0;
  int32_t per_sum = 0, q_stride = 0, n_ops = 0, n_ops_padded = 0;
  int32_t n_ops_eff = 0;           // ops per row after dropping NPI ops an MPI op covers
  std::vector<int32_t> npi_pairs;  // (npi column, mpi column) inside one iterated sum's block
  void *d_npi_pairs = nullptr;
  std::vector<fr::capi::PipeSieve> sieves;
  std::vector<int32_t> mpi_cols;   // columns inside one iterated sum's block
  std::vector<int32_t> key_cols;   // MAX columns (~column: MIN) inside one iterated sum's block
  // Arctic argmax (fr_pipeline_set_argmax): the OUTPUT rows are the L + L (L + 1) / 2 rows of every
  // word (running maxima and back-tracked positions, fruits/iss/semiring.py:239-284), not the
  // plan's; (n_words, 4) {first plan row, letters, first output row, 0}
  std::vector<int32_t> argmax_words;
  void *d_argmax_words = nullptr;
  int32_t argmax_rows = 0, argmax_max_len = 0;
  // PPV columns (~column: CPV) inside one iterated sum's block: the walk leaves counts there,
  // implicit_finalize_kernel divides them
  std::vector<int32_t> implicit_cols;
  void *d_implicit_cols = nullptr;
  int rows() const { return argmax_words.empty() ? plan->p->K : argmax_rows; }   // output rows
  void *d_ops = nullptr;           // (rows, n_ops_padded) FeatOp
  void *d_mpi_cols = nullptr;
  void *d_key_cols = nullptr;
  bool have_quantiles = false;
  // per-series cut table (fr_pipeline_set_series_cuts): device (cuts_N, cut_slots) int32, owned
  // by the caller; cut_slots_needed = 1 + the highest slot a sieve names
  const int32_t *d_series_cuts = nullptr;
  int64_t cuts_N = 0;
  int32_t cut_slots = 0, cut_slots_needed = 0;
  // per-series lengths (fr_pipeline_set_lengths): device (lengths_N,) int32 in [1, T], owned by
  // the caller; nullptr: every series is T long.  Read by STD's statistics pre-pass and by the
  // divisions of PPV / CPV; `implicit_series_cuts`: a PPV / CPV counts up to a slot of the cut table
  const int32_t *d_lengths = nullptr;
  int64_t lengths_N = 0;
  bool implicit_series_cuts = false;
  // fused preparation (fr_pipeline_set_preparation): 0 dims = none
  int32_t prep_D = 0, prep_n = 0, prep_std = 0;
  double prep_eps = 0.0;
  void *d_prep = nullptr;          // (prep_n, 4) int32
  // run-time compiled fused kernels (jit.cpp, walk_fused.h JitOps): the sieves' kind /
  // differencing order / shape / cuts, the same for every output row, as immediates; compiled by
  // fr_pipeline_prepare for the kernel instantiation the plan and T select, dropped when the
  // thresholds (and with them the ops) are set again
  // (fr_pipeline_prepare may run on another thread than fr_pipeline_run - a caller that does
  // not want to wait for the compiler: jit_mu guards this block, jit_gen says whether the ops a
  // compilation started from are still the pipeline's)
  std::mutex jit_mu;
  uint64_t jit_gen = 0;
  fr::FusedOps jit_ops;
  bool jit_uniform = false;        // every row's ops agree in what becomes an immediate
  std::map<uint32_t, fr::JitProgram> jit;
  std::map<uint32_t, std::string> jit_failed;
  std::set<uint32_t> jit_pending;  // being compiled right now
  // the same with the PLAN as an immediate too (small plans: walk_fused.h, fwalk_static), by
  // instantiation and groups per series: id | groups << 32
  std::map<uint64_t, fr::JitProgram> jit_static;
  std::set<uint64_t> jit_static_tried;
  // ... or, for a large plan, the plan in PIECES (plan.h, PiecedProgram; walk_fused.h,
  // fwalk_pieces): one kernel per piece type, by instantiation; the op table in walk order and
  // the walk position of every output row (uploaded by fr_pipeline_prepare on the caller's
  // thread; the kernels may come from a helper thread)
  std::vector<fr::FeatOp> h_ops;   // host copy of the op table
  struct Pieces {
    int max_piece = 0, device = -1;
    std::vector<fr::JitProgram> progs;   // one per piece type; empty: not compiled (yet)
    std::vector<char> fits;              // per type: compiled for units whose features fit the window
    void *d_tables = nullptr;
    const fr::FeatOp *d_ops_walk = nullptr;
    const int32_t *d_walk_of_row = nullptr;
  };
  std::map<uint32_t, Pieces> jit_pieces;
  std::set<uint32_t> jit_pieces_tried;
  void drop_pieces() {               // (caller holds jit_mu)
    for (auto &kv : jit_pieces) {
      for (fr::JitProgram &pr : kv.second.progs) fr::jit_unload(pr);
      if (kv.second.d_tables) (void)hipFree(kv.second.d_tables);
    }
    jit_pieces.clear();
    jit_pieces_tried.clear();
  }
};
