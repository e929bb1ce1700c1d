// The fused pipeline: the fr_pipeline_* entries, the table of feature ops and the run-time
// compilers of a pipeline's own kernels (sieves as immediates; small plans as straight-line code;
// large plans in pieces), with the bundle that ships them.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <limits>
#include <thread>
#include <utility>

#include "capi_pipeline.h"
#include "capi_plan.h"

namespace fr::capi {
namespace {

// Compiles (hipRTC, disk cache) and loads the pipeline's fused kernel with its sieves as
// immediates, once per instantiation; a failure leaves the pipeline on the generic kernel.
// (`cache_only`: from the disk cache or not at all - a miss leaves no trace, a later call compiles)
void ensure_fused_jit(fr_pipeline &pl, const fr::FusedKey &key, bool cache_only = false) {
  const uint32_t id = key.packed();
  fr::FusedOps ops;
  uint64_t gen;
  {
    std::lock_guard<std::mutex> lock(pl.jit_mu);
    if (!pl.jit_uniform || pl.jit.count(id) || pl.jit_failed.count(id) || pl.jit_pending.count(id))
      return;
    pl.jit_pending.insert(id);
    ops = pl.jit_ops;
    gen = pl.jit_gen;
  }
  fr::JitProgram prog;
  std::string err;
  const bool ok = fr::jit_fused(ops, key, prog, err, nullptr, cache_only);   // (seconds: nobody waits on a lock for it)
  std::lock_guard<std::mutex> lock(pl.jit_mu);
  pl.jit_pending.erase(id);
  if (!ok && cache_only && fr::jit_not_cached(err)) return;
  if (gen != pl.jit_gen) {   // the thresholds were set again meanwhile: not this pipeline's kernel
    if (ok) fr::jit_unload(prog);
    return;
  }
  if (ok)
    pl.jit[id] = prog;
  else
    pl.jit_failed[id] = err;
}

// The straight-line variant for the group program `gp` (a copy of its records goes into the source).
void ensure_fused_static(fr_pipeline &pl, const fr::FusedKey &key, const fr::FusedPlan &plan,
                         bool cache_only = false) {
  const uint64_t id = (uint64_t)key.packed() | (uint64_t)plan.groups() << 32;
  fr::FusedOps ops;
  uint64_t gen;
  {
    std::lock_guard<std::mutex> lock(pl.jit_mu);
    if (!pl.jit_uniform || pl.jit_static.count(id) || pl.jit_static_tried.count(id)) return;
    pl.jit_static_tried.insert(id);
    ops = pl.jit_ops;
    gen = pl.jit_gen;
  }
  fr::JitProgram prog;
  std::string err;
  const bool ok = fr::jit_fused(ops, key, prog, err, &plan, cache_only);
  std::lock_guard<std::mutex> lock(pl.jit_mu);
  if (!ok && cache_only && fr::jit_not_cached(err)) pl.jit_static_tried.erase(id);
  if (gen != pl.jit_gen) {
    if (ok) fr::jit_unload(prog);
    return;
  }
  if (ok) pl.jit_static[id] = prog;
}

// ---- a large plan in pieces (plan.h, PiecedProgram) ----------------------------------------
// Plans of more than kFusedStaticMaxNodes nodes (developer knobs: pieces=0 - never;
// piece_min=M - from M nodes on; piece_nodes=P - pieces of at most P nodes).
// Nodes of the largest piece: a body's code grows with nodes x feature ops per node, and the
// compiler's time faster than that - pipelines of more than two ops per output row (the experiment
// fruits' seven sieves: four ops with MPI sums and second differences) get pieces of half the size
// (the 115-node body of of_weight(6,2) with four ops: ~200 s on the build host, its 33 / 47 / 62-node
// bodies ~60 s together).
int piece_nodes_knob(const fr_pipeline &pl) {
  return debug_knob("piece_nodes", pl.n_ops_eff > 2 ? fr::kFusedPieceNodes / 2 : fr::kFusedPieceNodes);
}
bool pieces_eligible(const fr_pipeline &pl) {
  const fr::Plan &p = *pl.plan->p;
  // (with more than two feature ops per output row a whole plan of ~100 nodes is as much code as
  // a 200-node plan with two - a minute and more of compiler: in pieces from 65 nodes on)
  const int from = pl.n_ops_eff > 2 ? fr::kFusedPieceNodes / 2 + 1 : fr::kFusedStaticMaxNodes + 1;
  return !p.cos && !p.letter_sum && debug_knob("pieces", 1) != 0 && env_int("FRUITS_HIP_JIT", 1) != 0 &&
         (int)p.nodes.size() >= debug_knob("piece_min", from);
}

// Uploads the tables of every piece type once per plan.  Caller holds p.mu; never inside a capture.
int ensure_piece_tables(fr::Plan &p, fr::PiecedProgram &pp, const char *who) {
  int rc = claim_device(p, who);
  if (rc != FR_OK) return rc;
  for (fr::PieceType &t : pp.types) {
    if (t.d_blob) continue;
    size_t off = 0;
    const size_t o_recs = off;   off = align_up(off + t.recs.size() * sizeof(fr::NodeRec), 64);
    const size_t o_emit = off;   off = align_up(off + t.emit_rows.size() * 4, 64);
    const size_t o_items = off;  off = align_up(off + t.items.size() * 4, 64);
    const size_t o_ub = off;     off = align_up(off + t.unit_begin.size() * 4, 64);
    const size_t o_ur = off;     off = align_up(off + t.unit_row0.size() * 4, 64);
    std::vector<char> host(off + 64, 0);
    std::memcpy(host.data() + o_recs, t.recs.data(), t.recs.size() * sizeof(fr::NodeRec));
    std::memcpy(host.data() + o_emit, t.emit_rows.data(), t.emit_rows.size() * 4);
    std::memcpy(host.data() + o_items, t.items.data(), t.items.size() * 4);
    std::memcpy(host.data() + o_ub, t.unit_begin.data(), t.unit_begin.size() * 4);
    std::memcpy(host.data() + o_ur, t.unit_row0.data(), t.unit_row0.size() * 4);
    void *d = nullptr;
    HIP_TRY(hipMalloc(&d, host.size()));
    hipError_t e = hipMemcpy(d, host.data(), host.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      (void)hipFree(d);
      return hip_fail(e, "hipMemcpy(piece tables)");
    }
    char *b = static_cast<char *>(d);
    t.d_blob = d;
    t.d_recs = reinterpret_cast<const fr::NodeRec *>(b + o_recs);
    t.d_emit_rows = reinterpret_cast<const int32_t *>(b + o_emit);
    t.d_items = reinterpret_cast<const int32_t *>(b + o_items);
    t.d_unit_begin = reinterpret_cast<const int32_t *>(b + o_ub);
    t.d_unit_row0 = reinterpret_cast<const int32_t *>(b + o_ur);
  }
  return FR_OK;
}

// The pipeline's side of a plan in pieces: the op table in walk order (an op's column = its
// row's walk position x features per sum + its place in the block) and the walk position of
// every output row, for the instantiation `key`.  Synchronous uploads: the caller's thread,
// never inside a capture.  FR_OK also when the plan has no cover.
int ensure_pieces_tables(fr_pipeline &pl, const fr::FusedKey &key, const char *who) {
  fr::Plan &p = *pl.plan->p;
  const int max_piece = piece_nodes_knob(pl);
  fr::PiecedProgram *pp;
  {
    std::lock_guard<std::mutex> lock(p.mu);
    pp = &fr::pieced(p, max_piece, debug_knob("piece_unit", 0));
    if (!pp->ok) return FR_OK;
    int rc = ensure_piece_tables(p, *pp, who);
    if (rc != FR_OK) return rc;
  }
  std::lock_guard<std::mutex> lock(pl.jit_mu);
  if (!pl.jit_uniform) return FR_OK;
  fr_pipeline::Pieces &pcs = pl.jit_pieces[key.packed()];
  if (pcs.d_tables) return FR_OK;
  const int K = p.K, npad = pl.n_ops_padded;
  std::vector<fr::FeatOp> walk((size_t)K * npad);
  std::vector<int32_t> walk_of_row(K, 0);
  for (int q = 0; q < K; ++q) {
    const int k = pp->row_of_walk[q];
    walk_of_row[k] = q;
    for (int i = 0; i < npad; ++i) {
      fr::FeatOp o = pl.h_ops[(size_t)k * npad + i];
      if (i < pl.n_ops_eff) o.col = q * pl.per_sum + (o.col - k * pl.per_sum);
      walk[(size_t)q * npad + i] = o;
    }
  }
  const size_t ops_bytes = align_up(walk.size() * sizeof(fr::FeatOp), 256);
  void *d = nullptr;
  HIP_TRY(hipMalloc(&d, ops_bytes + (size_t)K * 4));
  hipError_t e = hipMemcpy(d, walk.data(), walk.size() * sizeof(fr::FeatOp), hipMemcpyHostToDevice);
  if (e == hipSuccess)
    e = hipMemcpy(static_cast<char *>(d) + ops_bytes, walk_of_row.data(), (size_t)K * 4, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(d);
    return hip_fail(e, "hipMemcpy(ops in walk order)");
  }
  pcs.max_piece = max_piece;
  pcs.device = current_device_id();
  pcs.d_tables = d;
  pcs.d_ops_walk = static_cast<const fr::FeatOp *>(d);
  pcs.d_walk_of_row = reinterpret_cast<const int32_t *>(static_cast<char *>(d) + ops_bytes);
  return FR_OK;
}

int piece_level_variant(int levels) { return levels <= 2 ? 2 : (levels <= 4 ? 4 : (levels <= 6 ? 6 : 8)); }

// Compiles (hipRTC, one helper thread per piece type; disk cache) and loads the kernels of the
// plan's piece types for the instantiation `key`; all of them or none.
void ensure_fused_pieces(fr_pipeline &pl, const fr::FusedKey &key, bool cache_only) {
  fr::Plan &p = *pl.plan->p;
  const uint32_t id = key.packed();
  fr::FusedOps ops;
  uint64_t gen;
  int max_piece;
  const int n_ops_eff = pl.n_ops_eff;
  const bool has_mpi = !pl.mpi_cols.empty();
  {
    std::lock_guard<std::mutex> lock(pl.jit_mu);
    auto it = pl.jit_pieces.find(id);
    if (!pl.jit_uniform || it == pl.jit_pieces.end() || !it->second.d_tables || !it->second.progs.empty() ||
        pl.jit_pieces_tried.count(id))
      return;
    pl.jit_pieces_tried.insert(id);
    ops = pl.jit_ops;
    gen = pl.jit_gen;
    max_piece = it->second.max_piece;
  }
  const fr::PiecedProgram *pp;
  {
    std::lock_guard<std::mutex> lock(p.mu);
    pp = &fr::pieced(p, max_piece);   // (map nodes are stable; built and uploaded by ensure_pieces_tables)
  }
  const int n_types = (int)pp->types.size();
  std::vector<fr::JitProgram> progs(n_types);
  std::vector<std::string> errs(n_types);
  std::vector<char> good(n_types, 0), type_fits(n_types, 0);
  const int dev = current_device_id();
  std::atomic<int> next{0};
  auto worker = [&] {
    (void)hipSetDevice(dev);   // (the current device is per thread)
    for (int t = next++; t < n_types; t = next++) {
      fr::FusedPlan fp;
      fp.w = pp->types[t].body_w;
      fp.piece = true;
      fr::FusedKey k = key;
      k.LV = piece_level_variant(pp->types[t].levels);
      // (whether the largest unit's features fit the window is known here: no flush test then)
      fr::FusedOps type_ops = ops;
      bool fits = false;
      (void)piece_window(p, pp->types[t], pl.T, ops.cps, n_ops_eff, has_mpi, fits);
      type_ops.window_fits = fits;
      type_fits[t] = fits ? 1 : 0;
      good[t] = fr::jit_fused(type_ops, k, progs[t], errs[t], &fp, cache_only) ? 1 : 0;
    }
  };
  const int hw = (int)std::thread::hardware_concurrency();
  const int n_threads = cache_only ? 1 : std::max(1, std::min({n_types, hw > 0 ? hw : 4, 16}));
  std::vector<std::thread> pool;
  for (int i = 1; i < n_threads; ++i) pool.emplace_back(worker);
  worker();
  for (std::thread &th : pool) th.join();
  bool all = true, missing = false;
  for (int t = 0; t < n_types; ++t) {
    if (!good[t]) all = false;
    if (!good[t] && cache_only && fr::jit_not_cached(errs[t])) missing = true;
  }
  std::lock_guard<std::mutex> lock(pl.jit_mu);
  auto it = pl.jit_pieces.find(id);
  if (!all || gen != pl.jit_gen || it == pl.jit_pieces.end()) {
    for (int t = 0; t < n_types; ++t)
      if (good[t]) fr::jit_unload(progs[t]);
    // (a miss of the cache-only look leaves no trace: a later call compiles)
    if (!all && missing && gen == pl.jit_gen) pl.jit_pieces_tried.erase(id);
    else if (!all)
      for (int t = 0; t < n_types; ++t)
        if (!good[t]) {
          pl.jit_failed[id | 0x80000000u] = errs[t];
          break;
        }
    return;
  }
  it->second.progs = std::move(progs);
  it->second.fits = std::move(type_fits);
}

// The host half of fr_pipeline_set_quantiles: the table of feature ops (and the NPI / MPI pairs
// that share a population), nothing on the device.
void build_pipeline_ops(fr_pipeline_t *pl, const double *h_quant, std::vector<fr::FeatOp> &ops,
                               std::vector<int32_t> &pairs) {
  const int K = pl->rows();
  ops.assign((size_t)K * pl->n_ops_padded, fr::FeatOp{});
  // An NPI feature whose band, cut and differencing order equal an MPI feature's is that
  // MPI op's population (experiments/fruit_reduced.py pairs NPI and MPI sieves with the
  // same arguments, fitted on the same values): such NPI ops are dropped from the walk
  // and filled in from the population table by mpi_finalize_kernel.  Only when the same
  // pairs match in every row (the finalize kernel works on column patterns).
  pairs.clear();
  for (int pass = 0; pass < 2; ++pass) {
    const bool merge = pass == 0;
    bool uniform = true;
    int n_ops_eff = 0;
    for (int k = 0; k < K && uniform; ++k) {
      std::vector<fr::FeatOp> row;
      for (const PipeSieve &sv : pl->sieves) {
        const int C = (int)sv.cuts.size() - 1;
        if (sv.kind == FR_SIEVE_END) {
          for (int j = 0; j < C; ++j) {
            if (sv.series_cuts) {   // the kernel reads cut_row[slot] - 1 (and wraps -1)
              row.push_back(fr::FeatOp{FR_SIEVE_END | (1 << 16), k * pl->per_sum + sv.col + j,
                                       sv.cuts[j + 1], 0, 0.0, 0.0});
              continue;
            }
            int idx = sv.cuts[j + 1] - 1;
            if (idx < 0) idx += (int)pl->T;  // numpy's wrap of index -1 (segment.py:213-218)
            row.push_back(fr::FeatOp{FR_SIEVE_END | (1 << 20), k * pl->per_sum + sv.col + j, idx, 0, 0.0, 0.0});
          }
          continue;
        }
        const double *q = h_quant + (size_t)k * pl->q_stride + sv.q_off;
        if (sv.kind == FR_SIEVE_PPV || sv.kind == FR_SIEVE_CPV) {
          // one op per feature: v >= q_b, or with segments q_b <= v < q_(b+1) - the thresholds as
          // fitted, not sorted (an empty band stays empty); the walk leaves the count
          const int nf = sv.Q1 - (sv.segments ? 1 : 0);
          // (per-series cuts: `hi` is the slot that holds the series' own length)
          for (int b = 0; b < nf; ++b)
            row.push_back(fr::FeatOp{sv.kind | (sv.segments ? fr::OPF_SEGMENTS : 0) |
                                         (sv.series_cuts ? (1 << 16) : 0),
                                     k * pl->per_sum + sv.col + b, sv.cuts[0], sv.cuts[1], q[b],
                                     sv.segments ? q[b + 1] : std::numeric_limits<double>::infinity()});
          continue;
        }
        for (int j = 0; j < C; ++j)
          for (int b = 0; b + 1 < sv.Q1; ++b) {
            // the common shapes get a short path in the fused walk (walk_fused.h, OPF_SHAPE_*):
            // a counting band over the whole series, of the values or their first differences,
            // with or without an upper threshold
            int32_t flags = sv.series_cuts ? (1 << 16) : 0;
            if (sv.kind == FR_SIEVE_NPI && !sv.series_cuts && sv.cuts[j] <= 0 &&
                sv.cuts[j + 1] >= pl->T && (sv.inc == 0 || sv.inc == 1)) {
              const bool no_hi = q[b + 1] == std::numeric_limits<double>::infinity();
              flags |= ((no_hi ? 2 : 4) | sv.inc) << 20;
            }
            row.push_back(fr::FeatOp{sv.kind | ((sv.inc & 0xff) << 8) | flags,
                                     k * pl->per_sum + sv.col + j * (sv.Q1 - 1) + b, sv.cuts[j],
                                     sv.cuts[j + 1], q[b], q[b + 1]});
          }
      }
      std::vector<int32_t> row_pairs;
      std::vector<char> drop(row.size(), 0), used(row.size(), 0);
      if (merge && !pl->mpi_cols.empty()) {
        for (size_t i = 0; i < row.size(); ++i) {
          if ((row[i].kind_inc & 0xff) != FR_SIEVE_NPI) continue;
          for (size_t m = 0; m < row.size(); ++m) {
            if ((row[m].kind_inc & 0xff) != FR_SIEVE_MPI || used[m]) continue;
            // (same differencing order and kind of cuts; the shape bits above are the walk's)
            if ((((row[m].kind_inc ^ row[i].kind_inc) >> 8) & 0x1ff) == 0 && row[m].lo == row[i].lo &&
                row[m].hi == row[i].hi && std::memcmp(&row[m].qlo, &row[i].qlo, 8) == 0 &&
                std::memcmp(&row[m].qhi, &row[i].qhi, 8) == 0) {
              drop[i] = used[m] = 1;
              row_pairs.push_back(row[i].col - k * pl->per_sum);
              row_pairs.push_back(row[m].col - k * pl->per_sum);
              break;
            }
          }
        }
      }
      if (k == 0) pairs = row_pairs;
      else if (row_pairs != pairs) uniform = false;
      fr::FeatOp *o = ops.data() + (size_t)k * pl->n_ops_padded;
      int i = 0;
      for (size_t j = 0; j < row.size(); ++j)
        if (!drop[j]) o[i++] = row[j];
      n_ops_eff = std::max(n_ops_eff, i);
      for (; i < pl->n_ops_padded; ++i)  // padding op: an END that never matches a chunk
        o[i] = fr::FeatOp{FR_SIEVE_END, 0, -(1 << 30), 0, 0.0, 0.0};
    }
    pl->n_ops_eff = n_ops_eff;
    if (uniform) break;
    pairs.clear();  // rows disagree: second pass without merging
  }
}

// What a run-time compiled kernel takes as immediates: per op kind | differencing order | shape
// and the cuts - the same for every output row (the shape only if every row's thresholds agree
// on it: an infinite threshold in one row alone keeps the generic band).  Caller holds jit_mu.
void set_pipeline_jit_ops(fr_pipeline_t *pl, const std::vector<fr::FeatOp> &ops) {
  const int K = pl->rows();
  pl->jit_ops = fr::FusedOps{};
  pl->jit_ops.n_padded = pl->n_ops_padded;
  pl->jit_ops.full_chunks = pl->T % fr::walk_chunk_elems(pl->T) == 0;
  for (const PipeSieve &sv : pl->sieves) {   // (a slot pair per differencing order >= 3 and per
    if (sv.kind == FR_SIEVE_END) continue;    // cumulation of a row: walk_device.h, fop)
    if (sv.inc > 2) pl->jit_ops.cps = std::max(pl->jit_ops.cps, 3 + 2 * (sv.inc - 2));
    if (sv.inc < 0) pl->jit_ops.cps = std::max(pl->jit_ops.cps, 15 + 2 * (-sv.inc));
  }
  // CPV: the value of the row in front of a time chunk, one slot behind all the others (the
  // LAST of the node's slots: walk_fused.h, WindowEpilogue)
  for (const PipeSieve &sv : pl->sieves)
    if (sv.kind == FR_SIEVE_CPV) {
      pl->jit_ops.cps += 1;
      break;
    }
  pl->jit_uniform = K > 0 && pl->n_ops_eff > 0 && pl->cut_slots_needed == 0;
  for (int i = 0; i < pl->n_ops_eff && pl->jit_uniform; ++i) {
    int32_t w0 = ops[i].kind_inc;
    for (int k = 1; k < K; ++k) {
      const fr::FeatOp &o = ops[(size_t)k * pl->n_ops_padded + i];
      if (o.kind_inc != w0) {
        if (((o.kind_inc ^ w0) & ~(7 << 20)) != 0) pl->jit_uniform = false;
        w0 &= ~(7 << 20);
      }
      if (o.lo != ops[i].lo || o.hi != ops[i].hi) pl->jit_uniform = false;
    }
    pl->jit_ops.w0.push_back(w0);
    pl->jit_ops.lo.push_back(ops[i].lo);
    pl->jit_ops.hi.push_back(ops[i].hi);
  }
}

// The kernel instantiation a fused launch of this pipeline over N series takes, or false when
// it has none of its own (CosWISS, wave-per-series kernels, letter sums, nothing fits).
bool fused_instance_of(fr_pipeline_t *pl, int64_t N, int32_t groups, fr::FusedKey &key,
                              const fr::WalkKnobs &k) {
  fr::Plan &p = *pl->plan->p;
  if (p.cos || N <= 0 || k.hip_jit == 0 || p.letter_sum) return false;
  bool total_inc = false;
  for (const PipeSieve &sv : pl->sieves)
    if (sv.kind != FR_SIEVE_END && sv.inc >= 1) total_inc = true;
  const fr::LaunchShape shape = fr::launch_shape(p, N, pl->T, groups, k);
  if (fr::walk_is_packed(shape, total_inc && p.weighting == FR_W_TOTAL) || !shape.fits) return false;
  key = fused_key_for(p, pl->T, total_inc, pl->jit_ops.cps > 3);
  return true;
}

int pipeline_prepare(fr_pipeline_t *pl, int64_t N, int32_t groups, bool cache_only,
                            const fr::WalkKnobs &k) {
  if (!pl || !pl->plan || !pl->plan->p || N < 0)
    return fail(FR_E_ARG, "fr_pipeline_prepare: bad argument");
  if (!pl->have_quantiles)
    return fail(FR_E_ARG, "fr_pipeline_prepare: call fr_pipeline_set_quantiles first");
  fr::Plan &p = *pl->plan->p;
  if (!pl->argmax_words.empty())   // (the plan runs as a materialising walk, the sieves in a kernel of the library)
    return prepare_plan(p, N, pl->T, groups, false, "fr_pipeline_prepare", k);
  int rc = prepare_plan(p, N, pl->T, groups, true, "fr_pipeline_prepare", k);
  if (rc != FR_OK) return rc;
  // The pipeline's own kernel: the fused walk with the sieves as compile-time constants (hipRTC,
  // 1-2 s once per pipeline shape, cached on disk); a failure is not the caller's - the generic
  // kernel runs the pipeline.  Not for the wave-per-series kernels (T <= 384) and CosWISS.
  fr::FusedKey key;
  if (fused_instance_of(pl, N, groups, key, k)) {
    // (a large plan runs in pieces: their tables go up here, on the caller's thread)
    if (pieces_eligible(*pl)) {
      rc = ensure_pieces_tables(*pl, key, "fr_pipeline_prepare");
      if (rc != FR_OK) return rc;
    }
    ensure_fused_jit(*pl, key, cache_only);
  }
  return FR_OK;
}

int pipeline_compile_plan(fr_pipeline_t *pl, int64_t N, int32_t groups, bool cache_only,
                                 const fr::WalkKnobs &k) {
  if (!pl || !pl->plan || !pl->plan->p || N < 0)
    return fail(FR_E_ARG, "fr_pipeline_compile_plan: bad argument");
  if (!pl->have_quantiles)
    return fail(FR_E_ARG, "fr_pipeline_compile_plan: call fr_pipeline_set_quantiles first");
  fr::Plan &p = *pl->plan->p;
  fr::FusedKey key;
  if (!fused_instance_of(pl, N, groups, key, k) || debug_knob("fused_static", 1) == 0) return FR_OK;
  // a large plan: in pieces, every piece type straight-line code in a kernel of its own; the
  // node shapes below only where the plan has no such cover
  if (pieces_eligible(*pl)) {
    if (!cache_only) {
      int rc = ensure_pieces_tables(*pl, key, "fr_pipeline_compile_plan");
      if (rc != FR_OK) return rc;
    }
    ensure_fused_pieces(*pl, key, cache_only);
    std::lock_guard<std::mutex> lock(pl->jit_mu);
    auto it = pl->jit_pieces.find(key.packed());
    if (it != pl->jit_pieces.end() && !it->second.progs.empty()) return FR_OK;
    if (cache_only) return FR_OK;   // (not in the cache: the loop kernels' cached variants are not looked up either)
  }
  // for the group program a launch over N series will pick (another group count at run time
  // simply takes the kernel of fr_pipeline_prepare)
  fr::FusedPlan fp;
  {
    std::lock_guard<std::mutex> lock(p.mu);
    const int G = fr::choose_walk_launch(p, walk_facts(p, N, pl->T, groups, true, key.TI != 0, true, k), k).G;
    const fr::GroupedProgram &gp = fr::grouped(p, G);
    if ((int)p.nodes.size() <= fr::kFusedStaticMaxNodes) {
      // a small plan: the records themselves (straight-line code)
      fp.w.reserve(gp.recs.size() * 16);
      for (const fr::NodeRec &r : gp.recs) fp.w.insert(fp.w.end(), r.w, r.w + 16);
      fp.group_begin.assign(gp.group_begin.begin(), gp.group_begin.begin() + gp.groups);
    } else {
      // a large one: its most frequent node shapes (the loop stays, the bodies are compiled
      // per shape; the rest takes the generic body)
      const size_t n = std::min<size_t>(gp.shapes.size(), fr::kFusedShapes);
      fp.shapes.assign(gp.shapes.begin(), gp.shapes.begin() + n);
      fp.n_groups = gp.groups;
    }
  }
  ensure_fused_static(*pl, key, fp, cache_only);
  return FR_OK;
}

}  // namespace
}  // namespace fr::capi

using namespace fr::capi;

extern "C" {

fr_pipeline_t *fr_pipeline_create(fr_plan_t *plan, int32_t n_sieves, const int32_t *kinds,
                                  const int32_t *incs, const int32_t *C1, const int32_t *Q1,
                                  const int64_t *cuts, int64_t T) {
  if (!plan || !plan->p || n_sieves < 1 || !kinds || !incs || !C1 || !Q1 || !cuts || T < 1) {
    fail(FR_E_ARG, "fr_pipeline_create: bad argument");
    return nullptr;
  }
  fr_pipeline_t *pl = new fr_pipeline_t;
  pl->plan = plan;
  pl->T = T;
  int32_t col = 0, qoff = 0, n_ops = 0;
  for (int i = 0; i < n_sieves; ++i) {
    PipeSieve sv;
    sv.kind = kinds[i] & 0xff;
    sv.series_cuts = (kinds[i] & FR_SIEVE_SERIES_CUTS) != 0;
    const bool implicit = sv.kind == FR_SIEVE_PPV || sv.kind == FR_SIEVE_CPV;
    sv.segments = implicit && (kinds[i] & FR_SIEVE_SEGMENTS) != 0;
    sv.inc = incs[i];
    sv.Q1 = Q1[i];
    const int c1 = C1[i];
    std::string bad;
    int code = FR_E_ARG;
    if (sv.kind < 0 || (sv.kind > FR_SIEVE_CUR && !implicit) || c1 < 2 ||
        ((kinds[i] & FR_SIEVE_SEGMENTS) && !implicit))
      bad = "bad sieve " + std::to_string(i);
    else if (implicit) {
      // PPV / CPV (fruits/sieving/implicit.py): the whole row itself, thresholds in the sieve's order
      // (with FR_SIEVE_SERIES_CUTS: of the series' first cut_row[slot 1] elements - its own length)
      if (c1 != 2 || sv.inc != 0) bad = "PPV / CPV look at the whole row itself (cuts {0, T}, inc 0)";
      else if (sv.Q1 < (sv.segments ? 2 : 1)) bad = "PPV / CPV need >= 1 thresholds, >= 2 with segments";
      else if (sv.Q1 - (sv.segments ? 1 : 0) > fr::kImplicitMaxFeatures) {
        bad = "at most 256 features per PPV / CPV sieve";
        code = FR_E_LIMIT;
      }
    }
    else if (sv.kind == FR_SIEVE_LPI) {
      // (a run crosses lanes, waves and time chunks: the window has no carry for it)
      bad = "LPI is not fused";
      code = FR_E_LIMIT;
    }
    if (bad.empty() && sv.kind != FR_SIEVE_END && !implicit) {
      if (sv.Q1 < 2) bad = "a band sieve needs >= 2 thresholds";
      else if (sv.inc < -8 || sv.inc > 8) {
        bad = "the fused epilogue supports inc -8 to 8";
        code = FR_E_LIMIT;
      }
    }
    if (!bad.empty()) {
      fail(code, "fr_pipeline_create: " + bad);
      delete pl;
      return nullptr;
    }
    for (int j = 0; j < c1 && sv.series_cuts; ++j) {
      // the "cuts" of such a sieve are slots of the per-series table
      const int64_t c = *cuts++;
      if (c < 0 || c > 0xffff) {
        fail(FR_E_ARG, "fr_pipeline_create: bad cut slot " + std::to_string(c));
        delete pl;
        return nullptr;
      }
      sv.cuts.push_back((int32_t)c);
      pl->cut_slots_needed = std::max(pl->cut_slots_needed, (int32_t)c + 1);
    }
    for (int j = 0; j < c1 && !sv.series_cuts; ++j) {
      const int64_t c = *cuts++;
      // END reads X[:, c - 1] (index -1 wraps like numpy): the reference raises IndexError
      // outside [-T, T-1] (np.take_along_axis, fruits/sieving/segment.py:213-218)
      if (sv.kind == FR_SIEVE_END && j > 0 && (c - 1 < -T || c - 1 > T - 1)) {
        fail(FR_E_INDEX, "fr_pipeline_create: END cut " + std::to_string(c) +
                             " is out of bounds for series of length " + std::to_string(T));
        delete pl;
        return nullptr;
      }
      sv.cuts.push_back((int32_t)(c < 0 ? 0 : (c > T ? T : c)));
    }
    const int nf = sv.kind == FR_SIEVE_END ? c1 - 1
                   : implicit ? sv.Q1 - (sv.segments ? 1 : 0) : (c1 - 1) * (sv.Q1 - 1);
    if (implicit) {   // (the cuts given are not looked at: the whole series - or they are slots)
      if (sv.series_cuts) pl->implicit_series_cuts = true;
      else sv.cuts = {0, (int32_t)(T > 0x7fffffffLL ? 0x7fffffff : T)};
      for (int f = 0; f < nf; ++f) pl->implicit_cols.push_back(sv.kind == FR_SIEVE_CPV ? ~(col + f) : col + f);
    }
    sv.col = col;
    sv.q_off = qoff;
    // (XPI is MPI of the positions: sum and population, divided by mpi_finalize_kernel)
    if (sv.kind == FR_SIEVE_MPI || sv.kind == FR_SIEVE_XPI)
      for (int f = 0; f < nf; ++f) pl->mpi_cols.push_back(col + f);
    // (MAX / MIN leave band keys, walk_types.h: band_key_finalize_kernel makes them values)
    if (sv.kind == FR_SIEVE_MAX || sv.kind == FR_SIEVE_MIN)
      for (int f = 0; f < nf; ++f) pl->key_cols.push_back(sv.kind == FR_SIEVE_MIN ? ~(col + f) : col + f);
    if (sv.kind != FR_SIEVE_END) qoff += sv.Q1;
    col += nf;
    n_ops += nf;
    pl->sieves.push_back(sv);
  }
  pl->per_sum = col;
  pl->q_stride = qoff > 0 ? qoff : 1;
  pl->n_ops = n_ops;
  pl->n_ops_padded = (n_ops + 1) / 2 * 2;
  return pl;
}

void fr_pipeline_destroy(fr_pipeline_t *pl) {
  if (!pl) return;
  {
    // (launches of the pipeline's own kernels may still run, a compilation may still be about to
    // store its result: wait for the device, and take the lock the compilations store under)
    std::lock_guard<std::mutex> lock(pl->jit_mu);
    ++pl->jit_gen;
    if (!pl->jit.empty() || !pl->jit_static.empty() || !pl->jit_pieces.empty()) (void)hipDeviceSynchronize();
  }
  if (pl->d_ops) (void)hipFree(pl->d_ops);
  if (pl->d_mpi_cols) (void)hipFree(pl->d_mpi_cols);
  if (pl->d_key_cols) (void)hipFree(pl->d_key_cols);
  if (pl->d_implicit_cols) (void)hipFree(pl->d_implicit_cols);
  if (pl->d_npi_pairs) (void)hipFree(pl->d_npi_pairs);
  if (pl->d_prep) (void)hipFree(pl->d_prep);
  if (pl->d_argmax_words) (void)hipFree(pl->d_argmax_words);
  for (auto &kv : pl->jit) fr::jit_unload(kv.second);
  for (auto &kv : pl->jit_static) fr::jit_unload(kv.second);
  pl->drop_pieces();
  delete pl;
}

int64_t fr_pipeline_info(const fr_pipeline_t *pl, int32_t what) {
  if (!pl) return fail(FR_E_ARG, "fr_pipeline_info: null pipeline");
  switch (what) {
    case 0: return pl->per_sum;
    case 1: return pl->q_stride;
    case 2: return (int64_t)pl->per_sum * pl->rows();
    case 3: {                                    // run-time compiled kernels loaded
      fr_pipeline *m = const_cast<fr_pipeline *>(pl);
      std::lock_guard<std::mutex> lock(m->jit_mu);
      return (int64_t)(m->jit.size() + m->jit_static.size());
    }
    case 4: {                                    // ... of them with the plan as straight-line code
      fr_pipeline *m = const_cast<fr_pipeline *>(pl);
      std::lock_guard<std::mutex> lock(m->jit_mu);
      return (int64_t)m->jit_static.size();
    }
    case 5: {                                    // kernels of piece types loaded (a plan in pieces)
      fr_pipeline *m = const_cast<fr_pipeline *>(pl);
      std::lock_guard<std::mutex> lock(m->jit_mu);
      int64_t n = 0;
      for (const auto &kv : m->jit_pieces) n += (int64_t)kv.second.progs.size();
      return n;
    }
    default: return fail(FR_E_ARG, "fr_pipeline_info: unknown selector");
  }
}

int fr_pipeline_set_argmax(fr_pipeline_t *pl, int32_t n_words, const int32_t *lengths) {
  if (!pl || !pl->plan || !pl->plan->p || n_words < 1 || !lengths)
    return fail(FR_E_ARG, "fr_pipeline_set_argmax: bad argument");
  const fr::Plan &p = *pl->plan->p;
  if (!p.letter_sum || p.semiring != fr::kSemiArctic || p.cos)
    return fail(FR_E_ARG, "fr_pipeline_set_argmax: the plan must be an Arctic letter-sum plan "
                          "(FR_PLAN_ARCTIC | FR_PLAN_LETTER_SUM) with every prefix of every word as a row");
  if (pl->have_quantiles)
    return fail(FR_E_ARG, "fr_pipeline_set_argmax: call it before fr_pipeline_set_quantiles");
  std::vector<int32_t> words;
  int64_t v0 = 0, o0 = 0;
  int max_len = 0;
  for (int w = 0; w < n_words; ++w) {
    const int L = lengths[w];
    if (L < 1 || L > 63) return fail(FR_E_LIMIT, "fr_pipeline_set_argmax: words of 1 to 63 letters");
    words.insert(words.end(), {(int32_t)v0, L, (int32_t)o0, 0});
    v0 += L;
    o0 += L + L * (L + 1) / 2;
    max_len = std::max(max_len, L);
  }
  if (v0 != p.K)
    return fail(FR_E_ARG, "fr_pipeline_set_argmax: the plan has " + std::to_string(p.K) +
                              " rows, the words' prefixes are " + std::to_string(v0));
  if (o0 > 0x7fffffffLL / std::max(1, pl->per_sum) || n_words > 65535)
    return fail(FR_E_LIMIT, "fr_pipeline_set_argmax: too many rows");
  for (const PipeSieve &sv : pl->sieves) {
    if (sv.kind != FR_SIEVE_END && (sv.inc < 0 || sv.inc > 2))
      return fail(FR_E_LIMIT, "fr_pipeline_set_argmax: differencing orders 0 to 2");
    if (sv.kind > FR_SIEVE_END)
      return fail(FR_E_LIMIT, "fr_pipeline_set_argmax: NPI, MPI and END only");
  }
  if (pl->T > 65535 || fr::argmax_sieve_lds(pl->T, max_len) > fr::kArgmaxSieveLds)
    return fail(FR_E_LIMIT, "fr_pipeline_set_argmax: a row of maxima and the positions of a word's "
                            "prefixes must fit a workgroup's LDS");
  if (pl->d_argmax_words) (void)hipFree(pl->d_argmax_words);
  pl->d_argmax_words = nullptr;
  HIP_TRY(hipMalloc(&pl->d_argmax_words, words.size() * 4));
  HIP_TRY(hipMemcpy(pl->d_argmax_words, words.data(), words.size() * 4, hipMemcpyHostToDevice));
  pl->argmax_words = words;
  pl->argmax_rows = (int32_t)o0;
  pl->argmax_max_len = max_len;
  return FR_OK;
}

int fr_pipeline_set_quantiles(fr_pipeline_t *pl, const double *h_quant) {
  if (!pl || !h_quant) return fail(FR_E_ARG, "fr_pipeline_set_quantiles: bad argument");
  std::vector<fr::FeatOp> ops;
  std::vector<int32_t> pairs;
  build_pipeline_ops(pl, h_quant, ops, pairs);
  if (pairs != pl->npi_pairs || (!pairs.empty() && !pl->d_npi_pairs)) {
    if (pl->d_npi_pairs) (void)hipFree(pl->d_npi_pairs);
    pl->d_npi_pairs = nullptr;
    pl->npi_pairs = pairs;
    if (!pairs.empty()) {
      HIP_TRY(hipMalloc(&pl->d_npi_pairs, pairs.size() * 4));
      HIP_TRY(hipMemcpy(pl->d_npi_pairs, pairs.data(), pairs.size() * 4, hipMemcpyHostToDevice));
    }
  }
  // (new thresholds: d_ops is rewritten in place and the kernels compiled for the old ops go - once
  // the launches that may still be reading or running them are done: fr_pipeline_run returns
  // without a synchronisation, and the hipMemcpy below does not wait for a non-blocking stream.
  // Whatever the pipeline holds: the generic kernel reads d_ops too.  A refit is rare and has
  // waited for a selection already.)
  std::lock_guard<std::mutex> jit_lock(pl->jit_mu);
  (void)hipDeviceSynchronize();
  ++pl->jit_gen;
  for (auto &kv : pl->jit) fr::jit_unload(kv.second);
  for (auto &kv : pl->jit_static) fr::jit_unload(kv.second);
  pl->jit.clear();
  pl->jit_static.clear();
  pl->jit_static_tried.clear();
  pl->jit_failed.clear();
  pl->drop_pieces();
  set_pipeline_jit_ops(pl, ops);
  const size_t bytes = ops.size() * sizeof(fr::FeatOp);
  pl->h_ops = ops;
  if (!pl->d_ops && bytes) HIP_TRY(hipMalloc(&pl->d_ops, bytes));
  if (bytes) HIP_TRY(hipMemcpy(pl->d_ops, ops.data(), bytes, hipMemcpyHostToDevice));
  if (!pl->mpi_cols.empty() && !pl->d_mpi_cols) {
    HIP_TRY(hipMalloc(&pl->d_mpi_cols, pl->mpi_cols.size() * 4));
    HIP_TRY(hipMemcpy(pl->d_mpi_cols, pl->mpi_cols.data(), pl->mpi_cols.size() * 4,
                      hipMemcpyHostToDevice));
  }
  if (!pl->key_cols.empty() && !pl->d_key_cols) {
    HIP_TRY(hipMalloc(&pl->d_key_cols, pl->key_cols.size() * 4));
    HIP_TRY(hipMemcpy(pl->d_key_cols, pl->key_cols.data(), pl->key_cols.size() * 4,
                      hipMemcpyHostToDevice));
  }
  if (!pl->implicit_cols.empty() && !pl->d_implicit_cols) {
    HIP_TRY(hipMalloc(&pl->d_implicit_cols, pl->implicit_cols.size() * 4));
    HIP_TRY(hipMemcpy(pl->d_implicit_cols, pl->implicit_cols.data(), pl->implicit_cols.size() * 4,
                      hipMemcpyHostToDevice));
  }
  pl->have_quantiles = true;
  return FR_OK;
}

int64_t fr_pipeline_workspace_bytes(const fr_pipeline_t *pl, int64_t N, int64_t lookup_rows) {
  if (!pl || N < 0) return fail(FR_E_ARG, "fr_pipeline_workspace_bytes: bad argument");
  const fr::Plan &p = *pl->plan->p;
  size_t b = align_up(work_layout(p, N, pl->T, p.weighting ? lookup_rows : 0).total(), 256);
  if (!pl->mpi_cols.empty()) b += align_up((size_t)N * pl->per_sum * pl->rows() * 8, 256);
  // (argmax: the running maxima of the plan's rows are materialised, the argmax rows are not)
  if (!pl->argmax_words.empty()) b += align_up((size_t)p.K * N * pl->T * 8, 256);
  if (pl->prep_n > 0 && pl->prep_std != 0) b += align_up((size_t)N * pl->prep_n * 16, 256);
  // (a plan in pieces leaves its features in walk order first)
  if (pieces_eligible(*pl)) b += align_up((size_t)N * pl->per_sum * p.K * 8, 256);
  return (int64_t)b;
}

int fr_pipeline_set_preparation(fr_pipeline_t *pl, int32_t D, int32_t inc_lag, int32_t as_new,
                                int32_t standardize, double std_eps) {
  if (!pl || !pl->plan || !pl->plan->p || D < 1 || inc_lag < 0 || standardize < 0 ||
      standardize > 2 || (as_new && inc_lag < 1))
    return fail(FR_E_ARG, "fr_pipeline_set_preparation: bad argument");
  const fr::Plan &p = *pl->plan->p;
  if (pl->d_prep) (void)hipFree(pl->d_prep);
  pl->d_prep = nullptr;
  pl->prep_D = pl->prep_n = pl->prep_std = 0;
  if (inc_lag == 0 && standardize == 0) return FR_OK;   // nothing to fuse
  if (!pl->argmax_words.empty())
    return fail(FR_E_LIMIT, "fr_pipeline_set_preparation: an argmax pipeline materialises the running "
                            "maxima from the prepared input");
  // (every fused kernel forms the prepared rows itself since round 4: the cooperative walk in its
  // staging, the wave-per-series kernels in theirs, CosWISS where it reads a letter's rows - all
  // but a CosWISS with the randomised ffn, whose units read transformed copies of the input)
  if (p.cos && p.cos->x_unit_stride != 0)
    return fail(FR_E_LIMIT, "fr_pipeline_set_preparation: a CosWISS with per-unit inputs (ffn) reads "
                            "transformed copies of the prepared input");
  const int n_prep = as_new ? 2 * D : D;
  std::vector<int32_t> tab((size_t)n_prep * 4, 0);
  for (int d = 0; d < n_prep; ++d) {
    const bool inc_row = as_new ? d >= D : inc_lag > 0;
    tab[4 * d] = as_new ? d % D : d;
    tab[4 * d + 1] = inc_row ? inc_lag : 0;
    tab[4 * d + 2] = standardize != 0 ? 1 : 0;
  }
  HIP_TRY(hipMalloc(&pl->d_prep, tab.size() * 4));
  hipError_t e = hipMemcpy(pl->d_prep, tab.data(), tab.size() * 4, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(pl->d_prep);
    pl->d_prep = nullptr;
    return hip_fail(e, "hipMemcpy(preparation table)");
  }
  pl->prep_D = D;
  pl->prep_n = n_prep;
  pl->prep_std = standardize;
  pl->prep_eps = std_eps;
  return FR_OK;
}

int fr_pipeline_prepare(fr_pipeline_t *pl, int64_t N, int32_t groups) {
  return pipeline_prepare(pl, N, groups, false, read_walk_knobs());
}

int fr_pipeline_compile_plan(fr_pipeline_t *pl, int64_t N, int32_t groups) {
  return pipeline_compile_plan(pl, N, groups, false, read_walk_knobs());
}

int fr_pipeline_prepare_cached(fr_pipeline_t *pl, int64_t N, int32_t groups) {
  const fr::WalkKnobs k = read_walk_knobs();
  int rc = pipeline_prepare(pl, N, groups, true, k);
  return rc != FR_OK ? rc : pipeline_compile_plan(pl, N, groups, true, k);
}

int32_t fr_pipeline_bundle(fr_pipeline_t *pl, const double *h_quant, int32_t groups, const char *dir,
                           char *msg, int64_t msg_cap) {
  if (msg && msg_cap > 0) msg[0] = 0;
  if (!pl || !pl->plan || !pl->plan->p || !h_quant || !dir || !*dir)
    return fail(FR_E_ARG, "fr_pipeline_bundle: bad argument");
  fr::Plan &p = *pl->plan->p;
  std::vector<fr::FeatOp> ops;
  std::vector<int32_t> pairs;
  build_pipeline_ops(pl, h_quant, ops, pairs);
  fr::FusedOps jops;
  {
    std::lock_guard<std::mutex> lock(pl->jit_mu);
    set_pipeline_jit_ops(pl, ops);
    if (!pl->jit_uniform) return 0;
    jops = pl->jit_ops;
  }
  fr::FusedKey key;
  if (!fused_instance_of(pl, 1 << 20, groups, key, read_walk_knobs())) return 0;
  std::vector<std::string> errs;
  std::atomic<int> done{0};
  std::mutex err_mu;
  auto one = [&](const fr::FusedOps &o, const fr::FusedKey &k, const fr::FusedPlan *fp) {
    std::string err;
    if (fr::jit_fused_into(o, k, fp, dir, err)) {
      ++done;
    } else {
      std::lock_guard<std::mutex> lock(err_mu);
      errs.push_back(err);
    }
  };
  if (pieces_eligible(*pl)) {                  // a large plan: a kernel per piece type
    const fr::PiecedProgram *pp;
    {
      std::lock_guard<std::mutex> lock(p.mu);
      pp = &fr::pieced(p, piece_nodes_knob(*pl), debug_knob("piece_unit", 0));
    }
    const int n_types = pp->ok ? (int)pp->types.size() : 0;
    // the largest bodies first (the compiler's time grows faster than a body); job -1: the kernel
    // with the sieves as immediates alone (the plan from its records)
    std::vector<int> order{-1};
    for (int t = 0; t < n_types; ++t) order.push_back(t);
    std::stable_sort(order.begin() + 1, order.end(), [&](int x, int y) {
      return pp->types[x].body_nodes > pp->types[y].body_nodes;
    });
    std::atomic<int> next{0};
    auto worker = [&] {
      for (int i = next++; i < (int)order.size(); i = next++) {
        const int t = order[i];
        if (t < 0) {
          one(jops, key, nullptr);
          continue;
        }
        fr::FusedPlan fp;
        fp.w = pp->types[t].body_w;
        fp.piece = true;
        fr::FusedKey k = key;
        k.LV = piece_level_variant(pp->types[t].levels);
        fr::FusedOps type_ops = jops;
        bool fits = false;
        (void)piece_window(p, pp->types[t], pl->T, jops.cps, pl->n_ops_eff, !pl->mpi_cols.empty(), fits);
        type_ops.window_fits = fits;
        one(type_ops, k, &fp);
      }
    };
    const int n_threads = std::max(1, std::min((int)order.size(), env_int("FRUITS_BUNDLE_THREADS", 4)));
    std::vector<std::thread> pool;
    for (int i = 1; i < n_threads; ++i) pool.emplace_back(worker);
    worker();
    for (std::thread &th : pool) th.join();
  } else if ((int)p.nodes.size() <= fr::kFusedStaticMaxNodes && debug_knob("fused_static", 1) != 0) {
    // a small plan as straight-line code, for the group program of `groups` groups per series
    std::thread sieves_only([&] { one(jops, key, nullptr); });
    fr::FusedPlan fp;
    {
      std::lock_guard<std::mutex> lock(p.mu);
      const fr::GroupedProgram &gp = fr::grouped(p, groups > 0 ? groups : 1);
      fp.w.reserve(gp.recs.size() * 16);
      for (const fr::NodeRec &r : gp.recs) fp.w.insert(fp.w.end(), r.w, r.w + 16);
      fp.group_begin.assign(gp.group_begin.begin(), gp.group_begin.begin() + gp.groups);
    }
    one(jops, key, &fp);
    sieves_only.join();
  } else {
    one(jops, key, nullptr);
  }
  if (!errs.empty()) {
    if (msg && msg_cap > 0) snprintf(msg, (size_t)msg_cap, "%s", errs[0].c_str());
    return fail(FR_E_LIMIT, "fr_pipeline_bundle: " + errs[0]);
  }
  return done.load();
}

int fr_pipeline_set_series_cuts(fr_pipeline_t *pl, const int32_t *d_cuts, int64_t N, int32_t slots) {
  if (!pl || N < 0 || slots < 0 || (N * slots > 0 && !d_cuts))
    return fail(FR_E_ARG, "fr_pipeline_set_series_cuts: bad argument");
  if (slots < pl->cut_slots_needed)
    return fail(FR_E_ARG, "fr_pipeline_set_series_cuts: the sieves name " +
                              std::to_string(pl->cut_slots_needed) + " slots, the table has " +
                              std::to_string(slots));
  pl->d_series_cuts = d_cuts;
  pl->cuts_N = N;
  pl->cut_slots = slots;
  return FR_OK;
}

int fr_pipeline_set_lengths(fr_pipeline_t *pl, const int32_t *d_lengths, int64_t N) {
  if (!pl || N < 0) return fail(FR_E_ARG, "fr_pipeline_set_lengths: bad argument");
  pl->d_lengths = d_lengths;
  pl->lengths_N = d_lengths ? N : 0;
  return FR_OK;
}

int fr_pipeline_run(fr_pipeline_t *pl, const double *d_X, int64_t N, int64_t D, int64_t T,
                    const double *d_lookup, int64_t lookup_rows, double *d_feats,
                    int64_t feat_stride, void *d_work, int64_t work_bytes, int32_t groups,
                    void *stream) {
  if (!pl || !pl->plan || !pl->plan->p) return fail(FR_E_ARG, "fr_pipeline_run: null pipeline");
  fr::Plan &p = *pl->plan->p;
  if (T != pl->T) return fail(FR_E_ARG, "fr_pipeline_run: pipeline was created for another T");
  if (!pl->have_quantiles)
    return fail(FR_E_ARG, "fr_pipeline_run: call fr_pipeline_set_quantiles first");
  const int64_t F = (int64_t)pl->per_sum * pl->rows();
  if (N == 0 || F == 0) return FR_OK;
  if (!d_feats || feat_stride < F) return fail(FR_E_ARG, "fr_pipeline_run: bad feature buffer");
  const int64_t need = fr_pipeline_workspace_bytes(pl, N, lookup_rows);
  if (need > 0 && (!d_work || work_bytes < need))
    return fail(FR_E_NOMEM, "fr_pipeline_run: workspace too small (need " +
                                std::to_string(need) + " bytes)");
  hipStream_t st = (hipStream_t)stream;
  const size_t plan_ws = align_up(work_layout(p, N, T, p.weighting ? lookup_rows : 0).total(), 256);
  FusedArgs fu;
  fu.pl = pl;
  fu.ops = static_cast<const fr::FeatOp *>(pl->d_ops);
  fu.feats = d_feats;
  fu.feat_stride = feat_stride;
  fu.n_ops = pl->n_ops_eff;
  fu.n_ops_padded = pl->n_ops_padded;
  for (const PipeSieve &sv : pl->sieves)
    if (sv.kind != FR_SIEVE_END && sv.inc >= 1) fu.total_inc = true;
  fu.carry_per_node = pl->jit_ops.cps;
  if (pl->cut_slots_needed > 0) {
    if (!pl->d_series_cuts || pl->cuts_N != N || pl->cut_slots < pl->cut_slots_needed)
      return fail(FR_E_ARG, "fr_pipeline_run: a sieve has per-series cuts - call "
                            "fr_pipeline_set_series_cuts with a table for these " +
                                std::to_string(N) + " series first");
    fu.series_cuts = pl->d_series_cuts;
    fu.cut_slots = pl->cut_slots;
  }
  if (pl->d_lengths && pl->lengths_N != N)
    return fail(FR_E_ARG, "fr_pipeline_run: fr_pipeline_set_lengths was called for " +
                              std::to_string(pl->lengths_N) + " series, the input has " + std::to_string(N));
  // (a PPV / CPV that counts up to the series' own length is divided by it)
  if (pl->implicit_series_cuts && !pl->d_lengths)
    return fail(FR_E_ARG, "fr_pipeline_run: a PPV / CPV sieve has per-series cuts - call "
                          "fr_pipeline_set_lengths first");
  const int32_t *implicit_lengths = pl->implicit_series_cuts ? pl->d_lengths : nullptr;
  // (the population table of MPI features shares the feature row stride)
  if (!pl->mpi_cols.empty() && feat_stride != F)
    return fail(FR_E_ARG, "fr_pipeline_run: MPI needs feat_stride == F");
  if (N < 0 || D < 1 || !d_X) return fail(FR_E_ARG, "fr_pipeline_run: bad input");
  if (pl->prep_n > 0 && D != pl->prep_D)
    return fail(FR_E_ARG, "fr_pipeline_run: the fused preparation was set for " +
                              std::to_string(pl->prep_D) + " raw dimensions, the input has " +
                              std::to_string(D));
  const int64_t D_words = pl->prep_n > 0 ? pl->prep_n : D;
  if (p.max_dim > D_words)
    return fail(FR_E_DIM, "fr_pipeline_run: a word references dimension " +
                              std::to_string(p.max_dim) + " but the input has only " +
                              std::to_string(D_words));
  if (p.weighting != 0 && !p.cos && (!d_lookup || (lookup_rows != 1 && lookup_rows != N)))
    return fail(FR_E_ARG, "fr_pipeline_run: weighted plan needs a lookup of 1 or N rows");
  // (every feature column - and population entry - is written exactly once by the unit that
  // owns it: nothing to clear)
  if (!pl->mpi_cols.empty()) {
    fu.cnt = reinterpret_cast<double *>(static_cast<char *>(d_work) + plan_ws);
    fu.has_mpi = true;
  } else {
    fu.cnt = d_feats;  // never touched without MPI sieves
  }
  if (pl->prep_n > 0) {
    fu.prep = static_cast<const int32_t *>(pl->d_prep);
    fu.n_prep = pl->prep_n;
    if (pl->prep_std != 0) {
      // STD's statistics of the prepared rows: a small pre-pass over the raw input
      size_t off = plan_ws;
      if (!pl->mpi_cols.empty()) off += align_up((size_t)N * F * 8, 256);
      double *stats = reinterpret_cast<double *>(static_cast<char *>(d_work) + off);
      hipError_t e = fr::launch_row_stats(d_X, N, D, T, pl->d_lengths, fu.prep, pl->prep_n,
                                          pl->prep_std == 2 ? 1 : 0, pl->prep_eps, stats, st);
      if (e != hipSuccess) return hip_fail(e, "row_stats launch");
      fu.stats = stats;
    }
  }
  if (!pl->argmax_words.empty()) {
    // Arctic argmax: the running maxima of every prefix (the plan's rows) as a (K, N, T) block of
    // the workspace, then ONE kernel that forms the argmax rows and their features
    size_t off = plan_ws;
    if (!pl->mpi_cols.empty()) off += align_up((size_t)N * F * 8, 256);
    double *V = reinterpret_cast<double *>(static_cast<char *>(d_work) + off);
    int rc = run_walk("fr_pipeline_run", p, d_X, N, D, T, d_lookup, lookup_rows, V, N * T, T, d_work,
                      (int64_t)plan_ws, groups, st, nullptr);
    if (rc != FR_OK) return rc;
    hipError_t e = fr::launch_argmax_sieves(V, N, T, pl->d_argmax_words, (int)pl->argmax_words.size() / 4,
                                            pl->argmax_max_len, fu.ops, fu.n_ops, fu.n_ops_padded, d_feats,
                                            fu.cnt, feat_stride, fu.series_cuts, fu.cut_slots, st);
    if (e != hipSuccess) return hip_fail(e, "argmax_sieves launch");
    if (!pl->mpi_cols.empty()) {
      e = fr::launch_mpi_finalize(d_feats, fu.cnt, N, feat_stride,
                                  static_cast<const int32_t *>(pl->d_mpi_cols), (int)pl->mpi_cols.size(),
                                  static_cast<const int32_t *>(pl->d_npi_pairs),
                                  (int)pl->npi_pairs.size() / 2, pl->per_sum, pl->rows(), st);
      if (e != hipSuccess) return hip_fail(e, "mpi_finalize launch");
    }
    return FR_OK;
  }
  const int32_t *walk_of_row = nullptr;
  if (pieces_eligible(*pl)) {
    size_t off = plan_ws;
    if (!pl->mpi_cols.empty()) off += align_up((size_t)N * F * 8, 256);
    if (pl->prep_n > 0 && pl->prep_std != 0) off += align_up((size_t)N * pl->prep_n * 16, 256);
    fu.walk_feats = reinterpret_cast<double *>(static_cast<char *>(d_work) + off);
    fu.walk_of_row = &walk_of_row;
  }
  int rc = run_walk("fr_pipeline_run", p, d_X, N, D, T, d_lookup, lookup_rows, nullptr, 0, 0,
                    d_work, (int64_t)plan_ws, groups, st, &fu);
  if (rc != FR_OK) return rc;
  if (walk_of_row != nullptr) {
    // the features are in walk order (plan.h, PiecedProgram): band means there, then the blocks
    // of every iterated sum to their columns
    if (!pl->mpi_cols.empty()) {
      hipError_t e = fr::launch_mpi_finalize(fu.walk_feats, fu.cnt, N, F,
                                             static_cast<const int32_t *>(pl->d_mpi_cols),
                                             (int)pl->mpi_cols.size(),
                                             static_cast<const int32_t *>(pl->d_npi_pairs),
                                             (int)pl->npi_pairs.size() / 2, pl->per_sum, p.K, st);
      if (e != hipSuccess) return hip_fail(e, "mpi_finalize launch");
    }
    if (!pl->key_cols.empty()) {
      hipError_t e = fr::launch_band_key_finalize(fu.walk_feats, N, F,
                                                  static_cast<const int32_t *>(pl->d_key_cols),
                                                  (int)pl->key_cols.size(), pl->per_sum, p.K, st);
      if (e != hipSuccess) return hip_fail(e, "band_key_finalize launch");
    }
    if (!pl->implicit_cols.empty()) {
      hipError_t e = fr::launch_implicit_finalize(fu.walk_feats, N, F,
                                                  static_cast<const int32_t *>(pl->d_implicit_cols),
                                                  (int)pl->implicit_cols.size(), pl->per_sum, p.K, T,
                                                  implicit_lengths, st);
      if (e != hipSuccess) return hip_fail(e, "implicit_finalize launch");
    }
    hipError_t e = fr::launch_gather_row_blocks(fu.walk_feats, d_feats, N, F, feat_stride, p.K,
                                                pl->per_sum, walk_of_row, st);
    if (e != hipSuccess) return hip_fail(e, "gather_row_blocks launch");
    return FR_OK;
  }
  if (!pl->mpi_cols.empty()) {
    hipError_t e = fr::launch_mpi_finalize(d_feats, fu.cnt, N, feat_stride,
                                           static_cast<const int32_t *>(pl->d_mpi_cols),
                                           (int)pl->mpi_cols.size(),
                                           static_cast<const int32_t *>(pl->d_npi_pairs),
                                           (int)pl->npi_pairs.size() / 2, pl->per_sum, p.K, st);
    if (e != hipSuccess) return hip_fail(e, "mpi_finalize launch");
  }
  if (!pl->key_cols.empty()) {
    hipError_t e = fr::launch_band_key_finalize(d_feats, N, feat_stride,
                                                static_cast<const int32_t *>(pl->d_key_cols),
                                                (int)pl->key_cols.size(), pl->per_sum, p.K, st);
    if (e != hipSuccess) return hip_fail(e, "band_key_finalize launch");
  }
  if (!pl->implicit_cols.empty()) {
    hipError_t e = fr::launch_implicit_finalize(d_feats, N, feat_stride,
                                                static_cast<const int32_t *>(pl->d_implicit_cols),
                                                (int)pl->implicit_cols.size(), pl->per_sum, p.K, T,
                                                  implicit_lengths, st);
    if (e != hipSuccess) return hip_fail(e, "implicit_finalize launch");
  }
  return FR_OK;
}

}  // extern "C"
