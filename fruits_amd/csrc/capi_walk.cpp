// The walk runner: one call of the trie walk or of CosWISS, materialising (fr_iss_run) or
// fused with a pipeline's sieves (fr_pipeline_run): checks, the launch choice (launch_choice.h),
// the kernel arguments and the launch.
#include <mutex>
#include <string>

#include "capi_pipeline.h"
#include "capi_plan.h"
#include "kernels.h"
#include "launch_cache.h"

namespace fr::capi {
namespace {

// One call of the walk (fr_iss_run, fr_pipeline_run): what run_walk's parts share.
struct WalkCall {
  const char *who;
  fr::Plan &p;
  const double *d_X;
  int64_t N, D, T;
  const double *d_lookup;
  int64_t lookup_rows;
  double *d_out;
  int64_t out_k_stride, out_n_stride;
  void *d_work;
  int64_t work_bytes;
  int32_t groups;
  hipStream_t st;
  const FusedArgs *fu;
  fr::IssArgs args() const {   // input, output and shape: the same for every kernel
    fr::IssArgs a{};
    a.X = d_X;
    a.out = d_out;
    a.N = N;
    a.D = D;
    a.T = T;
    a.out_k_stride = out_k_stride;
    a.out_n_stride = out_n_stride;
    return a;
  }
};

// `run` = false: nothing to compute.  (A CosWISS plan's own limits: run_coswiss.)
int check_walk_args(const WalkCall &c, bool &run) {
  const fr::Plan &p = c.p;
  const std::string w(c.who);
  run = false;
  if (c.N < 0 || c.D < 1 || c.T < 0) return fail(FR_E_ARG, w + ": bad shape");
  const int64_t D_words = (c.fu && c.fu->prep) ? c.fu->n_prep : c.D;   // dimensions the words may name
  if (p.max_dim > D_words)
    return fail(FR_E_DIM, w + ": a word references dimension " + std::to_string(p.max_dim) +
                              " but the input has only " + std::to_string(D_words));
  if (c.N == 0 || c.T == 0 || p.K == 0 || (!p.cos && p.nodes.empty())) return FR_OK;
  if (!c.d_X || (!c.fu && !c.d_out)) return fail(FR_E_ARG, w + ": null device pointer");
  run = true;
  if (p.cos) return FR_OK;
  if (p.weighting != 0) {
    if (!c.d_lookup) return fail(FR_E_ARG, w + ": weighted plan needs a lookup");
    if (c.lookup_rows != 1 && c.lookup_rows != c.N)
      return fail(FR_E_ARG, w + ": lookup_rows must be 1 or N");
  }
  const size_t need = work_layout(p, c.N, c.T, p.weighting ? c.lookup_rows : 0).total();
  if (need > 0 && (!c.d_work || (size_t)c.work_bytes < need))
    return fail(FR_E_NOMEM, w + ": workspace too small (need " + std::to_string(need) + " bytes)");
  // the staged rows (input dimensions + exp tables) of one time chunk must fit the LDS
  if (!fr::staged_rows_fit(p, c.T))
    return fail(FR_E_LIMIT, w + ": the plan stages " + std::to_string(p.rows_staged()) +
                                " rows per time chunk (input dimensions + exp tables of " +
                                std::to_string(p.alphas.size()) +
                                " distinct alphas), more than the LDS holds - split the word list");
  return FR_OK;
}

// The sieve side of a fused launch, the trie walk's and CosWISS's alike.
void apply_fused_args(const FusedArgs &fu, fr::IssArgs &a) {
  a.ops = fu.ops;
  a.feats = fu.feats;
  a.cnt = fu.cnt;
  a.feat_stride = fu.feat_stride;
  a.n_ops = fu.n_ops;
  a.n_ops_padded = fu.n_ops_padded;
  a.series_cuts = fu.series_cuts;
  a.cut_slots = fu.cut_slots;
  a.has_mpi = fu.has_mpi ? 1 : 0;
  if (fu.prep) {
    a.prep = fu.prep;
    a.stats = fu.stats;
    a.n_prep = fu.n_prep;
  }
}

int run_coswiss(const WalkCall &c, const fr::WalkKnobs &k) {
  fr::Plan &p = c.p;
  fr::CosProgram &cp = *p.cos;
  const FusedArgs *fu = c.fu;
  const std::string w(c.who);
  const int64_t T = c.T;
  if (cp.exponent > fr::kCosMaxExponent || p.levels > 16)
    return fail(FR_E_LIMIT, w + ": CosWISS kernels cover exponents <= 4 and words of <= 16 "
                            "letters");
  const size_t need = work_layout(p, c.N, T, 0).total();
  if (!c.d_work || (size_t)c.work_bytes < need)
    return fail(FR_E_NOMEM, w + ": workspace too small (need " + std::to_string(need) +
                                " bytes)");
  {
    std::lock_guard<std::mutex> lock(p.mu);
    int rc = ensure_cos_program(p, cp, c.st, c.who);
    if (rc != FR_OK) return rc;
  }
  double *trig = static_cast<double *>(c.d_work);
  hipError_t e = fr::launch_trig_tables(cp.d_freqs, cp.F, T, trig, c.st);
  if (e != hipSuccess) return hip_fail(e, "trig_tables launch");
  fr::IssArgs a = c.args();
  a.aux = trig;
  a.factors = cp.d_factors;
  a.cw_letter_begin = cp.d_letter_begin;
  a.cw_fac_begin = cp.d_fac_begin;
  a.cw_W = cp.W;
  a.cw_F = cp.F;
  a.cw_total = cp.total ? 1 : 0;
  if (cp.d_mask) {
    if (cp.mask_T != T)
      return fail(FR_E_ARG, w + ": the dropout mask was set for series of length " +
                                std::to_string(cp.mask_T));
    a.cw_mask = static_cast<const double *>(cp.d_mask);
    a.cw_Lmax = cp.Lmax;
  }
  a.cw_x_unit_stride = cp.x_unit_stride;
  if (fu && fu->prep && cp.x_unit_stride != 0)
    return fail(FR_E_LIMIT, w + ": a CosWISS with per-unit inputs (ffn) has no fused preparation");
  a.packed = (T <= 384 && k.packed != 0) ? 1 : 0;
  a.vec_ok = (T % 2 == 0) && aligned16(c.d_X) && aligned16(trig) &&
             (fu || (aligned16(c.d_out) && (c.out_k_stride % 2 == 0) && (c.out_n_stride % 2 == 0)));
  if (fu) {
    apply_fused_args(*fu, a);
    // feature window of the cooperative kernel: the ops of the unit's one output row
    a.feat_window = (fu->n_ops + 1) / 2 * 2;
    a.feat_fits = 1;
    if (a.feat_window > 4096)
      return fail(FR_E_LIMIT, w + ": too many sieve features per iterated sum for the fused launch");
  }
  // one short-lived workgroup per (series, word, frequency) unit: 0-2.5 % faster than a
  // persistent grid (exponent 2: 1515 -> 1478 us)
  a.persistent = 0;
  e = fr::launch_coswiss(a, cp.exponent, c.st);
  if (e != hipSuccess) return hip_fail(e, "coswiss launch");
  return FR_OK;
}

// What choose_walk_launch needs to know of this call.  Caller holds p.mu.
fr::WalkFacts gather_walk_facts(const WalkCall &c, bool vec_ok, const fr::WalkKnobs &k) {
  fr::Plan &p = c.p;
  const bool total_inc = c.fu && c.fu->total_inc && p.weighting == FR_W_TOTAL;
  fr::WalkFacts f = walk_facts(p, c.N, c.T, c.groups, c.fu != nullptr, total_inc, vec_ok, k);
  if (c.fu) f.carry_per_node = c.fu->carry_per_node;
  if (!fr::static_launch_possible(p, f, k)) return f;
  lookup_static_programs(p);
  // no ahead-of-time program: one compiled at run time by fr_plan_prepare - or right here
  // with FRUITS_HIP_JIT=2 (a couple of seconds, once per plan; never inside a capture)
  if (p.static_prog[1] <= 0 && k.hip_jit == 2 && !stream_is_capturing(c.st)) ensure_jit(p);
  for (int g = 1; g <= 3; ++g) f.aot[g] = p.static_prog[g];
  // (a module is loaded on ONE device: elsewhere the interpreter runs the plan)
  if (const JitState *js = static_cast<const JitState *>(p.jit))
    for (const auto &kv : js->progs)
      if (kv.first <= 3 && kv.second.device == fr::current_device()) f.jit[kv.first] = true;
  f.tail_groups = fr::static_program_tail_groups(p.static_prog[1]);
  f.mixed_resident = [&p, &c] { return query_mixed_resident(p.static_prog[1], c.N, c.T); };
  return f;
}

// The kernel arguments of the launch `ch` of group program `gp`; fills the exp tables.
int fill_walk_args(const WalkCall &c, const fr::GroupedProgram &gp, const fr::WalkChoice &ch,
                   bool vec_ok, const fr::WalkKnobs &k, fr::IssArgs &a) {
  const fr::Plan &p = c.p;
  const FusedArgs *fu = c.fu;
  const std::string w(c.who);
  const int64_t T = c.T;
  const WorkLayout wl = work_layout(p, c.N, T, p.weighting ? c.lookup_rows : 0);
  a.n_whole = ch.n_whole;
  a.recs = gp.d_recs;
  a.factors = gp.d_factors;
  a.emit_rows = gp.d_emit_rows;
  a.slot_rows = gp.d_slot_rows;
  a.group_row_begin = gp.d_group_row_begin;
  a.shape_ids = gp.d_shape_ids;
  a.group_begin = gp.d_group_begin;
  a.row_src = gp.d_row_src;
  a.G = gp.groups;
  a.R = p.rows_staged();
  a.total_nodes = (int32_t)p.nodes.size();
  char *work = static_cast<char *>(c.d_work);
  if (p.weighting != 0) {
    double *aux = reinterpret_cast<double *>(work);
    const int64_t count = c.lookup_rows * T;
    hipError_t e = fr::launch_exp_tables(c.d_lookup, count, gp.d_alphas, (int)p.alphas.size(), aux,
                                         p.semiring == fr::kSemiArctic, c.st);
    if (e != hipSuccess) return hip_fail(e, "exp_tables launch");
    a.aux = aux;
    a.aux_tab_stride = count;
    a.aux_n_stride = c.lookup_rows == 1 ? 0 : T;
  }
  if (wl.carry_bytes) a.carry = reinterpret_cast<double *>(work + wl.aux_bytes);
  a.vec_ok = vec_ok && (!a.aux || aligned16(a.aux));
  a.debug = k.stamps;
  if (a.debug & 16) {
    // diagnostic build only: stamps go to the tail of the workspace if the caller
    // sized it with FRUITS_HIP_DBG_BYTES extra bytes
    if (k.dbg_bytes > 0 && c.d_work && c.work_bytes >= (int64_t)wl.total() + k.dbg_bytes)
      a.dbg = reinterpret_cast<unsigned long long *>(work + align_up(wl.total(), 256));
  }
  a.persistent = ch.persistent;
  a.packed = ch.packed ? 1 : 0;
  a.prefetch_next = 24;  // longest unit (nodes) that touches its successor's rows
  a.semiring = p.semiring;
  a.letter_sum = p.letter_sum ? 1 : 0;
  a.k_stride_bytes32 = (c.out_k_stride > 0 && c.out_k_stride < (int64_t(1) << 29))
                           ? (uint32_t)(c.out_k_stride * 8) : 0u;
  a.xcd_map = ch.xcd_map;
  a.carry_slots = ch.carry_slots;
  a.carry_per_node = ch.carry_per_node;
  a.carry_in_lds = ch.carry_in_lds;
  a.static_prog = ch.static_prog > 0 ? ch.static_prog : 0;
  a.lds_pad = ch.lds_pad;
  a.wt = ch.wt;
  a.lean = ch.lean;
  a.nt_input = ch.nt_input;
  a.total_weighting = ((fu || ch.lean) && p.weighting == FR_W_TOTAL) ? 1 : 0;
  if (!fu) return FR_OK;
  apply_fused_args(*fu, a);
  a.total_inc = (fu->total_inc && p.weighting == FR_W_TOTAL) ? 1 : 0;
  a.high_order = fu->carry_per_node > 3 ? 1 : 0;
  if ((int64_t)p.K * fu->n_ops_padded * 32 >= (int64_t(1) << 32) || gp.recs.size() >= (size_t(1) << 26))
    return fail(FR_E_LIMIT, w + ": the program tables exceed 4 GiB - split the word list");
  if (!ch.packed) {
    const int64_t chunk = fr::walk_chunk_elems(T);
    const size_t other = ((size_t)a.R * chunk + 24 + (T > chunk ? a.carry_slots : 0)) * 8;
    bool fits = false;
    a.feat_window = fr::feat_window_for(gp, other, fu->n_ops, fu->has_mpi, fits);
    a.feat_fits = fits ? 1 : 0;
    if (a.feat_window == 0)
      return fail(FR_E_LIMIT, w + ": the chunk carries and the features of one node (output rows "
                                  "x sieve features) do not fit the LDS - split the word list");
    if (p.letter_sum)
      return fail(FR_E_LIMIT, w + ": letter-sum (argmax) plans have no fused walk");
  }
  return FR_OK;
}

// A large plan in pieces (plan.h, PiecedProgram), where the pipeline has compiled them: one
// launch per piece type, each over (series x the type's units); the features leave in walk
// order.  `done` = false: the pipeline has no pieces for this launch.
int launch_pieces(const WalkCall &c, const fr::IssArgs &a, bool &done) {
  fr::Plan &p = c.p;
  const FusedArgs *fu = c.fu;
  const int64_t T = c.T;
  done = false;
  if (fu->walk_feats == nullptr || fu->walk_of_row == nullptr) return FR_OK;
  const fr::FusedKey key = fused_key_for(p, T, fu->total_inc, fu->carry_per_node > 3);
  fr_pipeline::Pieces pcs;
  {
    std::lock_guard<std::mutex> lock(fu->pl->jit_mu);
    auto it = fu->pl->jit_pieces.find(key.packed());
    if (it != fu->pl->jit_pieces.end() && !it->second.progs.empty() &&
        it->second.device == fr::current_device())
      pcs = it->second;
  }
  if (pcs.progs.empty()) return FR_OK;
  const fr::PiecedProgram *pp;
  {
    std::lock_guard<std::mutex> lock(p.mu);
    pp = &p.pieced.at(pcs.max_piece);
  }
  const int64_t chunk = fr::walk_chunk_elems(T);
  const int64_t F = (int64_t)p.K * fu->pl->per_sum;
  // (one launch per type, back to back on the caller's stream.  Forked onto side streams -
  // normal or low priority - behind an event and joined again the launches were 0.5-2 %
  // SLOWER on configs 4 / 5: kernels of different code on one CU share its instruction cache)
  for (size_t t = 0; t < pp->types.size(); ++t) {
    const fr::PieceType &pt = pp->types[t];
    fr::IssArgs b = a;
    b.recs = pt.d_recs;
    b.emit_rows = pt.d_emit_rows;
    b.piece_items = pt.d_items;
    b.piece_unit_begin = pt.d_unit_begin;
    b.piece_unit_row0 = pt.d_unit_row0;
    b.group_begin = b.slot_rows = b.group_row_begin = b.shape_ids = nullptr;
    b.G = pt.units();
    b.xcd_map = (b.G > 1 && c.N % 8 == 0) ? 1 : 0;
    b.ops = pcs.d_ops_walk;
    b.feats = fu->walk_feats;
    b.feat_stride = F;
    b.carry_per_node = fu->carry_per_node;
    b.carry_slots = b.carry_per_node * pt.max_unit_nodes;
    b.carry_in_lds = 1;
    b.persistent = 0;
    b.nchunks = (int32_t)((T + chunk - 1) / chunk);
    const size_t other = piece_other_lds(p, pt, T, b.carry_per_node);
    bool fits = false;
    b.feat_window = piece_window(p, pt, T, b.carry_per_node, fu->n_ops, fu->has_mpi, fits);
    b.feat_fits = fits ? 1 : 0;
    if ((pcs.fits[t] != 0) != fits)   // (the kernel was compiled for exactly this: ensure_fused_pieces)
      return fail(FR_E_LIMIT, std::string(c.who) + ": a piece kernel was compiled for another feature window");
    if (b.feat_window == 0)
      return fail(FR_E_LIMIT, std::string(c.who) + ": the chunk carries and the features of one node do not fit the LDS");
    const size_t lds = other + fr::feat_window_bytes(b.feat_window, b.has_mpi != 0);
    hipError_t je = fr::jit_launch_fused(pcs.progs[t], b, lds, c.st);
    if (je != hipSuccess) return hip_fail(je, "fused walk (a piece type) launch");
  }
  *fu->walk_of_row = pcs.d_walk_of_row;
  done = true;
  return FR_OK;
}

// The pipeline's run-time compiled kernel for this instantiation (fr_pipeline_prepare).
// `done` = false: it has none on this device.
int launch_own_kernel(const WalkCall &c, const fr::GroupedProgram &gp, fr::IssArgs &a, bool &done) {
  const FusedArgs *fu = c.fu;
  done = false;
  const fr::FusedKey key = fused_key_for(c.p, c.T, fu->total_inc, fu->carry_per_node > 3);
  fr::JitProgram own{};
  {
    std::lock_guard<std::mutex> lock(fu->pl->jit_mu);
    auto st_it = fu->pl->jit_static.find((uint64_t)key.packed() | (uint64_t)gp.groups << 32);
    if (st_it != fu->pl->jit_static.end() && st_it->second.device == fr::current_device()) {
      own = st_it->second;   // (the plan as straight-line code, for exactly this group program)
    } else {
      auto it = fu->pl->jit.find(key.packed());
      if (it != fu->pl->jit.end()) own = it->second;
    }
  }
  if (own.fn == nullptr || own.device != fr::current_device()) return FR_OK;
  const int64_t chunk = fr::walk_chunk_elems(c.T);
  a.nchunks = (int32_t)((c.T + chunk - 1) / chunk);
  const size_t lds = ((size_t)a.R * chunk + 16 + 8 + (a.nchunks > 1 ? a.carry_slots : 0)) * 8 +
                     fr::feat_window_bytes(a.feat_window, a.has_mpi != 0);
  hipError_t je = fr::jit_launch_fused(own, a, lds, c.st);
  if (je != hipSuccess) return hip_fail(je, "fused walk (run-time compiled) launch");
  done = true;
  return FR_OK;
}

}  // namespace

// Shared body of fr_iss_run and fr_pipeline_run: validates, chooses the launch
// (launch_choice.h), fills the exp tables and launches the trie walk.
int run_walk(const char *who, fr::Plan &p, const double *d_X, int64_t N, int64_t D, int64_t T,
             const double *d_lookup, int64_t lookup_rows, double *d_out, int64_t out_k_stride,
             int64_t out_n_stride, void *d_work, int64_t work_bytes, int32_t groups,
             hipStream_t st, const FusedArgs *fu) {
  const WalkCall c{who, p, d_X, N, D, T, d_lookup, lookup_rows, d_out, out_k_stride, out_n_stride,
                   d_work, work_bytes, groups, st, fu};
  const fr::WalkKnobs k = read_walk_knobs();
  bool run = false, done = false;
  int rc = check_walk_args(c, run);
  if (rc != FR_OK || !run) return rc;
  if (p.cos) return run_coswiss(c, k);
  const bool vec_ok = (T % 2 == 0) && aligned16(d_X) &&
                      (fu || (aligned16(d_out) && (out_k_stride % 2 == 0) && (out_n_stride % 2 == 0)));
  fr::WalkChoice ch;
  fr::LastLaunch rec;
  fr::GroupedProgram *gp = nullptr;
  const fr::JitProgram *jit_prog = nullptr;
  {
    std::lock_guard<std::mutex> lock(p.mu);
    fr::WalkFacts f = gather_walk_facts(c, vec_ok, k);
    if (f.mixed_resident) {   // (the record keeps what the mixed instance reported)
      f.mixed_resident = [&rec, ask = f.mixed_resident] { return rec.mixed_resident = ask(); };
    }
    ch = fr::choose_walk_launch(p, f, k);
    rec.resident = f.resident;
    gp = &fr::grouped(p, ch.G);   // (map nodes are stable: the pointer outlives the lock)
    if (ch.static_prog < 0) jit_prog = &static_cast<JitState *>(p.jit)->progs[ch.G];
    if (!ch.static_prog) {   // (a static program reads no device tables)
      rc = ensure_device_program(p, *gp, st, who);
      if (rc != FR_OK) return rc;
    }
  }
  fr::IssArgs a = c.args();
  rc = fill_walk_args(c, *gp, ch, vec_ok, k, a);
  if (rc != FR_OK) return rc;
  rec.choice = ch;
  rec.family = fr::walk_family(ch, fu != nullptr);
  auto keep_record = [&p, &rec] {   // FR_INFO_STATIC_TAIL, FR_INFO_LAST_LAUNCH
    std::lock_guard<std::mutex> lock(p.mu);
    p.last_tail_series = rec.choice.tail_series;
    p.last_launch = rec;
  };
  if (fu && fu->pl && !ch.packed) {
    rc = launch_pieces(c, a, done);
    if (done) rec.family = fr::kWalkFusedPieces;
    if (rc == FR_OK && !done) {
      rc = launch_own_kernel(c, *gp, a, done);
      if (done) rec.family = fr::kWalkFusedJit;
    }
    if (rc != FR_OK || done) {
      if (done) keep_record();
      return rc;
    }
  }
  keep_record();
  hipError_t e = jit_prog ? fr::jit_launch(*jit_prog, a, st) : fr::launch_iss_walk(a, p.levels, st);
  if (e != hipSuccess) return hip_fail(e, "iss_walk launch");
  return FR_OK;
}

}  // namespace fr::capi

using namespace fr::capi;

extern "C" {

int fr_iss_run(fr_plan_t *plan, const double *d_X, int64_t N, int64_t D, int64_t T,
               const double *d_lookup, int64_t lookup_rows, double *d_out, int64_t out_k_stride,
               int64_t out_n_stride, void *d_work, int64_t work_bytes, int32_t groups,
               void *stream) {
  if (!plan || !plan->p) return fail(FR_E_ARG, "fr_iss_run: null plan");
  return run_walk("fr_iss_run", *plan->p, d_X, N, D, T, d_lookup, lookup_rows, d_out,
                  out_k_stride, out_n_stride, d_work, work_bytes, groups, (hipStream_t)stream,
                  nullptr);
}

int fr_iterated_sum_fast_host(const double *h_Z, int64_t N, int64_t D, int64_t T,
                              const int32_t *word, int32_t L, int32_t Dw, const float *alpha,
                              const double *h_lookup, int64_t extended, int32_t total_weighting,
                              double *h_out) {
  if (!h_Z || !word || !h_out || N < 0 || D < 1 || T < 0 || L < 1 || Dw < 1)
    return fail(FR_E_ARG, "fr_iterated_sum_fast_host: bad argument");
  if (extended < 1 || extended > L)
    return fail(FR_E_ARG, "fr_iterated_sum_fast_host: extended must be in [1, L]");
  const int weighting = h_lookup ? ((total_weighting & 1) ? FR_W_TOTAL : FR_W_NONTOTAL) : FR_W_NONE;
  const int plan_flags = (total_weighting & 2) ? FR_PLAN_ARCTIC
                                               : ((total_weighting & 4) ? FR_PLAN_BAYESIAN : 0);
  if (weighting != FR_W_NONE && !alpha)
    return fail(FR_E_ARG, "fr_iterated_sum_fast_host: weighted call needs alpha");
  const int32_t depth = (int32_t)extended;
  fr_plan_t *plan = fr_plan_create(1, word, &L, &Dw, alpha, &depth, weighting, plan_flags);
  if (!plan) return FR_E_ARG;
  int rc = FR_OK;
  void *dZ = nullptr, *dL = nullptr, *dO = nullptr, *dW = nullptr;
  const int64_t zb = N * D * T * 8, lb = h_lookup ? N * T * 8 : 0, ob = N * extended * T * 8;
  const int64_t wb = fr_plan_workspace_bytes(plan, N, T, h_lookup ? N : 0);
  do {
    if (N == 0 || T == 0) break;
    if ((rc = fr_malloc(&dZ, zb)) != FR_OK) break;
    if ((rc = fr_malloc(&dO, ob)) != FR_OK) break;
    if (lb && (rc = fr_malloc(&dL, lb)) != FR_OK) break;
    if (wb && (rc = fr_malloc(&dW, wb)) != FR_OK) break;
    if ((rc = fr_memcpy_h2d(dZ, h_Z, zb, nullptr)) != FR_OK) break;
    if (lb && (rc = fr_memcpy_h2d(dL, h_lookup, lb, nullptr)) != FR_OK) break;
    rc = fr_iss_run(plan, (const double *)dZ, N, D, T, (const double *)dL, h_lookup ? N : 0,
                    (double *)dO, /*k stride*/ T, /*n stride*/ extended * T, dW, wb, 0, nullptr);
    if (rc != FR_OK) break;
    if ((rc = fr_memcpy_d2h(h_out, dO, ob, nullptr)) != FR_OK) break;
    rc = fr_stream_sync(nullptr);
  } while (0);
  const std::string keep = g_err;
  (void)hipFree(dZ);
  (void)hipFree(dL);
  (void)hipFree(dO);
  (void)hipFree(dW);
  fr_plan_destroy(plan);
  if (rc != FR_OK) g_err = keep;
  return rc;
}

}  // extern "C"
