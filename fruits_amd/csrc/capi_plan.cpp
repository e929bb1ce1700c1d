// The plan's life: the fr_plan_* entries, the one-time uploads of a plan's tables, its
// run-time compiled static programs and the workspace layout.
#include <algorithm>
#include <cstring>
#include <vector>

#include "capi_plan.h"
#include "kernels.h"

namespace fr::capi {
namespace {

// Resident workgroups of the cooperative walk kernel instance that (plan, T, fused,
// vec_ok) selects: a dry run of the launcher (nothing is enqueued).
int64_t query_resident(const fr::Plan &p, int64_t N, int64_t T, bool fused, bool vec_ok,
                       const fr::WalkKnobs &k) {
  if (k.persist == 0) return 0;
  fr::IssArgs a{};
  int32_t resident = 0;
  double *const dummy = reinterpret_cast<double *>(uintptr_t(256));  // never dereferenced
  a.N = N;
  a.D = std::max(1, p.max_dim);
  a.T = T;
  a.G = 1;
  a.R = p.rows_staged();
  a.total_nodes = (int32_t)p.nodes.size();
  a.aux = p.weighting != 0 ? dummy : nullptr;
  a.carry = T > fr::walk_chunk_elems(T) ? dummy : nullptr;
  a.vec_ok = vec_ok ? 1 : 0;
  a.persistent = 1;
  a.semiring = p.semiring;
  a.carry_slots = fr::carry_slots_for(p, 1);
  a.carry_in_lds = (fused || fr::carries_fit_lds(p, T, 1)) ? 1 : 0;   // (the fused walk: always)
  a.feats = fused ? dummy : nullptr;
  a.feat_window = fused ? 128 : 0;   // (the launch's own window may differ a little)
  a.resident_out = &resident;
  if (fr::launch_iss_walk(a, p.levels, nullptr) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return resident;
}

}  // namespace

// Uploads the node order for G groups once per plan.  Allocates and copies
// synchronously: done by fr_plan_prepare, or by the first run outside a capture.
// Caller holds p.mu.
int ensure_device_program(fr::Plan &p, fr::GroupedProgram &gp, hipStream_t st, const char *who) {
  int rc = claim_device(p, who);
  if (rc != FR_OK) return rc;
  if (gp.d_blob) return FR_OK;
  if (stream_is_capturing(st))
    return fail(FR_E_ARG, std::string(who) + ": the stream is being captured and the plan's "
                          "tables for this shape are not on the device yet - call "
                          "fr_plan_prepare / fr_pipeline_prepare before the capture");
  const size_t n_recs = gp.recs.size();
  size_t off = 0;
  const size_t o_nodes = off;       off = align_up(off + n_recs * sizeof(fr::NodeRec), 64);
  const size_t o_gb = off;          off = align_up(off + gp.group_begin.size() * 4, 64);
  const size_t o_fac = off;         off = align_up(off + p.factors.size() * 4, 64);
  const size_t o_emit = off;        off = align_up(off + p.emit_rows.size() * 4, 64);
  const size_t o_rows = off;        off = align_up(off + p.row_src.size() * 4, 64);
  const size_t o_alpha = off;       off = align_up(off + p.alphas.size() * 4, 64);
  const size_t o_srows = off;       off = align_up(off + gp.slot_rows.size() * 4, 64);
  const size_t o_grb = off;         off = align_up(off + gp.group_row_begin.size() * 4, 64);
  const size_t o_shape = off;       off = align_up(off + gp.shape_ids.size() * 4, 64);
  std::vector<char> host(off + 64, 0);
  std::memcpy(host.data() + o_srows, gp.slot_rows.data(), gp.slot_rows.size() * 4);
  std::memcpy(host.data() + o_grb, gp.group_row_begin.data(), gp.group_row_begin.size() * 4);
  std::memcpy(host.data() + o_shape, gp.shape_ids.data(), gp.shape_ids.size() * 4);
  std::memcpy(host.data() + o_nodes, gp.recs.data(), n_recs * sizeof(fr::NodeRec));
  std::memcpy(host.data() + o_gb, gp.group_begin.data(), gp.group_begin.size() * 4);
  std::memcpy(host.data() + o_fac, p.factors.data(), p.factors.size() * 4);
  std::memcpy(host.data() + o_emit, p.emit_rows.data(), p.emit_rows.size() * 4);
  std::memcpy(host.data() + o_rows, p.row_src.data(), p.row_src.size() * 4);
  std::memcpy(host.data() + o_alpha, p.alphas.data(), p.alphas.size() * 4);
  void *d = nullptr;
  HIP_TRY(hipMalloc(&d, host.size()));
  hipError_t e = hipMemcpy(d, host.data(), host.size(), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(d);
    return hip_fail(e, "hipMemcpy(program)");
  }
  char *b = static_cast<char *>(d);
  gp.d_blob = d;
  gp.d_recs = reinterpret_cast<const fr::NodeRec *>(b + o_nodes);
  gp.d_group_begin = reinterpret_cast<const int32_t *>(b + o_gb);
  gp.d_factors = reinterpret_cast<const int32_t *>(b + o_fac);
  gp.d_emit_rows = reinterpret_cast<const int32_t *>(b + o_emit);
  gp.d_row_src = reinterpret_cast<const int32_t *>(b + o_rows);
  gp.d_alphas = reinterpret_cast<const float *>(b + o_alpha);
  gp.d_slot_rows = reinterpret_cast<const int32_t *>(b + o_srows);
  gp.d_group_row_begin = reinterpret_cast<const int32_t *>(b + o_grb);
  gp.d_shape_ids = reinterpret_cast<const int32_t *>(b + o_shape);
  return FR_OK;
}

// Caller holds p.mu.
int ensure_cos_program(fr::Plan &p, fr::CosProgram &c, hipStream_t st, const char *who) {
  int rc = claim_device(p, who);
  if (rc != FR_OK) return rc;
  if (c.d_blob) return FR_OK;
  if (stream_is_capturing(st))
    return fail(FR_E_ARG, std::string(who) + ": the stream is being captured and the CosWISS "
                          "program is not on the device yet - call fr_plan_prepare / "
                          "fr_pipeline_prepare before the capture");
  size_t off = 0;
  const size_t o_lb = off;    off = align_up(off + c.letter_begin.size() * 4, 64);
  const size_t o_fb = off;    off = align_up(off + c.fac_begin.size() * 4, 64);
  const size_t o_fac = off;   off = align_up(off + c.factors.size() * 4, 64);
  const size_t o_fr = off;    off = align_up(off + c.freqs.size() * 4, 64);
  std::vector<char> host(off + 64, 0);
  std::memcpy(host.data() + o_lb, c.letter_begin.data(), c.letter_begin.size() * 4);
  std::memcpy(host.data() + o_fb, c.fac_begin.data(), c.fac_begin.size() * 4);
  std::memcpy(host.data() + o_fac, c.factors.data(), c.factors.size() * 4);
  std::memcpy(host.data() + o_fr, c.freqs.data(), c.freqs.size() * 4);
  void *d = nullptr;
  HIP_TRY(hipMalloc(&d, host.size()));
  hipError_t e = hipMemcpy(d, host.data(), host.size(), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(d);
    return hip_fail(e, "hipMemcpy(coswiss program)");
  }
  char *b = static_cast<char *>(d);
  c.d_blob = d;
  c.d_letter_begin = reinterpret_cast<const int32_t *>(b + o_lb);
  c.d_fac_begin = reinterpret_cast<const int32_t *>(b + o_fb);
  c.d_factors = reinterpret_cast<const int32_t *>(b + o_fac);
  c.d_freqs = reinterpret_cast<const float *>(b + o_fr);
  return FR_OK;
}

// Resident workgroups of the mixed instance of ahead-of-time program `prog` (one group per series with its
// tail program, write-through stores, no LDS pad: the cache-sized window); 0: unknown
int64_t query_mixed_resident(int prog, int64_t N, int64_t T) {
  fr::IssArgs a{};
  int32_t resident = 0;
  a.N = N;
  a.T = T;
  a.G = 1;
  a.static_prog = prog;
  a.n_whole = 0;   // (asks the mixed instance)
  a.resident_out = &resident;
  if (fr::launch_iss_walk(a, 0, nullptr) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return resident;
}

// Compiles and loads the plan's static programs (one group and min(3, units) groups per
// series) unless an ahead-of-time program covers it.  Called with p.mu held; failures leave
// the plan on the interpreter.
void ensure_jit(fr::Plan &p) {
  if (p.jit == nullptr) p.jit = new JitState;
  JitState &js = *static_cast<JitState *>(p.jit);
  if (js.tried) return;
  js.tried = true;
  const int gmax = std::max(1, std::min(3, p.units()));
  for (int g : {1, gmax}) {
    if (js.progs.count(g)) continue;
    const fr::StaticSchedule sc = fr::static_schedule(p, g);
    if (!sc.ok || sc.groups != g) {
      js.error = "the plan does not qualify for a static program";
      return;
    }
    std::string code, err;
    fr::JitProgram prog;
    bool from_cache = false;
    bool ok = fr::jit_compile(sc, code, err, &from_cache) && fr::jit_load(code, sc, prog, err);
    if (!ok && from_cache) {
      // a cached code object the loader refuses (another ROCm, a damaged file): compile afresh
      fr::jit_cache_drop(sc);
      ok = fr::jit_compile(sc, code, err) && fr::jit_load(code, sc, prog, err);
    }
    if (!ok) {
      js.error = err;
      return;
    }
    js.progs[g] = prog;
  }
}

// The ahead-of-time static programs of the plan for 1, 2 and 3 groups per series (looked up
// once per plan).  Caller holds p.mu.
void lookup_static_programs(fr::Plan &p) {
  if (p.static_prog[0] >= 0) return;
  const fr::GroupedProgram &g1 = fr::grouped(p, 1);
  for (int g = 1; g <= 3; ++g)
    p.static_prog[g] = fr::static_program_for(g1.recs.data(), (int)g1.recs.size(), g, p.row_src.data(),
                                                   (int)p.row_src.size());
  p.static_prog[0] = 0;
}

// The facts of a launch without its static programs: what fr_plan_prepare and the pipeline's
// compilers choose the interpreter's node order from, and where a run starts.  Caller holds p.mu
// (`largest_group` lays the node order out).
fr::WalkFacts walk_facts(fr::Plan &p, int64_t N, int64_t T, int groups, bool fused, bool total_inc,
                         bool vec_ok, const fr::WalkKnobs &k) {
  fr::WalkFacts f{N, T, groups, fused, total_inc, 3, vec_ok};
  const bool packed = fr::walk_is_packed(fr::launch_shape(p, N, T, groups, k), total_inc);
  if (fr::host_chooses_groups(packed, groups, k)) f.resident = query_resident(p, N, T, fused, vec_ok, k);
  f.largest_group = [&p](int G) { return fr::largest_group(fr::grouped(p, G)); };
  return f;
}

// One-time uploads for the node order a run of this (N, T, groups) asks for.
int prepare_plan(fr::Plan &p, int64_t N, int64_t T, int32_t groups, bool fused, const char *who,
                 const fr::WalkKnobs &k) {
  std::lock_guard<std::mutex> lock(p.mu);
  if (p.cos) return ensure_cos_program(p, *p.cos, nullptr, who);
  if (N == 0 || T == 0 || p.K == 0 || p.nodes.empty()) return FR_OK;
  if (!fr::staged_rows_fit(p, T))
    return fail(FR_E_LIMIT, std::string(who) + ": the plan stages " +
                                std::to_string(p.rows_staged()) +
                                " rows per time chunk, more than the LDS holds - split the word list");
  // (the choice depends on the kernel instance - fused or not, 16-byte aligned or not -
  // which is only known when the pointers are: upload what either would ask for.  A static
  // program reads no tables: the node order is the one a run without it takes)
  for (const bool vec_ok : {true, false}) {
    if (fused && !vec_ok) break;
    const int G = fr::choose_walk_launch(p, walk_facts(p, N, T, groups, fused, false, vec_ok, k), k).G;
    int rc = ensure_device_program(p, fr::grouped(p, G), nullptr, who);
    if (rc != FR_OK) return rc;
  }
  return FR_OK;
}

WorkLayout work_layout(const fr::Plan &p, int64_t N, int64_t T, int64_t lookup_rows) {
  WorkLayout w;
  if (p.cos) {  // the (F, 2, T) sin / cos tables
    w.aux_bytes = align_up((size_t)p.cos->F * 2 * (size_t)T * 8, 256);
    return w;
  }
  if (p.weighting != 0)
    w.aux_bytes = align_up((size_t)p.aux_tables() * (size_t)lookup_rows * (size_t)T * 8, 256);
  if (T > fr::walk_chunk_elems(T))
    w.carry_bytes = align_up((size_t)N * 3 * p.nodes.size() * 8, 256);
  return w;
}

}  // namespace fr::capi

using namespace fr::capi;

extern "C" {

fr_plan_t *fr_plan_create(int32_t W, const int32_t *exps, const int32_t *L, const int32_t *Dw,
                          const float *alpha, const int32_t *depth, int32_t weighting,
                          int32_t flags) {
  std::string err;
  fr::Plan *p = fr::build_plan(W, exps, L, Dw, alpha, depth, weighting, flags, err);
  if (!p) {
    g_err = err;
    return nullptr;
  }
  fr_plan_t *h = new fr_plan_t;
  h->p = p;
  return h;
}

fr_plan_t *fr_plan_create_coswiss(int32_t W, const int32_t *exps, const int32_t *L,
                                  const int32_t *Dw, int32_t n_freqs, const float *freqs,
                                  int32_t exponent, int32_t total_weighting) {
  std::string err;
  fr::Plan *p = fr::build_coswiss_plan(W, exps, L, Dw, n_freqs, freqs, exponent,
                                       total_weighting, err);
  if (!p) {
    g_err = err;
    return nullptr;
  }
  fr_plan_t *h = new fr_plan_t;
  h->p = p;
  return h;
}

void fr_plan_destroy(fr_plan_t *plan) {
  if (!plan) return;
  if (plan->p) {
    if (plan->p->cos) {
      if (plan->p->cos->d_mask) (void)hipFree(plan->p->cos->d_mask);
      if (plan->p->cos->d_blob) (void)hipFree(plan->p->cos->d_blob);
      delete plan->p->cos;
    }
    for (auto &kv : plan->p->programs)
      if (kv.second.d_blob) (void)hipFree(kv.second.d_blob);
    for (auto &kv : plan->p->pieced)
      for (fr::PieceType &t : kv.second.types)
        if (t.d_blob) (void)hipFree(t.d_blob);
    if (plan->p->jit) {
      JitState *js = static_cast<JitState *>(plan->p->jit);
      for (auto &kv : js->progs) fr::jit_unload(kv.second);
      delete js;
    }
    release_grad_tables(*plan->p);
    delete plan->p;
  }
  delete plan;
}

int64_t fr_plan_info(const fr_plan_t *plan, int32_t what) {
  if (!plan || !plan->p) return fail(FR_E_ARG, "fr_plan_info: null plan");
  const fr::Plan &p = *plan->p;
  switch (what) {
    case FR_INFO_ROWS: return p.K;
    case FR_INFO_NODES: return (int64_t)p.nodes.size();
    case FR_INFO_LEVELS: return p.levels;
    case FR_INFO_DIMS_USED: return p.dims_used;
    case FR_INFO_MAX_DIM: return p.max_dim;
    case FR_INFO_ALPHAS: return (int64_t)p.alphas.size();
    case FR_INFO_GROUPS: return p.units();
    case FR_INFO_SHARED: return p.shared ? 1 : 0;
    case FR_INFO_STAGED_ROWS: return p.cos ? 0 : p.rows_staged();
    case FR_INFO_AOT_PROGRAM: {
      fr::Plan &q = *plan->p;
      if (q.cos) return 0;
      std::lock_guard<std::mutex> lock(q.mu);
      lookup_static_programs(q);
      return q.static_prog[1];
    }
    case FR_INFO_JIT_PROGRAMS:
      return p.jit ? (int64_t)static_cast<const JitState *>(p.jit)->progs.size() : 0;
    case FR_INFO_STATIC_TAIL: {
      fr::Plan &q = *plan->p;
      std::lock_guard<std::mutex> lock(q.mu);
      return q.last_tail_series;
    }
    case FR_INFO_LAST_LAUNCH:
    case FR_INFO_LAST_WHOLE: {
      fr::Plan &q = *plan->p;
      std::lock_guard<std::mutex> lock(q.mu);
      return what == FR_INFO_LAST_WHOLE ? (int64_t)q.last_launch.choice.n_whole
                                        : fr::pack_last_launch(q.last_launch);
    }
    case FR_INFO_GRAD_ROWS: {
      // a CosWISS plan's backward scratch in (N, T) rows: d_S holds u of the letters behind a
      // word's first, d_A dz of every letter and the (F, 2, T) trig rows behind them (2 F rows
      // are reserved whatever N)
      if (!p.cos) return 0;
      const int64_t letters = (int64_t)p.cos->fac_begin.size() - 1, F = p.cos->F;
      return (((letters - p.cos->W) * F) << 32) | (letters * F + 2 * F);
    }
    default: return fail(FR_E_ARG, "fr_plan_info: unknown selector");
  }
}

int32_t fr_plan_dump(const fr_plan_t *plan, int32_t *buf, int32_t cap) {
  if (!plan || !plan->p) return fail(FR_E_ARG, "fr_plan_dump: null plan");
  const fr::Plan &p = *plan->p;
  const int32_t n = (int32_t)p.nodes.size();
  for (int32_t i = 0; i < n && buf && (i + 1) * 8 <= cap; ++i) {
    const fr::NodeDesc &nd = p.nodes[i];
    int32_t *o = buf + (size_t)i * 8;
    o[0] = nd.level;
    o[1] = nd.flags;
    o[2] = nd.fac_count;
    o[3] = nd.emit_count;
    o[4] = nd.emit_count ? p.emit_rows[nd.emit_begin] : -1;
    o[5] = nd.emit_mul;
    o[6] = nd.z_mul;
    o[7] = p.unit_of[i];
  }
  return n;
}

int32_t fr_plan_records(fr_plan_t *plan, int32_t groups, int32_t *buf, int64_t cap_words) {
  if (!plan || !plan->p || plan->p->cos) return fail(FR_E_ARG, "fr_plan_records: not a trie plan");
  fr::Plan &p = *plan->p;
  std::lock_guard<std::mutex> lock(p.mu);
  const fr::GroupedProgram &gp = fr::grouped(p, groups);
  const int64_t n = (int64_t)gp.recs.size();
  if (buf != nullptr && cap_words >= n * 16)
    std::memcpy(buf, gp.recs.data(), (size_t)n * 64);
  return (int32_t)n;
}

int64_t fr_plan_pieces(fr_plan_t *plan, int32_t max_piece, int32_t *buf, int64_t cap_words) {
  if (!plan || !plan->p) return fail(FR_E_ARG, "fr_plan_pieces: null plan");
  fr::Plan &p = *plan->p;
  std::lock_guard<std::mutex> lock(p.mu);
  const fr::PiecedProgram &pp = fr::pieced(p, max_piece > 0 ? max_piece : fr::kFusedPieceNodes);
  if (!pp.ok) return 0;
  // header: types, K, node executions in chains, nodes of the plan; per type 8 words + its
  // records, items and unit tables; then the output row at every walk position
  std::vector<int32_t> out{(int32_t)pp.types.size(), p.K, pp.chain_nodes, (int32_t)p.nodes.size()};
  for (const fr::PieceType &t : pp.types) {
    out.insert(out.end(), {t.body_nodes, t.body_rows, t.levels, t.units(), (int32_t)t.items.size() / 4,
                           t.max_unit_nodes, (int32_t)t.recs.size(), t.max_unit_rows});
    for (const fr::NodeRec &r : t.recs) out.insert(out.end(), r.w, r.w + 16);
    out.insert(out.end(), t.items.begin(), t.items.end());
    out.insert(out.end(), t.unit_begin.begin(), t.unit_begin.end());
    out.insert(out.end(), t.unit_row0.begin(), t.unit_row0.end());
  }
  out.insert(out.end(), pp.row_of_walk.begin(), pp.row_of_walk.end());
  if (buf != nullptr && cap_words >= (int64_t)out.size()) std::memcpy(buf, out.data(), out.size() * 4);
  return (int64_t)out.size();
}

int32_t fr_plan_static_schedule(fr_plan_t *plan, int32_t groups, int32_t *buf, int64_t cap_words) {
  if (!plan || !plan->p) return fail(FR_E_ARG, "fr_plan_static_schedule: null plan");
  fr::Plan &p = *plan->p;
  std::lock_guard<std::mutex> lock(p.mu);
  const fr::StaticSchedule sc = fr::static_schedule(p, groups);
  if (!sc.ok) return 0;
  const int64_t n = (int64_t)sc.entries.size();
  // header (32 words): entries, rows, frames, groups, row sources [4..8), group_begin
  // [8..16), rows read by each group [16..24); then the entries
  const int64_t words = 32 + n * 16;
  if (sc.groups > 8) return 0;
  if (buf != nullptr && cap_words >= words) {
    std::memset(buf, 0, 128);
    buf[0] = (int32_t)n;
    buf[1] = sc.rows;
    buf[2] = sc.frames;
    buf[3] = sc.groups;
    for (int r = 0; r < sc.rows; ++r) buf[4 + r] = sc.row_src[r];
    for (int g = 0; g < sc.groups; ++g) {
      buf[8 + g] = sc.group_begin[g];
      buf[16 + g] = sc.group_rows[g];
    }
    std::memcpy(buf + 32, sc.entries.data(), (size_t)n * 64);
  }
  return (int32_t)n;
}

int64_t fr_plan_workspace_bytes(const fr_plan_t *plan, int64_t N, int64_t T, int64_t lookup_rows) {
  if (!plan || !plan->p || N < 0 || T < 0 || lookup_rows < 0)
    return fail(FR_E_ARG, "fr_plan_workspace_bytes: bad argument");
  return (int64_t)work_layout(*plan->p, N, T, lookup_rows).total();
}

int32_t fr_plan_fits(const fr_plan_t *plan, int64_t T) {
  if (!plan || !plan->p || T < 0) return fail(FR_E_ARG, "fr_plan_fits: bad argument");
  const fr::Plan &p = *plan->p;
  if (p.cos) return (p.cos->exponent <= fr::kCosMaxExponent && p.levels <= 16) ? 1 : 0;
  return fr::staged_rows_fit(p, T) ? 1 : 0;
}

int fr_plan_prepare(fr_plan_t *plan, int64_t N, int64_t T, int32_t groups) {
  if (!plan || !plan->p || N < 0 || T < 0) return fail(FR_E_ARG, "fr_plan_prepare: bad argument");
  fr::Plan &p = *plan->p;
  const fr::WalkKnobs k = read_walk_knobs();
  int rc = prepare_plan(p, N, T, groups, false, "fr_plan_prepare", k);
  if (rc != FR_OK) return rc;
  // a small plan without an ahead-of-time static program gets one compiled now (hipRTC,
  // cached on disk); a failure is not the caller's: the interpreter runs the plan
  if (fr::static_shape_ok(p, T, k) && k.hip_jit != 0 && k.hip_static != 0) {
    std::lock_guard<std::mutex> lock(p.mu);
    lookup_static_programs(p);
    if (p.static_prog[1] <= 0 && fr::static_schedule(p, 1).ok) ensure_jit(p);
  }
  return FR_OK;
}

int32_t fr_plan_jit(fr_plan_t *plan, int32_t groups, int32_t compile_only, char *msg, int64_t msg_cap) {
  if (!plan || !plan->p) return fail(FR_E_ARG, "fr_plan_jit: null plan");
  fr::Plan &p = *plan->p;
  std::lock_guard<std::mutex> lock(p.mu);
  auto say = [&](const std::string &s) {
    if (msg && msg_cap > 0) {
      const size_t n = std::min((size_t)msg_cap - 1, s.size());
      std::memcpy(msg, s.data(), n);
      msg[n] = 0;
    }
  };
  say("");
  if (compile_only) {   // needs no GPU: the code object's size, 0 when the plan has no schedule
    const fr::StaticSchedule sc = fr::static_schedule(p, groups);
    if (!sc.ok) return 0;
    std::string code, err;
    if (!fr::jit_compile(sc, code, err)) {
      say(err);
      return fail(FR_E_LIMIT, "fr_plan_jit: " + err);
    }
    return (int32_t)code.size();
  }
  ensure_jit(p);
  JitState &js = *static_cast<JitState *>(p.jit);
  say(js.error);
  return (int32_t)js.progs.size();
}

}  // extern "C"
