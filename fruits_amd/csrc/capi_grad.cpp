// fr_iss_backward: the gradient of unweighted Reals iterated sums with respect to their input;
// fr_iss_backward_max: the same for the max semirings Arctic and Bayesian;
// fr_iss_backward_weighted: the same for weighted Reals plans, total or not;
// fr_iss_backward_picked: any of the three with the sparse upstream of picked features.  The trie -
// parents, children, letters, exp tables - is read off the plan the plan compiler built (plan.cpp);
// the kernels are those of kernels_grad.hip.  One body (run_backward) serves the four entries.
// fr_plan_set_grad_lengths arms a plan with per-series lengths for the backward passes that follow,
// fr_plan_set_grad_pathlen a weighted plan with a path-length lookup (L1 / L2): the armed
// fr_iss_backward_weighted adds the gradient through the lookup.
// fr_iss_backward handed a CosWISS plan runs the adjoint of the factorised CosWISS kernels
// (run_backward_cos, kernels_grad_cos.hip): the plan itself, no prefix plan and no trie.
#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "capi_common.h"
#include "capi_plan.h"
#include "kernels.h"

using namespace fr::capi;

namespace {

// A table of the backward pass: the host copy and where it lies in the device blob.
struct Table {
  std::vector<int32_t> h;
  const int32_t *d = nullptr;
};

// The backward tables of a prefix plan.  The trie part is a function of the plan; the rows of G a
// node gathers are the caller's (`row_prefix`), kept to see whether a later call brings the same.
struct GradTables {
  std::vector<int32_t> row_prefix;
  // host only: where a depth begins in level_nodes (falling depth) and in inner_nodes (rising)
  std::vector<int32_t> level_begin, inner_begin;
  Table parent_srow, child_begin, child, fac_begin, fac, g_begin, g_row, level_nodes, dim_begin,
      dim_item, self_srow;
  // a weighted plan's: per node the exp tables {own E+, own E-, parent's E-} (-1: unused), the
  // nodes that have children by rising depth, and the bits of the plan's distinct alphas
  Table tab, inner_nodes, alpha_bits;
  // ... and, for a plan armed with a path-length lookup, the nodes whose carried sums the lookup
  // gather reads: those that have children or are an output row, by rising depth
  Table carried_nodes;
  std::vector<int32_t> carried_begin;
  int64_t dims = 0;        // dimensions dim_begin covers (the D of the call it was built for)
  void *d_blob = nullptr;
};

// Every table that goes to the device, with the kernel argument it fills (nullptr: none - the
// alphas go to launch_exp_tables).  upload_tables and the fill of GradArgs walk this list.
struct TableSlot {
  Table GradTables::*table;
  const int32_t *fr::GradArgs::*arg;
};
const TableSlot kDeviceTables[] = {
    {&GradTables::parent_srow, &fr::GradArgs::parent_srow},
    {&GradTables::child_begin, &fr::GradArgs::child_begin},
    {&GradTables::child, &fr::GradArgs::child},
    {&GradTables::fac_begin, &fr::GradArgs::fac_begin},
    {&GradTables::fac, &fr::GradArgs::fac},
    {&GradTables::g_begin, &fr::GradArgs::g_begin},
    {&GradTables::g_row, &fr::GradArgs::g_row},
    {&GradTables::level_nodes, &fr::GradArgs::level_nodes},
    {&GradTables::dim_begin, &fr::GradArgs::dim_begin},
    {&GradTables::dim_item, &fr::GradArgs::dim_item},
    {&GradTables::self_srow, &fr::GradArgs::self_srow},
    {&GradTables::tab, &fr::GradArgs::tab},
    {&GradTables::inner_nodes, &fr::GradArgs::inner_nodes},
    {&GradTables::alpha_bits, nullptr},
    {&GradTables::carried_nodes, nullptr},
};

const char *const kNotWeighted = "the exp factors of a node are not those of a weighted prefix plan";

// The trie behind a plan's DFS order.
struct Trie {
  std::vector<int> parent, depth, srow;
  std::vector<std::vector<int32_t>> kids;
  int deepest = 0;
};

// Trie and parents: an only child continues its parent's frame (F_CHAIN), the other nodes hang
// below the last node of the level above (as in plan.cpp, pieced).
std::string build_trie(const fr::Plan &p, Trie &t) {
  const int V = (int)p.nodes.size();
  t.parent.assign(V, -1);
  t.depth.assign(V, 1);
  t.srow.assign(V, -1);
  t.kids.assign(V, {});
  for (int u = 0; u < p.units(); ++u) {
    int last_at[fr::kMaxLevels + 1];
    for (int &x : last_at) x = -1;
    for (int i = p.unit_begin[u]; i < p.unit_begin[u + 1]; ++i) {
      const fr::NodeDesc &nd = p.nodes[i];
      if (nd.level < 0 || nd.level >= fr::kMaxLevels) return "a node beyond the frame limit";
      t.parent[i] = (nd.flags & fr::F_CHAIN) ? last_at[nd.level] : (nd.level > 0 ? last_at[nd.level - 1] : -1);
      last_at[nd.level] = i;
      if (t.parent[i] >= 0) t.depth[i] = t.depth[t.parent[i]] + 1;
      if (nd.emit_count != 1) return "not a prefix plan: every node has to emit exactly one row";
      t.srow[i] = p.emit_rows[nd.emit_begin];
      if (t.srow[i] < 0 || t.srow[i] >= V) return "an output row outside the plan";
    }
  }
  for (int i = 0; i < V; ++i) {
    if (t.parent[i] >= 0) t.kids[t.parent[i]].push_back(i);
    t.deepest = std::max(t.deepest, t.depth[i]);
  }
  return "";
}

// Letters and factors of node i, appended to g.fac: one factor code per occurrence
// (row | FAC_DIV), the occurrences of a dimension adjacent -> {dimension, exponent}.  Arctic: one
// code per dimension, fac_arctic(row, coefficient) with the coefficient in bits 8-15 ->
// {dimension, coefficient}.  A weighted plan's exp tables among the factors go to g.tab.
std::string build_letter(const fr::Plan &p, int i, int64_t D, GradTables &g,
                         std::vector<std::vector<int32_t>> &items) {
  std::vector<int32_t> &fac = g.fac.h, &tab = g.tab.h;
  const fr::NodeDesc &nd = p.nodes[i];
  const size_t begin = (size_t)g.fac_begin.h.back();
  for (int j = 0; j < nd.fac_count; ++j) {
    const int32_t code = p.factors[nd.fac_begin + j];
    const int row = code & fr::FAC_ROW_MASK;
    if (p.weighting != 0 && p.multiplicative() && row >= p.dims_used && row < (int)p.row_src.size()) {
      // an exp table, not an input dimension (plan.cpp, emit_node): an even table is the
      // node's own exp(+g alpha), an odd one its parent's exp(-g alpha)
      const int table = row - p.dims_used;
      if ((code & fr::FAC_DIV) || tab[3 * i + ((table & 1) ? 2 : 0)] >= 0) return kNotWeighted;
      tab[3 * i + ((table & 1) ? 2 : 0)] = table;
      continue;
    }
    if (row >= (int)p.row_src.size() || p.row_src[row] < 0) return "a factor that is no input dimension";
    const int32_t dim = p.row_src[row];
    if (dim >= D) return "a factor beyond the input's dimensions";
    if (p.semiring == fr::kSemiArctic) {
      fac.push_back(dim);
      fac.push_back((int32_t)(int8_t)((code >> 8) & 0xff));
      continue;
    }
    const int32_t sign = (code & fr::FAC_DIV) ? -1 : 1;
    if (fac.size() > begin * 2 && fac[fac.size() - 2] == dim) {
      fac.back() += sign;
    } else {
      fac.push_back(dim);
      fac.push_back(sign);
    }
  }
  for (size_t f = begin; f < fac.size() / 2; ++f) {
    if (fac[2 * f + 1] == 0) return "a letter with cancelling occurrences of one dimension";
    items[(size_t)fac[2 * f]].push_back(i);
    items[(size_t)fac[2 * f]].push_back((int32_t)f);
  }
  g.fac_begin.h.push_back((int32_t)(fac.size() / 2));
  return "";
}

// The exp tables of node i of a weighted plan: non-total - the weight of the child scan (inner
// nodes only, a leaf needs none); total - the factor among the letters and the weight of the
// emitted row.  A parent comes before its children: its tables are checked by then.
std::string build_exp_tables(const fr::Plan &p, int i, const Trie &t, GradTables &g) {
  const fr::NodeDesc &nd = p.nodes[i];
  int32_t *tb = &g.tab.h[3 * (size_t)i];
  if (p.weighting == 1 && nd.z_mul >= 0) {
    tb[0] = nd.z_mul - p.dims_used;
    tb[1] = tb[0] + 1;
  } else if (p.weighting == 2) {
    tb[1] = nd.emit_mul - p.dims_used;
  }
  const int tables = p.aux_tables(), parent = t.parent[i];
  if (p.weighting == 2 || !t.kids[i].empty())
    if (tb[0] < 0 || tb[0] + 1 >= tables || (tb[0] & 1) || tb[1] != tb[0] + 1) return kNotWeighted;
  if ((parent >= 0) != (tb[2] >= 0) || (parent >= 0 && tb[2] != g.tab.h[3 * (size_t)parent + 1]))
    return kNotWeighted;
  return "";
}

// Level orders (stable: DFS order within a depth): every node by falling depth - the adjoint runs
// leaves first -; a weighted plan's carried sums are formed root first: the nodes that have
// children, by rising depth (the others' are never read).
void build_level_orders(const Trie &t, bool weighted, GradTables &g) {
  const int V = (int)t.depth.size();
  g.level_nodes.h.clear();
  g.level_begin.assign(1, 0);
  for (int dep = t.deepest; dep >= 1; --dep) {
    for (int i = 0; i < V; ++i)
      if (t.depth[i] == dep) g.level_nodes.h.push_back(i);
    g.level_begin.push_back((int32_t)g.level_nodes.h.size());
  }
  g.inner_nodes.h.clear();
  g.inner_begin.assign(1, 0);
  for (int dep = 1; weighted && dep <= t.deepest; ++dep) {
    for (int i = 0; i < V; ++i)
      if (t.depth[i] == dep && !t.kids[i].empty()) g.inner_nodes.h.push_back(i);
    g.inner_begin.push_back((int32_t)g.inner_nodes.h.size());
  }
  g.carried_nodes.h.clear();
  g.carried_begin.assign(1, 0);
  for (int dep = 1; weighted && dep <= t.deepest; ++dep) {
    for (int i = 0; i < V; ++i)
      if (t.depth[i] == dep && (!t.kids[i].empty() || g.g_begin.h[i + 1] > g.g_begin.h[i]))
        g.carried_nodes.h.push_back(i);
    g.carried_begin.push_back((int32_t)g.carried_nodes.h.size());
  }
}

// Builds the host tables of a trie plan of any semiring, unweighted or - Reals - weighted (the
// caller has checked which); "" or what is wrong with the plan / the row map.
std::string build_tables(const fr::Plan &p, const int32_t *row_prefix, int64_t K, int64_t D,
                         GradTables &g) {
  const int V = (int)p.nodes.size();
  if (p.K != V) return "not a prefix plan: every node has to emit exactly one row";
  Trie t;
  std::string why = build_trie(p, t);
  if (!why.empty()) return why;
  std::vector<int> node_of_row(V, -1);
  for (int i = 0; i < V; ++i) {
    if (node_of_row[t.srow[i]] >= 0) return "not a prefix plan: two nodes emit one row";
    node_of_row[t.srow[i]] = i;
  }
  g.parent_srow.h.assign(V, -1);
  g.self_srow.h.assign(t.srow.begin(), t.srow.end());
  for (int i = 0; i < V; ++i)
    if (t.parent[i] >= 0) g.parent_srow.h[i] = t.srow[t.parent[i]];
  std::vector<std::vector<int32_t>> grows(V);
  for (int64_t k = 0; k < K; ++k) {
    if (row_prefix[k] < 0 || row_prefix[k] >= V)
      return "row " + std::to_string(k) + " of the gradient names prefix " +
             std::to_string(row_prefix[k]) + " of " + std::to_string(V);
    grows[node_of_row[row_prefix[k]]].push_back((int32_t)k);
  }
  g.row_prefix.assign(row_prefix, row_prefix + K);
  g.child_begin.h.assign(1, 0);
  g.g_begin.h.assign(1, 0);
  g.fac_begin.h.assign(1, 0);
  g.child.h.clear();
  g.g_row.h.clear();
  g.fac.h.clear();
  std::vector<std::vector<int32_t>> items((size_t)D);
  const bool weighted = p.weighting != 0;
  g.tab.h.assign(weighted ? (size_t)3 * V : 0, -1);
  for (int i = 0; i < V; ++i) {
    g.child.h.insert(g.child.h.end(), t.kids[i].begin(), t.kids[i].end());
    g.child_begin.h.push_back((int32_t)g.child.h.size());
    g.g_row.h.insert(g.g_row.h.end(), grows[i].begin(), grows[i].end());
    g.g_begin.h.push_back((int32_t)g.g_row.h.size());
    why = build_letter(p, i, D, g, items);
    if (why.empty() && weighted) why = build_exp_tables(p, i, t, g);
    if (!why.empty()) return why;
  }
  if (weighted) {
    g.alpha_bits.h.resize(p.alphas.size());
    if (!p.alphas.empty()) std::memcpy(g.alpha_bits.h.data(), p.alphas.data(), p.alphas.size() * 4);
  }
  g.dim_begin.h.assign(1, 0);
  g.dim_item.h.clear();
  for (int64_t d = 0; d < D; ++d) {
    g.dim_item.h.insert(g.dim_item.h.end(), items[(size_t)d].begin(), items[(size_t)d].end());
    g.dim_begin.h.push_back((int32_t)(g.dim_item.h.size() / 2));
  }
  g.dims = D;
  build_level_orders(t, weighted, g);
  return "";
}

// The backward tables of a CosWISS plan (kernels.h, CosGradArgs): the letters as {dimension,
// exponent} pairs, the rows of G of every unit, the units some row names (level_nodes) and per
// input dimension the {row of DZ, factor} pairs of those units' letters - a unit no row names
// is neither launched nor gathered.
std::string build_cos_tables(const fr::Plan &p, const int32_t *row_prefix, int64_t K, int64_t D,
                             GradTables &g) {
  const fr::CosProgram &c = *p.cos;
  const int units = c.W * c.F;
  std::vector<std::vector<int32_t>> grows((size_t)units);
  for (int64_t k = 0; k < K; ++k) {
    if (row_prefix[k] < 0 || row_prefix[k] >= units)
      return "row " + std::to_string(k) + " of the gradient names row " + std::to_string(row_prefix[k]) +
             " of " + std::to_string(units);
    grows[(size_t)row_prefix[k]].push_back((int32_t)k);
  }
  g.row_prefix.assign(row_prefix, row_prefix + K);
  g.fac_begin.h.assign(1, 0);
  g.fac.h.clear();
  const int letters = (int)c.fac_begin.size() - 1;
  for (int l = 0; l < letters; ++l) {
    const size_t begin = g.fac.h.size();
    for (int j = c.fac_begin[l]; j < c.fac_begin[l + 1]; ++j) {
      const int32_t dim = c.factors[j] & fr::FAC_ROW_MASK, sign = (c.factors[j] & fr::FAC_DIV) ? -1 : 1;
      if (dim >= D) return "a factor beyond the input's dimensions";
      if (g.fac.h.size() > begin && g.fac.h[g.fac.h.size() - 2] == dim) {
        g.fac.h.back() += sign;
      } else {
        g.fac.h.push_back(dim);
        g.fac.h.push_back(sign);
      }
    }
    g.fac_begin.h.push_back((int32_t)(g.fac.h.size() / 2));
  }
  g.g_begin.h.assign(1, 0);
  g.g_row.h.clear();
  g.level_nodes.h.clear();
  std::vector<std::vector<int32_t>> items((size_t)D);
  for (int u = 0; u < units; ++u) {
    g.g_row.h.insert(g.g_row.h.end(), grows[(size_t)u].begin(), grows[(size_t)u].end());
    g.g_begin.h.push_back((int32_t)g.g_row.h.size());
    if (grows[(size_t)u].empty()) continue;
    g.level_nodes.h.push_back(u);
    const int w = u / c.F, f = u % c.F;
    for (int l = c.letter_begin[w]; l < c.letter_begin[w + 1]; ++l)
      for (int32_t j = g.fac_begin.h[l]; j < g.fac_begin.h[l + 1]; ++j) {
        items[(size_t)g.fac.h[2 * j]].push_back(l * c.F + f);
        items[(size_t)g.fac.h[2 * j]].push_back(j);
      }
  }
  g.dim_begin.h.assign(1, 0);
  g.dim_item.h.clear();
  for (int64_t d = 0; d < D; ++d) {
    g.dim_item.h.insert(g.dim_item.h.end(), items[(size_t)d].begin(), items[(size_t)d].end());
    g.dim_begin.h.push_back((int32_t)(g.dim_item.h.size() / 2));
  }
  g.dims = D;
  return "";
}

int upload_tables(GradTables &g) {
  size_t size = 0;
  for (const TableSlot &s : kDeviceTables)
    size = align_up(size + (g.*s.table).h.size() * 4 + 4, 64);   // (+ 4: an empty table still has an address)
  std::vector<char> host(size, 0);
  void *d = nullptr;
  HIP_TRY(hipMalloc(&d, host.size()));
  size_t at = 0;
  for (const TableSlot &s : kDeviceTables) {
    Table &t = g.*s.table;
    if (!t.h.empty()) std::memcpy(host.data() + at, t.h.data(), t.h.size() * 4);
    t.d = reinterpret_cast<const int32_t *>(static_cast<char *>(d) + at);
    at = align_up(at + t.h.size() * 4 + 4, 64);
  }
  hipError_t e = hipMemcpy(d, host.data(), host.size(), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(d);
    return hip_fail(e, "hipMemcpy(backward tables)");
  }
  g.d_blob = d;
  return FR_OK;
}

}  // namespace

namespace fr::capi {
void release_grad_tables(fr::Plan &p) {
  GradTables *g = static_cast<GradTables *>(p.grad);
  if (!g) return;
  if (g->d_blob) (void)hipFree(g->d_blob);
  delete g;
  p.grad = nullptr;
}
}  // namespace fr::capi

namespace {

// The plan's backward tables for this row map and D, on the device: those it holds, or fresh
// ones - checked on the host before anything is uploaded or launched.  Caller holds p.mu.  With
// nothing to launch (N == 0 or T == 0) the tables are only checked.
int ensure_tables(fr::Plan &p, const std::string &who, const int32_t *h_row_prefix, int64_t K,
                  int64_t D, bool nothing_to_do, hipStream_t st, GradTables *&g) {
  g = static_cast<GradTables *>(p.grad);
  const bool same = g && g->dims == D && (int64_t)g->row_prefix.size() == K &&
                    (K == 0 || std::memcmp(g->row_prefix.data(), h_row_prefix, (size_t)K * 4) == 0);
  if (same) return FR_OK;
  GradTables fresh;
  const std::string why = p.cos ? build_cos_tables(p, h_row_prefix, K, D, fresh)
                                : build_tables(p, h_row_prefix, K, D, fresh);
  if (!why.empty()) return fail(FR_E_ARG, who + ": " + why);
  if (nothing_to_do) return FR_OK;
  if (stream_is_capturing(st))
    return fail(FR_E_ARG, who + ": the stream is being captured and the backward tables "
                          "are not on the device yet - run one backward pass before the capture");
  int rc = claim_device(p, who.c_str());
  if (rc != FR_OK) return rc;
  if (g) {
    // (kernels of an earlier call may still read the old tables)
    HIP_TRY(hipDeviceSynchronize());
    release_grad_tables(p);
  }
  g = new GradTables(std::move(fresh));
  rc = upload_tables(*g);
  if (rc != FR_OK) {
    delete g;
    g = nullptr;
    return rc;
  }
  p.grad = g;
  return FR_OK;
}

// What an entry brings besides the arguments all share.  `S`: the prefix plan's output
// (fr_iss_backward, fr_iss_backward_max); `lookup`, `C`, `aux`: fr_iss_backward_weighted's;
// `picked`: the upstream is F pairs (`pos`, `w`) per row instead of d_G (fr_iss_backward_picked).
enum class Entry { kReals, kMax, kWeighted };
struct BackwardCall {
  const char *name;
  Entry entry;
  const double *S = nullptr;
  const double *lookup = nullptr;
  int64_t lookup_rows = 0;
  double *C = nullptr, *aux = nullptr;
  bool picked = false;
  const int32_t *pos = nullptr;
  const double *w = nullptr;
  int32_t F = 0;
};

// Why the entry does not take the plan, or nullptr (what a plan is never changes after its
// creation).
const char *refused_plan(Entry entry, const fr::Plan &p) {
  switch (entry) {
    case Entry::kReals:
      if (p.cos || p.weighting != 0 || p.semiring != fr::kSemiReals)
        return "the plan is not an unweighted Reals trie plan";
      return nullptr;
    case Entry::kMax:
      if (p.cos) return "a CosWISS plan has no backward pass";
      if (p.semiring != fr::kSemiArctic && p.semiring != fr::kSemiBayesian)
        return "the plan is a Reals plan - its backward pass is fr_iss_backward";
      if (p.weighting != 0) return "a weighted plan has no backward pass";
      if (p.letter_sum) return "a letter-sum plan (Arctic argmax) has no backward pass";
      return nullptr;
    case Entry::kWeighted:
      if (p.cos) return "a CosWISS plan has no backward pass";
      if (p.semiring != fr::kSemiReals)
        return "the plan is an Arctic or a Bayesian plan - fr_iss_backward_max differentiates the "
               "unweighted ones, a weighted one has no backward pass";
      if (p.weighting == 0)
        return "the plan is an unweighted Reals plan - its backward pass is fr_iss_backward";
      return nullptr;
  }
  return nullptr;
}

// The body of the entries: the refusals in the entry's order, the tables, then - weighted -
// the exp tables and the carried sums root first, the adjoint leaves first, dX.
int run_backward(const BackwardCall &call, fr_plan_t *prefix_plan, const double *d_X, int64_t N, int64_t D,
                 int64_t T, const double *d_G, int64_t K, int64_t g_n_stride, int64_t g_k_stride,
                 int64_t g_t_stride, const int32_t *h_row_prefix, double *d_A, double *d_dX, void *stream) {
  const std::string who = call.name;
  const bool weighted = call.entry == Entry::kWeighted;
  if (!prefix_plan || !prefix_plan->p) return fail(FR_E_ARG, who + ": null plan");
  if (N < 0 || D < 1 || T < 0 || K < 0 || g_n_stride < 0 || g_k_stride < 0 || g_t_stride < 0)
    return fail(FR_E_ARG, who + ": bad shape");
  if (call.picked && call.F < 1) return fail(FR_E_ARG, who + ": a row needs at least one (position, weight) pair");
  if (call.picked && call.F > fr::kPickMaxFeatures)
    return fail(FR_E_LIMIT, who + ": at most 256 pairs per row, not " + std::to_string(call.F));
  if (call.picked && T > 0x7fffffffLL) return fail(FR_E_LIMIT, who + ": positions are 32-bit, T is not");
  if (weighted && call.lookup_rows != 1 && call.lookup_rows != N)
    return fail(FR_E_ARG, who + ": the lookup has to have 1 or N rows, not " + std::to_string(call.lookup_rows));
  if (K > 0 && !h_row_prefix) return fail(FR_E_ARG, who + ": null host table");
  fr::Plan &p = *prefix_plan->p;
  // (the weighted entry names a wrong plan before anything else about it, the others after the
  // pointers: each as it always did)
  const char *refused = refused_plan(call.entry, p);
  if (weighted && refused) return fail(FR_E_ARG, who + ": " + refused);
  if (p.max_dim > D)
    return fail(FR_E_DIM, who + ": a word references dimension " + std::to_string(p.max_dim) +
                              " but the input has only " + std::to_string(D));
  const int64_t V = (int64_t)p.nodes.size();
  if (N > 0 && T > 0) {
    const bool scratch = weighted ? call.C && d_A && call.aux : call.S && d_A;
    const bool upstream = call.picked ? call.pos && call.w : d_G != nullptr;
    if (!d_X || !d_dX || (weighted && !call.lookup) || (K > 0 && !upstream) || (V > 0 && !scratch))
      return fail(FR_E_ARG, who + ": null device pointer");
    if (d_X == d_dX) return fail(FR_E_ARG, who + ": the gradient must not alias the input");
    if (weighted && V > 0 && (call.C == d_A || call.aux == d_A || call.aux == call.C))
      return fail(FR_E_ARG, who + ": the scratches must be distinct buffers");
  }
  if (refused) return fail(FR_E_ARG, who + ": " + refused);
  hipStream_t st = (hipStream_t)stream;
  std::lock_guard<std::mutex> lock(p.mu);
  // (read once: the launches below carry the pointer by value, a setter after this changes nothing)
  const int32_t *lengths = p.grad_lengths;
  if (lengths && p.grad_lengths_n != N)
    return fail(FR_E_ARG, who + ": the lengths were set for " + std::to_string(p.grad_lengths_n) +
                              " series (fr_plan_set_grad_lengths), the call brings " + std::to_string(N));
  // (the same for the path-length lookup: the scratches, the norm and the scale)
  double *const dg = p.grad_pathlen_dg, *const pathlen_r = p.grad_pathlen_r;
  const int pathlen_norm = p.grad_pathlen_norm;
  const double pathlen_scale = p.grad_pathlen_scale;
  if (dg) {
    const std::string armed = who + ": the plan is armed with a path-length lookup (fr_plan_set_grad_pathlen)";
    if (!weighted || call.picked)
      return fail(FR_E_ARG, armed + " - only fr_iss_backward_weighted carries a gradient through it");
    if (lengths)
      return fail(FR_E_ARG, armed + " and with per-series lengths (fr_plan_set_grad_lengths) - the path "
                                    "length of a truncated series is another lookup: clear one of them");
    if (p.grad_pathlen_n != N)
      return fail(FR_E_ARG, who + ": the path-length lookup was set for " + std::to_string(p.grad_pathlen_n) +
                                " series (fr_plan_set_grad_pathlen), the call brings " + std::to_string(N));
    if (call.lookup_rows != N)
      return fail(FR_E_ARG, armed + " - the lookup has to have N rows, one per series, not " +
                                std::to_string(call.lookup_rows));
    const void *others[] = {d_X, d_dX, call.lookup, d_G, call.C, d_A, call.aux};
    for (const void *o : others)
      if (N > 0 && T > 0 && (o == dg || (pathlen_r && o == pathlen_r)))
        return fail(FR_E_ARG, who + ": the path-length scratches (fr_plan_set_grad_pathlen) must be "
                                    "distinct from the call's buffers");
  }
  GradTables *g = nullptr;
  int rc = ensure_tables(p, who, h_row_prefix, K, D, N == 0 || T == 0, st, g);
  if (rc != FR_OK || N == 0 || T == 0) return rc;
  rc = claim_device(p, who.c_str());
  if (rc != FR_OK) return rc;
  fr::GradArgs a{};
  for (const TableSlot &s : kDeviceTables)
    if (s.arg) a.*s.arg = (g->*s.table).d;
  a.N = N;
  a.D = D;
  a.T = T;
  a.X = d_X;
  a.S = call.S;
  a.G = d_G;
  if (call.picked) {
    // (the pairs of row (n, k) at (n * K + k) * F)
    a.pos = call.pos;
    a.w = call.w;
    a.F = call.F;
  }
  a.A = d_A;
  a.dX = d_dX;
  a.len = lengths;
  a.g_n = g_n_stride;
  a.g_k = g_k_stride;
  a.g_t = g_t_stride;
  int kind = fr::kGradReals;
  if (call.entry == Entry::kMax) kind = p.semiring == fr::kSemiArctic ? fr::kGradArctic : fr::kGradBayesian;
  const std::string limit_text = who + ": grid too large (N, N * D or T)";
  const char *limit = limit_text.c_str();
  if (weighted) {
    kind = p.weighting == FR_W_TOTAL ? fr::kGradTotal : fr::kGradNonTotal;
    a.C = call.C;
    a.aux = call.aux;
    a.aux_tab = call.lookup_rows * T;
    a.aux_n = call.lookup_rows == 1 ? 0 : T;
    rc = launched(fr::launch_exp_tables(call.lookup, a.aux_tab, reinterpret_cast<const float *>(g->alpha_bits.d),
                                        (int)p.alphas.size(), call.aux, false, st),
                  "exp_tables launch");
    if (rc != FR_OK) return rc;
    // (armed, total: the lookup gather reads S_v = C_v E-_v of every row - the longer node list)
    const std::vector<int32_t> *carried = &g->inner_begin;
    if (dg) {
      a.R = kind == fr::kGradNonTotal ? pathlen_r : nullptr;
      a.dg = dg;
      a.lookup = call.lookup;
      a.alphas = reinterpret_cast<const float *>(g->alpha_bits.d);
      a.V = (int)V;
      a.norm = pathlen_norm;
      a.scale = pathlen_scale;
      if (kind == fr::kGradTotal) {
        a.inner_nodes = g->carried_nodes.d;
        carried = &g->carried_begin;
      }
    }
    for (size_t l = 0; l + 1 < carried->size(); ++l) {
      const int first = (*carried)[l], count = (*carried)[l + 1] - first;
      rc = launched(fr::launch_grad_prefix(a, kind, first, count, st), "backward prefix launch", limit);
      if (rc != FR_OK) return rc;
    }
  }
  for (size_t l = 0; l + 1 < g->level_begin.size(); ++l) {
    const int first = g->level_begin[l], count = g->level_begin[l + 1] - first;
    rc = launched(call.entry == Entry::kMax ? fr::launch_grad_max_suffix(a, kind, first, count, st)
                                            : fr::launch_grad_suffix(a, kind, first, count, st),
                  "backward suffix launch", limit);
    if (rc != FR_OK) return rc;
  }
  rc = launched(fr::launch_grad_input(a, kind, st), "backward input launch", limit);
  if (rc != FR_OK || !dg) return rc;
  // the gradient through the lookup: dg over the nodes, then through the path length into
  // dX[:, 0, :] - behind the input gather on this stream, so the two additions keep their order
  rc = launched(fr::launch_grad_lookup(a, kind, st), "backward lookup launch", limit);
  if (rc != FR_OK) return rc;
  return launched(fr::launch_grad_pathlen(a, st), "backward path-length launch", limit);
}

// fr_iss_backward with a CosWISS plan: the checks in run_backward's order, the
// tables, the trig rows behind the rows of DZ in d_A, the unit kernel, dX.  d_S takes the
// recomputed u rows: it is written, never read before that.
int run_backward_cos(fr_plan_t *plan, const double *d_X, int64_t N, int64_t D, int64_t T, double *d_S,
                     const double *d_G, int64_t K, int64_t g_n_stride, int64_t g_k_stride, int64_t g_t_stride,
                     const int32_t *h_row_prefix, double *d_A, double *d_dX, void *stream) {
  const std::string who = "fr_iss_backward";
  if (N < 0 || D < 1 || T < 0 || K < 0 || g_n_stride < 0 || g_k_stride < 0 || g_t_stride < 0)
    return fail(FR_E_ARG, who + ": bad shape");
  if (K > 0 && !h_row_prefix) return fail(FR_E_ARG, who + ": null host table");
  fr::Plan &p = *plan->p;
  fr::CosProgram &cp = *p.cos;
  if (p.max_dim > D)
    return fail(FR_E_DIM, who + ": a word references dimension " + std::to_string(p.max_dim) +
                              " but the input has only " + std::to_string(D));
  const int64_t letters = (int64_t)cp.fac_begin.size() - 1;
  const int64_t u_rows = (letters - cp.W) * cp.F, dz_rows = letters * cp.F;
  if (N > 0 && T > 0) {
    if (!d_X || !d_dX || (K > 0 && !d_G) || (u_rows > 0 && !d_S) || (cp.F > 0 && !d_A))
      return fail(FR_E_ARG, who + ": null device pointer");
    if (d_X == d_dX) return fail(FR_E_ARG, who + ": the gradient must not alias the input");
    if (u_rows > 0 && d_S == d_A) return fail(FR_E_ARG, who + ": the scratches must be distinct buffers");
  }
  if (cp.exponent > fr::kCosMaxExponent || p.levels > fr::kCosGradLetters)
    return fail(FR_E_LIMIT, who + ": the CosWISS backward kernels cover exponents <= 8 and words of <= 16 "
                                  "letters");
  if (N > 0x7fffffffLL || N * D > 0x7fffffffLL || (T + 1023) / 1024 > 65535)
    return fail(FR_E_LIMIT, who + ": grid too large (N, N * D or T)");
  if (cp.d_mask)
    return fail(FR_E_ARG, who + ": the CosWISS plan has a dropout mask set - the backward pass has no dropout");
  if (cp.x_unit_stride != 0)
    return fail(FR_E_ARG, who + ": the CosWISS plan has a per-unit input stride (ffn) - the backward pass "
                                "differentiates the plain input alone");
  hipStream_t st = (hipStream_t)stream;
  std::lock_guard<std::mutex> lock(p.mu);
  if (p.grad_lengths)
    return fail(FR_E_ARG, who + ": the plan is armed with per-series lengths (fr_plan_set_grad_lengths) - "
                                "a CosWISS has none: its angle is a function of T");
  GradTables *g = nullptr;
  int rc = ensure_tables(p, who, h_row_prefix, K, D, N == 0 || T == 0, st, g);
  if (rc != FR_OK || N == 0 || T == 0) return rc;
  rc = ensure_cos_program(p, cp, st, who.c_str());
  if (rc != FR_OK) return rc;
  double *trig = d_A + dz_rows * N * T;
  rc = launched(fr::launch_trig_tables(cp.d_freqs, cp.F, T, trig, st), "trig_tables launch");
  if (rc != FR_OK) return rc;
  fr::CosGradArgs a{};
  a.X = d_X;
  a.G = d_G;
  a.trig = trig;
  a.U = d_S;
  a.DZ = d_A;
  a.dX = d_dX;
  a.N = N;
  a.D = D;
  a.T = T;
  a.g_n = g_n_stride;
  a.g_k = g_k_stride;
  a.g_t = g_t_stride;
  a.F = cp.F;
  a.total = cp.total ? 1 : 0;
  a.letter_begin = cp.d_letter_begin;
  a.fac_begin = g->fac_begin.d;
  a.fac = g->fac.d;
  a.g_begin = g->g_begin.d;
  a.g_row = g->g_row.d;
  a.units = g->level_nodes.d;
  a.dim_begin = g->dim_begin.d;
  a.dim_item = g->dim_item.d;
  const std::string limit_text = who + ": grid too large (N, N * D or T)";
  rc = launched(fr::launch_grad_cos_units(a, cp.exponent, 0, (int)g->level_nodes.h.size(), st),
                "backward CosWISS unit launch", limit_text.c_str());
  if (rc != FR_OK) return rc;
  return launched(fr::launch_grad_cos_input(a, st), "backward CosWISS input launch", limit_text.c_str());
}

}  // namespace

extern "C" {

int fr_plan_set_grad_lengths(fr_plan_t *prefix_plan, const int32_t *d_lengths, int64_t N) {
  if (!prefix_plan || !prefix_plan->p) return fail(FR_E_ARG, "fr_plan_set_grad_lengths: null plan");
  if (N < 0) return fail(FR_E_ARG, "fr_plan_set_grad_lengths: bad shape");
  fr::Plan &p = *prefix_plan->p;
  std::lock_guard<std::mutex> lock(p.mu);
  p.grad_lengths = d_lengths;
  p.grad_lengths_n = d_lengths ? N : 0;
  return FR_OK;
}

int fr_plan_set_grad_pathlen(fr_plan_t *prefix_plan, int64_t N, int32_t norm, double scale, double *d_dg,
                             double *d_R) {
  const std::string who = "fr_plan_set_grad_pathlen";
  if (!prefix_plan || !prefix_plan->p) return fail(FR_E_ARG, who + ": null plan");
  fr::Plan &p = *prefix_plan->p;
  if (d_dg) {
    if (N < 0) return fail(FR_E_ARG, who + ": bad shape");
    if (norm != 1 && norm != 2)
      return fail(FR_E_ARG, who + ": the norm has to be 1 (L1) or 2 (L2), not " + std::to_string(norm));
    if (!(scale == scale) || scale - scale != 0.0) return fail(FR_E_ARG, who + ": the scale has to be finite");
    if (p.cos || p.semiring != fr::kSemiReals || p.weighting == 0)
      return fail(FR_E_ARG, who + ": the plan is not a weighted Reals trie plan - only fr_iss_backward_weighted "
                                  "carries a gradient through a lookup");
    if (p.weighting != FR_W_TOTAL && !d_R)
      return fail(FR_E_ARG, who + ": a non-total plan needs the scratch d_R (V, N, T)");
    if (d_R == d_dg) return fail(FR_E_ARG, who + ": the scratches must be distinct buffers");
  }
  std::lock_guard<std::mutex> lock(p.mu);
  p.grad_pathlen_dg = d_dg;
  p.grad_pathlen_r = d_dg ? d_R : nullptr;
  p.grad_pathlen_n = d_dg ? N : 0;
  p.grad_pathlen_norm = d_dg ? norm : 0;
  p.grad_pathlen_scale = d_dg ? scale : 0.0;
  return FR_OK;
}

int fr_iss_backward_weighted(fr_plan_t *prefix_plan, const double *d_X, int64_t N, int64_t D,
                             int64_t T, const double *d_lookup, int64_t lookup_rows,
                             const double *d_G, int64_t K, int64_t g_n_stride, int64_t g_k_stride,
                             int64_t g_t_stride, const int32_t *h_row_prefix, double *d_C,
                             double *d_A, double *d_aux, double *d_dX, void *stream) {
  BackwardCall call{"fr_iss_backward_weighted", Entry::kWeighted};
  call.lookup = d_lookup;
  call.lookup_rows = lookup_rows;
  call.C = d_C;
  call.aux = d_aux;
  return run_backward(call, prefix_plan, d_X, N, D, T, d_G, K, g_n_stride, g_k_stride, g_t_stride,
                      h_row_prefix, d_A, d_dX, stream);
}

int fr_iss_backward(fr_plan_t *prefix_plan, const double *d_X, int64_t N, int64_t D, int64_t T,
                    const double *d_S, const double *d_G, int64_t K, int64_t g_n_stride,
                    int64_t g_k_stride, int64_t g_t_stride, const int32_t *h_row_prefix,
                    double *d_A, double *d_dX, void *stream) {
  // (a CosWISS plan: its own adjoint; d_S is scratch the entry writes)
  if (prefix_plan && prefix_plan->p && prefix_plan->p->cos)
    return run_backward_cos(prefix_plan, d_X, N, D, T, const_cast<double *>(d_S), d_G, K, g_n_stride,
                            g_k_stride, g_t_stride, h_row_prefix, d_A, d_dX, stream);
  return run_backward({"fr_iss_backward", Entry::kReals, d_S}, prefix_plan, d_X, N, D, T, d_G, K,
                      g_n_stride, g_k_stride, g_t_stride, h_row_prefix, d_A, d_dX, stream);
}

int fr_iss_backward_max(fr_plan_t *prefix_plan, const double *d_X, int64_t N, int64_t D, int64_t T,
                        const double *d_S, const double *d_G, int64_t K, int64_t g_n_stride,
                        int64_t g_k_stride, int64_t g_t_stride, const int32_t *h_row_prefix,
                        double *d_A, double *d_dX, void *stream) {
  return run_backward({"fr_iss_backward_max", Entry::kMax, d_S}, prefix_plan, d_X, N, D, T, d_G, K,
                      g_n_stride, g_k_stride, g_t_stride, h_row_prefix, d_A, d_dX, stream);
}

int fr_iss_backward_picked(fr_plan_t *prefix_plan, const double *d_X, int64_t N, int64_t D, int64_t T,
                           const double *d_S, const double *d_lookup, int64_t lookup_rows,
                           const int32_t *d_pos, const double *d_w, int64_t K, int32_t F,
                           const int32_t *h_row_prefix, double *d_C, double *d_A, double *d_aux,
                           double *d_dX, void *stream) {
  // the plan's kind names the adjoint, as the three dense entries name it themselves
  BackwardCall call{"fr_iss_backward_picked", Entry::kReals};
  if (prefix_plan && prefix_plan->p) {
    const fr::Plan &p = *prefix_plan->p;
    if (p.cos) return fail(FR_E_ARG, std::string(call.name) + ": a CosWISS plan has no backward pass");
    if (p.weighting != 0)
      call.entry = Entry::kWeighted;
    else if (p.semiring != fr::kSemiReals)
      call.entry = Entry::kMax;
  }
  if (call.entry == Entry::kWeighted) {
    call.lookup = d_lookup;
    call.lookup_rows = lookup_rows;
    call.C = d_C;
    call.aux = d_aux;
  } else {
    call.S = d_S;
  }
  call.picked = true;
  call.pos = d_pos;
  call.w = d_w;
  call.F = F;
  const int64_t row = F > 0 ? (int64_t)F : 0;   // (run_backward names a bad F itself)
  return run_backward(call, prefix_plan, d_X, N, D, T, nullptr, K, K * row, row, 0, h_row_prefix, d_A,
                      d_dX, stream);
}

}  // extern "C"
