// fr_iss_backward: the gradient of unweighted Reals iterated sums with respect to their input;
// fr_iss_backward_max: the same for the max semirings Arctic and Bayesian;
// fr_iss_backward_weighted: the same for weighted Reals plans, total or not.  The trie - parents,
// children, letters, exp tables - is read off the plan the plan compiler built (plan.cpp); the
// kernels are those of kernels_grad.hip.
#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "capi_common.h"
#include "kernels.h"

using namespace fr::capi;

namespace {

// The backward tables of a prefix plan: host copies, one device blob.  The trie part is a
// function of the plan; the rows of G a node gathers are the caller's (`row_prefix`), kept to
// see whether a later call brings the same.
struct GradTables {
  std::vector<int32_t> row_prefix;
  std::vector<int32_t> parent_srow, child_begin, child, fac_begin, fac, g_begin, g_row,
      level_nodes, level_begin, dim_begin, dim_item, self_srow;
  // a weighted plan's: per node the exp tables {own E+, own E-, parent's E-} (-1: unused), the
  // nodes that have children by rising depth, and the bits of the plan's distinct alphas
  std::vector<int32_t> tab, inner_nodes, inner_begin, alpha_bits;
  int64_t dims = 0;        // dimensions dim_begin covers (the D of the call it was built for)
  void *d_blob = nullptr;
  const int32_t *d_parent_srow = nullptr, *d_child_begin = nullptr, *d_child = nullptr,
                *d_fac_begin = nullptr, *d_fac = nullptr, *d_g_begin = nullptr, *d_g_row = nullptr,
                *d_level_nodes = nullptr, *d_dim_begin = nullptr, *d_dim_item = nullptr,
                *d_self_srow = nullptr, *d_tab = nullptr, *d_inner_nodes = nullptr,
                *d_alpha_bits = nullptr;
};

// Builds the host tables of a trie plan of any semiring, unweighted or - Reals - weighted (the
// caller has checked which); "" or what is wrong with the plan / the row map.
std::string build_tables(const fr::Plan &p, const int32_t *row_prefix, int64_t K, int64_t D,
                         GradTables &g) {
  const int V = (int)p.nodes.size();
  if (p.K != V) return "not a prefix plan: every node has to emit exactly one row";
  // the trie behind the DFS order: an only child continues its parent's frame (F_CHAIN), the
  // other nodes hang below the last node of the level above (as in plan.cpp, pieced)
  std::vector<int> parent(V, -1), depth(V, 1), srow(V, -1);
  for (int u = 0; u < p.units(); ++u) {
    int last_at[fr::kMaxLevels + 1];
    for (int &x : last_at) x = -1;
    for (int i = p.unit_begin[u]; i < p.unit_begin[u + 1]; ++i) {
      const fr::NodeDesc &nd = p.nodes[i];
      if (nd.level < 0 || nd.level >= fr::kMaxLevels) return "a node beyond the frame limit";
      parent[i] = (nd.flags & fr::F_CHAIN) ? last_at[nd.level] : (nd.level > 0 ? last_at[nd.level - 1] : -1);
      last_at[nd.level] = i;
      if (parent[i] >= 0) depth[i] = depth[parent[i]] + 1;
      if (nd.emit_count != 1) return "not a prefix plan: every node has to emit exactly one row";
      srow[i] = p.emit_rows[nd.emit_begin];
      if (srow[i] < 0 || srow[i] >= V) return "an output row outside the plan";
    }
  }
  std::vector<int> node_of_row(V, -1);
  for (int i = 0; i < V; ++i) {
    if (node_of_row[srow[i]] >= 0) return "not a prefix plan: two nodes emit one row";
    node_of_row[srow[i]] = i;
  }
  g.parent_srow.assign(V, -1);
  g.self_srow.assign(srow.begin(), srow.end());
  std::vector<std::vector<int32_t>> kids(V), grows(V);
  for (int i = 0; i < V; ++i)
    if (parent[i] >= 0) {
      g.parent_srow[i] = srow[parent[i]];
      kids[parent[i]].push_back(i);
    }
  for (int64_t k = 0; k < K; ++k) {
    if (row_prefix[k] < 0 || row_prefix[k] >= V)
      return "row " + std::to_string(k) + " of the gradient names prefix " +
             std::to_string(row_prefix[k]) + " of " + std::to_string(V);
    grows[node_of_row[row_prefix[k]]].push_back((int32_t)k);
  }
  g.row_prefix.assign(row_prefix, row_prefix + K);
  g.child_begin.assign(1, 0);
  g.g_begin.assign(1, 0);
  g.fac_begin.assign(1, 0);
  g.child.clear();
  g.g_row.clear();
  g.fac.clear();
  std::vector<std::vector<int32_t>> items((size_t)D);
  const bool weighted = p.weighting != 0;
  g.tab.assign(weighted ? (size_t)3 * V : 0, -1);
  const std::string not_weighted = "the exp factors of a node are not those of a weighted prefix plan";
  for (int i = 0; i < V; ++i) {
    g.child.insert(g.child.end(), kids[i].begin(), kids[i].end());
    g.child_begin.push_back((int32_t)g.child.size());
    g.g_row.insert(g.g_row.end(), grows[i].begin(), grows[i].end());
    g.g_begin.push_back((int32_t)g.g_row.size());
    // the letter: one factor code per occurrence (row | FAC_DIV), the occurrences of a
    // dimension adjacent -> {dimension, exponent}.  Arctic: one code per dimension,
    // fac_arctic(row, coefficient) with the coefficient in bits 8-15 -> {dimension, coefficient}
    const fr::NodeDesc &nd = p.nodes[i];
    for (int j = 0; j < nd.fac_count; ++j) {
      const int32_t code = p.factors[nd.fac_begin + j];
      const int row = code & fr::FAC_ROW_MASK;
      if (weighted && p.multiplicative() && row >= p.dims_used && row < (int)p.row_src.size()) {
        // an exp table, not an input dimension (plan.cpp, emit_node): an even table is the
        // node's own exp(+g alpha), an odd one its parent's exp(-g alpha)
        const int table = row - p.dims_used;
        if ((code & fr::FAC_DIV) || g.tab[3 * i + ((table & 1) ? 2 : 0)] >= 0) return not_weighted;
        g.tab[3 * i + ((table & 1) ? 2 : 0)] = table;
        continue;
      }
      if (row >= (int)p.row_src.size() || p.row_src[row] < 0) return "a factor that is no input dimension";
      const int32_t dim = p.row_src[row];
      if (dim >= D) return "a factor beyond the input's dimensions";
      if (p.semiring == fr::kSemiArctic) {
        g.fac.push_back(dim);
        g.fac.push_back((int32_t)(int8_t)((code >> 8) & 0xff));
        continue;
      }
      const int32_t sign = (code & fr::FAC_DIV) ? -1 : 1;
      const size_t begin = (size_t)g.fac_begin.back() * 2;
      if (g.fac.size() > begin && g.fac[g.fac.size() - 2] == dim) {
        g.fac.back() += sign;
      } else {
        g.fac.push_back(dim);
        g.fac.push_back(sign);
      }
    }
    for (size_t f = (size_t)g.fac_begin.back(); f < g.fac.size() / 2; ++f) {
      if (g.fac[2 * f + 1] == 0) return "a letter with cancelling occurrences of one dimension";
      items[(size_t)g.fac[2 * f]].push_back(i);
      items[(size_t)g.fac[2 * f]].push_back((int32_t)f);
    }
    g.fac_begin.push_back((int32_t)(g.fac.size() / 2));
    if (weighted) {
      // the node's own tables: non-total - the weight of the child scan (inner nodes only, a
      // leaf needs none); total - the factor above and the weight of the emitted row
      int32_t *tb = &g.tab[3 * (size_t)i];
      if (p.weighting == 1 && nd.z_mul >= 0) {
        tb[0] = nd.z_mul - p.dims_used;
        tb[1] = tb[0] + 1;
      } else if (p.weighting == 2) {
        tb[1] = nd.emit_mul - p.dims_used;
      }
      const int tables = p.aux_tables();
      const bool inner = !kids[i].empty();
      if (p.weighting == 2 || inner)
        if (tb[0] < 0 || tb[0] + 1 >= tables || (tb[0] & 1) || tb[1] != tb[0] + 1) return not_weighted;
      // (a parent comes before its children: its tables are checked by now)
      if ((parent[i] >= 0) != (tb[2] >= 0) || (parent[i] >= 0 && tb[2] != g.tab[3 * (size_t)parent[i] + 1]))
        return not_weighted;
    }
  }
  if (weighted) {
    g.alpha_bits.resize(p.alphas.size());
    if (!p.alphas.empty()) std::memcpy(g.alpha_bits.data(), p.alphas.data(), p.alphas.size() * 4);
  }
  g.dim_begin.assign(1, 0);
  g.dim_item.clear();
  for (int64_t d = 0; d < D; ++d) {
    g.dim_item.insert(g.dim_item.end(), items[(size_t)d].begin(), items[(size_t)d].end());
    g.dim_begin.push_back((int32_t)(g.dim_item.size() / 2));
  }
  g.dims = D;
  // the nodes by falling depth (stable: DFS order within a depth)
  int deepest = 0;
  for (int i = 0; i < V; ++i) deepest = std::max(deepest, depth[i]);
  g.level_nodes.clear();
  g.level_begin.assign(1, 0);
  for (int dep = deepest; dep >= 1; --dep) {
    for (int i = 0; i < V; ++i)
      if (depth[i] == dep) g.level_nodes.push_back(i);
    g.level_begin.push_back((int32_t)g.level_nodes.size());
  }
  // a weighted plan's carried sums are formed root first: the nodes that have children, by
  // rising depth (the others' are never read)
  g.inner_nodes.clear();
  g.inner_begin.assign(1, 0);
  for (int dep = 1; weighted && dep <= deepest; ++dep) {
    for (int i = 0; i < V; ++i)
      if (depth[i] == dep && !kids[i].empty()) g.inner_nodes.push_back(i);
    g.inner_begin.push_back((int32_t)g.inner_nodes.size());
  }
  return "";
}

int upload_tables(GradTables &g) {
  const std::vector<int32_t> *parts[] = {&g.parent_srow, &g.child_begin, &g.child, &g.fac_begin, &g.fac,
                                         &g.g_begin, &g.g_row, &g.level_nodes, &g.dim_begin, &g.dim_item,
                                         &g.self_srow, &g.tab, &g.inner_nodes, &g.alpha_bits};
  const int32_t **dst[] = {&g.d_parent_srow, &g.d_child_begin, &g.d_child, &g.d_fac_begin, &g.d_fac,
                           &g.d_g_begin, &g.d_g_row, &g.d_level_nodes, &g.d_dim_begin, &g.d_dim_item,
                           &g.d_self_srow, &g.d_tab, &g.d_inner_nodes, &g.d_alpha_bits};
  constexpr int kParts = 14;
  size_t off = 0, at[kParts];
  for (int i = 0; i < kParts; ++i) {
    at[i] = off;
    off = align_up(off + parts[i]->size() * 4 + 4, 64);   // (+ 4: an empty table still has an address)
  }
  std::vector<char> host(off, 0);
  for (int i = 0; i < kParts; ++i)
    if (!parts[i]->empty()) std::memcpy(host.data() + at[i], parts[i]->data(), parts[i]->size() * 4);
  void *d = nullptr;
  HIP_TRY(hipMalloc(&d, host.size()));
  hipError_t e = hipMemcpy(d, host.data(), host.size(), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(d);
    return hip_fail(e, "hipMemcpy(backward tables)");
  }
  g.d_blob = d;
  for (int i = 0; i < kParts; ++i) *dst[i] = reinterpret_cast<const int32_t *>(static_cast<char *>(d) + at[i]);
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
  const std::string why = build_tables(p, h_row_prefix, K, D, fresh);
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

// The kernel arguments that are the tables' and the shape's.
fr::GradArgs table_args(const GradTables &g, int64_t N, int64_t D, int64_t T) {
  fr::GradArgs a{};
  a.N = N;
  a.D = D;
  a.T = T;
  a.parent_srow = g.d_parent_srow;
  a.child_begin = g.d_child_begin;
  a.child = g.d_child;
  a.fac_begin = g.d_fac_begin;
  a.fac = g.d_fac;
  a.g_begin = g.d_g_begin;
  a.g_row = g.d_g_row;
  a.level_nodes = g.d_level_nodes;
  a.dim_begin = g.d_dim_begin;
  a.dim_item = g.d_dim_item;
  a.self_srow = g.d_self_srow;
  return a;
}

// The body of both entries.  `max_plus`: fr_iss_backward_max - the plan has to be an Arctic or
// a Bayesian one, and the kernels are the segmented ones.
int run_backward(const std::string &who, bool max_plus, fr_plan_t *prefix_plan, const double *d_X,
                 int64_t N, int64_t D, int64_t T, const double *d_S, const double *d_G, int64_t K,
                 int64_t g_n_stride, int64_t g_k_stride, int64_t g_t_stride,
                 const int32_t *h_row_prefix, double *d_A, double *d_dX, void *stream) {
  if (!prefix_plan || !prefix_plan->p) return fail(FR_E_ARG, who + ": null plan");
  if (N < 0 || D < 1 || T < 0 || K < 0 || g_n_stride < 0 || g_k_stride < 0 || g_t_stride < 0)
    return fail(FR_E_ARG, who + ": bad shape");
  if (K > 0 && !h_row_prefix) return fail(FR_E_ARG, who + ": null host table");
  fr::Plan &p = *prefix_plan->p;
  if (p.max_dim > D)
    return fail(FR_E_DIM, who + ": a word references dimension " + std::to_string(p.max_dim) +
                              " but the input has only " + std::to_string(D));
  const int64_t V = (int64_t)p.nodes.size();
  if (N > 0 && T > 0) {
    if (!d_X || !d_dX || (K > 0 && !d_G) || (V > 0 && (!d_S || !d_A)))
      return fail(FR_E_ARG, who + ": null device pointer");
    if (d_X == d_dX) return fail(FR_E_ARG, who + ": the gradient must not alias the input");
  }
  // which plans an entry takes (what a plan is never changes after its creation)
  const char *kind = nullptr;
  if (!max_plus) {
    if (p.cos || p.weighting != 0 || p.semiring != fr::kSemiReals)
      kind = "the plan is not an unweighted Reals trie plan";
  } else if (p.cos) {
    kind = "a CosWISS plan has no backward pass";
  } else if (p.semiring != fr::kSemiArctic && p.semiring != fr::kSemiBayesian) {
    kind = "the plan is a Reals plan - its backward pass is fr_iss_backward";
  } else if (p.weighting != 0) {
    kind = "a weighted plan has no backward pass";
  } else if (p.letter_sum) {
    kind = "a letter-sum plan (Arctic argmax) has no backward pass";
  }
  if (kind) return fail(FR_E_ARG, who + ": " + kind);
  hipStream_t st = (hipStream_t)stream;
  std::lock_guard<std::mutex> lock(p.mu);
  GradTables *g = nullptr;
  int rc = ensure_tables(p, who, h_row_prefix, K, D, N == 0 || T == 0, st, g);
  if (rc != FR_OK || N == 0 || T == 0) return rc;
  rc = claim_device(p, who.c_str());
  if (rc != FR_OK) return rc;
  fr::GradArgs a = table_args(*g, N, D, T);
  a.X = d_X;
  a.S = d_S;
  a.G = d_G;
  a.A = d_A;
  a.dX = d_dX;
  a.g_n = g_n_stride;
  a.g_k = g_k_stride;
  a.g_t = g_t_stride;
  const std::string limit_text = who + ": grid too large (N, N * D or T)";
  const char *limit = limit_text.c_str();
  for (size_t l = 0; l + 1 < g->level_begin.size(); ++l) {
    const int first = g->level_begin[l], count = g->level_begin[l + 1] - first;
    rc = launched(max_plus ? fr::launch_grad_max_suffix(a, p.semiring, first, count, st)
                           : fr::launch_grad_suffix(a, first, count, st),
                  "backward suffix launch", limit);
    if (rc != FR_OK) return rc;
  }
  return launched(max_plus ? fr::launch_grad_max_input(a, p.semiring, st) : fr::launch_grad_input(a, st),
                  "backward input launch", limit);
}

// fr_iss_backward_weighted: the exp tables, the carried sums root first, the adjoint leaves first.
int run_backward_weighted(fr_plan_t *prefix_plan, const double *d_X, int64_t N, int64_t D, int64_t T,
                          const double *d_lookup, int64_t lookup_rows, const double *d_G, int64_t K,
                          int64_t g_n_stride, int64_t g_k_stride, int64_t g_t_stride,
                          const int32_t *h_row_prefix, double *d_C, double *d_A, double *d_aux,
                          double *d_dX, void *stream) {
  const std::string who = "fr_iss_backward_weighted";
  if (!prefix_plan || !prefix_plan->p) return fail(FR_E_ARG, who + ": null plan");
  if (N < 0 || D < 1 || T < 0 || K < 0 || g_n_stride < 0 || g_k_stride < 0 || g_t_stride < 0)
    return fail(FR_E_ARG, who + ": bad shape");
  if (lookup_rows != 1 && lookup_rows != N)
    return fail(FR_E_ARG, who + ": the lookup has to have 1 or N rows, not " + std::to_string(lookup_rows));
  if (K > 0 && !h_row_prefix) return fail(FR_E_ARG, who + ": null host table");
  fr::Plan &p = *prefix_plan->p;
  // which plans the entry takes (what a plan is never changes after its creation)
  const char *kind = nullptr;
  if (p.cos)
    kind = "a CosWISS plan has no backward pass";
  else if (p.semiring != fr::kSemiReals)
    kind = "the plan is an Arctic or a Bayesian plan - fr_iss_backward_max differentiates the "
           "unweighted ones, a weighted one has no backward pass";
  else if (p.weighting == 0)
    kind = "the plan is an unweighted Reals plan - its backward pass is fr_iss_backward";
  if (kind) return fail(FR_E_ARG, who + ": " + kind);
  if (p.max_dim > D)
    return fail(FR_E_DIM, who + ": a word references dimension " + std::to_string(p.max_dim) +
                              " but the input has only " + std::to_string(D));
  const int64_t V = (int64_t)p.nodes.size();
  if (N > 0 && T > 0) {
    if (!d_X || !d_dX || !d_lookup || (K > 0 && !d_G) || (V > 0 && (!d_C || !d_A || !d_aux)))
      return fail(FR_E_ARG, who + ": null device pointer");
    if (d_X == d_dX) return fail(FR_E_ARG, who + ": the gradient must not alias the input");
    if (V > 0 && (d_C == d_A || d_aux == d_A || d_aux == d_C))
      return fail(FR_E_ARG, who + ": the scratches must be distinct buffers");
  }
  hipStream_t st = (hipStream_t)stream;
  std::lock_guard<std::mutex> lock(p.mu);
  GradTables *g = nullptr;
  int rc = ensure_tables(p, who, h_row_prefix, K, D, N == 0 || T == 0, st, g);
  if (rc != FR_OK || N == 0 || T == 0) return rc;
  rc = claim_device(p, who.c_str());
  if (rc != FR_OK) return rc;
  const int64_t count = lookup_rows * T;
  rc = launched(fr::launch_exp_tables(d_lookup, count, reinterpret_cast<const float *>(g->d_alpha_bits),
                                      (int)p.alphas.size(), d_aux, false, st),
                "exp_tables launch");
  if (rc != FR_OK) return rc;
  fr::GradWArgs w{};
  w.g = table_args(*g, N, D, T);
  w.g.X = d_X;
  w.g.G = d_G;
  w.g.A = d_A;
  w.g.dX = d_dX;
  w.g.g_n = g_n_stride;
  w.g.g_k = g_k_stride;
  w.g.g_t = g_t_stride;
  w.C = d_C;
  w.aux = d_aux;
  w.aux_tab = count;
  w.aux_n = lookup_rows == 1 ? 0 : T;
  w.tab = g->d_tab;
  w.inner_nodes = g->d_inner_nodes;
  const bool total = p.weighting == FR_W_TOTAL;
  const std::string limit_text = who + ": grid too large (N, N * D or T)";
  const char *limit = limit_text.c_str();
  for (size_t l = 0; l + 1 < g->inner_begin.size(); ++l) {
    const int first = g->inner_begin[l], n_nodes = g->inner_begin[l + 1] - first;
    rc = launched(fr::launch_grad_w_prefix(w, first, n_nodes, st), "backward prefix launch", limit);
    if (rc != FR_OK) return rc;
  }
  for (size_t l = 0; l + 1 < g->level_begin.size(); ++l) {
    const int first = g->level_begin[l], n_nodes = g->level_begin[l + 1] - first;
    rc = launched(fr::launch_grad_w_suffix(w, total, first, n_nodes, st), "backward suffix launch", limit);
    if (rc != FR_OK) return rc;
  }
  return launched(fr::launch_grad_w_input(w, total, st), "backward input launch", limit);
}

}  // namespace

extern "C" {

int fr_iss_backward_weighted(fr_plan_t *prefix_plan, const double *d_X, int64_t N, int64_t D,
                             int64_t T, const double *d_lookup, int64_t lookup_rows,
                             const double *d_G, int64_t K, int64_t g_n_stride, int64_t g_k_stride,
                             int64_t g_t_stride, const int32_t *h_row_prefix, double *d_C,
                             double *d_A, double *d_aux, double *d_dX, void *stream) {
  return run_backward_weighted(prefix_plan, d_X, N, D, T, d_lookup, lookup_rows, d_G, K, g_n_stride,
                               g_k_stride, g_t_stride, h_row_prefix, d_C, d_A, d_aux, d_dX, stream);
}

int fr_iss_backward(fr_plan_t *prefix_plan, const double *d_X, int64_t N, int64_t D, int64_t T,
                    const double *d_S, const double *d_G, int64_t K, int64_t g_n_stride,
                    int64_t g_k_stride, int64_t g_t_stride, const int32_t *h_row_prefix,
                    double *d_A, double *d_dX, void *stream) {
  return run_backward("fr_iss_backward", false, prefix_plan, d_X, N, D, T, d_S, d_G, K, g_n_stride,
                      g_k_stride, g_t_stride, h_row_prefix, d_A, d_dX, stream);
}

int fr_iss_backward_max(fr_plan_t *prefix_plan, const double *d_X, int64_t N, int64_t D, int64_t T,
                        const double *d_S, const double *d_G, int64_t K, int64_t g_n_stride,
                        int64_t g_k_stride, int64_t g_t_stride, const int32_t *h_row_prefix,
                        double *d_A, double *d_dX, void *stream) {
  return run_backward("fr_iss_backward_max", true, prefix_plan, d_X, N, D, T, d_S, d_G, K,
                      g_n_stride, g_k_stride, g_t_stride, h_row_prefix, d_A, d_dX, stream);
}

}  // extern "C"
