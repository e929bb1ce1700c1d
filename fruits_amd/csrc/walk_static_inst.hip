// Walk kernels whose program is a compile-time constant (walk.h, walk_static).  One
// translation unit per pre-generated program (STATIC_PROG = its index in
// static_programs.h, fruits_amd/gen_static.py), plus the registry (STATIC_REGISTRY) that
// capi_plan.cpp asks whether the plan it is about to run is one of them.
#include "walk.h"

#include <cstring>

#include "static_programs.h"

namespace fr {

#define SP_CAT2(a, b) a##b
#define SP_CAT(a, b) SP_CAT2(a, b)

#ifdef STATIC_REGISTRY
#define SP_DECL(i) hipError_t walk_static_launch_##i(const IssArgs &, hipStream_t);
SP_DECL(0) SP_DECL(1) SP_DECL(2) SP_DECL(3) SP_DECL(4) SP_DECL(5) SP_DECL(6) SP_DECL(7) SP_DECL(8) SP_DECL(9) SP_DECL(10) SP_DECL(11) SP_DECL(12) SP_DECL(13) SP_DECL(14) SP_DECL(15) SP_DECL(16) SP_DECL(17) SP_DECL(18) SP_DECL(19) SP_DECL(20) SP_DECL(21) SP_DECL(22)
static_assert(kStaticPrograms == 23, "list the generated programs above and below");

// index -> program, so that a program can name its tail program (StaticProgN::tail) by index
template <int I>
struct StaticProgAt {
  using type = void;
};
#define SP_AT(i) template <> struct StaticProgAt<i> { using type = StaticProg##i; };
SP_AT(0) SP_AT(1) SP_AT(2) SP_AT(3) SP_AT(4) SP_AT(5) SP_AT(6) SP_AT(7) SP_AT(8) SP_AT(9) SP_AT(10) SP_AT(11) SP_AT(12) SP_AT(13) SP_AT(14) SP_AT(15) SP_AT(16) SP_AT(17) SP_AT(18) SP_AT(19) SP_AT(20) SP_AT(21) SP_AT(22)

// The mixed launch of a one-group program and its tail program (walk_device.h,
// iss_walk_static_kernel<C, PG, PGT>): whole series in front, the tail program's finer units
// behind.  It exists where the one-group program runs with non-temporal input and sc1 stores
// (cache-sized batches), so it is built with that store policy only; it lives here, where
// the programs know of each other - a program's own translation unit holds its two instances.
template <int I>
hipError_t walk_static_launch_mixed(const IssArgs &a, hipStream_t st) {
  using PG = typename StaticProgAt<I>::type;
  if constexpr (PG::groups == 1 && PG::tail >= 0) {
    using PGT = typename StaticProgAt<PG::tail>::type;
    return launch_walk_static<WalkCfg<2, 2, 2, 0, true, false, 4, 0, 0, false, false, false, kStoreSc1>, PG, PGT>(a, st);
  } else {
    return hipErrorInvalidValue;
  }
}

struct StaticEntry {
  const int32_t *src;
  const int32_t *row_src;   // staged row -> input dimension: part of the program's identity
  int n_src, rows, groups;
  int tail;                 // index of the tail program (the same plan in finer units) or -1
  hipError_t (*launch)(const IssArgs &, hipStream_t);
  hipError_t (*launch_mixed)(const IssArgs &, hipStream_t);
};
#define SP_ENTRY(i) {StaticProg##i::src, StaticProg##i::row_src, StaticProg##i::n_src, StaticProg##i::rows, StaticProg##i::groups, StaticProg##i::tail, walk_static_launch_##i, walk_static_launch_mixed<i>}
static const StaticEntry kStaticTable[kStaticPrograms] = {
    SP_ENTRY(0), SP_ENTRY(1), SP_ENTRY(2), SP_ENTRY(3), SP_ENTRY(4), SP_ENTRY(5), SP_ENTRY(6), SP_ENTRY(7), SP_ENTRY(8), SP_ENTRY(9), SP_ENTRY(10), SP_ENTRY(11), SP_ENTRY(12), SP_ENTRY(13), SP_ENTRY(14), SP_ENTRY(15), SP_ENTRY(16), SP_ENTRY(17), SP_ENTRY(18), SP_ENTRY(19), SP_ENTRY(20), SP_ENTRY(21), SP_ENTRY(22)};

// 1 + index of the static program for `groups` groups per series whose interpreter records
// (one group) equal `recs` AND whose staged rows come from the same input dimensions (the
// records name LDS rows; `[4]` alone has the records of `[1]` alone), or 0
int static_program_for(const NodeRec *recs, int n, int groups, const int32_t *row_src, int rows) {
  for (int i = 0; i < kStaticPrograms; ++i)
    if (groups == kStaticTable[i].groups && n == kStaticTable[i].n_src &&
        rows == kStaticTable[i].rows &&
        std::memcmp(row_src, kStaticTable[i].row_src, (size_t)rows * 4) == 0 &&
        std::memcmp(recs, kStaticTable[i].src, (size_t)n * 64) == 0)
      return i + 1;
  return 0;
}

// groups per series of the tail program of static program `prog` (1 + index), 0: it has none
int static_program_tail_groups(int prog) {
  if (prog < 1 || prog > kStaticPrograms || kStaticTable[prog - 1].tail < 0) return 0;
  return kStaticTable[kStaticTable[prog - 1].tail].groups;
}

// materialising, one aligned 1024-element chunk, unweighted Reals; a.n_whole < a.N: the mixed
// launch with the program's tail program
hipError_t walk_static_launch(const IssArgs &a, hipStream_t st) {
  if (a.static_prog < 1 || a.static_prog > kStaticPrograms ||
      kStaticTable[a.static_prog - 1].groups != a.G)
    return hipErrorInvalidValue;
  if (a.n_whole < a.N) return kStaticTable[a.static_prog - 1].launch_mixed(a, st);
  return kStaticTable[a.static_prog - 1].launch(a, st);
}
#else
// Two instances per program: plain output stores, and the cache policy that the program's group
// count was measured to gain from in the window where the host asks for it (IssArgs::wt,
// capi_walk.cpp run_walk): one group (cache-sized batches, non-temporal input) writes through the L2
// (sc1); three groups (batches that stream through HBM, plain input loads shared by the sibling
// groups) write through and non-temporal (nt sc1).  Two-group programs keep plain stores only.
template <int G>
constexpr int static_store_policy() {
  return G == 1 ? kStoreSc1 : (G == 3 ? kStoreNtSc1 : kStorePlain);
}
// (the mixed launch of a one-group program with its tail program: the registry, above)

hipError_t SP_CAT(walk_static_launch_, STATIC_PROG)(const IssArgs &a, hipStream_t st) {
  using PG = SP_CAT(StaticProg, STATIC_PROG);
  constexpr int wt = static_store_policy<PG::groups>();
  if constexpr (wt != kStorePlain) {
    if (a.wt) return launch_walk_static<WalkCfg<2, 2, 2, 0, true, false, 4, 0, 0, false, false, false, wt>, PG>(a, st);
  }
  return launch_walk_static<WalkCfg<2, 2, 2, 0, true, false, 4, 0, 0>, PG>(a, st);
}
#endif

}  // namespace fr
