// How a trie walk is launched: choose_walk_launch, ONE pure function from facts (the plan, the
// shape, what the device and the registry report) and knobs (the environment, read by capi_core.cpp
// once per call) to a choice.  Host-only and free of HIP, so that a CPU test pins the choice
// (tests/native/launch_choice_host.cpp); capi_walk.cpp gathers the facts and carries the choice out.
#pragma once
#include <algorithm>
#include <climits>
#include <cstdint>
#include <functional>

#include "plan.h"
#include "walk_types.h"

namespace fr {

inline int walk_chunk_elems(int64_t T) { return T <= 512 ? 512 : 1024; }

// short series: four series per workgroup, one wave each (walk_packed.h)
inline bool packed_supported(int64_t T, int levels, int semiring) {
  (void)semiring;  // all three semirings are instantiated
  // measured against the cooperative kernel: T = 300 138 -> 88 us, T = 384 143 -> 100 us;
  // beyond (4 pieces per wave, 8 elements per lane) it is no faster (T = 512: 73 vs 79 us)
  return (T <= 256 && levels <= 8) || (T <= 384 && levels <= 4);
}

// The developer knobs of FRUITS_HIP_DEBUG (capi_core.cpp, debug_knob) and the environment switches a
// launch reads; the defaults are what an empty environment gives.
constexpr int kKnobUnset = INT_MIN;
struct WalkKnobs {
  int groups = 0, persist = kKnobUnset, packed = 1, lean = 1, wt = 1, tail = -1;
  int static_cache_x100 = 140, static_min_T = 384;
  int hip_static = 1, hip_jit = 1;   // FRUITS_HIP_STATIC, FRUITS_HIP_JIT
  int stamps = 0, dbg_bytes = 0;     // (the diagnostic timing build's: no part of the choice)
};

// What the choice needs beyond the plan.
struct WalkFacts {
  int64_t N = 0, T = 0;
  int groups = 0;            // asked for by the caller (<= 0: the host chooses)
  bool fused = false;        // features instead of the tensor
  bool total_inc = false;    // fused: a differencing sieve on a totally weighted plan
  int carry_per_node = 3;    // fused: chunk-carry slots of a node (3, + 2 per differencing order >= 3)
  bool vec_ok = false;       // 16-byte accesses of input and output are aligned
  int64_t resident = 0;      // one round of workgroups of the cooperative kernel; 0: not asked
  int aot[4] = {0, 0, 0, 0}; // [g]: the ahead-of-time static program for g groups per series (0: none)
  bool jit[4] = {false, false, false, false};   // [g]: a run-time compiled one is loaded on this device
  int tail_groups = 0;       // groups per series of the tail program of aot[1] (0: it has none)
  // one round of workgroups of the mixed instance of aot[1] (0: unknown) - a dry run of the
  // launcher, asked at most once and only inside the cache-sized window
  std::function<int64_t()> mixed_resident;
  std::function<int(int)> largest_group;   // records of the largest group of the node order for G groups
};

// (struct WalkChoice, what choose_walk_launch returns: plan.h - a plan keeps its most recent one)

inline int choose_groups(const Plan &p, int64_t N, int requested, const WalkKnobs &k) {
  const int U = p.units();
  if (U <= 1) return 1;
  int G = requested;
  if (G <= 0) G = k.groups;
  if (G <= 0) {
    // aim for a few thousand workgroups (256 CUs x several resident each)
    const int64_t target = 2048;
    G = (int)((target + N - 1) / (N > 0 ? N : 1));
  }
  if (G > U) G = U;
  if (G < 1) G = 1;
  return G;
}

// The part of the choice that needs no device: the same for a run, fr_plan_prepare and the
// pipeline's compilers.
struct LaunchShape {
  bool packed = false;    // wave-per-series kernel (short series)
  bool fits = true;       // the staged rows of one time chunk fit the LDS
  int G = 1;              // groups of root sub-tries per series
};

inline bool staged_rows_fit(const Plan &p, int64_t T) {
  return (size_t)p.rows_staged() * walk_chunk_elems(T) * 8 <= 150 * 1024;
}

inline LaunchShape launch_shape(const Plan &p, int64_t N, int64_t T, int requested_groups,
                                const WalkKnobs &k) {
  LaunchShape s;
  s.fits = staged_rows_fit(p, T);
  // short series: four series per workgroup, one wave each (their rows side by side in LDS)
  const int64_t packed_chunk = T <= 128 ? 128 : (T <= 256 ? 256 : 384);
  s.packed = k.packed != 0 && packed_supported(T, p.levels, p.semiring) &&
             (size_t)4 * p.rows_staged() * packed_chunk * 8 <= 64 * 1024;
  // (a packed workgroup holds four units: ask for four times the units)
  s.G = choose_groups(p, s.packed ? (N + 3) / 4 : N, requested_groups, k);
  return s;
}

// LDS carry slots of a multi-chunk walk: 3 per record of the program (nodes + one sentinel
// per group); sized for up to kSpanGroupsMax groups so that the kernel's LDS footprint -
// and with it the number of resident workgroups the group choice is made for - does not
// depend on the choice itself
constexpr int kSpanGroupsMax = 12;
inline int carry_slots_for(const Plan &p, int G) {
  return 3 * ((int)p.nodes.size() + std::max(G, kSpanGroupsMax));
}
inline bool carries_fit_lds(const Plan &p, int64_t T, int G) {
  // rows + carries must leave room for >= 4 workgroups per CU (160 KiB LDS)
  const size_t rows_bytes = (size_t)p.rows_staged() * walk_chunk_elems(T) * 8;
  return rows_bytes + (size_t)carry_slots_for(p, G) * 8 <= 40 * 1024;
}

inline int largest_group(const GroupedProgram &gp) {   // in records (nodes + the sentinel)
  int most = 0;
  for (int g = 0; g < gp.groups; ++g) most = std::max(most, gp.group_begin[g + 1] - gp.group_begin[g]);
  return most;
}

// LDS feature window of a fused cooperative launch (walk_device.h, feat_flush): as many slots
// as fit next to the rows and carries while four workgroups still share a CU's 160 KiB, at
// least what the widest node needs (output rows x feature ops).  `fits`: every group's
// features fit, so a unit flushes once.  0: the widest node does not fit the LDS at all.
// (widest: the slots one node needs; largest_group: the slots of the largest unit)
inline int feat_window_sized(int widest, int largest_group, size_t other_lds_bytes, bool mpi, bool &fits) {
  const size_t budget = 38 * 1024;
  int W = 64;
  while (W < 1024 && W < largest_group &&
         other_lds_bytes + feat_window_bytes(2 * W, mpi) <= budget)
    W *= 2;
  if (W < widest) W = (widest + 1) / 2 * 2;
  if (other_lds_bytes + feat_window_bytes(W, mpi) > 160 * 1024) return 0;
  fits = largest_group <= W;
  return W;
}
inline int feat_window_for(const GroupedProgram &gp, size_t other_lds_bytes, int n_ops, bool mpi,
                           bool &fits) {
  int widest = 0, largest_group = 0;
  for (int g = 0; g < gp.groups; ++g) {
    int total = 0;
    for (int i = gp.group_begin[g]; i < gp.group_begin[g + 1]; ++i) {
      if ((gp.recs[i].w[0] & 0xff) == kRecSentinelLevel) continue;
      const int need = gp.recs[i].w[6] * n_ops;
      widest = std::max(widest, need);
      total += need;
    }
    largest_group = std::max(largest_group, total);
  }
  return feat_window_sized(widest, largest_group, other_lds_bytes, mpi, fits);
}

// Groups per series for the cooperative kernel (walk.h): a unit is (series, group of root
// sub-tries) and stages the series' rows itself, so groups only pay where finer units help.
// Measured on config 2 and its 48-word tiling (tools/gpu_sched.sh: FRUITS_HIP_GROUPS = 1, 2,
// 3, 6, 9 against N = 64 ... 8192, `resident` = one round of workgroups, 1536 for these
// kernels):
//   N < resident        the batch alone cannot fill the chip: ceil(resident / N) groups, at
//                       most 6 (N = 64: G = 6 7.5 us vs 15.7 with 1; 256: 3; 512: 3; 768 and
//                       1000: 2)
//   N < 2 x resident    whole series (N = 1536: 41.7 us, G = 3 46.9; N = 2048: 64.5, G = 3 73.2)
//   beyond              small plans (<= 32 nodes): 3 groups - finer units even out the last
//                       rounds and their restaging hits the XCD's L2 (N = 4096: 135.5 vs
//                       146.6 us, N = 8192: 272 vs 291 us); larger plans keep whole series
//                       (config 3 / 4 / 5: no difference measured)
inline int choose_groups_walk(const Plan &p, int64_t N, int64_t T, int64_t resident, bool fused,
                              const WalkKnobs &k) {
  const int U = p.units();
  if (U <= 1 || N <= 0) return 1;
  if (resident <= 0) return choose_groups(p, N, 0, k);
  if (N < resident) {
    const int64_t G = std::min<int64_t>((resident + N - 1) / N, 6);
    return (int)std::max<int64_t>(1, std::min<int64_t>(G, U));
  }
  // fused launches run one short-lived workgroup per unit (choose_walk_launch): two groups per
  // series balance a little better than whole series on LONG plans (config 4, 1351 nodes: 13.08 vs
  // 13.32 ms); on shorter ones every extra unit is one more staging of the series' rows - the
  // word shards of config 4 over 8 ranks (~170 nodes each): 1.86 ms with whole series, 2.40 ms
  // with two groups (tools/bench_shards.py)
  // (round 3, the pipeline's own kernels: one-chunk plans of 668 / 683 nodes - two word shards of
  // config 4 - 4.74 / 4.84 ms with whole series, 5.47 / 5.48 ms with two groups; 1351 nodes: 9.53
  // vs 9.35 ms; config 5, 511 nodes over four time chunks - two groups also halve the LDS carries
  // of a unit: 17.8 vs 17.3 ms)
  if (fused)
    return p.nodes.size() >= (T > walk_chunk_elems(T) ? 400u : 1000u) ? std::min(U, 2) : 1;
  // materialising launches of long plans run one short-lived workgroup per unit too (the lean
  // walk, choose_walk_launch): two groups per series shorten the last round (of_weight(4,2),
  // N = 2048: 390 -> 372 us; the same at N = 8192) for one more staging of the series' rows
  if (!p.letter_sum && p.nodes.size() >= 64 && k.lean != 0) return std::min(U, 2);
  if (N < 2 * resident || p.nodes.size() > 32) return 1;
  return std::min(U, 3);
}

// batches below this many series run a static program with all its groups (to fill the chip)
constexpr int kStaticSplitBelow = 768;

// (T in (384, 512]: the 1024-element chunk with half of its lanes idle - still ahead of the
// interpreter's 512-element chunk on cache-sized batches, see choose_walk_launch)
inline bool static_shape_ok(const Plan &p, int64_t T, const WalkKnobs &k) {
  return !p.cos && p.weighting == 0 && p.semiring == kSemiReals && T > k.static_min_T && T <= 1024;
}

// input + output bytes of a materialising launch
inline double walk_footprint_bytes(const Plan &p, int64_t N, int64_t T) {
  return 8.0 * (double)N * (double)T * (double)(p.dims_used + p.K);
}
constexpr double kInfinityCacheBytes = 256.0 * 1024.0 * 1024.0;

// (a totally weighted plan with differencing sieves runs the cooperative kernels, which have
// the instantiation for it, also on short series)
inline bool walk_is_packed(const LaunchShape &shape, bool total_inc) { return shape.packed && !total_inc; }
// The host chooses the groups of a cooperative launch that nobody asked a count for, from one
// resident round of its kernel: these are the launches WalkFacts::resident is asked for.
inline bool host_chooses_groups(bool packed, int requested, const WalkKnobs &k) {
  return !packed && requested <= 0 && k.groups <= 0;
}

// A static program may run this launch (if the plan has one): the only launches that look for one.
inline bool static_launch_possible(const Plan &p, const WalkFacts &f, const WalkKnobs &k) {
  const bool packed = walk_is_packed(launch_shape(p, f.N, f.T, f.groups, k), f.total_inc);
  return !f.fused && !packed && f.vec_ok && static_shape_ok(p, f.T, k) && f.N > 0 &&
         (f.groups > 0 ? f.groups : k.groups) <= 3 && k.hip_static != 0;
}

// The launch of (plan, facts) under `k`: shape -> static program -> groups -> kernel family ->
// grid policy -> tail; every field of the choice is assigned once.
inline WalkChoice choose_walk_launch(const Plan &p, const WalkFacts &f, const WalkKnobs &k) {
  WalkChoice c;
  const int64_t N = f.N, T = f.T, chunk = walk_chunk_elems(T);
  const LaunchShape shape = launch_shape(p, N, T, f.groups, k);
  c.packed = walk_is_packed(shape, f.total_inc);
  const bool auto_groups = host_chooses_groups(c.packed, f.groups, k);
  const int asked = f.groups > 0 ? f.groups : k.groups;
  const double footprint = walk_footprint_bytes(p, N, T);

  // A pre-compiled static program (walk_static_inst.hip) runs plans whose records equal one
  // of the standard word sets': materialising, one aligned 1024-element chunk, unweighted
  // Reals, the group count its schedule was generated for.  It reads no device tables, so
  // nothing is uploaded for it (and a run of it is capturable without fr_plan_prepare).
  // No ahead-of-time program: one compiled at run time (capi_plan.cpp, ensure_jit) where this device
  // has it loaded.
  const bool static_ok = static_launch_possible(p, f, k);
  const bool aot = f.aot[1] > 0;
  auto have = [&](int g) { return f.aot[g] > 0 || (!aot && f.jit[g]); };
  // Groups per series.  Small batches: as many groups as the schedule has, to fill the
  // chip.  Batches whose input + output are at most 1.4 x the 256 MiB Infinity Cache: ONE
  // group - every input row is then read once, with non-temporal loads that do not
  // allocate in that cache, where the input would only evict output lines (config 2:
  // 69 -> 56 us).  Larger batches stream through HBM whatever is done; there the
  // finer units balance better (N = 8192: 273 vs 283 us).
  // (round 4, tools/static_window.py, fraction of 8 TB/s, one group + nt / three groups /
  // no static program: N = 2048 (1.31 x the cache) 0.763 / 0.654 / 0.656; 2304 (1.48 x)
  // 0.637 / 0.679 / 0.623; 3072 (1.97 x) 0.638 / 0.712 / 0.675; 4096 0.719 / 0.713 / 0.680 -
  // the window used to end at 2 x, where the sweep showed the static program behind the
  // walk without one)
  const int gmax = have(3) ? 3 : (have(2) ? 2 : 1);
  c.cache_sized = static_ok && N >= kStaticSplitBelow &&
                  footprint <= 0.01 * k.static_cache_x100 * kInfinityCacheBytes;
  // (tail=S: the one-group program with its tail program at any N - see the mixed launch below)
  const bool tail_forced = k.tail > 0 && asked <= 0 && aot && f.tail_groups > 0;
  const int static_groups = !static_ok ? 0 : tail_forced ? 1 : asked > 0 ? asked : (c.cache_sized ? 1 : gmax);
  // Batches that stream through HBM (beyond twice the cache): FOUR resident workgroups per
  // CU instead of six - fewer concurrent write streams suit the memory system better
  // (N = 4096 / 8192 / 16384: 134 -> 122, 263 -> 241, 525 -> 493 us); 16 KB of unused LDS
  // per workgroup is how a launch asks for that.  Cache-sized and small batches keep six
  // (N = 2048: 56.2 vs 58.6 us with four).
  // (the pad follows the shape, not the program: a launch of such a shape that ends on the
  // interpreter or the lean walk - T <= 512 beyond the cache - carries it too)
  c.lds_pad = (static_ok && !c.cache_sized && N >= kStaticSplitBelow) ? 16384 : 0;
  // Series of 385 ... 512 elements fill half of the program's 1024-element chunk: measured
  // (round 4, of_weight(2,3), fraction of 8 TB/s, interpreter with its 512-element chunk /
  // static program) T = 512: N = 2048 0.572 / 0.625, 4096 0.567 / 0.744, 8192 (streams through
  // HBM) 0.641 / 0.538; T = 400: 0.506 / 0.594, 0.559 / 0.736, 0.503 / 0.443 - the program on
  // cache-sized batches only
  c.static_prog = !(static_ok && have(static_groups) && (T > 512 || c.cache_sized)) ? 0
                  : f.aot[static_groups] > 0 ? f.aot[static_groups] : -1;
  // Cache policy of the output stores (walk_static_inst.hip: sc1 for one group, nt sc1 for
  // three).  A plain store leaves its line dirty in the XCD's 4 MiB L2 and the launch ends
  // with a write-back of up to 32 MiB that nothing overlaps; a write-through store sends the
  // bytes out during the body.  Measured (of_weight(2,3), T = 1024, back-to-back us, plain ->
  // policy, same box, three rounds): one group + nt input, N = 1536 40.5 -> 39.4, 2048
  // 57.4 -> 54.8 (nt sc1 there: 64.8); three groups, N = 3072 93.5 -> 79.3, 8192 248 -> 193
  // (sc1 there: 91.4, 245; at N = 2048 three groups + nt sc1 reach 61.3, behind one group).
  // So: one group in the cache-sized window, three groups where the batch streams through
  // HBM; small batches (unmeasured) and two-group programs keep plain stores.
  // FRUITS_HIP_DEBUG wt=0 turns it off (A/B of one build).
  c.wt = (c.static_prog > 0 && k.wt != 0 &&
          ((static_groups == 1 && c.cache_sized) || (static_groups == 3 && c.lds_pad != 0))) ? 1 : 0;

  // (clamped like fr::grouped clamps what it lays out)
  const int G = c.static_prog ? static_groups
                              : (auto_groups ? choose_groups_walk(p, N, T, f.resident, f.fused, k) : shape.G);
  c.G = std::max(1, std::min(G, std::max(1, p.units())));

  // Materialising launches of the interpreter's plans run through the fused walk's node loop with
  // a store epilogue (walk_fused.h, MODE 2: half the instructions per node) whenever that walk
  // covers the plan: chunk carries in LDS, no letter sums (Arctic argmax).
  // (short plans on batches of less than two resident rounds keep the interpreter's persistent
  // grid and its prefetch of the next unit's rows: of_weight(2,3) at N = 2048 66 vs 75 us)
  const int64_t round = f.resident > 0 ? f.resident : 1536;
  const bool two_rounds = N * (int64_t)c.G >= 2 * round;
  const bool lean_shape = !f.fused && !c.packed && !c.static_prog && !p.letter_sum && k.lean != 0 &&
                          (p.nodes.size() > 32 || two_rounds);
  const bool fused_coop = f.fused && !c.packed;
  const int most = (lean_shape || fused_coop) ? f.largest_group(c.G) : 0;
  c.lean = (lean_shape && (T <= chunk ||
                           ((size_t)p.rows_staged() * chunk + 24 + 3 * (size_t)most) * 8 <= 40 * 1024)) ? 1 : 0;
  // chunk carries: the lean and the fused walk keep them in LDS, three (fused: carry_per_node)
  // slots per record of the largest group; the interpreter where they fit
  c.carry_per_node = fused_coop ? f.carry_per_node : 3;
  c.carry_slots = (c.lean || fused_coop) ? c.carry_per_node * most : carry_slots_for(p, c.G);
  c.carry_in_lds = (c.lean || fused_coop || carries_fit_lds(p, T, c.G)) ? 1 : 0;

  // Persistent grid (one resident round of workgroups striding over the units) or one
  // short-lived workgroup per unit.  Measured (tools/gpu_persist.sh, gpu_static2.sh): the fused
  // kernels gain 3-12 % from the hardware dispatcher's balancing (config 4: 25.1 -> 22.1 ms,
  // config 5: 42.6 -> 37.3 ms); the materialising interpreter keeps the persistent grid up
  // to two resident rounds (config 2: 68.9 vs 73.7 us) and drops it beyond (N = 8192:
  // 287 -> 256 us).
  // wave-per-series kernels (short series), materialising: T <= 128 without the persistent
  // grid (16384 x 128: 86 -> 77 us, 32768 x 64: 120 -> 100 us), longer ones with (8192 x 256:
  // 71 vs 75 us)
  // static programs of several groups run one short-lived workgroup per unit: the hardware
  // dispatcher balances them and keeps the write front compact; so does the
  // lean walk
  const int by_shape = f.fused ? 0 : (c.packed ? (T > 192 ? 1 : 0) : (two_rounds ? 0 : 1));
  c.persistent = (c.static_prog || c.lean) ? 0 : (k.persist != kKnobUnset ? k.persist : by_shape);
  c.xcd_map = (c.G > 1 && N % 8 == 0) ? 1 : 0;
  // The interpreter's share of the non-temporal input loads, in the window where it was measured
  // to pay: one group per series and a batch just above the Infinity Cache (1 to 1.5 times its
  // 256 MiB - config 2: 70 -> 65 us; 264 MB: 43 -> 45 us, 440 MB: 88 -> 93 us, so not there).
  c.nt_input = (!f.fused && !c.packed && c.G == 1 && footprint > kInfinityCacheBytes &&
                footprint <= 1.5 * kInfinityCacheBytes) ? 1 : 0;

  // The mixed launch (walk_device.h, iss_walk_static_kernel<C, PG, PGT>): a batch of between one
  // and two resident rounds R of whole-series workgroups ends in a partial round whose workgroups
  // live as long as those of the full one, on a chip that empties around them (DESIGN.md 4.1:
  // N = 2048, R = 1536 - the second half of the span at a third of the occupancy).  The first R
  // series run as whole-series units as before; the other N - R run as the finer units of the
  // plan's multi-group program, at the end of the grid.  R is what the launcher reports for the
  // mixed instance on this device.  Ahead-of-time programs in the cache-sized window only.
  // NOT MEASURED YET (DESIGN.md 4.1 says how): expected from the node cost, 54.7 -> 39-47 us at
  // N = 2048 unless the drain of the Infinity Cache (about 48 us for 302 MB) caps it.
  // FRUITS_HIP_DEBUG tail=0 turns it off (A/B of one build); tail=S runs the last min(S, N)
  // series as finer units at any N (tests at small shapes).
  const bool tail_ok = c.static_prog > 0 && c.G == 1 && k.tail != 0 && f.tail_groups > 0 && N <= 0x7fffffff;
  const int64_t R = (tail_ok && k.tail < 0 && c.cache_sized && c.wt != 0) ? f.mixed_resident() : 0;
  c.tail_series = !tail_ok ? 0 : k.tail > 0 ? std::min<int64_t>(k.tail, N)
                                            : (R > 0 && R < N && N < 2 * R) ? N - R : 0;
  c.n_whole = (int32_t)(std::min<int64_t>(N, 0x7fffffff) - c.tail_series);
  return c;
}

// The family of kernels that the choice `c` names; a fused launch that the pipeline's own
// run-time compiled kernels took over is kWalkFusedJit / kWalkFusedPieces (capi_walk.cpp).
inline int walk_family(const WalkChoice &c, bool fused) {
  if (fused) return c.packed ? kWalkFusedPacked : kWalkFused;
  if (c.packed) return kWalkPacked;
  if (c.static_prog) return c.static_prog > 0 ? kWalkStaticAot : kWalkStaticJit;
  return c.lean ? kWalkLean : kWalkInterpreter;
}

// FR_INFO_LAST_LAUNCH: the launch as one word (0: the plan has not run a walk).  From bit 0:
// family (4 bits), G (8), persistent (4), xcd_map, nt_input, wt, an LDS pad was asked for,
// carry_in_lds (1 each); from bit 21 the resident round of the group choice and from bit 41 that
// of the mixed instance (20 bits each, 0: not asked).  Counts beyond their field read as its
// largest value.  tail_series and n_whole have words of their own (FR_INFO_STATIC_TAIL,
// FR_INFO_LAST_WHOLE): a batch may hold 2^31 series.
inline int64_t pack_last_launch(const LastLaunch &l) {
  auto field = [](int64_t v, int bits) { return std::max<int64_t>(0, std::min<int64_t>(v, (int64_t(1) << bits) - 1)); };
  const WalkChoice &c = l.choice;
  if (l.family == kWalkNone) return 0;
  return field(l.family, 4) | field(c.G, 8) << 4 | field(c.persistent, 4) << 12 |
         int64_t(c.xcd_map != 0) << 16 | int64_t(c.nt_input != 0) << 17 | int64_t(c.wt != 0) << 18 |
         int64_t(c.lds_pad != 0) << 19 | int64_t(c.carry_in_lds != 0) << 20 |
         field(l.resident, 20) << 21 | field(l.mixed_resident, 20) << 41;
}
// (the fields pack_last_launch keeps; lds_pad reads 1 where a pad was asked for)
inline LastLaunch unpack_last_launch(int64_t w) {
  LastLaunch l;
  l.family = (int)(w & 15);
  l.choice.G = (int)(w >> 4 & 255);
  l.choice.persistent = (int)(w >> 12 & 15);
  l.choice.xcd_map = (int)(w >> 16 & 1);
  l.choice.nt_input = (int)(w >> 17 & 1);
  l.choice.wt = (int)(w >> 18 & 1);
  l.choice.lds_pad = (int)(w >> 19 & 1);
  l.choice.carry_in_lds = (int)(w >> 20 & 1);
  l.resident = w >> 21 & 0xfffff;
  l.mixed_resident = w >> 41 & 0xfffff;
  return l;
}

}  // namespace fr
