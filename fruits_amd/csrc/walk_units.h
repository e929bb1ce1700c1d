// Which unit a workgroup of a trie walk runs.  A unit is (series n, group g of root sub-tries);
// every kernel decodes it from a unit index u in [0, N * G) - its workgroup index, or what a
// persistent grid strides over - with the functions below, and nothing else does.  Pure and free
// of host includes: device code (run-time compiled programs included: this file is part of their
// source text) and a CPU test (tests/native/walk_units_host.cpp: every (n, g) of a launch is
// produced exactly once, whatever N, G, the grid and the split of a mixed launch are).
#pragma once
#include "walk_types.h"   // FR_HOST_DEVICE

namespace fr {

struct WalkUnit {
  int64_t n;   // series
  int g;       // group of root sub-tries
};

// Plain numbering: the G groups of a series are consecutive units.
FR_HOST_DEVICE inline WalkUnit walk_unit_plain(int u, int G) {
  const int n = u / G;
  return WalkUnit{n, u - n * G};
}

// XCD-aware numbering, for N % 8 == 0: workgroups are dealt round-robin over the 8 XCDs, so the
// eight units 8 q ... 8 q + 7 are group q % G of the eight series 8 (q / G) ... + 7 - the groups
// of one series meet in one XCD's L2 (speed only; at another N it would name series >= N).
FR_HOST_DEVICE inline WalkUnit walk_unit_xcd(int u, int G) {
  const int q = u >> 3, r = u & 7;
  return WalkUnit{(int64_t)(q / G) * 8 + r, q % G};
}

FR_HOST_DEVICE inline WalkUnit walk_unit(int u, int G, bool xcd) {
  return xcd ? walk_unit_xcd(u, G) : walk_unit_plain(u, G);
}

// The series alone: the interpreter touches the rows of its NEXT unit while it runs this one.
// (Written out, like walk_tail_unit below: through walk_unit the compiler orders the same
// instructions differently.  The CPU test holds both to walk_unit.)
FR_HOST_DEVICE inline int64_t walk_unit_series(int u, int G, bool xcd) {
  return xcd ? (int64_t)((u >> 3) / G) * 8 + (u & 7) : (int64_t)(u / G);
}

// Mixed static launch: workgroup j behind the n_whole whole-series ones.  The last S = N - n_whole
// series run as GT finer units each, XCD-aware where S % 8 == 0 (the host launches exactly
// n_whole + GT * S workgroups).
FR_HOST_DEVICE inline WalkUnit walk_tail_unit(int j, int GT, int n_whole, int S) {
  if (S % 8 == 0) {
    const int q = j >> 3, r = j & 7;
    return WalkUnit{n_whole + (int64_t)(q / GT) * 8 + r, q % GT};
  }
  return WalkUnit{n_whole + j / GT, j % GT};
}

// Wave-per-series kernels: a workgroup holds `teams` waves with a unit each; team `team` of
// workgroup `block` of `grid` runs the units packed_first_unit, + packed_unit_stride, ... < N * G
// (the last workgroup's surplus teams find none), numbered plainly.
FR_HOST_DEVICE inline int64_t packed_first_unit(int64_t block, int teams, int team) {
  return block * teams + team;
}
FR_HOST_DEVICE inline int64_t packed_unit_stride(int64_t grid, int teams) { return grid * teams; }
FR_HOST_DEVICE inline WalkUnit packed_unit(int64_t u, int G) {
  return WalkUnit{u / G, (int)(u % G)};
}

}  // namespace fr
