// Host-only check of the walk kernels' unit decode (fruits_amd/csrc/walk_units.h - the functions
// the kernels themselves call), built by tests/test_host.py::test_walk_units_host - plainly, and with
// -fsanitize=address,undefined.  For every launch shape it walks the unit indices the way the
// kernel's workgroups do and counts how often every (series n, group g) comes out: exactly once
// for n < N, g < G, and nothing else.
//   strided loops (static programs of several groups, interpreter): workgroup b of `grid` runs
//     u = b, b + grid, ... < N * G; the interpreter also decodes the series of u + grid ahead;
//   one workgroup per unit (lean and fused walk, static programs): the same with grid = N * G;
//   mixed static launch: workgroups [0, n_whole) are whole series, the other GT * (N - n_whole)
//     the tail program's units;
//   wave-per-series kernels: TEAMS units per workgroup.
// XCD-aware numbering only where the host sets it (N % 8 == 0; the tail decides by S % 8 itself).
// The decode does not depend on the grid, so EVERY grid 1 ... 2 N G is walked for N <= 32 and a
// set around the powers of two, the resident rounds and N G itself for the larger N: what a grid
// can add is an index loop that skips or repeats u, which no N changes.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../fruits_amd/csrc/walk_units.h"

namespace {

long long checked = 0;
std::vector<int> seen;

void reset(int64_t N, int G) { seen.assign((size_t)(N * G), 0); }

bool mark(fr::WalkUnit w, int64_t N, int G, const char *what, long long a, long long b, long long c) {
  if (w.n < 0 || w.n >= N || w.g < 0 || w.g >= G) {
    printf("%s (%lld, %lld, %lld): unit (n=%lld, g=%d) outside N=%lld, G=%d\n", what, a, b, c,
           (long long)w.n, w.g, (long long)N, G);
    return false;
  }
  ++seen[(size_t)(w.n * G + w.g)];
  return true;
}

bool all_once(int64_t N, int G, const char *what, long long a, long long b, long long c) {
  for (int64_t n = 0; n < N; ++n)
    for (int g = 0; g < G; ++g)
      if (seen[(size_t)(n * G + g)] != 1) {
        printf("%s (%lld, %lld, %lld): unit (n=%lld, g=%d) produced %d times\n", what, a, b, c,
               (long long)n, g, seen[(size_t)(n * G + g)]);
        return false;
      }
  ++checked;
  return true;
}

// the strided loop of a persistent grid (grid = N * G: one workgroup per unit)
bool strided(int N, int G, int grid, bool xcd) {
  const int u_end = N * G;
  reset(N, G);
  for (int b = 0; b < grid && b < u_end; ++b)
    for (int u = b; u < u_end; u += grid) {
      if (!mark(fr::walk_unit(u, G, xcd), N, G, xcd ? "strided xcd" : "strided plain", N, G, grid)) return false;
      const int un = u + grid;   // the interpreter's prefetch of its next unit's rows
      if (un < u_end) {
        const int64_t n_next = fr::walk_unit_series(un, G, xcd);
        if (n_next < 0 || n_next >= N || n_next != fr::walk_unit(un, G, xcd).n) {
          printf("next unit (%d, %d, %d): series %lld of unit %d\n", N, G, grid, (long long)n_next, un);
          return false;
        }
      }
    }
  return all_once(N, G, xcd ? "strided xcd" : "strided plain", N, G, grid);
}

bool mixed(int N, int n_whole, int GT) {
  const int S = N - n_whole;
  // whole series count as one unit each here: slot (n, 0); the tail's units as (n, g)
  seen.assign((size_t)N * GT, 0);
  for (int b = 0; b < n_whole + GT * S; ++b) {
    if (b < n_whole) {
      for (int g = 0; g < GT; ++g) ++seen[(size_t)b * GT + g];   // the one-group program: all of it
    } else {
      const fr::WalkUnit w = fr::walk_tail_unit(b - n_whole, GT, n_whole, S);
      const fr::WalkUnit same = fr::walk_unit(b - n_whole, GT, S % 8 == 0);
      if (w.n != same.n + n_whole || w.g != same.g) {
        printf("mixed (%d, %d, %d): workgroup %d is not walk_unit's unit\n", N, n_whole, GT, b);
        return false;
      }
      if (w.n < n_whole) {
        printf("mixed (%d, %d, %d): tail unit in the whole part (n=%lld)\n", N, n_whole, GT, (long long)w.n);
        return false;
      }
      if (!mark(w, N, GT, "mixed", N, n_whole, GT)) return false;
    }
  }
  return all_once(N, GT, "mixed", N, n_whole, GT);
}

bool packed(int64_t N, int G, int teams, int64_t grid) {
  reset(N, G);
  const int64_t units = N * G;
  for (int64_t block = 0; block < grid; ++block)
    for (int team = 0; team < teams; ++team)
      for (int64_t u = fr::packed_first_unit(block, teams, team); u < units;
           u += fr::packed_unit_stride(grid, teams))
        if (!mark(fr::packed_unit(u, G), N, G, "packed", N, G, grid)) return false;
  return all_once(N, G, "packed", N, G, grid);
}

}  // namespace

int main() {
  std::vector<int> Ns;
  for (int N = 1; N <= 600; ++N) Ns.push_back(N);
  for (int N : {1535, 1536, 1537, 1544, 3071, 3072, 3073, 3080}) Ns.push_back(N);
  for (int N : Ns)
    for (int G = 1; G <= 12; ++G) {
      const int U = N * G;
      std::vector<int> grids;
      if (N <= 32) {
        for (int grid = 1; grid <= 2 * U; ++grid) grids.push_back(grid);
      } else {
        for (int grid : {1, 7, 8, 9, 256, 1536, U / 2 + 1, U - 8, U - 1, U, U + 1, 2 * U})
          if (grid >= 1) grids.push_back(grid);
      }
      for (int grid : grids) {
        if (!strided(N, G, grid, false)) return 1;
        if (N % 8 == 0 && !strided(N, G, grid, true)) return 1;
      }
    }
  // the mixed launch: every split of every N, with the group counts of the tail programs
  for (int N : Ns)
    for (int GT = 2; GT <= 3; ++GT) {
      if (N > 600 && GT != 3) continue;
      for (int n_whole = 0; n_whole <= N; ++n_whole)
        if (!mixed(N, n_whole, GT)) return 1;
    }
  // wave per series: four teams per workgroup (and other counts), one workgroup per four units
  // or a persistent grid
  for (int N : Ns)
    for (int G = 1; G <= 12; ++G) {
      if (N > 48 && G > 3 && N % 4 != 3) continue;
      const int64_t units = (int64_t)N * G;
      for (int teams : {1, 2, 4}) {
        const int64_t per_unit = (units + teams - 1) / teams;
        for (int64_t grid : {per_unit, (int64_t)1, (int64_t)2, (int64_t)7, (int64_t)256, (int64_t)2048,
                             per_unit / 2 + 1, per_unit - 1})
          if (grid >= 1 && grid <= per_unit && !packed(N, G, teams, grid)) return 1;
      }
    }
  // batches whose unit count approaches 2^31 keep their series in 64 bits (the last units only)
  {
    const int N = 178956968, G = 12;   // N % 8 == 0, N * G = 2147483616 < 2^31
    for (int u = N * G - 96; u < N * G; ++u) {
      const fr::WalkUnit p = fr::walk_unit(u, G, false), x = fr::walk_unit(u, G, true);
      if (p.n != u / G || p.g != u % G || x.n < 0 || x.n >= N || x.g != (u >> 3) % G ||
          x.n != (int64_t)((u >> 3) / G) * 8 + (u & 7)) {
        printf("large batch: unit %d\n", u);
        return 1;
      }
    }
    const fr::WalkUnit w = fr::packed_unit(((int64_t)1 << 33) + 5, 3);
    if (w.n != (((int64_t)1 << 33) + 5) / 3 || w.g != (int)((((int64_t)1 << 33) + 5) % 3)) return 1;
  }
  printf("walk units: %lld launch shapes, every unit exactly once\n", checked);
  return 0;
}
