// select_partition of csrc/select_partition.h (how the data passes of the rank selection share a
// row block among their workgroups), compiled for the host: exhaustive over grid 1 .. 512 and
// 4096, N 1 .. 600 and a few T around the sizes where the time axis is split.  For every
// combination the blocks' (series, [t_lo, t_hi)) intervals must tile every series' [0, T) exactly
// once; a block has nothing to do only where no block has more than one element (so never an
// idle block next to one that holds two parts' worth of a series); and N >= grid splits no series.
// Prints one line per failed combination (the first few); exit status 0 when there is none.
// Link with -pthread.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <thread>
#include <vector>

#include "select_partition.h"

namespace {

struct Piece {
  int64_t n;
  int lo, hi;
};

// nullptr, or what is wrong with the partition of (grid, N, T)
const char *check(int64_t grid, int64_t N, int64_t T, std::vector<int64_t> &end, std::vector<Piece> &late) {
  end.assign((size_t)N, 0);   // series n is covered exactly once up to end[n]
  late.clear();
  bool idle = false;
  int64_t most = 0;   // elements of the busiest block
  for (int64_t b = 0; b < grid; ++b) {
    const fr::SelPartition p = fr::select_partition(b, grid, N, T);
    if (p.n_first < 0 || p.n_step < 1 || p.t_lo < 0 || p.t_lo > p.t_hi || p.t_hi > T) return "range";
    if (N >= grid && (p.n_first != b || p.n_step != grid || p.t_lo != 0 || p.t_hi != T))
      return "N >= grid: not whole series b, b + grid, ...";
    int64_t mine = 0;
    if (p.t_lo < p.t_hi)
      for (int64_t n = p.n_first; n < N; n += p.n_step) {
        mine += p.t_hi - p.t_lo;
        if (end[(size_t)n] == p.t_lo) end[(size_t)n] = p.t_hi;   // (the parts usually come in order)
        else late.push_back(Piece{n, p.t_lo, p.t_hi});
      }
    idle = idle || mine == 0;
    most = std::max(most, mine);
  }
  std::sort(late.begin(), late.end(), [](const Piece &x, const Piece &y) {
    return x.n != y.n ? x.n < y.n : (x.lo != y.lo ? x.lo < y.lo : x.hi < y.hi);
  });
  for (const Piece &q : late) {
    if (end[(size_t)q.n] != q.lo) return q.lo < end[(size_t)q.n] ? "an element is visited twice" : "an element is not visited";
    end[(size_t)q.n] = q.hi;
  }
  for (int64_t n = 0; n < N; ++n)
    if (end[(size_t)n] != T) return "an element is not visited";
  if (idle && most > 1) return "a block has nothing to do while another has several elements";
  return nullptr;
}

}  // namespace

int main() {
  const int64_t Ts[] = {1, 2, 255, 4096, 4097, 5000, 9000, 40000};
  // (2.5 million combinations: the grids are dealt to a few threads)
  const unsigned n_threads = std::min(8u, std::max(1u, std::thread::hardware_concurrency()));
  std::vector<long> bad(n_threads, 0), done(n_threads, 0);
  std::vector<std::string> lines(n_threads);
  std::vector<std::thread> pool;
  for (unsigned w = 0; w < n_threads; ++w)
    pool.emplace_back([&, w] {
      std::vector<int64_t> end;
      std::vector<Piece> late;
      char line[160];
      for (int64_t gi = 1 + w; gi <= 513; gi += n_threads) {
        const int64_t grid = gi <= 512 ? gi : 4096;
        for (int64_t N = 1; N <= 600; ++N)
          for (const int64_t T : Ts) {
            ++done[w];
            if (const char *what = check(grid, N, T, end, late)) {
              if (bad[w]++ < 5) {
                std::snprintf(line, sizeof line, "FAIL grid %ld N %ld T %ld: %s\n", (long)grid, (long)N, (long)T, what);
                lines[w] += line;
              }
            }
          }
      }
    });
  long all_bad = 0, all_done = 0;
  for (unsigned w = 0; w < n_threads; ++w) {
    pool[w].join();
    std::fputs(lines[w].c_str(), stdout);
    all_bad += bad[w];
    all_done += done[w];
  }
  std::printf("%ld combinations, %ld checks failed\n", all_done, all_bad);
  return all_bad != 0;
}
