// How the data passes of the rank selection (kernels_select.hip: histogram, gather, successor)
// share the (N, T) elements of a row block among the `grid` workgroups of one group of jobs:
// select_partition, ONE pure function from (block, grid, N, T) to the block's series and time
// range.  Host-only and free of HIP, so that a CPU test pins the contract
// (tests/native/select_partition_host.cpp): for every grid >= 1, N >= 1, T >= 1 every (n, t) is
// visited by exactly one block.
#pragma once
#include "walk_types.h"   // FR_HOST_DEVICE

namespace fr {

// Block `block` visits the series n_first, n_first + n_step, ... (< N) and of each the
// elements t_lo <= t < t_hi.
struct SelPartition {
  int64_t n_first, n_step;
  int t_lo, t_hi;
};

// N >= grid: block b takes the whole series b, b + grid, ...
// N <  grid: every block takes a contiguous time part of ONE series.  The grid's q = grid / N
// blocks per series go round with r = grid % N left over: the first r series are cut into q + 1
// parts, the others into q, so every block has a part and every part a block.  The P parts of a
// series are T / P long, the first T % P of them one element longer: they tile [0, T) whatever T
// and P are (parts of a series shorter than its P blocks are empty).
// Three 32-bit divisions per BLOCK, none per element.  grid < 2^31; T < 2^31 (fr_select_ranks
// refuses more).
FR_HOST_DEVICE inline SelPartition select_partition(int64_t block, int64_t grid, int64_t N, int64_t T) {
  if (N >= grid) return SelPartition{block, grid, 0, (int)T};
  const uint32_t b = (uint32_t)block, series = (uint32_t)N, len = (uint32_t)T;
  const uint32_t q = (uint32_t)grid / series, r = (uint32_t)grid % series;
  const uint32_t wide = r * (q + 1);   // blocks of the series that are cut into q + 1 parts
  const uint32_t parts = b < wide ? q + 1 : q, at = b < wide ? b : b - wide;
  const uint32_t n = (b < wide ? 0 : r) + at / parts, part = at % parts;
  const uint32_t base = len / parts, longer = len % parts;
  const uint32_t t_lo = part * base + (part < longer ? part : longer);
  // (one series: the step only has to leave the row block)
  return SelPartition{(int64_t)n, N, (int)t_lo, (int)(t_lo + base + (part < longer ? 1u : 0u))};
}

}  // namespace fr
