// Rank selection for Fruit.fit: the order statistics np.quantile interpolates between, by a radix
// select over the order keys (walk_types.h) of the pre-transformed fit sample.
#include <hip/hip_runtime.h>
#include <vector>

#include "kernels.h"
#include "select_partition.h"

namespace fr {

// ---------------------------------------------------------------- rank selection (fit)
// SegmentSieve._fit needs np.quantile of the pre-transformed fit sample
// (fruits/sieving/segment.py:66-75, increment.py:73-74).  np.quantile interpolates
// between two ORDER STATISTICS; those are found here exactly by a radix select over the
// order-preserving 64-bit image of the doubles (one job per wanted rank), so the
// (N_fit, T) rows never leave the device.  Three histogram passes fix the leading 24 bits
// (sign, exponent, 12 mantissa bits); the few elements that share them (<= kSelSmall,
// else the histogram passes simply go on) are gathered in ONE more pass over the data and
// the remaining 40 bits are settled inside a workgroup: 4 passes over the data instead of 9.
constexpr int kSelGroupJobs = 8;   // jobs of one group (they read the same (N, T) row block)
struct SelJob {
  const double *base;        // (N, T) row block of one iterated sum
  unsigned long long prefix; // key bits fixed so far
  long long k;               // rank among the elements that match the prefix
  int inc;
  int pad;
};

// The data passes of the selection (histogram, gather, successor) walk the differencing orders
// 0 .. MI of an element in ONE unrolled loop: the triangle of differences advances a level (D_k:
// k-th differences, zero-padded, see diff_at) and the jobs of that level - a group's jobs are
// sorted by order - look at its value.  MI is the launch's largest order (0 / 1 / 2, or kMaxInc for
// anything beyond).  Nothing is indexed by a run-time value: an array of the levels' keys picked
// by a job's order ends up in LDS (the compiler's promotion of private arrays), which is what
// the first version of these kernels spent its time on.
template <int MI>
__device__ __forceinline__ void element_load(const double *__restrict__ row, int t, double (&v)[MI + 1]) {
  v[0] = row[t];
#pragma unroll
  for (int j = 1; j <= MI; ++j) v[j] = t - j >= 0 ? row[t - j] : 0.0;
}
// level LVL - 1 -> LVL: afterwards v[0] = D_LVL[t]
template <int MI, int LVL>
__device__ __forceinline__ void next_level(int t, double (&v)[MI + 1]) {
#pragma unroll
  for (int j = 0; j + LVL <= MI; ++j) v[j] = (t - j >= 1) ? v[j] - v[j + 1] : 0.0;
}
// The element loop of the data passes: which series and which part of the time axis a block takes is
// select_partition's business (select_partition.h: every element exactly once, for every grid; no
// per-element 64-bit division); its threads stride over the time range.  Every block of a launch
// goes through the loop - one whose range is empty (a series shorter than the blocks it is shared
// among) runs no iteration and takes part in whatever its kernel does around the loop.
// A wave takes FOUR elements per lane at a time wherever all of them exist (f4; the rest
// one by one, f1): the loads of the four are in flight together, only the first of them can lie in
// the zero-padded head of a series (the others need no bounds tests), and whatever a pass reads
// per JOB - its prefix, its histogram row - is read once for the four.
constexpr int kSelUnroll = 4;
constexpr int kSelBlocks = 4096;
template <int MI>
__device__ __forceinline__ void element_load_inner(const double *__restrict__ row, int t, double (&v)[MI + 1]) {
#pragma unroll
  for (int j = 0; j <= MI; ++j) v[j] = row[t - j];
}
template <int MI, int LVL>
__device__ __forceinline__ void next_level_inner(double (&v)[MI + 1]) {
#pragma unroll
  for (int j = 0; j + LVL <= MI; ++j) v[j] = v[j] - v[j + 1];
}
// level LVL - 1 -> LVL of four elements; only element 0 can be one of a series' first MI
template <int MI, int LVL>
__device__ __forceinline__ void next_level4(const int (&t)[kSelUnroll], double (&v)[kSelUnroll][MI + 1]) {
  next_level<MI, LVL>(t[0], v[0]);
#pragma unroll
  for (int u = 1; u < kSelUnroll; ++u) next_level_inner<MI, LVL>(v[u]);
}
template <int MI, class F4, class F1>
__device__ __forceinline__ void for_elements(const double *__restrict__ base, int64_t N, int64_t T, F4 f4, F1 f1) {
  static_assert(MI < 64, "elements 1 .. 3 of a group of four lie behind the padded head");
  const SelPartition mine = select_partition((int64_t)blockIdx.x, (int64_t)gridDim.x, N, T);
  const int t_lo = mine.t_lo, t_hi = mine.t_hi;
  const int step = (int)blockDim.x;
  const int wave_last = (int)(threadIdx.x | 63u);   // the wave's last lane
  for (int64_t n = mine.n_first; n < N; n += mine.n_step) {
    const double *__restrict__ row = base + n * T;
    for (int tb = t_lo; tb < t_hi; tb += step * kSelUnroll) {
      const int t0 = tb + (int)threadIdx.x;
      if (tb + (kSelUnroll - 1) * step + wave_last < t_hi) {   // (uniform in the wave)
        int t[kSelUnroll];
        double v[kSelUnroll][MI + 1];
#pragma unroll
        for (int u = 0; u < kSelUnroll; ++u) t[u] = t0 + u * step;
        element_load<MI>(row, t[0], v[0]);
#pragma unroll
        for (int u = 1; u < kSelUnroll; ++u) element_load_inner<MI>(row, t[u], v[u]);
        f4(t, v);
      } else {
        for (int t = t0; t < t_hi; t += step) {
          double v[MI + 1];
          element_load<MI>(row, t, v);
          f1(t, v);
        }
      }
    }
  }
}

// The leading 32 bits of the order-preserving key: all that the first three digits and the bucket
// tests of the gather pass look at (32-bit operations instead of 64-bit shifts and compares).
__device__ __forceinline__ unsigned int order_key_hi(double v) {
  const unsigned int h = (unsigned int)((unsigned long long)__double_as_longlong(v) >> 32);
  return (h >> 31) ? ~h : (h | 0x80000000u);
}

// A group's jobs in LDS, once per workgroup and pass: the descriptors, and the jobs that take
// part in this pass compacted by differencing order (level i: act[lvl[i]] .. act[lvl[i + 1])).
constexpr int kSelTrack = kSelTrackJobs;   // (kernels.h: the host flags the jobs)
struct SelGroup {
  unsigned long long prefix[kSelGroupJobs];
  int inc[kSelGroupJobs], pad[kSelGroupJobs];
  int act[kSelGroupJobs];
  unsigned int act_hi[kSelGroupJobs];   // leading dword of the job's prefix
  int lvl[kMaxInc + 2];
};
// `take(j)`: does job j take part in this pass?  Returns the number of jobs that do.
template <int MI, class F>
__device__ __forceinline__ int load_group(SelGroup &g, const SelJob *__restrict__ jobs, int jb, int nj,
                                          F take) {
  if ((int)threadIdx.x < nj) {
    g.prefix[threadIdx.x] = jobs[jb + threadIdx.x].prefix;
    g.inc[threadIdx.x] = jobs[jb + threadIdx.x].inc;
    g.pad[threadIdx.x] = jobs[jb + threadIdx.x].pad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int n = 0;
    for (int i = 0; i <= MI; ++i) {
      g.lvl[i] = n;
      for (int j = 0; j < nj; ++j)
        if ((g.inc[j] == i || (i == MI && g.inc[j] > MI)) && take(j)) {
          g.act[n] = j;
          g.act_hi[n] = (unsigned int)(g.prefix[j] >> 32);
          ++n;
        }
    }
    g.lvl[MI + 1] = n;
  }
  __syncthreads();
  return g.lvl[MI + 1];
}

// SelJob::pad: bit 0 the caller also wants the NEXT order statistic; bit 1 that one lies
// outside what this job has seen (select_succ_kernel finds it); bit 2 the candidates that
// share the job's leading 24 bits fit a workgroup (their number in pad >> 8): no further
// histogram passes, select_gather_kernel + select_small_kernel finish the job; bit 3 more
// candidates than that (heavy ties); bit 4 (set by the host for the first kSelTrack jobs of a
// group and differencing order that want the next statistic) the gather pass leaves the smallest
// key above the job's bucket in succ[]
constexpr int kSelSmall = kSelSmallCap;   // (the host sizes the candidate lists with it)
constexpr int kSelSmallShift = 40;   // bits below this are settled among the gathered candidates

// One block column per GROUP of jobs that read the same (N, T) row block (the ranks and
// differencing orders one iterated sum is asked for): every element is loaded once per
// pass for all of them.
template <int MI, int LVL>
__device__ __forceinline__ void hist_level(const SelGroup &g, unsigned int (*lh)[256], int t,
                                           double (&v)[MI + 1], int shift) {
  if constexpr (LVL <= MI) {
    if constexpr (LVL > 0) next_level<MI, LVL>(t, v);
    const int kb = __builtin_amdgcn_readfirstlane(g.lvl[LVL]), ke = __builtin_amdgcn_readfirstlane(g.lvl[LVL + 1]);
    if (kb != ke) {
      const unsigned int kh = order_key_hi(v[0]);
      const unsigned long long key = order_key(v[0]);
      for (int k = kb; k < ke; ++k) {
        const int job = g.act[k];
        bool match;
        unsigned int bin;
        if (shift >= 32) {   // (uniform) a digit of the leading dword
          match = shift == 56 || (kh >> (shift - 24)) == (g.act_hi[k] >> (shift - 24));
          bin = (kh >> (shift - 32)) & 255u;
        } else {
          match = (key >> (shift + 8)) == (g.prefix[job] >> (shift + 8));
          bin = (unsigned int)(key >> shift) & 255u;
        }
        // The leading digits (sign, exponent, high mantissa bits) are shared by almost all
        // elements: 64 lanes adding to ONE LDS counter serialise.  The lanes that hold the
        // first matching lane's digit are counted together - all of them in the usual case -
        // and in the first two digits the others add one by one (both signs of an increment);
        // later digits are spread out: there the split costs more than it saves.
        const unsigned long long m = __ballot(match);
        if (m == 0) continue;
        const int leader = __ffsll((long long)m) - 1;
        const unsigned int lead_bin = (unsigned int)__builtin_amdgcn_readlane((int)bin, leader);
        const bool same = match && bin == lead_bin;
        const unsigned long long ms = __ballot(same);
        bool todo = match;
        if (ms == m || shift >= 48) {
          if ((int)(threadIdx.x & 63) == leader) atomicAdd(&lh[job][lead_bin], (unsigned int)__popcll(ms));
          todo = match && !same;
        }
        if (todo) atomicAdd(&lh[job][bin], 1u);
      }
    }
    hist_level<MI, LVL + 1>(g, lh, t, v, shift);
  }
}

// The same for a group of four elements (for_elements) and a digit known at compile time (the
// four digits of the leading dword: every pass of a usual fit): a job's row and prefix are read
// once for the four, the digit and the prefix test are immediates.
template <int SHIFT>
__device__ __forceinline__ void hist_count(unsigned int *__restrict__ row, unsigned int kh, unsigned int ph) {
  static_assert(SHIFT >= 32 && SHIFT <= 56, "a digit of the leading dword");
  const bool match = SHIFT == 56 || ((kh ^ ph) >> (SHIFT - 24)) == 0u;
  const unsigned int bin = (kh >> (SHIFT - 32)) & 255u;
  unsigned long long m = __ballot(match);
  if (m == 0) return;
  bool todo = match;
  // the first digit (sign, seven exponent bits) has two to four values in a wave: two of them are
  // counted lane group by lane group (one: 2.26 ms for 64 groups, two: 2.14, three: 2.19)
  constexpr int kRounds = SHIFT == 56 ? 2 : 1;
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const int leader = __ffsll((long long)m) - 1;
    const unsigned int lead_bin = (unsigned int)__builtin_amdgcn_readlane((int)bin, leader);
    const bool same = todo && bin == lead_bin;
    const unsigned long long ms = __ballot(same);
    // (the first digit alone counts a partial lane group: in the second one - four exponent and
    // four mantissa bits - the rest of the wave is spread out already, 1.81 -> 1.74 ms)
    if (SHIFT >= 56 || ms == m) {
      if ((int)(threadIdx.x & 63) == leader) atomicAdd(&row[lead_bin], (unsigned int)__popcll(ms));
      todo = todo && !same;
      m &= ~ms;
    }
    if (m == 0) return;
  }
  if (todo) atomicAdd(&row[bin], 1u);
}
template <int MI, int SHIFT, int LVL>
__device__ __forceinline__ void hist_level4(const SelGroup &g, unsigned int (*lh)[256],
                                            const int (&t)[kSelUnroll], double (&v)[kSelUnroll][MI + 1]) {
  if constexpr (LVL <= MI) {
    if constexpr (LVL > 0) next_level4<MI, LVL>(t, v);
    const int kb = __builtin_amdgcn_readfirstlane(g.lvl[LVL]), ke = __builtin_amdgcn_readfirstlane(g.lvl[LVL + 1]);
    if (kb != ke) {
      unsigned int kh[kSelUnroll];
#pragma unroll
      for (int u = 0; u < kSelUnroll; ++u) kh[u] = order_key_hi(v[u][0]);
      for (int k = kb; k < ke; ++k) {
        unsigned int *row = lh[__builtin_amdgcn_readfirstlane(g.act[k])];
        const unsigned int ph = (unsigned int)__builtin_amdgcn_readfirstlane((int)g.act_hi[k]);
#pragma unroll
        for (int u = 0; u < kSelUnroll; ++u) hist_count<SHIFT>(row, kh[u], ph);
      }
    }
    hist_level4<MI, SHIFT, LVL + 1>(g, lh, t, v);
  }
}

// The FIRST digit (sign, seven exponent bits): every element takes part and a block sees a handful of
// values - as LDS adds they collide (the pass was bound by LDS conflicts: 1.9 TB/s against the third
// digit's 3.9).  A thread counts the digit's values it meets in kBinPairs register pairs per
// differencing order and only a further value evicts one to LDS; the pairs are added to the block's
// histogram once, at the end.
constexpr unsigned int kBinNone = 0xffffffffu;
// (pairs per differencing order, Fruit.fit of fruit_reduced on one box: none 19.3 ms, one 20.0, two 17.9,
// three 18.3, four 18.5, eight 18.8 - the compares are paid per element, two pairs hold the two signs)
constexpr int kBinPairs = 2;
struct BinCache {
  unsigned int bin[kBinPairs], cnt[kBinPairs];
};
__device__ __forceinline__ void bin_cache_add(BinCache &c, unsigned int b, unsigned int *__restrict__ row) {
  bool hit = false;
#pragma unroll
  for (int i = 0; i < kBinPairs; ++i) {
    const bool h = b == c.bin[i];
    c.cnt[i] += h ? 1u : 0u;
    hit = hit || h;
  }
  if (!hit) {   // (rare: a free pair, else the last one goes to LDS)
    bool placed = false;
#pragma unroll
    for (int i = 0; i + 1 < kBinPairs; ++i)
      if (!placed && c.bin[i] == kBinNone) {
        c.bin[i] = b;
        c.cnt[i] = 1u;
        placed = true;
      }
    if (!placed) {
      if (c.bin[kBinPairs - 1] != kBinNone) atomicAdd(&row[c.bin[kBinPairs - 1]], c.cnt[kBinPairs - 1]);
      c.bin[kBinPairs - 1] = b;
      c.cnt[kBinPairs - 1] = 1u;
    }
  }
}
template <int MI, int LVL>
__device__ __forceinline__ void hist_first4(const SelGroup &g, unsigned int (*lh)[256], BinCache (&bc)[MI + 1],
                                            const int (&t)[kSelUnroll], double (&v)[kSelUnroll][MI + 1]) {
  if constexpr (LVL <= MI) {
    if constexpr (LVL > 0) next_level4<MI, LVL>(t, v);
    const int kb = __builtin_amdgcn_readfirstlane(g.lvl[LVL]), ke = __builtin_amdgcn_readfirstlane(g.lvl[LVL + 1]);
    if (kb != ke) {   // (one job per order takes part in the first pass: the order's histogram)
      unsigned int *row = lh[__builtin_amdgcn_readfirstlane(g.act[kb])];
#pragma unroll
      for (int u = 0; u < kSelUnroll; ++u) bin_cache_add(bc[LVL], order_key_hi(v[u][0]) >> 24, row);
    }
    hist_first4<MI, LVL + 1>(g, lh, bc, t, v);
  }
}
template <int MI, int LVL>
__device__ __forceinline__ void hist_first_flush(const SelGroup &g, unsigned int (*lh)[256],
                                                 const BinCache (&bc)[MI + 1]) {
  if constexpr (LVL <= MI) {
    if (g.lvl[LVL] != g.lvl[LVL + 1]) {
      unsigned int *row = lh[g.act[g.lvl[LVL]]];
#pragma unroll
      for (int i = 0; i < kBinPairs; ++i)
        if (bc[LVL].bin[i] != kBinNone) atomicAdd(&row[bc[LVL].bin[i]], bc[LVL].cnt[i]);
    }
    hist_first_flush<MI, LVL + 1>(g, lh, bc);
  }
}

// SHIFT: the digit when it is one of the leading dword's (the four-wide path), else 0 - then the
// run-time `shift` counts (the low digits: jobs with heavy ties only)
template <int MI, int SHIFT>
__global__ __launch_bounds__(256) void select_hist_kernel(const SelJob *__restrict__ jobs,
                                                           const int2 *__restrict__ groups,
                                                           int64_t N, int64_t T, int shift,
                                                           unsigned int *__restrict__ hist) {
  __shared__ unsigned int lh[kSelGroupJobs][256];
  __shared__ SelGroup g;
  const int jb = groups[blockIdx.y].x, nj = groups[blockIdx.y].y;
  // jobs that finish among their gathered candidates take no part in later passes; first pass:
  // no prefix yet - jobs of one differencing order see the same histogram, which is counted
  // once and copied below
  if constexpr (SHIFT != 0) shift = SHIFT;
  const int n_act = load_group<MI>(g, jobs, jb, nj, [&](int j) {
    return !(g.pad[j] & 4) && !(shift == 56 && j > 0 && g.inc[j] == g.inc[j - 1]);
  });
  if (n_act == 0) return;
  for (int j = 0; j < nj; ++j) lh[j][threadIdx.x] = 0;
  __syncthreads();
  if constexpr (SHIFT == 56 && MI <= 2) {
    BinCache bc[MI + 1];
#pragma unroll
    for (int l = 0; l <= MI; ++l)
#pragma unroll
      for (int i = 0; i < kBinPairs; ++i) {
        bc[l].bin[i] = kBinNone;
        bc[l].cnt[i] = 0u;
      }
    for_elements<MI>(
        jobs[jb].base, N, T,
        [&](const int (&t)[kSelUnroll], double (&v)[kSelUnroll][MI + 1]) { hist_first4<MI, 0>(g, lh, bc, t, v); },
        [&](int t, double (&v)[MI + 1]) { hist_level<MI, 0>(g, lh, t, v, SHIFT); });
    hist_first_flush<MI, 0>(g, lh, bc);
  } else if constexpr (SHIFT != 0) {
    for_elements<MI>(
        jobs[jb].base, N, T,
        [&](const int (&t)[kSelUnroll], double (&v)[kSelUnroll][MI + 1]) { hist_level4<MI, SHIFT, 0>(g, lh, t, v); },
        [&](int t, double (&v)[MI + 1]) { hist_level<MI, 0>(g, lh, t, v, SHIFT); });
  } else {
    const auto one = [&](int t, double (&v)[MI + 1]) { hist_level<MI, 0>(g, lh, t, v, shift); };
    for_elements<MI>(jobs[jb].base, N, T,
                     [&](const int (&t)[kSelUnroll], double (&v)[kSelUnroll][MI + 1]) {
#pragma unroll
                       for (int u = 0; u < kSelUnroll; ++u) one(t[u], v[u]);
                     },
                     one);
  }
  __syncthreads();
  for (int j = 0; j < nj; ++j) {
    if (g.pad[j] & 4) continue;
    int src = j;   // first pass: the histogram of the first job of this differencing order
    if (shift == 56)
      while (src > 0 && g.inc[src - 1] == g.inc[j]) --src;
    if (lh[src][threadIdx.x]) atomicAdd(&hist[(jb + j) * 256 + threadIdx.x], lh[src][threadIdx.x]);
  }
}

__global__ void select_pick_kernel(SelJob *__restrict__ jobs, int shift,
                                   unsigned int *__restrict__ hist, double *__restrict__ out,
                                   unsigned long long *__restrict__ succ,
                                   unsigned int *__restrict__ n_big,
                                   unsigned long long *__restrict__ cand,
                                   unsigned int *__restrict__ cnt) {
  const int job = blockIdx.x;
  if (jobs[job].pad & 4) return;   // (its histogram received nothing)
  if (threadIdx.x == 0) {
    long long k = jobs[job].k, run = 0;
    int d = 0;
    for (; d < 255; ++d) {
      const long long c = hist[job * 256 + d];
      if (k < run + c) break;
      run += c;
    }
    jobs[job].k = k - run;
    jobs[job].prefix |= (unsigned long long)d << shift;
    if (shift == kSelSmallShift) {
      if (hist[job * 256 + d] <= (unsigned int)kSelSmall)
        jobs[job].pad |= 4 | ((int)hist[job * 256 + d] << 8);
      else {
        // too many candidates for a workgroup - usually ONE value many times (the zeros among
        // the increments of a running maximum): select_gather_kernel checks whether they are
        // all equal (cand[0] = the first one seen, cand[1] != 0 = another one exists)
        jobs[job].pad |= 8;
        cnt[job] = hist[job * 256 + d];
        cand[(int64_t)job * kSelSmall] = ~0ull;
        cand[(int64_t)job * kSelSmall + 1] = 0ull;
        atomicAdd(n_big, 1u);   // a job that stays in the histogram passes (unless resolved)
      }
    }
    if (shift == 0) {
      out[job] = order_key_value(jobs[job].prefix);
      // the NEXT order statistic (np.quantile interpolates between two neighbours): the same
      // value when more copies of it remain, else the smallest larger element (one more pass,
      // select_succ_kernel) - instead of a second 8-pass selection
      if (jobs[job].pad & 1) {
        if (k - run + 1 < (long long)hist[job * 256 + d])
          succ[job] = jobs[job].prefix;
        else
          jobs[job].pad |= 2;
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 256; i += blockDim.x) hist[job * 256 + i] = 0;
}

// One pass over the data: the keys that share a small job's leading bits go to its
// candidate list (cand[job][0 .. kSelSmall), filled through cnt[job]).
//
// The smallest key ABOVE a job's bucket is the next order statistic when the selected one is the
// bucket's largest - the usual case for the median of increments, which lies near zero where the
// 24-bit buckets of floating-point numbers hold an element or two.  It is found here, in the
// pass that reads everything anyway (jobs flagged with pad bit 4; per thread a running minimum
// in registers, `above`), instead of in a pass of its own (select_succ_kernel).
struct GatherBig {   // up to two jobs of the group whose candidates may all be equal
  int big0, big1;
  unsigned long long ref0, ref1;   // the first candidate anybody saw
  bool other0, other1;
};
// one element's key against job j of the group (hit: it lies in the job's bucket)
__device__ __forceinline__ void gather_job(int jb, int j, bool hit, unsigned long long key, GatherBig &gb,
                                           unsigned long long *__restrict__ cand,
                                           unsigned int *__restrict__ cnt) {
  if (j == gb.big0 || j == gb.big1) {
    unsigned long long &ref = j == gb.big0 ? gb.ref0 : gb.ref1;
    // nobody has published a candidate yet: ONE lane of the wave tries (a compare-and-swap
    // per thread on one address would serialise a hundred thousand of them) and tells
    // the others what the reference is
    const unsigned long long ask = __ballot(hit && ref == ~0ull);
    if (ask != 0) {
      const int leader = __ffsll((long long)ask) - 1;
      unsigned long long got = 0;
      if ((int)(threadIdx.x & 63) == leader) {
        const unsigned long long old = atomicCAS(&cand[(int64_t)(jb + j) * kSelSmall], ~0ull, key);
        got = old == ~0ull ? key : old;
      }
      const unsigned long long told = __shfl(got, leader);
      if (ref == ~0ull) ref = told;
    }
    if (hit && key != ref) (j == gb.big0 ? gb.other0 : gb.other1) = true;
  } else if (hit) {
    const unsigned int slot = atomicAdd(&cnt[jb + j], 1u);
    if (slot < (unsigned int)kSelSmall) cand[(int64_t)(jb + j) * kSelSmall + slot] = key;
  }
}
template <int MI, int LVL>
__device__ __forceinline__ void gather_level(const SelGroup &g, int jb, int t, double (&v)[MI + 1],
                                             unsigned long long (&above)[MI + 1][kSelTrack],
                                             const unsigned int (&track)[MI + 1][kSelTrack],
                                             GatherBig &gb, unsigned long long *__restrict__ cand,
                                             unsigned int *__restrict__ cnt) {
  if constexpr (LVL <= MI) {
    if constexpr (LVL > 0) next_level<MI, LVL>(t, v);
    const int kb = __builtin_amdgcn_readfirstlane(g.lvl[LVL]), ke = __builtin_amdgcn_readfirstlane(g.lvl[LVL + 1]);
    if (kb != ke) {
      // the bucket (leading 24 bits) of this element
      const unsigned int bucket = order_key_hi(v[0]) >> (kSelSmallShift - 32);
      const unsigned long long key = order_key(v[0]);
#pragma unroll
      for (int a = 0; a < kSelTrack; ++a)   // (the level's first jobs: the host flags only those)
        if (bucket > track[LVL][a] && key < above[LVL][a]) above[LVL][a] = key;
      for (int k = kb; k < ke; ++k)
        gather_job(jb, g.act[k], bucket == (g.act_hi[k] >> (kSelSmallShift - 32)), key, gb, cand, cnt);
    }
    gather_level<MI, LVL + 1>(g, jb, t, v, above, track, gb, cand, cnt);
  }
}
// ... of a group of four elements (for_elements): a job's bucket is read once for the four, and a
// job none of the wave's 256 elements falls to - nearly every job, nearly every time: a bucket holds
// at most kSelSmall of the millions - costs four compares and a branch
template <int MI, int LVL>
__device__ __forceinline__ void gather_level4(const SelGroup &g, int jb, const int (&t)[kSelUnroll],
                                              double (&v)[kSelUnroll][MI + 1],
                                              unsigned long long (&above)[MI + 1][kSelTrack],
                                              const unsigned int (&track)[MI + 1][kSelTrack],
                                              GatherBig &gb, unsigned long long *__restrict__ cand,
                                              unsigned int *__restrict__ cnt) {
  if constexpr (LVL <= MI) {
    if constexpr (LVL > 0) next_level4<MI, LVL>(t, v);
    const int kb = __builtin_amdgcn_readfirstlane(g.lvl[LVL]), ke = __builtin_amdgcn_readfirstlane(g.lvl[LVL + 1]);
    if (kb != ke) {
      unsigned int bucket[kSelUnroll];
      unsigned long long key[kSelUnroll];
#pragma unroll
      for (int u = 0; u < kSelUnroll; ++u) {
        bucket[u] = order_key_hi(v[u][0]) >> (kSelSmallShift - 32);
        key[u] = order_key(v[u][0]);
      }
#pragma unroll
      for (int a = 0; a < kSelTrack; ++a) {
        const unsigned int tr = (unsigned int)__builtin_amdgcn_readfirstlane((int)track[LVL][a]);
        if (tr == ~0u) continue;   // (nothing is tracked in this place)
#pragma unroll
        for (int u = 0; u < kSelUnroll; ++u)
          if (bucket[u] > tr && key[u] < above[LVL][a]) above[LVL][a] = key[u];
      }
      for (int k = kb; k < ke; ++k) {
        const int j = __builtin_amdgcn_readfirstlane(g.act[k]);
        const unsigned int jbucket =
            (unsigned int)__builtin_amdgcn_readfirstlane((int)g.act_hi[k]) >> (kSelSmallShift - 32);
        bool any = false;
#pragma unroll
        for (int u = 0; u < kSelUnroll; ++u) any = any || bucket[u] == jbucket;
        if (__ballot(any) == 0) continue;
#pragma unroll
        for (int u = 0; u < kSelUnroll; ++u) gather_job(jb, j, bucket[u] == jbucket, key[u], gb, cand, cnt);
      }
    }
    gather_level4<MI, LVL + 1>(g, jb, t, v, above, track, gb, cand, cnt);
  }
}
template <int MI, int LVL>
__device__ __forceinline__ void gather_publish(const SelGroup &g, int jb,
                                               const unsigned long long (&above)[MI + 1][kSelTrack],
                                               unsigned long long *__restrict__ succ) {
  if constexpr (LVL <= MI) {
    const int kb = g.lvl[LVL], ke = g.lvl[LVL + 1];
#pragma unroll
    for (int a = 0; a < kSelTrack; ++a) {
      if (kb + a < ke && (g.pad[g.act[kb + a]] & 16)) {
        unsigned long long b = above[LVL][a];
        for (int o = 32; o > 0; o >>= 1) {
          const unsigned long long w = __shfl_xor(b, o);
          b = w < b ? w : b;
        }
        if ((threadIdx.x & 63) == 0 && b != ~0ull) atomicMin(&succ[jb + g.act[kb + a]], b);
      }
    }
    gather_publish<MI, LVL + 1>(g, jb, above, succ);
  }
}

template <int MI>
__global__ __launch_bounds__(256) void select_gather_kernel(const SelJob *__restrict__ jobs,
                                                             const int2 *__restrict__ groups,
                                                             int64_t N, int64_t T,
                                                             unsigned long long *__restrict__ cand,
                                                             unsigned int *__restrict__ cnt,
                                                             unsigned long long *__restrict__ succ) {
  static_assert(kSelSmallShift >= 32, "the bucket test reads the leading dword of a key");
  __shared__ SelGroup g;
  const int jb = groups[blockIdx.y].x, nj = groups[blockIdx.y].y;
  if (load_group<MI>(g, jobs, jb, nj, [&](int j) { return (g.pad[j] & 12) != 0; }) == 0) return;
  GatherBig gb{-1, -1, ~0ull, ~0ull, false, false};
  for (int j = 0; j < nj; ++j) {
    if (g.pad[j] & 8) {
      if (gb.big0 < 0) gb.big0 = j;
      else if (gb.big1 < 0) gb.big1 = j;
    }
  }
  if (gb.big0 >= 0) gb.ref0 = cand[(int64_t)(jb + gb.big0) * kSelSmall];
  if (gb.big1 >= 0) gb.ref1 = cand[(int64_t)(jb + gb.big1) * kSelSmall];
  unsigned long long above[MI + 1][kSelTrack];
  unsigned int track[MI + 1][kSelTrack];   // bucket of a tracked job (else: nothing lies above it)
#pragma unroll
  for (int i = 0; i <= MI; ++i)
#pragma unroll
    for (int a = 0; a < kSelTrack; ++a) {
      above[i][a] = ~0ull;
      const int k = g.lvl[i] + a;
      const bool on = k < g.lvl[i + 1] && (g.pad[g.act[k < kSelGroupJobs ? k : 0]] & 16);
      track[i][a] = on ? g.act_hi[k < kSelGroupJobs ? k : 0] >> (kSelSmallShift - 32) : ~0u;
    }
  for_elements<MI>(
      jobs[jb].base, N, T,
      [&](const int (&t)[kSelUnroll], double (&v)[kSelUnroll][MI + 1]) {
        gather_level4<MI, 0>(g, jb, t, v, above, track, gb, cand, cnt);
      },
      [&](int t, double (&v)[MI + 1]) { gather_level<MI, 0>(g, jb, t, v, above, track, gb, cand, cnt); });
  if (gb.other0) cand[(int64_t)(jb + gb.big0) * kSelSmall + 1] = 1ull;
  if (gb.other1) cand[(int64_t)(jb + gb.big1) * kSelSmall + 1] = 1ull;
  gather_publish<MI, 0>(g, jb, above, succ);
}

// One workgroup per small job: the k-th smallest of its candidates (and the next one) by
// counting - every thread ranks its candidates against all of them in LDS.
__global__ __launch_bounds__(256) void select_small_kernel(SelJob *__restrict__ jobs,
                                                            const unsigned long long *__restrict__ cand,
                                                            const unsigned int *__restrict__ cnt,
                                                            double *__restrict__ out,
                                                            unsigned long long *__restrict__ succ,
                                                            unsigned int *__restrict__ n_big) {
  __shared__ unsigned long long next_key, s_prefix;
  __shared__ unsigned int lh[256];
  __shared__ int s_k, s_eq;
  const int job = blockIdx.x;
  if (jobs[job].pad & 8) {
    // more candidates than a workgroup settles: done all the same when they are ONE value
    if (threadIdx.x == 0) {
      const unsigned long long key = cand[(int64_t)job * kSelSmall];
      if (key != ~0ull && cand[(int64_t)job * kSelSmall + 1] == 0ull) {
        out[job] = order_key_value(key);
        jobs[job].prefix = key;
        // (the next one: another copy, else the smallest key above the bucket - already in
        // succ[job], select_gather_kernel)
        if (jobs[job].pad & 1) {
          if (jobs[job].k + 1 < (long long)cnt[job]) succ[job] = key;
          else if (!(jobs[job].pad & 16)) jobs[job].pad |= 2;
        }
        jobs[job].pad |= 4;
        atomicSub(n_big, 1u);
      }
    }
    return;
  }
  if (!(jobs[job].pad & 4)) return;
  int n = (int)cnt[job];
  if (n > kSelSmall) n = kSelSmall;   // (cannot happen: the histogram counted the same elements)
  // (the candidates stay where the gather pass put them: five sweeps over a list that is in L2)
  const unsigned long long *__restrict__ keys = cand + (int64_t)job * kSelSmall;
  if (threadIdx.x == 0) {
    next_key = ~0ull;
    s_prefix = jobs[job].prefix;   // (the leading 24 bits: every candidate has them)
    s_k = (int)jobs[job].k;
  }
  // the remaining five digits by the same radix selection, inside LDS (ranking every candidate
  // against all the others - 4 million compares for a full list - took as long as a pass over
  // the data)
  for (int shift = kSelSmallShift - 8; shift >= 0; shift -= 8) {
    lh[threadIdx.x] = 0;
    __syncthreads();
    const unsigned long long prefix = s_prefix;
    const int k = s_k;
    for (int i = threadIdx.x; i < n; i += blockDim.x)
      if ((keys[i] >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&lh[(keys[i] >> shift) & 255u], 1u);
    __syncthreads();
    if (threadIdx.x < 64) {   // lane l: bins 4 l .. 4 l + 3
      const int l = threadIdx.x;
      const unsigned int c0 = lh[4 * l], c1 = lh[4 * l + 1], c2 = lh[4 * l + 2], c3 = lh[4 * l + 3];
      const unsigned int mine = c0 + c1 + c2 + c3;
      unsigned int incl = mine;
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned int w = __shfl_up(incl, o);
        if (l >= o) incl += w;
      }
      const unsigned int excl = incl - mine;
      if ((unsigned int)k >= excl && (unsigned int)k < incl) {   // (one lane: k < the number counted)
        unsigned int r = (unsigned int)k - excl;
        int d = 4 * l;
        unsigned int c = c0;
        if (r >= c0) { r -= c0; ++d; c = c1;
          if (r >= c1) { r -= c1; ++d; c = c2;
            if (r >= c2) { r -= c2; ++d; c = c3; } } }
        s_k = (int)r;
        s_eq = (int)c;
        s_prefix = prefix | ((unsigned long long)d << shift);
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const unsigned long long mine = s_prefix;   // the k-th key; s_eq copies of it, s_k of them in front
    out[job] = order_key_value(mine);
    jobs[job].prefix = mine;
    if (jobs[job].pad & 1) {
      if (s_k + 1 < s_eq) succ[job] = mine;
      else next_key = ~0ull - 1;   // marks: look for the smallest larger key
    }
  }
  __syncthreads();
  if (!(jobs[job].pad & 1) || next_key == ~0ull) return;
  // the next order statistic is the smallest candidate above the selected key - or, when the
  // selected key is the largest candidate, the smallest key above the bucket
  const unsigned long long sel = s_prefix;
  unsigned long long best = ~0ull;
  for (int i = threadIdx.x; i < n; i += blockDim.x)
    if (keys[i] > sel && keys[i] < best) best = keys[i];
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long w = __shfl_xor(best, o);
    best = w < best ? w : best;
  }
  __syncthreads();
  if (threadIdx.x == 0) next_key = ~0ull;
  __syncthreads();
  if ((threadIdx.x & 63) == 0 && best != ~0ull) atomicMin(&next_key, best);
  __syncthreads();
  // (none: the selected key is the bucket's largest; succ[job] already holds the smallest key
  // above the bucket when the gather pass tracked it - pad bit 4 - else a pass of its own finds it)
  if (threadIdx.x == 0) {
    if (next_key != ~0ull) succ[job] = next_key;
    else if (!(jobs[job].pad & 16)) jobs[job].pad |= 2;
  }
}

// smallest key above the selected one, for the jobs flagged pad & 2 (select_pick_kernel at the
// last digit; select_small_kernel for jobs whose successor the gather pass did not track);
// succ[] starts at the largest key
template <int MI, int LVL>
__device__ __forceinline__ void succ_level(const SelGroup &g, int jb, int t, double (&v)[MI + 1],
                                           unsigned long long (&best)[MI + 1],
                                           unsigned long long *__restrict__ succ) {
  if constexpr (LVL <= MI) {
    if constexpr (LVL > 0) next_level<MI, LVL>(t, v);
    const int kb = __builtin_amdgcn_readfirstlane(g.lvl[LVL]), ke = __builtin_amdgcn_readfirstlane(g.lvl[LVL + 1]);
    if (kb != ke) {
      const unsigned long long key = order_key(v[0]);
      // the level's first job: a running minimum in a register, published at the end
      if (key > g.prefix[g.act[kb]] && key < best[LVL]) best[LVL] = key;
      // (the tail of a time range runs with some of a wave's lanes switched off - for_elements, f1:
      // a shuffle would read what such a lane does not hold)
      const bool whole_wave = __ballot(true) == ~0ull;
      for (int k = kb + 1; k < ke; ++k) {
        // (further jobs of a level are rare: the wave's smallest candidate straight to memory)
        unsigned long long b = key > g.prefix[g.act[k]] ? key : ~0ull;
        if (__ballot(b != ~0ull) == 0) continue;
        unsigned long long *dst = &succ[jb + g.act[k]];
        if (whole_wave) {
          for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long w = __shfl_xor(b, o);
            b = w < b ? w : b;
          }
          if ((threadIdx.x & 63) == 0 && b < *dst) atomicMin(dst, b);
        } else if (b < *dst) {   // lane by lane
          atomicMin(dst, b);
        }
      }
    }
    succ_level<MI, LVL + 1>(g, jb, t, v, best, succ);
  }
}
template <int MI, int LVL>
__device__ __forceinline__ void succ_publish(const SelGroup &g, int jb, const unsigned long long (&best)[MI + 1],
                                             unsigned long long *__restrict__ succ) {
  if constexpr (LVL <= MI) {
    if (g.lvl[LVL] != g.lvl[LVL + 1]) {
      unsigned long long b = best[LVL];
      for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long w = __shfl_xor(b, o);
        b = w < b ? w : b;
      }
      if ((threadIdx.x & 63) == 0 && b != ~0ull) atomicMin(&succ[jb + g.act[g.lvl[LVL]]], b);
    }
    succ_publish<MI, LVL + 1>(g, jb, best, succ);
  }
}
template <int MI>
__global__ __launch_bounds__(256) void select_succ_kernel(const SelJob *__restrict__ jobs,
                                                           const int2 *__restrict__ groups,
                                                           int64_t N, int64_t T,
                                                           unsigned long long *succ) {
  __shared__ SelGroup g;
  const int jb = groups[blockIdx.y].x, nj = groups[blockIdx.y].y;
  if (load_group<MI>(g, jobs, jb, nj, [&](int j) { return (g.pad[j] & 2) != 0; }) == 0) return;
  unsigned long long best[MI + 1];
#pragma unroll
  for (int i = 0; i <= MI; ++i) best[i] = ~0ull;
  const auto one = [&](int t, double (&v)[MI + 1]) { succ_level<MI, 0>(g, jb, t, v, best, succ); };
  for_elements<MI>(jobs[jb].base, N, T,
                   [&](const int (&t)[kSelUnroll], double (&v)[kSelUnroll][MI + 1]) {
#pragma unroll
                     for (int u = 0; u < kSelUnroll; ++u) one(t[u], v[u]);
                   },
                   one);
  succ_publish<MI, 0>(g, jb, best, succ);
}

// MI: the largest differencing order of the launch's jobs (kernels are compiled for 0, 1, 2 and
// kMaxInc)
template <int MI>
static hipError_t select_ranks_mi(SelJob *jb, int n_jobs, const int2 *gr, int n_groups,
                                  const int32_t *h_groups, int2 *gr_active, bool untracked, int64_t N, int64_t T,
                                  unsigned int *hist, double *out, unsigned long long *succ,
                                  unsigned long long *cand, unsigned int *cand_count, hipStream_t st) {
  // blocks per group: about kSelBlocks in all (16 per CU) - a block zeroes and publishes its
  // histograms whatever it counts (64 groups: 32768 blocks 2.62 ms, 8192 2.33, 4096 2.24, 2048 2.30)
  int64_t bpj = (N * T + 256 * 16 - 1) / (256 * 16);
  if (bpj > 512) bpj = 512;
  if (bpj * n_groups > kSelBlocks) bpj = (kSelBlocks + n_groups - 1) / n_groups;
  if (bpj < 1) bpj = 1;
  const int2 *pass_groups = gr;
  int pass_n = n_groups;
  bool trailing = false;   // some jobs go through all eight digits
  for (int shift = 56; shift >= 0; shift -= 8) {
    const dim3 hgrid((unsigned)bpj, (unsigned)pass_n);
    switch (shift) {
      case 56: hipLaunchKernelGGL((select_hist_kernel<MI, 56>), hgrid, dim3(256), 0, st, jb, pass_groups, N, T, shift, hist); break;
      case 48: hipLaunchKernelGGL((select_hist_kernel<MI, 48>), hgrid, dim3(256), 0, st, jb, pass_groups, N, T, shift, hist); break;
      case 40: hipLaunchKernelGGL((select_hist_kernel<MI, 40>), hgrid, dim3(256), 0, st, jb, pass_groups, N, T, shift, hist); break;
      case 32: hipLaunchKernelGGL((select_hist_kernel<MI, 32>), hgrid, dim3(256), 0, st, jb, pass_groups, N, T, shift, hist); break;
      default: hipLaunchKernelGGL((select_hist_kernel<MI, 0>), hgrid, dim3(256), 0, st, jb, pass_groups, N, T, shift, hist);
    }
    hipLaunchKernelGGL(select_pick_kernel, dim3((unsigned)n_jobs), dim3(64), 0, st, jb, shift,
                       hist, out, succ, cand_count + n_jobs, cand, cand_count);
    if (shift == kSelSmallShift) {
      hipLaunchKernelGGL(select_gather_kernel<MI>, dim3((unsigned)bpj, (unsigned)n_groups), dim3(256),
                         0, st, jb, gr, N, T, cand, cand_count, succ);
      hipLaunchKernelGGL(select_small_kernel, dim3((unsigned)n_jobs), dim3(256), 0, st, jb, cand,
                         cand_count, out, succ, cand_count + n_jobs);
      // (h_groups == nullptr - fr_select_ranks_begin: nothing is read back, the host does not wait.
      // The five remaining passes are launched whatever is left for them, over all groups: the
      // workgroups of a group without a job in them leave at once - eleven launches of a few
      // microseconds each in the usual case)
      if (h_groups == nullptr) {
        trailing = true;
        continue;
      }
      // no job left in the histogram passes (the usual case): done.  Else only the jobs with
      // too many candidates for a workgroup - heavy ties that are not ONE value - go on, and
      // the five remaining passes run over THEIR groups alone (the host reads the jobs' flags)
      unsigned int n_big = 1;
      if (hipMemcpyAsync(&n_big, cand_count + n_jobs, 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
          hipStreamSynchronize(st) != hipSuccess) {
        (void)hipGetLastError();
        n_big = 1;
      }
      if (n_big == 0) break;
      std::vector<SelJob> hj((size_t)n_jobs);
      if (hipMemcpy(hj.data(), jb, (size_t)n_jobs * sizeof(SelJob), hipMemcpyDeviceToHost) == hipSuccess) {
        std::vector<int32_t> active;
        for (int g = 0; g < n_groups; ++g) {
          bool left = false;
          for (int j = 0; j < h_groups[2 * g + 1]; ++j) left = left || !(hj[h_groups[2 * g] + j].pad & 4);
          if (left) {
            active.push_back(h_groups[2 * g]);
            active.push_back(h_groups[2 * g + 1]);
          }
        }
        if (active.empty()) break;
        if (hipMemcpy(gr_active, active.data(), active.size() * 4, hipMemcpyHostToDevice) == hipSuccess) {
          pass_groups = gr_active;
          pass_n = (int)active.size() / 2;
        } else {
          (void)hipGetLastError();
        }
      } else {
        (void)hipGetLastError();
      }
      trailing = true;
    }
  }
  // (jobs that went through all eight digits and need a neighbour outside what they saw: one
  // more pass over their groups; everybody else has it from the gather pass - unless a group
  // asks for more neighbours per differencing order than that pass tracks)
  if (untracked)
    hipLaunchKernelGGL(select_succ_kernel<MI>, dim3((unsigned)bpj, (unsigned)n_groups), dim3(256), 0, st,
                       jb, gr, N, T, succ);
  else if (trailing)
    hipLaunchKernelGGL(select_succ_kernel<MI>, dim3((unsigned)bpj, (unsigned)pass_n), dim3(256), 0, st,
                       jb, pass_groups, N, T, succ);
  return hipGetLastError();
}

hipError_t launch_select_ranks(void *jobs, int n_jobs, const void *groups, int n_groups,
                               const int32_t *h_groups, void *groups_scratch, int max_inc,
                               bool untracked, int64_t N, int64_t T, unsigned int *hist, double *out,
                               unsigned long long *succ, unsigned long long *cand,
                               unsigned int *cand_count, hipStream_t st) {
  if (n_jobs <= 0 || n_groups <= 0 || N * T <= 0) return hipSuccess;
  SelJob *jb = static_cast<SelJob *>(jobs);
  const int2 *gr = static_cast<const int2 *>(groups);
  int2 *ga = static_cast<int2 *>(groups_scratch);
  switch (max_inc) {
    case 0: return select_ranks_mi<0>(jb, n_jobs, gr, n_groups, h_groups, ga, untracked, N, T, hist, out, succ, cand, cand_count, st);
    case 1: return select_ranks_mi<1>(jb, n_jobs, gr, n_groups, h_groups, ga, untracked, N, T, hist, out, succ, cand, cand_count, st);
    case 2: return select_ranks_mi<2>(jb, n_jobs, gr, n_groups, h_groups, ga, untracked, N, T, hist, out, succ, cand, cand_count, st);
    default: return select_ranks_mi<kMaxInc>(jb, n_jobs, gr, n_groups, h_groups, ga, untracked, N, T, hist, out, succ, cand, cand_count, st);
  }
}

}  // namespace fr
