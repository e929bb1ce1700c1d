// HIP kernels of the ISS hot path for gfx950 (CDNA4, wave64).
//
// iss_walk_kernel: one 256-thread workgroup per (series n, group of sub-tries).
//   * the X rows (and exp tables) the words reference are staged ONCE per time
//     chunk into LDS with coalesced 16-byte loads;
//   * the workgroup walks the prefix trie in DFS order; the running exclusive
//     prefix of every open ancestor lives in registers (one "frame" per level);
//   * per node: multiply / divide the letters into the parent's prefix in the
//     reference's order (fruits/iss/semiring.py:143-149), then an inclusive
//     scan along time = thread-local sums -> wave64 DPP scan -> LDS cross-wave
//     offsets (+ the carry of earlier chunks), emit with 16-byte coalesced
//     stores into the reference's (K,N,T) layout (fruits/iss/iss.py:46).
// The kernel is HBM-bound (one write per output element, X read once per
// group); there is no contraction anywhere, so no MFMA.
#pragma once
#include "walk_types.h"
#include "walk_units.h"
#include "walk_scan.h"

namespace fr {

// ---------------------------------------------------------------- walk kernel
// Time layout of one chunk: wave w owns the contiguous span [w*SPAN, (w+1)*SPAN);
// the span is P pieces of 64*E elements; lane l holds E consecutive elements of
// every piece.  So every 16-byte global access of a wave is lane-contiguous
// (E = 2: 1 KiB per instruction) and only NW wave totals cross waves.
template <int E_, int P_, int MAXLV_, int MULTI_, bool VEC_, bool WEIGHTED_, int TEAM_ = 4,
          int MODE_ = 0, int SEMI_ = 0, bool NT_ = false, bool TOTALINC_ = false,
          bool HIGHORD_ = false, int WT_ = 0>
struct WalkCfg {
  // TOTALINC: fused epilogue of a TOTALLY weighted plan with differencing sieves - the
  // increments need the weight one step to the left (previous_weighted).  Its own
  // instantiation: compiled into the common weighted kernels it costs them 130-400 more
  // SGPR spills and 20 % of their speed (config 4: 21.5 -> 26.5 ms).
  static constexpr bool TOTALINC = TOTALINC_;
  // HIGHORD: fused epilogue with differencing orders >= 3 on series of SEVERAL time chunks (a
  // carry per order between chunks).  Its own instantiation like TOTALINC: compiled into the
  // common multi-chunk kernels it took them past 128 VGPRs (config 5: 24.9 -> 30.5 ms).
  static constexpr bool HIGHORD = HIGHORD_;
  // NT: the rows of X are staged with non-temporal loads (load_input; the host asks for it
  // when every row is read once per launch and the batch is about the size of the cache)
  static constexpr bool NT = NT_;
  // WT: cache policy of the full-chunk 16-byte stores of the (K,N,T) tensor (emit_store): 0 a
  // plain global store; otherwise the policy operand of a buffer store (kStoreSc1 = write-through,
  // the line is not kept dirty in the XCD's L2; kStoreNtSc1 = the same, non-temporal).  Ragged
  // chunks keep plain 8- and 16-byte stores; feature rows of the fused walk never use it.
  static constexpr int WT = WT_;
  // SEMI 0: Reals (+, x) with an exclusive shift between letters; SEMI 1: Arctic
  // (max, +), letters add el * x and children continue from the INCLUSIVE maximum;
  // SEMI 2: Bayesian (max, x): the letters and weights of Reals, the scan of Arctic
  static constexpr int SEMI = SEMI_;
  // MODE 0: write the (K,N,T) tensor.  MODE 1: fused sieve epilogue - the values of
  // a node go straight into NPI / MPI / END features, no tensor is written.
  static constexpr int MODE = MODE_;
  // TEAM waves scan one row together.  TEAM = 4: the whole workgroup works on one
  // (series, group) unit and waves exchange totals through LDS once per node.
  // TEAM = 1: every wave scans whole rows alone (no barrier, no LDS exchange) and
  // the 4 waves of a workgroup walk 4 different groups of the SAME series, so they
  // still share the staged rows.
  static constexpr int TEAM = TEAM_;
  static constexpr int TEAMS = (kWalkThreads / 64) / TEAM_;
  static constexpr bool WEIGHTED = WEIGHTED_;  // exp tables in play (emit_mul / z_mul)
  static constexpr bool VEC = VEC_;      // 16-byte global accesses are aligned
  static constexpr int E = E_;          // contiguous elements per lane per piece
  static constexpr int P = P_;          // pieces per wave
  static constexpr int EP = E_ * P_;
  static constexpr int MAXLV = MAXLV_;
  // more than one time chunk: 0 no, 1 per-node carries in LDS, 2 carries in global memory
  // (a global carry load is a vector load: waiting for it also waits for every output
  // store in flight, so LDS is preferred whenever the group's carries fit)
  static constexpr int MULTI = MULTI_;
  static constexpr int NW = TEAM_;
  static constexpr int PIECE = 64 * E_;          // elements per wave piece
  static constexpr int SPAN = PIECE * P_;        // elements per wave
  static constexpr int CHUNK = SPAN * NW;        // elements per time chunk
};

// LDS position of chunk element i (i even: 16-byte units never straddle).  For
// E = 4 the two halves of a lane's 4 elements live in two planes so that every
// ds_read_b128 of a wave is lane-contiguous (bank-conflict free).
template <class C>
__device__ __forceinline__ int lds_pos(int i) {
  if constexpr (C::E == 2) {
    return i;
  } else {
    static_assert(C::E == 4, "E must be 2 or 4");
    const int blk = i >> 8, r = i & 255;
    return (blk << 8) + ((r & 2) << 6) + ((r >> 2) << 1) + (r & 1);
  }
}

constexpr int kCarrySlots = 3;  // per node: scan, second scan (non-total), d1 tail (inc = 2)
// fused walk, series of several chunks (WalkCfg::HIGHORD): a slot pair per differencing order
// 3 .. 8 at kCarrySlots + 2 (k - 3), and per cumulation 1 .. 8 (inc < 0) from kCumCarryBase on
constexpr int kCumCarryBase = kCarrySlots + 2 * 6;
constexpr int kCarrySlotsAll = kCumCarryBase + 2 * 8;
constexpr int kStageRows = 3;  // rows staged per batch (registers: 4 * U VGPRs per row)

struct WalkCtx {
  const IssArgs *a;
  const double *rows;   // LDS: staged rows [R][CHUNK]
  double *tot;          // LDS: wave totals [2][NW]
  double *tail;         // LDS: last first-difference of every wave [2][NW] (fused inc = 2)
  int tail_buf;
  int slot;             // carry slot base of the node being processed
  int parity;           // fused walk: time chunk & 1 (the carries of differencing orders >= 3 have two
                        // buffers: several ops of a node read the old one and write the same new one)
  double *out_base;     // out + n*out_n_stride + t0
  double *feat_row;     // MODE 1: feats + n*feat_stride
  double *cnt_row;      // MODE 1: band population of MPI features
  // MODE 1, cooperative kernels: the features of a unit accumulate in an LDS window (value and
  // MPI population of every slot) and leave with plain stores (feat_flush); a unit owns its
  // feature columns, so nothing in global memory is ever added to atomically
  lds_f64 *fl_val;
  lds_f64 *fl_cnt;
  int fslot;            // first window slot of the node being processed
  int fused_used;       // slots of the window in use
  int frow0;            // the window's first output row: its position in IssArgs::slot_rows (feat_flush)
  int feat_window;      // slots of the window (a huge number when every group's features fit)
  int64_t series;          // MODE 1: index of the series being walked
  double *carry;        // carry slots of this series (multi-chunk; LDS or global) or nullptr
  int64_t t0;           // first time index of the chunk
  int tid, lane, wave, team;   // wave = index inside the team
  int pc_begin;                // first record of the group being walked
  int buf;
  int next_unit;               // static programs: the series whose rows are loaded next
  bool have_rows;              // static programs: the unit's rows are already in registers
  bool first_chunk;
  bool full_chunk;      // every element of the chunk is < T (no per-lane bounds checks)
#ifdef FRUITS_HIP_TIMING_BUILD
  unsigned long long seg[8];   // s_memtime sums per code segment (diagnostic build only)
  unsigned long long last;
#endif
};

#ifdef FRUITS_HIP_TIMING_BUILD
__device__ __forceinline__ unsigned long long stamp_now() {
  unsigned long long t;
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  __builtin_amdgcn_sched_barrier(0);
  return t;
}
#define STAMP(cx, i)                                  \
  do {                                                \
    if ((cx).a->debug & 16) {                         \
      const unsigned long long t_ = stamp_now();      \
      (cx).seg[i] += t_ - (cx).last;                  \
      (cx).last = t_;                                 \
    }                                                 \
  } while (0)
#else
#define STAMP(cx, i) do { } while (0)
#endif

// 16 bytes of an input row.  With one group per series every input element is read exactly
// once per launch: a NON-TEMPORAL load then keeps it from allocating in the Infinity Cache,
// where it would only evict output lines (measured with a pure data mover of the headline's
// traffic, tools/stream_mix.hip: 64 -> 51 us at 352 MB; no difference beyond 1 GB).
// Compile-time: a run-time select of the two loads is folded into one plain load.
template <bool NT>
__device__ __forceinline__ vd2 load_input(const double *p) {
  const vd2 *q = reinterpret_cast<const vd2 *>(p);
  if constexpr (NT) return __builtin_nontemporal_load(q);
  return *q;
}

// reads the lane's EP elements of staged row `row`
template <class C>
__device__ __forceinline__ void read_row(const WalkCtx &cx, int row, double (&v)[C::EP]) {
  constexpr int E = C::E, P = C::P;
  const double *base = cx.rows + row * C::CHUNK + cx.wave * C::SPAN;
#pragma unroll
  for (int h = 0; h < P; ++h) {
    if constexpr (E == 2) {
      const vd2 q = *reinterpret_cast<const vd2 *>(base + h * C::PIECE + cx.lane * 2);
      v[h * 2] = q.x;
      v[h * 2 + 1] = q.y;
    } else {
      const vd2 q0 = *reinterpret_cast<const vd2 *>(base + h * C::PIECE + cx.lane * 2);
      const vd2 q1 = *reinterpret_cast<const vd2 *>(base + h * C::PIECE + 128 + cx.lane * 2);
      v[h * 4] = q0.x;
      v[h * 4 + 1] = q0.y;
      v[h * 4 + 2] = q1.x;
      v[h * 4 + 3] = q1.y;
    }
  }
}

template <class C>
__device__ __forceinline__ void block_scan(WalkCtx &cx, const double (&s)[C::EP],
                                           double (&c)[C::EP], double (&x)[C::EP],
                                           int carry_slot) {
  constexpr int E = C::E, P = C::P, NW = C::NW;
  double l[C::EP];
  double incl[P], excl[P], ptot[P];
#pragma unroll
  for (int h = 0; h < P; ++h) {
    l[h * E] = s[h * E];
#pragma unroll
    for (int e = 1; e < E; ++e) l[h * E + e] = semi_add<C::SEMI>(l[h * E + e - 1], s[h * E + e]);
  }
#pragma unroll
  for (int h = 0; h < P; ++h) incl[h] = l[h * E + E - 1];
  wave_inclusive_scan_multi<P, C::SEMI>(incl);
#pragma unroll
  for (int h = 0; h < P; ++h) {
    excl[h] = wave_shift_right1<C::SEMI>(incl[h]);
    ptot[h] = wave_last_lane(incl[h]);
  }
  double carry_in = semi_zero<C::SEMI>();
  if constexpr (C::MULTI != 0) {
    if (!cx.first_chunk) carry_in = cx.carry[carry_slot];
  }
  double base = semi_zero<C::SEMI>();
  if constexpr (NW == 1) {
    STAMP(cx, 2);  // local sums + wave scans
    if constexpr (C::MULTI != 0) {
      double total = ptot[0];
#pragma unroll
      for (int h = 1; h < P; ++h) total = semi_add<C::SEMI>(total, ptot[h]);
      base = carry_in;
      if (cx.lane == 0) cx.carry[carry_slot] = semi_add<C::SEMI>(carry_in, total);
    }
  } else {
    double wave_total = ptot[0];
#pragma unroll
    for (int h = 1; h < P; ++h) wave_total = semi_add<C::SEMI>(wave_total, ptot[h]);
    STAMP(cx, 2);  // local sums + wave scans
    double *tot = cx.tot + cx.buf * NW;
    if (cx.lane == 0) tot[cx.wave] = wave_total;
#ifdef FRUITS_HIP_TIMING_BUILD
    if (cx.a->debug & 32)  // timing experiments only: the cost of the rendezvous itself
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    else
#endif
    lds_barrier();
    STAMP(cx, 3);  // LDS write + barrier
    // exclusive prefix of the wave totals
    static_assert(NW == 1 || NW == 4, "cross-wave prefix is written for 4 waves");
    const double t0 = tot[0], t1 = tot[1], t2 = tot[2], t3 = tot[3];
    const double p2 = semi_add<C::SEMI>(t0, t1), p3 = semi_add<C::SEMI>(p2, t2);
    base = cx.wave == 0 ? semi_zero<C::SEMI>() : (cx.wave == 1 ? t0 : (cx.wave == 2 ? p2 : p3));
    cx.buf ^= 1;
    if constexpr (C::MULTI == 1) {
      // LDS carry: every wave read it before the barrier above; one lane updates it
      base = semi_add<C::SEMI>(base, carry_in);
      if (cx.wave == 0 && cx.lane == 0)
        cx.carry[carry_slot] = semi_add<C::SEMI>(carry_in, semi_add<C::SEMI>(p3, t3));
    } else if constexpr (C::MULTI == 2) {
      base = semi_add<C::SEMI>(base, carry_in);
      // every wave stores the same value; a wave only ever re-reads its own store
      if (cx.lane == 0)
        cx.carry[carry_slot] = semi_add<C::SEMI>(carry_in, semi_add<C::SEMI>(p3, t3));
    }
  }
  // The last value of a lane is formed as base + (inclusive wave scan), the first
  // exclusive value of the NEXT lane as base + (that same scan value, shifted): the
  // two are bit-identical, so the stored row and the exclusive prefixes handed to
  // children / sieves are consistent across lanes and pieces (an increment that the
  // running sum absorbs is exactly 0, as in a sequential cumsum).
#pragma unroll
  for (int h = 0; h < P; ++h) {
    const double off = semi_add<C::SEMI>(base, excl[h]);
    x[h * E] = off;
#pragma unroll
    for (int e = 0; e + 1 < E; ++e) {
      c[h * E + e] = semi_add<C::SEMI>(off, l[h * E + e]);
      x[h * E + e + 1] = c[h * E + e];
    }
    c[h * E + E - 1] = semi_add<C::SEMI>(base, incl[h]);
    base = semi_add<C::SEMI>(base, ptot[h]);
  }
  STAMP(cx, 4);  // cross-wave prefix + final adds
}

// Cache-policy operands of a gfx950 buffer store (WalkCfg::WT): sc1 writes through the XCD's L2
// instead of leaving the line dirty there; nt sc1 also marks it non-temporal
constexpr int kStorePlain = 0, kStoreSc1 = 16, kStoreNtSc1 = 18;

typedef unsigned int vu4 __attribute__((ext_vector_type(4)));

// 16 bytes of output with the cache policy WT: `rs` is a wave-uniform descriptor of the output
// bytes, `off` the lane's byte offset in them
template <int WT>
__device__ __forceinline__ void store_policy(__amdgpu_buffer_rsrc_t rs, uint32_t off, vd2 v) {
  vu4 bits;
  __builtin_memcpy(&bits, &v, 16);
  __builtin_amdgcn_raw_buffer_store_b128(bits, rs, off, 0, WT);
}

template <class C>
__device__ __forceinline__ void emit_store(const WalkCtx &cx, const double (&v)[C::EP],
                                           double *dst) {
  constexpr int E = C::E, P = C::P;
  const int64_t T = cx.a->T;
#ifdef FRUITS_HIP_TIMING_BUILD
  // timing experiments only: keep the arithmetic alive, drop the stores
  if ((cx.a->debug & 1) && v[0] != 1.2345678e300) return;
#endif
  if constexpr (C::VEC) {
    if (cx.full_chunk) {
      // the common case, decided once per chunk: no per-lane bounds checks (each would
      // cost an exec-mask save / branch / restore around every store)
      if constexpr (C::WT != kStorePlain) {
        // one descriptor per row: `dst` is wave-uniform and the chunk's CHUNK elements are in
        // bounds (stride 0, size in bytes; 0x20000: dword 3 of a raw gfx9 buffer, 32-bit format)
        const __amdgpu_buffer_rsrc_t rs =
            __builtin_amdgcn_make_buffer_rsrc(dst, 0, C::CHUNK * (int)sizeof(double), 0x00020000);
#pragma unroll
        for (int h = 0; h < P; ++h) {
          const int idx = cx.wave * C::SPAN + h * C::PIECE + cx.lane * E;
#pragma unroll
          for (int e = 0; e < E; e += 2)
            store_policy<C::WT>(rs, (uint32_t)(idx + e) * 8u, vd2{v[h * E + e], v[h * E + e + 1]});
        }
        return;
      }
#pragma unroll
      for (int h = 0; h < P; ++h) {
        const int idx = cx.wave * C::SPAN + h * C::PIECE + cx.lane * E;
#pragma unroll
        for (int e = 0; e < E; e += 2)
          *reinterpret_cast<vd2 *>(dst + idx + e) = vd2{v[h * E + e], v[h * E + e + 1]};
      }
      return;
    }
  }
#pragma unroll
  for (int h = 0; h < P; ++h) {
    const int idx = cx.wave * C::SPAN + h * C::PIECE + cx.lane * E;
    if constexpr (C::VEC) {
#pragma unroll
      for (int e = 0; e < E; e += 2) {
        const vd2 val = {v[h * E + e], v[h * E + e + 1]};
        if (cx.t0 + idx + e < T) *reinterpret_cast<vd2 *>(dst + idx + e) = val;
      }
    } else {
#pragma unroll
      for (int e = 0; e < E; ++e)
        if (cx.full_chunk || cx.t0 + idx + e < T) dst[idx + e] = v[h * E + e];
    }
  }
}

// a NodeRec in registers (all wave-uniform, i.e. SGPRs)
struct Rec {
  int32_t w[16];
  __device__ __forceinline__ int level() const { return w[0] & 0xff; }
  __device__ __forceinline__ int flags() const { return w[0] >> 8; }
  __device__ __forceinline__ int fac_count() const { return w[1] & 0xffff; }
  __device__ __forceinline__ int emit_count() const { return w[6]; }
  __device__ __forceinline__ int node_id() const { return w[9]; }
  __device__ __forceinline__ int emit_mul() const { return w[10]; }
  __device__ __forceinline__ int z_mul() const { return w[11]; }
  __device__ __forceinline__ int fac_begin() const { return w[12]; }
  __device__ __forceinline__ int emit_begin() const { return w[13]; }
};

__device__ __forceinline__ Rec load_rec(const NodeRec *recs, int pc) {
  // uniform, 64-byte aligned address in the constant address space -> one
  // s_load_dwordx16; issued one node ahead of its use (see walk)
  cptr<int32_t> q = as_const(reinterpret_cast<const int32_t *>(
      __builtin_assume_aligned(recs + pc, 64)));
  Rec r;
#pragma unroll
  for (int i = 0; i < 16; ++i) r.w[i] = q[i];
  return r;
}

// s (x)= factor.  Reals: s *= row.  Arctic: s += el * row with the multiplier in bits
// 8-15 of the code; the product is rounded before the add like the reference's
// `tmp + el * Z[dim]` (no fused multiply-add), so max-plus results are bit-exact.
template <class C>
__device__ __forceinline__ void mul_row(const WalkCtx &cx, int code, double (&s)[C::EP]) {
  double v[C::EP];
  read_row<C>(cx, code & FAC_ROW_MASK, v);
  if constexpr (C::SEMI != 1) {
#pragma unroll
    for (int i = 0; i < C::EP; ++i) s[i] = s[i] * v[i];
  } else {
#pragma clang fp contract(off)  // the product must round before the add (no FMA)
    const double el = (double)(int)(int8_t)((code >> 8) & 0xff);
#pragma unroll
    for (int i = 0; i < C::EP; ++i) {
      const double prod = el * v[i];
      s[i] = s[i] + prod;
    }
  }
}

// Letters with a reciprocal factor or more than kRecInlineFactors factors: walk
// the factor table (codes row | FAC_DIV), one factor at a time, in order.
template <class C>
__device__ __forceinline__ void slow_factors(const WalkCtx &cx, int fac_begin, int nf,
                                          double (&s)[C::EP], const double (&pin)[C::EP],
                                          bool letter_sum) {
  bool folded = !letter_sum;
  for (int f = 0; f < nf; ++f) {
    const int code = as_const(cx.a->factors)[fac_begin + f];
    if constexpr (C::SEMI == 1) {
      if (!folded && (code & FAC_FOLD)) {   // prefix + (sum of the letter's terms), then weights
#pragma unroll
        for (int i = 0; i < C::EP; ++i) s[i] = pin[i] + s[i];
        folded = true;
      }
      mul_row<C>(cx, code, s);
      continue;
    }
    double v[C::EP];
    read_row<C>(cx, code & FAC_ROW_MASK, v);
    if (code & FAC_DIV) {
#pragma unroll
      for (int i = 0; i < C::EP; ++i) s[i] = s[i] / v[i];
    } else {
#pragma unroll
      for (int i = 0; i < C::EP; ++i) s[i] = s[i] * v[i];
    }
  }
  if constexpr (C::SEMI == 1) {
    if (!folded) {
#pragma unroll
      for (int i = 0; i < C::EP; ++i) s[i] = pin[i] + s[i];
    }
  }
}

// Address of output row k of the current series / chunk.  Rows are at most 4 GiB apart in
// every layout the host code uses, so the byte offset is ONE 32 x 32 -> 64 bit scalar
// multiply (the general 64 x 64 product costs ten scalar instructions per emitted row).
__device__ __forceinline__ double *emit_ptr(const WalkCtx &cx, int k) {
  const IssArgs &a = *cx.a;
  if (a.k_stride_bytes32 != 0) {
    const uint64_t off = (uint64_t)(uint32_t)k * (uint64_t)a.k_stride_bytes32;
    return reinterpret_cast<double *>(reinterpret_cast<char *>(cx.out_base) + off);
  }
  return cx.out_base + (int64_t)k * a.out_k_stride;
}

// `more` / `n_more`: further output rows of a STATIC program's node (compile-time constants,
// kSchedEmits entries); the interpreter reads rows beyond the inline two from the table
template <class C>
__device__ __forceinline__ void emit_all(const WalkCtx &cx, const Rec &nd,
                                         const double (&c)[C::EP], const int32_t *more = nullptr,
                                         int n_more = 0) {
  const IssArgs &a = *cx.a;
  const int ne = nd.emit_count();
  if (ne > 0) emit_store<C>(cx, c, emit_ptr(cx, nd.w[7]));
  if (ne > 1) {
    emit_store<C>(cx, c, emit_ptr(cx, nd.w[8]));
    for (int j = kRecInlineEmits; j < ne; ++j)
      emit_store<C>(cx, c, emit_ptr(cx, as_const(a.emit_rows)[nd.emit_begin() + j]));
  }
  for (int j = 0; j < n_more; ++j) emit_store<C>(cx, c, emit_ptr(cx, more[j]));
}

// ---------------------------------------------------------------- fused sieves
// Features of ONE output row k from the node's inclusive values c and their
// exclusive shifts x (x[t] = c[t-1]): what IncrementSieve._pre_transform +
// NPI/MPI._backend (fruits/sieving/increment.py:63-71,107-163) and END._transform
// (fruits/sieving/segment.py:210-219) compute on the materialised row.  The host
// flattens the sieves of row k into n_ops fixed-size "feature ops" (FeatOp) whose
// cuts and fitted thresholds are already resolved, so one scalar load per op
// brings everything and there are no dependent table look-ups.
//
// ONE evaluator (fop) serves every kernel with a fused epilogue: the cooperative fused walk
// (walk_fused.h), the wave-per-series kernel (walk_packed.h) and both CosWISS kernels (coswiss.h).
// What a family decides for itself:
//   * where a result goes (feat_put_*): a slot of the LDS feature window (TEAM 4; feat_flush
//     writes it to its column) or, where one wave holds the whole row (TEAM 1), the series'
//     feature and population rows directly;
//   * the policy EPI: the scan a cumulation (inc < 0) takes and the node's carry slot of the CPV
//     exchange - RowEpilogue below (packed, CosWISS), WindowEpilogue of walk_fused.h.

// feature-op flags (FeatOp::kind_inc), resolved by the host (capi_pipeline.cpp, fr_pipeline_set_quantiles)
constexpr int32_t OPF_SERIES_CUTS = 1 << 16;   // lo / hi name slots of the series' cut row
// bits 20-22: the op's SHAPE when it is one of the common ones (0: none of them)
constexpr int OPF_SHAPE_SHIFT = 20;
constexpr int OPF_SHAPE_END = 1;     // END at a fixed index (lo)
constexpr int OPF_SHAPE_BAND1 = 2;   // NPI over the whole series, qlo < v (qhi = +inf); | 1: of the first differences
constexpr int OPF_SHAPE_BAND2 = 4;   // NPI over the whole series, qlo < v <= qhi;       | 1: of the first differences

// Single-lane LDS operations of a whole wave in uniform control flow (EXEC all ones before and
// after): the lane is selected by writing EXEC, not by a compare + saved mask + branch - two
// scalar instructions, no mask registers kept alive.  `off` is an LDS BYTE address.
__device__ __forceinline__ void lds_store_lane63(int off, double v) {
  asm volatile("s_lshl_b64 exec, 1, 63\n\tds_write_b64 %0, %1\n\ts_mov_b64 exec, -1"
               :: "v"(off), "v"(v) : "memory", "scc");   // (s_lshl_b64 writes SCC)
}
__device__ __forceinline__ void lds_store_lane(int lane, int off, double v) {
  asm volatile("s_lshl_b64 exec, 1, %2\n\tds_write_b64 %0, %1\n\ts_mov_b64 exec, -1"
               :: "v"(off), "v"(v), "s"(__builtin_amdgcn_readfirstlane(lane)) : "memory", "scc");
}
__device__ __forceinline__ void lds_store_lane0_i32(int off, int v) {
  asm volatile("s_mov_b64 exec, 1\n\tds_write_b32 %0, %1\n\ts_mov_b64 exec, -1"
               :: "v"(off), "v"(v) : "memory");
}
__device__ __forceinline__ void lds_add_lane0(int off, double v) {
  asm volatile("s_mov_b64 exec, 1\n\tds_add_f64 %0, %1\n\ts_mov_b64 exec, -1"
               :: "v"(off), "v"(v) : "memory");
}
__device__ __forceinline__ void lds_add_lane63(int off, double v) {
  asm volatile("s_lshl_b64 exec, 1, 63\n\tds_add_f64 %0, %1\n\ts_mov_b64 exec, -1"
               :: "v"(off), "v"(v) : "memory", "scc");
}
__device__ __forceinline__ void lds_add2_lane63(int off0, double v0, int off1, double v1) {
  asm volatile("s_lshl_b64 exec, 1, 63\n\tds_add_f64 %0, %1\n\tds_add_f64 %2, %3\n\ts_mov_b64 exec, -1"
               :: "v"(off0), "v"(v0), "v"(off1), "v"(v1) : "memory", "scc");
}
__device__ __forceinline__ int lds_offset(const void __attribute__((address_space(3))) *p) {
  return (int)(unsigned)(__UINTPTR_TYPE__)p;
}

// The kernel arguments as seen from code that rarely runs (flushes, reciprocal factors, further
// output rows, per-series cuts): read through a pointer the optimiser cannot look through, so
// that they are loaded where they are used instead of being hoisted out of the node loop into
// scalar registers - there are only 102 of those, and the hot path needs them.
// (The IssArgs struct is the only argument of every kernel with a fused epilogue: it starts the
// kernel-argument segment.)
__device__ __forceinline__ cptr<IssArgs> cold_args() {
  cptr<IssArgs> ap = (cptr<IssArgs>)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(ap));
  return ap;
}
// this series' row of IssArgs::series_cuts (ops with OPF_SERIES_CUTS: coquantile positions,
// per-series lengths) - the one place series cuts are resolved
__device__ __forceinline__ cptr<int32_t> series_cut_row(const WalkCtx &cx, cptr<IssArgs> ca = cold_args()) {
  return as_const(ca->series_cuts + cx.series * ca->cut_slots);
}

__device__ __forceinline__ double bits_to_double(int lo, int hi) {
  return __hiloint2double(hi, lo);
}

// First differences d1[t] = c[t] - c[t-1] of the element BEFORE each of the lane's
// elements (second differences need them): inside a lane the neighbour, across lanes
// a DPP shift, across pieces lane 63, across waves an LDS exchange (one extra barrier,
// taken by every wave since the op list is uniform), across chunks a carry slot.
// `carry_at`: the node's carry slot of this exchange (2: the first differences' - advanced once
// per node and chunk, FusedScratch); `two_buffers` (orders >= 3 of the fused walk): the slot pair
// carry_at, carry_at + 1 - this chunk reads buffer `parity` and writes the other.
template <class C>
__device__ __forceinline__ void prev_first_differences(WalkCtx &cx, const double (&d1)[C::EP],
                                                       double (&dp)[C::EP], int carry_at = 2,
                                                       bool two_buffers = false) {
  constexpr int E = C::E, P = C::P, NW = C::NW;
  const int rd = cx.slot + carry_at + (two_buffers ? cx.parity : 0);
  const int wr = cx.slot + carry_at + (two_buffers ? (cx.parity ^ 1) : 0);
  (void)rd;
  (void)wr;
  double last[P];
#pragma unroll
  for (int h = 0; h < P; ++h) {
    last[h] = wave_last_lane(d1[h * E + E - 1]);
    const double from_left = wave_shift_right1<0>(d1[h * E + E - 1]);
    dp[h * E] = from_left;
#pragma unroll
    for (int e = 1; e < E; ++e) dp[h * E + e] = d1[h * E + e - 1];
  }
  double before_wave = 0.0;  // d1 of the element just before this wave's span
  if constexpr (NW > 1) {
    double *tl = cx.tail + cx.tail_buf * NW;
    if (cx.lane == 0) tl[cx.wave] = last[P - 1];
    lds_barrier();
    if (cx.wave > 0) before_wave = tl[cx.wave - 1];
    cx.tail_buf ^= 1;
    if constexpr (C::MULTI != 0) {
      const double carried = cx.first_chunk ? 0.0 : cx.carry[rd];
      if (cx.wave == 0) before_wave = carried;
      const double chunk_last = tl[NW - 1];
      if (C::MULTI == 1 ? (cx.wave == 0 && cx.lane == 0) : (cx.lane == 0))
        cx.carry[wr] = chunk_last;
    }
  } else if constexpr (C::MULTI != 0) {
    before_wave = cx.first_chunk ? 0.0 : cx.carry[rd];
    if (cx.lane == 0) cx.carry[wr] = last[P - 1];
  }
  if (cx.lane == 0) {
    dp[0] = before_wave;
#pragma unroll
    for (int h = 1; h < P; ++h) dp[h * E] = last[h - 1];
  }
}

// per-node scratch of the epilogue: the previous first differences are computed (and
// their chunk carry advanced) at most once per node, whatever the number of inc = 2 ops
template <int EP>
struct FusedScratch {
  double dp[EP];
  bool have_dp = false;
  // CPV: the value of the row one element to the left, exchanged once per node
  double cp[EP];
  bool have_cp = false;
};

// The epilogue policy of the kernels that hold a whole record (wave-per-series kernel, CosWISS):
// a cumulation is a block_scan - one-chunk series only, the host refuses longer ones: every
// cumulation would need a carry of its own -, the CPV exchange carries in the node's slot 3.
// No short paths for the shapes the host flags (OPF_SHAPE_*): these kernels never took them, and
// with them the deep wave-per-series instances need four more VGPRs (an occupancy step).
struct RowEpilogue {
  template <class CR>
  static __device__ __forceinline__ void cumulate(WalkCtx &cx, int, const double (&d)[CR::EP],
                                                  double (&cs)[CR::EP]) {
    double xs[CR::EP];
    block_scan<CR>(cx, d, cs, xs, 0);
  }
  static constexpr bool short_paths = false;
  static __device__ __forceinline__ int cpv_slot() { return 3; }
};

// Where a result goes (see above).  Counts are the same in every lane; a sum is its wave's total
// in lane 63 (wave_inclusive_scan); a key is the wave's largest in every lane.
template <class C>
__device__ __forceinline__ void feat_put_count(WalkCtx &cx, int slot, int col, int cnt) {
  if constexpr (C::TEAM != 1) lds_add_lane0(lds_offset(cx.fl_val + slot), (double)cnt);
  else if (cx.lane == 0) cx.feat_row[col] = (double)cnt;
}
template <class C>
__device__ __forceinline__ void feat_put_sum(WalkCtx &cx, int slot, int col, double sum) {
  if constexpr (C::TEAM != 1) lds_add_lane63(lds_offset(cx.fl_val + slot), sum);
  else if (cx.lane == 63) cx.feat_row[col] = sum;
}
template <class C>
__device__ __forceinline__ void feat_put_mean(WalkCtx &cx, int slot, int col, double sum, int cnt) {
  if constexpr (C::TEAM != 1) {
    // one LDS instruction pair per wave (ds_add_f64, nothing returned)
    lds_add2_lane63(lds_offset(cx.fl_val + slot), sum, lds_offset(cx.fl_cnt + slot), (double)cnt);
  } else if (cx.lane == 63) {
    cx.feat_row[col] = sum;
    cx.cnt_row[col] = (double)cnt;
  }
}
template <class C>
__device__ __forceinline__ void feat_put_key(WalkCtx &cx, int slot, int col, uint64_t key) {
  if (cx.lane == 0) {
    // (one ds_max_u64; the flush combines a window's keys with the row's by maximum)
    if constexpr (C::TEAM != 1) lds_max_u64(cx.fl_val + slot, key);
    else cx.feat_row[col] = __builtin_bit_cast(double, key);
  }
}

// c[eu] for a uniform eu: a chain of uniform branches (the empty asm keeps the arms apart: as
// selects, or as an index, the compiler would send the whole array through scratch memory)
template <int EP, int K>
__device__ __forceinline__ double pick_uniform(int eu, const double (&c)[EP]) {
  if constexpr (K + 1 >= EP) {
    return c[K];
  } else {
    double v;
    if (eu == K) {
      v = c[K];
      asm volatile("" : "+v"(v));
    } else {
      v = pick_uniform<EP, K + 1>(eu, c);
    }
    return v;
  }
}

// END: the value at series index `pick`
template <class C>
__device__ __forceinline__ void end_pick(WalkCtx &cx, int pick, int slot, int col,
                                         const double (&c)[C::EP]) {
  constexpr int E = C::E;
  const unsigned rel = (unsigned)(pick - (int)cx.t0);
  if (rel >= (unsigned)C::CHUNK) return;           // another time chunk's element
  if ((int)(rel / C::SPAN) != cx.wave) return;     // another wave's
  // the position is uniform: uniform selects of the register, ONE lane stores
  const unsigned q = rel % C::SPAN, r = q % C::PIECE;   // (piece q / PIECE, lane r / E, element r % E)
  const double v = pick_uniform<C::EP, 0>((int)(q / C::PIECE * E + r % E), c);
  if constexpr (C::TEAM != 1) lds_store_lane((int)(r / E), lds_offset(cx.fl_val + slot), v);
  else if (cx.lane == (int)(r / E)) cx.feat_row[col] = v;
}

// series index of the lane's element (h = 0, e = 0); element (h, e) is h * PIECE + e behind it
template <class C>
__device__ __forceinline__ int first_index(const WalkCtx &cx) {
  return (int)cx.t0 + cx.wave * C::SPAN + cx.lane * C::E;
}

// The band of an op: segment [lo, hi) x thresholds (qlo, qhi].  `count`: the elements of the wave
// inside, element by element (the AND of the compare masks: as one predicate it goes through a
// vector register).
struct Band {
  int lo, hi;
  double qlo, qhi;
  __device__ __forceinline__ bool in(int t, double v) const {
    return t >= lo && t < hi && qlo < v && v <= qhi;
  }
  __device__ __forceinline__ int count(int t, double v) const {
    return __popcll(__ballot(t >= lo && t < hi) & __ballot(qlo < v) & __ballot(v <= qhi));
  }
};

// PPV / CPV (fruits/sieving/implicit.py:114-129, 169-190): the indicator is closed BELOW -
// v >= qlo, or with OPF_SEGMENTS qlo <= v < qhi, a conjunction per element (the thresholds are
// not sorted: a band with qlo > qhi is empty; a NaN is never in, +inf is in above a finite qlo).
// PPV counts it; CPV counts its rising edges at t >= 1 - the first difference of the indicator
// is zero-padded (fruits/cache.py:8-13), a component that starts at t = 0 is not counted.  The
// indicator at t - 1 is taken from the VALUE the row holds there (c, what MODE 2 stores): the
// lane's own register, the neighbour lane's, the wave's in front through LDS, and across time
// chunks the node's carry slot EPI::cpv_slot().  The exchange is made once per node and chunk,
// whatever the number of CPV ops (FusedScratch, like the first differences of the inc = 2 ops),
// so one slot does.  Counts are integers; implicit_finalize_kernel divides them.  `hi`: T, or
// with OPF_SERIES_CUTS the slot of the series' own length.
template <class C, class EPI, class W>
__device__ __forceinline__ void fop_implicit(WalkCtx &cx, W w, int slot,
                                             const double (&c)[C::EP], FusedScratch<C::EP> &sc) {
  constexpr int E = C::E, P = C::P;
  const bool cpv = (w[0] & 0xff) == FR_SIEVE_CPV_K, seg = (w[0] & OPF_SEGMENTS) != 0;
  int hi = w[3];
  if ((w[0] & OPF_SERIES_CUTS) != 0) hi = series_cut_row(cx)[w[3]];
  const double qlo = bits_to_double(w[4], w[5]), qhi = bits_to_double(w[6], w[7]);
  if (cpv && !sc.have_cp) {
    int at = 0;
    if constexpr (C::MULTI != 0) at = EPI::cpv_slot();
    prev_first_differences<C>(cx, c, sc.cp, at);   // cp[t] = c[t - 1]
    sc.have_cp = true;
  }
  const auto inside = [&](double v) { return seg ? (qlo <= v && v < qhi) : (v >= qlo); };
  const int t_first = first_index<C>(cx);
  int cnt = 0;
#pragma unroll
  for (int h = 0; h < P; ++h)
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int t = t_first + h * C::PIECE + e;
      bool in = inside(c[h * E + e]);
      if (cpv) in = in && !inside(sc.cp[h * E + e]) && t >= 1;
      cnt += __popcll(__ballot(in && t < hi));
    }
  feat_put_count<C>(cx, slot, w[1], cnt);
}

// First differences d[t] = c[t] - c[t-1], zero-padded at element 0 of the series
// (fruits/cache.py:8-13).  `s` is the scan input the values came from (c = cumsum(s)) when
// seq_steps.  Then a Reals first difference is formed as fl(x + s) - x, the step a SEQUENTIAL
// cumsum takes from the same prefix (np.cumsum in the reference): a summand the running sum
// absorbs gives an increment of exactly 0, as in the reference, where the difference of
// two parallel-scan values is +-1 ulp of noise - which "number of positive increments"
// (NPI with its default q = (0, 1)) would count at random.
template <class C>
__device__ __forceinline__ void first_differences(const WalkCtx &cx, const double (&c)[C::EP],
                                                  const double (&x)[C::EP], const double (&s)[C::EP],
                                                  bool seq_steps, double (&d)[C::EP]) {
#pragma unroll
  for (int i = 0; i < C::EP; ++i) {
    double step = c[i] - x[i];
    if (C::SEMI == 0 && seq_steps) step = (x[i] + s[i]) - x[i];
    d[i] = step;
  }
  d[0] = (cx.first_chunk && cx.wave == 0 && cx.lane == 0) ? 0.0 : d[0];
}

// One feature op on the node's values: w = the op's eight words (FeatOp; loaded by the caller), `slot` its
// window slot.
template <class C, class EPI, class W>
__device__ __forceinline__ void fop(WalkCtx &cx, W w, int slot, const double (&c)[C::EP],
                                    const double (&x)[C::EP], const double (&s)[C::EP],
                                    bool seq_steps, FusedScratch<C::EP> &sc) {
  constexpr int E = C::E, P = C::P, EP = C::EP;
  // The shapes the host flags (OPF_SHAPE_*: END at a fixed index; a counting band over the whole
  // series, of the values or of their first differences, with or without an upper threshold)
  // are short straight-line paths where the family takes them (EPI::short_paths); everything else
  // takes the general one below, which gives the same counts.
  const int shape = EPI::short_paths ? (w[0] >> OPF_SHAPE_SHIFT) & 7 : 0;
  if (shape == OPF_SHAPE_END) {
    end_pick<C>(cx, w[2], slot, w[1], c);
    return;
  }
  if (shape != 0 && cx.full_chunk) {
    const double qlo = bits_to_double(w[4], w[5]);
    double d[EP];
    if (shape & 1) {
      first_differences<C>(cx, c, x, s, seq_steps, d);
    } else {
#pragma unroll
      for (int i = 0; i < EP; ++i) d[i] = c[i];
    }
    int cnt = 0;
    if (shape >= OPF_SHAPE_BAND2) {
      const double qhi = bits_to_double(w[6], w[7]);
#pragma unroll
      for (int i = 0; i < EP; ++i) cnt += __popcll(__ballot(qlo < d[i]) & __ballot(d[i] <= qhi));
    } else {
#pragma unroll
      for (int i = 0; i < EP; ++i) cnt += __popcll(__ballot(qlo < d[i]));
    }
    feat_put_count<C>(cx, slot, w[1], cnt);
    return;
  }
  const int kind = w[0] & 0xff, inc = (int)(int8_t)((w[0] >> 8) & 0xff);   // inc: signed
  const bool series_cuts = (w[0] & OPF_SERIES_CUTS) != 0;
  if (kind == FR_SIEVE_END_K) {
    int pick = w[2];                    // index of the value to pick
    if (series_cuts) {                  // X[:, cut - 1], index -1 wrapping like numpy
      cptr<IssArgs> ca = cold_args();
      pick = series_cut_row(cx, ca)[w[2]] - 1;
      if (pick < 0) pick += (int)ca->T;
    }
    end_pick<C>(cx, pick, slot, w[1], c);
    return;
  }
  if (kind == FR_SIEVE_PPV_K || kind == FR_SIEVE_CPV_K) {
    if constexpr (C::MODE == 1) fop_implicit<C, EPI>(cx, w, slot, c, sc);
    return;
  }
  Band band{w[2], w[3], bits_to_double(w[4], w[5]), bits_to_double(w[6], w[7])};
  if (series_cuts) {
    cptr<int32_t> cut_row = series_cut_row(cx);
    band.lo = cut_row[w[2]];
    band.hi = cut_row[w[3]];
  }
  // element 0 of the series: increments are zero-padded there (fruits/cache.py:8-13)
  const bool at0 = cx.first_chunk && cx.wave == 0 && cx.lane == 0;
  double d[EP];
  if (inc <= 0) {
#pragma unroll
    for (int i = 0; i < EP; ++i) d[i] = c[i];
    if constexpr (C::MULTI == 0 || C::HIGHORD) {
      // inc < 0: the row cumulated -inc times (np.cumsum, fruits/sieving/increment.py:68-70) -
      // a plain sum whatever the semiring of the plan, by the family's scan (EPI::cumulate).  On
      // series of several chunks (WalkCfg::HIGHORD) the j-th cumulation carries its running sum
      // in a slot pair of its own (walk_fused.h, WindowEpilogue).
      using CR = WalkCfg<C::E, C::P, C::MAXLV, C::MULTI, C::VEC, C::WEIGHTED, C::TEAM, C::MODE, 0>;
      for (int k = inc; k < 0; ++k) {
        double cs[EP];
        EPI::template cumulate<CR>(cx, k - inc, d, cs);
#pragma unroll
        for (int i = 0; i < EP; ++i) d[i] = cs[i];
      }
    }
  } else {
    first_differences<C>(cx, c, x, s, seq_steps, d);
    if (inc >= 2) {
      if (!sc.have_dp) {
        prev_first_differences<C>(cx, d, sc.dp);
        sc.have_dp = true;
      }
#pragma unroll
      for (int i = 0; i < EP; ++i) d[i] = d[i] - sc.dp[i];
      d[0] = at0 ? 0.0 : d[0];
      // third to eighth differences (IncrementSieve._pre_transform applies _increments inc times,
      // fruits/sieving/increment.py:63-71): one more neighbour exchange per order; on series of
      // several chunks (WalkCfg::HIGHORD; the host refuses them elsewhere) every order carries its
      // last value of the chunk in a slot pair of its own (IssArgs::carry_per_node =
      // 3 + 2 * (highest order - 2))
      if constexpr (C::MULTI == 0 || C::HIGHORD) {
        for (int k = 3; k <= inc; ++k) {
          double dq[EP];
          prev_first_differences<C>(cx, d, dq, 3 + 2 * (k - 3), C::MULTI != 0);
#pragma unroll
          for (int i = 0; i < EP; ++i) d[i] = d[i] - dq[i];
          d[0] = at0 ? 0.0 : d[0];
        }
      }
    }
  }
  // (the accumulation order inside a lane - pieces outer, elements inner - is part of the bits of
  // the real-valued sums)
  const int t_first = first_index<C>(cx);
  if (kind == FR_SIEVE_MAX_K || kind == FR_SIEVE_MIN_K) {
    // the largest band key of the wave (walk_types.h)
    uint64_t key = 0;
#pragma unroll
    for (int h = 0; h < P; ++h)
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const double v = d[h * E + e];
        const uint64_t kv = band_key(v, kind == FR_SIEVE_MIN_K);
        if (band.in(t_first + h * C::PIECE + e, v) && kv > key) key = kv;
      }
    feat_put_key<C>(cx, slot, w[1], wave_max_u64(key));
    return;
  }
  if (kind == FR_SIEVE_CUR_K) {
    // CUR (fruits/sieving/segment.py:228-272): the sum of the squares inside the band.  No
    // population and nothing to divide: the partial sums of the waves - and, through the flush,
    // of the time chunks - add up like NPI's counts
    double sum = 0.0;
#pragma unroll
    for (int h = 0; h < P; ++h)
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const double v = d[h * E + e];
        sum += band.in(t_first + h * C::PIECE + e, v) ? v * v : 0.0;
      }
    feat_put_sum<C>(cx, slot, w[1], wave_inclusive_scan<0>(sum));
    return;
  }
  // XPI: MPI of the positions relative to the segment start (integer sums: exact in any order).
  // Every op leaves its result, zero counts included: every feature column is written exactly
  // once per series and the feature tensor needs no clearing.
  const bool xpi = kind == FR_SIEVE_XPI_K;
  const bool mpi = kind == FR_SIEVE_MPI_K || xpi;
  int cnt = 0;
  double sum = 0.0;
#pragma unroll
  for (int h = 0; h < P; ++h)
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int t = t_first + h * C::PIECE + e;
      const double v = d[h * E + e];
      if (mpi) {
        const bool in = band.in(t, v);
        cnt += __popcll(__ballot(in));
        sum += in ? (xpi ? (double)(t - band.lo) : v) : 0.0;
      } else {
        cnt += band.count(t, v);
      }
    }
  if (mpi) feat_put_mean<C>(cx, slot, w[1], wave_inclusive_scan<0>(sum), cnt);
  else feat_put_count<C>(cx, slot, w[1], cnt);
}

// Flushes the LDS feature window of a cooperative kernel with plain stores (`add`: onto what
// earlier time chunks of the unit left there - the unit owns its columns, so a plain
// read-modify-write by the thread that wrote them), and clears the window.  The next adds come
// behind the next node's scan barrier.  No columns in the window: a slot is (output row r of the
// unit's walk, op i), its column the one the row's i-th op names; the window's first row is
// position cx.frow0 of IssArgs::slot_rows (GroupedProgram) or, without that table (a plan in
// pieces numbers its output rows in walk order; a CosWISS unit has ONE row), row cx.frow0 itself.
template <class C>
__device__ __forceinline__ void feat_flush(WalkCtx &cx, bool add) {
  lds_barrier();   // the adds of every wave are in
  cptr<IssArgs> ap = cold_args();
  const bool mpi = ap->has_mpi != 0;
  double *feat_row = ap->feats + cx.series * ap->feat_stride;
  double *cnt_row = ap->cnt + cx.series * ap->feat_stride;
  const int n_ops = ap->n_ops;
  for (int sl = cx.tid; sl < cx.fused_used; sl += kWalkThreads) {
    const int r = sl / n_ops, i = sl - r * n_ops;
    const int64_t k = ap->slot_rows != nullptr ? as_const(ap->slot_rows)[cx.frow0 + r] : cx.frow0 + r;
    cptr<FeatOp> op = as_const(ap->ops) + k * ap->n_ops_padded + i;
    const int col = op->col, kind = op->kind_inc & 0xff;
    const bool keyed = kind == FR_SIEVE_MAX_K || kind == FR_SIEVE_MIN_K;   // band keys, walk_types.h
    double v = cx.fl_val[sl];
    if (add) {
      const double before = feat_row[col];
      if (keyed) {   // MAX / MIN keys: the larger one (the window's 0.0 is key 0, the identity)
        if (__builtin_bit_cast(uint64_t, before) > __builtin_bit_cast(uint64_t, v)) v = before;
      } else {
        v = before + v;
      }
    }
    feat_row[col] = v;
    cx.fl_val[sl] = 0.0;
    if (mpi) {
      double n = cx.fl_cnt[sl];
      if (add) n = cnt_row[col] + n;
      cnt_row[col] = n;
      cx.fl_cnt[sl] = 0.0;
    }
  }
  cx.frow0 += cx.fused_used / n_ops;
  cx.fused_used = 0;
}

// Window slots of the next node (`need` = output rows x feature ops); a full window leaves first.
template <class C>
__device__ __forceinline__ void feat_reserve(WalkCtx &cx, int need) {
  if (cx.fused_used + need > cx.feat_window) feat_flush<C>(cx, !cx.first_chunk);
  cx.fslot = cx.fused_used;
  cx.fused_used += need;
}

// Two feature ops of one output row (64 bytes, one scalar load), requested a step ahead of their
// use in the wave-per-series kernel: without this prefetch it waits for every op (measured: 2 % on
// its fused benchmark line).
struct OpPair {
  int32_t w[16];
};
__device__ __forceinline__ OpPair load_op_pair(const IssArgs &a, int64_t k, int first) {
  cptr<int32_t> q = as_const(reinterpret_cast<const int32_t *>(
      __builtin_assume_aligned(a.ops + (k * a.n_ops_padded + first), 64)));
  OpPair o;
#pragma unroll
  for (int i = 0; i < 16; ++i) o.w[i] = q[i];
  return o;
}

// The feature ops of every output row of a node of the wave-per-series kernel.  `pre`: ops 0-1 of
// the first row, requested at the start of the node; the next pair is requested behind the
// current one.  Window slot of (output row j, op i): fslot + j * n + i.
template <class C>
__device__ __forceinline__ void fops_rows_ahead(WalkCtx &cx, const Rec &nd, const OpPair &pre,
                                                const double (&c)[C::EP], const double (&x)[C::EP],
                                                const double (&s)[C::EP], bool seq_steps) {
  const IssArgs &a = *cx.a;
  const int ne = nd.emit_count(), n = a.n_ops;
  int64_t k = nd.w[7];
  OpPair o = pre;
  FusedScratch<C::EP> sc;
  int slot = cx.fslot;
  for (int j = 0;;) {
    for (int i = 0;;) {
      fop<C, RowEpilogue>(cx, o.w, slot + i, c, x, s, seq_steps, sc);
      if (i + 1 < n) fop<C, RowEpilogue>(cx, o.w + 8, slot + i + 1, c, x, s, seq_steps, sc);
      i += 2;
      if (i >= n) break;
      o = load_op_pair(a, k, i);
    }
    if (++j >= ne) break;
    slot += n;
    k = j == 1 ? (int64_t)nd.w[8] : (int64_t)as_const(a.emit_rows)[nd.emit_begin() + j];
    o = load_op_pair(a, k, 0);
  }
}

// The same rows without the prefetch, an op's words read where they are used: CosWISS, whose unit
// is one node with one row - its S+1 scans leave no scalar registers for a pair held ahead (the
// prefetch costs the multi-chunk kernels spills, and nothing in time).
template <class C>
__device__ __forceinline__ void fops_rows(WalkCtx &cx, const Rec &nd, const double (&c)[C::EP],
                                          const double (&x)[C::EP], const double (&s)[C::EP],
                                          bool seq_steps) {
  const IssArgs &a = *cx.a;
  const int ne = nd.emit_count(), n = a.n_ops;
  FusedScratch<C::EP> sc;
  int slot = cx.fslot;
  for (int j = 0; j < ne; ++j, slot += n) {
    const int64_t k = j == 0 ? (int64_t)nd.w[7]
                             : (j == 1 ? (int64_t)nd.w[8] : (int64_t)as_const(a.emit_rows)[nd.emit_begin() + j]);
    for (int i = 0; i < n; ++i) {
      fop<C, RowEpilogue>(cx, as_const(reinterpret_cast<const int32_t *>(a.ops + (k * a.n_ops_padded + i))),
                          slot + i, c, x, s, seq_steps, sc);
    }
  }
}

// Totally weighted sums in the fused epilogue: the row the sieves see is c[t] (x) w[t] (Reals /
// Bayesian: c * exp(-g alpha); Arctic: c - g alpha), so its increment at t is
// c[t] (x) w[t] - c[t-1] (x) w[t-1] - the second term formed here from the exclusive prefix
// (x[t] = c[t-1] bit for bit) and the weight row read one element to the left (staged in LDS;
// the element in front of the chunk from the table itself).  The result takes x's place in
// fop, whose plain difference then is the increment of the stored row, rounded like it.
template <class C>
__device__ __forceinline__ void previous_weighted(const WalkCtx &cx, int emit_mul,
                                                  const double (&x)[C::EP], double (&xs)[C::EP]) {
  constexpr int E = C::E, P = C::P;
  const IssArgs &a = *cx.a;
  const double *row = cx.rows + emit_mul * C::CHUNK;
#pragma unroll
  for (int h = 0; h < P; ++h)
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int idx = cx.wave * C::SPAN + h * C::PIECE + cx.lane * E + e;
      double w = C::SEMI != 1 ? 1.0 : 0.0;
      if (idx > 0) {
        w = row[lds_pos<C>(idx - 1)];
      } else if (cx.t0 > 0) {
        const int src = as_const(a.row_src)[emit_mul];     // (an exp table: src < 0)
        w = (a.aux + (int64_t)(-src - 1) * a.aux_tab_stride + cx.series * a.aux_n_stride)[cx.t0 - 1];
      }
      if constexpr (C::SEMI != 1) {
        xs[h * E + e] = x[h * E + e] * w;
      } else {
#pragma clang fp contract(off)
        const double neg = -1.0 * w;                        // (as mul_row forms c + (-1) * row)
        xs[h * E + e] = x[h * E + e] + neg;
      }
    }
}

template <class C>
__device__ __forceinline__ void process_node(WalkCtx &cx, const Rec &nd, int slot,
                                             const double (&pin)[C::EP],
                                             double (&pout)[C::EP], const int32_t *more = nullptr,
                                             int n_more = 0) {
  constexpr int EP = C::EP;
  cx.slot = slot;
  double s[EP];
#pragma unroll
  for (int i = 0; i < EP; ++i) s[i] = pin[i];
  OpPair pre;  // MODE 1: the first two feature ops of the first output row, requested early
  if constexpr (C::MODE == 1) {
    if (nd.emit_count() > 0) pre = load_op_pair(*cx.a, nd.w[7], 0);
  }
  const int nf = nd.fac_count();
  bool letter_sum = false;
  if constexpr (C::SEMI == 1) {
    // Arctic argmax plans: C = sum of the letter's terms, then prefix + C
    // (fruits/iss/semiring.py:252-256); 0 + term is exact, so starting from zero changes
    // nothing but the association
    letter_sum = cx.a->letter_sum != 0;
    if (letter_sum) {
#pragma unroll
      for (int i = 0; i < EP; ++i) s[i] = 0.0;
    }
  }
  if (nd.flags() & F_SLOW) {
    slow_factors<C>(cx, nd.fac_begin(), nf, s, pin, letter_sum);
  } else {
    // multiply-only letter, factors in the reference's order (ascending dimension)
    if (nf > 0) mul_row<C>(cx, nd.w[2], s);
    if (nf > 1) {
      mul_row<C>(cx, nd.w[3], s);
      if (nf > 2) mul_row<C>(cx, nd.w[4], s);
      if (nf > 3) mul_row<C>(cx, nd.w[5], s);
    }
  }
  STAMP(cx, 1);  // factors
  const bool has_children = (nd.flags() & F_CHILDREN) != 0;
  const int z_mul = nd.z_mul(), emit_mul = nd.emit_mul();
  const bool need2 = C::WEIGHTED && has_children && z_mul >= 0;
  const bool need1 = nd.emit_count() > 0 || (has_children && !need2);
#ifdef FRUITS_HIP_TIMING_BUILD
  if (cx.a->debug & 2) {  // timing experiments only: stores without the scan
    emit_all<C>(cx, nd, s);
#pragma unroll
    for (int i = 0; i < EP; ++i) pout[i] = s[i];
    return;
  }
#endif
  if (need1) {
    double c[EP], x[EP];
    block_scan<C>(cx, s, c, x, slot);
    // Reals: children start from the exclusive shift (strictly increasing indices);
    // Arctic: from the inclusive maximum (semiring.py:282-338 has no shift).  Taken
    // BEFORE the emitted values are rescaled in place below.  Written whether or not
    // the node has children (a leaf's frame is never read: its next sibling starts from
    // the frame below, and a second scan - need2 - overwrites it): a conditional
    // hand-over compiles to a select per register.
#pragma unroll
    for (int i = 0; i < EP; ++i) pout[i] = C::SEMI == 0 ? x[i] : c[i];
    if (nd.emit_count() > 0) {
      // total weighting: Reals emit c * exp(-g alpha_k), Arctic emit c - g alpha_k
      if (C::WEIGHTED && emit_mul >= 0)
        mul_row<C>(cx, C::SEMI != 1 ? emit_mul : fac_arctic(emit_mul, -1), c);
      // (MODE 1 here is the wave-per-series kernel, which a totally weighted plan under a
      // differencing sieve never takes: launch_choice.h, walk_is_packed)
      if constexpr (C::MODE == 1)
        fops_rows_ahead<C>(cx, nd, pre, c, x, s, !(C::WEIGHTED && emit_mul >= 0));
      else
        emit_all<C>(cx, nd, c, more, n_more);
      STAMP(cx, 5);  // stores
    }
  }
  if constexpr (C::WEIGHTED) {
    if (need2) {
      double s2[EP], c[EP], x[EP];
#pragma unroll
      for (int i = 0; i < EP; ++i) s2[i] = s[i];
      mul_row<C>(cx, C::SEMI != 1 ? z_mul : fac_arctic(z_mul, 1), s2);
      block_scan<C>(cx, s2, c, x, slot + 1);
#pragma unroll
      for (int i = 0; i < EP; ++i) pout[i] = C::SEMI == 0 ? x[i] : c[i];
    }
  }
}

// carry slot of a node: LDS carries are indexed by the node's position inside its
// group, global ones by its plan-wide id
template <class C>
__device__ __forceinline__ int carry_slot_of(const WalkCtx &cx, const Rec &nd, int pc) {
  if constexpr (C::MULTI == 1) return kCarrySlots * (pc - cx.pc_begin);
  return kCarrySlots * nd.node_id();
}

// Walks the records of one group.  cx.cur always holds the record at cx.pc; the
// record after it is requested BEFORE the current node is processed, so its
// scalar-memory latency hides behind the node's vector work.  The sentinel at
// the end of every group (level 0xff) terminates all loops.
template <class C, int LV>
__device__ __forceinline__ void walk(WalkCtx &cx, Rec &cur, int &pc,
                                     const double (&pin)[C::EP]) {
  const IssArgs &a = *cx.a;
  if constexpr (C::MODE == 0 && C::MAXLV <= 4) {
    // two code sites per level (head of a chain / in-place continuation): no
    // register copies; affordable for the small materialising kernels
    while (cur.level() == LV) {
      const Rec nd = cur;
      const int slot = carry_slot_of<C>(cx, nd, pc);
      ++pc;
      cur = load_rec(a.recs, pc);
      double pout[C::EP];
      STAMP(cx, 0);  // interpreter: record decode / prefetch issue
      process_node<C>(cx, nd, slot, pin, pout);
      while (cur.level() == LV && (cur.flags() & F_CHAIN)) {
        const Rec nc = cur;
        const int slot2 = carry_slot_of<C>(cx, nc, pc);
        ++pc;
        cur = load_rec(a.recs, pc);
        process_node<C>(cx, nc, slot2, pout, pout);
      }
      if constexpr (LV + 1 < C::MAXLV) {
        if (cur.level() == LV + 1) walk<C, LV + 1>(cx, cur, pc, pout);
      }
    }
  } else {
    // one code site per level (code size matters for deep / fused kernels): an only
    // child continues in place in this frame (reads its parent's prefix from pout);
    // every other node of the level reads the frame below (pin)
    double pout[C::EP];
#pragma unroll
    for (int i = 0; i < C::EP; ++i) pout[i] = 0.0;
    while (cur.level() == LV) {
      const Rec nd = cur;
      const int slot = carry_slot_of<C>(cx, nd, pc);
      ++pc;
      cur = load_rec(a.recs, pc);
      double src[C::EP];
      if (nd.flags() & F_CHAIN) {
#pragma unroll
        for (int i = 0; i < C::EP; ++i) src[i] = pout[i];
      } else {
#pragma unroll
        for (int i = 0; i < C::EP; ++i) src[i] = pin[i];
      }
      STAMP(cx, 0);  // interpreter: record decode / prefetch issue
      process_node<C>(cx, nd, slot, src, pout);
      if constexpr (LV + 1 < C::MAXLV) {
        if (cur.level() == LV + 1) walk<C, LV + 1>(cx, cur, pc, pout);
      }
    }
  }
}

// ---------------------------------------------------------------- static programs
// The same walk with the program as a COMPILE-TIME constant: PG::w holds a SCHEDULE,
// 16 words per entry like a NodeRec, of one group (the whole plan):
//   node entries     the NodeRec of the node; w[14] / w[15] = the register frame its prefix
//                    is read from (-1: the semiring's one) / written to (-1: nobody reads it);
//   kSchedStage      w[1] = staged row whose registers go to LDS now (it is first read by
//                    the next node entry);
//   kSchedEmits      w[1] further output rows (w[2..]) of the node entry in front of it (a
//                    record holds two; SINGLE-mode plans with repeated words have more);
//   kSchedPrefetch   behind the last stage entry: the registers are free again - issue the
//                    loads of the workgroup's next unit into them;
//   sentinel         end of the schedule.
// Everything the interpreter decodes per node becomes an immediate, the walk is straight-line
// code, and - what the interpreter cannot do - the rows of a unit are loaded together but
// each is completed only in front of the first node that reads it: the nodes that need row 0
// alone run while the other rows are still in flight.  The host orders the schedule for that
// (plan.cpp, static_schedule): any order in which a parent precedes its children is a valid
// walk, since frames are registers named by constants, not a stack.

template <class PG, int PC>
__device__ __forceinline__ constexpr Rec static_rec() {
  Rec r{};
  for (int i = 0; i < 16; ++i) r.w[i] = PG::w[PC * 16 + i];
  return r;
}
template <class PG>
constexpr int static_kind(int pc) { return PG::w[pc * 16] & 0xff; }
template <class PG>
constexpr int static_more_emits(int pc) {   // rows in the kSchedEmits entries starting at pc
  int n = 0;
  while (static_kind<PG>(pc) == kSchedEmits) {
    n += PG::w[pc * 16 + 1];
    ++pc;
  }
  return n;
}

template <class C>
struct StaticRegs {
  static constexpr int U = C::CHUNK / 2 / kWalkThreads;
  vd2 v[kStaticMaxRows][U];                  // rows in flight (global -> registers -> LDS)
  double fr[kStaticMaxFrames][C::EP];        // open prefixes
};

// issues the loads of the rows in MASK of series n into rg.v
template <class C, class PG, int MASK>
__device__ __forceinline__ void static_load_rows(const WalkCtx &cx, StaticRegs<C> &rg, int64_t n) {
  const IssArgs &a = *cx.a;
#pragma unroll
  for (int r = 0; r < PG::rows; ++r) {
    if (!(MASK & (1 << r))) continue;
    const double *gp = a.X + (n * a.D + PG::row_src[r]) * a.T;
#pragma unroll
    for (int k = 0; k < StaticRegs<C>::U; ++k) {
      const int i = 2 * (k * kWalkThreads + cx.tid);
      rg.v[r][k] = vd2{0.0, 0.0};
      if (cx.full_chunk || i < a.T) rg.v[r][k] = load_input<PG::groups == 1>(gp + i);
    }
  }
}

template <class C, class PG, int PC>
__device__ __forceinline__ void walk_static(WalkCtx &cx, StaticRegs<C> &rg, double *rows_w) {
  constexpr int kind = static_kind<PG>(PC);
  if constexpr (kind == kRecSentinelLevel) {
    return;
  } else if constexpr (kind == kSchedPrefetch) {
    // (single-group programs only: the next unit is the same program on another series)
    cx.have_rows = cx.next_unit < (int)cx.a->N;
    if (cx.have_rows) static_load_rows<C, PG, PG::group_rows[0]>(cx, rg, cx.next_unit);
    walk_static<C, PG, PC + 1>(cx, rg, rows_w);
  } else if constexpr (kind == kSchedStage) {
    constexpr int r = PG::w[PC * 16 + 1];
#pragma unroll
    for (int k = 0; k < StaticRegs<C>::U; ++k) {
      const int i = 2 * (k * kWalkThreads + cx.tid);
      *reinterpret_cast<vd2 *>(rows_w + r * C::CHUNK + lds_pos<C>(i)) = rg.v[r][k];
    }
    lds_barrier();
    walk_static<C, PG, PC + 1>(cx, rg, rows_w);
  } else {
    constexpr Rec nd = static_rec<PG, PC>();
    constexpr int fin = nd.w[14], fout = nd.w[15];
    // further output rows of this node: kSchedEmits entries right behind it
    constexpr int n_more = static_more_emits<PG>(PC + 1);
    constexpr int skip = (n_more + kSchedEmitsPerEntry - 1) / kSchedEmitsPerEntry;
    int32_t more[n_more > 0 ? n_more : 1];
#pragma unroll
    for (int j = 0; j < n_more; ++j)
      more[j] = PG::w[(PC + 1 + j / kSchedEmitsPerEntry) * 16 + 2 + j % kSchedEmitsPerEntry];
    double ones[C::EP], dead[C::EP];
#pragma unroll
    for (int i = 0; i < C::EP; ++i) ones[i] = C::SEMI != 1 ? 1.0 : 0.0;
    if constexpr (fin < 0 && fout < 0)
      process_node<C>(cx, nd, 0, ones, dead, more, n_more);
    else if constexpr (fin < 0)
      process_node<C>(cx, nd, 0, ones, rg.fr[fout < 0 ? 0 : fout], more, n_more);
    else if constexpr (fout < 0)
      process_node<C>(cx, nd, 0, rg.fr[fin < 0 ? 0 : fin], dead, more, n_more);
    else
      process_node<C>(cx, nd, 0, rg.fr[fin], rg.fr[fout], more, n_more);
    walk_static<C, PG, PC + 1 + skip>(cx, rg, rows_w);
  }
}

template <class C, class PG, int GI>
__device__ __forceinline__ void static_run_group(WalkCtx &cx, StaticRegs<C> &rg, double *rows_w,
                                                 int64_t n, int g) {
  if constexpr (GI < PG::groups) {
    if (g == GI) {
      if (!cx.have_rows) static_load_rows<C, PG, PG::group_rows[GI]>(cx, rg, n);
      walk_static<C, PG, PG::group_begin[GI]>(cx, rg, rows_w);
    } else {
      static_run_group<C, PG, GI + 1>(cx, rg, rows_w, n, g);
    }
  }
}

// PGT of iss_walk_static_kernel: void = no tail program
template <class PGT>
struct StaticTail {
  static constexpr bool on = true;
};
template <>
struct StaticTail<void> {
  static constexpr bool on = false;
};
template <class PG, class PGT>
constexpr bool static_same_rows() {   // both programs stage the same rows of X
  if (PG::n_src != PGT::n_src || PG::rows != PGT::rows) return false;
  for (int r = 0; r < PG::rows; ++r)
    if (PG::row_src[r] != PGT::row_src[r]) return false;
  return true;
}

// Materialising walk of a static program: one aligned time chunk (MULTI = 0, VEC), a unit is
// (series, group of the schedule), at most kStaticMaxRows staged rows, all of them rows of X.
//
// With a tail program PGT (the same plan scheduled for several groups per series) ONE launch
// holds both granularities, one unit per workgroup: workgroup b < a.n_whole runs series b with
// the one-group program PG, the workgroups behind run the last N - n_whole series as
// (series, group) units of PGT.  The finer units sit at the end of the grid: they start as the
// first round of whole-series workgroups ends and fill the partial last round in pieces of a
// third of the length (speed only - no result depends on the order of dispatch).
template <class C, class PG, class PGT = void>
__global__ __launch_bounds__(kWalkThreads) void iss_walk_static_kernel(const IssArgs a) {
  static_assert(C::MODE == 0 && C::MULTI == 0 && C::VEC && C::TEAM == 4 && !C::WEIGHTED,
                "static programs: materialising, single chunk, aligned, unweighted");
  static_assert(PG::rows <= kStaticMaxRows && PG::frames <= kStaticMaxFrames, "static program too wide");
  if constexpr (StaticTail<PGT>::on) {
    static_assert(PG::groups == 1 && PGT::groups > 1, "whole series in front, finer units behind");
    static_assert(PGT::rows <= kStaticMaxRows && PGT::frames <= kStaticMaxFrames, "static program too wide");
    static_assert(static_same_rows<PG, PGT>(), "the tail program is another schedule of the same plan");
  }
  extern __shared__ double lds[];
  const int tid = threadIdx.x;
  WalkCtx cx;
  cx.a = &a;
  cx.rows = lds;
  cx.tot = lds + PG::rows * C::CHUNK;
  cx.tail = cx.tot + 2 * C::NW;
  cx.tid = tid;
  cx.lane = tid & 63;
  cx.wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  cx.team = 0;
  cx.buf = 0;
  cx.tail_buf = 0;
  cx.carry = nullptr;
  cx.pc_begin = 0;
  cx.t0 = 0;
  cx.first_chunk = true;
  cx.full_chunk = C::CHUNK <= a.T;
  StaticRegs<C> rg;
  // The rows of a unit travel global -> registers -> LDS.  A unit loads its rows when it
  // starts (all of them at once, each completed in front of its first reader) - unless the
  // kSchedPrefetch entry of the workgroup's previous unit has already loaded them, many nodes
  // ahead of their use and in front of most of that unit's stores (vmcnt counts in order: a
  // load issued behind a store waits for it).
  cx.have_rows = false;
#ifdef FRUITS_HIP_TIMING_BUILD
  unsigned long long t_unit[4] = {0, 0, 0, 0};
  int n_unit = 0;
  const unsigned long long real_begin = __builtin_amdgcn_s_memrealtime();
#endif
  if constexpr (StaticTail<PGT>::on) {
    // one unit per workgroup; the one-group schedule's kSchedPrefetch entry sees no next unit
    const int b = blockIdx.x;
    const int n_whole = a.n_whole;
    cx.next_unit = (int)a.N;
#ifdef FRUITS_HIP_TIMING_BUILD
    t_unit[n_unit++] = __builtin_amdgcn_s_memrealtime();
#endif
    if (b < n_whole) {
      cx.out_base = a.out + (int64_t)b * a.out_n_stride;
      static_run_group<C, PG, 0>(cx, rg, lds, b, 0);
    } else {
      // (S % 8 == 0: the groups of one series meet in one XCD's L2)
      const WalkUnit w = walk_tail_unit(b - n_whole, PGT::groups, n_whole, (int)a.N - n_whole);
      if (w.n < a.N) {   // (the host launches exactly n_whole + GT * S workgroups)
        cx.out_base = a.out + w.n * a.out_n_stride;
        static_run_group<C, PGT, 0>(cx, rg, lds, w.n, w.g);
      }
    }
  } else {
    bool first_unit = true;
    constexpr int G = PG::groups;
    const int u_end = (int)(a.N * G);
    for (int u = blockIdx.x; u < u_end; u += gridDim.x) {
      int64_t n = u;
      int g = 0;
      if constexpr (G > 1) {   // (xcd_map: the groups of one series meet in one XCD's L2)
        const WalkUnit w = walk_unit(u, G, a.xcd_map != 0);
        n = w.n;
        g = w.g;
      }
      cx.out_base = a.out + n * a.out_n_stride;
      cx.next_unit = u + (int)gridDim.x;
      if (!first_unit) lds_barrier();  // all reads of the previous unit's rows are done
      first_unit = false;
#ifdef FRUITS_HIP_TIMING_BUILD
      if (n_unit < 4) t_unit[n_unit++] = __builtin_amdgcn_s_memrealtime();
#endif
      static_run_group<C, PG, 0>(cx, rg, lds, n, g);
    }
  }
#ifdef FRUITS_HIP_TIMING_BUILD
  if ((a.debug & 16) && a.dbg != nullptr && cx.lane == 0) {
    unsigned long long *o = a.dbg + ((int64_t)blockIdx.x * 4 + cx.wave) * 12;
    for (int i = 0; i < 4; ++i) o[i] = t_unit[i];
    unsigned hw_id, xcc_id;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_id));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc_id));
    o[4] = hw_id;
    o[5] = xcc_id;
    o[8] = 1;
    o[10] = real_begin;
    o[11] = __builtin_amdgcn_s_memrealtime();
  }
#endif
}

template <class C>
__global__ __launch_bounds__(kWalkThreads) void iss_walk_kernel(const IssArgs a) {
  extern __shared__ double lds[];
  const int tid = threadIdx.x;
  WalkCtx cx;
  cx.a = &a;
  cx.rows = lds;
  cx.tot = lds + (int64_t)a.R * C::CHUNK;
  cx.tail = cx.tot + 2 * C::NW;
  cx.tid = tid;
  cx.lane = tid & 63;
  {
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    cx.wave = w % C::TEAM;
    cx.team = w / C::TEAM;
  }
  cx.buf = 0;
  cx.tail_buf = 0;
  double *rows_w = lds;
  bool first_unit = true;
#ifdef FRUITS_HIP_TIMING_BUILD
  if (a.debug & 4) return;
  for (int i = 0; i < 8; ++i) cx.seg[i] = 0;
  cx.last = stamp_now();
  const unsigned long long t_begin = cx.last;
  const unsigned long long real_begin = __builtin_amdgcn_s_memrealtime();  // 100 MHz, global
#endif
  // Persistent workgroups: the grid holds (at most) one resident round of workgroups and
  // each walks units b, b + grid, ...  A unit is (series n, group g of root sub-tries).
  // Workgroups are dealt round-robin over the 8 XCDs, so with the xcd_map numbering all
  // groups of one series meet in one XCD's L2 (speed only, never correctness).  In the
  // first round the resident workgroups write CONSECUTIVE series of every output plane.
  // (Round 2 tried contiguous spans of units per workgroup - even spans, one staging shared
  // by the groups of a series: 5-10 % slower at every batch size, docs/history.md 4.6.)
  int sink = 0;  // next-series prefetch (see below): one word per 128-byte line of the rows
  int pf_val = 0, pf_off = -1;
  static_assert(C::TEAM == 4 && C::MODE == 0,
                "the materialising interpreter (fused: walk_fused.h; short series: walk_packed.h)");
  {
    const int lines = (int)((a.T * 8 + 127) >> 7);
    if (a.prefetch_next && a.nchunks == 1 && a.D * a.T < (1 << 30) && tid < a.R * lines) {
      const int r = tid / lines, line = tid - r * lines;
      const int src = a.row_src[r];
      if (src >= 0) pf_off = src * (int)a.T + line * 16;
    }
  }
  const int u_end = (int)(a.N * a.G);  // (the host checks < 2^31)
  for (int u = blockIdx.x; u < u_end; u += gridDim.x) {
    const WalkUnit unit = walk_unit(u, a.G, a.xcd_map != 0);
    const int64_t n = unit.n;
    const int g0 = unit.g;
    const int node_begin = as_const(a.group_begin)[g0];
    if constexpr (C::MULTI == 1)
      cx.carry = lds + (int64_t)a.R * C::CHUNK + 4 * C::NW;
    else
      cx.carry = a.carry ? a.carry + n * (kCarrySlots * (int64_t)a.total_nodes) : nullptr;
    cx.pc_begin = node_begin;  // LDS carry slots are indexed from the group's first record
    for (int64_t chunk = 0; chunk < a.nchunks; ++chunk) {
      const int64_t t0 = chunk * C::CHUNK;
      cx.t0 = t0;
      cx.first_chunk = chunk == 0;
      cx.full_chunk = t0 + C::CHUNK <= a.T;
      cx.out_base = a.out + n * a.out_n_stride + t0;
      if (!first_unit || chunk > 0) lds_barrier();  // all reads of the old rows are done
      // stage the referenced rows of this chunk: coalesced 16-byte units, the
      // loads of kStageRows rows in flight before the first LDS write
#ifdef FRUITS_HIP_TIMING_BUILD
      if (!(a.debug & 8))
#endif
      for (int r0 = 0; r0 < a.R; r0 += kStageRows) {
        constexpr int U = C::CHUNK / 2 / kWalkThreads;
        vd2 v[kStageRows][U];
#pragma unroll
        for (int rr = 0; rr < kStageRows; ++rr) {
          if (r0 + rr < a.R) {
            const int src = as_const(a.row_src)[r0 + rr];
            const double *gp =
                src >= 0 ? a.X + (n * a.D + src) * a.T
                         : a.aux + (int64_t)(-src - 1) * a.aux_tab_stride + n * a.aux_n_stride;
#pragma unroll
            for (int k = 0; k < U; ++k) {
              const int i = 2 * (k * kWalkThreads + tid);
              const int64_t t = t0 + i;
              v[rr][k] = vd2{0.0, 0.0};
              if (a.vec_ok) {
                if (cx.full_chunk || t < a.T) v[rr][k] = load_input<C::NT>(gp + t);
              } else {
                if (t < a.T) v[rr][k].x = gp[t];
                if (t + 1 < a.T) v[rr][k].y = gp[t + 1];
              }
            }
          }
        }
#pragma unroll
        for (int rr = 0; rr < kStageRows; ++rr) {
          if (r0 + rr < a.R) {
#pragma unroll
            for (int k = 0; k < U; ++k) {
              const int i = 2 * (k * kWalkThreads + tid);
              *reinterpret_cast<vd2 *>(rows_w + (r0 + rr) * C::CHUNK + lds_pos<C>(i)) = v[rr][k];
            }
          }
        }
      }
      __syncthreads();
      {
        if (a.prefetch_next && a.nchunks == 1) {
          // Touch one word per 128-byte line of the rows of this workgroup's NEXT unit, so
          // that its staging - issued when the memory system is full of this kernel's
          // stores - finds them in the L2 / Infinity Cache.  The loaded value is only
          // consumed behind the next staging wait (no extra stall).
          sink += pf_val;
          pf_val = 0;
          // (lines touched a whole long unit ahead are evicted before they are used:
          // units of more than prefetch_next nodes do not prefetch)
          const int n_rec = as_const(a.group_begin)[g0 + 1] - node_begin;
          const int un = u + (int)gridDim.x;
          if (un < u_end && n_rec <= a.prefetch_next && pf_off >= 0) {
            const int64_t n_next = walk_unit_series(un, a.G, a.xcd_map != 0);
            pf_val = *reinterpret_cast<const int *>(a.X + n_next * a.D * a.T + pf_off);
          }
        }
      }
      STAMP(cx, 6);  // staging
      double ones[C::EP];  // identity of the semiring's product: 1 (Reals, Bayesian), 0 (Arctic)
#pragma unroll
      for (int i = 0; i < C::EP; ++i) ones[i] = C::SEMI != 1 ? 1.0 : 0.0;
      int pc = node_begin;
      Rec cur = load_rec(a.recs, pc);
      walk<C, 0>(cx, cur, pc, ones);
    }
    first_unit = false;
  }
  if (sink + pf_val == 0x7fffffff) a.out[0] = (double)sink;  // keeps the prefetch loads alive
#ifdef FRUITS_HIP_TIMING_BUILD
  if ((a.debug & 16) && a.dbg != nullptr && cx.lane == 0) {
    unsigned long long *o = a.dbg + ((int64_t)blockIdx.x * 4 + cx.team * C::TEAM + cx.wave) * 12;
    for (int i = 0; i < 8; ++i) o[i] = cx.seg[i];
    o[8] = stamp_now() - t_begin;
    o[9] = t_begin;
    o[10] = real_begin;
    o[11] = __builtin_amdgcn_s_memrealtime();
  }
#endif
}

}  // namespace fr
