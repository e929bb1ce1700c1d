// The fused walk: INC -> ISS -> NPI / MPI / END as ONE launch (what FruitSlice.transform runs,
// fruits/fruit.py:538-550 - K x |sieves| Python calls over a materialised (K,N,T) tensor there).
//
// Same plan, records and arithmetic as the materialising walk (walk_device.h); what differs is
// the shape of the code.  These kernels write almost nothing, so they are bound by instruction
// issue, and the interpreter that serves the materialising walk well spent as many scalar as
// vector instructions per node here (and 100-500 SGPR spills).  This kernel is written for
// the fused case alone:
//   * one short-lived workgroup per (series, group) unit, no persistent loop;
//   * the first 8 dwords of a record hold everything a node of a multiply-only letter needs
//     (the rest is fetched on demand), so two records in flight cost 16 SGPRs, not 32;
//   * ONE node body for every register level (the interpreter's recursion over levels copies
//     it once per level): frames are indexed through two small uniform switches, one around
//     the first factor's multiply, one around the hand-over to the children;
//   * the cross-wave step of a scan reads a zero-padded WINDOW of the wave totals
//     (wave w reads slots w .. w+2 of {Z, Z, Z, t0, t1, t2, t3}), so the exclusive prefix of
//     the totals is two adds for every wave and no select; lane 63 publishes its wave's
//     total straight from the scan register (no readlane / broadcast);
//   * feature ops carry host-resolved flags (whole series, one-sided band), the epilogue
//     takes the short path for them;
//   * the feature ops are walk_device.h's one evaluator (fop, with WindowEpilogue below): features
//     accumulate in the LDS window (feat_flush) and leave with plain stores; a slot's column
//     follows from the walk order (GroupedProgram::slot_rows).
// Results are bit-identical to the interpreter's (same association everywhere).
//
// What a kernel of this file knows at compile time is a template parameter:
//   iss_fused_kernel<C, TOTAL>                     the generic instances (walk_inst.hip): records
//                                                  and feature ops are decoded as they are read
//   iss_fused_kernel<C, TOTAL, JitOps>             a pipeline's own kernel (jit.cpp,
//                                                  fr_pipeline_prepare): the sieves as immediates
//   iss_fused_kernel<C, TOTAL, JitOps, JitPlan>    ... and the plan (fr_pipeline_compile_plan): a
//                                                  small one as straight-line code (fwalk_static),
//                                                  a large one in pieces (fwalk_pieces), or of a
//                                                  large one the node shapes (fwalk_shaped)
// and C::MODE == 2 is the same node loop with a store epilogue: the lean MATERIALISING walk of the
// plans that have no static program of walk_device.h's kind (emit_lean, two pieces per wave).
//
// All of them evaluate a node in ONE function, fnode_body, over a node DESCRIPTOR that says which
// fields of the record the kernel knows: RecNode (none: the record is loaded and decoded),
// ShapeNode (level, flags, output-row count), StaticNode (all of it).  The four drivers differ in
// how they step: fwalk (record loop), fwalk_shaped (shape-indexed loop), fwalk_static (template
// recursion over the records), fwalk_pieces (the items of a piece type: a chain by the record
// loop, a body by the recursion).
#pragma once
#include "walk_device.h"

namespace fr {

// Table reads of the node loop: base pointer + unsigned 32-bit BYTE offset (one scalar load with
// a register offset; a 64-bit index costs five scalar instructions of address arithmetic).
__device__ __forceinline__ cptr<int32_t> at_offset(const void *base, uint32_t off) {
  return (cptr<int32_t>)((cptr<char>)(base) + off);
}

__device__ __forceinline__ const void *uniform_ptr(const void *p) {
  const uint64_t u = reinterpret_cast<uint64_t>(p);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)u);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(u >> 32));
  return reinterpret_cast<const void *>(((uint64_t)hi << 32) | lo);
}

// One dword of a table line, loaded a node ahead of the real access: the line is then in the
// scalar cache and the real load (issued right where its registers are needed - prefetching INTO
// registers keeps 16 SGPRs alive across the node and ends in spills) is a cache hit.
__device__ __forceinline__ int touch(const void *base, uint32_t off) {
  return at_offset(base, off)[0];
}

// the first half of a NodeRec (w[0..7]): level | flags, factor count | weights, four inline
// factors, emit count, first output row
struct Rec8 {
  int32_t w[8];
  __device__ __forceinline__ int level() const { return w[0] & 0xff; }
  __device__ __forceinline__ int flags() const { return w[0] >> 8; }
  __device__ __forceinline__ int fac_count() const { return w[1] & 0xffff; }
  __device__ __forceinline__ int emit_count() const { return w[6]; }
};

__device__ __forceinline__ Rec8 load_rec8(const NodeRec *recs, uint32_t rec_off) {
  cptr<int32_t> q = at_offset(recs, rec_off);
  Rec8 r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.w[i] = q[i];
  return r;
}

// a field of the second half of a record (second output row, factor / emit table offsets)
__device__ __forceinline__ int rec_field(const NodeRec *recs, uint32_t rec_off, int i) {
  return at_offset(recs, rec_off)[i];
}

// s = src (x) factor: the first factor of a letter reads the prefix it continues
template <class C>
__device__ __forceinline__ void mul_row_from(const WalkCtx &cx, int code, const double (&src)[C::EP],
                                             double (&s)[C::EP]) {
  double v[C::EP];
  // (multiply-only codes of Reals / Bayesian records are bare row numbers: nothing to mask)
  read_row<C>(cx, C::SEMI != 1 ? code : (code & FAC_ROW_MASK), v);
  if constexpr (C::SEMI != 1) {
#pragma unroll
    for (int i = 0; i < C::EP; ++i) s[i] = src[i] * v[i];
  } else {
#pragma clang fp contract(off)  // the product must round before the add (no FMA)
    const double el = (double)(int)(int8_t)((code >> 8) & 0xff);
#pragma unroll
    for (int i = 0; i < C::EP; ++i) {
      const double prod = el * v[i];
      s[i] = src[i] + prod;
    }
  }
}

// s (x)= factor for the codes the fused walk meets outside the factor table: bare row numbers
// (Reals / Bayesian), row | multiplier << 8 (Arctic)
template <class C>
__device__ __forceinline__ void mul_rowp(const WalkCtx &cx, int code, double (&s)[C::EP]) {
  if constexpr (C::SEMI == 1) {
    mul_row<C>(cx, code, s);
  } else {
    double v[C::EP];
    read_row<C>(cx, code, v);
#pragma unroll
    for (int i = 0; i < C::EP; ++i) s[i] = s[i] * v[i];
  }
}

// The same scan for P pieces per wave (the materialising walk, MODE 2: lane l holds E = 2
// consecutive elements of each of its wave's two pieces, so that every 16-byte store instruction
// of a wave covers 1 KiB without holes): one DPP chain per piece, interleaved; the sums and their
// order are block_scan's.
template <class C>
__device__ __forceinline__ void fscan_pieces(WalkCtx &cx, const double (&s)[C::EP], double (&c)[C::EP],
                                             double (&x)[C::EP], int carry_slot) {
  constexpr int E = C::E, P = C::P;
  double l[C::EP], incl[P], excl[P];
#pragma unroll
  for (int h = 0; h < P; ++h) {
    l[h * E] = s[h * E];
#pragma unroll
    for (int e = 1; e < E; ++e) l[h * E + e] = semi_add<C::SEMI>(l[h * E + e - 1], s[h * E + e]);
    incl[h] = l[h * E + E - 1];
  }
  wave_inclusive_scan_multi<P, C::SEMI>(incl);
#pragma unroll
  for (int h = 0; h < P; ++h) excl[h] = wave_shift_right1<C::SEMI>(incl[h]);
  // lane 63: the totals of the pieces in order = the wave's total
  double total = incl[0];
#pragma unroll
  for (int h = 1; h < P; ++h) total = semi_add<C::SEMI>(total, incl[h]);
  double carry_in = semi_zero<C::SEMI>();
  if constexpr (C::MULTI != 0) {
    if (!cx.first_chunk) carry_in = cx.carry[carry_slot];
  }
  lds_f64 *tw = (lds_f64 *)(cx.tot + cx.buf * 8);   // {Z, Z, Z, t0, t1, t2, t3, -}
  lds_store_lane63(lds_offset(tw + 3 + cx.wave), total);
  lds_barrier();
  const double a0 = tw[cx.wave], a1 = tw[cx.wave + 1], a2 = tw[cx.wave + 2];
  double base = semi_add<C::SEMI>(semi_add<C::SEMI>(a0, a1), a2);
  cx.buf ^= 1;
  if constexpr (C::MULTI != 0) {
    if (cx.wave == 3)
      lds_store_lane63(lds_offset((lds_f64 *)cx.carry + carry_slot),
                       semi_add<C::SEMI>(carry_in, semi_add<C::SEMI>(base, total)));
    base = semi_add<C::SEMI>(base, carry_in);
  }
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
    if (h + 1 < P) base = semi_add<C::SEMI>(base, wave_last_lane(incl[h]));
  }
}

// Inclusive scan of one chunk row over the workgroup (P = 1: lane l holds E consecutive
// elements, wave w the span [w * 64 E, (w + 1) * 64 E)).  Same sums in the same order as
// block_scan; the cross-wave step reads the totals window (see the file comment).
// WINDOW = false: the identity slots hold another semiring's zero (the plain sums of a max-plus
// plan's cumulated rows, inc < 0) - select instead.
// `carry_wr`: the slot the advanced chunk carry goes to (default: the one it was read from; the
// cumulations of the epilogue keep two buffers, see WindowEpilogue).
template <class C, bool WINDOW = true>
__device__ __forceinline__ void fscan(WalkCtx &cx, const double (&s)[C::EP], double (&c)[C::EP],
                                      double (&x)[C::EP], int carry_slot, int carry_wr = -1) {
  static_assert(C::NW == 4, "four waves");
  if constexpr (C::P != 1) {
    fscan_pieces<C>(cx, s, c, x, carry_slot);
    return;
  }
  constexpr int E = C::E;
  double l[E];
  l[0] = s[0];
#pragma unroll
  for (int e = 1; e < E; ++e) l[e] = semi_add<C::SEMI>(l[e - 1], s[e]);
  const double incl = wave_inclusive_scan<C::SEMI>(l[E - 1]);
  const double excl = wave_shift_right1<C::SEMI>(incl);
  double carry_in = semi_zero<C::SEMI>();
  if constexpr (C::MULTI != 0) {
    if (!cx.first_chunk) carry_in = cx.carry[carry_slot];
  }
  lds_f64 *tw = (lds_f64 *)(cx.tot + cx.buf * 8);   // {Z, Z, Z, t0, t1, t2, t3, -}
  lds_store_lane63(lds_offset(tw + 3 + cx.wave), incl);
  lds_barrier();
  double base;
  if constexpr (WINDOW) {
    const double a0 = tw[cx.wave], a1 = tw[cx.wave + 1], a2 = tw[cx.wave + 2];
    base = semi_add<C::SEMI>(semi_add<C::SEMI>(a0, a1), a2);
  } else {
    const double t0 = tw[3], t1 = tw[4], t2 = tw[5];
    const double p2 = semi_add<C::SEMI>(t0, t1), p3 = semi_add<C::SEMI>(p2, t2);
    base = cx.wave == 0 ? semi_zero<C::SEMI>() : (cx.wave == 1 ? t0 : (cx.wave == 2 ? p2 : p3));
  }
  cx.buf ^= 1;
  if constexpr (C::MULTI != 0) {
    // the carry of earlier chunks: every wave read it before the barrier, the last lane of the
    // chunk advances it
    if (cx.wave == 3)
      lds_store_lane63(lds_offset((lds_f64 *)cx.carry + (carry_wr < 0 ? carry_slot : carry_wr)),
                       semi_add<C::SEMI>(carry_in, semi_add<C::SEMI>(base, incl)));
    base = semi_add<C::SEMI>(base, carry_in);
  }
  const double off = semi_add<C::SEMI>(base, excl);
  x[0] = off;
#pragma unroll
  for (int e = 0; e + 1 < E; ++e) {
    c[e] = semi_add<C::SEMI>(off, l[e]);
    x[e + 1] = c[e];
  }
  c[E - 1] = semi_add<C::SEMI>(base, incl);
}

// The epilogue policy of the fused walk (EPI of fop, walk_device.h): a cumulation is an fscan; on
// series of several chunks (WalkCfg::HIGHORD) the j-th cumulation of an op carries its running sum
// in a slot pair of its own behind the differencing orders' (kCumCarryBase + 2 j): this chunk reads
// buffer `parity` and writes the other, so several sieves of a node read the same old value.  The
// CPV exchange carries in the node's LAST slot (IssArgs::carry_per_node - 1).  The shapes the host
// flags take their short paths here.
struct WindowEpilogue {
  template <class CR>
  static __device__ __forceinline__ void cumulate(WalkCtx &cx, int j, const double (&d)[CR::EP],
                                                  double (&cs)[CR::EP]) {
    double xs[CR::EP];
    const int at = cx.slot + kCumCarryBase + 2 * j;
    fscan<CR, false>(cx, d, cs, xs, at + cx.parity, at + (cx.parity ^ 1));
  }
  static constexpr bool short_paths = true;
  static __device__ __forceinline__ int cpv_slot() { return cold_args()->carry_per_node - 1; }
};

// one feature op (32 bytes = one s_load_dwordx8)
struct Op1 {
  int32_t w[8];
};
// what the node loop reads of the kernel arguments, as scalars of their own
struct Hot {
  const NodeRec *recs;
  const FeatOp *ops;
  int n_ops;
  uint32_t op_row_bytes;   // bytes of one output row's ops (the host checks the table < 4 GiB)
  int cps;                 // carry slots per node (kCarrySlots; more with differencing orders >= 3)
  // a body of a plan in pieces (fwalk_pieces): its output rows and carry slots count from these
  // (0 everywhere else)
  uint32_t op_base;        // byte offset of the body's first output row in the op table
  int slot_base;           // carry slot of the body's first node
  // MODE 2 (the tensor is written): row 0 of this series' chunk, bytes between two output rows
  // (0: beyond 32 bits - the general product), whole aligned chunk (no per-lane checks)
  char *out;
  uint32_t k_stride;
  bool fast_store;
};
__device__ __forceinline__ Op1 load_op1(const Hot &a, uint32_t op_off) {
  cptr<int32_t> q = at_offset(a.ops, op_off);
  Op1 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o.w[j] = q[j];
  return o;
}

// What a kernel knows of the sieves at compile time.  DynOps: nothing - every op is decoded from
// its 32-byte record (kind, differencing order, shape, cuts).  A run-time compiled kernel (jit.cpp,
// fr_pipeline_prepare) is instantiated over a struct like
//   struct JitOps { static constexpr bool is_static = true; static constexpr int n = 2;
//                   static constexpr int32_t w0[n] = {...}, lo[n] = {...}, hi[n] = {...}; };
// - the ops of EVERY output row of a pipeline are the same sieves, only the thresholds and the
// column differ - so kind_inc / lo / hi are immediates: the op loop is unrolled and the decode of
// fop folds away (an END at a fixed index of a one-chunk series becomes one predicated LDS store).
struct DynOps {
  static constexpr bool is_static = false, window_fits = false, full_chunks = false;
  static constexpr int n = 0;
};

// Window slots of the next node.  OPS::window_fits (a kernel of a piece type whose largest unit
// fits the feature window: the host knows when it compiles the kernel): no test, and no copy of
// the flush behind every node of straight-line code.
template <class C, class OPS>
__device__ __forceinline__ void freserve(WalkCtx &cx, int need) {
  if constexpr (OPS::window_fits) {
    cx.fslot = cx.fused_used;
    cx.fused_used += need;
  } else {
    feat_reserve<C>(cx, need);
  }
}

// The j-th output row of a node, j >= 1 (the first is w[7] of its record): the second is inline in
// the record, further ones - SINGLE-mode plans with repeated words - come from the emit-row table.
__device__ __forceinline__ int emit_row(const Hot &a, uint32_t rec_off, int j) {
  return j == 1 ? rec_field(a.recs, rec_off, 8)
                : as_const(cold_args()->emit_rows)[rec_field(a.recs, rec_off, 13) + j];
}

template <class C, class OPS, bool SEQ, int I>
__device__ __forceinline__ void fops_static(WalkCtx &cx, const Hot &a, uint32_t op_off, int slot,
                                            const double (&c)[C::EP], const double (&x)[C::EP],
                                            const double (&s)[C::EP], FusedScratch<C::EP> &sc) {
  if constexpr (I < OPS::n) {
    const Op1 o = load_op1(a, op_off + 32u * (uint32_t)I);   // (column and thresholds: the row's own)
    const int32_t w[8] = {OPS::w0[I], o.w[1], OPS::lo[I], OPS::hi[I], o.w[4], o.w[5], o.w[6], o.w[7]};
    fop<C, WindowEpilogue, const int32_t *>(cx, w, slot + I, c, x, s, SEQ, sc);
    fops_static<C, OPS, SEQ, I + 1>(cx, a, op_off, slot, c, x, s, sc);
  }
}

// The feature ops of every output row of a node: ONE code site for an op; an op is loaded where
// it is evaluated (its line was touched at the start of the node: a scalar-cache hit).
template <class C, bool SEQ, class OPS>
__device__ __forceinline__ void fops_all(WalkCtx &cx, const Hot &a, int ne, uint32_t op_off,
                                         uint32_t rec_off, const double (&c)[C::EP],
                                         const double (&x)[C::EP], const double (&s)[C::EP]) {
  const int n = OPS::is_static ? OPS::n : a.n_ops;
  FusedScratch<C::EP> sc;
  int slot = cx.fslot;   // window slot of (output row j, op i): fslot + j * n + i
  for (int j = 0;;) {
    if constexpr (OPS::is_static) {
      fops_static<C, OPS, SEQ, 0>(cx, a, op_off, slot, c, x, s, sc);
    } else {
      for (int i = 0; i < n; ++i) {
        const Op1 o = load_op1(a, op_off + 32u * (uint32_t)i);
        fop<C, WindowEpilogue, const int32_t *>(cx, o.w, slot + i, c, x, s, SEQ, sc);
      }
    }
    if (++j >= ne) break;
    slot += n;
    op_off = a.op_base + (uint32_t)emit_row(a, rec_off, j) * a.op_row_bytes;
  }
}

// MODE 2: the node's values into every output row it names (two inline in the record, further
// ones - SINGLE-mode plans with repeated words - from the table).  A lane holds E consecutive
// elements: 16-byte stores, base = the row's uniform address, offset = one 32-bit register.
template <class C>
__device__ __forceinline__ void emit_lean(const WalkCtx &cx, const Hot &a, int ne, int k,
                                          uint32_t rec_off, const double (&c)[C::EP]) {
  constexpr int E = C::E, P = C::P;
  const uint32_t lane_bytes = (uint32_t)(cx.wave * C::SPAN + cx.lane * E) * 8u;
  for (int j = 0;;) {
    char *row = a.k_stride != 0
                    ? a.out + (uint64_t)(uint32_t)k * (uint64_t)a.k_stride
                    : a.out + (int64_t)k * cold_args()->out_k_stride * 8;
    if (a.fast_store) {
#pragma unroll
      for (int h = 0; h < P; ++h)
#pragma unroll
        for (int e = 0; e < E; e += 2)
          *reinterpret_cast<vd2 *>(row + lane_bytes + 8u * (h * C::PIECE + e)) = vd2{c[h * E + e], c[h * E + e + 1]};
    } else {
      const int64_t T = cold_args()->T;
#pragma unroll
      for (int h = 0; h < P; ++h)
#pragma unroll
        for (int e = 0; e < E; ++e) {
          const uint32_t at = lane_bytes + 8u * (h * C::PIECE + e);
          if (cx.t0 + (at >> 3) < T) *reinterpret_cast<double *>(row + at) = c[h * E + e];
        }
    }
    if (++j >= ne) break;
    k = emit_row(a, rec_off, j);
  }
}

// Register frames: f[k] holds the prefix the children of the open node of level k continue
// from.  They are only ever indexed by compile-time constants (the *_at functions; K < 0 is the
// semiring's one: a first letter).
template <class C>
__device__ __forceinline__ void semiring_one(double (&s)[C::EP]) {
#pragma unroll   // (identity of the semiring's product: 1 (Reals, Bayesian), 0 (Arctic))
  for (int i = 0; i < C::EP; ++i) s[i] = C::SEMI != 1 ? 1.0 : 0.0;
}
template <class C, int K>
__device__ __forceinline__ void frame_get_at(const double (&f)[C::MAXLV][C::EP], double (&s)[C::EP]) {
  if constexpr (K < 0) {
    semiring_one<C>(s);
  } else {
#pragma unroll
    for (int i = 0; i < C::EP; ++i) s[i] = f[K][i];
  }
}
template <class C, int K>
__device__ __forceinline__ void frame_mul_at(const WalkCtx &cx, int code, const double (&f)[C::MAXLV][C::EP],
                                             double (&s)[C::EP]) {
  if constexpr (K < 0) {
    double ones[C::EP];
    semiring_one<C>(ones);
    mul_row_from<C>(cx, code, ones, s);
  } else {
    mul_row_from<C>(cx, code, f[K], s);
  }
}
template <class C, int K>
__device__ __forceinline__ void frame_put_at(double (&f)[C::MAXLV][C::EP], const double (&x)[C::EP]) {
#pragma unroll
  for (int i = 0; i < C::EP; ++i) f[K][i] = x[i];
}
// A node's level as a run-time value selects a case through a chain of single-bit tests of
// 1 << level, deepest level first (that is where most nodes are; as a chain of equality tests the
// compiler builds a balanced switch with flag variables out of it).
template <class C, int K>
__device__ __forceinline__ void frame_mul(const WalkCtx &cx, unsigned rd_bit, int code,
                                          const double (&f)[C::MAXLV][C::EP], double (&s)[C::EP]) {
  if constexpr (K < 0) {
    frame_mul_at<C, -1>(cx, code, f, s);
  } else {
    if (rd_bit & (2u << K)) {
      frame_mul_at<C, K>(cx, code, f, s);
      asm volatile("" ::: "memory");  // (keeps the cases apart: merged, they cost selects)
    } else {
      frame_mul<C, K - 1>(cx, rd_bit, code, f, s);
    }
  }
}
template <class C, int K>
__device__ __forceinline__ void frame_get(unsigned rd_bit, const double (&f)[C::MAXLV][C::EP],
                                          double (&s)[C::EP]) {
  if constexpr (K < 0) {
    frame_get_at<C, -1>(f, s);
  } else {
    if (rd_bit & (2u << K)) {
      frame_get_at<C, K>(f, s);
      asm volatile("" ::: "memory");
    } else {
      frame_get<C, K - 1>(rd_bit, f, s);
    }
  }
}
template <class C, int K>
__device__ __forceinline__ void frame_put(unsigned lv_bit, double (&f)[C::MAXLV][C::EP],
                                          const double (&x)[C::EP]) {
  if constexpr (K >= 0) {
    if (lv_bit & (1u << K)) {
      frame_put_at<C, K>(f, x);
      asm volatile("" ::: "memory");
    } else {
      frame_put<C, K - 1>(lv_bit, f, x);
    }
  }
}

// ---------------------------------------------------------------- node descriptors
// What the node body (fnode_body below) is told about a node: for every field of the record, its
// value and whether the kernel knows it at compile time.  `knows_flags`: level and flags are the
// constants klevel / kflags - the frames are indexed directly, a test of a flag folds away;
// `knows_record`: so is everything else (knf: the factor count; the other fields are constants
// behind the same accessors).  Where a field comes from the record the body branches on it
// (uniform branches) and reaches the frames through the bit tests above.
//
// RecNode: a loaded record, nothing known - the generic instances, a pipeline's kernel with the
// sieves as immediates, the lean materialising walk (MODE 2), the chain in front of a piece.  Only
// here is there anything to prefetch: the lines of the next record and of the node's ops go to
// the scalar cache at the start of the node, and `r` leaves the body as the NEXT record (requested
// behind the first scan: a scalar-cache hit, in flight over the second).
struct RecNode {
  static constexpr bool knows_flags = false, knows_record = false;
  static constexpr int klevel = 0, kflags = 0, knf = 0;
  Rec8 &r;
  const uint32_t me;   // byte offset of the record
  __device__ __forceinline__ int level() const { return r.level(); }
  __device__ __forceinline__ int flags() const { return r.flags(); }
  __device__ __forceinline__ int fac_count() const { return r.fac_count(); }
  __device__ __forceinline__ int fac(int i) const { return r.w[2 + i]; }
  __device__ __forceinline__ int weights() const { return r.w[1]; }   // z_mul, emit_mul (Rec8)
  __device__ __forceinline__ int emit_count() const { return r.emit_count(); }
  __device__ __forceinline__ int first_row() const { return r.w[7]; }
  __device__ __forceinline__ int fac_begin(const Hot &a) const { return rec_field(a.recs, me, 12); }
  __device__ __forceinline__ int touch_next(const Hot &a) const { return touch(a.recs, me + 64u); }
  // (a node without output rows names row 0: a harmless touch)
  __device__ __forceinline__ int touch_ops(const Hot &a, uint32_t op_off) const { return touch(a.ops, op_off); }
  __device__ __forceinline__ void advance(const Hot &a, int touched, int &sink) const {
    sink += touched;
    r = load_rec8(a.recs, me + 64u);
  }
};

// ShapeNode: a run-time compiled kernel of a LARGE plan that is not cut into pieces knows the
// plan's node SHAPES - level, flags, output rows (GroupedProgram::shapes, the most frequent
// first); the rows, weights and offsets still come from the record.
template <class SH, int I>
struct SShape {
  static constexpr int d = SH::desc[I];
  static constexpr int level = d & 0xff, flags = (d >> 8) & 0xff;
  static constexpr int ne = (d >> 20) & 0xf;   // output rows; 3: more than two (read from the record)
};
template <class SH, int I>
struct ShapeNode : RecNode {
  using S = SShape<SH, I>;
  static constexpr bool knows_flags = true;
  static constexpr int klevel = S::level, kflags = S::flags;
  __device__ __forceinline__ ShapeNode(Rec8 &r, uint32_t me) : RecNode{r, me} {}
  __device__ __forceinline__ int emit_count() const { return S::ne < 3 ? S::ne : r.emit_count(); }
};

// StaticNode: a run-time compiled kernel may also know the PLAN (jit.cpp: a pipeline of at most
// kFusedStaticMaxNodes nodes, or one piece type of a larger one): PG::w holds the records, 16
// words per record like NodeRec.  Record PC is then a constant in every field: nothing is loaded,
// touched or decoded.
struct NoProg {
  static constexpr bool is_static = false, is_shaped = false, is_piece = false;
};
template <class PG, int PC>
struct StaticNode {
  static constexpr int w(int i) { return PG::w[PC * 16 + i]; }
  static constexpr bool knows_flags = true, knows_record = true;
  static constexpr int klevel = PG::w[PC * 16] & 0xff, kflags = PG::w[PC * 16] >> 8;
  static constexpr int knf = PG::w[PC * 16 + 1] & 0xffff;
  static constexpr uint32_t me = (uint32_t)PC * 64u;
  static constexpr int level() { return klevel; }
  static constexpr int flags() { return kflags; }
  static constexpr int fac_count() { return knf; }
  static constexpr int fac(int i) { return w(2 + i); }
  static constexpr int weights() { return w(1); }
  static constexpr int emit_count() { return w(6); }
  static constexpr int first_row() { return w(7); }
  static constexpr int fac_begin(const Hot &) { return w(12); }
  static constexpr int touch_next(const Hot &) { return 0; }
  static constexpr int touch_ops(const Hot &, uint32_t) { return 0; }
  static __device__ __forceinline__ void advance(const Hot &, int, int &) {}
};

// the children's prefix into the node's own frame
template <class C, class ND>
__device__ __forceinline__ void hand_over(unsigned lv_bit, double (&f)[C::MAXLV][C::EP],
                                          const double (&p)[C::EP]) {
  if constexpr (ND::knows_flags) frame_put_at<C, ND::klevel>(f, p);
  else frame_put<C, C::MAXLV - 1>(lv_bit, f, p);
}

// One node: the letters into the prefix it continues (the frame of the level below; its own
// level's for an only child, F_CHAIN; the semiring's one at level 0), the scan, the hand-over to
// the children, the feature ops (MODE 2: the stores) and, under a non-total weighting, the second
// scan.  The ONE place where the walk's node semantics are written: what a kernel knows of the node
// is the descriptor's (above), how it steps to the next the driver's (below).
//
// The tests of the node's fields are plain `if`s.  On a RecNode they are the uniform branches of
// the record loop.  On a field the descriptor knows, the condition is an integral constant
// expression and the compiler's front end emits no code for the arm not taken (nor does the
// body call anything that is instantiated per node), so a straight-line kernel pays nothing for
// the arms its nodes do not take: resources, code size and compile time of the bundled kernels
// against the earlier `if constexpr` bodies are in DESIGN.md 4.2.  Only the frames need
// `if constexpr`: their index is a template argument.
template <class C, bool TOTAL, class OPS, class ND>
__device__ __forceinline__ void fnode_body(WalkCtx &cx, const Hot &a, double (&f)[C::MAXLV][C::EP],
                                           ND &nd, int slot, int &sink) {
  constexpr int EP = C::EP;
  constexpr bool KF = ND::knows_flags;
  constexpr int kread = (ND::kflags & F_CHAIN) ? ND::klevel : ND::klevel - 1;   // the level read
  static_assert(C::MODE == 1 || !KF, "the lean materialising walk (MODE 2) decodes its records");
  static_assert(!KF || ND::klevel < C::MAXLV, "a node deeper than the kernel's register frames");
  const uint32_t me = nd.me;
  // (known fields by their static names: integral constants to the compiler's front end)
  const int flags = KF ? ND::kflags : nd.flags(), nf = ND::knows_record ? ND::knf : nd.fac_count();
  const int ne = nd.emit_count(), w1 = nd.weights();
  const uint32_t op_off = a.op_base + (uint32_t)nd.first_row() * a.op_row_bytes;
  const int t_rec = nd.touch_next(a);
  int t_ops = 0;
  if constexpr (C::MODE == 1) {
    // the op line and the window slots of the node's output rows.  The record loop does not look
    // whether the node has any: it reserves none then.  A node KNOWN to have none skips both (the
    // earlier straight-line body reserved 0 slots there, which only set cx.fslot - nobody reads it)
    if (!KF || (flags & F_EMIT)) {
      t_ops = nd.touch_ops(a, op_off);
      freserve<C, OPS>(cx, ne * a.n_ops);
    }
  }
  cx.slot = slot;
  const unsigned lv_bit = 1u << (KF ? ND::klevel : nd.level());
  const unsigned rd_bit = (flags & F_CHAIN) ? (lv_bit << 1) : lv_bit;   // 2 << (level read)
  double s[EP];
  if (flags & F_SLOW) {
    // a reciprocal factor, more than four or none: the factor table, one factor at a time
    if constexpr (KF) frame_get_at<C, kread>(f, s);
    else frame_get<C, C::MAXLV - 1>(rd_bit, f, s);
    slow_factors<C>(cx, nd.fac_begin(a), nf, s, s, false);
  } else {
    if constexpr (KF) frame_mul_at<C, kread>(cx, nd.fac(0), f, s);
    else frame_mul<C, C::MAXLV - 1>(cx, rd_bit, nd.fac(0), f, s);
    if (nf > 1) {
      mul_rowp<C>(cx, nd.fac(1), s);
      if (nf > 2) mul_rowp<C>(cx, nd.fac(2), s);
      if (nf > 3) mul_rowp<C>(cx, nd.fac(3), s);
    }
  }
  if (flags & F_NEED1) {
    double c[EP], x[EP];
    fscan<C>(cx, s, c, x, slot);
    // Reals: children start from the exclusive shift; Arctic / Bayesian: from the inclusive
    // maximum (taken before the emitted values are rescaled)
    if ((flags & (F_CHILDREN | F_NEED2)) == F_CHILDREN) hand_over<C, ND>(lv_bit, f, C::SEMI == 0 ? x : c);
    if (flags & F_EMIT) {
      constexpr bool RESCALED = C::WEIGHTED && TOTAL;
      [[maybe_unused]] const int emit_mul = ((w1 >> 24) & 0xff) - 1;
      // total weighting: the sieves see c * exp(-g alpha_k) (Arctic: c - g alpha_k)
      if constexpr (RESCALED) mul_rowp<C>(cx, C::SEMI != 1 ? emit_mul : fac_arctic(emit_mul, -1), c);
      if constexpr (C::MODE == 2) {
        emit_lean<C>(cx, a, ne, nd.first_row(), me, c);
      } else if constexpr (RESCALED && C::TOTALINC) {
        double xs[EP];
        previous_weighted<C>(cx, emit_mul, x, xs);
        fops_all<C, false, OPS>(cx, a, ne, op_off, me, c, xs, s);
      } else {
        fops_all<C, !RESCALED, OPS>(cx, a, ne, op_off, me, c, x, s);
      }
    }
  }
  nd.advance(a, t_rec + t_ops, sink);
  if constexpr (C::WEIGHTED && !TOTAL) {
    if (flags & F_NEED2) {
      // non-total weighting: the children continue from the scan of s * exp(+g alpha_k)
      const int z_mul = ((w1 >> 16) & 0xff) - 1;
      double c2[EP], x2[EP];
      mul_rowp<C>(cx, C::SEMI != 1 ? z_mul : fac_arctic(z_mul, 1), s);
      fscan<C>(cx, s, c2, x2, slot + 1);
      hand_over<C, ND>(lv_bit, f, C::SEMI == 0 ? x2 : c2);
    }
  }
}

// ---------------------------------------------------------------- the drivers
// Every driver begins with the same two lines: the node loop's arguments as scalars (hot_args) and
// the register frames, zeroed.  The zeroing is a macro and not a function on purpose: the scalar
// stores have to stand in the driver's own body.  A helper that zeroes the array (or `= {}`) is
// one store of the whole array by the time it is inlined, and the frames then live as ONE vector
// of MAXLV x EP doubles (48 more VGPRs in the lean kernels of six levels); frames declared once in
// the kernel and handed to the drivers cost the piece kernels 14 VGPRs, an occupancy step.
#define FR_ZEROED_FRAMES(f)                 \
  double f[C::MAXLV][C::EP];                \
  _Pragma("unroll") for (int k = 0; k < C::MAXLV; ++k) \
  _Pragma("unroll") for (int i = 0; i < C::EP; ++i) f[k][i] = 0.0

// What the node loop reads of the kernel arguments (see Hot).  A run-time compiled kernel knows the
// number of its ops and of a node's carry slots.
template <class C, class OPS>
__device__ __forceinline__ Hot hot_args(const WalkCtx &cx) {
  Hot a;
  const IssArgs &ka = *cx.a;
  // (through readfirstlane: scalars of their own, not pieces of one wide kernel-argument load
  // that is spilled and restored as a whole)
  a.recs = reinterpret_cast<const NodeRec *>(uniform_ptr(ka.recs));
  a.ops = reinterpret_cast<const FeatOp *>(uniform_ptr(ka.ops));
  if constexpr (OPS::is_static) {
    a.n_ops = OPS::n;
    a.op_row_bytes = (uint32_t)(OPS::n_padded * 32);
    a.cps = C::MULTI != 0 ? OPS::cps : kCarrySlots;
  } else {
    a.n_ops = __builtin_amdgcn_readfirstlane(ka.n_ops);
    a.op_row_bytes = __builtin_amdgcn_readfirstlane(ka.n_ops_padded * 32);
    a.cps = C::MULTI != 0 ? __builtin_amdgcn_readfirstlane(ka.carry_per_node) : kCarrySlots;
  }
  a.op_base = 0;
  a.slot_base = 0;
  if constexpr (C::MODE == 2) {
    a.out = static_cast<char *>(const_cast<void *>(uniform_ptr(cx.out_base)));
    a.k_stride = __builtin_amdgcn_readfirstlane(ka.k_stride_bytes32);
    a.fast_store = cx.full_chunk && ka.vec_ok != 0;
  }
  return a;
}

// The record loop: the records from rec_off on (DFS order) up to the sentinel; `slot`: the carry
// slots of the node, a.cps per record.
template <class C, bool TOTAL, class OPS>
__device__ __forceinline__ void fwalk_records(WalkCtx &cx, const Hot &a, double (&f)[C::MAXLV][C::EP],
                                              uint32_t &rec_off, int &slot, int &sink) {
  Rec8 r = load_rec8(a.recs, rec_off);
  while (r.level() != kRecSentinelLevel) {
    RecNode nd{r, rec_off};
    fnode_body<C, TOTAL, OPS>(cx, a, f, nd, slot, sink);
    rec_off += 64u;
    slot += a.cps;
  }
}
// the records of one group
template <class C, bool TOTAL, class OPS>
__device__ __forceinline__ void fwalk(WalkCtx &cx, int node_begin, int &sink) {
  const Hot a = hot_args<C, OPS>(cx);
  FR_ZEROED_FRAMES(f);
  uint32_t rec_off = (uint32_t)node_begin * 64u;
  int slot = 0;
  fwalk_records<C, TOTAL, OPS>(cx, a, f, rec_off, slot, sink);
}

// The shape-indexed loop: still a loop over records, but a node's shape index (one more dword per
// node, IssArgs::shape_ids) selects a body compiled for that shape through a chain of uniform
// tests, the most frequent shape first.  Shapes beyond the SH::n compiled ones take the record's.
template <class C, bool TOTAL, class OPS, class SH, int I>
__device__ __forceinline__ void fnode_by_shape(int shape, WalkCtx &cx, const Hot &a,
                                               double (&f)[C::MAXLV][C::EP], Rec8 &r, uint32_t me,
                                               int slot, int &sink) {
  if constexpr (I < SH::n) {
    if (shape == I) {
      ShapeNode<SH, I> nd(r, me);
      fnode_body<C, TOTAL, OPS>(cx, a, f, nd, slot, sink);
      asm volatile("" ::: "memory");  // (keeps the bodies apart)
    } else {
      fnode_by_shape<C, TOTAL, OPS, SH, I + 1>(shape, cx, a, f, r, me, slot, sink);
    }
  } else {
    RecNode nd{r, me};
    fnode_body<C, TOTAL, OPS>(cx, a, f, nd, slot, sink);
  }
}
template <class C, bool TOTAL, class OPS, class SH>
__device__ __forceinline__ void fwalk_shaped(WalkCtx &cx, int node_begin, int &sink) {
  const Hot a = hot_args<C, OPS>(cx);
  FR_ZEROED_FRAMES(f);
  const void *shape_ids = uniform_ptr(cx.a->shape_ids);
  uint32_t rec_off = (uint32_t)node_begin * 64u;
  int slot = 0;
  Rec8 r = load_rec8(a.recs, rec_off);
  int shape = at_offset(shape_ids, rec_off >> 4)[0];
  while (shape >= 0) {   // (the sentinel's shape index is -1)
    const int next_shape = at_offset(shape_ids, (rec_off + 64u) >> 4)[0];   // (in flight over the node)
    fnode_by_shape<C, TOTAL, OPS, SH, 0>(shape, cx, a, f, r, rec_off, slot, sink);
    shape = next_shape;
    rec_off += 64u;
    slot += a.cps;
  }
}

// Template recursion over the records of PG: the walk as straight-line code.  PC: the record; GB:
// the first record of its group (carry slots count from there).
template <class C, bool TOTAL, class OPS, class PG, int PC, int GB>
__device__ __forceinline__ void fwalk_static(WalkCtx &cx, const Hot &a, double (&f)[C::MAXLV][C::EP],
                                             int &sink) {
  if constexpr (StaticNode<PG, PC>::klevel != kRecSentinelLevel) {
    StaticNode<PG, PC> nd;
    fnode_body<C, TOTAL, OPS>(cx, a, f, nd, a.slot_base + a.cps * (PC - GB), sink);
    fwalk_static<C, TOTAL, OPS, PG, PC + 1, GB>(cx, a, f, sink);
  }
}
// the group a unit walks is a run-time value: one straight-line walk per group
template <class C, bool TOTAL, class OPS, class PG, int G>
__device__ __forceinline__ void fwalk_static_group(WalkCtx &cx, int g0, int &sink) {
  if constexpr (G < PG::groups) {
    if (g0 == G) {
      const Hot a = hot_args<C, OPS>(cx);
      FR_ZEROED_FRAMES(f);
      fwalk_static<C, TOTAL, OPS, PG, PG::group_begin[G], PG::group_begin[G]>(cx, a, f, sink);
    } else {
      fwalk_static_group<C, TOTAL, OPS, PG, G + 1>(cx, g0, sink);
    }
  }
}

// A large plan in pieces (plan.h, PiecedProgram): a kernel of this kind walks the items of ONE
// piece type - PG::w holds the records of the type's body, a forest of whole sub-tries as
// straight-line code, its output rows and carry slots counted from the item's - behind a CHAIN,
// the path from the trie's root to the node the forest hangs below, walked by the record loop in
// frame 0.  A unit = the items [unit_begin[u], unit_begin[u + 1]) on one series, one staging of
// its rows.
template <class C, bool TOTAL, class OPS, class PG>
__device__ __forceinline__ void fwalk_pieces(WalkCtx &cx, int unit, int &sink) {
  Hot a = hot_args<C, OPS>(cx);   // (op_base and slot_base move with the items)
  FR_ZEROED_FRAMES(f);
  const void *items = uniform_ptr(cx.a->piece_items);
  const void *unit_begin = uniform_ptr(cx.a->piece_unit_begin);
  uint32_t it = (uint32_t)at_offset(unit_begin, (uint32_t)unit * 4u)[0] * 16u;
  const uint32_t it_end = (uint32_t)at_offset(unit_begin, (uint32_t)unit * 4u)[1] * 16u;
  for (; it < it_end; it += 16u) {
    cptr<int32_t> iw = at_offset(items, it);
    uint32_t rec_off = (uint32_t)iw[0];
    const int row_base = iw[1], node_base = iw[2];
    // the chain: every node continues frame 0 (the semiring's one in front of the first)
    semiring_one<C>(f[0]);
    a.op_base = 0;
    int slot = a.cps * node_base;
    fwalk_records<C, TOTAL, OPS>(cx, a, f, rec_off, slot, sink);
    a.op_base = (uint32_t)row_base * a.op_row_bytes;
    a.slot_base = slot;
    fwalk_static<C, TOTAL, OPS, PG, 0, 0>(cx, a, f, sink);
  }
}

// Stages the rows of one time chunk of series n into LDS (coalesced 16-byte units, the loads of
// kStageRows rows in flight before the first LDS write); with a fused preparation the rows are
// formed from the RAW input on the way (INC / NEW(INC) / STD, see IssArgs::prep).
template <class C>
__device__ __forceinline__ void stage_chunk(const WalkCtx &cx, const IssArgs &a, int64_t n, int64_t t0,
                                            double *rows_w) {
  const int tid = cx.tid;
  for (int r0 = 0; r0 < a.R; r0 += kStageRows) {
    constexpr int U = C::CHUNK / 2 / kWalkThreads;
    vd2 v[kStageRows][U];
#pragma unroll
    for (int rr = 0; rr < kStageRows; ++rr) {
      if (r0 + rr < a.R) {
        const int src = as_const(a.row_src)[r0 + rr];
        if (a.prep != nullptr && src >= 0) {
          // INC (x[t] - x[t - lag], zero-padded: fruits/cache.py:8-13), NEW(INC) (the prepared
          // dimension names a raw dimension and a lag) and STD's apply step ((x - mean) /
          // (std + eps), fruits/preparation/transform.py:141-147; statistics: row_stats_kernel)
          const int raw = as_const(a.prep)[4 * src], lag = as_const(a.prep)[4 * src + 1];
          const bool standardise = as_const(a.prep)[4 * src + 2] != 0;
          const double *gp = a.X + (n * a.D + raw) * a.T;
          double mean = 0.0, den = 1.0;
          if (standardise) {
            mean = as_const(a.stats)[(n * a.n_prep + src) * 2];
            den = as_const(a.stats)[(n * a.n_prep + src) * 2 + 1];
          }
#pragma unroll
          for (int k = 0; k < U; ++k) {
            const int i = 2 * (k * kWalkThreads + tid);
            const int64_t t = t0 + i;
            double e0 = 0.0, e1 = 0.0;
            if (t < a.T) e0 = gp[t];
            if (t + 1 < a.T) e1 = gp[t + 1];
            if (lag > 0) {
              e0 = (t >= lag && t < a.T) ? e0 - gp[t - lag] : 0.0;
              e1 = (t + 1 >= lag && t + 1 < a.T) ? e1 - gp[t + 1 - lag] : 0.0;
            }
            if (standardise) {
              e0 = (e0 - mean) / den;
              e1 = (e1 - mean) / den;
            }
            // (elements beyond T stay what the unfused path stages there: zeros)
            v[rr][k] = vd2{t < a.T ? e0 : 0.0, t + 1 < a.T ? e1 : 0.0};
          }
        } else {
          const double *gp =
              src >= 0 ? a.X + (n * a.D + src) * a.T
                       : a.aux + (int64_t)(-src - 1) * a.aux_tab_stride + n * a.aux_n_stride;
#pragma unroll
          for (int k = 0; k < U; ++k) {
            const int i = 2 * (k * kWalkThreads + tid);
            const int64_t t = t0 + i;
            v[rr][k] = vd2{0.0, 0.0};
            if (a.vec_ok) {
              if (cx.full_chunk || t < a.T) v[rr][k] = *reinterpret_cast<const vd2 *>(gp + t);
            } else {
              if (t < a.T) v[rr][k].x = gp[t];
              if (t + 1 < a.T) v[rr][k].y = gp[t + 1];
            }
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
}

// LDS of the fused kernel: rows [R][CHUNK] | totals window [2][8] | tails [2][4] | carries
// [carry_slots] (MULTI) | feature window (values, populations)
// (No waves-per-SIMD attribute: every instance fits 128 VGPRs - four waves - without one, and
// with it the 8-level one-chunk instances spilled a few registers for nothing.)
template <class C, bool TOTAL, class OPS = DynOps, class PG = NoProg>
__global__ __launch_bounds__(kWalkThreads) void iss_fused_kernel(const IssArgs a) {
  static_assert((C::MODE == 1 || C::MODE == 2) && C::TEAM == 4 && (C::P == 1 || C::MODE == 2) && C::MULTI != 2,
                "fused (MODE 1) or lean materialising (MODE 2) configuration");
  extern __shared__ double lds[];
  const int tid = threadIdx.x;
  WalkCtx cx;
  cx.a = &a;
  cx.rows = lds;
  cx.tot = lds + (int64_t)a.R * C::CHUNK;
  cx.tail = cx.tot + 16;
  cx.carry = cx.tail + 8;
  cx.tid = tid;
  cx.lane = tid & 63;
  cx.wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  cx.team = 0;
  cx.buf = 0;
  cx.tail_buf = 0;
  if constexpr (C::MODE == 2) {
    if (tid < 6) cx.tot[(tid / 3) * 8 + tid % 3] = semi_zero<C::SEMI>();
  } else {
    double *fw = cx.carry + (C::MULTI == 1 ? a.carry_slots : 0);
    cx.fl_val = (lds_f64 *)fw;
    cx.fl_cnt = (lds_f64 *)(fw + a.feat_window);
    for (int sl = tid; sl < a.feat_window; sl += kWalkThreads) {
      cx.fl_val[sl] = 0.0;
      if (a.has_mpi) cx.fl_cnt[sl] = 0.0;
    }
    // the identity slots of both totals windows
    if (tid < 6) cx.tot[(tid / 3) * 8 + tid % 3] = semi_zero<C::SEMI>();
    cx.fused_used = 0;
    cx.fslot = 0;
    cx.feat_window = a.feat_fits ? 0x3fffffff : a.feat_window;
  }
  // one workgroup per unit (series n, group g0); with the xcd numbering the groups of one
  // series meet in one XCD's L2 (speed only)
  const WalkUnit unit = walk_unit((int)blockIdx.x, a.G, a.xcd_map != 0);
  const int64_t n = unit.n;
  const int g0 = unit.g;
  int node_begin = 0;
  if constexpr (!PG::is_piece) node_begin = as_const(a.group_begin)[g0];
  int sink = 0;
  cx.pc_begin = node_begin;
  cx.series = n;   // (feature rows, cut rows: addressed from it where they are needed)
  for (int chunk = 0; chunk < a.nchunks; ++chunk) {
    const int64_t t0 = (int64_t)chunk * C::CHUNK;
    cx.t0 = t0;
    cx.parity = chunk & 1;
    cx.first_chunk = chunk == 0;
    // (OPS::full_chunks - a run-time compiled kernel for a series length that is a multiple of the
    // chunk: the ops' paths for ragged chunks are not even compiled)
    cx.full_chunk = OPS::full_chunks || t0 + C::CHUNK <= a.T;
    if (chunk > 0) lds_barrier();  // all reads of the old rows are done
    stage_chunk<C>(cx, a, n, t0, lds);
    __syncthreads();
    if constexpr (C::MODE == 2) {
      cx.out_base = a.out + n * a.out_n_stride + t0;
    } else {
      cx.fused_used = 0;  // same slots in every chunk
      cx.frow0 = as_const(PG::is_piece ? a.piece_unit_row0 : a.group_row_begin)[g0];
    }
    static_assert(!(PG::is_piece || PG::is_static || PG::is_shaped) || (OPS::is_static && C::MODE == 1),
                  "a kernel that knows its plan is a fused one and comes with static ops");
    if constexpr (PG::is_piece) fwalk_pieces<C, TOTAL, OPS, PG>(cx, g0, sink);
    else if constexpr (PG::is_static) fwalk_static_group<C, TOTAL, OPS, PG, 0>(cx, g0, sink);
    else if constexpr (PG::is_shaped) fwalk_shaped<C, TOTAL, OPS, PG>(cx, node_begin, sink);
    else fwalk<C, TOTAL, OPS>(cx, node_begin, sink);
    if constexpr (C::MODE == 1) {
      // a unit whose features fit the window keeps them there over its time chunks; else every
      // chunk leaves its share (added onto the earlier chunks' in global memory)
      if (!a.feat_fits || chunk + 1 == a.nchunks) feat_flush<C>(cx, !a.feat_fits && chunk > 0);
    }
  }
  if (sink == 0x7fffffff) (C::MODE == 2 ? a.out : a.feats)[0] = 0.0;   // (keeps the cache-touching loads alive)
}

#undef FR_ZEROED_FRAMES

}  // namespace fr
