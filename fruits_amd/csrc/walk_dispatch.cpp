// Host-only dispatch over the walk-kernel and CosWISS instances (walk_inst.hip,
// walk_packed_inst.hip, walk_static_inst.hip, coswiss_inst.hip): no kernel lives here.
#include "kernels.h"

namespace fr {

using InstFn = hipError_t (*)(const IssArgs &, int, hipStream_t);

// the instances, by mode and deepest level (walk_inst.hip): declared and tabled from one list
#define WALK_INSTS(X, m) X(m, 2) X(m, 4) X(m, 6) X(m, 8)
#define DECL_INST(m, l) hipError_t walk_inst_m##m##_l##l(const IssArgs &, int, hipStream_t);
WALK_INSTS(DECL_INST, 0) WALK_INSTS(DECL_INST, 1) WALK_INSTS(DECL_INST, 2)
hipError_t walk_static_launch(const IssArgs &, hipStream_t);
hipError_t walk_packed_inst_m0(const IssArgs &, int, hipStream_t);
hipError_t walk_packed_inst_m1(const IssArgs &, int, hipStream_t);

// [mode][level slot]: mode 0 the record interpreter, 1 the fused walk (features), 2 the fused
// walk's node loop with a store epilogue (walk_fused.h, MODE 2); slot s serves levels <= 2 s + 2
#define INST_NAME(m, l) walk_inst_m##m##_l##l,
static const InstFn kWalkInst[3][4] = {
    {WALK_INSTS(INST_NAME, 0)}, {WALK_INSTS(INST_NAME, 1)}, {WALK_INSTS(INST_NAME, 2)}};
#undef INST_NAME
#undef DECL_INST
#undef WALK_INSTS

hipError_t launch_iss_walk(IssArgs &a, int levels, hipStream_t st) {
  const int chunk = walk_chunk_elems(a.T);
  a.nchunks = (int32_t)((a.T + chunk - 1) / chunk);
  if (a.N * a.G <= 0) return hipSuccess;
  if (a.nchunks > 1 && a.carry == nullptr) return hipErrorInvalidValue;
  if (a.packed) {
    if (!packed_supported(a.T, levels, a.semiring)) return hipErrorInvalidValue;
    return a.feats ? walk_packed_inst_m1(a, levels, st) : walk_packed_inst_m0(a, levels, st);
  }
  int mode = 0;
  if (a.feats) mode = 1;
  else if (a.static_prog != 0) return walk_static_launch(a, st);
  else if (a.lean) mode = 2;
  const int slot = levels <= 2 ? 0 : levels <= 4 ? 1 : levels <= 6 ? 2 : 3;
  return kWalkInst[mode][slot](a, chunk, st);
}

// CosWISS: one kernel per (series, word, frequency) unit, see coswiss.h
#define DECL_COS(s) hipError_t coswiss_inst_s##s(const IssArgs &, int, hipStream_t);
DECL_COS(1) DECL_COS(2) DECL_COS(3) DECL_COS(4) DECL_COS(5) DECL_COS(6) DECL_COS(7) DECL_COS(8)
#undef DECL_COS
static const InstFn kCoswissInst[kCosMaxExponent] = {coswiss_inst_s1, coswiss_inst_s2, coswiss_inst_s3,
                                                     coswiss_inst_s4, coswiss_inst_s5, coswiss_inst_s6,
                                                     coswiss_inst_s7, coswiss_inst_s8};

hipError_t launch_coswiss(IssArgs &a, int exponent, hipStream_t st) {
  const int chunk = walk_chunk_elems(a.T);
  a.nchunks = (int32_t)((a.T + chunk - 1) / chunk);
  if (a.N * a.cw_W * a.cw_F <= 0) return hipSuccess;
  if (exponent < 1 || exponent > kCosMaxExponent) return hipErrorInvalidValue;
  return kCoswissInst[exponent - 1](a, chunk, st);
}

}  // namespace fr
