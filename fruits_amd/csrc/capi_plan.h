// The plan's side of the C ABI (capi_plan.cpp) as the walk runner and the pipeline see it.
#pragma once
#include <map>

#include "capi_common.h"
#include "jit.h"

namespace fr::capi {

// Run-time compiled static programs of a plan (jit.cpp), by groups per series.
struct JitState {
  std::map<int, fr::JitProgram> progs;
  bool tried = false;
  std::string error;     // why the plan has none (not an error of the caller's)
};

// One-time uploads of a plan's tables (synchronous: never inside a capture).  Caller holds p.mu.
int ensure_device_program(fr::Plan &p, fr::GroupedProgram &gp, hipStream_t st, const char *who);
int ensure_cos_program(fr::Plan &p, fr::CosProgram &c, hipStream_t st, const char *who);

int64_t query_mixed_resident(int prog, int64_t N, int64_t T);

// Caller holds p.mu.
void ensure_jit(fr::Plan &p);
void lookup_static_programs(fr::Plan &p);
fr::WalkFacts walk_facts(fr::Plan &p, int64_t N, int64_t T, int groups, bool fused, bool total_inc,
                         bool vec_ok, const fr::WalkKnobs &k);

int prepare_plan(fr::Plan &p, int64_t N, int64_t T, int32_t groups, bool fused, const char *who,
                 const fr::WalkKnobs &k);

struct WorkLayout {
  size_t aux_bytes = 0, carry_bytes = 0;
  size_t total() const { return aux_bytes + carry_bytes; }
};

WorkLayout work_layout(const fr::Plan &p, int64_t N, int64_t T, int64_t lookup_rows);

}  // namespace fr::capi
