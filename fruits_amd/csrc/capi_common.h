// What the units of the C ABI (capi_*.cpp) share: the plan handle, the calling thread's error
// state, the knob readers and a few small helpers.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/fruits_hip.h"
#include "launch_choice.h"
#include "plan.h"

struct fr_plan {
  fr::Plan *p;
};

namespace fr::capi {

// (defined in capi_core.cpp)
extern thread_local std::string g_err;   // what fr_last_error returns
extern thread_local int g_last_code;     // of the entry points that return a handle (fr_select_ranks_begin)

int fail(int code, const std::string &msg);
int hip_fail(hipError_t e, const char *what);

#define HIP_TRY(expr)                                                \
  do {                                                               \
    hipError_t e_ = (expr);                                          \
    if (e_ != hipSuccess) return ::fr::capi::hip_fail(e_, #expr);    \
  } while (0)

// The tail of an entry that launches one kernel: FR_OK, or the failure `e` of the launch `what`.
// With a `limit_msg`, hipErrorInvalidValue is the launcher's refusal of a grid or a shape:
// FR_E_LIMIT with exactly that text.
inline int launched(hipError_t e, const char *what, const char *limit_msg = nullptr) {
  if (e == hipSuccess) return FR_OK;
  if (e == hipErrorInvalidValue && limit_msg) {
    (void)hipGetLastError();
    return fail(FR_E_LIMIT, limit_msg);
  }
  return hip_fail(e, what);
}

int env_int(const char *name, int dflt);
int debug_knob(const char *name, int dflt);   // FRUITS_HIP_DEBUG="name=value,..." (capi_core.cpp)
fr::WalkKnobs read_walk_knobs();

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

bool stream_is_capturing(hipStream_t st);
int current_device_id();
int claim_device(fr::Plan &p, const char *who);
// frees the backward tables a plan holds (capi_grad.cpp; fr_plan_destroy)
void release_grad_tables(fr::Plan &p);

}  // namespace fr::capi
