// C ABI of libfruits_hip.so (see include/fruits_hip.h for the contract and the reference
// interfaces each entry point replaces): the error state, the knob readers and the entries that
// wrap the runtime.  The rest of the ABI: capi_plan.cpp, capi_walk.cpp, capi_pipeline.cpp,
// capi_select.cpp, capi_kernels.cpp.
#include <cstdlib>
#include <cstring>

#include "capi_common.h"

namespace fr::capi {

thread_local std::string g_err;
thread_local int g_last_code = 0;

int fail(int code, const std::string &msg) {
  g_err = msg;
  g_last_code = code;
  return code;
}

int hip_fail(hipError_t e, const char *what) {
  g_err = std::string(what) + ": " + hipGetErrorString(e);
  g_last_code = FR_E_HIP;
  return FR_E_HIP;
}

int env_int(const char *name, int dflt) {
  const char *v = std::getenv(name);
  return v && *v ? std::atoi(v) : dflt;
}

// Developer knobs live in ONE variable: FRUITS_HIP_DEBUG="name=value,name=value" with
//   groups=G    groups of root sub-tries per series instead of the host's choice
//   persist=P   1 / 0: persistent grid / one workgroup per unit for the materialising walk
//   packed=0    cooperative kernels also for short series (the wave-per-series ones are default)
//   stamps=M    the diagnostic timing build's mask (IssArgs::debug), dbg_bytes=B its stamp buffer
//   wt=0        static programs keep plain output stores (no write-through instance)
//   tail=S      ahead-of-time static programs with a tail program (the same plan in finer units):
//               0 - never the mixed launch; S > 0 - the last min(S, N) series as finer units at
//               any N; unset / -1 - choose_walk_launch's rule
// Nothing here changes a result; the product reads none of them in normal operation.
int debug_knob(const char *name, int dflt) {
  const char *v = std::getenv("FRUITS_HIP_DEBUG");
  if (!v || !*v) return dflt;
  const size_t n = std::strlen(name);
  for (const char *p = v; *p;) {
    if (std::strncmp(p, name, n) == 0 && p[n] == '=') return std::atoi(p + n + 1);
    while (*p && *p != ',') ++p;
    if (*p == ',') ++p;
  }
  return dflt;
}

// The knobs and switches a launch reads: once per entry-point call, and on every call (a test
// flips FRUITS_HIP_DEBUG between two runs of one plan).  The only reader of the environment on
// the way to a launch: the choice itself (launch_choice.h) sees this struct.
fr::WalkKnobs read_walk_knobs() {
  fr::WalkKnobs k;
  const struct { const char *name; int *value; } debug[] = {
      {"groups", &k.groups}, {"persist", &k.persist}, {"packed", &k.packed}, {"lean", &k.lean},
      {"wt", &k.wt}, {"tail", &k.tail}, {"static_cache_x100", &k.static_cache_x100},
      {"static_min_T", &k.static_min_T}, {"stamps", &k.stamps}, {"dbg_bytes", &k.dbg_bytes}};
  for (const auto &d : debug) *d.value = debug_knob(d.name, *d.value);
  k.hip_static = env_int("FRUITS_HIP_STATIC", k.hip_static);
  k.hip_jit = env_int("FRUITS_HIP_JIT", k.hip_jit);
  return k;
}

// A stream that is being captured into a hipGraph must not see allocations or
// synchronous copies: the one-time uploads below refuse to run then (the caller
// prepares the plan first: fr_plan_prepare / fr_pipeline_prepare).
bool stream_is_capturing(hipStream_t st) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return cs != hipStreamCaptureStatusNone;
}

int current_device_id() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) (void)hipGetLastError();
  return dev;
}

// The tables of a plan live on the device that was current at their first upload.
int claim_device(fr::Plan &p, const char *who) {
  const int dev = current_device_id();
  if (p.device < 0) p.device = dev;
  if (p.device != dev)
    return fail(FR_E_ARG, std::string(who) + ": the plan's tables live on device " +
                              std::to_string(p.device) + " but device " + std::to_string(dev) +
                              " is current (plans are per device)");
  return FR_OK;
}

}  // namespace fr::capi

using namespace fr::capi;

extern "C" {

const char *fr_last_error(void) { return g_err.c_str(); }

int fr_version(void) { return 145; }

int fr_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}

int fr_malloc(void **d_ptr, int64_t bytes) {
  if (!d_ptr || bytes < 0) return fail(FR_E_ARG, "fr_malloc: bad argument");
  *d_ptr = nullptr;
  if (bytes == 0) return FR_OK;
  hipError_t e = hipMalloc(d_ptr, (size_t)bytes);
  if (e == hipErrorOutOfMemory) {
    (void)hipGetLastError();
    return fail(FR_E_NOMEM, "fr_malloc: out of device memory");
  }
  if (e != hipSuccess) return hip_fail(e, "hipMalloc");
  return FR_OK;
}

int fr_free(void *d_ptr) {
  if (!d_ptr) return FR_OK;
  HIP_TRY(hipFree(d_ptr));
  return FR_OK;
}

int fr_memcpy_h2d(void *d_dst, const void *h_src, int64_t bytes, void *stream) {
  if (bytes == 0) return FR_OK;
  if (!d_dst || !h_src || bytes < 0) return fail(FR_E_ARG, "fr_memcpy_h2d: bad argument");
  HIP_TRY(hipMemcpyAsync(d_dst, h_src, (size_t)bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
  return FR_OK;
}

int fr_memcpy_d2h(void *h_dst, const void *d_src, int64_t bytes, void *stream) {
  if (bytes == 0) return FR_OK;
  if (!h_dst || !d_src || bytes < 0) return fail(FR_E_ARG, "fr_memcpy_d2h: bad argument");
  HIP_TRY(hipMemcpyAsync(h_dst, d_src, (size_t)bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
  return FR_OK;
}

int fr_stream_sync(void *stream) {
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  return FR_OK;
}

}  // extern "C"
