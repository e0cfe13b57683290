// pnode_amd -- the one way the kernel files launch: plainly, or between two profiling events while profiling is on
// (pn_prof_enable; the bookkeeping lives in pn_kernels.hip behind pn::prof_events), and then a look at hipGetLastError.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <string>

#include "pn_dispatch.h"
#include "pn_internal.h"

namespace pn {

inline int check_launch(const char *name) {
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(std::string(name) + ": " + hipGetErrorString(err));
  return 0;
}

// kid >= 0: booked under that kernel id with `bytes` while profiling is on; kid < 0: never profiled.  Errors name `name`.
// The argument structs travel by value into the launch.
// Threads: prof_events books the record under the profiling lock and releases it before the launch below, so between
// the two another thread's pn_prof_collect (or the drain of a full record list) can meet a record whose events no launch
// has recorded yet, and a launch that fails leaves such a record behind; either ends that drain with a "prof:" error.
// Profile with one launching thread, and collect from that thread or after joining it.
template <typename Kern, typename... Args>
int launch_as(const char *name, int kid, double bytes, Kern kern, dim3 grid, dim3 block, hipStream_t st, const Args &...args) {
  void *e0 = nullptr, *e1 = nullptr;
  const int prof = kid < 0 ? 0 : prof_events(kid, bytes, &e0, &e1);
  if (prof < 0) return 1;
  if (prof) hipExtLaunchKernelGGL(kern, grid, block, 0, st, (hipEvent_t)e0, (hipEvent_t)e1, 0, args...);
  else hipLaunchKernelGGL(kern, grid, block, 0, st, args...);
  return check_launch(name);
}

// a profiled kernel: errors carry its pn_kernel_name
template <typename Kern, typename... Args>
int launch(int kid, double bytes, Kern kern, dim3 grid, dim3 block, hipStream_t st, const Args &...args) {
  return launch_as(pn_kernel_name(kid), kid, bytes, kern, grid, block, st, args...);
}

// an unprofiled kernel: errors carry the entry point's name
template <typename Kern, typename... Args>
int launch(const char *name, Kern kern, dim3 grid, dim3 block, hipStream_t st, const Args &...args) {
  return launch_as(name, -1, 0.0, kern, grid, block, st, args...);
}

// the refusal of a with_count / with_dtype that found no case
inline int or_fail(int rc, const char *text) { return rc == kNoCase ? fail(text) : rc; }

}  // namespace pn
