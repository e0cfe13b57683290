// pnode_amd -- internal helpers shared by the kernel launchers and the host engine.
#pragma once
#include <cstdint>
#include <string>

namespace pn {
// records the message for pn_last_error() and returns 1
int fail(const std::string &msg);
// For pn::launch (pn_launch.h).  0: profiling is off (launch plainly); 1: *e0 / *e1 are the start / stop events of the
// launch, the record is booked under kernel id `kid` with `bytes`; -1: failure (pn_last_error()).
int prof_events(int kid, double bytes, void **e0, void **e1);     // (hipEvent_t: this header is also read by plain g++)
// pn_wrms_partials(n): the doubles of the pinned block an error-norm launch over n entries writes -- the number of workgroups,
// then one partial per workgroup (at most one per kWrmsBlock entries) and a spare.  Here because the host finish of the
// infinity norm (pn_winf_finish, pn_ts.cpp) checks a block against it and pn_ts.cpp also links without the kernel files.
constexpr int kWrmsBlock = 256;
inline int64_t wrms_partials(int64_t n) { return (n + kWrmsBlock - 1) / kWrmsBlock + 2; }
}  // namespace pn
