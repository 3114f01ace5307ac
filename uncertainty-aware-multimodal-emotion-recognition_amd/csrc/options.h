// Launch-plan options of libmmdeer_hip.so (include/mmdeer.h: mmdeer_set_option / mmdeer_get_option).
// The library reads no environment variable: the defaults are the shipped plan, and a host that wants another one says
// so through the C ABI (mmdeer/_lib.py forwards MMDEER_<NAME> environment variables at load time for the A/B tools).
// Options are read at every call, so a process can switch plans between calls; the table is the library's only mutable
// process-wide state besides the communicator handles of comm.hip.
#pragma once

namespace mmdeer {

enum OptId {   // options.inc: what each option selects
#define X(id, name, dflt, lo, hi) id,
#include "options.inc"
#undef X
  OPT_COUNT
};

int opt(OptId id);                          // current value
int opt_set(const char* name, int value);   // 0 = ok, -1 = unknown name, -2 = value outside the option's range
int opt_range(const char* name, int* lo, int* hi);
int opt_get(const char* name, int* value);  // 0 = ok, -1 = unknown name
const char* opt_name(int i);                // nullptr past the end

}  // namespace mmdeer
