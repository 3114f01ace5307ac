// The launch-plan option table (options.h, options.inc) and its three C-ABI entry points.  Host code only.
#include <atomic>
#include <cstring>

#include "../../include/mmdeer.h"
#include "common.h"
#include "options.h"

namespace mmdeer {

namespace {
struct OptEntry { const char* name; int dflt, lo, hi; std::atomic<int> value; };
OptEntry g_opts[OPT_COUNT] = {
#define X(id, name, dflt, lo, hi) {name, dflt, lo, hi, {dflt}},
#include "options.inc"
#undef X
};
OptEntry* find(const char* name) {
  for (auto& o : g_opts)
    if (name && strcmp(name, o.name) == 0) return &o;
  return nullptr;
}
}  // namespace

int opt(OptId id) { return g_opts[id].value.load(std::memory_order_relaxed); }
const char* opt_name(int i) { return (i >= 0 && i < OPT_COUNT) ? g_opts[i].name : nullptr; }
int opt_set(const char* name, int value) {
  OptEntry* o = find(name);
  if (!o) return -1;
  if (value < o->lo || value > o->hi) return -2;
  o->value.store(value, std::memory_order_relaxed);
  return 0;
}
int opt_range(const char* name, int* lo, int* hi) {
  const OptEntry* o = find(name);
  if (!o) return -1;
  if (lo) *lo = o->lo;
  if (hi) *hi = o->hi;
  return 0;
}
int opt_get(const char* name, int* value) {
  const OptEntry* o = find(name);
  if (!o) return -1;
  if (value) *value = o->value.load(std::memory_order_relaxed);
  return 0;
}

}  // namespace mmdeer

using namespace mmdeer;

extern "C" {

int mmdeer_set_option(const char* name, int value) {
  const int rc = opt_set(name, value);
  if (rc == -2) {
    int lo = 0, hi = 0;
    opt_range(name, &lo, &hi);
    MMDEER_CHECK(false, "set_option: %s = %d is outside [%d, %d]", name, value, lo, hi);
  }
  MMDEER_CHECK(rc == 0, "set_option: unknown option '%s'", name ? name : "(null)");
  return 0;
}
int mmdeer_get_option(const char* name, int* value) {
  MMDEER_CHECK(opt_get(name, value) == 0, "get_option: unknown option '%s'", name ? name : "(null)");
  return 0;
}
const char* mmdeer_option_name(int i) { return opt_name(i); }

}  // extern "C"
