// The development switches (environment variables), one spelling per parse rule; DESIGN.md section 1 lists every switch with its rule,
// default and the time it is read. env_on: only a value that starts with 1 enables; env_not_off: any value that does not start with 0
// enables; both give dflt when the variable is not set. env_int: atoi of the value.
#pragma once
#include <cstdlib>

namespace dc {

inline bool env_set(const char *name) { return getenv(name) != nullptr; }
inline bool env_on(const char *name, bool dflt) { const char *e = getenv(name); return e ? e[0] == '1' : dflt; }
inline bool env_not_off(const char *name, bool dflt) { const char *e = getenv(name); return e ? e[0] != '0' : dflt; }
inline int env_int(const char *name, int dflt) { const char *e = getenv(name); return e ? atoi(e) : dflt; }

// DC_PK_H16 (read once per process): 0 = the fp32 direction planes in the packet kernels' 20-rows-per-thread instances
inline int pk_h16_enabled() {
  static const int h16 = env_int("DC_PK_H16", 1);
  return h16;
}

}  // namespace dc
