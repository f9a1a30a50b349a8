// The development switches (environment variables), one spelling per parse rule; DESIGN.md section 1 lists every switch with its rule,
// default and the time it is read. env_on: only a value that starts with 1 enables; env_not_off: any value that does not start with 0
// enables; both give dflt when the variable is not set. env_int: atoi of the value.
#pragma once
#include <cstdlib>
#include "dc_kernelplan.h"

namespace dc {

inline bool env_set(const char *name) { return getenv(name) != nullptr; }
inline bool env_on(const char *name, bool dflt) { const char *e = getenv(name); return e ? e[0] == '1' : dflt; }
inline bool env_not_off(const char *name, bool dflt) { const char *e = getenv(name); return e ? e[0] != '0' : dflt; }
inline int env_int(const char *name, int dflt) { const char *e = getenv(name); return e ? atoi(e) : dflt; }

// The switches that select kernel instances (dc_kernelplan.h: KernelSwitches), read once per process at the first dc_build: DC_FWD_VARIANT,
// DC_PK_H16, DC_BWD_THREADS, DC_SXCG
inline const KernelSwitches &kernel_switches() {
  static const KernelSwitches sw = [] {
    KernelSwitches s;
    if (env_set("DC_FWD_VARIANT")) s.fwd_variant = getenv("DC_FWD_VARIANT")[0] == 'g' ? kFwdVariantGlobal : env_int("DC_FWD_VARIANT", kFwdVariantDefault);
    s.pk_h16 = env_int("DC_PK_H16", 1) != 0;
    s.bwd_threads = env_int("DC_BWD_THREADS", 0);
    s.sxcg = env_not_off("DC_SXCG", true);
    return s;
  }();
  return sw;
}

// DC_TEST_SELFRO_LDS: floats of LDS the self-contact read-out's kernel may plan with (dc_self_readout.h), read at every read-out call; not
// set, 0 or negative = all a workgroup can have. A small value sends the rows through the kernel's global-memory walk.
inline int selfro_lds_limit(int dflt) { const int v = env_int("DC_TEST_SELFRO_LDS", 0); return v > 0 ? v : dflt; }

}  // namespace dc
