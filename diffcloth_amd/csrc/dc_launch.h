// HIP side of the launch plan (dc_launchplan.h has the sizes): the one place that configures a kernel instance's dynamic LDS.
#pragma once
#include <hip/hip_runtime.h>
#include "dc_launchplan.h"

namespace dc {

constexpr int kMaxDevices = 64;       // devices whose granted requests are remembered

// Makes sure the instance `Kernel` may be launched with `bytes` of dynamic LDS on the current device. The attribute is per (device, instance)
// and only ever raised here, so a high-water mark per device saves the call on every later launch; a request is recorded only once the
// runtime has granted it. Device ordinals outside [0, kMaxDevices) are not cached: the attribute is set on every launch.
template <auto Kernel>
hipError_t ensure_dynamic_lds(size_t bytes) {
  static size_t granted[kMaxDevices] = {};
  int dev = 0;
  (void) hipGetDevice(&dev);
  const bool cached = dev >= 0 && dev < kMaxDevices;
  if (cached && bytes <= granted[dev]) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute((const void *) Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) bytes);
  if (e == hipSuccess && cached) granted[dev] = bytes;
  return e;
}

}  // namespace dc
