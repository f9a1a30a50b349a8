// Movable obstacles (dc_set_primitive_offsets / dc_set_primitive_offset_schedule): the ONE rule that turns a per-group offset into the
// fp32 centre a flattened primitive is tested at. Plain C++ — the host path (dc_engine.hip), the conversion kernel of the device-pointer
// boundary (dc_boundary.hip) and the native check (tests/native/prim_offsets_check.cpp) all call these functions.
//
//   centre_p = fp32( (double) dc_primitive.center_p + d[group of p] )
//
// The sum is formed in fp64 and rounded once, so a context BUILT at the moved centre (its DevPrim holds fp32(center + d), with the caller
// adding in fp64) and a context GIVEN the offset see the same fp32 centre, bit for bit. A zero offset gives fp32(center): the built centre.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DC_HD __host__ __device__
#else
#define DC_HD
#endif

namespace dc {

DC_HD inline float offset_centre(double built, double offset) { return (float) (built + offset); }

// The centres [P][3] of one rollout's flattened primitives from its offsets d[G][3] (null = none): primitive p takes the offset of its
// compacted group group_of_prim[p] (the children of a LowerLeg share one and move together).
template <class T>
DC_HD inline void expand_centres(int P, const double *built /*[P][3]*/, const int *group_of_prim /*[P]*/, const T *d /*[G][3] or null*/, float *out /*[P][3]*/) {
  for (int p = 0; p < P; p++)
    for (int k = 0; k < 3; k++) out[3 * p + k] = offset_centre(built[3 * p + k], d ? (double) d[3 * group_of_prim[p] + k] : 0.0);
}

}  // namespace dc
