// Movable obstacles: the rounding rule and the group -> flattened-primitive expansion of csrc/dc_primoffset.h, the plain-C++ functions the
// engine's host path and the conversion kernel of the device-pointer boundary both call, against answers worked out by hand.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "dc_primoffset.h"

static int failures = 0;
#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); failures++; } \
  } while (0)

static unsigned bits(float f) { unsigned u; std::memcpy(&u, &f, 4); return u; }

int main() {
  using dc::offset_centre;
  // (a) zero offset: the built fp32 centre, whatever the double was
  const double c0 = 0.1 + 1e-12;      // not an fp32 number
  CHECK(bits(offset_centre(c0, 0.0)) == bits((float) c0));
  // (b) the sum is formed in fp64 and rounded ONCE. c = 1 + 2^-24 (the midpoint between the fp32 numbers 1 and 1 + 2^-23; fp32(c) = 1 by
  // round-to-even), d = 2^-30: c + d lies above the midpoint, so one rounding gives 1 + 2^-23, while rounding the centre first and adding
  // in fp32 gives fp32(1 + 2^-30) = 1, and rounding both terms first gives the same wrong 1.
  const double c = 1.0 + std::ldexp(1.0, -24), d = std::ldexp(1.0, -30);
  const float once = offset_centre(c, d);
  CHECK(once == 1.0f + std::ldexp(1.0f, -23));
  CHECK((float) c + (float) d == 1.0f);
  CHECK(once != (float) c + (float) d);
  // (c) a context built at the moved centre sees fp32(center + d) with the caller adding in fp64: the same bits
  const double cs[4] = {-0.5, 3.14159265358979, 1e-3, -16.0}, ds[4] = {0.125, -4.0, 0.03125 * 3, 1e-9};
  for (double cc : cs) for (double dd : ds) CHECK(bits(offset_centre(cc, dd)) == bits((float) (cc + dd)));
  // (d) dyadic centres and offsets are exact
  CHECK(offset_centre(2.5, 0.0625 + 0.03125 * 4) == 2.6875f);

  // (e) expansion: 5 flattened primitives in 3 compacted groups — a sphere (group 0), a LowerLeg's three children (group 1: joint, foot, leg,
  // one offset moves all of them), a plane (group 2)
  const int P = 5, G = 3;
  const double built[P * 3] = {0, 1, 2,   10, 11, 12,   10, 10, 10,   10, 11.5, 12,   -1, -2, -3};
  const int group_of_prim[P] = {0, 1, 1, 1, 2};
  const double off[G * 3] = {0.5, 0, 0,   0, 0.25, -0.25,   0, 0, 8};
  float out[P * 3];
  dc::expand_centres(P, built, group_of_prim, off, out);
  const float want[P * 3] = {0.5f, 1, 2,   10, 11.25f, 11.75f,   10, 10.25f, 9.75f,   10, 11.75f, 11.75f,   -1, -2, 5};
  for (int k = 0; k < P * 3; k++) CHECK(out[k] == want[k]);
  // the children keep their distances: one offset per group
  CHECK(out[3 * 3 + 1] - out[3 * 1 + 1] == 0.5f && out[3 * 2 + 1] - out[3 * 1 + 1] == -1.0f);
  // fp32 offsets (a float32 tensor at the device-pointer boundary) are widened exactly before the fp64 sum
  const float off32[G * 3] = {0.5f, 0, 0,   0, 0.25f, -0.25f,   0, 0, 8};
  float out32[P * 3];
  dc::expand_centres(P, built, group_of_prim, off32, out32);
  for (int k = 0; k < P * 3; k++) CHECK(bits(out32[k]) == bits(want[k]));
  // null offsets: the built centres, rounded
  dc::expand_centres(P, built, group_of_prim, (const double *) nullptr, out);
  for (int k = 0; k < P * 3; k++) CHECK(bits(out[k]) == bits((float) built[k]));
  // no primitives: nothing is read or written
  float guard = 7.f;
  dc::expand_centres(0, (const double *) nullptr, (const int *) nullptr, off, &guard);
  CHECK(guard == 7.f);

  if (failures) { std::printf("%d FAILED\n", failures); return 1; }
  std::printf("ALL OK\n");
  return 0;
}
