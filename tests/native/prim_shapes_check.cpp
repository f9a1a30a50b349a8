// Per-rollout obstacle shapes: the conversion of csrc/dc_primshape.h — dc_primitive -> shape row of 8 numbers -> fp32 row -> the shape fields
// of the device primitive — value for value. dc_build's fill and the host setters of dc_set_primitive_shapes both call these functions, so what
// holds here holds for a context BUILT with a shape and for a context GIVEN it.
#include <cmath>
#include <cstdio>
#include <cstring>
#include "dc_primshape.h"

static int failures = 0;
#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); failures++; } \
  } while (0)

static unsigned bits(float f) { unsigned u; std::memcpy(&u, &f, 4); return u; }

// the field names of the device primitive (csrc/dc_device.h: DevPrim); the fields the conversion must NOT touch carry sentinels
struct Prim {
  int kind = 77, group = 78, rotates = 79, pad = 80;
  float cx = 1.5f, cy = 2.5f, cz = 3.5f, radius = -1.f;
  float tx = -1.f, ty = -1.f, tz = -1.f, length = -1.f;
  float ux = -1.f, uy = -1.f, uz = -1.f, pad2 = 9.f;
};

int main() {
  static_assert(dc::kShapeRow == 8, "a shape row has 8 numbers");
  dc_primitive q;
  std::memset(&q, 0, sizeof q);
  q.kind = DC_PRIM_CAPSULE; q.group = 3; q.mu = 0.4; q.rotates = 1;
  q.center[0] = 10; q.center[1] = 11; q.center[2] = 12;
  // fp64 numbers that are no fp32 numbers, every field another
  q.top_offset[0] = 0.1; q.top_offset[1] = 3.0 + 1e-9; q.top_offset[2] = -0.7;
  q.corner2[0] = 1.5 + 1e-12; q.corner2[1] = -2.0 / 3.0; q.corner2[2] = 1e-3;
  q.radius = 2.125 + 1e-9; q.length = 3.3;

  // (a) the row is the fields of the same names, in the documented order, unrounded
  double row[8];
  dc::primitive_shape_row(q, row);
  const double want[8] = {q.top_offset[0], q.top_offset[1], q.top_offset[2], q.corner2[0], q.corner2[1], q.corner2[2], q.radius, q.length};
  for (int k = 0; k < 8; k++) CHECK(row[k] == want[k]);

  // (b) each value is rounded once to fp32
  float r32[8];
  dc::round_shape_row(row, r32);
  for (int k = 0; k < 8; k++) { CHECK(bits(r32[k]) == bits((float) want[k])); CHECK((double) r32[k] != want[k]); }
  // 1 + 2^-24 + 2^-30 lies above the midpoint of 1 and 1 + 2^-23: one rounding goes up
  const double mid[8] = {1.0 + std::ldexp(1.0, -24) + std::ldexp(1.0, -30), 0, 0, 0, 0, 0, 0, 0};
  float m32[8];
  dc::round_shape_row(mid, m32);
  CHECK(m32[0] == 1.0f + std::ldexp(1.0f, -23));

  // (c) fp32 input (a float32 tensor at the device-pointer boundary, widened by the cast kernel) gives the same bits as its widened value
  float in32[8];
  for (int k = 0; k < 8; k++) in32[k] = (float) want[k];
  float from32[8];
  dc::round_shape_row(in32, from32);
  for (int k = 0; k < 8; k++) CHECK(bits(from32[k]) == bits(r32[k]));

  // (d) the row lands in the shape fields of the device primitive and nowhere else
  Prim d;
  dc::shape_row_to_prim(r32, d);
  CHECK(bits(d.tx) == bits(r32[0]) && bits(d.ty) == bits(r32[1]) && bits(d.tz) == bits(r32[2]));
  CHECK(bits(d.ux) == bits(r32[3]) && bits(d.uy) == bits(r32[4]) && bits(d.uz) == bits(r32[5]));
  CHECK(bits(d.radius) == bits(r32[6]) && bits(d.length) == bits(r32[7]));
  CHECK(d.kind == 77 && d.group == 78 && d.rotates == 79 && d.pad == 80);
  CHECK(d.cx == 1.5f && d.cy == 2.5f && d.cz == 3.5f && d.pad2 == 9.f);

  // (e) dc_build's one call: the fields are what the plain casts gave before the conversion had a header of its own
  Prim b;
  dc::primitive_shape_to_prim(q, b);
  CHECK(bits(b.radius) == bits((float) q.radius) && bits(b.length) == bits((float) q.length));
  CHECK(bits(b.tx) == bits((float) q.top_offset[0]) && bits(b.ty) == bits((float) q.top_offset[1]) && bits(b.tz) == bits((float) q.top_offset[2]));
  CHECK(bits(b.ux) == bits((float) q.corner2[0]) && bits(b.uy) == bits((float) q.corner2[1]) && bits(b.uz) == bits((float) q.corner2[2]));
  CHECK(b.kind == 77 && b.cx == 1.5f && b.pad2 == 9.f);
  // given equals built: a caller's row holding the same fp64 numbers
  Prim g;
  float g32[8];
  dc::round_shape_row(want, g32);
  dc::shape_row_to_prim(g32, g);
  CHECK(std::memcmp(&g, &b, sizeof(Prim)) == 0);

  // (f) signed zero and large / tiny values survive as fp32 has them
  const double edge[8] = {-0.0, 1e-50, 1e30, -1e-40, 16777217.0, 0.5, 0.0, 1.0};
  float e32[8];
  dc::round_shape_row(edge, e32);
  CHECK(bits(e32[0]) == 0x80000000u && e32[1] == 0.0f && e32[2] == 1e30f && e32[4] == 16777216.0f && e32[5] == 0.5f);

  if (failures) { std::printf("%d FAILED\n", failures); return 1; }
  std::printf("ALL OK\n");
  return 0;
}
