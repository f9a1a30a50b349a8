// Per-rollout obstacle shapes (dc_set_primitive_shapes / dc_set_primitive_shape_schedule): the ONE conversion between a dc_primitive, the
// shape row of 8 numbers the C-ABI takes per flattened primitive, and the shape fields of DevPrim. Plain C++ — dc_build's DevPrim fill, the
// host setters (dc_engine.hip) and the native check (tests/native/prim_shapes_check.cpp) all call these functions.
//
//   row = {top_offset[3], corner2[3], radius, length}          device value = fp32(row[k]), each value rounded once
//
// A context BUILT with a shape holds fp32 of its dc_primitive fields in DevPrim; a context GIVEN the same fp64 numbers as a row holds the same
// fp32 numbers in its table, bit for bit, because both go through shape_value below. No arithmetic happens here: a caller who wants a
// rotated obstacle rotates top_offset and corner2 (functional.rotated_primitive_shapes) and the rounding is applied to the result.
#pragma once
#include "../../include/diffcloth_hip.h"

namespace dc {

constexpr int kShapeRow = 8;      // numbers per flattened primitive

template <class T>
inline float shape_value(T v) { return (float) v; }

// the shape row of a dc_primitive as the caller would pass it (fp64, unrounded)
inline void primitive_shape_row(const dc_primitive &q, double row[kShapeRow]) {
  for (int k = 0; k < 3; k++) { row[k] = q.top_offset[k]; row[3 + k] = q.corner2[k]; }
  row[6] = q.radius; row[7] = q.length;
}

// a caller's row (fp64, or fp32 widened exactly) -> the fp32 row of the device table
template <class T>
inline void round_shape_row(const T *row, float out[kShapeRow]) {
  for (int k = 0; k < kShapeRow; k++) out[k] = shape_value(row[k]);
}

// the fp32 row -> the shape fields of a DevPrim (Prim: any struct with DevPrim's field names)
template <class Prim>
inline void shape_row_to_prim(const float row[kShapeRow], Prim &d) {
  d.tx = row[0]; d.ty = row[1]; d.tz = row[2];
  d.ux = row[3]; d.uy = row[4]; d.uz = row[5];
  d.radius = row[6]; d.length = row[7];
}

// dc_build: the shape fields of DevPrim from the dc_primitive, through the row
template <class Prim>
inline void primitive_shape_to_prim(const dc_primitive &q, Prim &d) {
  double row[kShapeRow];
  float r32[kShapeRow];
  primitive_shape_row(q, row);
  round_shape_row(row, r32);
  shape_row_to_prim(r32, d);
}

}  // namespace dc
