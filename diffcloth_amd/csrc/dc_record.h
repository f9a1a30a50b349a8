// Host-side import of a forward record handed in from outside (dc_set_record): the caller's layered self-contact lists and primitive indices
// turned into the record layout the detection kernel leaves (dc_selflib.h) — contacts by layer, pairs in device numbering (.x = the caller's
// smaller id), working-set slots = rank of the caller's ids among the contact vertices, offsets and counts in the meta block. Plain C++: no
// device is needed, tests/native/record_import_check.cpp checks the layout on the CPU. dc_engine.hip uploads the vectors.
#pragma once
#include <string>
#include <vector>
#include "../../include/diffcloth_hip.h"

namespace dc {
namespace rec {

// dc_device.h's kMetaStride / kMaxLayers and HIP's int2 / float4 under names of their own (that header needs the HIP runtime);
// dc_engine.hip asserts that they agree
constexpr int kMetaStride = 4096;
constexpr int kMaxLayers = 4088;
struct alignas(8) Int2 { int x, y; };
struct alignas(16) Float4 { float x, y, z, w; };

}  // namespace rec

struct HostRecord {
  std::vector<int> meta;               // [B][kMetaStride]
  std::vector<int> verts;              // [B][2 * cap] contact vertices in device numbering, in the order of the caller's ids
  std::vector<rec::Int2> pair;         // [B][cap]
  std::vector<rec::Float4> nrm, dvec;  // [B][cap] normal (.w = bits of slot1 | slot2 << 16), d
  std::vector<double> sn, sd;          // [B][cap][3] the normals and d as passed (fp64)
  std::vector<int> prim;               // [B][N] primitive per vertex in device numbering, -1 = none
  int code = DC_OK;
  std::string error;

  // user_of / dev_of: the context's renumbering (empty = identity). False: `code` and `error` say why, the vectors are unspecified.
  bool build(const dc_record &r, int B, int N, int cap, int np, const std::vector<int> &user_of, const std::vector<int> &dev_of);
};

}  // namespace dc
