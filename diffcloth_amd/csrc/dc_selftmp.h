// Size of the per-rollout scratch of the self-contact layering (DevWork::sd_tmp; layout: SelfTmp in dc_selflib.h).
#pragma once
#include "dc_launchplan.h"      // kSelfCells, kSelfDetectLdsInts
namespace dc {
// in ints; U = 2 cap + 2 entries per per-vertex array (a contact list of C pairs has at most 2 C distinct vertices)
__host__ __device__ constexpr int self_tmp_ints(int cap) { return 10 * (2 * cap + 2) + 4 * cap + 16; }
}  // namespace dc
