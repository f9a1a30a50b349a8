// Arguments, LDS plan and launcher of the self-contact read-out (dc_self_readout.hip; dc_get_self_contact_readout[_dev]). The plan is plain
// integer arithmetic shared by the kernel, the launcher and the engine, in the manner of dc_launchplan.h.
#pragma once
#include <hip/hip_runtime.h>
#include "dc_device.h"
#include "dc_launchplan.h"

namespace dc {

// values per (slot, rollout) of the read-out's totals: {contacts evaluated, layers, distinct vertices, sum jn, sum |r_k - jn_k n_k|, take-off,
// stick, slide}
constexpr int kSelfRoTotals = 8;
// floats of dynamic LDS a workgroup of the read-out may plan with at most (its static LDS, the totals' partial sums, fits the reserve)
constexpr int kSelfRoLdsFloatsMax = (kLdsLimitBytes - kLdsReserveBytes) / 4;

// The kernel's LDS image of one record with M working-set vertices, C contacts and nl layers, in floats from the start of the dynamic LDS:
//   [0, 4C)            float4 normal of every contact, .w its two working-set slots (SelfRec::nrm)
//   [4C, 4C + 6M)      double r_self[3][M], the per-vertex sums
//   then f[3][M], g - f = r[3][M] (r_p at the start), 1 / m [M], and the nl + 1 layer offsets
constexpr long long selfro_lds_need(int M, int C, int nl) { return 4ll * C + 13ll * M + nl + 1; }

// What the host can know without a synchronisation: the largest record the context can hold has min(N, 2 self_cap) working-set vertices,
// self_cap contacts and kMaxLayers layers. `limit` = floats the kernel may plan with (kSelfRoLdsFloatsMax, or less under DC_TEST_SELFRO_LDS).
// lds_floats: dynamic LDS of every launch; scratch: some record may not fit it, the global-memory walk needs its [B][3][N] planes.
struct SelfRoPlan { int lds_floats; bool scratch; };
inline SelfRoPlan selfro_plan(int N, int self_cap, int limit) {
  limit = std::max(0, std::min(limit, kSelfRoLdsFloatsMax));
  const long long need = selfro_lds_need(std::min(N, 2 * self_cap), self_cap, kMaxLayers);
  return {(int) std::min<long long>(need, limit), need > limit};
}

struct SelfRoArgs {
  const float *F, *NRM;       // [rows][3][N] of the range's first row, as every pointer below
  const int *PRIM;            // [rows][N]
  const float *PV;            // [rows][G][kPvRow] or null
  const float *mu;            // [B][G]
  SelfRec R;
  int B, row0;                // rollouts per slot; first row of this launch (rows count from the range's first record)
  int cap_out;                // entries per row of pairs / impulse
  int lds_floats;             // dynamic LDS of the launch, in floats
  float *scratch;             // [B][3][N] g - f of the rows that do not fit the LDS, or null: every possible record fits
  double *sums;               // [B][3][N] their per-vertex sums
};
// (launch_self_readout is declared with the other launchers in dc_device.h)

}  // namespace dc
