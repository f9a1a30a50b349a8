// Host-side plan of the banded direct adjoint solve (dc_params::adjoint_mode = 3, dc_adjoint_band.h): the band's width and storage from the
// mesh's matrix bandwidth, and the one statement of which meshes the mode accepts. Plain C++17 integer arithmetic with no HIP header, in the
// style of dc_launchplan.h: the engine's checks (dc_set_params, dc_build, dc_set_adjoint_band), dc_get_adjoint_band on host-only contexts and
// the kernels' launchers share these definitions.
#pragma once
#include <algorithm>
#include <cstddef>
#include "dc_launchplan.h"

namespace dc {

constexpr int kBandPanel = 32;                               // columns of one LU panel (= kLuPanel of the dense solve)
constexpr long long kBandBudgetBytes = 8ll << 30;            // scratch of one chunk of rollouts, as the dense solve's
constexpr int kBandLdsReserveBytes = 1024;                   // kept free for the step kernel's static LDS (reduction scratch)
constexpr int kBandLdsBytes = kLdsLimitBytes - kBandLdsReserveBytes;      // dynamic LDS the band kernels may ask for

constexpr int band_round16(int v) { return (v + 15) / 16 * 16; }
// half-bandwidth kl = ku of K with the unknowns interleaved (3 i + c): P's bandwidth `bw` widened by `extra` vertices, 3 x 3 blocks
constexpr int band_kl(int N, int bw, int extra) {
  const long long w = std::min<long long>((long long) bw + (long long) extra, (long long) N);
  return (int) std::min<long long>(3ll * N - 1, 3 * w + 2);
}
// LAPACK-style band storage: kl rows of fill, ku super-diagonals, the diagonal, kl sub-diagonals
constexpr int band_ldab(int kl) { return band_round16(3 * kl + 1); }
constexpr long long band_bytes(int N, int kl) { return (long long) band_ldab(kl) * 3 * N * (long long) sizeof(double); }
// leading dimension of the factorisation's panel block (kBandPanel columns of kl + kBandPanel rows); the panel kernel holds it in LDS where
// it fits and works in global memory where it does not
constexpr int band_pld(int kl) { return band_round16(kl + kBandPanel); }
constexpr bool band_panel_in_lds(int kl) { return (long long) sizeof(double) * kBandPanel * band_pld(kl) <= (long long) kBandLdsBytes; }
// The substitution's panel block next to the right-hand side (3N doubles, rounded) in the step kernel's dynamic LDS: the multipliers of
// `cols` columns (kl each) in the forward sweep, as many as fit up to a panel, and the kBandPanel^2 diagonal block of the backward sweep.
// The least a mesh needs is one column.
constexpr int band_sub_cols(int N, int kl) {
  const long long room = (long long) kBandLdsBytes / (long long) sizeof(double) - band_round16(3 * N);
  return room < 1 ? 0 : (int) std::min<long long>(kBandPanel, room / std::max(kl, 1));
}
constexpr long long band_blk_doubles(int kl, int cols) { return std::max<long long>((long long) cols * kl, (long long) kBandPanel * kBandPanel); }
constexpr long long band_lds_bytes(int N, int kl, int cols) { return (long long) sizeof(double) * ((long long) band_round16(3 * N) + band_blk_doubles(kl, cols)); }

// Whether adjoint_mode 3 takes a mesh of N vertices with matrix bandwidth bw and `extra` vertices of widening: the band of one rollout
// within the budget, and the step kernel's LDS within what a workgroup is granted.
// (lds_bytes: with one column of multipliers, the least the solve can run with; sub_cols: the columns the step kernel will hold.)
struct BandPlan { int kl, ldab; long long bytes, lds_bytes; int sub_cols; bool ok; };
constexpr BandPlan band_plan(int N, int bw, int extra) {
  const int kl = band_kl(N, bw, extra);
  const long long bytes = band_bytes(N, kl), lds = band_lds_bytes(N, kl, 1);
  return {kl, band_ldab(kl), bytes, lds, band_sub_cols(N, kl), bytes <= kBandBudgetBytes && lds <= (long long) kBandLdsBytes};
}

}  // namespace dc
