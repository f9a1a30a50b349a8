// Host-side plan of the step kernels' dynamic LDS: how many bytes every launcher asks for, where the pieces lie in them, and the bounds the
// split plan (dc_clusterplan.cpp) accepts a part under. Plain C++17 integer arithmetic with no HIP header, so that the kernels, the launchers
// and the plan share ONE definition of each size and tests/native/launch_plan_check.cpp checks it on the CPU. The constexpr functions are
// usable in device code as they stand (hipcc treats constexpr functions as __host__ __device__). dc_launch.h is the HIP side.
#pragma once
#include <algorithm>
#include <cstddef>

namespace dc {

// ---- limits ----
constexpr int kLdsLimitBytes = 160 * 1024;      // LDS of a gfx950 CU: the most a workgroup can be granted
constexpr int kLdsReserveBytes = 256;           // kept free for an instance's static LDS (reduction scratch)
constexpr int kClusterLdsBytes = kLdsLimitBytes - kLdsReserveBytes;      // dynamic LDS a workgroup of the split kernels may ask for (the exchange's tail included)
constexpr int kDeflReserveBytes = 512;          // the deflated split instances have 384 bytes of static LDS more

// ---- sizes the kernels, the launchers and the plan share ----
constexpr int kXchWaves = 16;          // sum granules per (part, parity): one per wave of the publishing workgroup (<= 1024 threads)
constexpr int kXchLdsFloats = 32;      // tail of the dynamic LDS the exchange uses (lsum[2][4], ldead, padding; [16, 32): the six-sum totals, two parities of 8)
constexpr int kGranuleBytes = 16;      // one exchange granule {x, y, z, tag} (v4i, dc_cluster.h)
constexpr long long kSpinLimit = 200000000ll;     // bound of every spin of the exchange: 2 s of the 100 MHz wall clock
constexpr int kSelfCells = 4096;               // bins of the 2-D broad-phase grid of the self-contact detection
constexpr int kSelfDetectLdsInts = 16 + (kSelfCells + 1) + kSelfCells + 1 + 2048;   // LDS ints self_detect_rollout needs
constexpr int kPkOfsBatchInt4 = 4 * 64 + 32;   // 16-byte units of a 64-row chunk's batch (12 non-zeros per row) in the packet matrix's byte-offset layout (dc_packets.h)
constexpr int kPkTplSlots = 12;                // column offsets of the packet matrix's template layout (dc_packets.h): one batch per row
constexpr int kPkTplBatchInt4 = 3 * 64;        // 16-byte units of a 64-row chunk in that layout: 12 values per row, nothing else
// bytes of zero rows the template layout keeps on each side of the direction's 8-byte rows: a slot of a boundary row may point max_abs_off rows
// before row 0 or behind the last row
constexpr int pk_tpl_guard_bytes(int max_abs_off) { return (8 * max_abs_off + 15) / 16 * 16; }
constexpr int kCoarseVectors = 16;
constexpr int kCoarseLdsFloats = 2 * (16 * 3 * kCoarseVectors + 3 * kCoarseVectors);      // scratch of precondition64 in floats (16 = waves or parts, at most)
// explicit inverse of small systems (dc_denselib.h): number of column chunks the product is split into so that every wave of the workgroup
// has ~4 (row group, chunk) units, and the floats of LDS the partial sums need
constexpr int dense_chunks(int ld, int waves) {
  const int R = ld >> 6;
  const int C = (4 * waves + R - 1) / R;
  return C < 1 ? 1 : (C > 8 ? 8 : C);
}
constexpr int dense_lds_floats(int ld, int waves) { return 3 * ld * dense_chunks(ld, waves); }

constexpr int round4(int floats) { return (floats + 3) / 4 * 4; }

// ---- one workgroup per rollout ----
// forward, packet kernel (dc_forward_pk_kernel.h): direction (8-byte rows with H16) + XL rows of the iterate per thread, the explicit inverse's
// partial sums behind them; the element windows and the inlined detection reuse the same bytes. guard_bytes: the zero rows on each side of the
// direction when the packet matrix is in its template layout (pk_tpl_guard_bytes), 0 otherwise
inline size_t pk_lds_bytes(int threads, int vpt, int xl, bool h16, bool dense, int dense_ld, bool win_ok, int win_lds_bytes, bool inline_detect, int guard_bytes = 0) {
  size_t lds = (size_t) threads * ((h16 ? 2 : 3) * vpt + 3 * xl) * sizeof(float) + 2 * (size_t) guard_bytes;
  if (dense) lds += sizeof(float) * (size_t) dense_lds_floats(dense_ld, threads / 64);
  if (win_ok) lds = std::max(lds, (size_t) win_lds_bytes);
  if (inline_detect) lds = std::max(lds, sizeof(int) * (size_t) kSelfDetectLdsInts);
  return lds;
}
// forward, resident kernel (dc_forward_res.hip): the search direction
inline size_t res_lds_bytes(int threads, int vpt) { return (size_t) 3 * threads * vpt * sizeof(float); }
// adjoint (dc_adjoint.hip), before the y list: the element windows, or what the explicit inverse / the coarse level need when that is more;
// nothing without windows
inline size_t adj_lds_bytes(int threads, bool win_ok, int win_lds_bytes, bool dense, int dense_ld, bool coarse) {
  if (!win_ok) return 0;
  size_t lds = (size_t) win_lds_bytes;
  if (dense) lds = std::max(lds, sizeof(float) * (size_t) (3 * dense_ld + dense_lds_floats(dense_ld, threads / 64)));
  if (coarse) lds = std::max(lds, sizeof(float) * (size_t) kCoarseLdsFloats);
  return lds;
}
// The contact vertices' y list (AdjCtx::ylist) in what `lds` bytes of windows leave of the CU's LDS — for the 1024-thread kernels, which have
// their CU to themselves at 128 registers per lane whatever their LDS (4 waves per SIMD): the larger request costs no mesh a second workgroup
// per CU. `lds_limit` = what the device grants a workgroup, `static_lds` = the instance's own static LDS: both queried by the launcher, not
// assumed. 12 bytes per entry, at most one entry per vertex and two per self contact; `bytes` = the launch's dynamic LDS with the list.
struct AdjYlist { int ycap, ybase; size_t bytes; };
inline AdjYlist adj_ylist(int threads, size_t lds, size_t lds_limit, size_t static_lds, int N, int self_cap) {
  AdjYlist y{0, (int) (lds / 4), lds};
  const size_t reserve = static_lds + kLdsReserveBytes;
  if (threads != 1024 || lds + reserve + 12 > lds_limit) return y;
  y.ycap = (int) std::min((lds_limit - reserve - lds) / 12, (size_t) N + 2 * (size_t) self_cap);
  y.bytes = lds + (size_t) y.ycap * 12;
  return y;
}

// The tail of the list's room (3 * ycap floats from ybase), from its end backwards: the contact mask (one bit per vertex, adj_mask_words), one
// count per mask word of the set bits in the words before it (the same number of words), and the step-resident contact tables of
// adjoint_operator (dc_adjoint.hip). With the list ordered by vertex index a contact vertex's slot is its rank among the mask's set bits.
constexpr int adj_mask_words(int N) { return 2 * ((N + 63) >> 6); }
constexpr int adj_rank(const unsigned *mask, const unsigned *prefix, int i) {
  return (int) prefix[i >> 5] + __builtin_popcount(mask[i >> 5] & ((1u << (i & 31)) - 1u));
}
// floats of the tables: a four-word header; per self contact the float4 normal (with its two slots) and the float4 d; per working-set slot
// 1 / mass and the vertex; the layer offsets; per primitive-contact vertex nine planes (vertex, working-set slot or -1, n, d, mu)
constexpr int adj_tables_floats(int nplist, int nself_verts, int nself, int nlayers) {
  return round4(4 + 8 * nself + 2 * nself_verts + (nlayers + 1) + 9 * nplist);
}
// "fits": list (an entry per primitive-contact vertex and per working-set vertex), mask, counts and tables (with 3 floats for their 16-byte
// alignment) inside the room, and the tables inside `tab_cap` floats (BwdArgs::ytab: 0 = no tables, the test hook caps them)
constexpr bool adj_tables_fit(int ycap, int N, int nplist, int nself_verts, int nself, int nlayers, int tab_cap) {
  const long long tab = adj_tables_floats(nplist, nself_verts, nself, nlayers);
  return tab <= tab_cap && 3ll * (nplist + nself_verts) + 2ll * adj_mask_words(N) + tab + 3 <= 3ll * ycap;
}

// ---- split execution: K workgroups per rollout, R rows and HB boundary rows each side per part ----
// forward (dc_forward_cl_kernel.h): [0, fric_floats) the gather arrays of the CG — with the single-exchange loop (`pipe`) the direction as
// 8-byte rows and the neighbours' residual rows — or the element windows, which is also what the layered friction pass is offered; the
// inlined detection may need more; the exchange's tail at tail_off (floats).
struct ClForwardLds { int fric_floats, tail_off; size_t bytes; bool ok; };
inline ClForwardLds cl_forward_lds(int R, int HB, int win_lds_bytes, bool pipe, bool detect, bool defl) {
  const int GL = R + 2 * HB, fric_floats = std::max((pipe ? 2 : 3) * GL + (pipe ? 6 * HB : 0), win_lds_bytes / 4);
  const int tail_off = round4(detect ? std::max(fric_floats, kSelfDetectLdsInts) : fric_floats);
  const size_t bytes = sizeof(float) * (size_t) (tail_off + kXchLdsFloats);
  // (defl: ClusterPlan::fit accepts parts up to kClusterLdsBytes, so a plan within kDeflReserveBytes of the cap is refused here by the deflated
  // instances alone; launch_plan_check.cpp counts such plans on its grids)
  return {fric_floats, tail_off, bytes, bytes <= (size_t) (kClusterLdsBytes - (defl ? kDeflReserveBytes : 0))};
}
// adjoint (dc_adjoint_cl.hip): the element windows, the six halo rows at hc_off, the exchange's tail at tail_off (floats)
struct ClAdjointLds { int hc_off, tail_off; size_t bytes; bool ok; };
inline ClAdjointLds cl_adjoint_lds(int HB, int win_lds_bytes) {
  const int hc_off = round4(win_lds_bytes / 4), tail_off = hc_off + 6 * HB;
  const size_t bytes = sizeof(float) * (size_t) (tail_off + kXchLdsFloats);
  return {hc_off, tail_off, bytes, bytes <= (size_t) kClusterLdsBytes};
}
// What ClusterPlan::fit accepts a part under: upper bounds, in floats before the tail, on cl_forward_lds / cl_adjoint_lds over every instance the
// launchers can choose (pipe and detect on or off; `vpt` rows per thread). Forward: with GL = R + 2 HB the launcher needs at most
// max(2 GL + 6 HB, 3 GL, windows, detection). Up to 6 rows per thread the bound's 6 GL covers 2 GL + 6 HB because GL >= 3 HB (HB <= R); with more
// rows R > 3072 >= 4 HB (HB <= 512), so GL >= 6 HB and 3 GL covers it. The adjoint's bound is its tail_off exactly. cl_bound_fits leaves 4 floats
// for the forward's rounding to a multiple of 4. Which plans are accepted is behaviour: the arithmetic is the one the planner has always used
// (tests/native/cluster_plan_check.cpp pins it), and launch_plan_check.cpp checks on its grids that no accepted plan is refused by a launcher.
inline int cl_forward_floats_bound(int vpt, int R, int HB, int win_floats) { return std::max(std::max((vpt <= 6 ? 6 : 3) * (R + 2 * HB), win_floats), kSelfDetectLdsInts); }
inline int cl_adjoint_floats_bound(int HB, int win_floats) { return round4(win_floats) + 6 * HB; }
inline bool cl_bound_fits(int floats) { return floats + 4 <= kClusterLdsBytes / 4 - kXchLdsFloats; }

}  // namespace dc
