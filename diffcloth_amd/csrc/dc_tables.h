// Host-side table plan of a context: every table dc_build uploads besides the plain HostSystem arrays, in exactly the layout the kernels
// read (dc_device.h: DevSystem), and the kernel-set decisions that follow from them. Built from the HostSystem, the parameters and the
// values of the development switches that gate tables; no device is needed, so a host-only context (dc_create(-1)) reports the decisions
// of the same code a device context runs, and tests/native/host_tables_check.cpp checks the tables on the CPU.
// The deflation space of the forward solve stays with the context (its cache survives rebuilds): the plan supplies the row padding of its
// tables (defl_rows) and turns the outcome into fwd_defl / adj_coarse (set_deflation).
#pragma once
#include <vector>
#include "../../include/diffcloth_hip.h"
#include "dc_dense.h"
#include "dc_packets.h"
#include "dc_system.h"
#include "dc_windows.h"

namespace dc {

constexpr size_t kWindowLdsBudget = (size_t) 150 * 1024;   // LDS the element windows of the one-workgroup kernels may take

inline int round64(int v) { return (v + 63) / 64 * 64; }

// values of the development switches dc_build reads (defaults: everything on)
struct TableSwitches {
  bool windows = true;      // DC_WINDOWS=0: no element windows, the global-memory corner passes
  int dense_max_n = 0;      // DC_DENSE_MAX_N: largest mesh that gets the explicit inverse (0 disables)
  bool self_lds = true;     // DC_SELF_LDS=0: layered self-contact passes through global memory
  bool adj_coarse = true;   // DC_ADJ_COARSE=0: no coarse level over the deflation space in the adjoint's fall-back
  bool pk_h16 = true;       // DC_PK_H16=0: the packet kernels' 20- and 14-rows-per-thread instances keep the fp32 direction planes
  bool pk_ofs = true;       // DC_PK_OFS=0: the instances with the direction as halves read the packet matrix in its first layout
  bool pk_tpl = true;       // DC_PK_TPL=0: a matrix with a column-offset template keeps the byte-offset layout too
  int pk_threads = 0;       // DC_PK_THREADS: 512 / 768 = threads of the packet kernel where both shapes exist (0: the default, dc_kernelplan.h)
  bool bend_rows = true;    // DC_BEND_ROWS=0: a mesh whose flaps are all flat at rest keeps the per-flap passes too (dc_windows.h: rows)
};

struct HostTables {
  // ---- decisions ----
  int bandwidth = 0;                   // max |column - row| of P
  int win_ok = 0, nwin = 0;            // element windows (win)
  int pk_ok = 0, pk_vpt = 0, pk_threads = 0;   // packet matrix (pk): rows per thread and threads of its kernel, 0 when the tables are refused
  int bend_rows = 0;                   // the windows of the one-workgroup kernels carry the bending term as matrix rows, no flaps (win.rows)
  int pk_ofs = 0;                      // pk is in the byte-offset layout (dc_packets.h): the kernel that runs holds the direction as halves
  int pk_tpl = 0, pk_guard_bytes = 0;  // set_deflation: pk went on to the template layout (values only, dc_packets.h); the zero rows each side of the direction
  int defl_rows = 0;                   // row padding of the deflation tables: the packet kernel's rows, or N rounded up to 64; 0 = no space wanted
  int fwd_defl = 0, adj_coarse = 0;    // set_deflation
  bool defl_built = false;             // set_deflation: the context has a deflation space
  int dense_ld = 0;                    // explicit inverse (dense): its leading dimension, 0 = not built
  int self_cap = 0, self_lds = 1;
  float max_radii = 0.f;

  // ---- tables ----
  std::vector<int> tri_v, bend_v;      // [3][T], [4][E] planar vertex indices
  std::vector<float> bend_nw;          // [E][2] (rest norm, weight^2)
  std::vector<float> dinv;             // [N] 1 / P_ii
  std::vector<int> att_of_vertex;      // [N] fixed-point index or -1
  std::vector<double> tri_D64, bend_w64, bend_nw64;   // [4][T], [4][E], [2][E] planar fp64 rest-shape tables
  std::vector<float> tri_Dlo, bend_lo; // [T][4], [E][4] value - fl32(value): inv_deltaUV; cotan weights 1..3 and the rest norm (.w)
  std::vector<int> ell;                // wave-sliced ELL copy of P: (column, float bits) per entry; padding entries (min(row, N - 1), 0.0f)
  std::vector<int> ell_ptr, ell_w;     // per 64-row chunk: first entry, width (its widest row)
  std::vector<float> sq_dinv;          // without packet tables only: [round64(N)] sqrt(1 / P_ii) (with them: pk.sq_dinv)
  HostWindows win;
  HostPackets pk;
  HostDense dense;

  void build(const HostSystem &H, const dc_params &p, const TableSwitches &sw);
  // `built`: the context has a deflation space for defl_rows rows. Also the last layout decision, which needs this one: the packet matrix
  // goes from byte offsets to the template layout when it has a template, the plain (not deflated) halves instance runs, and the guard rows
  // fit the LDS and one store per thread; otherwise it stays in the byte-offset layout, byte for byte
  void set_deflation(bool built, const TableSwitches &sw);
  // the decisions as the kernel choices of dc_kernelplan.h take them (after set_deflation)
  PlanFacts facts(int N) const;
};

}  // namespace dc
