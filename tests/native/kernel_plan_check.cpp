// Test harness (CPU): the host-side plan of which kernel instance runs a step (csrc/dc_kernelplan.h) — the forward, adjoint and split choices
// against answers written out by hand from the launchers as they were before the plan existed, and the closure of the choices over the
// instance tables for every mesh size, on the decisions HostTables::build really takes.
//   g++ -O2 -std=c++17 -Wall -I diffcloth_amd/csrc tests/native/kernel_plan_check.cpp diffcloth_amd/csrc/dc_tables.cpp
//       diffcloth_amd/csrc/dc_clusterplan.cpp diffcloth_amd/csrc/dc_system.cpp diffcloth_amd/csrc/dc_windows.cpp diffcloth_amd/csrc/dc_packets.cpp
//       diffcloth_amd/csrc/dc_dense.cpp -o kernel_plan_check
// Prints one line per group of checks and exits non-zero on the first failure (driven by tests/test_host_native.py).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>
#include "dc_clusterplan.h"
#include "dc_kernelplan.h"
#include "dc_tables.h"

using namespace dc;

static void fail(const std::string &what) { std::printf("FAIL %s\n", what.c_str()); std::exit(1); }

// ---- meshes ----
// triangle strip of N >= 3 vertices, vertex i at column i / 2 of row i % 2 (bandwidth 3 with the flaps); far > 0 exchanges the numbers of
// vertices 0 and far: the neighbours 1 ... 3 of the first then reach far - 1 columns, those of the other far + 3
static bool strip(HostSystem &H, int N, int far) {
  std::mt19937 rng(7);
  std::uniform_real_distribution<double> jit(-0.002, 0.002);
  std::vector<double> pos(3 * (size_t) N);
  std::vector<int> tri;
  auto name = [&](int v) { return far > 0 && v == 0 ? far : (far > 0 && v == far ? 0 : v); };
  for (int i = 0; i < N; i++) {
    const int v = name(i);
    pos[3 * v] = 0.05 * (i / 2) + jit(rng); pos[3 * v + 1] = 0.05 * (i % 2) + jit(rng); pos[3 * v + 2] = jit(rng);
  }
  for (int i = 0; i + 2 < N; i++) {
    if (i % 2 == 0) tri.insert(tri.end(), {name(i), name(i + 1), name(i + 2)});
    else tri.insert(tri.end(), {name(i + 1), name(i), name(i + 2)});
  }
  return H.set_mesh(N, pos.data(), (int) tri.size() / 3, tri.data()) && H.build_numerics(1.0 / 120, 0.3, 200.0, 0.02, 1e4);
}
// triangulated nx x ny grid in row-major numbering (the grid of cluster_plan_check.cpp / launch_plan_check.cpp)
static bool grid(HostSystem &H, int nx, int ny, int *bandwidth) {
  std::mt19937 rng(7);
  std::uniform_real_distribution<double> jit(-0.01, 0.01);
  std::vector<double> pos(3 * (size_t) nx * ny);
  std::vector<int> tri;
  for (int a = 0; a < ny; a++)
    for (int b = 0; b < nx; b++) {
      const int v = a * nx + b;
      pos[3 * v] = 0.05 * b + jit(rng); pos[3 * v + 1] = 0.05 * a + jit(rng); pos[3 * v + 2] = jit(rng);
    }
  for (int a = 0; a + 1 < ny; a++)
    for (int b = 0; b + 1 < nx; b++) {
      const int v00 = a * nx + b, v01 = v00 + 1, v10 = v00 + nx, v11 = v10 + 1;
      tri.insert(tri.end(), {v00, v01, v11});
      tri.insert(tri.end(), {v00, v11, v10});
    }
  if (!H.set_mesh(nx * ny, pos.data(), (int) tri.size() / 3, tri.data()) || !H.build_numerics(1.0 / 120, 0.3, 200.0, 0.02, 1e4)) return false;
  *bandwidth = 0;
  for (int r = 0; r < H.N; r++)
    for (int k = H.P_ptr[r]; k < H.P_ptr[r + 1]; k++) *bandwidth = std::max(*bandwidth, std::abs(H.P_col[k] - r));
  return true;
}

// ---- the switch combinations ----
struct Combo {
  int win = 1, h16 = 1, pk_threads = 0;      // DC_WINDOWS, DC_PK_H16, DC_PK_THREADS (0 = unset)
  int variant = kFwdVariantDefault;          // DC_FWD_VARIANT: unset, 0, 1, kFwdVariantGlobal
  int defl = 0, inv = 1, ofs = 1;            // a deflation space is built when the plan wants one; DC_DENSE_MAX_N = 768 or 0; DC_PK_OFS
};
static TableSwitches table_switches(const Combo &q) {
  TableSwitches sw;
  sw.windows = q.win != 0; sw.pk_h16 = q.h16 != 0; sw.pk_threads = q.pk_threads; sw.pk_ofs = q.ofs != 0; sw.dense_max_n = q.inv ? 768 : 0;
  return sw;
}
static KernelSwitches kernel_switches_of(const Combo &q) {
  KernelSwitches k;
  k.fwd_variant = q.variant; k.pk_h16 = q.h16 != 0;
  return k;
}
static std::string tag(int N, const Combo &q, int bandwidth) {
  return "N " + std::to_string(N) + " windows " + std::to_string(q.win) + " h16 " + std::to_string(q.h16) + " pk_threads " + std::to_string(q.pk_threads) + " variant " +
         std::to_string(q.variant) + " deflation " + std::to_string(q.defl) + " inverse " + std::to_string(q.inv) + " ofs " + std::to_string(q.ofs) + " bandwidth " + std::to_string(bandwidth);
}
// the decisions of HostTables::build / set_deflation on a real mesh
static PlanFacts table_facts(const HostSystem &H, const Combo &q) {
  dc_params prm;
  std::memset(&prm, 0, sizeof(prm));
  prm.time_step = 1.0 / 120;
  const TableSwitches sw = table_switches(q);
  HostTables plan;
  plan.build(H, prm, sw);
  plan.set_deflation(q.defl && plan.defl_rows > 0, sw);
  return plan.facts(H.N);
}
// the same decisions from the shape rule alone (every N, no mesh), for a mesh whose windows and inverse build when they are wanted:
// windows_fit = its element windows fit the LDS budget
static PlanFacts rule_facts(int N, const Combo &q, int bandwidth, bool windows_fit, int win_lds_bytes) {
  PlanFacts f;
  f.N = N;
  f.win_ok = q.win && windows_fit;
  f.win_lds_bytes = f.win_ok ? win_lds_bytes : 0;
  const int shape = bandwidth <= 511 ? pk_shape_for(N, q.pk_threads) : -1;
  f.pk_ok = shape >= 0;
  if (f.pk_ok) { f.pk_threads = kPkShapes[shape].threads; f.pk_vpt = kPkShapes[shape].vpt; }
  f.pk_ofs = f.pk_ok && q.ofs && q.h16 && f.win_ok && kPkShapes[shape].xl_h16 >= 0;
  f.dense_inv = f.pk_ok && f.win_ok && q.inv && N <= 768;
  f.defl_space = q.defl && f.win_ok;
  f.fwd_defl = f.defl_space && (!f.pk_ok || kPkShapes[shape].defl);
  f.adj_coarse = f.defl_space;
  return f;
}
static bool same_facts(const PlanFacts &a, const PlanFacts &b) {
  return a.N == b.N && a.pk_ok == b.pk_ok && a.win_ok == b.win_ok && a.pk_ofs == b.pk_ofs && a.fwd_defl == b.fwd_defl && a.adj_coarse == b.adj_coarse &&
         a.pk_threads == b.pk_threads && a.pk_vpt == b.pk_vpt && a.defl_space == b.defl_space && a.dense_inv == b.dense_inv && a.win_lds_bytes == b.win_lds_bytes;
}

// ---- 1. pinned answers ----
enum { P = kFwdPacket, D = kFwdPacketDeflated, R = kFwdResident, G = kFwdGlobal };
struct Pin {
  int N; Combo q; int far;      // far: strip() — 508 gives bandwidth 511, 509 gives 512
  int family, threads, vpt, xl, h16, ofs, dense, fusable;
};
static Combo combo(int win, int h16, int pk_threads, int variant, int defl, int inv) {
  Combo q;
  q.win = win; q.h16 = h16; q.pk_threads = pk_threads; q.variant = variant; q.defl = defl; q.inv = inv;
  return q;
}
static const int U = kFwdVariantDefault, GL = kFwdVariantGlobal;
// Written down from launch_pd_step / launch_pd_step_packet(_deflated) / launch_pd_step_resident / HostPackets::build / HostTables::build as they
// stood before dc_kernelplan.h: packet rows per thread = the first of {1, 2, 3, 4, 6, 8, 10, 12, 16, 20} >= ceil(N / 512), XL 0 up to 12 rows,
// 2 at 16, 6 at 20 (12 with halves); 768 x 14 (XL 3, 7 with halves) only when forced and 9 216 < N <= 10 240; halves and byte offsets need
// DC_PK_H16 and the windows; the explicit inverse up to 768 vertices with packets and windows, used by the 1 ... 3-row instances; deflated
// instances for 512 threads x >= 4 rows; the resident ladder; the global kernel's 256 / 512 / 1024 threads.
static const Pin kPins[] = {
    //  N     win h16 thr var defl inv   far   family thr  vpt xl h16 ofs dense fusable
    // defaults, windows on and off
    {1,     combo(1, 1, 0, U, 0, 1), 0,   P, 512, 1, 0, 0, 0, 1, 1},    {1,     combo(0, 1, 0, U, 0, 1), 0,   P, 512, 1, 0, 0, 0, 0, 1},
    {512,   combo(1, 1, 0, U, 0, 1), 0,   P, 512, 1, 0, 0, 0, 1, 1},    {512,   combo(0, 1, 0, U, 0, 1), 0,   P, 512, 1, 0, 0, 0, 0, 1},
    {513,   combo(1, 1, 0, U, 0, 1), 0,   P, 512, 2, 0, 0, 0, 1, 1},    {513,   combo(0, 1, 0, U, 0, 1), 0,   P, 512, 2, 0, 0, 0, 0, 1},
    {1536,  combo(1, 1, 0, U, 0, 1), 0,   P, 512, 3, 0, 0, 0, 0, 1},    {1536,  combo(0, 1, 0, U, 0, 1), 0,   P, 512, 3, 0, 0, 0, 0, 1},
    {1537,  combo(1, 1, 0, U, 0, 1), 0,   P, 512, 4, 0, 0, 0, 0, 1},    {1537,  combo(0, 1, 0, U, 0, 1), 0,   P, 512, 4, 0, 0, 0, 0, 1},
    {2048,  combo(1, 1, 0, U, 0, 1), 0,   P, 512, 4, 0, 0, 0, 0, 1},    {2048,  combo(0, 1, 0, U, 0, 1), 0,   P, 512, 4, 0, 0, 0, 0, 1},
    {2049,  combo(1, 1, 0, U, 0, 1), 0,   P, 512, 6, 0, 0, 0, 0, 1},    {2049,  combo(0, 1, 0, U, 0, 1), 0,   P, 512, 6, 0, 0, 0, 0, 1},
    {4096,  combo(1, 1, 0, U, 0, 1), 0,   P, 512, 8, 0, 0, 0, 0, 1},    {4096,  combo(0, 1, 0, U, 0, 1), 0,   P, 512, 8, 0, 0, 0, 0, 1},
    {4097,  combo(1, 1, 0, U, 0, 1), 0,   P, 512, 10, 0, 0, 0, 0, 1},   {4097,  combo(0, 1, 0, U, 0, 1), 0,   P, 512, 10, 0, 0, 0, 0, 1},
    {5120,  combo(1, 1, 0, U, 0, 1), 0,   P, 512, 10, 0, 0, 0, 0, 1},   {5121,  combo(1, 1, 0, U, 0, 1), 0,   P, 512, 12, 0, 0, 0, 0, 1},
    {6144,  combo(1, 1, 0, U, 0, 1), 0,   P, 512, 12, 0, 0, 0, 0, 1},   {6144,  combo(0, 1, 0, U, 0, 1), 0,   P, 512, 12, 0, 0, 0, 0, 1},
    {6145,  combo(1, 1, 0, U, 0, 1), 0,   P, 512, 16, 2, 0, 0, 0, 1},   {6145,  combo(0, 1, 0, U, 0, 1), 0,   P, 512, 16, 2, 0, 0, 0, 1},
    {8192,  combo(1, 1, 0, U, 0, 1), 0,   P, 512, 16, 2, 0, 0, 0, 1},   {8192,  combo(0, 1, 0, U, 0, 1), 0,   P, 512, 16, 2, 0, 0, 0, 1},
    {8193,  combo(1, 1, 0, U, 0, 1), 0,   P, 512, 20, 12, 1, 1, 0, 1},  {8193,  combo(0, 1, 0, U, 0, 1), 0,   P, 512, 20, 6, 0, 0, 0, 1},
    {9216,  combo(1, 1, 0, U, 0, 1), 0,   P, 512, 20, 12, 1, 1, 0, 1},  {9216,  combo(0, 1, 0, U, 0, 1), 0,   P, 512, 20, 6, 0, 0, 0, 1},
    {9217,  combo(1, 1, 0, U, 0, 1), 0,   P, 512, 20, 12, 1, 1, 0, 1},  {9217,  combo(0, 1, 0, U, 0, 1), 0,   P, 512, 20, 6, 0, 0, 0, 1},
    {10000, combo(1, 1, 0, U, 0, 1), 0,   P, 512, 20, 12, 1, 1, 0, 1},  {10000, combo(0, 1, 0, U, 0, 1), 0,   P, 512, 20, 6, 0, 0, 0, 1},
    {10240, combo(1, 1, 0, U, 0, 1), 0,   P, 512, 20, 12, 1, 1, 0, 1},  {10240, combo(0, 1, 0, U, 0, 1), 0,   P, 512, 20, 6, 0, 0, 0, 1},
    {10241, combo(1, 1, 0, U, 0, 1), 0,   R, 1024, 12, 0, 0, 0, 0, 0},  {10241, combo(0, 1, 0, U, 0, 1), 0,   R, 1024, 12, 0, 0, 0, 0, 0},
    {10752, combo(1, 1, 0, U, 0, 1), 0,   R, 1024, 12, 0, 0, 0, 0, 0},  {10752, combo(0, 1, 0, U, 0, 1), 0,   R, 1024, 12, 0, 0, 0, 0, 0},
    {12288, combo(1, 1, 0, U, 0, 1), 0,   R, 1024, 12, 0, 0, 0, 0, 0},  {12288, combo(0, 1, 0, U, 0, 1), 0,   R, 1024, 12, 0, 0, 0, 0, 0},
    {12289, combo(1, 1, 0, U, 0, 1), 0,   G, 1024, 0, 0, 0, 0, 0, 0},   {12289, combo(0, 1, 0, U, 0, 1), 0,   G, 1024, 0, 0, 0, 0, 0, 0},
    // DC_PK_H16=0: fp32 planes, no offsets
    {8193,  combo(1, 0, 0, U, 0, 1), 0,   P, 512, 20, 6, 0, 0, 0, 1},   {10000, combo(1, 0, 0, U, 0, 1), 0,   P, 512, 20, 6, 0, 0, 0, 1},
    {8192,  combo(1, 0, 0, U, 0, 1), 0,   P, 512, 16, 2, 0, 0, 0, 1},   {512,   combo(1, 0, 0, U, 0, 1), 0,   P, 512, 1, 0, 0, 0, 1, 1},
    // DC_PK_THREADS: 512 = the default; 768 takes 768 x 14 for 9 217 ... 10 240 rows only
    {10000, combo(1, 1, 512, U, 0, 1), 0, P, 512, 20, 12, 1, 1, 0, 1},  {9217,  combo(1, 1, 512, U, 0, 1), 0, P, 512, 20, 12, 1, 1, 0, 1},
    {9216,  combo(1, 1, 768, U, 0, 1), 0, P, 512, 20, 12, 1, 1, 0, 1},  {9217,  combo(1, 1, 768, U, 0, 1), 0, P, 768, 14, 7, 1, 1, 0, 1},
    {10000, combo(1, 1, 768, U, 0, 1), 0, P, 768, 14, 7, 1, 1, 0, 1},   {10240, combo(1, 1, 768, U, 0, 1), 0, P, 768, 14, 7, 1, 1, 0, 1},
    {10241, combo(1, 1, 768, U, 0, 1), 0, R, 1024, 12, 0, 0, 0, 0, 0},  {10752, combo(1, 1, 768, U, 0, 1), 0, R, 1024, 12, 0, 0, 0, 0, 0},
    {9217,  combo(1, 0, 768, U, 0, 1), 0, P, 768, 14, 3, 0, 0, 0, 1},   {10000, combo(0, 1, 768, U, 0, 1), 0, P, 768, 14, 3, 0, 0, 0, 1},
    {8193,  combo(1, 1, 768, U, 0, 1), 0, P, 512, 20, 12, 1, 1, 0, 1},  {4096,  combo(1, 1, 768, U, 0, 1), 0, P, 512, 8, 0, 0, 0, 0, 1},
    // DC_FWD_VARIANT=0 / 1: the resident ladder and its second thread shape; never fusable
    {1,     combo(1, 1, 0, 0, 0, 1), 0,   R, 256, 1, 0, 0, 0, 0, 0},    {512,   combo(1, 1, 0, 0, 0, 1), 0,   R, 256, 2, 0, 0, 0, 0, 0},
    {513,   combo(1, 1, 0, 0, 0, 1), 0,   R, 256, 4, 0, 0, 0, 0, 0},    {1536,  combo(1, 1, 0, 0, 0, 1), 0,   R, 256, 6, 0, 0, 0, 0, 0},
    {1537,  combo(1, 1, 0, 0, 0, 1), 0,   R, 512, 4, 0, 0, 0, 0, 0},    {2048,  combo(1, 1, 0, 0, 0, 1), 0,   R, 512, 4, 0, 0, 0, 0, 0},
    {2049,  combo(1, 1, 0, 0, 0, 1), 0,   R, 512, 8, 0, 0, 0, 0, 0},    {4096,  combo(1, 1, 0, 0, 0, 1), 0,   R, 512, 8, 0, 0, 0, 0, 0},
    {4097,  combo(1, 1, 0, 0, 0, 1), 0,   R, 512, 12, 0, 0, 0, 0, 0},   {6144,  combo(1, 1, 0, 0, 0, 1), 0,   R, 512, 12, 0, 0, 0, 0, 0},
    {6145,  combo(1, 1, 0, 0, 0, 1), 0,   R, 1024, 8, 0, 0, 0, 0, 0},   {8192,  combo(1, 1, 0, 0, 0, 1), 0,   R, 1024, 8, 0, 0, 0, 0, 0},
    {8193,  combo(1, 1, 0, 0, 0, 1), 0,   R, 1024, 10, 0, 0, 0, 0, 0},  {10240, combo(1, 1, 0, 0, 0, 1), 0,   R, 1024, 10, 0, 0, 0, 0, 0},
    {10241, combo(1, 1, 0, 0, 0, 1), 0,   R, 1024, 12, 0, 0, 0, 0, 0},  {12288, combo(1, 1, 0, 0, 0, 1), 0,   R, 1024, 12, 0, 0, 0, 0, 0},
    {12289, combo(1, 1, 0, 0, 0, 1), 0,   G, 1024, 0, 0, 0, 0, 0, 0},   {12289, combo(1, 1, 0, 1, 0, 1), 0,   G, 1024, 0, 0, 0, 0, 0, 0},
    {6144,  combo(1, 1, 0, 1, 0, 1), 0,   R, 512, 12, 0, 0, 0, 0, 0},   {8192,  combo(1, 1, 0, 1, 0, 1), 0,   R, 1024, 8, 0, 0, 0, 0, 0},
    {8193,  combo(1, 1, 0, 1, 0, 1), 0,   R, 512, 20, 0, 0, 0, 0, 0},   {10000, combo(0, 1, 0, 1, 0, 1), 0,   R, 512, 20, 0, 0, 0, 0, 0},
    {10240, combo(1, 1, 0, 1, 0, 1), 0,   R, 512, 20, 0, 0, 0, 0, 0},   {10241, combo(1, 1, 0, 1, 0, 1), 0,   R, 512, 24, 0, 0, 0, 0, 0},
    {12288, combo(1, 1, 0, 1, 0, 1), 0,   R, 512, 24, 0, 0, 0, 0, 0},   {10000, combo(1, 1, 768, 0, 0, 1), 0, R, 1024, 10, 0, 0, 0, 0, 0},
    // DC_FWD_VARIANT=global: 256 threads up to 1 536 vertices, 512 up to 6 144, else 1024
    {1,     combo(1, 1, 0, GL, 0, 1), 0,  G, 256, 0, 0, 0, 0, 0, 0},    {1536,  combo(0, 1, 0, GL, 0, 1), 0,  G, 256, 0, 0, 0, 0, 0, 0},
    {1537,  combo(1, 1, 0, GL, 0, 1), 0,  G, 512, 0, 0, 0, 0, 0, 0},    {6144,  combo(1, 1, 0, GL, 0, 1), 0,  G, 512, 0, 0, 0, 0, 0, 0},
    {6145,  combo(1, 1, 0, GL, 0, 1), 0,  G, 1024, 0, 0, 0, 0, 0, 0},   {10000, combo(1, 1, 0, GL, 1, 1), 0,  G, 1024, 0, 0, 0, 0, 0, 0},
    // a deflation space: the deflated instances from 4 rows per thread on 512 threads; below, and on 768 threads, the plain ones
    {513,   combo(1, 1, 0, U, 1, 1), 0,   P, 512, 2, 0, 0, 0, 1, 1},    {1536,  combo(1, 1, 0, U, 1, 1), 0,   P, 512, 3, 0, 0, 0, 0, 1},
    {1537,  combo(1, 1, 0, U, 1, 1), 0,   D, 512, 4, 0, 0, 0, 0, 1},    {2049,  combo(1, 1, 0, U, 1, 1), 0,   D, 512, 6, 0, 0, 0, 0, 1},
    {4096,  combo(1, 1, 0, U, 1, 1), 0,   D, 512, 8, 0, 0, 0, 0, 1},    {4097,  combo(1, 1, 0, U, 1, 1), 0,   D, 512, 10, 0, 0, 0, 0, 1},
    {6144,  combo(1, 1, 0, U, 1, 1), 0,   D, 512, 12, 0, 0, 0, 0, 1},   {6145,  combo(1, 1, 0, U, 1, 1), 0,   D, 512, 16, 2, 0, 0, 0, 1},
    {10000, combo(1, 1, 0, U, 1, 1), 0,   D, 512, 20, 12, 1, 1, 0, 1},  {10000, combo(1, 0, 0, U, 1, 1), 0,   D, 512, 20, 6, 0, 0, 0, 1},
    {10000, combo(1, 1, 768, U, 1, 1), 0, P, 768, 14, 7, 1, 1, 0, 1},   {10000, combo(0, 1, 0, U, 1, 1), 0,   P, 512, 20, 6, 0, 0, 0, 1},      // (no windows: no space is wanted)
    {10241, combo(1, 1, 0, U, 1, 1), 0,   R, 1024, 12, 0, 0, 0, 0, 0},  {12289, combo(1, 1, 0, U, 1, 1), 0,   G, 1024, 0, 0, 0, 0, 0, 0},
    // the explicit inverse absent (DC_DENSE_MAX_N=0), and beyond its 768 vertices
    {512,   combo(1, 1, 0, U, 0, 0), 0,   P, 512, 1, 0, 0, 0, 0, 1},    {513,   combo(1, 1, 0, U, 0, 0), 0,   P, 512, 2, 0, 0, 0, 0, 1},
    {1536,  combo(1, 1, 0, U, 0, 0), 0,   P, 512, 3, 0, 0, 0, 0, 1},    {513,   combo(1, 1, 0, 0, 0, 0), 0,   R, 256, 4, 0, 0, 0, 0, 0},
    // matrix bandwidth 511: packet tables; 512: none, the resident kernel (windows off: whether they build on this numbering is not the point)
    {10000, combo(0, 1, 0, U, 0, 1), 508, P, 512, 20, 6, 0, 0, 0, 1},   {10000, combo(0, 1, 0, U, 0, 1), 509, R, 1024, 10, 0, 0, 0, 0, 0},
    {2049,  combo(0, 1, 0, U, 0, 1), 508, P, 512, 6, 0, 0, 0, 0, 1},    {2049,  combo(0, 1, 0, U, 0, 1), 509, R, 512, 8, 0, 0, 0, 0, 0},
    {10000, combo(0, 1, 0, 1, 0, 1), 509, R, 512, 20, 0, 0, 0, 0, 0},   {12289, combo(0, 1, 0, U, 0, 1), 509, G, 1024, 0, 0, 0, 0, 0, 0},
};

static void check_choice(const FwdChoice &c, const Pin &p, const std::string &what) {
  const bool same = (int) c.family == p.family && c.threads == p.threads && c.vpt == p.vpt && c.xl == p.xl && c.h16 == (p.h16 != 0) && c.ofs == (p.ofs != 0) &&
                    c.dense == (p.dense != 0) && c.fusable == (p.fusable != 0);
  if (!same)
    fail(what + ": family " + std::to_string(c.family) + " " + std::to_string(c.threads) + " x " + std::to_string(c.vpt) + " xl " + std::to_string(c.xl) + " h16 " +
         std::to_string(c.h16) + " ofs " + std::to_string(c.ofs) + " dense " + std::to_string(c.dense) + " fusable " + std::to_string(c.fusable) + ", expected family " +
         std::to_string(p.family) + " " + std::to_string(p.threads) + " x " + std::to_string(p.vpt) + " xl " + std::to_string(p.xl) + " h16 " + std::to_string(p.h16) + " ofs " +
         std::to_string(p.ofs) + " dense " + std::to_string(p.dense) + " fusable " + std::to_string(p.fusable));
}

// the adjoint's conditions as launch_adjoint_step / launch_adj / launch_adj_b stated them: {threads, WIN, DENSE, BLK, COARSE}
struct AdjWant { int threads; bool win, dense, blk, coarse; };
static AdjWant adjoint_before(bool dense_inv, bool win_ok, bool adj_coarse, bool defl_u, int win_lds_bytes, int mode, bool block_pre, int forced) {
  const int threads = (forced == 256 || forced == 512 || forced == 1024) ? forced : 1024;      // pick_threads_bwd
  // launch_adj<1024, true>: BLK only when !DENSE; launch_adj_b drops WIN, DENSE and BLK together without windows (here win_ok holds)
  if (dense_inv && win_ok && mode == 0 && threads == 1024) return {1024, true, true, false, false};
  if (adj_coarse && defl_u && win_ok && win_lds_bytes / 4 >= kCoarseLdsFloats && block_pre && mode == 1 && threads == 1024) return {1024, true, false, true, true};
  if (!win_ok) return {threads, false, false, false, false};
  return {threads, true, false, block_pre && mode == 1, false};
}

int main() {
  // ---- the tables themselves, by hand ----
  {
    static const int pk[11][6] = {{768, 14, 3, 7, 0, 0}, {512, 1, 0, -1, 1, 0}, {512, 2, 0, -1, 1, 0}, {512, 3, 0, -1, 1, 0}, {512, 4, 0, -1, 0, 1}, {512, 6, 0, -1, 0, 1},
                                  {512, 8, 0, -1, 0, 1}, {512, 10, 0, -1, 0, 1}, {512, 12, 0, -1, 0, 1}, {512, 16, 2, -1, 0, 1}, {512, 20, 6, 12, 0, 1}};
    if (kPkShapeCount != 11) fail("kPkShapes: eleven shapes");
    for (int i = 0; i < 11; i++) {
      const PkShape &s = kPkShapes[i];
      if (s.threads != pk[i][0] || s.vpt != pk[i][1] || s.xl != pk[i][2] || s.xl_h16 != pk[i][3] || s.dense != (pk[i][4] != 0) || s.defl != (pk[i][5] != 0))
        fail("kPkShapes[" + std::to_string(i) + "]");
      if (s.min_n != (i == 0 ? 9217 : 0)) fail("kPkShapes: 768 x 14 from 9 217 rows on, the 512-thread shapes form the default ladder");
      if (s.dense != (s.vpt <= 3) || s.defl != (s.threads == 512 && s.vpt >= 4)) fail("kPkShapes: DENSE where rows <= 3, DEFL where 512 threads and rows >= 4");
      // the LDS of either form fits a workgroup (dc_launchplan.h)
      if (pk_lds_bytes(s.threads, s.vpt, s.xl, false, false, 0, false, 0, false) > (size_t) kLdsLimitBytes) fail("kPkShapes: fp32 planes beyond the LDS");
      if (s.xl_h16 >= 0 && pk_lds_bytes(s.threads, s.vpt, s.xl_h16, true, false, 0, false, 0, false) > (size_t) kLdsLimitBytes) fail("kPkShapes: halves beyond the LDS");
    }
    static const int cl[7] = {1, 2, 3, 4, 6, 8, 12};
    if (kClRowsCount != 7 || kClThreads != 512) fail("kClRows: seven values, 512 threads");
    for (int i = 0; i < 7; i++) if (kClRows[i] != cl[i]) fail("kClRows[" + std::to_string(i) + "]");
    if (cl_rows_for(1) != 1 || cl_rows_for(512) != 1 || cl_rows_for(513) != 2 || cl_rows_for(2049) != 6 || cl_rows_for(4097) != 12 || cl_rows_for(6144) != 12 || cl_rows_for(6145) != 0)
      fail("cl_rows_for");
    if (kResCount != 10 || kGlobalCount != 3 || kAdjShapeCount != 5) fail("ladder lengths");
    std::printf("ok instance tables\n");
  }

  // ---- 1. pinned forward answers, on the decisions of real tables (N < 3: no mesh has so few vertices, the shape rule alone) ----
  int win_lds_bytes_10000 = 0;
  {
    int built = 0;
    for (const Pin &p : kPins) {
      PlanFacts f;
      if (p.N >= 3) {
        HostSystem H;
        if (!strip(H, p.N, p.far)) fail("strip mesh of " + std::to_string(p.N) + " vertices");
        int bw = 0;
        for (int r = 0; r < H.N; r++)
          for (int k = H.P_ptr[r]; k < H.P_ptr[r + 1]; k++) bw = std::max(bw, std::abs(H.P_col[k] - r));
        if (bw != (p.far == 0 ? 3 : p.far + 3)) fail("strip mesh: bandwidth " + std::to_string(bw));
        f = table_facts(H, p.q);
        if (p.q.win && !f.win_ok) fail("strip mesh of " + std::to_string(p.N) + " vertices: no element windows");
        if (p.N == 10000 && f.win_ok) win_lds_bytes_10000 = f.win_lds_bytes;
        // the shape rule describes the same decisions
        if (!same_facts(f, rule_facts(p.N, p.q, bw, true, f.win_lds_bytes))) fail(tag(p.N, p.q, bw) + ": the shape rule and HostTables::build disagree");
        built++;
      } else f = rule_facts(p.N, p.q, 3, true, 4096);
      check_choice(forward_choice(f, kernel_switches_of(p.q)), p, tag(p.N, p.q, p.far ? p.far + 3 : 3));
    }
    std::printf("ok %d pinned forward choices, %d of them on built tables\n", (int) (sizeof(kPins) / sizeof(kPins[0])), built);
  }

  // ---- 1b. the adjoint, every combination ----
  {
    int n = 0;
    for (int m = 0; m < 64; m++)
      for (int wl : {4 * kCoarseLdsFloats - 4, 4 * kCoarseLdsFloats, 100000})
        for (int forced : {0, 256, 512, 1024, 768}) {
          PlanFacts f;
          f.N = 3000;
          f.win_ok = m & 1; f.dense_inv = m & 2; f.adj_coarse = m & 4; f.defl_space = m & 8;
          const int mode = (m >> 4) & 1;
          const bool block_pre = (m >> 5) & 1;
          f.win_lds_bytes = wl;
          const AdjChoice c = adjoint_choice(f, mode, block_pre, forced);
          const AdjWant w = adjoint_before(f.dense_inv, f.win_ok, f.adj_coarse, f.defl_space, wl, mode, block_pre, forced);
          if (c.threads != w.threads || c.win != w.win || c.dense != w.dense || c.blk != w.blk || c.coarse != w.coarse)
            fail("adjoint choice: combination " + std::to_string(m) + " windows' LDS " + std::to_string(wl) + " DC_BWD_THREADS " + std::to_string(forced) + ": " +
                 std::to_string(c.threads) + " win " + std::to_string(c.win) + " dense " + std::to_string(c.dense) + " blk " + std::to_string(c.blk) + " coarse " + std::to_string(c.coarse));
          // it names an entry of the table; no windows => no BLK, DENSE, COARSE
          bool found = false;
          for (const AdjShape &s : kAdjShapes) found = found || (s.threads == c.threads && s.dense == c.dense && s.coarse == c.coarse);
          if (!found || (!c.win && (c.blk || c.dense || c.coarse)) || (c.dense && c.blk)) fail("adjoint choice: no such instance");
          const ClAdjChoice a = cl_adjoint_choice(f, block_pre);
          if (a.blk != block_pre || a.coarse != (block_pre && f.adj_coarse && f.defl_space)) fail("split adjoint choice");
          n++;
        }
    // by hand: the headline (windows, mode 1, no block preconditioner) and the garments (block preconditioner; with the coarse level)
    PlanFacts f;
    f.N = 10000; f.win_ok = true; f.win_lds_bytes = 150000;
    AdjChoice c = adjoint_choice(f, 1, false, 0);
    if (c.threads != 1024 || !c.win || c.dense || c.blk || c.coarse) fail("adjoint choice: headline");
    c = adjoint_choice(f, 1, true, 0);
    if (c.threads != 1024 || !c.win || c.dense || !c.blk || c.coarse) fail("adjoint choice: block preconditioner");
    f.adj_coarse = f.defl_space = true;
    c = adjoint_choice(f, 1, true, 0);
    if (c.threads != 1024 || !c.win || c.dense || !c.blk || !c.coarse) fail("adjoint choice: coarse level");
    c = adjoint_choice(f, 1, true, 512);
    if (c.threads != 512 || !c.win || c.dense || !c.blk || c.coarse) fail("adjoint choice: coarse level needs 1024 threads");
    f.win_ok = false;
    c = adjoint_choice(f, 1, true, 0);
    if (c.threads != 1024 || c.win || c.dense || c.blk || c.coarse) fail("adjoint choice: no windows, no BLK");
    std::printf("ok %d adjoint choices\n", n);
  }

  // ---- 2. closure: every N, every switch combination; the choice names a compiled instance ----
  {
    long long n = 0, fused = 0;
    for (int N = 1; N <= 13000; N++)
      for (int m = 0; m < 128; m++)
        for (int thr : {0, 512, 768})
          for (int variant : {U, 0, 1, GL})
            {
              Combo q;
              q.win = m & 1; q.h16 = (m >> 1) & 1; q.defl = (m >> 2) & 1; q.inv = (m >> 3) & 1; q.ofs = (m >> 4) & 1; q.pk_threads = thr; q.variant = variant;
              const int bw = (m & 32) ? 512 : 511;
              const PlanFacts f = rule_facts(N, q, bw, !(m & 64), win_lds_bytes_10000);
              const FwdChoice c = forward_choice(f, kernel_switches_of(q));
              const std::string t = tag(N, q, bw);
              const bool packet = c.family == kFwdPacket || c.family == kFwdPacketDeflated;
              bool found = false;
              if (packet) {
                for (const PkShape &s : kPkShapes)
                  found = found || (s.threads == c.threads && s.vpt == c.vpt && c.xl == (c.h16 ? s.xl_h16 : s.xl) && (!c.h16 || s.xl_h16 >= 0) && (!c.dense || s.dense) &&
                                    (c.family != kFwdPacketDeflated || s.defl));
                if (c.threads * c.vpt < N || c.threads != f.pk_threads || c.vpt != f.pk_vpt) fail(t + ": the packet instance is not the one the tables are padded for");
                if (c.dense && (c.h16 || c.family == kFwdPacketDeflated)) fail(t + ": explicit inverse with halves or deflation");
              } else if (c.family == kFwdResident) {
                for (const ResShape &s : kResLadder) found = found || (c.threads == s.threads && c.vpt == s.vpt) || (c.threads == s.alt_threads && c.vpt == s.alt_vpt);
                if (c.threads * c.vpt < N) fail(t + ": the resident shape does not hold the mesh");
              } else if (c.family == kFwdGlobal) {
                for (const GlobalShape &s : kGlobalLadder) found = found || c.threads == s.threads;
              }
              if (!found) fail(t + ": the choice names no instance");
              if (c.fusable != packet) fail(t + ": fusable <=> a packet family");
              // the plan's pk_ofs <=> the instance that runs reads byte offsets (a forced family leaves the tables as they are)
              const bool reads_ofs = packet && c.h16 && c.ofs;
              if (variant == U ? f.pk_ofs != reads_ofs : reads_ofs) fail(t + ": pk_ofs <=> the instance reads byte offsets");
              if (packet && c.ofs != f.pk_ofs) fail(t + ": the choice's offsets are the plan's");
              // fwd_defl => the chosen packet instance is a deflated one
              if (packet && f.fwd_defl && c.family != kFwdPacketDeflated) fail(t + ": fwd_defl without a deflated instance");
              if (c.family == kFwdPacketDeflated && !(f.fwd_defl && f.defl_space)) fail(t + ": a deflated instance without a space");
              n++; fused += c.fusable;
            }
    if (fused == 0 || fused == n) fail("closure: both fusable and non-fusable choices must occur");
    // decisions no instance fits give kFwdNone, never another family
    PlanFacts f;
    f.N = 5000; f.pk_ok = true; f.pk_threads = 512; f.pk_vpt = 10; f.win_ok = true; f.pk_ofs = true;
    if (forward_choice(f, KernelSwitches()).family != kFwdNone) fail("offsets for a shape without a halves instance must name no instance");
    f.pk_ofs = false; f.pk_vpt = 14;
    if (forward_choice(f, KernelSwitches()).family != kFwdNone) fail("512 x 14 is no instance");
    f.pk_threads = 768; f.fwd_defl = f.defl_space = true;
    if (forward_choice(f, KernelSwitches()).family != kFwdNone) fail("768 x 14 has no deflated instance");
    std::printf("ok closure over %lld choices, %lld of them fusable\n", n, fused);
  }

  // ---- 3. the split: every plan fit accepts names rows per thread of the table, with an instance for SX on / off and deflation ----
  {
    int accepted = 0;
    const struct { int nx, ny; } grids[] = {{48, 48}, {100, 100}, {100, 125}};
    for (const auto &g : grids) {
      HostSystem H;
      int bw = 0;
      if (!grid(H, g.nx, g.ny, &bw)) fail("grid");
      for (int K = 2; K <= 8; K++)
        for (int forced = 0; forced < 2; forced++) {
          ClusterPlan plan;
          if (!plan.fit(H, bw, K, forced != 0)) continue;
          accepted++;
          if (plan.pk_vpt != cl_rows_for(plan.R) || plan.pk_vpt * kClThreads < plan.R) fail("split plan: rows per thread");
          for (int m = 0; m < 4; m++) {
            PlanFacts f;
            f.N = H.N; f.defl_space = f.fwd_defl = m & 1;
            KernelSwitches sw;
            sw.sxcg = m & 2;
            const ClFwdChoice c = cl_forward_choice(f, plan.pk_vpt, sw);
            if (!c.ok || c.vpt != plan.pk_vpt || c.defl != ((m & 1) != 0) || c.sx != ((m & 2) && !(m & 1))) fail("split forward choice");
          }
        }
    }
    if (accepted == 0) fail("split: nothing was accepted");
    if (cl_forward_choice(PlanFacts(), 5, KernelSwitches()).ok || cl_forward_choice(PlanFacts(), 0, KernelSwitches()).ok) fail("split forward choice: 5 and 0 rows are no instance");
    std::printf("ok split: %d accepted plans\n", accepted);
  }
  std::printf("ALL OK\n");
  return 0;
}
