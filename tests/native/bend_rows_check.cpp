// Test harness (CPU): flat-rest bending as per-vertex matrix rows (dc_windows.h: HostWindows::rows) against the per-flap evaluation.
//   g++ -O1 -std=c++17 -I diffcloth_amd/csrc tests/native/bend_rows_check.cpp diffcloth_amd/csrc/{dc_system,dc_windows,dc_packets,dc_dense,dc_tables}.cpp -o bend_rows_check
//   bend_rows_check [mesh.bin ...]      mesh.bin = int32 N, int32 T, double pos[3 N], int32 tri[3 T]: meshes with curved flaps, rows must be refused
// Always checks a 12 x 9 flat grid (regular, and with its vertices moved inside the plane) in two windows of 64 vertices and the 100 x 100 grid (the headline's mesh) in the windows dc_build chooses:
// rows are built, no window carries a flap, every entry position lies in its window's span, window count / size / spans equal those without
// rows, and for random fp64 x the decoded fp32 rows give sum_j coef_ij (x_j - x_i) = the per-flap sum within the one rounding of each
// coefficient. A grid with one vertex lifted out of plane, and every mesh file given, must be refused and get the tables without rows byte for
// byte. Prints one line per check and exits non-zero on the first failure (driven by tests/test_bend_rows.py).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>
#include "dc_system.h"
#include "dc_tables.h"
#include "dc_windows.h"

using namespace dc;

static void fail(const std::string &what) { std::printf("FAIL %s\n", what.c_str()); std::exit(1); }
static float asfloat(int b) { float f; std::memcpy(&f, &b, 4); return f; }

static const double kH = 1.0 / 180;

static bool same_tables(const HostWindows &A, const HostWindows &B) {
  return A.ok == B.ok && A.own == B.own && A.nwin == B.nwin && A.vcap == B.vcap && A.nrcap == B.nrcap && A.lds_bytes == B.lds_bytes && A.win == B.win &&
         A.tri_rec == B.tri_rec && A.bend_rec == B.bend_rec && A.inc == B.inc && A.inc_ptr == B.inc_ptr && A.inc_n == B.inc_n &&
         A.tri_D.size() == B.tri_D.size() && A.bend_w.size() == B.bend_w.size() && A.tri_Dlo.size() == B.tri_Dlo.size() && A.bend_lo.size() == B.bend_lo.size() &&
         (A.tri_D.empty() || !std::memcmp(A.tri_D.data(), B.tri_D.data(), 4 * A.tri_D.size())) &&
         (A.bend_w.empty() || !std::memcmp(A.bend_w.data(), B.bend_w.data(), 4 * A.bend_w.size())) &&
         (A.tri_Dlo.empty() || !std::memcmp(A.tri_Dlo.data(), B.tri_Dlo.data(), 4 * A.tri_Dlo.size())) &&
         (A.bend_lo.empty() || !std::memcmp(A.bend_lo.data(), B.bend_lo.data(), 4 * A.bend_lo.size()));
}

// W: built with rows wanted, W0: the same call without
static void check_rows(const HostSystem &H, const HostWindows &W, const HostWindows &W0, int expect_min_windows, const std::string &tag) {
  const int N = H.N, E = H.E;
  if (!W.ok || !W0.ok) fail(tag + ": build refused");
  if (!W.rows || W0.rows) fail(tag + ": rows must be built for a mesh that is flat at rest, and only when asked for");
  if (W.nwin != W0.nwin || W.own != W0.own || W.vcap != W0.vcap || W.nwin < expect_min_windows) fail(tag + ": window count / size must be those of the build without rows");
  if (!W.bend_rec.empty() || !W.bend_w.empty() || !W.bend_lo.empty()) fail(tag + ": no flap records with rows");
  if (W.tri_rec != W0.tri_rec || W.inc_ptr != W0.inc_ptr || W.inc_n != W0.inc_n) fail(tag + ": triangle records and packet counts must not move");
  if (W.nrcap >= W0.nrcap || W.lds_bytes >= W0.lds_bytes || W.lds_bytes != 4 * ((size_t) 6 * W.vcap + (size_t) 3 * W.nrcap)) fail(tag + ": nrcap / lds_bytes must shrink by the flaps' result slots");
  if ((int) W.brow_ptr.size() != N + 1 || W.brow_col.size() != W.brow_val.size() || W.brow_ptr[N] != (int) W.brow_col.size()) fail(tag + ": CSR copy sizes");
  // per-flap evaluation in fp64: sum_flaps (corner weight) h^2 w^2 sum_c w_c (x_c - x_0)
  std::mt19937 rng(11);
  std::uniform_real_distribution<double> u(-1, 1);
  std::vector<double> x(N), want(N, 0.0);
  for (double &v : x) v = u(rng);
  for (int e = 0; e < E; e++) {
    const int *q = &H.bend_v[4 * e];
    const double *w = &H.bend_w[4 * (size_t) e];
    double ev = 0;
    for (int c = 1; c < 4; c++) ev += w[c] * (x[q[c]] - x[q[0]]);
    for (int c = 0; c < 4; c++) want[q[c]] += w[c] * kH * kH * H.bend_w2[e] * ev;
  }
  std::vector<int> owner(N, 0);
  size_t entries = 0;
  double worst = 0;
  for (int w = 0; w < W.nwin; w++) {
    const int *d = &W.win[8 * w], *d0 = &W0.win[8 * w];
    const int v0 = d[0], v1 = d[1], lo = d[2], vs = d[3], nt = d[5], nb = d[7];
    if (nb != 0) fail(tag + ": a window carries flaps");
    for (int k = 0; k < 6; k++) if (d[k] != d0[k]) fail(tag + ": owned range, span and triangles of a window must be those of the build without rows");
    if (2 * nt + 1 + kWinDumpSlots > W.nrcap || vs > W.vcap) fail(tag + ": descriptor beyond nrcap / vcap");
    for (int v = v0; v < v1; v++) {
      owner[v]++;
      const int ch = v / 64, l = v % 64, nt4 = W.inc_n[ch] >> 16, nb4 = W.inc_n[ch] & 0xffff;
      for (int pk = 0; pk < nt4; pk++)           // triangle packets: untouched, and their padding points at the zero vector behind the triangles' results
        for (int k = 0; k < 4; k++) {
          const int word = W.inc[4 * ((size_t) W.inc_ptr[ch] + (size_t) pk * 64 + l) + k];
          for (int hh = 0; hh < 2; hh++) if ((((unsigned) word >> (16 * hh)) & 0xffff) >> 1 > (unsigned) (2 * nt)) fail(tag + ": triangle entry beyond the window's result vectors");
        }
      double s = 0, mag = 0;
      int k = W.brow_ptr[v], last = -1;
      bool padding = false;
      for (int pk = 0; pk < nb4; pk++) {
        const int *q = &W.inc[4 * ((size_t) W.inc_ptr[ch] + (size_t) (nt4 + pk) * 64 + l)];
        for (int hh = 0; hh < 2; hh++) {
          const int pos = q[2 * hh];
          const float coef = asfloat(q[2 * hh + 1]);
          if (pos < 0 || pos >= vs) fail(tag + ": entry position outside the window's span");
          const int j = lo + pos;
          if (j == v) {       // padding: the vertex's own slot, coefficient +0 — and nothing but padding behind it
            if (q[2 * hh + 1] != 0) fail(tag + ": a padding entry (the vertex's own slot) must have coefficient 0");
            padding = true;
            continue;
          }
          if (padding) fail(tag + ": entries behind the first padding entry must be padding");
          if (j <= last) fail(tag + ": a row's entries must be ordered by column");
          last = j;
          if (k >= W.brow_ptr[v + 1] || W.brow_col[k] != j || (float) W.brow_val[k] != coef) fail(tag + ": packet entry differs from the CSR copy (column, fl32 of the value)");
          k++; entries++;
          const double t = (double) coef * (x[j] - x[v]);
          s += t; mag += std::fabs(t);
        }
      }
      if (k != W.brow_ptr[v + 1]) fail(tag + ": a CSR entry is missing from the packets");
      // one rounding of each coefficient (2^-24 relative) + the fp64 roundings of two orders of summation
      const double bound = std::ldexp(mag, -24) + 1e-15 * mag;
      if (!(std::fabs(s - want[v]) <= bound)) {
        std::printf("vertex %d: rows %.17g flaps %.17g bound %.3g\n", v, s, want[v], bound);
        fail(tag + ": row sum differs from the per-flap evaluation");
      }
      if (mag > 0) worst = std::max(worst, std::fabs(s - want[v]) / mag);
    }
  }
  for (int v = 0; v < N; v++) if (owner[v] != 1) fail(tag + ": every vertex must be owned by exactly one window");
  std::printf("ok %s N=%d E=%d nwin=%d own=%d off-diagonals=%zu (%.2f per row) nrcap %d -> %d lds %zu -> %zu worst |rows - flaps| / sum|terms| = %.2e (2^-24 = 6.0e-8)\n", tag.c_str(), N, E, W.nwin,
              W.own, entries, (double) entries / N, W0.nrcap, W.nrcap, W0.lds_bytes, W.lds_bytes, worst);
}

static void check_refused(const HostSystem &H, const std::string &tag) {
  bool curved = false;
  for (int e = 0; e < H.E; e++) curved = curved || (float) H.bend_n[e] > 1e-6f;
  if (!curved) fail(tag + ": the mesh of a refusal case must have a flap with rest norm above 1e-6");
  HostWindows A, B;
  if (!A.build(H, kWindowLdsBudget, true, kH) || !B.build(H, kWindowLdsBudget)) fail(tag + ": build refused");
  if (A.rows || !A.brow_ptr.empty() || !A.brow_col.empty() || !A.brow_val.empty()) fail(tag + ": rows must be refused when any flap is curved at rest");
  if (!same_tables(A, B)) fail(tag + ": a refused mesh must get the tables without rows byte for byte");
  HostWindows C, D;
  if (!C.build_own(H, 64, true, kH) || !D.build_own(H, 64) || C.rows || !same_tables(C, D)) fail(tag + ": the same for a given window size");
  dc_params prm;
  std::memset(&prm, 0, sizeof(prm));
  prm.time_step = kH;
  TableSwitches sw;
  HostTables P, Q;
  P.build(H, prm, sw);
  sw.bend_rows = false;
  Q.build(H, prm, sw);
  if (P.bend_rows || Q.bend_rows || P.win_ok != Q.win_ok || (P.win_ok && !same_tables(P.win, Q.win))) fail(tag + ": the plan of a refused mesh must not depend on the switch");
  std::printf("ok refused %s N=%d E=%d nwin=%d\n", tag.c_str(), H.N, H.E, A.nwin);
}

static void grid(int nx, int ny, std::vector<double> &pos, std::vector<int> &tri) {
  pos.assign(3 * (size_t) nx * ny, 0.0);
  for (int a = 0; a < ny; a++)
    for (int b = 0; b < nx; b++) { pos[3 * (a * nx + b)] = 0.05 * b; pos[3 * (a * nx + b) + 1] = 0.05 * a; }
  tri.clear();
  for (int a = 0; a + 1 < ny; a++)
    for (int b = 0; b + 1 < nx; b++) {
      const int v00 = a * nx + b, v01 = v00 + 1, v10 = v00 + nx, v11 = v10 + 1;
      tri.insert(tri.end(), {v00, v01, v11});
      tri.insert(tri.end(), {v00, v11, v10});
    }
}

static void build(HostSystem &H, int N, const std::vector<double> &pos, const std::vector<int> &tri, const std::string &tag) {
  if (!H.set_mesh(N, pos.data(), (int) tri.size() / 3, tri.data())) fail(tag + ": set_mesh");
  if (!H.build_numerics(kH, 0.3, 200.0, 0.02, 1e4)) fail(tag + ": build_numerics");
}

int main(int argc, char **argv) {
  std::vector<double> pos;
  std::vector<int> tri;
  {
    grid(12, 9, pos, tri);
    HostSystem H;
    build(H, 12 * 9, pos, tri, "grid 12 x 9");
    HostWindows W, W0;
    W.build_own(H, 64, true, kH); W0.build_own(H, 64);
    check_rows(H, W, W0, 2, "grid 12 x 9, windows of 64");
    HostWindows Wd;
    Wd.build_own(H, 64, false, kH);
    if (Wd.rows || !same_tables(Wd, W0)) fail("grid 12 x 9: without the request the tables must be today's");
    {   // the same grid with its vertices moved inside the plane: still flat, but no two cotan weights of a flap are equal any more (on the
        // regular grid a flap's two opposite vertices carry the same weight, and exchanging them goes unnoticed)
      std::vector<double> pj = pos;
      std::mt19937 rng(5);
      std::uniform_real_distribution<double> u(-0.015, 0.015);
      for (int v = 0; v < 12 * 9; v++) { pj[3 * v] += u(rng); pj[3 * v + 1] += u(rng); }
      HostSystem Hj;
      build(Hj, 12 * 9, pj, tri, "grid 12 x 9, jittered in plane");
      HostWindows Wj, Wj0;
      Wj.build_own(Hj, 64, true, kH); Wj0.build_own(Hj, 64);
      check_rows(Hj, Wj, Wj0, 2, "grid 12 x 9 jittered in plane, windows of 64");
    }
    // one vertex lifted out of plane: its flaps are curved at rest
    pos[3 * (4 * 12 + 5) + 2] = 0.01;
    HostSystem Hc;
    build(Hc, 12 * 9, pos, tri, "grid 12 x 9, one vertex lifted");
    check_refused(Hc, "grid 12 x 9, one vertex lifted");
  }
  {
    grid(100, 100, pos, tri);
    HostSystem H;
    build(H, 100 * 100, pos, tri, "grid 100 x 100");
    HostWindows W, W0;
    W.build(H, kWindowLdsBudget, true, kH); W0.build(H, kWindowLdsBudget);
    check_rows(H, W, W0, 2, "grid 100 x 100");
    // the plan's decision and its switch
    dc_params prm;
    std::memset(&prm, 0, sizeof(prm));
    prm.time_step = kH;
    TableSwitches sw;
    HostTables T;
    T.build(H, prm, sw);
    if (!T.win_ok || !T.bend_rows || !T.win.rows || !same_tables(T.win, W) || T.win.brow_val != W.brow_val) fail("plan: the 10 000-vertex grid must get the rows, built with the parameters' time step");
    sw.bend_rows = false;
    T.build(H, prm, sw);
    if (T.bend_rows || T.win.rows || !same_tables(T.win, W0)) fail("plan: DC_BEND_ROWS=0 must keep the per-flap tables");
    pos[3 * (50 * 100 + 50) + 2] = 0.01;
    HostSystem Hc;
    build(Hc, 100 * 100, pos, tri, "grid 100 x 100, one vertex lifted");
    check_refused(Hc, "grid 100 x 100, one vertex lifted");
    std::printf("ok plan decisions\n");
  }
  for (int a = 1; a < argc; a++) {
    FILE *f = std::fopen(argv[a], "rb");
    int hdr[2];
    if (!f || std::fread(hdr, 4, 2, f) != 2) fail(std::string(argv[a]) + ": cannot read");
    const int N = hdr[0], T = hdr[1];
    pos.resize(3 * (size_t) N); tri.resize(3 * (size_t) T);
    if (std::fread(pos.data(), 8, pos.size(), f) != pos.size() || std::fread(tri.data(), 4, tri.size(), f) != tri.size()) fail(std::string(argv[a]) + ": short file");
    std::fclose(f);
    if (mesh_bandwidth(T, tri.data()) > 511) {        // as dc_build: reverse Cuthill-McKee
      const std::vector<int> order = rcm_order(N, T, tri.data());
      std::vector<int> inv(N);
      for (int k = 0; k < N; k++) inv[order[k]] = k;
      std::vector<double> p2(pos.size());
      for (int k = 0; k < N; k++) for (int d = 0; d < 3; d++) p2[3 * (size_t) k + d] = pos[3 * (size_t) order[k] + d];
      for (int &v : tri) v = inv[v];
      pos.swap(p2);
    }
    HostSystem H;
    build(H, N, pos, tri, argv[a]);
    check_refused(H, "mesh " + std::to_string(a));
  }
  std::printf("ALL OK\n");
  return 0;
}
