// Test harness (CPU): the fp64 rows of flat-rest bending as the fp64 adjoint operator applies them (dc_adjoint64.h: apply_K64 with S.win_rows)
// against the per-flap fp64 pass they replace (element_pass64's flap loop, linear branch, summed over the corners of every vertex).
//   g++ -O1 -std=c++17 -I diffcloth_amd/csrc tests/native/bend_rows64_check.cpp diffcloth_amd/csrc/{dc_system,dc_windows,dc_packets,dc_dense,dc_tables}.cpp -o bend_rows64_check
// For the 12 x 9 grid (two windows of 64 vertices) and the 100 x 100 grid (the headline's mesh, the windows dc_build chooses) and a random fp64
// vector y of three components per vertex:  sum_k brow_val[k] (y_col[k] - y_i), k ascending as on the device, equals
// sum over the flaps e of i and its corner c there of  w_c h^2 w2_e sum_{c' = 1..3} w_c' (y_c' - y_0)  to 1e-13 of the sum of the terms' magnitudes.
// Also: in HostSystem::inc_idx a vertex's triangle corners precede its flap corners (the device loop ends a vertex's corner sum at the first flap corner).
// The comparison is then seen to FAIL on a copy of the rows with one coefficient dropped. Prints one line per check and exits non-zero on the
// first failure (driven by tests/test_bend_rows64.py; also built with -fsanitize=address,undefined there).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>
#include "dc_system.h"
#include "dc_tables.h"
#include "dc_windows.h"

using namespace dc;

static void fail(const std::string &what) { std::printf("FAIL %s\n", what.c_str()); std::exit(1); }

static const double kH = 1.0 / 180;
static const double kTol = 1e-13;

// the vertex loop's rows term of apply_K64, on the host: planar y [3][N], the result planar [3][N], the terms' magnitudes per vertex
static void rows_apply(int N, const std::vector<int> &ptr, const std::vector<int> &col, const std::vector<double> &val, const std::vector<double> &y,
                       std::vector<double> &out, std::vector<double> &mag) {
  out.assign(3 * (size_t) N, 0.0); mag.assign(N, 0.0);
  for (int i = 0; i < N; i++) {
    double bx = 0, by = 0, bz = 0, m = 0;
    for (int k = ptr[i]; k < ptr[i + 1]; k++) {
      const int j = col[k];
      const double c = val[k];
      const double tx = (y[j] - y[i]) * c, ty = (y[N + j] - y[N + i]) * c, tz = (y[2 * N + j] - y[2 * N + i]) * c;
      bx += tx; by += ty; bz += tz;
      m += std::fabs(tx) + std::fabs(ty) + std::fabs(tz);
    }
    out[i] = bx; out[N + i] = by; out[2 * N + i] = bz; mag[i] = m;
  }
}

// the flap loop of element_pass64 (rest norm 0: res = ey) and the corner sums of apply_K64's vertex loop, in fp64
static void flaps_apply(const HostSystem &H, const std::vector<double> &y, std::vector<double> &out) {
  const int N = H.N, E = H.E;
  const double h2 = kH * kH;
  out.assign(3 * (size_t) N, 0.0);
  for (int e = 0; e < E; e++) {
    const int *q = &H.bend_v[4 * e];
    const double *w = &H.bend_w[4 * (size_t) e];
    for (int d = 0; d < 3; d++) {
      const double *yd = &y[(size_t) d * N];
      const double ey = (yd[q[1]] - yd[q[0]]) * w[1] + (yd[q[2]] - yd[q[0]]) * w[2] + (yd[q[3]] - yd[q[0]]) * w[3];
      const double res = ey * (h2 * H.bend_w2[e]);
      for (int c = 0; c < 4; c++) out[(size_t) d * N + q[c]] += res * w[c];
    }
  }
}

// worst |rows - flaps| over the vertices, relative to the sum of the vertex's terms' magnitudes (a vertex without terms must agree exactly)
static double worst_ratio(int N, const std::vector<double> &rows, const std::vector<double> &mag, const std::vector<double> &flaps) {
  double worst = 0;
  for (int i = 0; i < N; i++)
    for (int d = 0; d < 3; d++) {
      const double diff = std::fabs(rows[(size_t) d * N + i] - flaps[(size_t) d * N + i]);
      if (mag[i] > 0) worst = std::max(worst, diff / mag[i]);
      else if (diff != 0) worst = 1.0;
    }
  return worst;
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

static void check(int nx, int ny, int own, unsigned seed) {
  const std::string tag = "grid " + std::to_string(nx) + " x " + std::to_string(ny);
  std::vector<double> pos;
  std::vector<int> tri;
  grid(nx, ny, pos, tri);
  HostSystem H;
  if (!H.set_mesh(nx * ny, pos.data(), (int) tri.size() / 3, tri.data())) fail(tag + ": set_mesh");
  if (!H.build_numerics(kH, 0.3, 200.0, 0.02, 1e4)) fail(tag + ": build_numerics");
  HostWindows W;
  if (own > 0) W.build_own(H, own, true, kH); else W.build(H, kWindowLdsBudget, true, kH);
  const int N = H.N;
  if (!W.ok || !W.rows || (int) W.brow_ptr.size() != N + 1 || W.brow_ptr[N] != (int) W.brow_col.size() || W.brow_col.size() != W.brow_val.size())
    fail(tag + ": a flat grid must get the rows");
  for (int e = 0; e < H.E; e++) if ((float) H.bend_n[e] > 1e-6f) fail(tag + ": a flap outside the linear branch");
  // apply_K64 stops a vertex's corner sum at its first flap corner: in inc_idx every triangle corner (< 3 T) of a vertex must precede its flap corners
  for (int v = 0; v < N; v++) {
    bool flaps_began = false;
    for (int k = H.inc_ptr[v]; k < H.inc_ptr[v + 1]; k++) {
      if (H.inc_idx[k] >= 3 * H.T) flaps_began = true;
      else if (flaps_began) fail(tag + ": a triangle corner behind a flap corner in a vertex's incidence list");
    }
  }
  std::mt19937 rng(seed);
  std::uniform_real_distribution<double> u(-1, 1);
  std::vector<double> y(3 * (size_t) N), rows, mag, flaps;
  for (double &v : y) v = u(rng);
  flaps_apply(H, y, flaps);
  rows_apply(N, W.brow_ptr, W.brow_col, W.brow_val, y, rows, mag);
  const double worst = worst_ratio(N, rows, mag, flaps);
  if (!(worst <= kTol)) { std::printf("worst %.3e\n", worst); fail(tag + ": the fp64 rows differ from the per-flap fp64 pass"); }
  // one coefficient dropped (the middle entry of the middle vertex's row): the same comparison must fail
  std::vector<double> val = W.brow_val;
  const int vm = N / 2, km = (W.brow_ptr[vm] + W.brow_ptr[vm + 1]) / 2;
  if (W.brow_ptr[vm + 1] == W.brow_ptr[vm] || val[km] == 0.0) fail(tag + ": the dropped coefficient must exist");
  val[km] = 0.0;
  rows_apply(N, W.brow_ptr, W.brow_col, val, y, rows, mag);
  const double broken = worst_ratio(N, rows, mag, flaps);
  if (broken <= kTol) fail(tag + ": a dropped coefficient went unnoticed");
  std::printf("ok %s N=%d E=%d nwin=%d entries=%d worst |rows - flaps| / sum|terms| = %.2e (bound %.0e); one coefficient dropped: %.2e\n", tag.c_str(), N, H.E, W.nwin,
              W.brow_ptr[N], worst, kTol, broken);
}

int main() {
  check(12, 9, 64, 11);
  check(100, 100, 0, 12);
  std::printf("ALL OK\n");
  return 0;
}
