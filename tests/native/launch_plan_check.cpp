// Test harness (CPU): the host-side plan of the step kernels' dynamic LDS (csrc/dc_launchplan.h) — the byte counts the launchers ask for, the
// offsets they hand to the kernels, the limits they refuse at — against figures worked out by hand (the arithmetic is in the comments), and
// the planner's bounds against the launchers: a plan ClusterPlan::fit accepts is never refused by a non-deflated split launcher.
//   g++ -O2 -std=c++17 -Wall -I diffcloth_amd/csrc tests/native/launch_plan_check.cpp diffcloth_amd/csrc/dc_clusterplan.cpp
//       diffcloth_amd/csrc/dc_system.cpp diffcloth_amd/csrc/dc_windows.cpp diffcloth_amd/csrc/dc_packets.cpp -o launch_plan_check
// Prints one line per group of checks and exits non-zero on the first failure (driven by tests/test_host_native.py).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>
#include "dc_clusterplan.h"
#include "dc_launchplan.h"

using namespace dc;

static void fail(const std::string &what) { std::printf("FAIL %s\n", what.c_str()); std::exit(1); }
static void eq(long long got, long long want, const std::string &what) {
  if (got != want) fail(what + ": " + std::to_string(got) + ", expected " + std::to_string(want));
}

// triangulated nx x ny grid in row-major numbering (the grid of cluster_plan_check.cpp)
struct Mesh {
  HostSystem H;
  int bandwidth = 0;
  Mesh(int nx, int ny) {
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
    if (!H.set_mesh(nx * ny, pos.data(), (int) tri.size() / 3, tri.data()) || !H.build_numerics(1.0 / 120, 0.3, 200.0, 0.02, 1e4)) fail("mesh");
    for (int r = 0; r < H.N; r++)
      for (int k = H.P_ptr[r]; k < H.P_ptr[r + 1]; k++) bandwidth = std::max(bandwidth, std::abs(H.P_col[k] - r));
  }
};

int main() {
  // ---- the shared sizes: 160 KB - 256; detection 16 + 4097 + 4096 + 1 + 2048 ints; coarse 2 (16 x 48 + 48) floats ----
  eq(kLdsLimitBytes, 163840, "kLdsLimitBytes"); eq(kClusterLdsBytes, 163584, "kClusterLdsBytes");
  eq(kSelfDetectLdsInts, 10258, "kSelfDetectLdsInts"); eq(kCoarseLdsFloats, 1632, "kCoarseLdsFloats");
  eq(kXchWaves, 16, "kXchWaves"); eq(kXchLdsFloats, 32, "kXchLdsFloats"); eq(kGranuleBytes, 16, "kGranuleBytes");
  // dense_chunks = ceil(4 waves / (ld / 64)) clamped to 1 .. 8: ld 768 = 12 row groups, 8 waves: ceil(32 / 12) = 3; 16 waves: ceil(64 / 12) = 6;
  // ld 64, 16 waves: 64 -> 8; ld 2048 = 32 row groups, 4 waves: ceil(16 / 32) = 1. dense_lds_floats = 3 ld chunks
  eq(dense_chunks(768, 8), 3, "dense_chunks(768, 8)"); eq(dense_chunks(768, 16), 6, "dense_chunks(768, 16)");
  eq(dense_chunks(64, 16), 8, "dense_chunks(64, 16)"); eq(dense_chunks(2048, 4), 1, "dense_chunks(2048, 4)");
  eq(dense_lds_floats(768, 8), 6912, "dense_lds_floats(768, 8)");
  std::printf("ok shared sizes\n");

  // ---- pk_lds_bytes: threads x ((H16 ? 2 : 3) vpt + 3 xl) x 4 ----
  eq(pk_lds_bytes(512, 20, 12, true, false, 0, false, 0, false), 155648, "pk 512/20/12 H16");      // 512 x 76 x 4
  eq(pk_lds_bytes(512, 20, 6, false, false, 0, false, 0, false), 159744, "pk 512/20/6 fp32");      // 512 x 78 x 4
  eq(pk_lds_bytes(768, 14, 7, true, false, 0, false, 0, false), 150528, "pk 768/14/7 H16");        // 768 x 49 x 4
  eq(pk_lds_bytes(768, 14, 3, false, false, 0, false, 0, false), 156672, "pk 768/14/3 fp32");      // 768 x 51 x 4
  // widened by larger windows (only when the mesh has them), by the detection (10 258 ints = 41 032 bytes; 256/1/1 alone: 256 x 6 x 4 = 6 144)
  // and by the explicit inverse's partial sums behind the rows (512/3/3: 512 x 18 x 4 = 36 864, + 6 912 floats = 27 648 bytes)
  eq(pk_lds_bytes(512, 20, 12, true, false, 0, true, 156000, false), 156000, "pk widened by the windows");
  eq(pk_lds_bytes(512, 20, 12, true, false, 0, true, 100000, false), 155648, "pk with smaller windows");
  eq(pk_lds_bytes(512, 20, 12, true, false, 0, false, 156000, false), 155648, "pk without windows ignores their size");
  eq(pk_lds_bytes(256, 1, 1, false, false, 0, false, 0, true), 41032, "pk widened by the detection");
  eq(pk_lds_bytes(256, 1, 1, false, false, 0, false, 0, false), 6144, "pk 256/1/1");
  eq(pk_lds_bytes(512, 20, 12, true, false, 0, false, 0, true), 155648, "pk above the detection's need");
  eq(pk_lds_bytes(512, 3, 3, false, true, 768, false, 0, false), 64512, "pk with the explicit inverse");
  eq(pk_lds_bytes(512, 3, 3, false, false, 768, false, 0, false), 36864, "pk 512/3/3");
  eq(res_lds_bytes(512, 24), 147456, "res 512/24");      // 3 x 512 x 24 x 4
  eq(res_lds_bytes(256, 1), 3072, "res 256/1");
  std::printf("ok pk_lds_bytes / res_lds_bytes\n");

  // ---- cl_forward_lds(R = 1280, HB = 256): GL = 1792; pipe 2 GL + 6 HB = 5 120, else 3 GL = 5 376; detection 10 258 -> 10 260; (10 260 + 32) x 4 ----
  {
    ClForwardLds l = cl_forward_lds(1280, 256, 0, true, true, false);
    eq(l.fric_floats, 5120, "cl forward pipe+detect fric_floats"); eq(l.tail_off, 10260, "cl forward pipe+detect tail_off"); eq(l.bytes, 41168, "cl forward pipe+detect bytes");
    if (!l.ok) fail("cl forward pipe+detect refused");
    l = cl_forward_lds(1280, 256, 0, false, false, false);
    eq(l.fric_floats, 5376, "cl forward plain fric_floats"); eq(l.tail_off, 5376, "cl forward plain tail_off"); eq(l.bytes, 21632, "cl forward plain bytes");      // (5 376 + 32) x 4
    l = cl_forward_lds(1280, 256, 0, true, false, false);
    eq(l.fric_floats, 5120, "cl forward pipe fric_floats"); eq(l.tail_off, 5120, "cl forward pipe tail_off");
    l = cl_forward_lds(1280, 256, 24004, true, false, false);      // windows of 6 001 floats: offered to the friction pass as they are, the tail rounded up to 6 004
    eq(l.fric_floats, 6001, "cl forward windows fric_floats"); eq(l.tail_off, 6004, "cl forward windows tail_off"); eq(l.bytes, 24144, "cl forward windows bytes");
    // the limit: 163 584 bytes = (40 864 + 32) x 4, reached with windows of 163 456 bytes; one granule (16 bytes) more is refused.
    // The deflated instances stop 512 bytes earlier: 163 072 = (40 736 + 32) x 4, windows of 162 944 bytes.
    l = cl_forward_lds(256, 64, 163456, true, true, false);
    eq(l.bytes, 163584, "cl forward last fit bytes"); if (!l.ok) fail("cl forward: the last byte count that fits is refused");
    l = cl_forward_lds(256, 64, 163472, true, true, false);
    eq(l.bytes, 163600, "cl forward first refusal bytes"); if (l.ok) fail("cl forward: one granule above the limit is accepted");
    l = cl_forward_lds(256, 64, 162944, false, true, true);
    eq(l.bytes, 163072, "cl forward deflated last fit bytes"); if (!l.ok) fail("cl forward deflated: the last byte count that fits is refused");
    l = cl_forward_lds(256, 64, 162960, false, true, true);
    eq(l.bytes, 163088, "cl forward deflated first refusal bytes"); if (l.ok) fail("cl forward deflated: one granule above its limit is accepted");
    if (!cl_forward_lds(256, 64, 162960, false, true, false).ok) fail("cl forward: the deflated limit applied to a plain instance");
  }
  // ---- cl_adjoint_lds(HB = 256, windows of 100 004 bytes = 25 001 floats): hc_off 25 004, + 6 x 256 = 26 540, (26 540 + 32) x 4 ----
  {
    ClAdjointLds l = cl_adjoint_lds(256, 100004);
    eq(l.hc_off, 25004, "cl adjoint hc_off"); eq(l.tail_off, 26540, "cl adjoint tail_off"); eq(l.bytes, 106288, "cl adjoint bytes");
    if (!l.ok) fail("cl adjoint refused");
    // the limit with HB = 64: 40 864 - 384 = 40 480 floats of windows = 161 920 bytes
    l = cl_adjoint_lds(64, 161920);
    eq(l.bytes, 163584, "cl adjoint last fit bytes"); if (!l.ok) fail("cl adjoint: the last byte count that fits is refused");
    l = cl_adjoint_lds(64, 161936);
    eq(l.bytes, 163600, "cl adjoint first refusal bytes"); if (l.ok) fail("cl adjoint: one granule above the limit is accepted");
  }
  std::printf("ok cl_forward_lds / cl_adjoint_lds\n");

  // ---- adj_lds_bytes: the windows; the explicit inverse 3 ld + 3 ld chunks floats (ld 768, 16 waves: 2 304 + 13 824 = 16 128 floats = 64 512 bytes);
  // the coarse level 1 632 floats = 6 528 bytes; nothing without windows ----
  eq(adj_lds_bytes(1024, false, 100000, true, 768, true), 0, "adj without windows");
  eq(adj_lds_bytes(1024, true, 100000, false, 0, false), 100000, "adj windows");
  eq(adj_lds_bytes(1024, true, 50000, true, 768, false), 64512, "adj explicit inverse");
  eq(adj_lds_bytes(1024, true, 100000, true, 768, false), 100000, "adj explicit inverse under larger windows");
  eq(adj_lds_bytes(1024, true, 4000, false, 0, true), 6528, "adj coarse level");
  eq(adj_lds_bytes(1024, true, 8000, false, 0, true), 8000, "adj coarse level under larger windows");
  // ---- adj_ylist(1024, lds 140 000, limit 163 840, static 4 096): reserve 4 352, room 19 488 = 1 624 entries of 12 bytes; list starts at float 35 000 ----
  {
    AdjYlist y = adj_ylist(1024, 140000, 163840, 4096, 10000, 0);
    eq(y.ycap, 1624, "ylist ycap"); eq(y.ybase, 35000, "ylist ybase"); eq(y.bytes, 159488, "ylist bytes");      // 140 000 + 19 488
    y = adj_ylist(1024, 140000, 163840, 4096, 1000, 100);      // one entry per vertex and two per self contact bind: 1 200
    eq(y.ycap, 1200, "ylist capped ycap"); eq(y.ybase, 35000, "ylist capped ybase"); eq(y.bytes, 154400, "ylist capped bytes");
    y = adj_ylist(512, 140000, 163840, 4096, 10000, 0);
    eq(y.ycap, 0, "ylist 512 threads ycap"); eq(y.ybase, 35000, "ylist 512 threads ybase"); eq(y.bytes, 140000, "ylist 512 threads bytes");
    y = adj_ylist(1024, 159476, 163840, 4096, 10000, 0);       // 159 476 + 4 352 + 12 = 163 840: room for exactly one entry
    eq(y.ycap, 1, "ylist last room ycap"); eq(y.bytes, 159488, "ylist last room bytes");
    y = adj_ylist(1024, 159480, 163840, 4096, 10000, 0);       // 4 bytes more: lds + reserve + 12 > limit
    eq(y.ycap, 0, "ylist no room ycap"); eq(y.ybase, 39870, "ylist no room ybase"); eq(y.bytes, 159480, "ylist no room bytes");
    y = adj_ylist(1024, 163000, 163840, 4096, 10000, 0);       // (the windows alone beyond the limit less the reserve: no underflow)
    eq(y.ycap, 0, "ylist beyond ycap"); eq(y.bytes, 163000, "ylist beyond bytes");
  }
  std::printf("ok adj_lds_bytes / adj_ylist\n");

  // ---- the planner's bounds, by hand: 6 x 1 792 = 10 752 (> detection); 8 rows per thread: 3 x (3 456 + 512) = 11 904; small part: the detection;
  // adjoint 25 004 + 1 536; the cap 163 584 / 4 - 32 = 40 864 floats, 4 of them left for the rounding ----
  eq(cl_forward_floats_bound(3, 1280, 256, 0), 10752, "forward bound vpt 3"); eq(cl_forward_floats_bound(8, 3456, 256, 0), 11904, "forward bound vpt 8");
  eq(cl_forward_floats_bound(1, 320, 128, 0), 10258, "forward bound small part"); eq(cl_forward_floats_bound(3, 1280, 256, 30001), 30001, "forward bound windows");
  eq(cl_adjoint_floats_bound(256, 25001), 26540, "adjoint bound");
  if (!cl_bound_fits(40860) || cl_bound_fits(40861)) fail("cl_bound_fits: 40 860 + 4 <= 40 864 < 40 861 + 4");
  std::printf("ok bounds\n");

  // ---- the bounds are upper bounds: every shape fit can hand over (R, HB multiples of 64, 64 <= HB <= 512, HB <= R, the smallest allowed rows per
  // thread with vpt x 512 >= R) with windows of every size class, whichever instance the launchers choose ----
  {
    static const int allowed[] = {1, 2, 3, 4, 6, 8, 12};
    long long shapes = 0, fits = 0;
    for (int R = 64; R <= 6144; R += 64)
      for (int HB = 64; HB <= std::min(R, 512); HB += 64)
        for (int wf : {0, 1, 2, 3, 10257, 10259, 20001, 30002, 36000, 37783, 37784, 39321, 39324, 39325, 40859, 40860, 40861}) {
          int v = 0;
          for (int a : allowed) if (a * 512 >= R) { v = a; break; }
          shapes++;
          if (!cl_bound_fits(cl_forward_floats_bound(v, R, HB, wf)) || !cl_bound_fits(cl_adjoint_floats_bound(HB, wf))) continue;
          fits++;
          for (int pd = 0; pd < 4; pd++)
            if (!cl_forward_lds(R, HB, 4 * wf, pd & 1, pd & 2, false).ok)
              fail("a shape within the forward bound is refused: R " + std::to_string(R) + " HB " + std::to_string(HB) + " windows " + std::to_string(wf) + " floats");
          if (!cl_adjoint_lds(HB, 4 * wf).ok)
            fail("a shape within the adjoint bound is refused: R " + std::to_string(R) + " HB " + std::to_string(HB) + " windows " + std::to_string(wf) + " floats");
        }
    if (fits == 0 || fits == shapes) fail("the shape sweep must have both accepted and refused shapes");
    std::printf("ok bounds cover the launchers on %lld of %lld shapes within them\n", fits, shapes);
  }

  // ---- sweep: every plan ClusterPlan::fit accepts on the grids of cluster_plan_check.cpp is launched by every non-deflated instance ----
  {
    int accepted = 0, near_cap = 0;
    const struct { int nx, ny; } grids[] = {{48, 48}, {100, 100}, {100, 125}};
    for (const auto &g : grids) {
      const Mesh M(g.nx, g.ny);
      for (int K = 2; K <= 8; K++)
        for (int forced = 0; forced < 2; forced++) {
          ClusterPlan P;
          if (!P.fit(M.H, M.bandwidth, K, forced != 0)) continue;
          accepted++;
          const std::string tag = std::to_string(g.nx) + "x" + std::to_string(g.ny) + " K=" + std::to_string(K);
          const int win = (int) P.win.lds_bytes;
          size_t most = 0;
          for (int pd = 0; pd < 4; pd++) {
            const ClForwardLds l = cl_forward_lds(P.R, P.HB, win, pd & 1, pd & 2, false);
            if (!l.ok) fail(tag + ": accepted by fit, refused by the forward launcher (" + std::to_string(l.bytes) + " bytes)");
            most = std::max(most, l.bytes);
          }
          const ClAdjointLds a = cl_adjoint_lds(P.HB, win);
          if (!a.ok) fail(tag + ": accepted by fit, refused by the adjoint launcher (" + std::to_string(a.bytes) + " bytes)");
          near_cap += most > (size_t) (kClusterLdsBytes - kDeflReserveBytes);
        }
    }
    if (accepted == 0) fail("sweep: nothing was accepted");
    // (reported, not asserted: such a plan would be refused by the deflated forward instances, which keep 512 bytes more free)
    std::printf("ok sweep: %d accepted plans launch; %d of them within %d bytes of the cap\n", accepted, near_cap, kDeflReserveBytes);
  }
  std::printf("ALL OK\n");
  return 0;
}
