// Test harness (CPU): the host-side plan of the split execution (csrc/dc_clusterplan.cpp) — which K a batch gets, what the per-K search
// accepts and refuses, how many rollouts a launch carries — on triangulated grids, against answers that were NOT produced by that file:
//   [hand]    worked out from the rules for meshes small enough to do so: the figures are in the comments;
//   [parent]  written down from the engine's choose_cluster / build_cluster as they stood before this file existed (compiled unchanged
//             against a stand-in context), for the larger grids.
//   g++ -O2 -std=c++17 -pthread -I diffcloth_amd/csrc tests/native/cluster_plan_check.cpp diffcloth_amd/csrc/dc_clusterplan.cpp
//       diffcloth_amd/csrc/dc_system.cpp diffcloth_amd/csrc/dc_windows.cpp diffcloth_amd/csrc/dc_packets.cpp -o cluster_plan_check
// Prints one line per check and exits non-zero on the first failure (driven by tests/test_host_native.py).
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <thread>
#include <vector>
#include "dc_clusterplan.h"

using namespace dc;

static void fail(const std::string &what) { std::printf("FAIL %s\n", what.c_str()); std::exit(1); }

// triangulated nx x ny grid in row-major numbering (the grid of host_tables_check.cpp): the bandwidth of P is 2 nx + 1
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
    if (bandwidth != 2 * nx + 1) fail("grid bandwidth");
  }
};

struct Case {      // the inputs of ClusterPlan::build besides the mesh
  int B = 4, cus = 256;
  bool host_only = false, pk_ok = true, win_ok = true, dense_inv = false;
  ClusterSwitches sw;
};
static ClusterPlan plan_of(const Mesh &M, const Case &c) {
  ClusterPlan P;
  P.build(M.H, M.bandwidth, c.B, c.cus, c.host_only, c.pk_ok, c.win_ok, c.dense_inv, c.sw);
  return P;
}

// 3. the shape every accepted plan has
static void check_shape(const ClusterPlan &P, int N, const std::string &tag) {
  if (P.K < 2 || P.K > 8) fail(tag + ": K out of 2 .. 8");
  if (P.R % 64 || P.HB % 64 || P.HB < 64 || P.HB > P.R) fail(tag + ": R / HB are multiples of 64 with 64 <= HB <= R");
  if (!((long long) (P.K - 1) * P.R < N && N <= (long long) P.K * P.R)) fail(tag + ": (K - 1) R < N <= K R");
  if (P.pk_vpt * 512 < P.R || P.pk_vpt > 12) fail(tag + ": pk_vpt x 512 >= R, pk_vpt <= 12");
  if (P.xch_stride != cplan::kXchWaves + 2 * P.HB) fail(tag + ": xch_stride");
  if (!P.pk.ok || (int) P.pk.sq_dinv.size() != P.K * P.R || (int) P.pk.pk_ptr.size() != P.K * P.R / 64) fail(tag + ": packet tables are built for K R rows");
  if (!P.win.ok || P.wpp < 1 || P.win.own * P.wpp != P.R || P.win.nwin != (N + P.win.own - 1) / P.win.own) fail(tag + ": windows of R / wpp owned vertices");
  if (P.nb < 1 || P.xch_bytes != (size_t) P.nb * P.K * 2 * P.xch_stride * 16) fail(tag + ": exchange area");
}

struct Want { int ok, K, R, HB, wpp, vpt, nb; };
static void expect(const ClusterPlan &P, int N, const Want &w, const std::string &tag) {
  if (P.ok != (w.ok != 0) || P.K != w.K) fail(tag + ": ok / K = " + std::to_string(P.ok) + " / " + std::to_string(P.K) + ", expected " + std::to_string(w.ok) + " / " + std::to_string(w.K));
  if (!P.ok) { std::printf("ok %s: no split\n", tag.c_str()); return; }
  check_shape(P, N, tag);
  if (P.R != w.R || P.HB != w.HB || P.wpp != w.wpp || P.pk_vpt != w.vpt || P.nb != w.nb)
    fail(tag + ": (R, HB, wpp, vpt, nb) = (" + std::to_string(P.R) + ", " + std::to_string(P.HB) + ", " + std::to_string(P.wpp) + ", " + std::to_string(P.pk_vpt) + ", " +
         std::to_string(P.nb) + ")");
  std::printf("ok %s: K=%d R=%d HB=%d wpp=%d vpt=%d nb=%d\n", tag.c_str(), P.K, P.R, P.HB, P.wpp, P.pk_vpt, P.nb);
}
static const Want kNoSplit = {0, 1, 0, 0, 0, 0, 0};

// the per-K search alone; w.nb is not compared (fit does not size the launch)
static void expect_fit(const Mesh &M, int bandwidth, int K, bool forced, const Want &w, const std::string &tag) {
  ClusterPlan P;
  const bool got = P.fit(M.H, bandwidth, K, forced);
  if (got != (w.ok != 0)) fail(tag + (got ? ": accepted" : ": refused"));
  if (!got) { std::printf("ok %s: refused\n", tag.c_str()); return; }
  if (P.K != K || P.R != w.R || P.HB != w.HB || P.wpp != w.wpp || P.pk_vpt != w.vpt)
    fail(tag + ": (R, HB, wpp, vpt) = (" + std::to_string(P.R) + ", " + std::to_string(P.HB) + ", " + std::to_string(P.wpp) + ", " + std::to_string(P.pk_vpt) + ")");
  std::printf("ok %s: R=%d HB=%d wpp=%d vpt=%d\n", tag.c_str(), P.R, P.HB, P.wpp, P.pk_vpt);
}

// 1. residency, for every B: with the launch padded to a multiple of 8 rollouts and the parts of a rollout on one XCD, ceil(nb / 8) K
// workgroups share the cus / 8 CUs of an XCD; the launches cover the batch; balance: no launch more than one rollout smaller than another
static void check_residency(const Mesh &M, int cus, bool pk_ok, bool balance, const char *name) {
  std::atomic<int> split{0}, chunked{0};
  auto stripe = [&](int first, int stride) {
    for (int B = first; B <= 300; B += stride) {
      Case c; c.B = B; c.cus = cus; c.pk_ok = pk_ok;
      const ClusterPlan P = plan_of(M, c);
      if (!P.ok) { if (P.K != 1) fail("no split must report K = 1"); continue; }
      const std::string tag = std::string(name) + " cus=" + std::to_string(cus) + " B=" + std::to_string(B);
      check_shape(P, M.H.N, tag);
      const int launches = (B + P.nb - 1) / P.nb, last = B - (launches - 1) * P.nb;
      if ((P.nb + 7) / 8 * P.K > cus / 8) fail(tag + ": " + std::to_string((P.nb + 7) / 8 * P.K) + " workgroups on an XCD of " + std::to_string(cus / 8) + " CUs");
      if (P.nb * launches < B || last < 1) fail(tag + ": the launches do not cover the batch");
      if (balance && last < P.nb - 1) fail(tag + ": a launch of " + std::to_string(last) + " rollouts next to launches of " + std::to_string(P.nb));
      split++; chunked += launches > 1;
    }
  };
  // the 300 plans are independent (each builds its own tables): eight stripes of batch sizes, one thread each
  std::vector<std::thread> pool;
  for (int t = 0; t < 8; t++) pool.emplace_back(stripe, 1 + t, 8);
  for (std::thread &t : pool) t.join();
  std::printf("ok residency %s cus=%d%s: %d of 300 batch sizes split, %d of them in several launches\n", name, cus, pk_ok ? "" : " (no packet tables: kmin 2)", split.load(), chunked.load());
  if (split == 0) fail("residency: nothing was split");
}

int main() {
  const Mesh G100(100, 100), G48(48, 48);

  // ---- the documented anchors (docs/HISTORY.md): cus = 256, 100 x 100 [parent, and DESIGN's own figures] ----
  {
    const struct { int B; Want w; } anchors[] = {{32, {1, 8, 1280, 256, 1, 3, 32}}, {64, {1, 4, 2560, 256, 2, 6, 64}}, {128, {1, 2, 5120, 256, 4, 12, 128}}, {256, kNoSplit},
                                                 {33, {1, 6, 1792, 256, 2, 4, 33}}, {40, {1, 6, 1792, 256, 2, 4, 40}}, {200, kNoSplit}};
    for (const auto &a : anchors) { Case c; c.B = a.B; expect(plan_of(G100, c), 10000, a.w, "100x100 B=" + std::to_string(a.B)); }
    // [parent] 48 x 48 (N = 2304, bandwidth 97 -> HB 128): K = 7 leaves part 6 empty (R = 384, 6 x 384 = 2304), so B = 33 .. 40 get 6
    const struct { int B; Want w; } small[] = {{1, {1, 8, 320, 128, 1, 1, 1}}, {8, {1, 8, 320, 128, 1, 1, 8}}, {32, {1, 8, 320, 128, 1, 1, 32}}, {33, {1, 6, 384, 128, 1, 1, 33}},
                                               {40, {1, 6, 384, 128, 1, 1, 40}}, {64, {1, 4, 576, 128, 1, 2, 64}}, {200, kNoSplit}};
    for (const auto &a : small) { Case c; c.B = a.B; expect(plan_of(G48, c), 2304, a.w, "48x48 B=" + std::to_string(a.B)); }
  }

  // ---- 1. residency: a condition, for every batch size ----
  for (int cus : {256, 304, 64}) { check_residency(G48, cus, true, true, "48x48"); check_residency(G100, cus, true, true, "100x100"); }
  // a mesh without packet tables must be split whatever B is: the batch then runs in several launches (equal chunks; their balance is
  // not part of the residency rule and is not asserted here)
  check_residency(G48, 256, false, false, "48x48");

  // ---- 2. every rejection of the per-K search, on the smallest grid that triggers it ----
  {
    // [hand] 16 x 20: N = 320, bandwidth 33 -> HB = 64. Rows of a part at w = 1: round64(ceil(320 / K)) = 192, 128, 128, 64, 64, 64, 64 for K = 2 .. 8.
    const Mesh G(16, 20);
    // a part would be empty: (K - 1) R >= N — K = 4: 3 x 128 = 384; K = 6, 7, 8: 5 x 64 = 320, 384, 448
    for (int K : {4, 6, 7, 8}) expect_fit(G, G.bandwidth, K, true, kNoSplit, "16x20 forced K=" + std::to_string(K) + " (a part would be empty)");
    // R < 256 is refused unless forced; the same mesh forced: R = 192 / 128 / 64 for K = 2 / 3 / 5 (4 x 64 = 256 < 320), one row per thread
    for (int K : {2, 3, 5}) expect_fit(G, G.bandwidth, K, false, kNoSplit, "16x20 K=" + std::to_string(K) + " (R < 256, not forced)");
    expect_fit(G, G.bandwidth, 2, true, {1, 2, 192, 64, 1, 1, 0}, "16x20 forced K=2");
    expect_fit(G, G.bandwidth, 3, true, {1, 3, 128, 64, 1, 1, 0}, "16x20 forced K=3");
    expect_fit(G, G.bandwidth, 5, true, {1, 5, 64, 64, 1, 1, 0}, "16x20 forced K=5");
    // K < 2 is no split
    expect_fit(G, G.bandwidth, 1, true, kNoSplit, "16x20 K=1");
    // bandwidth 0 (no system) and > 511 (the packet format's column deltas) are refused whatever the mesh; 511 is not
    expect_fit(G, 0, 2, true, kNoSplit, "16x20 bandwidth 0");
    expect_fit(G, 512, 2, true, kNoSplit, "16x20 bandwidth 512");
    // [hand] 40 x 8: N = 320 again, bandwidth 81 -> HB = 128. K = 5: R = 64, 4 x 64 = 256 < 320 (no part empty) but R < HB: the halo would come
    // from beyond the direct neighbour. K = 3: R = 128 = HB is accepted.
    const Mesh W(40, 8);
    expect_fit(W, W.bandwidth, 5, true, kNoSplit, "40x8 forced K=5 (R < HB)");
    expect_fit(W, W.bandwidth, 3, true, {1, 3, 128, 128, 1, 1, 0}, "40x8 forced K=3");
    // [hand] rows per thread beyond 12: 100 x 125, N = 12 500, K = 2 — a part has at least 6 250 rows > 12 x 512 however many windows it
    // is cut into. [parent] K = 3: R = 4352 in 4 windows, 12 rows per thread.
    const Mesh L(100, 125);
    expect_fit(L, L.bandwidth, 2, true, kNoSplit, "100x125 forced K=2 (more than 12 rows per thread)");
    expect_fit(L, L.bandwidth, 3, true, {1, 3, 4352, 256, 4, 12, 0}, "100x125 forced K=3");
    // [parent] bandwidth 511 -> HB = 512: wider halos cost LDS, the search goes to 3 windows per part
    expect_fit(G100, 511, 4, true, {1, 4, 2688, 512, 3, 6, 0}, "100x100 bandwidth:=511 K=4");
    // A window whose reach leaves the halo: HB >= the bandwidth of P, and the elements of a window couple only vertices that P couples, so
    // no mesh triggers this with its true bandwidth (none of the grids here does). An understated bandwidth does: 100 x 100 claimed to have
    // bandwidth 1 -> HB = 64 while the elements reach 101 rows back; K = 8 (R = 1280) passes every other rule, as the anchor above shows.
    for (int K : {2, 4, 8}) expect_fit(G100, 1, K, true, kNoSplit, "100x100 bandwidth:=1 K=" + std::to_string(K) + " (element reach leaves the halo)");
  }

  // ---- 4. the K walk and the early returns ----
  {
    const Mesh G(16, 20);
    Case c;
    // [hand] forced 8 on the mesh that fits 2, 3 and 5 only: 8, 7, 6 refused, ends at 5; capacity(256, 5) = 8 x (32 / 5) = 48 >= 4: one launch
    c.sw.forced = 8; expect(plan_of(G, c), 320, {1, 5, 64, 64, 1, 1, 4}, "16x20 DC_CLUSTER=8");
    c.sw.forced = 12; expect(plan_of(G, c), 320, {1, 5, 64, 64, 1, 1, 4}, "16x20 DC_CLUSTER=12 (K <= 8)");
    // [hand] not forced: every K down to 2 has R < 256
    c.sw.forced = -1; expect(plan_of(G, c), 320, kNoSplit, "16x20 not forced");
    // kmin > 1 (a mesh without the one-workgroup tables; kmin = 2 here): the walk ends at kmin, here without a fit. (That it does not go below kmin
    // cannot show in an answer: kmin > 2 needs N > 12 288, where K < kmin has more than 12 rows per thread anyway.)
    c.pk_ok = false; expect(plan_of(G, c), 320, kNoSplit, "16x20 not forced, no packet tables");
  }
  {
    Case c; c.B = 32;
    c.sw.forced = 0; expect(plan_of(G100, c), 10000, kNoSplit, "100x100 DC_CLUSTER=0");
    c.sw.forced = 1; expect(plan_of(G100, c), 10000, kNoSplit, "100x100 DC_CLUSTER=1");
    c.sw.forced = -1;
    c.dense_inv = true; expect(plan_of(G100, c), 10000, kNoSplit, "100x100 explicit inverse, not forced");
    c.sw.forced = 4; expect(plan_of(G100, c), 10000, {1, 4, 2560, 256, 2, 6, 32}, "100x100 explicit inverse, DC_CLUSTER=4");      // [parent]
    c = Case(); c.B = 32;
    c.host_only = true; expect(plan_of(G100, c), 10000, kNoSplit, "100x100 host-only");
    c.host_only = false; c.B = 0; expect(plan_of(G100, c), 10000, kNoSplit, "100x100 B=0");
    // [parent] kmin = 2, more rollouts than fit at once: the scoring branch (B = 100: capacity(256, 2) = 128 holds them; 129: K = 3, 80 per launch -> 65 + 64)
    c = Case(); c.pk_ok = false;
    const struct { int B; Want w; } scored[] = {{8, {1, 8, 1280, 256, 1, 3, 8}}, {100, {1, 2, 5120, 256, 4, 12, 100}}, {129, {1, 3, 3456, 256, 3, 8, 65}},
                                                {200, {1, 2, 5120, 256, 4, 12, 100}}, {300, {1, 3, 3456, 256, 3, 8, 75}}};
    for (const auto &a : scored) { c.B = a.B; expect(plan_of(G100, c), 10000, a.w, "100x100 no packet tables B=" + std::to_string(a.B)); }
    // [parent] kmin = 3 (N = 12 500 without the one-workgroup tables)
    const Mesh L(100, 125);
    c.win_ok = false;
    c.B = 4; expect(plan_of(L, c), 12500, {1, 8, 1664, 256, 2, 4, 4}, "100x125 no tables B=4");
    c.B = 300; expect(plan_of(L, c), 12500, {1, 3, 4352, 256, 4, 12, 75}, "100x125 no tables B=300");
  }
  {   // the switches that only travel through [hand: kSpinLimit = 200 000 000 ticks of 10 ns; 200 ms = 20 000 000]
    Case c; c.B = 32;
    ClusterPlan P = plan_of(G100, c);
    if (P.spin_limit != 200000000ll || cplan::kSpinLimit != 200000000ll || P.redundant_self != 1 || P.test_drop != 0 || P.test_skew != -1) fail("switch defaults");
    c.sw.spin_ms = -5; if (plan_of(G100, c).spin_limit != 200000000ll) fail("DC_TEST_SPIN_MS <= 0 leaves kSpinLimit");
    c.sw.spin_ms = 200; c.sw.redundant_self = false; c.sw.test_drop = true; c.sw.test_skew = 2;
    P = plan_of(G100, c);
    if (P.spin_limit != 20000000ll || P.redundant_self != 0 || P.test_drop != 1 || P.test_skew != 2) fail("switch values");
    if (P.K != 8 || P.nb != 32) fail("the test hooks must not change the plan");
    std::printf("ok switches\n");
  }
  // cluster_capacity [hand]: 8 x floor((cus / 8) / K), at least 1
  if (cluster_capacity(256, 8) != 32 || cluster_capacity(256, 7) != 32 || cluster_capacity(256, 6) != 40 || cluster_capacity(256, 3) != 80 || cluster_capacity(304, 8) != 32 ||
      cluster_capacity(304, 2) != 152 || cluster_capacity(64, 8) != 8 || cluster_capacity(64, 5) != 8 || cluster_capacity(32, 8) != 1 || cluster_capacity(256, 0) != 256)
    fail("cluster_capacity");
  std::printf("ALL OK\n");
  return 0;
}
