#include "dc_clusterplan.h"
#include <algorithm>
#include "dc_tables.h"

namespace dc {

int cluster_capacity(int cus, int K) { return std::max(1, 8 * ((cus / 8) / std::max(K, 1))); }

bool ClusterPlan::fit(const HostSystem &H, int bandwidth, int Kc, bool forced) {
  const int N = H.N;
  if (Kc < 2 || bandwidth <= 0 || bandwidth > 511) return false;
  const int HBc = std::max(64, round64(bandwidth));
  HostWindows HW;
  int Rf = 0, w_f = 0, vpt = 0;
  for (int w = 1; w <= 8 && Rf == 0; w++) {
    const int own_w = round64((N + Kc * w - 1) / (Kc * w));
    const int Rc = own_w * w;
    if ((long long) (Kc - 1) * Rc >= N) break;          // a part would be empty
    if (Rc < HBc) break;                                 // halo rows must come from the direct neighbours only
    if (Rc < 256 && !forced) break;                      // parts of fewer rows than half a workgroup: nothing left to save (the 1426-vertex
                                                         // T-shirt, one rollout: 21.9 / 19.0 / 18.4 / 18.2 ms per fwd+bwd step at K = 1 / 4 / 6 / 8
                                                         // once its parts share an XCD, tools/bench_tshirt_k.py)
    const int v = cl_rows_for(Rc);                       // (dc_kernelplan.h: the instances of the split kernels)
    if (v == 0) continue;                                // more rows per part than the kernel holds in registers: more windows do not help
    if (!HW.build_own(H, own_w)) continue;
    const int win_floats = (int) (HW.lds_bytes / 4);
    // both split kernels' dynamic LDS, whichever instance the launchers choose, within the workgroup's limit (dc_launchplan.h)
    if (!cl_bound_fits(cl_forward_floats_bound(v, Rc, HBc, win_floats)) || !cl_bound_fits(cl_adjoint_floats_bound(HBc, win_floats))) continue;
    // the element reach of every window must stay inside the boundary rows its part receives
    bool reach_ok = true;
    for (int q = 0; q < HW.nwin; q++) {
      const int part = q / w, p0 = part * Rc;
      const int lo = HW.win[8 * q + 2], vs = HW.win[8 * q + 3];
      if (lo < p0 - HBc || lo + vs > p0 + Rc + HBc) reach_ok = false;
    }
    if (!reach_ok) continue;
    Rf = Rc; w_f = w; vpt = v;
  }
  if (Rf == 0) return false;
  HostPackets HP;
  if (!HP.build_rows(H, Kc * Rf)) return false;
  K = Kc; R = Rf; HB = HBc; wpp = w_f; pk_vpt = vpt; xch_stride = kXchWaves + 2 * HBc;
  win = std::move(HW); pk = std::move(HP);
  return true;
}

void ClusterPlan::build(const HostSystem &H, int bandwidth, int B, int cus, bool host_only, bool pk_ok, bool win_ok, bool dense_inv, const ClusterSwitches &sw) {
  *this = ClusterPlan();
  if (host_only || B <= 0) return;
  const int forced = sw.forced;
  if (forced == 0 || forced == 1) return;
  if (dense_inv && forced < 2) return;     // small meshes: the explicit-inverse kernels are the faster ones
  // Fewer rollouts than CUs: as many parts as fit (B K <= CUs), up to 8 — a rollout's speed-up grows with K (measured on C4: 1.3 /
  // 1.9 / 3.0 x at K = 2 / 4 / 8). A mesh too large for one workgroup needs kmin parts; when that oversubscribes the device the
  // batch runs in several launches and K is the one that wastes the least: score = fraction of the CUs busy x per-CU efficiency.
  // per-CU efficiency of K parts against one workgroup per rollout, re-measured in round 6 on the C4 workload (bench.py --total-batch 128 / 64 / 32
  // against 256: 6 032 / 5 031 / 4 003 against 9 880 rollout-steps/s -> 0.61 / 0.51 / 0.405 at K = 2 / 4 / 8; K = 3, 5, 6, 7 interpolated)
  static const double eff[9] = {0, 1.0, 0.61, 0.56, 0.51, 0.48, 0.45, 0.43, 0.405};
  const int kmin = (!pk_ok || !win_ok) ? std::max(2, std::min(8, (H.N + 6143) / 6144)) : 1;
  int Kc = 1;
  if (forced >= 2) Kc = std::min(forced, 8);
  else if (B <= cluster_capacity(cus, std::max(kmin, 2))) { Kc = std::max(kmin, 2); while (Kc + 1 <= 8 && B <= cluster_capacity(cus, Kc + 1)) Kc++; }
  else if (kmin > 1) {
    double best = -1;
    for (int k = kmin; k <= 8; k++) {
      const int nbmax = cluster_capacity(cus, k), nchunks = (B + nbmax - 1) / nbmax, nbk = (B + nchunks - 1) / nchunks;
      const double score = (double) nbk * k / cus * eff[k];
      if (score > best + 1e-9) { best = score; Kc = k; }
    }
  }
  for (; Kc >= 2; Kc--) {
    ok = fit(H, bandwidth, Kc, forced >= 2);
    if (ok) break;
    if (forced < 2 && Kc <= kmin) break;
  }
  if (!ok) return;
  {   // rollouts per launch: all of them when they fit, else equal chunks (never a last launch with a handful of rollouts)
    const int nbmax = cluster_capacity(cus, K), nchunks = (B + nbmax - 1) / nbmax;
    nb = std::max(1, (B + nchunks - 1) / nchunks);
  }
  xch_bytes = (size_t) nb * K * 2 * xch_stride * kGranuleBytes;
  redundant_self = sw.redundant_self; test_drop = sw.test_drop; test_skew = sw.test_skew;
  if (sw.spin_ms > 0) spin_limit = (long long) sw.spin_ms * 100000ll;      // test hook
}

}  // namespace dc
