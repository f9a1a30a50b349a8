// Host-side plan of the split execution (dc_cluster.h: one rollout run by K workgroups): how many parts a batch of B rollouts gets on a
// device of `cus` compute units, the rows / halo / element windows / rows per thread of a part, how many rollouts one launch carries, and
// the window and packet tables of that split. A function of the HostSystem, its bandwidth, B, the CU count, three kernel-set decisions and
// the values of the development switches; no device is needed, tests/native/cluster_plan_check.cpp checks the residency rule and every
// rejection on the CPU. dc_engine.hip reads the switches (dc_alloc_batch), builds the plan and uploads it.
#pragma once
#include <cstddef>
#include <vector>
#include "dc_launchplan.h"
#include "dc_packets.h"
#include "dc_system.h"
#include "dc_windows.h"

namespace dc {

namespace cplan {      // the exchange's sizes (dc_launchplan.h) under the names this plan's check knows them by
using dc::kXchWaves;
using dc::kSpinLimit;
}  // namespace cplan

// values of the development switches dc_alloc_batch reads (defaults: nothing forced, no test hook)
struct ClusterSwitches {
  int forced = -1;              // DC_CLUSTER=k: k parts (0 / 1 = no split); < 0 = choose
  bool redundant_self = true;   // DC_SELF_REDUNDANT=0: the layered self friction on part 0 alone
  int spin_ms = 0;              // DC_TEST_SPIN_MS: > 0 = bound of every spin in ms instead of kSpinLimit
  bool test_drop = false;       // DC_TEST_DROP_PART
  int test_skew = -1;           // DC_TEST_SKEW_PART
};

// Rollouts one launch of the split kernels can hold with EVERY workgroup resident (the exchange spins on its peers: a part that is not
// scheduled until another rollout has finished its whole sweep would let them run into the spin limit). A launch is padded to a
// multiple of 8 rollouts and the parts of rollout j all run on XCD j mod 8 (cluster_map, dc_cluster.h), so what bounds it is one XCD:
// ceil(nb / 8) * K workgroups on cus / 8 CUs, one workgroup (160 KB of LDS, up to 1024 threads) per CU.
int cluster_capacity(int cus, int K);

struct ClusterPlan {
  bool ok = false;              // false: one workgroup per rollout (K = 1, nothing else is set)
  int K = 1;                    // parts per rollout
  int R = 0, HB = 0;            // rows per part, boundary rows exchanged each side (multiples of 64, HB <= R)
  int wpp = 0, pk_vpt = 0;      // element windows per part, rows per thread of the 512-thread forward kernel
  int xch_stride = 0;           // granules per (part, parity)
  int nb = 0;                   // rollouts per launch: all B when they fit, else equal chunks
  size_t xch_bytes = 0;         // exchange area of one launch
  long long spin_limit = kSpinLimit;
  int redundant_self = 1, test_drop = 0, test_skew = -1;
  HostWindows win;              // windows of R / wpp owned vertices
  HostPackets pk;               // packet matrix padded to K R rows

  // K for this batch: enough parts to give every CU a workgroup (B rollouts x K <= CUs, K <= 8), at least as many as a mesh too large
  // for the one-workgroup kernel needs (pk_ok / win_ok: that kernel has its tables), none for a mesh with the explicit inverse (dense_inv)
  // unless forced; then K downwards until the mesh fits.
  void build(const HostSystem &H, int bandwidth, int B, int cus, bool host_only, bool pk_ok, bool win_ok, bool dense_inv, const ClusterSwitches &sw);
  // (R, wpp, pk_vpt) and the tables for K parts per rollout; false when K does not fit this mesh. `forced`: parts of fewer than 256 rows are accepted.
  bool fit(const HostSystem &H, int bandwidth, int K, bool forced);
};

}  // namespace dc
