// Device helpers the two direct adjoint solves share (dc_adjoint_dense.hip, adjoint_mode 2; dc_adjoint_band.hip, adjoint_mode 3): the
// record's Adj64 without LDS, the accessor that probes the element pass on unit vectors, and the pivot search's merge rule.
#pragma once
#include "dc_devlib.h"
#include "dc_adjoint64.h"

namespace dc {
namespace {

// Adj64 of rollout b for record A (as k_adjoint_step sets it up; no LDS: the layered self pass takes its global-memory path)
__device__ __forceinline__ Adj64 dense_adj64(const DevSystem &S, const BwdArgs &A, int b) {
  const int N = S.N;
  const size_t off = (size_t) b * 3 * N;
  Adj64 C;
  C.xnew = A.x_new + off; C.rec_f = A.rec_f + off; C.rec_n = A.rec_n + off;
  C.mu = A.mu + (size_t) b * S.ngroups;
  C.pvel = A.pvel ? A.pvel + (size_t) b * kPvRow * S.ngroups : nullptr;      // obstacle velocities of the record's step (null: none set)
  C.d_pvel = A.d_pvel ? A.d_pvel + (size_t) b * kPvRow * S.ngroups : nullptr;
  C.xprev = A.x_prev + off; C.vnew = A.v_new + off;
  C.rec_prim = A.rec_prim + (size_t) b * N;
  C.self = A.self; C.b = b;
  C.nself = (S.contact_enabled && S.self_enabled) ? A.self.meta[(size_t) b * kMetaStride] : 0;
  C.lds = nullptr; C.lds_floats = 0;
  adj64_inject(C, A, b, N, S.self_cap);
  return C;
}

// One accessor type for the three vectors element_pass64 touches (it takes them as one template type): x_new (plain loads), a unit
// vector y = e_u, and a corner sink that keeps the three components of corner `k` only.
struct ProbeV {
  int kind;                  // 0 = plain, 1 = unit vector, 2 = corner sink
  const double *p;
  int u, k, NC;
  d3 *o;
  __device__ __forceinline__ double ld(int idx) const { return kind == 0 ? p[idx] : (idx == u ? 1.0 : 0.0); }
  __device__ __forceinline__ void st(int idx, double v) const {
    if (idx == k) o->x = v;
    else if (idx == NC + k) o->y = v;
    else if (idx == 2 * NC + k) o->z = v;
  }
};

// (value, row) maximum with ties to the lower row
__device__ __forceinline__ void amax_merge(double &v, int &r, double v2, int r2) {
  if (v2 > v || (v2 == v && r2 < r)) { v = v2; r = r2; }
}

}  // namespace
}  // namespace dc
