// Contact read-out (dc_get_contact_readout / dc_get_contact_readout_dev): what the obstacles feel, formed on the device from the tape.
//
// One workgroup per (slot, rollout) row, every row of the range in ONE launch; lanes stride over the vertices in device numbering. A vertex
// with prim = PRIM[slot][b][i] >= 0 re-forms the argument of the friction law exactly as the step that wrote the record did — d = prim_d(prim, n, f,
// m_i, motion row of this slot and rollout), n and f from the fp32 record — and evaluates
//   state = contact_state(n, d, mu)   (1 take-off, 2 stick, 3 slide; 0 = not in primitive contact)
//   r_p   = dry_friction(n, d, mu)    the PRIMITIVE part of the record's r, whatever the self-contact layers added to the stored r afterwards
//   jn    = r_p . n                   normal impulse (>= 0)
// with mu = mu[b][group] the context's current value, as the backward step reads it. Per group g one row of kWrenchRow values:
//   J = -sum r_p,  tau = -sum (x_i - c_g) x r_p,  sum jn,  the numbers of take-off / stick / slide contacts
// x_i from X[slot], c_g the centre of the group's FIRST flattened primitive in PC[slot]. Sums run in fp64 in a fixed order (lane-strided partial
// sums, wave shuffle tree, the waves' sums added in wave order — the scheme of k_dfv_scale) and are rounded once; no atomics: bit-reproducible.
// The kernel makes one pass over the row per group when the sums are asked for (a vertex is evaluated in the pass of its group; the other
// passes read its 4-byte primitive index only), one pass otherwise. Per-vertex outputs go out in the caller's numbering.
// Traffic model: f, n, x (12 B each), prim, mass (4 B each) = 44 B per vertex and slot, plus what is written.
#define DC_KERNEL_TU
#include "dc_devlib.h"

namespace dc {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

template <class T>
__global__ __launch_bounds__(kThreads) void k_contact_readout(const DevSystem *__restrict__ Sp, const float *__restrict__ X, const float *__restrict__ F,
                                                              const float *__restrict__ NRM, const int *__restrict__ PRIM, const float *__restrict__ PC,
                                                              const float *__restrict__ PV, const float *__restrict__ mu, int B, int *__restrict__ state,
                                                              T *__restrict__ jn_out, T *__restrict__ wrench) {
  __shared__ double part[kWaves][kWrenchRow];
  const DevSystem &S = *Sp;
  const int N = S.N, G = S.ngroups, P = S.nprim;
  const long row = blockIdx.x;
  const int b = (int) (row % B);
  const float *x = X + row * 3 * N, *f = F + row * 3 * N, *nr = NRM + row * 3 * N;
  const int *pr = PRIM + row * N;
  const float *cen = PC + row * 3 * P;
  const float *wv = PV ? PV + row * G * kPvRow : nullptr;
  const float *mub = mu + (long) b * G;
  const int DC_G *user_of = S.user_of;
  const int npass = wrench ? G : 1;
  for (int g = 0; g < npass; g++) {
    f3 c = mk(0, 0, 0);
    if (wrench) {
      int p0 = 0;
      while (p0 < P - 1 && S.prims[p0].group != g) p0++;
      c = mk(cen[3 * p0], cen[3 * p0 + 1], cen[3 * p0 + 2]);
    }
    double acc[kWrenchRow] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = threadIdx.x; i < N; i += kThreads) {
      const int prim = pr[i];
      const int grp = prim >= 0 ? S.prims[prim].group : -1;
      const long o = row * N + (user_of ? user_of[i] : i);
      if (prim < 0 || (wrench && grp != g)) {
        if (prim < 0 && g == 0) {
          if (state) state[o] = 0;
          if (jn_out) jn_out[o] = (T) 0;
        }
        continue;
      }
      const f3 n = ld3(nr, i, N);
      const f3 d = prim_d(S.prims[prim], n, ld3(f, i, N), S.mass[i], wv);
      const float m = mub[grp];
      const int st = contact_state(n, d, m);
      const f3 r = dry_friction(n, d, m);
      const double jn = (double) r.x * (double) n.x + (double) r.y * (double) n.y + (double) r.z * (double) n.z;
      if (state) state[o] = st;
      if (jn_out) jn_out[o] = (T) jn;
      if (wrench) {
        const f3 xi = ld3(x, i, N);
        const double ax = (double) xi.x - (double) c.x, ay = (double) xi.y - (double) c.y, az = (double) xi.z - (double) c.z;
        const double rx = r.x, ry = r.y, rz = r.z;
        acc[0] -= rx; acc[1] -= ry; acc[2] -= rz;
        acc[3] -= ay * rz - az * ry; acc[4] -= az * rx - ax * rz; acc[5] -= ax * ry - ay * rx;
        acc[6] += jn;
        acc[7] += st == 1; acc[8] += st == 2; acc[9] += st == 3;
      }
    }
    if (!wrench) break;
#pragma unroll
    for (int k = 0; k < kWrenchRow; k++) {
      double v = acc[k];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
      if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < kWrenchRow) {
      double s = 0;
      for (int w = 0; w < kWaves; w++) s += part[w][threadIdx.x];
      wrench[(row * G + g) * kWrenchRow + threadIdx.x] = (T) s;
    }
    __syncthreads();
  }
}

}  // namespace

void launch_contact_readout(const DevSystem &S, const float *X, const float *F, const float *NRM, const int *PRIM, const float *PC, const float *PV,
                            const float *mu, long rows, int B, int *state, void *jn, void *wrench, int is_f32, hipStream_t st) {
  if (rows <= 0 || S.N <= 0) return;
  const dim3 g((unsigned) rows), b(kThreads);
  if (is_f32) hipLaunchKernelGGL(k_contact_readout<float>, g, b, 0, st, S.self_dev, X, F, NRM, PRIM, PC, PV, mu, B, state, (float *) jn, (float *) wrench);
  else hipLaunchKernelGGL(k_contact_readout<double>, g, b, 0, st, S.self_dev, X, F, NRM, PRIM, PC, PV, mu, B, state, (double *) jn, (double *) wrench);
}

}  // namespace dc
