// Adjoint of the contact read-out (dc_set_contact_readout_gradients): turns dL/d(read-out) of the records a backward sweep passes through into
// adjoint seeds and gradient terms, without touching the adjoint step kernels. All fp64 arithmetic on the fp32 record.
//
// For a vertex i in contact with a primitive of group g in the step that produced record s, with the incoming weights J^, tau^, S^ (the wrench row
// of g: entries 0..2, 3..5, 6) and jn^_i,
//   phi_i = dPhi/dr_p,i = -J^ - tau^ x (x_i - c_g) + (jn^_i + S^) n_i          (c_g, n_i constant, as everywhere in the adjoint)
//   q_i   = (dr_p,i/dd_i)^T phi_i                                               (the friction case of the read-out; 0 at every other vertex)
// r_p depends on f alone, before the self-contact layers, so q enters after the layers as a shift of y = (I + dr_df)^T u: the backward step
// through record s is the plain step with
//   1. g   += -(1/h) h^2 (A - dp/dx)^T A q - r_p,i x tau^       (loss gradient w.r.t. x at slot s: the fp64 element operator of dc_adjoint64.h
//                                                                 at the same x_new, no contact part, no mass term)
//   2. dL/dv_n += m_i q_i                                        (loss gradient w.r.t. v at slot s - 1)
//   3. y~ = y + q / h wherever finish_gradients64 reads y: the force gradients, dL_dxfixed, the dL/dk sums, the w = y - u term of dL_ddensity
//   4. u_i + phi_i / h wherever u_i multiplies a primitive-contact derivative: dL/dmu, dL/dw, dL/domega
// Everything is linear in q, and q does not depend on u. Two launches of one kernel, one workgroup per rollout, the slots of the sweep walked
// serially (the rollout's fp64 work vectors are per rollout):
//   SEED (before the step kernels): items 1 and 2 added to the sweep's loss gradients — the carried gradient for the sweep's first record, the
//     engine's combined seed rows (caller's schedule + this) for the others;
//   PARAM (after them): items 3 and 4 added to what the step kernels left, each sum in fp64 in a fixed order (TeamOne::sum3), rounded once.
// No atomics: bit-reproducible. Work vectors: W.x64 (x_new), W.y64 (q), W.c64 (corners), W.k64[0] (phi), W.k64[1] (r_p) — idle outside the steps.
#define DC_KERNEL_TU
#define DC_ADJ_VELOCITY
#include <algorithm>
#include "dc_devlib.h"
#include "dc_adjoint64.h"
#include "dc_readout_adjoint.h"

namespace dc {
namespace {

constexpr int kThreads = 512;       // one workgroup per rollout; 8 waves keep 256 registers per lane: at 1024 threads the parameter pass spills (26 VGPRs, 76 B of scratch)

// (dr/dd)^T u, r and dr/dmu of one contact in fp64 for a given case (1 take-off, 2 stick, 3 slide): the expressions of dri_dfi_T_d / dri_dmu_d
struct ContactD {
  d3 n, d;
  double mu;
  int st;          // 0 = not in primitive contact
  __device__ __forceinline__ d3 JT(d3 u) const {
    if (st < 2) return mkd(0, 0, 0);
    if (st == 2) return mkd(0, 0, 0) - u;
    const double sd = dot(d, n);
    const d3 dT = d - n * sd;
    const double nT = sqrt(dot(dT, dT));
    const d3 a = dT * (1.0 / nT);
    d3 q = u - a * dot(a, u);
    q = q - n * dot(n, q);
    d3 w = n * (-dot(n, u));
    w = w + (q * (sd / nT) + n * dot(a, u)) * mu;
    return w;
  }
  __device__ __forceinline__ d3 r() const {
    if (st < 2) return mkd(0, 0, 0);
    if (st == 2) return mkd(0, 0, 0) - d;
    const double sd = dot(d, n);
    const d3 dN = n * sd, dT = d - dN;
    const double nT = sqrt(dot(dT, dT));
    return mkd(0, 0, 0) - dN - dT * (mu * fabs(sd) / nT);
  }
  __device__ __forceinline__ d3 dmu() const {
    if (st != 3) return mkd(0, 0, 0);
    const double sd = dot(d, n);
    const d3 dT = d - n * sd;
    return dT * (-fabs(sd) / sqrt(dot(dT, dT)));
  }
};

// the contact of vertex i as the backward step sees it: case decided by the fp32 arithmetic of the read-out on the fp32 record (contact_state),
// or in fp64 for a record handed in from outside, exactly as contact_JT_d / finish_gradients64 do
__device__ __forceinline__ ContactD contact_of(const DevSystem &S, const Adj64 &C, int i) {
  ContactD K;
  K.st = 0; K.mu = 0; K.n = mkd(0, 0, 0); K.d = mkd(0, 0, 0);
  const int prim = C.rec_prim[i];
  if (prim < 0) return K;
  const int N = S.N;
  const float muf = C.mu[S.prims[prim].group];
  K.mu = (double) muf;
  if (C.inj_f) {
    K.n = ld3d(C.inj_n, i, N);
    K.d = prim_d_d(S.prims[prim], K.n, ld3d(C.inj_f, i, N), S.mass64[i], C.pvel);
    const double sd = dot(K.d, K.n);
    if (sd >= 0.0) K.st = 1;
    else {
      const d3 dT = K.d - K.n * sd;
      K.st = sqrt(dot(dT, dT)) <= K.mu * fabs(sd) ? 2 : 3;
    }
    return K;
  }
  const f3 nf = ld3(C.rec_n, i, N);
  const f3 df = prim_d(S.prims[prim], nf, ld3(C.rec_f, i, N), S.mass[i], C.pvel);
  K.st = contact_state(nf, df, muf);
  K.n = tod(nf); K.d = tod(df);
  return K;
}

}  // namespace

// (named in namespace dc, like the step kernels: tests/test_kernel_resources_readout.py finds the instances by name in the code object)
template <int PHASE>
__global__ __launch_bounds__(kThreads) void k_readout_adjoint(const DevSystem *__restrict__ Sp, const DevWork W, const ReadoutAdjArgs A) {
  __shared__ double red[3 * (kThreads / 64)];
  const DevSystem &S = *Sp;
  const int N = S.N, G = S.ngroups, P = S.nprim, NC = S.NC, B = A.B, Af = S.Af;
  const int b = blockIdx.x, tid = threadIdx.x;
  const size_t se = (size_t) B * 3 * N, off = (size_t) b * 3 * N;
  const double h = S.h64, ih = 1.0 / h, h2 = h * h;
  TeamOne<kThreads> tm{N, red};
  double *wx = W.x64 + off, *wq = W.y64 + off, *wphi = W.k64[0] + off, *wr = W.k64[1] + off, *wc = W.c64 + (size_t) b * 3 * NC;
  const auto X = tm.yv(wx), Y = tm.yv(wq), CV = tm.yv(wc, NC);
  const bool rows = S.win_rows != 0 && S.brow_ptr != nullptr;
  // the seed phase also visits record first - 1: its part of the loss gradient at the state the call arrives at is a seed row like the others
  const int last = PHASE == 0 ? (A.first - 1 >= 1 ? A.first - 1 : A.first) : A.first;
  for (int s = A.slot; s >= last; s--) {
    if (!A.has[s]) continue;
    __syncthreads();
    const size_t row = (size_t) s * B + b;
    Adj64 C;
    C.xnew = A.X + se * s + off; C.rec_f = A.F + se * s + off; C.rec_n = A.NRM + se * s + off;
    C.xprev = A.X + se * (s - 1) + off; C.vnew = A.V + se * s + off;
    C.rec_prim = A.PRIM + row * N;
    C.mu = A.mu + (size_t) b * G;
    C.pvel = A.PV ? A.PV + row * G * kPvRow : nullptr; C.d_pvel = nullptr;
    C.nself = 0; C.b = b; C.lds = nullptr; C.lds_floats = 0;
    const bool inj = s == A.inj_slot && A.inj_x;
    C.inj_x = inj ? A.inj_x + off : nullptr; C.inj_f = inj ? A.inj_f + off : nullptr; C.inj_n = inj ? A.inj_n + off : nullptr;
    C.inj_sn = nullptr; C.inj_sd = nullptr;
    const float *wj = A.WJ + row * N, *ww = A.WW + row * (size_t) (G > 0 ? G : 1) * kWrenchRow;
    const float *cen = A.PC + row * 3 * P;
    const float *xs = C.xnew;
    // phi, q and r_p of every vertex; x_new in fp64
    for (int i = tid; i < N; i += kThreads) {
      st3d(wx, i, N, xnew64(S, C, i));
      const ContactD K = contact_of(S, C, i);
      d3 phi = mkd(0, 0, 0), q = phi, r = phi;
      if (K.st >= 2) {
        const int g = S.prims[C.rec_prim[i]].group;
        int p0 = 0;
        while (p0 < P - 1 && S.prims[p0].group != g) p0++;
        const float *w = ww + (size_t) g * kWrenchRow;
        const d3 Jh = mkd((double) w[0], (double) w[1], (double) w[2]), th = mkd((double) w[3], (double) w[4], (double) w[5]);
        const f3 xi = ld3(xs, i, N);
        const d3 arm = mkd((double) xi.x - (double) cen[3 * p0], (double) xi.y - (double) cen[3 * p0 + 1], (double) xi.z - (double) cen[3 * p0 + 2]);
        phi = mkd(0, 0, 0) - Jh - cross(th, arm) + K.n * ((double) wj[i] + (double) w[6]);
        q = K.JT(phi);
        r = K.r();
      }
      st3d(wphi, i, N, phi); st3d(wq, i, N, q); st3d(wr, i, N, r);
    }
    __syncthreads();
    if constexpr (PHASE == 0) {
      // item 1: the adjoint's element operator applied to q (apply_K64 without its mass term and contact part), and the direct dependence of tau on x
      element_pass64<kThreads>(S, X, Y, CV, 0, S.T, 0, rows ? 0 : S.E);
      __syncthreads();
      const double hk = h2 * S.k_att64;
      const int flap0 = 3 * S.T;
      float *tx = s == A.slot ? (A.top_done ? nullptr : A.gx + off) : A.rsx + se * s + off;      // loss gradient w.r.t. x at slot s (a chain has it)
      float *tv = s >= A.first ? A.rsv + se * (s - 1) + off : nullptr;                             // ... w.r.t. v at slot s - 1: a record of this call
      for (int i = tid; i < N; i += kThreads) {
        d3 o = mkd(0, 0, 0);
        const int k1 = S.inc_ptr[i + 1];
        if (rows) {
          for (int k = S.inc_ptr[i]; k < k1; k++) { const int c = S.inc_idx[k]; if (c >= flap0) break; o = o + ld3y(CV, c, NC); }
          const d3 yi = ld3y(Y, i, N);
          d3 bb = mkd(0, 0, 0);
          const int r1 = S.brow_ptr[i + 1];
          for (int k = S.brow_ptr[i]; k < r1; k++) bb = bb + (ld3y(Y, S.brow_col[k], N) - yi) * S.brow_val[k];
          o = o + bb;
        } else {
          for (int k = S.inc_ptr[i]; k < k1; k++) o = o + ld3y(CV, S.inc_idx[k], NC);
        }
        if (S.att_of_vertex[i] >= 0) o = o + ld3y(Y, i, N) * hk;
        d3 g1 = mkd(0, 0, 0) - o * ih;
        const int prim = C.rec_prim[i];
        if (prim >= 0) {
          const float *w = ww + (size_t) S.prims[prim].group * kWrenchRow;
          g1 = g1 - cross(ld3d(wr, i, N), mkd((double) w[3], (double) w[4], (double) w[5]));
        }
        if (tx) st3(tx, i, N, tof(tod(ld3(tx, i, N)) + g1));
        if (tv) st3(tv, i, N, tof(tod(ld3(tv, i, N)) + ld3d(wq, i, N) * S.mass64[i]));
      }
    } else {
      // items 3 and 4: what finish_gradients64 forms from y and u, with q / h in place of y and phi / h in place of u
      double s3[3];
      double pacc[7] = {0, 0, 0, 0, 0, 0, 0};
      const int T = S.T, E = S.E;
      for (int t = tid; t < T; t += kThreads) {
        const int i0 = S.tri_v[t], i1 = S.tri_v[T + t], i2 = S.tri_v[2 * T + t];
        // q is zero away from the contacts: an element none of whose vertices is in primitive contact adds an exact zero
        if (C.rec_prim[i0] < 0 && C.rec_prim[i1] < 0 && C.rec_prim[i2] < 0) continue;
        const double Dx = S.tri_D64[t], Dy = S.tri_D64[T + t], Dz = S.tri_D64[2 * T + t], Dw = S.tri_D64[3 * T + t];
        const d3 x0 = ld3y(X, i0, N);
        const d3 e0 = ld3y(X, i1, N) - x0, e1 = ld3y(X, i2, N) - x0;
        const d3 f0 = e0 * Dx + e1 * Dz, f1 = e0 * Dy + e1 * Dw;
        const PolarD Pl = polar3x2d(f0, f1);
        const double w2 = S.tri_w2_64[t];
        const d3 g0 = (Pl.t0 - f0) * w2, g1 = (Pl.t1 - f1) * w2;
        const d3 c1 = g0 * Dx + g1 * Dy, c2 = g0 * Dz + g1 * Dw;
        const d3 q0 = ld3y(Y, i0, N);
        pacc[0] += dot(c1, ld3y(Y, i1, N) - q0) + dot(c2, ld3y(Y, i2, N) - q0);
      }
      for (int e = tid; e < E; e += kThreads) {
        const int i0 = S.bend_v[e], i1 = S.bend_v[E + e], i2 = S.bend_v[2 * E + e], i3 = S.bend_v[3 * E + e];
        if (C.rec_prim[i0] < 0 && C.rec_prim[i1] < 0 && C.rec_prim[i2] < 0 && C.rec_prim[i3] < 0) continue;
        const double w1 = S.bend_w64[E + e], w2 = S.bend_w64[2 * E + e], w3 = S.bend_w64[3 * E + e];
        const double nrest = S.bend_nw64[e], wsq = S.bend_nw64[E + e];
        const d3 x0 = ld3y(X, i0, N);
        const d3 ev = (ld3y(X, i1, N) - x0) * w1 + (ld3y(X, i2, N) - x0) * w2 + (ld3y(X, i3, N) - x0) * w3;
        d3 p = mkd(0, 0, 0);
        if (nrest > 1e-6) { const double n2 = dot(ev, ev); p = n2 > 0 ? ev * (nrest * rsqrt_d(n2)) : ev * nrest; }
        const d3 q0 = ld3y(Y, i0, N);
        const d3 ey = (ld3y(Y, i1, N) - q0) * w1 + (ld3y(Y, i2, N) - q0) * w2 + (ld3y(Y, i3, N) - q0) * w3;
        pacc[1] += dot((p - ev) * wsq, ey);
      }
      double dmu_part[kMaxPrims];
#pragma unroll
      for (int k = 0; k < kMaxPrims; k++) dmu_part[k] = 0.0;
      float *dxf = A.DXF + ((size_t) s * B + b) * 3 * Af;
      const float *xf = A.XF + ((size_t) s * B + b) * 3 * Af;
      const float *vp = A.V + se * (s - 1) + off;
      float *ys = A.YS ? A.YS + se * s + off : nullptr;
      float *y32 = s == A.first ? W.vbest + off : nullptr;
      const d3 grav = mkd(S.g64[0], S.g64[1], S.g64[2]);
      for (int i = tid; i < N; i += kThreads) {
        const d3 qi = ld3d(wq, i, N), qh = qi * ih;
        const double m = S.mass64[i];
        const int a = S.att_of_vertex[i];
        if (a >= 0) {
          pacc[2] += S.k_att64 * dot(tod(ld3(xf, a, Af)) - ld3y(X, i, N), qh);
          st3(dxf, a, Af, tof(tod(ld3(dxf, a, Af)) + qi * (h * S.k_att64)));
        }
        pacc[3] += (m / S.density64) * dot(qi, tod(ld3(vp, i, N)) + grav * h);
        pacc[4] += h * qi.x; pacc[5] += h * qi.y; pacc[6] += h * qi.z;
        const int prim = C.rec_prim[i];
        if (prim >= 0) {
          const int grp = S.prims[prim].group;
          const double contrib = dot(contact_of(S, C, i).dmu(), ld3d(wphi, i, N));
#pragma unroll
          for (int k = 0; k < kMaxPrims; k++) dmu_part[k] += (k == grp) ? contrib : 0.0;
          if (ys) st3(ys, i, N, tof(tod(ld3(ys, i, N)) + qh));
          if (y32) st3(y32, i, N, tof(tod(ld3(y32, i, N)) + qh));
        }
      }
      const bool writer = tid == 0;
      for (int k0 = 0; k0 < G; k0 += 3) {
        double val[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
          val[c] = 0.0;
#pragma unroll
          for (int k = 0; k < kMaxPrims; k++) val[c] += (k == k0 + c) ? dmu_part[k] : 0.0;
        }
        tm.sum3(val[0], val[1], val[2], s3);
        if (writer)
          for (int c = 0; c < 3 && k0 + c < G; c++) { float *o = A.DMU + (size_t) b * G + k0 + c; *o = (float) ((double) *o + s3[c]); }
      }
      if (A.DPV) {
        float *dw = A.DPV + row * G * kPvRow;
        for (int g = 0; g < G; g++) {
          d3 acc = mkd(0, 0, 0), spin = mkd(0, 0, 0);
          for (int i = tid; i < N; i += kThreads) {
            const int prim = C.rec_prim[i];
            if (prim >= 0 && S.prims[prim].group == g) {
              const d3 gi = ld3d(wq, i, N) * S.mass64[i];
              acc = acc + gi;
              if (S.prims[prim].kind == DC_PRIM_SPHERE)
                spin = spin + cross(C.inj_f ? ld3d(C.inj_n, i, N) : tod(ld3(C.rec_n, i, N)), gi) * (double) S.prims[prim].radius;
            }
          }
          tm.sum3(acc.x, acc.y, acc.z, s3);
          if (writer)
            for (int c = 0; c < 3; c++) dw[kPvRow * g + c] = (float) ((double) dw[kPvRow * g + c] - s3[c]);
          tm.sum3(spin.x, spin.y, spin.z, s3);
          if (writer)
            for (int c = 0; c < 3; c++) dw[kPvRow * g + 3 + c] = (float) ((double) dw[kPvRow * g + 3 + c] - s3[c]);
        }
      }
      float *dp = A.DPAR + row * 8;
      const double scale[7] = {S.k_stretch64 > 0 ? h2 / S.k_stretch64 : 0.0, S.k_bend64 > 0 ? h2 / S.k_bend64 : 0.0,
                               S.k_att64 > 0 ? h2 / S.k_att64 : 0.0, 1.0, 1.0, 1.0, 1.0};
      pacc[0] *= ih; pacc[1] *= ih;
      for (int k0 = 0; k0 < 7; k0 += 3) {
        tm.sum3(pacc[k0], k0 + 1 < 7 ? pacc[k0 + 1 < 7 ? k0 + 1 : 6] : 0.0, k0 + 2 < 7 ? pacc[k0 + 2 < 7 ? k0 + 2 : 6] : 0.0, s3);
        if (writer)
          for (int c = 0; c < 3 && k0 + c < 7; c++) dp[k0 + c] = (float) ((double) dp[k0 + c] + s3[c] * scale[k0 + c]);
      }
    }
  }
}

namespace {

// [rows][n] weights in the caller's vertex numbering (fp32 or fp64) -> fp32 in device numbering
template <class T>
__global__ void k_vertex_rows_in(const T *__restrict__ src, float *__restrict__ dst, long rows, int n, const int *__restrict__ user_of) {
  const long total = rows * n;
  for (long k = (long) blockIdx.x * blockDim.x + threadIdx.x; k < total; k += (long) gridDim.x * blockDim.x) {
    const long r = k / n;
    const int i = (int) (k - r * n);
    dst[k] = (float) src[r * n + (user_of ? user_of[i] : i)];
  }
}

}  // namespace

void launch_readout_adjoint(const DevSystem &S, const DevWork &W, const ReadoutAdjArgs &A, int phase, hipStream_t st) {
  if (A.B <= 0 || S.N <= 0 || A.slot < A.first) return;
  const dim3 g((unsigned) A.B), b(kThreads);
  if (phase == 0) hipLaunchKernelGGL(k_readout_adjoint<0>, g, b, 0, st, S.self_dev, W, A);
  else hipLaunchKernelGGL(k_readout_adjoint<1>, g, b, 0, st, S.self_dev, W, A);
}

void launch_vertex_rows_in(const void *src, int is_f32, float *dst, long rows, int n, const int *user_of, hipStream_t st) {
  const long total = rows * n;
  if (total <= 0) return;
  const dim3 g((unsigned) std::min<long>((total + 255) / 256, 4096)), b(256);
  if (is_f32) hipLaunchKernelGGL(k_vertex_rows_in<float>, g, b, 0, st, (const float *) src, dst, rows, n, user_of);
  else hipLaunchKernelGGL(k_vertex_rows_in<double>, g, b, 0, st, (const double *) src, dst, rows, n, user_of);
}

}  // namespace dc
