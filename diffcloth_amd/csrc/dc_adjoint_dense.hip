// CDNA4 (gfx950) dense direct adjoint solve, dc_params::adjoint_mode = 2 (dc_adjoint_dense.h): the GPU counterpart of
// Simulation::solveDirect (reference Simulation.cpp:1431-1440), which builds K = P - dP^T and factors it with SparseLU.
//
//   assembly   K = M + E Y,  E = h^2 (A - dp/dx)^T A + h^2 k_att (attachments),  Y = (I + dr_df)^T = Pprim S_0 S_1 ... S_{L-1}
//              (form_y64, dc_adjoint64.h: the self layers L-1 .. 0 act first, the block-diagonal primitive part last). E's entries are
//              probed from the operator's own element pass (element_pass64 on unit vectors), the contact factors from its own dr_df^T
//              (contact_JT_d, dri_dfi_T_d / _dd); one thread owns the three rows of a vertex, so every entry is summed in a fixed order
//              (no atomics, bitwise reproducible). Right-multiplying by a contact factor is row-local: each row walks the contacts.
//   LU         partial pivoting (ties: the lowest row), fp64 VALU, blocked right-looking with panels of kLuPanel columns: a panel kernel
//              (one workgroup per matrix, column by column), the panel's row swaps + unit-lower TRSM of U12 (one thread per column),
//              the trailing update A22 -= L21 U12 tiled over (matrix, 64 x 64 tile). A zero or non-finite pivot flags the rollout.
//   solve      k_adjoint_dense_step: the adjoint step of dc_adjoint.hip with the correction solve replaced by forward / back substitution
//              with the factors (b in LDS), each followed by the fp64 residual (residual64); at most kDenseRefine cycles, then (or for a
//              flagged rollout) the fp64 BiCGSTAB fall-back (bicgstab64). Gradients, clipping and statistics as in k_adjoint_step.
#define DC_KERNEL_TU
#define DC_ADJ_VELOCITY      // the direct solves read the obstacle-velocity rows when the context has them (dc_adjoint64.h)
#include "dc_devlib.h"
#include "dc_adjprecond.h"
#include "dc_adjoint64.h"
#include "dc_adjoint_dense.h"
#include "dc_adjoint_direct.h"

namespace dc {

constexpr int kDenseRefine = 3;        // substitutions (each followed by an fp64 residual) before the fp64 BiCGSTAB fall-back

namespace {

// x_new in fp64 (xnew64, as prepare_x64 forms it), the primitive contacts' (I + dr_df)^T blocks and the self contacts' G blocks
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_dense_prep(const DevSystem *__restrict__ Sp, BwdArgs A, double *x64, DenseAdjWork D, int b0) {
  const DevSystem &S = *Sp;
  const int b = b0 + blockIdx.x, tid = threadIdx.x, N = S.N;
  const Adj64 C = dense_adj64(S, A, b);
  double *xb = x64 + (size_t) b * 3 * N, *pm = D.pm + (size_t) blockIdx.x * 9 * N;
  const d3 e[3] = {mkd(1, 0, 0), mkd(0, 1, 0), mkd(0, 0, 1)};
  for (int i = tid; i < N; i += THREADS) {
    st3d(xb, i, N, xnew64(S, C, i));
    if (C.rec_prim[i] < 0) continue;
    for (int c = 0; c < 3; c++) {           // column c of (I + J_i^T): e_c + dr_df^T e_c
      const d3 col = e[c] + contact_JT_d(S, C, i, e[c]);
      pm[(3 * c) * N + i] = col.x; pm[(3 * c + 1) * N + i] = col.y; pm[(3 * c + 2) * N + i] = col.z;
    }
  }
  if (C.nself <= 0) return;
  const int cap = S.self_cap;
  const int *meta = C.self.meta + (size_t) b * kMetaStride;
  const int Cn = min(meta[0], cap);
  const int2 *pair = C.self.pair + (size_t) b * cap;
  double *sg = D.sg + (size_t) blockIdx.x * 9 * cap;
  for (int k = tid; k < Cn; k += THREADS) {
    const int2 ab = pair[k];
    const double mA = S.mass64[ab.x], mB = S.mass64[ab.y], mred = (mA * mB) / (mA + mB);
    for (int c = 0; c < 3; c++) {
      d3 g;
      if (C.inj_sn) {
        const d3 n = mkd(C.inj_sn[3 * k], C.inj_sn[3 * k + 1], C.inj_sn[3 * k + 2]), d = mkd(C.inj_sd[3 * k], C.inj_sd[3 * k + 1], C.inj_sd[3 * k + 2]);
        g = dri_dfi_T_dd(n, d, (double) kClothMu, e[c]) * mred;
      } else {
        const float4 n4 = C.self.nrm[(size_t) b * cap + k], d4 = C.self.dvec[(size_t) b * cap + k];
        g = dri_dfi_T_d(mk(n4.x, n4.y, n4.z), mk(d4.x, d4.y, d4.z), kClothMu, e[c]) * mred;
      }
      sg[(size_t) k * 9 + 3 * c] = g.x; sg[(size_t) k * 9 + 3 * c + 1] = g.y; sg[(size_t) k * 9 + 3 * c + 2] = g.z;
    }
  }
}

// K of one rollout: thread = vertex i, owner of rows i, N + i, 2N + i
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_dense_assemble(const DevSystem *__restrict__ Sp, BwdArgs A, const double *x64, DenseAdjWork D, int b0) {
  const DevSystem &S = *Sp;
  const int N = S.N, T = S.T, E = S.E, NC = S.NC, n = 3 * N, ld = D.ld, tid = threadIdx.x;
  const int i = blockIdx.x * THREADS + tid, b = b0 + blockIdx.y;
  if (i >= N) return;
  double *K = D.K + (size_t) blockIdx.y * ld * ld;
  const int r[3] = {i, N + i, 2 * N + i};
  for (int col = 0; col < n; col++) { double *q = K + (size_t) col * ld; q[r[0]] = 0.0; q[r[1]] = 0.0; q[r[2]] = 0.0; }
  auto add = [&](int col, d3 v) { double *q = K + (size_t) col * ld; q[r[0]] += v.x; q[r[1]] += v.y; q[r[2]] += v.z; };
  // E: the element corners of vertex i, in the order of its incidence list, probed column by column
  const ProbeV X{0, x64 + (size_t) b * 3 * N, 0, 0, NC, nullptr};
  for (int k = S.inc_ptr[i]; k < S.inc_ptr[i + 1]; k++) {
    const int kk = S.inc_idx[k];
    int vs[4], nv, t0 = 0, t1 = 0, e0 = 0, e1 = 0;
    if (kk < 3 * T) {
      const int t = kk % T;
      vs[0] = S.tri_v[t]; vs[1] = S.tri_v[T + t]; vs[2] = S.tri_v[2 * T + t]; nv = 3;
      t0 = t - tid; t1 = t + 1;               // exactly element t for this thread (element_pass64<1> strides from threadIdx.x)
    } else {
      const int e = (kk - 3 * T) % E;
      vs[0] = S.bend_v[e]; vs[1] = S.bend_v[E + e]; vs[2] = S.bend_v[2 * E + e]; vs[3] = S.bend_v[3 * E + e]; nv = 4;
      e0 = e - tid; e1 = e + 1;
    }
    for (int jv = 0; jv < nv; jv++)
      for (int c = 0; c < 3; c++) {
        d3 o = mkd(0, 0, 0);
        const ProbeV Y{1, nullptr, c * N + vs[jv], 0, NC, nullptr}, CV{2, nullptr, 0, kk, NC, &o};
        element_pass64<1>(S, X, Y, CV, t0, t1, e0, e1);
        add(c * N + vs[jv], o);
      }
  }
  if (S.att_of_vertex[i] >= 0) {              // attachment: h^2 k_att I (apply_K64; dp/dx = 0, AttachmentSpring.cpp:35-37)
    const double hk = S.h64 * S.h64 * S.k_att64;
    for (int c = 0; c < 3; c++) K[(size_t) r[c] * ld + r[c]] += hk;
  }
  // E Pprim: column block j of every primitive contact vertex times (I + J_j^T)
  const Adj64 C = dense_adj64(S, A, b);
  const double *pm = D.pm + (size_t) blockIdx.y * 9 * N;
  for (int j = 0; j < N; j++) {
    if (C.rec_prim[j] < 0) continue;
    double m[9];
    for (int q = 0; q < 9; q++) m[q] = pm[q * N + j];     // m[3 c' + c] = entry (c, c')
    for (int a = 0; a < 3; a++) {
      double *x0 = K + (size_t) j * ld + r[a], *x1 = x0 + (size_t) N * ld, *x2 = x1 + (size_t) N * ld;
      const double v0 = *x0, v1 = *x1, v2 = *x2;
      *x0 = v0 * m[0] + v1 * m[1] + v2 * m[2];
      *x1 = v0 * m[3] + v1 * m[4] + v2 * m[5];
      *x2 = v0 * m[6] + v1 * m[7] + v2 * m[8];
    }
  }
  // ... S_0 S_1 ... S_{L-1}: per contact (a, b) of layer l, W = X_a / m_a - X_b / m_b, X_a += W G, X_b -= W G
  if (C.nself > 0) {
    const int cap = S.self_cap;
    const int *meta = C.self.meta + (size_t) b * kMetaStride;
    const int nl = meta[1];
    const int2 *pair = C.self.pair + (size_t) b * cap;
    const double *sg = D.sg + (size_t) blockIdx.y * 9 * cap;
    for (int l = 0; l < nl; l++) {
      const int k1 = meta[2 + l + 1];
      for (int k = meta[2 + l]; k < k1; k++) {
        const int2 ab = pair[k];
        const double iA = 1.0 / S.mass64[ab.x], iB = 1.0 / S.mass64[ab.y];
        double g[9];
        for (int q = 0; q < 9; q++) g[q] = sg[(size_t) k * 9 + q];     // g[3 c' + c] = entry (c, c')
        for (int a = 0; a < 3; a++) {
          double *pa = K + (size_t) ab.x * ld + r[a], *pb = K + (size_t) ab.y * ld + r[a];
          const size_t s = (size_t) N * ld;
          const double xa0 = pa[0], xa1 = pa[s], xa2 = pa[2 * s], xb0 = pb[0], xb1 = pb[s], xb2 = pb[2 * s];
          const double w0 = xa0 * iA - xb0 * iB, w1 = xa1 * iA - xb1 * iB, w2 = xa2 * iA - xb2 * iB;
          const double q0 = w0 * g[0] + w1 * g[1] + w2 * g[2], q1 = w0 * g[3] + w1 * g[4] + w2 * g[5], q2 = w0 * g[6] + w1 * g[7] + w2 * g[8];
          pa[0] = xa0 + q0; pa[s] = xa1 + q1; pa[2 * s] = xa2 + q2;
          pb[0] = xb0 - q0; pb[s] = xb1 - q1; pb[2 * s] = xb2 - q2;
        }
      }
    }
  }
  const double m = S.mass64[i];
  for (int c = 0; c < 3; c++) K[(size_t) r[c] * ld + r[c]] += m;
}

// Panel [k0, k0 + kb) of one matrix, column by column: pivot search, row swap across the panel, scaling, rank-1 update of the rest of
// the panel. The update of column j also finds column j + 1's candidate pivot of each thread.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_lu_panel(DenseAdjWork D, int n, int k0, int kb) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  constexpr int NW = THREADS / 64;
  if (D.flag[blockIdx.x]) return;
  double *A = D.K + (size_t) blockIdx.x * D.ld * D.ld;
  int *piv = D.piv + (size_t) blockIdx.x * D.ld;
  const size_t ld = D.ld;
  __shared__ double sv[NW], urow[kLuPanel];
  __shared__ int si[NW];
  double tv = -1.0;
  int tr = n;
  for (int i = k0 + tid; i < n; i += THREADS) amax_merge(tv, tr, fabs(A[(size_t) k0 * ld + i]), i);
  for (int j = k0; j < k0 + kb; j++) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) amax_merge(tv, tr, __shfl_xor(tv, o, 64), __shfl_xor(tr, o, 64));
    if (lane == 0) { sv[wv] = tv; si[wv] = tr; }
    __syncthreads();                            // (also: the previous column's update is complete)
    double pv = sv[0];
    int p = si[0];
    for (int w = 1; w < NW; w++) amax_merge(pv, p, sv[w], si[w]);
    if (!(pv > 0.0) || !isfinite(pv) || p >= n) {      // singular or non-finite: this rollout takes the fall-back
      if (tid == 0) D.flag[blockIdx.x] = 1;
      return;
    }
    if (tid < kb) {
      double *q = A + (size_t) (k0 + tid) * ld;
      const double a = q[j], c = q[p];
      q[j] = c; q[p] = a;
      urow[tid] = c;
    }
    if (tid == 0) piv[j] = p;
    __syncthreads();
    const double inv = 1.0 / urow[j - k0];
    tv = -1.0; tr = n;
    for (int i = j + 1 + tid; i < n; i += THREADS) {
      double *q = A + (size_t) j * ld + i;
      const double l = *q * inv;
      *q = l;
      for (int jj = j + 1 - k0; jj < kb; jj++) {
        double *a = A + (size_t) (k0 + jj) * ld + i;
        const double v = *a - l * urow[jj];
        *a = v;
        if (jj == j + 1 - k0) amax_merge(tv, tr, fabs(v), i);
      }
    }
  }
}

// Row swaps of panel [k0, k0 + kLuPanel) and U12 = L11^-1 A12 on the columns right of it: one thread per column
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_lu_trsm(DenseAdjWork D, int n, int k0) {
  const int tid = threadIdx.x;
  if (D.flag[blockIdx.y]) return;
  const size_t ld = D.ld;
  double *A = D.K + (size_t) blockIdx.y * ld * ld;
  const int *piv = D.piv + (size_t) blockIdx.y * ld;
  __shared__ double L[kLuPanel][kLuPanel + 1];      // L[jj][ii] = entry (k0 + ii, k0 + jj)
  __shared__ int sp[kLuPanel];
  for (int q = tid; q < kLuPanel * kLuPanel; q += THREADS) { const int jj = q / kLuPanel, ii = q % kLuPanel; L[jj][ii] = A[(size_t) (k0 + jj) * ld + k0 + ii]; }
  if (tid < kLuPanel) sp[tid] = piv[k0 + tid];
  __syncthreads();
  const int c = k0 + kLuPanel + blockIdx.x * THREADS + tid;
  if (c >= n) return;
  double *q = A + (size_t) c * ld;
  for (int jj = 0; jj < kLuPanel; jj++) {
    const int p = sp[jj];
    if (p != k0 + jj) { const double a = q[k0 + jj]; q[k0 + jj] = q[p]; q[p] = a; }
  }
  double x[kLuPanel];
#pragma unroll
  for (int ii = 0; ii < kLuPanel; ii++) x[ii] = q[k0 + ii];
#pragma unroll
  for (int jj = 0; jj < kLuPanel; jj++)
#pragma unroll
    for (int ii = jj + 1; ii < kLuPanel; ii++) x[ii] -= L[jj][ii] * x[jj];
#pragma unroll
  for (int ii = 0; ii < kLuPanel; ii++) q[k0 + ii] = x[ii];
}

// Trailing update A22 -= L21 U12 for panel [k0, k0 + kLuPanel): one 64 x 64 tile of one matrix per workgroup, 4 x 4 entries per thread
constexpr int kTile = 64;
__global__ __launch_bounds__(256) void k_lu_update(DenseAdjWork D, int n, int k0, int tiles) {
  const int tid = threadIdx.x;
  if (D.flag[blockIdx.y]) return;
  const size_t ld = D.ld;
  double *A = D.K + (size_t) blockIdx.y * ld * ld;
  const int k1 = k0 + kLuPanel;
  const int i0 = k1 + (blockIdx.x % tiles) * kTile, j0 = k1 + (blockIdx.x / tiles) * kTile;
  __shared__ double Ls[kLuPanel][kTile], Us[kLuPanel][kTile + 1];
  for (int q = tid; q < kLuPanel * kTile; q += 256) {
    const int k = q / kTile, ii = q % kTile;
    Ls[k][ii] = (i0 + ii < n) ? A[(size_t) (k0 + k) * ld + i0 + ii] : 0.0;
    const int jj = q / kLuPanel, kk = q % kLuPanel;
    Us[kk][jj] = (j0 + jj < n) ? A[(size_t) (j0 + jj) * ld + k0 + kk] : 0.0;
  }
  __syncthreads();
  const int tx = tid & 15, ty = tid >> 4;
  double acc[4][4] = {};
#pragma unroll 8
  for (int k = 0; k < kLuPanel; k++) {
    double l[4], u[4];
#pragma unroll
    for (int a = 0; a < 4; a++) { l[a] = Ls[k][tx + 16 * a]; u[a] = Us[k][ty + 16 * a]; }
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
      for (int c = 0; c < 4; c++) acc[a][c] = fma(l[a], u[c], acc[a][c]);
  }
#pragma unroll
  for (int c = 0; c < 4; c++) {
    const int j = j0 + ty + 16 * c;
    if (j >= n) continue;
#pragma unroll
    for (int a = 0; a < 4; a++) {
      const int i = i0 + tx + 16 * a;
      if (i < n) A[(size_t) j * ld + i] -= acc[a][c];
    }
  }
}

// d = K^-1 r with the LU factors of this rollout, in LDS (bv: n doubles, blk: kLuPanel^2 doubles); every thread of the workgroup
template <int THREADS>
__device__ __forceinline__ void lu_substitute(const double *__restrict__ A, const int *__restrict__ piv, int n, size_t ld, double *bv, double *blk) {
  const int tid = threadIdx.x;
  // forward: per panel the row swaps, the unit-lower diagonal block (one wave), the rows below
  for (int k0 = 0; k0 < n; k0 += kLuPanel) {
    const int kb = min(kLuPanel, n - k0);
    for (int q = tid; q < kb * kb; q += THREADS) { const int jj = q / kb, ii = q % kb; blk[jj * kLuPanel + ii] = A[(size_t) (k0 + jj) * ld + k0 + ii]; }
    if (tid == 0)
      for (int jj = 0; jj < kb; jj++) { const int p = piv[k0 + jj]; if (p != k0 + jj) { const double a = bv[k0 + jj]; bv[k0 + jj] = bv[p]; bv[p] = a; } }
    __syncthreads();
    if (tid < 64) {
      for (int jj = 0; jj < kb; jj++) {
        const double x = bv[k0 + jj];
        if (tid > jj && tid < kb) bv[k0 + tid] -= blk[jj * kLuPanel + tid] * x;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      }
    }
    __syncthreads();
    for (int i = k0 + kb + tid; i < n; i += THREADS) {
      double s = 0.0;
      for (int jj = 0; jj < kb; jj++) s += A[(size_t) (k0 + jj) * ld + i] * bv[k0 + jj];
      bv[i] -= s;
    }
    __syncthreads();
  }
  // backward: per panel from the last, the upper diagonal block (one wave), then the rows above
  for (int k0 = (n - 1) / kLuPanel * kLuPanel; k0 >= 0; k0 -= kLuPanel) {
    const int kb = min(kLuPanel, n - k0);
    for (int q = tid; q < kb * kb; q += THREADS) { const int jj = q / kb, ii = q % kb; blk[jj * kLuPanel + ii] = A[(size_t) (k0 + jj) * ld + k0 + ii]; }
    __syncthreads();
    if (tid < 64) {
      for (int jj = kb - 1; jj >= 0; jj--) {
        const double x = bv[k0 + jj] / blk[jj * kLuPanel + jj];
        if (tid < jj) bv[k0 + tid] -= blk[jj * kLuPanel + tid] * x;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        if (tid == 0) bv[k0 + jj] = x;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      }
    }
    __syncthreads();
    for (int i = tid; i < k0; i += THREADS) {
      double s = 0.0;
      for (int jj = 0; jj < kb; jj++) s += A[(size_t) (k0 + jj) * ld + i] * bv[k0 + jj];
      bv[i] -= s;
    }
    __syncthreads();
  }
}

// The adjoint step of one rollout with the dense factors (k_adjoint_step's mode-2 counterpart; one step per launch)
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_adjoint_dense_step(const DevSystem *__restrict__ Sp, DevWork W, BwdArgs A, DenseAdjWork D, int b0) {
  const DevSystem &S = *Sp;
  __shared__ double red[3 * (THREADS / 64)];
  __shared__ double bv[3 * kDenseMaxN], blk[kLuPanel * kLuPanel];
  const int b = b0 + blockIdx.x, tid = threadIdx.x;
  const int N = S.N, n = 3 * N;
  const size_t off = (size_t) b * 3 * N;
  float *gx = A.gx + off;
  // ---- gradient clipping (Simulation.cpp:1460-1466), as k_adjoint_step ----
  float part = 0.f;
  for (int i = tid; i < N; i += THREADS) { f3 q = ld3(gx, i, N); part += dot(q, q); }
  double gnorm = sqrt(block_sum<THREADS>((double) part, red));
  float gscale = 1.f;
  int clipped = 0;
  if (A.clip && gnorm > (double) A.clip_thr * N) { gscale = (float) ((double) A.clip_thr * N / gnorm); clipped = 1; gnorm = (double) A.clip_thr * N; }
  int status = 1, cycles = 0, iters64 = 0, used_direct = 0;      // (a zero gradient has the solution u = 0)
  double udiff = 0;
  TeamOne<THREADS> tm{N, red};
  const Adj64 C64 = dense_adj64(S, A, b);
  Work64 W64;
  W64.u = W.u64 + off; W64.r = W.r64 + off; W64.y = W.y64 + off; W64.x = W.x64 + off; W64.corner = W.c64 + (size_t) b * 3 * S.NC;
  W64.rhat = W.k64[0] + off; W64.p = W.k64[1] + off; W64.v = W.k64[2] + off; W64.t = W.k64[3] + off; W64.ph = W.k64[4] + off; W64.sh = W.k64[5] + off;
  for (int i = tid; i < N; i += THREADS) st3d(W64.u, i, N, mkd(0, 0, 0));
  prepare_x64<THREADS>(S, C64, tm, W64.x);
  if (gnorm > 0) {
    used_direct = 2;
    const double stop = (double) A.rel_tol * (double) A.rel_tol * gnorm * gnorm;
    const double *K = D.K + (size_t) blockIdx.x * D.ld * D.ld;
    const int *piv = D.piv + (size_t) blockIdx.x * D.ld;
    // r = g (u = 0)
    for (int i = tid; i < N; i += THREADS) st3d(W64.r, i, N, tod(ld3(gx, i, N) * gscale));
    double rr_true = gnorm * gnorm;
    status = 0;
    const bool factored = D.flag[blockIdx.x] == 0;
    __syncthreads();
    for (; factored && cycles < kDenseRefine; ) {
      for (int q = tid; q < n; q += THREADS) bv[q] = W64.r[q];
      __syncthreads();
      lu_substitute<THREADS>(K, piv, n, (size_t) D.ld, bv, blk);
      for (int q = tid; q < n; q += THREADS) W64.u[q] += bv[q];
      __syncthreads();
      cycles++;
      const double rr_new = residual64<THREADS>(S, C64, tm, W64, gx, gscale).rr;
      if (!(rr_new < rr_true)) {               // no progress (NaN-safe): take the correction back, the fall-back goes on from there
        for (int q = tid; q < n; q += THREADS) W64.u[q] -= bv[q];
        __syncthreads();
        rr_true = residual64<THREADS>(S, C64, tm, W64, gx, gscale).rr;
        break;
      }
      rr_true = rr_new;
      if (rr_true <= stop) { status = 1; break; }
    }
    if (status != 1) {
      // ---- fp64 BiCGSTAB on the same operator from (u, r), as the mixed-precision direct solve's fall-back (dc_adjoint.hip) ----
      float *minv = W.minv + (size_t) b * 9 * N;
      for (int i = tid; i < N; i += THREADS)
        store_block_inverse(elastic_diag_block(S, C64.xnew, i), S.mass[i], [&](f3 e) { return tof(contact_JT_d(S, C64, i, tod(e))); }, minv, i, N);
      __syncthreads();
      const double stop_fb = fmax(stop * 1e-8, 1e-26 * gnorm * gnorm);
      double rr64 = rr_true;
      for (int pass = 0; pass < 3; pass++) {
        const auto r64 = bicgstab64<THREADS>(S, C64, tm, W64, minv, stop_fb, 20000, rr64, iters64);
        iters64 = r64.iters;
        rr64 = residual64<THREADS>(S, C64, tm, W64, gx, gscale).rr;
        if (rr64 <= stop) status = 1;
        if (rr64 <= stop_fb || r64.res == 0) break;
      }
      rr_true = rr64;
    }
    udiff = sqrt(rr_true) / gnorm;
  }
  __syncthreads();
  // ---- gradients w.r.t. the previous state and parameters (Simulation.cpp:1534, 1608-1650), in fp64 from u ----
  finish_gradients64<THREADS>(S, C64, tm, W64, A, W.vbest + off);
  if (tid == 0) {
    dc_bwd_stats s;
    s.converged = status; s.adjoint_iters = 0; s.cg_iters = 0; s.clipped = clipped;
    s.used_direct = used_direct; s.last_udiff = (float) udiff;
    s.refine_cycles = cycles; s.fp64_iters = iters64; s.residual_verified = used_direct ? 1 : 0;
    s.workgroups = 1;
    A.stats[b] = s;
  }
}

}  // namespace

void launch_dense_assemble(const DevSystem &S, const BwdArgs &A, double *x64, const DenseAdjWork &D, int b0, int nb, hipStream_t st) {
  hipLaunchKernelGGL(k_dense_prep<256>, dim3(nb), dim3(256), 0, st, S.self_dev, A, x64, D, b0);
  hipLaunchKernelGGL(k_dense_assemble<64>, dim3((S.N + 63) / 64, nb), dim3(64), 0, st, S.self_dev, A, (const double *) x64, D, b0);
}

void launch_dense_prep(const DevSystem &S, const BwdArgs &A, double *x64, const DenseAdjWork &D, int b0, int nb, hipStream_t st) {
  hipLaunchKernelGGL(k_dense_prep<256>, dim3(nb), dim3(256), 0, st, S.self_dev, A, x64, D, b0);
}

int launch_dense_factor(const DenseAdjWork &D, int n, int nb, hipStream_t st) {
  int launches = 0;
  for (int k0 = 0; k0 < n; k0 += kLuPanel) {
    const int kb = std::min(kLuPanel, n - k0);
    hipLaunchKernelGGL(k_lu_panel<1024>, dim3(nb), dim3(1024), 0, st, D, n, k0, kb);
    launches++;
    const int rest = n - k0 - kb;
    if (rest <= 0) continue;
    hipLaunchKernelGGL(k_lu_trsm<256>, dim3((rest + 255) / 256, nb), dim3(256), 0, st, D, n, k0);
    const int tiles = (rest + kTile - 1) / kTile;
    hipLaunchKernelGGL(k_lu_update, dim3(tiles * tiles, nb), dim3(256), 0, st, D, n, k0, tiles);
    launches += 2;
  }
  return launches;
}

void launch_dense_adjoint_step(const DevSystem &S, const DevWork &W, const BwdArgs &A, const DenseAdjWork &D, int b0, int nb, hipStream_t st) {
  hipLaunchKernelGGL(k_adjoint_dense_step<1024>, dim3(nb), dim3(1024), 0, st, S.self_dev, W, A, D, b0);
}

}  // namespace dc
