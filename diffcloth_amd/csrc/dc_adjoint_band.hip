// CDNA4 (gfx950) banded direct adjoint solve, dc_params::adjoint_mode = 3 (dc_adjoint_band.h): dc_adjoint_dense.hip restricted to the band
// of K, with the unknowns interleaved (3 i + c) and K in LAPACK band storage.
//
//   assembly   as k_dense_assemble (the thread of vertex i owns its three rows, E probed from element_pass64 on unit vectors, attachment,
//              the primitive factor per column block, the layered self factors row-locally in the operator's order, the mass), over the
//              row's window of column blocks |i - j| <= (kl - 2) / 3 only. A coupling that leaves the window sets the rollout's flag:
//              an element corner outside it (no mesh has one: the window covers P's bandwidth), or a self contact (a, b) with one block
//              inside the window and one outside while the inside block of this row is non-zero (then the true K has a non-zero there).
//   LU         partial pivoting (ties: the lowest row) among the kl + 1 rows of a column, fp64 VALU, blocked right-looking with panels of
//              kLuPanel columns: a panel kernel (one workgroup per matrix, the (kl + kb) x kb panel in LDS where it fits), the panel's row swaps + unit-
//              lower TRSM on the columns k0 + kb ... k0 + kb + kl + ku - 1 (one thread per column), the trailing update of the kl x (kl + ku)
//              window in 64 x 64 tiles (every tile of that window meets the band). A zero or non-finite pivot flags the rollout.
//   solve      k_adjoint_band_step: k_adjoint_dense_step with band forward / back substitution (b in LDS in interleaved order, a panel
//              block next to it), each followed by the fp64 residual; at most kBandRefine cycles, then (or for a flagged rollout) bicgstab64.
// No inter-workgroup communication, no atomics; every loop is bounded by n, kl or ku.
#define DC_KERNEL_TU
#define DC_ADJ_VELOCITY      // the direct solves read the obstacle-velocity rows when the context has them (dc_adjoint64.h)
#include "dc_devlib.h"
#include "dc_adjprecond.h"
#include "dc_adjoint64.h"
#include "dc_adjoint_band.h"
#include "dc_adjoint_direct.h"
#include "dc_launch.h"

namespace dc {

constexpr int kBandRefine = 3;        // substitutions (each followed by an fp64 residual) before the fp64 BiCGSTAB fall-back

namespace {

// K of one rollout in band storage: thread = vertex i, owner of rows 3 i, 3 i + 1, 3 i + 2
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_band_assemble(const DevSystem *__restrict__ Sp, BwdArgs A, const double *x64, BandAdjWork D, int b0) {
  const DevSystem &S = *Sp;
  const int N = S.N, T = S.T, E = S.E, NC = S.NC, n = D.n, kl = D.kl, kv = 2 * D.kl, tid = threadIdx.x;
  const size_t ldab = D.ldab;
  const int i = blockIdx.x * THREADS + tid, b = b0 + blockIdx.y;
  if (i >= N) return;
  double *AB = D.AB + (size_t) blockIdx.y * ldab * n;
  int *flag = D.flag + blockIdx.y;
  const int wv = (kl - 2) / 3;                            // blocks (i, j) with |i - j| <= wv lie wholly inside the band
  const int jlo = max(0, i - wv), jhi = min(N - 1, i + wv);
  auto at = [&](int r, int c) { return AB + (size_t) c * ldab + (kv + r - c); };
  for (int a = 0; a < 3; a++) {                           // the rows' whole band, the fill included
    const int r = 3 * i + a, c1 = min(n - 1, r + kv);
    for (int c = max(0, r - kl); c <= c1; c++) *at(r, c) = 0.0;
  }
  auto add = [&](int j, int c, d3 v) { *at(3 * i, 3 * j + c) += v.x; *at(3 * i + 1, 3 * j + c) += v.y; *at(3 * i + 2, 3 * j + c) += v.z; };
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
    for (int jv = 0; jv < nv; jv++) {
      if (vs[jv] < jlo || vs[jv] > jhi) { *flag = 1; continue; }
      for (int c = 0; c < 3; c++) {
        d3 o = mkd(0, 0, 0);
        const ProbeV Y{1, nullptr, c * N + vs[jv], 0, NC, nullptr}, CV{2, nullptr, 0, kk, NC, &o};
        element_pass64<1>(S, X, Y, CV, t0, t1, e0, e1);
        add(vs[jv], c, o);
      }
    }
  }
  if (S.att_of_vertex[i] >= 0) {              // attachment: h^2 k_att I (apply_K64; dp/dx = 0, AttachmentSpring.cpp:35-37)
    const double hk = S.h64 * S.h64 * S.k_att64;
    for (int c = 0; c < 3; c++) *at(3 * i + c, 3 * i + c) += hk;
  }
  // E Pprim: column block j of every primitive contact vertex of the window times (I + J_j^T)
  const Adj64 C = dense_adj64(S, A, b);
  const double *pm = D.pm + (size_t) blockIdx.y * 9 * N;
  for (int j = jlo; j <= jhi; j++) {
    if (C.rec_prim[j] < 0) continue;
    double m[9];
    for (int q = 0; q < 9; q++) m[q] = pm[q * N + j];     // m[3 c' + c] = entry (c, c')
    for (int a = 0; a < 3; a++) {
      double *x0 = at(3 * i + a, 3 * j), *x1 = at(3 * i + a, 3 * j + 1), *x2 = at(3 * i + a, 3 * j + 2);
      const double v0 = *x0, v1 = *x1, v2 = *x2;
      *x0 = v0 * m[0] + v1 * m[1] + v2 * m[2];
      *x1 = v0 * m[3] + v1 * m[4] + v2 * m[5];
      *x2 = v0 * m[6] + v1 * m[7] + v2 * m[8];
    }
  }
  // ... S_0 S_1 ... S_{L-1}: per contact (a, b) of layer l, W = X_a / m_a - X_b / m_b, X_a += W G, X_b -= W G. A block outside the window
  // is zero as long as the rollout is not flagged: both outside = nothing to do; one outside = the outside block would become W G.
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
        const bool inA = ab.x >= jlo && ab.x <= jhi, inB = ab.y >= jlo && ab.y <= jhi;
        if (!inA && !inB) continue;
        const double iA = 1.0 / S.mass64[ab.x], iB = 1.0 / S.mass64[ab.y];
        double g[9];
        for (int q = 0; q < 9; q++) g[q] = sg[(size_t) k * 9 + q];     // g[3 c' + c] = entry (c, c')
        for (int a = 0; a < 3; a++) {
          const int r = 3 * i + a;
          double xa0 = 0, xa1 = 0, xa2 = 0, xb0 = 0, xb1 = 0, xb2 = 0;
          if (inA) { xa0 = *at(r, 3 * ab.x); xa1 = *at(r, 3 * ab.x + 1); xa2 = *at(r, 3 * ab.x + 2); }
          if (inB) { xb0 = *at(r, 3 * ab.y); xb1 = *at(r, 3 * ab.y + 1); xb2 = *at(r, 3 * ab.y + 2); }
          if (!(inA && inB)) {
            if (xa0 == 0.0 && xa1 == 0.0 && xa2 == 0.0 && xb0 == 0.0 && xb1 == 0.0 && xb2 == 0.0) continue;
            *flag = 1;                                   // the true K has a non-zero outside the band
          }
          const double w0 = xa0 * iA - xb0 * iB, w1 = xa1 * iA - xb1 * iB, w2 = xa2 * iA - xb2 * iB;
          const double q0 = w0 * g[0] + w1 * g[1] + w2 * g[2], q1 = w0 * g[3] + w1 * g[4] + w2 * g[5], q2 = w0 * g[6] + w1 * g[7] + w2 * g[8];
          if (inA) { *at(r, 3 * ab.x) = xa0 + q0; *at(r, 3 * ab.x + 1) = xa1 + q1; *at(r, 3 * ab.x + 2) = xa2 + q2; }
          if (inB) { *at(r, 3 * ab.y) = xb0 - q0; *at(r, 3 * ab.y + 1) = xb1 - q1; *at(r, 3 * ab.y + 2) = xb2 - q2; }
        }
      }
    }
  }
  const double m = S.mass64[i];
  for (int c = 0; c < 3; c++) *at(3 * i + c, 3 * i + c) += m;
}

// Panel [k0, k0 + kb) of one band: rows k0 ... min(n, k0 + kb + kl) - 1 as a dense block in LDS (P[jj pld + i] = entry (k0 + i, k0 + jj),
// zero where the band stores nothing), factored column by column as k_lu_panel does (pivot search among the column's kl + 1 rows, swap of
// the whole panel row, scaling, rank-1 update). The block goes to D.panel as it stands (L11 / L21 of k_band_trsm / k_band_update); the
// panel's swaps are then undone on the multipliers, which go to the band with U. A flagged panel stores nothing. LDS = false: the block
// does not fit LDS and is worked on in global memory (D.panel's second block; the barriers order the workgroup's accesses to it).
template <int THREADS, bool LDS>
__global__ __launch_bounds__(THREADS) void k_band_panel(BandAdjWork D, int k0, int kb) {
  extern __shared__ __attribute__((aligned(16))) double Plds[];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  constexpr int NW = THREADS / 64;
  if (D.flag[blockIdx.x]) return;
  const int n = D.n, kl = D.kl, kv = 2 * D.kl, pld = D.pld;
  const size_t ldab = D.ldab;
  double *AB = D.AB + (size_t) blockIdx.x * ldab * n;
  const int m = min(n, k0 + kb + kl) - k0;             // rows of the panel
  double *Ps = D.panel + (size_t) blockIdx.x * 2 * kLuPanel * pld;
  double *P = Plds;
  if constexpr (!LDS) P = Ps + (size_t) kLuPanel * pld;
  __shared__ double sv[NW], urow[kLuPanel];
  __shared__ int si[NW], sp[kLuPanel];
  for (int q = tid; q < kb * m; q += THREADS) {
    const int jj = q / m, i = q - jj * m, d = i - jj;      // d = row - column
    P[jj * pld + i] = (d <= kl && -d <= kv) ? AB[(size_t) (k0 + jj) * ldab + (kv + d)] : 0.0;
  }
  __syncthreads();
  for (int jl = 0; jl < kb; jl++) {
    const int hi = min(jl + kl, m - 1);                // the column's last row
    double tv = -1.0;
    int tr = n;
    for (int i = jl + tid; i <= hi; i += THREADS) amax_merge(tv, tr, fabs(P[jl * pld + i]), k0 + i);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) amax_merge(tv, tr, __shfl_xor(tv, o, 64), __shfl_xor(tr, o, 64));
    if (lane == 0) { sv[wv] = tv; si[wv] = tr; }
    __syncthreads();
    double pv = sv[0];
    int p = si[0];
    for (int w = 1; w < NW; w++) amax_merge(pv, p, sv[w], si[w]);
    if (!(pv > 0.0) || !isfinite(pv) || p >= n) {      // singular or non-finite: this rollout takes the fall-back
      if (tid == 0) D.flag[blockIdx.x] = 1;
      return;
    }
    const int pl = p - k0;
    if (tid < kb) {
      double *q = P + tid * pld;
      const double a = q[jl], c = q[pl];
      q[jl] = c; q[pl] = a;
      urow[tid] = c;
    }
    if (tid == 0) sp[jl] = p;
    __syncthreads();
    const double inv = 1.0 / urow[jl];
    for (int i = jl + 1 + tid; i <= hi; i += THREADS) {
      const double l = P[jl * pld + i] * inv;
      P[jl * pld + i] = l;
      for (int jj = jl + 1; jj < kb; jj++) P[jj * pld + i] -= l * urow[jj];
    }
    __syncthreads();
  }
  for (int q = tid; q < kb * m; q += THREADS) { const int jj = q / m, i = q - jj * m; Ps[jj * pld + i] = P[jj * pld + i]; }
  if (tid < kb) D.piv[(size_t) blockIdx.x * D.npiv + k0 + tid] = sp[tid];
  __syncthreads();
  if (tid < kb) {                                      // column tid's multipliers back to the rows they were computed in
    double *q = P + tid * pld;
    for (int jj = kb - 1; jj > tid; jj--) {
      const int pl = sp[jj] - k0;
      if (pl != jj) { const double a = q[jj]; q[jj] = q[pl]; q[pl] = a; }
    }
  }
  __syncthreads();
  for (int q = tid; q < kb * m; q += THREADS) {
    const int jj = q / m, i = q - jj * m, d = i - jj;
    if (d <= kl && -d <= kv) AB[(size_t) (k0 + jj) * ldab + (kv + d)] = P[jj * pld + i];
  }
}

// Row swaps of panel [k0, k0 + kLuPanel) and U12 = L11^-1 A12 on the columns k0 + kLuPanel ... cend - 1 right of it: one thread per column.
// Rows above c - kv of column c are outside the band: zero before and after (a pivot row p <= j + kl ends at column j + kv).
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_band_trsm(BandAdjWork D, int k0, int cend) {
  const int tid = threadIdx.x;
  if (D.flag[blockIdx.y]) return;
  const int n = D.n, kv = 2 * D.kl, pld = D.pld;
  const size_t ldab = D.ldab;
  double *AB = D.AB + (size_t) blockIdx.y * ldab * n;
  const double *Ps = D.panel + (size_t) blockIdx.y * 2 * kLuPanel * pld;
  const int *piv = D.piv + (size_t) blockIdx.y * D.npiv;
  __shared__ double L[kLuPanel][kLuPanel + 1];      // L[jj][ii] = entry (k0 + ii, k0 + jj), swapped rows
  __shared__ double xs[kLuPanel][kLuPanel + 1];     // the right-hand sides of the window's last columns, one column each
  __shared__ int sp[kLuPanel];
  for (int q = tid; q < kLuPanel * kLuPanel; q += THREADS) { const int jj = q / kLuPanel, ii = q % kLuPanel; L[jj][ii] = Ps[jj * pld + ii]; }
  if (tid < kLuPanel) sp[tid] = piv[k0 + tid];
  __syncthreads();
  const int c = k0 + kLuPanel + blockIdx.x * THREADS + tid;
  if (c >= cend) return;
  double *q = AB + (size_t) c * ldab + (kv - c);    // q[r] = entry (r, c), r in [c - kv, c + kl]
  const int j0 = max(0, c - kv - k0);               // first panel row inside the band of column c
  for (int jj = j0; jj < kLuPanel; jj++) {
    const int p = sp[jj];
    if (p != k0 + jj) { const double a = q[k0 + jj]; q[k0 + jj] = q[p]; q[p] = a; }
  }
  if (j0 > 0) {       // the window's last kLuPanel - 1 columns (rows above j0 are zero and not stored): rolled loops on an LDS column
    const int t = j0 - 1;                           // c - kv - k0 - 1: one column of xs per such thread
    for (int ii = j0; ii < kLuPanel; ii++) xs[ii][t] = q[k0 + ii];
    for (int jj = j0; jj < kLuPanel; jj++) {
      const double xj = xs[jj][t];
      for (int ii = jj + 1; ii < kLuPanel; ii++) xs[ii][t] -= L[jj][ii] * xj;
    }
    for (int ii = j0; ii < kLuPanel; ii++) q[k0 + ii] = xs[ii][t];
    return;
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

// Trailing update A22 -= L21 U12 for panel [k0, k0 + kLuPanel) on rows k1 ... rend - 1, columns k1 ... cend - 1 (k1 = k0 + kLuPanel): one
// 64 x 64 tile of one band per workgroup, 4 x 4 entries per thread. The whole window lies inside the band (row - column < kl,
// column - row < kl + ku).
constexpr int kBandTile = 64;
__global__ __launch_bounds__(256) void k_band_update(BandAdjWork D, int k0, int rend, int cend, int tiles) {
  const int tid = threadIdx.x;
  if (D.flag[blockIdx.y]) return;
  const int n = D.n, kv = 2 * D.kl, pld = D.pld;
  const size_t ldab = D.ldab;
  double *AB = D.AB + (size_t) blockIdx.y * ldab * n;
  const double *Ps = D.panel + (size_t) blockIdx.y * 2 * kLuPanel * pld;
  const int k1 = k0 + kLuPanel;
  const int i0 = k1 + (blockIdx.x % tiles) * kBandTile, j0 = k1 + (blockIdx.x / tiles) * kBandTile;
  __shared__ double Ls[kLuPanel][kBandTile], Us[kLuPanel][kBandTile + 1];
  for (int q = tid; q < kLuPanel * kBandTile; q += 256) {
    const int k = q / kBandTile, ii = q % kBandTile;
    Ls[k][ii] = (i0 + ii < rend) ? Ps[k * pld + (i0 + ii - k0)] : 0.0;
    const int jj = q / kLuPanel, kk = q % kLuPanel, c = j0 + jj;
    Us[kk][jj] = (c < cend && c - (k0 + kk) <= kv) ? AB[(size_t) c * ldab + (kv + k0 + kk - c)] : 0.0;
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
    if (j >= cend) continue;
#pragma unroll
    for (int a = 0; a < 4; a++) {
      const int i = i0 + tx + 16 * a;
      if (i < rend) AB[(size_t) j * ldab + (kv + i - j)] -= acc[a][c];
    }
  }
}

// d = K^-1 r with the band factors of this rollout, in LDS (bv: n doubles in interleaved order, blk: band_blk_doubles(kl, cols) doubles);
// every thread of the workgroup. Forward, per `cols` columns: their multipliers to blk, then one wave column by column (the swap, then the
// column's kl rows: swaps and eliminations interleave, LINPACK-style). Backward as lu_substitute: the upper diagonal block (one wave), then
// the kl + ku rows above it.
template <int THREADS>
__device__ __forceinline__ void band_substitute(const double *__restrict__ AB, const int *__restrict__ piv, int n, int kl, size_t ldab, int cols, double *bv, double *blk) {
  const int tid = threadIdx.x, kv = 2 * kl;
  for (int k0 = 0; k0 < n && kl > 0; k0 += cols) {
    const int kb = min(cols, n - k0);
    for (int q = tid; q < kb * kl; q += THREADS) {
      const int jj = q / kl, d = q - jj * kl, j = k0 + jj;          // entry (j + 1 + d, j)
      blk[jj * kl + d] = (j + 1 + d < n) ? AB[(size_t) j * ldab + (kv + 1 + d)] : 0.0;
    }
    __syncthreads();
    if (tid < 64) {
      for (int jj = 0; jj < kb; jj++) {
        const int j = k0 + jj, p = piv[j], cnt = min(kl, n - 1 - j);
        if (tid == 0 && p != j) { const double a = bv[j]; bv[j] = bv[p]; bv[p] = a; }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        const double x = bv[j];
        for (int d = tid; d < cnt; d += 64) bv[j + 1 + d] -= blk[jj * kl + d] * x;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      }
    }
    __syncthreads();
  }
  for (int k0 = (n - 1) / kLuPanel * kLuPanel; k0 >= 0; k0 -= kLuPanel) {
    const int kb = min(kLuPanel, n - k0);
    for (int q = tid; q < kb * kb; q += THREADS) {
      const int jj = q / kb, ii = q % kb, d = ii - jj;
      blk[jj * kLuPanel + ii] = (d <= kl && -d <= kv) ? AB[(size_t) (k0 + jj) * ldab + (kv + d)] : 0.0;
    }
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
    for (int i = max(0, k0 - kv) + tid; i < k0; i += THREADS) {
      double s = 0.0;
      for (int jj = 0; jj < kb; jj++) {
        const int c = k0 + jj;
        if (c - i <= kv) s += AB[(size_t) c * ldab + (kv + i - c)] * bv[c];
      }
      bv[i] -= s;
    }
    __syncthreads();
  }
}

// The adjoint step of one rollout with the band factors (k_adjoint_dense_step's mode-3 counterpart; one step per launch)
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_adjoint_band_step(const DevSystem *__restrict__ Sp, DevWork W, BwdArgs A, BandAdjWork D, int b0) {
  const DevSystem &S = *Sp;
  extern __shared__ __attribute__((aligned(16))) double dyn[];      // bv [n rounded to 16], blk [band_blk_doubles(kl, sub_cols)]
  __shared__ double red[3 * (THREADS / 64)];
  const int b = b0 + blockIdx.x, tid = threadIdx.x;
  const int N = S.N, n = 3 * N;
  double *bv = dyn, *blk = dyn + band_round16(n);
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
    used_direct = 3;
    const double stop = (double) A.rel_tol * (double) A.rel_tol * gnorm * gnorm;
    const double *AB = D.AB + (size_t) blockIdx.x * D.ldab * n;
    const int *piv = D.piv + (size_t) blockIdx.x * D.npiv;
    // r = g (u = 0)
    for (int i = tid; i < N; i += THREADS) st3d(W64.r, i, N, tod(ld3(gx, i, N) * gscale));
    double rr_true = gnorm * gnorm;
    status = 0;
    const bool factored = D.flag[blockIdx.x] == 0;
    __syncthreads();
    for (; factored && cycles < kBandRefine; ) {
      for (int q = tid; q < n; q += THREADS) { const int i = q / 3, c = q - 3 * i; bv[q] = W64.r[c * N + i]; }      // planar -> interleaved
      __syncthreads();
      band_substitute<THREADS>(AB, piv, n, D.kl, (size_t) D.ldab, D.sub_cols, bv, blk);
      for (int q = tid; q < n; q += THREADS) { const int i = q / 3, c = q - 3 * i; W64.u[c * N + i] += bv[q]; }
      __syncthreads();
      cycles++;
      const double rr_new = residual64<THREADS>(S, C64, tm, W64, gx, gscale).rr;
      if (!(rr_new < rr_true)) {               // no progress (NaN-safe): take the correction back, the fall-back goes on from there
        for (int q = tid; q < n; q += THREADS) { const int i = q / 3, c = q - 3 * i; W64.u[c * N + i] -= bv[q]; }
        __syncthreads();
        rr_true = residual64<THREADS>(S, C64, tm, W64, gx, gscale).rr;
        break;
      }
      rr_true = rr_new;
      if (rr_true <= stop) { status = 1; break; }
    }
    if (status != 1) {
      // ---- fp64 BiCGSTAB on the same operator from (u, r), as in k_adjoint_dense_step ----
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

void launch_band_assemble(const DevSystem &S, const BwdArgs &A, double *x64, const BandAdjWork &D, int b0, int nb, hipStream_t st) {
  DenseAdjWork P{};
  P.pm = D.pm; P.sg = D.sg;
  launch_dense_prep(S, A, x64, P, b0, nb, st);
  hipLaunchKernelGGL(k_band_assemble<64>, dim3((S.N + 63) / 64, nb), dim3(64), 0, st, S.self_dev, A, (const double *) x64, D, b0);
}

hipError_t launch_band_factor(const BandAdjWork &D, int nb, hipStream_t st, int *launches) {
  const int n = D.n, kl = D.kl, kv = 2 * D.kl;
  const bool in_lds = band_panel_in_lds(kl);
  const size_t lds = in_lds ? sizeof(double) * (size_t) kLuPanel * D.pld : 0;
  if (in_lds) {
    const hipError_t e = ensure_dynamic_lds<k_band_panel<1024, true>>(lds);
    if (e != hipSuccess) return e;
  }
  int count = 0;
  for (int k0 = 0; k0 < n; k0 += kLuPanel) {
    const int kb = std::min(kLuPanel, n - k0), k1 = k0 + kb;
    if (in_lds) hipLaunchKernelGGL((k_band_panel<1024, true>), dim3(nb), dim3(1024), lds, st, D, k0, kb);
    else hipLaunchKernelGGL((k_band_panel<1024, false>), dim3(nb), dim3(1024), 0, st, D, k0, kb);
    count++;
    const int cend = std::min(n, k1 + kv), rend = std::min(n, k1 + kl);
    if (cend <= k1) continue;
    hipLaunchKernelGGL(k_band_trsm<256>, dim3((cend - k1 + 255) / 256, nb), dim3(256), 0, st, D, k0, cend);
    count++;
    if (rend <= k1) continue;
    const int tiles = (rend - k1 + kBandTile - 1) / kBandTile, ctiles = (cend - k1 + kBandTile - 1) / kBandTile;
    hipLaunchKernelGGL(k_band_update, dim3(tiles * ctiles, nb), dim3(256), 0, st, D, k0, rend, cend, tiles);
    count++;
  }
  if (launches) *launches += count;
  return hipSuccess;
}

hipError_t launch_band_adjoint_step(const DevSystem &S, const DevWork &W, const BwdArgs &A, const BandAdjWork &D, int b0, int nb, hipStream_t st) {
  if (D.sub_cols < 1) return hipErrorInvalidValue;
  const size_t lds = (size_t) band_lds_bytes(S.N, D.kl, D.sub_cols);
  const hipError_t e = ensure_dynamic_lds<k_adjoint_band_step<1024>>(lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_adjoint_band_step<1024>, dim3(nb), dim3(1024), lds, st, S.self_dev, W, A, D, b0);
  return hipSuccess;
}

}  // namespace dc
