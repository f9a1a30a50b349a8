#include "dc_tables.h"
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace dc {

static float low_part(double v) { return (float) (v - (double) (float) v); }

void HostTables::build(const HostSystem &H, const dc_params &p, const TableSwitches &sw) {
  *this = HostTables();
  const int N = H.N, T = H.T, E = H.E, Af = (int) H.att_vertex.size();
  tri_v.resize(3 * (size_t) T); tri_D64.resize(4 * (size_t) T); tri_Dlo.resize(4 * (size_t) T);
  for (int t = 0; t < T; t++) {
    for (int k = 0; k < 3; k++) tri_v[(size_t) k * T + t] = H.tri[3 * t + k];
    for (int k = 0; k < 4; k++) { tri_D64[(size_t) k * T + t] = H.tri_D[4 * (size_t) t + k]; tri_Dlo[4 * (size_t) t + k] = low_part(H.tri_D[4 * (size_t) t + k]); }
  }
  bend_v.resize(4 * (size_t) E); bend_nw.resize(2 * (size_t) E); bend_w64.resize(4 * (size_t) E); bend_nw64.resize(2 * (size_t) E); bend_lo.resize(4 * (size_t) E);
  for (int e = 0; e < E; e++) {
    for (int k = 0; k < 4; k++) { bend_v[(size_t) k * E + e] = H.bend_v[4 * e + k]; bend_w64[(size_t) k * E + e] = H.bend_w[4 * (size_t) e + k]; }
    bend_nw[2 * e] = (float) H.bend_n[e]; bend_nw[2 * e + 1] = (float) H.bend_w2[e];
    bend_nw64[e] = H.bend_n[e]; bend_nw64[(size_t) E + e] = H.bend_w2[e];
    for (int k = 1; k < 4; k++) bend_lo[4 * (size_t) e + k - 1] = low_part(H.bend_w[4 * (size_t) e + k]);
    bend_lo[4 * (size_t) e + 3] = low_part(H.bend_n[e]);
  }
  dinv.resize(N);
  std::vector<double> diag(N, 0.0);
  for (int r = 0; r < N; r++)
    for (int k = H.P_ptr[r]; k < H.P_ptr[r + 1]; k++) {
      bandwidth = std::max(bandwidth, std::abs(H.P_col[k] - r));
      if (H.P_col[k] == r) diag[r] = H.P_val[k];
    }
  for (int r = 0; r < N; r++) dinv[r] = (float) (1.0 / diag[r]);
  att_of_vertex.assign(N, -1);
  for (int a = 0; a < Af; a++) att_of_vertex[H.att_vertex[a]] = a;
  {
    double mr = H.radii.empty() ? 0.0 : H.radii[0];
    for (double r : H.radii) mr = std::max(mr, r);
    max_radii = (float) mr;
    // capacity of the per-rollout contact list: the caller's, or sized from the mesh (a fold brings every vertex of the upper
    // layer into contact with one of the lower: ~N/2 pairs). Slots of the working set are 16-bit: at most 16000 pairs.
    self_cap = std::min(p.max_self_contacts > 0 ? p.max_self_contacts : std::max(2048, N), 16000);
    self_lds = sw.self_lds ? 1 : 0;
  }
  {  // wave-sliced ELL copy of P for the LDS-resident PCG
    const int nchunks = (N + 63) / 64;
    ell_ptr.resize(nchunks); ell_w.resize(nchunks);
    for (int ch = 0; ch < nchunks; ch++) {
      int w = 0;
      for (int r = 64 * ch; r < std::min(N, 64 * ch + 64); r++) w = std::max(w, H.P_ptr[r + 1] - H.P_ptr[r]);
      ell_ptr[ch] = (int) (ell.size() / 2); ell_w[ch] = w;
      ell.resize(ell.size() + (size_t) 2 * 64 * w);
      for (int s = 0; s < w; s++)
        for (int l = 0; l < 64; l++) {
          const int r = 64 * ch + l;
          int col = std::min(r, N - 1);
          float val = 0.f;
          if (r < N && H.P_ptr[r] + s < H.P_ptr[r + 1]) { col = H.P_col[H.P_ptr[r] + s]; val = (float) H.P_val[H.P_ptr[r] + s]; }
          int bits;
          std::memcpy(&bits, &val, sizeof(int));
          const size_t o = 2 * ((size_t) ell_ptr[ch] + (size_t) s * 64 + l);
          ell[o] = col; ell[o + 1] = bits;
        }
    }
  }
  // element windows: the local step and the adjoint's element pass run inside LDS
  if (sw.windows && win.build(H, kWindowLdsBudget, sw.bend_rows, p.time_step)) { win_ok = 1; nwin = win.nwin; bend_rows = win.rows ? 1 : 0; }
  // packet-ELL copy of the scaled matrix for dc_forward_pk.hip (dc_packets.h)
  if (pk.build(H, sw.pk_threads)) {
    pk_ok = 1; pk_vpt = pk.vpt; pk_threads = pk.threads;
    // the instances that hold the search direction as halves (the shapes of kPkShapes that have one, with the element windows) gather by
    // byte offsets
    if (sw.pk_ofs && sw.pk_h16 && win_ok && kPkShapes[pk.shape].xl_h16 >= 0) { pk.to_offsets(); pk_ofs = 1; }
  } else {
    // no packet tables (matrix bandwidth beyond the +-511 of their column deltas: the reference's 17 562-vertex dress, 647 after
    // renumbering): the scaling D^-1/2 alone, for the coarse level of the ADJOINT's preconditioner (dc_adjoint64.h), which such a mesh needs
    sq_dinv.assign((size_t) round64(N), 0.f);
    for (int r = 0; r < N; r++) if (diag[r] != 0.0) sq_dinv[r] = (float) (1.0 / std::sqrt(diag[r]));
  }
  // irregular garments: the 16 lowest eigenvectors of the scaled matrix as a deflation space of the forward solve (dc_deflate.h)
  defl_rows = win_ok ? (pk_ok ? pk_threads * pk_vpt : round64(N)) : 0;
  // small meshes: explicit inverse of the scaled matrix (dc_dense.h) for the forward global step
  if (pk_ok && win_ok && dense.build(H, sw.dense_max_n)) dense_ld = dense.ld;
}

void HostTables::set_deflation(bool built, const TableSwitches &sw) {
  // (the deflated FORWARD kernels exist for the shapes kPkShapes marks: meshes of more than 1536 vertices, dc_forward_pk_defl.hip; smaller meshes
  //  solve their forward step with the explicit inverse and use the space for the adjoint's coarse level only; a mesh without packet tables
  //  runs the global-memory kernel, which projects too — dc_devlib.h: deflate_global)
  fwd_defl = (built && (!pk_ok || kPkShapes[pk.shape].defl)) ? 1 : 0;
  defl_built = built;
  adj_coarse = (built && sw.adj_coarse) ? 1 : 0;
  // The template layout (dc_packets.h) for the plain halves instance: the deflated instances use the direction's LDS as float scratch and keep
  // the byte offsets. The guards must fit the CU's LDS next to everything pk_lds_bytes counts (with the inlined detection, the larger request)
  // and the kernel's static LDS, and the kernel zeroes them with one 8-byte store per thread.
  if (sw.pk_tpl && pk_ofs && !pk_tpl && !fwd_defl) {
    HostPackets t = pk;
    if (t.to_template()) {
      const PkShape &s = kPkShapes[pk.shape];
      const int guard = pk_tpl_guard_bytes(t.tpl_reach);
      const size_t lds = pk_lds_bytes(s.threads, s.vpt, s.xl_h16, true, false, 0, win_ok != 0, (int) win.lds_bytes, true, guard);
      const size_t static_lds = sizeof(double) * 3 * (size_t) (s.threads / 64);      // the kernel's reduction scratch: red, red2
      if (lds + std::max(static_lds, (size_t) kLdsReserveBytes) <= (size_t) kLdsLimitBytes && 2 * (guard / 8) <= s.threads) {
        pk = std::move(t);
        pk_tpl = 1; pk_guard_bytes = guard;
      }
    }
  }
}

PlanFacts HostTables::facts(int N) const {
  PlanFacts f;
  f.N = N;
  f.pk_ok = pk_ok != 0; f.pk_threads = pk_threads; f.pk_vpt = pk_vpt; f.win_ok = win_ok != 0; f.pk_ofs = pk_ofs != 0; f.pk_tpl = pk_tpl != 0;
  f.fwd_defl = fwd_defl != 0; f.adj_coarse = adj_coarse != 0; f.defl_space = defl_built; f.dense_inv = dense_ld != 0;
  f.win_lds_bytes = win_ok ? (int) win.lds_bytes : 0;
  return f;
}

}  // namespace dc
