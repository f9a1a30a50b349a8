// Test harness (CPU): the byte-offset layout of the packet matrix (dc_packets.h, HostPackets::to_offsets) decoded back and compared with
// the first layout's decode and with the CSR of the scaled matrix.
//   g++ -O1 -std=c++17 -I diffcloth_amd/csrc tests/native/packet_offsets_check.cpp diffcloth_amd/csrc/{dc_system,dc_windows,dc_packets,dc_dense,dc_tables}.cpp -o packet_offsets_check
//   packet_offsets_check [mesh.bin ...]      mesh.bin = int32 N, int32 T, double pos[3 N], int32 tri[3 T]
// Always checks the 100 x 100 grid (the headline's mesh); every mesh file given is renumbered (RCM) when its bandwidth needs it, as dc_build does.
// Prints one line per check and exits non-zero on the first failure (driven by tests/test_packet_offsets.py).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "dc_packets.h"
#include "dc_system.h"
#include "dc_tables.h"

using namespace dc;

static void fail(const std::string &what) { std::printf("FAIL %s\n", what.c_str()); std::exit(1); }

struct Entry { int col; int bits; bool pad; };

// per-row entries of the first layout, in the order the kernel consumes them
static std::vector<std::vector<Entry>> decode_deltas(const HostPackets &P, int rows) {
  std::vector<std::vector<Entry>> out(rows);
  for (int r = 0; r < rows; r++) {
    const int ch = r / 64, l = r % 64;
    for (int s = 0; s < P.pk_n[ch]; s++) {
      const int *q = &P.pk[4 * ((size_t) P.pk_ptr[ch] + (size_t) s * 64 + l)];
      for (int k = 0; k < 3; k++) {
        const int d = (q[3] >> (10 * k)) & 1023;
        out[r].push_back({r + d - 512, q[k], q[k] == 0 && d == 512});
      }
    }
  }
  return out;
}

// the same from the byte-offset layout, with the checks only that layout needs
static std::vector<std::vector<Entry>> decode_offsets(const HostPackets &Q, int rows, const std::string &tag) {
  std::vector<std::vector<Entry>> out(rows);
  size_t at = 0;
  for (int ch = 0; ch < rows / 64; ch++) {
    if (Q.pk_n[ch] % 4 != 0 || Q.pk_n[ch] < 4) fail(tag + ": rows must keep a multiple of 4 packets");
    if ((size_t) Q.pk_ptr[ch] != at) fail(tag + ": chunks must lie back to back, pk_ptr in 16-byte units");
    at += (size_t) kPkOfsBatchInt4 * (Q.pk_n[ch] / 4);
  }
  if (Q.pk.size() != 4 * at) fail(tag + ": stream length must be 6 bytes per stored non-zero");
  for (int r = 0; r < rows; r++) {
    const int ch = r / 64, l = r % 64;
    for (int t = 0; t < Q.pk_n[ch] / 4; t++) {
      const int *b = &Q.pk[4 * ((size_t) Q.pk_ptr[ch] + (size_t) kPkOfsBatchInt4 * t)];
      for (int n = 0; n < 12; n++) {
        const int bits = b[4 * (32 + 64 * (n / 4) + l) + n % 4];
        const unsigned w = (unsigned) (n < 8 ? b[4 * (32 + 64 * 3 + l) + n / 2] : b[2 * l + (n - 8) / 2]);
        const unsigned o = (n & 1) ? w >> 16 : w & 0xffffu;       // what the kernel's add selects
        if (o % 8 != 0 || o < 8 || o > 8 * 1023) fail(tag + ": offset field is not 8 d with d in [1, 1023]");
        const int col = r + (int) (o / 8) - 512;
        if (col < 0 || col >= rows) fail(tag + ": offset points outside the direction array");
        const bool pad = bits == 0 && o == 8 * 512;
        out[r].push_back({col, bits, pad});
      }
    }
  }
  return out;
}

static void check(const HostSystem &H, const std::string &tag) {
  HostPackets P;
  if (!P.build(H)) fail(tag + ": packet build refused");
  HostPackets Q = P;
  Q.to_offsets();
  const int rows = P.threads * P.vpt;
  if (!Q.ofs || P.ofs || Q.pk_n != P.pk_n || Q.sq_dinv != P.sq_dinv || Q.vpt != P.vpt || Q.threads != P.threads) fail(tag + ": to_offsets changed more than the stream");
  const auto a = decode_deltas(P, rows), b = decode_offsets(Q, rows, tag);
  std::vector<double> sq(H.N, 0.0);          // D^-1/2 as the packer forms it: the square root of the fp32 preconditioner entry
  for (int r = 0; r < H.N; r++)
    for (int q = H.P_ptr[r]; q < H.P_ptr[r + 1]; q++) if (H.P_col[q] == r) sq[r] = std::sqrt((double) (float) (1.0 / H.P_val[q]));
  size_t nnz = 0, wide = 0;
  for (int r = 0; r < rows; r++) {
    if (a[r].size() != b[r].size()) fail(tag + ": entries per row");
    for (size_t k = 0; k < a[r].size(); k++)
      if (a[r][k].col != b[r][k].col || a[r][k].bits != b[r][k].bits || a[r][k].pad != b[r][k].pad) fail(tag + ": entry differs from the first layout's, or its place in the row does");
    // against the CSR: the non-padding entries are the row's off-diagonals in CSR order, value as the packer scales it
    size_t k = 0;
    if (r < H.N)
      for (int q = H.P_ptr[r]; q < H.P_ptr[r + 1]; q++) {
        const int col = H.P_col[q];
        if (col == r) continue;
        if (k >= b[r].size() || b[r][k].pad) fail(tag + ": a CSR entry is missing");
        const float want = (float) (H.P_val[q] * sq[r] * sq[col]);
        int wb;
        std::memcpy(&wb, &want, 4);
        if (b[r][k].col != col || b[r][k].bits != wb) fail(tag + ": (row, column, value) differs from the CSR's");
        k++; nnz++;
      }
    if (k > 12) wide++;
    for (; k < b[r].size(); k++) if (!b[r][k].pad) fail(tag + ": entries behind the row's last non-zero must be padding");
  }
  std::printf("ok %s N=%d rows=%d off-diagonals=%zu rows wider than one batch=%zu stream %zu -> %zu bytes\n", tag.c_str(), H.N, rows, nnz, wide, 4 * P.pk.size(), 4 * Q.pk.size());
}

static void grid(int nx, int ny, std::vector<double> &pos, std::vector<int> &tri) {
  pos.assign(3 * (size_t) nx * ny, 0.0);
  for (int a = 0; a < ny; a++)
    for (int b = 0; b < nx; b++) { pos[3 * (a * nx + b)] = 0.05 * b; pos[3 * (a * nx + b) + 1] = 0.05 * a; }
  tri.clear();
  for (int a = 0; a + 1 < ny; a++)
    for (int b = 0; b + 1 < nx; b++) {
      const int v00 = a * nx + b, v01 = v00 + 1, v10 = v00 + nx, v11 = v10 + 1;
      tri.insert(tri.end(), {v00, v01, v11});
      tri.insert(tri.end(), {v00, v11, v10});
    }
}

static void build(HostSystem &H, int N, const std::vector<double> &pos, const std::vector<int> &tri, const std::string &tag) {
  if (!H.set_mesh(N, pos.data(), (int) tri.size() / 3, tri.data())) fail(tag + ": set_mesh");
  if (!H.build_numerics(1.0 / 120, 0.3, 200.0, 0.02, 1e4)) fail(tag + ": build_numerics");
}

int main(int argc, char **argv) {
  std::vector<double> pos;
  std::vector<int> tri;
  {
    grid(100, 100, pos, tri);
    HostSystem H;
    build(H, 100 * 100, pos, tri, "grid 100 x 100");
    check(H, "grid 100 x 100");
    // the plan's decision: byte offsets exactly where the kernel that runs holds the direction as halves (512 x 20 rows with element windows)
    dc_params prm;
    std::memset(&prm, 0, sizeof(prm));
    TableSwitches sw;
    HostTables T;
    T.build(H, prm, sw);
    if (!T.pk_ok || T.pk_vpt != 20 || !T.win_ok || !T.pk_ofs || !T.pk.ofs) fail("plan: the 10 000-vertex grid must get the byte-offset layout");
    sw.pk_ofs = false;
    T.build(H, prm, sw);
    if (T.pk_ofs || T.pk.ofs) fail("plan: DC_PK_OFS=0 must keep the first layout");
    sw.pk_ofs = true; sw.pk_h16 = false;
    T.build(H, prm, sw);
    if (T.pk_ofs || T.pk.ofs) fail("plan: the fp32-plane instance reads the first layout");
    sw.pk_h16 = true; sw.windows = false;
    T.build(H, prm, sw);
    if (T.pk_ofs || T.pk.ofs) fail("plan: without element windows the fp32-plane instance runs");
    grid(60, 40, pos, tri);
    HostSystem Hs;
    build(Hs, 60 * 40, pos, tri, "grid 60 x 40");
    sw = TableSwitches();
    T.build(Hs, prm, sw);
    if (!T.pk_ok || T.pk_ofs || T.pk.ofs) fail("plan: a mesh of fewer rows per thread keeps the first layout");
    std::printf("ok plan decisions\n");
  }
  for (int a = 1; a < argc; a++) {
    FILE *f = std::fopen(argv[a], "rb");
    int hdr[2];
    if (!f || std::fread(hdr, 4, 2, f) != 2) fail(std::string(argv[a]) + ": cannot read");
    const int N = hdr[0], T = hdr[1];
    pos.resize(3 * (size_t) N); tri.resize(3 * (size_t) T);
    if (std::fread(pos.data(), 8, pos.size(), f) != pos.size() || std::fread(tri.data(), 4, tri.size(), f) != tri.size()) fail(std::string(argv[a]) + ": short file");
    std::fclose(f);
    if (mesh_bandwidth(T, tri.data()) > 511) {        // as dc_build: reverse Cuthill-McKee
      const std::vector<int> order = rcm_order(N, T, tri.data());
      std::vector<int> inv(N);
      for (int k = 0; k < N; k++) inv[order[k]] = k;
      std::vector<double> p2(pos.size());
      for (int k = 0; k < N; k++) for (int d = 0; d < 3; d++) p2[3 * (size_t) k + d] = pos[3 * (size_t) order[k] + d];
      for (int &v : tri) v = inv[v];
      pos.swap(p2);
    }
    HostSystem H;
    build(H, N, pos, tri, argv[a]);
    check(H, "mesh " + std::to_string(a));
  }
  std::printf("ALL OK\n");
  return 0;
}
