// Test harness (CPU): the template layout of the packet matrix (dc_packets.h, HostPackets::to_template — values only under one set of at most
// twelve column offsets for the whole matrix) decoded back and compared with the byte-offset layout's decode and with the CSR of the scaled
// matrix; the table plan's decision (dc_tables.h: HostTables::set_deflation) on the headline's grid and on the meshes that must fall back.
//   g++ -O1 -std=c++17 -I diffcloth_amd/csrc tests/native/packet_template_check.cpp diffcloth_amd/csrc/{dc_system,dc_windows,dc_packets,dc_dense,dc_tables}.cpp -o packet_template_check
//   packet_template_check [slope96.bin dress.bin]      mesh.bin = int32 N, int32 T, double pos[3 N], int32 tri[3 T]
// Always checks the 100 x 100 grid in the headline's triangulation. With the two mesh files: the 96 x 96 slope fabric (template or fall-back,
// whichever the rule computed here from the CSR says) and the 7 742-vertex dress (rows of more than one batch: falls back).
// Prints one line per check and exits non-zero on the first failure (driven by tests/test_packet_template.py).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>
#include "dc_packets.h"
#include "dc_system.h"
#include "dc_tables.h"

using namespace dc;

static void fail(const std::string &what) { std::printf("FAIL %s\n", what.c_str()); std::exit(1); }

struct Entry { int col; int bits; };

// per-row entries of the byte-offset layout in the order the kernel consumes them, padding (value 0 on the row itself) dropped
static std::vector<std::vector<Entry>> decode_offsets(const HostPackets &Q, int rows) {
  std::vector<std::vector<Entry>> out(rows);
  for (int r = 0; r < rows; r++) {
    const int ch = r / 64, l = r % 64;
    for (int t = 0; t < Q.pk_n[ch] / 4; t++) {
      const int *b = &Q.pk[4 * ((size_t) Q.pk_ptr[ch] + (size_t) kPkOfsBatchInt4 * t)];
      for (int n = 0; n < 12; n++) {
        const int bits = b[4 * (32 + 64 * (n / 4) + l) + n % 4];
        const unsigned w = (unsigned) (n < 8 ? b[4 * (32 + 64 * 3 + l) + n / 2] : b[2 * l + (n - 8) / 2]);
        const unsigned o = (n & 1) ? w >> 16 : w & 0xffffu;
        if (o == 8 * 512 && bits == 0) continue;
        out[r].push_back({r + (int) (o / 8) - 512, bits});
      }
    }
  }
  return out;
}

// the rule, from the CSR alone: at most 12 distinct (column - row) over the off-diagonals and no row of more than 12 of them
static bool rule_has_template(const HostSystem &H, std::set<int> &offs) {
  offs.clear();
  bool wide = false;
  for (int r = 0; r < H.N; r++) {
    int n = 0;
    for (int q = H.P_ptr[r]; q < H.P_ptr[r + 1]; q++) if (H.P_col[q] != r) { offs.insert(H.P_col[q] - r); n++; }
    wide = wide || n > 12;
  }
  return !wide && offs.size() <= 12;
}

// the template stream of T (a plan that took the template) against the CSR and against the byte-offset stream of the same matrix
static void check_stream(const HostSystem &H, const HostTables &T, const std::string &tag) {
  const HostPackets &Q = T.pk;
  if (!Q.ok || !Q.ofs || !Q.tpl) fail(tag + ": not a template stream");
  HostPackets P;
  if (!P.build(H)) fail(tag + ": packet build refused");
  P.to_offsets();
  const int rows = P.threads * P.vpt;
  if (Q.pk_n != P.pk_n || Q.sq_dinv != P.sq_dinv || Q.vpt != P.vpt || Q.threads != P.threads || Q.shape != P.shape) fail(tag + ": to_template changed more than the stream");
  if (Q.pk.size() != (size_t) 4 * kPkTplBatchInt4 * (rows / 64)) fail(tag + ": stream length must be 48 bytes per row");
  for (int ch = 0; ch < rows / 64; ch++) if (Q.pk_ptr[ch] != kPkTplBatchInt4 * ch) fail(tag + ": chunks must lie kPkTplBatchInt4 apart");
  int reach = 0;
  for (int j = 0; j < kPkTplSlots; j++) {
    reach = std::max(reach, std::abs(Q.tpl_off[j]));
    if (j > 0 && Q.tpl_off[j] != 0 && Q.tpl_off[j] <= Q.tpl_off[j - 1]) fail(tag + ": template offsets must ascend");
    if (Q.tpl_off[j] == 0 && j + 1 < kPkTplSlots && Q.tpl_off[j + 1] != 0) fail(tag + ": unused slots stand last");
  }
  if (reach != Q.tpl_reach) fail(tag + ": tpl_reach is not max |offset|");
  const auto ref = decode_offsets(P, rows);
  std::vector<double> sq(H.N, 0.0);          // D^-1/2 as the packer forms it: the square root of the fp32 preconditioner entry
  for (int r = 0; r < H.N; r++)
    for (int q = H.P_ptr[r]; q < H.P_ptr[r + 1]; q++) if (H.P_col[q] == r) sq[r] = std::sqrt((double) (float) (1.0 / H.P_val[q]));
  size_t nnz = 0, zeros = 0, outside = 0;
  const int guard_rows = pk_tpl_guard_bytes(Q.tpl_reach) / 8;
  for (int r = 0; r < rows; r++) {
    const int ch = r / 64, l = r % 64;
    std::vector<Entry> got;                   // the slots that hold a value, in slot order = the order of the kernel's products
    for (int j = 0; j < kPkTplSlots; j++) {
      const int bits = Q.pk[4 * ((size_t) Q.pk_ptr[ch] + 64 * (j / 4) + l) + j % 4];
      const int col = r + Q.tpl_off[j];
      if (col < -guard_rows || col >= rows + guard_rows) fail(tag + ": a slot points outside the guards");
      if (col < 0 || col >= rows) outside++;
      if (bits == 0) { zeros++; continue; }
      if (Q.tpl_off[j] == 0) fail(tag + ": an unused slot holds a value");
      got.push_back({col, bits});
    }
    // against the byte-offset layout, entry by entry (a stored non-zero whose value is exactly 0 would be dropped from both sides here)
    size_t k = 0;
    for (const Entry &e : ref[r]) {
      if (e.bits == 0) continue;
      if (k >= got.size() || got[k].col != e.col || got[k].bits != e.bits) fail(tag + ": entry differs from the byte-offset layout's, or its place in the row does");
      k++;
    }
    if (k != got.size()) fail(tag + ": a slot holds a value the byte-offset layout lacks");
    // against the CSR: (row, column, value) in CSR order, value as the packer scales it; zeros only where the row lacks the neighbour
    k = 0;
    if (r < H.N)
      for (int q = H.P_ptr[r]; q < H.P_ptr[r + 1]; q++) {
        const int col = H.P_col[q];
        if (col == r) continue;
        const float want = (float) (H.P_val[q] * sq[r] * sq[col]);
        int wb;
        std::memcpy(&wb, &want, 4);
        if (wb == 0) continue;
        if (k >= got.size() || got[k].col != col || got[k].bits != wb) fail(tag + ": (row, column, value) differs from the CSR's");
        k++; nnz++;
      }
    if (k != got.size()) fail(tag + ": a slot holds a value where the row has no neighbour");
  }
  std::printf("ok %s N=%d rows=%d off-diagonals=%zu zero slots=%zu (%zu of them outside the matrix) reach=%d stream %zu -> %zu bytes\n", tag.c_str(), H.N, rows, nnz, zeros,
              outside, Q.tpl_reach, 4 * P.pk.size(), 4 * Q.pk.size());
}

// the headline's triangulation (workloads.grid_cloth): per cell (upper right, up, this) and (left, this, up)
static void bench_grid(int nx, int ny, std::vector<double> &pos, std::vector<int> &tri) {
  pos.assign(3 * (size_t) nx * ny, 0.0);
  for (int a = 0; a < ny; a++)
    for (int b = 0; b < nx; b++) { pos[3 * (a * nx + b)] = 4.5 / (nx - 1) * b; pos[3 * (a * nx + b) + 1] = -4.5 / (ny - 1) * a; }
  tri.clear();
  for (int i = 0; i < ny; i++)
    for (int j = 0; j < nx; j++) {
      const int t = i * nx + j;
      if (i > 0 && j + 1 < nx) tri.insert(tri.end(), {t - nx + 1, t - nx, t});
      if (i > 0 && j > 0) tri.insert(tri.end(), {t - 1, t, t - nx});
    }
}

static void build(HostSystem &H, int N, const std::vector<double> &pos, const std::vector<int> &tri, const std::string &tag) {
  if (!H.set_mesh(N, pos.data(), (int) tri.size() / 3, tri.data())) fail(tag + ": set_mesh");
  if (!H.build_numerics(1.0 / 180, 0.3, 150.0, 1e-5, 1e4)) fail(tag + ": build_numerics");
}

static void renumber(int N, std::vector<double> &pos, std::vector<int> &tri) {      // as dc_set_mesh: reverse Cuthill-McKee
  const std::vector<int> order = rcm_order(N, (int) tri.size() / 3, tri.data());
  std::vector<int> inv(N);
  for (int k = 0; k < N; k++) inv[order[k]] = k;
  std::vector<double> p2(pos.size());
  for (int k = 0; k < N; k++) for (int d = 0; d < 3; d++) p2[3 * (size_t) k + d] = pos[3 * (size_t) order[k] + d];
  for (int &v : tri) v = inv[v];
  pos.swap(p2);
}

static void plan(HostTables &T, const HostSystem &H, const TableSwitches &sw, bool deflation = false) {
  dc_params prm;
  std::memset(&prm, 0, sizeof(prm));
  prm.time_step = 1.0 / 180;
  T.build(H, prm, sw);
  T.set_deflation(deflation && T.defl_rows > 0, sw);
}

static bool read_mesh(const char *path, int &N, std::vector<double> &pos, std::vector<int> &tri) {
  FILE *f = std::fopen(path, "rb");
  int hdr[2];
  if (!f || std::fread(hdr, 4, 2, f) != 2) return false;
  N = hdr[0];
  pos.resize(3 * (size_t) hdr[0]); tri.resize(3 * (size_t) hdr[1]);
  const bool ok = std::fread(pos.data(), 8, pos.size(), f) == pos.size() && std::fread(tri.data(), 4, tri.size(), f) == tri.size();
  std::fclose(f);
  return ok;
}

int main(int argc, char **argv) {
  std::vector<double> pos;
  std::vector<int> tri;
  {
    bench_grid(100, 100, pos, tri);
    HostSystem H;
    build(H, 100 * 100, pos, tri, "grid 100 x 100");
    std::set<int> offs;
    if (!rule_has_template(H, offs)) fail("grid 100 x 100: the CSR has a template");
    const int want[12] = {-199, -101, -100, -99, -98, -1, 1, 98, 99, 100, 101, 199};
    if (!std::equal(offs.begin(), offs.end(), want) || offs.size() != 12) fail("grid 100 x 100: the CSR's offsets are not the expected twelve");
    TableSwitches sw;
    HostTables T;
    plan(T, H, sw);
    if (!T.pk_ok || T.pk_vpt != 20 || T.pk_threads != 512 || !T.win_ok || !T.pk_ofs || !T.pk_tpl || !T.pk.tpl) fail("plan: the 10 000-vertex grid must get the template layout");
    for (int j = 0; j < 12; j++) if (T.pk.tpl_off[j] != want[j]) fail("grid 100 x 100: the template is not the twelve offsets");
    check_stream(H, T, "grid 100 x 100");
    // guards: 199 rows each side, rounded up to 16 bytes; the kernel's LDS request with them inside the CU's 160 KB next to its static LDS
    if (T.pk_guard_bytes != 1600 || T.pk_guard_bytes < 8 * T.pk.tpl_reach || T.pk_guard_bytes % 16 != 0) fail("grid 100 x 100: guard size");
    const PkShape &s = kPkShapes[T.pk.shape];
    for (int detect = 0; detect < 2; detect++) {
      const size_t lds = pk_lds_bytes(s.threads, s.vpt, s.xl_h16, true, false, 0, true, (int) T.win.lds_bytes, detect != 0, T.pk_guard_bytes);
      if (lds < (size_t) 155648 + 2 * 1600 || lds + 192 > (size_t) 160 * 1024) fail("grid 100 x 100: pk_lds_bytes with the guards must fit 160 KB");
    }
    if (2 * (T.pk_guard_bytes / 8) > s.threads) fail("grid 100 x 100: one guard store per thread");
    const PlanFacts f = T.facts(H.N);
    const FwdChoice c = forward_choice(f, KernelSwitches());
    if (!f.pk_tpl || c.family != kFwdPacket || !c.h16 || !c.ofs || !c.tpl || c.threads != 512 || c.vpt != 20) fail("plan: the choice must name the template instance");
    std::printf("ok plan: template, guards %d bytes\n", T.pk_guard_bytes);

    // DC_PK_TPL=0: the byte-offset layout, byte for byte
    HostTables T0;
    sw.pk_tpl = false;
    plan(T0, H, sw);
    HostPackets P;
    P.build(H);
    P.to_offsets();
    if (T0.pk_tpl || T0.pk.tpl || T0.pk_guard_bytes != 0 || !T0.pk_ofs || !T0.pk.ofs || T0.pk.pk != P.pk || T0.pk.pk_ptr != P.pk_ptr) fail("plan: DC_PK_TPL=0 must keep the byte-offset layout byte for byte");
    if (forward_choice(T0.facts(H.N), KernelSwitches()).tpl) fail("plan: DC_PK_TPL=0 must not name the template instance");
    // the layouts the template follows from: none of them, no template
    sw = TableSwitches(); sw.pk_ofs = false;
    plan(T0, H, sw);
    if (T0.pk_tpl || T0.pk.tpl || T0.pk.ofs) fail("plan: DC_PK_OFS=0 keeps the first layout");
    sw = TableSwitches(); sw.pk_h16 = false;
    plan(T0, H, sw);
    if (T0.pk_tpl || T0.pk.tpl) fail("plan: the fp32-plane instance reads the first layout");
    // a deflated solve keeps the byte offsets (its projection writes floats into the direction's LDS)
    sw = TableSwitches();
    plan(T0, H, sw, true);
    if (!T0.fwd_defl || T0.pk_tpl || T0.pk.tpl || !T0.pk_ofs || T0.pk.pk != P.pk) fail("plan: the deflated instance keeps the byte-offset layout");
    std::printf("ok plan: fall-backs by switch and deflation\n");

    // the same grid renumbered (DC_RENUMBER=1): the offsets are per-row data again
    renumber(100 * 100, pos, tri);
    HostSystem Hr;
    build(Hr, 100 * 100, pos, tri, "grid 100 x 100 renumbered");
    if (rule_has_template(Hr, offs)) fail("grid 100 x 100 renumbered: expected more than twelve offsets");
    plan(T0, Hr, sw);
    if (!T0.pk_ok || !T0.pk_ofs || T0.pk_tpl || T0.pk.tpl) fail("plan: the renumbered grid must fall back to byte offsets");
    std::printf("ok plan: renumbered grid falls back (%zu offsets)\n", offs.size());
  }
  for (int a = 1; a < argc; a++) {
    int N = 0;
    if (!read_mesh(argv[a], N, pos, tri)) fail(std::string(argv[a]) + ": cannot read");
    if (2 * mesh_bandwidth((int) tri.size() / 3, tri.data()) > 511) renumber(N, pos, tri);
    HostSystem H;
    build(H, N, pos, tri, argv[a]);
    std::set<int> offs;
    const bool rule = rule_has_template(H, offs);
    TableSwitches sw;
    HostTables T;
    plan(T, H, sw);
    // the rule: a template in the CSR, a halves instance with byte offsets, guards that fit
    bool want = rule && T.pk_ok && T.pk_ofs;
    if (want) {
      int reach = 0;
      for (int d : offs) reach = std::max(reach, std::abs(d));
      const PkShape &s = kPkShapes[T.pk.shape];
      const int guard = pk_tpl_guard_bytes(reach);
      want = pk_lds_bytes(s.threads, s.vpt, s.xl_h16, true, false, 0, T.win_ok != 0, (int) T.win.lds_bytes, true, guard) + 3 * 8 * (s.threads / 64) <= (size_t) kLdsLimitBytes &&
             2 * (guard / 8) <= s.threads;
    }
    if ((T.pk_tpl != 0) != want || T.pk.tpl != want) fail(std::string(argv[a]) + ": the plan's decision is not the rule's");
    if (want) check_stream(H, T, "mesh " + std::to_string(a));
    std::printf("ok mesh %d N=%d distinct offsets=%zu template in the CSR=%d plan=%s\n", a, N, offs.size(), (int) rule, want ? "template" : "fall-back");
    if (a == 2 && want) fail("the dress (rows of more than one batch) must fall back");
  }
  std::printf("ALL OK\n");
  return 0;
}
