// Host-side builder of the packet-ELL copy of the system matrix used by the resident PCG (dc_forward_pk.hip):
// P symmetrically scaled to unit diagonal (D^-1/2 P D^-1/2, so that plain CG on it is Jacobi-preconditioned CG on P),
// off-diagonals packed three to a 16-byte packet {v0, v1, v2, d0 | d1 << 10 | d2 << 20} with d = column - row + 512,
// wave-sliced: chunk c = rows 64c .. 64c+63, packet (s, lane) at pk[4 * (pk_ptr[c] + 64 s + lane)], pk_n[c] packets per
// row (a multiple of 4). Padding packets are {0, 0, 0, 512 | 512 << 10 | 512 << 20} (value 0 on the row itself).
//
// Second layout (to_offsets; the kernels that hold the search direction as 8-byte rows of halves): the same non-zeros in the same order,
// each with the BYTE offset 8 d of its column's direction entry from the entry of row - 512, as a 16-bit field — the kernel forms the
// LDS address of a gather with one add that selects the field (dc_pklib.h: gather_o) instead of a bit-field extract and a shift-add.
// A batch of 4 packets (12 non-zeros) becomes 18 dwords per lane, wave-sliced as one 8-byte slice of offsets {o8 | o9 << 16, o10 | o11 << 16},
// three 16-byte slices of values {v0 .. v3}, {v4 .. v7}, {v8 .. v11} and one 16-byte slice of offsets {o0 | o1 << 16, ..., o6 | o7 << 16} (the
// 8-byte slice first: every slice then lies within the 4095 bytes a global load's immediate offset reaches from the batch's start):
// batch t of chunk c starts at pk[4 * (pk_ptr[c] + kPkOfsBatchInt4 * t)], the 8-byte slice at + 2 * lane, 16-byte slice j at
// + 4 * (32 + 64 j + lane). 6 B per non-zero instead of 5.33. pk_n stays the packet count of the first layout (4 per batch), pk_ptr stays in
// 16-byte units. Padding entries are value 0, offset 8 * 512 (the row itself).
//
// Third layout (to_template, from the second): values only. On a mesh whose numbering is regular — a row-major grid — the off-diagonals of
// every row stand at the same few columns relative to the row: when the whole matrix has at most kPkTplSlots = 12 distinct offsets
// (column - row) and no row needs a second batch, the offsets are a property of the matrix, not of the row. The template holds them in
// ascending order (padded with 0, the row itself), a row is 12 fp32 values, slot j the coefficient of column row + tpl_off[j], and a slot
// whose neighbour the row lacks holds 0: the same non-zeros in the same order, exact zeros interleaved. Chunk c is three 16-byte slices
// {v0 .. v3}, {v4 .. v7}, {v8 .. v11} at pk[4 * (kPkTplBatchInt4 * c + 64 j + lane)]: 48 B per row instead of 72. A zero slot of a boundary
// row may point up to tpl_reach rows outside the matrix: the kernel keeps that many zero rows on each side of the direction (dc_launchplan.h).
#pragma once
#include <vector>
#include "dc_kernelplan.h"
#include "dc_system.h"

namespace dc {

struct HostPackets {
  bool ok = false;
  bool ofs = false;               // pk is in the second layout (byte-offset fields)
  bool tpl = false;               // pk is in the third layout (values only; implies ofs: not the first layout)
  int tpl_off[kPkTplSlots] = {};  // third layout: column - row of slot j, ascending; unused slots 0
  int tpl_reach = 0;              // third layout: max |tpl_off|
  int vpt = 0;                    // rows per thread of the kernel the tables are padded for (threads * vpt rows)
  int threads = 512;              // threads of that kernel: 512, or 768 for the largest meshes (3 waves per SIMD, dc_forward_pk.hip)
  int shape = -1;                 // that kernel's entry of kPkShapes (dc_kernelplan.h); -1 = padded by build_rows for another kernel
  int bandwidth = 0;              // max |column - row| of P
  std::vector<int> pk;            // 4 ints per packet
  std::vector<int> pk_ptr, pk_n;  // per 64-row chunk
  std::vector<float> sq_dinv;     // [512 * vpt] sqrt(1 / P_ii), 0 for padding rows

  // false when the tables cannot be used: N > 10 240 rows or bandwidth > 511. want_threads: the value of DC_PK_THREADS, 0 = the default
  bool build(const HostSystem &H, int want_threads = 0);
  // the same tables padded to `rows_padded` rows (a multiple of 64, >= N), any N; false when the bandwidth exceeds 511
  bool build_rows(const HostSystem &H, int rows_padded);
  // rewrites pk / pk_ptr from the first layout into the second (pk_n, sq_dinv unchanged)
  void to_offsets();
  // rewrites pk / pk_ptr from the second layout into the third; false (and nothing changed) when the matrix has more than kPkTplSlots distinct
  // offsets, a row of more than one batch, or a row whose entries are not in ascending column order
  bool to_template();
};

}  // namespace dc
