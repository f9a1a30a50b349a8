// CDNA4 (gfx950) forward step, packet-ELL resident variant (N <= 10240, matrix bandwidth <= 511).
//
// Same algorithm and per-rollout workgroup ownership as dc_forward.hip / dc_forward_res.hip; the inner Jacobi PCG
// (>95 % of the sweeps of a step) is restructured around what bounds it on a CU, the 64 B/clk vector-memory pipe
// that streams the shared matrix, and the register file:
//   * the PCG runs on the symmetrically scaled system  (D^-1/2 P D^-1/2) xs = D^-1/2 rhs  (unit diagonal): plain CG
//     on it IS the Jacobi-preconditioned CG on P (same iterates, same r^T D^-1 r stopping rule) but needs no
//     diagonal / preconditioner traffic inside the loop;
//   * off-diagonals travel as 16-byte packets {v0, v1, v2, d0 | d1 << 10 | d2 << 20}: three fp32 values and three
//     10-bit column deltas relative to the row (biased by 512) = 5.33 B per non-zero instead of 8, one
//     global_load_dwordx4 per three non-zeros, wave-sliced so a wave reads 1 KiB contiguous per instruction;
//     the next row's packets are in flight while the current row is consumed; the instances that hold the direction
//     as halves read 12 values + 12 16-bit byte offsets per batch instead (6 B per non-zero, dc_packets.h), which
//     takes one address instruction per non-zero instead of two;
//   * the search direction p lives in LDS as a float2 (x, y) plane + a float z plane (a neighbour costs one
//     ds_read_b64 + one ds_read_b32), the residual r and A p in registers, the iterate x in registers for the
//     first VPT - XL rows of a thread and in the LDS left over by p for the rest: nothing of a CG iteration
//     touches global memory except the (L2-resident, batch-shared) packet stream;
//   * the per-constraint work of a PD iteration (local projections, friction, right-hand side) runs through the LDS
//     element windows of dc_winlib.h, and a launch can carry all time steps of a rollout (FwdArgs::nsteps) with the
//     self-collision detection of each step inlined (dc_selflib.h).
// Reference: Simulation::step (Simulation.cpp:1043-1428), global solve :1267 (SimplicialLLT::solve) replaced by
// this PCG on the correction system (see dc_forward.hip header).
#define DC_KERNEL_TU
#include "dc_forward_pk_kernel.h"

namespace dc {

// 512 (or 768) threads own VPT = pk_vpt rows each: the packet tables are padded for exactly the shape the table plan picked from kPkShapes
// (dc_packets.cpp, dc_kernelplan.h), and the choice names that shape's instance.
hipError_t launch_pd_step_packet(const DevSystem &S, const DevWork &W, const FwdArgs &A, const FwdChoice &ch, int B, hipStream_t st) {
  return launch_pk_choice<false>(S, W, A, ch, B, st);
}

}  // namespace dc
