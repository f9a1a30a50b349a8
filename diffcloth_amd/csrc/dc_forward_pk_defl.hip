// CDNA4 (gfx950) forward step, packet-ELL resident variant with spectral deflation: the instances of k_pd_step_pk (dc_forward_pk_kernel.h)
// whose PCG solves start with the Galerkin projection onto the 16 lowest eigenvectors of the scaled system matrix (dc_deflate.h) — the
// engine builds that space only for meshes on which plain Jacobi-PCG needs hundreds of iterations (the reference's 7 742-vertex dress: 262 per
// PD iteration). Reference: the global solve of Simulation::step, Simulation.cpp:1267.
#define DC_KERNEL_TU
#include "dc_forward_pk_kernel.h"

namespace dc {

hipError_t launch_pd_step_packet_deflated(const DevSystem &S, const DevWork &W, const FwdArgs &A, const FwdChoice &ch, int B, hipStream_t st) {
  return launch_pk_choice<true>(S, W, A, ch, B, st);
}

}  // namespace dc
