// CDNA4 (gfx950) forward step, split variant with spectral deflation: the instances of k_pd_step_cl (dc_forward_cl_kernel.h) whose PCG solves
// start with the Galerkin projection onto the 16 lowest eigenvectors of the scaled system matrix (dc_deflate.h; built by the engine for meshes on
// which plain Jacobi-PCG needs hundreds of iterations). Reference: the global solve of Simulation::step, Simulation.cpp:1267.
#define DC_KERNEL_TU
#include "dc_forward_cl_kernel.h"

namespace dc {

hipError_t launch_pd_step_cluster_deflated(const DevSystem &S, const DevCluster &CL, const DevWork &W, const FwdArgs &A, const ClFwdChoice &ch, int b0, int nb, hipStream_t st) {
  if (!S.defl_u) return hipErrorInvalidValue;
  return launch_cl_choice<true>(S, CL, W, A, ch, b0, nb, st);
}

}  // namespace dc
