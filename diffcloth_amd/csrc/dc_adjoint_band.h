// Banded direct adjoint solve (dc_params::adjoint_mode = 3; kernels in dc_adjoint_band.hip): the dense solve of dc_adjoint_dense.h restricted
// to the band of K. Without self contacts that couple outside it, K = M + E Y has the sparsity of P (x) 3 x 3 in the device's numbering; with
// the unknowns interleaved (index 3 i + c, i the device vertex) its half-bandwidth is kl = ku = 3 (bw + extra) + 2 (dc_bandplan.h). LU with
// partial pivoting then costs at most 2 n kl (kl + ku) flops and needs ldab n doubles, with no n^2 term.
//
// Band layout (LAPACK's): element (r, c) at AB[(kl + ku + r - c) + c ldab], ldab = 2 kl + ku + 1 rounded up to 16; the upper kl rows take
// the fill of pivoting and are zero on entry. One band, one pivot vector [n] and one flag per rollout of a chunk.
// Factors in place, LINPACK-style throughout: the row swap of column j is applied to the columns right of j only, the multipliers of a
// column stay in the rows they were computed in (a band has no room for swapped ones: row p <= j + kl of a column c < j lies up to
// kl + (j - c) below the diagonal). Inside a panel the kernels work LAPACK-style on a dense copy (the `panel` scratch: the trailing
// kernels read L11 / L21 from it) and undo the panel's swaps on the multipliers before they store them.
#pragma once
#include <cstddef>
#include "dc_device.h"
#include "dc_adjoint_dense.h"
#include "dc_bandplan.h"

namespace dc {

static_assert(kBandPanel == kLuPanel, "the band solve uses the dense solve's panel width");

// scratch of the band solve for a chunk of nb rollouts
struct BandAdjWork {
  double *AB;       // [nb][n][ldab] the bands, then their LU factors
  int *piv;         // [nb][npiv] pivot row of every column (absolute row)
  int *flag;        // [nb] 1 = K has an entry outside the band, or the factorisation met a zero or non-finite pivot: fp64 BiCGSTAB fall-back
  double *pm;       // [nb][9][N] as DenseAdjWork::pm
  double *sg;       // [nb][cap][9] as DenseAdjWork::sg
  double *panel;    // [nb][2][kLuPanel][pld] block 0: the current panel with its swaps applied to whole rows (L11, L21 of the trailing
                    // kernels); block 1: the panel kernel's working copy where the panel does not fit LDS
  int n, kl, ldab, pld, npiv;
  int sub_cols;     // columns of multipliers the substitution holds in LDS at a time (dc_bandplan.h: band_sub_cols)
};

// K of rollouts b0 .. b0 + nb - 1 of the record A describes (A.nsteps must be 1), in band storage; x64 as launch_dense_assemble's
void launch_band_assemble(const DevSystem &S, const BwdArgs &A, double *x64, const BandAdjWork &D, int b0, int nb, hipStream_t st);
// LU of the nb bands in place; *launches += the kernel launches it enqueued
hipError_t launch_band_factor(const BandAdjWork &D, int nb, hipStream_t st, int *launches);
// the adjoint step of rollouts b0 .. b0 + nb - 1 with the factors of D
hipError_t launch_band_adjoint_step(const DevSystem &S, const DevWork &W, const BwdArgs &A, const BandAdjWork &D, int b0, int nb, hipStream_t st);

}  // namespace dc
