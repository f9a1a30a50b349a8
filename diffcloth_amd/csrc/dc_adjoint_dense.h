// Dense direct adjoint solve (dc_params::adjoint_mode = 2; kernels in dc_adjoint_dense.hip): per rollout the adjoint operator
// K = M + h^2 (A - dp/dx)^T A (I + dr_df)^T of dc_adjoint64.h is assembled as a dense fp64 matrix, factored by LU with partial
// pivoting, and the adjoint step solves K u = g by forward / back substitution with those factors, refined against the fp64
// residual (the GPU counterpart of Simulation::solveDirect, reference Simulation.cpp:1431-1440, which factors K with SparseLU).
//
// Matrix layout: column-major, rows and columns in the kernels' planar vector order (row c N + i = component c of device vertex i),
// leading dimension dense_adj_ld(N) (3N rounded up to a multiple of 16); one matrix of ld^2 doubles per rollout of a chunk.
// Factors in place: LINPACK-style across panels of kLuPanel columns (the row swaps of a panel are applied to the columns right of it,
// not to the factored columns left of it), LAPACK-style inside a panel; pivots [n] per rollout, absolute row indices.
#pragma once
#include <cstddef>
#include "dc_device.h"

namespace dc {

// Largest mesh of the dense kernels: the forward pass's explicit inverse (dc_dense.h) and the dense adjoint solve (3 x 768 = 2 304 unknowns,
// 42 MB of factors per rollout).
constexpr int kDenseMaxN = 768;
constexpr int kLuPanel = 32;       // columns of one LU panel (inner dimension of the trailing update)

inline int dense_adj_ld(int N) { return (3 * N + 15) / 16 * 16; }

// scratch of the dense solve for a chunk of nb rollouts
struct DenseAdjWork {
  double *K;        // [nb][ld][ld] the matrices, then their LU factors
  int *piv;         // [nb][ld] pivot row of every column
  int *flag;        // [nb] 1 = the factorisation met a zero or non-finite pivot: the adjoint step takes the fp64 BiCGSTAB fall-back
  double *pm;       // [nb][9][N] (I + dr_df)^T of every vertex's primitive contact (column-major 3 x 3, planar by entry)
  double *sg;       // [nb][cap][9] the self contacts' G = mred * dr_df^T (column-major 3 x 3)
  int ld;
};

// K of rollouts b0 .. b0 + nb - 1 of the record A describes (A.nsteps must be 1); x64 = the rollouts' fp64 x_new scratch ([B][3][N], W.x64)
void launch_dense_assemble(const DevSystem &S, const BwdArgs &A, double *x64, const DenseAdjWork &D, int b0, int nb, hipStream_t st);
// the first kernel of launch_dense_assemble alone: x64 and D.pm / D.sg of the rollouts (D.K is not touched); the band solve's assembly
// (dc_adjoint_band.h) starts from the same blocks
void launch_dense_prep(const DevSystem &S, const BwdArgs &A, double *x64, const DenseAdjWork &D, int b0, int nb, hipStream_t st);
// LU of the nb matrices in place; returns the number of kernel launches it enqueued
int launch_dense_factor(const DenseAdjWork &D, int n, int nb, hipStream_t st);
// the adjoint step of rollouts b0 .. b0 + nb - 1 with the factors of D
void launch_dense_adjoint_step(const DevSystem &S, const DevWork &W, const BwdArgs &A, const DenseAdjWork &D, int b0, int nb, hipStream_t st);

}  // namespace dc
