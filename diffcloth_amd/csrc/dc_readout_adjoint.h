// Arguments and launchers of the contact read-out's adjoint (dc_readout_adjoint.hip; dc_set_contact_readout_gradients).
#pragma once
#include "dc_device.h"

namespace dc {

// Every table pointer is that of tape slot 0; the kernel walks the records slot, slot - 1 ... first (the seed phase also first - 1, for its part of
// the loss gradient at the state the call arrives at) of rollout blockIdx.x and skips those whose
// has[] entry is 0 (no weights were given: zeros).
struct ReadoutAdjArgs {
  const float *X, *V, *F, *NRM;     // [slot][B][3][N] tape
  const int *PRIM;                  // [slot][B][N]
  const float *PC;                  // [slot][B][P][3] primitive centres
  const float *PV;                  // [slot][B][G][kPvRow] obstacle motion, null = none set
  const float *XF;                  // [slot][B][3][Af] fixed-point targets
  const float *mu;                  // [B][G]
  const float *WJ;                  // [slot][B][N] dL/djn, device numbering
  const float *WW;                  // [slot][B][G][kWrenchRow] dL/dwrench (entries 7..9 unread)
  const unsigned char *has;         // [slot] 1 = the slot carries weights
  int B, slot, first;
  int top_done;                     // 1 = the carried gradient already holds the read-out's part of record `slot` (the call continues a chain)
  // record handed in from outside (dc_set_record): [B][3][N] doubles, valid for inj_slot only; null = none
  const double *inj_x, *inj_f, *inj_n;
  int inj_slot;
  // seed phase: the carried gradient (loss gradient at `slot`) and the engine's combined seed rows, [slot][B][3][N]
  float *gx, *rsx, *rsv;
  // parameter phase: what the step kernels left
  float *DPAR;                      // [slot][B][8]
  float *DXF;                       // [slot][B][3][Af]
  float *YS;                        // [slot][B][3][N] kept y tape or null
  float *DMU;                       // [B][G]
  float *DPV;                       // [slot][B][G][kPvRow] or null
};

// phase 0 = seeds (before the step kernels), 1 = parameter terms (after them)
void launch_readout_adjoint(const DevSystem &S, const DevWork &W, const ReadoutAdjArgs &A, int phase, hipStream_t st);
// `rows` rows of n per-vertex values in the caller's numbering (fp32 or fp64) -> fp32 rows in device numbering, one launch
void launch_vertex_rows_in(const void *src, int is_f32, float *dst, long rows, int n, const int *user_of, hipStream_t st);

}  // namespace dc
