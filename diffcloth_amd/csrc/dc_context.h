// The context behind the C-ABI handle (include/diffcloth_hip.h: dc_ctx) and the error helpers of the translation units that implement its
// entry points (dc_engine.hip, dc_comm.cpp). Private to csrc/.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include <vector>
#include "dc_device.h"
#include "dc_system.h"
#include "dc_deflate.h"
#include "dc_cluster.h"
#include "dc_adjoint_dense.h"
#include "dc_adjoint_band.h"

// Tables of the split kernels (dc_cluster.h) for one K, built when the batch size is known (dc_alloc_batch).
struct ClusterSet {
  bool ok = false;
  int K = 1, nb = 0;              // workgroups per rollout; rollouts per launch (K nb <= CUs)
  dc::DevCluster D;
  std::vector<void *> allocs;
  size_t xch_bytes = 0;
};

struct dc_ctx {
  int device = 0;
  bool host_only = false;   // dc_create(-1): table building / inspection only, every compute call fails
  hipStream_t stream = nullptr;
  hipStream_t own_stream = nullptr; // the stream dc_create made (dc_use_stream may point `stream` at the caller's)
  std::string err;
  dc::HostSystem host;
  dc_params params;
  std::vector<dc_primitive> prims;
  std::vector<int> group_of_prim;
  int ngroups = 0;
  bool mesh_set = false, built = false;
  // vertex renumbering on the device (empty = identity): user_of[device index] = caller's index, dev_of = inverse
  std::vector<int> user_of, dev_of;
  std::vector<int> att_user;        // attachment vertices in the caller's numbering
  const int *d_user_of = nullptr;   // device copy of user_of (null = identity)

  dc::DevSystem S;
  dc::PlanFacts facts;              // the table plan's decisions and the forward step's kernel instance chosen from them (dc_kernelplan.h),
  dc::FwdChoice fwd;                // set by dc_build with the other decisions (host-only contexts too)
  std::vector<void *> table_allocs;

  int B = 0, tape = 0;
  dc::DevWork W;
  std::vector<void *> batch_allocs;
  float *X = nullptr, *V = nullptr, *F = nullptr, *R = nullptr, *NRM = nullptr;   // [(tape+1)][B][3][N]
  int *PRIM = nullptr;                                                            // [(tape+1)][B][N]
  int2 *SC_pair = nullptr;          // [(tape+1)][B][cap] self contacts per record
  float4 *SC_nrm = nullptr, *SC_d = nullptr;
  int *SC_meta = nullptr;           // [(tape+1)][B][kMetaStride]
  int *SC_verts = nullptr;          // [(tape+1)][B][2 * cap] working-set vertex lists of the self contacts
  int self_cap = 0;
  float *xf_cur = nullptr;          // [B][3][Af]
  float *XF = nullptr;              // [(tape+1)][B][3][Af] fixed-point targets per record
  float *DPAR = nullptr;            // [(tape+1)][B][8] per-step parameter gradients
  float *mu = nullptr, *fu = nullptr;
  bool fu_set = false;
  float *fv = nullptr;              // [B][3][N] per-vertex extra force
  bool fv_set = false;
  float *fv2 = nullptr;             // [B][3][N] second per-vertex force term, factor 1 (dc_set_vertex_force_field)
  bool fv2_set = false;
  int start_slot = 0;              // dc_set_trajectory_start: the tape slot of the trajectory's initial state (-1: none in this tape)
  float *GX = nullptr, *GV = nullptr, *IX = nullptr, *IV = nullptr, *DMU = nullptr, *target = nullptr;
  float *DXF = nullptr;             // [(tape+1)][B][3][Af] dL_dxfixed of the step that produced the slot
  // device-resident schedules of the fused rollouts (dc_set_*_schedule); flags per tape slot
  float *FU_S = nullptr;            // [(tape+1)][B][3] uniform force of the step that produces the slot
  float *FVS_S = nullptr;           // [(tape+1)][B] factor on fv of that step
  float *SEEDX = nullptr, *SEEDV = nullptr;   // [(tape+1)][B][3][N] loss gradient w.r.t. the state at the slot (allocated on first use)
  std::vector<char> sched_xf, sched_fu, sched_fvs, sched_seed;
  // gradients of a loss on the contact read-out (dc_set_contact_readout_gradients), allocated by the first setter after dc_alloc_batch: the
  // weights per record in device numbering, a device flag per slot, and the seed rows the backward sweep reads in place of the caller's schedule
  // while a record of the sweep carries weights (caller's entry + the read-out's part; the caller's schedule is never written)
  float *RWJ = nullptr;             // [(tape+1)][B][N] dL/djn
  float *RWW = nullptr;             // [(tape+1)][B][G][10] dL/dwrench
  unsigned char *rw_has = nullptr;  // [(tape+1)] 1 = the slot carries weights
  float *RSX = nullptr, *RSV = nullptr;       // [(tape+1)][B][3][N]
  std::vector<char> sched_rw;
  int rw_arrived = -1;              // the state the last backward call arrived at when the gradient it left holds the read-out's part of that record; -1 = none
  int rw_launches = 0;              // launches of the read-out's adjoint passes in the sweep being enqueued (dc_kernel_times counts them)
  // self-contact read-out (dc_get_self_contact_readout): the planes of the global-memory walk, allocated by the first call after dc_alloc_batch
  // whose LDS plan (dc_self_readout.h) cannot hold every possible record; null otherwise
  float *sro_scratch = nullptr;     // [B][3][N] g - f
  double *sro_sums = nullptr;       // [B][3][N] per-vertex sums
  // movable obstacles (dc_set_primitive_offsets / dc_set_primitive_offset_schedule, dc_primoffset.h): absolute fp32 centres of the P flattened
  // primitives. Every row of PC is valid at all times — the built centres until something else is written — and the forward kernels always
  // read the row of the slot their step produces, so a slot says where its obstacle was (dc_get_primitive_centers).
  float *PC = nullptr;              // [(tape+1)][B][P][3] centres used by the step that produces the slot
  float *pc_cur = nullptr;          // [B][P][3] centres of the NEXT steps that have no schedule entry
  const double *pc_built = nullptr; // [P][3] device copy of dc_primitive::center, and of group_of_prim, for the conversion kernel
  const int *pc_group = nullptr;
  // which version of pc_cur a row of PC holds: 0 = the built centres, -1 = a schedule entry, > 0 = the pc_cur of that dc_set_primitive_offsets
  // call; an unscheduled step copies pc_cur into its row only when the two differ (never, while no offsets are set)
  std::vector<int> pc_row_gen;
  int pc_gen = 0, pc_gen_last = 0;
  std::vector<char> sched_pc;
  // obstacle motion: velocities w (dc_set_primitive_velocities / dc_set_primitive_velocity_schedule) and angular velocities omega
  // (dc_set_primitive_spins / dc_set_primitive_spin_schedule), fp32, one row {w[3], omega[3]} (dc::kPvRow floats) per primitive GROUP. All three
  // arrays are allocated by the first setter of either kind after dc_alloc_batch and zeroed; while PV is null the kernels get null pointers and
  // evaluate the static contact law. Row `slot` of PV is what the step that produced `slot` used and what the backward step through record
  // `slot` reads. The two halves of a row are set, scheduled and read independently (sched_pv: w, sched_pw: omega).
  float *PV = nullptr;              // [(tape+1)][B][G][6]
  float *pv_cur = nullptr;          // [B][G][6] motion of the NEXT steps; a half applies where that half has no schedule entry
  float *DPV = nullptr;             // [(tape+1)][B][G][6] {dL/dw, dL/domega} of the backward step through record `slot` (overwritten per step)
  std::vector<char> sched_pv, sched_pw;
  bool pv_set = false, pw_set = false;      // a velocity / a spin setter has run on this batch (the gradient getters of a kind fail before)
  // obstacle shapes (dc_set_primitive_shapes / dc_set_primitive_shape_schedule, dc_primshape.h): fp32 rows {top_offset, corner2, radius, length}
  // per flattened primitive. Allocated by the first shape setter after dc_alloc_batch and filled with the built shapes; while PS is null the
  // kernels get a null pointer and read DevPrim. Row `slot` of PS is what the step that produced `slot` used.
  float *PS = nullptr;              // [(tape+1)][B][P][8]
  float *ps_cur = nullptr;          // [B][P][8] shapes of the NEXT steps that have no schedule entry
  const float *ps_built = nullptr;  // [B][P][8] the built shapes (what dc_set_primitive_shapes_dev(NULL) restores without a synchronisation)
  // which version of ps_cur a row of PS holds, the scheme of pc_row_gen: 0 = the built shapes, -1 = a schedule entry, > 0 = the ps_cur of that
  // dc_set_primitive_shapes call
  std::vector<int> ps_row_gen;
  int ps_gen = 0, ps_gen_last = 0;
  std::vector<char> sched_ps;
  void *comm = nullptr;             // RCCL communicator of dc_comm_init (ncclComm_t), one rank per context
  int comm_ranks = 0;
  std::vector<void *> sched_pool;
  float *YS = nullptr;              // [(tape+1)][B][3][N] y of every backward step (dc_keep_force_gradients), allocated on first use
  bool keep_y = false;
  // record handed in from outside (dc_set_record): fp64 values of x_new, f, primitive-contact normals [B][3][N], self-contact normals / d
  // [B][cap][3]; allocated on first use, valid for tape slot inj_slot only (-1 = none)
  double *INJ_X = nullptr, *INJ_F = nullptr, *INJ_N = nullptr, *INJ_SN = nullptr, *INJ_SD = nullptr;
  int inj_slot = -1;
  dc_step_stats *fstats = nullptr;  // [(tape+1)][B]
  dc_bwd_stats *bstats = nullptr;   // [(tape+1)][B], indexed by the slot whose record was differentiated
  int *adj_path = nullptr;          // [B][2] backward steps run by an instance with step-resident contact tables, and those that used them (dc_get_adjoint_contact_path)
  double *stage[4] = {nullptr, nullptr, nullptr, nullptr};   // staging of the host <-> device conversions, handed out by stage_take (dc_engine.hip)
  int stage_live = 0;               // how many of them have been handed out since the stream was last synchronised by stage_sync
  size_t stage_elems = 0;
  hipEvent_t ev_a = nullptr, ev_b = nullptr, ev_t0 = nullptr, ev_t1 = nullptr;
  float fwd_ms = 0, bwd_ms = 0;
  int fwd_launches = 0, bwd_launches = 0;
  ClusterSet cl;
  int cus = 0;                      // compute units of the device
  int bandwidth = 0;                // of the scalar system matrix in device numbering
  int defl_k = 0, defl_probe = 0;   // deflation space of the forward solve (dc_deflate.h)
  // the last deflation build of this context and what it was built from: a rebuild that leaves P unchanged (another tolerance, contact flags,
  // primitives ...) skips the probe solve and the eigen-solve (0.9 s on the 7 742-vertex dress)
  dc::HostDeflation defl_cache;
  uint64_t defl_key = 0;
  bool defl_cache_valid = false, defl_cache_built = false;
  // dense direct adjoint solve (adjoint_mode 2, dc_adjoint_dense.h): matrices / factors of a chunk of dense_nb rollouts, allocated in the
  // batch pool on the first mode-2 backward step; phase times (assembly, factorisation, solve) when DC_DENSE_TIMES=1
  dc::DenseAdjWork dense{};
  int dense_nb = 0;
  int dense_launches = 0;           // kernel launches of the mode-2 backward steps enqueued (counter; dc_rollout_backward adds the difference)
  int dense_mark = 0;               // that counter when the rollout call began
  bool dense_timing = false;
  float dense_ms[3] = {0, 0, 0};
  hipEvent_t ev_d[4] = {nullptr, nullptr, nullptr, nullptr};
  // banded direct adjoint solve (adjoint_mode 3, dc_adjoint_band.h): bands / factors of a chunk of band_nb rollouts, in a pool of their own
  // (dc_set_adjoint_band changes their size: re-allocated at the next mode-3 backward step); counters, timing and events are mode 2's
  dc::BandAdjWork band{};
  int band_nb = 0;
  int band_extra = 0;               // dc_set_adjoint_band: vertices added to the matrix bandwidth
  std::vector<void *> band_allocs;
};

inline int fail(dc_ctx *c, int code, const std::string &msg) {
  if (c) c->err = msg;
  return code;
}
#define HIPCHK(c, call)                                                                         \
  do {                                                                                          \
    hipError_t e_ = (call);                                                                     \
    if (e_ != hipSuccess)                                                                       \
      return fail(c, DC_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_));            \
  } while (0)
