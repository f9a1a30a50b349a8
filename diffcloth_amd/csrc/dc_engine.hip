// C-ABI layer of libdiffcloth_hip.so: context, device memory, tape, and the calls that enqueue the
// persistent step kernels. See include/diffcloth_hip.h for the contract of every entry point.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "dc_clusterplan.h"
#include "dc_context.h"
#include "dc_env.h"
#include "dc_primoffset.h"
#include "dc_primshape.h"
#include "dc_readout_adjoint.h"
#include "dc_record.h"
#include "dc_self_readout.h"
#include "dc_tables.h"
#include "dc_spheremesh.h"
#include "dc_selftmp.h"

using namespace dc;

namespace dc {
hipError_t launch_pd_step_cluster(const DevSystem &S, const DevCluster &CL, const DevWork &W, const FwdArgs &A, const ClFwdChoice &ch, int b0, int nb, hipStream_t st);
hipError_t launch_adjoint_step_cluster(const DevSystem &S, const DevCluster &CL, const DevWork &W, const BwdArgs &A, const ClAdjChoice &ch, int b0, int nb, hipStream_t st);
}

static_assert(rec::kMetaStride == kMetaStride && rec::kMaxLayers == kMaxLayers, "dc_record.h restates dc_device.h's record sizes");
static_assert(sizeof(rec::Int2) == sizeof(int2) && alignof(rec::Int2) == alignof(int2), "dc_record.h: Int2 is uploaded as int2");
static_assert(sizeof(rec::Float4) == sizeof(float4) && alignof(rec::Float4) == alignof(float4), "dc_record.h: Float4 is uploaded as float4");

namespace {

template <typename T>
int dev_alloc(dc_ctx *c, std::vector<void *> &pool, T **out, size_t count) {
  void *p = nullptr;
  size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
  HIPCHK(c, hipMalloc(&p, bytes));
  HIPCHK(c, hipMemsetAsync(p, 0, bytes, c->stream));
  pool.push_back(p);
  *out = (T *) p;
  return DC_OK;
}
template <typename T, typename U>
int upload(dc_ctx *c, const T **out, const std::vector<U> &src) {
  std::vector<T> tmp(src.begin(), src.end());
  T *p = nullptr;
  int rc = dev_alloc(c, c->table_allocs, &p, tmp.size());
  if (rc) return rc;
  if (!tmp.empty()) HIPCHK(c, hipMemcpy(p, tmp.data(), tmp.size() * sizeof(T), hipMemcpyHostToDevice));
  *out = p;
  return DC_OK;
}
// the same, behind a pointer to the kernels' vector type (int2 / int4 / float2 / float4 tables are built as flat arrays of T)
template <typename T, typename V, typename U>
int upload_as(dc_ctx *c, const V **out, const std::vector<U> &src) {
  const T *p = nullptr;
  const int rc = upload<T>(c, &p, src);
  *out = (const V *) p;
  return rc;
}
void free_pool(std::vector<void *> &pool) {
  for (void *p : pool) (void) hipFree(p);
  pool.clear();
}
// elements of one tape slot of the per-vertex arrays / of the fixed-point arrays, and the slots of the per-record arrays
size_t slot_elems(const dc_ctx *c) { return (size_t) c->B * 3 * c->host.N; }
size_t xf_elems(const dc_ctx *c) { return (size_t) c->B * 3 * c->S.Af; }
float *xf_slot(const dc_ctx *c, int slot) { return c->XF + xf_elems(c) * slot; }
float *dxf_slot(const dc_ctx *c, int slot) { return c->DXF + xf_elems(c) * slot; }
float *dpar_slot(const dc_ctx *c, int slot) { return c->DPAR + (size_t) c->B * 8 * slot; }
size_t pc_elems(const dc_ctx *c) { return (size_t) c->B * c->S.nprim * 3; }
float *pc_slot(const dc_ctx *c, int slot) { return c->PC + pc_elems(c) * slot; }
size_t pv_rows(const dc_ctx *c) { return (size_t) c->B * c->ngroups; }      // motion rows {w[3], omega[3]} per slot
size_t pv_elems(const dc_ctx *c) { return pv_rows(c) * kPvRow; }
float *pv_slot(const dc_ctx *c, int slot) { return c->PV + pv_elems(c) * slot; }
float *dpv_slot(const dc_ctx *c, int slot) { return c->DPV + pv_elems(c) * slot; }
size_t ps_elems(const dc_ctx *c) { return (size_t) c->B * c->S.nprim * kShapeRow; }
float *ps_slot(const dc_ctx *c, int slot) { return c->PS + ps_elems(c) * slot; }
// one rollout's built rows, [P][8], as dc_build rounded them
void built_shape_rows(const dc_ctx *c, std::vector<float> &rows) {
  const int P = c->S.nprim;
  rows.assign((size_t) P * kShapeRow, 0.0f);
  for (int p = 0; p < P; p++) {
    double row[kShapeRow];
    primitive_shape_row(c->prims[p], row);
    round_shape_row(row, rows.data() + (size_t) p * kShapeRow);
  }
}
float *seedx_slot(const dc_ctx *c, int slot) { return c->SEEDX + slot_elems(c) * slot; }
float *seedv_slot(const dc_ctx *c, int slot) { return c->SEEDV + slot_elems(c) * slot; }
SelfRec self_slot(const dc_ctx *c, int slot) {      // self contacts of record `slot`
  const size_t sc = (size_t) c->B * c->self_cap * slot, sm = (size_t) c->B * kMetaStride * slot;
  SelfRec R;
  R.pair = c->SC_pair + sc; R.nrm = c->SC_nrm + sc; R.dvec = c->SC_d + sc; R.meta = c->SC_meta + sm; R.verts = c->SC_verts + 2 * sc;
  return R;
}

int pd_cap(const dc_ctx *c) {
  if (c->params.pd_iter_cap >= 0) return c->params.pd_iter_cap;
  return (int) ((-std::log10(c->params.forward_tol)) * 150);   // Simulation.cpp:1182
}

// The staging buffers of the host <-> device conversions are handed out in turn; one that has been handed out since the last stage_sync is
// not handed out again before the stream has been synchronised. Entry points end their staged copies with stage_sync: a host-to-device copy
// has completed when the call returns (the caller may reuse its buffer), a device-to-host result is complete before the host touches it.
int stage_sync(dc_ctx *c) {
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->stage_live = 0;
  return DC_OK;
}
int stage_take(dc_ctx *c, double **buf) {
  if (c->stage_live == 4) { const int rc = stage_sync(c); if (rc) return rc; }
  *buf = c->stage[c->stage_live++];
  return DC_OK;
}
// per_vertex: the array is indexed by vertex (the device renumbering applies); false: by attachment / other index
int h2d_planar(dc_ctx *c, const double *src, float *dst, int n_per_rollout, bool per_vertex) {
  size_t elems = (size_t) c->B * 3 * n_per_rollout;
  double *stage;
  int rc = stage_take(c, &stage);
  if (rc) return rc;
  HIPCHK(c, hipMemcpyAsync(stage, src, elems * sizeof(double), hipMemcpyHostToDevice, c->stream));
  launch_f64i_to_f32p(stage, dst, c->B, n_per_rollout, per_vertex ? c->d_user_of : nullptr, c->stream);
  return DC_OK;
}
int d2h_planar(dc_ctx *c, const float *src, double *dst, int n_per_rollout, bool per_vertex) {
  size_t elems = (size_t) c->B * 3 * n_per_rollout;
  double *stage;
  int rc = stage_take(c, &stage);
  if (rc) return rc;
  launch_f32p_to_f64i(src, stage, c->B, n_per_rollout, per_vertex ? c->d_user_of : nullptr, c->stream);
  HIPCHK(c, hipMemcpyAsync(dst, stage, elems * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  return DC_OK;
}

int check_batch(dc_ctx *c, int slot_lo, int slot_hi) {
  if (!c->built) return fail(c, DC_ERR_STATE, "dc_build has not been called");
  if (c->B <= 0) return fail(c, DC_ERR_STATE, "dc_alloc_batch has not been called");
  if (slot_lo < 0 || slot_hi > c->tape) return fail(c, DC_ERR_INVALID, "tape slot out of range");
  return DC_OK;
}

// The reference's self-contact list has no limit (Simulation.cpp:281-352, 422-624); ours has, and says so: a step whose list
// was cut is not the reference's step.
int check_self_overflow(dc_ctx *c, const dc_step_stats *st, int slot) {
  for (int b = 0; b < c->B; b++)
    if (st[b].self_overflow)
      return fail(c, DC_ERR_CAPACITY, "self-contact list overflow in the step that produced slot " + std::to_string(slot) + ", rollout " +
                  std::to_string(b) + ((st[b].self_overflow & 1) ? ": more pairs than max_self_contacts = " + std::to_string(c->self_cap) : (st[b].self_overflow & 2) ? std::string(": more than 4088 contact layers") : std::string(": inconsistent contact tables (internal error)")) +
                  " (raise dc_params::max_self_contacts and repeat the step)");
  return DC_OK;
}

FwdArgs fwd_args(dc_ctx *c, int slot) {
  const size_t se = slot_elems(c), sp = (size_t) c->B * c->host.N;
  FwdArgs A;
  A.x_in = c->X + se * slot; A.v_in = c->V + se * slot;
  A.x_out = c->X + se * (slot + 1); A.v_out = c->V + se * (slot + 1);
  A.rec_f = c->F + se * (slot + 1); A.rec_r = c->R + se * (slot + 1); A.rec_n = c->NRM + se * (slot + 1);
  A.rec_prim = c->PRIM + sp * (slot + 1);
  A.x_fixed = c->xf_cur; A.mu = c->mu; A.fu = c->fu_set ? c->fu : nullptr; A.fv = c->fv_set ? c->fv : nullptr;
  A.fv2 = c->fv2_set ? c->fv2 : nullptr;
  A.fv_scale = nullptr; A.slot_xfix = 0; A.slot_fu = 0; A.slot_fvs = 0;
  A.pcen = pc_slot(c, slot + 1); A.slot_pcen = pc_elems(c);      // (enqueue_forward_steps has brought the rows up to date)
  A.pvel = c->PV ? pv_slot(c, slot + 1) : nullptr; A.slot_pvel = c->PV ? pv_elems(c) : 0;      // (likewise; null = no velocity was ever set)
  A.pshp = c->PS ? ps_slot(c, slot + 1) : nullptr; A.slot_pshp = c->PS ? ps_elems(c) : 0;      // (likewise; null = no shape was ever set: DevPrim's)
  // scheduled values of this step (dc_set_*_schedule) take precedence over the current ones
  if (c->S.Af > 0 && c->sched_xf[slot + 1]) A.x_fixed = xf_slot(c, slot + 1);
  if (c->sched_fu[slot + 1]) A.fu = c->FU_S + (size_t) c->B * 3 * (slot + 1);
  if (c->sched_fvs[slot + 1] && A.fv) A.fv_scale = c->FVS_S + (size_t) c->B * (slot + 1);
  A.stats = c->fstats + (size_t) c->B * (slot + 1);
  A.self = self_slot(c, slot + 1);
  A.fwd_tol = (float) c->params.forward_tol;
  A.cg_tol = (float) (c->params.cg_rel_tol > 0 ? c->params.cg_rel_tol : 1e-4);
  A.pd_cap = pd_cap(c);
  A.cg_max = c->params.cg_max_iter > 0 ? c->params.cg_max_iter : 500;
  A.stall_window = c->params.stall_window > 0 ? c->params.stall_window : 0x7fffffff;   // off by default: reference semantics
  static const bool seed_on = env_not_off("DC_CG_SEED", true);     // development switch
  A.cg_seed = seed_on ? 1 : 0;
  A.self_full = env_on("DC_FWD_SELFFULL", false);
  A.nsteps = 1; A.inline_detect = 0; A.slot_state = se; A.slot_prim = sp; A.slot_stats = (size_t) c->B;
  A.slot_self = (size_t) c->B * c->self_cap; A.slot_meta = (size_t) c->B * kMetaStride;
  return A;
}
// where a backward step takes the loss gradient w.r.t. the state it started from: nowhere, the caller's init gradients (IX / IV), or the
// seed schedule's entry of that state, when there is one (dc_set_seed_schedule)
enum class Seeds { none, init, schedule };
BwdArgs bwd_args(dc_ctx *c, int slot, bool is_start, Seeds seeds) {
  const size_t se = slot_elems(c), sp = (size_t) c->B * c->host.N;
  BwdArgs A;
  A.x_new = c->X + se * slot; A.rec_f = c->F + se * slot; A.rec_n = c->NRM + se * slot;
  A.rec_prim = c->PRIM + sp * slot; A.mu = c->mu;
  A.self = self_slot(c, slot);
  A.gx = c->GX; A.gv = c->GV;
  A.ix = nullptr; A.iv = nullptr; A.slot_ix = 0;
  if (seeds == Seeds::init) { A.ix = c->IX; A.iv = c->IV; }
  if (seeds == Seeds::schedule && c->SEEDX && c->sched_seed[slot - 1]) { A.ix = seedx_slot(c, slot - 1); A.iv = seedv_slot(c, slot - 1); A.slot_ix = se; }
  A.d_xfixed = dxf_slot(c, slot); A.d_mu = c->DMU;
  A.d_param = dpar_slot(c, slot);
  A.x_fixed = xf_slot(c, slot);
  A.x_prev = c->X + se * (slot - 1); A.v_prev = c->V + se * (slot - 1); A.v_new = c->V + se * slot; A.stats = c->bstats + (size_t) c->B * slot;
  A.bwd_tol = (float) c->params.backward_tol;
  A.cg_tol = (float) (c->params.cg_rel_tol > 0 ? c->params.cg_rel_tol : 1e-4);
  A.clip_thr = (float) c->params.gradient_clipping_threshold;
  A.it_cap = c->params.adjoint_iter_cap > 0 ? c->params.adjoint_iter_cap : 400;   // Simulation.cpp:1562
  A.cg_max = c->params.cg_max_iter > 0 ? c->params.cg_max_iter : 500;
  A.is_start = is_start; A.clip = c->params.gradient_clipping;
  A.start_at = c->start_slot + 1;
  A.mode = c->params.adjoint_mode;
  A.rel_tol = (float) (c->params.adjoint_rel_tol > 0 ? c->params.adjoint_rel_tol : 1e-6);
  A.stall_window = c->params.stall_window > 0 ? c->params.stall_window : 0x7fffffff;   // off by default: reference semantics
  A.block_pre = env_not_off("DC_BLOCK_PRE", c->params.adjoint_block_precond != 0);     // (development switches)
  A.fp32_only = env_on("DC_ADJ_FP32", c->params.adjoint_fp32_only != 0);
  A.dense_y = env_on("DC_ADJ_DENSEY", false);
  A.verify_all = env_on("DC_ADJ_VERIFY", false);
  A.warm = env_on("DC_ADJ_WARM", false);
  A.cg_first = env_on("DC_ADJ_CG", true);                                                     // (A/B switch: 0 = BiCGSTAB correction solves only)
  A.ycap = 0; A.ybase = 0;                                                                                    // (set by the launch, dc_adjoint.hip)
  A.ytab = env_not_off("DC_ADJ_RESIDENT", true) ? std::max(env_int("DC_TEST_YTAB_CAP", 0x7fffffff), 0) : 0;      // (A/B switch; test hook: cap of the tables' floats)
  A.nsteps = 1; A.slot = slot;
  const bool inj = c->inj_slot == slot && c->INJ_X;
  A.inj_x = inj ? c->INJ_X : nullptr; A.inj_f = inj ? c->INJ_F : nullptr; A.inj_n = inj ? c->INJ_N : nullptr;
  A.inj_sn = inj ? c->INJ_SN : nullptr; A.inj_sd = inj ? c->INJ_SD : nullptr;
  A.ys = (c->keep_y && c->YS) ? c->YS + se * slot : nullptr;
  A.adj_path = c->adj_path;
  A.pvel = c->PV ? pv_slot(c, slot) : nullptr; A.d_pvel = c->PV ? dpv_slot(c, slot) : nullptr; A.slot_pvel = c->PV ? pv_elems(c) : 0;
  A.slot_state = se; A.slot_prim = sp; A.slot_self = (size_t) c->B * c->self_cap; A.slot_meta = (size_t) c->B * kMetaStride;
  A.slot_param = (size_t) c->B * 8; A.slot_xf = xf_elems(c); A.slot_stats = (size_t) c->B;
  return A;
}


// ---- split execution (dc_cluster.h): choice of K, tables, launches ------------------------------------------------------------
void free_cluster(dc_ctx *c) {
  for (void *p : c->cl.allocs) (void) hipFree(p);
  c->cl = ClusterSet();
}

// The tables of a split plan and the exchange area of one launch, uploaded; c->cl.ok only when all of it is there (what a failed allocation
// leaves behind stays in c->cl.allocs for free_cluster).
int upload_cluster(dc_ctx *c, const ClusterPlan &P) {
  ClusterSet &cl = c->cl;
  DevCluster &D = cl.D;
  std::memset(&D, 0, sizeof(D));
  D.K = P.K; D.R = P.R; D.HB = P.HB; D.wpp = P.wpp; D.nb = P.nb; D.xch_stride = P.xch_stride; D.pk_vpt = P.pk_vpt;
  D.spin_limit = P.spin_limit; D.redundant_self = P.redundant_self; D.test_drop = P.test_drop; D.test_skew = P.test_skew;
  const HostWindows &HW = P.win;
  const HostPackets &HP = P.pk;
  D.nwin = HW.nwin; D.win_vcap = HW.vcap; D.win_nrcap = HW.nrcap; D.win_lds_bytes = (int) HW.lds_bytes;
  // (host vector, the DevCluster pointer it goes behind): int and float tables alike are flat arrays of 4-byte elements
  const struct { const void *src; size_t count; void *dst; } tables[] = {
    {HW.win.data(), HW.win.size(), &D.win}, {HW.tri_rec.data(), HW.tri_rec.size(), &D.wtri_rec}, {HW.tri_D.data(), HW.tri_D.size(), &D.wtri_D},
    {HW.bend_rec.data(), HW.bend_rec.size(), &D.wbend_rec}, {HW.bend_w.data(), HW.bend_w.size(), &D.wbend_w},
    {HW.tri_Dlo.data(), HW.tri_Dlo.size(), &D.wtri_Dlo}, {HW.bend_lo.data(), HW.bend_lo.size(), &D.wbend_lo},
    {HW.inc.data(), HW.inc.size(), &D.winc}, {HW.inc_ptr.data(), HW.inc_ptr.size(), &D.winc_ptr}, {HW.inc_n.data(), HW.inc_n.size(), &D.winc_n},
    {HP.pk.data(), HP.pk.size(), &D.pk}, {HP.pk_ptr.data(), HP.pk_ptr.size(), &D.pk_ptr}, {HP.pk_n.data(), HP.pk_n.size(), &D.pk_n},
    {HP.sq_dinv.data(), HP.sq_dinv.size(), &D.sq_dinv}};
  static_assert(sizeof(int) == 4 && sizeof(float) == 4, "4-byte table elements");
  int rc;
  for (const auto &t : tables) {
    int *p = nullptr;
    if ((rc = dev_alloc(c, cl.allocs, &p, t.count))) return rc;
    if (t.count) HIPCHK(c, hipMemcpy(p, t.src, t.count * 4, hipMemcpyHostToDevice));
    std::memcpy(t.dst, &p, sizeof(p));
  }
  if ((rc = dev_alloc(c, cl.allocs, &D.xch, P.xch_bytes / sizeof(v4i)))) return rc;
  if ((rc = dev_alloc(c, cl.allocs, &D.err, 4))) return rc;
  if ((rc = dev_alloc(c, cl.allocs, &D.self_path, 2 * (size_t) c->B))) return rc;
  DevCluster *dD = nullptr;
  if ((rc = dev_alloc(c, cl.allocs, &dD, 1))) return rc;
  D.self_dev = dD;
  HIPCHK(c, hipMemcpy(dD, &D, sizeof(DevCluster), hipMemcpyHostToDevice));
  cl.K = P.K; cl.nb = P.nb; cl.xch_bytes = P.xch_bytes;
  cl.ok = true;
  return DC_OK;
}

// Which deflation space the forward solve wants (dc_params::forward_deflation: -1 decide by the probe solve, 0 never, > 0 always; the
// development switch DC_DEFLATION overrides it: 0 = off, 1 = always) — one rule for device and host-only contexts, read at every build.
static int deflation_want(const dc_params &p) {
  if (env_set("DC_DEFLATION")) return env_int("DC_DEFLATION", 0) > 0 ? 16 : 0;
  return p.forward_deflation > 0 ? 16 : p.forward_deflation;
}
// HostDeflation::build through the context's cache (key: the scalar system matrix, the request, the padded row count)
static bool build_deflation_cached(dc_ctx *c, const HostSystem &H, int want, int rows_padded, HostDeflation **out) {
  uint64_t h = 1469598103934665603ull;
  auto mix = [&](const void *q, size_t n) { const unsigned char *b = (const unsigned char *) q; for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 1099511628211ull; } };
  mix(&H.N, sizeof(int)); mix(&want, sizeof(int)); mix(&rows_padded, sizeof(int));
  mix(H.P_ptr.data(), H.P_ptr.size() * sizeof(H.P_ptr[0])); mix(H.P_col.data(), H.P_col.size() * sizeof(H.P_col[0]));
  mix(H.P_val.data(), H.P_val.size() * sizeof(H.P_val[0])); mix(H.mass.data(), H.mass.size() * sizeof(H.mass[0]));
  if (!c->defl_cache_valid || c->defl_key != h) {
    c->defl_cache_built = c->defl_cache.build(H, want, rows_padded);
    c->defl_key = h; c->defl_cache_valid = true;
  }
  *out = &c->defl_cache;
  return c->defl_cache_built;
}

// What both kinds of context take from the table plan: the DevSystem fields of the kernel set dc_get_layout reports and of what sizes the
// batch, and the forward step's kernel instance (dc_kernelplan.h; after set_deflation)
static void set_decisions(dc_ctx *c, const HostTables &plan) {
  DevSystem &S = c->S;
  c->facts = plan.facts(c->host.N);
  c->fwd = forward_choice(c->facts, kernel_switches());
  S.win_ok = plan.win_ok; S.nwin = plan.nwin; S.pk_ok = plan.pk_ok; S.pk_vpt = plan.pk_vpt; S.pk_threads = plan.pk_threads;
  S.pk_ofs = plan.pk_ofs; S.win_rows = plan.bend_rows;
  S.pk_tpl = plan.pk_tpl; S.pk_guard = plan.pk_guard_bytes;
  for (int j = 0; j < kPkTplSlots; j++) S.pk_tpl_off[j] = plan.pk_tpl ? plan.pk.tpl_off[j] : 0;
  S.fwd_defl = plan.fwd_defl; S.adj_coarse = plan.adj_coarse; S.dense_ld = plan.dense_ld;
  S.max_radii = plan.max_radii; S.self_cap = plan.self_cap; S.self_lds = plan.self_lds;
}

// The split of this batch (dc_clusterplan.h): the development switches are read here, once per dc_alloc_batch; DC_CLUSTER=k forces k parts
// (0 / 1 = off).
int choose_cluster(dc_ctx *c) {
  free_cluster(c);
  ClusterSwitches sw;
  sw.forced = env_int("DC_CLUSTER", -1);
  sw.redundant_self = env_on("DC_SELF_REDUNDANT", true);
  sw.spin_ms = env_int("DC_TEST_SPIN_MS", 0);                  // test hooks
  sw.test_drop = env_on("DC_TEST_DROP_PART", false);
  sw.test_skew = env_int("DC_TEST_SKEW_PART", -1);
  ClusterPlan plan;
  plan.build(c->host, c->bandwidth, c->B, c->cus, c->host_only, c->S.pk_ok != 0, c->S.win_ok != 0, c->S.dense_inv != nullptr, sw);
  return plan.ok ? upload_cluster(c, plan) : DC_OK;
}

// The error word of the split kernels is sticky on the device: it is zero until an exchange times out and is cleared only AFTER that
// has been reported — an asynchronous call (dc_step_forward without statistics, dc_step_backward ...) can therefore not lose a
// time-out to the next call: whichever synchronising call comes first (statistics, dc_get_state / gradient / record, dc_sync) reports it.
int cluster_check(dc_ctx *c) {       // after a synchronisation
  if (!c->cl.ok) return DC_OK;
  unsigned e[4] = {0, 0, 0, 0};
  HIPCHK(c, hipMemcpy(e, c->cl.D.err, sizeof(e), hipMemcpyDeviceToHost));
  if (e[0]) HIPCHK(c, hipMemset(c->cl.D.err, 0, 16));
  if (e[0]) return fail(c, DC_ERR_HIP, "split kernels: an inter-workgroup exchange timed out (waiting for sequence " + std::to_string(e[1]) + ", saw tag " +
                        std::to_string(e[2]) + ", site " + std::to_string(e[3] & 255u) + ", part " + std::to_string((e[3] >> 8) & 15u) + ", granule " +
                        std::to_string(e[3] >> 12) + "; set DC_CLUSTER=1 to run one workgroup per rollout)");
  return DC_OK;
}

bool use_cluster_fwd(const dc_ctx *c) { return c->cl.ok; }
bool use_cluster_bwd(const dc_ctx *c) { return c->cl.ok && c->params.adjoint_mode == 1; }

// adjoint_mode 2 needs the whole K of a rollout as a dense matrix: meshes of at most kDenseMaxN vertices
int check_dense_mode(dc_ctx *c, int mode, int N, const char *who) {
  if (mode == 2 && N > kDenseMaxN)
    return fail(c, DC_ERR_INVALID, std::string(who) + ": adjoint_mode 2 (dense direct adjoint solve) is limited to meshes of at most " +
                std::to_string(kDenseMaxN) + " vertices; this mesh has " + std::to_string(N));
  return DC_OK;
}

// adjoint_mode 3 keeps K of a rollout in band storage: the one rule of dc_bandplan.h (band bytes within the chunk budget, the step kernel's
// right-hand side and panel block within a workgroup's LDS). The matrix bandwidth is known once dc_build has planned the tables.
int check_band_mode(dc_ctx *c, int mode, int extra, const char *who) {
  if (mode != 3) return DC_OK;
  const BandPlan bp = band_plan(c->host.N, c->bandwidth, extra);
  if (bp.ok) return DC_OK;
  return fail(c, DC_ERR_INVALID, std::string(who) + ": adjoint_mode 3 (banded direct adjoint solve) does not take this mesh (" + std::to_string(c->host.N) +
              " vertices, matrix bandwidth " + std::to_string(c->bandwidth) + " + " + std::to_string(extra) + "): the band of one rollout needs " +
              std::to_string(bp.bytes) + " bytes of the " + std::to_string(kBandBudgetBytes) + " allowed, the solve " + std::to_string(bp.lds_bytes) +
              " bytes of LDS of the " + std::to_string(kBandLdsBytes) + " allowed");
}

// Scratch of the dense adjoint solve, on first use: as many rollouts per chunk as fit a budget of 8 GB (DC_DENSE_CHUNK=k caps the chunk at
// k rollouts, development switch: the chunked path on small batches). DC_DENSE_FLAG=b, development switch read by enqueue_dense_adjoint:
// rollout b is marked as if its factorisation had met a zero pivot (no valid scene does), so its adjoint step takes the fp64 BiCGSTAB
// fall-back from u = 0; the other rollouts are untouched.
int dense_ensure(dc_ctx *c) {
  if (c->dense.K) return DC_OK;
  const int N = c->host.N, ld = dense_adj_ld(N), cap = std::max(c->self_cap, 1);
  const size_t per = (size_t) ld * ld * sizeof(double) + (size_t) ld * sizeof(int) + sizeof(int) + (size_t) 9 * N * sizeof(double) +
                     (size_t) 9 * cap * sizeof(double);
  const size_t budget = (size_t) 8 << 30;
  int nb = (int) std::max<size_t>(1, std::min<size_t>((size_t) c->B, budget / per));
  const int chunk = env_int("DC_DENSE_CHUNK", 0);
  if (chunk > 0) nb = std::min(nb, chunk);
  int rc;
  DenseAdjWork &D = c->dense;
  D.ld = ld;
  if ((rc = dev_alloc(c, c->batch_allocs, &D.K, (size_t) nb * ld * ld))) return rc;
  if ((rc = dev_alloc(c, c->batch_allocs, &D.piv, (size_t) nb * ld))) return rc;
  if ((rc = dev_alloc(c, c->batch_allocs, &D.flag, (size_t) nb))) return rc;
  if ((rc = dev_alloc(c, c->batch_allocs, &D.pm, (size_t) nb * 9 * N))) return rc;
  if ((rc = dev_alloc(c, c->batch_allocs, &D.sg, (size_t) nb * 9 * cap))) return rc;
  c->dense_nb = nb;
  c->dense_timing = env_on("DC_DENSE_TIMES", false);
  if (c->dense_timing)
    for (auto &e : c->ev_d) if (!e) HIPCHK(c, hipEventCreate(&e));
  return DC_OK;
}

// Scratch of the band adjoint solve, on first use and again after dc_set_adjoint_band changed the band: chunks under the dense solve's budget
// and switches (DC_DENSE_CHUNK, DC_DENSE_TIMES; DC_DENSE_FLAG in enqueue_dense_adjoint).
int band_ensure(dc_ctx *c) {
  int rc;
  if ((rc = check_band_mode(c, 3, c->band_extra, "adjoint_mode 3"))) return rc;
  const BandPlan bp = band_plan(c->host.N, c->bandwidth, c->band_extra);
  if (c->band.AB && c->band.kl == bp.kl) return DC_OK;
  if (c->band.AB) HIPCHK(c, hipStreamSynchronize(c->stream));
  free_pool(c->band_allocs);
  c->band = BandAdjWork{};
  const int N = c->host.N, n = 3 * N, cap = std::max(c->self_cap, 1);
  BandAdjWork D{};
  D.n = n; D.kl = bp.kl; D.ldab = bp.ldab; D.pld = band_pld(bp.kl); D.npiv = band_round16(n); D.sub_cols = bp.sub_cols;
  const size_t per = (size_t) bp.bytes + (size_t) D.npiv * sizeof(int) + sizeof(int) + (size_t) 9 * N * sizeof(double) + (size_t) 9 * cap * sizeof(double) +
                     (size_t) 2 * kBandPanel * D.pld * sizeof(double);
  int nb = (int) std::max<size_t>(1, std::min<size_t>((size_t) c->B, (size_t) kBandBudgetBytes / per));
  const int chunk = env_int("DC_DENSE_CHUNK", 0);
  if (chunk > 0) nb = std::min(nb, chunk);
  if ((rc = dev_alloc(c, c->band_allocs, &D.AB, (size_t) nb * D.ldab * n))) return rc;
  if ((rc = dev_alloc(c, c->band_allocs, &D.piv, (size_t) nb * D.npiv))) return rc;
  if ((rc = dev_alloc(c, c->band_allocs, &D.flag, (size_t) nb))) return rc;
  if ((rc = dev_alloc(c, c->band_allocs, &D.pm, (size_t) nb * 9 * N))) return rc;
  if ((rc = dev_alloc(c, c->band_allocs, &D.sg, (size_t) nb * 9 * cap))) return rc;
  if ((rc = dev_alloc(c, c->band_allocs, &D.panel, (size_t) nb * 2 * kBandPanel * D.pld))) return rc;
  c->band = D;
  c->band_nb = nb;
  c->dense_timing = env_on("DC_DENSE_TIMES", false);
  if (c->dense_timing)
    for (auto &e : c->ev_d) if (!e) HIPCHK(c, hipEventCreate(&e));
  return DC_OK;
}

// one mode-2 or mode-3 backward step (A.nsteps == 1): per chunk of rollouts assemble K -> factor -> adjoint step with the factors. The
// chunk loop, DC_DENSE_FLAG and DC_DENSE_TIMES are the same for both; the modes differ in the three launches (`launch3`: phase 0 / 1 / 2 of
// rollouts b0 .. b0 + nb - 1, adding its kernel launches to c->dense_launches).
template <typename Launch3>
int direct_adjoint_chunks(dc_ctx *c, int chunk_nb, int *flag, Launch3 launch3) {
  static const int one = 1;
  const int forced = env_int("DC_DENSE_FLAG", -1);
  for (int b0 = 0; b0 < c->B; b0 += chunk_nb) {
    const int nb = std::min(chunk_nb, c->B - b0);
    if (c->dense_timing) HIPCHK(c, hipEventRecord(c->ev_d[0], c->stream));
    HIPCHK(c, hipMemsetAsync(flag, 0, sizeof(int) * nb, c->stream));
    if (forced >= b0 && forced < b0 + nb) HIPCHK(c, hipMemcpyAsync(flag + (forced - b0), &one, sizeof(int), hipMemcpyHostToDevice, c->stream));
    for (int phase = 0; phase < 3; phase++) {
      HIPCHK(c, launch3(phase, b0, nb));
      if (c->dense_timing) HIPCHK(c, hipEventRecord(c->ev_d[phase + 1], c->stream));
    }
    HIPCHK(c, hipGetLastError());
    if (c->dense_timing) {
      HIPCHK(c, hipEventSynchronize(c->ev_d[3]));
      for (int k = 0; k < 3; k++) {
        float ms = 0;
        HIPCHK(c, hipEventElapsedTime(&ms, c->ev_d[k], c->ev_d[k + 1]));
        c->dense_ms[k] += ms;
      }
    }
  }
  return DC_OK;
}
int enqueue_dense_adjoint(dc_ctx *c, const BwdArgs &A) {
  const bool band = c->params.adjoint_mode == 3;
  if (A.nsteps != 1) return fail(c, DC_ERR_INVALID, "adjoint_mode 2 / 3 runs one backward step per launch");
  int rc;
  if ((rc = band ? band_ensure(c) : dense_ensure(c))) return rc;
  if (band) {
    const BandAdjWork &D = c->band;
    return direct_adjoint_chunks(c, c->band_nb, D.flag, [&](int phase, int b0, int nb) -> hipError_t {
      if (phase == 0) { launch_band_assemble(c->S, A, c->W.x64, D, b0, nb, c->stream); c->dense_launches += 2; return hipSuccess; }
      if (phase == 1) return launch_band_factor(D, nb, c->stream, &c->dense_launches);
      c->dense_launches += 1;
      return launch_band_adjoint_step(c->S, c->W, A, D, b0, nb, c->stream);
    });
  }
  const DenseAdjWork &D = c->dense;
  const int n = 3 * c->host.N;
  return direct_adjoint_chunks(c, c->dense_nb, D.flag, [&](int phase, int b0, int nb) -> hipError_t {
    if (phase == 0) { launch_dense_assemble(c->S, A, c->W.x64, D, b0, nb, c->stream); c->dense_launches += 2; }
    else if (phase == 1) c->dense_launches += launch_dense_factor(D, n, nb, c->stream);
    else { launch_dense_adjoint_step(c->S, c->W, A, D, b0, nb, c->stream); c->dense_launches += 1; }
    return hipSuccess;
  });
}

// Outcome of a step launcher that was handed a kernel choice (dc_kernelplan.h). The launchers return hipErrorInvalidValue without launching
// when the choice names no instance of this build (development builds compile a subset), else the runtime's error, peeked: it is cleared
// here, which also tells the two apart. Never followed by another kernel family. The message is formatted on failure only.
static int launched(dc_ctx *c, hipError_t e, const char *step, int threads, int rows) {
  const hipError_t runtime = hipGetLastError();
  if (e == hipSuccess) return DC_OK;
  const std::string shape = std::string(step) + " (" + std::to_string(threads) + " threads x " + std::to_string(rows) + " rows, N " + std::to_string(c->facts.N) + ")";
  if (e == hipErrorInvalidValue && runtime == hipSuccess) return fail(c, DC_ERR_HIP, shape + ": this build has no such kernel instance");
  return fail(c, DC_ERR_HIP, shape + ": " + hipGetErrorString(e));
}

int enqueue_pd_step(dc_ctx *c, const FwdArgs &A) {
  c->rw_arrived = -1;      // records are being rewritten: no backward chain continues across a forward step
  {   // a forward step overwrites records: a record handed in from outside for one of them (dc_set_record) is gone
    const long first = (long) ((A.x_out - c->X) / (long) slot_elems(c));
    if (c->inj_slot >= first && c->inj_slot < first + A.nsteps) c->inj_slot = -1;
  }
  if (!use_cluster_fwd(c)) {
    const FwdChoice &ch = c->fwd;
    return launched(c, launch_pd_step(c->S, c->W, A, ch, c->B, c->stream), ch.family == kFwdPacketDeflated ? "forward step, deflated packet kernel" :
                    ch.family == kFwdPacket ? (ch.h16 ? "forward step, packet kernel with halves" : "forward step, packet kernel") :
                    ch.family == kFwdResident ? "forward step, resident kernel" : ch.family == kFwdGlobal ? "forward step, global-memory kernel" :
                    "forward step, no kernel family", ch.threads, ch.vpt);
  }
  const ClFwdChoice ch = cl_forward_choice(c->facts, c->cl.D.pk_vpt, kernel_switches());
  for (int b0 = 0; b0 < c->B; b0 += c->cl.nb) {
    HIPCHK(c, hipMemsetAsync(c->cl.D.xch, 0, c->cl.xch_bytes, c->stream));
    HIPCHK(c, launch_pd_step_cluster(c->S, c->cl.D, c->W, A, ch, b0, std::min(c->cl.nb, c->B - b0), c->stream));
  }
  return DC_OK;
}
int enqueue_adjoint_step(dc_ctx *c, const BwdArgs &A) {
  if (c->params.adjoint_mode == 2 || c->params.adjoint_mode == 3) return enqueue_dense_adjoint(c, A);
  if (!use_cluster_bwd(c)) {
    const AdjChoice ch = adjoint_choice(c->facts, A.mode, A.block_pre != 0, kernel_switches().bwd_threads);
    return launched(c, launch_adjoint_step(c->S, c->W, A, ch, c->B, c->stream), ch.dense ? "adjoint step, explicit inverse" : ch.coarse ? "adjoint step, coarse level" :
                    ch.blk ? "adjoint step, block preconditioner" : "adjoint step", ch.threads, 0);
  }
  const ClAdjChoice ch = cl_adjoint_choice(c->facts, A.block_pre != 0);
  for (int b0 = 0; b0 < c->B; b0 += c->cl.nb) {
    HIPCHK(c, hipMemsetAsync(c->cl.D.xch, 0, c->cl.xch_bytes, c->stream));
    HIPCHK(c, launch_adjoint_step_cluster(c->S, c->cl.D, c->W, A, ch, b0, std::min(c->cl.nb, c->B - b0), c->stream));
  }
  return DC_OK;
}

// DC_FUSE_STEPS=0 (development switch, read once per process): one launch per step in dc_rollout_forward / dc_rollout_backward
bool fuse_steps_enabled() {
  static const bool on = env_not_off("DC_FUSE_STEPS", true);
  return on;
}

// The forward steps slot -> slot + 1 ... -> slot + nsteps, enqueued on the context's stream: the targets of every step that has no schedule entry
// (dc_set_fixed_point_schedule) go from xf_cur into the step's XF slot, then self-collision detection and the step kernel per step, or, fused,
// all steps of a rollout inside ONE launch (detection inlined per step), so that a rollout never waits for the slowest rollout of the batch
// between steps. carry_targets (the rollout call; the per-step calls leave xf_cur alone): later unscheduled steps continue from the last
// scheduled targets. Returns the number of step-kernel launches per chunk of rollouts in *launches.
int enqueue_forward_steps(dc_ctx *c, int slot, int nsteps, bool carry_targets, int *launches) {
  const bool self_on = c->S.contact_enabled && c->S.self_enabled, has_xf = c->S.Af > 0;
  const bool fused = fuse_steps_enabled() && nsteps > 1 && (use_cluster_fwd(c) || c->fwd.fusable);
  const size_t xf_bytes = sizeof(float) * xf_elems(c);
  int rc;
  FwdArgs FA = fwd_args(c, slot);          // fused: points x_fixed / fu / fv_scale at the first step's schedule entries
  if (fused) {      // a schedule (dc_set_*_schedule) has to cover all steps of a fused sweep or none of them
    int nxf = 0, nfu = 0, nfvs = 0, npc = 0, npv = 0, nps = 0, npw = 0;
    for (int k = 1; k <= nsteps; k++) {
      nxf += c->sched_xf[slot + k]; nfu += c->sched_fu[slot + k]; nfvs += c->sched_fvs[slot + k]; npc += c->sched_pc[slot + k]; npv += c->sched_pv[slot + k];
      nps += c->sched_ps[slot + k]; npw += c->sched_pw[slot + k];
    }
    if ((nxf % nsteps) || (nfu % nsteps) || (nfvs % nsteps) || (npc % nsteps) || (npv % nsteps) || (nps % nsteps) || (npw % nsteps))
      return fail(c, DC_ERR_INVALID, "dc_rollout_forward: a fixed-point / force / primitive-offset / primitive-velocity / primitive-shape / primitive-spin schedule covers only part of the steps " + std::to_string(slot) + " .. " + std::to_string(slot + nsteps));
    if (nxf) FA.slot_xfix = xf_elems(c);
    if (nfu) FA.slot_fu = (size_t) c->B * 3;
    if (nfvs && FA.fv_scale) FA.slot_fvs = (size_t) c->B;
    FA.nsteps = nsteps; FA.inline_detect = self_on ? 1 : 0;
  }
  for (int k = 0; k < nsteps; k++) {
    if (has_xf && !c->sched_xf[slot + k + 1]) HIPCHK(c, hipMemcpyAsync(xf_slot(c, slot + k + 1), c->xf_cur, xf_bytes, hipMemcpyDeviceToDevice, c->stream));
    // the primitive centres of a step without a schedule entry are the current ones; its row already holds them unless offsets were set since
    if (c->S.nprim > 0 && !c->sched_pc[slot + k + 1] && c->pc_row_gen[slot + k + 1] != c->pc_gen) {
      HIPCHK(c, hipMemcpyAsync(pc_slot(c, slot + k + 1), c->pc_cur, sizeof(float) * pc_elems(c), hipMemcpyDeviceToDevice, c->stream));
      c->pc_row_gen[slot + k + 1] = c->pc_gen;
    }
    // likewise the obstacle motion, once a context has it: the row of an unscheduled step takes the current set, each half (velocity, spin)
    // where that half has no schedule entry
    if (c->PV) {
      const bool sv = c->sched_pv[slot + k + 1], sw = c->sched_pw[slot + k + 1];
      if (!sv && !sw) HIPCHK(c, hipMemcpyAsync(pv_slot(c, slot + k + 1), c->pv_cur, sizeof(float) * pv_elems(c), hipMemcpyDeviceToDevice, c->stream));
      else if (!sv || !sw)
        HIPCHK(c, hipMemcpy2DAsync(pv_slot(c, slot + k + 1) + (sv ? 3 : 0), sizeof(float) * kPvRow, c->pv_cur + (sv ? 3 : 0), sizeof(float) * kPvRow,
                                   sizeof(float) * 3, pv_rows(c), hipMemcpyDeviceToDevice, c->stream));
    }
    // and the obstacle shapes: like the centres, a row is copied only when the current set changed since it was written
    if (c->PS && !c->sched_ps[slot + k + 1] && c->ps_row_gen[slot + k + 1] != c->ps_gen) {
      HIPCHK(c, hipMemcpyAsync(ps_slot(c, slot + k + 1), c->ps_cur, sizeof(float) * ps_elems(c), hipMemcpyDeviceToDevice, c->stream));
      c->ps_row_gen[slot + k + 1] = c->ps_gen;
    }
    if (fused) continue;
    if (k) FA = fwd_args(c, slot + k);
    if (self_on) launch_self_detect(c->S, c->W, FA, c->B, c->stream);
    if ((rc = enqueue_pd_step(c, FA))) return rc;
  }
  if (fused && (rc = enqueue_pd_step(c, FA))) return rc;
  if (carry_targets && has_xf && c->sched_xf[slot + nsteps])
    HIPCHK(c, hipMemcpyAsync(c->xf_cur, xf_slot(c, slot + nsteps), xf_bytes, hipMemcpyDeviceToDevice, c->stream));
  if (launches) *launches = fused ? 1 : nsteps;
  return DC_OK;
}

// drops the read-out weights (both pointers NULL, dc_clear_schedules): enqueued, the tables keep their memory
int clear_readout_gradients(dc_ctx *c) {
  std::fill(c->sched_rw.begin(), c->sched_rw.end(), 0);
  c->rw_arrived = -1;
  if (c->rw_has) HIPCHK(c, hipMemsetAsync(c->rw_has, 0, (size_t) c->tape + 1, c->stream));
  return DC_OK;
}
ReadoutAdjArgs readout_adjoint_args(dc_ctx *c, int slot, int first) {
  ReadoutAdjArgs A;
  A.X = c->X; A.V = c->V; A.F = c->F; A.NRM = c->NRM; A.PRIM = c->PRIM; A.PC = c->PC; A.PV = c->PV; A.XF = c->XF; A.mu = c->mu;
  A.WJ = c->RWJ; A.WW = c->RWW; A.has = c->rw_has;
  A.B = c->B; A.slot = slot; A.first = first;
  const bool inj = c->inj_slot >= first - 1 && c->inj_slot <= slot && c->INJ_X;
  A.inj_x = inj ? c->INJ_X : nullptr; A.inj_f = inj ? c->INJ_F : nullptr; A.inj_n = inj ? c->INJ_N : nullptr; A.inj_slot = inj ? c->inj_slot : -1;
  A.gx = c->GX; A.rsx = c->RSX; A.rsv = c->RSV;
  A.DPAR = c->DPAR; A.DXF = c->DXF; A.YS = (c->keep_y && c->YS) ? c->YS : nullptr; A.DMU = c->DMU; A.DPV = c->PV ? c->DPV : nullptr;
  return A;
}

// The backward steps through the records slot, slot - 1 ... slot - nsteps + 1, enqueued on the context's stream: dL_dxfixed of those slots is
// zeroed (the kernels add to it; DMU is the caller's: the per-step calls zero it, a sweep accumulates into what dc_seed_gradient / dc_set_gradient
// zeroed), then one launch per step or, fused, the whole sweep of a rollout in ONE launch. A record handed in from outside (dc_set_record) gets
// a launch of its own, and so does every step of adjoint_mode 2 (assemble -> factor -> step). seeds: where the steps take the loss gradient
// w.r.t. the state they started from (the rollout call: the seed schedule, which has to cover all steps of the sweep or none; the per-step
// calls: their init gradients or nothing). is_start: null = the step that started from the trajectory's initial state (isStart,
// Simulation.cpp:3947). Returns the number of step-kernel launches per chunk of rollouts in *launches.
int enqueue_backward_steps(dc_ctx *c, int slot, int nsteps, Seeds seeds, const bool *is_start, int *launches) {
  const int first = slot - nsteps + 1;
  int rc;
  if (seeds == Seeds::schedule && c->SEEDX) {
    int ns = 0;
    for (int s = first; s <= slot; s++) ns += c->sched_seed[s - 1];
    if (ns % nsteps) return fail(c, DC_ERR_INVALID, "dc_rollout_backward: the seed schedule covers only part of the slots " + std::to_string(first - 1) + " .. " + std::to_string(slot - 1));
  }
  if (c->S.Af > 0) HIPCHK(c, hipMemsetAsync(dxf_slot(c, first), 0, sizeof(float) * xf_elems(c) * nsteps, c->stream));
  const bool inj_inside = c->inj_slot >= first && c->inj_slot <= slot;
  const bool fused = fuse_steps_enabled() && nsteps > 1 && !inj_inside && c->params.adjoint_mode != 2 && c->params.adjoint_mode != 3;
  auto start_of = [&](int s) { return is_start ? *is_start : s == c->start_slot + 1; };
  // A record of the sweep carries read-out weights (dc_set_contact_readout_gradients): the seed pass adds the read-out's part of the loss gradient
  // to the engine's own seed rows of the states slot - 1 .. first - 1, which start as the caller's entries (schedule, init gradients or zeros) and
  // which every step of this sweep then reads in their place; the parameter pass follows the steps. The gradient a call leaves is that of the
  // state it ARRIVES at, first - 1, and holds the read-out's part of record first - 1 (its row is a seed row like the others): a call that starts
  // where the last one arrived (a chain of per-step calls or of sweeps) finds it in the carried gradient, every other call adds the part of its
  // top record to the carried gradient itself. Either way the part is added to the caller's entry first and enters the step's fp64 sum as one
  // fp32 vector: a fused sweep and a chain of per-step calls over the same tape give the same bits.
  bool rw = false;
  if (c->RSV) for (int s = std::max(first - 1, 1); s <= slot; s++) rw = rw || c->sched_rw[s];
  const bool top_done = rw && c->rw_arrived == slot;
  c->rw_arrived = (rw && first - 1 >= 1 && c->sched_rw[first - 1]) ? first - 1 : -1;
  c->rw_launches = 0;
  const size_t se = slot_elems(c);
  ReadoutAdjArgs RA;
  if (rw) {
    float *bx = c->RSX + se * (first - 1), *bv = c->RSV + se * (first - 1);
    const size_t bytes = sizeof(float) * se * nsteps;
    if (seeds == Seeds::schedule && c->SEEDX && c->sched_seed[slot - 1]) {
      HIPCHK(c, hipMemcpyAsync(bx, seedx_slot(c, first - 1), bytes, hipMemcpyDeviceToDevice, c->stream));
      HIPCHK(c, hipMemcpyAsync(bv, seedv_slot(c, first - 1), bytes, hipMemcpyDeviceToDevice, c->stream));
    } else if (seeds == Seeds::init) {
      for (int k = 0; k < nsteps; k++) {
        HIPCHK(c, hipMemcpyAsync(bx + se * k, c->IX, sizeof(float) * se, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(bv + se * k, c->IV, sizeof(float) * se, hipMemcpyDeviceToDevice, c->stream));
      }
    } else {
      HIPCHK(c, hipMemsetAsync(bx, 0, bytes, c->stream));
      HIPCHK(c, hipMemsetAsync(bv, 0, bytes, c->stream));
    }
    RA = readout_adjoint_args(c, slot, first);
    RA.top_done = top_done ? 1 : 0;
    launch_readout_adjoint(c->S, c->W, RA, 0, c->stream);
    HIPCHK(c, hipGetLastError());
  }
  auto args_of = [&](int s) {
    BwdArgs A = bwd_args(c, s, start_of(s), seeds);
    if (rw) { A.ix = c->RSX + se * (s - 1); A.iv = c->RSV + se * (s - 1); A.slot_ix = se; }
    return A;
  };
  if (fused) {
    BwdArgs A = args_of(slot);
    A.nsteps = nsteps;
    if ((rc = enqueue_adjoint_step(c, A))) return rc;
  } else {
    for (int s = slot; s >= first; s--)
      if ((rc = enqueue_adjoint_step(c, args_of(s)))) return rc;
  }
  if (rw) {
    launch_readout_adjoint(c->S, c->W, RA, 1, c->stream);
    HIPCHK(c, hipGetLastError());
    c->rw_launches = 2;
  }
  if (launches) *launches = fused ? 1 : nsteps;
  return DC_OK;
}

// The bracket of dc_kernel_times around the enqueues of a rollout call: begin before the first, end after the last. end waits for the sweep,
// adds its time and its launches (`launches` per chunk of rollouts of the split kernels; adjoint_mode 2: what enqueue_dense_adjoint counted)
// and reports a time-out of the split kernels.
int kernel_time_begin(dc_ctx *c) {
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipEventRecord(c->ev_a, c->stream));
  c->dense_mark = c->dense_launches;
  return DC_OK;
}
int kernel_time_end(dc_ctx *c, bool bwd, int launches) {
  HIPCHK(c, hipEventRecord(c->ev_b, c->stream));
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventSynchronize(c->ev_b));
  float ms = 0;
  HIPCHK(c, hipEventElapsedTime(&ms, c->ev_a, c->ev_b));
  const int chunks = (bwd ? use_cluster_bwd(c) : use_cluster_fwd(c)) ? (c->B + c->cl.nb - 1) / c->cl.nb : 1;
  (bwd ? c->bwd_ms : c->fwd_ms) += ms;
  (bwd ? c->bwd_launches : c->fwd_launches) += (bwd && (c->params.adjoint_mode == 2 || c->params.adjoint_mode == 3)) ? c->dense_launches - c->dense_mark : launches * chunks;
  if (bwd) c->bwd_launches += c->rw_launches;      // the read-out's seed and parameter passes, when the sweep ran them
  return cluster_check(c);
}

}  // namespace

extern "C" {

const char *dc_version(void) { return "diffcloth_hip 0.1 (gfx950)"; }

void dc_default_params(dc_params *p) {
  std::memset(p, 0, sizeof(*p));
  p->time_step = 1.0 / 90; p->density = 0.1; p->k_stretch = 100; p->k_bend = 0.01; p->k_att = 10000;   // AttachmentSpring.cpp:10
  p->gravity[0] = 0; p->gravity[1] = -9.8; p->gravity[2] = 0;                                          // Simulation.h:356
  p->forward_tol = 1e-7; p->backward_tol = 5e-5;                                                        // Simulation.cpp:17-19
  p->gravity_enabled = 1; p->contact_enabled = 1; p->selfcollision_enabled = 0;
  p->gradient_clipping = 1; p->gradient_clipping_threshold = 16.0;                                      // Simulation.h:330-331
  p->pd_iter_cap = -1; p->adjoint_iter_cap = 400; p->cg_rel_tol = 1e-4; p->cg_max_iter = 500; p->stall_window = 0;
  p->adjoint_mode = 0; p->adjoint_rel_tol = 1e-6; p->adjoint_block_precond = 1; p->adjoint_fp32_only = 0;
  p->max_self_contacts = 0;      /* sized from the mesh in dc_build */
  p->forward_deflation = -1;     /* decided in dc_build by a probe solve */
}

int dc_create(int device_id, dc_ctx **out) {
  if (!out) return DC_ERR_INVALID;
  *out = nullptr;
  if (device_id == -1) {   // host-only context: no device memory, no kernels, no CPU compute path either
    dc_ctx *c = new dc_ctx();
    c->device = -1; c->host_only = true;
    dc_default_params(&c->params);
    std::memset(&c->S, 0, sizeof(c->S));
    std::memset(&c->W, 0, sizeof(c->W));
    *out = c;
    return DC_OK;
  }
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return DC_ERR_HIP;   // no CPU fallback: fail loudly
  if (device_id < 0 || device_id >= count) return DC_ERR_INVALID;
  dc_ctx *c = new dc_ctx();
  c->device = device_id;
  dc_default_params(&c->params);
  std::memset(&c->S, 0, sizeof(c->S));
  std::memset(&c->W, 0, sizeof(c->W));
  if (hipSetDevice(device_id) != hipSuccess || hipStreamCreate(&c->stream) != hipSuccess) { delete c; return DC_ERR_HIP; }
  c->own_stream = c->stream;
  if (hipDeviceGetAttribute(&c->cus, hipDeviceAttributeMultiprocessorCount, device_id) != hipSuccess || c->cus <= 0) c->cus = 256;
  if (hipEventCreate(&c->ev_a) != hipSuccess || hipEventCreate(&c->ev_b) != hipSuccess || hipEventCreate(&c->ev_t0) != hipSuccess ||
      hipEventCreate(&c->ev_t1) != hipSuccess) { delete c; return DC_ERR_HIP; }
  *out = c;
  return DC_OK;
}

int dc_destroy(dc_ctx *c) {
  if (!c) return DC_OK;
  if (c->host_only) { delete c; return DC_OK; }
  (void) hipSetDevice(c->device);
  (void) hipStreamSynchronize(c->stream);
  (void) dc_comm_destroy(c);
  free_cluster(c);
  free_pool(c->table_allocs);
  free_pool(c->batch_allocs);
  free_pool(c->band_allocs);
  (void) hipEventDestroy(c->ev_a); (void) hipEventDestroy(c->ev_b);
  (void) hipEventDestroy(c->ev_t0); (void) hipEventDestroy(c->ev_t1);
  for (hipEvent_t e : c->ev_d) if (e) (void) hipEventDestroy(e);
  (void) hipStreamDestroy(c->own_stream);
  delete c;
  return DC_OK;
}

const char *dc_last_error(const dc_ctx *c) { return c ? c->err.c_str() : "null context"; }

int dc_set_mesh(dc_ctx *c, int n, const double *pos, int t, const int *tris) {
  if (!c) return DC_ERR_INVALID;
  c->built = false;
  c->user_of.clear(); c->dev_of.clear();
  if (!c->host.set_mesh(n, pos, t, tris)) { c->mesh_set = false; return fail(c, DC_ERR_TOPOLOGY, c->host.error); }
  // Renumber the vertices on the device when the caller's numbering couples far-apart indices (typical of
  // modelling-tool exports): the packet-ELL matrix (|i - j| <= 511 over two rings) and the element windows need
  // locality. DC_RENUMBER=0 / 1 forces it off / on (development switch).
  const bool env = env_set("DC_RENUMBER");
  const bool want = env_on("DC_RENUMBER", 2 * mesh_bandwidth(t, tris) > 511);
  if (want) {
    std::vector<int> order = rcm_order(n, t, tris);
    std::vector<int> inv(n);
    for (int k = 0; k < n; k++) inv[order[k]] = k;
    std::vector<int> tri2(3 * (size_t) t);
    for (size_t k = 0; k < tri2.size(); k++) tri2[k] = inv[tris[k]];
    if (2 * mesh_bandwidth(t, tri2.data()) < 2 * mesh_bandwidth(t, tris) || env) {
      std::vector<double> pos2(3 * (size_t) n);
      for (int k = 0; k < n; k++) for (int d = 0; d < 3; d++) pos2[3 * (size_t) k + d] = pos[3 * (size_t) order[k] + d];
      if (!c->host.set_mesh(n, pos2.data(), t, tri2.data())) { c->mesh_set = false; return fail(c, DC_ERR_TOPOLOGY, c->host.error); }
      c->user_of = order; c->dev_of = inv;
    }
  }
  c->mesh_set = true;
  return DC_OK;
}

int dc_set_attachments(dc_ctx *c, int count, const int *vertex) {
  if (!c || count < 0 || (count > 0 && !vertex)) return fail(c, DC_ERR_INVALID, "dc_set_attachments: bad arguments");
  c->att_user.assign(vertex, vertex + count);
  c->built = false;
  return DC_OK;
}

int dc_set_params(dc_ctx *c, const dc_params *p) {
  if (!c || !p) return DC_ERR_INVALID;
  if (!(p->time_step > 0) || !(p->density > 0)) return fail(c, DC_ERR_INVALID, "dc_set_params: time_step and density must be > 0");
  if (c->mesh_set) { const int rc = check_dense_mode(c, p->adjoint_mode, c->host.N, "dc_set_params"); if (rc) return rc; }
  if (c->mesh_set && c->built) { const int rc = check_band_mode(c, p->adjoint_mode, c->band_extra, "dc_set_params"); if (rc) return rc; }
  c->params = *p;
  c->built = false;
  return DC_OK;
}

int dc_set_primitives(dc_ctx *c, int count, const dc_primitive *prims) {
  if (!c || count < 0 || count > kMaxPrims) return fail(c, DC_ERR_INVALID, "dc_set_primitives: at most 8 flattened primitives");
  if (count > 0 && !prims) return fail(c, DC_ERR_INVALID, "dc_set_primitives: null primitive array");
  int discretised = 0;
  for (int k = 0; k < count; k++) {
    if (prims[k].kind < DC_PRIM_SPHERE || prims[k].kind > DC_PRIM_SPHERE_DISCRETIZED) return fail(c, DC_ERR_INVALID, "dc_set_primitives: unknown primitive kind");
    if (prims[k].kind == DC_PRIM_SPHERE_DISCRETIZED) {
      discretised++;
      if (!(prims[k].radius > 0) || prims[k].length < 0 || prims[k].length > 512) return fail(c, DC_ERR_INVALID, "dc_set_primitives: discretised sphere needs radius > 0 and a resolution (length) of 0 or 3 ... 512");
    }
  }
  if (discretised > 1) return fail(c, DC_ERR_INVALID, "dc_set_primitives: at most one discretised sphere per context");
  c->prims.assign(prims, prims + count);
  // compact the caller's group ids to 0..ngroups-1 in order of first appearance
  std::vector<int> seen;
  c->group_of_prim.assign(count, 0);
  for (int k = 0; k < count; k++) {
    int g = -1;
    for (size_t s = 0; s < seen.size(); s++) if (seen[s] == prims[k].group) g = (int) s;
    if (g < 0) { g = (int) seen.size(); seen.push_back(prims[k].group); }
    c->group_of_prim[k] = g;
  }
  c->ngroups = (int) seen.size();
  c->built = false;
  return DC_OK;
}

int dc_build(dc_ctx *c) {
  if (!c) return DC_ERR_INVALID;
  if (!c->mesh_set) return fail(c, DC_ERR_STATE, "dc_build: dc_set_mesh has not been called");
  { const int rc = check_dense_mode(c, c->params.adjoint_mode, c->host.N, "dc_build"); if (rc) return rc; }
  c->inj_slot = -1;      // a rebuilt system no longer matches a record handed in before (dc_set_record)
  const dc_params &p = c->params;
  HostSystem &H = c->host;
  H.att_vertex = c->att_user;
  for (int &a : H.att_vertex) {
    if (a < 0 || a >= H.N) return fail(c, DC_ERR_INVALID, "dc_build: attachment vertex out of range");
    if (!c->dev_of.empty()) a = c->dev_of[a];
  }
  if (!H.build_numerics(p.time_step, p.density, p.k_stretch, p.k_bend, p.k_att)) return fail(c, DC_ERR_TOPOLOGY, H.error);
  // every table and every kernel-set decision comes from the host-side plan (dc_tables.h); the development switches that gate tables are read here
  TableSwitches sw;
  sw.windows = env_not_off("DC_WINDOWS", true);               // 0 keeps the global-memory corner passes
  sw.dense_max_n = env_int("DC_DENSE_MAX_N", kDenseMaxN);     // 0 disables, other values move the size limit
                                                    // (default 2.4 MB: the matrix must stay in every XCD's 4 MB L2 next to the other tables)
  sw.self_lds = env_not_off("DC_SELF_LDS", true);             // 0 = global-memory layer passes
  static const bool adj_coarse = env_int("DC_ADJ_COARSE", 1) != 0;      // 0 = block preconditioner only in the adjoint's fall-back
  sw.adj_coarse = adj_coarse;
  sw.pk_h16 = kernel_switches().pk_h16;                       // (read once per process with the other switches that select kernel instances)
  sw.pk_threads = env_int("DC_PK_THREADS", 0);                // 512 / 768 = threads of the packet kernel for meshes of 9 217 ... 10 240 vertices
  sw.pk_ofs = env_not_off("DC_PK_OFS", true);                 // 0 = the first packet layout (10-bit column deltas) for the halves instances too
  sw.pk_tpl = env_not_off("DC_PK_TPL", true);                 // 0 = a matrix with a column-offset template keeps the byte-offset layout (values and offsets per row)
  sw.bend_rows = env_not_off("DC_BEND_ROWS", true);          // 0 = per-flap bending passes on meshes that are flat at rest too
  HostTables plan;
  plan.build(H, p, sw);
  HostDeflation *HD = nullptr;
  const bool defl = plan.defl_rows > 0 && build_deflation_cached(c, H, deflation_want(p), plan.defl_rows, &HD);
  plan.set_deflation(defl, sw);
  c->bandwidth = plan.bandwidth;
  { const int rc = check_band_mode(c, p.adjoint_mode, c->band_extra, "dc_build"); if (rc) return rc; }
  c->defl_k = HD ? HD->k : 0; c->defl_probe = HD ? HD->probe_iterations : 0;
  DevSystem &S = c->S;
  if (c->host_only) {       // which kernel set this system would get (dc_get_layout): the same plan, nothing uploaded
    std::memset(&S, 0, sizeof(S));
    set_decisions(c, plan);
    c->built = true;
    return DC_OK;
  }
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  free_cluster(c);
  free_pool(c->table_allocs);
  std::memset(&S, 0, sizeof(S));
  set_decisions(c, plan);
  S.N = H.N; S.T = H.T; S.E = H.E; S.Af = (int) H.att_vertex.size(); S.NC = 3 * H.T + 4 * H.E;
  c->d_user_of = nullptr;
  int rc;
  if (!c->user_of.empty()) {
    if ((rc = upload<int>(c, &S.user_of, c->user_of))) return rc;
    if ((rc = upload<int>(c, &S.dev_of, c->dev_of))) return rc;
    c->d_user_of = S.user_of;
  }
  if ((rc = upload<int>(c, &S.tri_v, plan.tri_v))) return rc;
  if ((rc = upload_as<float>(c, &S.tri_D, H.tri_D))) return rc;
  if ((rc = upload<float>(c, &S.tri_w2, H.tri_w2))) return rc;
  if ((rc = upload<int>(c, &S.bend_v, plan.bend_v))) return rc;
  if ((rc = upload_as<float>(c, &S.bend_w, H.bend_w))) return rc;
  if ((rc = upload_as<float>(c, &S.bend_nw, plan.bend_nw))) return rc;
  if ((rc = upload<int>(c, &S.att_vertex, H.att_vertex))) return rc;
  if ((rc = upload<int>(c, &S.att_of_vertex, plan.att_of_vertex))) return rc;
  if ((rc = upload<float>(c, &S.mass, H.mass))) return rc;
  if ((rc = upload<float>(c, &S.dinv, plan.dinv))) return rc;
  // fp64 rest-shape tables of the adjoint's fp64 operator (dc_adjoint64.h), planar, and their fp32 low parts
  if ((rc = upload<double>(c, &S.tri_D64, plan.tri_D64))) return rc;
  if ((rc = upload<double>(c, &S.tri_w2_64, H.tri_w2))) return rc;
  if ((rc = upload<double>(c, &S.bend_w64, plan.bend_w64))) return rc;
  if ((rc = upload<double>(c, &S.bend_nw64, plan.bend_nw64))) return rc;
  if ((rc = upload<double>(c, &S.mass64, H.mass))) return rc;
  if ((rc = upload_as<float>(c, &S.tri_Dlo, plan.tri_Dlo))) return rc;
  if ((rc = upload_as<float>(c, &S.bend_lo, plan.bend_lo))) return rc;
  if ((rc = upload<int>(c, &S.P_ptr, H.P_ptr))) return rc;
  if ((rc = upload<int>(c, &S.P_col, H.P_col))) return rc;
  if ((rc = upload<float>(c, &S.P_val, H.P_val))) return rc;
  if ((rc = upload<int>(c, &S.inc_ptr, H.inc_ptr))) return rc;
  if ((rc = upload<int>(c, &S.inc_idx, H.inc_idx))) return rc;
  if ((rc = upload<float>(c, &S.radii, H.radii))) return rc;
  if ((rc = upload<int>(c, &S.conn_ptr, H.conn_ptr))) return rc;
  if ((rc = upload<int>(c, &S.conn_idx, H.conn_idx))) return rc;
  if ((rc = upload_as<int>(c, &S.ell, plan.ell))) return rc;
  if ((rc = upload<int>(c, &S.ell_ptr, plan.ell_ptr))) return rc;
  if ((rc = upload<int>(c, &S.ell_w, plan.ell_w))) return rc;
  if (plan.win_ok) {
    const HostWindows &HW = plan.win;
    if ((rc = upload_as<int>(c, &S.win, HW.win))) return rc;
    if ((rc = upload_as<int>(c, &S.wtri_rec, HW.tri_rec))) return rc;
    if ((rc = upload_as<float>(c, &S.wtri_D, HW.tri_D))) return rc;
    if ((rc = upload_as<int>(c, &S.wbend_rec, HW.bend_rec))) return rc;
    if ((rc = upload_as<float>(c, &S.wbend_w, HW.bend_w))) return rc;
    if ((rc = upload_as<float>(c, &S.wtri_Dlo, HW.tri_Dlo))) return rc;
    if ((rc = upload_as<float>(c, &S.wbend_lo, HW.bend_lo))) return rc;
    if ((rc = upload_as<int>(c, &S.winc, HW.inc))) return rc;
    if ((rc = upload<int>(c, &S.winc_ptr, HW.inc_ptr))) return rc;
    if ((rc = upload<int>(c, &S.winc_n, HW.inc_n))) return rc;
    if (HW.rows) {
      if ((rc = upload<int>(c, &S.brow_ptr, HW.brow_ptr))) return rc;
      if ((rc = upload<int>(c, &S.brow_col, HW.brow_col))) return rc;
      if ((rc = upload<double>(c, &S.brow_val, HW.brow_val))) return rc;
    }
    S.win_vcap = HW.vcap; S.win_nrcap = HW.nrcap; S.win_lds_bytes = (int) HW.lds_bytes;
  }
  if (plan.pk_ok) {
    if ((rc = upload_as<int>(c, &S.pk, plan.pk.pk))) return rc;
    if ((rc = upload<int>(c, &S.pk_ptr, plan.pk.pk_ptr))) return rc;
    if ((rc = upload<int>(c, &S.pk_n, plan.pk.pk_n))) return rc;
  }
  if ((rc = upload<float>(c, &S.sq_dinv, plan.pk_ok ? plan.pk.sq_dinv : plan.sq_dinv))) return rc;
  if (defl) {
    if ((rc = upload<float>(c, &S.defl_u, HD->U))) return rc;
    if ((rc = upload<float>(c, &S.defl_au, HD->AU))) return rc;
    if ((rc = upload<float>(c, &S.defl_g, HD->G))) return rc;
  }
  if (plan.dense_ld && (rc = upload<float>(c, &S.dense_inv, plan.dense.inv))) return rc;
  S.h = (float) p.time_step; S.k_att = (float) p.k_att;
  S.k_stretch = (float) p.k_stretch; S.k_bend = (float) p.k_bend; S.density = (float) p.density;
  S.gx = p.gravity_enabled ? (float) p.gravity[0] : 0.f;
  S.gy = p.gravity_enabled ? (float) p.gravity[1] : 0.f;
  S.gz = p.gravity_enabled ? (float) p.gravity[2] : 0.f;
  S.h64 = p.time_step; S.k_att64 = p.k_att; S.k_stretch64 = p.k_stretch; S.k_bend64 = p.k_bend; S.density64 = p.density;
  for (int k = 0; k < 3; k++) S.g64[k] = p.gravity_enabled ? p.gravity[k] : 0.0;
  S.contact_enabled = p.contact_enabled; S.self_enabled = p.selfcollision_enabled;
  S.nprim = (int) c->prims.size(); S.ngroups = std::max(c->ngroups, 1);
  S.dsph_tri = nullptr; S.dsph_ntri = 0;
  for (int k = 0; k < S.nprim; k++) {
    const dc_primitive &q = c->prims[k];
    if (q.kind == DC_PRIM_SPHERE_DISCRETIZED) {      // the face table of the sphere's own mesh (Sphere::Sphere, Primitive.cpp:133-216)
      const int res = q.length >= 3 ? (int) q.length : 40;
      const std::vector<double> tab = sphere_mesh_table(q.radius, res);
      if ((rc = upload<double>(c, &S.dsph_tri, tab))) return rc;
      S.dsph_ntri = (int) tab.size() / 12;
    }
    DevPrim &d = S.prims[k];
    d.kind = q.kind; d.group = c->group_of_prim[k]; d.rotates = q.rotates; d.pad = 0;
    d.cx = (float) q.center[0]; d.cy = (float) q.center[1]; d.cz = (float) q.center[2]; d.pad2 = 0.f;
    primitive_shape_to_prim(q, d);      // radius, top_offset, length, corner2: the rule of dc_primshape.h, shared with dc_set_primitive_shapes
  }
  {  // device-resident copy of the descriptor itself (kernels take a pointer to it)
    DevSystem *dS = nullptr;
    if ((rc = dev_alloc(c, c->table_allocs, &dS, 1))) return rc;
    S.self_dev = dS;
    HIPCHK(c, hipMemcpy(dS, &S, sizeof(DevSystem), hipMemcpyHostToDevice));
  }
  c->built = true;
  // a batch allocated for a different system size is no longer valid
  if (c->B > 0) {
    int B = c->B, tape = c->tape;
    c->B = 0;
    return dc_alloc_batch(c, B, tape);
  }
  return DC_OK;
}

int dc_set_solver(dc_ctx *c, double forward_tol, double backward_tol, int gradient_clipping, double clip_threshold, int force_direct_adjoint) {
  if (!c) return DC_ERR_INVALID;
  c->params.forward_tol = forward_tol; c->params.backward_tol = backward_tol;
  c->params.gradient_clipping = gradient_clipping; c->params.gradient_clipping_threshold = clip_threshold;
  // a direct solve is asked for: the dense one (mode 2) and the banded one (mode 3) are, so they stay; otherwise the Krylov direct solve (mode 1)
  c->params.adjoint_mode = force_direct_adjoint ? ((c->params.adjoint_mode == 2 || c->params.adjoint_mode == 3) ? c->params.adjoint_mode : 1) : 0;
  return DC_OK;   // solver knobs are kernel arguments: no rebuild, the batch and its tape stay valid
}

int dc_set_flags(dc_ctx *c, int gravity_enabled, int contact_enabled, int selfcollision_enabled) {
  if (!c) return DC_ERR_INVALID;
  c->params.gravity_enabled = gravity_enabled; c->params.contact_enabled = contact_enabled;
  c->params.selfcollision_enabled = selfcollision_enabled;
  if (!c->built || c->host_only) return DC_OK;
  DevSystem &S = c->S;
  S.gx = gravity_enabled ? (float) c->params.gravity[0] : 0.f;
  S.gy = gravity_enabled ? (float) c->params.gravity[1] : 0.f;
  S.gz = gravity_enabled ? (float) c->params.gravity[2] : 0.f;
  for (int k = 0; k < 3; k++) S.g64[k] = gravity_enabled ? c->params.gravity[k] : 0.0;
  S.contact_enabled = contact_enabled; S.self_enabled = selfcollision_enabled;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy((void *) S.self_dev, &S, sizeof(DevSystem), hipMemcpyHostToDevice));
  return DC_OK;
}

int dc_get_counts(const dc_ctx *c, int *out6) {
  if (!c || !out6 || !c->mesh_set) return DC_ERR_INVALID;
  out6[0] = c->host.N; out6[1] = c->host.T; out6[2] = c->host.E; out6[3] = (int) c->host.att_vertex.size();
  out6[4] = (int) c->host.P_col.size(); out6[5] = c->host.rows();
  return DC_OK;
}
int dc_get_system_matrix(const dc_ctx *c, int *row_ptr, int *col, double *val) {
  if (!c || !c->built) return DC_ERR_STATE;
  const HostSystem &H = c->host;
  if (c->user_of.empty()) {
    std::memcpy(row_ptr, H.P_ptr.data(), sizeof(int) * H.P_ptr.size());
    std::memcpy(col, H.P_col.data(), sizeof(int) * H.P_col.size());
    std::memcpy(val, H.P_val.data(), sizeof(double) * H.P_val.size());
    return DC_OK;
  }
  // back to the caller's numbering: row u = device row dev_of[u], columns relabelled and sorted
  row_ptr[0] = 0;
  std::vector<std::pair<int, double>> row;
  for (int u = 0; u < H.N; u++) {
    const int i = c->dev_of[u];
    row.clear();
    for (int k = H.P_ptr[i]; k < H.P_ptr[i + 1]; k++) row.push_back({c->user_of[H.P_col[k]], H.P_val[k]});
    std::sort(row.begin(), row.end());
    for (size_t k = 0; k < row.size(); k++) { col[row_ptr[u] + k] = row[k].first; val[row_ptr[u] + k] = row[k].second; }
    row_ptr[u + 1] = row_ptr[u] + (int) row.size();
  }
  return DC_OK;
}
int dc_get_vertex_data(const dc_ctx *c, double *mass, double *area, double *radii) {
  if (!c || !c->built) return DC_ERR_STATE;
  const int N = c->host.N;
  for (int i = 0; i < N; i++) {
    const int u = c->user_of.empty() ? i : c->user_of[i];
    if (mass) mass[u] = c->host.mass[i];
    if (area) area[u] = c->host.area[i];
    if (radii) radii[u] = c->host.radii[i];
  }
  return DC_OK;
}

int dc_alloc_batch(dc_ctx *c, int B, int tape) {
  if (!c) return DC_ERR_INVALID;
  if (c->host_only) return fail(c, DC_ERR_STATE, "host-only context (dc_create(-1)): no device, and there is no CPU compute path");
  if (!c->built) return fail(c, DC_ERR_STATE, "dc_alloc_batch: dc_build has not been called");
  if (B <= 0 || tape <= 0) return fail(c, DC_ERR_INVALID, "dc_alloc_batch: batch and tape_steps must be > 0");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  free_pool(c->batch_allocs);
  free_pool(c->band_allocs);
  c->dense = DenseAdjWork{}; c->dense_nb = 0;
  c->band = BandAdjWork{}; c->band_nb = 0;
  c->B = B; c->tape = tape; c->start_slot = 0;
  const int N = c->host.N, Af = (int) c->host.att_vertex.size(), NC = c->S.NC, G = c->S.ngroups;
  const size_t se = (size_t) B * 3 * N, slots = (size_t) tape + 1;
  auto &pool = c->batch_allocs;
  int rc;
  if ((rc = dev_alloc(c, pool, &c->X, se * slots))) return rc;
  if ((rc = dev_alloc(c, pool, &c->V, se * slots))) return rc;
  if ((rc = dev_alloc(c, pool, &c->F, se * slots))) return rc;
  if ((rc = dev_alloc(c, pool, &c->R, se * slots))) return rc;
  if ((rc = dev_alloc(c, pool, &c->NRM, se * slots))) return rc;
  if ((rc = dev_alloc(c, pool, &c->PRIM, (size_t) B * N * slots))) return rc;
  if ((rc = dev_alloc(c, pool, &c->W.g, se))) return rc;
  if ((rc = dev_alloc(c, pool, &c->W.vnow, se))) return rc;
  if ((rc = dev_alloc(c, pool, &c->W.vbest, se))) return rc;
  if ((rc = dev_alloc(c, pool, &c->W.cg_r, se))) return rc;
  if ((rc = dev_alloc(c, pool, &c->W.cg_p, se))) return rc;
  if ((rc = dev_alloc(c, pool, &c->W.cg_ap, se))) return rc;
  if ((rc = dev_alloc(c, pool, &c->W.cg_x, se))) return rc;
  if ((rc = dev_alloc(c, pool, &c->W.corner, (size_t) B * 3 * NC))) return rc;
  if ((rc = dev_alloc(c, pool, &c->W.ap4, (size_t) B * N))) return rc;
  if ((rc = dev_alloc(c, pool, &c->W.pre_p, se))) return rc;
  if ((rc = dev_alloc(c, pool, &c->W.pre_s, se))) return rc;
  if ((rc = dev_alloc(c, pool, &c->W.minv, (size_t) B * 9 * N))) return rc;
  if ((rc = dev_alloc(c, pool, &c->W.u64, se))) return rc;
  if ((rc = dev_alloc(c, pool, &c->W.r64, se))) return rc;
  if ((rc = dev_alloc(c, pool, &c->W.y64, se))) return rc;
  if ((rc = dev_alloc(c, pool, &c->W.x64, se))) return rc;
  if ((rc = dev_alloc(c, pool, &c->W.c64, (size_t) B * 3 * NC))) return rc;
  for (int k = 0; k < 6; k++) if ((rc = dev_alloc(c, pool, &c->W.k64[k], se))) return rc;
  {
    const int cap = c->S.self_cap;
    c->self_cap = cap;
    if ((rc = dev_alloc(c, pool, &c->SC_pair, (size_t) B * cap * slots))) return rc;
    if ((rc = dev_alloc(c, pool, &c->SC_nrm, (size_t) B * cap * slots))) return rc;
    if ((rc = dev_alloc(c, pool, &c->SC_d, (size_t) B * cap * slots))) return rc;
    if ((rc = dev_alloc(c, pool, &c->SC_meta, (size_t) B * kMetaStride * slots))) return rc;
    if ((rc = dev_alloc(c, pool, &c->SC_verts, (size_t) B * 2 * cap * slots))) return rc;
    if ((rc = dev_alloc(c, pool, &c->W.sd_cell, (size_t) B * N))) return rc;
    if ((rc = dev_alloc(c, pool, &c->W.sd_order, (size_t) B * N))) return rc;
    if ((rc = dev_alloc(c, pool, &c->W.sd_sx, se))) return rc;
    if ((rc = dev_alloc(c, pool, &c->W.sd_rawpair, (size_t) B * cap))) return rc;
    if ((rc = dev_alloc(c, pool, &c->W.sd_rawn, (size_t) B * cap))) return rc;
    if ((rc = dev_alloc(c, pool, &c->W.sd_tmp, (size_t) B * self_tmp_ints(cap)))) return rc;
  }
  if ((rc = dev_alloc(c, pool, &c->xf_cur, (size_t) B * 3 * Af))) return rc;
  if ((rc = dev_alloc(c, pool, &c->XF, (size_t) B * 3 * Af * slots))) return rc;
  if ((rc = dev_alloc(c, pool, &c->DPAR, (size_t) B * 8 * slots))) return rc;
  if ((rc = dev_alloc(c, pool, &c->mu, (size_t) B * G))) return rc;
  if ((rc = dev_alloc(c, pool, &c->fu, (size_t) B * 3))) return rc;
  if ((rc = dev_alloc(c, pool, &c->fv, (size_t) B * 3 * N))) return rc;
  if ((rc = dev_alloc(c, pool, &c->fv2, (size_t) B * 3 * N))) return rc;
  if ((rc = dev_alloc(c, pool, &c->GX, se))) return rc;
  if ((rc = dev_alloc(c, pool, &c->GV, se))) return rc;
  if ((rc = dev_alloc(c, pool, &c->IX, se))) return rc;
  if ((rc = dev_alloc(c, pool, &c->IV, se))) return rc;
  if ((rc = dev_alloc(c, pool, &c->DXF, (size_t) B * 3 * Af * slots))) return rc;
  if ((rc = dev_alloc(c, pool, &c->FU_S, (size_t) B * 3 * slots))) return rc;
  if ((rc = dev_alloc(c, pool, &c->FVS_S, (size_t) B * slots))) return rc;
  {   // primitive centres: every row and the current set start as the built centres; offsets and their schedule are gone (B or G changed)
    const int P = c->S.nprim;
    std::vector<double> built((size_t) 3 * P);
    for (int k = 0; k < P; k++) for (int d = 0; d < 3; d++) built[3 * (size_t) k + d] = c->prims[k].center[d];
    double *pb = nullptr;
    int *pg = nullptr;
    if ((rc = dev_alloc(c, pool, &pb, built.size()))) return rc;
    if ((rc = dev_alloc(c, pool, &pg, (size_t) P))) return rc;
    if (P > 0) {
      HIPCHK(c, hipMemcpy(pb, built.data(), built.size() * sizeof(double), hipMemcpyHostToDevice));
      HIPCHK(c, hipMemcpy(pg, c->group_of_prim.data(), (size_t) P * sizeof(int), hipMemcpyHostToDevice));
    }
    c->pc_built = pb; c->pc_group = pg;
    if ((rc = dev_alloc(c, pool, &c->PC, (size_t) B * P * 3 * slots))) return rc;
    if ((rc = dev_alloc(c, pool, &c->pc_cur, (size_t) B * P * 3))) return rc;
    launch_prim_centres(c->pc_built, c->pc_group, nullptr, 0, c->PC, (long) slots * B, P, c->ngroups, c->stream);
    launch_prim_centres(c->pc_built, c->pc_group, nullptr, 0, c->pc_cur, (long) B, P, c->ngroups, c->stream);
    HIPCHK(c, hipGetLastError());
    c->pc_row_gen.assign(slots + 1, 0); c->sched_pc.assign(slots + 1, 0);
    c->pc_gen = 0; c->pc_gen_last = 0;
  }
  c->PV = c->pv_cur = c->DPV = nullptr; c->pv_set = c->pw_set = false; c->sched_pv.assign(slots + 1, 0); c->sched_pw.assign(slots + 1, 0);      // obstacle velocities and spins: allocated by their first setter
  c->PS = c->ps_cur = nullptr; c->sched_ps.assign(slots + 1, 0);      // obstacle shapes: likewise
  c->ps_row_gen.assign(slots + 1, 0); c->ps_gen = 0; c->ps_gen_last = 0;
  {   // ... but the built rows of the batch go up now, while this call synchronises anyway: the first shape setter, which may be a _dev form
      // between enqueued sweeps, then fills table and current set with device-to-device copies on the stream
    std::vector<float> one;
    built_shape_rows(c, one);
    std::vector<float> all((size_t) B * one.size());
    for (int b = 0; b < B; b++) std::copy(one.begin(), one.end(), all.begin() + (size_t) b * one.size());
    float *pb = nullptr;
    if ((rc = dev_alloc(c, pool, &pb, all.size()))) return rc;
    if (!all.empty()) HIPCHK(c, hipMemcpy(pb, all.data(), all.size() * sizeof(float), hipMemcpyHostToDevice));
    c->ps_built = pb;
  }
  c->SEEDX = c->SEEDV = nullptr;
  c->RWJ = c->RWW = c->RSX = c->RSV = nullptr; c->rw_has = nullptr; c->sched_rw.assign(slots + 1, 0); c->rw_arrived = -1;      // read-out weights: allocated by their first setter
  c->INJ_X = c->INJ_F = c->INJ_N = c->INJ_SN = c->INJ_SD = nullptr; c->inj_slot = -1;
  c->YS = nullptr; c->keep_y = false;
  c->sro_scratch = nullptr; c->sro_sums = nullptr;
  c->sched_xf.assign(slots + 1, 0); c->sched_fu.assign(slots + 1, 0); c->sched_fvs.assign(slots + 1, 0); c->sched_seed.assign(slots + 1, 0);
  if ((rc = dev_alloc(c, pool, &c->DMU, (size_t) B * G))) return rc;
  if ((rc = dev_alloc(c, pool, &c->target, (size_t) 3 * N))) return rc;
  if ((rc = dev_alloc(c, pool, &c->fstats, (size_t) B * slots))) return rc;
  if ((rc = dev_alloc(c, pool, &c->bstats, (size_t) B * slots))) return rc;
  if ((rc = dev_alloc(c, pool, &c->adj_path, 2 * (size_t) B))) return rc;
  c->stage_elems = se;
  for (int k = 0; k < 4; k++) if ((rc = dev_alloc(c, pool, &c->stage[k], se))) return rc;
  c->fu_set = false; c->fv_set = false; c->fv2_set = false;
  // default fixed-point targets = rest positions of the attached vertices (FixedPoint::pos = pos_rest)
  if (Af > 0) {
    std::vector<float> xf((size_t) B * 3 * Af);
    for (int b = 0; b < B; b++)
      for (int a = 0; a < Af; a++)
        for (int d = 0; d < 3; d++) xf[((size_t) b * 3 + d) * Af + a] = (float) c->host.rest[3 * c->host.att_vertex[a] + d];
    HIPCHK(c, hipMemcpy(c->xf_cur, xf.data(), xf.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  if ((rc = choose_cluster(c))) return rc;
  return dc_set_mu(c, nullptr);
}

int dc_set_mu(dc_ctx *c, const double *mu) {
  if (!c || c->B <= 0) return fail(c, DC_ERR_STATE, "dc_set_mu: no batch");
  const int G = c->S.ngroups;
  std::vector<float> m((size_t) c->B * G, 0.f);
  for (int b = 0; b < c->B; b++)
    for (int g = 0; g < G; g++) {
      double v = 0;
      if (mu) v = mu[(size_t) b * G + g];
      else for (size_t k = 0; k < c->prims.size(); k++) if (c->group_of_prim[k] == g) { v = c->prims[k].mu; break; }
      m[(size_t) b * G + g] = (float) v;
    }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(c->mu, m.data(), m.size() * sizeof(float), hipMemcpyHostToDevice));
  return DC_OK;
}

int dc_set_uniform_force(dc_ctx *c, const double *f) {
  if (!c || c->B <= 0) return fail(c, DC_ERR_STATE, "dc_set_uniform_force: no batch");
  if (!f) { c->fu_set = false; return DC_OK; }
  std::vector<float> v((size_t) c->B * 3);
  for (size_t k = 0; k < v.size(); k++) v[k] = (float) f[k];
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(c->fu, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
  c->fu_set = true;
  return DC_OK;
}

int dc_set_vertex_force_field(dc_ctx *c, const double *f) {
  if (!c || c->B <= 0) return fail(c, DC_ERR_STATE, "dc_set_vertex_force_field: no batch");
  if (!f) { c->fv2_set = false; return DC_OK; }
  HIPCHK(c, hipSetDevice(c->device));
  int rc = h2d_planar(c, f, c->fv2, c->host.N, true);
  if (rc) return rc;
  if ((rc = stage_sync(c))) return rc;
  c->fv2_set = true;
  return DC_OK;
}

int dc_set_vertex_forces(dc_ctx *c, const double *f) {
  if (!c || c->B <= 0) return fail(c, DC_ERR_STATE, "dc_set_vertex_forces: no batch");
  if (!f) { c->fv_set = false; return DC_OK; }
  HIPCHK(c, hipSetDevice(c->device));
  int rc = h2d_planar(c, f, c->fv, c->host.N, true);
  if (rc) return rc;
  if ((rc = stage_sync(c))) return rc;
  c->fv_set = true;
  return DC_OK;
}

int dc_get_force_gradient(dc_ctx *c, double *dL_df) {
  int rc = check_batch(c, 0, 0);
  if (rc) return rc;
  if (!dL_df) return fail(c, DC_ERR_INVALID, "dc_get_force_gradient: null output");
  // the adjoint kernel leaves y = (I + dr_df)^T u* of its last step in the work vector it shares with the forward kernel
  if ((rc = d2h_planar(c, c->W.vbest, dL_df, c->host.N, true))) return rc;
  if ((rc = stage_sync(c))) return rc;
  const double h2 = c->params.time_step * c->params.time_step;
  const size_t n = (size_t) c->B * 3 * c->host.N;
  for (size_t k = 0; k < n; k++) dL_df[k] *= h2;
  return DC_OK;
}

int dc_keep_force_gradients(dc_ctx *c, int keep) {
  int rc = check_batch(c, 0, 0);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  if (keep && !c->YS && (rc = dev_alloc(c, c->batch_allocs, &c->YS, slot_elems(c) * ((size_t) c->tape + 1)))) return rc;
  c->keep_y = keep != 0;
  return DC_OK;
}

int dc_get_force_gradients(dc_ctx *c, int slot0, int nslots, double *dL_df) {
  int rc = check_batch(c, slot0, slot0 + nslots - 1);
  if (rc) return rc;
  if (slot0 < 1 || nslots < 1 || !dL_df) return fail(c, DC_ERR_INVALID, "dc_get_force_gradients: slot 0 has no record");
  if (!c->YS) return fail(c, DC_ERR_STATE, "dc_get_force_gradients: dc_keep_force_gradients(1) was not set before the backward sweep");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t se = slot_elems(c);
  const double h2 = c->params.time_step * c->params.time_step;
  for (int k = 0; k < nslots; k++)
    if ((rc = d2h_planar(c, c->YS + se * (slot0 + k), dL_df + se * k, c->host.N, true))) return rc;
  if ((rc = stage_sync(c))) return rc;
  for (size_t q = 0; q < se * (size_t) nslots; q++) dL_df[q] *= h2;
  return cluster_check(c);
}

int dc_set_state(dc_ctx *c, int slot, const double *x, const double *v) {
  int rc = check_batch(c, slot, slot);
  if (rc) return rc;
  if (!x || !v) return fail(c, DC_ERR_INVALID, "dc_set_state: null state");
  HIPCHK(c, hipSetDevice(c->device));
  if (slot == c->inj_slot || slot + 1 == c->inj_slot) c->inj_slot = -1;      // a record handed in with dc_set_record described the state overwritten here
  const size_t se = slot_elems(c);
  if ((rc = h2d_planar(c, x, c->X + se * slot, c->host.N, true))) return rc;
  if ((rc = h2d_planar(c, v, c->V + se * slot, c->host.N, true))) return rc;
  return stage_sync(c);   // host buffers may be reused by the caller
}

int dc_get_state(dc_ctx *c, int slot, double *x, double *v) {
  int rc = check_batch(c, slot, slot);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t se = slot_elems(c);
  if (x && (rc = d2h_planar(c, c->X + se * slot, x, c->host.N, true))) return rc;
  if (v && (rc = d2h_planar(c, c->V + se * slot, v, c->host.N, true))) return rc;
  if ((rc = stage_sync(c))) return rc;
  return cluster_check(c);          // a state written by split kernels whose exchange timed out is not a state
}

int dc_step_forward(dc_ctx *c, int slot, const double *fixed_pts, dc_step_stats *stats) {
  int rc = check_batch(c, slot, slot + 1);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  const int Af = c->S.Af;
  if (fixed_pts && Af > 0) {
    if ((rc = h2d_planar(c, fixed_pts, c->xf_cur, Af, false))) return rc;
    c->sched_xf[slot + 1] = 0;               // explicit targets win over a schedule entry of this step
  }
  if ((rc = enqueue_forward_steps(c, slot, 1, false, nullptr))) return rc;
  if (stats) {
    HIPCHK(c, hipMemcpyAsync(stats, c->fstats + (size_t) c->B * (slot + 1), sizeof(dc_step_stats) * c->B, hipMemcpyDeviceToHost, c->stream));
    if ((rc = stage_sync(c))) return rc;
    if ((rc = cluster_check(c))) return rc;
    if ((rc = check_self_overflow(c, stats, slot + 1))) return rc;
  } else if (fixed_pts && Af > 0) {
    if ((rc = stage_sync(c))) return rc;
  }
  return DC_OK;
}

int dc_get_record(dc_ctx *c, int slot, double *f, double *r) {
  int rc = check_batch(c, slot, slot);
  if (rc) return rc;
  if (slot < 1) return fail(c, DC_ERR_INVALID, "dc_get_record: slot 0 has no record");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t se = slot_elems(c);
  if (f && (rc = d2h_planar(c, c->F + se * slot, f, c->host.N, true))) return rc;
  if (r && (rc = d2h_planar(c, c->R + se * slot, r, c->host.N, true))) return rc;
  if ((rc = stage_sync(c))) return rc;
  return cluster_check(c);
}

int dc_get_contacts(dc_ctx *c, int slot, int *prim_group, double *normal) {
  int rc = check_batch(c, slot, slot);
  if (rc) return rc;
  if (slot < 1) return fail(c, DC_ERR_INVALID, "dc_get_contacts: slot 0 has no record");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t se = slot_elems(c), sp = (size_t) c->B * c->host.N;
  if (normal && (rc = d2h_planar(c, c->NRM + se * slot, normal, c->host.N, true))) return rc;
  if ((rc = stage_sync(c))) return rc;
  if (prim_group) {
    std::vector<int> dev(sp);
    HIPCHK(c, hipMemcpy(dev.data(), c->PRIM + sp * slot, sp * sizeof(int), hipMemcpyDeviceToHost));
    const int N = c->host.N;
    for (int b = 0; b < c->B; b++)
      for (int i = 0; i < N; i++) {
        const int g = dev[(size_t) b * N + i];
        prim_group[(size_t) b * N + (c->user_of.empty() ? i : c->user_of[i])] = g >= 0 ? c->prims[g].group : g;
      }
  }
  return DC_OK;
}

int dc_get_self_contacts(dc_ctx *c, int slot, int rollout, int cap, int *count, int *num_layers, int *pairs, int *layer, double *normal) {
  int rc = check_batch(c, slot, slot);
  if (rc) return rc;
  if (slot < 1 || rollout < 0 || rollout >= c->B) return fail(c, DC_ERR_INVALID, "dc_get_self_contacts: bad slot / rollout");
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const SelfRec R = self_slot(c, slot);
  std::vector<int> meta_v(kMetaStride); int *meta = meta_v.data();
  HIPCHK(c, hipMemcpy(meta, R.meta + (size_t) rollout * kMetaStride, sizeof(int) * kMetaStride, hipMemcpyDeviceToHost));
  const int C = meta[0], nl = meta[1];
  if (count) *count = C;
  if (num_layers) *num_layers = nl;
  const int n = std::min(C, cap);
  if (n <= 0) return DC_OK;
  const size_t base = (size_t) rollout * c->self_cap;
  std::vector<int2> pr(n);
  std::vector<float4> nr(n);
  HIPCHK(c, hipMemcpy(pr.data(), R.pair + base, sizeof(int2) * n, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(nr.data(), R.nrm + base, sizeof(float4) * n, hipMemcpyDeviceToHost));
  for (int k = 0; k < n; k++) {
    if (pairs) {
      pairs[2 * k] = c->user_of.empty() ? pr[k].x : c->user_of[pr[k].x];
      pairs[2 * k + 1] = c->user_of.empty() ? pr[k].y : c->user_of[pr[k].y];
    }
    if (normal) { normal[3 * k] = nr[k].x; normal[3 * k + 1] = nr[k].y; normal[3 * k + 2] = nr[k].z; }
    if (layer) { int l = 0; while (l + 1 < nl && k >= meta[2 + l + 1]) l++; layer[k] = l; }
  }
  return DC_OK;
}

int dc_set_record(dc_ctx *c, int slot, const dc_record *rec) {
  int rc = check_batch(c, slot, slot);
  if (rc) return rc;
  if (slot < 1) return fail(c, DC_ERR_INVALID, "dc_set_record: slot 0 has no record");
  if (!rec || !rec->x || !rec->v || !rec->f || !rec->prim || !rec->normal) return fail(c, DC_ERR_INVALID, "dc_set_record: x, v, f, prim and normal are required");
  if (rec->self_count && (!rec->self_pairs || !rec->self_layer || !rec->self_normal || !rec->self_d)) return fail(c, DC_ERR_INVALID, "dc_set_record: incomplete self-contact lists");
  HIPCHK(c, hipSetDevice(c->device));
  const int N = c->host.N, B = c->B, Af = c->S.Af, cap = c->self_cap;
  const size_t se = slot_elems(c), sp = (size_t) B * N;
  if (!c->INJ_X) {
    if ((rc = dev_alloc(c, c->batch_allocs, &c->INJ_X, se))) return rc;
    if ((rc = dev_alloc(c, c->batch_allocs, &c->INJ_F, se))) return rc;
    if ((rc = dev_alloc(c, c->batch_allocs, &c->INJ_N, se))) return rc;
    if ((rc = dev_alloc(c, c->batch_allocs, &c->INJ_SN, (size_t) B * cap * 3))) return rc;
    if ((rc = dev_alloc(c, c->batch_allocs, &c->INJ_SD, (size_t) B * cap * 3))) return rc;
  }
  c->inj_slot = -1;
  HostRecord H;      // primitive indices and self contacts in the record layout of the kernels (dc_record.h)
  if (!H.build(*rec, B, N, cap, (int) c->prims.size(), c->user_of, c->dev_of)) return fail(c, H.code, H.error);
  // per-vertex part: fp32 tape entries + fp64 planes (device numbering)
  struct { const double *src; float *dst32; double *dst64; } planes[5] = {
      {rec->x, c->X + se * slot, c->INJ_X}, {rec->v, c->V + se * slot, nullptr}, {rec->f, c->F + se * slot, c->INJ_F},
      {rec->r, c->R + se * slot, nullptr}, {rec->normal, c->NRM + se * slot, c->INJ_N}};
  for (auto &pl : planes) {
    if (!pl.src) continue;
    double *stage;
    if ((rc = stage_take(c, &stage))) return rc;
    HIPCHK(c, hipMemcpyAsync(stage, pl.src, se * sizeof(double), hipMemcpyHostToDevice, c->stream));
    launch_f64i_to_f32p(stage, pl.dst32, B, N, c->d_user_of, c->stream);
    if (pl.dst64) launch_f64i_to_f64p(stage, pl.dst64, B, N, c->d_user_of, c->stream);
  }
  if ((rc = stage_sync(c))) return rc;
  HIPCHK(c, hipMemcpy(c->PRIM + sp * slot, H.prim.data(), sp * sizeof(int), hipMemcpyHostToDevice));
  if (rec->x_fixed && Af > 0) {
    if ((rc = h2d_planar(c, rec->x_fixed, xf_slot(c, slot), Af, false))) return rc;
    if ((rc = stage_sync(c))) return rc;
  }
  const SelfRec R = self_slot(c, slot);
  HIPCHK(c, hipMemcpy(R.meta, H.meta.data(), H.meta.size() * sizeof(int), hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(R.pair, H.pair.data(), H.pair.size() * sizeof(int2), hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(R.nrm, H.nrm.data(), H.nrm.size() * sizeof(float4), hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(R.dvec, H.dvec.data(), H.dvec.size() * sizeof(float4), hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(R.verts, H.verts.data(), H.verts.size() * sizeof(int), hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(c->INJ_SN, H.sn.data(), H.sn.size() * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(c->INJ_SD, H.sd.data(), H.sd.size() * sizeof(double), hipMemcpyHostToDevice));
  c->inj_slot = slot;
  return DC_OK;
}

int dc_step_backward(dc_ctx *c, int slot, const double *dL_dxnew, const double *dL_dvnew, const double *dL_dxinit,
                     const double *dL_dvinit, int is_start, double *dL_dx, double *dL_dv, double *dL_dxfixed,
                     double *dL_dmu, dc_bwd_stats *stats) {
  int rc = check_batch(c, slot, slot);
  if (rc) return rc;
  if (slot < 1) return fail(c, DC_ERR_INVALID, "dc_step_backward: slot 0 has no record");
  if (!dL_dxnew || !dL_dvnew || !dL_dx || !dL_dv) return fail(c, DC_ERR_INVALID, "dc_step_backward: null gradient");
  HIPCHK(c, hipSetDevice(c->device));
  const int N = c->host.N, Af = c->S.Af, G = c->S.ngroups;
  if ((rc = h2d_planar(c, dL_dxnew, c->GX, N, true))) return rc;
  if ((rc = h2d_planar(c, dL_dvnew, c->GV, N, true))) return rc;
  const bool with_init = dL_dxinit && dL_dvinit, start = is_start != 0;
  if (with_init) {
    if ((rc = h2d_planar(c, dL_dxinit, c->IX, N, true))) return rc;
    if ((rc = h2d_planar(c, dL_dvinit, c->IV, N, true))) return rc;
  }
  HIPCHK(c, hipMemsetAsync(c->DMU, 0, sizeof(float) * c->B * G, c->stream));
  if ((rc = enqueue_backward_steps(c, slot, 1, with_init ? Seeds::init : Seeds::none, &start, nullptr))) return rc;
  if ((rc = d2h_planar(c, c->GX, dL_dx, N, true))) return rc;
  if ((rc = d2h_planar(c, c->GV, dL_dv, N, true))) return rc;
  if (dL_dxfixed && Af > 0 && (rc = d2h_planar(c, dxf_slot(c, slot), dL_dxfixed, Af, false))) return rc;
  std::vector<float> dmu((size_t) c->B * G);
  HIPCHK(c, hipMemcpyAsync(dmu.data(), c->DMU, dmu.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  if (stats) HIPCHK(c, hipMemcpyAsync(stats, c->bstats + (size_t) c->B * slot, sizeof(dc_bwd_stats) * c->B, hipMemcpyDeviceToHost, c->stream));
  if ((rc = stage_sync(c))) return rc;
  if ((rc = cluster_check(c))) return rc;
  if (dL_dmu) for (size_t k = 0; k < dmu.size(); k++) dL_dmu[k] = dmu[k];
  return DC_OK;
}

// ---- device-pointer boundary: the per-step calls for callers whose tensors live on this GPU
//      (the RL / controller-training loop: functional.py:20-102, hatController.py:78-105 run one stepNN + stepBackwardNN per step).
//      Buffers are DEVICE pointers in the caller's layout — xyz interleaved, B rollouts concatenated, fp32 (is_f32 = 1, torch's default)
//      or fp64 — converted on the device; nothing crosses PCIe and nothing synchronises: every call is enqueued on the context's stream.
int dc_use_stream(dc_ctx *c, void *hip_stream) {
  if (!c || c->host_only) return fail(c, DC_ERR_STATE, "dc_use_stream: no device context");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->stream = hip_stream ? (hipStream_t) hip_stream : c->own_stream;
  return DC_OK;
}

int dc_set_state_dev(dc_ctx *c, int slot, const void *d_x, const void *d_v, int is_f32) {
  int rc = check_batch(c, slot, slot);
  if (rc) return rc;
  if (!d_x || !d_v) return fail(c, DC_ERR_INVALID, "dc_set_state_dev: null state");
  HIPCHK(c, hipSetDevice(c->device));
  if (slot == c->inj_slot || slot + 1 == c->inj_slot) c->inj_slot = -1;      // (see dc_set_state)
  const size_t se = slot_elems(c);
  launch_dev_to_planar(d_x, is_f32, c->X + se * slot, c->B, c->host.N, c->d_user_of, c->stream);
  launch_dev_to_planar(d_v, is_f32, c->V + se * slot, c->B, c->host.N, c->d_user_of, c->stream);
  HIPCHK(c, hipGetLastError());
  return DC_OK;
}

int dc_get_state_dev(dc_ctx *c, int slot, void *d_x, void *d_v, int is_f32) {
  int rc = check_batch(c, slot, slot);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t se = slot_elems(c);
  if (d_x) launch_planar_to_dev(c->X + se * slot, d_x, is_f32, c->B, c->host.N, c->d_user_of, c->stream);
  if (d_v) launch_planar_to_dev(c->V + se * slot, d_v, is_f32, c->B, c->host.N, c->d_user_of, c->stream);
  HIPCHK(c, hipGetLastError());
  return DC_OK;
}

int dc_step_forward_dev(dc_ctx *c, int slot, const void *d_fixed_pts, int is_f32) {
  int rc = check_batch(c, slot, slot + 1);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  const int Af = c->S.Af;
  if (d_fixed_pts && Af > 0) {
    launch_dev_to_planar(d_fixed_pts, is_f32, c->xf_cur, c->B, Af, nullptr, c->stream);
    c->sched_xf[slot + 1] = 0;
  }
  return enqueue_forward_steps(c, slot, 1, false, nullptr);
}

int dc_step_backward_dev(dc_ctx *c, int slot, const void *d_dL_dxnew, const void *d_dL_dvnew, const void *d_dL_dxinit, const void *d_dL_dvinit,
                         int is_start, void *d_dL_dx, void *d_dL_dv, void *d_dL_dxfixed, void *d_dL_dmu, int is_f32) {
  int rc = check_batch(c, slot, slot);
  if (rc) return rc;
  if (slot < 1) return fail(c, DC_ERR_INVALID, "dc_step_backward_dev: slot 0 has no record");
  if (!d_dL_dxnew || !d_dL_dvnew || !d_dL_dx || !d_dL_dv) return fail(c, DC_ERR_INVALID, "dc_step_backward_dev: null gradient");
  HIPCHK(c, hipSetDevice(c->device));
  const int N = c->host.N, Af = c->S.Af, G = c->S.ngroups;
  launch_dev_to_planar(d_dL_dxnew, is_f32, c->GX, c->B, N, c->d_user_of, c->stream);
  launch_dev_to_planar(d_dL_dvnew, is_f32, c->GV, c->B, N, c->d_user_of, c->stream);
  const bool with_init = d_dL_dxinit && d_dL_dvinit, start = is_start != 0;
  if (with_init) {
    launch_dev_to_planar(d_dL_dxinit, is_f32, c->IX, c->B, N, c->d_user_of, c->stream);
    launch_dev_to_planar(d_dL_dvinit, is_f32, c->IV, c->B, N, c->d_user_of, c->stream);
  }
  HIPCHK(c, hipMemsetAsync(c->DMU, 0, sizeof(float) * c->B * G, c->stream));
  if ((rc = enqueue_backward_steps(c, slot, 1, with_init ? Seeds::init : Seeds::none, &start, nullptr))) return rc;
  launch_planar_to_dev(c->GX, d_dL_dx, is_f32, c->B, N, c->d_user_of, c->stream);
  launch_planar_to_dev(c->GV, d_dL_dv, is_f32, c->B, N, c->d_user_of, c->stream);
  if (d_dL_dxfixed && Af > 0) launch_planar_to_dev(dxf_slot(c, slot), d_dL_dxfixed, is_f32, c->B, Af, nullptr, c->stream);
  if (d_dL_dmu) launch_copy_cast(c->DMU, d_dL_dmu, is_f32, (long) c->B * G, c->stream);
  HIPCHK(c, hipGetLastError());
  return DC_OK;
}

int dc_rollout_forward(dc_ctx *c, int slot, int nsteps) {
  int rc = check_batch(c, slot, slot + nsteps);
  if (rc) return rc;
  if ((rc = kernel_time_begin(c))) return rc;
  int launches = 0;
  if ((rc = enqueue_forward_steps(c, slot, nsteps, true, &launches))) return rc;
  return kernel_time_end(c, false, launches);
}

int dc_seed_gradient(dc_ctx *c, int slot, const double *target, double scale_x) {
  int rc = check_batch(c, slot, slot);
  if (rc) return rc;
  c->rw_arrived = -1;
  HIPCHK(c, hipSetDevice(c->device));
  const int N = c->host.N;
  std::vector<float> t(3 * (size_t) N);
  for (int i = 0; i < N; i++)
    for (int d = 0; d < 3; d++)
      t[(size_t) d * N + i] = (float) (target ? target[3 * (size_t) (c->user_of.empty() ? i : c->user_of[i]) + d] : c->host.rest[3 * i + d]);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(c->target, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice));
  launch_seed_gradient(c->X + slot_elems(c) * slot, c->target, c->GX, c->GV, c->B, N, (float) scale_x, c->stream);
  HIPCHK(c, hipMemsetAsync(c->DMU, 0, sizeof(float) * c->B * c->S.ngroups, c->stream));
  return DC_OK;
}

int dc_rollout_backward(dc_ctx *c, int slot, int nsteps) {
  int rc = check_batch(c, slot - nsteps + 1, slot);
  if (rc) return rc;
  if (slot - nsteps + 1 < 1) return fail(c, DC_ERR_INVALID, "dc_rollout_backward: would run past slot 1");
  if ((rc = kernel_time_begin(c))) return rc;
  int launches = 0;
  if ((rc = enqueue_backward_steps(c, slot, nsteps, Seeds::schedule, nullptr, &launches))) return rc;
  return kernel_time_end(c, true, launches);
}

int dc_set_trajectory_start(dc_ctx *c, int start_slot) {
  if (!c) return DC_ERR_INVALID;
  if (start_slot < -1) return fail(c, DC_ERR_INVALID, "dc_set_trajectory_start: start_slot must be >= -1");
  c->start_slot = start_slot;
  return DC_OK;
}

int dc_get_gradient(dc_ctx *c, double *dL_dx, double *dL_dv, double *dL_dmu) {
  int rc = check_batch(c, 0, 0);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  const int N = c->host.N, G = c->S.ngroups;
  if (dL_dx && (rc = d2h_planar(c, c->GX, dL_dx, N, true))) return rc;
  if (dL_dv && (rc = d2h_planar(c, c->GV, dL_dv, N, true))) return rc;
  if ((rc = stage_sync(c))) return rc;
  if (dL_dmu) {
    std::vector<float> dmu((size_t) c->B * G);
    HIPCHK(c, hipMemcpy(dmu.data(), c->DMU, dmu.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < dmu.size(); k++) dL_dmu[k] = dmu[k];
  }
  return DC_OK;
}

// ---- device-resident schedules of the fused rollouts (stepFixPoints / fillForces / the per-frame loss seeds
// of runBackwardTask, Simulation.cpp:55-116, 964-1018, 3938-3952, as streams on the device) ----
int dc_set_fixed_point_schedule(dc_ctx *c, int slot0, int nsteps, const double *xf) {
  int rc = check_batch(c, slot0, slot0 + nsteps);
  if (rc) return rc;
  if (nsteps < 1 || !xf) return fail(c, DC_ERR_INVALID, "dc_set_fixed_point_schedule: null schedule");
  const int Af = c->S.Af;
  if (Af <= 0) return DC_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t per = xf_elems(c);
  for (int k = 0; k < nsteps; k++) {
    if ((rc = h2d_planar(c, xf + per * k, xf_slot(c, slot0 + k + 1), Af, false))) return rc;
    c->sched_xf[slot0 + k + 1] = 1;
  }
  return stage_sync(c);
}

int dc_set_force_schedule(dc_ctx *c, int slot0, int nsteps, const double *fu, const double *fv_scale) {
  int rc = check_batch(c, slot0, slot0 + nsteps);
  if (rc) return rc;
  if (nsteps < 1) return fail(c, DC_ERR_INVALID, "dc_set_force_schedule: nsteps < 1");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (fu) {
    std::vector<float> v((size_t) nsteps * c->B * 3);
    for (size_t k = 0; k < v.size(); k++) v[k] = (float) fu[k];
    HIPCHK(c, hipMemcpy(c->FU_S + (size_t) c->B * 3 * (slot0 + 1), v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  if (fv_scale) {
    std::vector<float> v((size_t) nsteps * c->B);
    for (size_t k = 0; k < v.size(); k++) v[k] = (float) fv_scale[k];
    HIPCHK(c, hipMemcpy(c->FVS_S + (size_t) c->B * (slot0 + 1), v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  for (int k = 1; k <= nsteps; k++) { c->sched_fu[slot0 + k] = fu ? 1 : 0; c->sched_fvs[slot0 + k] = fv_scale ? 1 : 0; }
  return DC_OK;
}

int dc_set_seed_schedule(dc_ctx *c, int slot0, int nslots, const double *dL_dx, const double *dL_dv) {
  int rc = check_batch(c, slot0, slot0 + nslots - 1);
  if (rc) return rc;
  if (nslots < 1 || !dL_dx) return fail(c, DC_ERR_INVALID, "dc_set_seed_schedule: null schedule");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t se = slot_elems(c), slots = (size_t) c->tape + 1;
  if (!c->SEEDX) {
    if ((rc = dev_alloc(c, c->batch_allocs, &c->SEEDX, se * slots))) return rc;
    if ((rc = dev_alloc(c, c->batch_allocs, &c->SEEDV, se * slots))) return rc;
  }
  const int N = c->host.N;
  for (int k = 0; k < nslots; k++) {
    if ((rc = h2d_planar(c, dL_dx + se * k, seedx_slot(c, slot0 + k), N, true))) return rc;
    if (dL_dv) { if ((rc = h2d_planar(c, dL_dv + se * k, seedv_slot(c, slot0 + k), N, true))) return rc; }
    else HIPCHK(c, hipMemsetAsync(seedv_slot(c, slot0 + k), 0, se * sizeof(float), c->stream));
    c->sched_seed[slot0 + k] = 1;
  }
  return stage_sync(c);
}

int dc_clear_schedules(dc_ctx *c) {
  if (!c || c->B <= 0) return fail(c, DC_ERR_STATE, "dc_clear_schedules: no batch");
  std::fill(c->sched_xf.begin(), c->sched_xf.end(), 0); std::fill(c->sched_fu.begin(), c->sched_fu.end(), 0);
  std::fill(c->sched_fvs.begin(), c->sched_fvs.end(), 0); std::fill(c->sched_seed.begin(), c->sched_seed.end(), 0);
  std::fill(c->sched_pc.begin(), c->sched_pc.end(), 0);      // (the rows keep their entries until a step overwrites them: pc_row_gen = -1)
  std::fill(c->sched_pv.begin(), c->sched_pv.end(), 0); std::fill(c->sched_pw.begin(), c->sched_pw.end(), 0);
  std::fill(c->sched_ps.begin(), c->sched_ps.end(), 0);      // (like the centres: the rows keep their entries until a step overwrites them, ps_row_gen = -1)
  return clear_readout_gradients(c);
}

// ---- movable obstacles: per-rollout, per-step offsets of the primitive groups' centres (dc_primoffset.h holds the rule). The reference reads
//      Primitive::center at every step (Simulation.cpp:153-191) and exposes it read-write (python_interface.cpp:285) ----
namespace {
// the checks the four setters share: a batch on a device context (DC_ERR_STATE otherwise), primitives to move (DC_ERR_INVALID)
int check_offsets(dc_ctx *c, const char *who, int slot_lo, int slot_hi) {
  int rc = check_batch(c, slot_lo, slot_hi);
  if (rc) return rc;
  if (c->ngroups <= 0 || c->S.nprim <= 0) return fail(c, DC_ERR_INVALID, std::string(who) + ": the context has no primitives");
  return DC_OK;
}
// rows x [G][3] offsets on the host -> rows x [P][3] centres
void host_centres(const dc_ctx *c, const double *d, long rows, std::vector<float> &out) {
  const int P = c->S.nprim, G = c->ngroups;
  std::vector<double> built((size_t) 3 * P);
  for (int k = 0; k < P; k++) for (int q = 0; q < 3; q++) built[3 * (size_t) k + q] = c->prims[k].center[q];
  out.resize((size_t) rows * P * 3);
  for (long r = 0; r < rows; r++) expand_centres(P, built.data(), c->group_of_prim.data(), d ? d + (size_t) r * G * 3 : nullptr, out.data() + (size_t) r * P * 3);
}
}  // namespace

int dc_set_primitive_offsets(dc_ctx *c, const double *d) {
  int rc = check_offsets(c, "dc_set_primitive_offsets", 0, 0);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  std::vector<float> cen;
  host_centres(c, d, c->B, cen);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(c->pc_cur, cen.data(), cen.size() * sizeof(float), hipMemcpyHostToDevice));
  c->pc_gen = d ? ++c->pc_gen_last : 0;
  return DC_OK;
}

int dc_set_primitive_offsets_dev(dc_ctx *c, const void *d_d, int is_f32) {
  int rc = check_offsets(c, "dc_set_primitive_offsets_dev", 0, 0);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  launch_prim_centres(c->pc_built, c->pc_group, d_d, is_f32, c->pc_cur, c->B, c->S.nprim, c->ngroups, c->stream);
  HIPCHK(c, hipGetLastError());
  c->pc_gen = d_d ? ++c->pc_gen_last : 0;
  return DC_OK;
}

int dc_set_primitive_offset_schedule(dc_ctx *c, int slot0, int nsteps, const double *d) {
  int rc = check_offsets(c, "dc_set_primitive_offset_schedule", slot0, slot0 + nsteps);
  if (rc) return rc;
  if (nsteps < 1 || !d) return fail(c, DC_ERR_INVALID, "dc_set_primitive_offset_schedule: null schedule");
  HIPCHK(c, hipSetDevice(c->device));
  std::vector<float> cen;
  host_centres(c, d, (long) nsteps * c->B, cen);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(pc_slot(c, slot0 + 1), cen.data(), cen.size() * sizeof(float), hipMemcpyHostToDevice));
  for (int k = 1; k <= nsteps; k++) { c->sched_pc[slot0 + k] = 1; c->pc_row_gen[slot0 + k] = -1; }
  return DC_OK;
}

int dc_set_primitive_offset_schedule_dev(dc_ctx *c, int slot0, int nsteps, const void *d_d, int is_f32) {
  int rc = check_offsets(c, "dc_set_primitive_offset_schedule_dev", slot0, slot0 + nsteps);
  if (rc) return rc;
  if (nsteps < 1 || !d_d) return fail(c, DC_ERR_INVALID, "dc_set_primitive_offset_schedule_dev: null schedule");
  HIPCHK(c, hipSetDevice(c->device));
  launch_prim_centres(c->pc_built, c->pc_group, d_d, is_f32, pc_slot(c, slot0 + 1), (long) nsteps * c->B, c->S.nprim, c->ngroups, c->stream);
  HIPCHK(c, hipGetLastError());
  for (int k = 1; k <= nsteps; k++) { c->sched_pc[slot0 + k] = 1; c->pc_row_gen[slot0 + k] = -1; }
  return DC_OK;
}

int dc_get_primitive_centers(dc_ctx *c, int slot, double *out) {
  int rc = check_batch(c, slot, slot);
  if (rc) return rc;
  if (slot < 1 || !out) return fail(c, DC_ERR_INVALID, "dc_get_primitive_centers: slot 0 has no record");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::vector<float> v(pc_elems(c));
  if (!v.empty()) HIPCHK(c, hipMemcpy(v.data(), pc_slot(c, slot), v.size() * sizeof(float), hipMemcpyDeviceToHost));
  for (size_t k = 0; k < v.size(); k++) out[k] = v[k];
  return DC_OK;
}

// ---- moving obstacles: a velocity w[b][g] per rollout and primitive group, per step (include/diffcloth_hip.h holds the rule). The reference
//      carries the quantity (v_out = this->velocity in every isInContact of Primitive.cpp) and never sets it ----
namespace {
// The motion table (rows {w[3], omega[3]} per group), its current set and the gradient table come with the first velocity or spin setter after
// dc_alloc_batch, all zero: a context that never calls one hands null pointers to its kernels. Every entry below addresses its half of the
// rows (half 0 = w, 1 = omega); the caller's layout is the dense [..][B][G][3] of either kind.
int ensure_velocities(dc_ctx *c) {
  if (c->PV) return DC_OK;
  const size_t per = pv_elems(c), slots = (size_t) c->tape + 1;
  float *pv = nullptr, *cur = nullptr, *dpv = nullptr;
  int rc;
  if ((rc = dev_alloc(c, c->batch_allocs, &pv, per * slots))) return rc;
  if ((rc = dev_alloc(c, c->batch_allocs, &cur, per))) return rc;
  if ((rc = dev_alloc(c, c->batch_allocs, &dpv, per * slots))) return rc;
  HIPCHK(c, hipMemsetAsync(pv, 0, sizeof(float) * per * slots, c->stream));
  HIPCHK(c, hipMemsetAsync(cur, 0, sizeof(float) * per, c->stream));
  HIPCHK(c, hipMemsetAsync(dpv, 0, sizeof(float) * per * slots, c->stream));
  c->PV = pv; c->pv_cur = cur; c->DPV = dpv;      // (steps enqueued from here on see the table; those already enqueued ran the static law)
  return DC_OK;
}
// host values [rows][3] -> fp32 in one half of `rows` motion rows at `dst`; null = zeros. Synchronises, like the host forms of the offsets.
int upload_motion(dc_ctx *c, const double *w, float *dst, size_t rows, int half) {
  std::vector<float> v(rows * 3, 0.0f);
  if (w) for (size_t k = 0; k < v.size(); k++) v[k] = (float) w[k];
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy2D(dst + 3 * half, sizeof(float) * kPvRow, v.data(), sizeof(float) * 3, sizeof(float) * 3, rows, hipMemcpyHostToDevice));
  return DC_OK;
}
// one half of `rows` motion rows at `src` -> host [rows][3], widened. Synchronises.
int download_motion(dc_ctx *c, const float *src, double *out, size_t rows, int half) {
  std::vector<float> v(rows * 3);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy2D(v.data(), sizeof(float) * 3, src + 3 * half, sizeof(float) * kPvRow, sizeof(float) * 3, rows, hipMemcpyDeviceToHost));
  for (size_t k = 0; k < v.size(); k++) out[k] = v[k];
  return DC_OK;
}
// What a host spin setter refuses: a value that is not finite, and a non-zero omega for a group that holds no DC_PRIM_SPHERE (the term would be
// silently zero there). omega: [rows][G][3].
int check_spins(dc_ctx *c, const char *who, const double *omega, size_t rows) {
  if (!omega) return DC_OK;
  const int G = c->ngroups;
  std::vector<char> has_sphere(G, 0);
  for (size_t k = 0; k < c->prims.size(); k++) if (c->prims[k].kind == DC_PRIM_SPHERE) has_sphere[c->group_of_prim[k]] = 1;
  for (size_t r = 0; r < rows; r++)
    for (int g = 0; g < G; g++)
      for (int q = 0; q < 3; q++) {
        const double v = omega[(r * G + g) * 3 + q];
        if (!std::isfinite(v)) return fail(c, DC_ERR_INVALID, std::string(who) + ": an angular velocity is not finite");
        if (v != 0.0 && !has_sphere[g])
          return fail(c, DC_ERR_INVALID, std::string(who) + ": primitive group " + std::to_string(g) + " holds no DC_PRIM_SPHERE; only a sphere has a spin term");
      }
  return DC_OK;
}
void mark_motion_set(dc_ctx *c, int half) { (half ? c->pw_set : c->pv_set) = true; }
bool motion_was_set(const dc_ctx *c, int half) { return half ? c->pw_set : c->pv_set; }
void mark_motion_scheduled(dc_ctx *c, int half, int slot0, int nsteps) {
  std::vector<char> &s = half ? c->sched_pw : c->sched_pv;
  for (int k = 1; k <= nsteps; k++) s[slot0 + k] = 1;
}

// the bodies of the velocity (half 0) and spin (half 1) entries
int set_motion(dc_ctx *c, const char *who, int half, const double *w) {
  int rc = check_offsets(c, who, 0, 0);
  if (rc) return rc;
  if (half && (rc = check_spins(c, who, w, (size_t) c->B))) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = ensure_velocities(c))) return rc;
  mark_motion_set(c, half);
  return upload_motion(c, w, c->pv_cur, pv_rows(c), half);
}
int set_motion_dev(dc_ctx *c, const char *who, int half, const void *d_w, int is_f32) {
  int rc = check_offsets(c, who, 0, 0);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = ensure_velocities(c))) return rc;
  mark_motion_set(c, half);
  if (d_w) launch_cast_in_half(d_w, is_f32, c->pv_cur, (long) pv_rows(c), half, c->stream);
  else HIPCHK(c, hipMemset2DAsync(c->pv_cur + 3 * half, sizeof(float) * kPvRow, 0, sizeof(float) * 3, pv_rows(c), c->stream));
  HIPCHK(c, hipGetLastError());
  return DC_OK;
}
int set_motion_schedule(dc_ctx *c, const char *who, int half, int slot0, int nsteps, const double *w) {
  int rc = check_offsets(c, who, slot0, slot0 + nsteps);
  if (rc) return rc;
  if (nsteps < 1 || !w) return fail(c, DC_ERR_INVALID, std::string(who) + ": null schedule");
  if (half && (rc = check_spins(c, who, w, (size_t) nsteps * c->B))) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = ensure_velocities(c))) return rc;
  mark_motion_set(c, half);
  if ((rc = upload_motion(c, w, pv_slot(c, slot0 + 1), pv_rows(c) * nsteps, half))) return rc;
  mark_motion_scheduled(c, half, slot0, nsteps);
  return DC_OK;
}
int set_motion_schedule_dev(dc_ctx *c, const char *who, int half, int slot0, int nsteps, const void *d_w, int is_f32) {
  int rc = check_offsets(c, who, slot0, slot0 + nsteps);
  if (rc) return rc;
  if (nsteps < 1 || !d_w) return fail(c, DC_ERR_INVALID, std::string(who) + ": null schedule");
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = ensure_velocities(c))) return rc;
  mark_motion_set(c, half);
  launch_cast_in_half(d_w, is_f32, pv_slot(c, slot0 + 1), (long) (pv_rows(c) * nsteps), half, c->stream);      // one launch for all slots
  HIPCHK(c, hipGetLastError());
  mark_motion_scheduled(c, half, slot0, nsteps);
  return DC_OK;
}
int get_motion(dc_ctx *c, const char *who, int half, int slot, double *w) {
  int rc = check_batch(c, slot, slot);
  if (rc) return rc;
  if (slot < 1 || !w) return fail(c, DC_ERR_INVALID, std::string(who) + ": slot 0 has no record");
  const size_t n = pv_rows(c) * 3;
  if (!c->PV || !n) {      // (none was ever set: the step used none)
    for (size_t k = 0; k < n; k++) w[k] = 0.0;
    return DC_OK;
  }
  return download_motion(c, pv_slot(c, slot), w, pv_rows(c), half);
}
int get_motion_gradients(dc_ctx *c, const char *who, int half, int slot0, int nslots, double *out) {
  int rc = check_batch(c, slot0, slot0 + nslots - 1);
  if (rc) return rc;
  if (slot0 < 1 || nslots < 1 || !out) return fail(c, DC_ERR_INVALID, std::string(who) + ": slot 0 has no record");
  if (!c->PV || !motion_was_set(c, half))
    return fail(c, DC_ERR_STATE, std::string(who) + (half ? ": no primitive spin has been set on this batch" : ": no primitive velocity has been set on this batch"));
  return download_motion(c, dpv_slot(c, slot0), out, pv_rows(c) * nslots, half);
}
int get_motion_gradients_dev(dc_ctx *c, const char *who, int half, int slot0, int nslots, void *d_out, int is_f32) {
  int rc = check_batch(c, slot0, slot0 + nslots - 1);
  if (rc) return rc;
  if (slot0 < 1 || nslots < 1 || !d_out) return fail(c, DC_ERR_INVALID, std::string(who) + ": slot 0 has no record");
  if (!c->PV || !motion_was_set(c, half))
    return fail(c, DC_ERR_STATE, std::string(who) + (half ? ": no primitive spin has been set on this batch" : ": no primitive velocity has been set on this batch"));
  HIPCHK(c, hipSetDevice(c->device));
  launch_copy_cast_half(dpv_slot(c, slot0), d_out, is_f32, (long) (pv_rows(c) * nslots), half, c->stream);
  HIPCHK(c, hipGetLastError());
  return DC_OK;
}
}  // namespace

int dc_set_primitive_velocities(dc_ctx *c, const double *w) { return set_motion(c, "dc_set_primitive_velocities", 0, w); }
int dc_set_primitive_velocities_dev(dc_ctx *c, const void *d_w, int is_f32) { return set_motion_dev(c, "dc_set_primitive_velocities_dev", 0, d_w, is_f32); }
int dc_set_primitive_velocity_schedule(dc_ctx *c, int slot0, int nsteps, const double *w) {
  return set_motion_schedule(c, "dc_set_primitive_velocity_schedule", 0, slot0, nsteps, w);
}
int dc_set_primitive_velocity_schedule_dev(dc_ctx *c, int slot0, int nsteps, const void *d_w, int is_f32) {
  return set_motion_schedule_dev(c, "dc_set_primitive_velocity_schedule_dev", 0, slot0, nsteps, d_w, is_f32);
}
int dc_get_primitive_velocities(dc_ctx *c, int slot, double *w) { return get_motion(c, "dc_get_primitive_velocities", 0, slot, w); }
int dc_get_primitive_velocity_gradients(dc_ctx *c, int slot0, int nslots, double *dL_dw) {
  return get_motion_gradients(c, "dc_get_primitive_velocity_gradients", 0, slot0, nslots, dL_dw);
}
int dc_get_primitive_velocity_gradients_dev(dc_ctx *c, int slot0, int nslots, void *d_dL_dw, int is_f32) {
  return get_motion_gradients_dev(c, "dc_get_primitive_velocity_gradients_dev", 0, slot0, nslots, d_dL_dw, is_f32);
}

// ---- spinning obstacles: an angular velocity omega[b][g] per rollout and primitive group, per step: the other half of the motion rows, under
//      the rules of the velocity entries (include/diffcloth_hip.h holds the rule). The reference's only spin is its hard-wired `rotates` sphere ----
int dc_set_primitive_spins(dc_ctx *c, const double *omega) { return set_motion(c, "dc_set_primitive_spins", 1, omega); }
int dc_set_primitive_spins_dev(dc_ctx *c, const void *d_omega, int is_f32) { return set_motion_dev(c, "dc_set_primitive_spins_dev", 1, d_omega, is_f32); }
int dc_set_primitive_spin_schedule(dc_ctx *c, int slot0, int nsteps, const double *omega) {
  return set_motion_schedule(c, "dc_set_primitive_spin_schedule", 1, slot0, nsteps, omega);
}
int dc_set_primitive_spin_schedule_dev(dc_ctx *c, int slot0, int nsteps, const void *d_omega, int is_f32) {
  return set_motion_schedule_dev(c, "dc_set_primitive_spin_schedule_dev", 1, slot0, nsteps, d_omega, is_f32);
}
int dc_get_primitive_spins(dc_ctx *c, int slot, double *omega) { return get_motion(c, "dc_get_primitive_spins", 1, slot, omega); }
int dc_get_primitive_spin_gradients(dc_ctx *c, int slot0, int nslots, double *dL_domega) {
  return get_motion_gradients(c, "dc_get_primitive_spin_gradients", 1, slot0, nslots, dL_domega);
}
int dc_get_primitive_spin_gradients_dev(dc_ctx *c, int slot0, int nslots, void *d_dL_domega, int is_f32) {
  return get_motion_gradients_dev(c, "dc_get_primitive_spin_gradients_dev", 1, slot0, nslots, d_dL_domega, is_f32);
}

// ---- obstacle shapes: a row {top_offset[3], corner2[3], radius, length} per rollout, flattened primitive and step (dc_primshape.h holds the
//      conversion, shared with dc_build's DevPrim fill: a context given a shape equals a context built with it) ----
namespace {
// The shape table and its current set come with the first setter after dc_alloc_batch, every row holding the built shapes: a context that
// never calls one hands a null pointer to its kernels, which then read DevPrim.
int ensure_shapes(dc_ctx *c) {
  if (c->PS) return DC_OK;
  const size_t per = ps_elems(c), slots = (size_t) c->tape + 1;
  float *ps = nullptr, *cur = nullptr;
  int rc;
  if ((rc = dev_alloc(c, c->batch_allocs, &ps, per * slots))) return rc;
  if ((rc = dev_alloc(c, c->batch_allocs, &cur, per))) return rc;
  // (enqueued, no synchronisation: ps_built has been on the device since dc_alloc_batch)
  HIPCHK(c, hipMemcpyAsync(cur, c->ps_built, per * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
  for (size_t s = 0; s < slots; s++) { HIPCHK(c, hipMemcpyAsync(ps + per * s, c->ps_built, per * sizeof(float), hipMemcpyDeviceToDevice, c->stream)); }
  c->PS = ps; c->ps_cur = cur;      // (steps enqueued from here on see the table; those already enqueued read DevPrim: the same values)
  c->ps_row_gen.assign(slots + 1, 0); c->ps_gen = 0; c->ps_gen_last = 0;
  return DC_OK;
}
// rows x [P][8] host values -> fp32 in `dst`; null = the built shapes. Refuses non-finite values and, for a discretised sphere (whose face table
// was built for one radius and whose row the kernels do not read), a row that differs from the built one after rounding. Synchronises.
int upload_shapes(dc_ctx *c, const char *who, const double *s, float *dst, long rows) {
  const int P = c->S.nprim;
  std::vector<float> one;
  built_shape_rows(c, one);
  std::vector<float> v((size_t) rows * P * kShapeRow);
  for (long r = 0; r < rows; r++)
    for (int p = 0; p < P; p++) {
      float *out = v.data() + ((size_t) r * P + p) * kShapeRow;
      const float *built = one.data() + (size_t) p * kShapeRow;
      if (!s) { std::copy(built, built + kShapeRow, out); continue; }
      const double *in = s + ((size_t) r * P + p) * kShapeRow;
      for (int k = 0; k < kShapeRow; k++)
        if (!std::isfinite(in[k])) return fail(c, DC_ERR_INVALID, std::string(who) + ": non-finite shape value");
      round_shape_row(in, out);
      if (c->prims[p].kind == DC_PRIM_SPHERE_DISCRETIZED && std::memcmp(out, built, sizeof(float) * kShapeRow) != 0)
        return fail(c, DC_ERR_INVALID, std::string(who) + ": the shape of a discretised sphere cannot change (its face table is built for one radius)");
    }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (!v.empty()) HIPCHK(c, hipMemcpy(dst, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
  return DC_OK;
}
}  // namespace

int dc_set_primitive_shapes(dc_ctx *c, const double *s) {
  int rc = check_offsets(c, "dc_set_primitive_shapes", 0, 0);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = ensure_shapes(c))) return rc;
  if ((rc = upload_shapes(c, "dc_set_primitive_shapes", s, c->ps_cur, c->B))) return rc;
  c->ps_gen = s ? ++c->ps_gen_last : 0;
  return DC_OK;
}

int dc_set_primitive_shapes_dev(dc_ctx *c, const void *d_s, int is_f32) {
  int rc = check_offsets(c, "dc_set_primitive_shapes_dev", 0, 0);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = ensure_shapes(c))) return rc;
  if (d_s) launch_cast_in(d_s, is_f32, c->ps_cur, (long) ps_elems(c), c->stream);
  else HIPCHK(c, hipMemcpyAsync(c->ps_cur, c->ps_built, sizeof(float) * ps_elems(c), hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipGetLastError());
  c->ps_gen = d_s ? ++c->ps_gen_last : 0;
  return DC_OK;
}

int dc_set_primitive_shape_schedule(dc_ctx *c, int slot0, int nsteps, const double *s) {
  int rc = check_offsets(c, "dc_set_primitive_shape_schedule", slot0, slot0 + nsteps);
  if (rc) return rc;
  if (nsteps < 1 || !s) return fail(c, DC_ERR_INVALID, "dc_set_primitive_shape_schedule: null schedule");
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = ensure_shapes(c))) return rc;
  if ((rc = upload_shapes(c, "dc_set_primitive_shape_schedule", s, ps_slot(c, slot0 + 1), (long) nsteps * c->B))) return rc;
  for (int k = 1; k <= nsteps; k++) { c->sched_ps[slot0 + k] = 1; c->ps_row_gen[slot0 + k] = -1; }
  return DC_OK;
}

int dc_set_primitive_shape_schedule_dev(dc_ctx *c, int slot0, int nsteps, const void *d_s, int is_f32) {
  int rc = check_offsets(c, "dc_set_primitive_shape_schedule_dev", slot0, slot0 + nsteps);
  if (rc) return rc;
  if (nsteps < 1 || !d_s) return fail(c, DC_ERR_INVALID, "dc_set_primitive_shape_schedule_dev: null schedule");
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = ensure_shapes(c))) return rc;
  launch_cast_in(d_s, is_f32, ps_slot(c, slot0 + 1), (long) (ps_elems(c) * nsteps), c->stream);      // one launch for all slots
  HIPCHK(c, hipGetLastError());
  for (int k = 1; k <= nsteps; k++) { c->sched_ps[slot0 + k] = 1; c->ps_row_gen[slot0 + k] = -1; }
  return DC_OK;
}

int dc_get_primitive_shapes(dc_ctx *c, int slot, double *s) {
  int rc = check_batch(c, slot, slot);
  if (rc) return rc;
  if (slot < 1 || !s) return fail(c, DC_ERR_INVALID, "dc_get_primitive_shapes: slot 0 has no record");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::vector<float> v(ps_elems(c));
  if (c->PS) {
    if (!v.empty()) HIPCHK(c, hipMemcpy(v.data(), ps_slot(c, slot), v.size() * sizeof(float), hipMemcpyDeviceToHost));
  } else {      // no shape was ever set: the step read DevPrim
    std::vector<float> one;
    built_shape_rows(c, one);
    for (int b = 0; b < c->B; b++) std::copy(one.begin(), one.end(), v.begin() + (size_t) b * one.size());
  }
  for (size_t k = 0; k < v.size(); k++) s[k] = v[k];
  return DC_OK;
}

int dc_set_gradient(dc_ctx *c, const double *dL_dx, const double *dL_dv) {
  int rc = check_batch(c, 0, 0);
  if (rc) return rc;
  if (!dL_dx || !dL_dv) return fail(c, DC_ERR_INVALID, "dc_set_gradient: null gradient");
  c->rw_arrived = -1;      // a gradient from outside: no chain
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = h2d_planar(c, dL_dx, c->GX, c->host.N, true))) return rc;
  if ((rc = h2d_planar(c, dL_dv, c->GV, c->host.N, true))) return rc;
  HIPCHK(c, hipMemsetAsync(c->DMU, 0, sizeof(float) * c->B * c->S.ngroups, c->stream));
  return stage_sync(c);
}

int dc_get_states(dc_ctx *c, int slot0, int nslots, double *x, double *v) {
  int rc = check_batch(c, slot0, slot0 + nslots - 1);
  if (rc) return rc;
  if (nslots < 1) return fail(c, DC_ERR_INVALID, "dc_get_states: nslots < 1");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t se = slot_elems(c);
  for (int k = 0; k < nslots; k++) {
    if (x && (rc = d2h_planar(c, c->X + se * (slot0 + k), x + se * k, c->host.N, true))) return rc;
    if (v && (rc = d2h_planar(c, c->V + se * (slot0 + k), v + se * k, c->host.N, true))) return rc;
  }
  return stage_sync(c);
}

int dc_get_dxfixed(dc_ctx *c, int slot0, int nslots, double *dL_dxfixed) {
  int rc = check_batch(c, slot0, slot0 + nslots - 1);
  if (rc) return rc;
  if (slot0 < 1 || nslots < 1 || !dL_dxfixed) return fail(c, DC_ERR_INVALID, "dc_get_dxfixed: slot 0 has no record");
  const int Af = c->S.Af;
  if (Af <= 0) return DC_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t per = xf_elems(c);
  for (int k = 0; k < nslots; k++)
    if ((rc = d2h_planar(c, dxf_slot(c, slot0 + k), dL_dxfixed + per * k, Af, false))) return rc;
  return stage_sync(c);
}

int dc_get_param_gradients(dc_ctx *c, int slot, double *out) {
  int rc = check_batch(c, slot, slot);
  if (rc) return rc;
  if (slot < 1 || !out) return fail(c, DC_ERR_INVALID, "dc_get_param_gradients: slot 0 has no record");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::vector<float> v((size_t) c->B * 8);
  HIPCHK(c, hipMemcpy(v.data(), dpar_slot(c, slot), v.size() * sizeof(float), hipMemcpyDeviceToHost));
  for (size_t k = 0; k < v.size(); k++) out[k] = v[k];
  return DC_OK;
}

// ---- whole-sweep device-pointer boundary: the rollout calls, the schedule setters and the getters of a sweep's results for callers whose
//      tensors live on this GPU (diffcloth_amd/functional.py: sim_rollout). Every buffer is a DEVICE pointer in the caller's layout, all slots
//      of an array are converted in one launch (dc_boundary.hip), everything is enqueued on the context's stream and nothing synchronises.
int dc_rollout_forward_async(dc_ctx *c, int slot, int nsteps) {
  int rc = check_batch(c, slot, slot + nsteps);
  if (rc) return rc;
  if (nsteps < 1) return fail(c, DC_ERR_INVALID, "dc_rollout_forward_async: nsteps < 1");
  HIPCHK(c, hipSetDevice(c->device));
  return enqueue_forward_steps(c, slot, nsteps, true, nullptr);
}

int dc_rollout_backward_async(dc_ctx *c, int slot, int nsteps) {
  int rc = check_batch(c, slot - nsteps + 1, slot);
  if (rc) return rc;
  if (nsteps < 1 || slot - nsteps + 1 < 1) return fail(c, DC_ERR_INVALID, "dc_rollout_backward_async: would run past slot 1");
  HIPCHK(c, hipSetDevice(c->device));
  return enqueue_backward_steps(c, slot, nsteps, Seeds::schedule, nullptr, nullptr);
}

int dc_set_fixed_point_schedule_dev(dc_ctx *c, int slot0, int nsteps, const void *d_xf, int is_f32) {
  int rc = check_batch(c, slot0, slot0 + nsteps);
  if (rc) return rc;
  if (nsteps < 1 || !d_xf) return fail(c, DC_ERR_INVALID, "dc_set_fixed_point_schedule_dev: null schedule");
  const int Af = c->S.Af;
  if (Af <= 0) return DC_OK;
  HIPCHK(c, hipSetDevice(c->device));
  launch_rows_to_planar(d_xf, is_f32, xf_slot(c, slot0 + 1), (long) nsteps * c->B, Af, nullptr, c->stream);
  HIPCHK(c, hipGetLastError());
  for (int k = 1; k <= nsteps; k++) c->sched_xf[slot0 + k] = 1;
  return DC_OK;
}

int dc_set_force_schedule_dev(dc_ctx *c, int slot0, int nsteps, const void *d_fu, const void *d_fv_scale, int is_f32) {
  int rc = check_batch(c, slot0, slot0 + nsteps);
  if (rc) return rc;
  if (nsteps < 1) return fail(c, DC_ERR_INVALID, "dc_set_force_schedule_dev: nsteps < 1");
  HIPCHK(c, hipSetDevice(c->device));
  if (d_fu) launch_cast_in(d_fu, is_f32, c->FU_S + (size_t) c->B * 3 * (slot0 + 1), (long) nsteps * c->B * 3, c->stream);
  if (d_fv_scale) launch_cast_in(d_fv_scale, is_f32, c->FVS_S + (size_t) c->B * (slot0 + 1), (long) nsteps * c->B, c->stream);
  HIPCHK(c, hipGetLastError());
  for (int k = 1; k <= nsteps; k++) { c->sched_fu[slot0 + k] = d_fu ? 1 : 0; c->sched_fvs[slot0 + k] = d_fv_scale ? 1 : 0; }
  return DC_OK;
}

int dc_set_seed_schedule_dev(dc_ctx *c, int slot0, int nslots, const void *d_dL_dx, const void *d_dL_dv, int is_f32) {
  int rc = check_batch(c, slot0, slot0 + nslots - 1);
  if (rc) return rc;
  if (nslots < 1) return fail(c, DC_ERR_INVALID, "dc_set_seed_schedule_dev: nslots < 1");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t se = slot_elems(c), slots = (size_t) c->tape + 1;
  if (!c->SEEDX) {
    if ((rc = dev_alloc(c, c->batch_allocs, &c->SEEDX, se * slots))) return rc;
    if ((rc = dev_alloc(c, c->batch_allocs, &c->SEEDV, se * slots))) return rc;
  }
  const long rows = (long) nslots * c->B;
  if (d_dL_dx) launch_rows_to_planar(d_dL_dx, is_f32, seedx_slot(c, slot0), rows, c->host.N, c->d_user_of, c->stream);
  else HIPCHK(c, hipMemsetAsync(seedx_slot(c, slot0), 0, se * nslots * sizeof(float), c->stream));
  if (d_dL_dv) launch_rows_to_planar(d_dL_dv, is_f32, seedv_slot(c, slot0), rows, c->host.N, c->d_user_of, c->stream);
  else HIPCHK(c, hipMemsetAsync(seedv_slot(c, slot0), 0, se * nslots * sizeof(float), c->stream));
  HIPCHK(c, hipGetLastError());
  for (int k = 0; k < nslots; k++) c->sched_seed[slot0 + k] = 1;
  return DC_OK;
}

int dc_set_gradient_dev(dc_ctx *c, const void *d_dL_dx, const void *d_dL_dv, int is_f32) {
  int rc = check_batch(c, 0, 0);
  if (rc) return rc;
  if (!d_dL_dx || !d_dL_dv) return fail(c, DC_ERR_INVALID, "dc_set_gradient_dev: null gradient");
  c->rw_arrived = -1;
  HIPCHK(c, hipSetDevice(c->device));
  launch_rows_to_planar(d_dL_dx, is_f32, c->GX, c->B, c->host.N, c->d_user_of, c->stream);
  launch_rows_to_planar(d_dL_dv, is_f32, c->GV, c->B, c->host.N, c->d_user_of, c->stream);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemsetAsync(c->DMU, 0, sizeof(float) * c->B * c->S.ngroups, c->stream));
  return DC_OK;
}

int dc_get_gradient_dev(dc_ctx *c, void *d_dL_dx, void *d_dL_dv, void *d_dL_dmu, int is_f32) {
  int rc = check_batch(c, 0, 0);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  if (d_dL_dx) launch_planar_to_rows(c->GX, d_dL_dx, is_f32, c->B, c->host.N, c->d_user_of, c->stream);
  if (d_dL_dv) launch_planar_to_rows(c->GV, d_dL_dv, is_f32, c->B, c->host.N, c->d_user_of, c->stream);
  if (d_dL_dmu) launch_copy_cast(c->DMU, d_dL_dmu, is_f32, (long) c->B * c->S.ngroups, c->stream);
  HIPCHK(c, hipGetLastError());
  return DC_OK;
}

int dc_get_states_dev(dc_ctx *c, int slot0, int nslots, void *d_x, void *d_v, int is_f32) {
  int rc = check_batch(c, slot0, slot0 + nslots - 1);
  if (rc) return rc;
  if (nslots < 1) return fail(c, DC_ERR_INVALID, "dc_get_states_dev: nslots < 1");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t se = slot_elems(c);
  const long rows = (long) nslots * c->B;
  if (d_x) launch_planar_to_rows(c->X + se * slot0, d_x, is_f32, rows, c->host.N, c->d_user_of, c->stream);
  if (d_v) launch_planar_to_rows(c->V + se * slot0, d_v, is_f32, rows, c->host.N, c->d_user_of, c->stream);
  HIPCHK(c, hipGetLastError());
  return DC_OK;
}

int dc_get_dxfixed_dev(dc_ctx *c, int slot0, int nslots, void *d_dL_dxfixed, int is_f32) {
  int rc = check_batch(c, slot0, slot0 + nslots - 1);
  if (rc) return rc;
  if (slot0 < 1 || nslots < 1 || !d_dL_dxfixed) return fail(c, DC_ERR_INVALID, "dc_get_dxfixed_dev: slot 0 has no record");
  const int Af = c->S.Af;
  if (Af <= 0) return DC_OK;
  HIPCHK(c, hipSetDevice(c->device));
  launch_planar_to_rows(dxf_slot(c, slot0), d_dL_dxfixed, is_f32, (long) nslots * c->B, Af, nullptr, c->stream);
  HIPCHK(c, hipGetLastError());
  return DC_OK;
}

int dc_get_force_schedule_gradients_dev(dc_ctx *c, int slot0, int nslots, void *d_dL_dfu, void *d_dL_dfv_scale, void *d_dL_dfv, int is_f32) {
  int rc = check_batch(c, slot0, slot0 + nslots - 1);
  if (rc) return rc;
  if (slot0 < 1 || nslots < 1) return fail(c, DC_ERR_INVALID, "dc_get_force_schedule_gradients_dev: slot 0 has no record");
  if ((d_dL_dfv_scale || d_dL_dfv) && !c->YS)
    return fail(c, DC_ERR_STATE, "dc_get_force_schedule_gradients_dev: dc_keep_force_gradients(1) was not set before the backward sweep");
  if (d_dL_dfv_scale && !c->fv_set) return fail(c, DC_ERR_STATE, "dc_get_force_schedule_gradients_dev: no per-vertex force is set (dc_set_vertex_forces)");
  HIPCHK(c, hipSetDevice(c->device));
  const double h2 = c->params.time_step * c->params.time_step;
  const float *ys = c->YS ? c->YS + slot_elems(c) * slot0 : nullptr;
  if (d_dL_dfu) launch_dfu_from_param(dpar_slot(c, slot0), d_dL_dfu, is_f32, (long) nslots * c->B, c->stream);
  if (d_dL_dfv_scale) launch_dfv_scale(ys, c->fv, d_dL_dfv_scale, is_f32, nslots, c->B, c->host.N, h2, c->stream);
  if (d_dL_dfv) {
    // the factors of the steps through these records: the fv_scale schedule where one is set on all of them, else 1
    int nfvs = 0;
    for (int k = 0; k < nslots; k++) nfvs += c->sched_fvs[slot0 + k];
    if (nfvs % nslots) return fail(c, DC_ERR_INVALID, "dc_get_force_schedule_gradients_dev: the fv_scale schedule covers only part of the slots");
    launch_dfv(ys, nfvs ? c->FVS_S + (size_t) c->B * slot0 : nullptr, d_dL_dfv, is_f32, nslots, c->B, c->host.N, c->d_user_of, h2, c->stream);
  }
  HIPCHK(c, hipGetLastError());
  return DC_OK;
}

// ---- contact read-out (dc_readout.hip): state, normal impulse and per-group wrench rows of the records slot0 .. slot0 + nslots - 1
namespace {
int readout_check(dc_ctx *c, const char *who, int slot0, int nslots, const void *state, const void *jn, const void *wrench) {
  if (!c) return DC_ERR_INVALID;
  const std::string w(who);
  if (slot0 < 1) return fail(c, DC_ERR_INVALID, w + ": slot 0 has no record");
  if (nslots < 1) return fail(c, DC_ERR_INVALID, w + ": nslots < 1");
  if (!state && !jn && !wrench) return fail(c, DC_ERR_INVALID, w + ": state, normal_impulse and wrench are all null");
  if (!c->built) return fail(c, DC_ERR_STATE, "dc_build has not been called");
  if (wrench && c->ngroups < 1) return fail(c, DC_ERR_INVALID, w + ": wrench asked of a context with no primitive group");
  if (c->B > 0 && (long) slot0 + nslots - 1 > c->tape) return fail(c, DC_ERR_INVALID, w + ": slots " + std::to_string(slot0) + " .. " + std::to_string((long) slot0 + nslots - 1) + " reach past the tape of " + std::to_string(c->tape) + " steps");
  return check_batch(c, slot0, slot0 + nslots - 1);
}
void readout_enqueue(dc_ctx *c, int slot0, int nslots, int *state, void *jn, void *wrench, int is_f32) {
  const size_t se = slot_elems(c), sp = (size_t) c->B * c->host.N;
  launch_contact_readout(c->S, c->X + se * slot0, c->F + se * slot0, c->NRM + se * slot0, c->PRIM + sp * slot0, pc_slot(c, slot0),
                         c->PV ? pv_slot(c, slot0) : nullptr, c->mu, (long) nslots * c->B, c->B, state, jn, wrench, is_f32, c->stream);
}
// device memory of one host-form call, freed when the call returns
struct ReadoutStage {
  void *p = nullptr;
  ~ReadoutStage() { if (p) (void) hipFree(p); }
};
}  // namespace

int dc_get_contact_readout_dev(dc_ctx *c, int slot0, int nslots, void *d_state, void *d_normal_impulse, void *d_wrench, int is_f32) {
  int rc = readout_check(c, "dc_get_contact_readout_dev", slot0, nslots, d_state, d_normal_impulse, d_wrench);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  readout_enqueue(c, slot0, nslots, (int *) d_state, d_normal_impulse, d_wrench, is_f32);
  HIPCHK(c, hipGetLastError());
  return DC_OK;
}

int dc_get_contact_readout(dc_ctx *c, int slot0, int nslots, int *state, double *normal_impulse, double *wrench) {
  int rc = readout_check(c, "dc_get_contact_readout", slot0, nslots, state, normal_impulse, wrench);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t nv = (size_t) nslots * c->B * c->host.N, nw = (size_t) nslots * c->B * c->ngroups * kWrenchRow;
  ReadoutStage ds, dj, dw;
  if (state) HIPCHK(c, hipMalloc(&ds.p, nv * sizeof(int)));
  if (normal_impulse) HIPCHK(c, hipMalloc(&dj.p, nv * sizeof(double)));
  if (wrench) HIPCHK(c, hipMalloc(&dw.p, nw * sizeof(double)));
  readout_enqueue(c, slot0, nslots, (int *) ds.p, dj.p, dw.p, 0);
  HIPCHK(c, hipGetLastError());
  if (state) HIPCHK(c, hipMemcpyAsync(state, ds.p, nv * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  if (normal_impulse) HIPCHK(c, hipMemcpyAsync(normal_impulse, dj.p, nv * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (wrench) HIPCHK(c, hipMemcpyAsync(wrench, dw.p, nw * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return cluster_check(c);
}

// ---- self-contact read-out (dc_self_readout.hip): per-pair impulses, per-vertex sums and totals of the records slot0 .. slot0 + nslots - 1
namespace {
int self_readout_check(dc_ctx *c, const char *who, int slot0, int nslots, int cap, const void *pairs, const void *impulse, const void *vimp,
                       const void *totals) {
  if (!c) return DC_ERR_INVALID;
  const std::string w(who);
  if (slot0 < 1) return fail(c, DC_ERR_INVALID, w + ": slot 0 has no record");
  if (nslots < 1) return fail(c, DC_ERR_INVALID, w + ": nslots < 1");
  if (!pairs && !impulse && !vimp && !totals) return fail(c, DC_ERR_INVALID, w + ": pairs, impulse, vertex_impulse and totals are all null");
  if (cap < 1 && (pairs || impulse)) return fail(c, DC_ERR_INVALID, w + ": cap < 1 while pairs or impulse is asked for");
  if (!c->built) return fail(c, DC_ERR_STATE, "dc_build has not been called");
  if (c->B > 0 && (long) slot0 + nslots - 1 > c->tape) return fail(c, DC_ERR_INVALID, w + ": slots " + std::to_string(slot0) + " .. " + std::to_string((long) slot0 + nslots - 1) + " reach past the tape of " + std::to_string(c->tape) + " steps");
  return check_batch(c, slot0, slot0 + nslots - 1);
}
// Enqueues the range: ONE launch when every record the context can hold fits the kernel's LDS plan; otherwise slot by slot, because the rows
// that take the global-memory walk share the [B] scratch planes (allocated here, by the first such call after dc_alloc_batch).
int self_readout_enqueue(dc_ctx *c, int slot0, int nslots, int cap, int *pairs, void *impulse, void *vimp, void *totals, int is_f32) {
  const SelfRoPlan plan = selfro_plan(c->host.N, c->self_cap, selfro_lds_limit(kSelfRoLdsFloatsMax));
  int rc;
  if (plan.scratch && !c->sro_sums) {      // (sro_sums is the second of the two: a failed allocation leaves it null and the next call starts over)
    if ((rc = dev_alloc(c, c->batch_allocs, &c->sro_scratch, slot_elems(c)))) return rc;
    if ((rc = dev_alloc(c, c->batch_allocs, &c->sro_sums, slot_elems(c)))) return rc;
  }
  const size_t se = slot_elems(c), sp = (size_t) c->B * c->host.N;
  SelfRoArgs A;
  A.F = c->F + se * slot0; A.NRM = c->NRM + se * slot0; A.PRIM = c->PRIM + sp * slot0;
  A.PV = c->PV ? pv_slot(c, slot0) : nullptr; A.mu = c->mu; A.R = self_slot(c, slot0);
  A.B = c->B; A.row0 = 0; A.cap_out = std::max(cap, 0); A.lds_floats = plan.lds_floats;
  A.scratch = plan.scratch ? c->sro_scratch : nullptr; A.sums = plan.scratch ? c->sro_sums : nullptr;
  if (!plan.scratch) {
    HIPCHK(c, launch_self_readout(c->S, A, (long) nslots * c->B, pairs, impulse, vimp, totals, is_f32, c->stream));
    return DC_OK;
  }
  for (int k = 0; k < nslots; k++) {
    A.row0 = k * c->B;
    HIPCHK(c, launch_self_readout(c->S, A, c->B, pairs, impulse, vimp, totals, is_f32, c->stream));
  }
  return DC_OK;
}
}  // namespace

int dc_get_self_contact_readout_dev(dc_ctx *c, int slot0, int nslots, int cap, void *d_pairs, void *d_impulse, void *d_vertex_impulse, void *d_totals,
                                    int is_f32) {
  int rc = self_readout_check(c, "dc_get_self_contact_readout_dev", slot0, nslots, cap, d_pairs, d_impulse, d_vertex_impulse, d_totals);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  return self_readout_enqueue(c, slot0, nslots, cap, (int *) d_pairs, d_impulse, d_vertex_impulse, d_totals, is_f32);
}

int dc_get_self_contact_readout(dc_ctx *c, int slot0, int nslots, int cap, int *pairs, double *impulse, double *vertex_impulse, double *totals) {
  int rc = self_readout_check(c, "dc_get_self_contact_readout", slot0, nslots, cap, pairs, impulse, vertex_impulse, totals);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t rows = (size_t) nslots * c->B, np = rows * (size_t) std::max(cap, 0) * 4, nv = rows * 3 * c->host.N, nt = rows * kSelfRoTotals;
  ReadoutStage dp, di, dv, dt;
  if (pairs) HIPCHK(c, hipMalloc(&dp.p, np * sizeof(int)));
  if (impulse) HIPCHK(c, hipMalloc(&di.p, np * sizeof(double)));
  if (vertex_impulse) HIPCHK(c, hipMalloc(&dv.p, nv * sizeof(double)));
  if (totals) HIPCHK(c, hipMalloc(&dt.p, nt * sizeof(double)));
  if ((rc = self_readout_enqueue(c, slot0, nslots, cap, (int *) dp.p, di.p, dv.p, dt.p, 0))) return rc;
  if (pairs) HIPCHK(c, hipMemcpyAsync(pairs, dp.p, np * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  if (impulse) HIPCHK(c, hipMemcpyAsync(impulse, di.p, np * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (vertex_impulse) HIPCHK(c, hipMemcpyAsync(vertex_impulse, dv.p, nv * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (totals) HIPCHK(c, hipMemcpyAsync(totals, dt.p, nt * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return cluster_check(c);
}

// ---- gradients of a loss on the contact read-out (dc_readout_adjoint.hip) ----
namespace {
int readout_gradients_check(dc_ctx *c, const char *who, int slot0, int nslots, const void *jn, const void *wrench) {
  if (!c) return DC_ERR_INVALID;
  const std::string w(who);
  if (!jn && !wrench) {      // clear
    if (!c->built) return fail(c, DC_ERR_STATE, "dc_build has not been called");
    if (c->B <= 0) return fail(c, DC_ERR_STATE, w + ": dc_alloc_batch has not been called");
    return DC_OK;
  }
  if (slot0 < 1) return fail(c, DC_ERR_INVALID, w + ": slot 0 has no record");
  if (nslots < 1) return fail(c, DC_ERR_INVALID, w + ": nslots < 1");
  if (!c->built) return fail(c, DC_ERR_STATE, "dc_build has not been called");
  if (wrench && c->ngroups < 1) return fail(c, DC_ERR_INVALID, w + ": wrench weights given to a context with no primitive group");
  if (c->B > 0 && (long) slot0 + nslots - 1 > c->tape) return fail(c, DC_ERR_INVALID, w + ": slots " + std::to_string(slot0) + " .. " + std::to_string((long) slot0 + nslots - 1) + " reach past the tape of " + std::to_string(c->tape) + " steps");
  return check_batch(c, slot0, slot0 + nslots - 1);
}
// the weights of records slot0 .. slot0 + nslots - 1 from DEVICE buffers, enqueued; a null pointer = zeros for those records
int readout_gradients_enqueue(dc_ctx *c, int slot0, int nslots, const void *d_jn, const void *d_wrench, int is_f32) {
  int rc;
  const int N = c->host.N, G = std::max(c->ngroups, 1);
  const size_t slots = (size_t) c->tape + 1, pj = (size_t) c->B * N, pw = (size_t) c->B * G * kWrenchRow, se = slot_elems(c);
  if (!c->RSV) {      // (RSV is the last of the five: a failed allocation leaves it null and the next call starts over)
    auto &pool = c->batch_allocs;
    if ((rc = dev_alloc(c, pool, &c->RWJ, pj * slots))) return rc;
    if ((rc = dev_alloc(c, pool, &c->RWW, pw * slots))) return rc;
    if ((rc = dev_alloc(c, pool, &c->rw_has, slots))) return rc;
    if ((rc = dev_alloc(c, pool, &c->RSX, se * slots))) return rc;
    if ((rc = dev_alloc(c, pool, &c->RSV, se * slots))) return rc;
  }
  if (d_jn) launch_vertex_rows_in(d_jn, is_f32, c->RWJ + pj * slot0, (long) nslots * c->B, N, c->d_user_of, c->stream);
  else HIPCHK(c, hipMemsetAsync(c->RWJ + pj * slot0, 0, sizeof(float) * pj * nslots, c->stream));
  if (d_wrench) launch_cast_in(d_wrench, is_f32, c->RWW + pw * slot0, (long) (pw * nslots), c->stream);
  else HIPCHK(c, hipMemsetAsync(c->RWW + pw * slot0, 0, sizeof(float) * pw * nslots, c->stream));
  HIPCHK(c, hipMemsetAsync(c->rw_has + slot0, 1, (size_t) nslots, c->stream));
  HIPCHK(c, hipGetLastError());
  for (int k = 0; k < nslots; k++) c->sched_rw[slot0 + k] = 1;
  c->rw_arrived = -1;
  return DC_OK;
}
}  // namespace

int dc_set_contact_readout_gradients_dev(dc_ctx *c, int slot0, int nslots, const void *d_dL_djn, const void *d_dL_dwrench, int is_f32) {
  int rc = readout_gradients_check(c, "dc_set_contact_readout_gradients_dev", slot0, nslots, d_dL_djn, d_dL_dwrench);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  if (!d_dL_djn && !d_dL_dwrench) return clear_readout_gradients(c);
  return readout_gradients_enqueue(c, slot0, nslots, d_dL_djn, d_dL_dwrench, is_f32);
}

int dc_set_contact_readout_gradients(dc_ctx *c, int slot0, int nslots, const double *dL_djn, const double *dL_dwrench) {
  int rc = readout_gradients_check(c, "dc_set_contact_readout_gradients", slot0, nslots, dL_djn, dL_dwrench);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  if (!dL_djn && !dL_dwrench) return clear_readout_gradients(c);
  const size_t nj = (size_t) nslots * c->B * c->host.N, nw = (size_t) nslots * c->B * c->ngroups * kWrenchRow;
  ReadoutStage dj, dw;
  if (dL_djn) {
    HIPCHK(c, hipMalloc(&dj.p, nj * sizeof(double)));
    HIPCHK(c, hipMemcpyAsync(dj.p, dL_djn, nj * sizeof(double), hipMemcpyHostToDevice, c->stream));
  }
  if (dL_dwrench) {
    HIPCHK(c, hipMalloc(&dw.p, nw * sizeof(double)));
    HIPCHK(c, hipMemcpyAsync(dw.p, dL_dwrench, nw * sizeof(double), hipMemcpyHostToDevice, c->stream));
  }
  if ((rc = readout_gradients_enqueue(c, slot0, nslots, dj.p, dw.p, 0))) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return DC_OK;
}

int dc_set_mu_dev(dc_ctx *c, const void *d_mu, int is_f32) {
  int rc = check_batch(c, 0, 0);
  if (rc) return rc;
  if (!d_mu) return fail(c, DC_ERR_INVALID, "dc_set_mu_dev: null mu (dc_set_mu(NULL) restores the defaults)");
  HIPCHK(c, hipSetDevice(c->device));
  launch_cast_in(d_mu, is_f32, c->mu, (long) c->B * c->S.ngroups, c->stream);
  HIPCHK(c, hipGetLastError());
  return DC_OK;
}

int dc_set_vertex_forces_dev(dc_ctx *c, const void *d_f, int is_f32) {
  int rc = check_batch(c, 0, 0);
  if (rc) return rc;
  if (!d_f) { c->fv_set = false; return DC_OK; }
  HIPCHK(c, hipSetDevice(c->device));
  launch_rows_to_planar(d_f, is_f32, c->fv, c->B, c->host.N, c->d_user_of, c->stream);
  HIPCHK(c, hipGetLastError());
  c->fv_set = true;
  return DC_OK;
}

int dc_get_stats(dc_ctx *c, int slot, dc_step_stats *fwd, dc_bwd_stats *bwd) {
  int rc = check_batch(c, slot, slot);
  if (rc) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (fwd) HIPCHK(c, hipMemcpy(fwd, c->fstats + (size_t) c->B * slot, sizeof(dc_step_stats) * c->B, hipMemcpyDeviceToHost));
  if (fwd && slot >= 1 && (rc = check_self_overflow(c, fwd, slot))) return rc;
  if (bwd) HIPCHK(c, hipMemcpy(bwd, c->bstats + (size_t) c->B * slot, sizeof(dc_bwd_stats) * c->B, hipMemcpyDeviceToHost));
  return DC_OK;
}

int dc_sync(dc_ctx *c) {
  if (!c) return DC_ERR_INVALID;
  if (c->host_only) return DC_OK;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return cluster_check(c);
}

int dc_get_deflation(const dc_ctx *c, int *vectors, int *probe_iterations) {
  if (!c) return DC_ERR_INVALID;
  if (!c->built) return DC_ERR_STATE;
  if (vectors) *vectors = c->defl_k;
  if (probe_iterations) *probe_iterations = c->defl_probe;
  return DC_OK;
}

int dc_get_packet_layout(const dc_ctx *c, int *byte_offsets) {
  if (!c || !byte_offsets) return DC_ERR_INVALID;
  if (!c->built) return DC_ERR_STATE;
  *byte_offsets = c->S.pk_tpl ? 2 : c->S.pk_ofs;
  return DC_OK;
}

int dc_get_bend_rows(const dc_ctx *c, int *rows) {
  if (!c || !rows) return DC_ERR_INVALID;
  if (!c->built) return DC_ERR_STATE;
  *rows = c->S.win_rows;
  return DC_OK;
}

int dc_get_layout(const dc_ctx *c, int *out6) {
  if (!c || !out6) return DC_ERR_INVALID;
  if (!c->built) return DC_ERR_STATE;
  out6[0] = c->user_of.empty() ? 0 : 1; out6[1] = c->bandwidth; out6[2] = c->S.pk_ok; out6[3] = c->S.win_ok; out6[4] = c->S.nwin;
  out6[5] = c->S.dense_ld > 0 ? 1 : 0;
  return DC_OK;
}

int dc_get_cluster(const dc_ctx *c, int *workgroups_per_rollout, int *rollouts_per_launch) {
  if (!c) return DC_ERR_INVALID;
  if (workgroups_per_rollout) *workgroups_per_rollout = c->cl.ok ? c->cl.K : 1;
  if (rollouts_per_launch) *rollouts_per_launch = c->cl.ok ? c->cl.nb : c->B;
  return DC_OK;
}

int dc_get_cluster_rows(const dc_ctx *c, int *rows_per_part, int *halo_rows) {
  if (!c) return DC_ERR_INVALID;
  if (rows_per_part) *rows_per_part = c->cl.ok ? c->cl.D.R : 0;
  if (halo_rows) *halo_rows = c->cl.ok ? c->cl.D.HB : 0;
  return DC_OK;
}

int dc_get_self_friction_path(dc_ctx *c, int *out, int reset) {
  if (!c || !out) return DC_ERR_INVALID;
  std::memset(out, 0, sizeof(int) * 2 * (size_t) std::max(c->B, 0));
  if (!c->cl.ok || c->B <= 0) return DC_OK;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(out, c->cl.D.self_path, sizeof(int) * 2 * (size_t) c->B, hipMemcpyDeviceToHost));
  if (reset) HIPCHK(c, hipMemsetAsync(c->cl.D.self_path, 0, sizeof(int) * 2 * (size_t) c->B, c->stream));
  return DC_OK;
}

int dc_get_adjoint_contact_path(dc_ctx *c, int *out, int reset) {
  if (!c || !out) return DC_ERR_INVALID;
  std::memset(out, 0, sizeof(int) * 2 * (size_t) std::max(c->B, 0));
  if (!c->adj_path || c->B <= 0) return DC_OK;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(out, c->adj_path, sizeof(int) * 2 * (size_t) c->B, hipMemcpyDeviceToHost));
  if (reset) HIPCHK(c, hipMemsetAsync(c->adj_path, 0, sizeof(int) * 2 * (size_t) c->B, c->stream));
  return DC_OK;
}

int dc_timer_start(dc_ctx *c) {
  if (!c) return DC_ERR_INVALID;
  HIPCHK(c, hipEventRecord(c->ev_t0, c->stream));
  return DC_OK;
}
int dc_timer_stop(dc_ctx *c, float *ms) {
  if (!c || !ms) return DC_ERR_INVALID;
  HIPCHK(c, hipEventRecord(c->ev_t1, c->stream));
  HIPCHK(c, hipEventSynchronize(c->ev_t1));
  HIPCHK(c, hipEventElapsedTime(ms, c->ev_t0, c->ev_t1));
  return DC_OK;
}
int dc_get_adjoint_matrix(dc_ctx *c, int slot, int rollout, double *K) {
  int rc = check_batch(c, slot, slot);
  if (rc) return rc;
  if (slot < 1 || rollout < 0 || rollout >= c->B || !K) return fail(c, DC_ERR_INVALID, "dc_get_adjoint_matrix: bad slot / rollout / output");
  const int N = c->host.N, n = 3 * N;
  if ((rc = check_dense_mode(c, 2, N, "dc_get_adjoint_matrix"))) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  if (c->params.adjoint_mode == 3) {      // the band-assembled K, exact zeros outside the band
    if ((rc = band_ensure(c))) return rc;
    const BandAdjWork &D = c->band;
    launch_band_assemble(c->S, bwd_args(c, slot, false, Seeds::none), c->W.x64, D, rollout, 1, c->stream);
    HIPCHK(c, hipGetLastError());
    std::vector<double> Bd((size_t) D.ldab * n);
    HIPCHK(c, hipMemcpyAsync(Bd.data(), D.AB, Bd.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::fill(K, K + (size_t) n * n, 0.0);
    for (int col = 0; col < n; col++) {
      const int uj = c->user_of.empty() ? col / 3 : c->user_of[col / 3];
      for (int r = std::max(0, col - D.kl); r <= std::min(n - 1, col + D.kl); r++) {
        const int ui = c->user_of.empty() ? r / 3 : c->user_of[r / 3];
        K[(size_t) (3 * ui + r % 3) * n + 3 * uj + col % 3] = Bd[(size_t) col * D.ldab + (2 * D.kl + r - col)];
      }
    }
    return DC_OK;
  }
  if ((rc = dense_ensure(c))) return rc;
  const DenseAdjWork &D = c->dense;
  launch_dense_assemble(c->S, bwd_args(c, slot, false, Seeds::none), c->W.x64, D, rollout, 1, c->stream);
  HIPCHK(c, hipGetLastError());
  std::vector<double> Kd((size_t) D.ld * n);
  HIPCHK(c, hipMemcpyAsync(Kd.data(), D.K, Kd.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  // device (planar, renumbered, column-major) -> the caller's (xyz interleaved, caller's numbering, row-major)
  for (int cj = 0; cj < 3; cj++)
    for (int j = 0; j < N; j++) {
      const int uj = c->user_of.empty() ? j : c->user_of[j];
      const double *col = Kd.data() + (size_t) (cj * N + j) * D.ld;
      for (int ci = 0; ci < 3; ci++)
        for (int i = 0; i < N; i++) {
          const int ui = c->user_of.empty() ? i : c->user_of[i];
          K[(size_t) (3 * ui + ci) * n + 3 * uj + cj] = col[ci * N + i];
        }
    }
  return DC_OK;
}

int dc_set_adjoint_band(dc_ctx *c, int extra_vertices) {
  if (!c) return DC_ERR_INVALID;
  if (extra_vertices < 0) return fail(c, DC_ERR_INVALID, "dc_set_adjoint_band: extra_vertices must be >= 0");
  if (c->built) { const int rc = check_band_mode(c, c->params.adjoint_mode, extra_vertices, "dc_set_adjoint_band"); if (rc) return rc; }
  c->band_extra = extra_vertices;       // (band_ensure compares the band it allocated with the one now asked for)
  return DC_OK;
}

int dc_get_adjoint_band(const dc_ctx *c, int *kl, int *ldab, long long *bytes_per_rollout) {
  if (!c) return DC_ERR_INVALID;
  if (!c->built) return DC_ERR_STATE;
  const BandPlan bp = band_plan(c->host.N, c->bandwidth, c->band_extra);
  if (kl) *kl = bp.kl;
  if (ldab) *ldab = bp.ldab;
  if (bytes_per_rollout) *bytes_per_rollout = bp.bytes;
  return DC_OK;
}

int dc_dense_phase_times(dc_ctx *c, float *ms3, int reset) {
  if (!c || !ms3) return DC_ERR_INVALID;
  for (int k = 0; k < 3; k++) ms3[k] = c->dense_ms[k];
  if (reset) for (float &v : c->dense_ms) v = 0;
  return DC_OK;
}

int dc_kernel_times(dc_ctx *c, float *fwd_ms, int *fwd_launches, float *bwd_ms, int *bwd_launches, int reset) {
  if (!c) return DC_ERR_INVALID;
  if (fwd_ms) *fwd_ms = c->fwd_ms;
  if (fwd_launches) *fwd_launches = c->fwd_launches;
  if (bwd_ms) *bwd_ms = c->bwd_ms;
  if (bwd_launches) *bwd_launches = c->bwd_launches;
  if (reset) { c->fwd_ms = c->bwd_ms = 0; c->fwd_launches = c->bwd_launches = 0; }
  return DC_OK;
}

}  // extern "C"
