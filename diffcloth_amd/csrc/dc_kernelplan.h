// Host-side plan of WHICH compiled instance of a step kernel runs: the tables of the instances that exist, and the pure functions that choose
// one from the table plan's decisions (dc_tables.h), the values of the development switches and, for the adjoint, the step's arguments. Plain
// C++17 with no HIP header: the host builders pick their paddings from these tables (dc_packets.cpp, dc_tables.cpp, dc_clusterplan.cpp), the
// launcher files instantiate one kernel per table entry (for_first_index below) and launch the entry a choice names, and
// tests/native/kernel_plan_check.cpp checks tables and choices on the CPU. A choice without a compiled instance is an error of the launch
// (hipErrorInvalidValue), never another kernel family.
#pragma once
#include <climits>
#include <cstddef>
#include <type_traits>
#include <utility>
#include "dc_launchplan.h"

namespace dc {

// ---- the instances that exist ----
// Forward, packet kernel (k_pd_step_pk, dc_forward_pk_kernel.h): threads x rows per thread; xl = rows of the iterate held in LDS with the fp32
// direction planes, xl_h16 = with the direction as halves (-1: no such instance); dense = an instance with the explicit-inverse solve (rows <= 3);
// defl = an instance with the deflated solve (512 threads, rows >= 4: dc_forward_pk_defl.hip). The halves instances read the packet matrix by
// byte offsets, by its 10-bit column deltas when the tables kept those (k_pd_step_pk_d10), or values only when the matrix has a column-offset
// template (k_pd_step_pk_tpl). min_n: a shape that is taken only when
// DC_PK_THREADS (or the default) names its thread count, and then from this many rows on; 0 = a shape of the default ladder. Order: the order
// the launcher files instantiate in, which is the order the kernels stand in the code objects.
struct PkShape { int threads, vpt, xl, xl_h16; bool dense, defl; int min_n; };
constexpr PkShape kPkShapes[] = {
    {768, 14, 3, 7, false, false, 768 * 12 + 1},      // (up to 768 x 12 rows a 512-thread shape has no more rows per thread than 768 threads would)
    {512, 1, 0, -1, true, false, 0},  {512, 2, 0, -1, true, false, 0},  {512, 3, 0, -1, true, false, 0},  {512, 4, 0, -1, false, true, 0},
    {512, 6, 0, -1, false, true, 0},  {512, 8, 0, -1, false, true, 0},  {512, 10, 0, -1, false, true, 0}, {512, 12, 0, -1, false, true, 0},
    {512, 16, 2, -1, false, true, 0}, {512, 20, 6, 12, false, true, 0},
};
constexpr int kPkShapeCount = (int) (sizeof(kPkShapes) / sizeof(kPkShapes[0]));
constexpr int kPkDefaultThreads = 512;      // (measured default; DC_PK_THREADS=512 / 768 forces)
// The shape the packet tables of an N-row mesh are padded for, as an index into kPkShapes; -1 = too large for the one-workgroup kernel. The
// smallest shape of the default ladder that holds N rows; with 768 threads wanted, meshes of 9 217 ... 10 240 rows take 768 x 14 (12 waves = 3
// per SIMD at 168 registers instead of 2 per SIMD: the resident PCG and the element windows are latency-bound, a third wave per SIMD hides
// more of it).
inline int pk_shape_for(int N, int want_threads) {
  int narrow = -1;
  for (int i = 0; i < kPkShapeCount && narrow < 0; i++)
    if (kPkShapes[i].min_n == 0 && kPkShapes[i].threads * kPkShapes[i].vpt >= N) narrow = i;
  if (narrow < 0) return -1;
  for (int i = 0; i < kPkShapeCount; i++) {
    const PkShape &s = kPkShapes[i];
    if (s.min_n > 0 && s.threads == (want_threads ? want_threads : kPkDefaultThreads) && N >= s.min_n && N <= s.threads * s.vpt) return i;
  }
  return narrow;
}

// Forward and adjoint, split kernels (k_pd_step_cl, k_adjoint_step_cl): 512 threads; the forward's rows per thread. Every entry has the four
// plain forward instances (detection inlined or not, single- or two-exchange CG) and the two deflated ones (two-exchange CG).
constexpr int kClRows[] = {1, 2, 3, 4, 6, 8, 12};
constexpr int kClRowsCount = (int) (sizeof(kClRows) / sizeof(kClRows[0]));
constexpr int kClThreads = 512;
// rows per thread of a part of R rows; 0 = more rows than the kernel holds in registers
inline int cl_rows_for(int R) {
  for (int v : kClRows) if (v * kClThreads >= R) return v;
  return 0;
}

// Forward, ELL resident kernel (k_pd_step_res, dc_forward_res.hip): (threads, rows per thread) so that threads x rows >= N with as many waves as
// the register budget allows; alt_* = the second thread shape DC_FWD_VARIANT=1 selects (the same shape up to 8 192 vertices).
struct ResShape { int max_n, threads, vpt, alt_threads, alt_vpt; };
constexpr ResShape kResLadder[] = {
    {256, 256, 1, 256, 1},    {512, 256, 2, 256, 2},     {1024, 256, 4, 256, 4},       {1536, 256, 6, 256, 6},        {2048, 512, 4, 512, 4},
    {4096, 512, 8, 512, 8},   {6144, 512, 12, 512, 12},  {8192, 1024, 8, 1024, 8},     {10240, 1024, 10, 512, 20},    {12288, 1024, 12, 512, 24},
};
constexpr int kResCount = (int) (sizeof(kResLadder) / sizeof(kResLadder[0]));

// Forward, global-memory kernel (k_pd_step, dc_forward.hip): any N
struct GlobalShape { int max_n, threads; };
constexpr GlobalShape kGlobalLadder[] = {{1536, 256}, {6144, 512}, {INT_MAX, 1024}};
constexpr int kGlobalCount = (int) (sizeof(kGlobalLadder) / sizeof(kGlobalLadder[0]));

// Adjoint, one workgroup per rollout (k_adjoint_step, dc_adjoint.hip): every thread count has the instance without element windows and the
// windowed ones with and without the block preconditioner; the explicit-inverse (dense) and the coarse-level instances exist for 1024 threads.
// Order: the order dc_adjoint.hip instantiates in.
struct AdjShape { int threads; bool dense, coarse; };
constexpr AdjShape kAdjShapes[] = {{1024, true, false}, {1024, false, true}, {256, false, false}, {512, false, false}, {1024, false, false}};
constexpr int kAdjShapeCount = (int) (sizeof(kAdjShapes) / sizeof(kAdjShapes[0]));
// 16 waves per rollout at every mesh size: the Krylov iteration is a chain of barrier-separated phases with global-memory round trips, and with
// one workgroup per CU (256 rollouts) only the waves of that workgroup can hide them — measured 1.3 - 1.7 x over 256 / 512 threads from N = 579
// to N = 3634 (tools/bench_configs.py), even with idle lanes at N < 1024
constexpr int kAdjDefaultThreads = 1024;

// f(std::integral_constant<size_t, I>{}) for I = 0 ... N - 1 until one returns true: how a launcher walks a table at compile time, with one
// template instance per entry (a left fold: the compiler instantiates the entries, and emits their kernels, in table order)
template <class F, size_t... I>
inline bool for_first_index(F &&f, std::index_sequence<I...>) { return (... || f(std::integral_constant<size_t, I>{})); }
template <size_t N, class F>
inline bool for_first_index(F &&f) { return for_first_index(f, std::make_index_sequence<N>{}); }

// ---- what a choice is made from ----
// values of the development switches that select instances (dc_env.h reads them, once per process)
constexpr int kFwdVariantDefault = -2, kFwdVariantGlobal = -1;
struct KernelSwitches {
  int fwd_variant = kFwdVariantDefault;   // DC_FWD_VARIANT: "global..." = kFwdVariantGlobal, else its integer: 0 / 1 = the ELL resident kernel's thread shapes
  bool pk_h16 = true;                     // DC_PK_H16=0: fp32 direction planes in the packet instances that have halves
  int bwd_threads = 0;                    // DC_BWD_THREADS: 256 / 512 / 1024 = threads of the one-workgroup adjoint
  bool sxcg = true;                       // DC_SXCG=0: the two-exchange CG loop of the split forward kernel
};
// the decisions of the table plan (HostTables::facts)
struct PlanFacts {
  int N = 0;
  bool pk_ok = false, win_ok = false, pk_ofs = false, fwd_defl = false, adj_coarse = false;
  bool pk_tpl = false;                    // the packet matrix went on from byte offsets to the template layout (dc_packets.h)
  int pk_threads = 0, pk_vpt = 0;
  bool defl_space = false;                // a deflation space was built (DevSystem::defl_u)
  bool dense_inv = false;                 // the explicit inverse was built (DevSystem::dense_inv)
  int win_lds_bytes = 0;                  // LDS of the element windows, 0 without them
};

// ---- forward step, one workgroup per rollout ----
enum FwdFamily { kFwdNone = 0, kFwdPacket, kFwdPacketDeflated, kFwdResident, kFwdGlobal };
struct FwdChoice {
  FwdFamily family = kFwdNone;            // kFwdNone: the decisions name no compiled instance
  int threads = 0, vpt = 0, xl = 0;
  bool h16 = false, ofs = false, dense = false;   // packet families: direction as halves, matrix by byte offsets, explicit-inverse solve
  bool tpl = false;                       // kFwdPacket with halves: the matrix is in its template layout, k_pd_step_pk_tpl runs (dc_forward_pk_tpl.hip)
  bool fusable = false;                   // the kernel honours FwdArgs::nsteps (all steps of a rollout in one launch): the packet families
};
// The packet kernel when its tables exist (deflated when the plan says so), else the ELL resident kernel up to its largest shape, else the
// global-memory kernel; DC_FWD_VARIANT forces the second or the third. Decisions that fit no packet instance (offsets for a shape without
// halves, deflation for a shape without a deflated instance, a shape that is not in the table) give kFwdNone.
inline FwdChoice forward_choice(const PlanFacts &f, const KernelSwitches &sw) {
  FwdChoice c;
  if (sw.fwd_variant == kFwdVariantDefault && f.pk_ok) {
    const bool defl = f.defl_space && f.fwd_defl;
    for (const PkShape &s : kPkShapes) {
      if (s.threads != f.pk_threads || s.vpt != f.pk_vpt) continue;
      const bool h16 = sw.pk_h16 && f.win_ok && s.xl_h16 >= 0;      // the halves need the element windows
      if ((defl && !s.defl) || (f.pk_ofs && !h16) || (f.pk_tpl && (defl || !f.pk_ofs))) break;
      c.family = defl ? kFwdPacketDeflated : kFwdPacket;
      c.threads = s.threads; c.vpt = s.vpt; c.xl = h16 ? s.xl_h16 : s.xl;
      c.h16 = h16; c.ofs = f.pk_ofs; c.tpl = f.pk_tpl; c.dense = !defl && s.dense && f.dense_inv;
      c.fusable = true;
      break;
    }
    return c;
  }
  if (sw.fwd_variant != kFwdVariantGlobal)
    for (const ResShape &s : kResLadder)
      if (f.N <= s.max_n) {
        const bool alt = sw.fwd_variant == 1;
        c.family = kFwdResident; c.threads = alt ? s.alt_threads : s.threads; c.vpt = alt ? s.alt_vpt : s.vpt;
        return c;
      }
  for (const GlobalShape &s : kGlobalLadder)
    if (f.N <= s.max_n) { c.family = kFwdGlobal; c.threads = s.threads; break; }
  return c;
}

// ---- adjoint step, one workgroup per rollout; mode / block_pre: BwdArgs ----
struct AdjChoice { int threads = 0; bool win = false, dense = false, blk = false, coarse = false; };
inline AdjChoice adjoint_choice(const PlanFacts &f, int mode, bool block_pre, int bwd_threads) {
  AdjChoice c;
  c.threads = kAdjDefaultThreads;
  for (const AdjShape &s : kAdjShapes) if (s.threads == bwd_threads) c.threads = bwd_threads;
  c.win = f.win_ok;
  const bool wide = c.threads == 1024;
  // small meshes, reference iteration (mode 0): the inner solve with P is one product with the explicit inverse (dc_dense.h)
  c.dense = f.dense_inv && f.win_ok && mode == 0 && wide;
  // the coarse level of the preconditioner (meshes with a deflation space, direct solve, block preconditioner) when its scratch fits the windows' LDS
  c.coarse = !c.dense && f.adj_coarse && f.defl_space && f.win_ok && f.win_lds_bytes / 4 >= kCoarseLdsFloats && block_pre && mode == 1 && wide;
  // the block preconditioner belongs to the direct solve (mode 1); the reference's iteration (mode 0) uses P^-1 as the reference does.
  // No windows => no BLK: the one instance without windows has the diag(P) preconditioner only.
  c.blk = c.win && block_pre && mode == 1;
  return c;
}

// ---- split kernels ----
// adjoint (direct solve only): block preconditioner, coarse level over the deflation space with it
struct ClAdjChoice { bool blk = false, coarse = false; };
inline ClAdjChoice cl_adjoint_choice(const PlanFacts &f, bool block_pre) { return {block_pre, block_pre && f.adj_coarse && f.defl_space}; }
// forward: rows per thread of the split plan (ClusterPlan::pk_vpt; ok = an entry of kClRows), the single-exchange CG (sx) unless DC_SXCG=0
// or the deflated instances run, which keep the two-exchange loop
struct ClFwdChoice { int vpt = 0; bool sx = false, defl = false, ok = false; };
inline ClFwdChoice cl_forward_choice(const PlanFacts &f, int vpt, const KernelSwitches &sw) {
  ClFwdChoice c;
  c.vpt = vpt; c.defl = f.defl_space && f.fwd_defl; c.sx = !c.defl && sw.sxcg;
  for (int v : kClRows) c.ok = c.ok || v == vpt;
  return c;
}

}  // namespace dc
