/* diffcloth_hip.h — C-ABI of the MI355X-native DiffCloth stepper (libdiffcloth_hip.so).
 *
 * Drop-in boundary for the hot path of omegaiota/DiffCloth: the Projective-Dynamics forward step with
 * Signorini–Coulomb dry friction and its adjoint backward step. Each entry point names the reference
 * interface it replaces (paths relative to /root/reference/src/code/simulation/). The C++ host class
 * `Simulation` (diffcloth_amd/csrc/host/) keeps the reference's step()/stepNN()/stepBackward()/
 * stepBackwardNN() signatures and forwards to these functions; INTEGRATION.md shows the binding.
 *
 * Conventions
 *  - plain C, opaque handle, int status (0 = DC_OK); no exceptions cross the boundary;
 *    dc_last_error() returns a message for the last failing call on that context.
 *  - host vectors are float64, xyz-interleaved, length 3N (or 3*Af) PER ROLLOUT, rollouts concatenated:
 *    exactly the reference's VecXd layout (Simulation.h: ForwardInformation::x etc.), batched.
 *  - the device state is fp32, component-planar [B][3][N]; the step computes in fp32 with fp64 where a difference
 *    of nearly equal quantities decides the result: element strains in the forward step, residual / fall-back solve / gradient
 *    sums in the adjoint (dc_params::adjoint_fp32_only).
 *  - a context owns one HIP stream; calls are enqueued in order; calls that return host data synchronise.
 *  - "slot" k of the tape holds the state after k steps; slot 0 is the initial state.
 */
#ifndef DIFFCLOTH_HIP_H
#define DIFFCLOTH_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dc_ctx dc_ctx;

enum { DC_OK = 0, DC_ERR_INVALID = 1, DC_ERR_HIP = 2, DC_ERR_STATE = 3, DC_ERR_TOPOLOGY = 4, DC_ERR_CAPACITY = 5 };

/* Primitive kinds (Primitive.h PrimitiveType; only the analytic isInContact family is on the hot path). */
enum { DC_PRIM_SPHERE = 0, DC_PRIM_CAPSULE = 1, DC_PRIM_PLANE = 2, DC_PRIM_BOWL = 3,
       DC_PRIM_SPHERE_DISCRETIZED = 4   /* Sphere with discretized = true (Primitive.cpp:230-253; the BIG_SPHERE scene, Simulation.cpp:1905-1911):
                                           contact normal = face normal of the sphere's own latitude / longitude mesh; `length` = its
                                           resolution (0 = the reference's 40). At most one per context. */ };

/* One analytic obstacle. A LowerLeg (Primitive.cpp:383-418) is passed as its three children
 * (joint sphere, foot capsule, leg capsule) sharing one `group`; friction uses the group's mu and the
 * first child in contact wins, as LowerLeg::isInContact does.                                          */
typedef struct dc_primitive {
  int kind;            /* DC_PRIM_*                                                              */
  int group;           /* primitive id seen by the caller (index into Simulation::primitives)    */
  double center[3];    /* world position tested against: center_prim (+ child centerInit)        */
  double top_offset[3];/* capsule: globalRotation * (0,length,0)  (Primitive.cpp:582);
                          plane: corner upperLeft relative to the centre (Plane ctor, Primitive.cpp:13-21) */
  double corner2[3];   /* plane: corner upperRight relative to the centre (the rectangle's other two corners are
                          the negatives; Plane::isInContact Primitive.cpp:66-130). Unused otherwise           */
  double radius;       /* sphere, capsule; bowl: the hemisphere shell Bowl::isInContact tests (Primitive.cpp:362-381) */
  double length;       /* capsule length                                                         */
  double mu;           /* Primitive::mu (default for rollouts without a per-rollout override)     */
  int rotates;         /* Sphere::rotates (Primitive.cpp:255-257)                                 */
} dc_primitive;

/* Scene / solver parameters. Mirrors the process-global statics of the reference
 * (Simulation.h:325-338, Simulation.cpp:9-22) and SceneConfiguration / FabricConfiguration.           */
typedef struct dc_params {
  double time_step;                 /* sceneConfig.timeStep                                       */
  double density;                   /* fabric.density                                             */
  double k_stretch, k_bend, k_att;  /* Triangle::k_stiff, TriangleBending::k_stiff, AttachmentSpring::k_stiff */
  double gravity[3];                /* Simulation::gravity                                        */
  double forward_tol;               /* Simulation::forwardConvergenceThreshold                    */
  double backward_tol;              /* Simulation::backwardConvergenceThreshold                   */
  int gravity_enabled, contact_enabled, selfcollision_enabled;
  int gradient_clipping;            /* Simulation::gradientClipping                               */
  double gradient_clipping_threshold;
  int pd_iter_cap;                  /* <0: (-log10(forward_tol))*150 as Simulation.cpp:1182       */
  int adjoint_iter_cap;             /* <=0: 400 as Simulation.cpp:1562                            */
  /* inner block-Jacobi PCG (replaces SimplicialLLT::solve, Simulation.cpp:1267 / :1577) */
  double cg_rel_tol;                /* stop when |r|_{D^-1} <= cg_rel_tol * |r0|_{D^-1}; <=0: 1e-4 */
  int cg_max_iter;                  /* <=0: 500                                                   */
  /* optional fp32-floor guard, OFF by default (<= 0): leave the PD / adjoint loop when the update norm has set no new
   * minimum for this many consecutive iterations, return the best iterate and report converged = 2. The scene tables
   * ask for 1e-9..1e-10, below fp32 resolution for stiff scenes, where the loop otherwise runs to the cap and
   * reverts to the best iterate exactly as the reference does (Simulation.cpp:1357-1367). It is off by default
   * because |x_new - x_now| is NOT monotone under contact mode switching: plateaus of > 100 iterations occur in the
   * reference's own T-shirt run and a short window would stop early there (tests/test_gpu_parity.py, golden rollout). */
  int stall_window;
  /* adjoint solver: 0 = the reference's fixed-point iteration u <- P^-1 (g + dP^T u) (Simulation.cpp:1561-1600)
   * with a direct solve when the cap is hit (:1589-1594); 1 = always the direct solve, i.e. the semantics of
   * Simulation::backwardGradientForceDirectSolver / solveDirect (:1431-1440). On the GPU the direct solve is a
   * block-Jacobi preconditioned BiCGSTAB on (P - dP^T) run to adjoint_rel_tol (relative residual; <=0: 1e-6).
   * 2 = the dense direct solve, the counterpart of solveDirect's SparseLU: per rollout and step K = P - dP^T is assembled as a dense fp64
   * matrix and factored by LU with partial pivoting on the device; u comes from forward / back substitution with the factors, refined
   * against the fp64 residual (at most 3 substitutions) to adjoint_rel_tol; a rollout whose factorisation meets a zero or non-finite pivot
   * takes the fp64 BiCGSTAB fall-back. Meshes of at most 768 vertices (dc_set_params / dc_build fail with DC_ERR_INVALID above);
   * one backward step per launch, one workgroup per rollout. dc_set_solver(force_direct_adjoint = 1) keeps mode 2.
   * 3 = the same solve on K in band storage (opt-in): with the unknowns interleaved (3 i + c, device numbering) K has half-bandwidth
   * kl = ku = min(3N - 1, 3 (bw + extra) + 2), bw = the matrix bandwidth dc_get_layout reports, extra = dc_set_adjoint_band (default 0).
   * LU with partial pivoting in LAPACK band storage (ldab = 2 kl + ku + 1 rounded up to 16) costs at most 2 n kl (kl + ku) flops, n = 3N,
   * against (2/3) n^3 for mode 2, and ldab n doubles. No 768-vertex cap: a mesh is taken when the band of one rollout fits 8 GB and
   * 3N doubles plus the substitution's block (one column of kl multipliers, at least 32 x 32 doubles) fit the workgroup's LDS; dc_set_params (on a built context), dc_build and
   * dc_set_adjoint_band fail with DC_ERR_INVALID and a message naming both numbers otherwise. A rollout whose K has a non-zero outside
   * the band (a self contact between vertices further apart than bw + extra) is flagged and takes the fp64 BiCGSTAB fall-back from
   * u = 0, as a zero pivot does: never silent (fp64_iters > 0), never a wrong answer. dc_set_solver(force_direct_adjoint = 1) keeps mode 3. */
  int adjoint_mode;
  double adjoint_rel_tol;
  /* direct adjoint solve: 1 (default) = block-Jacobi preconditioner from the 3x3 diagonal blocks of K = P - dP^T itself, rebuilt
   * from x_new every backward step (in-plane stiff / normal soft, sticking contacts decoupled); 0 = the forward solve's Jacobi
   * diag(P)^-1. Changes the iteration count only, not what the solve converges to.                                      */
  int adjoint_block_precond;
  /* direct adjoint solve, precision: 0 (default) = mixed — fp32 Krylov solves (CG first, BiCGSTAB once CG stalls; round 6) for corrections of the residual g - K u evaluated
   * in fp64 from fp64 rest-shape tables, until |g - K u| <= adjoint_rel_tol |g| holds in fp64; when the fp32 solve makes no
   * progress (adjoint systems beyond fp32, e.g. a compressed fine garment) a block-Jacobi BiCGSTAB in fp64 on the same operator
   * takes over — the role of the reference's fp64 SparseLU (Simulation.cpp:1431-1440), which always returns a solution.
   * 1 = one fp32 BiCGSTAB solve alone, never CG, for up to 4 x adjoint_iter_cap iterations with no early hand-over (round-2 behaviour:
   * gradients at eps_fp32 * cond(K), 1-3e-4 on stiff / large scenes; systems beyond fp32 end unconverged after that budget;
   * dc_bwd_stats: fp64_iters = residual_verified = 0, last_udiff = the recurrence residual, and with adjoint_mode 1 cg_iters = 0).   */
  int adjoint_fp32_only;
  int max_self_contacts;            /* capacity of the per-rollout self-contact list of one step; <=0: sized from the mesh,
                                       max(2048, N) pairs (at most 16000); overflow is reported, never silent: dc_step_stats */
  /* spectral deflation for ill-conditioned meshes (csrc/dc_deflate.h): < 0 (default) = decided in dc_build by a probe solve (16 eigenvectors of
   * the scaled system matrix when Jacobi-PCG needs more than 80 iterations on a smooth right-hand side: the reference's 7 742-vertex dress
   * needs 337, the hat 171; the cloth / T-shirt / sock / dress-3634 meshes 15 ... 39 and get none), 0 = never, > 0 = always.
   * Forward step (meshes of more than 1536 vertices; smaller ones solve with the explicit inverse): every PCG solve starts with a Galerkin
   * projection onto those vectors, after its recycled first direction. Adjoint (direct solve with the block preconditioner): the vectors are
   * the coarse level of the BiCGSTAB preconditioner. Stopping rules and what the solves converge to are unchanged. dc_get_deflation reports
   * what dc_build decided.                                                                                                            */
  int forward_deflation;
} dc_params;

/* Per-rollout statistics of one forward step (ForwardInformation::converged/convergeIter). */
typedef struct dc_step_stats {
  int converged;         /* 1: tolerance met; 2: stalled at the fp32 floor, best iterate returned; 0: cap hit */
  int pd_iters;
  int cg_iters;          /* total inner PCG iterations over the step */
  int prim_contacts;
  int self_contacts;
  float last_xdiff;      /* |x_new - x_now|_2 / N of the final iteration */
  int self_overflow;     /* 0: the self-contact list is complete (the reference has no limit, Simulation.cpp:281-352, 422-624);
                            bit 0: more pairs than dc_params::max_self_contacts were found and the list was cut (the step's
                            result is NOT the reference's: raise max_self_contacts and repeat the step); bit 1: more layers
                            than the layer table holds (4088). Calls that return these statistics fail with DC_ERR_CAPACITY */
} dc_step_stats;

/* Per-rollout statistics of one backward step (BackwardInformation::converged/backwardIters). */
typedef struct dc_bwd_stats {
  int converged;         /* 1: tolerance met; 2: stalled at the fp32 floor; 0: cap hit (reference falls back to SparseLU) */
  int adjoint_iters;
  int cg_iters;
  int clipped;
  int used_direct;       /* 1 when the direct (Krylov) solve ran; adjoint_iters then counts its iterations too; 2 = the dense direct solve
                            (adjoint_mode 2): refine_cycles = substitutions with the LU factors, adjoint_iters = cg_iters = 0, fp64_iters =
                            iterations of the fall-back, last_udiff = the fp64 residual |g - K u| / |g| (residual_verified = 1); 3 = the banded
                            direct solve (adjoint_mode 3), the other fields as for 2                                                      */
  float last_udiff;      /* mode 0: |u_new - u|_2 / N; direct solve: relative residual |g - K u| / |g| — mixed precision: the TRUE
                            residual evaluated in fp64 (residual_verified = 1), or, when the last fp32 correction solve was accepted
                            without a further fp64 evaluation, an upper bound: its recurrence residual + twice the measured fp32
                            operator error (residual_verified = 0); adjoint_fp32_only: the fp32 recurrence's                 */
  int refine_cycles;     /* direct solve, mixed precision: fp32 solves run (each followed by an fp64 residual evaluation)    */
  int fp64_iters;        /* BiCGSTAB iterations of the fp64 fall-back (0: the fp32 corrections were enough)                 */
  int residual_verified; /* direct solve, mixed precision: 1 = last_udiff is an fp64-evaluated residual, 0 = the bound described there */
  int workgroups;        /* workgroups that ran this rollout's backward step. Smaller than dc_get_cluster's K when the split adjoint kernel
                            does not implement the configuration — adjoint_mode 0 (the reference's fixed-point iteration, Simulation.cpp:
                            1569-1600) runs on ONE workgroup per rollout although the forward steps are split — reported, not silent   */
} dc_bwd_stats;

/* ---- lifetime ------------------------------------------------------------------------------------ */
/* device_id >= 0: HIP device; fails with DC_ERR_HIP when no device is present — there is no CPU compute path.
 * device_id == -1: host-only context for building / inspecting the constraint system (dc_set_*, dc_build,
 * dc_get_counts/system_matrix/vertex_data); every batch or step call on it fails with DC_ERR_STATE.      */
int dc_create(int device_id, dc_ctx **out);
int dc_destroy(dc_ctx *ctx);
const char *dc_last_error(const dc_ctx *ctx);
const char *dc_version(void);

/* ---- system definition: replaces createClothMeshFromModel/…FromConfig (Simulation.cpp:2170-2255,
 *      2611-2757), createBendingConstraints (:2096-2131), updateCollisionRadii (:2407-2431),
 *      updateAreaMatrix/updateMassMatrix (:2894-2966), initializePrefactoredMatrices (:2969-3059).
 *      The caller passes the already oriented / normalised rest positions.                           */
int dc_set_mesh(dc_ctx *ctx, int num_vertices, const double *rest_pos /*3N*/, int num_triangles, const int *tris /*3T*/);
int dc_set_attachments(dc_ctx *ctx, int num_fixed, const int *vertex /*Af*/);   /* SystemMatrix::attachments */
int dc_set_params(dc_ctx *ctx, const dc_params *p);
int dc_set_primitives(dc_ctx *ctx, int count, const dc_primitive *prims);       /* Simulation::primitives */
int dc_build(dc_ctx *ctx);      /* (re)assemble A, P = M + h^2 A^T A and upload; call after any of the setters */
void dc_default_params(dc_params *p);
/* The reference reads its process-global statics at every step (Simulation::forwardConvergenceThreshold,
 * backwardConvergenceThreshold, gradientClipping[Threshold], backwardGradientForceDirectSolver, and the
 * gravity/contact/self-collision switches of setWindAncCollision): these two calls change them between steps
 * without rebuilding the system or invalidating the batch / tape.                                          */
int dc_set_solver(dc_ctx *ctx, double forward_tol, double backward_tol, int gradient_clipping, double clip_threshold,
                  int force_direct_adjoint);
int dc_set_flags(dc_ctx *ctx, int gravity_enabled, int contact_enabled, int selfcollision_enabled);

/* sizes: N, T, E (bending flaps), Af, nnz(P), constraint rows (6T + 3E + 3Af) */
int dc_get_counts(const dc_ctx *ctx, int *out6);
/* host-side tables for inspection / parity tests: scalar P in CSR; per-vertex mass, area, radii */
int dc_get_system_matrix(const dc_ctx *ctx, int *row_ptr /*N+1*/, int *col /*nnz*/, double *val /*nnz*/);
int dc_get_vertex_data(const dc_ctx *ctx, double *mass, double *area, double *radii);

/* ---- batch state ---------------------------------------------------------------------------------- */
/* B independent rollouts sharing the system; tape_steps = how many forward steps can be recorded. */
int dc_alloc_batch(dc_ctx *ctx, int batch, int tape_steps);
/* Simulation::resetSystem / stepNN's state injection (Simulation.cpp:1020-1030): write slot `slot`. */
int dc_set_state(dc_ctx *ctx, int slot, const double *x /*B*3N*/, const double *v /*B*3N*/);
int dc_get_state(dc_ctx *ctx, int slot, double *x, double *v);
/* per-rollout friction coefficient per primitive group: mu[b*num_groups + g]; NULL restores the defaults */
int dc_set_mu(dc_ctx *ctx, const double *mu);
/* uniform external force added to every vertex of rollout b during the NEXT forward steps (wind*windNorm*
 * windFactor of fillForces, Simulation.cpp:96-105): f[b*3+d]; NULL = none                              */
int dc_set_uniform_force(dc_ctx *ctx, const double *f);
/* per-vertex external force added during the NEXT forward steps: f[b*3N + 3i + d] (xyz interleaved like the states). Carries
 * what fillForces adds per vertex beyond gravity and the uniform wind: wind * windNorm * windFactor (.) windFallOff for
 * WIND_SIN_AND_FALLOFF / WIND_FACTOR_PER_STEP and the constant force field (Simulation.cpp:87-105); NULL = none       */
int dc_set_vertex_forces(dc_ctx *ctx, const double *f /*B*3N or NULL*/);
/* a SECOND per-vertex external force, added with factor 1 in every step: the constant force field of fillForces
 * (`if (enableConstantForcefield) f_ext += external_force_field`, Simulation.cpp:91-93) next to a wind with fall-off whose per-step
 * factor travels with dc_set_vertex_forces + dc_set_force_schedule (fv_scale) — the two per-vertex terms of a step have different
 * time factors, and a fused rollout needs both on the device. Same layout as dc_set_vertex_forces; NULL = none                    */
int dc_set_vertex_force_field(dc_ctx *ctx, const double *f /*B*3N or NULL*/);

/* ---- the hot path --------------------------------------------------------------------------------- */
/* Simulation::step()/stepNN() (Simulation.cpp:1020-1428): advance slot -> slot+1 for all rollouts.
 * fixed_pts: rlFixedPointPos per rollout, B*3Af (NULL: keep the previous targets / rest positions).
 * stats (optional, length B) is filled after synchronising; pass NULL to stay asynchronous.            */
int dc_step_forward(dc_ctx *ctx, int slot, const double *fixed_pts, dc_step_stats *stats);
/* ForwardInformation fields of the step that produced `slot` (f, r): B*3N each; NULL to skip. */
int dc_get_record(dc_ctx *ctx, int slot, double *f, double *r);
/* per-vertex primitive contact of that step: group id or -1 (B*N) and contact normal (B*3N) */
int dc_get_contacts(dc_ctx *ctx, int slot, int *prim_group, double *normal);

/* layered self contacts of that step for ONE rollout (ForwardInformation::collisionInfos.second, the output of
 * contactSorting, Simulation.cpp:422-624): pairs (particleId1 < particleId2) in layer order, layer index and normal
 * per contact; at most `cap` entries are written, *count receives the total.                                  */
int dc_get_self_contacts(dc_ctx *ctx, int slot, int rollout, int cap, int *count, int *num_layers, int *pairs /*2*cap*/,
                         int *layer /*cap*/, double *normal /*3*cap*/);

/* A forward record handed in from OUTSIDE. Simulation::stepBackward differentiates the ForwardInformation it is given, whoever made it
 * (Simulation.cpp:1455-1551 reads forwardInfo_new.x / .x_prev / .v_prev / .f / .x_fixedpoints / .collisionInfos; records also come from
 * disk, resetForwardRecordsFromFolder): dc_set_record writes record `slot` of all B rollouts — the tape entries in fp32 AND the values
 * as passed (fp64) for the adjoint's fp64 operator, so that dc_step_backward(slot) solves the adjoint system of exactly this record
 * (teacher-forced parity tests upload the fp64 oracle's record; the forward kernels are not involved). The state the step started from
 * (x_prev, v_prev) is slot - 1 (dc_set_state). The fp64 copy belongs to this one slot and is dropped when a forward step overwrites the
 * slot, when the slot's state or the system is rewritten (dc_set_state*, dc_build), when another record is set, or by dc_alloc_batch; a
 * fused backward sweep over an injected slot runs step by step. Self contacts come in layer order and the contacts of one layer must be
 * vertex-disjoint (they are applied in parallel, as contactSorting builds them: Simulation.cpp:422-624) — DC_ERR_INVALID otherwise.       */
typedef struct dc_record {
  const double *x, *v;          /* B*3N  ForwardInformation::x, ::v — the state after the step                                       */
  const double *f;              /* B*3N  ForwardInformation::f (b~ - C v of the last PD iteration: the contact vectors d derive from it) */
  const double *r;              /* B*3N  ForwardInformation::r, may be NULL (the adjoint does not read it)                           */
  const int *prim;              /* B*N   primitive in contact with the vertex: index into the dc_set_primitives array (LowerLeg children
                                          flattened), -1 = none (PrimitiveCollisionInformation::primitiveId)                          */
  const double *normal;         /* B*3N  contact normal at the vertices in contact (ignored elsewhere)                               */
  const double *x_fixed;        /* B*3Af ForwardInformation::x_fixedpoints of the step; NULL keeps the slot's                        */
  /* layered self contacts (collisionInfos.second, the output of contactSorting): self_count[b] contacts per rollout, concatenated in
   * rollout order; within a rollout in layer order (self_layer non-decreasing, starting at 0)                                       */
  const int *self_count;        /* B, or NULL = no self contacts                                                                     */
  const int *self_pairs;        /* 2 per contact: particleId1 < particleId2                                                          */
  const int *self_layer;        /* 1 per contact: layerId                                                                            */
  const double *self_normal;    /* 3 per contact                                                                                     */
  const double *self_d;         /* 3 per contact: SelfCollisionInformation::d of the last friction evaluation                        */
} dc_record;
int dc_set_record(dc_ctx *ctx, int slot, const dc_record *rec);

/* Simulation::stepBackward()/stepBackwardNN() (Simulation.cpp:1443-1780) through the step that produced
 * `slot` (forwardInfo_new = record `slot`). Inputs B*3N each; dL_dxinit/dL_dvinit may be NULL (zeros).
 * Outputs: dL_dx, dL_dv (B*3N), dL_dxfixed (B*3Af, may be NULL), dL_dmu (B*num_groups, may be NULL).    */
int dc_step_backward(dc_ctx *ctx, int slot, const double *dL_dxnew, const double *dL_dvnew,
                     const double *dL_dxinit, const double *dL_dvinit, int is_start, double *dL_dx,
                     double *dL_dv, double *dL_dxfixed, double *dL_dmu, dc_bwd_stats *stats);

/* Parameter gradients of the LAST backward step through record `slot` (Simulation.cpp:1672-1764), 8 doubles per
 * rollout: [0..2] this step's contribution to dL/dk of {stretch, bending, attachment} (dL_dk_pertype), [3] to
 * dL/ddensity (adddr_dd = false), [4..6] h^2 * sum_i ((I + dr_df)^T u*)_i = the summed dL_dfext_vec from which the
 * caller forms dL_dfext / dL_dwind (multiply by windFactor, cos(...) etc. as :1730-1760), [7] unused.            */
int dc_get_param_gradients(dc_ctx *ctx, int slot, double *out /*B*8*/);
/* dL/df per vertex of the LAST backward step: h^2 ((I + dr_df)^T u*)_i, B*3N xyz interleaved — the vector the reference
 * calls dL_dfext_vec (Simulation.cpp:1700-1760), from which dL_dconstantForceField (sum over the steps), dL_dwindtimestep
 * (dot with (wind * windNorm) (.) windFallOff) and the fall-off variants of dL_dfext / dL_dwind are formed.            */
int dc_get_force_gradient(dc_ctx *ctx, double *dL_df /*B*3N*/);
/* The same vector of EVERY step of a backward sweep: with keep = 1 the backward kernels also store y = (I + dr_df)^T u* of the step through
 * record `slot` in a tape-sized array (allocated on first use, one [B][3][N] fp32 plane per slot), so that a fused sweep
 * (dc_rollout_backward: all steps in one launch) leaves what Simulation::stepBackward forms per step from dL_dfext_vec — dL_dconstantForceField
 * (the sum over the steps), dL_dwindtimestep[step] (its dot with the wind field), the fall-off variants of dL_dfext / dL_dwind
 * (Simulation.cpp:1700-1764) — readable afterwards: dc_get_force_gradients returns h^2 y of the records slot0 .. slot0 + nslots - 1. */
int dc_keep_force_gradients(dc_ctx *ctx, int keep);
int dc_get_force_gradients(dc_ctx *ctx, int slot0, int nslots, double *dL_df /*nslots*B*3N*/);

/* ---- device-pointer boundary: the per-step calls for callers whose tensors already live on this GPU (torch-ROCm: the controller /
 * RL training loops, reference src/python_code/pySim/functional.py:20-102 and hatController.py:78-105, call stepNN + stepBackwardNN
 * once per time step). Same semantics as dc_set_state / dc_get_state / dc_step_forward / dc_step_backward, but every buffer is a
 * DEVICE pointer in the caller's layout — xyz interleaved, B rollouts concatenated, fp32 (is_f32 = 1, torch's default dtype) or
 * fp64 (0) — converted to / from the planar device layout by a kernel: no host copy, no synchronisation; the calls are enqueued on
 * the context's stream and return at once. dc_use_stream makes that stream the caller's (e.g. torch.cuda.current_stream()), so that
 * the calls are ordered with the caller's own kernels; NULL returns to the context's own stream. Statistics of such steps: dc_get_stats. */
int dc_use_stream(dc_ctx *ctx, void *hip_stream);
int dc_set_state_dev(dc_ctx *ctx, int slot, const void *d_x /*B*3N*/, const void *d_v /*B*3N*/, int is_f32);
int dc_get_state_dev(dc_ctx *ctx, int slot, void *d_x /*B*3N or NULL*/, void *d_v /*B*3N or NULL*/, int is_f32);
int dc_step_forward_dev(dc_ctx *ctx, int slot, const void *d_fixed_pts /*B*3Af or NULL*/, int is_f32);
int dc_step_backward_dev(dc_ctx *ctx, int slot, const void *d_dL_dxnew, const void *d_dL_dvnew, const void *d_dL_dxinit /*or NULL*/,
                         const void *d_dL_dvinit /*or NULL*/, int is_start, void *d_dL_dx, void *d_dL_dv, void *d_dL_dxfixed /*B*3Af or NULL*/,
                         void *d_dL_dmu /*B*num_groups or NULL*/, int is_f32);

/* ---- device-resident rollouts (no host copies inside; used by bench.py and batched callers) --------- */
/* nsteps forward steps slot -> slot+nsteps; fixed points held at their current values. Returns when the sweep has finished on the
 * device (its kernel time and the split kernels' error word are read back; a self-contact overflow of a step is reported by
 * dc_get_stats for that slot: DC_ERR_CAPACITY). When the packet
 * kernel is in use all steps of a rollout run inside ONE launch (each rollout advances on its own, self-collision
 * detection inlined per step); results are bitwise those of nsteps dc_step_forward calls.                          */
int dc_rollout_forward(dc_ctx *ctx, int slot, int nsteps);
/* Seed the carried gradient (dL_dx, dL_dv) on the device: g_x = scale_x * (x[slot] - target), g_v = 0
 * (the MATCH-shape loss gradient of Simulation.cpp:3237-3488); target NULL means the rest shape.        */
int dc_seed_gradient(dc_ctx *ctx, int slot, const double *target /*3N or NULL*/, double scale_x);
/* nsteps backward steps from record `slot` down to slot-nsteps+1, carrying (dL_dx, dL_dv) on the device
 * exactly as Simulation::runBackwardTask does (Simulation.cpp:3938-3952), all steps in one launch. dL_dmu accumulates
 * over the steps; the per-step parameter gradients (dc_get_param_gradients) and dL_dx_fixed of every step (dc_get_dxfixed) stay
 * readable per slot. Returns when the sweep has finished on the device.                                              */
int dc_rollout_backward(dc_ctx *ctx, int slot, int nsteps);
int dc_get_gradient(dc_ctx *ctx, double *dL_dx, double *dL_dv, double *dL_dmu /*B*num_groups or NULL*/);
/* Carried gradient of the backward sweep set from the host (the loss gradient w.r.t. the last state, Simulation.cpp:3925-3936);
 * also clears the accumulated dL_dmu. */
int dc_set_gradient(dc_ctx *ctx, const double *dL_dx /*B*3N*/, const double *dL_dv /*B*3N*/);

/* ---- device-resident schedules: what the host loop of Simulation::runBackwardTask (Simulation.cpp:3853-3961) feeds into every
 * step — stepFixPoints targets (:964-1018), fillForces terms (:55-116), the per-frame loss gradients dL_dxinit / dL_dvinit
 * (:3938-3952) — uploaded once per rollout, so that a whole loss + gradient evaluation is dc_rollout_forward + dc_rollout_backward.
 * A schedule entry belongs to a tape slot and stays until it is overwritten, dc_clear_schedules or dc_alloc_batch; the per-step
 * calls honour force / fixed-point entries of their slot as well (explicit fixed_pts of dc_step_forward win). A fused sweep needs
 * each kind of schedule on all of its steps or on none (DC_ERR_INVALID otherwise). */
/* targets of the steps slot0+k -> slot0+k+1, k = 0..nsteps-1: xf[k*B*3Af ...] laid out like dc_step_forward's fixed_pts */
int dc_set_fixed_point_schedule(dc_ctx *ctx, int slot0, int nsteps, const double *xf /*nsteps*B*3Af*/);
/* external forces of those steps: fu = uniform force per rollout (wind * windNorm * windFactor(t)), fv_scale = factor on the
 * per-vertex force of dc_set_vertex_forces (windFactor(t) for a wind with fall-off; pass the factor-free field there). Either may
 * be NULL (= the current dc_set_uniform_force value / factor 1). */
int dc_set_force_schedule(dc_ctx *ctx, int slot0, int nsteps, const double *fu /*nsteps*B*3 or NULL*/, const double *fv_scale /*nsteps*B or NULL*/);
/* loss gradient w.r.t. the state AT slot slot0+k (k = 0..nslots-1): added by dc_rollout_backward when its sweep arrives at that
 * state, i.e. it is the dL_dxinit / dL_dvinit argument of the step through record slot0+k+1. dL_dv may be NULL (zeros).
 * Costs two more tape-sized arrays, allocated on first use. dc_step_backward ignores it (its seeds are its arguments). */
int dc_set_seed_schedule(dc_ctx *ctx, int slot0, int nslots, const double *dL_dx /*nslots*B*3N*/, const double *dL_dv /*or NULL*/);
int dc_clear_schedules(dc_ctx *ctx);
/* ---- movable obstacles: per-rollout, per-step primitive centres. The reference reads Primitive::center at every step (isInContactWithObstacle,
 * Simulation.cpp:153-191) and exposes it read-write (python_interface.cpp:285): a caller moves an obstacle between steps by writing it.
 * ONE rule: an OFFSET d[b][g][3] per rollout b and primitive group g (the compacted group index of dc_set_mu, G = num_groups); every flattened
 * primitive p of group g is tested at
 *     centre_p = fp32( (double) dc_primitive.center_p + d[b][g] )          (the sum in fp64, rounded once)
 * so a context built at the moved centre and a context given the offset see the same fp32 centre, bit for bit. The children of a LowerLeg share
 * a group and move together (center_prim + child->centerInit in the reference). Nothing else of the primitive changes: radius, plane corners and
 * capsule axis (relative to the centre), mu, rotates, the discretised sphere's mesh (relative to the centre). An offset alone leaves the obstacle
 * static in the reference's sense (v_out has no translation term): a caller who MOVES an obstacle also gives its velocity, below. The adjoint holds
 * the contact normal of the record constant, as the reference's does: there is no gradient w.r.t. the centre.
 * dc_set_primitive_offsets: offsets of the NEXT forward steps, like dc_set_uniform_force (d = B*G*3; NULL restores the built centres).
 * dc_set_primitive_offset_schedule: the step that advances slot slot0 + s to slot0 + s + 1 uses d[s] (nsteps*B*G*3); the rules of
 * dc_set_force_schedule hold — an entry stays until it is overwritten, dc_clear_schedules or dc_alloc_batch, the per-step calls honour it, and a
 * fused sweep needs it on all of its steps or on none (DC_ERR_INVALID otherwise).
 * The _dev forms take DEVICE pointers (fp32 or fp64) on the context's stream, converted by one launch for all slots, no synchronisation.
 * dc_get_primitive_centers: the absolute centres of the P flattened primitives (dc_set_primitives order) that the step which produced `slot`
 * used, B*P*3, the fp32 values widened — on the per-step path as in a sweep: a slot says where its obstacle was. Synchronises.
 * dc_alloc_batch, dc_set_primitives and dc_build drop offsets and schedule (B or G changed). A host-only context refuses all of these with
 * DC_ERR_STATE; without primitives (G == 0) the setters fail with DC_ERR_INVALID.                                                              */
int dc_set_primitive_offsets(dc_ctx *ctx, const double *d /*B*G*3 or NULL*/);
int dc_set_primitive_offset_schedule(dc_ctx *ctx, int slot0, int nsteps, const double *d /*nsteps*B*G*3*/);
int dc_set_primitive_offsets_dev(dc_ctx *ctx, const void *d_d /*B*G*3 or NULL*/, int is_f32);
int dc_set_primitive_offset_schedule_dev(dc_ctx *ctx, int slot0, int nsteps, const void *d_d /*nsteps*B*G*3*/, int is_f32);
int dc_get_primitive_centers(dc_ctx *ctx, int slot, double *c /*B*P*3*/);
/* ---- moving obstacles: a velocity per rollout, primitive group and step. The reference carries the quantity (v_out = this->velocity in every
 * isInContact of Primitive.cpp) and never sets it; without it a sphere moved through the cloth by a centre schedule brakes the cloth towards
 * rest in the world frame. ONE rule, next to the centre rule above: rollout b, group g and step have w[b][g][3]; the device stores fp32(w), the
 * fp64 operator of the adjoint uses (double) fp32(w). It enters the step in two places.
 *  1. Friction, forward and adjoint: for a vertex in contact with a flattened primitive p of group g
 *         d = (f - v_rot(p, n) m) - w[b][g] m            (v_rot: the rotating sphere's spin term; evaluated in this order, so w = +0 changes no bit)
 *     in every forward kernel family, in the fp32 adjoint operators and in the fp64 operator and dL_dmu (recorded and dc_set_record branches).
 *  2. Detection look-ahead: the sample points of group g become pos + (vel - w[b][g]) h k / 2, k = 0, 1, 2, tested against the step's centre:
 *     the centre row is the obstacle's position at the START of the step and the obstacle moves by w h during it. (The reference's text uses the
 *     absolute vel; the two agree wherever the reference is exercised, w = 0.) With both, the step is Galilean invariant: every obstacle moving at
 *     w and the cloth at (x, v + w) — attachment targets moved by w h — is the static step at (x, v), shifted by (w h, w).
 * A caller who moves an obstacle along c(t) passes offsets[s] = c(t_s) - c_built and velocities[s] = (c(t_{s+1}) - c(t_s)) / h.
 * Storage: a table of rows {w[3], omega[3]} [slot][B][G][6], per GROUP, shared with the spin entries below and allocated (all zero) by the first
 * setter of either kind after dc_alloc_batch; every entry addresses its half, so the layouts here stay B*G*3. Until then the kernels evaluate the
 * static law (a null pointer: one uniform branch in the forward kernels, and the adjoint step kernels of such a context are the instances compiled
 * without the table). Row `slot` is what the step that PRODUCED `slot` used and what the backward step through record
 * `slot` reads: a record handed in with dc_set_record at `slot` gets its velocity from a one-step schedule at slot - 1.
 * dc_set_primitive_velocities: velocities of the NEXT forward steps without a schedule entry (w = B*G*3; NULL = zeros).
 * dc_set_primitive_velocity_schedule: the step slot0 + s -> slot0 + s + 1 uses w[s]. The rules of the offset entries hold throughout: an entry
 * stays until it is overwritten, dc_clear_schedules or dc_alloc_batch; the per-step calls honour it; a fused sweep needs it on all of its steps
 * or on none (DC_ERR_INVALID); dc_alloc_batch, dc_set_primitives and dc_build drop everything; a host-only context answers DC_ERR_STATE;
 * G == 0 gives DC_ERR_INVALID. The _dev forms take DEVICE pointers (fp32 or fp64) on the context's stream: one launch for all slots, no
 * synchronisation.
 * dc_get_primitive_velocities: the fp32 values, widened, that the step which produced `slot` used (zeros when none was ever set). Synchronises.
 * The gradient: a velocity, unlike a centre, enters the adjoint smoothly (r depends on w only through d), so under the adjoint's own rules — normals
 * constant, contact set not differentiated — every backward step leaves, in the convention of dL_dmu,
 *         dL/dw[b][g] = -h * sum over the vertices i in contact with group g of  m_i (dr_i/dd_i)^T u_i
 * summed in fp64 without atomics (bit-reproducible, one workgroup or split), written per record slot and OVERWRITTEN by the next backward step
 * through that slot. dL_ddensity keeps the reference's omission of the dr/dd term (adddr_dd = false): a moving obstacle's step carries that
 * omission exactly as the rotating sphere's does. The getters return slots slot0 .. slot0 + nslots - 1 (nslots*B*G*3) and fail with DC_ERR_STATE
 * before any velocity setter; the host form synchronises, the _dev form is enqueued. There is still no gradient w.r.t. the centre.            */
int dc_set_primitive_velocities(dc_ctx *ctx, const double *w /*B*G*3 or NULL = zeros*/);
int dc_set_primitive_velocity_schedule(dc_ctx *ctx, int slot0, int nsteps, const double *w /*nsteps*B*G*3*/);
int dc_set_primitive_velocities_dev(dc_ctx *ctx, const void *d_w /*B*G*3 or NULL = zeros*/, int is_f32);
int dc_set_primitive_velocity_schedule_dev(dc_ctx *ctx, int slot0, int nsteps, const void *d_w /*nsteps*B*G*3*/, int is_f32);
int dc_get_primitive_velocities(dc_ctx *ctx, int slot, double *w /*B*G*3*/);
int dc_get_primitive_velocity_gradients(dc_ctx *ctx, int slot0, int nslots, double *dL_dw /*nslots*B*G*3*/);
int dc_get_primitive_velocity_gradients_dev(dc_ctx *ctx, int slot0, int nslots, void *d_dL_dw /*nslots*B*G*3*/, int is_f32);
/* ---- spinning obstacles: an angular velocity per rollout, primitive group and step. The reference's only spin is its hard-wired `rotates`
 * sphere (fixed axis, fixed speed, no gradient). ONE rule, next to the centre and velocity rules above: rollout b, group g and step have
 * omega[b][g][3] in rad/s; the device stores fp32(omega), the fp64 operator of the adjoint uses (double) fp32(omega). It enters the step in ONE
 * place, the v_out of the friction law: for a vertex in contact with a flattened primitive p of group g whose kind is DC_PRIM_SPHERE
 *         v_spin = radius_p (omega[b][g] x n)         (radius_p: the BUILT radius; n: the contact normal the law already uses)
 *         d = ((f - v_rot(p, n) m) - w[b][g] m) - v_spin m
 * evaluated in this order and skipped, by a test that is uniform per group, when all three components of the stored omega are +-0: omega = 0 and
 * "never set" are the same step bit for bit, with and without velocities. Every other kind has NO spin term — plane, bowl, capsule, the
 * discretised sphere (its normal is a face normal) and the capsule child of a LowerLeg; the sphere children of a LowerLeg do contribute (about
 * their own centres). The reference's rotates sphere is the special case omega = (0, 8 / radius, 0); `rotates` stays as it is and the two add.
 * Detection is unchanged: a sphere spinning about its centre occupies the same space. The term applies in every forward kernel family, in the
 * fp32 adjoint operators, in the fp64 operator, the fall-back and dL_dmu (recorded and dc_set_record branches). A caller who also changes the
 * radius through a shape schedule scales omega by r_step / r_built themselves: the adjoint does not read the shape.
 * The entries mirror the velocity entries and every rule there holds: row `slot` is what the step that PRODUCED `slot` used and what the backward
 * step through record `slot` reads (a dc_set_record record gets its spin from a one-step schedule at slot - 1); an entry stays until it is
 * overwritten, dc_clear_schedules or dc_alloc_batch; the per-step calls honour the schedule; a fused sweep needs it on all of its steps or on
 * none (DC_ERR_INVALID; spin entries and velocity entries are tracked separately); dc_alloc_batch, dc_set_primitives and dc_build drop
 * everything; a host-only context answers DC_ERR_STATE; G == 0 gives DC_ERR_INVALID. The host setters refuse (DC_ERR_INVALID) a value
 * that is not finite and a non-zero omega for a group that holds no DC_PRIM_SPHERE. The _dev forms take DEVICE pointers (fp32 or fp64) on the context's
 * stream — one launch for all slots, no synchronisation — and cannot look: there the term is simply zero for such a group.
 * The gradient, under the adjoint's own rules (normals constant, contact set not differentiated), with g_i = (dr_i/dd_i)^T u_i:
 *         dL/domega[b][g] = -h * sum over the vertices i in contact with a DC_PRIM_SPHERE p of group g of  m_i radius_p (n_i x g_i)
 * summed in fp64 without atomics (bit-reproducible, one workgroup or split), written per record slot and OVERWRITTEN by the next backward step
 * through that slot, as dL/dw is. dL_ddensity keeps the reference's omission (adddr_dd = false). The gradient getters fail with DC_ERR_STATE
 * before any spin setter.                                                                                                                    */
int dc_set_primitive_spins(dc_ctx *ctx, const double *omega /*B*G*3 or NULL = zeros*/);
int dc_set_primitive_spin_schedule(dc_ctx *ctx, int slot0, int nsteps, const double *omega /*nsteps*B*G*3*/);
int dc_set_primitive_spins_dev(dc_ctx *ctx, const void *d_omega /*B*G*3 or NULL = zeros*/, int is_f32);
int dc_set_primitive_spin_schedule_dev(dc_ctx *ctx, int slot0, int nsteps, const void *d_omega /*nsteps*B*G*3*/, int is_f32);
int dc_get_primitive_spins(dc_ctx *ctx, int slot, double *omega /*B*G*3*/);
int dc_get_primitive_spin_gradients(dc_ctx *ctx, int slot0, int nslots, double *dL_domega /*nslots*B*G*3*/);
int dc_get_primitive_spin_gradients_dev(dc_ctx *ctx, int slot0, int nslots, void *d_dL_domega /*nslots*B*G*3*/, int is_f32);
/* ---- obstacle shapes per rollout and step: radius, capsule axis and length, the two corners of a finite plane. ONE rule, next to the two above:
 * a SHAPE ROW of 8 numbers per rollout b and FLATTENED primitive p (dc_set_primitives order, P <= 8; per primitive, not per group: the children
 * of a LowerLeg each have their own), the dc_primitive fields of the same names,
 *         s[b][p] = {top_offset[3], corner2[3], radius, length}
 * and the device stores fp32(value), each value rounded once — what dc_build does when it fills its primitive table (one conversion,
 * csrc/dc_primshape.h, called by both). The kernels do no rotation arithmetic: they read the eight numbers of the step's row in place of the
 * built ones, so a context GIVEN a shape and a context BUILT with that shape compute the same step bit for bit. A caller who tilts a plane or
 * swings a capsule about its centre rotates top_offset and corner2 and passes the result. kind, group, mu, rotates and the centre stay what they
 * are (the centre has its own entries above; a capsule's centre is its lower end, so swinging it about its middle needs both). The bowl's "below
 * the centre" test stays world-up. For a DC_PRIM_SPHERE_DISCRETIZED the kernels do NOT read the row — its face table is built for one radius —
 * and the host setters refuse (DC_ERR_INVALID) a row for it that differs from the built one after rounding.
 * A shape schedule alone leaves the surface STATIC in the friction law, as an offset alone does: the surface velocity of a rotating or growing
 * obstacle is not modelled. A caller who wants the translation part passes velocities (dc_set_primitive_velocities); the spin of a sphere is
 * given through the spin entries (dc_set_primitive_spins). There is no gradient with
 * respect to a shape: the adjoint holds the record's normals and contact set constant and does not read the shape at all.
 * Storage: a table [slot][B][P][8] in fp32 and a current set [B][P][8], allocated by the first of these setters after dc_alloc_batch and filled
 * with the built shapes; until then the kernels read the built primitive table (a null pointer: one uniform branch). Row `slot` is what the step
 * that PRODUCED `slot` used.
 * dc_set_primitive_shapes: shapes of the NEXT forward steps without a schedule entry (s = B*P*8; NULL = the built shapes).
 * dc_set_primitive_shape_schedule: the step slot0 + k -> slot0 + k + 1 uses s[k]. The rules of the offset and velocity entries hold throughout:
 * an entry stays until it is overwritten, dc_clear_schedules or dc_alloc_batch; the per-step calls honour it; a fused sweep needs it on all of
 * its steps or on none (DC_ERR_INVALID); dc_alloc_batch, dc_set_primitives and dc_build drop everything; a host-only context answers
 * DC_ERR_STATE; P == 0 gives DC_ERR_INVALID. The host forms refuse non-finite values (DC_ERR_INVALID). The _dev forms take DEVICE pointers (fp32
 * or fp64) on the context's stream — one launch for all slots, no synchronisation — and so cannot look at the values: a degenerate shape (a
 * zero-length capsule axis, collinear plane corners, a non-finite number, another radius for a discretised sphere's unread row) gives what a
 * context built with it would give.
 * dc_get_primitive_shapes: the fp32 rows, widened, that the step which produced `slot` used (B*P*8; the built shapes when none was ever set).
 * Synchronises.                                                                                                                             */
int dc_set_primitive_shapes(dc_ctx *ctx, const double *s /*B*P*8 or NULL = the built shapes*/);
int dc_set_primitive_shape_schedule(dc_ctx *ctx, int slot0, int nsteps, const double *s /*nsteps*B*P*8*/);
int dc_set_primitive_shapes_dev(dc_ctx *ctx, const void *d_s /*B*P*8 or NULL*/, int is_f32);
int dc_set_primitive_shape_schedule_dev(dc_ctx *ctx, int slot0, int nsteps, const void *d_s /*nsteps*B*P*8*/, int is_f32);
int dc_get_primitive_shapes(dc_ctx *ctx, int slot, double *s /*B*P*8*/);
/* states of nslots consecutive slots in one call: x[k*B*3N ...], v likewise (either may be NULL) */
int dc_get_states(dc_ctx *ctx, int slot0, int nslots, double *x, double *v);
/* dL_dxfixed of the steps through records slot0 .. slot0+nslots-1 of the last backward sweep / step (B*3Af each) */
int dc_get_dxfixed(dc_ctx *ctx, int slot0, int nslots, double *dL_dxfixed /*nslots*B*3Af*/);
/* ---- device-pointer boundary of whole sweeps: a loss + gradient evaluation over an episode for callers whose tensors live on this GPU
 * (diffcloth_amd/functional.py: sim_rollout — trajectory optimisation over clip targets, identification of mu or wind, any loss over all
 * frames: the host loop of Simulation::runBackwardTask, Simulation.cpp:3853-3961, with nothing crossing PCIe). The conventions of the
 * per-step dc_*_dev calls hold: every buffer is a DEVICE pointer in the caller's layout — xyz interleaved, rollouts concatenated, slots
 * concatenated, fp32 (is_f32 = 1) or fp64 (0), any element alignment — all slots of an array are converted by ONE kernel, the call is
 * enqueued on the context's stream (dc_use_stream) and returns at once: no host copy, no synchronisation. Slot ranges and states are
 * checked as in the host versions; a host-only context fails with DC_ERR_STATE.                                                       */
/* dc_rollout_forward / dc_rollout_backward without the wait: the same checks and the same launches, enqueued only. They add NOTHING to
 * dc_kernel_times (no event is read), and what a sweep reports after it has run — a timed-out exchange of the split kernels, a
 * self-contact overflow — surfaces at the next dc_sync / dc_get_stats, as for the per-step dc_*_dev calls.                            */
int dc_rollout_forward_async(dc_ctx *ctx, int slot, int nsteps);
int dc_rollout_backward_async(dc_ctx *ctx, int slot, int nsteps);
/* dc_set_fixed_point_schedule / dc_set_force_schedule (either force pointer may be NULL, as there) from device buffers */
int dc_set_fixed_point_schedule_dev(dc_ctx *ctx, int slot0, int nsteps, const void *d_xf /*nsteps*B*3Af*/, int is_f32);
int dc_set_force_schedule_dev(dc_ctx *ctx, int slot0, int nsteps, const void *d_fu /*nsteps*B*3 or NULL*/, const void *d_fv_scale /*nsteps*B or NULL*/, int is_f32);
/* dc_set_seed_schedule from device buffers. A NULL d_dL_dx or d_dL_dv means zeros for those slots: a loss that does not touch some states
 * still gives the complete schedule a fused sweep asks for.                                                                          */
int dc_set_seed_schedule_dev(dc_ctx *ctx, int slot0, int nslots, const void *d_dL_dx /*nslots*B*3N or NULL*/, const void *d_dL_dv /*or NULL*/, int is_f32);
/* dc_set_gradient (clears the accumulated dL_dmu as well) and dc_get_gradient (any pointer may be NULL) */
int dc_set_gradient_dev(dc_ctx *ctx, const void *d_dL_dx /*B*3N*/, const void *d_dL_dv /*B*3N*/, int is_f32);
int dc_get_gradient_dev(dc_ctx *ctx, void *d_dL_dx /*B*3N or NULL*/, void *d_dL_dv /*B*3N or NULL*/, void *d_dL_dmu /*B*num_groups or NULL*/, int is_f32);
/* dc_get_states (either pointer may be NULL) and dc_get_dxfixed */
int dc_get_states_dev(dc_ctx *ctx, int slot0, int nslots, void *d_x /*nslots*B*3N or NULL*/, void *d_v /*nslots*B*3N or NULL*/, int is_f32);
int dc_get_dxfixed_dev(dc_ctx *ctx, int slot0, int nslots, void *d_dL_dxfixed /*nslots*B*3Af*/, int is_f32);
/* Gradients w.r.t. the force schedule of the steps through records slot0 .. slot0 + nslots - 1 of the last backward sweep, reduced on the
 * device; replaces reading dc_get_param_gradients per slot and dc_get_force_gradients (nslots*B*3N doubles) back to the host to form
 * dL_dwindtimestep / dL_dconstantForceField there (Simulation.cpp:1700-1764). Any of the three may be NULL.
 *   d_dL_dfu[k][b][0..2]   = elements 4..6 of that step's parameter gradients (h^2 sum_i y_i): gradient w.r.t. the step's uniform force
 *   d_dL_dfv_scale[k][b]   = h^2 sum_{d,i} y[slot0+k][b][d][i] fv[b][d][i]: w.r.t. the step's factor on the dc_set_vertex_forces field
 *   d_dL_dfv[b][3 i + d]   = h^2 sum_k w[k][b] y[slot0+k][b][d][i], w = the fv_scale schedule of those steps or 1 where none is set:
 *                            w.r.t. the factor-free field; with w = 1 the reference's dL_dconstantForceField
 * The last two read the kept y tape: DC_ERR_STATE without dc_keep_force_gradients(1) before the sweep, as dc_get_force_gradients.
 * Sums are accumulated in fp64 in a fixed order without atomics and rounded once: bit-reproducible from run to run.                  */
int dc_get_force_schedule_gradients_dev(dc_ctx *ctx, int slot0, int nslots, void *d_dL_dfu /*nslots*B*3 or NULL*/,
                                        void *d_dL_dfv_scale /*nslots*B or NULL*/, void *d_dL_dfv /*B*3N or NULL*/, int is_f32);
/* Contact read-out: what the obstacles feel. For the records slot0 .. slot0 + nslots - 1 (slot0 >= 1) ONE kernel launch on the context's stream
 * re-forms, per vertex in primitive contact, the friction law's argument exactly as the step did — d = f - m (v_rot + w + v_spin), n and f from the
 * fp32 record `slot`, the motion row {w, omega} of `slot` (the step that produced it), mu = the context's CURRENT mu[b][group], as the backward
 * step reads it — and reports
 *   state[k][b][i]            0 = vertex i not in primitive contact, 1 = take-off, 2 = stick, 3 = slide (CollisionType + 1 of the reference), by the
 *                             comparisons of the friction law itself: sd = d.n >= 0 -> take-off, else |dT| <= mu |sd| -> stick, else slide
 *   normal_impulse[k][b][i]   jn = r_p . n >= 0, r_p = r(d) the PRIMITIVE part of the step's r (the stored r of dc_get_record also holds what
 *                             the self-contact layers added afterwards); 0 where state is 0 or 1
 *   wrench[k][b][g][0..9]     per primitive group g: J[3] = -sum r_p, the momentum handed to the obstacle during the step (the mean force
 *                             is J / time_step); tau[3] = -sum (x_i - c_g) x r_p, x_i the state of `slot`, c_g the centre of the group's FIRST
 *                             flattened primitive in that step (dc_get_primitive_centers: an offset schedule moves the reference point with
 *                             the obstacle); sum jn; the numbers of take-off, stick and slide contacts. A group without contacts: zeros.
 * Per-vertex outputs are in the caller's vertex numbering. Sums run in fp64 in a fixed order without atomics and are rounded once:
 * bit-reproducible. Each output may be NULL and is then not computed; all three NULL is DC_ERR_INVALID, as are slot0 < 1, nslots < 1, a
 * range past the tape, and a wrench pointer on a context with no primitive group. A record handed in with dc_set_record is read like any
 * other (its fp32 values). The outputs themselves carry no derivative; dc_set_contact_readout_gradients takes a loss's gradient with respect to them.
 * The host form copies back through device buffers of its own and synchronises. The _dev form only enqueues: d_state is int32, the other two
 * fp32 (is_f32 = 1) or fp64; nothing crosses PCIe.                                                                                   */
int dc_get_contact_readout(dc_ctx *ctx, int slot0, int nslots, int *state /*nslots*B*N or NULL*/,
                           double *normal_impulse /*nslots*B*N or NULL*/, double *wrench /*nslots*B*num_groups*10 or NULL*/);
int dc_get_contact_readout_dev(dc_ctx *ctx, int slot0, int nslots, void *d_state /*int32, nslots*B*N or NULL*/, void *d_normal_impulse /*nslots*B*N or NULL*/,
                               void *d_wrench /*nslots*B*num_groups*10 or NULL*/, int is_f32);
/* Gradients of a loss on the contact read-out. dL_djn[k][b][i] and dL_dwrench[k][b][g][0..9] are the derivatives of a loss with respect to
 * normal_impulse and wrench of the records slot0 .. slot0 + nslots - 1 as dc_get_contact_readout reports them (vertex numbering: the caller's;
 * entries 7..9 of a wrench row, the counts, are ignored). They stay set, per slot, until they are overwritten or cleared, and every backward step
 * that passes through such a record — dc_rollout_backward[_async] and dc_step_backward[_dev]; fused and unfused sweeps, records handed in with
 * dc_set_record, adjoint_mode 0..3, split launches — adds the read-out's part to everything it leaves: dL_dx / dL_dv, dL_dmu, dL_dxfixed, the
 * parameter gradients (dc_get_param_gradients), the force gradients (dc_get_force_gradient[s], dc_get_force_schedule_gradients_dev) and
 * {dL/dw, dL/domega}. THE RULE, for a vertex i in contact with a primitive of group g in the step that produced record s, with J^, tau^, S^ the
 * weights of J, tau and sum jn of group g and jn^_i that of the vertex's impulse:
 *     phi_i = -J^ - tau^ x (x_i - c_g) + (jn^_i + S^) n_i        q_i = (dr_p,i/dd_i)^T phi_i  (take-off: 0, stick: -phi_i; 0 at every other vertex)
 * c_g and n_i are held constant, as everywhere in the adjoint; the friction case is the one the read-out reports (current mu, the record's motion
 * row) — with ONE exception: for a record handed in with dc_set_record the case is decided in fp64 on the handed-in values, as the adjoint's
 * fp64 operator decides it for such a record, so that the seeds and the operator they enter differentiate the same law; the read-out reads that
 * record's fp32 values, and within fp32 rounding of a boundary of the friction law (1e-6 |d|) the two can differ. r_p depends on f alone, before the self-contact layers, so the backward step through record s is the plain step with
 *   1. dL/dx at slot s      += -(1/h) h^2 (A - dp/dx)^T A q - r_p,i x tau^    (the adjoint's fp64 element operator at the same x_new, without contact
 *                                                                               part and mass term; the direct dependence of tau on x_i)
 *   2. dL/dv at slot s - 1  += m_i q_i
 *   3. y~ = y + q / h wherever y = (I + dr_df)^T u is read: the force gradients, dL_dxfixed, the dL/dk sums, the w = y - u term of dL_ddensity
 *      (adddr_dd = false as before)
 *   4. u_i + phi_i / h wherever u_i multiplies a primitive-contact derivative: dL_dmu[g] += sum (dr_p,i/dmu) . phi_i, dL/dw[g] += -sum m_i q_i,
 *      dL/domega[g] += -sum m_i radius_p (n_i x q_i) for a DC_PRIM_SPHERE
 * Items 1 and 2 are added to the loss gradients the sweep already takes, in rows of the engine's own that start as the caller's entries (the seed
 * schedule, or dL_dxinit / dL_dvinit of a per-step call, or zeros): the caller's schedule is never modified, and gradient clipping, where
 * enabled, acts on the total. WHICH CALL ADDS ITEM 1: the gradient a backward call leaves is that of the state it ARRIVES at, slot - nsteps, and
 * holds item 1 of the record of that state when it carries weights (added to that state's seed row, like those of the states above it). A call
 * that starts where the previous backward call on the context arrived — a chain of dc_step_backward calls handing dL_dx on as dL_dxnew, or of
 * sweeps carrying the gradient on the device — therefore finds item 1 of its top record in what it is given; every other call adds it to the
 * carried gradient itself. A chain is broken, and the next call adds its top record's part, by dc_set_gradient[_dev], dc_seed_gradient, any
 * forward step, this setter, dc_clear_schedules and dc_alloc_batch; a caller who passes an UNRELATED dL_dxnew to dc_step_backward for exactly
 * the record the previous call arrived at calls this setter (or dc_set_gradient) first. With this rule a fused sweep and the chain of per-step
 * calls over the same tape give the same dL_dx, dL_dv, parameter rows and force gradients bit for bit. Items 3 and 4 are added after the steps to what
 * they left. All of it is fp64 arithmetic on the fp32 record with sums in a fixed order, no atomics, rounded once: the same sweep twice gives the
 * same bits. All-zero weights, weights never set and weights cleared give the same gradients, and a sweep none of whose records carries weights
 * enqueues no additional kernel. There is no gradient through the contact set, the normals, the centres, the shapes or the counts.
 * One pointer NULL: zeros for those slots; both NULL (slot0, nslots ignored) clears all weights, as dc_clear_schedules and dc_alloc_batch do.
 * DC_ERR_INVALID: slot0 < 1, nslots < 1, a range past the tape, wrench weights on a context with no primitive group; a host-only context answers
 * DC_ERR_STATE. Costs two tape-sized fp32 arrays and the weight tables, allocated by the first call after dc_alloc_batch.
 * The host form synchronises; the _dev form takes DEVICE pointers (fp32 or fp64, any element alignment) and only enqueues.                    */
int dc_set_contact_readout_gradients(dc_ctx *ctx, int slot0, int nslots, const double *dL_djn /*nslots*B*N or NULL*/,
                                     const double *dL_dwrench /*nslots*B*num_groups*10 or NULL*/);
int dc_set_contact_readout_gradients_dev(dc_ctx *ctx, int slot0, int nslots, const void *d_dL_djn /*nslots*B*N or NULL*/,
                                         const void *d_dL_dwrench /*nslots*B*num_groups*10 or NULL*/, int is_f32);
/* Self-contact read-out: what the cloth's sheets press on each other with. For the records slot0 .. slot0 + nslots - 1 (slot0 >= 1) the layered
 * cloth-cloth friction of the step (Simulation.cpp:655-678) is re-formed on the device from the fp32 tape values; nothing is computed that the
 * step did not compute. THE RULE, for record s of rollout b:
 *   1. g_i = f_i + r_p,i at every vertex of the record's self-contact working set: f from the record, r_p,i the primitive part exactly as
 *      dc_get_contact_readout re-forms it (prim_d with the motion row of s, the friction law with the context's CURRENT mu[b][group]), 0 where
 *      the vertex is in no primitive contact.
 *   2. The layers are walked in record order, the pairs of a layer in any order (they are vertex-disjoint: dc_record's contract). For pair
 *      k = (A, B) with normal n_k:   d_k = g_A / m_A - g_B / m_B,   r_k = r(n_k, d_k, 0.1) / (1/m_A + 1/m_B)  (the reduced mass
 *      m_A m_B / (m_A + m_B), formed as the step forms it),   state_k = the friction law's case on d_k,   then g_A += r_k, g_B -= r_k.
 *      The device functions and the fp32 expressions are those of the step's layered pass.
 *   3. r_self,i = sum of +-r_k over the pairs that contain i.
 * The record's stored d per pair and its stored r are neither read nor written; a record handed in with dc_set_record is read like any other,
 * through its fp32 values. Outputs, each optional (NULL = not computed):
 *   pairs[k][b][c][0..3]          int32 {id1, id2, layer, state} of contact c, in the order of dc_get_self_contacts and in the caller's vertex
 *                                 numbering; state 1 = take-off, 2 = stick, 3 = slide; entries c >= count hold {-1, -1, -1, 0}. `cap` = entries
 *                                 per rollout; contacts beyond cap are not written but still enter the sums.
 *   impulse[k][b][c][0..3]        {r_k (x, y, z), jn_k = r_k . n_k >= 0}: r_k is the impulse on id1, id2 receives -r_k; zeros beyond count
 *   vertex_impulse[k][b][i][0..2] r_self,i in the caller's numbering, 0 at every other vertex (host form: nslots*B*3N doubles, xyz-interleaved)
 *   totals[k][b][0..7]            {contacts evaluated, layers, distinct vertices, sum jn, sum |r_k - jn_k n_k|, take-off, stick, slide}
 * All sums are fp64, run in a fixed order without atomics and are rounded once: bit-reproducible. A context without self-collision and a
 * record without self contacts answer zeros (-1 ids). DC_ERR_INVALID: slot0 < 1, nslots < 1, a range past the tape, all four outputs NULL,
 * cap < 1 while pairs or impulse is asked for; a host-only or unbuilt context answers DC_ERR_STATE.
 * There is NO GRADIENT: the outputs carry no derivative and no setter takes a loss's gradient with respect to them (a later change).
 * The host form stages through device buffers of its own and synchronises. The _dev form takes DEVICE pointers — pairs int32, the others
 * fp32 (is_f32 = 1) or fp64, any element alignment — and only enqueues on the context's stream: no synchronisation, and no allocation
 * after the first call (a context whose largest possible record does not fit one workgroup's LDS allocates two [B][3][N] scratch arrays
 * then and enqueues the range slot by slot; otherwise the whole range is ONE launch).                                                  */
int dc_get_self_contact_readout(dc_ctx *ctx, int slot0, int nslots, int cap, int *pairs /*nslots*B*cap*4 or NULL*/,
                                double *impulse /*nslots*B*cap*4 or NULL*/, double *vertex_impulse /*nslots*B*3N or NULL*/,
                                double *totals /*nslots*B*8 or NULL*/);
int dc_get_self_contact_readout_dev(dc_ctx *ctx, int slot0, int nslots, int cap, void *d_pairs /*int32, nslots*B*cap*4 or NULL*/,
                                    void *d_impulse /*nslots*B*cap*4 or NULL*/, void *d_vertex_impulse /*nslots*B*N*3 or NULL*/,
                                    void *d_totals /*nslots*B*8 or NULL*/, int is_f32);
/* dc_set_mu (d_mu must not be NULL: dc_set_mu(NULL) restores the defaults) and dc_set_vertex_forces (NULL = none) from device buffers */
int dc_set_mu_dev(dc_ctx *ctx, const void *d_mu /*B*num_groups*/, int is_f32);
int dc_set_vertex_forces_dev(dc_ctx *ctx, const void *d_f /*B*3N or NULL*/, int is_f32);
/* Which tape slot holds the trajectory's INITIAL state (default 0): the backward step through record start_slot + 1 is the reference's isStart step
 * (Simulation.cpp:3947, :1534: dL_dx of the initial state takes no dL_dv / h term) in dc_rollout_backward. -1: this tape holds a LATER segment of a
 * trajectory — no step of it is the start. With it a trajectory can be run as a chain of fused segments over several contexts (e.g. one context per
 * attachment set, SceneConfiguration::customAttachmentVertexIdx, Simulation.cpp:1053-1068): state handed on with dc_get_state_dev / dc_set_state_dev,
 * the carried gradient on the way back with dc_get_gradient / dc_set_gradient (tests/test_gpu_schedules.py). dc_step_backward takes is_start itself.
 * (Each context of such a chain has its own primitive offsets — dc_set_primitive_offsets / dc_set_primitive_offset_schedule — and dc_alloc_batch,
 * dc_set_primitives and dc_build drop them: the caller sends them to every context of the chain.) */
int dc_set_trajectory_start(dc_ctx *ctx, int start_slot);
int dc_get_stats(dc_ctx *ctx, int slot, dc_step_stats *fwd /*B or NULL*/, dc_bwd_stats *bwd /*B or NULL*/);
int dc_sync(dc_ctx *ctx);
/* Split execution: with fewer rollouts than compute units (BASELINE C4 sharded over 8 GPUs: 32 per GPU; hatController.py: 20 rollouts)
 * or a mesh too large for one workgroup's LDS, a rollout is run by K workgroups that own K contiguous vertex ranges and exchange
 * boundary rows and partial sums inside the launch (csrc/dc_cluster.h). K is chosen in dc_alloc_batch from the batch size, the mesh
 * and the device (environment DC_CLUSTER=k forces k; 0 or 1 = one workgroup per rollout). Results agree with the one-workgroup
 * kernels to solver tolerance (different summation order), not bitwise. Reports K and how many rollouts one launch covers. */
int dc_get_cluster(const dc_ctx *ctx, int *workgroups_per_rollout, int *rollouts_per_launch);
/* Rows of the split: part p of a rollout owns device rows [p * rows_per_part, (p + 1) * rows_per_part) — vertex i of a mesh that was not
 * renumbered (dc_get_layout) belongs to part i / rows_per_part — and exchanges halo_rows boundary rows with each neighbour. 0, 0 with one
 * workgroup per rollout. Read-only.                                                                                                     */
int dc_get_cluster_rows(const dc_ctx *ctx, int *rows_per_part, int *halo_rows);
/* Which path the split forward kernel took for the layered self friction (Simulation.cpp:655-678), counted per rollout since dc_alloc_batch
 * (or the last reset): out[2 b] = PD iterations that ran a self-friction pass, out[2 b + 1] = those of them in which every part evaluated the
 * layers itself (the parts share an XCD and the working set fits the LDS; DC_SELF_REDUNDANT=0 turns it off) instead of part 0 alone. All zero
 * when the batch runs one workgroup per rollout. Synchronises; reset != 0 zeroes the counters afterwards.                                    */
int dc_get_self_friction_path(dc_ctx *ctx, int *out /*B*2*/, int reset);
/* Which form the contact phase of the adjoint operator took, counted per rollout since dc_alloc_batch (or the last reset): out[2 b] = backward
 * steps run by a kernel instance that can hold the step's contact tables in LDS (one workgroup per rollout, 1024 threads, diag(P)
 * preconditioner), out[2 b + 1] = those of them whose tables fitted and were built: the CG applications of such a step take the contact phase
 * from them (DC_ADJ_RESIDENT=0 turns them off; none are built for a step without self contacts on a mesh of fewer than 4 element windows,
 * whose applications form y while staging). All zero for every other instance. Synchronises; reset != 0 zeroes the counters afterwards.   */
int dc_get_adjoint_contact_path(dc_ctx *ctx, int *out /*B*2*/, int reset);
/* Which kernel set dc_build chose for this system (works on a host-only context too): out6 = {vertices renumbered on the device
 * (0 / 1), bandwidth of the system matrix in device numbering, packet-matrix forward kernel usable (needs bandwidth <= 511),
 * LDS element windows usable, number of element windows, explicit-inverse solve (small meshes)}. A mesh that fails the packet /
 * window conditions runs on the global-memory fallback kernels — correct, but several times slower. */
int dc_get_layout(const dc_ctx *ctx, int *out6);
/* Layout of the packet matrix dc_build chose (works on a host-only context): 1 = 16-bit byte offsets (the forward kernel instances that hold
 * the search direction as halves), 0 = 10-bit column deltas or no packet matrix, 2 = values only under a matrix-wide template of at most 12
 * column offsets (regularly numbered meshes: a row-major grid). DC_PK_OFS=0 at dc_build keeps the column deltas, DC_PK_TPL=0 the byte offsets. */
int dc_get_packet_layout(const dc_ctx *ctx, int *byte_offsets);
/* Whether dc_build turned the bending term of the one-workgroup kernels into per-vertex matrix rows (works on a host-only context): 1 = every
 * flap of the mesh is flat at rest (fp32 rest norm <= 1e-6) and the element windows carry no flaps, 0 = per-flap passes (any curved flap, no
 * element windows, or DC_BEND_ROWS=0 at dc_build). The split kernels keep their flaps either way.                                     */
int dc_get_bend_rows(const dc_ctx *ctx, int *rows);
/* Deflation space of the forward solve dc_build chose (works on a host-only context): number of vectors (0 = none) and the iteration
 * count of the probe solve that decided (Jacobi-PCG to 1e-4 on a smooth right-hand side).                                            */
int dc_get_deflation(const dc_ctx *ctx, int *vectors, int *probe_iterations);

/* ---- collective for C++ callers: one context (= one GPU) per rank; the optimiser sums [loss, dL/dtheta] over the ranks once per
 * evaluation, the only exchange of the rollout-sharded job. RCCL is bound at run time when these are first used.
 * rank 0 obtains a 128-byte id (dc_comm_unique_id) and hands it to the other ranks by whatever the caller has (MPI_Bcast, a file, a
 * socket); every rank then calls dc_comm_init with the same id. dc_allreduce_sum: in-place sum of `count` doubles over the ranks
 * through the context's stream (host buffer in, host buffer out; blocks). Python callers use torch.distributed instead
 * (diffcloth_amd/distributed.py). */
int dc_comm_unique_id(char *id128 /*128 bytes out*/);
int dc_comm_init(dc_ctx *ctx, int nranks, int rank, const char *id128);
int dc_allreduce_sum(dc_ctx *ctx, double *inout, int count);
int dc_comm_destroy(dc_ctx *ctx);
/* HIP-event timing of everything enqueued between the two calls on the context's stream (ms). */
int dc_timer_start(dc_ctx *ctx);
int dc_timer_stop(dc_ctx *ctx, float *ms);
/* accumulated device time (ms) and launch count of the forward / backward step kernels since the last
 * reset, measured with HIP events on the context's stream; used by bench.py's roofline block. A dc_rollout_* call
 * may run all its time steps in ONE launch (every rollout advances on its own), so launches <= steps.            */
int dc_kernel_times(dc_ctx *ctx, float *fwd_ms, int *fwd_launches, float *bwd_ms, int *bwd_launches, int reset);
/* Diagnostics of the dense direct adjoint solve (adjoint_mode 2, meshes of at most 768 vertices; any adjoint_mode may call it).
 * dc_get_adjoint_matrix: K = P - dP^T of record `slot`, rollout `rollout`, as the device assembles it for the dense solve: (3N)^2 doubles,
 * row-major, rows and columns xyz interleaved in the caller's vertex numbering (index 3 i + c) — the layout of the fp64 oracle's matrix.
 * dc_dense_phase_times: accumulated device time (ms) of the mode-2 backward steps split into assembly, factorisation and solve; measured
 * only when the environment sets DC_DENSE_TIMES=1 (each chunk then synchronises); reset != 0 zeroes them afterwards.            */
int dc_get_adjoint_matrix(dc_ctx *ctx, int slot, int rollout, double *K /*(3N)^2*/);
int dc_dense_phase_times(dc_ctx *ctx, float *ms3, int reset);
/* The banded direct adjoint solve (adjoint_mode 3). Under mode 3 dc_get_adjoint_matrix returns the band-assembled K, expanded with exact
 * zeros outside the band (same layout, same 768-vertex limit of the getter), and dc_dense_phase_times the mode-3 steps' split.
 * dc_set_adjoint_band: extra half-bandwidth in vertices for self contacts that couple outside the matrix band; >= 0, default 0; takes effect
 * at the next backward step (the band scratch is re-allocated).
 * dc_get_adjoint_band: what mode 3 would use for the built system (works on a host-only context): kl (= ku), ldab, bytes of band storage
 * per rollout.                                                                                                                          */
int dc_set_adjoint_band(dc_ctx *ctx, int extra_vertices);
int dc_get_adjoint_band(const dc_ctx *ctx, int *kl, int *ldab, long long *bytes_per_rollout);

#ifdef __cplusplus
}
#endif
#endif /* DIFFCLOTH_HIP_H */
