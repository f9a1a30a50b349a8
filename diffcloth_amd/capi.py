"""ctypes binding of libdiffcloth_hip.so (include/diffcloth_hip.h).

This is the thinnest possible Python view of the C-ABI: numpy float64 arrays in the reference's layout
(xyz-interleaved, length 3N per rollout) go straight to the `dc_*` entry points. There is no CPU fallback:
if the library is missing, or no HIP device is present, construction raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libdiffcloth_hip.so")

DC_PRIM_SPHERE, DC_PRIM_CAPSULE, DC_PRIM_PLANE, DC_PRIM_BOWL, DC_PRIM_SPHERE_DISCRETIZED = 0, 1, 2, 3, 4


class DcError(RuntimeError):
    pass


class dc_primitive(C.Structure):
    _fields_ = [("kind", C.c_int), ("group", C.c_int), ("center", C.c_double * 3), ("top_offset", C.c_double * 3),
                ("corner2", C.c_double * 3), ("radius", C.c_double), ("length", C.c_double), ("mu", C.c_double), ("rotates", C.c_int)]


class dc_params(C.Structure):
    _fields_ = [("time_step", C.c_double), ("density", C.c_double), ("k_stretch", C.c_double), ("k_bend", C.c_double),
                ("k_att", C.c_double), ("gravity", C.c_double * 3), ("forward_tol", C.c_double),
                ("backward_tol", C.c_double), ("gravity_enabled", C.c_int), ("contact_enabled", C.c_int),
                ("selfcollision_enabled", C.c_int), ("gradient_clipping", C.c_int),
                ("gradient_clipping_threshold", C.c_double), ("pd_iter_cap", C.c_int), ("adjoint_iter_cap", C.c_int),
                ("cg_rel_tol", C.c_double), ("cg_max_iter", C.c_int), ("stall_window", C.c_int),
                ("adjoint_mode", C.c_int), ("adjoint_rel_tol", C.c_double), ("adjoint_block_precond", C.c_int), ("adjoint_fp32_only", C.c_int),
                ("max_self_contacts", C.c_int), ("forward_deflation", C.c_int)]


class dc_step_stats(C.Structure):
    _fields_ = [("converged", C.c_int), ("pd_iters", C.c_int), ("cg_iters", C.c_int), ("prim_contacts", C.c_int),
                ("self_contacts", C.c_int), ("last_xdiff", C.c_float), ("self_overflow", C.c_int)]


class dc_bwd_stats(C.Structure):
    _fields_ = [("converged", C.c_int), ("adjoint_iters", C.c_int), ("cg_iters", C.c_int), ("clipped", C.c_int), ("used_direct", C.c_int),
                ("last_udiff", C.c_float), ("refine_cycles", C.c_int), ("fp64_iters", C.c_int), ("residual_verified", C.c_int), ("workgroups", C.c_int)]


class dc_record(C.Structure):
    _fields_ = [("x", C.POINTER(C.c_double)), ("v", C.POINTER(C.c_double)), ("f", C.POINTER(C.c_double)), ("r", C.POINTER(C.c_double)),
                ("prim", C.POINTER(C.c_int)), ("normal", C.POINTER(C.c_double)), ("x_fixed", C.POINTER(C.c_double)),
                ("self_count", C.POINTER(C.c_int)), ("self_pairs", C.POINTER(C.c_int)), ("self_layer", C.POINTER(C.c_int)),
                ("self_normal", C.POINTER(C.c_double)), ("self_d", C.POINTER(C.c_double))]


EXPORTED_SYMBOLS = [
    "dc_create", "dc_destroy", "dc_last_error", "dc_version", "dc_set_mesh", "dc_set_attachments", "dc_set_params",
    "dc_set_primitives", "dc_build", "dc_default_params", "dc_set_solver", "dc_set_flags", "dc_get_counts", "dc_get_system_matrix",
    "dc_get_vertex_data", "dc_alloc_batch", "dc_set_state", "dc_get_state", "dc_set_mu", "dc_set_uniform_force", "dc_set_vertex_forces", "dc_set_vertex_force_field", "dc_get_force_gradient",
    "dc_step_forward", "dc_get_record", "dc_get_contacts", "dc_get_self_contacts", "dc_step_backward", "dc_rollout_forward",
    "dc_seed_gradient", "dc_rollout_backward", "dc_get_gradient", "dc_get_param_gradients", "dc_get_stats", "dc_sync", "dc_timer_start",
    "dc_timer_stop", "dc_kernel_times", "dc_get_cluster", "dc_get_cluster_rows", "dc_set_gradient", "dc_set_fixed_point_schedule", "dc_set_force_schedule",
    "dc_set_seed_schedule", "dc_clear_schedules", "dc_get_states", "dc_get_dxfixed", "dc_get_layout", "dc_get_packet_layout", "dc_get_bend_rows", "dc_comm_unique_id", "dc_comm_init", "dc_allreduce_sum", "dc_comm_destroy",
    "dc_get_deflation", "dc_set_record", "dc_set_trajectory_start", "dc_keep_force_gradients", "dc_get_force_gradients", "dc_use_stream", "dc_set_state_dev", "dc_get_state_dev", "dc_step_forward_dev", "dc_step_backward_dev",
    "dc_get_self_friction_path", "dc_get_adjoint_contact_path", "dc_get_adjoint_matrix", "dc_dense_phase_times", "dc_set_adjoint_band", "dc_get_adjoint_band",
    "dc_rollout_forward_async", "dc_rollout_backward_async", "dc_set_fixed_point_schedule_dev", "dc_set_force_schedule_dev", "dc_set_seed_schedule_dev",
    "dc_set_gradient_dev", "dc_get_gradient_dev", "dc_get_states_dev", "dc_get_dxfixed_dev", "dc_get_force_schedule_gradients_dev", "dc_set_mu_dev",
    "dc_set_vertex_forces_dev",
    "dc_set_primitive_offsets", "dc_set_primitive_offset_schedule", "dc_set_primitive_offsets_dev", "dc_set_primitive_offset_schedule_dev",
    "dc_get_primitive_centers",
    "dc_set_primitive_velocities", "dc_set_primitive_velocity_schedule", "dc_set_primitive_velocities_dev", "dc_set_primitive_velocity_schedule_dev",
    "dc_get_primitive_velocities", "dc_get_primitive_velocity_gradients", "dc_get_primitive_velocity_gradients_dev",
    "dc_set_primitive_spins", "dc_set_primitive_spin_schedule", "dc_set_primitive_spins_dev", "dc_set_primitive_spin_schedule_dev",
    "dc_get_primitive_spins", "dc_get_primitive_spin_gradients", "dc_get_primitive_spin_gradients_dev",
    "dc_set_primitive_shapes", "dc_set_primitive_shape_schedule", "dc_set_primitive_shapes_dev", "dc_set_primitive_shape_schedule_dev",
    "dc_get_primitive_shapes",
    "dc_get_contact_readout", "dc_get_contact_readout_dev",
    "dc_set_contact_readout_gradients", "dc_set_contact_readout_gradients_dev",
    "dc_get_self_contact_readout", "dc_get_self_contact_readout_dev",
]

_lib = None
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)


def load_library():
    """Loads libdiffcloth_hip.so; raises if it has not been built (see diffcloth_amd/build.py)."""
    global _lib
    if _lib is None:
        path = os.environ.get("DC_LIB", LIB_PATH)        # development switch: A/B runs of two builds of the library
        if not os.path.exists(path):
            raise DcError(f"{path} not found: run `python -m diffcloth_amd.build` (hipcc, gfx950)")
        lib = C.CDLL(path)
        lib.dc_last_error.restype = C.c_char_p
        lib.dc_version.restype = C.c_char_p
        lib.dc_get_self_contact_readout.restype = C.c_int
        lib.dc_get_self_contact_readout.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.dc_get_self_contact_readout_dev.restype = C.c_int
        lib.dc_get_self_contact_readout_dev.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        _lib = lib
    return _lib


def _d(a):
    return a.ctypes.data_as(_dp) if a is not None else None


def _i(a):
    return a.ctypes.data_as(_ip) if a is not None else None


def _f64(a):
    return None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.float64))


def _i32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.int32))


def _stats_to_dict(arr, fields):
    return {f: np.array([getattr(s, f) for s in arr]) for f in fields}


class Engine:
    """One dc_ctx. Mirrors the call sequence of include/diffcloth_hip.h one to one."""

    def __init__(self, device=0):
        self.lib = load_library()
        h = C.c_void_p()
        rc = self.lib.dc_create(C.c_int(device), C.byref(h))
        if rc != 0:
            raise DcError(f"dc_create failed with code {rc}: no HIP device available (there is no CPU fallback)")
        self.h = h
        self.device = device
        self.params = dc_params()
        self.lib.dc_default_params(C.byref(self.params))
        self.N = self.T = self.E = self.Af = 0
        self.B = 0
        self.ngroups = 1
        self.nprims = 0
        self._built_shapes = np.zeros((0, 8))

    def close(self):
        if getattr(self, "h", None):
            self.lib.dc_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise DcError(f"code {rc}: {self.lib.dc_last_error(self.h).decode()}")

    # ---- system ----
    def set_mesh(self, verts, tris):
        v = _f64(verts).reshape(-1)
        t = _i32(tris).reshape(-1)
        self._chk(self.lib.dc_set_mesh(self.h, C.c_int(v.size // 3), _d(v), C.c_int(t.size // 3), _i(t)))

    def set_attachments(self, vertices):
        a = _i32(vertices).reshape(-1)
        self._chk(self.lib.dc_set_attachments(self.h, C.c_int(a.size), _i(a)))

    def set_params(self, **kw):
        for k, v in kw.items():
            if k == "gravity":
                for d in range(3):
                    self.params.gravity[d] = float(v[d])
            elif hasattr(self.params, k):
                setattr(self.params, k, v)
            else:
                raise KeyError(k)
        self._chk(self.lib.dc_set_params(self.h, C.byref(self.params)))

    def set_solver(self, forward_tol=None, backward_tol=None, gradient_clipping=None, clip_threshold=None, force_direct_adjoint=None):
        """dc_set_solver: the solver knobs the reference reads from its process-global statics at every step; no rebuild, the batch and
        its tape stay valid. Arguments left None keep their current value."""
        p = self.params
        if forward_tol is not None: p.forward_tol = forward_tol
        if backward_tol is not None: p.backward_tol = backward_tol
        if gradient_clipping is not None: p.gradient_clipping = int(gradient_clipping)
        if clip_threshold is not None: p.gradient_clipping_threshold = clip_threshold
        # a direct solve asked for keeps the dense one (adjoint_mode 2) and the banded one (adjoint_mode 3), as dc_set_solver does
        if force_direct_adjoint is not None: p.adjoint_mode = (p.adjoint_mode if p.adjoint_mode in (2, 3) else 1) if force_direct_adjoint else 0
        self._chk(self.lib.dc_set_solver(self.h, C.c_double(p.forward_tol), C.c_double(p.backward_tol), C.c_int(p.gradient_clipping),
                                         C.c_double(p.gradient_clipping_threshold), C.c_int(int(p.adjoint_mode in (1, 2, 3)))))

    def set_primitives(self, prims):
        """prims: list of dicts(kind, group, center, top_offset, radius, length, mu, rotates)."""
        arr = (dc_primitive * max(len(prims), 1))()
        groups = []
        for k, p in enumerate(prims):
            arr[k].kind = p.get("kind", DC_PRIM_SPHERE)
            arr[k].group = p.get("group", k)
            for d in range(3):
                arr[k].center[d] = float(p["center"][d])
                arr[k].top_offset[d] = float(p.get("top_offset", (0, 0, 0))[d])
                arr[k].corner2[d] = float(p.get("corner2", (0, 0, 0))[d])
            arr[k].radius = float(p["radius"])
            arr[k].length = float(p.get("length", 0.0))
            arr[k].mu = float(p.get("mu", 0.0))
            arr[k].rotates = int(p.get("rotates", 0))
            if arr[k].group not in groups:
                groups.append(arr[k].group)
        self.ngroups = max(len(groups), 1)
        self.nprims = len(prims)
        self._built_shapes = np.array([[arr[k].top_offset[d] for d in range(3)] + [arr[k].corner2[d] for d in range(3)] + [arr[k].radius, arr[k].length]
                                       for k in range(len(prims))], dtype=np.float64).reshape(len(prims), 8)
        self._chk(self.lib.dc_set_primitives(self.h, C.c_int(len(prims)), arr))

    def build(self):
        self._chk(self.lib.dc_build(self.h))
        c = _i32(np.zeros(6))
        self._chk(self.lib.dc_get_counts(self.h, _i(c)))
        self.N, self.T, self.E, self.Af, self.nnz, self.rows = [int(x) for x in c]
        return self

    def system_matrix(self):
        ptr = _i32(np.zeros(self.N + 1)); col = _i32(np.zeros(self.nnz)); val = _f64(np.zeros(self.nnz))
        self._chk(self.lib.dc_get_system_matrix(self.h, _i(ptr), _i(col), _d(val)))
        return ptr, col, val

    def vertex_data(self):
        m = _f64(np.zeros(self.N)); a = _f64(np.zeros(self.N)); r = _f64(np.zeros(self.N))
        self._chk(self.lib.dc_get_vertex_data(self.h, _d(m), _d(a), _d(r)))
        return m, a, r

    # ---- batch ----
    def alloc_batch(self, batch, tape_steps):
        self._chk(self.lib.dc_alloc_batch(self.h, C.c_int(batch), C.c_int(tape_steps)))
        self.B = batch
        self.tape = tape_steps

    def _vec(self, a, per):
        a = _f64(a).reshape(-1)
        if a.size != self.B * per:
            raise ValueError(f"expected {self.B}x{per} values, got {a.size}")
        return a

    def set_state(self, slot, x, v):
        x = self._vec(x, 3 * self.N); v = self._vec(v, 3 * self.N)
        self._chk(self.lib.dc_set_state(self.h, C.c_int(slot), _d(x), _d(v)))

    def get_state(self, slot):
        x = np.zeros((self.B, 3 * self.N)); v = np.zeros((self.B, 3 * self.N))
        self._chk(self.lib.dc_get_state(self.h, C.c_int(slot), _d(x), _d(v)))
        return x, v

    def set_mu(self, mu):
        m = None if mu is None else self._vec(mu, self.ngroups)
        self._chk(self.lib.dc_set_mu(self.h, _d(m)))

    def set_uniform_force(self, f):
        a = None if f is None else self._vec(f, 3)
        self._chk(self.lib.dc_set_uniform_force(self.h, _d(a)))

    def set_vertex_forces(self, f):
        a = None if f is None else self._vec(f, 3 * self.N)
        self._chk(self.lib.dc_set_vertex_forces(self.h, _d(a)))

    def set_vertex_force_field(self, f):
        """second per-vertex force term with factor 1 (the constant force field next to a scheduled wind with fall-off)"""
        a = None if f is None else self._vec(f, 3 * self.N)
        self._chk(self.lib.dc_set_vertex_force_field(self.h, _d(a)))

    def set_primitive_offsets(self, d):
        """d: [B][G][3] offsets of the primitive groups' centres for the NEXT forward steps (dc_set_primitive_offsets: every primitive of group g
        of rollout b is tested at fp32(center + d[b][g]), the sum in fp64); None restores the built centres"""
        a = None if d is None else self._vec(d, 3 * self.ngroups)
        self._chk(self.lib.dc_set_primitive_offsets(self.h, _d(a)))

    def set_primitive_offset_schedule(self, slot0, d):
        """d: [nsteps][B][G][3]: the step slot0+k -> slot0+k+1 uses d[k] (dc_set_primitive_offset_schedule)"""
        d = np.ascontiguousarray(np.asarray(d, dtype=np.float64).reshape(-1, self.B, self.ngroups, 3))
        self._chk(self.lib.dc_set_primitive_offset_schedule(self.h, C.c_int(slot0), C.c_int(d.shape[0]), _d(d)))

    def get_primitive_centers(self, slot):
        """[B][P][3] absolute centres of the flattened primitives that the step which produced `slot` used (fp32 values, widened)"""
        out = np.zeros((self.B, self.nprims, 3))
        self._chk(self.lib.dc_get_primitive_centers(self.h, C.c_int(slot), _d(out)))
        return out

    def set_primitive_velocities(self, w):
        """w: [B][G][3] velocities of the primitive groups for the NEXT forward steps (dc_set_primitive_velocities: d = (f - v_rot m) - w m in
        the friction law, detection samples pos + (vel - w) h k / 2; stored as fp32); None = zeros"""
        a = None if w is None else self._vec(w, 3 * self.ngroups)
        self._chk(self.lib.dc_set_primitive_velocities(self.h, _d(a)))

    def set_primitive_velocity_schedule(self, slot0, w):
        """w: [nsteps][B][G][3]: the step slot0+k -> slot0+k+1 uses w[k] (dc_set_primitive_velocity_schedule)"""
        w = np.ascontiguousarray(np.asarray(w, dtype=np.float64).reshape(-1, self.B, self.ngroups, 3))
        self._chk(self.lib.dc_set_primitive_velocity_schedule(self.h, C.c_int(slot0), C.c_int(w.shape[0]), _d(w)))

    def get_primitive_velocities(self, slot):
        """[B][G][3] velocities that the step which produced `slot` used (fp32 values, widened; zeros when none was ever set)"""
        out = np.zeros((self.B, self.ngroups, 3))
        self._chk(self.lib.dc_get_primitive_velocities(self.h, C.c_int(slot), _d(out)))
        return out

    def get_primitive_velocity_gradients(self, slot0, nslots):
        """[nslots][B][G][3] dL/dw of the backward steps through records slot0 .. slot0+nslots-1 (dc_get_primitive_velocity_gradients)"""
        out = np.zeros((nslots, self.B, self.ngroups, 3))
        self._chk(self.lib.dc_get_primitive_velocity_gradients(self.h, C.c_int(slot0), C.c_int(nslots), _d(out)))
        return out

    def built_primitive_shapes(self):
        """[P][8] float64 shape rows {top_offset[3], corner2[3], radius, length} of the dicts last given to set_primitives, unrounded: what
        set_primitive_shapes takes per rollout (host side, no C call)"""
        return self._built_shapes.copy()

    def set_primitive_shapes(self, s):
        """s: [B][P][8] shape rows {top_offset[3], corner2[3], radius, length} of the flattened primitives for the NEXT forward steps
        (dc_set_primitive_shapes: stored as fp32, read by the kernels in place of the built values); None restores the built shapes"""
        a = None if s is None else self._vec(s, 8 * self.nprims)
        self._chk(self.lib.dc_set_primitive_shapes(self.h, _d(a)))

    def set_primitive_shape_schedule(self, slot0, s):
        """s: [nsteps][B][P][8]: the step slot0+k -> slot0+k+1 uses s[k] (dc_set_primitive_shape_schedule)"""
        s = np.ascontiguousarray(np.asarray(s, dtype=np.float64).reshape(-1, self.B, self.nprims, 8))
        self._chk(self.lib.dc_set_primitive_shape_schedule(self.h, C.c_int(slot0), C.c_int(s.shape[0]), _d(s)))

    def get_primitive_shapes(self, slot):
        """[B][P][8] shape rows that the step which produced `slot` used (fp32 values, widened; the built shapes when none was ever set)"""
        out = np.zeros((self.B, self.nprims, 8))
        self._chk(self.lib.dc_get_primitive_shapes(self.h, C.c_int(slot), _d(out)))
        return out

    def set_primitive_spins(self, omega):
        """omega: [B][G][3] angular velocities (rad/s) of the primitive groups for the NEXT forward steps (dc_set_primitive_spins: a DC_PRIM_SPHERE
        adds v_spin = radius (omega x n) to the v_out of the friction law; stored as fp32); None = zeros"""
        a = None if omega is None else self._vec(omega, 3 * self.ngroups)
        self._chk(self.lib.dc_set_primitive_spins(self.h, _d(a)))

    def set_primitive_spin_schedule(self, slot0, omega):
        """omega: [nsteps][B][G][3]: the step slot0+k -> slot0+k+1 uses omega[k] (dc_set_primitive_spin_schedule)"""
        omega = np.ascontiguousarray(np.asarray(omega, dtype=np.float64).reshape(-1, self.B, self.ngroups, 3))
        self._chk(self.lib.dc_set_primitive_spin_schedule(self.h, C.c_int(slot0), C.c_int(omega.shape[0]), _d(omega)))

    def get_primitive_spins(self, slot):
        """[B][G][3] angular velocities that the step which produced `slot` used (fp32 values, widened; zeros when none was ever set)"""
        out = np.zeros((self.B, self.ngroups, 3))
        self._chk(self.lib.dc_get_primitive_spins(self.h, C.c_int(slot), _d(out)))
        return out

    def get_primitive_spin_gradients(self, slot0, nslots):
        """[nslots][B][G][3] dL/domega of the backward steps through records slot0 .. slot0+nslots-1 (dc_get_primitive_spin_gradients)"""
        out = np.zeros((nslots, self.B, self.ngroups, 3))
        self._chk(self.lib.dc_get_primitive_spin_gradients(self.h, C.c_int(slot0), C.c_int(nslots), _d(out)))
        return out

    def get_force_gradient(self):
        """h^2 (I + dr_df)^T u* per vertex of the last backward step (dL_dfext_vec of the reference)."""
        out = np.zeros((self.B, 3 * self.N))
        self._chk(self.lib.dc_get_force_gradient(self.h, _d(out)))
        return out

    def keep_force_gradients(self, keep=True):
        self._chk(self.lib.dc_keep_force_gradients(self.h, C.c_int(int(keep))))

    def get_force_gradients(self, slot0, nslots):
        """h^2 (I + dr_df)^T u* per vertex of the backward steps through records slot0 .. slot0 + nslots - 1 (after keep_force_gradients)."""
        out = np.zeros((nslots, self.B, 3 * self.N))
        self._chk(self.lib.dc_get_force_gradients(self.h, C.c_int(slot0), C.c_int(nslots), _d(out)))
        return out

    # ---- hot path ----
    def step_forward(self, slot, fixed_pts=None, want_stats=True):
        fp = None if fixed_pts is None else self._vec(fixed_pts, 3 * self.Af)
        st = (dc_step_stats * self.B)() if want_stats else None
        self._chk(self.lib.dc_step_forward(self.h, C.c_int(slot), _d(fp), st))
        if want_stats:
            return _stats_to_dict(st, ["converged", "pd_iters", "cg_iters", "prim_contacts", "self_contacts", "last_xdiff", "self_overflow"])
        return None

    def get_record(self, slot):
        f = np.zeros((self.B, 3 * self.N)); r = np.zeros((self.B, 3 * self.N))
        self._chk(self.lib.dc_get_record(self.h, C.c_int(slot), _d(f), _d(r)))
        return f, r

    def set_record(self, slot, x, v, f, prim, normal, r=None, x_fixed=None, self_contacts=None):
        """dc_set_record: the forward record of `slot` handed in from outside (fp64 values kept for the adjoint's fp64 operator).
        prim: [B][N] index into the primitive list or -1; self_contacts: per rollout a dict(pairs [C][2], layer [C], normal [C][3], d [C][3])
        in layer order, or None."""
        rec = dc_record()
        keep = []

        def dptr(a, per):
            if a is None:
                return None
            a = self._vec(a, per); keep.append(a)
            return _d(a)
        n3 = 3 * self.N
        rec.x = dptr(x, n3); rec.v = dptr(v, n3); rec.f = dptr(f, n3); rec.r = dptr(r, n3); rec.normal = dptr(normal, n3)
        rec.x_fixed = dptr(x_fixed, 3 * self.Af)
        pr = _i32(prim).reshape(-1)
        if pr.size != self.B * self.N:
            raise ValueError("prim: expected B x N entries")
        keep.append(pr); rec.prim = _i(pr)
        if self_contacts is not None:
            cnt = _i32([0 if sc is None else len(sc["layer"]) for sc in self_contacts])
            live = [sc for sc in self_contacts if sc is not None and len(sc["layer"])]
            pairs = _i32(np.concatenate([np.asarray(sc["pairs"]).reshape(-1, 2) for sc in live]) if live else np.zeros((0, 2)))
            layer = _i32(np.concatenate([np.asarray(sc["layer"]).reshape(-1) for sc in live]) if live else np.zeros(0))
            nrm = _f64(np.concatenate([np.asarray(sc["normal"]).reshape(-1, 3) for sc in live]) if live else np.zeros((0, 3)))
            dd = _f64(np.concatenate([np.asarray(sc["d"]).reshape(-1, 3) for sc in live]) if live else np.zeros((0, 3)))
            keep += [cnt, pairs, layer, nrm, dd]
            rec.self_count = _i(cnt); rec.self_pairs = _i(pairs); rec.self_layer = _i(layer); rec.self_normal = _d(nrm); rec.self_d = _d(dd)
        self._chk(self.lib.dc_set_record(self.h, C.c_int(slot), C.byref(rec)))

    def get_contacts(self, slot):
        g = np.zeros((self.B, self.N), dtype=np.int32); n = np.zeros((self.B, 3 * self.N))
        self._chk(self.lib.dc_get_contacts(self.h, C.c_int(slot), _i(g), _d(n)))
        return g, n

    def _readout_range(self, slot0, nslots):
        slot0, nslots = int(slot0), int(nslots)
        if slot0 < 1:
            raise ValueError("contact_readout: slot 0 has no record (slot0 >= 1)")
        if nslots < 1:
            raise ValueError("contact_readout: nslots must be >= 1")
        return slot0, nslots

    def contact_readout(self, slot0, nslots=1, state=True, normal_impulse=True, wrench=True):
        """dc_get_contact_readout of the records slot0 .. slot0 + nslots - 1: dict(state [nslots][B][N] int32 — 0 not in primitive contact,
        1 take-off, 2 stick, 3 slide —, normal_impulse [nslots][B][N], wrench [nslots][B][G][10] = {J[3], tau[3], sum jn, take-off, stick,
        slide counts} per primitive group; J is the momentum handed to the obstacle in the step, J / time_step the mean force). Each output
        can be switched off (its entry is then None); the call synchronises."""
        slot0, nslots = self._readout_range(slot0, nslots)
        if not (state or normal_impulse or wrench):
            raise ValueError("contact_readout: nothing asked for")
        s = np.zeros((nslots, self.B, self.N), dtype=np.int32) if state else None
        j = np.zeros((nslots, self.B, self.N)) if normal_impulse else None
        w = np.zeros((nslots, self.B, self.ngroups, 10)) if wrench else None
        self._chk(self.lib.dc_get_contact_readout(self.h, C.c_int(slot0), C.c_int(nslots), _i(s), _d(j), _d(w)))
        return dict(state=s, normal_impulse=j, wrench=w)

    def contact_readout_dev(self, slot0, nslots, state=None, normal_impulse=None, wrench=None):
        """dc_get_contact_readout_dev into CUDA tensors: state int32 [nslots][B][N], normal_impulse [nslots][B][N] and wrench
        [nslots][B][G][10] of one floating dtype; None skips an output. Only enqueued on the context's stream."""
        import torch
        slot0, nslots = self._readout_range(slot0, nslots)
        if state is None and normal_impulse is None and wrench is None:
            raise ValueError("contact_readout_dev: nothing asked for")
        ps = None
        if state is not None:
            if not state.is_cuda or not state.is_contiguous() or state.dtype != torch.int32 or state.numel() != nslots * self.B * self.N:
                raise ValueError(f"state: expected a contiguous CUDA int32 tensor of {nslots * self.B * self.N} elements, got {state.dtype} {tuple(state.shape)} on {state.device}")
            if state.device.index != self.device:
                raise ValueError(f"tensor on cuda:{state.device.index}, the engine runs on device {self.device}")
            ps = C.c_void_p(state.data_ptr())
        (pj, pw), f = self._tps((normal_impulse, self.B * self.N, nslots), (wrench, self.B * self.ngroups * 10, nslots))
        self._chk(self.lib.dc_get_contact_readout_dev(self.h, C.c_int(slot0), C.c_int(nslots), ps, pj, pw, C.c_int(f)))

    def set_contact_readout_gradients(self, slot0=1, dL_djn=None, dL_dwrench=None):
        """dc_set_contact_readout_gradients: the gradient of a loss with respect to the contact read-out of the records slot0 .. slot0 + nslots - 1,
        dL_djn [nslots][B][N] and / or dL_dwrench [nslots][B][G][10] (entries 7..9, the counts, are ignored); nslots is the arrays' leading
        dimension. The backward steps and sweeps through those records then add the read-out's part to every gradient they leave. One of the
        two may be None (zeros); both None clears all weights, as clear_schedules and alloc_batch do."""
        j, w = _f64(dL_djn), _f64(dL_dwrench)
        if j is None and w is None:
            self._chk(self.lib.dc_set_contact_readout_gradients(self.h, C.c_int(int(slot0)), C.c_int(0), None, None))
            return
        nslots = None
        if j is not None:
            j = j.reshape(-1, self.B, self.N)
            nslots = j.shape[0]
        if w is not None:
            w = w.reshape(-1, self.B, self.ngroups, 10)
            if nslots is not None and w.shape[0] != nslots:
                raise ValueError(f"set_contact_readout_gradients: dL_djn covers {nslots} slot(s), dL_dwrench {w.shape[0]}")
            nslots = w.shape[0]
        slot0, nslots = self._readout_range(slot0, nslots)
        self._chk(self.lib.dc_set_contact_readout_gradients(self.h, C.c_int(slot0), C.c_int(nslots), _d(j), _d(w)))

    def set_contact_readout_gradients_dev(self, slot0, nslots, dL_djn=None, dL_dwrench=None):
        """dc_set_contact_readout_gradients_dev from CUDA tensors of one floating dtype: dL_djn [nslots][B][N], dL_dwrench [nslots][B][G][10];
        one may be None (zeros), both None clears all weights. Only enqueued on the context's stream."""
        if dL_djn is None and dL_dwrench is None:
            self._chk(self.lib.dc_set_contact_readout_gradients_dev(self.h, C.c_int(int(slot0)), C.c_int(0), None, None, C.c_int(1)))
            return
        slot0, nslots = self._readout_range(slot0, nslots)
        (pj, pw), f = self._tps((dL_djn, self.B * self.N, nslots), (dL_dwrench, self.B * self.ngroups * 10, nslots))
        self._chk(self.lib.dc_set_contact_readout_gradients_dev(self.h, C.c_int(slot0), C.c_int(nslots), pj, pw, C.c_int(f)))

    @property
    def max_self_contacts(self):
        """entries of a rollout's self-contact list as dc_build sizes it: dc_params::max_self_contacts, max(2048, N) where that is 0, at most 16000"""
        m = int(self.params.max_self_contacts)
        return min(m if m > 0 else max(2048, self.N), 16000)

    def _self_readout_range(self, who, slot0, nslots, cap, listed):
        slot0, nslots = int(slot0), int(nslots)
        if slot0 < 1:
            raise ValueError(f"{who}: slot 0 has no record (slot0 >= 1)")
        if nslots < 1:
            raise ValueError(f"{who}: nslots must be >= 1")
        cap = self.max_self_contacts if cap is None else int(cap)
        if listed and cap < 1:
            raise ValueError(f"{who}: cap must be >= 1 where pairs or impulse is asked for")
        return slot0, nslots, max(cap, 0)

    def self_contact_readout(self, slot0, nslots=1, cap=None, pairs=True, impulse=True, vertex_impulse=True, totals=True):
        """dc_get_self_contact_readout of the records slot0 .. slot0 + nslots - 1: dict(pairs [nslots][B][cap][4] int32 = {id1, id2, layer,
        state} — state 1 take-off, 2 stick, 3 slide; {-1, -1, -1, 0} behind the list —, impulse [nslots][B][cap][4] = {r_k, jn_k}, r_k the
        impulse on id1 (id2 receives -r_k), vertex_impulse [nslots][B][N][3] = the per-vertex sums, totals [nslots][B][8] = {contacts, layers,
        distinct vertices, sum jn, sum |r_T|, take-off, stick, slide}). cap None = the context's max_self_contacts. Each output can be
        switched off (its entry is then None); the call synchronises. The outputs carry no gradient."""
        if not (pairs or impulse or vertex_impulse or totals):
            raise ValueError("self_contact_readout: nothing asked for")
        slot0, nslots, cap = self._self_readout_range("self_contact_readout", slot0, nslots, cap, pairs or impulse)
        p = np.zeros((nslots, self.B, cap, 4), dtype=np.int32) if pairs else None
        r = np.zeros((nslots, self.B, cap, 4)) if impulse else None
        v = np.zeros((nslots, self.B, self.N, 3)) if vertex_impulse else None
        t = np.zeros((nslots, self.B, 8)) if totals else None
        self._chk(self.lib.dc_get_self_contact_readout(self.h, slot0, nslots, cap, _i(p), _d(r), _d(v), _d(t)))
        return dict(pairs=p, impulse=r, vertex_impulse=v, totals=t)

    def self_contact_readout_dev(self, slot0, nslots, cap, pairs=None, impulse=None, vertex_impulse=None, totals=None):
        """dc_get_self_contact_readout_dev into CUDA tensors: pairs int32 [nslots][B][cap][4], impulse [nslots][B][cap][4], vertex_impulse
        [nslots][B][N][3] and totals [nslots][B][8] of one floating dtype; None skips an output. Only enqueued on the context's stream."""
        import torch
        if pairs is None and impulse is None and vertex_impulse is None and totals is None:
            raise ValueError("self_contact_readout_dev: nothing asked for")
        slot0, nslots, cap = self._self_readout_range("self_contact_readout_dev", slot0, nslots, cap, pairs is not None or impulse is not None)
        pp = None
        if pairs is not None:
            if not pairs.is_cuda or not pairs.is_contiguous() or pairs.dtype != torch.int32 or pairs.numel() != nslots * self.B * cap * 4:
                raise ValueError(f"pairs: expected a contiguous CUDA int32 tensor of {nslots * self.B * cap * 4} elements, got {pairs.dtype} {tuple(pairs.shape)} on {pairs.device}")
            if pairs.device.index != self.device:
                raise ValueError(f"tensor on cuda:{pairs.device.index}, the engine runs on device {self.device}")
            pp = C.c_void_p(pairs.data_ptr())
        (pi, pv, pt), f = self._tps((impulse, self.B * cap * 4, nslots), (vertex_impulse, self.B * self.N * 3, nslots), (totals, self.B * 8, nslots))
        self._chk(self.lib.dc_get_self_contact_readout_dev(self.h, slot0, nslots, cap, pp, pi, pv, pt, f))

    def get_self_contacts(self, slot, rollout=0, cap=8192):
        cnt = C.c_int(); nl = C.c_int()
        pairs = np.zeros((cap, 2), dtype=np.int32); layer = np.zeros(cap, dtype=np.int32); nrm = np.zeros((cap, 3))
        self._chk(self.lib.dc_get_self_contacts(self.h, C.c_int(slot), C.c_int(rollout), C.c_int(cap), C.byref(cnt), C.byref(nl),
                                                _i(pairs), _i(layer), _d(nrm)))
        n = min(cnt.value, cap)
        return dict(count=cnt.value, layers=nl.value, pairs=pairs[:n], layer=layer[:n], normal=nrm[:n])

    def step_backward(self, slot, dL_dxnew, dL_dvnew, dL_dxinit=None, dL_dvinit=None, is_start=False):
        n3 = 3 * self.N
        gx = self._vec(dL_dxnew, n3); gv = self._vec(dL_dvnew, n3)
        ix = None if dL_dxinit is None else self._vec(dL_dxinit, n3)
        iv = None if dL_dvinit is None else self._vec(dL_dvinit, n3)
        dx = np.zeros((self.B, n3)); dv = np.zeros((self.B, n3))
        dxf = np.zeros((self.B, max(3 * self.Af, 1))); dmu = np.zeros((self.B, self.ngroups))
        st = (dc_bwd_stats * self.B)()
        self._chk(self.lib.dc_step_backward(self.h, C.c_int(slot), _d(gx), _d(gv), _d(ix), _d(iv), C.c_int(int(is_start)),
                                            _d(dx), _d(dv), _d(dxf), _d(dmu), st))
        out = dict(dL_dx=dx, dL_dv=dv, dL_dxfixed=dxf[:, :3 * self.Af], dL_dmu=dmu)
        out.update(_stats_to_dict(st, ["converged", "adjoint_iters", "cg_iters", "clipped", "used_direct", "last_udiff", "refine_cycles", "fp64_iters", "residual_verified", "workgroups"]))
        return out

    # ---- device-pointer boundary (torch tensors on this GPU: no host copies, no synchronisation) ----
    def _tp(self, t, per, lead=1):
        """(device pointer, is_f32) of a contiguous CUDA tensor of lead * per elements, fp32 or fp64, on the engine's GPU; `lead` counts the
        leading dimension of the whole-sweep calls (tape slots), 1 for the per-step ones"""
        dev = getattr(self, "device", None)
        import torch
        if t is None:
            return None, 1
        if t.is_cuda and dev is not None and t.device.index != dev:
            raise ValueError(f"tensor on cuda:{t.device.index}, the engine runs on device {dev}")
        if not t.is_cuda or not t.is_contiguous() or t.dtype not in (torch.float32, torch.float64) or t.numel() != lead * per:
            raise ValueError(f"expected a contiguous CUDA float32 / float64 tensor of {lead * per} elements, got {t.dtype} {tuple(t.shape)} on {t.device}")
        return C.c_void_p(t.data_ptr()), int(t.dtype == torch.float32)

    def _tps(self, *specs):
        """pointers of the tensors of ONE call, specs = (tensor or None, elements per slot, slots): they must share one dtype; returns
        ([pointers], is_f32)"""
        ptrs, kinds = [], set()
        for t, per, lead in specs:
            p, f = self._tp(t, per, lead)
            ptrs.append(p)
            if t is not None:
                kinds.add(f)
        if len(kinds) > 1:
            raise ValueError("all tensors of a call must have one dtype")
        return ptrs, (kinds.pop() if kinds else 1)

    def use_stream(self, stream=None):
        """run the context on a torch.cuda.Stream (None: back to its own stream)"""
        self._chk(self.lib.dc_use_stream(self.h, C.c_void_p(stream.cuda_stream) if stream is not None else None))

    def set_state_dev(self, slot, x, v):
        px, f = self._tp(x, self.B * 3 * self.N); pv, f2 = self._tp(v, self.B * 3 * self.N)
        assert f == f2, "x and v must have one dtype"
        self._chk(self.lib.dc_set_state_dev(self.h, C.c_int(slot), px, pv, C.c_int(f)))

    def get_state_dev(self, slot, x, v):
        px, f = self._tp(x, self.B * 3 * self.N); pv, f2 = self._tp(v, self.B * 3 * self.N)
        assert f == f2, "x and v must have one dtype"
        self._chk(self.lib.dc_get_state_dev(self.h, C.c_int(slot), px, pv, C.c_int(f)))

    def step_forward_dev(self, slot, fixed_pts=None):
        p, f = self._tp(fixed_pts, self.B * 3 * self.Af)
        self._chk(self.lib.dc_step_forward_dev(self.h, C.c_int(slot), p, C.c_int(f)))

    def step_backward_dev(self, slot, gx, gv, dx, dv, dxfixed=None, dmu=None, ix=None, iv=None, is_start=False):
        n = self.B * 3 * self.N
        pgx, f = self._tp(gx, n); pgv, _ = self._tp(gv, n); pdx, f3_ = self._tp(dx, n); pdv, _ = self._tp(dv, n)
        pix, _ = self._tp(ix, n); piv, _ = self._tp(iv, n)
        pxf, _ = self._tp(dxfixed, self.B * 3 * self.Af); pmu, _ = self._tp(dmu, self.B * self.ngroups)
        for t in (gv, dx, dv, ix, iv, dxfixed, dmu):
            assert t is None or t.dtype == gx.dtype, "all tensors of a call must have one dtype"
        self._chk(self.lib.dc_step_backward_dev(self.h, C.c_int(slot), pgx, pgv, pix, piv, C.c_int(int(is_start)), pdx, pdv, pxf, pmu, C.c_int(f)))

    # ---- device-resident rollouts ----
    def rollout_forward(self, slot, nsteps):
        self._chk(self.lib.dc_rollout_forward(self.h, C.c_int(slot), C.c_int(nsteps)))

    def seed_gradient(self, slot, target=None, scale=1.0):
        t = None if target is None else _f64(target).reshape(-1)
        self._chk(self.lib.dc_seed_gradient(self.h, C.c_int(slot), _d(t), C.c_double(scale)))

    def set_trajectory_start(self, start_slot):
        """tape slot of the trajectory's initial state (default 0; -1: this tape holds a later segment — no backward step of it is the isStart step)"""
        self._chk(self.lib.dc_set_trajectory_start(self.h, C.c_int(start_slot)))

    def rollout_backward(self, slot, nsteps):
        self._chk(self.lib.dc_rollout_backward(self.h, C.c_int(slot), C.c_int(nsteps)))

    # ---- whole-sweep device-pointer boundary (torch tensors on this GPU; enqueued on the context's stream, nothing synchronises) ----
    def rollout_forward_async(self, slot, nsteps):
        """dc_rollout_forward without the wait (adds nothing to kernel_times; errors of the sweep surface at sync / get_stats)"""
        self._chk(self.lib.dc_rollout_forward_async(self.h, C.c_int(slot), C.c_int(nsteps)))

    def rollout_backward_async(self, slot, nsteps):
        self._chk(self.lib.dc_rollout_backward_async(self.h, C.c_int(slot), C.c_int(nsteps)))

    def set_fixed_point_schedule_dev(self, slot0, nsteps, xf):
        """xf: [nsteps][B][3 Af] targets of the steps slot0+k -> slot0+k+1"""
        (p,), f = self._tps((xf, self.B * 3 * self.Af, nsteps))
        self._chk(self.lib.dc_set_fixed_point_schedule_dev(self.h, C.c_int(slot0), C.c_int(nsteps), p, C.c_int(f)))

    def set_force_schedule_dev(self, slot0, nsteps, fu=None, fv_scale=None):
        (pu, ps), f = self._tps((fu, self.B * 3, nsteps), (fv_scale, self.B, nsteps))
        self._chk(self.lib.dc_set_force_schedule_dev(self.h, C.c_int(slot0), C.c_int(nsteps), pu, ps, C.c_int(f)))

    def set_seed_schedule_dev(self, slot0, nslots, dL_dx=None, dL_dv=None):
        """loss gradient w.r.t. the states at slots slot0 .. slot0+nslots-1, [nslots][B][3 N] each; None = zeros"""
        n = self.B * 3 * self.N
        (px, pv), f = self._tps((dL_dx, n, nslots), (dL_dv, n, nslots))
        self._chk(self.lib.dc_set_seed_schedule_dev(self.h, C.c_int(slot0), C.c_int(nslots), px, pv, C.c_int(f)))

    def set_gradient_dev(self, dL_dx, dL_dv):
        n = self.B * 3 * self.N
        (px, pv), f = self._tps((dL_dx, n, 1), (dL_dv, n, 1))
        self._chk(self.lib.dc_set_gradient_dev(self.h, px, pv, C.c_int(f)))

    def get_gradient_dev(self, dL_dx=None, dL_dv=None, dL_dmu=None):
        n = self.B * 3 * self.N
        (px, pv, pm), f = self._tps((dL_dx, n, 1), (dL_dv, n, 1), (dL_dmu, self.B * self.ngroups, 1))
        self._chk(self.lib.dc_get_gradient_dev(self.h, px, pv, pm, C.c_int(f)))

    def get_states_dev(self, slot0, nslots, x=None, v=None):
        n = self.B * 3 * self.N
        (px, pv), f = self._tps((x, n, nslots), (v, n, nslots))
        self._chk(self.lib.dc_get_states_dev(self.h, C.c_int(slot0), C.c_int(nslots), px, pv, C.c_int(f)))

    def get_dxfixed_dev(self, slot0, nslots, dxfixed):
        (p,), f = self._tps((dxfixed, self.B * 3 * self.Af, nslots))
        self._chk(self.lib.dc_get_dxfixed_dev(self.h, C.c_int(slot0), C.c_int(nslots), p, C.c_int(f)))

    def get_force_schedule_gradients_dev(self, slot0, nslots, dfu=None, dfv_scale=None, dfv=None):
        """gradients w.r.t. the force schedule of the steps through records slot0 .. slot0+nslots-1: dfu [nslots][B][3], dfv_scale
        [nslots][B], dfv [B][3 N] (the last two need keep_force_gradients before the sweep)"""
        (pu, ps, pv), f = self._tps((dfu, self.B * 3, nslots), (dfv_scale, self.B, nslots), (dfv, self.B * 3 * self.N, 1))
        self._chk(self.lib.dc_get_force_schedule_gradients_dev(self.h, C.c_int(slot0), C.c_int(nslots), pu, ps, pv, C.c_int(f)))

    def set_mu_dev(self, mu):
        (p,), f = self._tps((mu, self.B * self.ngroups, 1))
        self._chk(self.lib.dc_set_mu_dev(self.h, p, C.c_int(f)))

    def set_vertex_forces_dev(self, fv):
        (p,), f = self._tps((fv, self.B * 3 * self.N, 1))
        self._chk(self.lib.dc_set_vertex_forces_dev(self.h, p, C.c_int(f)))

    def set_primitive_offsets_dev(self, d):
        """dc_set_primitive_offsets from a CUDA tensor [B][G][3] (a non-contiguous view is copied first); None restores the built centres"""
        self._offsets_dev = d = None if d is None else d.contiguous()      # (kept alive until the next call: the conversion is only enqueued)
        (p,), f = self._tps((d, self.B * self.ngroups * 3, 1))
        self._chk(self.lib.dc_set_primitive_offsets_dev(self.h, p, C.c_int(f)))

    def set_primitive_offset_schedule_dev(self, slot0, nsteps, d):
        """dc_set_primitive_offset_schedule from a CUDA tensor [nsteps][B][G][3] (a non-contiguous view is copied first)"""
        self._offset_schedule_dev = d = d.contiguous()
        (p,), f = self._tps((d, self.B * self.ngroups * 3, nsteps))
        self._chk(self.lib.dc_set_primitive_offset_schedule_dev(self.h, C.c_int(slot0), C.c_int(nsteps), p, C.c_int(f)))

    def set_primitive_velocities_dev(self, w):
        """dc_set_primitive_velocities from a CUDA tensor [B][G][3] (a non-contiguous view is copied first); None = zeros"""
        self._velocities_dev = w = None if w is None else w.contiguous()      # (kept alive until the next call: the conversion is only enqueued)
        (p,), f = self._tps((w, self.B * self.ngroups * 3, 1))
        self._chk(self.lib.dc_set_primitive_velocities_dev(self.h, p, C.c_int(f)))

    def set_primitive_velocity_schedule_dev(self, slot0, nsteps, w):
        """dc_set_primitive_velocity_schedule from a CUDA tensor [nsteps][B][G][3] (a non-contiguous view is copied first)"""
        self._velocity_schedule_dev = w = w.contiguous()
        (p,), f = self._tps((w, self.B * self.ngroups * 3, nsteps))
        self._chk(self.lib.dc_set_primitive_velocity_schedule_dev(self.h, C.c_int(slot0), C.c_int(nsteps), p, C.c_int(f)))

    def set_primitive_shapes_dev(self, s):
        """dc_set_primitive_shapes from a CUDA tensor [B][P][8] (a non-contiguous view is copied first); None restores the built shapes"""
        self._shapes_dev = s = None if s is None else s.contiguous()      # (kept alive until the next call: the conversion is only enqueued)
        (p,), f = self._tps((s, self.B * self.nprims * 8, 1))
        self._chk(self.lib.dc_set_primitive_shapes_dev(self.h, p, C.c_int(f)))

    def set_primitive_shape_schedule_dev(self, slot0, nsteps, s):
        """dc_set_primitive_shape_schedule from a CUDA tensor [nsteps][B][P][8] (a non-contiguous view is copied first)"""
        self._shape_schedule_dev = s = s.contiguous()
        (p,), f = self._tps((s, self.B * self.nprims * 8, nsteps))
        self._chk(self.lib.dc_set_primitive_shape_schedule_dev(self.h, C.c_int(slot0), C.c_int(nsteps), p, C.c_int(f)))

    def get_primitive_velocity_gradients_dev(self, slot0, nslots, dw):
        """dL/dw of the backward steps through records slot0 .. slot0+nslots-1 into a contiguous CUDA tensor [nslots][B][G][3]"""
        (p,), f = self._tps((dw, self.B * self.ngroups * 3, nslots))
        self._chk(self.lib.dc_get_primitive_velocity_gradients_dev(self.h, C.c_int(slot0), C.c_int(nslots), p, C.c_int(f)))

    def set_primitive_spins_dev(self, omega):
        """dc_set_primitive_spins from a CUDA tensor [B][G][3] (a non-contiguous view is copied first); None = zeros"""
        self._spins_dev = omega = None if omega is None else omega.contiguous()      # (kept alive until the next call: the conversion is only enqueued)
        (p,), f = self._tps((omega, self.B * self.ngroups * 3, 1))
        self._chk(self.lib.dc_set_primitive_spins_dev(self.h, p, C.c_int(f)))

    def set_primitive_spin_schedule_dev(self, slot0, nsteps, omega):
        """dc_set_primitive_spin_schedule from a CUDA tensor [nsteps][B][G][3] (a non-contiguous view is copied first)"""
        self._spin_schedule_dev = omega = omega.contiguous()
        (p,), f = self._tps((omega, self.B * self.ngroups * 3, nsteps))
        self._chk(self.lib.dc_set_primitive_spin_schedule_dev(self.h, C.c_int(slot0), C.c_int(nsteps), p, C.c_int(f)))

    def get_primitive_spin_gradients_dev(self, slot0, nslots, dw):
        """dL/domega of the backward steps through records slot0 .. slot0+nslots-1 into a contiguous CUDA tensor [nslots][B][G][3]"""
        (p,), f = self._tps((dw, self.B * self.ngroups * 3, nslots))
        self._chk(self.lib.dc_get_primitive_spin_gradients_dev(self.h, C.c_int(slot0), C.c_int(nslots), p, C.c_int(f)))

    # ---- device-resident schedules (dc_set_*_schedule) ----
    def set_gradient(self, dL_dx, dL_dv):
        n3 = 3 * self.N
        self._chk(self.lib.dc_set_gradient(self.h, _d(self._vec(dL_dx, n3)), _d(self._vec(dL_dv, n3))))

    def set_fixed_point_schedule(self, slot0, xf):
        """xf: [nsteps][B][3 Af] targets of the steps slot0+k -> slot0+k+1"""
        xf = np.ascontiguousarray(np.asarray(xf, dtype=np.float64).reshape(-1, self.B, 3 * self.Af))
        self._chk(self.lib.dc_set_fixed_point_schedule(self.h, C.c_int(slot0), C.c_int(xf.shape[0]), _d(xf)))

    def set_force_schedule(self, slot0, nsteps, fu=None, fv_scale=None):
        fu = None if fu is None else np.ascontiguousarray(np.asarray(fu, dtype=np.float64).reshape(nsteps, self.B, 3))
        fs = None if fv_scale is None else np.ascontiguousarray(np.asarray(fv_scale, dtype=np.float64).reshape(nsteps, self.B))
        self._chk(self.lib.dc_set_force_schedule(self.h, C.c_int(slot0), C.c_int(nsteps), _d(fu), _d(fs)))

    def set_seed_schedule(self, slot0, dL_dx, dL_dv=None):
        """dL_dx: [nslots][B][3 N] loss gradient w.r.t. the state at slot slot0+k"""
        gx = np.ascontiguousarray(np.asarray(dL_dx, dtype=np.float64).reshape(-1, self.B, 3 * self.N))
        gv = None if dL_dv is None else np.ascontiguousarray(np.asarray(dL_dv, dtype=np.float64).reshape(gx.shape))
        self._chk(self.lib.dc_set_seed_schedule(self.h, C.c_int(slot0), C.c_int(gx.shape[0]), _d(gx), _d(gv)))

    def clear_schedules(self):
        self._chk(self.lib.dc_clear_schedules(self.h))

    def get_states(self, slot0, nslots):
        x = np.zeros((nslots, self.B, 3 * self.N)); v = np.zeros((nslots, self.B, 3 * self.N))
        self._chk(self.lib.dc_get_states(self.h, C.c_int(slot0), C.c_int(nslots), _d(x), _d(v)))
        return x, v

    def get_dxfixed(self, slot0, nslots):
        out = np.zeros((nslots, self.B, max(3 * self.Af, 1)))
        if self.Af > 0:
            out = np.zeros((nslots, self.B, 3 * self.Af))
            self._chk(self.lib.dc_get_dxfixed(self.h, C.c_int(slot0), C.c_int(nslots), _d(out)))
        return out[:, :, :3 * self.Af]

    def get_gradient(self):
        dx = np.zeros((self.B, 3 * self.N)); dv = np.zeros((self.B, 3 * self.N)); dmu = np.zeros((self.B, self.ngroups))
        self._chk(self.lib.dc_get_gradient(self.h, _d(dx), _d(dv), _d(dmu)))
        return dx, dv, dmu

    def get_mu_gradient(self):
        """dL/dmu accumulated by the backward sweep, per rollout and friction group (small copy; waits for the stream)."""
        dmu = np.zeros((self.B, self.ngroups))
        self._chk(self.lib.dc_get_gradient(self.h, None, None, _d(dmu)))
        return dmu

    def get_param_gradients(self, slot):
        out = np.zeros((self.B, 8))
        self._chk(self.lib.dc_get_param_gradients(self.h, C.c_int(slot), _d(out)))
        return dict(dL_dk=out[:, 0:3], dL_ddensity=out[:, 3], sum_dfext=out[:, 4:7])

    def get_stats(self, slot):
        f = (dc_step_stats * self.B)(); b = (dc_bwd_stats * self.B)()
        self._chk(self.lib.dc_get_stats(self.h, C.c_int(slot), f, b))
        return (_stats_to_dict(f, ["converged", "pd_iters", "cg_iters", "prim_contacts", "self_contacts", "last_xdiff", "self_overflow"]),
                _stats_to_dict(b, ["converged", "adjoint_iters", "cg_iters", "clipped", "used_direct", "last_udiff", "refine_cycles", "fp64_iters", "residual_verified", "workgroups"]))

    def sync(self):
        self._chk(self.lib.dc_sync(self.h))

    # ---- RCCL collective of the C-ABI (C++ callers; Python callers normally use torch.distributed) ----
    @staticmethod
    def comm_unique_id():
        lib = load_library()
        buf = C.create_string_buffer(128)
        rc = lib.dc_comm_unique_id(buf)
        if rc != 0:
            raise DcError(f"code {rc}: dc_comm_unique_id failed (RCCL not available?)")
        return buf.raw

    def comm_init(self, nranks, rank, unique_id):
        self._chk(self.lib.dc_comm_init(self.h, C.c_int(nranks), C.c_int(rank), C.c_char_p(unique_id)))

    def allreduce_sum(self, values):
        a = np.ascontiguousarray(np.asarray(values, dtype=np.float64).reshape(-1)).copy()
        self._chk(self.lib.dc_allreduce_sum(self.h, _d(a), C.c_int(a.size)))
        return a

    def comm_destroy(self):
        self._chk(self.lib.dc_comm_destroy(self.h))

    def layout(self):
        """which kernel set dc_build chose (dc_get_layout)"""
        c = _i32(np.zeros(6))
        self._chk(self.lib.dc_get_layout(self.h, _i(c)))
        return dict(renumbered=bool(c[0]), bandwidth=int(c[1]), packet_kernel=bool(c[2]), element_windows=bool(c[3]), windows=int(c[4]), dense_inverse=bool(c[5]))

    def packet_byte_offsets(self):
        """True when dc_build laid the packet matrix out with byte offsets (dc_get_packet_layout; DC_PK_OFS=0 keeps the column deltas)"""
        k = C.c_int()
        self._chk(self.lib.dc_get_packet_layout(self.h, C.byref(k)))
        return bool(k.value)

    def packet_layout(self):
        """0 = column deltas (or no packet matrix), 1 = byte offsets, 2 = values only under a matrix-wide column-offset template
        (dc_get_packet_layout; DC_PK_TPL=0 keeps the byte offsets)"""
        k = C.c_int()
        self._chk(self.lib.dc_get_packet_layout(self.h, C.byref(k)))
        return int(k.value)

    def bend_rows(self):
        """True when dc_build turned the bending term into per-vertex matrix rows (dc_get_bend_rows; a mesh flat at rest, DC_BEND_ROWS=0 keeps the flaps)"""
        k = C.c_int()
        self._chk(self.lib.dc_get_bend_rows(self.h, C.byref(k)))
        return bool(k.value)

    def deflation(self):
        """(vectors, probe iterations): the deflation space dc_build chose for the forward solve (dc_get_deflation)"""
        k = C.c_int(); pi = C.c_int()
        self._chk(self.lib.dc_get_deflation(self.h, C.byref(k), C.byref(pi)))
        return k.value, pi.value

    def cluster(self):
        """workgroups per rollout the engine chose for this batch (dc_get_cluster); 1 = one workgroup per rollout"""
        k = C.c_int(); nb = C.c_int()
        self._chk(self.lib.dc_get_cluster(self.h, C.byref(k), C.byref(nb)))
        return k.value

    def cluster_rows(self):
        """(rows per part, halo rows) of the split (dc_get_cluster_rows): part p owns device rows [p R, (p + 1) R); (0, 0) without a split"""
        r = C.c_int(); hb = C.c_int()
        self._chk(self.lib.dc_get_cluster_rows(self.h, C.byref(r), C.byref(hb)))
        return r.value, hb.value

    def self_friction_path(self, reset=False):
        """[B, 2] per rollout since alloc_batch (or the last reset): PD iterations of the split forward kernel that ran a layered self-friction pass, and
        those of them in which every part evaluated the layers itself (dc_get_self_friction_path); zeros with one workgroup per rollout"""
        out = np.zeros((self.B, 2), dtype=np.int32)
        self._chk(self.lib.dc_get_self_friction_path(self.h, _i(out), C.c_int(int(reset))))
        return out

    def adjoint_contact_path(self, reset=False):
        """[B, 2] per rollout since alloc_batch (or the last reset): backward steps run by an adjoint instance that can hold the step's contact
        tables in LDS, and those of them that used the tables (dc_get_adjoint_contact_path); zeros for every other instance"""
        out = np.zeros((self.B, 2), dtype=np.int32)
        self._chk(self.lib.dc_get_adjoint_contact_path(self.h, _i(out), C.c_int(int(reset))))
        return out

    def timer_start(self):
        self._chk(self.lib.dc_timer_start(self.h))

    def timer_stop(self):
        ms = C.c_float()
        self._chk(self.lib.dc_timer_stop(self.h, C.byref(ms)))
        return ms.value

    def adjoint_matrix(self, slot, rollout):
        """K = P - dP^T of record `slot`, rollout `rollout`, as the dense adjoint solve assembles it (dc_get_adjoint_matrix): (3N, 3N) float64,
        xyz interleaved in the caller's numbering"""
        n = 3 * self.N
        K = np.zeros((n, n))
        self._chk(self.lib.dc_get_adjoint_matrix(self.h, C.c_int(slot), C.c_int(rollout), _d(K)))
        return K

    def set_adjoint_band(self, extra_vertices):
        """adjoint_mode 3: vertices added to the matrix bandwidth for self contacts that couple outside it (dc_set_adjoint_band)"""
        self._chk(self.lib.dc_set_adjoint_band(self.h, C.c_int(int(extra_vertices))))

    def adjoint_band(self):
        """what adjoint_mode 3 would use for the built system (dc_get_adjoint_band; host-only contexts too): kl (= ku), ldab and the bytes of
        band storage per rollout"""
        kl = C.c_int(); ldab = C.c_int(); nbytes = C.c_longlong()
        self._chk(self.lib.dc_get_adjoint_band(self.h, C.byref(kl), C.byref(ldab), C.byref(nbytes)))
        return dict(kl=kl.value, ldab=ldab.value, bytes_per_rollout=nbytes.value)

    def dense_phase_times(self, reset=False):
        """device ms of the mode-2 / mode-3 backward steps: (assembly, factorisation, solve); only with DC_DENSE_TIMES=1 (dc_dense_phase_times)"""
        ms = (C.c_float * 3)()
        self._chk(self.lib.dc_dense_phase_times(self.h, ms, C.c_int(int(reset))))
        return tuple(float(v) for v in ms)

    def kernel_times(self, reset=False):
        a = C.c_float(); b = C.c_float(); na = C.c_int(); nb = C.c_int()
        self._chk(self.lib.dc_kernel_times(self.h, C.byref(a), C.byref(na), C.byref(b), C.byref(nb), C.c_int(int(reset))))
        return dict(fwd_ms=a.value, fwd_launches=na.value, bwd_ms=b.value, bwd_launches=nb.value)
