"""Batched counterpart of the reference's `pySim/functional.py` (SimFunction, src/python_code/pySim/functional.py:18-106):
a `torch.autograd.Function` that advances B independent rollouts by one time step on the GPU and back-propagates through
it — the building block of the controller training loops (hatController.py) for a whole batch of rollouts at once.

The reference's function wraps ONE `diffcloth_py.Simulation` (stepNN / stepBackwardNN) and is called once per rollout and
step; here `x`, `v`, `a` carry a leading batch dimension and the step runs through the C-ABI of libdiffcloth_hip.so
(`diffcloth_amd.capi.Engine`). Behaviours kept from the reference function:
  * teacher forcing: the state given to `forward` replaces the stored one (stepNN, Simulation.cpp:1020-1042);
  * the step that reaches `step_num` back-propagates with zero incoming gradients and the loss gradient passed as
    dL_dxinit / dL_dvinit (functional.py:66-75) — for that step the adjoint is the identity;
  * the gradient w.r.t. the action (fixed-point targets) is rescaled to a norm within [0.05, 4 * dim] per rollout
    (functional.py:88-97).
`sim_rollout` is the whole-episode counterpart for open-loop problems (trajectory optimisation over clip targets, identification of mu
or wind, any loss over all frames): one fused forward sweep and one fused backward sweep per evaluation, schedules and results crossing
the boundary as device pointers (the whole-sweep dc_*_dev calls). Closed-loop controllers, whose action depends on the state of every
step, stay on `sim_step`.
CUDA tensors (fp32 or fp64) never leave the GPU: states, actions and gradients cross the boundary as device pointers
(dc_*_dev of include/diffcloth_hip.h), the step is enqueued on torch's current stream and nothing synchronises — the
reference copies every tensor through numpy on the host (functional.py:30-34, 60-64), which for B = 256 rollouts of 10 000
vertices is 246 MB over PCIe per step. CPU tensors still take the host path (float64 arrays, as in the reference).
"""
import numpy as np
import torch


class BatchedSim:
    """B rollouts of one scene on one GPU: a `capi.Engine` with an allocated batch, the step counter of the episode and
    the episode length `step_num` (sceneConfig.stepNum of the reference)."""

    def __init__(self, engine, step_num, strict=False):
        """strict: an adjoint solve that did not converge raises at the end of the episode's backward sweep. Off by default: the reference
        does not stop on non-convergence (it prints and goes on, Simulation.cpp:1589-1600) and controller loops that tolerate an occasional
        unconverged step keep running — they get ONE warning per episode instead, with the number of unconverged (step, rollout) pairs and the worst residual
        (also left in `self.unconverged`, so a training loop can act on it without parsing warnings). Hard errors (a timed-out exchange of the split kernels, a
        self-contact list overflow) always raise."""
        if engine.B <= 0:
            raise ValueError("the engine needs alloc_batch(B, tape) before it is wrapped (tape >= the steps of an episode)")
        self.engine = engine
        self.step_num = int(step_num)
        self.step_idx = 0
        self._stream = None
        self._bwd_slots = set()
        self.strict = bool(strict)
        self.unconverged = 0
        self._episode = 0              # counts sim_rollout episodes: a backward pass must find the tape of ITS forward pass

    def on_current_stream(self, device=None):
        """order the engine's work with torch's current CUDA stream of the tensors' device (once per stream change). torch's default
        stream has handle 0, which dc_use_stream reads as "the context's own stream": ordering with torch's kernels on the legacy
        default stream then rests on its implicit synchronisation with blocking streams (the context's stream is a blocking one)."""
        st = torch.cuda.current_stream(device)
        if self._stream is None or self._stream.cuda_stream != st.cuda_stream:
            self.engine.use_stream(st)
            self._stream = st

    def check_episode(self):
        """Surface engine errors of the episode so far: the device-pointer calls (dc_*_dev) only enqueue work and report nothing, so a
        timed-out exchange of the split kernels (sticky error word) or a self-contact list overflow would otherwise flow into the optimiser as
        garbage states / gradients. One synchronisation + the statistics of the recorded steps; called at the end of an episode's backward
        sweep (slot 1, host and device path alike) and by reset(). Raises capi.DcError; an adjoint solve that did not converge raises
        RuntimeError when `strict`, else warns once per episode (the reference goes on as well)."""
        import warnings
        e = self.engine
        e.sync()                                     # raises on a timed-out exchange
        bad_pairs, worst, first, worst_at = 0, -1.0, None, None
        for slot in range(1, self.step_idx + 1):
            fwd, bwd = e.get_stats(slot)             # raises DC_ERR_CAPACITY on a self-contact overflow of that step
            if slot in self._bwd_slots and (bwd["converged"] == 0).any():
                bad = np.nonzero(bwd["converged"] == 0)[0]
                bad_pairs += len(bad)
                # a non-finite residual (a diverged solve) is the worst there is
                res = np.asarray(bwd["last_udiff"], dtype=np.float64)[bad]
                res = np.where(np.isfinite(res), res, np.inf)
                w = int(bad[np.argmax(res)])
                if first is None:
                    first = (slot, int(bad[0]))
                if worst_at is None or res.max() > worst:
                    worst, worst_at = float(res.max()), (slot, w)
        self.unconverged = bad_pairs                 # (step, rollout) pairs of the episode whose adjoint solve did not converge
        if bad_pairs:
            msg = (f"BatchedSim: {bad_pairs} adjoint solve(s) of this episode did not converge (first: step {first[0]}, rollout {first[1]}; "
                   f"worst relative residual {worst:.2e} at step {worst_at[0]}, rollout {worst_at[1]}): the gradients of those rollouts are not converged")
            if self.strict:
                raise RuntimeError(msg)
            warnings.warn(msg, RuntimeWarning, stacklevel=2)

    def contact_readout(self, slot0=1, nslots=None, dtype=torch.float32, state=True, normal_impulse=True, wrench=True):
        """What the obstacles feel in the steps of this episode (dc_get_contact_readout_dev): CUDA tensors of the records slot0 ..
        slot0 + nslots - 1 (nslots None: up to the last step taken), formed on the engine's GPU on torch's current stream, without a
        synchronisation. Usable after sim_step and after a sim_rollout forward pass.
          state           int32 [nslots, B, N]: 0 not in primitive contact, 1 take-off, 2 stick, 3 slide
          normal_impulse  [nslots, B, N]: r_p . n of the primitive part of the contact response
          wrench          [nslots, B, G, 10] per primitive group: J[3] = -sum r_p (momentum handed to the obstacle in the step; J / time_step is
                          the mean force), tau[3] about the centre of the group's first primitive in that step, sum of the normal impulses,
                          take-off / stick / slide counts
        An output switched off (or, for wrench, a scene without primitives) is None. The outputs carry NO gradient (requires_grad is False):
        they are observations, not differentiable functions of the inputs."""
        e = self.engine
        slot0 = int(slot0)
        if slot0 < 1:
            raise ValueError("contact_readout: slot 0 has no record (slot0 >= 1)")
        if nslots is None:
            nslots = self.step_idx - slot0 + 1
        nslots = int(nslots)
        if nslots < 1 or slot0 + nslots - 1 > self.step_idx:
            raise ValueError(f"contact_readout: records {slot0} .. {slot0 + nslots - 1} asked for, the episode has taken {self.step_idx} step(s)")
        if dtype not in (torch.float32, torch.float64):
            raise ValueError("contact_readout: dtype must be torch.float32 or torch.float64")
        wrench = bool(wrench) and e.ngroups > 0
        if not (state or normal_impulse or wrench):
            raise ValueError("contact_readout: nothing asked for")
        dev = torch.device("cuda", e.device)
        self.on_current_stream(dev)
        s = torch.empty((nslots, e.B, e.N), dtype=torch.int32, device=dev) if state else None
        j = torch.empty((nslots, e.B, e.N), dtype=dtype, device=dev) if normal_impulse else None
        w = torch.empty((nslots, e.B, e.ngroups, 10), dtype=dtype, device=dev) if wrench else None
        e.contact_readout_dev(slot0, nslots, s, j, w)
        return dict(state=s, normal_impulse=j, wrench=w)

    def self_contact_readout(self, slot0=1, nslots=None, cap=None, dtype=torch.float32, pairs=True, impulse=True, vertex_impulse=True, totals=True):
        """What the cloth's sheets press on each other with in the steps of this episode (dc_get_self_contact_readout_dev): CUDA tensors of the
        records slot0 .. slot0 + nslots - 1 (nslots None: up to the last step taken), formed on the engine's GPU on torch's current stream,
        without a synchronisation. Usable after sim_step and after a sim_rollout forward pass.
          pairs           int32 [nslots, B, cap, 4]: {id1, id2, layer, state} per self contact in the order of Engine.get_self_contacts; state 1
                          take-off, 2 stick, 3 slide; {-1, -1, -1, 0} behind the list. cap None: the engine's max_self_contacts
          impulse         [nslots, B, cap, 4]: {r_k (x, y, z), jn_k = r_k . n_k}; r_k acts on id1, -r_k on id2
          vertex_impulse  [nslots, B, N, 3]: the sum of the +-r_k of the pairs a vertex is in, 0 elsewhere
          totals          [nslots, B, 8]: contacts, layers, distinct vertices, sum jn, sum |r_k - jn_k n_k|, take-off / stick / slide counts
        An output switched off is None. The outputs carry NO gradient (requires_grad is False): they are observations."""
        e = self.engine
        slot0 = int(slot0)
        if slot0 < 1:
            raise ValueError("self_contact_readout: slot 0 has no record (slot0 >= 1)")
        if nslots is None:
            nslots = self.step_idx - slot0 + 1
        nslots = int(nslots)
        if nslots < 1 or slot0 + nslots - 1 > self.step_idx:
            raise ValueError(f"self_contact_readout: records {slot0} .. {slot0 + nslots - 1} asked for, the episode has taken {self.step_idx} step(s)")
        if dtype not in (torch.float32, torch.float64):
            raise ValueError("self_contact_readout: dtype must be torch.float32 or torch.float64")
        if not (pairs or impulse or vertex_impulse or totals):
            raise ValueError("self_contact_readout: nothing asked for")
        cap = e.max_self_contacts if cap is None else int(cap)
        if (pairs or impulse) and cap < 1:
            raise ValueError("self_contact_readout: cap must be >= 1 where pairs or impulse is asked for")
        dev = torch.device("cuda", e.device)
        self.on_current_stream(dev)
        p = torch.empty((nslots, e.B, cap, 4), dtype=torch.int32, device=dev) if pairs else None
        r = torch.empty((nslots, e.B, cap, 4), dtype=dtype, device=dev) if impulse else None
        v = torch.empty((nslots, e.B, e.N, 3), dtype=dtype, device=dev) if vertex_impulse else None
        t = torch.empty((nslots, e.B, 8), dtype=dtype, device=dev) if totals else None
        e.self_contact_readout_dev(slot0, nslots, cap, p, r, v, t)
        return dict(pairs=p, impulse=r, vertex_impulse=v, totals=t)

    def reset(self, x0, v0=None):
        """Start a new episode from the given states ([B, 3N]); returns them as float32 tensors like getStateInfo()."""
        if self.step_idx > 0:
            self.check_episode()
        self._bwd_slots = set()
        x0 = np.asarray(x0, dtype=np.float64).reshape(self.engine.B, -1)
        v0 = np.zeros_like(x0) if v0 is None else np.asarray(v0, dtype=np.float64).reshape(self.engine.B, -1)
        self.engine.set_state(0, x0, v0)
        self.step_idx = 0
        return torch.as_tensor(x0).float(), torch.as_tensor(v0).float()


class BatchedSimFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, v, a, sim):
        e = sim.engine
        slot = sim.step_idx
        if slot >= e.tape:
            raise RuntimeError("BatchedSimFunction: tape exhausted, call BatchedSim.reset()")
        ctx.sim = sim
        ctx.slot = slot + 1
        if x.is_cuda:           # device path: pointers in, pointers out, torch's stream
            sim.on_current_stream(x.device)
            xd, vd = x.detach().contiguous(), v.detach().to(x.dtype).contiguous()
            e.set_state_dev(slot, xd, vd)
            e.step_forward_dev(slot, None if e.Af == 0 else a.detach().to(x.dtype).contiguous())
            xn, vn = torch.empty_like(xd), torch.empty_like(vd)
            e.get_state_dev(slot + 1, xn, vn)
            sim.step_idx = slot + 1            # (only once the step is enqueued: a raised error leaves the tape index where it was)
            return xn, vn
        e.set_state(slot, np.float64(x.contiguous().detach().numpy()), np.float64(v.contiguous().detach().numpy()))
        act = None if e.Af == 0 else np.float64(a.contiguous().detach().numpy())
        e.step_forward(slot, fixed_pts=act, want_stats=False)
        xn, vn = e.get_state(slot + 1)
        sim.step_idx = slot + 1
        return torch.as_tensor(xn).to(x.dtype), torch.as_tensor(vn).to(v.dtype)

    @staticmethod
    def backward(ctx, dL_dx_next, dL_dv_next):
        sim, slot = ctx.sim, ctx.slot
        e = sim.engine
        last = slot == sim.step_num            # functional.py:66-75
        sim._bwd_slots.add(slot)
        if dL_dx_next.is_cuda:
            sim.on_current_stream(dL_dx_next.device)
            gx = dL_dx_next.detach().contiguous(); gv = dL_dv_next.detach().to(gx.dtype).contiguous()
            dx, dv = torch.empty_like(gx), torch.empty_like(gx)
            da = torch.zeros((e.B, max(3 * e.Af, 1)), dtype=gx.dtype, device=gx.device)[:, :3 * e.Af].contiguous()
            zero = torch.zeros_like(gx) if last else None
            if last:
                e.step_backward_dev(slot, zero, zero, dx, dv, dxfixed=da if e.Af else None, ix=gx, iv=gv, is_start=(slot == 1))
            else:
                e.step_backward_dev(slot, gx, gv, dx, dv, dxfixed=da if e.Af else None, is_start=(slot == 1))
            if e.Af:                           # functional.py:88-97, per rollout, on the device
                n = da.norm(dim=1, keepdim=True)
                scale = torch.where(n > 1e-7, n.clamp(min=0.05, max=4.0 * da.shape[1]) / n.clamp(min=1e-30), torch.ones_like(n))
                da = da * scale
            if slot == 1:
                sim.check_episode()            # end of the episode's backward sweep: one synchronisation, errors surface here
            return dx, dv, da, None
        gx = np.float64(dL_dx_next.contiguous().detach().numpy())
        gv = np.float64(dL_dv_next.contiguous().detach().numpy())
        if last:
            out = e.step_backward(slot, np.zeros_like(gx), np.zeros_like(gv), dL_dxinit=gx, dL_dvinit=gv, is_start=(slot == 1))
        else:
            out = e.step_backward(slot, gx, gv, is_start=(slot == 1))
        if slot == 1:
            sim.check_episode()                # (the host path checks where the device path does)
        da = out["dL_dxfixed"].copy()
        for b in range(da.shape[0]):        # functional.py:88-97, per rollout
            n = np.linalg.norm(da[b])
            if n > 1e-7:
                da[b] *= max(min(da.shape[1] * 4.0, n), 0.05) / n
        dt = dL_dx_next.dtype
        return torch.as_tensor(out["dL_dx"]).to(dt), torch.as_tensor(out["dL_dv"]).to(dt), torch.as_tensor(da).to(dt), None


def sim_step(sim, x, v, a):
    """One differentiable time step of all rollouts: (x', v') = step(x, v; a). x, v: [B, 3N]; a: [B, 3 Af] clip targets.
    CUDA tensors stay on the GPU (device-pointer boundary); CPU tensors go through the host path."""
    return BatchedSimFunction.apply(x, v, a, sim)


# ---- a whole episode as ONE differentiable function ------------------------------------------------------------------------------
_ROLLOUT_INPUTS = ("x0", "v0", "actions", "uniform_force", "vertex_force_scale", "vertex_forces", "mu")


def _rollout_steps(sim, steps, x0, v0, actions, uniform_force, vertex_force_scale, vertex_forces, mu, primitive_offsets=None, primitive_velocities=None,
                   primitive_shapes=None, primitive_spins=None):
    """Checks the arguments of sim_rollout against the engine's sizes and returns the episode length T. Touches no device."""
    e = sim.engine
    B, N, Af, G = e.B, e.N, e.Af, e.ngroups
    given = dict(zip(_ROLLOUT_INPUTS, (x0, v0, actions, uniform_force, vertex_force_scale, vertex_forces, mu)))
    given["primitive_offsets"] = primitive_offsets
    given["primitive_velocities"] = primitive_velocities
    given["primitive_shapes"] = primitive_shapes
    given["primitive_spins"] = primitive_spins
    if torch.is_tensor(primitive_offsets) and primitive_offsets.requires_grad:
        raise ValueError("sim_rollout: primitive_offsets requires grad, but there is no gradient with respect to an obstacle's centre: the adjoint "
                         "holds the contact normals of the record constant, as the reference's does. Pass primitive_offsets.detach()")
    if torch.is_tensor(primitive_shapes) and primitive_shapes.requires_grad:
        raise ValueError("sim_rollout: primitive_shapes requires grad, but there is no gradient with respect to an obstacle's shape: the adjoint "
                         "holds the normals and the contact set of the record constant and does not see an obstacle's shape at all. "
                         "Pass primitive_shapes.detach()")
    if x0 is None or v0 is None:
        raise ValueError("sim_rollout: x0 and v0 are required")
    for name, t in given.items():
        if t is None:
            continue
        if not torch.is_tensor(t):
            raise ValueError(f"sim_rollout: {name} must be a torch tensor")
        if t.dtype != x0.dtype:
            raise ValueError(f"sim_rollout: mixed dtypes: {name} is {t.dtype}, x0 is {x0.dtype}")
        if t.device != x0.device:
            raise ValueError(f"sim_rollout: mixed devices: {name} is on {t.device}, x0 on {x0.device}")
    if x0.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"sim_rollout: float32 or float64 tensors, got {x0.dtype}")
    if x0.is_cuda and getattr(e, "device", None) is not None and x0.device.index != e.device:
        raise ValueError(f"sim_rollout: tensors on {x0.device}, the engine runs on device {e.device}")
    if actions is not None and Af == 0:
        raise ValueError("sim_rollout: actions given, but the scene has no attached vertices (Af == 0)")
    if vertex_force_scale is not None and vertex_forces is None:
        raise ValueError("sim_rollout: vertex_force_scale given without vertex_forces (the field the factors apply to)")
    T = None
    for name in ("actions", "uniform_force", "vertex_force_scale"):
        if given[name] is not None and given[name].dim() > 0:
            T = int(given[name].shape[0])
            break
    for name in ("primitive_offsets", "primitive_velocities"):
        if T is None and given[name] is not None and given[name].dim() == 4:
            T = int(given[name].shape[0])
    if T is None and primitive_shapes is not None and primitive_shapes.dim() == 4:
        T = int(primitive_shapes.shape[0])
    if T is None and primitive_spins is not None and primitive_spins.dim() == 4:
        T = int(primitive_spins.shape[0])
    if T is None:
        if steps is None:
            raise ValueError("sim_rollout: no schedule given, pass steps=")
        T = int(steps)
    elif steps is not None and int(steps) != T:
        raise ValueError(f"sim_rollout: steps = {steps}, but the first schedule has {T} steps")
    if T < 1:
        raise ValueError("sim_rollout: an episode has at least one step")
    want = dict(x0=(B, 3 * N), v0=(B, 3 * N), actions=(T, B, 3 * Af), uniform_force=(T, B, 3), vertex_force_scale=(T, B),
                vertex_forces=(B, 3 * N), mu=(B, G))
    for name, t in given.items():
        if name in ("primitive_offsets", "primitive_velocities", "primitive_spins"):
            if t is not None and tuple(t.shape) not in ((T, B, G, 3), (B, G, 3)):
                raise ValueError(f"sim_rollout: wrong shape: {name} is {tuple(t.shape)}, expected {(T, B, G, 3)} (one per step) or {(B, G, 3)}")
        elif name == "primitive_shapes":
            if t is not None:
                P = e.nprims       # (read only when the argument is given: an engine without the attribute still runs every other episode)
                if tuple(t.shape) not in ((T, B, P, 8), (B, P, 8)):
                    raise ValueError(f"sim_rollout: wrong shape: {name} is {tuple(t.shape)}, expected {(T, B, P, 8)} (one per step) or {(B, P, 8)}")
        elif t is not None and tuple(t.shape) != want[name]:
            raise ValueError(f"sim_rollout: wrong shape: {name} is {tuple(t.shape)}, expected {want[name]}")
    if T > e.tape:
        raise RuntimeError(f"sim_rollout: an episode of {T} steps needs tape slots 0 .. {T}, the batch was allocated with tape = {e.tape}")
    return T


def _np64(t):
    return None if t is None else t.detach().double().contiguous().numpy()


class RolloutFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sim, T, x0, v0, actions, uniform_force, vertex_force_scale, vertex_forces, mu, primitive_offsets=None, primitive_velocities=None,
                primitive_shapes=None, primitive_spins=None, contact_readout=False):
        e = sim.engine
        B, N = e.B, e.N
        ctx.contact_readout = bool(contact_readout)
        if primitive_offsets is not None and primitive_offsets.dim() == 3:      # constant over the episode: the same entry in every step
            primitive_offsets = primitive_offsets.detach().unsqueeze(0).expand(T, *primitive_offsets.shape)
        ctx.velocities_per_episode = primitive_velocities is not None and primitive_velocities.dim() == 3      # (its gradient: summed over the steps)
        if ctx.velocities_per_episode:
            primitive_velocities = primitive_velocities.detach().unsqueeze(0).expand(T, *primitive_velocities.shape)
        if primitive_shapes is not None and primitive_shapes.dim() == 3:
            primitive_shapes = primitive_shapes.detach().unsqueeze(0).expand(T, *primitive_shapes.shape)
        ctx.spins_per_episode = primitive_spins is not None and primitive_spins.dim() == 3      # (its gradient: summed over the steps)
        if ctx.spins_per_episode:
            primitive_spins = primitive_spins.detach().unsqueeze(0).expand(T, *primitive_spins.shape)
        sim._episode += 1
        ctx.sim, ctx.T, ctx.episode = sim, T, sim._episode
        ctx.save_for_backward(vertex_forces, vertex_force_scale)
        sim._bwd_slots = set()
        if x0.is_cuda:          # device path: every array of the episode crosses as a device pointer, on torch's stream
            sim.on_current_stream(x0.device)
            c = lambda t: None if t is None else t.detach().contiguous()
            e.set_trajectory_start(0)
            e.clear_schedules()
            e.set_state_dev(0, c(x0), c(v0))
            if mu is not None:
                e.set_mu_dev(c(mu))
            if vertex_forces is not None:
                e.set_vertex_forces_dev(c(vertex_forces))
            if actions is not None:
                e.set_fixed_point_schedule_dev(0, T, c(actions))
            if uniform_force is not None or vertex_force_scale is not None:
                e.set_force_schedule_dev(0, T, fu=c(uniform_force), fv_scale=c(vertex_force_scale))
            if primitive_offsets is not None:
                e.set_primitive_offset_schedule_dev(0, T, primitive_offsets.detach())
            if primitive_velocities is not None:
                e.set_primitive_velocity_schedule_dev(0, T, primitive_velocities.detach())
            if primitive_shapes is not None:
                e.set_primitive_shape_schedule_dev(0, T, primitive_shapes.detach())
            if primitive_spins is not None:
                e.set_primitive_spin_schedule_dev(0, T, primitive_spins.detach())
            e.rollout_forward_async(0, T)
            xs = torch.empty((T, B, 3 * N), dtype=x0.dtype, device=x0.device)
            vs = torch.empty_like(xs)
            e.get_states_dev(1, T, xs, vs)
            sim.step_idx = T
            if ctx.contact_readout:
                jn = torch.empty((T, B, N), dtype=x0.dtype, device=x0.device)
                wr = torch.empty((T, B, e.ngroups, 10), dtype=x0.dtype, device=x0.device)
                e.contact_readout_dev(1, T, None, jn, wr)
                return xs, vs, jn, wr
            return xs, vs
        e.set_trajectory_start(0)
        e.clear_schedules()
        e.set_state(0, _np64(x0), _np64(v0))
        if mu is not None:
            e.set_mu(_np64(mu))
        if vertex_forces is not None:
            e.set_vertex_forces(_np64(vertex_forces))
        if actions is not None:
            e.set_fixed_point_schedule(0, _np64(actions))
        if uniform_force is not None or vertex_force_scale is not None:
            e.set_force_schedule(0, T, fu=_np64(uniform_force), fv_scale=_np64(vertex_force_scale))
        if primitive_offsets is not None:
            e.set_primitive_offset_schedule(0, _np64(primitive_offsets))
        if primitive_velocities is not None:
            e.set_primitive_velocity_schedule(0, _np64(primitive_velocities))
        if primitive_shapes is not None:
            e.set_primitive_shape_schedule(0, _np64(primitive_shapes))
        if primitive_spins is not None:
            e.set_primitive_spin_schedule(0, _np64(primitive_spins))
        e.rollout_forward(0, T)
        xs, vs = e.get_states(1, T)
        sim.step_idx = T
        if ctx.contact_readout:
            ro = e.contact_readout(1, T, state=False)
            return (torch.as_tensor(xs).to(x0.dtype), torch.as_tensor(vs).to(x0.dtype), torch.as_tensor(ro["normal_impulse"]).to(x0.dtype),
                    torch.as_tensor(ro["wrench"]).to(x0.dtype))
        return torch.as_tensor(xs).to(x0.dtype), torch.as_tensor(vs).to(x0.dtype)

    @staticmethod
    def backward(ctx, grad_xs, grad_vs, grad_jn=None, grad_wrench=None):
        sim, T = ctx.sim, ctx.T
        e = sim.engine
        B, N, Af, G = e.B, e.N, e.Af, e.ngroups
        if ctx.episode != sim._episode:
            raise RuntimeError("sim_rollout: the tape holds a later episode; back-propagate an episode before the next sim_rollout on this BatchedSim")
        vertex_forces, vertex_force_scale = ctx.saved_tensors
        _, _, _, _, need_a, need_fu, need_fvs, need_fv, need_mu = ctx.needs_input_grad[:9]
        need_w = len(ctx.needs_input_grad) > 10 and ctx.needs_input_grad[10]
        need_om = len(ctx.needs_input_grad) > 12 and ctx.needs_input_grad[12]
        keep = bool(need_fvs or need_fv)
        sim._bwd_slots.update(range(1, T + 1))
        dt = grad_xs.dtype
        if grad_xs.is_cuda:
            dev = grad_xs.device
            sim.on_current_stream(dev)
            gxs = grad_xs.detach().contiguous(); gvs = grad_vs.detach().to(dt).contiguous()
            e.keep_force_gradients(keep)
            e.set_seed_schedule_dev(0, 1)                                # the loss does not see the initial state: zeros
            if T > 1:
                e.set_seed_schedule_dev(1, T - 1, gxs[:T - 1], gvs[:T - 1])
            e.set_gradient_dev(gxs[T - 1], gvs[T - 1])
            if ctx.contact_readout:        # the loss's gradient w.r.t. the read-out: the sweep adds its part to every gradient it leaves
                e.set_contact_readout_gradients_dev(1, T, grad_jn.detach().to(dt).contiguous(), grad_wrench.detach().to(dt).contiguous())
            try:
                e.rollout_backward_async(T, T)
            finally:
                if ctx.contact_readout:          # (a sweep that raises must not leave the weights on the context)
                    e.set_contact_readout_gradients_dev(1, T, None, None)
            new = lambda *shape: torch.empty(shape, dtype=dt, device=dev)
            dx0, dv0 = new(B, 3 * N), new(B, 3 * N)
            dmu = new(B, G) if need_mu else None
            e.get_gradient_dev(dx0, dv0, dmu)
            da = None
            if need_a:
                da = new(T, B, 3 * Af)
                e.get_dxfixed_dev(1, T, da)
            dfu = new(T, B, 3) if need_fu else None
            dfvs = new(T, B) if need_fvs else None
            dfv = new(B, 3 * N) if need_fv else None
            if need_fu or keep:
                e.get_force_schedule_gradients_dev(1, T, dfu=dfu, dfv_scale=dfvs, dfv=dfv)
            dw = None
            if need_w:
                dw = new(T, B, G, 3)
                e.get_primitive_velocity_gradients_dev(1, T, dw)
                if ctx.velocities_per_episode:
                    dw = dw.sum(0)
            dom = None
            if need_om:
                dom = new(T, B, G, 3)
                e.get_primitive_spin_gradients_dev(1, T, dom)
                if ctx.spins_per_episode:
                    dom = dom.sum(0)
            sim.check_episode()                # the single synchronisation of the episode: errors of both sweeps surface here
            return None, None, dx0, dv0, da, dfu, dfvs, dfv, dmu, None, dw, None, dom, None
        gxs, gvs = _np64(grad_xs), _np64(grad_vs)
        e.keep_force_gradients(keep)
        zero = np.zeros((1, B, 3 * N))
        e.set_seed_schedule(0, np.concatenate([zero, gxs[:T - 1]]), np.concatenate([zero, gvs[:T - 1]]))
        e.set_gradient(gxs[T - 1], gvs[T - 1])
        if ctx.contact_readout:
            e.set_contact_readout_gradients(1, _np64(grad_jn), _np64(grad_wrench))
        try:
            e.rollout_backward(T, T)
        finally:
            if ctx.contact_readout:
                e.set_contact_readout_gradients(1, None, None)
        dx0, dv0, dmu = e.get_gradient()
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dt)
        da = t(e.get_dxfixed(1, T)) if need_a else None
        dfu = t(np.stack([e.get_param_gradients(s)["sum_dfext"] for s in range(1, T + 1)])) if need_fu else None
        dfvs = dfv = None
        if keep:                               # the force-schedule reductions of the host path: numpy, fp64
            y = e.get_force_gradients(1, T)    # h^2 y of every step, [T][B][3 N]
            if need_fvs:
                dfvs = t(np.einsum("kbq,bq->kb", y, _np64(vertex_forces)))
            if need_fv:
                w = np.ones((T, B)) if vertex_force_scale is None else _np64(vertex_force_scale)
                dfv = t(np.einsum("kb,kbq->bq", w, y))
        dw = None
        if need_w:
            dw = e.get_primitive_velocity_gradients(1, T)
            dw = t(dw.sum(0) if ctx.velocities_per_episode else dw)
        dom = None
        if need_om:
            dom = e.get_primitive_spin_gradients(1, T)
            dom = t(dom.sum(0) if ctx.spins_per_episode else dom)
        sim.check_episode()
        return None, None, t(dx0), t(dv0), da, dfu, dfvs, dfv, (t(dmu) if need_mu else None), None, dw, None, dom, None


def sim_rollout(sim, x0, v0, actions=None, *, steps=None, uniform_force=None, vertex_force_scale=None, vertex_forces=None, mu=None,
                primitive_offsets=None, primitive_velocities=None, primitive_shapes=None, primitive_spins=None, contact_readout=False):
    """A whole differentiable episode of all rollouts: the states after every step, (xs, vs), [T, B, 3N] each in the dtype of x0.

    contact_readout=True returns (xs, vs, jn, wrench): the contact read-out of every step as DIFFERENTIABLE outputs, jn [T, B, N] the normal
    impulse per vertex and wrench [T, B, G, 10] the row {J[3], tau[3], sum jn, take-off, stick, slide counts} per primitive group
    (BatchedSim.contact_readout describes them), in the dtype of x0, on the device path and on the host path. A loss on them back-propagates
    to every tensor argument that receives a gradient — x0, v0, actions, the forces, mu, primitive_velocities, primitive_spins: the
    backward pass hands the incoming jn and wrench gradients to Engine.set_contact_readout_gradients[_dev] before the sweep and clears them
    afterwards. The contact set, the normals and the groups' centres are held constant, as everywhere in the adjoint, and the counts
    (entries 7..9) carry no derivative. The default returns (xs, vs) exactly as before. `sim_step` has no such output: the per-step
    function is out of scope for the read-out's gradient (use Engine.set_contact_readout_gradients with Engine.step_backward there).

    x0, v0: [B, 3N] initial state. actions: [T, B, 3 Af] clip targets of every step. uniform_force: [T, B, 3] force on every vertex per
    step. vertex_forces: [B, 3N] per-vertex force field, vertex_force_scale: [T, B] its factor per step (1 when omitted; the field is the
    factor-free one). mu: [B, G] friction coefficient per primitive group. T comes from the first schedule given, or from `steps`.
    Gradients flow to every tensor argument that requires one, except primitive_offsets and primitive_shapes.

    primitive_offsets: [T, B, G, 3] offset of every primitive group's centre per step and rollout, or [B, G, 3] for the whole episode
    (Engine.set_primitive_offset_schedule: the obstacle of group g is tested at fp32(center + offset)). When omitted the schedule is cleared
    like the others and the engine's current offsets (Engine.set_primitive_offsets; none by default) apply. A tensor that requires grad is
    refused: the adjoint holds the contact normals constant, as the reference's does, so no gradient with respect to the centre exists.

    primitive_velocities: [T, B, G, 3] velocity of every primitive group per step and rollout, or [B, G, 3] for the whole episode
    (Engine.set_primitive_velocity_schedule: the friction law sees the momentum relative to the moving obstacle, d = (f - v_rot m) - w m,
    and the detection looks ahead along vel - w). When omitted the schedule is cleared like the others and the engine's current velocities
    (Engine.set_primitive_velocities; none by default) apply. A tensor that requires grad receives dL/dw of every step, summed over the
    steps for the [B, G, 3] form (normals and contact set held constant, as everywhere in the adjoint). The two go together: a caller who
    moves an obstacle along c(t) passes offsets[s] = c(t_s) - c_built and velocities[s] = (c(t_{s+1}) - c(t_s)) / h — the offset is the
    obstacle's position at the start of step s, and it moves by velocities[s] h during the step.

    primitive_shapes: [T, B, P, 8] shape row {top_offset[3], corner2[3], radius, length} of every flattened primitive (Engine.set_primitives
    order) per step and rollout, or [B, P, 8] for the whole episode (Engine.set_primitive_shape_schedule: the kernels read fp32 of these
    numbers in place of the built ones; Engine.built_primitive_shapes() gives the built rows and rotated_primitive_shapes tilts them). When
    omitted the schedule is cleared like the others and the engine's current shapes (Engine.set_primitive_shapes; the built ones by
    default) apply. A tensor that requires grad is refused: the adjoint does not see an obstacle's shape. A shape schedule alone leaves
    the surface static in the friction law; the translation part of a swinging obstacle's motion goes into primitive_velocities.

    primitive_spins: [T, B, G, 3] angular velocity (rad/s) of every primitive group per step and rollout, or [B, G, 3] for the whole
    episode (Engine.set_primitive_spin_schedule: a DC_PRIM_SPHERE of the group adds the surface velocity radius (omega x n) to the
    obstacle's velocity in the friction law, with its built radius; every other kind has no spin term, and a non-zero value for a group
    without a sphere is refused on the host path). When omitted the schedule is cleared like the others and the engine's current spins
    (Engine.set_primitive_spins; none by default) apply. A tensor that requires grad receives dL/domega of every step, summed over the
    steps for the [B, G, 3] form (normals and contact set held constant, as everywhere in the adjoint).

    The episode occupies tape slots 0 .. T (T <= the tape of alloc_batch) and replaces what the tape held: the function sets the trajectory
    start to slot 0, clears the schedules it does not set, and leaves sim.step_idx = T. `mu` and `vertex_forces`, when given, stay set on
    the engine as after Engine.set_mu / set_vertex_forces; when omitted the engine's current values apply, as does its current uniform
    force when there is no uniform_force schedule. An episode is back-propagated before the next sim_rollout on the same BatchedSim.

    CUDA tensors: the state and the schedules are uploaded by the dc_*_dev setters, one fused forward sweep, one conversion of the states of
    slots 1 .. T; backward: the incoming gradients become the seed schedule (slot 0 zeros, slots 1 .. T-1 grad[:-1]) and the carried
    gradient (grad[-1]), one fused backward sweep, every gradient comes back on the device; all on torch's current stream. The only
    synchronisation of the episode is BatchedSim.check_episode at the end of backward. CPU tensors take the host calls (float64 arrays).

    The action gradient is dL_dxfixed of every step as the adjoint gives it: it is NOT rescaled. The clamp of its norm belongs to
    `sim_step`, which mirrors the reference's per-step function (functional.py:88-97)."""
    T = _rollout_steps(sim, steps, x0, v0, actions, uniform_force, vertex_force_scale, vertex_forces, mu, primitive_offsets, primitive_velocities,
                       primitive_shapes, primitive_spins)
    if not isinstance(contact_readout, (bool, np.bool_)):
        raise ValueError(f"sim_rollout: contact_readout must be True or False, got {type(contact_readout).__name__}")
    if contact_readout and sim.engine.nprims < 1:
        raise ValueError("sim_rollout: contact_readout=True, but the scene has no primitive: there is no contact to read out")
    return RolloutFunction.apply(sim, T, x0, v0, actions, uniform_force, vertex_force_scale, vertex_forces, mu, primitive_offsets,
                                 primitive_velocities, primitive_shapes, primitive_spins, bool(contact_readout))


def rotated_primitive_shapes(shapes, R):
    """Shape rows with their vectors rotated: shapes [..., P, 8] = {top_offset[3], corner2[3], radius, length} per flattened primitive, R
    [..., P, 3, 3] rotation matrices (leading dimensions broadcast). Returns rows of the broadcast shape with top_offset and corner2
    replaced by R top_offset and R corner2, computed in the tensors' dtype, radius and length kept. This is how a caller tilts a plane or
    swings a capsule about its centre with sim_rollout(primitive_shapes=...) / Engine.set_primitive_shapes: the kernels do no rotation
    arithmetic, they read the rotated vectors."""
    shapes, R = torch.as_tensor(shapes), torch.as_tensor(R)
    if shapes.shape[-1] != 8 or R.shape[-2:] != (3, 3):
        raise ValueError(f"rotated_primitive_shapes: shapes [..., P, 8] and R [..., P, 3, 3], got {tuple(shapes.shape)} and {tuple(R.shape)}")
    R = R.to(shapes.dtype)
    lead = torch.broadcast_shapes(shapes.shape[:-1], R.shape[:-2])
    shapes = shapes.expand(*lead, 8)
    top = (R @ shapes[..., 0:3].unsqueeze(-1)).squeeze(-1)
    ur = (R @ shapes[..., 3:6].unsqueeze(-1)).squeeze(-1)
    return torch.cat([top, ur, shapes[..., 6:8]], dim=-1)
