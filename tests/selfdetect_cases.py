"""Inputs and the plain fp64 model of the self-contact detection tests, shared by the GPU tests (tests/test_gpu_selfdetect_cases.py,
tests/test_gpu_self_layers.py: the device's self_detect_rollout, csrc/dc_selflib.h) and their CPU companion
(tests/test_selfdetect_companion.py: the model against the oracle, the conditions on the inputs, the liveness of every targeted branch).

The model restates the reference's detection (oracle/orc_sim.cpp::collisionDetection / isSelfCollision) over ALL unconnected vertex pairs,
with no broad phase: a pair (i, j) is a contact when
    min(d0, d1) < r_i + r_j,   d0 = |x_i - x_j|,   d1 = |x_i - x_j + (v_i - v_j) h|           (isSelfCollision)
    d0 <= 1.0                                                                                  (the early-out of the sweep)
    |cell_i - cell_j| < window                                                                 (the 1-D sweep only visits those cells)
where v is the velocity the step hands to the detection (v_n + h g: gravity is the only external force of these cases), cell is the 1-D cell
id along the longest axis of the bounding box (which also holds s_n[0] = x_0 + v_0 h, the reference's particles[0].pos at that point) and
window = ceil(2 maxR / cellDim) + 4.
The reference's third candidate, the distance at tMid = -2 (v . v0) / |v|^2, is left out: with that factor 2 the point v0 + v tMid is the
mirror image of v0 in the plane normal to v, so its length is |v0| = d0 again and the term never changes the minimum.

Each switch of detect_model() turns one term off IN THE MODEL; the companion counts what each one changes, which shows that the cases would
notice the same term missing from the kernel.

layering_model() restates contactSorting (greedy frontier walk over std::map / std::set orders) in plain Python.

Every case is deterministic from the seed listed in CASES; the seeds were picked so that the conditions of check_conditions() hold (about
half of all seeds do; the three cloud_hubs seeds are the first of them with a hub of degree 6, about one seed in fifty): no decision of
the detection sits closer to its threshold than ~100 fp32 ulps, so the fp32 kernel and the fp64 oracle must decide every pair alike.
"""
import numpy as np

import meshes

GRAVITY = np.array([0.0, -9.8, 0.0])
MARGIN = 1e-5                # distance decisions: ~100 fp32 ulps at these magnitudes
AXIS_MARGIN = 1e-3
MIN_D0 = 1e-2                # accepted pairs: the normal (x_i - x_j) / d0 is well conditioned
SPHERE_EPS = 0.1             # Sphere::isInContact: dist < 0.1
MATERIAL = dict(density=0.3, k_stretch=150.0, k_bend=0.05)


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


# ------------------------------------------------------------------------------------------------------------------- the mesh's tables
def radii_of(V, F):
    """min incident edge / 2 - 0.01 (orc_sim.cpp, Simulation.cpp:2407-2431)"""
    r = np.full(len(V), 100.0)
    for a, b in ((0, 1), (1, 2), (2, 0)):
        L = np.linalg.norm(V[F[:, a]] - V[F[:, b]], axis=1)
        np.minimum.at(r, F[:, a], L)
        np.minimum.at(r, F[:, b], L)
    return r / 2.0 - 0.01


def connected_pairs(F):
    """ordered pairs (p, q) of vertices that share a triangle (pointpointConnectionTable), p == q included"""
    p = np.concatenate([F[:, a] for a in range(3) for b in range(3)])
    q = np.concatenate([F[:, b] for a in range(3) for b in range(3)])
    return p, q


# ------------------------------------------------------------------------------------------------------------------- detection model
def detect_model(X, Vel, V, F, h, window_reject=True, use_d1=True, unit_cut=True, rows=384):
    """All pairs, fp64, in row blocks of `rows` vertices (6 241 vertices: ~20 M pairs, ~0.4 GB per block of temporaries).
    X, Vel: [N][3] state; V, F: rest mesh. Returns the accepted pair set and, for every unconnected pair whose swept distance is below
    its threshold (`cand`: whatever the window and the 1.0 cut then do with it), the quantities of the decision."""
    X = np.asarray(X, dtype=np.float64); N = len(X)
    r = radii_of(V, F)
    Vg = np.asarray(Vel, dtype=np.float64) + GRAVITY * h
    p0 = X[0] + Vg[0] * h
    mx = np.maximum(X.max(0), p0); mn = np.minimum(X.min(0), p0); dim = mx - mn
    axis = 0
    for d in (1, 2):
        if dim[d] > dim[axis]:
            axis = d
    maxR = r.max()
    cells_f = dim[axis] / (2 * maxR)
    cellNum = max(min(512, int(cells_f)), 1)
    cellDim = dim[axis] / cellNum
    window = int(np.ceil(2 * maxR / cellDim)) + 4
    cf = (X[:, axis] - mn[axis]) / cellDim
    cell = np.minimum(cf.astype(np.int64), cellNum - 1)
    cp, cq = connected_pairs(F)
    margin_thresh = margin_unit = np.inf
    out = {k: [] for k in ("i", "j", "d0", "d1", "thresh")}
    for a in range(0, N, rows):
        b = min(a + rows, N)
        conn = np.zeros((b - a, N), dtype=bool)
        sel = (cp >= a) & (cp < b)
        conn[cp[sel] - a, cq[sel]] = True
        valid = (np.arange(N)[None, :] > np.arange(a, b)[:, None]) & ~conn
        v0 = X[a:b, None, :] - X[None, :, :]
        d0 = np.sqrt((v0 * v0).sum(-1))
        v0 += (Vg[a:b, None, :] - Vg[None, :, :]) * h
        d1 = np.sqrt((v0 * v0).sum(-1))
        del v0
        th = r[a:b, None] + r[None, :]
        md = np.minimum(d0, d1) if use_d1 else d0
        margin_thresh = min(margin_thresh, np.abs(np.minimum(d0, d1) - th)[valid].min(initial=np.inf))
        margin_unit = min(margin_unit, np.abs(d0 - 1.0)[valid].min(initial=np.inf))
        ii, jj = np.nonzero(valid & (md < th))
        out["i"].append(ii + a); out["j"].append(jj)
        out["d0"].append(d0[ii, jj]); out["d1"].append(d1[ii, jj]); out["thresh"].append(th[ii, jj])
    c = {k: np.concatenate(v) for k, v in out.items()}
    c["cell_i"], c["cell_j"] = cell[c["i"]], cell[c["j"]]
    c["near"] = c["d0"] <= 1.0
    c["inwin"] = np.abs(c["cell_i"] - c["cell_j"]) < window
    acc = np.ones(len(c["i"]), dtype=bool)
    if unit_cut:
        acc &= c["near"]
    if window_reject:
        acc &= c["inwin"]
    c["accepted"] = acc
    pairs = set(zip(c["i"][acc].tolist(), c["j"][acc].tolist()))
    second = max(dim[d] for d in range(3) if d != axis)
    return dict(pairs=pairs, cand=c, axis=axis, dim=dim, cellNum=cellNum, cellDim=cellDim, window=window, cells_f=cells_f, maxR=maxR,
                radii=r, Vg=Vg, margin_thresh=float(margin_thresh), margin_unit=float(margin_unit), margin_axis=float(dim[axis] - second))


def sphere_model(X, Vg, h, center, radius):
    """isInContactWithObstacle for one sphere: the vertex is tested at t = 0, h / 2, h; returns the vertices in contact and the margin"""
    hit = np.zeros(len(X), dtype=bool); margin = np.inf
    for t in (0.0, 0.5, 1.0):
        d = np.linalg.norm(X + Vg * (h * t) - np.asarray(center), axis=1) - radius
        hit |= d < SPHERE_EPS
        margin = min(margin, np.abs(d - SPHERE_EPS).min())
    return set(np.nonzero(hit)[0].tolist()), float(margin)


def kernel_grid_fp64(m, h):
    """The 2-D broad-phase grid of self_detect_rollout restated in fp64: reach_max, the cell size cs and K = ceil(reach_max / cs), next to
    the cell size the same formulas give at rest (vmax = 0)."""
    vmax = np.linalg.norm(m["Vg"], axis=1).max()
    dims = sorted(m["dim"], reverse=True)[:2]
    reach_max = min(2 * m["maxR"] + 2 * vmax * h, 1.0)
    cs = max(reach_max, max(dims) / 64.0)
    cs_rest = max(2 * m["maxR"], max(dims) / 64.0)
    return dict(reach_max=reach_max, cs=cs, K=int(np.ceil(reach_max / cs)), cs_rest=cs_rest, vmax=vmax)


# ------------------------------------------------------------------------------------------------------------------- LDS working set
PK_ROWS_PER_THREAD = (1, 2, 3, 4, 6, 8, 10, 12, 16, 20)      # the default ladder of the packet forward kernel, 512 threads (kPkShapes)


def self_lds_need(M, C, layers):
    """floats the layered self-contact passes need to run in LDS: M distinct vertices, C contacts (self_lds_need, csrc/dc_devlib.h)"""
    return 7 * M + 8 * C + layers + 2


def forward_lds_floats(N):
    """floats the one-workgroup packet forward kernel offers those passes: 3 NP, NP = 512 x the rows per thread of the smallest shape that
    holds N rows (pk_shape_for, csrc/dc_kernelplan.h; the call sites in csrc/dc_forward_pk_kernel.h)"""
    return 3 * 512 * next(v for v in PK_ROWS_PER_THREAD if 512 * v >= N)


def adjoint_lds_floats_at_least(N, windows):
    """a lower bound of what the one-workgroup adjoint offers, the LDS of the element windows: 6 vcap + 3 nrcap floats
    (csrc/dc_windows.cpp). The largest of W windows owns at least N / W vertices, vcap is at least that, and nrcap counts two result
    vectors for every triangle that touches the window — at least a third as many triangles as owned vertices: 8 N / W floats."""
    return 8 * -(-N // windows) if windows >= 1 else 0


# ------------------------------------------------------------------------------------------------------------------- layering model
def layering_model(pairs, prim_vertices=(), neighbours_ascending=True, seed_frontier=True, stats=None):
    """contactSorting: pairs = sorted list of (id1 < id2); returns the layer of every pair. neighbours_ascending=False walks a vertex's
    neighbours in descending order (what a wrong adjacency order of a hub would do); seed_frontier=False ignores the primitive contacts;
    stats (a dict) receives how often the walk restarted from a chain head and from a loop (no vertex of degree 1 left)."""
    pairs = sorted(pairs)
    nb = {}
    for a, b in pairs:
        nb.setdefault(a, set()).add(b); nb.setdefault(b, set()).add(a)
    index = {p: k for k, p in enumerate(pairs)}
    layer = [-1] * len(pairs)

    def remove(a, b):
        nb[a].discard(b); nb[b].discard(a)

    frontier = set(p for p in prim_vertices if nb.get(p)) if seed_frontier else set()
    done = 0
    for pid in sorted(nb):
        if len(nb[pid]) != 1:
            continue
        other = next(iter(nb[pid]))
        if len(nb[other]) != 1 or pid in frontier or other in frontier:
            continue
        layer[index[(min(pid, other), max(pid, other))]] = 0
        remove(pid, other); done += 1
    current = 1
    while done != len(pairs):
        while frontier:
            new, involved = set(), set()
            for pid in sorted(frontier):
                if not nb[pid] or pid in involved:
                    continue
                for other in sorted(nb[pid], reverse=not neighbours_ascending):
                    if other in involved:
                        continue
                    layer[index[(min(pid, other), max(pid, other))]] = current
                    remove(pid, other); done += 1
                    involved.update((pid, other))
                    if nb[other]:
                        new.add(other)
                    break
            current += 1
            frontier = new
        if done != len(pairs):
            live = [p for p in sorted(nb) if nb[p]]
            heads = [p for p in live if len(nb[p]) == 1]
            frontier = {heads[0] if heads else live[0]}
            if stats is not None:
                key = "head_picks" if heads else "loop_picks"
                stats[key] = stats.get(key, 0) + 1
    return dict(zip(pairs, layer))


def graph_stats(pairs, N):
    """max degree and the number of independent cycles (edges - vertices + components) of the contact graph"""
    pairs = sorted(pairs)
    deg = np.zeros(N, dtype=int)
    parent = list(range(N))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]; a = parent[a]
        return a
    for a, b in pairs:
        deg[a] += 1; deg[b] += 1
        parent[find(a)] = find(b)
    used = np.nonzero(deg)[0]
    comps = len({find(int(a)) for a in used})
    return dict(max_degree=int(deg.max(initial=0)), cycles=len(pairs) - len(used) + comps, deg=deg)


# ------------------------------------------------------------------------------------------------------------------- generators
def _mesh(nx, size):
    V, F = meshes.grid_cloth(nx, nx, size, size, "DOWN")
    return f32(V), np.asarray(F, dtype=np.int32)


def _case(name, V, F, X, Vel, h, sphere=None, fwd_tol=1e-6, pd_iter_cap=1, **extra):
    return dict(name=name, V=V, F=F, X=f32(X), Vel=f32(Vel), h=h, sphere=sphere, fwd_tol=fwd_tol, pd_iter_cap=pd_iter_cap, **extra)


def cloud(name, nx, size, box, vs, seed, nfast=0, h=1 / 180, plant=0):
    """vertices uniform in `box`, velocities vs N(0, 1), `nfast` of them 20 x faster; `plant` vertices are moved next to an unconnected
    one (a list that is not empty where the cloud alone is too sparse)"""
    V, F = _mesh(nx, size)
    N = len(V)
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (N, 3)) * np.array(box, dtype=np.float64)
    vel = vs * rng.standard_normal((N, 3))
    if nfast:
        vel[rng.choice(N, nfast, replace=False)] *= 20
    for k in range(plant):
        a, b = 3 + 7 * k, N - 5 - 11 * k                 # far apart in the grid: unconnected
        X[b] = X[a] + np.array([0.05, 0.03, 0.02]) * (1 + 0.1 * k)
    return _case(name, V, F, X, vel, h)


def planted_window(name, seed, nx=12, size=2.0, box=(2.5, 1.2, 1.2), h=1 / 30, npairs=3):
    """A sparse, slow cloud plus designated pairs (grid vertices far apart, hence unconnected):
      sep 0.9  along the longest axis x, 6 cells apart: outside the sweep window, the reference never tests them -> no contact
      sep 0.5  along x, 3 cells apart: inside the window, contact through d1 only
      sep 1.05 along y (same 1-D cell): inside the window, cut by d0 > 1.0
    each closing at (sep - 0.1) / h, so that d1 = 0.1 < r_i + r_j = 0.162 for all of them."""
    V, F = _mesh(nx, size)
    N = len(V)
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (N, 3)) * np.array(box, dtype=np.float64)
    X[0] = (0.0, 0.6, 0.6); X[N - 1] = (box[0], 0.6, 0.6)     # pin the bounding box along x; both are slow, s_n[0] stays inside in y, z
    vel = 0.2 * rng.standard_normal((N, 3))
    vel[0] = 0                                               # s_n[0] = x_0 + h^2 g: inside the box along x
    maxR = radii_of(V, F).max()
    cellNum = int(box[0] / (2 * maxR)); cellDim = box[0] / cellNum
    ids = [k for k in range(14, N - 14, 5)]
    planted = dict(window=[], d1=[], unit=[])
    q = 0
    for kind, sep, ax, frac in (("window", 0.9, 0, 0.8), ("d1", 0.5, 0, 0.3), ("unit", 1.05, 1, 0.5)):
        for k in range(npairs):
            a, b = ids[q], ids[q] + 60 if ids[q] + 60 < N - 1 else ids[q] - 60
            q += 1
            base = np.array([(1 + 2 * k + frac) * cellDim, 0.06 + 0.02 * k, 0.1 + 0.12 * (q - 1)])
            if ax == 1:
                base[0] = (2 + 4 * k + frac) * cellDim
            X[a] = base
            X[b] = base; X[b, ax] += sep
            vel[a] = 0; vel[b] = 0
            vel[b, ax] = -(sep - 0.1) / h                          # relative velocity: gravity is common to both
            planted[kind].append((min(a, b), max(a, b)))
    return _case(name, V, F, X, vel, h, planted=planted)


def stack_state(V, stack, gap, rng, noise=0.004):
    """the grid folded in `stack` strips along x: strip k is mirrored when odd and lifted by k gap"""
    X = V.copy()
    x0 = X[:, 0].min(); w = (X[:, 0].max() - x0) / stack
    k = np.floor((X[:, 0] - x0) / w).clip(0, stack - 1)
    u = (X[:, 0] - x0) - k * w
    X[:, 0] = np.where(k % 2 == 1, w - u, u)
    X[:, 1] += gap * k
    X += noise * rng.standard_normal(X.shape)
    return X, k


def stack(name, nx, nstrips, gap, seed, sphere, lift=0.05):
    V, F = _mesh(nx, 4.5)
    rng = np.random.default_rng(seed)
    X, k = stack_state(V, nstrips, gap, rng)
    vel = 0.05 * rng.standard_normal(X.shape)
    vel[:, 1] -= 0.3 * k                                     # the upper strips come down on the lower ones
    sph = None
    if sphere:
        sph = dict(center=f32([X[:, 0].mean(), X[:, 1].min() - 2.0 + lift, X[:, 2].mean()]), radius=2.0, mu=0.3)
    return _case(name + ("_sphere" if sphere else ""), V, F, X, vel, 1 / 180, sphere=sph, fwd_tol=1e-9, pd_iter_cap=-1)


def zigzag(name, nx, rows, gap, seed):
    """the last 2 rows - 1 grid rows folded back over the cloth and forward again: `rows` rows lie `gap` above the cloth, rows - 1 rows
    2 gap above it, every vertex straight above one of the strip below (the diagonal neighbours are out of reach). Few contacts on many
    vertices — chains of two, one layer each: a deep contact list whose working set fits the LDS the one-workgroup kernels offer."""
    V, F = _mesh(nx, 4.5)
    rng = np.random.default_rng(seed)
    G = V.reshape(nx, nx, 3).copy()
    level = np.zeros((nx, nx))
    i1 = nx - 2 * rows
    up = np.array([0.0, gap, 0.0])
    for d in range(1, rows + 1):
        G[i1 + d] = V.reshape(nx, nx, 3)[i1 - d] + up
        level[i1 + d] = 1
    for d in range(1, rows):
        G[i1 + rows + d] = V.reshape(nx, nx, 3)[i1 - rows + d] + 2 * up
        level[i1 + rows + d] = 2
    X = G.reshape(-1, 3) + 0.004 * rng.standard_normal(V.shape)
    vel = 0.05 * rng.standard_normal(X.shape)
    vel[:, 1] -= 0.3 * level.reshape(-1)
    return _case(name, V, F, X, vel, 1 / 180, fwd_tol=1e-9, pd_iter_cap=-1)


def with_sphere(case, center, radius, mu=0.3):
    c = dict(case)
    c["name"] = case["name"] + "_sphere"
    c["sphere"] = dict(center=f32(center), radius=radius, mu=mu)
    return c


HUBS = dict(nx=12, size=2.0, box=(2.5, 1.2, 1.2), vs=3.0, nfast=20)
HUBS_SPHERE = dict(center=(1.25, 0.6, 0.6), radius=0.5)
# name -> (generator, arguments); the seed is part of the arguments
CASES = {
    "cloud_hubs": (cloud, dict(HUBS, seed=8)),
    "cloud_hubs_b": (cloud, dict(HUBS, seed=94)),             # the batch of three: same family, other contact counts
    "cloud_hubs_c": (cloud, dict(HUBS, seed=154)),
    "cloud_axis_y": (cloud, dict(nx=12, size=2.0, box=(1.0, 3.0, 1.0), vs=1.0, seed=4)),
    "cloud_512_cells": (cloud, dict(nx=12, size=2.0, box=(1.0, 1.0, 90.0), vs=1.0, seed=0, plant=6)),
    "planted_window": (planted_window, dict(seed=0)),
    "cloud_window_b": (cloud, dict(nx=12, size=2.0, box=(2.5, 1.2, 1.2), vs=1.0, seed=3, h=1 / 30)),      # beside planted_window: its h
    "cloud_window_c": (cloud, dict(nx=12, size=2.0, box=(1.0, 3.0, 1.0), vs=2.0, seed=4, h=1 / 30, nfast=5)),
    "cloud_512_threads": (cloud, dict(nx=40, size=4.5, box=(3.0, 2.0, 2.0), vs=1.0, seed=1, nfast=20)),
    "cloud_1024_threads": (cloud, dict(nx=79, size=9.0, box=(7.0, 5.0, 5.0), vs=1.0, seed=0, nfast=20)),
    "stack3": (stack, dict(nx=16, nstrips=3, gap=0.1, seed=3, sphere=False)),
    "stack3_sphere": (stack, dict(nx=16, nstrips=3, gap=0.1, seed=3, sphere=True, lift=0.0)),   # lower: 160 layers (148 at 0.05)
    "stack4": (stack, dict(nx=16, nstrips=4, gap=0.1, seed=3, sphere=False)),
    "stack4_sphere": (stack, dict(nx=16, nstrips=4, gap=0.1, seed=3, sphere=True)),
    "stack4_29": (stack, dict(nx=29, nstrips=4, gap=0.08, seed=3, sphere=False)),
    "stack4_29_sphere": (stack, dict(nx=29, nstrips=4, gap=0.08, seed=3, sphere=True)),
    "zigzag40": (zigzag, dict(nx=40, rows=4, gap=0.06, seed=0)),
}
CLOUDS = ["cloud_hubs", "cloud_hubs_b", "cloud_hubs_c", "cloud_axis_y", "cloud_512_cells", "planted_window", "cloud_window_b",
          "cloud_window_c", "cloud_512_threads", "cloud_1024_threads", "with_sphere"]
STACKS = ["stack3", "stack3_sphere", "stack4", "stack4_sphere", "stack4_29", "stack4_29_sphere", "zigzag40"]
ALL = CLOUDS + STACKS
UNIT_CUT_ON_DECIDING_PAIRS = ("cloud_512_threads", "cloud_1024_threads", "zigzag40")      # the meshes of 1 600 vertices and more


def make(name, seed=None):
    if name == "with_sphere":
        c = with_sphere(make("cloud_hubs", seed), **HUBS_SPHERE)
        c["name"] = name
        return c
    gen, kw = CASES[name]
    kw = dict(kw, seed=kw["seed"] if seed is None else seed)
    name = name[:-len("_sphere")] if name.endswith("_sphere") else name
    return gen(name, **kw)


# ------------------------------------------------------------------------------------------------------------------- conditions
def check_conditions(case, m=None):
    """The margins of every decision of the detection on `case` (see the module text); returns the dict of figures and the list of the
    conditions that do NOT hold."""
    m = detect_model(case["X"], case["Vel"], case["V"], case["F"], case["h"]) if m is None else m
    c = m["cand"]
    bad = []
    fig = dict(margin_thresh=m["margin_thresh"], margin_unit=m["margin_unit"], margin_axis=m["margin_axis"])
    if not (np.isfinite(case["X"]).all() and np.isfinite(case["Vel"]).all()):
        bad.append("non-finite input")
    if m["margin_thresh"] < MARGIN:
        bad.append(f"|min(d0, d1) - thresh| = {m['margin_thresh']:.2e}")
    # the 1.0 cut: over all unconnected pairs; on the meshes of 1 600 vertices and more over the pairs it can decide (swept distance below the threshold).
    # There a pair lands within 1e-5 of d0 = 1 about 27 times per seed (pairs x 4 pi 2e-5 / box volume), so no seed passes the first
    # form, and a pair whose swept distance is above its threshold by the margin is no contact whatever the cut says.
    c_unit = float(np.abs(c["d0"] - 1.0).min(initial=np.inf))
    fig["margin_unit_deciding"] = c_unit
    unit = c_unit if case["name"] in UNIT_CUT_ON_DECIDING_PAIRS else m["margin_unit"]
    if unit < MARGIN:
        bad.append(f"|d0 - 1| = {unit:.2e}")
    passed = c["near"]                                       # cand already holds min(d0, d1) < thresh
    diff = np.abs(c["cell_i"] - c["cell_j"])[passed]
    w = m["window"]
    fig["window_unsafe"] = int(((diff > w - 2) & (diff < w + 1)).sum())
    if fig["window_unsafe"]:
        bad.append(f"{fig['window_unsafe']} pairs within one cell of the window edge")
    if m["margin_axis"] < AXIS_MARGIN:
        bad.append(f"longest axis margin {m['margin_axis']:.2e}")
    # the cell count is a truncation: keep it away from the next integer (below the 512 cap)
    fig["margin_cellnum"] = float(min(m["cells_f"] - np.floor(m["cells_f"]), np.ceil(m["cells_f"]) - m["cells_f"])) if m["cells_f"] < 512 else float(m["cells_f"] - 512)
    if fig["margin_cellnum"] < 1e-4:
        bad.append(f"cell count margin {fig['margin_cellnum']:.2e}")
    acc = c["accepted"]
    fig["min_d0"] = float(c["d0"][acc].min(initial=np.inf))
    if fig["min_d0"] < MIN_D0:
        bad.append(f"accepted pair at d0 = {fig['min_d0']:.2e}")
    if case["sphere"] is not None:
        _, ms = sphere_model(case["X"], m["Vg"], case["h"], case["sphere"]["center"], case["sphere"]["radius"])
        fig["margin_sphere"] = ms
        if ms < MARGIN:
            bad.append(f"sphere margin {ms:.2e}")
    return fig, bad


# ------------------------------------------------------------------------------------------------------------------- the oracle's run
def oracle_of(case, threads=1):
    """The fp64 oracle set up for `case` (imported here: the generators and the model above need no compiled code)."""
    import orc
    o = orc.Oracle(case["V"], case["F"], h=case["h"], fwd_tol=case["fwd_tol"], bwd_tol=1e-9, selfcollision=True, contact=True,
                   gradient_clipping=False, pd_iter_cap=case["pd_iter_cap"], threads=threads, **MATERIAL)
    if case["sphere"] is not None:
        o.add_sphere(case["sphere"]["center"], case["sphere"]["radius"], case["sphere"]["mu"])
    o.build()
    return o


_REFERENCE = {}


def reference(name):
    """(case, oracle, its step, its layered contact list [(layer, id1, id2)] and contact dict) — computed once per process and shared;
    nobody writes to it."""
    if name not in _REFERENCE:
        case = make(name)
        o = oracle_of(case, threads=8 if case["pd_iter_cap"] < 0 else 1)
        ref = o.step(case["X"].reshape(-1), case["Vel"].reshape(-1))
        sc = o.self_contacts(ref["id"])
        layered = sorted((int(l), int(a), int(b)) for l, a, b in zip(sc["layer"], sc["p1"], sc["p2"]))
        _REFERENCE[name] = (case, o, ref, layered, sc)
    return _REFERENCE[name]


def engine_of(case, adjoint_mode=1, **params):
    """The engine set up for `case` like oracle_of(); the caller allocates the batch (and closes the engine)."""
    from diffcloth_amd import capi
    e = capi.Engine(0)
    e.set_mesh(case["V"], case["F"])
    kw = dict(time_step=case["h"], forward_tol=case["fwd_tol"], backward_tol=1e-9, cg_rel_tol=1e-6, cg_max_iter=2000, gradient_clipping=0,
              selfcollision_enabled=1, adjoint_mode=adjoint_mode, adjoint_rel_tol=1e-7, **MATERIAL)
    if case["pd_iter_cap"] > 0:
        kw["pd_iter_cap"] = case["pd_iter_cap"]
    kw.update(params)
    e.set_params(**kw)
    if case["sphere"] is not None:
        s = case["sphere"]
        e.set_primitives([dict(kind=capi.DC_PRIM_SPHERE, group=0, center=s["center"], radius=s["radius"], mu=s["mu"])])
    e.build()
    return e
