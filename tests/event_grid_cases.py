"""Problems on PER-INSTANCE event grids for tests/test_event_forms.py and tests/test_gpu_event_forms.py (a plain module, no fixtures).

hsqp_problem::dt_nodes is [B][N]: every instance may carry its own ocs2 event-node grid, padded to N = n_nodes + event_nodes intervals by a run of
zero-length intervals in front of the last one (include/hsqp_grid.h; reference.padded_event_grid is its mirror).  The builders below make such batches
from make_problem's per-instance gait phases and ASSERT what makes them worth testing — the grids differ between neighbours, inside a wave of 16 nodes
and modulo 16 — so that a drift of the inputs stops the tests instead of silently leaving them on a grid every index is right on.

Every problem and every oracle result is computed once per process and handed out read-only."""
import collections

import numpy as np

from wb_humanoid_mpc_amd import _abi
from wb_humanoid_mpc_amd.reference import (TargetTrajectories, build_centroidal_node_params, build_node_params_at, cold_start, make_centroidal_problem, make_problem,
                                           padded_event_grid)

DT_MIN = 1e-4
WAVE_NODES = 16        # nodes per wave of the limb-lane kernels and of the value pass on quads of lanes
WORKGROUP_NODES = 32   # nodes per workgroup of the limb-lane kernels (173 x 97 nodes are 525 workgroups, tests/test_gpu_parity.py)

EventProblem = collections.namedtuple("EventProblem", "x0 x u par dts node_times n_intervals")

# the named cases: (B, n_nodes, event_nodes, gait, seed); N = n_nodes + event_nodes
CASES = {
    "A_walk": (5, 12, 6, "walk", 31),    # N = 18
    "A_run": (5, 12, 6, "run", 32),
    "S": (6, 30, 10, "walk", 33),        # N = 40: events on the last and on the first stage of a segment for P = 7 and P = 3
    "P": (3, 50, 14, "walk", 34),        # N = 64 >= HSQP_SCAN_AUTO_MIN_NODES: the first two instances are the scan's automatic range
}
CENT_CASE = (3, 12, 6, "walk", 35)       # the centroidal twin, N = 18
# two node ranges of the limb-lane kernels, 173 x 97 nodes with the range boundary inside instance 86: from the mirror, 14 event nodes overflow on this
# batch, 15 leave every instance 1 .. 3 padding intervals
RANGE_CASE = (173, 82, 15, "walk", 3)


def event_intervals(dts_b):
    """indices of the zero-length intervals (events and padding) of one instance's grid"""
    return np.flatnonzero(np.asarray(dts_b) == 0.0)


def padding_intervals(prob):
    """zero-length padding intervals per instance: N - n_intervals"""
    return prob.dts.shape[1] - prob.n_intervals


def seg_bound(p, N, P):
    """csrc/hsqp_segment.h: the first stage of segment p of P over N stages"""
    return (p * N) // P


def grid_facts(dts, n_intervals):
    """The properties of a batch of grids the tests rest on, each a bool (see the module docstring and check_grids)."""
    dts = np.asarray(dts)
    B, N = dts.shape
    pad = N - np.asarray(n_intervals)
    sets = [frozenset((event_intervals(d) % WAVE_NODES).tolist()) for d in dts]
    mixed = False
    for w in range((B * N + WAVE_NODES - 1) // WAVE_NODES):
        flat = np.arange(w * WAVE_NODES, min((w + 1) * WAVE_NODES, B * N))
        inst, node = flat // N, flat % N
        for o in set(inst.tolist()):
            # a lane of this wave whose own dt is not what instance o (also in this wave) has at the same node
            mixed |= bool(np.any((inst != o) & (dts[inst, node] != dts[o, node])))
    return dict(neighbours_differ=all(not np.array_equal(dts[b], dts[b + 1]) for b in range(B - 1)),
                events_differ_mod_wave=len(set(sets)) > 1,
                long_padding_run=bool((pad >= 3).any()),
                short_padding_run=bool((pad <= 1).any()),
                wave_mixes_instances=mixed,
                partial_workgroup=(B * N) % WORKGROUP_NODES != 0)


def check_grids(dts, n_intervals):
    """What every batch from the builders must have, or the tests would not see a wrong grid index:
      * no two neighbouring instances share a grid, and the sets of zero-length intervals are not all equal modulo 16 (an index that is off by an
        instance, or by a wave, lands on another dt);
      * some 16-node wave of the flattened [B * N] node axis holds nodes of two instances whose dt differ at the same node (a wave that takes ONE
        instance's row for all its lanes is wrong there);
      * some instance pads with a run of >= 3 zero-length intervals (every position of the factored roll-out's groups of three stages is an event).
    Where N is a multiple of 16 no wave spans two instances and the second property cannot hold (case P, N = 64, which is there for the scan kernels:
    one workgroup per node); it is asserted wherever N is not.  The remaining two properties of grid_facts — an instance with at most ONE padding
    interval, B * N no multiple of 32 — do not hold for every named case either (walk horizons of 12, 30 and 50 nodes leave at least 2, 3 and 5 spare
    intervals; 3 x 64 = 192): tests/test_event_forms.py pins them, and the padding counts, per case."""
    f = grid_facts(dts, n_intervals)
    for key in ("neighbours_differ", "events_differ_mod_wave", "long_padding_run"):
        assert f[key], (key, f)
    assert f["wave_mixes_instances"] == (np.shape(dts)[1] % WAVE_NODES != 0), f
    assert not np.any(np.asarray(dts)[:, -1] == 0.0) and np.all(np.asarray(dts) >= 0.0)
    return f


def _grids(schedules, t0, n_nodes, dt, event_nodes):
    rows = [padded_event_grid(t0, n_nodes, dt, s.event_times, event_nodes, DT_MIN) for s in schedules]       # raises GridOverflow
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]), np.array([r[2] for r in rows], np.int32)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return EventProblem(*arrays)


_cache = {}


def per_instance_event_problem(model, B, n_nodes, event_nodes, seed, gait):
    """Whole-body batch on per-instance padded event grids: make_problem's perturbed initial states and random gait phases, every instance's own
    padded_event_grid, its parameters on its own node times, the cold start left by 0.01 N(0,1) in x and 0.5 N(0,1) in u (so that the jump defects
    are non-zero).  Returns EventProblem(x0 [B][58], x [B][N+1][58], u [B][N][35], par [B][N+1][72], dts [B][N], node_times [B][N+1], n_intervals [B])."""
    key = ("wb", B, n_nodes, event_nodes, seed, gait)
    if key not in _cache:
        x0, _, _, _, dt, (schedules, targets, t0) = make_problem(model, n_nodes=n_nodes, batch=B, perturb=True, seed=seed, gait=gait, with_reference=True)
        dts, node_times, n_intervals = _grids(schedules, t0, n_nodes, dt, event_nodes)
        check_grids(dts, n_intervals)
        par = np.stack([build_node_params_at(model, schedules[b], targets[b], node_times[b]) for b in range(B)])
        xu = [cold_start(model, x0[b], par[b]) for b in range(B)]
        x, u = np.stack([a for a, _ in xu]), np.stack([a for _, a in xu])
        rng = np.random.default_rng(seed + 1000)
        x = x + 0.01 * rng.standard_normal(x.shape)
        u = u + 0.5 * rng.standard_normal(u.shape)
        _cache[key] = _frozen(x0, x, u, par, dts, node_times, n_intervals)
    return _cache[key]


def per_instance_centroidal_event_problem(cmodel, B, n_nodes, event_nodes, seed, gait):
    """The centroidal twin: make_centroidal_problem's instances, build_centroidal_node_params per node time of every instance's own grid, only the
    states perturbed around the cold start (as tests/test_event_nodes.py::test_device_centroidal_event_grid_equals_the_oracle does)."""
    key = ("cent", B, n_nodes, event_nodes, seed, gait)
    if key not in _cache:
        x0, _, _, _, dt, (schedules, targets, t0) = make_centroidal_problem(cmodel, n_nodes=n_nodes, batch=B, perturb=True, seed=seed, gait=gait, with_reference=True)
        dts, node_times, n_intervals = _grids(schedules, t0, n_nodes, dt, event_nodes)
        check_grids(dts, n_intervals)
        unpadded = [TargetTrajectories(t.times, t.states[:, :_abi.CNX]) for t in targets]
        par = np.stack([np.stack([build_centroidal_node_params(cmodel, schedules[b], unpadded[b], t, dt, 0)[0] for t in node_times[b]]) for b in range(B)])
        xu = [cold_start(cmodel, x0[b], par[b]) for b in range(B)]
        x, u = np.stack([a for a, _ in xu]), np.stack([a for _, a in xu])
        rng = np.random.default_rng(seed + 1000)
        x[:, :, :_abi.CNX] += 0.01 * rng.standard_normal((B, n_nodes + event_nodes + 1, _abi.CNX))
        _cache[key] = _frozen(x0, x, u, par, dts, node_times, n_intervals)
    return _cache[key]


def case(model, name):
    B, n_nodes, event_nodes, gait, seed = CASES[name]
    return per_instance_event_problem(model, B, n_nodes, event_nodes, seed, gait)


def centroidal_case(cmodel):
    B, n_nodes, event_nodes, gait, seed = CENT_CASE
    return per_instance_centroidal_event_problem(cmodel, B, n_nodes, event_nodes, seed, gait)


def range_case(model):
    B, n_nodes, event_nodes, gait, seed = RANGE_CASE
    return per_instance_event_problem(model, B, n_nodes, event_nodes, seed, gait)


def instance(prob, b):
    """(x0, x, u, par, dts) of instance b"""
    return prob.x0[b], prob.x[b], prob.u[b], prob.par[b], prob.dts[b]


def permuted(prob, perm):
    return EventProblem(*(np.ascontiguousarray(a[perm]) for a in prob))


_oracle_cache = {}


def oracle_iteration(oracle, prob, b, threads=4):
    """oracle.sqp_iteration (cent_sqp_iteration for a centroidal oracle) of instance b under set_grid(its own dts), with its LQ blocks under "lq"
    (whole-body only) — computed once."""
    key = (id(prob), b, bool(oracle.model.centroidal))
    if key not in _oracle_cache:
        x0, x, u, par, dts = instance(prob, b)
        oracle.set_grid(dts)
        try:
            if oracle.model.centroidal:
                r = oracle.cent_sqp_iteration(0.0, x0, x, u, par, threads=threads)
            else:
                r = oracle.sqp_iteration(0.0, x0, x, u, par, threads=threads)
                r["lq"] = oracle.lq(0.0, x, u, par, threads=threads)
        finally:
            oracle.set_grid(None)
        _oracle_cache[key] = r
    return _oracle_cache[key]


def step_scale(r):
    return max(np.abs(r["dx"]).max(), np.abs(r["du"]).max())


def step_error(out, r, b=None):
    """max |dx|, |du| difference of a result (instance b of a batch, or a single instance's arrays) from an oracle result"""
    dx, du = (out["dx"], out["du"]) if b is None else (out["dx"][b], out["du"][b])
    return max(np.abs(dx - r["dx"]).max(), np.abs(du - r["du"]).max())
