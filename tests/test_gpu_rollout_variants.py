"""Every instantiation of the rollout kernel (csrc/hsqp_rollout.h: rollout_dispatch) on the MI355X against a float64 reference.  k_rollout_plant<SW> is
compiled once per stage workspace, with its own LDS layout and register allocation, and its body spells the per-option loads out beside rollout_entry, which
the host emulation runs: a run on the device against an independent reference, per instantiation, is the only check those bodies get.

  instantiation                                                     compared with a reference on the device in
  StageWST<false>, CentWST<false>                                   test_gpu_rollout.py
  PlantStage                                                        test_gpu_plant.py, here
  PlantContactStage                                                 test_gpu_contact.py, here
  PlantActStage, PlantContactActStage                               test_gpu_actuator.py, here
  PlantVaried<PlantStage>, PlantVaried<PlantContactActStage>        test_gpu_inertia.py, here
  PlantTerrainStage                                                 test_gpu_terrain.py, here
  PlantVaried<PlantContactStage>, PlantVaried<PlantActStage>        here
  PlantTerrainActStage                                              here
  PlantVaried<PlantTerrainStage>, PlantVaried<PlantTerrainActStage> here

The reference is tests/variant_ref.py (composed of the older restatements, and held to them bit for bit by tests/test_rollout_variants.py); the case set, the
steps, the durations and the bounds are that file's, on the policies of the device's own solve: 8 nodes, 3 instances, 2^-6 s, two samples, RK4.  Then: no
state leaks between instantiations on one handle, batch independence of the largest workspace, ODE45 against a tight solution and the resident loop (with its
metrics) with every option on.

Measured on the MI355X, the worst instance of (uniform, feed-forward) / (events, feedback), x error of max(1, |x|):
  PlantStage 1.9e-11 / 1.7e-11, PlantActStage 1.5e-12 / 4.1e-12, PlantVaried<PlantStage> 2.3e-11 / 5.0e-11, PlantVaried<PlantActStage> 4.7e-12 / 5.0e-12;
  PlantContactStage 4.9e-11 / 8.5e-12, PlantContactActStage 4.6e-11 / 4.7e-11, PlantVaried<PlantContactStage> 2.8e-11 / 5.0e-11,
  PlantVaried<PlantContactActStage> 2.7e-11 / 4.8e-11; PlantTerrainStage 5.0e-11 / 1.9e-11, PlantTerrainActStage 2.0e-11 / 2.3e-11,
  PlantVaried<PlantTerrainStage> 2.5e-11 / 2.0e-11, PlantVaried<PlantTerrainActStage> 3.1e-11 / 1.7e-11 — the errors of the host emulation on the same cases, to
  two digits; u errors <= 5.3e-11, record errors <= 1.4e-11.  An option switched off alone moves x by 1.4e-2 at the least.  ODE45 on the largest: error /
  tolerance 0.08, tight error 2.0e-10.  The loop's metrics with a limit of 20 N m: saturated_joint_samples [1, 0, 1, 0, 0]."""
import signal

import numpy as np
import pytest

import actuator_ref as A
import contact_ref as CR
import inertia_ref as IR
import plant_ref as PL
import rollout_ref as R
import terrain_ref as TR
import test_gpu_metrics as GM
import variant_ref as V
from test_contact import EPS, RK4_STEP
from test_gpu_actuator import LIMITED, golden_limits
from test_gpu_contact import grounds
from test_gpu_loop import loop_case
from test_gpu_plant import GAINS
from test_gpu_push import B, KEYS, N, S0, by_hand, loop_start, problem, solved, start
from test_gpu_rollout import policies
from test_gpu_terrain import ALL_MAPS, mixed
from test_plant import FD_TOL
from test_rollout_variants import CASES, CONFIGS, HOLD, NEW, PAIRS, REC_TOL, STEP_FREE, U_TOL, pushes_of
from test_terrain import MAPS, TERRAIN_RK4_STEP, check_forces
from wb_humanoid_mpc_amd import _abi
from wb_humanoid_mpc_amd.solver import HipSqpSolver

pytestmark = pytest.mark.gpu
NX, NU, NV, NJ = _abi.NX, _abi.NU, _abi.NV, _abi.NJ
NAMES = ("ledge", None, "rubble")              # tests/test_gpu_terrain.py::mixed: a map, the plane (map = -1), another map in one launch
LARGEST = "PlantVaried<PlantTerrainActStage>"
# x without a ground: ten times the host emulation's error against the same reference (tests/test_rollout_variants.py::
# test_the_emulation_matches_the_composed_reference prints, worst instance, (uniform, feed-forward) / (events, feedback)), not below 1e-10 — the convention
# of tests/test_gpu_plant.py / test_gpu_inertia.py
EMU_X_ERROR = {"PlantStage": (6.66e-12, 3.35e-12), "PlantActStage": (2.29e-11, 1.56e-11), "PlantVaried<PlantStage>": (4.92e-12, 5.38e-12),
               "PlantVaried<PlantActStage>": (1.95e-11, 1.20e-11)}


# ---- the steps and durations of the device's cases.  The policies are those of the device's own solve, so the cases are not those of
# tests/test_rollout_variants.py, and its criterion — a perturbation of 1e-12 of the start state ends below 1e-9 in the reference — was measured again for
# all 24, on the CPU, with the policies read back from the device (the same perturbations; the largest entry over the three instances, (uniform,
# feed-forward) / (events, feedback)):
#   without a ground, 0.004 s over 2^-6 s     PlantStage 9.9e-11 / 8.3e-11, PlantActStage 1.1e-10 / 4.1e-10, PlantVaried<PlantStage> 1.1e-10 / 1.5e-10,
#                                             PlantVaried<PlantActStage> 7.3e-11 / 2.5e-10
#   on a map, 0.25 ms over 2^-6 s             PlantTerrainStage 9.8e-10 / 6.6e-10, PlantTerrainActStage 6.0e-10 / 3.2e-10, PlantVaried<PlantTerrainActStage>
#                                             7.4e-10 / 3.5e-10, PlantVaried<PlantTerrainStage> 1.4e-9 / 4.4e-10 — the first 1.1e-9 at 0.0625 ms still, and
#                                             6.3e-10 over 2^-7 s at 0.25 ms: half the duration
#   on the plane, 1 ms over 2^-6 s            PlantContactStage 8.3e-6 / 1.3e-9, PlantContactActStage 9.3e-10 / 9.8e-8, PlantVaried<PlantContactActStage> 1.3e-9 /
#                                             2.1e-9: instance 2 of PlantContactStage (uniform) is past RK4's stability limit at 1 ms — there the host emulation
#                                             itself lies 5.8e-7 from the reference, as the device does.  At 0.5 ms five of the eight still miss the criterion (1.2e-9
#                                             .. 3.5e-9): the cases' own sensitivity over 2^-6 s, which a smaller step does not settle.  Over 2^-7 s at 0.5 ms:
#                                             PlantContactStage 1.4e-9 / 4.7e-10, PlantContactActStage 7.1e-10 / 4.9e-10, PlantVaried<PlantContactStage> 1.2e-9 /
#                                             9.5e-10, PlantVaried<PlantContactActStage> 5.0e-10 / 4.9e-10; the two that miss it, at 0.25 ms: 7.2e-10 and 5.7e-10.
# So: the plane cases run over 2^-7 s at 0.5 ms (two of them at 0.25 ms), everything else as in tests/test_rollout_variants.py.
STEP = {("PlantContactStage", 0): RK4_STEP / 4, ("PlantVaried<PlantContactStage>", 0): RK4_STEP / 4}
DURATION = {("PlantVaried<PlantTerrainStage>", 0): 2.0 ** -7}


def step_of(name, pair):
    ground, terrain, _, _ = CONFIGS[name]
    return STEP.get((name, pair), TERRAIN_RK4_STEP if terrain else RK4_STEP / 2 if ground else STEP_FREE)


def duration_of(name, pair):
    ground, terrain, _, _ = CONFIGS[name]
    return DURATION.get((name, pair), 2.0 ** -7 if ground and not terrain else 2.0 ** -6)


def x_tol(name, pair):
    """Grounded: FD_TOL on the accelerations over the case's duration, times 10 (tests/test_gpu_contact.py X_TOL)."""
    return FD_TOL * duration_of(name, pair) * 10 if CONFIGS[name][0] else max(10 * EMU_X_ERROR[name][pair], 1e-10)


@pytest.fixture(autouse=True)
def time_limit():
    def expired(signum, frame):
        raise TimeoutError("test_gpu_rollout_variants: a test ran past its 120 s limit")
    old = signal.signal(signal.SIGALRM, expired)
    signal.alarm(120)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


@pytest.fixture(scope="module")
def handles(model):
    """One solved handle per grid, shared by the whole matrix: {grid: (solver, solution, dts, dt, x0)}."""
    hs = {grid: solved(model, False, grid) for grid, _ in PAIRS}
    yield hs
    for h in hs.values():
        h[0].close()


@pytest.fixture(scope="module")
def merged(model):
    return [IR.merged_oracle(model, *t) for t in table()]


@pytest.fixture(scope="module")
def shared():
    """What the matrix left behind for the tests after it: {(name, pair): the device's result}."""
    return {}


def table():
    return IR.variations(np.random.default_rng(2026))


def clear_all(s):
    s.clear_plant()
    s.clear_contact()
    s.clear_terrain()
    s.clear_actuator()
    s.clear_inertia()
    s.clear_pushes()


class Setup:
    """What one configuration sets on a handle, and the same for the reference.  rows: the instances the handle holds."""

    def __init__(self, model, oracle, name, xs, s0, actuator=None):
        self.model, self.oracle, self.name, self.xs, self.s0 = model, oracle, name, xs, s0
        self.on_ground, self.on_terrain, self.actuated, self.varied = CONFIGS[name]
        self.place = self.g = None
        if self.on_terrain:
            self.place, self.g = mixed(oracle, model, xs, NAMES[:len(xs)])
        elif self.on_ground:
            self.g = grounds(oracle, model, xs)
        self.actuator = dict(command_period=HOLD, **LIMITED) if actuator is None else actuator
        self.pushes = pushes_of(s0)[:len(xs)]
        self.tab = table()[:len(xs)]

    def apply(self, s, rows=slice(None), copies=1, table=True, actuator=True, ground=True, place=True):
        """Clears the five settings and the pushes, then sets exactly this configuration's; a keyword False switches that option off alone."""
        clear_all(s)
        s.set_plant(**GAINS)
        if self.on_ground:
            s.set_contact(enabled=ground)
            s.set_contact_instances(np.repeat(self.g[rows], copies, axis=0))
        if self.on_terrain:
            s.set_terrain_maps(ALL_MAPS)
            s.set_terrain_instances((self.place[rows] if place else [None] * len(self.place[rows])) * copies)
        if self.actuated:
            s.set_actuator(enabled=actuator, **self.actuator)
        if self.varied and table:
            tab = self.tab[rows] * copies
            s.set_inertia_instances(np.array([t[0] for t in tab]), [t[1] for t in tab])
        s.set_pushes(self.pushes[rows] * copies)

    def contact(self, b):
        return None if self.g is None else CR.with_ground(CR.contact(self.model), self.g[b])

    def terrain(self, b):
        return None if self.place is None or self.place[b] is None else (MAPS[NAMES[b]], self.place[b])

    def closed_loop(self, b, pol, xt, ctl, merged):
        ac = A.actuator(self.actuator["command_period"], self.actuator["effort_limit"], self.actuator["damping"], self.actuator["friction"]) if self.actuated else None
        return V.ClosedLoop(self.oracle, self.model, pol, xt, PL.plant(**GAINS), ctl, varied=merged[b] if self.varied else None, ct=self.contact(b),
                            terrain=self.terrain(b), ac=ac)


def kwargs(name, pair):
    return dict(integrator="rk4", controller="feedback" if PAIRS[pair][1] == R.FEEDBACK else "feedforward", initial_step=step_of(name, pair))


def check_contact_forces(s, su, x_end):
    """contact_forces() at the reference's final states against the reference's forces: check_forces of tests/test_terrain.py on a map (its bound on d extended
    by 8 x the reference's own rounding, measured against np.longdouble on this state), tests/test_gpu_contact.py's rule on the plane."""
    f, d = s.contact_forces(x_end)
    for b in range(len(x_end)):
        ct, ter = su.contact(b), su.terrain(b)
        fb, db = f[b].reshape(8, 3), d[b].ravel()
        if ter is not None:
            ref = TR.forces(su.oracle, su.model, x_end[b], ct, ter, velocity="frame")
            wide = TR.forces(su.oracle, su.model, x_end[b], ct, ter, velocity="frame", dtype=np.longdouble)
            check_forces(NAMES[b], "end", b, fb, db, ref, ct, float(np.abs(ref["d"] - wide["d"]).max()))
        else:
            ref = CR.forces(su.oracle, su.model, x_end[b], ct, velocity="frame")
            scale = np.abs(ref["P"][:, 2]) + abs(ct["ground_height"])
            Ab = ct["stiffness"] * 64 * EPS * scale[:, None]
            assert (np.abs(db - ref["d"]) <= 64 * EPS * scale).all(), b
            assert (np.abs(fb - ref["f"]) <= Ab + Ab * np.linalg.norm(ref["f"], axis=1)[:, None]).all(), b


# ---------------------------------------------------------------------------------------------- the matrix
@pytest.mark.parametrize("name,pair", CASES)
def test_rk4_matches_the_composed_reference(model, oracle, merged, handles, shared, name, pair):
    grid, ctl = PAIRS[pair]
    s, out, dts, dt, x0 = handles[grid]
    s0, xs, T = S0[grid], start(x0, False), duration_of(name, pair)
    su = Setup(model, oracle, name, xs, s0)
    su.apply(s)
    kw = kwargs(name, pair)
    r = s.rollout_policy(s0, xs, T, 2, **kw)
    last = np.array(s.actuator_torques()).transpose(1, 0, 2) if su.actuated else None
    shared[name, pair] = (r, last)
    assert (r["status"] == 0).all() and (r["rejected"] == 0).all()
    pols = policies(s, out, dts, dt, grid, False)
    st = R.settings(R.RK4, ctl, initial_step=kw["initial_step"])
    refs = [V.rollout(su.closed_loop(b, pols[b], out["x"][b], ctl, merged), pols[b], st, s0[b], xs[b], T, 2, su.pushes[b]) for b in range(B)]
    ex, eu, er = [], [], []
    for b, (xr, ur, sr, nr, rr, rec) in enumerate(refs):
        assert sr == R.OK and rr == 0 and r["steps"][b] == nr, (b, sr, r["steps"][b], nr)
        ex.append(float(np.abs(r["x"][b] - xr).max() / max(1.0, np.abs(xr).max())))
        eu.append(float(np.abs(r["u"][b] - ur).max() / max(1.0, np.abs(ur).max())))
        if rec is not None:
            er.append(float(np.abs(last[b] - rec).max() / max(1.0, np.abs(rec).max())))
    print(f"{name}, {grid}, controller {ctl}: steps {[x[3] for x in refs]}, x error " + " ".join(f"{e:.2e}" for e in ex) + ", u error " +
          " ".join(f"{e:.2e}" for e in eu) + (", record error " + " ".join(f"{e:.2e}" for e in er) if er else ""))
    if su.actuated:           # the reference first: the limit of 5 N m clamps a joint of some instance at the end
        assert any((np.abs(x[5][0]) > LIMITED["effort_limit"]).any() for x in refs)
        assert (np.abs(last[:, 1]) <= LIMITED["effort_limit"]).all()
    assert max(ex) <= x_tol(name, pair) and max(eu) <= U_TOL, (ex, eu)
    assert not er or max(er) <= REC_TOL, er
    if su.on_ground:
        check_contact_forces(s, su, np.array([x[0][-1] for x in refs]))


@pytest.mark.parametrize("name", NEW)
def test_every_option_acts(model, oracle, handles, name):
    """tests/test_rollout_variants.py::test_every_option_acts on the device, for the five instantiations that are new here: an option switched off alone moves
    the instances it concerns by more than 1e-6 of max(1, |x|), and leaves the others' bits (the table's neutral entry 0, the plane instance 1)."""
    pair = 1
    grid = PAIRS[pair][0]
    s, out, dts, dt, x0 = handles[grid]
    s0, xs, T = S0[grid], start(x0, False), duration_of(name, pair)
    su = Setup(model, oracle, name, xs, s0)
    su.apply(s)
    full = s.rollout_policy(s0, xs, T, 2, **kwargs(name, pair))
    assert (full["status"] == 0).all()
    moved = {}
    for on, what, rows, still in ((su.varied, "table", (1, 2), (0,)), (su.actuated, "actuator", (0, 1, 2), ()), (su.on_terrain, "place", (0, 2), (1,)),
                                  (su.on_ground, "ground", (0, 1, 2), ())):
        if not on:
            continue
        su.apply(s, **{what: False})
        off = s.rollout_policy(s0, xs, T, 2, **kwargs(name, pair))
        assert (off["status"] == 0).all(), what
        moved[what] = [float(np.abs(full["x"][b] - off["x"][b]).max() / max(1.0, np.abs(off["x"][b]).max())) for b in rows]
        for b in still:
            assert np.array_equal(full["x"][b], off["x"][b]), (what, b)
    print(f"{name}: switched off alone, an option moves x by " + ", ".join(f"{k} " + " ".join(f"{v:.2e}" for v in vs) for k, vs in moved.items()))
    assert len(moved) == sum(CONFIGS[name])
    assert all(v > 1e-6 for vs in moved.values() for v in vs), moved


# ---------------------------------------------------------------------------------------------- no state leaks between instantiations
def test_a_fresh_handle_gives_the_shared_handles_bits(model, oracle, handles, shared):
    """The shared handle has by now run whatever came before in this module (the whole matrix in a full run: eleven other instantiations, each with its own
    LDS layout and device-side tables); the largest instantiation on it equals the same call on a handle that has run nothing else, bit for bit — and the
    result the matrix itself got, where it ran."""
    pair = 1
    grid = PAIRS[pair][0]
    s, _, _, _, x0 = handles[grid]
    fresh = solved(model, False, grid)[0]
    try:
        s0, xs = S0[grid], start(x0, False)
        su = Setup(model, oracle, LARGEST, xs, s0)
        got = []
        for h in (s, fresh):
            su.apply(h)
            r = h.rollout_policy(s0, xs, duration_of(LARGEST, pair), 2, **kwargs(LARGEST, pair))
            got.append((r, np.array(h.actuator_torques()).transpose(1, 0, 2)))
        assert (got[0][0]["status"] == 0).all()
        for other in [got[1]] + ([shared[LARGEST, pair]] if (LARGEST, pair) in shared else []):
            assert all(np.array_equal(got[0][0][k], other[0][k]) for k in KEYS) and np.array_equal(got[0][1], other[1])
    finally:
        fresh.close()


# ---------------------------------------------------------------------------------------------- batch independence of the largest workspace
def test_every_instance_of_the_largest_equals_its_solo_rollout(model, oracle, handles):
    pair = 1
    grid = PAIRS[pair][0]
    s, _, _, _, x0 = handles[grid]
    s0, xs, T = S0[grid], start(x0, False), duration_of(LARGEST, pair)
    su = Setup(model, oracle, LARGEST, xs, s0)
    su.apply(s)
    r = s.rollout_policy(s0, xs, T, 2, **kwargs(LARGEST, pair))
    tq = s.actuator_torques()
    assert (r["status"] == 0).all()
    for b in range(B):
        one = slice(b, b + 1)
        solo = solved(model, False, grid, rows=one)[0]
        try:
            su.apply(solo, rows=one)
            r1 = solo.rollout_policy(s0[one], xs[one], T, 2, **kwargs(LARGEST, pair))
            for k in KEYS:
                assert np.array_equal(r1[k], r[k][one]), (b, k)
            assert all(np.array_equal(g, w[one]) for g, w in zip(solo.actuator_torques(), tq)), b
        finally:
            solo.close()


def test_sixty_four_copies_of_the_largest_equal_the_solo_result(model, oracle):
    """tests/test_gpu_actuator.py::test_sixty_four_copies_equal_the_solo_result with every option on: several workgroups per CU with the largest workspace.
    Instance 2: the payloads, the rubble map."""
    x0, x, u, par, dt = problem(model, False)
    one = slice(2, 3)
    big = HipSqpSolver(model, max_nodes=N, max_batch=64, riccati="serial")
    solo = HipSqpSolver(model, max_nodes=N, max_batch=64, riccati="serial")
    try:
        rep = lambda a: np.ascontiguousarray(np.repeat(a[one], 64, axis=0))   # noqa: E731
        big.run(rep(x0), rep(x), rep(u), rep(par), dt)
        solo.run(x0[one], x[one], u[one], par[one], dt)
        s0, xs = S0["uniform"], start(x0, False, 5)
        su = Setup(model, oracle, LARGEST, xs, s0)
        su.apply(big, rows=one, copies=64)
        su.apply(solo, rows=one)
        kw = dict(integrator="rk4", controller="feedback", initial_step=TERRAIN_RK4_STEP)
        r1 = solo.rollout_policy(s0[one], xs[one], 2.0 ** -6, 2, **kw)
        r = big.rollout_policy(np.repeat(s0[one], 64), np.repeat(xs[one], 64, axis=0), 2.0 ** -6, 2, **kw)
        assert (r1["status"] == 0).all()
        for k in KEYS:
            assert np.array_equal(r[k], np.repeat(r1[k], 64, axis=0)), k
        assert all(np.array_equal(g, np.repeat(w, 64, axis=0)) for g, w in zip(big.actuator_torques(), solo.actuator_torques()))
    finally:
        big.close()
        solo.close()


# ---------------------------------------------------------------------------------------------- ODE45 against a tight solution
ODE45_INSTANCE = 1


ODE45_MAPS = ("rubble", "rubble", "rubble")
ODE45_FRICTION = 0.0


def ode45_setup(model, oracle, x0, names=ODE45_MAPS, friction=ODE45_FRICTION):
    """The case of the ODE45 test: the instances on the maps `names`, the table, the actuator with the limits of the reference's model file
    (tests/test_gpu_actuator.py's ODE45 case) and a period of 0.003 s: five ticks inside 2^-6 s; no pushes."""
    xs = start(x0, False, 1)
    su = Setup(model, oracle, LARGEST, xs, S0["uniform"], actuator=dict(command_period=HOLD, effort_limit=golden_limits(model), damping=0.05, friction=friction))
    su.place, su.g = mixed(oracle, model, xs, names)
    su.terrain = lambda b: (MAPS[names[b]], su.place[b])
    su.pushes = [[], [], []]
    return su, xs


def test_ode45_on_the_largest_against_a_tight_solution(model, oracle, merged, handles):
    """The rule of tests/test_gpu_terrain.py::test_ode45_against_a_tight_solution: the tight solution is RK4 at 2^-15 s on the reference (restarted at the
    ticks, the command sampled at each), for ONE instance; ODE45 at the default tolerances within 10 x (abs_tol + rel_tol |x|) of it — 50 x with a node stamp
    inside the interval —, at tolerances of 1e-10 within 1e-7.
    The instance was chosen on the CPU, with the policies read back from the device: instance 1 on the rubble map, whose tight solutions at 2^-15 s and at
    2^-16 s agree to 1.1e-10 (the host emulation's ODE45 on it: error / tolerance 0.08, tight error 2.0e-10) — WITHOUT joint friction.  With the friction of
    0.1 N m of the other cases no instance has a tight RK4 solution: 2^-15 s against 2^-16 s gives 6.2e-7 for this one, 3.0e-5 and 2.4e-6 for its
    neighbours, and 1.2e-7 .. 3.0e-6 on the ramp and the ledge (a joint velocity crosses the friction's regularisation of 0.01 rad/s within a few steps of
    2^-15 s; the device's ODE45 at 1e-10 lies 7.8e-7 from that solution, as the host emulation's does).  Without it: 3.0e-11 (ledge, instance 0), 1.9e-8 and
    2.7e-8 (instance 1 on the ledge and the ramp), 3.7e-7 (ramp, instance 0).  So the case keeps the hold, the limits and the damping, and sets the friction
    to zero."""
    s, out, dts, dt, x0 = handles["uniform"]
    s0, T, b = S0["uniform"], 2.0 ** -6, ODE45_INSTANCE
    su, xs = ode45_setup(model, oracle, x0)
    pols = policies(s, out, dts, dt, "uniform", False)
    cl = su.closed_loop(b, pols[b], out["x"][b], R.FEEDFORWARD, merged)
    ref, _ = V.tight_solution(cl, pols[b], s0[b], xs[b], T)
    assert np.isfinite(ref).all()
    su.apply(s)
    r = s.rollout_policy(s0, xs, T, 1)
    assert (r["status"] == 0).all() and (r["steps"] < 10000).all()
    assert (r["steps"] >= 6).all()                                      # a restart at every tick: 6 intervals in 2^-6 s
    r2 = s.rollout_policy(s0, xs, T, 1, abs_tol=1e-10, rel_tol=1e-10)
    assert (r2["status"] == 0).all() and (r2["steps"] > r["steps"]).all() and (r2["steps"] < 10000).all()
    err = float(np.abs(r2["x"][b, 0] - ref).max())
    ratio = float((np.abs(r["x"][b, 0] - ref) / (1e-5 + 1e-3 * np.abs(ref))).max())
    print(f"T {T}: steps {r['steps']} rejected {r['rejected']} error / tolerance {ratio:.2f}; tight steps {r2['steps']} rejected {r2['rejected']} "
          f"tight error {err:.2e}")
    stamps = np.arange(N + 1) * dt
    kink = any(((stamps - la > s0[b]) & (stamps - la < s0[b] + T)).any() for la in (0.0, PL.plant(**GAINS)["lookahead"]))
    assert ratio <= (50.0 if kink else 10.0), (kink, ratio)
    assert err <= 1e-7, err


# ---------------------------------------------------------------------------------------------- the resident loop
def loop_options(s, model, oracle, x0, names, mus, cap=np.inf):
    """Every option on a loop handle over the states x0: the ground and the maps `names`, the actuator (a period of 0.002 s, the limits of the reference's
    model file, none above `cap` — under 5 N m the robot folds within the loop's cycles), the table (repeated past its three entries); returns the limits."""
    lim = np.minimum(golden_limits(model), cap)
    n = len(x0)
    place, g = mixed(oracle, model, x0, names, mus=mus)
    tab = (table() * n)[:n]
    s.set_plant(**GAINS)
    s.set_contact()
    s.set_contact_instances(g)
    s.set_terrain_maps(ALL_MAPS)
    s.set_terrain_instances(place)
    s.set_actuator(command_period=0.002, effort_limit=lim, damping=0.05, friction=0.1)
    s.set_inertia_instances(np.array([t[0] for t in tab]), [t[1] for t in tab])
    return lim


def test_the_loop_with_every_option_equals_the_calls_it_replaces(model, oracle):
    """The pattern of tests/test_gpu_terrain.py::test_the_loop_on_the_ledge_equals_the_calls_it_replaces."""
    case = loop_case(model, batch=B)
    s = HipSqpSolver(model, max_nodes=N, max_batch=B, linesearch=True, riccati="serial")
    try:
        s.set_plant(**GAINS)
        loop_start(s, model, case)
        plain = s.loop_run(3)
        loop_options(s, model, oracle, case["x0"], ("ledge", "ramp", "ledge"), (0.3, 0.6, 1.0))
        want = by_hand(s, model, case, 3, "feedforward")         # the settings survive the uploads
        want_last = s.actuator_torques()
        loop_start(s, model, case)                               # ... and the start of a loop
        got = s.loop_run(3)
        got_last = s.actuator_torques()
    finally:
        s.close()
    assert got["cycles_done"] == 3 and np.isfinite(got["x"]).all()
    assert np.array_equal(got["x"], want["x"]) and np.array_equal(got["u"], want["u"])
    assert np.isfinite(got_last[0]).all() and all(np.array_equal(g, w) for g, w in zip(got_last, want_last))
    assert not np.array_equal(got["x"], plain["x"])


def test_the_loops_metrics_see_a_varied_actuated_plant_on_a_map(model, oracle):
    """k_loop_metrics<ContactTerrainSet> with the table and the actuator model: the sample counts of the records equal those rebuilt from the public calls
    after every single cycle (tests/test_gpu_metrics.py::single_cycles, its shapes: 5 instances, 20 nodes), over three cycles."""
    case = loop_case(model, batch=GM.B)
    s = HipSqpSolver(model, max_nodes=GM.N, max_batch=GM.B, linesearch=True, riccati="serial")
    try:
        lim = loop_options(s, model, oracle, case["x0"], ("ramp",) * GM.B, (0.3, 0.6, 1.0, 0.8, 0.5), cap=20.0)      # (a standing knee carries more)
        GM.begin(s, model, case)
        want = GM.single_cycles(s, 3, torque_limits=lim, ground=True).arrays()
        got = s.loop_metrics()
    finally:
        s.close()
    print("torque_samples", got["torque_samples"].tolist(), "ground_samples", got["ground_samples"].tolist(), "saturated_joint_samples",
          got["saturated_joint_samples"].tolist())
    assert (got["cycles"] == 3).all() and (got["torque_samples"] == 3).all() and (got["ground_samples"] == 3).all()
    assert (got["saturated_joint_samples"] > 0).any()
    for k in ("torque_samples", "ground_samples", "saturated_joint_samples"):
        assert np.array_equal(got[k], want[k]), (k, got[k], want[k])
