"""The height-map terrain under the torque plant (include/hsqp_terrain.h) on the MI355X, through the C ABI: heights and normals, contact forces and the RK4
rollout against the numpy restatement (tests/terrain_ref.py), ODE45 against a tight RK4 solution of that reference, a plane instance inside a terrain batch
and the paths without a terrain bit for bit, batch independence and chaining, the _device entry points, the resident loop, the iteration untouched, and the
argument errors.  The shapes of tests/test_gpu_contact.py: 8 nodes, 3 instances, 2^-6 s, the tests' gains; the maps, the placements and the bounds of
tests/test_terrain.py (the ground of every instance 1 mm above its lowest sole corner at that corner's (X, Y))."""
import ctypes as C
import signal

import numpy as np
import pytest

import contact_ref as CR
import plant_ref as PL
import rollout_ref as R
import terrain_ref as TR
from test_contact import EPS, RK4_STEP
from test_gpu_contact import X_TOL
from test_gpu_feedback_policy import DeviceBuffer
from test_gpu_loop import loop_case
from test_gpu_plant import GAINS, U_TOL
from test_gpu_push import B, D, KEYS, N, S0, by_hand, loop_start, problem, same, solved, start
from test_gpu_rollout import policies
from test_terrain import MAPS, MAP_INDEX, TERRAIN_RK4_STEP, check_forces, force_cases, height_bounds, place_under, sample_points
from wb_humanoid_mpc_amd import _abi
from wb_humanoid_mpc_amd.solver import HipSqpSolver, HsqpError

pytestmark = pytest.mark.gpu
NX, NU, NV, NJ = _abi.NX, _abi.NU, _abi.NV, _abi.NJ
ALL_MAPS = [(MAPS[k]["H"], MAPS[k]["cell"]) for k in ("ramp", "ledge", "rubble")]     # the handle's list: MAP_INDEX
_dp = C.POINTER(C.c_double)


@pytest.fixture(autouse=True)
def time_limit():
    def expired(signum, frame):
        raise TimeoutError("test_gpu_terrain: a test ran past its 120 s limit")
    old = signal.signal(signal.SIGALRM, expired)
    signal.alarm(120)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


def table_doubles(place):
    """The placement table as the doubles a DeviceBuffer uploads (an entry is 32 bytes)."""
    tab = HipSqpSolver.pack_terrain_instances(place)
    return np.frombuffer(bytes(tab), dtype=np.float64).reshape(len(place), 4).copy()


def mixed(oracle, model, xs, names=("ledge", None, "rubble"), mus=(0.2, 0.6, 1.0)):
    """(place [B], ground [B, 2]) of a mixed batch: instance b on the map names[b] (None: map = -1), its ground 1 mm above its lowest corner."""
    place, ground = [], []
    for b, name in enumerate(names):
        if name is None:
            place.append(None)
            ground.append((float(CR.points(oracle, model, xs[b][:NV])[:, 2].min() + 1e-3), mus[b]))
        else:
            pl, hgt = place_under(oracle, model, name, xs[b])
            place.append(pl)
            ground.append((hgt, mus[b]))
    return place, np.array(ground)


# ---------------------------------------------------------------------------------------------- 1. height and normal
@pytest.mark.parametrize("name", ["ramp", "ledge", "rubble"])
def test_height_and_normal_match_the_reference(model, name):
    """The bounds of tests/test_terrain.py::test_height_and_normal_match_the_reference (the device contracts the rotation into fused multiply-adds: a
    coordinate moves by its rounding, which those bounds count — far outside the grid it is the rounding of a difference of large products), far outside
    the grid with finite coordinates only."""
    rng = np.random.default_rng(12)
    mp = MAPS[name]
    places = [TR.placement((0.0, 0.0), 0.0, MAP_INDEX[name]), TR.placement((0.3, -0.8), 0.7, MAP_INDEX[name]), None]
    pts = [sample_points(mp, pl, rng) for pl in places[:2]]
    flat = [[p for cls in ("interior", "lines", "outside") for p in d[cls]] for d in pts]
    cls_of = [[cls for cls in ("interior", "lines", "outside") for _ in d[cls]] for d in pts]
    xy = np.array(flat + [flat[0]])
    s = HipSqpSolver(model, max_nodes=N, max_batch=B)
    try:
        s.set_plant(kind="flow", **GAINS)                  # (any plant kind, no resident solution)
        s.set_contact(ground_height=0.37, enabled=False)
        s.set_terrain_maps(ALL_MAPS)
        s.set_terrain_instances(places)
        g, n = s.terrain_height(xy)
        for k, pl in enumerate(places[:2]):
            for (X, Y), cls, gi, ni in zip(flat[k], cls_of[k], g[k], n[k]):
                hm, nr, _ = TR.height_normal(mp, pl, X, Y)
                tol_h, tol_n, dH = height_bounds(mp, pl, X, Y, 0.37)
                assert abs(gi - (0.37 + hm)) <= tol_h, (name, k, cls, X, Y, gi - 0.37 - hm)
                if cls == "lines":                         # (on a cell line either side's patch: tests/test_terrain.py)
                    e = 1e-7 * mp["cell"]
                    around = [TR.height_normal(mp, pl, X + sx * e, Y + sy * e)[1] for sx in (-1, 1) for sy in (-1, 1)]
                    assert min(np.abs(ni - a).max() for a in around) <= tol_n + 1e-6 * dH / mp["cell"], (name, k, cls, X, Y)
                else:
                    assert np.abs(ni - nr).max() <= tol_n, (name, k, cls, X, Y, ni, nr)
                assert abs(np.linalg.norm(ni) - 1.0) <= 4 * EPS
        assert (g[2] == 0.37).all() and (n[2] == [0.0, 0.0, 1.0]).all()      # map = -1: the plane
        # the device entry point gives the same bits
        dxy, dg, dn = DeviceBuffer(xy.shape), DeviceBuffer(g.shape), DeviceBuffer(n.shape)
        try:
            dxy.upload(xy)
            cast = lambda p: C.cast(p.ptr, _dp)   # noqa: E731
            s._check(s.lib.hsqp_terrain_eval_device(s.h, B, xy.shape[1], cast(dxy), cast(dg), cast(dn)))
            assert np.array_equal(dg.numpy(), g) and np.array_equal(dn.numpy(), n)
        finally:
            for buf in (dxy, dg, dn):
                buf.free()
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------- 2. contact forces on the terrain
@pytest.mark.parametrize("name", ["ramp", "ledge", "rubble"])
def test_contact_forces_match_the_reference(model, oracle, name):
    """tests/test_terrain.py::test_forces_and_penetrations_match_the_reference on the device, with its bounds (the old rule plus 8 x the reference's own
    rounding in d, measured there against np.longdouble), on the start states and the deep states; then the table and the states in device memory.
    Measured on the MI355X: worst d error / bound 0.13 (ramp), 0.17 (ledge), 0.29 (rubble) — 0.33 of the old bound —, worst force error / bound 0.005."""
    x0 = problem(model, False)[0]
    xs = start(x0, False)
    cases, ref_d = force_cases(oracle, model, xs, name)
    s = HipSqpSolver(model, max_nodes=N, max_batch=2 * B)
    try:
        xa = np.array([c[4] for c in cases])
        place = [c[2] for c in cases]
        g = np.array([(c[3]["ground_height"], c[3]["mu"]) for c in cases])
        s.set_contact()
        s.set_contact_instances(g)
        plane_f = s.contact_forces(xa)[0]
        s.set_terrain_maps(ALL_MAPS)
        assert np.array_equal(s.contact_forces(xa)[0], plane_f)          # maps without a table: the plane model
        s.set_terrain_instances(place)
        f, d = s.contact_forces(xa)
        assert not np.array_equal(f, plane_f)
        active = sloped = 0
        for k, (kind, b, pl, ct, x, ref) in enumerate(cases):
            check_forces(name, kind, b, f[k].reshape(8, 3), d[k].ravel(), ref, ct, ref_d)
            active += ref["cls"].count("a")
            sloped += int((np.abs(ref["grad"]).sum(axis=1) > 0.0).sum())
        assert active >= B and sloped >= 1
        tab = table_doubles(place)
        dt, dx, df, dd = DeviceBuffer(tab.shape), DeviceBuffer(xa.shape), DeviceBuffer(f.shape), DeviceBuffer(d.shape)
        try:
            dt.upload(tab)
            dx.upload(xa)
            s.set_terrain_instances(None)
            assert np.array_equal(s.contact_forces(xa)[0], plane_f)
            s.set_terrain_instances_device(2 * B, dt.ptr.value)
            cast = lambda p: C.cast(p.ptr, _dp)   # noqa: E731
            s._check(s.lib.hsqp_contact_eval_device(s.h, 2 * B, cast(dx), cast(df), cast(dd)))
            assert np.array_equal(df.numpy(), f) and np.array_equal(dd.numpy(), d)
            got = s.get_terrain_instances(2 * B)
            assert [p["map"] for p in got] == [MAP_INDEX[name]] * (2 * B) and got[0]["origin"] == place[0]["origin"]
        finally:
            for buf in (dt, dx, df, dd):
                buf.free()
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------- 6. RK4 against terrain_ref
@pytest.mark.parametrize("grid,controller", [("uniform", "feedforward"), ("events", "feedback")])
def test_rk4_matches_the_reference(model, oracle, grid, controller):
    """At TERRAIN_RK4_STEP (tests/test_terrain.py: at the plane's 1 ms the rubble case is past RK4's stability limit).  Instance 0 on the ledge, instance 2 on the rubble, each against its own reference (X_TOL / U_TOL of tests/test_gpu_contact.py: the reference carries a
    finite-difference Jacobian), equal step counts, the runs differ from the plane run by > 1e-6; instance 1 (map = -1) is the plane run, bit for bit."""
    s, out, dts, dt, x0 = solved(model, False, grid)
    try:
        s0 = S0[grid]
        xs = start(x0, False)
        place, g = mixed(oracle, model, xs)
        s.set_plant(**GAINS)
        s.set_contact()
        s.set_contact_instances(g)
        kw = dict(integrator="rk4", controller=controller, initial_step=TERRAIN_RK4_STEP)
        plane = s.rollout_policy(s0, xs, D, 2, **kw)
        s.set_terrain_maps(ALL_MAPS)
        s.set_terrain_instances(place)
        r = s.rollout_policy(s0, xs, D, 2, **kw)
        assert (r["status"] == 0).all() and (r["rejected"] == 0).all() and (plane["status"] == 0).all()
        for k in KEYS:
            assert np.array_equal(r[k][1], plane[k][1]), k                   # 4. map = -1 inside a terrain batch
        pl, ct0 = PL.plant(**GAINS), CR.contact(model)
        pols = policies(s, out, dts, dt, grid, False)
        ctl = R.FEEDBACK if controller == "feedback" else R.FEEDFORWARD
        st = R.settings(R.RK4, ctl, initial_step=TERRAIN_RK4_STEP)
        for b, name in ((0, "ledge"), (2, "rubble")):
            cl = TR.closed_loop(oracle, model, pols[b], out["x"][b], pl, ctl, CR.with_ground(ct0, g[b]), (MAPS[name], place[b]))
            xr, ur, sr, nr, _ = PL.rollout(cl, pols[b], st, s0[b], xs[b], D, 2)
            assert sr == R.OK and r["steps"][b] == nr, (b, r["steps"][b], nr)
            err = np.abs(r["x"][b] - xr).max() / max(1.0, np.abs(xr).max())
            erru = np.abs(r["u"][b] - ur).max() / max(1.0, np.abs(ur).max())
            diff = np.abs(r["x"][b] - plane["x"][b]).max() / max(1.0, np.abs(plane["x"][b]).max())
            print(f"{grid} {controller} instance {b} ({name}): steps {nr}, x error {err:.2e}, u error {erru:.2e}, against the plane run {diff:.2e}")
            assert err <= X_TOL, (b, err)
            assert erru <= U_TOL, (b, erru)
            assert diff > 1e-6, (b, diff)
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------- 7. ODE45 against a tight solution
def test_ode45_against_a_tight_solution(model, oracle):
    """tests/test_gpu_contact.py::test_ode45_against_a_tight_solution on the rubble map, with its tolerance rule; the tight solution is RK4 at 2^-15 s on
    terrain_ref, for ONE instance: instance 1, which stands on one corner on a slope of 0.12 throughout (95 N at the end).  (Not instance 0: there the RK4
    solution is not tight — measured, it lies 3.0e-5 from ODE45 at tolerances of 1e-10 AND of 1e-12, which agree with each other to 5.4e-9, and 1.8e-6 at
    2^-16 s: three corners touch down and lift off within the interval.)  Measured for instance 1: error / tolerance 0.16, tight error 6.8e-11."""
    s, out, dts, dt, x0 = solved(model, False, "uniform")
    try:
        s0 = S0["uniform"]
        T = 2.0 ** -6
        xs = start(x0, False, 1)
        place, g = mixed(oracle, model, xs, ("rubble", "rubble", "rubble"))
        pl, ct0 = PL.plant(**GAINS), CR.contact(model)
        pols = policies(s, out, dts, dt, "uniform", False)
        b = 1
        cl = TR.closed_loop(oracle, model, pols[b], out["x"][b], pl, R.FEEDFORWARD, CR.with_ground(ct0, g[b]), (MAPS["rubble"], place[b]))
        ref = PL.tight_solution(cl, pols[b], s0[b], xs[b], T)
        assert np.isfinite(ref).all()
        s.set_plant(**GAINS)
        s.set_contact()
        s.set_contact_instances(g)
        s.set_terrain_maps(ALL_MAPS)
        s.set_terrain_instances(place)
        r = s.rollout_policy(s0, xs, T, 1)
        assert (r["status"] == 0).all() and (r["steps"] < 10000).all()
        r2 = s.rollout_policy(s0, xs, T, 1, abs_tol=1e-10, rel_tol=1e-10)
        assert (r2["status"] == 0).all() and (r2["steps"] > r["steps"]).all() and (r2["steps"] < 10000).all()
        err = float(np.abs(r2["x"][b, 0] - ref).max())
        ratio = float((np.abs(r["x"][b, 0] - ref) / (1e-5 + 1e-3 * np.abs(ref))).max())
        print(f"T {T}: steps {r['steps']} rejected {r['rejected']} error / tolerance {ratio:.2f}; tight steps {r2['steps']} rejected {r2['rejected']} "
              f"tight error {err:.2e}")
        stamps = np.arange(N + 1) * dt
        kink = any(((stamps - la > s0[b]) & (stamps - la < s0[b] + T)).any() for la in (0.0, pl["lookahead"]))
        assert ratio <= (50.0 if kink else 10.0), (kink, ratio)
        assert err <= 1e-7, err
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------- 4. the paths without a terrain, bit for bit
def test_stored_and_inert_equals_a_handle_without_a_terrain(model, oracle):
    s, _, _, _, x0 = solved(model, False, "events")
    fresh, _, _, _, _ = solved(model, False, "events")
    try:
        s0 = S0["events"]
        xs = start(x0, False, 2)
        place, g = mixed(oracle, model, xs, ("ledge", "ramp", "rubble"))
        for h in (s, fresh):
            h.set_contact()
            h.set_contact_instances(g)
        for integrator in ("ode45", "rk4"):
            kw = dict(integrator=integrator, controller="feedback", initial_step=RK4_STEP if integrator == "rk4" else 0.015)
            fresh.clear_plant()
            flow = fresh.rollout_policy(s0, xs, D, 2, **kw)
            fresh.set_plant(**GAINS)
            ground = fresh.rollout_policy(s0, xs, D, 2, **kw)
            fresh.set_contact(enabled=False)
            torque = fresh.rollout_policy(s0, xs, D, 2, **kw)
            fresh.set_contact()
            s.set_plant(**GAINS)
            s.set_terrain_maps(ALL_MAPS)
            assert same(s.rollout_policy(s0, xs, D, 2, **kw), ground), "maps, no table"
            s.set_terrain_instances(place)
            on = s.rollout_policy(s0, xs, D, 2, **kw)
            assert (on["status"] == 0).all() and not same(on, ground), "terrain set"
            s.set_terrain_instances(None)
            assert same(s.rollout_policy(s0, xs, D, 2, **kw), ground), "table removed"
            s.set_terrain_instances(place)
            s.set_contact(enabled=False)
            assert same(s.rollout_policy(s0, xs, D, 2, **kw), torque), "contact off"
            s.set_contact()
            s.set_plant(kind="flow", **GAINS)
            assert same(s.rollout_policy(s0, xs, D, 2, **kw), flow), "kind flow"
            s.clear_plant()
            assert same(s.rollout_policy(s0, xs, D, 2, **kw), flow), "no plant"
            assert len(s.get_terrain_maps()) == 3 and s.get_terrain_instances(B)[2]["map"] == MAP_INDEX["rubble"]      # stored and inert
            s.set_plant(**GAINS)
            assert same(s.rollout_policy(s0, xs, D, 2, **kw), on), "the terrain survived hsqp_plant_set / _clear and hsqp_contact_set"
            s.clear_terrain()
            assert same(s.rollout_policy(s0, xs, D, 2, **kw), ground), "cleared"
            assert s.get_terrain_maps() == [] and all(p["map"] == -1 for p in s.get_terrain_instances(B))
    finally:
        s.close()
        fresh.close()


def test_run_is_bit_identical_with_and_without_a_terrain(model, oracle):
    """The MPC never sees the map: an SQP iteration with a terrain resident equals one without, bit for bit."""
    x0, x, u, par, dt = problem(model, False, 5)
    s = HipSqpSolver(model, max_nodes=N, max_batch=B)
    twin = HipSqpSolver(model, max_nodes=N, max_batch=B)
    try:
        place, g = mixed(oracle, model, x0, ("ledge", "ramp", "rubble"))
        s.set_plant(**GAINS)
        s.set_contact()
        s.set_contact_instances(g)
        s.set_terrain_maps(ALL_MAPS)
        s.set_terrain_instances(place)
        a, b = s.run(x0, x, u, par, dt), twin.run(x0, x, u, par, dt)
        assert all(np.array_equal(a[k], b[k]) for k in ("x", "u"))
        r = s.rollout_policy(S0["uniform"], x0, D, 1, integrator="rk4", initial_step=RK4_STEP)
        assert (r["status"] == 0).all()
        for h in (s, twin):
            h.iterate(1, take_step=True)
        a, b = s.download(), twin.download()
        assert all(np.array_equal(a[k], b[k]) for k in ("x", "u", "dx", "du"))
        assert len(s.get_terrain_maps()) == 3                       # ... and the terrain survived the uploads
    finally:
        s.close()
        twin.close()


# ---------------------------------------------------------------------------------------------- 8. batch behaviour
def test_every_instance_equals_its_solo_rollout_and_chained_calls_equal_one_call(model, oracle):
    s, _, _, _, x0 = solved(model, False, "events")
    try:
        s0 = S0["events"]
        xs = start(x0, False, 4)
        place, g = mixed(oracle, model, xs)
        s.set_plant(**GAINS)
        s.set_contact()
        s.set_contact_instances(g)
        s.set_terrain_maps(ALL_MAPS)
        s.set_terrain_instances(place)
        rs = {c: s.rollout_policy(s0, xs, D, 2, controller=c) for c in ("feedforward", "feedback")}
        assert all((r["status"] == 0).all() for r in rs.values())
        # two half-duration calls equal one call
        c0 = np.array([0.0, 2.0 ** -5, 2.0 ** -4])
        d = 2.0 ** -7
        for integrator in ("ode45", "rk4"):
            kw = dict(integrator=integrator, controller="feedback", initial_step=RK4_STEP if integrator == "rk4" else 0.015)
            r = s.rollout_policy(c0, xs, 2 * d, 2, **kw)
            assert (r["status"] == 0).all()
            a = s.rollout_policy(c0, xs, d, 1, **kw)
            b = s.rollout_policy(c0 + d, a["x"][:, 0].copy(), d, 1, **kw)
            assert np.array_equal(a["x"][:, 0], r["x"][:, 0]) and np.array_equal(a["u"][:, 0], r["u"][:, 0]), integrator
            assert np.array_equal(b["x"][:, 0], r["x"][:, 1]) and np.array_equal(b["u"][:, 0], r["u"][:, 1]), integrator
            assert np.array_equal(a["steps"] + b["steps"], r["steps"])
    finally:
        s.close()
    for b in (0, 2):
        solo, _, _, _, _ = solved(model, False, "events", rows=slice(b, b + 1))
        try:
            solo.set_plant(**GAINS)
            solo.set_contact()
            solo.set_contact_instances(g[b:b + 1])
            solo.set_terrain_maps(ALL_MAPS)
            solo.set_terrain_instances(place[b:b + 1])
            for c, r in rs.items():
                r1 = solo.rollout_policy(s0[b:b + 1], xs[b:b + 1], D, 2, controller=c)
                for k in KEYS:
                    assert np.array_equal(r1[k], r[k][b:b + 1]), (b, c, k)
        finally:
            solo.close()


# ---------------------------------------------------------------------------------------------- the resident loop
def test_the_loop_on_the_ledge_equals_the_calls_it_replaces(model, oracle):
    case = loop_case(model, batch=B)
    s = HipSqpSolver(model, max_nodes=N, max_batch=B, linesearch=True, riccati="serial")
    try:
        place, g = mixed(oracle, model, case["x0"], ("ledge", "ledge", "ledge"), mus=(0.3, 0.6, 1.0))
        s.set_plant(**GAINS)
        s.set_contact()
        s.set_contact_instances(g)
        loop_start(s, model, case)
        plain = s.loop_run(3)
        s.set_terrain_maps(ALL_MAPS)
        s.set_terrain_instances(place)
        want = by_hand(s, model, case, 3, "feedforward")         # the terrain survives the uploads
        loop_start(s, model, case)                               # ... and the start of a loop
        got = s.loop_run(3)
        assert [p["map"] for p in s.get_terrain_instances(B)] == [MAP_INDEX["ledge"]] * B
    finally:
        s.close()
    assert got["cycles_done"] == 3 and np.isfinite(got["x"]).all()
    assert np.array_equal(got["x"], want["x"]) and np.array_equal(got["u"], want["u"])
    assert not np.array_equal(got["x"], plain["x"])


# ---------------------------------------------------------------------------------------------- 9. errors
def test_errors(model, cmodel):
    nx, ny, cell, hs = HipSqpSolver.pack_terrain_maps(ALL_MAPS)
    ip = C.POINTER(C.c_int32)
    c = HipSqpSolver(cmodel, max_nodes=N, max_batch=B)
    try:
        for call in (lambda: c.set_terrain_maps(ALL_MAPS), lambda: c.set_terrain_instances([None]), lambda: c.set_terrain_instances(None), c.clear_terrain,
                     c.get_terrain_maps, lambda: c.get_terrain_instances(1), lambda: c.terrain_height(np.zeros((1, 1, 2)))):
            with pytest.raises(HsqpError) as ei:
                call()
            assert ei.value.code == _abi.ERR_BAD_ARG and "hsqp_terrain_" in str(ei.value) and "whole-body handles only" in str(ei.value)
    finally:
        c.close()
    s = HipSqpSolver(model, max_nodes=N, max_batch=B)
    err = lambda: s.lib.hsqp_last_error(s.h).decode()   # noqa: E731

    def refused_maps(what, n=3, nx=nx, ny=ny, cell=cell, hs=hs):
        rc = s.lib.hsqp_terrain_set_maps(s.h, n, None if nx is None else nx.ctypes.data_as(ip), None if ny is None else ny.ctypes.data_as(ip),
                                         None if cell is None else cell.ctypes.data_as(_dp), None if hs is None else hs.ctypes.data_as(_dp))
        assert rc == _abi.ERR_BAD_ARG and "hsqp_terrain_set_maps" in err() and what in err(), (what, rc, err())

    def refused_table(what, place, batch=None, entry="hsqp_terrain_set_instances"):
        tab = HipSqpSolver.pack_terrain_instances(place)
        rc = getattr(s.lib, entry)(s.h, len(tab) if batch is None else batch, tab)
        assert rc == _abi.ERR_BAD_ARG and entry in err() and what in err(), (what, rc, err())
    try:
        assert s.get_terrain_maps() == [] and [p["map"] for p in s.get_terrain_instances(B)] == [-1] * B
        refused_maps("n_maps", n=-1)
        refused_maps("n_maps", n=_abi.TERRAIN_MAX_MAPS + 1)
        for k in ("nx", "ny", "cell", "hs"):
            refused_maps("null", **{k: None})
        for bad in (1, _abi.TERRAIN_MAX_DIM + 1, 0, -3):
            refused_maps("map 1: nx or ny", nx=np.array([nx[0], bad, nx[2]], np.int32))
            refused_maps("map 2: nx or ny", ny=np.array([ny[0], ny[1], bad], np.int32))
        for bad in (0.0, -0.01, np.nan, np.inf):
            refused_maps("map 0: cell", cell=np.array([bad, cell[1], cell[2]]))
        for bad in (np.nan, np.inf, -np.inf):
            h2 = hs.copy()
            h2[4 + 7] = bad                                            # (inside the ledge: map 1)
            refused_maps("map 1: non-finite height", hs=h2)
        assert s.get_terrain_maps() == []                              # no refused call left maps behind
        # placements before any map: only the plane
        refused_table("instance 0: map", [TR.placement(index=0)])
        s.set_terrain_instances([None, None])
        s.set_terrain_maps(ALL_MAPS)
        got = s.get_terrain_maps()
        assert len(got) == 3 and all(np.array_equal(a[0], b[0]) and a[1] == b[1] for a, b in zip(got, ALL_MAPS))
        ok = [TR.placement((0.1, 0.2), 0.7, 2), None, TR.placement((0.0, 0.0), 0.0, 0)]
        refused_table("batch", ok, batch=0)
        refused_table("batch", ok + [None], batch=B + 1)
        refused_table("batch", ok, batch=B + 1, entry="hsqp_terrain_set_instances_device")
        assert s.lib.hsqp_terrain_set_instances(s.h, -1, None) == _abi.ERR_BAD_ARG and "batch" in err()
        refused_table("instance 1: reserved", [ok[0], dict(ok[0], reserved=1)])
        refused_table("instance 2: map", [ok[0], ok[1], TR.placement(index=3)])
        refused_table("instance 0: map", [TR.placement(index=-2)])
        for bad in (np.nan, np.inf):
            refused_table("instance 0: non-finite", [TR.placement((bad, 0.0), 0.0, 1)])
            refused_table("instance 1: non-finite", [ok[0], TR.placement((0.0, bad), 0.0, 1)])
            refused_table("instance 0: non-finite", [TR.placement((0.0, 0.0), bad, 1)])
        s.set_terrain_instances(ok)
        back = s.get_terrain_instances(B)
        assert [p["map"] for p in back] == [2, -1, 0] and back[0]["origin"] == (0.1, 0.2) and back[0]["yaw"] == 0.7
        # fewer maps than the resident table refers to
        refused_maps("refers to map 2", n=2)
        refused_maps("refers to map 2", n=0)
        assert len(s.get_terrain_maps()) == 3
        s.set_terrain_instances(ok[1:])                                 # (the table now refers to map 0 only)
        s.set_terrain_maps(ALL_MAPS[:1])
        assert len(s.get_terrain_maps()) == 1 and [p["map"] for p in s.get_terrain_instances(B)] == [-1, 0, -1]
        # the evaluation and the read-back
        z = np.zeros((B + 1, 2, 2))
        for entry in ("hsqp_terrain_eval", "hsqp_terrain_eval_device"):
            f = getattr(s.lib, entry)
            assert f(s.h, 1, 1, None, None, None) == _abi.ERR_BAD_ARG and entry in err() and "null" in err()
            for batch in (0, B + 1):
                assert f(s.h, batch, 2, z.ctypes.data_as(_dp), None, None) == _abi.ERR_BAD_ARG and entry in err() and "batch" in err()
            for n_pts in (0, -1, (1 << 24) + 1):
                assert f(s.h, 1, n_pts, z.ctypes.data_as(_dp), None, None) == _abi.ERR_BAD_ARG and entry in err() and "n_pts" in err()
        tab = HipSqpSolver.pack_terrain_instances(ok)
        assert s.lib.hsqp_terrain_get_instances(s.h, B, None) == _abi.ERR_BAD_ARG and "hsqp_terrain_get_instances" in err() and "null" in err()
        for batch in (0, B + 1):
            assert s.lib.hsqp_terrain_get_instances(s.h, batch, tab) == _abi.ERR_BAD_ARG and "batch" in err()
        assert s.lib.hsqp_terrain_get_maps(s.h, None, None, None, None, None, 0) == _abi.ERR_BAD_ARG and "hsqp_terrain_get_maps" in err() and "null" in err()
        n1, few = np.zeros(1, np.int32), np.zeros(3)
        assert s.lib.hsqp_terrain_get_maps(s.h, n1.ctypes.data_as(ip), None, None, None, few.ctypes.data_as(_dp), 3) == _abi.ERR_BAD_ARG and "max_heights" in err()
        # a table through the _device entry is not read back: an index out of range is clamped by the kernel (here: to the only map, and to the plane)
        wild = table_doubles([TR.placement((0.0, 0.0), 0.0, 9), TR.placement((0.0, 0.0), 0.0, -7), TR.placement((0.0, 0.0), 0.0, 0)])
        dt = DeviceBuffer(wild.shape)
        try:
            dt.upload(wild)
            s.set_terrain_instances_device(B, dt.ptr.value)
            xy = np.tile(np.array([[0.2, 0.1]]), (B, 1, 1))
            hgt, nrm = s.terrain_height(xy)
            assert hgt[0, 0] == hgt[2, 0] != 0.0 and hgt[1, 0] == 0.0 and tuple(nrm[1, 0]) == (0.0, 0.0, 1.0)
        finally:
            dt.free()
        s.clear_terrain()
        assert s.get_terrain_maps() == [] and [p["map"] for p in s.get_terrain_instances(B)] == [-1] * B
    finally:
        s.close()
