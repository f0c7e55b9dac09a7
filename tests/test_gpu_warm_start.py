"""The receding-horizon warm start built on the device (hsqp_reference::warm_start) on the MI355X: after every SHIFT upload the resident
linearisation trajectory equals the adaptor's host warm start (reference.host_warm_start) applied to the downloaded previous solution, bit
for bit; a loop driven by SHIFT equals the same loop driven by host warm starts through HSQP_WARM_CALLER; the C++ adaptor gives the same
MPC_BASE::run results with deviceWarmStart on and off; rejected requests leave the resident solution shiftable."""
import os
import subprocess

import numpy as np
import pytest

from wb_humanoid_mpc_amd import _abi
from wb_humanoid_mpc_amd.reference import (centroidal_velocity_command_targets, cold_start, event_grid, host_warm_start, mode_to_contact_flags,
                                           pack_reference, pad_targets, raw_stamps, swing_config, tile_gait, velocity_command_targets)
from wb_humanoid_mpc_amd.solver import HipSqpSolver, HsqpError

pytestmark = pytest.mark.gpu

GAITS = ("walk", "trot", "slow_trot", "fast_walk")


def device_mass(m):
    """DevModel::total_mass: the bodies' masses summed in order (hsqp_host.h)."""
    s = 0.0
    for b in m.desc.bodies:
        s += b.mass
    return s


class Loop:
    """B instances of one receding-horizon MPC loop: gaits with different phases, velocity-command targets."""

    def __init__(self, m, B, cent=False, horizon=1.0, event_nodes=True, gaits=GAITS):
        self.m, self.B, self.cent, self.horizon, self.event_nodes = m, B, cent, horizon, event_nodes
        self.nx = _abi.CNX if cent else _abi.NX
        self.dt = m.sqp["dt"]
        self.schedules = [tile_gait(m.gaits[gaits[b % len(gaits)]], 0.25 + 0.37 * b / B, 8.0) for b in range(B)]
        x0 = m.initial_state.copy()
        tg = (centroidal_velocity_command_targets if cent else velocity_command_targets)(m, (0.3, 0.0, 0.7925, 0.0), 0.0, x0, 4.0)
        self.ref = pack_reference(self.schedules, [pad_targets(tg) if cent else tg] * B)
        self.x_init = np.zeros((B, _abi.NX))
        self.x_init[:, :self.nx] = x0[:self.nx]
        self.mass = device_mass(m)

    def grid(self, t0):
        """(N, dt argument, node_times or None, raw stamps [B][N+1]) at t0: event grids of equal N (each instance's horizon stretched by
        fractions of dt until its node count matches), or the uniform grid."""
        if not self.event_nodes:
            N = int(round(self.horizon / self.dt))
            return N, self.dt, None, np.tile(t0 + np.arange(N + 1) * self.dt, (self.B, 1))
        grids = lambda h: [event_grid(t0, t0 + h, self.dt, s.event_times) for s in self.schedules]  # noqa: E731
        target = max(len(d) for d, _ in grids(self.horizon))
        while True:
            out = []
            for s in self.schedules:
                for j in range(64):
                    d, nt = event_grid(t0, t0 + self.horizon + j * self.dt / 8, self.dt, s.event_times)
                    if len(d) == target:
                        out.append((d, nt))
                        break
            if len(out) == self.B:
                dts, nts = np.stack([d for d, _ in out]), np.stack([nt for _, nt in out])
                return target, dts, nts, raw_stamps(dts, nts)
            target += 1

    def flags(self, node_times, N, t0):
        nt = node_times if node_times is not None else np.tile(t0 + np.arange(N + 1) * self.dt, (self.B, 1))
        return np.array([[mode_to_contact_flags(s.mode_at(t)) for t in nt[b]] for b, s in enumerate(self.schedules)], dtype=float)

    def upload_warm(self, s, t0, x_init, mode):
        N, dts, nt, st = self.grid(t0)
        s.upload_reference_warm(x_init, N, dts, t0, *self.ref, swing_config(self.m), node_times=nt, mode=mode)
        return N, nt, st

    def upload_host(self, s, t0, x_init, prev):
        """The adaptor's path: host warm start from the downloaded previous solution, uploaded through HSQP_WARM_CALLER."""
        N, dts, nt, st = self.grid(t0)
        x, u = host_warm_start(self.mass, x_init, st, self.flags(nt, N, t0), prev, self.nx)
        s.upload_reference(x_init, x, u, dts, t0, *self.ref, swing_config(self.m), node_times=nt)
        return N, nt, st


def contact_of(s):
    return s.device_params()[:, :, _abi.P_CONTACT:_abi.P_CONTACT + 2]


def check_resident_warm_start(loop, s, x_init, st, prev):
    assert np.array_equal(s.stamps(), st)
    x, u = s.device_trajectory()
    xr, ur = host_warm_start(loop.mass, x_init, st, contact_of(s), prev, loop.nx)
    assert np.array_equal(x, xr) and np.array_equal(u, ur), (np.abs(x - xr).max(), np.abs(u - ur).max())
    return x, u


@pytest.mark.parametrize("shape", ["events_4", "uniform_256x100"])
def test_shift_upload_equals_the_host_warm_start(model, shape):
    events = shape == "events_4"
    B = 4 if events else 256
    loop = Loop(model, B, horizon=1.0 if events else 100 * model.sqp["dt"], event_nodes=events)
    s = HipSqpSolver(model, max_nodes=64 if events else 100, max_batch=B, linesearch=True)
    try:
        t, x_init, prev, Ns = 0.0, loop.x_init.copy(), None, set()
        for c in range(4 if events else 3):
            N, nt, st = loop.upload_warm(s, t, x_init, "cold" if c == 0 else "shift")
            Ns.add(N)
            x, u = check_resident_warm_start(loop, s, x_init, st, prev)
            if c == 0:   # COLD = reference.cold_start with the device's mass
                class M:
                    nu, total_mass = _abi.NU, loop.mass
                par = s.device_params()
                for b in range(B):
                    xc, uc = cold_start(M, x_init[b], par[b])
                    assert np.array_equal(x[b], xc) and np.array_equal(u[b], uc)
            else:
                covered = st <= prev["times"][..., -1:]
                assert covered.any() and (~covered).any()       # both halves of the warm start are exercised
            s.iterate(1, take_step=True, linesearch=True)
            out = s.download()
            prev = dict(times=st, x=out["x"], u=out["u"])
            xs, _, _ = s.evaluate_policy(np.full(B, 0.02))
            x_init = xs
            t += 0.02                                        # not a multiple of dt
        if events:
            assert len(Ns) > 1                               # events enter and leave the horizon: N changes between cycles
    finally:
        s.close()


@pytest.mark.parametrize("formulation", ["wb", "centroidal"])
def test_shift_loop_equals_the_host_warm_start_loop(model, cmodel, formulation):
    cent = formulation == "centroidal"
    m = cmodel if cent else model
    loop = Loop(m, 4, cent=cent, horizon=0.6 if cent else 1.0)
    dev = HipSqpSolver(m, max_nodes=64, max_batch=4, linesearch=True)
    host = HipSqpSolver(m, max_nodes=64, max_batch=4, linesearch=True)
    try:
        t, x_init, prev = 0.0, loop.x_init.copy(), None
        for c in range(5):
            loop.upload_warm(dev, t, x_init, "cold" if c == 0 else "shift")
            N, nt, st = loop.upload_host(host, t, x_init, prev)
            for s in (dev, host):
                s.iterate(1, take_step=True, linesearch=True)
            a, b = dev.download(), host.download()
            for k in ("x", "u", "alpha", "step_type"):
                assert np.array_equal(a[k], b[k]), (c, k)
            assert a["perf_after"] == b["perf_after"], c
            prev = dict(times=st, x=b["x"], u=b["u"])
            xs, _, _ = dev.evaluate_policy(np.full(4, 0.02))
            x_init = xs
            if cent:
                x_init[:, _abi.CNX:] = 0.0
            t += 0.02
    finally:
        dev.close(); host.close()


@pytest.mark.parametrize("formulation", ["wb", "centroidal"])
def test_adaptor_device_warm_start_equals_the_host_path(tmp_path, model, cmodel, formulation):
    from test_adaptor import LIBDIR, ROOT, write_case
    cent = formulation == "centroidal"
    m = cmodel if cent else model
    nx = _abi.CNX if cent else _abi.NX
    schedule = tile_gait(m.gaits["walk"], 0.3, 6.0)
    x0 = m.initial_state.copy()
    targets = (centroidal_velocity_command_targets if cent else velocity_command_targets)(m, (0.3, 0.0, 0.7925, 0.0), 0.0, x0, 3.0)
    write_case(tmp_path, m, schedule, targets, x0, 0.6 if cent else 1.05, 0.02, 3, nx)
    exe = tmp_path / "adaptor_warm_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "tests", "stubs", "ocs2"), "-I", os.path.join(LIBDIR, "host"),
                           "-I", os.path.join(ROOT, "tests", "adaptor"), os.path.join(ROOT, "tests", "adaptor_warm", "adaptor_warm_driver.cpp"),
                           "-L", LIBDIR, "-lhsqp_hip", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-o", str(exe)])
    image = os.path.join(LIBDIR, "data", "g1_centroidal.json" if cent else "g1_wb.json")
    outs = []
    for flag in (0, 1):
        out = tmp_path / f"out{flag}.txt"
        r = subprocess.run([str(exe), image, str(tmp_path / "case.txt"), str(out), str(flag)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and f"deviceWarmStart={flag}" in r.stdout, (r.stdout, r.stderr)
        outs.append(out.read_text())
    assert outs[0].count("\n") > 3 * 10 and outs[0] == outs[1]


def test_rejected_shift_requests_leave_the_solution_shiftable(model):
    loop = Loop(model, 2, horizon=0.7, event_nodes=False)
    s = HipSqpSolver(model, max_nodes=32, max_batch=2, linesearch=True)
    bad = lambda: pytest.raises(HsqpError, match="hsqp error -1")  # noqa: E731
    try:
        with bad():                                               # fresh handle: nothing to shift
            loop.upload_warm(s, 0.0, loop.x_init, "shift")
        t, st = 0.0, None

        def solve_and_shift(t, st):
            s.iterate(1, take_step=True, linesearch=True)
            out = s.download()
            t += 0.02
            N, nt, st2 = loop.upload_warm(s, t, loop.x_init, "shift")
            check_resident_warm_start(loop, s, loop.x_init, st2, dict(times=st, x=out["x"], u=out["u"]))
            return t, st2

        _, _, st = loop.upload_warm(s, t, loop.x_init, "cold")
        t, st = solve_and_shift(t, st)
        s.iterate(1, take_step=True, linesearch=True)
        N, dts, nt, _ = loop.grid(t + 0.02)
        n_ev, ev, seq, tt, ts = loop.ref
        cases = [
            lambda: s._upload_reference(1, N, loop.x_init[:1], None, None, dts, t + 0.02, n_ev[:1], ev[:1], seq[:1], tt[:1], ts[:1],
                                        swing_config(model), 0.0, True, None, _abi.WARM_SHIFT),                     # another batch size
            lambda: s._upload_reference(2, N, loop.x_init, np.zeros((2, N + 1, _abi.NX)), np.zeros((2, N, _abi.NU)), dts, t + 0.02, *loop.ref,
                                        swing_config(model), 0.0, True, None, _abi.WARM_SHIFT),                     # x_traj / u_traj given
            lambda: s._upload_reference(2, N, loop.x_init, None, None, dts, t + 0.02, *loop.ref, swing_config(model), 0.0, True, None, 3),
        ]
        for case in cases:
            before = s.download()
            with bad():
                case()
            after = s.download()                                  # the resident solution is untouched ...
            assert all(np.array_equal(before[k], after[k]) for k in ("x", "u"))
            t += 0.02                                             # ... and shifts as it would have
            _, _, st2 = loop.upload_warm(s, t, loop.x_init, "shift")
            check_resident_warm_start(loop, s, loop.x_init, st2, dict(times=st, x=after["x"], u=after["u"]))
            st = st2
            s.iterate(1, take_step=True, linesearch=True)
        # hsqp_upload forgets the stamps: SHIFT is refused until a problem comes through hsqp_upload_reference again
        x, u = s.device_trajectory()
        s.upload(loop.x_init, x, u, s.device_params(), loop.dt)
        s.iterate(1, take_step=True, linesearch=True)
        with bad():
            loop.upload_warm(s, t + 0.02, loop.x_init, "shift")
        _, _, st = loop.upload_warm(s, t, loop.x_init, "cold")
        solve_and_shift(t, st)
    finally:
        s.close()
