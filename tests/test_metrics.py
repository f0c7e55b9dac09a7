"""Per-instance episode metrics of the resident loop (include/hsqp_metrics.h, csrc/hsqp_metrics.h) on the CPU: the header, the exported entry points
and the binding's struct; the host build of the kernel source (tests/metrics/metrics_emu.cpp, one-lane context, -ffp-contract=off) against the numpy
restatement tests/metrics_ref.py over a few hundred random samples fed cycle by cycle; the ground group against tests/contact_ref.py on flat ground;
the boundary rules, driven together with the triage of the episode sources (the host build of tests/test_episode.py); and a program of its own under
the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import contact_ref as CR
import metrics_ref as MR
import rollout_emu as E
from test_contact import EPS, contact_struct, ground_array
from test_episode import Batch, emu as episode_emu, emu_triage, np_verdict, random_cycle, settings  # noqa: F401  (episode_emu is a fixture)
from wb_humanoid_mpc_amd import _abi, solver
from wb_humanoid_mpc_amd.solver import metrics_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wb_humanoid_mpc_amd", "csrc")
NX, NV, NJ, CMD_N = _abi.NX, _abi.NV, _abi.NJ, _abi.CMD_N
_dp, _ip, _mp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(_abi.Metrics)
ALIVE = _abi.EP_ALIVE
# sums that involve sin / cos: at most a few hundred terms, each a few ulp
TRIG = {k: (1e-13, 0.0) for k in MR.TRIG_FIELDS}


# ---------------------------------------------------------------------------------------------- 1. header, library, binding
def _header_functions():
    src = open(os.path.join(ROOT, "include", "hsqp_metrics.h")).read()
    src = src[src.index("#ifndef HSQP_METRICS_H"):]
    return sorted(set(re.findall(r"\b(hsqp_[a-z_]+)\s*\(", src)))


OFFSET_FIELDS = ("cycles", "end_cause", "touchdowns", "rollout_rejected", "duration", "end_xy", "height_min", "tau_ratio_max", "penetration_max", "equality_sse_max")


def test_header_library_and_binding_agree(tmp_path):
    assert _header_functions() == sorted(_abi.METRICS_ENTRY_POINTS)
    syms = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "wb_humanoid_mpc_amd", "libhsqp_hip.so")], text=True)
    names = {line.split()[-1] for line in syms.splitlines() if line.strip()}
    lib = solver.load_library()
    for n in _abi.METRICS_ENTRY_POINTS:
        assert n in names, n
        assert getattr(lib, n).argtypes is not None, n
    body = ('#include <stddef.h>\n#include <stdio.h>\n#include "hsqp_metrics.h"\nint main(void){printf("%zu ' + "%zu " * len(OFFSET_FIELDS) + '%d %d %d %d %d\\n", sizeof(hsqp_metrics),' +
            "".join(f" offsetof(hsqp_metrics, {k})," for k in OFFSET_FIELDS) +
            " HSQP_METRICS_CURRENT, HSQP_METRICS_PREVIOUS, HSQP_METRICS_END_OPEN, HSQP_METRICS_END_HOST, HSQP_ABI_VERSION);return 0;}\n")
    M = _abi.Metrics
    want = [C.sizeof(M)] + [getattr(M, k).offset for k in OFFSET_FIELDS] + [_abi.METRICS_CURRENT, _abi.METRICS_PREVIOUS, _abi.METRICS_END_OPEN, _abi.METRICS_END_HOST, 7]
    for name, cc, std in (("sz.c", "gcc", "-std=c99"), ("sz.cpp", "g++", "-std=c++17")):      # the header as C and as C++
        (tmp_path / name).write_text(body)
        subprocess.check_call([cc, std, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(tmp_path / name), "-o", str(tmp_path / "sz")])
        assert [int(v) for v in subprocess.check_output([str(tmp_path / "sz")]).split()] == want, cc
    assert C.sizeof(M) == 35 * 8 and all(f[1] in (C.c_int64, C.c_double) or C.sizeof(f[1]) == 16 for f in M._fields_)      # 8-byte fields only
    assert _abi.ABI_VERSION == 7 and lib.hsqp_abi_version() == 7


def test_null_handle():
    lib = solver.load_library()
    out = (_abi.Metrics * 2)()
    ids = np.zeros(2, np.int32).ctypes.data_as(_ip)
    assert lib.hsqp_loop_metrics_enable(None) == _abi.ERR_BAD_ARG
    assert lib.hsqp_loop_metrics_disable(None) == _abi.ERR_BAD_ARG
    assert lib.hsqp_loop_metrics_restart(None, 1, ids) == _abi.ERR_BAD_ARG
    assert lib.hsqp_loop_metrics(None, _abi.METRICS_CURRENT, out) == _abi.ERR_BAD_ARG
    assert lib.hsqp_loop_metrics_device(None, _abi.METRICS_PREVIOUS, out) == _abi.ERR_BAD_ARG


def test_summary():
    r = MR.Records(3)
    for c in range(4):
        MR.sample(r.cur[0], c, np.zeros(NX), np.r_[0.1 * (c + 1), np.zeros(NX - 1)], np.zeros(4), 0.5, (1.0, 0.0, 0.0), 3, 1,
                  torque=(np.ones(NJ), np.ones(NJ), np.full(NJ, np.inf)))
    MR.sample(r.cur[1], 0, np.zeros(NX), np.zeros(NX), np.zeros(4), 0.5, (1.0, 0.0, 0.0), 3, 1)
    r.close(1, _abi.EP_FAILED_BOUNDS)
    sm = solver.metrics_summary(r.arrays(), mass=2.0, gravity=-10.0)
    assert sm["instances"] == 3 and sm["survivors"] == 1 and sm["samples"] == 4 and sm["distance"] == pytest.approx(0.4)
    assert sm["rms_tracking"] == 0.0 and sm["cost_of_transport"] == pytest.approx(r.cur[0]["work_pos"] / (2.0 * 10.0 * 0.4))
    assert solver.metrics_summary(MR.Records(2).arrays(), 1.0) == dict(instances=2, survivors=0, samples=0, rms_tracking=None, distance=None, cost_of_transport=None)


# ---------------------------------------------------------------------------------------------- the host build of the kernel source
class MetCall(C.Structure):
    """met_call (tests/metrics/metrics_emu.h)"""
    _fields_ = [(k, C.c_int32) for k in ("B", "isolate", "cycle", "form")] + [("period", C.c_double), ("st", C.POINTER(_abi.EpisodeSettings)), ("it_status", _ip),
               ("perf", _dp), ("ro_status", _ip), ("xs", _dp), ("x_before", _dp), ("cmd", _dp), ("ep_state", _ip), ("steps", _ip), ("rejected", _ip),
               ("act_last", _dp), ("act_limit", _dp), ("rec", _mp), ("feet", _ip), ("contact", C.POINTER(_abi.ContactSettings)), ("ground", C.POINTER(_abi.ContactGround))]


def build_emu(path, *defines):
    lib = E.build(path, os.path.join("metrics", "metrics_emu.cpp"), "-ffp-contract=off", *defines)
    lib.met_open.argtypes = [C.c_int, _mp, _ip]
    lib.met_cycle.argtypes = [C.c_void_p, C.POINTER(MetCall)]
    lib.met_host_close.argtypes = [C.c_int, _ip, _mp, _ip]
    lib.met_ws_bytes.argtypes = [C.c_int]
    return lib


class Emu:
    """The host build, and the device arrays of B instances' records."""

    def __init__(self, lib, model, B):
        self.lib, self.h, self.B = lib, E.create(lib, model), B
        self.rec, self.feet = (_abi.Metrics * (2 * B))(), np.full(2 * B, 7, np.int32)
        lib.met_open(B, self.rec, self.feet.ctypes.data_as(_ip))

    def close(self):
        self.lib.emu_destroy(self.h)

    def cycle(self, cycle, period, xs, x_before, cmd, perf, steps, rejected, it_status=None, ro_status=None, st=None, ep_state=None, act=None, limit=None,
              form=0, contact=None, ground=None):
        B = self.B
        keep = [np.ascontiguousarray(a, dtype=np.float64) for a in (xs, x_before, cmd, perf)] + [np.ascontiguousarray(a, dtype=np.int32) for a in (steps, rejected)]
        keep += [np.zeros(B, np.int32) if a is None else np.ascontiguousarray(a, dtype=np.int32) for a in (it_status, ro_status)]
        c = MetCall(B=B, isolate=0 if st is None else 1, cycle=cycle, form=form, period=period)
        c.xs, c.x_before, c.cmd, c.perf = (a.ctypes.data_as(_dp) for a in keep[:4])
        c.steps, c.rejected, c.it_status, c.ro_status = (a.ctypes.data_as(_ip) for a in keep[4:8])
        if st is not None:
            keep.append(np.ascontiguousarray(ep_state, dtype=np.int32))
            c.st, c.ep_state = C.pointer(st), keep[-1].ctypes.data_as(_ip)
        if act is not None:
            keep += [np.ascontiguousarray(act, dtype=np.float64), np.ascontiguousarray(limit, dtype=np.float64)]
            c.act_last, c.act_limit = keep[-2].ctypes.data_as(_dp), keep[-1].ctypes.data_as(_dp)
        if form:
            keep += [contact, ground]
            c.contact = C.pointer(contact)
            if ground is not None:
                c.ground = C.cast(ground, C.POINTER(_abi.ContactGround))
        c.rec, c.feet = C.cast(self.rec, _mp), self.feet.ctypes.data_as(_ip)
        self.lib.met_cycle(self.h, C.byref(c))

    def host_close(self, ids=None):
        n = self.B if ids is None else len(ids)
        ids = None if ids is None else np.ascontiguousarray(ids, dtype=np.int32)
        self.lib.met_host_close(n, None if ids is None else ids.ctypes.data_as(_ip), C.cast(self.rec, _mp), self.feet.ctypes.data_as(_ip))

    def arrays(self, which="current"):
        all_ = metrics_dict(self.rec)
        return {k: v[(0 if which == "current" else 1)::2] for k, v in all_.items()}


@pytest.fixture(scope="module")
def emu_lib(tmp_path_factory):
    return build_emu(tmp_path_factory.mktemp("metrics") / "libmetrics_emu.so")


def random_sample(rng, B, x_prev):
    xs = x_prev + 0.05 * rng.standard_normal((B, NX))
    xs[:, 3] = rng.uniform(-3.0, 3.0, B)
    cmd = np.column_stack([rng.uniform(-0.5, 0.5, B), rng.uniform(-0.2, 0.2, B), rng.uniform(0.7, 0.8, B), rng.uniform(-0.3, 0.3, B)])
    perf = np.abs(rng.standard_normal((B, 4)))
    return xs, cmd, perf, rng.integers(1, 20, B).astype(np.int32), rng.integers(0, 4, B).astype(np.int32)


def check(emu, ref, where, close=None):
    for which in ("current", "previous"):
        MR.assert_records(emu.arrays(which), ref.arrays(which), close=dict(TRIG, **(close or {})), where=(where, which))


# ---------------------------------------------------------------------------------------------- 2. the sample against the restatement
@pytest.mark.parametrize("limits", [None, "finite", "infinite", "mixed"])
def test_samples_match_the_restatement(emu_lib, model, rng, limits):
    """B = 8 instances, 40 cycles: 320 samples.  Counts, copies, minima, maxima and the torque group (products and sums of the same doubles in index
    order) exactly; the two sums behind sin / cos to 1e-13 relative."""
    B, cycles, T = 8, 40, 1.0 / 60.0
    emu, ref = Emu(emu_lib, model, B), MR.Records(B)
    limit = None if limits is None else {"finite": np.full(NJ, 0.8), "infinite": np.full(NJ, np.inf), "mixed": np.where(np.arange(NJ) % 3 == 0, np.inf, 0.5)}[limits]
    try:
        check(emu, ref, "empty")
        assert (emu.feet == 0).all()
        x = rng.standard_normal((B, NX))
        for c in range(cycles):
            xs, cmd, perf, steps, rej = random_sample(rng, B, x)
            act = None if limit is None else rng.standard_normal((B, 3, NJ))
            emu.cycle(c, T, xs, x, cmd, perf, steps, rej, act=act, limit=limit)
            for b in range(B):
                ref.cycle(b, ALIVE, True, c, x_before=x[b], x=xs[b], cmd=cmd[b], period=T, perf=perf[b, 1:], steps=steps[b], rejected=rej[b],
                          torque=None if limit is None else (act[b, 0], act[b, 1], limit))
            x = xs
            if c % 13 == 12:
                check(emu, ref, c)
        check(emu, ref, "end")
        got = emu.arrays()
        assert (got["cycles"] == cycles).all() and (got["duration"] == cycles * T).all() and (got["torque_samples"] == (0 if limit is None else cycles)).all()
        if limits == "finite":
            assert (got["saturated_joint_samples"] > got["saturated_samples"]).all() and (got["saturated_samples"] > 0).all() and (got["tau_ratio_max"] > 1.0).all()
        if limits == "infinite":
            assert (got["saturated_samples"] == 0).all() and (got["tau_ratio_max"] == 0.0).all() and (got["tau_sq"] > 0.0).all()
    finally:
        emu.close()


# ---------------------------------------------------------------------------------------------- 2. the ground group against contact_ref
@pytest.mark.parametrize("form", [1, 2])
def test_ground_group_matches_the_contact_reference(emu_lib, model, oracle, rng, form):
    """Flat ground, 4 instances x 25 cycles; the ground of an instance 1 mm above the lowest sole corner of its first state, the base moved up and
    down by millimetres from cycle to cycle so that feet load, unload and fly.  The forces of the reference are tests/contact_ref.py's (closed-form
    velocities); the bound per force component is tests/test_contact.py's, A + A |f| with A = k 64 eps (|P_z| + |ground_height|) per point, summed
    over the corners of a sample: load_max to the largest sample's bound, load_sum to the bounds' sum; penetration_max to 64 eps of the same scale.
    Counts must agree exactly (a corner whose load class the bound could flip is asserted not to occur).  form 2: the terrain set with every instance
    on the plane."""
    B, cycles, T = 4, 25, 1.0 / 60.0
    emu, ref = Emu(emu_lib, model, B), MR.Records(B)
    try:
        base = np.tile(model.initial_state, (B, 1))
        base[:, 6:6 + NJ] += 0.01 * rng.standard_normal((B, NJ))
        base[:, 4:6] += 0.01 * rng.standard_normal((B, 2))
        ground = np.array([(float(CR.points(oracle, model, x[:NV])[:, 2].min() + 1e-3), 0.5 + 0.1 * b) for b, x in enumerate(base)])
        ct = CR.contact(model)
        cs, ga = contact_struct(ct), ground_array(ground)
        tol_sum, tol_max, tol_pen = np.zeros(B), np.zeros(B), np.zeros(B)
        x = base.copy()
        for c in range(cycles):
            xs, cmd, perf, steps, rej = random_sample(rng, B, base)
            xs[:, :NV] = base[:, :NV]
            xs[:, 2] += rng.uniform(-2e-3, 4e-3, B)
            xs[:, 4:6] += 0.01 * rng.standard_normal((B, 2))
            xs[:, 3] = base[:, 3]
            emu.cycle(c, T, xs, x, cmd, perf, steps, rej, form=form, contact=cs, ground=ga)
            for b in range(B):
                r = CR.forces(oracle, model, xs[b], CR.with_ground(ct, ground[b]), velocity="frame")
                scale = np.abs(r["P"][:, 2]) + abs(ground[b, 0])
                A = ct["stiffness"] * 64 * EPS * scale
                assert (np.abs(r["d"]) > 64 * EPS * scale).all()                     # no corner within the bound of touching: the classes cannot flip
                tol = float((A + A * np.linalg.norm(r["f"], axis=1)).sum())
                tol_sum[b] += tol
                tol_max[b] = max(tol_max[b], tol)
                tol_pen[b] = max(tol_pen[b], 64 * EPS * scale.max())
                ref.cycle(b, ALIVE, True, c, x_before=x[b], x=xs[b], cmd=cmd[b], period=T, perf=perf[b, 1:], steps=steps[b], rejected=rej[b], ground=(r["f"], r["d"]))
            x = xs
        got, want = emu.arrays(), ref.arrays()
        print("touchdowns", got["touchdowns"].tolist(), "flight", got["flight_samples"].tolist(), "load_max", got["load_max"].tolist())
        for k, tol in (("load_sum", tol_sum), ("load_max", tol_max), ("penetration_max", tol_pen)):
            err = np.abs(got[k] - want[k])
            print(k, "error", err.max(), "bounds from", tol.min())
            assert (err <= tol).all(), (k, err, tol)
        MR.assert_records(got, want, exact=[k for k in MR.FIELDS if k not in MR.GROUND_FIELDS and k not in TRIG], where="ground")
        assert (got["ground_samples"] == cycles).all() and got["touchdowns"].sum() > 0 and (got["load_max"] > 0.0).all()
    finally:
        emu.close()


def test_the_workspace_fits_the_lds(emu_lib):
    sizes = [emu_lib.met_ws_bytes(f) for f in range(3)]
    print("workspace bytes (no ground, plane, terrain):", sizes)
    assert sizes[0] <= 16 and sizes[0] < sizes[1] <= sizes[2] <= 65536


# ---------------------------------------------------------------------------------------------- 3. boundaries, with the triage
@pytest.mark.parametrize("policy", [_abi.EPISODE_PARK, _abi.EPISODE_RESET])
def test_boundary_rules_with_the_triage(emu_lib, episode_emu, model, rng, policy):
    """The metrics kernel in front of the triage, as loop_cycle queues them, on what tests/test_episode.py::random_cycle leaves (every cause, NaN and
    infinite data): a failure under PARK and under RESET, the host's reset (of alive, parked and empty instances), hsqp_loop_metrics_restart, closing
    an empty record, and cycles + first_cycle == fail_cycle for every record a failure closed."""
    B, cycles, T, box = 24, 30, 1.0 / 60.0, (0.7, 0.9, 0.3)
    st = settings(policy, *box)
    emu, ref, bt = Emu(emu_lib, model, B), MR.Records(B), Batch(rng, B)
    limit = np.full(NJ, 1.5)
    closed_by_failure = 0
    try:
        for c in range(cycles):
            it_status, perf, ro_status, xs = random_cycle(rng, B, *box)
            steps, rej, act = rng.integers(1, 20, B).astype(np.int32), rng.integers(0, 4, B).astype(np.int32), rng.standard_normal((B, 3, NJ))
            x_before, cmd, state = bt.x.copy(), bt.v_use.copy(), bt.state.copy()
            emu.cycle(c, T, xs, x_before, cmd, perf, steps, rej, it_status=it_status, ro_status=ro_status, st=st, ep_state=state, act=act, limit=limit)
            bt.x[:] = xs                                                     # step 5
            causes = emu_triage(episode_emu, st, c, bt, it_status, perf, ro_status, xs, None, None)
            for b in range(B):
                assert causes[b] == np_verdict(st, it_status[b], perf[b], ro_status[b], xs[b])
                had = ref.cur[b]["cycles"]
                ref.cycle(b, causes[b], state[b] == ALIVE, c, x_before=x_before[b], x=xs[b], cmd=cmd[b], period=T, perf=perf[b, 1:], steps=steps[b], rejected=rej[b],
                          torque=(act[b, 0], act[b, 1], limit))
                if causes[b] != ALIVE and had:
                    closed_by_failure += 1
                    p = ref.prev[b]
                    assert p["end_cause"] == causes[b] == bt.cause[b] and p["cycles"] + p["first_cycle"] == bt.fail_cycle[b] == c
                if causes[b] != ALIVE or state[b] != ALIVE:
                    assert ref.cur[b]["cycles"] == 0                         # a failed cycle is not accumulated, a parked instance accumulates nothing
            check(emu, ref, c)
            if c % 7 == 6:                                                   # the host: a reset of three instances (twice: the second closes empty records) ...
                ids = np.array([1, 5, 9], np.int32)
                for _ in range(2):
                    episode_emu.ep_host_reset(3, ids.ctypes.data_as(_ip), None, None, bt.x_reset.ctypes.data_as(_dp), *[getattr(bt, k).ctypes.data_as(_ip) for k in
                                              ("state", "cause", "fail_cycle", "n_failures", "n_episodes", "mode", "reset")], *[getattr(bt, k).ctypes.data_as(_dp) for k in
                                              ("x", "v_cmd", "v_filt", "v_use")])
                    emu.host_close(ids)
                    for b in ids:
                        ref.close(b, _abi.METRICS_END_HOST)
                    check(emu, ref, (c, "host reset"))
                emu.host_close([2, 6])                                       # ... and a restart of two others, their episodes untouched
                for b in (2, 6):
                    ref.close(b, _abi.METRICS_END_HOST)
                check(emu, ref, (c, "restart"))
        emu.host_close()                                                     # ids NULL: all
        for b in range(B):
            ref.close(b, _abi.METRICS_END_HOST)
        check(emu, ref, "restart all")
        assert closed_by_failure > 10 and (emu.arrays()["cycles"] == 0).all()
        prev = emu.arrays("previous")
        print("records closed by a failure:", closed_by_failure, "end causes now", np.bincount(prev["end_cause"] + 1, minlength=5).tolist())
        if policy == _abi.EPISODE_RESET:
            assert (prev["first_cycle"] > 0).any()                           # a record that opened behind a failure
    finally:
        emu.close()


def test_reverse_order_emulation_is_bit_identical(emu_lib, tmp_path, model, rng):
    """The items of every phase in reverse order (-DHSQP_EMU_REVERSE): the same records, so no phase depends on the order of its items."""
    rev = build_emu(tmp_path / "libmetrics_emu_rev.so", "-DHSQP_EMU_REVERSE")
    B, T = 3, 0.02
    st = settings(_abi.EPISODE_RESET, 0.7, 0.9, 0.3)
    cs = contact_struct(CR.contact(model, ground_height=0.0))
    a, b = Emu(emu_lib, model, B), Emu(rev, model, B)
    try:
        x = np.tile(model.initial_state, (B, 1))
        for c in range(6):
            xs, cmd, perf, steps, rej = random_sample(rng, B, x)
            xs[:, 2] = [0.8, 0.95 if c == 3 else 0.8, 0.8]                  # instance 1 leaves the box in cycle 3
            for e in (a, b):
                e.cycle(c, T, xs, x, cmd, perf, steps, rej, st=st, ep_state=np.zeros(B, np.int32), form=1, contact=cs)
            x = xs
        for which in ("current", "previous"):
            MR.assert_records(a.arrays(which), b.arrays(which), where=which)
        assert a.arrays("previous")["cycles"].tolist() == [0, 3, 0] and a.arrays()["first_cycle"].tolist() == [0, 4, 0]
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------------------------------------- 4. sanitizers: a program of its own
def test_every_path_under_sanitizers(tmp_path, model):
    exe, desc = tmp_path / "metrics_sanitize", tmp_path / "desc.bin"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "metrics", "metrics_emu.cpp"),
                           os.path.join(ROOT, "tests", "metrics", "metrics_sanitize.cpp"), "-o", str(exe)])
    desc.write_bytes(bytes(model.desc))
    out = subprocess.check_output([str(exe), str(desc)], text=True)
    assert out.strip() == "metrics ok"
