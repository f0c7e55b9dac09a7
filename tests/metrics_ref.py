"""TEST HELPER: the numpy restatement of the per-instance episode metrics of the resident loop (include/hsqp_metrics.h, csrc/hsqp_metrics.h): the
sample of one cycle, and the closing / reopening of a record.  Scalars are Python floats (IEEE double, never fused), every per-joint and
per-corner sum runs in index order, so everything agrees with the kernel source exactly apart from sin / cos (math's against the device's)."""
import math

import numpy as np

from wb_humanoid_mpc_amd import _abi

NV, NJ = _abi.NV, _abi.NJ
INT_FIELDS = ("cycles", "first_cycle", "end_cause", "torque_samples", "ground_samples", "flight_samples", "touchdowns", "saturated_samples",
              "saturated_joint_samples", "rollout_steps", "rollout_rejected")
FIELDS = tuple(name for name, _ in _abi.Metrics._fields_)
# which fields are exact restatements (counts, copies, minima, maxima, products of the same doubles in a fixed order) and which carry sin / cos
TRIG_FIELDS = ("vel_err_sq", "vel_err_max")
GROUND_FIELDS = ("load_sum", "load_max", "penetration_max")


def empty():
    r = {k: 0.0 for k in FIELDS if k not in INT_FIELDS}
    r.update({k: 0 for k in INT_FIELDS})
    r.update(first_cycle=-1, end_cause=_abi.METRICS_END_OPEN, touchdowns=[0, 0], start_xy=[0.0, 0.0], end_xy=[0.0, 0.0], height_min=math.inf, height_max=-math.inf)
    r["_feet"] = [0, 0]
    return r


def sample(r, cycle, x_before, x, cmd, period, perf, steps, rejected, torque=None, ground=None):
    """One cycle's sample into the open record r.  perf: (cost, dynamics_sse, equality_sse); torque: (tau_cmd [23], tau_act [23], effort_limit [23]) or
    None; ground: (force [8][3], penetration [8]) or None."""
    x, x0, cmd = [float(v) for v in x], [float(v) for v in x_before], [float(v) for v in cmd]
    T = float(period)
    if r["cycles"] == 0:
        r["first_cycle"], r["start_xy"] = int(cycle), [x0[0], x0[1]]
    r["cycles"] += 1
    r["duration"] = float(r["cycles"]) * T
    c, s = math.cos(x[3]), math.sin(x[3])
    wx, wy = c * cmd[0] - s * cmd[1], s * cmd[0] + c * cmd[1]
    ex, ey = x[NV] - wx, x[NV + 1] - wy
    e2 = ex * ex + ey * ey
    r["vel_err_sq"] += e2
    r["vel_err_max"] = max(r["vel_err_max"], math.sqrt(e2))
    ew, eh = x[NV + 3] - cmd[3], x[2] - cmd[2]
    r["yaw_rate_err_sq"] += ew * ew
    r["height_err_sq"] += eh * eh
    r["height_min"], r["height_max"] = min(r["height_min"], x[2]), max(r["height_max"], x[2])
    r["tilt_max"] = max(r["tilt_max"], max(abs(x[4]), abs(x[5])))
    dx, dy = x[0] - x0[0], x[1] - x0[1]
    r["path_length"] += math.sqrt(dx * dx + dy * dy)
    r["end_xy"] = [x[0], x[1]]
    if torque is not None:
        tc, ta, lim = ([float(v) for v in a] for a in torque)
        sat, sq, ratio, wp, wa = 0, 0.0, 0.0, 0.0, 0.0
        for j in range(NJ):
            ac = abs(tc[j])
            if ac > lim[j]:
                sat += 1
            q = 0.0 if lim[j] == math.inf else (ac / lim[j] if lim[j] != 0.0 else (math.inf if ac > 0.0 else math.nan))
            if q > ratio:
                ratio = q
            sq += ta[j] * ta[j]
            p = ta[j] * x[NV + 6 + j]
            wp += p if p > 0.0 else 0.0
            wa += abs(p)
        r["torque_samples"] += 1
        r["saturated_joint_samples"] += sat
        r["saturated_samples"] += 1 if sat else 0
        r["tau_sq"] += sq
        r["tau_ratio_max"] = max(r["tau_ratio_max"], ratio)
        r["work_pos"] += T * wp
        r["work_abs"] += T * wa
    if ground is not None:
        force, pen = np.asarray(ground[0], dtype=float).reshape(8, 3), np.asarray(ground[1], dtype=float).reshape(8)
        loaded = [int(force[4 * f:4 * f + 4].any()) for f in range(2)]
        load, dmax = 0.0, r["penetration_max"]
        for i in range(8):
            load += float(force[i, 2])
            if float(pen[i]) > dmax:
                dmax = float(pen[i])
        if not loaded[0] and not loaded[1]:
            r["flight_samples"] += 1
        for f in range(2):
            if r["ground_samples"] > 0 and loaded[f] and not r["_feet"][f]:
                r["touchdowns"][f] += 1
            r["_feet"][f] = loaded[f]
        r["ground_samples"] += 1
        r["load_sum"] += load
        r["load_max"] = max(r["load_max"], load)
        r["penetration_max"] = dmax
    cost, dyn, eq = (float(v) for v in perf)
    r["cost_sum"] += cost
    r["dynamics_sse_max"] = max(r["dynamics_sse_max"], dyn)
    r["equality_sse_max"] = max(r["equality_sse_max"], eq)
    r["rollout_steps"] += int(steps)
    r["rollout_rejected"] += int(rejected)


class Records:
    """The two records (CURRENT, PREVIOUS) of B instances and the boundary rules of include/hsqp_metrics.h."""

    def __init__(self, B):
        self.cur, self.prev = [empty() for _ in range(B)], [empty() for _ in range(B)]

    def close(self, b, cause):
        if self.cur[b]["cycles"] == 0:
            return
        self.cur[b]["end_cause"] = int(cause)
        self.prev[b], self.cur[b] = self.cur[b], empty()

    def cycle(self, b, verdict, alive_before, cycle, **sample_args):
        """Instance b behind the rollout of `cycle`: verdict (_abi.EP_*) is the triage's, alive_before whether it was ALIVE before the cycle."""
        if verdict != _abi.EP_ALIVE:
            self.close(b, verdict)
        elif alive_before:
            sample(self.cur[b], cycle, **sample_args)

    def arrays(self, which="current"):
        """The records as the binding's dict of arrays (solver.metrics_dict)."""
        recs = self.cur if which == "current" else self.prev
        return {k: np.array([r[k] for r in recs], dtype=np.int64 if k in INT_FIELDS else np.float64) for k in FIELDS}


def assert_records(got, want, exact=None, close=None, where=""):
    """got / want: dicts of arrays.  Every field in `exact` (default: all but those in `close`) bit for bit; close: {field: (rtol, atol)}."""
    close = close or {}
    for k in FIELDS:
        if k in close:
            rtol, atol = close[k]
            assert np.allclose(got[k], want[k], rtol=rtol, atol=atol), (where, k, got[k], want[k])
        elif exact is None or k in exact:
            assert np.array_equal(got[k], want[k]), (where, k, got[k], want[k])
