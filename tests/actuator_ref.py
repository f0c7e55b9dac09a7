"""TEST HELPER: numpy restatement of the actuator model on the torque plant (include/hsqp_actuator.h) on top of tests/plant_ref.py (and
tests/contact_ref.py for the ground), written from the header's text:

  command   (q_p, v_p, tau_ff, W_p): period 0 — steps 1-2 of hsqp_plant.h at the evaluation; period > 0 — sampled at the last tick, held
  tau_cmd = tau_ff + kp (q_p - q) + kd (v_p - v)   at the plant's current (q, v)
  tau_act = clip(tau_cmd, -limit, +limit);  tau_pas = -damping v - friction v / sqrt(v^2 + v_s^2);  tau = tau_act + tau_pas
  ticks     T_k = s0 + k period (one product, one sum); a tick strictly inside a sample interval is a break point; a tick on an event, a push
            edge or a sample time samples once; a sample time is not a tick
  record    (tau_cmd, tau_act, tau_pas) at the final state of the last sample under the command in force (held: the last tick's before the end)

The integrators, the push edges and the grid's events are those of plant_ref / push_ref / rollout_ref, unchanged."""
import numpy as np

import contact_ref as CT
import plant_ref as PL
import push_ref as P
import rollout_ref as R
from wb_humanoid_mpc_amd import _abi

NX, NU, NV, NJ = _abi.NX, _abi.NU, _abi.NV, _abi.NJ


def actuator(command_period=0.002, effort_limit=np.inf, damping=0.0, friction=0.0, friction_velocity=0.01):
    """The setting as a dict of arrays (the header's defaults)."""
    b = lambda v: np.broadcast_to(np.asarray(v, float), (NJ,)).copy()   # noqa: E731
    return dict(command_period=float(command_period), effort_limit=b(effort_limit), damping=b(damping), friction=b(friction),
                friction_velocity=float(friction_velocity))


def joint_law(ac, pl, cmd, x):
    """(tau, tau_cmd, tau_act, tau_pas) [23] each of the command cmd = (q_p, v_p, tau_ff, W_p) at the plant state x."""
    qp, vp, tff, _ = cmd
    q, v = x[6:NV], x[NV + 6:]
    tau_cmd = (tff + pl["kp"] * (qp - q)) + pl["kd"] * (vp - v)
    tau_act = np.where(tau_cmd > ac["effort_limit"], ac["effort_limit"], np.where(tau_cmd < -ac["effort_limit"], -ac["effort_limit"], tau_cmd))
    vs = ac["friction_velocity"]
    tau_pas = -ac["damping"] * v - ac["friction"] * v / np.sqrt(v * v + vs * vs)
    return tau_act + tau_pas, tau_cmd, tau_act, tau_pas


def command(oracle, pol, xt, pl, controller, s, x):
    """The joint command of time s and the measured state x: steps 1-2 of hsqp_plant.h."""
    xp, up = PL.policy(pol, xt, pl, controller, s, x)
    return xp[6:NV].copy(), xp[NV + 6:].copy(), PL.tau_ff(oracle, xp, up), up[:12].copy()


class ClosedLoop:
    """f(s, x, active pushes) -> xdot [58] of the torque plant under the actuator model; `held`: the command in force (period > 0), set by
    sample().  ct: the ground of contact_ref (None: the plant without one, which applies the command's wrenches)."""

    def __init__(self, oracle, model, pol, xt, pl, controller, ac, ct=None, exact_feet=True):
        self.oracle, self.model, self.pol, self.xt, self.pl, self.controller, self.ac, self.ct, self.exact_feet = oracle, model, pol, xt, pl, controller, ac, ct, exact_feet
        self.held = None

    def sample(self, s, x):
        self.held = command(self.oracle, self.pol, self.xt, self.pl, self.controller, s, x)

    def in_force(self, s, x):
        return self.held if self.ac["command_period"] > 0.0 else command(self.oracle, self.pol, self.xt, self.pl, self.controller, s, x)

    def __call__(self, s, x, active):
        cmd = self.in_force(s, x)
        tau = joint_law(self.ac, self.pl, cmd, x)[0]
        extra = PL.push_force(self.oracle, self.model, x, active, self.exact_feet) if active else None
        if self.ct is not None:
            return np.r_[x[NV:], CT.accel(self.oracle, self.model, x, tau, self.pl["armature"], self.ct, extra)]
        vd, _ = PL.accel(self.oracle, x, tau, cmd[3], self.pl["armature"], extra)
        return np.r_[x[NV:], vd]

    def record(self, s, x):
        return np.array(joint_law(self.ac, self.pl, self.in_force(s, x), x)[1:])


def ticks_upto(s0, period, end):
    """[T_k] with T_k < end."""
    out, k = [], 0
    while s0 + k * period < end:
        out.append(s0 + k * period)
        k += 1
    return out


def rollout(cl, pol, st, s0, x0, duration, n, pushes=(), stamp0=0.0, log=None, segments=None):
    """plant_ref.rollout on the closed loop cl with the ticks of its actuator: (x [n][58], u [n][35], status, accepted steps, rejected steps,
    record [3][23] — NaN unless the status is OK).  segments (a list): gets (start, end, sampled) of every segment."""
    period = cl.ac["command_period"]
    pushes = list(pushes)
    live = P.edges(pushes, stamp0)
    run = PL._Run(pol, st, log)
    run.cl = cl
    x = np.asarray(x0, dtype=float).copy()
    xs, us = np.full((n, NX), np.nan), np.full((n, NU), np.nan)
    stat, ta, k = R.OK, s0, 0          # k: the next tick that has not been sampled
    for j in range(n):
        tb = R.sample_time(s0, duration, j, n)
        if stat == R.OK:
            cap = st["max_steps_per_second"] * max(tb - ta, 1.0)
            acc, t = [0], ta
            while stat == R.OK and t < tb:
                te = P.next_break(pol, live, t, tb)
                sampled = False
                if period > 0.0:
                    if s0 + k * period == t:
                        cl.sample(t, x)
                        sampled = True
                        k += 1
                    assert s0 + k * period > t
                    te = min(te, s0 + k * period)
                run.active = [p for e0, e1, p in live if e0 <= t < e1]
                stat, x = run.segment(x, t, te, cap, acc)
                if segments is not None:
                    segments.append((t, te, sampled))
                t = te
            if stat == R.OK:
                u = pol.control(tb, x, st["controller"])
                if not np.isfinite(u).all():
                    stat = R.NONFINITE
        if stat == R.OK:
            xs[j] = x
            us[j] = u
        ta = tb
    rec = cl.record(s0 + duration, x) if stat == R.OK else np.full((3, NJ), np.nan)
    return xs, us, stat, run.nacc, run.nrej, rec


def tight_solution(cl, pol, s0, x0, duration, pushes=(), steps_per_second=2 ** 15):
    """plant_ref.tight_solution with the ticks: RK4 with steps of at most 1 / steps_per_second, piece by piece between the break points (the ticks
    among them, the command sampled at each); a stage at the end time of a piece is evaluated one ulp before it.  Returns (x at the end, the set of
    saturated joints of every piece's start and end as a list of frozensets)."""
    period = cl.ac["command_period"]
    live = P.edges(list(pushes), 0.0)
    x = np.asarray(x0, dtype=float).copy()
    t, tb, k = s0, s0 + duration, 0
    sat = []

    def saturated(s, xx):
        r = cl.record(s, xx)
        return frozenset(np.nonzero(np.abs(r[0]) > cl.ac["effort_limit"])[0].tolist())
    while t < tb:
        te = P.next_break(pol, live, t, tb)
        if period > 0.0:
            if s0 + k * period == t:
                cl.sample(t, x)
                k += 1
            te = min(te, s0 + k * period)
        active = [p for e0, e1, p in live if e0 <= t < e1]
        left = np.nextafter(te, t)

        def f(s, xx):
            return cl(min(s, left), xx, active)
        n = max(1, int(np.ceil((te - t) * steps_per_second)))
        h = (te - t) / n
        for i in range(n):
            a = t + i * h
            sat.append(saturated(min(a, left), x))
            k1 = f(a, x)
            k2 = f(a + 0.5 * h, x + 0.5 * h * k1)
            k3 = f(a + 0.5 * h, x + 0.5 * h * k2)
            k4 = f(a + h, x + h * k3)
            x = x + h / 6.0 * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
        sat.append(saturated(left, x))
        t = te
    return x, sat
