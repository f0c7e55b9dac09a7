"""TEST HELPER: the float64 reference of EVERY torque-plant configuration of the rollout (ground x terrain x actuator model x inertia table), composed once
from the restatements already there.  It states no physics of its own and only routes:

  command, tau_ff    actuator_ref.command / plant_ref.policy, plant_ref.tau_ff      on the NOMINAL oracle
  joint torque       actuator_ref.joint_law under the actuator model, else the PD law as plant_ref.closed_loop writes it (the same parentheses)
  ground             terrain_ref.forces on a map, contact_ref.forces on the plane (points and Jacobians: the nominal oracle), else the command's wrenches
  pushes             plant_ref.push_force                                            on the nominal oracle
  M, nle, the solve  plant_ref.accel                                                 on the merged oracle `varied` (inertia_ref.merged_oracle), else the nominal one
  integration        actuator_ref.rollout / tight_solution under the actuator model (the ticks), else plant_ref's

tests/test_rollout_variants.py holds it to the seven older closed loops bit for bit."""
import numpy as np

import actuator_ref as A
import contact_ref as CR
import plant_ref as PL
import terrain_ref as TR
from wb_humanoid_mpc_amd import _abi

NX, NU, NV, NJ = _abi.NX, _abi.NU, _abi.NV, _abi.NJ


class ClosedLoop:
    """f(s, x, active pushes) -> xdot [58].  varied: the merged oracle of the instance (None: the nominal body); ct: the contact setting of the instance
    (None: no ground); terrain: (map, placement) of the instance over that ground (None: the plane); ac: the actuator setting (None: the PD law, continuous).
    sample / in_force / record as actuator_ref.ClosedLoop (the record needs ac)."""

    def __init__(self, oracle, model, pol, xt, pl, controller, *, varied=None, ct=None, terrain=None, ac=None, exact_feet=True):
        assert terrain is None or ct is not None, "a terrain lies under a ground"
        self.oracle, self.model, self.pol, self.xt, self.pl, self.controller = oracle, model, pol, xt, pl, controller
        self.varied, self.ct, self.terrain, self.ac, self.exact_feet = varied, ct, terrain, ac, exact_feet
        self.held = None

    def sample(self, s, x):
        self.held = A.command(self.oracle, self.pol, self.xt, self.pl, self.controller, s, x)

    def in_force(self, s, x):
        if self.ac is not None and self.ac["command_period"] > 0.0:
            return self.held
        return A.command(self.oracle, self.pol, self.xt, self.pl, self.controller, s, x)

    def ground_force(self, x):
        """sum J_P^T f [29] of the ground under the state x (None: no ground)."""
        if self.terrain is not None:
            return CR.generalised_force(TR.forces(self.oracle, self.model, x, self.ct, self.terrain))
        if self.ct is not None:
            return CR.generalised_force(CR.forces(self.oracle, self.model, x, self.ct))
        return None

    def __call__(self, s, x, active):
        pl = self.pl
        if self.ac is not None:
            cmd = self.in_force(s, x)
            tau, W = A.joint_law(self.ac, pl, cmd, x)[0], cmd[3]
        else:
            xp, up = PL.policy(self.pol, self.xt, pl, self.controller, s, x)
            tau = (PL.tau_ff(self.oracle, xp, up) + pl["kp"] * (xp[6:NV] - x[6:NV])) + pl["kd"] * (xp[NV + 6:] - x[NV + 6:])
            W = up[:12]
        extra = PL.push_force(self.oracle, self.model, x, active, self.exact_feet) if active else None
        dyn = self.varied if self.varied is not None else self.oracle
        g = self.ground_force(x)
        if g is None:
            return np.r_[x[NV:], PL.accel(dyn, x, tau, W, pl["armature"], extra)[0]]
        if extra is not None:
            g = g + extra
        return np.r_[x[NV:], PL.accel(dyn, x, tau, np.zeros(12), pl["armature"], g)[0]]

    def record(self, s, x):
        return np.array(A.joint_law(self.ac, self.pl, self.in_force(s, x), x)[1:])


def rollout(cl, pol, st, s0, x0, duration, n, pushes=(), stamp0=0.0):
    """(x [n][58], u [n][35], status, accepted steps, rejected steps, record [3][23] or None): actuator_ref.rollout under the actuator model, else
    plant_ref.rollout (no record)."""
    if cl.ac is not None:
        return A.rollout(cl, pol, st, s0, x0, duration, n, pushes, stamp0)
    return PL.rollout(cl, pol, st, s0, x0, duration, n, pushes, stamp0) + (None,)


def tight_solution(cl, pol, s0, x0, duration, pushes=(), steps_per_second=2 ** 15):
    """(x at the end, the saturated sets or None): actuator_ref.tight_solution under the actuator model, else plant_ref.tight_solution."""
    if cl.ac is not None:
        return A.tight_solution(cl, pol, s0, x0, duration, pushes, steps_per_second)
    return PL.tight_solution(cl, pol, s0, x0, duration, pushes, steps_per_second), None
