"""TEST HELPER: the reference of the per-instance inertial variations of the torque plant (include/hsqp_inertia.h): the UNCHANGED oracle on a
MERGED model.  For one instance every body's (s m, com, s I) and its payloads are combined into one rigid body — summed mass, mass-weighted centre
of mass, the parallel-axis theorem about the new centre of mass —, the description is rebuilt with G1Model._build_desc and a second Oracle is made
of it: its full_dynamics gives M and nle of the varied plant.  The closed loop is plant_ref.closed_loop (contact_ref's on the ground,
actuator_ref's under the actuator model) with the accelerations on the merged oracle and tau_ff on the nominal one."""
import copy

import numpy as np

import actuator_ref as A
import contact_ref as CR
import plant_ref as PL
from wb_humanoid_mpc_amd import _abi
from wb_humanoid_mpc_amd.model import G1Model

NX, NU, NV, NJ, NB = _abi.NX, _abi.NU, _abi.NV, _abi.NJ, _abi.NB
TORSO, L_ELBOW = 15, 19   # links of the G1 tree (tests/test_plant.py)


def payload(body, mass, com=(0.0, 0.0, 0.0), inertia=(0.0,) * 6):
    """One payload as the binding takes it: inertia = (xx, xy, xz, yy, yz, zz) about its own centre of mass, link axes."""
    return dict(body=int(body), mass=float(mass), com=[float(v) for v in com], inertia=[float(v) for v in inertia])


# the two payloads of the issue: 5 kg on the torso, a 1 kg point mass on the left elbow link
PAYLOADS = [payload(TORSO, 5.0, (0.05, 0.0, 0.2), (0.02, 0.0, 0.0, 0.03, 0.0, 0.01)), payload(L_ELBOW, 1.0, (0.1, 0.0, 0.0))]


def scales(rng):
    """Link scales log-uniform in [0.8, 1.25]."""
    return np.exp(rng.uniform(np.log(0.8), np.log(1.25), NB))


def variations(rng):
    """The three instances of the tests: neutral, scales only, scales + both payloads, as (mass_scale [24], payloads)."""
    return [(np.ones(NB), []), (scales(rng), []), (scales(rng), PAYLOADS)]


def sym(i6):
    xx, xy, xz, yy, yz, zz = i6
    return np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]])


def merged_bodies(raw, mass_scale, payloads):
    """(mass, com [3], inertia [3][3]) of every body after the merge."""
    out = []
    for i, b in enumerate(raw["bodies"]):
        parts = [(mass_scale[i] * b["mass"], np.array(b["com"], float), mass_scale[i] * np.array(b["inertia"], float).reshape(3, 3))]
        parts += [(p["mass"], np.array(p["com"], float), sym(p["inertia"])) for p in payloads if p["body"] == i]
        m = sum(p[0] for p in parts)
        c = sum(p[0] * p[1] for p in parts) / m
        inertia = np.zeros((3, 3))
        for mp, cp, ip in parts:
            d = cp - c
            inertia += ip + mp * (d @ d * np.eye(3) - np.outer(d, d))
        out.append((m, c, inertia))
    return out


def merged_model(model, mass_scale, payloads):
    """A model whose description carries the merged bodies (everything else the nominal model's)."""
    raw = copy.deepcopy(model.raw)
    for b, (m, c, inertia) in zip(raw["bodies"], merged_bodies(model.raw, mass_scale, payloads)):
        b["mass"], b["com"], b["inertia"] = float(m), [float(v) for v in c], [float(v) for v in inertia.reshape(9)]
    raw["total_mass"] = float(sum(b["mass"] for b in raw["bodies"]))
    m2 = copy.copy(model)
    m2.raw, m2.total_mass, m2.desc = raw, raw["total_mass"], G1Model._build_desc(raw)
    return m2


def merged_oracle(model, mass_scale, payloads):
    from hsqp_oracle import Oracle
    return Oracle(merged_model(model, mass_scale, payloads))


def accel(oracle, varied, model, x, tau, W, armature, ct=None, extra=None):
    """vd [29] of the varied plant: plant_ref.accel / contact_ref.accel with the mass matrix and the bias of the merged oracle `varied`.  The
    Jacobians of the wrenches, the pushes and the contact points are kinematic: they come from the nominal `oracle`, as on the nominal plant."""
    if ct is None:
        return PL.accel(varied, x, tau, W, armature, extra)[0]
    g = CR.generalised_force(CR.forces(oracle, model, x, ct))
    return PL.accel(varied, x, tau, np.zeros(12), armature, g if extra is None else g + extra)[0]


def closed_loop(oracle, varied, model, pol, xt, pl, controller, ct=None, exact_feet=True):
    """plant_ref.closed_loop (ct: contact_ref.closed_loop, on the ground) with the accelerations on the merged oracle `varied` and tau_ff on the
    nominal `oracle`: the mismatch being modelled."""
    def f(s, x, active):
        xp, up = PL.policy(pol, xt, pl, controller, s, x)
        tau = (PL.tau_ff(oracle, xp, up) + pl["kp"] * (xp[6:NV] - x[6:NV])) + pl["kd"] * (xp[NV + 6:] - x[NV + 6:])
        extra = PL.push_force(oracle, model, x, active, exact_feet) if active else None
        return np.r_[x[NV:], accel(oracle, varied, model, x, tau, up[:12], pl["armature"], ct, extra)]
    return f


class ActuatedClosedLoop(A.ClosedLoop):
    """actuator_ref.ClosedLoop on the varied plant: the command (tau_ff among it) on the nominal oracle, the accelerations on the merged one."""

    def __init__(self, oracle, varied, model, pol, xt, pl, controller, ac, ct=None, exact_feet=True):
        super().__init__(oracle, model, pol, xt, pl, controller, ac, ct, exact_feet)
        self.varied = varied

    def __call__(self, s, x, active):
        cmd = self.in_force(s, x)
        tau = A.joint_law(self.ac, self.pl, cmd, x)[0]
        extra = PL.push_force(self.oracle, self.model, x, active, self.exact_feet) if active else None
        return np.r_[x[NV:], accel(self.oracle, self.varied, self.model, x, tau, cmd[3], self.pl["armature"], self.ct, extra)]
