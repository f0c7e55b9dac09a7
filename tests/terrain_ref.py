"""TEST HELPER: numpy restatement of the height-map terrain under the torque plant (include/hsqp_terrain.h), kept in two parts that know nothing of the
robot — height_normal (steps 1-7 of the header) and force_law (the force at one point over a ground of height g and normal n) — and the kinematics of
tests/contact_ref.py UNCHANGED (points, frame_velocities, jacobians).  forces / accel / closed_loop are built from them as contact_ref.py builds its own.

A terrain is (map, place): map = dict(H [ny][nx], cell), place = dict(origin (x, y), yaw); None: the horizontal plane.  Every function computes in the
dtype of `dtype` (float64; np.longdouble for the measurement of the reference's own rounding)."""
import numpy as np

import contact_ref as CR
import plant_ref as PL
from wb_humanoid_mpc_amd import _abi

NX, NU, NV, NJ = _abi.NX, _abi.NU, _abi.NV, _abi.NJ
NPTS = CR.NPTS


def terrain_map(H, cell):
    return dict(H=np.asarray(H, dtype=float), cell=float(cell))


def placement(origin=(0.0, 0.0), yaw=0.0, index=0):
    """index: the map's number in the handle's list (the binding's `map`)."""
    return dict(map=int(index), origin=(float(origin[0]), float(origin[1])), yaw=float(yaw))


def _cell(a, n, T):
    """(i, s, clamped) of one grid coordinate: clamped into [0, n - 1] before it becomes an integer."""
    clamped = False
    if a < 0:
        a, clamped = T(0), True
    elif a > n - 1:
        a, clamped = T(n - 1), True
    i = min(int(a), n - 2)
    return i, a - T(i), clamped


def height_normal(mp, place, X, Y, dtype=np.float64):
    """(hm, n [3], (hx, hy)) of the map mp placed by `place` under the world point (X, Y); mp None: the plane.  A non-finite coordinate: hm NaN."""
    T = dtype
    if mp is None:
        return T(0), np.array([0, 0, 1], dtype=T), (T(0), T(0))
    H, cell = np.asarray(mp["H"], dtype=T), T(mp["cell"])
    ny, nx = H.shape
    cy, sy = np.cos(T(place["yaw"])), np.sin(T(place["yaw"]))
    dx, dy = T(X) - T(place["origin"][0]), T(Y) - T(place["origin"][1])
    a, b = (cy * dx + sy * dy) / cell, (cy * dy - sy * dx) / cell
    if not (np.isfinite(a) and np.isfinite(b)):
        return T(np.nan), np.array([0, 0, 1], dtype=T), (T(0), T(0))
    i, s, ca = _cell(a, nx, T)
    j, t, cb = _cell(b, ny, T)
    h00, h10, h01, h11 = H[j, i], H[j, i + 1], H[j + 1, i], H[j + 1, i + 1]
    h0, h1 = h00 + s * (h10 - h00), h01 + s * (h11 - h01)
    hm = h0 + t * (h1 - h0)
    gx = T(0) if ca else ((h10 - h00) + t * ((h11 - h01) - (h10 - h00))) / cell
    gy = T(0) if cb else (h1 - h0) / cell
    hx, hy = cy * gx - sy * gy, sy * gx + cy * gy
    r = np.sqrt((1 + hx * hx) + hy * hy)
    return hm, np.array([-hx / r, -hy / r, 1 / r], dtype=T), (hx, hy)


def force_law(P, Pdot, ground, ct, dtype=np.float64):
    """(d, F [3], class) at a point of world position P and velocity Pdot over the ground (g, n): g the ground's height under the point, n its unit
    normal.  Classes as in contact_ref.py: 'a' force, 'b' d <= 0, 'c' clamped at zero."""
    T = dtype
    P, Pdot = np.asarray(P, dtype=T), np.asarray(Pdot, dtype=T)
    g, n = T(ground[0]), np.asarray(ground[1], dtype=T)
    d = (g - P[2]) * n[2]
    if not d > 0:
        return d, np.zeros(3, dtype=T), "b"
    vn = (Pdot[0] * n[0] + Pdot[1] * n[1]) + Pdot[2] * n[2]
    fn = T(ct["stiffness"]) * d * (1 + T(ct["damping"]) * -vn)
    if not fn > 0:
        return d, np.zeros(3, dtype=T), "c"
    vt = Pdot - vn * n
    ft = -T(ct["mu"]) * fn * vt / np.sqrt(((vt[0] * vt[0] + vt[1] * vt[1]) + vt[2] * vt[2]) + T(ct["slip_velocity"]) ** 2)
    return d, fn * n + ft, "a"


def forces(oracle, model, x, ct, terrain, velocity="fd", dtype=np.float64):
    """contact_ref.forces on the terrain: dict(P, Pdot, d, f, J, cls, g [8], n [8][3], grad [8][2])."""
    q, v = np.asarray(x[:NV], dtype=float), np.asarray(x[NV:], dtype=float)
    P, J = CR.points(oracle, model, q), CR.jacobians(oracle, model, q)
    Pdot = J @ v if velocity == "fd" else CR.frame_velocities(oracle, model, x)
    mp, place = terrain if terrain is not None else (None, None)
    d, f, cls = np.zeros(NPTS, dtype=dtype), np.zeros((NPTS, 3), dtype=dtype), []
    g, n, grad = np.zeros(NPTS, dtype=dtype), np.zeros((NPTS, 3), dtype=dtype), np.zeros((NPTS, 2), dtype=dtype)
    for i in range(NPTS):
        hm, n[i], grad[i] = height_normal(mp, place, P[i, 0], P[i, 1], dtype)
        g[i] = dtype(ct["ground_height"]) + hm
        d[i], f[i], c = force_law(P[i], Pdot[i], (g[i], n[i]), ct, dtype)
        cls.append(c)
    return dict(P=P, Pdot=Pdot, d=d, f=f, J=J, cls=cls, g=g, n=n, grad=grad)


def accel(oracle, model, x, tau, armature, ct, terrain, extra=None):
    gf = CR.generalised_force(forces(oracle, model, x, ct, terrain))
    if extra is not None:
        gf = gf + extra
    return PL.accel(oracle, x, tau, np.zeros(12), armature, gf)[0]


def closed_loop(oracle, model, pol, xt, pl, controller, ct, terrain, exact_feet=True):
    """contact_ref.closed_loop on the terrain: f(s, x, active pushes) -> xdot [58]."""
    def f(s, x, active):
        xp, up = PL.policy(pol, xt, pl, controller, s, x)
        tau = (PL.tau_ff(oracle, xp, up) + pl["kp"] * (xp[6:NV] - x[6:NV])) + pl["kd"] * (xp[NV + 6:] - x[NV + 6:])
        extra = PL.push_force(oracle, model, x, active, exact_feet) if active else None
        return np.r_[x[NV:], accel(oracle, model, x, tau, pl["armature"], ct, terrain, extra)]
    return f


# ---- the maps of the tests
def ramp_map(deg=5.0, cell=0.5):
    """2 x 2: a plane rising along the map's x by tan(deg)."""
    r = np.tan(np.radians(deg)) * cell
    return terrain_map([[0.0, r], [0.0, r]], cell)


def ledge_map(height=0.03, cell=0.01):
    """5 x 4 (nx = 5, ny = 4): flat at 0 for x <= 2 cell, one cell of slope, flat at `height` from x = 3 cell on."""
    row = [0.0, 0.0, 0.0, height, height]
    return terrain_map([row] * 4, cell)


def rubble_map(seed=20240, n=6, amplitude=0.01, cell=0.04):
    return terrain_map(np.random.default_rng(seed).uniform(-amplitude, amplitude, (n, n)), cell)
