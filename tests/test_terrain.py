"""The height-map terrain under the torque plant (include/hsqp_terrain.h, csrc/hsqp_terrain.h) on the CPU: the header and the exported entry points, the
numpy restatement tests/terrain_ref.py checked against itself, and the host build of the kernel source (tests/terrain/terrain_emu.cpp, -ffp-contract=off)
against it — heights and normals, forces and penetrations, the paths without a terrain bit for bit, RK4 and ODE45 rollouts, batch behaviour — and a
sanitizer run of the index arithmetic as a program of its own.  Maps: a 2 x 2 ramp of 5 degrees placed with yaw 0.7, a 5 x 4 ledge of 3 cm over one 1 cm
cell, a 6 x 6 map from a fixed seed (amplitude 1 cm, cell 4 cm).  Three instances, 2^-6 s, the ground of every instance 1 mm above its lowest sole corner
at that corner's (X, Y) (place_under)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import contact_ref as CR
import plant_ref as PL
import rollout_emu as E
import rollout_ref as R
import terrain_ref as TR
from test_contact import EPS, RK4_STEP, contact_struct, ground_array
from test_plant import FD_TOL, plant_case, settings_struct
from test_rollout import rel, start_states
from wb_humanoid_mpc_amd import _abi, solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wb_humanoid_mpc_amd", "csrc")
LIBDIR = os.path.join(ROOT, "wb_humanoid_mpc_amd")
NX, NU, NV, NJ = _abi.NX, _abi.NU, _abi.NV, _abi.NJ
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_tp = C.POINTER(_abi.TerrainPlacement)
B = 3
D = 2.0 ** -6
GAINS = dict(kp=100.0, kd=2.0, armature=0.01, lookahead=0.005)   # tests/test_gpu_plant.py GAINS
U_TOL = 1e-9                 # tests/test_contact.py::test_rk4_rollout_matches_numpy
X_TOL = FD_TOL * D * 10      # tests/test_contact.py::test_rk4_rollout_matches_numpy: the reference carries a finite-difference Jacobian
# The RK4 step of the comparisons against the reference.  The step is the caller's choice (assumption C2 of include/hsqp_contact.h), and it has to integrate
# the stiffest mode stably: the Hunt-Crossley damping k d c grows with the penetration d, and on uneven ground a sole corner over a bump goes deeper than the
# 1 mm the instances start with (2.6 mm within 2^-6 s in tests/test_gpu_terrain.py's rubble case).  There RK4 at tests/test_contact.py's 1 ms is past its
# stability limit: measured on the host build with that case's policy, a perturbation of 1e-12 of the start state ends as 8.5e-3 at 1 ms, as 5.9e-11 at 0.5 ms
# and as 5.7e-11 at 0.25 ms — at 1 ms the comparison would hold two amplified roundings against each other.  A quarter of the plane's step: 64 steps.
TERRAIN_RK4_STEP = 2.5e-4


def _p(a):
    return None if a is None else a.ctypes.data_as(_dp)


# ---------------------------------------------------------------------------------------------- header, exports, null arguments
def test_header_compiles_and_the_library_exports_the_entry_points(tmp_path):
    src = tmp_path / "c.c"
    src.write_text('#include <stdio.h>\n#include "hsqp_terrain.h"\n'
                   'int main(void){ hsqp_terrain_placement p;\n'
                   ' int (*a)(hsqp_handle*, int, const int32_t*, const int32_t*, const double*, const double*) = hsqp_terrain_set_maps;\n'
                   ' int (*b)(hsqp_handle*, int, const hsqp_terrain_placement*) = hsqp_terrain_set_instances;\n'
                   ' int (*c)(hsqp_handle*, int, const hsqp_terrain_placement*) = hsqp_terrain_set_instances_device;\n'
                   ' int (*d)(hsqp_handle*) = hsqp_terrain_clear;\n'
                   ' int (*e)(hsqp_handle*, int32_t*, int32_t*, int32_t*, double*, double*, size_t) = hsqp_terrain_get_maps;\n'
                   ' int (*f)(hsqp_handle*, int, hsqp_terrain_placement*) = hsqp_terrain_get_instances;\n'
                   ' int (*g)(hsqp_handle*, int, int, const double*, double*, double*) = hsqp_terrain_eval;\n'
                   ' int (*i)(hsqp_handle*, int, int, const double*, double*, double*) = hsqp_terrain_eval_device;\n'
                   ' p.map = -1; p.reserved = 0; p.origin_x = p.origin_y = p.yaw = 0.0;\n'
                   ' printf("%d %d %d %d\\n", HSQP_ABI_VERSION, a != 0 && b != 0 && c != 0 && d != 0 && e != 0 && f != 0 && g != 0 && i != 0,'
                   ' (int)sizeof p + p.map, HSQP_TERRAIN_MAX_MAPS + HSQP_TERRAIN_MAX_DIM); return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "c.o")])
    syms = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(LIBDIR, "libhsqp_hip.so")], text=True)
    names = {line.split()[-1] for line in syms.splitlines() if line.strip()}
    lib = solver.load_library()
    for n in _abi.TERRAIN_ENTRY_POINTS:
        assert n in names and getattr(lib, n).argtypes is not None, n
    assert C.sizeof(_abi.TerrainPlacement) == 8 + 3 * 8
    assert (_abi.TERRAIN_MAX_MAPS, _abi.TERRAIN_MAX_DIM) == (16, 256)
    assert _abi.ABI_VERSION == 7           # additions only: no revision bump


def test_a_null_handle_is_a_bad_argument_and_the_binding_packs_the_tables():
    lib = solver.load_library()
    nx, ny, cell, hs = solver.HipSqpSolver.pack_terrain_maps([(np.zeros((4, 5)), 0.01), (np.ones((2, 2)), 0.5)])
    assert nx.tolist() == [5, 2] and ny.tolist() == [4, 2] and cell.tolist() == [0.01, 0.5] and hs.shape == (24,) and hs[20:].tolist() == [1.0] * 4
    tab = solver.HipSqpSolver.pack_terrain_instances([dict(map=1, origin=(0.25, -1.0), yaw=0.7), None])
    assert (tab[0].map, tab[0].reserved, tab[0].origin_x, tab[0].origin_y, tab[0].yaw) == (1, 0, 0.25, -1.0, 0.7) and tab[1].map == -1
    with pytest.raises(ValueError):
        solver.HipSqpSolver.pack_terrain_maps([(np.zeros(4), 0.01)])
    n, z = np.zeros(1, np.int32), np.zeros(8)
    assert lib.hsqp_terrain_set_maps(None, 2, nx.ctypes.data_as(_ip), ny.ctypes.data_as(_ip), _p(cell), _p(hs)) == _abi.ERR_BAD_ARG
    assert lib.hsqp_terrain_set_instances(None, 2, tab) == _abi.ERR_BAD_ARG
    assert lib.hsqp_terrain_set_instances_device(None, 2, tab) == _abi.ERR_BAD_ARG
    assert lib.hsqp_terrain_clear(None) == _abi.ERR_BAD_ARG
    assert lib.hsqp_terrain_get_maps(None, n.ctypes.data_as(_ip), None, None, None, None, 0) == _abi.ERR_BAD_ARG
    assert lib.hsqp_terrain_get_instances(None, 2, tab) == _abi.ERR_BAD_ARG
    assert lib.hsqp_terrain_eval(None, 1, 1, _p(z), _p(z), None) == _abi.ERR_BAD_ARG
    assert lib.hsqp_terrain_eval_device(None, 1, 1, _p(z), _p(z), None) == _abi.ERR_BAD_ARG


# ---------------------------------------------------------------------------------------------- the reference against itself
def rot(axis, angle):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def test_the_reference_height_is_the_closed_form_of_a_plane_under_any_yaw():
    """A map sampled from z = alpha xl + beta yl + c is reproduced by the bilinear patches exactly (up to rounding): under a placement (origin, yaw) the
    world height is c + (alpha, beta) . Rz(-yaw) (X - origin) and the world gradient Rz(yaw) (alpha, beta), at interior points of every cell."""
    rng = np.random.default_rng(5)
    al, be, c, cell = 0.21, -0.13, 0.4, 0.07
    ix, iy = np.meshgrid(np.arange(6), np.arange(5))
    mp = TR.terrain_map(c + al * ix * cell + be * iy * cell, cell)
    for yaw in (0.0, 0.7, -2.9, 1.0e-3):
        pl = TR.placement((0.3, -0.8), yaw)
        cy, sy = np.cos(yaw), np.sin(yaw)
        for _ in range(40):
            loc = rng.uniform(0.0, 1.0, 2) * np.array([5, 4]) * cell
            X, Y = 0.3 + cy * loc[0] - sy * loc[1], -0.8 + sy * loc[0] + cy * loc[1]
            hm, n, (hx, hy) = TR.height_normal(mp, pl, X, Y)
            assert abs(hm - (c + al * loc[0] + be * loc[1])) <= 16 * EPS
            gw = np.array([cy * al - sy * be, sy * al + cy * be])
            assert np.abs(np.array([hx, hy]) - gw).max() <= 64 * EPS      # (a difference of heights ~ 0.4 over a 0.07 cell)
            want = np.r_[-gw, 1.0] / np.sqrt(1.0 + gw @ gw)
            assert np.abs(n - want).max() <= 64 * EPS and abs(np.linalg.norm(n) - 1.0) <= 4 * EPS


def test_the_reference_force_law_turns_with_the_ground():
    """For a plane tilted by a rotation Q the force law is equivariant: force_law(Q P, Q Pdot, the tilted plane) = Q force_law(P, Pdot, the flat plane), to a
    few ulp of the force — d is the distance to the plane, vn and v_t the components along and across its normal.  The tilted plane through Q (0, 0, g0)
    with normal n = Q e_z has, under the point's own (X, Y), the height g = (n . Q (0, 0, g0) - n_x X - n_y Y) / n_z."""
    rng = np.random.default_rng(6)
    ct = dict(stiffness=5e4, damping=10.0, mu=0.6, slip_velocity=0.01, ground_height=0.0)
    seen = set()
    for k in range(60):
        Q = rot(rng.standard_normal(3) * [1, 1, 0.3], rng.uniform(0.0, 0.5))
        P = np.r_[rng.uniform(-0.5, 0.5, 2), 0.1 - rng.uniform(-1e-3, 3e-3)]
        Pdot = rng.standard_normal(3) * (0.05 if k % 3 else 0.3)
        g0 = 0.1
        d0, F0, c0 = TR.force_law(P, Pdot, (g0, np.array([0.0, 0.0, 1.0])), ct)
        n = Q @ np.array([0.0, 0.0, 1.0])
        QP = Q @ P
        g = (n @ (Q @ np.array([0.0, 0.0, g0])) - n[0] * QP[0] - n[1] * QP[1]) / n[2]
        d1, F1, c1 = TR.force_law(QP, Q @ Pdot, (g, n), ct)
        if abs(d0) < 1e-9 or (c0 == "a") != (c1 == "a"):
            continue                       # (at the kink itself rounding picks the side)
        seen.add(c0)
        assert abs(d1 - d0) <= 16 * EPS * (abs(g0) + abs(P[2]) + 1.0), (d0, d1)
        tol = 64 * EPS * (ct["stiffness"] * (abs(g0) + abs(P[2]) + 1.0) + np.linalg.norm(F0))
        assert np.abs(F1 - Q @ F0).max() <= tol, (F1, Q @ F0)
    assert seen >= {"a", "b"}


# ---------------------------------------------------------------------------------------------- host build of the kernel source
class EmuTerrain(C.Structure):
    """emu_terrain (tests/terrain/terrain_emu.h)"""
    _fields_ = [("n_maps", C.c_int32), ("reserved", C.c_int32), ("nx", _ip), ("ny", _ip), ("cell", _dp), ("heights", _dp), ("place", _tp)]


def terrain_struct(maps, place):
    """(emu_terrain, what it points to) of maps = [terrain_ref map] and place = [terrain_ref placement or None (the plane)] per instance, or None: no table."""
    nx, ny, cell, hs = solver.HipSqpSolver.pack_terrain_maps([(m["H"], m["cell"]) for m in maps])
    tab = None if place is None else solver.HipSqpSolver.pack_terrain_instances(place)
    t = EmuTerrain(n_maps=len(maps), reserved=0, nx=nx.ctypes.data_as(_ip), ny=ny.ctypes.data_as(_ip), cell=_p(cell), heights=_p(hs),
                   place=None if tab is None else C.cast(tab, _tp))
    return t, (nx, ny, cell, hs, tab)


class OnTerrain:
    """A stand-in for the emulator library whose emu_rollout runs with a terrain resident: tests/rollout_emu.py's rollout() drives it unchanged."""
    def __init__(self, lib, t):
        self.lib, self.t = lib, t

    def emu_rollout(self, h, call):
        self.lib.emu_rollout_terrain(h, call, C.byref(self.t))


def build_emu(path, *defines):
    lib = E.build(path, os.path.join("terrain", "terrain_emu.cpp"), "-ffp-contract=off", *defines)
    _cs, _cg = C.POINTER(_abi.ContactSettings), C.POINTER(_abi.ContactGround)
    lib.emu_rollout_terrain.argtypes = [C.c_void_p, C.POINTER(E.Call), C.POINTER(EmuTerrain)]
    lib.emu_ws_bytes_terrain.argtypes = [C.c_int, C.c_int]
    lib.emu_terrain_eval.argtypes = [_cs, _cg, C.POINTER(EmuTerrain), C.c_int, _dp, _dp, _dp]
    lib.emu_contact_eval.argtypes = [C.c_void_p, _cs, _cg, C.POINTER(EmuTerrain), _dp, _dp, _dp]
    return lib


class Emu:
    def __init__(self, lib, model):
        self.lib, self.h = lib, E.create(lib, model)

    def close(self):
        self.lib.emu_destroy(self.h)

    def height(self, ct, terrain, xy, ground=None):
        """(g [n], normal [n][3]) of one instance; terrain: (map, placement) or None."""
        xy = np.ascontiguousarray(xy, dtype=float).reshape(-1, 2)
        g, n = np.zeros(len(xy)), np.zeros((len(xy), 3))
        cs = contact_struct(ct)
        t, keep = terrain_struct([terrain[0]], [terrain[1]]) if terrain is not None else (None, None)
        self.lib.emu_terrain_eval(C.byref(cs), ground_array(None if ground is None else [ground]), None if t is None else C.byref(t), len(xy), _p(xy), _p(g), _p(n))
        return g, n

    def eval(self, ct, x, terrain, ground=None):
        """(force [8][3], penetration [8]) of one instance; terrain: (map, placement) or None."""
        f, d = np.zeros((8, 3)), np.zeros(8)
        cs = contact_struct(ct)
        t, keep = terrain_struct([terrain[0]], [terrain[1]]) if terrain is not None else (None, None)
        self.lib.emu_contact_eval(self.h, C.byref(cs), ground_array(None if ground is None else [ground]), None if t is None else C.byref(t),
                                  _p(np.ascontiguousarray(x)), _p(f), _p(d))
        return f, d

    def rollout(self, pl, ct, st, case, s0, x0, duration, n, ground=None, maps=None, place=None, **kw):
        """tests/rollout_emu.py's rollout (x, u, status, steps, rejected) with the terrain (maps, place) resident; maps None: emu_rollout itself."""
        lib = self.lib
        if maps is not None:
            t, keep = terrain_struct(maps, place)
            lib = OnTerrain(self.lib, t)
        return E.rollout(lib, self.h, case, st, s0, x0, duration, n, plant=settings_struct(pl), contact=None if ct is None else contact_struct(ct),
                         ground=ground_array(ground), **kw)[:5]


@pytest.fixture(scope="module")
def emu(tmp_path_factory, model):
    e = Emu(build_emu(tmp_path_factory.mktemp("terrain") / "libterrain_emu.so"), model)
    yield e
    e.close()


@pytest.fixture(scope="module")
def emu_reverse(tmp_path_factory, model):
    e = Emu(build_emu(tmp_path_factory.mktemp("terrain_rev") / "libterrain_emu_rev.so", "-DHSQP_EMU_REVERSE"), model)
    yield e
    e.close()


# ---------------------------------------------------------------------------------------------- the case set (shared with tests/test_gpu_terrain.py)
MAPS = dict(ramp=TR.ramp_map(), ledge=TR.ledge_map(), rubble=TR.rubble_map())
MAP_INDEX = dict(ramp=0, ledge=1, rubble=2)


def place_under(oracle, model, name, x):
    """The placement of map `name` under the state x, and the instance's ground height: 1 mm above its lowest sole corner at that corner's (X, Y) — lowest
    over the ground, i.e. the corner that would touch first: the instance stands 1 mm deep in its terrain at that corner and nowhere deeper, as the instances
    of tests/test_gpu_contact.py stand in their planes.  (Grounding by the corner lowest in z instead would bury the corners over higher cells by the map's
    amplitude, centimetres: the Hunt-Crossley damping k d c grows with the penetration d, and at d = 2 cm its rate k d c / m_foot ~ 1e4 / s is far past what
    RK4 at RK4_STEP = 1 ms integrates stably (2.78 / h) — the rollouts would compare two unstable integrations, which amplify rounding.)
    ramp: yaw 0.7, the map's centre under the centre of the eight corners.  ledge: yaw 0, the lowest corner in the middle of the slope cell (a = 2.5) and on
    the cell line b = 1 (the corner lowest in z: placement only) — along that line both neighbours are the same patch (the ledge does not vary along y), so the side rounding picks changes nothing.
    rubble: yaw 0, the map's centre under the centre of the corners."""
    P = CR.points(oracle, model, x[:NV])
    low = P[int(np.argmin(P[:, 2]))]
    mp = MAPS[name]
    ny, nx = mp["H"].shape
    if name == "ledge":
        pl = TR.placement((low[0] - 2.5 * mp["cell"], low[1] - 1.0 * mp["cell"]), 0.0, MAP_INDEX[name])
    else:
        yaw = 0.7 if name == "ramp" else 0.0
        half = 0.5 * mp["cell"] * np.array([nx - 1, ny - 1])
        c = P[:, :2].mean(axis=0)
        pl = TR.placement((c[0] - (np.cos(yaw) * half[0] - np.sin(yaw) * half[1]), c[1] - (np.sin(yaw) * half[0] + np.cos(yaw) * half[1])), yaw, MAP_INDEX[name])
    over = np.array([TR.height_normal(mp, pl, c[0], c[1])[0] for c in P]) - P[:, 2]      # the map's height over every corner
    return pl, float(1e-3 - over.max())


def deep_of(xs):
    """tests/test_gpu_contact.py's deep states: the base pushed down by 2 mm, the joint velocities scaled by 3."""
    deep = xs.copy()
    deep[:, 2] -= 0.002
    deep[:, NV + 6:] *= 3.0
    return deep


@pytest.fixture(scope="module")
def xs(model):
    return start_states(model, False, np.random.default_rng(31), B)


# ---------------------------------------------------------------------------------------------- 1. height and normal
def sample_points(mp, pl, rng):
    """World points of one placed map, by class: interior, exactly on cell lines and nodes (in map coordinates; exact in world coordinates with yaw 0
    and an origin of 0), outside every edge and corner."""
    ny, nx = mp["H"].shape
    cell, cy, sy = mp["cell"], np.cos(pl["yaw"]), np.sin(pl["yaw"])
    loc = dict(interior=[(rng.uniform(0, nx - 1), rng.uniform(0, ny - 1)) for _ in range(12)],
               lines=[(float(i), rng.uniform(0, ny - 1)) for i in range(nx)] + [(rng.uniform(0, nx - 1), float(j)) for j in range(ny)] +
                     [(float(i), float(j)) for i in range(nx) for j in range(ny)],
               outside=[(a, b) for a in (-1.7, 0.37 * (nx - 1), nx - 1 + 2.3, -1e9, 1e300) for b in (-0.6, 0.61 * (ny - 1), ny - 1 + 5.1, 1e12)
                        if not (0 <= a <= nx - 1 and 0 <= b <= ny - 1)])
    out = {}
    for k, pts in loc.items():
        out[k] = [(pl["origin"][0] + (cy * a - sy * b) * cell, pl["origin"][1] + (sy * a + cy * b) * cell) for a, b in pts]
    return out


def height_bounds(mp, pl, X, Y, ground_height):
    """(bound on the height, bound on a component of the normal) at the world point (X, Y) — see test_height_and_normal_match_the_reference."""
    H, cell = mp["H"], mp["cell"]
    ny, nx = H.shape
    dH = max(np.abs(np.diff(H, axis=0)).max(), np.abs(np.diff(H, axis=1)).max(), 1e-300)
    d2H = np.abs(H[1:, 1:] - H[1:, :-1] - H[:-1, 1:] + H[:-1, :-1]).max()
    coord = 4 * EPS * (abs(X - pl["origin"][0]) + abs(Y - pl["origin"][1])) / cell
    tol_h = 32 * EPS * (abs(ground_height) + np.abs(H).max() + max(nx, ny) * dH) + min(coord * dH, H.max() - H.min())
    tol_n = 8 * EPS * dH / cell + 8 * EPS + min(coord * d2H / cell, 2.0)
    return tol_h, tol_n, dH


@pytest.mark.parametrize("name", ["ramp", "ledge", "rubble"])
def test_height_and_normal_match_the_reference(emu, model, name):
    """Tolerances (height_bounds).  The height is a chain of ~10 roundings on values of size max|H| + |ground_height| and on a map coordinate inside the grid
    whose rounding eps |a| moves it by eps |a| cell |grad| <= eps |a| max|dH|: 32 eps (|ground_height| + max|H| + n max|dH|), n the larger dimension.  The
    normal: a gradient component is a difference of heights over the cell, 8 eps max|dH| / cell, and n is that over sqrt(1 + |grad|^2) <= 1 — plus 8 eps.
    Far outside the grid under a rotated placement a map coordinate is a difference of two large products: it carries 4 eps (|X - origin_x| + |Y -
    origin_y|) / cell cells of rounding, whatever its own size — the coordinate that is NOT clamped then moves the height by that times max|dH| (at most the
    map's range) and a gradient component by that times the largest mixed difference of a cell over the cell size; both terms vanish near the map.
    At a point meant to lie exactly ON a cell line a rotated placement (or a non-zero origin) leaves the coordinate an ulp to either side, and the
    two sides have different patches: there the emulator's normal must be that of one of the patches around the point (the reference a hair to either
    side), not of the side the reference's own rounding picked."""
    rng = np.random.default_rng(12)
    mp = MAPS[name]
    ct = CR.contact(model, ground_height=0.37)
    ny, nx = mp["H"].shape
    for pl in (TR.placement((0.0, 0.0), 0.0), TR.placement((0.3, -0.8), 0.7)):
        exact = pl["yaw"] == 0.0
        for cls, pts in sample_points(mp, pl, rng).items():
            g, n = emu.height(ct, (mp, dict(pl, map=0)), pts)
            for (X, Y), gi, ni in zip(pts, g, n):
                hm, nr, grad = TR.height_normal(mp, pl, X, Y)
                tol_h, tol_n, dH = height_bounds(mp, pl, X, Y, 0.37)
                assert abs(gi - (0.37 + hm)) <= tol_h, (name, cls, X, Y, gi - 0.37 - hm)
                if cls == "lines" and not exact:
                    e = 1e-7 * mp["cell"]
                    around = [TR.height_normal(mp, pl, X + sx * e, Y + sy * e)[1] for sx in (-1, 1) for sy in (-1, 1)]
                    assert min(np.abs(ni - a).max() for a in around) <= tol_n + 1e-6 * dH / mp["cell"], (name, cls, X, Y)   # (curvature over the hair: t moves by 1e-7)
                else:
                    assert np.abs(ni - nr).max() <= tol_n, (name, cls, X, Y, ni, nr)
                assert abs(np.linalg.norm(ni) - 1.0) <= 4 * EPS
    # outside an edge the clamped component of the MAP gradient is zero: under yaw 0 that is the world's
    pl = TR.placement((0.0, 0.0), 0.0)
    w = (nx - 1) * mp["cell"]
    g, n = emu.height(ct, (mp, pl), [(-1.0, 0.5 * mp["cell"]), (w + 1.0, 0.5 * mp["cell"]), (0.5 * mp["cell"], -3.0), (-2.0, -2.0), (1e300, -1e300)])
    assert n[0, 0] == 0.0 and n[1, 0] == 0.0 and n[2, 1] == 0.0 and tuple(n[3]) == (0.0, 0.0, 1.0) and tuple(n[4]) == (0.0, 0.0, 1.0)
    assert g[3] == 0.37 + mp["H"][0, 0] and g[4] == 0.37 + mp["H"][0, -1]
    # the plane, and a non-finite coordinate
    g, n = emu.height(ct, None, [(0.3, 0.2), (np.inf, 0.0)])
    assert (g == 0.37).all() and (n == [0.0, 0.0, 1.0]).all()
    g, n = emu.height(ct, (mp, pl), [(np.nan, 0.0), (0.0, np.inf), (-np.inf, np.inf)], ground=(0.5, 0.3))
    assert np.isnan(g).all() and (n == [0.0, 0.0, 1.0]).all()
    assert emu.height(ct, (mp, pl), [(0.0, 0.0)], ground=(0.5, 0.3))[0][0] == 0.5 + mp["H"][0, 0]      # the per-instance height is the offset under the map


# ---------------------------------------------------------------------------------------------- 2. forces and penetrations
def force_bounds(ref, ct, mp, ref_d):
    """tests/test_contact.py's rule with scale = |P_z| + |ground_height| + max|H|, the bound on d extended by 8 x the reference's own rounding ref_d
    (force_cases): (bound on d [8], A [8][1])."""
    scale = np.abs(ref["P"][:, 2]) + abs(ct["ground_height"]) + np.abs(mp["H"]).max()
    return 64 * EPS * scale + 8.0 * ref_d, ct["stiffness"] * 64 * EPS * scale[:, None]


def force_cases(oracle, model, xs, name):
    """([(kind, b, placement, setting, state, reference)], ref_d) of map `name`: the start states and the deep states of every instance, and the float64
    reference's own rounding in d — the largest |d - d_longdouble| over the set, the same reference evaluated in np.longdouble on the same kinematics."""
    out, ref_d = [], 0.0
    for kind, states in (("start", xs), ("deep", deep_of(xs))):
        for b in range(len(xs)):
            pl, hgt = place_under(oracle, model, name, xs[b])
            ct = CR.contact(model, ground_height=hgt)
            ref = TR.forces(oracle, model, states[b], ct, (MAPS[name], pl), velocity="frame")
            wide = TR.forces(oracle, model, states[b], ct, (MAPS[name], pl), velocity="frame", dtype=np.longdouble)
            ref_d = max(ref_d, float(np.abs(ref["d"] - wide["d"]).max()))
            out.append((kind, b, pl, ct, states[b], ref))
    return out, ref_d


def check_forces(name, kind, b, f, d, ref, ct, ref_d):
    """The assertions of the force test on one instance; returns (d error / bound, force error / bound)."""
    tol_d, A = force_bounds(ref, ct, MAPS[name], ref_d)
    err_d, err_f = np.abs(d - ref["d"]), np.abs(f - ref["f"])
    tol_f = A + A * np.linalg.norm(ref["f"], axis=1)[:, None]
    print(f"{name} {kind} {b}: classes {''.join(ref['cls'])}, |f| {np.abs(ref['f']).max():.3e}, |grad| {np.abs(ref['grad']).max():.2e}, "
          f"d error {err_d.max():.2e}, / bound {(err_d / tol_d).max():.2e}, / old bound {(err_d / (tol_d - 8.0 * ref_d)).max():.2e}, "
          f"force error / bound {(err_f / tol_f).max():.2e}")
    assert (err_d <= tol_d).all(), (name, kind, b, err_d.max())
    assert (err_f <= tol_f).all(), (name, kind, b, err_f.max())
    for i, c in enumerate(ref["cls"]):
        if c != "a":
            assert not f[i].any() and not np.signbit(f[i]).any()          # no force: +0 in every component
    return (err_d / tol_d).max(), (err_f / tol_f).max()


@pytest.mark.parametrize("name", ["ramp", "ledge", "rubble"])
def test_forces_and_penetrations_match_the_reference(emu, model, oracle, xs, name):
    """The rule of tests/test_contact.py::test_forces_and_penetrations_match_the_reference with scale = |P_z| + |ground_height| + max|H| per point:
    |d - d_ref| <= 64 eps scale, |f - f_ref| <= A + A |f_ref| with A = k 64 eps scale; the reference's velocities in closed form.  Start states and the
    deep states of tests/test_gpu_contact.py.
    The host build MISSES the bound on d on the rubble map (deep states of instances 1 and 2: d error / bound 1.04 and 1.07, errors of 2.5e-16 — the
    soles stand near z = 0, so scale is ~ 0.012 and the bound is about one rounding of the base height the point's P_z is summed from); the forces meet theirs
    with a margin of 60.  So the bound on d is the old one plus 8 x the float64 reference's own rounding, measured against the same reference in
    np.longdouble over the map's case set (force_cases).  Measured: the reference's own rounding in d is 8.2e-18 (ramp), 6.9e-18 (ledge), 9.3e-18 (rubble);
    with it the host build's worst d error / bound is 0.29, 0.24 and 0.81, its worst force error / bound 0.006, 0.004 and 0.017."""
    mp = MAPS[name]
    cases, ref_d = force_cases(oracle, model, xs, name)
    active = sloped = 0
    worst_d = worst_f = 0.0
    for kind, b, pl, ct, x, ref in cases:
        f, d = emu.eval(ct, x, (mp, dict(pl, map=0)))
        wd, wf = check_forces(name, kind, b, f, d, ref, ct, ref_d)
        worst_d, worst_f = max(worst_d, wd), max(worst_f, wf)
        active += ref["cls"].count("a")
        sloped += int((np.abs(ref["grad"]).sum(axis=1) > 0.0).sum())
        if name == "ledge" and b == 1 and kind == "start":
            a = (ref["P"][:, 0] - pl["origin"][0]) / mp["cell"]
            bb = (ref["P"][:, 1] - pl["origin"][1]) / mp["cell"]
            assert ((a > 2.0) & (a < 3.0) & (np.abs(ref["grad"][:, 0]) > 1.0)).any()       # a corner stands on the slope cell ...
            assert (np.abs(bb - 1.0) <= 1e-9).any()                                         # ... and one sits on a cell line
    print(f"{name}: active points {active}, points on a slope {sloped}, reference's own rounding in d {ref_d:.2e}, worst d error / bound {worst_d:.2e}, "
          f"worst force error / bound {worst_f:.2e}")
    assert active >= B and sloped >= 1


# ---------------------------------------------------------------------------------------------- 3. a map of zeros is the plane
def test_a_map_of_zeros_with_yaw_zero_equals_the_plane_contact(emu, model, oracle, xs):
    """To 64 eps relative, not to bits: the two forms (d n_z against d, Pdot . n against Pdot_z) may be contracted differently by a compiler."""
    flat = TR.terrain_map(np.zeros((3, 4)), 0.05)
    for states in (xs, deep_of(xs)):
        for b in range(B):
            P = CR.points(oracle, model, xs[b][:NV])
            ct = CR.contact(model, ground_height=float(P[:, 2].min() + 1e-3))
            pl = TR.placement((P[0, 0] - 0.02, P[0, 1] - 0.03), 0.0)
            f, d = emu.eval(ct, states[b], (flat, pl))
            f0, d0 = emu.eval(ct, states[b], None)
            assert (np.abs(d - d0) <= 64 * EPS * np.abs(d0)).all() and (np.abs(f - f0) <= 64 * EPS * np.abs(f0)).all()
            assert f0[:, 2].sum() > 0.0


# ---------------------------------------------------------------------------------------------- 4., 8. batch behaviour
def batch_setup(model, oracle, xs, names=("ledge", None, "rubble")):
    """(maps, place [B], ground [B]) of a mixed batch: instance b on the map names[b] (None: map = -1, the plane)."""
    place, ground = [], []
    for b, name in enumerate(names):
        if name is None:
            place.append(None)
            ground.append((float(CR.points(oracle, model, xs[b][:NV])[:, 2].min() + 1e-3), 0.6))
        else:
            pl, hgt = place_under(oracle, model, name, xs[b])
            place.append(pl)
            ground.append((hgt, (0.2, 0.6, 1.0)[b]))
    return [MAPS["ramp"], MAPS["ledge"], MAPS["rubble"]], place, ground


def same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def test_a_plane_instance_in_a_terrain_batch_equals_the_run_without_a_terrain(emu, model, oracle, xs):
    rng = np.random.default_rng(17)
    case = plant_case(model, "events", rng)
    pl, ct = PL.plant(**GAINS), CR.contact(model)
    maps, place, ground = batch_setup(model, oracle, xs)
    s0 = np.array([0.0, 0.013, 0.003])
    for integrator, controller in ((R.RK4, R.FEEDFORWARD), (R.ODE45, R.FEEDBACK)):
        st = R.settings(integrator, controller, initial_step=RK4_STEP if integrator == R.RK4 else 0.015)
        on = emu.rollout(pl, ct, st, case, s0, xs, D, 2, ground, maps, place)
        off = emu.rollout(pl, ct, st, case, s0, xs, D, 2, ground)
        assert (on[2] == R.OK).all() and (off[2] == R.OK).all()
        assert all(np.array_equal(a[1], b[1]) for a, b in zip(on, off))              # map = -1: the bits of the plane contact
        assert rel(on[0][0], off[0][0]) > 1e-6 and rel(on[0][2], off[0][2]) > 1e-6   # the others feel their maps
        # 8. instance b alone equals instance b in the batch, bit for bit
        for b in range(B):
            solo = emu.rollout(pl, ct, st, case, s0[b:b + 1], xs[b:b + 1], D, 2, ground[b:b + 1], maps, place[b:b + 1])
            assert all(np.array_equal(a[0], c[b]) for a, c in zip(solo, on)), (integrator, b)
        # ... and two half-duration calls equal one call (the pattern of the contact tests)
        d = 2.0 ** -7
        r = emu.rollout(pl, ct, st, case, s0, xs, 2 * d, 2, ground, maps, place)
        a = emu.rollout(pl, ct, st, case, s0, xs, d, 1, ground, maps, place)
        c = emu.rollout(pl, ct, st, case, s0 + d, a[0][:, 0].copy(), d, 1, ground, maps, place)
        assert np.array_equal(a[0][:, 0], r[0][:, 0]) and np.array_equal(a[1][:, 0], r[1][:, 0]), integrator
        assert np.array_equal(c[0][:, 0], r[0][:, 1]) and np.array_equal(c[1][:, 0], r[1][:, 1]), integrator
        assert np.array_equal(a[3] + c[3], r[3])


def test_reverse_order_emulation_is_bit_identical(emu, emu_reverse, model, oracle, xs):
    rng = np.random.default_rng(18)
    case = plant_case(model, "events", rng)
    pl, ct = PL.plant(**GAINS), CR.contact(model)
    maps, place, ground = batch_setup(model, oracle, xs)
    for b in range(B):
        if place[b] is not None:
            t = (maps[place[b]["map"]], dict(place[b], map=0))
            assert same(emu.eval(ct, xs[b], t, ground[b]), emu_reverse.eval(ct, xs[b], t, ground[b]))
    for integrator in (R.ODE45, R.RK4):
        st = R.settings(integrator, R.FEEDBACK, initial_step=RK4_STEP if integrator == R.RK4 else 0.015)
        a = emu.rollout(pl, ct, st, case, np.zeros(B), xs, D, 2, ground, maps, place)
        assert (a[2] == R.OK).all() and same(a, emu_reverse.rollout(pl, ct, st, case, np.zeros(B), xs, D, 2, ground, maps, place))


# ---------------------------------------------------------------------------------------------- 5. no terrain: the ten configurations keep their bits
def test_without_a_terrain_every_configuration_keeps_its_bits(emu, model, cmodel, oracle, xs):
    """The ten configurations (the two flow maps; the torque plant x ground x actuator x inertia table — the list of
    tests/test_inertia.py::test_every_torque_configuration_with_inert_parts_is_the_plant_bit_for_bit, here with parts that act) through emu_rollout and
    through the terrain's entry with what does NOT make a terrain: maps but no placement table, and (where there is no ground) maps and a table.  Same bits,
    and the workspaces of the ten keep their sizes: the terrain instantiations are four more, larger ones."""
    lib = solver.load_library()
    rng = np.random.default_rng(74)
    case = plant_case(model, "uniform", rng)
    s0 = np.array([0.0, 0.003, 0.013])
    pl = settings_struct(PL.plant(**GAINS))
    ct = contact_struct(CR.contact(model))
    ground = ground_array([(float(CR.points(oracle, model, x[:NV])[:, 2].min() + 1e-3), 0.6) for x in xs])
    act = _abi.ActuatorSettings()
    lib.hsqp_actuator_defaults(C.byref(act))
    act.command_period = 0.003
    tab = solver.HipSqpSolver.pack_inertia(np.array([1.0, 1.1, 0.9]), [[], [dict(body=12, mass=2.0)], []])
    maps, place, _ = batch_setup(model, oracle, xs)
    no_table, keep1 = terrain_struct(maps, None)
    table, keep2 = terrain_struct(maps, place)
    st = R.settings(R.RK4, R.FEEDBACK, initial_step=RK4_STEP)
    ch = E.create(emu.lib, cmodel)
    try:
        from test_rollout import make_case
        ccase = make_case(model, True, "uniform", rng)
        cx = start_states(model, True, rng, B)
        configs = [("centroidal flow", ch, ccase, cx, {}), ("whole-body flow", emu.h, case, xs, {})]
        for v in (0, 1):
            for a in (0, 1):
                for g in (0, 1):
                    kw = dict(plant=pl)
                    if g:
                        kw.update(contact=ct, ground=ground)
                    if a:
                        kw.update(actuator=act)
                    if v:
                        kw.update(inertia=tab)
                    configs.append((f"torque ground {g} actuator {a} varied {v}", emu.h, case, xs, kw))
        assert len(configs) == 10
        for label, h, cs, x0, kw in configs:
            want = E.rollout(emu.lib, h, cs, st, s0, x0, D, 2, **kw)
            assert (want[2] == R.OK).all(), label
            got = E.rollout(OnTerrain(emu.lib, no_table), h, cs, st, s0, x0, D, 2, **kw)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want)), label
            if "contact" not in kw:           # a table too, but no ground (or no torque plant): stored and inert
                got = E.rollout(OnTerrain(emu.lib, table), h, cs, st, s0, x0, D, 2, **kw)
                assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want)), label
    finally:
        emu.lib.emu_destroy(ch)
    sizes = [emu.lib.emu_ws_bytes(0, 1, k & 1, (k >> 1) & 1, k >> 2) for k in range(8)]
    tsizes = [emu.lib.emu_ws_bytes_terrain(k & 1, k >> 1) for k in range(4)]
    print("rollout workspaces of the torque plant:", sizes, " on the terrain (plain, actuator, varied, both):", tsizes)
    assert sizes[0] == 33200 and len(set(sizes + tsizes)) == 12 and all(0 < s <= 65536 for s in tsizes)
    for k in range(4):
        assert 0 < tsizes[k] - sizes[1 | (k << 1)] <= 128      # the instance's map on top of the grounded workspace: well under 128 bytes


# ---------------------------------------------------------------------------------------------- 6. RK4 rollout against terrain_ref
@pytest.mark.parametrize("name", ["ledge", "rubble"])
@pytest.mark.parametrize("grid", ["uniform", "events"])
@pytest.mark.parametrize("controller", [R.FEEDFORWARD, R.FEEDBACK])
def test_rk4_rollout_matches_numpy(emu, model, oracle, xs, controller, grid, name):
    """At TERRAIN_RK4_STEP.  X_TOL / U_TOL as in tests/test_contact.py::test_rk4_rollout_matches_numpy (the reference carries a finite-difference Jacobian: FD_TOL on the
    accelerations over the duration, times 10; 1e-9 on the inputs), equal step counts, and the run differs from the plane run by > 1e-6."""
    rng = np.random.default_rng(43 + controller)
    case = plant_case(model, grid, rng)
    pl = PL.plant(**GAINS)
    st = R.settings(R.RK4, controller, initial_step=TERRAIN_RK4_STEP)
    b = 2                      # (an instance whose soles carry force from the start: instance 1's lowest corner separates faster than 1 / c)
    place, hgt = place_under(oracle, model, name, xs[b])
    ct = CR.contact(model, ground_height=hgt)
    x0, s0 = xs[b:b + 1], np.array([0.003])
    x, u, status, steps, rej = emu.rollout(pl, ct, st, case, s0, x0, D, 2, None, [MAPS[name]], [dict(place, map=0)])
    pol = R.Policy(case["ut"], case["dt"], case["dts"], case["K"], case["uff"], 0, False)
    cl = TR.closed_loop(oracle, model, pol, case["xt"], pl, controller, ct, (MAPS[name], place))
    xr, ur, sr, nr, rr = PL.rollout(cl, pol, st, s0[0], x0[0], D, 2)
    assert status[0] == sr == R.OK and rej[0] == rr == 0 and steps[0] == nr, (status[0], sr, steps[0], nr)
    ex, eu = rel(x[0], xr), rel(u[0], ur)
    print(f"{name}, controller {controller}, {grid}: steps {nr}, emulation against numpy: x error {ex:.2e}, u error {eu:.2e}")
    assert ex <= X_TOL and eu <= U_TOL, (ex, eu)
    plane = emu.rollout(pl, ct, st, case, s0, x0, D, 2)
    assert (plane[2] == R.OK).all() and rel(x[0], plane[0][0]) > 1e-6


# ---------------------------------------------------------------------------------------------- 7. ODE45 against a tight solution
def test_ode45_against_a_tight_solution(emu, model, oracle, xs):
    """The rule of the contact model's own tight-solution test (tests/test_gpu_contact.py::test_ode45_against_a_tight_solution): the tight solution is RK4 at
    2^-15 s on the reference, for ONE instance; ODE45 at the default tolerances stays within 10 x (abs_tol + rel_tol |x|) of it — 50 x where a node stamp
    (a kink of the interpolated controller) lies inside the interval —, and at tolerances of 1e-10 within 1e-7."""
    rng = np.random.default_rng(47)
    case = plant_case(model, "uniform", rng)
    pl = PL.plant(**GAINS)
    b, name = 2, "rubble"
    place, hgt = place_under(oracle, model, name, xs[b])
    ct = CR.contact(model, ground_height=hgt)
    x0, s0, T = xs[b:b + 1], np.array([0.003]), D
    pol = R.Policy(case["ut"], case["dt"], case["dts"], case["K"], case["uff"], 0, False)
    cl = TR.closed_loop(oracle, model, pol, case["xt"], pl, R.FEEDFORWARD, ct, (MAPS[name], place))
    ref = PL.tight_solution(cl, pol, s0[0], x0[0], T)
    assert np.isfinite(ref).all()
    args = (case, s0, x0, T, 1, None, [MAPS[name]], [dict(place, map=0)])
    r = emu.rollout(pl, ct, R.settings(R.ODE45, R.FEEDFORWARD), *args)
    r2 = emu.rollout(pl, ct, R.settings(R.ODE45, R.FEEDFORWARD, abs_tol=1e-10, rel_tol=1e-10), *args)
    assert r[2][0] == R.OK and r2[2][0] == R.OK and r2[3][0] > r[3][0] and r2[3][0] < 10000
    err = float(np.abs(r2[0][0, 0] - ref).max())
    ratio = float((np.abs(r[0][0, 0] - ref) / (1e-5 + 1e-3 * np.abs(ref))).max())
    print(f"steps {r[3][0]} rejected {r[4][0]} error / tolerance {ratio:.2f}; tight steps {r2[3][0]} rejected {r2[4][0]} tight error {err:.2e}")
    stamps = np.arange(len(case["ut"]) + 1) * case["dt"]
    kink = any(((stamps - la > s0[0]) & (stamps - la < s0[0] + T)).any() for la in (0.0, pl["lookahead"]))
    assert ratio <= (50.0 if kink else 10.0), (kink, ratio)
    assert err <= 1e-7, err


# ---------------------------------------------------------------------------------------------- a non-finite coordinate ends the instance
def test_a_non_finite_coordinate_ends_the_instance_non_finite(emu, model, oracle, xs):
    """On the plane the base's x and y do not enter the dynamics; on a map a non-finite one makes the height NaN (the map is not read) and the instance
    ends HSQP_ROLLOUT_NONFINITE, the others keep their bits."""
    rng = np.random.default_rng(19)
    case = plant_case(model, "uniform", rng)
    pl, ct = PL.plant(**GAINS), CR.contact(model)
    maps, place, ground = batch_setup(model, oracle, xs, ("rubble", "ledge", "rubble"))
    st = R.settings(R.RK4, R.FEEDFORWARD, initial_step=RK4_STEP)
    want = emu.rollout(pl, ct, st, case, np.zeros(B), xs, D, 1, ground, maps, place)
    bad = xs.copy()
    bad[1, 0] = np.inf
    got = emu.rollout(pl, ct, st, case, np.zeros(B), bad, D, 1, ground, maps, place)
    assert got[2].tolist() == [R.OK, R.NONFINITE, R.OK] and np.isnan(got[0][1]).all()
    assert np.array_equal(got[0][[0, 2]], want[0][[0, 2]])


# ---------------------------------------------------------------------------------------------- sanitizers: a program of its own
def test_the_index_arithmetic_under_sanitizers(tmp_path, model):
    exe, desc = tmp_path / "terrain_sanitize", tmp_path / "desc.bin"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "terrain", "terrain_emu.cpp"),
                           os.path.join(ROOT, "tests", "terrain", "terrain_sanitize.cpp"), "-o", str(exe)])
    desc.write_bytes(bytes(model.desc))
    out = subprocess.check_output([str(exe), str(desc)], text=True)
    assert out.strip() == "terrain ok"
