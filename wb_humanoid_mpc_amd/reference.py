"""Host-side per-node parameter generation.

Mirrors, for the solver's node grid, what the reference's solver pulls through its
callbacks every iteration:
  * mode schedule / contact flags  — GaitSchedule::tileModeSequenceTemplate
    (humanoid_nmpc/humanoid_common_mpc/src/gait/GaitSchedule.cpp:101-131),
    ModeSchedule::modeAtTime (upstream ocs2: lower_bound on the event times),
    modeNumber2StanceLeg (…/gait/MotionPhaseDefinition.h:58-76)
  * swing-foot height splines and impact-proximity factor — SwingTrajectoryPlanner::update
    (…/swing_foot_planner/SwingTrajectoryPlanner.cpp:87-191), SplineCpg.cpp:38-62, CubicSpline.cpp:38-80
  * gait phase variable for the arm-swing reference — SwitchedModelReferenceManager::getPhaseVariable
    (…/reference_manager/SwitchedModelReferenceManager.cpp:62-80)
  * target trajectories from a commanded base velocity — WBMpcTargetTrajectoriesCalculator::
    commandedVelocityToTargetTrajectories (humanoid_nmpc/humanoid_wb_mpc/src/command/WBMpcTargetTrajectoriesCalculator.cpp:80-136)
  * cold-start trajectory — WeightCompInitializer::compute (…/initialization/WeightCompInitializer.cpp:66-70)

The result is the POD table hsqp_problem::node_params (include/hsqp.h).  In the ROS
deployment the ocs2 adaptor fills the same table from the reference's own
ReferenceManager / SwingTrajectoryPlanner objects.
"""
import bisect
import math

import numpy as np

from . import _abi

FLY, RF, LF, STANCE = 0, 1, 2, 3
MODE_BY_NAME = {"FLY": FLY, "RF": RF, "LF": LF, "STANCE": STANCE}


def mode_to_contact_flags(mode):
    """{left, right} stance flags (MotionPhaseDefinition.h:58-76)."""
    return (mode in (LF, STANCE), mode in (RF, STANCE))


class ModeSchedule:
    def __init__(self, event_times, mode_sequence):
        assert len(mode_sequence) == len(event_times) + 1
        self.event_times = list(event_times)
        self.mode_sequence = list(mode_sequence)

    def index_at(self, t):
        # lookup::findIndexInTimeArray == std::lower_bound
        return bisect.bisect_left(self.event_times, t)

    def mode_at(self, t):
        return self.mode_sequence[self.index_at(t)]


def tile_gait(gait, t_start, t_final):
    """STANCE until t_start, then the template tiled until the tiling passes t_final, then STANCE
    (GaitSchedule::tileModeSequenceTemplate: 'add a initial time', tile, 'default final phase')."""
    modes = [MODE_BY_NAME[m] for m in gait["modeSequence"]]
    times = gait["switchingTimes"]
    event_times = [t_start]
    seq = [STANCE]
    while event_times[-1] < t_final:
        for i, m in enumerate(modes):
            seq.append(m)
            event_times.append(event_times[-1] + (times[i + 1] - times[i]))
    seq.append(STANCE)
    return ModeSchedule(event_times, seq)


# ------------------------------------------------------------------------------------ splines
class CubicSpline:
    def __init__(self, t0, p0, v0, t1, p1, v1):
        self.t0, self.dt = t0, t1 - t0
        dp, dv = p1 - p0, v1 - v0
        dc1, dc2, dc3 = v0, -(3.0 * v0 + dv), (2.0 * v0 + dv)
        self.c0 = p0
        self.c1 = dc1 * self.dt
        self.c2 = dc2 * self.dt + 3.0 * dp
        self.c3 = dc3 * self.dt - 2.0 * dp

    def _tn(self, t):
        return (t - self.t0) / self.dt

    def position(self, t):
        tn = self._tn(t)
        return self.c3 * tn ** 3 + self.c2 * tn ** 2 + self.c1 * tn + self.c0

    def velocity(self, t):
        tn = self._tn(t)
        return (3.0 * self.c3 * tn * tn + 2.0 * self.c2 * tn + self.c1) / self.dt

    def acceleration(self, t):
        tn = self._tn(t)
        return (6.0 * self.c3 * tn + 2.0 * self.c2) / (self.dt * self.dt)


class SplineCpg:
    def __init__(self, lift_off, mid_height, touch_down):
        (t0, p0, v0), (t1, p1, v1) = lift_off, touch_down
        self.mid = 0.5 * (t0 + t1)
        self.left = CubicSpline(t0, p0, v0, self.mid, mid_height, 0.0)
        self.right = CubicSpline(self.mid, mid_height, 0.0, t1, p1, v1)

    def _s(self, t):
        return self.left if t < self.mid else self.right

    def position(self, t):
        return self._s(t).position(t)

    def velocity(self, t):
        return self._s(t).velocity(t)

    def acceleration(self, t):
        return self._s(t).acceleration(t)


class SwingTrajectoryPlanner:
    """Per-leg z-height and impact-proximity splines over a mode schedule: flat terrain at terrain_height (the reference's two-argument update), or,
    with lift and touch ([2][phases] each, foot the outer index), its three-argument update (SwingTrajectoryPlanner.cpp:101-191): phase p of leg j reads
    lift[j][p] and touch[j][p]; touch already holds touchDownHeightOffset."""

    def __init__(self, cfg, schedule, terrain_height=0.0, lift=None, touch=None):
        assert (lift is None) == (touch is None)
        rows, lift_rows, touch_rows = lift is not None, lift, touch
        self.schedule = schedule
        seq, ev = schedule.mode_sequence, schedule.event_times
        n = len(seq)
        self.height = [[], []]
        self.impact = [[], []]
        for leg in range(2):
            flags = [mode_to_contact_flags(m)[leg] for m in seq]
            for p in range(n):
                lift = float(lift_rows[leg][p]) if rows else terrain_height
                touch = float(touch_rows[leg][p]) if rows else terrain_height + cfg["touchDownHeightOffset"]
                if flags[p]:
                    self.height[leg].append(SplineCpg((0.0, lift, 0.0), lift, (1.0, lift, 0.0)))
                    self.impact[leg].append(SplineCpg((0.0, 1.0, 0.0), 1.0, (1.0, 1.0, 0.0)))
                    continue
                start = next((ip for ip in range(p - 1, -1, -1) if flags[ip]), -1)
                final = next((ip - 1 for ip in range(p + 1, n) if flags[ip]), n - 1)
                if start < 0 or final >= n - 1:
                    raise RuntimeError(f"swing phase {p} of leg {leg} has no lift-off/touch-down inside the schedule")
                t0, t1 = ev[start], ev[final]
                scaling = min(1.0, (t1 - t0) / cfg["swingTimeScale"])
                mp = cfg["impactProximityFactorMidPointValue"]
                if flags[p - 1] and flags[p + 1]:
                    mid = min(lift, touch) + scaling * cfg["swingHeight"]
                    self.height[leg].append(SplineCpg((t0, lift, scaling * cfg["liftOffVelocity"]), mid,
                                                      (t1, touch, scaling * cfg["touchDownVelocity"])))
                    self.impact[leg].append(SplineCpg((t0, 1.0, scaling * cfg["impactProximityFactorLiftOffVelocity"]), mp,
                                                      (t1, 1.0, scaling * cfg["impactProximityFactorTouchDownVelocity"])))
                elif flags[p - 1]:
                    mid = lift + cfg["swingHeight"]
                    self.height[leg].append(SplineCpg((t0, lift, cfg["liftOffVelocity"]), mid, (t1, mid, 0.0)))
                    self.impact[leg].append(SplineCpg((t0, 1.0, cfg["impactProximityFactorLiftOffVelocity"]), mp, (t1, mp, 0.0)))
                elif flags[p + 1]:
                    mid = touch + cfg["swingHeight"]
                    self.height[leg].append(SplineCpg((t0, mid, 0.0), mid, (t1, touch, cfg["touchDownVelocity"])))
                    self.impact[leg].append(SplineCpg((t0, mp, 0.0), mp, (t1, 1.0, cfg["impactProximityFactorTouchDownVelocity"])))
                else:
                    mid = touch + cfg["swingHeight"]
                    self.height[leg].append(SplineCpg((t0, mid, 0.0), mid, (t1, mid, 0.0)))
                    self.impact[leg].append(SplineCpg((t0, mp, 0.0), mp, (t1, mp, 0.0)))

    def z_refs(self, leg, t):
        s = self.height[leg][self.schedule.index_at(t)]
        return s.position(t), s.velocity(t), s.acceleration(t)

    def impact_proximity(self, leg, t):
        return self.impact[leg][self.schedule.index_at(t)].position(t)


def phase_variable(schedule, t):
    """SwitchedModelReferenceManager::getPhaseVariable (upper_bound on the event times)."""
    ev = schedule.event_times
    it = bisect.bisect_right(ev, t)
    if it <= 0 or it >= len(ev):
        return 0.0
    nxt, prv = ev[it], ev[it - 1]
    mode = schedule.mode_at(t)
    if mode == LF:
        return 0.5 * (t - prv) / (nxt - prv)
    if mode == RF:
        return 0.5 + 0.5 * (t - prv) / (nxt - prv)
    return 0.5 if schedule.mode_at(prv - 0.01) == LF else 0.0


# ------------------------------------------------------------------------------------ targets
class TargetTrajectories:
    def __init__(self, times, states):
        self.times = np.asarray(times, dtype=float)
        self.states = np.asarray(states, dtype=float)

    def desired_state(self, t):
        """ocs2 LinearInterpolation: clamped piece-wise linear."""
        if t <= self.times[0]:
            return self.states[0].copy()
        if t >= self.times[-1]:
            return self.states[-1].copy()
        i = int(np.searchsorted(self.times, t, side="right")) - 1
        a = (self.times[i + 1] - t) / (self.times[i + 1] - self.times[i])
        return a * self.states[i] + (1.0 - a) * self.states[i + 1]


def velocity_command_targets(model, v_cmd, t0, x0, horizon, filter_alpha=0.0, v_filt=None):
    """commandedVelocityToTargetTrajectories.  Default: the command filter at steady state (the reference's first-call transient of the
    function-local static filter — TargetTrajectoriesCalculatorBase.cpp:117-119 — is deliberately not reproduced).  With filter_alpha > 0
    the knots are formed from alpha v_filt + (1 - alpha) v_cmd (filterAndTransformVelCommandToLocal, 0.8 in the reference); v_filt is the
    caller's filter state ([4], updated IN PLACE when it is a numpy array; None: the command).  The device form is hsqp_command_targets."""
    nj = model.nj
    if filter_alpha != 0.0:
        cmd = np.asarray(v_cmd, dtype=float)
        new = filter_alpha * (cmd if v_filt is None else np.asarray(v_filt, dtype=float)) + (1.0 - filter_alpha) * cmd
        if isinstance(v_filt, np.ndarray):
            v_filt[:] = new
        v_cmd = tuple(float(v) for v in new)
    elif isinstance(v_filt, np.ndarray):
        v_filt[:] = v_cmd
    vx, vy, height, wz = v_cmd
    pose = np.array(x0[:6], dtype=float)
    pose[4] = pose[5] = 0.0
    yaw = pose[3]
    gvx = math.cos(yaw) * vx - math.sin(yaw) * vy
    gvy = math.sin(yaw) * vx + math.cos(yaw) * vy
    target_vel = np.array([gvx, gvy, 0.0, wz, 0.0, 0.0])
    base_vel = np.asarray(x0[6 + nj: 12 + nj])
    t_mid = 0.7 * horizon
    pose[2] = height

    def integrate(p, v3, h, dt):
        q = p.copy()
        q[0] += v3[0] * dt
        q[1] += v3[1] * dt
        q[2] = h
        q[3] += v3[2] * dt
        q[4] = q[5] = 0.0
        return q

    mid = integrate(pose, [(base_vel[0] + gvx) / 2, (base_vel[1] + gvy) / 2, (base_vel[5] + wz) / 2], height, t_mid)
    fin = integrate(mid, [gvx, gvy, wz], height, horizon - t_mid)
    jt = model.default_joint_state
    mk = lambda p: np.concatenate([p, jt, target_vel, np.zeros(nj)])
    return TargetTrajectories([t0, t0 + t_mid, t0 + horizon], [mk(pose), mk(mid), mk(fin)])


# ------------------------------------------------------------------------------------ node table
def weight_compensating_input(model, flags):
    u = np.zeros(model.nu)
    ns = int(flags[0]) + int(flags[1])
    if ns:
        fz = model.total_mass * 9.81 / ns
        if flags[0]:
            u[2] = fz
        if flags[1]:
            u[8] = fz
    return u


def build_node_params(model, schedule, targets, t0, dt, n_nodes, arm_swing=True, terrain_height=0.0, lift=None, touch=None):
    """[N+1][HSQP_NODE_PARAMS] table for one instance on the uniform grid t_k = t0 + k dt.  lift, touch ([2][phases]): the planner's three-argument
    update (include/hsqp_perceive.h) in place of terrain_height."""
    planner = SwingTrajectoryPlanner(model.swing, schedule, terrain_height, lift, touch)
    par = np.zeros((n_nodes + 1, _abi.NODE_PARAMS))
    for k in range(n_nodes + 1):
        t = t0 + k * dt
        flags = mode_to_contact_flags(schedule.mode_at(t))
        par[k, _abi.P_XDES:_abi.P_XDES + model.nx] = targets.desired_state(t)
        par[k, _abi.P_ARMSWING] = math.sin(2.0 * math.pi * (phase_variable(schedule, t) - 0.15)) if arm_swing else 0.0
        par[k, _abi.P_CONTACT:_abi.P_CONTACT + 2] = flags
        for leg in range(2):
            par[k, _abi.P_SWING + 3 * leg:_abi.P_SWING + 3 * leg + 3] = planner.z_refs(leg, t)
            par[k, _abi.P_IMPACT + leg] = planner.impact_proximity(leg, t)
    return par


def swing_config(model):
    """hsqp_swing_config from task.info's swing_trajectory_config."""
    c = model.swing
    return _abi.SwingConfig(lift_off_velocity=c["liftOffVelocity"], touch_down_velocity=c["touchDownVelocity"], swing_height=c["swingHeight"],
                            touch_down_height_offset=c["touchDownHeightOffset"], swing_time_scale=c["swingTimeScale"],
                            impact_mid=c["impactProximityFactorMidPointValue"], impact_lift_velocity=c["impactProximityFactorLiftOffVelocity"],
                            impact_touch_velocity=c["impactProximityFactorTouchDownVelocity"])


def pack_reference(schedules, targets):
    """Compact per-instance reference for hsqp_upload_reference: (n_events[B], event_times[B,E], mode_sequence[B,E+1],
    target_times[B,K], target_states[B,K,58]) from ModeSchedule / TargetTrajectories objects."""
    B = len(schedules)
    E = max(len(s.event_times) for s in schedules)
    K = len(targets[0].times)
    n_events = np.array([len(s.event_times) for s in schedules], dtype=np.int32)
    ev = np.zeros((B, E))
    seq = np.full((B, E + 1), STANCE, dtype=np.int32)
    for b, s in enumerate(schedules):
        ev[b, :n_events[b]] = s.event_times
        ev[b, n_events[b]:] = s.event_times[-1]
        seq[b, :n_events[b] + 1] = s.mode_sequence
    tt = np.stack([t.times for t in targets])
    ts = np.stack([t.states for t in targets])
    assert tt.shape == (B, K) and ts.shape[:2] == (B, K)
    return n_events, ev, seq, tt, ts


def cold_start(model, x0, par):
    """WeightCompInitializer: x_k = x0, u_k = weight compensation for the node's contact flags."""
    n_nodes = par.shape[0] - 1
    x = np.tile(np.asarray(x0, dtype=float), (n_nodes + 1, 1))
    u = np.stack([weight_compensating_input(model, par[k, _abi.P_CONTACT:_abi.P_CONTACT + 2] > 0.5) for k in range(n_nodes)])
    return x, u


# ------------------------------------------------------------------------------------ time grid with event nodes
EVENT_EPS = 1e-9   # a post-event node is sampled at t_event + EVENT_EPS (ocs2 getIntervalStart adds an epsilon of its own)


def time_discretization_with_events(t0, tf, dt, event_times, dt_min=1e-4):
    """ocs2 multiple-shooting time grid (upstream ocs2_oc timeDiscretizationWithEvents, restated from the published source; the fork's
    copy is absent): nodes every dt from t0, an event time inside (t0, tf) becomes a PRE-event node and a POST-event node with the same
    time stamp, the node before it is dropped if it would be closer than dt_min, the last interval is shortened to hit tf.
    Returns (times[n+1], is_post_event[n+1])."""
    times, post = [float(t0)], [False]
    ev = [e for e in event_times if t0 < e < tf]
    ie = 0
    while times[-1] < tf:
        t_next, is_event = times[-1] + dt, False
        if ie < len(ev) and t_next >= ev[ie]:
            t_next, is_event = ev[ie], True
            ie += 1
        if t_next >= tf:
            t_next, is_event = float(tf), False
        if t_next > times[-1] + dt_min or post[-1]:
            times.append(t_next); post.append(False)
        else:
            times[-1] = t_next
        if is_event:
            times.append(t_next); post.append(True)
    return np.array(times), np.array(post)


def event_grid(t0, tf, dt, event_times):
    """(dt_nodes[N], node_times[N+1]) for hsqp_problem::dt_nodes / hsqp_reference::node_times: interval lengths with 0 on the
    pre -> post event intervals, and the sampling time of every node (post-event nodes at t + EVENT_EPS, so that look-ups by
    lower_bound see the new mode)."""
    times, post = time_discretization_with_events(t0, tf, dt, event_times)
    return np.diff(times), times + EVENT_EPS * post


class GridOverflow(RuntimeError):
    """padded_event_grid: the ocs2 grid needs more than n_nodes + event_nodes intervals (HSQP_GRID_OVERFLOW), or the events admit no grid."""


def padded_event_grid(t0, n_nodes, dt, event_times, event_nodes, dt_min=1e-4):
    """The Python mirror of csrc/hsqp_grid.h (include/hsqp_grid.h), operation by operation: event_grid(t0, t0 + n_nodes * dt, dt, events) with the
    builder's bounded loop, padded to N = n_nodes + event_nodes intervals by N - N_b zero-length intervals directly in front of the last interval
    (the padding nodes duplicate node N_b - 1, its sampling time included).  Returns (dts[N], node_times[N + 1], n_intervals = N_b); raises
    GridOverflow where the device answers HSQP_GRID_OVERFLOW."""
    N = int(n_nodes) + int(event_nodes)
    t0, dt, dt_min = float(t0), float(dt), float(dt_min)
    ev = [float(e) for e in event_times]
    tf = t0 + n_nodes * dt
    dts, nts = [0.0] * N, [0.0] * (N + 1)
    n, ie, last, prev, last_post = 1, 0, t0, t0, False
    nts[0] = t0
    cap, passes = N + len(ev) + 2, 0
    while last < tf:
        passes += 1
        if passes > cap:
            raise GridOverflow("the grid's loop does not end")
        while ie < len(ev) and not (t0 < ev[ie] and ev[ie] < tf):
            ie += 1
        t_next, is_event = last + dt, False
        if ie < len(ev) and t_next >= ev[ie]:
            t_next, is_event = ev[ie], True
            ie += 1
        if t_next >= tf:
            t_next, is_event = tf, False
        if t_next > last + dt_min or last_post:
            if n > N:
                raise GridOverflow("more than %d intervals" % N)
            nts[n], dts[n - 1] = t_next, t_next - last
            n, prev, last, last_post = n + 1, last, t_next, False
        else:
            nts[n - 1] = t_next
            if n > 1:
                dts[n - 2] = t_next - prev
            last = t_next
        if is_event:
            if n > N:
                raise GridOverflow("more than %d intervals" % N)
            nts[n], dts[n - 1] = t_next + EVENT_EPS, t_next - last
            n, prev, last, last_post = n + 1, last, t_next, True
    nb = n - 1
    if nb < 1 or not dts[nb - 1] > 0.0 or any(not (dts[k] >= 0.0) or not (dts[k] <= 1e6) for k in range(nb)):
        raise GridOverflow("the events admit no grid")
    if nb < N:
        d_last, t_end, t_dup = dts[nb - 1], nts[nb], nts[nb - 1]
        for k in range(nb - 1, N - 1):
            dts[k], nts[k + 1] = 0.0, t_dup
        dts[N - 1], nts[N] = d_last, t_end
    return np.array(dts), np.array(nts), nb


def raw_stamps(dts, node_times):
    """PrimalSolution time stamps of a grid from its interval lengths and sampling times (event_grid): a post-event node takes the stamp of
    the node before it, so pre- and post-event node share one (what hsqp_upload_reference records, HSQP_BLK_STAMPS)."""
    st = np.array(node_times, dtype=np.float64)
    dts = np.broadcast_to(dts, st.shape[:-1] + (st.shape[-1] - 1,))
    for k in range(1, st.shape[-1]):
        st[..., k] = np.where(dts[..., k - 1] == 0.0, st[..., k - 1], st[..., k])
    return st


def stamped_inputs(times, u):
    """The inputs of a PrimalSolution (HipSqpSolverAdaptor step 5, upstream toPrimalSolution): [..][N+1][35] from [..][N][35] and the raw
    stamps [N+1]; a pre-event node (zero-length interval k, 0 < k < N) repeats the input before it, the last input is repeated."""
    u = np.array(u, dtype=np.float64)
    N = u.shape[-2]
    for k in range(1, N):
        if times[k + 1] == times[k]:
            u[..., k, :] = u[..., k - 1, :]
    return np.concatenate([u, u[..., N - 1:N, :]], axis=-2)


def _interp_at(t, v, tau):
    """ocs2 LinearInterpolation (clamped, std::upper_bound on the stamps t) of rows v[B][len(t)][n] at the times tau, unfused like the host."""
    i = np.clip(np.searchsorted(t, tau, side="right"), 1, len(t) - 1)
    h = t[i] - t[i - 1]
    a = np.where(h > 0.0, (tau - t[i - 1]) / np.where(h > 0.0, h, 1.0), 1.0)
    blend = (1.0 - a)[None, :, None] * v[:, i - 1] + a[None, :, None] * v[:, i]
    return np.where((tau <= t[0])[None, :, None], v[:, :1], np.where((tau >= t[-1])[None, :, None], v[:, -1:], blend))


def host_warm_start(total_mass, x_init, times, contact, prev=None, nx=_abi.NX):
    """The adaptor's host warm start (HipSqpSolverAdaptor::runImpl steps 2 and 5; upstream SqpSolver::runImpl with the reference's
    WeightCompInitializer), batched: the previous solution interpolated onto the new grid's raw stamps, the nodes past its last stamp
    from the initializer (state of the node before / x_init, weight-compensating input of the node's contact flags).
    x_init [B][58]; times: raw stamps [N+1] (shared) or [B][N+1]; contact: flags [B][N(+1)][2]; prev: None (cold start) or
    dict(times=[Np+1] or [B][Np+1], x=[B][Np+1][58], u=[B][Np][35]) — the solution as hsqp_download returns it.  The arithmetic of the
    adaptor, element by element (what hsqp_reference::warm_start reproduces on the device).  Returns (x [B][N+1][58], u [B][N][35])."""
    x_init = np.asarray(x_init, dtype=np.float64)
    B = x_init.shape[0]
    times = np.asarray(times, dtype=np.float64)
    pt = None if prev is None else np.asarray(prev["times"], dtype=np.float64)
    if times.ndim == 2 or (pt is not None and pt.ndim == 2):
        outs = [host_warm_start(total_mass, x_init[b:b + 1], times[b] if times.ndim == 2 else times, contact[b:b + 1],
                                None if prev is None else dict(times=pt[b] if pt.ndim == 2 else pt, x=prev["x"][b:b + 1], u=prev["u"][b:b + 1]), nx)
                for b in range(B)]
        return np.concatenate([o[0] for o in outs]), np.concatenate([o[1] for o in outs])
    N = len(times) - 1
    x, u = np.zeros((B, N + 1, _abi.NX)), np.zeros((B, N, _abi.NU))
    kc = 0 if pt is None else int(np.count_nonzero(times <= pt[-1]))   # the stamps do not decrease: the covered nodes are a prefix
    if kc:
        x[:, :kc, :nx] = _interp_at(pt, np.asarray(prev["x"], dtype=np.float64)[:, :, :nx], times[:kc])
        ku = min(kc, N)
        u[:, :ku] = _interp_at(pt, stamped_inputs(pt, prev["u"]), times[:ku])
    x[:, kc:, :nx] = (x[:, kc - 1, :nx] if kc else x_init[:, :nx])[:, None, :]
    c = np.asarray(contact)[:, kc:N] > 0.5
    ns = c[..., 0].astype(np.int64) + c[..., 1].astype(np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        fz = total_mass * 9.81 / ns
    u[:, kc:, 2] = np.where(c[..., 0], fz, 0.0)
    u[:, kc:, 8] = np.where(c[..., 1], fz, 0.0)
    return x, u


def build_node_params_at(model, schedule, targets, node_times, arm_swing=True, terrain_height=0.0, lift=None, touch=None):
    """build_node_params on explicit node times (non-uniform grid / event nodes)."""
    planner = SwingTrajectoryPlanner(model.swing, schedule, terrain_height, lift, touch)
    par = np.zeros((len(node_times), _abi.NODE_PARAMS))
    for k, t in enumerate(node_times):
        flags = mode_to_contact_flags(schedule.mode_at(t))
        par[k, _abi.P_XDES:_abi.P_XDES + model.nx] = targets.desired_state(t)
        par[k, _abi.P_ARMSWING] = math.sin(2.0 * math.pi * (phase_variable(schedule, t) - 0.15)) if arm_swing else 0.0
        par[k, _abi.P_CONTACT:_abi.P_CONTACT + 2] = flags
        for leg in range(2):
            par[k, _abi.P_SWING + 3 * leg:_abi.P_SWING + 3 * leg + 3] = planner.z_refs(leg, t)
            par[k, _abi.P_IMPACT + leg] = planner.impact_proximity(leg, t)
    return par


# ------------------------------------------------------------------------------------ benchmark configs
BENCH_SEED = 20250808


def make_problem(model, n_nodes=100, batch=1, gait="walk", v_cmd=(0.3, 0.0, 0.7925, 0.0), dt=None, perturb=False,
                 seed=BENCH_SEED, t0=0.0, with_reference=False):
    """Synthetic inputs of BASELINE.md configs 3-5: (x_init[B,58], x[B,N+1,58], u[B,N,35], params[B,N+1,72], dt).

    perturb=False: every instance starts at task.info's initialState with gait phase offset 0 (config 3).
    with_reference=True additionally returns (schedules, targets, t0) for the device-side parameter generation.
    perturb=True : x0 + N(0, sigma^2) (0.02 m base position, 0.05 rad euler/joints, 0.1 velocities; joints clipped to
                   limits - 0.05 rad) and a per-instance gait phase offset U[0, 1.4 s) from numpy PCG64(seed) (configs 4-5).
    """
    dt = model.sqp["dt"] if dt is None else dt
    horizon = n_nodes * dt
    rng = np.random.Generator(np.random.PCG64(seed))
    nj = model.nj
    xs, us, ps, x0s = [], [], [], []
    schedules, targets_all = [], []
    for _ in range(batch):
        x0 = model.initial_state.copy()
        offset = 0.0
        if perturb:
            sig = np.concatenate([np.full(3, 0.02), np.full(3 + nj, 0.05), np.full(6 + nj, 0.1)])
            x0 = x0 + sig * rng.standard_normal(model.nx)
            x0[6:6 + nj] = np.clip(x0[6:6 + nj], model.q_lo + 0.05, model.q_hi - 0.05)
            offset = rng.uniform(0.0, 1.4)
        # the gait starts `offset` seconds before t0, preceded by stance; tile far enough past the horizon that
        # every swing phase has a touch-down inside the schedule
        schedule = tile_gait(model.gaits[gait], t0 - offset - 1e-9, t0 + 2.0 * horizon + 3.0)
        targets = velocity_command_targets(model, v_cmd, t0, x0, horizon)
        par = build_node_params(model, schedule, targets, t0, dt, n_nodes)
        x, u = cold_start(model, x0, par)
        xs.append(x); us.append(u); ps.append(par); x0s.append(x0)
        schedules.append(schedule); targets_all.append(targets)
    if with_reference:
        return np.stack(x0s), np.stack(xs), np.stack(us), np.stack(ps), dt, (schedules, targets_all, t0)
    return np.stack(x0s), np.stack(xs), np.stack(us), np.stack(ps), dt


# ------------------------------------------------------------------------------------ centroidal formulation
# Host-side parameter generation of the centroidal problem.  States are handled unpadded (35) in this section and padded to the
# ABI's 58-double rows by make_centroidal_problem().
def _rot_axis(axis, q):
    a = np.asarray(axis, dtype=float)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(q) * K + (1.0 - math.cos(q)) * (K @ K)


def body_placements(model, q):
    """World placements (R[NB], p[NB]) of the MPC model's bodies at q = [p_b, eulerZYX, q_j] (composite Translation +
    SphericalZYX base: createPinocchioModel.cpp:60-67)."""
    bodies = model.raw["bodies"]
    R, p = [None] * len(bodies), [None] * len(bodies)
    R[0] = _rot_axis([0, 0, 1], q[3]) @ _rot_axis([0, 1, 0], q[4]) @ _rot_axis([1, 0, 0], q[5])
    p[0] = np.array(q[:3], dtype=float)
    for i in range(1, len(bodies)):
        b = bodies[i]
        par = b["parent"]
        R[i] = R[par] @ np.array(b["R"]).reshape(3, 3) @ _rot_axis(b["axis"], q[5 + i])
        p[i] = p[par] + R[par] @ np.array(b["p"])
    return R, p


def contact_frame_xy(model, q, f):
    """World xy of contact frame f at q = [p_b, eulerZYX, q_j]."""
    R, p = body_placements(model, q)
    fr = model.raw["frames"]["contact"][f]
    return (p[fr["body"]] + R[fr["body"]] @ np.array(fr["p"], dtype=float))[:2]


def foot_height_sequences(model, x, t, schedule, targets, ground, offset=None):
    """The rule of include/hsqp_perceive.h for one instance (OURS, not the reference's): (lift[2][n], touch[2][n], foothold_xy[2][n][2]) over the n
    phases of `schedule` from the state x at time t; targets: the TargetTrajectories; ground(X, Y): the instance's ground height under a world point
    (hsqp_terrain_eval's answer); offset: touchDownHeightOffset (None: the model's).  A contact run that began at or before the phase of t stands where
    the foot is; a run ahead lands where the targets carry the nominal foothold (the contact frame at the default joint state, base at the origin) at
    its touch-down time.  A non-finite state: NaN rows."""
    offset = model.swing["touchDownHeightOffset"] if offset is None else offset
    seq, ev = schedule.mode_sequence, schedule.event_times
    n = len(seq)
    lift, touch, fxy = np.zeros((2, n)), np.zeros((2, n)), np.zeros((2, n, 2))
    x = np.asarray(x, dtype=float)
    if not np.isfinite(x).all():
        return lift + np.nan, touch + np.nan, fxy + np.nan
    p_now = schedule.index_at(t)
    nv = 6 + model.nj
    q_nominal = np.concatenate([np.zeros(6), model.default_joint_state])
    for f in range(2):
        c = [mode_to_contact_flags(m)[f] for m in seq]
        P, o = contact_frame_xy(model, x[:nv], f), contact_frame_xy(model, q_nominal, f)
        h_run, F_run = [None] * n, [None] * n
        for p in range(n):
            if not c[p]:
                continue
            if p > 0 and c[p - 1]:
                h_run[p], F_run[p] = h_run[p - 1], F_run[p - 1]
                continue
            if p <= p_now:
                F = P
            else:
                d = targets.desired_state(ev[p - 1])
                X, Y, psi = d[0], d[1], d[3]
                F = np.array([X + math.cos(psi) * o[0] - math.sin(psi) * o[1], Y + math.sin(psi) * o[0] + math.cos(psi) * o[1]])
            h_run[p], F_run[p] = ground(F[0], F[1]), F
        for p in range(n):
            if c[p]:
                lift[f, p], touch[f, p], fxy[f, p] = h_run[p], h_run[p] + offset, F_run[p]
                continue
            before = next((q for q in range(p - 1, -1, -1) if c[q]), None)
            after = next((q for q in range(p + 1, n) if c[q]), None)
            lift[f, p] = h_run[before] if before is not None else ground(P[0], P[1])
            touch[f, p] = (h_run[after] if after is not None else lift[f, p]) + offset
            fxy[f, p] = F_run[after] if after is not None else P
    return lift, touch, fxy


def euler_rate_axes(q):
    """World axes of the euler Z, Y, X rates: omega = E @ [zdot, ydot, xdot]."""
    Rz = _rot_axis([0, 0, 1], q[3])
    Rzy = Rz @ _rot_axis([0, 1, 0], q[4])
    return np.stack([np.array([0.0, 0.0, 1.0]), Rz[:, 1], Rzy[:, 0]], axis=1)


def centroidal_base_velocity(model, q, h_normalized, qd_j=None):
    """v_b = A_b^-1 (m h - A_j qd_j): CentroidalModelPinocchioMapping::getPinocchioJointVelocity (upstream ocs2_centroidal_model,
    FullCentroidalDynamics) evaluated from the composite inertia of the whole robot about its centre of mass."""
    bodies = model.raw["bodies"]
    R, p = body_placements(model, q)
    m = model.total_mass
    cs = [p[i] + R[i] @ np.array(b["com"]) for i, b in enumerate(bodies)]
    com = sum(b["mass"] * c for b, c in zip(bodies, cs)) / m
    Ic = np.zeros((3, 3))
    for i, b in enumerate(bodies):
        d = cs[i] - com
        Ic += R[i] @ np.array(b["inertia"]).reshape(3, 3) @ R[i].T + b["mass"] * (d @ d * np.eye(3) - np.outer(d, d))
    lin_j, ang_j = np.zeros(3), np.zeros(3)
    if qd_j is not None:   # momentum of the joint motion about the centre of mass
        om, v = [np.zeros(3)] * len(bodies), [np.zeros(3)] * len(bodies)
        for i in range(1, len(bodies)):
            b = bodies[i]
            par = b["parent"]
            w = R[par] @ np.array(b["R"]).reshape(3, 3) @ np.array(b["axis"])
            om[i] = om[par] + w * qd_j[i - 1]
            v[i] = v[par] + np.cross(om[par], p[i] - p[par])
            vc = v[i] + np.cross(om[i], cs[i] - p[i])
            lin_j = lin_j + b["mass"] * vc
            ang_j = ang_j + R[i] @ np.array(b["inertia"]).reshape(3, 3) @ R[i].T @ om[i] + np.cross(cs[i] - com, b["mass"] * vc)
    E = euler_rate_axes(q)
    rhs_lin, rhs_ang = m * np.asarray(h_normalized[:3]) - lin_j, m * np.asarray(h_normalized[3:6]) - ang_j
    euler_rates = np.linalg.solve(Ic @ E, rhs_ang)
    omega = E @ euler_rates
    vlin = rhs_lin / m - np.cross(omega, com - p[0])
    return np.concatenate([vlin, euler_rates])


def matrix_to_quaternion(R):
    """x, y, z, w (Eigen coefficient order), w >= 0 branch first (oracle ASSUMPTION A8)."""
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0.0:
        s = math.sqrt(tr + 1.0) * 2.0
        return np.array([(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, 0.25 * s])
    i = int(np.argmax(np.diag(R)))
    j, k = (i + 1) % 3, (i + 2) % 3
    s = math.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k]) * 2.0
    qv = np.zeros(4)
    qv[i] = 0.25 * s
    qv[j] = (R[i, j] + R[j, i]) / s
    qv[k] = (R[i, k] + R[k, i]) / s
    qv[3] = (R[k, j] - R[j, k]) / s
    return qv


def torso_reference(model, x_ref):
    """EndEffectorKinematicsQuadraticCost::getReferenceCostElement (EndEffectorKinematicsQuadraticCost.cpp:92-104): the torso
    link's position, orientation quaternion and LOCAL_WORLD_ALIGNED velocities at (xRef, uRef = 0)."""
    t = model.raw["torso"]
    q = np.asarray(x_ref[6:35], dtype=float)
    R, p = body_placements(model, q)
    b = t["body"]
    vb = centroidal_base_velocity(model, q, x_ref[:6])
    omega = euler_rate_axes(q) @ vb[3:6]
    r = R[b] @ np.array(t["p"])
    pos = p[b] + r
    vlin = vb[:3] + np.cross(omega, pos - p[0])
    return np.concatenate([pos, matrix_to_quaternion(R[b] @ np.array(t["R"]).reshape(3, 3)), vlin, omega])


def centroidal_velocity_command_targets(model, v_cmd, t0, x0, horizon, filter_alpha=0.0, v_filt=None):
    """CentroidalMpcTargetTrajectoriesCalculator::commandedVelocityToTargetTrajectories
    (humanoid_centroidal_mpc/src/command/CentroidalMpcTargetTrajectoriesCalculator.cpp:88-158).  Default: the command filter at steady state;
    filter_alpha, v_filt: the semantics of velocity_command_targets (v_filt [4] is updated IN PLACE when it is a numpy array).  The device form
    is hsqp_centroidal_command_targets."""
    if filter_alpha != 0.0:
        cmd = np.asarray(v_cmd, dtype=float)
        new = filter_alpha * (cmd if v_filt is None else np.asarray(v_filt, dtype=float)) + (1.0 - filter_alpha) * cmd
        if isinstance(v_filt, np.ndarray):
            v_filt[:] = new
        v_cmd = tuple(float(v) for v in new)
    elif isinstance(v_filt, np.ndarray):
        v_filt[:] = v_cmd
    vx, vy, height, wz = v_cmd
    pose = np.array(x0[6:12], dtype=float)
    pose[4] = pose[5] = 0.0
    yaw = pose[3]
    gvx = math.cos(yaw) * vx - math.sin(yaw) * vy
    gvy = math.sin(yaw) * vx + math.cos(yaw) * vy
    target_momentum = np.array([gvx, gvy, 0.0, 0.0, 0.0, wz / model.total_mass])
    base_vel = centroidal_base_velocity(model, np.asarray(x0[6:35]), x0[:6])   # "assumes no joint velocities"
    # the reference reads baseVel[5] (the euler X rate) as the yaw rate here; reproduced
    t_mid = 0.7 * horizon
    pose[2] = height

    def integrate(pp, v3, h, dt):
        qq = pp.copy()
        qq[0] += v3[0] * dt
        qq[1] += v3[1] * dt
        qq[2] = h
        qq[3] += v3[2] * dt
        qq[4] = qq[5] = 0.0
        return qq

    mid = integrate(pose, [(base_vel[0] + gvx) / 2, (base_vel[1] + gvy) / 2, (base_vel[5] + wz) / 2], height, t_mid)
    fin = integrate(mid, [gvx, gvy, wz], height, horizon - t_mid)
    jt = model.default_joint_state
    mk = lambda pp: np.concatenate([target_momentum, pp, jt])
    return TargetTrajectories([t0, t0 + t_mid, t0 + horizon], [mk(pose), mk(mid), mk(fin)])


def build_centroidal_node_params(model, schedule, targets, t0, dt, n_nodes, arm_swing=True):
    """[N+1][HSQP_NODE_PARAMS] table of the centroidal problem (layout: include/hsqp.h)."""
    planner = SwingTrajectoryPlanner(model.swing, schedule)
    par = np.zeros((n_nodes + 1, _abi.NODE_PARAMS))
    for k in range(n_nodes + 1):
        t = t0 + k * dt
        flags = mode_to_contact_flags(schedule.mode_at(t))
        xd = targets.desired_state(t)
        par[k, _abi.P_XDES:_abi.P_XDES + _abi.CNX] = xd
        par[k, _abi.PC_TORSO:_abi.PC_TORSO + 13] = torso_reference(model, xd)
        par[k, _abi.P_ARMSWING] = math.sin(2.0 * math.pi * (phase_variable(schedule, t) - 0.15)) if arm_swing else 0.0
        par[k, _abi.P_CONTACT:_abi.P_CONTACT + 2] = flags
        for leg in range(2):
            z, zd, _ = planner.z_refs(leg, t)
            par[k, _abi.P_SWING + 3 * leg:_abi.P_SWING + 3 * leg + 3] = (z, zd, 0.0)
            par[k, _abi.P_IMPACT + leg] = planner.impact_proximity(leg, t)
    return par


def pad_targets(targets):
    """TargetTrajectories with the 35-wide centroidal knots padded to the ABI's 58-double rows (for pack_reference)."""
    st = np.zeros((len(targets.times), _abi.NX))
    st[:, :_abi.CNX] = targets.states
    return TargetTrajectories(targets.times, st)


def make_centroidal_problem(model, n_nodes=100, batch=1, gait="walk", v_cmd=(0.3, 0.0, 0.7925, 0.0), dt=None, perturb=False,
                            seed=BENCH_SEED, t0=0.0, with_reference=False):
    """Synthetic inputs of BASELINE.md configs 1-2 in the ABI's padded layout: (x_init[B,58], x[B,N+1,58], u[B,N,35],
    params[B,N+1,72], dt); only the first 35 entries of a state row are used.  Cold start as CentroidalWeightCompInitializer
    (x_k = x0 with the momentum extended, u_k = weight compensation)."""
    assert model.centroidal
    dt = model.sqp["dt"] if dt is None else dt
    horizon = n_nodes * dt
    rng = np.random.Generator(np.random.PCG64(seed))
    nj = model.nj
    xs, us, ps, x0s = [], [], [], []
    schedules, targets_all = [], []
    for _ in range(batch):
        x0 = model.initial_state.copy()
        offset = 0.0
        if perturb:
            sig = np.concatenate([np.full(6, 0.1), np.full(3, 0.02), np.full(3 + nj, 0.05)])
            x0 = x0 + sig * rng.standard_normal(model.nx)
            x0[12:12 + nj] = np.clip(x0[12:12 + nj], model.q_lo + 0.05, model.q_hi - 0.05)
            offset = rng.uniform(0.0, 1.4)
        schedule = tile_gait(model.gaits[gait], t0 - offset - 1e-9, t0 + 2.0 * horizon + 3.0)
        targets = centroidal_velocity_command_targets(model, v_cmd, t0, x0, horizon)
        par = build_centroidal_node_params(model, schedule, targets, t0, dt, n_nodes)
        x0p = np.zeros(_abi.NX)
        x0p[:_abi.CNX] = x0
        x, u = cold_start(model, x0p, par)
        xs.append(x); us.append(u); ps.append(par); x0s.append(x0p)
        schedules.append(schedule); targets_all.append(pad_targets(targets))
    if with_reference:
        return np.stack(x0s), np.stack(xs), np.stack(us), np.stack(ps), dt, (schedules, targets_all, t0)
    return np.stack(x0s), np.stack(xs), np.stack(us), np.stack(ps), dt


# ---- Riccati feedback policy (include/hsqp_feedback.h): the rules of csrc/hsqp_feedback.h restated for the tests
def feedback_source_nodes(dts):
    """Node whose gains each of the N + 1 policy entries carries (dts: the N interval lengths, 0 = event): node N takes node N - 1's, a
    pre-event node i (0 < i, dts[i] == 0) node i - 1's, chained over consecutive events."""
    dts = np.asarray(dts, dtype=float)
    N = len(dts)
    out = np.empty(N + 1, dtype=int)
    for i in range(N + 1):
        k = min(i, N - 1)
        while k > 0 and dts[k] == 0.0:
            k -= 1
        out[i] = k
    return out


def feedback_gains(Px, Pu, Kt, nut, cent=False):
    """K = Px + Pu[:, :nut] K~[:nut] of one node (Px [35][58], Pu [35][23], K~ [23][58]); centroidal: columns 35.. are zero."""
    nc = _abi.CNX if cent else _abi.NX
    K = np.zeros((_abi.NU, _abi.NX))
    K[:, :nc] = Px[:, :nc] + Pu[:, :nut] @ Kt[:nut, :nc]
    return K


def policy_input_segment(N, dt, s, dts=None):
    """(ku, au): the input segment and weight of the policy evaluation at s (csrc/hsqp_feedback.h policy_segment_*; dts None: uniform dt)."""
    if dts is None:
        a = max(s / dt, 0.0)
        ku = int(a)
        au = a - ku
        if ku > N - 2:
            ku = max(N - 2, 0)
            au = min(a - ku, 1.0) if N >= 2 else 0.0
        return ku, au
    s = max(s, 0.0)
    tk, kx = 0.0, 0
    while kx < N - 1 and tk + dts[kx] <= s:
        tk += dts[kx]
        kx += 1
    while kx < N - 1 and dts[kx] == 0.0:
        kx += 1
    h = dts[kx]
    ax = min((s - tk) / h if h > 0.0 else 1.0, 1.0)
    ku, au = kx, ax
    if ku > N - 2:
        ku, au = max(N - 2, 0), (1.0 if N >= 2 else 0.0)
    if N >= 2 and dts[ku] == 0.0:
        au = 1.0
    elif N >= 2 and ku + 1 <= N - 1 and dts[ku + 1] == 0.0:
        au = 0.0
    return ku, au


def linear_controller_input(times, uff, K, t, x):
    """ocs2 LinearController::computeInput: uff(t) + K(t) x on LinearInterpolation::timeSegment (std::lower_bound on the stamps; the value is
    alpha v[i] + (1 - alpha) v[i + 1]).  times [n], uff [n][nu], K [n][nu][nx], x [nx]."""
    times = np.asarray(times, dtype=float)
    n = len(times)
    if n <= 1:
        i, alpha = 0, 1.0
    else:
        idx = int(np.searchsorted(times, t, side="left"))
        if idx <= 0:
            i, alpha = 0, 1.0
        elif idx > n - 1:
            i, alpha = n - 2, 0.0
        else:
            i, alpha = idx - 1, (times[idx] - t) / (times[idx] - times[idx - 1])
    j = min(i + 1, n - 1)
    Ks = alpha * K[i] + (1.0 - alpha) * K[j]
    return alpha * uff[i] + (1.0 - alpha) * uff[j] + Ks @ x


# ---- per-instance gait schedule and gait ladder (include/hsqp_gait.h): csrc/hsqp_gait.h restated for the tests, line by line from
#      GaitSchedule.cpp:53-145, GaitScheduleUpdater.cpp:45-69 and ProceduralMpcMotionManager.cpp:86-159.  Python floats are IEEE doubles and
#      nothing here is fused, so the mirror, the host build of the kernel source and the device agree bit for bit.
GAIT_OK, GAIT_OVERFLOW, GAIT_BAD_TILING = 0, 1, 2
# ProceduralMpcMotionManager.h:110-118: gaitCommand, minLinVelCmd, maxLinVelCmd, minAngVelCmd, maxAngVelCmd, linVelErrorThresh, angVelErrorThresh
GAIT_LADDER = (("stance", -0.1, 0.1, -0.1, 0.1, 10.0, 10.0),      # "Large threshold allows switching away from stance purely command based"
               ("slow_walk", 0.05, 0.3, 0.05, 0.2, 0.05, 0.05),
               ("walk", 0.25, 0.5, 0.15, 0.35, 0.05, 0.05),
               ("slower_trot", 0.45, 0.7, 0.3, 0.55, 0.1, 0.1),
               ("slow_trot", 0.65, 0.9, 0.5, 0.7, 0.2, 0.2),
               ("trot", 0.8, 1.3, 0.65, 10.0, 0.2, 0.2),
               ("run", 1.2, 10.0, 0.65, 10.0, 0.2, 0.2))


class GaitTilingError(RuntimeError):
    """'The initial time for template-tiling is not greater than the last event time.' (GaitSchedule.cpp:127-129)"""


class GaitOverflow(RuntimeError):
    """the schedule would exceed max_events (a limit of the device form, not of the reference)"""


class GaitSchedule:
    """GaitSchedule.cpp.  template: (switching_times, modes) with modes as numbers; max_events: None (the reference) or the device's capacity."""

    def __init__(self, event_times, mode_sequence, template, phase_transition_stance_time=0.0, max_events=None):
        self.event_times, self.mode_sequence = list(event_times), list(mode_sequence)
        self.template = (list(template[0]), list(template[1]))
        self.phase_transition_stance_time = phase_transition_stance_time
        self.max_events = max_events

    def _push_event(self, t):
        if self.max_events is not None and len(self.event_times) >= self.max_events:
            raise GaitOverflow()
        self.event_times.append(t)

    def _push_mode(self, m):
        if self.max_events is not None and len(self.mode_sequence) > self.max_events:
            raise GaitOverflow()
        self.mode_sequence.append(m)

    def tile(self, start, final):
        """tileModeSequenceTemplate (GaitSchedule.cpp:115-145)"""
        times, modes = self.template
        if not modes:
            return
        if self.event_times and start <= self.event_times[-1]:
            raise GaitTilingError()
        self._push_event(start)
        while self.event_times[-1] < final:
            for i, m in enumerate(modes):
                self._push_mode(m)
                self._push_event(self.event_times[-1] + (times[i + 1] - times[i]))
        self._push_mode(STANCE)

    def insert_template(self, template, start, final):
        """insertModeSequenceTemplate (GaitSchedule.cpp:53-80)"""
        self.template = (list(template[0]), list(template[1]))
        ev, seq = self.event_times, self.mode_sequence
        index = bisect.bisect_left(ev, start)
        if index < len(ev):
            del ev[index:]
            del seq[index + 1:]
        pts = self.phase_transition_stance_time
        if seq and seq[-1] == STANCE:
            pts = 0.0
        if pts > 0.0:
            self._push_event(start)
            self._push_mode(STANCE)
        self.tile(start + pts, final)

    def get_mode_schedule(self, lower, upper):
        """getModeSchedule (GaitSchedule.cpp:85-110): trims and re-tiles the resident schedule, returns copies of (event_times, mode_sequence)"""
        ev, seq = self.event_times, self.mode_sequence
        index = bisect.bisect_left(ev, lower)
        if index > 0:
            del ev[:index - 1]
            del seq[:index - 1]
            seq[0] = STANCE
        if not ev:
            raise GaitTilingError()      # (the reference erases end() - 1 of an empty vector)
        tiling_start = ev[-1]
        del ev[-1:]
        del seq[-1:]
        self.tile(tiling_start, upper)
        return list(ev), list(seq)


def update_gait_schedule(gs, template, init_time, final_time):
    """GaitScheduleUpdater::updateGaitSchedule (GaitScheduleUpdater.cpp:45-69)"""
    horizon = final_time - init_time
    earliest = 0.7 * final_time + 0.3 * init_time
    ev, seq = gs.get_mode_schedule(init_time, final_time + horizon)
    it = bisect.bisect_right(ev, earliest)
    if it == len(ev):
        nxt = final_time
    elif seq[bisect.bisect_left(ev, ev[it])] == LF:       # modeSchedule.modeAtTime(*it)
        if it == 0:
            raise GaitTilingError()                        # (*(it - 1) of begin(): not reachable, the front mode of a trimmed schedule is STANCE)
        nxt = ev[it - 1]
    else:
        nxt = ev[it]
    gs.insert_template(template, nxt, 1.5 * horizon)      # a duration where a time is expected: kept


def transition_to_faster_gait(cmd, base_vel, cfg):
    """cfg: a row of GAIT_LADDER (or of gait_settings' rungs) without its name: (minLin, maxLin, minAng, maxAng, linThresh, angThresh)"""
    _, max_lin, _, max_ang, lin_thr, ang_thr = cfg
    requested = abs(cmd[0]) > max_lin or abs(cmd[1]) > max_lin or abs(cmd[3]) > max_ang
    within = abs(base_vel[0]) > max_lin - lin_thr or abs(base_vel[1]) > max_lin - lin_thr or abs(base_vel[3]) > max_ang - ang_thr
    return requested and within


def transition_to_slower_gait(cmd, base_vel, cfg):
    min_lin, _, min_ang, _, lin_thr, ang_thr = cfg
    requested = abs(cmd[0]) < min_lin and abs(cmd[1]) < min_lin and abs(cmd[3]) < min_ang
    # the third clause tests velCommandVec(3), not baseVelocity(3) (ProceduralMpcMotionManager.cpp:110): kept
    slow_enough = abs(base_vel[0]) < min_lin + lin_thr and abs(base_vel[1]) < min_lin + lin_thr and abs(cmd[3]) < min_ang + ang_thr
    return requested and slow_enough


def gait_settings(model, ladder=GAIT_LADDER, phase_transition_stance_time=None, min_change_interval=0.2, max_events=128):
    """_abi.GaitSettings: the ladder's thresholds and names with the templates of model.gaits (gait.info) under the rungs' names;
    phase_transition_stance_time None: the exported task.info value."""
    s = _abi.GaitSettings()
    s.n_rungs, s.max_events, s.min_change_interval = len(ladder), int(max_events), float(min_change_interval)
    s.phase_transition_stance_time = float(model.raw["phase_transition_stance_time"] if phase_transition_stance_time is None else phase_transition_stance_time)
    for r, row in enumerate(ladder):
        c, g = s.rungs[r], model.gaits[row[0]]
        (c.min_lin_vel_cmd, c.max_lin_vel_cmd, c.min_ang_vel_cmd, c.max_ang_vel_cmd, c.lin_vel_error_thresh, c.ang_vel_error_thresh) = [float(v) for v in row[1:]]
        c.name = row[0].encode()[:_abi.GAIT_NAME_LEN - 1]
        c.n_phases = len(g["modeSequence"])
        for i, t in enumerate(g["switchingTimes"]):
            c.switching_times[i] = float(t)
        for i, m in enumerate(g["modeSequence"]):
            c.modes[i] = MODE_BY_NAME[m]
    return s


class GaitInstance:
    """The state of one instance after hsqp_gait_reset(settings, t0)."""

    def __init__(self, settings, t0=0.0):
        self.settings = settings
        self.rung = self.command = self.last_command = 0
        self.last_change_time = t0
        self.schedule = GaitSchedule([t0 + 0.5], [STANCE, STANCE], self.template_of(0), settings.phase_transition_stance_time, settings.max_events)

    def template_of(self, r):
        c = self.settings.rungs[r]
        return list(c.switching_times[:c.n_phases + 1]), list(c.modes[:c.n_phases])

    def thresholds_of(self, r):
        c = self.settings.rungs[r]
        return (c.min_lin_vel_cmd, c.max_lin_vel_cmd, c.min_ang_vel_cmd, c.max_ang_vel_cmd, c.lin_vel_error_thresh, c.ang_vel_error_thresh)


def gait_cycle(state, t, horizon, v, x):
    """One update (include/hsqp_gait.h steps 1 to 3) of a GaitInstance at time t with the filtered command v [4] and the measured state x [58]:
    (status, event_times, mode_sequence) of this cycle's schedule.  All or nothing, like the device: a status other than GAIT_OK leaves `state`
    as it was (the schedule of step 1 is still returned where step 1 succeeded)."""
    import copy
    nj = _abi.NJ
    final_time = t + horizon
    th = final_time - t
    s = copy.copy(state)
    s.schedule = copy.deepcopy(state.schedule)
    ev = seq = None
    try:
        ev, seq = s.schedule.get_mode_schedule(t - th, final_time + th)                       # 1. SwitchedModelReferenceManager::modifyReferences
        base_vel = [float(a) for a in x[6 + nj:12 + nj]]                                       # WBAccelMpcRobotModel::getBaseComVelocity
        if t > s.last_change_time + s.settings.min_change_interval:                            # 2. ProceduralMpcMotionManager.cpp:134-152
            cfg = s.thresholds_of(s.rung)
            step = 1 if transition_to_faster_gait(v, base_vel, cfg) else -1 if transition_to_slower_gait(v, base_vel, cfg) else 0
            if step:
                s.rung = min(max(s.rung + step, 0), s.settings.n_rungs - 1)                    # (the clamp is not in the reference)
                s.command = s.rung
                s.last_change_time = t
        if s.command != s.last_command:                                                        # 3. ProceduralMpcMotionManager.cpp:154-159
            update_gait_schedule(s.schedule, s.template_of(s.command), t, final_time)
            s.last_command = s.command
    except GaitOverflow:
        return GAIT_OVERFLOW, ev, seq
    except GaitTilingError:
        return GAIT_BAD_TILING, ev, seq
    state.__dict__.update(s.__dict__)
    return GAIT_OK, ev, seq
