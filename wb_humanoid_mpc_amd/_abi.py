"""ctypes mirror of include/hsqp.h (the C ABI of the HIP SQP library).

Field order and sizes must match the header exactly; tests/test_abi.py checks
sizeof() of every struct against the values the C library reports.
"""
import ctypes as C

NJ, NV, NX, NU, NB = 23, 29, 58, 35, 24
NZ = NX + NU
NE_MAX = 14
NODE_PARAMS = 72
P_XDES, P_ARMSWING, P_CONTACT, P_SWING, P_IMPACT = 0, 58, 59, 61, 67
FORM_WB, FORM_CENTROIDAL = 0, 1
CNX, PC_TORSO = 35, 35

ABI_VERSION = 7   # HSQP_ABI_VERSION of include/hsqp.h (tests/test_abi.py compares them)

OK, ERR_BAD_ARG, ERR_NO_DEVICE, ERR_OOM, ERR_NUMERIC, ERR_HIP, ERR_NOT_CONVERGED = 0, -1, -2, -3, -4, -5, -6

BLK_AB, BLK_BVEC, BLK_H, BLK_G, BLK_CDE, BLK_NE, BLK_COST, BLK_DX, BLK_DU, BLK_FLOW = range(1, 11)
BLK_PARAMS, BLK_FORMS = 11, 12
BLK_X, BLK_U, BLK_STAMPS = 13, 14, 15
WARM_CALLER, WARM_SHIFT, WARM_COLD = 0, 1, 2   # hsqp_reference::warm_start
COMM_ID_BYTES = 128   # HSQP_COMM_ID_BYTES
# hsqp_iterate_device flags (include/hsqp.h; VALUE_FUNCTION: include/hsqp_value.h)
ITER_TAKE_STEP, ITER_KKT, ITER_LINESEARCH, ITER_UNTIL_CONVERGED, ITER_VALUE_FUNCTION = 1, 2, 4, 8, 16
VF_SIZE = NX * NX + NX   # one node of the sweeps' value-function record: S row-major, then s
VALUE_ENTRY_POINTS = ("hsqp_value_function", "hsqp_value_function_device", "hsqp_evaluate_value_function", "hsqp_evaluate_value_function_device")


class Body(C.Structure):
    _fields_ = [("parent", C.c_int32), ("reserved", C.c_int32), ("R", C.c_double * 9), ("p", C.c_double * 3),
                ("axis", C.c_double * 3), ("mass", C.c_double), ("com", C.c_double * 3),
                ("inertia", C.c_double * 9), ("q_lo", C.c_double), ("q_hi", C.c_double)]


class Frame(C.Structure):
    _fields_ = [("body", C.c_int32), ("reserved", C.c_int32), ("p", C.c_double * 3)]


class Barrier(C.Structure):
    _fields_ = [("mu", C.c_double), ("delta", C.c_double)]


class ModelDesc(C.Structure):
    _fields_ = [("formulation", C.c_int32), ("n_joints", C.c_int32), ("bodies", Body * NB),
                ("contact", Frame * 2), ("collision_p1", Frame * 2), ("collision_p2", Frame * 2),
                ("ankle", Frame * 2), ("knee", Frame * 2), ("gravity", C.c_double),
                ("Q", C.c_double * NX), ("R", C.c_double * NU), ("Qf", C.c_double * NX),
                ("foot_sqrt_w", C.c_double * 18),
                ("gain_pos_z", C.c_double), ("gain_ori", C.c_double), ("gain_linvel_z", C.c_double),
                ("gain_linvel_xy", C.c_double), ("gain_angvel", C.c_double), ("gain_linacc_z", C.c_double),
                ("gain_linacc_xy", C.c_double), ("gain_angacc", C.c_double),
                ("friction_mu", C.c_double), ("friction_reg", C.c_double), ("friction_grip", C.c_double),
                ("friction_hess_shift", C.c_double), ("friction_barrier", Barrier),
                ("rect_x_min", C.c_double), ("rect_x_max", C.c_double), ("rect_y_min", C.c_double),
                ("rect_y_max", C.c_double), ("moment_barrier", Barrier), ("joint_limit_barrier", Barrier),
                ("r_foot", C.c_double), ("r_knee", C.c_double), ("collision_barrier", Barrier),
                ("arm_swing_joint", C.c_int32 * 4),
                ("torso", Frame), ("torso_R", C.c_double * 9), ("torso_sqrt_w", C.c_double * 12),
                ("cent_foot_sqrt_w", C.c_double * 12), ("ext_torque_sqrt_w", (C.c_double * 6) * 2),
                ("ext_torque_joint", (C.c_int32 * 6) * 2)]


class Settings(C.Structure):
    _fields_ = [("max_nodes", C.c_int32), ("max_batch", C.c_int32), ("device", C.c_int32), ("flags", C.c_int32)]


class Problem(C.Structure):
    _fields_ = [("batch", C.c_int32), ("n_nodes", C.c_int32), ("dt", C.c_double),
                ("x_init", C.POINTER(C.c_double)), ("x_traj", C.POINTER(C.c_double)),
                ("u_traj", C.POINTER(C.c_double)), ("node_params", C.POINTER(C.c_double)), ("dt_nodes", C.POINTER(C.c_double))]


class Perf(C.Structure):
    _fields_ = [("merit", C.c_double), ("cost", C.c_double), ("dynamics_sse", C.c_double),
                ("equality_sse", C.c_double)]


class Timings(C.Structure):
    _fields_ = [("lq_approximation", C.c_double), ("solve_qp", C.c_double), ("linesearch", C.c_double),
                ("compute_controller", C.c_double), ("total", C.c_double)]


class Solution(C.Structure):
    _fields_ = [("x", C.POINTER(C.c_double)), ("u", C.POINTER(C.c_double)), ("dx", C.POINTER(C.c_double)),
                ("du", C.POINTER(C.c_double)), ("perf_before", C.POINTER(Perf)), ("perf_after", C.POINTER(Perf)),
                ("kkt", C.POINTER(C.c_double)), ("alpha", C.POINTER(C.c_double)), ("step_type", C.POINTER(C.c_int32)),
                ("armijo", C.POINTER(C.c_double)), ("grad_inf", C.POINTER(C.c_double)), ("timings", Timings)]


class SwingConfig(C.Structure):
    _fields_ = [("lift_off_velocity", C.c_double), ("touch_down_velocity", C.c_double), ("swing_height", C.c_double),
                ("touch_down_height_offset", C.c_double), ("swing_time_scale", C.c_double), ("impact_mid", C.c_double),
                ("impact_lift_velocity", C.c_double), ("impact_touch_velocity", C.c_double)]


class Reference(C.Structure):
    _fields_ = [("batch", C.c_int32), ("n_nodes", C.c_int32), ("t0", C.c_double), ("dt", C.c_double), ("max_events", C.c_int32),
                ("n_events", C.POINTER(C.c_int32)), ("event_times", C.POINTER(C.c_double)), ("mode_sequence", C.POINTER(C.c_int32)),
                ("n_knots", C.c_int32), ("target_times", C.POINTER(C.c_double)), ("target_states", C.POINTER(C.c_double)),
                ("swing", SwingConfig), ("terrain_height", C.c_double), ("arm_swing", C.c_int32), ("warm_start", C.c_int32),
                ("node_times", C.POINTER(C.c_double))]


class LinesearchSettings(C.Structure):
    _fields_ = [("g_max", C.c_double), ("g_min", C.c_double), ("gamma_c", C.c_double), ("armijo_factor", C.c_double),
                ("alpha_decay", C.c_double), ("alpha_min", C.c_double), ("delta_tol", C.c_double), ("cost_tol", C.c_double)]


class TermWeights(C.Structure):
    _fields_ = [("foot_sqrt_w", C.c_double * 18)] + [(k, C.c_double) for k in ("gain_pos_z", "gain_ori", "gain_linvel_z", "gain_linvel_xy", "gain_angvel", "gain_linacc_z",
                                                                               "gain_linacc_xy", "gain_angacc")] + \
               [(k, Barrier) for k in ("friction_barrier", "moment_barrier", "joint_limit_barrier", "collision_barrier")] + \
               [("torso_sqrt_w", C.c_double * 12), ("cent_foot_sqrt_w", C.c_double * 12), ("ext_torque_sqrt_w", (C.c_double * 6) * 2)]


class RolloutSettings(C.Structure):   # include/hsqp_rollout.h: hsqp_rollout_settings
    _fields_ = [("integrator", C.c_int32), ("controller", C.c_int32), ("abs_tol", C.c_double), ("rel_tol", C.c_double), ("initial_step", C.c_double),
                ("max_steps_per_second", C.c_double)]


class LoopSettings(C.Structure):   # include/hsqp_loop.h: hsqp_loop_settings
    _fields_ = [("period", C.c_double), ("filter_alpha", C.c_double), ("n_nodes", C.c_int32), ("iterations", C.c_int32), ("dt", C.c_double),
                ("iterate_flags", C.c_int32), ("arm_swing", C.c_int32), ("rollout", RolloutSettings), ("swing", SwingConfig),
                ("terrain_height", C.c_double)]


CMD_N, CMD_KNOTS = 4, 3   # HSQP_CMD_N, HSQP_CMD_KNOTS
# entry points of include/hsqp_loop.h (tests/test_loop.py checks that the library exports each of them and the binding declares it)
LOOP_ENTRY_POINTS = ("hsqp_set_default_joint_state", "hsqp_command_targets", "hsqp_command_targets_device", "hsqp_loop_defaults", "hsqp_loop_start",
                     "hsqp_loop_command", "hsqp_loop_command_device", "hsqp_loop_run", "hsqp_loop_run_device", "hsqp_loop_state", "hsqp_loop_state_device")
# entry points of include/hsqp_cent_loop.h (tests/test_cent_loop.py)
CENT_LOOP_ENTRY_POINTS = ("hsqp_centroidal_command_targets", "hsqp_centroidal_command_targets_device", "hsqp_loop_start_centroidal")

# include/hsqp_gait.h
GAIT_MAX_RUNGS, GAIT_MAX_PHASES, GAIT_MAX_EVENTS, GAIT_NAME_LEN = 16, 6, 256, 16
GAIT_OK, GAIT_OVERFLOW, GAIT_BAD_TILING = 0, 1, 2


class GaitRung(C.Structure):   # hsqp_gait_rung
    _fields_ = [("min_lin_vel_cmd", C.c_double), ("max_lin_vel_cmd", C.c_double), ("min_ang_vel_cmd", C.c_double), ("max_ang_vel_cmd", C.c_double),
                ("lin_vel_error_thresh", C.c_double), ("ang_vel_error_thresh", C.c_double), ("n_phases", C.c_int32), ("reserved", C.c_int32),
                ("switching_times", C.c_double * (GAIT_MAX_PHASES + 1)), ("modes", C.c_int32 * GAIT_MAX_PHASES), ("name", C.c_char * GAIT_NAME_LEN)]


class GaitSettings(C.Structure):   # hsqp_gait_settings
    _fields_ = [("n_rungs", C.c_int32), ("max_events", C.c_int32), ("phase_transition_stance_time", C.c_double), ("min_change_interval", C.c_double),
                ("rungs", GaitRung * GAIT_MAX_RUNGS)]


# entry points of include/hsqp_gait.h (tests/test_gait.py checks that the library exports each of them and the binding declares it)
GAIT_ENTRY_POINTS = ("hsqp_gait_ladder_defaults", "hsqp_gait_reset", "hsqp_gait_update", "hsqp_gait_update_device", "hsqp_gait_state", "hsqp_gait_state_device",
                     "hsqp_loop_start_gait")

# include/hsqp_episode.h
EPISODE_PARK, EPISODE_RESET = 0, 1
EP_ALIVE, EP_FAILED_NUMERIC, EP_FAILED_ROLLOUT, EP_FAILED_BOUNDS = 0, 1, 2, 3


class EpisodeSettings(C.Structure):   # hsqp_episode_settings
    _fields_ = [("on_failure", C.c_int32), ("reserved", C.c_int32), ("min_base_height", C.c_double), ("max_base_height", C.c_double), ("max_tilt", C.c_double)]


# entry points of include/hsqp_episode.h (tests/test_episode.py checks that the library exports each of them and the binding declares it)
EPISODE_ENTRY_POINTS = ("hsqp_episode_defaults", "hsqp_loop_isolate", "hsqp_loop_reset_instances", "hsqp_loop_episodes", "hsqp_loop_episodes_device")

# include/hsqp_metrics.h
METRICS_CURRENT, METRICS_PREVIOUS = 0, 1
METRICS_END_OPEN, METRICS_END_HOST = -1, 0


class Metrics(C.Structure):   # hsqp_metrics: 8-byte fields only
    _fields_ = [(k, C.c_int64) for k in ("cycles", "first_cycle", "end_cause", "torque_samples", "ground_samples", "flight_samples")] + \
               [("touchdowns", C.c_int64 * 2)] + [(k, C.c_int64) for k in ("saturated_samples", "saturated_joint_samples", "rollout_steps", "rollout_rejected")] + \
               [("duration", C.c_double), ("start_xy", C.c_double * 2), ("end_xy", C.c_double * 2)] + \
               [(k, C.c_double) for k in ("path_length", "vel_err_sq", "vel_err_max", "yaw_rate_err_sq", "height_err_sq", "height_min", "height_max", "tilt_max",
                                          "tau_sq", "tau_ratio_max", "work_pos", "work_abs", "load_sum", "load_max", "penetration_max", "cost_sum",
                                          "dynamics_sse_max", "equality_sse_max")]


# entry points of include/hsqp_metrics.h (tests/test_metrics.py checks that the library exports each of them and the binding declares it)
METRICS_ENTRY_POINTS = ("hsqp_loop_metrics_enable", "hsqp_loop_metrics_disable", "hsqp_loop_metrics_restart", "hsqp_loop_metrics", "hsqp_loop_metrics_device")

# include/hsqp_push.h
PUSH_MAX = 8


class Push(C.Structure):   # hsqp_push
    _fields_ = [("body", C.c_int32), ("reserved", C.c_int32), ("t_start", C.c_double), ("duration", C.c_double), ("point", C.c_double * 3),
                ("force", C.c_double * 3)]


# entry points of include/hsqp_push.h (tests/test_push.py checks that the library exports each of them and the binding declares it)
PUSH_ENTRY_POINTS = ("hsqp_push_set", "hsqp_push_set_device", "hsqp_push_clear", "hsqp_push_get")

# include/hsqp_plant.h
PLANT_FLOW, PLANT_TORQUE = 0, 1


class PlantSettings(C.Structure):   # hsqp_plant_settings
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_int32), ("lookahead", C.c_double), ("kp", C.c_double * NJ), ("kd", C.c_double * NJ),
                ("armature", C.c_double * NJ)]


# entry points of include/hsqp_plant.h (tests/test_plant.py checks that the library exports each of them and the binding declares it)
PLANT_ENTRY_POINTS = ("hsqp_plant_defaults", "hsqp_plant_set", "hsqp_plant_clear", "hsqp_plant_get")

# include/hsqp_contact.h
CONTACT_FEET, CONTACT_CORNERS = 2, 4


class ContactSettings(C.Structure):   # hsqp_contact_settings
    _fields_ = [("enabled", C.c_int32), ("reserved", C.c_int32), ("stiffness", C.c_double), ("damping", C.c_double), ("mu", C.c_double),
                ("slip_velocity", C.c_double), ("ground_height", C.c_double)]


class ContactGround(C.Structure):   # hsqp_contact_ground
    _fields_ = [("height", C.c_double), ("mu", C.c_double)]


# entry points of include/hsqp_contact.h (tests/test_contact.py checks that the library exports each of them and the binding declares it)
CONTACT_ENTRY_POINTS = ("hsqp_contact_defaults", "hsqp_contact_set", "hsqp_contact_set_instances", "hsqp_contact_set_instances_device", "hsqp_contact_clear",
                        "hsqp_contact_get", "hsqp_contact_eval", "hsqp_contact_eval_device")


# include/hsqp_actuator.h
class ActuatorSettings(C.Structure):   # hsqp_actuator_settings
    _fields_ = [("enabled", C.c_int32), ("reserved", C.c_int32), ("command_period", C.c_double), ("effort_limit", C.c_double * NJ),
                ("damping", C.c_double * NJ), ("friction", C.c_double * NJ), ("friction_velocity", C.c_double)]


# entry points of include/hsqp_actuator.h (tests/test_actuator.py checks that the library exports each of them and the binding declares it)
ACTUATOR_ENTRY_POINTS = ("hsqp_actuator_defaults", "hsqp_actuator_set", "hsqp_actuator_clear", "hsqp_actuator_get", "hsqp_actuator_last",
                         "hsqp_actuator_last_device")


# include/hsqp_inertia.h
INERTIA_PAYLOADS = 2


class InertiaPayload(C.Structure):   # hsqp_inertia_payload
    _fields_ = [("body", C.c_int32), ("reserved", C.c_int32), ("mass", C.c_double), ("com", C.c_double * 3), ("inertia", C.c_double * 6)]


class InertiaInstance(C.Structure):   # hsqp_inertia_instance
    _fields_ = [("mass_scale", C.c_double * NB), ("n_payloads", C.c_int32), ("reserved", C.c_int32), ("payload", InertiaPayload * INERTIA_PAYLOADS)]


# entry points of include/hsqp_inertia.h (tests/test_inertia.py checks that the library exports each of them and the binding declares it)
INERTIA_ENTRY_POINTS = ("hsqp_inertia_defaults", "hsqp_inertia_set_instances", "hsqp_inertia_set_instances_device", "hsqp_inertia_clear",
                        "hsqp_inertia_get_instances", "hsqp_inertia_eval", "hsqp_inertia_eval_device")


# include/hsqp_terrain.h
TERRAIN_MAX_MAPS, TERRAIN_MAX_DIM = 16, 256


class TerrainPlacement(C.Structure):   # hsqp_terrain_placement
    _fields_ = [("map", C.c_int32), ("reserved", C.c_int32), ("origin_x", C.c_double), ("origin_y", C.c_double), ("yaw", C.c_double)]


# entry points of include/hsqp_terrain.h (tests/test_terrain.py checks that the library exports each of them and the binding declares it)
TERRAIN_ENTRY_POINTS = ("hsqp_terrain_set_maps", "hsqp_terrain_set_instances", "hsqp_terrain_set_instances_device", "hsqp_terrain_clear",
                        "hsqp_terrain_get_maps", "hsqp_terrain_get_instances", "hsqp_terrain_eval", "hsqp_terrain_eval_device")


# include/hsqp_observe.h
OBS_MAX_DELAY = 8


class ObserveSettings(C.Structure):   # hsqp_observe_settings
    _fields_ = [("sensor_delay", C.c_int32), ("compute_delay", C.c_int32), ("seed", C.c_uint64)]


class ObserveInstance(C.Structure):   # hsqp_observe_instance
    _fields_ = [("bias", C.c_double * NX), ("sigma", C.c_double * NX)]


# entry points of include/hsqp_observe.h (tests/test_observe.py checks that the library exports each of them and the binding declares it)
OBSERVE_ENTRY_POINTS = ("hsqp_observe_defaults", "hsqp_observe_instance_defaults", "hsqp_observe_set", "hsqp_observe_set_instances",
                        "hsqp_observe_set_instances_device", "hsqp_observe_clear", "hsqp_observe_get", "hsqp_observe_eval", "hsqp_observe_eval_device",
                        "hsqp_observe_last", "hsqp_observe_last_device")

# include/hsqp_grid.h
GRID_OK, GRID_OVERFLOW = 0, 1


class GridSettings(C.Structure):   # hsqp_grid_settings
    _fields_ = [("event_nodes", C.c_int32), ("reserved", C.c_int32), ("dt_min", C.c_double)]


# entry points of include/hsqp_grid.h (tests/test_grid.py checks that the library exports each of them and the binding declares it)
GRID_ENTRY_POINTS = ("hsqp_grid_defaults", "hsqp_event_grid", "hsqp_event_grid_device", "hsqp_loop_event_grid", "hsqp_loop_grid", "hsqp_loop_grid_device")


# include/hsqp_ground.h
class GroundSettings(C.Structure):   # hsqp_ground_settings
    _fields_ = [("enabled", C.c_int32), ("box_above_ground", C.c_int32), ("filter_alpha", C.c_double), ("initial_height", C.c_double)]


# entry points of include/hsqp_ground.h (tests/test_ground.py checks that the library exports each of them and the binding declares it)
GROUND_ENTRY_POINTS = ("hsqp_ground_defaults", "hsqp_ground_estimate", "hsqp_ground_estimate_device", "hsqp_upload_reference_ground", "hsqp_loop_ground",
                       "hsqp_loop_ground_state", "hsqp_loop_ground_state_device")


# include/hsqp_perceive.h
class PerceiveSettings(C.Structure):   # hsqp_perceive_settings
    _fields_ = [("enabled", C.c_int32), ("reserved", C.c_int32)]


# entry points of include/hsqp_perceive.h (tests/test_perceive.py checks that the library exports each of them and the binding declares it)
PERCEIVE_ENTRY_POINTS = ("hsqp_perceive_defaults", "hsqp_upload_reference_heights", "hsqp_foot_heights", "hsqp_foot_heights_device", "hsqp_loop_perceive",
                         "hsqp_loop_foot_heights", "hsqp_loop_foot_heights_device")

ROLLOUT_ODE45, ROLLOUT_RK4 = 0, 1
ROLLOUT_FEEDFORWARD, ROLLOUT_FEEDBACK = 0, 1
ROLLOUT_OK, ROLLOUT_MAX_STEPS, ROLLOUT_NONFINITE = 0, 1, 2

STEP_COST, STEP_DUAL, STEP_CONSTRAINT, STEP_ZERO, STEP_FULL = 0, 1, 2, 3, 4
FLAG_LINESEARCH = 1
FLAG_SERIAL_RICCATI, FLAG_PARALLEL_RICCATI, SCAN_AUTO_BATCH, SCAN_AUTO_MIN_NODES = 2, 4, 2, 48
FLAG_SEGMENTED_RICCATI = 8   # the two-level (segmented) sweep (csrc/hsqp_segment.h): opt-in, declared relaxation of the trajectory tolerance
BLK_PARAMS = 11
