"""Host-side mirror of the reference's solver interface over the HIP C ABI.

The reference drives its solver through ocs2::SolverBase / MPC_BASE
(humanoid_nmpc/humanoid_wb_mpc_ros2/src/WBMpcSqpNode.cpp:64-89,
 humanoid_nmpc/humanoid_wb_mpc/src/mrt/WBMpcMrtJointController.cpp:200-213):
reset(), run(t0, x0, tf), getPrimalSolution(), getPerformanceIndeces(), and the fork's
SqpSolver::getBenchmarks() (humanoid_common_mpc_ros2/src/benchmarks/SqpBenchmarksPublisher.cpp:44-57).
HipSqpSolver keeps those names and meanings for a batch of independent MPC instances; the C++
adaptor of INTEGRATION.md is the same thin layer in the reference's own language.

There is no CPU path: constructing a solver without the built HIP library or without a GPU raises.
"""
import ctypes as C
import os

import numpy as np

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HSQP_LIB") or os.path.join(_HERE, "libhsqp_hip.so")   # HSQP_LIB: debug builds only
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_lib = None


class HsqpError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"hsqp error {code}: {msg}")
        self.code = code


def load_library():
    """Load libhsqp_hip.so (built in-tree by wb_humanoid_mpc_amd.build / __graft_entry__.build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: build it with `python -m wb_humanoid_mpc_amd.build` "
                           "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    lib.hsqp_create.argtypes = [C.POINTER(_abi.ModelDesc), C.POINTER(_abi.Settings), C.POINTER(C.c_void_p)]
    lib.hsqp_destroy.argtypes = [C.c_void_p]
    lib.hsqp_solve.argtypes = [C.c_void_p, C.POINTER(_abi.Problem), C.POINTER(_abi.Solution)]
    lib.hsqp_upload.argtypes = [C.c_void_p, C.POINTER(_abi.Problem)]
    lib.hsqp_upload_reference.argtypes = [C.c_void_p, C.POINTER(_abi.Problem), C.POINTER(_abi.Reference)]
    lib.hsqp_iterate_device.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.hsqp_last_iterations.argtypes = [C.c_void_p]
    lib.hsqp_iteration_log.argtypes = [C.c_void_p, C.c_int, C.POINTER(_abi.Perf), _dp, C.POINTER(C.c_int32)]
    lib.hsqp_update_weights.argtypes = [C.c_void_p, _dp, _dp, _dp]
    lib.hsqp_host_register.argtypes = [C.c_void_p, C.c_size_t]
    lib.hsqp_host_unregister.argtypes = [C.c_void_p]
    lib.hsqp_download.argtypes = [C.c_void_p, C.POINTER(_abi.Solution)]
    lib.hsqp_upload_device.argtypes = [C.c_void_p, C.POINTER(_abi.Problem)]
    lib.hsqp_download_device.argtypes = [C.c_void_p, C.POINTER(_abi.Solution)]
    lib.hsqp_debug_read.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_longlong]
    lib.hsqp_debug_read.restype = C.c_longlong
    lib.hsqp_last_kernel_ms.argtypes = [C.c_void_p, _dp]
    lib.hsqp_last_error.argtypes = [C.c_void_p]
    lib.hsqp_last_error.restype = C.c_char_p
    lib.hsqp_scan_fallbacks.argtypes = [C.c_void_p]
    lib.hsqp_scan_fallbacks.restype = C.c_longlong
    lib.hsqp_get_term_weights.argtypes = [C.c_void_p, C.c_void_p]
    lib.hsqp_update_term_weights.argtypes = [C.c_void_p, C.c_void_p]
    lib.hsqp_scan_backoffs.argtypes = [C.c_void_p]
    lib.hsqp_scan_backoffs.restype = C.c_longlong
    lib.hsqp_version.restype = C.c_char_p
    lib.hsqp_set_scan_backoff_persistent.argtypes = [C.c_void_p, C.c_int]
    # hsqp_comm_*: the batch axis over the GPUs of one node behind the C ABI (the Python host uses torch.distributed instead: distributed.py)
    lib.hsqp_comm_unique_id.argtypes = [C.c_void_p]
    lib.hsqp_comm_create.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_int, C.c_int, C.c_int]
    lib.hsqp_comm_destroy.argtypes = [C.c_void_p]
    lib.hsqp_comm_destroy.restype = None
    lib.hsqp_comm_create_error.restype = C.c_char_p
    lib.hsqp_comm_last_error.argtypes = [C.c_void_p]
    lib.hsqp_comm_last_error.restype = C.c_char_p
    lib.hsqp_comm_rank.argtypes = [C.c_void_p]
    lib.hsqp_comm_world.argtypes = [C.c_void_p]
    lib.hsqp_comm_shard.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.hsqp_comm_shard_of.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.hsqp_comm_broadcast.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int]
    lib.hsqp_comm_scatter_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_int]
    lib.hsqp_comm_gather_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_int]
    lib.hsqp_comm_max.argtypes = [C.c_void_p, _dp, C.c_int]
    lib.hsqp_comm_barrier.argtypes = [C.c_void_p]
    if lib.hsqp_abi_version() != _abi.ABI_VERSION:
        raise RuntimeError(f"libhsqp_hip ABI {lib.hsqp_abi_version()} != the binding's {_abi.ABI_VERSION} (include/hsqp.h: HSQP_ABI_VERSION)")
    lib.hsqp_joint_torques.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp]
    lib.hsqp_evaluate_policy.argtypes = [C.c_void_p, _dp, _dp, _dp, _dp]
    # include/hsqp_feedback.h
    lib.hsqp_feedback_policy.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp, _dp]
    lib.hsqp_feedback_policy_device.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp, _dp]
    lib.hsqp_evaluate_feedback_policy.argtypes = [C.c_void_p, _dp, _dp, _dp, _dp, _dp]
    # include/hsqp_value.h
    lib.hsqp_value_function.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _dp]
    lib.hsqp_value_function_device.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _dp]
    lib.hsqp_evaluate_value_function.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp, _dp, _dp]
    lib.hsqp_evaluate_value_function_device.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp, _dp, _dp]
    # include/hsqp_rollout.h
    _ip = C.POINTER(C.c_int32)
    lib.hsqp_rollout_defaults.argtypes = [C.POINTER(_abi.RolloutSettings)]
    lib.hsqp_rollout_defaults.restype = None
    lib.hsqp_rollout_policy.argtypes = [C.c_void_p, C.POINTER(_abi.RolloutSettings), _dp, _dp, C.c_double, C.c_int, _dp, _dp, _ip, _ip, _ip]
    lib.hsqp_rollout_policy_device.argtypes = [C.c_void_p, C.POINTER(_abi.RolloutSettings), _dp, _dp, C.c_double, C.c_int, _dp, _dp, _ip, _ip, _ip]
    # include/hsqp_push.h
    _pp = C.POINTER(_abi.Push)
    lib.hsqp_push_set.argtypes = [C.c_void_p, C.c_int, C.c_int, _ip, _pp]
    lib.hsqp_push_set_device.argtypes = [C.c_void_p, C.c_int, C.c_int, _ip, _pp]
    lib.hsqp_push_clear.argtypes = [C.c_void_p]
    lib.hsqp_push_get.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), _ip, _pp]
    # include/hsqp_plant.h
    _pl = C.POINTER(_abi.PlantSettings)
    lib.hsqp_plant_defaults.argtypes = [_pl]
    lib.hsqp_plant_defaults.restype = None
    lib.hsqp_plant_set.argtypes = [C.c_void_p, _pl]
    lib.hsqp_plant_clear.argtypes = [C.c_void_p]
    lib.hsqp_plant_get.argtypes = [C.c_void_p, _pl]
    # include/hsqp_contact.h
    _cs, _cg = C.POINTER(_abi.ContactSettings), C.POINTER(_abi.ContactGround)
    lib.hsqp_contact_defaults.argtypes = [C.c_void_p, _cs]
    lib.hsqp_contact_defaults.restype = None
    lib.hsqp_contact_set.argtypes = [C.c_void_p, _cs]
    lib.hsqp_contact_set_instances.argtypes = [C.c_void_p, C.c_int, _cg]
    lib.hsqp_contact_set_instances_device.argtypes = [C.c_void_p, C.c_int, _cg]
    lib.hsqp_contact_clear.argtypes = [C.c_void_p]
    lib.hsqp_contact_get.argtypes = [C.c_void_p, _cs]
    lib.hsqp_contact_eval.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp]
    lib.hsqp_contact_eval_device.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp]
    # include/hsqp_actuator.h
    _as = C.POINTER(_abi.ActuatorSettings)
    lib.hsqp_actuator_defaults.argtypes = [_as]
    lib.hsqp_actuator_defaults.restype = None
    lib.hsqp_actuator_set.argtypes = [C.c_void_p, _as]
    lib.hsqp_actuator_clear.argtypes = [C.c_void_p]
    lib.hsqp_actuator_get.argtypes = [C.c_void_p, _as]
    lib.hsqp_actuator_last.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp]
    lib.hsqp_actuator_last_device.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp]
    # include/hsqp_inertia.h
    _ii = C.POINTER(_abi.InertiaInstance)
    lib.hsqp_inertia_defaults.argtypes = [_ii]
    lib.hsqp_inertia_defaults.restype = None
    lib.hsqp_inertia_set_instances.argtypes = [C.c_void_p, C.c_int, _ii]
    lib.hsqp_inertia_set_instances_device.argtypes = [C.c_void_p, C.c_int, _ii]
    lib.hsqp_inertia_clear.argtypes = [C.c_void_p]
    lib.hsqp_inertia_get_instances.argtypes = [C.c_void_p, C.c_int, _ii]
    lib.hsqp_inertia_eval.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp, _dp]
    lib.hsqp_inertia_eval_device.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp, _dp]
    # include/hsqp_terrain.h
    _tp = C.POINTER(_abi.TerrainPlacement)
    lib.hsqp_terrain_set_maps.argtypes = [C.c_void_p, C.c_int, _ip, _ip, _dp, _dp]
    lib.hsqp_terrain_set_instances.argtypes = [C.c_void_p, C.c_int, _tp]
    lib.hsqp_terrain_set_instances_device.argtypes = [C.c_void_p, C.c_int, _tp]
    lib.hsqp_terrain_clear.argtypes = [C.c_void_p]
    lib.hsqp_terrain_get_maps.argtypes = [C.c_void_p, _ip, _ip, _ip, _dp, _dp, C.c_size_t]
    lib.hsqp_terrain_get_instances.argtypes = [C.c_void_p, C.c_int, _tp]
    lib.hsqp_terrain_eval.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _dp]
    lib.hsqp_terrain_eval_device.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _dp]
    # include/hsqp_observe.h
    _os, _oi = C.POINTER(_abi.ObserveSettings), C.POINTER(_abi.ObserveInstance)
    lib.hsqp_observe_defaults.argtypes = [_os]
    lib.hsqp_observe_defaults.restype = None
    lib.hsqp_observe_instance_defaults.argtypes = [_oi]
    lib.hsqp_observe_instance_defaults.restype = None
    lib.hsqp_observe_set.argtypes = [C.c_void_p, _os]
    lib.hsqp_observe_set_instances.argtypes = [C.c_void_p, C.c_int, _oi]
    lib.hsqp_observe_set_instances_device.argtypes = [C.c_void_p, C.c_int, _oi]
    lib.hsqp_observe_clear.argtypes = [C.c_void_p]
    lib.hsqp_observe_get.argtypes = [C.c_void_p, _os, C.c_int, _oi]
    lib.hsqp_observe_eval.argtypes = [C.c_void_p, C.c_int, C.c_uint32, _dp, _dp]
    lib.hsqp_observe_eval_device.argtypes = [C.c_void_p, C.c_int, C.c_uint32, _dp, _dp]
    lib.hsqp_observe_last.argtypes = [C.c_void_p, _dp, _dp]
    lib.hsqp_observe_last_device.argtypes = [C.c_void_p, _dp, _dp]
    # include/hsqp_loop.h
    _ls = C.POINTER(_abi.LoopSettings)
    lib.hsqp_set_default_joint_state.argtypes = [C.c_void_p, _dp]
    lib.hsqp_command_targets.argtypes = [C.c_void_p, C.c_int, _dp, _dp, C.c_double, _dp, C.c_double, C.c_double, _dp, _dp]
    lib.hsqp_command_targets_device.argtypes = [C.c_void_p, C.c_int, _dp, _dp, C.c_double, _dp, C.c_double, C.c_double, _dp, _dp]
    lib.hsqp_loop_defaults.argtypes = [C.c_void_p, _ls]
    # include/hsqp_cent_loop.h
    lib.hsqp_centroidal_command_targets.argtypes = [C.c_void_p, C.c_int, _dp, _dp, C.c_double, _dp, C.c_double, C.c_double, _dp, _dp, _dp]
    lib.hsqp_centroidal_command_targets_device.argtypes = [C.c_void_p, C.c_int, _dp, _dp, C.c_double, _dp, C.c_double, C.c_double, _dp, _dp, _dp]
    lib.hsqp_loop_start_centroidal.argtypes = [C.c_void_p, _ls, C.c_int, C.c_double, _dp, _dp, C.c_int, _ip, _dp, _ip]
    lib.hsqp_loop_defaults.restype = None
    lib.hsqp_loop_start.argtypes = [C.c_void_p, _ls, C.c_int, C.c_double, _dp, _dp, C.c_int, _ip, _dp, _ip]
    lib.hsqp_loop_command.argtypes = [C.c_void_p, _dp]
    lib.hsqp_loop_command_device.argtypes = [C.c_void_p, _dp]
    lib.hsqp_loop_run.argtypes = [C.c_void_p, C.c_int, _dp, _dp, C.POINTER(C.c_int)]
    lib.hsqp_loop_run_device.argtypes = [C.c_void_p, C.c_int, _dp, _dp, C.POINTER(C.c_int)]
    lib.hsqp_loop_state.argtypes = [C.c_void_p, _dp, _dp, _dp]
    lib.hsqp_loop_state_device.argtypes = [C.c_void_p, _dp, _dp, _dp]
    # include/hsqp_gait.h
    _gs = C.POINTER(_abi.GaitSettings)
    lib.hsqp_gait_ladder_defaults.argtypes = [_gs]
    lib.hsqp_gait_ladder_defaults.restype = None
    lib.hsqp_gait_reset.argtypes = [C.c_void_p, _gs, C.c_int, C.c_double]
    lib.hsqp_gait_update.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_double, _dp, _dp, _ip, _dp, _ip]
    lib.hsqp_gait_update_device.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_double, _dp, _dp, _ip, _dp, _ip]
    lib.hsqp_gait_state.argtypes = [C.c_void_p, _ip, _dp, _ip, _dp, _ip]
    lib.hsqp_gait_state_device.argtypes = [C.c_void_p, _ip, _dp, _ip, _dp, _ip]
    lib.hsqp_loop_start_gait.argtypes = [C.c_void_p, _ls, _gs, C.c_int, C.c_double, _dp, _dp]
    _es = C.POINTER(_abi.EpisodeSettings)
    lib.hsqp_episode_defaults.argtypes = [_es]
    lib.hsqp_episode_defaults.restype = None
    lib.hsqp_loop_isolate.argtypes = [C.c_void_p, _es, _dp]
    lib.hsqp_loop_reset_instances.argtypes = [C.c_void_p, C.c_int, _ip, _dp, _dp]
    lib.hsqp_loop_episodes.argtypes = [C.c_void_p, _ip, _ip, _ip, _ip, _ip]
    lib.hsqp_loop_episodes_device.argtypes = [C.c_void_p, _ip, _ip, _ip, _ip, _ip]
    _mp = C.POINTER(_abi.Metrics)
    lib.hsqp_loop_metrics_enable.argtypes = [C.c_void_p]
    lib.hsqp_loop_metrics_disable.argtypes = [C.c_void_p]
    lib.hsqp_loop_metrics_restart.argtypes = [C.c_void_p, C.c_int, _ip]
    lib.hsqp_loop_metrics.argtypes = [C.c_void_p, C.c_int, _mp]
    lib.hsqp_loop_metrics_device.argtypes = [C.c_void_p, C.c_int, _mp]
    # include/hsqp_grid.h
    _gr = C.POINTER(_abi.GridSettings)
    lib.hsqp_grid_defaults.argtypes = [_gr]
    lib.hsqp_grid_defaults.restype = None
    lib.hsqp_event_grid.argtypes = [C.c_void_p, _gr, C.c_int, C.c_double, C.c_int, C.c_double, C.c_int, _ip, _dp, _ip, _dp, _dp, _ip]
    lib.hsqp_event_grid_device.argtypes = [C.c_void_p, _gr, C.c_int, C.c_double, C.c_int, C.c_double, C.c_int, _ip, _dp, _ip, _dp, _dp, _ip]
    lib.hsqp_loop_event_grid.argtypes = [C.c_void_p, _gr]
    lib.hsqp_loop_grid.argtypes = [C.c_void_p, _ip, _dp, _dp]
    lib.hsqp_loop_grid_device.argtypes = [C.c_void_p, _ip, _dp, _dp]
    # include/hsqp_ground.h
    _gs = C.POINTER(_abi.GroundSettings)
    lib.hsqp_ground_defaults.argtypes = [_gs]
    lib.hsqp_ground_defaults.restype = None
    lib.hsqp_ground_estimate.argtypes = [C.c_void_p, C.c_int, C.c_double, _dp, C.c_int, _ip, _dp, _ip, C.c_double, _dp, _dp]
    lib.hsqp_ground_estimate_device.argtypes = [C.c_void_p, C.c_int, C.c_double, _dp, C.c_int, _ip, _dp, _ip, C.c_double, _dp, _dp]
    lib.hsqp_upload_reference_ground.argtypes = [C.c_void_p, C.POINTER(_abi.Problem), C.POINTER(_abi.Reference), _dp]
    lib.hsqp_loop_ground.argtypes = [C.c_void_p, _gs, _dp]
    lib.hsqp_loop_ground_state.argtypes = [C.c_void_p, _dp, _dp]
    lib.hsqp_loop_ground_state_device.argtypes = [C.c_void_p, _dp, _dp]
    # include/hsqp_perceive.h
    _ps = C.POINTER(_abi.PerceiveSettings)
    lib.hsqp_perceive_defaults.argtypes = [_ps]
    lib.hsqp_perceive_defaults.restype = None
    lib.hsqp_upload_reference_heights.argtypes = [C.c_void_p, C.POINTER(_abi.Problem), C.POINTER(_abi.Reference), _dp, _dp]
    lib.hsqp_foot_heights.argtypes = [C.c_void_p, C.c_int, C.c_double, _dp, C.c_int, _ip, _dp, _ip, C.c_int, _dp, _dp, C.c_double, _dp, _dp, _dp]
    lib.hsqp_foot_heights_device.argtypes = [C.c_void_p, C.c_int, C.c_double, _dp, C.c_int, _ip, _dp, _ip, C.c_int, _dp, _dp, C.c_double, _dp, _dp, _dp]
    lib.hsqp_loop_perceive.argtypes = [C.c_void_p, _ps]
    lib.hsqp_loop_foot_heights.argtypes = [C.c_void_p, _dp, _dp, _dp]
    lib.hsqp_loop_foot_heights_device.argtypes = [C.c_void_p, _dp, _dp, _dp]
    lib.hsqp_linesearch_defaults.argtypes = [C.POINTER(_abi.LinesearchSettings)]
    lib.hsqp_linesearch_defaults.restype = None
    lib.hsqp_set_linesearch.argtypes = [C.c_void_p, C.POINTER(_abi.LinesearchSettings)]
    _lib = lib
    return lib


def _c(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def metrics_dict(rec):
    """A ctypes array of hsqp_metrics ([B]) as a dict of numpy arrays, one per field."""
    raw = np.frombuffer(bytes(rec), dtype=np.uint8).reshape(len(rec), C.sizeof(_abi.Metrics))
    out = {}
    for name, _ in _abi.Metrics._fields_:
        f = getattr(_abi.Metrics, name)   # (the counts come first: every field in front of `duration` is int64)
        words = np.ascontiguousarray(raw[:, f.offset:f.offset + f.size]).view(np.int64 if f.offset < _abi.Metrics.duration.offset else np.float64)
        out[name] = words[:, 0].copy() if words.shape[1] == 1 else words.copy()
    return out


def metrics_summary(records, mass, gravity=9.81):
    """What a batch of records (loop_metrics()) says as a whole: survivors (records still open with samples), RMS velocity tracking error over
    all samples, mean straight-line distance, and the cost of transport work_pos / (m g |end - start|) over the instances that have torque
    samples and moved (None: none did)."""
    cycles = records["cycles"]
    have = cycles > 0
    dist = np.linalg.norm(records["end_xy"] - records["start_xy"], axis=1)
    n = int(cycles.sum())
    moved = have & (records["torque_samples"] > 0) & (dist > 0.0)
    return dict(instances=int(cycles.shape[0]), survivors=int((have & (records["end_cause"] == _abi.METRICS_END_OPEN)).sum()), samples=n,
                rms_tracking=float(np.sqrt(records["vel_err_sq"].sum() / n)) if n else None,
                distance=float(dist[have].mean()) if have.any() else None,
                cost_of_transport=float(records["work_pos"][moved].sum() / (mass * abs(gravity) * dist[moved].sum())) if moved.any() else None)


class HipSqpSolver:
    def __init__(self, model, max_nodes, max_batch=1, device=0, linesearch=False, riccati="auto"):
        """linesearch=True: run() uses the filter line search (ocs2 SqpSolver behaviour) instead of the full step.
        riccati: "auto" (serial recursion; KKT-gated parallel-in-time scan for <= 2 instances on >= 48 nodes), "serial", "parallel" (the scan
        for every size), "segmented" (the KKT-gated two-level sweep of hsqp_segment.h for mid-sized batches: faster, but a declared
        relaxation — its step is up to 4e-10 of the step's scale from the serial recursion's)."""
        self.lib = load_library()
        self.model = model
        flags = (_abi.FLAG_LINESEARCH if linesearch else 0) | {"auto": 0, "serial": _abi.FLAG_SERIAL_RICCATI, "parallel": _abi.FLAG_PARALLEL_RICCATI, "segmented": _abi.FLAG_SEGMENTED_RICCATI}[riccati]
        st = _abi.Settings(max_nodes=max_nodes, max_batch=max_batch, device=device, flags=flags)
        h = C.c_void_p()
        rc = self.lib.hsqp_create(C.byref(model.desc), C.byref(st), C.byref(h))
        if rc != 0:
            raise HsqpError(rc, self.lib.hsqp_last_error(None).decode())
        self.h = h
        self.max_nodes, self.max_batch = max_nodes, max_batch
        self._shape = None
        self._sol = None
        self._loop_batch = 0
        self._loop_nodes = self._grid_nodes = 0
        # the velocity-command generators' joint targets (reference.info defaultJointState) are not part of hsqp_model_desc
        self._check(self.lib.hsqp_set_default_joint_state(h, _c(model.default_joint_state).ctypes.data_as(_dp)))

    def close(self):
        if getattr(self, "h", None):
            self.lib.hsqp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise HsqpError(rc, self.lib.hsqp_last_error(self.h).decode())

    # ---- SolverBase::reset
    def reset(self):
        self._shape = None
        self._sol = None

    def _problem(self, x_init, x_traj, u_traj, params, dt):
        x_traj, u_traj, params, x_init = _c(x_traj), _c(u_traj), _c(params), _c(x_init)
        if x_traj.ndim == 2:
            x_traj, u_traj, params, x_init = x_traj[None], u_traj[None], params[None], x_init[None]
        B, N = u_traj.shape[0], u_traj.shape[1]
        if x_traj.shape != (B, N + 1, _abi.NX) or u_traj.shape != (B, N, _abi.NU) or \
                params.shape != (B, N + 1, _abi.NODE_PARAMS) or x_init.shape != (B, _abi.NX):
            raise ValueError("inconsistent problem array shapes")
        dt, grid = self._grid(dt, B, N)
        keep = (x_init, x_traj, u_traj, params, grid)
        p = _abi.Problem(batch=B, n_nodes=N, dt=dt, x_init=x_init.ctypes.data_as(_dp), x_traj=x_traj.ctypes.data_as(_dp),
                         u_traj=u_traj.ctypes.data_as(_dp), node_params=params.ctypes.data_as(_dp),
                         dt_nodes=None if grid is None else grid.ctypes.data_as(_dp))
        return p, keep, (B, N)

    @staticmethod
    def _grid(dt, B, N):
        """dt: the uniform node spacing, or the interval lengths of a non-uniform grid ([N] shared by all instances or [B][N];
        a zero marks an event interval, hsqp_problem::dt_nodes)."""
        if np.ndim(dt) == 0:
            return float(dt), None
        grid = np.ascontiguousarray(np.broadcast_to(np.asarray(dt, dtype=np.float64), (B, N)))
        return 0.0, grid

    def _alloc_solution(self, B, N):
        out = dict(x=np.zeros((B, N + 1, _abi.NX)), u=np.zeros((B, N, _abi.NU)), dx=np.zeros((B, N + 1, _abi.NX)),
                   du=np.zeros((B, N, _abi.NU)), kkt=np.zeros((B, 2)), alpha=np.zeros(B), step_type=np.zeros(B, dtype=np.int32),
                   armijo=np.zeros(B), grad_inf=np.zeros(B))
        pb, pa = (_abi.Perf * B)(), (_abi.Perf * B)()
        s = _abi.Solution(x=out["x"].ctypes.data_as(_dp), u=out["u"].ctypes.data_as(_dp), dx=out["dx"].ctypes.data_as(_dp),
                          du=out["du"].ctypes.data_as(_dp), perf_before=pb, perf_after=pa, kkt=out["kkt"].ctypes.data_as(_dp),
                          alpha=out["alpha"].ctypes.data_as(_dp), step_type=out["step_type"].ctypes.data_as(C.POINTER(C.c_int32)),
                          armijo=out["armijo"].ctypes.data_as(_dp), grad_inf=out["grad_inf"].ctypes.data_as(_dp))
        return s, out, pb, pa

    @staticmethod
    def _perf(arr):
        return [dict(merit=p.merit, cost=p.cost, dynamics_sse=p.dynamics_sse, equality_sse=p.equality_sse) for p in arr]

    def _finish(self, s, out, pb, pa):
        out["perf_before"], out["perf_after"] = self._perf(pb), self._perf(pa)
        t = s.timings
        out["benchmarks"] = dict(linearQuadraticApproximationTime=t.lq_approximation, solveQpTime=t.solve_qp,
                                 linesearchTime=t.linesearch, computeControllerTime=t.compute_controller, total=t.total)
        self._sol = out
        return out

    # ---- SolverBase::run (one SQP iteration, sqpIteration = 1 as in task.info:81)
    def pin(self, *arrays):
        """hsqp_host_register on caller-owned numpy arrays (page-locked: one DMA per transfer); unpin() before they are freed."""
        for a in arrays:
            self._check(self.lib.hsqp_host_register(a.ctypes.data_as(C.c_void_p), a.nbytes))

    def unpin(self, *arrays):
        for a in arrays:
            self._check(self.lib.hsqp_host_unregister(a.ctypes.data_as(C.c_void_p)))

    def alloc_solution(self, B, N):
        """Solution buffers for run(..., into=...): allocate (and pin) once, reuse every cycle."""
        return self._alloc_solution(B, N)

    def run(self, x_init, x_traj, u_traj, params, dt, into=None):
        p, keep, (B, N) = self._problem(x_init, x_traj, u_traj, params, dt)
        s, out, pb, pa = into if into is not None else self._alloc_solution(B, N)
        self._check(self.lib.hsqp_solve(self.h, C.byref(p), C.byref(s)))
        self._shape = (B, N)
        return self._finish(s, out, pb, pa)

    # ---- device-resident loop (bench): upload once, iterate, download
    def upload(self, x_init, x_traj, u_traj, params, dt):
        p, keep, self._shape = self._problem(x_init, x_traj, u_traj, params, dt)
        self._check(self.lib.hsqp_upload(self.h, C.byref(p)))

    def upload_reference(self, x_init, x_traj, u_traj, dt, t0, n_events, event_times, mode_sequence, target_times, target_states,
                         swing, terrain_height=0.0, arm_swing=True, node_times=None):
        """hsqp_upload_reference: the per-node parameter table is generated on the device from the compact reference
        (mode schedule + target knots per instance; see reference.pack_reference).  Non-uniform grid: dt = interval lengths
        ([N] or [B][N]) together with node_times ([N+1] or [B][N+1])."""
        x_traj, u_traj, x_init = _c(x_traj), _c(u_traj), _c(x_init)
        if x_traj.ndim == 2:
            x_traj, u_traj, x_init = x_traj[None], u_traj[None], x_init[None]
        B, N = u_traj.shape[0], u_traj.shape[1]
        self._upload_reference(B, N, x_init, x_traj, u_traj, dt, t0, n_events, event_times, mode_sequence, target_times, target_states,
                               swing, terrain_height, arm_swing, node_times, _abi.WARM_CALLER)

    def upload_reference_warm(self, x_init, n_nodes, dt, t0, n_events, event_times, mode_sequence, target_times, target_states,
                              swing, terrain_height=0.0, arm_swing=True, mode="shift", node_times=None):
        """hsqp_upload_reference with the warm start built on the device (hsqp_reference::warm_start): mode="shift" interpolates the
        solution resident in the handle onto the new grid and fills the uncovered tail with the weight-compensating input; mode="cold"
        is that initializer alone (x_k = x_init).  Arguments as upload_reference, without x_traj / u_traj; x_init is [B][58]."""
        x_init = _c(x_init)
        if x_init.ndim == 1:
            x_init = x_init[None]
        warm = {"shift": _abi.WARM_SHIFT, "cold": _abi.WARM_COLD}[mode]
        self._upload_reference(x_init.shape[0], int(n_nodes), x_init, None, None, dt, t0, n_events, event_times, mode_sequence, target_times,
                               target_states, swing, terrain_height, arm_swing, node_times, warm)

    def _upload_reference(self, B, N, x_init, x_traj, u_traj, dt, t0, n_events, event_times, mode_sequence, target_times, target_states,
                          swing, terrain_height, arm_swing, node_times, warm, terrain_heights=None, heights=None):
        n_events = np.ascontiguousarray(n_events, dtype=np.int32)
        mode_sequence = np.ascontiguousarray(mode_sequence, dtype=np.int32)
        event_times, target_times, target_states = _c(event_times), _c(target_times), _c(target_states)
        if event_times.shape[0] != B or mode_sequence.shape != (B, event_times.shape[1] + 1) or target_states.shape != (B, target_times.shape[1], _abi.NX) \
                or x_init.shape != (B, _abi.NX):
            raise ValueError("inconsistent reference array shapes")
        ip = C.POINTER(C.c_int32)
        dt, grid = self._grid(dt, B, N)
        nt = None if node_times is None else np.ascontiguousarray(np.broadcast_to(np.asarray(node_times, dtype=np.float64), (B, N + 1)))
        p = _abi.Problem(batch=B, n_nodes=N, dt=dt, x_init=x_init.ctypes.data_as(_dp), x_traj=None if x_traj is None else x_traj.ctypes.data_as(_dp),
                         u_traj=None if u_traj is None else u_traj.ctypes.data_as(_dp), node_params=None, dt_nodes=None if grid is None else grid.ctypes.data_as(_dp))
        r = _abi.Reference(batch=B, n_nodes=N, t0=t0, dt=dt, node_times=None if nt is None else nt.ctypes.data_as(_dp), max_events=event_times.shape[1], n_events=n_events.ctypes.data_as(ip),
                           event_times=event_times.ctypes.data_as(_dp), mode_sequence=mode_sequence.ctypes.data_as(ip),
                           n_knots=target_times.shape[1], target_times=target_times.ctypes.data_as(_dp),
                           target_states=target_states.ctypes.data_as(_dp), swing=swing, terrain_height=terrain_height,
                           arm_swing=1 if arm_swing else 0, warm_start=warm)
        if heights is not None:   # include/hsqp_perceive.h: one lift-off and one touch-down height per foot and phase
            lift, touch = (_c(a) for a in heights)
            if lift.shape != (B, 2, event_times.shape[1] + 1) or touch.shape != lift.shape:
                raise ValueError("lift_off and touch_down must be [B][2][max_events + 1]")
            self._check(self.lib.hsqp_upload_reference_heights(self.h, C.byref(p), C.byref(r), lift.ctypes.data_as(_dp), touch.ctypes.data_as(_dp)))
        elif terrain_heights is None:
            self._check(self.lib.hsqp_upload_reference(self.h, C.byref(p), C.byref(r)))
        else:   # include/hsqp_ground.h: one terrain height per instance
            th = _c(np.broadcast_to(np.asarray(terrain_heights, dtype=np.float64), (B,)))
            self._check(self.lib.hsqp_upload_reference_ground(self.h, C.byref(p), C.byref(r), th.ctypes.data_as(_dp)))
        self._shape = (B, N)

    def device_trajectory(self):
        """The linearisation trajectory resident on the device (HSQP_BLK_X / HSQP_BLK_U): (x[B][N+1][58], u[B][N][35])."""
        return self.debug_read(_abi.BLK_X), self.debug_read(_abi.BLK_U)

    def stamps(self):
        """The raw time stamps of the resident grid (HSQP_BLK_STAMPS, [B][N+1]): pre- and post-event node share one."""
        return self.debug_read(_abi.BLK_STAMPS)

    def device_params(self):
        """The per-node parameter table resident on the device ([B][N+1][72])."""
        B, N = self._shape
        a = np.zeros((B, N + 1, _abi.NODE_PARAMS))
        n = self.lib.hsqp_debug_read(self.h, _abi.BLK_PARAMS, a.ctypes.data_as(C.c_void_p), a.nbytes)
        if n < 0:
            raise HsqpError(n, self.lib.hsqp_last_error(self.h).decode())
        return a

    def iterate(self, n_iterations=1, take_step=False, kkt=False, linesearch=False, until_converged=False, value_function=False):
        """until_converged: n_iterations is an upper bound; the call ends when every instance's step is below deltaTol (or no step length
        was accepted): ocs2's SqpSolver::checkConvergence.  value_function: keep the Riccati value function of the last iteration
        (HSQP_ITER_VALUE_FUNCTION; value_function / evaluate_value_function below).  Returns the number of iterations run."""
        self._check(self.lib.hsqp_iterate_device(self.h, n_iterations, (1 if take_step else 0) | (2 if kkt else 0) | (4 if linesearch else 0) |
                                                 (8 if until_converged else 0) | (_abi.ITER_VALUE_FUNCTION if value_function else 0)))
        return int(self.lib.hsqp_last_iterations(self.h))

    def iteration_log(self, iteration):
        """(perf[B], alpha[B], step_type[B]) iteration `iteration` of the last until_converged call ended with."""
        B, _ = self._shape
        perf, alpha, st = (_abi.Perf * B)(), np.zeros(B), np.zeros(B, dtype=np.int32)
        self._check(self.lib.hsqp_iteration_log(self.h, iteration, perf, alpha.ctypes.data_as(_dp), st.ctypes.data_as(C.POINTER(C.c_int32))))
        return self._perf(perf), alpha, st

    def update_weights(self, Q=None, R=None, Qf=None):
        """hsqp_update_weights: new diagonal Q[58] / R[35] / Qf[58] of the live handle (None keeps the current one)."""
        arrs = [None if a is None else _c(a) for a in (Q, R, Qf)]
        self._check(self.lib.hsqp_update_weights(self.h, *[None if a is None else a.ctypes.data_as(_dp) for a in arrs]))

    def term_weights(self):
        """hsqp_get_term_weights: the handle's current foot-cost weights, foot-constraint gains, barrier parameters (an _abi.TermWeights)."""
        w = _abi.TermWeights()
        self._check(self.lib.hsqp_get_term_weights(self.h, C.byref(w)))
        return w

    def update_term_weights(self, w):
        """hsqp_update_term_weights: replace them (what the reference's gains updaters retune at run time)."""
        self._check(self.lib.hsqp_update_term_weights(self.h, C.byref(w)))

    # ---- sqp::Settings of the line search (task.info sqp block + upstream defaults)
    def linesearch_settings(self):
        s = _abi.LinesearchSettings()
        self.lib.hsqp_linesearch_defaults(C.byref(s))
        return s

    def set_linesearch(self, **kw):
        s = self.linesearch_settings()
        for k, v in kw.items():
            if not hasattr(s, k):
                raise ValueError(f"unknown line-search setting {k}")
            setattr(s, k, float(v))
        self._check(self.lib.hsqp_set_linesearch(self.h, C.byref(s)))
        return s

    # ---- multi-GPU data path: problem shards / solutions that are already in this GPU's HBM (e.g. the tensors RCCL
    #      scattered / will gather); pointers are raw device addresses (torch: tensor.data_ptr())
    def upload_device(self, batch, n_nodes, dt, x_init_ptr, x_ptr, u_ptr, params_ptr, dt_nodes_ptr=0):
        cast = lambda a: C.cast(C.c_void_p(int(a)), _dp) if a else None  # noqa: E731
        p = _abi.Problem(batch=batch, n_nodes=n_nodes, dt=float(dt), x_init=cast(x_init_ptr), x_traj=cast(x_ptr), u_traj=cast(u_ptr),
                         node_params=cast(params_ptr), dt_nodes=cast(dt_nodes_ptr))
        self._check(self.lib.hsqp_upload_device(self.h, C.byref(p)))
        self._shape = (batch, n_nodes)

    def download_device(self, x_ptr=0, u_ptr=0, dx_ptr=0, du_ptr=0, perf_before_ptr=0, perf_after_ptr=0, kkt_ptr=0, grad_inf_ptr=0):
        cast = lambda a, t=_dp: C.cast(C.c_void_p(int(a)), t) if a else None  # noqa: E731
        s = _abi.Solution(x=cast(x_ptr), u=cast(u_ptr), dx=cast(dx_ptr), du=cast(du_ptr), perf_before=cast(perf_before_ptr, C.POINTER(_abi.Perf)),
                          perf_after=cast(perf_after_ptr, C.POINTER(_abi.Perf)), kkt=cast(kkt_ptr), grad_inf=cast(grad_inf_ptr))
        self._check(self.lib.hsqp_download_device(self.h, C.byref(s)))

    def download(self):
        B, N = self._shape
        s, out, pb, pa = self._alloc_solution(B, N)
        self._check(self.lib.hsqp_download(self.h, C.byref(s)))
        return self._finish(s, out, pb, pa)

    def kernel_ms(self):
        ms = np.zeros(5)
        self._check(self.lib.hsqp_last_kernel_ms(self.h, ms.ctypes.data_as(_dp)))
        return dict(lq=ms[0], project=ms[1], riccati=ms[2], step_perf=ms[3], total=ms[4])

    def kernel_forms(self):
        """Which kernel forms the handle runs (HSQP_BLK_FORMS): {"lq_limb": bool, "value_quad": bool, "lq_ranges": int, "ric_fact": bool, "chain_fused": bool}."""
        f = np.zeros(5, dtype=np.int32)
        n = self.lib.hsqp_debug_read(self.h, _abi.BLK_FORMS, f.ctypes.data_as(C.c_void_p), f.nbytes)
        if n < 0:
            self._check(int(n))
        return {"lq_limb": bool(f[0]), "value_quad": bool(f[1]), "lq_ranges": int(f[2]), "ric_fact": bool(f[3]), "chain_fused": bool(f[4])}

    def set_scan_backoff_persistent(self, on=True):
        """hsqp_set_scan_backoff_persistent: the KKT gate's back-off survives uploads of the same shape (receding-horizon use)."""
        self._check(self.lib.hsqp_set_scan_backoff_persistent(self.h, 1 if on else 0))

    def scan_backoffs(self):
        """Iterations that ran the serial recursion because the automatic sweep choice was backing off (hsqp_scan_backoffs)."""
        return int(self.lib.hsqp_scan_backoffs(self.h))

    def scan_fallbacks(self):
        """Iterations whose parallel-in-time sweep failed the KKT gate and were redone with the serial recursion (hsqp_scan_fallbacks)."""
        return int(self.lib.hsqp_scan_fallbacks(self.h))

    # ---- the step after the solve: MPC_MRT_Interface::evaluatePolicy + computeJointTorques (WBMpcMrtJointController.cpp:136-147)
    def evaluate_policy(self, s):
        """Feed-forward policy of the device-resident solution at s[b] seconds after the first node: (x[B,58], u[B,35], tau[B,23])."""
        B, _ = self._shape
        s = _c(np.broadcast_to(s, (B,)))
        x, u, tau = np.zeros((B, _abi.NX)), np.zeros((B, _abi.NU)), np.zeros((B, _abi.NJ))
        self._check(self.lib.hsqp_evaluate_policy(self.h, s.ctypes.data_as(_dp), x.ctypes.data_as(_dp), u.ctypes.data_as(_dp), tau.ctypes.data_as(_dp)))
        return x, u, tau

    # ---- the Riccati feedback policy (include/hsqp_feedback.h; ocs2 LinearController, useFeedbackPolicy)
    def feedback_policy(self, first=0, count=None):
        """Entries [first, first + count) of the feedback policy u = uff + K x of every instance (count None: up to node N):
        (K[B, count, 35, 58], uff[B, count, 35])."""
        B, N = self._shape
        if count is None:
            count = N + 1 - first
        K, uff = np.zeros((B, max(count, 0), _abi.NU, _abi.NX)), np.zeros((B, max(count, 0), _abi.NU))
        self._check(self.lib.hsqp_feedback_policy(self.h, int(first), int(count), K.ctypes.data_as(_dp), uff.ctypes.data_as(_dp)))
        return K, uff

    def feedback_policy_device(self, first, count, K_ptr=0, uff_ptr=0):
        """hsqp_feedback_policy_device: the same entries into device memory (K_ptr / uff_ptr: device addresses, 0 = not wanted)."""
        cast = lambda a: C.cast(C.c_void_p(int(a)), _dp) if a else None  # noqa: E731
        self._check(self.lib.hsqp_feedback_policy_device(self.h, int(first), int(count), cast(K_ptr), cast(uff_ptr)))

    def evaluate_feedback_policy(self, s, x_meas):
        """Feedback policy at s[b] seconds after the first node and the measured states x_meas[b]: (x[B,58], u[B,35], tau[B,23])."""
        B, _ = self._shape
        s = _c(np.broadcast_to(s, (B,)))
        x_meas = _c(np.broadcast_to(x_meas, (B, _abi.NX)))
        x, u, tau = np.zeros((B, _abi.NX)), np.zeros((B, _abi.NU)), np.zeros((B, _abi.NJ))
        self._check(self.lib.hsqp_evaluate_feedback_policy(self.h, s.ctypes.data_as(_dp), x_meas.ctypes.data_as(_dp), x.ctypes.data_as(_dp),
                                                           u.ctypes.data_as(_dp), tau.ctypes.data_as(_dp)))
        return x, u, tau

    # ---- the Riccati value function (include/hsqp_value.h; ocs2 SqpSolver::getValueFunction, createValueFunction)
    def value_function(self, k0=0, k1=None):
        """The record of nodes k0 .. k1 (k1 None: node N) an iterate(..., value_function=True) left: (S[B, n, 58, 58] symmetric, s[B, n, 58],
        xbar[B, n, 58]) — the cost-to-go s' dx + 1/2 dx' S dx in dx = x - xbar, xbar the trajectory the QP was linearised at."""
        B, N = self._shape
        if k1 is None:
            k1 = N
        n = max(int(k1) - int(k0) + 1, 0)
        S, s, xbar = np.zeros((B, n, _abi.NX, _abi.NX)), np.zeros((B, n, _abi.NX)), np.zeros((B, n, _abi.NX))
        self._check(self.lib.hsqp_value_function(self.h, int(k0), int(k1), S.ctypes.data_as(_dp), s.ctypes.data_as(_dp), xbar.ctypes.data_as(_dp)))
        return S, s, xbar

    def value_function_device(self, k0, k1, S_ptr=0, s_ptr=0, xbar_ptr=0):
        """hsqp_value_function_device: the same into device memory (device addresses, 0 = not wanted)."""
        cast = lambda a: C.cast(C.c_void_p(int(a)), _dp) if a else None  # noqa: E731
        self._check(self.lib.hsqp_value_function_device(self.h, int(k0), int(k1), cast(S_ptr), cast(s_ptr), cast(xbar_ptr)))

    def evaluate_value_function(self, s, x, hessian=True):
        """getValueFunction(t, x) at s[B, n] (or [B]: one query per instance) seconds after the first node and the states x[B, n, 58]:
        (dV[B, n], dfdx[B, n, 58], dfdxx[B, n, 58, 58] or None without hessian); dV = s' dx + 1/2 dx' S dx is the value relative to the nominal."""
        B, _ = self._shape
        s = np.asarray(s, dtype=np.float64)
        s = _c(s.reshape(B, -1) if s.ndim else np.full((B, 1), float(s)))
        n = s.shape[1]
        x = np.asarray(x, dtype=np.float64)
        x = _c(np.broadcast_to(x.reshape(B, 1, _abi.NX) if x.ndim == 2 else x, (B, n, _abi.NX)))   # ([B, 58]: the same state for an instance's queries)
        dV, g = np.zeros((B, n)), np.zeros((B, n, _abi.NX))
        H = np.zeros((B, n, _abi.NX, _abi.NX)) if hessian else None
        self._check(self.lib.hsqp_evaluate_value_function(self.h, n, s.ctypes.data_as(_dp), x.ctypes.data_as(_dp), dV.ctypes.data_as(_dp), g.ctypes.data_as(_dp),
                                                          H.ctypes.data_as(_dp) if hessian else None))
        return dV, g, H

    def evaluate_value_function_device(self, n_queries, s_ptr, x_ptr, dV_ptr=0, dfdx_ptr=0, dfdxx_ptr=0):
        """hsqp_evaluate_value_function_device: every array in device memory (device addresses, 0 = output not wanted)."""
        cast = lambda a: C.cast(C.c_void_p(int(a)), _dp) if a else None  # noqa: E731
        self._check(self.lib.hsqp_evaluate_value_function_device(self.h, int(n_queries), cast(s_ptr), cast(x_ptr), cast(dV_ptr), cast(dfdx_ptr), cast(dfdxx_ptr)))

    # ---- batched policy rollout (include/hsqp_rollout.h; ocs2 MRT_BASE::rolloutPolicy)
    _INTEGRATORS = {"ode45": _abi.ROLLOUT_ODE45, "rk4": _abi.ROLLOUT_RK4}
    _CONTROLLERS = {"feedforward": _abi.ROLLOUT_FEEDFORWARD, "feedback": _abi.ROLLOUT_FEEDBACK}

    def rollout_settings(self, integrator="ode45", controller="feedforward", **tolerances):
        """hsqp_rollout_settings: hsqp_rollout_defaults (the task.info rollout block) with the named fields replaced (abs_tol, rel_tol,
        initial_step, max_steps_per_second)."""
        st = _abi.RolloutSettings()
        self.lib.hsqp_rollout_defaults(C.byref(st))
        st.integrator = self._INTEGRATORS[integrator] if isinstance(integrator, str) else int(integrator)
        st.controller = self._CONTROLLERS[controller] if isinstance(controller, str) else int(controller)
        for k, v in tolerances.items():
            if k not in ("abs_tol", "rel_tol", "initial_step", "max_steps_per_second"):
                raise TypeError(f"unknown rollout setting {k!r}")
            setattr(st, k, float(v))
        return st

    def rollout_policy(self, s0, x0, duration, n_samples=1, integrator="ode45", controller="feedforward", **tolerances):
        """Every instance from x0[b] at s0[b] under the resident policy: dict(x[B, n, 58], u[B, n, 35], status[B], steps[B], rejected[B]).
        A failed instance (step cap: HSQP_ERR_NOT_CONVERGED, non-finite: HSQP_ERR_NUMERIC) raises HsqpError with the complete result of the
        call as its `result` attribute."""
        B = self._shape[0] if self._shape else 1      # (no problem uploaded: the library reports it)
        st = self.rollout_settings(integrator, controller, **tolerances)
        s0 = _c(np.broadcast_to(s0, (B,)))
        x0 = _c(np.broadcast_to(x0, (B, _abi.NX)))
        n = max(int(n_samples), 1)
        out = dict(x=np.zeros((B, n, _abi.NX)), u=np.zeros((B, n, _abi.NU)), status=np.zeros(B, np.int32), steps=np.zeros(B, np.int32),
                   rejected=np.zeros(B, np.int32))
        ip = C.POINTER(C.c_int32)
        rc = self.lib.hsqp_rollout_policy(self.h, C.byref(st), s0.ctypes.data_as(_dp), x0.ctypes.data_as(_dp), C.c_double(duration), int(n_samples),
                                          out["x"].ctypes.data_as(_dp), out["u"].ctypes.data_as(_dp), out["status"].ctypes.data_as(ip),
                                          out["steps"].ctypes.data_as(ip), out["rejected"].ctypes.data_as(ip))
        self._check_rollout(rc, out)
        return out

    def rollout_policy_device(self, s0_ptr, x0_ptr, duration, n_samples=1, x_ptr=0, u_ptr=0, status_ptr=0, steps_ptr=0, rejected_ptr=0,
                              integrator="ode45", controller="feedforward", **tolerances):
        """hsqp_rollout_policy_device: the same with every array in device memory (addresses; 0 = not wanted for x, u, steps, rejected).
        Returns the library's return code after raising for everything but a failed instance (HSQP_ERR_NOT_CONVERGED / HSQP_ERR_NUMERIC)."""
        st = self.rollout_settings(integrator, controller, **tolerances)
        cast = lambda a: C.cast(C.c_void_p(int(a)), _dp) if a else None  # noqa: E731
        icast = lambda a: C.cast(C.c_void_p(int(a)), C.POINTER(C.c_int32)) if a else None  # noqa: E731
        rc = self.lib.hsqp_rollout_policy_device(self.h, C.byref(st), cast(s0_ptr), cast(x0_ptr), C.c_double(duration), int(n_samples), cast(x_ptr),
                                                 cast(u_ptr), icast(status_ptr), icast(steps_ptr), icast(rejected_ptr))
        if rc not in (0, _abi.ERR_NOT_CONVERGED, _abi.ERR_NUMERIC):
            self._check(rc)
        return rc

    def _check_rollout(self, rc, result):
        if rc != 0:
            err = HsqpError(rc, self.lib.hsqp_last_error(self.h).decode())
            if rc in (_abi.ERR_NOT_CONVERGED, _abi.ERR_NUMERIC):
                err.result = result
            raise err

    # ---- include/hsqp_push.h: per-instance external pushes on the plant of the rollout and the resident loop
    @staticmethod
    def pack_pushes(pushes, max_pushes=None):
        """(n_pushes int32 [B], table (_abi.Push * max_pushes) * B, max_pushes) from a list, one entry per instance, of lists of pushes: dicts
        (body, t_start, duration, point, force; reserved optional) or tuples in that order."""
        B = len(pushes)
        mp = max(1, max((len(p) for p in pushes), default=1)) if max_pushes is None else int(max_pushes)
        n = np.array([len(p) for p in pushes], dtype=np.int32)
        table = ((_abi.Push * mp) * max(B, 1))()
        for b, row in enumerate(pushes):
            for i, p in enumerate(row[:mp]):
                if not isinstance(p, dict):
                    p = dict(zip(("body", "t_start", "duration", "point", "force"), p))
                e = table[b][i]
                e.body, e.reserved = int(p["body"]), int(p.get("reserved", 0))
                e.t_start, e.duration = float(p["t_start"]), float(p["duration"])
                e.point[:] = [float(v) for v in p.get("point", (0.0, 0.0, 0.0))]
                e.force[:] = [float(v) for v in p["force"]]
        return n, table, mp

    def set_pushes(self, pushes, max_pushes=None):
        """hsqp_push_set: the resident push table, pushes[b] the pushes of instance b (pack_pushes).  It stays until clear_pushes() or the
        next set_pushes(); every rollout and loop cycle of a problem with len(pushes) instances applies it."""
        n, table, mp = self.pack_pushes(pushes, max_pushes)
        self._check(self.lib.hsqp_push_set(self.h, len(pushes), mp, n.ctypes.data_as(C.POINTER(C.c_int32)), C.cast(table, C.POINTER(_abi.Push))))

    def set_pushes_device(self, batch, max_pushes, n_pushes_ptr, pushes_ptr):
        """hsqp_push_set_device: both arrays in device memory (addresses); their values are not checked."""
        self._check(self.lib.hsqp_push_set_device(self.h, int(batch), int(max_pushes), C.cast(C.c_void_p(int(n_pushes_ptr)), C.POINTER(C.c_int32)),
                                                  C.cast(C.c_void_p(int(pushes_ptr)), C.POINTER(_abi.Push))))

    def clear_pushes(self):
        self._check(self.lib.hsqp_push_clear(self.h))

    def get_pushes(self):
        """hsqp_push_get: the resident table as set_pushes takes it (a list per instance of dicts); HsqpError if none is set."""
        B, mp = C.c_int(0), C.c_int(0)
        self._check(self.lib.hsqp_push_get(self.h, C.byref(B), C.byref(mp), None, None))
        n = np.zeros(B.value, np.int32)
        table = ((_abi.Push * mp.value) * B.value)()
        self._check(self.lib.hsqp_push_get(self.h, None, None, n.ctypes.data_as(C.POINTER(C.c_int32)), C.cast(table, C.POINTER(_abi.Push))))
        return [[dict(body=int(e.body), t_start=e.t_start, duration=e.duration, point=list(e.point), force=list(e.force)) for e in table[b][:n[b]]]
                for b in range(B.value)]

    # ---- include/hsqp_plant.h: the plant of the rollout and the resident loop
    def plant_settings(self, kind="torque", kp=None, kd=None, armature=None, lookahead=None, reserved=0):
        """hsqp_plant_defaults with the given fields replaced (kp, kd, armature: a scalar for every joint or 23 values)."""
        st = _abi.PlantSettings()
        self.lib.hsqp_plant_defaults(C.byref(st))
        st.kind = {"flow": _abi.PLANT_FLOW, "torque": _abi.PLANT_TORQUE}.get(kind, kind)
        st.reserved = int(reserved)
        if lookahead is not None:
            st.lookahead = float(lookahead)
        for name, v in (("kp", kp), ("kd", kd), ("armature", armature)):
            if v is not None:
                getattr(st, name)[:] = [float(e) for e in np.broadcast_to(np.asarray(v, dtype=float), (_abi.NJ,))]
        return st

    def set_plant(self, kind="torque", kp=None, kd=None, armature=None, lookahead=None):
        """hsqp_plant_set: the resident plant of every rollout and loop cycle of this handle.  kind "torque": full forward dynamics under the joint
        law tau = tau_ff + kp (q_p - q) + kd (v_p - v) with the policy evaluated `lookahead` seconds ahead; "flow": the MPC's own flow map.
        It stays until clear_plant() or the next set_plant()."""
        st = self.plant_settings(kind, kp, kd, armature, lookahead)
        self._check(self.lib.hsqp_plant_set(self.h, C.byref(st)))

    def clear_plant(self):
        self._check(self.lib.hsqp_plant_clear(self.h))

    def get_plant(self):
        """hsqp_plant_get: dict(kind "flow" / "torque", lookahead, kp [23], kd [23], armature [23])."""
        st = _abi.PlantSettings()
        self._check(self.lib.hsqp_plant_get(self.h, C.byref(st)))
        return dict(kind="torque" if st.kind == _abi.PLANT_TORQUE else "flow", lookahead=st.lookahead, kp=np.array(st.kp[:]), kd=np.array(st.kd[:]),
                    armature=np.array(st.armature[:]))

    # ---- include/hsqp_contact.h: the ground under the torque plant
    def contact_settings(self, enabled=True, stiffness=None, damping=None, mu=None, slip_velocity=None, ground_height=None, reserved=0):
        """hsqp_contact_defaults (mu: the model's friction_mu) with the given fields replaced."""
        st = _abi.ContactSettings()
        self.lib.hsqp_contact_defaults(getattr(self, "h", None), C.byref(st))
        st.enabled, st.reserved = int(bool(enabled)), int(reserved)
        for name, v in (("stiffness", stiffness), ("damping", damping), ("mu", mu), ("slip_velocity", slip_velocity), ("ground_height", ground_height)):
            if v is not None:
                setattr(st, name, float(v))
        return st

    def set_contact(self, enabled=True, stiffness=None, damping=None, mu=None, slip_velocity=None, ground_height=None):
        """hsqp_contact_set: compliant ground contact with Coulomb friction at the eight sole corners of the torque plant (set_plant("torque")); inert
        on the flow plant.  It stays until clear_contact() or the next set_contact(); the MPC never sees it."""
        st = self.contact_settings(enabled, stiffness, damping, mu, slip_velocity, ground_height)
        self._check(self.lib.hsqp_contact_set(self.h, C.byref(st)))

    def set_contact_instances(self, ground):
        """hsqp_contact_set_instances: ground [B, 2] = (height, mu) of every instance, or None: every instance back to the setting's values."""
        if ground is None:
            self._check(self.lib.hsqp_contact_set_instances(self.h, 0, None))
            return
        g = _c(ground).reshape(-1, 2)
        self._check(self.lib.hsqp_contact_set_instances(self.h, len(g), C.cast(g.ctypes.data_as(_dp), C.POINTER(_abi.ContactGround))))

    def set_contact_instances_device(self, batch, ground_ptr):
        """hsqp_contact_set_instances_device: the table in device memory (address); its values are not checked."""
        self._check(self.lib.hsqp_contact_set_instances_device(self.h, int(batch), C.cast(C.c_void_p(int(ground_ptr)), C.POINTER(_abi.ContactGround))))

    def clear_contact(self):
        self._check(self.lib.hsqp_contact_clear(self.h))

    def get_contact(self):
        """hsqp_contact_get: dict(enabled, stiffness, damping, mu, slip_velocity, ground_height)."""
        st = _abi.ContactSettings()
        self._check(self.lib.hsqp_contact_get(self.h, C.byref(st)))
        return dict(enabled=bool(st.enabled), stiffness=st.stiffness, damping=st.damping, mu=st.mu, slip_velocity=st.slip_velocity, ground_height=st.ground_height)

    def contact_forces(self, x):
        """hsqp_contact_eval at the states x [B, 58] with the handle's setting and table: (force [B, 2, 4, 3] on the feet in world axes — (ft_x, ft_y, fn)
        per sole corner —, penetration [B, 2, 4]).  Needs no resident solution."""
        x = _c(np.atleast_2d(x))
        B = x.shape[0]
        f, d = np.zeros((B, _abi.CONTACT_FEET, _abi.CONTACT_CORNERS, 3)), np.zeros((B, _abi.CONTACT_FEET, _abi.CONTACT_CORNERS))
        self._check(self.lib.hsqp_contact_eval(self.h, B, x.ctypes.data_as(_dp), f.ctypes.data_as(_dp), d.ctypes.data_as(_dp)))
        return f, d

    # ---- include/hsqp_terrain.h: per-instance height-map terrain under that ground
    @staticmethod
    def pack_terrain_maps(maps):
        """The arrays of hsqp_terrain_set_maps: maps = a list of (heights [ny, nx], cell) -> (nx, ny int32 [n], cell [n], heights concatenated)."""
        hs = [np.ascontiguousarray(h, dtype=np.float64) for h, _ in maps]
        if any(h.ndim != 2 for h in hs):
            raise ValueError("a map is heights [ny, nx] (row-major: H[iy][ix])")
        nx, ny = np.array([h.shape[1] for h in hs], np.int32), np.array([h.shape[0] for h in hs], np.int32)
        cell = np.array([float(c) for _, c in maps], np.float64)
        return nx, ny, cell, (np.concatenate([h.ravel() for h in hs]) if hs else np.zeros(0))

    @staticmethod
    def pack_terrain_instances(place):
        """The table of hsqp_terrain_set_instances as a ctypes array: per instance dict(map, origin (x, y), yaw) — map -1 (or None for the entry): the plane."""
        tab = (_abi.TerrainPlacement * len(place))()
        for t, p in zip(tab, place):
            p = p or dict(map=-1)
            ox, oy = p.get("origin", (0.0, 0.0))
            t.map, t.reserved, t.origin_x, t.origin_y, t.yaw = int(p["map"]), int(p.get("reserved", 0)), float(ox), float(oy), float(p.get("yaw", 0.0))
        return tab

    def set_terrain_maps(self, maps):
        """hsqp_terrain_set_maps: the height maps all instances share — a list of (heights [ny, nx], cell), at most 16, 2 .. 256 nodes per axis; an empty
        list frees them.  A map acts under the instances set_terrain_instances places on it, on the torque plant with contact on; the MPC never sees it."""
        nx, ny, cell, heights = self.pack_terrain_maps(maps)
        self._check(self.lib.hsqp_terrain_set_maps(self.h, len(nx), nx.ctypes.data_as(_ip), ny.ctypes.data_as(_ip), cell.ctypes.data_as(_dp), heights.ctypes.data_as(_dp)))

    def set_terrain_instances(self, place):
        """hsqp_terrain_set_instances: per instance dict(map, origin (x, y) — the world position of grid node (0, 0) —, yaw), map -1: the plane; None: no
        table.  The instance's contact ground height (set_contact / set_contact_instances) is an offset under its map."""
        if place is None:
            self._check(self.lib.hsqp_terrain_set_instances(self.h, 0, None))
            return
        tab = self.pack_terrain_instances(place)
        self._check(self.lib.hsqp_terrain_set_instances(self.h, len(tab), tab))

    def set_terrain_instances_device(self, batch, place_ptr):
        """hsqp_terrain_set_instances_device: the table in device memory (address); its values are not checked (the kernels clamp the map index)."""
        self._check(self.lib.hsqp_terrain_set_instances_device(self.h, int(batch), C.cast(C.c_void_p(int(place_ptr)), C.POINTER(_abi.TerrainPlacement))))

    def clear_terrain(self):
        self._check(self.lib.hsqp_terrain_clear(self.h))

    def get_terrain_maps(self):
        """hsqp_terrain_get_maps: a list of (heights [ny, nx], cell)."""
        n = np.zeros(1, np.int32)
        nx, ny, cell = np.zeros(_abi.TERRAIN_MAX_MAPS, np.int32), np.zeros(_abi.TERRAIN_MAX_MAPS, np.int32), np.zeros(_abi.TERRAIN_MAX_MAPS)
        self._check(self.lib.hsqp_terrain_get_maps(self.h, n.ctypes.data_as(_ip), nx.ctypes.data_as(_ip), ny.ctypes.data_as(_ip), cell.ctypes.data_as(_dp), None, 0))
        total = int((nx[:n[0]].astype(np.int64) * ny[:n[0]]).sum())
        heights = np.zeros(max(total, 1))
        self._check(self.lib.hsqp_terrain_get_maps(self.h, n.ctypes.data_as(_ip), None, None, None, heights.ctypes.data_as(_dp), total))
        out, at = [], 0
        for m in range(int(n[0])):
            cnt = int(nx[m]) * int(ny[m])
            out.append((heights[at:at + cnt].reshape(int(ny[m]), int(nx[m])).copy(), float(cell[m])))
            at += cnt
        return out

    def get_terrain_instances(self, batch):
        """hsqp_terrain_get_instances: per instance dict(map, origin, yaw); instances past the table have map -1."""
        tab = (_abi.TerrainPlacement * int(batch))()
        self._check(self.lib.hsqp_terrain_get_instances(self.h, int(batch), tab))
        return [dict(map=int(t.map), origin=(t.origin_x, t.origin_y), yaw=t.yaw) for t in tab]

    def terrain_height(self, xy):
        """hsqp_terrain_eval at the world points xy [B, n, 2]: (height [B, n] — the instance's ground height plus its map's —, normal [B, n, 3]).  Works
        with any plant kind and needs no resident solution."""
        xy = _c(xy)
        if xy.ndim != 3 or xy.shape[2] != 2:
            raise ValueError("xy: [B, n, 2]")
        B, n = xy.shape[:2]
        hgt, nrm = np.zeros((B, n)), np.zeros((B, n, 3))
        self._check(self.lib.hsqp_terrain_eval(self.h, B, n, xy.ctypes.data_as(_dp), hgt.ctypes.data_as(_dp), nrm.ctypes.data_as(_dp)))
        return hgt, nrm

    # ---- include/hsqp_actuator.h: the actuator model on the torque plant
    def actuator_settings(self, enabled=True, command_period=None, effort_limit=None, damping=None, friction=None, friction_velocity=None, reserved=0):
        """hsqp_actuator_defaults with the given fields replaced (effort_limit, damping, friction: a scalar for every joint or 23 values)."""
        st = _abi.ActuatorSettings()
        self.lib.hsqp_actuator_defaults(C.byref(st))
        st.enabled, st.reserved = int(bool(enabled)), int(reserved)
        if command_period is not None:
            st.command_period = float(command_period)
        if friction_velocity is not None:
            st.friction_velocity = float(friction_velocity)
        for name, v in (("effort_limit", effort_limit), ("damping", damping), ("friction", friction)):
            if v is not None:
                getattr(st, name)[:] = [float(e) for e in np.broadcast_to(np.asarray(v, dtype=float), (_abi.NJ,))]
        return st

    def set_actuator(self, enabled=True, command_period=None, effort_limit=None, damping=None, friction=None, friction_velocity=None):
        """hsqp_actuator_set: the actuator model of the torque plant (set_plant("torque")) — the joint command sampled every command_period seconds
        and held (0: continuous), the actuator torque clamped to +-effort_limit, viscous damping and regularised dry friction at the joints; inert
        on the flow plant.  It stays until clear_actuator() or the next set_actuator(); the MPC never sees it."""
        st = self.actuator_settings(enabled, command_period, effort_limit, damping, friction, friction_velocity)
        self._check(self.lib.hsqp_actuator_set(self.h, C.byref(st)))

    def clear_actuator(self):
        self._check(self.lib.hsqp_actuator_clear(self.h))

    def get_actuator(self):
        """hsqp_actuator_get: dict(enabled, command_period, effort_limit [23], damping [23], friction [23], friction_velocity)."""
        st = _abi.ActuatorSettings()
        self._check(self.lib.hsqp_actuator_get(self.h, C.byref(st)))
        return dict(enabled=bool(st.enabled), command_period=st.command_period, effort_limit=np.array(st.effort_limit[:]), damping=np.array(st.damping[:]),
                    friction=np.array(st.friction[:]), friction_velocity=st.friction_velocity)

    def actuator_torques(self, batch=None):
        """hsqp_actuator_last: (tau_cmd, tau_act, tau_passive) [batch, 23] each at the final state of the most recent rollout (or loop cycle) on the
        actuator model (batch None: the resident problem's); NaN rows for an instance that did not end OK.  |tau_cmd| > effort_limit: the joint
        is saturated."""
        if batch is None:
            batch = self._shape[0] if self._shape else 1
        out = [np.zeros((int(batch), _abi.NJ)) for _ in range(3)]
        self._check(self.lib.hsqp_actuator_last(self.h, int(batch), *(o.ctypes.data_as(_dp) for o in out)))
        return tuple(out)

    # ---- include/hsqp_inertia.h: per-instance link mass scales and rigid payloads of the torque plant
    @staticmethod
    def pack_inertia(mass_scale, payloads=None):
        """The table of hsqp_inertia_set_instances as a ctypes array: mass_scale [B, 24], or [B] broadcast over the links; payloads: per instance a list
        of dict(body, mass, com [3], inertia [6] = xx, xy, xz, yy, yz, zz about its own centre of mass; com and inertia default to zero), or None."""
        ms = np.asarray(mass_scale, dtype=float)
        if ms.ndim == 1:
            ms = np.repeat(ms[:, None], _abi.NB, axis=1)
        if ms.ndim != 2 or ms.shape[1] != _abi.NB:
            raise ValueError("mass_scale: [B, %d] or [B]" % _abi.NB)
        B = ms.shape[0]
        if payloads is not None and len(payloads) != B:
            raise ValueError("payloads: one list per instance")
        tab = (_abi.InertiaInstance * B)()
        for b in range(B):
            tab[b].mass_scale[:] = [float(v) for v in ms[b]]
            mine = list(payloads[b]) if payloads is not None else []
            if len(mine) > _abi.INERTIA_PAYLOADS:
                raise ValueError("instance %d: more than %d payloads" % (b, _abi.INERTIA_PAYLOADS))
            tab[b].n_payloads = len(mine)
            for i, p in enumerate(mine):
                q = tab[b].payload[i]
                q.body, q.reserved, q.mass = int(p["body"]), int(p.get("reserved", 0)), float(p["mass"])
                q.com[:] = [float(v) for v in p.get("com", (0.0, 0.0, 0.0))]
                q.inertia[:] = [float(v) for v in p.get("inertia", (0.0,) * 6)]
        return tab

    def set_inertia_instances(self, mass_scale, payloads=None):
        """hsqp_inertia_set_instances: the inertial variation of every instance's torque PLANT (set_plant("torque")) — link i's mass and rotational
        inertia times mass_scale[b, i], and up to two rigid payloads per instance (pack_inertia); None: no table.  Inert on the flow plant.  It
        stays until clear_inertia() or the next call; the MPC never sees it."""
        if mass_scale is None:
            self._check(self.lib.hsqp_inertia_set_instances(self.h, 0, None))
            return
        tab = self.pack_inertia(mass_scale, payloads)
        self._check(self.lib.hsqp_inertia_set_instances(self.h, len(tab), tab))

    def set_inertia_instances_device(self, batch, table_ptr):
        """hsqp_inertia_set_instances_device: the table in device memory (address); its values are not checked."""
        self._check(self.lib.hsqp_inertia_set_instances_device(self.h, int(batch), C.cast(C.c_void_p(int(table_ptr)), C.POINTER(_abi.InertiaInstance))))

    def clear_inertia(self):
        self._check(self.lib.hsqp_inertia_clear(self.h))

    def get_inertia_instances(self, batch):
        """hsqp_inertia_get_instances: (mass_scale [batch, 24], payloads: per instance a list of dict(body, mass, com, inertia)); instances past the
        table are neutral."""
        tab = (_abi.InertiaInstance * int(batch))()
        self._check(self.lib.hsqp_inertia_get_instances(self.h, int(batch), tab))
        ms = np.array([list(t.mass_scale) for t in tab])
        pay = [[dict(body=int(t.payload[i].body), mass=t.payload[i].mass, com=list(t.payload[i].com), inertia=list(t.payload[i].inertia))
                for i in range(min(max(int(t.n_payloads), 0), _abi.INERTIA_PAYLOADS))] for t in tab]   # (an unchecked device table: clamped as the kernels do)
        return ms, pay

    def plant_dynamics(self, x):
        """hsqp_inertia_eval at the states x [B, 58] with instance b's entry of the table (none: the nominal model): (M [B, 29, 29] the plant's mass
        matrix without armature, nle [B, 29] its bias forces, mass [B] its total mass).  Needs no resident solution."""
        x = _c(np.atleast_2d(x))
        B = x.shape[0]
        M, nle, mass = np.zeros((B, _abi.NV, _abi.NV)), np.zeros((B, _abi.NV)), np.zeros(B)
        self._check(self.lib.hsqp_inertia_eval(self.h, B, x.ctypes.data_as(_dp), M.ctypes.data_as(_dp), nle.ctypes.data_as(_dp), mass.ctypes.data_as(_dp)))
        return M, nle, mass

    # ---- include/hsqp_observe.h: what the MPC of the resident loop measures of the plant — bias, noise, sensor and compute delay
    def set_observation(self, sensor_delay=0, compute_delay=0, seed=0):
        """hsqp_observe_set: the measurement is sensor_delay + compute_delay MPC periods old when its policy takes over; the controller knows of
        compute_delay only (it poses the problem at t - compute_delay * period and the plant enters the policy at that offset).  seed: the key of
        the noise stream of set_observation_instances.  Delays cannot change under a started loop."""
        st = _abi.ObserveSettings()
        st.sensor_delay, st.compute_delay, st.seed = int(sensor_delay), int(compute_delay), int(seed)
        self._check(self.lib.hsqp_observe_set(self.h, C.byref(st)))

    @staticmethod
    def pack_observation(bias, sigma):
        """The table of hsqp_observe_set_instances as a ctypes array: bias and sigma [B, 58], each broadcast from [B], [58] or a scalar against the other."""
        bias, sigma = np.asarray(bias, dtype=np.float64), np.asarray(sigma, dtype=np.float64)
        if bias.ndim == 1 and bias.shape[0] != _abi.NX:
            bias = bias[:, None]
        if sigma.ndim == 1 and sigma.shape[0] != _abi.NX:
            sigma = sigma[:, None]
        B = max([a.shape[0] for a in (bias, sigma) if a.ndim == 2] + [1])
        bias, sigma = _c(np.broadcast_to(bias, (B, _abi.NX))), _c(np.broadcast_to(sigma, (B, _abi.NX)))
        tab = (_abi.ObserveInstance * B)()
        for b in range(B):
            tab[b].bias[:] = bias[b].tolist()
            tab[b].sigma[:] = sigma[b].tolist()
        return tab

    def set_observation_instances(self, bias, sigma):
        """hsqp_observe_set_instances: per instance a constant bias and the standard deviation of white Gaussian noise on every entry of the state
        the MPC measures (pack_observation); bias None: no table.  The plant never sees it."""
        if bias is None:
            self._check(self.lib.hsqp_observe_set_instances(self.h, 0, None))
            return
        tab = self.pack_observation(bias, sigma)
        self._check(self.lib.hsqp_observe_set_instances(self.h, len(tab), tab))

    def set_observation_instances_device(self, batch, table_ptr):
        """hsqp_observe_set_instances_device: the table in device memory (address); its values are not checked."""
        self._check(self.lib.hsqp_observe_set_instances_device(self.h, int(batch), C.cast(C.c_void_p(int(table_ptr)), C.POINTER(_abi.ObserveInstance))))

    def clear_observation(self):
        self._check(self.lib.hsqp_observe_clear(self.h))

    def get_observation(self, batch):
        """hsqp_observe_get: dict(sensor_delay, compute_delay, seed, bias [batch, 58], sigma [batch, 58]); instances past the table are neutral."""
        st, tab = _abi.ObserveSettings(), (_abi.ObserveInstance * int(batch))()
        self._check(self.lib.hsqp_observe_get(self.h, C.byref(st), int(batch), tab))
        return dict(sensor_delay=int(st.sensor_delay), compute_delay=int(st.compute_delay), seed=int(st.seed),
                    bias=np.array([list(t.bias) for t in tab]), sigma=np.array([list(t.sigma) for t in tab]))

    def observe(self, x, draw):
        """hsqp_observe_eval: y [B, 58], what instance b's entry of the table makes of x[b] at draw index `draw` (bias and noise, no delay)."""
        x = _c(np.atleast_2d(x))
        y = np.zeros_like(x)
        self._check(self.lib.hsqp_observe_eval(self.h, x.shape[0], C.c_uint32(int(draw)), x.ctypes.data_as(_dp), y.ctypes.data_as(_dp)))
        return y

    def observe_device(self, batch, draw, x_ptr, y_ptr):
        """hsqp_observe_eval_device: the same with both arrays in device memory (addresses)."""
        cast = lambda a: C.cast(C.c_void_p(int(a)), _dp)  # noqa: E731
        self._check(self.lib.hsqp_observe_eval_device(self.h, int(batch), C.c_uint32(int(draw)), cast(x_ptr), cast(y_ptr)))

    def last_observation(self):
        """hsqp_observe_last: (y [B, 58], t_p) — the observation the last completed cycle of the loop used and its problem time."""
        y, tp = np.zeros((max(self._loop_batch, 1), _abi.NX)), C.c_double(0.0)
        self._check(self.lib.hsqp_observe_last(self.h, y.ctypes.data_as(_dp), C.byref(tp)))
        return y, tp.value

    # ---- include/hsqp_loop.h: velocity-command targets and the resident closed loop
    def command_targets(self, v_cmd, x0, t0, horizon, filter_alpha=0.0, v_filt=None, base_velocity=False):
        """hsqp_command_targets: (target_times[B, 3], target_states[B, 3, 58], v_filt[B, 4]) of B instances from their commands
        (vx, vy, height, yaw rate) and measured states; v_filt: the filter state before the call (None: the commands, a converged filter).
        The arithmetic of reference.velocity_command_targets.
        A centroidal solver calls hsqp_centroidal_command_targets (include/hsqp_cent_loop.h, reference.centroidal_velocity_command_targets);
        base_velocity=True then appends its by-product, the base velocity [B, 6] from the centroidal momentum, to the result."""
        x0 = _c(np.atleast_2d(x0))
        B = x0.shape[0]
        v_cmd = _c(np.broadcast_to(v_cmd, (B, _abi.CMD_N)))
        vf = v_cmd.copy() if v_filt is None else _c(np.broadcast_to(v_filt, (B, _abi.CMD_N))).copy()
        tt, ts = np.zeros((B, _abi.CMD_KNOTS)), np.zeros((B, _abi.CMD_KNOTS, _abi.NX))
        if self.model.centroidal:
            if x0.shape != (B, _abi.NX):
                raise ValueError("x0 must be [B][58] (centroidal rows padded with zeros)")
            bv = np.zeros((B, 6)) if base_velocity else None
            self._check(self.lib.hsqp_centroidal_command_targets(self.h, B, v_cmd.ctypes.data_as(_dp), vf.ctypes.data_as(_dp), C.c_double(filter_alpha),
                                                                 x0.ctypes.data_as(_dp), C.c_double(t0), C.c_double(horizon), tt.ctypes.data_as(_dp),
                                                                 ts.ctypes.data_as(_dp), bv.ctypes.data_as(_dp) if base_velocity else None))
            return (tt, ts, vf, bv) if base_velocity else (tt, ts, vf)
        if base_velocity:
            raise ValueError("base_velocity: a by-product of the centroidal generator (the whole-body state row carries the base velocity)")
        self._check(self.lib.hsqp_command_targets(self.h, B, v_cmd.ctypes.data_as(_dp), vf.ctypes.data_as(_dp), C.c_double(filter_alpha), x0.ctypes.data_as(_dp),
                                                  C.c_double(t0), C.c_double(horizon), tt.ctypes.data_as(_dp), ts.ctypes.data_as(_dp)))
        return tt, ts, vf

    def command_targets_device(self, batch, v_cmd_ptr, v_filt_ptr, x0_ptr, t0, horizon, target_times_ptr, target_states_ptr, filter_alpha=0.0, base_vel_ptr=0):
        """hsqp_command_targets_device: the same with every array in device memory (addresses); v_filt is updated in place.  A centroidal solver
        calls hsqp_centroidal_command_targets_device; base_vel_ptr (0: not wanted) receives its base velocities [B][6]."""
        cast = lambda a: C.cast(C.c_void_p(int(a)), _dp)  # noqa: E731
        if self.model.centroidal:
            self._check(self.lib.hsqp_centroidal_command_targets_device(self.h, int(batch), cast(v_cmd_ptr), cast(v_filt_ptr), C.c_double(filter_alpha), cast(x0_ptr),
                                                                        C.c_double(t0), C.c_double(horizon), cast(target_times_ptr), cast(target_states_ptr),
                                                                        cast(base_vel_ptr) if base_vel_ptr else None))
            return
        if base_vel_ptr:
            raise ValueError("base_vel_ptr: a by-product of the centroidal generator")
        self._check(self.lib.hsqp_command_targets_device(self.h, int(batch), cast(v_cmd_ptr), cast(v_filt_ptr), C.c_double(filter_alpha), cast(x0_ptr),
                                                         C.c_double(t0), C.c_double(horizon), cast(target_times_ptr), cast(target_states_ptr)))

    def loop_settings(self, n_nodes, dt, period=None, filter_alpha=None, iterations=1, take_step=True, kkt=False, linesearch=True, swing=None,
                      terrain_height=0.0, arm_swing=True, integrator="ode45", controller="feedforward", **tolerances):
        """hsqp_loop_settings: hsqp_loop_defaults (period 1 / 60 s, filter_alpha 0.8) with the grid, the iteration flags of iterate(), the
        rollout settings of rollout_settings() and the model's swing configuration.  On a centroidal solver the defaults are still the
        whole-body task file's: pass dt and period from model.sqp."""
        from .reference import swing_config
        st = _abi.LoopSettings()
        self.lib.hsqp_loop_defaults(self.h, C.byref(st))
        st.n_nodes, st.dt, st.iterations = int(n_nodes), float(dt), int(iterations)
        if period is not None:
            st.period = float(period)
        if filter_alpha is not None:
            st.filter_alpha = float(filter_alpha)
        st.iterate_flags = (1 if take_step else 0) | (2 if kkt else 0) | (4 if linesearch else 0)
        st.rollout = self.rollout_settings(integrator, controller, **tolerances)
        st.swing = swing_config(self.model) if swing is None else swing
        st.terrain_height, st.arm_swing = float(terrain_height), 1 if arm_swing else 0
        return st

    def loop_start(self, settings, t0, x0, v_cmd, n_events=None, event_times=None, mode_sequence=None, gait=None):
        """hsqp_loop_start: B = len(x0) instances, their commands [B][4] and mode schedules (reference.pack_reference's first three arrays),
        uploaded once.  gait (an _abi.GaitSettings, reference.gait_settings) instead of the schedules: hsqp_loop_start_gait, the resident
        gait schedule and ladder of include/hsqp_gait.h own the schedule."""
        x0 = _c(np.atleast_2d(x0))
        B = x0.shape[0]
        v_cmd = _c(np.broadcast_to(v_cmd, (B, _abi.CMD_N)))
        if gait is not None:
            if n_events is not None or event_times is not None or mode_sequence is not None:
                raise ValueError("either mode schedules or gait settings")
            if x0.shape != (B, _abi.NX):
                raise ValueError("inconsistent loop array shapes")
            self._loop_batch = 0
            self._check(self.lib.hsqp_loop_start_gait(self.h, C.byref(settings), C.byref(gait), B, C.c_double(t0), x0.ctypes.data_as(_dp), v_cmd.ctypes.data_as(_dp)))
            self._loop_batch = self._gait_batch = B
            self._gait_events = self._loop_events = int(gait.max_events)
            self._shape = (B, int(settings.n_nodes))
            self._loop_nodes = int(settings.n_nodes)
            return
        n_events = np.ascontiguousarray(n_events, dtype=np.int32)
        mode_sequence = np.ascontiguousarray(mode_sequence, dtype=np.int32)
        event_times = _c(event_times)
        if x0.shape != (B, _abi.NX) or n_events.shape != (B,) or event_times.ndim != 2 or event_times.shape[0] != B or \
                mode_sequence.shape != (B, event_times.shape[1] + 1):
            raise ValueError("inconsistent loop array shapes")
        ip = C.POINTER(C.c_int32)
        self._loop_batch = 0
        start = self.lib.hsqp_loop_start_centroidal if self.model.centroidal else self.lib.hsqp_loop_start   # (include/hsqp_cent_loop.h)
        self._check(start(self.h, C.byref(settings), B, C.c_double(t0), x0.ctypes.data_as(_dp), v_cmd.ctypes.data_as(_dp), event_times.shape[1],
                          n_events.ctypes.data_as(ip), event_times.ctypes.data_as(_dp), mode_sequence.ctypes.data_as(ip)))
        self._loop_batch = B
        self._loop_events = int(event_times.shape[1])
        self._shape = (B, int(settings.n_nodes))
        self._loop_nodes = int(settings.n_nodes)

    def loop_command(self, v_cmd):
        """hsqp_loop_command: new commands [B][4], in effect from the next cycle."""
        v_cmd = _c(np.broadcast_to(v_cmd, (self._loop_batch, _abi.CMD_N)) if self._loop_batch else v_cmd)   # (no loop: the library reports it)
        self._check(self.lib.hsqp_loop_command(self.h, v_cmd.ctypes.data_as(_dp)))

    def loop_command_device(self, v_cmd_ptr):
        self._check(self.lib.hsqp_loop_command_device(self.h, C.cast(C.c_void_p(int(v_cmd_ptr)), _dp)))

    def loop_run(self, n_cycles, log=True):
        """hsqp_loop_run: dict(x[n, B, 58], u[n, B, 35], cycles_done) (x, u: the rows of the completed cycles; None without log).  A cycle
        that fails raises HsqpError with that dict as its `result` attribute."""
        B, n = max(self._loop_batch, 1), max(int(n_cycles), 1)
        x = np.zeros((n, B, _abi.NX)) if log else None
        u = np.zeros((n, B, _abi.NU)) if log else None
        done = C.c_int(0)
        rc = self.lib.hsqp_loop_run(self.h, int(n_cycles), x.ctypes.data_as(_dp) if log else None, u.ctypes.data_as(_dp) if log else None, C.byref(done))
        out = dict(x=x[:done.value] if log else None, u=u[:done.value] if log else None, cycles_done=done.value)
        if rc != 0:
            err = HsqpError(rc, self.lib.hsqp_last_error(self.h).decode())
            err.result = out
            raise err
        return out

    def loop_run_device(self, n_cycles, x_log_ptr=0, u_log_ptr=0):
        """hsqp_loop_run_device: logs in device memory (addresses; 0 = not wanted).  Returns the cycles done."""
        cast = lambda a: C.cast(C.c_void_p(int(a)), _dp) if a else None  # noqa: E731
        done = C.c_int(0)
        self._check(self.lib.hsqp_loop_run_device(self.h, int(n_cycles), cast(x_log_ptr), cast(u_log_ptr), C.byref(done)))
        return done.value

    def loop_state(self):
        """hsqp_loop_state: (t, x[B, 58], v_filt[B, 4]) where the loop stands."""
        B = max(self._loop_batch, 1)
        t, x, vf = C.c_double(0.0), np.zeros((B, _abi.NX)), np.zeros((B, _abi.CMD_N))
        self._check(self.lib.hsqp_loop_state(self.h, C.byref(t), x.ctypes.data_as(_dp), vf.ctypes.data_as(_dp)))
        return t.value, x, vf

    def loop_state_device(self, x_ptr=0, v_filt_ptr=0):
        cast = lambda a: C.cast(C.c_void_p(int(a)), _dp) if a else None  # noqa: E731
        t = C.c_double(0.0)
        self._check(self.lib.hsqp_loop_state_device(self.h, C.byref(t), cast(x_ptr), cast(v_filt_ptr)))
        return t.value

    # ---- include/hsqp_episode.h: per-instance failure isolation and episode reset
    def episode_settings(self, on_failure="park", min_base_height=None, max_base_height=None, max_tilt=None):
        """hsqp_episode_settings: hsqp_episode_defaults (park, bounds off) with the given policy ("park" / "reset") and box."""
        st = _abi.EpisodeSettings()
        self.lib.hsqp_episode_defaults(C.byref(st))
        st.on_failure = {"park": _abi.EPISODE_PARK, "reset": _abi.EPISODE_RESET}.get(on_failure, on_failure)
        for k, v in (("min_base_height", min_base_height), ("max_base_height", max_base_height), ("max_tilt", max_tilt)):
            if v is not None:
                setattr(st, k, float(v))
        return st

    def loop_isolate(self, settings=None, x_reset=None):
        """hsqp_loop_isolate on the started loop: a failed instance is parked or reset on the device (settings: episode_settings()), the others
        go on.  x_reset [B][58]: where a failed instance restarts (None: the measured states the loop holds now)."""
        settings = self.episode_settings() if settings is None else settings
        if x_reset is not None:
            x_reset = _c(np.broadcast_to(x_reset, (max(self._loop_batch, 1), _abi.NX)))
        self._check(self.lib.hsqp_loop_isolate(self.h, C.byref(settings), x_reset.ctypes.data_as(_dp) if x_reset is not None else None))

    def loop_reset(self, ids, x0=None, v_cmd=None):
        """hsqp_loop_reset_instances: a new episode for the instances `ids`, from x0 [n][58] (None: their x_reset) with the commands v_cmd [n][4]
        (None: keep), in effect from the next cycle."""
        ids = np.ascontiguousarray(np.atleast_1d(ids), dtype=np.int32)
        n = ids.shape[0]
        if x0 is not None:
            x0 = _c(np.broadcast_to(x0, (n, _abi.NX)))
        if v_cmd is not None:
            v_cmd = _c(np.broadcast_to(v_cmd, (n, _abi.CMD_N)))
        self._check(self.lib.hsqp_loop_reset_instances(self.h, n, ids.ctypes.data_as(C.POINTER(C.c_int32)), x0.ctypes.data_as(_dp) if x0 is not None else None,
                                                       v_cmd.ctypes.data_as(_dp) if v_cmd is not None else None))

    def loop_episodes(self):
        """hsqp_loop_episodes: dict(state[B], cause[B], fail_cycle[B], n_failures[B], n_episodes[B]) (_abi.EP_*)."""
        names = ("state", "cause", "fail_cycle", "n_failures", "n_episodes")
        out = {k: np.zeros(max(self._loop_batch, 1), np.int32) for k in names}
        self._check(self.lib.hsqp_loop_episodes(self.h, *[out[k].ctypes.data_as(C.POINTER(C.c_int32)) for k in names]))
        return out

    def loop_episodes_device(self, state_ptr=0, cause_ptr=0, fail_cycle_ptr=0, n_failures_ptr=0, n_episodes_ptr=0):
        icast = lambda a: C.cast(C.c_void_p(int(a)), C.POINTER(C.c_int32)) if a else None  # noqa: E731
        self._check(self.lib.hsqp_loop_episodes_device(self.h, icast(state_ptr), icast(cause_ptr), icast(fail_cycle_ptr), icast(n_failures_ptr), icast(n_episodes_ptr)))

    # ---- include/hsqp_metrics.h: per-instance episode metrics accumulated on the device
    def loop_metrics_enable(self):
        """hsqp_loop_metrics_enable on the started loop: every record empty, one sample per instance behind every cycle's rollout from now on."""
        self._check(self.lib.hsqp_loop_metrics_enable(self.h))

    def loop_metrics_disable(self):
        """hsqp_loop_metrics_disable: accumulation stops; the records stay readable until the next start."""
        self._check(self.lib.hsqp_loop_metrics_disable(self.h))

    def loop_metrics_restart(self, ids=None):
        """hsqp_loop_metrics_restart: the records of the instances `ids` (None: all) are closed (END_HOST) and reopened; their episodes are untouched."""
        if ids is None:
            self._check(self.lib.hsqp_loop_metrics_restart(self.h, 0, None))
            return
        ids = np.ascontiguousarray(np.atleast_1d(ids), dtype=np.int32)
        self._check(self.lib.hsqp_loop_metrics_restart(self.h, ids.shape[0], ids.ctypes.data_as(C.POINTER(C.c_int32))))

    @staticmethod
    def _metrics_which(which):
        return {"current": _abi.METRICS_CURRENT, "previous": _abi.METRICS_PREVIOUS}.get(which, which)

    def loop_metrics(self, which="current"):
        """hsqp_loop_metrics: the records of every instance ("current": the open one, "previous": the last closed one) as a dict of arrays, one
        per field of hsqp_metrics ([B], touchdowns / start_xy / end_xy [B][2])."""
        B = max(self._loop_batch, 1)
        rec = (_abi.Metrics * B)()
        self._check(self.lib.hsqp_loop_metrics(self.h, int(self._metrics_which(which)), rec))
        return metrics_dict(rec)

    def loop_metrics_device(self, which, out_ptr):
        """hsqp_loop_metrics_device: the records [B] into device memory at the address out_ptr (B * sizeof(hsqp_metrics) bytes)."""
        self._check(self.lib.hsqp_loop_metrics_device(self.h, int(self._metrics_which(which)), C.cast(C.c_void_p(int(out_ptr)), C.POINTER(_abi.Metrics))))

    def metrics_summary(self, records):
        """metrics_summary(records) with the model's total mass and gravity."""
        return metrics_summary(records, self.model.total_mass, self.model.desc.gravity)

    # ---- include/hsqp_grid.h: the ocs2 event-node time grid built per instance on the device
    def grid_settings(self, event_nodes=None, dt_min=None):
        """hsqp_grid_settings: hsqp_grid_defaults (32 event nodes, dt_min 1e-4) with the given values."""
        st = _abi.GridSettings()
        self.lib.hsqp_grid_defaults(C.byref(st))
        if event_nodes is not None:
            st.event_nodes = int(event_nodes)
        if dt_min is not None:
            st.dt_min = float(dt_min)
        return st

    def event_grid(self, t0, n_nodes, dt, n_events, event_times, settings=None):
        """hsqp_event_grid: the padded event-node grid of every instance from its events (n_events [B], event_times [B][E]):
        dict(n_intervals[B], dt_nodes[B, N], node_times[B, N + 1], status[B]), N = n_nodes + event_nodes — what upload_reference takes as dt and
        node_times.  An instance without a grid (_abi.GRID_OVERFLOW) raises HsqpError with that dict as its `result` attribute."""
        settings = self.grid_settings() if settings is None else settings
        n_events, event_times = np.ascontiguousarray(n_events, dtype=np.int32), _c(event_times)
        B = n_events.shape[0]
        if event_times.ndim != 2 or event_times.shape[0] != B:
            raise ValueError("inconsistent event array shapes")
        N = max(int(n_nodes) + int(settings.event_nodes), 0)
        out = dict(n_intervals=np.zeros(B, np.int32), dt_nodes=np.zeros((B, N)), node_times=np.zeros((B, N + 1)), status=np.zeros(B, np.int32))
        rc = self.lib.hsqp_event_grid(self.h, C.byref(settings), B, C.c_double(t0), int(n_nodes), C.c_double(dt), event_times.shape[1], n_events.ctypes.data_as(_ip),
                                      event_times.ctypes.data_as(_dp), out["n_intervals"].ctypes.data_as(_ip), out["dt_nodes"].ctypes.data_as(_dp),
                                      out["node_times"].ctypes.data_as(_dp), out["status"].ctypes.data_as(_ip))
        if rc != 0:
            err = HsqpError(rc, self.lib.hsqp_last_error(self.h).decode())
            err.result = out
            raise err
        return out

    def event_grid_device(self, settings, batch, t0, n_nodes, dt, max_events, n_events_ptr, event_times_ptr, n_intervals_ptr, dt_nodes_ptr, node_times_ptr, status_ptr=0):
        """hsqp_event_grid_device: the same with every array in device memory (addresses); the events are not checked."""
        cast = lambda a: C.cast(C.c_void_p(int(a)), _dp) if a else None  # noqa: E731
        icast = lambda a: C.cast(C.c_void_p(int(a)), _ip) if a else None  # noqa: E731
        self._check(self.lib.hsqp_event_grid_device(self.h, C.byref(settings), int(batch), C.c_double(t0), int(n_nodes), C.c_double(dt), int(max_events), icast(n_events_ptr),
                                                    cast(event_times_ptr), icast(n_intervals_ptr), cast(dt_nodes_ptr), cast(node_times_ptr), icast(status_ptr)))

    def loop_event_grid(self, settings=None, on=True):
        """hsqp_loop_event_grid on the started loop: from the next cycle every problem is posed on the padded event-node grid of its instance
        (settings: grid_settings()); on=False: back to the uniform grid.  debug_read / device_trajectory / stamps take the new node count from
        here on, which the device has after the next cycle."""
        if not on:
            self._check(self.lib.hsqp_loop_event_grid(self.h, None))
            if self._shape is not None and getattr(self, "_loop_nodes", 0):
                self._shape = (self._shape[0], self._loop_nodes)
            return
        settings = self.grid_settings() if settings is None else settings
        self._check(self.lib.hsqp_loop_event_grid(self.h, C.byref(settings)))
        self._grid_nodes = self._loop_nodes + int(settings.event_nodes)
        self._shape = (self._loop_batch, self._grid_nodes)

    def loop_grid(self):
        """hsqp_loop_grid: dict(n_intervals[B], dt_nodes[B, N], node_times[B, N + 1]) of the last completed cycle (which ran on the event grid)."""
        B, N = max(self._loop_batch, 1), max(getattr(self, "_grid_nodes", 0), 1)
        out = dict(n_intervals=np.zeros(B, np.int32), dt_nodes=np.zeros((B, N)), node_times=np.zeros((B, N + 1)))
        self._check(self.lib.hsqp_loop_grid(self.h, out["n_intervals"].ctypes.data_as(_ip), out["dt_nodes"].ctypes.data_as(_dp), out["node_times"].ctypes.data_as(_dp)))
        return out

    def loop_grid_device(self, n_intervals_ptr=0, dt_nodes_ptr=0, node_times_ptr=0):
        cast = lambda a: C.cast(C.c_void_p(int(a)), _dp) if a else None  # noqa: E731
        icast = lambda a: C.cast(C.c_void_p(int(a)), _ip) if a else None  # noqa: E731
        self._check(self.lib.hsqp_loop_grid_device(self.h, icast(n_intervals_ptr), cast(dt_nodes_ptr), cast(node_times_ptr)))

    # ---- include/hsqp_ground.h: per-instance ground-height estimate from the stance feet
    def ground_settings(self, enabled=True, box_above_ground=False, filter_alpha=None, initial_height=None):
        """hsqp_ground_settings: hsqp_ground_defaults (on, absolute box, the raw estimate, initial height 0) with the given values."""
        st = _abi.GroundSettings()
        self.lib.hsqp_ground_defaults(C.byref(st))
        st.enabled, st.box_above_ground = int(enabled), int(box_above_ground)
        if filter_alpha is not None:
            st.filter_alpha = float(filter_alpha)
        if initial_height is not None:
            st.initial_height = float(initial_height)
        return st

    def ground_estimate(self, x, t, n_events, event_times, mode_sequence, g=None, filter_alpha=0.0):
        """hsqp_ground_estimate: (g[B], foot_z[B, 2]) — the new latch of every instance from its state x [B][58], its mode schedule at time t and its latch
        g (None: zeros), and the heights of both contact frames."""
        x = _c(np.atleast_2d(x))
        B = x.shape[0]
        n_events, mode_sequence, event_times = np.ascontiguousarray(n_events, dtype=np.int32), np.ascontiguousarray(mode_sequence, dtype=np.int32), _c(event_times)
        if x.shape != (B, _abi.NX) or n_events.shape != (B,) or event_times.ndim != 2 or event_times.shape[0] != B or mode_sequence.shape != (B, event_times.shape[1] + 1):
            raise ValueError("inconsistent ground-estimate array shapes")
        g = np.zeros(B) if g is None else _c(np.broadcast_to(g, (B,))).copy()
        fz = np.zeros((B, 2))
        self._check(self.lib.hsqp_ground_estimate(self.h, B, C.c_double(t), x.ctypes.data_as(_dp), event_times.shape[1], n_events.ctypes.data_as(_ip),
                                                  event_times.ctypes.data_as(_dp), mode_sequence.ctypes.data_as(_ip), C.c_double(filter_alpha), g.ctypes.data_as(_dp),
                                                  fz.ctypes.data_as(_dp)))
        return g, fz

    def ground_estimate_device(self, batch, t, x_ptr, max_events, n_events_ptr, event_times_ptr, mode_sequence_ptr, g_ptr, foot_z_ptr=0, filter_alpha=0.0):
        """hsqp_ground_estimate_device: the same with every array in device memory (addresses); g is updated in place."""
        cast = lambda a: C.cast(C.c_void_p(int(a)), _dp) if a else None  # noqa: E731
        icast = lambda a: C.cast(C.c_void_p(int(a)), _ip) if a else None  # noqa: E731
        self._check(self.lib.hsqp_ground_estimate_device(self.h, int(batch), C.c_double(t), cast(x_ptr), int(max_events), icast(n_events_ptr), cast(event_times_ptr),
                                                         icast(mode_sequence_ptr), C.c_double(filter_alpha), cast(g_ptr), cast(foot_z_ptr)))

    def upload_reference_ground(self, x_init, n_nodes, dt, t0, n_events, event_times, mode_sequence, target_times, target_states, swing, terrain_heights,
                                arm_swing=True, mode="cold", node_times=None, x_traj=None, u_traj=None):
        """hsqp_upload_reference_ground: upload_reference_warm (mode "shift" / "cold") or, with x_traj and u_traj, upload_reference, with one terrain
        height per instance (terrain_heights [B]) in place of the reference's terrain_height."""
        x_init = _c(np.atleast_2d(x_init))
        caller = x_traj is not None
        warm = _abi.WARM_CALLER if caller else {"shift": _abi.WARM_SHIFT, "cold": _abi.WARM_COLD}[mode]
        if caller:
            x_traj, u_traj = _c(x_traj), _c(u_traj)
            if x_traj.ndim == 2:
                x_traj, u_traj = x_traj[None], u_traj[None]
        self._upload_reference(x_init.shape[0], int(n_nodes), x_init, x_traj, u_traj, dt, t0, n_events, event_times, mode_sequence, target_times, target_states,
                               swing, 0.0, arm_swing, node_times, warm, terrain_heights=terrain_heights)

    def loop_ground(self, settings=None, g_init=None, on=True):
        """hsqp_loop_ground on the started loop: from the next cycle every instance's ground height is estimated from its stance feet, the command's
        height entry means height above it and step 2 takes it as the instance's terrain height (settings: ground_settings(); g_init [B]: the latches'
        start values, None: settings.initial_height).  on=False: off again."""
        if not on:
            self._check(self.lib.hsqp_loop_ground(self.h, None, None))
            return
        settings = self.ground_settings() if settings is None else settings
        if g_init is not None:
            g_init = _c(np.broadcast_to(g_init, (max(self._loop_batch, 1),)))
        self._check(self.lib.hsqp_loop_ground(self.h, C.byref(settings), g_init.ctypes.data_as(_dp) if g_init is not None else None))

    def loop_ground_state(self):
        """hsqp_loop_ground_state: (g[B], foot_z[B, 2]) — the latches and the contact-frame heights of the last completed cycle."""
        B = max(self._loop_batch, 1)
        g, fz = np.zeros(B), np.zeros((B, 2))
        self._check(self.lib.hsqp_loop_ground_state(self.h, g.ctypes.data_as(_dp), fz.ctypes.data_as(_dp)))
        return g, fz

    def loop_ground_state_device(self, g_ptr=0, foot_z_ptr=0):
        cast = lambda a: C.cast(C.c_void_p(int(a)), _dp) if a else None  # noqa: E731
        self._check(self.lib.hsqp_loop_ground_state_device(self.h, cast(g_ptr), cast(foot_z_ptr)))

    # ---- include/hsqp_perceive.h: per-foot swing heights read from the height map
    def perceive_settings(self, enabled=True):
        """hsqp_perceive_settings: hsqp_perceive_defaults (on) with the given value."""
        st = _abi.PerceiveSettings()
        self.lib.hsqp_perceive_defaults(C.byref(st))
        st.enabled = int(enabled)
        return st

    def foot_heights(self, x, t, n_events, event_times, mode_sequence, target_times, target_states, touch_down_height_offset):
        """hsqp_foot_heights: (lift_off[B, 2, E + 1], touch_down[B, 2, E + 1], foothold_xy[B, 2, E + 1, 2]) — for every instance and foot the lift-off and
        touch-down height of every phase of its schedule, read from the resident height map under the foot (a contact run that has begun) or under the
        foothold the targets carry to its touch-down time (a run ahead), from the state x [B][58] at time t."""
        x = _c(np.atleast_2d(x))
        B = x.shape[0]
        n_events, mode_sequence, event_times = np.ascontiguousarray(n_events, dtype=np.int32), np.ascontiguousarray(mode_sequence, dtype=np.int32), _c(event_times)
        target_times, target_states = _c(target_times), _c(target_states)
        if (x.shape != (B, _abi.NX) or n_events.shape != (B,) or event_times.ndim != 2 or event_times.shape[0] != B or mode_sequence.shape != (B, event_times.shape[1] + 1)
                or target_times.ndim != 2 or target_times.shape[0] != B or target_states.shape != (B, target_times.shape[1], _abi.NX)):
            raise ValueError("inconsistent foot-height array shapes")
        E = event_times.shape[1]
        lift, touch, fxy = np.zeros((B, 2, E + 1)), np.zeros((B, 2, E + 1)), np.zeros((B, 2, E + 1, 2))
        self._check(self.lib.hsqp_foot_heights(self.h, B, C.c_double(t), x.ctypes.data_as(_dp), E, n_events.ctypes.data_as(_ip), event_times.ctypes.data_as(_dp),
                                               mode_sequence.ctypes.data_as(_ip), target_times.shape[1], target_times.ctypes.data_as(_dp),
                                               target_states.ctypes.data_as(_dp), C.c_double(touch_down_height_offset), lift.ctypes.data_as(_dp),
                                               touch.ctypes.data_as(_dp), fxy.ctypes.data_as(_dp)))
        return lift, touch, fxy

    def foot_heights_device(self, batch, t, x_ptr, max_events, n_events_ptr, event_times_ptr, mode_sequence_ptr, n_knots, target_times_ptr, target_states_ptr,
                            touch_down_height_offset, lift_off_ptr, touch_down_ptr, foothold_xy_ptr=0):
        """hsqp_foot_heights_device: the same with every array in device memory (addresses)."""
        cast = lambda a: C.cast(C.c_void_p(int(a)), _dp) if a else None  # noqa: E731
        icast = lambda a: C.cast(C.c_void_p(int(a)), _ip) if a else None  # noqa: E731
        self._check(self.lib.hsqp_foot_heights_device(self.h, int(batch), C.c_double(t), cast(x_ptr), int(max_events), icast(n_events_ptr), cast(event_times_ptr),
                                                      icast(mode_sequence_ptr), int(n_knots), cast(target_times_ptr), cast(target_states_ptr),
                                                      C.c_double(touch_down_height_offset), cast(lift_off_ptr), cast(touch_down_ptr), cast(foothold_xy_ptr)))

    def upload_reference_heights(self, x_init, n_nodes, dt, t0, n_events, event_times, mode_sequence, target_times, target_states, swing, lift_off, touch_down,
                                 arm_swing=True, mode="cold", node_times=None, x_traj=None, u_traj=None):
        """hsqp_upload_reference_heights: upload_reference_warm (mode "shift" / "cold") or, with x_traj and u_traj, upload_reference, with the planner's
        three-argument update: lift_off, touch_down [B][2][max_events + 1] in place of the reference's terrain_height (touch_down holds the offset)."""
        x_init = _c(np.atleast_2d(x_init))
        caller = x_traj is not None
        warm = _abi.WARM_CALLER if caller else {"shift": _abi.WARM_SHIFT, "cold": _abi.WARM_COLD}[mode]
        if caller:
            x_traj, u_traj = _c(x_traj), _c(u_traj)
            if x_traj.ndim == 2:
                x_traj, u_traj = x_traj[None], u_traj[None]
        self._upload_reference(x_init.shape[0], int(n_nodes), x_init, x_traj, u_traj, dt, t0, n_events, event_times, mode_sequence, target_times, target_states,
                               swing, 0.0, arm_swing, node_times, warm, heights=(lift_off, touch_down))

    def loop_perceive(self, settings=None, on=True):
        """hsqp_loop_perceive on the started loop: from the next cycle step 2 takes every instance's per-foot lift-off and touch-down heights from the
        resident height map (settings: perceive_settings()).  on=False: off again."""
        if not on:
            self._check(self.lib.hsqp_loop_perceive(self.h, None))
            return
        settings = self.perceive_settings() if settings is None else settings
        self._check(self.lib.hsqp_loop_perceive(self.h, C.byref(settings)))

    def loop_foot_heights(self):
        """hsqp_loop_foot_heights: (lift_off[B, 2, E + 1], touch_down[B, 2, E + 1], foothold_xy[B, 2, E + 1, 2]) of the last completed cycle; E the
        max_events of the loop's schedule (a resident gait: its settings')."""
        B, E = max(self._loop_batch, 1), max(getattr(self, "_loop_events", 1), 1)
        lift, touch, fxy = np.zeros((B, 2, E + 1)), np.zeros((B, 2, E + 1)), np.zeros((B, 2, E + 1, 2))
        self._check(self.lib.hsqp_loop_foot_heights(self.h, lift.ctypes.data_as(_dp), touch.ctypes.data_as(_dp), fxy.ctypes.data_as(_dp)))
        return lift, touch, fxy

    def loop_foot_heights_device(self, lift_off_ptr=0, touch_down_ptr=0, foothold_xy_ptr=0):
        cast = lambda a: C.cast(C.c_void_p(int(a)), _dp) if a else None  # noqa: E731
        self._check(self.lib.hsqp_loop_foot_heights_device(self.h, cast(lift_off_ptr), cast(touch_down_ptr), cast(foothold_xy_ptr)))

    # ---- include/hsqp_gait.h: per-instance gait schedule and ladder
    def gait_reset(self, settings, batch, t0=0.0):
        """hsqp_gait_reset: `batch` instances in the initial state ({[t0 + 0.5], [STANCE, STANCE]}, rung 0) under `settings` (reference.gait_settings)."""
        self._gait_batch = 0
        self._check(self.lib.hsqp_gait_reset(self.h, C.byref(settings), int(batch), C.c_double(t0)))
        self._gait_batch, self._gait_events = int(batch), int(settings.max_events)

    def _gait_arrays(self):
        B, E = max(getattr(self, "_gait_batch", 0), 1), max(getattr(self, "_gait_events", 0), 1)
        return np.zeros(B, np.int32), np.zeros((B, E)), np.zeros((B, E + 1), np.int32)

    def gait_update(self, t, horizon, v_filt, x):
        """hsqp_gait_update: one update of every instance at time t from the filtered commands [B][4] and the measured states [B][58]:
        (n_events[B], event_times[B, E], mode_sequence[B, E + 1]) of this cycle, the layout upload_reference takes.  A failed update raises
        HsqpError (the state is unchanged) with those arrays as its `result` attribute."""
        ne, ev, seq = self._gait_arrays()
        B = ne.shape[0]
        v_filt, x = _c(np.broadcast_to(v_filt, (B, _abi.CMD_N))), _c(np.broadcast_to(x, (B, _abi.NX)))
        ip = C.POINTER(C.c_int32)
        rc = self.lib.hsqp_gait_update(self.h, B, C.c_double(t), C.c_double(horizon), v_filt.ctypes.data_as(_dp), x.ctypes.data_as(_dp), ne.ctypes.data_as(ip),
                                       ev.ctypes.data_as(_dp), seq.ctypes.data_as(ip))
        if rc != 0:
            err = HsqpError(rc, self.lib.hsqp_last_error(self.h).decode())
            err.result = (ne, ev, seq)
            raise err
        return ne, ev, seq

    def gait_update_device(self, batch, t, horizon, v_filt_ptr, x_ptr, n_events_ptr, event_times_ptr, mode_sequence_ptr):
        """hsqp_gait_update_device: the same with every array in device memory (addresses)."""
        cast = lambda a: C.cast(C.c_void_p(int(a)), _dp)  # noqa: E731
        icast = lambda a: C.cast(C.c_void_p(int(a)), C.POINTER(C.c_int32))  # noqa: E731
        self._check(self.lib.hsqp_gait_update_device(self.h, int(batch), C.c_double(t), C.c_double(horizon), cast(v_filt_ptr), cast(x_ptr), icast(n_events_ptr),
                                                     cast(event_times_ptr), icast(mode_sequence_ptr)))

    def gait_state(self):
        """hsqp_gait_state: dict(rung[B], last_change_time[B], n_events[B], event_times[B, E], mode_sequence[B, E + 1]) of the resident state
        (a gait loop's: that of its last completed cycle)."""
        ne, ev, seq = self._gait_arrays()
        rung, tc = np.zeros_like(ne), np.zeros(ne.shape[0])
        ip = C.POINTER(C.c_int32)
        self._check(self.lib.hsqp_gait_state(self.h, rung.ctypes.data_as(ip), tc.ctypes.data_as(_dp), ne.ctypes.data_as(ip), ev.ctypes.data_as(_dp), seq.ctypes.data_as(ip)))
        return dict(rung=rung, last_change_time=tc, n_events=ne, event_times=ev, mode_sequence=seq)

    def gait_state_device(self, rung_ptr=0, last_change_time_ptr=0, n_events_ptr=0, event_times_ptr=0, mode_sequence_ptr=0):
        cast = lambda a: C.cast(C.c_void_p(int(a)), _dp) if a else None  # noqa: E731
        icast = lambda a: C.cast(C.c_void_p(int(a)), C.POINTER(C.c_int32)) if a else None  # noqa: E731
        self._check(self.lib.hsqp_gait_state_device(self.h, icast(rung_ptr), cast(last_change_time_ptr), icast(n_events_ptr), cast(event_times_ptr),
                                                    icast(mode_sequence_ptr)))

    def joint_torques(self, x, u):
        x, u = _c(np.atleast_2d(x)), _c(np.atleast_2d(u))
        tau = np.zeros((x.shape[0], _abi.NJ))
        self._check(self.lib.hsqp_joint_torques(self.h, x.shape[0], x.ctypes.data_as(_dp), u.ctypes.data_as(_dp), tau.ctypes.data_as(_dp)))
        return tau

    # ---- reference-named accessors
    def getPrimalSolution(self):
        return self._sol["x"], self._sol["u"]

    def getPerformanceIndeces(self):
        return self._sol["perf_after"]

    def getBenchmarks(self):
        return self._sol["benchmarks"]

    # ---- parity/debug access to intermediate blocks of the last iteration
    def debug_read(self, what):
        B, N = self._shape
        shapes = {_abi.BLK_AB: (B, N, _abi.NX, _abi.NZ), _abi.BLK_BVEC: (B, N, _abi.NX), _abi.BLK_H: (B, N, _abi.NZ, _abi.NZ),
                  _abi.BLK_G: (B, N, _abi.NZ), _abi.BLK_CDE: (B, N, _abi.NE_MAX, _abi.NZ + 1), _abi.BLK_NE: (B, N),
                  _abi.BLK_COST: (B, N + 1), _abi.BLK_DX: (B, N + 1, _abi.NX), _abi.BLK_DU: (B, N, _abi.NU),
                  _abi.BLK_FLOW: (B, N, _abi.NX), _abi.BLK_X: (B, N + 1, _abi.NX), _abi.BLK_U: (B, N, _abi.NU), _abi.BLK_STAMPS: (B, N + 1)}
        a = np.zeros(shapes[what], dtype=np.int32 if what == _abi.BLK_NE else np.float64)
        n = self.lib.hsqp_debug_read(self.h, what, a.ctypes.data_as(C.c_void_p), a.nbytes)
        if n < 0:
            raise HsqpError(n, self.lib.hsqp_last_error(self.h).decode())
        assert n == a.nbytes, (n, a.nbytes)
        return a
