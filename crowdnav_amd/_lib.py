"""ctypes binding of libcrowdnav_amd.so (include/crowdnav_amd.h).

The shared library is the product: there is no CPU fallback.  If it has not been built
(`python -c "import __graft_entry__ as g; g.build()"` or `make -C crowdnav_amd/csrc`) importing this
module raises, and creating an engine without a visible gfx950 device raises CrowdNavAmdError.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# CROWDNAV_AMD_LIB: another build of the same library (kernel A/B experiments, scripts/gpu_ab.sh); default in-tree
LIB_PATH = os.environ.get('CROWDNAV_AMD_LIB') or os.path.join(HERE, 'lib', 'libcrowdnav_amd.so')
ABI_VERSION = 12

CN_OK, CN_ERR_INVALID, CN_ERR_UNSUPPORTED, CN_ERR_HIP, CN_ERR_NO_DEVICE = 0, -1, -2, -3, -4
INFO_NAMES = ('Nothing', 'Danger', 'ReachGoal', 'Collision', 'Timeout')
NOTHING, DANGER, REACH_GOAL, COLLISION, TIMEOUT = range(5)
ROBOT_EXTERNAL, ROBOT_ORCA = 0, 1
CIRCLE_CROSSING, SQUARE_CROSSING, MIXED = 0, 1, 2
HOLONOMIC, UNICYCLE = 0, 1
RECORD_FIELDS, SUMMARY_FIELDS = 6, 8
LAUNCH_COUNTERS = ('rollout_kernels', 'scheduled_kernels', 'ring_fills', 'async_fills', 'sarl_narrow', 'sarl_decide_steps')  # CN_COUNT_*
ROLLOUT_ROUTES = ('generic', 'fused', 'fused_split', 'shard')  # CN_ROUTE_*
SARL_ROUTES = ('lds_tile', 'lds_chunked', 'narrow', 'reg_sarl', 'reg_sarl_chunk', 'reg_cadrl', 'reg_lstm', 'reg_lstm2',
               'split_f16')  # CN_SARL_ROUTE_*
PRECISIONS = ('f32', 'f16x2')  # CN_PRECISION_*
FLAG_ASYNC_SCENARIO_FILL = 1
HUMANS_ORCA, HUMANS_CONSTANT_VELOCITY = 0, 1  # CN_HUMANS_*
HUMAN_MODELS = ('orca', 'constant_velocity')
MODES_MEAN, MODES_MIN = 0, 1  # CN_MODES_*
MODES_REDUCE = ('mean', 'min')
MODES_MAX = 8  # cn_path_modes.n_modes
PREDICT_CONSTANT_VELOCITY, PREDICT_TO_GOAL = 0, 1  # CN_PREDICT_*
PREDICT_MODELS = ('constant_velocity', 'to_goal')
PREDICT_ALIASES = {'cv': 'constant_velocity'}
GOALS_ENGINE, GOALS_HEADING = 0, 1  # CN_GOALS_*
GOALS_BASES = ('engine', 'heading')


class CrowdNavAmdError(RuntimeError):
    def __init__(self, status, message):
        super().__init__('libcrowdnav_amd: %s (status %d)' % (message, status))
        self.status = status


class CnConfig(C.Structure):
    """struct cn_config (include/crowdnav_amd.h)."""
    _fields_ = [
        ('num_envs', C.c_int32), ('num_humans', C.c_int32),
        ('time_step', C.c_double), ('time_limit', C.c_double),
        ('success_reward', C.c_double), ('collision_penalty', C.c_double),
        ('discomfort_dist', C.c_double), ('discomfort_penalty_factor', C.c_double),
        ('robot_visible', C.c_int32), ('robot_policy', C.c_int32),
        ('robot_safety_space', C.c_double), ('human_safety_space', C.c_double),
        ('neighbor_dist', C.c_double),
        ('max_neighbors', C.c_int32), ('scenario_rule', C.c_int32),
        ('time_horizon', C.c_double), ('time_horizon_obst', C.c_double),
        ('circle_radius', C.c_double), ('square_width', C.c_double),
        ('human_radius', C.c_double), ('human_v_pref', C.c_double),
        ('robot_radius', C.c_double), ('robot_v_pref', C.c_double),
        ('randomize_attributes', C.c_int32), ('device', C.c_int32),
        ('robot_kinematics', C.c_int32), ('flags', C.c_int32),
    ]


class CnRolloutIo(C.Structure):
    """struct cn_rollout_io (include/crowdnav_amd.h)."""
    _fields_ = [
        ('seed_base', C.c_uint32), ('seed_mod', C.c_uint32),
        ('episode_limit', C.c_int64), ('env_offset', C.c_int64), ('env_stride', C.c_int64),
        ('record_capacity', C.c_int32),
        ('ep_outcome', C.c_void_p), ('ep_steps', C.c_void_p), ('ep_return', C.c_void_p),
        ('ep_time', C.c_void_p), ('ep_danger', C.c_void_p), ('ep_danger_dmin_sum', C.c_void_p),
        ('ep_count', C.c_void_p), ('cur_steps', C.c_void_p), ('cur_return', C.c_void_p),
        ('cur_danger', C.c_void_p), ('cur_danger_dmin_sum', C.c_void_p),
        ('active', C.c_void_p), ('transitions', C.c_void_p),
        ('summary', C.c_void_p), ('blocks', C.c_void_p), ('blocks_records', C.c_int32),
        ('env_transitions', C.c_void_p),  # ABI v6
    ]


class CnLookaheadOut(C.Structure):
    """struct cn_lookahead_out (include/crowdnav_amd.h): device pointers; final_state8 and final_theta may be NULL."""
    _fields_ = [
        ('ret', C.c_void_p), ('info', C.c_void_p), ('steps', C.c_void_p), ('time', C.c_void_p),
        ('final_state8', C.c_void_p), ('final_theta', C.c_void_p),
    ]


class CnPathModes(C.Structure):
    """struct cn_path_modes (include/crowdnav_amd.h): M predicted futures and how their returns are reduced; weight may be NULL."""
    _fields_ = [
        ('n_modes', C.c_int32), ('reduce', C.c_int32), ('risk_penalty', C.c_double),
        ('human_vel', C.c_void_p), ('weight', C.c_void_p),
    ]


class CnPredictors(C.Structure):
    """struct cn_predictors (include/crowdnav_amd.h): the device predictors of M futures, the scratch table they fill and how the
    planner reduces the M returns; weight may be NULL."""
    _fields_ = [
        ('n_modes', C.c_int32), ('model', C.c_int32 * 8), ('reduce', C.c_int32), ('risk_penalty', C.c_double),
        ('human_vel', C.c_void_p), ('weight', C.c_void_p),
    ]


class CnModesOut(C.Structure):
    """struct cn_modes_out (include/crowdnav_amd.h): device pointers; everything but score may be NULL."""
    _fields_ = [
        ('score', C.c_void_p), ('risk', C.c_void_p), ('worst_mode', C.c_void_p), ('worst_info', C.c_void_p),
        ('worst_steps', C.c_void_p), ('worst_time', C.c_void_p),
        ('ret', C.c_void_p), ('info', C.c_void_p), ('steps', C.c_void_p), ('time', C.c_void_p),
    ]


class CnPlanCfg(C.Structure):
    """struct cn_plan_cfg (include/crowdnav_amd.h): the CEM planner's settings."""
    _fields_ = [
        ('n_steps', C.c_int32), ('n_candidates', C.c_int32), ('n_elites', C.c_int32), ('iterations', C.c_int32),
        ('bootstrap', C.c_int32), ('sort_humans', C.c_int32),
        ('init_std', C.c_double), ('min_std', C.c_double), ('smoothing', C.c_double), ('seed', C.c_uint64),
    ]


class CnPlan(C.Structure):
    """struct cn_plan (include/crowdnav_amd.h): device pointers; order may be NULL, final_state8 / value / score without bootstrap."""
    _fields_ = [
        ('mean', C.c_void_p), ('std', C.c_void_p), ('best_actions', C.c_void_p), ('best_score', C.c_void_p),
        ('action', C.c_void_p), ('candidates', C.c_void_p), ('look', CnLookaheadOut),
        ('value', C.c_void_p), ('score', C.c_void_p), ('order', C.c_void_p),
    ]


class CnTraceOut(C.Structure):
    """struct cn_trace_out (include/crowdnav_amd.h): device pointers; reward, info and dmin may be NULL."""
    _fields_ = [
        ('state8', C.c_void_p), ('episode', C.c_void_p), ('step', C.c_void_p),
        ('reward', C.c_void_p), ('info', C.c_void_p), ('dmin', C.c_void_p),
    ]


class CnSarlConfig(C.Structure):
    """struct cn_sarl_config (include/crowdnav_amd.h)."""
    _fields_ = [
        ('n_actions', C.c_int32), ('with_om', C.c_int32), ('cell_num', C.c_int32), ('om_channel_size', C.c_int32),
        ('cell_size', C.c_double), ('gamma', C.c_double), ('with_global_state', C.c_int32),
        ('mlp1_dims', C.c_int32 * 2), ('mlp2_dims', C.c_int32 * 2), ('attention_dims', C.c_int32 * 3),
        ('mlp3_dims', C.c_int32 * 4), ('model', C.c_int32), ('interaction_dims', C.c_int32 * 4),
        ('constant_velocity_model', C.c_int32), ('precision', C.c_int32),
    ]


# name -> (restype, argtypes); every symbol include/crowdnav_amd.h declares
_P = C.c_void_p
SYMBOLS = {
    'cn_last_error': (C.c_char_p, []),
    'cn_abi_version': (C.c_int, []),
    'cn_create': (C.c_int, [C.POINTER(CnConfig), C.POINTER(_P)]),
    'cn_destroy': (C.c_int, [_P]),
    'cn_set_stream': (C.c_int, [_P, _P]),
    'cn_sync': (C.c_int, [_P]),
    'cn_set_state': (C.c_int, [_P, _P, _P]),
    'cn_get_state': (C.c_int, [_P, _P, _P]),
    'cn_set_theta': (C.c_int, [_P, _P]),
    'cn_get_theta': (C.c_int, [_P, _P]),
    'cn_get_human_count': (C.c_int, [_P, _P]),
    'cn_drop_robot_sim': (C.c_int, [_P]),
    'cn_drop_sims': (C.c_int, [_P]),
    'cn_set_robot_sim': (C.c_int, [_P, _P, C.c_float]),
    'cn_reset': (C.c_int, [_P, _P, _P, _P]),
    'cn_orca': (C.c_int, [_P, _P]),
    'cn_step': (C.c_int, [_P, _P, C.c_int, _P, _P, _P, _P, _P, _P, _P]),
    'cn_set_gamma': (C.c_int, [_P, C.c_double]),
    'cn_rollout_begin': (C.c_int, [_P, C.POINTER(CnRolloutIo)]),
    'cn_rollout': (C.c_int, [_P, C.POINTER(CnRolloutIo), C.c_int]),
    'cn_rollout_step': (C.c_int, [_P, C.POINTER(CnRolloutIo), _P]),
    'cn_sarl_configure': (C.c_int, [_P, C.POINTER(CnSarlConfig), _P]),
    'cn_sarl_set_weights': (C.c_int, [_P, C.POINTER(_P)]),
    'cn_sarl_select': (C.c_int, [_P, _P, _P, _P]),
    'cn_sarl_select_attention': (C.c_int, [_P, _P, _P, _P, _P]),
    'cn_sarl_explore': (C.c_int, [_P, C.c_double, _P, _P, _P, _P]),
    'cn_sarl_transform': (C.c_int, [_P, _P, C.c_int64, C.c_int]),
    'cn_sarl_sample_step': (C.c_int, [_P, C.c_double, _P, _P, _P, _P, C.c_int64, C.c_int, _P, _P, _P, _P]),
    'cn_sarl_values': (C.c_int, [_P, _P, C.c_int64, _P]),
    'cn_sarl_export': (C.c_int, [_P, C.c_int, _P, C.c_uint64]),
    'cn_rollout_records': (C.c_int, [_P, C.POINTER(CnRolloutIo), C.c_int, _P]),
    'cn_gather_records': (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P]),
    'cn_records_summary': (C.c_int, [_P, C.c_int64, C.c_int, C.c_int, _P, _P]),
    'cn_rollout_summary': (C.c_int, [_P, C.POINTER(CnRolloutIo), _P]),
    'cn_launch_counts': (C.c_int, [_P, _P]),
    'cn_lagged_fills': (C.c_int, [_P, _P]),
    'cn_mt_random': (C.c_int, [_P, C.c_uint32, C.c_int, _P]),
    # two-wave rollout: first steps solved at fill time — counters, and a ring slot as the last fill left it (no version bump)
    'cn_fresh_starts': (C.c_int, [_P, _P]),
    'cn_ring_slot': (C.c_int, [_P, C.c_int, C.c_int, _P, _P, C.POINTER(C.c_int)]),
    # device SGD step (added after v12, no version bump)
    'cn_trainer_create': (C.c_int, [C.POINTER(CnSarlConfig), C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    'cn_trainer_destroy': (C.c_int, [_P]),
    'cn_trainer_set_stream': (C.c_int, [_P, _P]),
    'cn_train_step': (C.c_int, [_P, C.POINTER(_P), C.POINTER(_P), _P, _P, C.c_int64, _P, C.c_int64, C.c_double, C.c_double, _P]),
    'cn_trainer_steps': (C.c_int, [_P, C.POINTER(C.c_int64)]),
    # per-step record of a batched ORCA rollout (added after v12, no version bump)
    'cn_rollout_trace': (C.c_int, [_P, C.POINTER(CnRolloutIo), C.c_int, C.POINTER(CnTraceOut)]),
    # which transition kernel cn_rollout would launch (added after v12, no version bump)
    'cn_rollout_route': (C.c_int, [_P, C.c_int, C.POINTER(C.c_int)]),
    # which kernel family runs the value network (added after v12, no version bump)
    'cn_sarl_network_route': (C.c_int, [_P, C.POINTER(C.c_int)]),
    # n cn_rollout_step calls with a table of actions as one launch (added after v12, no version bump)
    'cn_rollout_actions': (C.c_int, [_P, C.POINTER(CnRolloutIo), C.c_int, _P, C.POINTER(CnTraceOut)]),
    # K candidate action sequences per env scored from the current state, engine untouched (no version bump)
    'cn_lookahead_actions': (C.c_int, [_P, C.c_int, C.c_int, _P, C.POINTER(CnLookaheadOut)]),
    # how the humans of a lookahead's branches move: ORCA (default) or constant velocity (no version bump)
    'cn_lookahead_set_human_model': (C.c_int, [_P, C.c_int]),
    'cn_lookahead_get_human_model': (C.c_int, [_P, C.POINTER(C.c_int)]),
    'cn_lookahead_set_goal_weight': (C.c_int, [_P, C.c_double]),
    'cn_lookahead_get_goal_weight': (C.c_int, [_P, C.POINTER(C.c_double)]),
    # V of joint states the caller holds in the env layout, and the lookahead that bootstraps with it (no version bump)
    'cn_sarl_state_values': (C.c_int, [_P, _P, _P, C.c_int64, C.c_int, _P]),
    'cn_lookahead_values': (C.c_int, [_P, C.c_int, C.c_int, _P, C.POINTER(CnLookaheadOut), C.c_int, _P, _P]),
    # device CEM planner: draw, score (through the two lookaheads), refit, step, shift (no version bump)
    'cn_plan_reset': (C.c_int, [_P, C.POINTER(CnPlanCfg), C.POINTER(CnPlan), _P]),
    'cn_plan_draw': (C.c_int, [_P, C.POINTER(CnPlanCfg), C.POINTER(CnPlan), C.c_uint32]),
    'cn_plan_refit': (C.c_int, [_P, C.POINTER(CnPlanCfg), C.POINTER(CnPlan), C.c_int]),
    'cn_plan_cem': (C.c_int, [_P, C.POINTER(CnPlanCfg), C.POINTER(CnPlan), C.c_uint32]),
    'cn_plan_shift': (C.c_int, [_P, C.POINTER(CnRolloutIo), C.POINTER(CnPlanCfg), C.POINTER(CnPlan)]),
    'cn_plan_rollout': (C.c_int, [_P, C.POINTER(CnRolloutIo), C.c_int, C.POINTER(CnPlanCfg), C.POINTER(CnPlan), C.c_uint32]),
    # device MPPI update beside the refit: softmax-weighted mean, the mean's first row as the action (no version bump)
    'cn_plan_mppi_update': (C.c_int, [_P, C.POINTER(CnPlanCfg), C.POINTER(CnPlan), C.c_double, C.c_int, C.c_int]),
    'cn_plan_mppi': (C.c_int, [_P, C.POINTER(CnPlanCfg), C.POINTER(CnPlan), C.c_double, C.c_int, C.c_uint32]),
    'cn_plan_mppi_rollout': (C.c_int, [_P, C.POINTER(CnRolloutIo), C.c_int, C.POINTER(CnPlanCfg), C.POINTER(CnPlan), C.c_double,
                                       C.c_int, C.c_uint32]),
    # the lookaheads and the planning steps against caller-predicted human velocities [B][n][A - 1][2] (no version bump)
    'cn_lookahead_paths': (C.c_int, [_P, C.c_int, C.c_int, _P, _P, C.POINTER(CnLookaheadOut)]),
    'cn_lookahead_paths_values': (C.c_int, [_P, C.c_int, C.c_int, _P, _P, C.POINTER(CnLookaheadOut), C.c_int, _P, _P]),
    'cn_plan_cem_paths': (C.c_int, [_P, C.POINTER(CnPlanCfg), C.POINTER(CnPlan), _P, C.c_uint32]),
    'cn_plan_mppi_paths': (C.c_int, [_P, C.POINTER(CnPlanCfg), C.POINTER(CnPlan), _P, C.c_double, C.c_int, C.c_uint32]),
    # the lookahead and the planning steps against M predicted futures [B][M][n][A - 1][2], reduced per branch (no version bump)
    'cn_lookahead_modes': (C.c_int, [_P, C.c_int, C.c_int, _P, C.POINTER(CnPathModes), C.POINTER(CnModesOut)]),
    'cn_plan_cem_modes': (C.c_int, [_P, C.POINTER(CnPlanCfg), C.POINTER(CnPlan), C.POINTER(CnPathModes), C.c_uint32]),
    'cn_plan_mppi_modes': (C.c_int, [_P, C.POINTER(CnPlanCfg), C.POINTER(CnPlan), C.POINTER(CnPathModes), C.c_double, C.c_int,
                                     C.c_uint32]),
    # the shipped predictors on the device, and the closed loop that predicts, plans, steps and shifts in one call (no version bump)
    'cn_predict': (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(C.c_int32), _P]),
    'cn_plan_cem_predict_rollout': (C.c_int, [_P, C.POINTER(CnRolloutIo), C.c_int, C.POINTER(CnPlanCfg), C.POINTER(CnPlan),
                                              C.POINTER(CnPredictors), C.c_uint32]),
    'cn_plan_mppi_predict_rollout': (C.c_int, [_P, C.POINTER(CnRolloutIo), C.c_int, C.POINTER(CnPlanCfg), C.POINTER(CnPlan),
                                               C.POINTER(CnPredictors), C.c_double, C.c_int, C.c_uint32]),
    # ORCA among the humans, the robot unseen, as one slot of such a table; the closed loop with that slot (no version bump)
    'cn_predict_orca': (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P]),
    'cn_plan_cem_predict_orca_rollout': (C.c_int, [_P, C.POINTER(CnRolloutIo), C.c_int, C.POINTER(CnPlanCfg), C.POINTER(CnPlan),
                                                   C.POINTER(CnPredictors), C.c_int, C.c_uint32]),
    'cn_plan_mppi_predict_orca_rollout': (C.c_int, [_P, C.POINTER(CnRolloutIo), C.c_int, C.POINTER(CnPlanCfg), C.POINTER(CnPlan),
                                                    C.POINTER(CnPredictors), C.c_int, C.c_double, C.c_int, C.c_uint32]),
    # the ORCA predictor with the robot in sight on a table of actions; the closed loop on the plan's nominal sequence (no version bump)
    'cn_predict_orca_robot': (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, C.c_int64, _P]),
    'cn_plan_cem_predict_orca_nominal_rollout': (C.c_int, [_P, C.POINTER(CnRolloutIo), C.c_int, C.POINTER(CnPlanCfg),
                                                           C.POINTER(CnPlan), C.POINTER(CnPredictors), C.c_int, C.c_uint32]),
    'cn_plan_mppi_predict_orca_nominal_rollout': (C.c_int, [_P, C.POINTER(CnRolloutIo), C.c_int, C.POINTER(CnPlanCfg),
                                                            C.POINTER(CnPlan), C.POINTER(CnPredictors), C.c_int, C.c_double, C.c_int,
                                                            C.c_uint32]),
    # the planners on a unicycle engine: the rotation bound and the rotation deviation, which opt the engine in (no version bump)
    'cn_plan_set_unicycle': (C.c_int, [_P, C.c_double, C.c_double]),
    'cn_plan_get_unicycle': (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    # the ORCA predictor on M sets of hypothesised human goals [B][M][A - 1][2], and the sampler of such sets (no version bump)
    'cn_predict_orca_goals': (C.c_int, [_P, C.c_int, C.c_int, _P, _P]),
    'cn_goal_hypotheses': (C.c_int, [_P, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, C.c_uint64, C.c_uint32, _P]),
}
# exported for the tests and not declared in the header: the workgroup geometry an engine got (E, threads, LDS bytes, grid)
DEBUG_SYMBOLS = {
    'cn_debug_geometry': (C.c_int, [_P, C.POINTER(C.c_int)]),
}

_lib = None


def load():
    """dlopen the in-tree library and bind every declared symbol; raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            'crowdnav_amd: %s is missing. Build the HIP library first (make -C crowdnav_amd/csrc, or '
            '__graft_entry__.build()); there is no CPU fallback.' % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in list(SYMBOLS.items()) + list(DEBUG_SYMBOLS.items()):
        fn = getattr(lib, name)  # AttributeError if the library does not export it
        fn.restype = res
        fn.argtypes = args
    got = lib.cn_abi_version()
    if got != ABI_VERSION:
        raise ImportError('crowdnav_amd: library ABI %d != binding ABI %d; rebuild' % (got, ABI_VERSION))
    _lib = lib
    return lib


def check(status):
    if status != CN_OK:
        raise CrowdNavAmdError(status, load().cn_last_error().decode('utf-8', 'replace'))
