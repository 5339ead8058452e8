"""Lookahead under predicted human motion without a GPU: the C-ABI surface (declared, bound, exported, no version bump, no
struct touched), the refusals that need no engine (made with pointers that address nothing: a refusal reads none of them), the
predict.* tables against hand-computed ones, and the host restatement (lookahead_paths_reference.py) on a crafted two-step
case whose outcome can be worked out by hand."""
import ctypes as C
import inspect
import math
import os

import numpy as np
import pytest

from conftest import ROOT

import lookahead_cv_reference as cv
import lookahead_paths_reference as ref
from support import built, DANGLING, filled  # noqa: F401  (built: module fixture)

DECLARATIONS = ('''int cn_lookahead_paths(cn_engine* e, int n_steps, int n_candidates,
                       const double* actions   /* [B][K][n][2] */,
                       const double* human_vel /* [B][n][A-1][2] */,
                       const cn_lookahead_out* out);''',
                '''int cn_lookahead_paths_values(cn_engine* e, int n_steps, int n_candidates, const double* actions,
                              const double* human_vel, const cn_lookahead_out* out,
                              int sort_humans, float* value, double* score);''',
                '''int cn_plan_cem_paths (cn_engine* e, const cn_plan_cfg* cfg, const cn_plan* plan,
                       const double* human_vel, uint32_t counter);''',
                '''int cn_plan_mppi_paths(cn_engine* e, const cn_plan_cfg* cfg, const cn_plan* plan,
                       const double* human_vel, double temperature, int fit_std, uint32_t counter);''')
NAMES = ('cn_lookahead_paths', 'cn_lookahead_paths_values', 'cn_plan_cem_paths', 'cn_plan_mppi_paths')


def test_header_binding_and_library_agree(built):
    text = open(os.path.join(ROOT, 'include', 'crowdnav_amd.h')).read()
    for decl in DECLARATIONS:
        assert decl in text, decl
    assert text.index('Lookahead human model') < text.index('Lookahead under predicted human motion') < text.index(
        'Value-bootstrapped lookahead')
    assert '#define CN_ABI_VERSION 12' in text and '#define CN_LAUNCH_COUNTERS 6' in text
    P, out, cfg, plan = C.c_void_p, C.POINTER(built.CnLookaheadOut), C.POINTER(built.CnPlanCfg), C.POINTER(built.CnPlan)
    assert built.SYMBOLS['cn_lookahead_paths'] == (C.c_int, [P, C.c_int, C.c_int, P, P, out])
    assert built.SYMBOLS['cn_lookahead_paths_values'] == (C.c_int, [P, C.c_int, C.c_int, P, P, out, C.c_int, P, P])
    assert built.SYMBOLS['cn_plan_cem_paths'] == (C.c_int, [P, cfg, plan, P, C.c_uint32])
    assert built.SYMBOLS['cn_plan_mppi_paths'] == (C.c_int, [P, cfg, plan, P, C.c_double, C.c_int, C.c_uint32])
    raw = C.CDLL(built.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
    assert built.HUMAN_MODELS == ('orca', 'constant_velocity')
    assert built.load().cn_abi_version() == 12 == built.ABI_VERSION and len(built.LAUNCH_COUNTERS) == 6
    assert C.sizeof(built.CnLookaheadOut) == 48 and C.sizeof(built.CnPlanCfg) == 56 and C.sizeof(built.CnPlan) == 120


def _out(built, **null):
    return filled(built.CnLookaheadOut, DANGLING, **dict.fromkeys(null))


def test_lookahead_refusals_that_need_no_engine(built):
    lib = built.load()
    ok, n, K = _out(built), 4, 3

    def refused(call, args, word, status=built.CN_ERR_INVALID):
        assert call(*args) == status, (args, lib.cn_last_error())
        assert word in lib.cn_last_error().decode(), lib.cn_last_error()

    for name, tail in (('cn_lookahead_paths', ()), ('cn_lookahead_paths_values', (0, DANGLING, DANGLING))):
        call = getattr(lib, name)
        # NULL human_vel first: before the NULL actions, the NULL out, the negative n_steps and the NULL engine beside it
        refused(call, (None, -1, 0, None, None, None) + tail, name + ': human_vel is NULL')
        refused(call, (None, n, K, DANGLING, None, C.byref(ok)) + tail, name + ': human_vel is NULL')
        # then cn_lookahead_check's, in its order and with its messages
        refused(call, (None, -1, 0, None, DANGLING, None) + tail, 'cn_lookahead_actions: actions is NULL')
        refused(call, (None, -1, 0, DANGLING, DANGLING, None) + tail, 'cn_lookahead_actions: out is NULL')
        for field in ('ret', 'info', 'steps', 'time'):
            first = {k: None for k in ('ret', 'info', 'steps', 'time')[('ret', 'info', 'steps', 'time').index(field):]}
            refused(call, (None, -1, 0, DANGLING, DANGLING, C.byref(_out(built, **first))) + tail,
                    'cn_lookahead_actions: out->%s is NULL' % field)
        refused(call, (None, -1, 0, DANGLING, DANGLING, C.byref(ok)) + tail, 'n_steps must be >= 0 (got -1)')
        refused(call, (None, n, 0, DANGLING, DANGLING, C.byref(ok)) + tail, 'n_candidates must be >= 1 (got 0)')
        # the NULL engine, last of what needs no engine (n_steps == 0 included: the checks come before the no-op)
        refused(call, (None, n, K, DANGLING, DANGLING, C.byref(ok)) + tail, 'cn_lookahead_actions: engine is NULL')
        refused(call, (None, 0, K, DANGLING, DANGLING, C.byref(ok)) + tail, 'cn_lookahead_actions: engine is NULL')


def test_plan_refusals_that_need_no_engine(built):
    lib = built.load()
    cfg = built.CnPlanCfg(n_steps=4, n_candidates=5, n_elites=2, iterations=1, bootstrap=0, sort_humans=0, init_std=0.3,
                          min_std=0.0, smoothing=0.0, seed=1)
    plan = built.CnPlan(mean=DANGLING, std=DANGLING, best_actions=DANGLING, best_score=DANGLING, action=DANGLING,
                        candidates=DANGLING, look=_out(built), value=DANGLING, score=DANGLING, order=DANGLING)
    no_mean = built.CnPlan(mean=None, std=DANGLING, best_actions=DANGLING, best_score=DANGLING, action=DANGLING,
                           candidates=DANGLING, look=_out(built), value=DANGLING, score=DANGLING, order=DANGLING)
    calls = {'cn_plan_cem_paths': lambda c, p, v, temperature=0.7: lib.cn_plan_cem_paths(None, c, p, v, 21),
             'cn_plan_mppi_paths': lambda c, p, v, temperature=0.7: lib.cn_plan_mppi_paths(None, c, p, v, temperature, 0, 21)}
    for name, call in calls.items():
        for args, word in (((None, None, None), name + ': human_vel is NULL'),
                           ((C.byref(cfg), C.byref(plan), None), name + ': human_vel is NULL'),
                           ((None, C.byref(plan), DANGLING), name + ': cfg is NULL'),
                           ((C.byref(cfg), None, DANGLING), name + ': plan is NULL'),
                           ((C.byref(cfg), C.byref(no_mean), DANGLING), name + ': plan->mean is NULL'),
                           ((C.byref(cfg), C.byref(plan), DANGLING), name + ': engine is NULL')):
            assert call(*args) == built.CN_ERR_INVALID, (name, word)
            assert word in lib.cn_last_error().decode(), lib.cn_last_error()
        few = built.CnPlanCfg.from_buffer_copy(cfg)
        few.n_candidates = 1
        assert call(C.byref(few), C.byref(plan), DANGLING) == built.CN_ERR_INVALID
        assert name + ': n_candidates must be >= 2 (got 1)' in lib.cn_last_error().decode()
    assert calls['cn_plan_mppi_paths'](C.byref(cfg), C.byref(plan), DANGLING, temperature=0.0) == built.CN_ERR_INVALID
    assert 'cn_plan_mppi_paths: temperature' in lib.cn_last_error().decode()


def test_the_python_surface_exists(built):
    from crowdnav_amd import predict
    from crowdnav_amd.compat.crowd_sim import CrowdSim
    from crowdnav_amd.engine import BatchedCrowdSim
    params = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert params(BatchedCrowdSim.lookahead_paths) == ['self', 'actions', 'human_vel', 'final_state', 'out', 'bootstrap', 'sort_humans']
    assert params(BatchedCrowdSim.lookahead) == ['self', 'actions', 'final_state', 'out', 'bootstrap', 'sort_humans']
    assert params(BatchedCrowdSim.plan_cem_paths) == ['self', 'plan', 'human_vel', 'counter']
    assert params(BatchedCrowdSim.plan_mppi_paths) == ['self', 'plan', 'human_vel', 'temperature', 'counter', 'fit_std']
    assert inspect.signature(BatchedCrowdSim.plan_mppi_paths).parameters['fit_std'].default is False
    assert params(CrowdSim.lookahead_paths) == ['self', 'sequences', 'human_velocities', 'policy']
    assert params(CrowdSim.lookahead) == ['self', 'sequences', 'policy', 'human_model']
    assert not hasattr(BatchedCrowdSim, 'plan_rollout_paths') and not hasattr(BatchedCrowdSim, 'plan_cem_paths_rollout')
    assert params(predict.constant_velocity) == ['state8', 'n'] and params(predict.to_goal) == ['state8', 'n', 'dt']
    assert params(predict.from_positions) == ['start_xy', 'positions', 'dt']
    eng = BatchedCrowdSim.__new__(BatchedCrowdSim)  # no device: the shapes are checked before the library is asked
    eng.B, eng.H, eng.A = 2, 3, 4
    with pytest.raises(ValueError, match='human_vel must be'):
        eng.lookahead_paths(np.zeros((2, 5, 4, 2)), np.zeros((2, 3, 3, 2)))  # n = 3 rows for n = 4 actions
    with pytest.raises(ValueError, match='actions must be'):
        eng.lookahead_paths(np.zeros((2, 5, 4, 3)), np.zeros((2, 4, 3, 2)))


# ---------------------------------------------------------------------------------------- predict.*
def _state():
    """One env: the robot, human 1 moving at (0.5, 0.25) with its goal 1.0 to the right, human 2 with its goal 0.625 below."""
    return np.array([[[0.0, -3.0, 0.0, 0.0, 0.0, 3.0, 0.3, 1.0],
                      [0.0, 0.0, 0.5, 0.25, 1.0, 0.0, 0.3, 1.0],
                      [2.0, 0.0, -1.0, 0.0, 2.0, -0.625, 0.3, 1.0]]])


def test_predict_constant_velocity():
    import torch
    from crowdnav_amd import predict
    got = predict.constant_velocity(_state(), 3)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (1, 3, 2, 2)
    assert got.tolist() == [[[[0.5, 0.25], [-1.0, 0.0]]] * 3]
    assert predict.constant_velocity(_state(), 0).shape == (1, 0, 2, 2)
    as_torch = predict.constant_velocity(torch.from_numpy(_state()), 3)
    assert torch.is_tensor(as_torch) and as_torch.dtype == torch.float64 and as_torch.is_contiguous()
    assert np.array_equal(as_torch.numpy(), got)
    with pytest.raises(ValueError):
        predict.constant_velocity(np.zeros((3, 8)), 2)


def test_predict_to_goal_stops_at_the_goal():
    from crowdnav_amd import predict
    got = predict.to_goal(_state(), 6, 0.25)
    assert got.dtype == np.float64 and got.shape == (1, 6, 2, 2)
    # human 1: 1.0 to go at speed 1, 0.25 per step: four full steps (the fourth lands on the goal), then it stands
    assert got[0, :, 0].tolist() == [[1.0, 0.0]] * 4 + [[0.0, 0.0]] * 2
    # human 2: 0.625 to go: two full steps down, a third shortened to the 0.125 left (speed 0.5), then it stands
    assert got[0, :, 1].tolist() == [[0.0, -1.0], [0.0, -1.0], [0.0, -0.5], [0.0, 0.0], [0.0, 0.0], [0.0, 0.0]]
    # a human at its goal never moves; a diagonal goal is approached at v_pref, not at v_pref per axis
    state = _state()
    state[0, 1, 4:6] = state[0, 1, 0:2]
    state[0, 2, 0:2], state[0, 2, 4:6], state[0, 2, 7] = (0.0, 0.0), (3.0, 4.0), 0.5
    got = predict.to_goal(state, 2, 0.25)
    assert got[0, :, 0].tolist() == [[0.0, 0.0]] * 2
    assert got[0, 0, 1].tolist() == [3.0 / 5.0 * 0.5, 4.0 / 5.0 * 0.5]
    assert math.hypot(*got[0, 1, 1]) == pytest.approx(0.5, abs=1e-15)


def test_predict_from_positions():
    from crowdnav_amd import predict
    start = np.array([[[0.0, 0.0], [1.0, 1.0]]])
    positions = np.array([[[[0.25, 0.0], [1.0, 1.0]], [[0.25, 0.5], [0.5, 1.0]], [[0.25, 0.5], [0.5, 1.0]]]])
    got = predict.from_positions(start, positions, 0.25)
    assert got.dtype == np.float64 and got.shape == (1, 3, 2, 2)
    assert got.tolist() == [[[[1.0, 0.0], [0.0, 0.0]], [[0.0, 2.0], [-2.0, 0.0]], [[0.0, 0.0], [0.0, 0.0]]]]
    with pytest.raises(ValueError):
        predict.from_positions(start[:, :1], positions, 0.25)
    # to_goal's table carries the humans where it says: positions -> velocities -> the same table
    table = predict.to_goal(_state(), 6, 0.25)
    walked = _state()[:, 1:, 0:2][:, None] + np.cumsum(table * 0.25, axis=1)  # (exact: every term is a multiple of 2^-3)
    assert np.array_equal(predict.from_positions(_state()[:, 1:, 0:2], walked, 0.25), table)


# ---------------------------------------------------------------------------------------- the restatement, two steps
def _scene():
    """The robot stands at the origin (goal 4 above it); one human 1.5 to its right, walking up."""
    return [[0.0, 0.0, 0.0, 0.0, 0.0, 4.0, 0.3, 1.0], [1.5, 0.0, 0.0, 1.0, 1.5, 4.0, 0.3, 1.0]]


def test_a_human_that_turns_between_the_steps():
    wait = [(0.0, 0.0), (0.0, 0.0)]
    table = cv.discount_table(0.9, ref.CFG)
    # the table repeats the state velocity: the constant-velocity branch, which passes 1.5 away
    straight = ref.branch(_scene(), 0.0, wait, [[(0.0, 1.0)], [(0.0, 1.0)]])
    want = cv.branch(_scene(), 0.0, wait)
    assert straight == want
    assert (straight['infos'], straight['steps']) == ([ref.NOTHING, ref.NOTHING], 2)
    assert straight['final_state8'][1][:4] == [1.5, 0.5, 0.0, 1.0]
    # the human turns: it chooses (-4, -1) from the first step on.  Step 0 is swept with the velocity it HAS, (0, 1) — nothing —
    # and moves it to (0.5, -0.25), 0.56 from the robot's centre with 0.6 needed; step 1, swept with (-4, -1), sees the collision
    turned = ref.branch(_scene(), 0.0, wait, [[(-4.0, -1.0)], [(-4.0, -1.0)]])
    assert (turned['infos'], turned['steps'], turned['time']) == ([ref.NOTHING, ref.COLLISION], 2, 0.5)
    assert turned['ret'] == (0.0 + table[0] * 0.0) + table[1] * -0.25
    # final_state8: the position after the last step, the velocity OF the last step; goal, radius and v_pref copied through
    assert turned['final_state8'][1] == [-0.5, -0.5, -4.0, -1.0, 1.5, 4.0, 0.3, 1.0]
    assert turned['final_state8'][0][:4] == [0.0, 0.0, 0.0, 0.0]
    # a turn between the steps — (0, 1), then (-4, -1) to (0.5, 0) — moves the human in step 1 and is swept in step 2, as a
    # turn of an ORCA human is (step_core reads the velocity of the step before): two steps pass, the third collides
    late = ref.branch(_scene(), 0.0, wait + [(0.0, 0.0)], [[(0.0, 1.0)], [(-4.0, -1.0)], [(0.0, 0.0)]])
    assert late['infos'] == [ref.NOTHING, ref.NOTHING, ref.COLLISION] and late['steps'] == 3
    assert late['final_state8'][1][:4] == [0.5, 0.0, 0.0, 0.0]
    assert ref.branch(_scene(), 0.0, wait, [[(0.0, 1.0)], [(-4.0, -1.0)]])['final_state8'][1][:4] == [0.5, 0.0, -4.0, -1.0]
    # the state velocity is read by the first swept test and by nothing else: a human that HAS (-4, 0) is seen crossing the robot
    # in step 0 although the table walks it straight up
    other = _scene()
    other[1][2:4] = [-4.0, 0.0]
    seen = ref.branch(other, 0.0, wait, [[(0.0, 1.0)], [(0.0, 1.0)]])
    assert (seen['infos'], seen['steps']) == ([ref.COLLISION], 1) and seen['final_state8'][1][:4] == [1.5, 0.25, 0.0, 1.0]
    # rows behind the end are not read
    nan = (math.nan, math.nan)
    assert ref.branch(_scene(), 0.0, wait + [nan], [[(-4.0, -1.0)], [(-4.0, -1.0)], [nan]]) == turned


def test_lookahead_shapes_of_the_restatement():
    state = np.array([_scene(), _scene()])
    actions = np.zeros((2, 3, 2, 2))
    vel = np.array([[[(0.0, 1.0)], [(0.0, 1.0)]], [[(-4.0, -1.0)], [(-4.0, -1.0)]]])
    got = ref.lookahead(state, [0.0, 0.0], actions, vel)
    assert got['info'].tolist() == [[ref.NOTHING] * 3, [ref.COLLISION] * 3] and got['final_state8'].shape == (2, 3, 2, 8)
    same = cv.lookahead(state[:1], [0.0], actions[:1])
    for key in ('ret', 'info', 'steps', 'time', 'final_state8'):
        assert np.array_equal(got[key][:1], same[key]), key
