"""The unicycle planners without a GPU: the C-ABI surface (two new symbols declared, bound and exported; no version bump, no
struct or counter touched), the setter's refusals that need no engine, the Python surface, the example parsers, and the host
restatement (plan_unicycle_reference.py) on rows worked out by hand: the clip, the prior's recurrence and its wrap."""
import ctypes as C
import importlib.util
import math
import os

import numpy as np
import pytest

from conftest import ROOT

import plan_unicycle_cases as cases
import plan_unicycle_reference as uni
from support import built  # noqa: F401  (built: module fixture)

DECLARATIONS = ('int cn_plan_set_unicycle(cn_engine* e, double max_rotation, double init_std_rotation);',
                'int cn_plan_get_unicycle(cn_engine* e, double* max_rotation, double* init_std_rotation);')
PI = math.pi


# ------------------------------------------------------------------------------------------------ the surface
def test_header_binding_and_library_agree(built):
    text = open(os.path.join(ROOT, 'include', 'crowdnav_amd.h')).read()
    for decl in DECLARATIONS:
        assert decl in text, decl
    assert 'Unicycle planners' in text
    assert '#define CN_ABI_VERSION 12' in text and '#define CN_LAUNCH_COUNTERS 6' in text
    assert built.SYMBOLS['cn_plan_set_unicycle'] == (C.c_int, [C.c_void_p, C.c_double, C.c_double])
    assert built.SYMBOLS['cn_plan_get_unicycle'] == (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)])
    raw = C.CDLL(built.LIB_PATH)
    assert hasattr(raw, 'cn_plan_set_unicycle') and hasattr(raw, 'cn_plan_get_unicycle')
    assert built.load().cn_abi_version() == 12 == built.ABI_VERSION and len(built.LAUNCH_COUNTERS) == 6
    assert C.sizeof(built.CnPlanCfg) == 56 and C.sizeof(built.CnPlan) == 120


@pytest.mark.parametrize('R, S', [(PI / 4, 0.3), (math.nan, 0.3), (-1.0, 0.3), (4.0, 0.3), (PI / 4, math.nan), (PI / 4, 0.0)])
def test_the_null_engine_is_refused_first(built, R, S):
    # the header's order: NULL engine, then max_rotation, then init_std_rotation, then the engine's kind — so without an engine
    # every argument, good or bad, meets the first refusal (the others need a device: tests/test_plan_unicycle.py)
    lib = built.load()
    assert lib.cn_plan_set_unicycle(None, R, S) == built.CN_ERR_INVALID
    assert 'cn_plan_set_unicycle: engine is NULL' in lib.cn_last_error().decode()


def test_the_getter_refuses_null(built):
    lib = built.load()
    r, s = C.c_double(7.0), C.c_double(8.0)
    assert lib.cn_plan_get_unicycle(None, C.byref(r), C.byref(s)) == built.CN_ERR_INVALID
    assert 'cn_plan_get_unicycle: engine is NULL' in lib.cn_last_error().decode() and (r.value, s.value) == (7.0, 8.0)
    assert lib.cn_plan_get_unicycle(None, None, None) == built.CN_ERR_INVALID


def test_the_python_surface_exists(built):
    from crowdnav_amd.engine import BatchedCrowdSim as E
    assert callable(E.set_plan_unicycle) and isinstance(E.plan_unicycle, property) and E.plan_unicycle.fset is None
    for f in (E.plan_begin, E.plan_reset, E.plan_draw, E.plan_shift, E.plan_mppi_update):
        assert 'set_plan_unicycle' in f.__doc__ and '(v, r)' in f.__doc__, f.__name__
    for path in ('crowdnav_amd/csrc/plan_kernels.h', 'crowdnav_amd/csrc/plan.hip', 'crowdnav_amd/engine.py', 'include/crowdnav_amd.h'):
        assert 'olonomic external robots only' not in open(os.path.join(ROOT, path)).read(), path


def _example(name):
    spec = importlib.util.spec_from_file_location('example_' + name, os.path.join(ROOT, 'examples', name + '.py'))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


@pytest.mark.parametrize('name, extra', [('shooting_planner', ['--cem', '--human-model', 'constant_velocity']),
                                         ('shooting_planner', ['--mppi', '--goal-weight', '0.1']),
                                         ('predicted_paths_planner', ['--futures', 'to_goal,orca', '--device-loop', '--orca-sees-plan'])])
def test_the_example_parsers_accept_the_flags(built, name, extra):
    ap = _example(name).parser()
    args = ap.parse_args(extra)
    assert args.kinematics == 'holonomic' and args.max_rotation == PI / 4 and args.rotation_std > 0
    args = ap.parse_args(extra + ['--kinematics', 'unicycle', '--max-rotation', '0.5', '--rotation-std', '0.2'])
    assert (args.kinematics, args.max_rotation, args.rotation_std) == ('unicycle', 0.5, 0.2)
    with pytest.raises(SystemExit):
        ap.parse_args(['--kinematics', 'tricycle'])


# ------------------------------------------------------------------------------------------------ the clip, by hand
def test_clip_on_crafted_rows():
    R = PI / 4
    rows = np.array([[-0.2, 0.1], [1.5, -0.1], [0.5, 2.0], [0.5, -2.0], [-3.0, 9.0], [0.3, 0.7], [0.0, -R], [1.0, R], [-0.0, 0.0]])
    got = uni.clip(rows, 1.0, R)
    want = np.array([[0.0, 0.1], [1.0, -0.1], [0.5, R], [0.5, -R], [0.0, R], [0.3, 0.7], [0.0, -R], [1.0, R], [-0.0, 0.0]])
    assert got.tobytes() == want.tobytes()  # a row inside the box, its edges included, keeps its bits (the sign of -0.0 too)
    assert uni.clip(rows, 0.25, 0.1).max(axis=0).tolist() == [0.25, 0.1]
    per_env = uni.clip(np.full((2, 3, 2), 5.0), np.array([0.5, 2.0])[:, None], R)  # v_pref per env
    assert (per_env[0] == [0.5, R]).all() and (per_env[1] == [2.0, R]).all()


def test_draw_candidate_zero_is_the_clipped_mean_and_rows_stay_in_the_box():
    mean = np.array([[[0.4, 0.2], [1.7, -3.0]], [[-0.5, 0.05], [0.9, 0.0]]])
    std = np.full((2, 2, 2), 0.8)
    for R in cases.ROTATIONS:
        cand = uni.draw(mean, std, 70, 5, 3, 1.0, R)
        assert cand[:, 0].tobytes() == uni.clip(mean, 1.0, R).tobytes()
        assert cand[..., 0].min() == 0.0 and cand[..., 0].max() == 1.0 and cand[..., 1].min() == -R and cand[..., 1].max() == R
        assert uni.draw(mean, np.zeros_like(std), 5, 5, 3, 1.0, R).tobytes() == np.repeat(cand[:, :1], 5, axis=1).tobytes()
    assert uni.draw(mean, std, 70, 5, 3, 1.0, 0.1)[:, :9].tobytes() == uni.draw(mean, std, 9, 5, 3, 1.0, 0.1).tobytes()


# ------------------------------------------------------------------------------------------------ the prior, by hand
def test_prior_facing_the_goal_drives_straight():
    rows = uni.prior_rows(-4.0, 0.0, 4.0, 0.0, 1.0, 0.0, 0.25, PI / 4, 8)  # along +x: cos = 1 and sin = 0 exactly
    assert rows.tobytes() == np.tile([1.0, 0.0], (8, 1)).tobytes()
    rows = uni.prior_rows(0.0, -4.0, 0.0, 4.0, 1.0, PI / 2, 0.25, PI / 4, 8)  # the scenario generator's start
    assert (rows[:, 0] == 1.0).all() and np.abs(rows[:, 1]).max() < 1e-15


@pytest.mark.parametrize('R', [PI / 4, 0.5])  # (at a small R the robot drives metres while it turns, and the bearing with it)
def test_prior_at_ninety_degrees_turns_then_drives(R):
    k = math.ceil((PI / 2) / R)
    rows = uni.prior_rows(0.0, -4.0, 0.0, 4.0, 1.0, 0.0, 0.25, R, k + 6)
    turning = int(np.argmin(rows[:, 1] == R))  # leading rows at the bound
    # ceil((pi / 2) / R) turning rows; the robot drives while it turns, so the bearing moves a little further left and the
    # last of them may or may not reach the bound
    assert k - 1 <= turning <= k, (turning, k)
    assert (rows[:, 0] == 1.0).all() and (np.abs(rows[turning + 1:, 1]) < R / 4).all() and (rows[:, 1] > -R / 4).all()
    assert abs(rows[:, 1].sum() - PI / 2) < 0.1  # the heading ends on the bearing, which has moved by less than 0.1 rad


def test_prior_reaches_a_near_goal_in_one_step_and_stops():
    rows = uni.prior_rows(-0.1, 0.0, 0.0, 0.0, 1.0, 0.0, 0.25, PI / 4, 4)
    assert rows.tolist() == [[0.1 / 0.25, 0.0], [0.0, 0.0], [0.0, 0.0], [0.0, 0.0]]  # speed = dist / dt; then dist == 0 exactly
    assert not uni.prior_rows(1.5, -2.0, 1.5, -2.0, 1.0, 0.7, 0.25, PI / 4, 5).any()  # dist == 0 from the start


def test_the_wrap_on_both_sides_of_pi():
    eps = 1e-6
    assert uni.wrap(0.0) == 0.0 and uni.wrap(1.0) == 1.0 and uni.wrap(-1.0) == -1.0
    assert uni.wrap(PI - eps) == PI - eps and abs(uni.wrap(PI + eps) - (-PI + eps)) < 1e-15
    assert uni.wrap(-PI + eps) == -PI + eps and abs(uni.wrap(-PI - eps) - (PI - eps)) < 1e-15
    assert uni.wrap(-PI) == -PI and uni.wrap(PI) == -PI  # [-pi, pi)
    assert abs(uni.wrap(6.0) - (6.0 - 2 * PI)) < 1e-15 and abs(uni.wrap(-6.0) - (2 * PI - 6.0)) < 1e-15
    # in the recurrence: heading -3, goal at bearing +3 — 6 rad to the left, 0.283 rad to the right: the robot turns right
    rows = uni.prior_rows(0.0, 0.0, 10 * math.cos(3.0), 10 * math.sin(3.0), 1.0, -3.0, 0.25, PI / 4, 2)
    assert abs(rows[0, 1] - (6.0 - 2 * PI)) < 1e-12 and abs(rows[1, 1]) < 1e-2
    # just past pi behind on either hand: the turn takes the side the goal is on, at the bound
    assert uni.prior_rows(0.0, 0.0, -10.0, 1e-3, 1.0, 0.0, 0.25, 0.3, 1)[0, 1] == 0.3
    assert uni.prior_rows(0.0, 0.0, -10.0, -1e-3, 1.0, 0.0, 0.25, 0.3, 1)[0, 1] == -0.3


def test_the_gpu_cases_keep_their_turns_away_from_pi():
    state8, theta = cases.install(np.zeros((3, 6, 8)) + [0, 0, 0, 0, 0, 0, 0.3, cases.V_PREF])
    reseed = np.array([[0.0, -4.0, 0.0, 4.0, cases.RESEED_THETA]] * 3)
    for robots_state, th in ((state8, theta), cases.install(state8, reseed)):
        for R in cases.ROTATIONS:
            turns = []
            rows = uni.prior(robots_state, th, cases.DT, R, cases.N, turns)
            assert len(turns) >= cases.N and min(PI - abs(t) for t in turns) >= cases.TURN_MARGIN, (R, max(abs(t) for t in turns))
            assert rows.shape == (3, cases.N, 2) and (rows[..., 0] <= cases.V_PREF).all() and (np.abs(rows[..., 1]) <= R).all()
    clipped = uni.prior(state8, theta, cases.DT, 0.1, cases.N)
    assert (np.abs(clipped[1, :10, 1]) == 0.1).all()  # case 1 turns at the bound for many steps
    near = uni.prior(state8, theta, cases.DT, PI / 4, cases.N)
    assert (near[2, :, 0] < cases.V_PREF).any()  # case 2 meets speed = dist / dt


def test_reset_shift_and_mppi_action_on_copies():
    state8, theta = cases.install(np.zeros((3, 6, 8)) + [0, 0, 0, 0, 0, 0, 0.3, 1.0])
    mean0, std0 = np.full((3, 4, 2), 7.0), np.full((3, 4, 2), 9.0)
    mean, std = uni.reset(state8, theta, 0.25, 0.5, mean0, std0, 0.3, 0.2, mask=[1, 0, 1])
    assert (mean[1] == 7.0).all() and (std[1] == 9.0).all() and (std[0] == [0.3, 0.2]).all() and (mean0 == 7.0).all()
    assert mean[0].tobytes() == uni.prior_rows(0.0, -4.0, 0.0, 4.0, 1.0, PI / 2, 0.25, 0.5, 4).tobytes()
    walk = np.arange(24.0).reshape(3, 4, 2)
    mean, std = uni.shift(state8, theta, 0.25, 0.5, [1, 1, 0], [3, 0, 0], walk, std0, 0.3, 0.2)
    assert mean[0].tolist() == [[2, 3], [4, 5], [6, 7], [6, 7]] and (std[0] == [0.3, 0.2]).all()  # shifted, the last row stays
    assert mean[1].tobytes() == uni.prior(state8, theta, 0.25, 0.5, 4)[1].tobytes() and (std[1] == [0.3, 0.2]).all()  # re-seeded
    assert mean[2].tobytes() == walk[2].tobytes() and (std[2] == 9.0).all()  # retired: untouched
    # the MPPI action: one candidate per env, so the updated mean is that candidate — outside the box, and clipped to it
    cand = np.array([[[[1.6, -2.0], [0.1, 0.1]]], [[[-0.4, 0.05], [0.1, 0.1]]]])
    out = uni.mppi_update(np.zeros((2, 1)), cand, np.zeros((2, 2, 2)), np.ones((2, 2, 2)), np.zeros((2, 2, 2)), np.zeros(2),
                          np.zeros((2, 2)), 1.0, False, False, 0.0, 0.0, 1.0, 0.5)
    assert out['mean'].tobytes() == cand[:, 0].tobytes() and out['action'].tolist() == [[1.0, -0.5], [0.0, 0.05]]
