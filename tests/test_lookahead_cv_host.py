"""The lookahead human model without a GPU: the C-ABI surface (declared, bound, exported, no version bump, no struct touched),
the refusals that need no engine, and the host restatement of a constant-velocity branch (lookahead_cv_reference.py) on
crafted single steps whose outcome can be worked out by hand."""
import ctypes as C
import math
import os

import pytest

from conftest import ROOT

import lookahead_cv_reference as ref
from lookahead_cv_reference import human_row as _human, robot_row as _robot
from support import built  # noqa: F401  (built: module fixture)

DECLARATIONS = ('enum { CN_HUMANS_ORCA = 0, CN_HUMANS_CONSTANT_VELOCITY = 1 };',
                'int cn_lookahead_set_human_model(cn_engine* e, int model);',
                'int cn_lookahead_get_human_model(const cn_engine* e, int* model_host);')


def test_header_binding_and_library_agree(built):
    text = open(os.path.join(ROOT, 'include', 'crowdnav_amd.h')).read()
    for decl in DECLARATIONS:
        assert decl in text, decl
    assert 'Lookahead human model' in text
    assert '#define CN_ABI_VERSION 12' in text and '#define CN_LAUNCH_COUNTERS 6' in text
    assert built.SYMBOLS['cn_lookahead_set_human_model'] == (C.c_int, [C.c_void_p, C.c_int])
    assert built.SYMBOLS['cn_lookahead_get_human_model'] == (C.c_int, [C.c_void_p, C.POINTER(C.c_int)])
    raw = C.CDLL(built.LIB_PATH)
    assert hasattr(raw, 'cn_lookahead_set_human_model') and hasattr(raw, 'cn_lookahead_get_human_model')
    assert (built.HUMANS_ORCA, built.HUMANS_CONSTANT_VELOCITY) == (0, 1)
    assert built.HUMAN_MODELS == ('orca', 'constant_velocity')
    assert built.load().cn_abi_version() == 12 == built.ABI_VERSION and len(built.LAUNCH_COUNTERS) == 6
    assert C.sizeof(built.CnLookaheadOut) == 48 and C.sizeof(built.CnPlanCfg) == 56 and C.sizeof(built.CnPlan) == 120


def test_refusals_that_need_no_engine(built):
    lib = built.load()
    model = C.c_int(7)
    for m in (built.HUMANS_ORCA, built.HUMANS_CONSTANT_VELOCITY, 2, -1):
        assert lib.cn_lookahead_set_human_model(None, m) == built.CN_ERR_INVALID
        assert 'engine is NULL' in lib.cn_last_error().decode()
    assert lib.cn_lookahead_get_human_model(None, C.byref(model)) == built.CN_ERR_INVALID
    assert 'engine is NULL' in lib.cn_last_error().decode() and model.value == 7
    assert lib.cn_lookahead_get_human_model(None, None) == built.CN_ERR_INVALID
    # (a NULL model_host on a live engine needs a device to make the engine: test_lookahead_cv.py)


def test_the_python_surface_exists(built):
    import inspect
    from crowdnav_amd.compat.crowd_sim import CrowdSim
    from crowdnav_amd.engine import BatchedCrowdSim
    assert callable(BatchedCrowdSim.set_lookahead_human_model) and isinstance(BatchedCrowdSim.lookahead_human_model, property)
    assert BatchedCrowdSim.lookahead_human_model.fset is None
    assert list(inspect.signature(CrowdSim.lookahead).parameters) == ['self', 'sequences', 'policy', 'human_model']
    assert inspect.signature(CrowdSim.lookahead).parameters['human_model'].default is None
    eng = BatchedCrowdSim.__new__(BatchedCrowdSim)  # no device: the name is checked before the library is asked
    eng._h = None
    with pytest.raises(ValueError, match='human model'):
        eng.set_lookahead_human_model('linear')


# ---------------------------------------------------------------------------------------- the restatement, single steps
def test_norm2_is_the_fused_form():
    assert ref.norm2(3.0, 4.0) == 5.0 and ref.norm2(0.0, 0.0) == 0.0
    # x * x is rounded, y * y is not: y * y = 1 + 2^-26 + 2^-54 exactly, x * x = 1.5625 * 2^-54; unfused, y * y loses its
    # 2^-54 and the sum (0.39 ulp above) rounds down; fused, 2.5625 * 2^-54 = 0.64 ulp rounds up
    x, y = 1.25 * 2.0 ** -27, 1.0 + 2.0 ** -27
    fused = 1.0 + 2.0 ** -26 + 2.0 ** -52
    assert x * x + y * y == 1.0 + 2.0 ** -26 != fused
    assert ref.norm2(x, y) == math.sqrt(fused)


def test_head_on_collision():
    state = [_robot(), _human(0.8, 0.0, -1.0, 0.0)]
    reward, done, info, dmin = ref.transition(state, 0.0, (1.0, 0.0), ref.CFG)
    # relative motion 0.8 -> 0.3 along x: the discs (0.3 + 0.3) overlap
    assert (reward, done, info) == (-0.25, True, ref.COLLISION) and dmin == math.inf
    assert state[0][:4] == [0.25, 0.0, 1.0, 0.0] and state[1][:4] == [0.55, 0.0, -1.0, 0.0]  # both moved, the human at ITS velocity


def test_graze_inside_discomfort_dist():
    state = [_robot(), _human(0.7, 0.0)]
    reward, done, info, dmin = ref.transition(state, 0.0, (0.0, 1.0), ref.CFG)
    # the human stands: seen from the robot it moves (0.7, 0) -> (0.7, -0.25), closest at the start, 0.7 - 0.6 clear
    assert info == ref.DANGER and not done
    assert dmin == pytest.approx(0.1, abs=1e-15) and reward == pytest.approx((0.1 - 0.2) * 0.5 * 0.25, abs=1e-15)
    assert reward == (dmin - 0.2) * 0.5 * 0.25
    assert state[1][:2] == [0.7, 0.0]


def test_degenerate_zero_relative_motion():
    state = [_robot(), _human(1.0, 0.0, 0.5, 0.5)]
    reward, done, info, dmin = ref.transition(state, 0.0, (0.5, 0.5), ref.CFG)  # human and robot move alike: sx = sy = 0
    assert (reward, done, info) == (0.0, False, ref.NOTHING) and dmin == (1.0 - 0.3) - 0.3
    assert state[1][:2] == [1.125, 0.125] and state[0][:2] == [0.125, 0.125]


def test_timeout_comes_first():
    cfg = dict(ref.CFG, time_limit=8.0)
    state = [_robot(), _human(0.8, 0.0, -1.0, 0.0)]  # the head-on collision again
    assert ref.transition([row[:] for row in state], 6.75, (1.0, 0.0), cfg)[2] == ref.COLLISION
    reward, done, info, _ = ref.transition(state, 7.0, (1.0, 0.0), cfg)  # gtime = time_limit - 1
    assert (reward, done, info) == (0.0, True, ref.TIMEOUT)
    got = ref.branch([_robot(), _human(5.0, 5.0)], 6.5, [(0.0, 0.0)] * 6, cfg)
    assert (got['info'], got['steps'], got['time'], got['ret']) == (ref.TIMEOUT, 3, 7.25, 0.0)


def test_dmin_is_the_minimum_before_the_first_collision():
    near, hit, nearer = _human(0.0, -0.65), _human(0.5, 0.0), _human(0.0, -0.61)
    _, _, info, dmin = ref.transition([_robot(), near, hit, nearer], 0.0, (0.0, 0.0), ref.CFG)
    assert info == ref.COLLISION and dmin == (0.65 - 0.3) - 0.3  # the nearer one behind the hit is not looked at
    _, _, info, dmin = ref.transition([_robot(), hit, near], 0.0, (0.0, 0.0), ref.CFG)
    assert info == ref.COLLISION and dmin == math.inf
    _, _, info, dmin = ref.transition([_robot(), near, nearer], 0.0, (0.0, 0.0), ref.CFG)
    assert info == ref.DANGER and dmin == (0.61 - 0.3) - 0.3


def test_a_branch_books_left_to_right_and_stops_at_done():
    cfg = dict(ref.CFG)
    table = ref.discount_table(0.9, cfg)
    assert len(table) == 108 and table[0] == 1.0 and table[4] == math.pow(0.9, 4 * 0.25 * 1.0)
    # straight at a standing human 1.2 ahead: Danger steps, then the collision; the actions behind it are not read
    got = ref.branch([_robot(), _human(0.0, 1.2)], 0.0, [(0.0, 1.0)] * 3 + [(math.nan, math.nan)] * 3, cfg, table)
    assert got['infos'] == [ref.NOTHING, ref.DANGER, ref.COLLISION] and got['steps'] == 3 and got['time'] == 0.75
    d1 = (1.2 - 0.5) - 0.3 - 0.3
    assert got['ret'] == (0.0 + table[0] * 0.0 + table[1] * ((d1 - 0.2) * 0.5 * 0.25)) + table[2] * -0.25
    assert got['final_state8'][0][:2] == [0.0, 0.75]
