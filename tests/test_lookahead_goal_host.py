"""The lookahead goal-progress term without a GPU: the C-ABI surface (declared, bound, exported, no version bump, no struct
touched), the refusals that need no engine, and the host restatement of the term (lookahead_goal_reference.py) on values worked
out by hand."""
import ctypes as C
import math
import os
from fractions import Fraction

import pytest

from conftest import ROOT

import lookahead_goal_reference as goal
from support import built  # noqa: F401  (built: module fixture)

DECLARATIONS = ('int cn_lookahead_set_goal_weight(cn_engine* e, double weight);',
                'int cn_lookahead_get_goal_weight(const cn_engine* e, double* weight_host);')


def test_header_binding_and_library_agree(built):
    text = open(os.path.join(ROOT, 'include', 'crowdnav_amd.h')).read()
    for decl in DECLARATIONS:
        assert decl in text, decl
    assert 'Lookahead goal-progress term' in text
    assert '#define CN_ABI_VERSION 12' in text and '#define CN_LAUNCH_COUNTERS 6' in text
    assert built.SYMBOLS['cn_lookahead_set_goal_weight'] == (C.c_int, [C.c_void_p, C.c_double])
    assert built.SYMBOLS['cn_lookahead_get_goal_weight'] == (C.c_int, [C.c_void_p, C.POINTER(C.c_double)])
    raw = C.CDLL(built.LIB_PATH)
    assert hasattr(raw, 'cn_lookahead_set_goal_weight') and hasattr(raw, 'cn_lookahead_get_goal_weight')
    assert built.load().cn_abi_version() == 12 == built.ABI_VERSION and len(built.LAUNCH_COUNTERS) == 6
    assert C.sizeof(built.CnLookaheadOut) == 48 and C.sizeof(built.CnPlanCfg) == 56 and C.sizeof(built.CnPlan) == 120


@pytest.mark.parametrize('bad, shown', [(math.nan, 'nan'), (math.inf, 'inf'), (-math.inf, '-inf'), (-1.0, '-1'),
                                        (-5e-324, '-4.94066e-324')])
def test_a_bad_weight_is_refused_before_the_null_engine(built, bad, shown):
    lib = built.load()
    assert lib.cn_lookahead_set_goal_weight(None, bad) == built.CN_ERR_INVALID
    msg = lib.cn_last_error().decode()
    assert 'cn_lookahead_set_goal_weight' in msg and 'weight must be' in msg and 'engine is NULL' not in msg
    assert ('got %s)' % shown) in msg.replace('-nan', 'nan'), msg


@pytest.mark.parametrize('fine', [0.0, -0.0, 0.1, 0.25, 1e300])
def test_a_good_weight_reaches_the_null_engine_refusal(built, fine):
    # -0.0 is not negative (IEEE: -0.0 < 0.0 is false): the header accepts it, it means 0.0
    lib = built.load()
    assert lib.cn_lookahead_set_goal_weight(None, fine) == built.CN_ERR_INVALID
    assert 'cn_lookahead_set_goal_weight: engine is NULL' in lib.cn_last_error().decode()


def test_the_getter_refuses_null(built):
    lib = built.load()
    w = C.c_double(7.0)
    assert lib.cn_lookahead_get_goal_weight(None, C.byref(w)) == built.CN_ERR_INVALID
    assert 'cn_lookahead_get_goal_weight: engine is NULL' in lib.cn_last_error().decode() and w.value == 7.0
    assert lib.cn_lookahead_get_goal_weight(None, None) == built.CN_ERR_INVALID
    assert 'cn_lookahead_get_goal_weight' in lib.cn_last_error().decode()
    # (a NULL weight_host on a live engine needs a device to make the engine: test_lookahead_goal.py)


def test_the_python_surface_exists(built):
    from crowdnav_amd.compat.crowd_sim import CrowdSim
    from crowdnav_amd.engine import BatchedCrowdSim
    for cls in (BatchedCrowdSim, CrowdSim):
        assert callable(cls.set_lookahead_goal_weight) and isinstance(cls.lookahead_goal_weight, property)
        assert cls.lookahead_goal_weight.fset is None
    for f in (BatchedCrowdSim.lookahead, BatchedCrowdSim.lookahead_paths, BatchedCrowdSim.lookahead_modes, BatchedCrowdSim.plan_begin):
        assert 'set_lookahead_goal_weight' in f.__doc__


# ---------------------------------------------------------------------------------------- the restatement, by hand
def test_goal_term_on_exact_values():
    # a 3-4-5 start 10 from the goal, an end 5 from it: every operation exact
    assert goal.goal_term(0.25, (6.0, 8.0), (0.0, 0.0), (3.0, 4.0)) == 0.25 * 5.0 == 1.25
    assert goal.goal_term(0.25, (3.0, 4.0), (0.0, 0.0), (6.0, 8.0)) == -1.25  # moving away costs as much
    assert goal.goal_term(0.5, (0.0, -4.0), (0.0, 4.0), (0.0, -4.0)) == 0.0  # no move, no term
    assert goal.goal_term(0.0, (0.0, -4.0), (0.0, 4.0), (0.0, 0.0)) == 0.0
    assert goal.goal_term(2.0, (1.0, 1.0), (1.0, 1.0), (1.0, 4.0)) == -6.0  # d0 = 0
    # the goal is not the origin: the differences are formed first
    assert goal.goal_term(1.0, (1.0, -2.0), (1.0, 6.0), (4.0, 2.0)) == 8.0 - 5.0


def test_goal_term_is_a_rounded_product_then_a_rounded_sum():
    # circle crossing, three steps of 0.25 straight at the goal: d0 = 8, d1 = 7.25, progress 0.75 exactly; 0.1 is not a
    # binary fraction, so w * progress is rounded ...
    term = goal.goal_term(0.1, (0.0, -4.0), (0.0, 4.0), (0.0, -3.25))
    assert term == 0.1 * 0.75 == 0.07500000000000001
    assert Fraction(term) != Fraction(0.1) * Fraction(0.75)
    # ... and the rule adds that rounded product to ret: a fused multiply-add, which rounds the exact product's sum once, gives
    # another double behind a discomfort penalty of -0.0125
    ret = -0.0125
    fused = float(Fraction(ret) + Fraction(0.1) * Fraction(0.75))
    assert ret + term == 0.06250000000000001 and fused == 0.0625
    # the same under a discounted success reward
    assert 0.9 + term == 0.9750000000000001 and float(Fraction(0.9) + Fraction(0.1) * Fraction(0.75)) == 0.975


def test_goal_term_uses_the_fused_norm():
    import lookahead_cv_reference as ref
    assert goal.norm2 is ref.norm2
    # tests/test_lookahead_cv_host.py's pair whose fused and unfused radicands differ, as the end point
    x, y = 1.25 * 2.0 ** -27, 1.0 + 2.0 ** -27
    fused = 1.0 + 2.0 ** -26 + 2.0 ** -52
    assert x * x + y * y != fused and ref.norm2(x, y) == math.sqrt(fused)
    assert goal.goal_term(0.25, (0.0, 2.0), (0.0, 0.0), (x, y)) == 0.25 * (2.0 - math.sqrt(fused))
