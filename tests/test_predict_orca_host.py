"""The ORCA predictor (cn_predict_orca) and its closed loop without a GPU: the C-ABI surface (declared, bound, exported, no
version bump, nothing that existed moved), the refusals that depend on the arguments alone, in the header's order (made with a
NULL engine and pointers that address nothing: a refusal reads none of them), the python entry points' own checks with the
library stubbed, and — on the CPU oracle alone — what the scenes of test_predict_orca.py must contain for its bit-for-bit
comparison to bite."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from conftest import ROOT

import predict_orca_cases as cases
from support import built, DANGLING, predictors as _predictors, Recorder as _Recorder  # noqa: F401  (built: module fixture)

DECLARATIONS = ('''int cn_predict_orca(cn_engine* e, int n_steps, int n_modes, int mode,
                    double* human_vel /* DEVICE [B][n_modes][n_steps][A-1][2], 16-byte aligned */);''',
                '''int cn_plan_cem_predict_orca_rollout (cn_engine* e, const cn_rollout_io* io, int n_real_steps, const cn_plan_cfg* cfg,
                                      const cn_plan* plan, const cn_predictors* pred, int orca_mode, uint32_t counter);''',
                '''int cn_plan_mppi_predict_orca_rollout(cn_engine* e, const cn_rollout_io* io, int n_real_steps, const cn_plan_cfg* cfg,
                                      const cn_plan* plan, const cn_predictors* pred, int orca_mode, double temperature,
                                      int fit_std, uint32_t counter);''')
NAMES = ('cn_predict_orca', 'cn_plan_cem_predict_orca_rollout', 'cn_plan_mppi_predict_orca_rollout')


def test_header_binding_and_library_agree(built):
    text = open(os.path.join(ROOT, 'include', 'crowdnav_amd.h')).read()
    for decl in DECLARATIONS:
        assert decl in text, decl
    P, io, cfg, plan = C.c_void_p, C.POINTER(built.CnRolloutIo), C.POINTER(built.CnPlanCfg), C.POINTER(built.CnPlan)
    pred = C.POINTER(built.CnPredictors)
    assert built.SYMBOLS['cn_predict_orca'] == (C.c_int, [P, C.c_int, C.c_int, C.c_int, P])
    assert built.SYMBOLS['cn_plan_cem_predict_orca_rollout'] == (C.c_int, [P, io, C.c_int, cfg, plan, pred, C.c_int, C.c_uint32])
    assert built.SYMBOLS['cn_plan_mppi_predict_orca_rollout'] == (C.c_int, [P, io, C.c_int, cfg, plan, pred, C.c_int, C.c_double,
                                                                            C.c_int, C.c_uint32])
    raw = C.CDLL(built.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
    # nothing that existed moved
    assert 'enum { CN_PREDICT_CONSTANT_VELOCITY = 0, CN_PREDICT_TO_GOAL = 1 };' in text
    assert '#define CN_ABI_VERSION 12' in text and '#define CN_LAUNCH_COUNTERS 6' in text
    assert 'There is deliberately no *_rollout form: a prediction is made from the' in text
    sections = ['Device MPPI update', 'Device predictors and the closed loop on predicted futures',
                'The ORCA predictor: humans that avoid each other, the robot unseen']
    assert [text.count(s) for s in sections] == [1, 1, 1] and sorted(sections, key=text.index) == sections
    assert text.index('int cn_plan_mppi_predict_rollout(') < text.index(sections[2]) < text.index('int cn_predict_orca(')
    assert built.load().cn_abi_version() == 12 == built.ABI_VERSION and len(built.LAUNCH_COUNTERS) == 6
    assert [C.sizeof(s) for s in (built.CnPlanCfg, built.CnPlan, built.CnPathModes, built.CnLookaheadOut, built.CnModesOut,
                                  built.CnPredictors)] == [56, 120, 32, 48, 80, 64]
    assert built.PREDICT_MODELS == ('constant_velocity', 'to_goal') and built.PREDICT_ALIASES == {'cv': 'constant_velocity'}
    # cn_predict keeps refusing every other code: the new predictor is not one of its models
    lib = built.load()
    for code in (2, 3, 4, 5, 7, 9, -1):
        assert lib.cn_predict(None, 4, 1, (C.c_int32 * 1)(code), DANGLING) == built.CN_ERR_INVALID
        assert ('cn_predict: model[0] = %d unknown' % code) in lib.cn_last_error().decode()


def test_predict_orca_refusals_in_order(built):
    lib = built.load()
    INV, UNS = built.CN_ERR_INVALID, built.CN_ERR_UNSUPPORTED

    def refused(args, word, status=INV):
        assert lib.cn_predict_orca(*args) == status, (word, lib.cn_last_error())
        assert word in lib.cn_last_error().decode(), lib.cn_last_error()

    # (engine, n_steps, n_modes, mode, human_vel): each refusal with everything behind it wrong as well
    refused((None, -1, 0, -1, None), 'cn_predict_orca: human_vel is NULL')
    refused((None, 4, 2, 1, None), 'cn_predict_orca: human_vel is NULL')
    for m in (0, -3):
        refused((None, -1, m, 9, DANGLING), 'cn_predict_orca: n_modes must be >= 1 (got %d)' % m)
    refused((None, -1, 9, 9, DANGLING), 'cn_predict_orca: n_modes = 9 exceeds the 8 modes', UNS)
    for M, mode in ((1, 1), (1, -1), (8, 8), (3, -2), (2, 7)):
        refused((None, -1, M, mode, DANGLING), 'cn_predict_orca: mode = %d is outside 0 .. n_modes - 1 = %d' % (mode, M - 1))
    refused((None, -1, 2, 1, DANGLING), 'cn_predict_orca: n_steps must be >= 0 (got -1)')
    refused((None, -5, 8, 7, DANGLING), 'cn_predict_orca: n_steps must be >= 0 (got -5)')
    # the engine — n_steps == 0 included: the checks come before the no-op
    refused((None, 4, 2, 1, DANGLING), 'cn_predict_orca: engine is NULL')
    refused((None, 0, 1, 0, DANGLING), 'cn_predict_orca: engine is NULL')
    refused((None, 0, 8, 7, DANGLING), 'cn_predict_orca: engine is NULL')


def test_rollout_refusals_in_order(built):
    """cn_plan_*_predict_rollout's refusals, in their order and with this call's name; orca_mode directly behind the models."""
    lib = built.load()
    INV, UNS = built.CN_ERR_INVALID, built.CN_ERR_UNSUPPORTED
    look = built.CnLookaheadOut(ret=DANGLING, info=DANGLING, steps=DANGLING, time=DANGLING, final_state8=DANGLING, final_theta=DANGLING)
    cfg = built.CnPlanCfg(n_steps=4, n_candidates=5, n_elites=2, iterations=1, bootstrap=0, sort_humans=0, init_std=0.3,
                          min_std=0.0, smoothing=0.0, seed=1)
    plan = built.CnPlan(mean=DANGLING, std=DANGLING, best_actions=DANGLING, best_score=DANGLING, action=DANGLING,
                        candidates=DANGLING, look=look, value=DANGLING, score=DANGLING, order=DANGLING)
    io = C.cast(DANGLING, C.POINTER(built.CnRolloutIo))
    no_mean = built.CnPlan.from_buffer_copy(plan)
    no_mean.mean = None
    few = built.CnPlanCfg.from_buffer_copy(cfg)
    few.n_candidates = 1
    ok = _predictors(built)
    calls = {'cn_plan_cem_predict_orca_rollout':
             lambda c, p, q, mode=1, T=0.7, n_real=2: lib.cn_plan_cem_predict_orca_rollout(None, io, n_real, c, p, q, mode, 21),
             'cn_plan_mppi_predict_orca_rollout':
             lambda c, p, q, mode=1, T=0.7, n_real=2: lib.cn_plan_mppi_predict_orca_rollout(None, io, n_real, c, p, q, mode, T, 0, 21)}
    for name, call in calls.items():
        for args, mode, status, word in (
                # 1. pred and its table, before everything beside them
                ((None, None, None), 9, INV, name + ': pred is NULL'),
                ((C.byref(cfg), C.byref(plan), None), 1, INV, name + ': pred is NULL'),
                ((None, None, C.byref(_predictors(built, human_vel=None, n_modes=0))), 9, INV, name + ': pred->human_vel is NULL'),
                # 2. n_modes, 3. the models, before orca_mode
                ((None, None, C.byref(_predictors(built, n_modes=0, reduce=7))), 9, INV, name + ': n_modes must be >= 1 (got 0)'),
                ((None, None, C.byref(_predictors(built, n_modes=9, model=[5] * 8))), 9, UNS, name + ': n_modes = 9 exceeds the 8 modes'),
                ((None, None, C.byref(_predictors(built, n_modes=3, model=[1, 0, 2, 9]))), 9, INV, name + ': model[2] = 2 unknown'),
                # ... the slot orca_mode overwrites must still name a model cn_predict knows
                ((C.byref(cfg), C.byref(plan), C.byref(_predictors(built, model=[0, 5]))), 1, INV, name + ': model[1] = 5 unknown'),
                # 4. orca_mode, behind the models and before the plan, its settings and the engine
                ((None, None, C.byref(ok)), 2, INV, name + ': orca_mode = 2 is outside 0 .. n_modes - 1 = 1'),
                ((None, None, C.byref(ok)), -1, INV, name + ': orca_mode = -1 is outside 0 .. n_modes - 1 = 1'),
                ((C.byref(few), C.byref(no_mean), C.byref(_predictors(built, n_modes=1))), 1, INV,
                 name + ': orca_mode = 1 is outside 0 .. n_modes - 1 = 0'),
                # 5. what the cn_plan_* calls refuse, in their order
                ((None, C.byref(plan), C.byref(ok)), 1, INV, name + ': cfg is NULL'),
                ((C.byref(cfg), None, C.byref(ok)), 0, INV, name + ': plan is NULL'),
                ((C.byref(cfg), C.byref(no_mean), C.byref(ok)), 1, INV, name + ': plan->mean is NULL'),
                ((C.byref(few), C.byref(plan), C.byref(ok)), 1, INV, name + ': n_candidates must be >= 2 (got 1)'),
                # ... the engine last of what needs none: a bad reduce (M > 1) is not looked at before it, nor is n_real_steps
                ((C.byref(cfg), C.byref(plan), C.byref(_predictors(built, reduce=7, model=[1, 0, 9]))), 0, INV, name + ': engine is NULL'),
                ((C.byref(cfg), C.byref(plan), C.byref(_predictors(built, n_modes=1, weight=None, reduce=-4))), 0, INV,
                 name + ': engine is NULL')):
            assert call(*args, mode=mode) == status, (name, word, lib.cn_last_error())
            assert word in lib.cn_last_error().decode(), lib.cn_last_error()
        assert call(C.byref(cfg), C.byref(plan), C.byref(ok), n_real=-1) == INV and name + ': engine is NULL' in lib.cn_last_error().decode()
    mppi = calls['cn_plan_mppi_predict_orca_rollout']
    assert mppi(C.byref(cfg), C.byref(plan), C.byref(ok), T=0.0) == INV
    assert 'cn_plan_mppi_predict_orca_rollout: temperature' in lib.cn_last_error().decode()
    # the models and orca_mode come before the temperature
    assert mppi(C.byref(cfg), C.byref(plan), C.byref(_predictors(built, model=[0, 3])), T=0.0) == INV
    assert 'model[1] = 3 unknown' in lib.cn_last_error().decode()
    assert mppi(C.byref(cfg), C.byref(plan), C.byref(ok), mode=2, T=0.0) == INV and 'orca_mode = 2' in lib.cn_last_error().decode()


def test_the_python_surface_and_its_own_checks(built):
    import torch
    from crowdnav_amd import engine as E
    from crowdnav_amd import predict
    params = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    default = lambda f, name: inspect.signature(f).parameters[name].default  # noqa: E731
    Sim = E.BatchedCrowdSim
    assert params(Sim.predict_orca) == ['self', 'n', 'out', 'mode']
    assert default(Sim.predict_orca, 'out') is None and default(Sim.predict_orca, 'mode') is None
    assert params(Sim.plan_predict_orca_rollout) == ['self', 'plan', 'pred', 'n_real', 'counter', 'orca_mode', 'temperature', 'fit_std']
    assert default(Sim.plan_predict_orca_rollout, 'orca_mode') == 0 and default(Sim.plan_predict_orca_rollout, 'temperature') is None
    assert default(Sim.plan_predict_orca_rollout, 'fit_std') is False
    # what existed keeps its signature, and keeps refusing the name: the new predictor has entry points of its own
    assert params(Sim.predict) == ['self', 'n', 'models', 'out'] and default(Sim.predict, 'models') == 'to_goal'
    assert params(Sim.plan_predict_begin) == ['self', 'plan', 'models', 'weights', 'reduce', 'risk_penalty']
    assert params(Sim.plan_predict_rollout) == ['self', 'plan', 'pred', 'n_real', 'counter', 'temperature', 'fit_std']
    assert 'predict_orca' in predict.__doc__ and not hasattr(predict, 'orca')

    eng = Sim.__new__(Sim)
    eng.B, eng.H, eng.A, eng.device, eng._lib, eng._h = 2, 3, 4, torch.device('cpu'), _Recorder(), C.c_void_p(0x10)
    eng._rollout = (built.CnRolloutIo(), {})
    plan = eng.plan_begin(5, 4, 2, 1, 0.3)
    for bad in ('orca', ('cv', 'orca')):
        with pytest.raises(ValueError, match='unknown predictor'):
            eng.predict(4, bad)
        with pytest.raises(ValueError, match='unknown predictor'):
            eng.plan_predict_begin(plan, bad)
    assert eng._lib.calls == []
    # n
    with pytest.raises(ValueError, match='n must be >= 0'):
        eng.predict_orca(-1)
    # n = 0: a no-op that does not reach the library, in either form
    assert tuple(eng.predict_orca(0).shape) == (2, 0, 3, 2)
    empty = torch.zeros((2, 3, 0, 3, 2), dtype=torch.float64)
    assert eng.predict_orca(0, out=empty, mode=2) is empty and eng._lib.calls == []
    # out without a mode: lookahead_paths' table
    for out in (torch.zeros((2, 4, 3, 2), dtype=torch.float32), torch.zeros((2, 4, 3, 3), dtype=torch.float64),
                torch.zeros((2, 4, 3, 2, 2), dtype=torch.float64)[..., 0], np.zeros((2, 4, 3, 2)),
                torch.zeros((2, 1, 4, 3, 2), dtype=torch.float64)):
        with pytest.raises(ValueError, match='out must be a contiguous'):
            eng.predict_orca(4, out=out)
    # a mode needs the table it is a slot of
    with pytest.raises(ValueError, match='mode needs out'):
        eng.predict_orca(4, mode=0)
    for out in (torch.zeros((2, 4, 3, 2), dtype=torch.float64), torch.zeros((2, 0, 4, 3, 2), dtype=torch.float64),
                torch.zeros((2, 9, 4, 3, 2), dtype=torch.float64), np.zeros((2, 4, 3, 2)), [[0.0]]):
        with pytest.raises(ValueError, match='out must be .*M in 1..8'):
            eng.predict_orca(4, out=out, mode=0)
    table = torch.zeros((2, 3, 4, 3, 2), dtype=torch.float64)
    for bad in (3, -1, 1.0, '1', True, (1,)):
        with pytest.raises(ValueError, match='mode must be an int in 0 .. M - 1 = 2'):
            eng.predict_orca(4, out=table, mode=bad)
    for out in (torch.zeros((2, 3, 4, 3, 2), dtype=torch.float32), torch.zeros((2, 3, 5, 3, 2), dtype=torch.float64),
                torch.zeros((3, 3, 4, 3, 2), dtype=torch.float64), torch.zeros((2, 3, 4, 3, 2, 2), dtype=torch.float64)[..., 0],
                np.zeros((2, 3, 4, 3, 2))):
        with pytest.raises(ValueError, match='out must be a contiguous'):
            eng.predict_orca(4, out=out, mode=1)
    assert eng._lib.calls == []
    # what reaches the library: (engine, n, M, mode, the table's address)
    got = eng.predict_orca(4)
    assert tuple(got.shape) == (2, 4, 3, 2) and got.dtype == torch.float64
    assert eng.predict_orca(4, out=table, mode=np.int64(2)) is table
    one = torch.zeros((2, 4, 3, 2), dtype=torch.float64)
    assert eng.predict_orca(4, out=one) is one
    names, args = zip(*eng._lib.calls)
    assert names == ('cn_predict_orca',) * 3
    assert [a[1:4] for a in args] == [(4, 1, 0), (4, 3, 2), (4, 1, 0)]
    assert [a[4].value for a in args] == [got.data_ptr(), table.data_ptr(), one.data_ptr()]
    del eng._lib.calls[:]
    # the rollout: pred is plan_predict_begin's; orca_mode is checked against its M before the library is asked
    pred = eng.plan_predict_begin(plan, ('cv', 'to_goal'), reduce='min')
    other = eng.plan_begin(5, 4, 2, 1, 0.3)
    for args in ((object(), pred), (plan, object()), (other, pred), (plan, pred.c)):
        with pytest.raises(ValueError, match='plan_begin|plan_predict_begin'):
            eng.plan_predict_orca_rollout(*args, 3, 0)
    for bad in (2, -1, 0.0, None, True):
        with pytest.raises(ValueError, match='orca_mode must be an int in 0 .. M - 1 = 1'):
            eng.plan_predict_orca_rollout(plan, pred, 3, 0, orca_mode=bad)
    assert eng._lib.calls == []
    assert eng.plan_predict_orca_rollout(plan, pred, 3, 2 ** 32 + 7, orca_mode=1) is eng._rollout[1]
    assert eng.plan_predict_orca_rollout(plan, pred, 3, 7, temperature=0.5, fit_std=True) is eng._rollout[1]
    (cem, a), (mppi, b) = eng._lib.calls
    assert cem == 'cn_plan_cem_predict_orca_rollout' and a[2] == 3 and a[6:] == (1, 7)
    assert mppi == 'cn_plan_mppi_predict_orca_rollout' and b[2] == 3 and b[6:] == (0, 0.5, 1, 7)
    eng._rollout = None
    with pytest.raises(RuntimeError, match='rollout_begin'):
        eng.plan_predict_orca_rollout(plan, pred, 3, 0)


@pytest.mark.parametrize('crowd', sorted(cases.CROWDS))
def test_the_scenes_bite(oracle_mod, crowd):
    """On the CPU oracle alone: in the scenes of test_predict_orca.py the ORCA table is neither to_goal's nor constant
    velocity's, the larger crowds take the 3-D fallback, and humans that saw the robot would choose otherwise at once."""
    from crowdnav_amd import predict
    state, gtime = cases.oracle_start(oracle_mod, crowd)
    vel, fallback, done = cases.oracle_table(oracle_mod, crowd, state, gtime)
    H = state.shape[1] - 1
    assert vel.shape == (cases.B, cases.N, H, 2) and np.isfinite(vel).all()
    from_goal = cases.differs_from(vel, predict.to_goal(state, cases.N, 0.25))
    from_cv = cases.differs_from(vel, predict.constant_velocity(state, cases.N))
    seen = np.sqrt(((cases.visible_first_step(oracle_mod, crowd, state, gtime) - vel[:, 0]) ** 2).sum(axis=-1))
    print(crowd, 'furthest from to_goal %.3f (nearest human %.3g), from constant velocity %.3f, fallback solves %d, robot seen %.3f, '
          'rows after done %d' % (from_goal.max(), from_goal.min(), from_cv.max(), fallback.sum(), seen.max(), done.sum()))
    assert seen.max() > 1e-3  # a kernel that left the robot in fails at row 0
    if crowd in ('h5', 'h12', 'h20'):
        assert (from_goal > 1e-3).all() and (from_cv > 1e-3).any()
    if crowd in ('h12', 'h20'):
        assert fallback.any()
    if crowd == 'h1':  # one human, nobody to avoid: to_goal up to float32 rounding
        assert from_goal.max() < 1e-6
    if crowd == 'h5_mixed':  # parked placeholders take part
        parked = state[:, 1:, 0] >= 1.0e5
        assert parked.any() and not parked.all()
    # the table is a prefix in n
    assert cases.oracle_table(oracle_mod, crowd, state, gtime, n=5)[0].tobytes() == np.ascontiguousarray(vel[:, :5]).tobytes()
