"""The device predictors and the closed loop on predicted futures without a GPU: the C-ABI surface (declared, bound, exported, no
version bump, no existing struct touched), the refusals that depend on the arguments alone (made with pointers that address
nothing: a refusal reads none of them), the python entry points' own checks, and what the crafted scene of test_plan_predict.py
must contain for its bit-for-bit comparison to cover every case of the to_goal rule."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from conftest import ROOT

import plan_predict_cases as cases
from support import built, DANGLING, models as _models, predictors as _predictors  # noqa: F401  (built: module fixture)

DECLARATIONS = ('enum { CN_PREDICT_CONSTANT_VELOCITY = 0, CN_PREDICT_TO_GOAL = 1 };',
                '''int cn_predict(cn_engine* e, int n_steps, int n_modes,
               const int32_t* models /* HOST [n_modes] */,
               double* human_vel     /* DEVICE [B][M][n][A-1][2], 16-byte aligned */);''',
                '''int cn_plan_cem_predict_rollout (cn_engine* e, const cn_rollout_io* io, int n_real_steps, const cn_plan_cfg* cfg,
                                 const cn_plan* plan, const cn_predictors* pred, uint32_t counter);''',
                '''int cn_plan_mppi_predict_rollout(cn_engine* e, const cn_rollout_io* io, int n_real_steps, const cn_plan_cfg* cfg,
                                 const cn_plan* plan, const cn_predictors* pred, double temperature, int fit_std,
                                 uint32_t counter);''')
NAMES = ('cn_predict', 'cn_plan_cem_predict_rollout', 'cn_plan_mppi_predict_rollout')  # + struct cn_predictors, enum CN_PREDICT_*


def test_header_binding_and_library_agree(built):
    text = open(os.path.join(ROOT, 'include', 'crowdnav_amd.h')).read()
    for decl in DECLARATIONS:
        assert decl in text, decl
    assert '#define CN_ABI_VERSION 12' in text and '#define CN_LAUNCH_COUNTERS 6' in text
    # the sentences the earlier sections state stay; the new calls stand beside them
    assert 'There is deliberately no *_rollout form: a prediction is made from the' in text
    assert text.index('Device MPPI update') < text.index('Device predictors and the closed loop on predicted futures')
    body = text[text.index('typedef struct cn_predictors {'):text.index('} cn_predictors;')]
    declared = [line.split(';')[0].split()[-1].lstrip('*').split('[')[0] for line in body.splitlines()[1:] if ';' in line]
    assert declared == [name for name, _ in built.CnPredictors._fields_], declared
    S = built.CnPredictors
    assert C.sizeof(S) == 64
    assert [getattr(S, name).offset for name, _ in S._fields_] == [0, 4, 36, 40, 48, 56]
    assert S.model.size == 32
    P, io, cfg, plan, pred = C.c_void_p, C.POINTER(built.CnRolloutIo), C.POINTER(built.CnPlanCfg), C.POINTER(built.CnPlan), C.POINTER(S)
    assert built.SYMBOLS['cn_predict'] == (C.c_int, [P, C.c_int, C.c_int, C.POINTER(C.c_int32), P])
    assert built.SYMBOLS['cn_plan_cem_predict_rollout'] == (C.c_int, [P, io, C.c_int, cfg, plan, pred, C.c_uint32])
    assert built.SYMBOLS['cn_plan_mppi_predict_rollout'] == (C.c_int, [P, io, C.c_int, cfg, plan, pred, C.c_double, C.c_int, C.c_uint32])
    raw = C.CDLL(built.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
    assert (built.PREDICT_CONSTANT_VELOCITY, built.PREDICT_TO_GOAL) == (0, 1)
    assert built.PREDICT_MODELS == ('constant_velocity', 'to_goal') and built.PREDICT_ALIASES == {'cv': 'constant_velocity'}
    # nothing that existed moved
    assert built.load().cn_abi_version() == 12 == built.ABI_VERSION and len(built.LAUNCH_COUNTERS) == 6
    assert C.sizeof(built.CnPlanCfg) == 56 and C.sizeof(built.CnPlan) == 120 and C.sizeof(built.CnPathModes) == 32
    assert C.sizeof(built.CnLookaheadOut) == 48 and C.sizeof(built.CnModesOut) == 80


def test_predict_refusals_that_need_no_engine(built):
    lib = built.load()
    INV, UNS = built.CN_ERR_INVALID, built.CN_ERR_UNSUPPORTED

    def refused(args, word, status=INV):
        assert lib.cn_predict(*args) == status, (word, lib.cn_last_error())
        assert word in lib.cn_last_error().decode(), lib.cn_last_error()

    good = _models(0, 1)
    # 1. the two pointers, models first, before everything beside them
    refused((None, -1, 0, None, None), 'cn_predict: models is NULL')
    refused((None, 4, 2, None, DANGLING), 'cn_predict: models is NULL')
    refused((None, -1, 0, good, None), 'cn_predict: human_vel is NULL')
    # 2. n_modes, before the models are read (the pointer addresses nothing here)
    for m in (0, -3):
        refused((None, -1, m, C.cast(DANGLING, C.POINTER(C.c_int32)), DANGLING), 'cn_predict: n_modes must be >= 1 (got %d)' % m)
    refused((None, -1, 9, C.cast(DANGLING, C.POINTER(C.c_int32)), DANGLING), 'cn_predict: n_modes = 9 exceeds the 8 modes', UNS)
    # 3. a model that is neither value, by index and value; the first such one; entries behind n_modes are not read
    refused((None, -1, 3, _models(0, 1, 5), DANGLING), 'cn_predict: model[2] = 5 unknown')
    refused((None, -1, 8, _models(1, -1, 7, 0, 0, 0, 0, 0), DANGLING), 'cn_predict: model[1] = -1 unknown')
    refused((None, -1, 2, _models(0, 1, 5), DANGLING), 'cn_predict: n_steps must be >= 0 (got -1)')
    # 4. n_steps, 5. the engine — n_steps == 0 included: the checks come before the no-op
    refused((None, -1, 2, good, DANGLING), 'cn_predict: n_steps must be >= 0 (got -1)')
    refused((None, 4, 2, good, DANGLING), 'cn_predict: engine is NULL')
    refused((None, 0, 2, good, DANGLING), 'cn_predict: engine is NULL')
    refused((None, 0, 8, _models(0, 1, 0, 1, 0, 1, 0, 1), DANGLING), 'cn_predict: engine is NULL')


def test_rollout_refusals_that_need_no_engine(built):
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
    calls = {'cn_plan_cem_predict_rollout': lambda c, p, q, T=0.7, n_real=2: lib.cn_plan_cem_predict_rollout(None, io, n_real, c, p, q, 21),
             'cn_plan_mppi_predict_rollout': lambda c, p, q, T=0.7, n_real=2: lib.cn_plan_mppi_predict_rollout(None, io, n_real, c, p, q, T, 0, 21)}
    for name, call in calls.items():
        for args, status, word in (
                # 1. pred and its table, before everything beside them
                ((None, None, None), INV, name + ': pred is NULL'),
                ((C.byref(cfg), C.byref(plan), None), INV, name + ': pred is NULL'),
                ((None, None, C.byref(_predictors(built, human_vel=None, n_modes=0))), INV, name + ': pred->human_vel is NULL'),
                # 2. n_modes, 3. the models — entries behind n_modes are not read; reduce and risk_penalty not yet
                ((None, None, C.byref(_predictors(built, n_modes=0, reduce=7))), INV, name + ': n_modes must be >= 1 (got 0)'),
                ((None, None, C.byref(_predictors(built, n_modes=9, model=[5] * 8))), UNS, name + ': n_modes = 9 exceeds the 8 modes'),
                ((None, None, C.byref(_predictors(built, n_modes=3, model=[1, 0, 2, 9], risk_penalty=-1.0))), INV,
                 name + ': model[2] = 2 unknown'),
                # 4. what the cn_plan_* calls refuse, in their order
                ((None, C.byref(plan), C.byref(ok)), INV, name + ': cfg is NULL'),
                ((C.byref(cfg), None, C.byref(ok)), INV, name + ': plan is NULL'),
                ((C.byref(cfg), C.byref(no_mean), C.byref(ok)), INV, name + ': plan->mean is NULL'),
                ((C.byref(few), C.byref(plan), C.byref(ok)), INV, name + ': n_candidates must be >= 2 (got 1)'),
                # ... the engine last of what needs none: a bad reduce (M > 1) is not looked at before it, nor is n_real_steps
                ((C.byref(cfg), C.byref(plan), C.byref(_predictors(built, reduce=7, model=[1, 0, 9]))), INV, name + ': engine is NULL'),
                ((C.byref(cfg), C.byref(plan), C.byref(_predictors(built, n_modes=1, weight=None, reduce=-4))), INV, name + ': engine is NULL')):
            assert call(*args) == status, (name, word, lib.cn_last_error())
            assert word in lib.cn_last_error().decode(), lib.cn_last_error()
        assert call(C.byref(cfg), C.byref(plan), C.byref(ok), n_real=-1) == INV and name + ': engine is NULL' in lib.cn_last_error().decode()
    assert calls['cn_plan_mppi_predict_rollout'](C.byref(cfg), C.byref(plan), C.byref(ok), T=0.0) == INV
    assert 'cn_plan_mppi_predict_rollout: temperature' in lib.cn_last_error().decode()
    # the models come before the temperature
    assert calls['cn_plan_mppi_predict_rollout'](C.byref(cfg), C.byref(plan), C.byref(_predictors(built, model=[0, 3])), T=0.0) == INV
    assert 'model[1] = 3 unknown' in lib.cn_last_error().decode()


def test_the_python_surface_and_its_own_checks(built):
    from crowdnav_amd import engine as E
    from crowdnav_amd import predict
    params = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    default = lambda f, name: inspect.signature(f).parameters[name].default  # noqa: E731
    B = E.BatchedCrowdSim
    assert params(B.predict) == ['self', 'n', 'models', 'out'] and default(B.predict, 'models') == 'to_goal' and default(B.predict, 'out') is None
    assert params(B.plan_predict_begin) == ['self', 'plan', 'models', 'weights', 'reduce', 'risk_penalty']
    assert default(B.plan_predict_begin, 'weights') is None and default(B.plan_predict_begin, 'reduce') == 'mean'
    assert default(B.plan_predict_begin, 'risk_penalty') == 0.0
    assert params(B.plan_predict_rollout) == ['self', 'plan', 'pred', 'n_real', 'counter', 'temperature', 'fit_std']
    assert default(B.plan_predict_rollout, 'temperature') is None and default(B.plan_predict_rollout, 'fit_std') is False
    # predict.py keeps its functions as they were: they are the oracle of the device form, which its docstring points to
    assert params(predict.constant_velocity) == ['state8', 'n'] and params(predict.to_goal) == ['state8', 'n', 'dt']
    assert params(predict.from_positions) == ['start_xy', 'positions', 'dt']
    assert 'cn_predict' in predict.__doc__ and 'BatchedCrowdSim.predict' in predict.__doc__

    class NoLibrary(object):  # an unknown name is refused before the library is called
        def __getattr__(self, name):
            raise AssertionError('the library was asked for ' + name)

    import torch
    eng = B.__new__(B)
    eng.B, eng.H, eng.A, eng.device, eng._lib, eng._h = 2, 3, 4, torch.device('cpu'), NoLibrary(), C.c_void_p(0x10)
    eng._rollout = (built.CnRolloutIo(), {})
    for bad in ('orca', 'TO_GOAL', '', ('cv', 'straight'), ['to_goal', None], (0,)):
        with pytest.raises(ValueError, match='unknown predictor'):
            eng.predict(4, bad)
    for bad in ((), [], ('cv',) * 9, None, 3, {'cv': 1}):
        with pytest.raises(ValueError, match='models must be a name or a sequence of 1 .. 8 names'):
            eng.predict(4, bad)
    with pytest.raises(ValueError, match='n must be >= 0'):
        eng.predict(-1, 'cv')
    for models, shape in (('cv', (2, 4, 3, 2)), (('cv',), (2, 1, 4, 3, 2)), (('to_goal', 'constant_velocity', 'cv'), (2, 3, 4, 3, 2))):
        for out in (torch.zeros(shape, dtype=torch.float32), torch.zeros(shape[:-1] + (3,), dtype=torch.float64),
                    torch.zeros(shape + (2,), dtype=torch.float64)[..., 0], np.zeros(shape)):
            with pytest.raises(ValueError, match='out must be a contiguous'):
                eng.predict(4, models, out=out)
    # n = 0: a no-op that does not reach the library either
    assert tuple(eng.predict(0, 'to_goal').shape) == (2, 0, 3, 2) and tuple(eng.predict(0, ('cv', 'to_goal')).shape) == (2, 2, 0, 3, 2)
    plan = eng.plan_begin(5, 4, 2, 1, 0.3)
    with pytest.raises(ValueError, match='a Plan made by'):
        eng.plan_predict_begin(object(), 'cv')
    with pytest.raises(ValueError, match='unknown predictor'):
        eng.plan_predict_begin(plan, ('cv', 'orca'))
    with pytest.raises(ValueError, match='models must be'):
        eng.plan_predict_begin(plan, ())
    for bad in ('max', 'MEAN', 0, None):
        with pytest.raises(ValueError, match='reduce must be one of'):
            eng.plan_predict_begin(plan, ('cv', 'to_goal'), reduce=bad)
    for bad in (np.ones(2), np.ones((2, 3)), np.ones((3, 2))):
        with pytest.raises(ValueError, match='weights must be'):
            eng.plan_predict_begin(plan, ('cv', 'to_goal'), weights=bad)
    pred = eng.plan_predict_begin(plan, ('cv', 'to_goal', 'cv'), weights=np.array([[0.5, 0.25, 0.25]] * 2), reduce='min', risk_penalty=0.5)
    assert isinstance(pred, E.Predictors) and tuple(pred.human_vel.shape) == (2, 3, 4, 3, 2) and pred.human_vel.dtype == torch.float64
    assert pred.models == ('constant_velocity', 'to_goal', 'constant_velocity')
    assert (pred.c.n_modes, list(pred.c.model), pred.c.reduce, pred.c.risk_penalty) == (3, [0, 1, 0, 0, 0, 0, 0, 0], built.MODES_MIN, 0.5)
    assert pred.c.human_vel == pred.human_vel.data_ptr() and pred.c.weight == pred.weights.data_ptr()
    one = eng.plan_predict_begin(plan, 'to_goal')
    assert tuple(one.human_vel.shape) == (2, 1, 4, 3, 2) and one.c.n_modes == 1 and one.c.model[0] == built.PREDICT_TO_GOAL and not one.c.weight
    other = eng.plan_begin(5, 4, 2, 1, 0.3)
    for args in ((object(), pred), (plan, object()), (other, pred), (plan, one.c)):
        with pytest.raises(ValueError, match='plan_begin|plan_predict_begin'):
            eng.plan_predict_rollout(*args, 3, 0)


def test_to_goal_on_numpy_is_ieee_arithmetic_operation_by_operation():
    """The oracle of the device kernel has to be what the header writes down: every product, quotient and sum one IEEE operation
    and a correctly rounded square root.  Python's float arithmetic and math.sqrt are that; torch's float64 sqrt on the CPU is
    within an ulp of it but differs on about 1 % of arguments, which is why predict.to_goal takes numpy's there."""
    import math
    from crowdnav_amd import predict
    rng = np.random.RandomState(5)
    B, H, n, dt = 40, 5, 13, cases.DT
    state = np.zeros((B, H + 1, 8))
    state[:, :, 0:2], state[:, :, 4:6] = rng.uniform(-4.0, 4.0, (B, H + 1, 2)), rng.uniform(-4.0, 4.0, (B, H + 1, 2))
    state[:, :, 6], state[:, :, 7] = 0.3, rng.uniform(0.5, 1.5, (B, H + 1))
    state[:, 1, 4:6] = state[:, 1, 0:2] + rng.uniform(-0.5, 0.5, (B, 2))  # some arrive within the horizon
    want = np.zeros((B, n, H, 2))
    for b in range(B):
        for h in range(H):
            px, py, _, _, gx, gy, _, v_pref = (float(x) for x in state[b, h + 1])
            for t in range(n):
                dx, dy = gx - px, gy - py
                dist = math.sqrt(dx * dx + dy * dy)
                v = (0.0, 0.0) if not dist > 0.0 else (dx / dt, dy / dt) if dist <= v_pref * dt else ((dx / dist) * v_pref, (dy / dist) * v_pref)
                want[b, t, h] = v
                px, py = px + v[0] * dt, py + v[1] * dt
    got = predict.to_goal(state, n, dt)
    assert got.dtype == np.float64 and got.tobytes() == want.tobytes(), int((got != want).sum())
    counted = cases.to_goal_cases(state, n, dt)
    assert counted['zero'] >= 1 and counted['short'] >= 1 and counted['cruise'] >= 1000, counted


def test_the_crafted_scene_takes_every_case_of_the_to_goal_rule():
    """dt = 0.25, n = 6, the five crafted humans: 19 steps at the goal, 1 whose distance is v_pref dt exactly, 2 shortened ones
    and 8 at v_pref — counted on predict.to_goal's own table."""
    state = cases.crafted_state(5)[None]
    assert state.shape == (1, 6, 8) and np.array_equal(state[0, 1:], np.array(cases.CRAFTED))
    got = cases.to_goal_cases(state, 6, cases.DT)
    print(got)
    assert got == dict(zero=19, exact=1, short=2, cruise=8)
    # cut and padded: the shapes of the device test keep at least a cruising and a standing human, and H = 5, 12 all four cases
    assert cases.to_goal_cases(cases.crafted_state(1)[None], 6, cases.DT) == dict(zero=6, exact=0, short=0, cruise=0)
    padded = cases.to_goal_cases(cases.crafted_state(12)[None], 13, cases.DT)
    print(padded)
    assert all(padded[k] >= 2 for k in cases.CASES) and sum(padded.values()) == 12 * 13
    # the padding repeats the humans 8 m further out without changing what they do
    far = cases.crafted_state(12)
    assert np.array_equal(far[6:11, 0] - far[1:6, 0], np.full(5, 8.0)) and np.array_equal(far[6:11, 1:4], far[1:6, 1:4])
