"""The ORCA predictor with the robot in sight (cn_predict_orca_robot) and its closed loop without a GPU: the C-ABI surface
(declared, bound, exported, no version bump, nothing that existed moved), the refusals that depend on the arguments alone, in the
header's order (NULL engine, pointers that address nothing), the python entry points' own checks with the library stubbed, and
— on the CPU oracle alone — what the scenes of test_predict_orca_robot.py must contain for its bit-for-bit comparisons to bite."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from conftest import ROOT

import predict_orca_cases as base
import predict_orca_robot_cases as cases
from support import built, DANGLING, predictors as _predictors, Recorder as _Recorder  # noqa: F401  (built: module fixture)

NAMES = ('cn_predict_orca_robot', 'cn_plan_cem_predict_orca_nominal_rollout', 'cn_plan_mppi_predict_orca_nominal_rollout')


def _flat(text):
    return ' '.join(text.split())


def test_header_binding_and_library_agree(built):
    text = _flat(open(os.path.join(ROOT, 'include', 'crowdnav_amd.h')).read())
    for decl in ('int cn_predict_orca_robot(cn_engine* e, int n_steps, int n_modes, int mode, const double* robot_actions',
                 'int64_t env_stride /* rows between envs; 0 means n_steps */, double* human_vel',
                 'int cn_plan_cem_predict_orca_nominal_rollout (cn_engine* e, const cn_rollout_io* io, int n_real_steps, '
                 'const cn_plan_cfg* cfg, const cn_plan* plan, const cn_predictors* pred, int orca_mode, uint32_t counter);',
                 'int cn_plan_mppi_predict_orca_nominal_rollout(cn_engine* e, const cn_rollout_io* io, int n_real_steps, '
                 'const cn_plan_cfg* cfg, const cn_plan* plan, const cn_predictors* pred, int orca_mode, double temperature, '
                 'int fit_std, uint32_t counter);'):
        assert decl in text, decl
    P, io, cfg, plan = C.c_void_p, C.POINTER(built.CnRolloutIo), C.POINTER(built.CnPlanCfg), C.POINTER(built.CnPlan)
    pred = C.POINTER(built.CnPredictors)
    assert built.SYMBOLS['cn_predict_orca_robot'] == (C.c_int, [P, C.c_int, C.c_int, C.c_int, P, C.c_int64, P])
    assert built.SYMBOLS['cn_plan_cem_predict_orca_nominal_rollout'] == built.SYMBOLS['cn_plan_cem_predict_orca_rollout'] \
        == (C.c_int, [P, io, C.c_int, cfg, plan, pred, C.c_int, C.c_uint32])
    assert built.SYMBOLS['cn_plan_mppi_predict_orca_nominal_rollout'] == built.SYMBOLS['cn_plan_mppi_predict_orca_rollout'] \
        == (C.c_int, [P, io, C.c_int, cfg, plan, pred, C.c_int, C.c_double, C.c_int, C.c_uint32])
    raw = C.CDLL(built.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
    # nothing that existed moved: the version, the counters, the layouts the new calls take
    assert '#define CN_ABI_VERSION 12' in text and '#define CN_LAUNCH_COUNTERS 6' in text
    assert built.load().cn_abi_version() == 12 == built.ABI_VERSION and len(built.LAUNCH_COUNTERS) == 6
    assert [C.sizeof(s) for s in (built.CnPlanCfg, built.CnPlan, built.CnPredictors)] == [56, 120, 64]
    assert [getattr(built.CnPredictors, f).offset for f in ('n_modes', 'model', 'reduce', 'risk_penalty', 'human_vel', 'weight')] \
        == [0, 4, 36, 40, 48, 56]
    assert text.index('int cn_plan_mppi_predict_orca_rollout(') < text.index('The ORCA predictor with the robot in sight') \
        < text.index('int cn_predict_orca_robot(')


def test_predict_orca_robot_refusals_in_order(built):
    lib = built.load()
    INV, UNS = built.CN_ERR_INVALID, built.CN_ERR_UNSUPPORTED
    who = 'cn_predict_orca_robot: '

    def refused(args, word, status=INV):
        assert lib.cn_predict_orca_robot(*args) == status, (word, lib.cn_last_error())
        assert who + word in lib.cn_last_error().decode(), lib.cn_last_error()

    # (engine, n_steps, n_modes, mode, robot_actions, env_stride, human_vel): each refusal with everything behind it wrong as well
    refused((None, -1, 0, -1, None, -1, None), 'human_vel is NULL')
    refused((None, 4, 2, 1, DANGLING, 0, None), 'human_vel is NULL')
    refused((None, -1, 0, -1, None, -1, DANGLING), 'robot_actions is NULL')
    refused((None, 4, 9, 9, DANGLING, -1, DANGLING), 'env_stride = -1 rows')
    refused((None, 4, 0, 9, DANGLING, 3, DANGLING), 'env_stride = 3 rows must be 0 (= n_steps) or >= n_steps = 4')
    refused((None, 4, 0, 9, DANGLING, -2 ** 40, DANGLING), 'env_stride = %d rows' % -2 ** 40)
    # ... then cn_predict_orca's own, in its order, under this call's name; strides that are fine: 0, n, more than n, 64-bit
    for stride in (0, 4, 5 * 4, 2 ** 40):
        for m in (0, -3):
            refused((None, 4, m, 9, DANGLING, stride, DANGLING), 'n_modes must be >= 1 (got %d)' % m)
        refused((None, 4, 9, 9, DANGLING, stride, DANGLING), 'n_modes = 9 exceeds the 8 modes', UNS)
        for M, mode in ((1, 1), (1, -1), (8, 8), (3, -2)):
            refused((None, 4, M, mode, DANGLING, stride, DANGLING), 'mode = %d is outside 0 .. n_modes - 1 = %d' % (mode, M - 1))
        refused((None, 4, 2, 1, DANGLING, stride, DANGLING), 'engine is NULL')
    refused((None, -1, 2, 1, DANGLING, 0, DANGLING), 'n_steps must be >= 0 (got -1)')
    refused((None, -5, 8, 7, DANGLING, 7, DANGLING), 'n_steps must be >= 0 (got -5)')
    # the engine — n_steps == 0 included: the checks come before the no-op
    refused((None, 0, 1, 0, DANGLING, 0, DANGLING), 'engine is NULL')
    refused((None, 0, 8, 7, DANGLING, 3, DANGLING), 'engine is NULL')
    # the robot-unseen call keeps its own name in the same refusals
    assert lib.cn_predict_orca(None, 4, 2, 1, DANGLING) == INV and 'cn_predict_orca: engine is NULL' in lib.cn_last_error().decode()


def test_nominal_rollout_refusals_in_order(built):
    """The *_predict_orca_rollout calls' refusals, in their order, under the new names."""
    lib = built.load()
    INV, UNS = built.CN_ERR_INVALID, built.CN_ERR_UNSUPPORTED
    look = built.CnLookaheadOut(ret=DANGLING, info=DANGLING, steps=DANGLING, time=DANGLING, final_state8=DANGLING, final_theta=DANGLING)
    cfg = built.CnPlanCfg(n_steps=4, n_candidates=5, n_elites=2, iterations=1, bootstrap=0, sort_humans=0, init_std=0.3,
                          min_std=0.0, smoothing=0.0, seed=1)
    plan = built.CnPlan(mean=DANGLING, std=DANGLING, best_actions=DANGLING, best_score=DANGLING, action=DANGLING,
                        candidates=DANGLING, look=look, value=DANGLING, score=DANGLING, order=DANGLING)
    io = C.cast(DANGLING, C.POINTER(built.CnRolloutIo))
    no_candidates = built.CnPlan.from_buffer_copy(plan)
    no_candidates.candidates = None
    few = built.CnPlanCfg.from_buffer_copy(cfg)
    few.n_candidates = 1
    ok = _predictors(built)
    calls = {'cn_plan_cem_predict_orca_nominal_rollout':
             lambda c, p, q, mode=1, T=0.7, n_real=2: lib.cn_plan_cem_predict_orca_nominal_rollout(None, io, n_real, c, p, q, mode, 21),
             'cn_plan_mppi_predict_orca_nominal_rollout':
             lambda c, p, q, mode=1, T=0.7, n_real=2: lib.cn_plan_mppi_predict_orca_nominal_rollout(None, io, n_real, c, p, q, mode, T, 0,
                                                                                                    21)}
    for name, call in calls.items():
        for args, mode, status, word in (
                ((None, None, None), 9, INV, name + ': pred is NULL'),
                ((None, None, C.byref(_predictors(built, human_vel=None, n_modes=0))), 9, INV, name + ': pred->human_vel is NULL'),
                ((None, None, C.byref(_predictors(built, n_modes=0, reduce=7))), 9, INV, name + ': n_modes must be >= 1 (got 0)'),
                ((None, None, C.byref(_predictors(built, n_modes=9, model=[5] * 8))), 9, UNS, name + ': n_modes = 9 exceeds the 8 modes'),
                ((C.byref(cfg), C.byref(plan), C.byref(_predictors(built, model=[0, 5]))), 1, INV, name + ': model[1] = 5 unknown'),
                ((None, None, C.byref(ok)), 2, INV, name + ': orca_mode = 2 is outside 0 .. n_modes - 1 = 1'),
                ((None, C.byref(plan), C.byref(ok)), 1, INV, name + ': cfg is NULL'),
                ((C.byref(cfg), None, C.byref(ok)), 0, INV, name + ': plan is NULL'),
                ((C.byref(cfg), C.byref(no_candidates), C.byref(ok)), 1, INV, name + ': plan->candidates is NULL'),
                ((C.byref(few), C.byref(plan), C.byref(ok)), 1, INV, name + ': n_candidates must be >= 2 (got 1)'),
                ((C.byref(cfg), C.byref(plan), C.byref(_predictors(built, reduce=7))), 0, INV, name + ': engine is NULL')):
            assert call(*args, mode=mode) == status, (name, word, lib.cn_last_error())
            assert word in lib.cn_last_error().decode(), lib.cn_last_error()
        assert call(C.byref(cfg), C.byref(plan), C.byref(ok), n_real=-1) == INV and name + ': engine is NULL' in lib.cn_last_error().decode()
    mppi = calls['cn_plan_mppi_predict_orca_nominal_rollout']
    assert mppi(C.byref(cfg), C.byref(plan), C.byref(ok), T=0.0) == INV
    assert 'cn_plan_mppi_predict_orca_nominal_rollout: temperature' in lib.cn_last_error().decode()


def test_the_python_surface_and_its_own_checks(built):
    import torch
    from crowdnav_amd import engine as E
    params = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    Sim = E.BatchedCrowdSim
    assert params(Sim.predict_orca_robot) == ['self', 'n', 'robot_actions', 'out', 'mode']
    assert params(Sim.plan_predict_orca_nominal_rollout) == params(Sim.plan_predict_orca_rollout)
    eng = Sim.__new__(Sim)
    eng.B, eng.H, eng.A, eng.device, eng._lib, eng._h = 2, 3, 4, torch.device('cpu'), _Recorder(), C.c_void_p(0x10)
    eng._rollout = (built.CnRolloutIo(), {})
    eng.sync = lambda: eng._lib.calls.append(('sync', ()))
    dense = torch.zeros((2, 4, 2), dtype=torch.float64)
    with pytest.raises(ValueError, match='n must be >= 0'):
        eng.predict_orca_robot(-1, dense)
    with pytest.raises(ValueError, match='robot_actions is required'):
        eng.predict_orca_robot(4, None)
    for bad in (torch.zeros((2, 5, 2), dtype=torch.float64), torch.zeros((3, 4, 2), dtype=torch.float64), np.zeros((2, 4, 3)),
                torch.zeros((2, 4), dtype=torch.float64), [[0.0, 0.0]]):
        with pytest.raises(ValueError, match=r'robot_actions must be \[2, n = 4, 2\]'):
            eng.predict_orca_robot(4, bad)
    wide = torch.zeros((2, 4, 4), dtype=torch.float64)
    for bad in (wide[:, :, :2], wide[:, :, ::2], torch.zeros((2, 2, 4), dtype=torch.float64).transpose(1, 2)):
        with pytest.raises(ValueError, match='last two dimensions must be contiguous'):
            eng.predict_orca_robot(4, bad)
    odd = torch.zeros(2 * 9 + 8, dtype=torch.float64).as_strided((2, 4, 2), (9, 2, 1))        # 4.5 rows between envs
    overlap = torch.zeros(3 * 2 * 2 + 8, dtype=torch.float64).as_strided((2, 4, 2), (6, 2, 1))  # 3 rows: env 1 starts inside env 0
    same = dense[:1].expand(2, 4, 2)                                                              # stride 0
    for bad in (odd, overlap, same):
        with pytest.raises(ValueError, match='not a whole number of rows >= n = 4'):
            eng.predict_orca_robot(4, bad)
    # out and mode: predict_orca's checks under this name
    with pytest.raises(ValueError, match='predict_orca_robot: mode needs out'):
        eng.predict_orca_robot(4, dense, mode=0)
    with pytest.raises(ValueError, match='predict_orca_robot: out must be a contiguous'):
        eng.predict_orca_robot(4, dense, out=torch.zeros((2, 4, 3, 2), dtype=torch.float32))
    table = torch.zeros((2, 3, 4, 3, 2), dtype=torch.float64)
    with pytest.raises(ValueError, match='predict_orca_robot: mode must be an int in 0 .. M - 1 = 2'):
        eng.predict_orca_robot(4, dense, out=table, mode=3)
    assert eng._lib.calls == []
    # n = 0 does not reach the library
    assert tuple(eng.predict_orca_robot(0, torch.zeros((2, 0, 2), dtype=torch.float64)).shape) == (2, 0, 3, 2) and eng._lib.calls == []
    # what reaches it: (engine, n, M, mode, the rows' address, rows between envs, the table's address)
    cand = torch.zeros((2, 5, 4, 2), dtype=torch.float64)  # a plan's candidates [B, K, n, 2]
    got = eng.predict_orca_robot(4, dense)
    assert eng.predict_orca_robot(4, cand[:, 0], out=table, mode=2) is table
    eng.predict_orca_robot(4, cand[:, 3])
    eng.predict_orca_robot(3, cand[:, 1, 1:])
    eng.predict_orca_robot(4, np.ones((2, 4, 2)))
    eng.predict_orca_robot(4, dense.to(torch.float32))
    calls = eng._lib.calls
    assert [c[0] for c in calls] == ['cn_predict_orca_robot'] * 5 + ['sync', 'cn_predict_orca_robot', 'sync']  # copies are waited for
    lib_calls = [c[1] for c in calls if c[0] != 'sync']
    assert [a[1:4] for a in lib_calls] == [(4, 1, 0), (4, 3, 2), (4, 1, 0), (3, 1, 0), (4, 1, 0), (4, 1, 0)]
    assert [a[5] for a in lib_calls] == [4, 20, 20, 20, 4, 4]
    assert [a[4].value for a in lib_calls[:4]] == [dense.data_ptr(), cand.data_ptr(), cand[:, 3].data_ptr(), cand[:, 1, 1:].data_ptr()]
    assert lib_calls[0][6].value == got.data_ptr() and lib_calls[1][6].value == table.data_ptr()
    # a one-env engine: what lies between envs is not looked at
    one = Sim.__new__(Sim)
    one.B, one.H, one.A, one.device, one._lib, one._h = 1, 3, 4, torch.device('cpu'), _Recorder(), C.c_void_p(0x10)
    one.predict_orca_robot(4, same[:1])
    assert one._lib.calls[0][1][5] == 4
    # the robot-unseen call is as it was
    del eng._lib.calls[:]
    eng.predict_orca(4)
    assert [c[0] for c in eng._lib.calls] == ['cn_predict_orca'] and len(eng._lib.calls[0][1]) == 5
    # the closed loop: plan_predict_orca_rollout's checks, the *_nominal_rollout entry points
    del eng._lib.calls[:]
    plan = eng.plan_begin(5, 4, 2, 1, 0.3)
    pred = eng.plan_predict_begin(plan, ('cv', 'to_goal'), reduce='min')
    for args in ((object(), pred), (plan, object()), (eng.plan_begin(5, 4, 2, 1, 0.3), pred)):
        with pytest.raises(ValueError, match='plan_begin|plan_predict_begin'):
            eng.plan_predict_orca_nominal_rollout(*args, 3, 0)
    for bad in (2, -1, 0.0, None, True):
        with pytest.raises(ValueError, match='plan_predict_orca_nominal_rollout: orca_mode must be an int in 0 .. M - 1 = 1'):
            eng.plan_predict_orca_nominal_rollout(plan, pred, 3, 0, orca_mode=bad)
    assert eng._lib.calls == []
    assert eng.plan_predict_orca_nominal_rollout(plan, pred, 3, 2 ** 32 + 7, orca_mode=1) is eng._rollout[1]
    assert eng.plan_predict_orca_nominal_rollout(plan, pred, 3, 7, temperature=0.5, fit_std=True) is eng._rollout[1]
    (cem, a), (mppi, b) = eng._lib.calls
    assert cem == 'cn_plan_cem_predict_orca_nominal_rollout' and a[2] == 3 and a[6:] == (1, 7)
    assert mppi == 'cn_plan_mppi_predict_orca_nominal_rollout' and b[2] == 3 and b[6:] == (0, 0.5, 1, 7)
    eng._rollout = None
    with pytest.raises(RuntimeError, match='rollout_begin'):
        eng.plan_predict_orca_nominal_rollout(plan, pred, 3, 0)


@pytest.mark.parametrize('crowd', sorted(cases.CROWDS))
def test_the_scenes_bite(oracle_mod, crowd):
    """On the CPU oracle alone: the table of the scene differs by more than 1e-3 m/s from the robot-unseen table, from the one of
    a robot that stands (at some row t >= 1) and from the one of a robot that moves but is seen with its start velocity; the
    larger crowds take the 3-D fallback; the table is a prefix in n."""
    state, gtime = cases.start(oracle_mod, crowd)
    placed, _, _ = cases.place_robot(state)
    actions = cases.sequences()
    assert (actions[:, 1:] != actions[:, :-1]).any(axis=(1, 2)).all()  # every env's sequence turns
    want, fallback, done = cases.oracle_table(oracle_mod, crowd, placed, gtime, actions)
    assert want.shape == (cases.B, cases.N, placed.shape[1] - 1, 2) and np.isfinite(want).all()
    unseen = cases.furthest(want, base.oracle_table(oracle_mod, crowd, placed, gtime)[0])
    stands = cases.furthest(want[:, 1:], cases.oracle_table(oracle_mod, crowd, placed, gtime, actions, robot='stands')[0][:, 1:])
    stale = cases.furthest(want, cases.oracle_table(oracle_mod, crowd, placed, gtime, actions, robot='stale')[0])
    print(crowd, 'furthest from robot unseen %.3f, robot standing (t >= 1) %.3f, stale velocity %.3f; fallback solves %d, rows '
          'behind done %d' % (unseen, stands, stale, fallback.sum(), done.sum()))
    assert unseen > 1e-3 and stands > 1e-3 and stale > 1e-3
    if crowd in ('h12', 'h20'):
        assert fallback.any()
    short = cases.oracle_table(oracle_mod, crowd, placed, gtime, actions[:, :5])[0]
    assert short.tobytes() == np.ascontiguousarray(want[:, :5]).tobytes()


def test_the_unicycle_scene_bites(oracle_mod):
    state, gtime = cases.start(oracle_mod, 'h5', robot_kinematics=1)
    placed, _, _ = cases.place_robot(state)
    actions = cases.sequences(unicycle=True)
    assert (actions[:, :, 1] != 0.0).all() and (cases.wraps(cases.THETA, actions) >= 1).any()
    kw = dict(theta=cases.THETA, robot_kinematics=1)
    want = cases.oracle_table(oracle_mod, 'h5', placed, gtime, actions, **kw)[0]
    unseen = cases.furthest(want, base.oracle_table(oracle_mod, 'h5', placed, gtime)[0])
    stands = cases.furthest(want[:, 1:], cases.oracle_table(oracle_mod, 'h5', placed, gtime, actions, robot='stands', **kw)[0][:, 1:])
    stale = cases.furthest(want, cases.oracle_table(oracle_mod, 'h5', placed, gtime, actions, robot='stale', **kw)[0])
    # ... and the rows are not read as (vx, vy), nor the heading taken as 0
    holonomic = cases.furthest(want, cases.oracle_table(oracle_mod, 'h5', placed, gtime, actions)[0])
    no_theta = cases.furthest(want, cases.oracle_table(oracle_mod, 'h5', placed, gtime, actions, robot_kinematics=1)[0])
    print('unicycle: unseen %.3f stands %.3f stale %.3f read as (vx, vy) %.3f theta 0 %.3f' % (unseen, stands, stale, holonomic, no_theta))
    assert min(unseen, stands, stale, holonomic, no_theta) > 1e-3


@pytest.mark.parametrize('crowd', ['h1', 'h5', 'h12'])
def test_the_replay_scene_bites(oracle_mod, crowd):
    """_replay_scene's K = 9 branches on an oracle whose humans see the robot: a Collision, a ReachGoal and one that runs all n."""
    from predict_orca_cases import replay_scene as _replay_scene
    state, gtime = cases.start(oracle_mod, crowd)
    placed, table = _replay_scene(state, 9, 10)
    info, steps = cases.oracle_branches(oracle_mod, crowd, placed, gtime, table)
    print('replay', crowd, 'info', info.tolist(), 'steps', steps.tolist())
    assert (info == 3).any() and (info == 2).any() and ((steps == 10) & (info < 2)).any()  # CN_COLLISION, CN_REACH_GOAL
