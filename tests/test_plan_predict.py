"""The device predictors (cn_predict) and the closed loop on predicted futures (cn_plan_*_predict_rollout) on the GPU:
1. predict() against crowdnav_amd.predict on the host copy of the state, bit for bit; 2. nothing of the engine moves; 3. the
table feeds lookahead_paths to the bits of the constant-velocity lookahead; 4. the rollout against the per-step loop on a twin
engine (host prediction, plan_*_paths / plan_*_modes, rollout_step, plan_shift), bit for bit on everything either leaves behind;
5. n_real = 0 and chunked calls; 6. the refusals that need an engine; 7. the example prints the same line either way."""
import ctypes as C

import numpy as np
import pytest

import plan_predict_cases as cases
from support import (  # noqa: F401  (amd: module fixture)
    amd, assert_twins_equal as _assert_twins_equal, example_line as _example_line, np_of as _np, roll_on as _roll_on,
    same_bits as _same_bits, sarl_engine, seeded_engine as _engine, smoothed_plan as _plan, snapshot as _snapshot)

pytestmark = pytest.mark.gpu

BEGIN = dict(seed_base=1000, seed_mod=500, record_capacity=8)
DT = cases.DT
MODELS = {'cv': 'cv', 'to_goal': 'to_goal', 'two': ('cv', 'to_goal'), 'eight': ('cv', 'to_goal') * 4}


def _advance(eng, steps=3):
    external = eng.config['robot_policy'] == 0
    for _ in range(steps):
        eng.step(np.tile([0.3, 0.2], (eng.B, 1)) if external else None, update=True, want_obs=False)


def _host_table(state8, n, models):
    """What crowdnav_amd.predict gives on a numpy state: [B, n, H, 2] for a name, [B, M, n, H, 2] for a sequence."""
    from crowdnav_amd import predict
    one = lambda name: predict.constant_velocity(state8, n) if name == 'cv' else predict.to_goal(state8, n, DT)  # noqa: E731
    return one(models) if isinstance(models, str) else predict.stack_modes(*(one(name) for name in models))


# ------------------------------------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize('H', [1, 5, 12])
def test_predict_is_predict_py_bit_for_bit(amd, H):
    """Seeded scenarios advanced three ORCA steps (humans under way, with velocities, none at its goal), and the last env set to
    the crafted scene that takes to_goal through all four cases of its rule (test_plan_predict_host.py counts them)."""
    B = 3
    eng = _engine(amd, B, H)
    _advance(eng)
    state, gtime = (_np(t).copy() for t in eng.get_state())
    state[B - 1] = cases.crafted_state(H)
    eng.set_state(state, gtime)
    state = _np(eng.get_state()[0]).copy()  # the host copy the oracle reads
    assert _same_bits(state[B - 1], cases.crafted_state(H)) and (state[:B - 1, 1:, 2:4] != 0.0).any()
    for n in (1, 6, 13):
        for key, models in sorted(MODELS.items()):
            got, want = eng.predict(n, models), _host_table(state, n, models)
            M = None if isinstance(models, str) else len(models)
            assert tuple(got.shape) == ((B, n, H, 2) if M is None else (B, M, n, H, 2))
            assert _same_bits(got, want), (H, n, key, np.argwhere(_np(got) != want)[:4])
    if H == 5:
        counted = cases.to_goal_cases(state[B - 1:], 6, DT)
        assert counted == dict(zero=19, exact=1, short=2, cruise=8), counted
    # `out` is written where it lies; one name is the sequence of that one name without the M axis
    import torch
    out = torch.full((B, 2, 6, H, 2), -7.0, dtype=torch.float64, device=eng.device)
    assert eng.predict(6, ('to_goal', 'cv'), out=out) is out and _same_bits(out, _host_table(state, 6, ('to_goal', 'cv')))
    assert _same_bits(eng.predict(6, ('to_goal',))[:, 0], _host_table(state, 6, 'to_goal'))
    assert _same_bits(eng.predict(6, 'constant_velocity'), _host_table(state, 6, 'cv'))
    assert tuple(eng.predict(0, 'cv').shape) == (B, 0, H, 2)


def test_predict_gives_the_parked_placeholders_zeros(amd):
    B, H, n = 3, 5, 6
    eng = _engine(amd, B, H, scenario_rule=2)
    state = _np(eng.get_state()[0]).copy()
    parked = state[:, 1:, 0] >= 1.0e5
    assert (_np(eng.human_count()) < H).any() and parked.any() and not parked.all()
    for models in (('cv', 'to_goal'), 'to_goal', 'cv'):
        got, want = _np(eng.predict(n, models)), _host_table(state, n, models)
        assert _same_bits(got, want)
        rows = got if got.ndim == 5 else got[:, None]
        there = np.broadcast_to(parked[:, None, None, :, None], rows.shape)
        assert (rows[there].view(np.uint64) == 0).all()  # exactly +0.0
    assert (_np(eng.predict(n, 'to_goal'))[:, 0][~parked] != 0.0).any()


# ------------------------------------------------------------------------------------------------ 2. a reader
@pytest.mark.parametrize('kind', ['external', 'orca_robot', 'unicycle'])
def test_predict_moves_nothing_of_the_engine(amd, kind):
    import torch
    B, H, n = 3, 5, 6
    cfg = dict(external={}, orca_robot=dict(robot_policy=amd.ROBOT_ORCA), unicycle=dict(robot_kinematics=1))[kind]
    eng = _engine(amd, B, H, **cfg)
    bufs = eng.rollout_begin(**BEGIN)
    _roll_on(eng, kind, 3)
    if kind == 'external':
        eng.set_lookahead_human_model('constant_velocity')
    before, io_before = _snapshot(eng), {k: v.clone() for k, v in bufs.items()}
    counts, model = eng.launch_counts(), eng.lookahead_human_model
    state = _np(before[0]).copy()
    for models in ('cv', 'to_goal', MODELS['two'], MODELS['eight']):
        assert _same_bits(eng.predict(n, models), _host_table(state, n, models))
    assert eng.launch_counts() == counts and 'lagged_fills' in counts and eng.lookahead_human_model == model
    for a, b in zip(before, _snapshot(eng)):
        assert torch.equal(a, b)
    for k, v in io_before.items():
        assert torch.equal(v, bufs[k]), k
    # ... and the rollout goes on as if the calls had not been made
    twin = _engine(amd, B, H, **cfg)
    tbufs = twin.rollout_begin(**BEGIN)
    _roll_on(twin, kind, 4)
    _roll_on(eng, kind, 1)
    for a, b in zip(_snapshot(eng), _snapshot(twin)):
        assert torch.equal(a, b)
    for k, v in tbufs.items():
        assert torch.equal(v, bufs[k]), k


# ------------------------------------------------------------------------------------------------ 3. composition
def test_the_cv_table_feeds_lookahead_paths_to_the_bits_of_the_cv_lookahead(amd):
    import torch
    B, H, K, n = 3, 5, 70, 13
    eng = _engine(amd, B, H, discomfort_dist=0.5)
    _advance(eng)
    rng = np.random.RandomState(11)
    actions = rng.uniform(-0.7, 0.7, (B, K, n, 2))
    actions[:, 0] = (0.0, 1.0)
    actions = torch.from_numpy(actions).to(eng.device)
    got = eng.lookahead_paths(actions, eng.predict(n, 'cv'), final_state=True)
    eng.set_lookahead_human_model('constant_velocity')
    want = eng.lookahead(actions, final_state=True)
    assert sorted(got) == sorted(want)
    for k, v in want.items():
        assert torch.equal(v, got[k]), k
    assert len(np.unique(_np(got['info']))) >= 2  # the branches do meet the humans


# ------------------------------------------------------------------------------------------------ 4. the closed loop
def _sarl_engine(amd, B, H=5, **cfg):
    return sarl_engine(amd, B, H, weights='seeded', **cfg)


WEIGHTS = np.array([[0.75, 0.25], [0.5, 0.5], [0.125, 0.875]])
FUTURES = {'one': dict(models='to_goal'),
           'mean': dict(models=('cv', 'to_goal'), reduce='mean', risk_penalty=0.5, weights=WEIGHTS),
           'min': dict(models=('cv', 'to_goal'), reduce='min', risk_penalty=0.5, weights=WEIGHTS),
           'one_bootstrap': dict(models='to_goal')}
UPDATES = {'cem': None, 'mppi': dict(temperature=1.0, fit_std=False), 'mppi_fit_std': dict(temperature=1.0, fit_std=True)}
LOOPS = [(f, u) for f in ('one', 'mean', 'min') for u in sorted(UPDATES)] + [('one_bootstrap', 'cem')]


def _host_step(eng, plan, futures, update, counter, n):
    """One step of the loop the rollout replaces: the prediction made on the HOST from get_state()."""
    state = _np(eng.get_state()[0])
    vel = _host_table(state, n, futures['models'])
    extra = {k: futures[k] for k in ('weights', 'reduce', 'risk_penalty') if k in futures}
    if update is None:
        (eng.plan_cem_modes if extra else eng.plan_cem_paths)(plan, vel, counter, **extra)
    else:
        (eng.plan_mppi_modes if extra else eng.plan_mppi_paths)(plan, vel, update['temperature'], counter, fit_std=update['fit_std'], **extra)
    eng.rollout_step(plan.action)
    eng.plan_shift(plan)
    return vel


def _twins(amd, futures, time_limit, episode_limit, B=3):
    made = []
    for _ in range(2):
        boot = futures == 'one_bootstrap'
        eng = _sarl_engine(amd, B, time_limit=time_limit) if boot else _engine(amd, B, time_limit=time_limit)
        bufs = eng.rollout_begin(episode_limit=episode_limit, **BEGIN)
        made.append((eng, bufs, _plan(eng, bootstrap=boot)))
    return made


@pytest.mark.parametrize('time_limit,episode_limit', [(1.0, 17), (2.0, 5)])
@pytest.mark.parametrize('futures,update', LOOPS)
def test_rollout_is_the_python_loop(amd, futures, update, time_limit, episode_limit):
    """test_plan.py's method and its two regimes.  time_limit 1.0 s: every step ends its episode in Timeout, so every prediction
    after the first is made from a NEW scenario and the shift only re-seeds; of 17 episodes env 2 gets five and retires one
    step before the call ends.  time_limit 2.0 s: five-step episodes, the plans of running envs shift; of 5 episodes env 2 gets
    one and retires at step five."""
    B, n, I, steps, counter = 3, 4, 2, 6, 100
    (x, xbufs, xplan), (y, ybufs, yplan) = _twins(amd, futures, time_limit, episode_limit)
    F, U = FUTURES[futures], UPDATES[update]
    pred = x.plan_predict_begin(xplan, **F)
    assert x.plan_predict_rollout(xplan, pred, steps, counter, **(U or {})) is xbufs
    for s in range(steps):
        vel = _host_step(y, yplan, F, U, counter + s * I, n)
    _assert_twins_equal(x, xbufs, xplan, y, ybufs, yplan)
    # the scratch table holds the prediction the last planning step scored against
    assert _same_bits(pred.human_vel, vel.reshape(_np(pred.human_vel).shape))
    print(futures, update, 'ep_count', _np(xbufs['ep_count']).tolist(), 'active', _np(xbufs['active']).tolist(),
          'outcome', _np(xbufs['ep_outcome'])[:, :2].tolist())
    assert x.launch_counts()['rollout_kernels'] >= steps
    if time_limit == 1.0:
        assert _np(xbufs['ep_count']).tolist() == [6, 6, 5] and _np(xbufs['active'])[2] == 0
    else:  # every first episode has ended by step five, so the five episodes are dealt and the last env to end one retires
        assert int(_np(xbufs['ep_count']).sum()) >= 3 and int((_np(xbufs['active']) == 0).sum()) >= 1
    if futures == 'one_bootstrap' and time_limit == 2.0:  # (at 1.0 s every branch ends in Timeout and gets no bootstrap)
        assert not np.array_equal(_np(xplan.look['score']), _np(xplan.look['ret']))  # the bootstrap says something


# ------------------------------------------------------------------------------------------------ 5. no steps, and chunks
@pytest.mark.parametrize('futures,update', [('one', 'cem'), ('min', 'mppi_fit_std')])
def test_no_steps_is_a_no_op_and_chunks_add_up(amd, futures, update):
    import torch
    I, counter = 2, 100
    (x, xbufs, xplan), (y, ybufs, yplan) = _twins(amd, futures, 2.0, 5)
    F, U = FUTURES[futures], UPDATES[update] or {}
    xpred, ypred = x.plan_predict_begin(xplan, **F), y.plan_predict_begin(yplan, **F)
    xpred.human_vel.fill_(-7.0)
    keep, counts, before = {k: v.clone() for k, v in xplan.tensors().items()}, x.launch_counts(), _snapshot(x)
    assert x.plan_predict_rollout(xplan, xpred, 0, counter, **U) is xbufs
    assert x.launch_counts() == counts and bool((xpred.human_vel == -7.0).all())
    for a, b in zip(before, _snapshot(x)):
        assert torch.equal(a, b)
    for k, v in keep.items():
        assert torch.equal(v, xplan.tensors()[k]), k
    x.plan_predict_rollout(xplan, xpred, 3, counter, **U)
    x.plan_predict_rollout(xplan, xpred, 3, counter + 3 * I, **U)
    y.plan_predict_rollout(yplan, ypred, 6, counter, **U)
    _assert_twins_equal(x, xbufs, xplan, y, ybufs, yplan)
    assert torch.equal(xpred.human_vel, ypred.human_vel) and not bool((xpred.human_vel == -7.0).any())


# ------------------------------------------------------------------------------------------------ 6. refusals on an engine
def test_refusals_on_an_engine(amd):
    import torch
    lib = amd._lib
    INV, UNS = lib.CN_ERR_INVALID, lib.CN_ERR_UNSUPPORTED
    two = dict(models=('cv', 'to_goal'))

    def refused(eng, plan, pred, status, *words, after=None):
        pred.human_vel.fill_(-7.0)
        eng.sync()
        counts, keep = eng.launch_counts(), {k: v.clone() for k, v in plan.tensors().items()}
        for name, args in (('cn_plan_cem_predict_rollout', {}), ('cn_plan_mppi_predict_rollout', dict(temperature=1.0))):
            with pytest.raises(amd.CrowdNavAmdError) as ei:
                eng.plan_predict_rollout(plan, pred, 2, 3, **args)
            text = str(ei.value)
            assert ei.value.status == status and (after or name) in text and all(w in text for w in words), (name, text)
        eng.sync()
        assert eng.launch_counts() == counts and bool((pred.human_vel == -7.0).all())  # nothing enqueued, the table untouched
        for k, v in keep.items():
            assert torch.equal(v, plan.tensors()[k]), k

    # the engines no cn_plan_* call serves — cn_predict itself serves both (test_predict_moves_nothing_of_the_engine)
    orca = amd.BatchedCrowdSim(num_envs=3, num_humans=5, robot_policy=amd.ROBOT_ORCA)
    orca.rollout_begin(**BEGIN)
    plan = orca.plan_begin(5, 4, 2, 1, 0.3)
    for F in (dict(models='to_goal'), two):
        refused(orca, plan, orca.plan_predict_begin(plan, **F), INV, 'CN_ROBOT_EXTERNAL')
    uni = _engine(amd, 3, robot_kinematics=1)
    uni.rollout_begin(**BEGIN)
    plan = uni.plan_begin(5, 4, 2, 1, 0.3)
    for F in (dict(models='to_goal'), two):
        refused(uni, plan, uni.plan_predict_begin(plan, **F), UNS, 'CN_UNICYCLE')
    # bootstrap with M = 2: the branch-end states are per mode (M = 1 serves it: test_rollout_is_the_python_loop)
    boot = _sarl_engine(amd, 3)
    boot.rollout_begin(**BEGIN)
    plan = _plan(boot, bootstrap=True)
    refused(boot, plan, boot.plan_predict_begin(plan, **two), UNS, 'bootstrap')
    # a reduce that is neither value, a risk penalty below zero (python checks the names; the struct by hand): M > 1 only
    eng = _engine(amd, 3)
    bufs = eng.rollout_begin(**BEGIN)
    plan = _plan(eng)
    pred = eng.plan_predict_begin(plan, **two)
    pred.c.reduce = 7
    refused(eng, plan, pred, INV, 'reduce 7 unknown', after='cn_lookahead_modes')
    pred.c.reduce, pred.c.risk_penalty = lib.MODES_MIN, -1.0
    refused(eng, plan, pred, INV, 'risk_penalty', after='cn_lookahead_modes')
    one = eng.plan_predict_begin(plan, 'to_goal')
    one.c.reduce, one.c.risk_penalty = 7, -1.0  # not read with M = 1
    eng.plan_predict_rollout(plan, one, 1, 0)
    # the models, the step count and the io block, on a live engine
    pred.c.risk_penalty = 0.0
    pred.c.model[1] = 4
    refused(eng, plan, pred, INV, 'model[1] = 4 unknown')
    pred.c.model[1] = lib.PREDICT_TO_GOAL
    pred.human_vel.fill_(-7.0)
    with pytest.raises(amd.CrowdNavAmdError, match='n_real_steps') as ei:
        eng.plan_predict_rollout(plan, pred, -1, 0)
    assert ei.value.status == INV
    L, io = lib.load(), eng._rollout[0]
    bad = lib.CnRolloutIo.from_buffer_copy(io)
    bad.seed_base = io.seed_base + 1
    assert L.cn_plan_cem_predict_rollout(eng._h, C.byref(bad), 2, C.byref(plan.cfg), C.byref(plan.c), C.byref(pred.c), 0) == INV
    assert 'cn_rollout_begin' in L.cn_last_error().decode()
    assert L.cn_plan_mppi_predict_rollout(eng._h, None, 2, C.byref(plan.cfg), C.byref(plan.c), C.byref(pred.c), 1.0, 0, 0) == INV
    assert 'io is NULL' in L.cn_last_error().decode()
    eng.sync()
    assert bool((pred.human_vel == -7.0).all()) and _np(bufs['cur_steps']).tolist() == [1, 1, 1]
    fresh = _engine(amd, 3)
    fplan = _plan(fresh)
    with pytest.raises(RuntimeError, match='rollout_begin'):
        fresh.plan_predict_rollout(fplan, fresh.plan_predict_begin(fplan, 'cv'), 1, 0)
    with pytest.raises(ValueError, match='plan_begin'):
        fresh.plan_predict_rollout(plan, pred, 1, 0)  # another engine's plan
    # cn_predict on a live engine: the table's rows beyond an int
    models = (C.c_int32 * 8)(*[0, 1] * 4)
    assert L.cn_predict(eng._h, 2 ** 31 - 1, 8, models, C.c_void_p(pred.human_vel.data_ptr())) == UNS
    assert 'cn_predict' in L.cn_last_error().decode() and 'rows exceed' in L.cn_last_error().decode()
    assert L.cn_predict(eng._h, 0, 8, models, C.c_void_p(pred.human_vel.data_ptr())) == lib.CN_OK
    eng.sync()
    assert bool((pred.human_vel == -7.0).all())


# ------------------------------------------------------------------------------------------------ 7. the example
EXAMPLE = {'to_goal': ['--predictor', 'to_goal'],
           'futures_min_mppi': ['--futures', 'cv,to_goal', '--reduce', 'min', '--risk-penalty', '0.5', '--mppi']}
_host_lines = {}


@pytest.mark.parametrize('chunk', [[], ['--chunk', '3']], ids=['chunk8', 'chunk3'])
@pytest.mark.parametrize('case', sorted(EXAMPLE))
def test_the_example_prints_the_same_line_with_the_device_loop(amd, case, chunk):
    if case not in _host_lines:  # the per-step loop through the host: run once per case
        _host_lines[case] = _example_line(EXAMPLE[case])
    got = _example_line(EXAMPLE[case] + ['--device-loop'] + chunk)
    print(case, chunk, got)
    assert got == _host_lines[case]
