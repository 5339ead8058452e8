"""The kernels that came after the settings suite at environment settings other than the shipped env.config
(env_settings_planning_cases.py), on the MI355X: a. cn_predict, b. cn_predict_orca, c. cn_predict_orca_robot, d.
cn_lookahead_modes, e. the goal-progress term on every lookahead route, f. the unicycle planners, g. the one-call closed loops
on predicted futures.  Every comparison is bit for bit — against crowdnav_amd.predict, the CPU oracle or a host restatement fed
the ENGINE's dt and v_pref — but the draw's and the unicycle prior's, whose bounds are named where they are used; the loops of
(g) are held against the per-step calls (a) to (f) pin.  What each scene must contain is asserted without a device by
test_env_settings_planning_host.py.

Shapes: B = 3; n = 12 for the ORCA predictors' tables (33 for cn_predict: the seeded scenes land inside 33 steps, not 12);
K, n = (5, 33) and (70, 4) for the lookaheads and the planners; M = 3."""
import math

import numpy as np
import pytest

import env_setting_cases as settings
import env_settings_planning_cases as cases
import lookahead_cv_reference as cv
import lookahead_modes_reference as modes_ref
import plan_reference as plan_ref
import plan_unicycle_cases as uni_cases
import plan_unicycle_reference as uni
import predict_orca_robot_cases as robot_cases
from support import (  # noqa: F401  (amd: module fixture)
    amd, assert_twins_equal, begin_plan as _plan, np_of as _np, put as _put, same_bits as _same_bits, SEED,
    seeded_engine as _seeded, smoothed_plan as _smoothed)

pytestmark = pytest.mark.gpu

BY_NAME = settings.BY_NAME
B, N, M, W = cases.B, cases.N_TABLE, cases.M, cases.GOAL_WEIGHT
BEGIN = dict(seed_base=1000, seed_mod=500, record_capacity=8)
ROWS = ('ret', 'info', 'steps', 'time')
REDUCED = ('score', 'risk', 'worst_mode', 'worst_info', 'worst_steps', 'worst_time')


def _engine(amd, s, state, gtime, **extra):
    """An external-robot engine of the entry that holds (state, gtime)."""
    eng = amd.BatchedCrowdSim(num_envs=len(state), robot_policy=amd.ROBOT_EXTERNAL, **settings.engine_config(s, robot_visible=1, **extra))
    eng.set_gamma(cases.GAMMA)
    eng.set_state(state, gtime)
    assert _same_bits(eng.get_state()[0], state)
    return eng


# ------------------------------------------------------------------------------------------------ a. cn_predict
@pytest.mark.parametrize('name', cases.PREDICT_ENTRIES)
def test_predict_is_predict_py_at_the_engine_s_dt(amd, oracle_mod, name):
    s = BY_NAME[name]
    dt = cases.whole(s)['time_step']
    state, gtime, _ = cases.predict_state(oracle_mod, s)
    eng = _engine(amd, s, state, gtime)
    assert eng.config['time_step'] == dt
    for n in (N, 33):
        for models in ('to_goal', 'cv', ('to_goal', 'cv')):
            got, want = eng.predict(n, models), cases.host_table(state, n, dt, models)
            differ = _np(got) != want
            print(name, n, models, 'entries that differ:', int(differ.sum()), 'of', differ.size, np.argwhere(differ)[:3].tolist())
            assert _same_bits(got, want), (name, n, models)
    print(name, 'landing steps, misses of p + (d / dt) dt:', cases.landing_misses(state, 33, dt))


# ------------------------------------------------------------------------------------------------ b. cn_predict_orca
@pytest.mark.parametrize('name,seconds', [(n, sec) for n in cases.ORCA_ENTRIES for sec in cases.orca_scenes(n)])
def test_predict_orca_is_the_oracle_at_the_entry(amd, oracle_mod, name, seconds):
    """The entry with its oracle-only keys: the table against N steps of the CPU oracle under the same settings, humans that do
    not see the robot, fresh simulators."""
    s = BY_NAME[name]
    state, gtime = cases.orca_state(oracle_mod, s, seconds)
    want, fallback, done = cases.orca_table(oracle_mod, s, state, gtime)
    eng = _engine(amd, s, state, gtime)
    got = eng.predict_orca(N)
    differ = _np(got) != want
    print(name, seconds, 'entries that differ:', int(differ.sum()), 'of', differ.size, 'first', np.argwhere(differ)[:3].tolist(),
          'fallback solves', int(fallback.sum()))
    assert tuple(got.shape) == (B, N, s.humans, 2) and _same_bits(got, want)
    if name == 'near_sighted':  # a slot of a modes table: the other slots keep cn_predict's bits
        dt = cases.whole(s)['time_step']
        out = eng.predict(N, ('cv', 'to_goal', 'cv'))
        assert eng.predict_orca(N, out=out, mode=1) is out
        assert _same_bits(out[:, 1], want) and _same_bits(out[:, 0], cases.host_table(state, N, dt, 'cv'))
        assert _same_bits(out[:, 2], cases.host_table(state, N, dt, 'cv'))


def test_predict_orca_never_solves_the_robot_s_simulator(amd, oracle_mod):
    """Two engines that differ in robot_safety_space alone (0.15 against 0.0) give the same table: the oracle's."""
    s = BY_NAME['radii_rewards']
    state, gtime = cases.orca_state(oracle_mod, s)
    want = cases.orca_table(oracle_mod, s, state, gtime)[0]
    assert s.config['robot_safety_space'] == 0.15
    for space in (0.15, 0.0):
        eng = _engine(amd, s, state, gtime, robot_safety_space=space)
        assert eng.config['robot_safety_space'] == space
        assert _same_bits(eng.predict_orca(N), want), space


# ------------------------------------------------------------------------------------------------ c. cn_predict_orca_robot
@pytest.mark.parametrize('name,unicycle', [(n, False) for n in cases.ROBOT_SEEN_ENTRIES] + [('dt_inexact', True)])
def test_predict_orca_robot_is_the_oracle_at_the_entry(amd, oracle_mod, name, unicycle):
    import torch
    s = BY_NAME[name]
    state, gtime = cases.orca_state(oracle_mod, s)
    placed, _, _ = robot_cases.place_robot(state)
    actions = cases.robot_sequences(s, unicycle)
    kw = dict(theta=robot_cases.THETA, robot_kinematics=1) if unicycle else {}
    want, fallback, _ = cases.robot_table(oracle_mod, s, placed, gtime, actions, **kw)
    eng = _engine(amd, s, placed, gtime, **({'robot_kinematics': 1} if unicycle else {}))
    if unicycle:
        eng.set_theta(torch.as_tensor(robot_cases.THETA))
    got = eng.predict_orca_robot(N, actions)
    differ = _np(got) != want
    print(name, 'unicycle' if unicycle else 'holonomic', 'entries that differ:', int(differ.sum()), 'of', differ.size, 'first',
          np.argwhere(differ)[:3].tolist(), 'fallback solves', int(fallback.sum()))
    assert _same_bits(got, want)
    if unicycle:
        assert _same_bits(eng.get_theta(), robot_cases.THETA)


# ------------------------------------------------------------------------------------------------ d. cn_lookahead_modes
def _modes_engine(amd, oracle_mod, name, K, n):
    state, gtime, c, table, vel, want = cases.modes_case(oracle_mod, name, K, n)
    return _engine(amd, BY_NAME[name], state, gtime), state, gtime, c, table, vel, want


def _dict(out):
    return {k: _np(v) for k, v in out.items()}


@pytest.mark.parametrize('K,n', cases.SHAPES)
@pytest.mark.parametrize('name', cases.ROBOT_ENTRIES)
def test_modes_are_the_paths_call_and_the_restatement(amd, oracle_mod, name, K, n):
    eng, state, gtime, c, table, vel, want = _modes_engine(amd, oracle_mod, name, K, n)
    got = _dict(eng.lookahead_modes(table, vel, per_mode=True))
    for m in range(M):
        rows = _dict(eng.lookahead_paths(table, np.ascontiguousarray(vel[:, m])))
        for key in ROWS:
            assert _same_bits(got[key][:, :, m], rows[key]), (name, m, key)
    for key in ROWS:
        assert _same_bits(got[key], want[key]), (name, key, np.argwhere(got[key] != want[key])[:3].tolist())
    weights = modes_ref.weights_table(B, M)
    for w in (weights, None):
        for reduce in (modes_ref.MEAN, modes_ref.MIN):
            red = _dict(eng.lookahead_modes(table, vel, weights=w, reduce=reduce, risk_penalty=0.5))
            ref = modes_ref.reduced(want, w, reduce, 0.5)
            for key in REDUCED:
                assert _same_bits(red[key], ref[key]), (name, w is None, reduce, key)


# ------------------------------------------------------------------------------------------------ e. the goal term
def _route(eng, route, table, vel=None, **kw):
    if route == 'paths':
        return _dict(eng.lookahead_paths(table, vel, **kw))
    eng.set_lookahead_human_model('orca' if route == 'orca' else 'constant_velocity')
    return _dict(eng.lookahead(table, **kw))


@pytest.mark.parametrize('K,n', cases.SHAPES)
@pytest.mark.parametrize('name', cases.ROBOT_ENTRIES)
def test_goal_term_on_every_route(amd, oracle_mod, name, K, n):
    """The constant-velocity route against the restatements; ORCA, paths and modes against the same run without the term plus
    w * (d0 - d1), d0 from the state, d1 from the robot row of the call's own branch ends (test_lookahead_goal.py's rule)."""
    eng, state, gtime, c, table, vel, want_modes = _modes_engine(amd, oracle_mod, name, K, n)
    assert eng.lookahead_goal_weight == 0.0
    plain = {r: _route(eng, r, table, np.ascontiguousarray(vel[:, 2]), final_state=True) for r in ('orca', 'cv', 'paths')}
    plain_modes = _dict(eng.lookahead_modes(table, vel, per_mode=True))
    eng.set_lookahead_goal_weight(W)
    want = cv.lookahead(state, gtime, table, c, cases.GAMMA)
    got = _route(eng, 'cv', table, final_state=True)
    want_ret = want['ret'] + cases.goal_terms(W, state, want['final_state8'][:, :, 0, 0:2])
    assert _same_bits(got['ret'], want_ret), (name, np.abs(got['ret'] - want_ret).max())
    assert _same_bits(got['final_state8'], want['final_state8'])
    for r in ('orca', 'cv', 'paths'):
        got = _route(eng, r, table, np.ascontiguousarray(vel[:, 2]), final_state=True)
        want_ret = plain[r]['ret'] + cases.goal_terms(W, state, got['final_state8'][:, :, 0, 0:2])
        assert _same_bits(got['ret'], want_ret), (name, r, np.abs(got['ret'] - want_ret).max())
        assert (got['ret'] != plain[r]['ret']).any(), r
        for key in ('info', 'steps', 'time', 'final_state8', 'final_theta'):
            assert _same_bits(got[key], plain[r][key]), (name, r, key)
    # the modes: every mode's row is the paths call under the same weight, and the reductions are the header's on those rows
    rows = _dict(eng.lookahead_modes(table, vel, per_mode=True))
    for m in range(M):
        one = _route(eng, 'paths', table, np.ascontiguousarray(vel[:, m]), final_state=True)
        want_ret = plain_modes['ret'][:, :, m] + cases.goal_terms(W, state, one['final_state8'][:, :, 0, 0:2])
        assert _same_bits(rows['ret'][:, :, m], want_ret) and _same_bits(one['ret'], want_ret), (name, m)
    assert (rows['ret'] != plain_modes['ret']).any()
    for key in ('info', 'steps', 'time'):
        assert _same_bits(rows[key], plain_modes[key]) and _same_bits(rows[key], want_modes[key]), key
    weights = modes_ref.weights_table(B, M)
    for reduce in (modes_ref.MEAN, modes_ref.MIN):
        red = _dict(eng.lookahead_modes(table, vel, weights=weights, reduce=reduce, risk_penalty=0.5))
        ref = modes_ref.reduced({k: rows[k] for k in ROWS}, weights, reduce, 0.5)
        for key in REDUCED:
            assert _same_bits(red[key], ref[key]), (name, reduce, key)


@pytest.mark.parametrize('name', cases.ROBOT_ENTRIES)
def test_goal_term_in_the_bootstrap_score(amd, oracle_mod, name):
    from crowdnav_amd.compat.sarl import build_action_space
    from support import value_network
    import torch
    K, n = 5, 4
    eng, state, gtime, c, table, vel, _ = _modes_engine(amd, oracle_mod, name, 70, n)
    table = np.ascontiguousarray(table[:, :K])
    eng.sarl_configure(actions=np.array([list(a) for a in build_action_space(c['robot_v_pref'])[0]], dtype=np.float64), gamma=cases.GAMMA)
    torch.manual_seed(11)
    eng.sarl_set_weights(value_network(13).state_dict())
    for route in ('orca', 'cv', 'paths'):
        eng.set_lookahead_goal_weight(0.0)
        plain = _route(eng, route, table, np.ascontiguousarray(vel[:, 2]), bootstrap=True)
        eng.set_lookahead_goal_weight(W)
        got = _route(eng, route, table, np.ascontiguousarray(vel[:, 2]), bootstrap=True)
        for key in ('info', 'steps', 'time', 'final_state8', 'final_theta', 'value'):
            assert _same_bits(got[key], plain[key]), (name, route, key)
        want_ret = plain['ret'] + cases.goal_terms(W, state, got['final_state8'][:, :, 0, 0:2])
        assert _same_bits(got['ret'], want_ret) and (got['ret'] != plain['ret']).any(), (name, route)
        ended = got['info'] >= cv.REACH_GOAL
        assert ended.any() and not ended.all()
        for b in range(B):
            for k in range(K):
                boot = math.pow(cases.GAMMA, int(got['steps'][b, k]) * c['time_step'] * c['robot_v_pref']) * float(np.float64(got['value'][b, k]))
                score = got['ret'][b, k] if ended[b, k] else got['ret'][b, k] + boot
                assert _same_bits(got['score'][b, k], np.float64(score)), (name, route, b, k)
        assert (got['score'] != plain['score']).any()


# ------------------------------------------------------------------------------------------------ f. the unicycle planners
DT, V = cases.UNICYCLE['time_step'], cases.UNICYCLE['robot_v_pref']
R4, S = cases.ROTATION, cases.STD_ROTATION
# test_plan_unicycle.py's rule for the draw: 4 x the 5.551e-17 measured for the holonomic draw, scaled by max(v_pref, R) — the
# difference is the device libm's log / cos / sin alone, relative to max(1, r std)
DRAW_BOUND = 4 * 5.551e-17 * max(V, R4)
# The prior's floor, test_plan_unicycle.py's PRIOR_BOUND (4 x the 2.22e-15 measured at the shipped setting).  At this setting
# no device figure existed, so the rule measures the REFERENCE: E_numpy and E_device are the largest component differences of the
# float64 restatement and of the kernel from the recurrence restated in long double, and two float64 evaluations that scatter
# around that truth may lie 8 x E_numpy apart (test_train_step.py's factor); the floor covers the robots whose E_numpy is 0.
PRIOR_BOUND = 4 * 2.2204460492503131e-15


def _uni(amd, R=R4, **cfg):
    eng = _seeded(amd, B, 5, robot_kinematics=1, **dict(cases.UNICYCLE, **cfg))
    eng.set_plan_unicycle(R, S)
    assert eng.config['time_step'] == DT and np.all(_np(eng.get_state()[0])[:, 0, 7] == V)
    return eng


def _mean_std(n, seed=2):
    rng = np.random.RandomState(seed)
    mean = np.stack([rng.uniform(-0.2, 1.2, (B, n)) * V, rng.uniform(-1.0, 1.0, (B, n))], axis=-1)  # some rows outside the box
    return mean, rng.uniform(0.05, 0.3, (B, n, 2))


@pytest.mark.parametrize('K,n', [(70, 4), (5, 33)])
def test_unicycle_draw_clips_to_the_engine_s_v_pref(amd, K, n):
    eng = _uni(amd)
    mean, std = _mean_std(n)
    got = _np(eng.plan_draw(_plan(eng, K, n, mean=mean, std=std), 11))
    want = uni.draw(mean, std, K, SEED, 11, V, R4)
    _, _, r = plan_ref.normal_pairs(B, K, n, SEED, 11)
    err = np.abs(got - want) / np.maximum(1.0, r[..., None] * std[:, None])
    print('plan_draw (v, r) at v_pref %g, K=%d n=%d: largest |device - reference| / max(1, r std) = %.3e, bound %.3e' % (V, K, n, err.max(), DRAW_BOUND))
    assert err.max() <= DRAW_BOUND
    assert _same_bits(got[:, 0], uni.clip(mean, V, R4))
    wide = _np(eng.plan_draw(_plan(eng, 70, 4, mean=mean[:, :4], std=np.full((B, 4, 2), 3.0)), 7))
    assert wide[..., 0].min() == 0.0 and wide[..., 0].max() == V and wide[..., 1].min() == -R4 and wide[..., 1].max() == R4
    inside = (got[..., 0] > 0) & (got[..., 0] < V) & (np.abs(got[..., 1]) < R4)
    assert inside.any() and (got[..., 0] == V).any()


@pytest.mark.parametrize('R', uni_cases.ROTATIONS)
def test_unicycle_prior_within_the_measured_error_of_the_reference(amd, R):
    n = uni_cases.N
    eng = _uni(amd, R)
    state8, theta = cases.prior_robots(_np(eng.get_state()[0]))
    eng.set_state(state8, np.zeros(B))
    eng.set_theta(theta)
    turns = []
    uni.prior(state8, theta, DT, R, n, turns)
    assert min(math.pi - abs(t) for t in turns) >= uni_cases.TURN_MARGIN
    plan = _plan(eng, 5, n)
    mean0, std0 = _mean_std(n, seed=4)
    for mask in ([1, 0, 1], None):
        _put(plan.mean, mean0), _put(plan.std, std0)
        eng.plan_reset(plan, mask=None if mask is None else np.array(mask, np.uint8))
        want = uni.reset(state8, theta, DT, R, mean0, std0, 0.3, S, mask=mask)
        assert _same_bits(plan.std, want[1])
        got = _np(plan.mean)
        if mask is not None:
            assert _same_bits(got[1], mean0[1])  # the masked env keeps its bits
            continue
        e_numpy, e_device = cases.prior_errors(got, state8, theta, DT, R, n)
        for b in range(B):
            print('plan_reset (v, r) prior dt=%g v_pref=%g R=%.4f n=%d robot %d: E_numpy %.3e E_device %.3e bound %.3e'
                  % (DT, V, R, n, b, e_numpy[b], e_device[b], max(PRIOR_BOUND, 8 * e_numpy[b])))
        for b in range(B):
            assert e_device[b] <= max(PRIOR_BOUND, 8 * e_numpy[b]), (R, b, e_device[b], e_numpy[b])
    assert (want[0][..., 0] <= V).all() and (want[0][0, :, 0] == V).all() and (R != R4 or (want[0][2, :, 0] < V).any())
    assert _same_bits(eng.get_theta(), theta) and _same_bits(eng.get_state()[0], state8)


def test_unicycle_shift_moves_running_plans_up_bit_for_bit(amd):
    K, n = 5, 4
    eng = _uni(amd)
    bufs = eng.rollout_begin(**BEGIN)
    plan = eng.plan_reset(_plan(eng, K, n, 2))
    for s in range(4):
        eng.plan_cem(plan, 10 + s)
        eng.rollout_step(plan.action)
        before = _np(plan.mean).copy(), _np(plan.std).copy()
        active, cur_steps = _np(bufs['active']).copy(), _np(bufs['cur_steps']).copy()
        assert active.all() and (cur_steps == s + 1).all()  # time_limit 12 s: every env runs on
        state, theta = _np(eng.get_state()[0]), _np(eng.get_theta())
        eng.plan_shift(plan)
        want = uni.shift(state, theta, DT, R4, active, cur_steps, before[0], before[1], 0.3, S)
        assert _same_bits(plan.mean, want[0]) and _same_bits(plan.std, want[1]), s
        assert _same_bits(_np(plan.mean)[:, :-1], before[0][:, 1:])
    act = _np(plan.action)
    assert (act[:, 0] >= 0).all() and (act[:, 0] <= V).all() and (np.abs(act[:, 1]) <= R4).all()


def _facing_scene(eng):
    """Every env: the robot at the origin heading along +y for a goal 8 m ahead, human 1 about a metre ahead walking at it (the
    humans do not see the robot), the others at rest far away: the branches collide at different steps."""
    H = eng.H
    state = np.zeros((B, H + 1, 8))
    for h in range(H):
        state[:, h + 1] = (8.0 + 1.5 * h, 8.0, 0.0, 0.0, 8.0 + 1.5 * h, 8.0, 0.3, 1.0)
    state[:, 0] = (0.0, 0.0, 0.0, 0.0, 0.0, 8.0, 0.3, V)
    for b in range(B):
        state[b, 1] = (0.0, 0.9 + 0.1 * b, 0.0, -1.0, 0.0, -5.0, 0.3, 1.0)
    eng.set_state(state, np.zeros(B))
    eng.set_theta(np.full(B, math.pi / 2))
    return state


@pytest.mark.parametrize('update', ['cem', 'mppi'])
@pytest.mark.parametrize('K,n', [(70, 4), (5, 33)])
def test_unicycle_planners_are_draw_lookahead_update(amd, K, n, update):
    import torch
    eng = _uni(amd)
    _facing_scene(eng)
    one, parts = (eng.plan_reset(_plan(eng, K, n, 2)) for _ in range(2))
    assert (np.abs(_np(one.mean)[..., 0] - V) <= 1e-15).all()  # the prior drives at the engine's v_pref, not at 1
    if update == 'cem':
        eng.plan_cem(one, 21)
    else:
        eng.plan_mppi(one, 0.05, 21)
    cand = eng.plan_draw(parts, 21)
    look = eng.lookahead(cand)
    for k, t in look.items():
        parts.look[k].copy_(t)
    if update == 'cem':
        eng.plan_refit(parts)
    else:
        eng.plan_mppi_update(parts, 0.05)
    eng.sync()
    for k, t in parts.tensors().items():
        assert torch.equal(t, one.tensors()[k]), (update, k)
    ret = _np(look['ret'])
    print(update, K, n, 'distinct returns per env', [len(np.unique(r)) for r in ret], 'infos', np.bincount(_np(look['info']).ravel(), minlength=5).tolist())
    assert all(len(np.unique(r)) >= 2 for r in ret)  # the ranking has something to rank
    c = _np(one.candidates)
    assert c[..., 0].min() >= 0.0 and c[..., 0].max() <= V and np.abs(c[..., 1]).max() <= R4
    if update == 'mppi':
        assert _same_bits(one.action, uni.clip(_np(one.mean)[:, 0], V, R4))
    else:
        best = _np(one.order)[:, 0]
        assert _same_bits(one.action, c[np.arange(B), best, 0]) and _same_bits(one.best_score, ret[np.arange(B), best])


# ------------------------------------------------------------------------------------------------ g. the one-call closed loops
FUTURES = {'one': dict(models='to_goal', orca_mode=0), 'two': dict(models=('to_goal', 'cv'), orca_mode=1, reduce='min')}
UPDATES = {'cem': None, 'mppi': dict(temperature=1.0, fit_std=False)}


def _loop_step(eng, plan, F, U, counter, kind):
    """One real step of the loop a *_predict_*rollout call replaces, every part by its own call."""
    many = not isinstance(F['models'], str)
    if kind == 'nominal':
        eng.plan_draw(plan, counter)
    vel = eng.predict(plan.n, F['models'])
    if kind == 'orca':
        eng.predict_orca(plan.n, out=vel, mode=F['orca_mode'] if many else None)
    if kind == 'nominal':
        eng.predict_orca_robot(plan.n, plan.candidates[:, 0], out=vel, mode=F['orca_mode'] if many else None)
    if many and U is None:
        eng.plan_cem_modes(plan, vel, counter, reduce=F['reduce'])
    elif many:
        eng.plan_mppi_modes(plan, vel, U['temperature'], counter, reduce=F['reduce'], fit_std=U['fit_std'])
    elif U is None:
        eng.plan_cem_paths(plan, vel, counter)
    else:
        eng.plan_mppi_paths(plan, vel, U['temperature'], counter, fit_std=U['fit_std'])
    eng.rollout_step(plan.action)
    eng.plan_shift(plan)
    return vel


@pytest.mark.parametrize('kind,futures,update,unicycle', [('predict', 'two', 'mppi', False), ('orca', 'one', 'cem', False),
                                                          ('nominal', 'two', 'cem', False), ('predict', 'one', 'cem', True)])
def test_the_one_call_loops_hand_on_the_engine_s_dt_and_v_pref(amd, kind, futures, update, unicycle):
    """Six real steps in one call against the per-step loop on a twin engine; the episodes end at their fifth step and re-seed
    inside the call.  The per-step calls read the engine's dt and v_pref ((a) to (f)); a loop that handed its predictor or its
    prior the defaults would part from them in the first table or the first re-seeded plan."""
    import torch
    F, U = FUTURES[futures], UPDATES[update]
    steps, I = 6, 2
    made = []
    for _ in range(2):
        if unicycle:
            eng = _seeded(amd, B, 5, robot_kinematics=1, robot_visible=1, **cases.UNICYCLE_LOOP)
            eng.set_plan_unicycle(R4, S)
        else:
            eng = _seeded(amd, B, 5, robot_visible=1, **cases.LOOP)
        bufs = eng.rollout_begin(episode_limit=cases.LOOP_EPISODES, **BEGIN)
        made.append((eng, bufs, _smoothed(eng)))
    (x, xbufs, xplan), (y, ybufs, yplan) = made
    assert xplan.iterations == I and xplan.n == 4
    pred = x.plan_predict_begin(xplan, **{k: v for k, v in F.items() if k != 'orca_mode'})
    call = dict(predict=x.plan_predict_rollout, orca=x.plan_predict_orca_rollout, nominal=x.plan_predict_orca_nominal_rollout)[kind]
    assert call(xplan, pred, steps, 100, **(U or {}), **({} if kind == 'predict' else dict(orca_mode=F['orca_mode']))) is xbufs
    for s in range(steps):
        vel = _loop_step(y, yplan, F, U, 100 + s * I, kind)
    assert_twins_equal(x, xbufs, xplan, y, ybufs, yplan)
    assert torch.equal(pred.human_vel, vel.reshape(pred.human_vel.shape))
    print(kind, futures, update, 'unicycle' if unicycle else 'holonomic', 'ep_count', _np(xbufs['ep_count']).tolist(), 'active',
          _np(xbufs['active']).tolist())
    assert int(_np(xbufs['ep_count']).sum()) >= 3 and (_np(xbufs['ep_outcome'])[:, 0] == amd.TIMEOUT).any()
    v = cases.LOOP['robot_v_pref']
    act = _np(xplan.action)
    if unicycle:
        assert (act[:, 0] >= 0).all() and (act[:, 0] <= v).all() and (np.abs(act[:, 1]) <= R4).all()
    else:
        assert (np.hypot(act[:, 0], act[:, 1]) <= v * (1 + 1e-12)).all()
