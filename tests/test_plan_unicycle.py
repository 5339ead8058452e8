"""The device planners on a unicycle engine (cn_plan_set_unicycle; rows (v, r)) on the MI355X:
1. the gate: refused until the setter is called, served afterwards; the setter's refusals; a holonomic engine is left alone;
2. the draw: invariances, the box, parity with tests/plan_unicycle_reference.py;
3. reset and shift against the restatement (the prior within the measured bound, everything else bit for bit);
4. the refit and the MPPI update on (v, r) candidates, bit for bit;
5. plan_cem / plan_mppi = draw + lookahead + update, nothing of the engine moved; I = 3; the best sequence replayed;
6. every planner family once against its per-step composition on a twin engine;
7. the closed loops against the Python loop on a twin;   8. goal weight and bootstrap;   9. the examples.
The lookaheads, the predictors and the real step serve unicycle engines already and are never the code under test here.

Shapes: the planner suites' smallest — B = 3; 5 humans (1 and 12 where stated); K = 5 and 70; n = 4 and 33."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden

import plan_reference as ref
import plan_unicycle_cases as cases
import plan_unicycle_reference as uni
from support import (  # noqa: F401  (amd: module fixture)
    action_space, amd, assert_twins_equal, begin_plan as _plan, np_of as _np, put as _put, same_bits as _same_bits, SEED,
    seeded_engine as _engine, snapshot as _snapshot)

pytestmark = pytest.mark.gpu

BEGIN = dict(seed_base=1000, seed_mod=500, record_capacity=8)
DT, V_PREF = cases.DT, cases.V_PREF
R4, S = math.pi / 4, 0.2  # the reference's action-space bound; the rotation's initial deviation
# The holonomic draw's bound (tests/test_plan.py: 4 x the measured 5.551e-17 of profiles/plan_cem_parity.txt), scaled by max(v_pref, R):
# the difference is the device libm's log / cos / sin alone, and the components are of that size.
DRAW_BOUND = 4 * 5.551e-17 * max(V_PREF, R4)
# The prior: atan2 / cos / sin of the device libm through an n-step recurrence, for which no bound can be derived.  Largest
# component difference against the restatement at n = 33 over plan_unicycle_cases' robots and both rotation bounds, measured on
# the MI355X (profiles/plan_unicycle_parity.txt); the bound is 4 x that, the rule DESIGN.md 3.8.4 set for the draw.
PRIOR_MEASURED = 2.2204460492503131e-15
PRIOR_BOUND = 4 * PRIOR_MEASURED
OUTPUTS = ('order', 'best_actions', 'best_score', 'action', 'mean', 'std')
STRAIGHT = [1.0, 0.0]  # (v, r): full speed along the heading, which starts at pi / 2 — from (0, -4) towards (0, 4)


def _uni(amd, B=3, H=5, R=R4, std_rotation=S, **cfg):
    """A seeded unicycle engine opted in to the planners."""
    eng = _engine(amd, B, H, robot_kinematics=1, **cfg)
    eng.set_plan_unicycle(R, std_rotation)
    return eng


def _mean_std(B, n, seed=1):
    rng = np.random.RandomState(seed)
    mean = np.stack([rng.uniform(-0.2, 1.2, (B, n)), rng.uniform(-1.0, 1.0, (B, n))], axis=-1)  # some rows outside the box
    return mean, rng.uniform(0.05, 0.3, (B, n, 2))


# ------------------------------------------------------------------------------------------------ 1. the gate
def test_the_gate(amd):
    import torch
    UNS, INV = amd._lib.CN_ERR_UNSUPPORTED, amd._lib.CN_ERR_INVALID
    eng = _engine(amd, 3, robot_kinematics=1)
    bufs = eng.rollout_begin(**BEGIN)
    plan = _plan(eng)
    vel = eng.predict(plan.n, 'to_goal')
    assert eng.plan_unicycle == (0.0, 0.0)
    keep, counts = {k: v.clone() for k, v in plan.tensors().items()}, eng.launch_counts()
    calls = dict(plan_reset=lambda: eng.plan_reset(plan), plan_cem=lambda: eng.plan_cem(plan, 3),
                 plan_mppi=lambda: eng.plan_mppi(plan, 1.0, 3), plan_cem_paths=lambda: eng.plan_cem_paths(plan, vel, 3),
                 plan_rollout=lambda: eng.plan_rollout(plan, 2, 3))
    for name, call in calls.items():
        with pytest.raises(amd.CrowdNavAmdError, match='CN_UNICYCLE engines are not served') as ei:
            call()
        assert ei.value.status == UNS and 'cn_' + name in str(ei.value) and 'cn_plan_set_unicycle' in str(ei.value), name
    eng.sync()
    assert eng.launch_counts() == counts and all(torch.equal(v, plan.tensors()[k]) for k, v in keep.items())
    # the setter's refusals, in the header's order; nothing is set by a refused call
    for bad in (math.nan, math.inf, 0.0, -0.5, np.nextafter(math.pi, 4.0)):
        with pytest.raises(amd.CrowdNavAmdError, match='max_rotation') as ei:
            eng.set_plan_unicycle(bad, math.nan)  # a bad max_rotation is named before a bad init_std_rotation
        assert ei.value.status == INV and 'init_std_rotation' not in str(ei.value)
    for bad in (math.nan, math.inf, 0.0, -0.1):
        with pytest.raises(amd.CrowdNavAmdError, match='init_std_rotation') as ei:
            eng.set_plan_unicycle(R4, bad)
        assert ei.value.status == INV
    assert eng.plan_unicycle == (0.0, 0.0)
    orca = amd.BatchedCrowdSim(num_envs=3, num_humans=5, robot_policy=amd.ROBOT_ORCA)  # (cn_create refuses a unicycle ORCA robot)
    for other in (orca, _engine(amd, 3)):
        with pytest.raises(amd.CrowdNavAmdError, match='cn_plan_set_unicycle is for CN_UNICYCLE engines') as ei:
            other.set_plan_unicycle(R4, S)
        assert ei.value.status == INV and other.plan_unicycle == (0.0, 0.0)
        with pytest.raises(amd.CrowdNavAmdError, match='max_rotation'):  # ... behind the arguments' own refusals
            other.set_plan_unicycle(-1.0, S)
    # after the setter every call runs; pi itself is a rotation bound
    eng.set_plan_unicycle(math.pi, 0.3)
    eng.set_plan_unicycle(R4, S)
    assert eng.plan_unicycle == (R4, S)
    for call in calls.values():
        call()
    eng.sync()
    assert _np(bufs['cur_steps']).tolist() == [2, 2, 2] and eng.launch_counts() != counts
    assert _np(plan.std)[0, 0].tolist() == [0.3, S]  # the shift's (init_std, init_std_rotation)
    eng.reset(1000 + np.arange(3))
    assert eng.plan_unicycle == (R4, S)  # the setting survives reset()
    fresh = _plan(eng)
    assert _np(fresh.std)[0, 0].tolist() == [0.3, S] and eng.plan_reset(fresh) is fresh


def test_a_holonomic_engine_is_left_alone(amd):
    """Two holonomic twins, one of which has had the setter refused: every plan output is bit for bit the same."""
    import torch
    made = []
    for attempt in (True, False):
        eng = _engine(amd, 3, time_limit=2.0)
        bufs = eng.rollout_begin(episode_limit=5, **BEGIN)
        if attempt:
            with pytest.raises(amd.CrowdNavAmdError):
                eng.set_plan_unicycle(R4, S)
        plan = eng.plan_reset(_plan(eng, I=2, smoothing=0.25, min_std=0.01))
        eng.plan_cem(plan, 5)
        eng.plan_mppi(plan, 1.0, 7, fit_std=True)
        eng.plan_rollout(plan, 3, 9)
        eng.plan_mppi_rollout(plan, 3, 1.0, 15)
        made.append((eng, bufs, plan))
    assert_twins_equal(*made[0], *made[1])
    assert torch.equal(made[0][2].action, made[1][2].action) and made[0][0].plan_unicycle == (0.0, 0.0)


# ------------------------------------------------------------------------------------------------ 2. the draw
@pytest.mark.parametrize('R', cases.ROTATIONS)
def test_draw_invariances_and_the_box(amd, R):
    import torch
    eng, two = _uni(amd, 3, R=R), _uni(amd, 2, R=R)
    mean, std = _mean_std(3, 4)
    mean[1, 2], mean[2, 0], mean[0, 1] = (3.0, -4.0), (-0.9, 0.8), (0.5, 0.05)  # two rows outside the box, one inside
    draw = lambda e, K, n, c=7, m=mean, s=std: e.plan_draw(_plan(e, K, n, mean=m[:e.B, :n], std=s[:e.B, :n]), c).clone()  # noqa: E731
    nine = draw(eng, 9, 4)
    assert nine.shape == (3, 9, 4, 2) and nine.dtype == torch.float64
    assert _same_bits(nine[:, 0], uni.clip(mean, V_PREF, R))  # candidate 0 is the clipped mean: k = 0 is clipped too
    assert _same_bits(nine[0, 0, 1], mean[0, 1]) and _np(nine)[1, 0, 2].tolist() == [V_PREF, -R]  # inside: its bits; outside: the corner
    assert torch.equal(draw(eng, 5, 4), nine[:, :5])       # a row depends on neither K ...
    assert torch.equal(draw(eng, 9, 1), nine[:, :, :1])    # ... nor n ...
    assert torch.equal(draw(two, 9, 4), nine[:2])          # ... nor B
    assert torch.equal(draw(eng, 9, 4), nine)
    other = draw(eng, 9, 4, c=8)                            # another counter: candidate 0 stays, the drawn rows move
    assert torch.equal(other[:, 0], nine[:, 0]) and not torch.equal(other[:, 1:], nine[:, 1:])
    seventy = draw(eng, 70, 4)
    assert torch.equal(seventy[:, :9], nine)
    still = draw(eng, 9, 4, s=np.zeros_like(std))
    assert torch.equal(still, nine[:, :1].expand(-1, 9, -1, -1))  # std = 0: the clipped mean in every row
    wide = _np(draw(eng, 70, 4, s=np.full_like(std, 3.0)))
    assert wide[..., 0].min() == 0.0 and wide[..., 0].max() == V_PREF and wide[..., 1].min() == -R and wide[..., 1].max() == R
    drawn = _np(seventy)
    inside = (drawn[..., 0] > 0) & (drawn[..., 0] < V_PREF) & (np.abs(drawn[..., 1]) < R)
    print('R = %.4f: rows of 3 x 70 x 4 strictly inside the box: %d' % (R, int(inside.sum())))
    assert inside.any()


@pytest.mark.parametrize('K,n', [(70, 4), (5, 33)])
def test_draw_against_the_reference(amd, K, n):
    eng = _uni(amd, 3)
    mean, std = _mean_std(3, n, seed=2)
    got = _np(eng.plan_draw(_plan(eng, K, n, mean=mean, std=std), 11))
    want = uni.draw(mean, std, K, SEED, 11, V_PREF, R4)
    _, _, r = ref.normal_pairs(3, K, n, SEED, 11)
    err = np.abs(got - want) / np.maximum(1.0, r[..., None] * std[:, None])
    edge = (want[..., 0] == 0.0) | (want[..., 0] == V_PREF) | (np.abs(want[..., 1]) == R4)
    print('plan_draw (v, r) parity K=%d n=%d: largest |device - reference| / max(1, r std) = %.3e (rows on the box\'s edge: %d of %d)'
          % (K, n, err.max(), int(edge.sum()), edge.size))
    assert DRAW_BOUND < 1e-9 and err.max() <= DRAW_BOUND
    assert edge.any() and not edge.all()


# ------------------------------------------------------------------------------------------------ 3. reset and shift
def _margin(state8, theta, R, n):
    turns = []
    uni.prior(state8, theta, DT, R, n, turns)
    return min(math.pi - abs(t) for t in turns)


@pytest.mark.parametrize('R', cases.ROTATIONS)
def test_reset_against_the_reference(amd, R):
    B, n = 3, cases.N
    eng = _uni(amd, B, R=R)
    state8, theta = cases.install(_np(eng.get_state()[0]))
    eng.set_state(state8, np.zeros(B))
    eng.set_theta(theta)
    assert _margin(state8, theta, R, n) >= cases.TURN_MARGIN  # (asserted without a device by the host suite, too)
    plan = _plan(eng, 5, n)
    mean0, std0 = _mean_std(B, n, seed=4)
    _put(plan.mean, mean0), _put(plan.std, std0)
    eng.plan_reset(plan, mask=np.array([1, 0, 1], np.uint8))
    want = uni.reset(state8, theta, DT, R, mean0, std0, 0.3, S, mask=[1, 0, 1])
    err = np.abs(_np(plan.mean) - want[0])
    print('plan_reset (v, r) parity R=%.4f n=%d: largest |device - reference| = %.3e (per env %s), bound %.3e'
          % (R, n, err.max(), err.max(axis=(1, 2)).tolist(), PRIOR_BOUND))
    assert _same_bits(plan.std, want[1]) and _same_bits(plan.mean[1], mean0[1])  # std; the masked env: bit for bit
    assert err.max() <= PRIOR_BOUND
    eng.plan_reset(plan)
    want = uni.reset(state8, theta, DT, R, mean0, std0, 0.3, S)
    assert _same_bits(plan.std, want[1]) and np.abs(_np(plan.mean) - want[0]).max() <= PRIOR_BOUND
    assert (np.abs(want[0][1, :3, 1]) == R).all() and (want[0][2, :, 0] < V_PREF).any()  # the cases are what they claim to be
    assert _same_bits(eng.get_theta(), theta) and _same_bits(eng.get_state()[0], state8)  # nothing of the engine moved


def test_shift_against_the_reference(amd):
    """Six real steps on an engine whose episodes time out at their fifth step: the shift meets running envs (row t <- row
    t + 1, bit for bit), envs whose episode has just ended (the prior of the new scenario, heading pi / 2) and a retired one."""
    B, K, n = 3, 5, 4
    eng = _uni(amd, B, time_limit=2.0)
    bufs = eng.rollout_begin(episode_limit=5, **BEGIN)
    plan = eng.plan_reset(_plan(eng, K, n, 2, init_std=0.3))
    seen = set()
    for s in range(6):
        eng.plan_cem(plan, 10 + s)
        eng.rollout_step(plan.action)
        before = _np(plan.mean).copy(), _np(plan.std).copy()
        active, cur_steps = _np(bufs['active']).copy(), _np(bufs['cur_steps']).copy()
        state, theta = _np(eng.get_state()[0]), _np(eng.get_theta())
        eng.plan_shift(plan)
        want = uni.shift(state, theta, DT, R4, active, cur_steps, before[0], before[1], 0.3, S)
        got = _np(plan.mean)
        assert _same_bits(plan.std, want[1]), s
        for b in range(B):
            kind = 'retired' if not active[b] else 'ended' if cur_steps[b] == 0 else 'running'
            seen.add(kind)
            if kind == 'ended':  # re-seeded: the prior from its new state and theta = pi / 2
                assert theta[b] == cases.RESEED_THETA and _margin(state[b:b + 1], theta[b:b + 1], R4, n) >= cases.TURN_MARGIN
                assert np.abs(got[b] - want[0][b]).max() <= PRIOR_BOUND and (want[0][b, :, 0] == V_PREF).all(), (s, b)
            else:  # shifted rows, and a retired env's plan (std included): bit for bit
                assert _same_bits(got[b], want[0][b]), (s, b, kind)
            if kind == 'retired':
                assert _same_bits(got[b], before[0][b]) and _same_bits(_np(plan.std)[b], before[1][b])
            if kind == 'running':
                assert _same_bits(got[b, :-1], before[0][b, 1:]) and _same_bits(got[b, -1], before[0][b, -1])
    assert seen == {'retired', 'ended', 'running'}, seen


# ------------------------------------------------------------------------------------------------ 4. refit and MPPI update
@pytest.mark.parametrize('K,n,E', [(5, 4, 2), (70, 33, 64)])
def test_refit_against_the_reference(amd, K, n, E):
    B = 3
    eng = _uni(amd, B)
    mean, std = _mean_std(B, n, seed=3)
    plan = _plan(eng, K, n, E, mean=mean, std=std, smoothing=0.5, min_std=0.08)
    cand = _np(eng.plan_draw(plan, 5)).copy()  # the device's own (v, r) candidates
    scores = np.random.RandomState(K + n).randint(0, 4, (B, K)) / 4.0 - 0.5  # four levels: exact ties everywhere
    scores[2] = 0.25
    held = dict(best_actions=np.full((B, n, 2), 7.0), best_score=np.array([100.0, -100.0, 0.25]), action=np.full((B, 2), 7.0))
    _put(plan.look['ret'], scores)
    for k, v in held.items():
        _put(getattr(plan, k), v)
    eng.plan_refit(plan, keep_best=True)
    want = ref.refit(scores, cand, mean, std, E=E, keep_best=1, smoothing=0.5, min_std=0.08, **held)
    for k, v in want.items():
        assert _same_bits(getattr(plan, k), v), k
    assert (want['std'] >= 0.08).all()  # min_std floors both components


@pytest.mark.parametrize('K,n', [(5, 4), (70, 33)])
@pytest.mark.parametrize('fit_std,keep_best,smoothing,min_std', [(0, 0, 0.0, 0.0), (1, 1, 0.5, 0.08)])
def test_mppi_update_against_the_reference_where_exp_is_exact(amd, K, n, fit_std, keep_best, smoothing, min_std):
    """tests/test_plan_mppi.py's score patterns, whose weights are exactly 0 or 1: env 0 all equal, env 1 one-hot, env 2 two
    holders of the top score.  The prior mean of env 1 has its first row far outside the box."""
    B = 3
    eng = _uni(amd, B)
    rng = np.random.RandomState(K + n)
    cand = np.stack([rng.uniform(0.0, V_PREF, (B, K, n)), rng.uniform(-R4, R4, (B, K, n))], axis=-1)
    mean, std = _mean_std(B, n, seed=5)
    mean[1, 0], mean[2, 0] = (3.0, -4.0), (-2.0, 2.5)
    held = dict(best_actions=np.full((B, n, 2), 7.0), best_score=np.array([100.0, -1e7, 0.25]), action=np.full((B, 2), 7.0))
    scores = np.full((B, K), -1e6)
    scores[0], scores[1, 0] = 0.25, 0.0
    scores[2, [K - 1, 2]] = 3.0
    plan = _plan(eng, K, n, smoothing=smoothing, min_std=min_std)
    _put(plan.candidates, cand), _put(plan.mean, mean), _put(plan.std, std), _put(plan.look['ret'], scores)
    for k, v in held.items():
        _put(getattr(plan, k), v)
    eng.plan_mppi_update(plan, 1.0, fit_std=bool(fit_std), keep_best=bool(keep_best))
    want = uni.mppi_update(scores, cand, mean, std, temperature=1.0, fit_std=fit_std, keep_best=keep_best, smoothing=smoothing,
                           min_std=min_std, v_pref=V_PREF, R=R4, **held)
    for k in OUTPUTS:
        assert _same_bits(getattr(plan, k), want[k]), (k, _np(getattr(plan, k)), want[k])
    if smoothing:  # half of the far rows is kept: the mean lies outside the box, the action on its corner
        assert want['mean'][1, 0, 0] > V_PREF and want['action'][1].tolist() == [V_PREF, -R4]
        assert want['mean'][2, 0, 0] < 0.0 and want['action'][2].tolist() == [0.0, R4]
    else:  # the weighted mean of rows inside the box lies inside it: no clip
        assert _same_bits(plan.action, want['mean'][:, 0])


# ------------------------------------------------------------------------------------------------ 5. cem and mppi, composed
# discomfort_dist = 0.5 m and fourteen steps straight at the goal first: the robot stands 0.5 m short of the circle's centre when
# the humans cross it, so the candidates' returns differ (tests/test_plan.py)
NEAR, ADVANCE = dict(discomfort_dist=0.5), 14
COMPOSED = {'h5': dict(B=3, H=5, K=5, n=4), 'h5_k70_n33': dict(B=3, H=5, K=70, n=33), 'one_human': dict(B=3, H=1, K=5, n=4),
            'twelve_humans_kd': dict(B=2, H=12, K=5, n=4, cfg={})}  # (twelve fit the circle at the default distance only)


def _advanced(amd, B, H, cfg, goal_weight=0.0):
    eng = _uni(amd, B, H, **cfg)
    eng.set_lookahead_goal_weight(goal_weight)
    bufs = eng.rollout_begin(**BEGIN)
    for _ in range(ADVANCE):
        eng.rollout_step(np.tile(STRAIGHT, (B, 1)))
    return eng, bufs


def _composed(eng, bufs, K, n, update, E=2):
    """plan_cem (update None) or plan_mppi in one call against plan_draw + lookahead + the update; nothing of the engine moves."""
    import torch
    one, parts = (eng.plan_reset(_plan(eng, K, n, E)) for _ in range(2))
    snap, io_before, counts = _snapshot(eng), {k: v.clone() for k, v in bufs.items()}, eng.launch_counts()
    eng.plan_cem(one, 21) if update is None else eng.plan_mppi(one, counter=21, **update)
    for a, b in zip(snap, _snapshot(eng)):  # state, global time, theta
        assert torch.equal(a, b)
    for k, v in io_before.items():
        assert torch.equal(v, bufs[k]), k
    assert eng.launch_counts() == counts
    eng.plan_draw(parts, 21)
    look = eng.lookahead(parts.candidates)
    for k, v in look.items():
        parts.look[k].copy_(v)
    eng.plan_refit(parts) if update is None else eng.plan_mppi_update(parts, **update)
    eng.sync()
    for k, v in parts.tensors().items():
        assert torch.equal(v, one.tensors()[k]), k
    cand = _np(one.candidates)
    assert cand[..., 0].min() >= 0.0 and cand[..., 0].max() <= V_PREF and np.abs(cand[..., 1]).max() <= R4
    return one, look


@pytest.mark.parametrize('update', ['cem', 'mppi'])
@pytest.mark.parametrize('case', sorted(COMPOSED))
def test_cem_and_mppi_are_draw_lookahead_update(amd, case, update):
    import torch
    c = COMPOSED[case]
    eng, bufs = _advanced(amd, c['B'], c['H'], c.get('cfg', NEAR))
    one, look = _composed(eng, bufs, c['K'], c['n'], None if update == 'cem' else dict(temperature=1.0, fit_std=True))
    best = one.order[:, 0].long()
    rows = torch.arange(c['B'], device=best.device)
    assert torch.equal(one.best_score, look['ret'][rows, best]) and torch.equal(one.best_actions, one.candidates[rows, best])
    if update == 'cem':
        assert torch.equal(one.action, one.best_actions[:, 0])
    else:
        assert _same_bits(one.action, uni.clip(_np(one.mean)[:, 0], V_PREF, R4))
    print(case, update, 'ret', _np(look['ret'])[:, :5].tolist(), 'order', _np(one.order)[:, :5].tolist())
    if case == 'h5':
        assert len(np.unique(_np(look['ret']))) > 2  # the ranking has something to rank


def test_three_iterations_are_three_calls_and_the_best_replays(amd):
    import torch
    B, K, n, E = 3, 70, 33, 2  # 33 steps: the goal, 18 steps ahead, lies inside the horizon, so the best score is not 0.0
    eng, bufs = _advanced(amd, B, 5, NEAR)
    three, ones = (eng.plan_reset(_plan(eng, K, n, E, I=i, smoothing=0.5, min_std=0.02)) for i in (3, 1))
    eng.plan_cem(three, 40)
    scores, actions = [], []
    for i in range(3):
        eng.plan_cem(ones, 40 + i)
        scores.append(ones.best_score.clone()), actions.append(ones.best_actions.clone())
    for k in ('mean', 'std', 'candidates', 'order'):
        assert torch.equal(getattr(three, k), getattr(ones, k)), k
    scores, actions = torch.stack(scores), torch.stack(actions)
    assert torch.equal(three.best_score, scores.max(dim=0).values)
    first = (scores == scores.max(dim=0).values).float().argmax(dim=0)  # the EARLIEST call attaining it
    assert torch.equal(three.best_actions, actions[first, torch.arange(B, device=first.device)])
    assert torch.equal(three.action, three.best_actions[:, 0])
    m_three, m_ones = (eng.plan_reset(_plan(eng, K, n, E, I=i, smoothing=0.5, min_std=0.02)) for i in (3, 1))
    eng.plan_mppi(m_three, 1.0, 40, fit_std=True)
    for i in range(3):
        eng.plan_mppi(m_ones, 1.0, 40 + i, fit_std=True)
    for k in ('mean', 'std', 'candidates', 'order', 'action'):
        assert torch.equal(getattr(m_three, k), getattr(m_ones, k)), k
    # the best sequence replayed by real steps (rollout_actions, traced with rewards) gives the score it was ranked by:
    # sum_t gamma^(t dt v_pref) r_t summed left to right, up to the step that ends the episode (tests/test_lookahead.py)
    episode0 = _np(bufs['ep_count']).copy()
    rows = {k: _np(v) for k, v in eng.rollout_actions(three.best_actions, trace=True, rewards=True).items()}
    replay = np.zeros(B)
    for b in range(B):
        for t in range(n):
            if rows['episode'][b, t] != episode0[b]:
                break
            replay[b] = replay[b] + math.pow(0.9, t * DT * V_PREF) * float(rows['reward'][b, t])
    print('best score per call', _np(scores).tolist(), 'replayed', replay.tolist())
    assert _same_bits(three.best_score, replay) and (replay != 0.0).all()


# ------------------------------------------------------------------------------------------------ 6. every family once
UPDATES = {'cem': None, 'mppi': dict(temperature=1.0, fit_std=False)}


def _twins(amd, **cfg):
    """Two engines, begun rollouts and plans alike: [(engine, bufs, plan)] * 2."""
    made = []
    for _ in range(2):
        eng = _uni(amd, 3, 5, robot_visible=1, **cfg)
        bufs = eng.rollout_begin(episode_limit=5, **BEGIN)
        for _ in range(4):  # the humans are under way
            eng.rollout_step(np.tile(STRAIGHT, (3, 1)))
        made.append((eng, bufs, eng.plan_reset(_plan(eng, 5, 4, 2, I=2, smoothing=0.25, min_std=0.01))))
    return made


def _update(eng, plan, update):
    eng.plan_refit(plan, keep_best=update[1]) if update[0] is None else eng.plan_mppi_update(plan, keep_best=update[1], **update[0])


@pytest.mark.parametrize('update', sorted(UPDATES))
def test_paths_planners_are_draw_lookahead_paths_update(amd, update):
    U = UPDATES[update]
    (x, xbufs, xplan), (y, ybufs, yplan) = _twins(amd)
    vel = x.predict(4, 'to_goal')
    assert _same_bits(vel, _np(y.predict(4, 'to_goal')))
    if U is None:
        x.plan_cem_paths(xplan, vel, 30)
    else:
        x.plan_mppi_paths(xplan, vel, U['temperature'], 30, fit_std=U['fit_std'])
    for i in range(2):
        y.plan_draw(yplan, 30 + i)
        for k, v in y.lookahead_paths(yplan.candidates, vel).items():
            yplan.look[k].copy_(v)
        _update(y, yplan, (U, i > 0))
    assert_twins_equal(x, xbufs, xplan, y, ybufs, yplan)


@pytest.mark.parametrize('reduce', ['mean', 'min'])
def test_modes_planner_is_draw_lookahead_modes_refit(amd, reduce):
    (x, xbufs, xplan), (y, ybufs, yplan) = _twins(amd)
    vel = x.predict(4, ('to_goal', 'cv', 'to_goal'))
    x.predict_orca(4, out=vel, mode=2)  # M = 3: to_goal, constant velocity, ORCA among the humans
    x.plan_cem_modes(xplan, vel, 30, reduce=reduce, risk_penalty=0.5)
    for i in range(2):
        y.plan_draw(yplan, 30 + i)
        out = y.lookahead_modes(yplan.candidates, vel, reduce=reduce, risk_penalty=0.5)
        for k, src in (('ret', 'score'), ('info', 'worst_info'), ('steps', 'worst_steps'), ('time', 'worst_time')):
            yplan.look[k].copy_(out[src])
        y.plan_refit(yplan, keep_best=i > 0)
    assert_twins_equal(x, xbufs, xplan, y, ybufs, yplan)


FUTURES = {'one': dict(models='to_goal', orca_mode=0), 'two': dict(models=('to_goal', 'cv'), orca_mode=1, reduce='min')}


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


@pytest.mark.parametrize('kind,futures,update', [('predict', 'one', 'cem'), ('predict', 'two', 'mppi'), ('orca', 'one', 'mppi'),
                                                 ('orca', 'two', 'cem'), ('nominal', 'one', 'cem'), ('nominal', 'two', 'mppi')])
def test_predict_rollouts_are_the_per_step_loop(amd, kind, futures, update):
    """plan_predict_rollout, plan_predict_orca_rollout and plan_predict_orca_nominal_rollout, 4 real steps in one call, against
    the per-step loop on a twin.  time_limit 2.0 s: the episodes end at their fifth step — the fourth was made before the call
    — so the call re-seeds every env from a new scenario and shifts it afterwards."""
    import torch
    F, U = FUTURES[futures], UPDATES[update]
    (x, xbufs, xplan), (y, ybufs, yplan) = _twins(amd, time_limit=2.0)
    pred = x.plan_predict_begin(xplan, **{k: v for k, v in F.items() if k != 'orca_mode'})
    extra = {} if U is None else U
    call = dict(predict=x.plan_predict_rollout, orca=x.plan_predict_orca_rollout, nominal=x.plan_predict_orca_nominal_rollout)[kind]
    assert call(xplan, pred, 4, 100, **extra, **({} if kind == 'predict' else dict(orca_mode=F['orca_mode']))) is xbufs
    for s in range(4):
        vel = _loop_step(y, yplan, F, U, 100 + s * 2, kind)
    assert_twins_equal(x, xbufs, xplan, y, ybufs, yplan)
    assert torch.equal(pred.human_vel, vel.reshape(pred.human_vel.shape))
    assert int(_np(xbufs['ep_count']).sum()) >= 3 and (_np(x.get_theta()) != math.pi / 2).any()
    act = _np(xplan.action)
    assert (act[:, 0] >= 0).all() and (act[:, 0] <= V_PREF).all() and (np.abs(act[:, 1]) <= R4).all()


# ------------------------------------------------------------------------------------------------ 7. the closed loops
@pytest.mark.parametrize('update', sorted(UPDATES))
@pytest.mark.parametrize('time_limit,episode_limit', [(1.0, 17), (2.0, 5)])
def test_rollouts_are_the_python_loop(amd, time_limit, episode_limit, update):
    """time_limit 1.0 s: every step ends its episode in Timeout and the shift only re-seeds; of 17 episodes env 2 gets five and
    retires one step before the call ends.  time_limit 2.0 s: five-step episodes, so the call also shifts running plans; of 5
    episodes env 2 gets one and retires at step five (tests/test_plan.py)."""
    B, K, n, E, I, steps, counter = 3, 5, 4, 2, 2, 6, 100
    U = UPDATES[update]
    made = []
    for _ in range(2):
        eng = _uni(amd, B, time_limit=time_limit)
        bufs = eng.rollout_begin(episode_limit=episode_limit, **BEGIN)
        made.append((eng, bufs, eng.plan_reset(_plan(eng, K, n, E, I=I, smoothing=0.25, min_std=0.01))))
    (x, xbufs, xplan), (y, ybufs, yplan) = made
    if U is None:
        assert x.plan_rollout(xplan, steps, counter) is xbufs
    else:
        assert x.plan_mppi_rollout(xplan, steps, U['temperature'], counter, fit_std=U['fit_std']) is xbufs
    for s in range(steps):
        if U is None:
            y.plan_cem(yplan, counter + s * I)
        else:
            y.plan_mppi(yplan, U['temperature'], counter + s * I, fit_std=U['fit_std'])
        y.rollout_step(yplan.action)
        y.plan_shift(yplan)
    assert_twins_equal(x, xbufs, xplan, y, ybufs, yplan)
    assert _np(xbufs['ep_count']).tolist() == ([6, 6, 5] if time_limit == 1.0 else [1, 1, 1])
    assert _np(xbufs['active'])[2] == 0 and (_np(xbufs['ep_outcome'])[:, 0] == amd.TIMEOUT).all()
    assert (_np(xplan.std)[:2, :, 1] == S).all() if U is not None else True  # MPPI without fit_std: the shift's deviations


# ------------------------------------------------------------------------------------------------ 8. goal weight, bootstrap
def test_goal_weight_ranks_as_the_composition(amd):
    eng, bufs = _advanced(amd, 3, 5, NEAR, goal_weight=0.1)
    plain, pbufs = _advanced(amd, 3, 5, NEAR)
    one, look = _composed(eng, bufs, 70, 4, None)
    other, plain_look = _composed(plain, pbufs, 70, 4, dict(temperature=1.0, fit_std=False))
    assert _same_bits(one.candidates, _np(other.candidates))  # the same draw ...
    assert not _same_bits(look['ret'], _np(plain_look['ret']))  # ... scored with the term and without


def test_bootstrap_ranks_by_the_score_of_lookahead_values(amd):
    import torch
    B, K, n, E = 3, 70, 4, 2
    eng = _uni(amd, B, 5, robot_visible=1)
    eng.sarl_configure(actions=action_space(unicycle=True))
    g = load_golden('sarl_plain.npz')
    eng.sarl_set_weights({k[len('param_'):]: torch.from_numpy(v) for k, v in g.items() if k.startswith('param_')})
    plan = eng.plan_reset(_plan(eng, K, n, E, bootstrap=True))
    assert 'final_theta' in plan.look  # the unicycle's branch-end headings, which the bootstrap requires
    eng.plan_cem(plan, 3)
    cand = plan.candidates.clone()
    look = eng.lookahead(cand, bootstrap=True)
    for k, v in look.items():
        assert torch.equal(v, plan.look[k]), k
    score = _np(look['score'])
    assert not np.array_equal(score, _np(look['ret']))  # the bootstrap says something
    order = np.stack([np.argsort(ref.ranks(s)) for s in score])
    assert _same_bits(plan.order, order.astype(np.int32))
    rows = np.arange(B)
    assert _same_bits(plan.best_score, score[rows, order[:, 0]]) and _same_bits(plan.best_actions, _np(cand)[rows, order[:, 0]])


# ------------------------------------------------------------------------------------------------ 9. the examples
@pytest.mark.parametrize('script,args', [('shooting_planner.py', ['--cem']),
                                         ('predicted_paths_planner.py', ['--futures', 'to_goal,orca', '--device-loop', '--orca-sees-plan'])])
def test_the_examples_run_with_a_unicycle(amd, script, args):
    cmd = [sys.executable, os.path.join(ROOT, 'examples', script), '--kinematics', 'unicycle', '--cases', '2', '--candidates', '8',
           '--horizon', '4'] + args
    done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    text = done.stdout.decode()
    assert done.returncode == 0, text
    lines = [line.split('INFO: ', 1)[1] for line in text.splitlines() if 'TEST  has success rate:' in line]
    assert len(lines) == 1, text
    words = lines[0].replace(',', '').split()
    rates = [float(words[words.index(w) + 1]) for w in ('rate:', 'time:', 'reward:')]  # the line parses
    assert 0.0 <= rates[0] <= 1.0 and 'collision rate:' in lines[0], lines[0]
