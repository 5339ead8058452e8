"""The device MPPI update on the MI355X (cn_plan_mppi_*): the update against tests/plan_mppi_reference.py — bit for bit where the
weights are exactly 0 or 1, within a derived bound where exp decides —, cn_plan_mppi against the calls it is made of,
cn_plan_mppi_rollout against a twin engine driven by the Python loop.  The draw, the lookahead, the real step and the shift are
the existing ones and are never the code under test here.

Shapes: B = 3 at 5 humans, K = 5 and K = 70 (the second pass of the 64-lane loops over k), n = 4 and n = 33 (2 n = 66
components: the second pass of the component loop).

Bounds of the random-score cases.  Device and numpy exp are each within 1 ulp of the true value, so a weight differs by at most
2^-51 relatively between the two sides; both sides run the same sequential sums over k, whose roundings differ by at most K 2^-52
of Z v_pref once the weights differ; the quotient and the blend add a few more 2^-52.  With |a_k| <= v_pref that gives
|mean - ref| <= (K + 4) 2^-52 v_pref and, the deviations being at most 2 v_pref, |std^2 - ref^2| <= 2 (K + 4) 2^-52 v_pref^2;
the bounds asserted carry a factor 4 of margin: 4 (K + 4) 2^-52 v_pref and 8 (K + 4) 2^-52 v_pref^2."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import plan_mppi_reference as mref
import plan_reference as ref
from support import (  # noqa: F401  (amd: module fixture)
    amd, begin_plan as _plan, np_of as _np, put as _put, same_bits as _same_bits, sarl_engine as _sarl_engine,
    seeded_engine as _engine, snapshot as _snapshot)

pytestmark = pytest.mark.gpu

BEGIN = dict(seed_base=1000, seed_mod=500, record_capacity=8)
V_PREF = 1.0  # the engines' default robot_v_pref
SHAPES = [(5, 4), (70, 4), (5, 33), (70, 33)]
OUTPUTS = ('order', 'best_actions', 'best_score', 'action', 'mean', 'std')


def _inputs(B, K, n, seed):
    """Caller-made candidates inside the speed disc, a prior mean with one row far outside it, a prior std, held best rows."""
    rng = np.random.RandomState(seed)
    cand = rng.uniform(-0.6, 0.6, (B, K, n, 2))
    mean, std = rng.uniform(-0.4, 0.4, (B, n, 2)), rng.uniform(0.05, 0.3, (B, n, 2))
    mean[1, 0] = (3.0, -4.0)
    held = dict(best_actions=np.full((B, n, 2), 7.0), best_score=np.array([100.0, -1e7, 0.25][:B]), action=np.full((B, 2), 7.0))
    return cand, mean, std, held


def _run_update(eng, K, n, scores, cand, mean, std, held, temperature, fit_std, keep_best, smoothing, min_std):
    plan = _plan(eng, K, n, smoothing=smoothing, min_std=min_std)
    _put(plan.candidates, cand), _put(plan.mean, mean), _put(plan.std, std), _put(plan.look['ret'], scores)
    for k, v in held.items():
        _put(getattr(plan, k), v)
    eng.plan_mppi_update(plan, temperature, fit_std=fit_std, keep_best=keep_best)
    eng.sync()
    assert _same_bits(plan.candidates, cand) and _same_bits(plan.look['ret'], scores)  # inputs are left alone
    want = mref.mppi_update(scores, cand, mean, std, temperature=temperature, fit_std=fit_std, keep_best=keep_best,
                            smoothing=smoothing, min_std=min_std, v_pref=V_PREF, **held)
    return plan, want


# ------------------------------------------------------------------------------------------------ 1. the update, bit for bit
@pytest.mark.parametrize('K,n', SHAPES)
@pytest.mark.parametrize('fit_std,keep_best,smoothing,min_std', [(0, 0, 0.0, 0.0), (1, 1, 0.5, 0.08), (1, 0, 0.0, 0.0)])
def test_update_against_the_reference_where_exp_is_exact(amd, K, n, fit_std, keep_best, smoothing, min_std):
    """Env 0: all scores equal (every weight 1).  Env 1: (0, -1e6, ...) (every other weight 0).  Env 2: two holders of the top
    score, the rest 1e6 below (two weights of 1; k* the lower index)."""
    B = 3
    eng = _engine(amd, B)
    cand, mean, std, held = _inputs(B, K, n, seed=K + n)
    scores = np.full((B, K), -1e6)
    scores[0] = 0.25
    scores[1, 0] = 0.0
    scores[2, [K - 1, 2]] = 3.0
    plan, want = _run_update(eng, K, n, scores, cand, mean, std, held, 1.0, fit_std, keep_best, smoothing, min_std)
    for k in OUTPUTS:
        assert _same_bits(getattr(plan, k), want[k]), (k, _np(getattr(plan, k)), want[k])
    # ... and the restatement says what the issue says
    assert want['order'][0].tolist() == list(range(K)) and want['order'][1, 0] == 0 and want['order'][2, :2].tolist() == [2, K - 1]
    if not fit_std:
        assert _same_bits(plan.std, std)
    if smoothing == 0.0:
        assert _same_bits(plan.mean[1], cand[1, 0]) and _same_bits(plan.mean[2], (cand[2, 2] + cand[2, K - 1]) / 2.0)
        assert _same_bits(plan.action, want['mean'][:, 0])  # candidates lie inside the disc: no clip
        if fit_std:
            assert not _np(plan.std)[1].any()
    else:  # the prior's far row, half kept: the action is clipped onto the disc, the mean is not
        assert np.hypot(*want['mean'][1, 0]) > 2.0 and abs(np.hypot(*_np(plan.action)[1]) - V_PREF) < 1e-15
        assert (_np(plan.std)[1] >= min_std).all() and (_np(plan.std)[1] == np.maximum(min_std, 0.5 * std[1])).all()
    if keep_best:  # env 0 holds a better one, env 1 a worse one, env 2 ... a worse one too (0.25 < 3): strict
        assert (want['best_actions'][0] == 7.0).all() and _same_bits(plan.best_actions[1], cand[1, 0])
    else:
        assert _same_bits(plan.best_actions, cand[np.arange(B), want['order'][:, 0]])
    assert (want['action'] != 7.0).all()  # the action is the mean's, whatever is held


def test_keep_best_is_strict_on_the_device(amd):
    B, K, n = 3, 5, 4
    eng = _engine(amd, B)
    cand, mean, std, held = _inputs(B, K, n, seed=1)
    scores = np.tile([0.0, 1.0, 1.0, -1.0, 0.5], (B, 1))
    held['best_score'] = np.array([1.0, np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0)])  # equal, just below, just above
    plan, want = _run_update(eng, K, n, scores, cand, mean, std, held, 1.0, 0, 1, 0.0, 0.0)
    for k in ('order', 'best_actions', 'best_score', 'std'):
        assert _same_bits(getattr(plan, k), want[k]), k
    for k in ('mean', 'action'):  # exp(-1) etc. decide: within the bound of the random-score cases
        assert np.abs(_np(getattr(plan, k)) - want[k]).max() <= 4 * (K + 4) * 2.0 ** -52 * V_PREF, k
    got = _np(plan.best_actions)
    assert (got[0] == 7.0).all() and np.array_equal(got[1], cand[1, 1]) and (got[2] == 7.0).all()
    assert _np(plan.best_score).tolist() == [1.0, 1.0, np.nextafter(1.0, 2.0)]


# ------------------------------------------------------------------------------------------------ 2. random scores, the bounds
@pytest.mark.parametrize('K,n', SHAPES)
@pytest.mark.parametrize('temperature', [0.05, 1.0])
def test_update_against_the_reference_within_the_derived_bounds(amd, K, n, temperature):
    B = 3
    eng = _engine(amd, B)
    cand, mean, std, held = _inputs(B, K, n, seed=100 + K + n)
    assert np.hypot(cand[..., 0], cand[..., 1]).max() <= V_PREF
    scores = np.random.RandomState(7 * K + n).uniform(-1.0, 0.5, (B, K))
    plan, want = _run_update(eng, K, n, scores, cand, mean, std, held, temperature, 1, 0, 0.0, 0.0)
    for k in ('order', 'best_actions', 'best_score'):
        assert _same_bits(getattr(plan, k), want[k]), k
    mean_err = np.abs(_np(plan.mean) - want['mean']).max()
    var_err = np.abs(_np(plan.std) ** 2 - want['std'] ** 2).max()
    act_err = np.abs(_np(plan.action) - want['action']).max()
    mean_bound, var_bound = 4 * (K + 4) * 2.0 ** -52 * V_PREF, 8 * (K + 4) * 2.0 ** -52 * V_PREF ** 2
    print('plan_mppi parity K=%d n=%d T=%g: largest |mean - ref| = %.3e (bound %.3e), |std^2 - ref^2| = %.3e (bound %.3e), '
          '|action - ref| = %.3e' % (K, n, temperature, mean_err, mean_bound, var_err, var_bound, act_err))
    assert mean_err <= mean_bound and var_err <= var_bound and act_err <= mean_bound
    # the case is what it claims to be: the weights are neither all 1 nor one-hot, and the mean is not the best row
    w, Z, top = mref.weights(scores[0], temperature)
    assert 1.0 < Z < K and not np.array_equal(want['mean'][0], cand[0, top])


# ------------------------------------------------------------------------------------------------ 3. composition
# discomfort_dist = 0.5 m and fourteen steps straight at the goal first: the robot stands 0.5 m short of the circle's centre when
# the humans cross it, so the candidates' returns differ and the weights have something to weigh
NEAR, ADVANCE = dict(discomfort_dist=0.5), 14
CASES = {'h5': dict(B=3, H=5, K=5, n=4, fit_std=False), 'h5_k70': dict(B=3, H=5, K=70, n=4, fit_std=True),
         'one_human': dict(B=3, H=1, K=5, n=4, fit_std=True),
         'twelve_humans_kd': dict(B=2, H=12, K=5, n=4, fit_std=False, cfg={})}  # (twelve fit the circle at the default distance only)


@pytest.mark.parametrize('case', sorted(CASES))
def test_mppi_is_draw_lookahead_update(amd, case):
    import torch
    c = CASES[case]
    eng = _engine(amd, c['B'], c['H'], **c.get('cfg', NEAR))
    bufs = eng.rollout_begin(**BEGIN)
    for _ in range(ADVANCE):
        eng.rollout_step(np.tile([0.0, 1.0], (c['B'], 1)))
    one, parts = (eng.plan_reset(_plan(eng, c['K'], c['n'])) for _ in range(2))
    snap, io_before, counts = _snapshot(eng), {k: v.clone() for k, v in bufs.items()}, eng.launch_counts()
    eng.plan_mppi(one, 0.05, 21, fit_std=c['fit_std'])
    for a, b in zip(snap, _snapshot(eng)):  # nothing of the engine moved
        assert torch.equal(a, b)
    for k, v in io_before.items():
        assert torch.equal(v, bufs[k]), k
    assert eng.launch_counts() == counts
    eng.plan_draw(parts, 21)
    look = eng.lookahead(parts.candidates)
    for k, v in look.items():
        parts.look[k].copy_(v)
    eng.plan_mppi_update(parts, 0.05, fit_std=c['fit_std'])
    eng.sync()
    for k, v in parts.tensors().items():
        assert torch.equal(v, one.tensors()[k]), k
    for k, v in look.items():
        assert torch.equal(v, one.look[k]), k
    best = one.order[:, 0].long()
    rows = torch.arange(c['B'], device=best.device)
    assert torch.equal(one.best_score, look['ret'][rows, best]) and torch.equal(one.best_actions, one.candidates[rows, best])
    assert torch.equal(one.best_score, look['ret'].max(dim=1).values)
    assert _same_bits(one.action, ref.clip(_np(one.mean)[:, 0], V_PREF))  # the mean's first row, not the best sequence's
    if not c['fit_std']:
        assert (one.std == 0.3).all()
    print(case, 'ret', _np(look['ret'])[:, :5].tolist(), 'order', _np(one.order)[:, :5].tolist())
    if case == 'h5':
        assert len(np.unique(_np(look['ret']))) > 2  # ... and the case is what it claims to be


def test_three_iterations_are_three_calls(amd):
    import torch
    B, K, n = 3, 70, 4
    eng = _engine(amd, B, **NEAR)
    for _ in range(ADVANCE):
        eng.step(np.tile([0.0, 1.0], (B, 1)), update=True, want_obs=False)
    kw = dict(smoothing=0.5, min_std=0.02)
    three, ones = eng.plan_reset(_plan(eng, K, n, I=3, **kw)), eng.plan_reset(_plan(eng, K, n, I=1, **kw))
    eng.plan_mppi(three, 0.05, 40, fit_std=True)
    eng.plan_mppi(ones, 0.05, 40, fit_std=True)  # I = 1: keep_best off
    scores = [ones.best_score.clone()]
    for i in (1, 2):
        eng.plan_draw(ones, 40 + i)
        for k, v in eng.lookahead(ones.candidates).items():
            ones.look[k].copy_(v)
        eng.plan_mppi_update(ones, 0.05, fit_std=True, keep_best=True)
        scores.append(ones.look['ret'].max(dim=1).values.clone())
    eng.sync()
    for k, v in ones.tensors().items():
        assert torch.equal(v, three.tensors()[k]), k
    scores = torch.stack(scores)
    assert torch.equal(three.best_score, scores.max(dim=0).values)
    print('best score per iteration', _np(scores).tolist())
    assert len(np.unique(_np(scores))) > 1  # the iterations found different bests somewhere


# ------------------------------------------------------------------------------------------------ 4. bootstrap
def test_bootstrap_weighs_by_the_score_of_lookahead_values(amd):
    import torch
    B, K, n, T = 3, 70, 4, 0.05
    eng = _sarl_engine(amd, B)
    plan = eng.plan_reset(_plan(eng, K, n, bootstrap=True))
    mean0, std0 = _np(plan.mean).copy(), _np(plan.std).copy()
    eng.plan_mppi(plan, T, 3, fit_std=True)
    cand = plan.candidates.clone()
    look = eng.lookahead(cand, bootstrap=True)
    for k, v in look.items():
        assert torch.equal(v, plan.look[k]), k
    score = _np(look['score'])
    assert not np.array_equal(score, _np(look['ret']))  # the bootstrap says something
    want = mref.mppi_update(score, _np(cand), mean0, std0, np.zeros((B, n, 2)), np.zeros(B), np.zeros((B, 2)), temperature=T,
                            fit_std=True, keep_best=False, smoothing=0.0, min_std=0.0, v_pref=V_PREF)
    for k in ('order', 'best_actions', 'best_score'):
        assert _same_bits(getattr(plan, k), want[k]), k
    assert np.abs(_np(plan.mean) - want['mean']).max() <= 4 * (K + 4) * 2.0 ** -52 * V_PREF
    assert np.abs(_np(plan.std) ** 2 - want['std'] ** 2).max() <= 8 * (K + 4) * 2.0 ** -52 * V_PREF ** 2
    by_ret = mref.mppi_update(_np(look['ret']), _np(cand), mean0, std0, np.zeros((B, n, 2)), np.zeros(B), np.zeros((B, 2)),
                              temperature=T, fit_std=True, keep_best=False, smoothing=0.0, min_std=0.0, v_pref=V_PREF)
    assert np.abs(by_ret['mean'] - want['mean']).max() > 1e-9  # ... and weighing by the return alone would show


def test_bootstrap_refusals_are_those_of_lookahead_values(amd):
    B = 2
    for eng, status, word in ((_sarl_engine(amd, B, weights=False), amd._lib.CN_ERR_INVALID, 'configure and set weights first'),
                              (_engine(amd, B), amd._lib.CN_ERR_INVALID, 'configure and set weights first'),
                              (_sarl_engine(amd, B, with_om=True), amd._lib.CN_ERR_UNSUPPORTED, 'occupancy maps'),
                              (_sarl_engine(amd, B, scenario_rule=2), amd._lib.CN_ERR_UNSUPPORTED, 'mixed rule')):
        plan = _plan(eng, bootstrap=True)
        eng.rollout_begin(**BEGIN)
        for call in (lambda: eng.plan_mppi(plan, 1.0, 0), lambda: eng.plan_mppi_update(plan, 1.0),
                     lambda: eng.plan_mppi_rollout(plan, 2, 1.0, 0)):
            with pytest.raises(amd.CrowdNavAmdError, match=word) as ei:
                call()
            assert ei.value.status == status and 'cn_lookahead_values' in str(ei.value)


# ------------------------------------------------------------------------------------------------ 5. the closed loop
@pytest.mark.parametrize('time_limit,episode_limit', [(1.0, 17), (2.0, 5)])
def test_rollout_is_the_python_loop(amd, time_limit, episode_limit):
    """time_limit 1.0 s: global_time >= time_limit - 1 holds at once, so EVERY step ends its episode in Timeout and the shift
    only re-seeds; of 17 episodes env 2 gets five and retires one step before the call ends.  time_limit 2.0 s: five-step
    episodes, so the same call also shifts running plans; of 5 episodes env 2 gets one and retires at step five."""
    import torch
    B, K, n, I, steps, counter, T = 3, 5, 4, 2, 6, 100, 0.05
    made = []
    for _ in range(2):
        eng = _engine(amd, B, time_limit=time_limit)
        bufs = eng.rollout_begin(episode_limit=episode_limit, **BEGIN)
        made.append((eng, bufs, eng.plan_reset(_plan(eng, K, n, I=I, smoothing=0.25, min_std=0.01))))
    (x, xbufs, xplan), (y, ybufs, yplan) = made
    assert x.plan_mppi_rollout(xplan, steps, T, counter, fit_std=True) is xbufs
    for s in range(steps):
        y.plan_mppi(yplan, T, counter + s * I, fit_std=True)
        y.rollout_step(yplan.action)
        y.plan_shift(yplan)
    for a, b in zip(_snapshot(x), _snapshot(y)):
        assert torch.equal(a, b)
    for k, v in ybufs.items():
        assert torch.equal(v, xbufs[k]), k
    for k, v in yplan.tensors().items():
        assert torch.equal(v, xplan.tensors()[k]), k
    assert x.launch_counts() == y.launch_counts() and x.launch_counts()['rollout_kernels'] >= steps
    print('ep_count', _np(xbufs['ep_count']).tolist(), 'active', _np(xbufs['active']).tolist(), 'outcome', _np(xbufs['ep_outcome'])[:, :2].tolist())
    assert _np(xbufs['ep_count']).tolist() == ([6, 6, 5] if time_limit == 1.0 else [1, 1, 1])
    assert _np(xbufs['active'])[2] == 0 and (_np(xbufs['ep_outcome'])[:, 0] == amd.TIMEOUT).all()


# ------------------------------------------------------------------------------------------------ 6. the rest
def test_refusals_on_an_engine(amd):
    import torch
    lib = amd._lib
    INV, UNS = lib.CN_ERR_INVALID, lib.CN_ERR_UNSUPPORTED

    def refused(eng, plan, status, *words, T=1.0):
        counts = eng.launch_counts()
        for name, args in (('plan_mppi_update', (T,)), ('plan_mppi', (T, 3)), ('plan_mppi_rollout', (2, T, 3))):
            with pytest.raises(amd.CrowdNavAmdError) as ei:
                getattr(eng, name)(plan, *args)
            assert ei.value.status == status and ('cn_' + name + ' ') in str(ei.value).replace(':', ' ') \
                and all(w in str(ei.value) for w in words), (name, ei.value)
        assert eng.launch_counts() == counts

    eng = _engine(amd, 3)
    bufs = eng.rollout_begin(**BEGIN)
    good = eng.plan_reset(_plan(eng))
    eng.plan_mppi(good, 1.0, 0)
    eng.sync()
    keep = {k: v.clone() for k, v in good.tensors().items()}
    orca = amd.BatchedCrowdSim(num_envs=3, num_humans=5, robot_policy=amd.ROBOT_ORCA)
    orca.rollout_begin(**BEGIN)
    refused(orca, _plan(orca), INV, 'CN_ROBOT_EXTERNAL')
    uni = _engine(amd, 3, robot_kinematics=1)
    uni.rollout_begin(**BEGIN)
    refused(uni, _plan(uni), UNS, 'CN_UNICYCLE')
    for bad in (0.0, -1.0, float('inf'), float('nan')):
        refused(eng, good, INV, 'temperature', T=bad)
        refused(orca, _plan(orca), INV, 'temperature', T=bad)  # before the engine is looked at
    refused(eng, _plan(eng, K=1025, E=64), UNS, 'n_candidates', '1025')
    refused(eng, _plan(eng, E=6), INV, 'n_elites')  # range-checked although not read
    with pytest.raises(amd.CrowdNavAmdError, match='n_real_steps') as ei:
        eng.plan_mppi_rollout(good, -1, 1.0, 0)
    assert ei.value.status == INV and 'cn_plan_mppi_rollout' in str(ei.value)
    fresh = _engine(amd, 3)
    with pytest.raises(RuntimeError, match='rollout_begin'):
        fresh.plan_mppi_rollout(_plan(fresh), 1, 1.0, 0)
    with pytest.raises(ValueError, match='plan_begin'):
        fresh.plan_mppi(good, 1.0, 0)  # another engine's plan
    # n_real = 0: CN_OK, nothing enqueued; and none of the refusals above enqueued anything
    assert eng.plan_mppi_rollout(good, 0, 1.0, 0) is bufs
    eng.sync()
    for k, v in keep.items():
        assert torch.equal(v, good.tensors()[k]), k
    assert _np(bufs['cur_steps']).tolist() == [0, 0, 0]


def test_the_example_runs_with_mppi(amd):
    done = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'shooting_planner.py'), '--mppi', '--cases', '4',
                           '--candidates', '8', '--horizon', '4'], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    text = done.stdout.decode()
    assert done.returncode == 0, text
    assert 'TEST  has success rate:' in text and 'total reward:' in text, text
