"""The device CEM planner on the MI355X (cn_plan_*): the draw against its own invariances and tests/plan_reference.py, the refit,
the prior and the shift against the numpy restatement bit for bit, cn_plan_cem against the calls it is made of, cn_plan_rollout
against a twin engine driven by the Python loop.  The lookahead that scores the candidates is the existing one and is never the
code under test here.

Shapes: B = 3 at 5 humans (one env per workgroup on one wave, as every batch up to 2048 envs gets; the lookahead and the real step
inside the closed loop run packed and on two waves in tests/test_workgroup_geometry.py), K = 5 and K = 70 (ranks crossing the
64-lane boundary), n = 4 and n = 1, E = 1, 2 and K elites."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import plan_reference as ref
from support import (  # noqa: F401  (amd: module fixture)
    amd, begin_plan as _plan, np_of as _np, put as _put, same_bits as _same_bits, sarl_engine as _sarl_engine, SEED,
    seeded_engine as _engine, snapshot as _snapshot)

pytestmark = pytest.mark.gpu

BEGIN = dict(seed_base=1000, seed_mod=500, record_capacity=8)
DT, V_PREF = 0.25, 1.0  # the engines' defaults (time_step, robot_v_pref)
# Largest |device - reference| / max(1, r std) of a drawn component (test_draw_against_the_reference): measured 5.551e-17 on the
# first run (profiles/plan_cem_parity.txt) — the device's log / cos / sin against libm's in the last bits — and bounded at 4 x
# that.  A wrong round, word or counter order gives O(1).
DRAW_BOUND = 4 * 5.551e-17


def _mean_std(B, n, seed=1, scale=0.4):
    rng = np.random.RandomState(seed)
    return rng.uniform(-scale, scale, (B, n, 2)), rng.uniform(0.05, 0.3, (B, n, 2))


# ------------------------------------------------------------------------------------------------ 1. draw
def test_draw_invariances(amd):
    import torch
    eng, two = _engine(amd, 3), _engine(amd, 2)
    mean, std = _mean_std(3, 4)
    mean[1, 2], mean[2, 0] = (3.0, -4.0), (-0.9, 0.8)  # outside the disc: candidate 0 is clipped too
    draw = lambda e, K, n, c=7, m=mean, s=std: e.plan_draw(_plan(e, K, n, mean=m[:e.B, :n], std=s[:e.B, :n]), c).clone()  # noqa: E731
    nine = draw(eng, 9, 4)
    assert nine.shape == (3, 9, 4, 2) and nine.dtype == torch.float64
    assert _same_bits(nine[:, 0], ref.clip(mean, V_PREF))  # candidate 0 is the clipped mean
    assert torch.equal(draw(eng, 5, 4), nine[:, :5])       # a row depends on neither K ...
    assert torch.equal(draw(eng, 9, 1), nine[:, :, :1])    # ... nor n ...
    assert torch.equal(draw(two, 9, 4), nine[:2])          # ... nor B
    assert torch.equal(draw(eng, 9, 4), nine)              # the same arguments, the same bits
    other = draw(eng, 9, 4, c=8)
    assert torch.equal(other[:, 0], nine[:, 0]) and (other[:, 1:] != nine[:, 1:]).any(dim=-1).all()  # every k >= 1 row differs
    seventy = draw(eng, 70, 4)
    assert torch.equal(seventy[:, :9], nine)
    still = draw(eng, 9, 4, s=np.zeros_like(std))
    assert torch.equal(still, still[:, :1].expand(-1, 9, -1, -1))  # std = 0: every candidate is candidate 0
    far = draw(eng, 70, 4, m=np.full((3, 4, 2), 5.0))
    norm = _np(far.norm(dim=-1))
    assert norm.max() <= V_PREF * (1 + 1e-12) and norm.min() > 0.999 * V_PREF  # every row clipped onto the disc


@pytest.mark.parametrize('K,n', [(70, 4), (5, 1)])
def test_draw_against_the_reference(amd, K, n):
    eng = _engine(amd, 3)
    mean, std = _mean_std(3, n, seed=2, scale=0.2)
    got = _np(eng.plan_draw(_plan(eng, K, n, mean=mean, std=std), 11))
    want = ref.draw(mean, std, K, SEED, 11, V_PREF)
    _, _, r = ref.normal_pairs(3, K, n, SEED, 11)
    err = np.abs(got - want) / np.maximum(1.0, r[..., None] * std[:, None])
    print('plan_draw parity K=%d n=%d: largest |device - reference| / max(1, r std) = %.3e (clipped rows: %d)'
          % (K, n, err.max(), int((np.hypot(want[..., 0], want[..., 1]) >= V_PREF * (1 - 1e-12)).sum())))
    assert DRAW_BOUND < 1e-9 and err.max() <= DRAW_BOUND


def test_draw_statistics(amd):
    B, K, n, sd = 8, 65, 8, 0.01 * V_PREF
    eng = _engine(amd, B)
    got = _np(eng.plan_draw(_plan(eng, K, n, mean=np.zeros((B, n, 2)), std=np.full((B, n, 2), sd)), 0))
    assert not got[:, 0].any()
    z = got[:, 1:]  # [8, 64, 8, 2]: no row clips
    N = z.size
    assert N == 8 * 64 * 8 * 2 and np.abs(z).max() < 0.1
    corr = lambda a, b: float(np.mean(a * b)) / (sd * sd)  # noqa: E731
    figures = dict(mean=z.mean(), var=z.var(), xy=corr(z[..., 0], z[..., 1]), adjacent_t=corr(z[:, :, :-1], z[:, :, 1:]))
    print('plan_draw statistics over %d samples:' % N, figures)
    assert abs(figures['mean']) <= 5 * sd / np.sqrt(N)
    assert abs(figures['var'] - sd * sd) <= 5 * sd * sd * np.sqrt(2.0 / N)
    assert abs(figures['xy']) <= 5 / np.sqrt(N) and abs(figures['adjacent_t']) <= 5 / np.sqrt(N)


# ------------------------------------------------------------------------------------------------ 2. refit, prior, shift
@pytest.mark.parametrize('K,n,E', [(5, 4, 5), (5, 4, 2), (5, 1, 1), (70, 4, 2), (70, 1, 1), (70, 4, 64)])
@pytest.mark.parametrize('keep_best,smoothing,min_std', [(0, 0.0, 0.0), (1, 0.5, 0.08), (1, 0.0, 0.0)])
def test_refit_against_the_reference(amd, K, n, E, keep_best, smoothing, min_std):
    B = 3
    eng = _engine(amd, B)
    mean, std = _mean_std(B, n, seed=3)
    plan = _plan(eng, K, n, E, mean=mean, std=std, smoothing=smoothing, min_std=min_std)
    cand = _np(eng.plan_draw(plan, 5)).copy()  # the device's own candidates
    rng = np.random.RandomState(K + n)
    scores = rng.randint(0, 4, (B, K)) / 4.0 - 0.5  # four levels: exact ties everywhere
    scores[2] = 0.25                                # ... and an env whose scores are all equal
    held = dict(best_actions=np.full((B, n, 2), 7.0), best_score=np.array([100.0, -100.0, 0.25]), action=np.full((B, 2), 7.0))
    _put(plan.look['ret'], scores)
    for k, v in held.items():
        _put(getattr(plan, k), v)
    eng.plan_refit(plan, keep_best=bool(keep_best))
    want = ref.refit(scores, cand, mean, std, E=E, keep_best=keep_best, smoothing=smoothing, min_std=min_std, **held)
    for k, v in want.items():
        assert _same_bits(getattr(plan, k), v), (k, _np(getattr(plan, k)), v)
    assert _same_bits(plan.candidates, cand) and _same_bits(plan.look['ret'], scores)  # inputs are left alone
    assert sorted(want['order'][0].tolist()) == list(range(K)) and want['order'][2].tolist() == list(range(K))
    if keep_best:  # env 0 holds a better one, env 1 a worse one, env 2 an equal one: strict, so it stays
        assert (want['best_actions'][0] == 7.0).all() and (want['best_actions'][1] != 7.0).any() and (want['best_actions'][2] == 7.0).all()
    else:
        assert (want['action'] == want['best_actions'][:, 0]).all() and (want['best_actions'] != 7.0).any(axis=(1, 2)).all()
    if min_std > 0 and E == 1:
        assert (want['std'] == min_std).any()  # one elite: no spread, the floor binds where smoothing * std is below it
    if E == K:
        assert np.allclose(want['mean'], smoothing * mean + (1 - smoothing) * cand.mean(axis=1), rtol=0, atol=1e-15)


def test_reset_and_shift_against_the_reference(amd):
    """Six real steps on an engine whose episodes time out at their fifth step (global_time >= time_limit - 1): the shift
    meets running envs, envs whose episode has just ended (re-seeded from the new scenario) and, with five episodes for three
    envs, a retired one."""
    B, K, n = 3, 5, 4
    eng = _engine(amd, B, time_limit=2.0)
    bufs = eng.rollout_begin(episode_limit=5, **BEGIN)
    plan = _plan(eng, K, n, 2, init_std=0.3)
    mean0, std0 = _mean_std(B, n, seed=4)
    _put(plan.mean, mean0), _put(plan.std, std0)
    state = _np(eng.get_state()[0])
    eng.plan_reset(plan, mask=np.array([1, 0, 1], np.uint8))
    want = ref.reset(state, DT, mean0, std0, 0.3, mask=[1, 0, 1])
    assert _same_bits(plan.mean, want[0]) and _same_bits(plan.std, want[1]) and (want[0][0] == [0.0, 1.0]).all()
    eng.plan_reset(plan)
    want = ref.reset(state, DT, mean0, std0, 0.3)
    assert _same_bits(plan.mean, want[0]) and _same_bits(plan.std, want[1])
    seen = set()
    for s in range(6):
        eng.plan_cem(plan, 10 + s)
        eng.rollout_step(plan.action)
        before = _np(plan.mean).copy(), _np(plan.std).copy()
        active, cur_steps, state = _np(bufs['active']).copy(), _np(bufs['cur_steps']).copy(), _np(eng.get_state()[0])
        eng.plan_shift(plan)
        want = ref.shift(state, DT, active, cur_steps, before[0], before[1], 0.3)
        assert _same_bits(plan.mean, want[0]) and _same_bits(plan.std, want[1]), s
        seen |= {'retired' if not a else 'ended' if c == 0 else 'running' for a, c in zip(active, cur_steps)}
        for b in np.flatnonzero(active == 0):  # a retired env's plan is left alone, std included
            assert _same_bits(want[0][b], before[0][b]) and _same_bits(want[1][b], before[1][b])
    assert seen == {'retired', 'ended', 'running'}, seen


# ------------------------------------------------------------------------------------------------ 3. - 5. cem
# discomfort_dist = 0.5 m and fourteen steps straight at the goal first: the robot stands 0.5 m short of the circle's centre when
# the humans cross it, so the candidates' returns differ and the ranking has something to rank
NEAR, ADVANCE = dict(discomfort_dist=0.5), 14
CEM_CASES = {'h5': dict(B=3, H=5, K=5, n=4, E=2), 'h5_k70_n1': dict(B=3, H=5, K=70, n=1, E=1),
             'one_human': dict(B=3, H=1, K=5, n=4, E=2), 'twelve_humans_kd': dict(B=2, H=12, K=5, n=4, E=5, cfg={})}  # (twelve fit the circle at the default distance only)


@pytest.mark.parametrize('case', sorted(CEM_CASES))
def test_cem_is_draw_lookahead_refit(amd, case):
    import torch
    c = CEM_CASES[case]
    eng = _engine(amd, c['B'], c['H'], **c.get('cfg', NEAR))
    bufs = eng.rollout_begin(**BEGIN)
    for _ in range(ADVANCE):
        eng.rollout_step(np.tile([0.0, 1.0], (c['B'], 1)))
    one, parts = (eng.plan_reset(_plan(eng, c['K'], c['n'], c['E'])) for _ in range(2))
    snap, io_before, counts = _snapshot(eng), {k: v.clone() for k, v in bufs.items()}, eng.launch_counts()
    eng.plan_cem(one, 21)
    for a, b in zip(snap, _snapshot(eng)):  # nothing of the engine moved
        assert torch.equal(a, b)
    for k, v in io_before.items():
        assert torch.equal(v, bufs[k]), k
    assert eng.launch_counts() == counts
    eng.plan_draw(parts, 21)
    look = eng.lookahead(parts.candidates)
    for k, v in look.items():
        parts.look[k].copy_(v)
    eng.plan_refit(parts)
    eng.sync()
    for k, v in parts.tensors().items():
        assert torch.equal(v, one.tensors()[k]), k
    for k, v in look.items():
        assert torch.equal(v, one.look[k]), k
    best = one.order[:, 0].long()
    rows = torch.arange(c['B'], device=best.device)
    assert torch.equal(one.best_score, look['ret'][rows, best]) and torch.equal(one.best_actions, one.candidates[rows, best])
    assert torch.equal(one.action, one.best_actions[:, 0]) and torch.equal(one.best_score, look['ret'].max(dim=1).values)
    print(case, 'ret', _np(look['ret'])[:, :5].tolist(), 'order', _np(one.order)[:, :5].tolist())
    if case == 'h5':
        assert len(np.unique(_np(look['ret']))) > 2  # ... and the case is what it claims to be


def test_three_iterations_are_three_calls_and_the_best_replays(amd):
    import torch
    B, K, n, E = 3, 70, 4, 2
    eng = _engine(amd, B, **NEAR)
    for _ in range(ADVANCE):
        eng.step(np.tile([0.0, 1.0], (B, 1)), update=True, want_obs=False)
    three, ones = eng.plan_reset(_plan(eng, K, n, E, I=3, smoothing=0.5, min_std=0.02)), \
        eng.plan_reset(_plan(eng, K, n, E, I=1, smoothing=0.5, min_std=0.02))
    eng.plan_cem(three, 40)
    scores, actions = [], []
    for i in range(3):
        eng.plan_cem(ones, 40 + i)
        scores.append(ones.best_score.clone()), actions.append(ones.best_actions.clone())
    for k in ('mean', 'std', 'candidates', 'order'):
        assert torch.equal(getattr(three, k), getattr(ones, k)), k
    scores, actions = torch.stack(scores), torch.stack(actions)  # [3, B], [3, B, n, 2]
    assert torch.equal(three.best_score, scores.max(dim=0).values)
    first = (scores == scores.max(dim=0).values).float().argmax(dim=0)  # the EARLIEST call attaining it
    assert torch.equal(three.best_actions, actions[first, torch.arange(B, device=first.device)])
    assert torch.equal(three.action, three.best_actions[:, 0])
    print('best score per call', _np(scores).tolist(), 'earliest', _np(first).tolist())
    assert len(np.unique(_np(scores))) > 1  # the calls found different bests somewhere
    replay = eng.lookahead(three.best_actions[:, None].contiguous())
    assert torch.equal(replay['ret'][:, 0], three.best_score)


# ------------------------------------------------------------------------------------------------ 6. bootstrap
def test_bootstrap_ranks_by_the_score_of_lookahead_values(amd):
    import torch
    B, K, n, E = 3, 70, 4, 2
    eng = _sarl_engine(amd, B)
    plan = eng.plan_reset(_plan(eng, K, n, E, bootstrap=True))
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


def test_bootstrap_refusals_are_those_of_lookahead_values(amd):
    B = 2
    for eng, status, word in ((_sarl_engine(amd, B, weights=False), amd._lib.CN_ERR_INVALID, 'configure and set weights first'),
                              (_engine(amd, B), amd._lib.CN_ERR_INVALID, 'configure and set weights first'),
                              (_sarl_engine(amd, B, with_om=True), amd._lib.CN_ERR_UNSUPPORTED, 'occupancy maps'),
                              (_sarl_engine(amd, B, scenario_rule=2), amd._lib.CN_ERR_UNSUPPORTED, 'mixed rule')):
        plan = _plan(eng, bootstrap=True)
        eng.rollout_begin(**BEGIN)
        for call in (lambda: eng.plan_cem(plan, 0), lambda: eng.plan_draw(plan, 0), lambda: eng.plan_rollout(plan, 2, 0)):
            with pytest.raises(amd.CrowdNavAmdError, match=word) as ei:
                call()
            assert ei.value.status == status and 'cn_lookahead_values' in str(ei.value)


# ------------------------------------------------------------------------------------------------ 7. the closed loop
@pytest.mark.parametrize('time_limit,episode_limit', [(1.0, 17), (2.0, 5)])
def test_rollout_is_the_python_loop(amd, time_limit, episode_limit):
    """time_limit 1.0 s: global_time >= time_limit - 1 holds at once, so EVERY step ends its episode in Timeout and the shift
    only re-seeds; of 17 episodes env 2 gets five and retires one step before the call ends.  time_limit 2.0 s: five-step
    episodes, so the same call also shifts running plans; of 5 episodes env 2 gets one and retires at step five."""
    import torch
    B, K, n, E, I, steps, counter = 3, 5, 4, 2, 2, 6, 100
    made = []
    for _ in range(2):
        eng = _engine(amd, B, time_limit=time_limit)
        bufs = eng.rollout_begin(episode_limit=episode_limit, **BEGIN)
        made.append((eng, bufs, eng.plan_reset(_plan(eng, K, n, E, I=I, smoothing=0.25, min_std=0.01))))
    (x, xbufs, xplan), (y, ybufs, yplan) = made
    assert x.plan_rollout(xplan, steps, counter) is xbufs
    for s in range(steps):
        y.plan_cem(yplan, counter + s * I)
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


# ------------------------------------------------------------------------------------------------ 8. the rest
def test_refusals_on_an_engine(amd):
    import torch
    lib, L = amd._lib, amd._lib.load()
    INV, UNS = lib.CN_ERR_INVALID, lib.CN_ERR_UNSUPPORTED

    def refused(eng, plan, status, *words, calls=('plan_reset', 'plan_draw', 'plan_refit', 'plan_cem', 'plan_shift', 'plan_rollout')):
        for name in calls:
            args = {'plan_draw': (3,), 'plan_cem': (3,), 'plan_rollout': (2, 3)}.get(name, ())
            with pytest.raises(amd.CrowdNavAmdError) as ei:
                getattr(eng, name)(plan, *args)
            assert ei.value.status == status and 'cn_' + name in str(ei.value) and all(w in str(ei.value) for w in words), (name, ei.value)

    eng = _engine(amd, 3)
    bufs = eng.rollout_begin(**BEGIN)
    good = eng.plan_reset(_plan(eng))
    eng.plan_cem(good, 0)
    keep, counts = {k: v.clone() for k, v in good.tensors().items()}, eng.launch_counts()
    refused(eng, _plan(eng, K=1025, E=64), UNS, 'n_candidates', '1025')
    refused(eng, _plan(eng, K=100, E=65), UNS, 'n_elites', '65')
    refused(eng, _plan(eng, n=257), UNS, 'n_steps', '257')
    refused(eng, _plan(eng, K=1, E=1), INV, 'n_candidates')
    refused(eng, _plan(eng, E=6), INV, 'n_elites')
    refused(eng, _plan(eng, E=0), INV, 'n_elites')
    refused(eng, _plan(eng, I=0), INV, 'iterations')
    refused(eng, _plan(eng, init_std=0.0), INV, 'init_std')
    refused(eng, _plan(eng, min_std=-1.0), INV, 'min_std')
    refused(eng, _plan(eng, smoothing=1.0), INV, 'smoothing')
    orca = amd.BatchedCrowdSim(num_envs=3, num_humans=5, robot_policy=amd.ROBOT_ORCA)
    orca.rollout_begin(**BEGIN)
    refused(orca, _plan(orca), INV, 'CN_ROBOT_EXTERNAL')
    uni = _engine(amd, 3, robot_kinematics=1)
    uni.rollout_begin(**BEGIN)
    refused(uni, _plan(uni), UNS, 'CN_UNICYCLE')
    # a required array: the C structs by hand
    for field in ('mean', 'candidates'):
        broken = lib.CnPlan.from_buffer_copy(good.c)
        setattr(broken, field, None)
        assert L.cn_plan_cem(eng._h, C.byref(good.cfg), C.byref(broken), 0) == INV and ('plan->' + field) in L.cn_last_error().decode()
    # what cn_rollout_step refuses for the io block: shift and rollout only, and before anything is enqueued
    io = eng._rollout[0]
    for change, word in ((dict(seed_mod=0), 'seed_mod'), (dict(seed_base=io.seed_base + 1), 'cn_rollout_begin'), (dict(active=None), 'active')):
        bad = lib.CnRolloutIo.from_buffer_copy(io)
        for k, v in change.items():
            setattr(bad, k, v)
        assert L.cn_plan_shift(eng._h, C.byref(bad), C.byref(good.cfg), C.byref(good.c)) == INV and word in L.cn_last_error().decode()
        assert L.cn_plan_rollout(eng._h, C.byref(bad), 2, C.byref(good.cfg), C.byref(good.c), 0) == INV and word in L.cn_last_error().decode()
    assert L.cn_plan_rollout(eng._h, None, 2, C.byref(good.cfg), C.byref(good.c), 0) == INV and 'io is NULL' in L.cn_last_error().decode()
    with pytest.raises(amd.CrowdNavAmdError, match='n_real_steps') as ei:
        eng.plan_rollout(good, -1, 0)
    assert ei.value.status == INV
    fresh = _engine(amd, 3)
    with pytest.raises(RuntimeError, match='rollout_begin'):
        fresh.plan_shift(_plan(fresh))
    with pytest.raises(ValueError, match='plan_begin'):
        fresh.plan_cem(good, 0)  # another engine's plan
    # n_real = 0: CN_OK, nothing enqueued; and none of the refusals above enqueued or counted anything
    assert eng.plan_rollout(good, 0, 0) is bufs
    eng.sync()
    assert eng.launch_counts() == counts
    for k, v in keep.items():
        assert torch.equal(v, good.tensors()[k]), k
    assert _np(bufs['cur_steps']).tolist() == [0, 0, 0]


def test_the_example_runs_with_cem(amd):
    done = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'shooting_planner.py'), '--cem', '--cases', '4',
                           '--candidates', '8', '--horizon', '4'], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    text = done.stdout.decode()
    assert done.returncode == 0, text
    assert 'TEST  has success rate:' in text and 'total reward:' in text, text
