"""The lagged scenario-ring fill (crowdnav_amd/csrc/fill_plan.h; CROWDNAV_AMD_LAGGED_FILL, default 1): engines of at most 8
humans keep 2 D ring slots per env and top the ring up on a side stream BESIDE a launch, for the call after it; a launch
still looks at most D scenarios ahead.  Every case runs the same calls on two fresh engines, switch 1 and switch 0 (D slots,
every fill in front of its launch), and compares EVERY output bit for bit — each buffer of rollout_begin, get_state,
rollout_summary — and, where test_ring_wrap.py does, the oracle's rollout.  The rule's own arithmetic is checked without a
GPU by test_fill_plan_host.py."""
import numpy as np
import pytest

from ring_cases import oracle_rollout, records_in_order
from support import amd, environ, np_of as _np, same_tensors as _same  # noqa: F401  (amd: module fixture)

pytestmark = pytest.mark.gpu

K = 64
BEGIN = dict(seed_base=1000, seed_mod=500, episode_limit=-1, record_capacity=K, per_env_transitions=True)


def _engine(amd, lagged, B, depth, humans=5, policy=None, envs_per_wave=2):
    with environ(CROWDNAV_AMD_LAGGED_FILL=1 if lagged else 0, CROWDNAV_AMD_RING_DEPTH=depth, CROWDNAV_AMD_FUSED_SPLIT=1,
                 CROWDNAV_AMD_ENVS_PER_WAVE=envs_per_wave):
        return amd.BatchedCrowdSim(num_envs=B, num_humans=humans, robot_visible=1,
                                   robot_policy=amd.ROBOT_ORCA if policy is None else policy)


def _outputs(eng, bufs):
    eng.sync()
    out = dict(bufs)
    out['state'], out['global_time'] = eng.get_state()
    out['rollout_summary'] = eng.rollout_summary()
    return out


def _run(amd, lagged, B, depth, launches, route='fused_split', **engine):
    eng = _engine(amd, lagged, B, depth, **engine)
    assert eng.rollout_route(launches[0]) == route
    bufs = eng.rollout_begin(**BEGIN)
    counts = [eng.launch_counts()]
    for n in launches:
        eng.rollout(n)
        counts.append(eng.launch_counts())
    deltas = [{k: b[k] - a[k] for k in ('ring_fills', 'lagged_fills', 'rollout_kernels')} for a, b in zip(counts, counts[1:])]
    return _outputs(eng, bufs), deltas


def _oracle(oracle_mod, B, steps, humans=5):
    return oracle_rollout(oracle_mod, B, steps, K, num_humans=humans, robot_visible=1)


def _records_in_order(out, rec):
    return records_in_order(out, rec, K)


@pytest.mark.parametrize('depth', [2, 3])
def test_a_ring_that_runs_dry_pauses_the_same_envs(amd, oracle_mod, depth):
    """(a) headline geometry on the two-wave kernel, launches far beyond a ring of 2 / 3: envs pause inside the 120-step calls
    and resume after the next fill — the same envs, at the same steps, whether that fill ran in front of the launch or beside
    the previous one."""
    B, launches = 64, [120, 3, 120, 1, 2]
    want, d0 = _run(amd, False, B, depth, launches)
    got, d1 = _run(amd, True, B, depth, launches)
    _same(got, want)
    assert int(want['env_transitions'].sum()) < B * sum(launches)  # some env paused
    assert sum(d['lagged_fills'] for d in d1) >= 2 and sum(d['lagged_fills'] for d in d0) == 0
    _, _, rec, _, _ = _oracle(oracle_mod, B, sum(launches))
    _records_in_order(got, rec)


def test_default_depth_calls_longer_than_the_ring(amd, oracle_mod):
    """(b) the default ring, calls of 60 > 48 steps: calls 2 and 3 use up what is ahead and top the ring up beside themselves,
    for a repeat; the 7-step call takes up to 7 of those 48, so the last 60-step call fills in front of its launch again.
    Nobody pauses: everything equals the oracle's rollout."""
    B, launches = 64, [60, 60, 60, 7, 60]
    want, d0 = _run(amd, False, B, None, launches)
    got, d1 = _run(amd, True, B, None, launches)
    _same(got, want)
    assert [d['ring_fills'] for d in d0] == [1, 1, 1, 1, 1] and [d['lagged_fills'] for d in d0] == [0] * 5
    # 96 ahead after the fill in front of call 1, 48 after it: enough for call 2, which leaves 0 and a fill beside it (48 again)
    assert [d['lagged_fills'] for d in d1] == [0, 1, 1, 0, 0] and [d['ring_fills'] for d in d1] == [1, 1, 1, 0, 1]
    o, total, rec, cur_steps, cur_ret = _oracle(oracle_mod, B, sum(launches))
    assert int(got['env_transitions'].sum()) == total == B * sum(launches)
    assert np.array_equal(_records_in_order(got, rec), rec['count'])
    assert np.array_equal(_np(got['cur_steps']), cur_steps)
    assert np.allclose(_np(got['cur_return']), cur_ret, rtol=0, atol=1e-12)
    assert np.abs(_np(got['state']) - o.get_state()[0]).max() <= 1e-9


def test_a_mispredicted_sequence_falls_back_to_the_fill_in_front(amd):
    """(c) [5, 100, 5, 100] at the default depth, by fill_plan.h's rule (tests/fill_plan_check.cpp states the same sequence):
    call 1 fills to 96 ahead; call 2 (48 consumed at most) leaves 43 < 48, so a fill runs beside it, good for a repeat: 48
    ahead; call 3 takes up to 5 of those; call 4 needs 48, finds 43 and fills in front of its launch."""
    B, launches = 64, [5, 100, 5, 100]
    want, d0 = _run(amd, False, B, None, launches)
    got, d1 = _run(amd, True, B, None, launches)
    _same(got, want)
    assert [d['ring_fills'] for d in d1] == [1, 1, 0, 1] and [d['lagged_fills'] for d in d1] == [0, 1, 0, 0]
    assert [d['ring_fills'] for d in d0] == [1, 1, 1, 1] and [d['lagged_fills'] for d in d0] == [0, 0, 0, 0]
    assert all(d['rollout_kernels'] == 1 for d in d0 + d1)


def test_three_humans_on_the_one_wave_kernel(amd, oracle_mod):
    """(d) a geometry the two-wave kernel does not take: 3 humans, one-wave fused kernel, 130 steps through a ring of 3"""
    B, launches = 21, [50, 3, 70, 7]
    want, _ = _run(amd, False, B, 3, launches, route='fused', humans=3, envs_per_wave=None)
    got, d1 = _run(amd, True, B, 3, launches, route='fused', humans=3, envs_per_wave=None)
    _same(got, want)
    assert sum(d['lagged_fills'] for d in d1) >= 2
    _, _, rec, _, _ = _oracle(oracle_mod, B, sum(launches), humans=3)
    _records_in_order(got, rec)


def test_external_robot_through_rollout_step(amd):
    """(d) cn_rollout_step: 130 one-step calls with actions from outside, ring of 3 — a fill beside every third call"""
    import torch
    B, steps = 20, 130
    rng = np.random.RandomState(3)
    actions = torch.from_numpy(rng.uniform(-1.0, 1.0, (steps, B, 2)) * 0.7).cuda()

    def run(lagged):
        eng = _engine(amd, lagged, B, 3, policy=amd.ROBOT_EXTERNAL, envs_per_wave=None)
        bufs = eng.rollout_begin(**BEGIN)
        for t in range(steps):
            eng.rollout_step(actions[t])
        return _outputs(eng, bufs), eng.launch_counts()

    want, c0 = run(False)
    got, c1 = run(True)
    _same(got, want)
    assert int(got['ep_count'].min()) >= 1 and int(got['env_transitions'].sum()) == B * steps
    assert c0['lagged_fills'] == 0 and c1['lagged_fills'] >= steps // 3 - 2 and c1['ring_fills'] - c1['lagged_fills'] == 1


def test_reset_and_get_state_while_a_fill_is_in_flight(amd):
    """(e) entry points that touch env state from outside wait for the side stream first: get_state after a call that has a
    fill beside it, then a masked reset of some envs after another, then more calls"""
    B = 64
    seeds = 7000 + np.arange(B)
    mask = (np.arange(B) % 3 == 0).astype(np.uint8)

    def run(lagged):
        eng = _engine(amd, lagged, B, 3)
        bufs = eng.rollout_begin(**BEGIN)
        eng.rollout(40)
        eng.rollout(40)  # (a fill beside it)
        mid = [t.clone() for t in eng.get_state()]
        eng.rollout(40)  # (and beside this one)
        eng.reset(seeds, mask)
        eng.rollout(40)
        eng.rollout(5)
        out = _outputs(eng, bufs)
        out['mid_state'], out['mid_time'] = mid
        return out, eng.launch_counts()

    want, _ = run(False)
    got, c1 = run(True)
    _same(got, want)
    assert c1['lagged_fills'] >= 3


def test_rollout_begin_twice(amd):
    """(f) cn_rollout_begin while a fill of the previous rollout is in flight: it waits for it, restarts the ring, and the
    second rollout is the first one again"""
    B, launches = 64, [50, 50, 9]

    def run(lagged):
        eng = _engine(amd, lagged, B, 3)
        outs = []
        for _ in range(2):
            bufs = eng.rollout_begin(**BEGIN)  # (the second one right behind a call with a fill beside it: no sync in between)
            for n in launches:
                eng.rollout(n)
            eng.rollout(50)
            outs.append(bufs)
        eng.sync()
        return [{k: v for k, v in b.items()} for b in outs], eng.launch_counts()

    want, _ = run(False)
    got, c1 = run(True)
    _same(got[0], want[0])
    _same(got[1], want[1])
    _same(got[1], got[0])
    assert c1['lagged_fills'] >= 4
