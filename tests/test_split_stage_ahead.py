"""The two-wave fused rollout kernel around episode ends.  Its ORCA wave stages the view of the NEXT step ahead of barrier 1 and
keeps two per-episode constants (the pairs' combined radii, which agents solve) in registers, refreshed only in an iteration
that follows an episode end (rollout_fused.h: split_orca_wave) — so what this file pins is every way an episode end can fall:

    in a launch's first step, in its last step, in two consecutive steps of a workgroup, in one env of a workgroup only and in
    both at once, in launches of 1 and of 2 steps, with the state carried across launches; an env that pauses because the ring
    ran dry and an env that retires at its episode limit (both stop solving: a refreshed constant is read).

The ends are placed by construction, not found by seeds: a time limit of a few steps (crowd_sim.py: Timeout once global_time >=
time_limit - 1, so time_limit = 1 + k dt ends every episode in its step k + 1), global_time offsets per env (cn_set_state) that
stagger the envs of a workgroup, and a robot whose goal is one step away (ReachGoal in the first step of the launch).

Every case runs the two-wave kernel against the one-wave kernel (CROWDNAV_AMD_FUSED_SPLIT=0): EVERY output bit for bit.  The
cases without a pause or a retirement — the oracle models neither — also run against the oracle: global_time, episode counts,
record rings (outcome, steps, time, Danger steps) and the running episode's counters exactly; returns (float64 sums) and the
state — which after an auto-reset holds device-generated scenarios — to the suite's 1e-9."""
import numpy as np
import pytest

from support import amd, environ, np_of as _np  # noqa: F401  (amd: module fixture)

pytestmark = pytest.mark.gpu

DT = 0.25
K = 16  # record ring slots


def _cfg(time_limit):
    return dict(num_humans=5, robot_visible=1, time_limit=time_limit)


def _start(oracle_mod, B, cfg, near_goal=()):
    """the seeded first scenarios (seed 1000 + env), the robots of `near_goal` 0.2 m from their goals"""
    ora = oracle_mod.CrowdOracle(num_envs=B, robot_policy=1, **cfg)
    ora.reset(1000 + np.arange(B))
    st = ora.get_state()[0].copy()
    for b in near_goal:
        st[b, 0, 4:6] = st[b, 0, 0:2] + np.array([0.0, 0.2])
    return st


def _run(amd, split, B, launches, cfg, state, gtime, ring_depth=None, **begin):
    with environ(CROWDNAV_AMD_FUSED_SPLIT=1 if split else 0, CROWDNAV_AMD_ENVS_PER_WAVE=2, CROWDNAV_AMD_RING_DEPTH=ring_depth,
                 CROWDNAV_AMD_FUSED=None, CROWDNAV_AMD_SPLIT_ASSIST=None):
        eng = amd.BatchedCrowdSim(num_envs=B, robot_policy=amd.ROBOT_ORCA, **cfg)
    assert eng.rollout_route(launches[0]) == ('fused_split' if split else 'fused')
    begin.setdefault('episode_limit', -1)
    bufs = eng.rollout_begin(seed_base=1000, seed_mod=500, record_capacity=K, per_env_transitions=True, **begin)
    eng.set_state(state, gtime)
    for n in launches:
        eng.rollout(n)
    eng.sync()
    s, g = eng.get_state()
    out = {k: _np(v) for k, v in bufs.items()}
    out['state'], out['global_time'] = _np(s), _np(g)
    return out


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k


def _oracle(oracle_mod, B, cfg, state, gtime, steps):
    ora = oracle_mod.CrowdOracle(num_envs=B, robot_policy=1, **cfg)
    ora.reset(1000 + np.arange(B))
    ora.set_state(state, gtime)
    total, rec, cur = ora.rollout_full(steps, 1000, 500, K)
    s, g = ora.get_state()
    return total, rec, cur, s, g


def _same_as_oracle(got, want, B, steps):
    total, rec, cur, s, g = want
    assert total == B * steps and np.array_equal(got['env_transitions'].astype(np.int64), np.full(B, steps))  # nobody paused
    assert np.array_equal(got['ep_count'], rec['count'])
    live = np.arange(K)[None, :] < rec['count'][:, None]
    assert rec['count'].max() <= K
    for key, name in (('ep_outcome', 'outcome'), ('ep_steps', 'steps'), ('ep_time', 'time'), ('ep_danger', 'danger')):
        assert np.array_equal(np.where(live, got[key], 0), np.where(live, rec[name], 0)), key
    assert np.abs(np.where(live, got['ep_return'] - rec['ret'], 0)).max() <= 1e-9
    assert np.array_equal(got['cur_steps'], cur['steps']) and np.array_equal(got['cur_danger'], cur['danger'])
    assert np.abs(got['cur_return'] - cur['ret']).max() <= 1e-9
    assert np.array_equal(got['active'], np.ones(B, dtype=got['active'].dtype)), ('active', got['active'])
    assert np.array_equal(got['global_time'], g), ('global_time', got['global_time'], g)
    # a state behind an auto-reset holds scenarios the DEVICE generated: its sin / cos may differ from libm's in the last ulp,
    # so the suite holds such states to 1e-9 (test_bench_size_parity.py); the kernels among themselves are byte-equal (above)
    assert np.abs(got['state'] - s).max() <= 1e-9, ('state', np.argwhere(got['state'] != s).tolist())


# time_limit = 1 + k dt: an episode that starts at global_time 0 ends (Timeout) in its step k + 1; `offsets` (in steps) is the
# global_time the envs start with, so env b's first episode ends in step k + 1 - offsets[b] and every k + 1 steps after that.
# ends: the launch steps (1-based, over the concatenated launches) in which env b must have ended an episode — asserted.
CASES = {
    # every step ends an episode of every env: first step, last step, consecutive steps, both envs of a workgroup at once
    'every_step': dict(B=2, k=0, offsets=[0, 0], launches=[4], ends=[[1, 2, 3, 4]] * 2),
    'every_step_n1': dict(B=2, k=0, offsets=[0, 0], launches=[1], ends=[[1]] * 2),
    'every_step_n2': dict(B=2, k=0, offsets=[0, 0], launches=[2], ends=[[1, 2]] * 2),
    # k = 2: env 0 ends in steps 3, 6, env 1 (one step ahead) in 2, 5: one env of the workgroup only, in consecutive steps;
    # the second workgroup (envs 2, 3) ends both at once; 6 = the launch's last step
    'staggered': dict(B=4, k=2, offsets=[0, 1, 0, 0], launches=[6], ends=[[3, 6], [2, 5], [3, 6], [3, 6]]),
    # the same 6 steps across launches: ends in a launch's first step (step 3 = first of the second launch, step 6 = first of
    # the fourth) and last step (2, 5), launches of 1 and 2 steps, the carried state
    'staggered_cut': dict(B=4, k=2, offsets=[0, 1, 0, 0], launches=[2, 1, 2, 1], ends=[[3, 6], [2, 5], [3, 6], [3, 6]]),
    # a robot one step from its goal: ReachGoal in the launch's first step, in env 0 of the workgroup only
    'goal_in_first_step': dict(B=2, k=6, offsets=[0, 0], launches=[2, 3], near_goal=(0,), ends=[[1], []]),
    'goal_in_first_step_n1': dict(B=2, k=6, offsets=[0, 0], launches=[1, 1], near_goal=(0, 1), ends=[[1], [1]]),
}


def _inputs(oracle_mod, case):
    cfg = _cfg(1.0 + case['k'] * DT)
    B = case['B']
    state = _start(oracle_mod, B, cfg, case.get('near_goal', ()))
    gtime = np.asarray(case['offsets'], dtype=np.float64) * DT
    return cfg, B, state, gtime


@pytest.mark.parametrize('name', list(CASES))
def test_episode_ends_by_construction(amd, oracle_mod, name):
    case = CASES[name]
    cfg, B, state, gtime = _inputs(oracle_mod, case)
    launches, steps = case['launches'], sum(case['launches'])
    # the oracle first: the ends fall where the case says (steps of the records, in order)
    want = _oracle(oracle_mod, B, cfg, state, gtime, steps)
    rec = want[1]
    for b in range(B):
        ends = np.cumsum(rec['steps'][b, :rec['count'][b]]).tolist()  # (record steps count the steps run here)
        assert ends == case['ends'][b], (name, b, ends)
    one = _run(amd, False, B, launches, cfg, state, gtime)
    two = _run(amd, True, B, launches, cfg, state, gtime)
    _same(two, one)
    _same_as_oracle(two, want, B, steps)


def test_pause_and_retire(amd, oracle_mod):
    """Every step ends an episode (time_limit = 1).  A ring of two scenarios runs dry inside the first launch: the envs pause
    (no agent solves any more: the ORCA wave must see the refreshed constant, not the last episode's), resume after the next
    call's fill, and pause again.  With an episode limit of B the envs retire after their first episode instead."""
    cfg = _cfg(1.0)
    B = 4
    state = _start(oracle_mod, B, cfg)
    gtime = np.zeros(B)
    launches = [5, 1, 2, 4]
    one = _run(amd, False, B, launches, cfg, state, gtime, ring_depth=2)
    two = _run(amd, True, B, launches, cfg, state, gtime, ring_depth=2)
    _same(two, one)
    assert (one['env_transitions'] < sum(launches)).all() and (one['ep_count'] >= 3).all()  # paused, resumed
    one = _run(amd, False, B, [3, 1], cfg, state, gtime, episode_limit=B)
    two = _run(amd, True, B, [3, 1], cfg, state, gtime, episode_limit=B)
    _same(two, one)
    assert (one['active'] == 0).all() and (one['ep_count'] == 1).all() and (one['env_transitions'] == 1).all()  # retired
