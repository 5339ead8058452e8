"""cn_rollout_trace on the MI355X: the per-step rows of a batched ORCA rollout against the paths that already exist — the
stepwise loop (get_state + rollout(1): the fused / shard / generic kernels), cn_rollout's bookkeeping, the episode records and
the reference's trajectory fixtures.  Every comparison is bit for bit (np.array_equal): the traced kernel is the generic rollout
kernel's arithmetic with stores added, there is nothing to tolerate."""
import numpy as np
import pytest

from conftest import TRAJ_FIXTURES, episodes_of, load_golden
from support import amd, environ, np_of as _np  # noqa: F401  (amd: module fixture)

pytestmark = pytest.mark.gpu

FILL = dict(state8=-123.0, step=-5, reward=-123.0, info=77, dmin=-123.0)  # what rows the kernel must not write keep


def _engine(amd, B, H, **cfg):
    return amd.BatchedCrowdSim(num_envs=B, num_humans=H, robot_policy=amd.ROBOT_ORCA, **cfg)


def _begin(eng, L=-1):
    return eng.rollout_begin(seed_base=1000, seed_mod=500, episode_limit=L, record_capacity=8)


def _filled_out(eng, n):
    import torch
    B, A = eng.B, eng.A
    mk = lambda shape, dt, v: torch.full(shape, v, dtype=dt, device=eng.device)  # noqa: E731
    return dict(state8=mk((B, n, A, 8), torch.float64, FILL['state8']), episode=mk((B, n), torch.int32, 0),
                step=mk((B, n), torch.int32, FILL['step']), reward=mk((B, n), torch.float64, FILL['reward']),
                info=mk((B, n), torch.uint8, FILL['info']), dmin=mk((B, n), torch.float64, FILL['dmin']))


def _trace(eng, n, **kw):
    return {k: _np(v) for k, v in eng.rollout_trace(n, **kw).items()}


def _stepwise(eng, n):
    """n times (state, ep_count, cur_steps, active, then rollout(1)): what every env held before each step, and whether it
    made a transition there (its step or episode counter moved)."""
    import torch
    bufs = eng._rollout[1]
    st, ep, cs, ac = [], [], [], []
    for _ in range(n):
        st.append(eng.get_state()[0])
        ep.append(bufs['ep_count'].clone()), cs.append(bufs['cur_steps'].clone()), ac.append(bufs['active'].clone())
        eng.rollout(1)
    ep.append(bufs['ep_count'].clone()), cs.append(bufs['cur_steps'].clone())
    st, ep, cs, ac = (_np(torch.stack(x)) for x in (st, ep, cs, ac))
    moved = (ep[1:] != ep[:-1]) | (cs[1:] != cs[:-1])
    return dict(state8=st.transpose(1, 0, 2, 3), episode=ep[:-1].T, step=cs[:-1].T, running=(ac == 1).T, moved=moved.T)


CASES = {
    # the geometry of every engine above 2048 envs, asked for here: B = 3 leaves the second workgroup half full
    'two_envs_per_workgroup_ragged': dict(B=3, H=5, n=120, knobs=dict(CROWDNAV_AMD_ENVS_PER_WAVE=2)),
    'envs_retire': dict(B=5, H=5, n=120, L=7),
    'random_attributes_invisible': dict(B=4, H=5, n=90, cfg=dict(robot_visible=0, randomize_attributes=1)),
    'square_crossing': dict(B=4, H=5, n=90, cfg=dict(scenario_rule=1)),
    'one_human': dict(B=2, H=1, n=60),
    'ten_humans_maxl10': dict(B=2, H=10, n=60),
    'twenty_humans_kd': dict(B=3, H=20, n=60),
    'twenty_humans_async_fill': dict(B=3, H=20, n=60, cfg=dict(flags=1)),
}


@pytest.mark.parametrize('case', sorted(CASES))
def test_trace_equals_the_stepwise_path(amd, case):
    c = CASES[case]
    B, H, n, L, cfg = c['B'], c['H'], c['n'], c.get('L', -1), c.get('cfg', {})
    asynchronous = bool(cfg.get('flags', 0) & amd.FLAG_ASYNC_SCENARIO_FILL)
    with environ(**c.get('knobs', {})):
        x, y, z = (_engine(amd, B, H, **cfg) for _ in range(3))
    if 'knobs' in c:
        assert [e.geometry()['E'] for e in (x, y, z)] == [c['knobs']['CROWDNAV_AMD_ENVS_PER_WAVE']] * 3
    _begin(x, L)
    want = _stepwise(x, n)
    ybufs = _begin(y, L)
    got = _trace(y, n, rewards=True, out=_filled_out(y, n))
    y.sync()
    run = want['running']
    # With the synchronous ring fill (48 scenarios ahead of every env) no env ever waits, so "running before the step" and
    # "made a transition" are the same thing and X and Y move in lock step.  With the asynchronous fill an env may wait for its
    # next scenario at a moment that depends on when the side stream got there: X (n launches) and Y (one) need not pause alike.
    # Then the rows are matched by (env, episode, step) instead of by position; where neither paused that is the same check.
    paused = asynchronous and not (np.array_equal(run, want['moved']) and np.array_equal(got['episode'] >= 0, run))
    if not asynchronous:
        assert np.array_equal(run, want['moved'])
    if not paused:
        assert np.array_equal(got['episode'], np.where(run, want['episode'], -1))
        assert np.array_equal(got['step'][run], want['step'][run])
        assert np.array_equal(got['state8'][run], want['state8'][run])
    else:
        seen = {}
        for b, t in zip(*np.nonzero(run & want['moved'])):
            seen[(b, want['episode'][b, t], want['step'][b, t])] = want['state8'][b, t]
        common = 0
        for b, t in zip(*np.nonzero(got['episode'] >= 0)):
            key = (b, got['episode'][b, t], got['step'][b, t])
            if key in seen:
                common += 1
                assert np.array_equal(got['state8'][b, t], seen[key]), key
        assert common >= B * 20  # (no 20-human episode ends, hence no env waits, inside 20 steps)
    # rows of an env that made no transition: episode -1, everything else as the caller left it
    idle = got['episode'] < 0
    assert (got['state8'][idle] == FILL['state8']).all() and (got['step'][idle] == FILL['step']).all()
    assert (got['reward'][idle] == FILL['reward']).all() and (got['info'][idle] == FILL['info']).all()
    assert (got['dmin'][idle] == FILL['dmin']).all()
    live = ~idle
    assert (got['info'][live] <= amd.TIMEOUT).all() and (got['step'][live] >= 0).all()
    if L >= 0:
        assert idle.any() and live.any()  # some env retired inside the call
    # the engine afterwards: exactly what one rollout(n) leaves
    zbufs = _begin(z, L)
    z.rollout(n)
    z.sync()
    assert y.launch_counts()['rollout_kernels'] == 1 == z.launch_counts()['rollout_kernels']
    assert y.launch_counts()['scheduled_kernels'] == 0
    same_pauses = not asynchronous or (int(_np(ybufs['transitions'])[0]) == B * n == int(_np(zbufs['transitions'])[0]))
    if same_pauses:
        assert sorted(ybufs) == sorted(zbufs)
        for k in ybufs:
            assert np.array_equal(_np(ybufs[k]), _np(zbufs[k])), k
        assert np.array_equal(_np(y.get_state()[0]), _np(z.get_state()[0]))
        assert np.array_equal(_np(y.get_state()[1]), _np(z.get_state()[1]))
        assert int(_np(ybufs['transitions'])[0]) == int(live.sum())


def test_chunks_concatenate(amd):
    B, H = 3, 5
    whole_eng = _engine(amd, B, H)
    _begin(whole_eng)
    whole = _trace(whole_eng, 120, rewards=True)
    assert (whole['episode'] >= 0).all() and whole['episode'].max() >= 2  # every row written; several auto-resets
    a = _engine(amd, B, H)
    _begin(a)
    first, second = _trace(a, 37, rewards=True), _trace(a, 83, rewards=True)
    for k in whole:
        assert np.array_equal(np.concatenate([first[k], second[k]], axis=1), whole[k]), k
    # an untraced call in between: the traced rows on either side are the matching rows of the whole
    b = _engine(amd, B, H)
    _begin(b)
    head = _trace(b, 37, rewards=True)
    b.rollout(10)
    tail = _trace(b, 73, rewards=True)
    for k in whole:
        assert np.array_equal(head[k], whole[k][:, :37]), k
        assert np.array_equal(tail[k], whole[k][:, 47:]), k
    # without rewards: the same required arrays, nothing else
    c = _engine(amd, B, H)
    _begin(c)
    bare = _trace(c, 120)
    assert sorted(bare) == ['episode', 'state8', 'step']
    for k in bare:
        assert np.array_equal(bare[k], whole[k]), k


def test_records_follow_from_the_trace(amd):
    from crowdnav_amd.trace import episodes
    B, H, n, gamma = 3, 5, 150, 0.9  # (4, 6 and 5 finished episodes: inside the 8-record ring)
    eng = _engine(amd, B, H)
    eng.set_gamma(gamma)
    bufs = _begin(eng)
    tr = _trace(eng, n, rewards=True)
    rec = {k: _np(v) for k, v in bufs.items()}
    eps = episodes(tr)
    dt, v_pref = eng.config['time_step'], eng.config['robot_v_pref']
    finished = 0
    for b in range(B):
        assert 2 <= rec['ep_count'][b] <= 8  # several episodes, none overwritten in the 8-record ring
        for j in range(int(rec['ep_count'][b])):
            e = eps[b + j * B]
            finished += 1
            assert e['complete'] is True
            assert int((tr['episode'][b] == j).sum()) == len(e['state8']) == rec['ep_steps'][b, j]
            assert e['info'][-1] == rec['ep_outcome'][b, j]
            ret = 0.0
            for t, r in enumerate(e['reward'].tolist()):  # explorer.py:71: python's left-to-right sum
                ret = ret + pow(gamma, t * dt * v_pref) * r
            assert np.float64(ret).tobytes() == rec['ep_return'][b, j].tobytes()
            danger = e['info'] == amd.DANGER
            dsum = 0.0
            for d in e['dmin'][danger].tolist():
                dsum += d
            assert int(danger.sum()) == rec['ep_danger'][b, j]
            assert np.float64(dsum).tobytes() == rec['ep_danger_dmin_sum'][b, j].tobytes()
        cur = eps.get(b + int(rec['ep_count'][b]) * B)  # the episode the call cut
        assert (0 if cur is None else len(cur['state8'])) == rec['cur_steps'][b]
        assert cur is None or cur['complete'] is False
    assert finished == int(rec['ep_count'].sum())


@pytest.mark.parametrize('name', ['traj_invisible_h5.npz', 'traj_visible_h5.npz', 'traj_visible_h5_square.npz',
                                  'traj_visible_h10.npz', 'traj_visible_h20.npz', 'traj_debug_case.npz'])
def test_trace_vs_reference_fixtures(amd, name):
    """The fixtures of test_free_running_trajectories_vs_reference, free running from their initial states inside ONE traced
    call: the rows of every env's ordinal 0 are the reference's env.states, rewards and infos.  (dmins: where the info is
    Danger — the reference reports a min_dist with Danger only, the fixtures hold NaN elsewhere.)"""
    g = load_golden(name)
    eps = episodes_of(g)
    B = len(eps)
    T = max(len(e['actions']) for e in eps)
    eng = amd.BatchedCrowdSim(num_envs=B, robot_policy=amd.ROBOT_ORCA, **TRAJ_FIXTURES[name])
    _begin(eng)
    eng.set_state(np.stack([e['states'][0] for e in eps]), np.zeros(B))
    tr = _trace(eng, T, rewards=True)
    for b, e in enumerate(eps):
        Tb = len(e['actions'])
        assert np.array_equal(np.flatnonzero(tr['episode'][b] == 0), np.arange(Tb))
        assert np.array_equal(tr['step'][b, :Tb], np.arange(Tb))
        assert np.array_equal(tr['state8'][b, :Tb], e['states'][:Tb])
        assert np.array_equal(tr['reward'][b, :Tb], e['rewards'])
        assert np.array_equal(tr['info'][b, :Tb], e['infos'])
        danger = e['infos'] == amd.DANGER
        assert np.array_equal(tr['dmin'][b, :Tb][danger], e['dmins'][danger])
        if Tb < T:  # the next row is the next episode's reset state
            assert tr['episode'][b, Tb] == 1 and tr['step'][b, Tb] == 0


def test_refusals(amd):
    import torch
    ext = amd.BatchedCrowdSim(num_envs=2, num_humans=5, robot_policy=amd.ROBOT_EXTERNAL)
    _begin(ext)
    with pytest.raises(amd.CrowdNavAmdError) as ei:
        ext.rollout_trace(5)
    assert ei.value.status == -2 and 'cn_rollout_step' in str(ei.value)  # CN_ERR_UNSUPPORTED
    eng = _engine(amd, 2, 5)
    with pytest.raises(RuntimeError):
        eng.rollout_trace(5)  # no rollout_begin yet
    _begin(eng)
    before = eng.launch_counts()
    good = eng.rollout_trace(0, rewards=True)  # a no-op, as rollout(0)
    assert good['state8'].shape == (2, 0, 6, 8) and eng.launch_counts() == before
    out = _filled_out(eng, 6)
    for k, bad in (('state8', out['state8'][:, :5]), ('episode', out['episode'].to(torch.int64)),
                   ('step', out['step'].cpu()), ('info', None)):
        wrong = dict(out)
        wrong[k] = bad
        with pytest.raises(ValueError):
            eng.rollout_trace(6, rewards=True, out=wrong)
    with pytest.raises(ValueError):
        eng.rollout_trace(5, out=out)  # rows for 6 steps
    assert eng.launch_counts() == before
    eng.rollout_trace(6, rewards=True, out=out)  # and the right one goes through, reused in place
    assert eng.launch_counts()['rollout_kernels'] == before['rollout_kernels'] + 1
    assert (_np(out['episode']) == 0).all() and (_np(out['step'])[:, 0] == 0).all()


def _explorer(keep):
    import crowdnav_amd.compat as c
    from crowdnav_amd.compat import explorer as explorer_mod
    cfg = c.default_env_config()
    env = c.CrowdSim()
    env.configure(cfg)
    robot = c.Robot(cfg, 'robot')
    policy = c.ORCA()
    robot.set_policy(policy)
    env.set_robot(robot)
    policy.set_env(env)
    ex = c.Explorer(env, robot, 'cuda:0', gamma=0.9)
    if keep is not None:
        ex.keep_trajectories = keep
    return explorer_mod, env, ex


def test_explorer_keeps_trajectories_on_request(amd, monkeypatch):
    explorer_mod, env, ex = _explorer(None)
    assert ex.keep_trajectories is False and explorer_mod.Explorer.keep_trajectories is False

    class Spy(amd.BatchedCrowdSim):
        engines = []

        def __init__(self, **cfg):
            super().__init__(**cfg)
            self.calls = []
            Spy.engines.append(self)

        def rollout(self, n_steps):
            self.calls.append('rollout')
            return super().rollout(n_steps)

        def rollout_trace(self, n_steps, rewards=False, out=None):
            self.calls.append('rollout_trace')
            return super().rollout_trace(n_steps, rewards=rewards, out=out)

    monkeypatch.setattr(explorer_mod, 'BatchedCrowdSim', Spy)
    # default: nothing recorded, one rollout launch (the fused kernel) per loop turn as before
    ex.run_k_episodes(20, 'test')
    plain = dict(ex.last_batch)
    assert 'trajectories' not in plain
    eng = Spy.engines[-1]
    assert eng.calls and set(eng.calls) == {'rollout'}
    assert eng.launch_counts()['rollout_kernels'] == len(eng.calls)
    # on request: the same episodes, and their states
    explorer_mod2, env2, ex2 = _explorer(True)
    ex2.run_k_episodes(20, 'test')
    lb = ex2.last_batch
    eng2 = Spy.engines[-1]
    assert eng2 is not eng and set(eng2.calls) == {'rollout_trace'} and len(eng2.calls) == len(eng.calls)
    assert eng2.launch_counts()['rollout_kernels'] == len(eng2.calls)
    assert {k: lb[k] for k in plain} == plain
    traj = lb['trajectories']
    assert len(traj) == 20 and [len(t) for t in traj] == lb['steps']
    assert all(t.dtype == np.float64 and t.shape[1:] == (6, 8) for t in traj)
    fresh = amd.BatchedCrowdSim(**env2.engine_config(20, 5, 'circle_crossing', amd.ROBOT_ORCA))
    fresh.reset(1000 + np.arange(20))  # the test phase's cases 0..19
    assert np.array_equal(np.stack([t[0] for t in traj]), _np(fresh.get_state()[0]))
