"""cn_rollout_actions on the MI355X: one launch with a table of actions against the n rollout_step launches it replaces (bit for
bit: the table kernel is the step kernel's arithmetic with another address for the action), its per-step rows against the
step loop's snapshots and cn_step, the reference's own recorded episodes replayed, and a captured call."""
import contextlib
import os

import numpy as np
import pytest

from conftest import load_golden
from support import (  # noqa: F401  (amd: module fixture)
    action_table, amd, environ, external_engine as _engine, np_of as _np, rollout_after as _after,
    rollout_step_loop as _step_loop, same_tensors as _same)

pytestmark = pytest.mark.gpu

BEGIN = dict(seed_base=1000, seed_mod=500, record_capacity=8)


def _table(B, T, unicycle=False, seed=7):
    return action_table(B, T, unicycle=unicycle, seed=seed)


def _case_engine(amd, c):
    """The case's engine; under the case's `knobs`, with the geometry they ask for asserted."""
    with environ(**c.get('knobs', {})):
        eng = _engine(amd, c['B'], c['H'], **c['cfg'])
    if 'knobs' in c:
        assert eng.geometry()['E'] == c['knobs']['CROWDNAV_AMD_ENVS_PER_WAVE'], eng.geometry()
    return eng


CASES = {
    # T = 70 over 32-step episodes (time_limit 8): every env passes two episode ends; two envs per workgroup (the geometry of
    # every engine above 2048 envs, asked for here), so B = 3 half-fills the last workgroup
    'ragged_two_episode_ends': dict(B=3, H=5, T=70, cfg=dict(robot_visible=1, time_limit=8.0),
                                    knobs=dict(CROWDNAV_AMD_ENVS_PER_WAVE=2)),
    'one_human': dict(B=2, H=1, T=70, cfg=dict(robot_visible=1, time_limit=8.0)),
    'twelve_humans_ten_half_planes_kd': dict(B=2, H=12, T=40, cfg=dict(robot_visible=1, time_limit=8.0)),
    'unicycle': dict(B=3, H=5, T=70, cfg=dict(robot_visible=1, time_limit=8.0, robot_kinematics=1), unicycle=True),
    'mixed_rule': dict(B=4, H=5, T=70, cfg=dict(robot_visible=1, time_limit=8.0, scenario_rule=2)),
    'two_calls_33_37': dict(B=3, H=5, T=70, cfg=dict(robot_visible=1, time_limit=8.0), split=(33, 37)),
    'envs_retire': dict(B=3, H=5, T=70, cfg=dict(robot_visible=1, time_limit=8.0), limit=4),
}


@pytest.mark.parametrize('case', sorted(CASES))
def test_one_table_call_equals_the_step_loop(amd, case):
    import torch
    c = CASES[case]
    B, H, T, cfg, limit = c['B'], c['H'], c['T'], c['cfg'], c.get('limit', -1)
    table = torch.from_numpy(_table(B, T, c.get('unicycle', False))).cuda()
    x = _case_engine(amd, c)
    xbufs = x.rollout_begin(episode_limit=limit, **BEGIN)
    _step_loop(x, xbufs, table)
    want = _after(x, xbufs)
    y = _case_engine(amd, c)
    ybufs = y.rollout_begin(episode_limit=limit, **BEGIN)
    before = y.launch_counts()
    calls = c.get('split', (T,))
    t0 = 0
    for n in calls:
        assert y.rollout_actions(table[:, t0:t0 + n].contiguous()) is ybufs
        t0 += n
    got = _after(y, ybufs)
    counts = y.launch_counts()
    assert counts['rollout_kernels'] == before['rollout_kernels'] + len(calls)
    assert counts['scheduled_kernels'] == before['scheduled_kernels']
    assert x.launch_counts()['rollout_kernels'] == T
    _same(got, want)
    # ... and the case is what it claims to be
    ep_count, outcome = _np(got['ep_count']), _np(got['ep_outcome'])
    if limit < 0:
        assert (ep_count >= (2 if T >= 64 else 1)).all(), ep_count
        assert int(_np(got['transitions'])[0]) == B * T  # nobody waited for a scenario
    else:  # episode_limit = B + 1: env 0 runs a second episode, the others retire after their first
        assert ep_count.tolist() == [2] + [1] * (B - 1) and _np(got['active']).tolist() == [0] * B
    if case == 'ragged_two_episode_ends':
        assert (outcome[:, :2] == amd.TIMEOUT).any()
    if case == 'unicycle':
        assert (_np(got['theta']) != np.pi / 2).any()  # the heading was carried


def test_retired_envs_keep_their_last_state_and_write_no_rows(amd):
    import torch
    c = CASES['envs_retire']
    B, H, T = c['B'], c['H'], c['T']
    table = torch.from_numpy(_table(B, T)).cuda()
    y = _engine(amd, B, H, **c['cfg'])
    ybufs = y.rollout_begin(episode_limit=c['limit'], **BEGIN)
    tr = {k: _np(v) for k, v in y.rollout_actions(table, trace=True, rewards=True).items()}
    y.sync()
    steps = _np(ybufs['ep_steps'])
    final = _np(y.get_state()[0])
    for b in range(1, B):
        n = int(steps[b, 0])
        assert (tr['episode'][b, :n] == 0).all() and (tr['episode'][b, n:] == -1).all()
        # its state stays as the last transition left it: the positions of row n - 1 moved by that step, not a reset state
        x = _engine(amd, B, H, **c['cfg'])
        xbufs = x.rollout_begin(episode_limit=c['limit'], **BEGIN)
        _step_loop(x, xbufs, table[:, :n])
        x.sync()
        assert np.array_equal(_np(x.get_state()[0])[b], final[b])
    n0 = int(steps[0, 0]) + int(steps[0, 1])
    assert (tr['episode'][0, :n0] >= 0).all() and (tr['episode'][0, n0:] == -1).all() and tr['episode'][0, n0 - 1] == 1


@pytest.fixture(scope='module')
def case_one(amd):
    """Case one, three ways: the step loop with snapshots (X), one traced table call with rewards (Y), and cn_step on an
    engine reset to the same seeds and driven by the same actions (Z)."""
    import torch
    c = CASES['ragged_two_episode_ends']
    B, H, T, cfg = c['B'], c['H'], c['T'], c['cfg']
    table = torch.from_numpy(_table(B, T)).cuda()
    x = _case_engine(amd, c)
    xbufs = x.rollout_begin(**BEGIN)
    snaps = dict(state8=[], ep_count=[], cur_steps=[], active=[])
    _step_loop(x, xbufs, table, snaps)
    want = _after(x, xbufs)
    snaps = {k: _np(torch.stack(v)).swapaxes(0, 1) for k, v in snaps.items()}  # [B, T, ...]
    y = _case_engine(amd, c)
    ybufs = y.rollout_begin(**BEGIN)
    before = y.launch_counts()['rollout_kernels']
    rows = y.rollout_actions(table, trace=True, rewards=True)
    got = _after(y, ybufs)
    assert y.launch_counts()['rollout_kernels'] == before + 1
    z = _engine(amd, B, H, **cfg)
    z.reset(BEGIN['seed_base'] + np.arange(B))
    stepped = dict(reward=[], info=[], dmin=[])
    for t in range(T):
        out = z.step(table[:, t].contiguous(), want_obs=False)
        for k in stepped:
            stepped[k].append(out[k].clone())
    stepped = {k: _np(torch.stack(v)).T for k, v in stepped.items()}  # [B, T]
    return dict(B=B, T=T, table=table, want=want, got=got, snaps=snaps, rows={k: _np(v) for k, v in rows.items()},
                stepped=stepped, cfg=cfg, H=H)


def test_trace_rows_are_the_step_loops_snapshots(amd, case_one):
    s, rows = case_one['snaps'], case_one['rows']
    _same(case_one['got'], case_one['want'])  # tracing changes nothing of the rollout
    run = s['active'] == 1
    assert run.all()  # (ring depth 48: no env waits, none retires)
    assert np.array_equal(rows['episode'], s['ep_count'])
    assert np.array_equal(rows['step'], s['cur_steps'])
    assert np.array_equal(rows['state8'], s['state8'])


def test_trace_rewards_are_cn_steps(amd, case_one):
    rows, stepped = case_one['rows'], case_one['stepped']
    first = rows['episode'] == 0
    assert first[:, 0].all() and first.sum() == int(_np(case_one['got']['ep_steps'])[:, 0].sum())
    for k in ('reward', 'info', 'dmin'):
        assert np.array_equal(rows[k][first].view(np.uint8), stepped[k][first].view(np.uint8)), k


def test_trace_cuts_into_the_recorded_episodes(amd, case_one):
    from crowdnav_amd.trace import episodes
    B, got = case_one['B'], {k: _np(v) for k, v in case_one['got'].items()}
    eps = episodes(case_one['rows'])
    finished = 0
    for b in range(B):
        assert 2 <= got['ep_count'][b] <= 8
        for j in range(int(got['ep_count'][b])):
            e = eps[b + j * B]
            finished += 1
            assert e['complete'] is True and len(e['state8']) == got['ep_steps'][b, j]
            assert e['info'][-1] == got['ep_outcome'][b, j]
        cut = eps.get(b + int(got['ep_count'][b]) * B)
        assert (0 if cut is None else len(cut['state8'])) == got['cur_steps'][b]
        assert cut is None or cut['complete'] is False
    assert finished == int(got['ep_count'].sum()) == sum(1 for e in eps.values() if e['complete'])


def test_untraced_call_and_reused_rows_give_the_same_bits(amd, case_one):
    import torch
    B, H, T, table = case_one['B'], case_one['H'], case_one['T'], case_one['table']
    y = _engine(amd, B, H, **case_one['cfg'])
    ybufs = y.rollout_begin(**BEGIN)
    y.rollout_actions(table)
    _same(_after(y, ybufs), case_one['want'])
    # without rewards: the required arrays only; a host table is copied (and the call synchronises)
    ybufs = y.rollout_begin(**BEGIN)
    bare = y.rollout_actions(_np(table), trace=True)
    assert sorted(bare) == ['episode', 'state8', 'step']
    for k in bare:
        assert np.array_equal(_np(bare[k]), case_one['rows'][k]), k
    # the previous call's dict as out: validated, refilled, written in place
    ybufs = y.rollout_begin(**BEGIN)
    bare['step'].fill_(-5)
    again = y.rollout_actions(table, trace=True, out=bare)
    assert again['state8'].data_ptr() == bare['state8'].data_ptr()
    assert np.array_equal(_np(again['step']), case_one['rows']['step'])
    with pytest.raises(ValueError):
        y.rollout_actions(table[:, :5].contiguous(), trace=True, out=bare)  # rows for T steps
    with pytest.raises(ValueError):
        y.rollout_actions(table[:, :, :1])
    assert torch.equal(y.rollout_actions(table[:, :0])['ep_count'], ybufs['ep_count'])  # no steps: no-op


def test_refusals_on_an_engine(amd):
    import ctypes as C
    import torch
    from crowdnav_amd import _lib
    table = torch.zeros(2, 4, 2, dtype=torch.float64, device='cuda')
    orca = amd.BatchedCrowdSim(num_envs=2, num_humans=5, robot_policy=amd.ROBOT_ORCA)
    orca.rollout_begin(**BEGIN)
    before = orca.launch_counts()
    with pytest.raises(amd.CrowdNavAmdError) as ei:
        orca.rollout_actions(table)
    assert ei.value.status == _lib.CN_ERR_INVALID and 'cn_rollout' in str(ei.value)
    assert orca.launch_counts() == before
    ext = _engine(amd, 2, 5)
    with pytest.raises(RuntimeError):
        ext.rollout_actions(table)  # no rollout_begin yet
    ext.rollout_begin(**BEGIN)
    before = ext.launch_counts()
    lib, io = ext._lib, ext._rollout[0]
    ptr = C.c_void_p(table.data_ptr())
    assert lib.cn_rollout_actions(ext._h, C.byref(io), 0, ptr, None) == _lib.CN_OK  # nothing launched, nothing counted
    assert lib.cn_rollout_actions(ext._h, C.byref(io), -1, ptr, None) == _lib.CN_ERR_INVALID
    assert lib.cn_rollout_actions(ext._h, C.byref(io), 4, None, None) == _lib.CN_ERR_INVALID
    assert lib.cn_rollout_actions(ext._h, C.byref(io), 4, ptr, C.byref(_lib.CnTraceOut())) == _lib.CN_ERR_INVALID
    bad = _lib.CnRolloutIo.from_buffer_copy(io)
    bad.seed_mod = 0
    assert lib.cn_rollout_actions(ext._h, C.byref(bad), 4, ptr, None) == _lib.CN_ERR_INVALID
    assert 'seed_mod' in lib.cn_last_error().decode()
    assert ext.launch_counts() == before
    ext.rollout_actions(table)
    assert ext.launch_counts()['rollout_kernels'] == before['rollout_kernels'] + 1


# ------------------------------------------------------------------------------------- the reference's own episodes
@pytest.mark.parametrize('name', ['rl_sarl_plain.npz', 'rl_lstm_rl_om.npz'])
def test_reference_episodes_replayed(amd, name):
    """The epsilon-greedy train-phase episodes the unmodified reference ran (oracle/gen_golden_rl.py), replayed open loop from
    their recorded action indices: same outcomes, lengths and times, and the rewards of every step.
    Reward tolerance: 1e-6, what tests/test_rl_pipeline.py allows between these fixtures' memory_values — float32 TD targets
    whose terminal rows ARE these rewards — and the device's."""
    import torch
    from rl_pipeline_cases import setup as _setup
    g = load_golden(name)
    c, env, robot, policy = _setup(g)
    k, steps = int(g['k']), g['ep_steps'].astype(np.int64)
    T = int(steps.max())
    ex = c.Explorer(env, robot, torch.device('cpu'), None, float(g['gamma']), target_policy=policy)
    human_num, rule, offset = ex._scenario_of('train')
    idx = g['ep_actions'][:, :T]
    table = np.where((idx >= 0)[..., None], g['action_space'][np.maximum(idx, 0)], 0.0)
    eng = amd.BatchedCrowdSim(**env.engine_config(k, human_num, rule, amd.ROBOT_EXTERNAL))
    assert eng.config['robot_visible'] == int(g['robot_visible'])
    eng.set_gamma(float(g['gamma']))
    bufs = eng.rollout_begin(seed_base=offset + int(g['first_case']), seed_mod=env.case_size['train'], episode_limit=k,
                             record_capacity=1)
    rows = eng.rollout_actions(torch.from_numpy(table).to(eng.device), trace=True, rewards=True)
    eng.sync()
    assert _np(bufs['ep_count']).tolist() == [1] * k and _np(bufs['active']).tolist() == [0] * k
    assert np.array_equal(_np(bufs['ep_outcome'])[:, 0], g['ep_outcome'])
    assert np.array_equal(_np(bufs['ep_steps'])[:, 0], steps)
    # The fixture's ep_time is env.global_time when the episode ended.  The engine's record is the time Explorer.run_k_episodes
    # books (explorer.py:52-62): the same for ReachGoal and Collision, env.time_limit for Timeout (tests/test_gpu_parity.py pins
    # that for every rollout path).  So: the record against the fixture where the two mean the same and against time_limit
    # where they do not, and the fixture's own number against the clock of the traced rows (last step index + 1) x time_step,
    # for every episode.
    timeout = g['ep_outcome'] == amd.TIMEOUT
    booked = np.where(timeout, eng.config['time_limit'], g['ep_time'])
    last = np.array([_np(rows['step'])[b, int(steps[b]) - 1] for b in range(k)])
    clock = (last + 1) * eng.config['time_step']
    print('ep_time: largest difference %.3e (records), %.3e (clock of the rows)'
          % (np.abs(_np(bufs['ep_time'])[:, 0] - booked).max(), np.abs(clock - g['ep_time']).max()))
    assert np.abs(_np(bufs['ep_time'])[:, 0] - booked).max() <= 1e-9
    assert np.abs(clock - g['ep_time']).max() <= 1e-9
    reward, episode = _np(rows['reward']), _np(rows['episode'])
    worst = 0.0
    for b in range(k):
        n = int(steps[b])
        assert (episode[b, :n] == 0).all() and (episode[b, n:] == -1).all()
        worst = max(worst, float(np.abs(reward[b, :n] - g['ep_rewards'][b, :n]).max()))
    print('rewards: largest difference %.3e' % worst)
    assert worst <= 1e-6


# ------------------------------------------------------------------------------------- capture
@contextlib.contextmanager
def _environ(**values):
    old = {k: os.environ.get(k) for k in values}
    os.environ.update({k: str(v) for k, v in values.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def test_a_captured_call_replays_to_the_bits_of_the_eager_call(amd):
    import torch
    c = CASES['ragged_two_episode_ends']
    B, H, T = c['B'], c['H'], c['T']
    table = torch.from_numpy(_table(B, T)).cuda()
    with _environ(CROWDNAV_AMD_LAGGED_FILL=0):  # no side-stream branch beside the launch (read when the engine is built)
        eng = _engine(amd, B, H, **c['cfg'])
    bufs = eng.rollout_begin(**BEGIN)
    eng.rollout_actions(table)
    eager = _after(eng, bufs)
    assert eng.launch_counts()['lagged_fills'] == 0
    bufs = eng.rollout_begin(**BEGIN)
    eng.sync()
    graph = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(graph):
            eng.use_current_stream()  # the capturing stream
            eng.rollout_actions(table)
    finally:
        eng.use_current_stream()
    bufs = eng.rollout_begin(**BEGIN)  # capturing ran nothing; a freshly begun rollout
    eng.sync()
    assert int(_np(bufs['transitions'])[0]) == 0
    graph.replay()
    torch.cuda.synchronize()
    _same(_after(eng, bufs), eager)
