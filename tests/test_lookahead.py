"""cn_lookahead_actions on the MI355X: K candidate action sequences per env scored in one launch, against the futures the
existing entry points produce from the same state — cn_step loops (with set_state / set_theta where a state has to be put
back), cn_step(update=0) for the one-step form, rollout_step on a twin engine for "nothing moved" — bit for bit.  The
reference is never the code under test.

"A call before set_gamma" (test_refusals_on_an_engine): an engine has a discount table from cn_create on (gamma = 0.9), so
such a call is treated exactly as cn_rollout_begin treats it — accepted, scored with 0.9 — and that is what is asserted."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from support import (  # noqa: F401  (amd: module fixture)
    action_space as _space, action_table, amd, assert_branch as _assert_branch, external_engine as _engine, np_of as _np,
    restore as _restore, snapshot as _snapshot, step_loop as _step_loop)

pytestmark = pytest.mark.gpu

BEGIN = dict(seed_base=1000, seed_mod=500, record_capacity=8)


def _table(B, K, n, unicycle=False, seed=11):
    return action_table(B, K, n, unicycle=unicycle, seed=seed)


def test_the_predicted_future_is_the_one_that_happens(amd):
    B, H, K, n = 3, 5, 3, 40
    eng = _engine(amd, B, H, time_limit=8.0)  # 32-step episodes: every branch has ended inside the 40 actions
    eng.reset(np.array([1000, 1001, 1002]))
    warm = _table(B, 1, 4, seed=3)[:, 0]
    for t in range(4):
        eng.step(warm[:, t], update=True, want_obs=False)
    table = _table(B, K, n)
    look = {k: _np(v) for k, v in eng.lookahead(table, final_state=True).items()}
    assert look['ret'].shape == (B, K) and look['final_state8'].shape == (B, K, H + 1, 8)
    assert look['info'].dtype == np.uint8 and look['steps'].dtype == np.int32
    want = _step_loop(eng, table[:, 0])  # no set_state in between: the real engine, candidate 0's actions
    print('lookahead steps', look['steps'].tolist(), 'info', look['info'].tolist(), 'step loop', want['steps'].tolist())
    _assert_branch(look, 0, want)
    assert (look['steps'] >= 1).all() and (look['steps'] < n).all() and (look['info'] >= amd.REACH_GOAL).all()


def _every_candidate_and_nothing_moved(amd, B, H, K, n, cfg, unicycle=False, advance=5, after=30):
    """Engine Y: a begun rollout, `advance` bookkept steps, ONE lookahead, `after` more steps.  Twin X: the same without the
    lookahead.  Z: the snapshot put back per candidate and stepped by cn_step."""
    import torch
    table = _table(B, K, n, unicycle)
    table[:, 0, :] = (1.0, 0.0) if unicycle else (0.0, 1.0)  # candidate 0: full speed straight on, from (0, -4) towards (0, 4)
    drive = torch.from_numpy(_table(B, 1, advance + after, unicycle, seed=5)[:, 0]).cuda()
    y, x = _engine(amd, B, H, **cfg), _engine(amd, B, H, **cfg)
    ybufs, xbufs = y.rollout_begin(**BEGIN), x.rollout_begin(**BEGIN)
    for t in range(advance):
        y.rollout_step(drive[:, t].contiguous())
        x.rollout_step(drive[:, t].contiguous())
    snap = _snapshot(y)
    io_before = {k: v.clone() for k, v in ybufs.items()}
    counts_before = y.launch_counts()
    look = y.lookahead(table, final_state=True)
    y.sync()
    # nothing moved: state, heading, the rollout's io tensors, the launch counters
    for a, b in zip(snap, _snapshot(y)):
        assert torch.equal(a, b)
    for k, v in io_before.items():
        assert torch.equal(v, ybufs[k]), k
    assert y.launch_counts() == counts_before
    # ... and the rollout goes on as on the twin that never called it
    for t in range(advance, advance + after):
        y.rollout_step(drive[:, t].contiguous())
        x.rollout_step(drive[:, t].contiguous())
    for a, b in zip(_snapshot(y), _snapshot(x)):
        assert torch.equal(a, b)
    for k, v in xbufs.items():
        assert torch.equal(v, ybufs[k]), k
    assert y.launch_counts() == x.launch_counts()
    # every candidate against the step loop from the snapshot
    look = {k: _np(v) for k, v in look.items()}
    z = _engine(amd, B, H, **cfg)
    wants = []
    for k in range(K):
        _restore(z, snap)
        wants.append(_step_loop(z, table[:, k]))
        _assert_branch(look, k, wants[-1], cfg)
    return y, snap, look, wants


def test_every_candidate_and_nothing_moved(amd):
    _, _, look, wants = _every_candidate_and_nothing_moved(amd, 3, 5, 3, 40, dict(time_limit=8.0))
    print('steps', look['steps'].tolist(), 'info', look['info'].tolist())
    assert not np.array_equal(wants[0]['final_state8'], wants[1]['final_state8'])  # the candidates are different futures


def _standing(x, y, radius=0.3, v_pref=1.0):
    return [x, y, 0.0, 0.0, x, y, radius, v_pref]  # at its goal: ORCA's preferred velocity is zero


def _crafted(H):
    """Four envs, state8 [4, H + 1, 8] and global_time: a robot 0.2 below its goal; a robot 0.1 clear of a human above it;
    a robot far from everybody 1.5 s before the time limit's last second; the same with time to spare."""
    far = [_standing(8.0 + i, -8.0) for i in range(H)]
    state = np.array([
        [[0.0, 3.8, 0.0, 0.0, 0.0, 4.0, 0.3, 1.0]] + far,
        [[0.0, 0.0, 0.0, 0.0, 0.0, 4.0, 0.3, 1.0], _standing(0.0, 0.7)] + far[1:],
        [[-6.0, -6.0, 0.0, 0.0, 6.0, 6.0, 0.3, 1.0]] + far,
        [[-6.0, -6.0, 0.0, 0.0, 6.0, 6.0, 0.3, 1.0]] + far], dtype=np.float64)
    return state, np.array([1.0, 2.0, 23.5, 3.0])


def test_all_endings_occur(amd):
    """Crafted states (invisible holonomic robot, humans standing at their goals): env 0 a step from its goal, env 1 heading
    into a human, env 2 within two steps of the time limit, env 3 standing still far from everybody."""
    B, H, K, n = 4, 5, 2, 6
    eng = _engine(amd, B, H)
    state, gtime = _crafted(H)
    table = np.zeros((B, K, n, 2))
    table[0, 0, :], table[1, 0, :] = (0.0, 1.0), (0.0, 1.0)  # candidate 0: to the goal; into the human; standing; standing
    table[:, 1] = _table(B, 1, n, seed=2)[:, 0]               # candidate 1: random actions from the same states
    eng.set_state(state, gtime)
    snap = _snapshot(eng)
    look = {k: _np(v) for k, v in eng.lookahead(table, final_state=True).items()}
    wants = []
    for k in range(K):
        _restore(eng, snap)
        wants.append(_step_loop(eng, table[:, k]))
    w0 = wants[0]
    print('reference: info', [w['info'].tolist() for w in wants], 'steps', [w['steps'].tolist() for w in wants])
    # the REFERENCE produced each ending
    assert w0['info'][0] == amd.REACH_GOAL and w0['steps'][0] == 1
    assert w0['info'][1] == amd.COLLISION and w0['steps'][1] < n
    assert w0['info'][2] == amd.TIMEOUT and w0['steps'][2] == 3 and w0['time'][2] == 24.25
    assert w0['info'][3] in (amd.NOTHING, amd.DANGER) and w0['steps'][3] == n
    for k in range(K):
        _assert_branch(look, k, wants[k])


# discomfort_dist = 0.5 m (the scenario generators keep that distance too; `mixed` keeps its default): with candidate 0
# walking straight at the goal through the crowd, the returns and endings compared are not all zero and "still running"
NEAR = dict(discomfort_dist=0.5)
GEOMETRIES = {
    'one_human': dict(B=3, H=1, K=3, n=40, cfg=dict(NEAR)),
    # 10 half-planes and the kd bookkeeping; random scenes have no exact distance ties, so the order set_state cannot
    # put back decides nothing in the reference
    'twelve_humans_kd': dict(B=2, H=12, K=3, n=24, cfg=dict()),  # (twelve fit the circle at the default distance only)
    'unicycle': dict(B=3, H=5, K=3, n=40, cfg=dict(NEAR, robot_kinematics=1, time_limit=8.0), unicycle=True),
    'mixed_rule': dict(B=4, H=5, K=3, n=40, cfg=dict(scenario_rule=2)),
    'visible_robot': dict(B=3, H=5, K=3, n=40, cfg=dict(NEAR, robot_visible=1, time_limit=8.0)),
    'one_candidate': dict(B=3, H=5, K=1, n=40, cfg=dict(NEAR)),
    'one_step': dict(B=3, H=5, K=3, n=1, cfg=dict(NEAR)),
}


@pytest.mark.parametrize('case', sorted(GEOMETRIES))
def test_geometries(amd, case):
    c = GEOMETRIES[case]
    y, snap, look, wants = _every_candidate_and_nothing_moved(amd, c['B'], c['H'], c['K'], c['n'], c['cfg'],
                                                              c.get('unicycle', False), after=10)
    print(case, 'steps', look['steps'].tolist(), 'info', look['info'].tolist(), 'ret', look['ret'].tolist())
    # ... and the case is what it claims to be
    if case == 'unicycle':
        assert (look['final_theta'] != _np(snap[2])[:, None]).any()  # the heading was carried
    if case == 'mixed_rule':
        _restore(y, snap)
        assert (_np(y.human_count()) < 5).any(), _np(y.human_count())


def test_one_step_of_every_action_is_onestep_lookahead(amd):
    import torch
    B, H = 4, 5
    eng = _engine(amd, B, H, robot_visible=1)
    eng.set_state(*_crafted(H))  # (states where the 81 actions lead to different rewards and codes)
    acts = _space()
    table = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(acts[None, :, None, :], (B, 81, 1, 2)))).cuda()
    look = {k: _np(v) for k, v in eng.lookahead(table).items()}
    assert sorted(look) == ['info', 'ret', 'steps', 'time']
    for a in range(81):
        out = eng.step(np.broadcast_to(acts[a], (B, 2)).copy(), update=False, want_obs=False)
        assert np.array_equal(look['ret'][:, a].view(np.uint64), _np(out['reward']).view(np.uint64)), a  # gamma ** 0 == 1
        assert np.array_equal(look['info'][:, a], _np(out['info'])), a
    assert (look['steps'] == 1).all()
    assert {amd.NOTHING, amd.DANGER, amd.REACH_GOAL, amd.COLLISION} <= set(look['info'].ravel().tolist())


def test_refusals_on_an_engine(amd):
    import torch
    from crowdnav_amd import _lib
    B, H, K, n = 3, 5, 2, 5
    table = torch.from_numpy(_table(B, K, n)).cuda()
    orca = amd.BatchedCrowdSim(num_envs=B, num_humans=H, robot_policy=amd.ROBOT_ORCA)
    with pytest.raises(_lib.CrowdNavAmdError) as ei:
        orca.lookahead(table)
    assert ei.value.status == _lib.CN_ERR_INVALID and 'CN_ROBOT_EXTERNAL' in str(ei.value)
    # Before set_gamma.  cn_create installs the table of gamma = 0.9, so an engine is never without one and
    # cn_rollout_begin refuses nobody for it: the lookahead does as cn_rollout_begin does and scores with 0.9.  (The
    # refusal in the entry point guards an engine whose cn_set_gamma failed half way.)  A table set later is the one used.
    eng = _engine(amd, B, H)
    eng.reset(np.array([1000, 1001, 1002]))
    snap = _snapshot(eng)
    eng.rollout_begin(**BEGIN)  # accepted without set_gamma, too
    _restore(eng, snap)
    default = {k: _np(v) for k, v in eng.lookahead(table).items()}
    eng.set_gamma(0.5)
    half = {k: _np(v) for k, v in eng.lookahead(table).items()}
    for k in range(K):
        _restore(eng, snap)
        _assert_branch(default, k, _step_loop(eng, _np(table)[:, k], gamma=0.9))
        _restore(eng, snap)
        _assert_branch(half, k, _step_loop(eng, _np(table)[:, k], gamma=0.5))
    # n = 0: nothing launched, nothing written
    _restore(eng, snap)
    out = dict(ret=torch.full((B, K), 7.5, dtype=torch.float64), info=torch.full((B, K), 9, dtype=torch.uint8),
               steps=torch.full((B, K), -3, dtype=torch.int32), time=torch.full((B, K), 2.5, dtype=torch.float64),
               final_state8=torch.full((B, K, H + 1, 8), 1.5, dtype=torch.float64),
               final_theta=torch.full((B, K), 0.5, dtype=torch.float64))
    out = {k: v.cuda() for k, v in out.items()}
    keep = {k: v.clone() for k, v in out.items()}
    got = eng.lookahead(table[:, :, :0].contiguous(), final_state=True, out=out)
    eng.sync()
    for k, v in keep.items():
        assert got[k] is out[k] and torch.equal(v, out[k]), k
    # `out` is reused, and validated
    again = eng.lookahead(table, final_state=True, out=out)
    eng.sync()
    assert again['ret'] is out['ret'] and np.array_equal(_np(out['ret']), half['ret'])
    with pytest.raises(ValueError, match='out'):
        eng.lookahead(table, out=dict(out, steps=out['steps'].to(torch.int64)))


def test_the_gym_surface(amd):
    import crowdnav_amd.compat as c
    cfg = c.default_env_config()
    env = c.CrowdSim()
    env.configure(cfg)
    robot = c.Robot(cfg, 'robot')
    robot.kinematics = 'holonomic'
    env.set_robot(robot)
    K, n = 3, 40
    rows = _table(1, K, n, seed=4)[0]
    rows[0, :] = (0.0, 1.0)  # candidate 0 walks straight at its goal, through the crowd: 8 m in 32 steps
    sequences = [[c.ActionXY(float(vx), float(vy)) for vx, vy in seq] for seq in rows]
    env.reset('test', 0)
    got = env.lookahead(sequences)
    assert len(got) == K
    for k in range(K):
        env.reset('test', 0)
        ret, steps, info = 0.0, 0, None
        for t, action in enumerate(sequences[k]):
            _, reward, done, info = env.step(action)
            ret = ret + math.pow(0.9, t * env.time_step * robot.v_pref) * reward
            steps = t + 1
            if done:
                break
        print('gym candidate', k, got[k], (ret, info, steps))
        assert got[k][0] == ret and type(got[k][1]) is type(info) and got[k][2] == steps
    env.reset('test', 0)
    with pytest.raises(TypeError):
        env.lookahead([[c.ActionRot(1.0, 0.0)]])
    with pytest.raises(ValueError):
        env.lookahead([sequences[0], sequences[1][:-1]])


def test_the_example_runs(amd):
    done = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'shooting_planner.py'), '--cases', '4', '--candidates', '8',
                           '--horizon', '6'], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    text = done.stdout.decode()
    assert done.returncode == 0, text
    assert 'TEST  has success rate:' in text and 'total reward:' in text, text
