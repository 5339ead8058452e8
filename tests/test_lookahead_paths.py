"""cn_lookahead_paths and what is built on it, on the MI355X: the lookahead whose humans take the velocities the caller predicts.

(a) Constant velocity as a special case: the table that repeats the state velocity gives lookahead() under 'constant_velocity'.
(b) Replay of ORCA: the velocities recorded from humans that do not see the robot give lookahead() under 'orca'.
(c) Turning humans: every branch against the host restatement (lookahead_paths_reference.py), bit for bit.
(d) A branch that ends at step s; rows behind the ends; prefixes in K, B and n.
(e) Nothing of the engine moves.   (f) The bootstrap.   (g) The planners.   (h) The gym surface and the example.

Shapes: B = 3; 1, 5 and 12 humans, the `mixed` rule, a unicycle robot; K = 5 and K = 70 (two workgroups per env, the second
with a 6-lane tail); n = 1, 4 and 33."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

from lookahead_cv_reference import cfg_of as _cfg_of
import lookahead_paths_reference as ref
from support import (  # noqa: F401  (amd: module fixture)
    action_table as _table, amd, external_engine as _engine, np_of as _np, same_bits as _same_bits, sarl_engine as _sarl_engine,
    smoothed_plan as _plan, snapshot as _snapshot)

pytestmark = pytest.mark.gpu

BEGIN = dict(seed_base=1000, seed_mod=500, record_capacity=8)
DT, V_PREF, GAMMA = 0.25, 1.0, 0.9
CV, ORCA = 'constant_velocity', 'orca'
KEYS = ('ret', 'info', 'steps', 'time', 'final_state8', 'final_theta')
SHAPES = [(5, 1), (5, 4), (5, 33), (70, 1), (70, 4), (70, 33)]
UNROUNDABLE = 0.3 + 2.0 ** -40  # a velocity float32 cannot hold


def _paths(eng, table, vel, **kw):
    return {k: _np(v) for k, v in eng.lookahead_paths(table, vel, **kw).items()}


def _look(eng, table, model, **kw):
    """lookahead() under `model`; the engine's setting is put back."""
    was = eng.lookahead_human_model
    eng.set_lookahead_human_model(model)
    out = {k: _np(v) for k, v in eng.lookahead(table, **kw).items()}
    eng.set_lookahead_human_model(was)
    return out


CASES = {'h1': dict(H=1, cfg=dict(discomfort_dist=0.5)), 'h5': dict(H=5, cfg=dict(discomfort_dist=0.5)), 'h12': dict(H=12, cfg=dict()),
         'h5_mixed': dict(H=5, cfg=dict(scenario_rule=2)), 'h5_unicycle': dict(H=5, cfg=dict(discomfort_dist=0.5, robot_kinematics=1))}


def _moving_engine(amd, case, B=3, near_goal=False, **more):
    """A seeded reset and 3 real steps straight on: the humans move.  Then the last env gets a start time 2 s before the time
    limit's last second (its branches time out at their ninth step), and with near_goal the robot's goal is put 1.0 ahead."""
    c = CASES[case]
    eng = _engine(amd, B, c['H'], **dict(c['cfg'], **more))
    eng.reset(1000 + np.arange(B))
    straight_on = [1.0, 0.0] if case.endswith('unicycle') else [0.0, 1.0]
    for _ in range(3):
        eng.step(np.tile(straight_on, (B, 1)), update=True, want_obs=False)
    state, gtime = (_np(x).copy() for x in eng.get_state())
    gtime[B - 1] = eng.config['time_limit'] - 1.0 - 2.0
    if near_goal:
        state[:, 0, 4:6] = state[:, 0, 0:2] + np.array([0.0, 1.0])
    eng.set_state(state, gtime)
    return eng, state, gtime


# ------------------------------------------------------------------------------------------------ (a) constant velocity
@pytest.mark.parametrize('K,n', SHAPES)
@pytest.mark.parametrize('case', sorted(CASES))
def test_constant_velocity_is_a_special_case(amd, case, K, n):
    from crowdnav_amd import predict
    eng, state, gtime = _moving_engine(amd, case)
    B, unicycle = len(state), case.endswith('unicycle')
    if case == 'h5_mixed':
        parked = state[:, 1:, 0] >= 1.0e5
        assert (_np(eng.human_count()) < 5).any() and parked.any()  # parked placeholders take part ...
        assert (state[:, 1:, 2:4][parked] == 0.0).all()             # ... with the zeros the caller is asked to write
    state[0, 1, 2] = UNROUNDABLE
    eng.set_state(state, gtime)
    table = _table(B, K, n, unicycle=unicycle)
    vel = predict.constant_velocity(state, n)
    assert vel.shape == (B, n, CASES[case]['H'], 2) and vel[0, :, 0, 0].tolist() == [UNROUNDABLE] * n
    want = _look(eng, table, CV, final_state=True)
    for model in (ORCA, CV):  # the engine's setting is neither read nor written
        eng.set_lookahead_human_model(model)
        got = _paths(eng, table, vel, final_state=True)
        assert eng.lookahead_human_model == model
        for key in KEYS:
            assert _same_bits(got[key], want[key]), (case, K, n, model, key)
    if (K, n) == (70, 33):
        ended = want['info'] >= amd.REACH_GOAL
        print(case, 'ended', int(ended.sum()), 'of', ended.size, 'collisions', int((want['info'] == amd.COLLISION).sum()))
        assert ended.any() and not ended.all()
    if unicycle:
        assert (want['final_theta'] != _np(eng.get_theta())[:, None]).any()  # the heading was carried


# ------------------------------------------------------------------------------------------------ (b) replay of ORCA
def _replay_scene(state):
    """The robot 1.0 ahead of human 1 on that human's way to its goal, its own goal 1.5 to the side: straight to the goal is
    ReachGoal at the fifth step, standing still is run over (the humans do not see the robot), walking ahead of human 1 — at
    its speed or a little slower — runs on."""
    placed = state.copy()
    B, K, n = len(state), 9, 10
    table = _table(B, K, n, seed=7)
    for b in range(B):
        human = state[b, 1]
        d = (human[4:6] - human[0:2]) / np.hypot(*(human[4:6] - human[0:2]))
        side = np.array([-d[1], d[0]])
        at = human[0:2] + d * 1.0
        placed[b, 0, 0:2], placed[b, 0, 2:4], placed[b, 0, 4:6] = at, 0.0, at + side * 1.5
        table[b, 0], table[b, 1], table[b, 2], table[b, 3] = side, 0.0, d, 0.9 * d
    return placed, table


_REPLAY = {}


def _replay(amd, H):
    """(want, got, vel) of the replay at H humans, computed once: lookahead() under 'orca' on an engine whose humans do not see
    the robot, and lookahead_paths() on the same engine with the velocities recorded from a twin."""
    if H in _REPLAY:
        return _REPLAY[H]
    B, K, n = 3, 9, 10
    eng, twin = (_engine(amd, B, H, robot_visible=0) for _ in range(2))
    for e in (eng, twin):
        e.reset(1000 + np.arange(B))
        for _ in range(4):
            e.step(np.tile([0.0, 1.0], (B, 1)), update=True, want_obs=False)
    state, gtime = (_np(x).copy() for x in eng.get_state())
    assert _same_bits(_np(twin.get_state()[0]), state)
    placed, table = _replay_scene(state)
    eng.set_state(placed, gtime)
    # the twin: the same humans, the robot parked far from the crowd; the velocity a human has after step t is the one it took
    far = state.copy()
    far[:, 0, 0:2], far[:, 0, 2:4], far[:, 0, 4:6] = (50.0, 50.0), 0.0, (50.0, 60.0)
    twin.set_state(far, gtime)
    vel = np.zeros((B, n, H, 2))
    for t in range(n):
        twin.step(np.zeros((B, 2)), update=True, want_obs=False)
        vel[:, t] = _np(twin.get_state()[0])[:, 1:, 2:4]
    want = _look(eng, table, ORCA, final_state=True)
    got = _paths(eng, table, vel, final_state=True)
    _REPLAY[H] = (want, got, vel)
    return _REPLAY[H]


def _replay_preconditions(amd, want, vel, n=10):
    # all three outcomes, on the ORCA result
    assert (want['info'] == amd.COLLISION).any() and (want['info'] == amd.REACH_GOAL).any()
    ran_on = (want['steps'] == n) & (want['info'] < amd.REACH_GOAL)
    assert ran_on.any() and (want['steps'][want['info'] >= amd.REACH_GOAL] < n).any()
    # the precondition, asserted: the humans' motion does not depend on the branch — every branch of an env that made all n
    # steps leaves the same human rows
    pairs = 0
    for b in range(len(want['steps'])):
        full = np.flatnonzero(want['steps'][b] == n)
        for k in full[1:]:
            assert _same_bits(want['final_state8'][b, k, 1:], want['final_state8'][b, full[0], 1:]), (b, k)
            pairs += 1
    assert pairs >= 1
    assert (vel[:, 1:] != vel[:, :-1]).any()  # the humans turn: not the constant-velocity case


@pytest.mark.parametrize('H', [1, 5, 12])
def test_replay_of_orca(amd, H):
    """With the velocities recorded from humans that do not see the robot, lookahead_paths equals lookahead() under 'orca' bit
    for bit on every output of all K = 9 branches: the recorded table is the humans' policy, and the transition around it is
    step_core's — the swept test of step t with the velocity a human has when the step starts, the move with the one it chooses."""
    want, got, vel = _replay(amd, H)
    print('replay H', H, 'info', want['info'].tolist(), 'steps', want['steps'].tolist())
    _replay_preconditions(amd, want, vel)
    for key in KEYS:  # the figures, before the assertions
        differ = got[key] != want[key]
        print('replay H', H, key, 'entries that differ:', int(differ.sum()), 'of', differ.size,
              '' if key != 'ret' else 'max |difference| %.3g' % np.abs(got[key] - want[key]).max())
    for key in KEYS:
        assert _same_bits(got[key], want[key]), (H, key, got[key], want[key])


@pytest.mark.parametrize('H', [1, 5, 12])
def test_replay_of_orca_moves_the_humans_as_orca_does(amd, H):
    """The replay moves the humans as ORCA does: every branch leaves every human, and the robot, where its ORCA twin leaves
    them, with the velocity ORCA left them (a narrower statement than test_replay_of_orca's, kept because it names what a
    failure of that one would be about: the humans' motion or the robot's outcome)."""
    want, got, vel = _replay(amd, H)
    _replay_preconditions(amd, want, vel)
    alike = got['steps'] == want['steps']
    print('replay H', H, 'branches with the same number of steps:', int(alike.sum()), 'of', alike.size)
    assert alike.sum() >= alike.size // 2 and (want['steps'][alike] == 10).any() and (want['steps'][alike] < 10).any()
    assert _same_bits(got['final_state8'][alike][:, 1:], want['final_state8'][alike][:, 1:])
    assert _same_bits(got['time'][alike], want['time'][alike]) and _same_bits(got['final_theta'], want['final_theta'])
    assert _same_bits(got['final_state8'][alike][:, 0], want['final_state8'][alike][:, 0])  # and the robot, moved by the same rows


# ------------------------------------------------------------------------------------------------ (c) turning humans
def _turning(state, n, seed=5):
    """[B, n, H, 2]: every human starts from its own velocity and turns a little every step (a random walk of the velocity);
    human 1 of env 0 takes a velocity no float32 holds at step 0."""
    B, H = len(state), state.shape[1] - 1
    walk = np.cumsum(np.random.RandomState(seed).normal(0.0, 0.15, (B, 33, H, 2)), axis=1)[:, :n]  # (a prefix in n)
    vel = np.ascontiguousarray(state[:, None, 1:, 2:4] + walk)
    vel[0, 0, 0, 0] = UNROUNDABLE
    assert float(np.float32(UNROUNDABLE)) != UNROUNDABLE
    return vel


def _turning_table(B, K, n):
    table = _table(B, K, n)
    table[:, 0] = (0.0, 1.0)  # candidate 0 walks to the goal 1.0 ahead
    return table


_REFERENCE = {}


def _reference(case, state, gtime, cfg, K, n):
    """The restatement's branches of (case, K, n), computed once and shared."""
    key = (case, K, n)
    if key not in _REFERENCE:
        _REFERENCE[key] = (state.copy(), ref.lookahead(state, gtime, _turning_table(len(state), K, n), _turning(state, n), cfg, GAMMA))
    assert np.array_equal(_REFERENCE[key][0], state)  # (the device state the reference was made for is reproduced)
    return _REFERENCE[key][1]


def _outcomes(want, n):
    count = {name: int((want['info'] == code).sum()) for name, code in (('collision', ref.COLLISION), ('reach_goal', ref.REACH_GOAL),
                                                                       ('timeout', ref.TIMEOUT))}
    count['danger_and_on'] = sum(ref.DANGER in infos[:-1] for row in want['infos'] for infos in row)
    count['ran_on'] = int(((want['steps'] == n) & (want['info'] < ref.REACH_GOAL)).sum())
    return count


def test_the_turning_cases_contain_every_outcome(amd):
    """On the restatement's own output: the K = 70, n = 33 cases below contain branches that end in Collision, ReachGoal and
    Timeout, branches that pass a Danger step and go on, and branches that run all n steps."""
    total = {}
    for case in ('h1', 'h12', 'h5'):
        eng, state, gtime = _moving_engine(amd, case, near_goal=True)
        count = _outcomes(_reference(case, state, gtime, _cfg_of(eng), 70, 33), 33)
        print(case, count)
        assert count['reach_goal'] >= 1 and count['ran_on'] >= 1, (case, count)
        total = {k: total.get(k, 0) + v for k, v in count.items()}
    assert all(v >= 1 for v in total.values()), total


@pytest.mark.parametrize('K,n', SHAPES)
@pytest.mark.parametrize('case', ['h1', 'h12', 'h5'])
def test_turning_humans_against_the_restatement(amd, case, K, n):
    eng, state, gtime = _moving_engine(amd, case, near_goal=True)
    B = len(state)
    want = _reference(case, state, gtime, _cfg_of(eng), K, n)
    got = _paths(eng, _turning_table(B, K, n), _turning(state, n), final_state=True)
    for key in ('ret', 'info', 'steps', 'time', 'final_state8'):
        assert _same_bits(got[key], want[key]), (case, K, n, key, got[key], want[key])
    assert _same_bits(got['final_theta'], np.broadcast_to(_np(eng.get_theta())[:, None], (B, K)).copy())
    first = got['steps'][0] == 1  # a branch of env 0 that made one step holds step 0's velocity, unrounded
    assert got['final_state8'][0, first, 1, 2].tolist() == [UNROUNDABLE] * int(first.sum()) and (n > 1 or first.all())


# ------------------------------------------------------------------------------------------------ (d) ends, holes, prefixes
def test_a_branch_that_ends_at_step_s(amd):
    B, K, n = 3, 70, 33
    eng, state, _ = _moving_engine(amd, 'h5', near_goal=True)
    table, vel = _turning_table(B, K, n), _turning(state, n)
    full = _paths(eng, table, vel, final_state=True)
    ended = full['info'] >= amd.REACH_GOAL
    # where the humans are after every step: p <- p + v dt, one multiply and one add, sequential
    after = np.zeros((B, n, 5, 2))
    p = state[:, 1:, 0:2].copy()
    for t in range(n):
        p = p + vel[:, t] * DT
        after[:, t] = p
    checked = 0
    for b in range(B):
        for k in np.flatnonzero(ended[b, :64]):  # a lane of the env's first wave whose branch ended at step s ...
            s = int(full['steps'][b, k]) - 1
            if not (full['steps'][b, :64] >= s + 4).any():  # ... while another lane of that wave runs on for 3 more steps or longer
                continue
            assert _same_bits(full['final_state8'][b, k, 1:, 2:4], vel[b, s]), (b, k, s)
            assert _same_bits(full['final_state8'][b, k, 1:, 0:2], after[b, s]), (b, k, s)
            assert _same_bits(full['final_state8'][b, k, 1:, 4:8], state[b, 1:, 4:8]), (b, k, s)
            checked += 1
    print('branches that ended under a running wave:', checked)
    assert checked >= 3
    for b in range(B):  # and those that made all n steps: the last row
        for k in np.flatnonzero(full['steps'][b] == n):
            assert _same_bits(full['final_state8'][b, k, 1:, 2:4], vel[b, n - 1]) and _same_bits(full['final_state8'][b, k, 1:, 0:2], after[b, n - 1])
    # NaN rows behind every branch's end change nothing: action rows behind the branch's own end, velocity rows behind the
    # end of the env's longest branch
    holes, vholes = table.copy(), vel.copy()
    holes[np.arange(n)[None, None, :] >= full['steps'][:, :, None]] = np.nan
    vholes[np.arange(n)[None, :] >= full['steps'].max(axis=1)[:, None]] = np.nan
    assert np.isnan(holes).any() and np.isnan(vholes).any()
    again = _paths(eng, holes, vholes, final_state=True)
    for key in KEYS:
        assert _same_bits(again[key], full[key]), key
    # prefixes.  K: the first 5 candidates alone
    few = _paths(eng, table[:, :5].copy(), vel, final_state=True)
    for key in KEYS:
        assert _same_bits(few[key], full[key][:, :5]), key
    # B: the first two envs alone, on an engine of two
    two = _engine(amd, 2, 5, discomfort_dist=0.5)
    two.set_state(*(_np(x)[:2].copy() for x in eng.get_state()))
    two.set_theta(_np(eng.get_theta())[:2].copy())
    pair = _paths(two, table[:2].copy(), vel[:2].copy(), final_state=True)
    for key in KEYS:
        assert _same_bits(pair[key], full[key][:2]), key
    # n: a branch that ended inside the first 4 steps is the same branch in the n = 4 call; one still running has made 4 steps
    four = _paths(eng, table[:, :, :4].copy(), vel[:, :4].copy(), final_state=True)
    inside = ended & (full['steps'] <= 4)
    assert inside.any() and not inside.all()
    for key in KEYS:
        assert _same_bits(four[key][inside], full[key][inside]), key
    assert (four['steps'][~inside] == 4).all() and _same_bits(four['final_state8'][~inside][:, 1:, 2:4],
                                                               np.broadcast_to(vel[:, None, 3], (B, K, 5, 2))[~inside])


# ------------------------------------------------------------------------------------------------ (e) nothing moved
def test_the_engine_is_untouched(amd):
    import torch
    B, K, n = 3, 5, 12
    table = _table(B, K, n)
    drive = torch.from_numpy(_table(B, 1, 15, seed=5)[:, 0]).cuda()
    y, x = (_engine(amd, B, 5, discomfort_dist=0.5) for _ in range(2))
    ybufs, xbufs = y.rollout_begin(**BEGIN), x.rollout_begin(**BEGIN)
    for t in range(5):
        y.rollout_step(drive[:, t].contiguous())
        x.rollout_step(drive[:, t].contiguous())
    y.set_lookahead_human_model(CV)
    snap, io_before, counts = _snapshot(y), {k: v.clone() for k, v in ybufs.items()}, y.launch_counts()
    vel = _turning(_np(snap[0]), n)
    first = _paths(y, table, vel, final_state=True)
    y.sync()
    for a, b in zip(snap, _snapshot(y)):
        assert torch.equal(a, b)
    for k, v in io_before.items():
        assert torch.equal(v, ybufs[k]), k
    assert y.launch_counts() == counts and y.lookahead_human_model == CV
    assert (first['steps'] >= 1).all()
    # ... and the rollout goes on as on the twin that never looked ahead (scenario ring levels included: the episodes that end
    # in the next steps take the same scenarios)
    for t in range(5, 15):
        y.rollout_step(drive[:, t].contiguous())
        x.rollout_step(drive[:, t].contiguous())
        y.lookahead_paths(table, vel)
    for a, b in zip(_snapshot(y), _snapshot(x)):
        assert torch.equal(a, b)
    for k, v in xbufs.items():
        assert torch.equal(v, ybufs[k]), k
    assert y.launch_counts() == x.launch_counts() and y.lookahead_human_model == CV and x.lookahead_human_model == ORCA


def test_n_zero_is_a_no_op(amd):
    import torch
    from crowdnav_amd import _lib
    from crowdnav_amd.engine import _struct
    B, K, H = 3, 4, 5
    eng = _engine(amd, B, H)
    eng.reset(1000 + np.arange(B))
    out = dict(ret=torch.full((B, K), 7.5, dtype=torch.float64), info=torch.full((B, K), 9, dtype=torch.uint8),
               steps=torch.full((B, K), -3, dtype=torch.int32), time=torch.full((B, K), 2.5, dtype=torch.float64),
               final_state8=torch.full((B, K, H + 1, 8), 1.5, dtype=torch.float64),
               final_theta=torch.full((B, K), 0.5, dtype=torch.float64))
    out = {k: v.cuda() for k, v in out.items()}
    keep = {k: v.clone() for k, v in out.items()}
    got = eng.lookahead_paths(torch.zeros((B, K, 0, 2), dtype=torch.float64).cuda(),
                              torch.zeros((B, 0, H, 2), dtype=torch.float64).cuda(), final_state=True, out=out)
    eng.sync()
    for k, v in keep.items():
        assert got[k] is out[k] and torch.equal(v, out[k]), k
    dummy = torch.zeros(2, dtype=torch.float64).cuda()  # (an empty tensor has no address: the C call itself)
    lo = _struct(_lib.CnLookaheadOut, out)
    assert eng._lib.cn_lookahead_paths(eng._h, 0, K, dummy.data_ptr(), dummy.data_ptr(), C.byref(lo)) == _lib.CN_OK
    eng.sync()
    for k, v in keep.items():
        assert torch.equal(v, out[k]), k
    # on a live engine: NULL human_vel first, then the lookahead's own refusals; the shapes, in Python
    assert eng._lib.cn_lookahead_paths(eng._h, -1, K, None, None, C.byref(lo)) == _lib.CN_ERR_INVALID
    assert 'cn_lookahead_paths: human_vel is NULL' in eng._lib.cn_last_error().decode()
    assert eng._lib.cn_lookahead_paths(eng._h, -1, K, dummy.data_ptr(), dummy.data_ptr(), C.byref(lo)) == _lib.CN_ERR_INVALID
    assert 'n_steps must be >= 0' in eng._lib.cn_last_error().decode()
    with pytest.raises(ValueError, match='human_vel must be'):
        eng.lookahead_paths(np.zeros((B, K, 3, 2)), np.zeros((B, 3, H + 1, 2)))
    orca = amd.BatchedCrowdSim(num_envs=B, num_humans=H, robot_policy=amd.ROBOT_ORCA)
    with pytest.raises(_lib.CrowdNavAmdError) as ei:
        orca.lookahead_paths(np.zeros((B, K, 3, 2)), np.zeros((B, 3, H, 2)))
    assert ei.value.status == _lib.CN_ERR_INVALID and 'CN_ROBOT_EXTERNAL' in str(ei.value)


# ------------------------------------------------------------------------------------------------ (f) bootstrap
def test_bootstrap(amd):
    from crowdnav_amd import predict
    B, K, n = 3, 70, 6
    eng = _sarl_engine(amd, B)
    for _ in range(3):
        eng.step(np.tile([0.0, 1.0], (B, 1)), update=True, want_obs=False)
    state, gtime = (_np(x).copy() for x in eng.get_state())
    gtime[B - 1] = eng.config['time_limit'] - 1.0 - 0.5  # the last env's branches end in Timeout at their third step
    eng.set_state(state, gtime)
    table, vel = _table(B, K, n), _turning(state, n)
    look = eng.lookahead_paths(table, vel, bootstrap=True)
    direct = _np(eng.sarl_state_values(look['final_state8']))
    look = {k: _np(v) for k, v in look.items()}
    plain = _paths(eng, table, vel, final_state=True)
    for key in KEYS:
        assert _same_bits(look[key], plain[key]), key  # the branches are cn_lookahead_paths'
    want = ref.lookahead(state, gtime, table, vel, _cfg_of(eng), GAMMA)
    assert _same_bits(look['ret'], want['ret']) and _same_bits(look['final_state8'], want['final_state8'])
    assert _same_bits(look['value'], direct.reshape(B, K))
    ended = look['info'] >= amd.REACH_GOAL
    print('bootstrap: ended', int(ended.sum()), 'of', ended.size)
    assert ended.any() and not ended.all()
    for b in range(B):
        for k in range(K):
            boot = math.pow(GAMMA, int(look['steps'][b, k]) * DT * V_PREF) * float(np.float64(look['value'][b, k]))
            score = look['ret'][b, k] if ended[b, k] else look['ret'][b, k] + boot
            assert _same_bits(look['score'][b, k], np.float64(score)), (b, k)
    # with the table of (a): lookahead(bootstrap=True) under the constant-velocity model
    same = {k: _np(v) for k, v in eng.lookahead_paths(table, predict.constant_velocity(state, n), bootstrap=True).items()}
    under_cv = _look(eng, table, CV, bootstrap=True)
    for key in KEYS + ('value', 'score'):
        assert _same_bits(same[key], under_cv[key]), key


def test_bootstrap_refusals_are_those_of_lookahead_values(amd):
    B, K, n = 2, 5, 4
    table, vel = _table(B, K, n), np.zeros((B, n, 5, 2))
    for eng, status, word in ((_engine(amd, B, 5), amd._lib.CN_ERR_INVALID, 'configure and set weights first'),
                              (_sarl_engine(amd, B, with_om=True), amd._lib.CN_ERR_UNSUPPORTED, 'occupancy maps (with_om) are not served'),
                              (_sarl_engine(amd, B, scenario_rule=2), amd._lib.CN_ERR_UNSUPPORTED, 'engines under the mixed rule are not served')):
        counts = eng.launch_counts()
        with pytest.raises(amd.CrowdNavAmdError) as ei:
            eng.lookahead_paths(table, vel, bootstrap=True)
        assert ei.value.status == status and word in str(ei.value) and 'cn_lookahead_paths_values' in str(ei.value), str(ei.value)
        plan = eng.plan_begin(K, n, 2, 1, 0.3, bootstrap=True)
        for call in (lambda: eng.plan_cem_paths(plan, vel, 0), lambda: eng.plan_mppi_paths(plan, vel, 1.0, 0)):
            with pytest.raises(amd.CrowdNavAmdError) as ei:
                call()
            assert ei.value.status == status and word in str(ei.value), str(ei.value)
        assert eng.launch_counts() == counts


# ------------------------------------------------------------------------------------------------ (g) planners
@pytest.mark.parametrize('bootstrap', [False, True])
@pytest.mark.parametrize('update', ['cem', 'mppi'])
def test_a_planning_step_is_draw_lookahead_paths_update(amd, update, bootstrap):
    import torch
    from crowdnav_amd import predict
    B, K, n, I, counter = 3, 5, 4, 3, 21
    if bootstrap:
        eng = _sarl_engine(amd, B)
        for _ in range(3):
            eng.step(np.tile([0.0, 1.0], (B, 1)), update=True, want_obs=False)
    else:
        eng, _, _ = _moving_engine(amd, 'h5')
    state, gtime = (_np(x).copy() for x in eng.get_state())
    vel = torch.from_numpy(_turning(state, n)).cuda()
    one, parts = _plan(eng, K, n, I=I, bootstrap=bootstrap), _plan(eng, K, n, I=I, bootstrap=bootstrap)
    counts = eng.launch_counts()
    if update == 'cem':
        eng.plan_cem_paths(one, vel, counter)
    else:
        eng.plan_mppi_paths(one, vel, 0.7, counter)
    if not bootstrap:
        assert eng.launch_counts() == counts  # (with bootstrap the narrow tiles' launches count, as for cn_lookahead_values)
    for i in range(I):  # the same step composed from the public calls
        eng.plan_draw(parts, counter + i)
        assert eng.lookahead_paths(parts.candidates, vel, out=parts.look, bootstrap=bootstrap)['ret'] is parts.look['ret']
        if update == 'cem':
            eng.plan_refit(parts, keep_best=i > 0)
        else:
            eng.plan_mppi_update(parts, 0.7, keep_best=i > 0)
    eng.sync()
    for k, v in parts.tensors().items():
        assert torch.equal(v, one.tensors()[k]), k
    want = ref.lookahead(state, gtime, _np(one.candidates), _np(vel), _cfg_of(eng), GAMMA)
    assert _same_bits(one.look['ret'], want['ret'])  # ... and the lookahead inside was the paths one, on the last draw
    # with the table of (a): plan_cem / plan_mppi under the constant-velocity model, on a twin plan with the same seed and counter
    paths, model = _plan(eng, K, n, I=I, bootstrap=bootstrap), _plan(eng, K, n, I=I, bootstrap=bootstrap)
    still = predict.constant_velocity(torch.from_numpy(state).cuda(), n)
    eng.set_lookahead_human_model(CV)
    if update == 'cem':
        eng.plan_cem_paths(paths, still, counter)
        eng.plan_cem(model, counter)
    else:
        eng.plan_mppi_paths(paths, still, 0.7, counter)
        eng.plan_mppi(model, 0.7, counter)
    eng.sync()
    for k, v in model.tensors().items():
        assert torch.equal(v, paths.tensors()[k]), k


def test_planner_refusals(amd):
    B, K, n = 2, 5, 4
    vel = np.zeros((B, n, 5, 2))
    for eng, status, word in ((amd.BatchedCrowdSim(num_envs=B, num_humans=5, robot_policy=amd.ROBOT_ORCA), amd._lib.CN_ERR_INVALID,
                               'CN_ROBOT_EXTERNAL'),
                              (_engine(amd, B, 5, robot_kinematics=1), amd._lib.CN_ERR_UNSUPPORTED, 'CN_UNICYCLE engines are not served')):
        eng.reset(1000 + np.arange(B))
        plan = eng.plan_begin(K, n, 2, 1, 0.3)
        counts = eng.launch_counts()
        for name, call in (('cn_plan_cem_paths', lambda: eng.plan_cem_paths(plan, vel, 0)),
                           ('cn_plan_mppi_paths', lambda: eng.plan_mppi_paths(plan, vel, 1.0, 0))):
            with pytest.raises(amd.CrowdNavAmdError) as ei:
                call()
            assert ei.value.status == status and word in str(ei.value) and name in str(ei.value), str(ei.value)
        assert eng.launch_counts() == counts
    eng = _engine(amd, B, 5)
    plan, other = eng.plan_begin(K, n, 2, 1, 0.3), _engine(amd, B, 5).plan_begin(K, n, 2, 1, 0.3)
    with pytest.raises(ValueError):
        eng.plan_cem_paths(plan, np.zeros((B, n + 1, 5, 2)), 0)  # the table's n is the plan's
    with pytest.raises(ValueError):
        eng.plan_cem_paths(plan, None, 0)
    with pytest.raises(ValueError):
        eng.plan_mppi_paths(other, vel, 1.0, 0)  # another engine's plan
    with pytest.raises(amd.CrowdNavAmdError, match='temperature'):
        eng.plan_mppi_paths(plan, vel, 0.0, 0)


# ------------------------------------------------------------------------------------------------ (h) compat and example
def test_the_gym_surface(amd):
    import crowdnav_amd.compat as c
    from crowdnav_amd import predict
    from crowdnav_amd.compat.types import info_from_code
    cfg = c.default_env_config()
    env = c.CrowdSim()
    env.configure(cfg)
    robot = c.Robot(cfg, 'robot')
    robot.kinematics = 'holonomic'
    env.set_robot(robot)
    K, n = 3, 12
    rows = _table(1, K, n, seed=4)[0]
    rows[0, :] = (0.0, 1.0)
    sequences = [[c.ActionXY(float(vx), float(vy)) for vx, vy in seq] for seq in rows]
    env.reset('test', 0)
    state, gtime = (_np(x) for x in env._eng.get_state())
    vel = predict.to_goal(state, n, env.time_step)
    was = env._eng.lookahead_human_model
    got = env.lookahead_paths(sequences, vel[0])
    assert env._eng.lookahead_human_model == was
    want = _paths(env._eng, rows[None].copy(), vel)
    restated = ref.lookahead(state, gtime, rows[None], vel, _cfg_of(env._eng), GAMMA)
    for k in range(K):
        assert len(got[k]) == 3 and got[k][0] == float(want['ret'][0, k]) == float(restated['ret'][0, k])
        assert got[k][2] == int(want['steps'][0, k]) and type(got[k][1]) is type(info_from_code(int(want['info'][0, k])))
    rows_of = lambda scored: [(r[0], type(r[1]), r[2]) for r in scored]  # noqa: E731
    assert rows_of(env.lookahead_paths(sequences, vel[0].tolist())) == rows_of(got)  # anything np.asarray reads
    with pytest.raises(ValueError):
        env.lookahead_paths(sequences, vel[0, :n - 1])
    with pytest.raises(ValueError):
        env.lookahead_paths([], vel[0])


@pytest.mark.parametrize('mode', ['cem', 'mppi'])
def test_the_example_runs(amd, mode):
    cmd = [sys.executable, os.path.join(ROOT, 'examples', 'predicted_paths_planner.py'), '--cases', '2', '--candidates', '8', '--horizon', '4',
           '--iterations', '2'] + (['--mppi'] if mode == 'mppi' else [])
    done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    text = done.stdout.decode()
    assert done.returncode == 0, text
    assert 'TEST  has success rate:' in text and 'collision rate:' in text and 'nav time:' in text, text
