"""cn_lookahead_actions under CN_HUMANS_CONSTANT_VELOCITY on the MI355X.

1. Still humans: the ORCA lookahead and the constant-velocity one are the same function there, device against device, bit for bit.
2. Moving humans: every branch against the host restatement (lookahead_cv_reference.py, written from step_core), bit for bit.
3. Invariances: prefixes in K, B and n; rows after a branch's end; the engine untouched; switching back; n = 0.
4. What inherits the model through the lookahead: the bootstrap, the CEM and MPPI planning steps, the closed loop.
5. Refusals and the Python surface.

Shapes: B = 3; 1, 5 and 12 humans and the `mixed` rule; K = 5 and K = 70 (two workgroups per env, the second with a 6-lane
tail); n = 1, 4 and 33."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import lookahead_cv_reference as ref
from lookahead_cv_reference import cfg_of as _cfg_of
from support import (  # noqa: F401  (amd: module fixture)
    action_table as _table, amd, configure_sarl, external_engine, np_of as _np, prior_plan as _plan, same_bits as _same_bits,
    snapshot as _snapshot)

pytestmark = pytest.mark.gpu

BEGIN = dict(seed_base=1000, seed_mod=500, record_capacity=8)
DT, V_PREF, GAMMA = 0.25, 1.0, 0.9
CV, ORCA = 'constant_velocity', 'orca'


def _engine(amd, B, H, model=CV, **cfg):
    eng = external_engine(amd, B, H, **cfg)
    eng.set_lookahead_human_model(model)
    return eng


def _look(eng, table, **kw):
    return {k: _np(v) for k, v in eng.lookahead(table, **kw).items()}


def _both(eng, table, **kw):
    """The same call under 'orca' and under 'constant_velocity'; the engine is left under 'constant_velocity'."""
    eng.set_lookahead_human_model(ORCA)
    orca = _look(eng, table, **kw)
    eng.set_lookahead_human_model(CV)
    return orca, _look(eng, table, **kw)


# ------------------------------------------------------------------------------------------------ 1. still humans
def _still_scene(H):
    """state8 [H + 1, 8]: robot at (0, -3) bound for (0, 3); human 1 at (0.75, 0); the others out of the way; every human at
    its own goal with zero velocity."""
    if H == 12:
        others = [(4.0 * math.cos(math.radians(15.0 + 30.0 * k)), 4.0 * math.sin(math.radians(15.0 + 30.0 * k))) for k in range(11)]
    else:
        others = [(-2.0, 1.5), (2.0, 1.0), (-1.5, -2.0), (1.75, -1.5)][:H - 1]
    rows = [[0.0, -3.0, 0.0, 0.0, 0.0, 3.0, 0.3, 1.0]]
    rows += [[x, y, 0.0, 0.0, x, y, 0.3, 1.0] for x, y in [(0.75, 0.0)] + others]
    return np.array(rows, dtype=np.float64)


def _still_sequences(n, unicycle):
    """[3, n, 2]: to the goal, into human 1, standing still."""
    seq = np.zeros((3, n, 2))
    if unicycle:  # (v, r) from heading pi / 2: straight on; one turn towards (0.75, 0) and straight on; waiting
        seq[0, :, 0] = 1.0
        seq[1, :, 0], seq[1, 0, 1] = 1.0, math.atan2(3.0, 0.75) - math.pi / 2
    else:
        seq[0, :] = (0.0, 1.0)
        seq[1, :] = np.array([0.75, 3.0]) / math.hypot(0.75, 3.0)
    return seq


@pytest.mark.parametrize('n', [40, 10])
@pytest.mark.parametrize('case', ['h1', 'h5', 'h12_kd', 'h5_unicycle'])
def test_still_humans_the_two_models_agree(amd, case, n):
    import torch
    H = {'h1': 1, 'h5': 5, 'h12_kd': 12, 'h5_unicycle': 5}[case]
    unicycle = case.endswith('unicycle')
    B, K = 3, 3
    eng = _engine(amd, B, H, robot_visible=0, time_limit=8.0, robot_kinematics=1 if unicycle else 0)
    start = np.broadcast_to(_still_scene(H), (B, H + 1, 8)).copy()
    eng.set_state(start, np.array([0.0, 0.0, 1.0]))
    eng.set_theta(np.full(B, math.pi / 2))
    table = np.broadcast_to(_still_sequences(n, unicycle), (B, K, n, 2)).copy()
    orca, cv = _both(eng, table, final_state=True)
    print(case, n, 'steps', orca['steps'].tolist(), 'info', orca['info'].tolist())
    # the precondition, asserted: under ORCA the humans did not move, so the agreement below is not vacuous
    assert np.array_equal(orca['final_state8'][:, :, 1:], np.broadcast_to(start[:, None, 1:], (B, K, H, 8)))
    for key in ('ret', 'info', 'steps', 'time'):
        assert _same_bits(cv[key], orca[key]), (key, cv[key], orca[key])
    assert torch.equal(torch.from_numpy(cv['final_state8']), torch.from_numpy(orca['final_state8']))
    assert torch.equal(torch.from_numpy(cv['final_theta']), torch.from_numpy(orca['final_theta']))
    if n == 40:  # every branch has ended, each in its own way
        assert cv['info'].tolist() == [[amd.REACH_GOAL, amd.COLLISION, amd.TIMEOUT]] * B
        if not unicycle:
            assert cv['steps'][0].tolist() == [23, 10, 29] and cv['steps'][2].tolist() == [23, 10, 25]
    else:
        assert (cv['steps'][:, [0, 2]] == n).all() and (cv['info'][:, [0, 2]] < amd.REACH_GOAL).all()
    if unicycle:
        assert (cv['final_theta'][:, 1] != math.pi / 2).all()  # the heading was carried


# ------------------------------------------------------------------------------------------------ 2. moving humans
# Seeds 1000..1002, chosen with the restatement on the CPU oracle's states: over the 3 x 70 branches of 33 steps every engine
# below has branches that end in Collision, branches that pass a Danger step and go on, and branches that run all 33 steps.
MOVING = {'h1': dict(H=1, cfg=dict(discomfort_dist=0.5)), 'h5': dict(H=5, cfg=dict(discomfort_dist=0.5)),
          'h12': dict(H=12, cfg=dict()), 'h5_mixed': dict(H=5, cfg=dict(scenario_rule=2))}
UNROUNDABLE = 0.3 + 2.0 ** -40  # a velocity float32 cannot hold


def _moving_engine(amd, case, B=3, model=CV, **more):
    """A seeded reset and 3 real steps straight on: the humans carry float32-valued ORCA velocities.  Then human 1 of env 0
    gets a velocity no float32 holds, and the last env a start time 2 s before the time limit's last second."""
    c = MOVING[case]
    eng = _engine(amd, B, c['H'], model, **dict(c['cfg'], **more))
    eng.reset(1000 + np.arange(B))
    for _ in range(3):
        eng.step(np.tile([0.0, 1.0], (B, 1)), update=True, want_obs=False)
    state, gtime = (_np(x).copy() for x in eng.get_state())
    assert (state[:, 1:, 2:4] == state[:, 1:, 2:4].astype(np.float32)).all()
    state[0, 1, 2] = UNROUNDABLE
    assert float(np.float32(UNROUNDABLE)) != UNROUNDABLE
    gtime[B - 1] = eng.config['time_limit'] - 1.0 - 2.0
    eng.set_state(state, gtime)
    return eng, state, gtime


_REFERENCE = {}


def _reference(case, state, gtime, cfg, K, n):
    """The restatement's branches of (case, K, n), computed once and shared."""
    key = (case, K, n)
    if key not in _REFERENCE:
        _REFERENCE[key] = (state.copy(), ref.lookahead(state, gtime, _table(len(state), K, n), cfg, GAMMA))
    assert np.array_equal(_REFERENCE[key][0], state)  # (the device state the reference was made for is reproduced)
    return _REFERENCE[key][1]


@pytest.mark.parametrize('K,n', [(5, 1), (5, 4), (5, 33), (70, 1), (70, 4), (70, 33)])
@pytest.mark.parametrize('case', sorted(MOVING))
def test_moving_humans_against_the_restatement(amd, case, K, n):
    eng, state, gtime = _moving_engine(amd, case)
    B = len(state)
    if case == 'h5_mixed':
        assert (_np(eng.human_count()) < 5).any()  # parked placeholders take part
    want = _reference(case, state, gtime, _cfg_of(eng), K, n)
    if (K, n) == (70, 33):  # the spread of outcomes, on the restatement's own output
        ended_in_collision = int((want['info'] == ref.COLLISION).sum())
        danger_and_on = sum(ref.DANGER in infos[:-1] for row in want['infos'] for infos in row)
        ran_all = int(((want['steps'] == n) & (want['info'] < ref.REACH_GOAL)).sum())
        timeouts = int((want['info'] == ref.TIMEOUT).sum())
        print(case, 'collision', ended_in_collision, 'danger and on', danger_and_on, 'ran all', ran_all, 'timeout', timeouts)
        assert ended_in_collision >= 1 and danger_and_on >= 1 and ran_all >= 1 and timeouts >= 1
    got = _look(eng, _table(B, K, n), final_state=True)
    for key in ('ret', 'info', 'steps', 'time', 'final_state8'):
        assert _same_bits(got[key], want[key]), (case, K, n, key, got[key], want[key])
    assert _same_bits(got['final_theta'], np.broadcast_to(_np(eng.get_theta())[:, None], (B, K)).copy())
    assert got['final_state8'][0, :, 1, 2].tolist() == [UNROUNDABLE] * K  # the human's own velocity, unrounded


# ------------------------------------------------------------------------------------------------ 3. invariances
def test_prefixes_in_k_b_and_n(amd):
    B, K, n = 3, 70, 33
    eng, state, gtime = _moving_engine(amd, 'h5')
    table = _table(B, K, n)
    full = _look(eng, table, final_state=True)
    # K: the first 5 candidates alone
    few = _look(eng, table[:, :5].copy(), final_state=True)
    for key, v in few.items():
        assert _same_bits(v, full[key][:, :5]), key
    # B: the first two envs alone, on an engine of two
    two = _engine(amd, 2, 5, discomfort_dist=0.5)
    two.set_state(state[:2], gtime[:2])
    two.set_theta(_np(eng.get_theta())[:2].copy())
    pair = _look(two, table[:2].copy(), final_state=True)
    for key, v in pair.items():
        assert _same_bits(v, full[key][:2]), key
    # n: the n = 4 call is the first 4 steps — a branch still running after them, continued from where the n = 4 call left
    # it with its remaining 29 rows, arrives where the n = 33 call arrives; one that ended inside them is the same branch
    four = _look(eng, table[:, :, :4].copy(), final_state=True)
    ended = four['info'] >= amd.REACH_GOAL
    for key in ('ret', 'info', 'steps', 'time', 'final_state8'):
        assert _same_bits(four[key][ended], full[key][ended]), key
    k = int(np.flatnonzero(~ended.any(axis=0))[0])
    eng.set_state(four['final_state8'][:, k].copy(), four['time'][:, k].copy())
    rest = _look(eng, table[:, k:k + 1, 4:].copy(), final_state=True)
    for key in ('info', 'time', 'final_state8'):
        assert _same_bits(rest[key][:, 0], full[key][:, k]), key
    assert (rest['steps'][:, 0] + 4 == full['steps'][:, k]).all()
    print('n prefix: steps', full['steps'][:, k].tolist(), 'ended inside 4:', int(ended.sum()))


def test_rows_after_the_end_are_not_used(amd):
    B, K, n = 3, 70, 33
    eng, _, _ = _moving_engine(amd, 'h5')
    table = _table(B, K, n)
    full = _look(eng, table, final_state=True)
    holes = table.copy()
    holes[np.arange(n)[None, None, :] >= full['steps'][:, :, None]] = np.nan
    assert np.isnan(holes).any()
    again = _look(eng, holes, final_state=True)
    for key, v in again.items():
        assert _same_bits(v, full[key]), key


def test_the_engine_is_untouched_and_switching_back(amd):
    import torch
    B, K, n = 3, 5, 12
    table = _table(B, K, n)
    drive = torch.from_numpy(_table(B, 1, 15, seed=5)[:, 0]).cuda()
    y, x = (_engine(amd, B, 5, ORCA, discomfort_dist=0.5) for _ in range(2))
    ybufs, xbufs = y.rollout_begin(**BEGIN), x.rollout_begin(**BEGIN)
    for t in range(5):
        y.rollout_step(drive[:, t].contiguous())
        x.rollout_step(drive[:, t].contiguous())
    snap, io_before, counts = _snapshot(y), {k: v.clone() for k, v in ybufs.items()}, y.launch_counts()
    before = _look(y, table, final_state=True)
    y.set_lookahead_human_model(CV)
    cv = _look(y, table, final_state=True)
    y.sync()
    for a, b in zip(snap, _snapshot(y)):
        assert torch.equal(a, b)
    for k, v in io_before.items():
        assert torch.equal(v, ybufs[k]), k
    assert y.launch_counts() == counts
    assert not np.array_equal(cv['final_state8'], before['final_state8'])  # the models are different futures
    # switching back: the ORCA lookahead gives the bits it gave
    y.set_lookahead_human_model(ORCA)
    after = _look(y, table, final_state=True)
    for key, v in after.items():
        assert _same_bits(v, before[key]), key
    # ... and the rollout goes on as on the twin that never looked ahead (scenario ring levels included: the episodes that end
    # in the next steps take the same scenarios)
    y.set_lookahead_human_model(CV)
    for t in range(5, 15):
        y.rollout_step(drive[:, t].contiguous())
        x.rollout_step(drive[:, t].contiguous())
        y.lookahead(table)
    for a, b in zip(_snapshot(y), _snapshot(x)):
        assert torch.equal(a, b)
    for k, v in xbufs.items():
        assert torch.equal(v, ybufs[k]), k
    assert y.launch_counts() == x.launch_counts()


def test_n_zero_is_a_no_op_under_either_model(amd):
    import torch
    B, K, H = 3, 4, 5
    eng = _engine(amd, B, H)
    eng.reset(1000 + np.arange(B))
    out = dict(ret=torch.full((B, K), 7.5, dtype=torch.float64), info=torch.full((B, K), 9, dtype=torch.uint8),
               steps=torch.full((B, K), -3, dtype=torch.int32), time=torch.full((B, K), 2.5, dtype=torch.float64),
               final_state8=torch.full((B, K, H + 1, 8), 1.5, dtype=torch.float64),
               final_theta=torch.full((B, K), 0.5, dtype=torch.float64))
    out = {k: v.cuda() for k, v in out.items()}
    keep = {k: v.clone() for k, v in out.items()}
    empty = torch.zeros((B, K, 0, 2), dtype=torch.float64).cuda()
    for model in (CV, ORCA):
        eng.set_lookahead_human_model(model)
        got = eng.lookahead(empty, final_state=True, out=out)
        eng.sync()
        for k, v in keep.items():
            assert got[k] is out[k] and torch.equal(v, out[k]), (model, k)
        dummy = torch.zeros(2, dtype=torch.float64).cuda()  # (an empty tensor has no address: the C call itself)
        import ctypes as C
        from crowdnav_amd import _lib
        from crowdnav_amd.engine import _struct
        lo = _struct(_lib.CnLookaheadOut, out)
        assert eng._lib.cn_lookahead_actions(eng._h, 0, K, dummy.data_ptr(), C.byref(lo)) == _lib.CN_OK
        eng.sync()
        for k, v in keep.items():
            assert torch.equal(v, out[k]), (model, k)


# ------------------------------------------------------------------------------------------------ 4. what inherits
def _sarl_engine(amd, B, H=5, **cfg):
    eng = _engine(amd, B, H, robot_visible=1, **cfg)
    eng.reset(1000 + np.arange(B))
    return configure_sarl(eng)


def test_bootstrap_under_the_model(amd):
    B, K, n = 3, 70, 6
    eng = _sarl_engine(amd, B)
    for _ in range(3):
        eng.step(np.tile([0.0, 1.0], (B, 1)), update=True, want_obs=False)
    state, gtime = (_np(x).copy() for x in eng.get_state())
    gtime[B - 1] = eng.config['time_limit'] - 1.0 - 0.5  # the last env's branches end in Timeout at their third step
    eng.set_state(state, gtime)
    table = _table(B, K, n)
    look = eng.lookahead(table, bootstrap=True)
    direct = _np(eng.sarl_state_values(look['final_state8']))
    look = {k: _np(v) for k, v in look.items()}
    plain = _look(eng, table, final_state=True)
    for key, v in plain.items():
        assert _same_bits(look[key], v), key  # the branches are the model's
    want = ref.lookahead(*(_np(x) for x in eng.get_state()), table, dict(_cfg_of(eng)), GAMMA)
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


@pytest.mark.parametrize('update', ['cem', 'mppi'])
def test_a_planning_step_is_draw_lookahead_update_under_the_model(amd, update):
    import torch
    eng, _, _ = _moving_engine(amd, 'h5')
    one, parts = _plan(eng), _plan(eng)
    if update == 'cem':
        eng.plan_cem(one, 21)
    else:
        eng.plan_mppi(one, 0.7, 21)
    eng.plan_draw(parts, 21)
    look = eng.lookahead(parts.candidates)
    for k, v in look.items():
        parts.look[k].copy_(v)
    if update == 'cem':
        eng.plan_refit(parts)
    else:
        eng.plan_mppi_update(parts, 0.7)
    eng.sync()
    for k, v in parts.tensors().items():
        assert torch.equal(v, one.tensors()[k]), k
    state, gtime = (_np(x) for x in eng.get_state())
    want = ref.lookahead(state, gtime, _np(one.candidates), _cfg_of(eng), GAMMA)
    assert _same_bits(one.look['ret'], want['ret'])  # ... and the lookahead inside was the constant-velocity one
    # the switch reaches the planner: the same plan scored under ORCA leaves other returns somewhere
    # (16 candidates of 12 steps: long enough for the humans' two futures to part inside a Danger step)
    plans = []
    for model in (CV, ORCA):
        eng.set_lookahead_human_model(model)
        plans.append(_plan(eng, K=16, n=12))
        if update == 'cem':
            eng.plan_cem(plans[-1], 21)
        else:
            eng.plan_mppi(plans[-1], 0.7, 21)
    eng.sync()
    assert torch.equal(plans[0].candidates, plans[1].candidates)
    print(update, 'ret under the two models', _np(plans[0].look['ret'])[0, :4].tolist(), _np(plans[1].look['ret'])[0, :4].tolist())
    assert not torch.equal(plans[0].look['ret'], plans[1].look['ret'])


def test_the_closed_loop_is_the_python_loop_and_its_real_steps_are_orca(amd):
    import torch
    B, K, n, E, I, steps, counter = 3, 5, 4, 2, 2, 3, 100
    made = []
    for _ in range(3):
        eng = _engine(amd, B, 5, discomfort_dist=0.5)
        eng.reset(1000 + np.arange(B))
        bufs = eng.rollout_begin(**BEGIN)
        made.append((eng, bufs, eng.plan_reset(eng.plan_begin(K, n, E, I, 0.3, seed=5, smoothing=0.25, min_std=0.01))))
    (x, xbufs, xplan), (y, ybufs, yplan), (z, _, _) = made
    assert x.plan_rollout(xplan, steps, counter) is xbufs
    actions = []
    for s in range(steps):
        y.plan_cem(yplan, counter + s * I)
        actions.append(yplan.action.clone())
        y.rollout_step(yplan.action)
        y.plan_shift(yplan)
    for a, b in zip(_snapshot(x), _snapshot(y)):
        assert torch.equal(a, b)
    for k, v in ybufs.items():
        assert torch.equal(v, xbufs[k]), k
    for k, v in yplan.tensors().items():
        assert torch.equal(v, xplan.tensors()[k]), k
    assert x.launch_counts() == y.launch_counts()
    # the real steps: the same actions through cn_step on an engine that was never told about the model
    z.set_lookahead_human_model(ORCA)
    for a in actions:
        z.step(a, update=True, want_obs=False)
    for a, b in zip(_snapshot(x), _snapshot(z)):
        assert torch.equal(a, b)
    assert x.lookahead_human_model == CV


# ------------------------------------------------------------------------------------------------ 5. refusals and surface
def test_setter_getter_and_refusals(amd):
    import ctypes as C
    import torch
    from crowdnav_amd import _lib
    B, H, K, n = 3, 5, 2, 5
    eng = amd.BatchedCrowdSim(num_envs=B, num_humans=H, robot_policy=amd.ROBOT_EXTERNAL)
    assert eng.lookahead_human_model == ORCA  # what cn_create installs
    eng.set_lookahead_human_model(CV)
    assert eng.lookahead_human_model == CV
    L = eng._lib
    for bad in (2, -1, 77):
        assert L.cn_lookahead_set_human_model(eng._h, bad) == _lib.CN_ERR_INVALID
        assert str(bad) in L.cn_last_error().decode() and 'model' in L.cn_last_error().decode()
        assert eng.lookahead_human_model == CV  # left as it was
    assert L.cn_lookahead_get_human_model(eng._h, None) == _lib.CN_ERR_INVALID
    with pytest.raises(ValueError):
        eng.set_lookahead_human_model('linear')
    with pytest.raises(AttributeError):
        eng.lookahead_human_model = ORCA
    eng.reset(1000 + np.arange(B))
    eng.rollout_begin(**BEGIN)
    eng.rollout_step(np.tile([0.0, 1.0], (B, 1)))
    assert eng.lookahead_human_model == CV  # cn_reset and the rollout calls do not change it
    # the lookahead's own refusals, unchanged under the model, nothing counted
    table = torch.from_numpy(_table(B, K, n)).cuda()
    counts = eng.launch_counts()
    out = eng.lookahead(table)
    from crowdnav_amd.engine import _struct
    lo = _struct(_lib.CnLookaheadOut, out)
    no_ret = _struct(_lib.CnLookaheadOut, {k: v for k, v in out.items() if k != 'ret'})
    for args, word in (((n, K, None, C.byref(lo)), 'actions is NULL'), ((n, K, table.data_ptr(), None), 'out is NULL'),
                       ((n, K, table.data_ptr(), C.byref(no_ret)), 'out->ret is NULL'),
                       ((-1, K, table.data_ptr(), C.byref(lo)), 'n_steps'), ((n, 0, table.data_ptr(), C.byref(lo)), 'n_candidates')):
        assert L.cn_lookahead_actions(eng._h, *args) == _lib.CN_ERR_INVALID
        assert word in L.cn_last_error().decode(), L.cn_last_error()
    assert eng.launch_counts() == counts
    orca = amd.BatchedCrowdSim(num_envs=B, num_humans=H, robot_policy=amd.ROBOT_ORCA)
    orca.set_lookahead_human_model(CV)
    with pytest.raises(_lib.CrowdNavAmdError) as ei:
        orca.lookahead(table)
    assert ei.value.status == _lib.CN_ERR_INVALID and 'CN_ROBOT_EXTERNAL' in str(ei.value)


def test_the_gym_surface(amd):
    import crowdnav_amd.compat as c
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
    orca = env.lookahead(sequences)
    assert env._eng.lookahead_human_model == ORCA
    got = env.lookahead(sequences, human_model=CV)
    assert env._eng.lookahead_human_model == CV
    want = _look(env._eng, rows[None].copy())
    state, gtime = (_np(x) for x in env._eng.get_state())
    restated = ref.lookahead(state, gtime, rows[None], _cfg_of(env._eng), GAMMA)
    for k in range(K):
        assert got[k][0] == float(want['ret'][0, k]) == float(restated['ret'][0, k])
        assert got[k][2] == int(want['steps'][0, k]) and type(got[k][1]) is type(info_from_code(int(want['info'][0, k])))
    rows_of = lambda scored: [(r[0], type(r[1]), r[2]) for r in scored]  # noqa: E731
    assert rows_of(env.lookahead(sequences)) == rows_of(got)  # None leaves the engine's setting alone
    assert rows_of(env.lookahead(sequences, human_model=ORCA)) == rows_of(orca)
    with pytest.raises(ValueError):
        env.lookahead(sequences, human_model='linear')


@pytest.mark.parametrize('mode', ['shooting', 'cem'])
def test_the_example_runs_under_the_model(amd, mode):
    cmd = [sys.executable, os.path.join(ROOT, 'examples', 'shooting_planner.py'), '--cases', '4', '--candidates', '8', '--horizon', '6',
           '--human-model', 'constant_velocity'] + (['--cem', '--iterations', '2'] if mode == 'cem' else [])
    done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    text = done.stdout.decode()
    assert done.returncode == 0, text
    assert 'TEST  has success rate:' in text and 'total reward:' in text, text
