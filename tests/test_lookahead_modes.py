"""cn_lookahead_modes and what is built on it, on the MI355X: the lookahead against M predicted futures at once.

(a) Every mode is the existing paths call: ret, info, steps and time of mode m bit-equal to lookahead_paths(actions, human_vel[:, m]).
(b) The reductions against the host restatement (lookahead_modes_reference.py), bit for bit.
(c) Prefixes in K, B, n and M.   (d) NaN rows behind every branch's end.   (e) Nothing of the engine moves; n = 0.
(f) The planners.   (g) The gym surface and the example.

Shapes: B = 3; 1, 5 and 12 humans, the `mixed` rule, a unicycle robot, 63 humans; K = 5 and K = 70 (two workgroups per env,
the second with a 6-lane tail); n = 1, 4 and 33; M = 1, 3 and 8 (12 humans x 8 modes = 96 human rows, more than the 64 lanes)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import lookahead_modes_reference as ref
from support import (  # noqa: F401  (amd: module fixture)
    amd, np_of as _np, same_bits as _same_bits, smoothed_plan as _plan, snapshot as _snapshot)

pytestmark = pytest.mark.gpu

BEGIN = dict(seed_base=1000, seed_mod=500, record_capacity=8)
ROWS = ('ret', 'info', 'steps', 'time')
REDUCED = ('score', 'risk', 'worst_mode', 'worst_info', 'worst_steps', 'worst_time')


def _engine(amd, B, H, **cfg):
    return amd.BatchedCrowdSim(num_envs=B, num_humans=H, robot_policy=amd.ROBOT_EXTERNAL, **dict(dict(discomfort_dist=0.5), **cfg))


def _scene_engine(amd, B, H, **cfg):
    """An engine holding lookahead_modes_reference.scene(B, H)."""
    eng = _engine(amd, B, H, **cfg)
    state, gtime = ref.scene(B, H)
    eng.set_state(state, gtime)
    return eng, state, gtime


def _modes(eng, *args, **kw):
    return {k: _np(v) for k, v in eng.lookahead_modes(*args, **kw).items()}


def _paths(eng, table, vel):
    return {k: _np(v) for k, v in eng.lookahead_paths(table, vel).items()}


# ------------------------------------------------------------------------------------------------ (a) every mode is the paths call
def _parity(eng, table, vel):
    got = _modes(eng, table, vel, per_mode=True)
    B, K = table.shape[:2]
    M = vel.shape[1]
    for key in ROWS:
        assert got[key].shape == (B, K, M)
    for m in range(M):
        want = _paths(eng, table, np.ascontiguousarray(vel[:, m]))
        for key in ROWS:
            assert _same_bits(got[key][:, :, m], want[key]), (m, key, got[key][:, :, m], want[key])
    return got


@pytest.mark.parametrize('M', [1, 3, 8])
@pytest.mark.parametrize('K,n', [(5, 1), (5, 4), (70, 4), (70, 33)])
@pytest.mark.parametrize('H', [1, 5, 12])
def test_every_mode_is_the_paths_call(amd, H, K, n, M):
    eng, state, _ = _scene_engine(amd, 3, H)
    got = _parity(eng, ref.action_table(3, K, n), ref.mode_tables(state, n, M))
    if (K, n, M) == (70, 33, 8):
        print('H', H, 'info', np.bincount(got['info'].ravel(), minlength=5).tolist(), 'steps', got['steps'].min(), got['steps'].max())
        ended = got['info'] >= amd.REACH_GOAL
        assert ended.any() and not ended.all() and (got['steps'].max(-1) != got['steps'].min(-1)).any()


def test_every_mode_is_the_paths_call_mixed(amd):
    """The `mixed` rule: parked placeholders take part in every mode, with the zeros the caller is asked to write."""
    B, H, K, n, M = 3, 5, 70, 33, 8
    eng = _engine(amd, B, H, scenario_rule=2)
    eng.reset(1000 + np.arange(B))
    for _ in range(3):
        eng.step(np.tile([0.0, 1.0], (B, 1)), update=True, want_obs=False)
    state = _np(eng.get_state()[0]).copy()
    parked = state[:, 1:, 0] >= 1.0e5
    assert (_np(eng.human_count()) < H).any() and parked.any() and (state[:, 1:, 2:4][parked] == 0.0).all()
    vel = ref.mode_tables(state, n, M)
    vel[np.broadcast_to(parked[:, None, None, :], vel.shape[:4])] = 0.0
    _parity(eng, ref.action_table(B, K, n), vel)


def test_every_mode_is_the_paths_call_unicycle(amd):
    B, H, K, n, M = 3, 5, 70, 33, 8
    from crowdnav_amd.compat.sarl import build_action_space
    space = np.array([list(a) for a in build_action_space(1.0, 5, 5, 'unicycle')[0]], dtype=np.float64)
    eng, state, _ = _scene_engine(amd, B, H, robot_kinematics=1)
    eng.set_theta(np.array([1.5, 1.0, 2.0]))
    table = space[np.random.RandomState(11).randint(len(space), size=(B, K, n))]
    table[:, 0] = (1.0, 0.0)
    got = _parity(eng, table, ref.mode_tables(state, n, M))
    assert (got['info'] == amd.COLLISION).any() and got['steps'].max() > got['steps'].min()


def test_63_humans_8_modes(amd):
    """504 human rows: the bound of the workgroup's LDS, eight rows per owner lane."""
    B, H, K, n, M = 1, 63, 5, 2, 8
    eng = _engine(amd, B, H)
    state, gtime = ref.scene(B, H)
    gtime[:] = 0.0
    eng.set_state(state, gtime)
    got = _parity(eng, ref.action_table(B, K, n), ref.mode_tables(state, n, M))
    want = ref.per_mode(state, gtime, ref.action_table(B, K, n), ref.mode_tables(state, n, M))
    for key in ROWS:
        assert _same_bits(got[key], want[key]), key


# ------------------------------------------------------------------------------------------------ (b) the reductions
@pytest.mark.parametrize('H,K,n,M', ref.REDUCTION_CASES)
def test_reductions_against_the_restatement(amd, H, K, n, M):
    state, gtime, actions, vel, want_modes = ref.case(H, K, n, M)
    eng = _engine(amd, 3, H)
    eng.set_state(state, gtime)
    weights = ref.weights_table(3, M)
    for w in (weights, None):
        for reduce in (ref.MEAN, ref.MIN):
            for penalty in (0.0, 0.5):
                got = _modes(eng, actions, vel, weights=w, reduce=reduce, risk_penalty=penalty, per_mode=True)
                for key in ROWS:
                    assert _same_bits(got[key], want_modes[key]), (key, w is None, reduce, penalty)
                want = ref.reduced(want_modes, w, reduce, penalty)
                for key in REDUCED:
                    assert _same_bits(got[key], want[key]), (key, w is None, reduce, penalty, got[key], want[key])
                short = _modes(eng, actions, vel, weights=w, reduce=reduce, risk_penalty=penalty)  # without the per-mode rows
                assert sorted(short) == sorted(REDUCED)
                for key in REDUCED:
                    assert _same_bits(short[key], want[key]), key
    assert (want['worst_mode'] != 0).any()


# ------------------------------------------------------------------------------------------------ (c) prefixes, (d) holes
def test_prefixes_and_rows_behind_the_ends(amd):
    H, K, n, M = 5, 70, 33, 8
    eng, state, gtime = _scene_engine(amd, 3, H)
    table, vel, weights = ref.action_table(3, K, n), ref.mode_tables(state, n, M), ref.weights_table(3, M)
    kw = dict(weights=weights, risk_penalty=0.5, per_mode=True)
    full = _modes(eng, table, vel, **kw)
    # (d) NaN behind every end: action rows behind the end of a branch's longest mode, table rows of a mode behind the end of
    # the env's longest branch
    longest = full['steps'].max(-1)
    holes, vholes = table.copy(), vel.copy()
    holes[np.arange(n)[None, None, :] >= longest[:, :, None]] = np.nan
    vholes[np.broadcast_to((np.arange(n)[None, :] >= longest.max(axis=1)[:, None])[:, None, :], vel.shape[:3])] = np.nan
    assert np.isnan(holes).any() and np.isnan(vholes).any()
    again = _modes(eng, holes, vholes, **kw)
    for key in ROWS + REDUCED:
        assert _same_bits(again[key], full[key]), key
    # K: the first 5 candidates alone
    few = _modes(eng, table[:, :5].copy(), vel, **kw)
    for key in ROWS + REDUCED:
        assert _same_bits(few[key], full[key][:, :5]), key
    # B: the first two envs alone, on an engine of two
    two = _engine(amd, 2, H)
    two.set_state(state[:2].copy(), gtime[:2].copy())
    pair = _modes(two, table[:2].copy(), vel[:2].copy(), **dict(kw, weights=weights[:2].copy()))
    for key in ROWS + REDUCED:
        assert _same_bits(pair[key], full[key][:2]), key
    # n: a mode that ended inside the first 4 steps is the same mode in the n = 4 call; one still running has made 4 steps
    four = _modes(eng, table[:, :, :4].copy(), vel[:, :, :4].copy(), **kw)
    inside = (full['info'] >= amd.REACH_GOAL) & (full['steps'] <= 4)
    assert inside.any() and not inside.all()
    for key in ROWS:
        assert _same_bits(four[key][inside], full[key][inside]), key
    assert (four['steps'][~inside] == 4).all()
    # M: dropping the last mode leaves the other modes' rows unchanged
    less = _modes(eng, table, vel[:, :M - 1].copy(), **dict(kw, weights=weights[:, :M - 1].copy()))
    for key in ROWS:
        assert less[key].shape == (3, K, M - 1) and _same_bits(less[key], full[key][:, :, :M - 1]), key
    want = ref.reduced(less, weights[:, :M - 1], ref.MEAN, 0.5)
    for key in REDUCED:
        assert _same_bits(less[key], want[key]), key


# ------------------------------------------------------------------------------------------------ (e) nothing moved
def test_the_engine_is_untouched(amd):
    import torch
    B, K, n, M = 3, 5, 12, 3
    table = ref.action_table(B, K, n)
    drive = torch.from_numpy(ref.action_table(B, 3, 15, seed=5)[:, 2]).cuda()
    y, x = (_engine(amd, B, 5) for _ in range(2))
    ybufs, xbufs = y.rollout_begin(**BEGIN), x.rollout_begin(**BEGIN)
    for t in range(5):
        y.rollout_step(drive[:, t].contiguous())
        x.rollout_step(drive[:, t].contiguous())
    y.set_lookahead_human_model('constant_velocity')
    snap, io_before, counts = _snapshot(y), {k: v.clone() for k, v in ybufs.items()}, y.launch_counts()
    vel = ref.mode_tables(_np(snap[0]), n, M)
    first = _modes(y, table, vel, per_mode=True)
    y.sync()
    for a, b in zip(snap, _snapshot(y)):
        assert torch.equal(a, b)
    for k, v in io_before.items():
        assert torch.equal(v, ybufs[k]), k
    assert y.launch_counts() == counts and y.lookahead_human_model == 'constant_velocity'
    assert (first['steps'] >= 1).all()
    # ... and the rollout goes on as on the twin that never looked ahead
    for t in range(5, 15):
        y.rollout_step(drive[:, t].contiguous())
        x.rollout_step(drive[:, t].contiguous())
        y.lookahead_modes(table, vel)
    for a, b in zip(_snapshot(y), _snapshot(x)):
        assert torch.equal(a, b)
    for k, v in xbufs.items():
        assert torch.equal(v, ybufs[k]), k
    assert y.launch_counts() == x.launch_counts() and y.lookahead_human_model == 'constant_velocity' and x.lookahead_human_model == 'orca'


def test_n_zero_is_a_no_op_and_live_refusals(amd):
    import torch
    from crowdnav_amd import _lib
    from crowdnav_amd.engine import _struct
    B, K, H, M = 3, 4, 5, 3
    eng = _engine(amd, B, H)
    eng.reset(1000 + np.arange(B))
    fill = dict(score=7.5, risk=1.5, worst_mode=-3, worst_info=9, worst_steps=-4, worst_time=2.5, ret=3.5, info=8, steps=-5, time=4.5)
    dtype = dict(score=torch.float64, risk=torch.float64, worst_mode=torch.int32, worst_info=torch.uint8, worst_steps=torch.int32,
                 worst_time=torch.float64, ret=torch.float64, info=torch.uint8, steps=torch.int32, time=torch.float64)
    out = {k: torch.full((B, K, M) if k in ROWS else (B, K), v, dtype=dtype[k]).cuda() for k, v in fill.items()}
    keep = {k: v.clone() for k, v in out.items()}
    got = eng.lookahead_modes(torch.zeros((B, K, 0, 2), dtype=torch.float64).cuda(),
                              torch.zeros((B, M, 0, H, 2), dtype=torch.float64).cuda(), per_mode=True, out=out)
    eng.sync()
    for k, v in keep.items():
        assert got[k] is out[k] and torch.equal(v, out[k]), k
    dummy = torch.zeros(2, dtype=torch.float64).cuda()  # (an empty tensor has no address: the C call itself)
    mo = _struct(_lib.CnModesOut, out)
    modes = _lib.CnPathModes(n_modes=M, reduce=0, risk_penalty=0.0, human_vel=dummy.data_ptr(), weight=None)
    counts = eng.launch_counts()
    assert eng._lib.cn_lookahead_modes(eng._h, 0, K, dummy.data_ptr(), C.byref(modes), C.byref(mo)) == _lib.CN_OK
    eng.sync()
    for k, v in keep.items():
        assert torch.equal(v, out[k]), k
    # on a live engine: the call's own refusals first, then the lookahead's
    modes.n_modes = 9
    assert eng._lib.cn_lookahead_modes(eng._h, -1, K, None, C.byref(modes), C.byref(mo)) == _lib.CN_ERR_UNSUPPORTED
    assert 'n_modes = 9' in eng._lib.cn_last_error().decode()
    modes.n_modes = M
    assert eng._lib.cn_lookahead_modes(eng._h, -1, K, dummy.data_ptr(), C.byref(modes), C.byref(mo)) == _lib.CN_ERR_INVALID
    assert 'n_steps must be >= 0' in eng._lib.cn_last_error().decode()
    assert eng.launch_counts() == counts
    with pytest.raises(ValueError, match='out\\[.score.\\]'):
        eng.lookahead_modes(np.zeros((B, K, 3, 2)), np.zeros((B, M, 3, H, 2)), out=dict(out, score=out['score'][:, :2]))
    orca = amd.BatchedCrowdSim(num_envs=B, num_humans=H, robot_policy=amd.ROBOT_ORCA)
    with pytest.raises(_lib.CrowdNavAmdError) as ei:
        orca.lookahead_modes(np.zeros((B, K, 3, 2)), np.zeros((B, M, 3, H, 2)))
    assert ei.value.status == _lib.CN_ERR_INVALID and 'CN_ROBOT_EXTERNAL' in str(ei.value)


# ------------------------------------------------------------------------------------------------ (f) planners
@pytest.mark.parametrize('reduce', ['mean', 'min'])
@pytest.mark.parametrize('update', ['cem', 'mppi'])
def test_a_planning_step_is_draw_lookahead_modes_update(amd, update, reduce):
    import torch
    B, H, K, n, I, M, counter = 3, 5, 5, 4, 3, 3, 21
    eng, state, gtime = _scene_engine(amd, B, H)
    vel = torch.from_numpy(ref.mode_tables(state, n, M)).cuda()
    weights = torch.from_numpy(ref.weights_table(B, M)).cuda()
    kw = dict(weights=weights, reduce=reduce, risk_penalty=0.5)
    one, parts = _plan(eng, K, n, I=I), _plan(eng, K, n, I=I)
    counts = eng.launch_counts()
    if update == 'cem':
        eng.plan_cem_modes(one, vel, counter, **kw)
    else:
        eng.plan_mppi_modes(one, vel, 0.7, counter, **kw)
    assert eng.launch_counts() == counts
    for i in range(I):  # the same step composed from the public calls
        eng.plan_draw(parts, counter + i)
        got = eng.lookahead_modes(parts.candidates, vel, **kw)
        parts.look['ret'].copy_(got['score'])
        parts.look['info'].copy_(got['worst_info'])
        parts.look['steps'].copy_(got['worst_steps'])
        parts.look['time'].copy_(got['worst_time'])
        if update == 'cem':
            eng.plan_refit(parts, keep_best=i > 0)
        else:
            eng.plan_mppi_update(parts, 0.7, keep_best=i > 0)
    eng.sync()
    for k, v in parts.tensors().items():
        assert torch.equal(v, one.tensors()[k]), k
    # ... and the lookahead inside was the modes one, on the last draw
    want = ref.reduced(ref.per_mode(state, gtime, _np(one.candidates), _np(vel)), _np(weights), reduce, 0.5)
    assert _same_bits(one.look['ret'], want['score']) and _same_bits(one.look['info'], want['worst_info'])
    assert _same_bits(one.look['steps'], want['worst_steps']) and _same_bits(one.look['time'], want['worst_time'])


@pytest.mark.parametrize('update', ['cem', 'mppi'])
def test_one_mode_of_weight_one_is_the_paths_planner(amd, update):
    import torch
    B, H, K, n, I, counter = 3, 5, 5, 4, 3, 21
    eng, state, _ = _scene_engine(amd, B, H)
    vel = torch.from_numpy(ref.mode_tables(state, n, 1)).cuda()
    ones = torch.ones((B, 1), dtype=torch.float64).cuda()
    modes, paths = _plan(eng, K, n, I=I), _plan(eng, K, n, I=I)
    if update == 'cem':
        eng.plan_cem_modes(modes, vel, counter, weights=ones)
        eng.plan_cem_paths(paths, vel[:, 0].contiguous(), counter)
    else:
        eng.plan_mppi_modes(modes, vel, 0.7, counter, weights=ones)
        eng.plan_mppi_paths(paths, vel[:, 0].contiguous(), 0.7, counter)
    eng.sync()
    for k, v in paths.tensors().items():
        assert torch.equal(v, modes.tensors()[k]), k


def test_bootstrap_plans_are_refused_with_counters_unchanged(amd):
    """On an engine whose value network is configured — where plan_cem_paths would bootstrap — the modes planners refuse."""
    import torch
    from conftest import load_golden
    from crowdnav_amd.compat.sarl import build_action_space
    B, K, n, M = 2, 5, 4, 3
    eng = _engine(amd, B, 5, robot_visible=1)
    eng.reset(1000 + np.arange(B))
    eng.sarl_configure(actions=np.array([list(a) for a in build_action_space(1.0)[0]], dtype=np.float64))
    g = load_golden('sarl_plain.npz')
    eng.sarl_set_weights({k[len('param_'):]: torch.from_numpy(v) for k, v in g.items() if k.startswith('param_')})
    vel = np.zeros((B, M, n, 5, 2))
    plan = eng.plan_begin(K, n, 2, 1, 0.3, bootstrap=True)
    before = {k: v.clone() for k, v in plan.tensors().items()}
    counts = eng.launch_counts()
    for name, call in (('cn_plan_cem_modes', lambda: eng.plan_cem_modes(plan, vel, 0)),
                       ('cn_plan_mppi_modes', lambda: eng.plan_mppi_modes(plan, vel, 1.0, 0))):
        with pytest.raises(amd.CrowdNavAmdError) as ei:
            call()
        assert ei.value.status == amd._lib.CN_ERR_UNSUPPORTED and 'bootstrap' in str(ei.value) and name in str(ei.value), str(ei.value)
    eng.sync()
    assert eng.launch_counts() == counts
    for k, v in before.items():
        assert torch.equal(v, plan.tensors()[k]), k
    # the engines every cn_plan_* call refuses stay refused, under the call's own name
    for other, status, word in ((amd.BatchedCrowdSim(num_envs=B, num_humans=5, robot_policy=amd.ROBOT_ORCA), amd._lib.CN_ERR_INVALID,
                                 'CN_ROBOT_EXTERNAL'),
                                (_engine(amd, B, 5, robot_kinematics=1), amd._lib.CN_ERR_UNSUPPORTED, 'CN_UNICYCLE engines are not served')):
        p = other.plan_begin(K, n, 2, 1, 0.3)
        with pytest.raises(amd.CrowdNavAmdError) as ei:
            other.plan_cem_modes(p, vel, 0)
        assert ei.value.status == status and word in str(ei.value) and 'cn_plan_cem_modes' in str(ei.value), str(ei.value)
    plain = eng.plan_begin(K, n, 2, 1, 0.3)
    with pytest.raises(ValueError):
        eng.plan_cem_modes(plain, np.zeros((B, M, n + 1, 5, 2)), 0)  # the table's n is the plan's
    with pytest.raises(amd.CrowdNavAmdError, match='temperature'):
        eng.plan_mppi_modes(plain, vel, 0.0, 0)
    with pytest.raises(amd.CrowdNavAmdError, match='risk_penalty'):
        eng.plan_cem_modes(plain, vel, 0, risk_penalty=-1.0)


# ------------------------------------------------------------------------------------------------ (g) compat and example
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
    rows = ref.action_table(1, K, n, seed=4)[0]
    sequences = [[c.ActionXY(float(vx), float(vy)) for vx, vy in seq] for seq in rows]
    env.reset('test', 0)
    state = _np(env._eng.get_state()[0])
    vel = predict.stack_modes(predict.constant_velocity(state, n), predict.to_goal(state, n, env.time_step))
    was = env._eng.lookahead_human_model
    got = env.lookahead_modes(sequences, vel[0], weights=[0.75, 0.25], reduce='min', risk_penalty=0.5)
    assert env._eng.lookahead_human_model == was
    want = _modes(env._eng, rows[None].copy(), vel, weights=np.array([[0.75, 0.25]]), reduce='min', risk_penalty=0.5)
    for k in range(K):
        assert len(got[k]) == 4 and got[k][:3] == (float(want['score'][0, k]), float(want['risk'][0, k]), int(want['worst_mode'][0, k]))
        assert type(got[k][3]) is type(info_from_code(int(want['worst_info'][0, k])))
    assert [r[:3] for r in env.lookahead_modes(sequences, vel[0].tolist(), [0.75, 0.25], 'min', 0.5)] == [r[:3] for r in got]
    with pytest.raises(ValueError):
        env.lookahead_modes(sequences, vel[0, :, :n - 1])
    with pytest.raises(ValueError):
        env.lookahead_modes(sequences, vel[0, 0])
    with pytest.raises(ValueError):
        env.lookahead_modes([], vel[0])


@pytest.mark.parametrize('args', [['--futures', 'cv,to_goal'], ['--futures', 'cv,to_goal', '--reduce', 'min', '--risk-penalty', '0.5', '--mppi']])
def test_the_example_runs_with_futures(amd, args):
    cmd = [sys.executable, os.path.join(ROOT, 'examples', 'predicted_paths_planner.py'), '--cases', '2', '--candidates', '8', '--horizon', '4',
           '--iterations', '2'] + args
    done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    text = done.stdout.decode()
    assert done.returncode == 0, text
    assert 'TEST  has success rate:' in text and 'collision rate:' in text and 'nav time:' in text, text
