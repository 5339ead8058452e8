"""Packed and multi-wave workgroups through the kernels that share the step kernel's workgroup, on the MI355X.

pick_geometry gives a small engine one env per workgroup on one wave, so at the sizes the other suites run none of these kernels
ever sees ebase != 0, a second env's slots of the LDS tables, a ragged last workgroup or the multi-wave block_sync — which is
what every engine above 2048 envs runs.  Here the engines are created under geometry_cases.py's (E, W) (proved on the host by
test_geometry_cases_host.py), every engine's geometry() is asserted, and each kernel family is compared bit for bit with the
reference its own suite uses:

  step_kernel, orca_kernel            the CPU oracle from its own reset state (the unicycle row: the device's sin / cos against libm's,
                                      within test_gpu_parity.py's bounds, and a twin at the default geometry bit for bit)
  rollout_actions[_trace]_kernel      the rollout_step loop (test_rollout_actions.py) on a default-geometry engine
  rollout_trace_kernel                the oracle stepped from the same state (an ORCA robot)
  rollout_lookahead[_goal]_kernel     the cn_step loop per candidate from the restored snapshot (test_lookahead.py), the goal
                                      term's restatement, sarl_state_values of the loop's end states for the bootstrap
  predict_orca[_robot|_goals]_kernel  predict_orca_cases' oracle tables
  sarl_decide_step_kernel             a default-geometry engine on the same seeds, weights and numpy streams
  the planners' closed loops          a default-geometry twin, support.assert_twins_equal

A reference engine is created with the knobs unset and must report E = 1 on one wave; what makes it right is the other suites.
No tolerance but the unicycle row's (above) is used.  Horizons: n <= 24, K and M 3 (5 at E = 3), B <= 9."""
import math

import numpy as np
import pytest

import geometry_cases as cases
import predict_orca_cases as orca_cases
import predict_orca_goals_cases as goals_cases
import predict_orca_robot_cases as robot_cases
from lookahead_goal_reference import goal_term
from support import (  # noqa: F401  (amd: module fixture)
    action_table, amd, assert_branch, assert_twins_equal, external_engine, np_of as _np, restore, rollout_after,
    rollout_step_loop, same_bits, same_tensors, sarl_engine, seeded_engine, smoothed_plan, snapshot, step_loop)

pytestmark = pytest.mark.gpu

BEGIN = dict(seed_base=1000, seed_mod=500, record_capacity=8)
_CACHE = {}  # references, made once per (family, crowd, settings, B) and only read afterwards


def _seeds(B):
    return 1000 + np.arange(B)


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _ref_key(family, row, **more):
    return (family, row['crowd'], tuple(sorted(row['cfg'].items())), row['B'], tuple(sorted(more.items())))


def _geometry_engine(amd, row, **cfg):
    """An engine of the row's crowd at the row's (E, W), asserted."""
    policy = cfg.pop('robot_policy', amd.ROBOT_EXTERNAL)
    with cases.knobs(row):
        eng = amd.BatchedCrowdSim(num_envs=row['B'], robot_policy=policy, **cases.engine_config(row, **cfg))
    cases.assert_geometry(eng, row)
    return eng


def _default_engine(amd, row, **cfg):
    """The reference twin: the same engine at the geometry pick_geometry chooses by itself."""
    policy = cfg.pop('robot_policy', amd.ROBOT_EXTERNAL)
    with cases.default_knobs():
        eng = amd.BatchedCrowdSim(num_envs=row['B'], robot_policy=policy, **cases.engine_config(row, **cfg))
    cases.assert_default_geometry(eng)
    return eng


def _unicycle(row):
    return bool(row['cfg'].get('robot_kinematics'))


# ------------------------------------------------------------------------------------------------ step_kernel, orca_kernel
@pytest.mark.parametrize('name', cases.NAMES)
def test_step_and_orca_against_the_oracle(amd, oracle_mod, name):
    """12 cn_step calls with caller-supplied actions from the oracle's own reset state: orca_vel, reward, done, info, dmin of
    every step and the state after it; cn_orca before the first and after the last."""
    row, T = cases.BY_NAME[name], 12
    B, uni = row['B'], _unicycle(row)
    cfg = cases.engine_config(row, robot_visible=1)
    o = oracle_mod.CrowdOracle(num_envs=B, robot_policy=0, **cfg)
    o.reset(_seeds(B))
    eng = _geometry_engine(amd, row, robot_visible=1)
    twin = _default_engine(amd, row, robot_visible=1) if uni else None
    for e in filter(None, (eng, twin)):
        e.set_state(o.get_state()[0], np.zeros(B))
        if uni:
            e.set_theta(o.get_theta())
    table = action_table(B, T, unicycle=uni, seed=13)
    theta0 = o.get_theta()
    assert same_bits(_np(eng.orca())[:, 1:], o.orca()[:, 1:])  # (the same start, bit for bit: nothing has turned yet)
    ended = np.zeros(B, bool)
    for t in range(T):
        got = {k: _np(v) for k, v in eng.step(table[:, t], update=True, want_obs=False).items() if v is not None}
        want = o.step(table[:, t], update=True)
        state, gtime = (_np(x) for x in eng.get_state())
        if not uni:
            for k in ('reward', 'done', 'info', 'dmin', 'action'):
                assert same_bits(got[k], want[k]), (name, t, k)
            assert same_bits(got['orca_vel'][:, 1:], want['orca_vel'][:, 1:]), (name, t)
            assert same_bits(state, o.get_state()[0]) and same_bits(gtime, o.get_state()[1]), (name, t)
        else:  # ActionRot: the device's cos / sin against libm's (test_unicycle_robot_vs_reference_and_oracle's bounds) ...
            assert np.array_equal(got['done'], want['done']) and np.array_equal(got['info'], want['info']), (name, t)
            assert np.abs(got['reward'] - want['reward']).max() <= 1e-9
            assert np.abs(state - o.get_state()[0]).max() <= 1e-9 and np.abs(_np(eng.get_theta()) - o.get_theta()).max() <= 1e-9
            # ... and the default geometry bit for bit
            ref = {k: _np(v) for k, v in twin.step(table[:, t], update=True, want_obs=False).items() if v is not None}
            for k in ('reward', 'done', 'info', 'dmin', 'action', 'orca_vel'):
                assert same_bits(got[k], ref[k]), (name, t, k)
            for a, b in zip(snapshot(eng), snapshot(twin)):
                assert same_bits(a, _np(b)), (name, t)
        ended |= want['done'] != 0
    if uni:
        assert (_np(eng.get_theta()) != theta0).any()  # the heading was carried
        assert same_bits(eng.orca(), _np(twin.orca()))
    else:
        assert same_bits(_np(eng.orca())[:, 1:], o.orca()[:, 1:])
    print(name, 'envs whose episode ended inside the 12 steps:', int(ended.sum()))


# ------------------------------------------------------------------------------------------------ rollout_actions
ACTIONS_CALLS = (16, 24)  # 32-step episodes (time_limit 8): the second call takes every env across its first episode end


def _actions_reference(amd, row):
    """The rollout_step loop with snapshots, and the traced table calls, on default-geometry engines."""
    import torch
    B, T = row['B'], sum(ACTIONS_CALLS)
    cfg = dict(robot_visible=1, time_limit=8.0)
    table = torch.from_numpy(action_table(B, T, unicycle=_unicycle(row), seed=7)).cuda()
    x = _default_engine(amd, row, **cfg)
    xbufs = x.rollout_begin(**BEGIN)
    snaps = dict(state8=[], ep_count=[], cur_steps=[], active=[])
    rollout_step_loop(x, xbufs, table, snaps)
    want = rollout_after(x, xbufs)
    snaps = {k: _np(torch.stack(v)).swapaxes(0, 1) for k, v in snaps.items()}  # [B, T, ...]
    w = _default_engine(amd, row, **cfg)
    w.rollout_begin(**BEGIN)
    rows = _traced_calls(w, table)
    assert (snaps['active'] == 1).all()  # nobody waited or retired: rows and snapshots line up by position
    assert (_np(want['ep_count']) >= 1).all(), _np(want['ep_count'])  # an episode end per env
    return dict(table=table, cfg=cfg, want=want, snaps=snaps, rows=rows)


def _traced_calls(eng, table):
    parts, t0 = [], 0
    for n in ACTIONS_CALLS:
        parts.append({k: _np(v) for k, v in eng.rollout_actions(table[:, t0:t0 + n].contiguous(), trace=True, rewards=True).items()})
        t0 += n
    return {k: np.concatenate([p[k] for p in parts], axis=1) for k in parts[0]}


@pytest.mark.parametrize('trace', [False, True], ids=['plain', 'trace'])
@pytest.mark.parametrize('name', cases.NAMES)
def test_rollout_actions_is_the_step_loop(amd, name, trace):
    """40 steps as two table calls of 16 and 24 across every env's first episode end: state, books and — traced — the rows."""
    row = cases.BY_NAME[name]
    ref = _cached(_ref_key('actions', row), lambda: _actions_reference(amd, row))
    table = ref['table']
    y = _geometry_engine(amd, row, **ref['cfg'])
    ybufs = y.rollout_begin(**BEGIN)
    if trace:
        rows = _traced_calls(y, table)
    else:
        t0 = 0
        for n in ACTIONS_CALLS:
            assert y.rollout_actions(table[:, t0:t0 + n].contiguous()) is ybufs
            t0 += n
    same_tensors(rollout_after(y, ybufs), ref['want'])
    assert y.launch_counts()['rollout_kernels'] == len(ACTIONS_CALLS)
    if trace:
        s = ref['snaps']
        assert same_bits(rows['episode'], s['ep_count']) and same_bits(rows['step'], s['cur_steps'])
        assert same_bits(rows['state8'], s['state8'])
        assert sorted(rows) == sorted(ref['rows'])
        for k in rows:
            assert same_bits(rows[k], ref['rows'][k]), (name, k)


# ------------------------------------------------------------------------------------------------ rollout_trace
TRACE_CASES = [(n, 0) for n in cases.HOLONOMIC] + [(n, 1) for n in cases.HOLONOMIC if cases.BY_NAME[n]['crowd'] == 'h20']


def _oracle_orca_run(oracle_mod, row, n):
    """n steps of an oracle whose robot is ORCA from its own reset state: the state before every step, what the step returned."""
    B = row['B']
    o = oracle_mod.CrowdOracle(num_envs=B, robot_policy=1, **cases.engine_config(row, robot_visible=1))
    o.reset(_seeds(B))
    run = dict(before=[], reward=[], info=[], dmin=[], done=[])
    for _ in range(n):
        run['before'].append(o.get_state()[0])
        out = o.step(None, update=True)
        for k in ('reward', 'info', 'dmin', 'done'):
            run[k].append(out[k])
    run = {k: np.stack(v, axis=1) for k, v in run.items()}  # [B, n, ...]
    run['after'] = o.get_state()[0]
    return run


@pytest.mark.parametrize('name,flags', TRACE_CASES)
def test_rollout_trace_against_the_oracle(amd, oracle_mod, name, flags):
    """One traced call of 24 steps of an ORCA-robot engine from the oracle's reset state: every row up to an env's first episode
    end is the oracle's state, reward, info and dmin.  flags = 1: the asynchronous scenario fill (20 humans)."""
    row, n = cases.BY_NAME[name], 24
    B = row['B']
    want = _cached(_ref_key('trace', row), lambda: _oracle_orca_run(oracle_mod, row, n))
    eng = _geometry_engine(amd, row, robot_policy=amd.ROBOT_ORCA, robot_visible=1, flags=flags)
    bufs = eng.rollout_begin(**BEGIN)
    eng.set_state(want['before'][:, 0], np.zeros(B))
    tr = {k: _np(v) for k, v in eng.rollout_trace(n, rewards=True).items()}
    eng.sync()
    whole = compared = 0
    for b in range(B):
        ends = np.flatnonzero(want['done'][b])
        Tb = int(ends[0]) + 1 if len(ends) else n
        compared += Tb
        assert (tr['episode'][b, :Tb] == 0).all() and np.array_equal(tr['step'][b, :Tb], np.arange(Tb)), (name, b)
        assert same_bits(tr['state8'][b, :Tb], want['before'][b, :Tb]), (name, b)
        for k in ('reward', 'info', 'dmin'):
            assert same_bits(tr[k][b, :Tb], want[k][b, :Tb]), (name, b, k)
        if not len(ends):
            whole += 1
            assert same_bits(_np(eng.get_state()[0])[b], want['after'][b]), (name, b)
            assert int(_np(bufs['cur_steps'])[b]) == n and int(_np(bufs['ep_count'])[b]) == 0
        elif Tb < n and not flags:  # the next row is the next episode's reset state
            assert tr['episode'][b, Tb] == 1 and tr['step'][b, Tb] == 0
    print(name, 'flags', flags, 'envs traced over all', n, 'steps:', whole, 'of', B, '; rows compared:', compared, 'of', B * n)
    assert compared >= 3 * B * n // 4  # (the 20-human episodes end in a collision after 21 steps and more)
    assert eng.launch_counts()['rollout_kernels'] == 1


# ------------------------------------------------------------------------------------------------ lookahead under 'orca'
LOOK_N, LOOK_K = 24, 5
NEAR = ('h1', 'h5')  # the crowds whose generators fit discomfort_dist = 0.5 (test_lookahead.py: GEOMETRIES)


def _look_cfg(row, **more):
    return dict({'discomfort_dist': 0.5} if row['crowd'] in NEAR else {}, **more)


def _look_table(row):
    """[B, 5, 24, 2]: candidate 0 walks straight on at full speed, candidate 1 at half speed, the rest are random rows."""
    uni = _unicycle(row)
    table = action_table(row['B'], LOOK_K, LOOK_N, unicycle=uni)
    table[:, 0], table[:, 1] = ((1.0, 0.0), (0.5, 0.0)) if uni else ((0.0, 1.0), (0.0, 0.5))
    return table


def _look_scene(eng):
    """After a seeded reset the robot's goal is put 1.5 m straight ahead: the full-speed candidate arrives after five steps,
    the half-speed one after ten, the random ones later or never — branches of one workgroup end at different steps."""
    eng.reset(_seeds(eng.B))
    state, gtime = (_np(x).copy() for x in eng.get_state())
    state[:, 0, 4] = state[:, 0, 0]
    state[:, 0, 5] = state[:, 0, 1] + 1.5
    eng.set_state(state, gtime)
    eng.set_theta(np.full(eng.B, math.pi / 2))  # (read by unicycle engines only: heading along +y)
    return snapshot(eng)


def _engine_kwargs(row, **more):
    """engine_config without num_humans (external_engine / sarl_engine take H by position)."""
    cfg = cases.engine_config(row, **more)
    return cfg.pop('num_humans'), cfg


def _assert_branches_end_apart(row, K, steps, n):
    """Two branches of one workgroup end with different `steps`, one of them before the horizon."""
    flat = steps.reshape(-1)
    apart = [g for g in cases.workgroups(row['B'] * K, row['E']) if len(set(flat[g].tolist())) >= 2 and flat[g].min() < n]
    if row['E'] >= 2:
        assert apart, (row['name'], steps.tolist())
    assert (steps.min(axis=1) < n).all() and (steps.max(axis=1) > steps.min(axis=1)).all(), steps.tolist()


@pytest.mark.parametrize('name', cases.NAMES)
def test_lookahead_is_the_step_loop_per_candidate(amd, name):
    """lookahead() under 'orca' without and with the goal weight 0.1: every output of every branch, and nothing moved."""
    import torch
    row = cases.BY_NAME[name]
    B, K = row['B'], row['K']
    H, cfg = _engine_kwargs(row, **_look_cfg(row))

    def reference():
        with cases.default_knobs():
            z = external_engine(amd, B, H, **cfg)
        cases.assert_default_geometry(z)
        snap, table = _look_scene(z), _look_table(row)
        wants = []
        for k in range(LOOK_K):
            restore(z, snap)
            wants.append(step_loop(z, table[:, k]))
        return dict(snap=snap, table=table, wants=wants)

    ref = _cached(_ref_key('look', row), reference)
    snap, table, wants = ref['snap'], np.ascontiguousarray(ref['table'][:, :K]), ref['wants'][:K]
    with cases.knobs(row):
        y = external_engine(amd, B, H, **cfg)
    cases.assert_geometry(y, row)
    restore(y, snap)
    plain = {k: _np(v) for k, v in y.lookahead(table, final_state=True).items()}
    for k in range(K):
        assert_branch(plain, k, wants[k], name)
    _assert_branches_end_apart(row, K, plain['steps'], LOOK_N)
    print(name, 'steps', plain['steps'].tolist(), 'info', plain['info'].tolist())
    y.set_lookahead_goal_weight(0.1)
    goal = {k: _np(v) for k, v in y.lookahead(table, final_state=True).items()}
    start = _np(snap[0])
    for k in range(K):
        term = np.array([goal_term(0.1, start[b, 0, 0:2], start[b, 0, 4:6], wants[k]['final_state8'][b, 0, 0:2]) for b in range(B)])
        assert_branch(goal, k, dict(wants[k], ret=wants[k]['ret'] + term), name)
    assert not same_bits(goal['ret'], plain['ret'])
    for a, b in zip(snap, snapshot(y)):  # nothing of the engine moved
        assert torch.equal(a, b)


@pytest.mark.parametrize('name', cases.H5)
def test_bootstrapped_lookahead_is_the_step_loop_and_the_value_of_its_end_states(amd, name):
    """lookahead(bootstrap=True) on the golden SARL weights: the branches as above, value = sarl_state_values of the step loop's
    end states on the default-geometry engine, score by the header's rule."""
    import torch
    row = cases.BY_NAME[name]
    B, K = row['B'], row['K']
    H, cfg = _engine_kwargs(row, **_look_cfg(row))

    def reference():
        with cases.default_knobs():
            z = sarl_engine(amd, B, H, **cfg)
        cases.assert_default_geometry(z)
        snap, table = _look_scene(z), _look_table(row)
        wants = []
        for k in range(LOOK_K):
            restore(z, snap)
            wants.append(step_loop(z, table[:, k]))
        value = _np(z.sarl_state_values(np.stack([w['final_state8'] for w in wants], axis=1))).reshape(B, LOOK_K)
        for k in range(LOOK_K):
            wants[k]['value'] = np.ascontiguousarray(value[:, k])
        return dict(snap=snap, table=table, wants=wants)

    ref = _cached(_ref_key('boot', row), reference)
    snap, table, wants = ref['snap'], np.ascontiguousarray(ref['table'][:, :K]), ref['wants'][:K]
    with cases.knobs(row):
        y = sarl_engine(amd, B, H, **cfg)
    cases.assert_geometry(y, row)
    restore(y, snap)
    look = {k: _np(v) for k, v in y.lookahead(table, bootstrap=True).items()}
    assert sorted(look) == ['final_state8', 'final_theta', 'info', 'ret', 'score', 'steps', 'time', 'value']
    for k in range(K):
        assert_branch(look, k, wants[k], name)  # `value` among them
    _assert_branches_end_apart(row, K, look['steps'], LOOK_N)
    ended = look['info'] >= amd.REACH_GOAL
    assert ended.any() and not ended.all()
    dt, v_pref = y.config['time_step'], y.config['robot_v_pref']
    for b in range(B):
        for k in range(K):
            boot = math.pow(0.9, int(look['steps'][b, k]) * dt * v_pref) * float(np.float64(look['value'][b, k]))
            want = look['ret'][b, k] if ended[b, k] else look['ret'][b, k] + boot
            assert same_bits(look['score'][b, k], np.float64(want)), (name, b, k)
    for a, b in zip(snap, snapshot(y)):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ the ORCA predictors
N = orca_cases.N


def _under_way(amd, row, **cfg):
    """predict_orca_cases.engine at the row's geometry: a seeded reset and four real steps straight on."""
    with cases.knobs(row):
        eng = orca_cases.engine(amd, row['crowd'], envs=row['B'], **dict(row['cfg'], **cfg))
    cases.assert_geometry(eng, row)
    return eng


def _oracle_table(oracle_mod, row, state, gtime, **settings):
    key = ('unseen', row['crowd'], state.tobytes(), gtime.tobytes(), tuple(sorted(settings.items())))
    return _cached(key, lambda: orca_cases.oracle_table(oracle_mod, row['crowd'], state, gtime, **settings))


@pytest.mark.parametrize('name', cases.HOLONOMIC)
def test_predict_orca_is_the_oracle(amd, oracle_mod, name):
    row = cases.BY_NAME[name]
    eng = _under_way(amd, row, robot_visible=1)
    state, gtime = (_np(x).copy() for x in eng.get_state())
    want, fallback, _ = _oracle_table(oracle_mod, row, state, gtime)
    if row['crowd'] in ('h12', 'h20'):
        assert fallback.any()  # a 3-D fallback solve somewhere in the table
    got = eng.predict_orca(N)
    differ = _np(got) != want
    print(name, 'entries that differ:', int(differ.sum()), 'of', differ.size, 'first', np.argwhere(differ)[:3].tolist())
    assert same_bits(got, want)


@pytest.mark.parametrize('name', cases.NAMES)
def test_predict_orca_robot_is_the_oracle(amd, oracle_mod, name):
    """The robot in human 1's way on a sequence that turns; the unicycle row from headings that wrap."""
    import torch
    row = cases.BY_NAME[name]
    B, uni = row['B'], _unicycle(row)
    eng = _under_way(amd, row, robot_visible=1)
    state, gtime = (_np(x).copy() for x in eng.get_state())
    placed, _, _ = robot_cases.place_robot(state)
    eng.set_state(placed, gtime)
    actions = robot_cases.sequences(envs=B, unicycle=uni)
    kw = {}
    if uni:
        theta = np.resize(robot_cases.THETA, B)
        eng.set_theta(torch.as_tensor(theta))
        assert (robot_cases.wraps(theta, actions) >= 1).any()
        kw = dict(theta=theta, robot_kinematics=1)
    want, fallback, _ = robot_cases.oracle_table(oracle_mod, row['crowd'], placed, gtime, actions, **kw)
    unseen = robot_cases.furthest(want, _oracle_table(oracle_mod, row, placed, gtime)[0])
    assert unseen > 1e-3  # a kernel that leaves the robot out fails
    if row['crowd'] in ('h12', 'h20'):
        assert fallback.any()
    got = eng.predict_orca_robot(N, actions)
    differ = _np(got) != want
    print(name, 'entries that differ:', int(differ.sum()), 'of', differ.size, 'first', np.argwhere(differ)[:3].tolist())
    assert same_bits(got, want)
    if uni:
        assert same_bits(eng.get_theta(), theta)  # the heading is read, not written


def _goal_maps(state, crowd, M):
    """[B, M, H, 2]: predict_orca_goals_cases' three maps, then quarter-turn-and-a-half rotations of the humans' own goals."""
    maps = goals_cases.goal_maps(state, crowd)
    if M > 3:
        maps = np.concatenate([maps, goals_cases.rotations(state, 8)[:, [1, 3][:M - 3]]], axis=1)
    return np.ascontiguousarray(maps)


@pytest.mark.parametrize('name', cases.HOLONOMIC)
def test_predict_orca_goals_is_the_oracle_per_mode(amd, oracle_mod, name):
    """B M virtual envs: the envs of one workgroup are modes of one env, or the last mode of one env and the first of the next."""
    import torch
    row = cases.BY_NAME[name]
    B, M = row['B'], row['M']
    eng = _under_way(amd, row, robot_visible=1)
    state, gtime = (_np(x).copy() for x in eng.get_state())
    maps = _goal_maps(state, row['crowd'], M)
    moving = ~goals_cases.parked(state)
    for m in range(M):  # the maps differ per mode ...
        for other in range(m):
            assert (maps[:, m][moving] != maps[:, other][moving]).any(), (m, other)
    for b in range(1, B):  # ... and per env
        assert not np.array_equal(maps[b], maps[b - 1])
    goals = torch.from_numpy(maps).to(eng.device)
    got = eng.predict_orca_goals(N, goals)
    assert tuple(got.shape) == (B, M, N, eng.H, 2) and same_bits(goals, maps)
    fallbacks = 0
    for m in range(M):
        want, fallback, _ = _oracle_table(oracle_mod, row, goals_cases.regoaled(state, maps[:, m]), gtime)
        fallbacks += int(fallback.sum())
        differ = _np(got[:, m]) != want
        print(name, 'mode', m, 'entries that differ:', int(differ.sum()), 'of', differ.size, 'first', np.argwhere(differ)[:3].tolist())
        assert same_bits(got[:, m].contiguous(), want), (name, m)
    if row['crowd'] in ('h12', 'h20'):
        assert fallbacks > 0
    assert not torch.equal(got[:, 1], got[:, 0]) and not torch.equal(got[:, 2], got[:, 1])


# ------------------------------------------------------------------------------------------------ the SARL decision
def _fused(row):
    """sarl_abi.hip: the fused decision + step kernel covers one-wave workgroups (without kd bookkeeping) only."""
    return row['W'] == 1


def _sarl_twins(amd, row):
    H, cfg = _engine_kwargs(row)
    with cases.knobs(row):
        y = sarl_engine(amd, row['B'], H, **cfg)
    with cases.default_knobs():
        x = sarl_engine(amd, row['B'], H, **cfg)
    cases.assert_geometry(y, row)
    cases.assert_default_geometry(x)
    assert y.sarl_network_route() == x.sarl_network_route() == 'narrow'
    return y, x


@pytest.mark.parametrize('name', cases.H5)
def test_sarl_select_and_step(amd, name):
    """Three decisions and steps: values, chosen action, and the transition (cn_orca's kernel in front of the network)."""
    row = cases.BY_NAME[name]
    y, x = _sarl_twins(amd, row)
    for t in range(3):
        got, want = y.sarl_select(), x.sarl_select()
        for k in ('values', 'best', 'action'):
            assert same_bits(got[k], _np(want[k])), (name, t, k)
        a, b = y.step(got['action'], update=True, want_obs=False), x.step(want['action'], update=True, want_obs=False)
        for k in ('reward', 'done', 'info', 'dmin', 'orca_vel'):
            assert same_bits(a[k], _np(b[k])), (name, t, k)
        for u, v in zip(snapshot(y), snapshot(x)):
            assert same_bits(u, _np(v)), (name, t)
    assert len(set(_np(got['best']).tolist())) >= 2  # not one action for every env


@pytest.mark.parametrize('name', cases.H5)
def test_sarl_sample_step(amd, name):
    """12 epsilon-greedy cn_sarl_sample_step calls: at one wave per workgroup the fused sarl_decide_step_kernel, at two the
    route the engine falls back to (cn_orca's kernel, the network with the decision, cn_step's kernel) — the launch counters
    say which.  Histories, chosen actions and states against the default geometry, where the env was still sampling."""
    import torch
    row, T, D, eps = cases.BY_NAME[name], 12, 13, 0.3
    B, H = row['B'], 5

    def run(eng):
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=eng.device)  # noqa: E731
        h = dict(traj=z((B, T, H, D), torch.float32), rew=z((T, B), torch.float64), info=z((T, B), torch.uint8),
                 dmin=z((T, B), torch.float64), act=z((T, B), torch.int32), alive=z((B,), torch.uint8), done=z((B,), torch.uint8),
                 action=z((B, 2), torch.float64))
        h['alive'].fill_(1)
        step = eng.sarl_sampler(**h)
        before, sampled = eng.launch_counts(), []
        for t in range(T):
            step(t, eps)
            sampled.append(h['alive'].clone())
        eng.sync()
        counts = {k: v - before[k] for k, v in eng.launch_counts().items()}
        out = {k: _np(v) for k, v in h.items()}
        out['sampled'] = _np(torch.stack(sampled)).astype(bool)  # [T, B]: alive after call t = the env took step t
        out['state'] = _np(eng.get_state()[0])
        return out, counts

    y, x = _sarl_twins(amd, row)
    (got, ycounts), (want, xcounts) = run(y), run(x)
    assert xcounts['sarl_narrow'] == T and xcounts['sarl_decide_steps'] == T
    assert ycounts['sarl_narrow'] == T and ycounts['sarl_decide_steps'] == (T if _fused(row) else 0), (name, ycounts)
    s = want['sampled']
    assert np.array_equal(got['sampled'], s) and s[0].all()
    assert same_bits(got['traj'][s.T], want['traj'][s.T])
    for k in ('rew', 'info', 'dmin', 'act'):
        assert same_bits(got[k][s], want[k][s]), (name, k)
    assert same_bits(got['state'][s[-1]], want['state'][s[-1]])
    assert len(set(want['act'][s].tolist())) >= 3  # decisions and explorations, not one action


# ------------------------------------------------------------------------------------------------ the planners' closed loops
def _closed_loop(amd, row, default):
    with (cases.default_knobs() if default else cases.knobs(row)):
        # time_limit 1.5 s: the third real step ends every env's first episode in Timeout (test_lookahead_goal.py)
        eng = seeded_engine(amd, row['B'], 5, robot_visible=1, time_limit=1.5)
    (cases.assert_default_geometry(eng) if default else cases.assert_geometry(eng, row))
    bufs = eng.rollout_begin(**BEGIN)
    return eng, bufs, smoothed_plan(eng, K=5, n=4, E=2, I=2)


PLANNERS = {
    'cem': lambda eng, plan, pred: eng.plan_rollout(plan, 3, 100),
    'mppi': lambda eng, plan, pred: eng.plan_mppi_rollout(plan, 3, 0.05, 100, fit_std=True),
    'predict_orca_nominal': lambda eng, plan, pred: eng.plan_predict_orca_nominal_rollout(plan, pred, 3, 100, orca_mode=1),
}


@pytest.mark.parametrize('planner', sorted(PLANNERS))
@pytest.mark.parametrize('name', cases.H5)
def test_a_closed_loop_per_planner(amd, name, planner):
    """K = 5, n = 4, three real steps in one call: the lookahead over B K virtual envs (or predict_orca_robot's kernel and the
    modes) and the real step at the row's geometry against a twin at the default one."""
    import torch
    row = cases.BY_NAME[name]
    (x, xbufs, xplan), (y, ybufs, yplan) = _closed_loop(amd, row, False), _closed_loop(amd, row, True)
    preds = [None, None]
    if planner == 'predict_orca_nominal':  # M = 2: to_goal, and the ORCA predictor's table in slot 1
        preds = [e.plan_predict_begin(p, models=('to_goal', 'cv'), reduce='min') for e, p in ((x, xplan), (y, yplan))]
    assert PLANNERS[planner](x, xplan, preds[0]) is xbufs
    assert PLANNERS[planner](y, yplan, preds[1]) is ybufs
    assert_twins_equal(x, xbufs, xplan, y, ybufs, yplan)
    if preds[0] is not None:
        assert torch.equal(preds[0].human_vel, preds[1].human_vel)
    assert (_np(xbufs['ep_count']) >= 1).all() and x.launch_counts()['rollout_kernels'] >= 3
