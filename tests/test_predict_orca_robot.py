"""The ORCA predictor with the robot in sight (cn_predict_orca_robot) and its closed loop (cn_plan_*_predict_orca_nominal_rollout) on
the GPU:
1. the environment is the oracle: predict_orca_robot(n, actions) against n steps of a CrowdOracle whose humans see the robot and
   whose robot takes the actions, bit for bit — holonomic and unicycle;
2. replay: for a sequence itself, lookahead_paths on its table is lookahead() under 'orca' on a robot_visible = 1 engine;
3. strided action rows, slots of a modes table, prefixes in n, independence of B;
4. any engine gives the robot_visible = 1 oracle's table, and nothing of it moves;   5. the refusals that need a live engine;
6. the closed loop against the per-step loop on a twin engine, bit for bit;   7. the example, with and without --device-loop.

Shapes: predict_orca_cases' — B = 3, n = 12; 1, 5, 12 and 20 humans and the `mixed` rule."""
import numpy as np
import pytest

import predict_orca_cases as base
import predict_orca_robot_cases as cases
from predict_orca_cases import BEGIN, FUTURES, KEYS, UPDATES, engine as _engine, replay_scene as _replay_scene
from support import (  # noqa: F401  (amd: module fixture)
    amd, example_line as _example_line, np_of as _np, roll_on as _roll_on, same_bits as _same_bits, smoothed_plan as _plan,
    snapshot as _snapshot)

pytestmark = pytest.mark.gpu

B, N = cases.B, cases.N


def _placed(eng):
    """The engine's robot put 1.0 m ahead of human 1, on that human's way; returns (placed state, gtime) as numpy."""
    state, gtime = (_np(x).copy() for x in eng.get_state())
    placed, _, _ = cases.place_robot(state)
    eng.set_state(placed, gtime)
    return placed, gtime


# ------------------------------------------------------------------------------------------------ 1. the environment is the oracle
@pytest.mark.parametrize('crowd', sorted(cases.CROWDS))
def test_the_environment_is_the_oracle(amd, oracle_mod, crowd):
    """From the state of an engine under way, the robot in human 1's way with a sequence that turns: predict_orca_robot(12, a) is
    orca_vel[:, 1:] of twelve steps step(a[:, t]) of the CPU oracle with robot_visible = 1 and fresh simulators, every row — the
    rows behind the oracle's `done` too."""
    eng = _engine(amd, crowd, robot_visible=1)
    placed, gtime = _placed(eng)
    actions = cases.sequences()
    want, fallback, done = cases.oracle_table(oracle_mod, crowd, placed, gtime, actions)
    unseen = cases.furthest(want, base.oracle_table(oracle_mod, crowd, placed, gtime)[0])
    stands = cases.furthest(want[:, 1:], cases.oracle_table(oracle_mod, crowd, placed, gtime, actions, robot='stands')[0][:, 1:])
    stale = cases.furthest(want, cases.oracle_table(oracle_mod, crowd, placed, gtime, actions, robot='stale')[0])
    print(crowd, 'furthest from robot unseen %.3f, standing (t >= 1) %.3f, stale velocity %.3f; fallback solves %d, rows behind '
          'done %d' % (unseen, stands, stale, fallback.sum(), done.sum()))
    assert unseen > 1e-3    # (a) a kernel that leaves the robot out fails
    assert stands > 1e-3    # (b) one that does not move it
    assert stale > 1e-3     # (c) one that moves it but shows the humans a stale velocity
    if crowd in ('h12', 'h20'):
        assert fallback.any()
    got = eng.predict_orca_robot(N, actions)
    assert tuple(got.shape) == (B, N, placed.shape[1] - 1, 2)
    differ = _np(got) != want
    print(crowd, 'entries that differ:', int(differ.sum()), 'of', differ.size, 'first', np.argwhere(differ)[:3].tolist())
    assert _same_bits(got, want)


def test_the_environment_is_the_oracle_unicycle(amd, oracle_mod):
    """A CN_UNICYCLE engine: the rows are ActionRot(v, r), r != 0, from headings that wrap through python's % at least once."""
    import torch
    eng = _engine(amd, 'h5', robot_visible=1, robot_kinematics=1)
    placed, gtime = _placed(eng)
    eng.set_theta(torch.as_tensor(cases.THETA))
    actions = cases.sequences(unicycle=True)
    assert (actions[:, :, 1] != 0.0).all() and (cases.wraps(cases.THETA, actions) >= 1).any()
    kw = dict(theta=cases.THETA, robot_kinematics=1)
    want = cases.oracle_table(oracle_mod, 'h5', placed, gtime, actions, **kw)[0]
    wrong = {'robot unseen': base.oracle_table(oracle_mod, 'h5', placed, gtime)[0],
             'stands': cases.oracle_table(oracle_mod, 'h5', placed, gtime, actions, robot='stands', **kw)[0],
             'stale velocity': cases.oracle_table(oracle_mod, 'h5', placed, gtime, actions, robot='stale', **kw)[0],
             'rows read as (vx, vy)': cases.oracle_table(oracle_mod, 'h5', placed, gtime, actions)[0],
             'heading 0': cases.oracle_table(oracle_mod, 'h5', placed, gtime, actions, robot_kinematics=1)[0]}
    for name, table in wrong.items():
        print('unicycle: furthest from', name, '%.3f' % cases.furthest(want[:, 1:], table[:, 1:]))
        assert cases.furthest(want[:, 1:], table[:, 1:]) > 1e-3, name
    got = eng.predict_orca_robot(N, actions)
    differ = _np(got) != want
    print('unicycle entries that differ:', int(differ.sum()), 'of', differ.size, 'first', np.argwhere(differ)[:3].tolist())
    assert _same_bits(got, want)
    assert _same_bits(eng.get_theta(), cases.THETA)  # the heading is read, not written


# ------------------------------------------------------------------------------------------------ 2. replay
@pytest.mark.parametrize('crowd', ['h1', 'h5', 'h12'])
def test_replay_of_orca(amd, crowd):
    """For each of _replay_scene's K = 9 sequences s_k: lookahead_paths(s_k as its own K = 1 table, predict_orca_robot(n, s_k)) is
    row k of lookahead(table) under 'orca' on every output — the table is the humans' policy when they see the robot on s_k."""
    K, n = 9, 10
    eng = _engine(amd, crowd, robot_visible=1)
    state, gtime = (_np(x).copy() for x in eng.get_state())
    placed, table = _replay_scene(state, K, n)
    eng.set_state(placed, gtime)
    eng.drop_sims()
    assert eng.lookahead_human_model == 'orca'
    want = {k: _np(v) for k, v in eng.lookahead(table, final_state=True).items()}
    print('replay', crowd, 'info', want['info'].tolist(), 'steps', want['steps'].tolist())
    assert (want['info'] == amd.COLLISION).any() and (want['info'] == amd.REACH_GOAL).any()
    assert ((want['steps'] == n) & (want['info'] < amd.REACH_GOAL)).any()
    unseen = eng.predict_orca(n)
    unseen_differs = 0
    for k in range(K):
        s_k = np.ascontiguousarray(table[:, k])
        got = {key: _np(v) for key, v in eng.lookahead_paths(s_k[:, None], eng.predict_orca_robot(n, s_k), final_state=True).items()}
        blind = {key: _np(v) for key, v in eng.lookahead_paths(s_k[:, None], unseen, final_state=True).items()}
        unseen_differs += any(not _same_bits(blind[key][:, 0], want[key][:, k]) for key in KEYS)
        for key in KEYS:
            differ = got[key][:, 0] != want[key][:, k]
            if differ.any():
                print('replay', crowd, 'branch', k, key, 'entries that differ:', int(differ.sum()), 'of', differ.size)
            assert _same_bits(got[key][:, 0], want[key][:, k]), (crowd, k, key)
    print('replay', crowd, 'branches the robot-unseen table gets wrong:', unseen_differs)
    assert unseen_differs >= 1


# ------------------------------------------------------------------------------------------------ 3. strides, slots, prefixes, B
@pytest.mark.parametrize('crowd', ['h5', 'h12'])
def test_strides_slots_prefixes_and_other_envs(amd, crowd):
    import torch
    eng = _engine(amd, crowd, robot_visible=1)
    placed, gtime = _placed(eng)
    # plan.candidates[:, 0] where it lies: K N rows between envs
    plan = _plan(eng, n=N)
    strided = eng.plan_draw(plan, 3)[:, 0]
    assert strided.data_ptr() == plan.candidates.data_ptr() and not strided.is_contiguous() and strided.stride(0) == 5 * N * 2
    alone = eng.predict_orca_robot(N, strided)
    assert torch.equal(alone, eng.predict_orca_robot(N, strided.contiguous()))
    assert not torch.equal(alone, eng.predict_orca_robot(N, plan.candidates[:, 1]))  # another candidate, another table
    assert not torch.equal(alone, eng.predict_orca(N))
    # a numpy table is copied to the device
    a = torch.as_tensor(cases.sequences(), device=eng.device)
    mine = eng.predict_orca_robot(N, a)
    assert torch.equal(mine, eng.predict_orca_robot(N, cases.sequences())) and not torch.equal(mine, alone)
    # slots: only slot m is written
    out = torch.full((B, 3, N, eng.H, 2), -7.0, dtype=torch.float64, device=eng.device)
    assert eng.predict_orca_robot(N, a, out=out, mode=1) is out
    assert bool((out[:, 0] == -7.0).all()) and bool((out[:, 2] == -7.0).all()) and torch.equal(out[:, 1], mine)
    one = torch.full((B, N, eng.H, 2), -7.0, dtype=torch.float64, device=eng.device)
    assert eng.predict_orca_robot(N, a, out=one) is one and torch.equal(one, mine)
    # a prefix in n — its rows N apart — and the no-op at n = 0
    assert torch.equal(eng.predict_orca_robot(5, a[:, :5]), mine[:, :5]) and torch.equal(eng.predict_orca_robot(1, a[:, :1]), mine[:, :1])
    assert tuple(eng.predict_orca_robot(0, a[:, :0]).shape) == (B, 0, eng.H, 2)
    # env 1 alone in a B = 1 engine given the same state
    single = _engine(amd, crowd, envs=1, steps=0, robot_visible=1)
    single.set_state(placed[1:2], gtime[1:2])
    assert torch.equal(single.predict_orca_robot(N, a[1:2]), mine[1:2])


# ------------------------------------------------------------------------------------------------ 4. any engine, and nothing moves
KINDS = {'robot_unseen': ('h12', dict(robot_visible=0)), 'orca_robot': ('h12', dict(robot_policy=1, robot_visible=1)),
         'unicycle': ('h5', dict(robot_kinematics=1, robot_visible=0))}


@pytest.mark.parametrize('kind', sorted(KINDS))
def test_any_engine_gives_the_table_and_nothing_of_it_moves(amd, oracle_mod, kind):
    """Engines whose humans do not see the robot, with an ORCA robot, with a unicycle robot, in the middle of a rollout: the
    table is the robot_visible = 1 external-robot oracle's from the same state; state, heading, launch counters, the human-model
    setting and the rollout's buffers are as before, and the rollout and a step() that follow give what a twin gives that was
    never asked — on the kd route (12 humans) that includes the simulators' visiting order and the ORCA robot's own simulator."""
    import torch
    crowd, cfg = KINDS[kind]
    cfg = dict(cfg)
    if 'robot_policy' in cfg:
        cfg['robot_policy'] = amd.ROBOT_ORCA
    eng, twin = (_engine(amd, crowd, steps=0, **cfg) for _ in range(2))
    bufs, tbufs = eng.rollout_begin(**BEGIN), twin.rollout_begin(**BEGIN)
    for e in (eng, twin):
        _roll_on(e, kind, 3)
    before, io_before = _snapshot(eng), {k: v.clone() for k, v in bufs.items()}
    counts, model = eng.launch_counts(), eng.lookahead_human_model
    unicycle = kind == 'unicycle'
    actions = cases.sequences(unicycle=unicycle)
    table = eng.predict_orca_robot(N, actions)
    slot = eng.predict_orca_robot(N, actions, out=eng.predict(N, ('cv', 'to_goal')), mode=0)
    state, gtime, theta = (_np(x) for x in before)
    kw = dict(theta=theta, robot_kinematics=1) if unicycle else {}
    want = cases.oracle_table(oracle_mod, crowd, state, gtime, actions, **kw)[0]
    print(kind, 'furthest from the robot-unseen table %.3f' % cases.furthest(want, base.oracle_table(oracle_mod, crowd, state, gtime)[0]))
    assert _same_bits(table, want) and _same_bits(slot[:, 0], want)
    assert eng.launch_counts() == counts and eng.lookahead_human_model == model
    for a, b in zip(before, _snapshot(eng)):
        assert torch.equal(a, b)
    for k, v in io_before.items():
        assert torch.equal(v, bufs[k]), k
    # ... the rollout goes on as if the calls had not been made, and so does a plain step
    for e in (eng, twin):
        _roll_on(e, kind, 2)
    for a, b in zip(_snapshot(eng), _snapshot(twin)):
        assert torch.equal(a, b)
    for k, v in tbufs.items():
        assert torch.equal(v, bufs[k]), k
    eng.predict_orca_robot(3, actions[:, :3])
    action = None if kind == 'orca_robot' else np.tile([0.3, 0.2], (B, 1))
    got, want_step = (e.step(action, update=True, want_obs=True) for e in (eng, twin))
    assert sorted(got) == sorted(want_step)
    for k, v in want_step.items():
        assert (v is None and got[k] is None) or torch.equal(v, got[k]), k
    for a, b in zip(_snapshot(eng), _snapshot(twin)):
        assert torch.equal(a, b)
    assert eng.launch_counts() == twin.launch_counts()


# ------------------------------------------------------------------------------------------------ 5. refusals on a live engine
def test_refusals_on_an_engine(amd):
    import ctypes as C
    import torch
    lib = amd._lib
    INV, UNS = lib.CN_ERR_INVALID, lib.CN_ERR_UNSUPPORTED
    L = lib.load()
    eng = _engine(amd, 'h5', steps=0, robot_visible=1)
    eng.rollout_begin(**BEGIN)
    table = torch.full((B, 2, N, eng.H, 2), -7.0, dtype=torch.float64, device=eng.device)
    rows = torch.zeros((B, N, 2), dtype=torch.float64, device=eng.device)
    eng.sync()
    counts = eng.launch_counts()
    vel, act = C.c_void_p(table.data_ptr()), C.c_void_p(rows.data_ptr())
    for args, status, word in (((N, 2, 1, act, 0, None), INV, 'human_vel is NULL'),
                               ((N, 2, 1, None, 0, vel), INV, 'robot_actions is NULL'),
                               ((N, 2, 1, act, -1, vel), INV, 'env_stride = -1'),
                               ((N, 2, 1, act, N - 1, vel), INV, 'env_stride = %d' % (N - 1)),
                               ((N, 0, 1, act, 0, vel), INV, 'n_modes must be >= 1'),
                               ((N, 9, 1, act, 0, vel), UNS, 'n_modes = 9 exceeds'),
                               ((N, 2, 2, act, 0, vel), INV, 'mode = 2 is outside 0 .. n_modes - 1 = 1'),
                               ((-1, 2, 1, act, 0, vel), INV, 'n_steps must be >= 0'),
                               ((2 ** 31 - 1, 8, 7, act, 0, vel), UNS, 'rows exceed')):
        assert L.cn_predict_orca_robot(eng._h, *args) == status, (word, L.cn_last_error())
        assert 'cn_predict_orca_robot: ' in L.cn_last_error().decode() and word in L.cn_last_error().decode(), L.cn_last_error()
    assert L.cn_predict_orca_robot(eng._h, 0, 2, 1, act, 0, vel) == lib.CN_OK  # zero steps: nothing written
    eng.sync()
    assert bool((table == -7.0).all()) and eng.launch_counts() == counts

    # the closed loop: the engines no cn_plan_* call serves stay refused under the new names
    def refused(e, plan, pred, status, *words):
        pred.human_vel.fill_(-7.0)
        e.sync()
        counts, keep = e.launch_counts(), {k: v.clone() for k, v in plan.tensors().items()}
        for name, args in (('cn_plan_cem_predict_orca_nominal_rollout', {}),
                           ('cn_plan_mppi_predict_orca_nominal_rollout', dict(temperature=1.0))):
            with pytest.raises(amd.CrowdNavAmdError) as ei:
                e.plan_predict_orca_nominal_rollout(plan, pred, 2, 3, **args)
            text = str(ei.value)
            assert ei.value.status == status and name in text and all(w in text for w in words), (name, text)
        e.sync()
        assert e.launch_counts() == counts and bool((pred.human_vel == -7.0).all())
        for k, v in keep.items():
            assert torch.equal(v, plan.tensors()[k]), k

    orca = amd.BatchedCrowdSim(num_envs=B, num_humans=5, robot_policy=amd.ROBOT_ORCA)
    orca.rollout_begin(**BEGIN)
    plan = orca.plan_begin(5, 4, 2, 1, 0.3)
    refused(orca, plan, orca.plan_predict_begin(plan, ('cv', 'to_goal')), INV, 'CN_ROBOT_EXTERNAL')
    uni = _engine(amd, 'h5', steps=0, robot_kinematics=1)
    uni.rollout_begin(**BEGIN)
    plan = uni.plan_begin(5, 4, 2, 1, 0.3)
    refused(uni, plan, uni.plan_predict_begin(plan, 'to_goal'), UNS, 'CN_UNICYCLE')
    plan = _plan(eng)
    pred = eng.plan_predict_begin(plan, ('cv', 'to_goal'))
    pred.c.model[1] = 4
    refused(eng, plan, pred, INV, 'model[1] = 4 unknown')
    pred.c.model[1] = lib.PREDICT_TO_GOAL
    with pytest.raises(amd.CrowdNavAmdError, match='n_real_steps'):
        eng.plan_predict_orca_nominal_rollout(plan, pred, -1, 0)
    fresh = _engine(amd, 'h5', steps=0)
    fplan = _plan(fresh)
    with pytest.raises(RuntimeError, match='rollout_begin'):
        fresh.plan_predict_orca_nominal_rollout(fplan, fresh.plan_predict_begin(fplan, 'cv'), 1, 0)


# ------------------------------------------------------------------------------------------------ 6. the closed loop
def _loop_step(eng, plan, futures, update, counter, n):
    """One step of the loop the nominal rollout replaces, every part by its own call."""
    many = not isinstance(futures['models'], str)
    eng.plan_draw(plan, counter)
    vel = eng.predict(n, futures['models'])
    eng.predict_orca_robot(n, plan.candidates[:, 0], out=vel, mode=futures['orca_mode'] if many else None)
    if many:
        if update:
            eng.plan_mppi_modes(plan, vel, update['temperature'], counter, reduce=futures['reduce'], fit_std=update['fit_std'])
        else:
            eng.plan_cem_modes(plan, vel, counter, reduce=futures['reduce'])
    elif update:
        eng.plan_mppi_paths(plan, vel, update['temperature'], counter, fit_std=update['fit_std'])
    else:
        eng.plan_cem_paths(plan, vel, counter)
    eng.rollout_step(plan.action)
    eng.plan_shift(plan)
    return vel


@pytest.mark.parametrize('update', sorted(UPDATES))
@pytest.mark.parametrize('futures', sorted(FUTURES))
def test_the_closed_loop_is_the_per_step_loop(amd, futures, update):
    """plan_predict_orca_nominal_rollout against plan_draw + predict + predict_orca_robot(candidates[:, 0]) + plan_*_paths |
    plan_*_modes + rollout_step + plan_shift on a twin, six real steps, K = 5, n = 4, I = 2.  time_limit 2.0 s: five-step
    episodes, so the plans of running envs shift and every env is predicted from a new scenario inside the call; of 5 episodes
    the last env to end one retires."""
    import torch
    n, I, steps, counter = 4, 2, 6, 100
    F, U = FUTURES[futures], UPDATES[update]

    def make():
        eng = _engine(amd, 'h5', steps=0, robot_visible=1, time_limit=2.0)
        return eng, eng.rollout_begin(episode_limit=5, **BEGIN), _plan(eng)

    (x, xbufs, xplan), (y, ybufs, yplan) = make(), make()
    begin = {k: v for k, v in F.items() if k not in ('orca_mode',)}
    pred = x.plan_predict_begin(xplan, **begin)
    assert x.plan_predict_orca_nominal_rollout(xplan, pred, steps, counter, orca_mode=F['orca_mode'], **U) is xbufs
    for s in range(steps):
        vel = _loop_step(y, yplan, F, U, counter + s * I, n)
    for a, b in zip(_snapshot(x), _snapshot(y)):
        assert torch.equal(a, b)
    for k, v in ybufs.items():
        assert torch.equal(v, xbufs[k]), k
    assert sorted(xplan.tensors()) == sorted(yplan.tensors())
    for k, v in yplan.tensors().items():
        assert torch.equal(v, xplan.tensors()[k]), k
    assert torch.equal(x.rollout_records(), y.rollout_records())
    assert x.launch_counts() == y.launch_counts()
    assert torch.equal(pred.human_vel, vel.reshape(pred.human_vel.shape))
    print(futures, update, 'ep_count', _np(xbufs['ep_count']).tolist(), 'active', _np(xbufs['active']).tolist())
    assert int(_np(xbufs['ep_count']).sum()) >= 3 and int((_np(xbufs['active']) == 0).sum()) >= 1
    # the robot-unseen loop leaves another table behind
    w, wbufs, wplan = make()
    wpred = w.plan_predict_begin(wplan, **begin)
    w.plan_predict_orca_rollout(wplan, wpred, steps, counter, orca_mode=F['orca_mode'], **U)
    assert not torch.equal(wpred.human_vel, pred.human_vel)
    # chunks add up: 3 + 3 steps on another engine; zero steps is a no-op
    z, zbufs, zplan = make()
    zpred = z.plan_predict_begin(zplan, **begin)
    keep = {k: v.clone() for k, v in zplan.tensors().items()}
    zpred.human_vel.fill_(-7.0)
    assert z.plan_predict_orca_nominal_rollout(zplan, zpred, 0, counter, orca_mode=F['orca_mode'], **U) is zbufs
    assert bool((zpred.human_vel == -7.0).all()) and all(torch.equal(v, zplan.tensors()[k]) for k, v in keep.items())
    z.plan_predict_orca_nominal_rollout(zplan, zpred, 3, counter, orca_mode=F['orca_mode'], **U)
    z.plan_predict_orca_nominal_rollout(zplan, zpred, 3, counter + 3 * I, orca_mode=F['orca_mode'], **U)
    for a, b in zip(_snapshot(x), _snapshot(z)):
        assert torch.equal(a, b)
    assert torch.equal(zpred.human_vel, pred.human_vel)


# ------------------------------------------------------------------------------------------------ 7. the example
def test_the_example_sees_the_plan_with_and_without_the_device_loop(amd):
    """--futures to_goal,orca --orca-sees-plan: the per-step loop (plan_draw + predict_orca_robot per real step) and the one-call
    loop (plan_predict_orca_nominal_rollout, in chunks of 3) print the same line."""
    args = ['--futures', 'to_goal,orca', '--reduce', 'min', '--risk-penalty', '0.5', '--orca-sees-plan']
    host = _example_line(args)
    got = _example_line(args + ['--device-loop', '--chunk', '3'])
    print(host)
    assert got == host
