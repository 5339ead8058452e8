"""The ORCA predictor (cn_predict_orca) and its closed loop (cn_plan_*_predict_orca_rollout) on the GPU:
1. the environment is the oracle: predict_orca(n) against n steps of a CrowdOracle whose humans do not see the robot, bit for bit;
2. replay: on an engine whose humans do not see the robot, lookahead_paths on that table is lookahead() under 'orca';
3. slots of a modes table, prefixes in n, independence of B;   4. nothing of the engine moves;
5. the closed loop against the per-step loop on a twin engine, bit for bit, and the refusals that need a live engine.

Shapes: B = 3, n = 12; 1, 5, 12 and 20 humans (the 5-half-plane kernels, the kd route, the two-sweep pair phase) and the `mixed`
rule."""
import numpy as np
import pytest

import predict_orca_cases as cases
from predict_orca_cases import BEGIN, FUTURES, KEYS, UPDATES, engine as _engine, replay_scene as _replay_scene
from support import (  # noqa: F401  (amd: module fixture)
    amd, example_line as _example_line, np_of as _np, roll_on as _roll_on, same_bits as _same_bits, smoothed_plan as _plan,
    snapshot as _snapshot)

pytestmark = pytest.mark.gpu

B, N = cases.B, cases.N


# ------------------------------------------------------------------------------------------------ 1. the environment is the oracle
@pytest.mark.parametrize('seen_before', [1, 0], ids=['robot_visible', 'robot_unseen_stale_sims'])
@pytest.mark.parametrize('crowd', sorted(cases.CROWDS))
def test_the_environment_is_the_oracle(amd, oracle_mod, crowd, seen_before):
    """From the state of an engine under way, predict_orca(12) is orca_vel[:, 1:] of twelve steps of the CPU oracle with
    robot_visible = 0 and fresh simulators, every row — the rows behind the oracle's `done` too.  robot_unseen_stale_sims: the
    engine's humans never saw the robot and it made six more steps, so its own kd rows are not a fresh simulator's; the table
    is the fresh-simulator oracle's all the same."""
    from crowdnav_amd import predict
    eng = _engine(amd, crowd, steps=4 if seen_before else 10, robot_visible=seen_before)
    state, gtime = (_np(x).copy() for x in eng.get_state())
    want, fallback, done = cases.oracle_table(oracle_mod, crowd, state, gtime)
    H = state.shape[1] - 1
    # the preconditions, on the oracle's table
    from_goal = cases.differs_from(want, predict.to_goal(state, N, 0.25))
    seen = np.sqrt(((cases.visible_first_step(oracle_mod, crowd, state, gtime) - want[:, 0]) ** 2).sum(axis=-1))
    print(crowd, 'seen before', seen_before, 'furthest from to_goal %.3f (nearest human %.3g), fallback solves %d, robot seen %.3f, '
          'rows after done %d' % (from_goal.max(), from_goal.min(), fallback.sum(), seen.max(), done.sum()))
    if seen_before:
        if crowd in ('h5', 'h12', 'h20'):
            assert (from_goal > 1e-3).all()
        if crowd in ('h12', 'h20'):
            assert fallback.any()
        assert seen.max() > 1e-3  # a kernel that left the robot in fails at row 0
    got = eng.predict_orca(N)
    assert tuple(got.shape) == (B, N, H, 2)
    differ = _np(got) != want
    print(crowd, 'entries that differ:', int(differ.sum()), 'of', differ.size, 'first', np.argwhere(differ)[:3].tolist())
    assert _same_bits(got, want)
    if crowd == 'h5_mixed':
        parked = state[:, 1:, 0] >= 1.0e5
        assert parked.any() and not parked.all()


# ------------------------------------------------------------------------------------------------ 2. replay
@pytest.mark.parametrize('crowd', ['h1', 'h5', 'h12'])
def test_replay_of_orca(amd, crowd):
    """lookahead_paths(actions, predict_orca(n)) equals lookahead(actions) under 'orca' on every output of all K = 9 branches:
    the table is the humans' policy when they do not see the robot.  Fresh simulators on both sides (the kd route)."""
    K, n = 9, 10
    eng = _engine(amd, crowd, robot_visible=0)
    state, gtime = (_np(x).copy() for x in eng.get_state())
    placed, table = _replay_scene(state, K, n)
    eng.set_state(placed, gtime)
    eng.drop_sims()
    vel = eng.predict_orca(n)
    assert eng.lookahead_human_model == 'orca'
    want = {k: _np(v) for k, v in eng.lookahead(table, final_state=True).items()}
    got = {k: _np(v) for k, v in eng.lookahead_paths(table, vel, final_state=True).items()}
    print('replay', crowd, 'info', want['info'].tolist(), 'steps', want['steps'].tolist())
    assert (want['info'] == amd.COLLISION).any() and (want['info'] == amd.REACH_GOAL).any()
    assert ((want['steps'] == n) & (want['info'] < amd.REACH_GOAL)).any()
    assert (_np(vel)[:, 1:] != _np(vel)[:, :-1]).any()  # the humans turn: not the constant-velocity case
    for key in KEYS:
        differ = got[key] != want[key]
        print('replay', crowd, key, 'entries that differ:', int(differ.sum()), 'of', differ.size)
    for key in KEYS:
        assert _same_bits(got[key], want[key]), (crowd, key)


# ------------------------------------------------------------------------------------------------ 3. slots, prefixes, B
@pytest.mark.parametrize('crowd', ['h5', 'h12'])
def test_slots_prefixes_and_other_envs(amd, crowd):
    import torch
    eng = _engine(amd, crowd, robot_visible=1)
    alone = eng.predict_orca(N)
    out = eng.predict(N, ('cv', 'to_goal', 'cv'))
    made = out.clone()
    assert eng.predict_orca(N, out=out, mode=2) is out
    assert torch.equal(out[:, :2], made[:, :2]) and torch.equal(out[:, 2], alone) and not torch.equal(out[:, 2], made[:, 2])
    # a slot in the middle, of a table nobody initialised: the others keep their bits
    out = torch.full((B, 3, N, eng.H, 2), -7.0, dtype=torch.float64, device=eng.device)
    eng.predict_orca(N, out=out, mode=1)
    assert bool((out[:, 0] == -7.0).all()) and bool((out[:, 2] == -7.0).all()) and torch.equal(out[:, 1], alone)
    # `out` without a mode is written where it lies; M = 1, mode 0 is the same table
    one = torch.full((B, N, eng.H, 2), -7.0, dtype=torch.float64, device=eng.device)
    assert eng.predict_orca(N, out=one) is one and torch.equal(one, alone)
    assert torch.equal(eng.predict_orca(N, out=torch.zeros_like(one)[:, None].contiguous(), mode=0)[:, 0], alone)
    # a prefix in n, and no-op at n = 0
    assert torch.equal(eng.predict_orca(5), alone[:, :5]) and torch.equal(eng.predict_orca(1), alone[:, :1])
    assert tuple(eng.predict_orca(0).shape) == (B, 0, eng.H, 2)
    # env 1 alone in a B = 1 engine given the same state
    state, gtime = eng.get_state()
    single = _engine(amd, crowd, envs=1, steps=0, robot_visible=1)
    single.set_state(state[1:2].contiguous(), gtime[1:2].contiguous())
    assert torch.equal(single.predict_orca(N), alone[1:2])


# ------------------------------------------------------------------------------------------------ 4. nothing moves
KINDS = {'external': ('h12', {}), 'orca_robot': ('h12', dict(robot_policy=1)), 'unicycle': ('h5', dict(robot_kinematics=1))}


@pytest.mark.parametrize('kind', sorted(KINDS))
def test_predict_orca_moves_nothing_of_the_engine(amd, kind):
    """In the middle of a rollout_begin / rollout_step sequence: state, heading, launch counters, the human-model setting and
    the rollout's buffers are as before, and the rollout and a step() that follow give what a twin gives that was never
    asked — on the kd route (12 humans) that includes the simulators' visiting order and the ORCA robot's captured simulator."""
    import torch
    crowd, cfg = KINDS[kind]
    cfg = dict(cfg, robot_visible=1)
    if 'robot_policy' in cfg:
        cfg['robot_policy'] = amd.ROBOT_ORCA
    eng, twin = (_engine(amd, crowd, steps=0, **cfg) for _ in range(2))
    bufs, tbufs = eng.rollout_begin(**BEGIN), twin.rollout_begin(**BEGIN)
    for e in (eng, twin):
        _roll_on(e, kind, 3)
    if kind == 'external':
        for e in (eng, twin):
            e.set_lookahead_human_model('constant_velocity')
    before, io_before = _snapshot(eng), {k: v.clone() for k, v in bufs.items()}
    counts, model = eng.launch_counts(), eng.lookahead_human_model
    table = eng.predict_orca(N)
    eng.predict_orca(N, out=eng.predict(N, ('cv', 'to_goal')), mode=0)
    assert bool(torch.isfinite(table).all()) and bool((table != 0.0).any())
    assert eng.launch_counts() == counts and 'lagged_fills' in counts and eng.lookahead_human_model == model
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
    eng.predict_orca(3)
    action = None if kind == 'orca_robot' else np.tile([0.3, 0.2], (B, 1))
    got, want = (e.step(action, update=True, want_obs=True) for e in (eng, twin))
    assert sorted(got) == sorted(want)
    for k, v in want.items():
        assert (v is None and got[k] is None) or torch.equal(v, got[k]), k
    for a, b in zip(_snapshot(eng), _snapshot(twin)):
        assert torch.equal(a, b)
    assert eng.launch_counts() == twin.launch_counts()


# ------------------------------------------------------------------------------------------------ 5. the closed loop
def _loop_step(eng, plan, futures, update, counter, n):
    """One step of the loop the rollout replaces, every part by its own call."""
    many = not isinstance(futures['models'], str)
    vel = eng.predict(n, futures['models'])
    eng.predict_orca(n, out=vel, mode=futures['orca_mode'] if many else None)
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
    """plan_predict_orca_rollout against predict + predict_orca + plan_*_paths | plan_*_modes + rollout_step + plan_shift on a
    twin, six real steps, K = 5, n = 4, I = 2.  time_limit 2.0 s: five-step episodes, so the plans of running envs shift and
    every env is predicted from a new scenario inside the call; of 5 episodes the last env to end one retires."""
    import torch
    n, I, steps, counter = 4, 2, 6, 100
    F, U = FUTURES[futures], UPDATES[update]
    made = []
    for _ in range(2):
        eng = _engine(amd, 'h5', steps=0, robot_visible=1, time_limit=2.0)
        bufs = eng.rollout_begin(episode_limit=5, **BEGIN)
        made.append((eng, bufs, _plan(eng)))
    (x, xbufs, xplan), (y, ybufs, yplan) = made
    begin = {k: v for k, v in F.items() if k not in ('orca_mode',)}
    pred = x.plan_predict_begin(xplan, **begin)
    assert x.plan_predict_orca_rollout(xplan, pred, steps, counter, orca_mode=F['orca_mode'], **U) is xbufs
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
    # the scratch table holds what the last planning step scored against: the ORCA slot over cn_predict's
    assert torch.equal(pred.human_vel, vel.reshape(pred.human_vel.shape))
    print(futures, update, 'ep_count', _np(xbufs['ep_count']).tolist(), 'active', _np(xbufs['active']).tolist())
    assert int(_np(xbufs['ep_count']).sum()) >= 3 and int((_np(xbufs['active']) == 0).sum()) >= 1
    # chunks add up: 3 + 3 steps on a third engine
    z = _engine(amd, 'h5', steps=0, robot_visible=1, time_limit=2.0)
    zbufs = z.rollout_begin(episode_limit=5, **BEGIN)
    zplan = _plan(z)
    zpred = z.plan_predict_begin(zplan, **begin)
    keep = {k: v.clone() for k, v in zplan.tensors().items()}
    zpred.human_vel.fill_(-7.0)
    assert z.plan_predict_orca_rollout(zplan, zpred, 0, counter, orca_mode=F['orca_mode'], **U) is zbufs  # no steps: a no-op
    assert bool((zpred.human_vel == -7.0).all()) and all(torch.equal(v, zplan.tensors()[k]) for k, v in keep.items())
    z.plan_predict_orca_rollout(zplan, zpred, 3, counter, orca_mode=F['orca_mode'], **U)
    z.plan_predict_orca_rollout(zplan, zpred, 3, counter + 3 * I, orca_mode=F['orca_mode'], **U)
    for a, b in zip(_snapshot(x), _snapshot(z)):
        assert torch.equal(a, b)
    assert torch.equal(zpred.human_vel, pred.human_vel)


def test_refusals_on_an_engine(amd):
    import ctypes as C
    import torch
    lib = amd._lib
    INV, UNS = lib.CN_ERR_INVALID, lib.CN_ERR_UNSUPPORTED
    two = dict(models=('cv', 'to_goal'))

    def refused(eng, plan, pred, status, *words, orca_mode=0):
        pred.human_vel.fill_(-7.0)
        eng.sync()
        counts, keep = eng.launch_counts(), {k: v.clone() for k, v in plan.tensors().items()}
        for name, args in (('cn_plan_cem_predict_orca_rollout', {}), ('cn_plan_mppi_predict_orca_rollout', dict(temperature=1.0))):
            with pytest.raises(amd.CrowdNavAmdError) as ei:
                eng.plan_predict_orca_rollout(plan, pred, 2, 3, orca_mode=orca_mode, **args)
            text = str(ei.value)
            assert ei.value.status == status and name in text and all(w in text for w in words), (name, text)
        eng.sync()
        assert eng.launch_counts() == counts and bool((pred.human_vel == -7.0).all())  # nothing enqueued, the table untouched
        for k, v in keep.items():
            assert torch.equal(v, plan.tensors()[k]), k

    # the engines no cn_plan_* call serves — cn_predict_orca itself serves both (test_predict_orca_moves_nothing_of_the_engine)
    orca = amd.BatchedCrowdSim(num_envs=B, num_humans=5, robot_policy=amd.ROBOT_ORCA)
    orca.rollout_begin(**BEGIN)
    plan = orca.plan_begin(5, 4, 2, 1, 0.3)
    for F in (dict(models='to_goal'), two):
        refused(orca, plan, orca.plan_predict_begin(plan, **F), INV, 'CN_ROBOT_EXTERNAL')
    uni = _engine(amd, 'h5', steps=0, robot_kinematics=1)
    uni.rollout_begin(**BEGIN)
    plan = uni.plan_begin(5, 4, 2, 1, 0.3)
    for F in (dict(models='to_goal'), two):
        refused(uni, plan, uni.plan_predict_begin(plan, **F), UNS, 'CN_UNICYCLE')
    # bootstrap with M = 2: the branch-end states are per mode
    from crowdnav_amd.compat.sarl import ValueNetwork, build_action_space
    boot = _engine(amd, 'h5', steps=0, robot_visible=1)
    boot.sarl_configure(actions=np.array([list(a) for a in build_action_space(1.0)[0]], dtype=np.float64))
    torch.manual_seed(7)
    boot.sarl_set_weights(ValueNetwork(13, 6, [150, 100], [100, 50], [150, 100, 100, 1], [100, 100, 1], True, 1.0, 4).state_dict())
    boot.rollout_begin(**BEGIN)
    plan = _plan(boot, bootstrap=True)
    refused(boot, plan, boot.plan_predict_begin(plan, **two), UNS, 'bootstrap', orca_mode=1)
    # the slot's model must still be one cn_predict knows; orca_mode against the struct's M (python checks it first: by hand)
    eng = _engine(amd, 'h5', steps=0)
    eng.rollout_begin(**BEGIN)
    plan = _plan(eng)
    pred = eng.plan_predict_begin(plan, **two)
    pred.c.model[1] = 4
    refused(eng, plan, pred, INV, 'model[1] = 4 unknown', orca_mode=1)
    pred.c.model[1] = lib.PREDICT_TO_GOAL
    L, io = lib.load(), eng._rollout[0]
    pred.human_vel.fill_(-7.0)
    assert L.cn_plan_cem_predict_orca_rollout(eng._h, C.byref(io), 2, C.byref(plan.cfg), C.byref(plan.c), C.byref(pred.c), 2, 0) == INV
    assert 'orca_mode = 2 is outside 0 .. n_modes - 1 = 1' in L.cn_last_error().decode()
    with pytest.raises(amd.CrowdNavAmdError, match='n_real_steps'):
        eng.plan_predict_orca_rollout(plan, pred, -1, 0)
    # cn_predict_orca on a live engine: the table's rows beyond an int; zero steps write nothing
    ptr = C.c_void_p(pred.human_vel.data_ptr())
    assert L.cn_predict_orca(eng._h, 2 ** 31 - 1, 8, 7, ptr) == UNS
    assert 'cn_predict_orca' in L.cn_last_error().decode() and 'rows exceed' in L.cn_last_error().decode()
    assert L.cn_predict_orca(eng._h, 0, 2, 1, ptr) == lib.CN_OK
    eng.sync()
    assert bool((pred.human_vel == -7.0).all())
    fresh = _engine(amd, 'h5', steps=0)
    fplan = _plan(fresh)
    with pytest.raises(RuntimeError, match='rollout_begin'):
        fresh.plan_predict_orca_rollout(fplan, fresh.plan_predict_begin(fplan, 'cv'), 1, 0)


# ------------------------------------------------------------------------------------------------ 6. the example
def test_the_example_takes_the_orca_future_with_and_without_the_device_loop(amd):
    """--futures to_goal,orca: the per-step loop (predict_orca per real step) and the one-call loop (plan_predict_orca_rollout, in
    chunks of 3) print the same line."""
    args = ['--futures', 'to_goal,orca', '--reduce', 'min', '--risk-penalty', '0.5']
    host = _example_line(args)
    got = _example_line(args + ['--device-loop', '--chunk', '3'])
    print(host)
    assert got == host
