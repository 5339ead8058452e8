"""cn_sarl_state_values and cn_lookahead_values on the MI355X: V of joint states the caller holds in the env layout, and the
lookahead that bootstraps its return with it.  The oracles are what exists already: sarl_transform rows through the torch module
(seeded random weights), sarl_select's exported buffers for the one-step case, cn_step loops for n steps, a twin engine for
"nothing moved".  Bounds against torch are the project's own for the kernel that runs: 2e-6 where the narrow kernel reads the
rows (test_values_of_caller_held_states_vs_torch), 2e-5 on the LDS, register and split-f16 kernels
(test_sarl_mlp_vs_torch_fp32_random_inputs, test_split_f16_vs_float64_on_random_networks)."""
import math

import numpy as np
import pytest
import torch

from support import (  # noqa: F401  (amd: module fixture)
    action_space as _space, amd, np_of as _np, restore as _restore, same_bits as _same_bits, snapshot as _snapshot,
    step_loop as _step_loop)

pytestmark = pytest.mark.gpu

DT, V_PREF, GAMMA = 0.25, 1.0, 0.9  # the engines' defaults (time_step, robot_v_pref) and sarl_configure's / cn_create's gamma
ROUTE_ENV = {'default': {}, 'lds': {'CROWDNAV_AMD_SARL_NARROW': '0'}, 'reg': {'CROWDNAV_AMD_SARL_REG': '2'}}

_NETS = {}


def _net(model, seed=7):
    """(torch module with seeded random weights, sarl_configure keywords) of a model at the shipped widths; built once."""
    if (model, seed) not in _NETS:
        from crowdnav_amd.compat import cadrl, lstm_rl
        from crowdnav_amd.compat.sarl import ValueNetwork
        torch.manual_seed(seed)
        if model == 'sarl':
            made = ValueNetwork(13, 6, [150, 100], [100, 50], [150, 100, 100, 1], [100, 100, 1], True, 1.0, 4), {}
        elif model == 'cadrl':
            made = cadrl.ValueNetwork(13, [150, 100, 100, 1]), dict(model='cadrl', mlp3_dims=(150, 100, 100, 1))
        elif model == 'lstm_rl':
            made = (lstm_rl.ValueNetwork1(13, 6, [150, 100, 100, 1], 50),
                    dict(model='lstm_rl', mlp1_dims=(50, 1), mlp3_dims=(150, 100, 100, 1)))
        else:
            made = (lstm_rl.ValueNetwork2(13, 6, [150, 100, 100, 50], [150, 100, 100, 1], 50),
                    dict(model='lstm_rl', mlp1_dims=(50, 1), mlp3_dims=(150, 100, 100, 1), interaction_dims=(150, 100, 100, 50)))
        _NETS[(model, seed)] = made
    return _NETS[(model, seed)]


def _torch_values(model, rows, on_device):
    """The torch module on transform rows [n, H, 13] -> float32 [n]; cadrl.ValueNetwork: the minimum over the pairs."""
    net = _net(model)[0]
    rows = rows if on_device else rows.cpu()
    net = net.to(rows.device)
    n, H = rows.shape[:2]
    with torch.no_grad():
        if model == 'cadrl':
            out = net(rows.reshape(n * H, 13)).reshape(n, H).min(dim=1).values
        else:
            out = net(rows).reshape(n)
    net.cpu()
    return out.cpu().numpy()


def _engine(amd, B, H, model='sarl', unicycle=False, weights=True, precision='f32', **cfg):
    eng = amd.BatchedCrowdSim(num_envs=B, num_humans=H, robot_policy=amd.ROBOT_EXTERNAL, robot_visible=1,
                              robot_kinematics=1 if unicycle else 0, **cfg)
    net, kw = _net(model)
    eng.sarl_configure(actions=_space(unicycle), precision=precision, **kw)
    if weights:
        eng.sarl_set_weights(net.state_dict())
    return eng


def _bound_and_oracle(eng, model):
    """(bound, torch on the device?) for the kernel sarl_state_values runs on this engine: the narrow kernel reads caller rows
    for every model but CADRL, which runs the one-tile LDS kernel there."""
    narrow_rows = eng.sarl_network_route() == 'narrow' and model != 'cadrl'
    return (2e-6, True) if narrow_rows else (2e-5, False)


CASES = ([('sarl', h, 0) for h in (1, 3, 5, 8)] + [('cadrl', h, 0) for h in (1, 5)] +
         [('lstm_rl', h, s) for h in (3, 5) for s in (0, 1)] + [('lstm_rl2', 5, 0)])


@pytest.mark.parametrize('route', sorted(ROUTE_ENV))
@pytest.mark.parametrize('model,H,sort', CASES)
def test_rows_and_values_against_transform_and_torch(amd, monkeypatch, model, H, sort, route):
    for k, v in ROUTE_ENV[route].items():
        monkeypatch.setenv(k, v)
    B = 7
    eng = _engine(amd, B, H, model)
    got_route = eng.sarl_network_route()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    narrow_fits = model != 'lstm_rl2' and -(-B * 81 // (16 // H)) <= cus  # at most one narrow tile per compute unit
    if route == 'default':
        assert got_route == ('narrow' if narrow_fits else got_route) and got_route in ('narrow', 'lds_tile', 'lds_chunked')
    elif route == 'lds':
        assert got_route in ('lds_tile', 'lds_chunked')
    else:
        assert got_route == {'sarl': 'reg_sarl' if H <= 5 else 'reg_sarl_chunk', 'cadrl': 'reg_cadrl', 'lstm_rl': 'reg_lstm',
                             'lstm_rl2': 'reg_lstm2'}[model]
    eng.reset(1000 + np.arange(B))
    for _ in range(2):  # velocities are non-zero
        eng.step(np.tile([0.3, 0.4], (B, 1)), update=True, want_obs=False)
    state8, _ = eng.get_state()
    rows = eng.sarl_transform(sort_humans=bool(sort))
    bound, on_device = _bound_and_oracle(eng, model)
    want = _torch_values(model, rows, on_device)
    got = _np(eng.sarl_state_values(state8, sort_humans=bool(sort)))
    err = float(np.abs(got - want).max())
    print('%s H %d sort %d route %s: max |V - torch| %.3g (bound %.0e)' % (model, H, sort, got_route, err, bound))
    assert got.dtype == np.float32 and got.shape == (B,)
    assert err <= bound
    if sort:  # the order matters to the network: env order gives other values somewhere
        assert not np.array_equal(got, _np(eng.sarl_state_values(state8, sort_humans=False)))
    eng.close()


def test_split_f16_engine(amd, monkeypatch):
    monkeypatch.setenv('CROWDNAV_AMD_SARL_NARROW', '0')
    B, H = 7, 5
    eng = _engine(amd, B, H, precision='f16x2')
    assert eng.sarl_network_route() == 'split_f16'
    eng.reset(1000 + np.arange(B))
    for _ in range(2):
        eng.step(np.tile([0.3, 0.4], (B, 1)), update=True, want_obs=False)
    state8, _ = eng.get_state()
    want = _torch_values('sarl', eng.sarl_transform(), False)
    got = _np(eng.sarl_state_values(state8))
    print('split_f16: max |V - torch| %.3g' % float(np.abs(got - want).max()))
    assert np.abs(got - want).max() <= 2e-5
    eng.close()


@pytest.mark.parametrize('route', sorted(ROUTE_ENV))
def test_passes_and_tile_slots_do_not_matter(amd, monkeypatch, route):
    for k, v in ROUTE_ENV[route].items():
        monkeypatch.setenv(k, v)
    src = _engine(amd, 7, 5)
    src.reset(2000 + np.arange(7))
    for _ in range(2):
        src.step(np.tile([0.3, 0.4], (7, 1)), update=True, want_obs=False)
    pool, _ = src.get_state()
    eng = _engine(amd, 3, 5)  # never reset: 3 x 81 = 243 groups per pass
    assert eng.sarl_network_route() == {'default': 'narrow', 'lds': 'lds_tile', 'reg': 'reg_sarl'}[route]
    pool = pool.to(eng.device)
    ref = _np(eng.sarl_state_values(pool))
    assert len(set(ref.tolist())) == 7  # distinct states
    for n in (1, 15, 16, 17, 243, 244, 500):
        states = pool[torch.arange(n, device=pool.device) % 7].contiguous()
        got = _np(eng.sarl_state_values(states))
        assert _same_bits(got, ref[np.arange(n) % 7]), (route, n)
    eng.close()


def _every_action(B):
    acts = _space()
    return acts, torch.from_numpy(np.ascontiguousarray(np.broadcast_to(acts[None, :, None, :], (B, 81, 1, 2)))).cuda()


@pytest.mark.parametrize('H', [2, 5])
def test_one_step_is_the_decision(amd, H):
    """Holonomic: lookahead(bootstrap=True) over the 81-action table, one step, evaluates the rows sarl_select evaluates, with
    the same kernel: V, reward and reward + gamma V have sarl_select's bits."""
    B = 3
    eng = _engine(amd, B, H)
    eng.reset(3000 + np.arange(B))
    for _ in range(2):
        eng.step(np.tile([0.0, 0.5], (B, 1)), update=True, want_obs=False)
    state, gtime = (_np(x).copy() for x in eng.get_state())
    state[0, 0, 0:2] = state[0, 0, 4:6] - np.array([0.0, 0.4])              # a step short of its goal
    state[1, 0, 0:2] = state[1, 1, 0:2] + np.array([0.75, 0.0])             # 0.15 m clear of human 0 (radii 0.3 + 0.3)
    eng.set_state(state, gtime)
    sel = eng.sarl_select()
    V, reward, values = _np(eng.sarl_export('V')), _np(eng.sarl_export('reward')), _np(sel['values'])
    acts, table = _every_action(B)
    look = {k: _np(v) for k, v in eng.lookahead(table, bootstrap=True).items()}
    ended = look['info'] >= amd.REACH_GOAL
    print('H %d: ended %d of %d branches, info codes %s' % (H, ended.sum(), ended.size, np.unique(look['info']).tolist()))
    assert ended.any() and (~ended).any()
    assert (look['info'][0] == amd.REACH_GOAL).any() and (look['info'][1] == amd.COLLISION).any()
    assert (look['steps'] == 1).all()
    assert _same_bits(look['value'], V.reshape(B, 81))
    assert _same_bits(look['ret'], reward)
    host = look['ret'] + math.pow(GAMMA, 1 * DT * V_PREF) * look['value'].astype(np.float64)
    assert _same_bits(host, values)
    assert _same_bits(look['score'][~ended], values[~ended])
    assert _same_bits(look['score'][ended], look['ret'][ended])
    eng.close()


def _bootstrap_against_the_step_loop(amd, eng, table, snap, unicycle):
    """lookahead(bootstrap=True) from `snap` against, per candidate, the snapshot put back and stepped by cn_step."""
    B, K, n = table.shape[:3]
    _restore(eng, snap)
    look = eng.lookahead(table, bootstrap=True)
    direct = _np(eng.sarl_state_values(look['final_state8'], theta=look['final_theta'] if unicycle else None))
    look = {k: _np(v) for k, v in look.items()}
    assert sorted(look) == ['final_state8', 'final_theta', 'info', 'ret', 'score', 'steps', 'time', 'value']
    assert _same_bits(look['value'], direct.reshape(B, K))
    bound, on_device = _bound_and_oracle(eng, 'sarl')
    for k in range(K):
        _restore(eng, snap)
        want = _step_loop(eng, table[:, k])
        for key, ref in want.items():
            assert _same_bits(look[key][:, k], ref), (key, k, look[key][:, k], ref)
        eng.set_state(want['final_state8'], want['time'])
        eng.set_theta(want['final_theta'])
        v = _torch_values('sarl', eng.sarl_transform(sort_humans=False), on_device)
        err = float(np.abs(look['value'][:, k] - v).max())
        print('candidate %d: steps %s info %s max |V - torch| %.3g' % (k, want['steps'].tolist(), want['info'].tolist(), err))
        assert err <= bound
    ended = look['info'] >= amd.REACH_GOAL
    for b in range(B):
        for k in range(K):
            boot = math.pow(GAMMA, int(look['steps'][b, k]) * DT * V_PREF) * float(np.float64(look['value'][b, k]))
            want = look['ret'][b, k] if ended[b, k] else look['ret'][b, k] + boot
            assert _same_bits(look['score'][b, k], np.float64(want)), (b, k)
    return look, ended


def test_n_steps(amd):
    B, H, K, n = 3, 5, 4, 6
    eng = _engine(amd, B, H, time_limit=3.0)  # 12-step episodes
    eng.reset(4000 + np.arange(B))
    for _ in range(2):
        eng.step(np.tile([0.0, 0.5], (B, 1)), update=True, want_obs=False)
    state, _ = eng.get_state()
    eng.set_state(state, np.array([1.0, 0.0, 1.25]))  # envs 0 and 2 run out of time inside the horizon, env 1 does not
    snap = _snapshot(eng)
    acts = _space()
    table = acts[np.random.RandomState(5).randint(len(acts), size=(B, K, n))]
    look, ended = _bootstrap_against_the_step_loop(amd, eng, table, snap, False)
    assert (look['info'] == amd.TIMEOUT).any() and (~ended).any()
    assert ((look['info'] == amd.TIMEOUT) & (look['steps'] > 1) & (look['steps'] < n)).any()  # (global_time >= time_limit - 1)
    eng.close()


def test_unicycle(amd):
    B, H, K, n = 2, 5, 3, 6
    eng = _engine(amd, B, H, unicycle=True)
    assert len(_space(True)) == 26
    eng.reset(5000 + np.arange(B))
    for _ in range(3):
        eng.step(np.tile([0.5, 0.3], (B, 1)), update=True, want_obs=False)  # (v, r): the heading turns
    state8, _ = eng.get_state()
    theta = eng.get_theta()
    assert (_np(theta) != math.pi / 2).all()
    bound, on_device = _bound_and_oracle(eng, 'sarl')
    want = _torch_values('sarl', eng.sarl_transform(sort_humans=False), on_device)
    got = _np(eng.sarl_state_values(state8, theta))
    assert np.abs(got - want).max() <= bound
    assert not np.array_equal(got, _np(eng.sarl_state_values(state8, theta + 0.5)))  # the heading is read
    with pytest.raises(amd.CrowdNavAmdError, match='theta') as ei:
        eng.sarl_state_values(state8)
    assert ei.value.status == amd._lib.CN_ERR_INVALID
    acts = _space(True)
    table = acts[np.random.RandomState(6).randint(len(acts), size=(B, K, n))]
    look, _ = _bootstrap_against_the_step_loop(amd, eng, table, _snapshot(eng), True)
    assert (look['final_theta'] != _np(theta)[:, None]).any()
    eng.close()


def test_nothing_moved(amd):
    B, H, K, n, advance, after = 3, 5, 3, 6, 5, 10
    acts = _space()
    table = acts[np.random.RandomState(8).randint(len(acts), size=(B, K, n))]
    drive = torch.from_numpy(acts[np.random.RandomState(9).randint(len(acts), size=(B, advance + after))]).cuda()
    begin = dict(seed_base=1000, seed_mod=500, record_capacity=8)
    y, x = _engine(amd, B, H, time_limit=8.0), _engine(amd, B, H, time_limit=8.0)
    ybufs, xbufs = y.rollout_begin(**begin), x.rollout_begin(**begin)
    for t in range(advance):
        y.rollout_step(drive[:, t].contiguous())
        x.rollout_step(drive[:, t].contiguous())
    snap = _snapshot(y)
    io_before = {k: v.clone() for k, v in ybufs.items()}
    counts_before = y.launch_counts()
    look = y.lookahead(table, bootstrap=True)
    y.sync()
    assert torch.isfinite(look['score']).all() and torch.isfinite(look['value']).all()
    for a, b in zip(snap, _snapshot(y)):
        assert torch.equal(a, b)
    for k, v in io_before.items():
        assert torch.equal(v, ybufs[k]), k
    counts = y.launch_counts()
    assert y.sarl_network_route() == 'narrow' and counts['sarl_narrow'] == counts_before['sarl_narrow'] + 1
    assert {k: v for k, v in counts.items() if k != 'sarl_narrow'} == {k: v for k, v in counts_before.items() if k != 'sarl_narrow'}
    for t in range(advance, advance + after):
        y.rollout_step(drive[:, t].contiguous())
        x.rollout_step(drive[:, t].contiguous())
    for a, b in zip(_snapshot(y), _snapshot(x)):
        assert torch.equal(a, b)
    for k, v in xbufs.items():
        assert torch.equal(v, ybufs[k]), k
    y.close(), x.close()


def test_gym_surface_scores_with_the_policy_s_network(amd, name='sarl'):
    """compat.CrowdSim.lookahead(sequences, policy): the 81 one-step sequences score what robot.act's decision holds in
    policy.action_values (reward + gamma V, the same bits) wherever the step does not end the episode; without a policy the
    call is the 3-tuple form."""
    import crowdnav_amd.compat as c
    from crowdnav_amd.compat.sarl import default_policy_config
    cfg = c.default_env_config({('robot', 'visible'): 'true'})
    env = c.CrowdSim()
    env.configure(cfg)
    robot = c.Robot(cfg, 'robot')
    policy = c.policy_factory[name]()
    policy.configure(default_policy_config({}))
    torch.manual_seed(11)
    for p in policy.get_model().parameters():
        torch.nn.init.normal_(p, std=0.1)
    robot.set_policy(policy)
    env.set_robot(robot)
    policy.set_phase('test')
    policy.set_device(torch.device('cpu'))
    policy.set_env(env)
    ob = env.reset('test', 1)
    for _ in range(3):
        ob, _, done, _ = env.step(robot.act(ob))
        assert not done
    robot.act(ob)
    values = list(policy.action_values)
    sequences = [[a] for a in policy.action_space]
    scored = env.lookahead(sequences, policy=policy)
    plain = env.lookahead(sequences)
    assert len(scored) == len(plain) == len(values) == 81
    running = 0
    for (ret, info, steps, score), (ret3, info3, steps3), value in zip(scored, plain, values):
        assert (ret, type(info), steps) == (ret3, type(info3), steps3) and steps == 1
        if isinstance(info, (c.ReachGoal, c.Collision, c.Timeout)):
            assert score == ret
        else:
            assert score == value
            running += 1
    assert running > 40


def test_refusals_on_an_engine(amd):
    lib = amd._lib
    B, H = 2, 5
    state8 = torch.zeros((B, H + 1, 8), dtype=torch.float64, device='cuda')
    acts, _ = _every_action(B)
    table = np.ascontiguousarray(np.broadcast_to(acts[None, :3, None, :], (B, 3, 1, 2)))

    def refused(eng, status, word):
        for call in (lambda: eng.sarl_state_values(state8), lambda: eng.lookahead(table, bootstrap=True)):
            with pytest.raises(amd.CrowdNavAmdError, match=word) as ei:
                call()
            assert ei.value.status == status

    bare = amd.BatchedCrowdSim(num_envs=B, num_humans=H, robot_policy=amd.ROBOT_EXTERNAL, robot_visible=1)
    refused(bare, lib.CN_ERR_INVALID, 'configure and set weights first')
    refused(_engine(amd, B, H, weights=False), lib.CN_ERR_INVALID, 'configure and set weights first')
    from crowdnav_amd.compat.sarl import ValueNetwork
    om = amd.BatchedCrowdSim(num_envs=B, num_humans=H, robot_policy=amd.ROBOT_EXTERNAL, robot_visible=1)
    om.sarl_configure(actions=_space(), with_om=True)
    om.sarl_set_weights(ValueNetwork(61, 6, [150, 100], [100, 50], [150, 100, 100, 1], [100, 100, 1], True, 1.0, 4).state_dict())
    refused(om, lib.CN_ERR_UNSUPPORTED, 'occupancy maps')
    refused(_engine(amd, B, H, scenario_rule=2), lib.CN_ERR_UNSUPPORTED, 'mixed rule')
    eng = _engine(amd, B, H)
    with pytest.raises(amd.CrowdNavAmdError) as ei:
        eng.sarl_state_values(state8[:0])
    assert ei.value.status == lib.CN_ERR_INVALID
    # n_steps = 0: CN_OK, the tensors come back unwritten
    first = eng.lookahead(table, bootstrap=True)
    # the bootstrap's own arguments, behind cn_lookahead_actions' checks: final_state8, value, score
    import ctypes as C
    ptr = {k: v.data_ptr() for k, v in first.items()}
    rows = {k: ptr[k] for k in ('ret', 'info', 'steps', 'time', 'final_state8', 'final_theta')}
    dev_table = torch.from_numpy(table).cuda()
    for missing, word in (('final_state8', 'out->final_state8'), ('value', 'value is NULL'), ('score', 'score is NULL')):
        out = lib.CnLookaheadOut(**{k: (None if k == missing else v) for k, v in rows.items()})
        value, score = (None if missing == k else C.c_void_p(ptr[k]) for k in ('value', 'score'))
        rc = eng._lib.cn_lookahead_values(eng._h, 1, 3, C.c_void_p(dev_table.data_ptr()), C.byref(out), 0, value, score)
        assert rc == lib.CN_ERR_INVALID and word in eng._lib.cn_last_error().decode(), (missing, eng._lib.cn_last_error())
    for v in first.values():
        v.fill_(7)
    again = eng.lookahead(table[:, :, :0], out=first, bootstrap=True)
    eng.sync()
    assert sorted(again) == sorted(first)
    for k, v in again.items():
        assert v.data_ptr() == first[k].data_ptr() and bool((v == 7).all()), k
