"""SARL's attention weights on the device path (cn_sarl_select_attention, ABI v12): every value-network route writes the
softmax weights it already holds, [B][n_actions][H]; compat's SARL keeps env 0's row of the LAST action, which is what the
reference's last forward of MultiHumanRL.predict leaves for get_attention_weights() (sarl.py:54, 88-89;
multi_human_rl.py:35-51) and CrowdSim.step records (crowd_sim.py:396-397).  tests/golden/sarl_attention.npz comes from the
unmodified reference (scripts/gen_golden_attention.py)."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from sarl_attention_cases import check as _check
from support import value_network as _net

FIXTURES = ('plain', 'om', 'h12', 'mixed')


def _fixture_net(g, name):
    prefix = 'om_param_' if int(g[name + '_with_om']) else 'param_'
    net = _net(g[name + '_x_last'].shape[2])
    net.load_state_dict({k[len(prefix):]: torch.from_numpy(v) for k, v in g.items() if k.startswith(prefix)})
    return net


def _parked_states(states):
    """fixture rows padded with NaN -> the engine's representation: absent humans parked at rest far away, behind the present
    ones (as tests/test_mixed.py does)"""
    s = states.copy()
    for b in range(len(s)):
        for i in range(1, s.shape[1]):
            if np.isnan(s[b, i, 0]):
                x = 1.0e6 + 100.0 * i
                s[b, i] = [x, 1.0e6, 0.0, 0.0, x, 1.0e6, 0.3, 1.0]
    return s


# ---- CPU ---------------------------------------------------------------------------------------------------------------
def test_binding_declares_select_attention_abi12():
    from crowdnav_amd import _lib
    assert _lib.ABI_VERSION == 12
    assert _lib.SYMBOLS['cn_sarl_select_attention'][1] == [_lib._P] * 5


@pytest.mark.parametrize('name', FIXTURES)
def test_mirror_reproduces_reference_attention_of_the_last_action_cpu(name):
    """The torch mirror on the reference's input of its last forward gives the weights CrowdSim recorded at that step: the
    recorded row IS the last action's lookahead state (and the fixture pins that to the reference's own loop)."""
    g = load_golden('sarl_attention.npz')
    net = _fixture_net(g, name)
    count, x, want = g[name + '_count'], g[name + '_x_last'], g[name + '_attention']
    assert len(count) >= 4
    if name == 'mixed':
        assert count.max() < 5 and count.min() == 1
    for t in range(len(count)):
        n = int(count[t])
        with torch.no_grad():
            net(torch.from_numpy(x[t][None, :n]))
        got = net.attention_weights
        assert got.shape == (n,) and np.abs(got - want[t][:n]).max() <= 1e-6
        assert np.isnan(want[t][n:]).all()


# ---- GPU: every route ----------------------------------------------------------------------------------------------
def _engine(humans, B, with_om, seed=3000, radius=None):
    import crowdnav_amd
    kw = dict(circle_radius=radius) if radius else {}
    eng = crowdnav_amd.BatchedCrowdSim(num_envs=B, num_humans=humans, robot_policy=crowdnav_amd.ROBOT_EXTERNAL, robot_visible=1,
                                       **kw)
    eng.reset(seed + np.arange(B))
    eng.step(np.zeros((B, 2)), update=True)
    return eng


ROUTES = {  # (CROWDNAV_AMD_SARL_REG, CROWDNAV_AMD_SARL_NARROW), the launch counter of the narrow route
    'reg': ('2', '0'), 'reg-chunk': ('2', '0'), 'pipe': ('0', '0'), 'lds-chunked': ('0', '0'), 'narrow': ('0', '2'),
}


@pytest.mark.gpu
@pytest.mark.parametrize('route,humans,B,with_om', [
    ('reg', 1, 7, False), ('reg', 3, 7, False), ('reg', 3, 7, True), ('reg', 5, 7, False), ('reg', 5, 7, True),
    ('reg-chunk', 6, 7, False), ('reg-chunk', 9, 7, True), ('reg-chunk', 13, 7, False),
    ('pipe', 5, 7, False), ('pipe', 5, 7, True), ('pipe', 8, 5, False),
    ('lds-chunked', 9, 5, False), ('lds-chunked', 20, 3, False),
    ('narrow', 5, 1, False), ('narrow', 5, 1, True), ('narrow', 5, 3, False), ('narrow', 5, 3, True), ('narrow', 3, 2, False),
])
def test_select_attention_matches_the_torch_mirror(route, humans, B, with_om, monkeypatch):
    from crowdnav_amd.compat.sarl import build_action_space
    reg, narrow = ROUTES[route]
    monkeypatch.setenv('CROWDNAV_AMD_SARL_REG', reg)
    monkeypatch.setenv('CROWDNAV_AMD_SARL_NARROW', narrow)
    torch.manual_seed(100 + humans)
    net = _net(61 if with_om else 13)
    eng = _engine(humans, B, with_om, radius=6.0 if humans > 8 else None)
    space, _, _ = build_action_space(1.0)
    eng.sarl_configure(actions=np.array([[a.vx, a.vy] for a in space]), with_om=with_om)
    eng.sarl_set_weights(net.state_dict())
    _check(eng, net)
    assert eng.launch_counts()['sarl_narrow'] == (2 if route == 'narrow' else 0)  # (two selects)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize('kernels', ['pipe', 'reg', 'narrow'])
def test_select_attention_masks_the_absent_humans_of_a_mixed_episode(kernels, monkeypatch):
    import crowdnav_amd
    reg, narrow = ROUTES[kernels]
    monkeypatch.setenv('CROWDNAV_AMD_SARL_REG', reg)
    monkeypatch.setenv('CROWDNAV_AMD_SARL_NARROW', narrow)
    g = load_golden('mixed_sarl.npz')
    states = _parked_states(g['sarl_states'])
    eng = crowdnav_amd.BatchedCrowdSim(num_envs=len(states), num_humans=5, robot_policy=crowdnav_amd.ROBOT_EXTERNAL,
                                       robot_visible=1, scenario_rule=crowdnav_amd.MIXED)
    eng.set_state(states, g['sarl_gtime'])
    net = _net(13)
    net.load_state_dict({k[len('sarl_param_'):]: torch.from_numpy(v) for k, v in g.items() if k.startswith('sarl_param_')})
    eng.sarl_configure(actions=g['sarl_action_space'], gamma=0.9)
    eng.sarl_set_weights(net.state_dict())
    att = _check(eng, net, counts=g['sarl_count'])
    assert eng.launch_counts()['sarl_narrow'] == (2 if kernels == 'narrow' else 0)
    assert (att[g['sarl_count'] == 1][:, :, 0] == 1).all()


@pytest.mark.gpu
@pytest.mark.parametrize('model', ['cadrl', 'lstm_rl'])
def test_select_attention_is_unsupported_without_attention(model):
    import crowdnav_amd
    import crowdnav_amd.compat as c
    from crowdnav_amd import _lib
    from crowdnav_amd.compat.sarl import build_action_space, default_policy_config
    eng = _engine(5, 2, False)
    space, _, _ = build_action_space(1.0)
    cfg = dict(model='cadrl', mlp3_dims=(150, 100, 100, 1)) if model == 'cadrl' else \
        dict(model='lstm_rl', mlp1_dims=(50, 1), mlp3_dims=(150, 100, 100, 1))
    eng.sarl_configure(actions=np.array([[a.vx, a.vy] for a in space]), **cfg)
    policy = c.policy_factory[model]()
    policy.configure(default_policy_config())
    eng.sarl_set_weights(policy.get_model().state_dict())
    with pytest.raises(crowdnav_amd.CrowdNavAmdError) as ei:
        eng.sarl_select(want_attention=True)
    assert ei.value.status == _lib.CN_ERR_UNSUPPORTED
    assert eng.sarl_select()['best'].shape == (2,)  # the engine is still usable
    assert not hasattr(policy, 'get_attention_weights')
    eng.close()


# ---- GPU: the reference's drop-in surface ---------------------------------------------------------------------------
def _setup(g, name, device='cpu'):
    import crowdnav_amd.compat as c
    from crowdnav_amd.compat.sarl import default_policy_config
    with_om, humans = bool(int(g[name + '_with_om'])), g[name + '_states'].shape[1] - 1
    ov = {('robot', 'visible'): 'true', ('sim', 'human_num'): humans}
    if name == 'mixed':
        ov[('sim', 'test_sim')] = 'mixed'
    cfg = c.default_env_config(ov)
    env = c.CrowdSim()
    env.configure(cfg)
    robot = c.Robot(cfg, 'robot')
    policy = c.policy_factory['sarl']()
    policy.configure(default_policy_config({('sarl', 'with_om'): 'true' if with_om else 'false'}))
    policy.get_model().load_state_dict(_fixture_net(g, name).state_dict())
    robot.set_policy(policy)
    env.set_robot(robot)
    policy.set_phase('test')
    policy.set_device(torch.device(device))
    policy.set_env(env)
    return env, robot, policy


def _episodes(g, name):
    case = g[name + '_case']
    for c_ in sorted(set(case.tolist()), key=case.tolist().index):
        yield c_, np.nonzero(case == c_)[0]


def _at(env, g, name, t):
    """the reference's exact state before decision t (absent humans of a `mixed` episode parked behind)"""
    s = g[name + '_states'][t:t + 1]
    env._eng.set_state(_parked_states(s) if name == 'mixed' else s, g[name + '_gtime'][t:t + 1])
    env._pull()
    return [h.get_observable_state() for h in env.humans]


@pytest.mark.gpu
@pytest.mark.parametrize('name', FIXTURES)
def test_crowd_sim_records_the_reference_attention_weights(name):
    """env.reset / robot.act (SARL.predict on the device) / env.step as the reference loop: env.attention_weights[t] is the
    reference's at every step, trimmed to the episode's humans under the `mixed` rule."""
    g = load_golden('sarl_attention.npz')
    env, robot, policy = _setup(g, name)
    for case, steps in _episodes(g, name):
        env.reset('test', int(case))
        assert len(env.humans) == g[name + '_count'][steps[0]] and env.attention_weights == []
        for i, t in enumerate(steps):
            assert g[name + '_step'][t] == i
            ob = _at(env, g, name, t)
            action = robot.act(ob)
            env.step(action)
            got, want = env.attention_weights[-1], g[name + '_attention'][t]
            n = int(g[name + '_count'][t])
            assert isinstance(got, np.ndarray) and got.shape == (n,)
            assert np.abs(got - want[:n]).max() <= 1e-6
            assert policy.get_attention_weights() is got
        assert len(env.attention_weights) == len(steps)


@pytest.mark.gpu
def test_a_torch_forward_after_a_decision_wins_again():
    """After a device decision get_attention_weights() is the decision's row; after a Trainer step (a replayed graph on the
    device, or an eager step) it is the torch forward's row 0 again, as in the reference; the next decision takes over."""
    from crowdnav_amd.compat.trainer import DeviceReplayMemory, Trainer
    g = load_golden('sarl_attention.npz')
    env, robot, policy = _setup(g, 'plain', device='cuda')
    env.reset('test', int(g['plain_case'][0]))
    robot.act(_at(env, g, 'plain', 0))
    first = policy.get_attention_weights()
    assert np.abs(first - g['plain_attention'][0]).max() <= 1e-6
    torch.manual_seed(0)
    mem = DeviceReplayMemory(16, device='cuda')
    mem.push_batch(torch.rand(16, 5, 13), torch.rand(16))
    tr = Trainer(policy.get_model(), mem, torch.device('cuda'), batch_size=8)
    tr.set_learning_rate(0.001)
    for rnd in range(2):  # the first call captures the SGD step, the second replays it
        tr.optimize_batch(1)
        torch.cuda.synchronize()
        got = policy.get_attention_weights()
        want = policy.get_model()._attention_row.cpu().numpy()
        assert got.shape == (5,) and np.array_equal(got, want)
        assert not np.array_equal(got, first)
        robot.act(_at(env, g, 'plain', 1 + rnd))
        assert policy.get_attention_weights().shape == (5,)
        assert not np.array_equal(policy.get_attention_weights(), want)
