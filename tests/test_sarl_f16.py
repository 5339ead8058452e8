"""CN_PRECISION_F16X2 on the device: sarl_f16_kernel (split-f16 matrix instructions) behind
sarl_configure(precision='f16x2').  Small batches leave the narrow tiles through CROWDNAV_AMD_SARL_NARROW=0, so that the
configuration's fp32 route is the one-tile LDS kernel, which the split route replaces; sarl_network_route() proves it ran.

Bounds.  Against the reference's fixtures: those of tests/test_sarl.py for the fp32 kernels (V and values 1e-6, arg-max equal
where the reference's top-2 gap exceeds 4e-5).  On random networks the truth is the torch module in float64 on the exported
X, and the split route's error must stay within max(8 x the fp32 route's error on the same state, 2^-20) — factor and floor
of the device SGD step's bound (tests/test_train_step.py): the split drops terms of 2^-22 relative per product, an fp32 product rounds at 2^-24, sums of
~100 such terms in another order differ by a few units of either."""
import logging

import numpy as np
import pytest
import torch

from conftest import load_golden, report_argmax
from support import value_network as _net

pytestmark = pytest.mark.gpu

# fixture -> (engine keywords, sarl_configure keywords, reward tolerance: that of the fixture's own fp32 test — the unicycle
# end point goes through device cos / sin)
FIVE_HUMAN_FIXTURES = {
    'sarl_plain': (dict(), dict(), 0),
    'sarl_om': (dict(), dict(with_om=True), 0),
    'sarl_unicycle': (dict(robot_visible=1, unicycle=True), dict(), 1e-12),
    'sarl_noquery_om': (dict(robot_visible=1), dict(with_om=True, query_env=False), 0),
    'sarl_noquery_unicycle': (dict(robot_visible=0, unicycle=True), dict(query_env=False), 1e-12),
}


@pytest.fixture(autouse=True)
def _leave_the_narrow_tiles(monkeypatch):
    monkeypatch.setenv('CROWDNAV_AMD_SARL_NARROW', '0')


def _actions():
    from crowdnav_amd.compat.sarl import build_action_space
    space, _, _ = build_action_space(1.0)
    return np.array([[a.vx, a.vy] for a in space])


def _engine(humans, B, seed=1000, **kw):
    import crowdnav_amd
    eng = crowdnav_amd.BatchedCrowdSim(num_envs=B, num_humans=humans, robot_policy=crowdnav_amd.ROBOT_EXTERNAL, robot_visible=1, **kw)
    eng.reset(seed + np.arange(B))
    eng.step(np.zeros((B, 2)), update=True)  # humans get non-zero velocities
    return eng


@pytest.mark.parametrize('name', sorted(FIVE_HUMAN_FIXTURES))
def test_split_f16_select_vs_reference(name):
    import crowdnav_amd
    eng_kw, cfg_kw, reward_tol = FIVE_HUMAN_FIXTURES[name]
    g = load_golden(name + '.npz')
    n = len(g['states'])
    with_om = bool(cfg_kw.get('with_om'))
    assert with_om == bool(int(g['with_om'])) and g['states'].shape[1] - 1 == 5
    eng_kw = dict(eng_kw)
    kin = dict(robot_kinematics=crowdnav_amd.UNICYCLE) if eng_kw.pop('unicycle', False) else {}
    eng = crowdnav_amd.BatchedCrowdSim(num_envs=n, num_humans=5, robot_policy=crowdnav_amd.ROBOT_EXTERNAL,
                                       robot_visible=eng_kw.get('robot_visible', int(g['robot_visible'])), **kin)
    eng.set_state(g['states'], g['gtime'])
    if kin:
        eng.set_theta(g['theta'])
    eng.sarl_configure(actions=g['action_space'], gamma=0.9, precision='f16x2', **cfg_kw)
    assert eng.sarl_network_route() == 'split_f16'
    net = _net(61 if with_om else 13)
    net.load_state_dict({k[len('param_'):]: torch.from_numpy(v) for k, v in g.items() if k.startswith('param_')})
    eng.sarl_set_weights(net.state_dict())
    out = eng.sarl_select()
    eng.sync()
    cpu = lambda t: t.cpu().numpy()  # noqa: E731
    if reward_tol == 0:
        assert np.array_equal(cpu(eng.sarl_export('reward')), g['rewards'])  # float64 lookahead: exact
    else:
        assert np.abs(cpu(eng.sarl_export('reward')) - g['rewards']).max() <= reward_tol
    assert np.array_equal(cpu(eng.sarl_export('next_obs')), g['next_obs'])
    X = cpu(eng.sarl_export('X'))
    assert X.shape == g['inputs'].shape
    assert np.abs(X - g['inputs']).max() <= 5e-6
    if with_om:
        assert np.abs(cpu(eng.sarl_export('om')) - g['inputs'][:, 0, :, 13:]).max() <= 5e-6
    V = cpu(eng.sarl_export('V'))
    print('%s: max |V - net_out| = %.3g' % (name, np.abs(V - g['net_out']).max()))
    assert np.abs(V - g['net_out']).max() <= 1e-6
    values = cpu(out['values'])
    assert np.abs(values - g['values']).max() <= 1e-6
    best = cpu(out['best'])
    top2 = np.sort(g['values'], axis=1)[:, -2:]
    report_argmax(name, best, g['best'], g['values'], route='split_f16')
    clear = (top2[:, 1] - top2[:, 0]) > 4e-5
    assert clear.sum() >= n // 4
    assert np.array_equal(best[clear], g['best'][clear])
    assert np.array_equal(cpu(out['action'])[clear], g['action'][clear])
    # wherever the arg-max differs it is a numerical tie: the value picked is within tolerance of the maximum
    assert np.all(g['values'][np.arange(n), best] >= g['values'].max(axis=1) - 4e-5)
    eng.close()


def _errors(humans, B, with_om, net, seed=1000):
    """(V of the split route, V of the fp32 route, torch fp32, torch float64) on the same engine state and exported X"""
    got = {}
    for precision in ('f16x2', 'f32'):
        eng = _engine(humans, B, seed)
        eng.sarl_configure(actions=_actions(), with_om=with_om, precision=precision)
        assert eng.sarl_network_route() == ('split_f16' if precision == 'f16x2' else 'lds_tile')
        eng.sarl_set_weights(net.state_dict())
        out = eng.sarl_select()
        got[precision] = (eng.sarl_export('V').cpu().numpy(), eng.sarl_export('X').cpu(), out['best'].cpu().numpy())
        eng.close()
    X = got['f16x2'][1]
    assert torch.equal(X, got['f32'][1])
    d = X.shape[-1]
    with torch.no_grad():
        v32 = net(X.reshape(B * 81, humans, d)).reshape(B, 81).numpy()
        net64 = _net(d).double()
        net64.load_state_dict({k: v.double() for k, v in net.state_dict().items()})
        v64 = net64(X.double().reshape(B * 81, humans, d)).reshape(B, 81).numpy()
    assert np.all(got['f16x2'][2] >= 0)
    return got['f16x2'][0], got['f32'][0], v32, v64


CASES = [(1, 37, False), (2, 37, False), (2, 37, True), (3, 37, False), (3, 37, True), (4, 37, False), (4, 37, True),
         (5, 37, False), (5, 37, True),      # 2997 groups: 188 tiles, the last one of 5 groups
         (5, 1, False), (3, 1, True),        # one env: 81 groups, 6 tiles, the last one of 1 group
         (5, 16, False), (2, 16, True)]      # exactly 81 tiles


@pytest.mark.parametrize('humans,B,with_om', CASES)
def test_split_f16_vs_float64_on_random_networks(humans, B, with_om):
    torch.manual_seed(3)
    net = _net(61 if with_om else 13)
    split, fp32, v32, v64 = _errors(humans, B, with_om, net)
    e_split, e_fp32 = np.abs(split - v64).max(), np.abs(fp32 - v64).max()
    print('H %d B %d om %d: E_split %.3g E_fp32 %.3g' % (humans, B, with_om, e_split, e_fp32))
    assert e_split <= max(8 * e_fp32, 2.0 ** -20)
    assert np.abs(split - v32).max() <= 2e-5


@pytest.mark.parametrize('humans,B,with_om', [(5, 37, False), (3, 37, True), (1, 16, False)])
def test_split_f16_vs_float64_with_larger_activations(humans, B, with_om):
    """mlp1.0's weights x 8: activations of tens instead of ones; the bound relative to the largest value"""
    torch.manual_seed(3)
    net = _net(61 if with_om else 13)
    with torch.no_grad():
        net.mlp1[0].weight.mul_(8.0)
    split, fp32, v32, v64 = _errors(humans, B, with_om, net)
    scale = np.abs(v64).max()
    e_split, e_fp32 = np.abs(split - v64).max() / scale, np.abs(fp32 - v64).max() / scale
    print('H %d B %d om %d: relative E_split %.3g E_fp32 %.3g (max |V| %.3g)' % (humans, B, with_om, e_split, e_fp32, scale))
    assert e_split <= max(8 * e_fp32, 2.0 ** -20)


@pytest.mark.parametrize('humans,B,with_om', [(1, 7, False), (3, 7, True), (5, 7, False), (5, 7, True)])
def test_split_f16_select_attention(humans, B, with_om):
    """values / best / action bit-identical to the plain split select; the weights within tests/test_sarl_attention.py's
    tolerance (1e-6) of the torch mirror on the exported X, summing to 1"""
    from sarl_attention_cases import check as _check
    torch.manual_seed(100 + humans)
    net = _net(61 if with_om else 13)
    eng = _engine(humans, B, seed=3000)
    eng.sarl_configure(actions=_actions(), with_om=with_om, precision='f16x2')
    assert eng.sarl_network_route() == 'split_f16'
    eng.sarl_set_weights(net.state_dict())
    _check(eng, net)
    assert eng.launch_counts()['sarl_narrow'] == 0
    eng.close()


def test_split_f16_is_deterministic():
    torch.manual_seed(5)
    net = _net(61)
    eng = _engine(5, 37)
    eng.sarl_configure(actions=_actions(), with_om=True, precision='f16x2')
    eng.sarl_set_weights(net.state_dict())
    runs = []
    for _ in range(2):
        out = eng.sarl_select()
        runs.append([eng.sarl_export('V').cpu().numpy()] + [out[k].cpu().numpy() for k in ('values', 'best', 'action')])
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
    eng.close()


def test_split_f16_activation_beyond_the_f16_range_ends_as_no_finite_value():
    """The documented limit: an activation above 65504 becomes +inf / -inf in the split, every value it feeds NaN, and the
    decision best = -2 (no finite value) — never a wrong finite number.  mlp1.0's weights x 1e5 put mlp1's first layer there."""
    torch.manual_seed(3)
    net = _net(13)
    with torch.no_grad():
        net.mlp1[0].weight.mul_(1.0e5)
    eng = _engine(3, 7)
    eng.sarl_configure(actions=_actions(), precision='f16x2')
    assert eng.sarl_network_route() == 'split_f16'
    eng.sarl_set_weights(net.state_dict())
    out = eng.sarl_select()
    X = eng.sarl_export('X').cpu()
    with torch.no_grad():
        assert float(torch.relu(net.mlp1[0](X.reshape(-1, 13))).max()) > 65504.0  # the case is what it claims to be
    V = eng.sarl_export('V').cpu().numpy()
    assert not np.isfinite(V).any()
    assert (out['best'].cpu().numpy() == -2).all()
    eng.close()


REFUSALS = {
    '12 humans': (dict(humans=12), dict(), '1..5 humans'),
    'cadrl': (dict(humans=5), dict(model='cadrl', mlp3_dims=(150, 100, 100, 1)), 'CADRL'),
    'lstm_rl': (dict(humans=5), dict(model='lstm_rl', mlp1_dims=(50, 1), mlp3_dims=(150, 100, 100, 1)), 'LSTM-RL'),
    'widths': (dict(humans=5), dict(mlp1_dims=(160, 100)), 'shipped layer widths'),
    'mixed': (dict(humans=5, mixed=True), dict(), 'mixed rule'),
}


@pytest.mark.parametrize('case', sorted(REFUSALS))
def test_split_f16_refuses_what_it_does_not_cover(case):
    import crowdnav_amd
    from crowdnav_amd import _lib
    eng_kw, cfg_kw, reason = REFUSALS[case]
    kw = dict(scenario_rule=crowdnav_amd.MIXED) if eng_kw.get('mixed') else {}
    eng = crowdnav_amd.BatchedCrowdSim(num_envs=4, num_humans=eng_kw['humans'], robot_policy=crowdnav_amd.ROBOT_EXTERNAL,
                                       robot_visible=1, **kw)
    with pytest.raises(crowdnav_amd.CrowdNavAmdError) as ei:
        eng.sarl_configure(actions=_actions(), precision='f16x2', **cfg_kw)
    assert ei.value.status == _lib.CN_ERR_UNSUPPORTED
    assert 'CN_PRECISION_F16X2' in str(ei.value) and reason in str(ei.value)
    with pytest.raises(crowdnav_amd.CrowdNavAmdError):
        eng.sarl_network_route()  # the refusal left the engine unconfigured
    eng.sarl_configure(actions=_actions(), precision='f32', **cfg_kw)  # ... and free to configure in fp32
    assert eng.sarl_network_route() != 'split_f16'
    eng.close()


def test_split_f16_unknown_precision_is_invalid():
    import crowdnav_amd
    from crowdnav_amd import _lib
    eng = crowdnav_amd.BatchedCrowdSim(num_envs=4, num_humans=5, robot_policy=crowdnav_amd.ROBOT_EXTERNAL, robot_visible=1)
    with pytest.raises(crowdnav_amd.CrowdNavAmdError) as ei:
        eng.sarl_configure(actions=_actions(), precision=7)
    assert ei.value.status == _lib.CN_ERR_INVALID and 'precision' in str(ei.value)
    eng.sarl_configure(actions=_actions())
    assert eng.sarl_network_route() == 'lds_tile'
    eng.close()


def _compat(policy_name, weights=None):
    import crowdnav_amd.compat as c
    from crowdnav_amd.compat.sarl import default_policy_config
    cfg = c.default_env_config({('robot', 'visible'): 'true'})
    env = c.CrowdSim()
    env.configure(cfg)
    robot = c.Robot(cfg, 'robot')
    policy = c.policy_factory[policy_name]()
    policy.configure(default_policy_config())
    if weights is not None:
        policy.get_model().load_state_dict(weights)
    robot.set_policy(policy)
    env.set_robot(robot)
    policy.set_phase('test')
    policy.set_device(torch.device('cpu'))
    policy.set_env(env)
    return c.Explorer(env, robot, 'cpu', gamma=0.9)


def test_compat_switch_takes_the_split_route(monkeypatch, caplog):
    monkeypatch.setenv('CROWDNAV_AMD_SARL_PRECISION', 'f16x2')
    g = load_golden('sarl_plain.npz')
    ex = _compat('sarl', {k[len('param_'):]: torch.from_numpy(v) for k, v in g.items() if k.startswith('param_')})
    with caplog.at_level(logging.WARNING):
        ex.run_k_episodes(8, 'test')
    assert ex.last_batch['network_route'] == 'split_f16'
    assert not [r for r in caplog.records if 'CROWDNAV_AMD_SARL_PRECISION' in r.getMessage()]
    assert len(ex.last_batch['outcome']) == 8 and all(o in (2, 3, 4) for o in ex.last_batch['outcome'])
    assert min(ex.last_batch['steps']) >= 1
    stats = ex.last_stats
    assert all(np.isfinite(stats[k]) for k in ('success_rate', 'collision_rate', 'nav_time', 'total_reward'))


def test_compat_switch_logs_a_refusal_once_and_runs_fp32(monkeypatch, caplog):
    monkeypatch.setenv('CROWDNAV_AMD_SARL_PRECISION', 'f16x2')
    torch.manual_seed(7)
    ex = _compat('cadrl')
    with caplog.at_level(logging.WARNING):
        ex.run_k_episodes(8, 'test')
        ex.run_k_episodes(8, 'test')  # a second engine: no second line
    lines = [r.getMessage() for r in caplog.records if 'CROWDNAV_AMD_SARL_PRECISION' in r.getMessage()]
    assert len(lines) == 1 and 'CADRL' in lines[0] and 'fp32' in lines[0]
    assert ex.last_batch['network_route'] not in (None, 'split_f16')
    assert len(ex.last_batch['outcome']) == 8 and all(o in (2, 3, 4) for o in ex.last_batch['outcome'])
