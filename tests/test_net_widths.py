"""Value-network layer widths other than the shipped ones, and with_global_state = 0, on the MI355X.

cn_sarl_configure takes any layer widths; every other value-network test runs the shipped ones.  The settings of
net_width_cases.py (pinned by test_net_widths_host.py) go through the generic kernels here — the one-tile LDS kernels, the streamed
ones, the narrow tiles — for sarl.ValueNetwork with and without the global state, cadrl.ValueNetwork and both LSTM-RL networks.
Values: V against the same torch module in float64 on the X the device exports, E = max|V - V64| / max|V64| per case,
E_kernel <= max(8 E_torch32, 2^-20): test_train_step.py's FACTOR and FLOOR, for the reasons given there; the attention weights
by the same rule.  Routes against each other: bit for bit.  CROWDNAV_AMD_NET_WIDTHS_REPORT=<file> appends the measured pairs and
routes (profiles/net_widths_parity.txt)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import net_width_cases as cases
from support import environ as _env

pytestmark = pytest.mark.gpu
FACTOR, FLOOR = 8.0, 2.0 ** -20
GAMMA_BAR = 0.9 ** (0.25 * 1.0)  # pow(gamma, time_step * v_pref), multi_human_rl.py:52
SARL = [s for s in cases.SETTINGS if s.model == 'sarl']
# one 81-action case per model: more than one tile per env
MANY_ACTIONS = {'odd': 5, 'cadrl_37_29_7': 5, 'lstm_h33_64_150_40': 5}


def _report(line):
    path = os.environ.get('CROWDNAV_AMD_NET_WIDTHS_REPORT')
    print(line)
    if path:
        with open(path, 'a') as f:
            f.write(line + '\n')


def _sweep(humans, admits):
    """[(setting, H)] for the H of `humans` at which admits(setting, H), as pytest params with readable ids."""
    return [pytest.param(s, H, id='%s-H%d' % (s.name, H)) for s in cases.SETTINGS for H in humans if admits(s, H)]


@functools.lru_cache(maxsize=None)
def _net(name):
    return cases.network(cases.BY_NAME[name])


@functools.lru_cache(maxsize=None)
def _net64(name):
    return cases.double_of(_net(name))


def _engine(s, state8, n_act=5, seeds=None, **kw):
    import crowdnav_amd
    B, A = state8.shape[:2]
    eng = crowdnav_amd.BatchedCrowdSim(num_envs=B, num_humans=A - 1, robot_policy=crowdnav_amd.ROBOT_EXTERNAL, robot_visible=1)
    if seeds is not None:
        eng.reset(np.asarray(seeds))
    else:
        eng.set_state(state8, np.zeros(B))
    eng.sarl_configure(actions=cases.actions(n_act), **dict(cases.configure_kwargs(s), **kw))
    eng.sarl_set_weights(_net(s.name).state_dict())
    return eng


@functools.lru_cache(maxsize=None)
def _decision(name, humans, narrow='0', n_act=5, reg='1', attention=False):
    """One sarl_select (or sarl_select_attention) on the three crowds; everything the tests compare, as host arrays."""
    s = cases.BY_NAME[name]
    with _env(CROWDNAV_AMD_SARL_NARROW=narrow, CROWDNAV_AMD_SARL_REG=reg):
        eng = _engine(s, cases.crowd(humans), n_act=n_act)
        out = eng.sarl_select(want_attention=attention)
        got = dict(route=eng.sarl_network_route(), narrow_launches=eng.launch_counts()['sarl_narrow'],
                   V=eng.sarl_export('V').cpu().numpy(), X=eng.sarl_export('X').cpu().numpy(),
                   reward=eng.sarl_export('reward').cpu().numpy(), values=out['values'].cpu().numpy(),
                   best=out['best'].cpu().numpy(), action=out['action'].cpu().numpy(),
                   attention=out['attention'].cpu().numpy() if attention else None)
        eng.close()
    return got


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same_decision(a, b, where):
    for k in ('V', 'values', 'best', 'action'):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), (where, k)


@functools.lru_cache(maxsize=None)
def _truth(name, humans, n_act=5):
    """The float64 truth and the float32 yardstick of the case, on the X its one-tile / streamed decision exported."""
    s, d = cases.BY_NAME[name], _decision(name, humans, n_act=n_act)
    B, K, H, width = d['X'].shape
    x = torch.from_numpy(d['X'].reshape(B * K, H, width))
    V64 = cases.evaluate(s, _net64(name), x.double()).reshape(B, K).numpy()
    V32 = cases.evaluate(s, _net(name), x).reshape(B, K).numpy().astype(np.float64)
    scale = np.abs(V64).max()
    return dict(x=x, V64=V64, scale=scale, E_torch=np.abs(V32 - V64).max() / scale)


def _check_case_conditions(s, d, t, where):
    """Conditions on the case, never used as filters: change the seed in net_width_cases.py, not a bound."""
    V64 = t['V64']
    assert np.isfinite(V64).all() and t['scale'] > 0, where
    # the humans and the action reach the value: a kernel that lost either would fail the comparison
    assert ((V64.max(axis=1) - V64.min(axis=1)) >= 1e-3 * t['scale']).all(), (where, V64)
    if s.model == 'sarl':
        scores, _ = cases.attention(_net64(s.name), t['x'].double())
        assert not (scores == 0).all(dim=1).any(), where
    if s.name.startswith(('tiny', 'odd')):
        alive = cases.relu_layers_alive(_net(s.name), t['x'])
        assert alive and all(ok for _, ok in alive), (where, alive)


def _check_values(V, t, where):
    """The rule: E_kernel <= max(8 E_torch32, 2^-20).  Returns (E_kernel, the allowed absolute error of a V)."""
    assert np.isfinite(V).all(), where
    E_kernel = np.abs(V.astype(np.float64) - t['V64']).max() / t['scale']
    allowed = max(FACTOR * t['E_torch'], FLOOR)
    print('%s E_torch32 %.3e E_kernel %.3e' % (where, t['E_torch'], E_kernel))
    assert E_kernel <= allowed, (where, t['E_torch'], E_kernel)
    return E_kernel, allowed * t['scale']


def _check_best(d, t, tol_v, where):
    """best is the float64 arg-max of reward + gamma_bar V64 wherever the runner-up is further away than twice the allowed value
    error; elsewhere one of the two."""
    want = d['reward'] + GAMMA_BAR * t['V64']
    tol = 2.0 * GAMMA_BAR * tol_v
    for b in range(len(want)):
        order = np.argsort(-want[b], kind='stable')
        first, second = order[0], order[1]
        if want[b, first] - want[b, second] > tol:
            assert d['best'][b] == first, (where, b, want[b], d['best'][b])
        else:
            assert d['best'][b] in (first, second), (where, b, want[b], d['best'][b])
        assert np.array_equal(d['action'][b], cases.actions(want.shape[1])[d['best'][b]]), (where, b)
    # what the device returned as values is reward + gamma_bar V of its own V, in float64
    assert np.allclose(d['values'], d['reward'] + GAMMA_BAR * d['V'].astype(np.float64), rtol=1e-15, atol=0), where


# ---- 1. values against float64 on the one-tile and the streamed kernels
def _value_cases():
    out = _sweep(cases.HUMANS, lambda s, H: cases.lds_route(s, H) is not None)
    return [pytest.param(*p.values, 5, id=p.id) for p in out] + [
        pytest.param(cases.BY_NAME[name], H, 81, id='%s-H%d-K81' % (name, H)) for name, H in MANY_ACTIONS.items()]


@pytest.mark.parametrize('s,humans,n_act', _value_cases())
def test_values_against_float64(s, humans, n_act):
    d, t = _decision(s.name, humans, n_act=n_act), _truth(s.name, humans, n_act)
    where = 'value %-22s H=%d K=%2d route %-11s' % (s.name, humans, n_act, d['route'])
    assert d['route'] == cases.lds_route(s, humans) and d['narrow_launches'] == 0, where  # the table predicts the kernel
    assert d['X'].shape == (cases.ENVS, n_act, humans, 13) and np.isfinite(d['X']).all(), where
    _check_case_conditions(s, d, t, where)
    E_kernel, tol_v = _check_values(d['V'], t, where)
    _check_best(d, t, tol_v, where)
    _report('%s E_torch32 %.3e E_kernel %.3e' % (where, t['E_torch'], E_kernel))


def test_wide_is_one_tile_at_two_humans_and_streams_at_five():
    assert _decision('wide', 2)['route'] == 'lds_tile' and _decision('wide', 5)['route'] == 'lds_chunked'
    assert all(_decision(s.name, 9)['route'] == 'lds_chunked' for s in cases.SETTINGS)


@pytest.mark.parametrize('name', ['odd_noglobal', 'widening', 'wide'])
def test_more_tiles_than_compute_units(name):
    """The one-tile kernel is persistent: with more tiles than compute units a workgroup takes a second tile and runs the value
    head of the first on its side waves (7..15, then 7..13) beside the second tile's layers — at `widening`'s 140- and 150-wide
    head that is 9 and 10 column tiles on 7 waves, a second trip of the side chain's column-tile loop the shipped head (7 tiles)
    never makes.  64 envs x 81 actions = 324 tiles; every group against float64 by the same rule."""
    s, humans, B, K = cases.BY_NAME[name], 2, 64, 81
    assert (B * K + 15) // 16 > torch.cuda.get_device_properties(0).multi_processor_count
    state8 = np.concatenate([cases.crowd(humans, salt) for salt in range(22)])[:B]
    with _env(CROWDNAV_AMD_SARL_NARROW='0', CROWDNAV_AMD_SARL_REG='1'):
        eng = _engine(s, state8, n_act=K)
        eng.sarl_select()
        route, V, X = eng.sarl_network_route(), eng.sarl_export('V').cpu().numpy(), eng.sarl_export('X').cpu()
        eng.close()
    assert route == 'lds_tile'
    x = X.reshape(B * K, humans, 13)
    V64 = cases.evaluate(s, _net64(name), x.double()).reshape(B, K).numpy()
    V32 = cases.evaluate(s, _net(name), x).reshape(B, K).numpy().astype(np.float64)
    t = dict(V64=V64, scale=np.abs(V64).max(), E_torch=np.abs(V32 - V64).max() / np.abs(V64).max())
    where = 'value %-22s H=%d K=%2d route %-11s B=%d' % (name, humans, K, route, B)
    E_kernel, _ = _check_values(V, t, where)
    _report('%s E_torch32 %.3e E_kernel %.3e  (persistent: side-chain value head)' % (where, t['E_torch'], E_kernel))


# ---- 2. the narrow tiles, bit for bit
@pytest.mark.parametrize('s,humans', _sweep((1, 2, 5), cases.narrow_admits))
def test_narrow_route_is_bit_identical(s, humans):
    wide, narrow = _decision(s.name, humans), _decision(s.name, humans, narrow='2')
    where = 'narrow %-21s H=%d' % (s.name, humans)
    assert narrow['route'] == 'narrow' and narrow['narrow_launches'] == 1 and wide['narrow_launches'] == 0, (where, narrow['route'])
    _same_decision(narrow, wide, where)
    assert np.array_equal(_bits(narrow['X']), _bits(wide['X'])) and np.array_equal(narrow['reward'], wide['reward']), where
    E_kernel, _ = _check_values(narrow['V'], _truth(s.name, humans), where)
    tail = any(cases.kpad(K) > cases.NARROW_K for _, _, K, _, _ in cases.layers(s))
    _report('%s K= 5 route %-11s E_torch32 %.3e E_kernel %.3e%s' % (where.replace('narrow', 'value '), narrow['route'],
                                                                    _truth(s.name, humans)['E_torch'], E_kernel,
                                                                    '  (k tail beyond the registers)' if tail else ''))


def test_the_narrow_k_tail_has_run():
    """wide at 2 humans is the case that enters narrow_dense's `kpad > kNarrowK` tail; CADRL's 272-wide layer does too."""
    for name in ('wide', 'cadrl_272_100_36'):
        s = cases.BY_NAME[name]
        assert any(cases.kpad(K) > cases.NARROW_K for _, _, K, _, _ in cases.layers(s)) and cases.narrow_admits(s, 2)
        assert _decision(name, 2, narrow='2')['route'] == 'narrow'


@pytest.mark.parametrize('s,humans', _sweep((1, 2, 5), lambda s, H: s.model == 'lstm_rl' and not cases.narrow_admits(s, H)))
def test_forcing_the_narrow_route_beyond_its_limits_changes_nothing(s, humans):
    """LSTM hidden 64 is one past the W_hh rows the narrow kernel holds (ValueNetwork2 has no narrow kernel): forced, the
    configuration stays on the one-tile kernel with the same bits."""
    wide, forced = _decision(s.name, humans), _decision(s.name, humans, narrow='2')
    assert forced['route'] == 'lds_tile' and forced['narrow_launches'] == 0, (s.name, humans, forced['route'])
    _same_decision(forced, wide, (s.name, humans))


# ---- 3. attention weights
def _attention_cases():
    out = []
    for s in SARL:
        for H in (2, 5, 9):
            out.append(pytest.param(s, H, '0', id='%s-H%d-%s' % (s.name, H, cases.lds_route(s, H))))
            if cases.narrow_admits(s, H):
                out.append(pytest.param(s, H, '2', id='%s-H%d-narrow' % (s.name, H)))
    return out


@pytest.mark.parametrize('s,humans,narrow', _attention_cases())
def test_attention_weights(s, humans, narrow):
    plain, att = _decision(s.name, humans, narrow=narrow), _decision(s.name, humans, narrow=narrow, attention=True)
    where = 'attn  %-22s H=%d K= 5 route %-11s' % (s.name, humans, att['route'])
    assert att['route'] == plain['route'] == ('narrow' if narrow == '2' else cases.lds_route(s, humans)), where
    _same_decision(att, plain, where)
    x = _truth(s.name, humans)['x']
    _, w64 = cases.attention(_net64(s.name), x.double())
    _, w32 = cases.attention(_net(s.name), x)
    w64, w32 = w64.numpy(), w32.numpy().astype(np.float64)
    got = att['attention'].reshape(-1, humans)
    scale = np.abs(w64).max()
    E_torch, E_kernel = np.abs(w32 - w64).max() / scale, np.abs(got.astype(np.float64) - w64).max() / scale
    _report('%s E_torch32 %.3e E_kernel %.3e' % (where, E_torch, E_kernel))
    assert np.isfinite(got).all() and E_kernel <= max(FACTOR * E_torch, FLOOR), (where, E_torch, E_kernel)
    assert (np.abs(got.astype(np.float64).sum(axis=1) - 1.0) <= 4 * np.spacing(np.float32(1.0))).all(), where


# ---- 4. the kernels compiled for the shipped widths stay away
@pytest.mark.parametrize('s,humans', _sweep((2, 5), lambda s, H: True))
def test_register_kernels_stay_away(s, humans):
    asked = _decision(s.name, humans, reg='2')
    assert asked['route'] == cases.lds_route(s, humans), (s.name, humans, asked['route'])
    _same_decision(asked, _decision(s.name, humans), (s.name, humans))


def test_register_kernels_still_take_the_shipped_widths():
    """The control of the test above: the same request on the shipped network IS served by the register-resident kernel."""
    shipped = cases.Setting('shipped', 'sarl', dict(cases.SHIPPED), True, 0, '')
    with _env(CROWDNAV_AMD_SARL_NARROW='0', CROWDNAV_AMD_SARL_REG='2'):
        import crowdnav_amd
        eng = crowdnav_amd.BatchedCrowdSim(num_envs=3, num_humans=5, robot_policy=crowdnav_amd.ROBOT_EXTERNAL, robot_visible=1)
        eng.sarl_configure(actions=cases.actions(5), **cases.configure_kwargs(shipped))
        assert eng.sarl_network_route() == 'reg_sarl'
        eng.close()


@pytest.mark.parametrize('name,reason', [('shipped_noglobal', 'with_global_state = 0'), ('odd', 'shipped layer widths'),
                                         ('odd_noglobal', 'with_global_state = 0')])
def test_split_f16_is_refused_by_name(name, reason):
    import crowdnav_amd
    from crowdnav_amd import _lib
    eng = crowdnav_amd.BatchedCrowdSim(num_envs=3, num_humans=5, robot_policy=crowdnav_amd.ROBOT_EXTERNAL, robot_visible=1)
    with pytest.raises(crowdnav_amd.CrowdNavAmdError) as ei:
        eng.sarl_configure(actions=cases.actions(5), precision='f16x2', **cases.configure_kwargs(cases.BY_NAME[name]))
    assert ei.value.status == _lib.CN_ERR_UNSUPPORTED and 'CN_PRECISION_F16X2' in str(ei.value) and reason in str(ei.value), str(ei.value)
    eng.sarl_configure(actions=cases.actions(5), **cases.configure_kwargs(cases.BY_NAME[name]))  # the refusal left it unconfigured
    assert eng.sarl_network_route() in ('lds_tile', 'narrow')
    eng.close()


# ---- 5. caller-held states
HELD = ['tiny', 'tiny_noglobal', 'odd', 'odd_noglobal', 'shipped_noglobal', 'lstm_h7_31_13_7', 'lstm_h33_64_150_40']


def _rows_of(s, state8):
    """The float32 rows [n, H, 13] sarl_transform writes for the joint states state8 [n, A, 8], env order."""
    eng = _engine(s, state8)
    rows = eng.sarl_transform(sort_humans=False).cpu()
    eng.close()
    return rows


def _check_held(s, V, rows, where):
    V64 = cases.evaluate(s, _net64(s.name), rows.double()).numpy()
    V32 = cases.evaluate(s, _net(s.name), rows).numpy().astype(np.float64)
    scale = np.abs(V64).max()
    E_torch, E_kernel = np.abs(V32 - V64).max() / scale, np.abs(V.astype(np.float64) - V64).max() / scale
    _report('%s E_torch32 %.3e E_kernel %.3e' % (where, E_torch, E_kernel))
    assert np.isfinite(V).all() and np.isfinite(V64).all() and E_kernel <= max(FACTOR * E_torch, FLOOR), (where, E_torch, E_kernel)


@pytest.mark.parametrize('humans', [2, 5])
@pytest.mark.parametrize('name', HELD)
def test_values_of_caller_held_states(name, humans):
    s = cases.BY_NAME[name]
    B, K = cases.ENVS, 5
    many = np.concatenate([cases.crowd(humans, salt) for salt in range(6)])[:B * K + 1]  # 16 states: B K + 1
    rows = _rows_of(s, many)
    for narrow in ('0', '2'):
        with _env(CROWDNAV_AMD_SARL_NARROW=narrow):
            eng = _engine(s, cases.crowd(humans))
            route = eng.sarl_network_route()
            assert route == ('narrow' if narrow == '2' else 'lds_tile'), (name, humans, route)
            where = 'held  %-22s H=%d route %-8s' % (name, humans, route)
            own = eng.sarl_transform(sort_humans=False)
            assert np.array_equal(_bits(own.cpu().numpy()), _bits(rows[:B].numpy())), where
            if narrow == '2':  # cn_sarl_values: the narrow tiles read the caller's rows where they lie
                before = eng.launch_counts()['sarl_narrow']
                V = eng.sarl_values(own).cpu().numpy()
                assert eng.launch_counts()['sarl_narrow'] == before + 1, where
                _check_held(s, V, rows[:B], where + ' sarl_values      n=%2d' % B)
            V = eng.sarl_state_values(eng.get_state()[0]).cpu().numpy()
            _check_held(s, V, rows[:B], where + ' state_values     n=%2d' % B)
            # one state; a ragged last tile (on a 17-state engine: one pass); more states than a pass holds: a second pass
            for n in (1, B * K + 1):
                V = eng.sarl_state_values(many[:n]).cpu().numpy()
                _check_held(s, V, rows[:n], where + ' state_values     n=%2d' % n)
            eng.close()


@pytest.mark.parametrize('name', ['odd', 'lstm_h33_64_150_40'])
def test_seventeen_caller_held_states_in_one_pass(name):
    """17 states on an engine whose pass holds 20: two tiles, the second with one state."""
    s, humans = cases.BY_NAME[name], 5
    many = np.concatenate([cases.crowd(humans, salt) for salt in range(6)])[:17]
    rows = _rows_of(s, many)
    with _env(CROWDNAV_AMD_SARL_NARROW='0'):
        eng = _engine(s, cases.crowd(humans, 7)[:1].repeat(4, axis=0))  # 4 envs x 5 actions
        V = eng.sarl_state_values(many).cpu().numpy()
        eng.close()
    _check_held(s, V, rows, 'held  %-22s H=%d route lds_tile state_values     n=17' % (name, humans))


# ---- 6. the fused sampling step against the five calls it replaces
@pytest.mark.parametrize('name', ['odd', 'odd_noglobal', 'lstm_h33_64_150_40'])
def test_sample_step_is_the_five_calls(name):
    from crowdnav_amd._lib import check
    s, B, H, K, EPS = cases.BY_NAME[name], cases.ENVS, 3, 5, 0.3
    lstm = s.model == 'lstm_rl'

    def buffers(eng):
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=eng.device)  # noqa: E731
        out = dict(traj=z((B, 1, H, 13), torch.float32), rew=z((1, B), torch.float64), inf=z((1, B), torch.uint8), dmn=z((1, B), torch.float64),
                   act=z((1, B), torch.int32), alive=z((B,), torch.uint8), done=z((B,), torch.uint8), action=z((B, 2), torch.float64))
        out['alive'].fill_(1)
        return out

    def finish(eng, t):
        eng.sync()
        got = {k: v.cpu().numpy() for k, v in t.items()}
        got['state'], got['counts'] = eng.get_state()[0].cpu().numpy(), eng.launch_counts()
        eng.close()
        return got

    def one_call(narrow, fused):
        with _env(CROWDNAV_AMD_SARL_NARROW=narrow, CROWDNAV_AMD_SARL_FUSED_STEP=fused):
            eng = _engine(s, cases.crowd(H), seeds=500 + np.arange(B))
        t = buffers(eng)
        eng.sarl_sampler(t['traj'], t['rew'], t['inf'], t['dmn'], t['act'], t['alive'], t['done'], t['action'])(0, EPS)
        return finish(eng, t)

    def five_calls():
        with _env(CROWDNAV_AMD_SARL_NARROW='0'):
            eng = _engine(s, cases.crowd(H), seeds=500 + np.arange(B))
        t = buffers(eng)
        lib, h, V = eng._lib, eng._h, C.c_void_p
        p = {k: V(v.data_ptr()) for k, v in t.items()}
        t['alive'].masked_fill_(t['done'].view(torch.bool), 0)
        check(lib.cn_sarl_select(h, None, p['act'], p['action']))
        check(lib.cn_sarl_explore(h, EPS, p['alive'], p['act'], p['action'], None))
        check(lib.cn_sarl_transform(h, p['traj'], H * 13, 1 if lstm else 0))
        check(lib.cn_step(h, p['action'], 1, p['rew'], p['done'], p['inf'], p['dmn'], None, None, None))
        return finish(eng, t)

    want = five_calls()
    assert np.isfinite(want['traj']).all() and (want['act'] >= 0).all() and want['counts']['sarl_narrow'] == 0
    for narrow, fused in (('2', '1'), ('2', '0'), ('0', '1')):
        got = one_call(narrow, fused)
        where = (name, narrow, fused)
        assert got['counts']['sarl_narrow'] == (1 if narrow == '2' else 0), (where, got['counts'])
        assert got['counts']['sarl_decide_steps'] == (1 if (narrow, fused) == ('2', '1') else 0), (where, got['counts'])
        for k in ('act', 'action', 'traj', 'rew', 'done', 'inf', 'dmn', 'alive', 'state'):
            assert np.array_equal(_bits(got[k]) if got[k].dtype.itemsize in (4, 8) else got[k],
                                  _bits(want[k]) if want[k].dtype.itemsize in (4, 8) else want[k]), (where, k)


# ---- 7. what the promise does not cover is refused, by name, and leaves the engine usable
def test_refusals_the_promise_allows():
    import crowdnav_amd
    from crowdnav_amd import _lib

    def engine(humans=5):
        return crowdnav_amd.BatchedCrowdSim(num_envs=3, num_humans=humans, robot_policy=crowdnav_amd.ROBOT_EXTERNAL, robot_visible=1)

    def refused(status, reason, humans=5, **kw):
        eng = engine(humans)
        with pytest.raises(crowdnav_amd.CrowdNavAmdError) as ei:
            eng.sarl_configure(actions=cases.actions(5), **kw)
        assert ei.value.status == status and reason in str(ei.value), (kw, str(ei.value))
        with pytest.raises(crowdnav_amd.CrowdNavAmdError):
            eng.sarl_network_route()  # the refusal left the engine unconfigured ...
        eng.close()                   # ... and it can still be destroyed
        fresh = engine(humans)        # a fresh engine is configured afterwards as if nothing had happened
        fresh.sarl_configure(actions=cases.actions(5))
        assert fresh.sarl_network_route() in ('lds_tile', 'lds_chunked', 'narrow')
        fresh.close()

    U, I = _lib.CN_ERR_UNSUPPORTED, _lib.CN_ERR_INVALID
    # a layer whose k loop (K = 1024: 256 k-steps -> kpad 260) or whose column tiles (N = 4100: 257) exceed the packed descriptor's bytes
    refused(U, 'layer 1024 -> 100 is wider than the packed descriptors hold', mlp1_dims=(1024, 100))
    refused(U, 'layer 13 -> 4100 is wider than the packed descriptors hold', mlp1_dims=(4100, 100))
    refused(U, 'wider than the packed descriptors hold', model='cadrl', mlp3_dims=(150, 1024, 100, 1))
    # every layer within the descriptors, the network beyond the 4 Mi floats of the weight arena (mlp2.0 alone: 255 x 255 x 64)
    refused(U, 'value network does not fit the weight arena', mlp1_dims=(1020, 1020), mlp2_dims=(4080, 50))
    # the single outputs the kernels are written for
    refused(U, 'attention must end in a single output', attention_dims=(100, 100, 2))
    refused(U, 'the value head must end in a single output', mlp3_dims=(150, 100, 100, 2))
    refused(U, 'the value head must end in a single output', model='cadrl', mlp3_dims=(150, 100, 100, 3))
    # widths that are no widths
    refused(I, 'bad mlp dims', mlp1_dims=(0, 100))
    refused(I, 'bad mlp dims', mlp2_dims=(100, -50))
    refused(I, 'bad mlp dims', mlp3_dims=(150, -1, 100, 1))
    refused(I, 'bad attention dims', attention_dims=(0, 100, 1))
    refused(I, 'mlp1_dims[0] must hold the hidden width', model='lstm_rl', mlp1_dims=(0, 1))
    refused(I, 'interaction_dims needs 4 positive widths', model='lstm_rl', mlp1_dims=(50, 1), interaction_dims=(150, 0, 100, 50))
    # sizes no LDS holds, one tile or streamed: the table's own predictions (net_width_cases.lds_route is None)
    refused(U, 'bytes of LDS per tile', **dict(cases.SHIPPED, mlp1_dims=(272, 100)))                # the streamed kernel: 202 496 B
    refused(U, 'bytes of LDS per tile', **dict(cases.SHIPPED, mlp1_dims=(16, 64), mlp2_dims=(128, 90), attention_dims=(120, 112, 1),
                                                mlp3_dims=(40, 140, 150, 1)))                       # ... 165 632 B
    for name in ('cadrl_272_100_36', 'cadrl_64_150_160'):                                           # CADRL streams by crowd size alone
        assert cases.lds_route(cases.BY_NAME[name], 8) is None
        refused(U, 'bytes of LDS per tile', humans=8, **cases.configure_kwargs(cases.BY_NAME[name]))
