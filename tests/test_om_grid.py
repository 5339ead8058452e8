"""Occupancy maps and value-network input widths other than the shipped 4 x 4 x 3 (13 / 61 inputs) on the MI355X.

Every map the device writes — the lookahead of a decision (occupancy_map_cap<8> / <64>), the replay-memory transform, the
fused sampling step (occupancy_maps_cooperative) — is compared with the host mirror of the reference's build_occupancy_maps
(pinned bit for bit against the unmodified reference by test_om_grid_host.py) applied to the float64 states the device itself
reports: sarl_export('next_obs') for decisions, get_state() for transforms.  A map is a discrete function, so:
  occupancy (the count channel of 1- and 3-channel maps, the set of non-zero cells) is EXACT, on the condition — asserted for
  every env of every case, never used as a filter — that no cell coordinate lies within om_grid_cases.MARGIN = 1e-9 of an
  integer (device atan2 / cos / sin differ from libm by a few float64 ulps, about 1e-15 in these coordinates);
  every velocity entry is within ONE float32 spacing of the mirror's: the float64 means differ by about 1e-15 relative, so
  the rounding to float32 can move by at most one step.
Values: V against torch float64 on an input built on the HOST (X[..., :13] + the mirror's maps, not the exported map
columns), E = max|V - V64| / max|V64| per case, E_kernel <= max(8 E_torch32, 2^-20) — test_train_step.py's FACTOR and FLOOR,
for the reasons given there.  CROWDNAV_AMD_OM_GRID_REPORT=<file> appends the measured pairs and routes."""
import functools
import os

import numpy as np
import pytest
import torch

import om_grid_cases as cases
from support import environ as _env

pytestmark = pytest.mark.gpu
FACTOR, FLOOR = 8.0, 2.0 ** -20
IDS = [cases.setting_id(s) for s in cases.GRID]
LSTM = dict(model='lstm_rl', mlp1_dims=(50, 1), mlp3_dims=(150, 100, 100, 1))


def _report(line):
    path = os.environ.get('CROWDNAV_AMD_OM_GRID_REPORT')
    print(line)
    if path:
        with open(path, 'a') as f:
            f.write(line + '\n')


@functools.lru_cache(maxsize=None)
def _actions(n):
    from crowdnav_amd.compat.sarl import build_action_space
    space, _, _ = build_action_space(1.0)
    return np.array([[a.vx, a.vy] for a in space[:n]])


@functools.lru_cache(maxsize=None)
def _net(width, model='sarl'):
    from crowdnav_amd.compat import lstm_rl
    from crowdnav_amd.compat.sarl import ValueNetwork
    torch.manual_seed(1300 + width)
    if model == 'lstm_rl':
        return lstm_rl.ValueNetwork1(width, 6, [150, 100, 100, 1], 50)
    return ValueNetwork(width, 6, [150, 100], [100, 50], [150, 100, 100, 1], [100, 100, 1], True, 1.0, 4)


def _crowds(setting, humans, shift=0.0):
    """Three envs: two random crowds and one whose human 0 sees the others 2^-20 cells either side of the grid's edges."""
    edge, _ = cases.near_edge_crowds(setting, humans, shift)
    return np.array([cases.state8_of(c) for c in (cases.random_crowd(setting, humans), cases.random_crowd(setting, humans, 1),
                                                  edge[humans % len(edge)])])


def _engine(state8, setting, with_om=True, n_act=5, model='sarl', query_env=True, step=True, seeds=None, **kw):
    import crowdnav_amd
    B, A = state8.shape[:2]
    eng = crowdnav_amd.BatchedCrowdSim(num_envs=B, num_humans=A - 1, robot_policy=crowdnav_amd.ROBOT_EXTERNAL, robot_visible=1)
    if seeds is not None:
        eng.reset(np.asarray(seeds))  # (the sampling step continues each env's random stream: it needs one)
    eng.set_state(state8, np.zeros(B))
    if step:
        eng.step(np.zeros((B, 2)), update=True, want_obs=False)  # the humans get ORCA velocities
    cell_num, cell_size, channels = setting
    eng.sarl_configure(actions=_actions(n_act), with_om=with_om, cell_num=cell_num, cell_size=cell_size, om_channel_size=channels,
                       query_env=query_env, **dict(LSTM if model == 'lstm_rl' else {}, **kw))
    eng.sarl_set_weights(_net(cases.in_dim(setting) if with_om else 13, model).state_dict())
    return eng


def _check_maps(om, states, setting, where):
    """om [B, H, width] float32 from the device against the mirror on states [B, H, 4+] float64 read back from the device."""
    cell_num, cell_size, channels = setting
    om, states = np.asarray(om), np.asarray(states, dtype=np.float64)
    assert om.shape == states.shape[:2] + (cell_num ** 2 * channels,), where
    for b in range(len(om)):
        margin = cases.cell_margin(states[b, :, :4], cell_num, cell_size)
        assert margin >= cases.MARGIN, (where, b, margin)  # a condition on the case, not a filter: change the seed, never the bound
        want = cases.mirror_maps(states[b], setting)
        got = om[b]
        assert np.array_equal(cases.cells_of_maps(got, setting), cases.cells_of_maps(want, setting)), (where, b)
        g3, w3 = got.reshape(len(got), -1, channels), want.reshape(len(want), -1, channels)
        if channels != 2:
            assert np.array_equal(g3[..., 0], w3[..., 0]), (where, b)  # occupied: 1, exactly
        if channels > 1:
            gv, wv = g3[..., -2:].astype(np.float64), w3[..., -2:]
            step = np.spacing(np.abs(wv)).astype(np.float64)  # float32 spacing at the mirror's value
            assert np.all(np.abs(gv - wv.astype(np.float64)) <= step), (where, b, np.abs(gv - wv).max())


@functools.lru_cache(maxsize=None)
def _decision(setting, humans, narrow='0', n_act=5, model='sarl', query_env=True):
    """One sarl_select on the three crowds; everything the tests compare, as host arrays."""
    with _env(CROWDNAV_AMD_SARL_NARROW=narrow):
        state8 = _crowds(setting, humans, 0.0 if query_env else cases.STEP_DT)
        eng = _engine(state8, setting, n_act=n_act, model=model, query_env=query_env, step=query_env)
        out = eng.sarl_select()
        got = dict(route=eng.sarl_network_route(), narrow_launches=eng.launch_counts()['sarl_narrow'],
                   V=eng.sarl_export('V').cpu().numpy(), best=out['best'].cpu().numpy(), action=out['action'].cpu().numpy(),
                   X=eng.sarl_export('X').cpu().numpy(), next_obs=eng.sarl_export('next_obs').cpu().numpy(),
                   om=eng.sarl_export('om').cpu().numpy(), state8=state8)
        eng.close()
    return got


def _check_decision(d, setting, where):
    where = '%s route %s' % (where, d['route'])
    assert np.isfinite(d['V']).all() and (d['best'] >= 0).all(), where
    _check_maps(d['om'], d['next_obs'], setting, where)
    B, K, H, _ = d['X'].shape
    want = np.broadcast_to(d['om'][:, None], (B, K, H, d['om'].shape[-1]))
    assert np.array_equal(d['X'][..., 13:].view(np.uint32), want.view(np.uint32)), where  # the map columns of X, bit for bit
    return where


# ---- (a) the maps of a decision's lookahead, every grid entry, 2..8 humans
@pytest.mark.parametrize('humans', [2, 3, 5, 8])
@pytest.mark.parametrize('setting', cases.GRID, ids=IDS)
def test_lookahead_maps_equal_the_mirror(setting, humans):
    d = _decision(setting, humans)
    where = _check_decision(d, setting, 'select %s H=%d' % (cases.setting_id(setting), humans))
    assert d['route'] in ('lds_tile', 'lds_chunked') and d['narrow_launches'] == 0, where
    _report('maps  %-9s in_dim %2d H=%d route %s' % (cases.setting_id(setting), cases.in_dim(setting), humans, d['route']))
    # the 13 rotated features do not depend on the maps: the same engine without them writes the same bits
    with _env(CROWDNAV_AMD_SARL_NARROW='0'):
        plain = _engine(d['state8'], setting, with_om=False)
        plain.sarl_select()
        X13 = plain.sarl_export('X').cpu().numpy()
        plain.close()
    assert X13.shape[-1] == 13 and np.array_equal(d['X'][..., :13].view(np.uint32), X13.view(np.uint32)), where


# ---- (b) the narrow tiles: both copy paths of the map columns (whole 16-byte quads; word by word at any other width)
@pytest.mark.parametrize('humans', [2, 3, 5])
@pytest.mark.parametrize('setting', cases.GRID, ids=IDS)
def test_narrow_route_is_bit_identical_at_every_width(setting, humans):
    wide, narrow = _decision(setting, humans), _decision(setting, humans, narrow='2')
    where = 'narrow %s H=%d' % (cases.setting_id(setting), humans)
    assert narrow['route'] == 'narrow' and narrow['narrow_launches'] == 1 and wide['narrow_launches'] == 0, (where, narrow['route'])
    for k in ('V', 'best', 'action', 'X', 'next_obs', 'om'):
        assert np.array_equal(narrow[k], wide[k]), (where, k)
    _check_maps(narrow['om'], narrow['next_obs'], setting, where)


# ---- (c) the values against torch on an input built on the host
@pytest.mark.parametrize('humans', [5, 8])
@pytest.mark.parametrize('setting', cases.GRID, ids=IDS)
def test_values_against_torch_on_a_host_built_input(setting, humans):
    width = cases.in_dim(setting)
    n_act = 81 if width in (22, 88) else 5
    d = _decision(setting, humans, n_act=n_act)
    where = _check_decision(d, setting, 'values %s H=%d K=%d' % (cases.setting_id(setting), humans, n_act))
    B, K, H, _ = d['X'].shape
    maps = np.stack([cases.mirror_maps(d['next_obs'][b], setting) for b in range(B)])  # [B, H, width - 13]
    X_host = np.concatenate([d['X'][..., :13], np.broadcast_to(maps[:, None], (B, K, H, width - 13))], axis=3)
    net = _net(width)
    with torch.no_grad():
        x = torch.from_numpy(X_host.reshape(B * K, H, width))
        V32 = net(x).reshape(B, K).numpy().astype(np.float64)
        net64 = type(net)(width, 6, [150, 100], [100, 50], [150, 100, 100, 1], [100, 100, 1], True, 1.0, 4).double()
        net64.load_state_dict({k: v.double() for k, v in net.state_dict().items()})
        V64 = net64(x.double()).reshape(B, K).numpy()
    scale = np.abs(V64).max()
    E_torch, E_kernel = np.abs(V32 - V64).max() / scale, np.abs(d['V'].astype(np.float64) - V64).max() / scale
    _report('value %-9s in_dim %2d H=%d K=%2d route %-11s E_torch32 %.3e E_kernel %.3e' % (
        cases.setting_id(setting), width, humans, n_act, d['route'], E_torch, E_kernel))
    assert E_kernel <= max(FACTOR * E_torch, FLOOR), (where, E_torch, E_kernel)


# ---- (d) the replay-memory transform of the CURRENT states, dense and strided, env order and LSTM-RL's order
def _check_transform(eng, setting, where):
    width = cases.in_dim(setting)
    state = eng.get_state()[0].cpu().numpy()  # [B, A, 8] float64: what the device holds
    B, H = state.shape[0], state.shape[1] - 1
    for sort in (False, True):
        dense = eng.sarl_transform(sort_humans=sort)
        T = 3
        traj = torch.full((B, T, H, width), -7.0, dtype=torch.float32, device=dense.device)
        eng.sarl_transform(out=traj[:, 1], env_stride=T * H * width, sort_humans=sort)
        dense, traj = dense.cpu().numpy(), traj.cpu().numpy()
        assert np.array_equal(traj[:, 1].view(np.uint32), dense.view(np.uint32)), (where, sort)
        assert np.all(traj[:, 0] == -7.0) and np.all(traj[:, 2] == -7.0), (where, sort)  # nothing beside the rows
        humans = state[:, 1:]
        if sort:  # LstmRL.predict's order: decreasing distance to the robot, ties in env order
            dist = np.linalg.norm(humans[:, :, :2] - state[:, :1, :2], axis=2)
            order = np.argsort(-dist, axis=1, kind='stable')
            humans = np.take_along_axis(humans, order[:, :, None], axis=1)
        _check_maps(dense[..., 13:], humans, setting, '%s sort=%s' % (where, sort))
        assert np.allclose(dense[..., 10], humans[..., 6]) and np.isfinite(dense).all()  # (column 10: the row's human radius)


@pytest.mark.parametrize('humans', [2, 3, 5, 8])
@pytest.mark.parametrize('setting', cases.GRID, ids=IDS)
def test_transform_maps_equal_the_mirror(setting, humans):
    state8 = _crowds(setting, humans)
    state8[:, 1:, 6] = 0.3 + 0.01 * np.arange(humans)  # radii tell the humans apart in the rows
    eng = _engine(state8, setting, step=False)
    assert np.array_equal(eng.get_state()[0].cpu().numpy(), state8)
    # the near-edge crowd reaches the device as built: its viewer sees humans 2^-20 cells from a boundary
    assert cases.cell_margin(state8[2, 1:, :4], setting[0], setting[1]) <= 1.01 * cases.EDGE_EPS
    _check_transform(eng, setting, 'transform %s H=%d' % (cases.setting_id(setting), humans))
    eng.close()


@pytest.mark.parametrize('setting', [s for s in cases.GRID if cases.exact_case(s) is not None],
                         ids=[cases.setting_id(s) for s in cases.GRID if cases.exact_case(s) is not None])
def test_transform_of_the_exact_case(setting):
    """Straight ahead at k cell_size, cell_size a power of two: xi lands exactly on cell_num - 1 and on cell_num with no rounding
    in any libm.  The viewer's cells are written out by hand (om_grid_cases.exact_case)."""
    states, cells = cases.exact_case(setting)
    state8 = np.array([cases.state8_of(states)] * 2)
    eng = _engine(state8, setting, step=False)
    rows = eng.sarl_transform(sort_humans=False).cpu().numpy()
    eng.close()
    for b in range(2):
        viewer = cases.cells_of_maps(rows[b, :, 13:], setting)[0]
        assert np.nonzero(viewer)[0].tolist() == cells, (setting, b)


# ---- (e) the sampling step: the fused decision + transition kernel shares the next decision's maps among its lanes
@pytest.mark.parametrize('humans', [2, 5, 8])
@pytest.mark.parametrize('setting', [(3, 0.5, 1), (4, 1.0, 2), (3, 1.0, 3), (5, 0.7, 3)], ids=cases.setting_id)
def test_sampling_step_maps_on_the_fused_route(setting, humans):
    width, B, T = cases.in_dim(setting), 2, 3
    state8 = _crowds(setting, humans)[:B]
    where = 'sampler %s H=%d' % (cases.setting_id(setting), humans)

    def run(fused, transform_first):
        with _env(CROWDNAV_AMD_SARL_NARROW='2', CROWDNAV_AMD_SARL_FUSED_STEP=fused):
            eng = _engine(state8, setting, step=False, seeds=300 + np.arange(B))
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=eng.device)  # noqa: E731
        traj, rew, inf, dmn = z((B, T, humans, width), torch.float32), z((T, B), torch.float64), z((T, B), torch.uint8), z((T, B), torch.float64)
        act, alive, done, action = z((T, B), torch.int32), z((B,), torch.uint8), z((B,), torch.uint8), z((B, 2), torch.float64)
        alive.fill_(1)
        step = eng.sarl_sampler(traj, rew, inf, dmn, act, alive, done, action)
        rows = []
        for t in range(T):
            if transform_first:
                rows.append(eng.sarl_transform(sort_humans=False).cpu().numpy())
            step(t, 0.0)
        eng.sync()
        out = dict(traj=traj.cpu().numpy(), rows=rows, counts=eng.launch_counts(), alive=alive.cpu().numpy(),
                   om=eng.sarl_export('om').cpu().numpy(), next_obs=eng.sarl_export('next_obs').cpu().numpy(),
                   state=eng.get_state()[0].cpu().numpy())
        eng.close()
        return out

    fused, plain = run('1', False), run('0', True)
    # (8 humans stream through the LDS kernel in chunks: no narrow tiles, so no fused step either; the comparisons hold all the same)
    expect = T if humans <= 5 else 0
    assert fused['counts']['sarl_narrow'] == expect and fused['counts']['sarl_decide_steps'] == expect, (where, fused['counts'])
    assert plain['counts']['sarl_decide_steps'] == 0, where
    assert fused['alive'].all() and plain['alive'].all(), where  # three steps end no episode here
    for t in range(T):
        got, want = fused['traj'][:, t, :, 13:], plain['rows'][t][..., 13:]
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (where, t)
        assert np.array_equal(plain['traj'][:, t].view(np.uint32), plain['rows'][t].view(np.uint32)), (where, t)
    assert np.array_equal(fused['state'], plain['state']), where
    # what the last call left for the next decision (fused: written by the step kernel; otherwise the last decision's own)
    _check_maps(fused['om'], fused['next_obs'], setting, where + ' fused')
    _check_maps(plain['om'], plain['next_obs'], setting, where + ' three launches')


# ---- (f) query_env = false: every human keeps its velocity; LSTM-RL feeds the sorted joint state (sort_lookahead)
@pytest.mark.parametrize('model,setting', [('sarl', (3, 0.5, 1)), ('lstm_rl', (4, 1.0, 2))], ids=['sarl-3x0.5x1', 'lstm_rl-4x1x2'])
def test_constant_velocity_lookahead_maps(model, setting):
    d = _decision(setting, 5, model=model, query_env=False)
    where = _check_decision(d, setting, 'query_env=False %s %s' % (model, cases.setting_id(setting)))
    # the humans moved by v dt onto the places the builder aimed at: the device saw the near-edge crowd AT the edges
    moved = d['state8'][:, 1:, :4].copy()
    moved[:, :, :2] += cases.STEP_DT * moved[:, :, 2:4]
    if model == 'lstm_rl':  # next_obs is in LstmRL.predict's order
        dist = np.linalg.norm(d['state8'][:, 1:, :2] - d['state8'][:, :1, :2], axis=2)
        moved = np.take_along_axis(moved, np.argsort(-dist, axis=1, kind='stable')[:, :, None], axis=1)
    assert np.array_equal(d['next_obs'][..., :4], moved), where
    assert cases.cell_margin(d['next_obs'][2, :, :4], setting[0], setting[1]) <= 1.01 * cases.EDGE_EPS, where
    _report('maps  %-9s in_dim %2d H=5 %s query_env=False route %s' % (cases.setting_id(setting), cases.in_dim(setting), model, d['route']))


# ---- (g) more than 8 humans: occupancy_map_cap<64>, the chunked LDS kernel, LSTM-RL one human per step
@pytest.mark.parametrize('model,humans', [('sarl', 9), ('sarl', 12), ('lstm_rl', 12)])
@pytest.mark.parametrize('setting', [(4, 1.0, 1), (3, 1.0, 3)], ids=cases.setting_id)
def test_more_than_eight_humans(setting, model, humans):
    d = _decision(setting, humans, model=model)
    where = _check_decision(d, setting, 'any-crowd %s %s H=%d' % (model, cases.setting_id(setting), humans))
    assert d['route'] == 'lds_chunked', where
    _report('maps  %-9s in_dim %2d H=%d %s route %s' % (cases.setting_id(setting), cases.in_dim(setting), humans, model, d['route']))
    eng = _engine(_crowds(setting, humans), setting, model=model, step=False)
    _check_transform(eng, setting, where + ' transform')
    eng.close()


# ---- (h) what the library cannot serve at these widths it refuses, by name
def test_refusals_stay_refusals(monkeypatch):
    import crowdnav_amd
    from crowdnav_amd import _lib
    setting = (4, 1.0, 1)  # 29 inputs
    om = dict(with_om=True, cell_num=4, cell_size=1.0, om_channel_size=1)

    def refused(eng, reason, **kw):
        with pytest.raises(crowdnav_amd.CrowdNavAmdError) as ei:
            eng.sarl_configure(actions=_actions(5), **dict(om, **kw))
        assert ei.value.status == _lib.CN_ERR_UNSUPPORTED and reason in str(ei.value), str(ei.value)
        with pytest.raises(crowdnav_amd.CrowdNavAmdError):
            eng.sarl_network_route()  # the refusal left the engine unconfigured

    def engine(**kw):
        return crowdnav_amd.BatchedCrowdSim(num_envs=3, num_humans=5, robot_policy=crowdnav_amd.ROBOT_EXTERNAL, robot_visible=1, **kw)

    def route(eng, **kw):
        eng.sarl_configure(actions=_actions(5), **kw)
        got = eng.sarl_network_route()
        eng.close()
        return got

    assert cases.in_dim(setting) == 29
    eng = engine()
    refused(eng, 'shipped layer widths', precision='f16x2')                  # the split-f16 kernel: 13 or 61 inputs only
    refused(eng, 'bytes of LDS per tile', mlp1_dims=(1000, 100))            # a tile no LDS holds, chunked or not
    eng.close()
    # the register-resident kernels are compiled for 13 / 61 inputs: asked for always, 29 inputs still take the LDS tile
    monkeypatch.setenv('CROWDNAV_AMD_SARL_REG', '2')
    monkeypatch.setenv('CROWDNAV_AMD_SARL_NARROW', '0')
    assert route(engine(), **om) == 'lds_tile'
    assert route(engine(), with_om=True) == 'reg_sarl'                       # (the control: 61 inputs do)
    # the mixed rule masks absent humans in the one-tile kernel: a network whose tile does not fit (a 170-wide mlp1: 164 928 B; the
    # chunked kernel's 157 696 B would) is refused, not streamed; the split-f16 kernel refuses 29 inputs there as anywhere; the
    # shipped widths at 29 inputs are served
    mixed = engine(scenario_rule=crowdnav_amd.MIXED)
    refused(mixed, 'mixed rule', mlp1_dims=(170, 100))
    refused(mixed, 'CN_PRECISION_F16X2', precision='f16x2')
    mixed.close()
    assert route(engine(scenario_rule=crowdnav_amd.MIXED), **om) == 'lds_tile'
