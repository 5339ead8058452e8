"""The device at environment settings other than the shipped env.config (env_setting_cases.py): cn_reset and the scenario ring,
cn_step, every cn_rollout route, the traced and action-table rollouts, the three lookaheads, the SARL decision, the planners and
the gym surface, against the unmodified reference's fixtures (tests/golden/settings_<name>.npz) and the CPU
oracle.  Every comparison is bit for bit unless a tolerance is named; the tolerances are those the existing tests use for the
same quantity (test_gpu_parity.py, test_bench_size_parity.py)."""
import math

import numpy as np
import pytest

import env_setting_cases as cases
import lookahead_cv_reference as cv
import lookahead_paths_reference as paths
import plan_reference as plan_ref
from conftest import load_golden
from env_settings_planning_cases import action_table as _table, lookahead_scene as _lookahead_scene
from support import amd, np_of as _np, same_bits as _same_bits  # noqa: F401  (amd: module fixture)

FIXTURES, flat, environ = cases.fixture_settings(), cases.flat, cases.environ

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ a. resets
def _reset_and_ring(amd, config, seeds):
    """cn_reset's states and draws, and the first states the scenario ring serves for the same seeds (the rows a traced first
    rollout step starts from)."""
    B = len(seeds)
    eng = amd.BatchedCrowdSim(num_envs=B, robot_policy=amd.ROBOT_ORCA, **config)
    draws = _np(eng.reset(seeds))
    state, gt = (_np(x) for x in eng.get_state())
    assert np.all(gt == 0.0)
    ring = amd.BatchedCrowdSim(num_envs=B, robot_policy=amd.ROBOT_ORCA, **config)
    ring.rollout_begin(seed_base=int(seeds[0]), seed_mod=cases.SEED_MOD, record_capacity=2)
    first = _np(ring.rollout_trace(1)['state8'])[:, 0]
    return state, draws, first


@pytest.mark.parametrize('s', FIXTURES, ids=cases.setting_id)
def test_reset_vs_reference_generator(amd, oracle_mod, s):
    """H = 5: the lane generators (dt_fifth_square: the square rule); H12_small: the wave generator's blocked-cell table;
    random_attributes at 12 humans: its prefilter path; H20_shard: the table at 20 humans."""
    g = load_golden(cases.fixture_name(s))
    want, seeds = g['reset_states'], g['reset_seeds']
    config = cases.fixture_config(g)
    got, draws, first = _reset_and_ring(amd, config, seeds)
    assert np.abs(got - want).max() <= 1e-12
    assert np.array_equal(got[:, :, 6:], want[:, :, 6:]) and np.array_equal(got[:, 0], want[:, 0])
    o = oracle_mod.CrowdOracle(num_envs=len(seeds), **config)
    assert np.array_equal(draws.astype(np.uint64), o.reset(seeds))  # same number of rejection attempts
    assert np.abs(first - want).max() <= 1e-12 and np.array_equal(first[:, :, 6:], want[:, :, 6:])


@pytest.mark.parametrize('s', cases.SETTINGS, ids=cases.setting_id)
def test_reset_vs_oracle_at_the_full_entry(amd, oracle_mod, s):
    """The entry with its oracle-only keys, on its own seeds."""
    seeds = cases.seeds(s)
    config = cases.engine_config(s)
    got, draws, first = _reset_and_ring(amd, config, seeds)
    o = oracle_mod.CrowdOracle(num_envs=len(seeds), **config)
    assert np.array_equal(draws.astype(np.uint64), o.reset(seeds))
    want = o.get_state()[0]
    assert np.abs(got - want).max() <= 1e-12 and np.abs(first - want).max() <= 1e-12
    assert np.array_equal(got[:, :, 6:], want[:, :, 6:]) and np.array_equal(got[:, 0], want[:, 0])


# ------------------------------------------------------------------------------------------------ b. cn_step
@pytest.mark.parametrize('update', [True, False])
@pytest.mark.parametrize('tag,visible', [('invisible', 0), ('visible', 1)])
@pytest.mark.parametrize('s', FIXTURES, ids=cases.setting_id)
def test_step_bit_exact_vs_reference_and_oracle(amd, oracle_mod, s, tag, visible, update):
    """Teacher-forced on every row of the fixture; the time is the one the reference accumulated."""
    g = load_golden(cases.fixture_name(s))
    before, after, t0, t1 = flat(g, tag)
    config = dict(cases.fixture_config(g), robot_visible=visible)
    eng = amd.BatchedCrowdSim(num_envs=len(before), robot_policy=amd.ROBOT_ORCA, **config)
    eng.set_state(before, t0)
    out = {k: _np(v) for k, v in eng.step(None, update=update).items()}
    state, gt = (_np(x) for x in eng.get_state())
    for k, name in (('reward', 'rewards'), ('done', 'dones'), ('info', 'infos'), ('action', 'actions')):
        assert np.array_equal(out[k], g['%s_%s' % (tag, name)]), k
    danger = g[tag + '_infos'] == 1
    assert np.array_equal(out['dmin'][danger], g[tag + '_dmins'][danger])
    assert np.array_equal(out['obs'], after[:, 1:, [0, 1, 2, 3, 6]])
    if update:
        assert np.array_equal(state, after) and np.array_equal(gt, t1)
    else:
        assert np.array_equal(state, before) and np.array_equal(gt, t0)
    o = oracle_mod.CrowdOracle(num_envs=len(before), robot_policy=1, **config)
    o.set_state(before, t0)
    want = o.step(None, update=update)
    assert np.array_equal(out['dmin'], want['dmin'])
    assert np.array_equal(out['orca_vel'].view(np.uint32), want['orca_vel'].view(np.uint32))


@pytest.mark.parametrize('s', [s for s in cases.SETTINGS if s.oracle_only], ids=cases.setting_id)
def test_free_running_steps_vs_oracle_at_the_full_entry(amd, oracle_mod, s):
    """The keys no fixture holds (ORCA's neighbour parameters, the humans' safety space): 40 steps from the entry's start states."""
    config = cases.engine_config(s, robot_visible=1)
    st = cases.start_states(oracle_mod, s)
    B = len(st)
    o = oracle_mod.CrowdOracle(num_envs=B, robot_policy=1, **config)
    o.set_state(st, np.zeros(B))
    eng = amd.BatchedCrowdSim(num_envs=B, robot_policy=amd.ROBOT_ORCA, **config)
    eng.set_state(st, np.zeros(B))
    for t in range(40):
        got = eng.step(None, update=True, want_obs=False)
        want = o.step(None, update=True)
        assert np.array_equal(_np(got['orca_vel']).view(np.uint32), want['orca_vel'].view(np.uint32)), t
        for k in ('reward', 'done', 'info', 'dmin', 'action'):
            assert np.array_equal(_np(got[k]), want[k]), (k, t)
    state, gt = (_np(x) for x in eng.get_state())
    assert np.array_equal(state, o.get_state()[0]) and np.array_equal(gt, o.get_state()[1])


# ------------------------------------------------------------------------------------------------ c. every rollout route
# (entry, the engine's switches, the route cn_rollout_route must report).  Two envs per wave is the headline geometry: the
# two-wave kernel, or with CROWDNAV_AMD_FUSED_SPLIT=0 the one-wave kernel that holds the same geometry as constants.
ROUTES = [
    ('dt_inexact', dict(CROWDNAV_AMD_ENVS_PER_WAVE=2), 'fused_split'),
    ('near_sighted', dict(CROWDNAV_AMD_ENVS_PER_WAVE=2), 'fused_split'),
    ('speeds', dict(CROWDNAV_AMD_ENVS_PER_WAVE=2, CROWDNAV_AMD_FUSED_SPLIT=0), 'fused'),
    ('radii_rewards', dict(CROWDNAV_AMD_ENVS_PER_WAVE=2), 'fused_split'),
    ('radii_rewards', dict(CROWDNAV_AMD_FUSED=0), 'generic'),
    ('dt_fifth_square', {}, 'fused'),
    ('table_edge', {}, 'fused'),
    ('random_attributes', {}, 'generic'),
    ('H12_small', {}, 'generic'),
    ('H20_shard', {}, 'shard'),
    ('H20_five_neighbours', {}, 'generic'),
]
RECORDS = 16


def test_route_table_takes_every_route_at_a_non_default_entry():
    taken = {route for _, _, route in ROUTES}
    assert taken == {'generic', 'fused', 'fused_split', 'shard'}
    assert {name for name, _, _ in ROUTES} == set(cases.BY_NAME)
    assert ('H20_five_neighbours', {}, 'generic') in ROUTES and ('H20_shard', {}, 'shard') in ROUTES


@pytest.mark.parametrize('name,switches,route', ROUTES, ids=['%s-%s%s' % (n, r, '-'.join([''] + sorted(sw))) for n, sw, r in ROUTES])
def test_rollout_vs_oracle(amd, oracle_mod, name, switches, route):
    s = cases.BY_NAME[name]
    B, config = s.envs, cases.engine_config(s, robot_visible=1)
    o = oracle_mod.CrowdOracle(num_envs=B, robot_policy=1, **config)
    o.set_gamma(cases.GAMMA)
    o.reset(cases.seeds(s))
    total, rec, cur = o.rollout_full(s.steps, cases.SEED_BASE, cases.SEED_MOD, RECORDS)
    assert rec['count'].max() <= RECORDS and rec['count'].sum() >= B // 2

    with environ(**switches):
        eng = amd.BatchedCrowdSim(num_envs=B, robot_policy=amd.ROBOT_ORCA, **config)
    eng.set_gamma(cases.GAMMA)
    took = eng.rollout_route(s.steps)
    print('route', name, switches, took)
    assert took == route
    bufs = eng.rollout_begin(seed_base=cases.SEED_BASE, seed_mod=cases.SEED_MOD, episode_limit=-1, record_capacity=RECORDS)
    for n in (1, 49, s.steps - 50):
        eng.rollout(n)
    eng.sync()
    assert int(_np(bufs['transitions'])[0]) == total == B * s.steps
    count = _np(bufs['ep_count'])
    assert np.array_equal(count, rec['count'])
    held = np.arange(RECORDS)[None] < count[:, None]
    for key, want, exact in (('ep_outcome', 'outcome', True), ('ep_steps', 'steps', True), ('ep_danger', 'danger', True),
                             ('ep_time', 'time', True), ('ep_return', 'ret', False), ('ep_danger_dmin_sum', 'dsum', False)):
        got = np.where(held, _np(bufs[key]), 0)
        ref = np.where(held, rec[want], 0)
        err = 0.0 if exact else float(np.abs(got - ref).max())
        print('  ', key, 'exact' if exact else 'max error %.3g' % err)
        assert np.array_equal(got, ref) if exact else err <= 1e-9, key
    assert np.array_equal(_np(bufs['cur_steps']), cur['steps']) and np.array_equal(_np(bufs['cur_danger']), cur['danger'])
    assert np.abs(_np(bufs['cur_return']) - cur['ret']).max() <= 1e-9
    state, gt = (_np(x) for x in eng.get_state())
    assert np.abs(state - o.get_state()[0]).max() <= 1e-9
    assert np.array_equal(gt, o.get_state()[1])  # the accumulated time of the running episodes


def test_table_edge_times_out_at_the_last_tabulated_step(amd, oracle_mod):
    """An external robot that stands still far from the crowd, robot invisible, one human parked inside its discomfort distance:
    a Danger reward at every step until the time limit, so the return reads the discount table up to its last used entry."""
    import torch
    s = cases.BY_NAME['table_edge']
    B = 8
    config = cases.engine_config(s, robot_visible=0)
    dt, limit = s.config['time_step'], s.config['time_limit']
    st = cases.still_robot(cases.start_states(oracle_mod, s, B))
    st[:, 1, :6] = [0.7, -40.0, 0.0, 0.0, 0.7, -40.0]  # at its goal, 0.1 from the robot's rim
    o = oracle_mod.CrowdOracle(num_envs=B, robot_policy=0, **config)
    o.set_state(st, np.zeros(B))
    ret, steps, danger = np.zeros(B), 0, 0
    while True:
        out = o.step(np.zeros((B, 2)), update=True)
        ret += pow(cases.GAMMA, steps * dt * 1.0) * out['reward']
        steps += 1
        danger += int(out['info'][0] == cases.INFO['danger'])
        assert np.all(out['info'] == out['info'][0])
        if out['done'][0]:
            break
    assert out['info'][0] == cases.INFO['timeout'] and steps == 241 and danger == 240 and np.all(ret < 0.0)
    assert steps + 8 <= 256 and (steps - 1) * dt == limit - 1.0  # crowd_sim.py:380: Timeout from global_time >= time_limit - 1 on

    eng = amd.BatchedCrowdSim(num_envs=B, robot_policy=amd.ROBOT_EXTERNAL, **config)
    eng.set_gamma(cases.GAMMA)
    bufs = eng.rollout_begin(seed_base=cases.SEED_BASE, seed_mod=cases.SEED_MOD, record_capacity=2)
    eng.set_state(st, np.zeros(B))
    eng.rollout_actions(torch.zeros(B, steps, 2, dtype=torch.float64, device=eng.device))
    eng.sync()
    assert np.all(_np(bufs['ep_count']) == 1) and np.all(_np(bufs['cur_steps']) == 0)
    assert np.all(_np(bufs['ep_outcome'])[:, 0] == cases.INFO['timeout']) and np.all(_np(bufs['ep_steps'])[:, 0] == steps)
    assert np.all(_np(bufs['ep_time'])[:, 0] == limit) and np.all(_np(bufs['ep_danger'])[:, 0] == danger)
    assert np.abs(_np(bufs['ep_return'])[:, 0] - ret).max() <= 1e-9


def test_one_step_past_the_table_is_refused(amd):
    """cn_create builds the engine's first table through cn_set_gamma, whose check reads time_limit and time_step alone: an engine
    one step past the table never exists, so there is none to call set_gamma or rollout_begin on."""
    s = cases.BY_NAME['table_edge']
    dt = s.config['time_step']
    with pytest.raises(amd.CrowdNavAmdError) as ei:
        amd.BatchedCrowdSim(num_envs=4, **cases.engine_config(s, time_limit=s.config['time_limit'] + dt))
    assert ei.value.status == -2  # CN_ERR_UNSUPPORTED
    assert '249 steps' in str(ei.value) and '248' in str(ei.value)


# ------------------------------------------------------------------------------------------------ d. traced rollouts, action tables
ROBOT_ENTRIES = ['dt_inexact', 'speeds', 'radii_rewards']
BEGIN = dict(seed_base=cases.SEED_BASE, seed_mod=cases.SEED_MOD, record_capacity=8)


@pytest.mark.parametrize('external', [False, True], ids=['rollout_trace', 'rollout_actions'])
@pytest.mark.parametrize('name', ROBOT_ENTRIES)
def test_traced_rollouts_are_the_step_loops(amd, name, external):
    """cn_rollout_trace (ORCA robot) and cn_rollout_actions (external robot, a random action table) against a twin engine that
    makes the same transitions one at a time — cn_step(update = false) for what the transition returns, then rollout(1) /
    rollout_step — through episode ends and resets.  The twin's clock before every step is the accumulated one."""
    import torch
    s = cases.BY_NAME[name]
    dt = s.config.get('time_step', 0.25)
    B, n = 8, int(round(15.0 / dt))  # 15 s: every env ends an episode and starts the next (60 or 150 steps)
    config = cases.engine_config(s, robot_visible=1, num_envs=B, robot_policy=amd.ROBOT_EXTERNAL if external else amd.ROBOT_ORCA)
    clock = [cases.accumulated(dt, k) for k in range(n + 1)]
    rng = np.random.RandomState(5)
    table = rng.uniform(-1.0, 1.0, (B, n, 2)) * s.config.get('robot_v_pref', 1.0)
    table[:, :, 1] = np.abs(table[:, :, 1])  # towards the crowd
    eng, twin = amd.BatchedCrowdSim(**config), amd.BatchedCrowdSim(**config)
    bufs, tbufs = eng.rollout_begin(**BEGIN), twin.rollout_begin(**BEGIN)
    rows = eng.rollout_actions(torch.from_numpy(table), trace=True, rewards=True) if external else eng.rollout_trace(n, rewards=True)
    eng.sync()
    rows = {k: _np(v) for k, v in rows.items()}
    assert np.all(rows['episode'] >= 0)
    for t in range(n):
        state, gtime = (_np(x) for x in twin.get_state())
        act = table[:, t] if external else None
        out = twin.step(act, update=False, want_obs=False)
        assert _same_bits(rows['state8'][:, t], state), t
        assert np.array_equal(gtime, [clock[k] for k in rows['step'][:, t]]), t
        for key in ('reward', 'info'):
            assert _same_bits(rows[key][:, t], _np(out[key])), (key, t)
        danger = rows['info'][:, t] == amd.DANGER
        assert _same_bits(rows['dmin'][:, t][danger], _np(out['dmin'])[danger]), t
        if external:
            twin.rollout_step(torch.from_numpy(np.ascontiguousarray(table[:, t])))
        else:
            twin.rollout(1)
    twin.sync()
    for k in bufs:
        assert torch.equal(bufs[k], tbufs[k]), k
    assert int(_np(bufs['ep_count']).sum()) >= 1 and (rows['step'] > 0).any()
    for a, b in zip(eng.get_state(), twin.get_state()):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ e. the three lookaheads
SHAPES = [(5, 33), (70, 4)]


def _step_loops(amd, config, state, gtime, table, gamma_table):
    """Every branch as cn_step loops on a twin engine of B x K envs."""
    B, K, n = table.shape[:3]
    twin = amd.BatchedCrowdSim(num_envs=B * K, robot_policy=amd.ROBOT_EXTERNAL, **config)
    twin.set_state(np.repeat(state, K, axis=0), np.repeat(gtime, K))
    acts = table.reshape(B * K, n, 2)
    got = dict(ret=np.zeros(B * K), info=np.zeros(B * K, np.uint8), steps=np.zeros(B * K, np.int32), time=np.zeros(B * K),
               final_state8=np.zeros((B * K, state.shape[1], 8)))
    running = np.ones(B * K, bool)
    for t in range(n):
        out = twin.step(np.ascontiguousarray(acts[:, t]), update=True, want_obs=False)
        st, gt = (_np(x) for x in twin.get_state())
        reward, done, info = (_np(out[k]) for k in ('reward', 'done', 'info'))
        got['ret'][running] = got['ret'][running] + gamma_table[t] * reward[running]
        got['info'][running], got['steps'][running], got['time'][running] = info[running], t + 1, gt[running]
        got['final_state8'][running] = st[running]
        running &= done == 0
    return {k: v.reshape((B, K) + v.shape[1:]) for k, v in got.items()}


def _compare_lookahead(look, want, who):
    for key in ('ret', 'info', 'steps', 'time', 'final_state8'):
        assert _same_bits(look[key], np.asarray(want[key], dtype=look[key].dtype)), (who, key)
    assert (look['info'] == cv.TIMEOUT).any(), who


@pytest.mark.parametrize('K,n', SHAPES)
@pytest.mark.parametrize('name', ROBOT_ENTRIES)
def test_lookaheads_vs_step_loops_and_restatements(amd, oracle_mod, name, K, n):
    s = cases.BY_NAME[name]
    eng, state, gtime, c = _lookahead_scene(amd, oracle_mod, s)
    B = len(state)
    table = _table(B, K, n, c['robot_v_pref'])
    disc = cv.discount_table(cases.GAMMA, c)
    config = cases.engine_config(s, robot_visible=1)
    # the clock of a branch is accumulated from the env's: k additions of dt, which k * dt does not give at these settings
    look = {k: _np(v) for k, v in eng.lookahead(table, final_state=True).items()}
    assert sorted(look) == ['final_state8', 'final_theta', 'info', 'ret', 'steps', 'time']
    _compare_lookahead(look, _step_loops(amd, config, state, gtime, table, disc), 'orca')
    print(name, K, n, 'non-zero returns', int((look['ret'] != 0).sum()), 'infos', np.bincount(look['info'].ravel(), minlength=5).tolist())
    if n == 4:
        assert (look['info'] < cv.REACH_GOAL).any()  # running branches beside the Timeout ones
    else:
        assert (look['ret'] != 0).any()  # the long horizon meets the crowd: something to discount
    want_time = np.array([[gtime[b] + 0.0 for _ in range(K)] for b in range(B)])
    for b in range(B):
        for k in range(K):
            for _ in range(int(look['steps'][b, k])):
                want_time[b, k] = want_time[b, k] + c['time_step']
    assert _same_bits(look['time'], want_time)
    eng.set_lookahead_human_model('constant_velocity')
    got = {k: _np(v) for k, v in eng.lookahead(table, final_state=True).items()}
    _compare_lookahead(got, cv.lookahead(state, gtime, table, c, cases.GAMMA), 'constant_velocity')
    eng.set_lookahead_human_model('orca')
    vel = np.random.RandomState(9).uniform(-1.0, 1.0, (B, n, s.humans, 2)) * c['human_v_pref'] / math.sqrt(2.0)
    got = {k: _np(v) for k, v in eng.lookahead_paths(table, vel, final_state=True).items()}
    _compare_lookahead(got, paths.lookahead(state, gtime, table, vel, c, cases.GAMMA), 'paths')


def _network(seed=11):
    import torch
    from crowdnav_amd.compat.sarl import ValueNetwork
    torch.manual_seed(seed)
    return ValueNetwork(13, 6, [150, 100], [100, 50], [150, 100, 100, 1], [100, 100, 1], True, 1.0, 4)


@pytest.mark.parametrize('name', ROBOT_ENTRIES)
def test_bootstrap_discounts_by_steps_dt_v_pref(amd, oracle_mod, name):
    from crowdnav_amd.compat.sarl import build_action_space
    s = cases.BY_NAME[name]
    eng, state, gtime, c = _lookahead_scene(amd, oracle_mod, s)
    B, K, n = len(state), 5, 4
    eng.sarl_configure(actions=np.array([list(a) for a in build_action_space(c['robot_v_pref'])[0]], dtype=np.float64), gamma=cases.GAMMA)
    eng.sarl_set_weights(_network().state_dict())
    table = _table(B, K, n, c['robot_v_pref'])
    look = eng.lookahead(table, bootstrap=True)
    direct = _np(eng.sarl_state_values(look['final_state8']))
    look = {k: _np(v) for k, v in look.items()}
    assert _same_bits(look['value'], direct.reshape(B, K))
    ended = look['info'] >= cv.REACH_GOAL
    assert ended.any() and (~ended).any()
    for b in range(B):
        for k in range(K):
            boot = math.pow(cases.GAMMA, int(look['steps'][b, k]) * c['time_step'] * c['robot_v_pref']) * float(np.float64(look['value'][b, k]))
            want = look['ret'][b, k] if ended[b, k] else look['ret'][b, k] + boot
            assert _same_bits(look['score'][b, k], np.float64(want)), (b, k)


# ------------------------------------------------------------------------------------------------ f. the SARL decision
def _sarl_engine(amd, g, query_env):
    import torch
    c = cases.config_from_overrides(__import__('json').loads(str(g['env_overrides_json'])))
    n = len(g['states'])
    eng = amd.BatchedCrowdSim(num_envs=n, num_humans=5, robot_policy=amd.ROBOT_EXTERNAL, robot_visible=1, **c)
    eng.reset(cases.SEED_BASE + np.arange(n))  # a seeded stream for the sampler's epsilon draw
    eng.set_state(g['states'], g['gtime'])
    eng.sarl_configure(actions=g['action_space'], gamma=0.9, query_env=query_env)
    net = _network()
    net.load_state_dict({k[len('param_'):]: torch.from_numpy(v) for k, v in g.items() if k.startswith('param_')})
    eng.sarl_set_weights(net.state_dict())
    return eng, c


@pytest.mark.parametrize('query_env', [True, False], ids=['query', 'noquery'])
def test_sarl_decision_vs_reference(amd, query_env):
    """Tolerances of test_sarl.py / test_noquery.py: rewards and next_obs exact, features 5e-6, network output and values 1e-6,
    the arg-max wherever the reference's top two values are more than 4e-6 apart."""
    g = load_golden('sarl_settings_query.npz' if query_env else 'sarl_settings_noquery.npz')
    eng, c = _sarl_engine(amd, g, query_env)
    n = len(g['states'])
    out = eng.sarl_select()
    eng.sync()
    reward = _np(eng.sarl_export('reward'))
    assert np.array_equal(reward, g['rewards'])
    assert np.abs(_np(eng.sarl_export('next_obs')) - g['next_obs']).max() == 0.0
    assert np.abs(_np(eng.sarl_export('X')) - g['inputs']).max() <= 5e-6
    assert np.abs(_np(eng.sarl_export('V')) - g['net_out']).max() <= 1e-6
    assert np.abs(_np(out['values']) - g['values']).max() <= 1e-6
    top2 = np.sort(g['values'], axis=1)[:, -2:]
    clear = (top2[:, 1] - top2[:, 0]) > 4e-6
    assert clear.sum() >= n // 4
    assert np.array_equal(_np(out['best'])[clear], g['best'][clear]) and np.array_equal(_np(out['action'])[clear], g['action'][clear])
    if query_env:  # reward[b, a] is cn_step(action a, update = false)'s
        for a in range(0, len(g['action_space']), 9):
            step = eng.step(np.tile(g['action_space'][a], (n, 1)), update=False, want_obs=False)
            assert _same_bits(reward[:, a], _np(step['reward'])), a


@pytest.mark.parametrize('query_env', [True, False], ids=['query', 'noquery'])
def test_sarl_sample_step_vs_reference(amd, query_env):
    """One cn_sarl_sample_step (epsilon 0) on the fixtures' states: where the decision is clear, the transition is the reference's."""
    import torch
    g = load_golden('sarl_settings_query.npz' if query_env else 'sarl_settings_noquery.npz')
    eng, c = _sarl_engine(amd, g, query_env)
    B, H, dev = len(g['states']), 5, eng.device
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
    traj, rew, info, dmin, act = z((B, 1, H, 13), torch.float32), z((1, B), torch.float64), z((1, B), torch.uint8), z((1, B), torch.float64), z((1, B), torch.int32)
    alive, done, action = torch.ones(B, dtype=torch.uint8, device=dev), z((B,), torch.uint8), z((B, 2), torch.float64)
    step = eng.sarl_sampler(traj, rew, info, dmin, act, alive, done, action)
    step(0, 0.0)
    eng.sync()
    top2 = np.sort(g['values'], axis=1)[:, -2:]
    clear = (top2[:, 1] - top2[:, 0]) > 4e-6
    assert clear.sum() >= B // 4
    assert np.array_equal(_np(act)[0][clear], g['best'][clear])
    assert np.array_equal(_np(rew)[0][clear], g['step_reward'][clear]) and np.array_equal(_np(info)[0][clear], g['step_info'][clear])
    state, gtime = (_np(x) for x in eng.get_state())
    assert np.array_equal(state[clear], g['next_states'][clear])
    assert np.array_equal(gtime[clear], (g['gtime'] + c['time_step'])[clear])


# ------------------------------------------------------------------------------------------------ g. planners
PLAN_SEED = (0x1234 << 32) | 0x9abcdef1
DRAW_BOUND = 4 * 5.551e-17  # test_plan.py's bound on |device - reference| / max(1, r std) of a drawn component


def test_planners_clip_to_the_robot_s_v_pref(amd, oracle_mod):
    """Under `speeds` (robot_v_pref 0.7): plan_reset's prior and plan_draw against plan_reference fed the engine's dt and v_pref;
    plan_cem is draw + lookahead + refit and plan_mppi draw + lookahead + update, and the action MPPI returns is the updated
    mean's first row clipped to 0.7."""
    import torch
    s = cases.BY_NAME['speeds']
    eng, state, gtime, c = _lookahead_scene(amd, oracle_mod, s)
    B, K, n, E, v = len(state), 70, 4, 5, c['robot_v_pref']
    assert np.all(state[:, 0, 7] == v) and v < 1.0
    plan = eng.plan_reset(eng.plan_begin(K, n, E, 1, 0.3, seed=PLAN_SEED))
    mean, std = plan_ref.reset(state, c['time_step'], np.zeros((B, n, 2)), np.zeros((B, n, 2)), 0.3)
    assert _same_bits(_np(plan.mean), mean) and _same_bits(_np(plan.std), std)
    assert np.abs(np.hypot(mean[..., 0], mean[..., 1]) - v).max() <= 1e-12  # full speed is v_pref, not 1
    got = _np(eng.plan_draw(plan, 11))
    want = plan_ref.draw(mean, std, K, PLAN_SEED, 11, v)
    _, _, r = plan_ref.normal_pairs(B, K, n, PLAN_SEED, 11)
    assert (np.abs(got - want) / np.maximum(1.0, r[..., None] * std[:, None])).max() <= DRAW_BOUND
    norm = np.hypot(got[..., 0], got[..., 1])
    assert norm.max() <= v * (1 + 1e-12) and (norm >= v * (1 - 1e-12)).sum() > K  # many rows clipped, onto 0.7
    for mppi in (False, True):
        one, parts = (eng.plan_reset(eng.plan_begin(K, n, E, 1, 0.3, seed=PLAN_SEED)) for _ in range(2))
        if mppi:
            eng.plan_mppi(one, 0.05, 21)
        else:
            eng.plan_cem(one, 21)
        cand = eng.plan_draw(parts, 21)
        look = eng.lookahead(cand)
        for k, t in look.items():
            parts.look[k].copy_(t)
        if mppi:
            eng.plan_mppi_update(parts, 0.05)
        else:
            eng.plan_refit(parts)
        eng.sync()
        for k, t in parts.tensors().items():
            assert torch.equal(t, one.tensors()[k]), (mppi, k)
        if mppi:
            assert _same_bits(_np(one.action), plan_ref.clip(_np(one.mean)[:, 0], v))
        else:
            held = dict(best_actions=np.zeros((B, n, 2)), best_score=np.zeros(B), action=np.zeros((B, 2)))
            want = plan_ref.refit(_np(look['ret']), _np(cand), mean, std, E=E, keep_best=False, smoothing=0.0, min_std=0.0, **held)
            for k in ('order', 'best_actions', 'best_score', 'action', 'mean', 'std'):
                assert _same_bits(_np(getattr(one, k)), want[k]), k


# ------------------------------------------------------------------------------------------------ h. the gym side
@pytest.mark.parametrize('tag,visible', [('invisible', False), ('visible', True)])
@pytest.mark.parametrize('s', [x for x in FIXTURES if x.humans == 5], ids=cases.setting_id)
def test_gym_surface_takes_the_overrides_and_replays_the_episodes(amd, s, tag, visible):
    """compat.CrowdSim.configure on a RawConfigParser that carries the fixture's overrides: the engine config it builds holds the
    fixture's keywords, and reset / robot.act / step replay the fixture's episodes (a fresh env and policy per case, as the fixture
    was made)."""
    import json
    import crowdnav_amd.compat as c
    g = load_golden(cases.fixture_name(s))
    overrides = json.loads(str(g['overrides_json']))
    safety = overrides.pop('robot_policy.safety_space', None)
    ov = {tuple(k.split('.')): v for k, v in overrides.items()}
    ov[('robot', 'visible')] = 'true' if visible else 'false'
    ov[('sim', 'human_num')] = int(g['num_humans'])
    for case, e in zip(g['cases'].tolist(), cases.episodes(g, tag)):
        cfg = c.default_env_config(ov)
        env = c.CrowdSim()
        env.configure(cfg)
        robot = c.Robot(cfg, 'robot')
        policy = c.ORCA()
        if safety is not None:
            policy.safety_space = safety
        robot.set_policy(policy)
        env.set_robot(robot)
        policy.set_env(env)
        built = env.engine_config(1, env.human_num, env.test_sim, 1)
        for k, v in cases.fixture_config(g).items():
            assert built[k] == v, k
        ob = env.reset('test', case)
        assert abs(ob[0].px - e['states'][0][1][0]) <= 1e-12
        env._eng.set_state(e['states'][:1], np.zeros(1))  # the reference's exact initial state
        env._pull()
        ob = [h.get_observable_state() for h in env.humans]
        for t in range(len(e['actions'])):
            action = robot.act(ob)
            assert (action.vx, action.vy) == tuple(e['actions'][t])
            ob, reward, done, info = env.step(action)
            assert reward == e['rewards'][t] and done == bool(e['dones'][t])
            assert type(info).__name__ == ('Nothing', 'Danger', 'ReachGoal', 'Collision', 'Timeout')[e['infos'][t]]
            assert np.array_equal(np.array([[h.px, h.py, h.vx, h.vy] for h in env.humans]), e['states'][t + 1][1:, :4])
            assert (robot.px, robot.py) == tuple(e['states'][t + 1][0, :2])
            assert env.global_time == e['times'][t]
        assert done
