"""The table of environment settings (env_setting_cases.py) on the CPU: the predicate behind every entry's `why`, every changed
key live and every claimed outcome present in the oracle's own runs, and the oracle pinned to the unmodified reference at these
settings by the fixtures tests/golden/settings_<name>.npz (oracle/gen_golden_settings.py)."""
import json
import math

import numpy as np
import pytest

import env_setting_cases as cases
from conftest import load_golden

FIXTURES = cases.fixture_settings()
_accumulated, _episodes, flat = cases.accumulated, cases.episodes, cases.flat


def _is_binary_fraction(x):
    return float(x * 2 ** 20).is_integer()


def test_table_names_known_keys_and_changes_each():
    for s in cases.SETTINGS:
        assert s.config and set(s.config) <= set(cases.SHIPPED), s.name
        assert all(s.config[k] != cases.SHIPPED[k] for k in s.config), s.name
        assert set(s.oracle_only) <= set(s.config) and 3 <= s.envs <= 48 and s.steps <= 250
        assert set(cases.reference_config(s)) <= set(cases.REFERENCE_KEY)
        assert cases.config_from_overrides(cases.reference_overrides(cases.reference_config(s))) == cases.reference_config(s)


@pytest.mark.parametrize('name', ['dt_inexact', 'dt_fifth_square'])
def test_dt_is_inexact_and_accumulation_parts_from_the_product(name):
    s = cases.BY_NAME[name]
    dt, limit = s.config['time_step'], s.config.get('time_limit', cases.SHIPPED['time_limit'])
    assert not _is_binary_fraction(dt)
    steps = int(math.ceil(limit / dt))
    assert any(_accumulated(dt, k) != k * dt for k in range(1, steps + 1))
    assert _is_binary_fraction(cases.SHIPPED['time_step'])  # what the shipped value hides


def test_speeds_separate_the_preferred_speed_from_v_pref_and_move_the_discount(oracle_mod):
    """orca.py:111-115: the preferred velocity of a goal further than 1 away is the unit vector whatever v_pref is, and maxSpeed is
    v_pref.  On the oracle: a lone human (robot invisible, far away) 6 m from its goal takes speed 1 — not its v_pref of 1.4 — and
    the ORCA robot, whose v_pref is 0.7 < 1, is held to 0.7 by maxSpeed.  Clipping the preferred velocity to v_pref instead
    would move the human at 1.4."""
    s = cases.BY_NAME['speeds']
    hv, rv = s.config['human_v_pref'], s.config['robot_v_pref']
    assert hv > 1.0 > rv  # one on either side of the clip at speed 1
    st = np.zeros((1, 2, 8))
    st[0, 0] = [50.0, 50.0, 0.0, 0.0, 53.0, 54.0, 0.3, rv]
    st[0, 1] = [0.0, 0.0, 0.0, 0.0, 3.6, 4.8, 0.3, hv]
    o = oracle_mod.CrowdOracle(num_envs=1, num_humans=1, robot_policy=1, robot_visible=0, **s.config)
    o.set_state(st, np.zeros(1))
    v = o.orca()[0].astype(np.float64)
    assert abs(np.hypot(*v[1]) - 1.0) <= 1e-6 and abs(np.hypot(*v[0]) - rv) <= 1e-6
    assert abs(np.hypot(*v[1]) - hv) > 0.3
    dt = cases.SHIPPED['time_step']
    assert all(t * dt * rv != t * 0.25 for t in range(1, 100))  # the discount exponent is not t / 4


def test_near_sighted_cuts_by_count_and_by_distance(oracle_mod):
    """Some candidate lies beyond 3 m on the start states, and within the first 30 steps of the entry's run from them some agent of
    a running episode has more than 3 candidates inside 3 m."""
    s = cases.BY_NAME['near_sighted']
    st = cases.start_states(oracle_mod, s)
    d = np.linalg.norm(st[:, :, None, :2] - st[:, None, :, :2], axis=-1)
    d[:, np.arange(s.humans + 1), np.arange(s.humans + 1)] = np.inf
    # (on the start states themselves — agents spread over the 4 m circle — nobody has more than 3 candidates inside 3 m: the
    # crowding is reached during the entry's own run, as the crowd meets in the middle)
    far = np.isfinite(d) & (d > s.config['neighbor_dist'])
    r = cases.run(oracle_mod, s.config, s.humans, st, 30, 1)
    pos = np.concatenate([st[None], r['state']])[..., :2]
    dd = np.linalg.norm(pos[:, :, :, None] - pos[:, :, None, :], axis=-1)
    dd[..., np.arange(s.humans + 1), np.arange(s.humans + 1)] = np.inf
    alive = np.concatenate([np.ones((1, s.envs), bool), r['info'] != 255])
    crowded = ((dd < s.config['neighbor_dist']).sum(axis=-1) > s.config['max_neighbors']) & alive[..., None]
    assert far.any() and crowded.any()


def test_table_edge_is_the_last_accepted_size():
    s = cases.BY_NAME['table_edge']
    assert math.ceil(s.config['time_limit'] / s.config['time_step']) + 8 == 256
    assert math.ceil((s.config['time_limit'] + s.config['time_step']) / s.config['time_step']) + 8 == 257
    assert _is_binary_fraction(s.config['time_step'])  # the edge itself, not dt, is what this entry is about


@pytest.mark.parametrize('name', ['H12_small', 'random_attributes'])
def test_wave_generator_entries_change_what_sizes_the_blocked_cell_table(name):
    s = cases.BY_NAME[name]
    assert s.humans > 8  # the wave generators are the default above 8 humans
    if name == 'H12_small':
        c = dict(cases.SHIPPED, **s.config)
        assert c['circle_radius'] + c['human_v_pref'] / 2 != 4.5 and 2 * c['human_radius'] + c['discomfort_dist'] != 0.8
    else:
        assert s.config['randomize_attributes'] == 1


def test_shard_entries_differ_in_max_neighbors_alone():
    a, b = cases.BY_NAME['H20_shard'], cases.BY_NAME['H20_five_neighbours']
    assert dict(a.config, max_neighbors=5) == b.config and 'max_neighbors' not in a.config
    every = set(cases.SHIPPED) - {'max_neighbors', 'scenario_rule', 'square_width', 'randomize_attributes'}
    assert set(a.config) == every  # non-default everywhere a circle crossing with fixed attributes reads


# ------------------------------------------------------------------------------------------------ every key live, every claim present
def _runs(oracle_mod, s, config, state0):
    return [cases.run(oracle_mod, config, s.humans, state0, s.steps, vis, still) for vis, still in ((0, False), (1, False), (1, True))]


@pytest.fixture(scope='module')
def entry_runs(oracle_mod):
    cache = {}

    def get(s):
        if s.name not in cache:
            st = cases.start_states(oracle_mod, s)
            cache[s.name] = (st, _runs(oracle_mod, s, s.config, st))
        return cache[s.name]
    return get


@pytest.mark.parametrize('s', cases.SETTINGS, ids=cases.setting_id)
def test_every_changed_key_is_live(oracle_mod, entry_runs, s):
    """One key back at its shipped value: some bit of reward, info, dmin, time or state changes within the entry's steps, in a run
    with the ORCA robot (invisible or visible) or with the robot standing aside.  A key the generator reads is put back in the
    reset too, and an attribute that lives in the state rows (radius, v_pref) is ALSO put back in the entry's own start states
    alone, where everything but those two columns is compared."""
    st, want = entry_runs(s)
    for key in s.config:
        config = {k: v for k, v in s.config.items() if k != key}
        start = st
        if key in cases.GENERATOR_KEYS:
            o = oracle_mod.CrowdOracle(num_envs=s.envs, num_humans=s.humans, **config)
            o.reset(cases.seeds(s))
            start = o.get_state()[0]
        got = _runs(oracle_mod, s, config, start)
        assert not all(cases.same(a, b) for a, b in zip(got, want)), key
        column = {'human_radius': (slice(1, None), 6), 'robot_radius': (0, 6), 'human_v_pref': (slice(1, None), 7), 'robot_v_pref': (0, 7)}.get(key)
        if column and not s.config.get('randomize_attributes'):
            start = st.copy()
            start[:, column[0], column[1]] = cases.SHIPPED[key]
            got = _runs(oracle_mod, s, config, start)
            strip = lambda r: dict(r, state=r['state'][..., :6])  # noqa: E731
            assert not all(cases.same(strip(a), strip(b)) for a, b in zip(got, want)), key


@pytest.mark.parametrize('s', cases.SETTINGS, ids=cases.setting_id)
def test_every_claimed_outcome_occurs(entry_runs, s):
    _, runs = entry_runs(s)
    seen = np.concatenate([r['info'].ravel() for r in runs[:2]])
    for claim in s.claims:
        assert (seen == cases.INFO[claim]).any(), claim
    assert (runs[2]['info'] == cases.INFO['timeout']).any() or s.steps * s.config.get('time_step', 0.25) < s.config.get('time_limit', 25.0) - 1
    if s.name == 'table_edge':  # the still robot's episode is the longest the discount table holds
        info = runs[2]['info']
        assert np.all(info[240] == cases.INFO['timeout']) and np.all(info[:240] != cases.INFO['timeout']) and len(info) == 241


# ------------------------------------------------------------------------------------------------ the oracle against the reference
@pytest.mark.parametrize('s', FIXTURES, ids=cases.setting_id)
def test_fixture_carries_the_table_entry(s):
    g = load_golden(cases.fixture_name(s))
    assert cases.fixture_config(g) == dict(cases.reference_config(s), num_humans=s.humans)
    assert cases.config_from_overrides(json.loads(str(g['overrides_json']))) == cases.reference_config(s)
    assert len(g['cases']) == s.cases and 4 <= s.cases <= 6
    dt = s.config.get('time_step', 0.25)
    for tag in ('invisible', 'visible'):
        for e in _episodes(g, tag):
            assert e['times'][-1] == _accumulated(dt, len(e['times']))  # accumulated, step by step
    if s.name == 'dt_inexact':
        t = g['invisible_times']
        assert (t != np.round(t / dt) * dt).any() and (g['invisible_infos'] == cases.INFO['timeout']).any()


@pytest.mark.parametrize('tag,visible', [('invisible', 0), ('visible', 1)])
@pytest.mark.parametrize('s', FIXTURES, ids=cases.setting_id)
def test_oracle_teacher_forced_bit_exact(oracle_mod, s, tag, visible):
    g = load_golden(cases.fixture_name(s))
    before, after, t0, t1 = flat(g, tag)
    o = oracle_mod.CrowdOracle(num_envs=len(before), robot_policy=1, robot_visible=visible, **cases.fixture_config(g))
    o.set_state(before, t0)
    out = o.step(None, update=True)
    state, gt = o.get_state()
    for k, name in (('reward', 'rewards'), ('done', 'dones'), ('info', 'infos'), ('action', 'actions')):
        assert np.array_equal(out[k], g['%s_%s' % (tag, name)]), k
    danger = g[tag + '_infos'] == 1
    assert np.array_equal(out['dmin'][danger], g[tag + '_dmins'][danger])
    assert np.array_equal(state, after)
    assert np.array_equal(gt, t1)


@pytest.mark.parametrize('tag,visible', [('invisible', 0), ('visible', 1)])
@pytest.mark.parametrize('s', FIXTURES, ids=cases.setting_id)
def test_oracle_free_running_bit_exact(oracle_mod, s, tag, visible):
    g = load_golden(cases.fixture_name(s))
    for e in _episodes(g, tag):
        o = oracle_mod.CrowdOracle(num_envs=1, robot_policy=1, robot_visible=visible, **cases.fixture_config(g))
        o.set_state(e['states'][:1], np.zeros(1))
        for t in range(len(e['actions'])):
            out = o.step(None, update=True)
            assert out['reward'][0] == e['rewards'][t] and out['done'][0] == e['dones'][t] and out['info'][0] == e['infos'][t]
            state, gt = o.get_state()
            assert np.array_equal(state[0], e['states'][t + 1]) and gt[0] == e['times'][t]
        assert out['done'][0] == 1


@pytest.mark.parametrize('s', FIXTURES, ids=cases.setting_id)
def test_oracle_reset_matches_reference_generator(oracle_mod, s):
    g = load_golden(cases.fixture_name(s))
    want, seeds = g['reset_states'], g['reset_seeds']
    o = oracle_mod.CrowdOracle(num_envs=len(seeds), **cases.fixture_config(g))
    draws = o.reset(seeds)
    got, gt = o.get_state()
    assert np.all(gt == 0.0) and np.abs(got - want).max() <= 1e-12
    assert np.array_equal(got[:, :, 6:], want[:, :, 6:]) and np.array_equal(got[:, 0], want[:, 0])
    for b, seed in enumerate(seeds):  # the stream stands where the reference's stood: the next value is the probe
        assert oracle_mod.mt_random(int(seed), int(draws[b]) + 1)[-1] == g['reset_probe'][b]


# ------------------------------------------------------------------------------------------------ the SARL fixtures at these settings
def test_sarl_fixtures_carry_the_settings():
    want = cases.reference_overrides(cases.sarl_env_config())
    for name in ('sarl_settings_query.npz', 'sarl_settings_noquery.npz'):
        g = load_golden(name)
        assert json.loads(str(g['env_overrides_json'])) == json.loads(json.dumps(want))
        assert g['states'].shape == (12, 6, 8) and g['gtime'][1] == cases.accumulated(0.1, 7)  # 2 cases x 6 decisions, from step 6 on
        assert np.all(g['states'][:, 1:, 6] == 0.4) and np.all(g['states'][:, 0, 6] == 0.2)


def _compute_reward(robot, humans, action, dt, collision, success, discomfort, factor):
    """multi_human_rl.py:65-88 on the constant-velocity next states, with the four constants as arguments."""
    nav = robot[:2] + action * dt
    nh = humans[:, :2] + humans[:, 2:4] * dt
    dmin = np.inf
    for h, p in zip(humans, nh):
        dist = np.linalg.norm((nav[0] - p[0], nav[1] - p[1])) - robot[6] - h[6]
        if dist < 0:
            return collision
        dmin = min(dmin, dist)
    if np.linalg.norm((nav[0] - robot[4], nav[1] - robot[5])) < robot[6]:
        return success
    return (dmin - discomfort) * factor * dt if dmin < discomfort else 0


def test_noquery_fixture_tells_hard_coded_constants_from_the_config():
    """With query_env = false the reference's rewards are compute_reward's with ITS constants (-0.25, 1, 0.2, 0.5); of the rows
    where either reading gives a non-zero reward, more than half differ from what [reward]'s values would give."""
    g = load_golden('sarl_settings_noquery.npz')
    c = cases.sarl_env_config()
    dt = c['time_step']
    hard = np.zeros(g['rewards'].shape)
    read = np.zeros(g['rewards'].shape)
    for d, st in enumerate(g['states']):
        for a, act in enumerate(g['action_space']):
            hard[d, a] = _compute_reward(st[0], st[1:], act, dt, -0.25, 1, 0.2, 0.5)
            read[d, a] = _compute_reward(st[0], st[1:], act, dt, c['collision_penalty'], c['success_reward'], c['discomfort_dist'],
                                         c['discomfort_penalty_factor'])
    assert np.array_equal(g['rewards'], hard)
    nonzero = g['rewards'] != 0
    assert nonzero.sum() >= 20 and (g['rewards'] != read)[nonzero].sum() * 2 > nonzero.sum()
    q = load_golden('sarl_settings_query.npz')  # the query fixture has rewards to compare too (the GPU test holds them against cn_step)
    assert (q['rewards'] != 0).sum() >= 20
