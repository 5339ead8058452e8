"""The scenes of test_env_settings_planning.py (env_settings_planning_cases.py) on the CPU: what each one must contain for its
bit-for-bit comparison on the device to mean something, asserted on the CPU oracle and on the host restatements alone, and that
the restatements given a dt / v_pref form keep the bits their earlier callers got.  The liveness checks follow
test_env_settings_host.py: one key back at its shipped value alone, and some bit of the call's own output changes."""
import math

import numpy as np
import pytest

import env_setting_cases as settings
import env_settings_planning_cases as cases
import lookahead_cv_reference as cv
import lookahead_modes_reference as modes_ref
import plan_predict_cases as predict_cases
import plan_reference as plan_ref
import plan_unicycle_cases as uni_cases
import plan_unicycle_reference as uni
import predict_orca_robot_cases as robot_cases

BY_NAME, SHIPPED = settings.BY_NAME, settings.SHIPPED


def _differ(a, b):
    return np.asarray(a).tobytes() != np.asarray(b).tobytes()


def test_the_entries_exist_and_say_what_the_scenes_need():
    for name in cases.PREDICT_ENTRIES + cases.ORCA_ENTRIES + cases.ROBOT_SEEN_ENTRIES + cases.ROBOT_ENTRIES:
        assert name in BY_NAME and BY_NAME[name].humans in cases.CROWD, name
    assert {BY_NAME[n].humans for n in cases.ORCA_ENTRIES} == {5, 12, 20}
    assert cases.N_TABLE == 12 and cases.SHAPES == [(5, 33), (70, 4)] and (cases.B, cases.M) == (3, 3)
    for c in (cases.UNICYCLE, cases.LOOP, cases.UNICYCLE_LOOP):  # dt no binary fraction, a robot slower than 1
        assert not float(c['time_step'] * 2 ** 20).is_integer() and c['robot_v_pref'] == 0.7
    assert all(c[k] != SHIPPED[k] for c in (cases.UNICYCLE, cases.LOOP) for k in c)


# ------------------------------------------------------------------------------------------------ the shared helpers keep their bits
def test_the_dt_forms_keep_the_bits_of_their_earlier_callers():
    for H in (1, 5, 12):
        old = predict_cases.crafted_state(H)
        assert old.tobytes() == predict_cases.crafted_state(H, predict_cases.DT, 1.0).tobytes()
        rows = [predict_cases.ROBOT] + [tuple(predict_cases.CRAFTED[h % 5][i] + (8.0 * (h // 5) if i in (0, 4) else 0.0) for i in range(8))
                                        for h in range(H)]
        assert old.tobytes() == np.array(rows, dtype=np.float64).tobytes()  # the rows as they were written down
    state8, theta = uni_cases.install(np.zeros((3, 6, 8)) + [0, 0, 0, 0, 0, 0, 0.3, 1.0])
    for R in uni_cases.ROTATIONS:
        a = uni.prior(state8, theta, 0.25, R, 33)
        assert a.dtype == np.float64 and a.tobytes() == uni.prior(state8, theta, 0.25, R, 33, real=np.float64).tobytes()
    assert uni.wrap(6.0) == 6.0 - uni.TWO_PI * math.floor((6.0 + uni.PI) / uni.TWO_PI) and type(uni.wrap(6.0)) is np.float64


# ------------------------------------------------------------------------------------------------ a. cn_predict
@pytest.mark.parametrize('name', cases.PREDICT_ENTRIES)
def test_predict_scene_takes_every_case_of_the_to_goal_rule(oracle_mod, name):
    s = BY_NAME[name]
    c = cases.whole(s)
    dt = c['time_step']
    state, gtime, seeded = cases.predict_state(oracle_mod, s)
    counted = predict_cases.to_goal_cases(seeded, 33, dt)
    print(name, 'seeded, n = 33:', counted, 'n = 12:', predict_cases.to_goal_cases(seeded, cases.N_TABLE, dt))
    assert counted['zero'] >= 1 and counted['short'] >= 1 and counted['cruise'] >= 1 and counted['exact'] == 0, counted
    crafted = predict_cases.to_goal_cases(state[cases.B - 1:], cases.N_TABLE, dt)
    print(name, 'crafted, dt %g, v_pref %g:' % (dt, c['human_v_pref']), crafted)
    assert all(crafted[k] >= 1 for k in predict_cases.CASES), crafted
    human = state[cases.B - 1, 2]
    assert human[0] == 0.0 and human[4] == c['human_v_pref'] * dt and human[7] == c['human_v_pref']
    landings, misses = cases.landing_misses(state, 33, dt)
    print(name, 'landing steps %d, of which p + (d / dt) dt misses the goal: %d' % (landings, misses))
    assert landings >= 1
    # dt is live for the table: the shipped one gives other bits (the landing steps and every step behind a first one)
    if dt != SHIPPED['time_step']:
        assert _differ(cases.host_table(state, cases.N_TABLE, dt, 'to_goal'), cases.host_table(state, cases.N_TABLE, SHIPPED['time_step'], 'to_goal'))
    if s.config.get('randomize_attributes'):
        assert len(np.unique(seeded[:, 1:, 7])) > s.humans  # per-human sampled v_pref


def test_the_existing_crafted_scene_loses_its_exact_row_at_other_time_steps():
    """Why the dt form exists: 0.25 = 1.0 * 0.25 is the reach at the shipped dt alone."""
    for dt in (0.1, 0.2):
        old = np.array([predict_cases.ROBOT] + list(predict_cases.CRAFTED))[None]
        assert predict_cases.to_goal_cases(old, 6, dt)['exact'] == 0
        for v in (1.0, 0.8, 1.4):
            assert predict_cases.to_goal_cases(predict_cases.crafted_state(5, dt, v)[None], 6, dt)['exact'] >= 1, (dt, v)


# ------------------------------------------------------------------------------------------------ b. cn_predict_orca
@pytest.fixture(scope='module')
def orca_tables(oracle_mod):
    cache = {}

    def get(name, seconds=cases.ORCA_SECONDS):
        if (name, seconds) not in cache:
            s = BY_NAME[name]
            state, gtime = cases.orca_state(oracle_mod, s, seconds)
            cache[name, seconds] = (state, gtime) + cases.orca_table(oracle_mod, s, state, gtime)
        return cache[name, seconds]
    return get


@pytest.mark.parametrize('name', cases.ORCA_ENTRIES)
def test_every_key_the_orca_predictor_reads_is_live(oracle_mod, orca_tables, name):
    """Every key of cn_config the predictor reads that the entry changes, put back alone, changes some bit of the table of one
    of the entry's scenes — of the scene 1 s on wherever the entry has no other."""
    s = BY_NAME[name]
    keys = [k for k in cases.ORCA_KEYS if k in s.config]
    assert keys or name in ('speeds', 'H12_small')  # (those two change what lies in the state rows alone)
    assert cases.orca_scenes(name)[0] == cases.ORCA_SECONDS
    live = set()
    for seconds in cases.orca_scenes(name):
        state, gtime, want, fallback, done = orca_tables(name, seconds)
        assert want.shape == (cases.B, cases.N_TABLE, s.humans, 2) and np.isfinite(want).all()
        here = {k for k in keys if _differ(cases.orca_table(oracle_mod, s, state, gtime, **{k: SHIPPED[k]})[0], want)}
        print(name, '%g s on: live' % seconds, sorted(here), 'of', keys, 'fallback solves', int(fallback.sum()), 'rows behind done', int(done.sum()))
        live |= here
        for column, key in ((6, 'human_radius'), (7, 'human_v_pref')):  # what the state rows carry: put back there
            if key in s.config and not s.config.get('randomize_attributes'):
                other = state.copy()
                other[:, 1:, column] = SHIPPED[key]
                assert _differ(cases.orca_table(oracle_mod, s, other, gtime)[0], want), key
    assert live == set(keys), (sorted(live), keys)


def test_some_orca_table_takes_the_3d_fallback(orca_tables):
    counts = {(name, sec): int(orca_tables(name, sec)[3].sum()) for name in cases.ORCA_ENTRIES for sec in cases.orca_scenes(name)}
    print(counts)
    assert sum(n > 0 for n in counts.values()) >= 3 and counts['H20_shard', 3.0] > 0 and counts['near_sighted', 1.0] > 0


def test_the_robot_s_safety_space_is_not_read_by_the_unseen_robot_table(oracle_mod, orca_tables):
    s = BY_NAME['radii_rewards']
    state, gtime, want = orca_tables('radii_rewards')[:3]
    assert s.config['robot_safety_space'] == 0.15
    assert not _differ(cases.orca_table(oracle_mod, s, state, gtime, robot_safety_space=0.0)[0], want)


# ------------------------------------------------------------------------------------------------ c. cn_predict_orca_robot
@pytest.mark.parametrize('name,unicycle', [(n, False) for n in cases.ROBOT_SEEN_ENTRIES] + [('dt_inexact', True)])
def test_the_robot_seen_scenes_bite(oracle_mod, name, unicycle):
    s = BY_NAME[name]
    state, gtime = cases.orca_state(oracle_mod, s)
    placed, _, _ = robot_cases.place_robot(state)
    actions = cases.robot_sequences(s, unicycle)
    c = cases.whole(s)
    speed = np.abs(actions[..., 0]) if unicycle else np.hypot(actions[..., 0], actions[..., 1])
    assert speed.max() <= c['robot_v_pref'] * (1 + 1e-12) and speed.max() >= 0.99 * c['robot_v_pref']
    kw = dict(theta=robot_cases.THETA, robot_kinematics=1) if unicycle else {}
    if unicycle:
        assert (actions[:, :, 1] != 0.0).all() and (robot_cases.wraps(robot_cases.THETA, actions) >= 1).any()
    want, fallback, done = cases.robot_table(oracle_mod, s, placed, gtime, actions, **kw)
    unseen = robot_cases.furthest(want, cases.orca_table(oracle_mod, s, placed, gtime)[0])
    stands = robot_cases.furthest(want[:, 1:], cases.robot_table(oracle_mod, s, placed, gtime, actions, robot='stands', **kw)[0][:, 1:])
    stale = robot_cases.furthest(want, cases.robot_table(oracle_mod, s, placed, gtime, actions, robot='stale', **kw)[0])
    print(name, 'unicycle' if unicycle else 'holonomic', 'furthest from robot unseen %.3f, standing (t >= 1) %.3f, stale velocity %.3f; '
          'fallback solves %d' % (unseen, stands, stale, fallback.sum()))
    assert unseen > 1e-3 and stands > 1e-3 and stale > 1e-3
    for key in [k for k in cases.ORCA_KEYS if k in s.config]:
        assert _differ(cases.robot_table(oracle_mod, s, placed, gtime, actions, **dict(kw, **{key: SHIPPED[key]}))[0], want), key
    if name == 'radii_rewards':  # the robot's radius lies in its state row: the humans keep clear of that disc
        assert placed[0, 0, 6] == s.config['robot_radius'] != SHIPPED['robot_radius']
        other = placed.copy()
        other[:, 0, 6] = SHIPPED['robot_radius']
        assert _differ(cases.robot_table(oracle_mod, s, other, gtime, actions, robot_radius=SHIPPED['robot_radius'])[0], want)
    if unicycle:
        assert _differ(cases.robot_table(oracle_mod, s, placed, gtime, actions)[0], want)  # the rows are not read as (vx, vy)


# ------------------------------------------------------------------------------------------------ d. e. modes and the goal term
MODES_KEYS = ('time_step', 'time_limit', 'success_reward', 'collision_penalty', 'discomfort_dist', 'discomfort_penalty_factor',
              'robot_v_pref')  # what the lookahead restatements read of a config (lookahead_cv_reference.CFG)


@pytest.mark.parametrize('name', cases.ROBOT_ENTRIES)
def test_the_modes_scenes_take_every_branch_kind_and_read_the_entry_s_keys(oracle_mod, name):
    assert set(MODES_KEYS) == set(cv.CFG)
    s = BY_NAME[name]
    seen, live = np.zeros(5, int), set()
    timed_out = running = False
    for K, n in cases.SHAPES:
        state, gtime, c, table, vel, want = cases.modes_case(oracle_mod, name, K, n)
        assert vel.shape == (cases.B, cases.M, n, s.humans, 2) and want['ret'].shape == (cases.B, K, cases.M)
        seen += np.bincount(want['info'].ravel(), minlength=5)
        timed_out |= bool((want['info'] == cv.TIMEOUT).any())
        running |= bool(((want['info'] < cv.REACH_GOAL) & (want['steps'] == n)).any())
        assert (want['info'][0] == cv.TIMEOUT).any()  # env 0 stands two and a half steps short of the rule
        for key in [k for k in MODES_KEYS if k in s.config]:
            back = modes_ref.per_mode(state, gtime, table[:, :5], vel, dict(c, **{key: SHIPPED[key]}), cases.GAMMA)
            mine = {k: v[:, :5] for k, v in want.items()}
            if any(_differ(back[k], mine[k]) for k in mine):
                live.add(key)
        if name == 'speeds':  # v_pref lies in the robot's state row too, and scales the table: nothing else for it to move
            assert np.all(state[:, 0, 7] == c['robot_v_pref']) and np.abs(table).max() <= c['robot_v_pref']
        # the modes differ from each other somewhere: a kernel that scored every mode on one table fails
        assert (want['ret'].max(-1) != want['ret'].min(-1)).any() or (want['steps'].max(-1) != want['steps'].min(-1)).any()
        # the reductions have something to choose: the worst mode is not always mode 0
        red = modes_ref.reduced(want, modes_ref.weights_table(cases.B, cases.M), modes_ref.MIN, 0.5)
        assert (red['worst_mode'] != 0).any() or n == 4
    print(name, 'infos', seen.tolist(), 'live', sorted(live))
    assert timed_out and running and seen[cv.COLLISION] > 0 and seen[cv.REACH_GOAL] > 0 and seen[cv.DANGER] > 0, seen
    assert live == {k for k in MODES_KEYS if k in s.config}, live


@pytest.mark.parametrize('name', cases.ROBOT_ENTRIES)
def test_the_goal_term_moves_some_return_of_the_restatement(oracle_mod, name):
    for K, n in cases.SHAPES:
        state, gtime, c, table, _, _ = cases.modes_case(oracle_mod, name, K, n)
        want = cv.lookahead(state, gtime, table, c, cases.GAMMA)
        terms = cases.goal_terms(cases.GOAL_WEIGHT, state, want['final_state8'][:, :, 0, 0:2])
        assert ((want['ret'] + terms) != want['ret']).any() and np.isfinite(terms).all()
        assert (terms > 0).any() and (terms < 0).any()  # branches that gain on the goal and branches that lose


# ------------------------------------------------------------------------------------------------ f. the unicycle prior
def _unicycle_state():
    c = cases.UNICYCLE
    return cases.prior_robots(np.zeros((3, 6, 8)) + [0, 0, 0, 0, 0, 0, 0.3, c['robot_v_pref']])


def test_the_unicycle_prior_at_the_setting_keeps_its_turns_away_from_pi_and_reads_dt_and_v_pref():
    c = cases.UNICYCLE
    dt, v = c['time_step'], c['robot_v_pref']
    state8, theta = _unicycle_state()
    reseed = np.array([[0.0, -4.0, 0.0, 4.0, uni_cases.RESEED_THETA]] * 3)
    for robots_state, th in ((state8, theta), uni_cases.install(state8, reseed)):
        for R in uni_cases.ROTATIONS:
            turns = []
            rows = uni.prior(robots_state, th, dt, R, uni_cases.N, turns)
            assert len(turns) >= uni_cases.N and min(math.pi - abs(t) for t in turns) >= uni_cases.TURN_MARGIN, R
            assert (rows[..., 0] <= v).all() and (np.abs(rows[..., 1]) <= R).all() and (rows[..., 0] == v).any()
    for R in uni_cases.ROTATIONS:
        mine = uni.prior(state8, theta, dt, R, uni_cases.N)
        assert _differ(mine, uni.prior(state8, theta, SHIPPED['time_step'], R, uni_cases.N))  # dt is live ...
        shipped = state8.copy()
        shipped[:, 0, 7] = SHIPPED['robot_v_pref']
        assert _differ(mine, uni.prior(shipped, theta, dt, R, uni_cases.N))  # ... and so is v_pref
    assert (uni.prior(state8, theta, dt, math.pi / 4, uni_cases.N)[2, :, 0] < v).any()  # speed = dist / dt is met


@pytest.mark.parametrize('setting', ['unicycle', 'shipped'])
def test_the_long_double_restatement_measures_the_float64_one(setting):
    """E_numpy of the bound's rule: finite, tiny and — for some robots — exactly zero, which is why the rule has a floor."""
    dt, v = (cases.UNICYCLE['time_step'], cases.UNICYCLE['robot_v_pref']) if setting == 'unicycle' else (uni_cases.DT, uni_cases.V_PREF)
    state8, theta = cases.prior_robots(np.zeros((3, 6, 8)) + [0, 0, 0, 0, 0, 0, 0.3, v])
    assert np.finfo(np.longdouble).eps < 2.0 ** -60
    for R in uni_cases.ROTATIONS:
        e_numpy, none = cases.prior_errors(None, state8, theta, dt, R, uni_cases.N)
        print('%s dt %g v_pref %g R %.4f: E_numpy per robot %s' % (setting, dt, v, R, e_numpy.tolist()))
        assert none is None and e_numpy.shape == (3,) and (e_numpy < 1e-13).all()
        # the float64 restatement measured against itself is zero; against a table one ulp off it is that ulp
        exact = uni.prior(state8, theta, dt, R, uni_cases.N)
        e_self = cases.prior_errors(exact, state8, theta, dt, R, uni_cases.N)
        assert e_self[0].tobytes() == e_self[1].tobytes()
        off = exact.copy()
        off[1, 0, 1] = np.nextafter(off[1, 0, 1], 4.0)
        assert cases.prior_errors(off, state8, theta, dt, R, uni_cases.N)[1][1] >= abs(off[1, 0, 1] - exact[1, 0, 1]) / 2


# ------------------------------------------------------------------------------------------------ g. the closed loops
def test_the_loops_setting_is_live_for_the_predictor_and_the_prior(oracle_mod):
    """What the one-call loops must hand on: the to_goal table reads dt and the humans' v_pref, the holonomic prior the robot's
    v_pref — on the start states the loops' engines reset to."""
    c = settings.whole_config(cases.LOOP)
    o = oracle_mod.CrowdOracle(num_envs=cases.B, num_humans=5, **cases.LOOP)
    o.reset(1000 + np.arange(cases.B))
    state = o.get_state()[0]
    assert np.all(state[:, 0, 7] == 0.7) and np.all(state[:, 1:, 7] == 1.4)
    n = 4
    mine = cases.host_table(state, n, c['time_step'], 'to_goal')
    assert _differ(mine, cases.host_table(state, n, SHIPPED['time_step'], 'to_goal'))
    shipped = state.copy()
    shipped[:, 1:, 7] = SHIPPED['human_v_pref']
    assert _differ(mine, cases.host_table(shipped, n, c['time_step'], 'to_goal'))
    prior = plan_ref.prior(state, c['time_step'])
    assert np.abs(np.hypot(prior[:, 0], prior[:, 1]) - 0.7).max() <= 1e-12
    # the episodes of the loops end inside six steps: Timeout from time_limit - 1 on
    for cfg in (cases.LOOP, cases.UNICYCLE_LOOP):
        steps = next(k for k in range(1, 50) if settings.accumulated(cfg['time_step'], k) >= cfg['time_limit'] - 1.0)
        assert steps <= 6, (cfg, steps)
