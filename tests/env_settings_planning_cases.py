"""Environment settings other than the shipped env.config through the kernels that came after the settings suite, shared by
test_env_settings_planning_host.py (CPU) and test_env_settings_planning.py (GPU): cn_predict, cn_predict_orca,
cn_predict_orca_robot, cn_lookahead_modes, the goal-progress term, the unicycle planners and the one-call closed loops on
predicted futures.  The entries are env_setting_cases'; here are the scenes each call is taken through at them, stated on the
CPU oracle and the host restatements alone, so that the host suite can assert what every scene must contain.  numpy only (the
engine a helper builds comes from the `amd` module its caller hands in)."""
import math

import numpy as np

import env_setting_cases as settings
import plan_predict_cases as predict_cases
import plan_unicycle_cases as uni_cases
import predict_orca_cases as orca_cases
import predict_orca_robot_cases as robot_cases

B, GAMMA = 3, settings.GAMMA
N_TABLE = orca_cases.N             # the predictor tables' 12 steps
SHAPES = [(5, 33), (70, 4)]        # (K, n) of the lookaheads
M = 3
GOAL_WEIGHT = 0.1

PREDICT_ENTRIES = ('dt_inexact', 'dt_fifth_square', 'speeds', 'random_attributes')
ORCA_ENTRIES = ('near_sighted', 'radii_rewards', 'speeds', 'dt_inexact', 'random_attributes', 'H12_small', 'H20_shard',
                'H20_five_neighbours')
ORCA_KEYS = ('time_step', 'neighbor_dist', 'max_neighbors', 'time_horizon', 'human_safety_space')  # what cn_predict_orca reads of cn_config
ROBOT_SEEN_ENTRIES = ('radii_rewards', 'near_sighted', 'dt_inexact', 'speeds')
ROBOT_ENTRIES = ('dt_inexact', 'speeds', 'radii_rewards')  # the lookaheads' (test_env_settings.py's too)
CROWD = {5: 'h5', 12: 'h12', 20: 'h20'}

# (f) one unicycle engine: a time step that is no binary fraction and a slow robot
UNICYCLE = dict(time_step=0.1, time_limit=12.0, robot_v_pref=0.7)
ROTATION, STD_ROTATION = math.pi / 4, 0.2
# (g) the closed loops: five-step episodes that end and re-seed inside the call
LOOP = dict(time_step=0.2, time_limit=2.0, robot_v_pref=0.7, human_v_pref=1.4)
LOOP_EPISODES = 5
UNICYCLE_LOOP = dict(UNICYCLE, time_limit=1.5)  # Timeout from 0.5 s on: five-step episodes at dt = 0.1


def whole(s):
    return settings.whole_config(s.config)


# ------------------------------------------------------------------------------------------------ states off the oracle
def oracle_state(oracle_mod, s, seconds, envs=B, **extra):
    """(state8 [envs, A, 8], global_time [envs]) of the entry: the oracle's reset of the 'test' seeds moved on by `seconds` of
    its ORCA robot under the entry's own settings."""
    o = oracle_mod.CrowdOracle(num_envs=envs, robot_policy=1, **settings.engine_config(s, robot_visible=1, **extra))
    o.reset(settings.seeds(s, envs))
    for _ in range(int(round(seconds / whole(s)['time_step']))):
        o.step(None, update=True)
    return o.get_state()


def lookahead_state(oracle_mod, s, envs=B, near_goal=False, **extra):
    """The lookaheads' scene: 3 s on (the crowd is about to meet), env 0's clock two and a half steps short of the Timeout rule.
    near_goal: the goal of env 1's robot is put its radius and one and a half full-speed steps straight ahead of it, so that
    the candidate that walks straight on arrives at its second step (the scene as the oracle leaves it has no ReachGoal branch).
    Returns (state8, global_time, the entry's whole config)."""
    state, gtime = oracle_state(oracle_mod, s, 3.0, envs, **extra)
    c = whole(s)
    gtime = gtime.copy()
    gtime[0] = c['time_limit'] - 1.0 - 2.5 * c['time_step']
    if near_goal:
        state = state.copy()
        state[1, 0, 4:6] = state[1, 0, 0:2] + [0.0, state[1, 0, 6] + 1.5 * c['robot_v_pref'] * c['time_step']]
    return state, gtime, c


def lookahead_scene(amd, oracle_mod, s, B=B, near_goal=False, **extra):
    """An external-robot engine of the entry that holds lookahead_state(): (engine, state8, global_time, whole config)."""
    state, gtime, c = lookahead_state(oracle_mod, s, B, near_goal, **extra)
    eng = amd.BatchedCrowdSim(num_envs=B, robot_policy=amd.ROBOT_EXTERNAL, **settings.engine_config(s, robot_visible=1, **extra))
    eng.set_gamma(GAMMA)
    eng.set_state(state, gtime)
    return eng, state, gtime, c


def action_table(B, K, n, v_pref, seed=3):
    """[B, K, n, 2]: seeded rows inside the square of side 2 v_pref; candidate 0 walks straight on at v_pref."""
    rng = np.random.RandomState(seed)
    t = rng.uniform(-1.0, 1.0, (B, K, n, 2)) * v_pref
    t[:, 0] = [0.0, v_pref]
    return t


# ------------------------------------------------------------------------------------------------ a. cn_predict
def predict_state(oracle_mod, s):
    """6 s on: humans at their goals, humans about to land and humans under way; the last env holds the crafted scene whose
    `exact` human stands v_pref dt (the float64 product) from its goal at the entry's dt and human v_pref."""
    state, gtime = oracle_state(oracle_mod, s, 6.0)
    c = whole(s)
    seeded = state.copy()
    state[B - 1] = predict_cases.crafted_state(s.humans, c['time_step'], c['human_v_pref'])
    return state, gtime, seeded


def host_table(state8, n, dt, models):
    """crowdnav_amd.predict's table: [B, n, H, 2] for a name, [B, M, n, H, 2] for a sequence of names."""
    from crowdnav_amd import predict
    one = lambda name: predict.constant_velocity(state8, n) if name == 'cv' else predict.to_goal(state8, n, dt)  # noqa: E731
    return one(models) if isinstance(models, str) else predict.stack_modes(*(one(name) for name in models))


def landing_misses(state8, n, dt):
    """(landing steps, those whose p + (d / dt) dt is not the goal's bits) over the to_goal table of [B, A, 8]."""
    from crowdnav_amd import predict
    state8 = np.asarray(state8, dtype=np.float64)
    table = predict.to_goal(state8, n, dt)
    p, goal, v_pref = state8[:, 1:, 0:2].copy(), state8[:, 1:, 4:6], state8[:, 1:, 7]
    landings = misses = 0
    for t in range(n):
        d = goal - p
        dist = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])
        lands = (dist > 0.0) & (dist <= v_pref * dt)
        p = p + table[:, t] * dt
        landings += int(lands.sum())
        misses += int((lands & (p != goal).any(axis=-1)).sum())
    return landings, misses


# ------------------------------------------------------------------------------------------------ b. c. the ORCA predictors
ORCA_SECONDS = 1.0
# 1 s on, the crowd is still spread over the circle: at 5 humans the cut by distance, the cut by count and the horizon all bite
# there (from 3 s on near_sighted's neighbor_dist no longer does).  The 20 humans of the H20 entries start 2.8 m apart on a 9 m
# circle and have not met by then — neighbor_dist and max_neighbors change no bit, no solve takes the 3-D fallback — so those
# entries are ALSO taken 3 s on, where they have.
ORCA_SCENES = {'H20_shard': (ORCA_SECONDS, 3.0), 'H20_five_neighbours': (ORCA_SECONDS, 3.0)}


def orca_scenes(name):
    """The scene times of an entry: every entry is taken 1 s on."""
    return ORCA_SCENES.get(name, (ORCA_SECONDS,))


def orca_state(oracle_mod, s, seconds=ORCA_SECONDS):
    return oracle_state(oracle_mod, s, seconds)


def orca_table(oracle_mod, s, state, gtime, n=N_TABLE, **put_back):
    """predict_orca_cases.oracle_table under the entry's settings, oracle-only keys included; put_back: keys over them."""
    return orca_cases.oracle_table(oracle_mod, CROWD[s.humans], state, gtime, n, **dict(s.config, **put_back))


def robot_sequences(s, unicycle=False):
    """predict_orca_robot_cases.sequences() scaled by the entry's robot_v_pref (a unicycle's rotation is left as it is)."""
    a = robot_cases.sequences(unicycle=unicycle)
    a[..., 0] *= whole(s)['robot_v_pref']
    if not unicycle:
        a[..., 1] *= whole(s)['robot_v_pref']
    return a


def robot_table(oracle_mod, s, placed, gtime, actions, **kw):
    return robot_cases.oracle_table(oracle_mod, CROWD[s.humans], placed, gtime, actions, **dict(s.config, **kw))


# ------------------------------------------------------------------------------------------------ d. e. modes and the goal term
def mode_tables(state, n, c, humans, seed=9):
    """[B, 3, n, H, 2]: constant velocity, to_goal at the entry's dt, and seeded rows inside the disc of the humans' v_pref."""
    from crowdnav_amd import predict
    rand = np.random.RandomState(seed).uniform(-1.0, 1.0, (len(state), n, humans, 2)) * c['human_v_pref'] / math.sqrt(2.0)
    return predict.stack_modes(predict.constant_velocity(state, n), predict.to_goal(state, n, c['time_step']), rand)


_MODES = {}


def modes_case(oracle_mod, name, K, n):
    """(state8, gtime, whole config, actions, human_vel, lookahead_modes_reference.per_mode's dict) of an entry and shape,
    computed once and shared; left unchanged."""
    import lookahead_modes_reference as ref
    if (name, K, n) not in _MODES:
        s = settings.BY_NAME[name]
        state, gtime, c = lookahead_state(oracle_mod, s, near_goal=True)
        table, vel = action_table(B, K, n, c['robot_v_pref']), mode_tables(state, n, c, s.humans)
        _MODES[name, K, n] = (state, gtime, c, table, vel, ref.per_mode(state, gtime, table, vel, c, GAMMA))
    return _MODES[name, K, n]


def goal_terms(w, state, end_xy):
    """lookahead_goal_reference.goal_term of every branch: state [B, A, 8], end_xy [B, K, 2] -> [B, K]."""
    from lookahead_goal_reference import goal_term
    out = np.zeros(end_xy.shape[:2])
    for b in range(end_xy.shape[0]):
        for k in range(end_xy.shape[1]):
            out[b, k] = goal_term(w, state[b, 0, 0:2], state[b, 0, 4:6], end_xy[b, k])
    return out


# ------------------------------------------------------------------------------------------------ f. the unicycle prior
def prior_robots(state8):
    """plan_unicycle_cases' robots installed over a state whose robot rows carry the engine's v_pref: (state8, theta)."""
    return uni_cases.install(state8)


def prior_errors(device, state8, theta, dt, R, n):
    """Per robot: (E_numpy, E_device), the largest component difference of the float64 restatement and of `device` ([B, n, 2],
    None: not measured) from the recurrence restated in np.longdouble on the same float64 inputs."""
    import plan_unicycle_reference as uni
    assert np.finfo(np.longdouble).eps < 2.0 ** -60, 'np.longdouble is no wider than float64 here'
    truth = uni.prior(state8, theta, dt, R, n, real=np.longdouble)
    assert truth.dtype == np.longdouble
    e_numpy = np.abs(uni.prior(state8, theta, dt, R, n).astype(np.longdouble) - truth).max(axis=(1, 2)).astype(np.float64)
    if device is None:
        return e_numpy, None
    return e_numpy, np.abs(np.asarray(device, np.float64).astype(np.longdouble) - truth).max(axis=(1, 2)).astype(np.float64)
