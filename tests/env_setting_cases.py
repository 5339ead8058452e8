"""Environment settings other than the shipped env.config, shared by test_env_settings_host.py (CPU) and test_env_settings.py
(GPU): named settings, the cn_config keys each one changes, and why.

Every entry is in the table for a property of its numbers, named in `why` and checked by a predicate in
test_env_settings_host.py: moving a number is fine as long as the predicate still holds.  Two predicates hold for every entry, on
the CPU oracle: each changed key is LIVE (put back to its shipped value alone, some output bit of the entry's own run changes
within the steps the GPU tests make), and every outcome the entry claims occurs in that run.

The reference reads most keys from env.config; `oracle_only` names the keys of an entry that it cannot express (ORCA's
neighbour parameters are literals in orca.py:60-66, the humans' safety space is an attribute of policies the env creates itself):
the entry's fixture tests/golden/settings_<name>.npz (oracle/gen_golden_settings.py) is made WITHOUT them, and the device is
compared with the oracle alone where they are set."""
import collections
import json

import numpy as np

from support import environ  # noqa: F401  (the suites take it from here)

# what every key is when an entry does not change it (crowd_nav/configs/env.config + orca.py:60-66)
SHIPPED = dict(
    time_step=0.25, time_limit=25.0, success_reward=1.0, collision_penalty=-0.25, discomfort_dist=0.2,
    discomfort_penalty_factor=0.5, robot_safety_space=0.0, human_safety_space=0.0, neighbor_dist=10.0, max_neighbors=10,
    scenario_rule=0, time_horizon=5.0, circle_radius=4.0, square_width=10.0, human_radius=0.3, human_v_pref=1.0,
    robot_radius=0.3, robot_v_pref=1.0, randomize_attributes=0)

# cn_config key -> the reference's 'section.key'.  'robot_policy.safety_space' is no config entry: the attribute of the robot's
# ORCA policy that crowd_nav/train.py:122-127 sets; the generator sets it the same way.
REFERENCE_KEY = dict(
    time_step='env.time_step', time_limit='env.time_limit', randomize_attributes='env.randomize_attributes',
    success_reward='reward.success_reward', collision_penalty='reward.collision_penalty', discomfort_dist='reward.discomfort_dist',
    discomfort_penalty_factor='reward.discomfort_penalty_factor', scenario_rule='sim.test_sim', square_width='sim.square_width',
    circle_radius='sim.circle_radius', human_radius='humans.radius', human_v_pref='humans.v_pref', robot_radius='robot.radius',
    robot_v_pref='robot.v_pref', robot_safety_space='robot_policy.safety_space')
RULES = ('circle_crossing', 'square_crossing')
# keys the scenario generator reads: putting one back changes the start states themselves
GENERATOR_KEYS = ('scenario_rule', 'square_width', 'circle_radius', 'human_radius', 'human_v_pref', 'robot_radius', 'robot_v_pref',
                  'randomize_attributes', 'discomfort_dist')
INFO = dict(nothing=0, danger=1, reach_goal=2, collision=3, timeout=4)

Setting = collections.namedtuple('Setting', 'name humans config oracle_only claims envs steps cases why')

SEED_BASE, SEED_MOD = 1000, 500  # the 'test' phase's seeds (crowd_sim.py:272-276)
GAMMA = 0.95


def _s(name, humans, config, why, oracle_only=(), claims=('reach_goal',), envs=24, steps=150, cases=4):
    return Setting(name, humans, dict(config), tuple(oracle_only), tuple(claims), envs, steps, cases, why)


_H20 = dict(time_step=0.2, time_limit=30.0, success_reward=1.5, collision_penalty=-0.4, discomfort_dist=0.3,
            discomfort_penalty_factor=0.7, robot_safety_space=0.1, human_safety_space=0.05, neighbor_dist=4.0, time_horizon=4.0,
            circle_radius=9.0, human_radius=0.25, human_v_pref=1.2, robot_radius=0.35, robot_v_pref=0.8)

SETTINGS = (
    _s('dt_inexact', 5, dict(time_step=0.1, time_limit=12.0),
       'dt is no binary fraction: t += dt and steps * dt part in bits inside an episode, so a kernel or restatement that multiplies '
       'where the environment accumulates shows; a 4 m crossing at speed 1 does not always fit into 12 s',
       claims=('timeout', 'collision', 'reach_goal', 'danger'), steps=250),
    _s('dt_fifth_square', 5, dict(time_step=0.2, scenario_rule=1, square_width=13.0, human_v_pref=0.8),
       'another inexact dt under the square-crossing rule at another width, slower humans', claims=('reach_goal', 'danger')),
    _s('speeds', 5, dict(human_v_pref=1.4, robot_v_pref=0.7),
       'v_pref != 1: ORCA\'s preferred velocity is clipped to speed 1, not to v_pref, while maxSpeed is v_pref; the discount exponent '
       't dt v_pref is not t / 4', claims=('reach_goal', 'collision', 'danger'), steps=200),
    _s('radii_rewards', 5, dict(human_radius=0.4, robot_radius=0.2, discomfort_dist=0.35, discomfort_penalty_factor=0.8,
                                success_reward=1.7, collision_penalty=-0.6, circle_radius=5.5, robot_safety_space=0.15,
                                human_safety_space=0.05),
       'every reward constant, both radii, both safety spaces and the circle differ from the shipped ones (and from the constants '
       'MultiHumanRL.compute_reward hard-codes)', oracle_only=('human_safety_space',),
       claims=('reach_goal', 'collision', 'danger'), steps=200),
    _s('near_sighted', 5, dict(neighbor_dist=3.0, max_neighbors=3, time_horizon=2.0),
       'ORCA keeps the 3 nearest of the agents inside 3 m: the cut by distance and the cut by count both bite',
       oracle_only=('neighbor_dist', 'max_neighbors', 'time_horizon'), claims=('reach_goal', 'collision', 'danger')),
    _s('table_edge', 5, dict(time_step=0.125, time_limit=31.0),
       'ceil(time_limit / time_step) + 8 is exactly the 256 entries of the discount table: the longest episode cn_set_gamma accepts',
       claims=('reach_goal', 'collision', 'danger'), steps=250),
    _s('random_attributes', 12, dict(randomize_attributes=1, robot_v_pref=0.7, robot_radius=0.25, time_step=0.2, circle_radius=6.0),
       'sampled human radii and speeds (the wave generator\'s prefilter path at 12 humans) beside a slow, small robot; the circle is wider because 24 start and goal points of radii up to 0.5 do not fit on the 4 m one',
       claims=('reach_goal', 'danger'), envs=12),
    _s('H12_small', 12, dict(human_radius=0.2, discomfort_dist=0.1, human_v_pref=1.4, circle_radius=5.0),
       'the wave generator\'s blocked-cell table at other radii, another margin and another table size (R + v_pref / 2)',
       claims=('reach_goal', 'danger'), envs=12),
    _s('H20_shard', 20, _H20,
       'the 20-human shard kernel (float64 parameters in LDS slots) with every parameter non-default but max_neighbors = 10',
       oracle_only=('neighbor_dist', 'time_horizon', 'human_safety_space'), claims=('reach_goal', 'danger', 'collision', 'timeout'), envs=24, steps=160),
    _s('H20_five_neighbours', 20, dict(_H20, max_neighbors=5),
       'max_neighbors = 5 at 20 humans: the shard kernel hard-codes 10, so the route must be the generic kernel',
       oracle_only=('neighbor_dist', 'time_horizon', 'human_safety_space', 'max_neighbors'), claims=('reach_goal', 'danger', 'collision', 'timeout'), envs=24,
       steps=160),
)
BY_NAME = {s.name: s for s in SETTINGS}
assert len(BY_NAME) == len(SETTINGS)
# entries whose reference-expressible part differs from another entry's: one fixture each (H20_five_neighbours would repeat H20_shard's)
FIXTURES = tuple(s.name for s in SETTINGS if set(s.config) - set(s.oracle_only) and s.name != 'H20_five_neighbours')


def setting_id(s):
    return s.name


def engine_config(s, **extra):
    """The cn_config / CrowdOracle keywords of the entry."""
    config = dict(s.config, num_humans=s.humans)
    config.update(extra)
    return config


def reference_config(s):
    """... without the keys the reference cannot express: what the entry's fixture was made with."""
    return {k: v for k, v in s.config.items() if k not in s.oracle_only}


def sarl_env_config():
    """The settings of the two SARL fixtures (sarl_settings_*.npz): radii_rewards + dt_inexact as far as env.config spells them
    (the robot policy's safety space belongs to an ORCA robot)."""
    config = dict(reference_config(BY_NAME['radii_rewards']), **reference_config(BY_NAME['dt_inexact']))
    del config['robot_safety_space']
    return config


def fixture_name(s):
    return 'settings_%s.npz' % s.name


def reference_overrides(config):
    """cn_config keywords -> {'section.key': value} as the reference's env.config spells them."""
    out = {}
    for k, v in config.items():
        if k == 'scenario_rule':
            v = RULES[v]
        elif k == 'randomize_attributes':
            v = 'true' if v else 'false'
        elif k == 'time_limit':  # crowd_sim.py:53 reads it with getint
            assert v == int(v), 'the reference takes whole seconds only'
            v = int(v)
        out[REFERENCE_KEY[k]] = v
    return out


def config_from_overrides(overrides):
    """The inverse: {'section.key': value} (strings as a config parser returns them are fine) -> cn_config keywords."""
    back = {v: k for k, v in REFERENCE_KEY.items()}
    out = {}
    for key, v in overrides.items():
        k = back[key]
        if k == 'scenario_rule':
            out[k] = RULES.index(v)
        elif k == 'randomize_attributes':
            out[k] = int(str(v).lower() == 'true')
        else:
            out[k] = float(v)
    return out


def fixture_config(g):
    """The cn_config keywords stored in a settings fixture (+ num_humans)."""
    return dict(json.loads(str(g['config_json'])), num_humans=int(g['num_humans']))


def seeds(s, envs=None):
    return SEED_BASE + np.arange(s.envs if envs is None else envs)


def start_states(oracle_mod, s, envs=None, **extra):
    """The entry's own start states: the oracle's reset of the 'test' seeds under the entry's config, [envs, A, 8]."""
    n = s.envs if envs is None else envs
    o = oracle_mod.CrowdOracle(num_envs=n, **engine_config(s, **extra))
    o.reset(seeds(s, n))
    return o.get_state()[0]


def still_robot(state0, far=40.0):
    """state0 with the robot parked at (0, -far), its goal `far` further on: with a zero action nobody reaches it and it never
    arrives, so every episode runs into the time limit."""
    st = np.array(state0, dtype=np.float64, copy=True)
    st[:, 0, :6] = [0.0, -far, 0.0, 0.0, 0.0, -2.0 * far]
    return st


def run(oracle_mod, config, humans, state0, steps, visible, still=False):
    """`steps` transitions of the oracle from state0 under config, with its ORCA robot or (still) an external robot that stands
    where still_robot() put it: dict of reward / info / dmin / time [steps, B] and state [steps, B, A, 8].  Rows of an env whose
    episode is over are masked (info 255, zeros elsewhere)."""
    B = len(state0)
    o = oracle_mod.CrowdOracle(num_envs=B, num_humans=humans, robot_policy=0 if still else 1, robot_visible=visible, **config)
    o.set_state(still_robot(state0) if still else state0, np.zeros(B))
    zero = np.zeros((B, 2)) if still else None
    out = dict(reward=[], info=[], dmin=[], time=[], state=[])
    alive = np.ones(B, bool)
    for _ in range(steps):
        r = o.step(zero, update=True)
        state, time = o.get_state()
        out['reward'].append(np.where(alive, r['reward'], 0.0))
        out['info'].append(np.where(alive, r['info'], 255).astype(np.uint8))
        out['dmin'].append(np.where(alive & (r['info'] == 1), r['dmin'], 0.0))
        out['time'].append(np.where(alive, time, 0.0))
        out['state'].append(np.where(alive[:, None, None], state, 0.0))
        alive &= r['done'] == 0
        if not alive.any():
            break
    return {k: np.array(v) for k, v in out.items()}


def same(a, b):
    """Whether two run() results agree in every bit."""
    return all(a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes() for k in a)


# ---------------------------------------------------------------------------------------- the settings fixtures, as the tests read them
def fixture_settings():
    """The entries that have a fixture."""
    return [BY_NAME[n] for n in FIXTURES]


def episodes(g, tag):
    """The episodes of a settings fixture under one visibility ('invisible' / 'visible'): dicts of states [T + 1, A, 8] and
    actions / rewards / dones / infos / dmins / times [T]."""
    out, s0, a0 = [], 0, 0
    for T in g[tag + '_steps'].tolist():
        e = {k: g['%s_%s' % (tag, k)][a0:a0 + T] for k in ('actions', 'rewards', 'dones', 'infos', 'dmins', 'times')}
        e['states'] = g[tag + '_states'][s0:s0 + T + 1]
        out.append(e)
        s0, a0 = s0 + T + 1, a0 + T
    return out


def flat(g, tag):
    """(state before, state after, time before, time after) of every step of a settings fixture, the time as the reference
    accumulated it."""
    eps = episodes(g, tag)
    before = np.concatenate([e['states'][:-1] for e in eps])
    after = np.concatenate([e['states'][1:] for e in eps])
    t0 = np.concatenate([np.concatenate([[0.0], e['times'][:-1]]) for e in eps])
    return before, after, t0, g[tag + '_times']


def accumulated(dt, k):
    """k sequential additions of dt from 0.0: the environment's clock after k steps."""
    t = 0.0
    for _ in range(k):
        t += dt
    return t


def whole_config(config):
    """config over the shipped values: every key a host restatement reads."""
    return dict(SHIPPED, **config)
