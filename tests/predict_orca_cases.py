"""What the predict_orca and predict_orca_robot suites, host (no GPU) and GPU, share: the crowds, the oracle's statement of the ORCA
predictor's table — the environment itself, stepped with the robot unseen and fresh simulators — and the preconditions a scene
must meet for the bit-for-bit comparison to mean something."""
import numpy as np

B, N = 3, 12
SEEDS = 1000 + np.arange(B)
CROWDS = {'h1': dict(num_humans=1), 'h5': dict(num_humans=5), 'h12': dict(num_humans=12), 'h20': dict(num_humans=20),
          'h5_mixed': dict(num_humans=5, scenario_rule=2)}


def oracle_start(oracle_mod, crowd, steps=4, robot_visible=1):
    """(state8 [B, A, 8], global_time [B]) after a seeded reset and `steps` real steps with the action (0, 1): what the GPU test
    takes from the engine, made by the oracle alone."""
    o = oracle_mod.CrowdOracle(num_envs=B, robot_policy=0, robot_visible=robot_visible, **CROWDS[crowd])
    o.reset(SEEDS)
    for _ in range(steps):
        o.step(np.tile([0.0, 1.0], (B, 1)), update=True)
    return o.get_state()


def oracle_table(oracle_mod, crowd, state, gtime, n=N, **settings):
    """The table predict_orca(n) must give from (state, gtime): n steps of an oracle whose humans do not see the robot, fresh
    simulators, the robot standing.  Returns (vel float64 [B, n, H, 2], fallback bool [B, n, H]: whose solve took the 3-D
    fallback, done uint8 [B, n]).  Rows after `done` count: the oracle keeps stepping."""
    state = np.asarray(state)
    o = oracle_mod.CrowdOracle(num_envs=len(state), robot_policy=0, robot_visible=0, **dict(CROWDS[crowd], **settings))
    o.set_state(state, gtime)
    o.drop_sims()
    H = state.shape[1] - 1
    vel, fallback, done = np.zeros((len(state), n, H, 2)), np.zeros((len(state), n, H), dtype=bool), np.zeros((len(state), n), np.uint8)
    for t in range(n):
        out = o.step(np.zeros((len(state), 2)), update=True)
        assert out['orca_vel'].dtype == np.float32
        vel[:, t], fallback[:, t], done[:, t] = out['orca_vel'][:, 1:].astype(np.float64), o.last_fallback()[:, 1:], out['done']
    return vel, fallback, done


def visible_first_step(oracle_mod, crowd, state, gtime):
    """[B, H, 2] float64: the humans' next velocities on an oracle whose humans DO see the robot (fresh simulators, the robot
    standing) — what a kernel that left the robot in would write into row 0."""
    o = oracle_mod.CrowdOracle(num_envs=len(state), robot_policy=0, robot_visible=1, **CROWDS[crowd])
    o.set_state(state, gtime)
    o.drop_sims()
    return o.step(np.zeros((len(state), 2)), update=False)['orca_vel'][:, 1:].astype(np.float64)


def differs_from(vel, other):
    """[B, H]: the furthest any row of human h's table lies from `other`'s (Euclidean, m/s)."""
    return np.sqrt(((vel - other) ** 2).sum(axis=-1)).max(axis=1)


# ------------------------------------------------------------------------------------------------ the GPU suites' shared parts
BEGIN = dict(seed_base=1000, seed_mod=500, record_capacity=8)
KEYS = ('ret', 'info', 'steps', 'time', 'final_state8', 'final_theta')
# the closed loops' futures and plan updates
FUTURES = {'one': dict(models='to_goal', orca_mode=0), 'two': dict(models=('to_goal', 'cv'), orca_mode=1, reduce='min')}
UPDATES = {'cem': {}, 'mppi': dict(temperature=1.0, fit_std=False)}


def engine(amd, crowd='h5', envs=B, steps=4, **cfg):
    """A seeded reset and `steps` real steps with the action (0, 1): the humans are under way."""
    cfg = dict(CROWDS[crowd], **cfg)
    eng = amd.BatchedCrowdSim(num_envs=envs, robot_policy=cfg.pop('robot_policy', amd.ROBOT_EXTERNAL), **cfg)
    eng.reset(1000 + np.arange(envs))
    straight_on = [1.0, 0.0] if cfg.get('robot_kinematics') else [0.0, 1.0]
    for _ in range(steps):
        eng.step(np.tile(straight_on, (envs, 1)) if eng.config['robot_policy'] == amd.ROBOT_EXTERNAL else None, update=True,
                 want_obs=False)
    return eng


def replay_scene(state, K=9, n=10):
    """test_lookahead_paths.py (b)'s scene: the robot 1.0 ahead of human 1 on that human's way to its goal, its own goal 1.5 to
    the side: straight to the goal is ReachGoal at the fifth step, standing still is run over (the humans do not see the
    robot), walking ahead of human 1 — at its speed or a little slower — runs on."""
    from crowdnav_amd.compat.sarl import build_action_space
    acts = np.array([list(a) for a in build_action_space(1.0)[0]], dtype=np.float64)
    placed = state.copy()
    table = acts[np.random.RandomState(7).randint(len(acts), size=(len(state), K, n))]
    for b in range(len(state)):
        human = state[b, 1]
        d = (human[4:6] - human[0:2]) / np.hypot(*(human[4:6] - human[0:2]))
        side = np.array([-d[1], d[0]])
        at = human[0:2] + d * 1.0
        placed[b, 0, 0:2], placed[b, 0, 2:4], placed[b, 0, 4:6] = at, 0.0, at + side * 1.5
        table[b, 0], table[b, 1], table[b, 2], table[b, 3] = side, 0.0, d, 0.9 * d
    return placed, table
