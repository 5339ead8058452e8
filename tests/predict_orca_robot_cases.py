"""What test_predict_orca_robot_host.py (no GPU) and test_predict_orca_robot.py (GPU) share: the scenes — predict_orca_cases'
crowds with the robot put in a human's way and given a turning action sequence — the oracle's statement of the table
cn_predict_orca_robot must give (the environment itself, humans seeing the robot, fresh simulators, stepped with the sequence), the
three wrong tables a kernel could make instead, and the branch outcomes of a replay scene on the oracle."""
import numpy as np

import predict_orca_cases as base

B, N = base.B, base.N
CROWDS = base.CROWDS
SEEDS = base.SEEDS
THETA = np.array([6.0, 0.1, 3.0])  # unicycle start headings: env 0 wraps past 2 pi with r > 0.29, env 1 below 0 with r < -0.1


def start(oracle_mod, crowd, steps=4, **settings):
    """(state8 [B, A, 8], global_time [B]) after a seeded reset and `steps` real steps straight on, made by the oracle alone: what
    the GPU tests take from an engine under way."""
    o = oracle_mod.CrowdOracle(num_envs=B, robot_policy=0, robot_visible=1, **dict(CROWDS[crowd], **settings))
    o.reset(SEEDS)
    straight_on = [1.0, 0.0] if settings.get('robot_kinematics') else [0.0, 1.0]
    for _ in range(steps):
        o.step(np.tile(straight_on, (B, 1)), update=True)
    return o.get_state()


def place_robot(state):
    """test_predict_orca.py's _replay_scene placement: the robot 1.0 m ahead of human 1 on that human's way to its goal, at rest,
    its own goal 1.5 m to the side.  Returns (placed state, d [B, 2] the human's direction, side [B, 2])."""
    placed = np.array(state, dtype=np.float64, copy=True)
    human = placed[:, 1]
    d = human[:, 4:6] - human[:, 0:2]
    far = np.hypot(d[:, 0], d[:, 1])
    d = np.where(far[:, None] > 0.0, d / np.where(far > 0.0, far, 1.0)[:, None], [1.0, 0.0])  # (a human at its goal: along x)
    side = np.stack([-d[:, 1], d[:, 0]], axis=1)
    at = human[:, 0:2] + d
    placed[:, 0, 0:2], placed[:, 0, 2:4], placed[:, 0, 4:6] = at, 0.0, at + side * 1.5
    return placed, d, side


def action_space(unicycle=False):
    from crowdnav_amd.compat.sarl import build_action_space
    space = build_action_space(1.0, kinematics='unicycle' if unicycle else 'holonomic')[0]
    return np.array([list(a) for a in space], dtype=np.float64)


def sequences(envs=B, n=N, unicycle=False, seed=11):
    """[envs, n, 2] float64: one action sequence per env, drawn from the SARL action space with a fixed seed — it turns.  The
    unicycle rows are ActionRot(v, r) with r != 0 (the stop action is left out; no rotation sample is zero)."""
    acts = action_space(unicycle)
    if unicycle:
        acts = acts[1:]
        assert (acts[:, 1] != 0.0).all()
    return acts[np.random.RandomState(seed).randint(len(acts), size=(envs, n))]


def wraps(theta, actions):
    """How often python's (theta + r) % (2 pi) leaves [0, 2 pi) before the % along each env's unicycle sequence."""
    count = np.zeros(len(theta), dtype=int)
    for b, th in enumerate(np.asarray(theta, dtype=np.float64)):
        for v, r in actions[b]:
            count[b] += not 0.0 <= th + r < 2 * np.pi
            th = (th + r) % (2 * np.pi)
    return count


def oracle_table(oracle_mod, crowd, state, gtime, actions, theta=None, robot='follows', **settings):
    """The table predict_orca_robot(n, actions) must give from (state, gtime[, theta]): n = actions.shape[1] steps of an oracle
    whose humans see the robot, fresh simulators, step(actions[:, t], update=True).  Returns (vel float64 [B, n, H, 2],
    fallback bool [B, n, H], done uint8 [B, n]); rows behind `done` count: the oracle keeps stepping.
    robot: 'follows' — the statement itself; 'stands' — the robot never moves (a kernel that does not move it); 'stale' — it
    moves, but the humans are shown its START velocity at every step (a kernel that moves it and stages a stale velocity)."""
    state = np.asarray(state, dtype=np.float64)
    envs, n, H = len(state), actions.shape[1], state.shape[1] - 1
    o = oracle_mod.CrowdOracle(num_envs=envs, robot_policy=0, robot_visible=1, **dict(CROWDS[crowd], **settings))
    o.set_state(state, gtime)
    if theta is not None:
        o.set_theta(theta)
    o.drop_sims()
    vel, fallback, done = np.zeros((envs, n, H, 2)), np.zeros((envs, n, H), dtype=bool), np.zeros((envs, n), np.uint8)
    for t in range(n):
        if robot == 'stale':
            now, g = o.get_state()
            now[:, 0, 2:4] = state[:, 0, 2:4]
            o.set_state(now, g)
        out = o.step(np.zeros((envs, 2)) if robot == 'stands' else actions[:, t], update=True)
        assert out['orca_vel'].dtype == np.float32
        vel[:, t], fallback[:, t], done[:, t] = out['orca_vel'][:, 1:].astype(np.float64), o.last_fallback()[:, 1:], out['done']
    return vel, fallback, done


def furthest(a, b):
    """The largest Euclidean distance (m/s) between rows of two tables."""
    return float(np.sqrt(((a - b) ** 2).sum(axis=-1)).max())


def oracle_branches(oracle_mod, crowd, placed, gtime, table):
    """(info [B, K], steps [B, K]) of every branch on an oracle whose humans see the robot: the first `done` and the steps to it."""
    envs, K, n = table.shape[:3]
    info, steps = np.zeros((envs, K), np.uint8), np.full((envs, K), n)
    for k in range(K):
        o = oracle_mod.CrowdOracle(num_envs=envs, robot_policy=0, robot_visible=1, **CROWDS[crowd])
        o.set_state(placed, gtime)
        o.drop_sims()
        over = np.zeros(envs, dtype=bool)
        for t in range(n):
            out = o.step(table[:, k, t], update=True)
            ends = ~over & (out['done'] != 0)
            info[ends, k], steps[ends, k] = out['info'][ends], t + 1
            last = ~over & ~ends if t == n - 1 else np.zeros(envs, dtype=bool)
            info[last, k] = out['info'][last]
            over |= ends
    return info, steps
