"""Host restatement of cn_lookahead_modes (include/crowdnav_amd.h, "Lookahead under several predicted futures"), and the scenes
its tests share.

Mode m of branch (b, k) is lookahead_paths_reference.branch with the table human_vel[b][m]; the reduction is the header's,
python floats, every product and sum one operation, sequential in m from 0.0.  Holonomic robots only, as the modules below it.

The scenes are made on the host (numpy, seeded), so that tests/test_lookahead_modes_host.py can check on the restatement,
without a device, that the cases tests/test_lookahead_modes.py runs on the device contain what they are meant to contain."""
import numpy as np

import lookahead_cv_reference as cv
import lookahead_paths_reference as paths

NOTHING, DANGER, REACH_GOAL, COLLISION, TIMEOUT = cv.NOTHING, cv.DANGER, cv.REACH_GOAL, cv.COLLISION, cv.TIMEOUT
CFG = dict(cv.CFG, discomfort_dist=0.5)  # the engine's defaults with the wider discomfort zone the paths tests use
GAMMA = 0.9
UNROUNDABLE = 0.3 + 2.0 ** -40  # a velocity float32 cannot hold
MEAN, MIN = 'mean', 'min'


# ------------------------------------------------------------------------------------------------ the restatement
def per_mode(state8, gtime, table_actions, human_vel, cfg=CFG, gamma=GAMMA):
    """state8 [B][A][8], gtime [B], table_actions [B][K][n][2], human_vel [B][M][n][A - 1][2] -> dict of numpy arrays [B, K, M]:
    ret, info (uint8), steps (int32), time — every mode's lookahead_paths branch."""
    B, K, M = len(table_actions), len(table_actions[0]), len(human_vel[0])
    table = cv.discount_table(gamma, cfg)
    out = dict(ret=np.zeros((B, K, M)), info=np.zeros((B, K, M), np.uint8), steps=np.zeros((B, K, M), np.int32),
               time=np.zeros((B, K, M)))
    for b in range(B):
        rows = [[float(x) for x in row] for row in state8[b]]
        for m in range(M):
            vel = [[(float(v[0]), float(v[1])) for v in step] for step in human_vel[b][m]]
            for k in range(K):
                got = paths.branch(rows, gtime[b], [tuple(a) for a in table_actions[b][k]], vel, cfg, table)
                for key in ('ret', 'info', 'steps', 'time'):
                    out[key][b, k, m] = got[key]
    return out


def reduce_branch(ret, info, steps, time, weights, reduce, risk_penalty):
    """The header's reduction of ONE branch: ret, info, steps, time of its M modes (sequences), weights (M floats or None = every
    weight 1.0 / M).  Returns (score, risk, worst_mode, worst_info, worst_steps, worst_time)."""
    M = len(ret)
    w = [1.0 / float(M)] * M if weights is None else [float(x) for x in weights]
    mean, risk, worst = 0.0, 0.0, 0
    for m in range(M):
        mean = mean + w[m] * float(ret[m])
        risk = risk + w[m] * (1.0 if int(info[m]) == COLLISION else 0.0)
        if float(ret[m]) < float(ret[worst]):  # strict: the smallest m that holds the lowest return
            worst = m
    if reduce not in (MEAN, MIN):
        raise ValueError(reduce)
    r = mean if reduce == MEAN else float(ret[worst])
    return r - float(risk_penalty) * risk, risk, worst, int(info[worst]), int(steps[worst]), float(time[worst])


def reduced(modes, weights=None, reduce=MEAN, risk_penalty=0.0):
    """per_mode()'s dict (or the device's per-mode rows as numpy) -> the dict lookahead_modes() returns, as numpy [B, K]."""
    B, K, _ = modes['ret'].shape
    out = dict(score=np.zeros((B, K)), risk=np.zeros((B, K)), worst_mode=np.zeros((B, K), np.int32),
               worst_info=np.zeros((B, K), np.uint8), worst_steps=np.zeros((B, K), np.int32), worst_time=np.zeros((B, K)))
    for b in range(B):
        for k in range(K):
            row = reduce_branch(modes['ret'][b, k], modes['info'][b, k], modes['steps'][b, k], modes['time'][b, k],
                                None if weights is None else weights[b], reduce, risk_penalty)
            for key, value in zip(('score', 'risk', 'worst_mode', 'worst_info', 'worst_steps', 'worst_time'), row):
                out[key][b, k] = value
    return out


# ------------------------------------------------------------------------------------------------ the scenes
def action_space():
    """81 holonomic actions: standing still, and 5 speeds up to 1.0 in 16 directions."""
    speeds = [(np.exp((i + 1) / 5.0) - 1.0) / (np.e - 1.0) for i in range(5)]
    rows = [(0.0, 0.0)] + [(s * np.cos(r), s * np.sin(r)) for r in np.linspace(0.0, 2.0 * np.pi, 16, endpoint=False) for s in speeds]
    return np.array(rows, dtype=np.float64)


def action_table(B, K, n, seed=11):
    """[B, K, n, 2]: random rows of the action space; candidate 0 walks straight to the goal 1.0 ahead, candidate 1 stands."""
    acts = action_space()
    table = acts[np.random.RandomState(seed).randint(len(acts), size=(B, K, n))]
    table[:, 0] = (0.0, 1.0)
    if K > 1:
        table[:, 1] = (0.0, 0.0)
    return table


def scene(B, H, seed=3, time_limit=CFG['time_limit']):
    """(state8 [B, H + 1, 8], gtime [B]): the robot at the origin, at rest, its goal 1.0 ahead; H humans 1.2 to 3.5 away, every
    one walking at 0.3 .. 1.0 towards a point within 0.6 of the robot, its goal across the crowd and to the side of its
    course (so that to_goal turns it).  The last env starts 2 s before the time limit's last second: its branches time out at
    their ninth step."""
    rs = np.random.RandomState(seed)
    state = np.zeros((B, H + 1, 8))
    state[:, 0] = (0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.3, 1.0)
    for b in range(B):
        for h in range(H):
            angle, dist = rs.uniform(0.0, 2.0 * np.pi), rs.uniform(1.2, 3.5)
            p = dist * np.array([np.cos(angle), np.sin(angle)])
            aim = rs.uniform(-0.6, 0.6, 2) - p
            v = aim / np.hypot(*aim) * rs.uniform(0.3, 1.0)
            turn = rs.uniform(0.5, 1.2) * rs.choice([-1.0, 1.0])
            goal = p + 6.0 * np.array([np.cos(turn) * v[0] - np.sin(turn) * v[1], np.sin(turn) * v[0] + np.cos(turn) * v[1]])
            state[b, h + 1] = (p[0], p[1], v[0], v[1], goal[0], goal[1], 0.3, 1.0)
    gtime = np.zeros(B)
    gtime[B - 1] = time_limit - 1.0 - 2.0
    return state, gtime


def turning(state, n, seed, sigma=0.15):
    """[B, n, H, 2]: every human starts from its own velocity and turns a little every step (a random walk of the velocity; a
    prefix in n)."""
    B, H = len(state), state.shape[1] - 1
    walk = np.cumsum(np.random.RandomState(seed).normal(0.0, sigma, (B, 33, H, 2)), axis=1)[:, :n]
    return np.ascontiguousarray(state[:, None, 1:, 2:4] + walk)


def mode_tables(state, n, M, dt=CFG['time_step']):
    """human_vel [B, M, n, H, 2] of a scene.  M == 1: one turning table.  Otherwise mode 0 constant velocity, mode 1
    predict.to_goal, modes 2 .. turning tables (the later ones turn harder); with M >= 3 the LAST mode repeats mode 1 — an exact
    tie wherever that future is the worst.  Mode 0 gives human 1 of env 0 a velocity no float32 holds at step 0."""
    from crowdnav_amd import predict
    tables = [predict.constant_velocity(state, n), predict.to_goal(state, n, dt)]
    tables += [turning(state, n, seed=5 + i, sigma=0.15 + 0.05 * i) for i in range(6)]
    if M == 1:
        tables = [tables[2]]
    elif M >= 3:
        tables = tables[:M - 1] + [tables[1].copy()]
    vel = predict.stack_modes(*tables[:M])
    vel[0, 0, 0, 0, 0] = UNROUNDABLE
    assert float(np.float32(UNROUNDABLE)) != UNROUNDABLE and vel.shape == (len(state), M, n, state.shape[1] - 1, 2)
    return vel


def weights_table(B, M, seed=9):
    """[B, M] weights that are exact powers of two (their products with a return are exact), not normalised."""
    return 2.0 ** -np.random.RandomState(seed).randint(1, 5, size=(B, M)).astype(np.float64)


# The cases test_lookahead_modes.py reduces on the device, (humans, K, n, M), B = 3 each
REDUCTION_CASES = [(5, 70, 33, 3), (12, 5, 4, 8), (1, 70, 4, 8)]
_CASES = {}


def case(H, K, n, M, B=3):
    """(state8, gtime, actions, human_vel, per_mode()'s dict) of a reduction case, computed once and shared; left unchanged."""
    key = (H, K, n, M, B)
    if key not in _CASES:
        state, gtime = scene(B, H)
        actions, vel = action_table(B, K, n), mode_tables(state, n, M)
        _CASES[key] = (state, gtime, actions, vel, per_mode(state, gtime, actions, vel))
    return _CASES[key]
