"""Host restatement of ONE branch of cn_lookahead_actions under CN_HUMANS_CONSTANT_VELOCITY (include/crowdnav_amd.h, "Lookahead
human model"): python floats are IEEE doubles, every product and sum below is one operation in the order the header writes it.
Written from step_core (crowdnav_amd/csrc/step_kernels.h) with the one substitution — a human's chosen velocity is its own
current velocity — not from the kernel that is tested against it.

norm2's fused multiply-add is restated exactly: y * y and the already rounded x * x are added as rationals and rounded once
(python 3.10 has no math.fma).  Holonomic robots only: a unicycle's cos / sin are the device libm's."""
import math
from fractions import Fraction

NOTHING, DANGER, REACH_GOAL, COLLISION, TIMEOUT = range(5)
CFG = dict(time_step=0.25, time_limit=25.0, success_reward=1.0, collision_penalty=-0.25, discomfort_dist=0.2,
           discomfort_penalty_factor=0.5, robot_v_pref=1.0)  # the engine's defaults


def norm2(x, y):
    """sqrt(fma(y, y, x * x)): the product x * x rounded, y * y exact, their sum rounded once, the root rounded."""
    return math.sqrt(float(Fraction(y) * Fraction(y) + Fraction(x * x)))


def discount_table(gamma, cfg, length=None):
    """cn_set_gamma's table: gamma ** (t * time_step * robot_v_pref), ceil(time_limit / time_step) + 8 entries."""
    n = int(math.ceil(cfg['time_limit'] / cfg['time_step'])) + 8 if length is None else length
    return [math.pow(gamma, t * cfg['time_step'] * cfg['robot_v_pref']) for t in range(n)]


def closest(px, py, ax, ay, human, dt, r_robot):
    """Swept distance of one human row (hx, hy, hvx, hvy, gx, gy, radius, v_pref) to the robot at (px, py) taking (ax, ay)."""
    hx, hy, hvx, hvy, radius = human[0], human[1], human[2], human[3], human[6]
    x1, y1 = hx - px, hy - py
    wx, wy = hvx - ax, hvy - ay
    x2, y2 = x1 + wx * dt, y1 + wy * dt
    sx, sy = x2 - x1, y2 - y1
    if sx == 0.0 and sy == 0.0:  # utils.py:11-13 (the device forms u = 0 / 0 = NaN here and does not use it)
        cx, cy = 0.0 - x1, 0.0 - y1
    else:
        u = ((0.0 - x1) * sx + (0.0 - y1) * sy) / (sx * sx + sy * sy)
        u = 1.0 if u > 1.0 else (0.0 if u < 0.0 else u)
        cx, cy = (x1 + u * sx) - 0.0, (y1 + u * sy) - 0.0
    return norm2(cx, cy) - radius - r_robot


def transition(state, gtime, action, cfg):
    """One step of a running branch.  state: list of A rows of 8 floats, changed in place.  Returns (reward, done, info, dmin)."""
    dt = cfg['time_step']
    robot = state[0]
    px, py, gx, gy, rad = robot[0], robot[1], robot[4], robot[5], robot[6]
    ax, ay = action
    dmin, collision = math.inf, False
    for human in state[1:]:
        c = closest(px, py, ax, ay, human, dt, rad)
        hit = c < 0.0
        if not collision and not hit and c < dmin:
            dmin = c
        collision = collision or hit
    ex, ey = px + ax * dt, py + ay * dt
    reaching = norm2(ex - gx, ey - gy) < rad
    if gtime >= cfg['time_limit'] - 1.0:
        reward, done, info = 0.0, True, TIMEOUT
    elif collision:
        reward, done, info = cfg['collision_penalty'], True, COLLISION
    elif reaching:
        reward, done, info = cfg['success_reward'], True, REACH_GOAL
    elif dmin < cfg['discomfort_dist']:
        reward, done, info = (dmin - cfg['discomfort_dist']) * cfg['discomfort_penalty_factor'] * dt, False, DANGER
    else:
        reward, done, info = 0.0, False, NOTHING
    robot[0], robot[1], robot[2], robot[3] = ex, ey, ax, ay
    for human in state[1:]:
        human[0] = human[0] + human[2] * dt
        human[1] = human[1] + human[3] * dt
    return reward, done, info, dmin


def branch(state8, gtime, actions, cfg=CFG, table=None, gamma=0.9):
    """Branch of one env: state8 [A][8] (cn_get_state's rows), its global_time, actions [n][2].  Returns a dict with ret, info,
    steps, time, final_state8 (list of rows) and infos (the code of every transition made)."""
    table = discount_table(gamma, cfg) if table is None else table
    state = [[float(x) for x in row] for row in state8]
    gtime, ret, steps, infos = float(gtime), 0.0, 0, []
    for t, action in enumerate(actions):
        reward, done, info, _ = transition(state, gtime, (float(action[0]), float(action[1])), cfg)
        disc = table[t] if t < len(table) and t < 256 else 0.0
        ret = ret + disc * reward
        steps = t + 1
        gtime = gtime + cfg['time_step']
        infos.append(info)
        if done:
            break
    return dict(ret=ret, info=infos[-1], steps=steps, time=gtime, final_state8=state, infos=infos)


def lookahead(state8, gtime, table_actions, cfg=CFG, gamma=0.9):
    """Every branch of a call: state8 [B][A][8], gtime [B], table_actions [B][K][n][2] -> numpy arrays shaped as the
    engine's lookahead() dict (ret, info, steps, time, final_state8) plus infos[b][k] (list of codes)."""
    import numpy as np
    B, K = len(table_actions), len(table_actions[0])
    A = len(state8[0])
    table = discount_table(gamma, cfg)
    out = dict(ret=np.zeros((B, K)), info=np.zeros((B, K), np.uint8), steps=np.zeros((B, K), np.int32), time=np.zeros((B, K)),
               final_state8=np.zeros((B, K, A, 8)))
    infos = [[None] * K for _ in range(B)]
    for b in range(B):
        rows = [[float(x) for x in row] for row in state8[b]]
        for k in range(K):
            got = branch(rows, gtime[b], [tuple(a) for a in table_actions[b][k]], cfg, table)
            out['ret'][b, k], out['info'][b, k], out['steps'][b, k], out['time'][b, k] = got['ret'], got['info'], got['steps'], got['time']
            out['final_state8'][b, k] = got['final_state8']
            infos[b][k] = got['infos']
    out['infos'] = infos
    return out


def robot_row(px=0.0, py=0.0, gx=0.0, gy=4.0):
    return [px, py, 0.0, 0.0, gx, gy, 0.3, 1.0]


def human_row(x, y, vx=0.0, vy=0.0):
    return [x, y, vx, vy, -x, -y, 0.3, 1.0]


def cfg_of(eng):
    """An engine's values of the settings CFG names."""
    return {k: float(eng.config[k]) for k in CFG}
