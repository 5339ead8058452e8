"""Host restatement of ONE branch of cn_lookahead_paths (include/crowdnav_amd.h, "Lookahead under predicted human motion"):
the constant-velocity branch of lookahead_cv_reference.py with the header's one substitution — the velocity a human CHOOSES at
step t is human_vel[t][h].  As in step_core, the swept test of a step reads the velocity a human HAS when the step starts (the
rows' velocity columns as they stand: the state velocity at t = 0, afterwards what the step before wrote), and the chosen
velocity moves the human and is written into the columns behind the step.  Built on lookahead_cv_reference.transition, whose
own move (by the velocity the human has) is replaced.  Python floats, holonomic robots only, as there."""
import lookahead_cv_reference as cv

NOTHING, DANGER, REACH_GOAL, COLLISION, TIMEOUT = cv.NOTHING, cv.DANGER, cv.REACH_GOAL, cv.COLLISION, cv.TIMEOUT
CFG = cv.CFG


def branch(state8, gtime, actions, human_vel, cfg=CFG, table=None, gamma=0.9):
    """state8 [A][8], its global_time, actions [n][2], human_vel [n][A - 1][2].  Returns lookahead_cv_reference.branch's dict."""
    table = cv.discount_table(gamma, cfg) if table is None else table
    state = [[float(x) for x in row] for row in state8]
    gtime, ret, steps, infos = float(gtime), 0.0, 0, []
    for t, action in enumerate(actions):
        before = [(human[0], human[1]) for human in state[1:]]
        reward, done, info, _ = cv.transition(state, gtime, (float(action[0]), float(action[1])), cfg)  # swept: the velocity it HAS
        for h, human in enumerate(state[1:]):  # the move and the state behind it: the velocity it CHOSE, one multiply and one add
            human[2], human[3] = float(human_vel[t][h][0]), float(human_vel[t][h][1])
            human[0] = before[h][0] + human[2] * cfg['time_step']
            human[1] = before[h][1] + human[3] * cfg['time_step']
        disc = table[t] if t < len(table) and t < 256 else 0.0
        ret = ret + disc * reward
        steps = t + 1
        gtime = gtime + cfg['time_step']
        infos.append(info)
        if done:
            break
    return dict(ret=ret, info=infos[-1], steps=steps, time=gtime, final_state8=state, infos=infos)


def lookahead(state8, gtime, table_actions, human_vel, cfg=CFG, gamma=0.9):
    """Every branch of a call: state8 [B][A][8], gtime [B], table_actions [B][K][n][2], human_vel [B][n][A - 1][2] -> numpy
    arrays shaped as the engine's lookahead_paths() dict (ret, info, steps, time, final_state8) plus infos[b][k]."""
    import numpy as np
    B, K = len(table_actions), len(table_actions[0])
    A = len(state8[0])
    table = cv.discount_table(gamma, cfg)
    out = dict(ret=np.zeros((B, K)), info=np.zeros((B, K), np.uint8), steps=np.zeros((B, K), np.int32), time=np.zeros((B, K)),
               final_state8=np.zeros((B, K, A, 8)))
    infos = [[None] * K for _ in range(B)]
    for b in range(B):
        rows = [[float(x) for x in row] for row in state8[b]]
        vel = [[(float(v[0]), float(v[1])) for v in step] for step in human_vel[b]]
        for k in range(K):
            got = branch(rows, gtime[b], [tuple(a) for a in table_actions[b][k]], vel, cfg, table)
            out['ret'][b, k], out['info'][b, k], out['steps'][b, k], out['time'][b, k] = got['ret'], got['info'], got['steps'], got['time']
            out['final_state8'][b, k] = got['final_state8']
            infos[b][k] = got['infos']
    out['infos'] = infos
    return out
