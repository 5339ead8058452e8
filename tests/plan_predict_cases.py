"""What test_plan_predict_host.py and test_plan_predict.py share: the crafted scene that takes predict.to_goal through all four
cases of its rule, and the count of those cases on the host restatement (crowdnav_amd.predict on numpy)."""
import numpy as np

DT = 0.25  # the engines' default time_step: a power of two, so v dt and (d / dt) dt are exact
ROBOT = (0.0, -4.0, 0.0, 0.0, 0.0, 4.0, 0.3, 1.0)
# (px, py, vx, vy, gx, gy, radius, v_pref)
CRAFTED = ((1.0, 0.0, 0.3, 0.1, 1.0, 0.0, 0.3, 1.0),      # stands on its goal, with a velocity: dist == 0 at every step
           (0.0, 0.0, 0.0, 1.0, 0.25, 0.0, 0.3, 1.0),     # dist == v_pref dt exactly: lands in one step, then stands
           (0.0, 0.0, 1.0, 0.0, 0.6, 0.0, 0.3, 1.0),      # two cruise steps, a shortened third, then stands
           (-1.0, -2.0, 0.0, 0.0, 2.0, 2.0, 0.3, 1.2),    # far away: cruises throughout (dist 5, 0.3 per step)
           (0.1, 0.2, -1.0, 0.0, 0.16, 0.28, 0.3, 0.8))   # dist 0.1 < v_pref dt = 0.2 at once, moving the other way
CASES = ('zero', 'exact', 'short', 'cruise')


def crafted_state(H, dt=DT, v_pref=None):
    """[1 + H, 8]: the robot and the crafted humans cut to H, or padded by going round them again, each round 8 m further out.
    dt, v_pref: the human of the `exact` case gets that v_pref (None: the 1.0 it has) and its goal at gx = v_pref * dt, the
    float64 product, so that its distance is the reach of one step at any time step — at the defaults the row keeps its bits."""
    rows = [ROBOT]
    for h in range(H):
        row, shift = list(CRAFTED[h % len(CRAFTED)]), 8.0 * (h // len(CRAFTED))
        if h % len(CRAFTED) == 1:
            row[7] = row[7] if v_pref is None else float(v_pref)
            row[4] = row[7] * float(dt)
        row[0], row[4] = row[0] + shift, row[4] + shift
        rows.append(tuple(row))
    return np.array(rows, dtype=np.float64)


def to_goal_cases(state8, n, dt):
    """How often each case of the to_goal rule is taken over [B, A, 8] and n steps, by name: the positions are those the table
    predict.to_goal returns moves the humans through (p <- p + v dt, one multiply and one add)."""
    from crowdnav_amd import predict
    state8 = np.asarray(state8, dtype=np.float64)
    table = predict.to_goal(state8, n, dt)
    p, goal, v_pref = state8[:, 1:, 0:2].copy(), state8[:, 1:, 4:6], state8[:, 1:, 7]
    counts = dict.fromkeys(CASES, 0)
    for t in range(n):
        d = goal - p
        dist = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])
        reach = v_pref * dt
        counts['zero'] += int((dist == 0.0).sum())
        counts['exact'] += int(((dist > 0.0) & (dist == reach)).sum())
        counts['short'] += int(((dist > 0.0) & (dist < reach)).sum())
        counts['cruise'] += int((dist > reach).sum())
        p = p + table[:, t] * dt
    return counts
