"""Host restatement of the lookahead goal-progress term (include/crowdnav_amd.h, "Lookahead goal-progress term"): python floats
are IEEE doubles, every operation below is one operation in the order the header writes it; norm2 is the project's
sqrt(fma(y, y, x * x)) as tests/lookahead_cv_reference.py restates it.  Written from the header, not from the kernels."""
from lookahead_cv_reference import norm2


def goal_term(w, start_xy, goal_xy, end_xy):
    """w * (d0 - d1): d0 the distance start -> goal, d1 the distance end -> goal.  One subtraction, then one multiply; the
    caller adds it to ret (the third operation of the rule)."""
    w = float(w)
    px0, py0 = float(start_xy[0]), float(start_xy[1])
    gx, gy = float(goal_xy[0]), float(goal_xy[1])
    px, py = float(end_xy[0]), float(end_xy[1])
    d0 = norm2(px0 - gx, py0 - gy)
    d1 = norm2(px - gx, py - gy)
    progress = d0 - d1
    return w * progress
