"""The robot rows the unicycle prior's GPU parity tests install (tests/test_plan_unicycle.py), shared with the host suite, which
asserts the condition they are chosen for (tests/test_plan_unicycle_host.py): at every step of the restated recurrence the turn
|wrap(bearing - heading)| stays at least TURN_MARGIN away from pi, so a last-bit difference of the device's atan2 cannot flip
the wrap and turn the robot the other way round.  numpy only."""
import numpy as np

DT, V_PREF = 0.25, 1.0  # the engines' defaults (time_step, robot_v_pref)
TURN_MARGIN = 1e-6
N = 33                  # the longest horizon the parity tests walk
ROTATIONS = (np.pi / 4, 0.1)

# (px, py, gx, gy, theta) of the robot of env 0, 1, 2
PRIOR_ROBOTS = np.array([
    [0.0, -4.0, 0.0, 4.0, np.pi / 2],   # the scenario generator's start: facing the goal
    [-1.5, 2.0, 3.0, -1.0, 2.5],        # the goal behind and to the right: a long turn, clipped for many steps
    [0.25, 0.5, 0.4, 0.55, -1.0],       # the goal within one step once the robot has turned: speed = dist / dt, then it circles it
])
# after a re-seed (cn_plan_shift, cur_steps == 0) the robot stands at a scenario's start with the heading of every episode start
RESEED_THETA = np.pi / 2


def install(state8, robots=PRIOR_ROBOTS):
    """state8 [B, A, 8] with the robot rows replaced by `robots` (velocity zero) -> (state8, theta [B])."""
    state8 = np.array(state8, np.float64)
    B = len(state8)
    state8[:, 0, 0:2], state8[:, 0, 2:4], state8[:, 0, 4:6] = robots[:B, 0:2], 0.0, robots[:B, 2:4]
    return state8, robots[:B, 4].copy()
