"""What test_predict_orca_host.py (no GPU) and test_predict_orca.py (GPU) share: the crowds, the oracle's statement of the ORCA
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
