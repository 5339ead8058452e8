"""What the predict_orca_goals suites, host (no GPU) and GPU, share: the fixed goal maps of the oracle comparison, the eight
rotations of the packing test, and the state an oracle is given for one mode of a table of goals."""
import numpy as np

PARKED_X = 0.5e6  # scenario_device.h: is_parked


def parked(state):
    """[B, H] bool: the placeholders of the `mixed` rule, which ignore their rows of a table of goals."""
    return np.asarray(state)[:, 1:, 0] >= PARKED_X


def goal_maps(state, crowd):
    """float64 [B, 3, H, 2]: mode 0 the humans' own goals, mode 1 every goal turned a quarter circle about the origin
    ((x, y) -> (-y, x)), mode 2 every goal the human's own position.  h5_mixed: mode 2 is every goal the origin instead — its
    scenes hold one to three humans, too far apart for a standing one to be pushed (the oracle's table is all zeros), so there
    the humans are sent to meet each other (test_predict_orca_goals_host.py: test_the_goal_maps_bite)."""
    state = np.asarray(state, dtype=np.float64)
    own = state[:, 1:, 4:6]
    turned = np.stack([-own[..., 1], own[..., 0]], axis=-1)
    third = np.zeros_like(own) if crowd == 'h5_mixed' else state[:, 1:, 0:2]
    return np.ascontiguousarray(np.stack([own, turned, third], axis=1))


def rotations(state, M=8):
    """float64 [B, M, H, 2]: the humans' goals turned about the origin by m / M of a full circle, m = 0 .. M - 1."""
    own = np.asarray(state, dtype=np.float64)[:, 1:, 4:6]
    out = np.empty((len(own), M) + own.shape[1:])
    for m in range(M):
        c, s = np.cos(2.0 * np.pi * m / M), np.sin(2.0 * np.pi * m / M)
        out[:, m, :, 0], out[:, m, :, 1] = c * own[..., 0] - s * own[..., 1], s * own[..., 0] + c * own[..., 1]
    out[:, 0] = own
    return out


def regoaled(state, goals):
    """state [B, A, 8] with the humans heading for goals [B, H, 2] — what mode m of predict_orca_goals steps; the parked
    placeholders keep their own."""
    out = np.array(state, dtype=np.float64, copy=True)
    moved = ~parked(state)
    out[:, 1:, 4:6][moved] = np.asarray(goals, dtype=np.float64)[moved]
    return out
