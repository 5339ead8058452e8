"""The unicycle planners' arithmetic restated in numpy float64 (include/crowdnav_amd.h, "Unicycle planners"): the (v, r) clip,
the draw, the prior's recurrence, the shift and the MPPI action's clip — one IEEE operation per product and sum, in the header's
order.  Philox, the Box-Muller pair, the ranks, the refit and the MPPI sums are plan_reference's and plan_mppi_reference's:
they are component-wise and know nothing of what a row means.  Everything but the draw's log / cos / sin and the prior's atan2 /
cos / sin equals the device bit for bit.  numpy only."""
import numpy as np

import plan_mppi_reference as mref
import plan_reference as ref

PI, TWO_PI = 3.141592653589793, 6.283185307179586


def clip(a, v_pref, R):
    """a float64 [..., 2] rows (v, r) onto the box [0, v_pref] x [-R, R]; v_pref broadcasts over the leading axes."""
    a = np.asarray(a, np.float64)
    v, r = a[..., 0], a[..., 1]
    v_pref = np.broadcast_to(np.asarray(v_pref, np.float64), v.shape)
    v = np.where(v < 0.0, 0.0, np.where(v > v_pref, v_pref, v))
    r = np.where(r < -R, -R, np.where(r > R, R, r))
    return np.stack([v, r], axis=-1)


def draw(mean, std, K, seed, counter, v_pref, R):
    """mean, std float64 [B, n, 2]; v_pref float or [B] -> candidates [B, K, n, 2], rows (v, r)."""
    B, n = mean.shape[:2]
    z0, z1, _ = ref.normal_pairs(B, K, n, seed, counter)
    a = np.empty((B, K, n, 2))
    a[..., 0] = mean[:, None, :, 0] + std[:, None, :, 0] * z0
    a[..., 1] = mean[:, None, :, 1] + std[:, None, :, 1] * z1
    a[:, 0] = mean
    return clip(a, np.broadcast_to(np.asarray(v_pref, np.float64), (B,))[:, None, None], R)


def wrap(d, real=np.float64):
    """d -> the same angle in [-pi, pi), by the header's explicit operations."""
    d = real(d)
    return d - real(TWO_PI) * np.floor((d + real(PI)) / real(TWO_PI))


def prior_rows(px, py, gx, gy, v_pref, theta, dt, R, n, turns=None, real=np.float64):
    """The prior of ONE env: rows [n, 2] of (v, r).  turns (a list): receives the unclipped turn of every step that has one.
    real: the type every operation is made in — np.float64, the device's; np.longdouble states the same recurrence on the same
    float64 inputs (pi and 2 pi too) at a higher precision, the truth two float64 evaluations are measured against."""
    px, py, th = real(px), real(py), real(theta)
    gx, gy, v_pref, dt, R = real(gx), real(gy), real(v_pref), real(dt), real(R)
    rows = np.zeros((n, 2), dtype=real)
    for t in range(n):
        dx, dy = gx - px, gy - py
        dist = np.sqrt(dx * dx + dy * dy)
        if not dist > 0.0:
            continue
        reach = dist / dt
        speed = v_pref if v_pref < reach else reach
        turn = wrap(np.arctan2(dy, dx) - th, real)
        if turns is not None:
            turns.append(float(turn))
        r = -R if turn < -R else (R if turn > R else turn)
        rows[t] = speed, r
        th = th + r
        px = px + np.cos(th) * speed * dt
        py = py + np.sin(th) * speed * dt
    return rows


def prior(state8, theta, dt, R, n, turns=None, real=np.float64):
    """state8 [B, A, 8] (px, py, vx, vy, gx, gy, radius, v_pref), agent 0 the robot; theta [B] -> the prior [B, n, 2]."""
    return np.stack([prior_rows(r[0], r[1], r[4], r[5], r[7], th, dt, R, n, turns, real) for r, th in zip(state8[:, 0], theta)])


def reset(state8, theta, dt, R, mean, std, init_std, std_rotation, mask=None):
    """cn_plan_reset on copies -> (mean, std)."""
    mean, std = mean.copy(), std.copy()
    sel = np.ones(len(mean), bool) if mask is None else np.asarray(mask).astype(bool)
    mean[sel] = prior(state8, theta, dt, R, mean.shape[1])[sel]
    std[sel] = init_std, std_rotation
    return mean, std


def shift(state8, theta, dt, R, active, cur_steps, mean, std, init_std, std_rotation):
    """cn_plan_shift on copies -> (mean, std): state8 and theta are the state AFTER the real step."""
    mean, std = mean.copy(), std.copy()
    p = prior(state8, theta, dt, R, mean.shape[1])
    for b in range(len(mean)):
        if not active[b]:
            continue
        if cur_steps[b] == 0:
            mean[b] = p[b]
        else:
            mean[b, :-1] = mean[b, 1:].copy()
        std[b] = init_std, std_rotation
    return mean, std


def mppi_update(scores, candidates, mean, std, best_actions, best_score, action, temperature, fit_std, keep_best, smoothing,
                min_std, v_pref, R):
    """plan_mppi_reference.mppi_update with the action clipped to the box: the sums do not depend on the clip."""
    out = mref.mppi_update(scores, candidates, mean, std, best_actions, best_score, action, temperature, fit_std, keep_best,
                           smoothing, min_std, v_pref)
    v_pref = np.broadcast_to(np.asarray(v_pref, np.float64), (len(mean),))
    out['action'] = clip(out['mean'][:, 0], v_pref, R)
    return out
