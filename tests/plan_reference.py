"""The device CEM planner's arithmetic restated in numpy float64 (include/crowdnav_amd.h, "Device CEM planner"): Philox4x32-10,
the draw and its clip, the refit, the goal-directed prior and the shift — one IEEE operation per product and sum, in the
header's order, so that everything but the draw's log / cos / sin equals the device bit for bit.  numpy only."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xffffffff)


def philox4x32_10(counter, key):
    """counter: uint32 [..., 4], key: uint32 [..., 2] (broadcast against each other) -> uint32 [..., 4]."""
    counter, key = np.asarray(counter, np.uint64), np.asarray(key, np.uint64)
    shape = np.broadcast_shapes(counter.shape[:-1], key.shape[:-1])
    c = [np.broadcast_to(counter[..., i], shape).copy() for i in range(4)]
    k = [np.broadcast_to(key[..., i], shape).copy() for i in range(2)]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]  # 32 x 32 -> 64 bits: no overflow
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + np.uint64(W0)) & MASK, (k[1] + np.uint64(W1)) & MASK]
    return np.stack(c, axis=-1).astype(np.uint32)


def normal_pairs(B, K, n, seed, counter):
    """(z0, z1) float64 [B, K, n] each, and r [B, K, n]: the Box-Muller pair of the block with counter words (t, k, b, counter)."""
    b, k, t = np.meshgrid(np.arange(B), np.arange(K), np.arange(n), indexing='ij')
    ctr = np.stack([t, k, b, np.full_like(t, int(counter) & 0xffffffff)], axis=-1)
    w = philox4x32_10(ctr, np.array([seed & 0xffffffff, (seed >> 32) & 0xffffffff])).astype(np.uint64)
    f = lambda x: x.astype(np.float64)  # noqa: E731
    u1 = (f(w[..., 0] >> np.uint64(5)) * 67108864.0 + f(w[..., 1] >> np.uint64(6)) + 1.0) / 9007199254740992.0
    u2 = (f(w[..., 2] >> np.uint64(5)) * 67108864.0 + f(w[..., 3] >> np.uint64(6))) / 9007199254740992.0
    r = np.sqrt(-2.0 * np.log(u1))
    ang = (2.0 * np.pi) * u2
    return r * np.cos(ang), r * np.sin(ang), r


def clip(a, v_pref):
    """a float64 [..., 2] scaled onto the disc of radius v_pref (broadcast over the leading axes) where it lies outside."""
    ax, ay = a[..., 0], a[..., 1]
    nrm = np.sqrt(ax * ax + ay * ay)
    with np.errstate(divide='ignore', invalid='ignore'):
        s = np.where(nrm > v_pref, v_pref / nrm, 1.0)
    out = np.where((nrm > v_pref)[..., None], np.stack([ax * s, ay * s], axis=-1), a)
    return out


def draw(mean, std, K, seed, counter, v_pref):
    """mean, std float64 [B, n, 2]; v_pref float or [B] -> candidates [B, K, n, 2]."""
    B, n = mean.shape[:2]
    z0, z1, _ = normal_pairs(B, K, n, seed, counter)
    a = np.empty((B, K, n, 2))
    a[..., 0] = mean[:, None, :, 0] + std[:, None, :, 0] * z0
    a[..., 1] = mean[:, None, :, 1] + std[:, None, :, 1] * z1
    a[:, 0] = mean
    return clip(a, np.broadcast_to(np.asarray(v_pref, np.float64), (B,))[:, None, None])


def ranks(scores):
    """scores [K] -> rank [K]: #{j : s_j > s_k, or s_j == s_k and j < k}."""
    s = np.asarray(scores, np.float64)
    j = np.arange(len(s))
    return ((s[None, :] > s[:, None]) | ((s[None, :] == s[:, None]) & (j[None, :] < j[:, None]))).sum(axis=1)


def refit(scores, candidates, mean, std, best_actions, best_score, action, E, keep_best, smoothing, min_std):
    """One cn_plan_refit on copies: scores [B, K], candidates [B, K, n, 2], the rest as in struct cn_plan.  Returns a dict
    of order, best_actions, best_score, action, mean, std."""
    B, K, n = candidates.shape[:3]
    out = dict(order=np.zeros((B, K), np.int32), best_actions=best_actions.copy(), best_score=best_score.copy(),
               action=action.copy(), mean=mean.copy(), std=std.copy())
    for b in range(B):
        order = np.zeros(K, np.int64)
        order[ranks(scores[b])] = np.arange(K)
        out['order'][b] = order
        top = order[0]
        if not keep_best or scores[b, top] > best_score[b]:
            out['best_actions'][b] = candidates[b, top]
            out['best_score'][b] = scores[b, top]
            out['action'][b] = candidates[b, top, 0]
        total = np.zeros((n, 2))
        for e in range(E):
            total = total + candidates[b, order[e]]
        m = total / float(E)
        dev2 = np.zeros((n, 2))
        for e in range(E):
            d = candidates[b, order[e]] - m
            dev2 = dev2 + d * d
        sd = np.sqrt(dev2 / float(E))
        keep = 1.0 - smoothing
        out['mean'][b] = smoothing * mean[b] + keep * m
        out['std'][b] = np.maximum(min_std, smoothing * std[b] + keep * sd)
    return out


def prior(state8, dt):
    """state8 [B, A, 8] (px, py, vx, vy, gx, gy, radius, v_pref), agent 0 the robot -> the prior's action [B, 2]."""
    r = state8[:, 0]
    dx, dy = r[:, 4] - r[:, 0], r[:, 5] - r[:, 1]
    dist = np.sqrt(dx * dx + dy * dy)
    speed = np.minimum(r[:, 7], dist / dt)
    with np.errstate(divide='ignore', invalid='ignore'):
        a = np.stack([(dx / dist) * speed, (dy / dist) * speed], axis=-1)
    return np.where((dist > 0.0)[:, None], a, 0.0)


def reset(state8, dt, mean, std, init_std, mask=None):
    """cn_plan_reset on copies -> (mean, std)."""
    mean, std = mean.copy(), std.copy()
    sel = np.ones(len(mean), bool) if mask is None else np.asarray(mask).astype(bool)
    mean[sel] = prior(state8, dt)[sel][:, None, :]
    std[sel] = init_std
    return mean, std


def shift(state8, dt, active, cur_steps, mean, std, init_std):
    """cn_plan_shift on copies -> (mean, std): state8 is the state AFTER the real step."""
    mean, std = mean.copy(), std.copy()
    p = prior(state8, dt)
    for b in range(len(mean)):
        if not active[b]:
            continue
        if cur_steps[b] == 0:
            mean[b] = p[b]
        else:
            mean[b, :-1] = mean[b, 1:].copy()
        std[b] = init_std
    return mean, std
