"""The device MPPI update's arithmetic restated in numpy float64 (include/crowdnav_amd.h, "Device MPPI update"): the refit's
ranks and best row, the weights exp((s_k - s_max) / temperature), and the weighted mean and deviation with every sum a python
loop over k from 0.0 — one IEEE operation per product and sum, in the header's order, so that everything but exp equals the
device bit for bit.  numpy only."""
import numpy as np

import plan_reference as ref


def weights(scores, temperature):
    """scores [K] -> (w [K], Z, k*): k* the rank-0 candidate, Z the sequential sum of w from 0.0."""
    s = np.asarray(scores, np.float64)
    top = int(np.flatnonzero(ref.ranks(s) == 0)[0])
    w = np.exp((s - s[top]) / np.float64(temperature))
    Z = np.float64(0.0)
    for k in range(len(s)):
        Z = Z + w[k]
    return w, Z, top


def mppi_update(scores, candidates, mean, std, best_actions, best_score, action, temperature, fit_std, keep_best, smoothing,
                min_std, v_pref):
    """One cn_plan_mppi_update on copies: scores [B, K], candidates [B, K, n, 2], v_pref float or [B], the rest as in struct
    cn_plan.  Returns a dict of order, best_actions, best_score, action, mean, std."""
    B, K, n = candidates.shape[:3]
    v_pref = np.broadcast_to(np.asarray(v_pref, np.float64), (B,))
    out = dict(order=np.zeros((B, K), np.int32), best_actions=best_actions.copy(), best_score=best_score.copy(),
               action=action.copy(), mean=mean.copy(), std=std.copy())
    keep = 1.0 - smoothing
    for b in range(B):
        order = np.zeros(K, np.int64)
        order[ref.ranks(scores[b])] = np.arange(K)
        out['order'][b] = order
        w, Z, top = weights(scores[b], temperature)
        assert top == order[0]
        if not keep_best or scores[b, top] > best_score[b]:
            out['best_actions'][b] = candidates[b, top]
            out['best_score'][b] = scores[b, top]
        num = np.zeros((n, 2))
        for k in range(K):
            num = num + w[k] * candidates[b, k]
        m = num / Z
        out['mean'][b] = smoothing * mean[b] + keep * m
        if fit_std:
            dev2 = np.zeros((n, 2))
            for k in range(K):
                d = candidates[b, k] - m
                dev2 = dev2 + w[k] * (d * d)
            sd = np.sqrt(dev2 / Z)
            out['std'][b] = np.maximum(min_std, smoothing * std[b] + keep * sd)
        out['action'][b] = ref.clip(out['mean'][b, 0], v_pref[b])
    return out
