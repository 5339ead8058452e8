"""Host-side reading of BatchedCrowdSim.rollout_trace / rollout_actions(trace=True) results (numpy only, no device work).

A trace is the dict either of them returns: state8 [B, n, A, 8], episode [B, n], step [B, n] and, with rewards, reward / info /
dmin [B, n] — row [b, t] is the t-th step of that call (include/crowdnav_amd.h: cn_rollout_trace, cn_rollout_actions).  episodes() cuts one trace,
or the traces of consecutive calls, into the episodes the envs ran: what the reference keeps as env.states per episode
(crowd_sim/envs/crowd_sim.py:246,393)."""
import numpy as np

from ._lib import COLLISION, REACH_GOAL, TIMEOUT

_OPTIONAL = ('reward', 'info', 'dmin')


def _host(x):
    if hasattr(x, 'detach'):  # a torch tensor, on any device
        x = x.detach().cpu().numpy()
    return np.asarray(x)


def episodes(trace, env_offset=0, env_stride=None):
    """{global episode id: dict(state8 [T, A, 8], reward [T], info [T], dmin [T], complete)} of one trace or of a list of traces
    from consecutive calls on one engine (in call order; every env's rows are joined along the step axis).

    The id of env b's ordinal j is env_offset + b + j * env_stride, as cn_rollout_io numbers it (env_stride defaults to the
    trace's own env count: one engine running the whole job).  Rows whose episode is -1 belong to no episode and are dropped.
    reward / info / dmin are None when the traces were recorded without rewards (all of them must agree).
    complete: True when the episode's first row (step 0) and its last transition (an info of ReachGoal, Collision or Timeout)
    both lie inside the traces given, with every step between them; False otherwise — an episode cut by a call boundary, or
    with rows missing because an untraced rollout() ran in between; None without rewards (the last transition cannot be told
    from the rows alone)."""
    traces = [trace] if isinstance(trace, dict) else list(trace)
    if not traces:
        return {}
    have = [k for k in _OPTIONAL if traces[0].get(k) is not None]
    for t in traces:
        if [k for k in _OPTIONAL if t.get(k) is not None] != have:
            raise ValueError('trace.episodes: some traces carry reward / info / dmin and some do not')
    cols = {k: np.concatenate([_host(t[k]) for t in traces], axis=1) for k in ['state8', 'episode', 'step'] + have}
    ep, st = cols['episode'], cols['step']
    B = ep.shape[0]
    if cols['state8'].shape[:2] != ep.shape or st.shape != ep.shape:
        raise ValueError('trace.episodes: state8 %s, episode %s and step %s do not belong together'
                         % (cols['state8'].shape, ep.shape, st.shape))
    stride = B if env_stride is None else int(env_stride)
    out = {}
    for b in range(B):
        rows = np.flatnonzero(ep[b] >= 0)
        if not len(rows):
            continue
        ords = ep[b, rows]
        cuts = np.flatnonzero(np.diff(ords) != 0) + 1
        for seg in np.split(rows, cuts):
            steps = st[b, seg]
            item = dict(state8=cols['state8'][b, seg])
            for k in _OPTIONAL:
                item[k] = cols[k][b, seg] if k in have else None
            if 'info' in have:
                whole = steps[0] == 0 and np.array_equal(steps, np.arange(len(seg)))
                item['complete'] = bool(whole and int(item['info'][-1]) in (REACH_GOAL, COLLISION, TIMEOUT))
            else:
                item['complete'] = None
            gid = int(env_offset) + b + int(ep[b, seg[0]]) * stride
            if gid in out:
                raise ValueError('trace.episodes: episode %d appears twice (env %d): are the traces in call order?' % (gid, b))
            out[gid] = item
    return out
