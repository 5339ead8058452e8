"""Tables of predicted human velocities for BatchedCrowdSim.lookahead_paths / plan_cem_paths / plan_mppi_paths
(cn_lookahead_paths): human_vel[b, t, h] is the (vx, vy) human h of env b takes during step t of the horizon.

    constant_velocity(state8, n)       every human keeps the velocity it has: the 'constant_velocity' human model as a table
    to_goal(state8, n, dt)             every human heads straight for its goal at v_pref and stops there
    from_positions(start_xy, pos, dt)  the velocities that carry the humans through predicted positions
    stack_modes(*tables)               M such tables as the [B, M, n, H, 2] of lookahead_modes / plan_*_modes

constant_velocity and to_goal also exist on the device: BatchedCrowdSim.predict (cn_predict) makes the same tables from the
engine's own state in one launch, bit for bit what these functions give on get_state() — they are its oracle — and
plan_predict_rollout runs the whole closed loop on them without the host.  A predictor of the caller's own goes through the
functions here and the per-step calls.

A third predictor exists on the device only: BatchedCrowdSim.predict_orca (cn_predict_orca) steps the humans with the engine's
own ORCA code, the robot unseen — humans that avoid each other, between to_goal (straight through every other human) and the
full 'orca' lookahead (humans that react to each candidate robot path) — and plan_predict_orca_rollout plans on it in closed
loop.  It has no host form here: its oracle is the environment itself, stepped with robot_visible = 0.
BatchedCrowdSim.predict_orca_robot (cn_predict_orca_robot) is the same with the robot in the humans' sight on a sequence of
actions the caller names — the plan's mean, say: plan_predict_orca_nominal_rollout — one prediction per planning step.
BatchedCrowdSim.predict_orca_goals (cn_predict_orca_goals) is predict_orca for M hypotheses about where the humans are heading,
side by side in one launch: the goals are an argument, [B, M, H, 2], not the simulator's.

    goal_hypotheses(state8, M, base, reach, ...)  such a table of goals, sampled around each human's heading (or its goal)

is BatchedCrowdSim.goal_hypotheses (cn_goal_hypotheses) restated in numpy, its oracle, with a small Philox of its own — and the
table for a caller whose predictor is not the engine's.

torch / numpy only, no device code: a numpy state gives a numpy table, a torch state a torch table on the same device.  Each
returns [B, n, H, 2] float64, H = A - 1 humans (state8 is get_state()'s [B, A, 8]: px, py, vx, vy, gx, gy, radius, v_pref; row 0 is
the robot).  Under the `mixed` rule the parked placeholders stand still at their goals with zero velocity, so constant_velocity
and to_goal give them zeros, as cn_lookahead_paths asks."""
import numpy as np
import torch


def _f64(x):
    """(x as a float64 torch tensor, whether the caller gave numpy)."""
    if torch.is_tensor(x):
        return x.to(torch.float64), False
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float64))), True


def _back(t, as_numpy):
    t = t.contiguous()
    return t.numpy() if as_numpy else t


def _sqrt(x):
    """The correctly rounded square root.  torch's float64 sqrt on the CPU goes through a vector math library that is within an
    ulp but not always correctly rounded (about 1 % of arguments differ); numpy's is the IEEE one, as is torch's on the device.
    cn_predict restates to_goal bit for bit, so every operation here has to be the IEEE one."""
    return torch.from_numpy(np.sqrt(x.numpy())) if x.device.type == 'cpu' else torch.sqrt(x)


def _humans(state8):
    s, as_numpy = _f64(state8)
    if s.dim() != 3 or s.shape[1] < 2 or s.shape[2] != 8:
        raise ValueError('state8 must be [B, A >= 2, 8], got %s' % (tuple(s.shape),))
    return s[:, 1:], as_numpy


def constant_velocity(state8, n):
    """human_vel[b, t, h] = the human's state velocity for every t: lookahead_paths then gives, bit for bit, what lookahead()
    gives under set_lookahead_human_model('constant_velocity')."""
    humans, as_numpy = _humans(state8)
    n = int(n)
    if n < 0:
        raise ValueError('n must be >= 0')
    return _back(humans[:, None, :, 2:4].expand(-1, n, -1, -1).clone(), as_numpy)


def to_goal(state8, n, dt):
    """Every human walks straight towards its goal at its v_pref and stops there.  Per step, with d = goal - p and dist = |d|:
    dist == 0: (0, 0); dist <= v_pref dt: d / dt, the shortened last step that lands on the goal; else (d / dist) v_pref.  Then
    p <- p + v dt, as the lookahead moves it."""
    humans, as_numpy = _humans(state8)
    n, dt = int(n), float(dt)
    if n < 0 or not dt > 0.0:
        raise ValueError('n must be >= 0 and dt > 0')
    p, goal, v_pref = humans[..., 0:2].clone(), humans[..., 4:6], humans[..., 7:8]
    out = torch.zeros((humans.shape[0], n, humans.shape[1], 2), dtype=torch.float64, device=humans.device)
    for t in range(n):
        d = goal - p
        dist = _sqrt(d[..., 0:1] * d[..., 0:1] + d[..., 1:2] * d[..., 1:2])
        cruise = d / torch.where(dist > 0.0, dist, torch.ones_like(dist)) * v_pref
        v = torch.where(dist <= v_pref * dt, d / dt, cruise)
        v = torch.where(dist > 0.0, v, torch.zeros_like(v))
        out[:, t] = v
        p = p + v * dt
    return _back(out, as_numpy)


def from_positions(start_xy, positions, dt):
    """start_xy [B, H, 2]: where the humans are now (state8[:, 1:, 0:2]); positions [B, n, H, 2]: where the predictor puts them
    after step 0, 1, .. n - 1.  human_vel[:, t] = (positions[:, t] - the position before it) / dt.  (The lookahead moves a human
    by p + v dt, which lands within an ulp or so of the predicted position, not always on it.)"""
    start, as_numpy = _f64(start_xy)
    pos, _ = _f64(positions)
    dt = float(dt)
    if pos.dim() != 4 or pos.shape[3] != 2 or tuple(start.shape) != (pos.shape[0], pos.shape[2], 2):
        raise ValueError('start_xy must be [B, H, 2] and positions [B, n, H, 2], got %s and %s' % (tuple(start.shape), tuple(pos.shape)))
    if not dt > 0.0:
        raise ValueError('dt must be > 0')
    before = torch.cat([start[:, None].to(pos.device), pos[:, :-1]], dim=1)
    return _back((pos - before) / dt, as_numpy)


def _philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11) on uint64 arrays that hold 32-bit words; returns the four output words."""
    mask, sh = np.uint64(0xffffffff), np.uint64(32)
    c0, c1, c2, c3 = (np.asarray(c, np.uint64) for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2  # 32 x 32 -> 64 bits: no overflow
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ k0, p1 & mask, (p0 >> sh) ^ c3 ^ k1, p0 & mask
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & mask, (k1 + np.uint64(0xBB67AE85)) & mask
    return c0, c1, c2, c3


GOAL_BASES = ('engine', 'heading')


def goal_hypotheses(state8, M, base='heading', reach=None, std_heading=0.0, std_distance=0.0, nominal_first=True, seed=0,
                    counter=0):
    """M sets of hypothesised human goals, float64 [B, M, H, 2]: BatchedCrowdSim.goal_hypotheses (cn_goal_hypotheses) restated
    in numpy float64, operation for operation — its oracle, equal to it apart from the device's log, cos and sin — and the
    table for a caller whose predictor is their own.  With (p, v, g) of human h its nominal offset d is g - p (base 'engine')
    or `reach` metres along v, (0, 0) for a standing human (base 'heading'; `reach` is required there, g is not read).  Mode 0
    under nominal_first is the nominal goal: g itself, or p + d.  Every other mode m is p + scale R(rot) d with
    rot = std_heading z1, scale = max(0, 1 + std_distance z2), (z1, z2) the Box-Muller pair of the Philox4x32-10 block with
    counter words (h, m, b, counter) and key (seed & 0xffffffff, seed >> 32): a row depends on neither B, M nor H."""
    humans, as_numpy = _humans(state8)
    device = humans.device
    s = humans.detach().cpu().numpy()
    M = int(M)
    if base not in GOAL_BASES:
        raise ValueError('goal_hypotheses: base must be one of %s, got %r' % (GOAL_BASES, base))
    if not 1 <= M <= 8:
        raise ValueError('goal_hypotheses: M must be in 1..8, got %d' % M)
    heading = base == 'heading'
    if heading and (reach is None or not (np.isfinite(reach) and reach > 0.0)):
        raise ValueError('goal_hypotheses: base \'heading\' needs reach > 0 (metres along the velocity), got %r' % (reach,))
    for name, v in (('std_heading', std_heading), ('std_distance', std_distance)):
        if not (np.isfinite(v) and v >= 0.0):
            raise ValueError('goal_hypotheses: %s must be >= 0 and finite, got %r' % (name, v))
    B, H = s.shape[:2]
    px, py, vx, vy, gx, gy = (s[:, None, :, i] for i in range(6))  # [B, 1, H]
    if heading:
        speed = np.sqrt(vx * vx + vy * vy)
        moving = speed > 0.0
        safe = np.where(moving, speed, 1.0)
        dx, dy = np.where(moving, (vx / safe) * float(reach), 0.0), np.where(moving, (vy / safe) * float(reach), 0.0)
    else:
        dx, dy = gx - px, gy - py
    b, m, h = np.arange(B)[:, None, None], np.arange(M)[None, :, None], np.arange(H)[None, None, :]
    seed = int(seed)
    w = _philox4x32_10(h, m, b, np.uint64(int(counter) & 0xffffffff), seed & 0xffffffff, (seed >> 32) & 0xffffffff)
    f = [x.astype(np.float64) for x in (w[0] >> np.uint64(5), w[1] >> np.uint64(6), w[2] >> np.uint64(5), w[3] >> np.uint64(6))]
    u1 = (f[0] * 67108864.0 + f[1] + 1.0) / 9007199254740992.0
    u2 = (f[2] * 67108864.0 + f[3]) / 9007199254740992.0
    r, ang = np.sqrt(-2.0 * np.log(u1)), 6.283185307179586 * u2
    z1, z2 = r * np.cos(ang), r * np.sin(ang)
    rot = float(std_heading) * z1
    scale = 1.0 + float(std_distance) * z2
    scale = np.where(scale < 0.0, 0.0, scale)
    c, sn = np.cos(rot), np.sin(rot)
    out = np.stack([px + scale * (c * dx - sn * dy), py + scale * (sn * dx + c * dy)], axis=-1)
    if nominal_first:
        out[:, 0] = np.stack([px + dx, py + dy], axis=-1)[:, 0] if heading else s[:, :, 4:6]
    out = np.ascontiguousarray(out)
    return out if as_numpy else torch.from_numpy(out).to(device)


def stack_modes(*tables):
    """M tables [B, n, H, 2] of one shape -> [B, M, n, H, 2] float64, the human_vel of lookahead_modes / plan_cem_modes /
    plan_mppi_modes (cn_lookahead_modes): mode m is tables[m].  numpy unless every table is a torch tensor; then torch, on the
    first table's device."""
    if not tables:
        raise ValueError('stack_modes: at least one table')
    as_numpy = not all(torch.is_tensor(t) for t in tables)
    ts = [_f64(t.cpu() if as_numpy and torch.is_tensor(t) else t)[0] for t in tables]
    for t in ts:
        if t.dim() != 4 or t.shape[3] != 2 or t.shape != ts[0].shape:
            raise ValueError('stack_modes: tables must share one shape [B, n, H, 2], got %s' % ([tuple(t.shape) for t in ts],))
    return _back(torch.stack([t.to(ts[0].device) for t in ts], dim=1), as_numpy)
