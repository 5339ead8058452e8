"""Jam scenes: joint states built on purpose so that MANY agents of one workgroup of the fused rollout kernels have an
infeasible planar program in the same step (oracle/rvo2_oracle.cpp: lp2 fails, lp3 runs).  With the 5-half-plane programs
an infeasible agent takes 10 item lanes of the 3-D fallback, so up to 6 infeasible agents of a workgroup are served in one
pass and 7 or more take the multi-pass branch of `fused_solve` (crowdnav_amd/csrc/rollout_fused.h) — a state that seeded
rollouts do not reach (they produce 1-3 infeasible agents per step).

Why a huddle is infeasible: a human at rest whose nearest neighbour, also at rest, is d < 0.11 m away.  Both radii are 0.3,
ORCA adds 0.01 to each agent's own radius and dt is 0.25, so the overlap half-plane asks for v . n >= (0.61 - d) / (2 dt) >
1 = max_speed: linearProgram2 fails at its first line.  Overlapping humans end no episode; only the robot's collisions do.

Every scene: float64 [B, A, 8] in the project's field order (px, py, vx, vy, gx, gy, radius, v_pref), every radius 0.3, every
v_pref 1, the robot at rest at least 3 m from every human (it walks away from the crowd), no two agents coincident.
Deterministic: numpy RandomState with fixed seeds.  test_jam_scenes_host.py proves on the CPU, with the oracle alone, that
every scene is what its name says; test_fused_jam_parity.py runs them through every rollout kernel."""
import numpy as np

from support import np_of

T = 8  # steps per scene: by then every jam has dissolved to 0-1 infeasible agents, so quiet steps after a jam are included

ROBOT_AT, ROBOT_GOAL = (-6.0, 0.0), (-6.0, 9.0)
# where the humans that are not part of a huddle stand (relative to the huddle's centre; each walks to the mirrored point)
FAR = ((3.2, 3.0), (3.4, -3.1), (4.6, 0.3), (0.6, 4.7), (0.4, -4.8))
# pairs of rising_env seeds, one pair per workgroup: the two envs together have 1..6 infeasible agents in step 0 and 7 or more in
# step 1 (6 -> 8, 6 -> 7, 5 -> 7), with no episode end in T steps.  Found with the oracle: search_rising() lists the seeds among
# 0..19 999 whose env alone has 3 or more infeasible agents in step 1 and no fewer than in step 0 (3 -> 4: 0.5 % of the seeds,
# 3 -> 3: 0.7 %, 3 -> 5 and 2 -> 3: a handful); two such envs side by side are a rising workgroup.
RISING_SEEDS = ((417, 460), (711, 239), (7623, 7))


def blank(B, H):
    st = np.zeros((B, H + 1, 8))
    st[:, :, 6] = 0.3
    st[:, :, 7] = 1.0
    st[:, 0, 0:2] = ROBOT_AT
    st[:, 0, 4:6] = ROBOT_GOAL
    return st


def _place_far(env, first, centre, rng):
    """humans first.. of `env` (a [A, 8] view): metres from the huddle and from each other, at rest, walking across"""
    for n, i in enumerate(range(first, env.shape[0])):
        p = np.array(FAR[n]) + rng.uniform(-0.2, 0.2, size=2)
        env[i, 0:2] = centre + p
        env[i, 4:6] = centre - p


def cluster_env(env, k, rng, centre=(0.0, 0.0), box=0.04, min_gap=0.004):
    """humans 1..k of `env` huddled at rest inside a box of `box` metres (pairwise at least min_gap apart), their goals 4 m
    away in the direction they are displaced from the centre; the others far away"""
    centre = np.asarray(centre, dtype=np.float64)
    pts = []
    while len(pts) < k:
        p = rng.uniform(-0.5 * box, 0.5 * box, size=2)
        if all(np.hypot(*(p - q)) >= min_gap for q in pts):
            pts.append(p)
    for i, p in enumerate(pts):
        env[1 + i, 0:2] = centre + p
        env[1 + i, 4:6] = centre + 4.0 * p / np.hypot(*p)
    _place_far(env, 1 + k, centre, rng)


def lattice_env(env, cells, rng, pitch=0.04):
    """every human on a lattice of `pitch` metres around the origin (cells: integer (i, j) per human): the float32 squared
    distances between lattice neighbours tie exactly"""
    cells = np.asarray(cells, dtype=np.float64)
    assert len(cells) == env.shape[0] - 1 and len({tuple(c) for c in cells.tolist()}) == len(cells)
    env[1:, 0:2] = cells * pitch
    goal_dir = cells - cells.mean(axis=0) + rng.uniform(-0.05, 0.05, size=cells.shape)
    env[1:, 4:6] = 4.0 * goal_dir / np.hypot(goal_dir[:, 0], goal_dir[:, 1])[:, None]


def clusters(sizes, seed, H=5):
    """one env per entry of `sizes`: that many huddled humans, the other H - k far away"""
    rng = np.random.RandomState(seed)
    st = blank(len(sizes), H)
    for b, k in enumerate(sizes):
        cluster_env(st[b], k, rng, centre=rng.uniform(-0.5, 0.5, size=2))
    return st


def rising_env(env, seed):
    """a loose packing: every human at rest inside a box of 0.3-0.9 m, every goal at the box's centre.  Neighbours overlap by
    0.1-0.5 m: a human is infeasible only where its neighbours push it from opposite sides, and who is squeezed changes as the
    packing moves — the number of infeasible agents goes up as well as down from one step to the next."""
    rng = np.random.RandomState(seed)
    centre = rng.uniform(-0.5, 0.5, size=2)
    box = rng.uniform(0.3, 0.9)
    pts = []
    while len(pts) < env.shape[0] - 1:
        p = rng.uniform(-0.5 * box, 0.5 * box, size=2)
        if all(np.hypot(*(p - q)) >= 0.004 for q in pts):
            pts.append(p)
    env[1:, 0:2] = centre + np.array(pts)
    env[1:, 4:6] = centre


def rising(pairs=None):
    pairs = RISING_SEEDS if pairs is None else pairs
    st = blank(2 * len(pairs), 5)
    for n, pair in enumerate(pairs):
        for e, seed in enumerate(pair):
            rising_env(st[2 * n + e], seed)
    return st


def _lattice_ten():
    rng = np.random.RandomState(41)
    st = blank(2, 5)
    lattice_env(st[0], [(0, 0), (1, 0), (-1, 0), (0, 1), (0, -1)], rng)  # a plus: four neighbours of the centre tie
    lattice_env(st[1], [(0, 0), (1, 0), (0, 1), (1, 1), (2, 0)], rng)    # a square and one more
    return st


def _huddle_all(B, H, seed):
    return clusters([H] * B, seed, H=H)


HEADLINE = dict(num_humans=5, robot_visible=1)

# name -> (engine / oracle config, CROWDNAV_AMD_ENVS_PER_WAVE, builder).  Smallest launches first: a wrong barrier rule hangs a
# workgroup, and a two-env launch is what should meet it.
CASES = {
    'six': (HEADLINE, 2, lambda: clusters([3, 3], 11)),
    'seven': (HEADLINE, 2, lambda: clusters([3, 4], 12)),
    'two_five': (HEADLINE, 2, lambda: clusters([2, 5], 13)),
    'all_ten': (HEADLINE, 2, lambda: clusters([5, 5], 14)),
    'lattice_ten': (HEADLINE, 2, _lattice_ten),
    'half_empty': (HEADLINE, 2, lambda: clusters([5, 5, 5], 15)),
    'rising': (HEADLINE, 2, rising),
    'mixed_batch': (HEADLINE, 2, lambda: clusters([0, 0, 3, 3, 5, 5, 1, 1], 16)),
    # the geometries of rollout_fused_kernel<false>: every human of every env huddled; one full workgroup and one partial
    'h5_invisible': (dict(num_humans=5, robot_visible=0), 2, lambda: _huddle_all(3, 5, 21)),
    'h4_visible': (dict(num_humans=4, robot_visible=1), 2, lambda: _huddle_all(3, 4, 22)),
    'h3_visible_e3': (dict(num_humans=3, robot_visible=1), 3, lambda: _huddle_all(4, 3, 23)),
    'h2_visible_e4': (dict(num_humans=2, robot_visible=1), 4, lambda: _huddle_all(5, 2, 24)),
}
HEADLINE_CASES = tuple(n for n, c in CASES.items() if c[0] is HEADLINE)
OTHER_CASES = tuple(n for n, c in CASES.items() if c[0] is not HEADLINE)

_scenes, _runs = {}, {}


def scene(name, cases=CASES, made=_scenes):
    """(config, envs per workgroup, state [B, A, 8]) — built once; callers must not write into the state"""
    if name not in made:
        cfg, epw, build = cases[name]
        st = build()
        st.setflags(write=False)
        made[name] = (dict(cfg), epw, st)
    return made[name]


def workgroup_counts(fallback, epw):
    """fallback [T, B, A] bool -> infeasible agents per step and workgroup [T, ceil(B / epw)] (workgroup w = envs w epw ..)"""
    per_env = np.asarray(fallback).sum(axis=2)
    steps, B = per_env.shape
    W = -(-B // epw)
    padded = np.zeros((steps, W * epw), dtype=np.int64)
    padded[:, :B] = per_env
    return padded.reshape(steps, W, epw).sum(axis=2)


def oracle_run(oracle_mod, name, state=None, cfg=None, epw=None, steps=T):
    """The oracle's T steps from a scene: states [T + 1, B, A, 8] and global_time [T + 1, B] (row t: after t steps), per step
    reward / done / info / dmin [T, B], orca_vel [T, B, A, 2] float32, fallback [T, B, A] and counts [T, W].  The named scenes
    are run once and shared: callers must not write into the result."""
    if state is None:
        if name in _runs:
            return _runs[name]
        cfg, epw, state = scene(name)
    B = state.shape[0]
    o = oracle_mod.CrowdOracle(num_envs=B, robot_policy=1, **cfg)
    o.set_state(state, np.zeros(B))
    out = dict(states=[state.copy()], global_time=[np.zeros(B)], reward=[], done=[], info=[], dmin=[], orca_vel=[], fallback=[])
    for _ in range(steps):
        r = o.step(None, update=True)
        for k in ('reward', 'done', 'info', 'dmin', 'orca_vel'):
            out[k].append(r[k])
        out['fallback'].append(o.last_fallback())
        s, g = o.get_state()
        out['states'].append(s), out['global_time'].append(g)
    out = {k: np.stack(v) for k, v in out.items()}
    out['counts'] = workgroup_counts(out['fallback'], epw)
    for v in out.values():
        v.setflags(write=False)
    if name is not None:
        _runs[name] = out
    return out


def search_rising(oracle_mod, n_seeds=20000):
    """The search behind RISING_SEEDS: {(count in step 0, count in step 1): [seeds]} of the rising_env seeds whose env has at
    least 3 infeasible agents in step 1, no fewer than in step 0, finite states and no episode end in T steps."""
    st = blank(n_seeds, 5)
    for seed in range(n_seeds):
        rising_env(st[seed], seed)
    run = oracle_run(oracle_mod, None, state=st, cfg=HEADLINE, epw=1)
    c = run['counts']
    ok = ~run['done'].astype(bool).any(axis=0) & np.isfinite(run['states']).reshape(T + 1, n_seeds, -1).all(axis=(0, 2))
    found = {}
    for seed in np.flatnonzero(ok & (c[1] >= 3) & (c[1] >= c[0])):
        found.setdefault((int(c[0, seed]), int(c[1, seed])), []).append(int(seed))
    return found


def same_state(eng, want, steps, where):
    """the engine's state and global_time against the oracle's after `steps` steps: bit for bit"""
    state, gtime = (np_of(x) for x in eng.get_state())
    ws, wg = want['states'][steps], want['global_time'][steps]
    assert state.dtype == ws.dtype == np.float64, (state.dtype, ws.dtype)
    vel, wvel = state[:, :, 2:4].astype(np.float32), ws[:, :, 2:4].astype(np.float32)
    assert np.array_equal(vel.view(np.uint32), wvel.view(np.uint32)), ('velocity bits', where, steps)
    assert np.array_equal(state[:, :, 2:4], ws[:, :, 2:4]), ('velocity', where, steps)
    assert np.array_equal(state[:, :, 0:2], ws[:, :, 0:2]), ('position', where, steps)
    assert np.array_equal(state, ws), ('state', where, steps)
    assert np.array_equal(gtime, wg), ('global_time', where, steps)
