"""Neighbour-rank scenes: joint states written so that the pair phase of the fused rollout kernels (rollout_fused.h:
fused_pair_body — the agent's candidate distances fetched from the lanes of its group, stable rank = RVO2's sorted-insertion
slot) meets what a lane exchange can get wrong, at the smallest shapes that have it:

    2 envs (one full workgroup), 3 envs (the second workgroup half empty: pairs that do not exist rank as +inf), 1 env;
    the robot invisible to the humans (a missing pair inside every human's group);
    1, 2, 3 and 4 humans (fewer than five candidates: slots k >= NC of the rank loop);
    exact ties: an agent with two, and with three, neighbours at bit-equal float32 squared distance;
    a neighbour exactly at neighbor_dist^2 (out: the test is strict), one ulp-scale beyond it (out) and inside it (in);
    max_neighbors below the number of neighbours in range — also with the cut falling INSIDE a group of tied neighbours, where
    the tie rule (the earlier candidate first) alone decides who is kept.

Every position is a float32 value (so the float32 view ORCA gets is the float64 position itself), ties are built from signed
unit offsets on dyadic coordinates, every radius is 0.3 and every v_pref 1.  Agents stand 1-2 m apart at rest and walk
through each other's places, so the neighbours matter from the first step.  `neighbour_table` restates RVO2's neighbour
list (oracle/rvo2_oracle.cpp: offerNeighbor — float32 distSq, strict `<` against the range, sorted insertion that keeps the
earlier of equals first, the range shrinking to the last kept once the list is full) for a single-leaf kd-tree (<= 10
agents), which is what the rank of the pair phase must reproduce; test_rank_scenes_host.py holds every scene to its name with
it and ties the table to the oracle's velocities."""
import numpy as np

import jam_scenes

T = 4  # steps per scene

F = np.float32
JUST_OUT = float(np.nextafter(F(2.0), F(3.0)))   # 2 + 2^-22: squared > 4


def _just_inside(x):
    """the largest float32 y with float32(x x + y y) < 4: a point 25 degrees off the x axis, ulps inside the 2 m range"""
    x = F(x)
    y = F(np.sqrt(F(4.0) - x * x))
    while not F(x * x + y * y) < F(4.0):
        y = np.nextafter(y, F(0.0))
    return float(y)


X_IN = 1.8125
Y_IN = _just_inside(X_IN)


def blank(B, H):
    st = np.zeros((B, H + 1, 8))
    st[:, :, 6] = 0.3
    st[:, :, 7] = 1.0
    return st


def _env(env, robot, humans):
    """agent rows from (position, goal) pairs: at rest"""
    for i, (p, g) in enumerate([robot] + list(humans)):
        env[i, 0:2] = p
        env[i, 4:6] = g


# humans of the tie scenes: human 1 in the middle; 2, 3 (and 4) at squared distance 1.0 from it
_ROBOT = ((-2.5, 0.5), (3.0, -0.5))
_TIE2 = [((0.0, 0.0), (0.5, 3.0)), ((1.0, 0.0), (-3.0, 0.25)), ((-1.0, 0.0), (3.0, -0.25)), ((0.25, 1.5), (0.0, -3.0)),
         ((-0.5, -1.75), (0.75, 3.0))]
_TIE3 = [((0.0, 0.0), (0.5, 3.0)), ((1.0, 0.0), (-3.0, 0.25)), ((-1.0, 0.0), (3.0, -0.25)), ((0.0, 1.0), (0.25, -3.0)),
         ((-0.5, -1.75), (0.75, 3.0))]
# the range scene (neighbor_dist = 2): from human 1, human 2 is exactly 2 m away, 3 just beyond, 4 just inside, 5 close; human 1
# walks between 2 and 4, inside the velocity obstacle of either: whether each is a neighbour shows in its first step
_RANGE = [((0.0, 0.0), (3.0, 0.625)), ((2.0, 0.0), (-3.0, 0.0)), ((0.0, JUST_OUT), (0.5, -3.0)), ((X_IN, Y_IN), (-3.0, -0.5)),
          ((-1.0, -0.75), (-0.5, 3.0))]


def _scene(B, H, humans, shift=0.0):
    """env b: the first H of `humans`, env b's copy moved by b * shift metres in y (a float32-exact shift keeps the ties)"""
    st = blank(B, H)
    for b in range(B):
        dy = np.array([0.0, b * shift])
        _env(st[b], (np.add(_ROBOT[0], dy), np.add(_ROBOT[1], dy)), [(np.add(p, dy), np.add(g, dy)) for p, g in humans[:H]])
    return st


VISIBLE5 = dict(num_humans=5, robot_visible=1)

# name -> (engine / oracle config, CROWDNAV_AMD_ENVS_PER_WAVE, builder); smallest launches first
CASES = {
    'tie2_one_env': (VISIBLE5, 2, lambda: _scene(1, 5, _TIE2)),
    'tie2': (VISIBLE5, 2, lambda: _scene(2, 5, _TIE2, 0.5)),
    'tie3_three_envs': (VISIBLE5, 2, lambda: _scene(3, 5, _TIE3, 0.25)),
    'range': (dict(VISIBLE5, neighbor_dist=2.0), 2, lambda: _scene(3, 5, _RANGE)),  # (no shift: Y_IN + b / 2 is no float32)
    'keep3': (dict(VISIBLE5, max_neighbors=3), 2, lambda: _scene(3, 5, _TIE2, 0.5)),
    'keep2_cut_in_tie': (dict(VISIBLE5, max_neighbors=2), 2, lambda: _scene(3, 5, _TIE3, 0.25)),
    # the geometries of rollout_fused_kernel<false>
    'invisible': (dict(num_humans=5, robot_visible=0), 2, lambda: _scene(3, 5, _TIE3, 0.25)),
    'h4': (dict(num_humans=4, robot_visible=1), 2, lambda: _scene(3, 4, _TIE3, 0.25)),
    'h3': (dict(num_humans=3, robot_visible=1), 2, lambda: _scene(3, 3, _TIE2, 0.5)),
    'h2': (dict(num_humans=2, robot_visible=1), 2, lambda: _scene(3, 2, _TIE2, 0.5)),
    'h1': (dict(num_humans=1, robot_visible=1), 2, lambda: _scene(3, 1, _TIE2, 0.5)),
    'h4_keep2_invisible': (dict(num_humans=4, robot_visible=0, max_neighbors=2), 2, lambda: _scene(3, 4, _TIE3, 0.25)),
}
HEADLINE_CASES = tuple(n for n, c in CASES.items() if c[0]['num_humans'] == 5 and c[0]['robot_visible'] == 1)

_scenes, _runs = {}, {}


def scene(name):
    return jam_scenes.scene(name, CASES, _scenes)


def neighbour_table(env, robot_visible, neighbor_dist=10.0, max_neighbors=10):
    """RVO2's neighbour list of every agent of one env [A, 8], single-leaf kd-tree: per agent a dict with
        offered   [(float32 distSq, id)] in the order the leaf offers them (ascending id, self left out; the robot sees the
                  humans, a human the other humans and — if visible — the robot, whose simulator id is the last)
        kept      [(distSq, id)] the list after every offer
        in_range  how many of the offered are inside neighbor_dist^2"""
    f = np.asarray(env, dtype=np.float64).astype(F)
    A = f.shape[0]
    out = []
    for q in range(A):
        if q == 0:
            ids = list(range(1, A))
        else:  # a human's simulator: the humans in order, then the robot (orca.py builds it that way)
            ids = [j for j in range(1, A) if j != q] + ([0] if robot_visible else [])
        offered = []
        for j in ids:
            dx, dy = F(f[q, 0] - f[j, 0]), F(f[q, 1] - f[j, 1])
            offered.append((F(F(dx * dx) + F(dy * dy)), j))
        base = F(F(neighbor_dist) * F(neighbor_dist))
        rng, kept = base, []
        for d, j in offered:
            if max_neighbors > 0 and d < rng:
                if len(kept) < max_neighbors:
                    kept.append((d, j))
                i = len(kept) - 1
                while i != 0 and d < kept[i - 1][0]:
                    kept[i] = kept[i - 1]
                    i -= 1
                kept[i] = (d, j)
                if len(kept) == max_neighbors:
                    rng = kept[-1][0]
        out.append(dict(offered=offered, kept=kept, in_range=sum(1 for d, _ in offered if d < base)))
    return out


def oracle_run(oracle_mod, name, cfg=None, steps=T):
    """The oracle's steps from a scene (as jam_scenes.oracle_run): states [T + 1, B, A, 8], global_time [T + 1, B], per step
    reward / done / info / dmin [T, B], orca_vel [T, B, A, 2] float32.  `cfg`: another config for the same state (not cached)."""
    if cfg is None and name in _runs:
        return _runs[name]
    own, _, state = scene(name)
    use = own if cfg is None else cfg
    B = state.shape[0]
    o = oracle_mod.CrowdOracle(num_envs=B, robot_policy=1, **use)
    o.set_state(state, np.zeros(B))
    out = dict(states=[state.copy()], global_time=[np.zeros(B)], reward=[], done=[], info=[], dmin=[], orca_vel=[])
    for _ in range(steps):
        r = o.step(None, update=True)
        for k in ('reward', 'done', 'info', 'dmin', 'orca_vel'):
            out[k].append(r[k])
        s, g = o.get_state()
        out['states'].append(s), out['global_time'].append(g)
    out = {k: np.stack(v) for k, v in out.items()}
    for v in out.values():
        v.setflags(write=False)
    if cfg is None:
        _runs[name] = out
    return out
