"""Occupancy-map settings other than the shipped 4 x 4 x 3, shared by test_om_grid_host.py (CPU), test_om_grid.py (GPU)
and oracle/gen_golden_om_grid.py (the fixture recipe): the grid of settings, deterministic crowd builders and the margin
every crowd keeps from a cell boundary.

A map is a discrete function — a cell index is floor(r / cell_size + cell_num / 2) — so two correct implementations agree
on it exactly unless a coordinate sits within their arithmetic error (about 1e-15 in these coordinates: a few float64 ulps
of atan2 / cos / sin) of an integer.  cell_margin() measures that distance; the tests require it to be at least MARGIN."""
import numpy as np

# (cell_num, cell_size, om_channel_size); in_dim = 13 + cell_num^2 * channels
GRID = [
    (1, 2.0, 1),  # 14: one cell, one map column
    (1, 1.0, 3),  # 16: the row ends exactly at k-step 3
    (2, 1.0, 1),  # 17: first word of a second column tile
    (3, 0.5, 1),  # 22: odd cell_num (half-integer offset), odd width 9
    (2, 1.5, 3),  # 25: width 12
    (4, 1.0, 1),  # 29: the reference's other channel modes on the shipped grid
    (4, 1.0, 2),  # 45
    (3, 1.0, 3),  # 40: width 27, not a multiple of 4
    (5, 0.7, 3),  # 88: more than 64 columns, cell_size not a power of two
    (4, 1.0, 3),  # 61: control
]
FIXTURE_HUMANS = (2, 3, 5, 8, 12)
MARGIN = 1e-9  # six orders above the arithmetic error, three below the 2^-20 cells of the near-edge crowds
EDGE_EPS = 2.0 ** -20  # cells
STEP_DT = 0.25  # the env's time step (near_edge_crowds(shift=...): the constant-velocity lookahead moves every human by v dt)


def setting_id(setting):
    return '%dx%gx%d' % setting


def in_dim(setting):
    return 13 + setting[0] ** 2 * setting[2]


def cell_coordinates(states, cell_num, cell_size):
    """[H, H-1, 2] float64: (x, y) cell coordinate r / cell_size + cell_num / 2 of every other human j in human i's frame,
    with the expressions of MultiHumanRL.build_occupancy_maps."""
    hs = np.asarray(states, dtype=np.float64)
    out = np.zeros((len(hs), len(hs) - 1, 2))
    for i, me in enumerate(hs):
        others = np.delete(hs, i, axis=0)
        ox, oy = others[:, 0] - me[0], others[:, 1] - me[1]
        rot = np.arctan2(oy, ox) - np.arctan2(me[3], me[2])
        dist = np.linalg.norm([ox, oy], axis=0)
        out[i, :, 0] = np.cos(rot) * dist / cell_size + cell_num / 2
        out[i, :, 1] = np.sin(rot) * dist / cell_size + cell_num / 2
    return out


def cell_margin(states, cell_num, cell_size):
    """The smallest distance of any cell coordinate of the crowd from an integer."""
    c = cell_coordinates(states, cell_num, cell_size)
    return float(np.abs(c - np.round(c)).min())


class _Human(object):
    def __init__(self, row):
        self.px, self.py, self.vx, self.vy = (float(v) for v in row[:4])


def mirror_maps(states, setting):
    """crowdnav_amd.compat.sarl.occupancy_maps (the host mirror of the reference) of one crowd [H, 4+]: float32 [H, width]."""
    from crowdnav_amd.compat.sarl import occupancy_maps
    return occupancy_maps([_Human(r) for r in np.asarray(states, dtype=np.float64)], *setting).numpy()


def cells_of_maps(maps, setting):
    """Occupied cells per human from a map: bool [H, cells] (any channel of the cell non-zero)."""
    cell_num, _, ch = setting
    return (np.asarray(maps).reshape(len(maps), cell_num ** 2, ch) != 0).any(axis=2)


def _seed(setting, humans, salt):
    return 7919 * GRID.index(setting) + 101 * humans + salt


def random_crowd(setting, humans, salt=0):
    """[H, 4] float64 (px, py, vx, vy): positions uniform in +-0.75 cell_num cell_size (some inside, some outside the grid, some
    sharing a cell), velocities uniform in +-1, one human at rest (atan2(0, 0))."""
    cell_num, cell_size, _ = setting
    rs = np.random.RandomState(_seed(setting, humans, salt))
    half = 0.75 * cell_num * cell_size
    s = np.concatenate([rs.uniform(-half, half, (humans, 2)), rs.uniform(-1.0, 1.0, (humans, 2))], axis=1)
    s[rs.randint(humans), 2:] = 0.0
    return s


def near_edge_placements(setting):
    """Cell coordinates (x, y) in the viewer's frame, 2^-20 cells inside and outside each of the four grid edges and one interior
    cell line, along both axes; the other coordinate is generic and inside the grid.  List of (label, side, (cx, cy))."""
    cell_num = setting[0]
    lines = [('low', 0, -1), ('high', cell_num, 1)]  # (name, the line, the direction that leaves the grid)
    if cell_num > 1:
        lines.append(('line', 1 if cell_num < 4 else 2, 0))
    out = []
    for axis in (0, 1):
        for n, (name, line, outward) in enumerate(lines):
            for k, sign in enumerate((-1, 1)):
                side = 'below' if sign < 0 else 'above'
                if outward:
                    side = 'outside' if sign == outward else 'inside'
                c = [0.0, 0.0]
                c[axis] = line + sign * EDGE_EPS
                # generic, inside the grid, different for every placement (no two humans on top of each other)
                c[1 - axis] = cell_num * (0.139 + 0.113 * (2 * n + k) + 0.047 * axis)
                out.append(('xy'[axis] + '_' + name, side, tuple(c)))
    return out


VIEWER_VELOCITY = (0.6, 0.37)  # a generic heading


def near_edge_crowds(setting, humans, shift=0.0):
    """Crowds of `humans` whose human 0 (the viewer, generic heading, never at rest) sees the others at near_edge_placements, humans - 1
    at a time, the last crowd filled from the start of the list.  Returns (crowds [n, H, 4], labels: per crowd the (label, side)
    of humans 1..).  shift: every human stands at its place minus shift x its velocity, so that it is AT its place after a
    constant-velocity step of `shift` seconds."""
    cell_num, cell_size, _ = setting
    places = near_edge_placements(setting)
    rs = np.random.RandomState(_seed(setting, humans, 5))
    heading = np.arctan2(VIEWER_VELOCITY[1], VIEWER_VELOCITY[0])
    c, s = np.cos(heading), np.sin(heading)
    per = humans - 1
    crowds, labels = [], []
    for first in range(0, len(places), per):
        crowd = np.zeros((humans, 4))
        crowd[0] = (0.25, -0.5) + VIEWER_VELOCITY
        mine = []
        for j in range(per):
            label, side, (cx, cy) = places[(first + j) % len(places)]
            rx, ry = (cx - cell_num / 2) * cell_size, (cy - cell_num / 2) * cell_size
            crowd[1 + j, :2] = crowd[0, 0] + rx * c - ry * s, crowd[0, 1] + rx * s + ry * c
            crowd[1 + j, 2:] = rs.uniform(-1.0, 1.0, 2)
            mine.append((label, side))
        crowd[:, :2] -= shift * crowd[:, 2:]
        crowds.append(crowd)
        labels.append(mine)
    return np.array(crowds), labels


def exact_case(setting):
    """The one sub-case that is exact in every libm: the viewer moves along +x (rotation == 0, cos == 1, sin == 0), the others stand
    straight ahead at k cell_size with cell_size a power of two, so xi = floor(k + cell_num / 2) and yi = floor(cell_num / 2) with
    no rounding anywhere.  k = cell_num / 2 lands exactly on cell_num (outside), k = cell_num / 2 - 1 exactly on cell_num - 1
    (inside; only where that k is positive — never behind the viewer or on top of it: no cos(pi), no atan2(0, 0) for a
    position), k = 0.25 is interior.  Returns (states [H, 4], the viewer's occupied cells written out) or None where cell_size
    is no power of two."""
    cell_num, cell_size, _ = setting
    if np.frexp(cell_size)[0] != 0.5:
        return None
    ks = [0.25, cell_num / 2.0] + ([cell_num / 2.0 - 1.0] if cell_num / 2.0 - 1.0 > 0 else [])
    states = [[0.0, 0.0, 0.75, 0.0]] + [[k * cell_size, 0.0, -0.3 + 0.2 * n, 0.45] for n, k in enumerate(ks)]
    expected = {  # by hand, cell = cell_num yi + xi
        1: [0],       # yi = floor(0.5) = 0.   k = 0.25: xi = floor(0.75) = 0;  k = 0.5: xi = 1 = cell_num (outside)
        2: [3],       # yi = floor(1) = 1.     k = 0.25: xi = floor(1.25) = 1;  k = 1: xi = 2 = cell_num (outside)
        3: [4, 5],    # yi = floor(1.5) = 1.   k = 0.25: xi = 1;  k = 1.5: xi = 3 (outside);  k = 0.5: xi = floor(2.0) = 2 = cell_num - 1
        4: [10, 11],  # yi = floor(2) = 2.     k = 0.25: xi = 2;  k = 2: xi = 4 (outside);    k = 1: xi = floor(3.0) = 3 = cell_num - 1
    }
    return np.array(states), expected[cell_num]


def state8_of(crowd, robot=(-6.0, -7.0)):
    """[H + 1, 8] (px, py, vx, vy, gx, gy, radius, v_pref) for BatchedCrowdSim.set_state: a robot at rest well away from the crowd
    (the crowds reach 3.75 m from the origin at most: no collision ends an episode within a few steps),
    then the humans, each with its goal straight ahead (ORCA's preferred velocity keeps its heading; the human at rest is at its
    goal)."""
    crowd = np.asarray(crowd, dtype=np.float64)
    rows = [[robot[0], robot[1], 0.0, 0.0, -robot[0], -robot[1], 0.3, 1.0]]
    for px, py, vx, vy in crowd:
        rows.append([px, py, vx, vy, px + 4.0 * vx, py + 4.0 * vy, 0.3, 1.0])
    return np.array(rows)


def fixture_crowds():
    """The crowds of tests/golden/om_grid.npz, in order: (key, setting, states)."""
    for n, setting in enumerate(GRID):
        for humans in FIXTURE_HUMANS:
            yield 's%d_h%d_random' % (n, humans), setting, random_crowd(setting, humans)
        crowds, _ = near_edge_crowds(setting, 5)
        for k, crowd in enumerate(crowds):
            yield 's%d_h5_edge%d' % (n, k), setting, crowd
        exact = exact_case(setting)
        if exact is not None:
            yield 's%d_exact' % n, setting, exact[0]
