"""The workgroup geometries the newer kernels are run at (test_workgroup_geometry.py, GPU) and the proof that each row is what
it says (test_geometry_cases_host.py, no GPU).

pick_geometry (crowdnav_amd/csrc/crowdnav_amd.hip) gives every kernel that shares the step kernel's workgroup E whole envs per
workgroup and W waves.  Its defaults are E = 1, W = 1 at every batch a test can afford (E = 2 only above 2048 envs of 5 humans),
so a small engine reaches the packed shapes through CROWDNAV_AMD_ENVS_PER_WAVE / CROWDNAV_AMD_WAVES_PER_BLOCK alone, and those are
clamped: E <= 64 / A, W <= ceil(E A NC / 64), W <= kMaxBlock / 64.  clamped() restates the three clamps.

A row: crowd (a key of CROWDS), the engine settings that go with it, (E, W), B, and K / M — the candidates per env of the
lookaheads and the modes per env of predict_orca_goals, whose kernels run over B K (B M) virtual envs, env v / K being the source
of virtual env v.  B leaves the last workgroup partly empty (E >= 2); K and M are odd and B K is no multiple of E, so some
workgroup holds branches of two source envs and the last one is ragged in virtual envs too.  K = M = 3, except at E = 3, where
every B K is a multiple of E: 5 there.  E = 1 (h20 at two waves) has no ragged workgroup; it is the multi-wave block_sync alone.

Ordered smallest launch first (pair items of one step over the batch, B A NC; then threads per workgroup), as jam_scenes.py
orders its scenes: if a geometry faults, the smallest one that does is met first."""
from support import environ

WAVE, MAX_BLOCK = 64, 512  # cn::kWave, cn::kMaxBlock

CROWDS = {'h1': dict(num_humans=1), 'h5': dict(num_humans=5), 'h12': dict(num_humans=12), 'h20': dict(num_humans=20),
          'h5_mixed': dict(num_humans=5, scenario_rule=2)}  # predict_orca_cases.CROWDS


def _row(crowd, E, W, B, K=3, M=3, **cfg):
    name = '%s%s_e%dw%d' % (crowd, '_unicycle' if cfg.get('robot_kinematics') else '', E, W)
    return dict(name=name, crowd=crowd, cfg=cfg, E=E, W=W, B=B, K=K, M=M)


ROWS = (
    _row('h1', 7, 1, B=9),
    _row('h5', 2, 1, B=7),  # the production geometry: every engine above 2048 envs of 5 humans
    _row('h5', 3, 1, B=7, K=5, M=5),
    _row('h5_mixed', 2, 1, B=7),
    _row('h5', 2, 1, B=7, robot_kinematics=1),
    _row('h5', 4, 2, B=7),
    _row('h12', 2, 1, B=7),
    _row('h12', 4, 2, B=7),
    _row('h20', 1, 2, B=3),
    _row('h20', 3, 1, B=7, K=5, M=5),
)
BY_NAME = {r['name']: r for r in ROWS}
NAMES = tuple(r['name'] for r in ROWS)
HOLONOMIC = tuple(r['name'] for r in ROWS if not r['cfg'].get('robot_kinematics'))
# the rows of the value-network decision and of the planners' closed loops: 5 humans, a holonomic robot on the 81 actions
H5 = ('h5_e2w1', 'h5_e3w1', 'h5_e4w2')


def agents(row):
    return CROWDS[row['crowd']]['num_humans'] + 1


def clamped(A, E, W):
    """(E, W) as pick_geometry leaves them for A agents per env."""
    NC = A - 1
    e_max = WAVE // A
    E = 1 if E < 1 else min(E, e_max)
    w_useful = (E * A * NC + WAVE - 1) // WAVE
    W = min(W, w_useful, MAX_BLOCK // WAVE)
    return E, max(W, 1)


def launch_size(row):
    """What the table is ordered by."""
    A = agents(row)
    return row['B'] * A * (A - 1), WAVE * row['W']


def workgroups(n_envs, E):
    """The envs (or virtual envs) of every workgroup of a launch over n_envs: lists of E, the last one shorter if ragged."""
    return [list(range(first, min(first + E, n_envs))) for first in range(0, n_envs, E)]


def engine_config(row, **more):
    """The keyword arguments of an engine of this row's crowd (without num_envs and robot_policy)."""
    return dict(CROWDS[row['crowd']], **dict(row['cfg'], **more))


def knobs(row):
    """The context in which cn_create reads this row's geometry."""
    return environ(CROWDNAV_AMD_ENVS_PER_WAVE=row['E'], CROWDNAV_AMD_WAVES_PER_BLOCK=row['W'])


def default_knobs():
    """... and the one in which it picks its own."""
    return environ(CROWDNAV_AMD_ENVS_PER_WAVE=None, CROWDNAV_AMD_WAVES_PER_BLOCK=None)


def assert_geometry(eng, row):
    """The engine got the (E, W) the row names, and the grid that follows from its B."""
    got = eng.geometry()
    want = dict(E=row['E'], threads=WAVE * row['W'], grid=len(workgroups(eng.B, row['E'])))
    assert {k: got[k] for k in want} == want and got['lds_bytes'] > 0, (row['name'], got, want)


def assert_default_geometry(eng):
    """A reference twin: one env per workgroup on one wave."""
    got = eng.geometry()
    assert (got['E'], got['threads'], got['grid']) == (1, WAVE, eng.B), got
