"""The jam scenes of tests/jam_scenes.py are what they claim to be — on the CPU, with the oracle alone (CrowdOracle.last_fallback:
per agent, whether linearProgram2 failed and linearProgram3 ran).  A workgroup of the fused rollout kernels serves the envs
(w E, .., w E + E - 1); with the 5-half-plane programs, 7 or more infeasible agents of a workgroup in one step take the multi-pass
branch of `fused_solve`.  These are conditions on the reference: they are the proof that test_fused_jam_parity.py reaches that
branch, the 6 / 7 boundary and both directions across it, with nothing added to the kernels to count it.

The oracle's counts (per case: one list per workgroup, one number per step):
    six            [6, 0, 0, 0, 0, 0, 0, 0]
    seven          [7, 2, 0, 0, 0, 0, 0, 0]
    two_five       [7, 5, 0, 0, 0, 0, 0, 0]
    all_ten        [10, 8, 0, 0, 0, 0, 0, 0]
    lattice_ten    [10, 10, 0, 0, 0, 0, 0, 0]
    half_empty     [10, 7, 0, ..] [5, 4, 0, ..]
    rising         [6, 8, 0, ..] [6, 7, 0, ..] [5, 7, 0, ..]
    mixed_batch    [0, 1, 2, 1, 1, 1, 1, 0] [6, 0, ..] [10, 10, 0, ..] [0, 0, 0, 0, 0, 1, 1, 0]
    h5_invisible   [10, 5, 0, ..] [5, 2, 0, ..]
    h4_visible     [8, 6, 0, ..] [4, 4, 0, ..]
    h3_visible_e3  [9, 0, ..] [3, 0, ..]
    h2_visible_e4  [8, 0, ..] [2, 0, ..]"""
import numpy as np
import pytest

import jam_scenes as js

ALL = ('six', 'seven', 'two_five', 'all_ten', 'lattice_ten', 'half_empty', 'rising', 'mixed_batch',
       'h5_invisible', 'h4_visible', 'h3_visible_e3', 'h2_visible_e4')


def test_every_case_is_present():
    assert tuple(js.CASES) == ALL and js.T == 8
    assert js.HEADLINE_CASES == ALL[:8] and js.OTHER_CASES == ALL[8:]
    for name in js.HEADLINE_CASES:
        cfg, epw, _ = js.scene(name)
        assert cfg == dict(num_humans=5, robot_visible=1) and epw == 2
    # (humans, robot visible, envs per workgroup) -> agents per workgroup
    want = {'h5_invisible': (5, 0, 2, 12), 'h4_visible': (4, 1, 2, 10), 'h3_visible_e3': (3, 1, 3, 12), 'h2_visible_e4': (2, 1, 4, 12)}
    for name, (H, visible, epw, agents) in want.items():
        cfg, e, st = js.scene(name)
        assert (cfg['num_humans'], cfg['robot_visible'], e, e * st.shape[1]) == (H, visible, epw, agents)


@pytest.mark.parametrize('name', ALL)
def test_scene_is_well_formed(name):
    cfg, epw, st = js.scene(name)
    B, A = st.shape[:2]
    assert st.dtype == np.float64 and st.shape == (B, cfg['num_humans'] + 1, 8) and 2 <= B <= 8
    assert (st[:, :, 6] == 0.3).all() and (st[:, :, 7] == 1.0).all()
    assert (st[:, 0, 2:4] == 0.0).all()  # the robot at rest
    gap = np.hypot(st[:, 1:, 0] - st[:, :1, 0], st[:, 1:, 1] - st[:, :1, 1])
    assert gap.min() >= 3.0  # ... at least 3 m from every human
    f = st.astype(np.float32)  # no two agents coincident, in the float32 view ORCA gets
    for b in range(B):
        pts = {(x, y) for x, y in f[b, :, 0:2].tolist()}
        assert len(pts) == A
    again = js.CASES[name][2]()  # deterministic
    assert np.array_equal(again, st)


@pytest.mark.parametrize('name', ALL)
def test_scene_does_what_it_is_for(oracle_mod, name):
    cfg, epw, st = js.scene(name)
    run = js.oracle_run(oracle_mod, name)
    assert run['fallback'].shape == (js.T, st.shape[0], st.shape[1])
    assert not run['done'].any()
    assert np.isfinite(run['states']).all() and np.isfinite(run['orca_vel']).all()
    assert not run['fallback'][:, :, 0].any()  # the robot is never in a jam
    c = run['counts']  # [T, workgroups]
    print(name, c.T.tolist())
    first, nxt = c[:-1], c[1:]
    falls = (first >= 7) & (nxt >= 1) & (nxt <= 6)
    rises = (first >= 1) & (first <= 6) & (nxt >= 7)
    if name == 'all_ten':
        assert c[0, 0] == 10 and (c[1:, 0] >= 7).any()
    elif name == 'six':
        assert c[0, 0] == 6 and c.max() == 6  # the last one-pass size, and never beyond it
    elif name == 'seven':
        assert c[0, 0] == 7
    elif name == 'two_five':
        assert run['fallback'][0].sum(axis=1).tolist() == [2, 5] and falls[:, 0].any()
    elif name == 'lattice_ten':
        assert c[0, 0] == 10
        # exact ties among an agent's float32 squared distances, as the rank of the pair phase sees them
        f = st.astype(np.float32)
        tied = 0
        for b in range(st.shape[0]):
            for q in range(1, st.shape[1]):
                d = [np.float32(np.float32((f[b, q, 0] - f[b, j, 0]) ** 2) + np.float32((f[b, q, 1] - f[b, j, 1]) ** 2))
                     for j in range(1, st.shape[1]) if j != q]
                tied += len(d) != len(set(d))
        assert tied >= 6
    elif name == 'half_empty':
        assert st.shape[0] == 3 and c.shape[1] == 2 and c[0].tolist() == [10, 5]
    elif name == 'rising':
        assert c.shape[1] >= 2 and rises.any(axis=0).all()  # every scene of the case rises
    elif name == 'mixed_batch':
        assert st.shape[0] == 8 and c[0].tolist() == [0, 6, 10, 0]
        assert (c[0] == 0).any() and ((c[0] >= 1) & (c[0] <= 6)).any() and (c[0] >= 7).any()
        assert not run['fallback'][0, 6:].any()  # a single "huddled" human is not infeasible
    else:
        table = {'h5_invisible': 10, 'h4_visible': 8, 'h3_visible_e3': 9, 'h2_visible_e4': 8}
        assert c[0, 0] == table[name]
        H = cfg['num_humans']
        assert run['fallback'][0, :, 1:].all() and c[0, -1] == H * (st.shape[0] - epw)  # the partial last workgroup
    # quiet steps after the jam are included
    assert (c[-1] <= 1).all()


def test_workgroup_counts():
    fb = np.zeros((2, 3, 4), dtype=bool)
    fb[0, 0, 1:] = True
    fb[0, 1, 2] = True
    fb[1, 2, 3] = True
    assert js.workgroup_counts(fb, 2).tolist() == [[4, 0], [0, 1]]
    assert js.workgroup_counts(fb, 3).tolist() == [[4], [1]]
    assert js.workgroup_counts(fb, 1).tolist() == [[3, 1, 0], [0, 0, 1]]


def test_last_fallback_leaves_the_step_alone(oracle_mod):
    """the new getter reads what the solve left: asking changes nothing, and a caller-supplied robot action reports no fallback"""
    cfg, _, st = js.scene('seven')
    B = st.shape[0]
    a = oracle_mod.CrowdOracle(num_envs=B, robot_policy=1, **cfg)
    b = oracle_mod.CrowdOracle(num_envs=B, robot_policy=1, **cfg)
    for o in (a, b):
        o.set_state(st, np.zeros(B))
    assert not a.last_fallback().any()  # nothing solved yet
    for _ in range(3):
        ra, rb = a.step(None, update=True), b.step(None, update=True)
        a.last_fallback()
        for k in ra:
            assert np.array_equal(ra[k], rb[k], equal_nan=True), k
    assert np.array_equal(a.get_state()[0], b.get_state()[0])
    ext = oracle_mod.CrowdOracle(num_envs=B, robot_policy=0, **cfg)
    ext.set_state(st, np.zeros(B))
    ext.step(np.zeros((B, 2)), update=False)
    fb = ext.last_fallback()
    assert fb.dtype == bool and not fb[:, 0].any() and fb[:, 1:].sum() == 7
    assert np.array_equal(ext.orca().shape, (B, st.shape[1], 2)) and ext.last_fallback()[:, 1:].sum() == 7
