"""The neighbour-rank scenes of tests/rank_scenes.py contain what their names say — on the CPU.  The oracle exposes no neighbour
list, so the list is restated here (rank_scenes.neighbour_table: oracle/rvo2_oracle.cpp's offerNeighbor for a single-leaf
kd-tree) and tied to the oracle: the oracle's step must CHANGE when the setting that the scene is about changes — max_neighbors
raised to hold every neighbour, or by one across the cut inside the tie; neighbor_dist one float32 step wider (the neighbour at
exactly 2 m comes in) and one narrower (the neighbour just inside drops out) — so the ties, the range boundary and the
truncation are live in the reference's result, not only in the restated list.  test_pair_rank_exchange.py runs the same scenes
through every fused rollout route on the GPU."""
import numpy as np
import pytest

import rank_scenes as rs

F = np.float32


def _table(name, b=0):
    cfg, _, st = rs.scene(name)
    return rs.neighbour_table(st[b], cfg['robot_visible'], cfg.get('neighbor_dist', 10.0), cfg.get('max_neighbors', 10))


def _ties(row):
    """sizes of the groups of bit-equal distances among the neighbours in range"""
    d = [x.tobytes() for x, _ in row['offered']]
    return sorted(d.count(v) for v in set(d))


@pytest.mark.parametrize('name', list(rs.CASES))
def test_scene_is_well_formed(name):
    cfg, epw, st = rs.scene(name)
    B, A = st.shape[:2]
    assert st.shape == (B, cfg['num_humans'] + 1, 8) and 1 <= B <= 3 and epw == 2 and rs.T <= 8
    pos = st[:, :, 0:2]
    assert np.array_equal(pos.astype(F).astype(np.float64), pos)  # positions are float32 values: the view ORCA gets is exact
    assert (st[:, :, 6] == 0.3).all() and (st[:, :, 7] == 1.0).all() and (st[:, :, 2:4] == 0.0).all()
    for b in range(B):
        assert len({(x, y) for x, y in st[b, :, 0:2].tolist()}) == A  # no two agents coincident
    assert np.array_equal(rs.CASES[name][2](), st)  # deterministic


@pytest.mark.parametrize('name,human,groups', [('tie2_one_env', 1, 2), ('tie2', 1, 2), ('tie3_three_envs', 1, 3), ('invisible', 1, 3),
                                               ('h4', 1, 3), ('h3', 1, 2), ('keep3', 1, 2), ('keep2_cut_in_tie', 1, 3),
                                               ('h4_keep2_invisible', 1, 3)])
def test_tied_neighbours(name, human, groups):
    _, _, st = rs.scene(name)
    for b in range(st.shape[0]):  # every env: the shift between envs keeps the ties
        row = _table(name, b)[human]
        assert _ties(row)[-1] == groups, (name, b, row['offered'])
        tied = [(d, j) for d, j in row['offered'] if d == F(1.0)]
        assert len(tied) == groups
        # RVO2 keeps equals in the order they were offered: ascending id among the humans
        kept_ids = [j for d, j in row['kept'] if d == F(1.0)]
        assert kept_ids == [j for _, j in tied][:len(kept_ids)]


def test_cut_inside_a_tie():
    """max_neighbors = 2 and three neighbours at the same distance in front: two of the three are kept — the first two offered"""
    for name in ('keep2_cut_in_tie', 'h4_keep2_invisible'):
        for b in range(3):
            row = _table(name, b)[1]
            assert row['in_range'] > 2 and len(row['kept']) == 2
            assert [d for d, _ in row['kept']] == [F(1.0), F(1.0)] and [j for _, j in row['kept']] == [2, 3]
            assert (F(1.0), 4) in row['offered']


def test_truncation():
    for name, keep in (('keep3', 3), ('keep2_cut_in_tie', 2), ('h4_keep2_invisible', 2)):
        cfg, _, st = rs.scene(name)
        for b in range(st.shape[0]):
            for q, row in enumerate(_table(name, b)):
                assert len(row['kept']) == min(keep, row['in_range'])
                if cfg['robot_visible'] or q > 0:
                    assert row['in_range'] > keep, (name, b, q)


def test_range_boundary():
    for b in range(3):
        row = _table('range', b)[1]
        d = {j: x for x, j in row['offered']}
        assert d[2] == F(4.0) and d[3] > F(4.0) and d[4] < F(4.0)
        assert float(d[3]) - 4.0 < 2e-6 and 4.0 - float(d[4]) < 2e-6  # ulp-scale on either side
        assert [j for _, j in row['kept']] == [5, 4]  # exactly at the range is out (strict), just inside is in
        assert row['in_range'] == 2


def test_few_humans_have_fewer_than_five_candidates():
    for name, H in (('h4', 4), ('h3', 3), ('h2', 2), ('h1', 1)):
        cfg, _, st = rs.scene(name)
        assert st.shape == (3, H + 1, 8)
        assert all(len(row['offered']) == H for row in _table(name))
    assert all(len(row['offered']) == (5 if q == 0 else 4) for q, row in enumerate(_table('invisible')))


def _first_step(oracle_mod, name, **change):
    cfg, _, _ = rs.scene(name)
    return rs.oracle_run(oracle_mod, name, cfg=dict(cfg, **change), steps=1)['orca_vel'][0]


def test_the_oracle_depends_on_what_the_scenes_are_about(oracle_mod):
    # truncation is live: with room for every neighbour the reference decides otherwise
    # (from the second step on at the latest: the states are the same until the velocities first differ)
    for name in ('keep3', 'keep2_cut_in_tie', 'h4_keep2_invisible'):
        cfg, _, _ = rs.scene(name)
        roomy = rs.oracle_run(oracle_mod, name, cfg=dict(cfg, max_neighbors=10))['orca_vel']
        assert not np.array_equal(rs.oracle_run(oracle_mod, name)['orca_vel'][:2], roomy[:2]), name
    # the cut inside the tie is live: keeping the third tied neighbour as well changes human 1's velocity
    a, b = _first_step(oracle_mod, 'keep2_cut_in_tie'), _first_step(oracle_mod, 'keep2_cut_in_tie', max_neighbors=3)
    assert not np.array_equal(a[:, 1], b[:, 1])
    # the range boundary: one float32 step wider takes the neighbour at exactly 2 m in (human 1 changes) ...
    wider = float(np.nextafter(F(2.0), F(3.0)))
    a, b = _first_step(oracle_mod, 'range'), _first_step(oracle_mod, 'range', neighbor_dist=wider)
    assert not np.array_equal(a[:, 1], b[:, 1])
    # ... and one step narrower drops the neighbour just inside
    c = _first_step(oracle_mod, 'range', neighbor_dist=float(np.nextafter(F(2.0), F(0.0))))
    assert not np.array_equal(a[:, 1], c[:, 1])


@pytest.mark.parametrize('name', list(rs.CASES))
def test_oracle_run_is_finite_and_ends_no_episode(oracle_mod, name):
    run = rs.oracle_run(oracle_mod, name)
    assert np.isfinite(run['states']).all() and np.isfinite(run['orca_vel']).all()
    assert not run['done'].any()
    assert (np.abs(run['orca_vel'][0][:, 1:]).max(axis=2) > 0).all()  # every human moves from the first step
