"""Occupancy maps at settings other than the shipped 4 x 4 x 3, CPU side: the host mirror (compat.sarl.occupancy_maps) against
what the unmodified reference's build_occupancy_maps returned for the same crowds (tests/golden/om_grid.npz, recipe
oracle/gen_golden_om_grid.py), and the properties of the crowds test_om_grid.py puts on the device (om_grid_cases.py)."""
import numpy as np
import pytest

import om_grid_cases as cases
from conftest import load_golden

IDS = [cases.setting_id(s) for s in cases.GRID]


def test_the_grid_reaches_the_widths_it_is_chosen_for():
    assert [cases.in_dim(s) for s in cases.GRID] == [14, 16, 17, 22, 25, 29, 45, 40, 88, 61]
    assert {s[2] for s in cases.GRID} == {1, 2, 3}
    assert sum((cases.in_dim(s) - 13) % 4 != 0 for s in cases.GRID) >= 4  # map rows that do not start 16-byte aligned


def test_host_mirror_equals_the_reference_fixture_bit_for_bit():
    g = load_golden('om_grid.npz')
    seen = 0
    for key, setting, states in cases.fixture_crowds():
        assert np.array_equal(g[key + '_states'], states), key  # the builders are deterministic
        got = cases.mirror_maps(g[key + '_states'], setting)
        want = g[key + '_maps']
        assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, key
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), key
        seen += 1
    assert 2 * seen == len(g)
    # the fixture is not trivially empty: every setting has occupied and free cells somewhere
    for n, setting in enumerate(cases.GRID):
        maps = np.concatenate([g['s%d_h%d_random_maps' % (n, h)].ravel() for h in cases.FIXTURE_HUMANS])
        assert (maps != 0).any() and (maps == 0).any(), setting


@pytest.mark.parametrize('setting', cases.GRID, ids=IDS)
def test_no_crowd_sits_on_a_cell_boundary(setting):
    cell_num, cell_size, _ = setting
    for humans in (2, 3, 5, 8, 9, 12):
        for salt in range(3):
            crowd = cases.random_crowd(setting, humans, salt)
            assert cases.cell_margin(crowd, cell_num, cell_size) >= cases.MARGIN, (humans, salt)
            assert (np.abs(crowd[:, 2:]).sum(axis=1) == 0).sum() == 1  # one human at rest
            if humans >= 5 and cell_num > 1:  # some inside, some outside
                cells = cases.cells_of_maps(cases.mirror_maps(crowd, setting), setting)
                coords = cases.cell_coordinates(crowd, cell_num, cell_size)
                inside = ((coords >= 0) & (coords < cell_num)).all(axis=2)
                assert cells.any() and inside.any()
        for shift in (0.0, cases.STEP_DT):
            crowds, _ = cases.near_edge_crowds(setting, humans, shift)
            for crowd in crowds:
                moved = crowd.copy()
                moved[:, :2] += shift * crowd[:, 2:]
                margin = cases.cell_margin(moved, cell_num, cell_size)
                assert cases.MARGIN <= margin <= 1.01 * cases.EDGE_EPS, (humans, shift, margin)
                assert np.abs(crowd[0, 2:]).min() > 0  # the viewer is never at rest


@pytest.mark.parametrize('setting', cases.GRID, ids=IDS)
def test_near_edge_crowds_put_humans_on_both_sides_of_every_edge(setting):
    """Counted from the mirror's output: the viewer's map holds exactly the humans placed inside, in the cells their placement
    names, and none of those placed outside."""
    cell_num, cell_size, channels = setting
    places = {(label, side): c for label, side, c in cases.near_edge_placements(setting)}
    want_labels = {(a + '_' + n, s) for a in 'xy' for n in ('low', 'high') for s in ('inside', 'outside')}
    if cell_num > 1:
        want_labels |= {(a + '_line', s) for a in 'xy' for s in ('below', 'above')}
    assert set(places) == want_labels
    for humans in (2, 3, 5, 8, 12):
        crowds, labels = cases.near_edge_crowds(setting, humans)
        seen = set()
        for crowd, mine in zip(crowds, labels):
            viewer = cases.cells_of_maps(cases.mirror_maps(crowd, setting), setting)[0]
            expect = np.zeros(cell_num ** 2, dtype=bool)
            for label, side in mine:
                cx, cy = places[(label, side)]
                xi, yi = int(np.floor(cx)), int(np.floor(cy))
                if side != 'outside':
                    assert 0 <= xi < cell_num and 0 <= yi < cell_num
                    expect[cell_num * yi + xi] = True
                else:
                    assert not (0 <= xi < cell_num and 0 <= yi < cell_num)
                seen.add((label, side))
            # (channels == 2 holds velocities alone: a cell shows unless its mean velocity is exactly zero — never, here)
            assert np.array_equal(viewer, expect), (humans, mine)
        assert seen == want_labels, humans
    # the two humans at an interior line fall into DIFFERENT cells
    if cell_num > 1:
        for axis in 'xy':
            below, above = places[(axis + '_line', 'below')], places[(axis + '_line', 'above')]
            assert np.floor(below).tolist() != np.floor(above).tolist()


@pytest.mark.parametrize('setting', cases.GRID, ids=IDS)
def test_exact_case_lands_on_the_last_cell_and_just_outside(setting):
    cell_num, cell_size, _ = setting
    exact = cases.exact_case(setting)
    if exact is None:
        assert setting == (5, 0.7, 3) or setting == (2, 1.5, 3)  # cell_size is no power of two
        return
    states, cells = exact
    coords = cases.cell_coordinates(states, cell_num, cell_size)[0]  # the viewer's frame: exact arithmetic
    assert float(cell_num) in coords[:, 0].tolist()
    if cell_num >= 3:
        assert float(cell_num - 1) in coords[:, 0].tolist()
    assert np.all(coords[:, 1] == cell_num / 2)
    viewer = cases.cells_of_maps(cases.mirror_maps(states, setting), setting)[0]
    assert np.nonzero(viewer)[0].tolist() == cells


def test_policy_configuration_carries_the_om_section():
    import crowdnav_amd.compat as c
    from crowdnav_amd.compat.sarl import default_policy_config
    for name in ('sarl', 'lstm_rl'):
        for cell_num, cell_size, channels in cases.GRID:
            policy = c.policy_factory[name]()
            policy.configure(default_policy_config({('om', 'cell_num'): cell_num, ('om', 'cell_size'): cell_size,
                                                    ('om', 'om_channel_size'): channels, (name, 'with_om'): 'true'}))
            policy.build_action_space(1.0)
            kw = policy.engine_kwargs()
            assert (kw['with_om'], kw['cell_num'], kw['cell_size'], kw['om_channel_size']) == (True, cell_num, cell_size, channels)
            assert policy.input_dim() == 13 + cell_num ** 2 * channels
            first = policy.get_model().mlp1[0] if name == 'sarl' else policy.get_model().lstm
            assert (first.in_features if name == 'sarl' else first.input_size) == policy.input_dim()
            states = cases.random_crowd((cell_num, cell_size, channels), 3)
            got = policy.build_occupancy_maps([cases._Human(r) for r in states]).numpy()
            assert np.array_equal(got, cases.mirror_maps(states, (cell_num, cell_size, channels)))
