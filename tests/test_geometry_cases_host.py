"""geometry_cases.py's table is what it says, without a GPU: every row survives pick_geometry's clamps, leaves a ragged last
workgroup, and — in the kernels over B K or B M virtual envs — packs branches of two source envs into one workgroup.  The clamps
are restated from crowdnav_amd/csrc/crowdnav_amd.hip (pick_geometry) and checked against its text, so that a change there is
noticed here."""
import os
import re

import pytest

from conftest import ROOT

import geometry_cases as cases
import predict_orca_cases

REQUIRED = {('h5', 2, 1, 0), ('h5', 3, 1, 0), ('h5', 4, 2, 0), ('h5_mixed', 2, 1, 0), ('h5', 2, 1, 1), ('h1', 7, 1, 0),
            ('h12', 2, 1, 0), ('h12', 4, 2, 0), ('h20', 3, 1, 0), ('h20', 1, 2, 0)}  # (crowd, E, W, unicycle)


def _source():
    return open(os.path.join(ROOT, 'crowdnav_amd', 'csrc', 'crowdnav_amd.hip')).read()


def test_the_table_holds_the_required_geometries_once_each():
    got = [(r['crowd'], r['E'], r['W'], int(r['cfg'].get('robot_kinematics', 0))) for r in cases.ROWS]
    assert len(got) == len(set(got)) and set(got) >= REQUIRED, sorted(REQUIRED - set(got))
    assert len(cases.NAMES) == len(set(cases.NAMES)) == len(cases.ROWS)
    assert set(cases.H5) <= set(cases.HOLONOMIC) < set(cases.NAMES)
    assert cases.CROWDS == predict_orca_cases.CROWDS  # the predictors' oracle tables are made for these crowds


def test_the_clamps_are_pick_geometrys():
    text = _source()
    body = text[text.index('static void pick_geometry'):text.index('static int rollout_route')]
    for line in ('const int e_max = cn::kWave / P.A;',
                 'P.E = e_want < 1 ? 1 : (e_want > e_max ? e_max : e_want);',
                 'const int w_useful = (P.E * P.A * P.NC + cn::kWave - 1) / cn::kWave;',
                 'if (w_want > w_useful) w_want = w_useful;',
                 'if (w_want > cn::kMaxBlock / cn::kWave) w_want = cn::kMaxBlock / cn::kWave;',
                 'P.threads = cn::kWave * (w_want < 1 ? 1 : w_want);'):
        assert line in body, line
    headers = ''.join(open(os.path.join(ROOT, 'crowdnav_amd', 'csrc', f)).read() for f in ('step_kernels.h', 'orca_device.h'))
    assert int(re.search(r'constexpr int kWave = (\d+);', headers).group(1)) == cases.WAVE
    assert int(re.search(r'constexpr int kMaxBlock = (\d+);', headers).group(1)) == cases.MAX_BLOCK
    # the restatement at the clamps' edges
    assert cases.clamped(6, 11, 1) == (10, 1) and cases.clamped(6, 0, 0) == (1, 1)       # E <= 64 / A; at least 1
    assert cases.clamped(6, 2, 2) == (2, 1) and cases.clamped(6, 3, 5) == (3, 2)         # W <= ceil(E A NC / 64)
    assert cases.clamped(64, 1, 99) == (1, 8)                                            # W <= kMaxBlock / 64


def test_the_defaults_give_one_env_on_one_wave_below_2049_envs():
    body = _source()
    assert 'small_lp ? (P.B > 2048 ? 2 : 1) : (P.B + 4095) / 4096' in body
    assert 'env_int("CROWDNAV_AMD_WAVES_PER_BLOCK", 1)' in body
    assert all(r['B'] <= 9 for r in cases.ROWS)  # so every twin at the default knobs is E = 1, W = 1


@pytest.mark.parametrize('name', cases.NAMES)
def test_the_row_survives_the_clamps(name):
    r = cases.BY_NAME[name]
    assert cases.clamped(cases.agents(r), r['E'], r['W']) == (r['E'], r['W'])


@pytest.mark.parametrize('name', cases.NAMES)
def test_the_last_workgroup_is_ragged(name):
    r = cases.BY_NAME[name]
    groups = cases.workgroups(r['B'], r['E'])
    assert len(groups) >= 2 and sum(len(g) for g in groups) == r['B'] <= 9
    assert groups[1][0] == r['E']  # ebase != 0
    if r['E'] == 1:  # no workgroup of one env can be partly empty: the row is there for its waves
        assert r['W'] >= 2
    else:
        assert 1 <= len(groups[-1]) < r['E'] and all(len(g) == r['E'] for g in groups[:-1])


@pytest.mark.parametrize('per_env', ['K', 'M'])
@pytest.mark.parametrize('name', cases.NAMES)
def test_a_workgroup_holds_branches_of_two_source_envs(name, per_env):
    r = cases.BY_NAME[name]
    n = r[per_env]
    assert n % 2 == 1 and 3 <= n <= 5
    if r['E'] == 1:
        return
    assert (r['B'] * n) % r['E'] != 0
    groups = cases.workgroups(r['B'] * n, r['E'])
    sources = [sorted({v // n for v in g}) for g in groups]
    assert 1 <= len(groups[-1]) < r['E']                       # ragged in virtual envs as well
    assert any(len(s) >= 2 for s in sources), sources          # two source envs side by side in one workgroup
    if r['E'] <= n:                                            # ... and, where they fit, two branches of one env
        assert any(len(s) == 1 and len(g) >= 2 for s, g in zip(sources, groups)), sources
    assert any(g[0] % n != 0 for g in groups)                  # a workgroup that starts in the middle of an env's branches


def test_the_table_is_ordered_smallest_launch_first():
    sizes = [cases.launch_size(r) for r in cases.ROWS]
    assert sizes == sorted(sizes), sizes
