"""ORACLE — TEST INFRASTRUCTURE ONLY.

Generates tests/golden/om_grid.npz with the UNMODIFIED reference: for every occupancy-map setting of tests/om_grid_cases.py
(cell_num, cell_size, om_channel_size other than the shipped 4 x 1 x 3 among them) and crowds of 2, 3, 5, 8 and 12 humans,
the human states (float64 [H, 4]: px, py, vx, vy) and what MultiHumanRL.build_occupancy_maps returns for them (float32
[H, cell_num^2 * om_channel_size]).  The crowds come from the builders of tests/om_grid_cases.py: random ones, humans 2^-20
cells either side of every grid edge, and the exact straight-ahead case.

    make -C oracle && PYTHONDONTWRITEBYTECODE=1 python oracle/gen_golden_om_grid.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import ref_harness as rh  # noqa: E402
import om_grid_cases as cases  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'om_grid.npz')


def reference_maps(states, setting):
    from crowd_nav.policy.policy_factory import policy_factory
    from crowd_sim.envs.utils.state import ObservableState
    cell_num, cell_size, channels = setting
    pcfg = rh.read_config('policy.config', {('sarl', 'with_om'): 'true', ('om', 'cell_num'): cell_num,
                                            ('om', 'cell_size'): cell_size, ('om', 'om_channel_size'): channels})
    policy = policy_factory['sarl']()
    policy.configure(pcfg)
    humans = [ObservableState(float(px), float(py), float(vx), float(vy), 0.3) for px, py, vx, vy in states]
    return policy.build_occupancy_maps(humans).numpy()


def generate():
    rh.activate()
    out = {}
    for key, setting, states in cases.fixture_crowds():
        maps = reference_maps(states, setting)
        assert maps.shape == (len(states), cases.in_dim(setting) - 13) and maps.dtype == np.float32
        out[key + '_states'] = np.asarray(states, dtype=np.float64)
        out[key + '_maps'] = maps
    # an .npz np.load reads, written member by member with a fixed date (np.savez stamps the time of day into the archive):
    # the same crowds give the same bytes
    import zipfile
    with zipfile.ZipFile(OUT, 'w') as z:
        for name, arr in out.items():
            info = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, 'w') as f:
                np.lib.format.write_array(f, np.ascontiguousarray(arr), allow_pickle=False)
    print(os.path.relpath(OUT, ROOT), len(out) // 2, 'crowds,', os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    assert rh.available()
    generate()
