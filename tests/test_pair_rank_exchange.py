"""The neighbour rank of the fused rollout kernels' pair phase — the agent's candidate distances fetched from the lanes of its
group (rollout_fused.h: fused_pair_body) — against the oracle, step for step, bit for bit, on the scenes of
tests/rank_scenes.py: exact distance ties of two and three neighbours, a neighbour exactly at / just beyond / just inside the
range, max_neighbors below the number in range (also cutting inside a tie), 1 / 2 / 3 envs (a half-empty workgroup: pairs that
do not exist), the robot invisible (a missing pair in every human's group) and 1-4 humans (fewer than five candidates).
test_rank_scenes_host.py proves on the CPU that the scenes contain these, and that the oracle's result depends on them.

Routes as in test_fused_jam_parity.py (each run asserts through rollout_route that it took the kernel it is named for): the
headline geometry runs generic / fused (one wave) / split / split_assist, the other geometries generic / fused.  Cuts of the
T = 4 steps: one step per call — after EVERY step the state, global_time and the running episode's accumulators (steps,
return: the rewards so far; Danger steps and their dmin sum: the infos so far; no episode finished: the dones so far) are the
oracle's — and one call.  Nothing but equality is accepted (the running return is a float64 sum held to the suite's 1e-9)."""
import numpy as np
import pytest

from jam_scenes import same_state as _same_state
import rank_scenes as rs
from support import amd, environ, np_of as _np  # noqa: F401  (amd: module fixture)

pytestmark = pytest.mark.gpu

T = rs.T
ROUTES = {
    'generic': (dict(CROWDNAV_AMD_FUSED=0, CROWDNAV_AMD_FUSED_SPLIT=None, CROWDNAV_AMD_SPLIT_ASSIST=None), 'generic'),
    'fused': (dict(CROWDNAV_AMD_FUSED=None, CROWDNAV_AMD_FUSED_SPLIT=0, CROWDNAV_AMD_SPLIT_ASSIST=None), 'fused'),
    'split': (dict(CROWDNAV_AMD_FUSED=None, CROWDNAV_AMD_FUSED_SPLIT=1, CROWDNAV_AMD_SPLIT_ASSIST=0), 'fused_split'),
    'split_assist': (dict(CROWDNAV_AMD_FUSED=None, CROWDNAV_AMD_FUSED_SPLIT=1, CROWDNAV_AMD_SPLIT_ASSIST=1), 'fused_split'),
}
CUTS = {'per_step': [1] * T, 'one_call': [T]}
RUNS = [(name, route, cut) for name in rs.CASES for route in (ROUTES if name in rs.HEADLINE_CASES else ('generic', 'fused'))
        for cut in CUTS]


def _same_book(amd, eng, bufs, want, steps, where):
    """the running episode after `steps` steps: rewards, infos and dones so far"""
    got = {k: _np(v) for k, v in bufs.items()}
    B = want['reward'].shape[1]
    assert (got['ep_count'] == 0).all() and (got['active'] == 1).all(), ('done', where, steps)
    assert (got['cur_steps'] == steps).all() and (got['env_transitions'] == steps).all(), ('steps', where, steps)
    dt, v_pref, gamma = eng.config['time_step'], eng.config['robot_v_pref'], 0.9
    ret, danger, dsum = np.zeros(B), np.zeros(B, dtype=np.int64), np.zeros(B)
    for t in range(steps):
        ret = ret + pow(gamma, t * dt * v_pref) * want['reward'][t]
        in_danger = want['info'][t] == amd.DANGER
        danger += in_danger
        dsum = np.where(in_danger, dsum + want['dmin'][t], dsum)
    assert np.abs(got['cur_return'] - ret).max() <= 1e-9, ('reward', where, steps)
    assert np.array_equal(got['cur_danger'], danger), ('info', where, steps)
    assert np.abs(got['cur_danger_dmin_sum'] - dsum).max() <= 1e-9, ('dmin', where, steps)


@pytest.mark.parametrize('name,route,cut', RUNS, ids=['%s-%s-%s' % r for r in RUNS])
def test_rollout_is_the_oracle_step_for_step(amd, oracle_mod, name, route, cut):
    want = rs.oracle_run(oracle_mod, name)
    cfg, epw, scene = rs.scene(name)
    B = scene.shape[0]
    switches, kernel = ROUTES[route]
    with environ(CROWDNAV_AMD_ENVS_PER_WAVE=epw, **switches):
        eng = amd.BatchedCrowdSim(num_envs=B, robot_policy=amd.ROBOT_ORCA, **cfg)
    assert eng.rollout_route(CUTS[cut][0]) == kernel
    bufs = eng.rollout_begin(seed_base=1000, seed_mod=500, episode_limit=-1, record_capacity=8, per_env_transitions=True)
    eng.set_state(np.array(scene), np.zeros(B))
    where = (name, route, cut)
    _same_state(eng, want, 0, where)
    done = 0
    for n in CUTS[cut]:
        eng.rollout(n)
        eng.sync()
        done += n
        _same_state(eng, want, done, where)
        _same_book(amd, eng, bufs, want, done, where)
    assert done == T
