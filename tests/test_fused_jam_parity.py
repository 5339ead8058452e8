"""Step-for-step oracle parity of the rollout kernels in jams: `cn_rollout` from states the caller wrote (cn_set_state), on
every route that can take them, against `oracle.step` — bit for bit.

The scenes are tests/jam_scenes.py's: huddles in which 6, 7, 8, 9 or 10 agents of ONE workgroup have an infeasible planar
program in the same step, so that the multi-pass 3-D fallback of `fused_solve` (rollout_fused.h: more than six infeasible
agents of a workgroup) runs, next to workgroups that take the one-pass form or none; sequences in which the count falls from
>= 7 to 1..6 and rises from 1..6 to >= 7 between two steps of one call, the boundaries of the two-wave kernel's prediction-word
rule (split_has_head).  That the scenes do this is proved on the CPU by test_jam_scenes_host.py, whose docstring lists the counts.

Routes (each run asserts through rollout_route that it took the kernel it is named for):
    generic        CROWDNAV_AMD_FUSED=0                                  rollout_kernel
    fused          CROWDNAV_AMD_FUSED_SPLIT=0                            the one-wave fused kernel (headline geometry:
                                                                         rollout_fused_kernel<true>, the others <false>)
    split          two-wave kernel, CROWDNAV_AMD_SPLIT_ASSIST=0          (headline geometry only)
    split_assist   two-wave kernel, CROWDNAV_AMD_SPLIT_ASSIST=1          (headline geometry only)
Cuts of the T = 8 steps: one step per call (every call starts with an empty prediction word: the plain parity of every step),
one call (the only form in which the prediction word lives across steps), 3 + 5, and 1 + 7 (these jams last two steps: the
call boundary falls inside them, and the second call meets the jam's second step with an empty word).  After EVERY call the
state and global_time are the oracle's after as many steps.  A fifth leg runs the scenes through cn_step, the path the
suite already pins to the oracle step by step.

Both sides start from the same float64 state and the device's claim is bit identity with the float32 RVO2 restatement:
nothing but equality is accepted (the running return is a float64 sum held to the suite's 1e-9)."""
import numpy as np
import pytest

import jam_scenes as js
from jam_scenes import same_state as _same_state
from support import amd, environ, np_of as _np  # noqa: F401  (amd: module fixture)

pytestmark = pytest.mark.gpu

T = js.T
ROUTES = {
    'generic': (dict(CROWDNAV_AMD_FUSED=0, CROWDNAV_AMD_FUSED_SPLIT=None, CROWDNAV_AMD_SPLIT_ASSIST=None), 'generic'),
    'fused': (dict(CROWDNAV_AMD_FUSED=None, CROWDNAV_AMD_FUSED_SPLIT=0, CROWDNAV_AMD_SPLIT_ASSIST=None), 'fused'),
    'split': (dict(CROWDNAV_AMD_FUSED=None, CROWDNAV_AMD_FUSED_SPLIT=1, CROWDNAV_AMD_SPLIT_ASSIST=0), 'fused_split'),
    'split_assist': (dict(CROWDNAV_AMD_FUSED=None, CROWDNAV_AMD_FUSED_SPLIT=1, CROWDNAV_AMD_SPLIT_ASSIST=1), 'fused_split'),
}
CUTS = {'8_calls': [1] * T, 'one_call': [T], '3_plus_5': [3, T - 3], '1_plus_7': [1, T - 1]}
# the smallest launches first (jam_scenes.CASES is in that order): a wrong barrier rule hangs a workgroup
RUNS = [(name, route, cut) for name in js.CASES for route in (ROUTES if name in js.HEADLINE_CASES else ('generic', 'fused'))
        for cut in CUTS]


def _engine(amd, name, switches):
    cfg, epw, st = js.scene(name)
    with environ(CROWDNAV_AMD_ENVS_PER_WAVE=epw, **switches):
        return amd.BatchedCrowdSim(num_envs=st.shape[0], robot_policy=amd.ROBOT_ORCA, **cfg)


@pytest.mark.parametrize('name,route,cut', RUNS, ids=['%s-%s-%s' % r for r in RUNS])
def test_rollout_from_a_jam_is_the_oracle_step_for_step(amd, oracle_mod, name, route, cut):
    want = js.oracle_run(oracle_mod, name)
    _, _, scene = js.scene(name)
    B = scene.shape[0]
    switches, kernel = ROUTES[route]
    eng = _engine(amd, name, switches)
    assert eng.rollout_route(CUTS[cut][0]) == kernel
    bufs = eng.rollout_begin(seed_base=1000, seed_mod=500, episode_limit=-1, record_capacity=8, per_env_transitions=True)
    eng.set_state(scene, np.zeros(B))
    _same_state(eng, want, 0, (name, route, cut))
    done = 0
    for n in CUTS[cut]:
        eng.rollout(n)
        eng.sync()
        done += n
        _same_state(eng, want, done, (name, route, cut))
    assert done == T
    got = {k: _np(v) for k, v in bufs.items()}
    assert (got['ep_count'] == 0).all() and (got['active'] == 1).all()
    assert (got['cur_steps'] == T).all() and (got['env_transitions'] == T).all()
    # the running episode's accumulators (explorer.py:71: python's left-to-right sum)
    dt, v_pref, gamma = eng.config['time_step'], eng.config['robot_v_pref'], 0.9
    ret, danger, dsum = np.zeros(B), np.zeros(B, dtype=np.int64), np.zeros(B)
    for t in range(T):
        ret = ret + pow(gamma, t * dt * v_pref) * want['reward'][t]
        in_danger = want['info'][t] == amd.DANGER
        danger += in_danger
        dsum = np.where(in_danger, dsum + want['dmin'][t], dsum)
    assert np.abs(got['cur_return'] - ret).max() <= 1e-9
    assert np.array_equal(got['cur_danger'], danger)
    assert np.abs(got['cur_danger_dmin_sum'] - dsum).max() <= 1e-9


@pytest.mark.parametrize('name', list(js.CASES))
def test_cn_step_from_a_jam_is_the_oracle(amd, oracle_mod, name):
    """the same scenes through cn_step: ties the fixtures to the path test_free_running_soak_vs_oracle / test_kd_ties.py pin"""
    want = js.oracle_run(oracle_mod, name)
    _, _, scene = js.scene(name)
    B = scene.shape[0]
    eng = _engine(amd, name, {})
    eng.set_state(scene, np.zeros(B))
    for t in range(T):
        g = eng.step(None, update=True, want_obs=False)
        assert np.array_equal(_np(g['orca_vel']).view(np.uint32), want['orca_vel'][t].view(np.uint32)), t
        for k in ('reward', 'done', 'info', 'dmin'):
            assert np.array_equal(_np(g[k]), want[k][t]), (k, t)
        _same_state(eng, want, t + 1, (name, 'cn_step'))
