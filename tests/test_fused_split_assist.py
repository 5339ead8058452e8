"""The env wave's assistance to the ORCA wave in the two-wave fused rollout kernel (`rollout_fused.h`: ASSIST, switched by
CROWDNAV_AMD_SPLIT_ASSIST when the engine is created) against the one-wave kernel: `cn_rollout` on two fresh engines with
the same seeds, one forced to the one-wave kernel (CROWDNAV_AMD_FUSED_SPLIT=0), and EVERY output compared bit for bit — the
state and global_time, every buffer of rollout_begin and rollout_summary().  The method is test_fused_split.py's.

Both values of the switch, i.e. both instantiations of the two-wave kernel: 1 (the default) — the head of the 3-D fallback runs on
the env wave for the agents that were infeasible one step ago, with a third workgroup barrier in exactly those iterations;
0 — the two-wave kernel without it, which test_fused_split.py no longer reaches now that 1 is the default.  A mistake in the rule
that decides which iterations have the third barrier hangs the workgroup, so these small shapes are what runs first; a mistake in what the env wave leaves in the fallback's scratch rows changes a velocity, and with
it everything after.

The geometry is the headline one: 5 humans, a visible ORCA robot, 2 envs per workgroup (CROWDNAV_AMD_ENVS_PER_WAVE=2)."""
import pytest

from support import amd, environ, same_tensors as _same  # noqa: F401  (amd: module fixture)

pytestmark = pytest.mark.gpu

ASSIST = (0, 1)


def _run(amd, assist, B, launches, ring_depth=None, **begin):
    """assist None: the one-wave kernel; else the two-wave kernel with CROWDNAV_AMD_SPLIT_ASSIST=assist"""
    split = assist is not None
    with environ(CROWDNAV_AMD_FUSED_SPLIT=1 if split else 0, CROWDNAV_AMD_SPLIT_ASSIST=assist, CROWDNAV_AMD_ENVS_PER_WAVE=2,
                 CROWDNAV_AMD_RING_DEPTH=ring_depth):
        eng = amd.BatchedCrowdSim(num_envs=B, num_humans=5, robot_policy=amd.ROBOT_ORCA, robot_visible=1, circle_radius=4.0)
    assert eng.rollout_route(launches[0]) == ('fused_split' if split else 'fused')
    begin.setdefault('episode_limit', -1)
    bufs = eng.rollout_begin(seed_base=1000, seed_mod=500, **begin)
    for n in launches:
        eng.rollout(n)
    eng.sync()
    state, gtime = eng.get_state()
    out = dict(bufs)
    out['state'], out['global_time'], out['rollout_summary'] = state, gtime, eng.rollout_summary()
    return out


CASES = {
    # a half-empty workgroup: its absent env must never post an end, never predict an agent
    'one_env': dict(B=1, launches=[160], record_capacity=8),
    'three_envs': dict(B=3, launches=[160], record_capacity=8, boundary_records=2),
    # jams on the 4 m circle: ~30 % of the wave-steps fall back, ~4 % are false alarms, ~7 % misses (CPU count), so hits, misses
    # and the third barrier in a step without fallback all occur; every env ends episodes inside the call
    'jams_ring_of_1': dict(B=64, launches=[160], record_capacity=1, per_env_transitions=True),
    # a ring of two scenarios runs dry: envs pause and resume; the redo path runs
    'ring_runs_dry': dict(B=64, launches=[120, 3, 120, 1, 2], ring_depth=2, record_capacity=8),
    # retirement at an episode's end
    'envs_retire': dict(B=64, launches=[40], episode_limit=64, record_capacity=8),
}

_wanted = {}


def _want(amd, name):
    """the one-wave kernel's result of a case: computed once, shared by the switch values"""
    if name not in _wanted:
        case = dict(CASES[name])
        _wanted[name] = _run(amd, None, case.pop('B'), case.pop('launches'), **case)
    return _wanted[name]


@pytest.mark.parametrize('assist', ASSIST)
@pytest.mark.parametrize('name', sorted(CASES))
def test_assisted_two_wave_kernel_is_bitwise_the_one_wave_kernel(amd, name, assist):
    case = dict(CASES[name])
    B, launches = case.pop('B'), case.pop('launches')
    want = _want(amd, name)
    got = _run(amd, assist, B, launches, **case)
    _same(got, want)
    # the case did what it is there for
    if name == 'ring_runs_dry':
        assert int(want['transitions'][0]) < B * sum(launches)  # some env paused
    elif name == 'envs_retire':
        assert int((want['active'] == 0).sum()) > 0 and int(want['ep_count'].max()) == 1
    else:
        assert int(want['ep_count'].min()) >= 2  # every env ended episodes inside the launch


@pytest.fixture(scope='module')
def one_call_64(amd):
    """64 envs x 120 steps in ONE call on the one-wave kernel: what every way of cutting the 120 steps must reproduce"""
    return _run(amd, None, 64, [120], record_capacity=8, per_env_transitions=True)


CUTS = {'one_call': [120], '120_calls': [1] * 120, '60_calls': [2] * 60, '3_4_5_108': [3, 4, 5, 108]}


@pytest.mark.parametrize('assist', ASSIST)
@pytest.mark.parametrize('cut', sorted(CUTS))
def test_prediction_word_across_call_boundaries(amd, one_call_64, cut, assist):
    """The prediction word starts empty in every call (its first step is at best a miss); episodes end on a call's last step."""
    assert sum(CUTS[cut]) == 120
    got = _run(amd, assist, 64, CUTS[cut], record_capacity=8, per_env_transitions=True)
    _same(got, one_call_64)
