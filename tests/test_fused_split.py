"""The two-wave fused rollout kernel (`rollout_fused.h`: rollout_fused_kernel<true, true>, an ORCA wave and an env wave per
workgroup) against the one-wave kernel it was split from: `cn_rollout` on two fresh engines with the same seeds, one with
CROWDNAV_AMD_FUSED_SPLIT=0, and EVERY output compared bit for bit — the state and global_time, every buffer of
rollout_begin (episode counters, the running episode's accumulators, the record rings, the transition counters, the
in-kernel summary / record blocks) and rollout_summary().  Both kernels run the same device functions for every number, so
nothing but exact equality is acceptable.

The geometry is always the headline one — 5 humans, a visible ORCA robot, 2 envs per workgroup (CROWDNAV_AMD_ENVS_PER_WAVE=2:
below 2049 envs the engine would otherwise put one env in a workgroup) — at the smallest sizes at which the split can go
wrong; every case asserts through rollout_route that the two engines really took different kernels.

Multi-pass 3-D fallback (more than six infeasible agents of a workgroup in one step): the seeded cases of this file never reach
it (they produce 1, 2 or 3 infeasible agents per step).  test_fused_jam_parity.py does, from the huddles of jam_scenes.py — 7 to 10
infeasible agents of a workgroup, on the one-wave and both two-wave kernels, step for step against the oracle — and
test_jam_scenes_host.py proves on the oracle that those scenes reach it."""
import pytest

from support import amd, environ, same_tensors as _same  # noqa: F401  (amd: module fixture)

pytestmark = pytest.mark.gpu


def _run(amd, split, B, launches, ring_depth=None, radius=4.0, **begin):
    with environ(CROWDNAV_AMD_FUSED_SPLIT=1 if split else 0, CROWDNAV_AMD_ENVS_PER_WAVE=2, CROWDNAV_AMD_RING_DEPTH=ring_depth):
        eng = amd.BatchedCrowdSim(num_envs=B, num_humans=5, robot_policy=amd.ROBOT_ORCA, robot_visible=1, circle_radius=radius)
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


@pytest.fixture(scope='module')
def one_call_64(amd):
    """64 envs x 120 steps in ONE call on the one-wave kernel: what every way of cutting the 120 steps must reproduce"""
    return _run(amd, False, 64, [120], record_capacity=8, per_env_transitions=True)


CASES = {
    # half-empty workgroup (its second env does not exist); ~4 episode ends, each one a discarded and redone ORCA step
    'one_env': dict(B=1, launches=[160], record_capacity=8),
    # odd count: the last workgroup half-empty beside a full one; the in-kernel summary and record blocks
    'three_envs': dict(B=3, launches=[160], record_capacity=8, boundary_records=2),
    # jams on the 4 m circle: some waves take the 3-D fallback (one-pass form); record ring of 1 and of 4 slots (wraps)
    'jams_ring_of_1': dict(B=64, launches=[160], record_capacity=1, per_env_transitions=True),
    'jams_ring_of_4': dict(B=64, launches=[160], record_capacity=4),
    # a ring of two scenarios runs dry inside a 120-step call (~4 episodes): envs pause (kWaitingScenario), resume after the
    # next call's fill, and the two ring slots are re-used many times
    'ring_runs_dry': dict(B=64, launches=[120, 3, 120, 1, 2], ring_depth=2, record_capacity=8),
    # one episode per env: an env retires (io.active = 0) as soon as its episode ends, most of them inside the launch
    'envs_retire': dict(B=64, launches=[40], episode_limit=64, record_capacity=8),
}


@pytest.mark.parametrize('name', sorted(CASES))
def test_two_wave_kernel_is_bitwise_the_one_wave_kernel(amd, name):
    case = dict(CASES[name])
    B, launches = case.pop('B'), case.pop('launches')
    want = _run(amd, False, B, launches, **case)
    got = _run(amd, True, B, launches, **case)
    _same(got, want)
    # the case did what it is there for
    if name == 'ring_runs_dry':
        assert int(want['transitions'][0]) < B * sum(launches)  # some env paused
    elif name == 'envs_retire':
        assert int((want['active'] == 0).sum()) > 0 and int(want['ep_count'].max()) == 1
    else:
        assert int(want['ep_count'].min()) >= 2  # every env ended episodes inside the launch


@pytest.mark.parametrize('launches', [[120], [7, 113], [1] * 120], ids=['one_call', '7_plus_113', '120_calls'])
def test_carried_state_survives_every_way_of_cutting_the_calls(amd, one_call_64, launches):
    """The prologue / epilogue round trip of everything an env carries from call to call — with one-step calls every episode
    end is an episode that ends on a call's last step."""
    got = _run(amd, True, 64, launches, record_capacity=8, per_env_transitions=True)
    _same(got, one_call_64)
