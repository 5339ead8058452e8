"""Fresh starts of the two-wave fused rollout kernel: the first ORCA step of every ring scenario is solved when
its slot is filled (`ring_first_step_kernel`), and an episode that starts inside a launch adopts those velocities instead of
having the workgroup compute the step a second time.

Parity: `cn_rollout` on two fresh engines with the same seeds and the same calls, one of them the one-wave kernel
(CROWDNAV_AMD_FUSED_SPLIT=0), and EVERY output compared bit for bit — every buffer of rollout_begin, the state, the times and
rollout_summary() — in the headline geometry (5 humans, visible ORCA robot, CROWDNAV_AMD_ENVS_PER_WAVE=2).  The same device
functions produce the numbers on both paths, so nothing but exact equality is acceptable.  `fresh_starts()` shows that the path
under test ran at all: episode starts adopted, iterations redone.

Solved velocities: `ring_vel0` of a slot against `cn_orca` of an engine set to the slot's scenario, bit for bit."""
import numpy as np
import pytest

from support import amd, environ, same_tensors as _same  # noqa: F401  (amd: module fixture)

pytestmark = pytest.mark.gpu


def _engine(amd, split, B, ring_depth=None, lagged=None, assist=None):
    with environ(CROWDNAV_AMD_FUSED_SPLIT=1 if split else 0, CROWDNAV_AMD_ENVS_PER_WAVE=2, CROWDNAV_AMD_RING_DEPTH=ring_depth,
                 CROWDNAV_AMD_LAGGED_FILL=lagged, CROWDNAV_AMD_SPLIT_ASSIST=assist):
        eng = amd.BatchedCrowdSim(num_envs=B, num_humans=5, robot_policy=amd.ROBOT_ORCA, robot_visible=1, circle_radius=4.0)
    assert eng.rollout_route(1) == ('fused_split' if split else 'fused')
    return eng


def _run(amd, split, B, calls, ring_depth=None, lagged=None, assist=None, **begin):
    """calls: launch lengths, or callables on the engine (between launches).  Returns every output and, per launch,
    fresh_starts() behind it."""
    eng = _engine(amd, split, B, ring_depth, lagged, assist)
    begin.setdefault('episode_limit', -1)
    begin.setdefault('record_capacity', 8)
    bufs = eng.rollout_begin(seed_base=1000, seed_mod=500, **begin)
    counts = []
    for c in calls:
        if callable(c):
            c(eng)
        else:
            eng.rollout(c)
            counts.append(eng.fresh_starts())
    eng.sync()
    state, gtime = eng.get_state()
    out = dict(bufs)
    out['state'], out['global_time'], out['rollout_summary'] = state, gtime, eng.rollout_summary()
    return out, counts, eng.launch_counts()


def _both(amd, B, calls, **kw):
    want, _, _ = _run(amd, False, B, calls, **kw)
    got, counts, launches = _run(amd, True, B, calls, **kw)
    _same(got, want)
    return want, counts, launches


@pytest.fixture(scope='module')
def one_call_64(amd):
    """64 envs x 120 steps in ONE call on the one-wave kernel: what every way of cutting the 120 steps must reproduce"""
    return _run(amd, False, 64, [120], per_env_transitions=True)[0]


@pytest.mark.parametrize('B', [1, 3, 64])
def test_one_call_adopts(amd, B):
    """(a) half-empty workgroup, odd count, many workgroups: ~4 episode ends per env inside the one call"""
    want, counts, _ = _both(amd, B, [160], boundary_records=2 if B == 3 else 0)
    assert int(want['ep_count'].min()) >= 2
    assert counts[-1]['adopted'] > 0 and counts[-1]['kernels'] >= 1


def test_single_step_calls_never_adopt(amd, one_call_64):
    """(b) every episode end is a launch's last step: nothing to adopt, and the state stored is the scenario's own"""
    got, counts, _ = _run(amd, True, 64, [1] * 120, per_env_transitions=True)
    _same(got, one_call_64)
    assert counts[-1]['adopted'] == 0 and counts[-1]['redone'] == 0
    assert int(one_call_64['ep_count'].min()) >= 2


def test_cuts_on_both_sides_of_episode_ends(amd, one_call_64):
    """(c) launches whose ends fall before, on and behind the envs' episode ends"""
    got, counts, _ = _run(amd, True, 64, [7, 13, 41, 59], per_env_transitions=True)
    _same(got, one_call_64)
    assert counts[-1]['adopted'] > 0


def test_ring_runs_dry(amd):
    """(d) a ring of two scenarios runs dry inside a call: envs pause (not fresh: redone) and resume after the next fill"""
    launches = [120, 3, 120, 1, 2]
    want, counts, _ = _both(amd, 64, launches, ring_depth=2)
    assert int(want['transitions'][0]) < 64 * sum(launches)  # some env paused
    assert counts[-1]['redone'] > 0 and counts[-1]['adopted'] > 0


def test_envs_retire(amd):
    """(e) one episode per env: an env retires when its episode ends, most of them inside the launch"""
    want, counts, _ = _both(amd, 64, [40], episode_limit=64)
    assert int((want['active'] == 0).sum()) > 0 and int(want['ep_count'].max()) == 1
    assert counts[-1]['adopted'] == 0


@pytest.mark.parametrize('lagged', [0, 1])
def test_fill_in_front_and_beside(amd, lagged):
    """(f) the solving kernel in both fill positions: with the lagged fill the later fills run beside a launch"""
    # (2 or 4 slots per env: the ~7 episodes of an env come from several fills)
    want, counts, launches = _both(amd, 64, [50] * 6, ring_depth=2, lagged=lagged)
    assert (launches['lagged_fills'] > 0) == (lagged == 1)
    assert counts[-1]['adopted'] > counts[2]['adopted'] > 0
    assert counts[-1]['kernels'] >= 3


def test_robot_sim_changes_between_launches(amd):
    """(g) set_robot_sim with radii unlike the scenarios', later drop_robot_sim: the solved steps are forgotten, episodes start
    with a redone step until a later fill has solved slots under the new simulator"""
    radii = np.array([0.45, 0.5, 0.35, 0.4, 0.55, 0.6], np.float32)
    calls = [100, lambda e: e.set_robot_sim(radii, 0.8), 100, 100, 100, 100, lambda e: e.drop_robot_sim(), 100, 100, 100, 100, 100]
    _, counts, _ = _both(amd, 64, calls, ring_depth=2)
    adopted = [c['adopted'] for c in counts]
    redone = [c['redone'] for c in counts]
    assert adopted[0] > 0
    assert adopted[1] == adopted[0] and redone[1] > redone[0]  # behind set_robot_sim: nothing solved is left
    assert adopted[4] > adopted[1]                              # ... until later fills
    assert adopted[5] == adopted[4] and redone[5] > redone[4]  # behind drop_robot_sim
    assert adopted[9] > adopted[5]


def test_without_assist(amd):
    """(h) the two-wave kernel without the fallback head on the env wave"""
    _, counts, _ = _both(amd, 64, [160], assist=0)
    assert counts[-1]['adopted'] > 0


def test_solved_velocities_are_cn_orca(amd):
    """ring_vel0 of three slots of two envs == cn_orca of an engine whose state is the slot's scenario, with the same robot
    simulator (what the first launch captured: float32(radius + 0.01 + safety) of the env's first scenario, the robot's v_pref)"""
    import torch
    B = 64
    eng = _engine(amd, True, B)
    eng.rollout_begin(seed_base=1000, seed_mod=500)
    first, _ = eng.get_state()
    eng.rollout(1)  # the fill in front of it solves every slot
    eng.sync()
    assert eng.fresh_starts()['kernels'] == 1
    ref = _engine(amd, False, B)
    for env in (0, B - 1):
        start = first[env].cpu().numpy()
        ref.set_robot_sim(np.float32(start[:, 6] + 0.01 + 0.0), float(np.float32(start[0, 7])))
        for slot in (1, 2, 7):
            state8, vel0, ok = eng.ring_slot(env, slot)
            assert ok
            assert not np.array_equal(state8[:, :2], start[:, :2])  # another scenario than the env's first
            ref.set_state(torch.from_numpy(np.tile(state8, (B, 1, 1))))
            want = ref.orca().cpu().numpy()
            assert np.array_equal(vel0.view(np.uint32), want[env].view(np.uint32))
            assert np.abs(vel0).max() > 0.0
