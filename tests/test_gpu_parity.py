"""Parity of the HIP path (through the C ABI) against the CPU oracle and the reference-generated fixtures.
Bar (BASELINE.json north_star): reward / done / info bit-exact, positions / velocities within 1e-5 — the
ORCA velocities and the float64 env arithmetic are in fact required to be bit-identical here; only scenario
generation (device cos/sin vs numpy's) is compared with a tolerance (1e-12)."""
import numpy as np
import pytest

from conftest import TRAJ_FIXTURES, episodes_of, flat_steps, load_golden
from support import amd, np_of as _np  # noqa: F401  (amd: module fixture)

pytestmark = pytest.mark.gpu


def test_mt19937_matches_numpy_stream(amd):
    g = load_golden('resets.npz')
    eng = amd.BatchedCrowdSim(num_envs=1)
    for s in (0, 1000, 2000, 4294965295):
        assert np.array_equal(_np(eng.mt_random(s, 700)), g['mt_random_%d' % s])


@pytest.mark.parametrize('name', sorted(TRAJ_FIXTURES))
def test_orca_velocities_bit_exact_vs_oracle(amd, oracle_mod, name):
    """K1 alone, teacher-forced on every state of the fixture: all agents, robot included."""
    g = load_golden(name)
    before, _, gtime = flat_steps(g)
    cfg = TRAJ_FIXTURES[name]
    eng = amd.BatchedCrowdSim(num_envs=len(before), robot_policy=amd.ROBOT_ORCA, **cfg)
    eng.set_state(before, gtime)
    got = _np(eng.orca())
    o = oracle_mod.CrowdOracle(num_envs=len(before), robot_policy=1, **cfg)
    o.set_state(before, gtime)
    want = o.orca()
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize('update', [True, False])
@pytest.mark.parametrize('name', sorted(TRAJ_FIXTURES))
def test_step_bit_exact_vs_golden_and_oracle(amd, oracle_mod, name, update):
    g = load_golden(name)
    before, after, gtime = flat_steps(g)
    cfg = TRAJ_FIXTURES[name]
    eng = amd.BatchedCrowdSim(num_envs=len(before), robot_policy=amd.ROBOT_ORCA, **cfg)
    eng.set_state(before, gtime)
    out = {k: (None if v is None else _np(v)) for k, v in eng.step(None, update=update).items()}
    state, gt = (_np(x) for x in eng.get_state())
    # vs the unmodified reference (fixtures)
    assert np.array_equal(out['reward'], g['rewards'])
    assert np.array_equal(out['done'], g['dones'])
    assert np.array_equal(out['info'], g['infos'])
    assert np.array_equal(out['action'], g['actions'])
    danger = g['infos'] == 1
    assert np.array_equal(out['dmin'][danger], g['dmins'][danger])
    if update:
        assert np.array_equal(state, after)
        assert np.array_equal(gt, gtime + 0.25)
        assert np.array_equal(out['obs'], after[:, 1:, [0, 1, 2, 3, 6]])
    else:
        assert np.array_equal(state, before) and np.array_equal(gt, gtime)
        assert np.array_equal(out['obs'], after[:, 1:, [0, 1, 2, 3, 6]])  # next observable states
    # vs the oracle, every field
    o = oracle_mod.CrowdOracle(num_envs=len(before), robot_policy=1, **cfg)
    o.set_state(before, gtime)
    want = o.step(None, update=update)
    assert np.array_equal(out['dmin'], want['dmin'])
    assert np.array_equal(out['orca_vel'].view(np.uint32), want['orca_vel'].view(np.uint32))


def test_external_action_step_vs_oracle(amd, oracle_mod):
    """CN_ROBOT_EXTERNAL (the path an RL robot policy uses): float64 actions supplied by the caller."""
    g = load_golden('traj_visible_h5.npz')
    before, _, gtime = flat_steps(g)
    n = len(before)
    rng = np.random.RandomState(7)
    action = rng.uniform(-1, 1, size=(n, 2))
    action[::7] = 0.0
    cfg = dict(num_humans=5, robot_visible=1)
    eng = amd.BatchedCrowdSim(num_envs=n, robot_policy=amd.ROBOT_EXTERNAL, **cfg)
    o = oracle_mod.CrowdOracle(num_envs=n, robot_policy=0, **cfg)
    for update in (False, True):
        eng.set_state(before, gtime)
        o.set_state(before, gtime)
        got = {k: _np(v) for k, v in eng.step(action, update=update).items()}
        want = o.step(action, update=update)
        for k in ('reward', 'done', 'info', 'dmin', 'action'):
            assert np.array_equal(got[k], want[k]), k
        assert np.array_equal(got['orca_vel'][:, 1:].view(np.uint32), want['orca_vel'][:, 1:].view(np.uint32))
        assert np.array_equal(_np(eng.get_state()[0]), o.get_state()[0])


@pytest.mark.parametrize('name', ['traj_invisible_h5.npz', 'traj_visible_h5.npz', 'traj_visible_h5_square.npz',
                                  'traj_visible_h10.npz', 'traj_visible_h20.npz', 'traj_debug_case.npz'])
def test_free_running_trajectories_vs_reference(amd, name):
    """Whole episodes from the fixture's initial states, no teacher forcing: step-for-step identical."""
    g = load_golden(name)
    eps = episodes_of(g)
    B = len(eps)
    T = max(len(e['actions']) for e in eps)
    eng = amd.BatchedCrowdSim(num_envs=B, robot_policy=amd.ROBOT_ORCA, **TRAJ_FIXTURES[name])
    eng.set_state(np.stack([e['states'][0] for e in eps]), np.zeros(B))
    for t in range(T):
        out = {k: _np(v) for k, v in eng.step(None, update=True, want_obs=False).items() if v is not None}
        state = _np(eng.get_state()[0])
        for b, e in enumerate(eps):
            if t < len(e['actions']):
                assert out['reward'][b] == e['rewards'][t] and out['done'][b] == e['dones'][t]
                assert out['info'][b] == e['infos'][t]
                assert np.abs(state[b] - e['states'][t + 1]).max() <= 1e-5
                assert np.array_equal(state[b], e['states'][t + 1])


RESET_SPECS = {
    'test_h5': dict(num_humans=5), 'train_h5': dict(num_humans=5), 'val_h5': dict(num_humans=5),
    'test_h5_random': dict(num_humans=5, randomize_attributes=1),
    'test_h5_square': dict(num_humans=5, scenario_rule=1),
    'test_h10': dict(num_humans=10), 'test_h20': dict(num_humans=20),
}


@pytest.mark.parametrize('name', sorted(RESET_SPECS))
def test_reset_vs_reference_generator(amd, oracle_mod, name):
    g = load_golden('resets.npz')
    want, seeds = g[name + '_states'], g[name + '_seeds']
    eng = amd.BatchedCrowdSim(num_envs=len(seeds), **RESET_SPECS[name])
    draws = _np(eng.reset(seeds))
    got, gt = (_np(x) for x in eng.get_state())
    assert np.all(gt == 0.0)
    assert np.abs(got - want).max() <= 1e-12
    assert np.array_equal(got[:, :, 6:], want[:, :, 6:]) and np.array_equal(got[:, 0], want[:, 0])
    o = oracle_mod.CrowdOracle(num_envs=len(seeds), **RESET_SPECS[name])
    assert np.array_equal(draws.astype(np.uint64), o.reset(seeds))  # same number of rejection attempts


def test_reset_mask_and_max_seed(amd):
    eng = amd.BatchedCrowdSim(num_envs=4)
    eng.reset([1000, 1001, 4294967295, 0])
    s0 = _np(eng.get_state()[0]).copy()
    eng.reset([5, 5, 5, 5], mask=[0, 1, 0, 1])
    s1 = _np(eng.get_state()[0])
    assert np.array_equal(s1[[0, 2]], s0[[0, 2]]) and np.array_equal(s1[1], s1[3])
    assert not np.array_equal(s1[1], s0[1])


def _records(bufs, k):
    return {name: _np(bufs[name])[:, :k] for name in ('ep_outcome', 'ep_steps', 'ep_return', 'ep_time',
                                                     'ep_danger', 'ep_danger_dmin_sum')}


@pytest.mark.parametrize('visible', [0, 1])
def test_rollout_500_test_cases_vs_reference(amd, visible):
    """Explorer.run_k_episodes(500, 'test') in one fused launch: per-case outcome, length, nav time and
    discounted return vs the unmodified reference (outcomes_500.npz); aggregate 213/284/3, 15 190 steps."""
    g = load_golden('outcomes_500.npz')
    tag = 'visible' if visible else 'invisible'
    eng = amd.BatchedCrowdSim(num_envs=500, robot_policy=amd.ROBOT_ORCA, robot_visible=visible)
    bufs = eng.rollout_begin(seed_base=1000, seed_mod=500, episode_limit=500, record_capacity=2)
    eng.rollout(100)
    eng.sync()
    rec = _records(bufs, 1)
    assert np.all(_np(bufs['ep_count']) == 1) and np.all(_np(bufs['active']) == 0)
    assert int(_np(bufs['transitions'])[0]) == int(g[tag + '_steps'].sum())
    assert np.array_equal(rec['ep_outcome'][:, 0], g[tag + '_info'])
    assert np.array_equal(rec['ep_steps'][:, 0], g[tag + '_steps'])
    assert np.allclose(rec['ep_return'][:, 0], g[tag + '_return'], rtol=0, atol=1e-9)
    timeout = g[tag + '_info'] == 4
    assert np.array_equal(rec['ep_time'][:, 0], np.where(timeout, 25.0, g[tag + '_steps'] * 0.25))


def test_rollout_vs_oracle_with_auto_reset(amd, oracle_mod):
    """64 envs x 150 transitions with in-kernel auto-reset, chunked launches, vs the oracle's rollout."""
    B, K = 64, 16
    eng = amd.BatchedCrowdSim(num_envs=B, robot_policy=amd.ROBOT_ORCA, robot_visible=1)
    bufs = eng.rollout_begin(seed_base=1000, seed_mod=500, episode_limit=-1, record_capacity=K)
    for n in (1, 49, 100):
        eng.rollout(n)
    eng.sync()
    o = oracle_mod.CrowdOracle(num_envs=B, robot_policy=1, robot_visible=1)
    o.reset(1000 + np.arange(B))
    ep_index, cur_steps, cur_ret = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.float64)
    total, rec = o.rollout(150, 1000, 500, K, ep_index, cur_steps, cur_ret)
    assert int(_np(bufs['transitions'])[0]) == total == B * 150
    cnt = _np(bufs['ep_count'])
    assert np.array_equal(cnt, rec['count'])
    got = _records(bufs, K)
    for b in range(B):
        k = cnt[b]
        assert np.array_equal(got['ep_outcome'][b, :k], rec['outcome'][b, :k])
        assert np.array_equal(got['ep_steps'][b, :k], rec['steps'][b, :k])
        assert np.allclose(got['ep_return'][b, :k], rec['ret'][b, :k], rtol=0, atol=1e-9)
    assert np.array_equal(_np(bufs['cur_steps']), cur_steps)
    assert np.abs(_np(eng.get_state()[0]) - o.get_state()[0]).max() <= 1e-9


def test_full_size_properties_4096x5(amd):
    """BASELINE config 2 size: determinism, sharding invariance and physical invariants."""
    B = 4096
    cfg = dict(robot_policy=amd.ROBOT_ORCA, robot_visible=1)

    def run(num_envs, offset):
        eng = amd.BatchedCrowdSim(num_envs=num_envs, **cfg)
        bufs = eng.rollout_begin(seed_base=2000, seed_mod=2 ** 32 - 2000, record_capacity=8,
                                 env_offset=offset, env_stride=B)
        eng.rollout(64)
        eng.sync()
        return _np(eng.get_state()[0]), {k: _np(v) for k, v in bufs.items()}

    s_full, b_full = run(B, 0)
    s_again, b_again = run(B, 0)
    assert np.array_equal(s_full, s_again)  # bitwise deterministic
    for k in b_full:
        assert np.array_equal(b_full[k], b_again[k]), k
    s_lo, b_lo = run(B // 2, 0)
    s_hi, b_hi = run(B // 2, B // 2)
    assert np.array_equal(np.concatenate([s_lo, s_hi]), s_full)  # sharding the env axis changes nothing
    for k in ('ep_count', 'ep_steps', 'ep_return', 'ep_outcome'):
        assert np.array_equal(np.concatenate([b_lo[k], b_hi[k]]), b_full[k]), k
    assert int(b_full['transitions'][0]) == B * 64
    speed = np.hypot(s_full[:, :, 2], s_full[:, :, 3])
    assert speed.max() <= 1.0 + 1e-4  # |v| <= maxSpeed (v_pref = 1)
    assert np.all(np.isfinite(s_full))
    done_eps = b_full['ep_count'].sum()
    assert done_eps > B // 2  # auto-reset happened (visible-robot episodes last ~40 steps)
    k = np.minimum(b_full['ep_count'], 8)
    outcomes = np.concatenate([b_full['ep_outcome'][b, :k[b]] for b in range(B)])
    assert set(np.unique(outcomes).tolist()) <= {2, 3, 4}


def test_lone_agent_and_head_on_symmetry(amd):
    """RVO2 known answers: a lone agent takes its (clipped) preferred velocity; the
    hand-derived 2-agent case gives (0.138, 0)."""
    eng = amd.BatchedCrowdSim(num_envs=2, num_humans=1, robot_policy=amd.ROBOT_ORCA, robot_visible=0)
    st = np.zeros((2, 2, 8))
    st[:, :, 6], st[:, :, 7] = 0.3, 1.0
    st[0, 0, :2], st[0, 0, 4:6] = (50, 50), (53, 54)       # robot far away: goal offset (3, 4)
    st[0, 1, :2], st[0, 1, 4:6] = (0, 0), (3, 4)           # lone human (robot invisible)
    st[1, 0, :2], st[1, 0, 4:6] = (0, 0), (10, 0)          # robot at origin heading +x ...
    st[1, 1, :2], st[1, 1, 4:6] = (2, 0), (2, 0)           # ... human 2 m ahead, at rest
    eng.set_state(st, np.zeros(2))
    v = _np(eng.orca())
    assert v[0, 1].tolist() == [np.float32(0.6000000238418579), np.float32(0.800000011920929)]
    assert v[1, 0].view(np.uint32).tolist() == [0x3e0d4fdf, 0]


def test_config4_shard_size_4096x20(amd, oracle_mod):
    """BASELINE configs[3] per-GPU shard (4096 envs x 20 humans): the oracle runs RVO2's kd-tree (21 agents > leaf
    size 10) while the kernel ranks brute force — identical up to exact distance ties.  A wider circle keeps the
    reference's rejection sampling cheap (at radius 4 it needs ~28 k draws per scenario)."""
    cfg = dict(num_humans=20, robot_policy=amd.ROBOT_ORCA, robot_visible=1, circle_radius=12.0)
    B = 4096

    def run(num_envs, offset):
        eng = amd.BatchedCrowdSim(num_envs=num_envs, **cfg)
        bufs = eng.rollout_begin(seed_base=2000, seed_mod=2 ** 32 - 2000, record_capacity=2, env_offset=offset,
                                 env_stride=B)
        eng.rollout(40)
        eng.sync()
        return _np(eng.get_state()[0]), {k: _np(v) for k, v in bufs.items()}

    s_full, b_full = run(B, 0)
    assert int(b_full['transitions'][0]) == B * 40 and np.all(np.isfinite(s_full))
    s_lo, _ = run(B // 2, 0)
    s_hi, _ = run(B // 2, B // 2)
    assert np.array_equal(np.concatenate([s_lo, s_hi]), s_full)
    # (no |v| <= maxSpeed property here: in crowded 21-agent sims the restated RVO2 fallback program itself returns
    # speeds slightly above maxSpeed, identically in the oracle)
    # first 48 envs step for step against the oracle (same seeds 2000 + env id)
    n = 48
    o = oracle_mod.CrowdOracle(num_envs=n, robot_policy=1, num_humans=20, robot_visible=1, circle_radius=12.0)
    o.reset(2000 + np.arange(n))
    eng = amd.BatchedCrowdSim(num_envs=n, **cfg)
    eng.set_state(o.get_state()[0], np.zeros(n))
    for _ in range(40):
        got = eng.step(None, update=True, want_obs=False)
        want = o.step(None, update=True)
        assert np.array_equal(_np(got['orca_vel']).view(np.uint32), want['orca_vel'].view(np.uint32))
        assert np.array_equal(_np(got['reward']), want['reward']) and np.array_equal(_np(got['info']), want['info'])
    assert np.array_equal(_np(eng.get_state()[0]), o.get_state()[0])
    still = b_full['ep_count'][:n] == 0  # envs still in their first episode: device-generated scenario vs oracle
    assert still.sum() >= n // 2 and np.abs(s_full[:n][still] - o.get_state()[0][still]).max() <= 1e-9


def test_config4_reference_geometry_20_humans_on_the_4m_circle(amd, oracle_mod):
    """BASELINE configs[3] at the reference's own geometry (env.config: 20 humans on the circle of radius 4, where the
    rejection sampling needs 28 k draws per scenario on average and 0.8 M for the worst of these seeds): the seeded
    reset (wave-cooperative generator) against the oracle's plain MT19937 — same draw counts, positions 1e-12 —, then the
    dense 21-agent crowd step for step (bit-identical velocities, rewards, states; the 10-half-plane programs and their
    3-D fallback are busy from the first step), then the fused rollout with auto-reset from the scenario ring."""
    n = 64
    cfg = dict(num_humans=20, robot_visible=1, circle_radius=4.0)
    seeds = 1000 + np.arange(n)  # the 'test' phase seeds (crowd_sim.py:272-276)
    o = oracle_mod.CrowdOracle(num_envs=n, robot_policy=1, **cfg)
    want_draws = o.reset(seeds)
    eng = amd.BatchedCrowdSim(num_envs=n, robot_policy=amd.ROBOT_ORCA, **cfg)
    draws = _np(eng.reset(seeds))
    assert np.array_equal(draws.astype(np.uint64), want_draws) and want_draws.max() > 100000
    s0 = o.get_state()[0]
    assert np.abs(_np(eng.get_state()[0]) - s0).max() <= 1e-12
    eng.set_state(s0, np.zeros(n))
    for t in range(100):
        got = eng.step(None, update=True, want_obs=False)
        want = o.step(None, update=True)
        assert np.array_equal(_np(got['orca_vel']).view(np.uint32), want['orca_vel'].view(np.uint32)), t
        for k in ('reward', 'done', 'info', 'dmin'):
            assert np.array_equal(_np(got[k]), want[k]), (k, t)
    assert np.array_equal(_np(eng.get_state()[0]), o.get_state()[0])
    # fused rollout with in-kernel auto-reset: 16 envs x 120 steps, episodes of ~15-40 steps end and restart from the ring
    m, K = 16, 12
    eng2 = amd.BatchedCrowdSim(num_envs=m, robot_policy=amd.ROBOT_ORCA, **cfg)
    bufs = eng2.rollout_begin(seed_base=1000, seed_mod=500, episode_limit=-1, record_capacity=K)
    for k in (30, 30, 60):
        eng2.rollout(k)
    eng2.sync()
    o2 = oracle_mod.CrowdOracle(num_envs=m, robot_policy=1, **cfg)
    o2.reset(1000 + np.arange(m))
    ep_index, cur_steps, cur_ret = np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros(m, np.float64)
    total, rec = o2.rollout(120, 1000, 500, K, ep_index, cur_steps, cur_ret)
    assert int(_np(bufs['transitions'])[0]) == total == m * 120
    cnt = _np(bufs['ep_count'])
    assert np.array_equal(cnt, rec['count']) and cnt.sum() >= m
    for b in range(m):
        k = min(cnt[b], K)
        assert np.array_equal(_np(bufs['ep_outcome'])[b, :k], rec['outcome'][b, :k])
        assert np.array_equal(_np(bufs['ep_steps'])[b, :k], rec['steps'][b, :k])
    assert np.abs(_np(eng2.get_state()[0]) - o2.get_state()[0]).max() <= 1e-9


@pytest.fixture
def wave_scenarios(monkeypatch):
    """Force the wave-per-scenario generators (default only for H > 8) so that they are checked on every fixture."""
    monkeypatch.setenv('CROWDNAV_AMD_WAVE_SCENARIOS', '1')


@pytest.mark.parametrize('name', sorted(RESET_SPECS))
def test_wave_cooperative_reset_vs_reference_generator(amd, oracle_mod, wave_scenarios, name):
    g = load_golden('resets.npz')
    want, seeds = g[name + '_states'], g[name + '_seeds']
    eng = amd.BatchedCrowdSim(num_envs=len(seeds), **RESET_SPECS[name])
    draws = _np(eng.reset(seeds))
    got, gt = (_np(x) for x in eng.get_state())
    assert np.all(gt == 0.0) and np.abs(got - want).max() <= 1e-12
    assert np.array_equal(got[:, :, 6:], want[:, :, 6:]) and np.array_equal(got[:, 0], want[:, 0])
    o = oracle_mod.CrowdOracle(num_envs=len(seeds), **RESET_SPECS[name])
    assert np.array_equal(draws.astype(np.uint64), o.reset(seeds))  # identical stream consumption


def test_wave_cooperative_equals_lane_generators_in_rollouts(amd, wave_scenarios, monkeypatch):
    """Same fused rollout with both generator families (ring fill + begin): bit-identical states and records."""
    def run():
        eng = amd.BatchedCrowdSim(num_envs=96, robot_policy=amd.ROBOT_ORCA, robot_visible=1, randomize_attributes=1)
        bufs = eng.rollout_begin(seed_base=2000, seed_mod=2 ** 32 - 2000, record_capacity=8)
        eng.rollout(120)
        eng.sync()
        return _np(eng.get_state()[0]), {k: _np(v) for k, v in bufs.items()}
    s_wave, b_wave = run()
    monkeypatch.setenv('CROWDNAV_AMD_WAVE_SCENARIOS', '0')
    s_lane, b_lane = run()
    assert np.array_equal(s_wave, s_lane)
    for k in b_wave:
        assert np.array_equal(b_wave[k], b_lane[k]), k
    assert b_wave['ep_count'].sum() > 96


@pytest.mark.parametrize('humans', [6, 12])
def test_unsatisfiable_scenario_is_reported_not_hung(amd, monkeypatch, humans):
    """A circle too small for the crowd makes the reference's rejection sampling loop forever; the engine gives up
    after a bounded number of attempts and reports it at the next sync (both generator families)."""
    monkeypatch.setenv('CROWDNAV_AMD_MAX_ATTEMPTS_LOG2', '10')
    eng = amd.BatchedCrowdSim(num_envs=8, num_humans=humans, circle_radius=0.3)
    with pytest.raises(amd.CrowdNavAmdError) as ei:
        eng.reset(1000 + np.arange(8))
    assert 'rejected placements' in str(ei.value)
    eng.sync()  # the flag is cleared once reported
    assert np.all(np.isfinite(_np(eng.get_state()[0])))


@pytest.mark.parametrize('cap_log2', [6, 8])
def test_window_generator_give_up_keeps_the_sequential_stream(amd, monkeypatch, cap_log2):
    """when a human exhausts its attempts in the window path (scenario_wave.h, CN_GEN_WINDOW), the give-up rule
    takes attempt N - 64 and the stream continues at attempt N - 63 — up to 62 attempts BEHIND the window base when the human
    started mid-window, i.e. at words the 1248-word ring may have overwritten (WaveRng::rewind_to regenerates the stream then).
    With a cap of 64 / 256 attempts on the reference's own crowded geometry (20 humans, 4 m circle) nearly every scenario
    gives up several times: placements, the number of random() calls consumed and the env's numpy stream BEHIND the scenario
    (what cn_sarl_explore draws from: mt_key / mt_pos) must be those of the plain sequential loop."""
    import ctypes as C
    import torch
    from generator_window_emulation import attempts_of, sequential
    monkeypatch.setenv('CROWDNAV_AMD_MAX_ATTEMPTS_LOG2', str(cap_log2))
    B, H, R, K = 64, 20, 4.0, 81
    eng = amd.BatchedCrowdSim(num_envs=B, num_humans=H, circle_radius=R, robot_policy=amd.ROBOT_EXTERNAL, robot_visible=1)
    eng.sarl_configure(actions=np.stack([np.arange(K), -np.arange(K)], axis=1).astype(np.float64))
    seeds = 1000 + 7 * np.arange(B)
    sd = torch.from_numpy(seeds.astype(np.uint32).view(np.int32)).to(eng.device)
    draws = torch.zeros(B, dtype=torch.int64, device=eng.device)
    from crowdnav_amd._lib import check
    check(eng._lib.cn_reset(eng._h, C.c_void_p(sd.data_ptr()), None, C.c_void_p(draws.data_ptr())))
    with pytest.raises(amd.CrowdNavAmdError) as ei:  # the give-ups are reported (once) at the next sync
        eng.sync()
    assert 'rejected placements' in str(ei.value)
    state, draws = _np(eng.get_state()[0]), _np(draws)
    gave_up = 0
    cap = 1 << cap_log2
    for b in range(B):
        placed, attempts, err = sequential(attempts_of(int(seeds[b]), H * (cap + 64)), H, R, 1.0, 0.8, cap)
        gave_up += int(err)
        assert draws[b] == 3 * attempts, (b, draws[b], 3 * attempts)
        want = np.array([(x, y, gx, gy) for x, y, gx, gy in placed])
        assert np.abs(state[b, 1:, [0, 1, 4, 5]].T - want).max() <= 1e-12, b
    assert gave_up >= B // 2
    # the env's own stream continues right behind the scenario's last draw
    sel = dict(best=torch.full((B,), 5, dtype=torch.int32, device=eng.device),
               action=torch.zeros(B, 2, dtype=torch.float64, device=eng.device))
    eng.sarl_explore(sel, 1.0)
    eng.sync()
    got = _np(sel['best'])
    for b in range(B):
        rs = np.random.RandomState(int(seeds[b]))
        rs.random_sample(int(draws[b]))
        assert rs.random_sample() < 1.0 and got[b] == int(rs.choice(K)), b


def test_head_generator_overflow_falls_back_exactly(amd, oracle_mod):
    """Lane-per-scenario generation tries a register-only generator good for 113 random() calls and regenerates
    with the memory-backed one beyond that: a crowded circle (8 humans, radius 2.6) needs both; stream-exact."""
    cfg = dict(num_humans=8, circle_radius=2.6)
    seeds = 3000 + np.arange(256)
    eng = amd.BatchedCrowdSim(num_envs=256, **cfg)
    draws = _np(eng.reset(seeds))
    o = oracle_mod.CrowdOracle(num_envs=256, **cfg)
    want_draws = o.reset(seeds)
    assert np.array_equal(draws.astype(np.uint64), want_draws)
    assert (want_draws > 113).sum() >= 3 and (want_draws <= 113).sum() >= 3  # both paths taken
    assert np.abs(_np(eng.get_state()[0]) - o.get_state()[0]).max() <= 1e-12


@pytest.mark.parametrize('humans,radius', [(1, 4.0), (63, 40.0)])
def test_minimum_and_maximum_crowd_sizes(amd, oracle_mod, humans, radius):
    """H = 1 (one candidate neighbour) and H = 63 (64 agents fill the wave; 4032 ordered pairs, 10 of 63 candidates
    kept): ORCA velocities and transitions bit-identical to the oracle (which walks RVO2's kd-tree at 64 agents)."""
    n = 6
    cfg = dict(num_humans=humans, robot_visible=1, circle_radius=radius)
    o = oracle_mod.CrowdOracle(num_envs=n, robot_policy=1, **cfg)
    o.reset(1000 + np.arange(n))
    eng = amd.BatchedCrowdSim(num_envs=n, robot_policy=amd.ROBOT_ORCA, **cfg)
    eng.set_state(o.get_state()[0], np.zeros(n))
    for _ in range(12):
        got = eng.step(None, update=True, want_obs=False)
        want = o.step(None, update=True)
        assert np.array_equal(_np(got['orca_vel']).view(np.uint32), want['orca_vel'].view(np.uint32))
        assert np.array_equal(_np(got['reward']), want['reward']) and np.array_equal(_np(got['done']), want['done'])
    assert np.array_equal(_np(eng.get_state()[0]), o.get_state()[0])


@pytest.mark.parametrize('envs_per_wave,waves', [(2, 1), (3, 1), (4, 2), (10, 5)])  # (2, 1) = the HEADLINE instantiation
def test_ragged_last_workgroup_and_geometry_knobs(amd, oracle_mod, monkeypatch, envs_per_wave, waves):
    """B not a multiple of the envs per workgroup (last workgroup partly empty) and multi-wave workgroups: the
    geometry is a pure performance knob — results identical to the oracle whatever it is."""
    monkeypatch.setenv('CROWDNAV_AMD_ENVS_PER_WAVE', str(envs_per_wave))
    monkeypatch.setenv('CROWDNAV_AMD_WAVES_PER_BLOCK', str(waves))
    n = 23
    cfg = dict(num_humans=5, robot_visible=1)
    eng = amd.BatchedCrowdSim(num_envs=n, robot_policy=amd.ROBOT_ORCA, **cfg)
    bufs = eng.rollout_begin(seed_base=1000, seed_mod=500, record_capacity=8)
    eng.rollout(90)
    eng.sync()
    o = oracle_mod.CrowdOracle(num_envs=n, robot_policy=1, **cfg)
    o.reset(1000 + np.arange(n))
    total, rec = o.rollout(90, 1000, 500, 8, np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.float64))
    assert int(_np(bufs['transitions'])[0]) == total == n * 90
    assert np.array_equal(_np(bufs['ep_count']), rec['count'])
    k = int(rec['count'].max())
    assert np.array_equal(_np(bufs['ep_outcome'])[:, :k] * (np.arange(k)[None] < rec['count'][:, None]),
                          rec['outcome'][:, :k] * (np.arange(k)[None] < rec['count'][:, None]))
    assert np.abs(_np(eng.get_state()[0]) - o.get_state()[0]).max() <= 1e-9


@pytest.mark.parametrize('seed', range(8))
def test_randomised_configurations_vs_oracle(amd, oracle_mod, seed):
    """Configuration fuzz: time step, limits, rewards, radii, preferred speeds, safety spaces, ORCA horizon /
    neighbour parameters, visibility, crowd size, attribute randomisation, both scenario rules — 48 envs stepped
    40 times with device-side ORCA robot, every output bit-identical to the oracle."""
    rng = np.random.RandomState(100 + seed)
    cfg = dict(
        num_humans=int(rng.choice([2, 3, 5, 7, 9, 12])), robot_visible=int(rng.rand() < 0.5),
        time_step=float(rng.choice([0.1, 0.2, 0.25, 0.5])), time_limit=float(rng.choice([6.0, 10.0, 25.0])),
        success_reward=float(rng.uniform(0.5, 2.0)), collision_penalty=float(-rng.uniform(0.1, 1.0)),
        discomfort_dist=float(rng.uniform(0.1, 0.4)), discomfort_penalty_factor=float(rng.uniform(0.2, 1.0)),
        robot_safety_space=float(rng.choice([0.0, 0.15])), human_safety_space=float(rng.choice([0.0, 0.05])),
        neighbor_dist=float(rng.choice([3.0, 10.0])), max_neighbors=int(rng.choice([3, 10])),
        time_horizon=float(rng.choice([2.0, 5.0])), circle_radius=float(rng.uniform(4.0, 7.0)),
        square_width=float(rng.uniform(10.0, 14.0)), scenario_rule=int(rng.rand() < 0.3),
        human_radius=float(rng.uniform(0.2, 0.4)), human_v_pref=float(rng.uniform(0.6, 1.4)),
        robot_radius=float(rng.uniform(0.2, 0.4)), robot_v_pref=float(rng.uniform(0.6, 1.4)),
        randomize_attributes=int(rng.rand() < 0.4))
    n = 48
    o = oracle_mod.CrowdOracle(num_envs=n, robot_policy=1, **cfg)
    o.reset(7000 + np.arange(n))
    eng = amd.BatchedCrowdSim(num_envs=n, robot_policy=amd.ROBOT_ORCA, **cfg)
    eng.set_state(o.get_state()[0], np.zeros(n))
    for _ in range(40):
        got = eng.step(None, update=True, want_obs=False)
        want = o.step(None, update=True)
        assert np.array_equal(_np(got['orca_vel']).view(np.uint32), want['orca_vel'].view(np.uint32))
        for k in ('reward', 'done', 'info', 'dmin', 'action'):
            assert np.array_equal(_np(got[k]), want[k]), (k, cfg)
    s, g = (_np(x) for x in eng.get_state())
    assert np.array_equal(s, o.get_state()[0]) and np.array_equal(g, o.get_state()[1])


def test_unicycle_robot_vs_reference_and_oracle(amd, oracle_mod):
    """ActionRot kinematics through cn_step (crowd_sim.py:339-341, agent.py:115-135): transitions of the unmodified
    reference driven by a unicycle SARL policy; device cos/sin vs numpy's: 1e-12, done/info exact; then 30 free-running
    steps against the oracle with random (v, r) actions."""
    g = load_golden('sarl_unicycle.npz')
    n = len(g['states'])
    cfg = dict(num_humans=5, robot_visible=1, robot_kinematics=amd.UNICYCLE)
    eng = amd.BatchedCrowdSim(num_envs=n, robot_policy=amd.ROBOT_EXTERNAL, **cfg)
    eng.set_state(g['states'], g['gtime'])
    eng.set_theta(g['theta'])
    out = {k: _np(v) for k, v in eng.step(g['action'], update=True, want_obs=False).items() if v is not None}
    assert np.array_equal(out['done'], g['step_done']) and np.array_equal(out['info'], g['step_info'])
    assert np.abs(out['reward'] - g['step_reward']).max() <= 1e-12
    assert np.array_equal(out['action'], g['action'])  # reported as given: (v, r)
    state = _np(eng.get_state()[0])
    assert np.abs(state - g['next_states']).max() <= 1e-12
    assert np.array_equal(state[:, 1:], g['next_states'][:, 1:])
    assert np.abs(_np(eng.get_theta()) - g['next_theta']).max() <= 1e-12

    o = oracle_mod.CrowdOracle(num_envs=n, robot_policy=0, robot_visible=1, robot_kinematics=1)
    o.set_state(g['states'], g['gtime'])
    o.set_theta(g['theta'])
    eng.set_state(g['states'], g['gtime'])
    eng.set_theta(g['theta'])
    rng = np.random.RandomState(5)
    for _ in range(30):
        act = np.stack([rng.uniform(0, 1, n), rng.uniform(-np.pi / 4, np.pi / 4, n)], axis=1)
        got = eng.step(act, update=True, want_obs=False)
        want = o.step(act, update=True)
        assert np.array_equal(_np(got['done']), want['done']) and np.array_equal(_np(got['info']), want['info'])
        assert np.abs(_np(got['reward']) - want['reward']).max() <= 1e-9
    assert np.abs(_np(eng.get_state()[0]) - o.get_state()[0]).max() <= 1e-9
    assert np.abs(_np(eng.get_theta()) - o.get_theta()).max() <= 1e-9


def test_rollout_step_with_external_actions_vs_oracle(amd, oracle_mod):
    """cn_rollout_step: the bookkept transition for a robot policy outside the engine.  Random actions, 70 steps,
    auto-reset from the scenario ring (refilled every ring_depth / 2 calls), vs the oracle stepped and reset by hand."""
    n, cfg = 40, dict(num_humans=5, robot_visible=1)
    eng = amd.BatchedCrowdSim(num_envs=n, robot_policy=amd.ROBOT_EXTERNAL, **cfg)
    bufs = eng.rollout_begin(seed_base=1000, seed_mod=500, record_capacity=8)
    o = oracle_mod.CrowdOracle(num_envs=n, robot_policy=0, **cfg)
    o.reset(1000 + np.arange(n))
    ep = np.zeros(n, np.int64)
    steps = np.zeros(n, np.int64)
    rec_steps, rec_outcome = [[] for _ in range(n)], [[] for _ in range(n)]
    rng = np.random.RandomState(11)
    import torch
    for _ in range(70):
        act = rng.uniform(-0.8, 0.8, size=(n, 2))
        eng.rollout_step(torch.from_numpy(act))
        out = o.step(act, update=True)
        steps += 1
        done = out['done'] != 0
        for b in np.nonzero(done)[0]:
            rec_steps[b].append(int(steps[b]))
            rec_outcome[b].append(int(out['info'][b]))
        ep += done
        steps[done] = 0
        if done.any():
            o.reset(1000 + (np.arange(n) + ep * n) % 500, mask=done.astype(np.uint8))
    eng.sync()
    assert int(_np(bufs['transitions'])[0]) == n * 70
    assert np.array_equal(_np(bufs['ep_count']), ep) and np.array_equal(_np(bufs['cur_steps']), steps)
    got_steps, got_out = _np(bufs['ep_steps']), _np(bufs['ep_outcome'])
    for b in range(n):
        k = min(len(rec_steps[b]), 8)
        assert got_steps[b, :k].tolist() == rec_steps[b][:k] and got_out[b, :k].tolist() == rec_outcome[b][:k]
    assert np.abs(_np(eng.get_state()[0]) - o.get_state()[0]).max() <= 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize('humans,envs,rounds,radius', [(5, 512, 3, 4.0), (20, 128, 2, 12.0), (10, 192, 2, 6.0)])
def test_free_running_soak_vs_oracle(amd, oracle_mod, humans, envs, rounds, radius):
    """Soak: hundreds of envs free-running for 100 steps per round (through and past their terminal states: contact,
    overlap, infeasible programs — the 3-D fallback in every variant), every output of every step bit-identical to
    the oracle; each round starts from fresh oracle-generated scenarios.  H = 20 / 10 run the lane-cooperative fallback."""
    cfg = dict(num_humans=humans, robot_visible=1, circle_radius=radius)
    eng = amd.BatchedCrowdSim(num_envs=envs, robot_policy=amd.ROBOT_ORCA, **cfg)
    for r in range(rounds):
        o = oracle_mod.CrowdOracle(num_envs=envs, robot_policy=1, **cfg)
        o.reset(50000 + 1000 * r + np.arange(envs))
        eng.drop_sims()  # a fresh oracle: fresh rvo2 simulators for every agent on this side too
        eng.set_state(o.get_state()[0], np.zeros(envs))
        for t in range(100):
            got = eng.step(None, update=True, want_obs=False)
            want = o.step(None, update=True)
            assert np.array_equal(_np(got['orca_vel']).view(np.uint32), want['orca_vel'].view(np.uint32)), (r, t)
            for k in ('reward', 'done', 'info', 'dmin', 'action'):
                assert np.array_equal(_np(got[k]), want[k]), (k, r, t)
        s, g = (_np(x) for x in eng.get_state())
        assert np.array_equal(s, o.get_state()[0]) and np.array_equal(g, o.get_state()[1])


@pytest.mark.gpu
def test_survey_known_answer_velocities_on_device(amd):
    """The same known-answer vectors (an independent float32 restatement of RVO2) through cn_step."""
    from oracle_golden_cases import SURVEY_KAT_CASE0
    g = load_golden('resets.npz')
    eng = amd.BatchedCrowdSim(num_envs=1, num_humans=5, robot_policy=amd.ROBOT_ORCA, robot_visible=0)
    eng.set_state(g['test_h5_states'][:1], np.zeros(1))
    for action, hexes in SURVEY_KAT_CASE0:
        out = eng.step(None, update=True, want_obs=False)
        assert tuple(_np(out['action'])[0]) == action and _np(out['reward'])[0] == 0.0
        assert ' '.join(v.tobytes().hex() for v in _np(out['orca_vel'])[0][1:]) == hexes
