"""Oracle parity AT THE SIZES AND IN THE ARRANGEMENT bench.py measures (VERDICT r4 "missing #1": every full-size test used to
be a self-comparison).  Three runs, each against oracle/crowd_oracle.cpp's rollout (co_rollout_full: the restatement of
/root/reference crowd_sim/envs/crowd_sim.py:317-420 + crowd_nav/utils/explorer.py:35-72 with everything explorer.py:46-62 keeps
per episode), OpenMP over envs — seconds on the GPU box's host:

  (a) BASELINE configs[1] exactly as bench.py's default `--steps 20 --warmup 5` run drives it: 4096 envs x 5 humans, episode
      seeds 2000 + c, launches of 200 / 5 / 20 steps, ABI-v6 arrangement (per-env transition counters, no in-kernel summary,
      ONE record per env) -> rollout_fused_kernel<true>; the shard-boundary numbers (cn_rollout_summary) against
      explorer.py:74-90 computed from the ORACLE's records.
  (b) configs[3]'s shard with its schedule engaging BY ITSELF (no CROWDNAV_AMD_SCHED_FORCE): 4096 envs x 20 humans, 12 m circle,
      launches of 150 / 49 / 3 steps -> rollout_kernel<10, false, true, true> as persistent workgroups on a device queue of
      (env, visit) items (the default) and as the static 3-of-4 sub-launches over 3072 workgroups; the engine's launch counters
      prove which path ran.
  (c) the same shard on the reference's own 4 m circle with CN_FLAG_ASYNC_SCENARIO_FILL: timing decides when an env pauses,
      never what it plays — every finished episode is the oracle's, in order.
Integer results bit-exact, float64 sums / states to 1e-9 (scenario generation: device sincos vs libm, <= 1e-12 per reset)."""
import numpy as np
import pytest

from support import amd, np_of as _np  # noqa: F401  (amd: module fixture)

pytestmark = pytest.mark.gpu

REACH_GOAL, COLLISION, TIMEOUT = 2, 3, 4


def _ring_view(rec, K):
    """What a K-deep record ring holds after the oracle's episodes: slot j = the env's most recent episode with ordinal
    congruent to j (include/crowdnav_amd.h: cn_rollout_io.record_capacity)."""
    B, M = rec['outcome'].shape
    assert rec['count'].max() <= M, 'oracle record table too small for this run'
    held = np.zeros((B, K), bool)
    ordinal = np.zeros((B, K), np.int64)
    for j in range(K):
        n = rec['count'].astype(np.int64)
        last = n - 1 - ((n - 1 - j) % K)  # largest ordinal < n congruent to j
        held[:, j] = (n > j)
        ordinal[:, j] = np.where(held[:, j], last, 0)
    take = lambda a: np.where(held, np.take_along_axis(a, ordinal, axis=1), 0)  # noqa: E731
    return held, {k: take(rec[k]) for k in ('outcome', 'steps', 'ret', 'time', 'danger', 'dsum')}


def _explorer_summary(rec, K):
    """explorer.py:50-62, 71-90 over the records a K-deep ring holds: the eight numbers of cn_records_summary"""
    held, r = _ring_view(rec, K)
    out = r['outcome']
    ok = held & (out == REACH_GOAL)
    return np.array([rec['count'].sum(), held.sum(), ok.sum(), (held & (out == COLLISION)).sum(),
                     (held & (out == TIMEOUT)).sum(), r['time'][ok].sum(), r['ret'][held].sum(), r['danger'][held].sum()],
                    dtype=np.float64)


def _compare_rings(bufs, rec, K):
    held, want = _ring_view(rec, K)
    for key, name, exact in (('ep_outcome', 'outcome', True), ('ep_steps', 'steps', True), ('ep_danger', 'danger', True),
                             ('ep_time', 'time', True), ('ep_return', 'ret', False), ('ep_danger_dmin_sum', 'dsum', False)):
        got = np.where(held, _np(bufs[key]), 0)
        if exact:
            assert np.array_equal(got, want[name]), key
        else:
            assert np.abs(got - want[name]).max() <= 1e-9, key


def test_configs1_as_bench_drives_it_vs_oracle(amd, oracle_mod):
    B, H, K = 4096, 5, 1
    launches = [200, 5, 20]  # bench.py: --preroll 200, --warmup 5, --steps 20 (chunk 1000)
    steps = sum(launches)
    cfg = dict(num_humans=H, robot_visible=1, circle_radius=4.0)
    ora = oracle_mod.CrowdOracle(num_envs=B, robot_policy=1, **cfg)
    ora.reset(2000 + np.arange(B))
    total, rec, cur = ora.rollout_full(steps, 2000, 2 ** 32 - 2000, 16)

    eng = amd.BatchedCrowdSim(num_envs=B, robot_policy=amd.ROBOT_ORCA, **cfg)
    bufs = eng.rollout_begin(seed_base=2000, seed_mod=2 ** 32 - 2000, episode_limit=-1, record_capacity=K, env_offset=0,
                             env_stride=B, boundary_records=0, per_env_transitions=True)
    eng.rollout(launches[0])
    eng.rollout_summary()  # bench.py warms the boundary up here
    eng.rollout(launches[1])
    before = eng.launch_counts()
    eng.rollout(launches[2])
    after = eng.launch_counts()
    summary = _np(eng.rollout_summary())
    eng.sync()
    # the launch bench.py times: ONE kernel, no scenario fill in front of it (ring budget: 5 + 20 <= 48 steps since the last fill)
    assert after['rollout_kernels'] - before['rollout_kernels'] == 1 and after['ring_fills'] == before['ring_fills']

    assert total == B * steps
    assert np.array_equal(_np(bufs['env_transitions']).astype(np.int64), np.full(B, steps))  # nobody paused
    assert np.array_equal(_np(bufs['ep_count']), rec['count']) and rec['count'].min() >= 3
    _compare_rings(bufs, rec, K)
    assert np.array_equal(_np(bufs['cur_steps']), cur['steps'])
    assert np.array_equal(_np(bufs['cur_danger']), cur['danger'])
    assert np.abs(_np(bufs['cur_return']) - cur['ret']).max() <= 1e-9
    assert np.abs(_np(bufs['cur_danger_dmin_sum']) - cur['dsum']).max() <= 1e-9
    s_eng, g_eng = eng.get_state()
    s_ora, g_ora = ora.get_state()
    assert np.array_equal(_np(g_eng), g_ora)
    assert np.abs(_np(s_eng) - s_ora).max() <= 1e-9
    # explorer.py:74-90 from the ORACLE's episodes against cn_rollout_summary
    want = _explorer_summary(rec, K)
    assert np.array_equal(summary[[0, 1, 2, 3, 4, 7]], want[[0, 1, 2, 3, 4, 7]])
    assert summary[5] == want[5]  # nav times are multiples of 0.25: exact in any order
    assert abs(summary[6] - want[6]) <= 1e-9 * max(1.0, abs(want[6]))
    assert want[1] == B  # every env holds its most recent episode


def _shard20(amd, oracle_mod, radius, flags, seed, launches, K):
    B, H = 4096, 20
    cfg = dict(num_humans=H, robot_visible=1, circle_radius=radius)
    ora = oracle_mod.CrowdOracle(num_envs=B, robot_policy=1, **cfg)
    ora.reset(seed[0] + np.arange(B) % seed[1])
    total, rec, cur = ora.rollout_full(sum(launches), seed[0], seed[1], K)
    eng = amd.BatchedCrowdSim(num_envs=B, robot_policy=amd.ROBOT_ORCA, flags=flags, **cfg)
    bufs = eng.rollout_begin(seed_base=seed[0], seed_mod=seed[1], episode_limit=-1, record_capacity=K)
    counts = [eng.launch_counts()]
    for n in launches:
        eng.rollout(n)
        counts.append(eng.launch_counts())
    eng.sync()
    return ora, total, rec, cur, eng, bufs, counts


@pytest.mark.parametrize('dynamic', [True, False])
def test_configs3_shard_schedule_engages_by_itself_vs_oracle(amd, oracle_mod, monkeypatch, dynamic):
    """dynamic: ONE launch of persistent workgroups taking (env, visit) items from a device queue (the default since round 5);
    static (CROWDNAV_AMD_SCHED_DYNAMIC=0, and whenever the caller asks for in-kernel statistics): the 3-of-4 sub-launches."""
    monkeypatch.delenv('CROWDNAV_AMD_SCHED_FORCE', raising=False)
    monkeypatch.delenv('CROWDNAV_AMD_SCHED_MIN_STEPS', raising=False)
    monkeypatch.setenv('CROWDNAV_AMD_SCHED_DYNAMIC', '1' if dynamic else '0')
    import torch
    if torch.cuda.get_device_properties(0).multi_processor_count != 256:
        pytest.skip('the round arithmetic of the 3-of-4 schedule is stated for 256 CUs')
    launches, K = [150, 49, 3], 16
    ora, total, rec, cur, eng, bufs, counts = _shard20(amd, oracle_mod, 12.0, 0, (1000, 500), launches, K)
    d = [{k: b[k] - a[k] for k in a} for a, b in zip(counts, counts[1:])]
    if dynamic:  # one persistent launch per call of 24+ steps; 3 steps: a plain launch over all envs
        assert [x['rollout_kernels'] for x in d] == [1, 1, 1]
        assert [x['scheduled_kernels'] for x in d] == [1, 1, 0]
    else:  # 150 = 3 x 50: four sub-launches; 49 = 3 x 16 + 1: one launch over all envs + four; 3 < 48: one plain launch
        assert [x['rollout_kernels'] for x in d] == [4, 5, 1]
        assert [x['scheduled_kernels'] for x in d] == [4, 4, 0]
    steps = sum(launches)
    assert int(_np(bufs['transitions'])[0]) == total == 4096 * steps
    assert np.array_equal(_np(bufs['ep_count']), rec['count']) and rec['count'].min() >= 1
    _compare_rings(bufs, rec, K)
    assert np.array_equal(_np(bufs['cur_steps']), cur['steps'])
    assert np.array_equal(_np(bufs['cur_danger']), cur['danger'])
    assert np.abs(_np(bufs['cur_return']) - cur['ret']).max() <= 1e-9
    assert np.abs(_np(eng.get_state()[0]) - ora.get_state()[0]).max() <= 1e-9
    assert np.array_equal(_np(eng.get_state()[1]), ora.get_state()[1])
    got, want = _np(eng.rollout_summary()), _explorer_summary(rec, K)
    assert np.array_equal(got[[0, 1, 2, 3, 4, 5, 7]], want[[0, 1, 2, 3, 4, 5, 7]])
    assert abs(got[6] - want[6]) <= 1e-9 * max(1.0, abs(want[6]))


def test_configs3_shard_reference_geometry_async_fill_vs_oracle(amd, oracle_mod, monkeypatch):
    monkeypatch.delenv('CROWDNAV_AMD_SCHED_FORCE', raising=False)
    B, H, K = 4096, 20, 32
    cold, warm = [150, 49, 3], [120]
    cfg = dict(num_humans=H, robot_visible=1, circle_radius=4.0)
    # 'test' phase seeds 1000 + c % 1021: the reference's own rejection sampling terminates on them (bench.py: measure_h20)
    ora = oracle_mod.CrowdOracle(num_envs=B, robot_policy=1, **cfg)
    ora.reset(1000 + np.arange(B) % 1021)
    total, rec, _ = ora.rollout_full(sum(cold) + sum(warm), 1000, 1021, K)
    eng = amd.BatchedCrowdSim(num_envs=B, robot_policy=amd.ROBOT_ORCA, flags=amd.FLAG_ASYNC_SCENARIO_FILL, **cfg)
    bufs = eng.rollout_begin(seed_base=1000, seed_mod=1021, episode_limit=-1, record_capacity=K)

    def check(n_calls, steps_so_far):
        counts = eng.launch_counts()
        assert counts['async_fills'] == n_calls and counts['ring_fills'] == 0
        cnt = _np(bufs['ep_count'])
        assert (cnt <= rec['count']).all() and cnt.max() <= K and cnt.min() >= 1  # paused envs are behind, never ahead
        steps = _np(bufs['ep_steps'])
        live = np.arange(K)[None, :] < cnt[:, None]
        for key, name in (('ep_outcome', 'outcome'), ('ep_steps', 'steps'), ('ep_time', 'time'), ('ep_danger', 'danger')):
            assert np.array_equal(np.where(live, _np(bufs[key]), 0), np.where(live, rec[name], 0)), key
        assert np.abs(np.where(live, _np(bufs['ep_return']) - rec['ret'], 0)).max() <= 1e-9
        ran = np.where(live, steps, 0).sum(axis=1) + _np(bufs['cur_steps'])
        assert int(_np(bufs['transitions'])[0]) == ran.sum() and ran.max() <= steps_so_far
        return ran

    # cold start: the generators have 4096 x 47 scenarios to produce beside the first launches: most envs wait for their second
    for n in cold:
        eng.rollout(n)
    eng.sync()  # (also drains the fill streams: the ring is full now)
    ran_cold = check(len(cold), sum(cold))
    # ... then on a full ring, the generators topping it up beside the launch
    for n in warm:
        eng.rollout(n)
    eng.sync()
    ran = check(len(cold) + len(warm), sum(cold) + sum(warm))
    assert ((ran - ran_cold) == sum(warm)).sum() >= B // 2, 'on a full ring most envs never wait in a 120-step call'
    print('paused env-steps: cold start %d of %d, full ring %d of %d'
          % (B * sum(cold) - ran_cold.sum(), B * sum(cold), B * sum(warm) - (ran - ran_cold).sum(), B * sum(warm)))
