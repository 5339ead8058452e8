"""What the scenario-ring suites (test_ring_wrap, test_shard20, test_lagged_fill) share: the oracle's rollout on the engines'
seeds, an engine run through a list of launches at a given ring depth, and the comparison of the episode records."""
import numpy as np

from support import environ, np_of


def oracle_rollout(oracle_mod, B, steps, K, **cfg):
    o = oracle_mod.CrowdOracle(num_envs=B, robot_policy=1, **cfg)
    o.reset(1000 + np.arange(B))
    ep_index, cur_steps, cur_ret = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.float64)
    total, rec = o.rollout(steps, 1000, 500, K, ep_index, cur_steps, cur_ret)
    return o, total, rec, cur_steps, cur_ret


def ring_engine(amd, B, launches, K, depth, flags=0, **cfg):
    with environ(CROWDNAV_AMD_RING_DEPTH=depth):
        eng = amd.BatchedCrowdSim(num_envs=B, robot_policy=amd.ROBOT_ORCA, flags=flags, **cfg)
    bufs = eng.rollout_begin(seed_base=1000, seed_mod=500, episode_limit=-1, record_capacity=K)
    for n in launches:
        eng.rollout(n)
    eng.sync()
    return eng, bufs


def records_in_order(bufs, rec, K):
    """every episode the engine finished is the oracle's episode of the same ordinal: outcome, length, return"""
    cnt = np_of(bufs['ep_count'])
    assert (cnt <= rec['count']).all() and cnt.max() <= K, (cnt, rec['count'], K)
    out, steps, ret = np_of(bufs['ep_outcome']), np_of(bufs['ep_steps']), np_of(bufs['ep_return'])
    for b in range(len(cnt)):
        k = cnt[b]
        assert np.array_equal(out[b, :k], rec['outcome'][b, :k]), b
        assert np.array_equal(steps[b, :k], rec['steps'][b, :k]), b
        assert np.allclose(ret[b, :k], rec['ret'][b, :k], rtol=0, atol=1e-12), b
    return cnt
