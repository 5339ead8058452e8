"""cn_rollout_trace without a GPU: the C-ABI surface (declared, exported, refuses NULL before any device work) and
crowdnav_amd.trace.episodes, a pure function of the trace arrays, on synthetic traces."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT
from support import built  # noqa: F401  (built: module fixture)


def test_header_declares_and_library_exports_the_entry_point(built):
    text = open(os.path.join(ROOT, 'include', 'crowdnav_amd.h')).read()
    assert 'int cn_rollout_trace(cn_engine* e, const cn_rollout_io* io, int n_steps, const cn_trace_out* out);' in text
    assert 'typedef struct cn_trace_out' in text
    assert '#define CN_LAUNCH_COUNTERS 6' in text
    lib = C.CDLL(built.LIB_PATH)
    assert hasattr(lib, 'cn_rollout_trace')
    assert 'cn_rollout_trace' in built.SYMBOLS
    assert built.load().cn_abi_version() == 12 == built.ABI_VERSION  # additive: no version bump


def test_struct_layouts(built):
    assert C.sizeof(built.CnTraceOut) == 48  # six device pointers
    assert [f[0] for f in built.CnTraceOut._fields_] == ['state8', 'episode', 'step', 'reward', 'info', 'dmin']
    assert C.sizeof(built.CnRolloutIo) == 176  # cn_rollout_io keeps its size


def test_null_arguments_are_refused_before_any_device_work(built):
    lib = built.load()
    io, out = built.CnRolloutIo(seed_mod=1), built.CnTraceOut()
    assert lib.cn_rollout_trace(None, C.byref(io), 1, C.byref(out)) == built.CN_ERR_INVALID
    assert 'engine' in lib.cn_last_error().decode()
    with pytest.raises(built.CrowdNavAmdError) as ei:
        built.check(lib.cn_rollout_trace(None, None, 0, None))
    assert ei.value.status == built.CN_ERR_INVALID


# ------------------------------------------------------------------------------------------------ trace.episodes
A = 3
INFO_END = {2, 3, 4}


def _synthetic(plan, n, rewards=True):
    """plan[b]: the (ordinal, step, info) of every step of the call for env b, None where the env made no transition.
    state8[b, t] is filled with a number that names (b, t); rows of idle envs keep a fill value."""
    B = len(plan)
    tr = dict(state8=np.full((B, n, A, 8), -7.0), episode=np.full((B, n), -1, np.int32), step=np.full((B, n), 99, np.int32))
    if rewards:
        tr.update(reward=np.full((B, n), -7.0), info=np.full((B, n), 9, np.uint8), dmin=np.full((B, n), -7.0))
    for b, rows in enumerate(plan):
        assert len(rows) == n
        for t, row in enumerate(rows):
            if row is None:
                continue
            tr['state8'][b, t] = 1000 * b + t + np.arange(A * 8).reshape(A, 8) / 100.0
            tr['episode'][b, t], tr['step'][b, t] = row[0], row[1]
            if rewards:
                tr['reward'][b, t], tr['info'][b, t], tr['dmin'][b, t] = 0.5 * t + b, row[2], 0.25 * t
    return tr


def _episode_rows(j, T, last_info, first=0, upto=None):
    """Steps first..upto-1 of an episode of T transitions that ends with last_info."""
    upto = T if upto is None else upto
    return [(j, s, last_info if s == T - 1 else (1 if s % 2 else 0)) for s in range(first, upto)]


def test_two_envs_with_episodes_that_end_inside_the_call():
    from crowdnav_amd.trace import episodes
    plan = [_episode_rows(0, 4, 2) + _episode_rows(1, 3, 3) + _episode_rows(2, 5, 4, upto=2),
            _episode_rows(0, 6, 3) + _episode_rows(1, 3, 2)]
    tr = _synthetic(plan, 9)
    eps = episodes(tr)
    assert sorted(eps) == [0, 1, 2, 3, 4]  # id = b + 2 j
    assert [len(eps[c]['state8']) for c in (0, 2, 4, 1, 3)] == [4, 3, 2, 6, 3]
    assert [eps[c]['complete'] for c in (0, 2, 4, 1, 3)] == [True, True, False, True, True]
    assert np.array_equal(eps[2]['state8'], tr['state8'][0, 4:7]) and eps[2]['state8'].shape == (3, A, 8)
    assert np.array_equal(eps[2]['reward'], tr['reward'][0, 4:7]) and np.array_equal(eps[2]['dmin'], tr['dmin'][0, 4:7])
    assert eps[2]['info'].tolist() == [0, 1, 3] and eps[1]['info'][-1] == 3
    assert np.array_equal(eps[3]['state8'], tr['state8'][1, 6:9])


def test_rows_of_a_retired_or_paused_env_are_dropped():
    from crowdnav_amd.trace import episodes
    plan = [_episode_rows(0, 3, 2) + [None] * 4,                                     # retired after its only episode
            _episode_rows(0, 2, 3) + [None, None] + _episode_rows(1, 3, 2),          # paused for two steps between episodes
            [None] * 7]                                                              # never ran
    tr = _synthetic(plan, 7)
    eps = episodes(tr)
    assert sorted(eps) == [0, 1, 4]
    assert all(e['complete'] for e in eps.values())
    assert np.array_equal(eps[4]['state8'], tr['state8'][1, 4:7])
    for e in eps.values():  # nothing of the fill values got in
        assert (e['state8'] >= 0).all() and (e['info'] < 9).all()


def test_an_episode_cut_by_the_call_boundary_is_joined_by_the_next_trace():
    from crowdnav_amd.trace import episodes
    first = _synthetic([_episode_rows(0, 2, 2) + _episode_rows(1, 6, 3, upto=3)], 5)
    second = _synthetic([_episode_rows(1, 6, 3, first=3) + _episode_rows(2, 4, 2, upto=1)], 4)
    a = episodes(first)
    assert a[0]['complete'] is True and a[1]['complete'] is False and len(a[1]['state8']) == 3
    b = episodes(second)
    assert b[1]['complete'] is False  # its first row is not here
    both = episodes([first, second])
    assert sorted(both) == [0, 1, 2]
    assert both[1]['complete'] is True and both[2]['complete'] is False
    assert np.array_equal(both[1]['state8'], np.concatenate([first['state8'][0, 2:5], second['state8'][0, 0:3]]))
    assert np.array_equal(both[1]['reward'], np.concatenate([first['reward'][0, 2:5], second['reward'][0, 0:3]]))
    # rows missing in the middle (an untraced call in between): joined, but not complete
    gap = _synthetic([_episode_rows(1, 6, 3, first=4) + [None] * 2], 4)
    assert episodes([first, gap])[1]['complete'] is False


def test_shard_numbering_and_traces_without_rewards():
    from crowdnav_amd.trace import episodes
    plan = [_episode_rows(0, 2, 2) + _episode_rows(1, 2, 3), _episode_rows(0, 3, 2) + _episode_rows(1, 1, 2)]
    tr = _synthetic(plan, 4)
    eps = episodes(tr, env_offset=6, env_stride=16)  # envs 6 and 7 of a 16-env job
    assert sorted(eps) == [6, 7, 22, 23]
    assert len(eps[22]['state8']) == 2 and len(eps[23]['state8']) == 1 and len(eps[7]['state8']) == 3
    bare = _synthetic(plan, 4, rewards=False)
    eps = episodes(bare, env_offset=6, env_stride=16)
    assert sorted(eps) == [6, 7, 22, 23]
    assert all(e['complete'] is None and e['reward'] is None and e['info'] is None and e['dmin'] is None for e in eps.values())
    assert np.array_equal(eps[23]['state8'], bare['state8'][1, 3:4])
    with pytest.raises(ValueError):
        episodes([tr, bare])
    assert episodes([]) == {}
