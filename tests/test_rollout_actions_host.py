"""cn_rollout_actions without a GPU: the C-ABI surface (declared, bound, exported, no version bump) and the refusals that
depend on the arguments alone — made with pointers that address nothing, so a call that dereferenced one would crash here."""
import ctypes as C
import os

import pytest

from conftest import ROOT
from support import built, NOWHERE  # noqa: F401  (built: module fixture)

DECLARATION = ('int cn_rollout_actions(cn_engine* e, const cn_rollout_io* io, int n_steps, const double* actions, '
               'const cn_trace_out* out);')


def test_header_binding_and_library_agree_on_the_entry_point(built):
    text = open(os.path.join(ROOT, 'include', 'crowdnav_amd.h')).read()
    assert DECLARATION in text
    assert '#define CN_ABI_VERSION 12' in text and '#define CN_LAUNCH_COUNTERS 6' in text
    res, args = built.SYMBOLS['cn_rollout_actions']
    assert res is C.c_int
    assert args == [C.c_void_p, C.POINTER(built.CnRolloutIo), C.c_int, C.c_void_p, C.POINTER(built.CnTraceOut)]
    assert hasattr(C.CDLL(built.LIB_PATH), 'cn_rollout_actions')
    assert built.load().cn_rollout_actions.argtypes == args
    assert built.load().cn_abi_version() == 12 == built.ABI_VERSION  # additive: no version bump
    assert C.sizeof(built.CnTraceOut) == 48 and C.sizeof(built.CnRolloutIo) == 176  # the structs it takes keep their layouts


def test_the_python_entry_point_exists_and_refuses_before_rollout_begin(built):
    from crowdnav_amd.engine import BatchedCrowdSim
    assert callable(BatchedCrowdSim.rollout_actions)
    eng = BatchedCrowdSim.__new__(BatchedCrowdSim)  # no device: only what the method checks first
    eng._rollout = None
    with pytest.raises(RuntimeError):
        eng.rollout_actions(None)
    with pytest.raises(RuntimeError):
        eng.rollout_actions(None, trace=True)
    eng._h = None  # (nothing for __del__ to destroy)


def test_refusals_that_need_no_engine_dereference_nothing(built):
    lib = built.load()
    io = built.CnRolloutIo(seed_mod=1)

    def refused(e, n, actions, out, word):
        assert lib.cn_rollout_actions(e, C.byref(io), n, actions, out) == built.CN_ERR_INVALID
        assert word in lib.cn_last_error().decode(), lib.cn_last_error()

    refused(None, 1, NOWHERE, None, 'engine')
    refused(NOWHERE, 1, None, None, 'actions')
    refused(None, 1, None, None, 'actions')
    for missing in ('state8', 'episode', 'step'):
        rows = {k: 0x10 for k in ('state8', 'episode', 'step', 'reward', 'info', 'dmin')}
        rows[missing] = None
        refused(NOWHERE, 1, NOWHERE, C.byref(built.CnTraceOut(**rows)), missing)
    # the optional arrays may be NULL: the next check speaks (here: the engine)
    bare = built.CnTraceOut(state8=0x10, episode=0x10, step=0x10)
    refused(None, 1, NOWHERE, C.byref(bare), 'engine')
    refused(NOWHERE, -1, NOWHERE, None, 'n_steps')
    refused(NOWHERE, -1, NOWHERE, C.byref(bare), 'n_steps')
    with pytest.raises(built.CrowdNavAmdError) as ei:
        built.check(lib.cn_rollout_actions(None, None, 0, None, None))
    assert ei.value.status == built.CN_ERR_INVALID
