"""cn_lookahead_actions without a GPU: the C-ABI surface (declared, bound, exported, no version bump, no new counter) and the
refusals that depend on the arguments alone, in the documented order — made with pointers that address nothing, so a call
that dereferenced one would crash here."""
import ctypes as C
import os

import pytest

from conftest import ROOT
from support import built, lookahead_out as _out, NOWHERE  # noqa: F401  (built: module fixture)

DECLARATION = ('int cn_lookahead_actions(cn_engine* e, int n_steps, int n_candidates, const double* actions /* [B][K][n][2] */,\n'
               '                         const cn_lookahead_out* out);')
REQUIRED = ('ret', 'info', 'steps', 'time')


def test_header_binding_and_library_agree_on_the_entry_point(built):
    text = open(os.path.join(ROOT, 'include', 'crowdnav_amd.h')).read()
    assert DECLARATION in text
    assert '#define CN_ABI_VERSION 12' in text and '#define CN_LAUNCH_COUNTERS 6' in text  # additive; the launch is not counted
    res, args = built.SYMBOLS['cn_lookahead_actions']
    assert res is C.c_int
    assert args == [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(built.CnLookaheadOut)]
    assert hasattr(C.CDLL(built.LIB_PATH), 'cn_lookahead_actions')
    assert built.load().cn_lookahead_actions.argtypes == args
    assert built.load().cn_abi_version() == 12 == built.ABI_VERSION
    assert [n for n, _ in built.CnLookaheadOut._fields_] == ['ret', 'info', 'steps', 'time', 'final_state8', 'final_theta']
    assert C.sizeof(built.CnLookaheadOut) == 48
    assert len(built.LAUNCH_COUNTERS) == 6


def test_the_python_entry_points_exist(built):
    from crowdnav_amd.compat.crowd_sim import CrowdSim
    from crowdnav_amd.engine import BatchedCrowdSim
    assert callable(BatchedCrowdSim.lookahead) and callable(CrowdSim.lookahead)
    eng = BatchedCrowdSim.__new__(BatchedCrowdSim)  # no device: only what the method checks first
    eng.B, eng._h = 3, None
    for bad in ([[0.0, 0.0]], [[[0.0, 0.0]]] * 3, [[[[0.0] * 3]]] * 3, [[[[0.0] * 2]]] * 2):
        with pytest.raises(ValueError, match='actions must be'):
            eng.lookahead(bad)


def test_refusals_that_need_no_engine_dereference_nothing(built):
    lib = built.load()

    def refused(e, n, k, actions, out, word):
        assert lib.cn_lookahead_actions(e, n, k, actions, out) == built.CN_ERR_INVALID
        assert word in lib.cn_last_error().decode(), lib.cn_last_error()

    full = _out(built)
    refused(NOWHERE, 1, 1, None, C.byref(full), 'actions')
    refused(None, -1, 0, None, None, 'actions')  # the first check in the documented order speaks
    refused(NOWHERE, 1, 1, NOWHERE, None, 'out is NULL')
    for missing in REQUIRED:
        refused(NOWHERE, 1, 1, NOWHERE, C.byref(_out(built, **{missing: None})), 'out->' + missing)
        refused(None, -1, 0, NOWHERE, C.byref(_out(built, **{missing: None})), 'out->' + missing)
    # the optional arrays may be NULL: the next check speaks
    bare = _out(built, final_state8=None, final_theta=None)
    refused(NOWHERE, -1, 1, NOWHERE, C.byref(bare), 'n_steps')
    refused(NOWHERE, -1, 0, NOWHERE, C.byref(full), 'n_steps')
    refused(NOWHERE, 0, 0, NOWHERE, C.byref(full), 'n_candidates')
    refused(NOWHERE, 5, -3, NOWHERE, C.byref(bare), 'n_candidates')
    refused(None, 1, 1, NOWHERE, C.byref(bare), 'engine')
    refused(None, 0, 1, NOWHERE, C.byref(full), 'engine')  # n_steps == 0 is a no-op of an ENGINE, not of nothing
    with pytest.raises(built.CrowdNavAmdError) as ei:
        built.check(lib.cn_lookahead_actions(None, 0, 0, None, None))
    assert ei.value.status == built.CN_ERR_INVALID
