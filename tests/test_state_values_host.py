"""cn_sarl_state_values and cn_lookahead_values without a GPU: the C-ABI surface (declared verbatim, bound, exported, no version
bump, no new counter, cn_lookahead_out unchanged) and the refusals that depend on the arguments alone, in the documented order —
made with pointers that address nothing, so a call that dereferenced one would crash here."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT
from support import built, lookahead_out as _out, NOWHERE  # noqa: F401  (built: module fixture)

STATE_VALUES = ('int cn_sarl_state_values(cn_engine* e, const double* state8, const double* theta, int64_t n, int sort_humans, '
                'float* value);')
LOOKAHEAD_VALUES = ('int cn_lookahead_values(cn_engine* e, int n_steps, int n_candidates, const double* actions, '
                    'const cn_lookahead_out* out,\n'
                    '                        int sort_humans, float* value, double* score);')
REQUIRED = ('ret', 'info', 'steps', 'time')


def test_header_bindings_and_library_agree_on_the_entry_points(built):
    text = open(os.path.join(ROOT, 'include', 'crowdnav_amd.h')).read()
    assert STATE_VALUES in text and LOOKAHEAD_VALUES in text
    assert '#define CN_ABI_VERSION 12' in text and '#define CN_LAUNCH_COUNTERS 6' in text  # additive, nothing new counted
    P = C.c_void_p
    want = {'cn_sarl_state_values': [P, P, P, C.c_int64, C.c_int, P],
            'cn_lookahead_values': [P, C.c_int, C.c_int, P, C.POINTER(built.CnLookaheadOut), C.c_int, P, P]}
    for name, args in want.items():
        res, got = built.SYMBOLS[name]
        assert res is C.c_int and got == args, name
        assert hasattr(C.CDLL(built.LIB_PATH), name)
        assert getattr(built.load(), name).argtypes == args
    assert built.load().cn_abi_version() == 12 == built.ABI_VERSION
    assert [n for n, _ in built.CnLookaheadOut._fields_] == ['ret', 'info', 'steps', 'time', 'final_state8', 'final_theta']
    assert C.sizeof(built.CnLookaheadOut) == 48
    assert len(built.LAUNCH_COUNTERS) == 6


def test_state_values_refuses_its_arguments_in_the_documented_order(built):
    lib = built.load()

    def refused(e, state8, theta, n, value, word):
        assert lib.cn_sarl_state_values(e, state8, theta, n, 0, value) == built.CN_ERR_INVALID
        assert word in lib.cn_last_error().decode(), lib.cn_last_error()

    refused(None, None, None, 0, None, 'state8 is NULL')  # the first check in the documented order speaks
    refused(NOWHERE, None, NOWHERE, 1, NOWHERE, 'state8 is NULL')
    refused(None, NOWHERE, None, 0, None, 'value is NULL')
    refused(NOWHERE, NOWHERE, NOWHERE, 1, None, 'value is NULL')
    refused(None, NOWHERE, None, 0, NOWHERE, 'n must be >= 1')
    refused(NOWHERE, NOWHERE, NOWHERE, -3, NOWHERE, 'n must be >= 1')
    refused(None, NOWHERE, None, 1, NOWHERE, 'engine is NULL')  # theta may be NULL: the next check speaks
    refused(None, NOWHERE, NOWHERE, 1 << 40, NOWHERE, 'engine is NULL')
    with pytest.raises(built.CrowdNavAmdError) as ei:
        built.check(lib.cn_sarl_state_values(None, None, None, 0, 1, None))
    assert ei.value.status == built.CN_ERR_INVALID


def test_lookahead_values_speaks_the_lookahead_s_own_refusals_first(built):
    lib = built.load()

    def refused(e, n, k, actions, out, value, score, word):
        assert lib.cn_lookahead_values(e, n, k, actions, out, 0, value, score) == built.CN_ERR_INVALID
        msg = lib.cn_last_error().decode()
        assert word in msg and msg.startswith('cn_lookahead_actions'), msg
        assert lib.cn_lookahead_actions(e, n, k, actions, out) == built.CN_ERR_INVALID  # the call without the bootstrap says the same
        assert lib.cn_last_error().decode() == msg

    full = _out(built)
    for value, score in ((NOWHERE, NOWHERE), (None, None)):  # whatever the bootstrap's own arguments are
        refused(NOWHERE, 1, 1, None, C.byref(full), value, score, 'actions')
        refused(None, -1, 0, None, None, value, score, 'actions')
        refused(NOWHERE, 1, 1, NOWHERE, None, value, score, 'out is NULL')
        for missing in REQUIRED:
            refused(NOWHERE, 1, 1, NOWHERE, C.byref(_out(built, **{missing: None})), value, score, 'out->' + missing)
        # final_state8 is the bootstrap's own requirement: it comes after every check of cn_lookahead_actions
        bare = _out(built, final_state8=None, final_theta=None)
        refused(NOWHERE, -1, 1, NOWHERE, C.byref(bare), value, score, 'n_steps')
        refused(NOWHERE, 0, 0, NOWHERE, C.byref(full), value, score, 'n_candidates')
        refused(None, 1, 1, NOWHERE, C.byref(bare), value, score, 'engine')
        refused(None, 0, 1, NOWHERE, C.byref(full), value, score, 'engine')  # n_steps == 0 is a no-op of an ENGINE


def test_the_python_entry_points_check_shapes_first(built):
    from crowdnav_amd.compat.crowd_sim import CrowdSim
    from crowdnav_amd.engine import BatchedCrowdSim
    assert callable(BatchedCrowdSim.sarl_state_values) and callable(CrowdSim.lookahead)
    eng = BatchedCrowdSim.__new__(BatchedCrowdSim)  # no device: only what the methods check first
    eng.B, eng.H, eng.A, eng._h = 3, 5, 6, None
    for bad in (np.zeros((6, 8)), np.zeros((2, 5, 8)), np.zeros((2, 6, 7)), np.zeros(8), np.zeros((4, 2, 7, 8))):
        with pytest.raises(ValueError, match='state8 must be'):
            eng.sarl_state_values(bad)
    for bad in (np.zeros(3), np.zeros((2, 3)), np.zeros((4, 1))):
        with pytest.raises(ValueError, match='theta must be'):
            eng.sarl_state_values(np.zeros((2, 2, 6, 8)), theta=bad)
    for bad in ([[0.0, 0.0]], [[[0.0, 0.0]]] * 3, [[[[0.0] * 3]]] * 3, [[[[0.0] * 2]]] * 2):
        with pytest.raises(ValueError, match='actions must be'):
            eng.lookahead(bad, bootstrap=True)
