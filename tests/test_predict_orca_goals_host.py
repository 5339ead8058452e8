"""The ORCA predictor on hypothesised goals (cn_predict_orca_goals) and the sampler of such goals (cn_goal_hypotheses) without a
GPU: crowdnav_amd.predict.goal_hypotheses — the sampler's numpy restatement and the device kernel's oracle — by its own
properties; on the CPU oracle alone, what the fixed goal maps of test_predict_orca_goals.py must do to the scenes for its
bit-for-bit comparison to mean something; the C-ABI surface; and the refusals that depend on the arguments alone, in the
header's order (made with a NULL engine and pointers that address nothing: a refusal reads none of them)."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT

import predict_orca_cases as cases
import predict_orca_goals_cases as goals_cases
from support import built, DANGLING  # noqa: F401  (built: module fixture)

STD = dict(std_heading=0.4, std_distance=0.3, seed=(7 << 32) | 5, counter=3)


def _state(B=3, H=5, seed=0):
    """A made-up [B, A, 8] state: human 1 of every env stands still."""
    rng = np.random.RandomState(seed)
    state = rng.uniform(-4.0, 4.0, size=(B, H + 1, 8))
    state[:, :, 6], state[:, :, 7] = 0.3, 1.0
    state[:, 1, 2:4] = 0.0
    return state


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------ predict.goal_hypotheses
def test_mode_0_and_the_unperturbed_modes():
    from crowdnav_amd import predict
    state = _state()
    p, v, g = state[:, 1:, 0:2], state[:, 1:, 2:4], state[:, 1:, 4:6]
    # 'engine' with nominal_first: mode 0 is the goal columns, bit for bit
    eng = predict.goal_hypotheses(state, 8, 'engine', **STD)
    assert eng.shape == (3, 8, 5, 2) and eng.dtype == np.float64 and _same(eng[:, 0], np.ascontiguousarray(g))
    assert all((eng[:, m] != g).any() for m in range(1, 8))
    # ... without it mode 0 is a sample like the others, and the others are what they were
    free = predict.goal_hypotheses(state, 8, 'engine', nominal_first=False, **STD)
    assert (free[:, 0] != g).any() and _same(free[:, 1:], eng[:, 1:])
    # 'heading': a standing human's goal is its position in every mode; a walking one's nominal goal lies `reach` ahead
    head = predict.goal_hypotheses(state, 8, 'heading', reach=2.5, **STD)
    assert _same(head[:, :, 0], np.ascontiguousarray(np.broadcast_to(p[:, None, 0], (3, 8, 2))))
    speed = np.sqrt(v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1])
    walking = speed > 0.0
    assert walking[:, 1:].all() and not walking[:, 0].any()
    safe = np.where(walking, speed, 1.0)
    d = np.where(walking[..., None], np.stack([(v[..., 0] / safe) * 2.5, (v[..., 1] / safe) * 2.5], axis=-1), 0.0)
    assert _same(head[:, 0], p + d)
    assert np.allclose(np.hypot(*np.moveaxis(head[:, 0] - p, -1, 0))[walking], 2.5, rtol=0, atol=1e-12)
    # both deviations 0: every perturbed mode is p + d exactly
    for base, nominal, kw in (('engine', p + (g - p), {}), ('heading', p + d, dict(reach=2.5))):
        flat = predict.goal_hypotheses(state, 8, base, std_heading=0.0, std_distance=0.0, nominal_first=False, seed=9, counter=1, **kw)
        assert _same(flat, np.ascontiguousarray(np.broadcast_to(nominal[:, None], flat.shape))), base
    # the stretch is not negative: with a huge deviation some samples land on the human itself, none behind it
    wild = predict.goal_hypotheses(state, 8, 'heading', reach=2.5, std_distance=50.0, nominal_first=False, seed=1)
    at = (wild == p[:, None]).all(axis=-1)[:, :, 1:]
    assert at.any() and not at.all()
    along = ((wild - p[:, None]) * d[:, None]).sum(axis=-1)
    assert (along >= 0.0).all()


def test_rows_depend_on_neither_B_M_nor_H():
    from crowdnav_amd import predict
    state = _state(B=3, H=5)
    for base, kw in (('engine', {}), ('heading', dict(reach=3.0))):
        full = predict.goal_hypotheses(state, 8, base, **STD, **kw)
        assert _same(predict.goal_hypotheses(state[:2], 8, base, **STD, **kw), np.ascontiguousarray(full[:2])), base
        assert _same(predict.goal_hypotheses(state, 3, base, **STD, **kw), np.ascontiguousarray(full[:, :3])), base
        assert _same(predict.goal_hypotheses(state[:, :4], 8, base, **STD, **kw), np.ascontiguousarray(full[:, :, :3])), base
        # the same arguments: the same bits; another counter or seed: other rows, mode 0 apart
        assert _same(predict.goal_hypotheses(state, 8, base, **STD, **kw), full)
        for other in (dict(counter=4), dict(seed=STD['seed'] + 1), dict(seed=STD['seed'] + (1 << 32))):
            moved = predict.goal_hypotheses(state, 8, base, **dict(STD, **other), **kw)
            assert _same(moved[:, 0], full[:, 0]) and (moved[:, 1:, 1:] != full[:, 1:, 1:]).any(axis=-1).all(), (base, other)


def test_numpy_in_numpy_out_torch_in_torch_out():
    import torch
    from crowdnav_amd import predict
    state = _state()
    want = predict.goal_hypotheses(state, 4, 'heading', reach=3.0, **STD)
    assert isinstance(want, np.ndarray)
    got = predict.goal_hypotheses(torch.from_numpy(state), 4, 'heading', reach=3.0, **STD)
    assert torch.is_tensor(got) and got.dtype == torch.float64 and got.is_contiguous() and _same(got.numpy(), want)
    assert 'goal_hypotheses' in predict.__doc__ and 'predict_orca_goals' in predict.__doc__
    for bad in (dict(base='track'), dict(M=0), dict(M=9), dict(base='heading', reach=None), dict(base='heading', reach=0.0),
                dict(std_heading=-1.0), dict(std_distance=float('nan'))):
        args = dict(dict(M=4, base='engine'), **bad)
        with pytest.raises(ValueError, match='goal_hypotheses'):
            predict.goal_hypotheses(state, **args)
    with pytest.raises(ValueError, match='state8'):
        predict.goal_hypotheses(state[0], 4, 'engine')


# ------------------------------------------------------------------------------------------------ the scenes of the GPU test
@pytest.mark.parametrize('crowd', ['h5', 'h12', 'h20', 'h5_mixed'])
def test_the_goal_maps_bite(oracle_mod, crowd):
    """On the CPU oracle alone, for every crowd of five or more: the three re-goaled states give three pairwise different
    tables; with the goals turned a quarter circle ORCA acts (some human's rows are not predict.to_goal's on that state);
    with every goal the human's own position some human is pushed off it (a row that is not zero).
    h5_mixed fails the last one with that map — one to three humans per scene, metres apart: the table of standing humans is
    all zeros — so its mode 2 sends every human to the origin instead (goal_maps), and beside the non-zero row ORCA must have
    acted there as in mode 1."""
    from crowdnav_amd import predict
    state, gtime = cases.oracle_start(oracle_mod, crowd)
    maps = goals_cases.goal_maps(state, crowd)
    states = [goals_cases.regoaled(state, maps[:, m]) for m in range(3)]
    assert _same(states[0], np.asarray(state, dtype=np.float64))
    tables = [cases.oracle_table(oracle_mod, crowd, s, gtime)[0] for s in states]
    for a, b in ((0, 1), (0, 2), (1, 2)):
        assert (tables[a] != tables[b]).any(), (a, b)
    from_goal = cases.differs_from(tables[1], predict.to_goal(states[1], cases.N, 0.25))
    pushed = np.abs(tables[2]).max()
    print(crowd, 'turned goals: furthest from to_goal %.3f; goals = positions: largest component %.3f' % (from_goal.max(), pushed))
    assert from_goal.max() > 1e-3
    assert pushed > 1e-3
    if crowd == 'h5_mixed':  # the placeholders keep their goals whatever the map says
        assert cases.differs_from(tables[2], predict.to_goal(states[2], cases.N, 0.25)).max() > 1e-3
        parked = goals_cases.parked(state)
        assert parked.any() and not parked.all()
        assert all(_same(s[:, 1:, 4:6][parked], np.asarray(state)[:, 1:, 4:6][parked]) for s in states)
        assert (maps[:, 1][parked] != np.asarray(state)[:, 1:, 4:6][parked]).any()


# ------------------------------------------------------------------------------------------------ the C surface
DECLARATIONS = ('''int cn_predict_orca_goals(cn_engine* e, int n_steps, int n_modes,
                          const double* goals /* DEVICE [B][n_modes][A-1][2], 16-byte aligned */,
                          double* human_vel   /* DEVICE [B][n_modes][n_steps][A-1][2], 16-byte aligned */);''',
                'enum { CN_GOALS_ENGINE = 0, CN_GOALS_HEADING = 1 };',
                '''int cn_goal_hypotheses(cn_engine* e, int n_modes, int base, double reach, double std_heading, double std_distance,
                       int nominal_first, uint64_t seed, uint32_t counter,''')


def test_header_binding_and_library_agree(built):
    text = open(os.path.join(ROOT, 'include', 'crowdnav_amd.h')).read()
    for decl in DECLARATIONS:
        assert decl in text, decl
    assert 'no version bump: new symbols only' in text and '#define CN_ABI_VERSION 12' in text
    P = C.c_void_p
    assert built.SYMBOLS['cn_predict_orca_goals'] == (C.c_int, [P, C.c_int, C.c_int, P, P])
    assert built.SYMBOLS['cn_goal_hypotheses'] == (C.c_int, [P, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int,
                                                             C.c_uint64, C.c_uint32, P])
    assert (built.GOALS_ENGINE, built.GOALS_HEADING) == (0, 1) and built.GOALS_BASES == ('engine', 'heading')
    raw = C.CDLL(built.LIB_PATH)
    assert hasattr(raw, 'cn_predict_orca_goals') and hasattr(raw, 'cn_goal_hypotheses')
    assert built.load().cn_abi_version() == 12 == built.ABI_VERSION
    from crowdnav_amd import engine as E
    assert callable(E.BatchedCrowdSim.predict_orca_goals) and callable(E.BatchedCrowdSim.goal_hypotheses)
    assert 'human_v_pref * time_step * 12' in E.BatchedCrowdSim.goal_hypotheses.__doc__


def test_predict_orca_goals_refusals_in_order(built):
    lib = built.load()
    INV, UNS = built.CN_ERR_INVALID, built.CN_ERR_UNSUPPORTED

    def refused(args, word, status=INV):
        assert lib.cn_predict_orca_goals(*args) == status, (word, lib.cn_last_error())
        assert word in lib.cn_last_error().decode(), lib.cn_last_error()

    # (engine, n_steps, n_modes, goals, human_vel): each refusal with everything behind it wrong as well
    refused((None, -1, 0, None, None), 'cn_predict_orca_goals: goals is NULL')
    refused((None, 4, 2, None, DANGLING), 'cn_predict_orca_goals: goals is NULL')
    refused((None, -1, 0, DANGLING, None), 'cn_predict_orca_goals: human_vel is NULL')
    for m in (0, -3):
        refused((None, -1, m, DANGLING, DANGLING), 'cn_predict_orca_goals: n_modes must be >= 1 (got %d)' % m)
    refused((None, -1, 9, DANGLING, DANGLING), 'cn_predict_orca_goals: n_modes = 9 exceeds the 8 modes', UNS)
    refused((None, -1, 2, DANGLING, DANGLING), 'cn_predict_orca_goals: n_steps must be >= 0 (got -1)')
    refused((None, -5, 8, DANGLING, DANGLING), 'cn_predict_orca_goals: n_steps must be >= 0 (got -5)')
    # the engine — n_steps == 0 included: the checks come before the no-op
    refused((None, 4, 2, DANGLING, DANGLING), 'cn_predict_orca_goals: engine is NULL')
    refused((None, 0, 1, DANGLING, DANGLING), 'cn_predict_orca_goals: engine is NULL')


def test_goal_hypotheses_refusals_in_order(built):
    lib = built.load()
    INV, UNS = built.CN_ERR_INVALID, built.CN_ERR_UNSUPPORTED
    nan, inf = float('nan'), float('inf')

    def refused(args, word, status=INV):
        assert lib.cn_goal_hypotheses(*args) == status, (word, lib.cn_last_error())
        assert word in lib.cn_last_error().decode(), lib.cn_last_error()

    # (engine, n_modes, base, reach, std_heading, std_distance, nominal_first, seed, counter, goals)
    refused((None, 0, 7, -1.0, -1.0, -1.0, 1, 0, 0, None), 'cn_goal_hypotheses: goals is NULL')
    for m in (0, -3):
        refused((None, m, 7, -1.0, -1.0, -1.0, 1, 0, 0, DANGLING), 'cn_goal_hypotheses: n_modes must be >= 1 (got %d)' % m)
    refused((None, 9, 7, -1.0, -1.0, -1.0, 1, 0, 0, DANGLING), 'cn_goal_hypotheses: n_modes = 9 exceeds the 8 modes', UNS)
    for base in (2, -1, 7):
        refused((None, 8, base, -1.0, -1.0, -1.0, 1, 0, 0, DANGLING), 'cn_goal_hypotheses: base = %d unknown' % base)
    for reach in (0.0, -1.0, nan, inf):
        refused((None, 8, built.GOALS_HEADING, reach, -1.0, -1.0, 1, 0, 0, DANGLING), 'cn_goal_hypotheses: reach')
    for bad in (-0.5, nan, inf):
        # (reach is not read under CN_GOALS_ENGINE)
        refused((None, 8, built.GOALS_ENGINE, -1.0, bad, -1.0, 1, 0, 0, DANGLING), 'cn_goal_hypotheses: std_heading')
        refused((None, 8, built.GOALS_HEADING, 3.0, 0.4, bad, 1, 0, 0, DANGLING), 'cn_goal_hypotheses: std_distance')
    refused((None, 8, built.GOALS_ENGINE, nan, 0.0, 0.0, 1, 0, 0, DANGLING), 'cn_goal_hypotheses: engine is NULL')
    refused((None, 1, built.GOALS_HEADING, 3.0, 0.4, 0.3, 0, 2 ** 64 - 1, 2 ** 32 - 1, DANGLING), 'cn_goal_hypotheses: engine is NULL')
