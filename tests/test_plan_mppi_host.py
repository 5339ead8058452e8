"""The device MPPI update without a GPU: the C-ABI surface (three new symbols declared, bound and exported; struct layouts, ABI
version and launch counters as they were), the refusals that depend on the arguments alone — made with pointers that address
nothing, so a call that dereferenced one would crash here — and the numpy restatement on crafted scores whose weights are
exactly 0 or 1."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT

import plan_mppi_reference as mref
import plan_reference as ref
from support import built, host_cfg as _cfg, host_plan as _plan, NOWHERE  # noqa: F401  (built: module fixture)

SYMBOLS = ('cn_plan_mppi_update', 'cn_plan_mppi', 'cn_plan_mppi_rollout')
DECLARATIONS = (
    'int cn_plan_mppi_update(cn_engine* e, const cn_plan_cfg* cfg, const cn_plan* plan, double temperature, int fit_std, '
    'int keep_best);',
    'int cn_plan_mppi(cn_engine* e, const cn_plan_cfg* cfg, const cn_plan* plan, double temperature, int fit_std, '
    'uint32_t counter);',
    'int cn_plan_mppi_rollout(cn_engine* e, const cn_rollout_io* io, int n_real_steps, const cn_plan_cfg* cfg, '
    'const cn_plan* plan,\n                         double temperature, int fit_std, uint32_t counter);')
REQUIRED = ('mean', 'std', 'best_actions', 'best_score', 'action', 'candidates')
LOOK_REQUIRED = ('ret', 'info', 'steps', 'time')


def test_header_binding_and_library_agree(built):
    text = open(os.path.join(ROOT, 'include', 'crowdnav_amd.h')).read()
    for decl in DECLARATIONS:
        assert decl in text, decl
    assert '#define CN_ABI_VERSION 12' in text and '#define CN_LAUNCH_COUNTERS 6' in text  # additive; nothing new is counted
    P, cfg, plan, io = C.c_void_p, C.POINTER(built.CnPlanCfg), C.POINTER(built.CnPlan), C.POINTER(built.CnRolloutIo)
    want = {'cn_plan_mppi_update': [P, cfg, plan, C.c_double, C.c_int, C.c_int],
            'cn_plan_mppi': [P, cfg, plan, C.c_double, C.c_int, C.c_uint32],
            'cn_plan_mppi_rollout': [P, io, C.c_int, cfg, plan, C.c_double, C.c_int, C.c_uint32]}
    raw = C.CDLL(built.LIB_PATH)
    for name in SYMBOLS:
        res, args = built.SYMBOLS[name]
        assert res is C.c_int and args == want[name], name
        assert hasattr(raw, name), name
        assert getattr(built.load(), name).argtypes == args
    assert built.load().cn_abi_version() == 12 == built.ABI_VERSION and len(built.LAUNCH_COUNTERS) == 6
    assert C.sizeof(built.CnPlanCfg) == 56 and C.sizeof(built.CnPlan) == 120


def test_the_python_entry_points_exist(built):
    from crowdnav_amd.engine import BatchedCrowdSim
    for name in ('plan_mppi_update', 'plan_mppi', 'plan_mppi_rollout'):
        assert callable(getattr(BatchedCrowdSim, name)), name
    eng = BatchedCrowdSim.__new__(BatchedCrowdSim)  # no device: only what the methods check first
    eng.B, eng._h, eng._rollout = 3, None, None
    for call in (lambda: eng.plan_mppi(object(), 1.0, 0), lambda: eng.plan_mppi_update(None, 1.0),
                 lambda: eng.plan_mppi_update('plan', 1.0, fit_std=True, keep_best=True)):
        with pytest.raises(ValueError, match='plan_begin'):
            call()
    with pytest.raises(RuntimeError, match='rollout_begin'):
        eng.plan_mppi_rollout(object(), 1, 1.0, 0)
    eng._rollout = (None, None)
    with pytest.raises(ValueError, match='plan_begin'):
        eng.plan_mppi_rollout(object(), 1, 1.0, 0, fit_std=True)


def _calls(lib):
    """Every new entry point as f(e, cfg, plan, temperature): the other arguments address nothing."""
    L = lib.load()
    io = C.cast(NOWHERE, C.POINTER(lib.CnRolloutIo))
    return {'cn_plan_mppi_update': lambda e, c, p, T: L.cn_plan_mppi_update(e, c, p, T, 1, 1),
            'cn_plan_mppi': lambda e, c, p, T: L.cn_plan_mppi(e, c, p, T, 0, 3),
            'cn_plan_mppi_rollout': lambda e, c, p, T: L.cn_plan_mppi_rollout(e, io, 2, c, p, T, 1, 3)}


def test_refusals_that_need_no_engine_dereference_nothing(built):
    L = built.load()
    full = _plan(built)
    for name, call in _calls(built).items():
        def refused(e, cfg, plan, status, *words, T=1.0):
            assert call(e, cfg, plan, T) == status, (name, L.cn_last_error())
            text = L.cn_last_error().decode()
            assert (name + ':') in text and all(w in text for w in words), text

        INV, UNS = built.CN_ERR_INVALID, built.CN_ERR_UNSUPPORTED
        good = C.byref(_cfg(built))
        # 1. NULL cfg, plan, a required array — the name speaks, the engine is not looked at
        refused(NOWHERE, None, C.byref(full), INV, 'cfg is NULL')
        refused(None, None, None, INV, 'cfg is NULL', T=0.0)
        refused(NOWHERE, good, None, INV, 'plan is NULL')
        for k in REQUIRED:
            refused(NOWHERE, good, C.byref(_plan(built, **{k: None})), INV, 'plan->' + k)
        for k in LOOK_REQUIRED:
            refused(NOWHERE, good, C.byref(_plan(built, look_missing=(k,))), INV, 'plan->look.' + k)
        boot = C.byref(_cfg(built, bootstrap=1))
        refused(NOWHERE, boot, C.byref(_plan(built, look_missing=('final_state8',))), INV, 'look.final_state8')
        refused(NOWHERE, boot, C.byref(_plan(built, value=None)), INV, 'plan->value')
        refused(NOWHERE, boot, C.byref(_plan(built, score=None)), INV, 'plan->score')
        refused(NOWHERE, C.byref(_cfg(built, n_steps=0)), C.byref(_plan(built, mean=None)), INV, 'plan->mean', T=-1.0)
        bare = _plan(built, look_missing=('final_state8', 'final_theta'), value=None, score=None, order=None)
        refused(None, good, C.byref(bare), INV, 'engine is NULL')
        # 2. ranges — n_elites is checked although the update does not read it
        p = C.byref(full)
        refused(NOWHERE, C.byref(_cfg(built, n_steps=0)), p, INV, 'n_steps', '0')
        refused(NOWHERE, C.byref(_cfg(built, n_steps=257)), p, UNS, 'n_steps', '257')
        refused(NOWHERE, C.byref(_cfg(built, n_candidates=1)), p, INV, 'n_candidates', '1')
        refused(NOWHERE, C.byref(_cfg(built, n_candidates=1025, n_elites=64)), p, UNS, 'n_candidates', '1025')
        refused(NOWHERE, C.byref(_cfg(built, n_elites=0)), p, INV, 'n_elites', '0')
        refused(NOWHERE, C.byref(_cfg(built, n_candidates=100, n_elites=65)), p, UNS, 'n_elites', '65')
        refused(NOWHERE, C.byref(_cfg(built, n_elites=6)), p, INV, 'n_elites', '6')  # E > K = 5
        refused(NOWHERE, C.byref(_cfg(built, iterations=0)), p, INV, 'iterations')
        for bad in (0.0, -1.0, float('inf'), float('nan')):
            refused(NOWHERE, C.byref(_cfg(built, init_std=bad)), p, INV, 'init_std')
        for bad in (-1e-9, float('inf'), float('nan')):
            refused(NOWHERE, C.byref(_cfg(built, min_std=bad)), p, INV, 'min_std')
        for bad in (-0.1, 1.0, float('nan')):
            refused(NOWHERE, C.byref(_cfg(built, smoothing=bad)), p, INV, 'smoothing')
        # 3. the temperature: after a bad range, before the engine — NULL or not — is looked at
        for bad in (0.0, -1.0, float('inf'), float('nan')):
            refused(NOWHERE, good, p, INV, 'temperature', T=bad)
            refused(None, good, p, INV, 'temperature', T=bad)
            refused(NOWHERE, C.byref(_cfg(built, smoothing=1.0)), p, INV, 'smoothing', T=bad)
            refused(NOWHERE, C.byref(_cfg(built, n_steps=257)), p, UNS, 'n_steps', T=bad)
        # 4. NULL engine, after everything above
        refused(None, good, p, INV, 'engine is NULL')
        refused(None, good, p, INV, 'engine is NULL', T=1e-300)
        refused(None, C.byref(_cfg(built, n_candidates=1024, n_elites=64, n_steps=256, smoothing=0.999)), p, INV, 'engine is NULL')


# ------------------------------------------------------------------------------------------------ the restatement
def _crafted(K=6, seed=0):
    """One env, n = 2: candidate rows inside the unit disc that no sum of a few of them represents exactly."""
    rng = np.random.RandomState(seed)
    cand = rng.uniform(-0.6, 0.6, (1, K, 2, 2))
    zeros = np.zeros((1, 2, 2))
    return cand, zeros


def _update(scores, cand, mean, std, **kw):
    B, n = cand.shape[0], cand.shape[2]
    args = dict(best_actions=np.zeros((B, n, 2)), best_score=np.full(B, -np.inf), action=np.zeros((B, 2)), temperature=1.0,
                fit_std=False, keep_best=False, smoothing=0.0, min_std=0.0, v_pref=1.0)
    args.update(kw)
    return mref.mppi_update(np.asarray(scores, np.float64), cand, mean, std, **args)


def _sequential_mean(rows):
    total = np.zeros_like(rows[0])
    for r in rows:
        total = total + r
    return total / np.float64(len(rows))


def test_equal_scores_give_the_plain_sequential_mean():
    cand, zeros = _crafted()
    w, Z, top = mref.weights(np.full(6, 0.25), 0.05)
    assert (w == 1.0).all() and Z == 6.0 and top == 0
    out = _update(np.full((1, 6), 0.25), cand, zeros + 9.0, zeros + 3.0, temperature=0.05)
    assert out['order'].tolist() == [list(range(6))]
    assert np.array_equal(out['mean'][0], _sequential_mean(cand[0]))
    assert np.array_equal(out['std'], zeros + 3.0)  # fit_std = 0: untouched
    assert np.array_equal(out['best_actions'][0], cand[0, 0]) and out['best_score'].tolist() == [0.25]
    assert np.array_equal(out['action'][0], out['mean'][0, 0])  # inside the disc: not clipped, and not the best row's
    assert not np.array_equal(out['action'][0], out['best_actions'][0, 0])


def test_one_dominant_score_gives_its_row_bit_for_bit():
    cand, zeros = _crafted()
    scores = np.array([[-1e6, -1e6, 0.0, -1e6, -2e6, -1e6]])
    w, Z, top = mref.weights(scores[0], 1.0)
    assert w.tolist() == [0.0, 0.0, 1.0, 0.0, 0.0, 0.0] and Z == 1.0 and top == 2
    std0 = zeros + 3.0
    out = _update(scores, cand, zeros, std0, fit_std=True, min_std=0.125)
    assert np.array_equal(out['mean'][0], cand[0, 2]) and np.array_equal(out['action'][0], cand[0, 2, 0])
    assert (out['std'] == 0.125).all()  # sd == 0 exactly: the floor binds
    assert np.array_equal(_update(scores, cand, zeros, std0, fit_std=True)['std'], zeros)
    assert _update(scores, cand, zeros, std0)['std'].tobytes() == std0.tobytes()  # fit_std = 0: std bitwise unchanged
    # the issue's own pattern: (0, -1e6, ...)
    lead = _update(np.array([[0.0] + [-1e6] * 5]), cand, zeros, std0, fit_std=True, min_std=0.125)
    assert np.array_equal(lead['mean'][0], cand[0, 0]) and (lead['std'] == 0.125).all() and lead['order'][0, 0] == 0


def test_a_tie_at_the_top_weights_both_and_takes_the_lower_index():
    cand, zeros = _crafted()
    scores = np.array([[-1e6, 3.0, -1e6, -1e6, 3.0, -1e6]])
    w, Z, top = mref.weights(scores[0], 1.0)
    assert w.tolist() == [0.0, 1.0, 0.0, 0.0, 1.0, 0.0] and Z == 2.0 and top == 1
    out = _update(scores, cand, zeros, zeros, fit_std=True)
    assert out['order'][0].tolist() == [1, 4, 0, 2, 3, 5]
    assert np.array_equal(out['best_actions'][0], cand[0, 1]) and out['best_score'].tolist() == [3.0]
    m = (cand[0, 1] + cand[0, 4]) / 2.0
    d1, d4 = cand[0, 1] - m, cand[0, 4] - m
    assert np.array_equal(out['mean'][0], m)
    assert np.array_equal(out['std'][0], np.sqrt((d1 * d1 + d4 * d4) / 2.0))


def test_smoothing_keep_best_and_the_action_clip():
    cand, zeros = _crafted()
    scores = np.array([[1.0, 3.0, 3.0, -2.0, 1.0, 3.0]])
    plain = _update(scores, cand, zeros, zeros, fit_std=True)
    mean0, std0 = zeros + 0.25, zeros + 2.0
    sm = _update(scores, cand, mean0, std0, fit_std=True, smoothing=0.5, min_std=0.01)
    assert np.array_equal(sm['mean'], 0.5 * mean0 + 0.5 * plain['mean'])
    assert np.array_equal(sm['std'], np.maximum(0.01, 0.5 * std0 + 0.5 * plain['std']))
    # the weights against a direct statement: three of 1, two of exp(-2), one of exp(-5), summed in index order
    w, Z, top = mref.weights(scores[0], 1.0)
    assert top == 1 and w[1] == w[2] == w[5] == 1.0 and w[0] == w[4] == np.exp(-2.0) and w[3] == np.exp(-5.0)
    assert Z == ((((w[0] + 1.0) + 1.0) + w[3]) + w[4]) + 1.0
    # keep_best is strict: an equal score does not replace what is held; a better one does; without keep_best it always does
    held = dict(best_actions=zeros + 7.0, best_score=np.array([3.0]), action=np.full((1, 2), 7.0))
    kept = _update(scores, cand, zeros, zeros, keep_best=True, **held)
    assert np.array_equal(kept['best_actions'], held['best_actions']) and kept['best_score'].tolist() == [3.0]
    assert np.array_equal(kept['action'], plain['action'])  # ... the action is the mean's whatever is held
    taken = _update(scores, cand, zeros, zeros, keep_best=False, **held)
    assert np.array_equal(taken['best_actions'][0], cand[0, 1])
    better = _update(scores, cand, zeros, zeros, keep_best=True, **dict(held, best_score=np.array([2.5])))
    assert np.array_equal(better['best_actions'][0], cand[0, 1]) and better['best_score'].tolist() == [3.0]
    # the clip: candidates lie inside the disc, so only a prior mean outside it, kept by smoothing, can push mean[0] out
    far = zeros.copy()
    far[0, 0] = (30.0, -40.0)
    out = _update(scores, cand, far, zeros, smoothing=0.5, v_pref=1.0)
    row = out['mean'][0, 0]
    nrm = np.sqrt(row[0] * row[0] + row[1] * row[1])
    assert nrm > 1.0 and np.array_equal(out['action'][0], row * (1.0 / nrm))
    assert abs(np.hypot(*out['action'][0]) - 1.0) < 1e-15 and np.array_equal(out['mean'][0, 0], 0.5 * far[0, 0] + 0.5 * plain['mean'][0, 0])
    half = _update(scores, cand, far, zeros, smoothing=0.5, v_pref=np.array([0.5]))
    assert np.array_equal(half['action'][0], row * (0.5 / nrm))
    assert np.array_equal(ref.clip(row, 1.0), out['action'][0])
