"""The device CEM planner without a GPU: the Philox restatement against the known-answer vectors, the C-ABI surface (declared,
bound, exported, struct layouts, no version bump, no new counter), the refusals that depend on the arguments alone — made with
pointers that address nothing, so a call that dereferenced one would crash here — and the refit restatement on crafted ties."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import plan_reference as ref
from support import built, host_cfg as _cfg, host_plan as _plan, NOWHERE  # noqa: F401  (built: module fixture)

SYMBOLS = ('cn_plan_reset', 'cn_plan_draw', 'cn_plan_refit', 'cn_plan_cem', 'cn_plan_shift', 'cn_plan_rollout')
DECLARATIONS = (
    'int cn_plan_reset(cn_engine* e, const cn_plan_cfg* cfg, const cn_plan* plan, const uint8_t* mask',
    'int cn_plan_draw(cn_engine* e, const cn_plan_cfg* cfg, const cn_plan* plan, uint32_t counter);',
    'int cn_plan_refit(cn_engine* e, const cn_plan_cfg* cfg, const cn_plan* plan, int keep_best);',
    'int cn_plan_cem(cn_engine* e, const cn_plan_cfg* cfg, const cn_plan* plan, uint32_t counter);',
    'int cn_plan_shift(cn_engine* e, const cn_rollout_io* io, const cn_plan_cfg* cfg, const cn_plan* plan);',
    'int cn_plan_rollout(cn_engine* e, const cn_rollout_io* io, int n_real_steps, const cn_plan_cfg* cfg, const cn_plan* plan,\n'
    '                    uint32_t counter);')
CFG_FIELDS = [('n_steps', 'int32_t'), ('n_candidates', 'int32_t'), ('n_elites', 'int32_t'), ('iterations', 'int32_t'),
              ('bootstrap', 'int32_t'), ('sort_humans', 'int32_t'), ('init_std', 'double'), ('min_std', 'double'),
              ('smoothing', 'double'), ('seed', 'uint64_t')]
PLAN_FIELDS = [('mean', 'double*'), ('std', 'double*'), ('best_actions', 'double*'), ('best_score', 'double*'),
               ('action', 'double*'), ('candidates', 'double*'), ('look', 'cn_lookahead_out'), ('value', 'float*'),
               ('score', 'double*'), ('order', 'int32_t*')]
REQUIRED = ('mean', 'std', 'best_actions', 'best_score', 'action', 'candidates')
LOOK_REQUIRED = ('ret', 'info', 'steps', 'time')


def _words(text):
    return [int(w, 16) for w in text.split()]


@pytest.mark.parametrize('counter, key, want', [
    ('0 0 0 0', '0 0', '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
    ('ffffffff ffffffff ffffffff ffffffff', 'ffffffff ffffffff', '408f276d 41c83b0e a20bc7c6 6d5451fd'),
    ('243f6a88 85a308d3 13198a2e 03707344', 'a4093822 299f31d0', 'd16cfe09 94fdcceb 5001e420 24126ea1')])
def test_philox_known_answers(counter, key, want):
    got = ref.philox4x32_10(np.array(_words(counter), np.uint32), np.array(_words(key), np.uint32))
    assert got.dtype == np.uint32 and got.tolist() == _words(want)


def test_philox_broadcasts_and_the_uniforms_stay_inside_their_intervals():
    ctr = np.array([_words('0 0 0 0'), _words('243f6a88 85a308d3 13198a2e 03707344')], np.uint32)
    key = np.array([_words('0 0'), _words('a4093822 299f31d0')], np.uint32)
    got = ref.philox4x32_10(ctr, key)
    assert got[0].tolist() == _words('6627e8d5 e169c58d bc57ac4c 9b00dbd8')
    assert got[1].tolist() == _words('d16cfe09 94fdcceb 5001e420 24126ea1')
    z0, z1, r = ref.normal_pairs(2, 3, 4, seed=(5 << 32) | 7, counter=9)
    assert z0.shape == (2, 3, 4) and np.isfinite(z0).all() and np.isfinite(z1).all() and (r >= 0).all()
    # a row does not depend on B, K or n
    y0, y1, _ = ref.normal_pairs(3, 5, 6, seed=(5 << 32) | 7, counter=9)
    assert np.array_equal(z0, y0[:2, :3, :4]) and np.array_equal(z1, y1[:2, :3, :4])


def _struct_fields(text, name):
    body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (name, name), text, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    out = []
    for decl in body.split(';'):
        decl = decl.strip()
        if decl:
            typ, field = decl.rsplit(None, 1)
            out.append((field, ''.join(typ.split())))
    return out


def test_header_binding_and_library_agree(built):
    text = open(os.path.join(ROOT, 'include', 'crowdnav_amd.h')).read()
    for decl in DECLARATIONS:
        assert decl in text, decl
    assert '#define CN_ABI_VERSION 12' in text and '#define CN_LAUNCH_COUNTERS 6' in text  # additive; nothing new is counted
    P, cfg, plan, io = C.c_void_p, C.POINTER(built.CnPlanCfg), C.POINTER(built.CnPlan), C.POINTER(built.CnRolloutIo)
    want = {'cn_plan_reset': [P, cfg, plan, P], 'cn_plan_draw': [P, cfg, plan, C.c_uint32],
            'cn_plan_refit': [P, cfg, plan, C.c_int], 'cn_plan_cem': [P, cfg, plan, C.c_uint32],
            'cn_plan_shift': [P, io, cfg, plan], 'cn_plan_rollout': [P, io, C.c_int, cfg, plan, C.c_uint32]}
    raw = C.CDLL(built.LIB_PATH)
    for name in SYMBOLS:
        res, args = built.SYMBOLS[name]
        assert res is C.c_int and args == want[name], name
        assert hasattr(raw, name), name
        assert getattr(built.load(), name).argtypes == args
    assert built.load().cn_abi_version() == 12 == built.ABI_VERSION and len(built.LAUNCH_COUNTERS) == 6
    # both struct layouts: names and order from the header, C types by name
    ctype = {'int32_t': C.c_int32, 'double': C.c_double, 'uint64_t': C.c_uint64, 'double*': C.c_void_p, 'float*': C.c_void_p,
             'int32_t*': C.c_void_p, 'cn_lookahead_out': built.CnLookaheadOut}
    assert _struct_fields(text, 'cn_plan_cfg') == CFG_FIELDS
    assert _struct_fields(text, 'cn_plan') == PLAN_FIELDS
    assert [(n, t) for n, t in built.CnPlanCfg._fields_] == [(n, ctype[t]) for n, t in CFG_FIELDS]
    assert [(n, t) for n, t in built.CnPlan._fields_] == [(n, ctype[t]) for n, t in PLAN_FIELDS]
    assert C.sizeof(built.CnPlanCfg) == 56 and built.CnPlanCfg.init_std.offset == 24 and built.CnPlanCfg.seed.offset == 48
    assert C.sizeof(built.CnPlan) == 120 and built.CnPlan.look.offset == 48 and built.CnPlan.value.offset == 96


def test_the_python_entry_points_exist(built):
    from crowdnav_amd.engine import BatchedCrowdSim, Plan
    for name in ('plan_begin', 'plan_reset', 'plan_draw', 'plan_refit', 'plan_cem', 'plan_shift', 'plan_rollout'):
        assert callable(getattr(BatchedCrowdSim, name)), name
    eng = BatchedCrowdSim.__new__(BatchedCrowdSim)  # no device: only what the methods check first
    eng.B, eng._h, eng._rollout = 3, None, None
    with pytest.raises(ValueError, match='K and n'):
        eng.plan_begin(0, 4, 1, 1, 0.5)
    for call in (lambda: eng.plan_cem(object(), 0), lambda: eng.plan_draw(None, 0), lambda: eng.plan_refit('plan')):
        with pytest.raises(ValueError, match='plan_begin'):
            call()
    with pytest.raises(RuntimeError, match='rollout_begin'):
        eng.plan_rollout(object(), 1, 0)
    assert callable(Plan.tensors)


def _calls(lib):
    """Every entry point as f(e, cfg, plan): the other arguments address nothing."""
    L = lib.load()
    io = C.cast(NOWHERE, C.POINTER(lib.CnRolloutIo))
    return {'cn_plan_reset': lambda e, c, p: L.cn_plan_reset(e, c, p, NOWHERE),
            'cn_plan_draw': lambda e, c, p: L.cn_plan_draw(e, c, p, 3),
            'cn_plan_refit': lambda e, c, p: L.cn_plan_refit(e, c, p, 1),
            'cn_plan_cem': lambda e, c, p: L.cn_plan_cem(e, c, p, 3),
            'cn_plan_shift': lambda e, c, p: L.cn_plan_shift(e, io, c, p),
            'cn_plan_rollout': lambda e, c, p: L.cn_plan_rollout(e, io, 2, c, p, 3)}


def test_refusals_that_need_no_engine_dereference_nothing(built):
    L = built.load()
    full = _plan(built)
    for name, call in _calls(built).items():
        def refused(e, cfg, plan, status, *words):
            assert call(e, cfg, plan) == status, (name, L.cn_last_error())
            text = L.cn_last_error().decode()
            assert name in text and all(w in text for w in words), text

        INV, UNS = built.CN_ERR_INVALID, built.CN_ERR_UNSUPPORTED
        good = C.byref(_cfg(built))
        # 1. NULL cfg, plan, a required array — the name speaks, the engine is not looked at
        refused(NOWHERE, None, C.byref(full), INV, 'cfg is NULL')
        refused(None, None, None, INV, 'cfg is NULL')
        refused(NOWHERE, good, None, INV, 'plan is NULL')
        for k in REQUIRED:
            refused(NOWHERE, good, C.byref(_plan(built, **{k: None})), INV, 'plan->' + k)
        for k in LOOK_REQUIRED:
            refused(NOWHERE, good, C.byref(_plan(built, look_missing=(k,))), INV, 'plan->look.' + k)
        boot = C.byref(_cfg(built, bootstrap=1))
        refused(NOWHERE, boot, C.byref(_plan(built, look_missing=('final_state8',))), INV, 'look.final_state8')
        refused(NOWHERE, boot, C.byref(_plan(built, value=None)), INV, 'plan->value')
        refused(NOWHERE, boot, C.byref(_plan(built, score=None)), INV, 'plan->score')
        # ... a missing array is named before a bad range
        refused(NOWHERE, C.byref(_cfg(built, n_steps=0)), C.byref(_plan(built, mean=None)), INV, 'plan->mean')
        # the optional ones may be NULL: the next check speaks (here: the engine)
        bare = _plan(built, look_missing=('final_state8', 'final_theta'), value=None, score=None, order=None)
        refused(None, good, C.byref(bare), INV, 'engine is NULL')
        # 2. ranges
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
        # 3. NULL engine, after everything above
        refused(None, good, p, INV, 'engine is NULL')
        refused(None, C.byref(_cfg(built, n_candidates=1024, n_elites=64, n_steps=256, smoothing=0.999)), p, INV, 'engine is NULL')


def _crafted():
    """One env, K = 6, n = 2: scores with two exact ties; candidate k's rows are (k, 10 k), (100 k, 1000 k)."""
    scores = np.array([[1.0, 3.0, 3.0, -2.0, 1.0, 3.0]])
    cand = np.zeros((1, 6, 2, 2))
    for k in range(6):
        cand[0, k] = [[k, 10.0 * k], [100.0 * k, 1000.0 * k]]
    zeros = np.zeros((1, 2, 2))
    return scores, cand, zeros


def test_refit_restatement_ties_pick_the_lower_index():
    scores, cand, zeros = _crafted()
    assert ref.ranks(scores[0]).tolist() == [3, 0, 1, 5, 4, 2]
    out = ref.refit(scores, cand, zeros, zeros + 1.0, zeros, np.array([-np.inf]), np.zeros((1, 2)), E=2, keep_best=False,
                    smoothing=0.0, min_std=0.0)
    assert out['order'].tolist() == [[1, 2, 5, 0, 4, 3]]
    assert out['best_score'].tolist() == [3.0] and np.array_equal(out['best_actions'][0], cand[0, 1])
    assert out['action'].tolist() == [[1.0, 10.0]]
    assert np.array_equal(out['mean'][0], (cand[0, 1] + cand[0, 2]) / 2.0)  # the elites are k = 1 and 2, not 5
    assert np.array_equal(out['std'][0], np.abs(cand[0, 1] - cand[0, 2]) / 2.0)
    # all scores equal: the order is the index order
    same = ref.refit(np.full((1, 6), 0.25), cand, zeros, zeros, zeros, np.array([0.0]), np.zeros((1, 2)), E=1, keep_best=False,
                     smoothing=0.0, min_std=0.0)
    assert same['order'].tolist() == [list(range(6))] and not same['mean'].any() and not same['std'].any()


def test_refit_restatement_keep_best_smoothing_and_the_plain_mean():
    scores, cand, zeros = _crafted()
    held = dict(best_actions=zeros + 7.0, best_score=np.array([3.0]), action=np.full((1, 2), 7.0))
    # keep_best is strict: an equal score does not replace what is held; without it, it does
    kept = ref.refit(scores, cand, zeros, zeros, E=6, keep_best=True, smoothing=0.0, min_std=0.0, **held)
    assert np.array_equal(kept['best_actions'], held['best_actions']) and kept['action'].tolist() == [[7.0, 7.0]]
    taken = ref.refit(scores, cand, zeros, zeros, E=6, keep_best=False, smoothing=0.0, min_std=0.0, **held)
    assert np.array_equal(taken['best_actions'][0], cand[0, 1])
    better = ref.refit(scores, cand, zeros, zeros, E=6, keep_best=True, smoothing=0.0, min_std=0.0,
                       **dict(held, best_score=np.array([2.5])))
    assert np.array_equal(better['best_actions'][0], cand[0, 1]) and better['best_score'].tolist() == [3.0]
    # E = K: the plain mean and the population deviation, whatever the order (these sums are exact)
    assert np.array_equal(kept['mean'][0], cand[0].mean(axis=0)) and np.allclose(kept['std'][0], cand[0].std(axis=0), rtol=1e-15)
    # smoothing and a binding min_std
    mean0, std0 = zeros + 4.0, zeros + 2.0
    sm = ref.refit(scores, cand, mean0, std0, E=6, keep_best=False, smoothing=0.5, min_std=1e4, **held)
    assert np.array_equal(sm['mean'], 0.5 * mean0 + 0.5 * kept['mean'])
    assert np.array_equal(sm['std'], np.maximum(1e4, 0.5 * std0 + 0.5 * kept['std'])) and (sm['std'] == 1e4).any()


def test_prior_and_shift_restatement():
    state = np.zeros((3, 2, 8))
    state[:, 0, 7] = 1.0
    state[0, 0, :2], state[0, 0, 4:6] = (0.0, -4.0), (0.0, 4.0)   # 8 m below its goal: full speed up
    state[1, 0, :2], state[1, 0, 4:6] = (1.0, 1.0), (1.0, 1.0)    # at its goal
    state[2, 0, :2], state[2, 0, 4:6] = (0.0, 0.0), (0.1, 0.0)    # 0.1 m away: what reaches it in one step
    assert ref.prior(state, 0.25).tolist() == [[0.0, 1.0], [0.0, 0.0], [0.4, 0.0]]
    mean = np.arange(3 * 4 * 2, dtype=np.float64).reshape(3, 4, 2)
    std = np.full((3, 4, 2), 9.0)
    m, s = ref.shift(state, 0.25, active=[1, 0, 1], cur_steps=[3, 0, 0], mean=mean, std=std, init_std=0.5)
    assert np.array_equal(m[0], np.concatenate([mean[0, 1:], mean[0, -1:]])) and (s[0] == 0.5).all()
    assert np.array_equal(m[1], mean[1]) and (s[1] == 9.0).all()  # retired: untouched
    assert (m[2] == [0.4, 0.0]).all() and (s[2] == 0.5).all()     # re-seeded
    m, s = ref.reset(state, 0.25, mean, std, 0.5, mask=[0, 1, 0])
    assert np.array_equal(m[0], mean[0]) and not m[1].any() and (s[1] == 0.5).all() and (s[2] == 9.0).all()
