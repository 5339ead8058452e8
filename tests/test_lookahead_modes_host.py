"""Lookahead under several predicted futures without a GPU: the C-ABI surface (declared, bound, exported, no version bump, no
existing struct touched), the refusals that need no engine (made with pointers that address nothing: a refusal reads none of
them), the python entry points' own checks, predict.stack_modes, the reduction of the host restatement
(lookahead_modes_reference.py) on crafted per-mode results, and — on that restatement — what the cases of
test_lookahead_modes.py must contain for its comparisons to mean something."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from conftest import ROOT

import lookahead_modes_reference as ref
from support import built, DANGLING, filled  # noqa: F401  (built: module fixture)

DECLARATIONS = ('enum { CN_MODES_MEAN = 0, CN_MODES_MIN = 1 };',
                '''int cn_lookahead_modes(cn_engine* e, int n_steps, int n_candidates, const double* actions /* [B][K][n][2] */,
                       const cn_path_modes* modes, const cn_modes_out* out);''',
                'int cn_plan_cem_modes (cn_engine* e, const cn_plan_cfg* cfg, const cn_plan* plan, const cn_path_modes* modes, uint32_t counter);',
                '''int cn_plan_mppi_modes(cn_engine* e, const cn_plan_cfg* cfg, const cn_plan* plan, const cn_path_modes* modes,
                       double temperature, int fit_std, uint32_t counter);''')
NAMES = ('cn_lookahead_modes', 'cn_plan_cem_modes', 'cn_plan_mppi_modes')


def test_header_binding_and_library_agree(built):
    text = open(os.path.join(ROOT, 'include', 'crowdnav_amd.h')).read()
    for decl in DECLARATIONS:
        assert decl in text, decl
    assert text.index('Lookahead under predicted human motion') < text.index('Lookahead under several predicted futures') < text.index(
        'Value-bootstrapped lookahead')
    assert '#define CN_ABI_VERSION 12' in text and '#define CN_LAUNCH_COUNTERS 6' in text
    # the structs, field for field in the header's order
    for struct, cls in (('cn_path_modes', built.CnPathModes), ('cn_modes_out', built.CnModesOut)):
        body = text[text.index('typedef struct %s {' % struct):text.index('} %s;' % struct)]
        declared = [line.split(';')[0].split()[-1].lstrip('*') for line in body.splitlines()[1:] if ';' in line]
        assert declared == [name for name, _ in cls._fields_], (struct, declared)
    assert C.sizeof(built.CnPathModes) == 32 and C.sizeof(built.CnModesOut) == 80
    assert built.CnPathModes.risk_penalty.offset == 8 and built.CnPathModes.human_vel.offset == 16
    P, cfg, plan = C.c_void_p, C.POINTER(built.CnPlanCfg), C.POINTER(built.CnPlan)
    modes, out = C.POINTER(built.CnPathModes), C.POINTER(built.CnModesOut)
    assert built.SYMBOLS['cn_lookahead_modes'] == (C.c_int, [P, C.c_int, C.c_int, P, modes, out])
    assert built.SYMBOLS['cn_plan_cem_modes'] == (C.c_int, [P, cfg, plan, modes, C.c_uint32])
    assert built.SYMBOLS['cn_plan_mppi_modes'] == (C.c_int, [P, cfg, plan, modes, C.c_double, C.c_int, C.c_uint32])
    raw = C.CDLL(built.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
    assert not hasattr(raw, 'cn_plan_cem_modes_rollout') and not hasattr(raw, 'cn_lookahead_modes_values')
    assert (built.MODES_MEAN, built.MODES_MIN) == (0, 1) and built.MODES_REDUCE == ('mean', 'min') and built.MODES_MAX == 8
    # nothing that existed moved
    assert built.load().cn_abi_version() == 12 == built.ABI_VERSION and len(built.LAUNCH_COUNTERS) == 6
    assert C.sizeof(built.CnLookaheadOut) == 48 and C.sizeof(built.CnPlanCfg) == 56 and C.sizeof(built.CnPlan) == 120


def _modes(built, **fields):
    base = dict(n_modes=3, reduce=built.MODES_MEAN, risk_penalty=0.5, human_vel=DANGLING, weight=DANGLING)
    base.update(fields)
    return built.CnPathModes(**base)


def _out(built, **fields):
    return filled(built.CnModesOut, DANGLING, **fields)


def test_lookahead_refusals_that_need_no_engine(built):
    lib = built.load()
    call, n, K = lib.cn_lookahead_modes, 4, 3
    ok_m, ok_o = _modes(built), _out(built)

    def refused(args, word, status=built.CN_ERR_INVALID):
        assert call(*args) == status, (word, lib.cn_last_error())
        assert word in lib.cn_last_error().decode(), lib.cn_last_error()

    # 1. the four pointers, before everything beside them
    refused((None, -1, 0, None, None, None), 'cn_lookahead_modes: modes is NULL')
    refused((None, n, K, DANGLING, None, C.byref(ok_o)), 'cn_lookahead_modes: modes is NULL')
    refused((None, -1, 0, None, C.byref(_modes(built, human_vel=None, n_modes=0)), None), 'cn_lookahead_modes: modes->human_vel is NULL')
    refused((None, -1, 0, None, C.byref(_modes(built, n_modes=0)), None), 'cn_lookahead_modes: out is NULL')
    refused((None, -1, 0, None, C.byref(_modes(built, n_modes=0)), C.byref(_out(built, score=None))), 'cn_lookahead_modes: out->score is NULL')
    # 2. n_modes
    for m in (0, -2):
        refused((None, -1, 0, None, C.byref(_modes(built, n_modes=m, reduce=7)), C.byref(ok_o)), 'n_modes must be >= 1 (got %d)' % m)
    refused((None, -1, 0, None, C.byref(_modes(built, n_modes=9, reduce=7)), C.byref(ok_o)), 'n_modes = 9 exceeds the 8 modes',
            built.CN_ERR_UNSUPPORTED)
    # 3. reduce, 4. risk_penalty
    refused((None, -1, 0, None, C.byref(_modes(built, n_modes=8, reduce=2, risk_penalty=-1.0)), C.byref(ok_o)), 'reduce 2 unknown')
    refused((None, -1, 0, None, C.byref(_modes(built, reduce=-1)), C.byref(ok_o)), 'reduce -1 unknown')
    for bad in (-0.5, float('inf'), float('nan')):
        refused((None, -1, 0, None, C.byref(_modes(built, reduce=built.MODES_MIN, risk_penalty=bad)), C.byref(ok_o)),
                'risk_penalty must be >= 0 and finite')
    # 5. cn_lookahead_actions' own for (n_steps, K, actions), in its order and with its messages; only `score` is required of out
    bare = _out(built, **{name: None for name, _ in built.CnModesOut._fields_ if name != 'score'})
    no_w = _modes(built, weight=None, risk_penalty=0.0)
    for m, o in ((ok_m, ok_o), (no_w, bare)):
        refused((None, -1, 0, None, C.byref(m), C.byref(o)), 'cn_lookahead_actions: actions is NULL')
        refused((None, -1, 0, DANGLING, C.byref(m), C.byref(o)), 'cn_lookahead_actions: n_steps must be >= 0 (got -1)')
        refused((None, n, 0, DANGLING, C.byref(m), C.byref(o)), 'cn_lookahead_actions: n_candidates must be >= 1 (got 0)')
        # the NULL engine, last of what needs no engine (n_steps == 0 included: the checks come before the no-op)
        refused((None, n, K, DANGLING, C.byref(m), C.byref(o)), 'cn_lookahead_actions: engine is NULL')
        refused((None, 0, K, DANGLING, C.byref(m), C.byref(o)), 'cn_lookahead_actions: engine is NULL')


def test_plan_refusals_that_need_no_engine(built):
    lib = built.load()
    look = built.CnLookaheadOut(ret=DANGLING, info=DANGLING, steps=DANGLING, time=DANGLING, final_state8=DANGLING, final_theta=DANGLING)
    cfg = built.CnPlanCfg(n_steps=4, n_candidates=5, n_elites=2, iterations=1, bootstrap=0, sort_humans=0, init_std=0.3,
                          min_std=0.0, smoothing=0.0, seed=1)
    plan = built.CnPlan(mean=DANGLING, std=DANGLING, best_actions=DANGLING, best_score=DANGLING, action=DANGLING,
                        candidates=DANGLING, look=look, value=DANGLING, score=DANGLING, order=DANGLING)
    no_mean = built.CnPlan.from_buffer_copy(plan)
    no_mean.mean = None
    modes, bad_modes = _modes(built), _modes(built, n_modes=0)
    calls = {'cn_plan_cem_modes': lambda c, p, m, temperature=0.7: lib.cn_plan_cem_modes(None, c, p, m, 21),
             'cn_plan_mppi_modes': lambda c, p, m, temperature=0.7: lib.cn_plan_mppi_modes(None, c, p, m, temperature, 0, 21)}
    for name, call in calls.items():
        for args, word in (((None, None, None), name + ': modes is NULL'),
                           ((C.byref(cfg), C.byref(plan), None), name + ': modes is NULL'),
                           ((None, C.byref(plan), C.byref(modes)), name + ': cfg is NULL'),
                           ((C.byref(cfg), None, C.byref(modes)), name + ': plan is NULL'),
                           ((C.byref(cfg), C.byref(no_mean), C.byref(modes)), name + ': plan->mean is NULL'),
                           # the planners' own refusals come before cn_lookahead_modes': a bad n_modes is not looked at yet
                           ((C.byref(cfg), C.byref(plan), C.byref(bad_modes)), name + ': engine is NULL')):
            assert call(*args) == built.CN_ERR_INVALID, (name, word)
            assert word in lib.cn_last_error().decode(), lib.cn_last_error()
        few = built.CnPlanCfg.from_buffer_copy(cfg)
        few.n_candidates = 1
        assert call(C.byref(few), C.byref(plan), C.byref(modes)) == built.CN_ERR_INVALID
        assert name + ': n_candidates must be >= 2 (got 1)' in lib.cn_last_error().decode()
    assert calls['cn_plan_mppi_modes'](C.byref(cfg), C.byref(plan), C.byref(modes), temperature=0.0) == built.CN_ERR_INVALID
    assert 'cn_plan_mppi_modes: temperature' in lib.cn_last_error().decode()


def test_the_python_surface_exists(built):
    from crowdnav_amd import predict
    from crowdnav_amd.compat.crowd_sim import CrowdSim
    from crowdnav_amd.engine import BatchedCrowdSim
    params = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    default = lambda f, name: inspect.signature(f).parameters[name].default  # noqa: E731
    assert params(BatchedCrowdSim.lookahead_modes) == ['self', 'actions', 'human_vel', 'weights', 'reduce', 'risk_penalty', 'per_mode', 'out']
    assert params(BatchedCrowdSim.plan_cem_modes) == ['self', 'plan', 'human_vel', 'counter', 'weights', 'reduce', 'risk_penalty']
    assert params(BatchedCrowdSim.plan_mppi_modes) == ['self', 'plan', 'human_vel', 'temperature', 'counter', 'weights', 'reduce',
                                                       'risk_penalty', 'fit_std']
    for f in (BatchedCrowdSim.lookahead_modes, BatchedCrowdSim.plan_cem_modes, BatchedCrowdSim.plan_mppi_modes, CrowdSim.lookahead_modes):
        assert default(f, 'weights') is None and default(f, 'reduce') == 'mean' and default(f, 'risk_penalty') == 0.0
    assert default(BatchedCrowdSim.lookahead_modes, 'per_mode') is False
    assert params(CrowdSim.lookahead_modes) == ['self', 'sequences', 'human_velocities', 'weights', 'reduce', 'risk_penalty']
    assert params(predict.stack_modes) == ['tables']
    assert not hasattr(BatchedCrowdSim, 'plan_rollout_modes') and not hasattr(BatchedCrowdSim, 'plan_cem_modes_rollout')
    eng = BatchedCrowdSim.__new__(BatchedCrowdSim)  # no device: shapes and `reduce` are checked before the library is asked
    eng.B, eng.H, eng.A = 2, 3, 4
    acts, vel = np.zeros((2, 5, 4, 2)), np.zeros((2, 3, 4, 3, 2))
    with pytest.raises(ValueError, match='actions must be'):
        eng.lookahead_modes(np.zeros((2, 5, 4, 3)), vel)
    for bad in (np.zeros((2, 4, 3, 2)), np.zeros((2, 3, 3, 3, 2)), np.zeros((2, 3, 4, 4, 2)), np.zeros((1, 3, 4, 3, 2)),
                np.zeros((2, 9, 4, 3, 2)), np.zeros((2, 0, 4, 3, 2))):  # no M; n, H, B that do not fit; M = 9; M = 0
        with pytest.raises(ValueError, match='human_vel must be'):
            eng.lookahead_modes(acts, bad)
    for bad in ('max', 'MEAN', 0, None):
        with pytest.raises(ValueError, match='reduce must be one of'):
            eng.lookahead_modes(acts, vel, reduce=bad)
    for bad in (np.ones(3), np.ones((2, 4)), np.ones((3, 2))):
        with pytest.raises(ValueError, match='weights must be'):
            eng.lookahead_modes(acts, vel, weights=bad)
    with pytest.raises(ValueError, match='a Plan made by'):
        eng.plan_cem_modes(object(), vel, 0)
    with pytest.raises(ValueError, match='a Plan made by'):
        eng.plan_mppi_modes(object(), vel, 0.7, 0)


# ---------------------------------------------------------------------------------------- predict.stack_modes
def test_stack_modes():
    import torch
    from crowdnav_amd import predict
    a = np.arange(2 * 3 * 2 * 2, dtype=np.float64).reshape(2, 3, 2, 2)
    b, c = a + 100.0, (a + 200.0).astype(np.float32)
    got = predict.stack_modes(a, b, c)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (2, 3, 3, 2, 2) and got.flags['C_CONTIGUOUS']
    for m, table in enumerate((a, b, c)):
        assert np.array_equal(got[:, m], table)
    one = predict.stack_modes(a)
    assert one.shape == (2, 1, 3, 2, 2) and np.array_equal(one[:, 0], a)
    t = predict.stack_modes(torch.from_numpy(a), torch.from_numpy(c))
    assert torch.is_tensor(t) and t.dtype == torch.float64 and t.is_contiguous() and np.array_equal(t.numpy(), got[:, [0, 2]])
    mixed = predict.stack_modes(torch.from_numpy(a), b)  # numpy unless every table is a torch tensor
    assert isinstance(mixed, np.ndarray) and np.array_equal(mixed, got[:, :2])
    for bad in ((), (a, a[:, :2]), (a[0],), (np.zeros((2, 3, 2, 3)),)):
        with pytest.raises(ValueError):
            predict.stack_modes(*bad)


# ---------------------------------------------------------------------------------------- the reduction, by hand
def test_the_reduction_on_crafted_modes():
    C_, N, R = ref.COLLISION, ref.NOTHING, ref.REACH_GOAL
    ret, info, steps, time = [0.5, -0.25, 1.0, -0.25], [N, C_, R, C_], [8, 3, 5, 2], [2.0, 0.75, 1.25, 0.5]
    w = [0.5, 0.25, 0.125, 0.125]  # exact powers of two: every product below is exact, so the sums can be written by hand
    # mean: 0.25 - 0.0625 + 0.125 - 0.03125 = 0.28125; risk: 0.25 + 0.125 = 0.375; the tie at -0.25 picks mode 1, not 3
    assert ref.reduce_branch(ret, info, steps, time, w, ref.MEAN, 0.0) == (0.28125, 0.375, 1, C_, 3, 0.75)
    assert ref.reduce_branch(ret, info, steps, time, w, ref.MEAN, 0.5) == (0.28125 - 0.1875, 0.375, 1, C_, 3, 0.75)
    # min does not read the weights for r (the risk still does)
    assert ref.reduce_branch(ret, info, steps, time, w, ref.MIN, 0.0) == (-0.25, 0.375, 1, C_, 3, 0.75)
    assert ref.reduce_branch(ret, info, steps, time, [64.0, 2.0, 4.0, 0.0], ref.MIN, 0.0)[0] == -0.25
    assert ref.reduce_branch(ret, info, steps, time, w, ref.MIN, 0.5) == (-0.25 - 0.1875, 0.375, 1, C_, 3, 0.75)
    # weights are used as given: not normalised
    assert ref.reduce_branch(ret, info, steps, time, [2.0, 2.0, 2.0, 2.0], ref.MEAN, 1.0) == (2.0 - 4.0, 4.0, 1, C_, 3, 0.75)
    # None = 1.0 / M each; sequential from 0.0: ((0.0 + 0.1/3) + 0.2/3) + 0.3/3 in that order
    third = 1.0 / 3.0
    want = ((0.0 + third * 0.1) + third * 0.2) + third * 0.3
    got = ref.reduce_branch([0.1, 0.2, 0.3], [N, N, N], [4, 4, 4], [1.0, 1.0, 1.0], None, ref.MEAN, 0.5)
    assert got == (want, 0.0, 0, N, 4, 1.0)
    # one mode; a later, strictly lower mode
    assert ref.reduce_branch([-0.25], [C_], [1], [0.25], None, ref.MEAN, 2.0) == (-0.25 - 2.0, 1.0, 0, C_, 1, 0.25)
    assert ref.reduce_branch([0.0, 0.0, -0.125], [N, N, ref.DANGER], [4, 4, 4], [1.0] * 3, None, ref.MIN, 0.0)[:3] == (-0.125, 0.0, 2)
    with pytest.raises(ValueError):
        ref.reduce_branch(ret, info, steps, time, w, 'max', 0.0)
    # reduced(): the same, over arrays [B, K, M], weights [B, M]
    modes = dict(ret=np.array([[ret, ret[::-1]]]), info=np.array([[info, info[::-1]]], np.uint8),
                 steps=np.array([[steps, steps[::-1]]], np.int32), time=np.array([[time, time[::-1]]]))
    out = ref.reduced(modes, np.array([w]), ref.MEAN, 0.5)
    assert out['score'].shape == (1, 2) and out['worst_mode'].tolist() == [[1, 0]] and out['worst_steps'].tolist() == [[3, 2]]
    assert out['score'][0, 0] == 0.28125 - 0.1875 and out['risk'][0, 0] == 0.375 and out['worst_time'].tolist() == [[0.75, 0.5]]


# ---------------------------------------------------------------------------------------- what the device cases contain
def test_the_device_cases_contain_what_they_are_meant_to():
    """On the restatement, over the case table test_lookahead_modes.py reduces on the device (ref.REDUCTION_CASES)."""
    outcomes, differ, worst_later, ties, early = set(), 0, 0, 0, 0
    for H, K, n, M in ref.REDUCTION_CASES:
        state, gtime, actions, vel, modes = ref.case(H, K, n, M)
        assert vel.shape == (3, M, n, H, 2) and vel[0, 0, 0, 0, 0] == ref.UNROUNDABLE  # a velocity no float32 holds
        if M >= 3:
            assert np.array_equal(vel[:, M - 1, :, :, :], vel[:, 1]) and not np.array_equal(vel[:, 0, 1:], vel[:, 1, 1:])
            assert (vel[:, 2, 1:] != vel[:, 2, :-1]).any() if n > 1 else True  # the turning tables turn
        outcomes |= set(np.unique(modes['info']).tolist())
        # modes of one branch that end at different steps with different info
        differ += int(((modes['steps'].max(-1) != modes['steps'].min(-1)) & (modes['info'].max(-1) != modes['info'].min(-1))).sum())
        red = ref.reduced(modes)
        worst_later += int((red['worst_mode'] != 0).sum())
        lowest = modes['ret'].min(-1, keepdims=True)
        tie = ((modes['ret'] == lowest).sum(-1) >= 2) & (lowest[..., 0] < 0.0)  # an exact tie at a lowest return something earned
        ties += int(tie.sum())
        assert (red['worst_mode'][tie] == np.argmax(modes['ret'] == lowest, axis=-1)[tie]).all()
        # a lane whose modes have all ended before n while its 64-lane workgroup runs on
        longest = modes['steps'].max(-1)
        for b in range(3):
            for first in range(0, K, 64):
                lanes = longest[b, first:first + 64]
                early += int((lanes < min(n, lanes.max())).sum()) if lanes.max() > lanes.min() else 0
        print((H, K, n, M), 'info', np.bincount(modes['info'].ravel(), minlength=5).tolist())
    print('differ', differ, 'worst_mode != 0', worst_later, 'ties', ties, 'lanes ended under a running workgroup', early)
    assert outcomes == {ref.NOTHING, ref.DANGER, ref.REACH_GOAL, ref.COLLISION, ref.TIMEOUT}
    assert differ >= 1 and worst_later >= 1 and ties >= 1 and early >= 1
