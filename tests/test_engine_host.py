"""engine.py's host rules without a GPU or the built library: an engine made with __new__ on the CPU device over a fake library whose
every cn_* symbol records its call and returns CN_OK.  Pinned: when a call synchronises (only after it copied an argument — and
always in set_state / set_theta / reset), how a caller's `out` is validated, what a rollout-bound method does before
rollout_begin, the no-op calls, the structs handed to the library and the names of the public surface.  What needs a device
(sarl_set_weights with temporaries: record_stream) is left to the GPU suite."""
import ctypes as C

import numpy as np
import pytest
import torch

from crowdnav_amd import engine as E
from crowdnav_amd._lib import CnLookaheadOut, CnRolloutIo, CnTraceOut

B, H, A = 2, 2, 3
F64, F32, I32, U8 = torch.float64, torch.float32, torch.int32, torch.uint8

# dir(BatchedCrowdSim) of the commit before the host rules were stated once: every public callable
PUBLIC = ['close', 'drop_robot_sim', 'drop_sims', 'gather_records_rccl', 'get_state', 'get_theta', 'human_count', 'launch_counts',
          'lookahead', 'mt_random', 'orca', 'plan_begin', 'plan_cem', 'plan_draw', 'plan_mppi', 'plan_mppi_rollout',
          'plan_mppi_update', 'plan_refit', 'plan_reset', 'plan_rollout', 'plan_shift', 'records_summary', 'reset', 'reset_async',
          'rollout', 'rollout_actions', 'rollout_begin', 'rollout_records', 'rollout_route', 'rollout_step', 'rollout_summary',
          'rollout_trace', 'sarl_configure', 'sarl_explore', 'sarl_export', 'sarl_network_route', 'sarl_sampler', 'sarl_select',
          'sarl_set_weights', 'sarl_state_values', 'sarl_transform', 'sarl_values', 'set_gamma', 'set_robot_sim', 'set_state',
          'set_theta', 'step', 'step_into', 'sync', 'use_current_stream']
SARL = ['sarl_configure', 'sarl_set_weights', 'sarl_select', 'sarl_export', 'sarl_explore', 'sarl_transform', 'sarl_sampler',
        'sarl_values', 'sarl_state_values']


class FakeLib(object):
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith('cn_'):
            raise AttributeError(name)

        def symbol(*args):
            self.calls.append((name, args))
            return 0
        return symbol

    def names(self):
        return [name for name, _ in self.calls]

    def take(self):
        """The calls so far, forgotten."""
        calls, self.calls = self.calls, []
        return calls


def make_engine(rollout=True):
    eng = E.BatchedCrowdSim.__new__(E.BatchedCrowdSim)
    eng.device, eng.B, eng.H, eng.A = torch.device('cpu'), B, H, A
    eng._h, eng._lib = C.c_void_p(0x10), FakeLib()
    eng._rollout = (CnRolloutIo(), {}) if rollout else None
    return eng


@pytest.fixture
def eng():
    return make_engine()


def copied_forms(dense):
    """The argument forms a call has to copy: a list, a numpy array, another dtype, a strided view."""
    other = dense.to(torch.bool if dense.dtype == U8 else F32)
    strided = torch.zeros(tuple(dense.shape) + (2,), dtype=dense.dtype)[..., 0]
    assert not strided.is_contiguous()
    return dict(list=dense.tolist(), numpy=dense.numpy(), dtype=other, strided=strided)


def borrowing_calls(eng):
    """name -> (library symbol, dense argument, call(argument))."""
    plan = eng.plan_begin(2, 2, 1, 1, 0.5)
    state = torch.zeros((4, A, 8), dtype=F64)
    theta = torch.zeros(4, dtype=F64)
    return {
        'step': ('cn_step', torch.zeros((B, 2), dtype=F64), eng.step),
        'rollout_step': ('cn_rollout_step', torch.zeros((B, 2), dtype=F64), eng.rollout_step),
        'rollout_actions': ('cn_rollout_actions', torch.zeros((B, 3, 2), dtype=F64), eng.rollout_actions),
        'lookahead': ('cn_lookahead_actions', torch.zeros((B, 2, 2, 2), dtype=F64), eng.lookahead),
        'lookahead_bootstrap': ('cn_lookahead_values', torch.zeros((B, 2, 2, 2), dtype=F64),
                                lambda a: eng.lookahead(a, bootstrap=True)),
        'plan_reset': ('cn_plan_reset', torch.zeros(B, dtype=U8), lambda m: eng.plan_reset(plan, m)),
        'state_values': ('cn_sarl_state_values', state, eng.sarl_state_values),
        'state_values_theta_held': ('cn_sarl_state_values', state, lambda s: eng.sarl_state_values(s, theta)),
        'state_values_state_held': ('cn_sarl_state_values', theta, lambda th: eng.sarl_state_values(state, th)),
    }


NAMES = ['step', 'rollout_step', 'rollout_actions', 'lookahead', 'lookahead_bootstrap', 'plan_reset', 'state_values',
         'state_values_theta_held', 'state_values_state_held']


@pytest.mark.parametrize('name', NAMES)
def test_a_call_synchronises_exactly_when_it_copied_an_argument(eng, name):
    symbol, dense, call = borrowing_calls(eng)[name]
    call(dense)
    assert [n for n, _ in eng._lib.take()] == [symbol]  # read where it lies: no sync
    for form, arg in copied_forms(dense).items():
        call(arg)
        assert [n for n, _ in eng._lib.take()] == [symbol, 'cn_sync'], form  # one sync, after the call


def test_state_values_synchronises_when_both_arguments_were_copied(eng):
    eng.sarl_state_values(np.zeros((4, A, 8)), np.zeros(4))
    assert eng._lib.names() == ['cn_sarl_state_values', 'cn_sync']


def test_step_without_an_action_does_not_synchronise(eng):
    out = eng.step(None, want_obs=False)
    assert eng._lib.names() == ['cn_step'] and out['obs'] is None and out['reward'].shape == (B,)


def test_set_state_set_theta_and_reset_always_synchronise_once(eng):
    s, g, th = torch.zeros((B, A, 8), dtype=F64), torch.zeros(B, dtype=F64), torch.zeros(B, dtype=F64)
    for call, symbol in ((lambda: eng.set_state(s, g), 'cn_set_state'), (lambda: eng.set_state(s.tolist()), 'cn_set_state'),
                         (lambda: eng.set_state(), 'cn_set_state'), (lambda: eng.set_theta(th), 'cn_set_theta'),
                         (lambda: eng.set_theta(th.numpy()), 'cn_set_theta'), (lambda: eng.reset([1, 2]), 'cn_reset'),
                         (lambda: eng.reset(torch.tensor([1, 2]), mask=torch.ones(B, dtype=U8)), 'cn_reset')):
        call()
        assert [n for n, _ in eng._lib.take()] == [symbol, 'cn_sync']
    draws = eng.reset(np.array([2 ** 32 - 1, 7], dtype=np.uint32))
    assert draws.dtype == torch.int64 and draws.shape == (B,) and not draws.any()
    with pytest.raises(ValueError, match='expected shape'):
        eng.set_theta(np.zeros(B + 1))


# ---------------------------------------------------------------------------------------- the caller's `out`
def out_calls(eng):
    """name -> (who, call(out) -> dict, the names a fresh dict holds)."""
    trace, look = ('state8', 'episode', 'step'), ('ret', 'info', 'steps', 'time')
    acts = torch.zeros((B, 2, 2), dtype=F64)
    cands = torch.zeros((B, 2, 2, 2), dtype=F64)
    return {
        'rollout_trace': ('rollout_trace', lambda out: eng.rollout_trace(2, out=out), trace),
        'rollout_trace_rewards': ('rollout_trace', lambda out: eng.rollout_trace(2, rewards=True, out=out),
                                  trace + ('reward', 'info', 'dmin')),
        'rollout_actions': ('rollout_actions', lambda out: eng.rollout_actions(acts, trace=True, rewards=True, out=out),
                            trace + ('reward', 'info', 'dmin')),
        'lookahead': ('lookahead', lambda out: eng.lookahead(cands, out=out), look),
        'lookahead_final': ('lookahead', lambda out: eng.lookahead(cands, final_state=True, out=out),
                            look + ('final_state8', 'final_theta')),
        'lookahead_bootstrap': ('lookahead', lambda out: eng.lookahead(cands, bootstrap=True, out=out),
                                look + ('final_state8', 'final_theta', 'value', 'score')),
    }


SHAPES = dict(state8=(F64, (B, 2, A, 8)), episode=(I32, (B, 2)), step=(I32, (B, 2)), reward=(F64, (B, 2)), dmin=(F64, (B, 2)),
              ret=(F64, (B, 2)), steps=(I32, (B, 2)), time=(F64, (B, 2)), final_state8=(F64, (B, 2, A, 8)),
              final_theta=(F64, (B, 2)), value=(F32, (B, 2)), score=(F64, (B, 2)), info=(U8, (B, 2)))


@pytest.mark.parametrize('name', ['rollout_trace', 'rollout_trace_rewards', 'rollout_actions', 'lookahead', 'lookahead_final',
                                  'lookahead_bootstrap'])
def test_out_is_made_fresh_or_validated_against_the_spec(eng, name):
    who, call, keys = out_calls(eng)[name]
    fresh = call(None)
    assert tuple(fresh) == keys
    for k, t in fresh.items():
        assert (t.dtype, tuple(t.shape)) == SHAPES[k] and t.is_contiguous() and t.device == eng.device, k
    if 'episode' in fresh:
        assert (fresh['episode'] == -1).all()
        fresh['episode'].fill_(5)
    # right: the caller's tensors come back, what the spec does not name is dropped, episode is refilled
    again = call(dict(fresh, extra=torch.zeros(1), score_of_another_call=None))
    assert tuple(again) == keys and all(again[k] is fresh[k] for k in keys)
    if 'episode' in fresh:
        assert (fresh['episode'] == -1).all()
    eng._lib.take()
    # wrong, every key in turn: dtype, shape, strides, absent, not a tensor
    for k in keys:
        dt, shape = SHAPES[k]
        bad = dict(dtype=torch.zeros(shape, dtype=torch.int64), shape=torch.zeros(shape[:1] + (1,) + shape[2:], dtype=dt),
                   strided=torch.zeros(shape + (2,), dtype=dt)[..., 0], numpy=np.zeros(shape), absent=None)
        for what, t in bad.items():
            out = dict(fresh)
            if what == 'absent':
                del out[k]
            else:
                out[k] = t
            with pytest.raises(ValueError) as ei:
                call(out)
            assert str(ei.value) == '%s: out[%r] must be a contiguous %s %s tensor on cpu' % (who, k, dt, shape), (k, what)
    assert eng._lib.calls == []  # refused before the library is reached


def test_a_plain_trace_drops_the_reward_rows_of_the_out_it_is_given(eng):
    full = eng.rollout_trace(2, rewards=True)
    assert tuple(eng.rollout_trace(2, out=full)) == ('state8', 'episode', 'step')
    with pytest.raises(ValueError, match='n_steps must be >= 0'):
        eng.rollout_trace(-1)


@pytest.mark.parametrize('which', ['records_summary', 'rollout_summary'])
def test_summary_out(eng, which):
    blocks = torch.zeros((3, 1 + 6 * 4), dtype=F64)
    call = (lambda out: eng.records_summary(blocks, out=out)) if which == 'records_summary' else \
        (lambda out: eng.rollout_summary(out=out))
    fresh = call(None)
    assert fresh.dtype == F64 and fresh.shape == (8,)
    assert call(fresh) is fresh
    for bad in (torch.zeros(8, dtype=F32), torch.zeros(7, dtype=F64), torch.zeros(16, dtype=F64)[::2]):
        with pytest.raises(ValueError, match=r'summary output: a contiguous float64 \[8\] tensor on cpu'):
            call(bad)
    symbol = 'cn_' + which
    assert eng._lib.names() == [symbol, symbol]
    if which == 'records_summary':
        assert eng._lib.calls[0][1][1:4] == (3, 4, 4)
        eng.records_summary(blocks, record_capacity=9)
        assert eng._lib.calls[-1][1][1:4] == (3, 4, 9)


def test_state_values_out_and_sarl_values(eng):
    state = torch.zeros((2, 2, A, 8), dtype=F64)
    got = eng.sarl_state_values(state, theta=torch.zeros((2, 2), dtype=F64), sort_humans=True)
    assert got.dtype == F32 and got.shape == (4,)
    name, args = eng._lib.take()[0]
    assert name == 'cn_sarl_state_values' and args[1].value == state.data_ptr() and args[3:5] == (4, 1)
    assert args[5].value == got.data_ptr()
    assert eng.sarl_state_values(state, out=got) is got
    for bad in (torch.zeros(4, dtype=F64), torch.zeros(3, dtype=F32), torch.zeros(8, dtype=F32)[::2], np.zeros(4, np.float32)):
        with pytest.raises(ValueError, match=r'sarl_state_values: out must be a contiguous float32 \[4\] tensor on cpu'):
            eng.sarl_state_values(state, out=bad)
    rows = torch.zeros((5, H, 13), dtype=F32)
    v = eng.sarl_values(rows)
    assert v.dtype == F32 and v.shape == (5,) and eng.sarl_values(rows, out=v) is v
    for bad in (rows.double(), torch.zeros((5, H, 12), dtype=F32), torch.zeros((5, H, 13, 2), dtype=F32)[..., 0]):
        with pytest.raises(ValueError, match=r'sarl_values: expected a contiguous float32 \[n, 2, 13\] tensor on cpu'):
            eng.sarl_values(bad)


# ---------------------------------------------------------------------------------------- the rollout
def rollout_bound(eng, plan):
    return {
        'rollout': lambda: eng.rollout(3),
        'rollout_trace': lambda: eng.rollout_trace(3),
        'rollout_step': lambda: eng.rollout_step(torch.zeros((B, 2), dtype=F64)),
        'rollout_actions': lambda: eng.rollout_actions(torch.zeros((B, 3, 2), dtype=F64)),
        'rollout_actions_trace': lambda: eng.rollout_actions(torch.zeros((B, 3, 2), dtype=F64), trace=True),
        'rollout_records': lambda: eng.rollout_records(4),
        'rollout_summary': lambda: eng.rollout_summary(),
        'plan_shift': lambda: eng.plan_shift(plan),
        'plan_rollout': lambda: eng.plan_rollout(plan, 3, 0),
        'plan_mppi_rollout': lambda: eng.plan_mppi_rollout(plan, 3, 1.0, 0),
    }


def test_every_rollout_bound_method_asks_for_rollout_begin_first():
    eng = make_engine(rollout=False)
    for plan in (eng.plan_begin(2, 2, 1, 1, 0.5), object()):  # ... in preference to the plan error
        for name, call in rollout_bound(eng, plan).items():
            with pytest.raises(RuntimeError, match=r'call rollout_begin\(\) first'):
                call()
    assert eng._lib.calls == []
    eng._rollout = (CnRolloutIo(), {})
    for name in ('plan_shift', 'plan_rollout', 'plan_mppi_rollout'):
        with pytest.raises(ValueError, match='plan_begin'):
            rollout_bound(eng, object())[name]()
        with pytest.raises(ValueError, match='plan_begin'):
            rollout_bound(eng, make_engine().plan_begin(2, 2, 1, 1, 0.5))[name]()  # another engine's plan
    assert eng._lib.calls == []


def test_rollout_bound_methods_hand_over_the_io_and_return_the_buffers(eng):
    io, bufs = eng._rollout
    plan = eng.plan_begin(2, 2, 1, 1, 0.5)
    returns_bufs = ('rollout', 'rollout_step', 'rollout_actions', 'plan_rollout', 'plan_mppi_rollout')
    for name, call in rollout_bound(eng, plan).items():
        got = call()
        (symbol, args), = eng._lib.take()
        assert symbol == 'cn_' + name.replace('_actions_trace', '_actions') and args[0] is eng._h
        assert args[1]._obj is io, name
        if name in returns_bufs:
            assert got is bufs, name
    assert eng.rollout_records(4).shape == (B, 25)


def test_zero_steps_reach_no_library_symbol(eng):
    assert tuple(eng.rollout_trace(0)['state8'].shape) == (B, 0, A, 8)
    assert eng.rollout_actions(torch.zeros((B, 0, 2), dtype=F64)) is eng._rollout[1]
    assert eng.rollout_actions(np.zeros((B, 0, 2)), trace=True)['episode'].shape == (B, 0)
    out = eng.lookahead(np.zeros((B, 3, 0, 2)), bootstrap=True)
    assert out['score'].shape == (B, 3)
    assert eng._lib.calls == []


def test_shape_refusals_come_before_the_device_and_the_library():
    eng = E.BatchedCrowdSim.__new__(E.BatchedCrowdSim)
    eng.B, eng.H, eng.A, eng._h, eng._rollout = B, H, A, None, (None, None)
    with pytest.raises(ValueError, match='lookahead: actions must be'):
        eng.lookahead(np.zeros((B, 0, 2, 2)))
    with pytest.raises(ValueError, match='rollout_actions: actions must be'):
        eng.rollout_actions(np.zeros((B, 2, 3)))
    with pytest.raises(ValueError, match='state8 must be'):
        eng.sarl_state_values(np.zeros((2, A, 7)))
    with pytest.raises(ValueError, match='theta must be'):
        eng.sarl_state_values(np.zeros((2, A, 8)), theta=np.zeros(3))
    with pytest.raises(ValueError, match='K and n'):
        eng.plan_begin(2, 0, 1, 1, 0.5)


# ---------------------------------------------------------------------------------------- structs
def test_the_trace_struct_names_the_rows(eng):
    out = eng.rollout_trace(2)
    tr = eng._lib.take()[0][1][3]._obj
    assert isinstance(tr, CnTraceOut) and [tr.reward, tr.info, tr.dmin] == [None] * 3
    assert all(getattr(tr, k) == out[k].data_ptr() for k in ('state8', 'episode', 'step'))
    acts = torch.zeros((B, 2, 2), dtype=F64)
    out = eng.rollout_actions(acts, trace=True, rewards=True)
    args = eng._lib.take()[0][1]
    assert args[2] == 2 and args[3].value == acts.data_ptr()
    assert all(getattr(args[4]._obj, k) == out[k].data_ptr() for k, _ in CnTraceOut._fields_)
    eng.rollout_actions(acts)
    assert eng._lib.take()[0][1][4] is None


def test_the_lookahead_struct_and_the_separate_value_and_score(eng):
    cands = torch.zeros((B, 2, 3, 2), dtype=F64)
    out = eng.lookahead(cands, bootstrap=True, sort_humans=True)
    (symbol, args), = eng._lib.take()
    assert symbol == 'cn_lookahead_values' and args[1:3] == (3, 2) and args[3].value == cands.data_ptr() and args[5] == 1
    lo = args[4]._obj
    assert isinstance(lo, CnLookaheadOut) and len(CnLookaheadOut._fields_) == 6
    assert all(getattr(lo, k) == out[k].data_ptr() for k, _ in CnLookaheadOut._fields_)
    assert args[6].value == out['value'].data_ptr() and args[7].value == out['score'].data_ptr()
    out = eng.lookahead(cands)
    (symbol, args), = eng._lib.take()
    assert symbol == 'cn_lookahead_actions' and len(args) == 5 and args[1:3] == (3, 2)
    lo = args[4]._obj
    assert lo.final_state8 is None and lo.final_theta is None and lo.ret == out['ret'].data_ptr()


def test_the_plan_struct(eng):
    plan = eng.plan_begin(3, 2, 2, 4, 0.5, min_std=0.1, smoothing=0.25, seed=-1)
    rows = ('mean', 'std', 'best_actions', 'best_score', 'action', 'candidates', 'order')
    assert all(getattr(plan.c, k) == getattr(plan, k).data_ptr() for k in rows)
    assert plan.c.value is None and plan.c.score is None  # NULL without bootstrap
    assert tuple(plan.look) == ('ret', 'info', 'steps', 'time')
    assert all(getattr(plan.c.look, k) == plan.look[k].data_ptr() for k in plan.look)
    assert plan.c.look.final_state8 is None and plan.c.look.final_theta is None
    assert (plan.std == 0.5).all() and not plan.mean.any() and plan.candidates.shape == (B, 3, 2, 2)
    cfg = plan.cfg
    assert (cfg.n_steps, cfg.n_candidates, cfg.n_elites, cfg.iterations, cfg.bootstrap, cfg.sort_humans) == (2, 3, 2, 4, 0, 0)
    assert (cfg.init_std, cfg.min_std, cfg.smoothing, cfg.seed) == (0.5, 0.1, 0.25, 2 ** 64 - 1)
    boot = eng.plan_begin(3, 2, 2, 4, 0.5, bootstrap=True, sort_humans=True)
    assert tuple(boot.look) == ('ret', 'info', 'steps', 'time', 'final_state8', 'final_theta', 'value', 'score')
    assert boot.c.value == boot.look['value'].data_ptr() and boot.c.score == boot.look['score'].data_ptr()
    assert all(getattr(boot.c.look, k) == boot.look[k].data_ptr() for k, _ in CnLookaheadOut._fields_)
    assert (boot.cfg.bootstrap, boot.cfg.sort_humans) == (1, 1)
    assert sorted(boot.tensors()) == sorted(rows + tuple('look.' + k for k in boot.look))


def test_the_planner_calls(eng):
    plan = eng.plan_begin(2, 2, 1, 1, 0.5)
    io, bufs = eng._rollout
    mask = torch.ones(B, dtype=U8)

    def args_of(symbol, got, want):
        (name, args), = eng._lib.take()
        assert name == symbol and args[0] is eng._h and got is want, symbol
        at = 2 if args[1]._obj is io else 1
        if symbol.endswith('rollout'):
            assert at == 2 and args[2] == 3
            at = 3
        elif symbol == 'cn_plan_shift':
            assert at == 2
        assert args[at]._obj is plan.cfg and args[at + 1]._obj is plan.c, symbol
        return args[at + 2:]

    assert args_of('cn_plan_reset', eng.plan_reset(plan), plan) == (None,)
    assert args_of('cn_plan_reset', eng.plan_reset(plan, mask), plan)[0].value == mask.data_ptr()
    assert args_of('cn_plan_draw', eng.plan_draw(plan, 2 ** 32 + 5), plan.candidates) == (5,)
    assert args_of('cn_plan_refit', eng.plan_refit(plan), plan) == (0,)
    assert args_of('cn_plan_refit', eng.plan_refit(plan, keep_best=True), plan) == (1,)
    assert args_of('cn_plan_cem', eng.plan_cem(plan, -1), plan) == (0xffffffff,)
    assert args_of('cn_plan_shift', eng.plan_shift(plan), plan) == ()
    assert args_of('cn_plan_rollout', eng.plan_rollout(plan, 3, 7), bufs) == (7,)
    assert args_of('cn_plan_mppi_update', eng.plan_mppi_update(plan, 0.5), plan) == (0.5, 0, 0)
    assert args_of('cn_plan_mppi_update', eng.plan_mppi_update(plan, 2, fit_std=True, keep_best=True), plan) == (2.0, 1, 1)
    assert args_of('cn_plan_mppi', eng.plan_mppi(plan, 0.5, 2 ** 32, fit_std=True), plan) == (0.5, 1, 0)
    assert args_of('cn_plan_mppi_rollout', eng.plan_mppi_rollout(plan, 3, 0.5, 9), bufs) == (0.5, 0, 9)
    for call in (lambda: eng.plan_reset(None), lambda: eng.plan_draw(object(), 0), lambda: eng.plan_mppi('plan', 1.0, 0)):
        with pytest.raises(ValueError, match=r"plan: a Plan made by this engine's plan_begin\(\)"):
            call()
    assert eng._lib.calls == []


# ---------------------------------------------------------------------------------------- the value-network methods
def configured(eng, model='sarl'):
    eng.sarl_configure(np.zeros((3, 2)), model=model, mlp3_dims=(150, 100, 100, 1))
    assert eng._lib.take()[0][0] == 'cn_sarl_configure'
    assert eng.sarl['n_actions'] == 3 and eng.sarl['in_dim'] == 13 and eng.sarl['model'] == model
    return eng


def test_select_transform_and_explore(eng):
    configured(eng)
    sel = eng.sarl_select()
    assert sel['values'].shape == (B, 3) and sel['best'].dtype == I32 and sel['action'].shape == (B, 2)
    best, action = torch.zeros(B, dtype=I32), torch.zeros((B, 2), dtype=F64)
    sel = eng.sarl_select(want_values=False, best=best, action=action, want_attention=True)
    assert sel['values'] is None and sel['best'] is best and sel['action'] is action and sel['attention'].shape == (B, 3, H)
    assert eng._lib.names() == ['cn_sarl_select', 'cn_sarl_select_attention']
    with pytest.raises(AssertionError):
        eng.sarl_select(best=torch.zeros(B, dtype=torch.int64))
    with pytest.raises(AssertionError):
        eng.sarl_transform(out=torch.zeros((B, H, 13), dtype=F64))
    with pytest.raises(AssertionError):
        eng.step_into(action, torch.zeros(B, dtype=F32), *(torch.zeros(B, dtype=d) for d in (U8, U8, F64)))
    eng._lib.take()
    x = eng.sarl_transform()
    assert x.shape == (B, H, 13) and x.dtype == F32 and eng._lib.take()[0][1][2:] == (0, 0)
    eng.sarl_explore(sel, 0.1, mask=torch.ones(B, dtype=U8), want_explored=False)
    assert sel['explored'] is None and eng._lib.names() == ['cn_sarl_explore']


def test_set_weights_reads_dense_float32_parameters_where_they_lie(eng):
    configured(eng, 'cadrl')
    sd = {k: torch.zeros(3, dtype=F32) for k in E.CADRL_PARAM_ORDER}
    sd['unrelated'] = None
    eng.sarl_set_weights(sd)
    (name, args), = eng._lib.take()  # no sync: the tensors are kept alive instead
    assert name == 'cn_sarl_set_weights' and list(args[1]) == [sd[k].data_ptr() for k in E.CADRL_PARAM_ORDER]
    assert all(a is sd[k] for a, k in zip(eng._sarl_weights_keepalive, E.CADRL_PARAM_ORDER))


def test_the_sampler_checks_its_tensors_and_precomputes_their_addresses(eng):
    configured(eng)
    T, D = 3, 13
    t = dict(traj=torch.zeros((B, T, H, D), dtype=F32), rew=torch.zeros((T, B), dtype=F64), info=torch.zeros((T, B), dtype=U8),
             dmin=torch.zeros((T, B), dtype=F64), act=torch.zeros((T, B), dtype=I32), alive=torch.ones(B, dtype=U8),
             done=torch.zeros(B, dtype=U8), action=torch.zeros((B, 2), dtype=F64))
    with pytest.raises(ValueError, match=r'traj is \[3, T, 2, D\]'):
        eng.sarl_sampler(**dict(t, traj=torch.zeros((3, T, H, D), dtype=F32)))
    for k, bad in (('rew', t['rew'].float()), ('info', torch.zeros((T, B + 1), dtype=U8)), ('act', torch.zeros((T, B, 2), dtype=I32)[..., 0]),
                   ('done', torch.zeros(B, dtype=torch.bool)), ('action', torch.zeros((B, 3), dtype=F64))):
        with pytest.raises(ValueError, match='sarl_sampler: expected a contiguous'):
            eng.sarl_sampler(**dict(t, **{k: bad}))
    step = eng.sarl_sampler(**t)
    assert all(any(k is v for k in step.keep) for v in t.values()) and eng._lib.calls == []
    step(1, 0.25)
    (name, a), = eng._lib.take()
    assert name == 'cn_sarl_sample_step' and a[0] is eng._h and a[1] == 0.25 and a[6:8] == (T * H * D, 0)
    got = [x.value for x in a[2:6] + a[8:]]
    assert got == [t['alive'].data_ptr(), t['act'].data_ptr() + 4 * B, t['action'].data_ptr(), t['traj'].data_ptr() + 4 * H * D,
                   t['rew'].data_ptr() + 8 * B, t['done'].data_ptr(), t['info'].data_ptr() + B, t['dmin'].data_ptr() + 8 * B]
    eng.close()
    with pytest.raises(RuntimeError, match='the engine has been closed'):
        step(2, 0.0)


# ---------------------------------------------------------------------------------------- the surface
def test_the_public_names_are_callable_attributes_of_the_class():
    for name in PUBLIC + SARL:
        assert callable(getattr(E.BatchedCrowdSim, name)), name
    assert set(SARL) <= set(PUBLIC)
    for name in ('SARL_PARAM_ORDER', 'LSTM_PARAM_ORDER', 'LSTM_PAIRWISE_MLP1_ORDER', 'CADRL_PARAM_ORDER', 'Plan', 'default_config'):
        assert hasattr(E, name), name
    assert len(E.SARL_PARAM_ORDER) == 22 and len(E.LSTM_PARAM_ORDER) == 12 and len(E.CADRL_PARAM_ORDER) == 8
    assert len(E.LSTM_PAIRWISE_MLP1_ORDER) == 8
