"""The ORCA predictor on hypothesised goals (cn_predict_orca_goals) and the sampler of such goals (cn_goal_hypotheses) on the GPU:
1. the environment is the oracle: mode m of predict_orca_goals(n, goals) against n steps of a CrowdOracle whose humans head for
   goals[:, m] and do not see the robot, bit for bit; mode 0 (their own goals) is predict_orca(n);
2. modes and packing do not matter: slot m of an M = 8 call is the M = 1 call on goals[:, m], with 3 and 7 envs; prefixes in n;
3. nothing of the engine moves;   4. goal_hypotheses against crowdnav_amd.predict.goal_hypotheses;
5. the refusals on a live engine;   6. the example's --goal-samples.

Shapes: B = 3, n = 12; 1, 5, 12 and 20 humans (the 5-half-plane kernels, the kd route, the two-sweep pair phase) and the `mixed`
rule.

GOALS_BOUND: the sampler's perturbed rows differ from the numpy restatement through the device's log, cos and sin alone.  The
largest |device - numpy| / max(1, |d|) of a goal component (test_goal_hypotheses_against_the_restatement, d the human's nominal
offset) measured 2.961e-16 on the first run (h5 and h5_mixed under 'heading'; 1.347e-16 and 1.447e-16 under 'engine';
1 to 6 of 120 rows differ at all) — the last bits — and is bounded at 4 x that = 1.184e-15, the margin tests/test_plan.py's
DRAW_BOUND gives the same libm calls.  A wrong round, word or counter order gives O(1); a measured figure above 1e-12 would be a
bug, not a bound."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import predict_orca_cases as cases
import predict_orca_goals_cases as goals_cases
from predict_orca_cases import BEGIN, engine as _engine
from support import (  # noqa: F401  (amd: module fixture)
    amd, example_line as _example_line, np_of as _np, roll_on as _roll_on, same_bits as _same_bits, snapshot as _snapshot)

pytestmark = pytest.mark.gpu

B, N = cases.B, cases.N
GOALS_MEASURED = 2.961e-16
GOALS_BOUND = 4 * GOALS_MEASURED


# ------------------------------------------------------------------------------------------------ 1. the environment is the oracle
@pytest.mark.parametrize('crowd', sorted(cases.CROWDS))
def test_the_environment_is_the_oracle(amd, oracle_mod, crowd):
    """From the state of an engine under way, mode m of predict_orca_goals(12, goal_maps) is orca_vel[:, 1:] of twelve steps of
    the CPU oracle on that state with the humans' goals replaced by goal_maps[:, m], robot_visible = 0 and fresh simulators —
    every row, the 3-D fallback's among them.  The parked placeholders of the `mixed` rule are handed re-mapped rows like
    everybody else and ignore them: the oracle's keep their own goals."""
    import torch
    eng = _engine(amd, crowd, robot_visible=1)
    state, gtime = (_np(x).copy() for x in eng.get_state())
    H = state.shape[1] - 1
    maps = goals_cases.goal_maps(state, crowd)
    goals = torch.from_numpy(maps).to(eng.device)
    got = eng.predict_orca_goals(N, goals)
    assert tuple(got.shape) == (B, 3, N, H, 2) and got.dtype == torch.float64
    assert _same_bits(goals, maps)  # the table is only read
    fallbacks = 0
    for m in range(3):
        want, fallback, _ = cases.oracle_table(oracle_mod, crowd, goals_cases.regoaled(state, maps[:, m]), gtime)
        differ = _np(got[:, m]) != want
        fallbacks += int(fallback.sum())
        print(crowd, 'mode', m, 'entries that differ:', int(differ.sum()), 'of', differ.size, 'first', np.argwhere(differ)[:3].tolist(),
              'fallback solves', int(fallback.sum()))
        assert _same_bits(got[:, m].contiguous(), want), (crowd, m)
    if crowd in ('h12', 'h20'):
        assert fallbacks > 0
    assert torch.equal(got[:, 0], eng.predict_orca(N))
    assert not torch.equal(got[:, 1], got[:, 0]) and not torch.equal(got[:, 2], got[:, 0]) and not torch.equal(got[:, 2], got[:, 1])
    if crowd == 'h5_mixed':
        parked = goals_cases.parked(state)
        assert parked.any() and not parked.all()
        assert (maps[:, 1][parked] != state[:, 1:, 4:6][parked]).any()  # rows that would have moved them


# ------------------------------------------------------------------------------------------------ 2. modes and packing
@pytest.mark.parametrize('envs', [3, 7])
@pytest.mark.parametrize('crowd', ['h1', 'h5', 'h12'])
def test_modes_and_packing_do_not_matter(amd, crowd, envs):
    """Slot m of an M = 8 call (the goals turned by m / 8 of a circle) is the M = 1 call on goals[:, m]: 3, 24, 7 and 56 virtual
    envs against workgroups of E envs, the last one partial.  The first 1 and 5 rows of the n = 12 table are the calls with
    that n."""
    import torch
    eng = _engine(amd, crowd, envs=envs, robot_visible=1)
    state = _np(eng.get_state()[0])
    goals = torch.from_numpy(goals_cases.rotations(state, 8)).to(eng.device)
    full = eng.predict_orca_goals(N, goals)
    assert tuple(full.shape) == (envs, 8, N, eng.H, 2) and bool(torch.isfinite(full).all())
    assert torch.equal(full[:, 0], eng.predict_orca(N))
    for m in range(8):
        one = eng.predict_orca_goals(N, goals[:, m].contiguous())
        assert tuple(one.shape) == (envs, N, eng.H, 2)
        assert torch.equal(one, full[:, m]), (crowd, envs, m)
        if m:
            assert not torch.equal(one, full[:, 0])
    # M = 1 as a [B, 1, H, 2] table keeps the mode axis; `out` is written where it lies
    kept = eng.predict_orca_goals(N, goals[:, 3:4].contiguous())
    assert tuple(kept.shape) == (envs, 1, N, eng.H, 2) and torch.equal(kept[:, 0], full[:, 3])
    out = torch.full((envs, 8, N, eng.H, 2), -7.0, dtype=torch.float64, device=eng.device)
    assert eng.predict_orca_goals(N, goals, out=out) is out and torch.equal(out, full)
    # a numpy table is copied to the device
    assert torch.equal(eng.predict_orca_goals(N, _np(goals)), full)
    for n in (1, 5):
        assert torch.equal(eng.predict_orca_goals(n, goals), full[:, :, :n]), n
    assert tuple(eng.predict_orca_goals(0, goals).shape) == (envs, 8, 0, eng.H, 2)


# ------------------------------------------------------------------------------------------------ 3. nothing moves
KINDS = {'external': ('h12', {}), 'orca_robot': ('h12', dict(robot_policy=1)), 'unicycle': ('h5', dict(robot_kinematics=1))}


@pytest.mark.parametrize('kind', sorted(KINDS))
def test_nothing_of_the_engine_moves(amd, kind):
    """In the middle of a rollout_begin / rollout_step sequence: state, heading, launch counters, the human-model setting, the
    rollout's buffers and the table of goals are as before, and the rollout and a step() that follow give what a twin gives
    that was never asked — on the kd route (12 humans) that includes the simulators' visiting order and the ORCA robot's
    captured simulator."""
    import torch
    crowd, cfg = KINDS[kind]
    cfg = dict(cfg, robot_visible=1)
    if 'robot_policy' in cfg:
        cfg['robot_policy'] = amd.ROBOT_ORCA
    eng, twin = (_engine(amd, crowd, steps=0, **cfg) for _ in range(2))
    bufs, tbufs = eng.rollout_begin(**BEGIN), twin.rollout_begin(**BEGIN)
    for e in (eng, twin):
        _roll_on(e, kind, 3)
    if kind == 'external':
        for e in (eng, twin):
            e.set_lookahead_human_model('constant_velocity')
    before, io_before = _snapshot(eng), {k: v.clone() for k, v in bufs.items()}
    counts, model = eng.launch_counts(), eng.lookahead_human_model
    goals = eng.goal_hypotheses(4, 'heading', std_heading=0.4, std_distance=0.3, seed=5, counter=2)
    held = goals.clone()
    table = eng.predict_orca_goals(N, goals)
    eng.goal_hypotheses(4, 'engine', std_heading=0.4, out=torch.empty_like(goals))
    eng.sync()
    assert bool(torch.isfinite(table).all()) and bool((table != 0.0).any()) and torch.equal(goals, held)
    assert eng.launch_counts() == counts and 'lagged_fills' in counts and eng.lookahead_human_model == model
    for a, b in zip(before, _snapshot(eng)):
        assert torch.equal(a, b)
    for k, v in io_before.items():
        assert torch.equal(v, bufs[k]), k
    # ... the rollout goes on as if the calls had not been made, and so does a plain step
    for e in (eng, twin):
        _roll_on(e, kind, 2)
    for a, b in zip(_snapshot(eng), _snapshot(twin)):
        assert torch.equal(a, b)
    for k, v in tbufs.items():
        assert torch.equal(v, bufs[k]), k
    eng.predict_orca_goals(3, eng.goal_hypotheses(2, 'engine'))
    action = None if kind == 'orca_robot' else np.tile([0.3, 0.2], (B, 1))
    got, want = (e.step(action, update=True, want_obs=True) for e in (eng, twin))
    assert sorted(got) == sorted(want)
    for k, v in want.items():
        assert (v is None and got[k] is None) or torch.equal(v, got[k]), k
    for a, b in zip(_snapshot(eng), _snapshot(twin)):
        assert torch.equal(a, b)
    assert eng.launch_counts() == twin.launch_counts()


# ------------------------------------------------------------------------------------------------ 4. the sampler
SAMPLER = dict(std_heading=0.4, std_distance=0.3, seed=(0x1234 << 32) | 0x9abcdef1, counter=17)


@pytest.mark.parametrize('base', ['engine', 'heading'])
@pytest.mark.parametrize('crowd', ['h5', 'h5_mixed'])
def test_goal_hypotheses_against_the_restatement(amd, crowd, base):
    import torch
    from crowdnav_amd import predict
    eng = _engine(amd, crowd, robot_visible=1)
    state, gtime = (_np(x).copy() for x in eng.get_state())
    p, g = state[:, 1:, 0:2], state[:, 1:, 4:6]
    reach = eng.config['human_v_pref'] * eng.config['time_step'] * 12
    kw = dict(reach=reach) if base == 'heading' else {}
    got = eng.goal_hypotheses(8, base, **SAMPLER)  # (reach=None: the documented default)
    want = predict.goal_hypotheses(state, 8, base, **SAMPLER, **kw)
    assert tuple(got.shape) == (B, 8, eng.H, 2) and got.dtype == torch.float64
    # exact: mode 0; every row with both deviations 0; the placeholders' goals
    assert _same_bits(got[:, 0].contiguous(), np.ascontiguousarray(want[:, 0]))
    if base == 'engine':
        assert _same_bits(got[:, 0].contiguous(), np.ascontiguousarray(g))
    flat = dict(SAMPLER, std_heading=0.0, std_distance=0.0)
    for first in (True, False):
        assert _same_bits(eng.goal_hypotheses(8, base, nominal_first=first, **flat),
                          predict.goal_hypotheses(state, 8, base, nominal_first=first, **flat, **kw)), first
    parked = goals_cases.parked(state)
    assert parked.any() == (crowd == 'h5_mixed')
    for m in range(8):
        assert _same_bits(_np(got)[:, m][parked], g[parked]), m
    # the perturbed rows, within the bound; they are perturbed
    d = want[:, :1] - p[:, None]
    err = np.abs(_np(got) - want) / np.maximum(1.0, np.sqrt((d * d).sum(axis=-1, keepdims=True)))
    moved = (want[:, 1:] != want[:, :1]).any(axis=-1)
    print('goal_hypotheses parity %s %s: largest |device - numpy| / max(1, |d|) = %.3e (bound %.3e), rows that differ %d of %d, '
          'perturbed rows %d' % (crowd, base, err.max(), GOALS_BOUND, int((err > 0).any(axis=-1).sum()), err[..., 0].size, int(moved.sum())))
    assert moved.any() and not moved[np.broadcast_to(parked[:, None], moved.shape)].any()
    assert GOALS_MEASURED <= 1e-12 and err.max() <= GOALS_BOUND
    # a row depends on neither B nor M; another counter gives other rows
    assert torch.equal(eng.goal_hypotheses(3, base, **SAMPLER), got[:, :3])
    two = _engine(amd, crowd, envs=2, steps=0, robot_visible=1)
    two.set_state(state[:2], gtime[:2])
    assert torch.equal(two.goal_hypotheses(8, base, **SAMPLER), got[:2])
    other = eng.goal_hypotheses(8, base, **dict(SAMPLER, counter=18))
    assert torch.equal(other[:, 0], got[:, 0]) and not torch.equal(other[:, 1:], got[:, 1:])
    assert torch.equal(eng.goal_hypotheses(8, base, **SAMPLER), got)


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_on_an_engine(amd):
    import torch
    lib = amd._lib
    L, INV, UNS = lib.load(), lib.CN_ERR_INVALID, lib.CN_ERR_UNSUPPORTED
    eng = _engine(amd, 'h5', steps=0)
    goals = eng.goal_hypotheses(2, 'engine')
    table = torch.full((B, 2, 4, eng.H, 2), -7.0, dtype=torch.float64, device=eng.device)
    held = goals.clone()
    eng.sync()
    counts = eng.launch_counts()
    g, t = C.c_void_p(goals.data_ptr()), C.c_void_p(table.data_ptr())

    def refused(call, args, status, *words):
        assert call(*args) == status, (args, L.cn_last_error())
        text = L.cn_last_error().decode()
        assert all(w in text for w in words), text

    # cn_predict_orca_goals, in the header's order, each with everything behind it wrong as well
    who = 'cn_predict_orca_goals'
    refused(L.cn_predict_orca_goals, (eng._h, -1, 0, None, None), INV, who, 'goals is NULL')
    refused(L.cn_predict_orca_goals, (eng._h, -1, 0, g, None), INV, who, 'human_vel is NULL')
    refused(L.cn_predict_orca_goals, (eng._h, -1, 0, g, t), INV, who, 'n_modes must be >= 1 (got 0)')
    refused(L.cn_predict_orca_goals, (eng._h, -1, 9, g, t), UNS, who, 'n_modes = 9 exceeds the 8 modes')
    refused(L.cn_predict_orca_goals, (eng._h, -1, 2, g, t), INV, who, 'n_steps must be >= 0 (got -1)')
    refused(L.cn_predict_orca_goals, (None, 2 ** 31 - 1, 8, g, t), INV, who, 'engine is NULL')
    refused(L.cn_predict_orca_goals, (eng._h, 2 ** 31 - 1, 8, g, t), UNS, who, 'rows exceed')
    # zero steps: nothing launched, nothing written
    assert L.cn_predict_orca_goals(eng._h, 0, 2, g, t) == lib.CN_OK
    # cn_goal_hypotheses
    who = 'cn_goal_hypotheses'
    nan = float('nan')
    refused(L.cn_goal_hypotheses, (eng._h, 0, 7, -1.0, -1.0, -1.0, 1, 0, 0, None), INV, who, 'goals is NULL')
    refused(L.cn_goal_hypotheses, (eng._h, 0, 7, -1.0, -1.0, -1.0, 1, 0, 0, g), INV, who, 'n_modes must be >= 1 (got 0)')
    refused(L.cn_goal_hypotheses, (eng._h, 9, 7, -1.0, -1.0, -1.0, 1, 0, 0, g), UNS, who, 'n_modes = 9 exceeds the 8 modes')
    refused(L.cn_goal_hypotheses, (eng._h, 2, 7, -1.0, -1.0, -1.0, 1, 0, 0, g), INV, who, 'base = 7 unknown')
    refused(L.cn_goal_hypotheses, (eng._h, 2, lib.GOALS_HEADING, 0.0, -1.0, -1.0, 1, 0, 0, g), INV, who, 'reach')
    refused(L.cn_goal_hypotheses, (eng._h, 2, lib.GOALS_HEADING, 3.0, nan, -1.0, 1, 0, 0, g), INV, who, 'std_heading')
    refused(L.cn_goal_hypotheses, (eng._h, 2, lib.GOALS_ENGINE, -1.0, 0.4, -1.0, 1, 0, 0, g), INV, who, 'std_distance')
    refused(L.cn_goal_hypotheses, (None, 2, lib.GOALS_ENGINE, -1.0, 0.4, 0.3, 1, 0, 0, g), INV, who, 'engine is NULL')
    eng.sync()
    assert torch.equal(goals, held) and bool((table == -7.0).all()) and eng.launch_counts() == counts
    # through python: the library's refusal arrives as CrowdNavAmdError, the shapes are checked before it is asked
    with pytest.raises(amd.CrowdNavAmdError) as ei:
        eng.goal_hypotheses(2, 'heading', reach=-1.0)
    assert ei.value.status == INV and 'reach' in str(ei.value)
    with pytest.raises(amd.CrowdNavAmdError) as ei:
        eng.goal_hypotheses(2, 'engine', std_distance=-0.5)
    assert ei.value.status == INV and 'std_distance' in str(ei.value)
    for bad in (dict(M=0), dict(M=9), dict(base='track'), dict(out=torch.zeros((B, 3, eng.H, 2), dtype=torch.float64, device=eng.device))):
        with pytest.raises(ValueError, match='goal_hypotheses'):
            eng.goal_hypotheses(**dict(dict(M=2, base='engine'), **bad))
    for bad in (goals[:, 0, 0], goals[:2], torch.zeros((B, 9, eng.H, 2), dtype=torch.float64), np.zeros((B, 2, eng.H, 3))):
        with pytest.raises(ValueError, match='predict_orca_goals: goals must be'):
            eng.predict_orca_goals(4, bad)
    with pytest.raises(ValueError, match='n must be >= 0'):
        eng.predict_orca_goals(-1, goals)
    with pytest.raises(ValueError, match='out must be a contiguous'):
        eng.predict_orca_goals(5, goals, out=table)
    assert eng.predict_orca_goals(4, goals, out=table) is table and bool((table != -7.0).all())


# ------------------------------------------------------------------------------------------------ 6. the example
GOAL_SAMPLES = ['--cases', '8', '--goal-samples', '4', '--goal-base', 'heading', '--goal-std-heading', '0.3', '--reduce', 'min']


@pytest.mark.parametrize('update', ['--cem', '--mppi'])
def test_the_example_plans_on_sampled_goals(amd, update):
    """--goal-samples 4 on 8 test cases under either update: it runs, prints its line, and the same line again from the same
    seed (the sampler's counter is the step)."""
    first = _example_line(GOAL_SAMPLES + [update])
    print(update, first)
    assert _example_line(GOAL_SAMPLES + [update]) == first


def test_the_example_refuses_the_device_loop(amd):
    cmd = [sys.executable, os.path.join(ROOT, 'examples', 'predicted_paths_planner.py')] + GOAL_SAMPLES + ['--device-loop']
    done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    text = done.stdout.decode()
    assert done.returncode == 2 and '--goal-samples runs the per-step loop only' in text and 'TEST' not in text, text
