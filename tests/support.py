"""What the test modules share, stated once: the two module fixtures, bit comparisons, engine snapshots, the switches cn_create
reads, action tables, engine and plan factories of the lookahead / planner / predictor suites, and the struct builders of their
host suites.  A plain module, imported like plan_reference and the *_cases modules; torch and crowdnav_amd are imported inside
the functions, so it loads without a GPU.  pytest does not rewrite the assertions of a helper module: each one here names what
failed."""
import contextlib
import ctypes as C
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden

SEED = (0x1234 << 32) | 0x9abcdef1  # the planners' Philox seed
NOWHERE = C.c_void_p(0x10)  # not NULL, not an address of anything
DANGLING = 0x1000  # an address nothing lives at: a refusal must not read through it


# ------------------------------------------------------------------------------------------------ the module fixtures
@pytest.fixture(scope='module')
def amd():
    import torch
    assert torch.cuda.is_available(), 'gpu tests need a MI355X'
    import crowdnav_amd
    return crowdnav_amd


@pytest.fixture(scope='module')
def built():
    import __graft_entry__ as ge
    ge.build()
    from crowdnav_amd import _lib
    return _lib


# ------------------------------------------------------------------------------------------------ tensors, arrays, engine state
def np_of(t):
    return t.detach().cpu().numpy()


def same_bits(got, want):
    """Tensors or arrays: the same dtype, shape and bytes."""
    got, want = np.ascontiguousarray(np_of(got) if hasattr(got, 'detach') else got), np.ascontiguousarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def same_tensors(a, b):
    """Two dicts of tensors: the same keys, and under each key the same dtype and values."""
    import torch
    assert a.keys() == b.keys(), (sorted(a), sorted(b))
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k


def load_params(net, g):
    """A fixture's param_* arrays into `net`."""
    import torch
    net.load_state_dict({k[len('param_'):]: torch.from_numpy(v) for k, v in g.items() if k.startswith('param_')})
    return net


def snapshot(eng):
    eng.sync()
    state, gtime = eng.get_state()
    return state.clone(), gtime.clone(), eng.get_theta().clone()


def restore(eng, snap):
    eng.set_state(snap[0], snap[1])
    eng.set_theta(snap[2])


def assert_twins_equal(x, xbufs, xplan, y, ybufs, yplan):
    """Two engines driven two ways: state, rollout buffers, plan tensors, records and launch counts are the same."""
    import torch
    for name, a, b in zip(('state', 'global_time', 'theta'), snapshot(x), snapshot(y)):
        assert torch.equal(a, b), name
    for k, v in ybufs.items():
        assert torch.equal(v, xbufs[k]), k
    assert sorted(xplan.tensors()) == sorted(yplan.tensors()), (sorted(xplan.tensors()), sorted(yplan.tensors()))
    for k, v in yplan.tensors().items():
        assert torch.equal(v, xplan.tensors()[k]), k
    assert torch.equal(x.rollout_records(), y.rollout_records()), 'rollout_records'
    assert x.launch_counts() == y.launch_counts(), (x.launch_counts(), y.launch_counts())


def put(t, a):
    import torch
    t.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(t.device))


@contextlib.contextmanager
def environ(**values):
    """cn_create reads the engine's switches when the engine is built.  None: unset for the duration."""
    old = {k: os.environ.get(k) for k in values}
    for k, v in values.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = str(v)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


# ------------------------------------------------------------------------------------------------ actions
def action_space(unicycle=False):
    """The value-network policies' 81 actions as [81, 2] float64 (26 (v, r) actions for a unicycle)."""
    from crowdnav_amd.compat.sarl import build_action_space
    space, _, _ = (build_action_space(1.0, 5, 5, 'unicycle') if unicycle else build_action_space(1.0))
    acts = np.array([list(a) for a in space], dtype=np.float64)
    assert len(acts) == (26 if unicycle else 81), len(acts)
    return acts


def action_table(*shape, unicycle=False, seed=11):
    """[*shape, 2] float64: seeded random rows of the action space."""
    acts = action_space(unicycle)
    return acts[np.random.RandomState(seed).randint(len(acts), size=shape)]


# ------------------------------------------------------------------------------------------------ engines and plans
def external_engine(amd, B, H, **cfg):
    """An engine whose robot the caller drives (unless cfg names another robot_policy)."""
    return amd.BatchedCrowdSim(num_envs=B, num_humans=H, robot_policy=cfg.pop('robot_policy', amd.ROBOT_EXTERNAL), **cfg)


def seeded_engine(amd, B=3, H=5, **cfg):
    """external_engine after reset(1000 + arange(B))."""
    eng = external_engine(amd, B, H, **cfg)
    eng.reset(1000 + np.arange(B))
    return eng


def value_network(in_dim):
    """SARL's value network at the shipped widths; in_dim 13, or 61 with the occupancy maps."""
    from crowdnav_amd.compat.sarl import ValueNetwork
    return ValueNetwork(in_dim, 6, [150, 100], [100, 50], [150, 100, 100, 1], [100, 100, 1], True, 1.0, 4)


def configure_sarl(eng, weights=True, with_om=False):
    """SARL on the 81 actions.  weights: True (golden sarl_plain.npz), 'seeded' (torch seed 7) or False (none set); the
    occupancy-map network has no golden weights and takes seeded ones."""
    import torch
    eng.sarl_configure(actions=action_space(), with_om=with_om)
    if with_om or weights == 'seeded':
        torch.manual_seed(7)
        eng.sarl_set_weights(value_network(61 if with_om else 13).state_dict())
    elif weights:
        g = load_golden('sarl_plain.npz')
        eng.sarl_set_weights({k[len('param_'):]: torch.from_numpy(v) for k, v in g.items() if k.startswith('param_')})
    return eng


def sarl_engine(amd, B, H=5, weights=True, with_om=False, **cfg):
    return configure_sarl(seeded_engine(amd, B, H, robot_visible=1, **cfg), weights, with_om)


def begin_plan(eng, K=5, n=4, E=2, I=1, init_std=0.3, mean=None, std=None, **kw):
    """plan_begin under SEED; mean / std written into the plan where given."""
    plan = eng.plan_begin(K, n, E, I, init_std, seed=kw.pop('seed', SEED), **kw)
    if mean is not None:
        put(plan.mean, mean)
    if std is not None:
        put(plan.std, std)
    return plan


def prior_plan(eng, K=5, n=4, E=2, I=1, **kw):
    """A plan at plan_reset's prior, init_std 0.3."""
    return eng.plan_reset(begin_plan(eng, K, n, E, I, **kw))


def smoothed_plan(eng, K=5, n=4, E=2, I=2, **kw):
    return prior_plan(eng, K, n, E, I, smoothing=0.25, min_std=0.01, **kw)


def roll_on(eng, kind, steps):
    import torch
    for _ in range(steps):
        if kind == 'orca_robot':
            eng.rollout(1)
        else:
            eng.rollout_step(torch.tensor([[0.3, 0.2]] * eng.B, dtype=torch.float64, device=eng.device))


def rollout_after(eng, bufs):
    """What a rollout left behind: copies of its bufs, the state, the clock and the heading."""
    eng.sync()
    out = {k: v.clone() for k, v in bufs.items()}
    out['state'], out['global_time'] = eng.get_state()
    out['theta'] = eng.get_theta()
    return out


def rollout_step_loop(eng, bufs, table, snapshots=None):
    """T rollout_step calls on table [B, T, 2]; snapshots (a dict of lists): what every env held before each of them."""
    for t in range(table.shape[1]):
        if snapshots is not None:
            snapshots['state8'].append(eng.get_state()[0])
            for k in ('ep_count', 'cur_steps', 'active'):
                snapshots[k].append(bufs[k].clone())
        eng.rollout_step(table[:, t].contiguous())


def step_loop(eng, seq, gamma=0.9):
    """What the engine's envs do under seq [B, n, 2] from where they stand, by cn_step(update=1): per env the discounted
    return summed left to right on the host, the last info code, the transitions made, global_time, state and heading — all
    taken at the step the env's episode ended (or after n).  The engine is left wherever the n steps took it.  The discount's
    exponent takes the engine's own time_step and robot_v_pref."""
    import math
    import torch
    B, n = seq.shape[:2]
    dt, v_pref = float(eng.config['time_step']), float(eng.config['robot_v_pref'])
    dev = torch.from_numpy(np.ascontiguousarray(seq)).to(eng.device)
    got = dict(ret=np.zeros(B), info=np.zeros(B, np.uint8), steps=np.zeros(B, np.int32), time=np.zeros(B),
               final_state8=np.zeros((B, eng.A, 8)), final_theta=np.zeros(B))
    running = np.ones(B, bool)
    for t in range(n):
        out = eng.step(dev[:, t].contiguous(), update=True, want_obs=False)
        state, gtime = eng.get_state()
        reward, done, info, state, gtime, theta = (np_of(x) for x in (out['reward'], out['done'], out['info'], state, gtime,
                                                                      eng.get_theta()))
        for b in np.flatnonzero(running):
            got['ret'][b] = got['ret'][b] + math.pow(gamma, t * dt * v_pref) * reward[b]
            got['info'][b], got['steps'][b], got['time'][b] = info[b], t + 1, gtime[b]
            got['final_state8'][b], got['final_theta'][b] = state[b], theta[b]
            running[b] = not done[b]
        if not running.any():
            break
    return got


def assert_branch(look, k, want, what=''):
    """Branch (., k) of a lookahead dict (numpy) equals a step_loop result, bit for bit."""
    for key, ref in want.items():
        if key in look:
            got = np.ascontiguousarray(look[key][:, k])
            assert got.dtype == ref.dtype and got.shape == ref.shape and got.tobytes() == ref.tobytes(), (what, key, k, got, ref)


def example_line(args):
    """The TEST line of examples/predicted_paths_planner.py on four cases."""
    cmd = [sys.executable, os.path.join(ROOT, 'examples', 'predicted_paths_planner.py'), '--cases', '4', '--candidates', '8', '--horizon', '4'] + args
    done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    text = done.stdout.decode()
    assert done.returncode == 0, text
    lines = [line.split('INFO: ', 1)[1] for line in text.splitlines() if 'TEST  has success rate:' in line]
    assert len(lines) == 1 and 'collision rate:' in lines[0] and 'total reward:' in lines[0], text
    return lines[0]


# ------------------------------------------------------------------------------------------------ the host suites' structs
def filled(struct, address, **fields):
    """A ctypes struct of pointers with every field at `address`, then `fields`."""
    base = {name: address for name, _ in struct._fields_}
    base.update(fields)
    return struct(**base)


def lookahead_out(lib, **missing):
    """A cn_lookahead_out whose rows address nothing."""
    return filled(lib.CnLookaheadOut, 0x10, **missing)


def host_cfg(lib, **over):
    d = dict(n_steps=4, n_candidates=5, n_elites=2, iterations=1, bootstrap=0, sort_humans=0, init_std=0.5, min_std=0.0,
             smoothing=0.0, seed=1)
    d.update(over)
    return lib.CnPlanCfg(**d)


def host_plan(lib, look_missing=(), **missing):
    """A cn_plan whose rows address nothing; look_missing: rows of its lookahead outputs that are NULL."""
    rows = {name: 0x10 for name, _ in lib.CnPlan._fields_ if name != 'look'}
    rows.update(missing)
    return lib.CnPlan(look=lookahead_out(lib, **dict.fromkeys(look_missing)), **rows)


def models(*values, size=None):
    """int32 model codes, zero-padded to `size` (cn_predictors.model holds 8)."""
    size = len(values) if size is None else size
    return (C.c_int32 * size)(*(list(values) + [0] * (size - len(values))))


def predictors(built, **fields):
    base = dict(n_modes=2, model=models(0, 1, size=8), reduce=built.MODES_MEAN, risk_penalty=0.5, human_vel=DANGLING, weight=DANGLING)
    base.update(fields)
    if not isinstance(base['model'], C.c_int32 * 8):
        base['model'] = models(*base['model'], size=8)
    return built.CnPredictors(**base)


class Recorder(object):
    """The library stubbed: every cn_* symbol records its call and returns CN_OK."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith('cn_'):
            raise AttributeError(name)

        def symbol(*args):
            self.calls.append((name, args))
            return 0
        return symbol
