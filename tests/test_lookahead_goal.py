"""The lookahead goal-progress term on the MI355X (include/crowdnav_amd.h, "Lookahead goal-progress term"):
ret' = ret + w * (d0 - d1), added in the kernels of every lookahead route, and what is built on them.

(a) The constant-velocity route against the host restatement.   (b) Every route against its own w = 0 run.
(c) Weight 0 is the lookahead without the term.   (d) The bootstrap.   (e) The modes.   (f) A tie broken.
(g) The planners and the closed loops.   (h) Setter, getter, refusals.

All comparisons are bit for bit.  The scene is written with set_state on B = 4 envs: env 0 has the robot 0.6 m from its goal
(ReachGoal inside the horizon), env 1 a human 0.9 m straight ahead walking at the robot (Collision for the forward candidates),
env 2 an open field (every branch runs the horizon), env 3 the scenario reset generated.  K = 70: two workgroups per env in the
lane-per-branch kernels, the second with a 6-lane tail; n = 6."""
import ctypes as C
import math

import numpy as np
import pytest

from conftest import load_golden

import lookahead_cv_reference as cv_ref
import lookahead_modes_reference as modes_ref
from lookahead_goal_reference import goal_term
from support import (  # noqa: F401  (amd: module fixture)
    amd, assert_twins_equal as _assert_loops_equal, np_of as _np, same_bits as _same_bits, snapshot as _snapshot)

pytestmark = pytest.mark.gpu

B, K, N = 4, 70, 6
BEGIN = dict(seed_base=1000, seed_mod=500, record_capacity=8)
DT, V_PREF, GAMMA = 0.25, 1.0, 0.9
CV, ORCA = 'constant_velocity', 'orca'
ROWS = ('info', 'steps', 'time', 'final_state8', 'final_theta')  # what the term leaves alone
WEIGHTS = (0.1, 0.25)
KINDS = {'holonomic': dict(), 'unicycle': dict(robot_kinematics=1), 'mixed': dict(scenario_rule=2)}


# ------------------------------------------------------------------------------------------------ the scene
def _scene_rows(H):
    """[3, H + 1, 8]: envs 0 .. 2 of the scene.  The humans that play no part stand 1.5 m apart, 8 m and more from every robot,
    at their own goals."""
    rows = np.zeros((3, H + 1, 8))
    for h in range(H):
        x = 8.0 + 1.5 * h
        rows[:, h + 1] = (x, 8.0, 0.0, 0.0, x, 8.0, 0.3, 1.0)
    rows[0, 0] = (0.0, 0.0, 0.0, 0.0, 0.0, 0.6, 0.3, 1.0)   # 0.6 m from the goal: the second forward step arrives
    rows[1, 0] = (0.0, 0.0, 0.0, 0.0, 0.0, 8.0, 0.3, 1.0)
    rows[1, 1] = (0.0, 0.9, 0.0, -1.0, 0.0, -5.0, 0.3, 1.0)  # 0.9 m ahead, walking at the robot, its goal behind the robot
    rows[2, 0] = (0.0, -4.0, 0.0, 0.0, 0.0, 4.0, 0.3, 1.0)  # the open field of a circle crossing without the crowd
    return rows


def _put_scene(eng):
    """reset, then the scene over envs 0 .. 2; env 3 keeps what reset generated.  Returns (state8, gtime) as numpy."""
    eng.reset(1000 + np.arange(B))
    state, gtime = (_np(x).copy() for x in eng.get_state())
    state[:3], gtime[:3] = _scene_rows(eng.H), 0.0
    eng.set_state(state, gtime)
    eng.set_theta(np.full(B, math.pi / 2))  # (read by unicycle engines only: heading along +y, towards the goals)
    got, _ = eng.get_state()
    assert _same_bits(got, state)
    return state, gtime


def _scene_engine(amd, kind='holonomic', H=5, **more):
    eng = amd.BatchedCrowdSim(num_envs=B, num_humans=H, robot_policy=amd.ROBOT_EXTERNAL, **dict(KINDS[kind], **more))
    state, gtime = _put_scene(eng)
    return eng, state, gtime


def _table(kind='holonomic', k=K, n=N):
    """[B, k, n, 2]: candidate 0 walks straight ahead at full speed, candidate 1 stands, the rest are random rows of the
    action space."""
    if kind != 'unicycle':
        return modes_ref.action_table(B, k, n)
    from crowdnav_amd.compat.sarl import build_action_space
    space = np.array([list(a) for a in build_action_space(1.0, 5, 5, 'unicycle')[0]], dtype=np.float64)
    table = space[np.random.RandomState(11).randint(len(space), size=(B, k, n))]
    table[:, 0], table[:, 1] = (1.0, 0.0), (0.0, 0.0)
    return table


def _human_vel(state, n=N, seed=5):
    """lookahead_paths' table: every human starts from its own velocity and turns a little every step."""
    return modes_ref.turning(state, n, seed)


def _run(eng, route, table, vel=None, **kw):
    """One lookahead by `route`: lookahead() under 'orca' or 'constant_velocity', or lookahead_paths() with vel."""
    if route == 'paths':
        out = eng.lookahead_paths(table, vel, **kw)
    else:
        eng.set_lookahead_human_model(ORCA if route == 'orca' else CV)
        out = eng.lookahead(table, **kw)
    return {k: _np(v) for k, v in out.items()}


def _assert_every_path_is_taken(amd, out, n=N):
    info, steps = out['info'], out['steps']
    horizon = (info < amd.REACH_GOAL) & (steps == n)
    assert (info == amd.REACH_GOAL).any() and (info == amd.COLLISION).any() and horizon.any(), np.bincount(info.ravel(), minlength=5)
    assert ((info >= amd.REACH_GOAL) & (steps < n)).any()


def _terms(w, state, end_xy):
    """goal_term of every branch: state [B, A, 8] the engine's, end_xy [B, K, 2] the robots' positions after the last transition."""
    out = np.zeros(end_xy.shape[:2])
    for b in range(end_xy.shape[0]):
        for k in range(end_xy.shape[1]):
            out[b, k] = goal_term(w, state[b, 0, 0:2], state[b, 0, 4:6], end_xy[b, k])
    return out


# ------------------------------------------------------------------------------------------------ (a) the host restatement
@pytest.mark.parametrize('H', [5, 1])
def test_constant_velocity_route_against_the_restatement(amd, H):
    eng, state, gtime = _scene_engine(amd, H=H)
    table = _table()
    cfg = {k: float(eng.config[k]) for k in cv_ref.CFG}
    want = cv_ref.lookahead(state, gtime, table, cfg, GAMMA)
    assert eng.lookahead_goal_weight == 0.0
    plain = _run(eng, 'cv', table, final_state=True)
    _assert_every_path_is_taken(amd, plain)
    assert _same_bits(plain['ret'], want['ret']) and _same_bits(plain['final_state8'], want['final_state8'])
    for w in WEIGHTS:
        eng.set_lookahead_goal_weight(w)
        got = _run(eng, 'cv', table, final_state=True)
        want_ret = want['ret'] + _terms(w, state, want['final_state8'][:, :, 0, 0:2])  # from the restatement's own end points
        assert _same_bits(got['ret'], want_ret), (H, w, got['ret'] - want_ret)
        assert not _same_bits(got['ret'], plain['ret'])
        for key in ROWS:
            assert _same_bits(got[key], plain[key]), (H, w, key)
    # the forward candidate of the open field: 6 steps of 0.25 m, every figure exact
    assert got['ret'][2, 0] == 0.25 * 1.5 and plain['ret'][2, 0] == 0.0


# ------------------------------------------------------------------------------------------------ (b) every route
ROUTES = [(kind, 5, route) for kind in ('holonomic', 'unicycle', 'mixed') for route in ('orca', 'cv', 'paths')] + [('holonomic', 12, 'orca')]


@pytest.mark.parametrize('kind,H,route', ROUTES)
def test_every_route_against_its_own_run_without_the_term(amd, kind, H, route):
    eng, state, gtime = _scene_engine(amd, kind, H)
    table, vel = _table(kind), _human_vel(state)
    if kind == 'mixed':
        vel[np.broadcast_to((state[:, 1:, 0] >= 1.0e5)[:, None, :], vel.shape[:3])] = 0.0  # the parked placeholders' rows
    plain = _run(eng, route, table, vel, final_state=True)
    _assert_every_path_is_taken(amd, plain)
    bare = _run(eng, route, table, vel)
    assert _same_bits(bare['ret'], plain['ret'])
    for w in WEIGHTS:
        eng.set_lookahead_goal_weight(w)
        assert eng.lookahead_goal_weight == w
        got = _run(eng, route, table, vel, final_state=True)
        # d0 from get_state(), d1 from the robot row of the SAME call's final_state8; one float64 add of the rounded term ...
        want_ret = plain['ret'] + _terms(w, state, got['final_state8'][:, :, 0, 0:2])
        assert _same_bits(got['ret'], want_ret), (kind, H, route, w, np.abs(got['ret'] - want_ret).max())
        assert not _same_bits(got['ret'], plain['ret'])
        for key in ROWS:
            assert _same_bits(got[key], plain[key]), (kind, H, route, w, key)
        # ... and ret does not depend on which optional outputs are asked for
        bare = _run(eng, route, table, vel)
        assert sorted(bare) == ['info', 'ret', 'steps', 'time']
        for key in bare:
            assert _same_bits(bare[key], got[key]), (kind, H, route, w, key)
    # nothing of the engine moved
    after, gafter = eng.get_state()
    assert _same_bits(after, state) and _same_bits(gafter, gtime)


# ------------------------------------------------------------------------------------------------ (c) weight 0 is today
def _modes_tables(state, n=N):
    """[B, 3, n, H, 2]: mode 0 every human keeps its velocity, mode 1 walks to its goal, mode 2 walks off along +y from the
    first step on — the human of env 1 then walks away from the robot instead of into it."""
    from crowdnav_amd import predict
    away = np.zeros((B, n, state.shape[1] - 1, 2))
    away[..., 1] = 1.0
    return predict.stack_modes(predict.constant_velocity(state, n), predict.to_goal(state, n, DT), away)


def test_weight_zero_is_the_lookahead_without_the_term(amd):
    never, state, _ = _scene_engine(amd)
    back, _, _ = _scene_engine(amd)
    table, vel, mvel = _table(), _human_vel(state), _modes_tables(state)
    back.set_lookahead_goal_weight(0.1)
    with_term = {route: _run(back, route, table, vel, final_state=True) for route in ('orca', 'cv', 'paths')}
    with_term['modes'] = {k: _np(v) for k, v in back.lookahead_modes(table, mvel, per_mode=True).items()}
    for zero in (0.0, -0.0):
        back.set_lookahead_goal_weight(zero)
        assert back.lookahead_goal_weight == 0.0
        for route in ('orca', 'cv', 'paths'):
            want, got = _run(never, route, table, vel, final_state=True), _run(back, route, table, vel, final_state=True)
            assert sorted(got) == sorted(want)
            for key in want:
                assert _same_bits(got[key], want[key]), (route, key)
            assert not _same_bits(with_term[route]['ret'], want['ret']), route
        want = {k: _np(v) for k, v in never.lookahead_modes(table, mvel, per_mode=True).items()}
        got = {k: _np(v) for k, v in back.lookahead_modes(table, mvel, per_mode=True).items()}
        assert sorted(got) == sorted(want)
        for key in want:
            assert _same_bits(got[key], want[key]), ('modes', key)
        assert not _same_bits(with_term['modes']['ret'], want['ret']) and not _same_bits(with_term['modes']['score'], want['score'])


# ------------------------------------------------------------------------------------------------ (d) the bootstrap
def _sarl_scene_engine(amd):
    import torch
    from crowdnav_amd.compat.sarl import build_action_space
    eng = amd.BatchedCrowdSim(num_envs=B, num_humans=5, robot_policy=amd.ROBOT_EXTERNAL)
    eng.reset(1000 + np.arange(B))
    eng.sarl_configure(actions=np.array([list(a) for a in build_action_space(1.0)[0]], dtype=np.float64))
    g = load_golden('sarl_plain.npz')
    eng.sarl_set_weights({k[len('param_'):]: torch.from_numpy(v) for k, v in g.items() if k.startswith('param_')})
    state, gtime = _put_scene(eng)
    return eng, state, gtime


@pytest.mark.parametrize('route', ['orca', 'cv', 'paths'])
def test_bootstrap_scores_take_the_term_and_values_do_not(amd, route):
    eng, state, _ = _sarl_scene_engine(amd)
    table, vel = _table(), _human_vel(state)
    plain = _run(eng, route, table, vel, bootstrap=True)
    _assert_every_path_is_taken(amd, plain)
    for w in WEIGHTS:
        eng.set_lookahead_goal_weight(w)
        got = _run(eng, route, table, vel, bootstrap=True)
        for key in ROWS + ('value',):
            assert _same_bits(got[key], plain[key]), (route, w, key)
        want_ret = plain['ret'] + _terms(w, state, got['final_state8'][:, :, 0, 0:2])
        assert _same_bits(got['ret'], want_ret), (route, w)
        ended = got['info'] >= amd.REACH_GOAL
        assert ended.any() and not ended.all()
        for b in range(B):
            for k in range(K):
                boot = math.pow(GAMMA, int(got['steps'][b, k]) * DT * V_PREF) * float(np.float64(got['value'][b, k]))
                score = got['ret'][b, k] if ended[b, k] else got['ret'][b, k] + boot
                assert _same_bits(got['score'][b, k], np.float64(score)), (route, w, b, k)
        assert not _same_bits(got['score'], plain['score'])


# ------------------------------------------------------------------------------------------------ (e) the modes
@pytest.mark.parametrize('kind', ['holonomic', 'unicycle'])
def test_modes_take_the_term_per_mode_before_the_reduction(amd, kind):
    M = 3
    eng, state, _ = _scene_engine(amd, kind)
    table, mvel = _table(kind), _modes_tables(state)
    weights = modes_ref.weights_table(B, M)
    plain = {k: _np(v) for k, v in eng.lookahead_modes(table, mvel, per_mode=True).items()}
    _assert_every_path_is_taken(amd, plain)
    # the standing candidate of env 1: walked into at the second step where the human keeps coming, never where it turns away
    assert plain['steps'][1, 1].tolist() == [2, 2, N] and plain['info'][1, 1, 0] == amd.COLLISION
    assert (plain['steps'].max(-1) != plain['steps'].min(-1)).any()
    for w in WEIGHTS:
        eng.set_lookahead_goal_weight(w)
        rows = None
        for wt in (None, weights):
            for reduce in (modes_ref.MEAN, modes_ref.MIN):
                for penalty in (0.0, 0.5):
                    got = {k: _np(v) for k, v in eng.lookahead_modes(table, mvel, weights=wt, reduce=reduce, risk_penalty=penalty,
                                                                     per_mode=True).items()}
                    if rows is None:  # every mode's row is lookahead_paths with that mode's table under the same weight
                        rows = {key: got[key] for key in ('ret', 'info', 'steps', 'time')}
                        for m in range(M):
                            want = _run(eng, 'paths', table, np.ascontiguousarray(mvel[:, m]))
                            for key in rows:
                                assert _same_bits(rows[key][:, :, m], want[key]), (kind, w, m, key)
                        assert not _same_bits(rows['ret'], plain['ret'])
                        for key in ('info', 'steps', 'time'):
                            assert _same_bits(rows[key], plain[key]), (kind, w, key)
                    for key in rows:
                        assert _same_bits(got[key], rows[key]), (kind, w, key)
                    want = modes_ref.reduced(rows, wt, reduce, penalty)  # the header's reduction, in its order
                    for key in want:
                        assert _same_bits(got[key], want[key]), (kind, w, wt is None, reduce, penalty, key)
                    short = {k: _np(v) for k, v in eng.lookahead_modes(table, mvel, weights=wt, reduce=reduce,
                                                                       risk_penalty=penalty).items()}
                    for key in want:
                        assert _same_bits(short[key], want[key]), (kind, w, key)
        if w == WEIGHTS[0]:  # the term moves the reduction somewhere, the worst mode included
            assert not _same_bits(got['score'], modes_ref.reduced(plain, weights, modes_ref.MIN, 0.5)['score'])


# ------------------------------------------------------------------------------------------------ (f) a tie broken
def test_the_term_breaks_the_tie_between_towards_and_away(amd):
    import torch
    eng, state, _ = _scene_engine(amd)
    table = np.zeros((B, 2, N, 2))
    table[:, 0, :, 1], table[:, 1, :, 1] = -1.0, 1.0  # candidate 0 straight away from the goal, candidate 1 straight at it
    plan = eng.plan_begin(2, N, 1, 1, 0.3)
    plan.candidates.copy_(torch.from_numpy(table))
    for route in ('cv', 'orca'):
        eng.set_lookahead_goal_weight(0.0)
        plain = _run(eng, route, table, final_state=True)
        assert plain['ret'][2].tolist() == [0.0, 0.0] and plain['steps'][2].tolist() == [N, N]  # the tie
        eng.lookahead(plan.candidates, out=plan.look)
        eng.plan_refit(plan)
        assert _np(plan.order)[2].tolist() == [0, 1] and _np(plan.action)[2].tolist() == [0.0, -1.0]  # broken by index: away
        eng.set_lookahead_goal_weight(0.25)
        got = _run(eng, route, table, final_state=True)
        d0 = cv_ref.norm2(0.0 - 0.0, -4.0 - 4.0)
        d1_away, d1_toward = (cv_ref.norm2(x - 0.0, y - 4.0) for x, y in got['final_state8'][2, :, 0, 0:2])
        assert (d0, d1_away, d1_toward) == (8.0, 9.5, 6.5)
        assert got['ret'][2].tolist() == [0.25 * (d0 - d1_away), 0.25 * (d0 - d1_toward)]
        assert got['ret'][2, 1] - got['ret'][2, 0] == 0.25 * (d1_away - d1_toward) == 0.75
        eng.lookahead(plan.candidates, out=plan.look)
        eng.plan_refit(plan)
        assert _np(plan.order)[2].tolist() == [1, 0] and _np(plan.action)[2].tolist() == [0.0, 1.0]  # the goal-ward one


# ------------------------------------------------------------------------------------------------ (g) planners, closed loops
def _ranked(ret):
    """The candidate index at every rank: by decreasing score, ties by candidate index."""
    return np.stack([np.argsort(-row, kind='stable') for row in ret]).astype(np.int32)


@pytest.mark.parametrize('model', [ORCA, CV])
@pytest.mark.parametrize('update', ['cem', 'mppi'])
def test_a_planning_step_ranks_the_returns_with_the_term(amd, update, model):
    k, n, I, counter = 16, N, 2, 21
    eng, state, _ = _scene_engine(amd)
    eng.set_lookahead_human_model(model)
    plans = {}
    for w in (0.0, 0.1):
        eng.set_lookahead_goal_weight(w)
        plan = plans[w] = eng.plan_reset(eng.plan_begin(k, n, 4, I, 0.3, seed=5, smoothing=0.25, min_std=0.01))
        if update == 'cem':
            eng.plan_cem(plan, counter)
        else:
            eng.plan_mppi(plan, 0.7, counter)
        want = _run(eng, model, _np(plan.candidates), final_state=True)
        assert _same_bits(plan.look['ret'], want['ret']), (update, model, w)
        assert _same_bits(plan.order, _ranked(want['ret'])), (update, model, w)
        # best_score is the best over the I iterations (a later one replaces it only by a strictly better score)
        assert (_np(plan.best_score) >= want['ret'][np.arange(B), _np(plan.order)[:, 0]]).all()
    ret0 = _np(plans[0.0].look['ret'])
    # without the term the open field's candidates all score 0.0; with it none of them ties with the best
    assert (ret0[2] == 0.0).all() and _np(plans[0.0].order)[2].tolist() == list(range(k))
    ret = _np(plans[0.1].look['ret'])
    assert (ret[2] != 0.0).any() and (ret[2] == ret[2].max()).sum() == 1


def _closed_loop_twins(amd, count):
    made = []
    for _ in range(count):
        # time_limit 1.5 s: the third real step ends every env's first episode in Timeout, so ep_return is written
        eng = amd.BatchedCrowdSim(num_envs=B, num_humans=5, robot_policy=amd.ROBOT_EXTERNAL, time_limit=1.5)
        eng.reset(1000 + np.arange(B))
        bufs = eng.rollout_begin(**BEGIN)
        made.append((eng, bufs, eng.plan_reset(eng.plan_begin(16, N, 4, 2, 0.3, seed=5, smoothing=0.25, min_std=0.01))))
    return made


def _assert_real_steps_know_nothing_of_the_term(x, xbufs, z, zbufs, actions):
    """z never heard of the weight: the same actions through rollout_actions give the same states, rewards and books."""
    import torch
    z.rollout_actions(torch.stack(actions, dim=1).contiguous())
    for a, b in zip(_snapshot(x), _snapshot(z)):
        assert torch.equal(a, b)
    for k, v in zbufs.items():
        assert torch.equal(v, xbufs[k]), k
    assert torch.equal(x.rollout_records(), z.rollout_records())
    assert (_np(xbufs['ep_count']) >= 1).all()  # (ep_return holds a finished episode of every env)


@pytest.mark.parametrize('model', [ORCA, CV])
def test_plan_rollout_is_the_python_loop_under_the_term(amd, model):
    import torch
    steps, I, counter = 3, 2, 100
    (x, xbufs, xplan), (y, ybufs, yplan), (z, zbufs, _), (p, pbufs, pplan) = _closed_loop_twins(amd, 4)
    for eng in (x, y, p):
        eng.set_lookahead_human_model(model)
    x.set_lookahead_goal_weight(0.1), y.set_lookahead_goal_weight(0.1)
    assert x.plan_rollout(xplan, steps, counter) is xbufs
    actions = []
    for s in range(steps):
        y.plan_cem(yplan, counter + s * I)
        actions.append(yplan.action.clone())
        y.rollout_step(yplan.action)
        y.plan_shift(yplan)
    _assert_loops_equal(x, xbufs, xplan, y, ybufs, yplan)
    _assert_real_steps_know_nothing_of_the_term(x, xbufs, z, zbufs, actions)
    assert x.lookahead_goal_weight == 0.1  # reset, the rollout calls and the planner leave it
    # the setting reached the loop: the same loop without the term scored its candidates otherwise
    p.plan_rollout(pplan, steps, counter)
    assert not torch.equal(pplan.look['ret'], xplan.look['ret'])


@pytest.mark.parametrize('update', [None, dict(temperature=0.7, fit_std=True)])
def test_plan_predict_rollout_is_the_python_loop_under_the_term(amd, update):
    import torch
    steps, I, counter, models = 3, 2, 100, ('cv', 'to_goal')
    (x, xbufs, xplan), (y, ybufs, yplan), (z, zbufs, _), (p, pbufs, pplan) = _closed_loop_twins(amd, 4)
    x.set_lookahead_goal_weight(0.1), y.set_lookahead_goal_weight(0.1)
    kw = dict(reduce='min', risk_penalty=0.5)
    pred = x.plan_predict_begin(xplan, models, **kw)
    assert x.plan_predict_rollout(xplan, pred, steps, counter, **(update or {})) is xbufs
    actions = []
    for s in range(steps):
        vel = y.predict(N, models)
        if update is None:
            y.plan_cem_modes(yplan, vel, counter + s * I, **kw)
        else:
            y.plan_mppi_modes(yplan, vel, update['temperature'], counter + s * I, fit_std=update['fit_std'], **kw)
        actions.append(yplan.action.clone())
        y.rollout_step(yplan.action)
        y.plan_shift(yplan)
    _assert_loops_equal(x, xbufs, xplan, y, ybufs, yplan)
    _assert_real_steps_know_nothing_of_the_term(x, xbufs, z, zbufs, actions)
    ppred = p.plan_predict_begin(pplan, models, **kw)
    p.plan_predict_rollout(pplan, ppred, steps, counter, **(update or {}))
    assert not torch.equal(pplan.look['ret'], xplan.look['ret'])


# ------------------------------------------------------------------------------------------------ (h) setter, getter, refusals
def test_setter_getter_and_refusals(amd):
    from crowdnav_amd import _lib
    eng, state, _ = _scene_engine(amd)
    L = _lib.load()
    assert eng.lookahead_goal_weight == 0.0  # what cn_create installs
    eng.set_lookahead_goal_weight(0.25)
    assert eng.lookahead_goal_weight == 0.25
    for bad, shown in ((math.nan, 'nan'), (-1.0, '-1'), (math.inf, 'inf')):
        with pytest.raises(amd.CrowdNavAmdError) as ei:
            eng.set_lookahead_goal_weight(bad)
        assert ei.value.status == _lib.CN_ERR_INVALID and 'cn_lookahead_set_goal_weight' in str(ei.value) and shown in str(ei.value)
        assert eng.lookahead_goal_weight == 0.25  # left as it was
    assert L.cn_lookahead_get_goal_weight(eng._h, None) == _lib.CN_ERR_INVALID
    assert 'cn_lookahead_get_goal_weight: weight_host is NULL' in L.cn_last_error().decode()
    with pytest.raises(AttributeError):
        eng.lookahead_goal_weight = 0.5
    eng.reset(1000 + np.arange(B))
    assert eng.lookahead_goal_weight == 0.25  # cn_reset does not change it
    # accepted on an engine no lookahead serves, where it touches nothing
    orca = amd.BatchedCrowdSim(num_envs=2, num_humans=5, robot_policy=amd.ROBOT_ORCA)
    orca.set_lookahead_goal_weight(0.5)
    assert orca.lookahead_goal_weight == 0.5
    # the gym surface forwards it to the episode's engine
    from crowdnav_amd.compat.crowd_sim import CrowdSim
    assert isinstance(CrowdSim.lookahead_goal_weight, property) and callable(CrowdSim.set_lookahead_goal_weight)
