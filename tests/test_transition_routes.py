"""One hand-built edge scene through every route that makes CrowdSim.step's transition (crowdnav_amd/csrc/transition.h).

The first transition's reward and info depend on the state and the action alone — the swept test reads the velocity a human HAS —
so step(update=False), step(update=True), a one-step rollout_actions (always the generic phase kernel), rollout_step on the
fused kernel and again under CROWDNAV_AMD_FUSED=0 (read from the episode book), lookahead under 'orca' and 'constant_velocity',
lookahead_paths and lookahead_modes (2 equal tables), all with n = 1, must give the reward and info of
lookahead_cv_reference.transition bit for bit, and step and rollout_actions its dmin.  Scenes: the corners of
test_lookahead_cv_host.py — head-on collision, graze inside discomfort_dist, zero relative motion, timeout ahead of a
collision, the three orderings of near / hit / nearer — one env per scene, engines of 1 to 3 humans, holonomic external robot."""
import numpy as np
import pytest

import lookahead_cv_reference as ref
from lookahead_cv_reference import human_row as _human, robot_row as _robot
from support import environ, np_of as _np, same_bits as _same_bits

NEAR, HIT, NEARER = (0.0, -0.65), (0.5, 0.0), (0.0, -0.61)
# name: (human rows, global_time, action, the info worked out by hand)
SCENES = {
    'head_on': ([_human(0.8, 0.0, -1.0, 0.0)], 0.0, (1.0, 0.0), ref.COLLISION),
    'graze': ([_human(0.7, 0.0)], 0.0, (0.0, 1.0), ref.DANGER),
    'zero_relative_motion': ([_human(1.0, 0.0, 0.5, 0.5)], 0.0, (0.5, 0.5), ref.NOTHING),
    'timeout_ahead_of_collision': ([_human(0.8, 0.0, -1.0, 0.0)], ref.CFG['time_limit'] - 1.0, (1.0, 0.0), ref.TIMEOUT),
    'hit_near': ([_human(*HIT), _human(*NEAR)], 0.0, (0.0, 0.0), ref.COLLISION),
    'near_nearer': ([_human(*NEAR), _human(*NEARER)], 0.0, (0.0, 0.0), ref.DANGER),
    'near_hit_nearer': ([_human(*NEAR), _human(*HIT), _human(*NEARER)], 0.0, (0.0, 0.0), ref.COLLISION),
}


def _batches():
    """Per human count: (names, state8 [B][A][8], gtime [B], actions [B][2], want reward / info / dmin [B] from the reference)."""
    out = {}
    for H in (1, 2, 3):
        names = [k for k, v in SCENES.items() if len(v[0]) == H]
        state = np.array([[_robot()] + SCENES[k][0] for k in names], dtype=np.float64)
        gtime = np.array([SCENES[k][1] for k in names], dtype=np.float64)
        actions = np.array([SCENES[k][2] for k in names], dtype=np.float64)
        got = [ref.transition([list(map(float, row)) for row in state[b]], float(gtime[b]), tuple(actions[b]), ref.CFG) for b in range(len(names))]
        want = dict(reward=np.array([g[0] for g in got], dtype=np.float64), info=np.array([g[2] for g in got], dtype=np.uint8),
                    dmin=np.array([g[3] for g in got], dtype=np.float64))
        out[H] = (names, state, gtime, actions, want)
    return out


def test_the_reference_gives_the_infos_worked_out_by_hand():
    for H, (names, _, _, _, want) in _batches().items():
        assert want['info'].tolist() == [SCENES[k][3] for k in names], (H, names)
    b = _batches()
    assert b[2][4]['dmin'].tolist() == [np.inf, (0.61 - 0.3) - 0.3] and b[3][4]['dmin'].tolist() == [(0.65 - 0.3) - 0.3]
    assert b[1][4]['reward'][0] == -0.25 and b[1][4]['reward'][3] == 0.0


BEGIN = dict(seed_base=1000, seed_mod=500, record_capacity=8)


@pytest.mark.gpu
@pytest.mark.parametrize('H', [1, 2, 3])
def test_every_route_makes_the_reference_transition(H):
    import torch
    assert torch.cuda.is_available(), 'gpu tests need a MI355X'
    import crowdnav_amd as amd
    names, state, gtime, actions, want = _batches()[H]
    B = len(names)

    def engine():
        eng = amd.BatchedCrowdSim(num_envs=B, num_humans=H, robot_policy=amd.ROBOT_EXTERNAL)
        eng.set_state(state, gtime)
        return eng

    def check(route, reward, info, dmin=None):
        reward, info = _np(reward).reshape(B), _np(info).reshape(B)
        print(route, names, reward.tolist(), info.tolist())
        assert _same_bits(reward, want['reward']), (route, names, reward, want['reward'])
        assert _same_bits(info, want['info']), (route, names, info, want['info'])
        if dmin is not None:
            assert _same_bits(_np(dmin).reshape(B), want['dmin']), (route, names, _np(dmin), want['dmin'])

    eng = engine()
    for update in (False, True):  # (update=False leaves the state as it is)
        out = eng.step(actions, update=update, want_obs=False)
        check('step(update=%s)' % update, out['reward'], out['info'], out['dmin'])

    # cn_rollout_actions always launches the generic phase kernel (step_core), whatever the geometry and the switch
    table = torch.from_numpy(actions.reshape(B, 1, 2)).to(eng.device).contiguous()
    roll = engine()
    roll.rollout_begin(**BEGIN)
    roll.set_state(state, gtime)
    rows = roll.rollout_actions(table, trace=True, rewards=True)
    check('rollout_actions', rows['reward'], rows['info'], rows['dmin'])

    # rollout_step: the fused kernel (rollout_fused.h: swept_distance, reduce_env) and its CROWDNAV_AMD_FUSED=0 twin on
    # rollout_kernel (step_core).  What the step was is read from the book: an episode that ended left its record in slot 0,
    # a running one its return (table[0] = 1.0: 0.0 + 1.0 * reward), its Danger count and that step's dmin
    for fused, route in ((None, 'fused'), (0, 'generic')):
        with environ(**({} if fused is None else dict(CROWDNAV_AMD_FUSED=fused))):
            roll = engine()
        assert roll.rollout_route(1) == route, (H, fused, roll.rollout_route(1))
        bufs = roll.rollout_begin(**BEGIN)
        roll.set_state(state, gtime)
        roll.rollout_step(table[:, 0].contiguous())
        roll.sync()
        got = {k: _np(v) for k, v in bufs.items()}
        ended = got['ep_count'] == 1
        assert (got['ep_count'] <= 1).all() and (got['cur_steps'][~ended] == 1).all() and (got['ep_steps'][ended, 0] == 1).all()
        reward = np.where(ended, got['ep_return'][:, 0], got['cur_return'])
        info = np.where(ended, got['ep_outcome'][:, 0], np.where(got['cur_danger'] == 1, amd.DANGER, amd.NOTHING)).astype(np.uint8)
        check('rollout_step, %s' % route, torch.from_numpy(reward), torch.from_numpy(info))
        danger = want['info'] == ref.DANGER
        assert _same_bits(got['cur_danger_dmin_sum'][danger], want['dmin'][danger]), (route, got['cur_danger_dmin_sum'], want['dmin'])

    eng = engine()
    look = table.reshape(B, 1, 1, 2).contiguous()  # K = 1, n = 1: ret = 1.0 * reward
    for model in ('orca', 'constant_velocity'):
        eng.set_lookahead_human_model(model)
        got = eng.lookahead(look)
        check('lookahead, ' + model, got['ret'], got['info'])
    vel = torch.from_numpy(state[:, 1:, 2:4].reshape(B, 1, H, 2).copy()).to(eng.device).contiguous()  # the velocity each human has
    got = eng.lookahead_paths(look, vel)
    check('lookahead_paths', got['ret'], got['info'])
    got = eng.lookahead_modes(look, torch.stack([vel, vel], dim=1).contiguous(), per_mode=True)
    for m in range(2):
        check('lookahead_modes, mode %d' % m, got['ret'][:, :, m], got['info'][:, :, m])
