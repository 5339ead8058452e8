"""A random-shooting robot on the reference's test cases: at every real step each env draws K candidate sequences of n actions
from the 81-action table of the value-network policies, scores all of them from its current state with ONE lookahead launch
(cn_lookahead_actions), and takes the first action of its best sequence with rollout_step.

    python examples/shooting_planner.py [--cases 8] [--candidates 16] [--horizon 8] [--seed 0]
    python examples/shooting_planner.py --model-dir DIR [--policy sarl]   # DIR/rl_model.pth (+ DIR/policy.config), as test.py's
    python examples/shooting_planner.py --cem [--elites 4] [--iterations 3] [--init-std 0.5]   # the device CEM planner
    python examples/shooting_planner.py --mppi [--temperature 1.0] [--iterations 3] [--init-std 0.5]   # ... with the MPPI update

The cases run as one batch, one env per case; the line printed at the end is Explorer.run_k_episodes' summary.  A usage
example and a smoke run, not a tuned planner: without --model-dir a candidate's score is its discounted return over the
horizon, nothing else.  With a trained value network the same launch sequence bootstraps it (cn_lookahead_values, DESIGN.md
§3.8.3): score = return + gamma^(steps * time_step * v_pref) * V(state behind the horizon), the n-step return the network's
TD targets mean; a candidate that ended inside the horizon scores its return alone.

--cem runs the same cases with the device planner instead (cn_plan_rollout): per env a Gaussian over action
sequences, K candidates drawn, scored and the Gaussian refitted to the best E of them, I times per real step, the plan carried to
the next step — one plan_rollout call per chunk of steps, with no host work inside a chunk; `active` is read once per chunk.

--mppi is the same loop with the other update (cn_plan_mppi_rollout): every candidate weighted by
exp((score - best score) / T), the mean moved to the weighted mean and its first row taken as the action; the sampling deviation
stays at --init-std.

--human-model constant_velocity (every mode) scores the candidates with humans that keep their current
velocity instead of reacting through ORCA (set_lookahead_human_model): what a planner outside the simulator can assume.  The
real steps stay the simulator's.

--goal-weight W (every mode) adds W * (metres of progress towards the goal over the sequence) to every
candidate's score (set_lookahead_goal_weight): the terminal term without which collision-free candidates that do not arrive
inside the horizon all tie at 0.0.  0 (the default) is the run without it.

--kinematics unicycle [--max-rotation R] [--rotation-std S] (every mode) drives a unicycle robot: action rows
are (v, r).  The random-shooting mode draws from the unicycle action table; --cem / --mppi plan over (v, r) with r clipped to
[-R, R] (set_plan_unicycle; R defaults to pi / 4, the reference's action-space bound) and r's deviation starting at S radians."""
import argparse
import logging
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import crowdnav_amd  # noqa: E402
import crowdnav_amd.compat as cn  # noqa: E402
from crowdnav_amd.compat.explorer import average, episode_statistics  # noqa: E402
from crowdnav_amd.compat.sarl import build_action_space  # noqa: E402


def load_policy(model_dir, name):
    """The value-network policy of a reference output directory: [DIR/policy.config, else the shipped defaults] + DIR/rl_model.pth
    (crowd_nav/test.py:24-40; the conventions of examples/test_policy.py)."""
    import configparser
    from crowdnav_amd.compat.sarl import default_policy_config
    policy = cn.policy_factory[name]()
    if not policy.trainable:
        raise SystemExit('--policy %s has no value network' % name)
    ini = os.path.join(model_dir, 'policy.config')
    if os.path.exists(ini):
        cfg = configparser.RawConfigParser()
        cfg.read(ini)
    else:
        cfg = default_policy_config({})
    policy.configure(cfg)
    weights = os.path.join(model_dir, 'rl_model.pth')
    if not os.path.exists(weights):
        raise SystemExit('cannot read %s' % weights)
    policy.get_model().load_state_dict(torch.load(weights, map_location='cpu'))
    return policy


CEM_CHUNK = 16  # real steps per plan_rollout call: how often the host looks whether every case has ended


def plan(cases, candidates, horizon, seed=0, gamma=0.9, policy=None, cem=None, human_model='orca', goal_weight=0.0,
         kinematics='holonomic', max_rotation=math.pi / 4, rotation_std=0.5):
    env_cfg = cn.default_env_config()
    env = cn.CrowdSim()
    env.configure(env_cfg)
    robot = cn.Robot(env_cfg, 'robot')
    env.set_robot(robot)
    robot.kinematics = kinematics  # ([robot] policy = none: the planner says what its action rows are, (vx, vy) or (v, r))
    eng = crowdnav_amd.BatchedCrowdSim(**env.engine_config(cases, env.human_num, env.test_sim, crowdnav_amd.ROBOT_EXTERNAL))
    eng.set_gamma(gamma)
    eng.set_lookahead_human_model(human_model)
    eng.set_lookahead_goal_weight(goal_weight)
    unicycle = kinematics == 'unicycle'
    if unicycle:  # the planners' rows are (v, r): the rotation bound and r's deviation opt the engine in
        eng.set_plan_unicycle(max_rotation, rotation_std)
    space, _, _ = build_action_space(robot.v_pref, 5, 5, 'unicycle') if unicycle else build_action_space(robot.v_pref)
    rank_by, extra = 'ret', {}
    if policy is not None:  # rank by the bootstrapped n-step return instead
        if policy.kinematics != robot.kinematics:
            raise SystemExit('the policy was configured for a %s robot, the env has a %s one' % (policy.kinematics, robot.kinematics))
        policy.build_action_space(robot.v_pref)
        policy.configure_engine(eng)
        eng.sarl_set_weights(policy.get_model().state_dict())
        rank_by, extra = 'score', dict(bootstrap=True, sort_humans=eng.sarl['model'] == 'lstm_rl')
    table = torch.tensor([list(a) for a in space], dtype=torch.float64, device=eng.device)
    gen = torch.Generator(device=eng.device)
    gen.manual_seed(seed)
    bufs = eng.rollout_begin(seed_base=env.case_capacity['val'], seed_mod=env.case_size['test'], episode_limit=cases,
                             record_capacity=1)
    env_ids = torch.arange(cases, device=eng.device)
    scores = None
    most = int(round(env.time_limit / env.time_step)) + 2  # every episode has ended by then (Timeout)
    if cem is not None:
        planner = eng.plan_begin(candidates, horizon, cem['elites'], cem['iterations'], cem['init_std'] * robot.v_pref, seed=seed,
                                 bootstrap=policy is not None, sort_humans=extra.get('sort_humans', False))
        eng.plan_reset(planner)
        for first in range(0, most, CEM_CHUNK):
            if cem.get('temperature') is None:
                eng.plan_rollout(planner, CEM_CHUNK, first * cem['iterations'])
            else:
                eng.plan_mppi_rollout(planner, CEM_CHUNK, cem['temperature'], first * cem['iterations'])
            if int(bufs['active'].sum().item()) == 0:
                break
        most = 0
    for _ in range(most):
        draw = torch.randint(len(space), (cases, candidates, horizon), generator=gen, device=eng.device)
        sequences = table[draw]  # [cases, K, n, 2], contiguous: read where it lies
        scores = eng.lookahead(sequences, out=scores, **extra)
        best = scores[rank_by].argmax(dim=1)
        eng.rollout_step(sequences[env_ids, best, 0].contiguous())
        if int(bufs['active'].sum().item()) == 0:
            break
    rec = {k: bufs[k].cpu().numpy()[:, 0] for k in ('ep_outcome', 'ep_time', 'ep_return', 'ep_danger', 'ep_danger_dmin_sum')}
    eng.close()
    success, collision, timeout, _, _, _, _, returns = episode_statistics(
        [int(o) for o in rec['ep_outcome']], [float(t) for t in rec['ep_time']], [float(r) for r in rec['ep_return']],
        [int(d) for d in rec['ep_danger']], [float(d) for d in rec['ep_danger_dmin_sum']], timeout_time=env.time_limit)
    assert len(success) + len(collision) + len(timeout) == cases
    return ('{:<5} has success rate: {:.2f}, collision rate: {:.2f}, nav time: {:.2f}, total reward: {:.4f}'.format(
        'TEST', len(success) / cases, len(collision) / cases, average(success) if success else env.time_limit, average(returns)))


def parser():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', type=int, default=8, help='test cases 0 .. cases - 1, one env each')
    ap.add_argument('--candidates', type=int, default=16, help='K: sequences scored per env and step')
    ap.add_argument('--horizon', type=int, default=8, help='n: actions per sequence')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--model-dir', default=None, help="a reference output directory: rl_model.pth and, if present, policy.config")
    ap.add_argument('--policy', default='sarl', choices=['sarl', 'cadrl', 'lstm_rl'], help='the policy --model-dir was trained with')
    how = ap.add_mutually_exclusive_group()
    how.add_argument('--cem', action='store_true', help='plan with the device CEM planner (one plan_rollout call per chunk of steps)')
    how.add_argument('--mppi', action='store_true', help='... with the MPPI update instead (one plan_mppi_rollout call per chunk)')
    ap.add_argument('--temperature', type=float, default=1.0, help='--mppi: T of the weights exp((score - best score) / T)')
    ap.add_argument('--elites', type=int, default=4, help='--cem: E, candidates the distribution is refitted to')
    ap.add_argument('--iterations', type=int, default=3, help='--cem / --mppi: I, draw / score / update rounds per real step')
    ap.add_argument('--init-std', type=float, default=0.5, help='--cem / --mppi: standard deviation a step starts from, in units of v_pref')
    ap.add_argument('--human-model', default='orca', choices=['orca', 'constant_velocity'],
                    help="how the humans move in the planner's lookahead (the real steps are always ORCA)")
    ap.add_argument('--goal-weight', type=float, default=0.0,
                    help="W: every candidate's score gains W per metre of progress towards the goal (0: the discounted return alone)")
    ap.add_argument('--kinematics', default='holonomic', choices=['holonomic', 'unicycle'],
                    help='the robot: action rows (vx, vy), or (v, r) for a unicycle')
    ap.add_argument('--max-rotation', type=float, default=math.pi / 4,
                    help='--kinematics unicycle with --cem / --mppi: R, r is clipped to [-R, R] radians per step')
    ap.add_argument('--rotation-std', type=float, default=0.5,
                    help="--kinematics unicycle with --cem / --mppi: standard deviation r's steps start from, in radians")
    return ap


def main():
    args = parser().parse_args()
    policy = load_policy(args.model_dir, args.policy) if args.model_dir else None
    cem = None
    if args.cem or args.mppi:
        cem = dict(elites=min(args.elites, args.candidates), iterations=args.iterations, init_std=args.init_std,
                   temperature=args.temperature if args.mppi else None)
    logging.info(plan(args.cases, args.candidates, args.horizon, args.seed, policy=policy, cem=cem, human_model=args.human_model,
                      goal_weight=args.goal_weight, kinematics=args.kinematics, max_rotation=args.max_rotation,
                      rotation_std=args.rotation_std))
    return 0


if __name__ == '__main__':
    logging.basicConfig(level=logging.INFO, format='%(asctime)s, %(levelname)s: %(message)s', datefmt='%Y-%m-%d %H:%M:%S')
    sys.exit(main())
