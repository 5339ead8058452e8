"""A random-shooting robot on the reference's test cases: at every real step each env draws K candidate sequences of n actions
from the 81-action table of the value-network policies, scores all of them from its current state with ONE lookahead launch
(cn_lookahead_actions), and takes the first action of its best sequence with rollout_step.

    python examples/shooting_planner.py [--cases 8] [--candidates 16] [--horizon 8] [--seed 0]

The cases run as one batch, one env per case; the line printed at the end is Explorer.run_k_episodes' summary.  A usage
example and a smoke run, not a tuned planner: a candidate's score is its discounted return over the horizon, nothing else."""
import argparse
import logging
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import crowdnav_amd  # noqa: E402
import crowdnav_amd.compat as cn  # noqa: E402
from crowdnav_amd.compat.explorer import average, episode_statistics  # noqa: E402
from crowdnav_amd.compat.sarl import build_action_space  # noqa: E402


def plan(cases, candidates, horizon, seed=0, gamma=0.9):
    env_cfg = cn.default_env_config()
    env = cn.CrowdSim()
    env.configure(env_cfg)
    robot = cn.Robot(env_cfg, 'robot')
    env.set_robot(robot)
    if robot.kinematics is None:  # ([robot] policy = none: the planner's actions are (vx, vy))
        robot.kinematics = 'holonomic'
    eng = crowdnav_amd.BatchedCrowdSim(**env.engine_config(cases, env.human_num, env.test_sim, crowdnav_amd.ROBOT_EXTERNAL))
    eng.set_gamma(gamma)
    space, _, _ = build_action_space(robot.v_pref)
    table = torch.tensor([list(a) for a in space], dtype=torch.float64, device=eng.device)
    gen = torch.Generator(device=eng.device)
    gen.manual_seed(seed)
    bufs = eng.rollout_begin(seed_base=env.case_capacity['val'], seed_mod=env.case_size['test'], episode_limit=cases,
                             record_capacity=1)
    env_ids = torch.arange(cases, device=eng.device)
    scores = None
    for _ in range(int(round(env.time_limit / env.time_step)) + 2):  # every episode has ended by then (Timeout)
        draw = torch.randint(len(space), (cases, candidates, horizon), generator=gen, device=eng.device)
        sequences = table[draw]  # [cases, K, n, 2], contiguous: read where it lies
        scores = eng.lookahead(sequences, out=scores)
        best = scores['ret'].argmax(dim=1)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', type=int, default=8, help='test cases 0 .. cases - 1, one env each')
    ap.add_argument('--candidates', type=int, default=16, help='K: sequences scored per env and step')
    ap.add_argument('--horizon', type=int, default=8, help='n: actions per sequence')
    ap.add_argument('--seed', type=int, default=0)
    args = ap.parse_args()
    logging.info(plan(args.cases, args.candidates, args.horizon, args.seed))
    return 0


if __name__ == '__main__':
    logging.basicConfig(level=logging.INFO, format='%(asctime)s, %(levelname)s: %(message)s', datefmt='%Y-%m-%d %H:%M:%S')
    sys.exit(main())
