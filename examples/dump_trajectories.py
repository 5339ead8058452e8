"""Every episode of a phase, step by step: the ORCA-robot evaluation of examples/test_policy.py (the reference's
`test.py --policy orca`, crowd_nav/test.py:14-110) with Explorer.keep_trajectories switched on, written to one .npz file.

    python examples/dump_trajectories.py test.npz                       # the 500 test cases, invisible robot
    python examples/dump_trajectories.py val.npz --phase val --visible  # [robot] visible = true

The whole phase runs as one device batch whose transitions are recorded by cn_rollout_trace.  Keys, in the
packed layout of tests/golden/traj_*.npz:
    states   float64 [sum(steps), A, 8]  the episodes one after another; per episode steps[i] rows, the joint state BEFORE each
                                         transition (px, py, vx, vy, gx, gy, radius, v_pref; agent 0 is the robot) — the
                                         reference's env.states without its last entry (those fixtures carry the final state too)
    steps    int32   [k]                 transitions of episode i
    outcome  uint8   [k]                 2 ReachGoal, 3 Collision, 4 Timeout
    cases    int32   [k]                 case number of episode i inside the phase
Rendering (matplotlib) stays outside the accelerated path."""
import argparse
import logging
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import crowdnav_amd.compat as cn  # noqa: E402


def run(args):
    if args.env_config:
        import configparser
        env_cfg = configparser.RawConfigParser()
        if not env_cfg.read(args.env_config):
            raise SystemExit('cannot read %s' % args.env_config)
    else:
        env_cfg = cn.default_env_config({('robot', 'visible'): 'true' if args.visible else 'false'})
    env = cn.CrowdSim()
    env.configure(env_cfg)
    if args.square:
        env.test_sim = 'square_crossing'
    robot = cn.Robot(env_cfg, 'robot')
    policy = cn.ORCA()
    robot.set_policy(policy)
    env.set_robot(robot)
    policy.set_phase(args.phase)
    policy.safety_space = 0  # test.py:78-85
    policy.set_env(env)
    explorer = cn.Explorer(env, robot, torch.device('cpu'), gamma=0.9)
    explorer.keep_trajectories = True
    first_case = env.case_counter[args.phase]
    k = env.case_size[args.phase] if args.episodes is None else args.episodes
    explorer.run_k_episodes(k, args.phase, print_failure=True)
    lb = explorer.last_batch
    if lb is None or 'trajectories' not in lb:
        raise SystemExit('the batched ORCA path did not run (more episodes than the phase has cases?): nothing recorded')
    np.savez_compressed(args.out, states=np.concatenate(lb['trajectories']), steps=np.asarray(lb['steps'], np.int32),
                        outcome=np.asarray(lb['outcome'], np.uint8), cases=first_case + np.arange(k, dtype=np.int32))
    logging.info('wrote %d trajectories (%d states) to %s', k, sum(lb['steps']), args.out)
    return dict(explorer.last_stats)


def parser():
    ap = argparse.ArgumentParser()
    ap.add_argument('out', metavar='FILE.npz')
    ap.add_argument('--phase', default='test', choices=['val', 'test'])
    ap.add_argument('--episodes', type=int, default=None, help='the first k cases of the phase (default: all of them)')
    ap.add_argument('--env-config', default=None, help="the reference's crowd_nav/configs/env.config")
    ap.add_argument('--visible', action='store_true', help='[robot] visible = true')
    ap.add_argument('--square', action='store_true')
    return ap


if __name__ == '__main__':
    logging.basicConfig(level=logging.INFO, format='%(asctime)s, %(levelname)s: %(message)s', datefmt='%Y-%m-%d %H:%M:%S')
    print(run(parser().parse_args()))
