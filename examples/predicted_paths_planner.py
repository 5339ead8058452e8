"""A planner with a predictor of its own: the test cases driven by the device CEM (or, with --mppi, MPPI) planner whose model
of the humans is neither ORCA (which reads their goals through the simulator) nor "straight on forever", but a table of
predicted velocities the CALLER makes from the state after every real step.

    python examples/predicted_paths_planner.py [--cases 8] [--candidates 16] [--horizon 8] [--cem | --mppi] [--predictor to_goal]
                                               [--futures cv,to_goal [--reduce min] [--risk-penalty 0.5]]
                                               [--device-loop [--chunk 8]] [--orca-sees-plan] [--goal-weight W]
                                               [--goal-samples M [--goal-base heading|engine] [--goal-std-heading S]
                                                [--goal-std-distance S]]

Per real step: read the state, predict (crowdnav_amd.predict.to_goal: every human heads straight for its goal at v_pref and
stops there; or constant_velocity), one plan_cem_paths / plan_mppi_paths call (draw, score against the table, update,
`iterations` times), rollout_step(plan.action), plan_shift.  The prediction goes through the host once per step, which is why
there is no *_rollout form of these calls; the real steps are ORCA, as always.  Prints the success rate, the collision rate
and the navigation time in the reference's format.
--futures plans against several predictors AT ONCE: one plan_cem_modes / plan_mppi_modes call scores every
candidate against each listed future (cv = constant_velocity, to_goal), equally weighted, and ranks the mean of the returns
(--reduce min: the worst one) less --risk-penalty times the share of futures that end in a collision.
--device-loop: the two predictors above also exist on the device (BatchedCrowdSim.predict), so the loop
need not come back to the host: ONE plan_predict_rollout call makes --chunk real steps — predict, plan, step, shift each —
and the host only looks at the rollout between chunks.  The predictor is bit-exact and the counters are the same
(step * iterations), so the line printed is the one the per-step loop prints.
--futures also takes `orca` (once), beside cv and to_goal: the humans avoid EACH OTHER by the engine's own ORCA code but do not
see the robot (BatchedCrowdSim.predict_orca) — a table made on the device in one launch per real step;
with --device-loop the one call is plan_predict_orca_rollout, which writes that future over its slot of the table.
--orca-sees-plan (with --futures ...,orca): the humans of that future DO see the robot, on the plan's nominal sequence — per
real step plan_draw, then BatchedCrowdSim.predict_orca_robot on candidate 0, the clipped mean; with
--device-loop the one call is plan_predict_orca_nominal_rollout.
--goal-weight W (every mode above, --device-loop included) adds W * (metres of progress towards the goal over
the sequence) to every candidate's return under every future (set_lookahead_goal_weight); 0 (the default) is the run without it.
--kinematics unicycle [--max-rotation R] [--rotation-std S] (every mode above): a unicycle robot, the plan a
Gaussian over (v, r) with r clipped to [-R, R] (set_plan_unicycle; R defaults to pi / 4, the reference's action-space bound)
and r's deviation starting at S radians.
--goal-samples M (1 .. 8) replaces the futures by M ORCA futures on SAMPLED human goals: per real step
goal_hypotheses(counter = step) makes M sets of goals on the device — --goal-base heading: twelve steps' walk at v_pref along each
human's velocity, what a planner outside the simulator can observe; engine: the simulator's goals — mode 0 the nominal one, the others
turned by --goal-std-heading z radians and stretched by 1 + --goal-std-distance z; predict_orca_goals steps the humans towards
each set in one launch, and plan_cem_modes / plan_mppi_modes plans against the M futures under --reduce and --risk-penalty.
--goal-weight and --kinematics apply as above.  The per-step loop only: with --device-loop it is refused."""
import argparse
import logging
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import crowdnav_amd  # noqa: E402
import crowdnav_amd.compat as cn  # noqa: E402
from crowdnav_amd import predict  # noqa: E402
from crowdnav_amd.compat.explorer import average, episode_statistics  # noqa: E402


def plan(cases, candidates, horizon, seed=0, gamma=0.9, elites=4, iterations=3, init_std=0.5, temperature=None,
         predictor='to_goal', futures=None, reduce='mean', risk_penalty=0.0, device_loop=False, chunk=8, orca_sees_plan=False,
         goal_weight=0.0, kinematics='holonomic', max_rotation=math.pi / 4, rotation_std=0.5, goal_samples=0, goal_base='heading',
         goal_std_heading=0.0, goal_std_distance=0.0):
    env_cfg = cn.default_env_config()
    env = cn.CrowdSim()
    env.configure(env_cfg)
    robot = cn.Robot(env_cfg, 'robot')
    env.set_robot(robot)
    robot.kinematics = kinematics  # ([robot] policy = none: the planner says what its action rows are, (vx, vy) or (v, r))
    eng = crowdnav_amd.BatchedCrowdSim(**env.engine_config(cases, env.human_num, env.test_sim, crowdnav_amd.ROBOT_EXTERNAL))
    eng.set_gamma(gamma)
    eng.set_lookahead_goal_weight(goal_weight)
    if kinematics == 'unicycle':  # rows (v, r): the rotation bound and r's deviation opt the engine in
        eng.set_plan_unicycle(max_rotation, rotation_std)
    bufs = eng.rollout_begin(seed_base=env.case_capacity['val'], seed_mod=env.case_size['test'], episode_limit=cases,
                             record_capacity=1)
    planner = eng.plan_reset(eng.plan_begin(candidates, horizon, elites, iterations, init_std * robot.v_pref, seed=seed))
    most = int(round(env.time_limit / env.time_step)) + 2  # every episode has ended by then (Timeout)
    orca_mode = futures.index('orca') if futures and 'orca' in futures else None
    if device_loop:  # the closed loop on the device, `chunk` real steps per call; the host looks at the rollout between calls
        # (the ORCA future's slot is first made by a predictor cn_predict knows, then overwritten)
        models = [('to_goal' if name == 'orca' else name) for name in futures] if futures else predictor
        pred = eng.plan_predict_begin(planner, models, reduce=reduce, risk_penalty=risk_penalty)
        for first in range(0, most, chunk):
            if orca_mode is None:
                eng.plan_predict_rollout(planner, pred, min(chunk, most - first), first * iterations, temperature=temperature)
            else:
                loop = eng.plan_predict_orca_nominal_rollout if orca_sees_plan else eng.plan_predict_orca_rollout
                loop(planner, pred, min(chunk, most - first), first * iterations, orca_mode=orca_mode, temperature=temperature)
            if int(bufs['active'].sum().item()) == 0:
                break
    for step in range(0 if device_loop else most):  # the per-step loop through the host (not entered with --device-loop)
        state8, _ = eng.get_state()  # what the planner observes: positions and velocities (to_goal also reads the goals)
        if orca_sees_plan:  # the nominal sequence: candidate 0 of this step's first draw, the mean under the clip rule
            eng.plan_draw(planner, step * iterations)
        tables = {'to_goal': lambda: predict.to_goal(state8, horizon, env.time_step),
                  'constant_velocity': lambda: predict.constant_velocity(state8, horizon),
                  'orca': lambda: (eng.predict_orca_robot(horizon, planner.candidates[:, 0]) if orca_sees_plan
                                   else eng.predict_orca(horizon))}
        if futures or goal_samples:  # several futures side by side, one call
            if goal_samples:  # M ORCA futures on sampled goals, nothing through the host
                goals = eng.goal_hypotheses(goal_samples, goal_base, std_heading=goal_std_heading, std_distance=goal_std_distance,
                                            seed=seed, counter=step)
                human_vel = eng.predict_orca_goals(horizon, goals)
            else:
                human_vel = predict.stack_modes(*(tables[name]() for name in futures))
            if temperature is None:
                eng.plan_cem_modes(planner, human_vel, step * iterations, reduce=reduce, risk_penalty=risk_penalty)
            else:
                eng.plan_mppi_modes(planner, human_vel, temperature, step * iterations, reduce=reduce, risk_penalty=risk_penalty)
        elif temperature is None:
            human_vel = tables[predictor]()
            eng.plan_cem_paths(planner, human_vel, step * iterations)
        else:
            human_vel = tables[predictor]()
            eng.plan_mppi_paths(planner, human_vel, temperature, step * iterations)
        eng.rollout_step(planner.action)
        eng.plan_shift(planner)
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
    ap.add_argument('--candidates', type=int, default=16, help='K: sequences scored per env and iteration')
    ap.add_argument('--horizon', type=int, default=8, help='n: actions per sequence, and steps the humans are predicted for')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--mppi', action='store_true', help='the MPPI update (plan_mppi_paths) instead of the CEM refit (plan_cem_paths)')
    ap.add_argument('--cem', action='store_true', help='the CEM refit, said aloud: it is the default, and excludes --mppi')
    ap.add_argument('--temperature', type=float, default=1.0, help='--mppi: T of the weights exp((score - best score) / T)')
    ap.add_argument('--elites', type=int, default=4, help='CEM: E, candidates the distribution is refitted to')
    ap.add_argument('--iterations', type=int, default=3, help='I, draw / score / update rounds per real step')
    ap.add_argument('--init-std', type=float, default=0.5, help='standard deviation a step starts from, in units of v_pref')
    ap.add_argument('--predictor', default='to_goal', choices=['to_goal', 'constant_velocity'],
                    help="the planner's model of the humans (the real steps are always ORCA)")
    ap.add_argument('--futures', default=None, help='comma-separated predictors (cv, to_goal, orca) to plan against at once, e.g. cv,to_goal')
    ap.add_argument('--reduce', default='mean', choices=['mean', 'min'], help='--futures: rank the mean or the worst of the returns')
    ap.add_argument('--risk-penalty', type=float, default=0.0, help='--futures: subtracted per unit of collision probability')
    ap.add_argument('--device-loop', action='store_true', help='predict on the device too: one plan_predict_rollout call per chunk')
    ap.add_argument('--chunk', type=int, default=8, help='--device-loop: real steps per call')
    ap.add_argument('--orca-sees-plan', action='store_true',
                    help="--futures ...,orca: that future's humans see the robot on the plan's nominal sequence")
    ap.add_argument('--goal-weight', type=float, default=0.0,
                    help="W: every candidate's return gains W per metre of progress towards the goal (0: the discounted return alone)")
    ap.add_argument('--kinematics', default='holonomic', choices=['holonomic', 'unicycle'],
                    help='the robot: action rows (vx, vy), or (v, r) for a unicycle')
    ap.add_argument('--max-rotation', type=float, default=math.pi / 4, help='--kinematics unicycle: R, r is clipped to [-R, R] radians per step')
    ap.add_argument('--rotation-std', type=float, default=0.5,
                    help="--kinematics unicycle: standard deviation r's steps start from, in radians")
    ap.add_argument('--goal-samples', type=int, default=0,
                    help='M in 1..8: plan against M ORCA futures on sampled human goals instead of the futures above (0: off)')
    ap.add_argument('--goal-base', default='heading', choices=['heading', 'engine'],
                    help="--goal-samples: the nominal goal, twelve steps' walk along the human's velocity or the simulator's own")
    ap.add_argument('--goal-std-heading', type=float, default=0.0, help='--goal-samples: deviation of the sampled turn, in radians')
    ap.add_argument('--goal-std-distance', type=float, default=0.0, help='--goal-samples: deviation of the sampled stretch, relative')
    return ap


def main():
    ap = parser()
    args = ap.parse_args()
    names = {'cv': 'constant_velocity', 'constant_velocity': 'constant_velocity', 'to_goal': 'to_goal', 'orca': 'orca'}
    futures = None
    if args.futures:
        unknown = [f for f in args.futures.split(',') if f not in names]
        if unknown:
            ap.error('--futures: unknown predictor(s) %s (cv, to_goal, orca)' % ', '.join(unknown))
        futures = [names[f] for f in args.futures.split(',')]
        if futures.count('orca') > 1:
            ap.error('--futures: orca may be listed once (the closed loop overwrites one slot of the table)')
    if args.device_loop and futures and len(futures) < 2:
        ap.error('--device-loop: --futures takes two or more predictors (one predictor: --predictor)')
    if args.chunk < 1:
        ap.error('--chunk must be >= 1')
    if args.orca_sees_plan and not (futures and 'orca' in futures):
        ap.error('--orca-sees-plan needs --futures with orca in it')
    if args.cem and args.mppi:
        ap.error('--cem and --mppi: one update or the other')
    if args.goal_samples and args.device_loop:
        ap.error('--goal-samples runs the per-step loop only: there is no one-call rollout on sampled goals, drop --device-loop')
    if args.goal_samples and (futures or args.orca_sees_plan):
        ap.error('--goal-samples replaces --futures: give one or the other')
    if not 0 <= args.goal_samples <= 8:
        ap.error('--goal-samples must be in 1 .. 8 (0: off)')
    logging.info(plan(args.cases, args.candidates, args.horizon, args.seed, elites=min(args.elites, args.candidates),
                      iterations=args.iterations, init_std=args.init_std, temperature=args.temperature if args.mppi else None,
                      predictor=args.predictor, futures=futures, reduce=args.reduce, risk_penalty=args.risk_penalty,
                      device_loop=args.device_loop, chunk=args.chunk, orca_sees_plan=args.orca_sees_plan,
                      goal_weight=args.goal_weight, kinematics=args.kinematics, max_rotation=args.max_rotation,
                      rotation_std=args.rotation_std, goal_samples=args.goal_samples, goal_base=args.goal_base,
                      goal_std_heading=args.goal_std_heading, goal_std_distance=args.goal_std_distance))
    return 0


if __name__ == '__main__':
    logging.basicConfig(level=logging.INFO, format='%(asctime)s, %(levelname)s: %(message)s', datefmt='%Y-%m-%d %H:%M:%S')
    sys.exit(main())
