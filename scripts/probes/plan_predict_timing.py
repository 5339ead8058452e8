"""What the closed loop on the device predictors saves: ONE plan_predict_rollout call (cn_plan_cem_predict_rollout) making `--steps`
closed-loop steps, against the per-step loop examples/predicted_paths_planner.py ran before it — get_state, predict.to_goal in
torch on the device state, plan_cem_paths (with --modes 2: predict.constant_velocity + to_goal, stack_modes, plan_cem_modes),
rollout_step, plan_shift and the example's look at bufs['active'] — alternating in one process.

    python scripts/probes/plan_predict_timing.py [--envs 4096] [--steps 4] [--modes 1] [--reps 20] [--no-poll]
                                                 [--out profiles/plan_predict_timing.txt]
    python scripts/probes/plan_predict_timing.py --kernel [--envs 4096] [--modes 1]     (under rocprofv3 --kernel-trace --stats)

--envs envs x 5 humans, external holonomic robot, K = 64 candidates, n = 12 steps, I = 3 iterations, E = 8 elites, init_std 0.5.
After one warm-up round, --reps rounds of (per-step loop, one call); each is timed by the host clock from its first call to the
end of a device synchronise.  Both engines start from the same seeds and the device predictor is bit-exact, so the two plan the
same trajectories with the same counters.  --no-poll drops the loop's bufs['active'].sum().item() per step (a synchronise the
example makes and a caller need not).  Prints median and standard deviation of both and whether the one-call form is no slower
than the loop by more than three pooled standard deviations, sqrt((sd_a^2 + sd_b^2) / 2).
--kernel: 50 predict() launches and 50 device copies of the bytes one launch writes (B M n H 16), each timed with device events
around the 50; run under the profiler for predict_kernel's own duration."""
import argparse
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

H, K, N, I, E, INIT_STD = 5, 64, 12, 3, 8, 0.5
MODELS = {1: ('to_goal',), 2: ('cv', 'to_goal')}


def kernel_only(crowdnav_amd, B, M, out):
    eng = crowdnav_amd.BatchedCrowdSim(num_envs=B, num_humans=H, robot_policy=crowdnav_amd.ROBOT_EXTERNAL, robot_visible=1)
    eng.reset(1000 + np.arange(B))
    table = eng.predict(N, MODELS[M])
    other = torch.empty_like(table)
    lines = []
    for name, call in (('predict()', lambda: eng.predict(N, MODELS[M], out=table)), ('device copy of the table', lambda: other.copy_(table))):
        for _ in range(5):
            call()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(50):
            call()
        end.record()
        torch.cuda.synchronize()
        lines.append('%-26s %9.2f us per launch (device events around 50 launches, launch gaps included)' % (name, start.elapsed_time(end) * 1e3 / 50))
    text = '\n'.join(['plan_predict_timing --kernel: %d envs x %d humans, M = %d, n = %d: %d bytes per table'
                      % (B, H, M, N, table.numel() * 8)] + lines)
    print(text)
    if out:
        with open(out, 'a') as f:
            f.write(text + '\n')
    eng.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--steps', type=int, default=4)
    ap.add_argument('--modes', type=int, default=1, choices=sorted(MODELS))
    ap.add_argument('--no-poll', action='store_true')
    ap.add_argument('--kernel', action='store_true')
    ap.add_argument('--out', default=None)
    cli = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('plan_predict_timing needs the MI355X: nothing is measured without it')
    import crowdnav_amd
    from crowdnav_amd import predict
    B, M = cli.envs, cli.modes
    if cli.kernel:
        return kernel_only(crowdnav_amd, B, M, cli.out)

    def engine():
        eng = crowdnav_amd.BatchedCrowdSim(num_envs=B, num_humans=H, robot_policy=crowdnav_amd.ROBOT_EXTERNAL, robot_visible=1)
        eng.set_gamma(0.9)
        bufs = eng.rollout_begin(seed_base=1000, seed_mod=500, record_capacity=1)
        return eng, bufs, eng.plan_reset(eng.plan_begin(K, N, E, I, INIT_STD, seed=1))

    (old, obufs, oplan), (new, _, nplan) = engine(), engine()
    pred = new.plan_predict_begin(nplan, MODELS[M])
    dt = old.config['time_step']
    counters = dict(old=0, new=0)

    def loop():
        for _ in range(cli.steps):
            state8, _ = old.get_state()
            if M == 1:
                old.plan_cem_paths(oplan, predict.to_goal(state8, N, dt), counters['old'])
            else:
                human_vel = predict.stack_modes(predict.constant_velocity(state8, N), predict.to_goal(state8, N, dt))
                old.plan_cem_modes(oplan, human_vel, counters['old'])
            old.rollout_step(oplan.action)
            old.plan_shift(oplan)
            counters['old'] += I
            if not cli.no_poll and int(obufs['active'].sum().item()) == 0:
                break
        old.sync()

    def one_call():
        new.plan_predict_rollout(nplan, pred, cli.steps, counters['new'])
        counters['new'] += cli.steps * I
        new.sync()

    kinds = (('per-step loop, torch predictor' + (', no poll' if cli.no_poll else ''), loop), ('1 plan_predict_rollout call', one_call))
    seconds = {k[0]: [] for k in kinds}
    for rep in range(-1, cli.reps):  # (-1: warm-up)
        for name, call in kinds:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            if rep >= 0:
                seconds[name].append(time.perf_counter() - t0)
    same = all(torch.equal(a, b) for a, b in zip(old.get_state(), new.get_state())) and torch.equal(oplan.mean, nplan.mean)
    lines = ['plan_predict_timing: %d envs x %d humans, M = %d (%s), K = %d, n = %d, I = %d, E = %d, %d closed-loop steps per call, %d '
             'alternating rounds in one process after one warm-up round; host clock around the calls + synchronise; the two engines '
             'end in the same state and plan: %s' % (B, H, M, ', '.join(MODELS[M]), K, N, I, E, cli.steps, cli.reps, same)]
    for name, _ in kinds:
        s = seconds[name]
        lines.append('%-44s median %9.3f ms  sd %7.3f ms  min %9.3f  max %9.3f  (%7.3f ms per closed-loop step)'
                     % (name, statistics.median(s) * 1e3, statistics.stdev(s) * 1e3 if len(s) > 1 else 0.0, min(s) * 1e3, max(s) * 1e3,
                        statistics.median(s) * 1e3 / cli.steps))
    a, b = seconds[kinds[0][0]], seconds[kinds[1][0]]
    slower = statistics.median(b) - statistics.median(a)
    pooled = math.sqrt((statistics.variance(a) + statistics.variance(b)) / 2.0) if cli.reps > 1 else float('nan')
    verdict = 'SLOWER by more than that margin' if slower > 3.0 * pooled else 'faster by more than that margin' if -slower > 3.0 * pooled \
        else 'within that margin'
    lines.append('loop / one call = %.2f (medians); one call - loop = %.3f ms against a bar of 3 pooled sd = %.3f ms: %s'
                 % (statistics.median(a) / statistics.median(b), slower * 1e3, 3.0 * pooled * 1e3, verdict))
    text = '\n'.join(lines)
    print(text)
    if cli.out:
        with open(cli.out, 'a') as f:
            f.write(text + '\n')
    old.close(), new.close()
    return 0


if __name__ == '__main__':
    sys.exit(main())
