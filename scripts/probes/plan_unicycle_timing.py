"""What planning over (v, r) costs (cn_plan_set_unicycle): the unicycle forms of the plan kernels against the holonomic ones, and
one plan_rollout call on a unicycle engine against the same loop made of the public per-step calls.

    python scripts/probes/plan_unicycle_timing.py [--envs 4096] [--reps 20] [--steps 4] [--inner 50] [--out profiles/plan_unicycle_timing.txt]

--envs envs x 5 humans, external robot, K = 64 candidates, n = 12 steps, I = 3 iterations, E = 8 elites, init_std 0.5; the unicycle
engine with max_rotation pi / 4 and init_std_rotation 0.5.
(a) plan_draw, plan_reset and plan_mppi_update on a unicycle engine and on a holonomic twin of the same shape: --inner calls
    enqueued back to back and one synchronise per timed window (a single launch is microseconds), the two engines alternating.
(b) ONE plan_rollout call of --steps closed-loop steps against --steps x (plan_cem, rollout_step, plan_shift), alternating on
    the same unicycle engine.
After one warm-up round, --reps rounds; the host clock from the first call to the end of a device synchronise.  Prints median
and standard deviation of each, the ratios of (a), and for (b) whether the one call's median is within three pooled standard
deviations of the loop's."""
import argparse
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

H, K, N, I, E, INIT_STD, TEMPERATURE, MAX_ROTATION, STD_ROTATION = 5, 64, 12, 3, 8, 0.5, 1.0, math.pi / 4, 0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--steps', type=int, default=4)
    ap.add_argument('--inner', type=int, default=50)
    ap.add_argument('--out', default=None)
    cli = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('plan_unicycle_timing needs the MI355X: nothing is measured without it')
    import crowdnav_amd
    B = cli.envs

    def planner(unicycle):
        eng = crowdnav_amd.BatchedCrowdSim(num_envs=B, num_humans=H, robot_policy=crowdnav_amd.ROBOT_EXTERNAL, robot_visible=1,
                                           robot_kinematics=1 if unicycle else 0)
        if unicycle:
            eng.set_plan_unicycle(MAX_ROTATION, STD_ROTATION)
        eng.set_gamma(0.9)
        eng.rollout_begin(seed_base=1000, seed_mod=500, record_capacity=1)
        plan = eng.plan_reset(eng.plan_begin(K, N, E, I, INIT_STD, seed=1))
        eng.plan_cem(plan, 0)  # scores for the MPPI update to weigh
        return eng, plan

    (uni, uni_plan), (holo, holo_plan) = planner(True), planner(False)
    loop, loop_plan = uni, uni.plan_reset(uni.plan_begin(K, N, E, I, INIT_STD, seed=1))
    counter = [1]

    def many(eng, call):
        def run():
            for _ in range(cli.inner):
                call()
            eng.sync()
        return run

    def one_call():
        uni.plan_rollout(uni_plan, cli.steps, counter[0])
        uni.sync()

    def per_step():
        for s in range(cli.steps):
            loop.plan_cem(loop_plan, counter[0] + s * I)
            loop.rollout_step(loop_plan.action)
            loop.plan_shift(loop_plan)
        loop.sync()

    kernels = []
    for name, of in (('plan_draw', lambda e, p: (lambda: e.plan_draw(p, counter[0]))),
                     ('plan_reset', lambda e, p: (lambda: e.plan_reset(p))),
                     ('plan_mppi_update', lambda e, p: (lambda: e.plan_mppi_update(p, TEMPERATURE)))):
        kernels.append((name + ' (v, r)', many(uni, of(uni, uni_plan)), cli.inner))
        kernels.append((name + ' (vx, vy)', many(holo, of(holo, holo_plan)), cli.inner))
    loops = [('1 plan_rollout call', one_call, 1), ('%d x (plan_cem, rollout_step, plan_shift)' % cli.steps, per_step, 1)]
    seconds = {k[0]: [] for k in kernels + loops}
    for rep in range(-1, cli.reps):  # (-1: warm-up)
        for name, call, per in kernels + loops:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            if rep >= 0:
                seconds[name].append((time.perf_counter() - t0) / per)
        counter[0] += cli.steps * I
    sd = lambda s: statistics.stdev(s) if len(s) > 1 else 0.0  # noqa: E731
    med = statistics.median
    lines = ['plan_unicycle_timing: %d envs x %d humans, K = %d, n = %d, I = %d, E = %d, max_rotation pi / 4; %d alternating rounds in one '
             'process after one warm-up round; host clock around the calls + synchronise'
             % (B, H, K, N, I, E, cli.reps),
             '(a) per call, %d calls back to back per timed window:' % cli.inner]
    for name, _, _ in kernels:
        s = seconds[name]
        lines.append('  %-28s median %9.2f us  sd %8.2f us  min %9.2f  max %9.2f' % (name, med(s) * 1e6, sd(s) * 1e6, min(s) * 1e6, max(s) * 1e6))
    for i in range(0, len(kernels), 2):
        a, b = seconds[kernels[i][0]], seconds[kernels[i + 1][0]]
        lines.append('  %s / %s = %.3f (medians)' % (kernels[i][0], kernels[i + 1][0], med(a) / med(b)))
    lines.append('(b) %d closed-loop steps on the unicycle engine:' % cli.steps)
    for name, _, _ in loops:
        s = seconds[name]
        lines.append('  %-44s median %9.3f ms  sd %7.3f ms  min %9.3f  max %9.3f  (%7.3f ms per closed-loop step)'
                     % (name, med(s) * 1e3, sd(s) * 1e3, min(s) * 1e3, max(s) * 1e3, med(s) * 1e3 / cli.steps))
    a, b = seconds[loops[0][0]], seconds[loops[1][0]]
    pooled = math.sqrt((sd(a) ** 2 + sd(b) ** 2) / 2.0)
    slower = med(a) - med(b)
    lines.append('  one call - loop = %.3f ms (medians) against a bar of 3 pooled sd = %.3f ms: %s'
                 % (slower * 1e3, 3e3 * pooled, 'not slower' if slower <= 3.0 * pooled else 'SLOWER by more than that margin'))
    text = '\n'.join(lines)
    print(text)
    if cli.out:
        with open(cli.out, 'a') as f:
            f.write(text + '\n')
    uni.close()
    holo.close()
    return 0


if __name__ == '__main__':
    sys.exit(main())
