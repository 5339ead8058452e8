"""What the goal-progress term costs: every lookahead route and one closed loop, with the engine's goal weight
at 0 — the kernels that know nothing of the term, instruction-identical to the parent's (profiles/lookahead_goal_kernels.txt) —
against the weight at 0.1, their goal forms; alternating in one process on one engine.

    python scripts/lookahead_goal_timing.py [--reps 20] [--inner 10] [--out profiles/lookahead_goal_timing.txt]

4096 envs x 5 humans, external holonomic robot, reset from the test seeds and advanced 20 steps; K = 64 candidates of n = 12
steps drawn from the 81-action space (a device tensor, made once); then the same at 8 envs.  Rows: lookahead() under 'orca' and
under 'constant_velocity', lookahead_paths() against predict.to_goal's table, lookahead_modes() at M = 4, and one plan_rollout
call of 4 real steps (K = 64, n = 12, 3 iterations; the engine is put back to the same state before every call, outside the
clock).  After one warm-up round of both weights, --reps rounds of (w = 0, w = 0.1); a sample is --inner calls (the closed loop:
one) timed by the host clock from the first call to the end of a device synchronise, reported per call.  Expected: no
difference — three float64 operations and one square root per branch.  Per row: medians, standard deviations, the difference and
whether it lies inside three pooled standard deviations, sqrt((sd_0^2 + sd_w^2) / 2)."""
import argparse
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, K, N, M, WEIGHT, REAL_STEPS = 5, 64, 12, 4, 0.1, 4


def measure(B, reps, inner):
    import crowdnav_amd
    from crowdnav_amd import predict
    from crowdnav_amd.compat.sarl import build_action_space
    space = np.array([list(a) for a in build_action_space(1.0)[0]], dtype=np.float64)
    rng = np.random.RandomState(0)
    eng = crowdnav_amd.BatchedCrowdSim(num_envs=B, num_humans=H, robot_policy=crowdnav_amd.ROBOT_EXTERNAL, robot_visible=1)
    eng.set_gamma(0.9)
    eng.reset(1000 + np.arange(B) % 500)
    warm = torch.from_numpy(space[rng.randint(len(space), size=(20, B))]).cuda()
    for t in range(20):
        eng.step(warm[t], update=True, want_obs=False)
    table = torch.from_numpy(space[rng.randint(len(space), size=(B, K, N))]).cuda()
    state, gtime = (x.clone() for x in eng.get_state())
    vel = predict.to_goal(state, N, 0.25)
    turned = torch.flip(vel, dims=(-1,))
    mvel = predict.stack_modes(predict.constant_velocity(state, N), vel, turned, -turned)
    outs = {}
    bufs = eng.rollout_begin(seed_base=1000, seed_mod=500, record_capacity=1)
    eng.set_state(state, gtime)
    plan = eng.plan_begin(K, N, 8, 3, 0.5, seed=5)

    def orca():
        eng.set_lookahead_human_model('orca')
        for _ in range(inner):
            outs['orca'] = eng.lookahead(table, out=outs.get('orca'))

    def cv():
        eng.set_lookahead_human_model('constant_velocity')
        for _ in range(inner):
            outs['cv'] = eng.lookahead(table, out=outs.get('cv'))

    def paths():
        for _ in range(inner):
            outs['paths'] = eng.lookahead_paths(table, vel, out=outs.get('paths'))

    def modes():
        for _ in range(inner):
            outs['modes'] = eng.lookahead_modes(table, mvel, out=outs.get('modes'))

    def loop():
        eng.plan_rollout(plan, REAL_STEPS, 0)

    def before_loop():  # the same start for every closed-loop sample, outside the clock
        eng.set_lookahead_human_model('orca')
        eng.set_state(state, gtime)
        eng.plan_reset(plan)
        eng.sync()

    rows = (('lookahead orca', orca, None, inner), ('lookahead constant_velocity', cv, None, inner), ('lookahead_paths', paths, None, inner),
            ('lookahead_modes M = %d' % M, modes, None, inner), ('plan_rollout %d steps' % REAL_STEPS, loop, before_loop, 1))
    seconds = {(name, w): [] for name, _, _, _ in rows for w in (0.0, WEIGHT)}
    for rep in range(-1, reps):  # (-1: warm-up)
        for name, call, prepare, calls in rows:
            for w in (0.0, WEIGHT):
                eng.set_lookahead_goal_weight(w)
                if prepare:
                    prepare()
                eng.sync()
                t0 = time.perf_counter()
                call()
                eng.sync()
                dt = (time.perf_counter() - t0) / calls
                if rep >= 0:
                    seconds[(name, w)].append(dt)
    assert int(bufs['transitions'].item()) > 0
    lines = ['%d envs x %d humans, K = %d, n = %d; %d alternating rounds after one warm-up round, %d calls per sample (plan_rollout: 1); '
             'host clock around the calls + synchronise, per call' % (B, H, K, N, reps, inner)]
    for name, _, _, _ in rows:
        a, b = seconds[(name, 0.0)], seconds[(name, WEIGHT)]
        pooled = math.sqrt((statistics.variance(a) + statistics.variance(b)) / 2.0) if reps > 1 else float('nan')
        diff = statistics.median(b) - statistics.median(a)
        verdict = 'inside' if abs(diff) <= 3.0 * pooled else 'BEYOND'
        lines.append('%-30s w = 0: median %9.4f ms sd %7.4f | w = %.1f: median %9.4f ms sd %7.4f | w - 0 = %+8.4f ms, 3 pooled sd = %7.4f ms: %s'
                     % (name, statistics.median(a) * 1e3, statistics.stdev(a) * 1e3 if reps > 1 else float('nan'), WEIGHT,
                        statistics.median(b) * 1e3, statistics.stdev(b) * 1e3 if reps > 1 else float('nan'), diff * 1e3, 3.0 * pooled * 1e3,
                        verdict))
    eng.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--inner', type=int, default=10)
    ap.add_argument('--envs', default='4096,8')
    ap.add_argument('--out', default=None)
    cli = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('lookahead_goal_timing needs the MI355X: nothing is measured without it')
    lines = ['lookahead_goal_timing: goal weight 0 (the plain kernels) against %.1f (the goal forms), one engine, one process' % WEIGHT]
    for B in (int(x) for x in cli.envs.split(',')):
        lines += measure(B, cli.reps, cli.inner)
    text = '\n'.join(lines)
    print(text)
    if cli.out:
        with open(cli.out, 'a') as f:
            f.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
