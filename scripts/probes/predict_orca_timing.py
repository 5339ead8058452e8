"""What the ORCA predictor costs and what it buys (BatchedCrowdSim.predict_orca, cn_predict_orca), three comparisons, each as
alternating rounds in one process:

    python scripts/probes/predict_orca_timing.py [--envs 4096] [--reps 20] [--out profiles/predict_orca_timing.txt]

--envs envs x 5 humans, external holonomic robot that the humans see, n = 12 predicted steps.
(a) predict_orca(12) against what a caller did before it — 12 step() calls of a twin engine whose humans do not see the robot
    (the twin is put back to the same state before every round, outside the timed window) — and against predict(12, 'to_goal').
(b) predict_orca(12) + lookahead_paths at K = 64 against lookahead() under 'orca' at the same K and n.  The two differ in
    MEANING: only in the second do the humans react to the robot's candidate path.
(c) one plan_predict_orca_rollout call of 4 closed-loop steps (K = 64, n = 12, I = 3, E = 8) against plan_predict_rollout with
    to_goal, and against the per-step loop predict + predict_orca + plan_cem_paths + rollout_step + plan_shift.
After one warm-up round, --reps rounds; in (a) and (b) a round times 10 back-to-back calls of each kind (the twin's 12 steps:
once), in (c) one; the host clock runs from the first call to the end of a device synchronise.  Prints median and standard
deviation per call and, per pair, whether the difference exceeds three pooled standard deviations, sqrt((sd_a^2 + sd_b^2) / 2)."""
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

H, K, N, I, E, INIT_STD, STEPS = 5, 64, 12, 3, 8, 0.5, 4


def rounds(kinds, reps, inner):
    """name -> seconds per call, one entry per round: `inner` calls of each kind per round, kinds alternating."""
    seconds = {name: [] for name, _, _ in kinds}
    for rep in range(-1, reps):  # (-1: warm-up)
        for name, before, call in kinds:
            if before:
                before()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(1 if before else inner):  # (a kind that is put back first makes one call per round)
                call()
            torch.cuda.synchronize()
            if rep >= 0:
                seconds[name].append((time.perf_counter() - t0) / (1 if before else inner))
    return seconds


def report(title, seconds, pairs):
    lines = [title]
    for name, s in seconds.items():
        lines.append('  %-58s median %9.3f ms  sd %7.3f ms  min %9.3f  max %9.3f'
                     % (name, statistics.median(s) * 1e3, statistics.stdev(s) * 1e3, min(s) * 1e3, max(s) * 1e3))
    for a, b in pairs:
        ma, mb = statistics.median(seconds[a]), statistics.median(seconds[b])
        pooled = math.sqrt((statistics.variance(seconds[a]) + statistics.variance(seconds[b])) / 2.0)
        verdict = 'beyond' if abs(ma - mb) > 3.0 * pooled else 'WITHIN'
        lines.append('  [%s] / [%s] = %.2f (medians); difference %.3f ms, %s the bar of 3 pooled sd = %.3f ms'
                     % (a, b, ma / mb, (ma - mb) * 1e3, verdict, 3.0 * pooled * 1e3))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    cli = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('predict_orca_timing needs the MI355X: nothing is measured without it')
    import crowdnav_amd
    B = cli.envs

    def engine(**cfg):
        eng = crowdnav_amd.BatchedCrowdSim(num_envs=B, num_humans=H, robot_policy=crowdnav_amd.ROBOT_EXTERNAL, **cfg)
        eng.reset(1000 + np.arange(B))
        eng.set_gamma(0.9)
        return eng

    lines = ['predict_orca_timing: %d envs x %d humans, n = %d; %d alternating rounds in one process after one warm-up round; host clock '
             'around the calls + synchronise' % (B, H, N, cli.reps)]
    # (a) the table: one launch, twelve steps of a twin, the to_goal launch
    eng, twin = engine(robot_visible=1), engine(robot_visible=0)
    straight_on = torch.tensor([[0.0, 1.0]] * B, dtype=torch.float64, device=eng.device)
    for e in (eng, twin):
        for _ in range(4):
            e.step(straight_on, update=True, want_obs=False)
    state, gtime = (x.clone() for x in eng.get_state())
    stand = torch.zeros((B, 2), dtype=torch.float64, device=eng.device)
    table, goal_table = eng.predict_orca(N), eng.predict(N, 'to_goal')

    def put_back():
        twin.set_state(state, gtime)
        twin.drop_sims()

    recorded = torch.empty_like(table)

    def twelve_steps():  # the table as a caller recorded it before: orca_vel of every step, widened into its row
        for t in range(N):
            recorded[:, t] = twin.step(stand, update=True, want_obs=False)['orca_vel'][:, 1:]

    put_back()
    twelve_steps()
    lines.append('the twin\'s 12 recorded steps equal predict_orca(12): %s' % torch.equal(recorded, table))
    names = ('predict_orca(12)', '12 step() calls of a robot_visible = 0 twin', "predict(12, 'to_goal')")
    seconds = rounds(((names[0], None, lambda: eng.predict_orca(N, out=table)), (names[1], put_back, twelve_steps),
                      (names[2], None, lambda: eng.predict(N, 'to_goal', out=goal_table))), cli.reps, 10)
    lines += report('(a) the table (per call, 10 back-to-back calls per round; the twin: its 12 steps and row copies, once per round)',
                    seconds, ((names[1], names[0]), (names[0], names[2])))
    # (b) the trade: table + paths lookahead against the full ORCA lookahead
    actions = torch.from_numpy(np.random.RandomState(3).uniform(-0.7, 0.7, (B, K, N, 2))).to(eng.device)
    names = ('predict_orca(12) + lookahead_paths, K = 64', "lookahead() under 'orca', K = 64")
    seconds = rounds(((names[0], None, lambda: eng.lookahead_paths(actions, eng.predict_orca(N, out=table))),
                      (names[1], None, lambda: eng.lookahead(actions))), cli.reps, 10)
    lines += report('(b) scoring K = 64 candidate paths of n = 12 (the two differ in meaning: only under \'orca\' do the humans react to '
                    'the candidate)', seconds, ((names[1], names[0]),))
    twin.close()
    # (c) the closed loop
    made = []
    for _ in range(3):
        e = engine(robot_visible=1)
        bufs = e.rollout_begin(seed_base=1000, seed_mod=500, record_capacity=1)
        made.append((e, bufs, e.plan_reset(e.plan_begin(K, N, E, I, INIT_STD, seed=1))))
    (x, _, xplan), (y, _, yplan), (z, _, zplan) = made
    xpred, ypred = x.plan_predict_begin(xplan, 'to_goal'), y.plan_predict_begin(yplan, 'to_goal')
    counters = dict(x=0, y=0, z=0)
    ztable = z.predict(N, 'to_goal')

    def orca_call():
        x.plan_predict_orca_rollout(xplan, xpred, STEPS, counters['x'])
        counters['x'] += STEPS * I

    def goal_call():
        y.plan_predict_rollout(yplan, ypred, STEPS, counters['y'])
        counters['y'] += STEPS * I

    def loop():
        for _ in range(STEPS):
            z.predict(N, 'to_goal', out=ztable)
            z.predict_orca(N, out=ztable)
            z.plan_cem_paths(zplan, ztable, counters['z'])
            z.rollout_step(zplan.action)
            z.plan_shift(zplan)
            counters['z'] += I

    names = ('1 plan_predict_orca_rollout call', "1 plan_predict_rollout call, 'to_goal'", 'per-step loop with predict_orca')
    seconds = rounds(((names[0], None, orca_call), (names[1], None, goal_call), (names[2], None, loop)), cli.reps, 1)
    same = all(torch.equal(a, b) for a, b in zip(x.get_state(), z.get_state())) and torch.equal(xplan.mean, zplan.mean)
    lines += report('(c) %d closed-loop steps per call, K = %d, n = %d, I = %d, E = %d; the one call and the loop end in the same state and '
                    'plan: %s' % (STEPS, K, N, I, E, same), seconds, ((names[0], names[1]), (names[2], names[0])))
    text = '\n'.join(lines)
    print(text)
    if cli.out:
        with open(cli.out, 'a') as f:
            f.write(text + '\n\n')
    for e in (eng, x, y, z):
        e.close()
    return 0


if __name__ == '__main__':
    sys.exit(main())
