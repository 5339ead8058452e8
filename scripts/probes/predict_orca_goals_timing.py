"""What M ORCA futures on hypothesised goals cost (BatchedCrowdSim.predict_orca_goals / goal_hypotheses: cn_predict_orca_goals,
cn_goal_hypotheses), each comparison as alternating rounds in one process (`rounds` / `report` of predict_orca_timing.py):

    python scripts/probes/predict_orca_goals_timing.py [--envs 4096] [--reps 20] [--out profiles/predict_orca_goals_timing.txt]

--envs envs x 5 humans, external holonomic robot, n = 12 predicted steps.
(a) predict_orca_goals(12, goals) at M = 4 and M = 8 against the M calls predict_orca(12, out, mode=m) that solve as much
    (the same goals M times over, but as many ORCA programs).
(b) goal_hypotheses at M = 8 against predict(12, 8 names): a streaming kernel of the same lanes, for scale.
(c) one planning step at K = 64, I = 3 on M = 4 sampled futures — goal_hypotheses + predict_orca_goals + plan_cem_modes +
    rollout_step + plan_shift — against one real step of plan_predict_orca_rollout with the futures to_goal,orca.
After one warm-up round, --reps rounds; a round times 10 back-to-back calls of each kind in (a) and (b), one in (c); the host
clock runs from the first call to the end of a device synchronise.  Median and standard deviation per call and, per pair,
whether the difference exceeds three pooled standard deviations."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from predict_orca_timing import ROOT, rounds, report  # noqa: E402,F401  (ROOT: on sys.path by that import)

H, K, N, I, E, INIT_STD = 5, 64, 12, 3, 8, 0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    cli = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('predict_orca_goals_timing needs the MI355X: nothing is measured without it')
    import crowdnav_amd
    B = cli.envs

    def engine():
        eng = crowdnav_amd.BatchedCrowdSim(num_envs=B, num_humans=H, robot_policy=crowdnav_amd.ROBOT_EXTERNAL, robot_visible=1)
        eng.reset(1000 + np.arange(B))
        eng.set_gamma(0.9)
        return eng

    lines = ['predict_orca_goals_timing: %d envs x %d humans, n = %d; %d alternating rounds in one process after one warm-up round; '
             'host clock around the calls + synchronise' % (B, H, N, cli.reps)]
    eng = engine()
    straight_on = torch.tensor([[0.0, 1.0]] * B, dtype=torch.float64, device=eng.device)
    for _ in range(4):
        eng.step(straight_on, update=True, want_obs=False)
    sample = dict(std_heading=0.3, std_distance=0.2, seed=1)
    # (a) M futures in one launch against M launches of one future
    for M in (4, 8):
        goals = eng.goal_hypotheses(M, 'heading', **sample)
        fused, slots = eng.predict_orca_goals(N, goals), torch.empty((B, M, N, H, 2), dtype=torch.float64, device=eng.device)
        own = eng.predict_orca_goals(N, eng.get_state()[0][:, None, 1:, 4:6].expand(B, M, H, 2).contiguous())

        def m_calls(M=M, slots=slots):
            for m in range(M):
                eng.predict_orca(N, out=slots, mode=m)

        m_calls()
        lines.append('M = %d: on the engine\'s own goals every mode of predict_orca_goals equals predict_orca: %s'
                     % (M, torch.equal(own, slots)))
        names = ('predict_orca_goals(12, goals), M = %d' % M, '%d predict_orca(12, out, mode=m) calls' % M)
        seconds = rounds(((names[0], None, lambda: eng.predict_orca_goals(N, goals, out=fused)), (names[1], None, m_calls)), cli.reps, 10)
        lines += report('(a) M = %d futures (per call, 10 back-to-back calls per round)' % M, seconds, ((names[0], names[1]),))
    # (b) the sampler beside a streaming kernel of its size
    goals8 = eng.goal_hypotheses(8, 'heading', **sample)
    models = ('cv', 'to_goal') * 4
    table8 = eng.predict(N, models)
    names = ('goal_hypotheses, M = 8', 'predict(12, 8 names)')
    seconds = rounds(((names[0], None, lambda: eng.goal_hypotheses(8, 'heading', out=goals8, **sample)),
                      (names[1], None, lambda: eng.predict(N, models, out=table8))), cli.reps, 10)
    lines += report('(b) the sampler: %d 16-byte rows against the table\'s %d' % (goals8.numel() // 2, table8.numel() // 2), seconds,
                    ((names[0], names[1]),))
    # (c) one planning step
    made = []
    for _ in range(2):
        e = engine()
        e.rollout_begin(seed_base=1000, seed_mod=500, record_capacity=1)
        made.append((e, e.plan_reset(e.plan_begin(K, N, E, I, INIT_STD, seed=1))))
    (x, xplan), (y, yplan) = made
    ypred = y.plan_predict_begin(yplan, ('to_goal', 'to_goal'), reduce='min')
    xgoals = x.goal_hypotheses(4, 'heading', **sample)
    xtable = x.predict_orca_goals(N, xgoals)
    counters = dict(x=0, y=0)

    def sampled_step():
        step = counters['x']
        x.goal_hypotheses(4, 'heading', counter=step, out=xgoals, **sample)
        x.predict_orca_goals(N, xgoals, out=xtable)
        x.plan_cem_modes(xplan, xtable, step * I, reduce='min')
        x.rollout_step(xplan.action)
        x.plan_shift(xplan)
        counters['x'] += 1

    def orca_step():
        y.plan_predict_orca_rollout(yplan, ypred, 1, counters['y'] * I, orca_mode=1)
        counters['y'] += 1

    names = ('goal_hypotheses + predict_orca_goals + plan_cem_modes + step + shift, M = 4', '1 step of plan_predict_orca_rollout, to_goal,orca')
    seconds = rounds(((names[0], None, sampled_step), (names[1], None, orca_step)), cli.reps, 1)
    lines += report('(c) one planning step, K = %d, n = %d, I = %d, E = %d, reduce min' % (K, N, I, E), seconds, ((names[0], names[1]),))
    text = '\n'.join(lines)
    print(text)
    if cli.out:
        with open(cli.out, 'a') as f:
            f.write(text + '\n\n')
    for e in (eng, x, y):
        e.close()
    return 0


if __name__ == '__main__':
    sys.exit(main())
