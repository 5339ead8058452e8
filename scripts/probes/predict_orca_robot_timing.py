"""What the ORCA predictor costs when its humans see the robot on a nominal sequence (BatchedCrowdSim.predict_orca_robot,
cn_predict_orca_robot), four comparisons, each as alternating rounds in one process:

    python scripts/probes/predict_orca_robot_timing.py [--envs 4096] [--reps 20] [--out profiles/predict_orca_robot_timing.txt]

--envs envs x 5 humans, external holonomic robot that the humans see, n = 12 predicted steps.
(a) predict_orca_robot(12, seq) against predict_orca(12) — the robot-unseen kernel, unchanged — in the same engine.
(b) predict_orca_robot(12, seq) against what a caller did before it: 12 step(seq[:, t]) calls of a robot_visible = 1 twin that
    records the same table (the twin is put back to the same state before every round, outside the timed window).
(c) predict_orca_robot(12, seq) + lookahead_paths at K = 64 against lookahead() under 'orca' at the same K and n.  The two differ
    in MEANING for every candidate but the nominal one: only under 'orca' do the humans react to each candidate.
(d) one plan_predict_orca_nominal_rollout call of 4 closed-loop steps (K = 64, n = 12, I = 3, E = 8) against
    plan_predict_orca_rollout, and against its own per-step loop plan_draw + predict + predict_orca_robot + plan_cem_paths +
    rollout_step + plan_shift.
After one warm-up round, --reps rounds; in (a) - (c) a round times 10 back-to-back calls of each kind (the twin's 12 steps:
once), in (d) one; the host clock runs from the first call to the end of a device synchronise.  Prints median and standard
deviation per call and, per pair, whether the difference exceeds three pooled standard deviations, sqrt((sd_a^2 + sd_b^2) / 2)."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from predict_orca_timing import E, H, I, INIT_STD, K, N, STEPS, report, rounds  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    cli = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('predict_orca_robot_timing needs the MI355X: nothing is measured without it')
    import crowdnav_amd
    B = cli.envs

    def engine(**cfg):
        eng = crowdnav_amd.BatchedCrowdSim(num_envs=B, num_humans=H, robot_policy=crowdnav_amd.ROBOT_EXTERNAL, **cfg)
        eng.reset(1000 + np.arange(B))
        eng.set_gamma(0.9)
        return eng

    lines = ['predict_orca_robot_timing: %d envs x %d humans, n = %d; %d alternating rounds in one process after one warm-up round; '
             'host clock around the calls + synchronise' % (B, H, N, cli.reps)]
    eng, twin = engine(robot_visible=1), engine(robot_visible=1)
    straight_on = torch.tensor([[0.0, 1.0]] * B, dtype=torch.float64, device=eng.device)
    for e in (eng, twin):
        for _ in range(4):
            e.step(straight_on, update=True, want_obs=False)
    state, gtime = (x.clone() for x in eng.get_state())
    seq = torch.from_numpy(np.random.RandomState(5).uniform(-0.7, 0.7, (B, N, 2))).to(eng.device)
    unseen, table = eng.predict_orca(N), eng.predict_orca_robot(N, seq)

    def put_back():
        twin.set_state(state, gtime)
        twin.drop_sims()

    recorded = torch.empty_like(table)

    def twelve_steps():  # the table as a caller recorded it before: orca_vel of every step, widened into its row
        for t in range(N):
            recorded[:, t] = twin.step(seq[:, t].contiguous(), update=True, want_obs=False)['orca_vel'][:, 1:]

    put_back()
    twelve_steps()
    lines.append('the twin\'s 12 recorded steps equal predict_orca_robot(12, seq): %s' % torch.equal(recorded, table))
    # (a), (b) the table
    names = ('predict_orca_robot(12, seq)', 'predict_orca(12)', '12 step(seq[:, t]) calls of a robot_visible = 1 twin')
    seconds = rounds(((names[0], None, lambda: eng.predict_orca_robot(N, seq, out=table)),
                      (names[1], None, lambda: eng.predict_orca(N, out=unseen)), (names[2], put_back, twelve_steps)), cli.reps, 10)
    lines += report('(a), (b) the table (per call, 10 back-to-back calls per round; the twin: its 12 steps and row copies, once per '
                    'round)', seconds, ((names[0], names[1]), (names[2], names[0])))
    twin.close()
    # (c) the trade: table + paths lookahead against the full ORCA lookahead
    actions = torch.from_numpy(np.random.RandomState(3).uniform(-0.7, 0.7, (B, K, N, 2))).to(eng.device)
    names = ('predict_orca_robot(12, seq) + lookahead_paths, K = 64', "lookahead() under 'orca', K = 64")
    seconds = rounds(((names[0], None, lambda: eng.lookahead_paths(actions, eng.predict_orca_robot(N, actions[:, 0], out=table))),
                      (names[1], None, lambda: eng.lookahead(actions))), cli.reps, 10)
    lines += report('(c) scoring K = 64 candidate paths of n = 12 (the two differ in meaning for every candidate but the nominal one: '
                    'only under \'orca\' do the humans react to each candidate)', seconds, ((names[1], names[0]),))
    # (d) the closed loop
    made = []
    for _ in range(3):
        e = engine(robot_visible=1)
        bufs = e.rollout_begin(seed_base=1000, seed_mod=500, record_capacity=1)
        made.append((e, bufs, e.plan_reset(e.plan_begin(K, N, E, I, INIT_STD, seed=1))))
    (x, _, xplan), (y, _, yplan), (z, _, zplan) = made
    xpred, ypred = x.plan_predict_begin(xplan, 'to_goal'), y.plan_predict_begin(yplan, 'to_goal')
    counters = dict(x=0, y=0, z=0)
    ztable = z.predict(N, 'to_goal')

    def nominal_call():
        x.plan_predict_orca_nominal_rollout(xplan, xpred, STEPS, counters['x'])
        counters['x'] += STEPS * I

    def unseen_call():
        y.plan_predict_orca_rollout(yplan, ypred, STEPS, counters['y'])
        counters['y'] += STEPS * I

    def loop():
        for _ in range(STEPS):
            z.plan_draw(zplan, counters['z'])
            z.predict(N, 'to_goal', out=ztable)
            z.predict_orca_robot(N, zplan.candidates[:, 0], out=ztable)
            z.plan_cem_paths(zplan, ztable, counters['z'])
            z.rollout_step(zplan.action)
            z.plan_shift(zplan)
            counters['z'] += I

    names = ('1 plan_predict_orca_nominal_rollout call', '1 plan_predict_orca_rollout call', 'per-step loop with predict_orca_robot')
    seconds = rounds(((names[0], None, nominal_call), (names[1], None, unseen_call), (names[2], None, loop)), cli.reps, 1)
    same = all(torch.equal(a, b) for a, b in zip(x.get_state(), z.get_state())) and torch.equal(xplan.mean, zplan.mean)
    lines += report('(d) %d closed-loop steps per call, K = %d, n = %d, I = %d, E = %d; the one call and the loop end in the same state '
                    'and plan: %s' % (STEPS, K, N, I, E, same), seconds, ((names[0], names[1]), (names[2], names[0])))
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
