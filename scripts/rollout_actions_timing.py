"""What a table of actions saves: ONE rollout_actions call (cn_rollout_actions) against the T rollout_step calls
(cn_rollout_step) it replaces, on the same engine, alternating in one process.

    python scripts/rollout_actions_timing.py [--reps 10] [--steps 1000] [--out profiles/rollout_actions_timing.txt]

4096 envs x 5 humans, external holonomic robot, T = 1000 actions per env drawn from the 81-action space (a device tensor, made
once).  After one warm-up round, --reps rounds of (step loop, table call, table call with trace=True and rewards); every kind
is timed by the host clock from its first call to the end of a device synchronise, and its transitions are read from the
rollout's own counter.  The step loop hands each call a contiguous [B, 2] block of a [T, B, 2] copy of the table, so that no
copy or synchronise sits between its launches; the traced call's time includes the fill of its episode array with -1, its
tensors are allocated once and reused.  For context only, rollout(T) on an ORCA-robot engine of the same shape (the fused
kernel; another robot, hence other episodes) is timed the same way.
Prints, per kind, median and standard deviation of the time per call sequence and per batched step, the median env-steps/s,
and whether the table call beats the step loop by more than three times the larger standard deviation."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, H = 4096, 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--steps', type=int, default=1000)
    ap.add_argument('--out', default=None)
    cli = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('rollout_actions_timing needs the MI355X: nothing is measured without it')
    import crowdnav_amd
    from crowdnav_amd.compat.sarl import build_action_space
    T = cli.steps
    space = np.array([list(a) for a in build_action_space(1.0)[0]], dtype=np.float64)
    table = torch.from_numpy(space[np.random.RandomState(0).randint(len(space), size=(B, T))]).cuda()
    by_step = table.transpose(0, 1).contiguous()  # [T, B, 2]: the step loop's blocks
    ext = crowdnav_amd.BatchedCrowdSim(num_envs=B, num_humans=H, robot_policy=crowdnav_amd.ROBOT_EXTERNAL, robot_visible=1)
    ext.set_gamma(0.9)
    ebufs = ext.rollout_begin(seed_base=1000, seed_mod=500, record_capacity=8)
    orca = crowdnav_amd.BatchedCrowdSim(num_envs=B, num_humans=H, robot_policy=crowdnav_amd.ROBOT_ORCA, robot_visible=1)
    orca.set_gamma(0.9)
    obufs = orca.rollout_begin(seed_base=1000, seed_mod=500, record_capacity=8)
    rows = ext.rollout_actions(table, trace=True, rewards=True)

    def step_loop():
        for t in range(T):
            ext.rollout_step(by_step[t])

    kinds = (('%d rollout_step calls' % T, ext, ebufs, step_loop),
             ('1 rollout_actions call', ext, ebufs, lambda: ext.rollout_actions(table)),
             ('1 rollout_actions call, trace+rewards', ext, ebufs,
              lambda: ext.rollout_actions(table, trace=True, rewards=True, out=rows)),
             ('rollout(%d), ORCA robot (context)' % T, orca, obufs, lambda: orca.rollout(T)))
    seconds, done = {k[0]: [] for k in kinds}, {k[0]: [] for k in kinds}
    for rep in range(-1, cli.reps):  # (-1: warm-up)
        for name, eng, bufs, call in kinds:
            before = int(bufs['transitions'].item())  # (a synchronise)
            t0 = time.perf_counter()
            call()
            eng.sync()
            dt = time.perf_counter() - t0
            if rep >= 0:
                seconds[name].append(dt), done[name].append(int(bufs['transitions'].item()) - before)
    lines = ['rollout_actions_timing: %d envs x %d humans, T = %d, %d alternating rounds in one process after one warm-up round; '
             'host clock around the calls + synchronise' % (B, H, T, cli.reps)]
    for name, _, _, _ in kinds:
        s = seconds[name]
        med, sd = statistics.median(s), statistics.stdev(s) if len(s) > 1 else 0.0
        rate = statistics.median([n / t for n, t in zip(done[name], s)])
        lines.append('%-40s median %9.3f ms  sd %7.3f ms  min %9.3f  max %9.3f  = %7.2f us per batched step  %8.2f M env-steps/s'
                     % (name, med * 1e3, sd * 1e3, min(s) * 1e3, max(s) * 1e3, med / T * 1e6, rate / 1e6))
    loop, one = seconds[kinds[0][0]], seconds[kinds[1][0]]
    traced = seconds[kinds[2][0]]
    gain = statistics.median(loop) - statistics.median(one)
    bar = 3.0 * max(statistics.stdev(loop), statistics.stdev(one)) if cli.reps > 1 else float('nan')
    lines.append('step loop / table call = %.2f (medians); step loop / traced table call = %.2f; gain %.3f ms against a bar of '
                 '3 x the larger sd = %.3f ms: %s' % (statistics.median(loop) / statistics.median(one),
                                                     statistics.median(loop) / statistics.median(traced), gain * 1e3, bar * 1e3,
                                                     'faster' if gain > bar else 'NOT faster by that margin'))
    text = '\n'.join(lines)
    print(text)
    if cli.out:
        with open(cli.out, 'a') as f:
            f.write(text + '\n')
    ext.close(), orca.close()
    return 0


if __name__ == '__main__':
    sys.exit(main())
