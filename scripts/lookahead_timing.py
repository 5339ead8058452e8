"""What one lookahead launch saves: ONE lookahead call (cn_lookahead_actions) scoring K candidate sequences of n actions for
each of B envs, against what a caller had to do for the same work before it existed — a second engine of B K envs, the current
state replicated K-fold into it (set_state with global_time, set_theta) and one rollout_actions(n) — alternating in one process.

    python scripts/lookahead_timing.py [--reps 10] [--candidates 16] [--horizon 20] [--out profiles/lookahead_timing.txt]

4096 envs x 5 humans, external holonomic robot, reset from the test seeds and advanced 20 steps; K = 16, n = 20, actions drawn
from the 81-action space (a device tensor, made once).  After one warm-up round, --reps rounds of (emulation, lookahead);
each is timed by the host clock from its first call to the end of a device synchronise.  The emulation is given every
advantage the old surface allows: its engine and rollout_begin are made once, outside the clock; the replication is one
repeat_interleave per array on the device; its outputs (return, end code, steps) would still have to be dug out of the record
rings, which is not timed.  It is not the same computation to the bit where a branch ends inside the horizon — the second
engine then resets into a next scenario and keeps stepping, which is why it cannot serve a planner as it stands — so the
virtual env-steps of both are reported: transitions made by branches up to their end (lookahead: the sum of `steps`), and
transitions of the second engine's counter.
Prints median and standard deviation of both, the implied virtual env-steps/s, and whether the one-call form is no slower than
the emulation by more than three times the larger standard deviation."""
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
    ap.add_argument('--candidates', type=int, default=16)
    ap.add_argument('--horizon', type=int, default=20)
    ap.add_argument('--out', default=None)
    cli = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('lookahead_timing needs the MI355X: nothing is measured without it')
    import crowdnav_amd
    from crowdnav_amd.compat.sarl import build_action_space
    K, n = cli.candidates, cli.horizon
    space = np.array([list(a) for a in build_action_space(1.0)[0]], dtype=np.float64)
    rng = np.random.RandomState(0)
    eng = crowdnav_amd.BatchedCrowdSim(num_envs=B, num_humans=H, robot_policy=crowdnav_amd.ROBOT_EXTERNAL, robot_visible=1)
    eng.set_gamma(0.9)
    eng.reset(1000 + np.arange(B) % 500)
    warm = torch.from_numpy(space[rng.randint(len(space), size=(20, B))]).cuda()
    for t in range(20):
        eng.step(warm[t], update=True, want_obs=False)
    table = torch.from_numpy(space[rng.randint(len(space), size=(B, K, n))]).cuda()
    flat = table.reshape(B * K, n, 2)
    twin = crowdnav_amd.BatchedCrowdSim(num_envs=B * K, num_humans=H, robot_policy=crowdnav_amd.ROBOT_EXTERNAL, robot_visible=1)
    twin.set_gamma(0.9)
    tbufs = twin.rollout_begin(seed_base=1000, seed_mod=500, record_capacity=1)
    out = eng.lookahead(table)

    def emulation():
        state, gtime = eng.get_state()
        twin.set_state(state.repeat_interleave(K, dim=0), gtime.repeat_interleave(K))
        twin.set_theta(eng.get_theta().repeat_interleave(K))
        twin.rollout_actions(flat)
        twin.sync()
        return None

    def one_call():
        eng.lookahead(table, out=out)
        eng.sync()
        return int(out['steps'].sum().item())

    kinds = (('second engine: set_state + set_theta + rollout_actions', emulation), ('1 lookahead call', one_call))
    seconds, done = {k[0]: [] for k in kinds}, {k[0]: [] for k in kinds}
    for rep in range(-1, cli.reps):  # (-1: warm-up)
        for name, call in kinds:
            before = int(tbufs['transitions'].item())  # (a synchronise)
            t0 = time.perf_counter()
            made = call()
            dt = time.perf_counter() - t0
            if made is None:
                made = int(tbufs['transitions'].item()) - before
            if rep >= 0:
                seconds[name].append(dt), done[name].append(made)
    lines = ['lookahead_timing: %d envs x %d humans, K = %d candidates, n = %d steps (%d virtual envs), %d alternating rounds in one '
             'process after one warm-up round; host clock around the calls + synchronise' % (B, H, K, n, B * K, cli.reps)]
    for name, _ in kinds:
        s = seconds[name]
        med, sd = statistics.median(s), statistics.stdev(s) if len(s) > 1 else 0.0
        rate = statistics.median([m / t for m, t in zip(done[name], s)])
        lines.append('%-56s median %9.3f ms  sd %7.3f ms  min %9.3f  max %9.3f  %9d virtual env-steps  %8.2f M virtual env-steps/s'
                     % (name, med * 1e3, sd * 1e3, min(s) * 1e3, max(s) * 1e3, statistics.median(done[name]), rate / 1e6))
    emu, one = seconds[kinds[0][0]], seconds[kinds[1][0]]
    slower = statistics.median(one) - statistics.median(emu)
    bar = 3.0 * max(statistics.stdev(emu), statistics.stdev(one)) if cli.reps > 1 else float('nan')
    lines.append('emulation / lookahead = %.2f (medians); lookahead - emulation = %.3f ms against a bar of 3 x the larger sd = %.3f ms: %s'
                 % (statistics.median(emu) / statistics.median(one), slower * 1e3, bar * 1e3,
                    'not slower' if slower <= bar else 'SLOWER by more than that margin'))
    text = '\n'.join(lines)
    print(text)
    if cli.out:
        with open(cli.out, 'a') as f:
            f.write(text + '\n')
    eng.close(), twin.close()
    return 0


if __name__ == '__main__':
    sys.exit(main())
