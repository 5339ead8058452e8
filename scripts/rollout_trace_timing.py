"""What recording every step costs: rollout_trace (cn_rollout_trace, with and without rewards) against rollout (cn_rollout) on
the same engine, alternating in one process.

    python scripts/rollout_trace_timing.py [--reps 10] [--out profiles/rollout_trace_timing.txt]

Two shapes: 4096 envs x 5 humans in 1000-step calls (cn_rollout runs the fused kernel there) and 4096 x 20 in 200-step calls (the
shard kernel under its schedule); the traced calls run the generic phase kernel at both.  After two warm-up calls of each
kind, --reps rounds of (rollout, trace, trace with rewards); every call is timed by the host clock around the call and a device
synchronise, and its transitions are read from the rollout's own counter.  A traced call's time includes the fill of its
episode array with -1 (rollout_trace does that before the launch); the trace tensors are allocated once and reused.
Prints, per shape and kind, the median env-steps/s with min / max over the rounds, and for the traced kinds the bytes the trace
stores put out per second ((64 A + 8 [+ 17]) x transitions / time) beside the HBM peak.  No floor: this is the inspection path."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_TBS, HBM_COPY_TBS = 8.0, 6.29  # MI355X: spec, and a measured float4 copy

SHAPES = ((4096, 5, 1000), (4096, 20, 200))


def measure(B, H, n, reps):
    import crowdnav_amd
    eng = crowdnav_amd.BatchedCrowdSim(num_envs=B, num_humans=H, robot_policy=crowdnav_amd.ROBOT_ORCA, robot_visible=1)
    eng.set_gamma(0.9)
    bufs = eng.rollout_begin(seed_base=1000, seed_mod=500, record_capacity=8)
    full = eng.rollout_trace(n, rewards=True)
    bare = {k: full[k] for k in ('state8', 'episode', 'step')}
    kinds = {'rollout': lambda: eng.rollout(n), 'trace': lambda: eng.rollout_trace(n, out=bare),
             'trace+rewards': lambda: eng.rollout_trace(n, rewards=True, out=full)}
    for _ in range(2):
        for call in kinds.values():
            call()
    eng.sync()
    rates, seconds, steps = ({k: [] for k in kinds} for _ in range(3))
    for _ in range(reps):
        for name, call in kinds.items():
            before = int(bufs['transitions'].item())  # (a synchronise)
            t0 = time.perf_counter()
            call()
            eng.sync()
            dt = time.perf_counter() - t0
            done = int(bufs['transitions'].item()) - before
            rates[name].append(done / dt), seconds[name].append(dt), steps[name].append(done)
    lines = []
    for name in kinds:
        r = rates[name]
        line = '%5d x %2d, %4d-step calls  %-14s median %8.2f M env-steps/s  min %8.2f  max %8.2f  (%.2f ms per call)' % (
            B, H, n, name, statistics.median(r) / 1e6, min(r) / 1e6, max(r) / 1e6, statistics.median(seconds[name]) * 1e3)
        if name != 'rollout':
            row = 64 * (H + 1) + 8 + (17 if name == 'trace+rewards' else 0)
            bw = statistics.median([row * s / t for s, t in zip(steps[name], seconds[name])])
            line += '  %4d B per env-step: %6.1f GB/s written = %.2f%% of the %.1f TB/s HBM peak (%.2f%% of a measured copy)' % (
                row, bw / 1e9, bw / (HBM_PEAK_TBS * 1e12) * 100, HBM_PEAK_TBS, bw / (HBM_COPY_TBS * 1e12) * 100)
        lines.append(line)
    base = statistics.median(rates['rollout'])
    lines.append('%5d x %2d  trace / rollout = %.3f, trace+rewards / rollout = %.3f (medians)' % (
        B, H, statistics.median(rates['trace']) / base, statistics.median(rates['trace+rewards']) / base))
    eng.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=None)
    cli = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('rollout_trace_timing needs the MI355X: nothing is measured without it')
    lines = ['rollout_trace_timing: %d rounds per shape, the three kinds alternating on one engine; host clock around call + '
             'synchronise' % cli.reps]
    for B, H, n in SHAPES:
        lines += measure(B, H, n, cli.reps)
    text = '\n'.join(lines)
    print(text)
    if cli.out:
        with open(cli.out, 'a') as f:
            f.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
