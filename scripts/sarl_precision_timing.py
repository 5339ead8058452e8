"""Time of cn_sarl_select on the fp32 route of the configuration (precision='f32': what the library ran before the split route
existed, the same kernels unchanged) against the split-f16 route (precision='f16x2'), two engines on the same state in one
process, alternating.

    python scripts/sarl_precision_timing.py [--reps 20] [--out profiles/sarl_precision_timing.txt]
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/sarl_precision_timing.py --reps 3     # kernel times

5 humans x 81 actions at 4096 envs (the benchmark's size: the fp32 route is sarl_reg_kernel) and at 100 envs (the one-tile LDS
kernel), 13- and 61-wide rows; HIP-event times of the whole call (ORCA, lookahead, features, network, selection) after warm-up.
Prints medians and spreads.  Condition at 4096 envs: the split median lies below the fp32 median by more than three times the
larger of the two standard deviations; the exit status says whether it held."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def engine(B, with_om, precision, net):
    import crowdnav_amd
    from crowdnav_amd.compat.sarl import build_action_space
    eng = crowdnav_amd.BatchedCrowdSim(num_envs=B, num_humans=5, robot_policy=crowdnav_amd.ROBOT_EXTERNAL, robot_visible=1)
    eng.reset(2000 + np.arange(B))
    eng.step(np.zeros((B, 2)), update=True)
    space, _, _ = build_action_space(1.0)
    eng.sarl_configure(actions=np.array([[a.vx, a.vy] for a in space]), with_om=with_om, precision=precision)
    eng.sarl_set_weights(net.state_dict())
    return eng


def main():
    from crowdnav_amd.compat.sarl import ValueNetwork
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    cli = ap.parse_args()
    lines = ['sarl_precision_timing: cn_sarl_select, 5 humans x 81 actions, %d repetitions per route after %d warm-up calls, '
             'alternating; HIP-event ms per call' % (cli.reps, cli.warmup)]
    ok = True
    for B in (4096, 100):
        for with_om in (False, True):
            torch.manual_seed(0)
            net = ValueNetwork(61 if with_om else 13, 6, [150, 100], [100, 50], [150, 100, 100, 1], [100, 100, 1], True, 1.0, 4)
            engines = {p: engine(B, with_om, p, net) for p in ('f32', 'f16x2')}
            routes = {p: e.sarl_network_route() for p, e in engines.items()}
            assert routes['f16x2'] == 'split_f16' and routes['f32'] != 'split_f16'
            outs = {}
            for p, e in engines.items():
                for _ in range(cli.warmup):
                    outs[p] = e.sarl_select(want_values=True)
            torch.cuda.synchronize()
            diff = float((outs['f32']['values'] - outs['f16x2']['values']).abs().max())
            same = float((outs['f32']['best'] == outs['f16x2']['best']).double().mean())
            times = {p: [] for p in engines}
            for _ in range(cli.reps):
                for p, e in engines.items():
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    e.sarl_select(want_values=False)
                    t1.record()
                    t1.synchronize()
                    times[p].append(t0.elapsed_time(t1))
            med, sd = {}, {}
            for p, ts in times.items():
                med[p], sd[p] = statistics.median(ts), statistics.pstdev(ts)
                lines.append('%4d envs D = %2d  %-5s (%-9s) median %7.3f  min %7.3f  max %7.3f  stdev %6.3f'
                             % (B, 61 if with_om else 13, p, routes[p], med[p], min(ts), max(ts), sd[p]))
            gain = med['f32'] - med['f16x2']
            note = ''
            if B == 4096:
                held = gain > 3 * max(sd.values())
                ok = ok and held
                note = '  (condition: gain %.3f > 3 x %.3f: %s)' % (gain, max(sd.values()), 'met' if held else 'MISSED')
            lines.append('%4d envs D = %2d  f16x2 / f32 = %.3f; max |values difference| %.2e, same arg-max in %.4f of the envs%s'
                         % (B, 61 if with_om else 13, med['f16x2'] / med['f32'], diff, same, note))
            for e in engines.values():
                e.close()
    text = '\n'.join(lines)
    print(text)
    if cli.out:
        with open(cli.out, 'a') as f:
            f.write(text + '\n')
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
