"""Per-batch time of Trainer.optimize_batch(100): today's path (CROWDNAV_AMD_SGD_KERNEL=0, the graph-replayed torch step)
against the device SGD step (=1), alternating in one process.

    python scripts/sgd_step_timing.py [--model sarl|lstm_rl] [--reps 20] [--batches 100] [--rows 100000]
                                      [--out profiles/sgd_step_timing.txt]
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/sgd_step_timing.py --only kernel --reps 3   # kernel times

Batch 100, H = 5, D = 13 and D = 61, a DeviceReplayMemory of --rows rows (the fixtures' rows tiled), after warm-up; every
repetition ends in a synchronise (optimize_batch's own .item()).  Prints medians and spreads.  --model sarl (the default): the
floor the opt-in path has to meet is kernel median <= torch median / 2 in both widths.  --model lstm_rl (lstm_rl.ValueNetwork1):
no floor was set before anything was measured; the ratio is reported and the exit status is 0."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


FIXTURES = {'sarl': ('rl_sarl_plain.npz', 'rl_sarl_om.npz'), 'lstm_rl': ('rl_lstm_rl.npz', 'rl_lstm_rl_om.npz')}


def network(model, input_dim):
    if model == 'lstm_rl':
        from crowdnav_amd.compat.lstm_rl import ValueNetwork1
        return ValueNetwork1(input_dim, 6, [150, 100, 100, 1], 50)
    from crowdnav_amd.compat.sarl import ValueNetwork
    return ValueNetwork(input_dim, 6, [150, 100], [100, 50], [150, 100, 100, 1], [100, 100, 1], True, 1.0, 4)


def trainer(switch, model, fixture, rows):
    from crowdnav_amd.compat.trainer import DeviceReplayMemory, Trainer
    g = np.load(os.path.join(ROOT, 'tests', 'golden', fixture))
    S, V = g['memory_states'], g['memory_values']
    reps = -(-rows // len(S))
    memory = DeviceReplayMemory(rows, 'cuda:0')
    memory.push_batch(torch.from_numpy(np.tile(S, (reps, 1, 1))[:rows]), torch.from_numpy(np.tile(V, reps)[:rows]))
    model = network(model, S.shape[2])
    model.load_state_dict({k[6:]: torch.from_numpy(g[k]) for k in g.files if k.startswith('param_')})
    os.environ['CROWDNAV_AMD_SGD_KERNEL'] = switch  # read when the Trainer is constructed
    t = Trainer(model.to('cuda:0'), memory, torch.device('cuda:0'), 100)
    t.set_learning_rate(0.001)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--model', choices=sorted(FIXTURES), default='sarl')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--batches', type=int, default=100)
    ap.add_argument('--rows', type=int, default=100000)
    ap.add_argument('--only', choices=['both', 'kernel', 'torch'], default='both')
    ap.add_argument('--out', default=None)
    cli = ap.parse_args()
    lines = ['sgd_step_timing%s: optimize_batch(%d) at batch 100, H = 5, memory of %d rows, %d repetitions per path, alternating; '
             'us per batch' % ('' if cli.model == 'sarl' else ' --model ' + cli.model, cli.batches, cli.rows, cli.reps)]
    ok = True
    for fixture in FIXTURES[cli.model]:
        paths = {}
        if cli.only in ('both', 'torch'):
            paths['torch'] = trainer('0', cli.model, fixture, cli.rows)
        if cli.only in ('both', 'kernel'):
            paths['kernel'] = trainer('1', cli.model, fixture, cli.rows)
        times = {k: [] for k in paths}
        for t in paths.values():  # warm-up: graph capture / scratch allocation
            t.optimize_batch(cli.batches)
        for _ in range(cli.reps):
            for name, t in paths.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                t.optimize_batch(cli.batches)  # ends in .item(): a synchronise
                times[name].append((time.perf_counter() - t0) / cli.batches * 1e6)
        if 'kernel' in paths:
            assert paths['kernel']._kstep is not None and paths['kernel']._kstep.steps == (cli.reps + 1) * cli.batches
        D = paths[next(iter(paths))].memory.states.shape[2]
        med = {}
        for name, ts in times.items():
            med[name] = statistics.median(ts)
            lines.append('D = %2d  %-6s median %8.1f  min %8.1f  max %8.1f  stdev %7.1f' % (D, name, med[name], min(ts), max(ts),
                                                                                         statistics.pstdev(ts)))
        if len(med) == 2:
            ratio = med['kernel'] / med['torch']
            if cli.model == 'sarl':
                ok = ok and ratio <= 0.5
                lines.append('D = %2d  kernel / torch = %.3f  (floor: <= 0.5: %s)' % (D, ratio, 'met' if ratio <= 0.5 else 'MISSED'))
            else:
                lines.append('D = %2d  kernel / torch = %.3f  (no floor set)' % (D, ratio))
    text = '\n'.join(lines)
    print(text)
    if cli.out:
        with open(cli.out, 'a') as f:
            f.write(text + '\n')
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
