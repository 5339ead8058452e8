"""What a lookahead costs under each human model: ONE lookahead() call under 'constant_velocity' against ONE under 'orca' on the
same engine, alternating in one process, beside a device-to-device copy of the bytes the call has to move.

    python scripts/probes/lookahead_cv_timing.py [--envs 4096 8] [--reps 20] [--out profiles/lookahead_cv_timing.txt]

Per --envs value: envs x 5 humans, external holonomic robot, K = 64 candidates of n = 12 steps drawn from the 81-action table,
from the state 6 real steps after a seeded reset; without and with final_state8.  After one warm-up round, --reps rounds of
(orca, constant_velocity, copy); each is timed by the host clock from its call to the end of a device synchronise, under a
limit of its own (--limit seconds: a region that takes longer ends the run).  The copy is the yardstick of the new kernel: the
action table [B][K][n][2] + the [B][K] outputs (ret, info, steps, time; final_theta with the final state) + final_state8
[B][K][A][8] where asked, each copied once by torch on the engine's stream.  Then one plan_rollout call (4 closed-loop steps,
I = 3, E = 8) under each model at the largest --envs, with no bar.  Prints medians and standard deviations and the two bars:
at the largest shape constant_velocity faster than orca by more than 3 standard deviations of either, at the smallest not
slower by that margin."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

H, K, N, I, E, INIT_STD, PLAN_STEPS = 5, 64, 12, 3, 8, 0.5, 4


def timed(call, sync, limit):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    call()
    sync()
    dt = time.perf_counter() - t0
    if dt > limit:
        sys.exit('a timed region took %.1f s, over its limit of %.1f s' % (dt, limit))
    return dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, nargs='+', default=[4096, 8])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--limit', type=float, default=20.0)
    ap.add_argument('--out', default=None)
    cli = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('lookahead_cv_timing needs the MI355X: nothing is measured without it')
    import crowdnav_amd
    from crowdnav_amd.compat.sarl import build_action_space
    acts = np.array([list(a) for a in build_action_space(1.0)[0]], dtype=np.float64)
    sd = lambda s: statistics.stdev(s) if len(s) > 1 else 0.0  # noqa: E731
    med = statistics.median
    lines = ['lookahead_cv_timing: envs x %d humans, K = %d, n = %d, %d alternating rounds (orca, constant_velocity, copy) in one '
             'process after one warm-up round; host clock around each call + synchronise' % (H, K, N, cli.reps)]
    verdicts = []
    for B in cli.envs:
        eng = crowdnav_amd.BatchedCrowdSim(num_envs=B, num_humans=H, robot_policy=crowdnav_amd.ROBOT_EXTERNAL, robot_visible=1)
        eng.set_gamma(0.9)
        eng.reset(1000 + np.arange(B))
        for _ in range(6):
            eng.step(np.tile([0.0, 1.0], (B, 1)), update=True, want_obs=False)
        table = torch.from_numpy(acts[np.random.RandomState(3).randint(len(acts), size=(B, K, N))]).to(eng.device).contiguous()
        for final_state in (False, True):
            out = {m: eng.lookahead(table[:, :, :0].contiguous(), final_state=final_state) for m in ('orca', 'constant_velocity')}
            src = [table] + [out['orca'][k] for k in sorted(out['orca'])]
            dst = [torch.empty_like(t) for t in src]
            nbytes = sum(t.numel() * t.element_size() for t in src)

            def run(model):
                eng.set_lookahead_human_model(model)
                eng.lookahead(table, final_state=final_state, out=out[model])

            def copy():
                for d, s in zip(dst, src):
                    d.copy_(s)

            kinds = (('orca', lambda: run('orca')), ('constant_velocity', lambda: run('constant_velocity')), ('copy', copy))
            seconds = {k: [] for k, _ in kinds}
            for rep in range(-1, cli.reps):  # (-1: warm-up)
                for name, call in kinds:
                    dt = timed(call, eng.sync, cli.limit)
                    if rep >= 0:
                        seconds[name].append(dt)
            shape = '%d envs, final_state8 %s, %.1f MB moved' % (B, 'on ' if final_state else 'off', nbytes / 1e6)
            for name, _ in kinds:
                s = seconds[name]
                lines.append('%-46s %-18s median %9.4f ms  sd %7.4f ms  min %9.4f  max %9.4f'
                             % (shape, name, med(s) * 1e3, sd(s) * 1e3, min(s) * 1e3, max(s) * 1e3))
            o, c, y = seconds['orca'], seconds['constant_velocity'], seconds['copy']
            gain, bar = med(o) - med(c), 3.0 * max(sd(o), sd(c))
            lines.append('%-46s orca / constant_velocity = %.1f x; constant_velocity / copy = %.2f x; orca - constant_velocity = '
                         '%.4f ms against a bar of 3 x the larger sd = %.4f ms' % (shape, med(o) / med(c), med(c) / med(y), gain * 1e3, bar * 1e3))
            verdicts.append((B, final_state, gain, bar))
        if B == max(cli.envs):
            plans = {}
            for model in ('orca', 'constant_velocity'):
                e2 = crowdnav_amd.BatchedCrowdSim(num_envs=B, num_humans=H, robot_policy=crowdnav_amd.ROBOT_EXTERNAL, robot_visible=1)
                e2.set_gamma(0.9)
                e2.set_lookahead_human_model(model)
                e2.rollout_begin(seed_base=1000, seed_mod=500, record_capacity=1)
                plans[model] = (e2, e2.plan_reset(e2.plan_begin(K, N, E, I, INIT_STD, seed=1)), [])
            for rep in range(-1, cli.reps):
                for model, (e2, plan, s) in plans.items():
                    dt = timed(lambda: e2.plan_rollout(plan, PLAN_STEPS, (rep + 1) * PLAN_STEPS * I), e2.sync, cli.limit)
                    if rep >= 0:
                        s.append(dt)
            for model, (e2, plan, s) in plans.items():
                lines.append('1 plan_rollout call (%d steps, %d envs, I = %d, E = %d) under %-18s median %9.3f ms  sd %7.3f ms  (%7.3f ms '
                             'per closed-loop step)' % (PLAN_STEPS, B, I, E, model, med(s) * 1e3, sd(s) * 1e3, med(s) * 1e3 / PLAN_STEPS))
                e2.close()
        eng.close()
    big, small = max(cli.envs), min(cli.envs)
    for B, final_state, gain, bar in verdicts:
        if B == big:
            lines.append('bar at %d envs (final_state8 %s): constant_velocity faster than orca by more than the margin: %s'
                         % (B, 'on' if final_state else 'off', 'MET' if gain > bar else 'NOT MET'))
        if B == small and small != big:
            lines.append('bar at %d envs (final_state8 %s): constant_velocity not slower than orca by more than the margin: %s'
                         % (B, 'on' if final_state else 'off', 'MET' if -gain <= bar else 'NOT MET'))
    text = '\n'.join(lines)
    print(text)
    if cli.out:
        with open(cli.out, 'a') as f:
            f.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
