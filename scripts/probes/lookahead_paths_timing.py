"""What the lookahead under predicted human motion costs: ONE lookahead_paths() call against ONE lookahead() call under
'constant_velocity' on the same engine — existing code, the yardstick — alternating in one process, beside a device-to-device
copy of the bytes each call has to move.

    python scripts/probes/lookahead_paths_timing.py [--envs 4096 8] [--reps 20] [--out profiles/lookahead_paths_timing.txt]

Per --envs value: envs x 5 humans, external holonomic robot, K = 64 candidates of n = 12 steps drawn from the 81-action table,
from the state 6 real steps after a seeded reset; the velocity table is predict.to_goal's; without and with final_state8.
After one warm-up round, --reps rounds of (constant_velocity, paths, copy of the constant-velocity call's bytes, copy of the
paths call's bytes); each is timed by the host clock from its call to the end of a device synchronise, under a limit of its
own (--limit seconds: a region that takes longer ends the run).  The bytes: the action table [B][K][n][2] + the [B][K]
outputs (ret, info, steps, time; final_theta with the final state) + final_state8 [B][K][A][8] where asked, and for the paths
call the velocity table [B][n][H][2] on top.  The bar: the paths call is not slower than the constant-velocity call by more
than 3 standard deviations of either, after allowing the extra bytes pro rata (the constant-velocity mean scaled by the ratio
of the bytes moved).  Then one plan_cem_paths call against one plan_cem call under 'constant_velocity' (I = 3, E = 8) at every
shape, with no bar.  Prints means, medians and standard deviations and whether the bar is met."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

H, K, N, I, E, INIT_STD = 5, 64, 12, 3, 8, 0.5


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
        sys.exit('lookahead_paths_timing needs the MI355X: nothing is measured without it')
    import crowdnav_amd
    from crowdnav_amd import predict
    from crowdnav_amd.compat.sarl import build_action_space
    acts = np.array([list(a) for a in build_action_space(1.0)[0]], dtype=np.float64)
    sd = lambda s: statistics.stdev(s) if len(s) > 1 else 0.0  # noqa: E731
    mean, med = statistics.mean, statistics.median
    lines = ['lookahead_paths_timing: envs x %d humans, K = %d, n = %d, %d alternating rounds (constant_velocity, paths, copy, copy + '
             'table) in one process after one warm-up round; host clock around each call + synchronise' % (H, K, N, cli.reps)]
    for B in cli.envs:
        eng = crowdnav_amd.BatchedCrowdSim(num_envs=B, num_humans=H, robot_policy=crowdnav_amd.ROBOT_EXTERNAL, robot_visible=1)
        eng.set_gamma(0.9)
        eng.set_lookahead_human_model('constant_velocity')
        eng.reset(1000 + np.arange(B))
        for _ in range(6):
            eng.step(np.tile([0.0, 1.0], (B, 1)), update=True, want_obs=False)
        table = torch.from_numpy(acts[np.random.RandomState(3).randint(len(acts), size=(B, K, N))]).to(eng.device).contiguous()
        human_vel = predict.to_goal(eng.get_state()[0], N, eng.config['time_step'])
        assert human_vel.is_cuda and human_vel.is_contiguous() and tuple(human_vel.shape) == (B, N, H, 2)
        for final_state in (False, True):
            out = {m: eng.lookahead(table[:, :, :0].contiguous(), final_state=final_state) for m in ('constant_velocity', 'paths')}
            src = [table] + [out['paths'][k] for k in sorted(out['paths'])]
            dst = [torch.empty_like(t) for t in src]
            vel_dst = torch.empty_like(human_vel)
            nbytes = sum(t.numel() * t.element_size() for t in src)
            vbytes = human_vel.numel() * human_vel.element_size()

            def copy(with_table):
                for d, s in zip(dst, src):
                    d.copy_(s)
                if with_table:
                    vel_dst.copy_(human_vel)

            kinds = (('constant_velocity', lambda: eng.lookahead(table, final_state=final_state, out=out['constant_velocity'])),
                     ('paths', lambda: eng.lookahead_paths(table, human_vel, final_state=final_state, out=out['paths'])),
                     ('copy', lambda: copy(False)), ('copy + table', lambda: copy(True)))
            seconds = {k: [] for k, _ in kinds}
            for rep in range(-1, cli.reps):  # (-1: warm-up)
                for name, call in kinds:
                    dt = timed(call, eng.sync, cli.limit)
                    if rep >= 0:
                        seconds[name].append(dt)
            shape = '%d envs, final_state8 %s, %.1f MB + %.2f MB table' % (B, 'on ' if final_state else 'off', nbytes / 1e6, vbytes / 1e6)
            for name, _ in kinds:
                s = seconds[name]
                lines.append('%-52s %-18s mean %9.4f ms  median %9.4f ms  sd %7.4f ms  min %9.4f  max %9.4f'
                             % (shape, name, mean(s) * 1e3, med(s) * 1e3, sd(s) * 1e3, min(s) * 1e3, max(s) * 1e3))
            c, p = seconds['constant_velocity'], seconds['paths']
            allowed = mean(c) * (nbytes + vbytes) / nbytes
            over, bar = mean(p) - allowed, 3.0 * max(sd(c), sd(p))
            lines.append('%-52s paths / constant_velocity = %.3f x (bytes %.3f x); paths - constant_velocity pro rata = %.4f ms against '
                         'a bar of 3 x the larger sd = %.4f ms: %s' % (shape, mean(p) / mean(c), (nbytes + vbytes) / nbytes, over * 1e3,
                                                                       bar * 1e3, 'MET' if over <= bar else 'NOT MET'))
        plans = {name: (eng.plan_reset(eng.plan_begin(K, N, E, I, INIT_STD, seed=1)), []) for name in ('plan_cem', 'plan_cem_paths')}
        for rep in range(-1, cli.reps):
            for name, (plan, s) in plans.items():
                counter = (rep + 1) * I
                call = (lambda: eng.plan_cem(plan, counter)) if name == 'plan_cem' else (lambda: eng.plan_cem_paths(plan, human_vel, counter))
                dt = timed(call, eng.sync, cli.limit)
                if rep >= 0:
                    s.append(dt)
        for name, (plan, s) in plans.items():
            lines.append('1 %-14s call (%d envs, I = %d, E = %d; plan_cem under constant_velocity)  mean %9.4f ms  median %9.4f ms  sd %7.4f ms'
                         % (name, B, I, E, mean(s) * 1e3, med(s) * 1e3, sd(s) * 1e3))
        eng.close()
    text = '\n'.join(lines)
    print(text)
    if cli.out:
        with open(cli.out, 'a') as f:
            f.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
