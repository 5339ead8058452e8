"""What scoring against M predicted futures costs: ONE lookahead_modes() call against the composition it replaces — M
lookahead_paths() calls on M contiguous tables (existing code with unchanged assembly: the yardstick), alone and followed by
the reduction in torch — alternating in one process, beside device-to-device copies of the bytes each side has to move.

    python scripts/probes/lookahead_modes_timing.py [--shapes 4096:4 4096:8 8:4] [--reps 20] [--out profiles/lookahead_modes_timing.txt]

Per --shapes value envs:M: envs x 5 humans, external holonomic robot, K = 64 candidates of n = 12 steps drawn from the 81-action
table, from the state 6 real steps after a seeded reset; mode 0 is predict.constant_velocity's table, mode 1 predict.to_goal's,
the others the state velocities under a seeded random walk.  After one warm-up round, --reps rounds of (M paths calls, M paths
calls + torch reduction, one modes call, copy of the composition's bytes, copy of the fused call's bytes); each is timed by the
host clock from its first call to the end of a device synchronise, under a limit of its own (--limit seconds: a region that
takes longer ends the run).  The bytes.  Composition: M x (action table [B][K][n][2] + ret, info, steps, time [B][K] + one table
[B][n][H][2]).  Fused: the action table once + score, risk, worst_mode, worst_info, worst_steps, worst_time [B][K] + the M
tables.  The bar, at 4096 envs only: the fused call's mean lies below the mean of the M paths calls alone by more than three
pooled standard deviations (sqrt of the mean of the two variances).  Smaller shapes are launch-bound on both sides: reported
without a bar.  Then one plan_cem_modes call (I = 3, E = 8) against the same planning step composed from Python (draw,
lookahead_modes, copies into plan.look, refit), with no bar."""
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

H, K, N, I, E, INIT_STD = 5, 64, 12, 3, 8, 0.5
BAR_ENVS = 4096


def timed(call, sync, limit):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    call()
    sync()
    dt = time.perf_counter() - t0
    if dt > limit:
        sys.exit('a timed region took %.1f s, over its limit of %.1f s' % (dt, limit))
    return dt


def nbytes(tensors):
    return sum(t.numel() * t.element_size() for t in tensors)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', nargs='+', default=['4096:4', '4096:8', '8:4'])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--limit', type=float, default=20.0)
    ap.add_argument('--out', default=None)
    cli = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('lookahead_modes_timing needs the MI355X: nothing is measured without it')
    import crowdnav_amd
    from crowdnav_amd import predict
    from crowdnav_amd.compat.sarl import build_action_space
    acts = np.array([list(a) for a in build_action_space(1.0)[0]], dtype=np.float64)
    sd = lambda s: statistics.stdev(s) if len(s) > 1 else 0.0  # noqa: E731
    mean, med = statistics.mean, statistics.median
    lines = ['lookahead_modes_timing: envs x %d humans, K = %d, n = %d, %d alternating rounds (M paths calls, M paths calls + torch '
             'reduction, 1 modes call, copies) in one process after one warm-up round; host clock around each region + synchronise'
             % (H, K, N, cli.reps)]
    met = True
    for shape in cli.shapes:
        B, M = (int(x) for x in shape.split(':'))
        eng = crowdnav_amd.BatchedCrowdSim(num_envs=B, num_humans=H, robot_policy=crowdnav_amd.ROBOT_EXTERNAL, robot_visible=1)
        eng.set_gamma(0.9)
        eng.reset(1000 + np.arange(B))
        for _ in range(6):
            eng.step(np.tile([0.0, 1.0], (B, 1)), update=True, want_obs=False)
        table = torch.from_numpy(acts[np.random.RandomState(3).randint(len(acts), size=(B, K, N))]).to(eng.device).contiguous()
        state = eng.get_state()[0]
        gen = torch.Generator().manual_seed(5)
        tables = [predict.constant_velocity(state, N), predict.to_goal(state, N, eng.config['time_step'])]
        for _ in range(2, M):
            walk = torch.cumsum(0.15 * torch.randn((B, N, H, 2), generator=gen, dtype=torch.float64), dim=1).to(eng.device)
            tables.append((tables[0] + walk).contiguous())
        tables = [t.contiguous() for t in tables[:M]]
        human_vel = predict.stack_modes(*tables)
        assert human_vel.is_cuda and human_vel.is_contiguous() and tuple(human_vel.shape) == (B, M, N, H, 2)
        weights = torch.full((B, M), 1.0 / M, dtype=torch.float64, device=eng.device)
        empty = table[:, :, :0].contiguous()
        outs = [eng.lookahead(empty) for _ in range(M)]  # (n = 0: the tensors, unwritten)
        fused = eng.lookahead_modes(empty, human_vel[:, :, :0].contiguous())
        collision = crowdnav_amd.COLLISION

        def composition():
            for m in range(M):
                eng.lookahead_paths(table, tables[m], out=outs[m])

        def reduction():
            composition()
            ret = torch.stack([o['ret'] for o in outs], dim=2)
            hit = torch.stack([o['info'] for o in outs], dim=2) == collision
            risk = (weights[:, None, :] * hit).sum(dim=2)
            score = (weights[:, None, :] * ret).sum(dim=2) - 0.5 * risk
            worst = ret.argmin(dim=2)
            return score, risk, worst

        src_c = [table] * M + [o[k] for o in outs for k in ('ret', 'info', 'steps', 'time')] + tables
        src_f = [table] + [fused[k] for k in sorted(fused)] + [human_vel]
        dst_c, dst_f = [torch.empty_like(t) for t in src_c], [torch.empty_like(t) for t in src_f]

        def copy(dst, src):
            for d, s in zip(dst, src):
                d.copy_(s)

        kinds = (('%d paths calls' % M, composition), ('%d paths calls + reduction' % M, reduction),
                 ('1 modes call', lambda: eng.lookahead_modes(table, human_vel, weights=weights, risk_penalty=0.5, out=fused)),
                 ('copy, composition', lambda: copy(dst_c, src_c)), ('copy, fused', lambda: copy(dst_f, src_f)))
        seconds = {k: [] for k, _ in kinds}
        for rep in range(-1, cli.reps):  # (-1: warm-up)
            for name, call in kinds:
                dt = timed(call, eng.sync, cli.limit)
                if rep >= 0:
                    seconds[name].append(dt)
        bytes_c, bytes_f = nbytes(src_c), nbytes(src_f)
        what = '%d envs, M = %d (%.1f MB composition, %.1f MB fused)' % (B, M, bytes_c / 1e6, bytes_f / 1e6)
        for name, _ in kinds:
            s = seconds[name]
            lines.append('%-52s %-28s mean %9.4f ms  median %9.4f ms  sd %7.4f ms  min %9.4f  max %9.4f'
                         % (what, name, mean(s) * 1e3, med(s) * 1e3, sd(s) * 1e3, min(s) * 1e3, max(s) * 1e3))
        c, r, f = (seconds[name] for name, _ in kinds[:3])
        pooled = math.sqrt((sd(c) ** 2 + sd(f) ** 2) / 2.0)
        gain = mean(c) - mean(f)
        verdict = 'no bar (launch-bound on both sides)'
        if B >= BAR_ENVS:
            ok = gain > 3.0 * pooled
            met = met and ok
            verdict = 'bar (more than 3 pooled sd = %.4f ms): %s' % (3.0 * pooled * 1e3, 'MET' if ok else 'NOT MET')
        lines.append('%-52s modes / paths calls = %.3f x, modes / (paths calls + reduction) = %.3f x, bytes fused / composition = %.3f x; '
                     'paths calls - modes = %.4f ms; %s' % (what, mean(f) / mean(c), mean(f) / mean(r), bytes_f / bytes_c, gain * 1e3, verdict))
        if M == 4:  # one planning step: the one C call against the same step composed from Python
            plans = {name: (eng.plan_reset(eng.plan_begin(K, N, E, I, INIT_STD, seed=1)), []) for name in ('plan_cem_modes', 'composed')}

            def composed(plan, counter):
                for i in range(I):
                    eng.plan_draw(plan, counter + i)
                    got = eng.lookahead_modes(plan.candidates, human_vel, weights=weights, risk_penalty=0.5, out=fused)
                    for key, row in (('ret', 'score'), ('info', 'worst_info'), ('steps', 'worst_steps'), ('time', 'worst_time')):
                        plan.look[key].copy_(got[row])
                    eng.plan_refit(plan, keep_best=i > 0)

            for rep in range(-1, cli.reps):
                for name, (plan, s) in plans.items():
                    counter = (rep + 1) * I
                    call = ((lambda: eng.plan_cem_modes(plan, human_vel, counter, weights=weights, risk_penalty=0.5))
                            if name == 'plan_cem_modes' else (lambda: composed(plan, counter)))
                    dt = timed(call, eng.sync, cli.limit)
                    if rep >= 0:
                        s.append(dt)
            for name, (plan, s) in plans.items():
                lines.append('1 %-14s planning step (%d envs, I = %d, E = %d, M = %d)  mean %9.4f ms  median %9.4f ms  sd %7.4f ms'
                             % (name, B, I, E, M, mean(s) * 1e3, med(s) * 1e3, sd(s) * 1e3))
        eng.close()
    lines.append('the bar at %d envs: %s' % (BAR_ENVS, 'MET' if met else 'NOT MET'))
    text = '\n'.join(lines)
    print(text)
    if cli.out:
        with open(cli.out, 'a') as f:
            f.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
