"""What the device CEM planner saves: ONE plan_rollout call (cn_plan_rollout) making `--steps` closed-loop steps, against the same
algorithm composed from the public API that existed before it, in torch — torch.randn, the clip, lookahead, topk, mean / std,
gather, rollout_step, the shift and the re-seed of ended episodes — with no .item() inside the loop; alternating in one process.

    python scripts/probes/plan_cem_timing.py [--envs 4096] [--reps 10] [--steps 8] [--out profiles/plan_cem_timing.txt]

--envs envs x 5 humans, external holonomic robot, K = 64 candidates, n = 12 steps, I = 3 iterations, E = 8 elites, init_std 0.5.
After one warm-up round, --reps rounds of (composition, plan_rollout); each is timed by the host clock from its first call to
the end of a device synchronise.  The two draw different random numbers (torch's generator against Philox keyed by the plan's
seed) and so plan different trajectories: the work per step is the same, the episodes are not, and nothing is compared but time.
Prints median and standard deviation of both and whether the one-call form is no slower than the composition by more than
three times the larger standard deviation."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

H, K, N, I, E, INIT_STD, V_PREF, DT = 5, 64, 12, 3, 8, 0.5, 1.0, 0.25


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--steps', type=int, default=8)
    ap.add_argument('--out', default=None)
    cli = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('plan_cem_timing needs the MI355X: nothing is measured without it')
    import crowdnav_amd
    B = cli.envs

    def engine():
        eng = crowdnav_amd.BatchedCrowdSim(num_envs=B, num_humans=H, robot_policy=crowdnav_amd.ROBOT_EXTERNAL, robot_visible=1)
        eng.set_gamma(0.9)
        return eng, eng.rollout_begin(seed_base=1000, seed_mod=500, record_capacity=1)

    (old, obufs), (new, _) = engine(), engine()
    plan = new.plan_reset(new.plan_begin(K, N, E, I, INIT_STD, seed=1))
    rows = torch.arange(B, device=old.device)

    def prior():
        robot = old.get_state()[0][:, 0]
        d = robot[:, 4:6] - robot[:, 0:2]
        dist = d.norm(dim=-1, keepdim=True)
        return torch.where(dist > 0, d / dist * torch.minimum(robot[:, 7:8], dist / DT), torch.zeros_like(d))

    held = dict(mean=prior()[:, None].repeat(1, N, 1), std=torch.full((B, N, 2), INIT_STD, dtype=torch.float64, device=old.device),
                look=None)

    def composition():
        mean, std = held['mean'], held['std']
        for _ in range(cli.steps):
            best_score = best = None
            for i in range(I):
                cand = mean[:, None] + std[:, None] * torch.randn((B, K, N, 2), dtype=torch.float64, device=old.device)
                cand[:, 0] = mean
                nrm = cand.norm(dim=-1, keepdim=True)
                cand = torch.where(nrm > V_PREF, cand * (V_PREF / nrm), cand).contiguous()
                held['look'] = old.lookahead(cand, out=held['look'])
                score, top = held['look']['ret'].topk(E, dim=1)
                elites = cand[rows[:, None], top]
                if i == 0:
                    best_score, best = score[:, 0].clone(), elites[:, 0].clone()
                else:
                    better = score[:, 0] > best_score
                    best_score = torch.where(better, score[:, 0], best_score)
                    best = torch.where(better[:, None, None], elites[:, 0], best)
                mean, std = elites.mean(dim=1), elites.std(dim=1, unbiased=False)
            old.rollout_step(best[:, 0].contiguous())
            ended = (obufs['cur_steps'] == 0)[:, None, None]
            mean = torch.where(ended, prior()[:, None], torch.cat([mean[:, 1:], mean[:, -1:]], dim=1))
            std = torch.full_like(std, INIT_STD)
        held['mean'], held['std'] = mean, std
        old.sync()

    counter = [0]

    def one_call():
        new.plan_rollout(plan, cli.steps, counter[0])
        counter[0] += cli.steps * I
        new.sync()

    kinds = (('composition in torch over the public API', composition), ('1 plan_rollout call', one_call))
    seconds = {k[0]: [] for k in kinds}
    for rep in range(-1, cli.reps):  # (-1: warm-up)
        for name, call in kinds:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            if rep >= 0:
                seconds[name].append(time.perf_counter() - t0)
    lines = ['plan_cem_timing: %d envs x %d humans, K = %d, n = %d, I = %d, E = %d, %d closed-loop steps per call, %d alternating rounds '
             'in one process after one warm-up round; host clock around the calls + synchronise' % (B, H, K, N, I, E, cli.steps, cli.reps)]
    for name, _ in kinds:
        s = seconds[name]
        lines.append('%-44s median %9.3f ms  sd %7.3f ms  min %9.3f  max %9.3f  (%7.3f ms per closed-loop step)'
                     % (name, statistics.median(s) * 1e3, statistics.stdev(s) * 1e3 if len(s) > 1 else 0.0, min(s) * 1e3, max(s) * 1e3,
                        statistics.median(s) * 1e3 / cli.steps))
    comp, one = seconds[kinds[0][0]], seconds[kinds[1][0]]
    slower = statistics.median(one) - statistics.median(comp)
    bar = 3.0 * max(statistics.stdev(comp), statistics.stdev(one)) if cli.reps > 1 else float('nan')
    lines.append('composition / plan_rollout = %.2f (medians); plan_rollout - composition = %.3f ms against a bar of 3 x the larger sd = '
                 '%.3f ms: %s' % (statistics.median(comp) / statistics.median(one), slower * 1e3, bar * 1e3,
                                  'not slower' if slower <= bar else 'SLOWER by more than that margin'))
    text = '\n'.join(lines)
    print(text)
    if cli.out:
        with open(cli.out, 'a') as f:
            f.write(text + '\n')
    old.close(), new.close()
    return 0


if __name__ == '__main__':
    sys.exit(main())
