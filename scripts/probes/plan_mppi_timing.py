"""What the MPPI update costs beside the CEM refit: ONE plan_mppi_rollout call (cn_plan_mppi_rollout) against ONE plan_rollout
call (cn_plan_rollout, CEM) making the same `--steps` closed-loop steps, alternating in one process.

    python scripts/probes/plan_mppi_timing.py [--envs 4096] [--reps 20] [--steps 4] [--cem-lib PATH] [--out profiles/plan_mppi_timing.txt]

--envs envs x 5 humans, external holonomic robot, K = 64 candidates, n = 12 steps, I = 3 iterations, init_std 0.5; CEM with
E = 8 elites, MPPI at temperature 1.0 with a fixed sampling deviation (fit_std off) — and, as a third column, with fit_std on,
which streams the candidates a second time.  --cem-lib: a libcrowdnav_amd.so of another revision (the parent commit's build) to
run the CEM column from, so that the yardstick is not the tree under test; without it the CEM column is this tree's.
After one warm-up round, --reps rounds of (CEM, MPPI, MPPI + fit_std); each is timed by the host clock from its call to the end of
a device synchronise.  The planners take different actions and so meet different episodes: the work per step is the same, and
nothing is compared but time.  Prints median and standard deviation of each and whether MPPI's median is within three times the
larger standard deviation of CEM's."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

H, K, N, I, E, INIT_STD, TEMPERATURE = 5, 64, 12, 3, 8, 0.5, 1.0


def other_library(path, lib_module):
    """Another revision's library, bound like the binding's own as far as it exports the binding's symbols."""
    lib = C.CDLL(path)
    for name, (res, args) in lib_module.SYMBOLS.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    if lib.cn_abi_version() != lib_module.ABI_VERSION:
        sys.exit('%s has ABI %d, the binding %d' % (path, lib.cn_abi_version(), lib_module.ABI_VERSION))
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--steps', type=int, default=4)
    ap.add_argument('--cem-lib', default=None)
    ap.add_argument('--out', default=None)
    cli = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('plan_mppi_timing needs the MI355X: nothing is measured without it')
    import crowdnav_amd
    from crowdnav_amd import _lib
    B = cli.envs
    mine = _lib.load()
    theirs = other_library(cli.cem_lib, _lib) if cli.cem_lib else mine

    def planner(lib):
        _lib._lib = lib  # the engine binds the library load() returns when it is made
        try:
            eng = crowdnav_amd.BatchedCrowdSim(num_envs=B, num_humans=H, robot_policy=crowdnav_amd.ROBOT_EXTERNAL, robot_visible=1)
        finally:
            _lib._lib = mine
        eng.set_gamma(0.9)
        eng.rollout_begin(seed_base=1000, seed_mod=500, record_capacity=1)
        return eng, eng.plan_reset(eng.plan_begin(K, N, E, I, INIT_STD, seed=1))

    (cem, cem_plan), (mppi, mppi_plan), (fit, fit_plan) = planner(theirs), planner(mine), planner(mine)
    counter = [0]

    def run_cem():
        cem.plan_rollout(cem_plan, cli.steps, counter[0])
        cem.sync()

    def run_mppi():
        mppi.plan_mppi_rollout(mppi_plan, cli.steps, TEMPERATURE, counter[0])
        mppi.sync()

    def run_fit():
        fit.plan_mppi_rollout(fit_plan, cli.steps, TEMPERATURE, counter[0], fit_std=True)
        fit.sync()

    cem_name = '1 plan_rollout call (CEM, %s)' % ('--cem-lib' if cli.cem_lib else 'this tree')
    kinds = ((cem_name, run_cem), ('1 plan_mppi_rollout call', run_mppi), ('1 plan_mppi_rollout call, fit_std', run_fit))
    seconds = {k[0]: [] for k in kinds}
    for rep in range(-1, cli.reps):  # (-1: warm-up)
        for name, call in kinds:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            if rep >= 0:
                seconds[name].append(time.perf_counter() - t0)
        counter[0] += cli.steps * I
    lines = ['plan_mppi_timing: %d envs x %d humans, K = %d, n = %d, I = %d, E = %d (CEM), temperature %g (MPPI), %d closed-loop steps '
             'per call, %d alternating rounds in one process after one warm-up round; host clock around the calls + synchronise'
             % (B, H, K, N, I, E, TEMPERATURE, cli.steps, cli.reps)]
    sd = lambda s: statistics.stdev(s) if len(s) > 1 else 0.0  # noqa: E731
    for name, _ in kinds:
        s = seconds[name]
        lines.append('%-44s median %9.3f ms  sd %7.3f ms  min %9.3f  max %9.3f  (%7.3f ms per closed-loop step)'
                     % (name, statistics.median(s) * 1e3, sd(s) * 1e3, min(s) * 1e3, max(s) * 1e3, statistics.median(s) * 1e3 / cli.steps))
    base = seconds[cem_name]
    for name, _ in kinds[1:]:
        s = seconds[name]
        slower, bar = statistics.median(s) - statistics.median(base), 3.0 * max(sd(base), sd(s))
        lines.append('%s - CEM = %.3f ms (medians) against a bar of 3 x the larger sd = %.3f ms: %s'
                     % (name, slower * 1e3, bar * 1e3, 'not slower' if slower <= bar else 'SLOWER by more than that margin'))
    text = '\n'.join(lines)
    print(text)
    if cli.out:
        with open(cli.out, 'a') as f:
            f.write(text + '\n')
    for eng in (cem, mppi, fit):
        eng.close()
    return 0


if __name__ == '__main__':
    sys.exit(main())
