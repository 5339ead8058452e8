"""The kernels behind transition.h that the other timing scripts do not reach, for an A/B of two builds of the library
(CROWDNAV_AMD_LIB): the unicycle instantiations of the lookahead and step_core kernels and the value network's narrow route.

    python scripts/probes/transition_unicycle_timing.py [--reps 20] [--limit 20]

Unicycle external robot, state 6 real steps after a seeded reset, actions from the 5 x 5 rotation space.  Per crowd — 4096
envs x 5 humans, 1024 x 8, 1024 x 12, 1024 x 12 with max_neighbors = 5: step_kernel<5, true, false>, <10, true, false>,
<10, true, true>, <5, true, true> and their rollout twins — one step(update=False), 12 rollout_step calls, one rollout_actions
of 12 steps without and with trace, one 'orca' lookahead (K = 8, n = 12); at 5 humans also one 'constant_velocity' lookahead, one
lookahead_paths and one lookahead_modes (M = 4) call at K = 64, n = 12.  Then 8 envs x 5 humans: sarl_select on the narrow route
without and with attention (holonomic), and 16 sampler steps of a unicycle engine at 5, 6 and 8 humans (on the narrow route
sarl_decide_step_kernel<5 | 10, true>, else step_kernel).  One warm-up, then --reps timed repetitions of every case in turn, host
clock around call + synchronise, each under --limit seconds; prints the median and standard deviation per case.  A case the
build refuses is reported as such and skipped."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

K, N, M = 64, 12, 4
BEGIN = dict(seed_base=1000, seed_mod=500, record_capacity=8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--limit', type=float, default=20.0)
    cli = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('transition_unicycle_timing needs the MI355X: nothing is measured without it')
    import crowdnav_amd as amd
    from crowdnav_amd import predict
    from crowdnav_amd.compat.sarl import ValueNetwork, build_action_space
    rot = np.array([list(a) for a in build_action_space(1.0, 5, 5, 'unicycle')[0]], dtype=np.float64)
    holo = np.array([list(a) for a in build_action_space(1.0)[0]], dtype=np.float64)
    cases, keep = [], []

    def unicycle_engine(B, H, **cfg):
        eng = amd.BatchedCrowdSim(num_envs=B, num_humans=H, robot_policy=amd.ROBOT_EXTERNAL, robot_visible=1, robot_kinematics=1, **cfg)
        eng.set_gamma(0.9)
        eng.reset(1000 + np.arange(B))
        for _ in range(6):
            eng.step(np.tile([1.0, 0.0], (B, 1)), update=True, want_obs=False)
        return eng

    for B, H, cfg in ((4096, 5, {}), (1024, 8, {}), (1024, 12, {}), (1024, 12, dict(max_neighbors=5))):
        what = '%d envs x %d humans%s, unicycle: ' % (B, H, ''.join(', %s = %s' % kv for kv in cfg.items()))
        eng = unicycle_engine(B, H, **cfg)
        rng = np.random.RandomState(3)
        one = torch.from_numpy(rot[rng.randint(len(rot), size=(B,))]).to(eng.device).contiguous()
        cases.append((what + 'step(update=False)', eng, lambda eng=eng, one=one: eng.step(one, update=False, want_obs=False)))
        roll = unicycle_engine(B, H, **cfg)
        roll.rollout_begin(**BEGIN)
        table = torch.from_numpy(rot[rng.randint(len(rot), size=(B, N))]).to(roll.device).contiguous()
        rows = [table[:, t].contiguous() for t in range(N)]
        cases.append((what + '%d rollout_step calls' % N, roll, lambda roll=roll, rows=rows: [roll.rollout_step(r) for r in rows]))
        cases.append((what + 'rollout_actions, %d steps' % N, roll, lambda roll=roll, table=table: roll.rollout_actions(table)))
        out = roll.rollout_actions(table, trace=True, rewards=True)
        cases.append((what + 'rollout_actions, %d steps, traced' % N, roll,
                      lambda roll=roll, table=table, out=out: roll.rollout_actions(table, trace=True, rewards=True, out=out)))
        look8 = torch.from_numpy(rot[rng.randint(len(rot), size=(B, 8, N))]).to(eng.device).contiguous()
        cases.append((what + "lookahead 'orca', K = 8, n = %d" % N, eng, lambda eng=eng, look8=look8: eng.lookahead(look8)))
        if H == 5:
            cv = unicycle_engine(B, H)
            cv.set_lookahead_human_model('constant_velocity')
            look = torch.from_numpy(rot[rng.randint(len(rot), size=(B, K, N))]).to(cv.device).contiguous()
            state = cv.get_state()[0]
            tables = [predict.constant_velocity(state, N).contiguous(), predict.to_goal(state, N, cv.config['time_step']).contiguous()]
            modes = predict.stack_modes(*(tables * (M // 2)))
            what = what + 'K = %d, n = %d: ' % (K, N)
            cases.append((what + "lookahead 'constant_velocity'", cv, lambda cv=cv, look=look: cv.lookahead(look)))
            cases.append((what + 'lookahead_paths', cv, lambda cv=cv, look=look, t=tables[1]: cv.lookahead_paths(look, t)))
            cases.append((what + 'lookahead_modes, M = %d' % M, cv, lambda cv=cv, look=look, modes=modes: cv.lookahead_modes(look, modes)))

    torch.manual_seed(0)
    net = ValueNetwork(13, 6, [150, 100], [100, 50], [150, 100, 100, 1], [100, 100, 1], True, 1.0, 4)
    try:
        se = amd.BatchedCrowdSim(num_envs=8, num_humans=5, robot_policy=amd.ROBOT_EXTERNAL, robot_visible=1)
        se.reset(2000 + np.arange(8))
        se.step(np.zeros((8, 2)), update=True)
        se.sarl_configure(actions=holo)
        se.sarl_set_weights(net.state_dict())
        route = se.sarl_network_route()
        cases.append(('8 envs x 5 humans: sarl_select (%s route)' % route, se, lambda se=se: se.sarl_select(want_values=False)))
        cases.append(('8 envs x 5 humans: sarl_select with attention (%s route)' % route, se,
                      lambda se=se: se.sarl_select(want_values=False, want_attention=True)))
    except Exception as err:  # noqa: BLE001
        print('REFUSED sarl_select cases: %s' % err)
    T = 16
    for H in (5, 6, 8):
        try:
            su = unicycle_engine(8, H)
            su.sarl_configure(actions=rot)
            su.sarl_set_weights(net.state_dict())
            dev = su.device
            bufs = dict(traj=torch.zeros((8, T, H, 13), dtype=torch.float32, device=dev), rew=torch.zeros((T, 8), dtype=torch.float64, device=dev),
                        info=torch.zeros((T, 8), dtype=torch.uint8, device=dev), dmin=torch.zeros((T, 8), dtype=torch.float64, device=dev),
                        act=torch.zeros((T, 8), dtype=torch.int32, device=dev), alive=torch.ones((8,), dtype=torch.uint8, device=dev),
                        done=torch.zeros((8,), dtype=torch.uint8, device=dev), action=torch.zeros((8, 2), dtype=torch.float64, device=dev))
            step = su.sarl_sampler(**bufs)
            keep.append((bufs, step))

            def sample(su=su, step=step, bufs=bufs):
                bufs['alive'].fill_(1), bufs['done'].zero_()
                for t in range(T):
                    step(t, 0.0)
            cases.append(('8 envs x %d humans, unicycle: %d sampler steps (%s route)' % (H, T, su.sarl_network_route()), su, sample))
        except Exception as err:  # noqa: BLE001
            print('REFUSED sampler case, %d humans: %s' % (H, err))

    seconds = {name: [] for name, _, _ in cases}
    for rep in range(-1, cli.reps):  # (-1: warm-up)
        for name, eng, call in cases:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            eng.sync()
            dt = time.perf_counter() - t0
            if dt > cli.limit:
                sys.exit('%s took %.1f s, over its limit of %.1f s' % (name, dt, cli.limit))
            if rep >= 0:
                seconds[name].append(dt)
    for name, _, _ in cases:
        s = seconds[name]
        print('%-88s median %9.4f ms  sd %7.4f ms' % (name, statistics.median(s) * 1e3, statistics.stdev(s) * 1e3 if len(s) > 1 else 0.0))
    return 0


if __name__ == '__main__':
    sys.exit(main())
