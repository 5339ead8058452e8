"""What the bootstrap of a lookahead costs (cn_lookahead_values), against the lookahead alone, against what a user did before it
existed, and against the value-network kernel's own rate in a decision — alternating in one process:

    (a) lookahead(final_state=True)                                the K n-step branches and their final states
    (b) lookahead(bootstrap=True)                                  (a) + V of every final state + the score
    (c) (a), then compat.sarl.rotate and the torch module on the device over the B K final states
    (d) one sarl_select()                                          B x n_actions groups through the same network kernel

    python scripts/probes/lookahead_values_timing.py [--envs 4096] [--reps 20] [--out profiles/lookahead_values_timing.txt]

SARL fp32 at the shipped widths, 5 humans, external holonomic robot, reset from the test seeds and advanced 20 steps; K = 16
candidates of n = 20 actions from the 81-action space (a device tensor, made once).  After one warm-up round, --reps rounds of
(a, b, c, d), each timed by the host clock from its first call to the end of a device synchronise.  Reports the medians, (b) - (a),
(c) - (a), and the yardstick for (b) - (a): (d) x B K / (B x 81), the same network kernel pro rata.  --envs 8 is the narrow route."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

H = 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--candidates', type=int, default=16)
    ap.add_argument('--horizon', type=int, default=20)
    ap.add_argument('--out', default=None)
    cli = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('lookahead_values_timing needs the MI355X: nothing is measured without it')
    import crowdnav_amd
    from crowdnav_amd.compat.sarl import ValueNetwork, build_action_space, rotate
    B, K, n = cli.envs, cli.candidates, cli.horizon
    space = np.array([list(a) for a in build_action_space(1.0)[0]], dtype=np.float64)
    rng = np.random.RandomState(0)
    torch.manual_seed(0)
    net = ValueNetwork(13, 6, [150, 100], [100, 50], [150, 100, 100, 1], [100, 100, 1], True, 1.0, 4)
    eng = crowdnav_amd.BatchedCrowdSim(num_envs=B, num_humans=H, robot_policy=crowdnav_amd.ROBOT_EXTERNAL, robot_visible=1)
    eng.set_gamma(0.9)
    eng.sarl_configure(actions=space)
    eng.sarl_set_weights(net.state_dict())
    eng.reset(1000 + np.arange(B) % 500)
    warm = torch.from_numpy(space[rng.randint(len(space), size=(20, B))]).cuda()
    for t in range(20):
        eng.step(warm[t], update=True, want_obs=False)
    table = torch.from_numpy(space[rng.randint(len(space), size=(B, K, n))]).cuda()
    dev_net = ValueNetwork(13, 6, [150, 100], [100, 50], [150, 100, 100, 1], [100, 100, 1], True, 1.0, 4)
    dev_net.load_state_dict(net.state_dict())
    dev_net = dev_net.cuda()
    plain = eng.lookahead(table, final_state=True)
    boot = eng.lookahead(table, bootstrap=True)

    def torch_values(final_state8):
        s = final_state8.reshape(B * K, H + 1, 8).float()
        robot = s[:, :1, [0, 1, 2, 3, 6, 4, 5, 7]].expand(-1, H, -1)
        joint = torch.cat([robot, torch.zeros_like(robot[:, :, :1]), s[:, 1:, [0, 1, 2, 3, 6]]], dim=2)
        with torch.no_grad():
            return dev_net(rotate(joint.reshape(B * K * H, 14)).reshape(B * K, H, 13)).reshape(B, K)

    def a():
        eng.lookahead(table, final_state=True, out=plain)

    def b():
        eng.lookahead(table, bootstrap=True, out=boot)

    def c():
        eng.lookahead(table, final_state=True, out=plain)
        torch_values(plain['final_state8'])

    def d():
        eng.sarl_select()

    kinds = (('(a) lookahead(final_state=True)', a), ('(b) lookahead(bootstrap=True)', b),
             ('(c) (a) + rotate + torch module on the device', c), ('(d) one sarl_select()', d))
    seconds = {name: [] for name, _ in kinds}
    for rep in range(-1, cli.reps):  # (-1: warm-up)
        for name, call in kinds:
            eng.sync()
            t0 = time.perf_counter()
            call()
            eng.sync()
            torch.cuda.synchronize()
            if rep >= 0:
                seconds[name].append(time.perf_counter() - t0)
    agree = float((torch_values(boot['final_state8']) - boot['value']).abs().max())
    med = {name: statistics.median(s) * 1e3 for name, s in seconds.items()}
    lines = ['lookahead_values_timing: %d envs x %d humans, SARL fp32 (route %s), K = %d candidates, n = %d steps (%d final states), '
             '%d alternating rounds in one process after one warm-up round; host clock around the calls + synchronise'
             % (B, H, eng.sarl_network_route(), K, n, B * K, cli.reps)]
    for name, _ in kinds:
        s = seconds[name]
        lines.append('%-48s median %9.3f ms  sd %7.3f ms  min %9.3f  max %9.3f'
                     % (name, med[name], (statistics.stdev(s) if len(s) > 1 else 0.0) * 1e3, min(s) * 1e3, max(s) * 1e3))
    na, nb, nc, nd = (k[0] for k in kinds)
    yard = med[nd] * (B * K) / (B * len(space))
    lines.append('(b) - (a) = %.3f ms   (c) - (a) = %.3f ms   yardstick (d) x %d / %d = %.3f ms: the bootstrap costs %.2f x the yardstick'
                 % (med[nb] - med[na], med[nc] - med[na], B * K, B * len(space), yard, (med[nb] - med[na]) / yard))
    lines.append('max |value - torch on the device| over the %d final states: %.3g' % (B * K, agree))
    text = '\n'.join(lines)
    print(text)
    if cli.out:
        with open(cli.out, 'a') as f:
            f.write(text + '\n')
    eng.close()
    return 0


if __name__ == '__main__':
    sys.exit(main())
