"""TEST INFRASTRUCTURE ONLY — runs where the reference is (oracle/ref_harness.py finds it); never on the GPU box.

Generates tests/golden/sarl_attention.npz with the UNMODIFIED reference: crowd_nav.policy.sarl.SARL (random-init weights,
torch.manual_seed(0), 'test' phase) driving crowd_sim CrowdSim on top of oracle/shims + the float32 rvo2 restatement, and
records what CrowdSim keeps of the policy's attention (crowd_sim.py:303-304, 396-397): after every env.step the new entry
of env.attention_weights — the softmax weights SARL's LAST forward left (sarl.py:54), i.e. those of the last action's
lookahead state (multi_human_rl.py:35-51).  Per decision also the agent states before it (padded with NaN to the fixture's
human slots under the `mixed` rule), the human count, the chosen action and the rotated network input of that last
forward (captured by a forward pre-hook; nothing of the reference is patched).  Four fixtures under one file, key prefix
<fixture>_: plain (5 humans), om (occupancy maps), h12 (12 humans), mixed (test_sim = mixed, episodes of 1..4 humans);
the weights once per input width: param_<key> (13 features), om_param_<key> (+ occupancy maps).

    make -C oracle && PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_attention.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
import ref_harness as rh  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'sarl_attention.npz')


def snapshot(env, slots):
    rows = np.full((1 + slots, 8), np.nan)
    for i, a in enumerate([env.robot] + env.humans):
        rows[i] = [a.px, a.py, a.vx, a.vy, a.gx, a.gy, a.radius, a.v_pref]
    return rows


def make(with_om, human_num, mixed):
    rh.activate()
    torch.manual_seed(0)
    pcfg = rh.read_config('policy.config', {('sarl', 'with_om'): 'true' if with_om else 'false'})
    env, robot, policy = rh.make_env(robot_visible=True, policy_name='sarl', policy_config=pcfg, human_num=human_num,
                                     overrides={('sim', 'test_sim'): 'mixed'} if mixed else None)
    policy.set_device(torch.device('cpu'))
    policy.set_phase('test')
    policy.set_env(env)
    return env, robot, policy


def run(out, name, with_om, human_num, cases, max_steps, mixed=False, min_humans=1):
    rec = dict(states=[], count=[], gtime=[], best=[], action=[], x_last=[], attention=[], case=[], step=[])
    params = None
    env = robot = policy = None
    for case in cases:
        if env is None or mixed:  # the reference survives one mixed reset per env (oracle/gen_golden_mixed.py)
            env, robot, policy = make(with_om, human_num, mixed)
            last = {}
            policy.get_model().register_forward_pre_hook(lambda m, inp: last.__setitem__('x', inp[0].detach().clone()))
        if params is None:
            params = {k: v.numpy().copy() for k, v in policy.get_model().state_dict().items()}
        ob = env.reset('test', case)
        if len(env.humans) < min_humans:
            continue
        done, t = False, 0
        while not done and t < max_steps:
            state8, gt = snapshot(env, human_num), env.global_time
            action = robot.act(ob)
            chosen = [i for i, a in enumerate(policy.action_space) if a == action]
            ob, _, done, _ = env.step(action)
            n = len(env.humans)
            att = np.full(human_num, np.nan, np.float32)
            att[:n] = env.attention_weights[-1]
            x = np.zeros((human_num, policy.input_dim()), np.float32)
            x[:n] = last['x'][0].numpy()
            rec['states'].append(state8)
            rec['count'].append(n)
            rec['gtime'].append(gt)
            rec['best'].append(chosen[0])
            rec['action'].append(list(action))
            rec['x_last'].append(x)
            rec['attention'].append(att)
            rec['case'].append(case)
            rec['step'].append(t)
            t += 1
        assert len(env.attention_weights) == t
    for k, v in rec.items():
        out['%s_%s' % (name, k)] = np.array(v)
    # the same seed gives the same weights to every network of the same input width: stored once per width
    prefix = 'om_param_' if with_om else 'param_'
    for k, v in params.items():
        assert prefix + k not in out or np.array_equal(out[prefix + k], v)
        out[prefix + k] = v
    out['%s_with_om' % name] = np.array(int(with_om))
    out['%s_action_space' % name] = np.array([list(a) for a in policy.action_space], dtype=np.float64)
    print(name, 'decisions', len(rec['best']), 'cases', sorted(set(rec['case'])), 'humans', sorted(set(rec['count'])))


def main():
    assert rh.available()
    out = {}
    run(out, 'plain', with_om=False, human_num=5, cases=[0, 1], max_steps=6)
    run(out, 'om', with_om=True, human_num=5, cases=[3], max_steps=6)
    run(out, 'h12', with_om=False, human_num=12, cases=[15], max_steps=4)
    # `mixed`: only episodes of fewer than 5 humans (the engine keeps 5 slots and parks the absent ones)
    run(out, 'mixed', with_om=False, human_num=5, cases=[c for c in range(12)], max_steps=3, mixed=True)
    keep = [i for i, n in enumerate(out['mixed_count']) if n < 5]
    for k in ('states', 'count', 'gtime', 'best', 'action', 'x_last', 'attention', 'case', 'step'):
        out['mixed_' + k] = out['mixed_' + k][keep]
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
