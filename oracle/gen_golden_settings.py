"""ORACLE — TEST INFRASTRUCTURE ONLY.

Generates tests/golden/settings_<name>.npz: the UNMODIFIED reference (ref_harness.make_env(overrides=...)) at the settings of
tests/env_setting_cases.py that env.config can express — a few 'test' episodes with the robot invisible and visible (the arrays of
traj_*.npz under the prefixes invisible_ / visible_, plus `times`: env.global_time after every step, as the reference accumulated
it) and the reset states, seeds and stream probe of resets.npz.  The overrides travel in the file as data: overrides_json
('section.key' -> value) and config_json (the cn_config keywords they map to).

    make -C oracle && PYTHONDONTWRITEBYTECODE=1 python oracle/gen_golden_settings.py [name ...]
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'tests'))
import gen_golden as gg  # noqa: E402
import ref_harness as rh  # noqa: E402
import env_setting_cases as cases  # noqa: E402

OUT = gg.OUT
RESETS = 8


def make_env(s, visible):
    """A fresh env, robot and ORCA policy per episode: a persistent policy keeps the radii of its first episode (orca.py:95-110)."""
    ov = cases.reference_overrides(cases.reference_config(s))
    safety = ov.pop('robot_policy.safety_space', None)
    env, robot, policy = rh.make_env(robot_visible=visible, human_num=s.humans,
                                     overrides={tuple(k.split('.')): v for k, v in ov.items()})
    if safety is not None:
        policy.safety_space = safety  # an attribute, as crowd_nav/train.py:122-127 sets it
    return env, robot, policy


def run_episode(env, robot, case):
    """gen_golden.run_episode + the accumulated env.global_time after every step."""
    ob = env.reset('test', case)
    e = dict(states=[gg.snapshot(env)], actions=[], rewards=[], dones=[], infos=[], dmins=[], times=[])
    done = False
    while not done:
        action = robot.act(ob)
        ob, reward, done, info = env.step(action)
        name = type(info).__name__
        e['states'].append(gg.snapshot(env))
        e['actions'].append([action.vx, action.vy])
        e['rewards'].append(float(reward))
        e['dones'].append(bool(done))
        e['infos'].append(gg.INFO_CODE[name])
        e['dmins'].append(float(info.min_dist) if name == 'Danger' else np.nan)
        e['times'].append(float(env.global_time))
    out = dict(states=np.array(e['states']), actions=np.array(e['actions'], dtype=np.float64),
               rewards=np.array(e['rewards'], dtype=np.float64), dones=np.array(e['dones'], dtype=np.uint8),
               infos=np.array(e['infos'], dtype=np.uint8), dmins=np.array(e['dmins'], dtype=np.float64),
               global_time=float(env.global_time))
    return out, np.array(e['times'], dtype=np.float64)


def generate(name, out_dir=None):
    s = cases.BY_NAME[name]
    config = cases.reference_config(s)
    d = dict(config_json=np.array(json.dumps(config, sort_keys=True)),
             overrides_json=np.array(json.dumps(cases.reference_overrides(config), sort_keys=True)),
             num_humans=np.array(s.humans), cases=np.arange(s.cases, dtype=np.int64))
    for tag, visible in (('invisible', False), ('visible', True)):
        eps, times = [], []
        for c in range(s.cases):
            env, robot, _ = make_env(s, visible)
            e, t = run_episode(env, robot, c)
            eps.append(e)
            times.append(t)
        packed = gg.pack(eps)
        packed['times'] = np.concatenate(times)
        d.update({tag + '_' + k: v for k, v in packed.items()})
        print(name, tag, 'steps', packed['steps'].tolist(), 'outcomes',
              np.bincount(packed['infos'][np.cumsum(packed['steps']) - 1], minlength=5).tolist(),
              'danger steps', int((packed['infos'] == 1).sum()))
    env, robot, _ = make_env(s, False)
    states, probes = [], []
    for c in range(RESETS):
        env.reset('test', c)
        states.append(gg.snapshot(env))
        probes.append(np.random.random())  # next value of the stream = position check
    d.update(reset_states=np.array(states), reset_probe=np.array(probes), reset_seeds=1000 + np.arange(RESETS, dtype=np.uint32))
    np.savez_compressed(os.path.join(out_dir or OUT, cases.fixture_name(s)), **d)


if __name__ == '__main__':
    assert rh.available(), 'needs the reference and oracle/_build (make -C oracle)'
    for n in sys.argv[1:] or cases.FIXTURES:
        generate(n)
