"""Explorer — the reference's episode driver surface (crowd_nav/utils/explorer.py:7-125).

run_k_episodes(k, phase, ...) keeps the reference's signature, bookkeeping and log lines.  When the robot's
policy lives on the device (ORCA) and no replay memory has to be filled, all k episodes run as ONE batch of
min(k, max_envs) envs inside the fused rollout kernel (cn_rollout): episode i of the call is the scenario the
reference would have produced on its i-th env.reset(phase).  Otherwise the reference's own loop runs on top of
CrowdSim.step (one launch per transition).  _route names the driver of a call; what the RL sampling phase keeps between
calls is rl_sampler.RlSampler, the target network's forward td_targets.TdTargets."""
import copy
import logging
import time

import numpy as np
import torch

from .. import _lib
from ..engine import BatchedCrowdSim
from .policy import is_device_orca
from .rl_sampler import UNWRITTEN, RlSampler
from .sarl import SARL
from ..sarl_rollout import SarlRollout
from .td_targets import TdTargets
from ..trace import episodes as trace_episodes
from .types import Collision, Danger, ReachGoal, Timeout


def average(values):
    return sum(values) / len(values) if values else 0


def episode_statistics(outcome, times, returns, danger_n, danger_sum, timeout_time=None):
    """The eight values _report takes (explorer.py:50-72) from per-episode lists in case order: end code, end time, discounted
    return, number of Danger steps and the sum of their min distances.  A timed-out episode counts with its own end time, or
    with timeout_time where one is given (the reference appends env.time_limit)."""
    ended = list(zip(outcome, times))
    too_close = sum(danger_n)
    return ([t for o, t in ended if o == _lib.REACH_GOAL],
            [t for o, t in ended if o == _lib.COLLISION],
            [t if timeout_time is None else timeout_time for o, t in ended if o == _lib.TIMEOUT],
            [i for i, o in enumerate(outcome) if o == _lib.COLLISION],
            [i for i, o in enumerate(outcome) if o == _lib.TIMEOUT],
            too_close, sum(danger_sum) / too_close if too_close else 0, returns)


def episode_ends(info):
    """info: [T, B] step codes of B lock-step envs that kept stepping (or kept stale rows) behind their episode's end.  Returns
    per env the steps of its episode (up to its first end code) and that code, and the indices of the episodes that enter the
    replay memory (ReachGoal / Collision: explorer.py:66-69)."""
    terminal = info >= _lib.REACH_GOAL
    if not terminal.any(axis=0).all():
        raise ValueError('Invalid end signal from environment')
    steps = terminal.argmax(axis=0) + 1
    last = info[steps - 1, np.arange(info.shape[1])]
    return steps, last, np.flatnonzero((last == _lib.REACH_GOAL) | (last == _lib.COLLISION))


def danger_sums(info, dmin, steps):
    """Per env: its Danger steps up to its episode's end and the sum of their min distances (dmin: [T, B]), as two lists."""
    danger_n, danger_sum = [], []
    for b, n in enumerate(steps):
        dang = info[:n, b] == _lib.DANGER
        danger_n.append(int(dang.sum()))
        danger_sum.append(float(dmin[:n, b][dang].sum()))
    return danger_n, danger_sum


def episodes_of_histories(info, dmin):
    """Lock-step histories -> episodes: steps, last code, Danger count, Danger min-distance sum, kept indices (the two rules
    above in one call; the RL driver runs the second behind its push, where the host's statistics overlap the device's work)."""
    steps, last, keep = episode_ends(info)
    return (steps, last) + danger_sums(info, dmin, steps) + (keep,)


def _no_lap(name):
    return None


def _laps(prof):
    """lap(name): the seconds since the previous lap, added to prof[name] (synchronising: debugging only).  prof None: no-op."""
    if prof is None:
        return _no_lap
    torch.cuda.synchronize()
    tp = [time.perf_counter()]

    def lap(name):
        torch.cuda.synchronize()
        tp.append(time.perf_counter())
        prof[name] = prof.get(name, 0.0) + tp[-1] - tp[-2]
    return lap


class Explorer(object):
    max_envs = 4096  # envs per batched launch
    # Batched ORCA-robot runs (_run_batched) keep every episode's joint states when this is set: last_batch['trajectories'] is
    # then a list in case order of float64 [steps, A, 8] arrays — the state before each transition, the reference's env.states
    # without its last entry (engine.rollout_trace).  An attribute, not a parameter: run_k_episodes keeps the reference's
    # signature.  Off: nothing is recorded, launched or allocated for it.
    keep_trajectories = False

    def __init__(self, env, robot, device, memory=None, gamma=None, target_policy=None):
        self.env = env
        self.robot = robot
        self.device = device
        self.memory = memory
        self.gamma = gamma
        self.target_policy = target_policy
        self.target_model = None
        self.last_batch = None  # per-episode arrays of the last batched call (for callers that want more)
        self.last_stats = None  # what the last call logged
        self.rl_profile = None  # dict: seconds per part of the RL sampling calls (scripts/probes/rl_parts.py)
        self.rl = RlSampler()   # what the RL sampling phase keeps between calls
        self.td = TdTargets()   # the target network's forward for the TD targets

    def update_target_model(self, target_model):
        """explorer.py:26-27 (copy.deepcopy).  When a target network of the same architecture exists already, its parameters
        are overwritten in place: the same values, and the captured graph of its forward (TdTargets) stays valid."""
        old = self.target_model
        if old is not None and type(old) is type(target_model):
            try:
                src, dst = target_model.state_dict(), old.state_dict()
                if src.keys() == dst.keys() and all(src[k].shape == dst[k].shape and src[k].dtype == dst[k].dtype and
                                                    src[k].device == dst[k].device for k in src):
                    old.load_state_dict(src)
                    old.train(target_model.training)  # (what copy.deepcopy would have carried over besides the parameters)
                    return
            except RuntimeError:
                pass
        self.target_model = copy.deepcopy(target_model)
        self.td.drop_graph()

    # The names under which callers written against the one-module Explorer read what now lives on self.rl and self.td
    # (read-only views; the histories have no such name: they were a tuple read by position, and are Explorer.rl.hist)
    _td_graph = property(lambda self: self.td.graph)
    _td_engine = property(lambda self: self.td.engine)
    _rl_engine_cache = property(lambda self: None if self.rl.eng is None else (self.rl._key, self.rl.eng, self.rl._space))

    def _rl_engine(self, B, human_num, rule):
        return self.rl.engine(self.env, self.robot, B, human_num, rule)

    def _td_values(self, nxt):
        """target_model(next states), flat: what TdTargets needs from here — the robot's policy and the sampling engine's
        configuration (None while there is no such engine)."""
        return self.td.values(self.target_model, nxt, self.robot.policy if self.robot is not None else None, self.rl.config)

    # ------------------------------------------------------------------ explorer.py:21-90
    def run_k_episodes(self, k, phase, update_memory=False, imitation_learning=False, episode=None,
                       print_failure=False):
        self.robot.policy.set_phase(phase)
        route = self._route(k, phase, update_memory, imitation_learning)
        if route == 'imitation':
            stats = self._run_batched_imitation(k, phase)
        elif route == 'rl':
            stats = self._run_batched_rl(k, phase)
        elif route == 'batched':
            stats = self._run_batched(k, phase)
        else:
            stats = self._run_sequential(k, phase, update_memory, imitation_learning)
        self._report(k, phase, episode, print_failure, *stats)

    def _route(self, k, phase, update_memory, imitation_learning):
        """Which driver runs this call: 'imitation' | 'rl' | 'batched' (one of the lock-step drivers on the device) or
        'sequential' (the reference's loop)."""
        env, policy, target = self.env, self.robot.policy, self.target_policy
        if not hasattr(env, 'engine_config'):  # not this package's env
            return 'sequential'
        orca, value_net = is_device_orca(policy), isinstance(policy, SARL)
        if (value_net or isinstance(target, SARL)) and update_memory and self._scenario_of(phase)[1] == 'mixed':
            # Acting under the mixed rule works (the kernels mask an episode's absent humans); FILLING A REPLAY MEMORY does
            # not: the states would hold a different number of humans per episode, which the reference cannot batch either
            # (its DataLoader stacks them; train.config keeps train_val_sim = circle_crossing).
            raise NotImplementedError('replay states under the mixed rule are ragged (a different number of humans per '
                                      'episode): train on circle_crossing / square_crossing as the reference does')
        start = env.case_counter[phase]
        if not (start >= 0 and start + k <= env.case_size[phase]):  # the k episodes would wrap the phase's case table
            return 'sequential'
        if not update_memory:
            return 'batched' if orca or (value_net and phase != 'train') else 'sequential'
        if (orca and imitation_learning and isinstance(target, SARL)
                and getattr(target, 'kinematics', 'holonomic') == 'holonomic'):
            return 'imitation'
        if value_net and phase == 'train' and not imitation_learning and getattr(policy, 'env', None) is env:
            return 'rl'
        return 'sequential'

    def _run_sequential(self, k, phase, update_memory, imitation_learning):
        success_times, collision_times, timeout_times = [], [], []
        too_close, min_dist, cumulative_rewards = 0, [], []
        collision_cases, timeout_cases = [], []
        for i in range(k):
            ob = self.env.reset(phase)
            done = False
            states, actions, rewards = [], [], []
            while not done:
                action = self.robot.act(ob)
                ob, reward, done, info = self.env.step(action)
                states.append(self.robot.policy.last_state)
                actions.append(action)
                rewards.append(reward)
                if isinstance(info, Danger):
                    too_close += 1
                    min_dist.append(info.min_dist)
            if isinstance(info, ReachGoal):
                success_times.append(self.env.global_time)
            elif isinstance(info, Collision):
                collision_cases.append(i)
                collision_times.append(self.env.global_time)
            elif isinstance(info, Timeout):
                timeout_cases.append(i)
                timeout_times.append(self.env.time_limit)
            else:
                raise ValueError('Invalid end signal from environment')
            if update_memory and isinstance(info, (ReachGoal, Collision)):
                self.update_memory(states, actions, rewards, imitation_learning)
            cumulative_rewards.append(sum([pow(self.gamma, t * self.robot.time_step * self.robot.v_pref) * reward
                                           for t, reward in enumerate(rewards)]))
        return (success_times, collision_times, timeout_times, collision_cases, timeout_cases, too_close,
                average(min_dist), cumulative_rewards)

    # ------------------------------------------------------------------ the lock-step drivers
    def _begin_phase(self, phase, value_policy=None):
        """What every batched driver starts with: the time step handed on as CrowdSim.reset does (crowd_sim.py:296-298), the
        value network's action space where one decides or transforms, and the phase's scenario and case numbers.  Episode i
        of the call is case start + i of the phase (no wrap: _route), whose seed is offset + start + i."""
        env = self.env
        self.robot.time_step = env.time_step
        self.robot.policy.time_step = env.time_step
        if value_policy is not None and value_policy.action_space is None:
            value_policy.build_action_space(self.robot.v_pref)
        human_num, rule, offset = self._scenario_of(phase)
        dt = env.time_step
        return human_num, rule, offset, env.case_counter[phase], env.case_size[phase], dt, int(round(env.time_limit / dt)) + 2

    def _end_phase(self, phase, start, size, k):
        self.env.case_counter[phase] = (start + k) % size

    def _run_batched(self, k, phase):
        env, policy = self.env, self.robot.policy
        orca = is_device_orca(policy)
        human_num, rule, offset, start, size, _, max_steps = self._begin_phase(phase, None if orca else policy)
        network_route = None  # value-network policies: the kernel family that took the decisions (sarl_network_route)
        B = int(min(k, self.max_envs))
        per_env = (k + B - 1) // B
        names = ('ep_outcome', 'ep_steps', 'ep_return', 'ep_time', 'ep_danger', 'ep_danger_dmin_sum')
        traces = []
        if orca:
            eng = BatchedCrowdSim(**env.engine_config(B, human_num, rule, _lib.ROBOT_ORCA))
            eng.set_gamma(self.gamma)
            self._share_robot_sim(eng, human_num, rule, offset + start)
            # (no job-wide counter, no in-kernel statistics: the records are read once below, as explorer.py:50-90 does)
            bufs = eng.rollout_begin(seed_base=offset + start, seed_mod=size, episode_limit=k, record_capacity=per_env,
                                     per_env_transitions=True)
            while True:
                if self.keep_trajectories:  # rows go to the host call by call: the device holds one call's trace at a time
                    tr = eng.rollout_trace(max_steps)
                    traces.append({n: v.cpu().numpy() for n, v in tr.items()})
                    del tr
                else:
                    eng.rollout(max_steps)
                if int(bufs['active'].sum().item()) == 0:
                    break
            rec = {n: bufs[n].cpu().numpy() for n in names}
        else:  # SARL value network: select + step + masked reset per batched step
            eng = BatchedCrowdSim(**env.engine_config(B, human_num, rule, _lib.ROBOT_EXTERNAL))
            policy.configure_engine(eng)
            network_route = eng.sarl_network_route()
            eng.sarl_set_weights(policy.model.state_dict())
            ro = SarlRollout(eng, self.gamma, seed_base=offset + start, seed_mod=size, episode_limit=k,
                             record_capacity=per_env)
            while ro.any_active():
                ro.run(8)
            rec = {n: ro.rec[m].cpu().numpy() for n, m in zip(names, ('outcome', 'steps', 'ret', 'time', 'danger', 'dsum'))}
        self._end_phase(phase, start, size, k)
        # episode id c = b + j*B  ->  record [b, j]
        order = [(c % B, c // B) for c in range(k)]
        outcome = [int(rec['ep_outcome'][b, j]) for b, j in order]
        times = [float(rec['ep_time'][b, j]) for b, j in order]
        returns = [float(rec['ep_return'][b, j]) for b, j in order]
        self.last_batch = dict(outcome=outcome, nav_time=times, discounted_return=returns,
                               steps=[int(rec['ep_steps'][b, j]) for b, j in order], network_route=network_route)
        if traces:  # global episode id c of the rollout = case c of this call
            per_episode = trace_episodes(traces)
            self.last_batch['trajectories'] = [per_episode[c]['state8'] for c in range(k)]
        return episode_statistics(outcome, times, returns, [int(rec['ep_danger'][b, j]) for b, j in order],
                                  [float(rec['ep_danger_dmin_sum'][b, j]) for b, j in order])  # a timeout's time: as recorded

    def _run_batched_imitation(self, k, phase):
        """Imitation-learning data collection (train.py:115-129): k ORCA-robot episodes in lock step on the device,
        then update_memory(..., imitation_learning=True) for all of them at once.  Per step cn_sarl_transform writes
        the target policy's transform of the joint state the ORCA robot saw (explorer.py:99:
        target_policy.transform(state), humans in env order) straight into a [B, T, H, D] trajectory tensor; values
        are the discounted Monte-Carlo returns of explorer.py:100-105 (host float64, the reference's left-to-right
        sum); (state, value) pairs enter the memory in the reference's order."""
        env, policy = self.env, self.target_policy
        human_num, rule, offset, start, size, dt, max_steps = self._begin_phase(phase, policy)
        vp = self.robot.v_pref
        D = policy.input_dim()
        single = policy.net_cfg.get('model') == 'cadrl'  # CADRL.transform (cadrl.py:174-185): one human, [13]
        outcome, length, rewards_all, danger_n, danger_sum = [], [], [], [], []
        for c0 in range(0, k, self.max_envs):
            B = min(self.max_envs, k - c0)
            eng = BatchedCrowdSim(**env.engine_config(B, human_num, rule, _lib.ROBOT_ORCA))
            eng.sarl_configure(**policy.engine_kwargs())  # only the transform runs on this engine
            self._share_robot_sim(eng, human_num, rule, offset + start)
            eng.reset(offset + start + c0 + np.arange(B))
            traj = torch.zeros(B, max_steps, human_num, D, dtype=torch.float32, device=eng.device)
            hist_r, hist_i, hist_d = [], [], []
            alive = torch.ones(B, dtype=torch.bool, device=eng.device)
            for t in range(max_steps):
                eng.sarl_transform(out=traj[:, t], env_stride=max_steps * human_num * D, sort_humans=False)
                out = eng.step(None, update=True, want_obs=False)
                hist_r.append(out['reward'])
                hist_i.append(out['info'])
                hist_d.append(out['dmin'])
                alive = alive & (out['done'] == 0)
                if t % 8 == 7 and not bool(alive.any().item()):
                    break
            R = torch.stack(hist_r).cpu().numpy()      # [T, B]
            steps, last, dn, ds, keep = episodes_of_histories(torch.stack(hist_i).cpu().numpy(), torch.stack(hist_d).cpu().numpy())
            outcome += [int(o) for o in last]
            length += [int(n) for n in steps]
            rewards_all += [R[:n, b].tolist() for b, n in enumerate(steps)]
            danger_n += dn
            danger_sum += ds
            # explorer.py:66-69, 92-125 for every ReachGoal / Collision episode of this batch
            if len(keep):
                if self.memory is None or self.gamma is None:
                    raise ValueError('Memory or gamma value is not set!')
                b_idx = np.repeat(keep, steps[keep])
                i_idx = np.concatenate([np.arange(steps[b]) for b in keep])
                x = traj[torch.as_tensor(b_idx, device=eng.device), torch.as_tensor(i_idx, device=eng.device)]
                values = []
                for b in keep:
                    rw = rewards_all[c0 + int(b)]
                    for i in range(len(rw)):
                        values.append(sum([pow(self.gamma, max(t - i, 0) * dt * vp) * r * (1 if t >= i else 0)
                                           for t, r in enumerate(rw)]))
                self._push_all(x[:, 0] if single else x, torch.Tensor(values))
        self._end_phase(phase, start, size, k)
        self.last_batch = dict(outcome=outcome, steps=length, env_steps=int(sum(length)))
        returns = [sum([pow(self.gamma, t * dt * vp) * r for t, r in enumerate(rw)]) for rw in rewards_all]
        return episode_statistics(outcome, [n * dt for n in length], returns, danger_n, danger_sum, env.time_limit)

    def _share_robot_sim(self, eng, human_num, rule, first_seed):
        """One persistent ORCA policy object = one captured rvo2 simulator (orca.py:95-110): every env of a batched run
        sees the radii the policy captured at its first episode — this call's first episode if it has none yet."""
        env = self.env
        if not (env.randomize_attributes and is_device_orca(self.robot.policy)):
            return  # constant radii: every capture is the same
        cap = getattr(self.robot.policy, '_rsim', None)
        if cap is None or len(cap[0]) != human_num + 1:
            one = BatchedCrowdSim(**env.engine_config(1, human_num, rule, _lib.ROBOT_ORCA))
            one.reset([first_seed])
            cap = env.robot_sim_capture(one.get_state()[0].cpu().numpy()[0, :, 6].tolist())
        eng.set_robot_sim(*cap)

    def _scenario_of(self, phase):
        env = self.env
        multi = getattr(self.robot.policy, 'multiagent_training', None)
        if phase == 'test':
            human_num, rule = env.human_num, env.test_sim
        else:  # crowd_sim.py:266-267, 277-279
            human_num, rule = (env.human_num if multi else 1), ('circle_crossing' if not multi else env.train_val_sim)
        offset = {'train': env.case_capacity['val'] + env.case_capacity['test'], 'val': 0,
                  'test': env.case_capacity['val']}[phase]
        return human_num, rule, offset

    def _push_all(self, states, values):
        """(state, value) pairs into the replay memory in the given order (explorer.py:125)."""
        if hasattr(self.memory, 'push_batch'):
            self.memory.push_batch(states, values)
        else:
            states, values = states.to(self.device), values.to(self.device)
            for j in range(states.shape[0]):
                self.memory.push((states[j], values[j].reshape(1)))

    def _run_batched_rl(self, k, phase):
        """RL-phase sampling (train.py:147-157: run_k_episodes(sample_episodes, 'train', update_memory=True)) with the
        epsilon-greedy value-network robot (SARL, CADRL or LSTM-RL), k episodes in lock step on the device.  Per
        batched step:
        cn_sarl_select (greedy action of every env) -> cn_sarl_explore (the epsilon branch of
        multi_human_rl.py:28-31 on each env's own numpy stream, continued after its scenario draws) ->
        cn_sarl_transform (policy.last_state, written straight into the trajectory tensor) -> cn_step.  Then
        update_memory (explorer.py:92-125) for all ReachGoal / Collision episodes at once (_push_td_rows).
        The laps of a batch: RlSampler.prepare, RlSampler.run_steps, read-back + _push_td_rows, the host's statistics."""
        env, policy = self.env, self.robot.policy
        if self.memory is None or self.gamma is None:
            raise ValueError('Memory or gamma value is not set!')
        if policy.epsilon is None:
            raise AttributeError('Epsilon attribute has to be set in training phase')
        human_num, rule, offset, start, size, dt, max_steps = self._begin_phase(phase, policy)
        vp = self.robot.v_pref
        gamma_bar = pow(self.gamma, dt * vp)
        D = policy.input_dim()
        single = policy.net_cfg.get('model') == 'cadrl'      # CADRL.transform: one human, [13]
        outcome, length, returns, danger_n, danger_sum, actions_taken = [], [], [], [], [], []
        n_steps = 0
        for c0 in range(0, k, self.max_envs):
            B = min(self.max_envs, k - c0)
            prof = self.rl_profile
            lap = _laps(prof)
            eng, h = self.rl.prepare(env, self.robot, B, human_num, rule, offset + start + c0, max_steps, D, lap)
            T = self.rl.run_steps(eng, h, float(policy.epsilon), lap)
            if prof is not None:
                prof['n_steps_issued'] = prof.get('n_steps_issued', 0) + T
            host = h.host_bytes()
            lap('  (histories to the host)')
            R, Dm, Ac, I = h.rows(host, T)
            I[I == UNWRITTEN] = _lib.NOTHING   # (rows behind an env's last step on the two-launch route)
            steps, last, keep = episode_ends(I)
            if ((Ac == -2) & (np.arange(T)[:, None] < steps[None, :])).any():   # greedy branch without a finite value
                raise ValueError('Value network is not well trained. ')         # multi_human_rl.py:57-58
            n_steps += int(steps.sum())
            if len(keep):
                self._push_td_rows(eng, h, R, steps, keep, single, gamma_bar, lap)
            lap('read-back + TD targets + push')
            for b in range(B):
                n = int(steps[b])
                outcome.append(int(last[b]))
                length.append(n)
                actions_taken.append(Ac[:n, b].tolist())
                returns.append(sum([pow(self.gamma, t * dt * vp) * r_ for t, r_ in enumerate(R[:n, b].tolist())]))
            dn, ds = danger_sums(I, Dm, steps)
            danger_n += dn
            danger_sum += ds
        self._end_phase(phase, start, size, k)
        times = [n * dt for n in length]
        self.last_batch = dict(outcome=outcome, steps=length, discounted_return=returns, nav_time=times, env_steps=n_steps,
                               actions=actions_taken)
        return episode_statistics(outcome, times, returns, danger_n, danger_sum, env.time_limit)

    def _push_td_rows(self, eng, h, R, steps, keep, single, gamma_bar, lap):
        """The kept episodes' (state, TD target) pairs into the memory: the targets r + gamma^(dt v_pref) * target_model(next
        state) come from ONE batched forward of the target network, the last step's is its reward.
        Rows in push order: episode by episode, step by step.  An episode's rows are slices of the histories (no index tensors
        to upload, no gathers): states [0, n), next states [1, n] — row n only feeds the value that the last step replaces by
        its reward."""
        traj, rew, pin, max_steps = h.traj, h.rew, h.pin, h.shape[0]
        ns = [int(steps[b]) for b in keep]
        if max(ns) < max_steps:
            cat = lambda parts: parts[0] if len(parts) == 1 else torch.cat(parts)  # noqa: E731
            states = cat([traj[b, :n_] for b, n_ in zip(keep, ns)])               # [N, H, D]
            nxt = cat([traj[b, 1:n_ + 1] for b, n_ in zip(keep, ns)])
            r = cat([rew[:n_, b] for b, n_ in zip(keep, ns)])
            ends = np.cumsum(ns) - 1                                              # the last step of every episode
            if pin:  # (a slice of the pinned history: goes up behind the steps, asynchronously)
                r = r.to(eng.device, non_blocking=True)
        else:  # (an episode as long as the histories: its row n does not exist)
            b_idx = np.repeat(keep, steps[keep])
            i_idx = np.concatenate([np.arange(steps[b]) for b in keep])
            bt = torch.as_tensor(b_idx, device=eng.device)
            it = torch.as_tensor(i_idx, device=eng.device)
            states, nxt = traj[bt, it], traj[bt, torch.clamp(it + 1, max=max_steps - 1)]
            r = torch.from_numpy(R[i_idx, b_idx]).to(eng.device) if pin else rew[it, bt]
            ends = np.flatnonzero(i_idx == steps[b_idx] - 1)
        if single:
            states, nxt = states[:, 0], nxt[:, 0]
        lap('  (rows of the episode)')
        with torch.no_grad():
            v_next = self._td_values(nxt).to(eng.device)
            lap('  (target network)')
            values = torch.add(r, v_next.double(), alpha=gamma_bar)   # float64, as the reference's Python floats
            if len(ends) == 1:
                values[-1:].copy_(r[-1:])
            else:
                e_idx = torch.as_tensor(ends, device=eng.device)
                values[e_idx] = r[e_idx]
        self._push_all(states, values.float())

    def _report(self, k, phase, episode, print_failure, success_times, collision_times, timeout_times,
                collision_cases, timeout_cases, too_close, avg_min_dist, cumulative_rewards):
        success, collision, timeout = len(success_times), len(collision_times), len(timeout_times)
        success_rate = success / k
        collision_rate = collision / k
        assert success + collision + timeout == k
        avg_nav_time = sum(success_times) / len(success_times) if success_times else self.env.time_limit
        extra_info = '' if episode is None else 'in episode {} '.format(episode)
        logging.info('{:<5} {}has success rate: {:.2f}, collision rate: {:.2f}, nav time: {:.2f}, total reward: {:.4f}'.
                     format(phase.upper(), extra_info, success_rate, collision_rate, avg_nav_time,
                            average(cumulative_rewards)))
        if phase in ['val', 'test']:
            num_step = sum(success_times + collision_times + timeout_times) / self.robot.time_step
            logging.info('Frequency of being in danger: %.2f and average min separate distance in danger: %.2f',
                         too_close / num_step, avg_min_dist)
        if print_failure:
            logging.info('Collision cases: ' + ' '.join([str(x) for x in collision_cases]))
            logging.info('Timeout cases: ' + ' '.join([str(x) for x in timeout_cases]))
        self.last_stats = dict(success_rate=success_rate, collision_rate=collision_rate, nav_time=avg_nav_time,
                               total_reward=average(cumulative_rewards), too_close=too_close,
                               collision_cases=collision_cases, timeout_cases=timeout_cases)

    # ------------------------------------------------------------------ explorer.py:92-125
    def update_memory(self, states, actions, rewards, imitation_learning=False):
        """(state, value) pairs of one episode into the replay memory (explorer.py:92-125).  The TD targets of the RL
        branch need the target network's value of every next state: they are evaluated in ONE batched forward instead of
        one per step."""
        if self.memory is None or self.gamma is None:
            raise ValueError('Memory or gamma value is not set!')
        dt_vp = self.robot.time_step * self.robot.v_pref
        next_values = None
        if not imitation_learning and len(states) > 1:
            with torch.no_grad():
                next_values = self.target_model(torch.stack(list(states[1:]))).reshape(-1).tolist()
        for i, state in enumerate(states):
            reward = rewards[i]
            if imitation_learning:
                state = self.target_policy.transform(state)
                value = sum([pow(self.gamma, max(t - i, 0) * dt_vp) * reward * (1 if t >= i else 0)
                             for t, reward in enumerate(rewards)])
            elif i == len(states) - 1:
                value = reward  # terminal state
            else:
                value = reward + pow(self.gamma, dt_vp) * next_values[i]
            self.memory.push((state, torch.Tensor([value]).to(self.device)))
