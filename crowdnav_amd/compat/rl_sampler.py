"""What the RL sampling phase keeps between Explorer.run_k_episodes calls (train.py calls it once per training episode: 10 000
times in the shipped schedule) — the engine, the policy's parameter table, the pinned seed buffers, the histories — and the two
laps of a call that only need those: prepare (engine, weights, seeds, histories) and the step stream."""
import os

import numpy as np
import torch

from .. import _lib
from ..engine import BatchedCrowdSim
from .td_targets import ParamTable

UNWRITTEN = 255  # info code of a history row that no kernel has written in this call


class Histories(object):
    """One engine's per-step rows.  They live as long as the engine (one allocation + fill per shape, not five per sampled
    episode); every row that is read has been written by the call's own steps, except traj's row T, which only feeds a value
    that the last step's reward replaces (stale rows are finite).
    A few envs (the two-launch route of cn_sarl_sample_step: train.py samples ONE episode per call): ALL four histories live in
    pinned host memory — the kernels only write them, a step's reward / min distance / action before its info code — so that
    the host reads an episode's rows the moment its end code has arrived: no copy back, no wait for the steps issued past the
    end, and the TD targets, the push and the host's statistics overlap."""

    def __init__(self, key, eng, B, max_steps, human_num, D, pin):
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=eng.device)  # noqa: E731
        self.key, self.pin, self.shape = key, pin, (max_steps, B)
        # reward / min-distance / action histories are three regions of ONE byte buffer: one blocking copy brings all of them
        # to the host (one each was a tenth of a millisecond per sampled episode)
        n = max_steps * B
        self.packed = torch.zeros((20 * n,), dtype=torch.uint8).pin_memory() if pin else z((20 * n,), torch.uint8)
        self.rew = self.packed[:8 * n].view(torch.float64).view(max_steps, B)
        self.dmin = self.packed[8 * n:16 * n].view(torch.float64).view(max_steps, B)
        self.act = self.packed[16 * n:20 * n].view(torch.int32).view(max_steps, B)
        # the info codes go to PINNED host memory: the kernels only write them, and the host watches the episode ends arrive
        # while it keeps issuing steps — no device synchronisation inside an episode (a check every 8 steps was a bubble of
        # ~40 us each time and 3.5 wasted steps per episode on average)
        self.info = torch.empty((max_steps, B), dtype=torch.uint8).pin_memory()
        self.info_np = self.info.numpy()
        self.traj = z((B, max_steps, human_num, D), torch.float32)
        self.alive, self.done, self.action = z((B,), torch.uint8), z((B,), torch.uint8), z((B, 2), torch.float64)

    def host_bytes(self):
        return (self.packed if self.pin else self.packed.cpu()).numpy()

    def rows(self, host, T):
        """reward, min distance, action [T, B] as views of host_bytes(), and a copy of the info codes as they are now."""
        (max_steps, B), n = self.shape, self.shape[0] * self.shape[1]
        return (host[:8 * n].view(np.float64).reshape(max_steps, B)[:T], host[8 * n:16 * n].view(np.float64).reshape(max_steps, B)[:T],
                host[16 * n:20 * n].view(np.int32).reshape(max_steps, B)[:T], self.info_np[:T].copy())


class RlSampler(object):
    def __init__(self):
        self.eng = None        # the batched engine of the sampling phase ...
        self.config = None     # ... the keyword arguments it was built from (env.engine_config) ...
        self._key = None       # ... the full key it is cached under, and the action-space list that key names by identity
        self._space = None     # (held, so that its id cannot be recycled)
        self._quick = None     # (fast key, env.config): what engine_config reads, without building its dict
        self.params = ParamTable()  # of the policy's model
        self._seeds = (None, None, None)  # (key, pinned int32 [B], device int32 [B])
        self.hist = None       # Histories of the last call's shape

    def engine(self, env, robot, B, human_num, rule):
        """The batched engine of the RL sampling phase, kept between calls."""
        policy = robot.policy
        # fast path: everything engine_config reads, by value or (the config object, the policy, its action-space list) by
        # identity — the dict below with its two configparser reads and its sort was 0.03 ms of a sampled episode, 0.1 ms behind
        # the schedule's SGD batches when the interpreter's own data is cold
        quick = (B, human_num, rule, env.time_step, env.time_limit, env.success_reward, env.collision_penalty, env.discomfort_dist,
                 env.discomfort_penalty_factor, robot.visible, getattr(policy, 'safety_space', 0), env.circle_radius,
                 env.square_width, robot.radius, robot.v_pref, env.randomize_attributes, env.device,
                 getattr(robot, 'kinematics', 'holonomic'), id(env.config), id(policy), id(policy.action_space))
        if self._quick is not None and self._quick[0] == quick and self.eng is not None:
            return self.eng
        cfg = env.engine_config(B, human_num, rule, _lib.ROBOT_EXTERNAL)
        # (the action table by the identity of the policy's action_space list — rebuilt tables are new lists; the sampler holds
        # the list, so its id cannot be recycled — instead of 81 tuples converted and hashed per sampled episode)
        key = (tuple(sorted(cfg.items())), id(policy), id(policy.action_space))
        if self.eng is None or self._key != key:
            eng = BatchedCrowdSim(**cfg)
            policy.configure_engine(eng)
            self.eng, self.config, self._key, self._space = eng, cfg, key, policy.action_space
        self._quick = (quick, env.config)  # (holds the config object: its id cannot be recycled)
        return self.eng

    def prepare(self, env, robot, B, human_num, rule, first_seed, max_steps, D, lap):
        """Engine, the policy's weights, the scenarios of seeds first_seed + [0, B), histories ready for step 0."""
        eng = self.engine(env, robot, B, human_num, rule)
        weights = self.params.of(robot.policy.model).by_name
        lap('  (engine lookup)')
        eng.sarl_set_weights(weights)
        lap('  (weight re-pack)')
        # the seeds go up from a pinned buffer behind the weight re-pack, without a synchronisation (engine.reset waits
        # for the scenarios: ~0.1 ms per sampled episode of device idle time in front of the first step)
        skey = (id(eng), B)
        if self._seeds[0] != skey:
            self._seeds = (skey, torch.empty(B, dtype=torch.int32).pin_memory(), torch.empty(B, dtype=torch.int32, device=eng.device))
        _, seeds_host, seeds_dev = self._seeds
        seeds_host.numpy()[:] = (first_seed + np.arange(B)).astype(np.uint32).view(np.int32)
        with torch.cuda.stream(eng._stream):
            seeds_dev.copy_(seeds_host, non_blocking=True)
        eng.reset_async(seeds_dev, None)
        lap('  (seeds + reset)')
        pin = B <= 8 and os.environ.get('CROWDNAV_AMD_RL_PINNED', '1') != '0'
        hkey = (id(eng), B, max_steps, human_num, D, pin)
        if self.hist is None or self.hist.key != hkey:
            self.hist = Histories(hkey, eng, B, max_steps, human_num, D, pin)
        h = self.hist
        h.alive.fill_(1)
        h.done.zero_()
        h.info_np.fill(UNWRITTEN)
        lap('weights + reset')
        return eng, h

    @staticmethod
    def run_steps(eng, h, eps, lap):
        """Issues the steps of one lock-step batch and watches the end codes arrive; returns the number of steps issued.
        Per step: ONE library call (cn_sarl_sample_step: two launches at one env) and no torch kernel — every result lands in
        its row of the histories, and an env leaves `alive` at the start of the step after its episode ended.  The host runs at
        most `ahead` steps in front of the device (the rows of info it has seen arrive tell it where the device is) and stops
        issuing once every env's episode-end code is there; the steps already issued for an env that has finished are skipped
        by the kernels (two-launch route) or step a retired env (general route)."""
        max_steps, B = h.shape
        inf_np = h.info_np
        step = eng.sarl_sampler(h.traj, h.rew, h.info, h.dmin, h.act, h.alive, h.done, h.action)
        fused_before = eng.launch_counts()['sarl_decide_steps']
        ahead, seen, spins = int(os.environ.get('CROWDNAV_AMD_RL_AHEAD', '2')), 0, 0
        finished = np.zeros(B, dtype=bool)
        T = 0
        for t in range(max_steps):
            step(t, eps)
            T = t + 1
            while seen < T:  # rows the device has completed: every env that still samples has written its code
                row = inf_np[seen]
                if ((row != UNWRITTEN) | finished).all():
                    finished |= (row != UNWRITTEN) & (row >= _lib.REACH_GOAL)
                    seen += 1
                    spins = 0
                elif T - seen > ahead and spins < 20000000:
                    spins += 1   # (bounded: a device error surfaces at eng.sync() below instead of hanging here)
                else:
                    break
            if finished.all():
                break
        # pinned histories are complete up to every env's end code once that code is there — provided the steps ran the
        # two-launch route (its last kernel writes a step's outputs in that order; launch counters: host-side, no device
        # work); anything else waits for the device as before
        fused_steps = eng.launch_counts()['sarl_decide_steps'] - fused_before
        if not (h.pin and fused_steps == T and finished.all()):
            eng.sync()
        lap('steps')
        return T
