"""BatchedCrowdSim — tensor-level host API over the C ABI (B independent CrowdSim envs on one GPU).

Mirrors, batched over B envs, the reference calls
    CrowdSim.configure / reset / step / onestep_lookahead   crowd_sim/envs/crowd_sim.py:51-79, 251-420
    ORCA.predict for every agent                            crowd_sim/envs/policy/orca.py:82-132
    Explorer.run_k_episodes' episode loop                   crowd_nav/utils/explorer.py:35-72
torch is used for device memory and streams only; all compute happens in libcrowdnav_amd.so.
Agent 0 of every env is the robot, agents 1..H the humans.
"""
import ctypes as C
import weakref

import numpy as np
import torch

from . import _lib
from ._lib import CnConfig, CnLookaheadOut, CnRolloutIo, CnTraceOut, check

# shipped defaults of crowd_nav/configs/env.config + the hard-coded ORCA constants (orca.py:60-66)
_DEFAULTS = dict(
    num_envs=1, num_humans=5, time_step=0.25, time_limit=25.0, success_reward=1.0,
    collision_penalty=-0.25, discomfort_dist=0.2, discomfort_penalty_factor=0.5, robot_visible=0,
    robot_policy=_lib.ROBOT_ORCA, robot_safety_space=0.0, human_safety_space=0.0, neighbor_dist=10.0,
    max_neighbors=10, scenario_rule=_lib.CIRCLE_CROSSING, time_horizon=5.0, time_horizon_obst=5.0,
    circle_radius=4.0, square_width=10.0, human_radius=0.3, human_v_pref=1.0, robot_radius=0.3,
    robot_v_pref=1.0, randomize_attributes=0, device=0, robot_kinematics=_lib.HOLONOMIC, flags=0)


def default_config(**overrides):
    d = dict(_DEFAULTS)
    unknown = set(overrides) - set(d)
    if unknown:
        raise TypeError('unknown config keys: %s' % sorted(unknown))
    d.update(overrides)
    return d


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _struct(cls, tensors, **fields):
    """A ctypes struct of device pointers: every field of cls that `tensors` names holds that tensor's address, the other
    pointers stay NULL; **fields are set as given."""
    return cls(**{k: tensors[k].data_ptr() for k, _ in cls._fields_ if k in tensors}, **fields)


# the state_dict names of each value network, in the order sarl_set_weights hands the parameters over
SARL_PARAM_ORDER = tuple('%s.%d.%s' % (m, i, p) for m, idxs in (('mlp1', (0, 2)), ('mlp2', (0, 2)),
                                                               ('attention', (0, 2, 4)), ('mlp3', (0, 2, 4, 6)))
                         for i in idxs for p in ('weight', 'bias'))


LSTM_PARAM_ORDER = tuple('mlp.%d.%s' % (i, p) for i in (0, 2, 4, 6) for p in ('weight', 'bias')) + (
    'lstm.weight_ih_l0', 'lstm.weight_hh_l0', 'lstm.bias_ih_l0', 'lstm.bias_hh_l0')
LSTM_PAIRWISE_MLP1_ORDER = tuple('mlp1.%d.%s' % (i, p) for i in (0, 2, 4, 6) for p in ('weight', 'bias'))
CADRL_PARAM_ORDER = tuple('value_network.%d.%s' % (i, p) for i in (0, 2, 4, 6) for p in ('weight', 'bias'))


class Plan(object):
    """What BatchedCrowdSim.plan_begin returns: the device tensors of a CEM planner (struct cn_plan) and its settings (struct
    cn_plan_cfg).  The tensors are the caller's to read and write between calls; they live as long as the object."""

    def __init__(self, eng, K, n, elites, iterations, init_std, min_std, smoothing, seed, bootstrap, sort_humans):
        B, dev = eng.B, eng.device
        self.engine = weakref.ref(eng)
        self.K, self.n, self.elites, self.iterations, self.bootstrap = K, n, elites, iterations, bootstrap
        f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)  # noqa: E731
        self.mean, self.std, self.best_actions = f64(B, n, 2), f64(B, n, 2).fill_(init_std), f64(B, n, 2)
        self.best_score, self.action, self.candidates = f64(B), f64(B, 2), f64(B, K, n, 2)
        self.order = torch.zeros((B, K), dtype=torch.int32, device=dev)
        self.look = dict(ret=f64(B, K), info=torch.zeros((B, K), dtype=torch.uint8, device=dev),
                         steps=torch.zeros((B, K), dtype=torch.int32, device=dev), time=f64(B, K))
        if bootstrap:
            self.look.update(final_state8=f64(B, K, eng.A, 8), final_theta=f64(B, K),
                             value=torch.zeros((B, K), dtype=torch.float32, device=dev), score=f64(B, K))
        self.cfg = _lib.CnPlanCfg(n_steps=n, n_candidates=K, n_elites=elites, iterations=iterations, bootstrap=int(bootstrap),
                                  sort_humans=int(sort_humans), init_std=init_std, min_std=min_std, smoothing=smoothing,
                                  seed=seed & 0xffffffffffffffff)
        # value and score (bootstrap only) are lookahead rows in Python and fields of cn_plan itself in C
        self.c = _struct(_lib.CnPlan, dict(self._own(), **self.look), look=_struct(CnLookaheadOut, self.look))

    def _own(self):
        return {k: getattr(self, k) for k in ('mean', 'std', 'best_actions', 'best_score', 'action', 'candidates', 'order')}

    def tensors(self):
        """Every tensor of the plan by name (the lookahead rows as look.<name>)."""
        out = self._own()
        out.update({'look.' + k: v for k, v in self.look.items()})
        return out


def _predict_models(who, models):
    """(CN_PREDICT_* values, whether `models` was a single name) of a predictor argument: a name or a sequence of 1 ..
    MODES_MAX names, 'cv' standing for 'constant_velocity'.  Checked before the library is asked."""
    single = isinstance(models, str)
    names = [models] if single else list(models) if isinstance(models, (list, tuple)) else None
    if names is None or not 1 <= len(names) <= _lib.MODES_MAX:
        raise ValueError('%s: models must be a name or a sequence of 1 .. %d names, got %r' % (who, _lib.MODES_MAX, models))
    codes = []
    for name in names:
        name = _lib.PREDICT_ALIASES.get(name, name) if isinstance(name, str) else name
        if name not in _lib.PREDICT_MODELS:
            raise ValueError("%s: unknown predictor %r (one of %s, or 'cv')" % (who, name, _lib.PREDICT_MODELS))
        codes.append(_lib.PREDICT_MODELS.index(name))
    return codes, single


class Predictors(object):
    """What BatchedCrowdSim.plan_predict_begin returns: the device predictors of M futures for one Plan (struct cn_predictors).
    human_vel float64 [B, M, plan.n, H, 2] is the scratch table plan_predict_rollout fills before every planning step — after
    a call it holds the prediction the LAST planning step scored against; weights float64 [B, M] or None."""

    def __init__(self, eng, plan, codes, weights, reduce, risk_penalty):
        self.engine, self.plan = weakref.ref(eng), weakref.ref(plan)
        self.models = tuple(_lib.PREDICT_MODELS[c] for c in codes)
        M = len(codes)
        self.human_vel = torch.zeros((eng.B, M, plan.n, eng.H, 2), dtype=torch.float64, device=eng.device)
        self.weights = None if weights is None else torch.as_tensor(weights, dtype=torch.float64).to(eng.device).contiguous().clone()
        self.c = _lib.CnPredictors(n_modes=M, model=(C.c_int32 * 8)(*codes), reduce=_lib.MODES_REDUCE.index(reduce),
                                   risk_penalty=float(risk_penalty), human_vel=self.human_vel.data_ptr(),
                                   weight=None if self.weights is None else self.weights.data_ptr())


class BatchedCrowdSim(object):
    """B crowd-navigation envs resident in HBM.  All tensors returned live on the engine's device."""

    def __init__(self, **config):
        self.config = default_config(**config)
        self.B = int(self.config['num_envs'])
        self.H = int(self.config['num_humans'])
        self.A = self.H + 1
        self._lib = _lib.load()
        self._h = C.c_void_p()
        cfg = CnConfig(**self.config)
        check(self._lib.cn_create(C.byref(cfg), C.byref(self._h)))
        self.device = torch.device('cuda', int(self.config['device']))
        self._rollout = None
        self.use_current_stream()

    def close(self):
        if getattr(self, '_h', None) is not None and self._h.value:
            self._lib.cn_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass

    # ---------------------------------------------------------------- plumbing
    def use_current_stream(self):
        """Launch on torch's current HIP stream so torch ops and torch.cuda.Event order with the engine."""
        with torch.cuda.device(self.device):
            self._stream = torch.cuda.current_stream()
            check(self._lib.cn_set_stream(self._h, C.c_void_p(self._stream.cuda_stream)))

    def sync(self):
        check(self._lib.cn_sync(self._h))

    def _new(self, shape, dtype):
        return torch.empty(shape, dtype=dtype, device=self.device)

    def _borrow(self, x, dtype, shape):
        """x as the library reads it, and whether that is a temporary copy: a contiguous tensor of that dtype on the engine's
        device is read where it lies, anything else is copied there; None passes through.  A call that handed a temporary over
        ends with _release: torch may otherwise free the copy while a kernel still reads it."""
        if x is None:
            return None, False
        t = torch.as_tensor(x, dtype=dtype).to(self.device).contiguous()
        if tuple(t.shape) != tuple(shape):
            raise ValueError('expected shape %s, got %s' % (tuple(shape), tuple(t.shape)))
        return t, not (torch.is_tensor(x) and t.data_ptr() == x.data_ptr())

    def _release(self, *temporary):
        """Synchronise if any argument of the call just made was a temporary copy (the flags _borrow returned)."""
        if any(temporary):
            self.sync()

    def _dense(self, t, dtype, shape, pinned_ok=False):
        """Whether the library can take t by its address: a contiguous tensor of that dtype and shape on the engine's device
        (pinned_ok: or in pinned host memory)."""
        return (torch.is_tensor(t) and (t.device == self.device or (pinned_ok and t.device.type == 'cpu' and t.is_pinned()))
                and t.dtype == dtype and tuple(t.shape) == tuple(shape) and t.is_contiguous())

    def _rows(self, who, spec, out):
        """The output tensors of a call by name, spec: name -> (dtype, shape).  Fresh tensors, or the caller's `out` validated
        and restricted to the names of the spec."""
        if out is None:
            return {k: self._new(shape, dt) for k, (dt, shape) in spec.items()}
        for k, (dt, shape) in spec.items():
            if not self._dense(out.get(k), dt, shape):
                raise ValueError('%s: out[%r] must be a contiguous %s %s tensor on %s' % (who, k, dt, shape, self.device))
        return {k: out[k] for k in spec}

    def _roll(self):
        """(io, bufs) of the rollout in progress: what every rollout-bound method starts with."""
        if self._rollout is None:
            raise RuntimeError('call rollout_begin() first')
        return self._rollout

    # ---------------------------------------------------------------- state
    def set_state(self, state8=None, global_time=None):
        """state8: [B, A, 8] float64 (px,py,vx,vy,gx,gy,radius,v_pref); global_time: [B] float64."""
        s, _ = self._borrow(state8, torch.float64, (self.B, self.A, 8))
        g, _ = self._borrow(global_time, torch.float64, (self.B,))
        check(self._lib.cn_set_state(self._h, _ptr(s), _ptr(g)))
        self.sync()  # s/g may be temporaries

    def get_state(self):
        s = self._new((self.B, self.A, 8), torch.float64)
        g = self._new((self.B,), torch.float64)
        check(self._lib.cn_get_state(self._h, _ptr(s), _ptr(g)))
        return s, g

    def set_theta(self, theta):
        """Robot heading per env, [B] float64 (FullState.theta)."""
        t, _ = self._borrow(theta, torch.float64, (self.B,))
        check(self._lib.cn_set_theta(self._h, _ptr(t)))
        self.sync()

    def get_theta(self):
        t = self._new((self.B,), torch.float64)
        check(self._lib.cn_get_theta(self._h, _ptr(t)))
        return t

    def human_count(self):
        """len(env.humans) per env, [B] int32 (differs from num_humans only under the `mixed` rule)."""
        n = self._new((self.B,), torch.int32)
        check(self._lib.cn_get_human_count(self._h, _ptr(n)))
        return n

    def set_robot_sim(self, radii, max_speed):
        """Every env gets the same captured robot simulator: radii float32 [A] (radius + 0.01 + safety_space as the
        persistent ORCA policy first saw them), max_speed (cn_set_robot_sim)."""
        r = np.ascontiguousarray(radii, dtype=np.float32).reshape(self.A)
        check(self._lib.cn_set_robot_sim(self._h, r.ctypes.data_as(C.c_void_p), C.c_float(float(max_speed))))

    def drop_robot_sim(self):
        check(self._lib.cn_drop_robot_sim(self._h))

    def drop_sims(self):
        """Fresh rvo2 simulators for every agent (cn_drop_sims): the robot's captured radii and every simulator's kd-tree
        order are forgotten — after teleporting the agents with set_state, when freshly built policies are meant."""
        check(self._lib.cn_drop_sims(self._h))

    def reset(self, seeds, mask=None):
        """np.random.seed(seeds[b]) + scenario generation per env; returns the np.random.random() call counts."""
        host = seeds.cpu().numpy() if torch.is_tensor(seeds) else np.asarray(seeds)
        bits = np.ascontiguousarray(host.astype(np.uint32)).view(np.int32)  # torch has no uint32 arithmetic
        sd, _ = self._borrow(torch.from_numpy(bits), torch.int32, (self.B,))
        m, _ = self._borrow(mask, torch.uint8, (self.B,))
        draws = torch.zeros(self.B, dtype=torch.int64, device=self.device)
        check(self._lib.cn_reset(self._h, _ptr(sd), _ptr(m), _ptr(draws)))
        self.sync()
        return draws

    def reset_async(self, seeds_i32, mask_u8):
        """cn_reset with device-resident seeds (int32 bit patterns of the uint32 seeds) and mask; no sync."""
        check(self._lib.cn_reset(self._h, _ptr(seeds_i32), _ptr(mask_u8), None))

    # ---------------------------------------------------------------- one transition
    def orca(self):
        out = self._new((self.B, self.A, 2), torch.float32)
        check(self._lib.cn_orca(self._h, _ptr(out)))
        return out

    def step(self, action=None, update=True, want_obs=True):
        """CrowdSim.step for every env.  action: [B, 2] float64 or None when the robot is ORCA on device."""
        a, temporary = self._borrow(action, torch.float64, (self.B, 2))
        out = dict(
            reward=self._new((self.B,), torch.float64), done=self._new((self.B,), torch.uint8),
            info=self._new((self.B,), torch.uint8), dmin=self._new((self.B,), torch.float64),
            action=self._new((self.B, 2), torch.float64),
            orca_vel=self._new((self.B, self.A, 2), torch.float32),
            obs=self._new((self.B, self.H, 5), torch.float64) if want_obs else None)
        check(self._lib.cn_step(self._h, _ptr(a), int(bool(update)), _ptr(out['reward']), _ptr(out['done']),
                                _ptr(out['info']), _ptr(out['dmin']), _ptr(out['action']),
                                _ptr(out['orca_vel']), _ptr(out['obs'])))
        self._release(temporary)
        return out

    def step_into(self, action, reward, done, info, dmin, update=True):
        """CrowdSim.step for every env, results written into the caller's device tensors (reward / dmin float64 [B], done / info
        uint8 [B]; e.g. row t of a [T, B] history) — nothing allocated, no optional outputs: the per-step form of the RL
        sampling loop, where a dozen small torch kernels per step were as expensive as the step itself."""
        for t, dt in ((action, torch.float64), (reward, torch.float64), (dmin, torch.float64), (done, torch.uint8), (info, torch.uint8)):
            assert t.dtype == dt and t.is_contiguous() and t.device.type == self.device.type
        check(self._lib.cn_step(self._h, _ptr(action), int(bool(update)), _ptr(reward), _ptr(done), _ptr(info), _ptr(dmin),
                                None, None, None))

    # ---------------------------------------------------------------- fused rollouts
    def set_gamma(self, gamma):
        check(self._lib.cn_set_gamma(self._h, float(gamma)))

    def rollout_begin(self, seed_base, seed_mod, episode_limit=-1, record_capacity=8, env_offset=0,
                      env_stride=None, boundary_records=0, per_env_transitions=False):
        """Start Explorer-style episode bookkeeping: env b runs global episodes b, b+B, b+2B, ... (< limit),
        episode c seeded with seed_base + c % seed_mod.  A shard of a larger job passes its first global env
        id as env_offset and the global env count as env_stride.
        boundary_records = K > 0: every rollout launch also leaves the shard-boundary outputs itself (its last workgroup):
        bufs['summary'] float64 [8] (what records_summary() returns for this engine) and bufs['blocks'] float64
        [B, 1 + 6 K] (what rollout_records(K) returns) — no boundary kernels on a single GPU, only the all-gather on many.
        per_env_transitions (ABI v6): instead of the ONE job-wide counter bufs['transitions'] every launch adds up (arrival
        tickets between the workgroups at the end of every launch), each env counts its own transitions in
        bufs['env_transitions'] int64 [B] and a launch ends without any hand-off — with boundary_records = 0 the statistics are
        then computed once, when the caller asks (rollout_records + records_summary), as explorer.py:74-90 does."""
        B, K = self.B, int(record_capacity)
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=self.device)  # noqa: E731
        bufs = dict(
            ep_outcome=z((B, K), torch.uint8), ep_steps=z((B, K), torch.int32), ep_return=z((B, K), torch.float64),
            ep_time=z((B, K), torch.float64), ep_danger=z((B, K), torch.int32),
            ep_danger_dmin_sum=z((B, K), torch.float64),
            ep_count=z((B,), torch.int32), cur_steps=z((B,), torch.int32), cur_return=z((B,), torch.float64),
            cur_danger=z((B,), torch.int32), cur_danger_dmin_sum=z((B,), torch.float64),
            active=z((B,), torch.uint8))
        if per_env_transitions:
            bufs['env_transitions'] = z((B,), torch.int64)
        else:
            bufs['transitions'] = z((1,), torch.int64)
        Kb = int(boundary_records)
        if Kb > 0:
            bufs['summary'] = z((_lib.SUMMARY_FIELDS,), torch.float64)
            bufs['blocks'] = z((B, 1 + Kb * _lib.RECORD_FIELDS), torch.float64)
        io = CnRolloutIo(seed_base=int(seed_base), seed_mod=int(seed_mod), episode_limit=int(episode_limit),
                         env_offset=int(env_offset), env_stride=int(B if env_stride is None else env_stride),
                         record_capacity=K, blocks_records=Kb, **{k: v.data_ptr() for k, v in bufs.items()})
        # the previous rollout's buffers stay referenced until cn_rollout_begin has returned: with the asynchronous scenario
        # fill, kernels of the old rollout may still be reading them on the engine's side streams (the call waits for them)
        previous = self._rollout
        check(self._lib.cn_rollout_begin(self._h, C.byref(io)))
        self._rollout = (io, bufs)
        del previous
        return bufs

    def rollout(self, n_steps):
        """n_steps transitions per active env in one kernel launch (in-kernel auto-reset)."""
        io, bufs = self._roll()
        check(self._lib.cn_rollout(self._h, C.byref(io), int(n_steps)))
        return bufs

    def rollout_trace(self, n_steps, rewards=False, out=None):
        """rollout(n_steps) that also records every step (cn_rollout_trace): the same transitions, counters and records, plus a
        dict of device tensors whose row [b, t] belongs to the t-th step of THIS call —
            state8  float64 [B, n, A, 8]  the joint state BEFORE the transition (get_state()'s layout; env.states of the reference)
            episode int32   [B, n]        ordinal j of env b's episode (global id env_offset + b + j * env_stride);
                                          -1 where the env made no transition (retired, or waiting for a scenario)
            step    int32   [B, n]        index of the transition inside its episode (0 = from the reset state)
        and with rewards=True reward float64, info uint8, dmin float64 [B, n]: what step() returns for that transition.
        Where episode is -1 the other arrays are not written (fresh tensors hold whatever torch.empty left there).  The state
        after an episode's last transition is not recorded: the next row is the next episode's reset state.
        Size: 64 * A + 8 bytes per env-step, plus 17 with rewards (4096 envs x 5 humans x 1000 steps: 1.6 GB) — trace in
        chunks, or pass the previous call's dict as `out` to reuse it (validated; episode is refilled with -1).
        One launch of the generic phase kernel whatever the geometry: slower than rollout(), which it may be mixed with freely.
        crowdnav_amd.trace.episodes() splits the result into episodes on the host."""
        io, _ = self._roll()
        out = self._trace_out('rollout_trace', n_steps, rewards, out)
        if out['episode'].shape[1] == 0:  # a no-op, as rollout(0) is (empty tensors have no address to hand over)
            return out
        check(self._lib.cn_rollout_trace(self._h, C.byref(io), int(n_steps), C.byref(_struct(CnTraceOut, out))))
        return out

    def _trace_out(self, who, n_steps, rewards, out):
        """The dict of per-step rows a traced call of n_steps writes (rollout_trace, rollout_actions): fresh tensors, or the
        caller's `out` validated; episode filled with -1."""
        n = int(n_steps)
        if n < 0:
            raise ValueError('n_steps must be >= 0')
        spec = dict(state8=(torch.float64, (self.B, n, self.A, 8)), episode=(torch.int32, (self.B, n)),
                    step=(torch.int32, (self.B, n)))
        if rewards:
            spec.update(reward=(torch.float64, (self.B, n)), info=(torch.uint8, (self.B, n)), dmin=(torch.float64, (self.B, n)))
        out = self._rows(who, spec, out)
        out['episode'].fill_(-1)
        return out

    def rollout_step(self, action):
        """One bookkept transition of every running env with caller-supplied actions ([B, 2] float64 device tensor):
        the external-policy counterpart of rollout() (robot_policy == ROBOT_EXTERNAL)."""
        io, bufs = self._roll()
        a, temporary = self._borrow(action, torch.float64, (self.B, 2))
        check(self._lib.cn_rollout_step(self._h, C.byref(io), _ptr(a)))
        self._release(temporary)
        return bufs

    def rollout_actions(self, actions, trace=False, rewards=False, out=None):
        """n bookkept transitions of every running env with the actions known in advance, in ONE launch (cn_rollout_actions):
        what n rollout_step(actions[:, t]) calls do, bit for bit, and may be mixed with.  actions: [B, n, 2] float64 — (vx, vy),
        or (v, r) for a unicycle robot; row [b, t] is env b's action at step t of THIS call, ignored where the env is retired or
        waiting for a scenario.  A contiguous float64 tensor on the engine's device is read where it lies (keep it alive until
        the call has run); anything else is copied and the call synchronises, as rollout_step does.
        Returns the rollout's bufs; with trace=True the dict rollout_trace returns instead (state8 / episode / step, and with
        rewards=True reward / info / dmin, rows [b, t]; `out` reuses a previous call's dict) — one launch either way.
        crowdnav_amd.trace.episodes() cuts it into episodes."""
        io, bufs = self._roll()
        shape = tuple(getattr(actions, 'shape', np.shape(actions)))
        if len(shape) != 3 or shape[0] != self.B or shape[2] != 2:
            raise ValueError('rollout_actions: actions must be [%d, n, 2], got %s' % (self.B, shape))
        n = int(shape[1])
        rows = self._trace_out('rollout_actions', n, rewards, out) if trace else None
        if n > 0:
            a, temporary = self._borrow(actions, torch.float64, (self.B, n, 2))
            tr = None if rows is None else C.byref(_struct(CnTraceOut, rows))
            check(self._lib.cn_rollout_actions(self._h, C.byref(io), n, _ptr(a), tr))
            self._release(temporary)
        return rows if trace else bufs

    def lookahead(self, actions, final_state=False, out=None, bootstrap=False, sort_humans=False):
        """Score K candidate action sequences per env from the CURRENT state, in one launch, leaving the engine as it is
        (cn_lookahead_actions): the n-step, K-candidate form of step(update=False).  actions: [B, K, n, 2] float64 — (vx, vy), or
        (v, r) for a unicycle robot; branch (b, k) starts from env b as it stands, applies actions[b, k, t] as step() would
        and stops after the first transition with done, or after n.  A contiguous float64 tensor on the engine's device is read
        where it lies (keep it alive until the call has run); anything else is copied and the call synchronises.
        Returns a dict of device tensors, rows [b, k]:
            ret   float64  sum_t gamma^(t dt v_pref) r_t, t = 0 at the branch point (set_gamma's table; 0.9 unless set)
            info  uint8    code of the last transition made (REACH_GOAL / COLLISION / TIMEOUT: the branch ended there)
            steps int32    transitions made, 1..n
            time  float64  global_time after the last transition made
        and with final_state=True final_state8 float64 [B, K, A, 8] (get_state()'s layout) and final_theta float64 [B, K]:
        the state after that transition.  `out` reuses a previous call's dict (validated).  No state, rollout buffer, ring
        level or launch counter changes; needs no rollout_begin.  n = 0 is a no-op: the tensors are returned unwritten.
        bootstrap=True (cn_lookahead_values; needs sarl_configure + sarl_set_weights, no occupancy maps, not the mixed rule): the
        dict also holds the final state (as with final_state=True) and
            value float32  V of that state under the engine's value network, for every branch, ended or not
            score float64  ret + gamma^(steps dt v_pref) * value — the n-step return; a branch that ended (REACH_GOAL / COLLISION /
                           TIMEOUT) gets no bootstrap: score = ret
        sort_humans: the humans of the network's rows by decreasing distance to the robot (LSTM-RL's replay-memory order), as
        in sarl_transform; False = env order.  The buffers sarl_export reads may be overwritten.
        The humans of the branches move by the engine's lookahead_human_model: through ORCA unless set_lookahead_human_model said
        'constant_velocity'.  With set_lookahead_goal_weight(w != 0), ret and score include w * (progress towards the goal)."""
        return self._lookahead('lookahead', actions, None, final_state, out, bootstrap, sort_humans)

    def lookahead_paths(self, actions, human_vel, final_state=False, out=None, bootstrap=False, sort_humans=False):
        """lookahead() against the human motion the CALLER predicts (cn_lookahead_paths; with bootstrap=True
        cn_lookahead_paths_values): human_vel [B, n, H, 2] float64 — human_vel[b, t, h] is the velocity human h of env b takes
        during step t of the horizon, shared by the K branches of env b; zeros for the parked placeholders of the mixed rule.
        Every branch is the 'constant_velocity' branch with the table as the humans' policy, in step()'s own order: the swept
        test of step t reads the velocity a human has when the step starts (its state velocity, then human_vel[b, t - 1, h]),
        the move and final_state8's velocity columns take human_vel[b, t, h].  The table that repeats the state velocity gives
        the 'constant_velocity' result, velocities recorded from ORCA humans that do not see the robot the 'orca' result, bit
        for bit; crowdnav_amd.predict builds tables (constant_velocity, to_goal, from_positions).  An argument, not a setting: lookahead_human_model is neither read nor
        changed.  Everything else — actions, the returned dict, final_state / out / bootstrap / sort_humans, n = 0, what is
        borrowed and what is copied — as in lookahead().  Non-finite velocities are not checked.  With
        set_lookahead_goal_weight(w != 0), ret and score include w * (progress towards the goal)."""
        return self._lookahead('lookahead_paths', actions, human_vel, final_state, out, bootstrap, sort_humans)

    def _lookahead(self, who, actions, human_vel, final_state, out, bootstrap, sort_humans):
        """lookahead() (human_vel None) and lookahead_paths(): shapes, the rows of `out`, the one C call."""
        shape = tuple(getattr(actions, 'shape', np.shape(actions)))
        if len(shape) != 4 or shape[0] != self.B or shape[1] < 1 or shape[3] != 2:
            raise ValueError('%s: actions must be [%d, K >= 1, n, 2], got %s' % (who, self.B, shape))
        K, n = int(shape[1]), int(shape[2])
        if human_vel is not None:
            vshape = tuple(getattr(human_vel, 'shape', np.shape(human_vel)))
            if vshape != (self.B, n, self.H, 2):
                raise ValueError('%s: human_vel must be [%d, n = %d, %d, 2], got %s' % (who, self.B, n, self.H, vshape))
        spec = dict(ret=(torch.float64, (self.B, K)), info=(torch.uint8, (self.B, K)), steps=(torch.int32, (self.B, K)),
                    time=(torch.float64, (self.B, K)))
        if final_state or bootstrap:
            spec.update(final_state8=(torch.float64, (self.B, K, self.A, 8)), final_theta=(torch.float64, (self.B, K)))
        if bootstrap:
            spec.update(value=(torch.float32, (self.B, K)), score=(torch.float64, (self.B, K)))
        out = self._rows(who, spec, out)
        if n > 0:
            a, temporary = self._borrow(actions, torch.float64, (self.B, K, n, 2))
            v, temporary_v = self._borrow(human_vel, torch.float64, (self.B, n, self.H, 2))
            lo = C.byref(_struct(CnLookaheadOut, out))
            head = (self._h, n, K, _ptr(a)) + (() if v is None else (_ptr(v),)) + (lo,)
            if bootstrap:
                call = self._lib.cn_lookahead_values if v is None else self._lib.cn_lookahead_paths_values
                check(call(*head, int(bool(sort_humans)), _ptr(out['value']), _ptr(out['score'])))
            else:
                check((self._lib.cn_lookahead_actions if v is None else self._lib.cn_lookahead_paths)(*head))
            self._release(temporary, temporary_v)
        return out

    def set_lookahead_human_model(self, model):
        """How the humans of a lookahead's branches move (cn_lookahead_set_human_model): 'orca' (the default: they react through
        ORCA, which knows their goals) or 'constant_velocity' (every human keeps its current velocity — what a planner fed
        observed positions and velocities can assume; one lane per branch instead of one wave, no ORCA).  Read by lookahead()
        and the plan_* calls that score through it; step(), the rollout calls and the real step inside plan_rollout stay ORCA."""
        if model not in _lib.HUMAN_MODELS:
            raise ValueError('lookahead human model: one of %s, got %r' % (_lib.HUMAN_MODELS, model))
        check(self._lib.cn_lookahead_set_human_model(self._h, _lib.HUMAN_MODELS.index(model)))

    @property
    def lookahead_human_model(self):
        """'orca' or 'constant_velocity' (cn_lookahead_get_human_model)."""
        model = C.c_int()
        check(self._lib.cn_lookahead_get_human_model(self._h, C.byref(model)))
        return _lib.HUMAN_MODELS[model.value]

    def set_lookahead_goal_weight(self, w):
        """The weight of the goal-progress term in every lookahead's return (cn_lookahead_set_goal_weight): with d0 the robot's
        distance to its goal now and d1 the distance after a branch's last transition, ret becomes ret + w * (d0 - d1) — added
        once, undiscounted, whatever way the branch ended — in lookahead(), lookahead_paths(), every mode of lookahead_modes()
        before the reduction, their bootstrap scores, and so in whatever the plan_* calls rank.  info, steps, time, the final
        state, step(), the rollout calls and the real steps inside the plan_*rollout loops do not change.  w >= 0 and finite;
        0.0 (the default) is the lookahead without the term, bit for bit.  Stays set across reset()."""
        check(self._lib.cn_lookahead_set_goal_weight(self._h, float(w)))

    @property
    def lookahead_goal_weight(self):
        """The weight set_lookahead_goal_weight set; 0.0 unless set (cn_lookahead_get_goal_weight)."""
        w = C.c_double()
        check(self._lib.cn_lookahead_get_goal_weight(self._h, C.byref(w)))
        return w.value

    # ---------------------------------------------------------------- device CEM planner (cn_plan_*)
    def plan_begin(self, K, n, elites, iterations, init_std, min_std=0.0, smoothing=0.0, seed=0, bootstrap=False,
                   sort_humans=False):
        """The tensors and settings of a cross-entropy-method planner over this engine (struct cn_plan / cn_plan_cfg): per env a
        Gaussian over sequences of n actions, K candidates drawn from it per iteration, refitted to the `elites` best,
        `iterations` times per planning step.  Returns a Plan whose attributes are device tensors —
            mean, std, best_actions float64 [B, n, 2]; best_score float64 [B]; action float64 [B, 2]
            candidates float64 [B, K, n, 2]; order int32 [B, K] (candidate index at rank r)
            look: the dict lookahead() returns, rows of the last iteration (with bootstrap: final state, value, score too)
        mean starts at zero and std at init_std: call plan_reset() for the goal-directed prior.  ROBOT_EXTERNAL engines: a
        holonomic robot, action rows (vx, vy); a unicycle robot once set_plan_unicycle() has been called, and then every row —
        mean, std, candidates, best_actions, action — is (v, r).  The settings are checked by the first call that uses the plan.  The planner's candidates are scored under the
        engine's lookahead_human_model (set_lookahead_human_model), as it stands when each plan_* call is made.  With
        set_lookahead_goal_weight(w != 0), the ret and score the planner ranks include w * (progress towards the goal)."""
        K, n = int(K), int(n)
        if K < 1 or n < 1:
            raise ValueError('plan_begin: K and n must be >= 1')
        plan = Plan(self, K, n, int(elites), int(iterations), float(init_std), float(min_std), float(smoothing), int(seed),
                    bool(bootstrap), bool(sort_humans))
        std_rotation = getattr(self, '_plan_std_rotation', 0.0)  # (kept by set_plan_unicycle: no library call here)
        if std_rotation > 0.0:  # the engine plans over (v, r): std starts at (init_std, init_std_rotation), as plan_reset leaves it
            plan.std[..., 1] = std_rotation
        return plan

    def set_plan_unicycle(self, max_rotation, init_std_rotation):
        """Opt a unicycle ROBOT_EXTERNAL engine into the plan_* calls (cn_plan_set_unicycle): action rows are then (v, r),
        clipped to v in [0, v_pref] and r in [-max_rotation, max_rotation] in place of the speed disc; plan_reset's prior turns
        towards the goal by at most max_rotation per step from get_theta()'s heading and drives at full speed; std starts at
        (the plan's init_std, init_std_rotation).  max_rotation in (0, pi] (the reference's action space: pi / 4),
        init_std_rotation > 0, radians.  Until it is called every plan_* call refuses a unicycle engine; it cannot be unset, and
        stays set across reset().  Any other engine: CN_ERR_INVALID."""
        check(self._lib.cn_plan_set_unicycle(self._h, float(max_rotation), float(init_std_rotation)))
        self._plan_std_rotation = float(init_std_rotation)

    @property
    def plan_unicycle(self):
        """(max_rotation, init_std_rotation) as set_plan_unicycle set them; (0.0, 0.0) until it has (cn_plan_get_unicycle)."""
        r, s = C.c_double(), C.c_double()
        check(self._lib.cn_plan_get_unicycle(self._h, C.byref(r), C.byref(s)))
        return r.value, s.value

    def _plan_call(self, name, plan, *args, rollout=False, n_real=None, counter=None):
        """check(cn_plan_<name>(engine, [io, [n_real,]] cfg, plan, *args[, counter])), the one way to the planner's entry points.
        rollout: the call takes the io of the rollout in progress (asked for before the plan is looked at) and its bufs are
        returned; counter: cut to the uint32 the library takes."""
        io, bufs = self._roll() if rollout else (None, None)
        if not isinstance(plan, Plan) or plan.engine() is not self:
            raise ValueError('plan: a Plan made by this engine\'s plan_begin()')
        head = [] if not rollout else [C.byref(io)] if n_real is None else [C.byref(io), int(n_real)]
        tail = [] if counter is None else [int(counter) & 0xffffffff]
        check(getattr(self._lib, 'cn_plan_' + name)(self._h, *head, C.byref(plan.cfg), C.byref(plan.c), *args, *tail))
        return bufs

    def plan_reset(self, plan, mask=None):
        """The goal-directed prior (cn_plan_reset): mean = full speed — or what reaches the goal in one step — from the robot
        towards its goal at every t, std = init_std; for the envs of `mask` ([B] bool / uint8, None = all).  With
        set_plan_unicycle: rows (v, r) that turn towards the goal by at most max_rotation a step, then drive straight; std =
        (init_std, init_std_rotation)."""
        m, temporary = self._borrow(mask, torch.uint8, (self.B,))
        self._plan_call('reset', plan, _ptr(m))
        self._release(temporary)
        return plan

    def plan_draw(self, plan, counter):
        """plan.candidates <- K sequences per env from N(mean, std), clipped to the robot's speed; candidate 0 is the mean
        (cn_plan_draw).  Philox4x32-10 keyed by the plan's seed, counter words (t, k, b, counter).  With set_plan_unicycle: rows
        (v, r), clipped to [0, v_pref] x [-max_rotation, max_rotation]."""
        self._plan_call('draw', plan, counter=counter)
        return plan.candidates

    def plan_refit(self, plan, keep_best=False):
        """Rank plan.candidates by plan.look['ret'] (['score'] with bootstrap), write order / best_* / action, refit mean and
        std to the elites (cn_plan_refit).  keep_best: the best sequence is replaced only by a strictly better one."""
        self._plan_call('refit', plan, int(bool(keep_best)))
        return plan

    def plan_cem(self, plan, counter):
        """One planning step (cn_plan_cem): `iterations` x (draw with counter + i, lookahead, refit), all enqueued by one
        call; plan.action then holds the first action of the best sequence found.  The engine is left as lookahead() leaves it."""
        self._plan_call('cem', plan, counter=counter)
        return plan

    def plan_shift(self, plan):
        """After rollout_step(plan.action) (cn_plan_shift): the plan of a running env moves up by one step (std back to
        init_std), an env whose episode has just ended gets the prior of its new scenario, a retired env is left alone.  With
        set_plan_unicycle: rows (v, r), std back to (init_std, init_std_rotation)."""
        self._plan_call('shift', plan, rollout=True)
        return plan

    def plan_rollout(self, plan, n_real, counter):
        """n_real closed-loop steps in ONE call without host work or synchronisation in between (cn_plan_rollout): per step
        plan_cem(counter + s * iterations), rollout_step(plan.action), plan_shift.  Returns the rollout's bufs."""
        return self._plan_call('rollout', plan, rollout=True, n_real=n_real, counter=counter)

    # ---------------------------------------------------------------- device MPPI update (cn_plan_mppi_*), on the same Plan
    def plan_mppi_update(self, plan, temperature, fit_std=False, keep_best=False):
        """The MPPI update in place of plan_refit (cn_plan_mppi_update): the same ranks, order and best_*; every candidate
        weighted by exp((score - best score) / temperature); mean <- the weighted mean (through smoothing), std <- the weighted
        deviation only with fit_std; plan.action <- the updated mean's first row, clipped to the robot's speed (with
        set_plan_unicycle: a (v, r) row clipped to its box).  The plan's `elites` is not read."""
        self._plan_call('mppi_update', plan, float(temperature), int(bool(fit_std)), int(bool(keep_best)))
        return plan

    def plan_mppi(self, plan, temperature, counter, fit_std=False):
        """One planning step (cn_plan_mppi): `iterations` x (draw with counter + i, lookahead, MPPI update), all enqueued by
        one call.  The engine is left as lookahead() leaves it."""
        self._plan_call('mppi', plan, float(temperature), int(bool(fit_std)), counter=counter)
        return plan

    # ---------------------------------------------------------------- planning against predicted human motion
    def _plan_paths(self, name, plan, human_vel, *args, counter):
        if not isinstance(plan, Plan) or plan.engine() is not self:
            raise ValueError('plan: a Plan made by this engine\'s plan_begin()')
        v, temporary = self._borrow(human_vel, torch.float64, (self.B, plan.n, self.H, 2))
        if v is None:
            raise ValueError('plan_%s: human_vel is required ([%d, %d, %d, 2])' % (name, self.B, plan.n, self.H))
        self._plan_call(name, plan, _ptr(v), *args, counter=counter)
        self._release(temporary)
        return plan

    def plan_cem_paths(self, plan, human_vel, counter):
        """plan_cem with its candidates scored by lookahead_paths (cn_plan_cem_paths): human_vel [B, n, H, 2] float64, the
        predicted velocity of every human at every step of the plan's horizon.  There is no rollout form: predict from the state
        after each real step — plan_cem_paths, rollout_step(plan.action), plan_shift."""
        return self._plan_paths('cem_paths', plan, human_vel, counter=counter)

    def plan_mppi_paths(self, plan, human_vel, temperature, counter, fit_std=False):
        """plan_mppi with its candidates scored by lookahead_paths (cn_plan_mppi_paths)."""
        return self._plan_paths('mppi_paths', plan, human_vel, float(temperature), int(bool(fit_std)), counter=counter)

    # ---------------------------------------------------------------- several predicted futures at once (cn_*_modes)
    def _path_modes(self, who, n, human_vel, weights, reduce, risk_penalty):
        """(struct cn_path_modes, M, what was borrowed) of a *_modes call: the shapes and `reduce` are checked before the
        library or the device is asked."""
        vshape = tuple(getattr(human_vel, 'shape', np.shape(human_vel)))
        if len(vshape) != 5 or vshape[:1] + vshape[2:] != (self.B, n, self.H, 2) or not 1 <= vshape[1] <= _lib.MODES_MAX:
            raise ValueError('%s: human_vel must be [%d, M in 1..%d, n = %d, %d, 2], got %s'
                             % (who, self.B, _lib.MODES_MAX, n, self.H, vshape))
        M = int(vshape[1])
        if reduce not in _lib.MODES_REDUCE:
            raise ValueError('%s: reduce must be one of %s, got %r' % (who, _lib.MODES_REDUCE, reduce))
        if weights is not None:
            wshape = tuple(getattr(weights, 'shape', np.shape(weights)))
            if wshape != (self.B, M):
                raise ValueError('%s: weights must be [%d, M = %d], got %s' % (who, self.B, M, wshape))
        v, temporary_v = self._borrow(human_vel, torch.float64, (self.B, M, n, self.H, 2))
        w, temporary_w = self._borrow(weights, torch.float64, (self.B, M))
        modes = _lib.CnPathModes(n_modes=M, reduce=_lib.MODES_REDUCE.index(reduce), risk_penalty=float(risk_penalty),
                                 human_vel=v.data_ptr(), weight=None if w is None else w.data_ptr())
        return modes, M, (v, w), (temporary_v, temporary_w)

    def lookahead_modes(self, actions, human_vel, weights=None, reduce='mean', risk_penalty=0.0, per_mode=False, out=None):
        """lookahead_paths() against M predicted futures at once, reduced per branch (cn_lookahead_modes): human_vel
        [B, M, n, H, 2] float64 — human_vel[b, m] is lookahead_paths' table of env b under mode m (predict.stack_modes builds it);
        weights [B, M] float64 or None = 1 / M each, used as given (not normalised).  The robot of a branch is moved once and
        tested against the M sets of humans: the action table is read once.  Mode m of branch (b, k) is lookahead_paths' branch
        with table human_vel[:, m], bit for bit; each mode ends at its own first done.  Returns a dict of device tensors, rows
        [b, k]:
            score       float64  r - risk_penalty * risk; r = sum_m w_m ret_m ('mean') or min_m ret_m ('min', weights not read)
            risk        float64  sum_m w_m [mode m ended in COLLISION]
            worst_mode  int32    the smallest m with the lowest ret_m; worst_info uint8, worst_steps int32, worst_time float64:
                                 that mode's info, steps and time
        and with per_mode=True ret float64, info uint8, steps int32, time float64 [B, K, M].  There is no final state and no
        bootstrap.  actions, `out`, n = 0, what is borrowed and what is copied: as in lookahead().  No state, rollout buffer,
        ring level, launch counter or lookahead_human_model changes.  With set_lookahead_goal_weight(w != 0), every mode's ret —
        and so score, worst_mode and the worst rows — includes w * (progress towards the goal at that mode's last step)."""
        who = 'lookahead_modes'
        shape = tuple(getattr(actions, 'shape', np.shape(actions)))
        if len(shape) != 4 or shape[0] != self.B or shape[1] < 1 or shape[3] != 2:
            raise ValueError('%s: actions must be [%d, K >= 1, n, 2], got %s' % (who, self.B, shape))
        K, n = int(shape[1]), int(shape[2])
        modes, M, keep, temporary = self._path_modes(who, n, human_vel, weights, reduce, risk_penalty)
        spec = dict(score=(torch.float64, (self.B, K)), risk=(torch.float64, (self.B, K)), worst_mode=(torch.int32, (self.B, K)),
                    worst_info=(torch.uint8, (self.B, K)), worst_steps=(torch.int32, (self.B, K)),
                    worst_time=(torch.float64, (self.B, K)))
        if per_mode:
            spec.update(ret=(torch.float64, (self.B, K, M)), info=(torch.uint8, (self.B, K, M)),
                        steps=(torch.int32, (self.B, K, M)), time=(torch.float64, (self.B, K, M)))
        out = self._rows(who, spec, out)
        if n > 0:
            a, temporary_a = self._borrow(actions, torch.float64, (self.B, K, n, 2))
            check(self._lib.cn_lookahead_modes(self._h, n, K, _ptr(a), C.byref(modes), C.byref(_struct(_lib.CnModesOut, out))))
            self._release(temporary_a, *temporary)
        del keep
        return out

    def _plan_modes(self, name, plan, human_vel, weights, reduce, risk_penalty, *args, counter):
        if not isinstance(plan, Plan) or plan.engine() is not self:
            raise ValueError('plan: a Plan made by this engine\'s plan_begin()')
        modes, _, keep, temporary = self._path_modes('plan_' + name, plan.n, human_vel, weights, reduce, risk_penalty)
        self._plan_call(name, plan, C.byref(modes), *args, counter=counter)
        self._release(*temporary)
        del keep
        return plan

    def plan_cem_modes(self, plan, human_vel, counter, weights=None, reduce='mean', risk_penalty=0.0):
        """plan_cem with its candidates scored by lookahead_modes (cn_plan_cem_modes): human_vel [B, M, n, H, 2], weights, reduce
        and risk_penalty as there.  plan.look['ret'] receives the reduced score — which the refit ranks — and look['info'] /
        ['steps'] / ['time'] the worst mode's rows.  A plan with bootstrap=True is refused.  No rollout form, as for
        plan_cem_paths."""
        return self._plan_modes('cem_modes', plan, human_vel, weights, reduce, risk_penalty, counter=counter)

    def plan_mppi_modes(self, plan, human_vel, temperature, counter, weights=None, reduce='mean', risk_penalty=0.0, fit_std=False):
        """plan_mppi with its candidates scored by lookahead_modes (cn_plan_mppi_modes)."""
        return self._plan_modes('mppi_modes', plan, human_vel, weights, reduce, risk_penalty, float(temperature),
                                int(bool(fit_std)), counter=counter)

    def plan_mppi_rollout(self, plan, n_real, temperature, counter, fit_std=False):
        """plan_rollout with the MPPI update (cn_plan_mppi_rollout): per step plan_mppi(counter + s * iterations),
        rollout_step(plan.action), plan_shift, in ONE call.  Returns the rollout's bufs."""
        return self._plan_call('mppi_rollout', plan, float(temperature), int(bool(fit_std)), rollout=True, n_real=n_real,
                               counter=counter)

    # ---------------------------------------------------------------- the shipped predictors on the device (cn_predict)
    def predict(self, n, models='to_goal', out=None):
        """The table of predicted human velocities crowdnav_amd.predict makes from get_state(), made on the device from the
        state as it stands, in one launch (cn_predict): bit for bit predict.constant_velocity(state8, n) or
        predict.to_goal(state8, n, time_step).  models: 'constant_velocity' (alias 'cv') or 'to_goal' returns float64
        [B, n, H, 2], lookahead_paths' table; a sequence of 1 .. 8 such names [B, M, n, H, 2], lookahead_modes' (mode m by
        models[m]).  `out` reuses a contiguous float64 device tensor of that shape.  Any engine, ORCA-robot and unicycle ones
        included: only the humans are read, and nothing of the engine — state, rollout buffers, ring levels,
        lookahead_human_model, launch counters — is written.  n = 0 is a no-op: the empty tensor is returned."""
        codes, single = _predict_models('predict', models)
        n = int(n)
        if n < 0:
            raise ValueError('predict: n must be >= 0')
        shape = (self.B, n, self.H, 2) if single else (self.B, len(codes), n, self.H, 2)
        if out is None:
            out = self._new(shape, torch.float64)
        elif not self._dense(out, torch.float64, shape):
            raise ValueError('predict: out must be a contiguous %s %s tensor on %s' % (torch.float64, shape, self.device))
        if n > 0:
            check(self._lib.cn_predict(self._h, n, len(codes), (C.c_int32 * len(codes))(*codes), _ptr(out)))
        return out

    def plan_predict_begin(self, plan, models, weights=None, reduce='mean', risk_penalty=0.0):
        """The device predictors a closed loop plans against (struct cn_predictors), for plan_predict_rollout: models as in
        predict() — one name: the plan_*_paths planners; a sequence of M names: the plan_*_modes planners with weights
        ([B, M] float64 or None = 1 / M each; copied), reduce ('mean' | 'min') and risk_penalty as in lookahead_modes (a
        sequence of ONE name is the paths planner too: M = 1 reads neither).  Returns a Predictors holder that owns the scratch
        table .human_vel [B, M, plan.n, H, 2] the predictions are written to."""
        if not isinstance(plan, Plan) or plan.engine() is not self:
            raise ValueError('plan: a Plan made by this engine\'s plan_begin()')
        codes, _ = _predict_models('plan_predict_begin', models)
        if reduce not in _lib.MODES_REDUCE:
            raise ValueError('plan_predict_begin: reduce must be one of %s, got %r' % (_lib.MODES_REDUCE, reduce))
        if weights is not None:
            wshape = tuple(getattr(weights, 'shape', np.shape(weights)))
            if wshape != (self.B, len(codes)):
                raise ValueError('plan_predict_begin: weights must be [%d, M = %d], got %s' % (self.B, len(codes), wshape))
        return Predictors(self, plan, codes, weights, reduce, risk_penalty)

    def plan_predict_rollout(self, plan, pred, n_real, counter, temperature=None, fit_std=False):
        """n_real closed-loop steps against the device predictors in ONE call, nothing on the host in between
        (cn_plan_cem_predict_rollout; with a temperature cn_plan_mppi_predict_rollout): per step predict() from the state as
        it stands into pred.human_vel, plan_cem_paths / plan_mppi_paths (M > 1: plan_cem_modes / plan_mppi_modes) with
        counter + s * iterations, rollout_step(plan.action), plan_shift — bit for bit what those calls give with
        crowdnav_amd.predict's tables of get_state().  Returns the rollout's bufs."""
        if not isinstance(plan, Plan) or plan.engine() is not self:
            raise ValueError('plan: a Plan made by this engine\'s plan_begin()')
        if not isinstance(pred, Predictors) or pred.engine() is not self or pred.plan() is not plan:
            raise ValueError('pred: the Predictors made by this engine\'s plan_predict_begin() for this plan')
        if temperature is None:
            return self._plan_call('cem_predict_rollout', plan, C.byref(pred.c), rollout=True, n_real=n_real, counter=counter)
        return self._plan_call('mppi_predict_rollout', plan, C.byref(pred.c), float(temperature), int(bool(fit_std)), rollout=True,
                               n_real=n_real, counter=counter)

    # ---------------------------------------------------------------- the ORCA predictor: the robot unseen (cn_predict_orca) ...
    def predict_orca(self, n, out=None, mode=None):
        """The table of human velocities ORCA among the humans gives when they do not see the robot, n steps from the state as
        it stands, in one launch (cn_predict_orca): what step() reports in orca_vel[:, 1:] on an engine with robot_visible = 0
        and freshly built simulators (drop_sims), step after step, as float64 — the humans' own policy, so on such an engine
        lookahead_paths(actions, predict_orca(n)) is lookahead(actions) under 'orca'.  mode=None returns float64 [B, n, H, 2],
        lookahead_paths' table (`out` reuses a contiguous float64 device tensor of that shape).  With `out` a contiguous
        float64 [B, M, n, H, 2] device tensor (M in 1 .. 8) and mode=m, slot m of it — one future of a lookahead_modes table
        whose other slots predict() or the caller made — is filled, no other slot is touched, and `out` is returned.  Any
        engine, ORCA-robot, unicycle and robot_visible = 1 ones included; nothing of the engine — state, rollout buffers, ring
        levels, simulators, lookahead_human_model, launch counters — is written.  n = 0 is a no-op."""
        return self._predict_orca('predict_orca', n, out, mode, None)

    def _predict_orca(self, who, n, out, mode, robot_actions):
        n = int(n)
        if n < 0:
            raise ValueError('%s: n must be >= 0' % who)
        rows = None if robot_actions is None else self._action_rows(who, robot_actions, n)
        if mode is None:
            M, m, shape = 1, 0, (self.B, n, self.H, 2)
            if out is None:
                out = self._new(shape, torch.float64)
        else:
            if out is None:
                raise ValueError('%s: mode needs out, the [%d, M, %d, %d, 2] table whose slot is filled' % (who, self.B, n, self.H))
            oshape = tuple(getattr(out, 'shape', ()))
            M = int(oshape[1]) if len(oshape) == 5 else 0
            if not 1 <= M <= _lib.MODES_MAX:
                raise ValueError('%s: out must be [%d, M in 1..%d, n = %d, %d, 2], got %s'
                                 % (who, self.B, _lib.MODES_MAX, n, self.H, oshape))
            if isinstance(mode, bool) or not isinstance(mode, (int, np.integer)) or not 0 <= mode < M:
                raise ValueError('%s: mode must be an int in 0 .. M - 1 = %d, got %r' % (who, M - 1, mode))
            m, shape = int(mode), (self.B, M, n, self.H, 2)
        if not self._dense(out, torch.float64, shape):
            raise ValueError('%s: out must be a contiguous %s %s tensor on %s' % (who, torch.float64, shape, self.device))
        if n > 0 and rows is None:
            check(self._lib.cn_predict_orca(self._h, n, M, m, _ptr(out)))
        elif n > 0:
            a, stride, temporary = rows
            check(self._lib.cn_predict_orca_robot(self._h, n, M, m, _ptr(a), stride, _ptr(out)))
            self._release(temporary)
        return out

    def _action_rows(self, who, robot_actions, n):
        """(tensor, rows between envs, whether it is a temporary copy) of a [B, n, 2] table of robot actions: a float64 tensor on
        the engine's device whose last two dimensions are contiguous is read where it lies, whatever lies between its envs —
        plan.candidates[:, 0] as it is; anything else is copied to a dense table there."""
        shape = tuple(getattr(robot_actions, 'shape', np.shape(robot_actions)))
        if shape != (self.B, n, 2):
            raise ValueError('%s: robot_actions must be [%d, n = %d, 2], got %s' % (who, self.B, n, shape))
        t = robot_actions
        if not (torch.is_tensor(t) and t.device == self.device and t.dtype == torch.float64):
            t, temporary = self._borrow(t, torch.float64, shape)
            return t, n, temporary
        if n == 0:
            return t, 0, False
        between, row, last = t.stride()
        if last != 1 or (n > 1 and row != 2):
            raise ValueError('%s: robot_actions: the last two dimensions must be contiguous (strides %s)' % (who, (between, row, last)))
        if self.B == 1:
            return t, n, False
        if between % 2 or between < 2 * n:
            raise ValueError('%s: robot_actions: %d elements between envs are not a whole number of rows >= n = %d'
                             % (who, between, n))
        return t, between // 2, False

    # ---------------------------------------------------------------- ... the robot in sight, on its nominal plan (cn_predict_orca_robot)
    def predict_orca_robot(self, n, robot_actions, out=None, mode=None):
        """predict_orca's table with the robot in the humans' sight, following robot_actions [B, n, 2] float64
        (cn_predict_orca_robot): what step(robot_actions[:, t]) reports in orca_vel[:, 1:], t = 0 .. n - 1, on an external-robot
        engine with robot_visible = 1 and fresh simulators started from this engine's state.  Within a step the humans solve
        against the robot where it stands and with the velocity it has, move, and then the robot takes its row: (vx, vy) used as
        given, not clipped; ActionRot (v, r) on a unicycle engine, from get_theta()'s heading.  The robot has no collision test
        and no episode end: all n rows are followed.  For the sequence itself lookahead_paths on this table is lookahead() under
        'orca' on a robot_visible = 1 engine with fresh simulators; for any other candidate the humans avoid the nominal robot,
        not that candidate.  robot_actions: a float64 tensor on the engine's device whose last two dimensions are contiguous is
        read where it lies — plan.candidates[:, 0], the plan's clipped mean after plan_draw, as it is (ValueError if what lies
        between its envs is not whole rows); a numpy array or CPU tensor is copied to the device.  out, mode, n = 0 and what
        the call leaves alone: as predict_orca.  Any engine, robot_visible = 0 ones included: the humans of this call see the
        robot all the same."""
        if robot_actions is None:
            raise ValueError('predict_orca_robot: robot_actions is required ([%d, n, 2]); predict_orca(n) leaves the robot out' % self.B)
        return self._predict_orca('predict_orca_robot', n, out, mode, robot_actions)

    def plan_predict_orca_rollout(self, plan, pred, n_real, counter, orca_mode=0, temperature=None, fit_std=False):
        """plan_predict_rollout with future `orca_mode` of pred made by predict_orca (cn_plan_cem_predict_orca_rollout; with a
        temperature cn_plan_mppi_predict_orca_rollout): per step predict() into pred.human_vel, predict_orca(plan.n,
        out=pred.human_vel, mode=orca_mode) over that slot, the paths (M = 1) or modes planner, rollout_step(plan.action),
        plan_shift — ONE call, bit for bit what those calls give.  pred: plan_predict_begin's, whose name for slot orca_mode is
        computed and overwritten.  Returns the rollout's bufs."""
        return self._orca_rollout('plan_predict_orca_rollout', 'predict_orca_rollout', plan, pred, n_real, counter, orca_mode,
                                  temperature, fit_std)

    def plan_predict_orca_nominal_rollout(self, plan, pred, n_real, counter, orca_mode=0, temperature=None, fit_std=False):
        """plan_predict_orca_rollout whose ORCA future sees the robot on the plan's nominal sequence
        (cn_plan_cem_predict_orca_nominal_rollout; with a temperature the mppi one): per step plan_draw(plan, c) with
        c = counter + s * iterations, predict() into pred.human_vel, predict_orca_robot(plan.n, plan.candidates[:, 0],
        out=pred.human_vel, mode=orca_mode), the paths or modes planner with c, rollout_step(plan.action), plan_shift — ONE
        call, bit for bit what those calls give.  One prediction per planning step, not per iteration."""
        return self._orca_rollout('plan_predict_orca_nominal_rollout', 'predict_orca_nominal_rollout', plan, pred, n_real, counter,
                                  orca_mode, temperature, fit_std)

    def _orca_rollout(self, who, name, plan, pred, n_real, counter, orca_mode, temperature, fit_std):
        if not isinstance(plan, Plan) or plan.engine() is not self:
            raise ValueError('plan: a Plan made by this engine\'s plan_begin()')
        if not isinstance(pred, Predictors) or pred.engine() is not self or pred.plan() is not plan:
            raise ValueError('pred: the Predictors made by this engine\'s plan_predict_begin() for this plan')
        if isinstance(orca_mode, bool) or not isinstance(orca_mode, (int, np.integer)) or not 0 <= orca_mode < pred.c.n_modes:
            raise ValueError('%s: orca_mode must be an int in 0 .. M - 1 = %d, got %r' % (who, pred.c.n_modes - 1, orca_mode))
        if temperature is None:
            return self._plan_call('cem_' + name, plan, C.byref(pred.c), int(orca_mode), rollout=True, n_real=n_real, counter=counter)
        return self._plan_call('mppi_' + name, plan, C.byref(pred.c), int(orca_mode), float(temperature), int(bool(fit_std)),
                               rollout=True, n_real=n_real, counter=counter)

    # ---------------------------------------------------------------- ... on hypothesised goals, M futures in one launch (cn_predict_orca_goals)
    def predict_orca_goals(self, n, goals, out=None):
        """predict_orca's table for M hypotheses about where the humans are heading, in one launch (cn_predict_orca_goals):
        goals float64 [B, M, H, 2] (M in 1 .. 8) returns float64 [B, M, n, H, 2], lookahead_modes' table — in mode m human h
        heads for goals[b, m, h] instead of its goal in the engine's state, everything else as predict_orca: the robot unseen,
        fresh simulators, all n rows written.  goals [B, H, 2] is taken as M = 1 and returns [B, n, H, 2], lookahead_paths'
        table.  With the engine's own goals (get_state()[0][:, 1:, 4:6]) a mode is predict_orca(n) bit for bit; a parked
        placeholder of the `mixed` rule ignores its row.  goals: a contiguous float64 tensor on the engine's device is read
        where it lies, anything else is copied there; goal_hypotheses() makes one from the state.  `out` reuses a contiguous
        float64 device tensor of the returned shape.  Any engine; nothing of the engine is written and the call is not in
        launch_counts().  n = 0 is a no-op."""
        n = int(n)
        if n < 0:
            raise ValueError('predict_orca_goals: n must be >= 0')
        gshape = tuple(getattr(goals, 'shape', np.shape(goals)))
        single = len(gshape) == 3
        M = 1 if single else (int(gshape[1]) if len(gshape) == 4 else 0)
        if not 1 <= M <= _lib.MODES_MAX or gshape != ((self.B, self.H, 2) if single else (self.B, M, self.H, 2)):
            raise ValueError('predict_orca_goals: goals must be [%d, M in 1..%d, %d, 2] or [%d, %d, 2], got %s'
                             % (self.B, _lib.MODES_MAX, self.H, self.B, self.H, gshape))
        shape = (self.B, n, self.H, 2) if single else (self.B, M, n, self.H, 2)
        if out is None:
            out = self._new(shape, torch.float64)
        elif not self._dense(out, torch.float64, shape):
            raise ValueError('predict_orca_goals: out must be a contiguous %s %s tensor on %s' % (torch.float64, shape, self.device))
        if n > 0:
            g, temporary = self._borrow(goals, torch.float64, gshape)
            check(self._lib.cn_predict_orca_goals(self._h, n, M, _ptr(g), _ptr(out)))
            self._release(temporary)
        return out

    def goal_hypotheses(self, M, base='heading', reach=None, std_heading=0.0, std_distance=0.0, nominal_first=True, seed=0,
                        counter=0, out=None):
        """M sets of hypothesised human goals, float64 [B, M, H, 2], made on the device from the state as it stands
        (cn_goal_hypotheses) — predict_orca_goals' table; bit for bit crowdnav_amd.predict.goal_hypotheses on get_state() apart
        from the device's log, cos and sin.  base 'heading': a human's nominal goal lies `reach` metres along its velocity (a
        standing human's is where it stands) — positions and velocities only, what a planner outside the simulator observes;
        reach=None means human_v_pref * time_step * 12, the way a human at its preferred speed makes in twelve steps, the
        horizon the planners here look ahead.  base 'engine': the nominal goal is the engine's own.  Mode 0 is the nominal goal
        when nominal_first; every other mode turns the offset from the human to it by std_heading * z1 radians and stretches
        it by 1 + std_distance * z2 (not below 0), (z1, z2) standard normal from Philox under (seed, counter): the same
        arguments give the same table, another counter another one.  `out` reuses a contiguous float64 device tensor.  Any
        engine; nothing of the engine is written."""
        if base not in _lib.GOALS_BASES:
            raise ValueError('goal_hypotheses: base must be one of %s, got %r' % (_lib.GOALS_BASES, base))
        M = int(M)
        if not 1 <= M <= _lib.MODES_MAX:
            raise ValueError('goal_hypotheses: M must be in 1..%d, got %d' % (_lib.MODES_MAX, M))
        if reach is None:
            reach = self.config['human_v_pref'] * self.config['time_step'] * 12 if base == 'heading' else 0.0
        shape = (self.B, M, self.H, 2)
        if out is None:
            out = self._new(shape, torch.float64)
        elif not self._dense(out, torch.float64, shape):
            raise ValueError('goal_hypotheses: out must be a contiguous %s %s tensor on %s' % (torch.float64, shape, self.device))
        check(self._lib.cn_goal_hypotheses(self._h, M, _lib.GOALS_BASES.index(base), float(reach), float(std_heading),
                                           float(std_distance), int(bool(nominal_first)), int(seed) & 0xffffffffffffffff,
                                           int(counter) & 0xffffffff, _ptr(out)))
        return out

    # ---------------------------------------------------------------- shard boundary (explorer.py:74-90)
    def rollout_records(self, max_records=None):
        """The finished episodes of this engine's rollout as ONE self-contained float64 block per env:
        [B, 1 + 6 K] = (episodes finished, K x (outcome, steps, discounted return, nav time, danger steps, danger dmin
        sum)); see distributed.split_blocks.  One kernel (cn_rollout_records)."""
        io, bufs = self._roll()
        K = int(bufs['ep_outcome'].shape[1] if max_records is None else max_records)
        blocks = self._new((self.B, 1 + K * _lib.RECORD_FIELDS), torch.float64)
        check(self._lib.cn_rollout_records(self._h, C.byref(io), K, _ptr(blocks)))
        return blocks

    def records_summary(self, blocks, record_capacity=None, out=None):
        """float64 [8]: episodes finished, records held, ReachGoal / Collision / Timeout among them, sum of successful nav
        times, sum of discounted returns, sum of Danger steps — of any [n, 1 + 6 K] record blocks, a shard's own or the
        gathered ones (cn_records_summary: one workgroup, fixed summation order)."""
        K = (int(blocks.shape[1]) - 1) // _lib.RECORD_FIELDS
        cap = K if record_capacity is None else int(record_capacity)
        out = self._summary_out(out)
        check(self._lib.cn_records_summary(self._h, int(blocks.shape[0]), K, cap, _ptr(blocks), _ptr(out)))
        return out

    def _summary_out(self, out):
        if out is None:
            return self._new((_lib.SUMMARY_FIELDS,), torch.float64)
        if not self._dense(out, torch.float64, out.shape) or out.numel() != _lib.SUMMARY_FIELDS:  # 8 numbers in any shape
            raise ValueError('summary output: a contiguous float64 [%d] tensor on %s' % (_lib.SUMMARY_FIELDS, self.device))
        return out

    def rollout_summary(self, out=None):
        """records_summary(rollout_records()) of this engine in ONE kernel, straight from its record rings (cn_rollout_summary):
        the statistics of explorer.py:74-90 for a run on one engine.  out: the caller's float64 [8] device tensor (a run that
        asks once per boundary keeps one: no allocation between the last launch and the kernel)."""
        io, _ = self._roll()
        out = self._summary_out(out)
        check(self._lib.cn_rollout_summary(self._h, C.byref(io), _ptr(out)))
        return out

    def gather_records_rccl(self, comm, n_ranks, blocks):
        """All-gather the record blocks of every rank over the caller's RCCL communicator (`comm`: the ncclComm_t as an
        integer, see crowdnav_amd.rccl) on the engine's stream (cn_gather_records): [n_ranks * B, 1 + 6 K]."""
        K = (int(blocks.shape[1]) - 1) // _lib.RECORD_FIELDS
        out = self._new((n_ranks * self.B, int(blocks.shape[1])), torch.float64)
        check(self._lib.cn_gather_records(self._h, C.c_void_p(int(comm)), int(n_ranks), K, _ptr(blocks), _ptr(out)))
        return out

    def launch_counts(self):
        """What the host has enqueued for this engine since it was created (cn_launch_counts): dict of _lib.LAUNCH_COUNTERS ->
        int, and 'lagged_fills' (cn_lagged_fills): how many of 'ring_fills' ran on the side stream beside a launch instead of in
        front of one.  Host-side, no device work: the difference of two calls says which launches a region contained."""
        out = (C.c_uint64 * len(_lib.LAUNCH_COUNTERS))()
        check(self._lib.cn_launch_counts(self._h, out))
        lagged = C.c_uint64()
        check(self._lib.cn_lagged_fills(self._h, C.byref(lagged)))
        return dict(zip(_lib.LAUNCH_COUNTERS, (int(v) for v in out)), lagged_fills=int(lagged.value))

    def fresh_starts(self):
        """Two-wave rollout kernel, since the engine was created (cn_fresh_starts): 'adopted' episode starts that took the first
        step solved when their ring slot was filled, 'redone' iterations a workgroup computed again because one could not, and
        'kernels', the launches of the solving kernel.  Waits for the engine's stream."""
        out = (C.c_uint64 * 3)()
        check(self._lib.cn_fresh_starts(self._h, out))
        return dict(adopted=int(out[0]), redone=int(out[1]), kernels=int(out[2]))

    def ring_slot(self, env, slot):
        """Ring slot `slot` of env `env` as the last fill left it (cn_ring_slot): (state8 float64 [A, 8] in get_state's layout,
        vel0 float32 [A, 2], ok) as numpy arrays and a bool — vel0 is the slot's solved first step where ok."""
        state8 = np.zeros((self.A, 8), np.float64)
        vel0 = np.zeros((self.A, 2), np.float32)
        ok = C.c_int(0)
        check(self._lib.cn_ring_slot(self._h, int(env), int(slot), state8.ctypes.data_as(C.c_void_p),
                                     vel0.ctypes.data_as(C.c_void_p), C.byref(ok)))
        return state8, vel0, bool(ok.value)

    def rollout_route(self, n_steps):
        """Which transition kernel rollout(n_steps) would launch now (cn_rollout_route): one of _lib.ROLLOUT_ROUTES — 'generic',
        'fused' (one wave per workgroup), 'fused_split' (an ORCA wave and an env wave per workgroup) or 'shard'.  Host-side,
        launches nothing."""
        route = C.c_int(-1)
        check(self._lib.cn_rollout_route(self._h, int(n_steps), C.byref(route)))
        return _lib.ROLLOUT_ROUTES[route.value]

    def sarl_network_route(self):
        """Which kernel family runs the value network of this engine's sarl_configure (cn_sarl_network_route): one of
        _lib.SARL_ROUTES — 'lds_tile', 'lds_chunked', 'narrow', 'reg_sarl', 'reg_sarl_chunk', 'reg_cadrl', 'reg_lstm', 'reg_lstm2'
        or 'split_f16' (precision='f16x2').  Host-side, launches nothing."""
        route = C.c_int(-1)
        check(self._lib.cn_sarl_network_route(self._h, C.byref(route)))
        return _lib.SARL_ROUTES[route.value]

    def geometry(self):
        """The workgroup geometry this engine got when it was created (cn_debug_geometry), after the clamps on the
        CROWDNAV_AMD_ENVS_PER_WAVE / CROWDNAV_AMD_WAVES_PER_BLOCK knobs: dict of 'E' (envs per workgroup), 'threads' (64 per
        wave), 'lds_bytes' and 'grid' (workgroups of the per-env kernels).  Read-only, host-side, launches nothing."""
        out = (C.c_int * 4)()
        check(self._lib.cn_debug_geometry(self._h, out))
        return dict(E=int(out[0]), threads=int(out[1]), lds_bytes=int(out[2]), grid=int(out[3]))

    def mt_random(self, seed, n):
        out = self._new((n,), torch.float64)
        check(self._lib.cn_mt_random(self._h, int(seed), int(n), _ptr(out)))
        return out

    # ---------------------------------------------------------------- SARL decision
    def sarl_configure(self, actions, gamma=0.9, with_om=False, cell_num=4, cell_size=1.0, om_channel_size=3,
                       with_global_state=True, mlp1_dims=(150, 100), mlp2_dims=(100, 50), attention_dims=(100, 100, 1),
                       mlp3_dims=(150, 100, 100, 1), model='sarl', interaction_dims=None, query_env=True, precision='f32'):
        """SARL.configure (or model='cadrl': mlp3_dims = [cadrl] mlp_dims; model='lstm_rl': mlp1_dims[0] = hidden width,
        mlp3_dims = [lstm_rl] mlp2_dims, interaction_dims = [lstm_rl] mlp1_dims when with_interaction_module) +
        build_action_space for
        this engine.  actions: [K, 2] float64 ActionXY table (host).  query_env=False: [action_space] query_env = false, the
        constant-velocity human model + MultiHumanRL.compute_reward instead of the env's lookahead.
        precision: 'f32', or 'f16x2' — the split-f16 matrix route (CN_PRECISION_F16X2: sarl.ValueNetwork at the shipped widths, 1..5
        humans; values within 1e-6 of fp32).  The library refuses what that route does not cover (CrowdNavAmdError, status
        CN_ERR_UNSUPPORTED, the engine stays unconfigured): it never falls back.  An integer is passed on as the raw CN_PRECISION_*."""
        acts = np.ascontiguousarray(np.asarray(actions, dtype=np.float64).reshape(-1, 2))
        cfg = _lib.CnSarlConfig(n_actions=len(acts), with_om=int(bool(with_om)), cell_num=int(cell_num),
                                om_channel_size=int(om_channel_size), cell_size=float(cell_size), gamma=float(gamma),
                                with_global_state=int(bool(with_global_state)),
                                mlp1_dims=(C.c_int32 * 2)(*mlp1_dims), mlp2_dims=(C.c_int32 * 2)(*mlp2_dims),
                                attention_dims=(C.c_int32 * 3)(*attention_dims), mlp3_dims=(C.c_int32 * 4)(*mlp3_dims),
                                model={'sarl': 0, 'cadrl': 1, 'lstm_rl': 2}[model],
                                interaction_dims=(C.c_int32 * 4)(*(interaction_dims or (0, 0, 0, 0))),
                                constant_velocity_model=0 if query_env else 1,
                                precision=_lib.PRECISIONS.index(precision) if isinstance(precision, str) else int(precision))
        check(self._lib.cn_sarl_configure(self._h, C.byref(cfg), acts.ctypes.data_as(C.c_void_p)))
        self.sarl = dict(n_actions=len(acts), in_dim=13 + (cell_num ** 2 * om_channel_size if with_om else 0),
                         actions=acts, model=model, pairwise=bool(interaction_dims))

    def sarl_set_weights(self, state_dict):
        """Hand the value network's parameters (sarl.ValueNetwork.state_dict()) to the device kernels."""
        order = {'cadrl': CADRL_PARAM_ORDER, 'lstm_rl': LSTM_PARAM_ORDER}.get(self.sarl['model'], SARL_PARAM_ORDER)
        if self.sarl.get('pairwise'):  # lstm_rl.ValueNetwork2: mlp1 first, as in its state_dict
            order = LSTM_PAIRWISE_MLP1_ORDER + order
        # parameters that live on the engine's device as dense float32 are read in place (the RL phase uploads weights once per
        # sampled episode: 22 conversions and stream records were ~0.1 ms of host time each time); anything else goes through a copy
        tensors, temporaries = [], []
        for k in order:
            t = state_dict[k]
            if not (t.device == self.device and t.dtype == torch.float32 and t.is_contiguous()):
                t = t.detach().to(device=self.device, dtype=torch.float32).contiguous()
                temporaries.append(t)
            tensors.append(t)
        ptrs = (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
        check(self._lib.cn_sarl_set_weights(self._h, ptrs))
        # the tensors above must outlive the repack kernel: kept until the next call — by then it is long behind on the engine's
        # stream; no synchronize per call.  The caching allocator is told that the engine's stream reads the TEMPORARIES: were the
        # caller inside another torch.cuda.stream(...) context, a freed temporary could otherwise be handed out again on THAT stream
        # while the repack kernel, on the stream captured at construction / use_current_stream(), still reads it.
        for t in temporaries:
            t.record_stream(self._stream)
        self._sarl_weights_keepalive = tensors

    def sarl_select(self, want_values=True, best=None, action=None, want_attention=False):
        """Greedy SARL action of every env: dict(values [B,K] f64, best [B] i32, action [B,2] f64).  best / action: the caller's
        device tensors to write into (e.g. row t of an action history) instead of fresh ones.  want_attention (SARL only): also
        attention [B,K,H] f32, the softmax weights of every lookahead state (cn_sarl_select_attention; 0 for absent humans)."""
        K = self.sarl['n_actions']
        if best is None:
            best = self._new((self.B,), torch.int32)
        if action is None:
            action = self._new((self.B, 2), torch.float64)
        assert best.dtype == torch.int32 and best.is_contiguous() and action.dtype == torch.float64 and action.is_contiguous()
        out = dict(values=self._new((self.B, K), torch.float64) if want_values else None, best=best, action=action)
        if want_attention:
            out['attention'] = self._new((self.B, K, self.H), torch.float32)
            check(self._lib.cn_sarl_select_attention(self._h, _ptr(out['values']), _ptr(out['best']), _ptr(out['action']),
                                                     _ptr(out['attention'])))
        else:
            check(self._lib.cn_sarl_select(self._h, _ptr(out['values']), _ptr(out['best']), _ptr(out['action'])))
        return out

    def sarl_export(self, name):
        """Internal buffers of the last sarl_select (tests): reward, V, next_obs, om, X (natural [B,K,H,ld] order)."""
        K, H = self.sarl['n_actions'], self.H
        if name == 'reward':
            t, which = self._new((self.B, K), torch.float64), 0
        elif name == 'V':
            t, which = self._new((self.B, K), torch.float32), 1
        elif name == 'next_obs':
            t, which = self._new((self.B, H, 5), torch.float64), 2
        elif name == 'om':
            t, which = self._new((self.B, H, self.sarl['in_dim'] - 13), torch.float32), 3
        elif name == 'X':
            d = self.sarl['in_dim']  # cn::sarl_ks: whole 16-column tiles, at least the k loop's 5-step chunks
            ks = max((d + 15) // 16 * 4, ((d + 3) // 4 + 4) // 5 * 5)
            tiles = (self.B * K + 15) // 16
            t, which = self._new((tiles, H, ks, 4, 16), torch.float32), 4  # MFMA A-fragment order
        else:
            raise KeyError(name)
        check(self._lib.cn_sarl_export(self._h, which, _ptr(t), t.numel() * t.element_size()))
        if name == 'X':  # [tile][h][k-step][k % 4][g] -> [B, K, H, in_dim]
            t = t.permute(0, 4, 1, 2, 3).reshape(-1, H, t.shape[2] * 4)[:self.B * K, :, :self.sarl['in_dim']]
            t = t.reshape(self.B, K, H, -1)
        return t

    def sarl_explore(self, sel, epsilon, mask=None, want_explored=True):
        """Epsilon-greedy on top of a sarl_select result (in place): each env draws np.random.random() — and, below
        epsilon, np.random.choice(K) — from the numpy stream its last reset() seeded (multi_human_rl.py:28-31)."""
        m, _ = self._borrow(mask, torch.uint8, (self.B,))
        explored = self._new((self.B,), torch.uint8) if want_explored else None
        check(self._lib.cn_sarl_explore(self._h, float(epsilon), _ptr(m), _ptr(sel['best']), _ptr(sel['action']),
                                        _ptr(explored)))
        sel['explored'] = explored
        return sel

    def sarl_transform(self, out=None, env_stride=0, sort_humans=None):
        """MultiHumanRL.transform of every env's current joint state: [B, H, in_dim] float32 (replay-memory state).
        With out (a float32 device tensor) and env_stride (floats between consecutive envs) the rows are written in place,
        e.g. out = traj[:, t] of a [B, T, H, D] trajectory tensor with env_stride = T * H * D.  sort_humans: LSTM-RL's
        decreasing-distance order (default for that model: the RL phase); False = env order (imitation learning)."""
        if out is None:
            out = self._new((self.B, self.H, self.sarl['in_dim']), torch.float32)
        assert out.dtype == torch.float32 and out.device.type == self.device.type
        if sort_humans is None:  # what a train-phase predict() of this model leaves in last_state
            sort_humans = self.sarl['model'] == 'lstm_rl'
        check(self._lib.cn_sarl_transform(self._h, C.c_void_p(out.data_ptr()), int(env_stride), int(bool(sort_humans))))
        return out

    def sarl_sampler(self, traj, rew, info, dmin, act, alive, done, action):
        """The train-phase decision + step of every env as ONE call per step: step(t, epsilon) is cn_sarl_sample_step —
        alive &= ~done (the previous step's episode ends; zero `done` before an episode's first step), then cn_sarl_select ->
        cn_sarl_explore (mask = alive) -> cn_sarl_transform -> cn_step — with row t of the caller's histories (traj [B, T, H, D]
        float32; rew / dmin [T, B] float64; info [T, B] uint8; act [T, B] int32: the chosen action index) as outputs, addresses
        precomputed.  For a few envs a streamed loop of these calls is two launches per step (include/crowdnav_amd.h); on that
        route the kernels skip an env whose episode is over (its rows of the histories are not written any more)."""
        B, T, H, D = traj.shape
        if B != self.B or H != self.H:
            raise ValueError('traj is [%d, T, %d, D]; the engine holds %d envs x %d humans' % (B, H, self.B, self.H))
        specs = ((traj, torch.float32, (B, T, H, D)), (act, torch.int32, (T, B)), (rew, torch.float64, (T, B)),
                 (dmin, torch.float64, (T, B)), (info, torch.uint8, (T, B)), (alive, torch.uint8, (B,)), (done, torch.uint8, (B,)),
                 (action, torch.float64, (B, 2)))
        for t_, dt, shape in specs:  # raw addresses go to the C ABI below: every tensor on the engine's device, dense, as declared
            # (info may live in PINNED host memory instead: the kernels only write it — posted stores over the host link — and a
            # caller that streams steps can watch the episode-end codes arrive without a device synchronisation)
            # (round 6, later: so may the reward / min-distance / action histories — written before the step's info code on the
            # two-launch route; on the other routes a kernel READS the action row back: correct over the host link, only slower)
            if not self._dense(t_, dt, shape, pinned_ok=any(t_ is w for w in (info, rew, dmin, act))):
                raise ValueError('sarl_sampler: expected a contiguous %s %s tensor on %s, got %s %s on %s (contiguous: %s)'
                                 % (dt, shape, self.device, t_.dtype, tuple(t_.shape), t_.device, t_.is_contiguous()))
        # the closure owns the tensors its addresses point into, but only a WEAK reference to the engine: stored on the engine or on
        # a rollout object it would otherwise form a cycle, and cn_destroy (a stream synchronize + hipFree) would run whenever the
        # cyclic collector gets to it — e.g. in the middle of somebody's timed region (bench.py closes its engines explicitly)
        keep = (traj, rew, info, dmin, act, alive, done, action)
        alive_engine = weakref.ref(self)
        lib, h, V = self._lib, self._h, C.c_void_p
        p_traj, p_rew, p_inf, p_dmn, p_act = traj.data_ptr(), rew.data_ptr(), info.data_ptr(), dmin.data_ptr(), act.data_ptr()
        p_alive, p_done, p_action = V(alive.data_ptr()), V(done.data_ptr()), V(action.data_ptr())
        sort = int(self.sarl['model'] == 'lstm_rl')
        stride = T * H * D

        def step(t, epsilon):
            eng = alive_engine()
            if eng is None or eng._h is not h or not h.value:
                raise RuntimeError('sarl_sampler: the engine has been closed')
            check(lib.cn_sarl_sample_step(h, epsilon, p_alive, V(p_act + 4 * B * t), p_action, V(p_traj + 4 * H * D * t), stride, sort,
                                          V(p_rew + 8 * B * t), p_done, V(p_inf + B * t), V(p_dmn + 8 * B * t)))
        step.keep = keep  # the tensors live as long as the step function does
        return step

    def sarl_values(self, states, out=None):
        """V(state) of joint states the caller holds (cn_sarl_values): float32 [n, H, 13] rows as sarl_transform / the sampler
        write them -> float32 [n], under the weights of the last sarl_set_weights.  One launch on the narrow tiles; the engine's
        env state is not touched.  What target_model(next_states) is to Explorer.update_memory's TD targets."""
        n = int(states.shape[0])
        if not self._dense(states, torch.float32, (n, self.H, 13)):
            raise ValueError('sarl_values: expected a contiguous float32 [n, %d, 13] tensor on %s' % (self.H, self.device))
        if out is None:
            out = self._new((n,), torch.float32)
        check(self._lib.cn_sarl_values(self._h, _ptr(states), n, _ptr(out)))
        return out

    def sarl_state_values(self, state8, theta=None, sort_humans=False, out=None):
        """V(state) of joint states the caller holds in the env layout (cn_sarl_state_values): state8 float64 [n, A, 8] — get_state()'s
        rows, a rollout trace's, lookahead()'s final_state8; any leading axes [..., A, 8] are flattened — and theta float64 [n] (or the
        same leading axes), the robot heading, required for a unicycle robot and ignored otherwise -> float32 [n], under the weights
        of the last sarl_set_weights.  The rows are sarl_transform's (sort_humans as there; False = env order).  Any n >= 1, through
        the engine's own network kernels in passes of num_envs x n_actions; the engine's env state is not touched, the buffers
        sarl_export reads may be overwritten.  Contiguous float64 tensors on the engine's device are read in place; anything else is
        copied and the call synchronises."""
        shape = tuple(getattr(state8, 'shape', np.shape(state8)))
        if len(shape) < 3 or shape[-2:] != (self.A, 8):
            raise ValueError('sarl_state_values: state8 must be [n, %d, 8] (or [..., %d, 8]), got %s' % (self.A, self.A, shape))
        n = int(np.prod(shape[:-2], dtype=np.int64))
        tshape = None
        if theta is not None:
            tshape = tuple(getattr(theta, 'shape', np.shape(theta)))
            if int(np.prod(tshape, dtype=np.int64)) != n or (len(tshape) != 1 and tshape != shape[:-2]):
                raise ValueError('sarl_state_values: theta must be [%d] or %s, got %s' % (n, shape[:-2], tshape))
        if out is None:
            out = self._new((n,), torch.float32)
        elif not self._dense(out, torch.float32, (n,)):
            raise ValueError('sarl_state_values: out must be a contiguous float32 [%d] tensor on %s' % (n, self.device))
        s, temporary_s = self._borrow(state8, torch.float64, shape)
        th, temporary_th = self._borrow(theta, torch.float64, tshape)
        check(self._lib.cn_sarl_state_values(self._h, _ptr(s), _ptr(th), n, int(bool(sort_humans)), _ptr(out)))
        self._release(temporary_s, temporary_th)
        return out
