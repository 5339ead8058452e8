"""target_model(next states) for the TD targets of Explorer.update_memory (crowd_nav/utils/explorer.py:113-116), and the
per-model parameter table that this forward and the RL sampler's weight upload share."""
import logging
import os
import weakref

import torch

from .. import _lib
from ..engine import BatchedCrowdSim


class ParamTable(object):
    """Where the parameters of ONE model object live, walked once per model: model.parameters() visits every submodule (twice
    per sampled episode it was ~0.09 ms of host time) and state_dict() builds 22 detached views (another ~0.09 ms).  `slots` are
    (module, name) pairs, `names` the state_dict names in the same order, `by_name` the Parameter objects the walk found — the
    optimizer updates those tensors in place, and a model that moves or reloads keeps its Parameter objects."""

    def __init__(self):
        self._model = None  # weak reference to the model the table describes
        self.slots, self.names, self.by_name = [], [], {}

    def of(self, model):
        if self._model is None or self._model() is not model:
            walk = [(m, k, (prefix + '.' if prefix else '') + k) for prefix, m in model.named_modules()
                    for k, p in m._parameters.items() if p is not None]
            self._model = weakref.ref(model)
            self.slots, self.names = [(m, k) for m, k, _ in walk], [n for _, _, n in walk]
            self.by_name = {n: m._parameters[k] for m, k, n in walk}
        return self

    def live(self):
        """The Parameter objects looked up afresh: a replaced or moved one changes every key that is built from them."""
        return [m._parameters[k] for m, k in self.slots]


class TdTargets(object):
    """The target network's forward on a sampled episode's next states, flat.  In this order: cn_sarl_values on an engine of its
    own (_on_engine), the forward replayed from a hipGraph, the framework's eager forward."""

    def __init__(self):
        self.params = ParamTable()  # of the target model
        self.graph = None           # dict(key, x, y, graph): the captured forward on a fixed number of rows
        self.graph_failed = False   # a capture failed once: eager from then on
        self.kernel_off = False     # the library refused cn_sarl_values once: the framework's forward from then on
        self.engine = None          # dict(model, envs, H, eng, sig): the engine that only holds the target's weights

    def drop_graph(self):
        self.graph = None

    def values(self, model, nxt, policy=None, sampling_config=None):
        """policy: the robot's (its net_cfg, action space and engine_kwargs describe the network); sampling_config: the keyword
        arguments the RL sampling engine was built from, None while there is none — no sampling engine, no cn_sarl_values.
        On a GPU the framework's forward — some 35 tiny kernels for a few dozen rows: launch-bound — is replayed from a hipGraph
        captured on a fixed number of rows (the rows beyond the call's hold earlier, finite inputs and are not read back).
        CROWDNAV_AMD_TD_GRAPH=0: always eager."""
        live = self.params.of(model).live()
        x = nxt.to(live[0].device)
        v = self._on_engine(model, live, x, policy, sampling_config)
        if v is not None:
            return v
        n = int(x.shape[0])
        if not x.is_cuda or n == 0 or self.graph_failed or os.environ.get('CROWDNAV_AMD_TD_GRAPH', '1') == '0':
            return model(x).reshape(-1)
        g = self.graph
        # the graph replays reads of the parameters' STORAGE: a model whose parameters moved (.to(), .half(), load_state_dict(
        # assign=True), another module at a recycled id) must be captured again, not replayed on the old weights
        key = (id(model), tuple(x.shape[1:]), x.dtype, tuple(p.data_ptr() for p in live), model.training)
        if g is None or g['key'] != key or g['x'].shape[0] < n:
            rows = max(128, 2 * n if g is not None and g['key'] == key else n)
            try:
                sx = torch.zeros((rows,) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side), torch.no_grad():
                    for _ in range(2):
                        model(sx)
                torch.cuda.current_stream().wait_stream(side)
                graph = torch.cuda.CUDAGraph()
                with torch.no_grad(), torch.cuda.graph(graph):
                    sy = model(sx)
                g = self.graph = dict(key=key, x=sx, y=sy, graph=graph)
            except Exception as exc:  # noqa: BLE001 - e.g. a layer whose library call cannot be captured: run eagerly from now on
                logging.warning('TD-target forward: graph capture failed (%s); running eagerly', exc)
                self.graph, self.graph_failed = None, True
                return model(x).reshape(-1)
        g['x'][:n].copy_(x)
        g['graph'].replay()
        return g['y'][:n].reshape(-1)  # (a view of the graph's output: consumed before the next replay — update_memory converts it at once)

    def _on_engine(self, model, live, x, policy, sampling_config):
        """The target network's forward by the library's own network kernel (cn_sarl_values: ONE launch on the narrow tiles, the
        rows read where they lie) on an engine that only holds the target's weights — uploaded again whenever a parameter's
        version counter or address moved (update_target_model's in-place copy bumps the versions).  None: not this configuration
        (another policy, occupancy maps, CPU, CROWDNAV_AMD_TD_KERNEL=0) — the caller runs the framework's forward."""
        cfg = getattr(policy, 'net_cfg', None)
        if (cfg is None or not x.is_cuda or x.dim() != 3 or x.shape[2] != 13 or x.dtype != torch.float32 or x.shape[0] == 0
                or cfg.get('model', 'sarl') not in ('sarl', 'lstm_rl') or cfg.get('with_om') or cfg.get('interaction_dims')
                or self.kernel_off or os.environ.get('CROWDNAV_AMD_TD_KERNEL', '1') == '0'
                or type(model) is not type(getattr(policy, 'model', None)) or sampling_config is None):
            return None
        n, H = int(x.shape[0]), int(x.shape[1])
        K = len(policy.action_space)
        envs = 2
        while envs * K < n:
            envs *= 2
        if envs > 8:  # (more rows than the narrow tiles take — one workgroup per CU: this call's forward is the framework's)
            return None
        sig = tuple((p.data_ptr(), p._version) for p in live)
        cached = self.engine
        try:
            if cached is None or cached['model']() is not model or cached['envs'] < envs or cached['H'] != H:
                base = dict(sampling_config)  # the same crowd, robot, widths
                if base['num_humans'] != H:
                    return None
                base['num_envs'] = envs
                eng = BatchedCrowdSim(**base)
                eng.sarl_configure(**policy.engine_kwargs())
                cached = self.engine = dict(model=weakref.ref(model), envs=envs, H=H, eng=eng, sig=None)
            if cached['sig'] != sig:
                cached['eng'].sarl_set_weights(dict(zip(self.params.names, live)))
                cached['sig'] = sig
            return cached['eng'].sarl_values(x.contiguous())
        except _lib.CrowdNavAmdError as exc:  # e.g. CN_ERR_UNSUPPORTED for widths / sizes off the narrow tiles
            logging.info('TD targets: cn_sarl_values not available here (%s); using the framework forward', exc)
            self.kernel_off = True
            return None
