"""Device SGD step for sarl.ValueNetwork and lstm_rl.ValueNetwork1 (cn_trainer_* / cn_train_step, include/crowdnav_amd.h):
tensors in, data_ptr() out, torch's current stream — the way BatchedCrowdSim binds its engine.  The parameters and momentum
buffers stay the caller's torch tensors; the handle holds only the scratch rows between its two kernels."""
import ctypes as C

import torch

from . import _lib
from ._lib import CnSarlConfig, CrowdNavAmdError, check

SHIPPED_DIMS = dict(mlp1_dims=(150, 100), mlp2_dims=(100, 50), attention_dims=(100, 100, 1), mlp3_dims=(150, 100, 100, 1))
CN_MODEL_SARL, CN_MODEL_LSTM_RL = 0, 2


def _set_input_width(cfg, input_dim, cell_num):
    """The input width as 13 + one occupancy-map channel block of input_dim - 13 columns."""
    extra = int(input_dim) - 13
    if extra < 0:
        raise CrowdNavAmdError(_lib.CN_ERR_UNSUPPORTED, 'input width %d < 13' % input_dim)
    cfg.with_om = int(extra > 0)
    cells = int(cell_num) * int(cell_num)
    if extra > 0 and extra % cells == 0:
        cfg.cell_num, cfg.om_channel_size = int(cell_num), extra // cells
    else:  # the trainer only needs the product
        cfg.cell_num, cfg.om_channel_size = 1, max(extra, 1)


def sarl_net_config(input_dim, with_global_state=True, cell_num=4, model=CN_MODEL_SARL, **dims):
    """cn_sarl_config of a value network for cn_trainer_create: layer widths (default: the shipped ones) and the input width."""
    d = dict(SHIPPED_DIMS, **dims)
    cfg = CnSarlConfig()
    cfg.model = int(model)
    cfg.with_global_state = int(bool(with_global_state))
    _set_input_width(cfg, input_dim, cell_num)
    for name in SHIPPED_DIMS:
        vals = tuple(int(v) for v in d[name])
        if len(vals) != len(SHIPPED_DIMS[name]):
            raise CrowdNavAmdError(_lib.CN_ERR_UNSUPPORTED, '%s has %d layers, the device SGD step is built for %d'
                                   % (name, len(vals), len(SHIPPED_DIMS[name])))
        setattr(cfg, name, (C.c_int32 * len(vals))(*vals))
    return cfg


def lstm_net_config(input_dim, hidden=50, mlp_dims=(150, 100, 100, 1), cell_num=4, interaction_dims=(0, 0, 0, 0)):
    """cn_sarl_config of an lstm_rl value network for cn_trainer_create, under compat.lstm_rl's convention: mlp1_dims =
    (hidden, 1), mlp3_dims = the head's widths, interaction_dims all zero (non-zero: ValueNetwork2, which the library refuses)."""
    cfg = CnSarlConfig()
    cfg.model = CN_MODEL_LSTM_RL
    _set_input_width(cfg, input_dim, cell_num)
    for name, vals, count in (('mlp1_dims', (hidden, 1), 2), ('mlp3_dims', mlp_dims, 4), ('interaction_dims', interaction_dims, 4)):
        vals = tuple(int(v) for v in vals)
        if len(vals) != count:
            raise CrowdNavAmdError(_lib.CN_ERR_UNSUPPORTED, '%s has %d entries, the device SGD step is built for %d'
                                   % (name, len(vals), count))
        setattr(cfg, name, (C.c_int32 * count)(*vals))
    return cfg


def module_net_config(model):
    """cn_sarl_config read from a compat.sarl.ValueNetwork (layer shapes, with_global_state) or a compat.lstm_rl.ValueNetwork1
    (input width, hidden width, head widths) itself."""
    import torch.nn as nn

    def widths(seq):
        return tuple(m.out_features for m in seq if isinstance(m, nn.Linear))

    if isinstance(getattr(model, 'lstm', None), nn.LSTM):
        pairwise = widths(model.mlp1) if hasattr(model, 'mlp1') else (0, 0, 0, 0)  # ValueNetwork2: the library names it
        return lstm_net_config(model.lstm.input_size if not hasattr(model, 'mlp1') else model.mlp1[0].in_features,
                               model.lstm.hidden_size, widths(model.mlp), cell_num=getattr(model, 'cell_num', 4) or 4,
                               interaction_dims=pairwise)
    return sarl_net_config(model.mlp1[0].in_features, with_global_state=model.with_global_state,
                           cell_num=getattr(model, 'cell_num', 4) or 4, mlp1_dims=widths(model.mlp1),
                           mlp2_dims=widths(model.mlp2), attention_dims=widths(model.attention), mlp3_dims=widths(model.mlp3))


class SarlTrainStep(object):
    """One handle per (network shape, crowd size, largest batch).  step() is two kernel launches on torch's current stream."""
    NETWORK, TENSORS = 'sarl.ValueNetwork', 22

    def __init__(self, net_config, num_humans, max_batch=128, device=0):
        self._lib = _lib.load()
        self._h = C.c_void_p()
        check(self._lib.cn_trainer_create(C.byref(net_config), int(num_humans), int(max_batch), int(device), C.byref(self._h)))
        self.num_humans, self.max_batch, self.device = int(num_humans), int(max_batch), int(device)
        self._ptrs = None

    def close(self):
        if getattr(self, '_h', None) is not None and self._h.value:
            self._lib.cn_trainer_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    @property
    def steps(self):
        """cn_train_step calls that launched their kernels."""
        n = C.c_int64()
        check(self._lib.cn_trainer_steps(self._h, C.byref(n)))
        return n.value

    def bind(self, params, momentum):
        """The network's parameter tensors (state_dict order: 22 of sarl.ValueNetwork, 12 of lstm_rl.ValueNetwork1) and their
        momentum buffers: float32, contiguous, on the device."""
        params, momentum = list(params), list(momentum)
        count = self.TENSORS
        if len(params) != count or len(momentum) != count:
            raise ValueError('%s has %d parameter tensors, got %d / %d' % (self.NETWORK, count, len(params), len(momentum)))
        for p, m in zip(params, momentum):
            if not (p.is_cuda and m.is_cuda and p.dtype == m.dtype == torch.float32 and p.is_contiguous()
                    and m.is_contiguous() and p.shape == m.shape):
                raise ValueError('parameters and momentum buffers must be contiguous float32 device tensors of equal shapes')
        self._keep = (params, momentum)
        self._ptrs = tuple((C.c_void_p * count)(*[t.data_ptr() for t in tensors]) for tensors in (params, momentum))

    def step(self, states, values, index, n, lr, momentum, loss_sum=None):
        """states [rows, H, D] / values [rows(, 1)] float32 device tensors read where they lie; index int64 [n] or None
        (rows 0..n-1); loss_sum: float64 device scalar the batch's MSE is added to."""
        if self._ptrs is None:
            raise ValueError('bind() the parameter and momentum tensors first')
        if not (states.is_cuda and states.dtype == torch.float32 and states.is_contiguous() and states.dim() == 3
                and states.shape[1] == self.num_humans):
            raise ValueError('states must be a contiguous float32 device tensor [rows, %d, D]' % self.num_humans)
        if not (values.is_cuda and values.dtype == torch.float32 and values.is_contiguous() and values.numel() == states.shape[0]):
            raise ValueError('values must be a contiguous float32 device tensor with one entry per row of states')
        if index is not None and not (index.is_cuda and index.dtype == torch.int64 and index.is_contiguous()
                                      and index.numel() >= n):
            raise ValueError('index must be a contiguous int64 device tensor of at least n entries')
        if loss_sum is not None and not (loss_sum.is_cuda and loss_sum.dtype == torch.float64):
            raise ValueError('loss_sum must be a float64 device tensor')
        check(self._lib.cn_trainer_set_stream(self._h, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        check(self._lib.cn_train_step(self._h, self._ptrs[0], self._ptrs[1], C.c_void_p(states.data_ptr()),
                                      C.c_void_p(values.data_ptr()), int(states.shape[0]),
                                      None if index is None else C.c_void_p(index.data_ptr()), int(n), float(lr),
                                      float(momentum), None if loss_sum is None else C.c_void_p(loss_sum.data_ptr())))


class LstmTrainStep(SarlTrainStep):
    """The same handle made from an lstm_net_config: bind() takes the 12 tensors of lstm_rl.ValueNetwork1 (mlp.{0,2,4,6}.{weight,
    bias}, lstm.weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0); step() is SarlTrainStep.step."""
    NETWORK, TENSORS = 'lstm_rl.ValueNetwork1', 12
