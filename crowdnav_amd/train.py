"""Device SGD step for sarl.ValueNetwork (cn_trainer_* / cn_train_step, include/crowdnav_amd.h): tensors in, data_ptr() out,
torch's current stream — the way BatchedCrowdSim binds its engine.  The parameters and momentum buffers stay the caller's
torch tensors; the handle holds only the scratch rows between its two kernels."""
import ctypes as C

import torch

from . import _lib
from ._lib import CnSarlConfig, CrowdNavAmdError, check

SHIPPED_DIMS = dict(mlp1_dims=(150, 100), mlp2_dims=(100, 50), attention_dims=(100, 100, 1), mlp3_dims=(150, 100, 100, 1))


def sarl_net_config(input_dim, with_global_state=True, cell_num=4, model=0, **dims):
    """cn_sarl_config of a value network for cn_trainer_create: layer widths (default: the shipped ones) and the input width
    as 13 + one occupancy-map channel block of input_dim - 13 columns."""
    d = dict(SHIPPED_DIMS, **dims)
    cfg = CnSarlConfig()
    cfg.model = int(model)
    cfg.with_global_state = int(bool(with_global_state))
    extra = int(input_dim) - 13
    if extra < 0:
        raise CrowdNavAmdError(_lib.CN_ERR_UNSUPPORTED, 'input width %d < 13' % input_dim)
    cfg.with_om = int(extra > 0)
    cells = int(cell_num) * int(cell_num)
    if extra > 0 and extra % cells == 0:
        cfg.cell_num, cfg.om_channel_size = int(cell_num), extra // cells
    else:  # the trainer only needs the product
        cfg.cell_num, cfg.om_channel_size = 1, max(extra, 1)
    for name in SHIPPED_DIMS:
        vals = tuple(int(v) for v in d[name])
        if len(vals) != len(SHIPPED_DIMS[name]):
            raise CrowdNavAmdError(_lib.CN_ERR_UNSUPPORTED, '%s has %d layers, the device SGD step is built for %d'
                                   % (name, len(vals), len(SHIPPED_DIMS[name])))
        setattr(cfg, name, (C.c_int32 * len(vals))(*vals))
    return cfg


def module_net_config(model):
    """cn_sarl_config read from a compat.sarl.ValueNetwork itself (layer shapes, with_global_state)."""
    import torch.nn as nn

    def widths(seq):
        return tuple(m.out_features for m in seq if isinstance(m, nn.Linear))

    return sarl_net_config(model.mlp1[0].in_features, with_global_state=model.with_global_state,
                           cell_num=getattr(model, 'cell_num', 4) or 4, mlp1_dims=widths(model.mlp1),
                           mlp2_dims=widths(model.mlp2), attention_dims=widths(model.attention), mlp3_dims=widths(model.mlp3))


class SarlTrainStep(object):
    """One handle per (network shape, crowd size, largest batch).  step() is two kernel launches on torch's current stream."""

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
        """The 22 parameter tensors (state_dict order) and their momentum buffers: float32, contiguous, on the device."""
        params, momentum = list(params), list(momentum)
        if len(params) != 22 or len(momentum) != 22:
            raise ValueError('sarl.ValueNetwork has 22 parameter tensors, got %d / %d' % (len(params), len(momentum)))
        for p, m in zip(params, momentum):
            if not (p.is_cuda and m.is_cuda and p.dtype == m.dtype == torch.float32 and p.is_contiguous()
                    and m.is_contiguous() and p.shape == m.shape):
                raise ValueError('parameters and momentum buffers must be contiguous float32 device tensors of equal shapes')
        self._keep = (params, momentum)
        self._ptrs = ((C.c_void_p * 22)(*[p.data_ptr() for p in params]), (C.c_void_p * 22)(*[m.data_ptr() for m in momentum]))

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
