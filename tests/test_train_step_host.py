"""The device SGD step (cn_trainer_* / cn_train_step, CROWDNAV_AMD_SGD_KERNEL) as far as a machine without a GPU can see it:
the ABI surface, argument validation before the device is touched, the arithmetic the kernels are written from against
torch autograd in float64, and that the switch changes nothing where the kernel path does not apply."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

import sgd_step_reference as ref
from conftest import ROOT
from support import built  # noqa: F401  (built: module fixture)

NEW_CALLS = ('cn_trainer_create', 'cn_trainer_destroy', 'cn_trainer_set_stream', 'cn_train_step', 'cn_trainer_steps')
_cpu_trainer = functools.partial(ref.cpu_trainer, ref)


def test_header_binding_and_library_agree_on_the_trainer_calls(built):
    text = open(os.path.join(ROOT, 'include', 'crowdnav_amd.h')).read()
    assert 'added after v12, no version bump' in text
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    lib = C.CDLL(built.LIB_PATH)
    for name in NEW_CALLS:
        assert re.search(r'\b%s\s*\(' % name, text), name
        assert name in built.SYMBOLS, name
        assert hasattr(lib, name), name
    assert built.ABI_VERSION == 12 and built.load().cn_abi_version() == 12
    assert C.sizeof(built.CnSarlConfig) == 112


def _create(built, num_humans=5, max_batch=100, **kw):
    from crowdnav_amd.train import sarl_net_config
    cfg = sarl_net_config(kw.pop('input_dim', 13), **kw)
    h = C.c_void_p()
    rc = built.load().cn_trainer_create(C.byref(cfg), num_humans, max_batch, 0, C.byref(h))
    return rc, built.load().cn_last_error().decode(), h


def test_validation_happens_before_the_device_is_touched(built):
    lib = built.load()
    rc, msg, _ = _create(built, model=1)  # CN_MODEL_CADRL
    assert rc == built.CN_ERR_UNSUPPORTED and 'model' in msg
    rc, msg, _ = _create(built, mlp1_dims=(160, 100))
    assert rc == built.CN_ERR_UNSUPPORTED and 'mlp1_dims' in msg and '160' in msg
    rc, msg, _ = _create(built, mlp3_dims=(150, 100, 64, 1))
    assert rc == built.CN_ERR_UNSUPPORTED and 'mlp3_dims' in msg
    rc, msg, _ = _create(built, with_global_state=False)
    assert rc == built.CN_ERR_UNSUPPORTED and 'with_global_state' in msg
    rc, msg, _ = _create(built, num_humans=9)
    assert rc == built.CN_ERR_UNSUPPORTED and 'num_humans' in msg
    rc, msg, _ = _create(built, max_batch=129)
    assert rc == built.CN_ERR_UNSUPPORTED and 'max_batch' in msg
    rc, msg, _ = _create(built, input_dim=13 + 64)
    assert rc == built.CN_ERR_UNSUPPORTED and 'input width' in msg
    assert lib.cn_trainer_create(None, 5, 100, 0, None) == built.CN_ERR_INVALID

    fake = (C.c_void_p * 22)(*[0x1000] * 22)  # never dereferenced: every call below is refused first
    args = lambda n: (fake, fake, C.c_void_p(0x1000), C.c_void_p(0x1000), 1000, None, n, 0.01, 0.9, None)  # noqa: E731
    assert lib.cn_train_step(None, *args(100)) == built.CN_ERR_INVALID and 'NULL trainer' in lib.cn_last_error().decode()
    assert lib.cn_trainer_set_stream(None, None) == built.CN_ERR_INVALID
    assert lib.cn_trainer_steps(None, None) == built.CN_ERR_INVALID
    assert lib.cn_trainer_destroy(None) == built.CN_OK

    for D in (13, 61):
        rc, msg, h = _create(built, input_dim=D)
        assert rc == built.CN_OK, msg
        assert lib.cn_train_step(h, *args(0)) == built.CN_ERR_INVALID
        assert re.search(r'\bn 0\b', lib.cn_last_error().decode())
        assert lib.cn_train_step(h, *args(101)) == built.CN_ERR_INVALID
        msg = lib.cn_last_error().decode()
        assert 'max_batch' in msg and '101' in msg
        assert lib.cn_train_step(h, None, fake, *args(10)[2:]) == built.CN_ERR_INVALID
        assert 'params_host_array' in lib.cn_last_error().decode()
        n = C.c_int64(-1)
        assert lib.cn_trainer_steps(h, C.byref(n)) == built.CN_OK and n.value == 0
        assert lib.cn_trainer_destroy(h) == built.CN_OK


@pytest.mark.parametrize('fixture', ref.FIXTURES)
@pytest.mark.parametrize('n', [100, 37, 1])
def test_float64_emulation_of_the_kernel_formulas_equals_autograd(fixture, n):
    """Pins the arithmetic the kernels are written from (masked softmax and its constant mask, mean-pool gradient / H, ReLU
    masks, buf = m buf + g, p -= lr buf): parameters and momentum buffers after 1 and after 10 steps, momentum 0.9."""
    P, S, V = ref.load(fixture)
    rng = np.random.RandomState(7 + n)
    batches = [(S[i], V[i]) for i in (rng.permutation(len(S))[:n] for _ in range(10))]
    for steps in (1, 10):
        tp, tb, tl, _ = ref.torch_steps(P, batches[:steps], 0.01, 0.9, torch.float64)
        p = {k: v.astype(np.float64) for k, v in P.items()}
        b = {k: np.zeros_like(v) for k, v in p.items()}
        for x, y in batches[:steps]:
            p, b, loss = ref.manual_step(p, x, y, 0.01, 0.9, b, np.float64)
        assert abs(loss - tl) <= 1e-9 * abs(tl)
        big = max(np.abs(v).max() for v in tb.values())
        for k in ref.NAMES:
            assert np.abs(p[k] - tp[k]).max() <= 1e-9 * np.abs(tp[k]).max(), (k, steps)
            # attention.4.bias has a zero true gradient (the softmax is shift-invariant): its scale gets the floor the GPU
            # test uses, 1e-6 of the network's largest buffer entry
            assert np.abs(b[k] - tb[k]).max() <= 1e-9 * max(np.abs(tb[k]).max(), 1e-6 * big), (k, steps)


@pytest.mark.parametrize('D', ref.OTHER_WIDTHS)
def test_float64_emulation_equals_autograd_at_other_input_widths(D, built):
    """The emulation takes the input width from the data: the same pin at the widths of other occupancy-map settings, H = 2 and 5,
    and cn_trainer_create serves each of them."""
    for H in (2, 5):
        P, S, V = ref.fresh_case(D, H)
        rng = np.random.RandomState(70 + D)
        batches = [(S[i], V[i]) for i in (rng.permutation(len(S))[:n] for n in (37, 1, 37))]
        tp, tb, tl, _ = ref.torch_steps(P, batches, 0.01, 0.9, torch.float64)
        p = {k: v.astype(np.float64) for k, v in P.items()}
        b = {k: np.zeros_like(v) for k, v in p.items()}
        for x, y in batches:
            p, b, loss = ref.manual_step(p, x, y, 0.01, 0.9, b, np.float64)
        assert abs(loss - tl) <= 1e-9 * abs(tl)
        big = max(np.abs(v).max() for v in tb.values())
        for k in ref.NAMES:
            assert np.abs(p[k] - tp[k]).max() <= 1e-9 * np.abs(tp[k]).max(), (k, H)
            assert np.abs(b[k] - tb[k]).max() <= 1e-9 * max(np.abs(tb[k]).max(), 1e-6 * big), (k, H)
    rc, msg, h = _create(built, input_dim=D)
    assert rc == built.CN_OK, msg
    assert built.load().cn_trainer_destroy(h) == built.CN_OK


def test_switch_on_without_a_gpu_model_is_todays_path_bit_for_bit(monkeypatch):
    P, S, V = ref.load('rl_sarl_plain.npz')
    on, on_losses = _cpu_trainer(monkeypatch, '1', P, S, V)
    off, off_losses = _cpu_trainer(monkeypatch, '0', P, S, V)
    assert on._kernel_on is True and off._kernel_on is False  # the switch was read ...
    assert on._kstep is None and not on._kernel_off           # ... and neither taken nor refused: nothing here is on a GPU
    assert on_losses == off_losses
    for a, b in zip(on.model.parameters(), off.model.parameters()):
        assert torch.equal(a, b)
    for a, b in zip(on.model.parameters(), off.model.parameters()):
        assert torch.equal(on.optimizer.state[a]['momentum_buffer'], off.optimizer.state[b]['momentum_buffer'])
