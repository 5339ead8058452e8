"""The device SGD step for lstm_rl.ValueNetwork1 (cn_trainer_create with CN_MODEL_LSTM_RL) as far as a machine without a GPU
can see it: what the library accepts and refuses before a device is touched, the arithmetic the kernel is written from against
torch autograd (float64: equal; float32 in the kernel's summation order: within the rule the GPU test applies), and that the
switch changes nothing where the kernel path does not apply."""
import ctypes as C
import functools
import re

import numpy as np
import pytest
import torch

import lstm_step_reference as ref
import sgd_step_reference
from support import built  # noqa: F401  (built: module fixture)

_cpu_trainer = functools.partial(sgd_step_reference.cpu_trainer, ref)


def _create(built, num_humans=5, max_batch=100, input_dim=13, **kw):
    from crowdnav_amd.train import lstm_net_config
    cfg = lstm_net_config(input_dim, **kw)
    h = C.c_void_p()
    rc = built.load().cn_trainer_create(C.byref(cfg), num_humans, max_batch, 0, C.byref(h))
    return rc, built.load().cn_last_error().decode(), h


def test_the_library_accepts_value_network_1_and_validates_its_steps_without_a_device(built):
    lib = built.load()
    assert C.sizeof(built.CnSarlConfig) == 112 and built.ABI_VERSION == 12 and lib.cn_abi_version() == 12
    fake = (C.c_void_p * 12)(*[0x1000] * 12)  # never dereferenced: every call below is refused first
    args = lambda n: (fake, fake, C.c_void_p(0x1000), C.c_void_p(0x1000), 1000, None, n, 0.01, 0.9, None)  # noqa: E731
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
        holed = (C.c_void_p * 12)(*([0x1000] * 11 + [None]))  # 12 entries are checked: the last one is NULL
        assert lib.cn_train_step(h, holed, fake, *args(10)[2:]) == built.CN_ERR_INVALID
        assert 'entry 11' in lib.cn_last_error().decode()
        n = C.c_int64(-1)
        assert lib.cn_trainer_steps(h, C.byref(n)) == built.CN_OK and n.value == 0
        assert lib.cn_trainer_destroy(h) == built.CN_OK


def test_what_the_library_refuses_names_the_field_and_the_value(built):
    for kw, field, value in ((dict(interaction_dims=(150, 100, 100, 50)), 'interaction_dims', '150'),  # ValueNetwork2
                             (dict(hidden=64), 'mlp1_dims', '64'),
                             (dict(mlp_dims=(150, 100, 64, 1)), 'mlp3_dims', '64'),
                             (dict(input_dim=13 + 64), 'input width', '77'),
                             (dict(num_humans=9), 'num_humans', '9'),
                             (dict(max_batch=129), 'max_batch', '129')):
        rc, msg, h = _create(built, **kw)
        assert rc == built.CN_ERR_UNSUPPORTED and not h.value, kw
        assert field in msg and re.search(r'\b%s\b' % value, msg), (kw, msg)


def test_module_net_config_reads_a_value_network_1():
    from crowdnav_amd.compat.lstm_rl import ValueNetwork1, ValueNetwork2
    from crowdnav_amd.train import CN_MODEL_LSTM_RL, module_net_config
    cfg = module_net_config(ValueNetwork1(61, 6, [150, 100, 100, 1], 50))
    assert cfg.model == CN_MODEL_LSTM_RL and tuple(cfg.mlp1_dims) == (50, 1) and tuple(cfg.mlp3_dims) == (150, 100, 100, 1)
    assert tuple(cfg.interaction_dims) == (0, 0, 0, 0) and 13 + cfg.with_om * cfg.cell_num ** 2 * cfg.om_channel_size == 61
    cfg = module_net_config(ValueNetwork2(13, 6, [150, 100, 100, 50], [150, 100, 100, 1], 50))
    assert tuple(cfg.interaction_dims) == (150, 100, 100, 50)


def _batches(S, V, n, count=10):
    rng = np.random.RandomState(7 + n)
    return [(S[i], V[i]) for i in (rng.permutation(len(S))[:n] for _ in range(count))]


@pytest.mark.parametrize('fixture', ref.FIXTURES)
@pytest.mark.parametrize('n', [100, 37, 1])
def test_float64_emulation_of_the_kernel_formulas_equals_autograd(fixture, n):
    """Pins the arithmetic the kernel is written from (gate order i f g o, c_t = f c_{t-1} + i g, h_t = o tanh c_t, the
    backward through time, both LSTM biases taking the sum of dGates, buf = m buf + g, p -= lr buf): parameters, momentum
    buffers and loss after 1 and after 10 steps, momentum 0.9."""
    P, S, V = ref.load(fixture)
    batches = _batches(S, V, n)
    for steps in (1, 10):
        tp, tb, tl, _ = ref.torch_steps(P, batches[:steps], 0.01, 0.9, torch.float64)
        p = {k: v.astype(np.float64) for k, v in P.items()}
        b = {k: np.zeros_like(v) for k, v in p.items()}
        for x, y in batches[:steps]:
            p, b, loss = ref.manual_step(p, x, y, 0.01, 0.9, b, np.float64)
        assert abs(loss - tl) <= 1e-9 * abs(tl)
        for k in ref.NAMES:
            assert np.abs(p[k] - tp[k]).max() <= 1e-9 * np.abs(tp[k]).max(), (k, steps)
            assert np.abs(b[k] - tb[k]).max() <= 1e-9 * np.abs(tb[k]).max(), (k, steps)
    assert torch.get_default_dtype() == torch.float32  # the float64 truth put torch's default back


@pytest.mark.parametrize('fixture', ref.FIXTURES)
@pytest.mark.parametrize('H', [1, 5])
def test_float32_emulation_in_the_kernels_order_meets_the_gpu_rule(fixture, H):
    """The rule of test_train_step_lstm.py with the numpy restatement in float32 (16-row partial sums) in the kernel's place and
    CPU torch float32 as the comparator: it can be met before a GPU is involved."""
    P, S, V = ref.load(fixture, H)
    E_t, E_m, L_t, L_m, absolute = {}, {}, 0.0, 0.0, 0.0
    zero = {k: np.zeros_like(v) for k, v in P.items()}
    for n in (100, 37, 1):
        for x, y in _batches(S, V, n, 4):
            _, b64, l64, g64 = ref.torch_steps(P, [(x, y)], 0.01, 0.9, torch.float64)
            _, b32, l32, _ = ref.torch_steps(P, [(x, y)], 0.01, 0.9, torch.float32)
            _, bm, lm = ref.manual_step(P, x, y, 0.01, 0.9, zero, np.float32)
            et, G = ref.errors(b32, b64, g64)
            ref.pool(E_t, et)
            ref.pool(E_m, ref.errors(bm, b64, g64)[0])
            L_t, L_m = max(L_t, abs(l32 - l64) / abs(l64)), max(L_m, abs(lm - l64) / abs(l64))
            if H == 1:
                assert not g64['lstm.weight_hh_l0'].any()  # h_0 = 0: an exactly zero gradient
                absolute = max(absolute, np.abs(bm['lstm.weight_hh_l0']).max() / G)
    _, bad = ref.check_pooled(E_t, E_m, H, '%s H=%d (numpy float32)' % (fixture, H))
    print('loss: E_torch %.3e E_numpy %.3e' % (L_t, L_m))
    assert not bad, bad
    assert absolute < ref.FLOOR
    assert L_m <= max(ref.FACTOR * L_t, ref.FLOOR), (L_t, L_m)


def test_switch_on_without_a_gpu_model_is_todays_path_bit_for_bit(monkeypatch):
    P, S, V = ref.load('rl_lstm_rl.npz')
    on, on_losses = _cpu_trainer(monkeypatch, '1', P, S, V)
    off, off_losses = _cpu_trainer(monkeypatch, '0', P, S, V)
    assert on._kernel_on is True and off._kernel_on is False  # the switch was read ...
    assert on._kstep is None and not on._kernel_off           # ... and neither taken nor refused: nothing here is on a GPU
    assert on_losses == off_losses
    for a, b in zip(on.model.parameters(), off.model.parameters()):
        assert torch.equal(a, b)
        assert torch.equal(on.optimizer.state[a]['momentum_buffer'], off.optimizer.state[b]['momentum_buffer'])
