"""CN_PRECISION_F16X2, the host half: the split-f16 arithmetic sarl_f16_kernel is written from as a torch
emulation on the reference's SARL fixtures, and the ABI of the request word and of cn_sarl_network_route.

The emulation, for every linear layer y = W a + b with S = 2^11:
    ah = f16(a), al = f16((a - ah) S);  Wh = f16(W), Wl = f16((W - Wh) S)
    y = sum ah Wh + (sum al Wh + sum ah Wl) / S + b          (f32 sums; al Wl dropped)
with f16 subnormals flushed to zero (the pessimistic assumption about the hardware) and everything between the layers in f32.
Bounds as for the fp32 kernels (tests/test_sarl.py): network output and action values 1e-6, arg-max equal wherever the
reference's top two values are more than 4e-5 apart, which at least a quarter of each fixture's decisions are."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

FIXTURES = ['sarl_plain', 'sarl_om', 'sarl_unicycle', 'sarl_noquery_om', 'sarl_noquery_unicycle', 'sarl_h12', 'sarl_om_h12']
S = 2048.0
F16_MIN_NORMAL = 2.0 ** -14


def f16(x):
    """round to f16 (nearest even), subnormals flushed, back in f32"""
    h = x.to(torch.float16).to(torch.float32)
    return torch.where(h.abs() < F16_MIN_NORMAL, torch.zeros_like(h), h)


def split(x):
    hi = f16(x)
    return hi, f16((x - hi) * S)


def split_linear(a, W, b):
    ah, al = split(a)
    Wh, Wl = split(W)
    main = ah @ Wh.t()
    cross = al @ Wh.t() + ah @ Wl.t()
    return main + cross * (1.0 / S) + b


def split_forward(p, x):
    """sarl.ValueNetwork.forward (crowdnav_amd/compat/sarl.py) with split_linear for nn.Linear; p: the state_dict, x [n, h, d]"""
    n, h, d = x.shape

    def stack(name, idxs, a, last_relu):
        for i in idxs:
            a = split_linear(a, p['%s.%d.weight' % (name, i)], p['%s.%d.bias' % (name, i)])
            if i != idxs[-1] or last_relu:
                a = torch.relu(a)
        return a

    hidden = stack('mlp1', (0, 2), x.reshape(-1, d), True)
    feats = stack('mlp2', (0, 2), hidden, False)
    glob = hidden.view(n, h, -1).mean(1, keepdim=True).expand(n, h, hidden.shape[1])
    scores = stack('attention', (0, 2, 4), torch.cat([hidden, glob.reshape(-1, hidden.shape[1])], dim=1), False).view(n, h)
    e = torch.exp(scores) * (scores != 0).float()
    weights = (e / e.sum(dim=1, keepdim=True)).unsqueeze(2)
    weighted = (weights * feats.view(n, h, -1)).sum(dim=1)
    return stack('mlp3', (0, 2, 4, 6), torch.cat([x[:, 0, :6], weighted], dim=1), False)


@pytest.mark.parametrize('name', FIXTURES)
def test_split_f16_emulation_keeps_fp32_grade_values_on_the_reference_fixtures_cpu(name):
    g = load_golden(name + '.npz')
    p = {k[len('param_'):]: torch.from_numpy(v) for k, v in g.items() if k.startswith('param_')}
    x = torch.from_numpy(g['inputs'])
    n, k, h, d = x.shape
    V = split_forward(p, x.reshape(n * k, h, d)).reshape(n, k).numpy()
    err = np.abs(V - g['net_out']).max()
    print('%s: max |V - net_out| = %.3g' % (name, err))
    assert err <= 1e-6
    gamma_bar = 0.9 ** (0.25 * 1.0)  # gamma ^ (time_step * v_pref), multi_human_rl.py:51
    values = g['rewards'] + gamma_bar * V.astype(np.float64)
    assert np.abs(values - g['values']).max() <= 1e-6
    top2 = np.sort(g['values'], axis=1)[:, -2:]
    clear = (top2[:, 1] - top2[:, 0]) > 4e-5
    print('%s: clear %d / %d' % (name, clear.sum(), n))
    assert clear.sum() >= n // 4
    assert np.array_equal(values.argmax(axis=1)[clear], g['best'][clear])


def test_precision_word_and_network_route_abi():
    from crowdnav_amd import _lib
    assert C.sizeof(_lib.CnSarlConfig) == 112 and _lib.ABI_VERSION == 12
    # `precision` is the former `reserved` word: the last int32, behind constant_velocity_model
    assert _lib.CnSarlConfig.precision.offset == 104 == _lib.CnSarlConfig.constant_velocity_model.offset + 4
    assert _lib.CnSarlConfig.precision.size == 4
    assert not hasattr(_lib.CnSarlConfig, 'reserved')
    assert _lib.PRECISIONS == ('f32', 'f16x2')
    header = open(os.path.join(ROOT, 'include', 'crowdnav_amd.h')).read()
    assert re.search(r'int32_t precision;', header) and 'int32_t reserved;' not in header
    assert re.search(r'CN_PRECISION_F32 = 0, CN_PRECISION_F16X2 = 1', header)
    assert re.search(r'int cn_sarl_network_route\(cn_engine\* e, int\* route_host\);', header)
    names = re.findall(r'CN_SARL_ROUTE_([A-Z0-9_]+) = (\d+)', header)
    assert [n.lower() for n, _ in names] == list(_lib.SARL_ROUTES) and [int(v) for _, v in names] == list(range(len(names)))
    assert _lib.SARL_ROUTES[-1] == 'split_f16'
    assert _lib.SYMBOLS['cn_sarl_network_route'] == (C.c_int, [_lib._P, C.POINTER(C.c_int)])
    assert len(_lib.LAUNCH_COUNTERS) == 6
    lib = _lib.load()
    route = C.c_int(-1)
    assert lib.cn_sarl_network_route(None, C.byref(route)) == _lib.CN_ERR_INVALID  # NULL engine: refused before anything is read
    assert route.value == -1
