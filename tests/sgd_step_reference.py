"""Shared by test_train_step_host.py / test_train_step.py: the fixtures' replay memories at other crowd sizes, torch's SGD
step as the reference Trainer takes it, and a numpy restatement of the formulas the device step (cn_train_step) is written
from — masked softmax, mean-pool, ReLU masks from the pre-activations, 16-row partial sums for the weight gradients."""
import os

import numpy as np
import torch

from conftest import GOLDEN, ROOT

FIXTURES = ('rl_sarl_plain.npz', 'rl_sarl_om.npz')
NAMES = ['%s.%d.%s' % (m, i, w) for m, idx in (('mlp1', (0, 2)), ('mlp2', (0, 2)), ('attention', (0, 2, 4)), ('mlp3', (0, 2, 4, 6)))
         for i in idx for w in ('weight', 'bias')]


def load(fixture, H=5, names=NAMES):
    """(params {name: float32 array}, states [rows, H, D], values [rows]); H = 1, 3: the first humans; 8: rows 0-4 then 0-2."""
    g = np.load(os.path.join(GOLDEN, fixture))
    P = {k[6:]: g[k] for k in g.files if k.startswith('param_')}
    assert list(P) == names, list(P)
    S, V = g['memory_states'], g['memory_values']
    S = np.concatenate([S, S[:, :H - 5]], 1) if H > 5 else S[:, :H]
    return P, np.ascontiguousarray(S), np.ascontiguousarray(V)


OTHER_WIDTHS = (14, 16, 17, 22, 40, 63)  # occupancy-map settings other than the shipped one: 1 x 1 x 1 ... 5 x 5 x 2, the widest below 64


def fresh_case(D, H, rows=64):
    """A freshly initialised ValueNetwork(D, ...) under a fixed torch seed, random float32 rows [rows, H, D] and values [rows]."""
    from crowdnav_amd.compat.sarl import ValueNetwork
    torch.manual_seed(400 + D)
    net = ValueNetwork(D, 6, [150, 100], [100, 50], [150, 100, 100, 1], [100, 100, 1], True, 1.0, 4)
    P = {k: v.detach().numpy().copy() for k, v in net.state_dict().items()}
    assert list(P) == NAMES and P['mlp1.0.weight'].shape == (150, D)
    rs = np.random.RandomState(10 * D + H)
    S = rs.uniform(-1.0, 1.0, (rows, H, D)).astype(np.float32)
    S[:, :, 13:] *= rs.uniform(size=(rows, H, D - 13)) < 0.3  # map columns: mostly zeros, as occupancy maps are
    V = rs.uniform(-0.5, 1.0, rows).astype(np.float32)
    return P, S, V


def network(P, dtype, device='cpu'):
    from crowdnav_amd.compat.sarl import ValueNetwork
    d = P['mlp1.0.weight'].shape[1]
    m = ValueNetwork(d, 6, [150, 100], [100, 50], [150, 100, 100, 1], [100, 100, 1], True, 1.0, 4).to(dtype)
    m.load_state_dict({k: torch.from_numpy(v).to(dtype) for k, v in P.items()})
    return m.to(device)


def torch_steps(P, batches, lr, mom, dtype, device='cpu', buf0=None):
    """The reference Trainer's step (trainer.py:56-66) on each (x, y) of batches.  Returns (params, buffers, last loss,
    last gradients) as float64 numpy dicts."""
    m = network(P, dtype, device)
    opt = torch.optim.SGD(m.parameters(), lr=lr, momentum=mom)
    if buf0 is not None:
        for (k, p) in m.named_parameters():
            opt.state[p]['momentum_buffer'] = torch.from_numpy(np.asarray(buf0[k])).to(dtype).to(device).clone()
    crit = torch.nn.MSELoss()
    for x, y in batches:
        opt.zero_grad()
        loss = crit(m(torch.from_numpy(x).to(dtype).to(device)), torch.from_numpy(y).to(dtype).to(device).reshape(-1, 1))
        loss.backward()
        opt.step()
    out = lambda f: {k: f(p).detach().double().cpu().numpy() for k, p in m.named_parameters()}  # noqa: E731
    return out(lambda p: p), out(lambda p: opt.state[p]['momentum_buffer']), float(loss.detach().double()), out(lambda p: p.grad)


def manual_step(P, x, y, lr, mom, buf, dt):
    """One step in dtype dt by the device step's formulas.  Returns (params, buffers, loss)."""
    P = {k: v.astype(dt) for k, v in P.items()}
    n, H, d = x.shape
    x, y = x.astype(dt), y.astype(dt).reshape(-1, 1)
    lin = lambda a, p: a @ P[p + '.weight'].T + P[p + '.bias']  # noqa: E731
    X = x.reshape(-1, d)
    a1 = lin(X, 'mlp1.0'); h1 = np.maximum(a1, 0); a2 = lin(h1, 'mlp1.2'); h2 = np.maximum(a2, 0)  # noqa: E702
    b1 = lin(h2, 'mlp2.0'); g1 = np.maximum(b1, 0); feat = lin(g1, 'mlp2.2')  # noqa: E702
    glob = h2.reshape(n, H, -1).mean(1, keepdims=True).repeat(H, 1).reshape(n * H, -1)
    ai = np.concatenate([h2, glob], 1)
    c1 = lin(ai, 'attention.0'); k1 = np.maximum(c1, 0); c2 = lin(k1, 'attention.2'); k2 = np.maximum(c2, 0)  # noqa: E702
    s = lin(k2, 'attention.4').reshape(n, H)
    e = np.exp(s) * (s != 0).astype(dt)  # the reference's masked softmax (sarl.py:52-53); the mask is a constant
    Z = e.sum(1, keepdims=True)
    w = e / Z
    F = feat.reshape(n, H, -1)
    j = np.concatenate([x[:, 0, :6], (w[:, :, None] * F).sum(1)], 1)
    d1 = lin(j, 'mlp3.0'); q1 = np.maximum(d1, 0); d2 = lin(q1, 'mlp3.2'); q2 = np.maximum(d2, 0)  # noqa: E702
    d3 = lin(q2, 'mlp3.4'); q3 = np.maximum(d3, 0); v = lin(q3, 'mlp3.6')  # noqa: E702
    loss = ((v - y) ** 2).mean(dtype=dt)
    G = {}

    def back(dout, ain, p):
        W = P[p + '.weight']
        gw, gb = np.zeros_like(W), np.zeros_like(P[p + '.bias'])
        for r in range(0, len(dout), 16):
            gw += dout[r:r + 16].T @ ain[r:r + 16]
            gb += dout[r:r + 16].sum(0)
        G[p + '.weight'], G[p + '.bias'] = gw, gb
        return dout @ W

    t = back((dt(2.0) / dt(n) * (v - y)).astype(dt), q3, 'mlp3.6') * (d3 > 0)
    t = back(t, q2, 'mlp3.4') * (d2 > 0)
    t = back(t, q1, 'mlp3.2') * (d1 > 0)
    dwf = back(t, j, 'mlp3.0')[:, 6:]
    dF = w[:, :, None] * dwf[:, None, :]
    dw = (F * dwf[:, None, :]).sum(2)
    ds = (dw / Z - (dw * e).sum(1, keepdims=True) / Z ** 2) * e
    t = back(ds.reshape(-1, 1), k2, 'attention.4') * (c2 > 0)
    t = back(t, k1, 'attention.2') * (c1 > 0)
    dai = back(t, ai, 'attention.0')
    dh2 = dai[:, :100] + (dai[:, 100:].reshape(n, H, -1).sum(1, keepdims=True) / H).repeat(H, 1).reshape(n * H, -1)
    t = back(dF.reshape(n * H, -1), g1, 'mlp2.2') * (b1 > 0)
    dh2 = dh2 + back(t, h2, 'mlp2.0')
    t = back(dh2 * (a2 > 0), h1, 'mlp1.2') * (a1 > 0)
    back(t, X, 'mlp1.0')
    newP, newB = {}, {}
    for k in P:
        newB[k] = (dt(mom) * buf[k].astype(dt) + G[k]).astype(dt)
        newP[k] = (P[k] - dt(lr) * newB[k]).astype(dt)
    return newP, newB, float(loss)


def report(key, value):
    """With CROWDNAV_AMD_SGD_REPORT set, merge {key: value} into profiles/sgd_step_parity.json (or the file the variable names)."""
    import json
    where = os.environ.get('CROWDNAV_AMD_SGD_REPORT')
    if not where:
        return
    path = os.path.join(ROOT, 'profiles', 'sgd_step_parity.json') if where in ('1', 'true', 'yes') else where
    data = {}
    if os.path.exists(path):
        with open(path) as f:
            data = json.load(f)
    data[key] = value
    with open(path, 'w') as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write('\n')


def pool(into, new):
    for k, v in new.items():
        into[k] = max(into.get(k, 0.0), float(v))


def cpu_trainer(ref, monkeypatch, switch, P, S, V):
    """compat's Trainer on the CPU over `ref`'s network (this module or lstm_step_reference), and the losses of a batch and an
    epoch under CROWDNAV_AMD_SGD_KERNEL = switch."""
    from crowdnav_amd.compat.trainer import ReplayMemory, Trainer
    monkeypatch.setenv('CROWDNAV_AMD_SGD_KERNEL', switch)
    torch.manual_seed(11)
    memory = ReplayMemory(1000)
    for s, v in zip(S, V):
        memory.push((torch.from_numpy(s), torch.from_numpy(v.reshape(1))))
    trainer = Trainer(ref.network(P, torch.float32), memory, torch.device('cpu'), 100)
    trainer.set_learning_rate(0.01)
    return trainer, [trainer.optimize_batch(3), trainer.optimize_epoch(1)]
