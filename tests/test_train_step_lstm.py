"""The device SGD step for lstm_rl.ValueNetwork1 (cn_train_step on a CN_MODEL_LSTM_RL trainer) on the MI355X against the
reference's arithmetic.

Metric and rule are those of test_train_step.py (lstm_step_reference.py holds them): torch float64 on the CPU is the truth, torch
float32 on the GPU the comparator; per parameter tensor the error of the MOMENTUM BUFFER after the step,
max|buf - buf64| / max(max|buf64|, 1e-6 G), pooled over the cases of one (fixture, H); required E_kernel <= max(8 E_torch,
2^-20), the loss likewise, and the parameters equal to p - lr buf in float32 bit for bit.  Float32 torch's own pooled error on
these fixtures is 2e-6 ... 1.3e-4 and the same for every tensor (the rounding of v - y dominates it), so the ratio means
something on all twelve.  One tensor is judged absolutely: at H = 1 nothing multiplies W_hh (h_0 = 0), its gradient is exactly
zero and the kernel's change of that buffer stays below 2^-20 G.  CROWDNAV_AMD_SGD_REPORT=1 (or =<file>) writes the tables to
profiles/sgd_step_parity.json under keys prefixed lstm/."""
import logging

import numpy as np
import pytest
import torch

import lstm_step_reference as ref
import sgd_step_reference as sarl_ref

pytestmark = pytest.mark.gpu
FACTOR, FLOOR = ref.FACTOR, ref.FLOOR
DEV = 'cuda:0'


class Kernel(object):
    """The handle plus device copies of one fixture's ring at one crowd size (either network: `family` is its reference module)."""

    def __init__(self, P, S, V, family=ref):
        from crowdnav_amd import train as cn_train
        self.P, self.names = P, family.NAMES
        self.model = family.network(P, torch.float32, DEV)
        self.params = [p.data for p in self.model.parameters()]
        self.bufs = [torch.zeros_like(p) for p in self.params]
        make = cn_train.LstmTrainStep if family is ref else cn_train.SarlTrainStep
        self.step = make(cn_train.module_net_config(self.model), S.shape[1], 128, 0)
        self.step.bind(self.params, self.bufs)
        self.states, self.values = torch.from_numpy(S).to(DEV), torch.from_numpy(V).to(DEV)
        self.loss = torch.zeros((), dtype=torch.float64, device=DEV)

    def set(self, bufs=None):
        for k, p, b in zip(self.names, self.params, self.bufs):
            p.copy_(torch.from_numpy(np.asarray(self.P[k], dtype=np.float32)))
            b.zero_() if bufs is None else b.copy_(torch.from_numpy(np.asarray(bufs[k], dtype=np.float32)))
        self.loss.zero_()

    def run(self, index, n, lr=0.01, mom=0.9, states=None, values=None):
        idx = None if index is None else torch.as_tensor(index, dtype=torch.int64).to(DEV)
        self.step.step(self.states if states is None else states, self.values if values is None else values, idx, n, lr, mom,
                       self.loss)
        torch.cuda.synchronize()

    def get(self):
        return ({k: p.cpu().numpy() for k, p in zip(self.names, self.params)},
                {k: b.cpu().numpy() for k, b in zip(self.names, self.bufs)}, self.loss.item())


@pytest.mark.parametrize('fixture', ref.FIXTURES)
@pytest.mark.parametrize('H', [1, 3, 5, 8])
def test_one_step_against_the_reference_arithmetic(fixture, H):
    """n = 16 and 17: one full tile, and a full tile plus a tile with a single valid row."""
    P, S, V = ref.load(fixture, H)
    K = Kernel(P, S, V)
    lr, mom = 0.01, 0.9
    other = np.random.RandomState(999).permutation(len(S))[:100]
    _, warm, _, _ = ref.torch_steps(P, [(S[other], V[other])], lr, mom, torch.float32, DEV)  # non-zero starting buffers
    warm = {k: v.astype(np.float32) for k, v in warm.items()}
    E_t, E_k, L_t, L_k, absolute = {}, {}, 0.0, 0.0, {}
    for start in (None, warm):
        for n in (100, 37, 17, 16, 1):
            for seed in range(8):
                idx = np.random.RandomState(1000 * n + seed).permutation(len(S))[:n]
                batch = [(S[idx], V[idx])]
                _, b64, l64, g64 = ref.torch_steps(P, batch, lr, mom, torch.float64, 'cpu', start)
                _, b32, l32, _ = ref.torch_steps(P, batch, lr, mom, torch.float32, DEV, start)
                K.set(bufs=start)
                K.run(idx, n, lr, mom)
                pk, bk, lk = K.get()
                et, G = ref.errors(b32, b64, g64)
                ek, _ = ref.errors(bk, b64, g64)
                ref.pool(E_t, et)
                ref.pool(E_k, ek)
                L_t, L_k = max(L_t, abs(l32 - l64) / abs(l64)), max(L_k, abs(lk - l64) / abs(l64))
                for k in ref.NAMES:
                    # p - lr * buf in float32 from the kernel's own buffer, bit for bit
                    assert np.array_equal(pk[k], P[k] - np.float32(lr) * bk[k]), (k, n, seed)
                    if ref.zero_gradient(k, H):
                        assert not g64[k].any()
                        carried = np.float32(mom) * start[k] if start is not None else np.zeros_like(bk[k])
                        change = np.abs(bk[k].astype(np.float64) - carried.astype(np.float64)).max()
                        ref.pool(absolute, {k: change / G})
    where = '%s H=%d' % (fixture, H)
    table, bad = ref.check_pooled(E_t, E_k, H, where)
    print('%-28s loss: E_torch %.3e E_kernel %.3e; zero-gradient tensors, largest |change| / G: %s' % (where, L_t, L_k, absolute))
    ref.report('lstm/one_step/' + where, dict(tensors=table, loss=dict(E_torch=L_t, E_kernel=L_k),
                                              zero_gradient_change_over_G=absolute))
    assert not bad, bad
    assert all(v < FLOOR for v in absolute.values()), absolute
    assert L_k <= max(FACTOR * L_t, FLOOR), (L_t, L_k)


@pytest.mark.parametrize('fixture', ref.FIXTURES)
def test_twenty_consecutive_steps(fixture):
    """Momentum 0.9, lr 0.01, a fresh index set per step, H = 5; the same metric on the buffers after the last step, pooled
    over four seeds."""
    P, S, V = ref.load(fixture, 5)
    K = Kernel(P, S, V)
    E_t, E_k = {}, {}
    for seed in range(4):
        rng = np.random.RandomState(50 + seed)
        sets = [rng.permutation(len(S))[:100] for _ in range(20)]
        batches = [(S[i], V[i]) for i in sets]
        _, b64, _, g64 = ref.torch_steps(P, batches, 0.01, 0.9, torch.float64)
        _, b32, _, _ = ref.torch_steps(P, batches, 0.01, 0.9, torch.float32, DEV)
        K.set()
        for i in sets:
            K.run(i, 100)
        _, bk, _ = K.get()
        ref.pool(E_t, ref.errors(b32, b64, g64)[0])
        ref.pool(E_k, ref.errors(bk, b64, g64)[0])
    table, bad = ref.check_pooled(E_t, E_k, 5, fixture + ' 20 steps')
    ref.report('lstm/twenty_steps/' + fixture, dict(tensors=table))
    assert not bad, bad


@pytest.mark.parametrize('fixture,H,n', [('rl_lstm_rl.npz', 5, 100), ('rl_lstm_rl_om.npz', 8, 37), ('rl_lstm_rl_om.npz', 3, 1)])
def test_the_same_two_steps_twice_give_the_same_bits(fixture, H, n):
    P, S, V = ref.load(fixture, H)
    K = Kernel(P, S, V)
    idx = np.random.RandomState(3).permutation(len(S))[:n]
    out = []
    for _ in range(2):
        K.set()
        K.run(idx, n)
        K.run(idx[::-1].copy(), n)  # a second step on non-zero buffers
        out.append(([p.clone() for p in K.params], [b.clone() for b in K.bufs], K.loss.clone()))
    for a, b in zip(out[0][0] + out[0][1] + [out[0][2]], out[1][0] + out[1][1] + [out[1][2]]):
        assert torch.equal(a, b)
    assert float(out[0][2]) > 0


def test_rows_are_read_where_they_lie():
    P, S, V = ref.load('rl_lstm_rl_om.npz', 5)
    K = Kernel(P, S, V)
    n = 100
    perm = np.random.RandomState(5).permutation(len(S))
    K.set()
    K.run(perm[:n], n)                                            # index into the ring
    ring = K.get()
    K.set()
    gathered = torch.from_numpy(S[perm[:n]]).to(DEV), torch.from_numpy(V[perm[:n]]).to(DEV)
    K.run(None, n, states=gathered[0], values=gathered[1])        # index == NULL on the gathered copy
    copy = K.get()
    for k in ref.NAMES:
        assert np.array_equal(ring[0][k], copy[0][k]) and np.array_equal(ring[1][k], copy[1][k]), k
        assert np.abs(ring[1][k]).max() > 0
    assert ring[2] == copy[2]


def test_a_captured_step_replays_to_the_bits_of_the_eager_call():
    P, S, V = ref.load('rl_lstm_rl.npz', 5)
    K = Kernel(P, S, V)
    idx = torch.from_numpy(np.random.RandomState(9).permutation(len(S))[:100]).to(DEV)
    K.set()
    K.step.step(K.states, K.values, idx, 100, 0.01, 0.9, K.loss)  # eager (and the handle's first step: it allocates)
    torch.cuda.synchronize()
    eager = K.get()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        K.step.step(K.states, K.values, idx, 100, 0.01, 0.9, K.loss)
    K.set()  # capturing ran nothing; start from the same state
    graph.replay()
    torch.cuda.synchronize()
    replay = K.get()
    for k in ref.NAMES:
        assert np.array_equal(eager[0][k], replay[0][k]) and np.array_equal(eager[1][k], replay[1][k]), k
    assert eager[2] == replay[2] and eager[2] > 0


def _trainer(monkeypatch, switch, model, S, V, batch_size=100):
    from crowdnav_amd.compat.trainer import DeviceReplayMemory, Trainer
    monkeypatch.setenv('CROWDNAV_AMD_SGD_KERNEL', switch)
    memory = DeviceReplayMemory(1000, DEV)
    memory.push_batch(torch.from_numpy(S), torch.from_numpy(V))
    trainer = Trainer(model, memory, torch.device(DEV), batch_size)
    trainer.set_learning_rate(0.01)
    return trainer


@pytest.mark.parametrize('fixture', ref.FIXTURES)
def test_trainer_end_to_end(fixture, monkeypatch):
    from crowdnav_amd import train as cn_train
    P, S, V = ref.load(fixture, 5)
    torch.manual_seed(21)
    on = _trainer(monkeypatch, '1', ref.network(P, torch.float32, DEV), S, V)
    off = _trainer(monkeypatch, '0', ref.network(P, torch.float32, DEV), S, V)

    # optimize_batch(1): the loss a switch-off Trainer returns on the same index set
    drawn = []
    draw = on._draw_batches
    monkeypatch.setattr(on, '_draw_batches', lambda count: (drawn.append(i.clone()) or i for i in draw(count)))
    loss_on = on.optimize_batch(1)
    assert len(drawn) == 1 and drawn[0].numel() == 100 and drawn[0].unique().numel() == 100
    idx = drawn[0]
    monkeypatch.setattr(off.memory, 'batches', lambda batch_size, limit=None: iter(
        [(off.memory.states.index_select(0, idx), off.memory.values.index_select(0, idx))]))
    loss_off = off.optimize_batch(1)
    monkeypatch.undo()
    i = idx.cpu().numpy()
    _, _, l64, _ = ref.torch_steps(P, [(S[i], V[i])], 0.01, 0.9, torch.float64)
    e_on, e_off = abs(loss_on - l64) / abs(l64), abs(loss_off - l64) / abs(l64)
    print('%s optimize_batch(1): float64 %.9e kernel %.9e (%.2e) torch %.9e (%.2e)' % (fixture, l64, loss_on, e_on, loss_off, e_off))
    assert e_on <= max(FACTOR * e_off, FLOOR)

    # it is the LSTM kernel that ran, on the optimizer's own momentum buffers
    kstep = on._kstep
    assert isinstance(kstep, cn_train.LstmTrainStep) and kstep.steps == 1 and off._kstep is None
    params = list(on.model.parameters())
    assert len(params) == 12
    for p, bound in zip(params, kstep._keep[1]):
        assert on.optimizer.state[p]['momentum_buffer'] is bound
    assert all(float(b.abs().max()) > 0 for b in kstep._keep[1])
    epoch = on.model._cn_weights_epoch
    many_on, many_off = on.optimize_batch(20), off.optimize_batch(20)
    assert on.model._cn_weights_epoch == epoch + 20 and kstep.steps == 21
    epochs_on, epochs_off = on.optimize_epoch(2), off.optimize_epoch(2)
    per_epoch = -(-len(S) // 100)
    assert kstep.steps == 21 + 2 * per_epoch and on.model._cn_weights_epoch == epoch + 20 + 2 * per_epoch
    assert np.isfinite([many_on, many_off, epochs_on, epochs_off]).all()
    assert all(torch.isfinite(p).all() for p in params)
    ref.report('lstm/trainer/' + fixture, dict(optimize_batch_1=dict(float64=l64, kernel=loss_on, torch=loss_off),
                                               optimize_batch_20=dict(kernel=many_on, torch=many_off),
                                               optimize_epoch_2=dict(kernel=epochs_on, torch=epochs_off)))

    # falling back to torch mid-run continues the same optimizer state: a torch step moves the very buffers the kernel wrote
    before = [b.clone() for b in kstep._keep[1]]
    on._kernel_off = True
    on.optimize_batch(1)
    assert kstep.steps == 21 + 2 * per_epoch
    assert all(on.optimizer.state[p]['momentum_buffer'] is b for p, b in zip(params, kstep._keep[1]))
    assert any(not torch.equal(a, b) for a, b in zip(before, kstep._keep[1]))

    # a new learning rate is a new optimizer: zero buffers, bound again
    on._kernel_off = False
    on.set_learning_rate(0.001)
    on.optimize_batch(1)
    assert kstep.steps == 22 + 2 * per_epoch
    assert all(on.optimizer.state[p]['momentum_buffer'] is b for p, b in zip(params, kstep._keep[1]))


def test_a_value_network_2_logs_the_fallback_once_and_trains_on_todays_path(monkeypatch, caplog):
    from crowdnav_amd.compat.lstm_rl import ValueNetwork2
    torch.manual_seed(2)
    _, S, V = ref.load('rl_lstm_rl.npz', 5)
    model = ValueNetwork2(13, 6, [150, 100, 100, 50], [150, 100, 100, 1], 50).to(DEV)
    trainer = _trainer(monkeypatch, '1', model, S, V)
    start = [p.detach().clone() for p in model.parameters()]
    with caplog.at_level(logging.WARNING):
        losses = [trainer.optimize_batch(2), trainer.optimize_batch(2), trainer.optimize_epoch(1)]
    logged = [r for r in caplog.records if 'CROWDNAV_AMD_SGD_KERNEL' in r.getMessage()]
    assert len(logged) == 1 and 'lstm_rl.ValueNetwork2' in logged[0].getMessage()
    assert trainer._kstep is None and trainer._kernel_off
    assert np.isfinite(losses).all() and any(not torch.equal(a, b) for a, b in zip(start, model.parameters()))


def test_a_sarl_and_an_lstm_handle_step_side_by_side():
    """Both trainers alive in one process, their single steps interleaved; each under the rule, pooled over four index sets."""
    cases = [(ref, ref.load('rl_lstm_rl.npz', 5)), (sarl_ref, sarl_ref.load('rl_sarl_plain.npz', 5))]
    kernels = [Kernel(P, S, V, family) for family, (P, S, V) in cases]
    rows = min(len(S) for _, (_, S, _) in cases)
    E_t, E_k, L_t, L_k = [{}, {}], [{}, {}], [0.0, 0.0], [0.0, 0.0]
    for seed in range(4):
        idx = np.random.RandomState(12 + seed).permutation(rows)[:100]
        for K in kernels:
            K.set()
        for K in kernels:
            K.run(idx, 100)
        for m, (K, (family, (P, S, V))) in enumerate(zip(kernels, cases)):
            batch = [(S[idx], V[idx])]
            _, b64, l64, g64 = family.torch_steps(P, batch, 0.01, 0.9, torch.float64)
            _, b32, l32, _ = family.torch_steps(P, batch, 0.01, 0.9, torch.float32, DEV)
            _, bk, lk = K.get()
            G = max(np.abs(g).max() for g in g64.values())
            scale = {k: max(np.abs(b64[k]).max(), 1e-6 * G) for k in family.NAMES}
            ref.pool(E_t[m], {k: np.abs(b32[k] - b64[k]).max() / scale[k] for k in family.NAMES})
            ref.pool(E_k[m], {k: np.abs(bk[k].astype(np.float64) - b64[k]).max() / scale[k] for k in family.NAMES})
            L_t[m], L_k[m] = max(L_t[m], abs(l32 - l64) / abs(l64)), max(L_k[m], abs(lk - l64) / abs(l64))
            if family is sarl_ref:  # its zero-gradient tensor (the softmax is shift-invariant) is judged absolutely
                assert np.abs(bk['attention.4.bias']).max() < FLOOR * G
    for m, (family, _) in enumerate(cases):
        for k in family.NAMES:
            if k != 'attention.4.bias':
                assert E_k[m][k] <= max(FACTOR * E_t[m][k], FLOOR), (family.__name__, k, E_t[m][k], E_k[m][k])
        assert L_k[m] <= max(FACTOR * L_t[m], FLOOR), (family.__name__, L_t[m], L_k[m])
        assert kernels[m].step.steps == 4
