"""The device SGD step (cn_train_step) on the MI355X against the reference's arithmetic.

Three ways from the same parameters and momentum buffers: torch float64 on the CPU (the truth), torch float32 on the GPU,
eager (the reference Trainer's own step), the kernel.  Metric per parameter tensor k: the error of the MOMENTUM BUFFER after
the step, max|buf - buf64| / max(max|buf64|, 1e-6 G), G = the largest gradient entry of the whole network in that case,
pooled (maximum) over the cases of one (fixture, H).  Required: E_kernel[k] <= max(8 E_torch[k], 2^-20).  Two float32
evaluations that differ only in summation order scatter around the float64 value alike (a float32 emulation with 16-row
partial sums came out at most 4.7 x torch's pooled error on these cases); 2^-20 is 8 float32 ulps of the tensor's scale, below
which a ratio of two rounding errors says nothing.  Tensors whose true gradient is zero — attention.4.bias at every H (the
softmax is shift-invariant), all of attention.* at H = 1 (the single weight is the constant 1) — are judged absolutely: the
kernel's buffer change stays below 2^-20 G.  The buffer and not the parameter: at these learning rates an update is often
below one ulp of the weight.  CROWDNAV_AMD_SGD_REPORT=1 (or =<file>) writes the tables to profiles/sgd_step_parity.json."""
import logging

import numpy as np
import pytest
import torch

import sgd_step_reference as ref
from sgd_step_reference import pool

pytestmark = pytest.mark.gpu
FACTOR, FLOOR = 8.0, 2.0 ** -20
DEV = 'cuda:0'


def zero_gradient(name, H):
    return name == 'attention.4.bias' or (H == 1 and name.startswith('attention.'))


class Kernel(object):
    """The handle plus device copies of one fixture's ring at one crowd size."""

    def __init__(self, P, S, V):
        from crowdnav_amd import train as cn_train
        self.P = P
        self.model = ref.network(P, torch.float32, DEV)
        self.params = [p.data for p in self.model.parameters()]
        self.bufs = [torch.zeros_like(p) for p in self.params]
        self.step = cn_train.SarlTrainStep(cn_train.module_net_config(self.model), S.shape[1], 128, 0)
        self.step.bind(self.params, self.bufs)
        self.states, self.values = torch.from_numpy(S).to(DEV), torch.from_numpy(V).to(DEV)
        self.loss = torch.zeros((), dtype=torch.float64, device=DEV)

    def set(self, params=None, bufs=None):
        for k, p, b in zip(ref.NAMES, self.params, self.bufs):
            p.copy_(torch.from_numpy(np.asarray((params or self.P)[k], dtype=np.float32)))
            b.zero_() if bufs is None else b.copy_(torch.from_numpy(np.asarray(bufs[k], dtype=np.float32)))
        self.loss.zero_()

    def run(self, index, n, lr=0.01, mom=0.9, states=None, values=None):
        idx = None if index is None else torch.as_tensor(index, dtype=torch.int64).to(DEV)
        self.step.step(self.states if states is None else states, self.values if values is None else values, idx, n, lr, mom,
                       self.loss)
        torch.cuda.synchronize()

    def get(self):
        return ({k: p.cpu().numpy() for k, p in zip(ref.NAMES, self.params)},
                {k: b.cpu().numpy() for k, b in zip(ref.NAMES, self.bufs)}, self.loss.item())


def errors(buf, buf64, grad64):
    G = max(np.abs(g).max() for g in grad64.values())
    return {k: np.abs(buf[k].astype(np.float64) - buf64[k]).max() / max(np.abs(buf64[k]).max(), 1e-6 * G) for k in ref.NAMES}, G


def check_pooled(E_torch, E_kernel, H, where):
    table, bad = {}, []
    for k in ref.NAMES:
        ratio = E_kernel[k] / E_torch[k] if E_torch[k] > 0 else float('inf')
        table[k] = dict(E_torch=E_torch[k], E_kernel=E_kernel[k], ratio=ratio, judged='absolute' if zero_gradient(k, H) else 'ratio')
        print('%-28s %-20s E_torch %.3e  E_kernel %.3e  ratio %6.2f  %s' % (where, k, E_torch[k], E_kernel[k], ratio, table[k]['judged']))
        if not zero_gradient(k, H) and not E_kernel[k] <= max(FACTOR * E_torch[k], FLOOR):
            bad.append((k, E_torch[k], E_kernel[k]))
    return table, bad


@pytest.mark.parametrize('fixture', ref.FIXTURES)
@pytest.mark.parametrize('H', [1, 3, 5, 8])
def test_one_step_against_the_reference_arithmetic(fixture, H):
    P, S, V = ref.load(fixture, H)
    K = Kernel(P, S, V)
    lr, mom = 0.01, 0.9
    other = np.random.RandomState(999).permutation(len(S))[:100]
    _, warm, _, _ = ref.torch_steps(P, [(S[other], V[other])], lr, mom, torch.float32, DEV)  # non-zero starting buffers
    warm = {k: v.astype(np.float32) for k, v in warm.items()}
    E_t, E_k, L_t, L_k, absolute = {}, {}, 0.0, 0.0, {}
    for start in (None, warm):
        for n in (100, 37, 1):
            for seed in range(8):
                idx = np.random.RandomState(1000 * n + seed).permutation(len(S))[:n]
                batch = [(S[idx], V[idx])]
                _, b64, l64, g64 = ref.torch_steps(P, batch, lr, mom, torch.float64, 'cpu', start)
                _, b32, l32, _ = ref.torch_steps(P, batch, lr, mom, torch.float32, DEV, start)
                K.set(bufs=start)
                K.run(idx, n, lr, mom)
                pk, bk, lk = K.get()
                et, G = errors(b32, b64, g64)
                ek, _ = errors(bk, b64, g64)
                pool(E_t, et)
                pool(E_k, ek)
                L_t, L_k = max(L_t, abs(l32 - l64) / abs(l64)), max(L_k, abs(lk - l64) / abs(l64))
                for k in ref.NAMES:
                    # p - lr * buf in float32 from the kernel's own buffer, bit for bit
                    assert np.array_equal(pk[k], P[k] - np.float32(lr) * bk[k]), (k, n, seed)
                    if zero_gradient(k, H):
                        carried = np.float32(mom) * start[k] if start is not None else np.zeros_like(bk[k])
                        change = np.abs(bk[k].astype(np.float64) - carried.astype(np.float64)).max()
                        pool(absolute, {k: change / G})
    where = '%s H=%d' % (fixture, H)
    table, bad = check_pooled(E_t, E_k, H, where)
    print('%-28s loss: E_torch %.3e E_kernel %.3e; zero-gradient tensors, largest |change| / G: %s' % (where, L_t, L_k, absolute))
    ref.report('one_step/' + where, dict(tensors=table, loss=dict(E_torch=L_t, E_kernel=L_k), zero_gradient_change_over_G=absolute))
    assert not bad, bad
    assert all(v < FLOOR for v in absolute.values()), absolute
    assert L_k <= max(FACTOR * L_t, FLOOR), (L_t, L_k)


@pytest.mark.parametrize('D', ref.OTHER_WIDTHS)
def test_one_step_at_other_input_widths(D):
    """train_tile_kernel / train_update_kernel at input widths other than 13 and 61: the same metric, bound and report as
    test_one_step_against_the_reference_arithmetic, pooled per (D, H) over n in {37, 1}, zero and warm starting buffers."""
    lr, mom = 0.01, 0.9
    for H in (2, 5):
        P, S, V = ref.fresh_case(D, H)
        K = Kernel(P, S, V)
        other = np.random.RandomState(999).permutation(len(S))[:40]
        _, warm, _, _ = ref.torch_steps(P, [(S[other], V[other])], lr, mom, torch.float32, DEV)
        warm = {k: v.astype(np.float32) for k, v in warm.items()}
        E_t, E_k, L_t, L_k, absolute = {}, {}, 0.0, 0.0, {}
        for start in (None, warm):
            for n in (37, 1):
                for seed in range(4):
                    idx = np.random.RandomState(1000 * n + seed).permutation(len(S))[:n]
                    batch = [(S[idx], V[idx])]
                    _, b64, l64, g64 = ref.torch_steps(P, batch, lr, mom, torch.float64, 'cpu', start)
                    _, b32, l32, _ = ref.torch_steps(P, batch, lr, mom, torch.float32, DEV, start)
                    K.set(bufs=start)
                    K.run(idx, n, lr, mom)
                    pk, bk, lk = K.get()
                    et, G = errors(b32, b64, g64)
                    ek, _ = errors(bk, b64, g64)
                    pool(E_t, et)
                    pool(E_k, ek)
                    L_t, L_k = max(L_t, abs(l32 - l64) / abs(l64)), max(L_k, abs(lk - l64) / abs(l64))
                    for k in ref.NAMES:
                        assert np.array_equal(pk[k], P[k] - np.float32(lr) * bk[k]), (k, n, seed)
                        if zero_gradient(k, H):
                            carried = np.float32(mom) * start[k] if start is not None else np.zeros_like(bk[k])
                            pool(absolute, {k: np.abs(bk[k].astype(np.float64) - carried.astype(np.float64)).max() / G})
        where = 'fresh D=%d H=%d' % (D, H)
        table, bad = check_pooled(E_t, E_k, H, where)
        print('%-28s loss: E_torch %.3e E_kernel %.3e; zero-gradient tensors, largest |change| / G: %s' % (where, L_t, L_k, absolute))
        ref.report('one_step/' + where, dict(tensors=table, loss=dict(E_torch=L_t, E_kernel=L_k), zero_gradient_change_over_G=absolute))
        assert not bad, bad
        assert all(v < FLOOR for v in absolute.values()), absolute
        assert L_k <= max(FACTOR * L_t, FLOOR), (L_t, L_k)
        K.step.close()


def test_an_input_wider_than_64_is_refused():
    """cell_num 5 with 3 channels is 88 inputs: cn_trainer_create refuses it by name, it does not truncate."""
    from crowdnav_amd import CrowdNavAmdError, _lib
    from crowdnav_amd import train as cn_train
    with pytest.raises(CrowdNavAmdError) as ei:
        cn_train.SarlTrainStep(cn_train.sarl_net_config(88, cell_num=5), 5, 128, 0)
    assert ei.value.status == _lib.CN_ERR_UNSUPPORTED
    assert 'input width 88' in str(ei.value) and 'exceeds 64' in str(ei.value)
    cn_train.SarlTrainStep(cn_train.sarl_net_config(63, cell_num=5), 5, 128, 0).close()  # 5 x 5 x 2 is served


@pytest.mark.parametrize('fixture', ref.FIXTURES)
def test_twenty_consecutive_steps(fixture):
    """Momentum 0.9, lr 0.01, a fresh index set per step, H = 5; the same metric on the buffers after the last step, pooled
    over four seeds.  A zero-gradient tensor's buffer is then a sum of twenty such changes weighted 0.9^t (<= 10 of them)."""
    P, S, V = ref.load(fixture, 5)
    K = Kernel(P, S, V)
    E_t, E_k, absolute = {}, {}, {}
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
        et, G = errors(b32, b64, g64)
        ek, _ = errors(bk, b64, g64)
        pool(E_t, et)
        pool(E_k, ek)
        pool(absolute, {'attention.4.bias': np.abs(bk['attention.4.bias']).max() / G})
    table, bad = check_pooled(E_t, E_k, 5, fixture + ' 20 steps')
    ref.report('twenty_steps/' + fixture, dict(tensors=table, zero_gradient_buffer_over_G=absolute))
    assert not bad, bad
    assert absolute['attention.4.bias'] < 10 * FLOOR, absolute


@pytest.mark.parametrize('fixture,H,n', [('rl_sarl_plain.npz', 5, 100), ('rl_sarl_om.npz', 8, 37), ('rl_sarl_om.npz', 3, 1)])
def test_the_same_step_twice_gives_the_same_bits(fixture, H, n):
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


def test_rows_are_read_where_they_lie():
    P, S, V = ref.load('rl_sarl_om.npz', 5)
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
    assert ring[2] == copy[2]
    # the same rows in another order: the same loss up to summation order (the 8 x rule, pooled over the orders tried)
    batch = [(S[perm[:n]], V[perm[:n]])]
    _, _, l64, _ = ref.torch_steps(P, batch, 0.01, 0.9, torch.float64)
    L_t, L_k = 0.0, 0.0
    for seed in range(8):
        order = np.random.RandomState(seed).permutation(n)
        _, _, l32, _ = ref.torch_steps(P, [(batch[0][0][order], batch[0][1][order])], 0.01, 0.9, torch.float32, DEV)
        K.set()
        K.run(perm[:n][order], n)
        L_t, L_k = max(L_t, abs(l32 - l64) / abs(l64)), max(L_k, abs(K.get()[2] - l64) / abs(l64))
    print('permuted index: loss E_torch %.3e E_kernel %.3e' % (L_t, L_k))
    assert L_k <= max(FACTOR * L_t, FLOOR), (L_t, L_k)


def test_a_captured_step_replays_to_the_bits_of_the_eager_call():
    P, S, V = ref.load('rl_sarl_plain.npz', 5)
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


def _trainer(monkeypatch, switch, P, S, V, batch_size=100):
    from crowdnav_amd.compat.trainer import DeviceReplayMemory, Trainer
    monkeypatch.setenv('CROWDNAV_AMD_SGD_KERNEL', switch)
    memory = DeviceReplayMemory(1000, DEV)
    memory.push_batch(torch.from_numpy(S), torch.from_numpy(V))
    trainer = Trainer(ref.network(P, torch.float32, DEV), memory, torch.device(DEV), batch_size)
    trainer.set_learning_rate(0.01)
    return trainer


@pytest.mark.parametrize('fixture', ref.FIXTURES)
def test_trainer_end_to_end(fixture, monkeypatch):
    P, S, V = ref.load(fixture, 5)
    torch.manual_seed(21)
    on, off = _trainer(monkeypatch, '1', P, S, V), _trainer(monkeypatch, '0', P, S, V)

    # optimize_batch(1): the loss a switch-off Trainer returns on the same index set
    drawn = []
    draw = on._draw_batches
    monkeypatch.setattr(on, '_draw_batches', lambda count: (drawn.append(i.clone()) or i for i in draw(count)))
    loss_on = on.optimize_batch(1)
    assert len(drawn) == 1 and drawn[0].numel() == 100 and drawn[0].unique().numel() == 100  # no duplicates inside a batch
    assert int(drawn[0].min()) >= 0 and int(drawn[0].max()) < len(S)
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

    # it is the kernel that ran, on the optimizer's own momentum buffers
    kstep = on._kstep
    assert kstep is not None and kstep.steps == 1 and off._kstep is None
    params = list(on.model.parameters())
    for p, bound in zip(params, kstep._keep[1]):
        assert on.optimizer.state[p]['momentum_buffer'] is bound
    assert all(float(b.abs().max()) > 0 for k, b in zip(ref.NAMES, kstep._keep[1]) if not zero_gradient(k, 5))
    epoch = on.model._cn_weights_epoch
    many_on, many_off = on.optimize_batch(20), off.optimize_batch(20)
    assert on.model._cn_weights_epoch == epoch + 20 and kstep.steps == 21
    epochs_on, epochs_off = on.optimize_epoch(2), off.optimize_epoch(2)
    per_epoch = -(-len(S) // 100)
    assert kstep.steps == 21 + 2 * per_epoch and on.model._cn_weights_epoch == epoch + 20 + 2 * per_epoch
    assert np.isfinite([many_on, many_off, epochs_on, epochs_off]).all()
    assert all(torch.isfinite(p).all() for p in params)
    ref.report('trainer/' + fixture, dict(optimize_batch_1=dict(float64=l64, kernel=loss_on, torch=loss_off),
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


def test_a_cadrl_model_logs_the_fallback_once_and_trains_on_todays_path(monkeypatch, caplog):
    from crowdnav_amd.compat.cadrl import ValueNetwork
    from crowdnav_amd.compat.trainer import DeviceReplayMemory, Trainer
    monkeypatch.setenv('CROWDNAV_AMD_SGD_KERNEL', '1')
    torch.manual_seed(2)
    P, S, V = ref.load('rl_sarl_plain.npz', 1)
    memory = DeviceReplayMemory(1000, DEV)
    memory.push_batch(torch.from_numpy(S[:, 0]), torch.from_numpy(V))  # CADRL's rows: one (robot, human) pair, [13]
    model = ValueNetwork(13, [150, 100, 100, 1]).to(DEV)
    trainer = Trainer(model, memory, torch.device(DEV), 100)
    trainer.set_learning_rate(0.01)
    start = [p.detach().clone() for p in model.parameters()]
    with caplog.at_level(logging.WARNING):
        losses = [trainer.optimize_batch(2), trainer.optimize_batch(2), trainer.optimize_epoch(1)]
    logged = [r for r in caplog.records if 'CROWDNAV_AMD_SGD_KERNEL' in r.getMessage()]
    assert len(logged) == 1 and 'cadrl.ValueNetwork' in logged[0].getMessage()
    assert trainer._kstep is None and trainer._kernel_off
    assert np.isfinite(losses).all() and any(not torch.equal(a, b) for a, b in zip(start, model.parameters()))


def test_a_batch_size_the_library_refuses_falls_back_once(monkeypatch, caplog):
    P, S, V = ref.load('rl_sarl_plain.npz', 5)
    trainer = _trainer(monkeypatch, '1', P, S, V, batch_size=150)
    with caplog.at_level(logging.WARNING):
        losses = [trainer.optimize_batch(1), trainer.optimize_batch(1)]
    logged = [r for r in caplog.records if 'CROWDNAV_AMD_SGD_KERNEL' in r.getMessage()]
    assert len(logged) == 1 and 'max_batch' in logged[0].getMessage()
    assert trainer._kstep is None and np.isfinite(losses).all()
