"""What the SARL attention suites (test_sarl_attention, test_sarl_f16) share: the torch mirror of every row's softmax weights and
the check of the device's attention output against it."""
import numpy as np
import torch


def weights(net, x):
    """every row's softmax weights exactly as ValueNetwork.forward computes them (it keeps only row 0's): x [n, h, d]"""
    n, h, d = x.shape
    with torch.no_grad():
        hidden = net.mlp1(x.reshape(-1, d))
        glob = hidden.view(n, h, -1).mean(1, keepdim=True).expand(n, h, net.global_state_dim)
        scores = net.attention(torch.cat([hidden, glob.reshape(-1, net.global_state_dim)], dim=1)).view(n, h)
        e = torch.exp(scores) * (scores != 0).float()
        return (e / e.sum(dim=1, keepdim=True)).numpy()


def check(eng, net, counts=None):
    """attention vs the torch mirror on the exported X (1e-6), sums to 1 over the humans present, 0 for absent ones; values /
    best / action bit-identical to cn_sarl_select on the same state"""
    plain = eng.sarl_select()
    plain = {k: plain[k].cpu().numpy() for k in ('values', 'best', 'action')}
    out = eng.sarl_select(want_attention=True)
    att = out['attention'].cpu().numpy()
    X = eng.sarl_export('X').cpu()
    for k in ('values', 'best', 'action'):
        assert np.array_equal(out[k].cpu().numpy(), plain[k]), k
    B, K, H, d = X.shape
    assert att.shape == (B, K, H) and att.dtype == np.float32, (att.shape, att.dtype)
    if counts is None:
        counts = np.full(B, H)
    for b in range(B):
        n = int(counts[b])
        want = weights(net, X[b, :, :n])
        assert np.abs(att[b, :, :n] - want).max() <= 1e-6, (b, np.abs(att[b, :, :n] - want).max())
        assert np.abs(att[b, :, :n].astype(np.float64).sum(1) - 1.0).max() <= 1e-6, b
        assert (att[b, :, n:] == 0).all(), b
    return att
