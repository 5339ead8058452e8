"""The emulation of the device's kd-tree bookkeeping (kd_order_emulation.py) against its transcription of RVO2's KdTree, on random
and on lattice (tie-heavy) point sets over many steps."""
import numpy as np

from kd_order_emulation import RvoTree, device_neighbours, f32, partition_bits, shared_tree


def _scenes(rng, n, steps, lattice):
    """positions per step: a random walk; on lattice steps every coordinate is a multiple of 0.25 (exact in float32,
    hundreds of exactly equal squared distances)"""
    p = rng.uniform(-4, 4, size=(n, 2))
    for t in range(steps):
        p = p + rng.uniform(-0.3, 0.3, size=p.shape)
        if lattice(t):
            q = np.round(p * 4) / 4
            # distinct lattice points (agents never coincide)
            seen = set()
            for i in range(n):
                while (q[i, 0], q[i, 1]) in seen:
                    q[i, 0] += 0.25
                seen.add((q[i, 0], q[i, 1]))
            yield q.astype(np.float32)
        else:
            yield p.astype(np.float32)


def _run(n, steps, lattice, seed, max_nb=10, range_sq=100.0):
    rng = np.random.RandomState(seed)
    sims = list(range(n))
    # simulator of agent q lists itself first, then the others in index order (orca.py:99-104)
    local = {q: [q] + [a for a in range(n) if a != q] for q in sims}
    rvo = {q: RvoTree(n) for q in sims}
    rows = {q: list(local[q]) for q in sims}  # device rows hold GLOBAL agent ids in the simulator's order
    ties = 0
    for pos in _scenes(rng, n, steps, lattice):
        pos = [(f32(x), f32(y)) for x, y in pos]
        nodes = shared_tree(pos, list(range(n)))
        for q in sims:
            lp = [pos[a] for a in local[q]]  # positions in the simulator's own numbering
            rvo[q].build(lp)
            for b, e, nl, left in nodes:
                partition_bits(rows[q], b, e, nl, left)
            assert [local[q][i] for i in rvo[q].order] == rows[q], 'permutation differs'
            want = [(d, local[q][i]) for d, i in rvo[q].neighbours(lp, 0, max_nb, range_sq)]
            got = device_neighbours(pos, rows[q], nodes, q, max_nb, range_sq)
            assert got == want, (q, got, want)
            ds = [d for d, _ in want]
            ties += len(ds) - len(set(ds))
    return ties


def test_random_walks_keep_the_same_permutation_and_neighbours():
    for n, seed in ((11, 0), (13, 1), (21, 2), (21, 3), (34, 4), (64, 5)):
        _run(n, 12, lambda t: False, seed)


def test_lattice_scenes_with_exact_ties_follow_rvo2_visit_order():
    ties = 0
    for n, seed in ((12, 10), (13, 11), (21, 12), (21, 13), (40, 14)):
        ties += _run(n, 10, lambda t: t % 3 != 1, seed)  # lattice, free, lattice, ... : the permutation carries history
    assert ties > 200  # the scenes really are tie-heavy


def test_small_neighbour_lists_and_short_range():
    for seed in range(3):
        _run(21, 6, lambda t: t % 2 == 0, 20 + seed, max_nb=3, range_sq=9.0)
        _run(14, 6, lambda t: True, 30 + seed, max_nb=10, range_sq=4.0)
