"""The table of value-network widths (net_width_cases.py) keeps what it is there for: host only, no library, no GPU.
Every property the width sweep of test_net_widths.py relies on is a predicate on the dims here, so a number moved in the table
cannot silently take a branch out of the sweep."""
import numpy as np
import pytest
import torch

import net_width_cases as cases

SARL = [s for s in cases.SETTINGS if s.model == 'sarl']
CADRL = [s for s in cases.SETTINGS if s.model == 'cadrl']
LSTM1 = [s for s in cases.SETTINGS if s.model == 'lstm_rl' and 'interaction_dims' not in s.dims]
LSTM2 = [s for s in cases.SETTINGS if s.model == 'lstm_rl' and 'interaction_dims' in s.dims]


def _all_layers(settings):
    return [(s, layer) for s in settings for layer in cases.layers(s)]


def test_the_table_is_self_consistent():
    assert len({s.name for s in cases.SETTINGS}) == len(cases.SETTINGS) and len({s.seed for s in cases.SETTINGS}) == len(cases.SETTINGS)
    for s in cases.SETTINGS:
        assert s.why and s.model in ('sarl', 'cadrl', 'lstm_rl'), s.name
        assert s.dims['mlp3_dims'][3] == 1 and all(d >= 1 for dims in s.dims.values() for d in dims), s.name
        if s.model == 'sarl':
            assert s.dims['attention_dims'][2] == 1, s.name
        b = cases.buffers(s)
        for name, N, K, src, dst in cases.layers(s):
            # the invariant the straight-line k loop rests on: a consumer's kpad never exceeds its input buffer's k-steps, and a
            # producer's whole column tiles fit its output buffer
            assert cases.kpad(K) <= b[src], (s.name, name)
            assert cases.ctiles(N) * 4 <= b[dst], (s.name, name)
            assert cases.kpad(K) <= 255 and cases.ctiles(N) <= 255, (s.name, name)
        # the sweep runs every setting at 1, 2, 5 and 9 humans: none of those may be a size cn_sarl_configure refuses
        for H in (1, 2, 5, 9):
            assert cases.lds_route(s, H) is not None, (s.name, H)
        assert cases.lds_route(s, 9) == 'lds_chunked', s.name
        assert not cases.is_shipped(s), s.name
    assert cases.is_shipped(cases.Setting('x', 'sarl', dict(cases.SHIPPED), True, 0, ''))


def test_the_sizing_restates_the_shipped_numbers():
    """The figures DESIGN.md and the header quote for the shipped networks come out of the table's formulas."""
    shipped = cases.Setting('shipped', 'sarl', dict(cases.SHIPPED), True, 0, '')
    assert cases.buffers(shipped) == dict(x=5, a=40, b=28, c=16, s=4)
    assert cases.tile_lds_bytes(shipped, 5) == 154688  # one tile holds 5 humans, not 6
    assert cases.lds_route(shipped, 5) == 'lds_tile' and cases.lds_route(shipped, 6) == 'lds_chunked'
    assert cases.chunked_lds_bytes(shipped) == 148736
    wider = cases.Setting('w', 'sarl', dict(cases.SHIPPED, mlp1_dims=(170, 100)), True, 0, '')
    assert cases.tile_lds_bytes(wider, 5) == 164928 > cases.LDS_LIMIT >= cases.chunked_lds_bytes(wider) == 157696  # (tests/test_om_grid.py quotes both)
    assert cases.lds_route(cases.Setting('w', 'sarl', dict(cases.SHIPPED, mlp1_dims=(1000, 100)), True, 0, ''), 5) is None
    assert (cases.ksteps(150), cases.kpad(150), cases.ctiles(150), cases.ks(150)) == (38, 40, 10, 40)


def test_required_settings_are_there():
    names = {s.name for s in cases.SETTINGS}
    assert {'shipped_noglobal', 'tiny', 'tiny_noglobal', 'odd', 'odd_noglobal', 'widening', 'exact', 'wide'} <= names
    noglobal = cases.BY_NAME['shipped_noglobal']
    assert not noglobal.with_global_state and all(tuple(noglobal.dims[k]) == cases.SHIPPED[k] for k in cases.SHIPPED)
    for pair in ('tiny', 'odd'):
        a, b = cases.BY_NAME[pair], cases.BY_NAME[pair + '_noglobal']
        assert a.dims == b.dims and a.with_global_state and not b.with_global_state
    assert len(CADRL) >= 4 and len(LSTM1) >= 5 and len(LSTM2) >= 2


def test_tiny_is_below_one_tile_everywhere():
    for s in (cases.BY_NAME['tiny'], cases.BY_NAME['tiny_noglobal']):
        for name, N, K, _, _ in cases.layers(s):
            assert N < 16, (s.name, name)
        assert any(K == 4 and cases.ksteps(K) == 1 for _, _, K, _, _ in cases.layers(s))
        assert s.dims['mlp2_dims'][1] == 1                                   # nf = 1
        assert [K for n, _, K, _, _ in cases.layers(s) if n == 'mlp3.0'] == [7]  # the joint state
    assert any(all(N < 16 for _, N, _, _, _ in cases.layers(s)) for s in CADRL)


def test_odd_has_no_multiple_of_four():
    for s in (cases.BY_NAME['odd'], cases.BY_NAME['odd_noglobal']):
        widths = [d for dims in s.dims.values() for d in dims if d != 1]
        assert widths and all(w % 4 for w in widths), s.name
    assert any(all(d % 4 for d in s.dims['mlp3_dims'][:3]) for s in CADRL)
    assert any(all(d % 4 for d in s.dims['interaction_dims']) for s in LSTM2)


def test_widening_reorders_which_layer_decides_a_buffer():
    s = cases.BY_NAME['widening']
    d = s.dims
    assert d['mlp1_dims'][0] < d['mlp1_dims'][1] < d['mlp2_dims'][0] and d['mlp3_dims'][0] < d['mlp3_dims'][1] < d['mlp3_dims'][2]
    joint = cases.SELF_DIM + d['mlp2_dims'][1]
    assert cases.ks(joint) < cases.buffers(s)['a']                                    # the joint state is not buffer A's widest layer
    assert cases.buffers(s)['a'] == cases.ks(d['mlp3_dims'][2]) > cases.ks(d['mlp1_dims'][0])  # ... a LATE layer is, not mlp1.0
    assert cases.buffers(s)['b'] == cases.ks(d['attention_dims'][1]) > cases.ks(d['mlp1_dims'][1])
    assert any(s.dims['mlp3_dims'][0] < s.dims['mlp3_dims'][2] for s in CADRL)        # CADRL: the third layer decides buffer A
    assert any(s.dims['interaction_dims'][0] < s.dims['interaction_dims'][2] for s in LSTM2)


def test_exact_has_no_padding_anywhere():
    s = cases.BY_NAME['exact']
    for name, N, K, _, _ in cases.layers(s):
        if K != cases.IN_DIM and not name.startswith('mlp3.0'):
            assert K % (4 * cases.K_CHUNK) == 0, name                # whole k-chunks: kpad == ksteps
        if N != 1:
            assert N % 16 == 0 or N == 20, name
    assert any(cases.ksteps(K) == cases.NARROW_K for _, _, K, _, _ in cases.layers(s))  # exactly the registers' 40 k-steps
    assert any(cases.ksteps(K) == cases.NARROW_K for c in CADRL for _, _, K, _, _ in cases.layers(c))


def test_wide_takes_the_second_trip_and_the_narrow_tail():
    s = cases.BY_NAME['wide']
    assert any(cases.ctiles(N) > cases.WAVES for _, N, _, _, _ in cases.layers(s))           # the 16-wave kernels go round again
    assert any(cases.ctiles(N) > 2 * cases.NARROW_WAVES for _, N, _, _, _ in cases.layers(s))  # the narrow kernel a third time
    assert any(cases.kpad(K) > cases.NARROW_K for _, _, K, _, _ in cases.layers(s))          # narrow_dense's tail from L2
    small = min(H for H in cases.HUMANS if cases.lds_route(s, H) == 'lds_tile')
    assert small == 1 and cases.lds_route(s, 2) == 'lds_tile' and cases.narrow_admits(s, 2)
    assert cases.tile_lds_bytes(s, 2) == 4 * (64 * (2 * (70 + 10 + 5 + 4) + 10 + 3 * 70) + 1024 + 16) == 106048 <= cases.LDS_LIMIT
    assert cases.tile_lds_bytes(s, 5) == 174400 > cases.LDS_LIMIT and cases.lds_route(s, 5) == 'lds_chunked'
    assert cases.chunked_lds_bytes(s) == 157952 <= cases.LDS_LIMIT
    # the shipped layers behind the 272 instead: the streamed form does not fit (why the entry's later layers are narrow)
    draft = cases.Setting('d', 'sarl', dict(cases.SHIPPED, mlp1_dims=(272, 100)), True, 0, '')
    assert cases.tile_lds_bytes(draft, 2) == 125504 and cases.chunked_lds_bytes(draft) == 202496 and cases.lds_route(draft, 5) is None
    # CADRL and the LSTM head have such a layer too
    assert any(cases.ctiles(N) > cases.WAVES and cases.kpad(N) > cases.NARROW_K for c in CADRL for _, N, _, _, _ in cases.layers(c))
    wide_cadrl = cases.BY_NAME['cadrl_272_100_36']
    assert cases.lds_route(wide_cadrl, 8) is None and cases.tile_lds_bytes(wide_cadrl, 8) == 208896  # (asserted as a refusal on the GPU)


def test_partial_tiles_and_k_steps_other_than_the_shipped_ones():
    shipped_n, shipped_k = {150 % 16, 100 % 16, 50 % 16, 1, 200 % 16}, {150 % 4, 100 % 4, 13 % 4, 56 % 4, 50 % 4}
    ns = {N % 16 for _, (_, N, _, _, _) in _all_layers(cases.SETTINGS)} - shipped_n
    k_rests = {K % 4 for _, (_, _, K, _, _) in _all_layers(cases.SETTINGS)}
    assert len(ns) >= 8 and k_rests == {0, 1, 2, 3} and shipped_k < k_rests
    # the 8-wave narrow kernel's column-tile loop beyond its second trip; the 16-wave kernels' beyond their first
    assert max(cases.ctiles(N) for _, (_, N, _, _, _) in _all_layers(cases.SETTINGS)) > 2 * cases.NARROW_WAVES


def test_lstm_gate_boundaries_and_the_narrow_limits():
    hidden = sorted(s.dims['mlp1_dims'][0] for s in LSTM1)
    assert hidden == [7, 16, 33, 60, 64]
    inside = [h for h in hidden if any((k * h) % 16 for k in (1, 2, 3))]
    assert 16 not in inside and {7, 33, 60} <= set(inside)            # boundaries inside a column tile, and one setting ON them
    assert {(k * 33) % 16 for k in (1, 2, 3)} != {(k * 50) % 16 for k in (1, 2, 3)}  # offsets other than hid = 50's
    by_hidden = {s.dims['mlp1_dims'][0]: s for s in LSTM1}
    for H in (1, 2, 5):
        assert cases.narrow_admits(by_hidden[60], H) and not cases.narrow_admits(by_hidden[64], H)
    assert cases.kpad(60) == 3 * cases.K_CHUNK and cases.kpad(64) > 3 * cases.K_CHUNK  # W_hh: the limit and one past it
    assert not any(cases.narrow_admits(s, H) for s in LSTM2 for H in (1, 2, 5))


def test_every_route_is_reached_by_every_model():
    """lds_tile, lds_chunked and narrow each appear for SARL with and without global state, for CADRL and for LSTM-RL."""
    groups = dict(sarl_global=[s for s in SARL if s.with_global_state], sarl_noglobal=[s for s in SARL if not s.with_global_state],
                  cadrl=CADRL, lstm_rl=LSTM1)
    for name, settings in groups.items():
        routes = {cases.lds_route(s, H) for s in settings for H in cases.HUMANS}
        assert {'lds_tile', 'lds_chunked'} <= routes, name
        assert any(cases.narrow_admits(s, H) for s in settings for H in (1, 2, 5)), name
    # 8 humans separate the one-tile kernel from the streamed one wherever the widths leave room
    assert [s.name for s in cases.SETTINGS if cases.lds_route(s, 8) == 'lds_tile'] and cases.lds_route(cases.BY_NAME['odd'], 8) == 'lds_tile'


@pytest.mark.parametrize('s', cases.SETTINGS, ids=cases.setting_id)
def test_the_torch_module_has_the_shapes_the_dims_say(s):
    net = cases.network(s)
    got = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    assert got == list(cases.state_dict_shapes(s).items())
    again = cases.network(s)  # the seed is the setting's own
    assert all(torch.equal(a, b) for a, b in zip(net.state_dict().values(), again.state_dict().values()))
    # the float64 twin and the precision-generic forward agree with the module's own forward
    x = cases.host_rows(cases.crowd(3), cases.actions(5)).reshape(-1, 3, 13)
    v32, v64 = cases.evaluate(s, net, x), cases.evaluate(s, cases.double_of(net), x.double())
    assert torch.isfinite(v64).all() and (v32.double() - v64).abs().max() <= 1e-4 * max(1.0, v64.abs().max().item())
    if s.model != 'cadrl':
        with torch.no_grad():
            assert torch.equal(net(x).reshape(-1), v32)


@pytest.mark.parametrize('s', [s for s in cases.SETTINGS if s.name.startswith(('tiny', 'odd'))], ids=cases.setting_id)
def test_small_networks_are_alive_under_their_seed(s):
    """torch's default initialisation can leave every unit of a 4-wide ReLU layer dead, and then the layers behind it are not
    tested: the seeds of the small settings are chosen so that each ReLU has a live unit (checked again on the device's X)."""
    for H in (1, 2, 5, 9):
        x = cases.host_rows(cases.crowd(H), cases.actions(5)).reshape(-1, H, 13)
        alive = cases.relu_layers_alive(cases.network(s), x)
        assert alive and all(ok for _, ok in alive), (s.name, H, alive)
        v = cases.evaluate(s, cases.double_of(cases.network(s)), x.double()).reshape(cases.ENVS, -1)
        assert ((v.max(dim=1)[0] - v.min(dim=1)[0]) >= 1e-3 * v.abs().max()).all(), (s.name, H)


def test_crowds_are_seeded_apart_and_inside_the_circle():
    for H in cases.HUMANS:
        c = cases.crowd(H)
        assert c.shape == (cases.ENVS, H + 1, 8) and np.array_equal(c, cases.crowd(H)) and not np.array_equal(c, cases.crowd(H, 1))
        for env in c:
            pos = env[:, :2]
            gap = np.linalg.norm(pos[:, None] - pos[None], axis=2) + 1e9 * np.eye(H + 1)
            assert gap.min() >= cases.CLEARANCE > env[:, 6].max() * 2
            assert (np.linalg.norm(pos[1:], axis=1) <= cases.CIRCLE).all()
            assert np.linalg.norm(pos[0] - env[0, 4:6]) > 1.0  # the robot is not at its goal
