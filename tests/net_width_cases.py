"""Value-network layer widths other than the shipped ones, and with_global_state = 0, shared by test_net_widths_host.py (CPU)
and test_net_widths.py (GPU): the table of network settings, each with the torch module that is its reference, a host restatement
of how cn_sarl_configure sizes a network (packed layers, LDS buffers, bytes per tile, the route), and the crowds the tests run.

Every entry is in the table for a property of its widths, named in `why` and checked by a predicate in test_net_widths_host.py:
moving a number is fine as long as the predicate still holds.  The sizing functions restate include/crowdnav_amd.h and
csrc/sarl_net.h (sarl_ks, PackedLinear) so that the table can say, without a GPU, which kernel a setting must take."""
import collections

import numpy as np

from env_setting_cases import setting_id  # noqa: F401  (a setting's name, for parametrize ids)

GROUPS = 16        # kSarlGroups: (env, action) groups per tile = rows of a matrix-instruction tile
K_CHUNK = 5        # kSarlKChunk: k-steps per trip of the k loop; a layer's kpad is a whole number of them
NARROW_K = 40      # kNarrowK: k-steps of a column tile the narrow kernel holds in registers; longer layers take its tail loop
WAVES, NARROW_WAVES = 16, 8
MAX_HUMANS = 8     # kSarlMaxHumans: more humans stream through in chunks whatever the widths
CHUNK = 5          # kSarlChunk: row tiles per chunk of the streamed kernels
THREADS = 1024     # kSarlThreads
LDS_LIMIT = 160 * 1024
SELF_DIM, IN_DIM = 6, 13
SHIPPED = dict(mlp1_dims=(150, 100), mlp2_dims=(100, 50), attention_dims=(100, 100, 1), mlp3_dims=(150, 100, 100, 1))
HEAD = (150, 100, 100, 1)

Setting = collections.namedtuple('Setting', 'name model dims with_global_state seed why')


def _sarl(name, mlp1, mlp2, attention, mlp3, glob, seed, why):
    return Setting(name, 'sarl', dict(mlp1_dims=mlp1, mlp2_dims=mlp2, attention_dims=attention, mlp3_dims=mlp3), glob, seed, why)


def _both(name, mlp1, mlp2, attention, mlp3, seeds, why):
    return [_sarl(name, mlp1, mlp2, attention, mlp3, True, seeds[0], why),
            _sarl(name + '_noglobal', mlp1, mlp2, attention, mlp3, False, seeds[1], why + '; attention.0 sees mlp1 alone')]


def _cadrl(dims, seed, why):
    return Setting('cadrl_' + '_'.join(str(d) for d in dims[:3]), 'cadrl', dict(mlp3_dims=dims), True, seed, why)


def _lstm(hidden, head, seed, why, interaction=None):
    name = 'lstm%s_h%d_%s' % ('2' if interaction else '', hidden, '_'.join(str(d) for d in (interaction or head)[:3]))
    dims = dict(mlp1_dims=(hidden, 1), mlp3_dims=head)
    if interaction:
        dims['interaction_dims'] = interaction
    return Setting(name, 'lstm_rl', dims, True, seed, why)


# Seeds: torch's default initialisation under the first of s, s + 1000, s + 2000, .. at which, on host_rows() of the crowds below, every
# ReLU layer has a live unit, no group's attention scores are all zero and V spreads over the actions by 5e-3 of max |V| (the
# GPU tests require 1e-3 on the device's own X)
SETTINGS = (
    # ---- sarl.ValueNetwork: mlp1 / mlp2 / attention / mlp3
    [_sarl('shipped_noglobal', (150, 100), (100, 50), (100, 100, 1), HEAD, False, 4101,
           'the shipped widths with with_global_state = 0: isolates the flag')]
    + _both('tiny', (8, 4), (4, 1), (4, 4, 1), (4, 4, 4, 1), (4110, 4111),
            'every N < 16 (one partial column tile), K = 4 is one k-step, nf = 1, the joint state is 7 wide')
    + _both('odd', (37, 29), (23, 11), (19, 17, 1), (31, 13, 7, 1), (6120, 13121),
            'no width is a multiple of 4: partial last k-steps and partial last column tiles everywhere')
    # (attention 120,112,1 would make buffer B 30 k-steps and the streamed kernel 165 632 B of LDS, refused from 5 humans on;
    # 120,100,1 is 28 k-steps and 162 560 B, and attention.2 still decides buffer B over the 64-wide mlp1 output)
    + [_sarl('widening', (16, 64), (128, 90), (120, 100, 1), (40, 140, 150, 1), True, 5130,
             'later layers wider than earlier ones; the joint state 6 + 90 is not the widest layer of buffer A'),
       _sarl('exact', (160, 80), (80, 20), (80, 80, 1), (160, 80, 20, 1), True, 5140,
             'every K a whole number of k-chunks, K = 160 exactly kNarrowK k-steps, every N whole column tiles'),
       # (272,100 / 100,50 / 100,100,1 — the shipped layers behind the 272 — is refused at 5 humans: the STREAMED kernel's five row tiles of a 70-k-step
       # buffer A beside 28- and 16-k-step B and C need 202 496 B of LDS.  Narrower layers behind the 272 keep every property:
       # 17 column tiles, K = 272 -> kpad 70 > kNarrowK, one tile at 2 humans, streamed at 5)
       _sarl('wide', (272, 32), (32, 16), (32, 32, 1), HEAD, True, 7150,
             '17 column tiles: the 16-wave kernels go round their column-tile loop a second time (the 8-wave narrow kernel a '
             'third); K = 272 into mlp1.2 is kpad 70 > kNarrowK; one tile at 2 humans, streamed at 5')]
    # ---- cadrl.ValueNetwork: mlp_dims
    + [_cadrl((8, 4, 4, 1), 10201, 'every N < 16, K = 4 and K = 8'),
       _cadrl((37, 29, 7, 1), 6202, 'no width a multiple of 4'),
       _cadrl((64, 150, 160, 1), 4203, 'widening: the third layer decides buffer A; K = 160 exactly kNarrowK k-steps'),
       _cadrl((272, 100, 36, 1), 5204, '17 column tiles, kpad 70 > kNarrowK (8 humans on one tile are refused: 208 896 B of LDS)')]
    # ---- lstm_rl.ValueNetwork1: hidden width, then the value head
    + [_lstm(7, (31, 13, 7, 1), 4301, 'gates 28 wide: i | f | g | o all inside two column tiles, boundaries at 7, 14, 21'),
       _lstm(16, HEAD, 4302, 'every gate boundary ON a column-tile boundary'),
       _lstm(33, (64, 150, 40, 1), 5303, 'gate boundaries at 33, 66, 99: inside column tiles 2, 4 and 6; widening head'),
       _lstm(60, HEAD, 4304, 'the largest hidden width the narrow route admits (W_hh: 15 k-steps, 15 column tiles)'),
       _lstm(64, HEAD, 6305, 'one past that limit (W_hh: 16 k-steps -> kpad 20): the narrow route must not be taken')]
    # ---- lstm_rl.ValueNetwork2: the interaction module in front of the LSTM
    + [_lstm(11, HEAD, 4401, 'odd interaction widths, LSTM input 11 wide', interaction=(37, 29, 23, 11)),
       _lstm(33, HEAD, 6402, 'widening interaction widths: buffer ping 128, pong 64', interaction=(16, 64, 128, 20))]
)
BY_NAME = {s.name: s for s in SETTINGS}
assert len(BY_NAME) == len(SETTINGS)
HUMANS = (1, 2, 5, 8, 9)  # 8: the largest crowd of a one-tile kernel; 9: streamed whatever the widths


def configure_kwargs(s):
    """What BatchedCrowdSim.sarl_configure takes for the setting (beside the action table)."""
    kw = dict(s.dims, model=s.model)
    if s.model == 'sarl':
        kw['with_global_state'] = s.with_global_state
    return kw


def is_shipped(s):
    d = dict(SHIPPED, **s.dims) if s.model == 'sarl' else s.dims
    if s.model == 'sarl':
        return bool(s.with_global_state) and all(tuple(d[k]) == SHIPPED[k] for k in SHIPPED)
    if s.model == 'cadrl':
        return tuple(d['mlp3_dims']) == HEAD
    return tuple(d['mlp3_dims']) == HEAD and d['mlp1_dims'][0] == 50 and tuple(d.get('interaction_dims', (150, 100, 100, 50))) == (150, 100, 100, 50)


def network(s):
    """The crowdnav_amd.compat module of the setting, torch's default initialisation under the setting's own seed."""
    import torch
    from crowdnav_amd.compat import cadrl, lstm_rl, sarl
    torch.manual_seed(s.seed)
    d = s.dims
    if s.model == 'sarl':
        return sarl.ValueNetwork(IN_DIM, SELF_DIM, list(d['mlp1_dims']), list(d['mlp2_dims']), list(d['mlp3_dims']),
                                 list(d['attention_dims']), bool(s.with_global_state), 1.0, 4)
    if s.model == 'cadrl':
        return cadrl.ValueNetwork(IN_DIM, list(d['mlp3_dims']))
    if 'interaction_dims' in d:
        return lstm_rl.ValueNetwork2(IN_DIM, SELF_DIM, list(d['interaction_dims']), list(d['mlp3_dims']), d['mlp1_dims'][0])
    return lstm_rl.ValueNetwork1(IN_DIM, SELF_DIM, list(d['mlp3_dims']), d['mlp1_dims'][0])


def double_of(net):
    """The same module in float64 (the truth of every comparison)."""
    import copy
    return copy.deepcopy(net).double()


def evaluate(s, net, x):
    """V [n] of the joint states x [n, H, 13] under the module, in x's precision (the module's must match): what the device's
    V is compared with.  CADRL: the minimum over the humans' rows (cadrl.py:162-163)."""
    import torch
    n, H, d = x.shape
    with torch.no_grad():
        if s.model == 'cadrl':
            return net(x.reshape(-1, d)).reshape(n, H).min(dim=1)[0]
        if s.model == 'lstm_rl':  # the modules' forward with an initial state of x's dtype
            seq = net.mlp1(x.reshape(-1, d)).reshape(n, H, -1) if hasattr(net, 'mlp1') else x
            zeros = torch.zeros(1, n, net.lstm_hidden_dim, dtype=x.dtype)
            _, (hn, _) = net.lstm(seq, (zeros, zeros.clone()))
            return net.mlp(torch.cat([x[:, 0, :net.self_state_dim], hn.squeeze(0)], dim=1)).reshape(n)
        return net(x).reshape(n)


def attention(net, x):
    """(scores, weights) [n, H] of sarl.ValueNetwork on x [n, H, 13], recomputed with the module's own layers (sarl.py:44-54):
    mlp1, the mean over the humans when the module has a global state, attention, exp over the sum."""
    import torch
    n, H, d = x.shape
    with torch.no_grad():
        hidden = net.mlp1(x.reshape(-1, d))
        if net.with_global_state:
            glob = hidden.view(n, H, -1).mean(1, keepdim=True).expand(n, H, hidden.shape[1]).reshape(n * H, -1)
            hidden = torch.cat([hidden, glob], dim=1)
        scores = net.attention(hidden).view(n, H)
        e = torch.exp(scores) * (scores != 0).to(x.dtype)
        return scores, e / e.sum(dim=1, keepdim=True)


# ---------------------------------------------------------------------------------------- sizes, as cn_sarl_configure computes them
def ksteps(K):
    return (K + 3) // 4


def kpad(K):
    return (ksteps(K) + K_CHUNK - 1) // K_CHUNK * K_CHUNK


def ctiles(N):
    return (N + 15) // 16


def ks(n):
    """cn::sarl_ks: k-steps per row tile of an LDS buffer that holds n features."""
    return max(ctiles(n) * 4, kpad(n))


def layers(s):
    """The linear layers of the setting in the order the kernels run them: [(name, N, K, input buffer, output buffer)].  A buffer is
    named as in sarl_size_network ('x', 'a', 'b', 'c'; LSTM-RL: 'g' the gates, 'h' the hidden state, 's' the one-column output)."""
    d = s.dims
    if s.model == 'cadrl':
        j = d['mlp3_dims']
        return [('mlp.0', j[0], IN_DIM, 'x', 'a'), ('mlp.2', j[1], j[0], 'a', 'b'), ('mlp.4', j[2], j[1], 'b', 'a'), ('mlp.6', 1, j[2], 'a', 's')]
    if s.model == 'lstm_rl':
        hid, j, inter = d['mlp1_dims'][0], d['mlp3_dims'], d.get('interaction_dims')
        out = []
        if inter:
            out += [('mlp1.0', inter[0], IN_DIM, 'x', 'b'), ('mlp1.2', inter[1], inter[0], 'b', 'c'),
                    ('mlp1.4', inter[2], inter[1], 'c', 'b'), ('mlp1.6', inter[3], inter[2], 'b', 'c')]
        out += [('lstm.ih', 4 * hid, inter[3] if inter else IN_DIM, 'c' if inter else 'x', 'g'), ('lstm.hh', 4 * hid, hid, 'h', 'g'),
                ('mlp.0', j[0], SELF_DIM + hid, 'a', 'a'), ('mlp.2', j[1], j[0], 'a', 'a'), ('mlp.4', j[2], j[1], 'a', 'a'), ('mlp.6', 1, j[2], 'a', 's')]
        return out
    m1, m2, at, j = d['mlp1_dims'], d['mlp2_dims'], d['attention_dims'], d['mlp3_dims']
    out = [('mlp1.0', m1[0], IN_DIM, 'x', 'a'), ('mlp1.2', m1[1], m1[0], 'a', 'b'), ('mlp2.0', m2[0], m1[1], 'b', 'a'),
           ('mlp2.2', m2[1], m2[0], 'a', 'c'), ('attention.0 local', at[0], m1[1], 'b', 'a')]
    if s.with_global_state:
        out.append(('attention.0 global', at[0], m1[1], 'b', 'a'))
    out += [('attention.2', at[1], at[0], 'a', 'b'), ('attention.4', 1, at[1], 'b', 's'),
            ('mlp3.0', j[0], SELF_DIM + m2[1], 'a', 'a'), ('mlp3.2', j[1], j[0], 'a', 'a'), ('mlp3.4', j[2], j[1], 'a', 'a'), ('mlp3.6', 1, j[2], 'a', 's')]
    return out


def buffers(s):
    """k-steps per row tile of the LDS buffers: dict x, a, b, c (sarl_size_network) and, for LSTM-RL, g and h."""
    d = s.dims
    j = d['mlp3_dims']
    if s.model == 'cadrl':
        return dict(x=ks(IN_DIM), a=ks(max(j[0], j[2])), b=max(ks(j[1]), ks(IN_DIM)), c=0, s=4)
    if s.model == 'lstm_rl':
        hid, inter = d['mlp1_dims'][0], d.get('interaction_dims')
        return dict(x=ks(IN_DIM), a=ks(max(j[0], j[1], j[2], SELF_DIM + hid)), b=ks(max(inter[0], inter[2])) if inter else 0,
                    c=ks(max(inter[1], inter[3])) if inter else 0, g=ctiles(4 * hid) * 4, h=ks(hid), s=4)
    m1, m2, at = d['mlp1_dims'], d['mlp2_dims'], d['attention_dims']
    return dict(x=ks(IN_DIM), a=ks(max(m1[0], m2[0], at[0], SELF_DIM + m2[1], j[0], j[1], j[2])),
                b=max(ks(max(m1[1], at[1])), ks(IN_DIM)), c=ks(m2[1]), s=4)


def tile_lds_bytes(s, H):
    """Bytes of LDS of the one-tile kernel at H humans (sarl_pipe_lds_bytes: the header's 4 x 64 x (H (ks_a + ks_b + ks_c + 4) + ks_b +
    3 ks_a) plus the partial sums and the human counts; cadrl_lds_bytes; lstm_lds_bytes)."""
    b = buffers(s)
    if s.model == 'cadrl':
        return 4 * 64 * H * (b['a'] + b['b'] + b['s'])
    if s.model == 'lstm_rl':
        return 4 * (64 * (H * (b['x'] + b['b'] + b['c']) + b['g'] + b['h'] + 2 * b['a'] + b['s']) + s.dims['mlp1_dims'][0] * GROUPS)
    return 4 * (64 * (H * (b['a'] + b['b'] + b['c'] + b['s']) + b['b'] + 3 * b['a']) + THREADS + GROUPS)


def chunked_lds_bytes(s):
    """... of the kernel that streams the humans: CHUNK row tiles at a time (LSTM-RL: one)."""
    b = buffers(s)
    if s.model == 'cadrl':
        return 4 * (64 * CHUNK * (b['a'] + b['b'] + b['s']) + GROUPS)
    if s.model == 'lstm_rl':
        return tile_lds_bytes(s, 1)
    return 4 * (64 * (CHUNK * (b['a'] + b['b'] + b['c'] + b['s']) + b['b'] + 2 * b['a'] + b['c'] + 1) + THREADS)


def narrow_lds_bytes(s, H):
    b = buffers(s)
    extra = THREADS + (2 + NARROW_WAVES) * GROUPS
    if s.model == 'lstm_rl':
        return 4 * (64 * (H * b['x'] + H * b['g'] + b['g'] + b['h'] + 2 * b['a'] + 1) + s.dims['mlp1_dims'][0] * GROUPS + extra)
    return 4 * (64 * (b['x'] + 4 * b['a'] + 2 * b['b'] + b['c'] + 1) + extra)


def streams(s, H):
    """sarl_size_network's `chunked`: the humans do not fit one tile."""
    if H > MAX_HUMANS:
        return True
    return s.model != 'cadrl' and tile_lds_bytes(s, H) > LDS_LIMIT


def lds_route(s, H):
    """The route with CROWDNAV_AMD_SARL_NARROW=0 (and no register-resident kernel): 'lds_tile', 'lds_chunked', or None where
    cn_sarl_configure refuses the size ('bytes of LDS per tile')."""
    chunked = streams(s, H)
    if (chunked_lds_bytes(s) if chunked else tile_lds_bytes(s, H)) > LDS_LIMIT:
        return None
    return 'lds_chunked' if chunked else 'lds_tile'


def narrow_admits(s, H):
    """Whether CROWDNAV_AMD_SARL_NARROW=2 gives the narrow tiles (sarl_route_f32 at 13 inputs, the env queried)."""
    if lds_route(s, H) != 'lds_tile' or H > MAX_HUMANS or narrow_lds_bytes(s, H) > LDS_LIMIT:
        return False
    if s.model == 'lstm_rl':
        hid = s.dims['mlp1_dims'][0]
        return ('interaction_dims' not in s.dims and kpad(IN_DIM) <= 4 * K_CHUNK and kpad(hid) <= 3 * K_CHUNK
                and kpad(SELF_DIM + hid) <= NARROW_K)
    return True


def state_dict_shapes(s):
    """What the dims say the module's state_dict holds: {key: shape}, in the module's own order."""
    d = s.dims

    def stack(prefix, first, widths):
        out, k = [], first
        for i, n in enumerate(widths):
            out += [('%s.%d.weight' % (prefix, 2 * i), (n, k)), ('%s.%d.bias' % (prefix, 2 * i), (n,))]
            k = n
        return out

    def lstm(k, hid):
        return [('lstm.weight_ih_l0', (4 * hid, k)), ('lstm.weight_hh_l0', (4 * hid, hid)), ('lstm.bias_ih_l0', (4 * hid,)),
                ('lstm.bias_hh_l0', (4 * hid,))]

    if s.model == 'cadrl':
        return collections.OrderedDict(stack('value_network', IN_DIM, d['mlp3_dims']))
    if s.model == 'lstm_rl':
        hid, inter = d['mlp1_dims'][0], d.get('interaction_dims')
        if inter:
            return collections.OrderedDict(stack('mlp1', IN_DIM, inter) + stack('mlp', SELF_DIM + hid, d['mlp3_dims']) + lstm(inter[3], hid))
        return collections.OrderedDict(stack('mlp', SELF_DIM + hid, d['mlp3_dims']) + lstm(IN_DIM, hid))
    m1 = d['mlp1_dims']
    return collections.OrderedDict(stack('mlp1', IN_DIM, m1) + stack('mlp2', m1[1], d['mlp2_dims'])
                                   + stack('attention', m1[1] * (2 if s.with_global_state else 1), d['attention_dims'])
                                   + stack('mlp3', SELF_DIM + d['mlp2_dims'][1], d['mlp3_dims']))


# ---------------------------------------------------------------------------------------- crowds
ENVS = 3
CIRCLE, CLEARANCE = 4.0, 0.75  # humans inside a 4 m circle, centres at least 0.75 m apart (radii 0.3: no overlap)


def crowd(humans, salt=0):
    """state8 [ENVS, humans + 1, 8] float64 (px, py, vx, vy, gx, gy, radius, v_pref): per env a robot on the circle's rim heading
    for the opposite side (never at its goal) and `humans` humans at seeded places inside the circle, no two agents closer than
    CLEARANCE, each walking towards a seeded goal.  (om_grid_cases.random_crowd scales with a grid setting and lets humans share
    a place: it does not fit here.)"""
    rs = np.random.RandomState(9001 + 131 * humans + salt)
    out = np.zeros((ENVS, humans + 1, 8))
    for b in range(ENVS):
        ang = rs.uniform(0.0, 2.0 * np.pi)
        robot = CIRCLE * np.array([np.cos(ang), np.sin(ang)])
        placed = [robot]
        out[b, 0] = [robot[0], robot[1], 0.0, 0.0, -robot[0], -robot[1], 0.3, 1.0]
        for h in range(humans):
            while True:
                r, a = CIRCLE * np.sqrt(rs.uniform()), rs.uniform(0.0, 2.0 * np.pi)
                p = np.array([r * np.cos(a), r * np.sin(a)])
                if min(np.linalg.norm(p - q) for q in placed) >= CLEARANCE:
                    break
            placed.append(p)
            goal = rs.uniform(-CIRCLE, CIRCLE, 2)
            speed = rs.uniform(0.2, 1.0)
            v = speed * (goal - p) / max(np.linalg.norm(goal - p), 1e-9)
            out[b, 1 + h] = [p[0], p[1], v[0], v[1], goal[0], goal[1], 0.3, 1.0]
    return out


def actions(n):
    """The first n rows of the shipped holonomic action table (stop, then rotations x speeds)."""
    from crowdnav_amd.compat.sarl import build_action_space
    space, _, _ = build_action_space(1.0)
    return np.array([[a.vx, a.vy] for a in space[:n]])


def host_rows(state8, acts, dt=0.25):
    """An X the host can build: CADRL.rotate of [propagate(robot, action) | human moved on by its own velocity], float32
    [B, K, H, 13].  The device's X differs (its humans take their ORCA velocities): this one is for choosing seeds and for the
    host test, the GPU tests take the exported X."""
    import torch
    from crowdnav_amd.compat.sarl import rotate
    state8, acts = np.asarray(state8, dtype=np.float64), np.asarray(acts, dtype=np.float64)
    B, A = state8.shape[:2]
    rows = np.zeros((B, len(acts), A - 1, 14))
    for k, (ax, ay) in enumerate(acts):
        rob = state8[:, 0]
        rows[:, k, :, :9] = np.stack([rob[:, 0] + ax * dt, rob[:, 1] + ay * dt, np.full(B, ax), np.full(B, ay), rob[:, 6], rob[:, 4], rob[:, 5],
                                      rob[:, 7], np.zeros(B)], axis=1)[:, None]
        hum = state8[:, 1:]
        rows[:, k, :, 9:] = np.stack([hum[..., 0] + hum[..., 2] * dt, hum[..., 1] + hum[..., 3] * dt, hum[..., 2], hum[..., 3], hum[..., 6]], axis=2)
    x = rotate(torch.from_numpy(rows.reshape(-1, 14)).float())
    return x.reshape(B, len(acts), A - 1, 13)


def relu_layers_alive(net, x):
    """Per ReLU of the module, whether at least one of its units is positive somewhere on the rows x [n, H, 13]: [(name, bool)]."""
    import torch
    seen = []
    hooks = [m.register_forward_hook(lambda mod, inp, out, name=name: seen.append((name, bool((out > 0).any()))))
             for name, m in net.named_modules() if isinstance(m, torch.nn.ReLU)]
    try:
        with torch.no_grad():
            net(x)
    finally:
        for h in hooks:
            h.remove()
    return seen
