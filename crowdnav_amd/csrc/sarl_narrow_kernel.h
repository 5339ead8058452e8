// sarl_narrow_kernel: the value networks for a FEW decisions, one 16-row tile of whole groups per workgroup (blocks: sarl_kernels.h)
#pragma once
#include "sarl_kernels.h"

namespace cn {

// The same network for a FEW decisions (the single-episode sampling of train.py:156-170: one env, 81 groups = 6 tiles): the
// one-tile kernels (sarl_lds_kernels.h) put a decision on 6 of 256 CUs for ~40 us.  Here a tile is ONE 16-row MFMA tile holding
// 16 / H whole groups — row r = (group r / H, human r % H), 3 groups x 5 humans + 1 idle row at the shipped size — so one
// decision spreads over 27 workgroups, each with a fifth of the matrix work behind the same chain of layers.  X is built in
// LDS by the workgroup that consumes it (sarl_feature_row: no feature kernel, nothing materialised); the mean over a group's
// humans, the softmax and the weighted feature sum run over ROWS of the tile instead of over row tiles, in the order and
// with the partial-sum slicing of sarl_mlp_pipe_kernel / dense_vec1<H>, so V is bit-identical to that kernel's.
// With one row tile a k-step is ONE MFMA, so a layer is bound by the latency of its weights, not by the matrix pipe: a wave
// holds the B fragments of a whole column tile in registers (up to kNarrowK k-steps, 8 waves x 256 VGPRs) and requests the
// NEXT layer's before it starts this layer's MFMAs — one L2 round trip per layer, hidden behind the previous layer, instead
// of one per five k-steps.  H <= 8.
constexpr int kNarrowWaves = 8, kNarrowThreads = kNarrowWaves * 64;
constexpr int kNarrowK = 40;  // k-steps of a column tile held in registers (K = 150 is 38 -> kpad 40); longer layers loop on
struct BTile {
    float b[kNarrowK];
    float bias;
};
__device__ __forceinline__ BTile narrow_fetch(const PackedLinear& P, int ct, int lane) {
    BTile t;
    const bool mine = ct < P.ctiles;  // (wave-uniform: a wave without a column tile of this layer requests nothing)
    const int c = mine ? ct : 0;
    const gfloat_p w = as_global(P.w) + (size_t)c * P.kpad * 64 + lane;
#pragma unroll
    for (int g = 0; g < kNarrowK / kSarlKChunk; ++g) {
        if (mine && g * kSarlKChunk < P.kpad) {
#pragma unroll
            for (int j = 0; j < kSarlKChunk; ++j) t.b[g * kSarlKChunk + j] = w[(g * kSarlKChunk + j) * 64];
        } else {
#pragma unroll
            for (int j = 0; j < kSarlKChunk; ++j) t.b[g * kSarlKChunk + j] = 0.0f;
        }
    }
    t.bias = mine ? as_global(P.bias)[c * 16 + (lane & 15)] : 0.0f;
    return t;
}
// out[r][n] = act(bias[n] + extra[r][n] + sum_k in[r][k] W[n][k]) for the 16 rows of the tile: dense_mfma<1>'s arithmetic
// (k-steps in order into one accumulator from zero, bias + extra added last).  `first` = the fragments of column tile `wave`.
// The k loop is straight-line code of G x 5 k-steps, G = 3 / 5 / 8 by the layer's length (fragments past kpad are zero in
// registers and meet finite LDS words: + 0.0f), so that the A reads from LDS and the MFMAs pipeline without a branch between.
template <int G>
__device__ __forceinline__ f32x4 narrow_k_loop(const float* afrag, const BTile& t) {
    float a[G * kSarlKChunk];
#pragma unroll
    for (int k = 0; k < G * kSarlKChunk; ++k) a[k] = afrag[k * 64];
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < G * kSarlKChunk; ++k) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[k], t.b[k], acc, 0, 0, 0);
    return acc;
}
__device__ __forceinline__ void dense_narrow(const PackedLinear& P, const float* in, float* out, bool relu, const float* extra,
                                             int wave, int lane, const BTile& first) {
    const int col = lane & 15, quad = lane >> 4;
    BTile t = first;
    for (int ct = wave; ct < P.ctiles; ct += kNarrowWaves) {
        const bool more = ct + kNarrowWaves < P.ctiles;  // (150-wide layers: ten column tiles on eight waves)
        BTile t2;
        if (more) t2 = narrow_fetch(P, ct + kNarrowWaves, lane);
        const int frag_off = ((ct * 4 + (col >> 2)) * 64) + (col & 3) * 16 + quad * 4;
        f32x4 addend = {t.bias, t.bias, t.bias, t.bias};
        if (extra) addend += *reinterpret_cast<const f32x4*>(extra + frag_off);
        const float* afrag = in + lane;
        f32x4 acc;
        if (P.kpad <= 3 * kSarlKChunk) acc = narrow_k_loop<3>(afrag, t);
        else if (P.kpad <= 4 * kSarlKChunk) acc = narrow_k_loop<4>(afrag, t);  // (61 inputs: 16 k-steps)
        else if (P.kpad <= 5 * kSarlKChunk) acc = narrow_k_loop<5>(afrag, t);
        else acc = narrow_k_loop<kNarrowK / kSarlKChunk>(afrag, t);
        if (P.kpad > kNarrowK) {  // wider than the shipped layers: the rest of the k loop straight from L2
            const gfloat_p w = as_global(P.w) + (size_t)ct * P.kpad * 64 + lane;
            for (int k = kNarrowK; k < P.kpad; ++k) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(afrag[k * 64], w[k * 64], acc, 0, 0, 0);
        }
        f32x4 v = acc + addend;
        if (relu) {
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = v[i] > 0.0f ? v[i] : 0.0f;
        }
        *reinterpret_cast<f32x4*>(out + frag_off) = v;
        if (more) t = t2;
    }
}

// (the four float64 helpers below are CALLED: inlined — tried in round 6 — the 2 KB / lane of scratch stays, it is the libm's
// private arrays, and 105 VGPRs of the network spill; the reservation costs nothing at launch: profiles/r06_scratch_launch.txt)
#define CN_NARROW_CALL __noinline__
// The decision behind the network (cn_sarl_sample_step), by the last workgroup of sarl_narrow_kernel: one wave per env.  Not
// inlined: its float64 reward / rotation code (registers, the libm's private arrays) stays out of the network's allocation.
__device__ CN_NARROW_CALL void narrow_decide(const SarlCfg& C, const SarlDecide& D, const double2* pos, const double2* goal,
                                           const double2* rv, int wave, int lane, const double* actions) {
    for (int b = wave; b < C.B; b += kNarrowWaves) {
        double bv = -__builtin_inf();
        int bi = -1;
        for (int a = lane; a < C.n_actions; a += kWaveSize) {
            const double v = __hip_atomic_load(&D.value[(size_t)b * C.n_actions + a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (v > bv) {
                bv = v;
                bi = a;
            }
        }
        sarl_pick_env(C, pos, goal, rv, actions, D.best, D.action, b, lane, bv, bi);
        if (lane == 0) {
            // alive: envs still sampling.  The episode-end flags of the PREVIOUS step are folded in here (explorer.py:56-65's
            // `while not done` per env) rather than by a kernel of their own behind cn_step.
            const bool keep = D.alive[b] && !(D.done && D.done[b]);
            D.alive[b] = keep ? 1 : 0;
            sarl_explore_env(C.B, C.n_actions, D.epsilon, D.mt_key, D.mt_pos, actions, !keep, D.best, D.action, nullptr, D.error, b);
        }
    }
}
// The joint state of env b for the replay memory (sarl_transform_row), on the idle wave of tile b
__device__ CN_NARROW_CALL void narrow_transform(const SarlCfg& C, const SarlDecide& D, const double2* pos, const double2* vel,
                                              const double2* goal, const double2* rv, const double* theta, int b, int h, bool maps) {
    sarl_transform_row(C, D.in_dim, D.sort_humans, pos, vel, goal, rv, theta, D.state_out, D.env_stride, b, h, maps);
}
// ... and its occupancy maps (the CURRENT human states, multi_human_rl.py:96-105) shared by the 64 lanes of that wave: a human's
// lane alone needs 30 us of float64 trigonometry for its map — longer than the whole network beside it
__device__ CN_NARROW_CALL void narrow_transform_maps(const SarlCfg& C, const SarlDecide& D, const double2* pos, const double2* vel, int b,
                                                   int lane, char* scratch) {
    const size_t g0 = (size_t)b * (C.H + 1);
    occupancy_maps_cooperative(
        C, 1, lane, kWaveSize, scratch,
        [&](int, int j, double& px, double& py, double& vx, double& vy) {
            px = pos[g0 + 1 + j].x, py = pos[g0 + 1 + j].y, vx = vel[g0 + 1 + j].x, vy = vel[g0 + 1 + j].y;
        },
        [] { wave_lds_sync(); },
        [&](int, int i) { return D.state_out + (size_t)b * D.env_stride + (size_t)i * D.in_dim + 13; });
}
// onestep_lookahead's reward of one (env, action) group, for the tile that holds it (not inlined: float64, the libm's arrays)
__device__ CN_NARROW_CALL double narrow_reward(const SarlCfg& C, const double2* pos, const double2* vel, const double2* goal,
                                             const double2* rv, const double* gtime, const double* theta, const double* actions,
                                             int b, int a) {
    return sarl_reward_of(C, pos, vel, goal, rv, gtime, theta, actions, b, a);
}

// LSTM (compile time): lstm_rl.ValueNetwork1 (lstm_rl.py:9-33) instead — the tile's rows are its 16 / H GROUPS, the humans are
// the LSTM's steps: X of step t is a row tile of its own (xs[t]), the input half of the gates of every step (W_ih x_t + b_ih)
// is computed up front with each wave holding its column tile of W_ih across the steps, the recurrent half with W_hh held in
// registers across them; then the joint MLP on [self_state | h].  dense_mfma<1>'s arithmetic layer by layer and the gate
// expressions of lstm_mlp_kernel: V is bit-identical to that kernel's.
// ATT (compile time; SARL, cn_sarl_select_attention): wave 0 also writes the weights of the tile's rows, att [n_groups][H].
template <bool LSTM = false, bool ATT = false>
__global__ __launch_bounds__(kNarrowThreads) void sarl_narrow_kernel(SarlNetRef net, SarlCfg C, const double2* pos, const double2* vel,
                                                                     const double2* goal, const double2* rv, const double* theta,
                                                                     const double* actions, const float* orca_vel, double* next_obs,
                                                                     float* V, SarlDecide D, const float* om, [[maybe_unused]] float* att = nullptr) {
    extern __shared__ float lds[];
    float* xs = lds;                          // [ks_x][64]  X of the tile
    float* bufA = xs + net.ks_x * 64;         // [ks_a][64]  wide hidden layers
    float* bufB = bufA + net.ks_a * 64;       // [ks_b][64]  mlp1 output (h2), then attention.2
    float* bufC = bufB + net.ks_b * 64;       // [ks_c][64]  mlp2 output (per-human feature)
    float* gbuf = bufC + net.ks_c * 64;       // [ks_b][64]  per row: the mean of h2 over the humans of the row's group
    float* jbuf = gbuf + net.ks_b * 64;       // [ks_a][64]  joint state (row = group) / value-head ping
    float* kbuf = jbuf + net.ks_a * 64;       // [ks_a][64]  global attention term
    float* mbuf = kbuf + net.ks_a * 64;       // [ks_a][64]  value-head pong
    float* sbuf = mbuf + net.ks_a * 64;       // [64]        attention scores -> weights (row r at word r)
    float* vbuf = sbuf + 64;                  // [kSarlThreads] partial sums of attention.4
    // LSTM: xs [H][ks_x][64] | gx [H][ks_g][64] input half of every step's gates | gates [ks_g][64] | hbuf [ks_h][64] |
    // cbuf [hid][16] | jbuf, kbuf [ks_a][64] | sbuf | vbuf   (net.nf = the hidden width; sarl_narrow_lds_bytes)
    const int lstm_ks_g = LSTM ? (int)((net.L[kL_mlp1_0].dims >> 8) & 0xffu) * 4 : 0, lstm_hid = LSTM ? net.nf : 0;
    float* const gx = xs + C.H * net.ks_x * 64;
    float* const gates = gx + C.H * lstm_ks_g * 64;
    float* const hbuf = gates + lstm_ks_g * 64;
    float* const cbuf = hbuf + sarl_ks(lstm_hid) * 64;
    if (LSTM) {
        jbuf = cbuf + lstm_hid * kSarlGroups, kbuf = jbuf + net.ks_a * 64, mbuf = kbuf;
        sbuf = kbuf + net.ks_a * 64, vbuf = sbuf + 64;
    }
    int* hc = reinterpret_cast<int*>(vbuf + kSarlThreads);  // [16] humans present in the tile's groups (H unless the `mixed` rule)
    int* const hl = hc + kSarlGroups;                       // [16] cn_sarl_sample_step: the group's env is still sampling
    int* const row_om = hl + kSarlGroups;                   // [16] (occupancy maps) where a row's map starts in `om`: wave 0's `wrow`, idle until the softmax
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int H = C.H, GT = kSarlGroups / H, rows = GT * H;
    // cn_sarl_sample_step on the two-launch route: an env whose episode is over (alive[b] && !done[b] is false: the flags as the
    // PREVIOUS call left them) needs no decision — a tile none of whose groups samples returns behind its prologue, the replay
    // state of such an env is not written, sarl_decide_step_kernel skips its transition.  A caller that streams calls past the
    // end of an episode (it cannot know the end without a round trip) pays two near-empty launches per dead step.
    const bool skip_dead = D.value != nullptr && D.counter == nullptr && D.alive != nullptr;
    const auto sampling = [&](int b) { return !skip_dead || (D.alive[b] != 0 && !(D.done != nullptr && D.done[b] != 0)); };
    // where row r = (group r / H, human r % H) of the tile keeps its features: its own row of the one X tile, or (LSTM) row
    // `group` of its human's X tile
    const auto xrow = [&](int r) { return LSTM ? (r % H) * net.ks_x * 64 + r / H : r; };
    const int n_groups = D.x_rows != nullptr ? D.ext_groups : C.B * C.n_actions;
    const size_t tile = blockIdx.x;
    const unsigned n_tiles = gridDim.x - (unsigned)D.side_wg;
    const SarlNetRef* n = &net;
    if (D.side_wg && blockIdx.x == n_tiles) {
        // cn_sarl_sample_step: the CURRENT joint state of every env for the replay memory (sarl_transform_row; nothing of it
        // depends on the network) by a workgroup of its own, beside the tiles on another CU — with occupancy maps a state is
        // ~5 us of float64 trigonometry even when a wave's lanes share it.  One wave per env.
        const bool coop = C.with_om && !D.sort_humans && occupancy_coop_ok(C, occupancy_coop_bytes(H), 1);
        char* scratch = reinterpret_cast<char*>(lds) + (size_t)wave * ((occupancy_coop_bytes(H) + 15) & ~(size_t)15);
        for (int b = wave; b < C.B; b += kNarrowWaves) {
            if (!sampling(b)) continue;
            if (lane < H) narrow_transform(C, D, pos, vel, goal, rv, theta, b, lane, !coop);
            if (coop) narrow_transform_maps(C, D, pos, vel, b, lane, scratch);
        }
        return;
    }
    CN_SARL_CLOCK_BEGIN();
    // (cadrl.ValueNetwork: its four layers live in the mlp3 slots)
    BTile cur = narrow_fetch(layer_of(*n, C.cadrl ? kL_mlp3_0 : kL_mlp1_0), wave, lane);
    // every word of LDS starts finite (k padding meets zero weights); meanwhile the tile's rows of X in registers
    {
        f32x4* z = reinterpret_cast<f32x4*>(lds);
        // ... vbuf included: narrow_k_loop reads 15 / 20 / 25 / 40 k-steps whatever the layer's kpad, so behind a last buffer (mbuf;
        // LSTM: kbuf) of fewer k-steps — any network narrower than the shipped ones — it runs on through sbuf into up to 9 k-steps
        // of vbuf, where words left by whatever held this LDS before would meet the zero weights as NaN
        for (int i = tid; i < (int)(vbuf + kSarlThreads - lds) / 4; i += kNarrowThreads) z[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }
    double my_reward = 0.0;
    const bool head_lane = wave == kNarrowWaves - 1 && lane < GT && tile * GT + lane < (size_t)n_groups;
    float f[13];
    bool row_valid = false;
    if (tid < rows) {
        const int g = tid / H, h = tid - g * H;
        const size_t G = tile * GT + g;
        row_valid = G < (size_t)n_groups;
        if (row_valid && D.x_rows != nullptr) {
            const float* xr = D.x_rows + (G * H + h) * 13;
#pragma unroll
            for (int k = 0; k < 13; ++k) f[k] = xr[k];
        } else if (row_valid)
            sarl_feature_row(C, (int)(G / C.n_actions), (int)(G % C.n_actions), h, pos, goal, rv, theta, actions, next_obs, vel,
                             orca_vel, f);
        if (h == 0) {  // len(state.human_states): under the `mixed` rule the env's absent humans are parked behind the present ones
            int present = H;
            if (row_valid && D.x_rows == nullptr) {
                const size_t e0 = (G / C.n_actions) * (size_t)(H + 1);
                present = 0;
                for (int j = 0; j < H; ++j) present += is_parked(pos[e0 + 1 + j]) ? 0 : 1;
            }
            hc[g] = present;
            hl[g] = (row_valid && (D.x_rows != nullptr || sampling((int)(G / C.n_actions)))) ? 1 : 0;
        }
        // (occupancy maps) where this row's map starts in `om`
        if (om != nullptr) row_om[tid] = row_valid ? (int)(((G / C.n_actions) * H + h) * (size_t)(D.in_dim - 13)) : -1;
    }
    lds_barrier();
    CN_SARL_TICK(0);
    if (skip_dead) {
        int live = 0;
        for (int g = 0; g < GT; ++g) live |= hl[g];
        if (live == 0) return;  // (uniform: every thread reads the same words)
    }
    if (row_valid) {
        float* const x = xs + xrow(tid);
#pragma unroll
        for (int k = 0; k < 13; ++k) x[tile_word(k)] = f[k];
    }
    if (om != nullptr) {
        // occupancy maps (multi_human_rl.py:46-49): columns 13.. of a row are its human's map among the humans' NEXT states —
        // the same for every action of the env (sarl_lookahead_kernel or the previous call's sarl_decide_step_kernel wrote
        // them).  Four consecutive cells per thread (one 16-byte load), the row's offset into `om` from its own thread (row_om)
        // A row of `om` starts at a multiple of `extra` floats: 16-byte aligned for every row only when the map width is a multiple
        // of four (16 x 3 at the shipped size).  Any other width takes the scalar loop for the whole row.
        const int extra = D.in_dim - 13, quads = (extra & 3) == 0 ? extra >> 2 : 0, rest = extra - 4 * quads;
        for (int i = tid; i < rows * quads; i += kNarrowThreads) {
            const int r = i / quads, q = i - r * quads;
            const int base = row_om[r];
            if (base >= 0) {
                const f32x4 m = *reinterpret_cast<const f32x4*>(om + base + 4 * q);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int kk = 13 + 4 * q + j;
                    xs[tile_word(kk) + xrow(r)] = m[j];
                }
            }
        }
        for (int i = tid; i < rows * rest; i += kNarrowThreads) {  // (a map width that is not a multiple of four)
            const int r = i / rest, k = 4 * quads + i - r * rest;
            const int base = row_om[r], kk = 13 + k;
            if (base >= 0) xs[tile_word(kk) + xrow(r)] = om[base + k];
        }
    }
    BTile nxt = narrow_fetch(layer_of(*n, C.cadrl ? kL_mlp3_2 : kL_mlp1_2), wave, lane);
    lds_barrier();
    CN_SARL_TICK(1);
    // What every tile does with the V of its groups (on the value head's wave), and what follows it under cn_sarl_sample_step
    const auto finish = [&](float v) {
        int arrived = 0;
        if (wave == kNarrowWaves - 1) {
            if (head_lane) {
                const size_t G = tile * GT + lane;
                V[G] = v;
                // multi_human_rl.py:52, as sarl_select_env.  An agent-scope atomic store: written through to where every XCD's
                // agent-scope load finds it — no write-back of this XCD's whole L2 (a release fence) for 3 doubles
                if (D.value)
                    __hip_atomic_store(&D.value[G], my_reward + C.gamma_bar * (double)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            if (D.counter) {
                __builtin_amdgcn_s_waitcnt(0x0f70);  // vmcnt(0): the stores above have been acknowledged before the tile counts as arrived
                if (lane == 0) arrived = atomicAdd(D.counter, 1) + 1;
            }
        }
        if (!D.counter) return;  // cn_sarl_select, or the decision is sarl_decide_step_kernel's: the network only
        // ---- the workgroup that finishes LAST decides for every env, one wave per env — arg-max of reward + gamma V, the
        // epsilon-greedy draw on the env's own stream (sarl_explore_env) — instead of three more launches behind this one (the
        // joint state for the replay memory was written by tile b meanwhile).
        int* last = reinterpret_cast<int*>(sbuf);
        if (wave == kNarrowWaves - 1 && lane == 0) {
            *last = arrived == (int)n_tiles ? 1 : 0;
            if (*last) atomicExch(D.counter, 0);  // ready for the next launch
        }
        __syncthreads();
        if (!*last) return;
        narrow_decide(C, D, pos, goal, rv, wave, lane, actions);
    };
    const auto reward_of_my_group = [&]() {
        // cn_sarl_sample_step: the reward of the tile's groups on the lanes that will hold their V — the value head's wave, which has
        // no column tile of the 100-wide layers: this float64 chain runs beside a 100-wide layer's MFMAs.  The decision behind the
        // network then only compares reward + gamma V.
        if (D.value && head_lane) {
            const size_t G = tile * GT + lane;
            my_reward = narrow_reward(C, pos, vel, goal, rv, D.gtime, theta, actions, (int)(G / C.n_actions), (int)(G % C.n_actions));
            D.reward[G] = my_reward;
        }
    };
    const auto replay_state_of_my_env = [&]() {
        // ... and (without the side workgroup) the CURRENT joint state of env b for the replay memory, by tile b's idle wave.
        // A small action table has fewer tiles than envs (one human, 13 actions, 6 envs: 5 tiles): the tiles stride over the envs.
        if (D.value && D.state_out && !D.side_wg && wave == kNarrowWaves - 1) {
            // (occupancy maps: the wave's lanes share them; mbuf — the value head's pong buffer — is idle until mlp3.0)
            const bool coop = C.with_om && !D.sort_humans && occupancy_coop_ok(C, sizeof(float) * 64 * (size_t)net.ks_a, 1);
            for (size_t b = tile; b < (size_t)C.B; b += n_tiles) {
                if (!sampling((int)b)) continue;
                if (lane < H) narrow_transform(C, D, pos, vel, goal, rv, theta, (int)b, lane, !coop);
                if (coop) narrow_transform_maps(C, D, pos, vel, (int)b, lane, reinterpret_cast<char*>(mbuf));
            }
        }
    };
    if constexpr (LSTM) {
        const int hid = lstm_hid, ks_g = lstm_ks_g;
        const PackedLinear Pi = layer_of(*n, kL_mlp1_0), Ph = layer_of(*n, kL_mlp1_2);  // weight_ih_l0 + bias_ih, weight_hh_l0 + bias_hh
        const int col = lane & 15, quad = lane >> 4;
        // W_hh: 4 hid / 16 column tiles on eight waves — both of a wave's tiles stay in registers across the steps (`nxt`: tile `wave`)
        BTile hh2 = narrow_fetch(Ph, wave + kNarrowWaves, lane);
        {   // the input half of the gates of EVERY step: gx[t] = W_ih x_t + b_ih (dense_mfma<1> with no extra term)
            BTile t = cur;
            for (int ct = wave; ct < Pi.ctiles; ct += kNarrowWaves) {
                const bool more = ct + kNarrowWaves < Pi.ctiles;
                BTile t2;
                if (more) t2 = narrow_fetch(Pi, ct + kNarrowWaves, lane);
                const int frag_off = ((ct * 4 + (col >> 2)) * 64) + (col & 3) * 16 + quad * 4;
                const f32x4 addend = {t.bias, t.bias, t.bias, t.bias};
                for (int tt = 0; tt < H; ++tt) {
                    const float* afrag = xs + tt * net.ks_x * 64 + lane;
                    const f32x4 acc = Pi.kpad <= 3 * kSarlKChunk ? narrow_k_loop<3>(afrag, t) : narrow_k_loop<4>(afrag, t);
                    *reinterpret_cast<f32x4*>(gx + tt * ks_g * 64 + frag_off) = acc + addend;
                }
                if (more) t = t2;
            }
        }
        reward_of_my_group();      // (the value head's wave has one column tile of W_ih where waves 0..4 have two)
        replay_state_of_my_env();
        cur = narrow_fetch(layer_of(*n, kL_mlp3_0), wave, lane);
        lds_barrier();
        for (int t = 0; t < H; ++t) {
            // gates = (W_hh h + b_hh) + gx[t]: h = 0 at the first step, multiplied out like every other (lstm_mlp_kernel does)
#pragma unroll
            for (int ci = 0; ci < 2; ++ci) {
                const int ct = wave + ci * kNarrowWaves;
                if (ct < Ph.ctiles) {
                    const BTile& w = ci ? hh2 : nxt;
                    const int frag_off = ((ct * 4 + (col >> 2)) * 64) + (col & 3) * 16 + quad * 4;
                    f32x4 addend = {w.bias, w.bias, w.bias, w.bias};
                    addend += *reinterpret_cast<const f32x4*>(gx + t * ks_g * 64 + frag_off);
                    const f32x4 acc = narrow_k_loop<3>(hbuf + lane, w);
                    *reinterpret_cast<f32x4*>(gates + frag_off) = acc + addend;
                }
            }
            lds_barrier();
            for (int i = tid; i < hid * kSarlGroups; i += kNarrowThreads) {
                const int g = i & 15, j = i >> 4;
                if (g >= GT || t >= hc[g]) continue;  // (`mixed` rule: this group's episode has fewer humans)
                auto at = [&](int k) { return gates[tile_word(k) + g]; };
                const float ig = 1.0f / (1.0f + expf(-at(j)));
                const float fg = 1.0f / (1.0f + expf(-at(hid + j)));
                const float gg = tanhf(at(2 * hid + j));
                const float og = 1.0f / (1.0f + expf(-at(3 * hid + j)));
                const float c = fg * cbuf[i] + ig * gg;
                cbuf[i] = c;
                hbuf[tile_word(j) + g] = og * tanhf(c);
            }
            lds_barrier();
        }
        nxt = narrow_fetch(layer_of(*n, kL_mlp3_2), wave, lane);
        // joint state [self_state = state[:, 0, :6] | h_n], row = group (lstm_rl.py:29-31)
        copy_self_state(jbuf, xs, tid, GT);
        for (int i = tid; i < hid * kSarlGroups; i += kNarrowThreads) {
            const int g = i & 15, j = i >> 4, f = 6 + j;
            if (g < GT) jbuf[(f >> 2) * 64 + (f & 3) * 16 + g] = hbuf[tile_word(j) + g];  // (tile_word(f), spelled out: the call moves this kernel's assembly)
        }
        lds_barrier();
        dense_narrow(layer_of(*n, kL_mlp3_0), jbuf, kbuf, true, nullptr, wave, lane, cur);
        cur = narrow_fetch(layer_of(*n, kL_mlp3_4), wave, lane);
        lds_barrier();
        dense_narrow(layer_of(*n, kL_mlp3_2), kbuf, jbuf, true, nullptr, wave, lane, nxt);
        nxt = narrow_fetch(layer_of(*n, kL_mlp3_6), wave, lane);
        lds_barrier();
        dense_narrow(layer_of(*n, kL_mlp3_4), jbuf, kbuf, true, nullptr, wave, lane, cur);
        lds_barrier();
        dense_narrow(layer_of(*n, kL_mlp3_6), kbuf, jbuf, false, nullptr, wave, lane, nxt);  // column 0 of the tile: row r at word r
        lds_barrier();
        const float v = (wave == kNarrowWaves - 1 && lane < GT) ? jbuf[lane] : 0.0f;
        CN_SARL_CLOCK_END();
        finish(v);
        return;
    }
    if (C.cadrl) {
        // cadrl.ValueNetwork (cadrl.py:22-29): the same MLP for every (robot, human) row — cadrl_mlp_kernel's four layers on the
        // tile's 16 rows — then the minimum over the humans of a group (cadrl.py:162-163: the first minimum's value)
        dense_narrow(layer_of(*n, kL_mlp3_0), xs, bufA, true, nullptr, wave, lane, cur);
        cur = narrow_fetch(layer_of(*n, kL_mlp3_4), wave, lane);
        lds_barrier();
        dense_narrow(layer_of(*n, kL_mlp3_2), bufA, bufB, true, nullptr, wave, lane, nxt);
        reward_of_my_group();
        nxt = narrow_fetch(layer_of(*n, kL_mlp3_6), wave, lane);
        lds_barrier();
        dense_narrow(layer_of(*n, kL_mlp3_4), bufB, bufA, true, nullptr, wave, lane, cur);
        replay_state_of_my_env();
        lds_barrier();
        dense_narrow(layer_of(*n, kL_mlp3_6), bufA, kbuf, false, nullptr, wave, lane, nxt);  // column 0 of the tile: row r at word r
        lds_barrier();
        float m = 0.0f;
        if (wave == kNarrowWaves - 1 && lane < GT) m = first_min_over_humans(kbuf, 1, lane * H, 1, H, hc[lane], kbuf[lane * H]);
        CN_SARL_CLOCK_END();
        finish(m);
        return;
    }
    // self_state = state[:, 0, :6] (sarl.py:36): the first human's row of the group
    float self_val = 0.0f;
    const int sg = tid & 15, sf = tid >> 4;
    if (tid < kSarlGroups * 6 && sg < GT) self_val = xs[tile_word(sf) + sg * H];
    dense_narrow(layer_of(*n, kL_mlp1_0), xs, bufA, true, nullptr, wave, lane, cur);
    cur = narrow_fetch(layer_of(*n, kL_mlp2_0), wave, lane);
    lds_barrier();
    CN_SARL_TICK(2);
    dense_narrow(layer_of(*n, kL_mlp1_2), bufA, bufB, true, nullptr, wave, lane, nxt);  // h2
    reward_of_my_group();
    nxt = narrow_fetch(layer_of(*n, kL_mlp2_2), wave, lane);
    lds_barrier();
    CN_SARL_TICK(3);
    if (n->with_global) {
        // the mean of h2 over a group's humans, once per (feature word, group) and copied to the group's H rows (it was summed
        // again for every row: five times the loads and divisions; rows beyond the tile's stay zero from the start)
        for (int i = tid; i < n->ks_b * 4 * GT; i += kNarrowThreads) {
            const int g = i % GT, first = (i / GT) * 16 + g * H;
            const int cnt = hc[g];
            float sum = 0.0f;
            for (int h = 0; h < H; ++h) sum += h < cnt ? bufB[first + h] : 0.0f;  // (as sarl_mlp_pipe_kernel masks a `mixed` episode)
            const float mean = sum / (float)cnt;
            for (int h = 0; h < H; ++h) gbuf[first + h] = mean;
        }
    }
    dense_narrow(layer_of(*n, kL_mlp2_0), bufB, bufA, true, nullptr, wave, lane, cur);
    replay_state_of_my_env();
    cur = narrow_fetch(layer_of(*n, kL_att0_global), wave, lane);
    lds_barrier();
    CN_SARL_TICK(4);
    dense_narrow(layer_of(*n, kL_mlp2_2), bufA, bufC, false, nullptr, wave, lane, nxt);  // features
    nxt = narrow_fetch(layer_of(*n, kL_att0_local), wave, lane);
    if (n->with_global) dense_narrow(layer_of(*n, kL_att0_global), gbuf, kbuf, false, nullptr, wave, lane, cur);
    cur = narrow_fetch(layer_of(*n, kL_att_2), wave, lane);
    lds_barrier();
    CN_SARL_TICK(5);
    dense_narrow(layer_of(*n, kL_att0_local), bufB, bufA, true, n->with_global ? kbuf : nullptr, wave, lane, nxt);
    nxt = narrow_fetch(layer_of(*n, kL_mlp3_0), wave, lane);
    lds_barrier();
    CN_SARL_TICK(6);
    dense_narrow(layer_of(*n, kL_att_2), bufA, bufB, true, nullptr, wave, lane, cur);
    cur = narrow_fetch(layer_of(*n, kL_mlp3_2), wave, lane);
    lds_barrier();
    CN_SARL_TICK(7);
    float* const wrow = reinterpret_cast<float*>(hl + kSarlGroups) + wave * 16;  // this wave's copy of the attention weights
    {   // attention.4 (one output) as dense_vec1<H> slices it: kSarlThreads / (16 H) k slices per row, summed in slice order
        const PackedLinear P = layer_of(*n, kL_att_4);
        const int slices = kSarlThreads / (H * 16);
        for (int i = tid; i < slices * 16; i += kNarrowThreads) {
            const int row = i & 15, slice = i >> 4;
            vbuf[slice * 16 + row] = dot_k_slice(P, bufB, row, slice, slices);
        }
        lds_barrier();
        CN_SARL_TICK(8);
        // EVERY wave: lane = row (four copies per wave): its score, then the softmax without max subtraction over the group's
        // humans (sarl.py:52-53) — into the wave's OWN copy of the weights, so that the joint state below follows without another
        // workgroup barrier (round 6: wave 0 alone computed them and seven waves waited at a barrier of their own)
        {
            const int r = lane & 15;
            const float v = fold_k_slices(P, vbuf, 16, r, slices);
            const int g0 = (r / H) * H;
            const bool present = r < rows ? (r - g0) < hc[r / H] : true;
            const float e = present ? masked_exp(v) : 0.0f;
            float total = 0.0f;
            for (int h = 0; h < H; ++h) total += __shfl(e, (g0 + h) & 15);  // (row 15 of 3 x 5 wraps: unused)
            if (lane < 16) wrow[lane] = e / total;
            if constexpr (ATT)
                if (wave == 0 && lane < rows && tile * GT + lane / H < (size_t)n_groups) att[tile * rows + lane] = wrow[lane];
        }
    }
    wave_lds_sync();
    CN_SARL_TICK(9);
    // the joint state, row = group: self features, weighted feature sum (sarl.py:60); everything else of jbuf is zero
    if (tid < kSarlGroups * 6 && sg < GT) jbuf[tile_word(sf) + sg] = self_val;
    const int nf = n->nf;
    for (int i = tid; i < GT * nf; i += kNarrowThreads) {  // (group, feature): the groups the tile really holds
        const int g = i % GT, c = i / GT;
        const int src = tile_word(c) + g * H;
        float sum = 0.0f;
        for (int h = 0; h < H; ++h) sum += wrow[g * H + h] * bufC[src + h];
        const int f = 6 + c;
        jbuf[tile_word(f) + g] = sum;
    }
    lds_barrier();
    CN_SARL_TICK(10);
    dense_narrow(layer_of(*n, kL_mlp3_0), jbuf, mbuf, true, nullptr, wave, lane, nxt);
    nxt = narrow_fetch(layer_of(*n, kL_mlp3_4), wave, lane);
    lds_barrier();
    CN_SARL_TICK(11);
    dense_narrow(layer_of(*n, kL_mlp3_2), mbuf, jbuf, true, nullptr, wave, lane, cur);
    lds_barrier();
    CN_SARL_TICK(12);
    dense_narrow(layer_of(*n, kL_mlp3_4), jbuf, mbuf, true, nullptr, wave, lane, nxt);
    lds_barrier();
    CN_SARL_TICK(13);
    float v = 0.0f;
    if (wave == kNarrowWaves - 1) v = dot_on_one_wave(layer_of(*n, kL_mlp3_6), mbuf, lane);  // mlp3.6 as value_head_on_one_wave
    CN_SARL_TICK(14);
    CN_SARL_CLOCK_END();
    finish(v);
}
__host__ inline size_t sarl_narrow_lds_bytes(const SarlNet& net, bool lstm = false) {
    if (lstm) {  // sarl_narrow_kernel<true>'s carve: xs, gx, gates, hbuf, cbuf, jbuf, kbuf, sbuf, vbuf, hc
        const size_t H = (size_t)net.H, ks_g = (size_t)net.L[kL_mlp1_0].ctiles * 4, hid = (size_t)net.L[kL_mlp1_2].K;
        return sizeof(float) * (64 * (H * net.ks_x + H * ks_g + ks_g + (size_t)sarl_ks((int)hid) + 2 * (size_t)net.ks_a + 1) +
                                hid * kSarlGroups + kSarlThreads + (2 + kNarrowWaves) * kSarlGroups);
    }
    return sizeof(float) * (64 * (size_t)(net.ks_x + 4 * net.ks_a + 2 * net.ks_b + net.ks_c + 1) + kSarlThreads + (2 + kNarrowWaves) * kSarlGroups);
}

}  // namespace cn
