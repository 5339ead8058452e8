// sarl.ValueNetwork.forward (crowd_nav/policy/sarl.py:28-65) with the ACTIVATIONS IN REGISTERS: the shipped widths
// (mlp1 150-100, mlp2 100-50, attention 100-100-1 with the global state, mlp3 150-100-100-1) and 5 humans.
//
// The LDS kernels (sarl_lds_kernels.h) compute Y = X W^T with the activations as the MFMA A operand: a layer's output has to
// travel through LDS to become the next layer's input, every layer ends in a workgroup barrier, and 7 column tiles on 16
// waves leave the MFMA pipes 54 % busy.  Here a wave computes Y^T = W X^T for ITS OWN 16 (env, action) groups x 5 humans
// (5 "N tiles" of 16 rows) through the whole network:
//
//   * A operand = weights (16 output features x 4 inputs), B operand = activations (4 inputs x 16 rows).  The accumulator
//     of v_mfma_f32_16x16x4_f32 holds, in lane l, rows 4*(l>>4) .. +3 of column l&15 — four OUTPUT FEATURES of one ROW —
//     and the B operand of a k-step wants, in lane l, input feature 4*ks + (l>>4) of row l&15.  With the output features of
//     a 16-feature tile dealt to the accumulator rows as  slot m = 4*lg + s  <->  feature 16*t + 4*s + lg  (a 4 x 4
//     transpose, done once in the weight packing), register s of output tile t IS the B operand of k-step 4*t + s of the
//     next layer.  No LDS, no barrier, no data movement between layers: bias is the accumulator's initial value, ReLU one
//     v_max per register.
//   * The reductions over a group's humans (mean for the global state, masked softmax, weighted feature sum) combine the
//     same register of the wave's 5 N tiles: lane-local.
//   * Weights stream from L2 (L1-shared by the 4 waves of a workgroup, which run the same sequence) in the exact order of
//     use as ONE linear array of 1-KiB "quads" (lane l: 4 consecutive k-steps of one output tile, or the bias of a tile),
//     kRegDepth quads ahead, across layer and tile boundaries — a wave never waits for a layer to start.
//   * One wave per SIMD (up to 512 registers: at most 310 activations live — the 80 registers of per-human features wait in
//     wave-private LDS while the attention layers run), 20 independent MFMAs per weight quad.
//
// Arithmetic: each output is the fma chain  bias, then inputs in ascending k  (the MFMA's own order) — the same products as
// the LDS kernels, which add the bias last; both within 1e-6 of torch (tests/test_sarl.py).
#pragma once
#include "sarl_reg_stream.h"

namespace cn {

__global__ void sarl_reg_pack_kernel(RegPackPlan plan, float* stream) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int xks = plan.xks;
    const int total = reg_total_quads(xks);
    if (idx >= total * 256) return;
    const int quad = idx >> 8, lane = (idx >> 2) & 63, kk = idx & 3;
    const int lg = lane >> 4, m = lane & 15;
    float v = 0.0f;
    int l = 0, base = 0;
    const int n_layers = reg_layers(xks);
    while (l < n_layers && quad >= base + reg_layer_quads(l, xks)) base += reg_layer_quads(l++, xks);
    if (l < n_layers) {
        const RegShape s = reg_shape(l, xks);
        const int S = reg_tile_quads(l, xks);
        const RegPackLayer& L = plan.L[l];
        const int r = quad - base;
        int mt, j;
        const int pairs = s.paired ? s.mt / 2 : 0;
        if (r < pairs * 2 * S) {
            const int rr = r % (2 * S);
            mt = 2 * (r / (2 * S)) + (rr & 1), j = rr >> 1;
        } else {
            const int r2 = r - pairs * 2 * S;
            mt = 2 * pairs + r2 / S, j = r2 % S;
        }
        if (reg_is_gates(xks)) {
            // output tile mt = units 4 mt .. 4 mt + 3: accumulator register kk of lane group lg = gate kk (torch order i, f, g, o)
            // of unit 4 mt + lg, so that a tile's f32x4 is everything the cell update of its 4 units needs and the new hidden
            // state lands in the B-operand layout of k-step mt
            if (j == 0) {
                const int u = 4 * mt + lg;
                v = u < kRegLstmHid ? L.b[kk * kRegLstmHid + u] + L.b2[kk * kRegLstmHid + u] : 0.0f;
            } else {
                const int ks = 4 * (j - 1) + kk, u = 4 * mt + (m >> 2), n = (m & 3) * kRegLstmHid + u;
                if (u < kRegLstmHid && ks < s.ks) {
                    if (ks < L.k_split) v = 4 * ks + lg < L.K ? L.W[(size_t)n * L.ldw + 4 * ks + lg] : 0.0f;
                    else v = 4 * (ks - L.k_split) + lg < kRegLstmHid ? L.W2[(size_t)n * kRegLstmHid + 4 * (ks - L.k_split) + lg] : 0.0f;
                }
            }
        } else if (s.bias && j == 0) {  // accumulator register kk of lane group lg = feature 16 mt + 4 kk + lg
            const int f = L.replicate ? 0 : 16 * mt + 4 * kk + lg;
            v = (L.b && f < L.N) ? L.b[f] : 0.0f;
        } else {
            const int ks = 4 * (j - s.bias) + kk;
            const int n = L.replicate ? 0 : 16 * mt + 4 * (m & 3) + (m >> 2);
            const int col = ks < s.ks ? reg_kcol(xks, l, L.K, L.k_off, ks, lg) : -1;
            v = (n < L.N && col >= 0) ? L.W[(size_t)n * L.ldw + col] : 0.0f;
        }
    }
    stream[idx] = v;
}

// X: the feature kernel's fragment order, X[((tile * 5 + h) * ks_x + ks) * 64 + lane] = feature 4 ks + (lane >> 4) of human h
// of group lane & 15 — exactly the B operand of k-step ks.  V[group] out.  Persistent: wave w of the grid takes tiles
// w, w + waves, ...; the next tile's X is requested while the value head of the current one runs.
// XKS = k-steps of the input read from X: only 4 is instantiated (13 rotated features; the 48 occupancy-map features of the 61-wide
// input do not depend on the action and come in through PRE, not as 81 copies inside X).
// NT = humans of the crowd (N tiles per wave), 1..5.  With NT = 1 the MFMAs of a k-step chain are dependent (40 instead of 32
// cycles each); from 2 humans on consecutive MFMAs alternate between accumulators.
// PRE (XKS = 4): `om` is the term of sarl_om_term_kernel, [env][human][10 tiles][4 lane groups][4 registers] — mlp1.0's
// accumulator for (row, output tile) in the lane's own order, one 16-byte load each, requested one output tile ahead.
// ATT (compile time; cn_sarl_select_attention): lanes 0..15 also write their group's softmax weights, att_out [n_groups][NT].
template <int XKS, int NT, bool PRE = false, bool ATT = false>
__global__ __launch_bounds__(kRegWaves * 64) void sarl_reg_kernel(const float* stream, const float* X, float* V, int n_groups,
                                                                  int n_tiles, int ks_x, const int* hcount,
                                                                  const float* om = nullptr, int n_actions = 1,
                                                                  [[maybe_unused]] float* att_out = nullptr) {
    static_assert(NT >= 1 && NT <= kRegHumans, "the activations of at most 5 humans fit the register file");
    static_assert(XKS == 4, "k-steps 4..15 of a 61-wide input are the hoisted occupancy-map term (PRE), never part of X");
    constexpr int KEY = PRE ? kRegSarlPre : XKS;
    constexpr int QT = reg_total_quads(KEY);
    const int lane = threadIdx.x & 63;
    const int wid = blockIdx.x * kRegWaves + (threadIdx.x >> 6), nw = gridDim.x * kRegWaves;
    RegStreamT<(NT == kRegHumans ? 6 : kRegDepth)> ws;
    ws.rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(stream), 0, QT * 1024, 0x00020000);  // raw, 32-bit elements
    ws.voff = (uint32_t)lane * 16u;
#pragma unroll
    for (int i = 0; i < ws.kDepth; ++i) ws.q[i] = reg_quad(ws, i);
    if (wid >= n_tiles) return;
    const gfloat_p Xg = as_global(X) + lane;
    float x[NT][XKS];
    int cnt;
    const auto load_x = [&](int t) {
        const gfloat_p xt = Xg + (size_t)t * NT * ks_x * 64;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int ks = 0; ks < XKS; ++ks) x[nt][ks] = xt[(nt * ks_x + ks) * 64];
    };
    load_x(wid < n_tiles ? wid : 0);
    cnt = hcount[(size_t)(wid < n_tiles ? wid : 0) * kSarlGroups + (lane & 15)];
    // PRE: mlp1.0's start values, output tile mt of N tile nt in pre[mt][nt] — all 10 x NT of the NEXT group tile are requested
    // with its X, when the value head starts and 200 registers fall free (one output tile ahead was too late: 20 MFMAs are 640
    // cycles, a loaded L2 answers later: 1.964 ms instead of 1.88)
    // Buffer loads as for the weight stream: ONE lane offset (the env's rows, the lane group's 16 bytes), the (nt, mt) part in the
    // instruction's immediate — with global_load the 50 64-bit addresses were 350 VALU instructions per tile.
    f32x4 pre[PRE ? 10 : 1][PRE ? NT : 1];
    __amdgpu_buffer_rsrc_t prsrc = ws.rsrc;
    if constexpr (PRE)
        prsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(om), 0, (int)(((long long)n_groups / n_actions) * NT * 640), 0x00020000);
    const auto load_pre = [&](int t) {
        const long long G = (long long)t * kSarlGroups + (lane & 15);
        const int env = (int)((G < n_groups ? G : (long long)n_groups - 1) / n_actions);
        const uint32_t voff = (uint32_t)env * (NT * 640u) + (uint32_t)(lane >> 4) * 16u;
#pragma unroll
        for (int mt = 0; mt < 10; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                pre[mt][nt] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(prsrc, voff + (nt * 40 + mt * 4) * 16, 0, 0));
    };
    if constexpr (PRE) load_pre(wid);
    // per-human features (mlp2 output, 80 registers) wait in LDS while the attention layers run: wave-private, no barrier
    __shared__ f32x4 park[kRegWaves][NT * 4][64];
    f32x4(*const mypark)[64] = park[threadIdx.x >> 6];
    const auto none = [](int) { return f32x4{0.0f, 0.0f, 0.0f, 0.0f}; };
    CN_SARL_CLOCK_BEGIN();
    for (int tile = wid; tile < n_tiles; tile += nw) {
        const float self0 = x[0][0], self1 = x[0][1];  // features 0..3 / 4..7 of human 0's row: the self state lives in 0..5
        f32x4 att[NT][7];
        {
            f32x4 h2[NT][7];
            {
                f32x4 h1[NT][10];
                if constexpr (PRE)
                    reg_dense_arr<KEY, kR_mlp1_0, NT, true>(
                        ws, [&](int nt, int ks) { return x[nt][ks]; },
                        [&](int nt, int mt) { return pre[mt][nt]; },
                        h1);
                else
                    reg_dense_arr<KEY, kR_mlp1_0, NT, true>(ws, [&](int nt, int ks) { return x[nt][ks]; }, none, h1);
                CN_SARL_TICK(1);
                reg_dense_arr<KEY, kR_mlp1_2, NT, false>(ws, [&](int nt, int ks) { return h1[nt][ks >> 2][ks & 3]; }, none, h2);
                CN_SARL_TICK(2);
            }
            {
                f32x4 t1[NT][7];
                reg_dense_arr<KEY, kR_mlp2_0, NT, true>(ws, [&](int nt, int ks) { return h2[nt][ks >> 2][ks & 3]; }, none, t1);
                CN_SARL_TICK(3);
                reg_dense<KEY, kR_mlp2_2, NT, false>(ws, [&](int nt, int ks) { return t1[nt][ks >> 2][ks & 3]; }, none,
                                                     [&](int nt, int mt, f32x4 v) { mypark[nt * 4 + mt][lane] = v; });
                CN_SARL_TICK(4);
            }
            // global state: mean over the humans present (sarl.py:42), elementwise over the 5 N tiles
            f32x4 gterm[7];
            {
                f32x4 gm[7];
                const float fc = (float)cnt;
#pragma unroll
                for (int t = 0; t < 7; ++t) {
                    f32x4 sum = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                        for (int i = 0; i < 4; ++i) sum[i] += nt < cnt ? h2[nt][t][i] : 0.0f;
#pragma unroll
                    for (int i = 0; i < 4; ++i) gm[t][i] = sum[i] / fc;
                }
                // attention.0 on [h2 | mean]: the global half (+ the layer's bias) is one N tile, shared by the 5 humans
                reg_dense1<KEY, kR_att0_global, false>(ws, [&](int ks) { return gm[ks >> 2][ks & 3]; }, gterm);
                CN_SARL_TICK(5);
            }
            f32x4 a0[NT][7];
            reg_dense_arr<KEY, kR_att0_local, NT, true>(ws, [&](int nt, int ks) { return h2[nt][ks >> 2][ks & 3]; },
                                                        [&](int mt) { return gterm[mt]; }, a0);
            CN_SARL_TICK(6);
            reg_dense_arr<KEY, kR_att_2, NT, false>(ws, [&](int nt, int ks) { return a0[nt][ks >> 2][ks & 3]; }, none, att);
            CN_SARL_TICK(7);
        }
        f32x4 wf[4];
        {
            float sc[NT];  // attention.4: the score of (human, group) in every register of the group's lanes
            // (stays on the matrix side although it is one output: the reference masks a score that is EXACTLY zero, sarl.py:52, and
            // a sum in another order lands on that discontinuity for other rows — one of 1.66 M at the benchmark size, measured)
            reg_dense<KEY, kR_att_4, NT, false>(ws, [&](int nt, int ks) { return att[nt][ks >> 2][ks & 3]; }, none,
                                                [&](int nt, int, f32x4 v) { sc[nt] = v[0]; });
            CN_SARL_TICK(8);
            // masked softmax without max subtraction (sarl.py:52-53); an absent human carries no weight
            float e[NT], total = 0.0f;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const float s = sc[nt];
                e[nt] = nt < cnt ? expf(s) * (s != 0.0f ? 1.0f : 0.0f) : 0.0f;
                total += e[nt];
            }
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) e[nt] = e[nt] / total;
            if constexpr (ATT) {  // the weights as they stand (absent humans 0), from the lanes that own a group
                const size_t G = (size_t)tile * kSarlGroups + lane;
                if (lane < kSarlGroups && G < (size_t)n_groups)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) att_out[G * NT + nt] = e[nt];
            }
            // weighted feature sum (sarl.py:60)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                f32x4 sum = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const f32x4 f = mypark[nt * 4 + t][lane];
#pragma unroll
                    for (int i = 0; i < 4; ++i) sum[i] += e[nt] * f[i];
                }
                wf[t] = sum;
            }
        }
        CN_SARL_TICK(9);
        // the next tile's input (and this tile's last use of x is behind us)
        const int next = tile + nw < n_tiles ? tile + nw : tile;
        load_x(next);
        if constexpr (PRE) load_pre(next);
        const int cnt_next = hcount[(size_t)next * kSarlGroups + (lane & 15)];
        // value head on joint = [self | weighted feature] (sarl.py:61-62)
        f32x4 j1[10], j2[7], j3[7], val[1];
        const float mix = lane < 32 ? wf[3][0] : self0;
        reg_dense1<KEY, kR_mlp3_0, true>(
            ws, [&](int ks) { return ks < 12 ? wf[ks >> 2][ks & 3] : ks == 12 ? mix : ks == 13 ? self1 : self0; }, j1);
        CN_SARL_TICK(10);
        reg_dense1<KEY, kR_mlp3_2, true>(ws, [&](int ks) { return j1[ks >> 2][ks & 3]; }, j2);
        CN_SARL_TICK(11);
        reg_dense1<KEY, kR_mlp3_4, true>(ws, [&](int ks) { return j2[ks >> 2][ks & 3]; }, j3);
        CN_SARL_TICK(12);
        reg_dense1<KEY, kR_mlp3_6, false>(ws, [&](int ks) { return j3[ks >> 2][ks & 3]; }, val);
        if (lane < kSarlGroups) {
            const size_t G = (size_t)tile * kSarlGroups + lane;
            if (G < (size_t)n_groups) V[G] = val[0][0];
        }
        cnt = cnt_next;
        // the stream position wraps to quad 0 here: the padding quads are consumed so that slot I % kRegDepth stays aligned
#pragma unroll
        for (int i = reg_qbase(reg_layers(KEY), KEY); i < QT; ++i) (void)reg_take<QT>(ws, i);
        CN_SARL_TICK(13);
    }
    CN_SARL_CLOCK_END_N((n_tiles - wid + nw - 1) / nw);
}

// b + W[:, 13:61] om for every (env, human) and mlp1.0 output feature, in sarl_reg_kernel<4, NT, true>'s accumulator order:
// term[((row * 10 + mt) * 4 + lg) * 4 + kk] = feature 16 mt + 4 kk + lg of row = env * H + human (0 beyond the 150 features).
// Plain fma chain, bias first, map values in ascending order.  Thread = accumulator slot: its 48 weights and its bias stay in
// registers for the block's rows, a row's 48 map values are scalar loads (uniform address).  wom = sarl_om_weights_kernel's
// [48][160] (map value, slot) then the 160 biases — already in slot order, zero beyond the 150 features.
constexpr int kOmTermRows = 8, kOmTermThreads = 192;  // (80 rows per block: 36 us — 640 waves, each waiting for its scalar loads row by row; 8: many waves per SIMD)
__global__ __launch_bounds__(kOmTermThreads) void sarl_om_term_kernel(const float* __restrict__ wom, const float* __restrict__ om, float* __restrict__ term, int rows) {
    const int tid = threadIdx.x;
    if (tid >= 160) return;
    float w[48];
#pragma unroll
    for (int k = 0; k < 48; ++k) w[k] = wom[k * 160 + tid];
    const float bias = wom[48 * 160 + tid];
    const int r0 = blockIdx.x * kOmTermRows, r1 = r0 + kOmTermRows < rows ? r0 + kOmTermRows : rows;
    for (int row = r0; row < r1; ++row) {
        const float* m = om + (size_t)row * 48;
        float v = bias;
#pragma unroll
        for (int k = 0; k < 48; ++k) v = __builtin_fmaf(w[k], m[k], v);
        term[(size_t)row * 160 + tid] = v;
    }
}
__global__ void sarl_om_weights_kernel(const float* W /*[150][61]*/, const float* b, float* wom) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= 49 * 160) return;
    const int k = idx / 160, slot = idx % 160;
    const int mt = slot >> 4, lg = (slot >> 2) & 3, kk = slot & 3, f = 16 * mt + 4 * kk + lg;  // slot (mt, lg, kk) <- feature
    wom[idx] = f < 150 ? (k < 48 ? W[f * 61 + 13 + k] : b[f]) : 0.0f;
}

}  // namespace cn
