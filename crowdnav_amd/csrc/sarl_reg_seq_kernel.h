// The register-resident kernels of the networks that take the humans of a group one after another (sarl_reg_kernel.h has the
// picture, sarl_reg_stream.h the streams and layers): cadrl.ValueNetwork and the two lstm_rl networks.  Templates only.
#pragma once
#include "sarl_reg_stream.h"

namespace cn {

// cadrl.ValueNetwork (cadrl.py:22-29) with the activations in registers: the same MLP for every (group, human) row — NT N tiles
// of 16 rows per wave, layers chained through the accumulator layout as above — then the minimum over the humans present
// (cadrl.py:162-163: torch.min over dim 0, the first minimum's value).  X, hcount, V as for sarl_reg_kernel.
template <int NT>
__global__ __launch_bounds__(kRegWaves * 64) void cadrl_reg_kernel(const float* stream, const float* X, float* V, int n_groups,
                                                                   int n_tiles, int ks_x, const int* hcount, int H, int n_chunks) {
    static_assert(NT >= 1 && NT <= kRegHumans, "the activations of at most 5 humans fit the register file");
    constexpr int NK = kRegCadrl, QT = reg_total_quads(NK);
    const int lane = threadIdx.x & 63;
    const int wid = blockIdx.x * kRegWaves + (threadIdx.x >> 6), nw = gridDim.x * kRegWaves;
    RegStream ws;
    ws.rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(stream), 0, QT * 1024, 0x00020000);
    ws.voff = (uint32_t)lane * 16u;
#pragma unroll
    for (int i = 0; i < kRegDepth; ++i) ws.q[i] = reg_quad(ws, i);
    if (wid >= n_tiles) return;
    const gfloat_p Xg = as_global(X) + lane;
    float x[NT][4];
    // chunk c of a tile = humans c NT .. c NT + NT - 1 (more than 5 humans: n_chunks > 1; indices beyond the crowd repeat its last
    // human and never win the minimum)
    const auto load_x = [&](int t, int c) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int h = c * NT + nt < H ? c * NT + nt : H - 1;
            const gfloat_p xt = Xg + ((size_t)t * H + h) * ks_x * 64;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) x[nt][ks] = xt[ks * 64];
        }
    };
    load_x(wid, 0);
    const auto none = [](int) { return f32x4{0.0f, 0.0f, 0.0f, 0.0f}; };
    for (int tile = wid; tile < n_tiles; tile += nw) {
        const int cnt = hcount[(size_t)tile * kSarlGroups + (lane & 15)];
        float m = 0.0f;
#pragma unroll 1
        for (int c = 0; c < n_chunks; ++c) {
            f32x4 h3[NT][7];
            {
                f32x4 h2[NT][7];
                {
                    f32x4 h1[NT][10];
                    reg_dense_arr<NK, 0, NT, true>(ws, [&](int nt, int ks) { return x[nt][ks]; }, none, h1);
                    // x is dead: the next chunk's (or the next tile's first chunk's) rows travel while this one computes
                    if (c + 1 < n_chunks) load_x(tile, c + 1);
                    else load_x(tile + nw < n_tiles ? tile + nw : tile, 0);
                    reg_dense_arr<NK, 1, NT, false>(ws, [&](int nt, int ks) { return h1[nt][ks >> 2][ks & 3]; }, none, h2);
                }
                reg_dense_arr<NK, 2, NT, true>(ws, [&](int nt, int ks) { return h2[nt][ks >> 2][ks & 3]; }, none, h3);
            }
            float sc[NT];
            reg_dense_valu1<NK, 3, NT>(ws, [&](int nt, int ks) { return h3[nt][ks >> 2][ks & 3]; },
                                       [&](int nt, int, f32x4 v) { sc[nt] = v[0]; });
#pragma unroll
            for (int i = reg_qbase(reg_layers(NK), NK); i < QT; ++i) (void)reg_take<QT>(ws, i);
            if (c == 0) m = sc[0];  // torch.min over dim 0: the first minimum's value
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) m = (c * NT + nt < cnt && sc[nt] < m) ? sc[nt] : m;
        }
        if (lane < kSarlGroups) {
            const size_t G = (size_t)tile * kSarlGroups + lane;
            if (G < (size_t)n_groups) V[G] = m;
        }
    }
}

// ---- lstm_rl.ValueNetwork1 (lstm_rl.py:9-33) with the state in registers ------------------------------------------------
// The recurrence is sequential over the humans of a group, so a wave carries NT TILES (16 groups each) through it side by
// side: per human one gate layer [x_t | h] -> 4 x 50 pre-activations as 13 output tiles x (XKS + 13) k-steps x NT independent
// MFMAs; the cell update of tile mt (sigmoid / tanh on its f32x4, c and h are one register per k-step) runs behind the first
// MFMAs of tile mt + 1.  Any number of humans: nothing is sized by H.  sigmoid(x) = 1 / (1 + 2^(-x log2 e)) and tanh(x) =
// 1 - 2 / (1 + 2^(2 x log2 e)) on v_exp_f32 / v_rcp_f32 (1 ulp each): absolute error ~1e-7 per activation, against expf /
// tanhf's ~20 instructions each on a wave that has nothing to hide them behind.
__device__ __forceinline__ float reg_sigmoid(float x) {
    return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.442695040888963f * x));
}
__device__ __forceinline__ float reg_tanh(float x) {
    return 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(2.885390081777927f * x));
}

// (m all ones: a, zero: b) as ONE v_bfi_b32 on values that are computed either way.  `present ? new : old` let hipcc sink the
// whole cell update under a divergent branch — s_and_saveexec / s_cbranch_execz / s_or_b64 around each of the 65 (tile, output
// tile) updates of a step, every one a scheduling barrier between the MFMAs of neighbouring output tiles.
__device__ __forceinline__ float reg_select(uint32_t m, float a, float b) {
    return __uint_as_float((__float_as_uint(a) & m) | (__float_as_uint(b) & ~m));
}

template <int XKS, int NT>
__device__ __forceinline__ void lstm_reg_bundle(RegStream& wg, RegStream& wh, const float* X, float* V, int n_groups, int H, int ks_x,
                                                const int* hcount, int base, int lane) {
    constexpr int GK = kRegLstmGates + XKS, HK = kRegLstmHead, KS = kRegLstmKs;
    constexpr int QG = reg_total_quads(GK), QH = reg_total_quads(HK);
    const gfloat_p Xg = as_global(X) + lane;
    float h[NT][KS], c[NT][KS], x[NT][XKS], self0[NT], self1[NT];
    int cnt[NT];
    const auto load_x = [&](int t, float (&dst)[NT][XKS]) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const gfloat_p xt = Xg + ((size_t)(base + nt) * H + t) * ks_x * 64;
#pragma unroll
            for (int ks = 0; ks < XKS; ++ks) dst[nt][ks] = xt[ks * 64];
        }
    };
    load_x(0, x);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        cnt[nt] = hcount[(size_t)(base + nt) * kSarlGroups + (lane & 15)];
        self0[nt] = x[nt][0], self1[nt] = x[nt][1];  // self_state = state[:, 0, :6]: the first row's k-steps 0, 1
#pragma unroll
        for (int j = 0; j < KS; ++j) h[nt][j] = 0.0f, c[nt][j] = 0.0f;
    }
    const auto none = [](int) { return f32x4{0.0f, 0.0f, 0.0f, 0.0f}; };
#pragma unroll 1
    for (int t = 0; t < H; ++t) {
        float xn[NT][XKS], hn[NT][KS];
        load_x(t + 1 < H ? t + 1 : t, xn);  // the next human's rows travel while this one computes
        uint32_t present[NT];  // `mixed` rule: a group whose episode has fewer humans keeps its state from here on
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) present[nt] = t < cnt[nt] ? 0xffffffffu : 0u;
        reg_dense<GK, 0, NT, false>(
            wg, [&](int nt, int ks) { return ks < XKS ? x[nt][ks] : h[nt][ks - XKS]; }, none,
            [&](int nt, int mt, f32x4 v) {
                const float cn_ = reg_sigmoid(v[1]) * c[nt][mt] + reg_sigmoid(v[0]) * reg_tanh(v[2]);
                const float hn_ = reg_sigmoid(v[3]) * reg_tanh(cn_);
                c[nt][mt] = reg_select(present[nt], cn_, c[nt][mt]);
                hn[nt][mt] = reg_select(present[nt], hn_, h[nt][mt]);
            });
#pragma unroll
        for (int i = reg_qbase(1, GK); i < QG; ++i) (void)reg_take<QG>(wg, i);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
            for (int j = 0; j < KS; ++j) h[nt][j] = hn[nt][j];
#pragma unroll
            for (int ks = 0; ks < XKS; ++ks) x[nt][ks] = xn[nt][ks];
        }
    }
    float val[NT];
    {
        f32x4 j3[NT][7];
        {
            f32x4 j2[NT][7];
            {
                f32x4 j1[NT][10];
                reg_dense_arr<HK, 0, NT, true>(
                    wh, [&](int nt, int ks) { return ks < KS ? h[nt][ks] : ks == KS ? self0[nt] : self1[nt]; }, none, j1);
                reg_dense_arr<HK, 1, NT, false>(wh, [&](int nt, int ks) { return j1[nt][ks >> 2][ks & 3]; }, none, j2);
            }
            reg_dense_arr<HK, 2, NT, true>(wh, [&](int nt, int ks) { return j2[nt][ks >> 2][ks & 3]; }, none, j3);
        }
        reg_dense<HK, 3, NT, false>(wh, [&](int nt, int ks) { return j3[nt][ks >> 2][ks & 3]; }, none,
                                    [&](int nt, int, f32x4 v) { val[nt] = v[0]; });
    }
#pragma unroll
    for (int i = reg_qbase(4, HK); i < QH; ++i) (void)reg_take<QH>(wh, i);
    if (lane < kSarlGroups) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const size_t G = (size_t)(base + nt) * kSarlGroups + lane;
            if (G < (size_t)n_groups) V[G] = val[nt];
        }
    }
}

// Persistent: full rounds of 5-tile bundles over all waves, then the remainder — as one more round of bundles when that is
// shorter than its single tiles one per wave (a single tile's MFMAs are one dependent chain: ~0.4 of a bundle's time).
template <int XKS>
__global__ __launch_bounds__(kRegWaves * 64) void lstm_reg_kernel(const float* gates, const float* head, const float* X, float* V,
                                                                  int n_groups, int n_tiles, int H, int ks_x, const int* hcount) {
    constexpr int GK = kRegLstmGates + XKS, NT = kRegHumans;
    const int lane = threadIdx.x & 63;
    const int wid = blockIdx.x * kRegWaves + (threadIdx.x >> 6), nw = gridDim.x * kRegWaves;
    RegStream wg, wh;
    wg.rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(gates), 0, reg_total_quads(GK) * 1024, 0x00020000);
    wh.rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(head), 0, reg_total_quads(kRegLstmHead) * 1024, 0x00020000);
    wg.voff = wh.voff = (uint32_t)lane * 16u;
#pragma unroll
    for (int i = 0; i < kRegDepth; ++i) wg.q[i] = reg_quad(wg, i), wh.q[i] = reg_quad(wh, i);
    const int rounds = n_tiles / (NT * nw);
    int done = 0;
    for (int k = 0; k < rounds; ++k)
        lstm_reg_bundle<XKS, NT>(wg, wh, X, V, n_groups, H, ks_x, hcount, (k * nw + wid) * NT, lane);
    done = rounds * NT * nw;
    if (n_tiles - done > 2 * nw) {
        const int nb = (n_tiles - done) / NT;
        if (wid < nb) lstm_reg_bundle<XKS, NT>(wg, wh, X, V, n_groups, H, ks_x, hcount, done + wid * NT, lane);
        done += nb * NT;
    }
    for (int tile = done + wid; tile < n_tiles; tile += nw)
        lstm_reg_bundle<XKS, 1>(wg, wh, X, V, n_groups, H, ks_x, hcount, tile, lane);
}

// ---- lstm_rl.ValueNetwork2 (lstm_rl.py:36-66): mlp1 on every human's row in front of the cell ----------------------------
// lstm_reg_bundle with one more stage per human: x_t -> mlp1 (150 - 100 - 100 - 50, ReLU between) as the value head's layers
// are run — accumulators of a layer are the next layer's B operands, AGPR / VGPR arrays alternating — and the gate layer reads
// [mlp1(x_t) | h] (13 + 13 k-steps).  NT tiles per wave: 3 (mlp1's 150-wide layer keeps 40 registers per tile alive beside the
// 100-wide one's 28 and the cell's 26).
template <int XKS, int NT>
__device__ __forceinline__ void lstm2_reg_bundle(RegStream& wm, RegStream& wg, RegStream& wh, const float* X, float* V, int n_groups,
                                                 int H, int ks_x, const int* hcount, int base, int lane) {
    constexpr int MK = kRegLstmMlp1 + XKS, GK = kRegLstmGates + kRegLstmKs, HK = kRegLstmHead, KS = kRegLstmKs;
    constexpr int QM = reg_total_quads(MK), QG = reg_total_quads(GK), QH = reg_total_quads(HK);
    const gfloat_p Xg = as_global(X) + lane;
    float h[NT][KS], c[NT][KS], x[NT][XKS], self0[NT], self1[NT];
    int cnt[NT];
    const auto load_x = [&](int t, float (&dst)[NT][XKS]) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const gfloat_p xt = Xg + ((size_t)(base + nt) * H + t) * ks_x * 64;
#pragma unroll
            for (int ks = 0; ks < XKS; ++ks) dst[nt][ks] = xt[ks * 64];
        }
    };
    load_x(0, x);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        cnt[nt] = hcount[(size_t)(base + nt) * kSarlGroups + (lane & 15)];
        self0[nt] = x[nt][0], self1[nt] = x[nt][1];  // self_state = state[:, 0, :6]: the first row's k-steps 0, 1
#pragma unroll
        for (int j = 0; j < KS; ++j) h[nt][j] = 0.0f, c[nt][j] = 0.0f;
    }
    const auto none = [](int) { return f32x4{0.0f, 0.0f, 0.0f, 0.0f}; };
#pragma unroll 1
    for (int t = 0; t < H; ++t) {
        float xn[NT][XKS], hn[NT][KS];
        load_x(t + 1 < H ? t + 1 : t, xn);  // the next human's rows travel while this one computes
        uint32_t present[NT];  // `mixed` rule: a group whose episode has fewer humans keeps its state from here on
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) present[nt] = t < cnt[nt] ? 0xffffffffu : 0u;
        f32x4 m4[NT][4];
        {
            f32x4 m3[NT][7];
            {
                f32x4 m2[NT][7];
                {
                    f32x4 m1[NT][10];
                    reg_dense_arr<MK, 0, NT, true>(wm, [&](int nt, int ks) { return x[nt][ks]; }, none, m1);
                    reg_dense_arr<MK, 1, NT, false>(wm, [&](int nt, int ks) { return m1[nt][ks >> 2][ks & 3]; }, none, m2);
                }
                reg_dense_arr<MK, 2, NT, true>(wm, [&](int nt, int ks) { return m2[nt][ks >> 2][ks & 3]; }, none, m3);
            }
            reg_dense<MK, 3, NT, false>(wm, [&](int nt, int ks) { return m3[nt][ks >> 2][ks & 3]; }, none,
                                        [&](int nt, int mt, f32x4 v) { m4[nt][mt] = v; });  // (cadrl.mlp: no ReLU behind the last layer)
        }
#pragma unroll
        for (int i = reg_qbase(4, MK); i < QM; ++i) (void)reg_take<QM>(wm, i);
        reg_dense<GK, 0, NT, false>(
            wg, [&](int nt, int ks) { return ks < KS ? m4[nt][ks >> 2][ks & 3] : h[nt][ks - KS]; }, none,
            [&](int nt, int mt, f32x4 v) {
                const float cn_ = reg_sigmoid(v[1]) * c[nt][mt] + reg_sigmoid(v[0]) * reg_tanh(v[2]);
                const float hn_ = reg_sigmoid(v[3]) * reg_tanh(cn_);
                c[nt][mt] = reg_select(present[nt], cn_, c[nt][mt]);
                hn[nt][mt] = reg_select(present[nt], hn_, h[nt][mt]);
            });
#pragma unroll
        for (int i = reg_qbase(1, GK); i < QG; ++i) (void)reg_take<QG>(wg, i);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
            for (int j = 0; j < KS; ++j) h[nt][j] = hn[nt][j];
#pragma unroll
            for (int ks = 0; ks < XKS; ++ks) x[nt][ks] = xn[nt][ks];
        }
    }
    float val[NT];
    {
        f32x4 j3[NT][7];
        {
            f32x4 j2[NT][7];
            {
                f32x4 j1[NT][10];
                reg_dense_arr<HK, 0, NT, true>(
                    wh, [&](int nt, int ks) { return ks < KS ? h[nt][ks] : ks == KS ? self0[nt] : self1[nt]; }, none, j1);
                reg_dense_arr<HK, 1, NT, false>(wh, [&](int nt, int ks) { return j1[nt][ks >> 2][ks & 3]; }, none, j2);
            }
            reg_dense_arr<HK, 2, NT, true>(wh, [&](int nt, int ks) { return j2[nt][ks >> 2][ks & 3]; }, none, j3);
        }
        reg_dense<HK, 3, NT, false>(wh, [&](int nt, int ks) { return j3[nt][ks >> 2][ks & 3]; }, none,
                                    [&](int nt, int, f32x4 v) { val[nt] = v[0]; });
    }
#pragma unroll
    for (int i = reg_qbase(4, HK); i < QH; ++i) (void)reg_take<QH>(wh, i);
    if (lane < kSarlGroups) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const size_t G = (size_t)(base + nt) * kSarlGroups + lane;
            if (G < (size_t)n_groups) V[G] = val[nt];
        }
    }
}

constexpr int kLstm2Tiles = 3;  // (measured at 4096 x 81 x 5: 2 / 3 / 4 tiles per wave 1.797 / 1.765 / 1.768 ms; 4 spill with 61 inputs)
template <int XKS>
__global__ __launch_bounds__(kRegWaves * 64) void lstm2_reg_kernel(const float* mlp1, const float* gates, const float* head, const float* X,
                                                                   float* V, int n_groups, int n_tiles, int H, int ks_x,
                                                                   const int* hcount) {
    constexpr int NT = kLstm2Tiles;
    const int lane = threadIdx.x & 63;
    const int wid = blockIdx.x * kRegWaves + (threadIdx.x >> 6), nw = gridDim.x * kRegWaves;
    RegStream wm, wg, wh;
    wm.rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(mlp1), 0, reg_total_quads(kRegLstmMlp1 + XKS) * 1024, 0x00020000);
    wg.rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(gates), 0, reg_total_quads(kRegLstmGates + kRegLstmKs) * 1024, 0x00020000);
    wh.rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(head), 0, reg_total_quads(kRegLstmHead) * 1024, 0x00020000);
    wm.voff = wg.voff = wh.voff = (uint32_t)lane * 16u;
#pragma unroll
    for (int i = 0; i < kRegDepth; ++i) wm.q[i] = reg_quad(wm, i), wg.q[i] = reg_quad(wg, i), wh.q[i] = reg_quad(wh, i);
    const int rounds = n_tiles / (NT * nw);
    int done = 0;
    for (int k = 0; k < rounds; ++k)
        lstm2_reg_bundle<XKS, NT>(wm, wg, wh, X, V, n_groups, H, ks_x, hcount, (k * nw + wid) * NT, lane);
    done = rounds * NT * nw;
    if (n_tiles - done > 2 * nw) {
        const int nb = (n_tiles - done) / NT;
        if (wid < nb) lstm2_reg_bundle<XKS, NT>(wm, wg, wh, X, V, n_groups, H, ks_x, hcount, done + wid * NT, lane);
        done += nb * NT;
    }
    for (int tile = done + wid; tile < n_tiles; tile += nw)
        lstm2_reg_bundle<XKS, 1>(wm, wg, wh, X, V, n_groups, H, ks_x, hcount, tile, lane);
}

}  // namespace cn
