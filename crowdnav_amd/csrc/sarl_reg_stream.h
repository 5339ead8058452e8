// The register-resident value-network kernels' weight streams and dense layers (sarl_reg_kernel.h has the picture): the
// stream keys and shapes, the packing plan, the quad queue and the layer templates.  Templates, constexpr and inline
// functions only: the units of the register-resident and the split-f16 kernels and the host's route choice include it.
#pragma once
#include "sarl_net.h"

namespace cn {

constexpr int kRegDepth = 4;   // weight quads in flight per wave (RegStreamT<6> in the 5-human SARL kernels: round 3, below)
constexpr int kRegPad = 12;    // a stream is a whole number of 4- AND 6-quad groups: one packing serves both depths
constexpr int kRegHumans = 5;  // N tiles per wave, at most
constexpr int kRegWaves = 4;   // waves per workgroup = SIMDs per CU

enum {
    kR_mlp1_0, kR_mlp1_2, kR_mlp2_0, kR_mlp2_2, kR_att0_global, kR_att0_local, kR_att_2, kR_att_4,
    kR_mlp3_0, kR_mlp3_2, kR_mlp3_4, kR_mlp3_6, kRegLayers
};

struct RegShape {
    int ks;      // k-steps (inputs / 4, rounded up)
    int mt;      // output tiles of 16 features
    int bias;    // 1: a bias quad opens every output tile (0: the accumulator starts from another layer's result)
    int paired;  // 1: one N tile only — two output tiles advance together so that consecutive MFMAs are independent
};

__host__ __device__ constexpr int reg_cdiv(int a, int b) { return (a + b - 1) / b; }

// The functions below describe a weight stream by a NETWORK KEY: for sarl.ValueNetwork the k-steps of its input, 4 (13
// features) or 16 (13 + 48 occupancy-map features); kRegCadrl for cadrl.ValueNetwork (cadrl.py:22-29: 13 -> 150 -> 100 ->
// 100 -> 1 on every (robot, human) row; layers 0..3).
// kRegSarlPre: sarl.ValueNetwork on 61 inputs with the occupancy-map half of mlp1.0 hoisted out of the action loop — the 48 map
// features of (env, human) are the same for all 81 actions, so  b + W[:, 13:61] om  is computed once per (env, human)
// (sarl_om_term_kernel) and mlp1.0's accumulators START from it: 4 k-steps instead of 16, no bias quad.
constexpr int kRegSarlPre = 5;
constexpr int kRegCadrl = 1004;
// lstm_rl.ValueNetwork1 (lstm_rl.py:9-33) is two streams: the LSTM cell's gate layer (one layer, re-read for every human:
// kRegLstmGates + k-steps of the input) and the value head on [self (6) | h_n (50)] (4 layers).
constexpr int kRegLstmGates = 2000, kRegLstmHead = 2100, kRegLstmHid = 50, kRegLstmKs = 13;  // 13 k-steps / output tiles of 50 units
__host__ __device__ constexpr bool reg_is_gates(int key) { return key > kRegLstmGates && key < kRegLstmHead; }
// lstm_rl.ValueNetwork2 (lstm_rl.py:36-66, with_interaction_module = true at the shipped widths mlp1_dims = 150, 100, 100, 50):
// every human's row passes mlp1 in front of the LSTM — a third stream (kRegLstmMlp1 + k-steps of the input: 4 layers, the last
// without ReLU, re-read for every human like the gate layer), and the gate layer's input is mlp1's 50 outputs (13 k-steps).
constexpr int kRegLstmMlp1 = 2200;
__host__ __device__ constexpr bool reg_is_lstm_mlp1(int key) { return key > kRegLstmMlp1 && key < kRegLstmMlp1 + 100; }
// sarl.ValueNetwork for MORE than 5 humans (sarl_reg_chunk_kernel): the humans pass in chunks of NT, so the network is three
// streams — A: mlp1.0, mlp1.2 (re-read per chunk, first pass; APre: mlp1.0 starts from the hoisted occupancy-map term),
// G: attention.0's global half, then — after the second pass — the value head (read once per tile, in this order),
// B: mlp2.0, mlp2.2, attention.0 local, attention.2, attention.4 (re-read per chunk, second pass).
constexpr int kRegChunkA = 3001, kRegChunkAPre = 3002, kRegChunkB = 3003, kRegChunkG = 3004;
__host__ __device__ constexpr int reg_layers(int key) {
    return key == kRegCadrl || key == kRegLstmHead || reg_is_lstm_mlp1(key) ? 4
           : reg_is_gates(key)                       ? 1
           : key == kRegChunkA || key == kRegChunkAPre ? 2
           : key == kRegChunkB || key == kRegChunkG    ? 5
                                                       : (int)kRegLayers;
}

__host__ __device__ constexpr RegShape reg_shape(int l, int xks) {
    if (reg_is_gates(xks)) return {xks - kRegLstmGates + kRegLstmKs, kRegLstmKs, 1, 0};  // [x_t | h_(t-1)] -> i, f, g, o of 4 units per tile
    if (reg_is_lstm_mlp1(xks)) {
        switch (l) {
            case 0: return {xks - kRegLstmMlp1, 10, 1, 0};
            case 1: return {38, 7, 1, 0};
            case 2: return {25, 7, 1, 0};
            default: return {25, 4, 1, 0};  // 50 outputs: k-steps 0..12 of the gate layer (units 50..63 of the last tile are zero)
        }
    }
    if (xks == kRegChunkA || xks == kRegChunkAPre)
        return l == 0 ? (xks == kRegChunkAPre ? RegShape{4, 10, 0, 0} : RegShape{4, 10, 1, 0}) : RegShape{38, 7, 1, 0};
    if (xks == kRegChunkB) {
        switch (l) {
            case 0: return {25, 7, 1, 0};   // mlp2.0
            case 1: return {25, 4, 1, 0};   // mlp2.2
            case 2: return {25, 7, 0, 0};   // attention.0, local half: starts from the global term
            case 3: return {25, 7, 1, 0};   // attention.2
            default: return {25, 1, 1, 0};  // attention.4
        }
    }
    if (xks == kRegChunkG) {
        switch (l) {
            case 0: return {25, 7, 1, 1};   // attention.0, global half (+ the layer's bias)
            case 1: return {15, 10, 1, 1};  // mlp3.0 on [weighted feature | self], as kR_mlp3_0
            case 2: return {38, 7, 1, 1};
            case 3: return {25, 7, 1, 1};
            default: return {25, 1, 1, 1};
        }
    }
    if (xks == kRegCadrl || xks == kRegLstmHead) {
        switch (l) {
            case 0: return {xks == kRegCadrl ? 4 : 15, 10, 1, 0};
            case 1: return {38, 7, 1, 0};
            case 2: return {25, 7, 1, 0};
            default: return {25, 1, 1, 0};
        }
    }
    switch (l) {
        case kR_mlp1_0: return xks == kRegSarlPre ? RegShape{4, 10, 0, 0} : RegShape{xks, 10, 1, 0};
        case kR_mlp1_2: return {38, 7, 1, 0};
        case kR_mlp2_0: return {25, 7, 1, 0};
        case kR_mlp2_2: return {25, 4, 1, 0};
        case kR_att0_global: return {25, 7, 1, 1};
        case kR_att0_local: return {25, 7, 0, 0};
        case kR_att_2: return {25, 7, 1, 0};
        case kR_att_4: return {25, 1, 1, 0};
        case kR_mlp3_0: return {15, 10, 1, 1};  // 12.5 k-steps of weighted feature + the self state from the X registers
        case kR_mlp3_2: return {38, 7, 1, 1};
        case kR_mlp3_4: return {25, 7, 1, 1};
        default: return {25, 1, 1, 1};          // kR_mlp3_6
    }
}
__host__ __device__ constexpr int reg_tile_quads(int l, int xks) { return reg_shape(l, xks).bias + reg_cdiv(reg_shape(l, xks).ks, 4); }
__host__ __device__ constexpr int reg_layer_quads(int l, int xks) { return reg_shape(l, xks).mt * reg_tile_quads(l, xks); }
__host__ __device__ constexpr int reg_qbase(int l, int xks) {
    int q = 0;
    for (int i = 0; i < l; ++i) q += reg_layer_quads(i, xks);
    return q;
}
// the stream is padded to a multiple of the queue depth (of every depth in use: kRegPad) so that quad I always lives in
// register slot I % depth
__host__ __device__ constexpr int reg_total_quads(int xks) {
    return reg_cdiv(reg_qbase(reg_layers(xks), xks), kRegPad) * kRegPad;
}
// position of item j (0 = bias if the layer has one, then the weight quads) of output tile mt inside its layer
__host__ __device__ constexpr int reg_qpos(int l, int xks, int mt, int j) {
    const RegShape s = reg_shape(l, xks);
    const int S = reg_tile_quads(l, xks);
    if (!s.paired || mt >= (s.mt / 2) * 2) return mt * S + j;
    return (mt / 2) * 2 * S + 2 * j + (mt & 1);
}
// input column of W that k-step ks, lane group lg multiplies (-1: none).  mlp3.0 reads joint = [self (6) | weighted feature]
// (sarl.py:61): k-steps 0..11 and lanes 0..31 of k-step 12 are the weighted feature's registers; lanes 32..63 of k-step 12
// take self features 2, 3 from X k-step 0, k-step 13 takes 4, 5 from X k-step 1 and k-step 14 takes 0, 1 from X k-step 0 —
// the registers that already hold them in those lanes.
// The LSTM-RL head reads joint = [self (6) | h_n (50)] (lstm_rl.py:30-31): k-steps 0..12 are the hidden state's registers
// (unit 4 ks + lg), k-step 13 is X k-step 0 of the first human's row (self features 0..3), k-step 14 its k-step 1 (4, 5).
__host__ __device__ constexpr int reg_kcol(int key, int l, int K, int k_off, int ks, int lg) {
    if (key == kRegLstmHead && l == 0)
        return ks < kRegLstmKs ? (4 * ks + lg < kRegLstmHid ? 6 + 4 * ks + lg : -1) : ks == 13 ? lg : lg < 2 ? 4 + lg : -1;
    if ((key >= 1000 && !(key == kRegChunkG && l == 1)) || (key < 1000 && l != kR_mlp3_0))
        return 4 * ks + lg < K ? k_off + 4 * ks + lg : -1;
    if (ks < 12) return 6 + 4 * ks + lg;
    if (ks == 12) return lg < 2 ? 6 + 48 + lg : lg;
    if (ks == 13) return lg < 2 ? 4 + lg : -1;
    return lg < 2 ? lg : -1;
}

struct RegPackLayer {
    const float* W;     // torch.nn.Linear weight [N][ldw]
    const float* b;     // bias or nullptr
    int N, ldw, K, k_off, replicate;  // replicate: the single output feature fills all 16 slots (attention score: every lane gets it)
    // LSTM gate layer (W = weight_ih [4 hid][K], b = bias_ih): the recurrent half; k-steps from k_split on multiply h
    const float* W2;    // weight_hh [4 hid][hid]
    const float* b2;    // bias_hh
    int k_split;
};
struct RegPackPlan {
    RegPackLayer L[kRegLayers];
    int xks;  // the network key
};

typedef const f32x4 __attribute__((address_space(1))) * gf32x4_p;

// Quad J is read as  buffer_load_dwordx4 v, voff, s[rsrc], soffset = J KiB offen : a buffer resource (4 SGPRs) over the
// stream, the lane offset in ONE VGPR that never changes, the quad's offset a scalar constant.  No per-quad address in
// vector registers: with global_load the 546 addresses were either hoisted out of the tile loop (474 of them spilled to
// scratch in the first build) or rebuilt as 64-bit vector adds whose destination the register allocator, out of VGPRs, put
// on top of loads still in flight (s_waitcnt vmcnt(0): the whole prefetch queue drained, several times per tile).
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
// DEPTH quads in flight.  4 everywhere but in the 5-human SARL kernels, which have the registers for 6 (round 3: the one-N-tile
// layers — attention.0's global half, the value head — consume a quad every 128 cycles, and 4 in flight cover 512 cycles of L2
// latency: cn_sarl_select 1.868 -> 1.838 ms, with occupancy maps 1.922 -> 1.907, 8 no better than 6).
template <int DEPTH>
struct RegStreamT {
    static constexpr int kDepth = DEPTH;
    __amdgpu_buffer_rsrc_t rsrc;
    uint32_t voff;     // lane * 16
    f32x4 q[DEPTH];    // quads I .. I + DEPTH - 1 of the running position (quad J in slot J % DEPTH)
};
typedef RegStreamT<kRegDepth> RegStream;
template <class WS>
__device__ __forceinline__ f32x4 reg_quad(const WS& s, int J) {
    // 4 quads share one scalar offset (the other 2 address bits go into the instruction's 12-bit immediate)
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(s.rsrc, s.voff + (J & 3) * 1024, (J >> 2) * 4096, 0));
}
template <int QT, class WS>
__device__ __forceinline__ f32x4 reg_take(WS& s, int I) {
    static_assert(QT % WS::kDepth == 0, "slot I % depth must survive the wrap of the stream");
    const f32x4 v = s.q[I % WS::kDepth];
    s.q[I % WS::kDepth] = reg_quad(s, (I + WS::kDepth) % QT);
    return v;
}

__device__ __forceinline__ f32x4 reg_relu(f32x4 v) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {  // max(x, 0) on the bit pattern: negative floats are negative integers (-0.0 too) — ONE
        const float f = v[i];                      // v_max_i32; fmaxf would quiet signalling NaNs first (a second v_max_f32)
        const int b = __float_as_int(f);           // (bit_cast straight on the vector element reads element 0 for every i)
        v[i] = __int_as_float(b > 0 ? b : 0);
    }
    return v;
}

// emit(nt, mt, act(W x + b)) for NT N tiles and every output tile mt; in(nt, ks) = the B operand of k-step ks; init(mt) =
// accumulator start when the layer has no bias quad
template <int XKS, int L, int NT, bool RELU, class WS, class In, class Init, class Emit>
__device__ __forceinline__ void reg_dense(WS& ws, In in, Init init, Emit emit) {
    constexpr RegShape S = reg_shape(L, XKS);
    constexpr int QT = reg_total_quads(XKS), QB = reg_qbase(L, XKS), KQ = reg_cdiv(S.ks, 4);
    static_assert(!S.paired, "use reg_dense1");
    // Output tile mt - 1 leaves the accumulators (AGPR -> VGPR, ReLU, or the LDS store) after the first MFMAs of tile mt have
    // issued, so that it never waits for the matrix pipe to drain (two accumulator sets).
    f32x4 acc[2][NT];
#pragma unroll
    for (int mt = 0; mt < S.mt; ++mt) {
        f32x4 c0;
        if constexpr (S.bias != 0) c0 = reg_take<QT>(ws, QB + reg_qpos(L, XKS, mt, 0));
        else c0 = init(mt);
#pragma unroll
        for (int q = 0; q < KQ; ++q) {
            const f32x4 a = reg_take<QT>(ws, QB + reg_qpos(L, XKS, mt, S.bias + q));
            __builtin_amdgcn_sched_barrier(0);  // the request for quad I + kRegDepth is issued HERE, not sunk to its use
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const int ks = 4 * q + kk;
                if (ks < S.ks) {
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt)
                        acc[mt & 1][nt] =
                            __builtin_amdgcn_mfma_f32_16x16x4f32(a[kk], in(nt, ks), ks == 0 ? c0 : acc[mt & 1][nt], 0, 0, 0);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            if (q == 0 && mt > 0) {
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) emit(nt, mt - 1, RELU ? reg_relu(acc[(mt - 1) & 1][nt]) : acc[(mt - 1) & 1][nt]);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
        emit(nt, S.mt - 1, RELU ? reg_relu(acc[(S.mt - 1) & 1][nt]) : acc[(S.mt - 1) & 1][nt]);
    __builtin_amdgcn_sched_barrier(0);
}

// A layer with ONE output (a value head, an attention score) on the vector ALUs: as a 16-wide MFMA tile it executes 16 x the
// multiply-adds it needs — 25 k-steps x NT matrix instructions of 32 cycles each for 100 inputs — and the FP32 MFMA runs at the
// vector rate, so nothing is gained by keeping it on the matrix side.  The stream's quads are the same (`replicate` packing: lane
// l's A fragment of k-step ks IS the weight of the input its own B fragment holds — feature 4 ks + (l >> 4) of row l & 15): every
// lane multiplies its 25 inputs by its 25 weights (v_fma_f32), the four lane groups of a row are summed through two cross-lane
// exchanges, the bias goes on last.  Every lane of a row ends with the row's value, as with the replicated tile.  Not the MFMA's
// summation order: ~1e-7 of it (tests: 1e-6 of the reference).
template <int XKS, int L, int NT, class WS, class In, class Emit>
__device__ __forceinline__ void reg_dense_valu1(WS& ws, In in, Emit emit) {
    constexpr RegShape S = reg_shape(L, XKS);
    constexpr int QT = reg_total_quads(XKS), QB = reg_qbase(L, XKS), KQ = reg_cdiv(S.ks, 4);
    static_assert(S.mt == 1 && S.bias && !S.paired, "one replicated output tile with a bias quad");
    const f32x4 c0 = reg_take<QT>(ws, QB + reg_qpos(L, XKS, 0, 0));
    float acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt] = 0.0f;
#pragma unroll
    for (int q = 0; q < KQ; ++q) {
        const f32x4 a = reg_take<QT>(ws, QB + reg_qpos(L, XKS, 0, 1 + q));
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const int ks = 4 * q + kk;
            if (ks < S.ks) {
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc[nt] = __builtin_fmaf(a[kk], in(nt, ks), acc[nt]);
            }
        }
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        float v = acc[nt];
        v += __shfl_xor(v, 16);
        v += __shfl_xor(v, 32);
        v += c0[0];
        emit(nt, 0, f32x4{v, v, v, v});
    }
}

// ReLU of one value; AG: the result goes to an AGPR (the asm's "=a" operand is what keeps the array in the accumulator half
// of the register file, where the next layer's MFMAs read it as their B operand directly — arrays the compiler moves there
// on its own are copied back with v_accvgpr_read before every use).
template <bool AG>
__device__ __forceinline__ float reg_relu1(float x) {
    const int b = __float_as_int(x);
    x = __int_as_float(b > 0 ? b : 0);  // v_max_i32: negative floats are negative integers
    if constexpr (AG) {
        float r;
        asm("v_accvgpr_write_b32 %0, %1" : "=a"(r) : "v"(x));
        return r;
    }
    return x;
}

// out[nt][mt] = relu(W x + b).  Every instruction a wave issues between two MFMAs delays the second one by ~5 cycles (one wave
// per SIMD: nothing else hides it; measured: tile time = 32 cycles x MFMAs + 5.4 x everything else — and WHERE it sits does
// not matter: round 3 spread the ReLU burst of tile mt - 1 one value per MFMA gap over tile mt's first 20 MFMAs with
// sched_group_barrier(MFMA 1, VALU 3) — gap histogram 62-instruction bursts -> 3..7 per gap — and cn_sarl_select went
// 1.834 -> 1.839 ms; -mllvm -amdgpu-mfma-vgpr-form removes the 802 v_accvgpr_read per tile and gains 0.8 %), so the layer is written
// for instruction count: a VGPR array (AG = false) is accumulated in place and rectified with one v_max_i32 per value; an
// AGPR array is accumulated in VGPRs, rectified there and moved with one v_accvgpr_write (2 per value; read - max - write on
// an AGPR accumulator would be 3).  The ReLU of tile mt - 1 follows the first MFMAs of tile mt, so that it never waits for
// the matrix pipe to drain.
template <int XKS, int L, int NT, bool AG, class WS, class In, class Init, int MT = reg_shape(L, XKS).mt>
__device__ __forceinline__ void reg_dense_arr(WS& ws, In in, Init init, f32x4 (&out)[NT][MT]) {
    constexpr RegShape S = reg_shape(L, XKS);
    constexpr int QT = reg_total_quads(XKS), QB = reg_qbase(L, XKS), KQ = reg_cdiv(S.ks, 4);
    static_assert(!S.paired && MT == S.mt && S.ks >= 4, "use reg_dense1");
    constexpr bool kPerTileInit = std::is_invocable_v<Init, int, int>;  // init(nt, mt): a start value per N tile
    f32x4 acc[2][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        f32x4 c0[kPerTileInit ? NT : 1];
        if constexpr (S.bias != 0) c0[0] = reg_take<QT>(ws, QB + reg_qpos(L, XKS, mt, 0));
        else if constexpr (kPerTileInit) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) c0[nt] = init(nt, mt);
        } else c0[0] = init(mt);
#pragma unroll
        for (int q = 0; q < KQ; ++q) {
            const f32x4 a = reg_take<QT>(ws, QB + reg_qpos(L, XKS, mt, S.bias + q));
            __builtin_amdgcn_sched_barrier(0);  // the request for quad I + kRegDepth is issued HERE, not sunk to its use
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const int ks = 4 * q + kk;
                if (ks < S.ks) {
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt)
                        acc[mt & 1][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                            a[kk], in(nt, ks), ks == 0 ? c0[kPerTileInit ? nt : 0] : acc[mt & 1][nt], 0, 0, 0);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            if (q == 0 && mt > 0) {
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                    for (int i = 0; i < 4; ++i) out[nt][mt - 1][i] = reg_relu1<AG>(acc[(mt - 1) & 1][nt][i]);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int i = 0; i < 4; ++i) out[nt][MT - 1][i] = reg_relu1<AG>(acc[(MT - 1) & 1][nt][i]);
    __builtin_amdgcn_sched_barrier(0);
}

// one N tile: output tiles two at a time (their MFMAs alternate: a dependent v_mfma_f32_16x16x4_f32 issues after 40 cycles,
// an independent one after 32)
template <int XKS, int L, bool RELU, class WS, class In, int MT = reg_shape(L, XKS).mt>
__device__ __forceinline__ void reg_dense1(WS& ws, In in, f32x4 (&out)[MT]) {
    constexpr RegShape S = reg_shape(L, XKS);
    constexpr int QT = reg_total_quads(XKS), QB = reg_qbase(L, XKS), KQ = reg_cdiv(S.ks, 4);
    static_assert(S.paired && S.bias && MT == S.mt, "use reg_dense");
#pragma unroll
    for (int p = 0; p < MT / 2; ++p) {
        const f32x4 c0 = reg_take<QT>(ws, QB + reg_qpos(L, XKS, 2 * p, 0));
        const f32x4 c1 = reg_take<QT>(ws, QB + reg_qpos(L, XKS, 2 * p + 1, 0));
        f32x4 acc0, acc1;
#pragma unroll
        for (int q = 0; q < KQ; ++q) {
            const f32x4 a0 = reg_take<QT>(ws, QB + reg_qpos(L, XKS, 2 * p, 1 + q));
            const f32x4 a1 = reg_take<QT>(ws, QB + reg_qpos(L, XKS, 2 * p + 1, 1 + q));
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const int ks = 4 * q + kk;
                if (ks < S.ks) {
                    const float x = in(ks);
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[kk], x, ks == 0 ? c0 : acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[kk], x, ks == 0 ? c1 : acc1, 0, 0, 0);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        out[2 * p] = RELU ? reg_relu(acc0) : acc0, out[2 * p + 1] = RELU ? reg_relu(acc1) : acc1;
        __builtin_amdgcn_sched_barrier(0);
    }
    if (MT & 1) {
        constexpr int mt = MT - 1;
        const f32x4 c0 = reg_take<QT>(ws, QB + reg_qpos(L, XKS, mt, 0));
        f32x4 acc;
#pragma unroll
        for (int q = 0; q < KQ; ++q) {
            const f32x4 a = reg_take<QT>(ws, QB + reg_qpos(L, XKS, mt, 1 + q));
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const int ks = 4 * q + kk;
                if (ks < S.ks) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[kk], in(ks), ks == 0 ? c0 : acc, 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        out[mt] = RELU ? reg_relu(acc) : acc;
        __builtin_amdgcn_sched_barrier(0);
    }
}

}  // namespace cn
