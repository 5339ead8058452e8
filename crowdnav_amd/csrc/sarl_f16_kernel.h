// sarl.ValueNetwork.forward (crowd_nav/policy/sarl.py:28-65) on the F16 matrix pipe with fp32-grade values: every operand of
// every linear layer is split into two f16 terms (CN_PRECISION_F16X2).  With S = 2^11:
//
//   ah = f16(a)   al = f16((a - f32(ah)) S)     per activation element, every layer, here in the kernel
//   Wh = f16(W)   Wl = f16((W - f32(Wh)) S)     once per cn_sarl_set_weights (sarl_f16_pack_kernel)
//   main  = sum ah Wh                            f32 accumulator of v_mfma_f32_16x16x32_f16
//   cross = sum al Wh + sum ah Wl                a second f32 accumulator
//   y = main + cross (1 / S) + b
//
// The term al Wl (2^-22 of the product) is dropped.  The scaling by S keeps the low parts (2^-11 of their values: ~2e-5 for the
// weights) out of the f16 subnormals.  Everything between the layers is f32, as in the fp32 kernels: bias, ReLU, the mean over
// the humans, the softmax with the reference's `score != 0` mask, the weighted feature sum, the joint state.
// LIMIT: an activation beyond the f16 range (|a| > 65504) gives ah = +-inf, al = -+inf, so every output it feeds is NaN
// (inf - inf, or inf 0 on a padded weight), the ReLU below keeps a NaN, and V ends as NaN: cn_sarl_select reports best = -2
// for that env.  Never a wrong finite value.
//
// Shape of the computation, as in sarl_reg_kernel: a wave computes Y^T = W X^T for its own 16 (env, action) groups x NT humans
// through the whole network, activations in registers, weights streamed from L2 in the order of use.
//   * A operand = weights: lane l holds output feature l & 15 of the tile, inputs 8 (l >> 4) .. + 7 of the 32-input block.
//     B operand = activations: lane l holds inputs 8 (l >> 4) .. + 7 of row l & 15.  The accumulator holds, in lane l, output
//     features 4 (l >> 4) .. + 3 of row l & 15.  So the registers of output tiles 2 j and 2 j + 1 ARE the B operand of input
//     block j of the next layer, once that layer's weight columns are packed in the order
//         position p = 8 lg + 4 u + i of block j  <->  feature 16 (2 j + u) + 4 lg + i        (f16_feature)
//     and each value has been split where it left the accumulator.  No LDS, no barrier, no data movement between layers.
//   * The stream is one array of 2-KiB items, one per (output tile, input block) in the order of use: lane l's 8 halves of Wh
//     (first KiB) and of Wl (second KiB).  4 or 6 items are in flight per wave, across layer and tile boundaries.  The
//     biases are a second small array, [output tile][lane][4] floats in accumulator order.
//   * attention.0 reads [h2 | mean]: 8 input blocks, the last 4 the split mean, the same operand for every human.
//   * mlp3.0 reads joint = [self (6) | weighted feature (50)]: blocks 0, 1 are the weighted feature's 4 tiles; the self state
//     takes the slots of features 50.. of the last tile (registers 2, 3), from X k-steps 0, 1 of the first human's row — the
//     registers that already hold it in those lanes.
#pragma once

#include "sarl_reg_stream.h"

namespace cn {

typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr int kF16Pad = 12;          // a stream is a whole number of 4- AND 6-item groups: one packing serves both queue depths
constexpr float kF16Scale = 2048.0f;  // S = 2^11
constexpr float kF16InvScale = 1.0f / 2048.0f;

// (mlp1 a second time for humans 3.. of a crowd of 4 or 5: see f16_dup)
enum {
    kF_mlp1_0, kF_mlp1_2, kF_mlp1_0b, kF_mlp1_2b, kF_mlp2_0, kF_mlp2_2, kF_att_0, kF_att_2, kF_att_4, kF_mlp3_0, kF_mlp3_2, kF_mlp3_4, kF_mlp3_6, kF16Layers
};

struct F16Shape {
    int kb;  // input blocks of 32
    int mt;  // output tiles of 16 features
};
// A stream is described by a KEY = xkb + 4 dup.  xkb: input blocks of mlp1.0 — 1 (13 features: X k-steps 0..3) or 2 (61 features:
// X k-steps 0..15).  dup (crowds of 4 and 5): mlp1 runs for humans 0..2, then again for the rest — 200 registers of mlp1.0's
// output for 5 humans beside mlp1.2's 140 do not fit the register file, and what the compiler spills to scratch shares the
// memory counter with the weight queue (every reload drains it) — so its two layers appear twice in the stream and the
// position stays linear.
__host__ __device__ constexpr int f16_key(int xkb, int humans) { return xkb + (humans >= 4 ? 4 : 0); }
__host__ __device__ constexpr int f16_xkb(int key) { return key & 3; }
__host__ __device__ constexpr bool f16_dup(int key) { return (key >> 2) != 0; }
__host__ __device__ constexpr int f16_canon(int l) { return l == kF_mlp1_0b ? (int)kF_mlp1_0 : l == kF_mlp1_2b ? (int)kF_mlp1_2 : l; }
// layer of the state_dict (0..10) behind stream layer l
__host__ __device__ constexpr int f16_src(int l) { return l <= kF_mlp1_2 ? l : l - 2; }
__host__ __device__ constexpr F16Shape f16_shape(int l, int key) {
    switch (l) {
        case kF_mlp1_0: return {f16_xkb(key), 10};
        case kF_mlp1_2: return {5, 7};
        case kF_mlp1_0b: return f16_dup(key) ? F16Shape{f16_xkb(key), 10} : F16Shape{0, 0};
        case kF_mlp1_2b: return f16_dup(key) ? F16Shape{5, 7} : F16Shape{0, 0};
        case kF_mlp2_0: return {4, 7};
        case kF_mlp2_2: return {4, 4};
        case kF_att_0: return {8, 7};
        case kF_att_2: return {4, 7};
        case kF_att_4: return {4, 1};
        case kF_mlp3_0: return {2, 10};
        case kF_mlp3_2: return {5, 7};
        case kF_mlp3_4: return {4, 7};
        default: return {4, 1};  // kF_mlp3_6
    }
}
__host__ __device__ constexpr int f16_layer_items(int l, int xkb) { return f16_shape(l, xkb).kb * f16_shape(l, xkb).mt; }
__host__ __device__ constexpr int f16_ibase(int l, int xkb) {
    int n = 0;
    for (int i = 0; i < l; ++i) n += f16_layer_items(i, xkb);
    return n;
}
__host__ __device__ constexpr int f16_tbase(int l, int xkb) {  // first bias tile of layer l
    int n = 0;
    for (int i = 0; i < l; ++i) n += f16_shape(i, xkb).mt;
    return n;
}
// the stream is padded to a multiple of the queue depth (of both depths in use) so that item I always lives in slot I % depth
__host__ __device__ constexpr int f16_total_items(int xkb) {
    return (f16_ibase(kF16Layers, xkb) + kF16Pad - 1) / kF16Pad * kF16Pad;
}
__host__ __device__ constexpr int f16_total_tiles(int xkb) { return f16_tbase(kF16Layers, xkb); }
__host__ __device__ constexpr size_t f16_stream_bytes(int xkb) { return (size_t)f16_total_items(xkb) * 2048; }

// feature of the previous layer's output that position p of input block kb holds
__host__ __device__ constexpr int f16_feature(int kb, int p) { return 16 * (2 * kb + ((p >> 2) & 1)) + 4 * (p >> 3) + (p & 3); }

// column of torch's W [N][ldw] that position p of input block kb of layer l multiplies (-1: none, the weight is zero)
__host__ __device__ constexpr int f16_col(int l_, int key, int kb, int p) {
    const int lg = p >> 3, r = p & 7, l = f16_canon(l_), xkb = f16_xkb(key);
    if (l == kF_mlp1_0) {  // X k-step ks of lane group lg = feature 4 ks + lg; block kb holds k-steps 8 kb .. + 7 (4..7 of a 13-wide row: none)
        if (xkb == 1 && r >= 4) return -1;
        const int f = 4 * (8 * kb + r) + lg;
        return f < (xkb == 1 ? 13 : 61) ? f : -1;
    }
    if (l == kF_mlp3_0) {  // joint = [self (6) | weighted feature (50)]
        if (kb == 1 && r == 6) return lg;                  // X k-step 0: self 0..3
        if (kb == 1 && r == 7) return lg < 2 ? 4 + lg : -1;  // X k-step 1: self 4, 5
        const int f = f16_feature(kb, p);
        return f < 50 ? 6 + f : -1;
    }
    if (l == kF_att_0) {  // [h2 (100) | mean (100)]
        const int f = f16_feature(kb & 3, p);
        return f < 100 ? (kb >> 2) * 100 + f : -1;
    }
    const int K = l == kF_mlp1_2 || l == kF_mlp3_2 ? 150 : 100;
    const int f = f16_feature(kb, p);
    return f < K ? f : -1;
}
__host__ __device__ constexpr int f16_ldw(int l_, int key) {
    const int l = f16_canon(l_), xkb = f16_xkb(key);
    return l == kF_mlp1_0 ? (xkb == 1 ? 13 : 61) : l == kF_mlp3_0 ? 56 : l == kF_att_0 ? 200 : l == kF_mlp1_2 || l == kF_mlp3_2 ? 150 : 100;
}
__host__ __device__ constexpr int f16_outputs(int l_) {
    const int l = f16_canon(l_);
    return l == kF_mlp1_0 || l == kF_mlp3_0 ? 150 : l == kF_mlp2_2 ? 50 : l == kF_att_4 || l == kF_mlp3_6 ? 1 : 100;
}
// a single output fills all 16 rows of its tile: every lane of a row gets the row's value
__host__ __device__ constexpr bool f16_replicate(int l) { return l == kF_att_4 || l == kF_mlp3_6; }

struct F16PackPlan {
    const float* W[11];  // torch.nn.Linear weights in state_dict order (the 11 layers of sarl.ValueNetwork)
    const float* b[11];
    int xkb;  // the stream's key
};

// thread = one half of one item (item, lane, j), then one float of the bias array
__global__ void sarl_f16_pack_kernel(F16PackPlan plan, _Float16* stream, float* bias) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int xkb = plan.xkb;
    const int n_w = f16_total_items(xkb) * 512, n_b = f16_total_tiles(xkb) * 256;
    if (idx >= n_w + n_b) return;
    if (idx >= n_w) {  // bias[tile][lane][i] = b[16 mt + 4 lg + i]
        const int t = (idx - n_w) >> 8, lane = ((idx - n_w) >> 2) & 63, i = idx & 3;
        int l = 0;
        while (l + 1 < kF16Layers && t >= f16_tbase(l + 1, xkb)) ++l;
        const int mt = t - f16_tbase(l, xkb);
        const int f = f16_replicate(l) ? 0 : 16 * mt + 4 * (lane >> 4) + i;
        bias[idx - n_w] = f < f16_outputs(l) ? plan.b[f16_src(l)][f] : 0.0f;
        return;
    }
    const int item = idx >> 9, lane = (idx >> 3) & 63, j = idx & 7;
    float w = 0.0f;
    if (item < f16_ibase(kF16Layers, xkb)) {
        int l = 0;
        while (l + 1 < kF16Layers && item >= f16_ibase(l + 1, xkb)) ++l;
        const F16Shape s = f16_shape(l, xkb);
        const int r = item - f16_ibase(l, xkb), mt = r / s.kb, kb = r % s.kb;
        const int n = f16_replicate(l) ? 0 : 16 * mt + (lane & 15);
        const int col = f16_col(l, xkb, kb, 8 * (lane >> 4) + j);
        if (n < f16_outputs(l) && col >= 0) w = plan.W[f16_src(l)][(size_t)n * f16_ldw(l, xkb) + col];
    }
    const _Float16 hi = (_Float16)w;
    const _Float16 lo = (_Float16)((w - (float)hi) * kF16Scale);
    stream[(size_t)item * 1024 + lane * 8 + j] = hi;
    stream[(size_t)item * 1024 + 512 + lane * 8 + j] = lo;
}

struct F16Item {
    f16x8 hi, lo;
};
// DEPTH items in flight per wave: 6, or 4 where the activations of 4 or 5 humans leave no room for more (there an item feeds
// 12 or 15 matrix instructions, ~200 cycles: 4 in flight cover the L2's latency as 6 do for the shorter items of smaller crowds)
template <int DEPTH>
struct F16StreamT {
    static constexpr int kDepth = DEPTH;
    __amdgpu_buffer_rsrc_t rsrc;
    uint32_t voff;    // lane * 16
    F16Item q[DEPTH];  // items I .. I + DEPTH - 1 of the running position (item J in slot J % DEPTH)
};
template <class WS>
__device__ __forceinline__ F16Item f16_item(const WS& s, int J) {
    F16Item it;
    it.hi = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(s.rsrc, s.voff, J * 2048, 0));
    it.lo = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(s.rsrc, s.voff + 1024, J * 2048, 0));
    return it;
}
template <int QT, class WS>
__device__ __forceinline__ F16Item f16_take(WS& s, int I) {
    static_assert(QT % WS::kDepth == 0, "slot I % depth must survive the wrap of the stream");
    const F16Item v = s.q[I % WS::kDepth];
    s.q[I % WS::kDepth] = f16_item(s, (I + WS::kDepth) % QT);
    return v;
}

// one output tile's worth of a row's activations (4 features per lane), split
struct F16Act {
    f16x4 hi, lo;
};
__device__ __forceinline__ F16Act f16_split(f32x4 a) {
    F16Act r;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const _Float16 h = (_Float16)a[i];
        r.hi[i] = h;
        r.lo[i] = (_Float16)((a[i] - (float)h) * kF16Scale);
    }
    return r;
}
// B operand of an input block: two consecutive output tiles of the previous layer
struct F16In {
    f16x8 hi, lo;
};
__device__ __forceinline__ F16In f16_join(const F16Act& a, const F16Act& b) {
    F16In r;
    r.hi = __builtin_shufflevector(a.hi, b.hi, 0, 1, 2, 3, 4, 5, 6, 7);
    r.lo = __builtin_shufflevector(a.lo, b.lo, 0, 1, 2, 3, 4, 5, 6, 7);
    return r;
}
// a row's activations of one layer, kept as the B operands they will be: block j = output tiles 2 j, 2 j + 1 (4 consecutive
// registers each for hi and lo: joining two tiles at the point of use costs moves and a fresh register tuple per instruction)
template <int KB>
struct F16Tiles {
    F16In blk[KB];
    __device__ __forceinline__ void set(int mt, const F16Act& v) {
#pragma unroll
        for (int i = 0; i < 4; ++i) blk[mt >> 1].hi[4 * (mt & 1) + i] = v.hi[i], blk[mt >> 1].lo[4 * (mt & 1) + i] = v.lo[i];
    }
};
// ReLU that keeps a NaN of either sign (v_max_f32 would return 0 for it)
__device__ __forceinline__ f32x4 f16_relu(f32x4 v) {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = v[i] < 0.0f ? 0.0f : v[i];
    return v;
}

// emit(nt, mt, act(main + cross / S + b)) for NT N tiles and every output tile; in(nt, kb) = the split B operand of block kb
template <int KEY, int L, int NT, bool RELU, class WS, class In, class Emit>
__device__ __forceinline__ void f16_dense(WS& ws, gf32x4_p bias, int lane, In in, Emit emit) {
    constexpr F16Shape S = f16_shape(L, KEY);
    constexpr int QT = f16_total_items(KEY), IB = f16_ibase(L, KEY), TB = f16_tbase(L, KEY);
#pragma unroll
    for (int mt = 0; mt < S.mt; ++mt) {
        const f32x4 b = bias[(TB + mt) * 64 + lane];
        f32x4 main[NT], cross[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) main[nt] = cross[nt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int kb = 0; kb < S.kb; ++kb) {
            const F16Item w = f16_take<QT>(ws, IB + mt * S.kb + kb);
            __builtin_amdgcn_sched_barrier(0);  // the request for item I + depth is issued HERE, not sunk to its use
            // (the two products of an N tile's cross term are NT instructions apart: no dependent pair back to back)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const F16In x = in(nt, kb);
                main[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w.hi, x.hi, main[nt], 0, 0, 0);
                cross[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w.hi, x.lo, cross[nt], 0, 0, 0);
            }
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) cross[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w.lo, in(nt, kb).hi, cross[nt], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            f32x4 y;
#pragma unroll
            for (int i = 0; i < 4; ++i) y[i] = __builtin_fmaf(cross[nt][i], kF16InvScale, main[nt][i]) + b[i];  // (1 / S is a power of two: the product is exact either way)
            emit(nt, mt, RELU ? f16_relu(y) : y);
        }
    }
}

// X: the feature kernel's fragment order, X[((tile * NT + h) * ks_x + ks) * 64 + lane] = feature 4 ks + (lane >> 4) of human h
// of group lane & 15.  V[group] out.  Persistent: wave w of the grid takes tiles w, w + waves, ...
// KEY = the stream's key (f16_key): input blocks of mlp1.0 — 1 (13-wide rows, X k-steps 0..3) or 2 (61-wide rows, k-steps
// 0..15) — + 4 for crowds of 4 and 5.
// NT = humans of the crowd (N tiles per wave), 1..5; hcount = humans present per group (the rest carry no weight).
// ATT (compile time; cn_sarl_select_attention): lanes 0..15 also write their group's softmax weights, att_out [n_groups][NT].
template <int KEY, int NT, bool ATT = false>
__global__ __launch_bounds__(kRegWaves * 64) void sarl_f16_kernel(const _Float16* stream, const float* bias_, const float* X, float* V,
                                                                  int n_groups, int n_tiles, int ks_x, const int* hcount,
                                                                  [[maybe_unused]] float* att_out = nullptr) {
    constexpr int XKB = f16_xkb(KEY);
    static_assert(NT >= 1 && NT <= kRegHumans && (XKB == 1 || XKB == 2) && KEY == f16_key(XKB, NT), "1..5 humans on 13- or 61-wide rows");
    constexpr int QT = f16_total_items(KEY), XKS = XKB == 1 ? 4 : 16;
    constexpr int NA = f16_dup(KEY) ? 3 : NT;  // humans of mlp1's first pass
    const int lane = threadIdx.x & 63;
    const int wid = blockIdx.x * kRegWaves + (threadIdx.x >> 6), nw = gridDim.x * kRegWaves;
    if (wid >= n_tiles) return;
    F16StreamT<(NT >= 4 ? 4 : 6)> ws;
    ws.rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16*>(stream), 0, QT * 2048, 0x00020000);  // raw, 32-bit elements
    ws.voff = (uint32_t)lane * 16u;
#pragma unroll
    for (int i = 0; i < ws.kDepth; ++i) ws.q[i] = f16_item(ws, i);
    const gf32x4_p bias0 = (gf32x4_p)bias_;
    // per-human features (mlp2's output, f32: 16 NT registers) wait in LDS while the attention layers run: wave-private, no barrier
    __shared__ f32x4 park[kRegWaves][NT * 4][64];
    f32x4(*const mypark)[64] = park[threadIdx.x >> 6];
    // ... and so does the split mean of mlp1's output (attention.0's second half), from where mlp1.2 leaves it
    __shared__ F16Act gpark[kRegWaves][8][64];
    F16Act(*const mygm)[64] = gpark[threadIdx.x >> 6];
    const gfloat_p Xg = as_global(X) + lane;
    const F16Act zero = {f16x4{0, 0, 0, 0}, f16x4{0, 0, 0, 0}};
    for (int tile = wid; tile < n_tiles; tile += nw) {
        // the biases are re-read per tile, a tile's 16 bytes at a time: opaque to the compiler here, or it hoists all 74 loads
        // (296 registers) out of this loop
        gf32x4_p bias = bias0;
        asm volatile("" : "+s"(bias));
        const gfloat_p xt = Xg + (size_t)tile * NT * ks_x * 64;
        const int cnt = hcount[(size_t)tile * kSarlGroups + (lane & 15)];
        // mlp1.0's operand: the lane's X k-steps, 4 or 8 to a block
        F16In xin[NT][XKB];
        float self0, self1;  // features 0..3 / 4..7 of human 0's row by lane group: the self state lives in 0..5
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            float x[XKS];
#pragma unroll
            for (int ks = 0; ks < XKS; ++ks) x[ks] = xt[(nt * ks_x + ks) * 64];
            if (nt == 0) self0 = x[0], self1 = x[1];
#pragma unroll
            for (int kb = 0; kb < XKB; ++kb) {
                const F16Act lo4 = f16_split(f32x4{x[8 * kb], x[8 * kb + 1], x[8 * kb + 2], x[8 * kb + 3]});
                const F16Act hi4 = XKB == 1 ? zero : f16_split(f32x4{x[(8 * kb + 4) % XKS], x[(8 * kb + 5) % XKS], x[(8 * kb + 6) % XKS], x[(8 * kb + 7) % XKS]});
                xin[nt][kb] = f16_join(lo4, hi4);
            }
        }
        F16Tiles<4> h2[NT];
        mygm[7][lane] = zero;
        const float fc = (float)cnt;
        // mlp1 for humans BASE .. BASE + N - 1; the sum of its output over the humans present, for the mean (sarl.py:42), passes
        // from the first pass to the second through the (still unused) feature rows of the LDS
        const auto mlp1 = [&](auto base_, auto n_, auto l0_, auto l2_) {
            constexpr int BASE = decltype(base_)::value, N = decltype(n_)::value, L0 = decltype(l0_)::value, L2 = decltype(l2_)::value;
            F16Tiles<5> h1[N];
            f32x4 msum;
            f16_dense<KEY, L0, N, true>(ws, bias, lane, [&](int nt, int kb) { return xin[BASE + nt][kb]; },
                                       [&](int nt, int mt, f32x4 y) { h1[nt].set(mt, f16_split(y)); });
            f16_dense<KEY, L2, N, true>(ws, bias, lane, [&](int nt, int kb) { return h1[nt].blk[kb]; },
                                       [&](int nt, int mt, f32x4 y) {
                                           h2[BASE + nt].set(mt, f16_split(y));
                                           if (nt == 0 && BASE != 0) msum = mypark[mt][lane];
#pragma unroll
                                           for (int i = 0; i < 4; ++i) {
                                               const float v = BASE + nt < cnt ? y[i] : 0.0f;
                                               msum[i] = BASE + nt == 0 ? v : msum[i] + v;
                                           }
                                           if (nt == N - 1 && BASE + N == NT) {
                                               f32x4 m;
#pragma unroll
                                               for (int i = 0; i < 4; ++i) m[i] = msum[i] / fc;
                                               mygm[mt][lane] = f16_split(m);
                                           } else if (nt == N - 1) {
                                               mypark[mt][lane] = msum;
                                           }
                                       });
        };
        using std::integral_constant;
        mlp1(integral_constant<int, 0>{}, integral_constant<int, NA>{}, integral_constant<int, kF_mlp1_0>{}, integral_constant<int, kF_mlp1_2>{});
        if constexpr (NA < NT)
            mlp1(integral_constant<int, NA>{}, integral_constant<int, NT - NA>{}, integral_constant<int, kF_mlp1_0b>{},
                 integral_constant<int, kF_mlp1_2b>{});
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) h2[nt].set(7, zero);
        {
            F16Tiles<4> t1[NT];
            f16_dense<KEY, kF_mlp2_0, NT, true>(ws, bias, lane, [&](int nt, int kb) { return h2[nt].blk[kb]; },
                                               [&](int nt, int mt, f32x4 y) { t1[nt].set(mt, f16_split(y)); });
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) t1[nt].set(7, zero);
            f16_dense<KEY, kF_mlp2_2, NT, false>(ws, bias, lane, [&](int nt, int kb) { return t1[nt].blk[kb]; },
                                                [&](int nt, int mt, f32x4 y) { mypark[nt * 4 + mt][lane] = y; });
        }
        float e[NT];
        {
            F16Tiles<4> a0[NT], a1[NT];
            f16_dense<KEY, kF_att_0, NT, true>(
                ws, bias, lane,
                [&](int nt, int kb) { return kb < 4 ? h2[nt].blk[kb] : f16_join(mygm[2 * kb - 8][lane], mygm[2 * kb - 7][lane]); },
                [&](int nt, int mt, f32x4 y) { a0[nt].set(mt, f16_split(y)); });
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) a0[nt].set(7, zero);
            f16_dense<KEY, kF_att_2, NT, true>(ws, bias, lane, [&](int nt, int kb) { return a0[nt].blk[kb]; },
                                              [&](int nt, int mt, f32x4 y) { a1[nt].set(mt, f16_split(y)); });
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) a1[nt].set(7, zero);
            float sc[NT];  // attention.4: the score of (human, group) in every register of the group's lanes
            f16_dense<KEY, kF_att_4, NT, false>(ws, bias, lane, [&](int nt, int kb) { return a1[nt].blk[kb]; },
                                               [&](int nt, int, f32x4 y) { sc[nt] = y[0]; });
            // masked softmax without max subtraction (sarl.py:52-53); an absent human carries no weight
            float total = 0.0f;
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
        }
        // weighted feature sum (sarl.py:60), then joint = [self | weighted feature] (sarl.py:61)
        F16Tiles<2> jn;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            f32x4 sum = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const f32x4 f = mypark[nt * 4 + t][lane];
#pragma unroll
                for (int i = 0; i < 4; ++i) sum[i] += e[nt] * f[i];
            }
            if (t == 3) sum[2] = self0, sum[3] = self1;  // the slots of features 50, 51 (lane group 0) .. 62, 63: zero weights but for self
            jn.set(t, f16_split(sum));
        }
        F16Tiles<5> j1;
        F16Tiles<4> j2, j3;
        float val = 0.0f;
        f16_dense<KEY, kF_mlp3_0, 1, true>(ws, bias, lane, [&](int, int kb) { return jn.blk[kb]; },
                                          [&](int, int mt, f32x4 y) { j1.set(mt, f16_split(y)); });
        f16_dense<KEY, kF_mlp3_2, 1, true>(ws, bias, lane, [&](int, int kb) { return j1.blk[kb]; },
                                          [&](int, int mt, f32x4 y) { j2.set(mt, f16_split(y)); });
        j2.set(7, zero);
        f16_dense<KEY, kF_mlp3_4, 1, true>(ws, bias, lane, [&](int, int kb) { return j2.blk[kb]; },
                                          [&](int, int mt, f32x4 y) { j3.set(mt, f16_split(y)); });
        j3.set(7, zero);
        f16_dense<KEY, kF_mlp3_6, 1, false>(ws, bias, lane, [&](int, int kb) { return j3.blk[kb]; },
                                           [&](int, int, f32x4 y) { val = y[0]; });
        if (lane < kSarlGroups) {
            const size_t G = (size_t)tile * kSarlGroups + lane;
            if (G < (size_t)n_groups) V[G] = val;
        }
        // the stream position wraps to item 0 here: the padding items are consumed so that slot I % depth stays aligned
#pragma unroll
        for (int i = f16_ibase(kF16Layers, KEY); i < QT; ++i) (void)f16_take<QT>(ws, i);
    }
}

}  // namespace cn
