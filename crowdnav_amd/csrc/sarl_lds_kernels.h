// The six LDS value-network kernels: a workgroup per tile of 16 groups, activations in LDS in fragment order (blocks: sarl_net.h)
#pragma once
#include "sarl_net.h"

namespace cn {

// ------------------------------------------------------------------------------------ LDS layouts
// One per kernel, written once: a list of declarations that carves the buffers out of `base` in order and ends with `end`.
// The kernel expands it on `lds` (P = float*) and so declares its buffer pointers — the very pointer additions it always
// made; the *_lds_bytes function below it expands the same text on a zero word offset (P = size_t) and returns the bytes to
// launch with, which sarl_size_network also tests against 160 KiB.  A buffer added to the list moves both.  (A layout object
// returned by a function was tried first: every kernel that took its pointers from one came out with other registers.)
// n: SarlNet or SarlNetRef (the ks_* members); rt: the row tiles the kernel holds at a time.
#define CN_SARL_PIPE_LDS(P, base, n, H)                                                                       \
    P bufA = base;                    /* [H][ks_a][64]  wide hidden layers */                                  \
    P bufB = bufA + H * n.ks_a * 64;  /* [H][ks_b][64]  X staging, then mlp1 output (h2), then attention.2 */  \
    P bufC = bufB + H * n.ks_b * 64;  /* [H][ks_c][64]  mlp2 output (per-human feature) */                     \
    P gbuf = bufC + H * n.ks_c * 64;  /* [ks_b][64]     mean over humans of h2 */                              \
    P jbuf = gbuf + n.ks_b * 64;      /* [ks_a][64]     joint state / value-head ping */                       \
    P kbuf = jbuf + n.ks_a * 64;      /* [ks_a][64]     global attention term */                               \
    P sbuf = kbuf + n.ks_a * 64;      /* [H][ks_s][64]  attention scores -> weights */                         \
    P vbuf = sbuf + H * n.ks_s * 64;  /* [kSarlThreads] partial sums of attention.4 */                         \
    P hcnt = vbuf + kSarlThreads;     /* [16] (int)     humans present per group */                            \
    P mbuf = hcnt + 16;               /* [ks_a][64]     value-head pong (side chain) */                        \
    P end = mbuf + n.ks_a * 64
__host__ inline size_t sarl_pipe_lds_bytes(const SarlNet& net, int H) {
    CN_SARL_PIPE_LDS(size_t, 0, net, H);
    return sizeof(float) * end;
}
#define CN_SARL_CHUNKED_LDS(P, base, n, rt)                                                         \
    P bufA = base;                     /* [rt][ks_a][64] */                                         \
    P bufB = bufA + rt * n.ks_a * 64;  /* [rt][ks_b][64] */                                         \
    P bufC = bufB + rt * n.ks_b * 64;  /* [rt][ks_c][64] */                                         \
    P gbuf = bufC + rt * n.ks_c * 64;  /* [ks_b][64]  sum, then mean, over humans of h2 */          \
    P jbuf = gbuf + n.ks_b * 64;       /* [ks_a][64] */                                             \
    P kbuf = jbuf + n.ks_a * 64;       /* [ks_a][64] */                                             \
    P sbuf = kbuf + n.ks_a * 64;       /* [rt][ks_s][64] */                                         \
    P wsum = sbuf + rt * n.ks_s * 64;  /* [ks_c][64]  sum_h exp(score_h) * feature_h */             \
    P den = wsum + n.ks_c * 64;        /* [64]        sum_h exp(score_h) (16 groups used) */        \
    P vbuf = den + 64;                 /* [kSarlThreads] (written before it is read: not zeroed) */ \
    [[maybe_unused]] P end = vbuf + kSarlThreads
__host__ inline size_t sarl_chunked_lds_bytes(const SarlNet& net) {
    CN_SARL_CHUNKED_LDS(size_t, 0, net, kSarlChunk);
    return sizeof(float) * end;
}
// cadrl_mlp_kernel (rt = H) and cadrl_mlp_chunked_kernel (rt = the chunk, vmin_words = 16: the running minimum per group)
#define CN_CADRL_LDS(P, base, n, rt, vmin_words)                                          \
    P bufA = base;                     /* [rt][ks_a][64]  first / third hidden layer */   \
    P bufB = bufA + rt * n.ks_a * 64;  /* [rt][ks_b][64]  X staging, second hidden layer */ \
    P sbuf = bufB + rt * n.ks_b * 64;  /* [rt][ks_s][64]  the rows' values */             \
    P vmin = sbuf + rt * n.ks_s * 64;  /* [vmin_words] */                                 \
    [[maybe_unused]] P end = vmin + vmin_words
__host__ inline size_t cadrl_lds_bytes(const SarlNet& net, int rt, bool chunked) {
    CN_CADRL_LDS(size_t, 0, net, rt, (chunked ? 16 : 0));
    return sizeof(float) * end;
}
// lstm_mlp_kernel (rt = H) and lstm_mlp_anyh_kernel (rt = 1: this step's input row tile alone)
#define CN_LSTM_LDS(P, base, n, rt, hid, ks_g, ks_h)                                                              \
    P xs = base;                        /* [rt][ks_x][64]  input row tiles (human t = LSTM step t) */             \
    P pbuf = xs + rt * n.ks_x * 64;     /* [rt][ks_b][64]  ValueNetwork2.mlp1 ping (ks_b = 0 otherwise) */        \
    P qbuf = pbuf + rt * n.ks_b * 64;   /* [rt][ks_c][64]  ... pong: the LSTM input when pairwise */              \
    P gates = qbuf + rt * n.ks_c * 64;  /* [ks_g][64]      i | f | g | o pre-activations */                       \
    P hbuf = gates + ks_g * 64;         /* [ks_h][64]      hidden state (A operand of the next step) */           \
    P cbuf = hbuf + ks_h * 64;          /* [hid][16]       cell state */                                          \
    P jbuf = cbuf + hid * kSarlGroups;  /* [ks_a][64] */                                                          \
    P kbuf = jbuf + n.ks_a * 64;        /* [ks_a][64] */                                                          \
    P sbuf = kbuf + n.ks_a * 64;        /* [ks_s][64] */                                                          \
    P end = sbuf + n.ks_s * 64
__host__ inline size_t lstm_lds_bytes(const SarlNet& net, int rt, int hid) {
    const int ks_g = net.L[kL_mlp1_0].ctiles * 4, ks_h = sarl_ks(hid);
    CN_LSTM_LDS(size_t, 0, net, rt, hid, ks_g, ks_h);
    return sizeof(float) * end;
}

// Persistent form: a workgroup (one per CU: the tile's activations fill the LDS) strides over the tiles; LDS is zeroed once
// per launch instead of once per tile (every k-padding word the MFMA loops read is either written by the producing layer —
// whole column tiles — or zeroed explicitly below); layers are separated by lds_barrier, and every layer's first B
// fragments are requested BEFORE the barrier that precedes it (dense_prefetch), while the previous layer's epilogue and the
// barrier wait are still in progress.
// The value head of tile t - 1 (mlp3: three 16-row layers + the single-output layer, 13 k of a tile's 84 k ticks when run
// on its own: 16 rows cannot fill the workgroup) runs on the waves that idle during tile t's 7-column-tile layers:
//   slot of tile t            main waves 0..6 (0..9)      side waves
//   mlp1.2                    h2                          7..15: mlp3.0 (t - 1)   jbuf -> mbuf
//   mean + mlp2.0                                         7..13: mlp3.2 (t - 1)   mbuf -> jbuf
//   mlp2.2 + att0 global      features, global term       7..13: mlp3.4 (t - 1)   jbuf -> mbuf
//   att0 local                                            15:    mlp3.6 (t - 1)   mbuf -> V   (one wave, shuffles)
// The side chain has its own pong buffer (mbuf: kbuf carries tile t's global attention term in the same slots) and the
// joint state of tile t is written — self features from registers, weighted sum, zero padding — only in tile t's last slot,
// after the side chain has consumed the previous one.  The last tile's head runs after the loop on all waves.
// ATT (compile time; cn_sarl_select_attention): the softmax threads also write their group's weights, att [n_groups][H].
// (the fragment words are spelled out here and in the kernels below, not tile_word(): through the call hipcc schedules
// sarl_mlp_pipe_kernel<1> and the LSTM kernels differently)
template <int H, bool ATT = false>
__global__ __launch_bounds__(kSarlThreads) void sarl_mlp_pipe_kernel(SarlNetRef net, const float* X, float* V, int n_groups,
                                                                     int n_tiles, const int* hcount, [[maybe_unused]] float* att = nullptr) {
    extern __shared__ float lds[];
    CN_SARL_PIPE_LDS(float*, lds, net, H);
    int* hc = reinterpret_cast<int*>(hcnt);
    int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    zero_lds(lds, (size_t)(end - lds), tid);
    const int nf = net.nf;
    const int x_words = H * net.ks_x * 64;
    float* xs = bufB;
    BFrag pre = dense_prefetch(layer_of(net, kL_mlp1_0), wave, lane);
    lds_barrier();
    int prev_tile = -1;
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        asm volatile("" : "+v"(tid), "+v"(lane));
        wave = __builtin_amdgcn_readfirstlane(tid >> 6);
        SarlNetRef nn = net;
        asm volatile("" : "+s"(nn.base));
        const SarlNetRef* n = &nn;
        const bool side = prev_tile >= 0;  // a previous tile's value head is pending
        const float* xg = X + (size_t)tile * x_words;
        for (int i = tid; i < x_words; i += kSarlThreads) xs[i] = xg[i];
        if (tid < kSarlGroups) hc[tid] = hcount[(size_t)tile * kSarlGroups + tid];
        __syncthreads();  // X came from global memory
        // self_state = state[:, 0, :6] (sarl.py:36): kept in a register until the joint state of this tile is assembled
        float self_val = 0.0f;
        if (tid < kSarlGroups * 6) {
            const int g = tid & 15, f = tid >> 4;
            self_val = xs[(f >> 2) * 64 + (f & 3) * 16 + g];
        }
        dense_mfma<H, true>(layer_of(*n, kL_mlp1_0), xs, n->ks_x, bufA, n->ks_a, true, nullptr, wave, lane, &pre);
        pre = dense_prefetch(layer_of(*n, kL_mlp1_2), wave, lane);
        lds_barrier();
        dense_mfma<H, true>(layer_of(*n, kL_mlp1_2), bufA, n->ks_a, bufB, n->ks_b, true, nullptr, wave, lane, &pre);  // h2
        if (side) dense_mfma<1>(layer_of(*n, kL_mlp3_0), jbuf, n->ks_a, mbuf, n->ks_a, true, nullptr, wave, lane, nullptr, 7, 9);
        pre = dense_prefetch(layer_of(*n, kL_mlp2_0), wave, lane);
        lds_barrier();
        if (n->with_global) {
            for (int i = tid; i < n->ks_b * 64; i += kSarlThreads) {
                const int cnt = hc[i & 15];
                float sum = 0.0f;
#pragma unroll
                for (int h = 0; h < H; ++h) sum += h < cnt ? bufB[h * n->ks_b * 64 + i] : 0.0f;
                gbuf[i] = sum / (float)cnt;
            }
        }
        dense_mfma<H, true>(layer_of(*n, kL_mlp2_0), bufB, n->ks_b, bufA, n->ks_a, true, nullptr, wave, lane, &pre);
        if (side) dense_mfma<1>(layer_of(*n, kL_mlp3_2), mbuf, n->ks_a, jbuf, n->ks_a, true, nullptr, wave, lane, nullptr, 7, 7);
        pre = dense_prefetch(layer_of(*n, kL_mlp2_2), wave, lane);
        lds_barrier();
        dense_mfma<H, true>(layer_of(*n, kL_mlp2_2), bufA, n->ks_a, bufC, n->ks_c, false, nullptr, wave, lane, &pre);  // features
        if (n->with_global) dense_mfma<1>(layer_of(*n, kL_att0_global), gbuf, n->ks_b, kbuf, n->ks_a, false, nullptr, wave, lane);
        if (side) dense_mfma<1>(layer_of(*n, kL_mlp3_4), jbuf, n->ks_a, mbuf, n->ks_a, true, nullptr, wave, lane, nullptr, 7, 7);
        pre = dense_prefetch(layer_of(*n, kL_att0_local), wave, lane);
        lds_barrier();
        dense_mfma<H, true>(layer_of(*n, kL_att0_local), bufB, n->ks_b, bufA, n->ks_a, true, n->with_global ? kbuf : nullptr,
                            wave, lane, &pre);
        if (side && wave == 15) value_head_on_one_wave(layer_of(*n, kL_mlp3_6), mbuf, V, (size_t)prev_tile, n_groups, lane);
        pre = dense_prefetch(layer_of(*n, kL_att_2), wave, lane);
        lds_barrier();
        dense_mfma<H, true>(layer_of(*n, kL_att_2), bufA, n->ks_a, bufB, n->ks_b, true, nullptr, wave, lane, &pre);
        lds_barrier();
        dense_vec1<H>(layer_of(*n, kL_att_4), bufB, n->ks_b, sbuf, n->ks_s, vbuf, tid);  // score (h, g) at h*ks_s*64 + g
        pre = dense_prefetch(layer_of(*n, kL_mlp1_0), wave, lane);  // the next tile's first layer
        lds_barrier();
        // masked softmax without max subtraction (sarl.py:52-53)
        if (tid < kSarlGroups) {
            float e[H], total = 0.0f;
            const int cnt = hc[tid];
#pragma unroll
            for (int h = 0; h < H; ++h) {
                const float sc = sbuf[h * n->ks_s * 64 + tid];
                e[h] = h < cnt ? masked_exp(sc) : 0.0f;
                total += e[h];
            }
#pragma unroll
            for (int h = 0; h < H; ++h) sbuf[h * n->ks_s * 64 + tid] = e[h] / total;
            if constexpr (ATT) {
                const size_t G = (size_t)tile * kSarlGroups + tid;
                if (G < (size_t)n_groups)
#pragma unroll
                    for (int h = 0; h < H; ++h) att[G * H + h] = sbuf[h * n->ks_s * 64 + tid];
            }
        }
        lds_barrier();
        // the joint state of this tile: self features, weighted feature sum (sarl.py:60), zero k padding
        if (tid < kSarlGroups * 6) {
            const int g = tid & 15, f = tid >> 4;
            jbuf[(f >> 2) * 64 + (f & 3) * 16 + g] = self_val;
        }
        for (int i = tid; i < kSarlGroups * nf; i += kSarlThreads) {
            const int g = i & 15, c = i >> 4;
            const int src = (c >> 2) * 64 + (c & 3) * 16 + g;
            float sum = 0.0f;
#pragma unroll
            for (int h = 0; h < H; ++h) sum += sbuf[h * n->ks_s * 64 + g] * bufC[h * n->ks_c * 64 + src];
            const int f = 6 + c;
            jbuf[(f >> 2) * 64 + (f & 3) * 16 + g] = sum;
        }
        for (int i = tid; i < kSarlGroups * (layer_of(*n, kL_mlp3_0).kpad * 4 - 6 - nf); i += kSarlThreads) {
            const int g = i & 15, f = 6 + nf + (i >> 4);
            jbuf[(f >> 2) * 64 + (f & 3) * 16 + g] = 0.0f;
        }
        lds_barrier();
        prev_tile = tile;
    }
    if (prev_tile >= 0) {  // the last tile's value head, on the whole workgroup
        dense_mfma<1>(layer_of(net, kL_mlp3_0), jbuf, net.ks_a, mbuf, net.ks_a, true, nullptr, wave, lane);
        lds_barrier();
        dense_mfma<1>(layer_of(net, kL_mlp3_2), mbuf, net.ks_a, jbuf, net.ks_a, true, nullptr, wave, lane);
        lds_barrier();
        dense_mfma<1>(layer_of(net, kL_mlp3_4), jbuf, net.ks_a, mbuf, net.ks_a, true, nullptr, wave, lane);
        lds_barrier();
        if (wave == 15) value_head_on_one_wave(layer_of(net, kL_mlp3_6), mbuf, V, (size_t)prev_tile, n_groups, lane);
    }
}

// sarl.ValueNetwork for MORE humans than one tile's LDS holds (H > kSarlMaxHumans; e.g. the 20-human crowds of
// BASELINE configs[3]): the humans of a tile's 16 groups stream through in chunks of HC row tiles.
//   pass 1  mlp1 of every chunk, summed over the humans -> the global state (mean) and its attention term
//   pass 2  mlp1 again (cheaper than parking [H][112] floats per group row in LDS), mlp2, attention; exp(score) and
//           exp(score) * feature accumulate per group in human order, the division by the total comes last
//           (the reference divides first: w_h = e_h / total, then sums w_h f_h — same value to rounding)
// then the value head.  Rows of a partial last chunk are computed on zero inputs and masked out of every sum.
// ATT (compile time): thread g < 16 writes exp(score) of its group's humans into att [n_groups][H] chunk by chunk and divides
// that row by the total after the last chunk.
template <int HC, bool ATT = false>
__global__ __launch_bounds__(kSarlThreads) void sarl_mlp_chunked_kernel(SarlNet net, const float* X, float* V,
                                                                        int n_groups, [[maybe_unused]] float* att = nullptr) {
    extern __shared__ float lds[];
    const int H = net.H;
    CN_SARL_CHUNKED_LDS(float*, lds, net, HC);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const size_t tile = blockIdx.x;
    const float* xg = X + tile * H * net.ks_x * 64;
    zero_lds(lds, (size_t)(vbuf - lds), tid);
    __syncthreads();
    copy_self_state(jbuf, xg, tid);
    auto stage = [&](int h0, int nh) {  // X rows of humans [h0, h0 + nh) -> bufB, zeros beyond
        for (int i = tid; i < HC * net.ks_x * 64; i += kSarlThreads)
            bufB[i] = (i / (net.ks_x * 64) < nh) ? xg[(size_t)h0 * net.ks_x * 64 + i] : 0.0f;
    };
    for (int h0 = 0; h0 < H; h0 += HC) {
        const int nh = H - h0 < HC ? H - h0 : HC;
        stage(h0, nh);
        __syncthreads();
        dense_mfma<HC>(net.L[kL_mlp1_0], bufB, net.ks_x, bufA, net.ks_a, true, nullptr, wave, lane);
        __syncthreads();
        dense_mfma<HC>(net.L[kL_mlp1_2], bufA, net.ks_a, bufB, net.ks_b, true, nullptr, wave, lane);
        __syncthreads();
        for (int i = tid; i < net.ks_b * 64; i += kSarlThreads) {
            float sum = gbuf[i];
            for (int rt = 0; rt < nh; ++rt) sum += bufB[rt * net.ks_b * 64 + i];
            gbuf[i] = sum;
        }
        __syncthreads();
    }
    if (net.with_global) {
        for (int i = tid; i < net.ks_b * 64; i += kSarlThreads) gbuf[i] = gbuf[i] / (float)H;
        __syncthreads();
        dense_mfma<1>(net.L[kL_att0_global], gbuf, net.ks_b, kbuf, net.ks_a, false, nullptr, wave, lane);
        __syncthreads();
    }
    const int nf = net.L[kL_mlp2_2].N;
    for (int h0 = 0; h0 < H; h0 += HC) {
        const int nh = H - h0 < HC ? H - h0 : HC;
        stage(h0, nh);
        __syncthreads();
        dense_mfma<HC>(net.L[kL_mlp1_0], bufB, net.ks_x, bufA, net.ks_a, true, nullptr, wave, lane);
        __syncthreads();
        dense_mfma<HC>(net.L[kL_mlp1_2], bufA, net.ks_a, bufB, net.ks_b, true, nullptr, wave, lane);
        __syncthreads();
        dense_mfma<HC>(net.L[kL_mlp2_0], bufB, net.ks_b, bufA, net.ks_a, true, nullptr, wave, lane);
        __syncthreads();
        dense_mfma<HC>(net.L[kL_mlp2_2], bufA, net.ks_a, bufC, net.ks_c, false, nullptr, wave, lane);
        __syncthreads();
        dense_mfma<HC>(net.L[kL_att0_local], bufB, net.ks_b, bufA, net.ks_a, true, net.with_global ? kbuf : nullptr,
                       wave, lane);
        __syncthreads();
        dense_mfma<HC>(net.L[kL_att_2], bufA, net.ks_a, bufB, net.ks_b, true, nullptr, wave, lane);
        __syncthreads();
        dense_vec1<HC>(net.L[kL_att_4], bufB, net.ks_b, sbuf, net.ks_s, vbuf, tid);
        __syncthreads();
        if (tid < kSarlGroups) {  // masked exp without max subtraction (sarl.py:52-53), humans in order
            float total = den[tid];
            for (int rt = 0; rt < nh; ++rt) {
                const float sc = sbuf[rt * net.ks_s * 64 + tid];
                const float e = masked_exp(sc);
                sbuf[rt * net.ks_s * 64 + tid] = e;
                total += e;
                if constexpr (ATT)
                    if (tile * kSarlGroups + tid < (size_t)n_groups) att[(tile * kSarlGroups + tid) * H + h0 + rt] = e;
            }
            den[tid] = total;
        }
        __syncthreads();
        for (int i = tid; i < kSarlGroups * nf; i += kSarlThreads) {
            const int g = i & 15, c = i >> 4;
            const int src = tile_word(c) + g;
            float sum = wsum[src];
            for (int rt = 0; rt < nh; ++rt) sum += sbuf[rt * net.ks_s * 64 + g] * bufC[rt * net.ks_c * 64 + src];
            wsum[src] = sum;
        }
        __syncthreads();
    }
    for (int i = tid; i < kSarlGroups * nf; i += kSarlThreads) {
        const int g = i & 15, c = i >> 4, n = 6 + c;
        jbuf[tile_word(n) + g] = wsum[tile_word(c) + g] / den[g];
    }
    if constexpr (ATT)  // the row this thread wrote above, normalised
        if (tid < kSarlGroups && tile * kSarlGroups + tid < (size_t)n_groups) {
            float* const row = att + (tile * kSarlGroups + tid) * H;
            for (int h = 0; h < H; ++h) row[h] = row[h] / den[tid];
        }
    __syncthreads();
    dense_mfma<1>(net.L[kL_mlp3_0], jbuf, net.ks_a, kbuf, net.ks_a, true, nullptr, wave, lane);
    __syncthreads();
    dense_mfma<1>(net.L[kL_mlp3_2], kbuf, net.ks_a, jbuf, net.ks_a, true, nullptr, wave, lane);
    __syncthreads();
    dense_mfma<1>(net.L[kL_mlp3_4], jbuf, net.ks_a, kbuf, net.ks_a, true, nullptr, wave, lane);
    __syncthreads();
    dense_vec1<1>(net.L[kL_mlp3_6], kbuf, net.ks_a, sbuf, net.ks_s, vbuf, tid);
    __syncthreads();
    if (tid < kSarlGroups) {
        const size_t G = tile * kSarlGroups + tid;
        if (G < (size_t)n_groups) V[G] = sbuf[tid];
    }
}

// cadrl.ValueNetwork (cadrl.py:22-29): the same MLP for every (robot, human) row, then the minimum over the humans
// of a group (cadrl.py:162-163).  Layers live in L[kL_mlp3_0 .. kL_mlp3_6].
template <int H>
__global__ __launch_bounds__(kSarlThreads) void cadrl_mlp_kernel(SarlNet net, const float* X, float* V, int n_groups,
                                                                 const int* hcount) {
    extern __shared__ float lds[];
    CN_CADRL_LDS(float*, lds, net, H, 0);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const size_t tile = blockIdx.x;
    zero_lds(lds, (size_t)H * (net.ks_a + net.ks_b + net.ks_s) * 64, tid);  // (= end - lds; in this form since the first version)
    __syncthreads();
    const float* xg = X + tile * H * net.ks_x * 64;
    for (int i = tid; i < H * net.ks_x * 64; i += kSarlThreads) bufB[i] = xg[i];
    __syncthreads();
    dense_mfma<H>(net.L[kL_mlp3_0], bufB, net.ks_x, bufA, net.ks_a, true, nullptr, wave, lane);
    __syncthreads();
    dense_mfma<H>(net.L[kL_mlp3_2], bufA, net.ks_a, bufB, net.ks_b, true, nullptr, wave, lane);
    __syncthreads();
    dense_mfma<H>(net.L[kL_mlp3_4], bufB, net.ks_b, bufA, net.ks_a, true, nullptr, wave, lane);
    __syncthreads();
    dense_mfma<H>(net.L[kL_mlp3_6], bufA, net.ks_a, sbuf, net.ks_s, false, nullptr, wave, lane);
    __syncthreads();
    if (tid < kSarlGroups) {
        const int cnt = hcount[tile * kSarlGroups + tid];  // humans present (H unless the `mixed` rule)
        const float m = first_min_over_humans(sbuf, net.ks_s * 64, tid, 1, H, cnt, sbuf[tid]);
        const size_t G = tile * kSarlGroups + tid;
        if (G < (size_t)n_groups) V[G] = m;
    }
}

// cadrl.ValueNetwork for MORE humans than the one-tile kernel holds (H > kSarlMaxHumans): the humans of a tile's 16
// groups stream through in chunks of HC row tiles, the per-group minimum (cadrl.py:162-163) accumulates in LDS.  Rows of a
// partial last chunk run on zero inputs and are left out of the minimum.
template <int HC>
__global__ __launch_bounds__(kSarlThreads) void cadrl_mlp_chunked_kernel(SarlNet net, const float* X, float* V,
                                                                         int n_groups) {
    extern __shared__ float lds[];
    const int H = net.H;
    CN_CADRL_LDS(float*, lds, net, HC, 16);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const size_t tile = blockIdx.x;
    const float* xg = X + tile * H * net.ks_x * 64;
    zero_lds(lds, (size_t)HC * (net.ks_a + net.ks_b + net.ks_s) * 64 + 16, tid);  // (= end - lds, as above)
    __syncthreads();
    for (int h0 = 0; h0 < H; h0 += HC) {
        const int nh = H - h0 < HC ? H - h0 : HC;
        for (int i = tid; i < HC * net.ks_x * 64; i += kSarlThreads)
            bufB[i] = (i / (net.ks_x * 64) < nh) ? xg[(size_t)h0 * net.ks_x * 64 + i] : 0.0f;
        __syncthreads();
        dense_mfma<HC>(net.L[kL_mlp3_0], bufB, net.ks_x, bufA, net.ks_a, true, nullptr, wave, lane);
        __syncthreads();
        dense_mfma<HC>(net.L[kL_mlp3_2], bufA, net.ks_a, bufB, net.ks_b, true, nullptr, wave, lane);
        __syncthreads();
        dense_mfma<HC>(net.L[kL_mlp3_4], bufB, net.ks_b, bufA, net.ks_a, true, nullptr, wave, lane);
        __syncthreads();
        dense_mfma<HC>(net.L[kL_mlp3_6], bufA, net.ks_a, sbuf, net.ks_s, false, nullptr, wave, lane);
        __syncthreads();
        if (tid < kSarlGroups) {
            float m = h0 == 0 ? sbuf[tid] : vmin[tid];
            for (int rt = (h0 == 0 ? 1 : 0); rt < nh; ++rt) {
                const float v = sbuf[rt * net.ks_s * 64 + tid];
                m = v < m ? v : m;  // torch.min over dim 0: the first minimum's value
            }
            vmin[tid] = m;
        }
        __syncthreads();
    }
    if (tid < kSarlGroups) {
        const size_t G = tile * kSarlGroups + tid;
        if (G < (size_t)n_groups) V[G] = vmin[tid];
    }
}

// lstm_rl.ValueNetwork1 / ValueNetwork2 (lstm_rl.py:9-66): an LSTM over the humans of a group (in the order the lookahead returns
// them), its final hidden state joined with the robot's 6 self features into the value head.  Layers: L[kL_mlp1_0] =
// weight_ih / bias_ih, L[kL_mlp1_2] = weight_hh / bias_hh (torch gate order i, f, g, o), L[kL_mlp3_*] = the head.
// Row tile t of X is human t of the 16 groups = LSTM time step t, so each step is a 16-row product.
template <int H>
__global__ __launch_bounds__(kSarlThreads) void lstm_mlp_kernel(SarlNet net, const float* X, float* V, int n_groups,
                                                                const int* hcount) {
    extern __shared__ float lds[];
    const int hid = net.L[kL_mlp1_2].K;                   // hidden width (50)
    const int ks_h = sarl_ks(hid), ks_g = net.L[kL_mlp1_0].ctiles * 4;
    CN_LSTM_LDS(float*, lds, net, H, hid, ks_g, ks_h);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const size_t tile = blockIdx.x;
    zero_lds(lds, (size_t)(end - lds), tid);
    __syncthreads();
    const float* xg = X + tile * H * net.ks_x * 64;
    for (int i = tid; i < H * net.ks_x * 64; i += kSarlThreads) xs[i] = xg[i];
    for (int i = tid; i < ks_h * 64; i += kSarlThreads) hbuf[i] = 0.0f;   // h0 = 0
    for (int i = tid; i < hid * kSarlGroups; i += kSarlThreads) cbuf[i] = 0.0f;  // c0 = 0
    for (int i = tid; i < net.ks_a * 64; i += kSarlThreads) jbuf[i] = 0.0f;
    __syncthreads();
    if (tid < kSarlGroups * 6) {
        const int g = tid & 15, n = tid >> 4;
        jbuf[(n >> 2) * 64 + (n & 3) * 16 + g] = xs[(n >> 2) * 64 + (n & 3) * 16 + g];  // self_state = state[:, 0, :6]
    }
    // lstm_rl.ValueNetwork2 (lstm_rl.py:36-66): mlp1 on every human's row first (ReLU between its 4 layers, none after)
    const bool pairwise = net.L[kL_mlp2_0].w != nullptr;
    const float* lstm_in = xs;
    int ks_in = net.ks_x;
    if (pairwise) {
        dense_mfma<H>(net.L[kL_mlp2_0], xs, net.ks_x, pbuf, net.ks_b, true, nullptr, wave, lane);
        __syncthreads();
        dense_mfma<H>(net.L[kL_mlp2_2], pbuf, net.ks_b, qbuf, net.ks_c, true, nullptr, wave, lane);
        __syncthreads();
        dense_mfma<H>(net.L[kL_att_2], qbuf, net.ks_c, pbuf, net.ks_b, true, nullptr, wave, lane);
        __syncthreads();
        dense_mfma<H>(net.L[kL_att_4], pbuf, net.ks_b, qbuf, net.ks_c, false, nullptr, wave, lane);
        __syncthreads();
        lstm_in = qbuf;
        ks_in = net.ks_c;
    }
    for (int t = 0; t < H; ++t) {
        dense_mfma<1>(net.L[kL_mlp1_0], lstm_in + t * ks_in * 64, ks_in, gates, ks_g, false, nullptr, wave, lane);
        __syncthreads();
        dense_mfma<1>(net.L[kL_mlp1_2], hbuf, ks_h, gates, ks_g, false, gates, wave, lane);  // + (W_hh h + b_hh)
        __syncthreads();
        for (int i = tid; i < hid * kSarlGroups; i += kSarlThreads) {
            const int g = i & 15, j = i >> 4;
            if (t >= hcount[tile * kSarlGroups + g]) continue;  // `mixed` rule: this group's episode has fewer humans
            auto at = [&](int n) { return gates[(n >> 2) * 64 + (n & 3) * 16 + g]; };
            const float ig = 1.0f / (1.0f + expf(-at(j)));
            const float fg = 1.0f / (1.0f + expf(-at(hid + j)));
            const float gg = tanhf(at(2 * hid + j));
            const float og = 1.0f / (1.0f + expf(-at(3 * hid + j)));
            const float c = fg * cbuf[i] + ig * gg;
            cbuf[i] = c;
            hbuf[(j >> 2) * 64 + (j & 3) * 16 + g] = og * tanhf(c);
        }
        __syncthreads();
    }
    for (int i = tid; i < hid * kSarlGroups; i += kSarlThreads) {
        const int g = i & 15, j = i >> 4, n = 6 + j;
        jbuf[(n >> 2) * 64 + (n & 3) * 16 + g] = hbuf[(j >> 2) * 64 + (j & 3) * 16 + g];
    }
    __syncthreads();
    dense_mfma<1>(net.L[kL_mlp3_0], jbuf, net.ks_a, kbuf, net.ks_a, true, nullptr, wave, lane);
    __syncthreads();
    dense_mfma<1>(net.L[kL_mlp3_2], kbuf, net.ks_a, jbuf, net.ks_a, true, nullptr, wave, lane);
    __syncthreads();
    dense_mfma<1>(net.L[kL_mlp3_4], jbuf, net.ks_a, kbuf, net.ks_a, true, nullptr, wave, lane);
    __syncthreads();
    dense_mfma<1>(net.L[kL_mlp3_6], kbuf, net.ks_a, sbuf, net.ks_s, false, nullptr, wave, lane);
    __syncthreads();
    if (tid < kSarlGroups) {
        const size_t G = tile * kSarlGroups + tid;
        if (G < (size_t)n_groups) V[G] = sbuf[tid];
    }
}

// lstm_rl.ValueNetwork1 / ValueNetwork2 for ANY number of humans (H > kSarlMaxHumans): the LSTM is sequential over the
// humans anyway, so human t's input row tile is staged (and, with the interaction module, passed through mlp1 as 16-row
// products) right before LSTM step t; nothing is sized by H.
__global__ __launch_bounds__(kSarlThreads) void lstm_mlp_anyh_kernel(SarlNet net, const float* X, float* V, int n_groups) {
    extern __shared__ float lds[];
    const int H = net.H;
    const int hid = net.L[kL_mlp1_2].K;
    const int ks_h = sarl_ks(hid), ks_g = net.L[kL_mlp1_0].ctiles * 4;
    CN_LSTM_LDS(float*, lds, net, 1, hid, ks_g, ks_h);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const size_t tile = blockIdx.x;
    zero_lds(lds, (size_t)(end - lds), tid);
    __syncthreads();
    const float* xg = X + tile * H * net.ks_x * 64;
    const bool pairwise = net.L[kL_mlp2_0].w != nullptr;
    for (int t = 0; t < H; ++t) {
        for (int i = tid; i < net.ks_x * 64; i += kSarlThreads) xs[i] = xg[(size_t)t * net.ks_x * 64 + i];
        __syncthreads();
        if (t == 0 && tid < kSarlGroups * 6) {  // self_state = state[:, 0, :6]
            const int g = tid & 15, n = tid >> 4;
            jbuf[(n >> 2) * 64 + (n & 3) * 16 + g] = xs[(n >> 2) * 64 + (n & 3) * 16 + g];
        }
        const float* lstm_in = xs;
        int ks_in = net.ks_x;
        if (pairwise) {
            dense_mfma<1>(net.L[kL_mlp2_0], xs, net.ks_x, pbuf, net.ks_b, true, nullptr, wave, lane);
            __syncthreads();
            dense_mfma<1>(net.L[kL_mlp2_2], pbuf, net.ks_b, qbuf, net.ks_c, true, nullptr, wave, lane);
            __syncthreads();
            dense_mfma<1>(net.L[kL_att_2], qbuf, net.ks_c, pbuf, net.ks_b, true, nullptr, wave, lane);
            __syncthreads();
            dense_mfma<1>(net.L[kL_att_4], pbuf, net.ks_b, qbuf, net.ks_c, false, nullptr, wave, lane);
            __syncthreads();
            lstm_in = qbuf;
            ks_in = net.ks_c;
        }
        dense_mfma<1>(net.L[kL_mlp1_0], lstm_in, ks_in, gates, ks_g, false, nullptr, wave, lane);
        __syncthreads();
        dense_mfma<1>(net.L[kL_mlp1_2], hbuf, ks_h, gates, ks_g, false, gates, wave, lane);
        __syncthreads();
        for (int i = tid; i < hid * kSarlGroups; i += kSarlThreads) {
            const int g = i & 15, j = i >> 4;
            auto at = [&](int n) { return gates[(n >> 2) * 64 + (n & 3) * 16 + g]; };
            const float ig = 1.0f / (1.0f + expf(-at(j)));
            const float fg = 1.0f / (1.0f + expf(-at(hid + j)));
            const float gg = tanhf(at(2 * hid + j));
            const float og = 1.0f / (1.0f + expf(-at(3 * hid + j)));
            const float c = fg * cbuf[i] + ig * gg;
            cbuf[i] = c;
            hbuf[(j >> 2) * 64 + (j & 3) * 16 + g] = og * tanhf(c);
        }
        __syncthreads();
    }
    for (int i = tid; i < hid * kSarlGroups; i += kSarlThreads) {
        const int g = i & 15, j = i >> 4, n = 6 + j;
        jbuf[(n >> 2) * 64 + (n & 3) * 16 + g] = hbuf[(j >> 2) * 64 + (j & 3) * 16 + g];
    }
    __syncthreads();
    dense_mfma<1>(net.L[kL_mlp3_0], jbuf, net.ks_a, kbuf, net.ks_a, true, nullptr, wave, lane);
    __syncthreads();
    dense_mfma<1>(net.L[kL_mlp3_2], kbuf, net.ks_a, jbuf, net.ks_a, true, nullptr, wave, lane);
    __syncthreads();
    dense_mfma<1>(net.L[kL_mlp3_4], jbuf, net.ks_a, kbuf, net.ks_a, true, nullptr, wave, lane);
    __syncthreads();
    dense_mfma<1>(net.L[kL_mlp3_6], kbuf, net.ks_a, sbuf, net.ks_s, false, nullptr, wave, lane);
    __syncthreads();
    if (tid < kSarlGroups) {
        const size_t G = tile * kSarlGroups + tid;
        if (G < (size_t)n_groups) V[G] = sbuf[tid];
    }
}

}  // namespace cn
